"""Lane-level Python model of the v5 encoder window loop (encode_block_v5 in
lz4mt_kernels.hip) for debugging on the CPU: runs the same window algorithm
with 64 explicit lanes and compares against the oracle.

usage: python tools/enc_model.py            (fuzz cases of tests/test_gpu.py)
"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402

POSB = 22
MASK = (1 << POSB) - 1


def rd32(s, i):
    return int.from_bytes(s[i:i + 4].ljust(4, b"\0"), "little")


def rd64(s, i):
    return int.from_bytes(s[i:i + 8].ljust(8, b"\0"), "little")


def h5(v8):
    return (((v8 << 24) & 0xFFFFFFFFFFFFFFFF) * 889523592379 & 0xFFFFFFFFFFFFFFFF) >> 52


def tag(w0):
    return ((w0 * 0x85EBCA77) & 0xFFFFFFFF) >> POSB


def poff(k):
    if k == 0:
        return 0
    q, r = (k - 1) >> 6, (k - 1) & 63
    return 1 + 32 * q * (q + 1) + r * (q + 1)


def ext_len(v):
    return (v - 15) // 255 + 1 if v >= 15 else 0


def encode(s, cap, last_lane_wins=True, xchg=False):
    """xchg=True: the exchange probe of encode_block_v5 (LZ4MT_ENC_XCHG):
    lanes exchange their entries in ascending lane order, so each gets its
    in-window predecessor's entry or the table's; no read-back, no
    predecessor resolution; lanes past the stop undo their inserts (the
    first of each bucket puts back what it displaced)."""
    if xchg:
        return encode_xchg(s, cap)
    n = len(s)
    assert 65547 <= n <= 1 << 22
    bound = n + n // 255 + 16
    limited = cap < bound
    T = [(tag(rd32(s, 0)) << POSB)] * 4096 + [0] * 64
    mfl = n - 12 + 1
    matchlimit = n - 5
    anchor = op = 0
    out = bytearray()
    insOn, testOn = True, False
    insPos = testPos = 0
    sPos, k0 = 1, 0
    while True:
        p, step = [0] * 64, [1] * 64
        for L in range(64):
            k = k0 + L - 2
            if L >= 2:
                p[L] = sPos + poff(k)
                step[L] = 1 if k == 0 else (63 + k) >> 6
        p[0], p[1] = insPos, testPos
        live = [(p[L] <= mfl) if L >= 2 else (insOn if L == 0 else testOn) for L in range(64)]
        term = [L >= 2 and live[L] and p[L] + step[L] > mfl for L in range(64)]
        w0 = [rd32(s, min(p[L], n - 8)) for L in range(64)]
        h = [h5(rd64(s, min(p[L], n - 8))) for L in range(64)]
        mark = [(p[L] | (tag(w0[L]) << POSB)) & 0xFFFFFFFF for L in range(64)]
        ti = [h[L] if live[L] else 4096 + L for L in range(64)]
        told = [T[ti[L]] for L in range(64)]
        order = range(64) if last_lane_wins else range(63, -1, -1)
        for L in order:
            T[ti[L]] = mark[L]
        sv = [T[ti[L]] for L in range(64)]
        pend = [sv[L] != mark[L] for L in range(64)]
        cand = [told[L] & MASK for L in range(64)]
        cok = [live[L] and L != 0 and not term[L] and cand[L] + 65535 >= p[L] for L in range(64)]
        maybe = [cok[L] and (told[L] >> POSB) == (mark[L] >> POSB) for L in range(64)]
        sm = [maybe[L] or term[L] for L in range(64)]
        mm = list(maybe)
        dd = False
        gmask = [{L} for L in range(64)]
        aliased = set()
        while True:
            w = next((L for L in range(64) if sm[L]), 64)
            collide = any(pend[L] for L in range(min(w, 63) + 1))
            if not dd and collide:
                dd = True
                pred = [-1] * 64
                for L in range(64):
                    if live[L]:
                        grp = [j for j in range(64) if live[j] and h[j] == h[L]]
                        gmask[L] = set(grp)
                        below = [j for j in grp if j < L]
                        pred[L] = below[-1] if below else -1
                ok = [False] * 64
                for L in range(64):
                    if pred[L] >= 0:
                        pp, pw = p[pred[L]], w0[pred[L]]
                        ok[L] = live[L] and L != 0 and not term[L] and pp + 65535 >= p[L] and pw == w0[L]
                        maybe[L] = False
                        cand[L] = pp
                mm = list(maybe)
                sm = [(ok[L] or maybe[L] or term[L]) and L not in aliased for L in range(64)]
                continue
            wTerm = w < 64 and term[w]
            if w == 64 or wTerm:
                break
            ip, cd = p[w], cand[w]
            if mm[w] and rd32(s, cd) != w0[w]:
                sm[w] = False
                aliased.add(w)
                continue
            break
        wlim = 63 if w == 64 else (w - 1 if wTerm else w)
        for L in range(64):
            if live[L] and L > wlim:
                T[h[L]] = told[L]
        if any(pend):
            for L in order:
                le = L <= wlim
                lastM = (not dd) or not any(j > L and j <= wlim for j in gmask[L])
                if live[L] and le and lastM:
                    T[h[L]] = mark[L]
        if w == 64:
            k0 += 62
            insOn = testOn = False
            continue
        if wTerm:
            break
        maxb = 0 if w == 1 else min(ip - anchor, cd)
        back = 0
        while back < maxb and s[ip - back - 1] == s[cd - back - 1]:
            back += 1
        lim = matchlimit - (ip + 4)
        mc = 0
        while mc < lim and s[ip + 4 + mc] == s[cd + 4 + mc]:
            mc += 1
        lit = ip - anchor - back
        mcf = mc + back
        litExt, mlExt = ext_len(lit), ext_len(mcf)
        if limited:
            if w != 1 and op + 1 + lit + 8 + lit // 255 > cap:
                return b""
            if op + 1 + litExt + lit + 2 + 6 + (mcf + 240) // 255 > cap:
                return b""
        tok = (min(lit, 15) << 4) | min(mcf, 15)
        seq = bytearray([tok])
        if lit >= 15:
            seq += b"\xff" * (litExt - 1) + bytes([(lit - 15) % 255])
        seq += s[anchor:anchor + lit]
        off = ip - cd
        seq += bytes([off & 255, off >> 8])
        if mcf >= 15:
            seq += b"\xff" * (mlExt - 1) + bytes([(mcf - 15) % 255])
        out += seq
        op += len(seq)
        ipe = ip + 4 + mc
        anchor = ipe
        if ipe >= mfl:
            break
        insOn = testOn = True
        insPos, testPos, sPos, k0 = ipe - 2, ipe, ipe + 1, 0
    run = n - anchor
    if limited and op + run + 1 + (run + 240) // 255 > cap:
        return b""
    out.append(min(run, 15) << 4)
    if run >= 15:
        out += b"\xff" * (ext_len(run) - 1) + bytes([(run - 15) % 255])
    out += s[anchor:]
    return bytes(out)


def tag_ht(w0):
    """the hash-product tag (LZ4MT_ENC_HTAG): bits 42..51 of hash5's product"""
    return ((((w0 << 24) * 889523592379) & 0xFFFFFFFFFFFFFFFF) >> (52 - (32 - POSB))) & ((1 << (32 - POSB)) - 1)


FAST_SPAN_MAX = 1016   # the span kFastEndGap was sized for; encode_block_v5: kFastEndGap, kFastOutSlack, kCountLanes
FAST_END_GAP = 1280
FAST_OUT_SLACK = 64
COUNT_LANES = 32
CATCH_WORDS = 16      # kCatchWords: the lanes behind the count lanes load the 64 bytes below cd / ip as words
FAST_BEG = 65536 + 4 * CATCH_WORDS   # kFastBeg
RING = 2048           # kSR


def back_from_words(s, ip, cd, maxb):
    """the fast body's catch-up from words in the idle lanes: backward lane i
    holds the words at cd - 4(i+1) and ip - 4(i+1); its equal bytes, counted
    from the word's high end, are clz(x) >> 3 (4 when x = 0); the first lane
    with fewer than 4 ends the catch-up unless the bound does so first"""
    for i in range(CATCH_WORDS):
        x = rd32(s, cd - 4 * (i + 1)) ^ rd32(s, ip - 4 * (i + 1))
        if x:
            return min(4 * i + ((32 - x.bit_length()) >> 3), maxb)
    return maxb


def encode_xchg(s, cap, phases=None, catch_words=False):
    """phases (a dict, optional): also runs encode_block_v5's phase rules
    (general -> fast -> general) beside the parse and asserts, at every
    window of the fast phase, that what the kernel's fast body drops has the
    value it assumes: every SEARCH lane live, none terminating, no clamp of
    hi, of the round trip's addresses or of the first count round binding,
    no wide window, neither margin test firing.  Counts the windows and
    phase entries into it.
    A fast window is a first window after a match (first windows only):
    the kernel's fast body folds the window state k0 = 0, s0 = 1, j1 = 65,
    mode = 1, spanHi = 61 into constants, and a window without a stop leaves
    the phase with the continuation state written as constants.  The model
    carries the kernel's window state (sBase, k0, s0, j1, spanHi) beside its
    own and asserts at every fast window that the folded values -- lane
    positions sBase + c(L), roleM = 3, every lane live, lo = sBase - 3,
    hi = sBase + 69, step 1, and the continuation state at a no-stop exit --
    equal the general formulas.  Also counted: fast_stop_lanes[L] (stops per
    lane in fast windows), cont1_stop_lanes[L] (stops per lane in the first
    continuation window after a fast exit), fast_exits_redo (fast windows
    left without a stop after a tag alias, the exit that redoes the table
    writes).
    catch_words=True: the rules of the catch-up from words and of the
    one-sided ring test as well (the kernel's fast body; without it, the fast
    body of first windows with the byte-wise catch-up).
    The phase is entered only after a match that ends at or above FAST_BEG,
    and at every stop of a fast window the model asserts what the fast body
    folds: the catch-up bound min(ip - anchor, cd) is w - 1, at most 62, the
    candidate lies 64 bytes or more into the block, and the catch-up read
    from the 16 backward words equals the byte loop's.  The model carries the
    source ring's base (SrcRing::cover) and asserts at every pending store of
    a fast window that the literals end inside the ring, so that the store's
    in-ring test is its lower bound alone.  Counted: catch_full[back] (stops
    of fast windows whose catch-up ate the whole literal run, back = w - 1),
    catch_part[back] (back < w - 1), fast_store_total[min(total, 130)] and
    fast_store_left_ring (pending stores of fast windows by sequence length,
    and those whose literals had left the ring)."""
    n = len(s)
    fast = False
    fast_beg = FAST_BEG if catch_words else 0
    ring_b = 0     # SrcRing::B
    pend = None    # the pending sequence: (anchor, lit, total)
    fast_end_v = n - FAST_END_GAP if n > FAST_END_GAP else 0
    assert 65547 <= n <= 1 << 22
    bound = n + n // 255 + 16
    limited = cap < bound
    fast_end_s = 0 if limited else fast_end_v   # 0: output safety (b) not established yet
    if phases is not None:
        phases.update(fast_windows=0, general_windows=0, entries=0, wide_general=0,
                      fast_stop_lanes=[0] * 64, cont1_stop_lanes=[0] * 64, fast_exits_redo=0,
                      catch_full=[0] * 64, catch_part=[0] * 64, fast_store_total=[0] * 131, fast_store_left_ring=0)
    j1, span_hi = 65, 61   # the kernel's window state beside sPos + poff(k0), k0 and s0 = step(k0)
    after_fast_exit = False   # this window is the first continuation window after a fast exit
    T = [(tag_ht(rd32(s, 0)) << POSB)] * 4096 + [0] * 64
    mfl = n - 12 + 1
    matchlimit = n - 5
    anchor = op = 0
    out = bytearray()
    mode = 2            # 2: INSERT 0 only; 1: INSERT + TEST after a match; 0: continuation
    sPos, k0 = 1, 0
    while True:
        p, step = [0] * 64, [1] * 64
        for L in range(2, 64):
            k = k0 + L - 2
            p[L] = sPos + poff(k)
            step[L] = 1 if k == 0 else (63 + k) >> 6
        p[0] = 0 if mode == 2 else sPos - 3
        p[1] = sPos - 1
        live = [p[L] <= mfl if L >= 2 else (mode != 0 if L == 0 else mode == 1) for L in range(64)]
        term = [L >= 2 and live[L] and p[L] + step[L] > mfl for L in range(64)]
        if phases is not None:
            lo = p[0] if mode != 0 else p[2]
            # the kernel's general formulas on its own window state
            sBase, s0 = sPos + poff(k0), max(1, (63 + k0) >> 6)
            assert span_hi == p[63] - p[2], (sPos, k0)
            for L in range(2, 64):
                assert p[L] == sBase + (L - 2) * s0 + max(0, L - 2 - j1), (sPos, k0, L)
                assert step[L] == s0 + (L - 2 >= j1), (sPos, k0, L)
            if fast:
                phases["fast_windows"] += 1
                # the folded values of the first window equal the general ones
                assert (mode, k0, s0, j1, span_hi) == (1, 0, 1, 65, 61), (sPos, mode, k0)
                assert p == [sBase + (-3 if L == 0 else -1 if L == 1 else L - 2) for L in range(64)], sPos
                assert (0x130 >> (4 * mode)) & 3 == 3 and all(live), sPos   # roleM, liveM
                assert step == [1] * 64, sPos
                assert lo == sBase - 3 and min(sBase + span_hi, mfl) + 8 == sBase + 69, sPos
                assert all(live[2:]) and not any(term), (sPos, k0)
                assert p[63] < mfl and p[63] + 8 - lo <= 1024, (sPos, k0)
                assert p[2] <= fast_end_s and p[63] - p[2] <= FAST_SPAN_MAX, (sPos, k0)
            else:
                phases["general_windows"] += 1
                phases["wide_general"] += min(p[63], mfl) + 8 - lo > 1024
        # the ring's advance at the window's head (not in a wide window), then
        # the pending sequence's store (the kernel: in the round trip's
        # shadow, or behind a window without a stop; once per sequence)
        lo_w = p[0] if mode != 0 else p[2]
        hi_w = min(p[63], mfl) + 8
        if hi_w - lo_w <= 1024 and hi_w > ring_b + RING:
            ring_b = (hi_w - RING + 511) & ~511
        if pend is not None:
            pa, pl, pt = pend
            if fast and catch_words:
                assert pa + pl <= ring_b + RING, (sPos, pa, pl, ring_b)   # the in-ring test's upper bound
                if phases is not None:
                    phases["fast_store_total"][min(pt, 130)] += 1
                    phases["fast_store_left_ring"] += pa < ring_b
            pend = None
        w0 = [rd32(s, min(p[L], n - 8)) for L in range(64)]
        h = [h5(rd64(s, min(p[L], n - 8))) for L in range(64)]
        mark = [(p[L] | (tag_ht(w0[L]) << POSB)) & 0xFFFFFFFF for L in range(64)]
        told = [0] * 64
        for L in range(64):   # the exchanges, in ascending lane order
            i = h[L] if live[L] else 4096 + L
            told[L] = T[i]
            T[i] = mark[L]
        cand = [told[L] & MASK for L in range(64)]
        maybe = [live[L] and L != 0 and not term[L] and cand[L] + 65535 >= p[L] and
                 (told[L] >> POSB) == (mark[L] >> POSB) for L in range(64)]
        aliased = set()
        redo = False

        def table_writes(wlim):
            if redo:   # re-insert the lanes up to the stop, in lane order
                for L in range(64):
                    if live[L] and L <= wlim:
                        T[h[L]] = mark[L]
            past = [L for L in range(64) if live[L] and L > wlim]
            # the first lane of each bucket past the stop restores: lanes are in
            # position order, so "displaced by no lane past the stop" is "the
            # displaced entry's position is at most lane wlim's" (the kernel's
            # table_writes; no mask scan for the first lane past the stop)
            pB = p[wlim] if wlim >= 0 else -1
            for L in past:
                if (told[L] & MASK) <= pB:
                    T[h[L]] = told[L]

        while True:
            w = next((L for L in range(64) if (maybe[L] or term[L]) and L not in aliased), 64)
            wTerm = w < 64 and term[w]
            if w < 64 and not wTerm and rd32(s, cand[w]) != w0[w]:
                aliased.add(w)     # tag alias: the stop moves on
                table_writes(w)    # (the kernel writes in the round trip's shadow, then redoes)
                redo = True
                continue
            break
        wlim = 63 if w == 64 else (w - 1 if wTerm else w)
        table_writes(wlim)
        if phases is not None and w < 64 and not wTerm:
            if fast:
                phases["fast_stop_lanes"][w] += 1
            elif after_fast_exit:
                phases["cont1_stop_lanes"][w] += 1
        after_fast_exit = False
        if w == 64:   # (probe offsets poff(k) count from the sequence's first search position)
            # the kernel's foot: the next window's state from this one's
            nb = sPos + poff(k0) + 62 * max(1, (63 + k0) >> 6) + max(0, 62 - j1)
            k0 += 62
            mode = 0
            s0 = (63 + k0) >> 6
            j1 = (65 if k0 < 65 else ((k0 - 1) & ~63) + 65) - k0
            span_hi = 61 * s0 + max(0, 61 - j1)
            assert nb == sPos + poff(k0), (sPos, k0)
            if fast:   # a fast window without a stop leaves the phase: the state it writes as constants
                assert (nb, k0, s0, j1, mode, span_hi) == (sPos + 62, 62, 1, 3, 0, 119), (sPos, k0)
                if phases is not None:
                    phases["fast_exits_redo"] += redo
                fast = False
                after_fast_exit = True
            continue
        if wTerm:
            break
        ip, cd = p[w], cand[w]
        if fast:   # the round trip's loads and the first count round need no clamp
            assert ip + 4 * COUNT_LANES < n - 4 and matchlimit - (ip + 4) >= 4 * COUNT_LANES, ip
        maxb = 0 if w == 1 else min(ip - anchor, cd)
        back = 0
        while back < maxb and s[ip - back - 1] == s[cd - back - 1]:
            back += 1
        if fast and catch_words:   # what the fast body folds (catch-up from words)
            assert ip >= FAST_BEG and cd >= 4 * CATCH_WORDS, (ip, cd)
            assert maxb == w - 1 <= 62 and back <= 62, (ip, w, maxb)
            assert back == back_from_words(s, ip, cd, w - 1), (ip, cd, w, back)
            if phases is not None:
                phases["catch_full" if back == w - 1 else "catch_part"][back] += 1
        lim = matchlimit - (ip + 4)
        mc = 0
        while mc < lim and s[ip + 4 + mc] == s[cd + 4 + mc]:
            mc += 1
        lit = ip - anchor - back
        mcf = mc + back
        litExt, mlExt = ext_len(lit), ext_len(mcf)
        if limited:
            fails = (w != 1 and op + 1 + lit + 8 + lit // 255 > cap) or \
                op + 1 + litExt + lit + 2 + 6 + (mcf + 240) // 255 > cap
            assert not (fast and fails), (ip, op)   # the fast body has no margin test
            if fails:
                return b""
        tok = (min(lit, 15) << 4) | min(mcf, 15)
        seq = bytearray([tok])
        if lit >= 15:
            seq += b"\xff" * (litExt - 1) + bytes([(lit - 15) % 255])
        seq += s[anchor:anchor + lit]
        off = ip - cd
        seq += bytes([off & 255, off >> 8])
        if mcf >= 15:
            seq += b"\xff" * (mlExt - 1) + bytes([(mcf - 15) % 255])
        out += seq
        op += len(seq)
        pend = (anchor, lit, len(seq))
        ipe = ip + 4 + mc
        anchor = ipe
        if fast:
            fast = ipe < fast_end_s
        else:
            if fast_end_s == 0 and op + (n - ipe) + (n - ipe) // 255 + FAST_OUT_SLACK <= cap:
                fast_end_s = fast_end_v
            fast = fast_beg <= ipe < fast_end_s
            if fast and phases is not None:
                phases["entries"] += 1
        if ipe >= mfl:
            break
        mode = 1
        sPos, k0 = ipe + 1, 0
        j1, span_hi = 65, 61
    run = n - anchor
    if limited and op + run + 1 + (run + 240) // 255 > cap:
        assert fast_end_s == 0, (anchor, op)   # (b) covers the last literals too
        return b""
    out.append(min(run, 15) << 4)
    if run >= 15:
        out += b"\xff" * (ext_len(run) - 1) + bytes([(run - 15) % 255])
    out += s[anchor:]
    return bytes(out)


def literal_run_sweep(n, seed):
    """Inputs for the first-window fast phase: units of r fresh random bytes
    followed by a copy of 8..40 earlier bytes from within 60 KB, r cycling
    through 0..199.  After the match that ends a unit the next search stops
    r positions on: at every SEARCH lane of the first window, on the TEST
    lane (r = 0, back-to-back matches) and, past 62 literals, at the lanes of
    the first and second continuation windows (the step rises inside the
    first one, at j1 = 3)."""
    rnd = random.Random(seed)
    out = bytearray(oracle.gen_random(4096, seed))
    r = 0
    while len(out) < n:
        out += oracle.gen_random(r, rnd.randrange(1 << 30)) if r else b""
        k = rnd.randrange(8, 41)
        a = rnd.randrange(max(0, len(out) - 60_000), len(out) - k)
        out += out[a:a + k]
        r = (r + 1) % 200
    return bytes(out[:n])


CATCH_SLOT = 34_000   # two slots are out of a candidate's range, one is inside it


def catch_up_cases():
    """(b, f) of the catch-up units: b bytes of catch-up behind f fresh
    bytes.  f = 0: the catch-up eats the literal run whole (back = w - 1,
    b = 0 is a stop on the TEST lane); f > 0: it ends on a differing byte
    (back < w - 1).  The stop's lane is w = f + b + 1 <= 63."""
    full = [(b, 0) for b in range(62)]
    part = [(b, 1 + (7 * b) % (62 - b)) for b in range(62)] + [(0, 62), (3, 1), (4, 1), (5, 1), (7, 50)]
    return full + part


def catch_up_units(n, seed, units):
    """A block of zero runs (long single matches, few table inserts) holding,
    per unit (b, f), three occurrences one slot apart: U0 = a 66-byte body;
    U1 = the body and 8 bytes t1 behind it, a match of U0 that ends at the
    body's end E (positions inside a match are never inserted, E - 2 is, by
    the next window's INSERT lane); P = f fresh bytes, the body's last b + 2
    bytes and t1.  At P the body's inner positions find U0, two slots back and
    out of range, or nothing; position E - 2's entry is found and the match
    catches up b bytes, to a differing fresh byte or to the previous match's
    end.  Whether a unit's table entries survive the inserts in between is
    left to the seed: callers assert the coverage they need.  Behind the
    slots: literal runs of 58 .. 61, 125 and 200 bytes before a short match
    (sequences of 62 .. 65, 129 and 204 bytes), each behind a zero run
    longer than the source ring."""
    rnd = random.Random(seed)

    def nz(k):
        return bytes(rnd.randrange(1, 256) for _ in range(k))

    buf = bytearray(n)
    groups = n // CATCH_SLOT - 2
    per = -(-len(units) // groups)
    stride = CATCH_SLOT // per
    assert groups >= 1 and stride >= 720, (groups, per, stride)
    for i, (b, f) in enumerate(units):
        g, j = divmod(i, per)
        body, t1 = nz(66), nz(8)
        fresh = nz(f)
        while f and fresh[-1] == body[-(b + 3)]:
            fresh = nz(f)
        at = g * CATCH_SLOT + j * stride
        buf[at + 100:at + 166] = body
        at += CATCH_SLOT
        buf[at + 266:at + 340] = body + t1
        at += CATCH_SLOT
        probe = fresh + body[-(b + 2):] + t1
        buf[at + 440:at + 440 + len(probe)] = probe
    at = (groups + 2) * CATCH_SLOT
    for lit in (58, 59, 60, 61, 125, 200, 59, 60, 61, 125):
        at += 2400
        run = nz(lit)
        tail = run[:8] + bytes([run[8] ^ 0x55 or 1])
        assert at + lit + 9 + 1500 < n, n
        buf[at:at + lit + 9] = run + tail
        at += lit + 9
    return bytes(buf)


def long_search_input(n, run, seed):
    """a compressible prefix, `run` random bytes (one search that leaves the
    fast phase and ends in the general one), a compressible suffix"""
    syn = oracle.gen_synthetic(n, seed)
    prefix = min(40_000, n // 4)
    return (syn[:prefix] + oracle.gen_random(run, seed + 1) + syn[prefix:])[:n]


def fuzz_cases():
    rnd = random.Random(3)
    syn = oracle.gen_synthetic(1 << 20)
    for t in range(80):
        n = rnd.choice([1, 7, 12, 13, 14, 20, 64, 100, 1000, 4095, 65535, 65546, 65547, 65548, 100_000, 262_144])
        kind = t % 5
        if kind == 0:
            d = syn[:n]
        elif kind == 1:
            d = bytes(rnd.randrange(3) for _ in range(n))
        elif kind == 2:
            d = oracle.gen_random(n, t)
        elif kind == 3:
            d = (bytes(rnd.randrange(256) for _ in range(rnd.randrange(1, 70))) * (n + 1))[:n]
        else:
            d = bytes(n)
        yield t, d


if __name__ == "__main__":
    for t, d in fuzz_cases():
        if len(d) < 65547:
            continue
        for cap in (len(d), len(d) + len(d) // 255 + 16):
            for llw in (True, False, "xchg"):
                got = encode(d, cap, xchg=True) if llw == "xchg" else encode(d, cap, llw)
                want = oracle.compress_block(d, cap)
                if got != want:
                    i = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
                    print(f"MISMATCH t={t} n={len(d)} cap={cap} lastLaneWins={llw} first diff at {i}")
                else:
                    print(f"ok t={t} n={len(d)} cap={cap} llw={llw}")
