"""An LZ4 block synthesizer and the source generator of the dictionary fuzz.

``synth`` writes a block sequence by sequence -- token, literal run, offset,
match length -- and computes the bytes the block stands for itself, with a
byte-by-byte copy out of the virtual history ``hist + plain``.  No encoder
chooses the sequences and no decoder computes the expected output, so a
decoder can be fed what an lz4 encoder never writes: a match that starts in
the dictionary, runs over its end and overlaps itself; such a match at an
output position a 16 KiB history ring no longer holds; twenty dictionary
matches in a row; offsets 1..7 that reach below position 0.

Positions: the block's output starts at 0, the dictionary ``hist`` of H bytes
is [-H, 0).  A match at output position P with offset ``off`` has its source
at ``src = P - off`` and reads positions [src, src + len).

Pure Python on a seeded ``random.Random``; nothing here needs a GPU.
"""
import collections

MINMATCH = 4
LASTLITERALS = 5
MFLIMIT = 12
MAX_OFF = 65535

LIT_CLASSES = (0, 1, 14, 15, 16, 64, 65, 269, 270, 271)
MLEN_CLASSES = (4, 18, 19, 20, 63, 64, 65, 128, 129, 130, 273, 274, 275)
MLEN_BIG = "above4096"
TOT_CLASSES = (63, 64, 65)       # literals + match around one wave step
FAR_MLEN = (128, 129, 130)       # match lengths counted again where the source is far (see _count)
# offsets inside the block; "tot" is the sequence's output length (literals + match)
OFF_CLASSES = ("1..7", "8..63", "64", "tot-1", "tot", "tot+1", "12287..12289", "16255..16257", "16383..16385",
               "16385..65535")
# sources in the dictionary (src < 0); end = src + len, one past the last byte read
#   inside       -H < src and end <= -2
#   first_byte   src == -H                       (only while H + P <= 65535)
#   off_65535    off == 65535, src < 0           (the lowest source there is once H + P >= 65535)
#   end_last     end == 0:  the last byte read is the dictionary's last byte
#   end_before   end == -1: it stops one byte before the dictionary's last byte
#   end_after    end == 1:  the last byte read is position 0
#   over         end >= 2, len <= off:  over the end into the block, no overlap
#   over_lap     end >= 2, len > off:   over the end, and the match reads its own output
#   off1..7      off in 1..7 with src < 0 (P < 7)
DICT_CLASSES = ("inside", "first_byte", "off_65535", "end_last", "end_before", "end_after", "over", "over_lap",
                "off1..7")
LOW_P = 64               # "low": P < 64
HIGH_P = (16384, 65535)  # "high": the bytes at position 0 have left a 16 KiB ring
RUN_MIN = 16             # sequences in a far / dictionary run: more than the decoder's far table per batch


def region(p):
    return "low" if p < LOW_P else "high" if HIGH_P[0] <= p <= HIGH_P[1] else "mid"


def lsic(n):
    """The length bytes after a token nibble of 15."""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


class Writer:
    """One block under construction: ``seq`` per sequence, ``finish`` for the last literals.
    ``matches`` lists every match as (output position, offset, length) for callers that
    classify sources themselves (lz4_frame_synth.py)."""

    def __init__(self, rnd, hist):
        self.rnd = rnd
        self.hist = bytes(hist)
        self.H = len(self.hist)
        self.block = bytearray()
        self.plain = bytearray()
        self.stats = collections.Counter()
        self.last_mlen = MFLIMIT
        self.valid = True
        self.matches = []

    @property
    def op(self):
        return len(self.plain)

    def seq(self, lit, off, mlen):
        """One sequence: ``lit`` literals, then ``mlen`` bytes from ``off`` back."""
        assert mlen >= MINMATCH and 0 < off <= MAX_OFF
        lits = self.rnd.randbytes(lit)
        self.block.append((min(lit, 15) << 4) | min(mlen - MINMATCH, 15))
        if lit >= 15:
            self.block += lsic(lit - 15)
        self.block += lits
        self.plain += lits
        self.block += off.to_bytes(2, "little")
        if mlen - MINMATCH >= 15:
            self.block += lsic(mlen - MINMATCH - 15)
        src = self.op - off
        self.matches.append((self.op, off, mlen))
        hist, H, plain = self.hist, self.H, self.plain
        for s in range(src, src + mlen):      # byte by byte: an overlapping match reads what it wrote
            if s >= 0:
                plain.append(plain[s])
            elif s >= -H:
                plain.append(hist[H + s])
            else:
                plain.append(0)
                self.valid = False
        self.last_mlen = mlen
        self.stats["sequences"] += 1

    def finish(self, lit=None):
        """The last sequence: literals only, at least 5, and the last match at or before n - 12
        (``lit``: exactly that many, for a block of a chosen size)."""
        if lit is None:
            lit = max(LASTLITERALS, MFLIMIT - self.last_mlen) + self.rnd.choice((0, 0, 1, 9, 10, 11, 40, 300))
        assert lit >= max(LASTLITERALS, MFLIMIT - self.last_mlen) or not self.matches
        lits = self.rnd.randbytes(lit)
        self.block.append(min(lit, 15) << 4)
        if lit >= 15:
            self.block += lsic(lit - 15)
        self.block += lits
        self.plain += lits
        return bytes(self.block), bytes(self.plain), self.stats


_Writer = Writer


def _count(w, lit, mlen, off_class=None, dict_class=None, p=None, far=False):
    """``far``: the source is certain to lie outside a 16 KiB history ring (more than 16 384 back, or
    wholly in the dictionary); counted for the match lengths around the 128 bytes a far load carries."""
    w.stats[("lit", lit)] += lit in LIT_CLASSES
    w.stats[("tot", lit + mlen)] += lit + mlen in TOT_CLASSES
    w.stats[("far", mlen)] += far and mlen in FAR_MLEN
    w.stats[("mlen", MLEN_BIG if mlen > 4096 else mlen)] += mlen > 4096 or mlen in MLEN_CLASSES
    if off_class:
        w.stats[("off", off_class)] += 1
    if dict_class:
        for c in dict_class:
            w.stats[("dict", region(p), c)] += 1


def _pick_lit(rnd):
    return rnd.choice(LIT_CLASSES) if rnd.random() < 0.4 else rnd.randrange(0, 30)


def _pick_mlen(rnd, room):
    r = rnd.random()
    if r < 0.4:
        m = rnd.choice(MLEN_CLASSES)
    elif r < 0.43 and room > 6000:
        m = rnd.randrange(4097, 5000)
    else:
        m = rnd.randrange(4, 40)
    return m


def _in_block(w, lit, mlen, cls=None):
    """A sequence whose source lies inside the block (P >= off); False when class ``cls`` does not fit."""
    rnd = w.rnd
    P = w.op + lit
    tot = lit + mlen
    cands = {"1..7": (1, 7), "8..63": (8, 63), "64": (64, 64), "tot-1": (tot - 1, tot - 1), "tot": (tot, tot),
             "tot+1": (tot + 1, tot + 1), "12287..12289": (12287, 12289), "16255..16257": (16255, 16257),
             "16383..16385": (16383, 16385), "16385..65535": (16385, 65535)}
    fit = [c for c, (lo, hi) in cands.items() if 1 <= lo <= min(P, MAX_OFF)]
    if cls is None:
        if not fit:
            return False
        # the rarer the class is reachable, the more often it is taken when it is
        cls = rnd.choice(fit[-3:] if rnd.random() < 0.5 else fit)
    elif cls not in fit:
        return False
    lo, hi = cands[cls]
    hi = min(hi, P, MAX_OFF)
    off = rnd.choice((lo, hi, rnd.randint(lo, hi)))
    _count(w, lit, mlen, off_class=cls, far=off > 16384)
    w.seq(lit, off, mlen)
    return True


def _dict_seq(w, lit, mlen, cls):
    """A sequence of dictionary class ``cls`` at P = op + lit; False when it does not fit there.
    The match length gives way to the class (a source wholly inside 8 bytes is 4..6 long)."""
    rnd, H = w.rnd, w.H
    P = w.op + lit
    lowest = max(-H, P - MAX_OFF)          # the lowest source an offset reaches
    if H == 0 or lowest >= 0:
        return False
    if cls == "inside":
        lo, hi = lowest + (lowest == -H), -MINMATCH - 2
        if lo > hi:
            return False
        src = rnd.randint(lo, hi)
        mlen = min(mlen, -2 - src)
    elif cls in ("first_byte", "off_65535"):
        if (cls == "first_byte") != (lowest == -H) and not (H + P == MAX_OFF):
            return False
        src = lowest
        if -src - 2 < MINMATCH:
            return False
        mlen = min(mlen, -src - 2)
    elif cls in ("end_before", "end_last", "end_after"):
        end = {"end_before": -1, "end_last": 0, "end_after": 1}[cls]
        mlen = min(mlen, end - lowest)
        if mlen < MINMATCH:
            return False
        src = end - mlen
    elif cls == "over":
        # k bytes from the dictionary, at least 2 from the block, len <= off = P + k
        mlen = min(mlen, P + min(-lowest, 40))
        kmin, kmax = max(1, mlen - P), min(-lowest, 40, mlen - 2)
        if mlen < MINMATCH or kmin > kmax:
            return False
        src = -rnd.randint(kmin, kmax)
    elif cls == "over_lap":
        k = rnd.randint(1, min(-lowest, 40))
        mlen = max(mlen, P + k + 1 + rnd.choice((0, 1, 7, 64, 200)), k + 2)
        src = -k
    elif cls == "off1..7":
        if P >= 7:
            return False
        src = P - rnd.randint(P + 1, 7)
    else:
        raise KeyError(cls)
    off = P - src
    assert src < 0 and -H <= src and 0 < off <= MAX_OFF and mlen >= MINMATCH, (cls, P, src, mlen)
    end = src + mlen
    is_a = {"inside": src > -H and end <= -2, "first_byte": src == -H, "off_65535": off == MAX_OFF,
            "end_before": end == -1, "end_last": end == 0, "end_after": end == 1,
            "over": end >= 2 and mlen <= off, "over_lap": end >= 2 and mlen > off, "off1..7": off <= 7}
    assert is_a[cls], (cls, P, src, mlen)
    _count(w, lit, mlen, dict_class=[c for c in DICT_CLASSES if is_a[c]], p=P, far=end <= 0)
    w.seq(lit, off, mlen)
    return True


def mixed_seq(w, room):
    """One sequence of the "mixed" kind: literal run, match length and source class at random."""
    rnd = w.rnd
    lit, mlen = _pick_lit(rnd), _pick_mlen(rnd, room)
    if w.H and rnd.random() < 0.3 and _dict_seq(w, lit, mlen, rnd.choice(DICT_CLASSES[:-2])):
        return
    if not _in_block(w, lit, mlen):
        # nothing to copy from yet: open with literals and a dictionary match, or a run of one byte
        if not (w.H and _dict_seq(w, lit, mlen, "end_last")):
            lit = max(lit, 1)
            _count(w, lit, mlen, off_class="1..7")
            w.seq(lit, 1, mlen)


def grow(w, upto):
    """Cheap bulk up to output position ``upto``: long matches close behind."""
    while w.op < upto:
        lit = w.rnd.randrange(20, 300)
        w.seq(lit, w.rnd.randrange(1, lit + 1), min(upto - w.op, w.rnd.randrange(1500, 4000)) + MINMATCH)


_mixed_seq, _grow = mixed_seq, grow      # the names older callers use


def _run_far(w):
    """RUN_MIN or more short sequences in a row whose sources all lie 16 400 or more back."""
    rnd = w.rnd
    n = rnd.randrange(RUN_MIN, RUN_MIN + 9)
    for _ in range(n):
        lit = rnd.randrange(0, 4)
        P = w.op + lit
        w.seq(lit, rnd.randint(16400, min(P, MAX_OFF)), rnd.randrange(4, 13))
    w.stats[("run", "far")] += 1


def _run_dict(w):
    """RUN_MIN or more short sequences in a row whose sources all lie wholly in the dictionary."""
    rnd = w.rnd
    n = rnd.randrange(RUN_MIN, RUN_MIN + 9)
    if w.H == 0 or w.op + n * 16 - MAX_OFF >= -MINMATCH - 2:
        return
    for _ in range(n):
        assert _dict_seq(w, rnd.randrange(0, 4), rnd.randrange(4, 13), "inside")
    w.stats[("run", "dict", region(w.op))] += 1


def _run_cross(w):
    """Fewer than 64 plain sequences (one length byte at most) whose output sums to more than 4096."""
    rnd = w.rnd
    start, k = w.op, 0
    while w.op - start <= 4096 + 300:
        lit, mlen = rnd.randrange(0, 15), rnd.randrange(100, 270)
        P = w.op + lit
        w.seq(lit, rnd.randint(min(P, lit + mlen), min(P, 3000)), mlen)
        k += 1
    assert k < 64
    w.stats[("run", "cross4096")] += 1


def synth(rnd, hist, n_target, profile="mixed", writer=None):
    """(block, plain, stats): an LZ4 block of about ``n_target`` decoded bytes against dictionary ``hist``.

    ``profile`` is a kind or a dict {"kind": ..., "low": c, "high": c}:
      "mixed"    every sequence draws its literal run, match length and source class at random
      "runs"     long runs of one kind: far sources, dictionary sources, and plain sequences whose
                 output crosses 4096 bytes within 64 sequences
      "invalid"  "mixed" with one offset that reaches exactly one byte below the dictionary's start
                 (below position 0 without a dictionary); ``plain`` is then None
    "low" / "high" ask for one dictionary class at P < 64 (the block's first sequence) and at the
    first P in [16384, 60000]; stats[("forced", ...)] says whether it fitted.  Valid blocks keep
    lz4's end-of-block rules, so the expected output of a valid block is ``plain`` for any decoder.
    ``writer``: a list that receives the Writer (its ``matches``) of the block.
    """
    p = {"kind": profile} if isinstance(profile, str) else dict(profile)
    kind, low, high = p.get("kind", "mixed"), p.get("low"), p.get("high")
    w = Writer(rnd, hist)
    if writer is not None:
        writer.append(w)
    bad_at = rnd.randrange(0, max(n_target - 40, 1)) if kind == "invalid" else None
    if low:
        # "first_byte" of a 65 535-byte dictionary is reachable from P = 0 only
        lit = rnd.randrange(0, 7) if low == "off1..7" else rnd.randrange(2, 40) if low == "over" else \
            rnd.randrange(0, max(min(60, MAX_OFF - w.H + 1), 1)) if low == "first_byte" else rnd.randrange(0, 60)
        w.stats[("forced", "low", low)] += _dict_seq(w, lit, _pick_mlen(rnd, 0), low) and region(lit) == "low"
    while w.op < n_target or bad_at is not None:
        room = n_target - w.op
        if bad_at is not None and w.op >= bad_at:
            lit = rnd.randrange(0, 20)
            off = w.op + lit + w.H + 1
            assert off <= MAX_OFF, "the invalid offset does not fit"
            w.seq(lit, off, rnd.choice((4, 8, 18, 19, 40, 300)))
            w.stats["invalid"] += 1
            bad_at = None
            continue
        if high and w.op >= HIGH_P[0]:
            lit = rnd.randrange(0, 20)
            at = region(w.op + lit)
            w.stats[("forced", "high", high)] += _dict_seq(w, lit, _pick_mlen(rnd, room), high) and at == "high"
            high = None
            continue
        if kind == "runs":
            c = rnd.randrange(4)
            if c == 0 and (w.op >= 16400 or room > 17000):
                grow(w, max(w.op, 16400 + rnd.randrange(0, 3000)))
                _run_far(w)
            elif c == 1:
                _run_dict(w)
            elif c == 2:
                if w.op < 100:
                    grow(w, 100)
                _run_cross(w)
            else:
                for _ in range(rnd.randrange(1, 12)):
                    mixed_seq(w, room)
        else:
            mixed_seq(w, room)
    block, plain, stats = w.finish()
    if kind == "invalid":
        assert stats["invalid"] == 1 and not w.valid
        return block, None, stats
    assert w.valid
    return block, plain, stats


# ---------------------------------------------------------------------------
# sources for the dictionary encoders (the differential fuzz, CPU and GPU)
# ---------------------------------------------------------------------------
def _copy(e, out, start, n):
    """Append n bytes of the virtual history ``e + out`` from ``start``, as an LZ77 copy does
    (a slice that reaches what it appends repeats)."""
    if start < len(e):
        take = e[start:start + n]
        out += take
        n -= len(take)
        start += len(take)
    if n > 0:
        s = start - len(e)
        seg = bytes(out[s:s + n])
        out += (seg * (n // len(seg) + 1))[:n]


def fuzz_source(rnd, d, n, text=b""):
    """``n`` bytes for a chunk compressed against dictionary ``d``: random slices of ``d + the
    source so far`` -- starting in the dictionary and crossing its end, on its first byte, on the
    last position LZ4_loadDict inserts, more than 65 535 back, periods 1..40 -- between random
    bytes, zero runs and pieces of ``text``."""
    e = b"" if len(d) < 8 else bytes(d[-65536:])
    out = bytearray()
    while len(out) < n:
        k = rnd.randrange(12)
        virt = len(e) + len(out)
        if k == 0 and e:                                   # from the dictionary over its end
            back = rnd.randrange(1, min(len(e), 300) + 1)
            _copy(e, out, len(e) - back, back + rnd.randrange(1, 300))
        elif k == 1 and e:                                 # the dictionary's first byte
            _copy(e, out, 0, rnd.randrange(4, 300))
        elif k == 2 and e:                                 # the last position loadDict inserts
            _copy(e, out, 3 * ((len(e) - 8) // 3), rnd.randrange(8, 40))
        elif k == 3 and virt > 65540:                      # too far back for an offset
            _copy(e, out, rnd.randrange(0, virt - 65536), rnd.randrange(4, 200))
        elif k == 4:                                       # periods 1..40
            seg = rnd.randbytes(rnd.randrange(1, 41))
            out += (seg * 40)[:rnd.randrange(4, 400)]
        elif k == 5:
            out += rnd.randbytes(rnd.randrange(1, 300))
        elif k == 6:
            out += bytes(rnd.randrange(1, 500))
        elif k == 7 and text:
            a = rnd.randrange(len(text) - 2000)
            out += text[a:a + rnd.randrange(20, 2000)]
        elif virt > 8:                                     # anywhere in the dictionary or the source so far
            _copy(e, out, rnd.randrange(0, virt - 4), rnd.randrange(4, 600))
    return bytes(out[:n])


def hand_tail_source(d, seed_bytes):
    """20 000 random bytes, then the dictionary's last 40 bytes followed by the chunk's own first 200."""
    assert len(seed_bytes) == 20000
    return seed_bytes + bytes(d[-40:]) + seed_bytes[:200]


def damaged(rnd, blk):
    """Byte flips, bit flips, truncations and appended bytes of one block."""
    out = []
    for _ in range(4):
        m = bytearray(blk)
        for _ in range(rnd.randrange(1, 4)):
            m[rnd.randrange(len(m))] ^= 1 << rnd.randrange(8)
        out.append(bytes(m))
    m = bytearray(blk)
    m[rnd.randrange(len(m))] = rnd.randrange(256)
    out.append(bytes(m))
    out.append(blk[:rnd.randrange(1, len(blk))] if len(blk) > 1 else blk)
    out.append(blk[:-1])
    out.append(blk + rnd.randbytes(rnd.randrange(1, 20)))
    return out
