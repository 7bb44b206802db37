// The window loop of encode_block_v5 (lz4mt_kernels.hip), included there once
// per phase with V5_FAST defined: false the general body, true the fast body
// (see the two phases at the include site).  Textual inclusion, not a
// lambda or a helper template: the instantiations without a fast phase
// then compile to the code they had as one loop, and the loop-carried state
// stays in the enclosing function's registers.
// FAST: every window of the phase is the first window after a match, so
// k0 = 0, s0 = 1, j1 = 65, mode = 1 and spanHi = 61 are constants here and
// not loop state (sBase is the only window state the fast body carries); the
// catch-up bytes come as words in the round trip's idle count lanes, bounded
// by w - 1; there is no margin test and no wide window; the pending store
// tests the ring's lower bound only; a window without a stop leaves the
// phase, and the continuation state is written once, behind the loop.
{
    constexpr bool FAST = V5_FAST;
    bool sw = false;   // leave this phase
    bool fcont = false;   // FAST: the phase was left by a window without a stop
    // ONE exit and no continue: the structurizer then needs no flow
    // variables and the loop-carried state stays in place across windows
    while (!done && !sw) {
      // general body: windows without a stop (continuations) loop here,
      // inside: the match-path state (anchor, op, pe) is not touched by them
      uint32_t w, ip, cd, maxb, cw, iw, bi, bc;
      bool wTerm;
      do {
        if (ST) acc[10] += 1;
        if (P17) {
            while (sBase >= nextSweep) {   // (long matches cross several)
                tab.sweep(nextSweep);
                nextSweep += 32768;
            }
        }
        // ---- probe positions.  SEARCH lane L probes k = k0 + j (j = L - 2) at
        // sBase + j*s0 + max(0, j - j1): the step s0 = step(k0) rises by one at
        // most once inside a window (at j = j1; never in the k0 = 0 window)
        const uint32_t j = L - 2;
        const int32_t jx = (int32_t)j - (int32_t)j1;
        // j < 62 and the step s0 < 2^24: a full-rate 24-bit multiply (lanes 0
        // and 1 wrap j, but take the INSERT / TEST position below)
        uint32_t p = sBase + __umul24(j, s0) + (uint32_t)max(jx, 0);
        const uint32_t step = FAST ? 1u : s0 + (jx >= 0 ? 1u : 0u);
        const uint32_t sHi = sBase + (FAST ? 61u : spanHi);
        const bool insOn = FAST ? true : mode != 0;
        const uint32_t insPos = !FAST && mode == 2 ? o0 : sBase - 3, testPos = sBase - 1;
        p = L == 0 ? insPos : (L == 1 ? testPos : p);
        // (FAST, j1 = 65 > j and s0 = 1: all of the above is one add of the
        // lane's constant offset, -3, -1 or L - 2)
        if constexpr (FAST) p = sBase + firstOff;
        // lane predicates as wave masks (SALU), turned back into per-lane
        // conditions with inverse_ballot (the mask is the select's condition):
        // no 0/1 materialisation chains.  Lane 0 / 1's bits come straight
        // from the mode (2: INSERT only, 1: both, 0: neither)
        const uint64_t roleM = FAST ? 3ull : (uint64_t)((0x130u >> (4 * mode)) & 3u);
        // (fast phase: every SEARCH lane is live and none is the block's last)
        const uint64_t liveM = FAST ? ~3ull | roleM : (bal(p <= mflimitP1) & ~3ull) | roleM;
        const uint64_t tmk = FAST ? 0ull : bal(p + step > mflimitP1) & liveM & ~3ull;
        const bool live = FAST ? true : __builtin_amdgcn_inverse_ballot_w64(liveM);
        const bool term = FAST ? false : __builtin_amdgcn_inverse_ballot_w64(tmk);
        const uint32_t lo = insOn ? insPos : sBase;
        const uint32_t hi = (FAST || sHi < mflimitP1 ? sHi : mflimitP1) + 8;
        uint64_t v8;
        // two if-regions and no else: the ring read is issued on both paths
        // (wasted, harmless, in the rare wide case), so the common path
        // carries no structurizer flow variable
        // (fast phase: hi - lo = 72, never wide)
        const bool wide = FAST ? false : hi - lo > 1024;
        if constexpr (kPrioT) {   // the check rides on the ring's advance (every 512 B of input or more)
            if (!wide && hi > V.B + kSR) {
                const uint32_t oldB = V.B;
                V.cover(hi);
                if (prioOn && ((oldB ^ V.B) >> tickShift)) prio.tick(V.B - o0, blen);
            }
        } else {
            if (!wide) V.cover(hi);
        }
        v8 = V.rd8(p);
        if (wide) {   // wide window (long searches): hash inputs straight from global
            if (ST) acc[13] += 1;
            v8 = gld8u(s + (p < n - 8 ? p : n - 8));
            uint32_t a = (uint32_t)v8, b = (uint32_t)(v8 >> 32);
            asm volatile("" : "+v"(a), "+v"(b));   // land it here, not at the join
            v8 = ((uint64_t)b << 32) | a;
        }
        const uint32_t w0 = (uint32_t)v8;
        uint32_t h, tg;
        if constexpr (G::HT && U16) {   // one product: hash4 = bits 19..31, tag = the TB bits below
            const uint32_t P = w0 * 2654435761u;
            h = P >> 19;
            tg = (P >> (19 - G::TB)) & ((1u << G::TB) - 1u);
        } else if constexpr (G::HT) {   // one product: hash5 = bits 52..63, tag = the TB bits below
            const uint64_t P = (v8 << 24) * 889523592379ull;
            h = (uint32_t)(P >> 52);
            tg = (uint32_t)(P >> (52 - G::TB)) & ((1u << G::TB) - 1u);
        } else {
            h = lz4_hash<U16>(w0, (uint32_t)(v8 >> 32));
            tg = G::tag(w0);
        }
        const uint32_t mark = (P17 ? p & G::PM : p) | (tg << G::PB);   // the lane's final table entry
        // ---- table probe: read, write the marker, read back (LDS ops of a wave run in order)
        const uint32_t ti = live ? h : dumIdx;
        uint32_t told;
        uint64_t pend = 0;   // same-bucket collisions inside the window (XCHG: none to resolve)
        if constexpr (XCHG) {
            told = tab.xchg(ti, mark);
        } else {
            told = tab.ld(ti);
            tab.st(ti, mark);
            WAVE_SYNC();
            const uint32_t sv = tab.rb(ti);
            pend = bal(sv != (mark & G::kRbMask));
        }
        const uint32_t dq = (p - told) & G::PM;   // P17: the distance, exact below 2^17
        uint32_t cand = P17 ? p - dq : told & G::PM;
        const uint64_t cokM = bal((P17 ? dq <= kDistMax : cand + kDistMax >= p) && (!LINK || cand >= lk.candLow)) &
                              liveM & ~tmk & ~1ull;
        uint64_t mm = cokM & bal((told >> G::PB) == (mark >> G::PB));
        bool maybe = __builtin_amdgcn_inverse_ballot_w64(mm);
        uint64_t sm = mm | tmk;
        STAMP_ADD(0, ts);
        // ---- resolve the first stop.  Exact in-window predecessors are
        // resolved (once) whenever a collision reaches the current stop
        // candidate -- also after a tag alias moved the stop further out.
        // The round trip: verify word + forward count words, catch-up bytes;
        // the previous sequence's stores go out behind them.
        w = 64;
        bool dd = false, twDone = false, twRedo = false;
        uint64_t gmask, aliased = 0;   // gmask: read only after dd set it
        // table writes for stop w: lanes past the stop put the old entry
        // back; on a collision (or when redone after a tag alias moved the
        // stop) the lanes up to the stop re-insert (last member of each group)
        // pB: the position of lane wlim (the last lane whose insert stays)
        auto table_writes = [&](uint32_t ws, bool wsTerm, uint32_t pB) {
            // (an SGPR-pinned version of this, w - ((tmk >> w) & 1) under an
            // asm "+s" constraint, drops a v_readfirstlane but costs 1 ms:
            // profiles/r04tidy_encoder_ab.txt)
            const int wlim = (ws == 64) ? 63 : (wsTerm ? (int)ws - 1 : (int)ws);
            const bool le = (int)L <= wlim;
            if constexpr (XCHG) {
                // after an alias moved the stop: the lanes up to it insert again
                // (exchanges, so the last of each bucket wins)
                if (twRedo) (void)tab.xchg((live && le) ? h : dumIdx, mark);
                // lanes past the stop: the first of each bucket puts back the
                // entry it displaced (the last mark up to the stop, or the
                // table's entry); a later one displaced a lane past the stop.
                // Lanes are in position order and every entry a lane can
                // displace is an older table entry or an earlier lane's
                // mark, so "displaced by no lane past the stop" is "its
                // position is at most lane wlim's" (P17 keeps positions
                // mod 2^17: compare distances from p)
                const bool first = P17 ? dq >= p - pB : (told & G::PM) <= pB;
                // (fast phase: a lane past the stop is a SEARCH lane, and live)
                tab.st(((FAST || live) && !le && first) ? h : dumIdx, told);
            } else {
                tab.st(((FAST || live) && !le) ? h : dumIdx, told);
                if (pend || twRedo) {
                    const uint64_t upto = wlim < 0 ? 0ull : mask_le((uint32_t)wlim);
                    const bool lastM = !dd || !(gmask & ~mask_le(L) & upto);
                    tab.st((live && le && lastM) ? h : dumIdx, mark);
                }
            }
            WAVE_SYNC();
        };
        // ip .. bc and wTerm are set on the path that reads them (a stop
        // inside the window): no per-window zeroing
        bool again = true;
        while (again) {
            w = sff1(sm);
            if (!dd && (pend & mask_le(w < 63 ? w : 63))) {
                if (ST) acc[12] += 1;
                dd = true;
                int pred = -1;
                gmask = 1ull << L;
                uint64_t todo = pend;
                while (todo) {   // one iteration per group of equal hashes
                    const uint32_t key = rdlane(h, (int)sff1(todo));
                    const uint64_t m = bal(live && h == key);
                    const bool inG = (m >> L) & 1;
                    const uint64_t below = m & ((1ull << L) - 1ull);
                    pred = inG ? (below ? 63 - __clzll((long long)below) : -1) : pred;
                    gmask = inG ? m : gmask;
                    todo &= ~m;
                }
                const int pi = (pred < 0 ? 0 : pred) * 4;
                const uint32_t pw = (uint32_t)__builtin_amdgcn_ds_bpermute(pi, (int)w0);   // predecessor's bytes
                const uint32_t pp = (uint32_t)__builtin_amdgcn_ds_bpermute(pi, (int)p);    // and position
                const bool ok = live && L != 0 && !term && pred >= 0 && pp + kDistMax >= p && pw == w0 &&
                                (!LINK || pp >= lk.candLow);
                maybe = maybe && pred < 0;
                cand = pred >= 0 ? pp : cand;
                mm = bal(maybe);
                sm = (bal(ok) | mm | tmk) & ~aliased;
            } else {
                wTerm = w < 64 && ((tmk >> w) & 1);
                again = false;
                if (w < 64 && !wTerm) {
                    ip = rdlane(p, (int)w);
                    cd = rdlane(cand, (int)w);
                    // every side from global memory: reading the near side(s)
                    // from the LDS ring when they lie in it was slower
                    // (profiles/r03j_encoder_ring_rt_ab.txt, r04s_encoder_ip_ring_ab.txt)
                    if constexpr (FAST) {
                        // first window after a match: anchor = sBase - 1 and lane w
                        // probes sBase + w - 2 (the TEST lane sBase - 1), so
                        // ip - anchor = w - 1, and cd >= 64 > w - 1 (fastBegS)
                        maxb = w - 1;
                        // lane 0: verify word; lanes 1 .. kCountLanes: count words;
                        // the next kCatchWords lanes: the 64 bytes below cd / ip as
                        // words (cd >= 64: inside the block); the rest repeat lane
                        // 0's address: one add of the lane's constant offset (and
                        // ip + 4 kCountLanes < last4: no clamp).  A backward lane
                        // whose word lies wholly beyond the bound (4 i >= maxb)
                        // also repeats lane 0's address, so fewer candidate-side
                        // lines are touched; whatever it then reports,
                        // 4 i + e >= maxb and the bound decides
                        const uint32_t ro = (int32_t)rtOff >= -(int32_t)((maxb + 3) & ~3u) ? rtOff : 0u;
                        cw = xld4(cd + ro);
                        iw = gld4u(s + (ip + ro));
                    } else {
                        // catch-up bound: lz4's lowLimit for the candidate's side
                        const uint32_t lowL = !LINK ? 0u : (cd >= o0 ? lk.lowIn : lk.lowDict);
                        maxb = w == 1 ? 0u : min(ip - anchor, cd > lowL ? cd - lowL : 0u);
                        // lane 0: verify word; lanes 1 .. kCountLanes: count words; the
                        // rest repeat lane 0's address (no further lines touched)
                        const bool cOn = L <= kCountLanes;
                        const uint32_t ci = cOn ? cd + 4 * L : cd, ii = cOn ? ip + 4 * L : ip;
                        // catch-up bytes: lane L the byte L + 1 below ip and below cd
                        // (L < 64 always holds, but the compiler does not know it:
                        // without the compare every encoder kernel's code moves)
                        const bool bOn = L < maxb && L < 64;
                        cw = xld4(ci < last4 ? ci : last4);
                        iw = gld4u(s + (ii < last4 ? ii : last4));
                        uint32_t bix = bOn ? ip - L - 1 : o0, bcx = bOn ? cd - L - 1 : o0;   // (o0: a byte of the block itself)
                        asm volatile("" : "+v"(bix), "+v"(bcx));   // 32-bit offsets, SGPR-base loads
                        bi = s[bix];
                        bc = xld1(bcx);
                    }
                    if (havePe) {
                        if constexpr (FAST) store_pending_fast();
                        else store_pending();
                    }
                    table_writes(w, false, ip);   // in the round trip's shadow; redone if w moves
                    twDone = true;
                    if (((mm >> w) & 1) && rdlane(cw, 0) != rdlane(w0, (int)w)) {   // tag alias: no match here
                        if (ST) acc[11] += 1;
                        // drain this try's loads here, so the loop head's load
                        // registers carry nothing pending into the common path
                        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
                        aliased |= 1ull << w;
                        sm &= ~(1ull << w);
                        again = true;
                        twDone = false;
                        twRedo = true;
                    }
                }
            }
        }
        if (havePe) {
            if constexpr (FAST) store_pending_fast();
            else store_pending();
        }
        // no stop in the window (w == 64): every insert stays, nothing to put
        // back -- unless an alias moved the stop here after the lanes past the
        // old one were put back (twRedo: they insert again)
        if (!twDone && (!XCHG || w < 64 || twRedo)) table_writes(w, wTerm, rdlane(p, (int)(w < 64 ? w - 1 : 63)));
        STAMP_ADD(1, ts);
        STAMP_ADD(2, ts);
        if constexpr (FAST) {
            // no stop: the search goes on in the general body, which resumes
            // it from the continuation state written behind this loop (about
            // 1 window in 20 is a continuation)
            if (w == 64) {
                sBase += 62;
                fcont = true;
                sw = true;
            }
        } else if (w == 64) {   // no stop: the search goes on
            sBase += 62 * s0 + (62 > j1 ? 62 - j1 : 0u);
            k0 += 62;
            s0 = (63 + k0) >> 6;   // k0 >= 62: no max(1, .) needed
            j1 = (k0 < 65 ? 65u : ((k0 - 1) & ~63u) + 65) - k0;
            mode = 0;
            spanHi = 61 * s0 + (61 > j1 ? 61 - j1 : 0u);
        }
      } while (!FAST && w == 64);
        if (FAST && w == 64) {
            // phase left inside a search: the general loop resumes it
        } else if (wTerm) {
            done = true;
        } else {
            // ---- catch-up (backwards) and LZ4_count (forwards from ip + 4).
            // bi/bc are consumed on every path, so no load of this window is
            // left pending into the next window's round trip.
            uint32_t back = 0;
            if constexpr (!FAST) {
                asm volatile("" ::"v"(bi), "v"(bc));
                uint64_t fm = ~(bal(L < maxb) & bal(bi == bc));
                while (fm == 0 && back + 64 < maxb) {   // catch-up longer than 64 bytes
                    back += 64;
                    const uint32_t kb = back + L + 1;
                    const bool on = kb <= maxb;
                    fm = ~bal(on && s[on ? ip - kb : o0] == xld1(on ? cd - kb : o0));
                }
                back = fm ? back + (uint32_t)__builtin_ctzll(fm) : maxb;
            }
            const uint32_t lim = matchlimit - (ip + kMinMatch);
            uint32_t mc;
            {
                const uint32_t x = cw ^ iw;
                uint32_t e;
                if constexpr (FAST) {
                    // equal bytes from the word's near end: its low end in a
                    // forward lane, its high end in a backward one
                    // (lim >= 4 kCountLanes: no clamp)
                    const bool bk = __builtin_amdgcn_inverse_ballot_w64(kBackLanes);
                    e = x ? ((bk ? (uint32_t)__builtin_clz(x) : (uint32_t)__builtin_ctz(x)) >> 3) : 4u;
                } else {
                    const uint32_t rel = 4 * L - 4;
                    e = x ? ((uint32_t)__builtin_ctz(x) >> 3) : 4u;
                    e = min(e, lim - rel);
                    e = rel < lim ? e : 0u;   // (lane 0's e is masked out below)
                }
                const uint64_t nfAll = bal(e < 4);
                const uint64_t nf = nfAll & (mask_le(kCountLanes) & ~1ull);
                if constexpr (FAST) {
                    // the first backward word with a difference ends the catch-up,
                    // unless the bound (at most 62 < 4 kCatchWords) does so first
                    const uint64_t nb = nfAll & kBackLanes;
                    if (nb) {
                        const uint32_t f = (uint32_t)__builtin_ctzll(nb);
                        back = min(4 * (f - (kCountLanes + 1)) + rdlane(e, (int)f), maxb);
                    } else {
                        back = maxb;
                    }
                }
                if (nf) {
                    const uint32_t f = (uint32_t)__builtin_ctzll(nf);
                    mc = 4 * (f - 1) + rdlane(e, (int)f);
                } else {
                    mc = 4 * kCountLanes;
                    uint64_t nf2 = 0;
                    while (!nf2) {   // long match: 256 bytes per round
                        const uint32_t r2 = mc + 4 * L;
                        const uint32_t a2 = ip + kMinMatch + r2, c2 = cd + kMinMatch + r2;
                        const uint32_t x2 = gld4u(s + (a2 < last4 ? a2 : last4)) ^ xld4(c2 < last4 ? c2 : last4);
                        uint32_t e2 = min(x2 ? ((uint32_t)__builtin_ctz(x2) >> 3) : 4u, lim - r2);
                        e2 = r2 < lim ? e2 : 0u;
                        nf2 = bal(e2 < 4);
                        mc += nf2 ? 4 * (uint32_t)__builtin_ctzll(nf2) + rdlane(e2, (int)__builtin_ctzll(nf2))
                                  : 256u;
                    }
                }
            }
            STAMP_ADD(3, ts);
            // ---- sequence layout (stored during the next round trip)
            const uint32_t lit = ip - anchor - back, mcf = mc + back;
            pe.lit = lit;
            pe.mcf = mcf;
            pe.off = ip - cd;
            pe.anchor = anchor;
            {
                const uint32_t litExt = ext_len(lit), mlExt = ext_len(mcf);
                pe.litExt = litExt;
                pe.mlExt = mlExt;
                // 1.9.3's limitedOutput margins; both hold whenever
                // op + 2 (lit + mcf) + 16 <= cap, so the exact test runs rarely
                // (fast phase: condition (b) above holds, neither can fire)
                if constexpr (!FAST) {
                    if (op + 2 * (lit + mcf) + 16 > capL) {
                        fail = (w != 1 && op + 1 + lit + 8 + lit / 255 > cap) ||
                               (op + 1 + litExt + lit + 2 + 6 + (mcf + 240) / 255 > cap);
                    }
                }
                pe.op = op;
                havePe = FAST ? true : !fail;
                if constexpr (PUB) {   // every sequence before this one has been stored: [0, op) is final
                    if ((op ^ (op + 1 + litExt + lit + 2 + mlExt)) >> kPubShift) publish_progress(pub, op);
                }
                op += 1 + litExt + lit + 2 + mlExt;
            }
            const uint32_t ipe = ip + kMinMatch + mc;
            anchor = ipe;
            if constexpr (FAST) {
                // one compare, as in the general phase: past fastEndS the
                // general loop decides whether the block is done
                sw = ipe >= fastEndS;
            } else {
                done = fail || ipe >= mflimitP1;
                if constexpr (kFastT) {
                    if (fastEndS == 0 && op + (n - ipe) + (n - ipe) / 255 + kFastOutSlack <= cap)
                        fastEndS = fastEndV;   // (b) holds from here to the block's end
                    sw = !fail && ipe < fastEndS;   // (fastEndS < mflimitP1)
                    // (c): every later ip of the phase is at or above this ipe
                    sw = sw && ipe >= fastBegS;
                }
            }
            sBase = ipe + 1;
            if constexpr (!FAST) {
                mode = 1;
                k0 = 0;
                s0 = 1;
                j1 = 65;
                spanHi = 61;
            }
            STAMP_ADD(4, ts);
        }
    }
    // FAST: the window state the general body resumes from, written once per
    // phase change and not per sequence -- the second window of a search
    // (k0 = 62: the step rises at j = 3), or the first window after a match
    if constexpr (FAST) {
        k0 = fcont ? 62u : 0u;
        j1 = fcont ? 3u : 65u;
        mode = fcont ? 0u : 1u;
        spanHi = fcont ? 119u : 61u;
        s0 = 1;
    }
}
