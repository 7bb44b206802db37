/*
 * lz4hc_dict_model.c — host model of LZ4-HC 1.9.3 with an external
 * dictionary, as the batched call lz4mtHipCompressBatchDictHC defines a chunk
 * (include/lz4mt_hip.h section 5c):
 *
 *   LZ4_resetStreamHC_fast(s, level); LZ4_loadDictHC(s, dict, dictSize);
 *   LZ4_compress_HC_continue(s, src, dst, n, cap);
 *
 * on a fresh stream, dictionary and source in buffers of their own.  It is
 * the restatement the kernels in lz4mt_amd/csrc/lz4mt_hc.hip (HcDictBlock)
 * were ported from, in the same coordinates: position P of the effective
 * dictionary (its last E <= 64 KiB bytes) is P in [0, E), chunk byte p is
 * position E + p; lz4hc's own index of a position is P + 64 KiB.  The chain
 * is held the way the kernels hold it: link[P] = lz4hc's chainTable value of
 * an inserted position (distance to the previous position with the same
 * hash, 65535 when there is none within reach), 0 for a position that is
 * never inserted (the dictionary's last three).
 *
 * tools/lz4hc_dict_diff.py builds this file and compares it with liblz4.
 * Not part of the library.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MINMATCH 4
#define LASTLITERALS 5
#define MFLIMIT 12
#define MIN_LENGTH 13
#define DIST_MAX 65535u
#define HASH_LOG 15
#define OPTIMAL_ML 18
#define OPT_NUM 4096
#define TRAILING_LITERALS 3

typedef struct {
    const uint8_t* dict;   /* effective dictionary, E bytes */
    uint32_t E;
    const uint8_t* s;      /* chunk, n bytes */
    uint32_t n;
    uint16_t* link;        /* E + n entries */
    uint32_t* head;        /* 32768: position + 1 of the hash's latest inserted position */
    uint32_t next;         /* next position to insert */
    int attempts, pattern;
} ctx_t;

static inline uint32_t rd32s(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
static inline uint32_t rd16s(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
static inline uint32_t hash4(uint32_t v) { return (v * 2654435761u) >> (32 - HASH_LOG); }

/* LZ4HC_Insert over one segment: positions [from, to) of seg (at position base) */
static void insert_seg(ctx_t* c, const uint8_t* seg, uint32_t base, uint32_t from, uint32_t to) {
    for (uint32_t p = from; p < to; ++p) {
        const uint32_t h = hash4(rd32s(seg + p)), P = base + p;
        const uint32_t q1 = c->head[h];
        const uint32_t d = q1 ? P + 1 - q1 : DIST_MAX;
        c->link[P] = (uint16_t)(d > DIST_MAX ? DIST_MAX : d);
        c->head[h] = P + 1;
    }
}
/* LZ4HC_Insert(ctx, ip): every chunk position below ip (local) */
static void insert_to(ctx_t* c, uint32_t ip) {
    if (c->next < ip) { insert_seg(c, c->s, c->E, c->next, ip); c->next = ip; }
}

/* LZ4HC_protectDictEnd */
static inline int protect(const ctx_t* c, uint32_t P) { return (uint32_t)((c->E - 1) - P) >= 3; }

/* LZ4HC_InsertAndGetWiderMatch; ip, iLow, iHigh are chunk offsets; *mpos is
 * the match position minus E (wrapping: ip - *mpos is the offset) */
static int wider(ctx_t* c, uint32_t ip, uint32_t iLow, uint32_t iHigh, int longest, uint32_t* mpos, uint32_t* spos,
                 int chainSwap) {
    const uint32_t E = c->E, IP = ip + E;
    const uint32_t lowest = IP > DIST_MAX ? IP - DIST_MAX : 0u;
    const uint32_t lookBack = ip - iLow;
    const uint8_t* s = c->s;
    const uint8_t* dict = c->dict;
    int nbAttempts = c->attempts;
    const uint32_t pat = rd32s(s + ip);
    const uint8_t pb = (uint8_t)pat;
    int repeat = 0;
    uint32_t srcPatLen = 0, mcp = 0;
    insert_to(c, ip);
    const uint32_t h1 = c->head[hash4(pat)];
    if (!h1) return longest;
    uint32_t m = h1 - 1;
    while (m >= lowest && nbAttempts > 0) {
        int matchLength = 0;
        --nbAttempts;
        if (m >= E) {   /* in the chunk */
            const uint32_t mc = m - E;
            if (rd16s(s + iLow + longest - 1) == rd16s(s + mc - lookBack + longest - 1) && rd32s(s + mc) == pat) {
                int back = 0;
                while (lookBack && (uint32_t)-back < lookBack && (uint32_t)-back < mc && s[ip + back - 1] == s[mc + back - 1])
                    --back;
                int ml = MINMATCH;
                while (ip + ml < iHigh && s[ip + ml] == s[mc + ml]) ++ml;
                ml -= back;
                matchLength = ml;
                if (ml > longest) { longest = ml; *mpos = mc + (uint32_t)back; *spos = ip + (uint32_t)back; }
            }
        } else {        /* in the dictionary: no pre-filter, counts run over its end into the chunk */
            /* One of the dictionary's last three positions (never inserted) is reached when the
             * optimal parser follows the chain of position m + mcp: lz4hc 1.9.3 reads its four
             * bytes, up to three of them past the dictionary's end.  Here that is "not equal". */
            if (m + 4 <= E && rd32s(dict + m) == pat) {
                uint32_t vLimit = ip + (E - m);
                if (vLimit > iHigh) vLimit = iHigh;
                int ml = MINMATCH;
                while (ip + ml < vLimit && s[ip + ml] == dict[m + ml]) ++ml;
                if (ip + ml == vLimit && vLimit < iHigh) {
                    uint32_t k = 0;
                    while (ip + ml + k < iHigh && s[ip + ml + k] == s[k]) ++k;
                    ml += (int)k;
                }
                int back = 0;
                while (lookBack && (uint32_t)-back < lookBack && (uint32_t)-back < m && s[ip + back - 1] == dict[m + back - 1])
                    --back;
                ml -= back;
                matchLength = ml;
                if (ml > longest) { longest = ml; *mpos = m + (uint32_t)back - E; *spos = ip + (uint32_t)back; }
            }
        }
        if (chainSwap && matchLength == longest && m + (uint32_t)longest <= IP) {
            uint32_t dtn = 1;
            const int end = longest - MINMATCH + 1;
            int step = 1, accel = 1 << 4;
            for (int pos = 0; pos < end; pos += step) {
                const uint32_t cd = c->link[m + (uint32_t)pos];
                step = accel++ >> 4;
                if (cd > dtn) { dtn = cd; mcp = (uint32_t)pos; accel = 1 << 4; }
            }
            if (dtn > 1) {
                if (dtn > m) break;   /* below the dictionary: under `lowest` */
                m -= dtn;
                continue;
            }
        }
        {
            const uint32_t distNext = c->link[m];
            if (c->pattern && distNext == 1 && mcp == 0) {
                const uint32_t cand = m - 1;
                if (repeat == 0) {
                    if (((pat & 0xFFFF) == (pat >> 16)) & ((pat & 0xFF) == (pat >> 24))) {
                        repeat = 1;
                        uint32_t k = ip + 4;
                        while (k < iHigh && s[k] == pb) ++k;
                        srcPatLen = k - ip;
                    } else {
                        repeat = 2;
                    }
                }
                if (repeat == 1 && cand >= lowest && protect(c, cand)) {
                    const int ext = cand < E;
                    const uint32_t c32 = ext ? rd32s(dict + cand) : rd32s(s + (cand - E));
                    if (c32 == pat) {
                        uint32_t fwd, back;
                        if (ext) {
                            uint32_t k = cand + 4;
                            while (k < E && dict[k] == pb) ++k;
                            fwd = k - cand;
                            if (k == E) {   /* the run goes on from the chunk's start */
                                uint32_t j = 0;
                                while (j < iHigh && s[j] == pb) ++j;
                                fwd += j;
                            }
                            back = 0;
                            while (back < cand && dict[cand - back - 1] == pb) ++back;
                        } else {
                            const uint32_t cl = cand - E;
                            uint32_t k = cl + 4;
                            while (k < iHigh && s[k] == pb) ++k;
                            fwd = k - cl;
                            back = 0;
                            while (back < cl && s[cl - back - 1] == pb) ++back;
                            if (back == cl && E > 0) {   /* ... and backward from the dictionary's end */
                                uint32_t j = 0;
                                while (j < E && dict[E - j - 1] == pb) ++j;
                                back += j;
                            }
                        }
                        {
                            const uint32_t lo = cand - back;
                            back = cand - (lo > lowest ? lo : lowest);
                        }
                        const uint32_t seg = back + fwd;
                        if (seg >= srcPatLen && fwd <= srcPatLen) {
                            const uint32_t nm = cand + fwd - srcPatLen;
                            m = protect(c, nm) ? nm : E;
                        } else {
                            const uint32_t nm = cand - back;
                            if (!protect(c, nm)) {
                                m = E;
                            } else {
                                m = nm;
                                if (lookBack == 0) {
                                    const uint32_t maxML = seg < srcPatLen ? seg : srcPatLen;
                                    if ((uint32_t)longest < maxML) {
                                        if (IP - m > DIST_MAX) break;
                                        longest = (int)maxML;
                                        *mpos = m - E;
                                        *spos = ip;
                                    }
                                    const uint32_t dn = c->link[m];
                                    if (dn > m) break;   /* below the dictionary: under `lowest` */
                                    m -= dn;
                                }
                            }
                        }
                        continue;
                    }
                }
            }
        }
        {
            const uint32_t dfol = c->link[m + mcp];
            if (m < dfol || dfol == 0) break;   /* (0: lz4hc would spend its attempts on the same position) */
            m -= dfol;
        }
    }
    return longest;
}

/* LZ4HC_encodeSequence; 1 = overflow */
static int encode(const ctx_t* c, uint32_t* ip, uint32_t* op, uint32_t* anchor, int ml, uint32_t ref, uint8_t* d,
                  int limit, uint32_t cap) {
    const uint32_t token = (*op)++;
    uint32_t length = *ip - *anchor;
    if (limit && (uint64_t)*op + length / 255 + length + (2 + 1 + LASTLITERALS) > cap) return 1;
    if (length >= 15) {
        uint32_t len = length - 15;
        d[token] = 15 << 4;
        for (; len >= 255; len -= 255) d[(*op)++] = 255;
        d[(*op)++] = (uint8_t)len;
    } else {
        d[token] = (uint8_t)(length << 4);
    }
    memcpy(d + *op, c->s + *anchor, length);
    *op += length;
    const uint32_t off = *ip - ref;
    d[(*op)++] = (uint8_t)off;
    d[(*op)++] = (uint8_t)(off >> 8);
    length = (uint32_t)ml - MINMATCH;
    if (limit && (uint64_t)*op + length / 255 + (1 + LASTLITERALS) > cap) return 1;
    if (length >= 15) {
        d[token] += 15;
        length -= 15;
        for (; length >= 255; length -= 255) d[(*op)++] = 255;
        d[(*op)++] = (uint8_t)length;
    } else {
        d[token] += (uint8_t)length;
    }
    *ip += (uint32_t)ml;
    *anchor = *ip;
    return 0;
}

static int last_literals(const ctx_t* c, uint32_t anchor, uint32_t op, uint8_t* d, int limit, uint32_t cap) {
    const uint32_t run = c->n - anchor;
    const uint32_t llAdd = (run + 255 - 15) / 255;
    if (limit && (uint64_t)op + 1 + llAdd + run > cap) return 0;
    if (run >= 15) {
        uint32_t acc = run - 15;
        d[op++] = 15 << 4;
        for (; acc >= 255; acc -= 255) d[op++] = 255;
        d[op++] = (uint8_t)acc;
    } else {
        d[op++] = (uint8_t)(run << 4);
    }
    memcpy(d + op, c->s + anchor, run);
    return (int)(op + run);
}

/* LZ4HC_compress_hashChain */
static int hash_chain(ctx_t* c, uint8_t* d, uint32_t cap, int limit) {
    const uint32_t n = c->n;
    uint32_t ip = 0, anchor = 0, op = 0;
    const uint32_t mflimit = n >= 12 ? n - 12 : 0, matchlimit = n >= 5 ? n - 5 : 0;
    int ml0, ml, ml2, ml3;
    uint32_t start0 = 0, ref0 = 0, ref = 0, start2 = 0, ref2 = 0, start3 = 0, ref3 = 0;
    if (n < MIN_LENGTH) return last_literals(c, anchor, op, d, limit, cap);
    while (ip <= mflimit) {
        {
            uint32_t useless = ip;
            ml = wider(c, ip, ip, matchlimit, MINMATCH - 1, &ref, &useless, 0);
        }
        if (ml < MINMATCH) { ++ip; continue; }
        start0 = ip; ref0 = ref; ml0 = ml;
    search2:
        if (ip + (uint32_t)ml <= mflimit) ml2 = wider(c, ip + (uint32_t)ml - 2, ip, matchlimit, ml, &ref2, &start2, 0);
        else ml2 = ml;
        if (ml2 == ml) {
            if (encode(c, &ip, &op, &anchor, ml, ref, d, limit, cap)) return 0;
            continue;
        }
        if (start0 < ip && start2 < ip + (uint32_t)ml0) { ip = start0; ref = ref0; ml = ml0; }
        if (start2 - ip < 3) {
            ml = ml2; ip = start2; ref = ref2;
            goto search2;
        }
    search3:
        if (start2 - ip < OPTIMAL_ML) {
            int nml = ml;
            if (nml > OPTIMAL_ML) nml = OPTIMAL_ML;
            if (ip + (uint32_t)nml > start2 + (uint32_t)ml2 - MINMATCH) nml = (int)(start2 - ip) + ml2 - MINMATCH;
            const int corr = nml - (int)(start2 - ip);
            if (corr > 0) { start2 += (uint32_t)corr; ref2 += (uint32_t)corr; ml2 -= corr; }
        }
        if (start2 + (uint32_t)ml2 <= mflimit)
            ml3 = wider(c, start2 + (uint32_t)ml2 - 3, start2, matchlimit, ml2, &ref3, &start3, 0);
        else ml3 = ml2;
        if (ml3 == ml2) {
            if (start2 < ip + (uint32_t)ml) ml = (int)(start2 - ip);
            if (encode(c, &ip, &op, &anchor, ml, ref, d, limit, cap)) return 0;
            ip = start2;
            if (encode(c, &ip, &op, &anchor, ml2, ref2, d, limit, cap)) return 0;
            continue;
        }
        if (start3 < ip + (uint32_t)ml + 3) {
            if (start3 >= ip + (uint32_t)ml) {
                if (start2 < ip + (uint32_t)ml) {
                    const int corr = (int)(ip + (uint32_t)ml - start2);
                    start2 += (uint32_t)corr; ref2 += (uint32_t)corr; ml2 -= corr;
                    if (ml2 < MINMATCH) { start2 = start3; ref2 = ref3; ml2 = ml3; }
                }
                if (encode(c, &ip, &op, &anchor, ml, ref, d, limit, cap)) return 0;
                ip = start3; ref = ref3; ml = ml3;
                start0 = start2; ref0 = ref2; ml0 = ml2;
                goto search2;
            }
            start2 = start3; ref2 = ref3; ml2 = ml3;
            goto search3;
        }
        if (start2 < ip + (uint32_t)ml) {
            if (start2 - ip < OPTIMAL_ML) {
                if (ml > OPTIMAL_ML) ml = OPTIMAL_ML;
                if (ip + (uint32_t)ml > start2 + (uint32_t)ml2 - MINMATCH) ml = (int)(start2 - ip) + ml2 - MINMATCH;
                const int corr = ml - (int)(start2 - ip);
                if (corr > 0) { start2 += (uint32_t)corr; ref2 += (uint32_t)corr; ml2 -= corr; }
            } else {
                ml = (int)(start2 - ip);
            }
        }
        if (encode(c, &ip, &op, &anchor, ml, ref, d, limit, cap)) return 0;
        ip = start2; ref = ref2; ml = ml2;
        start2 = start3; ref2 = ref3; ml2 = ml3;
        goto search3;
    }
    return last_literals(c, anchor, op, d, limit, cap);
}

typedef struct { int price, off, mlen, litlen; } opt_t;
static int lit_price(int l) { return l + (l >= 15 ? 1 + (l - 15) / 255 : 0); }
static int seq_price(int l, int m) { return 3 + lit_price(l) + (m >= 19 ? 1 + (m - 19) / 255 : 0); }

static void longer(ctx_t* c, uint32_t p, int minLen, int* len, int* off) {
    uint32_t mpos = 0, spos = p;
    const int ml = wider(c, p, p, c->n - LASTLITERALS, minLen, &mpos, &spos, 1);
    *len = ml > minLen ? ml : 0;
    *off = ml > minLen ? (int)(spos - mpos) : 0;
}

/* LZ4HC_compress_optimal */
static int optimal(ctx_t* c, uint8_t* d, uint32_t cap, int limit, int suff, int fullUpdate) {
    const uint32_t n = c->n;
    uint32_t ip = 0, anchor = 0, op = 0;
    opt_t* opt = (opt_t*)malloc(sizeof(opt_t) * (OPT_NUM + TRAILING_LITERALS + 1));
    int r = 0;
    if (suff >= OPT_NUM) suff = OPT_NUM - 1;
    const uint32_t mflimit = n >= 12 ? n - 12 : 0;
    while (n >= MFLIMIT && ip <= mflimit) {   /* (no LZ4_minLength test in the optimal parser) */
        const int llen = (int)(ip - anchor);
        int best_mlen, best_off, cur, last = 0, fmLen, fmOff;
        longer(c, ip, MINMATCH - 1, &fmLen, &fmOff);
        if (fmLen == 0) { ++ip; continue; }
        if (fmLen > suff) {
            if (encode(c, &ip, &op, &anchor, fmLen, ip - (uint32_t)fmOff, d, limit, cap)) goto done;
            continue;
        }
        for (int k = 0; k < MINMATCH; k++) {
            opt[k].mlen = 1; opt[k].off = 0; opt[k].litlen = llen + k; opt[k].price = lit_price(llen + k);
        }
        for (int k = MINMATCH; k <= fmLen; k++) {
            opt[k].mlen = k; opt[k].off = fmOff; opt[k].litlen = llen; opt[k].price = seq_price(llen, k);
        }
        last = fmLen;
        for (int a = 1; a <= TRAILING_LITERALS; a++) {
            opt[last + a].mlen = 1; opt[last + a].off = 0; opt[last + a].litlen = a;
            opt[last + a].price = opt[last].price + lit_price(a);
        }
        for (cur = 1; cur < last; cur++) {
            int nmLen, nmOff;
            if (ip + (uint32_t)cur > mflimit) break;
            if (fullUpdate) {
                if (opt[cur + 1].price <= opt[cur].price && opt[cur + MINMATCH].price < opt[cur].price + 3) continue;
            } else {
                if (opt[cur + 1].price <= opt[cur].price) continue;
            }
            longer(c, ip + (uint32_t)cur, fullUpdate ? MINMATCH - 1 : last - cur, &nmLen, &nmOff);
            if (!nmLen) continue;
            if (nmLen > suff || nmLen + cur >= OPT_NUM) {
                best_mlen = nmLen; best_off = nmOff; last = cur + 1;
                goto encode_path;
            }
            {
                const int bl = opt[cur].litlen;
                for (int l = 1; l < MINMATCH; l++) {
                    const int price = opt[cur].price - lit_price(bl) + lit_price(bl + l), pos = cur + l;
                    if (price < opt[pos].price) {
                        opt[pos].mlen = 1; opt[pos].off = 0; opt[pos].litlen = bl + l; opt[pos].price = price;
                    }
                }
            }
            for (int ml = MINMATCH; ml <= nmLen; ml++) {
                const int pos = cur + ml;
                int price, ll;
                if (opt[cur].mlen == 1) {
                    ll = opt[cur].litlen;
                    price = (cur > ll ? opt[cur - ll].price : 0) + seq_price(ll, ml);
                } else {
                    ll = 0;
                    price = opt[cur].price + seq_price(0, ml);
                }
                if (pos > last + TRAILING_LITERALS || price <= opt[pos].price) {
                    if (ml == nmLen && last < pos) last = pos;
                    opt[pos].mlen = ml; opt[pos].off = nmOff; opt[pos].litlen = ll; opt[pos].price = price;
                }
            }
            for (int a = 1; a <= TRAILING_LITERALS; a++) {
                opt[last + a].mlen = 1; opt[last + a].off = 0; opt[last + a].litlen = a;
                opt[last + a].price = opt[last].price + lit_price(a);
            }
        }
        best_mlen = opt[last].mlen;
        best_off = opt[last].off;
        cur = last - best_mlen;
    encode_path:
        {
            int cp = cur, sml = best_mlen, soff = best_off;
            for (;;) {
                const int nml = opt[cp].mlen, noff = opt[cp].off;
                opt[cp].mlen = sml; opt[cp].off = soff;
                sml = nml; soff = noff;
                if (nml > cp) break;
                cp -= nml;
            }
        }
        {
            int rPos = 0;
            while (rPos < last) {
                const int ml = opt[rPos].mlen, off = opt[rPos].off;
                if (ml == 1) { ++ip; ++rPos; continue; }
                rPos += ml;
                if (encode(c, &ip, &op, &anchor, ml, ip - (uint32_t)off, d, limit, cap)) goto done;
            }
        }
    }
    r = last_literals(c, anchor, op, d, limit, cap);
done:
    free(opt);
    return r;
}

/* The block of chunk src[0, n) against dict[0, dictSize) at `level` (3..12,
 * above counts as 12) into dst[0, cap); returns its size, 0 = does not fit. */
int hcdict_model_compress(const uint8_t* dict, uint32_t dictSize, const uint8_t* src, uint32_t n, uint8_t* dst,
                          uint32_t cap, int level) {
    static const int kAttempts[13] = {2, 2, 2, 4, 8, 16, 32, 64, 128, 256, 96, 512, 16384};
    static const int kTarget[13] = {16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 64, 128, OPT_NUM};
    if (level < 1) level = 9;
    if (level > 12) level = 12;
    ctx_t c;
    c.E = dictSize > 65536 ? 65536 : dictSize;
    c.dict = dict + (dictSize - c.E);
    c.s = src;
    c.n = n;
    c.link = (uint16_t*)calloc((size_t)c.E + n + 1, sizeof(uint16_t));
    c.head = (uint32_t*)calloc(1u << HASH_LOG, sizeof(uint32_t));
    c.next = 0;
    c.attempts = kAttempts[level];
    c.pattern = level >= 10 || kAttempts[level] > 128;
    if (c.E >= 4) insert_seg(&c, c.dict, 0, 0, c.E - 3);   /* LZ4_loadDictHC; the last 3 are never inserted */
    const int limit = (uint64_t)cap < (uint64_t)n + n / 255 + 16;
    const int r = level <= 9 ? hash_chain(&c, dst, cap, limit) : optimal(&c, dst, cap, limit, kTarget[level], level == 12);
    free(c.link);
    free(c.head);
    return r;
}
