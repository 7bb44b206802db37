"""The fixed frames of the synthesized-frame tests: seeds, block counts, sizes
and the variants that fail.  The CPU checks (test_frame_synth.py) and the GPU
tests (test_gpu_frame_synth.py) build the same bytes from here, so what the
CPU module asserts about the frames -- the oracle decodes every valid one to
the builder's text, every source class occurs -- holds for what the GPU is fed.

``cases(name)`` lists the frames of one recipe: each valid frame with block
checksums plus a content checksum ("SX") and with neither ("sx"), then the
variants that fail, each with the code and the index of the block that stops
the decode.  Block id 4 unless the name says otherwise.
"""
import collections
import functools
import random

import lz4_frame_synth as F
import lz4_synth as S
import oracle
import synth_cases as K

OK, BLOCK_CHECKSUM_MISMATCH, DECOMPRESS_FAIL, INVALID_BLOCK_SIZE = 0, 16, 18, 20

# frame: an F.Frame; code / fail: the expected result and the block that stops the decode (None: valid)
Case = collections.namedtuple("Case", "name frame code fail")

LINKED = ["short", "many", "chain", "span", "sizes", "prestart", "b5", "b7", "lz4f"]
INDEP = ["indep4", "indep5", "indep600"]
ROUNDS = ["short", "many", "chain", "span"]       # decoded again under the round caps
SHORT_BATCHES = ["short", "many", "chain"]        # every 16-block batch decodes less than 64 KiB

SHORT_BLOCKS = 300
MANY_BLOCKS = 1150
MANY_HI, MANY_LO = 1060, 500                       # failing indices above and below one scan pass (1024)
CHAIN_BLOCKS = 200
N_DAMAGED = 40


def _profile(i, runs=True):
    """Every third block in runs (where ``runs``), the dictionary classes in turn at P < 64."""
    kind = "runs" if runs and i % 3 == 1 else "mixed"
    return {"kind": kind, "low": S.DICT_CLASSES[i % len(S.DICT_CLASSES)]}


def _short(lz4f):
    """Short linked blocks of 20 to 6000 target bytes; every seventh stored, every eleventh with
    sources 1, 2, 3..9 and 10 or more blocks back."""
    b = F.FrameBuilder(4, lz4f=lz4f)
    rnd = random.Random(4100 + lz4f)
    for i in range(SHORT_BLOCKS):
        n = rnd.randrange(20, 6001)
        if i % 7 == 6:
            b.add_stored(rnd.randbytes(n))
        elif i % 11 == 5:
            b.add_directed(rnd, [1, 2, rnd.randrange(3, 10), rnd.randrange(10, 41)], span=i % 22 == 5)
        else:
            b.add_synth(rnd, n, _profile(i))
    return b


def _many():
    """More blocks than one scan pass of k_dlink_plan (1024), 12 to 100 target bytes each."""
    b = F.FrameBuilder(4)
    rnd = random.Random(4200)
    for i in range(MANY_BLOCKS):
        n = rnd.randrange(12, 101)
        if i % 7 == 6:
            b.add_stored(rnd.randbytes(n))
        elif i % 11 == 5:
            b.add_directed(rnd, [1, 2, rnd.randrange(3, 10), rnd.randrange(10, 200)], span=i % 22 == 5)
        else:
            b.add_synth(rnd, n, _profile(i, runs=False))
    return b


def _chain():
    """Every block copies the head of the previous one (offset = that block's length) and adds a
    few literals: a byte of block 0 reaches every block.  From block 2 on a second, short match
    starts two to five blocks back, so the bytes depend on what a gather takes from the blocks
    before b - 1 as well."""
    b = F.FrameBuilder(4)
    rnd = random.Random(4300)
    b.add_writer(b.writer(rnd), lit=rnd.randrange(70, 301))
    for i in range(1, CHAIN_BLOCKS):
        prev = b.sizes[-1]
        w = b.writer(rnd)
        w.seq(0, prev, rnd.randrange(60, min(prev, 270) + 1))
        if i >= 2:
            j = i - rnd.randrange(2, min(i, 5) + 1)
            G = b.starts[j] + rnd.randrange(b.sizes[j] - 8)
            w.seq(0, len(b.text) + w.op - G, rnd.randrange(4, 9))
        b.add_writer(w, lit=rnd.randrange(10, 21))
    return b


def _span(stored0):
    """Blocks of 50 literals; matches of 275 bytes and more that start three and ten blocks back
    and run into the block's own output, over a zero-size compressed block (the token 0x00) and,
    with ``stored0``, a stored block of length 0."""
    b = F.FrameBuilder(4)
    rnd = random.Random(4400)

    def fill(k):
        for _ in range(k):
            b.add_writer(b.writer(rnd), lit=50)

    def reach(back, lit, extra):
        G = b.starts[b.n - back] + 7
        w = b.writer(rnd)
        off = len(b.text) + lit - G
        w.seq(lit, off, off + extra)              # longer than its offset: through the history into itself
        b.add_writer(w, lit=12)

    fill(12)
    reach(3, 6, 275)
    b.add_block(b"\x00", b"")
    if stored0:
        b.add_stored(b"")
    fill(2)
    reach(10, 0, 275)
    fill(1)
    reach(3, 15, 300)                              # three back: over the two empty blocks
    fill(3)
    return b


def _exact(b, rnd, total):
    """A compressed block that decodes to exactly ``total`` bytes."""
    w = b.writer(rnd)
    for _ in range(5):
        S.mixed_seq(w, total)
    S.grow(w, total - 1000)
    return w, total - w.op


@functools.lru_cache(maxsize=None)
def _sizes():
    """Short blocks between blocks of exactly blockMax: decoded, stored, and as a record."""
    b = F.FrameBuilder(4)
    rnd = random.Random(4500)
    bm = b.bm
    alt = {}
    for i in range(3):
        b.add_synth(rnd, rnd.randrange(20, 3000), _profile(i))
    w, lit = _exact(b, rnd, bm + 1)                # same place, one byte too long
    alt["long"] = (b.n, F.rec(w.finish(lit)[0]))
    w, lit = _exact(b, rnd, bm)
    b.add_writer(w, lit)
    b.add_synth(rnd, 200, _profile(3))
    alt["word"] = (b.n, F.rec(rnd.randbytes(bm + 1), stored=True))
    b.add_stored(rnd.randbytes(bm))
    b.add_synth(rnd, 1000, _profile(4))
    b.add_stored(rnd.randbytes(bm - 1))
    b.add_synth(rnd, 60, _profile(5))
    b.add_writer(b.writer(rnd), lit=65279)         # literals only: 1 + 256 + 65279 = blockMax record bytes
    assert len(b.recs[-1].payload) == bm
    b.add_synth(rnd, 500, _profile(6))
    b.add_directed(rnd, [1, 2, 3, 4, 5, 6], span=True)
    assert b.sizes[3] == b.sizes[5] == bm
    return b, alt


def _prestart():
    """Sources that begin before the frame's first byte (they read zeros): in block 0 and in a
    block below text position 65 535."""
    b = F.FrameBuilder(4)
    rnd = random.Random(4600)
    w = b.writer(rnd)
    w.seq(3, 4, 10)                                # one byte before the start, into its own literals
    w.seq(0, S.MAX_OFF, 20)
    w.seq(5, w.op + 5 + 200, 8)                    # wholly before the start
    b.add_writer(w)
    for i in range(4):
        b.add_synth(rnd, rnd.randrange(100, 3000), _profile(i))
    T = len(b.text)
    assert 0 < T < 60000
    w = b.writer(rnd)
    w.seq(2, T + 2 + 1, 40)                        # from one byte before the start into the text
    w.seq(0, T + w.op + 300, 19)
    w.seq(7, S.MAX_OFF, 130)
    b.add_writer(w)
    for i in range(4):
        b.add_synth(rnd, rnd.randrange(100, 3000), _profile(i + 4))
    return b


def _big(bid):
    """24 blocks, short and up to 80 KiB decoded, two of them stored."""
    b = F.FrameBuilder(bid)
    rnd = random.Random(4700 + bid)
    for i in range(24):
        if i in (7, 17):
            b.add_stored(rnd.randbytes(rnd.randrange(1, 70000)))
            continue
        prof = _profile(i)
        if i % 3 == 0:                             # the big ones: a class at P >= 16 384, every other one in runs
            prof["high"] = K.HIGHS[(i // 3) % len(K.HIGHS)]
            prof["kind"] = "runs" if i % 2 else "mixed"
        b.add_synth(rnd, K.BIG[(i // 3) % len(K.BIG)] if i % 3 == 0 else ([60] + K.SMALL)[i % 7], prof)
    return b


def _indep(which):
    rnd = random.Random(4800)
    batch = [x for x in K.synth_batch(0)[0] if x.plain is not None]
    if which == "indep600":
        b = F.FrameBuilder(4, linked=False)
        for i in range(600):
            if i % 7 == 6:
                b.add_stored(rnd.randbytes(rnd.randrange(12, 101)))
            else:
                b.add_synth(rnd, rnd.randrange(12, 101), "mixed")
        return b
    bid = 4 if which == "indep4" else 5
    b = F.FrameBuilder(bid, linked=False)
    small = [x for x in batch if len(x.plain) <= 65536]
    pick = small if bid == 4 else [x for x in batch if len(x.plain) > 65536] + small[:9]
    for i, x in enumerate(pick):
        if i % 7 == 6:
            b.add_stored(rnd.randbytes(rnd.randrange(1, 5000)))
        else:
            b.add_block(x.block, x.plain, stats=x.stats)
    return b


@functools.lru_cache(maxsize=None)
def stored0_accepted():
    """Whether the oracle reads a stored record of length 0 (size word 0x80000000)."""
    f = _span(True).frame(False, False)
    return oracle.decompress_frame(f.frame, F.contract_cap(f) + 65536) == (0, f.text)


@functools.lru_cache(maxsize=None)
def builder(name):
    if name in ("short", "lz4f"):
        return _short(name == "lz4f")
    if name == "sizes":
        return _sizes()[0]
    if name in ("b5", "b7"):
        return _big(int(name[1]))
    if name in INDEP:
        return _indep(name)
    if name == "span":
        return _span(stored0_accepted())
    return {"many": _many, "chain": _chain, "prestart": _prestart}[name]()


def _swap(b, i, r):
    recs = list(b.recs)
    recs[i] = r
    return recs


def _truncated(b, i):
    """Block i with the last byte of its last literal run missing."""
    assert not b.recs[i].stored and b.sizes[i] > 0
    return F.rec(b.recs[i].payload[:-1])


@functools.lru_cache(maxsize=None)
def cases(name):
    b = builder(name)
    out = [Case(f"{name}-SX", b.frame(True, True), OK, None), Case(f"{name}-sx", b.frame(False, False), OK, None)]
    if name == "many":
        hi, lo = MANY_HI, MANY_LO
        r = b.recs[hi]
        bad = F.rec(r.payload, r.stored, checksum=F.xxh32(r.payload) ^ 1)
        out.append(Case("many-SX-checksum-hi", b.frame(True, True, _swap(b, hi, bad)), BLOCK_CHECKSUM_MISMATCH, hi))
        both = _swap(b, hi, _truncated(b, hi))
        both[lo] = _truncated(b, lo)
        for bck in (True, False):
            tag = "SX" if bck else "sx"
            out.append(Case(f"many-{tag}-decode-hi", b.frame(bck, bck, _swap(b, hi, _truncated(b, hi))),
                            DECOMPRESS_FAIL, hi))
            out.append(Case(f"many-{tag}-decode-lo-hi", b.frame(bck, bck, both), DECOMPRESS_FAIL, lo))
    if name == "sizes":
        alt = _sizes()[1]
        for bck in (True, False):
            tag = "SX" if bck else "sx"
            i, r = alt["long"]
            out.append(Case(f"sizes-{tag}-long", b.frame(bck, bck, _swap(b, i, r)), DECOMPRESS_FAIL, i))
            j, rw = alt["word"]
            out.append(Case(f"sizes-{tag}-word", b.frame(bck, bck, _swap(b, j, rw)), INVALID_BLOCK_SIZE, j))
            # a block that fails before the bad size word: the reader stops there and never sees the word
            both = _swap(b, i, r)
            both[j] = rw
            out.append(Case(f"sizes-{tag}-long-word", b.frame(bck, bck, both), DECOMPRESS_FAIL, i))
        bad = F.rec(b.recs[1].payload, b.recs[1].stored, checksum=F.xxh32(b.recs[1].payload) ^ 1)
        both = _swap(b, j, rw)
        both[1] = bad
        out.append(Case("sizes-SX-checksum-word", b.frame(True, True, both), BLOCK_CHECKSUM_MISMATCH, 1))
    if name in INDEP:
        bad = [x for x in K.synth_batch(0)[0] if x.plain is None]
        mid = b.n // 2
        for k, bck in enumerate((True, False)):
            tag = "SX" if bck else "sx"
            out.append(Case(f"{name}-{tag}-invalid", b.frame(bck, bck, _swap(b, mid, F.rec(bad[k].block))),
                            DECOMPRESS_FAIL, mid))
    return tuple(out)


def case(label):
    """The case of that label (its recipe is the label's first word)."""
    return next(c for c in cases(label.split("-")[0]) if c.name == label)


def labels(names):
    return [c.name for n in names for c in cases(n)]


def expected(c):
    """(result code, bytes) of a case, from the builder alone."""
    return (0, c.frame.text) if c.fail is None else (c.code, F.text_before(c.frame, c.fail))


@functools.lru_cache(maxsize=None)
def damaged_short():
    """N_DAMAGED damaged copies of the "short" frame without checksums (a flipped literal still
    decodes there) and, every fourth, with them."""
    rnd = random.Random(4900)
    sx, SX = case("short-sx").frame.frame, case("short-SX").frame.frame
    out = F.damaged_frames(rnd, sx, N_DAMAGED, case("short-sx").frame.records)
    for k, d in zip(range(3, N_DAMAGED, 4), F.damaged_frames(rnd, SX, N_DAMAGED, case("short-SX").frame.records)):
        out[k] = d
    return tuple(out)


def damaged_cap(d):
    """One blockMax slot per record a reader finds in the damaged frame, and one to spare."""
    return (F.walk(d) + 1) * F.block_max(4)
