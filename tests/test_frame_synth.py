"""The frame builder (lz4_frame_synth.py) and the fixed frames of the GPU tests
(frame_synth_cases.py), checked on the CPU:

  1. the builder's header is the frame writers' for every flag set it uses
  2. the oracle decodes every valid frame to the builder's text (no decoder computed that
     text) and gives every failing variant its code and the text of the blocks before
  3. liblz4 1.9.3's LZ4F_decompress, where present, decodes the frames it can read
  4. the frames hold what they are meant to: every blocks-back class, sources that span blocks,
     lie in stored blocks, begin before the frame, run into the block's own output; more than
     one scan pass of blocks; batches that decode less than the 64 KiB window
"""
import collections
import ctypes
import os

import pytest

import frame_synth_cases as C
import lz4_frame_synth as F
import oracle
import synth_cases as K

LIBLZ4 = "/lib/x86_64-linux-gnu/liblz4.so.1"
ALL = C.LINKED + C.INDEP


# ---------------------------------------------------------------------------
# 1. header
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bid", [4, 5, 6, 7])
def test_header_is_the_frame_writers(bid):
    for bck in (False, True):
        for sck in (False, True):
            h = F.header(F.Params(bid, False, bck, sck))
            assert h == oracle.compress_frame(b"abc", oracle.params(bid, sck, bck))[:7], (bid, bck, sck)
            h = F.header(F.Params(bid, True, bck, sck))
            assert h == oracle.bd_hc_frame(b"abc", bid, sck, bck)[:7], (bid, bck, sck)
    used = {c.frame.params for n in ALL for c in C.cases(n)}
    assert {p.bid for p in used} == {4, 5, 7} and {p.linked for p in used} == {True, False}
    assert {(p.block_checksum, p.content_checksum) for p in used} == {(True, True), (False, False)}


def test_frame_layout():
    """Record offsets, sizes and starts of a frame with and without checksums."""
    for c in C.cases("span")[:2]:
        f = c.frame
        per = 8 if f.params.block_checksum else 4
        assert f.records[0] == 7 and len(f.records) == len(f.recs) + 1
        for i, r in enumerate(f.recs):
            assert f.records[i + 1] - f.records[i] == per + len(r.payload)
            word = int.from_bytes(f.frame[f.records[i]:f.records[i] + 4], "little")
            assert word == len(r.payload) | (F.RAW_BIT if r.stored else 0)
        assert f.frame[f.records[-1]:f.records[-1] + 4] == bytes(4)
        assert len(f.frame) == f.records[-1] + 4 + (4 if f.params.content_checksum else 0)
        assert sum(f.sizes) == len(f.text) and f.starts == [sum(f.sizes[:i]) for i in range(len(f.sizes))]
        assert F.walk(f.frame) == len(f.recs)


# ---------------------------------------------------------------------------
# 2. the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_oracle_on_every_frame(name):
    cs = C.cases(name)
    assert [c.code for c in cs[:2]] == [0, 0]
    for c in cs:
        f = c.frame
        want = C.expected(c)
        if c.fail is not None:
            assert c.code != 0 and want[1] == b"".join(
                f.text[s:s + n] for s, n in zip(f.starts[:c.fail], f.sizes[:c.fail])), c.name
        assert oracle.decompress_frame(f.frame, F.contract_cap(f)) == want, c.name


def test_variants_are_the_ones_asked_for():
    assert [c.name.split("-", 1)[1] for c in C.cases("many")[2:]] == [
        "SX-checksum-hi", "SX-decode-hi", "SX-decode-lo-hi", "sx-decode-hi", "sx-decode-lo-hi"]
    assert [(c.code, c.fail) for c in C.cases("many")[2:]] == [
        (16, C.MANY_HI), (18, C.MANY_HI), (18, C.MANY_LO), (18, C.MANY_HI), (18, C.MANY_LO)]
    assert C.MANY_LO < 1024 < C.MANY_HI < C.MANY_BLOCKS
    b = C.builder("many")
    assert b.n == C.MANY_BLOCKS >= 1100
    lo_hi = C.case("many-sx-decode-lo-hi").frame       # both blocks fail there: the lower one wins
    assert lo_hi.recs[C.MANY_LO] != b.recs[C.MANY_LO] and lo_hi.recs[C.MANY_HI] != b.recs[C.MANY_HI]
    assert [(c.name.split("-", 2)[2], c.code, c.fail) for c in C.cases("sizes")[2:]] == [
        ("long", 18, 3), ("word", 20, 5), ("long-word", 18, 3)] * 2 + [("checksum-word", 16, 1)]
    assert C.builder("sizes").sizes[3] == C.builder("sizes").sizes[5] == 65536
    word = C.case("sizes-sx-word").frame
    at = word.records[5]
    assert int.from_bytes(word.frame[at:at + 4], "little") == F.RAW_BIT | 65537
    for n in C.INDEP:
        assert [(c.code, c.fail) for c in C.cases(n)[2:]] == [(18, C.builder(n).n // 2)] * 2


def test_a_failing_block_comes_before_a_later_read_error():
    """decompressBlockDependency handles each block as it reads it, so a block that fails its
    checksum or its decode ends the frame before the reader meets a later size word above
    blockMax or the end of the bytes: the block's code is the result, not the reader's."""
    for label, code in [("sizes-sx-long-word", 18), ("sizes-SX-long-word", 18), ("sizes-SX-checksum-word", 16)]:
        c = C.case(label)
        cap = F.contract_cap(c.frame)
        assert oracle.decompress_frame(c.frame.frame, cap) == (code, F.text_before(c.frame, c.fail)), label
        cut = c.frame.frame[:c.frame.records[c.fail + 1] + 2]       # ... or half of the next size word
        assert oracle.decompress_frame(cut, cap) == (code, F.text_before(c.frame, c.fail)), label
    c = C.case("sizes-sx-word")                                     # with no block failing, the reader's code
    assert oracle.decompress_frame(c.frame.frame, F.contract_cap(c.frame))[0] == 20
    cut = c.frame.frame[:c.frame.records[3] + 2]
    assert oracle.decompress_frame(cut, F.contract_cap(c.frame)) == (12, F.text_before(c.frame, 3))


def test_stored_record_of_length_zero_is_read():
    """The size word 0x80000000 is a stored block of no bytes, not the end mark: the oracle (the
    reference's read loop tests the whole word against 0) goes on past it."""
    assert C.stored0_accepted()
    f = C.case("span-sx").frame
    empty = [i for i, n in enumerate(f.sizes) if n == 0]
    assert [f.recs[i].stored for i in empty] == [False, True] and f.recs[empty[0]].payload == b"\x00"
    at = f.records[empty[1]]
    assert f.frame[at:at + 4] == (F.RAW_BIT).to_bytes(4, "little")


# ---------------------------------------------------------------------------
# 3. liblz4's frame decoder
# ---------------------------------------------------------------------------
def _lz4f():
    if not os.path.exists(LIBLZ4):
        pytest.skip("liblz4 not present")
    lz = ctypes.CDLL(LIBLZ4)
    if lz.LZ4_versionNumber() != 10903:
        pytest.skip("liblz4 is not 1.9.3")
    sz = ctypes.c_size_t
    lz.LZ4F_createDecompressionContext.restype = sz
    lz.LZ4F_createDecompressionContext.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    lz.LZ4F_freeDecompressionContext.argtypes = [ctypes.c_void_p]
    lz.LZ4F_decompress.restype = sz
    lz.LZ4F_decompress.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(sz), ctypes.c_void_p,
                                   ctypes.POINTER(sz), ctypes.c_void_p]
    lz.LZ4F_isError.argtypes = [sz]
    return lz


def lz4f_decompress(lz, frame, cap):
    """(ok, bytes): LZ4F_decompress over the whole frame, fed in pieces of 100 000 bytes."""
    ctx = ctypes.c_void_p()
    assert not lz.LZ4F_isError(lz.LZ4F_createDecompressionContext(ctypes.byref(ctx), 100))
    src = ctypes.create_string_buffer(frame, len(frame))
    dst = ctypes.create_string_buffer(cap + 1)
    ip = op = 0
    hint = 1
    try:
        while ip < len(frame) and hint:
            n_in, n_out = ctypes.c_size_t(min(len(frame) - ip, 100000)), ctypes.c_size_t(cap + 1 - op)
            hint = lz.LZ4F_decompress(ctx, ctypes.byref(dst, op), ctypes.byref(n_out), ctypes.byref(src, ip),
                                      ctypes.byref(n_in), None)
            if lz.LZ4F_isError(hint):
                return False, dst.raw[:op]
            ip += n_in.value
            op += n_out.value
        return hint == 0 and ip == len(frame), dst.raw[:op]
    finally:
        lz.LZ4F_freeDecompressionContext(ctx)


@pytest.mark.parametrize("name", ["lz4f"] + C.INDEP)
def test_liblz4_decodes_the_frames_it_can_read(name):
    lz = _lz4f()
    for c in C.cases(name)[:2]:
        assert lz4f_decompress(lz, c.frame.frame, len(c.frame.text)) == (True, c.frame.text), c.name
    for c in C.cases(name)[2:]:
        ok, out = lz4f_decompress(lz, c.frame.frame, len(c.frame.text))
        assert not ok and out == C.expected(c)[1][:len(out)], c.name


def test_liblz4_refuses_sources_before_the_frame():
    """What sets the "lz4f" recipe apart: liblz4 reads no zeros before the frame's first byte."""
    lz = _lz4f()
    c = C.case("prestart-sx")
    assert not lz4f_decompress(lz, c.frame.frame, len(c.frame.text))[0]


# ---------------------------------------------------------------------------
# 4. conditions on the inputs
# ---------------------------------------------------------------------------
BACKS = [1, 2, "3..9", "10+"]


@pytest.mark.parametrize("name", ["short", "many", "lz4f"])
def test_short_blocks_hold_every_source_class(name):
    st = C.builder(name).stats
    assert all(st[("back", k)] >= 1 for k in BACKS), name
    assert st["span2"] >= 1 and st["stored_src"] >= 1 and st["hist_to_own"] >= 1, name
    assert st[("blocks", "stored")] == C.builder(name).n // 7
    assert (st["prestart"] == 0) == (name == "lz4f")


def test_block_counts_and_sizes():
    short, many, chain = (C.builder(n) for n in ("short", "many", "chain"))
    assert short.n == C.SHORT_BLOCKS == 300 and chain.n == C.CHAIN_BLOCKS == 200
    assert many.n >= 1100 and many.n > 1024 + 100
    # "many": the small targets; a directed block with spanning matches is longer
    assert sorted(many.sizes)[many.n // 2] < 300 and max(many.sizes) < 16384
    assert min(short.sizes) < 200 and max(short.sizes) < 65536
    assert all(70 <= n <= 300 for n in chain.sizes)
    for name in ("b5", "b7"):
        b = C.builder(name)
        assert b.n == 24 and b.stats[("blocks", "stored")] == 2
        assert min(b.sizes) < 400 and 80000 < max(b.sizes) < 90000
    assert len({F.block_max(C.builder(n).bid) for n in ("short", "b5", "b7")}) == 3


def carried_reads(b, per=16):
    """The matches of batch k (``per`` blocks) whose source starts before batch k - 1 while that
    batch decodes less than the window: their bytes reach batch k only through the history the
    engine carries over two calls (k_dlink_hist_out below position 0).  Sources before the
    frame's first byte are left out: they read zeros whatever is carried."""
    n = 0
    for i, G, _ in b.sources:
        k = i // per
        if k >= 2 and sum(b.sizes[(k - 1) * per:k * per]) < F.WINDOW and 0 <= G < b.starts[(k - 1) * per]:
            n += 1
    return n


def test_batches_of_sixteen_blocks_decode_less_than_the_window():
    """With 1 MiB batches of 64 KiB blocks the callback engine decodes 16 blocks per call; the
    history it carries on is then old and new bytes mixed, and matches read the old ones."""
    for name in C.SHORT_BATCHES:
        b = C.builder(name)
        sums = [sum(b.sizes[i:i + 16]) for i in range(0, b.n, 16)]
        below = sum(s < F.WINDOW for s in sums)
        assert len(sums) >= 13 and below >= (len(sums) // 2 if name == "short" else len(sums)), (name, below)
    assert carried_reads(C.builder("short")) >= 20 and carried_reads(C.builder("many")) >= 20


def test_chain_copies_the_previous_block_in_every_block():
    b = C.builder("chain")
    assert all(bs[("back", 1)] == 1 for bs in b.block_stats[1:])
    # and from block 2 on a second match that starts two to five blocks back
    assert all(bs[("back", 2)] + bs[("back", "3..9")] == 1 for bs in b.block_stats[2:])
    f = C.case("chain-sx").frame
    for i in range(1, b.n):          # the match is the block's first sequence, its offset the previous block's length
        p = f.records[i] + 4
        assert f.frame[p] >> 4 == 0 and int.from_bytes(f.frame[p + 1:p + 3], "little") == f.sizes[i - 1]
    assert all(f.text[f.starts[i]:f.starts[i] + 60] == f.text[:60] for i in range(b.n))


def test_span_and_sizes_and_prestart_hold_their_cases():
    sp = C.builder("span")
    assert sp.stats[("blocks", "zero")] == 2 and sp.stats["hist_to_own"] == 3 and sp.stats["span2"] == 3
    assert sp.stats[("back", "3..9")] == 2 and sp.stats[("back", "10+")] == 1
    assert sorted(set(sp.sizes)) == [0, 50] + sorted(n for n in set(sp.sizes) if n > 275)
    sz = C.builder("sizes")
    assert sz.sizes.count(65536) == 2 and 65535 in sz.sizes and 65279 in sz.sizes and min(sz.sizes) < 400
    assert [r.stored for r, n in zip(sz.recs, sz.sizes) if n == 65536] == [False, True]
    assert [len(r.payload) for r in sz.recs].count(65536) == 2      # the stored one and the literal-only one
    pre = C.builder("prestart")
    assert pre.block_stats[0]["prestart"] >= 3 and pre.block_stats[5]["prestart"] >= 3
    assert 0 < pre.starts[5] < 65535 and pre.stats["prestart"] >= 2
    assert C.builder("lz4f").stats["prestart"] == 0


def test_block_classes_of_the_synthesizer_occur():
    total = collections.Counter(C.builder("short").stats)
    total.update(C.builder("b5").stats)
    missing = [k for k in K.required_classes(65536) if total[k] < 1]
    assert not missing, missing


def test_independent_frames():
    valid = [x for x in K.synth_batch(0)[0] if x.plain is not None]
    i4, i5, i600 = (C.builder(n) for n in C.INDEP)
    assert i4.n == sum(len(x.plain) <= 65536 for x in valid) and max(i4.sizes) <= 65536
    assert sum(n > 65536 for n in i5.sizes) == sum(len(x.plain) > 65536 for x in valid) >= 2
    assert i600.n == 600 and sorted(i600.sizes)[300] < 300
    for b in (i4, i5, i600):
        assert b.stats[("blocks", "stored")] == b.n // 7
    f = C.case("indep600-sx").frame
    gaps = [b - a for a, b in zip(f.records, f.records[1:])]
    assert min(gaps) < 24 and sorted(gaps)[300] < 200


def test_damaged_frames_are_neither_all_read_nor_all_refused():
    ds = C.damaged_short()
    assert len(ds) == C.N_DAMAGED == 40 and len(set(ds)) == 40
    codes = [oracle.decompress_frame(d, C.damaged_cap(d))[0] for d in ds]
    assert codes.count(0) >= 5 and sum(c != 0 for c in codes) >= 5
    assert len(set(codes)) >= 4, sorted(set(codes))
    valid = C.case("short-sx").frame
    changed = [d for d, c in zip(ds, codes) if c == 0 and oracle.decompress_frame(d, C.damaged_cap(d))[1] != valid.text]
    assert len(changed) >= 3      # read, but to other bytes
