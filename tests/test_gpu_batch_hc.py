"""Batched LZ4-HC on device memory (include/lz4mt_hip.h section 5:
lz4mtHipCompressBatchEx / lz4mtHipCompressBatchWorkspaceSize at level >= 3;
kernels k_hc_prev_batch, k_encode_hc_batch, k_encode_hc_opt_batch).

Everything is bit-exact against the CPU oracle (lz4 1.9.3's
LZ4_compressHC2_limitedOutput restated; LZ4_compress_limitedOutput below
level 3) and the liblz4 golden fixtures -- never against the library's other
paths.  The methods are test_gpu_batch.py's: inputs packed into one flat
device tensor so that chunk starts cover every offset mod 16 and the last
chunk ends on the tensor's last byte; every destination has 32 canary bytes
after its capacity, checked after each call.  One wave parses one chunk, so
chunks stay at or below 300 000 bytes (200 000 from level 10 up, the golden
fixtures apart).
"""
import ctypes
import hashlib
import random

import pytest
import torch

import oracle
from conftest import bd_input
from test_gpu_batch import BAD, FILL, Dst, bound, i64, pack, stream_ptr, u32
from test_gpu_hc import _mixed

pytestmark = pytest.mark.gpu

L = None
P = ctypes.c_void_p


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = lz4mt_amd
    assert L.device_count() > 0
    return L


def slot_bytes(max_chunk, level):
    return L.lib.lz4mtHipCompressBatchWorkspaceSize(max_chunk, 1, level)


def workspace(nbytes):
    """exactly nbytes of 256-byte-aligned device scratch, filled with 0xFF:
    stale-looking chain links and prices wherever the kernels do not write"""
    w = torch.full((max(nbytes, 1),), 0xFF, dtype=torch.uint8, device="cuda")
    assert w.data_ptr() % 256 == 0
    return w[:nbytes]


def ex_call(flat, soffs, sizes, caps, max_chunk, level, null_caps=False, dst=None, dst_ptrs=None, src_ptrs=None,
            ws="full"):
    """One lz4mtHipCompressBatchEx; returns (sizes as a list, Dst fetched).
    ws: "full" (lz4mtHipCompressBatchWorkspaceSize of the batch), a number of
    slots, or None (a NULL workspace)."""
    dst = dst or Dst(caps)
    sp = i64(src_ptrs if src_ptrs is not None else [flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    if ws is None:
        w, wp, wn = None, None, 0
    else:
        wn = (L.lib.lz4mtHipCompressBatchWorkspaceSize(max_chunk, len(sizes), level) if ws == "full"
              else ws * slot_bytes(max_chunk, level))
        w = workspace(wn)
        wp = w.data_ptr()
    r = L.lib.lz4mtHipCompressBatchEx(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes), P(dp.data_ptr()),
                                      P(None if null_caps else cp.data_ptr()), P(out.data_ptr()), level, P(wp), wn,
                                      stream_ptr())
    assert r == L.Result.OK, r
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def want_block(d, cap, level):
    return oracle.compress_block_hc(d, cap, level) if level >= 3 else oracle.compress_block(d, cap)


def check(datas, caps, level, got, dst, tag, skip=()):
    for i, (d, cap) in enumerate(zip(datas, caps)):
        if i in skip:
            continue
        want = want_block(d, cap, level)
        assert got[i] == len(want), (tag, i, len(d), cap, got[i], len(want))
        assert dst.data(i, len(want)) == want, (tag, i, len(d), cap)
    assert dst.canaries_ok(), tag


# ---------------------------------------------------------------------------
# 1. the liblz4 golden fixtures: one call per level
# ---------------------------------------------------------------------------
def test_golden_hc_blocks(golden, golden_inputs):
    inputs = dict(golden_inputs)
    inputs["bdmix300k"] = bd_input(300_000, 31)
    levels = sorted({v["level"] for v in golden["hc_blocks"]})
    assert levels and min(levels) >= 3 and any(x >= 10 for x in levels) and any(x <= 9 for x in levels)
    for level in levels:
        vs = [v for v in golden["hc_blocks"] if v["level"] == level]
        datas = [inputs[v["input"]][:v["n"]] for v in vs]
        caps = [v["cap"] for v in vs]
        flat, offs = pack(datas)
        got, dst = ex_call(flat, offs, [len(d) for d in datas], caps, max(len(d) for d in datas), level)
        for i, v in enumerate(vs):
            assert got[i] == v["ret"], v
            assert hashlib.sha1(dst.data(i, v["ret"])).hexdigest() == v["sha1"], v
        assert dst.canaries_ok(), level


# ---------------------------------------------------------------------------
# 2. a ragged batch against the oracle
# ---------------------------------------------------------------------------
RAGGED = [0, 1, 4, 11, 12, 13, 14, 64, 1000, 4095, 65535, 65536, 65547, 100_000, 300_000]


class Ragged:
    """The ragged batch, read-only: every chunk, and (levels 10 and up) the
    same without the 300 000-byte one, each packed on its own so that both
    end on their tensor's last byte."""

    def __init__(self):
        self.datas = [_mixed(n, 1000 + i) for i, n in enumerate(RAGGED)]
        assert [len(d) for d in self.datas] == RAGGED
        self.flat, self.offs = pack(self.datas)
        self.flat_opt, self.offs_opt = pack(self.datas[:-1])

    def at(self, level):
        if level >= 10:
            return self.datas[:-1], RAGGED[:-1], self.flat_opt, self.offs_opt
        return self.datas, RAGGED, self.flat, self.offs


@pytest.fixture(scope="module")
def ragged():
    return Ragged()


@pytest.mark.parametrize("capkind", ["n", "n-1", "third", "bound", "null"])
@pytest.mark.parametrize("level", [3, 9, 10, 12])
def test_ragged_batch_vs_oracle(ragged, level, capkind):
    datas, sizes, flat, offs = ragged.at(level)
    assert (300_000 in sizes) == (level < 10)
    caps = [{"n": n, "n-1": max(n - 1, 0), "third": n // 3, "bound": bound(n), "null": bound(n)}[capkind]
            for n in sizes]
    got, dst = ex_call(flat, offs, sizes, caps, max(sizes), level, null_caps=capkind == "null")
    check(datas, caps, level, got, dst, (level, capkind))


# ---------------------------------------------------------------------------
# 3. rounds: a slot serves several chunks of one call, long after short
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alternating():
    rnd = random.Random(5)
    sizes = [rnd.randrange(20_000, 60_000) if i % 2 == 0 else rnd.randrange(0, 600) for i in range(20)]
    sizes[3], sizes[7], sizes[11] = 0, 3, 13   # a slot's user that writes no chain entry, then one that writes few
    datas = [_mixed(n, 2000 + i) for i, n in enumerate(sizes)]
    flat, offs = pack(datas)
    return sizes, datas, flat, offs


@pytest.mark.parametrize("slots", [1, 3, "full"])
@pytest.mark.parametrize("level", [9, 12])
def test_rounds_and_slot_reuse(alternating, level, slots):
    sizes, datas, flat, offs = alternating
    caps = [bound(n) if i % 3 else n for i, n in enumerate(sizes)]
    got, dst = ex_call(flat, offs, sizes, caps, max(sizes), level, ws=slots)
    check(datas, caps, level, got, dst, (level, slots))


# ---------------------------------------------------------------------------
# 4. many small chunks: more workgroups than the device holds at once
# ---------------------------------------------------------------------------
def test_many_small_chunks_level_3():
    rnd = random.Random(9)
    pool = _mixed(1 << 20, 77)
    sizes = [rnd.randrange(64, 4097) for _ in range(5000)]
    sizes[0], sizes[1] = 64, 4096
    datas = []
    for n in sizes:
        a = rnd.randrange(len(pool) - n)
        datas.append(pool[a:a + n])
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    got, dst = ex_call(flat, offs, sizes, caps, 4096, 3)
    want = [oracle.compress_block_hc(d, c, 3) for d, c in zip(datas, caps)]
    assert got == [len(w) for w in want]
    for i, w in enumerate(want):
        assert dst.data(i, len(w)) == w, (i, sizes[i])
    assert dst.canaries_ok()


# ---------------------------------------------------------------------------
# 5. per-chunk rejection at level 9
# ---------------------------------------------------------------------------
def test_per_chunk_rejection_level_9():
    sizes = [100, 4096, 3000, 64, 5000, 0, 4095, 13, 700, 0]
    datas = [_mixed(n, 3000 + i) for i, n in enumerate(sizes)]
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    max_chunk = 4096
    mis, null, big, nosrc, empty_nosrc = 1, 3, 4, 8, 9
    dst = Dst(caps)
    ptrs = list(dst.ptrs)
    ptrs[mis] += 8          # a misaligned destination
    ptrs[null] = 0          # a null destination
    sptrs = [flat.data_ptr() + o for o in offs]
    sptrs[nosrc] = 0        # a null source with a non-zero size
    sptrs[empty_nosrc] = 0  # ... and with size 0: valid, the one-token block
    got, dst = ex_call(flat, offs, sizes, caps, max_chunk, 9, dst=dst, dst_ptrs=ptrs, src_ptrs=sptrs, ws=3)
    bad = (mis, null, big, nosrc)   # 5000 > maxChunkBytes
    for i in bad:
        assert got[i] == BAD, (i, got[i])
        assert dst.untouched_from(i, 0), i
    check(datas, caps, 9, got, dst, "rejection", skip=bad)
    assert got[empty_nosrc] == 1 and dst.data(empty_nosrc, 1) == b"\0"


# ---------------------------------------------------------------------------
# 6. levels: above 12 = 12; below 3 = the fast codec, no workspace
# ---------------------------------------------------------------------------
def test_level_handling(ragged):
    datas, sizes, flat, offs = ragged.at(17)
    caps = list(sizes)
    got, dst = ex_call(flat, offs, sizes, caps, max(sizes), 17)
    check(datas, caps, 17, got, dst, 17)
    for d, c in zip(datas, caps):   # (the oracle clamps as lz4hc does)
        assert oracle.compress_block_hc(d, c, 17) == oracle.compress_block_hc(d, c, 12)
    for level in (0, 2):
        for null_caps in (False, True):
            cc = [bound(n) for n in sizes] if null_caps else caps
            got, dst = ex_call(flat, offs, sizes, cc, max(sizes), level, null_caps=null_caps, ws=None)
            check(datas, cc, level, got, dst, (level, null_caps))


# ---------------------------------------------------------------------------
# 7. the Ex call and the decode captured into one HIP graph
# ---------------------------------------------------------------------------
def test_hc_batch_in_hip_graph():
    sizes = [0, 1, 13, 100, 1000, 4096, 4097, 20000, 65535, 65547, 70000, 30000]
    n = len(sizes)

    def contents(shift):
        return [_mixed(k, 4000 + 100 * shift + i) for i, k in enumerate(sizes)]

    datas = contents(0)
    flat, offs = pack(datas)
    caps = [bound(k) for k in sizes]
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")
    ws = workspace(5 * slot_bytes(max(sizes), 9))   # 5 slots for 12 chunks: three rounds inside the graph

    def call():
        st = stream_ptr()
        assert L.lib.lz4mtHipCompressBatchEx(P(sp.data_ptr()), P(sz.data_ptr()), max(sizes), n, P(cp_.data_ptr()),
                                             P(cc.data_ptr()), P(csz.data_ptr()), 9, P(ws.data_ptr()), ws.numel(),
                                             st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatch(P(cp_.data_ptr()), P(csz.data_ptr()), n, P(dp.data_ptr()),
                                             P(sz.data_ptr()), P(dsz.data_ptr()), st) == L.Result.OK

    def verify(datas, tag):
        torch.cuda.synchronize()
        cdst.fetch()
        ddst.fetch()
        got, back = csz.cpu().tolist(), dsz.cpu().tolist()
        for i, d in enumerate(datas):
            want = oracle.compress_block_hc(d, caps[i], 9)
            assert got[i] == len(want) and cdst.data(i, len(want)) == want, (tag, i)
            assert back[i] == len(d) and ddst.data(i, len(d)) == d, (tag, i)
        assert cdst.canaries_ok() and ddst.canaries_ok(), tag

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    verify(datas, "warm")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for rep in (1, 2):
        datas = contents(rep)
        new, offs2 = pack(datas)
        assert offs2 == offs
        flat.copy_(new)
        cdst.back.fill_(FILL)
        ddst.back.fill_(FILL)
        csz.zero_()
        dsz.zero_()
        g.replay()
        verify(datas, f"replay {rep}")


# ---------------------------------------------------------------------------
# 8. the Python wrapper on a side stream
# ---------------------------------------------------------------------------
def test_python_wrapper_level_9_on_side_stream(ragged):
    datas, _, flat, offs = ragged.at(12)
    pick = list(range(len(datas)))
    chunks = [flat[offs[i]:offs[i] + RAGGED[i]] for i in pick]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs, sizes = L.compress_batch(chunks, level=9, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    s.synchronize()
    csz = sizes.cpu().tolist()
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for i, b, k in zip(pick, blocks, csz):
        want = oracle.compress_block_hc(datas[i], bound(RAGGED[i]), 9)
        assert k == len(want) and bytes(b.cpu().numpy().tobytes()) == want, i
    back, dsz = L.decompress_batch(blocks, [RAGGED[i] for i in pick], stream=s)
    s.synchronize()
    assert dsz.cpu().tolist() == [RAGGED[i] for i in pick]
    for i, t in zip(pick, back):
        assert bytes(t.cpu().numpy().tobytes()) == datas[i], i
    # explicit capacities and a caller's workspace of two slots, at level 12
    ws = L.batch_compress_workspace(100_000, 2, 12)
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.numel() == 2 * slot_bytes(100_000, 12)
    outs, sizes = L.compress_batch(chunks, caps=[c.numel() // 3 for c in chunks], stream=s, level=12, workspace=ws)
    s.synchronize()
    assert sizes.cpu().tolist() == [len(oracle.compress_block_hc(datas[i], RAGGED[i] // 3, 12)) for i in pick]


def test_python_wrapper_empty_batch():
    for level in (0, 9, 12):
        outs, sizes = L.compress_batch([], level=level)
        assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    assert L.batch_compress_workspace(65536, 0, 9).numel() == 0
    assert L.batch_compress_workspace(65536, 5, 2).numel() == 0
    # and the C call: OK, nothing launched, null arrays and no workspace allowed
    assert L.lib.lz4mtHipCompressBatchEx(None, None, 0, 0, None, None, None, 9, None, 0, stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipCompressBatchEx(None, None, 0, 0, None, None, None, 0, None, 0, stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
