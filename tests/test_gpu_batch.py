"""Batched device-resident block operators (include/lz4mt_hip.h section 5:
lz4mtHipCompressBatch / lz4mtHipDecompressBatch, kernels k_encode_batch,
k_encode_batch16, k_decode_batch).

Everything is bit-exact against the CPU oracle (LZ4 1.9.3 restated) and the
liblz4 golden fixtures -- never against the library's other paths.  Inputs
are packed into one flat device tensor so that chunk starts cover every
offset mod 16 and the last chunk ends on the tensor's last byte; every
destination has 32 canary bytes after its capacity, checked after each call.
"""
import ctypes
import hashlib
import random

import numpy as np
import pytest
import torch
import xxhash

import oracle

pytestmark = pytest.mark.gpu

L = None
BAD = -(1 << 31)
CANARY = 32
FILL = 0xA5
KLIMIT = 65547   # LZ4_64Klimit: byU16 below, byU32 from here up


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = lz4mt_amd
    assert L.device_count() > 0
    return L


def bound(n):
    return n + n // 255 + 16


# ---------------------------------------------------------------------------
# helpers: packing, destinations with canaries, the raw C calls
# ---------------------------------------------------------------------------
def pack(datas):
    """One flat device tensor holding every chunk; chunk k starts at an
    offset = k (mod 16), gaps are 0xEE, and the last chunk ends on the
    tensor's last byte.  Returns (tensor, offsets)."""
    offs, o = [], 0
    for k, d in enumerate(datas):
        o += (k - o) % 16
        offs.append(o)
        o += len(d)
    buf = np.full(max(o, 1), 0xEE, dtype=np.uint8)
    for off, d in zip(offs, datas):
        if d:
            buf[off:off + len(d)] = np.frombuffer(d, dtype=np.uint8)
    assert {x % 16 for x in offs} == set(range(min(16, len(datas))))
    assert not datas or offs[-1] + len(datas[-1]) == o
    return torch.from_numpy(buf).cuda()[:o], offs


def i64(vals):
    return torch.tensor(list(vals), dtype=torch.int64, device="cuda")


def u32(vals):
    return torch.from_numpy(np.array(list(vals), dtype=np.uint32).view(np.int32)).cuda()


class Dst:
    """Destinations of one call: 16-byte-aligned slots of cap + 32 canary
    bytes in one backing tensor filled with FILL."""

    def __init__(self, caps):
        self.caps = list(caps)
        self.offs, o = [], 0
        for c in self.caps:
            self.offs.append(o)
            o += (c + CANARY + 15) & ~15
        self.back = torch.full((max(o, 16),), FILL, dtype=torch.uint8, device="cuda")
        assert self.back.data_ptr() % 16 == 0
        self.ptrs = [self.back.data_ptr() + x for x in self.offs]
        self.host = None

    def fetch(self):
        self.host = self.back.cpu().numpy()

    def data(self, i, n):
        return self.host[self.offs[i]:self.offs[i] + n].tobytes()

    def untouched_from(self, i, n):
        """slot i from byte n to the end of its canary is still FILL"""
        end = self.offs[i + 1] if i + 1 < len(self.offs) else len(self.host)
        return bool((self.host[self.offs[i] + n:end] == FILL).all())

    def canaries_ok(self):
        return all(self.untouched_from(i, c) for i, c in enumerate(self.caps))


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def compress_call(flat, soffs, sizes, caps, max_chunk, null_caps=False, dst=None, dst_ptrs=None):
    """One lz4mtHipCompressBatch; returns (sizes as a list, Dst fetched)."""
    dst = dst or Dst(caps)
    sp = i64([flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipCompressBatch(ctypes.c_void_p(sp.data_ptr()), ctypes.c_void_p(sz.data_ptr()), max_chunk,
                                    len(sizes), ctypes.c_void_p(dp.data_ptr()),
                                    ctypes.c_void_p(None if null_caps else cp.data_ptr()),
                                    ctypes.c_void_p(out.data_ptr()), stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def decompress_call(flat, soffs, sizes, caps, dst=None, dst_ptrs=None):
    dst = dst or Dst(caps)
    sp = i64([flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipDecompressBatch(ctypes.c_void_p(sp.data_ptr()), ctypes.c_void_p(sz.data_ptr()), len(sizes),
                                      ctypes.c_void_p(dp.data_ptr()), ctypes.c_void_p(cp.data_ptr()),
                                      ctypes.c_void_p(out.data_ptr()), stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def check_compressed(datas, caps, got, dst, tag):
    """sizes and bytes equal the oracle's for every chunk (0: does not fit)."""
    for i, (d, cap) in enumerate(zip(datas, caps)):
        want = oracle.compress_block(d, cap)
        assert got[i] == len(want), (tag, i, len(d), cap, got[i], len(want))
        assert dst.data(i, len(want)) == want, (tag, i, len(d), cap)
    assert dst.canaries_ok(), tag


# ---------------------------------------------------------------------------
# contents: the five kinds of test_block_compress_fuzz_vs_oracle
# ---------------------------------------------------------------------------
class Pools:
    def __init__(self, seed, n=1 << 19):
        r = np.random.RandomState(seed)
        self.rnd = random.Random(seed)
        self.n = n
        self.syn = oracle.gen_synthetic(n + 70000, seed)
        self.sym3 = r.randint(0, 3, n + 70000, dtype=np.uint8).tobytes()
        self.rand = oracle.gen_random(n + 70000, seed)

    def make(self, kind, n):
        a = self.rnd.randrange(self.n) if n <= 70000 else 0
        if kind == 0:
            return self.syn[a:a + n]
        if kind == 1:
            return self.sym3[a:a + n]
        if kind == 2:
            return self.rand[a:a + n]
        if kind == 3:
            p = self.rnd.randrange(1, 70)
            return (self.rand[a:a + p] * (n // p + 1))[:n]
        return bytes(n)


def mixed(n, seed):
    """test_gpu.py's _mixed: text, random runs, zero runs, repeats near and far."""
    rnd = random.Random(seed)
    syn = oracle.gen_synthetic(1 << 20, seed)
    out, size = [], 0
    while size < n:
        k = rnd.randrange(5)
        if k == 0:
            a = rnd.randrange(len(syn) - 5000)
            piece = syn[a:a + rnd.randrange(100, 5000)]
        elif k == 1:
            piece = oracle.gen_random(rnd.randrange(65, 700), rnd.randrange(1 << 30))
        elif k == 2:
            piece = bytes(rnd.randrange(1, 3000))
        elif k == 3 and out:
            prev = b"".join(out[-8:])
            a = rnd.randrange(len(prev))
            piece = prev[a:a + rnd.randrange(4, 2000)]
        else:
            piece = bytes([rnd.randrange(256)]) * rnd.randrange(1, 400)
        out.append(piece)
        size += len(piece)
    return b"".join(out)[:n]


RAGGED = [0, 1, 12, 13, 14, 64, 1000, 4095, 65535, 65546, 65547, 65548, 100_000, 262_144, (4 << 20) - 1, 4 << 20]


@pytest.fixture(scope="module")
def ragged():
    """(datas, flat device tensor, offsets) of the ragged batch; read-only."""
    pools = Pools(11)
    datas = [mixed(n, n) if n >= (4 << 20) - 1 else pools.make(i % 5, n) for i, n in enumerate(RAGGED)]
    assert [len(d) for d in datas] == RAGGED
    flat, offs = pack(datas)
    return datas, flat, offs


# ---------------------------------------------------------------------------
# 1. ragged compress through the mixed kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("capkind", ["n", "n-1", "bound", "half", "null"])
def test_ragged_compress_mixed_kernel(ragged, capkind):
    datas, flat, offs = ragged
    caps = [{"n": n, "n-1": max(n - 1, 0), "bound": bound(n), "half": n // 2, "null": bound(n)}[capkind]
            for n in RAGGED]
    got, dst = compress_call(flat, offs, RAGGED, caps, 4 << 20, null_caps=capkind == "null")
    check_compressed(datas, caps, got, dst, capkind)


# ---------------------------------------------------------------------------
# 2. the small-chunk kernel, and the mixed kernel on the same inputs
# ---------------------------------------------------------------------------
def test_small_chunk_kernel_and_mixed_kernel_agree_with_oracle():
    rnd = random.Random(77)
    pools = Pools(5)
    sizes = [rnd.choice([0, 1, 13, 64, 100, 4096, 4097, 65535, 65536]) for _ in range(1000)]
    datas = [pools.make(i % 5, n) for i, n in enumerate(sizes)]
    flat, offs = pack(datas)
    for capkind in ("n", "bound"):
        caps = [n if capkind == "n" else bound(n) for n in sizes]
        want = [oracle.compress_block(d, c) for d, c in zip(datas, caps)]
        for max_chunk in (65536, KLIMIT):   # k_encode_batch16, then k_encode_batch
            got, dst = compress_call(flat, offs, sizes, caps, max_chunk)
            assert got == [len(w) for w in want], (capkind, max_chunk)
            for i, w in enumerate(want):
                assert dst.data(i, len(w)) == w, (capkind, max_chunk, i, sizes[i])
            assert dst.canaries_ok(), (capkind, max_chunk)


# ---------------------------------------------------------------------------
# 3. many chunks: a grid larger than any frame test's
# ---------------------------------------------------------------------------
def test_many_small_chunks():
    n, k = 70_000, 64
    pools = Pools(9, 1 << 16)
    datas = [pools.make(i % 5, k) for i in range(n)]
    flat, offs = pack(datas)
    caps = [bound(k)] * n
    got, dst = compress_call(flat, offs, [k] * n, caps, k)
    want = [oracle.compress_block(d, caps[0]) for d in datas]
    assert got == [len(w) for w in want]
    for i, w in enumerate(want):
        assert dst.data(i, len(w)) == w, i
    assert dst.canaries_ok()
    # and back, 70 000 blocks in one decompress call
    wflat, woffs = pack(want)
    back, ddst = decompress_call(wflat, woffs, [len(w) for w in want], [k] * n)
    assert back == [k] * n
    for i, d in enumerate(datas):
        assert ddst.data(i, k) == d, i
    assert ddst.canaries_ok()


# ---------------------------------------------------------------------------
# 4. the liblz4 golden fixtures
# ---------------------------------------------------------------------------
def test_golden_blocks_compress(golden, golden_inputs):
    vs = golden["blocks"]
    datas = [golden_inputs[v["input"]][:v["n"]] for v in vs]
    caps = [v["cap"] for v in vs]
    flat, offs = pack(datas)
    got, dst = compress_call(flat, offs, [len(d) for d in datas], caps, 4 << 20)
    for i, v in enumerate(vs):
        assert got[i] == v["ret"], v
        assert hashlib.sha1(dst.data(i, v["ret"])).hexdigest() == v["sha1"], v
    assert dst.canaries_ok()


def test_golden_blocks_decompress(golden, decode_blob):
    vs = [(decode_blob[v["off"]:v["off"] + v["len"]], v) for v in golden["decode"]]
    vs += [(bytes.fromhex(v["block_hex"]), v) for v in golden["crafted"]]
    assert any(v["ret"] < 0 for _, v in vs) and any(v["ret"] > 0 for _, v in vs)
    blocks = [b for b, _ in vs]
    caps = [v["cap"] for _, v in vs]
    flat, offs = pack(blocks)
    got, dst = decompress_call(flat, offs, [len(b) for b in blocks], caps)
    for i, (_, v) in enumerate(vs):
        assert got[i] == v["ret"], v
        if v["ret"] >= 0:
            assert xxhash.xxh32(dst.data(i, v["ret"])).intdigest() == v["out_xxh32"], v
    assert dst.canaries_ok()


# ---------------------------------------------------------------------------
# 5. decompress fuzz: caps around the size, damaged blocks
# ---------------------------------------------------------------------------
def test_decompress_fuzz_vs_oracle(ragged):
    datas, _, _ = ragged
    good = [oracle.compress_block(d, bound(len(d))) for d in datas]
    rnd = random.Random(31)
    blocks, caps = [], []
    for d, b in zip(datas, good):
        for cap in (len(d), len(d) - 1, len(d) + 100, 0):
            if cap >= 0:
                blocks.append(b)
                caps.append(cap)
    for b, d in list(zip(good, datas))[3:13]:   # ten blocks, truncated and bit-flipped
        cut = bytes(b[:rnd.randrange(1, len(b))])
        flip = bytearray(b)
        for _ in range(rnd.randrange(1, 4)):
            flip[rnd.randrange(len(flip))] ^= 1 << rnd.randrange(8)
        for dmg in (cut, bytes(flip)):
            for cap in (len(d), len(d) + 100):
                blocks.append(dmg)
                caps.append(cap)
    flat, offs = pack(blocks)
    got, dst = decompress_call(flat, offs, [len(b) for b in blocks], caps)
    for i, (b, cap) in enumerate(zip(blocks, caps)):
        r, out = oracle.decompress_block(b, cap)
        assert got[i] == r, (i, len(b), cap, got[i], r)
        if r >= 0:
            assert dst.data(i, r) == out, (i, len(b), cap)
    assert dst.canaries_ok()


# ---------------------------------------------------------------------------
# 6. per-chunk rejection: misaligned, null, oversized; nothing faults
# ---------------------------------------------------------------------------
def test_per_chunk_rejection():
    pools = Pools(21)
    sizes = [100, 4096, 3000, 64, 5000, 0, 4095, 13]
    datas = [pools.make(i % 5, n) for i, n in enumerate(sizes)]
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    max_chunk = 4096
    mis, null, big = 1, 3, 4   # base + 8; a null destination; 5000 > maxChunkBytes
    dst = Dst(caps)
    ptrs = list(dst.ptrs)
    ptrs[mis] += 8
    ptrs[null] = 0
    got, dst = compress_call(flat, offs, sizes, caps, max_chunk, dst=dst, dst_ptrs=ptrs)
    for i, (d, cap) in enumerate(zip(datas, caps)):
        if i in (mis, null, big):
            assert got[i] == BAD, (i, got[i])
            assert dst.untouched_from(i, 0), i
        else:
            want = oracle.compress_block(d, cap)
            assert got[i] == len(want) and dst.data(i, len(want)) == want, i
    assert dst.canaries_ok()

    # the same through the decoder (no size promise there: two rejections)
    blocks = [oracle.compress_block(d, c) for d, c in zip(datas, caps)]
    bflat, boffs = pack(blocks)
    ddst = Dst(sizes)
    ptrs = list(ddst.ptrs)
    ptrs[mis] += 8
    ptrs[null] = 0
    got, ddst = decompress_call(bflat, boffs, [len(b) for b in blocks], sizes, dst=ddst, dst_ptrs=ptrs)
    for i, d in enumerate(datas):
        if i in (mis, null):
            assert got[i] == BAD, (i, got[i])
            assert ddst.untouched_from(i, 0), i
        else:
            assert got[i] == len(d) and ddst.data(i, len(d)) == d, i
    assert ddst.canaries_ok()


# ---------------------------------------------------------------------------
# 7. Python wrappers, interop with the oracle, a non-default stream
# ---------------------------------------------------------------------------
def test_python_wrappers_roundtrip_on_side_stream(ragged):
    datas, flat, offs = ragged
    pick = [i for i, n in enumerate(RAGGED) if n <= 262_144]
    chunks = [flat[offs[i]:offs[i] + RAGGED[i]] for i in pick]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    outs, sizes = L.compress_batch(chunks, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1   # one backing allocation
    s.synchronize()
    csz = sizes.cpu().tolist()
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for i, b, k in zip(pick, blocks, csz):
        assert k > 0
        # a batch-compressed chunk decodes with the oracle (and is its block)
        hb = bytes(b.cpu().numpy().tobytes())
        assert oracle.decompress_block(hb, RAGGED[i]) == (RAGGED[i], datas[i]), i
        assert hb == oracle.compress_block(datas[i], bound(RAGGED[i])), i
    back, dsz = L.decompress_batch(blocks, [RAGGED[i] for i in pick], stream=s)
    s.synchronize()
    assert dsz.cpu().tolist() == [RAGGED[i] for i in pick]
    for i, t in zip(pick, back):
        assert bytes(t.cpu().numpy().tobytes()) == datas[i], i
    # explicit capacities: what does not fit reports 0
    outs, sizes = L.compress_batch(chunks, caps=[c.numel() // 2 for c in chunks], stream=s)
    s.synchronize()
    assert sizes.cpu().tolist() == [len(oracle.compress_block(datas[i], RAGGED[i] // 2)) for i in pick]


def test_python_wrappers_empty_batch():
    outs, sizes = L.compress_batch([])
    assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    outs, sizes = L.decompress_batch([], [])
    assert outs == [] and sizes.numel() == 0
    # and the C calls: OK, nothing launched, null arrays allowed
    assert L.lib.lz4mtHipCompressBatch(None, None, 0, 0, None, None, None, stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDecompressBatch(None, None, 0, None, None, None, stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 8. both calls captured into one HIP graph, replayed on new bytes
# ---------------------------------------------------------------------------
def test_batch_calls_in_hip_graph():
    pools = Pools(41)
    sizes = [0, 1, 13, 100, 1000, 4096, 4097, 20000, 65535, 65546, 65547, 65548, 70000, 100_000, 150_000, 262_144]
    assert len(sizes) == 16

    def contents(shift):
        return [pools.make((i + shift) % 5, n) for i, n in enumerate(sizes)]

    datas = contents(0)
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    csz = torch.zeros(16, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(16, dtype=torch.int32, device="cuda")
    P = ctypes.c_void_p

    def call():
        st = stream_ptr()
        # one chain: the decode reads the encode's blocks and the sizes it wrote (device memory)
        assert L.lib.lz4mtHipCompressBatch(P(sp.data_ptr()), P(sz.data_ptr()), 262_144, 16, P(cp_.data_ptr()),
                                           P(cc.data_ptr()), P(csz.data_ptr()), st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatch(P(cp_.data_ptr()), P(csz.data_ptr()), 16, P(dp.data_ptr()),
                                             P(sz.data_ptr()), P(dsz.data_ptr()), st) == L.Result.OK

    def check(datas, tag):
        torch.cuda.synchronize()
        cdst.fetch()
        ddst.fetch()
        got, back = csz.cpu().tolist(), dsz.cpu().tolist()
        for i, d in enumerate(datas):
            want = oracle.compress_block(d, caps[i])
            assert got[i] == len(want) and cdst.data(i, len(want)) == want, (tag, i)
            assert back[i] == len(d) and ddst.data(i, len(d)) == d, (tag, i)
        assert cdst.canaries_ok() and ddst.canaries_ok(), tag

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the library outside the capture (the encoder-order check)
        call()
    check(datas, "warm")
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
        check(datas, f"replay {rep}")
