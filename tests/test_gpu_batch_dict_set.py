"""Batched block operators with a set of dictionaries and an index per chunk
(include/lz4mt_hip.h section 5d: lz4mtHipDictSetPrepare,
lz4mtHipCompressBatchDictSet, lz4mtHipDecompressBatchDictSet; kernels
k_dict_set_prepare, k_encode_batch_dict<XC, DictSet>, k_decode_batch_dict_set).

The references are liblz4 1.9.3 through the committed fixture
tests/golden/dict_blocks.json -- all its dictionaries in ONE call each way --
and the CPU oracle's restatement of both dictionary operations
(oracle.compress_block_dict / decompress_block_dict), never the library's
other paths.  Inputs are packed as test_gpu_batch.py packs them (chunk starts
at every offset mod 16, 32 canary bytes after every capacity); every
dictionary tensor starts at an odd address and ends on its tensor's last byte.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import dict_cases as C
import oracle
import test_gpu_batch as B
import test_gpu_batch_dict as BD
from conftest import GOLDEN
from test_gpu_batch import BAD, FILL, Dst, bound, i64, pack, stream_ptr, u32
from test_gpu_batch_dict import dict_tensor, sha1

pytestmark = pytest.mark.gpu

L = None
P = ctypes.c_void_p
NO_DICT = 0xFFFFFFFF
with open(os.path.join(GOLDEN, "dict_blocks.json")) as _f:
    FX = json.load(_f)


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = B.L = BD.L = lz4mt_amd   # the helpers of those modules call the library through their module's handle
    assert L.device_count() > 0 and L.BATCH_NO_DICT == NO_DICT
    return L


@pytest.fixture(params=["exchange", "readback"])
def probe(request, monkeypatch):
    """Both encoder instantiations (XC): the LDS-exchange probe and the read-back one."""
    if request.param == "readback":
        monkeypatch.setenv("LZ4MT_AMD_ENC_PROBE", "readback")
        assert L.lib.lz4mtHipEncoderProbe() == 0
        yield request.param
        monkeypatch.delenv("LZ4MT_AMD_ENC_PROBE")
    else:
        yield request.param
    assert L.lib.lz4mtHipEncoderProbe() == 1


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def state_size():
    return L.lib.lz4mtHipDictStateSize()


class DictSet:
    """The device arrays of a set: a tensor per dictionary, d_dictPtrs, d_dictSizes."""

    def __init__(self, dicts):
        self.tensors = [dict_tensor(d) for d in dicts]
        self.k = len(dicts)
        self.ptr_list = [t.data_ptr() if t.numel() else 0 for t in self.tensors]
        self.size_list = [t.numel() for t in self.tensors]
        self.upload()

    def upload(self):
        self.ptrs, self.sizes = i64(self.ptr_list), u32(self.size_list)

    def args(self):
        return P(self.ptrs.data_ptr() if self.k else None), P(self.sizes.data_ptr() if self.k else None), self.k

    def new_states(self):
        st = torch.full((max(self.k * state_size(), 256),), 0xCC, dtype=torch.uint8, device="cuda")
        assert st.data_ptr() % 256 == 0
        return st

    def prepare(self, states=None):
        states = self.new_states() if states is None else states
        assert L.lib.lz4mtHipDictSetPrepare(*self.args(), P(states.data_ptr()), states.numel(),
                                            stream_ptr()) == L.Result.OK
        return states


def set_compress(flat, soffs, sizes, caps, max_chunk, ds, states, which, null_caps=False):
    dst = Dst(caps)
    sp, dp = i64([flat.data_ptr() + o for o in soffs]), i64(dst.ptrs)
    sz, cp, wh = u32(sizes), u32(caps), u32(which)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipCompressBatchDictSet(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes),
                                           P(dp.data_ptr()), P(None if null_caps else cp.data_ptr()),
                                           P(out.data_ptr()), *ds.args(),
                                           P(states.data_ptr() if states is not None else None), P(wh.data_ptr()),
                                           stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def set_decompress(flat, soffs, sizes, caps, ds, which):
    dst = Dst(caps)
    sp, dp = i64([flat.data_ptr() + o for o in soffs]), i64(dst.ptrs)
    sz, cp, wh = u32(sizes), u32(caps), u32(which)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipDecompressBatchDictSet(P(sp.data_ptr()), P(sz.data_ptr()), len(sizes), P(dp.data_ptr()),
                                             P(cp.data_ptr()), P(out.data_ptr()), *ds.args(), P(wh.data_ptr()),
                                             stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def interleave(groups):
    """[(group, item)] of every item of every group, ordered so that no two neighbours come from the
    same group: always the fullest group other than the last one taken."""
    left = [list(reversed(g)) for g in groups]
    out, last = [], -1
    while any(left):
        k = max((i for i in range(len(left)) if left[i] and i != last), key=lambda i: len(left[i]))
        out.append((k, left[k].pop()))
        last = k
    assert all(a[0] != b[0] for a, b in zip(out, out[1:]))
    return out


def text(seed, skip, n):
    return C.make_chunk({"kind": "bd", "n": n, "seed": seed, "skip": skip}, b"")


# ---------------------------------------------------------------------------
# 1. the liblz4 fixture: every dictionary of it in one call
# ---------------------------------------------------------------------------
def test_fixture_compress_in_one_call():
    dicts = [C.make_dict(g["dict"]) for g in FX["compress"]]
    assert sorted({len(d) for d in dicts}) == sorted(C.DICT_SIZES)
    order = interleave([g["entries"] for g in FX["compress"]])
    assert len(order) == sum(len(g["entries"]) for g in FX["compress"])
    which = [k for k, _ in order]
    ents = [e for _, e in order]
    datas = [C.make_chunk(e["chunk"], dicts[k]) for k, e in order]
    flat, offs = pack(datas)
    ds = DictSet(dicts)
    sizes = [len(x) for x in datas]
    got, dst = set_compress(flat, offs, sizes, [e["cap"] for e in ents], max(sizes), ds, ds.prepare(), which)
    for i, e in enumerate(ents):
        assert got[i] == e["ret"], (FX["compress"][which[i]]["dict"], e, got[i])
        assert sha1(dst.data(i, e["ret"])) == e["sha1"], (FX["compress"][which[i]]["dict"], e)
    assert dst.canaries_ok()


def test_fixture_decode_in_one_call():
    groups = FX["decode"]
    dicts = [C.make_dict(g["dict"])[g["front"]:] for g in groups]
    order = interleave([g["entries"] for g in groups])
    # a group decoded without its dictionary names none
    which = [k if groups[k]["use"] else NO_DICT for k, _ in order]
    assert NO_DICT in which
    ents = [e for _, e in order]
    blocks = [bytes.fromhex(e["block"]) for e in ents]
    flat, offs = pack(blocks)
    got, dst = set_decompress(flat, offs, [len(b) for b in blocks], [e["cap"] for e in ents], DictSet(dicts), which)
    for i, e in enumerate(ents):
        assert got[i] == e["ret"], (groups[order[i][0]]["dict"], e["name"], got[i])
        if e["ret"] >= 0:
            assert sha1(dst.data(i, e["ret"])) == e["sha1"], e["name"]
    assert dst.canaries_ok()


# ---------------------------------------------------------------------------
# 2. states: byte for byte lz4mtHipDictPrepare's, and valid for either call
# ---------------------------------------------------------------------------
def test_states_equal_the_single_prepare():
    dicts = [C.make_dict({"kind": "bd", "size": s, "seed": C.DICT_SEED}) for s in C.DICT_SIZES]
    ds = DictSet(dicts)
    states = ds.prepare()
    singles = [BD.prepare(t) for t in ds.tensors]
    torch.cuda.synchronize()
    S = state_size()
    host = states.cpu().numpy()
    for k, one in enumerate(singles):
        assert host[k * S:(k + 1) * S].tobytes() == one.cpu().numpy().tobytes(), C.DICT_SIZES[k]
    # a set state under lz4mtHipCompressBatchDict, and single states laid out as a set under the set call
    k = C.DICT_SIZES.index(4096)
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": 4096, "seed": C.DICT_SEED})
    d, ents, datas = BD.group_inputs(g, only_bound=True)
    assert d == dicts[k]
    flat, offs = pack(datas)
    sizes = [len(x) for x in datas]
    caps = [e["cap"] for e in ents]
    got, dst = BD.compress_call(flat, offs, sizes, caps, max(sizes), ds.tensors[k], states[k * S:(k + 1) * S])
    BD.check_entries(ents, got, dst, "a set state under the shared-dictionary call")
    laid = torch.cat(singles)
    assert laid.data_ptr() % 256 == 0 and laid.numel() == len(dicts) * S
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, laid, [k] * len(sizes))
    BD.check_entries(ents, got, dst, "single states under the set call")


# ---------------------------------------------------------------------------
# 3. the index decides
# ---------------------------------------------------------------------------
def test_the_index_decides():
    d0 = C.make_dict({"kind": "bd", "size": 4096, "seed": C.DICT_SEED})
    d1 = C.make_dict({"kind": "bd", "size": 4096, "seed": C.GRAPH_SEEDS[0]})
    assert d0 != d1
    chunk = text(C.DICT_SEED, C.CHUNK_SKIP, 1500) + d1[100:900] + d0[2000:2900] + text(6, C.CHUNK_SKIP, 700)
    n = len(chunk)
    flat, offs = pack([chunk, chunk])
    ds = DictSet([d0, d1])
    got, dst = set_compress(flat, offs, [n, n], [bound(n)] * 2, n, ds, ds.prepare(), [0, 1])
    blocks = [dst.data(i, got[i]) for i in range(2)]
    assert blocks[0] == oracle.compress_block_dict(d0, chunk) and blocks[1] == oracle.compress_block_dict(d1, chunk)
    assert blocks[0] != blocks[1]
    assert dst.canaries_ok()
    # each block under each dictionary, in one call
    bflat, boffs = pack([blocks[0], blocks[1], blocks[0], blocks[1]])
    back, ddst = set_decompress(bflat, boffs, [len(blocks[i % 2]) for i in range(4)], [n] * 4, ds, [0, 1, 1, 0])
    for i in (0, 1):
        assert back[i] == n and ddst.data(i, n) == chunk, i
    for i, (b, d) in ((2, (blocks[0], d1)), (3, (blocks[1], d0))):
        ret, out = oracle.decompress_block_dict(b, n, d)
        assert back[i] == ret, i
        assert (ret, out) != (n, chunk)
        if ret > 0:
            assert ddst.data(i, ret) == out and out != chunk, i
    assert ddst.canaries_ok()


def test_hc_blocks_decode_with_the_set():
    """LZ4-HC compress with a set is not built; its blocks, one call per dictionary, decode in one set call."""
    dicts = [C.make_dict({"kind": "bd", "size": 4096, "seed": s}) for s in (C.DICT_SEED, C.GRAPH_SEEDS[0])]
    tensors = [dict_tensor(d) for d in dicts]
    datas = [text(C.DICT_SEED, C.CHUNK_SKIP + 300 * i, 1000 + 700 * i) + dicts[i % 2][500:900] for i in range(6)]
    flat, offs = pack(datas)
    chunks = [flat[o:o + len(x)] for o, x in zip(offs, datas)]
    blocks = [None] * len(datas)
    for k, level in ((0, 9), (1, 12)):
        mine = [i for i in range(len(datas)) if i % 2 == k]
        outs, sizes = L.compress_batch_dict_hc([chunks[i] for i in mine], L.prepare_dict_hc(tensors[k]), level)
        torch.cuda.synchronize()
        for i, o, n in zip(mine, outs, sizes.cpu().tolist()):
            assert n > 0
            blocks[i] = o[:n]
            # an ordinary block of that dictionary, by the oracle's decoder
            assert oracle.decompress_block_dict(bytes(o[:n].cpu().numpy().tobytes()), len(datas[i]),
                                                dicts[k]) == (len(datas[i]), datas[i])
    back, dsz = L.decompress_batch_dict_set(blocks, [len(x) for x in datas], tensors, [i % 2 for i in range(6)])
    torch.cuda.synchronize()
    assert dsz.cpu().tolist() == [len(x) for x in datas]
    for t, x in zip(back, datas):
        assert bytes(t.cpu().numpy().tobytes()) == x


# ---------------------------------------------------------------------------
# 4. the oracle: dictionaries of many sizes and none, mixed in one call
# ---------------------------------------------------------------------------
MIX_DICTS = [0, 7, 8, 9, 4095, 4096, 4097, 65535, 65536, 65537, 100000]
MIX_CHUNKS = [0, 1, 12, 13, 64, 4096, 65535, 65547, 70000]


@functools.lru_cache(maxsize=None)
def mixed_cases():
    """(dicts, cases): case = (which, chunk, cap, the oracle's block).  Dictionary k is a slice of its
    own of the text; a chunk starts with its dictionary's last bytes, goes on in the text the
    dictionaries come from, and holds a stretch of random bytes."""
    dicts = [text(C.DICT_SEED, 1000 * k, s) for k, s in enumerate(MIX_DICTS)]
    cases = []
    for j, n in enumerate(MIX_CHUNKS):
        for k in [*range(len(dicts)), NO_DICT]:
            d = dicts[k] if k != NO_DICT else b""
            body = d[-150:] + text(C.DICT_SEED, C.CHUNK_SKIP + 37 * j, min(n, 3000)) + oracle.gen_random(40, j) + \
                text(C.DICT_SEED, 2000 + 11 * j, n)
            chunk = body[:n]
            for kind in C.CAP_KINDS:
                cap = C.cap_of(kind, n)
                cases.append((k, chunk, cap, oracle.compress_block_dict(d, chunk, cap)))
    # neighbours use different dictionaries
    assert all(a[0] != b[0] for a, b in zip(cases[::4], cases[4::4]))
    return dicts, cases


def test_oracle_mixed_sizes_compress(probe):
    dicts, cases = mixed_cases()
    # the four capacities of a chunk stand apart, so that neighbours differ in dictionary
    order = [c for q in range(4) for c in cases[q::4]]
    datas = [c[1] for c in order]
    flat, offs = pack(datas)
    sizes, caps, which = [len(x) for x in datas], [c[2] for c in order], [c[0] for c in order]
    assert max(sizes) >= B.KLIMIT
    ds = DictSet(dicts)
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, ds.prepare(), which)
    for i, (k, chunk, cap, want) in enumerate(order):
        assert got[i] == len(want), (probe, k, len(chunk), cap, got[i], len(want))
        assert dst.data(i, len(want)) == want, (probe, k, len(chunk), cap)
    assert dst.canaries_ok()
    assert any(not c[3] for c in order) and sum(1 for c in order if c[3]) > len(order) // 2


def first_offset_at(block):
    """Position of the first sequence's offset in ``block``, or None when it holds literals only."""
    tok, i = block[0], 1
    lit = tok >> 4
    if lit == 15:
        while True:
            lit += block[i]
            i += 1
            if block[i - 1] != 255:
                break
    i += lit
    return i if i + 2 <= len(block) - 5 else None


def test_oracle_mixed_sizes_decode():
    dicts, cases = mixed_cases()
    blocks, caps, which, tags = [], [], [], []

    def add(k, block, cap, tag):
        blocks.append(block)
        caps.append(cap)
        which.append(k)
        tags.append(tag)

    for k, chunk, cap, block in cases[::4]:   # the blocks made at the bound
        n = len(chunk)
        assert cap == bound(n) and block
        add(k, block, n, "exact")
        add(k, block, n // 2, "too small")
        add(k, block[:-1], n, "truncated by one")
        add(k, block[:len(block) // 2], n, "cut in half")
        at = first_offset_at(block)
        if at is not None:
            for off in (9, 4097, 0xFFFF):
                add(k, block[:at] + off.to_bytes(2, "little") + block[at + 2:], n, f"offset {off}")
    assert sum(1 for t in tags if t == "offset 65535") > len(MIX_CHUNKS) * 4
    flat, offs = pack(blocks)
    got, dst = set_decompress(flat, offs, [len(b) for b in blocks], caps, DictSet(dicts), which)
    bad = 0
    for i, (k, b, cap, tag) in enumerate(zip(which, blocks, caps, tags)):
        d = dicts[k] if k != NO_DICT else b""
        ret, out = oracle.decompress_block_dict(b, cap, d)
        assert got[i] == ret, (tag, k, len(b), cap, got[i], ret)
        if ret > 0:
            assert dst.data(i, ret) == out, (tag, k, len(b), cap)
        if tag == "exact":
            assert ret == cap
        bad += ret < 0
        if k == NO_DICT or not d:   # LZ4_decompress_safe, every return
            assert (ret, out) == oracle.decompress_block(b, cap), (tag, k)
        if k == NO_DICT:
            assert (got[i], dst.data(i, max(got[i], 0))) == L.decompress_block(b, cap), (tag, len(b), cap)
    assert dst.canaries_ok()
    assert bad > len(blocks) // 4


# ---------------------------------------------------------------------------
# 5. per-chunk refusal
# ---------------------------------------------------------------------------
def test_per_chunk_refusal():
    d0 = C.make_dict({"kind": "bd", "size": 4096, "seed": C.DICT_SEED})
    d2 = C.make_dict({"kind": "bd", "size": 5000, "seed": C.GRAPH_SEEDS[0]})
    ds = DictSet([d0, d0, d2])
    ds.ptr_list[1] = 0                 # a null pointer of size 4096
    ds.size_list[2] = 4096             # prepared for 4096 bytes ...
    ds.upload()
    states = ds.prepare()
    torch.cuda.synchronize()
    S = state_size()
    words = states.cpu().numpy().view(np.uint32).reshape(3, S // 4)
    assert words[0, 4096] == 4096 and words[2, 4096] == 4096
    assert words[1, 4096] == 0xFFFFFFFF and not words[1, :4096].any() and not words[1, 4097:].any()
    ds.size_list[2] = 5000             # ... and used with a size entry of 5000
    ds.upload()
    which = [0, 3, 0xFFFFFFFE, NO_DICT, 1, 0, 2, NO_DICT, 0]
    refused = {1, 2, 4, 6}
    datas = [text(C.DICT_SEED, C.CHUNK_SKIP + 500 * i, 700 + 300 * i) for i in range(len(which))]
    sizes = [len(x) for x in datas]
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, states, which)
    good_blocks = {}
    for i, (k, x) in enumerate(zip(which, datas)):
        if i in refused:
            assert got[i] == BAD, (i, got[i])
            assert dst.untouched_from(i, 0), i
        else:
            want = oracle.compress_block_dict(d0 if k == 0 else b"", x)
            assert got[i] == len(want) and dst.data(i, len(want)) == want, i
            good_blocks[i] = want
    assert dst.canaries_ok()
    # the decoder: the index and the null dictionary (it needs no states, so 5000 bytes are dictionary 2)
    blocks = [good_blocks.get(i, good_blocks[0]) for i in range(len(which))]
    blocks[6] = oracle.compress_block_dict(d2, datas[6])
    bflat, boffs = pack(blocks)
    back, ddst = set_decompress(bflat, boffs, [len(b) for b in blocks], sizes, ds, which)
    for i, x in enumerate(datas):
        if i in (1, 2, 4):
            assert back[i] == BAD and ddst.untouched_from(i, 0), i
        else:
            assert back[i] == len(x) and ddst.data(i, len(x)) == x, i
    assert ddst.canaries_ok()


def test_no_dictionaries_at_all():
    datas = [text(C.DICT_SEED, C.CHUNK_SKIP, n) for n in (0, 1, 64, 4096, 70000)]
    sizes = [len(x) for x in datas]
    flat, offs = pack(datas)
    ds = DictSet([])
    assert ds.k == 0
    got, dst = set_compress(flat, offs, sizes, [bound(n) for n in sizes], max(sizes), ds, None,
                            [NO_DICT] * len(sizes))
    want = [oracle.compress_block_dict(b"", x) for x in datas]
    for i, w in enumerate(want):
        assert got[i] == len(w) and dst.data(i, len(w)) == w, i
    assert dst.canaries_ok()
    bflat, boffs = pack(want)
    back, ddst = set_decompress(bflat, boffs, [len(w) for w in want], sizes, ds, [NO_DICT] * len(sizes))
    assert back == sizes and all(ddst.data(i, len(x)) == x for i, x in enumerate(datas))
    # an index needs a dictionary to name
    got, dst = set_compress(flat, offs, sizes, [bound(n) for n in sizes], max(sizes), ds, None, [0] * len(sizes))
    assert got == [BAD] * len(sizes) and all(dst.untouched_from(i, 0) for i in range(len(sizes)))


# ---------------------------------------------------------------------------
# 6. prepare, compress and decompress in one linear HIP graph
# ---------------------------------------------------------------------------
def test_set_calls_in_hip_graph():
    seeds = [C.DICT_SEED, *C.GRAPH_SEEDS]
    sizes = C.CHUNK_SIZES
    n = len(sizes)

    def chunks_of(seed):
        return [text(seed, C.CHUNK_SKIP, k) for k in sizes]

    dicts = [C.make_dict({"kind": "bd", "size": 4096, "seed": s}) for s in seeds]
    ds = DictSet(dicts)
    states = ds.new_states()
    datas = chunks_of(seeds[0])
    flat, offs = pack(datas)
    caps = [bound(k) for k in sizes]
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    which = [i % 3 for i in range(n)]
    wh = u32(which)
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        st = stream_ptr()
        assert L.lib.lz4mtHipDictSetPrepare(*ds.args(), P(states.data_ptr()), states.numel(), st) == L.Result.OK
        assert L.lib.lz4mtHipCompressBatchDictSet(P(sp.data_ptr()), P(sz.data_ptr()), max(sizes), n,
                                                  P(cp_.data_ptr()), P(cc.data_ptr()), P(csz.data_ptr()),
                                                  *ds.args(), P(states.data_ptr()), P(wh.data_ptr()),
                                                  st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatchDictSet(P(cp_.data_ptr()), P(csz.data_ptr()), n, P(dp.data_ptr()),
                                                    P(sz.data_ptr()), P(dsz.data_ptr()), *ds.args(),
                                                    P(wh.data_ptr()), st) == L.Result.OK

    def check(dicts, datas, which, tag):
        torch.cuda.synchronize()
        cdst.fetch()
        ddst.fetch()
        got, back = csz.cpu().tolist(), dsz.cpu().tolist()
        for i, (k, x) in enumerate(zip(which, datas)):
            want = oracle.compress_block_dict(dicts[k] if k != NO_DICT else b"", x)
            assert got[i] == len(want) and cdst.data(i, len(want)) == want, (tag, i)
            assert back[i] == len(x) and ddst.data(i, len(x)) == x, (tag, i)
        assert cdst.canaries_ok() and ddst.canaries_ok(), tag

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the library outside the capture (the encoder-order check)
        call()
    check(dicts, datas, which, "warm")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for r, seed in enumerate(seeds[1:], 1):
        datas2 = chunks_of(seed)
        new, offs2 = pack(datas2)
        assert offs2 == offs and datas2 != datas
        flat.copy_(new)
        which2 = [(i + r) % 3 for i in range(n)]
        which2[r] = NO_DICT
        wh.copy_(u32(which2))
        dicts2 = list(dicts)
        dicts2[r] = text(seed, 250_000, 4096)      # one dictionary's bytes, in place
        assert dicts2[r] != dicts[r]
        ds.tensors[r].copy_(torch.frombuffer(bytearray(dicts2[r]), dtype=torch.uint8))
        states.fill_(0xCC)
        cdst.back.fill_(FILL)
        ddst.back.fill_(FILL)
        csz.zero_()
        dsz.zero_()
        g.replay()
        check(dicts2, datas2, which2, f"replay {r}")
        ds.tensors[r].copy_(torch.frombuffer(bytearray(dicts[r]), dtype=torch.uint8))


# ---------------------------------------------------------------------------
# 7. the Python wrappers on a side stream, 8. the empty batch and the empty set
# ---------------------------------------------------------------------------
def test_python_wrappers_on_side_stream():
    dicts = [C.make_dict({"kind": "bd", "size": s, "seed": C.DICT_SEED}) for s in (4096, 0, 65537)]
    tensors = [dict_tensor(d) for d in dicts]
    which = [0, None, 2, 1, None, 0, 2]
    datas = [text(C.DICT_SEED, C.CHUNK_SKIP + 100 * i, 500 + 900 * i) for i in range(len(which))]
    flat, offs = pack(datas)
    chunks = [flat[o:o + len(x)] for o, x in zip(offs, datas)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    prepared = L.prepare_dict_set(tensors, stream=s)
    assert isinstance(prepared, L.PreparedDictSet) and len(prepared) == 3
    assert all(a is b for a, b in zip(prepared.dictionaries, tensors))
    assert prepared.states.numel() == 3 * state_size() and prepared.states.data_ptr() % 256 == 0
    assert prepared.ptrs.dtype == torch.int64 and prepared.sizes.dtype == torch.int32
    outs, sizes = L.compress_batch_dict_set(chunks, prepared, which, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    s.synchronize()
    csz = sizes.cpu().tolist()
    want = [oracle.compress_block_dict(dicts[k] if k is not None else b"", x) for k, x in zip(which, datas)]
    assert csz == [len(w) for w in want]
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for b, w in zip(blocks, want):
        assert bytes(b.cpu().numpy().tobytes()) == w
    for dictionaries in (prepared, tensors):
        back, dsz = L.decompress_batch_dict_set(blocks, [len(x) for x in datas], dictionaries, which, stream=s)
        s.synchronize()
        assert dsz.cpu().tolist() == [len(x) for x in datas]
        for t, x in zip(back, datas):
            assert bytes(t.cpu().numpy().tobytes()) == x
    # explicit capacities: what does not fit reports 0
    caps = [len(x) // 3 for x in datas]
    outs, sizes = L.compress_batch_dict_set(chunks, prepared, which, caps=caps, stream=s)
    s.synchronize()
    assert sizes.cpu().tolist() == [len(oracle.compress_block_dict(dicts[k] if k is not None else b"", x, c))
                                    for k, x, c in zip(which, datas, caps)]
    with pytest.raises(ValueError):
        L.compress_batch_dict_set(chunks, prepared, [3] * len(chunks), stream=s)
    with pytest.raises(ValueError):
        L.compress_batch_dict_set(chunks, prepared, which[:-1], stream=s)
    with pytest.raises(TypeError):
        L.compress_batch_dict_set(chunks, tensors, which, stream=s)


def test_empty_batch_and_empty_set():
    dt = dict_tensor(C.make_dict({"kind": "bd", "size": 4096, "seed": C.DICT_SEED}))
    prepared = L.prepare_dict_set([dt])
    outs, sizes = L.compress_batch_dict_set([], prepared, [])
    assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    outs, sizes = L.decompress_batch_dict_set([], [], prepared, [])
    assert outs == [] and sizes.numel() == 0
    outs, sizes = L.decompress_batch_dict_set([], [], [dt], [])
    assert outs == [] and sizes.numel() == 0
    dp, dsz, st = P(prepared.ptrs.data_ptr()), P(prepared.sizes.data_ptr()), P(prepared.states.data_ptr())
    assert L.lib.lz4mtHipCompressBatchDictSet(None, None, 0, 0, None, None, None, dp, dsz, 1, st, None,
                                              stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDecompressBatchDictSet(None, None, 0, None, None, None, dp, dsz, 1, None,
                                                stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDictSetPrepare(None, None, 0, None, 0, stream_ptr()) == L.Result.OK
    # the empty set: every chunk names no dictionary
    none = L.prepare_dict_set([])
    assert len(none) == 0 and none.states.numel() == 0
    x = text(C.DICT_SEED, C.CHUNK_SKIP, 1000)
    chunk = torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    outs, sizes = L.compress_batch_dict_set([chunk], none, [None])
    torch.cuda.synchronize()
    k = sizes.cpu().tolist()[0]
    want = oracle.compress_block_dict(b"", x)
    assert k == len(want) and bytes(outs[0][:k].cpu().numpy().tobytes()) == want
    back, dsz = L.decompress_batch_dict_set([outs[0][:k]], [len(x)], [], [None])
    torch.cuda.synchronize()
    assert dsz.cpu().tolist() == [len(x)] and bytes(back[0].cpu().numpy().tobytes()) == x
