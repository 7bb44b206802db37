"""Batched block operators with a shared dictionary (include/lz4mt_hip.h
section 5b: lz4mtHipDictPrepare, lz4mtHipCompressBatchDict,
lz4mtHipDecompressBatchDict; kernels k_dict_prepare, k_encode_batch_dict,
k_decode_batch_dict).

The reference is liblz4 1.9.3 itself, through the committed fixture
tests/golden/dict_blocks.json (LZ4_loadDict + LZ4_compress_fast_continue,
LZ4_decompress_safe_usingDict; made by tests/golden/make_golden_dict.py,
pinned on hosts with liblz4 by test_dict_golden.py) -- never the library's
other paths.  Inputs are packed as test_gpu_batch.py packs them (chunk
starts at every offset mod 16, the last chunk on the tensor's last byte, 32
canary bytes after every capacity); the dictionary tensor starts at an odd
address and ends on its tensor's last byte.  A call takes one dictionary, so
the decode entries run as one call per dictionary of the fixture.
"""
import ctypes
import hashlib
import json
import os
import random

import numpy as np
import pytest
import torch

import dict_cases as C
from conftest import GOLDEN
from test_gpu_batch import BAD, FILL, Dst, bound, i64, pack, stream_ptr, u32

pytestmark = pytest.mark.gpu

L = None
P = ctypes.c_void_p
with open(os.path.join(GOLDEN, "dict_blocks.json")) as _f:
    FX = json.load(_f)
N_COMPRESS, N_DECODE = len(FX["compress"]), len(FX["decode"])
MAIN = [i for i, g in enumerate(FX["compress"]) if g["dict"]["seed"] == C.DICT_SEED]


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = lz4mt_amd
    assert L.device_count() > 0
    return L


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def sha1(b):
    return hashlib.sha1(b).hexdigest()


def dict_tensor(d):
    """The dictionary at an odd address, ending on the tensor's last byte."""
    buf = torch.full((len(d) + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    if d:
        buf[1:].copy_(torch.frombuffer(bytearray(d), dtype=torch.uint8))
    t = buf[1:]
    assert (not d or t.data_ptr() % 2 == 1) and t.numel() == len(d)
    return t


def dptr(t):
    return P(t.data_ptr() if t.numel() else None)


def new_state():
    st = torch.full((L.lib.lz4mtHipDictStateSize(),), 0xCC, dtype=torch.uint8, device="cuda")
    assert st.data_ptr() % 256 == 0
    return st


def prepare(dt, state=None):
    state = new_state() if state is None else state
    assert L.lib.lz4mtHipDictPrepare(dptr(dt), dt.numel(), P(state.data_ptr()), state.numel(),
                                     stream_ptr()) == L.Result.OK
    return state


def compress_call(flat, soffs, sizes, caps, max_chunk, dt, state, null_caps=False, dst=None, dst_ptrs=None,
                  src_ptrs=None, dict_size=None):
    dst = dst or Dst(caps)
    sp = i64(src_ptrs if src_ptrs is not None else [flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipCompressBatchDict(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes), P(dp.data_ptr()),
                                        P(None if null_caps else cp.data_ptr()), P(out.data_ptr()), dptr(dt),
                                        dt.numel() if dict_size is None else dict_size, P(state.data_ptr()),
                                        stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def decompress_call(flat, soffs, sizes, caps, dt, dst=None, dst_ptrs=None):
    dst = dst or Dst(caps)
    sp = i64([flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    r = L.lib.lz4mtHipDecompressBatchDict(P(sp.data_ptr()), P(sz.data_ptr()), len(sizes), P(dp.data_ptr()),
                                          P(cp.data_ptr()), P(out.data_ptr()), dptr(dt), dt.numel(), stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def group_inputs(g, only_bound=False):
    """(dictionary bytes, entries, chunk bytes per entry) of a compress group."""
    d = C.make_dict(g["dict"])
    ents = [e for e in g["entries"] if not only_bound or e["capkind"] == "bound"]
    return d, ents, [C.make_chunk(e["chunk"], d) for e in ents]


def check_entries(ents, got, dst, tag):
    for i, e in enumerate(ents):
        assert got[i] == e["ret"], (tag, e, got[i])
        assert sha1(dst.data(i, e["ret"])) == e["sha1"], (tag, e)
    assert dst.canaries_ok(), tag


# ---------------------------------------------------------------------------
# 1. the fixture: one compress call per dictionary, all its chunks and capacities
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(N_COMPRESS))
def test_fixture_compress(gi):
    g = FX["compress"][gi]
    d, ents, datas = group_inputs(g)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    state = prepare(dt)
    caps = [e["cap"] for e in ents]
    got, dst = compress_call(flat, offs, [len(x) for x in datas], caps, max(len(x) for x in datas), dt, state)
    check_entries(ents, got, dst, g["dict"])


@pytest.mark.parametrize("size", [0, 4096, 65536, 100000])
def test_null_capacities_are_the_bound(size):
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": size, "seed": C.DICT_SEED})
    d, ents, datas = group_inputs(g, only_bound=True)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    caps = [bound(len(x)) for x in datas]
    assert caps == [e["cap"] for e in ents]
    got, dst = compress_call(flat, offs, [len(x) for x in datas], caps, 4 << 20, dt, prepare(dt), null_caps=True)
    check_entries(ents, got, dst, ("null caps", size))


# ---------------------------------------------------------------------------
# 2. more workgroups than the device holds, every chunk decoded back
# ---------------------------------------------------------------------------
def test_many_chunks_round_trip():
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": 4096, "seed": C.DICT_SEED})
    d, ents, datas = group_inputs(g, only_bound=True)
    ents, datas = ents[:16], datas[:16]
    rnd = random.Random(5)
    pool = C.make_chunk({"kind": "bd", "n": 300_000, "seed": C.DICT_SEED, "skip": 150_000}, d) + \
        C.make_chunk({"kind": "mixed", "n": 70000, "seed": 70000}, d) + d
    while len(datas) < 5000:
        n = rnd.randrange(64, 4097)
        a = rnd.randrange(len(pool) - n)
        datas.append(pool[a:a + n])
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    got, dst = compress_call(flat, offs, sizes, caps, max(sizes), dt, prepare(dt))
    check_entries(ents, got[:16], dst, "first 16")
    assert all(0 < r <= c for r, c in zip(got, caps))
    assert dst.canaries_ok()
    # with the dictionary the text chunks come out smaller than on their own
    assert sum(got) < sum(sizes)
    # back: the blocks where the encoder left them
    ddst = Dst(sizes)
    sp, dp = i64(dst.ptrs), i64(ddst.ptrs)
    csz, cp = u32(got), u32(sizes)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert L.lib.lz4mtHipDecompressBatchDict(P(sp.data_ptr()), P(csz.data_ptr()), len(sizes), P(dp.data_ptr()),
                                             P(cp.data_ptr()), P(out.data_ptr()), dptr(dt), dt.numel(),
                                             stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
    ddst.fetch()
    assert out.cpu().tolist() == sizes
    for i, x in enumerate(datas):
        assert ddst.data(i, len(x)) == x, i
    assert ddst.canaries_ok()


# ---------------------------------------------------------------------------
# 3. decode: the fixture's entries, then every compress entry's block back to its source
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gi", range(N_DECODE))
def test_fixture_decode(gi):
    g = FX["decode"][gi]
    d = C.make_dict(g["dict"])[g["front"]:] if g["use"] else b""
    ents = g["entries"]
    blocks = [bytes.fromhex(e["block"]) for e in ents]
    caps = [e["cap"] for e in ents]
    flat, offs = pack(blocks)
    got, dst = decompress_call(flat, offs, [len(b) for b in blocks], caps, dict_tensor(d))
    for i, e in enumerate(ents):
        assert got[i] == e["ret"], (g["dict"], g["front"], g["use"], e["name"], got[i])
        if e["ret"] >= 0:
            assert sha1(dst.data(i, e["ret"])) == e["sha1"], e["name"]
    assert dst.canaries_ok()


@pytest.mark.parametrize("gi", MAIN)
def test_device_blocks_decode_back(gi):
    g = FX["compress"][gi]
    d, ents, datas = group_inputs(g, only_bound=True)
    sizes = [len(x) for x in datas]
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    got, cdst = compress_call(flat, offs, sizes, [bound(n) for n in sizes], max(sizes), dt, prepare(dt))
    assert got == [e["ret"] for e in ents]
    blocks = [cdst.data(i, r) for i, r in enumerate(got)]
    bflat, boffs = pack(blocks)
    # exact capacities, and the whole dictionary (the decoder does not trim it)
    back, ddst = decompress_call(bflat, boffs, got, sizes, dt)
    assert back == sizes
    for i, x in enumerate(datas):
        assert ddst.data(i, len(x)) == x, (g["dict"], ents[i]["chunk"])
    assert ddst.canaries_ok()


# ---------------------------------------------------------------------------
# 4. refused chunks, and a state prepared for another dictionary size
# ---------------------------------------------------------------------------
def test_per_chunk_rejection():
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": 4096, "seed": C.DICT_SEED})
    d, ents, datas = group_inputs(g, only_bound=True)
    pick = [i for i, x in enumerate(datas) if len(x) <= 4096][:8]
    ents, datas = [ents[i] for i in pick], [datas[i] for i in pick]
    sizes = [len(x) for x in datas]
    assert len(sizes) == 8 and sizes[5] != 0 and sizes[6] > 100
    flat, offs = pack(datas)
    caps = [bound(n) for n in sizes]
    mis, null, nosrc, big = 1, 3, 5, 6   # base + 8; null destination; null source of non-zero size; above maxChunkBytes
    dst = Dst(caps)
    ptrs = list(dst.ptrs)
    ptrs[mis] += 8
    ptrs[null] = 0
    sptrs = [flat.data_ptr() + o for o in offs]
    sptrs[nosrc] = 0
    dt = dict_tensor(d)
    got, dst = compress_call(flat, offs, sizes, caps, sizes[big] - 1, dt, prepare(dt), dst=dst, dst_ptrs=ptrs,
                             src_ptrs=sptrs)
    for i, e in enumerate(ents):
        if i in (mis, null, nosrc, big) or sizes[i] > sizes[big] - 1:
            assert got[i] == BAD, (i, got[i])
            assert dst.untouched_from(i, 0), i
        else:
            assert got[i] == e["ret"] and sha1(dst.data(i, e["ret"])) == e["sha1"], i
    assert dst.canaries_ok()
    # the decoder: misaligned and null destinations
    blocks = [bytes.fromhex(e["block"]) for e in FX["decode"][0]["entries"][:6]]
    assert FX["decode"][0]["dict"]["size"] == 4096 and FX["decode"][0]["use"]
    want = FX["decode"][0]["entries"][:6]
    bflat, boffs = pack(blocks)
    ddst = Dst([e["cap"] for e in want])
    ptrs = list(ddst.ptrs)
    ptrs[mis] += 8
    ptrs[null] = 0
    back, ddst = decompress_call(bflat, boffs, [len(b) for b in blocks], [e["cap"] for e in want], dt, dst=ddst,
                                 dst_ptrs=ptrs)
    for i, e in enumerate(want):
        if i in (mis, null):
            assert back[i] == BAD and ddst.untouched_from(i, 0), i
        else:
            assert back[i] == e["ret"] and sha1(ddst.data(i, e["ret"])) == e["sha1"], i
    assert ddst.canaries_ok()


def test_state_of_another_dictionary_size_refuses_every_chunk():
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": 65536, "seed": C.DICT_SEED})
    d, ents, datas = group_inputs(g, only_bound=True)
    keep = [i for i, x in enumerate(datas) if len(x) <= 4096]
    ents, datas = [ents[i] for i in keep], [datas[i] for i in keep]
    sizes = [len(x) for x in datas]
    flat, offs = pack(datas)
    dt = dict_tensor(d)                       # 65536 bytes
    stale = prepare(dt[-4096:])               # a state for its last 4096
    got, dst = compress_call(flat, offs, sizes, [bound(n) for n in sizes], 4096, dt, stale)
    assert got == [BAD] * len(sizes)
    assert all(dst.untouched_from(i, 0) for i in range(len(sizes)))
    # the same state with the dictionary it was made for
    got, dst = compress_call(flat, offs, sizes, [bound(n) for n in sizes], 4096, dt[-4096:], stale)
    assert all(r > 0 for r, n in zip(got, sizes) if n)
    # 65537 bytes have the effective size of 65536: no refusal, and other bytes are not the state's business
    fresh = prepare(dt)
    one = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), dt])
    got2, dst2 = compress_call(flat, offs, sizes, [bound(n) for n in sizes], 4096, one, fresh)
    check_entries(ents, got2, dst2, "65537 bytes on a 65536-byte state")


# ---------------------------------------------------------------------------
# 5. prepare, compress and decompress in one HIP graph, replayed on new chunks AND a new dictionary
# ---------------------------------------------------------------------------
def test_dict_calls_in_hip_graph():
    groups = {g["dict"]["seed"]: g for g in FX["compress"] if g["dict"]["size"] == 4096}
    seeds = [C.DICT_SEED, *C.GRAPH_SEEDS]

    def content(seed):
        g = groups[seed]
        d = C.make_dict(g["dict"])
        ents = [e for e in g["entries"] if e["capkind"] == "bound" and e["chunk"]["kind"] == "bd"]
        return d, ents, [C.make_chunk(e["chunk"], d) for e in ents]

    d, ents, datas = content(seeds[0])
    sizes = [len(x) for x in datas]
    assert sizes == C.CHUNK_SIZES
    n = len(sizes)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    state = new_state()
    caps = [bound(k) for k in sizes]
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        st = stream_ptr()
        assert L.lib.lz4mtHipDictPrepare(dptr(dt), dt.numel(), P(state.data_ptr()), state.numel(), st) == L.Result.OK
        assert L.lib.lz4mtHipCompressBatchDict(P(sp.data_ptr()), P(sz.data_ptr()), max(sizes), n, P(cp_.data_ptr()),
                                               P(cc.data_ptr()), P(csz.data_ptr()), dptr(dt), dt.numel(),
                                               P(state.data_ptr()), st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatchDict(P(cp_.data_ptr()), P(csz.data_ptr()), n, P(dp.data_ptr()),
                                                 P(sz.data_ptr()), P(dsz.data_ptr()), dptr(dt), dt.numel(),
                                                 st) == L.Result.OK

    def check(ents, datas, tag):
        torch.cuda.synchronize()
        cdst.fetch()
        ddst.fetch()
        got, back = csz.cpu().tolist(), dsz.cpu().tolist()
        for i, (e, x) in enumerate(zip(ents, datas)):
            assert got[i] == e["ret"] and sha1(cdst.data(i, e["ret"])) == e["sha1"], (tag, i)
            assert back[i] == len(x) and ddst.data(i, len(x)) == x, (tag, i)
        assert cdst.canaries_ok() and ddst.canaries_ok(), tag

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the library outside the capture (the encoder-order check)
        call()
    check(ents, datas, "warm")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for seed in seeds[1:]:
        d2, ents2, datas2 = content(seed)
        assert d2 != d and len(d2) == len(d)
        new, offs2 = pack(datas2)
        assert offs2 == offs
        flat.copy_(new)
        dt.copy_(torch.frombuffer(bytearray(d2), dtype=torch.uint8))
        state.fill_(0xCC)
        cdst.back.fill_(FILL)
        ddst.back.fill_(FILL)
        csz.zero_()
        dsz.zero_()
        g.replay()
        check(ents2, datas2, f"replay, dictionary seed {seed}")


# ---------------------------------------------------------------------------
# 6. the Python wrappers on a side stream, and the empty batch
# ---------------------------------------------------------------------------
def test_python_wrappers_on_side_stream():
    g = next(g for g in FX["compress"] if g["dict"] == {"kind": "bd", "size": 65537, "seed": C.DICT_SEED})
    d, ents, datas = group_inputs(g, only_bound=True)
    flat, offs = pack(datas)
    chunks = [flat[o:o + len(x)] for o, x in zip(offs, datas)]
    dt = dict_tensor(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    prepared = L.prepare_dict(dt, stream=s)
    assert isinstance(prepared, L.PreparedDict) and prepared.dictionary is dt
    assert prepared.state.numel() == L.lib.lz4mtHipDictStateSize() and prepared.state.data_ptr() % 256 == 0
    outs, sizes = L.compress_batch_dict(chunks, prepared, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    assert len({o.untyped_storage().data_ptr() for o in outs}) == 1   # one backing allocation
    s.synchronize()
    csz = sizes.cpu().tolist()
    assert csz == [e["ret"] for e in ents]
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for b, e in zip(blocks, ents):
        assert sha1(bytes(b.cpu().numpy().tobytes())) == e["sha1"], e
    for dictionary in (prepared, dt):
        back, dsz = L.decompress_batch_dict(blocks, [len(x) for x in datas], dictionary, stream=s)
        s.synchronize()
        assert dsz.cpu().tolist() == [len(x) for x in datas]
        for t, x in zip(back, datas):
            assert bytes(t.cpu().numpy().tobytes()) == x
    # explicit capacities: what does not fit reports 0
    third = [e for e in g["entries"] if e["capkind"] == "n/3"]
    assert [e["chunk"] for e in third] == [e["chunk"] for e in ents]
    outs, sizes = L.compress_batch_dict(chunks, prepared, caps=[e["cap"] for e in third], stream=s)
    s.synchronize()
    assert sizes.cpu().tolist() == [e["ret"] for e in third]
    with pytest.raises(TypeError):
        L.compress_batch_dict(chunks, dt)


def test_empty_batch():
    dt = dict_tensor(C.make_dict({"kind": "bd", "size": 4096, "seed": C.DICT_SEED}))
    prepared = L.prepare_dict(dt)
    outs, sizes = L.compress_batch_dict([], prepared)
    assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    outs, sizes = L.decompress_batch_dict([], [], prepared)
    assert outs == [] and sizes.numel() == 0
    st = P(prepared.state.data_ptr())
    assert L.lib.lz4mtHipCompressBatchDict(None, None, 0, 0, None, None, None, dptr(dt), dt.numel(), st,
                                           stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipCompressBatchDict(None, None, 0, 0, None, None, None, None, 0, st,
                                           stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDecompressBatchDict(None, None, 0, None, None, None, dptr(dt), dt.numel(),
                                             stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDecompressBatchDict(None, None, 0, None, None, None, None, 0, stream_ptr()) == L.Result.OK
    # an empty dictionary tensor is no dictionary
    none = L.prepare_dict(torch.empty(0, dtype=torch.uint8, device="cuda"))
    g = next(g for g in FX["compress"] if g["dict"]["size"] == 0)
    e = next(e for e in g["entries"] if e["chunk"]["n"] == 1000 and e["capkind"] == "bound")
    x = C.make_chunk(e["chunk"], b"")
    chunk = torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    outs, sizes = L.compress_batch_dict([chunk], none)
    torch.cuda.synchronize()
    k = sizes.cpu().tolist()[0]
    assert k == e["ret"] and sha1(bytes(outs[0][:k].cpu().numpy().tobytes())) == e["sha1"]
