"""Batched LZ4-HC compress with a shared dictionary (include/lz4mt_hip.h
section 5c: lz4mtHipDictPrepareHC, lz4mtHipCompressBatchDictHC; kernels
k_hc_dict_prepare, k_hc_prev_batch<HcSharedDict>,
k_encode_hc_batch<HcSharedDict>, k_encode_hc_opt_batch<HcSharedDict>).

The reference is liblz4 1.9.3 itself, through the committed fixtures
tests/golden/dict_hc_blocks.json and dict_hc_fuzz.json (LZ4_loadDictHC +
LZ4_compress_HC_continue on a fresh stream per chunk, dictionary and chunk in
separate buffers; made by tests/golden/make_golden_dict_hc.py, pinned on hosts
with liblz4 by test_dict_hc_golden.py) -- never the library's other paths.
Inputs are packed as test_gpu_batch_dict.py packs them (chunk starts at every
offset mod 16, the last chunk on the tensor's last byte, 32 canary bytes after
every capacity, the dictionary at an odd address ending on its tensor's last
byte).  A call takes one dictionary and one level, so the fixtures run as one
call per (dictionary, level); every block that fits is decoded back on the
device with lz4mtHipDecompressBatchDict.
"""
import ctypes
import hashlib
import json
import os
import random

import pytest
import torch

import dict_hc_cases as H
from conftest import GOLDEN
from test_gpu_batch import BAD, FILL, Dst, bound, i64, pack, stream_ptr, u32

pytestmark = pytest.mark.gpu

L = None
P = ctypes.c_void_p
with open(os.path.join(GOLDEN, "dict_hc_blocks.json")) as _f:
    FX = json.load(_f)
with open(os.path.join(GOLDEN, "dict_hc_fuzz.json")) as _f:
    FZ = json.load(_f)
CALLS = [(gi, lv) for gi, g in enumerate(FX["groups"]) for lv in sorted({e[1] for e in g["entries"]})]


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
    st = torch.full((L.lib.lz4mtHipDictStateSizeHC(),), 0xCC, dtype=torch.uint8, device="cuda")
    assert st.data_ptr() % 256 == 0
    return st


def prepare(dt, state=None):
    state = new_state() if state is None else state
    assert L.lib.lz4mtHipDictPrepareHC(dptr(dt), dt.numel(), P(state.data_ptr()), state.numel(),
                                       stream_ptr()) == L.Result.OK
    return state


def slot_bytes(max_chunk, level):
    return L.lib.lz4mtHipCompressBatchDictWorkspaceSize(max_chunk, 1, level)


def compress_call(flat, soffs, sizes, caps, max_chunk, dt, state, level, null_caps=False, dst=None, dst_ptrs=None,
                  src_ptrs=None, dict_size=None, slots=None):
    """One lz4mtHipCompressBatchDictHC with a workspace of ``slots`` slots (default: the full size)."""
    dst = dst or Dst(caps)
    sp = i64(src_ptrs if src_ptrs is not None else [flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nbytes = L.lib.lz4mtHipCompressBatchDictWorkspaceSize(max_chunk, len(sizes), level) if slots is None else \
        slots * slot_bytes(max_chunk, level)
    ws = torch.full((nbytes,), 0xDD, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    r = L.lib.lz4mtHipCompressBatchDictHC(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes), P(dp.data_ptr()),
                                          P(None if null_caps else cp.data_ptr()), P(out.data_ptr()), dptr(dt),
                                          dt.numel() if dict_size is None else dict_size, P(state.data_ptr()), level,
                                          P(ws.data_ptr()), ws.numel(), stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def decode_back(cdst, got, datas, dt, tag):
    """Every block of ``cdst`` that fits (got > 0), where the encoder left it, back to its source."""
    keep = [i for i, r in enumerate(got) if r > 0]
    if not keep:
        return
    sizes = [len(datas[i]) for i in keep]
    ddst = Dst(sizes)
    sp, dp = i64([cdst.ptrs[i] for i in keep]), i64(ddst.ptrs)
    csz, cp = u32([got[i] for i in keep]), u32(sizes)
    out = torch.full((len(keep),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert L.lib.lz4mtHipDecompressBatchDict(P(sp.data_ptr()), P(csz.data_ptr()), len(keep), P(dp.data_ptr()),
                                             P(cp.data_ptr()), P(out.data_ptr()), dptr(dt), dt.numel(),
                                             stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
    ddst.fetch()
    assert out.cpu().tolist() == sizes, tag
    for k, i in enumerate(keep):
        assert ddst.data(k, sizes[k]) == datas[i], (tag, i)
    assert ddst.canaries_ok(), tag


def group_inputs(g, level, only_bound=False):
    """(dictionary bytes, entries, chunk bytes per entry) of a fixture group at one level."""
    d = H.make_dict(g["dict"])
    ents = [e for e in g["entries"] if e[1] == level and (not only_bound or e[2] == "bound")]
    return d, ents, [H.make_chunk(e[0], d, g["dict"]["seed"]) for e in ents]


def check_entries(ents, got, dst, tag):
    for i, e in enumerate(ents):
        assert got[i] == e[3], (tag, e, got[i])
        assert sha1(dst.data(i, e[3])) == e[4], (tag, e)
    assert dst.canaries_ok(), tag


def main_group(size):
    return next(g for g in FX["groups"] if g["dict"] == H.dict_spec(size))


# ---------------------------------------------------------------------------
# 1. the fixture: one compress call per (dictionary, level), all its chunks and capacities; blocks decoded back
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("gi,level", CALLS)
def test_fixture_compress(gi, level):
    g = FX["groups"][gi]
    d, ents, datas = group_inputs(g, level)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    caps = [H.cap_of(e[2], len(x)) for e, x in zip(ents, datas)]
    got, dst = compress_call(flat, offs, [len(x) for x in datas], caps, max(len(x) for x in datas), dt, prepare(dt),
                             level)
    check_entries(ents, got, dst, (g["dict"], level))
    decode_back(dst, got, datas, dt, (g["dict"], level))


# ---------------------------------------------------------------------------
# 2. the seeded differential fixture, one call per (dictionary, level); one state per dictionary serves all levels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("di", range(len(FZ["dicts"])))
def test_seeded_cases(di):
    d = H.make_dict(FZ["dicts"][di])
    dt = dict_tensor(d)
    state = prepare(dt)
    cases = [c for c in FZ["cases"] if c[0] == di]
    assert cases
    for level in sorted({c[4] for c in cases}):
        ents = [c for c in cases if c[4] == level]
        datas = [H.fuzz_chunk(c[1], c[2], c[3], d) for c in ents]
        flat, offs = pack(datas)
        caps = [H.cap_of(c[5], c[2]) for c in ents]
        got, dst = compress_call(flat, offs, [c[2] for c in ents], caps, H.FUZZ_MAX_CHUNK, dt, state, level)
        for i, c in enumerate(ents):
            assert got[i] == c[6], (c, got[i])
            assert sha1(dst.data(i, c[6])) == c[7], c
        assert dst.canaries_ok(), (di, level)
        decode_back(dst, got, datas, dt, (di, level))


# ---------------------------------------------------------------------------
# 3. round trip on the device, independent of any reference: thousands of small chunks, rounds and slot reuse
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 10])
def test_many_chunks_round_trip_one_slot_and_full(level):
    d = H.make_dict(H.dict_spec(65536))
    rnd = random.Random(level)
    pool = H.make_chunk("bd:300000", d) + H.make_chunk("mixed:70000", d) + d
    datas = [b"", pool[:3], pool[5:18]]
    while len(datas) < 2000:
        n = rnd.choice([rnd.randrange(0, 300), rnd.randrange(300, 2049), 4096])
        a = rnd.randrange(len(pool) - n)
        datas.append(pool[a:a + n])
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    state = prepare(dt)
    full, fdst = compress_call(flat, offs, sizes, caps, max(sizes), dt, state, level)
    assert all(0 < r <= c for r, c in zip(full, caps)) and fdst.canaries_ok()
    assert sum(full) < sum(sizes) // 2          # the dictionary holds the pool's text
    decode_back(fdst, full, datas, dt, ("full", level))
    one, odst = compress_call(flat, offs, sizes, caps, max(sizes), dt, state, level, slots=1)   # 2000 rounds
    assert one == full and odst.canaries_ok()
    assert torch.equal(odst.back, fdst.back)    # identical bytes, slot by slot


# ---------------------------------------------------------------------------
# 4. null capacities, refused chunks, stale and foreign states
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size,level", [(0, 9), (4096, 3), (65536, 10), (100000, 12)])
def test_null_capacities_are_the_bound(size, level):
    g = main_group(size)
    d, ents, datas = group_inputs(g, level, only_bound=True)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    caps = [bound(len(x)) for x in datas]
    got, dst = compress_call(flat, offs, [len(x) for x in datas], caps, 4 << 20, dt, prepare(dt), level,
                             null_caps=True)
    check_entries(ents, got, dst, ("null caps", size, level))


@pytest.mark.parametrize("level", [9, 12])
def test_per_chunk_rejection(level):
    g = main_group(4096)
    d, ents, datas = group_inputs(g, level, only_bound=True)
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
    got, dst = compress_call(flat, offs, sizes, caps, sizes[big] - 1, dt, prepare(dt), level, dst=dst, dst_ptrs=ptrs,
                             src_ptrs=sptrs, slots=3)
    for i, e in enumerate(ents):
        if i in (mis, null, nosrc, big) or sizes[i] > sizes[big] - 1:
            assert got[i] == BAD, (i, got[i])
            assert dst.untouched_from(i, 0), i
        else:
            assert got[i] == e[3] and sha1(dst.data(i, e[3])) == e[4], i
    assert dst.canaries_ok()


def _small(g, level):
    d, ents, datas = group_inputs(g, level, only_bound=True)
    keep = [i for i, x in enumerate(datas) if len(x) <= 4096]
    return d, [ents[i] for i in keep], [datas[i] for i in keep]


@pytest.mark.parametrize("level", [3, 10])
def test_state_of_another_dictionary_size_refuses_every_chunk(level):
    d, ents, datas = _small(main_group(65536), level)
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    dt = dict_tensor(d)                       # 65536 bytes
    stale = prepare(dt[-4096:])               # a state for its last 4096
    got, dst = compress_call(flat, offs, sizes, caps, 4096, dt, stale, level)
    assert got == [BAD] * len(sizes)
    assert all(dst.untouched_from(i, 0) for i in range(len(sizes)))
    # the same state with the dictionary it was made for
    got, dst = compress_call(flat, offs, sizes, caps, 4096, dt[-4096:], stale, level)
    assert all(r > 0 for r in got)
    # 65537 bytes have the effective size of 65536: no refusal, and other bytes are not the state's business
    one = torch.cat([torch.zeros(1, dtype=torch.uint8, device="cuda"), dt])
    got2, dst2 = compress_call(flat, offs, sizes, caps, 4096, one, prepare(dt), level)
    check_entries(ents, got2, dst2, "65537 bytes on a 65536-byte state")
    # a state nothing has prepared
    got3, dst3 = compress_call(flat, offs, sizes, caps, 4096, dt, new_state(), level)
    assert got3 == [BAD] * len(sizes) and all(dst3.untouched_from(i, 0) for i in range(len(sizes)))


@pytest.mark.parametrize("level", [9, 12])
def test_the_two_kinds_of_state_refuse_each_other(level):
    """The header's section 5c: a state of lz4mtHipDictPrepare handed to the HC call, and an HC state handed
    to lz4mtHipCompressBatchDict, refuse every chunk -- for the same dictionary, so only the kind differs."""
    d, ents, datas = _small(main_group(4096), level)
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    hc = prepare(dt)
    fast = torch.full((hc.numel(),), 0xCC, dtype=torch.uint8, device="cuda")   # (as large as the HC call may read)
    assert L.lib.lz4mtHipDictPrepare(dptr(dt), dt.numel(), P(fast.data_ptr()), fast.numel(),
                                     stream_ptr()) == L.Result.OK
    got, dst = compress_call(flat, offs, sizes, caps, 4096, dt, fast, level)
    assert got == [BAD] * len(sizes) and all(dst.untouched_from(i, 0) for i in range(len(sizes)))
    # the other way round
    fdst = Dst(caps)
    sp, dp = i64([flat.data_ptr() + o for o in offs]), i64(fdst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert L.lib.lz4mtHipCompressBatchDict(P(sp.data_ptr()), P(sz.data_ptr()), 4096, len(sizes), P(dp.data_ptr()),
                                           P(cp.data_ptr()), P(out.data_ptr()), dptr(dt), dt.numel(),
                                           P(hc.data_ptr()), stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
    fdst.fetch()
    assert out.cpu().tolist() == [BAD] * len(sizes) and all(fdst.untouched_from(i, 0) for i in range(len(sizes)))
    # each with its own call still works
    got, dst = compress_call(flat, offs, sizes, caps, 4096, dt, hc, level)
    check_entries(ents, got, dst, "own state")


# ---------------------------------------------------------------------------
# 5. prepare, compress and decompress in one HIP graph, replayed on new chunks AND a new dictionary
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 10])
def test_dict_hc_calls_in_hip_graph(level):
    seeds = [H.C.DICT_SEED, *H.C.GRAPH_SEEDS]

    def content(seed):
        g = next(g for g in FX["groups"] if g["dict"] == H.dict_spec(4096, seed=seed))
        d = H.make_dict(g["dict"])
        ents = [e for e in g["entries"] if e[1] == level and e[2] == "bound" and e[0].startswith("bd:") and
                int(e[0][3:]) in H.CHUNK_SIZES]
        return d, ents, [H.make_chunk(e[0], d, seed) for e in ents]

    d, ents, datas = content(seeds[0])
    sizes = [len(x) for x in datas]
    assert sizes == H.CHUNK_SIZES
    n = len(sizes)
    flat, offs = pack(datas)
    dt = dict_tensor(d)
    state = new_state()
    caps = [bound(k) for k in sizes]
    ws = torch.full((4 * slot_bytes(max(sizes), level),), 0xDD, dtype=torch.uint8, device="cuda")   # 3 rounds
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        st = stream_ptr()
        assert L.lib.lz4mtHipDictPrepareHC(dptr(dt), dt.numel(), P(state.data_ptr()), state.numel(), st) == L.Result.OK
        assert L.lib.lz4mtHipCompressBatchDictHC(P(sp.data_ptr()), P(sz.data_ptr()), max(sizes), n, P(cp_.data_ptr()),
                                                 P(cc.data_ptr()), P(csz.data_ptr()), dptr(dt), dt.numel(),
                                                 P(state.data_ptr()), level, P(ws.data_ptr()), ws.numel(),
                                                 st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatchDict(P(cp_.data_ptr()), P(csz.data_ptr()), n, P(dp.data_ptr()),
                                                 P(sz.data_ptr()), P(dsz.data_ptr()), dptr(dt), dt.numel(),
                                                 st) == L.Result.OK

    def check(ents, datas, tag):
        torch.cuda.synchronize()
        cdst.fetch()
        ddst.fetch()
        got, back = csz.cpu().tolist(), dsz.cpu().tolist()
        for i, (e, x) in enumerate(zip(ents, datas)):
            assert got[i] == e[3] and sha1(cdst.data(i, e[3])) == e[4], (tag, i)
            assert back[i] == len(x) and ddst.data(i, len(x)) == x, (tag, i)
        assert cdst.canaries_ok() and ddst.canaries_ok(), tag

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # warm the library outside the capture
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
        ws.fill_(0xDD)
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
    g = main_group(65537)
    d, ents, datas = group_inputs(g, 9, only_bound=True)
    flat, offs = pack(datas)
    chunks = [flat[o:o + len(x)] for o, x in zip(offs, datas)]
    dt = dict_tensor(d)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    prepared = L.prepare_dict_hc(dt, stream=s)
    assert isinstance(prepared, L.PreparedDict) and prepared.dictionary is dt and prepared.is_hc
    assert prepared.state.numel() == L.lib.lz4mtHipDictStateSizeHC() and prepared.state.data_ptr() % 256 == 0
    outs, sizes = L.compress_batch_dict_hc(chunks, prepared, 9, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    s.synchronize()
    csz = sizes.cpu().tolist()
    assert csz == [e[3] for e in ents]
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for b, e in zip(blocks, ents):
        assert sha1(bytes(b.cpu().numpy().tobytes())) == e[4], e
    back, dsz = L.decompress_batch_dict(blocks, [len(x) for x in datas], prepared, stream=s)
    s.synchronize()
    assert dsz.cpu().tolist() == [len(x) for x in datas]
    for t, x in zip(back, datas):
        assert bytes(t.cpu().numpy().tobytes()) == x
    # explicit capacities and a caller's workspace of two slots, at level 12 with the same prepared dictionary
    third = [e for e in g["entries"] if e[1] == 12 and e[2] == "n/3"]
    assert [e[0] for e in third] == [e[0] for e in ents]
    ws = L.batch_compress_dict_workspace(max(len(x) for x in datas), 2, 12)
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.numel() == 2 * slot_bytes(max(len(x) for x in datas), 12)
    with torch.cuda.stream(s):
        ws.fill_(0)
    outs, sizes = L.compress_batch_dict_hc(chunks, prepared, 12, caps=[len(x) // 3 for x in datas], stream=s,
                                           workspace=ws)
    s.synchronize()
    assert sizes.cpu().tolist() == [e[3] for e in third]
    # the kinds do not mix
    fast = L.prepare_dict(dt, stream=s)
    assert not fast.is_hc
    with pytest.raises(TypeError):
        L.compress_batch_dict_hc(chunks, fast, 9)
    with pytest.raises(TypeError):
        L.compress_batch_dict(chunks, prepared)
    s.synchronize()


def test_empty_batch():
    dt = dict_tensor(H.make_dict(H.dict_spec(4096)))
    prepared = L.prepare_dict_hc(dt)
    outs, sizes = L.compress_batch_dict_hc([], prepared, 9)
    assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    st = P(prepared.state.data_ptr())
    for level in (3, 12):
        assert L.lib.lz4mtHipCompressBatchDictHC(None, None, 0, 0, None, None, None, dptr(dt), dt.numel(), st, level,
                                                 None, 0, stream_ptr()) == L.Result.OK
        assert L.lib.lz4mtHipCompressBatchDictHC(None, None, 0, 0, None, None, None, None, 0, st, level, None, 0,
                                                 stream_ptr()) == L.Result.OK
    # an empty dictionary tensor is no dictionary: the bytes of the fixture's 0-byte group
    none = L.prepare_dict_hc(torch.empty(0, dtype=torch.uint8, device="cuda"))
    e = next(e for e in main_group(0)["entries"] if e[:3] == ["bd:1000", 9, "bound"])
    x = H.make_chunk("bd:1000", b"")
    chunk = torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    outs, sizes = L.compress_batch_dict_hc([chunk], none, 9)
    torch.cuda.synchronize()
    k = sizes.cpu().tolist()[0]
    assert k == e[3] and sha1(bytes(outs[0][:k].cpu().numpy().tobytes())) == e[4]
