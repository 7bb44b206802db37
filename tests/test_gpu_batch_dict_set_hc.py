"""Batched LZ4-HC compress with a set of dictionaries and an index per chunk
(include/lz4mt_hip.h section 5e: lz4mtHipDictSetPrepareHC,
lz4mtHipCompressBatchDictSetHC; kernels k_hc_dict_set_prepare,
k_hc_prev_batch<HcDictSet>, k_encode_hc_batch<HcDictSet>,
k_encode_hc_opt_batch<HcDictSet>).

The reference is liblz4 1.9.3 itself, through the committed fixtures
tests/golden/dict_hc_blocks.json and dict_hc_fuzz.json (LZ4_loadDictHC +
LZ4_compress_HC_continue on a fresh stream per chunk; pinned on hosts with
liblz4 by test_dict_hc_golden.py) -- never the library's other paths, except
where a test is by its name an equality between two calls.  Here every
dictionary of a fixture goes into ONE set and every entry of a level into ONE
call.  Inputs are packed as test_gpu_batch_dict_hc.py packs them (chunk starts
at every offset mod 16, the last chunk on the tensor's last byte, 32 canary
bytes after every capacity, every dictionary at an odd address ending on its
tensor's last byte); every block that fits is decoded back on the device with
one lz4mtHipDecompressBatchDictSet call.
"""
import ctypes
import functools
import json
import os
import random

import numpy as np
import pytest
import torch

import dict_hc_cases as H
import test_gpu_batch_dict_hc as HC
from conftest import GOLDEN
from test_gpu_batch import BAD, FILL, Dst, bound, i64, pack, stream_ptr, u32
from test_gpu_batch_dict_hc import dict_tensor, dptr, sha1, slot_bytes

pytestmark = pytest.mark.gpu

L = None
P = ctypes.c_void_p
NO_DICT = 0xFFFFFFFF
with open(os.path.join(GOLDEN, "dict_hc_blocks.json")) as _f:
    FX = json.load(_f)
with open(os.path.join(GOLDEN, "dict_hc_fuzz.json")) as _f:
    FZ = json.load(_f)
GROUPS = FX["groups"]
LEVELS = sorted({e[1] for g in GROUPS for e in g["entries"]})
FUZZ_LEVELS = sorted({c[4] for c in FZ["cases"]})


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = HC.L = lz4mt_amd   # the helpers of that module call the library through their module's handle
    assert L.device_count() > 0 and L.BATCH_NO_DICT == NO_DICT
    return L


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def state_size():
    return L.lib.lz4mtHipDictStateSizeHC()


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
        assert L.lib.lz4mtHipDictSetPrepareHC(*self.args(), P(states.data_ptr()), states.numel(),
                                              stream_ptr()) == L.Result.OK
        return states


def set_compress(flat, soffs, sizes, caps, max_chunk, ds, states, which, level, null_caps=False, dst=None,
                 dst_ptrs=None, src_ptrs=None, slots=None):
    """One lz4mtHipCompressBatchDictSetHC with a workspace of ``slots`` slots (default: the full size)."""
    dst = dst or Dst(caps)
    sp = i64(src_ptrs if src_ptrs is not None else [flat.data_ptr() + o for o in soffs])
    dp = i64(dst_ptrs if dst_ptrs is not None else dst.ptrs)
    sz, cp, wh = u32(sizes), u32(caps), u32(which)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    nbytes = L.lib.lz4mtHipCompressBatchDictWorkspaceSize(max_chunk, len(sizes), level) if slots is None else \
        slots * slot_bytes(max_chunk, level)
    ws = torch.full((nbytes,), 0xDD, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    r = L.lib.lz4mtHipCompressBatchDictSetHC(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes),
                                             P(dp.data_ptr()), P(None if null_caps else cp.data_ptr()),
                                             P(out.data_ptr()), *ds.args(),
                                             P(states.data_ptr() if states is not None else None), P(wh.data_ptr()),
                                             level, P(ws.data_ptr()), ws.numel(), stream_ptr())
    assert r == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def ex_compress(flat, soffs, sizes, caps, max_chunk, level):
    """One lz4mtHipCompressBatchEx (no dictionary) with its full workspace."""
    dst = Dst(caps)
    sp, dp = i64([flat.data_ptr() + o for o in soffs]), i64(dst.ptrs)
    sz, cp = u32(sizes), u32(caps)
    out = torch.full((len(sizes),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ws = torch.full((L.lib.lz4mtHipCompressBatchWorkspaceSize(max_chunk, len(sizes), level),), 0xDD,
                    dtype=torch.uint8, device="cuda")
    assert L.lib.lz4mtHipCompressBatchEx(P(sp.data_ptr()), P(sz.data_ptr()), max_chunk, len(sizes), P(dp.data_ptr()),
                                         P(cp.data_ptr()), P(out.data_ptr()), level, P(ws.data_ptr()), ws.numel(),
                                         stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
    dst.fetch()
    return out.cpu().tolist(), dst


def decode_back(cdst, got, datas, ds, which, tag):
    """Every block of ``cdst`` that fits (got > 0), where the encoder left it, back to its source: one
    lz4mtHipDecompressBatchDictSet call over the same set and the same indices."""
    keep = [i for i, r in enumerate(got) if r > 0]
    if not keep:
        return
    sizes = [len(datas[i]) for i in keep]
    ddst = Dst(sizes)
    sp, dp = i64([cdst.ptrs[i] for i in keep]), i64(ddst.ptrs)
    csz, cp, wh = u32([got[i] for i in keep]), u32(sizes), u32([which[i] for i in keep])
    out = torch.full((len(keep),), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert L.lib.lz4mtHipDecompressBatchDictSet(P(sp.data_ptr()), P(csz.data_ptr()), len(keep), P(dp.data_ptr()),
                                                P(cp.data_ptr()), P(out.data_ptr()), *ds.args(), P(wh.data_ptr()),
                                                stream_ptr()) == L.Result.OK
    torch.cuda.synchronize()
    ddst.fetch()
    assert out.cpu().tolist() == sizes, tag
    for k, i in enumerate(keep):
        assert ddst.data(k, sizes[k]) == datas[i], (tag, i)
    assert ddst.canaries_ok(), tag


def spread(groups):
    """[(group, item)] of every item of every group, ordered so that neighbours come from different groups
    wherever more than one group has items left: always the fullest group other than the last one taken."""
    left = [list(reversed(g)) for g in groups]
    out, last = [], -1
    while any(left):
        cand = [i for i in range(len(left)) if left[i] and i != last] or [last]
        k = max(cand, key=lambda i: len(left[i]))
        out.append((k, left[k].pop()))
        last = k
    return out


@functools.lru_cache(maxsize=None)
def fixture_dicts():
    return tuple(H.make_dict(g["dict"]) for g in GROUPS)


@functools.lru_cache(maxsize=None)
def fixture_chunk(gi, name):
    return H.make_chunk(name, fixture_dicts()[gi], GROUPS[gi]["dict"]["seed"])


def group_index(size, seed=H.C.DICT_SEED):
    return next(i for i, g in enumerate(GROUPS) if g["dict"] == H.dict_spec(size, seed=seed))


def bound_entries(gi, level, max_size=None):
    """The entries of group ``gi`` at ``level`` and the bound capacity, optionally the small chunks only."""
    ents = [e for e in GROUPS[gi]["entries"] if e[1] == level and e[2] == "bound"]
    return [e for e in ents if max_size is None or len(fixture_chunk(gi, e[0])) <= max_size]


def check_entries(ents, got, dst, tag):
    for i, e in enumerate(ents):
        assert got[i] == e[3], (tag, i, e, got[i])
        assert sha1(dst.data(i, e[3])) == e[4], (tag, i, e)
    assert dst.canaries_ok(), tag


# ---------------------------------------------------------------------------
# 1. the fixture: one set of all its dictionaries, one call per level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_fixture_one_call_per_level(level):
    dicts = fixture_dicts()
    assert len(dicts) == 24 and len(dicts[0]) == 0
    order = spread([[e for e in g["entries"] if e[1] == level] for g in GROUPS])
    assert len(order) == sum(1 for g in GROUPS for e in g["entries"] if e[1] == level)
    if len({k for k, _ in order}) > 1:
        assert all(a[0] != b[0] for a, b in zip(order, order[1:]))
    # the 0-byte dictionary's entries: every other one through its index, the others without a dictionary
    which, zero = [], 0
    for k, _ in order:
        if k == 0:
            zero += 1
        which.append(NO_DICT if k == 0 and zero % 2 == 0 else k)
    if level in H.LEVELS_MAIN:
        assert which.count(NO_DICT) >= 6 and which.count(0) >= 6
    ents = [e for _, e in order]
    datas = [fixture_chunk(k, e[0]) for k, e in order]
    flat, offs = pack(datas)
    sizes = [len(x) for x in datas]
    caps = [H.cap_of(e[2], n) for e, n in zip(ents, sizes)]
    ds = DictSet(dicts)
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, ds.prepare(), which, level)
    check_entries(ents, got, dst, level)
    decode_back(dst, got, datas, ds, which, level)


# ---------------------------------------------------------------------------
# 2. the seeded differential fixture: one set of its 9 dictionaries prepared once, one call per level
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuzz_set():
    dicts = [H.make_dict(s) for s in FZ["dicts"]]
    ds = DictSet(dicts)
    return dicts, ds, ds.prepare()


@pytest.mark.parametrize("level", FUZZ_LEVELS)
def test_seeded_cases(level):
    assert len(FZ["cases"]) == 500 and len(FZ["dicts"]) == 9 and FUZZ_LEVELS == list(range(3, 13))
    dicts, ds, states = fuzz_set()
    order = spread([[c for c in FZ["cases"] if c[0] == di and c[4] == level] for di in range(len(dicts))])
    assert order
    which = [k for k, _ in order]
    cases = [c for _, c in order]
    datas = [H.fuzz_chunk(c[1], c[2], c[3], dicts[c[0]]) for c in cases]
    flat, offs = pack(datas)
    caps = [H.cap_of(c[5], c[2]) for c in cases]
    got, dst = set_compress(flat, offs, [c[2] for c in cases], caps, H.FUZZ_MAX_CHUNK, ds, states, which, level)
    for i, c in enumerate(cases):
        assert got[i] == c[6], (c, got[i])
        assert sha1(dst.data(i, c[6])) == c[7], c
    assert dst.canaries_ok(), level
    decode_back(dst, got, datas, ds, which, level)


# ---------------------------------------------------------------------------
# 3. states: byte for byte lz4mtHipDictPrepareHC's, and valid for either call
# ---------------------------------------------------------------------------
def test_states_equal_the_single_prepare():
    dicts = fixture_dicts()
    assert {len(d) for d in dicts} == set(H.DICT_SIZES)
    ds = DictSet(dicts)
    states = ds.prepare()
    singles = [HC.prepare(t) for t in ds.tensors]
    torch.cuda.synchronize()
    S = state_size()
    host = states.cpu().numpy()
    for k, one in enumerate(singles):
        assert host[k * S:(k + 1) * S].tobytes() == one.cpu().numpy().tobytes(), GROUPS[k]["dict"]
    for level in (9, 12):
        # single states laid out as a set, under the set call
        picks = spread([[(gi, e) for e in bound_entries(gi, level, 4096)]
                        for gi in (group_index(4096), group_index(65537), group_index(5))])
        picks = [p for _, p in picks]
        assert len(picks) >= 27
        ents = [e for _, e in picks]
        which = [gi for gi, _ in picks]
        datas = [fixture_chunk(gi, e[0]) for gi, e in picks]
        flat, offs = pack(datas)
        sizes = [len(x) for x in datas]
        caps = [bound(n) for n in sizes]
        laid = torch.cat(singles)
        assert laid.data_ptr() % 256 == 0 and laid.numel() == len(dicts) * S
        got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, laid, which, level)
        check_entries(ents, got, dst, ("single states under the set call", level))
        # a state cut out of the set's, under the shared-dictionary call
        gi = group_index(65537)
        mine = [i for i, k in enumerate(which) if k == gi]
        got, dst = HC.compress_call(flat, [offs[i] for i in mine], [sizes[i] for i in mine], [caps[i] for i in mine],
                                    max(sizes), ds.tensors[gi], states[gi * S:(gi + 1) * S], level)
        check_entries([ents[i] for i in mine], got, dst, ("a set state under the shared-dictionary call", level))


# ---------------------------------------------------------------------------
# 4. the index decides: one chunk under three dictionaries and none, in one call
#    (an equality between calls: the set call against the single-dictionary call and lz4mtHipCompressBatchEx)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [9, 12])
def test_one_chunk_under_three_dictionaries_and_none(level):
    d0 = H.make_dict(H.dict_spec(4096))
    d1 = H.make_dict(H.dict_spec(4096, seed=6))
    d2 = H.make_dict(H.dict_spec(65536))
    assert d0 != d1 and d0 != d2[-4096:]
    chunk = H.make_chunk("bd:1500", d0) + d1[100:900] + d0[2000:2900] + d2[300:1200] + d1[-64:] + \
        H.make_chunk("bd:700", d1, 6)
    n = len(chunk)
    flat, offs = pack([chunk] * 4)
    ds = DictSet([d0, d1, d2])
    which = [0, 1, 2, NO_DICT]
    got, dst = set_compress(flat, offs, [n] * 4, [bound(n)] * 4, n, ds, ds.prepare(), which, level)
    blocks = [dst.data(i, got[i]) for i in range(4)]
    assert all(0 < r < n for r in got) and len(set(blocks)) == 4
    assert dst.canaries_ok()
    for k in range(3):
        one, odst = HC.compress_call(flat, offs[k:k + 1], [n], [bound(n)], n, ds.tensors[k], HC.prepare(ds.tensors[k]),
                                     level)
        assert one[0] == got[k] and odst.data(0, one[0]) == blocks[k], k
    ex, edst = ex_compress(flat, offs[3:], [n], [bound(n)], n, level)
    assert ex[0] == got[3] and edst.data(0, ex[0]) == blocks[3]
    decode_back(dst, got, [chunk] * 4, ds, which, level)


# ---------------------------------------------------------------------------
# 5. rounds: a one-slot workspace gives the full workspace's bytes (a round slices d_chunkDict too)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 10])
def test_rounds_slice_the_index_array(level):
    rnd = random.Random(100 + level)
    dicts = [H.make_dict(H.dict_spec(s, seed=seed)) for s, seed in ((4096, 5), (4096, 6), (65536, 5), (300, 7), (0, 5))]
    pool = H.make_chunk("bd:300000", dicts[0]) + H.make_chunk("mixed:70000", dicts[0]) + dicts[2] + dicts[1]
    datas, which = [b"", pool[:3], pool[5:18]], [0, 1, 2]
    while len(datas) < 400:
        n = rnd.choice([rnd.randrange(0, 300), rnd.randrange(300, 2049), 2048])
        a = rnd.randrange(len(pool) - n)
        datas.append(pool[a:a + n])
        which.append(rnd.choice([0, 1, 2, 3, 4, NO_DICT]))
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    ds = DictSet(dicts)
    states = ds.prepare()
    full, fdst = set_compress(flat, offs, sizes, caps, max(sizes), ds, states, which, level)
    assert all(0 < r <= c for r, c in zip(full, caps)) and fdst.canaries_ok()
    decode_back(fdst, full, datas, ds, which, ("full", level))
    one, odst = set_compress(flat, offs, sizes, caps, max(sizes), ds, states, which, level, slots=1)   # 400 rounds
    assert one == full and odst.canaries_ok()
    assert torch.equal(odst.back, fdst.back)    # identical bytes, slot by slot
    # the dictionaries matter here: the same chunks all under dictionary 0 give other sizes
    same, _ = set_compress(flat, offs, sizes, caps, max(sizes), ds, states, [0] * len(sizes), level, slots=7)
    assert same != full


# ---------------------------------------------------------------------------
# 6. per-chunk refusals beside good chunks
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [9, 12])
def test_per_chunk_refusals_beside_good_chunks(level):
    g4, g0 = group_index(4096), 0
    d = fixture_dicts()[g4]
    other = H.make_dict(H.dict_spec(5000, seed=6))
    # 0 good | 1 null pointer of size 4096 | 2 prepared for 4096 bytes, listed with 5000 | 3 a fast state's bytes
    # | 4 unprepared | 5 good again (the same dictionary)
    ds = DictSet([d, d, other, d, d, d])
    ds.ptr_list[1] = 0
    ds.size_list[2] = 4096
    ds.upload()
    states = ds.prepare()
    S = state_size()
    fast = torch.full((L.lib.lz4mtHipDictStateSize(),), 0xCC, dtype=torch.uint8, device="cuda")
    assert L.lib.lz4mtHipDictPrepare(dptr(ds.tensors[3]), 4096, P(fast.data_ptr()), fast.numel(),
                                     stream_ptr()) == L.Result.OK
    states[3 * S:4 * S].fill_(0)
    states[3 * S:3 * S + fast.numel()].copy_(fast)
    states[4 * S:5 * S].fill_(0xCC)
    torch.cuda.synchronize()
    words = states.cpu().numpy().view(np.uint32).reshape(6, S // 4)
    assert words[0, 1] == 4096 and words[2, 1] == 4096 and words[5, 1] == 4096 and words[0, 0] == words[5, 0]
    assert words[1, 1] == 0xFFFFFFFF                       # no effective size: a state no dictionary matches
    assert (words[0] == words[5]).all()
    ds.size_list[2] = 5000
    ds.upload()

    good = bound_entries(g4, level, 4096)
    plain = bound_entries(g0, level, 4096)
    assert len(good) >= 9 and len(plain) >= 9
    # (group, entry or None, index, why refused or None)
    items = []
    for i, e in enumerate(good):
        items.append((g4, e, 0 if i % 2 else 5, None))
    for e in plain:
        items.append((g0, e, NO_DICT, None))
    text = next(e for e in good if e[0] == "bd:1000")
    for k, why in ((6, "index == nDicts"), (0xFFFFFFFE, "index 0xFFFFFFFE"), (1, "null dictionary"),
                   (2, "state of another size"), (3, "fast state"), (4, "unprepared state")):
        items.append((g4, text, k, why))
    for why in ("misaligned destination", "null destination", "null source", "above maxChunkBytes"):
        items.append((g4, text if why != "above maxChunkBytes" else ["bd:65535"], 0, why))
    rnd = random.Random(level)
    rnd.shuffle(items)
    while any(a[3] and b[3] for a, b in zip(items, items[1:])):   # every refusal beside good chunks
        rnd.shuffle(items)
    datas = [fixture_chunk(gi, e[0]) for gi, e, _, _ in items]
    sizes = [len(x) for x in datas]
    caps = [bound(n) for n in sizes]
    which = [k for _, _, k, _ in items]
    flat, offs = pack(datas)
    dst = Dst(caps)
    ptrs = list(dst.ptrs)
    sptrs = [flat.data_ptr() + o for o in offs]
    for i, (_, _, _, why) in enumerate(items):
        if why == "misaligned destination":
            ptrs[i] += 8
        elif why == "null destination":
            ptrs[i] = 0
        elif why == "null source":
            sptrs[i] = 0
    got, dst = set_compress(flat, offs, sizes, caps, 4096, ds, states, which, level, dst=dst, dst_ptrs=ptrs,
                            src_ptrs=sptrs, slots=3)
    for i, (_, e, k, why) in enumerate(items):
        if why:
            assert got[i] == BAD, (why, got[i])
            assert dst.untouched_from(i, 0), why
        else:
            assert got[i] == e[3] and sha1(dst.data(i, e[3])) == e[4], (i, e, k)
    assert dst.canaries_ok()
    assert sum(1 for it in items if it[3]) == 10


# ---------------------------------------------------------------------------
# 7. no dictionaries at all: null dictionary arrays, null states, every chunk LZ4MT_HIP_BATCH_NO_DICT
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 9, 10, 12])
def test_no_dictionaries_at_all(level):
    ents = bound_entries(0, level)
    datas = [fixture_chunk(0, e[0]) for e in ents]
    sizes = [len(x) for x in datas]
    assert max(sizes) == 70000 and 0 in sizes
    caps = [bound(n) for n in sizes]
    flat, offs = pack(datas)
    ds = DictSet([])
    assert ds.k == 0 and ds.args()[0].value is None and ds.args()[1].value is None
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, None, [NO_DICT] * len(sizes), level)
    check_entries(ents, got, dst, level)           # liblz4: no dictionary loaded
    ex, edst = ex_compress(flat, offs, sizes, caps, max(sizes), level)
    assert ex == got and torch.equal(edst.back, dst.back)   # the bytes of lz4mtHipCompressBatchEx
    # an index needs a dictionary to name
    got, dst = set_compress(flat, offs, sizes, caps, max(sizes), ds, None, [0] * len(sizes), level)
    assert got == [BAD] * len(sizes) and all(dst.untouched_from(i, 0) for i in range(len(sizes)))


# ---------------------------------------------------------------------------
# 8. prepare, compress and decompress in one linear HIP graph, replayed on new chunks, indices and dictionary bytes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [3, 10])
def test_set_hc_calls_in_hip_graph(level):
    seeds = [H.C.DICT_SEED, *H.C.GRAPH_SEEDS]

    def content(seed):
        gi = group_index(4096, seed=seed)
        ents = [e for e in GROUPS[gi]["entries"] if e[1] == level and e[2] == "bound" and e[0].startswith("bd:") and
                int(e[0][3:]) in H.CHUNK_SIZES]
        return fixture_dicts()[gi], ents, [fixture_chunk(gi, e[0]) for e in ents]

    d, ents, datas = content(seeds[0])
    sizes = [len(x) for x in datas]
    assert sizes == H.CHUNK_SIZES
    n = len(sizes)
    flat, offs = pack(datas)
    # dictionary 0 keeps seed 5's bytes, dictionary 1 holds seed 6's, dictionary 2 is rewritten in place
    ds = DictSet([d, content(seeds[1])[0], d])
    states = ds.new_states()
    caps = [bound(k) for k in sizes]
    ws = torch.full((4 * slot_bytes(max(sizes), level),), 0xDD, dtype=torch.uint8, device="cuda")   # 3 rounds
    cdst, ddst = Dst(caps), Dst(sizes)
    sp, cp_, dp = i64([flat.data_ptr() + o for o in offs]), i64(cdst.ptrs), i64(ddst.ptrs)
    sz, cc = u32(sizes), u32(caps)
    which = [0 if i % 2 else 2 for i in range(n)]
    wh = u32(which)
    csz = torch.zeros(n, dtype=torch.int32, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        st = stream_ptr()
        assert L.lib.lz4mtHipDictSetPrepareHC(*ds.args(), P(states.data_ptr()), states.numel(), st) == L.Result.OK
        assert L.lib.lz4mtHipCompressBatchDictSetHC(P(sp.data_ptr()), P(sz.data_ptr()), max(sizes), n,
                                                    P(cp_.data_ptr()), P(cc.data_ptr()), P(csz.data_ptr()),
                                                    *ds.args(), P(states.data_ptr()), P(wh.data_ptr()), level,
                                                    P(ws.data_ptr()), ws.numel(), st) == L.Result.OK
        assert L.lib.lz4mtHipDecompressBatchDictSet(P(cp_.data_ptr()), P(csz.data_ptr()), n, P(dp.data_ptr()),
                                                    P(sz.data_ptr()), P(dsz.data_ptr()), *ds.args(),
                                                    P(wh.data_ptr()), st) == L.Result.OK

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
    for r, seed in enumerate(seeds[1:], 1):
        d2, ents2, datas2 = content(seed)
        assert d2 != d and len(d2) == len(d)
        new, offs2 = pack(datas2)
        assert offs2 == offs
        flat.copy_(new)                                                           # the chunks
        ds.tensors[2].copy_(torch.frombuffer(bytearray(d2), dtype=torch.uint8))   # one dictionary's bytes
        which2 = [(1 if i % 2 else 2) for i in range(n)] if r == 1 else [2] * n   # the indices
        assert which2 != which
        wh.copy_(u32(which2))
        states.fill_(0xCC)
        ws.fill_(0xDD)
        cdst.back.fill_(FILL)
        ddst.back.fill_(FILL)
        csz.zero_()
        dsz.zero_()
        g.replay()
        check(ents2, datas2, f"replay, dictionary seed {seed}")


# ---------------------------------------------------------------------------
# 9. the Python wrappers on a side stream, and the empty batch
# ---------------------------------------------------------------------------
def test_python_wrappers_on_side_stream():
    gis = [group_index(65537), 0, group_index(4096)]
    tensors = [dict_tensor(fixture_dicts()[gi]) for gi in gis]
    names = [e[0] for e in bound_entries(gis[0], 9)]
    picks = [(j if (i + j) % 4 else None, gis[j], name) for i, name in enumerate(names) for j in range(3)]
    which = [w for w, _, _ in picks]
    assert None in which and {0, 1, 2} <= set(which)

    def entry(w, gi, name, level, kind):   # without a dictionary: the 0-byte group's answer
        return next(e for e in GROUPS[gi if w is not None else 0]["entries"] if e[:3] == [name, level, kind])

    datas = [fixture_chunk(gi, name) for _, gi, name in picks]
    flat, offs = pack(datas)
    chunks = [flat[o:o + len(x)] for o, x in zip(offs, datas)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    prepared = L.prepare_dict_set_hc(tensors, stream=s)
    assert isinstance(prepared, L.PreparedDictSet) and len(prepared) == 3 and prepared.is_hc and prepared.kind == "hc"
    assert all(a is b for a, b in zip(prepared.dictionaries, tensors))
    assert prepared.states.numel() == 3 * state_size() and prepared.states.data_ptr() % 256 == 0
    assert prepared.ptrs.dtype == torch.int64 and prepared.sizes.dtype == torch.int32
    outs, sizes = L.compress_batch_dict_set_hc(chunks, prepared, which, 9, stream=s)
    assert sizes.dtype == torch.int32 and sizes.is_cuda and len(outs) == len(chunks)
    assert all(o.data_ptr() % 16 == 0 and o.numel() == bound(c.numel()) for o, c in zip(outs, chunks))
    s.synchronize()
    csz = sizes.cpu().tolist()
    want = [entry(w, gi, name, 9, "bound") for w, gi, name in picks]
    assert csz == [e[3] for e in want]
    blocks = [o[:k] for o, k in zip(outs, csz)]
    for b, e in zip(blocks, want):
        assert sha1(bytes(b.cpu().numpy().tobytes())) == e[4], e
    for dictionaries in (prepared, tensors):   # a set of kind "hc" serves the decoder: only its dictionaries count
        back, dsz = L.decompress_batch_dict_set(blocks, [len(x) for x in datas], dictionaries, which, stream=s)
        s.synchronize()
        assert dsz.cpu().tolist() == [len(x) for x in datas]
        for t, x in zip(back, datas):
            assert bytes(t.cpu().numpy().tobytes()) == x
    # explicit capacities and a caller's workspace of two slots, at level 12 with the same prepared set
    big = max(len(x) for x in datas)
    ws = L.batch_compress_dict_workspace(big, 2, 12)
    assert ws.numel() == 2 * slot_bytes(big, 12)
    with torch.cuda.stream(s):
        ws.fill_(0)
    outs, sizes = L.compress_batch_dict_set_hc(chunks, prepared, which, 12, caps=[len(x) // 3 for x in datas],
                                               stream=s, workspace=ws)
    s.synchronize()
    assert sizes.cpu().tolist() == [entry(w, gi, name, 12, "n/3")[3] for w, gi, name in picks]
    # the kinds do not mix
    fast = L.prepare_dict_set(tensors, stream=s)
    assert not fast.is_hc and fast.kind == "fast"
    with pytest.raises(TypeError):
        L.compress_batch_dict_set_hc(chunks, fast, which, 9)
    with pytest.raises(TypeError):
        L.compress_batch_dict_set(chunks, prepared, which)
    with pytest.raises(ValueError):
        L.compress_batch_dict_set_hc(chunks, prepared, which, 2)
    with pytest.raises(ValueError):
        L.compress_batch_dict_set_hc(chunks, prepared, [3] * len(chunks), 9, stream=s)
    s.synchronize()


def test_empty_batch_and_empty_set():
    dt = dict_tensor(H.make_dict(H.dict_spec(4096)))
    prepared = L.prepare_dict_set_hc([dt])
    outs, sizes = L.compress_batch_dict_set_hc([], prepared, [], 9)
    assert outs == [] and sizes.numel() == 0 and sizes.dtype == torch.int32
    dp, dsz, st = P(prepared.ptrs.data_ptr()), P(prepared.sizes.data_ptr()), P(prepared.states.data_ptr())
    for level in (3, 12):
        assert L.lib.lz4mtHipCompressBatchDictSetHC(None, None, 0, 0, None, None, None, dp, dsz, 1, st, None, level,
                                                    None, 0, stream_ptr()) == L.Result.OK
    assert L.lib.lz4mtHipDictSetPrepareHC(None, None, 0, None, 0, stream_ptr()) == L.Result.OK
    # the empty set: every chunk names no dictionary, and gets the 0-byte group's bytes
    none = L.prepare_dict_set_hc([])
    assert len(none) == 0 and none.states.numel() == 0 and none.is_hc
    e = next(e for e in GROUPS[0]["entries"] if e[:3] == ["bd:1000", 9, "bound"])
    x = fixture_chunk(0, "bd:1000")
    chunk = torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    outs, sizes = L.compress_batch_dict_set_hc([chunk], none, [None], 9)
    torch.cuda.synchronize()
    k = sizes.cpu().tolist()[0]
    assert k == e[3] and sha1(bytes(outs[0][:k].cpu().numpy().tobytes())) == e[4]
