"""Host-side contract of the batched LZ4-HC compress with a set of dictionaries
(include/lz4mt_hip.h section 5e: lz4mtHipDictSetPrepareHC,
lz4mtHipCompressBatchDictSetHC), no GPU compute: the declarations, the Python
surface, and the argument checks in the header's order (null chunk arrays,
maxChunkBytes, the level, the dictionary arrays, the states, the workspace;
BAD_ARG, then ERROR without a device), each check before every later one.
"""
import ctypes
import inspect
import os
import re

import pytest

import lz4mt_amd as L
from conftest import ROOT

P = ctypes.c_void_p
ANY = P(256)   # non-null, 256-byte aligned: never dereferenced by the calls below
MAX = 4 << 20
STATE = L.lib.lz4mtHipDictStateSizeHC()
BIG = 1 << 40  # a workspace size no slot exceeds


def _prep(dp=ANY, ds=ANY, k=3, states=ANY, ssize=None):
    return L.lib.lz4mtHipDictSetPrepareHC(dp, ds, k, states, k * STATE if ssize is None else ssize, None)


def _comp(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY, dp=ANY, ds=ANY, k=3, states=ANY,
          which=ANY, level=9, ws=ANY, wsize=BIG):
    return L.lib.lz4mtHipCompressBatchDictSetHC(src, sizes, max_chunk, n, dst, caps, out, dp, ds, k, states, which,
                                                level, ws, wsize, None)


def _decl(text, name):
    m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", text)
    assert m, name
    return m.group(1), re.sub(r"\s+", " ", m.group(2))


def _slot(max_chunk, level):
    return L.lib.lz4mtHipCompressBatchDictWorkspaceSize(max_chunk, 1, level)


# later checks that are wrong as well: an earlier one must answer first either way
LATER_DICTS = [{"dp": None}, {"ds": None}]
LATER_STATES = [{"states": None}, {"states": P(1)}]
LATER_WS = [{"ws": None}, {"ws": P(128)}, {"wsize": 0}]


def test_header_declares_the_functions():
    raw = open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert _decl(text, "lz4mtHipDictSetPrepareHC") == (
        "Lz4MtResult", "const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts, "
        "void* d_statesHC, uint64_t statesSize, void* stream")
    assert _decl(text, "lz4mtHipCompressBatchDictSetHC") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes, "
        "uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, "
        "const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts, const void* d_statesHC, "
        "const uint32_t* d_chunkDict, int level, void* d_workspace, uint64_t workspaceSize, void* stream")
    # section 5e stands between 5d and 6 and holds both declarations
    a, b, c = raw.index("---- 5d."), raw.index("---- 5e."), raw.index("---- 6.")
    assert a < b < c
    sec = raw[b:c]
    assert "lz4mtHipDictSetPrepareHC(" in sec and "lz4mtHipCompressBatchDictSetHC(" in sec
    for word in ("LZ4MT_HIP_BATCH_NO_DICT", "LZ4MT_HIP_BATCH_BAD_CHUNK", "lz4mtHipDictStateSizeHC",
                 "lz4mtHipCompressBatchDictWorkspaceSize", "lz4mtHipCompressBatchEx", "graph-capturable"):
        assert word in sec, word
    # 5d points here and no longer tells the user to call once per dictionary "until" something
    assert "5e" in raw[a:b] and "Until that follow-up" not in raw


def test_abi_prototypes():
    from lz4mt_amd import _abi
    c = ctypes
    v, u32, u64, i = c.c_void_p, c.c_uint32, c.c_uint64, c.c_int
    assert _abi.PROTOTYPES["lz4mtHipDictSetPrepareHC"] == (c.c_int, [v, v, u32, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictSetHC"] == (
        c.c_int, [v, v, u32, u32, v, v, v, v, v, u32, v, v, i, v, u64, v])
    for name in ("lz4mtHipDictSetPrepareHC", "lz4mtHipCompressBatchDictSetHC"):
        assert getattr(L.lib, name).restype is c.c_int


def test_python_names_and_signatures():
    for name in ("prepare_dict_set_hc", "compress_batch_dict_set_hc"):
        assert name in L.__all__ and hasattr(L, name), name
    sig = inspect.signature(L.prepare_dict_set_hc)
    assert list(sig.parameters) == ["dictionaries", "stream"] and sig.parameters["stream"].default is None
    sig = inspect.signature(L.compress_batch_dict_set_hc)
    assert list(sig.parameters) == ["chunks", "prepared", "which", "level", "caps", "stream", "workspace"]
    assert sig.parameters["level"].default is inspect.Parameter.empty
    for name in ("caps", "stream", "workspace"):
        assert sig.parameters[name].default is None
    for slot in ("dictionaries", "ptrs", "sizes", "states", "kind"):
        assert slot in L.PreparedDictSet.__slots__
    four = L.PreparedDictSet([], None, None, None)   # the four-argument constructor
    assert four.kind == "fast" and not four.is_hc and len(four) == 0
    five = L.PreparedDictSet([], None, None, None, "hc")
    assert five.kind == "hc" and five.is_hc


def test_existing_signatures_are_unchanged():
    assert list(inspect.signature(L.prepare_dict_set).parameters) == ["dictionaries", "stream"]
    assert list(inspect.signature(L.compress_batch_dict_set).parameters) == [
        "chunks", "prepared", "which", "caps", "stream"]
    assert list(inspect.signature(L.decompress_batch_dict_set).parameters) == [
        "blocks", "caps", "dictionaries", "which", "stream"]
    assert list(inspect.signature(L.prepare_dict_hc).parameters) == ["dictionary", "stream"]
    assert list(inspect.signature(L.compress_batch_dict_hc).parameters) == [
        "chunks", "prepared", "level", "caps", "stream", "workspace"]
    assert list(inspect.signature(L.batch_compress_dict_workspace).parameters) == [
        "max_chunk", "n", "level", "device"]
    assert list(inspect.signature(L._batch).parameters) == [
        "fn_name", "srcs", "caps", "null_caps", "max_chunk", "stream", "level", "workspace", "dict_args"]
    from lz4mt_amd import _abi
    c = ctypes
    v, u32, u64 = c.c_void_p, c.c_uint32, c.c_uint64
    assert _abi.PROTOTYPES["lz4mtHipDictSetPrepare"] == (c.c_int, [v, v, u32, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictSet"] == (
        c.c_int, [v, v, u32, u32, v, v, v, v, v, u32, v, v, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictHC"] == (
        c.c_int, [v, v, u32, u32, v, v, v, v, u32, v, c.c_int, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipDictPrepareHC"] == (c.c_int, [v, u32, v, u64, v])


def test_wrappers_refuse_what_is_no_hc_set():
    fast = L.PreparedDictSet([], None, None, object())          # a set of kind "fast" that has states
    hc = L.PreparedDictSet([], None, None, object(), "hc")
    with pytest.raises(TypeError):
        L.compress_batch_dict_set_hc([], object(), [], 9)
    with pytest.raises(TypeError):   # a set built for decoding has no states
        L.compress_batch_dict_set_hc([], L.PreparedDictSet([], None, None, None, "hc"), [], 9)
    with pytest.raises(TypeError):
        L.compress_batch_dict_set_hc([], fast, [], 9)
    with pytest.raises(TypeError):
        L.compress_batch_dict_set([], hc, [])
    for level in (2, 0, -1):
        with pytest.raises(ValueError):
            L.compress_batch_dict_set_hc([], hc, [], level)
        with pytest.raises(ValueError):   # the level is looked at first
            L.compress_batch_dict_set_hc([], fast, [], level)


# ---- BAD_ARG, in the header's order ----------------------------------------
# 1. a null chunk array with nChunks > 0 (d_chunkDict counts as one; d_dstCaps may be null)
@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out", "which"])
def test_null_chunk_array_is_bad_arg(null):
    assert _comp(**{null: None}) == L.Result.BAD_ARG
    # ... before every later check, one at a time and all at once
    assert _comp(**{null: None}, max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(**{null: None}, level=2) == L.Result.BAD_ARG
    for later in LATER_DICTS + LATER_STATES + LATER_WS:
        assert _comp(**{null: None}, **later) == L.Result.BAD_ARG, later
    assert _comp(**{null: None}, max_chunk=MAX + 1, level=0, dp=None, ds=None, states=None, ws=None,
                 wsize=0) == L.Result.BAD_ARG
    assert _comp(**{null: None}, k=0, dp=None, ds=None, states=None) == L.Result.BAD_ARG


def test_null_capacities_are_allowed():
    if L.device_count() == 0:
        assert _comp(caps=None) == L.Result.ERROR        # the bound of each size: past every argument check


# 2. maxChunkBytes above the maximum
def test_max_chunk_above_the_maximum_is_bad_arg():
    assert _comp(max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, n=0) == L.Result.BAD_ARG
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0,
                 max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=(1 << 32) - 1) == L.Result.BAD_ARG
    # ... before the level, the dictionary arrays, the states and the workspace
    assert _comp(max_chunk=MAX + 1, level=2) == L.Result.BAD_ARG
    for later in LATER_DICTS + LATER_STATES + LATER_WS:
        assert _comp(max_chunk=MAX + 1, **later) == L.Result.BAD_ARG, later
    assert _comp(max_chunk=MAX + 1, level=1, dp=None, ds=None, states=None, ws=None, wsize=0) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, k=0, dp=None, ds=None, states=None) == L.Result.BAD_ARG


# 3. level < 3
@pytest.mark.parametrize("level", [2, 1, 0, -1, -(1 << 31)])
def test_level_below_3_is_bad_arg(level):
    assert _comp(level=level) == L.Result.BAD_ARG
    assert _comp(level=level, n=0) == L.Result.BAD_ARG
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0, level=level) == L.Result.BAD_ARG
    assert _comp(level=level, k=0, dp=None, ds=None, states=None) == L.Result.BAD_ARG
    # ... before the dictionary arrays, the states and the workspace
    for later in LATER_DICTS + LATER_STATES + LATER_WS:
        assert _comp(level=level, **later) == L.Result.BAD_ARG, later
    assert _comp(level=level, dp=None, ds=None, states=None, ws=None, wsize=0) == L.Result.BAD_ARG


# 4. a null d_dictPtrs or d_dictSizes with nDicts > 0
@pytest.mark.parametrize("k", [1, 3, (1 << 32) - 1])
@pytest.mark.parametrize("null", [{"dp": None}, {"ds": None}, {"dp": None, "ds": None}])
def test_null_dictionary_array_is_bad_arg(null, k):
    assert _prep(**null, k=k) == L.Result.BAD_ARG
    assert _comp(**null, k=k) == L.Result.BAD_ARG
    assert _comp(**null, k=k, n=0) == L.Result.BAD_ARG
    # ... before the states' and the workspace's checks
    assert _prep(**null, k=k, states=None) == L.Result.BAD_ARG
    assert _prep(**null, k=k, states=P(1)) == L.Result.BAD_ARG
    assert _prep(**null, k=k, ssize=0) == L.Result.BAD_ARG
    for later in LATER_STATES + LATER_WS:
        assert _comp(**null, k=k, **later) == L.Result.BAD_ARG, later
    assert _comp(**null, k=k, states=None, ws=None, wsize=0) == L.Result.BAD_ARG


# 5. the states (nDicts > 0); for prepare, statesSize
def test_bad_states_are_bad_arg():
    assert _prep(states=None) == L.Result.BAD_ARG
    assert _comp(states=None) == L.Result.BAD_ARG
    assert _comp(states=None, n=0) == L.Result.BAD_ARG
    for mis in (1, 16, 128, 256 + 64):
        assert _prep(states=P(mis)) == L.Result.BAD_ARG, mis
        assert _comp(states=P(mis)) == L.Result.BAD_ARG, mis
        assert _comp(states=P(mis), n=0) == L.Result.BAD_ARG, mis
    assert _prep(k=3, ssize=3 * STATE - 1) == L.Result.BAD_ARG
    assert _prep(k=3, ssize=STATE) == L.Result.BAD_ARG
    assert _prep(k=3, ssize=0) == L.Result.BAD_ARG
    assert _prep(k=1, ssize=L.lib.lz4mtHipDictStateSize()) == L.Result.BAD_ARG   # room for a fast state only
    # ... before the workspace's check
    for later in LATER_WS:
        assert _comp(states=None, **later) == L.Result.BAD_ARG, later
        assert _comp(states=P(64), **later) == L.Result.BAD_ARG, later


def test_states_size_product_is_64_bit():
    """nDicts * lz4mtHipDictStateSizeHC() with nDicts = 2^32 - 1 is about 1 PiB: it wraps in 32 bits (to
    2^32 - STATE: below 1 << 40) and must not."""
    k = (1 << 32) - 1
    assert k * STATE > 1 << 40 > (k * STATE) % (1 << 32)
    assert _prep(k=k, ssize=1 << 40) == L.Result.BAD_ARG
    assert _prep(k=k, ssize=(k * STATE) % (1 << 32)) == L.Result.BAD_ARG
    assert _prep(k=k, ssize=k * STATE - 1) == L.Result.BAD_ARG
    assert _prep(k=1 << 14, ssize=(1 << 14) * STATE - 1) == L.Result.BAD_ARG   # 2^14 states pass 2^32 bytes
    if L.device_count() == 0:
        assert _prep(k=k, ssize=k * STATE) == L.Result.ERROR
        assert _prep(k=1 << 14, ssize=(1 << 14) * STATE) == L.Result.ERROR


# 6. the workspace (nChunks > 0)
@pytest.mark.parametrize("level", [3, 9, 10, 12])
def test_bad_workspace_is_bad_arg(level):
    slot = _slot(65536, level)
    assert slot > 0 and slot % 256 == 0
    assert _comp(level=level, ws=None) == L.Result.BAD_ARG
    for mis in (1, 16, 128, 256 + 64):
        assert _comp(level=level, ws=P(mis)) == L.Result.BAD_ARG, mis
    assert _comp(level=level, wsize=0) == L.Result.BAD_ARG
    assert _comp(level=level, wsize=slot - 1) == L.Result.BAD_ARG
    assert _comp(level=level, n=1000, wsize=slot - 1) == L.Result.BAD_ARG
    assert _comp(level=level, k=0, dp=None, ds=None, states=None, ws=None) == L.Result.BAD_ARG
    if level >= 10:   # a slot of level 9 is too small from level 10 up (the price table)
        assert _comp(level=level, wsize=_slot(65536, 9)) == L.Result.BAD_ARG


# then: ERROR without a device; what launches nothing is OK with one
def test_valid_arguments_without_gpu():
    expect = L.Result.ERROR if L.device_count() == 0 else L.Result.OK
    # nDicts == 0 with null dictionary arrays and null states, nChunks == 0 with null chunk arrays and no workspace:
    # valid.  With a device these launch nothing, so the placeholder pointers are never read.
    assert _prep(k=0, dp=None, ds=None, states=None, ssize=0) == expect
    assert _prep(k=0) == expect
    assert _prep(k=0, states=P(1), ssize=0) == expect
    none = dict(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0)
    assert _comp(**none) == expect
    assert _comp(**none, ws=None, wsize=0) == expect
    assert _comp(**none, ws=P(1), wsize=0) == expect
    assert _comp(**none, k=0, dp=None, ds=None, states=None, ws=None, wsize=0) == expect
    assert _comp(**none, level=12) == expect
    assert _comp(**none, level=1 << 20) == expect          # above 12 counts as 12
    if L.device_count() > 0:
        return   # the calls below would launch kernels over the placeholder pointers
    assert _prep() == L.Result.ERROR
    assert _prep(k=1) == L.Result.ERROR
    assert _prep(ssize=1 << 50) == L.Result.ERROR
    for level in (3, 9, 10, 12, 100):
        assert _comp(level=level) == L.Result.ERROR
        assert _comp(level=level, wsize=_slot(65536, level)) == L.Result.ERROR     # one slot is enough
        assert _comp(level=level, n=1000, wsize=_slot(65536, level)) == L.Result.ERROR
    assert _comp(k=0, dp=None, ds=None, states=None) == L.Result.ERROR     # every chunk NO_DICT
    assert _comp(k=0, states=P(1)) == L.Result.ERROR                       # no states are needed for no dictionaries
    assert _comp(max_chunk=MAX, n=1000) == L.Result.ERROR
    assert _comp(max_chunk=0) == L.Result.ERROR
