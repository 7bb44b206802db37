"""Host-side contract of the batched operators with a set of dictionaries
(include/lz4mt_hip.h section 5d: lz4mtHipDictSetPrepare,
lz4mtHipCompressBatchDictSet, lz4mtHipDecompressBatchDictSet), no GPU
compute: the declarations, the Python surface, and the argument checks in the
header's order (null chunk arrays, maxChunkBytes, the dictionary arrays, the
states; BAD_ARG, then ERROR without a device), each check before every later
one.
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
STATE = L.lib.lz4mtHipDictStateSize()


def _prep(dp=ANY, ds=ANY, k=3, states=ANY, ssize=None):
    return L.lib.lz4mtHipDictSetPrepare(dp, ds, k, states, k * STATE if ssize is None else ssize, None)


def _comp(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY, dp=ANY, ds=ANY, k=3, states=ANY,
          which=ANY):
    return L.lib.lz4mtHipCompressBatchDictSet(src, sizes, max_chunk, n, dst, caps, out, dp, ds, k, states, which, None)


def _dec(src=ANY, sizes=ANY, n=1, dst=ANY, caps=ANY, out=ANY, dp=ANY, ds=ANY, k=3, which=ANY):
    return L.lib.lz4mtHipDecompressBatchDictSet(src, sizes, n, dst, caps, out, dp, ds, k, which, None)


def _decl(text, name):
    m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", text)
    assert m, name
    return m.group(1), re.sub(r"\s+", " ", m.group(2))


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read(), flags=re.S)
    assert _decl(text, "lz4mtHipDictSetPrepare") == (
        "Lz4MtResult", "const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts, "
        "void* d_states, uint64_t statesSize, void* stream")
    assert _decl(text, "lz4mtHipCompressBatchDictSet") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes, "
        "uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, "
        "const void* const* d_dictPtrs, const uint32_t* d_dictSizes, uint32_t nDicts, const void* d_states, "
        "const uint32_t* d_chunkDict, void* stream")
    assert _decl(text, "lz4mtHipDecompressBatchDictSet") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t nChunks, "
        "void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, const void* const* d_dictPtrs, "
        "const uint32_t* d_dictSizes, uint32_t nDicts, const uint32_t* d_chunkDict, void* stream")
    assert re.search(r"#define LZ4MT_HIP_BATCH_NO_DICT UINT32_MAX\b", text)
    assert L.BATCH_NO_DICT == 0xFFFFFFFF


def test_header_names_the_hc_follow_up():
    text = open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read()
    sec = text[text.index("---- 5d."):text.index("---- 6.")]
    assert "LZ4-HC" in sec and "follow-up" in sec and "lz4mtHipCompressBatchDictHC" in sec


def test_abi_prototypes():
    from lz4mt_amd import _abi
    c = ctypes
    v, u32, u64 = c.c_void_p, c.c_uint32, c.c_uint64
    assert _abi.BATCH_NO_DICT == 0xFFFFFFFF
    assert _abi.PROTOTYPES["lz4mtHipDictSetPrepare"] == (c.c_int, [v, v, u32, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictSet"] == (
        c.c_int, [v, v, u32, u32, v, v, v, v, v, u32, v, v, v])
    assert _abi.PROTOTYPES["lz4mtHipDecompressBatchDictSet"] == (c.c_int, [v, v, u32, v, v, v, v, v, u32, v, v])
    for name in ("lz4mtHipDictSetPrepare", "lz4mtHipCompressBatchDictSet", "lz4mtHipDecompressBatchDictSet"):
        assert getattr(L.lib, name).restype is c.c_int


def test_python_names_and_signatures():
    for name in ("BATCH_NO_DICT", "PreparedDictSet", "prepare_dict_set", "compress_batch_dict_set",
                 "decompress_batch_dict_set"):
        assert name in L.__all__ and hasattr(L, name), name
    sig = inspect.signature(L.prepare_dict_set)
    assert list(sig.parameters) == ["dictionaries", "stream"] and sig.parameters["stream"].default is None
    sig = inspect.signature(L.compress_batch_dict_set)
    assert list(sig.parameters) == ["chunks", "prepared", "which", "caps", "stream"]
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(L.decompress_batch_dict_set)
    assert list(sig.parameters) == ["blocks", "caps", "dictionaries", "which", "stream"]
    assert sig.parameters["stream"].default is None
    for slot in ("dictionaries", "ptrs", "sizes", "states"):
        assert slot in L.PreparedDictSet.__slots__


def test_existing_signatures_are_unchanged():
    assert list(inspect.signature(L.prepare_dict).parameters) == ["dictionary", "stream"]
    assert list(inspect.signature(L.compress_batch_dict).parameters) == ["chunks", "prepared", "caps", "stream"]
    assert list(inspect.signature(L.decompress_batch_dict).parameters) == ["blocks", "caps", "dictionary", "stream"]
    assert list(inspect.signature(L._batch).parameters) == [
        "fn_name", "srcs", "caps", "null_caps", "max_chunk", "stream", "level", "workspace", "dict_args"]


def test_wrappers_refuse_what_is_no_set():
    with pytest.raises(TypeError):
        L.compress_batch_dict_set([], object(), [])
    with pytest.raises(TypeError):   # a set built for decoding has no states
        L.compress_batch_dict_set([], L.PreparedDictSet([], None, None, None), [])


# ---- BAD_ARG, in the header's order ----------------------------------------
# 1. a null chunk array with nChunks > 0 (d_chunkDict counts as one)
@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out", "which"])
def test_null_chunk_array_is_bad_arg(null):
    assert _comp(**{null: None}) == L.Result.BAD_ARG
    assert _dec(**{null: None}) == L.Result.BAD_ARG
    # ... before every later check, one at a time and all at once
    assert _comp(**{null: None}, max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(**{null: None}, dp=None) == L.Result.BAD_ARG
    assert _comp(**{null: None}, ds=None) == L.Result.BAD_ARG
    assert _comp(**{null: None}, states=None) == L.Result.BAD_ARG
    assert _comp(**{null: None}, states=P(1)) == L.Result.BAD_ARG
    assert _comp(**{null: None}, max_chunk=MAX + 1, dp=None, ds=None, states=None) == L.Result.BAD_ARG
    assert _dec(**{null: None}, dp=None) == L.Result.BAD_ARG
    assert _dec(**{null: None}, ds=None) == L.Result.BAD_ARG
    assert _dec(**{null: None}, dp=None, ds=None) == L.Result.BAD_ARG
    assert _comp(**{null: None}, k=0, dp=None, ds=None, states=None) == L.Result.BAD_ARG
    assert _dec(**{null: None}, k=0, dp=None, ds=None) == L.Result.BAD_ARG


def test_null_capacities():
    assert _dec(caps=None) == L.Result.BAD_ARG           # decompress needs them
    assert _dec(caps=None, dp=None, ds=None) == L.Result.BAD_ARG
    if L.device_count() == 0:
        assert _comp(caps=None) == L.Result.ERROR        # compress: the bound of each size


# 2. maxChunkBytes above the maximum
def test_max_chunk_above_the_maximum_is_bad_arg():
    assert _comp(max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, n=0) == L.Result.BAD_ARG
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0,
                 max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=(1 << 32) - 1) == L.Result.BAD_ARG
    # ... before the dictionary arrays and the states
    assert _comp(max_chunk=MAX + 1, dp=None) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, ds=None) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, states=None) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, states=P(8)) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, dp=None, ds=None, states=None) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, k=0, dp=None, ds=None, states=None) == L.Result.BAD_ARG


# 3. a null d_dictPtrs or d_dictSizes with nDicts > 0
@pytest.mark.parametrize("k", [1, 3, (1 << 32) - 1])
@pytest.mark.parametrize("null", [{"dp": None}, {"ds": None}, {"dp": None, "ds": None}])
def test_null_dictionary_array_is_bad_arg(null, k):
    assert _prep(**null, k=k) == L.Result.BAD_ARG
    assert _comp(**null, k=k) == L.Result.BAD_ARG
    assert _dec(**null, k=k) == L.Result.BAD_ARG
    assert _comp(**null, k=k, n=0) == L.Result.BAD_ARG
    assert _dec(**null, k=k, n=0) == L.Result.BAD_ARG
    # ... before the states' check
    assert _prep(**null, k=k, states=None) == L.Result.BAD_ARG
    assert _prep(**null, k=k, states=P(1)) == L.Result.BAD_ARG
    assert _prep(**null, k=k, ssize=0) == L.Result.BAD_ARG
    assert _comp(**null, k=k, states=None) == L.Result.BAD_ARG
    assert _comp(**null, k=k, states=P(1)) == L.Result.BAD_ARG


# 4. the states (prepare, compress; nDicts > 0)
def test_bad_states_are_bad_arg():
    assert _prep(states=None) == L.Result.BAD_ARG
    assert _comp(states=None) == L.Result.BAD_ARG
    assert _comp(states=None, n=0) == L.Result.BAD_ARG
    for mis in (1, 16, 128, 256 + 64):
        assert _prep(states=P(mis)) == L.Result.BAD_ARG, mis
        assert _comp(states=P(mis)) == L.Result.BAD_ARG, mis
    assert _prep(k=3, ssize=3 * STATE - 1) == L.Result.BAD_ARG
    assert _prep(k=3, ssize=STATE) == L.Result.BAD_ARG
    assert _prep(k=3, ssize=0) == L.Result.BAD_ARG
    assert _prep(k=1, ssize=16384) == L.Result.BAD_ARG
    # the product does not wrap: 2^32 - 1 states are some 65 TiB
    assert _prep(k=(1 << 32) - 1, ssize=1 << 40) == L.Result.BAD_ARG
    assert _prep(k=1 << 18, ssize=(1 << 18) * STATE - 1) == L.Result.BAD_ARG


# 5. and 6.: ERROR without a device; what launches nothing is OK with one
def test_valid_arguments_without_gpu():
    expect = L.Result.ERROR if L.device_count() == 0 else L.Result.OK
    # nDicts == 0 with null dictionary arrays and null states, nChunks == 0 with null chunk arrays: valid.
    # With a device these launch nothing, so the placeholder pointers are never read.
    assert _prep(k=0, dp=None, ds=None, states=None, ssize=0) == expect
    assert _prep(k=0) == expect
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0) == expect
    assert _dec(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0) == expect
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0, k=0, dp=None, ds=None,
                 states=None) == expect
    assert _dec(src=None, sizes=None, dst=None, caps=None, out=None, which=None, n=0, k=0, dp=None,
                ds=None) == expect
    if L.device_count() > 0:
        return   # the calls below would launch kernels over the placeholder pointers
    assert _prep() == L.Result.ERROR
    assert _prep(k=1) == L.Result.ERROR
    assert _prep(ssize=1 << 40) == L.Result.ERROR
    assert _prep(k=1 << 18, ssize=(1 << 18) * STATE) == L.Result.ERROR
    assert _comp() == L.Result.ERROR
    assert _dec() == L.Result.ERROR
    assert _comp(k=0, dp=None, ds=None, states=None) == L.Result.ERROR     # every chunk NO_DICT
    assert _dec(k=0, dp=None, ds=None) == L.Result.ERROR
    assert _comp(k=0, states=P(1)) == L.Result.ERROR                       # no states are needed for no dictionaries
    assert _comp(max_chunk=MAX, n=1000) == L.Result.ERROR
    assert _comp(max_chunk=0) == L.Result.ERROR
