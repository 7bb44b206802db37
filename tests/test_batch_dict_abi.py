"""Host-side contract of the batched operators with a shared dictionary
(include/lz4mt_hip.h section 5b: lz4mtHipDictStateSize, lz4mtHipDictPrepare,
lz4mtHipCompressBatchDict, lz4mtHipDecompressBatchDict), no GPU compute: the
declarations, the Python surface, the state size, and the argument checks in
the header's order (null arrays, maxChunkBytes, the dictionary, the state;
BAD_ARG, then ERROR without a device).
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


def _prep(d=ANY, dsize=4096, state=ANY, ssize=None):
    return L.lib.lz4mtHipDictPrepare(d, dsize, state, STATE if ssize is None else ssize, None)


def _comp(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY, d=ANY, dsize=4096, state=ANY):
    return L.lib.lz4mtHipCompressBatchDict(src, sizes, max_chunk, n, dst, caps, out, d, dsize, state, None)


def _dec(src=ANY, sizes=ANY, n=1, dst=ANY, caps=ANY, out=ANY, d=ANY, dsize=4096):
    return L.lib.lz4mtHipDecompressBatchDict(src, sizes, n, dst, caps, out, d, dsize, None)


def _decl(text, name):
    m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", text)
    assert m, name
    return m.group(1), re.sub(r"\s+", " ", m.group(2))


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read(), flags=re.S)
    assert _decl(text, "lz4mtHipDictStateSize") == ("uint64_t", "void")
    assert _decl(text, "lz4mtHipDictPrepare") == (
        "Lz4MtResult", "const void* d_dict, uint32_t dictSize, void* d_state, uint64_t stateSize, void* stream")
    assert _decl(text, "lz4mtHipCompressBatchDict") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes, "
        "uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, "
        "const void* d_dict, uint32_t dictSize, const void* d_state, void* stream")
    assert _decl(text, "lz4mtHipDecompressBatchDict") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t nChunks, "
        "void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, const void* d_dict, "
        "uint32_t dictSize, void* stream")
    k = re.search(r"#define LZ4MT_HIP_DICT_WINDOW \((\d+)u << (\d+)\)", text)
    assert k and int(k.group(1)) << int(k.group(2)) == L.DICT_WINDOW == 65536


def test_abi_prototypes():
    from lz4mt_amd import _abi
    c = ctypes
    v, u32, u64 = c.c_void_p, c.c_uint32, c.c_uint64
    assert _abi.DICT_WINDOW == 65536
    assert _abi.PROTOTYPES["lz4mtHipDictStateSize"] == (u64, [])
    assert _abi.PROTOTYPES["lz4mtHipDictPrepare"] == (c.c_int, [v, u32, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDict"] == (c.c_int, [v, v, u32, u32, v, v, v, v, u32, v, v])
    assert _abi.PROTOTYPES["lz4mtHipDecompressBatchDict"] == (c.c_int, [v, v, u32, v, v, v, v, u32, v])
    assert L.lib.lz4mtHipDictStateSize.restype is u64
    for name in ("lz4mtHipDictPrepare", "lz4mtHipCompressBatchDict", "lz4mtHipDecompressBatchDict"):
        assert getattr(L.lib, name).restype is c.c_int


def test_python_names_and_signatures():
    for name in ("DICT_WINDOW", "PreparedDict", "prepare_dict", "compress_batch_dict", "decompress_batch_dict"):
        assert name in L.__all__ and hasattr(L, name), name
    assert list(inspect.signature(L.prepare_dict).parameters) == ["dictionary", "stream"]
    sig = inspect.signature(L.compress_batch_dict)
    assert list(sig.parameters) == ["chunks", "prepared", "caps", "stream"]
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    sig = inspect.signature(L.decompress_batch_dict)
    assert list(sig.parameters) == ["blocks", "caps", "dictionary", "stream"]
    assert sig.parameters["stream"].default is None
    assert inspect.signature(L.prepare_dict).parameters["stream"].default is None


def test_compress_batch_signature_is_unchanged():
    sig = inspect.signature(L.compress_batch)
    assert list(sig.parameters) == ["chunks", "caps", "stream", "level", "workspace"]
    assert sig.parameters["level"].default == 0 and sig.parameters["workspace"].default is None
    assert list(inspect.signature(L.decompress_batch).parameters) == ["blocks", "caps", "stream"]


def test_state_size():
    assert STATE % 256 == 0 and STATE >= 16384
    assert STATE < 16384 + 4096          # the table plus a small header
    assert L.lib.lz4mtHipDictStateSize() == STATE   # a constant


# ---- BAD_ARG, in the header's order ----------------------------------------
@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out"])
def test_null_array_is_bad_arg(null):
    assert _comp(**{null: None}) == L.Result.BAD_ARG
    assert _dec(**{null: None}) == L.Result.BAD_ARG
    # ... before every later check
    assert _comp(**{null: None}, max_chunk=MAX + 1, d=None, state=None) == L.Result.BAD_ARG
    assert _dec(**{null: None}, d=None) == L.Result.BAD_ARG


def test_null_capacities():
    assert _dec(caps=None) == L.Result.BAD_ARG           # decompress needs them
    if L.device_count() == 0:
        assert _comp(caps=None) == L.Result.ERROR        # compress: the bound of each size


def test_max_chunk_above_the_maximum_is_bad_arg():
    assert _comp(max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, n=0) == L.Result.BAD_ARG
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, n=0, max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, d=None, state=None) == L.Result.BAD_ARG


@pytest.mark.parametrize("dsize", [1, 7, 8, 4096, 65536, (1 << 32) - 1])
def test_null_dictionary_of_non_zero_size_is_bad_arg(dsize):
    assert _prep(d=None, dsize=dsize) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize) == L.Result.BAD_ARG
    assert _dec(d=None, dsize=dsize) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize, n=0) == L.Result.BAD_ARG
    assert _dec(d=None, dsize=dsize, n=0) == L.Result.BAD_ARG
    # ... before the state's check
    assert _prep(d=None, dsize=dsize, state=None) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize, state=P(1)) == L.Result.BAD_ARG


def test_bad_state_is_bad_arg():
    assert _prep(state=None) == L.Result.BAD_ARG
    assert _comp(state=None) == L.Result.BAD_ARG
    for mis in (1, 16, 128, 256 + 64):
        assert _prep(state=P(mis)) == L.Result.BAD_ARG, mis
        assert _comp(state=P(mis)) == L.Result.BAD_ARG, mis
    assert _prep(ssize=STATE - 1) == L.Result.BAD_ARG
    assert _prep(ssize=0) == L.Result.BAD_ARG
    assert _prep(ssize=16384) == L.Result.BAD_ARG
    # also with no dictionary and with nothing to do
    assert _prep(d=None, dsize=0, state=None) == L.Result.BAD_ARG
    assert _comp(n=0, state=None) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=0, state=P(8)) == L.Result.BAD_ARG


def test_valid_arguments_fail_without_gpu():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    for dsize in (0, 7, 8, 4096, 65536, 100000):
        assert _prep(dsize=dsize) == L.Result.ERROR
        assert _comp(dsize=dsize) == L.Result.ERROR
        assert _dec(dsize=dsize) == L.Result.ERROR
    assert _prep(d=None, dsize=0) == L.Result.ERROR          # no dictionary at all is valid
    assert _comp(d=None, dsize=0) == L.Result.ERROR
    assert _dec(d=None, dsize=0) == L.Result.ERROR
    assert _prep(ssize=1 << 40) == L.Result.ERROR
    assert _comp(max_chunk=MAX, n=1000) == L.Result.ERROR
    assert _comp(max_chunk=0) == L.Result.ERROR
    # nChunks == 0 with null arrays: valid, the missing device is still reported
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, n=0) == L.Result.ERROR
    assert _dec(src=None, sizes=None, dst=None, caps=None, out=None, n=0) == L.Result.ERROR
    assert _dec(src=None, sizes=None, dst=None, caps=None, out=None, n=0, d=None, dsize=0) == L.Result.ERROR
