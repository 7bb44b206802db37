"""Host-side contract of the batched LZ4-HC (include/lz4mt_hip.h section 5:
lz4mtHipCompressBatchWorkspaceSize / lz4mtHipCompressBatchEx), no GPU
compute: the workspace's slot arithmetic, and the argument checks, which come
before the device check in section 5's order (null arrays, maxChunkBytes,
then the workspace at level >= 3; BAD_ARG, then ERROR without a device).
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
HC_LEVELS = (3, 9, 10, 12)
MAXES = (0, 1, 4096, 65536, MAX)


def ws_size(max_chunk, n, level):
    return L.lib.lz4mtHipCompressBatchWorkspaceSize(max_chunk, n, level)


def _ex(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY, level=9, ws=ANY, ws_size_=None):
    if ws_size_ is None:
        ws_size_ = ws_size(min(max_chunk, MAX), 1, level)
    return L.lib.lz4mtHipCompressBatchEx(src, sizes, max_chunk, n, dst, caps, out, level, ws, ws_size_, None)


def test_header_declares_both_functions():
    text = open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read()
    assert re.search(r"uint64_t\s+lz4mtHipCompressBatchWorkspaceSize\(uint32_t maxChunkBytes, uint32_t nChunks, "
                     r"int level\);", text)
    m = re.search(r"Lz4MtResult\s+lz4mtHipCompressBatchEx\(([^;]*)\);", text)
    assert m
    args = re.sub(r"\s+", " ", m.group(1))
    assert args == ("const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes, "
                    "uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, "
                    "int level, void* d_workspace, uint64_t workspaceSize, void* stream")
    k = re.search(r"#define LZ4MT_HIP_BATCH_HC_SLOTS (\d+)u", text)
    assert k and int(k.group(1)) == L.BATCH_HC_SLOTS


def test_abi_prototypes():
    from lz4mt_amd import _abi
    c = ctypes
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchWorkspaceSize"] == (c.c_uint64, [c.c_uint32, c.c_uint32, c.c_int])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchEx"] == (
        c.c_int, [c.c_void_p, c.c_void_p, c.c_uint32, c.c_uint32, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int,
                  c.c_void_p, c.c_uint64, c.c_void_p])
    assert L.lib.lz4mtHipCompressBatchWorkspaceSize.restype is c.c_uint64
    assert L.lib.lz4mtHipCompressBatchEx.restype is c.c_int


def test_python_names_are_exported():
    assert "batch_compress_workspace" in L.__all__ and callable(L.batch_compress_workspace)
    assert "compress_batch" in L.__all__
    sig = inspect.signature(L.compress_batch)
    assert list(sig.parameters) == ["chunks", "caps", "stream", "level", "workspace"]
    assert sig.parameters["level"].default == 0 and sig.parameters["workspace"].default is None
    assert sig.parameters["caps"].default is None and sig.parameters["stream"].default is None
    assert list(inspect.signature(L.batch_compress_workspace).parameters) == ["max_chunk", "n", "level", "device"]


@pytest.mark.parametrize("level", [-1, 0, 1, 2])
def test_workspace_is_zero_below_level_3(level):
    for mx in MAXES:
        for n in (0, 1, 100, 1 << 31):
            assert ws_size(mx, n, level) == 0


@pytest.mark.parametrize("level", HC_LEVELS)
def test_workspace_slot_arithmetic(level):
    R = L.BATCH_HC_SLOTS
    for mx in MAXES:
        slot = ws_size(mx, 1, level)
        assert slot > 0 and slot % 256 == 0, (mx, level)
        assert slot >= 2 * mx, (mx, level)                 # a u16 per source byte
        assert ws_size(mx, 0, level) == 0
        for k in (2, 3, 7, 20, 100):
            assert ws_size(mx, k, level) == k * slot, (mx, level, k)
        # non-decreasing in n, and capped at R slots
        seq = [ws_size(mx, n, level) for n in (0, 1, 2, 1000, R - 1, R, R + 1, 10 * R, (1 << 32) - 1)]
        assert seq == sorted(seq), (mx, level)
        assert seq[-4] == seq[-3] == seq[-2] == seq[-1] == R * slot
        assert seq[-5] == (R - 1) * slot
    # non-decreasing in the chunk size as well
    slots = [ws_size(mx, 1, level) for mx in MAXES]
    assert slots == sorted(slots)


def test_level_10_slot_is_larger_than_level_9_slot():
    for mx in MAXES:
        assert ws_size(mx, 1, 10) > ws_size(mx, 1, 9)
        assert ws_size(mx, 1, 9) == ws_size(mx, 1, 3)
        assert ws_size(mx, 1, 10) == ws_size(mx, 1, 12) == ws_size(mx, 1, 17)


@pytest.mark.parametrize("level", [0, 2, 3, 9, 10, 12, 17])
@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out"])
def test_null_array_is_bad_arg(null, level):
    assert _ex(level=level, **{null: None}) == L.Result.BAD_ARG


@pytest.mark.parametrize("level", [0, 2, 3, 9, 10, 12])
def test_max_chunk_above_the_maximum_is_bad_arg(level):
    assert _ex(max_chunk=MAX + 1, level=level) == L.Result.BAD_ARG
    # ... also with nothing to do, and with no workspace
    assert _ex(max_chunk=MAX + 1, n=0, level=level) == L.Result.BAD_ARG
    assert _ex(max_chunk=MAX + 1, n=0, level=level, ws=None, ws_size_=0) == L.Result.BAD_ARG
    assert _ex(src=None, sizes=None, dst=None, caps=None, out=None, max_chunk=MAX + 1, n=0, level=level,
               ws=None, ws_size_=0) == L.Result.BAD_ARG


@pytest.mark.parametrize("level", HC_LEVELS)
def test_bad_workspace_is_bad_arg(level):
    for mx in (0, 4096, 65536, MAX):
        slot = ws_size(mx, 1, level)
        assert _ex(max_chunk=mx, level=level, ws=None, ws_size_=slot) == L.Result.BAD_ARG          # null
        assert _ex(max_chunk=mx, level=level, ws=None, ws_size_=0) == L.Result.BAD_ARG
        for mis in (1, 16, 128, 256 + 64):                                                         # misaligned
            assert _ex(max_chunk=mx, level=level, ws=P(mis), ws_size_=slot) == L.Result.BAD_ARG, mis
        assert _ex(max_chunk=mx, level=level, ws_size_=slot - 1) == L.Result.BAD_ARG               # below one slot
        assert _ex(max_chunk=mx, level=level, ws_size_=0) == L.Result.BAD_ARG
        # many chunks, still less than one slot
        assert _ex(max_chunk=mx, n=1000, level=level, ws_size_=slot - 1) == L.Result.BAD_ARG
    # a level 9 slot is too small for level 10
    assert _ex(level=10, ws_size_=ws_size(65536, 1, 9)) == L.Result.BAD_ARG


def test_valid_arguments_fail_without_gpu():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    for level in HC_LEVELS + (17,):
        assert _ex(level=level) == L.Result.ERROR
        assert _ex(level=level, caps=None) == L.Result.ERROR           # null capacities are valid
        assert _ex(level=level, max_chunk=MAX) == L.Result.ERROR
        assert _ex(level=level, max_chunk=0) == L.Result.ERROR
        assert _ex(level=level, n=1000) == L.Result.ERROR              # one slot serves any number of chunks
        assert _ex(level=level, ws_size_=1 << 40) == L.Result.ERROR
        # nChunks == 0: null arrays and no workspace are fine, the missing device is still reported
        assert _ex(src=None, sizes=None, dst=None, caps=None, out=None, n=0, level=level, ws=None,
                   ws_size_=0) == L.Result.ERROR
        assert _ex(n=0, level=level, ws=P(1), ws_size_=0) == L.Result.ERROR
    for level in (0, 2):   # below 3 the workspace is ignored: null, misaligned, any size
        assert _ex(level=level, ws=None, ws_size_=0) == L.Result.ERROR
        assert _ex(level=level, ws=P(1), ws_size_=5) == L.Result.ERROR
        assert _ex(src=None, sizes=None, dst=None, caps=None, out=None, n=0, level=level, ws=None,
                   ws_size_=0) == L.Result.ERROR
