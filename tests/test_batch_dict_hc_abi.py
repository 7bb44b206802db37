"""Host-side contract of the batched LZ4-HC compress with a shared dictionary
(include/lz4mt_hip.h section 5c: lz4mtHipDictStateSizeHC,
lz4mtHipDictPrepareHC, lz4mtHipCompressBatchDictWorkspaceSize,
lz4mtHipCompressBatchDictHC), no GPU compute: the declarations, the Python
surface, the sizes, and the argument checks in the header's order (null
arrays, maxChunkBytes, the level, the dictionary, the state, the workspace;
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
STATE = L.lib.lz4mtHipDictStateSizeHC()
BIG = 1 << 40


def _prep(d=ANY, dsize=4096, state=ANY, ssize=None):
    return L.lib.lz4mtHipDictPrepareHC(d, dsize, state, STATE if ssize is None else ssize, None)


def _comp(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY, d=ANY, dsize=4096, state=ANY, level=9,
          ws=ANY, wsize=BIG):
    return L.lib.lz4mtHipCompressBatchDictHC(src, sizes, max_chunk, n, dst, caps, out, d, dsize, state, level, ws,
                                             wsize, None)


def _decl(text, name):
    m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", text)
    assert m, name
    return m.group(1), re.sub(r"\s+", " ", m.group(2))


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read(), flags=re.S)
    assert _decl(text, "lz4mtHipDictStateSizeHC") == ("uint64_t", "void")
    assert _decl(text, "lz4mtHipDictPrepareHC") == (
        "Lz4MtResult", "const void* d_dict, uint32_t dictSize, void* d_state, uint64_t stateSize, void* stream")
    assert _decl(text, "lz4mtHipCompressBatchDictWorkspaceSize") == (
        "uint64_t", "uint32_t maxChunkBytes, uint32_t nChunks, int level")
    assert _decl(text, "lz4mtHipCompressBatchDictHC") == (
        "Lz4MtResult", "const void* const* d_srcPtrs, const uint32_t* d_srcSizes, uint32_t maxChunkBytes, "
        "uint32_t nChunks, void* const* d_dstPtrs, const uint32_t* d_dstCaps, int32_t* d_outSizes, "
        "const void* d_dict, uint32_t dictSize, const void* d_stateHC, int level, void* d_workspace, "
        "uint64_t workspaceSize, void* stream")
    assert "5c." in open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read()


def test_abi_prototypes():
    from lz4mt_amd import _abi
    c = ctypes
    v, u32, u64, i = c.c_void_p, c.c_uint32, c.c_uint64, c.c_int
    assert _abi.PROTOTYPES["lz4mtHipDictStateSizeHC"] == (u64, [])
    assert _abi.PROTOTYPES["lz4mtHipDictPrepareHC"] == (i, [v, u32, v, u64, v])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictWorkspaceSize"] == (u64, [u32, u32, i])
    assert _abi.PROTOTYPES["lz4mtHipCompressBatchDictHC"] == (i, [v, v, u32, u32, v, v, v, v, u32, v, i, v, u64, v])
    assert L.lib.lz4mtHipDictStateSizeHC.restype is u64
    assert L.lib.lz4mtHipCompressBatchDictWorkspaceSize.restype is u64
    for name in ("lz4mtHipDictPrepareHC", "lz4mtHipCompressBatchDictHC"):
        assert getattr(L.lib, name).restype is i


def test_python_names_and_signatures():
    for name in ("prepare_dict_hc", "compress_batch_dict_hc", "batch_compress_dict_workspace"):
        assert name in L.__all__ and hasattr(L, name), name
    assert list(inspect.signature(L.prepare_dict_hc).parameters) == ["dictionary", "stream"]
    sig = inspect.signature(L.compress_batch_dict_hc)
    assert list(sig.parameters) == ["chunks", "prepared", "level", "caps", "stream", "workspace"]
    assert all(sig.parameters[k].default is None for k in ("caps", "stream", "workspace"))
    assert list(inspect.signature(L.batch_compress_dict_workspace).parameters) == ["max_chunk", "n", "level", "device"]
    # the two kinds of prepared dictionary can be told apart, and the existing form is the fast kind
    fast, hc = L.PreparedDict(None, None), L.PreparedDict(None, None, "hc")
    assert (fast.kind, fast.is_hc, hc.kind, hc.is_hc) == ("fast", False, "hc", True)
    # a prepared dictionary of the wrong kind is a TypeError before anything touches a device
    with pytest.raises(TypeError):
        L.compress_batch_dict_hc([], fast, 9)
    with pytest.raises(TypeError):
        L.compress_batch_dict([], hc)
    with pytest.raises(TypeError):
        L.compress_batch_dict_hc([], object(), 9)
    with pytest.raises(ValueError):
        L.compress_batch_dict_hc([], hc, 2)


def test_sizes():
    assert STATE % 256 == 0 and L.lib.lz4mtHipDictStateSizeHC() == STATE   # a constant
    assert STATE >= 32768 * 4 + 65536 * 2 + 2 * 63                         # heads, links, the scan's padding
    assert STATE > L.lib.lz4mtHipDictStateSize()                           # (not the fast codec's state)
    ws = L.lib.lz4mtHipCompressBatchDictWorkspaceSize
    for level in (0, 2):
        assert ws(4096, 100, level) == 0
    for level in (3, 9, 10, 12, 17):
        one = ws(4096, 1, level)
        assert one > 0 and one % 256 == 0 and one >= 2 * 4096
        assert ws(4096, 100, level) == 100 * one
        assert ws(4096, 1 << 20, level) == L.BATCH_HC_SLOTS * one      # no more slots than a call uses
        assert ws(65536, 1, level) > one
    assert ws(0, 1, 9) > 0   # one slot is never empty


# ---- BAD_ARG, in the header's order ----------------------------------------
@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out"])
def test_null_array_is_bad_arg(null):
    assert _comp(**{null: None}) == L.Result.BAD_ARG
    # ... before every later check
    assert _comp(**{null: None}, max_chunk=MAX + 1, level=0, d=None, state=None, ws=None) == L.Result.BAD_ARG


def test_max_chunk_above_the_maximum_is_bad_arg():
    assert _comp(max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, n=0) == L.Result.BAD_ARG
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, n=0, max_chunk=MAX + 1) == L.Result.BAD_ARG
    assert _comp(max_chunk=MAX + 1, level=0, d=None, state=None, ws=None) == L.Result.BAD_ARG


@pytest.mark.parametrize("level", [-1, 0, 1, 2])
def test_level_below_3_is_bad_arg(level):
    assert _comp(level=level) == L.Result.BAD_ARG
    assert _comp(level=level, n=0) == L.Result.BAD_ARG
    # ... before the dictionary's, the state's and the workspace's checks
    assert _comp(level=level, d=None, state=None, ws=None) == L.Result.BAD_ARG


@pytest.mark.parametrize("dsize", [1, 3, 4, 4096, 65536, (1 << 32) - 1])
def test_null_dictionary_of_non_zero_size_is_bad_arg(dsize):
    assert _prep(d=None, dsize=dsize) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize, n=0) == L.Result.BAD_ARG
    # ... before the state's and the workspace's checks
    assert _prep(d=None, dsize=dsize, state=None) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=dsize, state=P(1), ws=None) == L.Result.BAD_ARG


def test_bad_state_is_bad_arg():
    assert _prep(state=None) == L.Result.BAD_ARG
    assert _comp(state=None) == L.Result.BAD_ARG
    for mis in (1, 16, 128, 256 + 64):
        assert _prep(state=P(mis)) == L.Result.BAD_ARG, mis
        assert _comp(state=P(mis)) == L.Result.BAD_ARG, mis
    assert _prep(ssize=STATE - 1) == L.Result.BAD_ARG
    assert _prep(ssize=0) == L.Result.BAD_ARG
    assert _prep(ssize=L.lib.lz4mtHipDictStateSize()) == L.Result.BAD_ARG   # the fast codec's state size
    # also with no dictionary and with nothing to do, and before the workspace's check
    assert _prep(d=None, dsize=0, state=None) == L.Result.BAD_ARG
    assert _comp(n=0, state=None) == L.Result.BAD_ARG
    assert _comp(d=None, dsize=0, state=P(8), ws=None) == L.Result.BAD_ARG


@pytest.mark.parametrize("level", [3, 9, 10, 12])
def test_bad_workspace_is_bad_arg(level):
    one = L.lib.lz4mtHipCompressBatchDictWorkspaceSize(65536, 1, level)
    assert _comp(level=level, ws=None) == L.Result.BAD_ARG
    assert _comp(level=level, ws=P(128)) == L.Result.BAD_ARG
    assert _comp(level=level, wsize=one - 1) == L.Result.BAD_ARG
    assert _comp(level=level, wsize=0) == L.Result.BAD_ARG
    if L.device_count() == 0:
        assert _comp(level=level, wsize=one) == L.Result.ERROR          # one slot is enough for any nChunks
        assert _comp(level=level, wsize=one, n=1000) == L.Result.ERROR
        assert _comp(level=level, n=0, ws=None, wsize=0) == L.Result.ERROR   # nothing to do: no workspace needed


def test_valid_arguments_fail_without_gpu():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    for dsize in (0, 3, 4, 4096, 65536, 100000):
        assert _prep(dsize=dsize) == L.Result.ERROR
        assert _comp(dsize=dsize) == L.Result.ERROR
    assert _prep(d=None, dsize=0) == L.Result.ERROR          # no dictionary at all is valid
    assert _comp(d=None, dsize=0) == L.Result.ERROR
    assert _prep(ssize=1 << 40) == L.Result.ERROR
    assert _comp(caps=None) == L.Result.ERROR                # the bound of each size
    assert _comp(level=17) == L.Result.ERROR                 # above 12 counts as 12
    assert _comp(max_chunk=MAX, n=1000) == L.Result.ERROR
    assert _comp(src=None, sizes=None, dst=None, caps=None, out=None, n=0) == L.Result.ERROR
