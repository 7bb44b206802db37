"""Host-side contract of the batched block operators (include/lz4mt_hip.h
section 5), no GPU compute: argument checks come before the device check, in
the order lz4mtHipCompressFrame's use (BAD_ARG, then ERROR without a device).
"""
import ctypes

import pytest

import lz4mt_amd as L

P = ctypes.c_void_p
ANY = P(256)   # a non-null, 16-byte-aligned value: never dereferenced by the calls below
MAX = 4 << 20


def _compress(src=ANY, sizes=ANY, max_chunk=65536, n=1, dst=ANY, caps=ANY, out=ANY):
    return L.lib.lz4mtHipCompressBatch(src, sizes, max_chunk, n, dst, caps, out, None)


def _decompress(src=ANY, sizes=ANY, n=1, dst=ANY, caps=ANY, out=ANY):
    return L.lib.lz4mtHipDecompressBatch(src, sizes, n, dst, caps, out, None)


def test_constants_match_the_header():
    import os
    import re

    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "lz4mt_hip.h")).read()
    assert re.search(r"#define LZ4MT_HIP_BATCH_MAX_CHUNK \(4u << 20\)", text)
    assert re.search(r"#define LZ4MT_HIP_BATCH_BAD_CHUNK INT32_MIN", text)
    assert L.BATCH_MAX_CHUNK == MAX and L.BATCH_BAD_CHUNK == -(1 << 31)


@pytest.mark.parametrize("null", ["src", "sizes", "dst", "out"])
def test_compress_null_array_is_bad_arg(null):
    assert _compress(**{null: None}) == L.Result.BAD_ARG


@pytest.mark.parametrize("null", ["src", "sizes", "dst", "caps", "out"])
def test_decompress_null_array_is_bad_arg(null):
    assert _decompress(**{null: None}) == L.Result.BAD_ARG


def test_max_chunk_above_the_maximum_is_bad_arg():
    assert _compress(max_chunk=MAX + 1) == L.Result.BAD_ARG
    # ... also with nothing to do, and before the null check can hide it
    assert _compress(max_chunk=MAX + 1, n=0) == L.Result.BAD_ARG


def test_valid_arguments_fail_without_gpu():
    if L.device_count() > 0:
        pytest.skip("a HIP device is present")
    assert _compress() == L.Result.ERROR
    assert _compress(caps=None) == L.Result.ERROR       # null capacities are valid for compress
    assert _compress(max_chunk=MAX) == L.Result.ERROR
    assert _decompress() == L.Result.ERROR
    # no launch is not no device: nChunks == 0 still reports the missing device
    assert _compress(src=None, sizes=None, dst=None, caps=None, out=None, n=0) == L.Result.ERROR
    assert _decompress(src=None, sizes=None, dst=None, caps=None, out=None, n=0) == L.Result.ERROR


def test_python_names_are_exported():
    for name in ("compress_batch", "decompress_batch", "batch_compress_bound"):
        assert name in L.__all__ and callable(getattr(L, name)), name
    for n in (0, 1, 64, 65547, MAX):
        assert L.batch_compress_bound(n) == n + n // 255 + 16


def test_python_wrappers_check_their_arguments():
    with pytest.raises(TypeError):
        L.compress_batch([b"host bytes"])
    with pytest.raises(TypeError):
        L.decompress_batch([b"host bytes"], [16])
