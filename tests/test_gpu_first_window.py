"""The frame encoder's first-window fast phase (first windows
only) on the GPU.

The fast body of encode_block_v5 runs the first window after a match only,
with the window state folded into constants (lane positions sBase + c(L),
both role lanes on, every lane live, step 1); a window without a stop writes
the continuation state as constants and leaves the phase, the general body
resumes the search and the phase is entered again after its match.  Every
comparison here is the encoder's block against the oracle's (LZ4 1.9.3
restated) through lz4mtHipCompressBlock, which runs the frame encoder's own
instantiation (k_encode; sizes above 262 144 B, so not k_encode_p17), with the
exchange probe and again with the read-back probe.

The inputs are those of tests/test_enc_model_first_window.py, where the lane
model shows what they reach: a stop on every lane of the first window and of
the first continuation window, and exits whose table writes are redone after
a tag alias.  Sizes: 300 000 B blocks and one of (1 << 20) + 13 B (the
SIMD-mate priority tick is on from 1 MiB)."""
import functools
import os
import random
import sys

import pytest
import torch

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import enc_model  # noqa: E402

pytestmark = pytest.mark.gpu

L = None
N = 300_000
SWEEP_SEED = 24   # the seed whose coverage tests/test_enc_model_first_window.py asserts


@pytest.fixture(scope="module", autouse=True)
def lib():
    global L
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    L = lz4mt_amd
    return L


@pytest.fixture(params=["exchange", "readback"])
def probe(request, monkeypatch):
    if request.param == "readback":
        monkeypatch.setenv("LZ4MT_AMD_ENC_PROBE", "readback")
        assert L.lib.lz4mtHipEncoderProbe() == 0
        yield request.param
        monkeypatch.delenv("LZ4MT_AMD_ENC_PROBE")
    else:
        yield request.param
    assert L.lib.lz4mtHipEncoderProbe() == 1


@functools.lru_cache(maxsize=None)
def _buf(name):
    if name == "sweep":
        return enc_model.literal_run_sweep(N, SWEEP_SEED)
    if name == "sweep1m":
        return enc_model.literal_run_sweep((1 << 20) + 13, SWEEP_SEED + 1)
    if name == "abc":
        return bytes(map(random.Random(4).randrange, [3] * N))
    if name == "search2k":
        return enc_model.long_search_input(N, 2 << 10, 5)
    if name == "search70k":
        return enc_model.long_search_input(N, 70 << 10, 5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, n, cap):
    return oracle.compress_block(_buf(name)[:n], cap)


def _check(name, n, cap):
    got = L.compress_block(_buf(name)[:n], cap)
    assert got == _want(name, n, cap), (name, n, cap, len(got), len(_want(name, n, cap)))


# ---- the three families: a stop on every lane of the first two windows of a
# search; tag aliases and same-bucket collisions in nearly every window;
# searches that leave the phase for many windows and come back
@pytest.mark.parametrize("name", ["sweep", "abc", "search2k", "search70k"])
def test_families(probe, name):
    for cap in (N, oracle.lib.orc_lz4_compress_bound(N)):
        _check(name, N, cap)


# ---- the block's end, and so the phase's last exit, on every position of a
# search that spans two windows: every n of a 130-byte range, cap = n
def test_sweep_truncated_at_every_length(probe):
    for n in range(N - 129, N + 1):
        _check("sweep", n, n)


def test_priority_tick_block(probe):
    """(1 << 20) + 13 B: the SIMD-mate priority tick rides on the ring's
    advance inside the folded window too."""
    n = (1 << 20) + 13
    for cap in (n, oracle.lib.orc_lz4_compress_bound(n)):
        _check("sweep1m", n, cap)
