"""The frame encoder's two-phase window loop: general -> fast ->
general.

Inside the fast phase encode_block_v5 drops the block-end predicates, the
round trip's end clamps, the per-sequence limitedOutput margin test and the
wide-window test; it may enter only once (a) the window is far enough from
the block's end and (b) the remaining input provably fits the output, and
must leave before either stops holding or the search step grows to a wide
window.  Every comparison here is the encoder's block against the oracle's
(LZ4 1.9.3 restated) through lz4mtHipCompressBlock, which runs the frame
encoder's own instantiation (k_encode; sizes above 262 144 B, so not
k_encode_p17), with the exchange probe and again with the read-back probe.

Sizes: 300 000 B blocks (about 5 ms each), one of (1 << 20) + 13 B (the
SIMD-mate priority tick is on from 1 MiB), two 16 MiB frames."""
import functools
import random

import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

L = None
N = 300_000


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


def _mixed(n, seed):
    # synthetic text, random runs (long literal runs > 64), zero runs and
    # repeats (matches longer than one 256-byte count round), near/far offsets
    rnd = random.Random(seed)
    syn = oracle.gen_synthetic(1 << 20, seed)
    out, size = [], 0
    while size < n:
        k = rnd.randrange(5)
        if k == 0:
            a = rnd.randrange(len(syn) - 5000)
            piece = syn[a:a + rnd.randrange(100, 5000)]
        elif k == 1:
            piece = oracle.gen_random(rnd.randrange(65, 700), rnd.randrange(1 << 30))
        elif k == 2:
            piece = bytes(rnd.randrange(1, 3000))
        elif k == 3 and out:
            prev = b"".join(out[-8:])
            a = rnd.randrange(len(prev))
            piece = prev[a:a + rnd.randrange(4, 2000)]
        else:
            piece = bytes([rnd.randrange(256)]) * rnd.randrange(1, 400)
        out.append(piece)
        size += len(piece)
    return b"".join(out)[:n]


def _search(prefix, run, total=N, seed=5):
    """compressible prefix, `run` random bytes (the search step grows past
    the wide bound inside it from about 70 KB on), compressible suffix"""
    syn = oracle.gen_synthetic(total, seed)
    return (syn[:prefix] + oracle.gen_random(run, seed + 1) + syn[prefix:])[:total]


@functools.lru_cache(maxsize=None)
def _buf(name):
    if name == "mixed":
        return _mixed(N, 21)
    if name == "mixed1m":
        return _mixed((1 << 20) + 13, 22)
    if name == "tail_match":   # the last 4 KB repeat bytes from 50 KB back: one match into matchlimit
        m = _mixed(N, 23)
        return m[:N - 4096] + m[N - 4096 - 50_000:N - 50_000]
    if name == "tail_zeros":   # a zero run reaches the end
        return _mixed(N - 3000, 24) + bytes(3000)
    if name == "search2k":
        return _search(40_000, 2 << 10)
    if name == "search70k":
        return _search(40_000, 70 << 10)
    if name == "search200k":
        return _search(40_000, 200 << 10)
    if name == "search_to_end":   # the random run reaches the block's end
        return _search(100_000, 200_000)
    if name == "shrink_then_grow":   # (b) holds early, then 100 KB of literals
        return (bytes(100_000) + b"abcdefg" * 14_286)[:200_000] + oracle.gen_random(100_000, 3)
    if name == "grow_then_shrink":   # (b) cannot hold before the last sequences
        return oracle.gen_random(100_000, 4) + (b"abcdefg" * 14_286 + bytes(100_000))[:200_000]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name, n, cap):
    return oracle.compress_block(_buf(name)[:n], cap)


def _check(name, n, cap):
    got = L.compress_block(_buf(name)[:n], cap)
    assert got == _want(name, n, cap), (name, n, cap, len(got), len(_want(name, n, cap)))


# ---- leaving the fast phase at the block's end: every n of a contiguous
# range of 603 (more than the ring's 512-byte advance), cap = n, so the exit
# threshold falls on every alignment relative to matches, literal runs and
# the ring's advance.  Three chunks per probe keep each case to a few seconds.
@pytest.mark.parametrize("lo", [N - 602, N - 401, N - 200])
def test_block_end_every_alignment(probe, lo):
    for n in range(lo, lo + 201):
        _check("mixed", n, n)


# the tail variants: the truncation point moves through the final match / the
# zero run, 160 lengths each (the match and the run are longer than that)
@pytest.mark.parametrize("name", ["tail_match", "tail_zeros"])
def test_block_end_long_tail(probe, name):
    for n in range(N - 159, N + 1):
        _check(name, n, n)


# ---- long searches: out of the fast phase when the step nears the wide
# bound, back in after the next match
@pytest.mark.parametrize("name", ["search2k", "search70k", "search200k", "search_to_end"])
def test_long_search_leaves_and_reenters(probe, name):
    n = len(_buf(name))
    bound = oracle.lib.orc_lz4_compress_bound(n)
    for cap in (n, bound):
        _check(name, n, cap)


# ---- margin proof: around the compressed size every cap either fits
# exactly or fails, whatever phase the encoder is in when it finds out
@pytest.mark.parametrize("name", ["mixed", "tail_match", "tail_zeros", "search2k", "search70k", "search200k",
                                  "search_to_end", "shrink_then_grow", "grow_then_shrink"])
def test_margin_at_every_cap_near_the_size(probe, name):
    n = len(_buf(name))
    c = len(_want(name, n, oracle.lib.orc_lz4_compress_bound(n)))
    assert c > 0
    for cap in list(range(c - 3, c + 81)) + [n, n - 1, n // 2]:
        _check(name, n, cap)
    assert _want(name, n, c - 1) == b"" and len(_want(name, n, c + 80)) in (0, c)


def test_priority_tick_block(probe):
    """(1 << 20) + 13 B: the SIMD-mate priority tick shares the ring-advance
    branch with nothing else in the fast phase."""
    n = (1 << 20) + 13
    c = len(_want("mixed1m", n, oracle.lib.orc_lz4_compress_bound(n)))
    for cap in (n, n - 1, c, c - 1, c + 40, oracle.lib.orc_lz4_compress_bound(n)):
        _check("mixed1m", n, cap)
    for m in (n - 1279, n - 1281, n - 700):
        _check("mixed1m", m, m)


@pytest.mark.parametrize("bid", [6, 7])
def test_whole_frames(probe, bid):
    """16 MiB of App. F: the frame path's own launch, bytes as the oracle's."""
    n = 16 << 20
    src = L.gen_synthetic(n, seed=42, device="cuda:0")
    sd = L.make_sd(bid, stream_checksum=True, block_checksum=True)
    got = bytes(L.compress_frame(src, sd).cpu().numpy().tobytes())
    assert got == _frame_want(bid)


@functools.lru_cache(maxsize=None)
def _frame_want(bid):
    return oracle.compress_frame(oracle.gen_synthetic(16 << 20, 42), oracle.params(bid, True, True))
