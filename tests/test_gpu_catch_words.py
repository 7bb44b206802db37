"""The fast body's catch-up from words, its phase entry at 65536 + 64 and its
leaner pending store (catch-up from words, one-sided ring test) on the
GPU.  Every comparison is the encoder's block against the oracle's (LZ4 1.9.3
restated) through lz4mtHipCompressBlock, which runs the frame encoder's own
instantiation (k_encode; 300 000 B blocks, about 5 ms each), with the
exchange probe and again with the read-back probe; one test goes through
lz4mtHipCompressBatch (k_encode_batch, the same instantiation).

Inputs: the unit blocks of tests/test_enc_model_catch_words.py (every
catch-up length 0 .. 61 that eats the literal run whole, 0 .. 60 that ends
on a differing byte, TEST-lane stops, sequences of 63, 64, 65 and 129 bytes,
literals that have left the ring; the coverage is asserted there); a match
ending at every offset within 70 bytes of the phase's entry bound; blocks
whose first 64 bytes recur just below and just above that bound, so that a
candidate in the block's first 64 bytes is reached from the general phase
and refused, out of range, from the fast one."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import enc_model  # noqa: E402

pytestmark = pytest.mark.gpu

L = None
N = 300_000
SEEDS = (1, 2, 3, 4, 5, 6)
BEG = enc_model.FAST_BEG   # 65536 + 64


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
def _units(seed):
    data = enc_model.catch_up_units(N, seed, enc_model.catch_up_cases())
    return data, oracle.compress_block(data, oracle.lib.orc_lz4_compress_bound(N)), oracle.compress_block(data, N)


@functools.lru_cache(maxsize=None)
def _entry_block(end):
    """App. F text with a zero run (one long match) that ends at `end`: the
    first match that may enter the fast phase ends on every alignment"""
    syn = bytearray(oracle.gen_synthetic(N, 11))
    syn[end - 400:end] = bytes(400)
    assert syn[end] != 0
    data = bytes(syn)
    return data, oracle.compress_block(data, N)


@functools.lru_cache(maxsize=None)
def _head_block(below, above, seed=7):
    """64 fresh bytes at the block's start, zero runs, a copy of them at
    `below` (candidates in the first 64 bytes, in range while ip <= cd +
    65535 < 65536 + 64: the general phase) and one at `above` (the first
    copy is out of range, the second one is not)"""
    head = bytes(1 + (b % 255) for b in oracle.gen_random(64, seed))
    buf = bytearray(N)
    buf[:64] = head
    buf[below:below + 64] = head
    buf[above:above + 64] = head
    tail = oracle.gen_synthetic(100_000, seed)
    buf[N - 100_000:] = tail
    data = bytes(buf)
    return data, oracle.compress_block(data, N)


HEADS = [(65_470, 65_600), (65_530, 65_601), (65_536, 65_610), (65_471, 65_663), (65_535, 65_599), (65_500, 65_564)]


@pytest.mark.parametrize("seed", SEEDS)
def test_unit_blocks(probe, seed):
    data, want_bound, want_n = _units(seed)
    assert L.compress_block(data, oracle.lib.orc_lz4_compress_bound(N)) == want_bound
    assert L.compress_block(data, N) == want_n


def test_phase_entry_on_every_alignment(probe):
    for end in range(BEG - 70, BEG + 71):
        data, want = _entry_block(end)
        got = L.compress_block(data, N)
        assert got == want, (end, len(got), len(want))


@pytest.mark.parametrize("below,above", HEADS)
def test_candidates_in_the_blocks_first_64_bytes(probe, below, above):
    data, want = _head_block(below, above)
    assert L.compress_block(data, N) == want


def _at_allocation_start(data):
    """a device tensor holding `data` whose first byte is the first byte of a
    device allocation (a segment of the caching allocator)"""
    torch.cuda.empty_cache()
    keep = []
    for _ in range(64):
        t = torch.empty(len(data), dtype=torch.uint8, device="cuda")
        if t.data_ptr() in {seg["address"] for seg in torch.cuda.memory_snapshot()}:
            t.copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
            return t, keep
        keep.append(t)
    pytest.fail("no tensor at the start of a device allocation")


def test_batch_chunk_at_its_allocations_first_byte():
    """k_encode_batch: the chunk's bytes below its first one are not the
    caller's; a backward word of the catch-up must never reach them"""
    chunks, wants, keep = [], [], []
    for below, above in HEADS[:3]:
        data, want = _head_block(below, above)
        t, k = _at_allocation_start(data)
        chunks.append(t)
        keep.append(k)
        wants.append(want)
    for seed in SEEDS[:2]:
        data, _, want = _units(seed)
        t, k = _at_allocation_start(data)
        chunks.append(t)
        keep.append(k)
        wants.append(want)
    outs, sizes = L.compress_batch(chunks, caps=[N] * len(chunks))
    torch.cuda.synchronize()
    sizes = sizes.cpu().tolist()
    for i, want in enumerate(wants):
        assert sizes[i] == len(want), (i, sizes[i], len(want))
        assert bytes(outs[i][:sizes[i]].cpu().numpy().tobytes()) == want, i
