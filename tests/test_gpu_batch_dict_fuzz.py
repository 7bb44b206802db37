"""Differential fuzz of the dictionary batch encoder (lz4mtHipDictPrepare +
lz4mtHipCompressBatchDict; k_dict_prepare, k_encode_batch_dict) against the
oracle's LZ4_loadDict + LZ4_compress_fast_continue restatement
(oracle.compress_block_dict, pinned against the liblz4 fixture and liblz4
itself by tests/test_oracle_dict.py): same return value, same bytes, and every
accepted block goes back through lz4mtHipDecompressBatchDict to its source.

Dictionaries and chunks are synth_cases.py's: dictionary contents that differ
per size, chunks built from slices of the dictionary and of the chunk so far
(over the dictionary's end, on its first byte and last inserted position, more
than 65 535 back, periods 1..40) between random bytes, zero runs and text.
Packing, canaries and the odd-address dictionary are test_gpu_batch_dict.py's.
"""
import random

import pytest
import torch

import oracle
import synth_cases as K
import test_gpu_batch as B
import test_gpu_batch_dict as BD
from test_gpu_batch import BAD, pack
from test_gpu_batch_dict import dict_tensor, prepare

pytestmark = pytest.mark.gpu

MAX_CHUNK = 4 << 20    # LZ4MT_HIP_BATCH_MAX_CHUNK


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    assert lz4mt_amd.device_count() > 0
    assert lz4mt_amd.BATCH_MAX_CHUNK == MAX_CHUNK
    B.L = BD.L = lz4mt_amd      # the helpers of both modules call the library through their module's handle
    return lz4mt_amd


def round_trip(blocks, sources, dt, tag):
    """Every block back through lz4mtHipDecompressBatchDict at its source's exact size."""
    flat, offs = pack(blocks)
    sizes = [len(s) for s in sources]
    back, dst = BD.decompress_call(flat, offs, [len(b) for b in blocks], sizes, dt)
    assert back == sizes, tag
    for i, s in enumerate(sources):
        assert dst.data(i, len(s)) == s, (tag, i, len(s))
    assert dst.canaries_ok(), tag


@pytest.mark.parametrize("size", K.FUZZ_DICTS)
def test_compress_fuzz_vs_oracle(size):
    d = K.fuzz_dict(size)
    chunks = K.fuzz_chunks(size)
    rnd = random.Random(size + 5)
    flat, offs = pack(chunks)
    picks, caps = [], []
    for i, c in enumerate(chunks):
        for cap in K.caps_of(rnd, len(c)):
            picks.append(i)
            caps.append(cap)
    assert len(caps) == len(chunks) * len(K.CAP_KINDS)
    want = [oracle.compress_block_dict(d, chunks[i], cap) for i, cap in zip(picks, caps)]
    dt = dict_tensor(d)
    state = prepare(dt)
    soffs, sizes = [offs[i] for i in picks], [len(chunks[i]) for i in picks]
    got, dst = BD.compress_call(flat, soffs, sizes, caps, max(sizes), dt, state)
    for k, (i, cap, w) in enumerate(zip(picks, caps, want)):
        assert got[k] == len(w), (size, len(chunks[i]), cap, got[k], len(w))
        assert dst.data(k, len(w)) == w, (size, len(chunks[i]), cap)
    assert dst.canaries_ok()
    assert any(not w for w in want) and sum(1 for w in want if w) > len(chunks)
    # null capacities are the bound
    bounds = [K.bound(len(c)) for c in chunks]
    ngot, ndst = BD.compress_call(flat, offs, [len(c) for c in chunks], bounds, MAX_CHUNK, dt, state, null_caps=True)
    for i, c in enumerate(chunks):
        w = want[i * len(K.CAP_KINDS)]
        assert caps[i * len(K.CAP_KINDS)] == bounds[i]
        assert ngot[i] == len(w) and ndst.data(i, len(w)) == w, (size, "null caps", len(c))
    assert ndst.canaries_ok()
    # every accepted block decodes back to its source (the device's own bytes)
    ok = [k for k, w in enumerate(want) if w]
    round_trip([dst.data(k, got[k]) for k in ok], [chunks[picks[k]] for k in ok], dt, size)


def test_largest_chunk_and_one_byte_more():
    """LZ4MT_HIP_BATCH_MAX_CHUNK bytes with a 64 KiB dictionary equal the oracle and round-trip;
    in the same call one byte more is refused and writes nothing."""
    d = K.fuzz_dict(65536)
    head = K.fuzz_chunks(65536)[15]
    assert len(head) == 70000
    body = B.mixed(MAX_CHUNK + 1 - len(head), 4)
    big, over = head + body[:-1], head + body
    assert len(big) == MAX_CHUNK and len(over) == MAX_CHUNK + 1
    flat, offs = pack([big, over])
    caps = [K.bound(len(big)), K.bound(len(over))]
    dt = dict_tensor(d)
    got, dst = BD.compress_call(flat, offs, [len(big), len(over)], caps, MAX_CHUNK, dt, prepare(dt))
    want = oracle.compress_block_dict(d, big)
    assert oracle.decompress_block_dict(want, len(big), d) == (len(big), big)
    assert oracle.decompress_block_dict(want, len(big), b"")[0] < 0     # it uses the dictionary
    assert got == [len(want), BAD], (got, len(want))
    assert dst.data(0, len(want)) == want
    assert dst.untouched_from(1, 0) and dst.canaries_ok()
    round_trip([dst.data(0, got[0])], [big], dt, "largest chunk")
