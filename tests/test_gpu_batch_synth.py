"""The batched decoders on blocks no lz4 encoder writes (lz4_synth.py):
k_decode_batch and k_decode_batch_dict against the plain text the synthesizer
computed byte by byte -- no decoder, the oracle included, stands behind the
expected bytes of a valid block.  The fixed batches (synth_cases.py) hold
every literal-run, match-length, offset and dictionary class per dictionary
size; tests/test_oracle_dict.py asserts that on the CPU.  Negative return
values, and the damaged blocks of the last test, are the oracle's
(LZ4_decompress_safe / LZ4_decompress_safe_usingDict restated, pinned against
liblz4).  Everything is bit-exact.

Inputs are packed as test_gpu_batch.py packs them (chunk starts at every
offset mod 16, the last block on the tensor's last byte, 32 canary bytes after
every capacity); the dictionary starts at an odd address and ends on its
tensor's last byte.
"""
import random

import pytest
import torch

import lz4_synth as S
import oracle
import synth_cases as K
import test_gpu_batch as B
import test_gpu_batch_dict as BD
from test_gpu_batch import pack
from test_gpu_batch_dict import dict_tensor

pytestmark = pytest.mark.gpu

INVALID_CAP = 1 << 17


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    import lz4mt_amd
    assert lz4mt_amd.device_count() > 0
    B.L = BD.L = lz4mt_amd      # the helpers of both modules call the library through their module's handle
    return lz4mt_amd


def decode(blocks, picks, caps, d):
    """One decompress call over entries (index into ``blocks``, capacity); with a dictionary of
    ``d`` bytes lz4mtHipDecompressBatchDict, without one (None) lz4mtHipDecompressBatch."""
    flat, offs = pack(blocks)
    soffs, sizes = [offs[i] for i in picks], [len(blocks[i]) for i in picks]
    if d is None:
        return B.decompress_call(flat, soffs, sizes, caps)
    return BD.decompress_call(flat, soffs, sizes, caps, dict_tensor(d))


def check_synth_batch(size, d):
    batch, _ = K.synth_batch(size)
    hist = K.synth_dict(size)
    blocks = [b.block for b in batch]
    picks, caps, want = [], [], []
    for i, b in enumerate(batch):
        if b.plain is None:
            picks.append(i)
            caps.append(INVALID_CAP)
            want.append(oracle.decompress_block_dict(b.block, INVALID_CAP, hist))
            assert want[-1][0] < 0
            continue
        n = len(b.plain)
        for cap in (n, n + 1, n + 100):
            picks.append(i)
            caps.append(cap)
            want.append((n, b.plain))
        picks.append(i)
        caps.append(n - 1)
        want.append(oracle.decompress_block_dict(b.block, n - 1, hist))
        assert want[-1][0] < 0
    got, dst = decode(blocks, picks, caps, d)
    for k, (i, cap, (ret, out)) in enumerate(zip(picks, caps, want)):
        assert got[k] == ret, (size, i, batch[i].profile, cap, got[k], ret)
        if ret >= 0:
            assert dst.data(k, ret) == out, (size, i, batch[i].profile, cap)
    assert dst.canaries_ok(), size


def test_synthesized_blocks_no_dictionary():
    check_synth_batch(0, None)


def test_synthesized_blocks_no_dictionary_through_the_dictionary_call():
    """dictSize 0 is the plain decoder (k_decode_batch behind lz4mtHipDecompressBatchDict)."""
    check_synth_batch(0, b"")


@pytest.mark.parametrize("size", K.SYNTH_DICTS)
def test_synthesized_blocks_with_dictionary(size):
    check_synth_batch(size, K.synth_dict(size))


@pytest.mark.parametrize("size", [4096, 65536])
def test_damaged_blocks(size):
    """Bit flips, truncations and appended bytes of synthesized blocks and of oracle-compressed
    dictionary blocks, at capacities 0, n - 1, n and n + 100: return value and bytes are
    LZ4_decompress_safe_usingDict's, canaries intact (a refused chunk writes nothing past its capacity)."""
    rnd = random.Random(size + 17)
    # synthesized blocks (their own random dictionary), then the encode fuzz's chunks (theirs)
    groups = [(K.synth_dict(size), [(b.block, len(b.plain)) for b in K.synth_batch(size)[0]
                                    if b.plain is not None and len(b.plain) <= 12000]),
              (K.fuzz_dict(size), [(oracle.compress_block_dict(K.fuzz_dict(size), c), len(c))
                                   for c in K.fuzz_chunks(size) if 0 < len(c) <= 20000])]
    for d, good in groups:
        assert len(good) >= 15
        blocks, picks, caps = [], [], []
        for blk, n in good:
            for v in S.damaged(rnd, blk):
                blocks.append(v)
                for cap in (0, n - 1, n, n + 100):
                    picks.append(len(blocks) - 1)
                    caps.append(cap)
        got, dst = decode(blocks, picks, caps, d)
        accepted = 0
        for k, (i, cap) in enumerate(zip(picks, caps)):
            ret, out = oracle.decompress_block_dict(blocks[i], cap, d)
            assert got[k] == ret, (size, i, len(blocks[i]), cap, got[k], ret)
            if ret >= 0:
                assert dst.data(k, ret) == out, (size, i, cap)
                accepted += 1
        assert dst.canaries_ok(), size
        assert 0 < accepted < len(picks)    # some damage decodes (to other bytes), most is refused
