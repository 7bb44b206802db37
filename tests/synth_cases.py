"""The fixed inputs of the synthesized-block and dictionary-fuzz tests: which
dictionaries, seeds, sizes and profiles they use.  The CPU checks
(test_oracle_dict.py) and the GPU tests (test_gpu_batch_synth.py,
test_gpu_batch_dict_fuzz.py) build the same bytes from here, so what the CPU
checks assert about the inputs -- every block decodes to its plain text with
the oracle, every class of lz4_synth occurs -- holds for what the GPU is fed.
"""
import collections
import functools
import random

import lz4_synth as S
import oracle

# --- synthesized blocks ----------------------------------------------------
SYNTH_DICTS = [8, 9, 63, 64, 4096, 16384, 65535, 65536, 65537, 100000]
N_BLOCKS = 60
BIG = [24000, 40000, 80000, 30000]              # every fifth block: past position 16 384, up to 80 KiB
SMALL = [200, 450, 1000, 2500, 6000, 12000]
N_INVALID = 6
INVALID_SIZES = [200, 3000, 20000]
LOWS = S.DICT_CLASSES
HIGHS = S.DICT_CLASSES[:-1]                     # offsets 1..7 reach below 0 only from P < 7
# an offset one byte below the dictionary's start must fit 16 bits
INVALID_DICTS = [h for h in SYNTH_DICTS if h + max(INVALID_SIZES) + 100 <= S.MAX_OFF]

Block = collections.namedtuple("Block", "block plain profile stats")


@functools.lru_cache(maxsize=None)
def synth_dict(size):
    """Random bytes: a wrong source position shows in every byte."""
    return random.Random(7000 + size).randbytes(size)


@functools.lru_cache(maxsize=None)
def synth_batch(size):
    """([Block], stats summed over the valid blocks) for the dictionary of ``size`` bytes (0: none).
    Read-only: the tests share it."""
    hist = synth_dict(size)
    rnd = random.Random(9000 + size)
    blocks, total = [], collections.Counter()
    for i in range(N_BLOCKS):
        big = i % 5 == 0
        prof = {"kind": "runs" if i % 3 == 1 else "mixed"}
        if size:
            prof["low"] = LOWS[i % len(LOWS)]
            if big:
                prof["high"] = HIGHS[(i // 5) % len(HIGHS)]
        n = BIG[(i // 5) % len(BIG)] if big else SMALL[i % len(SMALL)]
        block, plain, stats = S.synth(rnd, hist, n, prof)
        blocks.append(Block(block, plain, prof, stats))
        total.update(stats)
    if size == 0 or size in INVALID_DICTS:
        for i in range(N_INVALID):
            block, plain, stats = S.synth(rnd, hist, INVALID_SIZES[i % len(INVALID_SIZES)], "invalid")
            assert plain is None
            blocks.append(Block(block, None, "invalid", stats))
    return blocks, total


def required_classes(size):
    """The stats keys that synth_batch(size) must hold at least once."""
    need = [("lit", v) for v in S.LIT_CLASSES] + [("mlen", v) for v in S.MLEN_CLASSES + (S.MLEN_BIG,)]
    need += [("off", c) for c in S.OFF_CLASSES] + [("run", "far"), ("run", "cross4096")]
    need += [("tot", v) for v in S.TOT_CLASSES] + [("far", v) for v in S.FAR_MLEN]
    if size:
        both = ["inside", "end_last", "end_before", "end_after", "over", "over_lap"]
        need += [("dict", r, c) for r in ("low", "high") for c in both] + [("dict", "low", "off1..7")]
        # the dictionary's first byte while an offset reaches it, else the largest offset
        if size <= S.MAX_OFF:
            need.append(("dict", "low", "first_byte"))
        # the "high" class is placed at the first P >= 16 384; a sequence adds 5 300 bytes at the most
        if size <= S.MAX_OFF - 22000:
            need.append(("dict", "high", "first_byte"))
        if size >= S.MAX_OFF:
            need += [("dict", "low", "off_65535"), ("dict", "high", "off_65535")]
        need += [("run", "dict", "high")]
    return need


# --- sources and dictionaries of the encode fuzz ---------------------------
FUZZ_DICTS = [8, 9, 11, 12, 4095, 4096, 4097, 65535, 65536, 65537, 100000]
FUZZ_SIZES = [0, 1, 12, 13, 14, 63, 64, 65, 4095, 4096, 4097, 65535, 65546, 65547, 65548, 70000]
N_RANDOM_SIZES = 8
CAP_KINDS = ["bound", "n", "n-1", "n/3", "random"]


def bound(n):
    return n + n // 255 + 16


@functools.lru_cache(maxsize=None)
def _text():
    return oracle.gen_synthetic(1 << 20, 77)


@functools.lru_cache(maxsize=None)
def fuzz_dict(size, seed=0):
    """Dictionary contents that differ per seed: a mixture with repeats, so the buckets of the
    prepared table collide otherwise than the fixture's text does."""
    return S.fuzz_source(random.Random(100 * size + seed + 1), b"", size, _text())


@functools.lru_cache(maxsize=None)
def fuzz_chunks(size, seed=0):
    """The chunks compressed against fuzz_dict(size, seed): every size of FUZZ_SIZES, random sizes up
    to 20 000, and the hand case whose match starts in the dictionary's tail 20 000 bytes in."""
    d = fuzz_dict(size, seed)
    rnd = random.Random(31 * size + seed)
    sizes = FUZZ_SIZES + [rnd.randrange(1, 20001) for _ in range(N_RANDOM_SIZES)]
    chunks = [S.fuzz_source(rnd, d, n, _text()) for n in sizes]
    if size >= 40:
        chunks.append(S.hand_tail_source(d, rnd.randbytes(20000)))
    return chunks


def caps_of(rnd, n):
    """The capacity of each kind of CAP_KINDS for a chunk of n bytes."""
    return [bound(n), n, max(n - 1, 0), n // 3, rnd.randrange(0, bound(n) + 1)]
