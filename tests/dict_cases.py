"""The cases of the dictionary fixture (tests/golden/dict_blocks.json): which
dictionaries, chunks and capacities it holds and how their bytes are made.
Shared by the generator (tests/golden/make_golden_dict.py), the CPU check
(test_dict_golden.py) and the GPU tests (test_gpu_batch_dict.py); every input
comes from a generator that exists on any host, identified by kind, size and
seed:

  "bd"      bytes [skip, skip + n) of conftest.bd_input(TEXT_N, seed): word-like
            text.  A dictionary is the text's first bytes (skip 0), a chunk lies
            CHUNK_SKIP into the same text, so the dictionary holds its words
  "mixed"   test_gpu_hc._mixed(n, seed)
  "random"  oracle.gen_random(n, seed)
  "zeros"   n zero bytes
  "hand:*"  built from the entry's dictionary (hand_chunk)
"""
import functools

import oracle
from conftest import bd_input

TEXT_N = 500_000
CHUNK_SKIP = 100_000
DICT_SEED = 5
GRAPH_SEEDS = (6, 7)          # further 4096-byte dictionaries (the graph test swaps them in)
DICT_SIZES = [0, 7, 8, 9, 10, 11, 4096, 65535, 65536, 65537, 100000]
CHUNK_SIZES = [0, 1, 12, 13, 64, 1000, 4096, 65535, 70000]
BIG_CHUNK = 300000            # at the 65536-byte dictionary only
MIXED_SIZES = [1000, 4096, 70000]
CAP_KINDS = ["bound", "n", "n-1", "n/3"]
HAND = ["hand:over_end", "hand:dict_start", "hand:last_inserted", "hand:random", "hand:zeros"]
HAND_DICTS = [4096, 65536]
WINDOW = 65536


def bound(n):
    return n + n // 255 + 16


def cap_of(kind, n):
    return {"bound": bound(n), "n": n, "n-1": max(n - 1, 0), "n/3": n // 3}[kind]


@functools.lru_cache(maxsize=None)
def _text(seed):
    return bd_input(TEXT_N, seed)


@functools.lru_cache(maxsize=None)
def _mixed(n, seed):
    from test_gpu_hc import _mixed as mixed
    return mixed(n, seed)


def make_dict(spec):
    assert spec["kind"] == "bd"
    return _text(spec["seed"])[:spec["size"]]


def effective(d):
    """The bytes LZ4_loadDict keeps: the last 64 KiB, nothing below 8 bytes."""
    return b"" if len(d) < 8 else d[-WINDOW:]


def hand_chunk(kind, d):
    """Hand-built chunks against dictionary ``d`` (4096 or 65536 bytes)."""
    e = effective(d)
    if kind == "hand:over_end":
        # the dictionary's last 40 bytes, then the chunk's own first bytes again and again:
        # the match found in the dictionary runs over its end into the chunk
        return (e[-40:] * 8)[:300] + oracle.gen_random(20, 1)
    if kind == "hand:dict_start":
        # one foreign byte, then the dictionary's first 200 bytes: the catch-up stops at the dictionary's start
        return bytes([e[0] ^ 0xFF]) + e[:200] + oracle.gen_random(20, 2)
    if kind == "hand:last_inserted":
        # the 8 bytes at the last position loadDict inserts (the last p = start + 3k <= end - 8)
        p = 3 * ((len(e) - 8) // 3)
        return oracle.gen_random(16, 3) + e[p:p + 8] + oracle.gen_random(16, 4)
    if kind == "hand:random":
        return oracle.gen_random(1000, 9)
    if kind == "hand:zeros":
        return bytes(1000)
    raise KeyError(kind)


def make_chunk(spec, d):
    kind, n, seed = spec["kind"], spec["n"], spec["seed"]
    if kind == "bd":
        out = _text(seed)[spec["skip"]:spec["skip"] + n]
    elif kind == "mixed":
        out = _mixed(n, seed)
    elif kind == "random":
        out = oracle.gen_random(n, seed)
    elif kind == "zeros":
        out = bytes(n)
    else:
        out = hand_chunk(kind, d)
    assert len(out) == n, (spec, len(out))
    return out


def compress_plan():
    """[(dict spec, [(chunk spec, cap kind)])] in fixture order."""
    plan = []
    for size in DICT_SIZES:
        dspec = {"kind": "bd", "size": size, "seed": DICT_SEED}
        d = make_dict(dspec)
        chunks = [{"kind": "bd", "n": n, "seed": DICT_SEED, "skip": CHUNK_SKIP}
                  for n in CHUNK_SIZES + ([BIG_CHUNK] if size == 65536 else [])]
        chunks += [{"kind": "mixed", "n": n, "seed": n} for n in MIXED_SIZES]
        if size in HAND_DICTS:
            chunks += [{"kind": k, "n": len(hand_chunk(k, d)), "seed": 0} for k in HAND]
        plan.append((dspec, [(c, k) for c in chunks for k in CAP_KINDS]))
    for seed in GRAPH_SEEDS:
        dspec = {"kind": "bd", "size": 4096, "seed": seed}
        plan.append((dspec, [({"kind": "bd", "n": n, "seed": seed, "skip": CHUNK_SKIP}, "bound")
                             for n in CHUNK_SIZES]))
    return plan
