"""The cases of the LZ4-HC dictionary fixtures (tests/golden/dict_hc_blocks.json
and dict_hc_fuzz.json): which dictionaries, chunks, levels and capacities they
hold and how their bytes are made.  Shared by the generator
(tests/golden/make_golden_dict_hc.py), the CPU check (test_dict_hc_golden.py)
and the GPU tests (test_gpu_batch_dict_hc.py).  Inputs come from dict_cases'
generators, plus:

  dictionary "run": r   the dictionary's last r bytes replaced by RUN_BYTE (a
                        value the text does not hold, so the run is r long)
  chunk "tail:k"        the dictionary's last k bytes again and again (a match
                        found in the dictionary runs over its end into the
                        chunk), then 20 random bytes
  chunk "run:l"         l bytes RUN_BYTE, then 40 bytes of text: continues a
                        run that ends the dictionary
A chunk is named by a string: "bd:<n>" (text), "mixed:<n>", "hand:<name>"
(dict_cases.hand_chunk), "tail:<k>", "run:<l>".
"""
import random

import dict_cases as C
import oracle

LEVELS_MAIN = [3, 9, 10, 12]
LEVELS_CAPS = [9, 12]                       # capacities other than the bound: at these levels only
LEVELS_MORE = [4, 5, 6, 7, 8, 11]           # at the 4096-byte dictionary, 1000- and 4096-byte text chunks
DICT_SIZES = [0, 3, 4, 5, 8, 4096, 65535, 65536, 65537, 100000]
CHUNK_SIZES = C.CHUNK_SIZES                 # text
MIXED_SIZES = C.MIXED_SIZES
BIG_CHUNK = C.BIG_CHUNK                     # at the 65536-byte dictionary and level 9 only
HAND_DICTS = C.HAND_DICTS
TAIL_KS = [1, 2, 3, 4, 5, 6, 7, 40, 300]
RUN_TAILS = [1, 2, 3, 4, 8, 50]
RUN_LENS = [3, 10, 100, 1000]
RUN_BYTE = 0xAA
CAP_KINDS = C.CAP_KINDS

bound, cap_of = C.bound, C.cap_of


def dict_spec(size, seed=C.DICT_SEED, run=0):
    return {"kind": "bd", "size": size, "seed": seed, "run": run}


def make_dict(spec):
    d = C.make_dict({"kind": "bd", "size": spec["size"], "seed": spec["seed"]})
    r = spec.get("run", 0)
    assert RUN_BYTE not in d[-r - 1:] or r == 0
    return d[:len(d) - r] + bytes([RUN_BYTE]) * r if r else d


def effective(d):
    """The bytes LZ4_loadDictHC keeps: the last 64 KiB."""
    return d[-C.WINDOW:]


def make_chunk(name, d, seed=C.DICT_SEED):
    kind, _, arg = name.partition(":")
    if kind == "bd":
        return C.make_chunk({"kind": "bd", "n": int(arg), "seed": seed, "skip": C.CHUNK_SKIP}, d)
    if kind == "mixed":
        return C.make_chunk({"kind": "mixed", "n": int(arg), "seed": int(arg)}, d)
    if kind == "hand":
        return C.hand_chunk(name, d)
    if kind == "tail":
        k = int(arg)
        return (effective(d)[-k:] * (700 // k + 1))[:max(700, 3 * k)] + oracle.gen_random(20, k)
    if kind == "run":
        return bytes([RUN_BYTE]) * int(arg) + C.make_chunk({"kind": "bd", "n": 40, "seed": seed, "skip": 7}, d)
    raise KeyError(name)


def plan():
    """[(dict spec, [(chunk name, level, cap kind)])] in fixture order."""
    out = []
    for size in DICT_SIZES:
        chunks = [f"bd:{n}" for n in CHUNK_SIZES] + [f"mixed:{n}" for n in MIXED_SIZES]
        items = [(c, lv, "bound") for lv in LEVELS_MAIN for c in chunks]
        items += [(c, lv, k) for lv in LEVELS_CAPS for c in chunks for k in CAP_KINDS[1:]]
        if size == 4096:
            items += [(f"bd:{n}", lv, "bound") for lv in LEVELS_MORE for n in (1000, 4096)]
        if size == 65536:
            items.append((f"bd:{BIG_CHUNK}", 9, "bound"))
        if size in HAND_DICTS:
            hand = C.HAND + [f"tail:{k}" for k in TAIL_KS]
            items += [(c, lv, "bound") for lv in LEVELS_MAIN for c in hand]
        out.append((dict_spec(size), items))
    for size in HAND_DICTS:
        for r in RUN_TAILS:
            out.append((dict_spec(size, run=r), [(f"run:{n}", lv, "bound") for lv in LEVELS_MAIN for n in RUN_LENS]))
    for seed in C.GRAPH_SEEDS:   # further 4096-byte dictionaries (the graph test swaps them in)
        out.append((dict_spec(4096, seed=seed), [(f"bd:{n}", lv, "bound") for lv in (3, 10) for n in CHUNK_SIZES]))
    return out


# ---- the seeded differential fixture ----
FUZZ_N = 500
FUZZ_SEED = 20261
FUZZ_MAX_CHUNK = 20000
FUZZ_DICTS = [dict_spec(0), dict_spec(5), dict_spec(300, seed=11), dict_spec(4096, seed=12), dict_spec(4096, seed=13, run=6),
              dict_spec(20000, seed=14), dict_spec(65536, seed=15), dict_spec(65536, seed=16, run=3),
              dict_spec(70001, seed=17)]
FUZZ_KINDS = ["text", "near", "mixed", "tail", "run", "random"]


def fuzz_chunk(kind, n, seed, d):
    """n bytes of chunk ``kind``; ``d`` is the case's dictionary."""
    rnd = random.Random(seed)
    e = effective(d)
    if kind == "text":      # the dictionary's text, further on
        t = C._text(C.DICT_SEED)
        a = rnd.randrange(0, len(t) - n)
        out = t[a:a + n]
    elif kind == "near":    # pieces of the dictionary between pieces of random bytes
        out = bytearray()
        while len(out) < n:
            if e and rnd.random() < 0.7:
                a = rnd.randrange(len(e))
                out += e[a:a + rnd.randrange(4, 400)]
            else:
                out += oracle.gen_random(rnd.randrange(1, 40), rnd.randrange(1 << 30))
        out = bytes(out[:n])
    elif kind == "mixed":
        out = C._mixed(n, seed % 1000)
    elif kind == "tail":    # begins with the dictionary's last bytes, repeated
        k = rnd.randrange(1, 64)
        rep = (e[-k:] * (n // max(min(k, len(e)), 1) + 1)) if e else b""
        m = min(n, rnd.randrange(4, 600))
        out = rep[:m] + C._text(C.DICT_SEED)[1000:1000 + n - min(m, len(rep))]
        out = out[:n]
    elif kind == "run":     # begins with a run of the byte the dictionary may end in
        m = min(n, rnd.randrange(1, 300))
        out = bytes([RUN_BYTE]) * m + C._text(C.DICT_SEED)[2000:2000 + n - m]
    else:
        out = oracle.gen_random(n, seed)
    assert len(out) == n, (kind, n, len(out))
    return out


def fuzz_plan():
    """[(dict index, kind, n, seed, level, cap kind)], FUZZ_N of them."""
    rnd = random.Random(FUZZ_SEED)
    out = []
    for i in range(FUZZ_N):
        n = rnd.choice([rnd.randrange(0, 64), rnd.randrange(64, 2000), rnd.randrange(2000, FUZZ_MAX_CHUNK + 1)])
        out.append((rnd.randrange(len(FUZZ_DICTS)), rnd.choice(FUZZ_KINDS), n, rnd.randrange(1 << 30),
                    rnd.randrange(3, 13), rnd.choice(["bound", "bound", "bound", "n", "n-1", "n/3"])))
    return out
