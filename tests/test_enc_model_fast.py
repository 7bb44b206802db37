"""The two phases of encode_block_v5's window loop in the lane
model (tools/enc_model.py, encode_xchg(..., phases)): the model carries the
kernel's phase rules beside the parse and asserts at every fast-phase window
that each thing the kernel's fast body drops -- the live / terminating lane
predicates, the clamps of hi, of the round trip's addresses and of the first
count round, the wide-window test, the two limitedOutput margin tests, the
last-literals test once output safety is established -- has the value the
fast body assumes.  The blocks stay the oracle's."""
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import enc_model  # noqa: E402


def _near_incompressible(n, seed):
    """random runs of 0.3 .. 16 KB, each followed by a repeat of 100 .. 400
    earlier bytes: searches long enough for wide windows (about 10 KB without
    a match) between matches, output within a few hundred bytes of n"""
    rnd = random.Random(seed)
    out = bytearray(oracle.gen_random(2000, seed))
    while len(out) < n:
        out += oracle.gen_random(rnd.randrange(300, 16_000), rnd.randrange(1 << 30))
        a = rnd.randrange(max(0, len(out) - 60_000), len(out) - 400)
        out += out[a:a + rnd.randrange(100, 400)]
    return bytes(out[:n])


def _cases():
    rnd = random.Random(2)
    yield "abc", bytes(rnd.randrange(3) for _ in range(65547))
    yield "appf", oracle.gen_synthetic(70_000, 3)
    yield "near_incompressible", _near_incompressible(120_000, 7)
    yield "zeros_then_random", bytes(40_000) + oracle.gen_random(40_000, 9)


@pytest.mark.parametrize("name,data", list(_cases()), ids=[c[0] for c in _cases()])
def test_fast_phase_assumptions_hold_at_every_window(name, data):
    n = len(data)
    bound = n + n // 255 + 16
    caps = [n, bound]
    if name == "appf":   # a cap near the compressed size: (b) comes true late
        caps.append(len(oracle.compress_block(data, bound)) + 70)
    for cap in caps:
        ph = {}
        assert enc_model.encode_xchg(data, cap, ph) == oracle.compress_block(data, cap), (name, cap)
        if name in ("abc", "appf") and cap >= n:
            # cap = n: (b) comes true early in the block; unlimited: nothing to prove
            assert ph["entries"] >= 1 and ph["fast_windows"] > 4 * ph["general_windows"], (cap, ph)
        if name == "near_incompressible" and cap == bound:
            # wide windows occur, all of them in the general phase, and the
            # fast phase is entered again after the matches that follow
            assert ph["wide_general"] > 0 and ph["entries"] >= 2 and ph["fast_windows"] > 0, ph


def test_window_state_formulas():
    """The kernel carries sBase, s0, j1 and spanHi across continuation
    windows instead of probe offsets: they equal the model's poff(k), and
    spanHi <= 1016 bounds the step by 16 (the fast phase's end distance
    counts on 17 for p + step)."""
    sBase, k0, s0, j1, spanHi = 1, 0, 1, 65, 61
    for _ in range(40):
        assert sBase == 1 + enc_model.poff(k0)
        assert spanHi == enc_model.poff(k0 + 61) - enc_model.poff(k0)
        for j in range(62):
            assert sBase + j * s0 + max(0, j - j1) == 1 + enc_model.poff(k0 + j)
        if spanHi <= enc_model.FAST_SPAN_MAX:
            assert s0 <= 16
        sBase += 62 * s0 + (62 - j1 if 62 > j1 else 0)
        k0 += 62
        s0 = (63 + k0) >> 6
        j1 = (65 if k0 < 65 else ((k0 - 1) & ~63) + 65) - k0
        spanHi = 61 * s0 + (61 - j1 if 61 > j1 else 0)
