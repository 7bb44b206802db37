"""The first-window fast phase of encode_block_v5 (first windows
only) in the lane model (tools/enc_model.py, encode_xchg(..., phases)): a fast
window is the first window after a match, with k0 = 0, s0 = 1, j1 = 65,
mode = 1 and spanHi = 61 folded into constants, and a window without a stop
leaves the phase.  The model asserts at every fast window that the folded
values (lane positions, roleM, every lane live, lo / hi, step) equal the
general formulas and, at every no-stop exit, that the continuation state the
kernel writes as constants is the one the general foot computes.  The inputs
are built so that a search stops on every lane of the first window and of the
first continuation window, and so that a tag alias removes a fast window's
only stop (the exit that redoes the table writes).  The blocks stay the
oracle's."""
import functools
import os
import random
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import enc_model  # noqa: E402

SWEEP_SEED = 24   # tests/test_gpu_first_window.py runs the same bytes


def _bound(n):
    return n + n // 255 + 16


@functools.lru_cache(maxsize=None)
def _run(name):
    """phases at cap = bound and at cap = n (the 300 000 B three-letter block,
    the slowest in the model: bound only) of one input, each block checked
    against the oracle's"""
    if name == "sweep":
        data = enc_model.literal_run_sweep(300_000, SWEEP_SEED)
    elif name == "abc65547":
        data = bytes(map(random.Random(2).randrange, [3] * 65547))
    elif name == "abc300k":
        data = bytes(map(random.Random(4).randrange, [3] * 300_000))
    elif name == "search2k":
        data = enc_model.long_search_input(100_000, 2 << 10, 5)
    elif name == "search70k":
        data = enc_model.long_search_input(150_000, 70 << 10, 5)
    else:
        raise KeyError(name)
    n, res = len(data), []
    for cap in (_bound(n), n)[:1 if name == "abc300k" else 2]:
        ph = {}
        assert enc_model.encode_xchg(data, cap, ph) == oracle.compress_block(data, cap), (name, cap)
        res.append(ph)
    return res


@pytest.mark.parametrize("name", ["sweep", "abc65547", "abc300k", "search2k", "search70k"])
def test_folded_values_hold_and_blocks_are_the_oracles(name):
    """every assert of the model holds at every window, at cap = bound (the
    phase is open from the first match) and at cap = n (it opens once output
    safety holds)"""
    for ph in _run(name):
        assert ph["fast_windows"] > 0 and ph["entries"] >= 1, ph
        # every fast window either stops or leaves the phase
        assert sum(ph["fast_stop_lanes"]) <= ph["fast_windows"], ph
        assert ph["fast_stop_lanes"][0] == 0 and ph["cont1_stop_lanes"][:2] == [0, 0], ph


def test_sweep_stops_on_every_lane():
    ph = _run("sweep")[0]
    fast, cont = ph["fast_stop_lanes"], ph["cont1_stop_lanes"]
    # TEST lane 1 (back-to-back matches) and every SEARCH lane of the first window
    assert [lane for lane in range(1, 64) if not fast[lane]] == []
    # every SEARCH lane of the first continuation window (the step rises at lane 5, j1 = 3)
    assert [lane for lane in range(2, 64) if not cont[lane]] == []
    # searches that run on into the second continuation window and beyond
    exits = ph["fast_windows"] - sum(fast)
    assert exits > sum(cont) > 0, ph
    # the phase is left and entered once per such search
    assert ph["entries"] >= exits, ph


def test_alias_removes_a_fast_windows_only_stop():
    """the exit taken with twRedo set: the table writes are redone for all 64
    lanes before the phase is left.  (The three-letter blocks alias in nearly
    every window but always keep another stop; the sweep's random literals
    are where an aliased candidate is a window's only one: about 30 exits.)"""
    assert _run("sweep")[0]["fast_exits_redo"] >= 1
    assert sum(_run(name)[0]["fast_exits_redo"] for name in ("search2k", "search70k")) >= 1


@pytest.mark.parametrize("name", ["search2k", "search70k"])
def test_long_search_leaves_and_reenters(name):
    ph = _run(name)[0]
    assert ph["entries"] >= 2 and ph["general_windows"] > 0, ph
    if name == "search70k":   # the step grows to wide windows, all of them in the general phase
        assert ph["wide_general"] > 0, ph
