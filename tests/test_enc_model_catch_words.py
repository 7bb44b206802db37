"""The fast body's catch-up from words and its leaner pending store (DESIGN
4.1, catch-up from words and one-sided ring test) in the lane model (tools/enc_model.py,
encode_xchg(..., catch_words=True)).

With the catch-up from words the fast body reads the 64 bytes below the candidate and below
the stop as 16 words in lanes the count round leaves idle, takes the bound of
the catch-up as w - 1 (the stop's lane) and has no loop for longer catch-ups;
the phase is entered only after a match that ends at or above 65536 + 64.
With the one-sided ring test the pending store's in-ring test is its lower bound alone.  The
model asserts at every stop of a fast window that min(ip - anchor, cd) is
w - 1 <= 62, that the candidate lies 64 bytes or more into the block and that
the catch-up from the words is the byte loop's, and at every pending store of
a fast window that the literals end inside the source ring.

App. F text alone leaves many catch-up lengths out, so the inputs are built
from units (enc_model.catch_up_units) and the tests assert the coverage
itself: every catch-up of 0 .. 61 bytes that eats the literal run whole
(back = w - 1), every one of 0 .. 60 bytes that ends on a differing byte
(back < w - 1), stops on the TEST lane, sequences of 63, 64, 65 and 129
bytes, and literals that have left the ring before their store.  The blocks
stay the oracle's.  tests/test_gpu_catch_words.py runs the same bytes."""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import oracle  # noqa: E402
import enc_model  # noqa: E402

N = 300_000
SEEDS = (1, 2, 3, 4, 5, 6)   # tests/test_gpu_catch_words.py runs the same blocks


@functools.lru_cache(maxsize=None)
def _runs():
    """phases of every unit block at cap = bound, each block the oracle's"""
    res = []
    cap = N + N // 255 + 16
    for seed in SEEDS:
        data = enc_model.catch_up_units(N, seed, enc_model.catch_up_cases())
        ph = {}
        assert enc_model.encode_xchg(data, cap, ph, catch_words=True) == oracle.compress_block(data, cap), seed
        res.append(ph)
    return res


def _sum(key):
    return [sum(col) for col in zip(*(ph[key] for ph in _runs()))]


def test_phase_is_entered_and_asserts_hold():
    for ph in _runs():
        assert ph["entries"] >= 1 and ph["fast_windows"] > ph["general_windows"], ph


def test_catch_up_that_eats_the_literal_run_whole():
    full = _sum("catch_full")
    assert [b for b in range(62) if not full[b]] == []


def test_catch_up_that_ends_on_a_differing_byte():
    part = _sum("catch_part")
    assert [b for b in range(61) if not part[b]] == []


def test_stops_on_the_test_lane_and_on_every_search_lane():
    lanes = _sum("fast_stop_lanes")
    assert lanes[0] == 0 and [lane for lane in range(1, 64) if not lanes[lane]] == []
    # a TEST-lane stop has no catch-up: counted as back = 0 = w - 1
    assert _sum("catch_full")[0] >= lanes[1] > 0


def test_store_lengths_around_one_round_and_literals_out_of_the_ring():
    tot = _sum("fast_store_total")
    assert all(tot[t] for t in (62, 63, 64, 65, 129)), [tot[t] for t in (62, 63, 64, 65, 129)]
    assert tot[130] > 0   # 130 bytes and more (three rounds): the 200-byte literal run
    assert sum(ph["fast_store_left_ring"] for ph in _runs()) > 0


def test_without_the_new_rules_the_model_is_the_parents():
    """catch_words=False: the phase rules of first windows alone (entered from
    the block's first match on), same bytes"""
    data = enc_model.catch_up_units(N, SEEDS[0], enc_model.catch_up_cases())
    cap = N + N // 255 + 16
    old, new = {}, {}
    want = oracle.compress_block(data, cap)
    assert enc_model.encode_xchg(data, cap, old) == want
    assert enc_model.encode_xchg(data, cap, new, catch_words=True) == want
    assert old["fast_windows"] > new["fast_windows"] > 0
    assert sum(old["catch_full"]) == 0 == sum(old["fast_store_total"])


def test_back_from_words_against_the_byte_loop():
    """every length of agreement 0 .. 70 below the two positions, every bound 0 .. 62"""
    base = bytes(range(1, 101)) * 2
    for agree in range(71):
        s = bytearray(base + base)
        ip, cd = 300, 100
        s[ip - agree - 1] ^= 0x80
        for maxb in range(63):
            back = 0
            while back < maxb and s[ip - back - 1] == s[cd - back - 1]:
                back += 1
            assert enc_model.back_from_words(bytes(s), ip, cd, maxb) == back == min(agree, maxb)
