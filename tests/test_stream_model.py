"""The park / relaunch protocol of the streamed engines (k_encode_stream /
k_decode_stream, StreamMonitor::relaunch_locked), restated as a discrete
model of its control words and waits in tools/stream_model.py and run on the
CPU against seeded schedules.

The regime no GPU test of the protocol reached before: every wave holds a
finished block in its output wait and the reader is up to Rin blocks ahead.
There the published blocks between the device counter and the reader's
nextPub_ have no owner at a park, and a relaunch at nextPub_ (what the code
did) never encodes them: the writer waits for a record that never comes.
The relaunch at min(device next, nextPub_) is exact on every schedule of the
sweep below (tests/test_gpu_stream.py holds the same regime on the device)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stream_model as sm  # noqa: E402

SCHEDULES = 200   # per combination of the grid


def _not_writer(s):
    return sm.is_grid_or_io(s) and s != ("writer",)


def _write_stall_scenario(rule):
    """W = 2, Rin = 4, Rout = 1, N = 12; the write() of block 0 stalls;
    everything else to rest; park; the stall ends; relaunch; to rest."""
    m = sm.Model(2, 4, 1, 12, rule, stall=lambda kind, b: kind == "w" and b == 0)
    sm.drain(m, sm.is_grid_or_io)
    assert m.wstall and not m.park
    # block 0 went out without a wait (b < Rout), blocks 1 and 2 are done and
    # wait for the writer, the reader filled the staging ring behind them
    assert (m.held(), m.next, m.pub) == ([1, 2], 3, 7)
    assert [sm.STATE_NAMES[s] for s in m.wst] == ["outwait", "outwait"]
    m.step(("park",))
    sm.drain(m, sm.is_grid_or_io)
    assert [sm.STATE_NAMES[s] for s in m.wst] == ["pend", "pend"] and m.held() == [1, 2]
    assert (m.next, m.pub) == (3, 7)   # nothing was claimed, nothing published while parked
    m.step(("end_wstall",))
    m.step(("relaunch",))
    sm.drain(m, sm.is_grid_or_io)
    return m


def test_parent_rule_is_stuck_in_the_write_stall_scenario():
    """next = nextPub_ at the relaunch: the waves hold blocks 1 and 2, the
    device counter is 3, the reader is at 7; blocks 3..6 are published, never
    taken, and the run is stuck behind block 2."""
    m = _write_stall_scenario(sm.parent_rule)
    assert m.relaunches == [(3, 7, 7)]
    assert m.enabled() == [] and m.outcome() == "stuck"
    assert m.lost() == [3, 4, 5, 6]
    assert m.written == [0, 1, 2]          # the pend blocks went out, then nothing
    assert m.wph == sm.W_WAIT and m.wb == 3   # the writer waits for record 3
    assert m.rph == sm.R_SLOT and m.rb == 7   # the reader waits for block 7's slot: block 3 pulled
    assert sorted(m.wb_) == [7, 8] and list(m.wst) == [sm.INWAIT] * 2   # the waves wait for the reader


def test_min_rule_is_exact_in_the_write_stall_scenario():
    m = _write_stall_scenario(sm.min_rule)
    assert m.relaunches == [(3, 7, 3)]
    assert m.outcome() == "exact" and m.lost() == [] and m.written == list(range(12))


def _read_stall_behind_slow_writer(rule):
    """The mirror: W = 2, Rin = 4, Rout = 1, N = 12; the writer is slow (it
    takes a step only when nothing else can) but never stalls; read() number
    Rout + W + Rin + 2 (block 8) stalls: by then every wave is in its output
    wait again and the park is charged to the read()."""
    m = sm.Model(2, 4, 1, 12, rule, stall=lambda kind, b: kind == "r" and b == 8)
    slow_writer = lambda s: s == ("writer",)   # noqa: E731
    while not m.rstall:
        assert not m.finished()
        sm.drain(m, _not_writer)
        if not m.rstall:
            m.step(("writer",))
    sm.drain(m, _not_writer)
    assert not m.wstall and m.rph == sm.R_READ and m.rb == 8
    assert [sm.STATE_NAMES[s] for s in m.wst] == ["outwait", "outwait"]
    assert (m.held(), m.next, m.pub) == ([3, 4], 5, 8)
    m.step(("park",))
    sm.drain(m, _not_writer)
    assert [sm.STATE_NAMES[s] for s in m.wst] == ["pend", "pend"]
    m.step(("end_rstall",))
    m.step(("relaunch",))
    sm.drain(m, _not_writer, slow_writer)
    return m


def test_parent_rule_loses_blocks_in_the_read_stall_mirror():
    m = _read_stall_behind_slow_writer(sm.parent_rule)
    assert m.relaunches == [(5, 8, 8)]
    assert m.lost() == [5, 6, 7]
    assert m.enabled() == [] and m.outcome() == "stuck" and m.written == [0, 1, 2, 3, 4]


def test_min_rule_is_exact_in_the_read_stall_mirror():
    m = _read_stall_behind_slow_writer(sm.min_rule)
    assert m.relaunches == [(5, 8, 5)]
    assert m.outcome() == "exact" and m.lost() == []


def test_a_relaunch_below_the_lowest_free_block_is_noticed():
    """The model notices a relaunch that is too low as well as one that is
    too high: one block below the rule, a wave claims block 2 again, whose
    staging slot holds block 6 by now, and never leaves its input wait."""
    m = _write_stall_scenario(lambda dev_next, pub: min(dev_next, pub) - 1)
    assert m.written == list(range(12)) and m.outcome() == "stuck"
    assert [(sm.STATE_NAMES[s], b) for s, b in zip(m.wst, m.wb_) if s != sm.GONE] == [("inwait", 2)]


_sweep = {}


def _sweep_results():
    """The min rule over the whole grid, run once for the tests below."""
    if not _sweep:
        for combo in sm.sweep_grid():
            _sweep[combo] = [sm.run_random(*combo, sm.min_rule, seed) for seed in range(SCHEDULES)]
    return _sweep


def test_min_rule_is_exact_on_the_schedule_sweep():
    """W in {1, 2, 5} x Rin in {1, 3, 8} x Rout in {1, 2, 8} x N in {0, 1,
    Rout + W + Rin + 3, 40}: 108 combinations, 200 seeded schedules each
    (21 600 runs, about 12 s); write stalls, read stalls, both at once, a
    stall in the final read(), several parks per run.  Every run ends with
    all N blocks written in order, each once."""
    res = _sweep_results()
    assert len(res) == 108 and SCHEDULES >= 200
    bad = [(combo, seed, m.outcome(), m.wrong) for combo, runs in res.items() for seed, m in enumerate(runs)
           if m.outcome() != "exact" or m.lost()]
    assert not bad, bad[:5]


def test_the_sweep_reaches_the_case_and_mixes_its_stalls():
    """At least a quarter of the sweep's runs relaunch with the device counter
    below the reader's (N = 0 and N = 1, half the grid, never can: after the
    first claims the counter is at least W >= N), and the stalls are mixed."""
    runs = [m for rs in _sweep_results().values() for m in rs]
    reached = sum(m.reached() for m in runs)
    print(f"relaunch below the reader's block in {reached} of {len(runs)} runs")
    assert 4 * reached >= len(runs), (reached, len(runs))
    assert sum(m.parks >= 2 for m in runs) >= len(runs) // 10       # several parks per run
    assert sum(len(m.relaunches) < m.parks for m in runs) > 0       # a park that needs no relaunch (the end)
    assert sum(m.both > 0 for m in runs) >= len(runs) // 20         # a read() and a write() stalled at once
    assert sum(m.last_stall for m in runs) >= len(runs) // 4        # a stall in the read() that returns 0
    assert sum(m.last_stall and m.parks > len(m.relaunches) for m in runs) > 0
    for combo, rs in _sweep_results().items():
        if combo[3] > 1:   # every combination that can reach the case does
            assert sum(m.reached() for m in rs) >= SCHEDULES // 10, combo


def test_parent_rule_fails_wherever_the_sweep_reaches_the_case():
    """The sweep would have caught the old rule: on three combinations, every
    schedule that relaunches with the device counter below the reader's ends
    stuck with blocks lost, every other one exact."""
    hit = 0
    for combo in ((2, 3, 2, 40), (5, 8, 8, 24), (1, 1, 1, 6)):
        for seed in range(SCHEDULES):
            m = sm.run_random(*combo, sm.parent_rule, seed)
            if m.reached():
                hit += 1
                assert m.outcome() == "stuck" and m.lost(), (combo, seed)
            else:
                assert m.outcome() == "exact", (combo, seed)
    assert hit >= 150, hit
