"""Discrete model of the park / relaunch protocol of the streamed engines
(k_encode_stream / k_decode_stream in lz4mt_kernels.hip; compress_streamed,
decompress_streamed and StreamMonitor in lz4mt_frame.cpp) for the CPU: the
control words and the waits only, no payload bytes.

State, as in the code:
  next                  the device block counter (dNext)
  pub                   the reader's published count (StreamMonitor::nextPub_)
  in_seq / in_pulled    per staging slot: {seq = b + 1, pulled = b + 1}
  out_seq / out_written per output slot:  {seq = b + 1, written = b + 1}
  waves                 W of them, each: about to claim | input wait for b |
                        working on b (before / after the pull) | output wait
                        with b | pushing b | gone with pend b | gone
  park                  the park word g[7] (and the monitor's parked_)
  total                 g[0], set once the reader ends
  rb / wb               the reader's / the writer's position
  rstall / wstall       "inside a read() / write() that has run past the
                        park threshold"

Atomic steps (Model.enabled() lists them, Model.step() takes one):
  ("claim", w)     b = next++, then the input wait
  ("inwait", w)    slot word == b + 1: ok; else b >= total: gone (ended);
                   else park: gone -- stream_wait looks at the slot word
                   again after it has seen the park word, so a published
                   block is still taken (the same order of checks here)
  ("pull", w)      the staging slot is marked pulled
  ("work", w)      the block is encoded / decoded
  ("outwait", w)   b < Rout: no wait; written == b - Rout + 1: ok; else park:
                   gone with pend b
  ("push", w)      out_seq = b + 1
  ("reader",)      waits for slot b - Rin pulled, enters read() (a stall may
                   begin), leaves it (0 bytes at b == N: total = N), publishes
                   -- only while not parked
  ("writer",)      waits for out_seq == b + 1, enters write() (a stall may
                   begin), leaves it: written = b + 1
  ("end_rstall",) / ("end_wstall",)   the stalled callback gets on
  ("park",)        only while a stalled flag is up
  ("relaunch",)    only parked, no stalled flag up, every wave gone:
                   next = rule(next, pub); a wave with a pend resumes that
                   block at its output wait, the others claim

A run ends "exact" (all N blocks written, in order, each once, and every wave
gone), "stuck" (no step enabled, or a wave left in a wait for good: on the
machine, the engine's wait timeout) or "wrong" (a block pulled, pushed or
written twice or out of order).

usage: python tools/stream_model.py [seeds]   (the two rules on a small sweep)
"""
import random
import sys

CLAIM, INWAIT, PULL, WORK, OUTWAIT, PUSH, PEND, GONE = range(8)
STATE_NAMES = ("claim", "inwait", "pull", "work", "outwait", "push", "pend", "gone")
R_SLOT, R_READ, R_PUBLISH, R_DONE = range(4)
W_WAIT, W_WRITE, W_DONE = range(3)


def parent_rule(dev_next, pub):
    """What relaunch_locked did before: the reader's next block."""
    return pub


def min_rule(dev_next, pub):
    """The lowest block nobody took: claimed numbers >= pub were given up in
    an input wait, every claimed number < pub was published and so taken."""
    return min(dev_next, pub)


class Model:
    def __init__(self, W, Rin, Rout, N, rule, stall=None):
        """stall(kind, b) -> bool: whether the read() / write() ("r" / "w") of
        block b stalls past the park threshold (b == N: the final read())."""
        self.W, self.Rin, self.Rout, self.N, self.rule = W, Rin, Rout, N, rule
        self.stall = stall or (lambda kind, b: False)
        self.next = 0
        self.pub = 0
        self.in_seq = [0] * Rin
        self.in_pulled = [0] * Rin
        self.out_seq = [0] * Rout
        self.out_written = [0] * Rout
        self.wst = [CLAIM] * W
        self.wb_ = [-1] * W          # the block a wave holds / waits for
        self.park = False
        self.total = None
        self.rb, self.rph = 0, R_SLOT
        self.wb, self.wph = 0, W_WAIT
        self.rstall = self.wstall = False
        self.pulled = [0] * N        # times each block was pulled / pushed
        self.pushed = [0] * N
        self.written = []
        self.relaunches = []         # (device next, pub, relaunched at)
        self.parks = 0
        self.both = 0                # stalls that began while the other callback was stalled
        self.last_stall = False      # the final read() stalled
        self.wrong = None

    # -- which steps can be taken now -------------------------------------
    def _wave_enabled(self, w):
        s, b = self.wst[w], self.wb_[w]
        if s == INWAIT:
            return (self.in_seq[b % self.Rin] == b + 1 or (self.total is not None and b >= self.total)
                    or self.park)
        if s == OUTWAIT:
            return b < self.Rout or self.out_written[b % self.Rout] == b - self.Rout + 1 or self.park
        return s < PEND

    def _reader_enabled(self):
        p, b = self.rph, self.rb
        if p == R_SLOT:
            return b < self.Rin or self.in_pulled[b % self.Rin] == b - self.Rin + 1
        if p == R_READ:
            return not self.rstall
        return p == R_PUBLISH and not self.park

    def _writer_enabled(self):
        if self.wph == W_WAIT:
            return self.out_seq[self.wb % self.Rout] == self.wb + 1 or (self.total is not None and
                                                                        self.wb >= self.total)
        return self.wph == W_WRITE and not self.wstall

    def enabled(self):
        out = [(STATE_NAMES[self.wst[w]], w) for w in range(self.W) if self._wave_enabled(w)]
        if self._reader_enabled():
            out.append(("reader",))
        if self._writer_enabled():
            out.append(("writer",))
        if self.rstall:
            out.append(("end_rstall",))
        if self.wstall:
            out.append(("end_wstall",))
        if (self.rstall or self.wstall) and not self.park:
            out.append(("park",))
        if self.park and not self.rstall and not self.wstall and all(s >= PEND for s in self.wst):
            out.append(("relaunch",))
        return out

    # -- one step -----------------------------------------------------------
    def step(self, st):
        k = st[0]
        if len(st) == 2:
            self._wave_step(st[1])
        elif k == "reader":
            self._reader_step()
        elif k == "writer":
            self._writer_step()
        elif k == "end_rstall":
            self.rstall = False
        elif k == "end_wstall":
            self.wstall = False
        elif k == "park":
            assert (self.rstall or self.wstall) and not self.park
            self.park = True
            self.parks += 1
        elif k == "relaunch":
            assert self.park and not self.rstall and not self.wstall
            at = self.rule(self.next, self.pub)
            self.relaunches.append((self.next, self.pub, at))
            self.next = at
            self.park = False
            for w in range(self.W):
                assert self.wst[w] >= PEND
                self.wst[w] = OUTWAIT if self.wst[w] == PEND else CLAIM
        else:
            raise ValueError(st)

    def _wave_step(self, w):
        s, b = self.wst[w], self.wb_[w]
        if s == CLAIM:
            self.wb_[w] = self.next
            self.next += 1
            self.wst[w] = INWAIT
        elif s == INWAIT:
            if self.in_seq[b % self.Rin] == b + 1:
                self.wst[w] = PULL
            else:   # ended, or parked with the block still not there
                assert (self.total is not None and b >= self.total) or self.park
                self.wst[w] = GONE
        elif s == PULL:
            if self.pulled[b]:
                self.wrong = f"block {b} pulled twice"
            self.pulled[b] += 1
            self.in_pulled[b % self.Rin] = b + 1
            self.wst[w] = WORK
        elif s == WORK:
            self.wst[w] = OUTWAIT
        elif s == OUTWAIT:
            if b < self.Rout or self.out_written[b % self.Rout] == b - self.Rout + 1:
                self.wst[w] = PUSH
            else:
                assert self.park
                self.wst[w] = PEND
        elif s == PUSH:
            if self.pushed[b]:
                self.wrong = f"block {b} pushed twice"
            self.pushed[b] += 1
            self.out_seq[b % self.Rout] = b + 1
            self.wst[w] = CLAIM
        else:
            raise ValueError((w, s))

    def _reader_step(self):
        b = self.rb
        if self.rph == R_SLOT:
            self.rph = R_READ
            self.rstall = bool(self.stall("r", b))
            self.both += self.rstall and self.wstall
            self.last_stall |= self.rstall and b == self.N
        elif self.rph == R_READ:
            assert not self.rstall
            if b == self.N:   # read() returned 0
                self.total = b
                self.rph = R_DONE
            else:
                self.rph = R_PUBLISH
        elif self.rph == R_PUBLISH:
            assert not self.park
            self.in_seq[b % self.Rin] = b + 1
            self.pub = b + 1
            self.rb = b + 1
            self.rph = R_SLOT
        else:
            raise ValueError("reader done")

    def _writer_step(self):
        b = self.wb
        if self.wph == W_WAIT:
            if self.out_seq[b % self.Rout] == b + 1:
                self.wph = W_WRITE
                self.wstall = bool(self.stall("w", b))
                self.both += self.wstall and self.rstall
            else:
                assert self.total is not None and b >= self.total
                self.wph = W_DONE
        elif self.wph == W_WRITE:
            assert not self.wstall
            if self.written and self.written[-1] != b - 1 or (not self.written and b != 0):
                self.wrong = f"block {b} written out of order"
            self.written.append(b)
            self.out_written[b % self.Rout] = b + 1
            self.wb = b + 1
            self.wph = W_WAIT
        else:
            raise ValueError("writer done")

    # -- results ------------------------------------------------------------
    def finished(self):
        """Wrong, or the writer is done and the grid has come to rest."""
        return self.wrong is not None or (self.wph == W_DONE and
                                          not any(self._wave_enabled(w) for w in range(self.W)))

    def outcome(self):
        if self.wrong is not None:
            return "wrong"
        if self.wph != W_DONE:
            return "stuck"
        if self.written != list(range(self.N)):
            return "wrong"
        # the call then waits for the grid: a wave still in a wait ends it by the timeout
        return "exact" if all(s == GONE for s in self.wst) else "stuck"

    def lost(self):
        """Published blocks that no wave took."""
        return [b for b in range(self.pub) if not self.pulled[b]]

    def held(self):
        """The blocks the waves hold (output wait or pend), sorted."""
        return sorted(self.wb_[w] for w in range(self.W) if self.wst[w] in (OUTWAIT, PEND))

    def reached(self):
        """A relaunch happened with the device counter below the reader's."""
        return any(d < p for d, p, _ in self.relaunches)


def drain(m, *tiers, limit=100000):
    """Takes steps until none of the tiers has one: always the first enabled
    step of the first tier (a predicate on the step) that has any."""
    for _ in range(limit):
        if m.finished():
            return
        en = m.enabled()
        for t in tiers:
            pick = [s for s in en if t(s)]
            if pick:
                m.step(pick[0])
                break
        else:
            return
    raise RuntimeError("drain: no end")


def is_grid_or_io(s):
    """Every step but the stalls' ends and the monitor's."""
    return s[0] not in ("end_rstall", "end_wstall", "park", "relaunch")


def run_random(W, Rin, Rout, N, rule, seed, limit=200000):
    """One seeded schedule.  Six in seven runs are "deep": a stalled callback
    stays stalled and the monitor parks only once everything else has come to
    rest (the reader as far ahead as the staging ring lets it, every wave in
    its output wait), which is where the device counter falls behind the
    reader's; the others take every enabled step with equal weight, so stalls
    also end before the park and parks catch the grid mid-way.  Per run the
    seed also draws how often read() and write() stall, whether the final
    read() does, and how slow the writer is against the rest."""
    rnd = random.Random(seed)
    deep = rnd.random() < 0.85
    p_w = rnd.choice((0.0, 0.1, 0.3, 0.5))
    p_r = rnd.choice((0.0, 0.05, 0.15))
    if p_w == 0.0 and p_r == 0.0:
        p_w = 0.15
    p_last = rnd.choice((0.0, 1.0))
    w_weight = rnd.choice((1.0, 1.0, 0.05))   # a slow writer: the mirror scenario

    def stall(kind, b):
        if kind == "r":
            return rnd.random() < (p_last if b == N else p_r)
        return rnd.random() < p_w

    m = Model(W, Rin, Rout, N, rule, stall)
    for _ in range(limit):
        if m.finished():
            return m
        en = m.enabled()
        if not en:
            return m
        if deep and (m.rstall or m.wstall) and not m.park:
            rest = [s for s in en if is_grid_or_io(s)]
            en = rest if rest else [("park",)]
        if w_weight != 1.0 and len(en) > 1 and ("writer",) in en and rnd.random() > w_weight:
            en = [s for s in en if s != ("writer",)]
        m.step(en[rnd.randrange(len(en))] if len(en) > 1 else en[0])
    raise RuntimeError(f"run_random: no end ({W}, {Rin}, {Rout}, {N}, seed {seed})")


def sweep_grid():
    for W in (1, 2, 5):
        for Rin in (1, 3, 8):
            for Rout in (1, 2, 8):
                for N in (0, 1, Rout + W + Rin + 3, 40):
                    yield W, Rin, Rout, N


def main():
    seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    for name, rule in (("parent: next = nextPub_", parent_rule), ("min(device next, nextPub_)", min_rule)):
        tally = {"exact": 0, "stuck": 0, "wrong": 0}
        reached = runs = 0
        for W, Rin, Rout, N in sweep_grid():
            for seed in range(seeds):
                m = run_random(W, Rin, Rout, N, rule, seed)
                tally[m.outcome()] += 1
                reached += m.reached()
                runs += 1
        print(f"{name}: {runs} runs {tally}, relaunch below the reader's block in {reached}")


if __name__ == "__main__":
    main()
