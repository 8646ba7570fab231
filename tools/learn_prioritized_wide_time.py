"""What a wide PERD3QN minibatch costs on ONE MI355X (rl_learn_prioritized_wide_draw + rl_learn_prioritized_wide,
reinlife_amd/csrc/rl_learn_prio.hip and rl_learn_dueling_wide.hip) for 1 and 8 learners on FULL rings of 10,000 rows (a PERD3QN brain's
capacity), ONE update per call as PERD3QNAgent.train() makes, the draw and the learning call timed separately:

  prio    device-event times of ONE rl_learn_prioritized_draw (2 launches) and ONE rl_learn_prioritized (1 launch) at batch 64 -- the
          yardsticks, unchanged code, measured in the same process
  pwide   device-event times of ONE rl_learn_prioritized_wide_draw (2 launches: every ring row prepared, then one workgroup per draw) and
          ONE rl_learn_prioritized_wide (6 launches) at batch 64 / 256 / 1024 / 2048
  dwide   device-event time of ONE rl_learn_dueling_wide call on D3QN learners on the same rings at the same batches, its slot table
          drawn once outside the clock -- ALTERNATING with the pwide pair, repetition by repetition, in the same loop

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls in one process; the event pairs include the
launches' host-side issue gaps.

EXPECTATIONS, written down before the first measurement (DESIGN.md 5.26 has the derivations):
  E1  a rl_learn_prioritized_wide call costs what rl_learn_dueling_wide costs at the same batch and learner count, plus the prio_max pass
      over 10,000 floats (one 256-thread workgroup per learner, 40 loads a thread: a few microseconds, hidden beside the target / counter
      pass it rides in).  The tool's own spread on unchanged code is the yardstick: run the command twice; a pwide - dwide difference
      beyond the run-to-run spread of the dwide medians is reported as such.
  E2  the draw grows linearly with n_steps x batch x ring size: one learner at batch 2048 over 10,000 rows is 2.0e7 row visits at about
      29 lane-operations each plus a logf and a divide -- the low tens of microseconds on 256 CUs if nothing else limits it; eight
      learners about eight times that.  Nobody has measured this: the figures are recorded, with whether the draw or the update
      dominates a call at each batch.

    python tools/learn_prioritized_wide_time.py [--out profiles/learn_prioritized_wide.txt] [--reps 200]

No performance threshold is set: the figures are recorded and the expectations judged.  NOT measured here: a trainer() run with
learn_batch={"PERD3QN": B}, hardware counters, several GPUs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_dueling_wide_time import _ring  # noqa: E402

LEARNERS = (1, 8)
BATCHES = (64, 256, 1024, 2048)
RING, N_STEPS, WARM = 10_000, 1, 20


def _stats(t, reps):
    t = sorted(t)
    return t[reps // 2], t[0], t[reps * 9 // 10]


def measure(reps, say):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rng = np.random.RandomState(1)
    rings = [_ring(rng, dev) for _ in range(max(LEARNERS))]
    med = {}

    def events(k):
        return [[torch.cuda.Event(enable_timing=True) for _ in range(k)] for _ in range(reps)]

    def line(tag, part, entry, batch, n, t):
        m, lo, p90 = _stats(t, reps)
        say("%-6s %-5s %s, %d step x batch %d, %d learner(s), ring %d | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions"
            % (tag, part, entry, N_STEPS, batch, n, RING, m, lo, p90, reps))
        med[(tag, part, n, batch)] = m

    for n in LEARNERS:
        # the yardsticks: rl_learn_prioritized_draw + rl_learn_prioritized at batch 64
        ls = [DeviceLearner(Models.PERD3QN(), dev, ring=r, prioritized=True) for r in rings[:n]]
        for _ in range(WARM):
            dw.learn(ls, N_STEPS, slots=dw.draw_prioritized(ls, N_STEPS))
        torch.cuda.synchronize()
        ev = events(3)
        for e in ev:
            e[0].record(); slots = dw.draw_prioritized(ls, N_STEPS); e[1].record(); dw.learn(ls, N_STEPS, slots=slots); e[2].record()
        torch.cuda.synchronize()
        dw.check_error_flag()
        assert all(l.state.cpu().tolist() == [N_STEPS * (WARM + reps), WARM + reps] for l in ls)
        line("prio", "draw", "rl_learn_prioritized_draw", 64, n, [e[0].elapsed_time(e[1]) * 1e3 for e in ev])
        line("prio", "learn", "rl_learn_prioritized", 64, n, [e[1].elapsed_time(e[2]) * 1e3 for e in ev])
        for batch in BATCHES:
            pl = [DeviceLearner(Models.PERD3QN(), dev, ring=r, prioritized=True, prioritized_batch=batch) for r in rings[:n]]
            dl = [DeviceLearner(Models.D3QN(), dev, ring=r, dueling_batch=batch) for r in rings[:n]]
            dslots = dw.draw_slots_rank(dl, N_STEPS)
            for _ in range(WARM):
                dw.learn(pl, N_STEPS, slots=dw.draw_prioritized(pl, N_STEPS))
                dw.learn(dl, N_STEPS, slots=dslots)
            torch.cuda.synchronize()
            ev = events(4)
            for e in ev:   # the two calls alternate, repetition by repetition
                e[0].record(); slots = dw.draw_prioritized(pl, N_STEPS); e[1].record(); dw.learn(pl, N_STEPS, slots=slots); e[2].record()
                dw.learn(dl, N_STEPS, slots=dslots); e[3].record()
            torch.cuda.synchronize()
            dw.check_error_flag()
            assert all(l.state.cpu().tolist() == [N_STEPS * (WARM + reps), WARM + reps] for l in pl + dl)
            assert all(float(l.prio_max.item()) == float(l.priority.max().item()) > 0 for l in pl)
            line("pwide", "draw", "rl_learn_prioritized_wide_draw", batch, n, [e[0].elapsed_time(e[1]) * 1e3 for e in ev])
            line("pwide", "learn", "rl_learn_prioritized_wide", batch, n, [e[1].elapsed_time(e[2]) * 1e3 for e in ev])
            line("dwide", "learn", "rl_learn_dueling_wide", batch, n, [e[2].elapsed_time(e[3]) * 1e3 for e in ev])
            d, p = med[("pwide", "draw", n, batch)], med[("pwide", "learn", n, batch)]
            say("row    %d learner(s), batch %d | draw + update %.2f us = %.4f us per sampled row (rl_learn_prioritized pair: %.4f); the %s dominates (draw %.0f %%)"
                % (n, batch, d + p, (d + p) / (N_STEPS * batch), (med[("prio", "draw", n, 64)] + med[("prio", "learn", n, 64)]) / (N_STEPS * 64),
                   "draw" if d > p else "update", 100 * d / (d + p)))
    return med


def judge(med, say):
    for n in LEARNERS:
        diffs = ["%d: %+.2f us (%+.1f %%)" % (b, med[("pwide", "learn", n, b)] - med[("dwide", "learn", n, b)],
                                             100 * (med[("pwide", "learn", n, b)] / med[("dwide", "learn", n, b)] - 1)) for b in BATCHES]
        say("E1     %d learner(s): rl_learn_prioritized_wide - rl_learn_dueling_wide at batch %s -- compare with the run-to-run spread of the "
            "dwide medians (the command run twice)" % (n, "; ".join(diffs)))
        d = [med[("pwide", "draw", n, b)] for b in BATCHES]
        say("E2     %d learner(s): draw at batch %s = %s us; per draw and ring row %s ns; batch 2048 / batch 64 = %.1f x (32 x if linear from zero)"
            % (n, "/".join(map(str, BATCHES)), " / ".join("%.1f" % x for x in d),
               " / ".join("%.4f" % (1e3 * x / (N_STEPS * b * RING * n)) for x, b in zip(d, BATCHES)), d[-1] / d[0]))
    one, eight = med[("pwide", "draw", 1, 2048)], med[("pwide", "draw", 8, 2048)]
    say("E2     one learner at batch 2048 over %d rows: %.1f us (expected: the low tens of microseconds): %s; eight learners %.1f us = %.1f x "
        "(expected about 8 x)" % (RING, one, "CONFIRMED" if one <= 50 else "REFUTED", eight, eight / one))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    judge(measure(max(args.reps, 200), say), say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_prioritized_wide_time.py on ONE MI355X, one process: device events around one prioritised draw (2 launches) and one\n"
                     "# learning call (rl_learn_prioritized: 1 launch; rl_learn_prioritized_wide and rl_learn_dueling_wide: 6 launches; the event pairs\n"
                     "# include their host-side issue gaps), ONE step per call, 20 warm-up + >= 200 repetitions per figure, full rings of 10,000 rows.\n"
                     "# pwide and dwide alternate in the same loop.  Expected BEFORE measuring (DESIGN.md 5.26): E1 pwide learn = dwide learn + the\n"
                     "# prio_max pass; E2 the draw is linear in n_steps x batch x ring size, low tens of microseconds for one learner at batch 2048.\n"
                     "# NOT measured: a trainer() run with learn_batch={\"PERD3QN\": B}, hardware counters, several GPUs.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
