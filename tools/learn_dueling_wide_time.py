"""What a wide D3QN minibatch costs on ONE MI355X (rl_learn_dueling_wide, reinlife_amd/csrc/rl_learn_dueling_wide.hip) next to
rl_learn_dueling, for 1 and 8 learners on FULL rings of 10,000 rows (a D3QN brain's capacity), ONE update per call as D3QNAgent.train()
makes:

  duel    device-event time of ONE rl_learn_dueling call: 1 step x batch 64, one launch, one 512-thread workgroup per learner -- the
          yardstick, unchanged code, measured in the same process
  wide    device-event time of ONE rl_learn_dueling_wide call: 1 step x batch 64 / 256 / 1024 / 2048, 3 + 3 = 6 launches, one workgroup
          per (learner, 64-row tile) in the two tile passes; the event pair includes the launches' host-side issue gaps

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls in one process; the slot tables are drawn once
(DeviceWorlds.draw_slots_rank), outside the clock.  The line to read is "us per sampled row": the call's median over its batch rows.

EXPECTATION, written down before the first measurement and derived from the code alone:
  E1  a wide step costs about one rl_learn_dueling step plus one extra eval forward plus five launch gaps.  Per row, a forward pass is
      53.5 k multiply-adds (153 x 128 + 2 x 128 x 128 + 9 x 128) and the backward pass 87 k (the two 128 x 128 transposed products and
      the weight gradients), so a k_learn_d3qn step is 2 x 53.5 + 87 = 194 k and the extra forward adds 28 %; a launch gap on this
      runtime is taken as 6 us.  expected(one tile) = 1.28 x duel + 30 us.  Called CONFIRMED when the measured one-tile call is within
      25 % of that, REFUTED otherwise -- and said plainly when the one-tile call is slower than rl_learn_dueling itself (E1 expects so).
  E2  the cost per sampled row falls by about the tile count while learners x tiles <= 256 CUs: the 158 KB of LDS let one workgroup
      onto a CU, so every tile of such a call runs at once and the call takes what the one-tile call takes (the apply pass reads
      T x 216 KB per learner more: microseconds).  8 learners x 2048 rows = 256 tiles is the edge; beyond it tiles queue.  Called
      CONFIRMED when every call with learners x tiles <= 256 takes at most 1.25 x the one-tile call of the same learner count.

    python tools/learn_dueling_wide_time.py [--out profiles/learn_dueling_wide.txt] [--reps 200]

No performance threshold is set: the figures are recorded and the two expectations judged.  NOT measured here: a trainer() run with
learn_batch={"D3QN": B}, hardware counters, several GPUs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LEARNERS = (1, 8)
BATCHES = (64, 256, 1024, 2048)
RING, N_STEPS, TILE, CUS = 10_000, 1, 64, 256
EXTRA_FORWARD, GAPS_US, WITHIN = 0.28, 5 * 6.0, 0.25


def _ring(rng, dev):
    import numpy as np
    import torch

    def rows():
        x = (rng.random_sample((RING, 153)) < 0.15) * rng.choice(np.array([1.0, -1.0, 0.5], np.float32), size=(RING, 153))
        return torch.as_tensor(x.astype(np.float32), device=dev)
    return {"state": rows(), "state_prime": rows(), "action": torch.as_tensor(rng.randint(0, 8, size=RING).astype(np.int8), device=dev),
            "reward": torch.as_tensor(rng.choice(np.array([0, 0.05, 0.3, -1, 5, -10], np.float32), size=RING), device=dev),
            "done": torch.as_tensor((rng.random_sample(RING) < 0.2).astype(np.uint8), device=dev), "prob": None,
            "age": torch.as_tensor(rng.randint(0, 200, size=RING).astype(np.int32), device=dev),
            "count": torch.full((1,), RING, dtype=torch.int64, device=dev)}


def _time(fn, reps):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); fn(); e[1].record()
    torch.cuda.synchronize()
    return sorted(e[0].elapsed_time(e[1]) * 1e3 for e in ev)


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
    for n in LEARNERS:
        for entry, batch in [("rl_learn_dueling", 64)] + [("rl_learn_dueling_wide", b) for b in BATCHES]:
            wide = {"dueling_batch": batch} if entry == "rl_learn_dueling_wide" else {}
            ls = [DeviceLearner(Models.D3QN(), dev, ring=r, **wide) for r in rings[:n]]
            slots = dw.draw_slots_rank(ls, N_STEPS)
            torch.cuda.synchronize()
            t = _time(lambda: dw.learn(ls, N_STEPS, slots=slots), reps)
            dw.check_error_flag()
            assert all(l.state.cpu().tolist() == [N_STEPS * (20 + reps), 20 + reps] for l in ls)
            tag = "duel" if entry == "rl_learn_dueling" else "wide"
            what = "%s, %d step x batch %d, %d learner(s), ring %d" % (entry, N_STEPS, batch, n, RING)
            say("%-6s %s | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions" % (tag, what, t[reps // 2], t[0], t[reps * 9 // 10], reps))
            med[(tag, n, batch)] = t[reps // 2]
            per_row, base = t[reps // 2] / (N_STEPS * batch), med[("duel", n, 64)] / (N_STEPS * 64)
            say("row    %s | %8.4f us per sampled row = %6.2f x fewer than rl_learn_dueling's %.4f" % (what, per_row, base / per_row, base))
    return med


def judge(med, say):
    for n in LEARNERS:
        duel, one = med[("duel", n, 64)], med[("wide", n, 64)]
        expected = (1 + EXTRA_FORWARD) * duel + GAPS_US
        ok = abs(one - expected) <= WITHIN * expected
        say("E1     %d learner(s): one-tile wide call %.2f us, expected 1.28 x %.2f + 30 = %.2f us (measured / expected %.2f): %s%s"
            % (n, one, duel, expected, one / expected, "CONFIRMED" if ok else "REFUTED",
               "; the one-tile wide call is SLOWER than rl_learn_dueling (%.2f x)" % (one / duel) if one > duel else
               "; the one-tile wide call is not slower than rl_learn_dueling (%.2f x)" % (one / duel)))
        inside = [b for b in BATCHES if n * ((b + TILE - 1) // TILE) <= CUS]
        worst = max(med[("wide", n, b)] / one for b in inside)
        falls = all(med[("wide", n, b)] / b < med[("wide", n, a)] / a for a, b in zip(BATCHES, BATCHES[1:]))
        say("E2     %d learner(s): batches %s keep learners x tiles <= %d; the slowest of them takes %.2f x the one-tile call (<= 1.25 expected): %s; "
            "us per sampled row %s with every widening" % (n, list(inside), CUS, worst, "CONFIRMED" if worst <= 1.25 else "REFUTED",
                                                          "falls" if falls else "DOES NOT fall"))


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
            fh.write("# tools/learn_dueling_wide_time.py on ONE MI355X, one process: device events around one rl_learn_dueling (one launch) and one\n"
                     "# rl_learn_dueling_wide (6 launches: the event pair includes their host-side issue gaps), ONE step per call, 20 warm-up + >= 200\n"
                     "# repetitions per figure, full rings of 10,000 rows, slot tables drawn outside the clock (rl_learn_draw_rank).\n"
                     "# Expected BEFORE measuring (the tool's docstring has the derivation): E1 one-tile wide call = 1.28 x rl_learn_dueling + 30 us\n"
                     "# (one extra eval forward, five launch gaps of 6 us), within 25 %; E2 calls with learners x tiles <= 256 take at most 1.25 x the\n"
                     "# one-tile call, so the cost per sampled row falls by about the tile count.\n"
                     "# NOT measured: a trainer() run with learn_batch={\"D3QN\": B}, hardware counters, several GPUs.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
