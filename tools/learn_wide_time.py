"""What a wide DQN minibatch costs on ONE MI355X (rl_learn_wide, reinlife_amd/csrc/rl_learn_wide.hip) next to rl_learn, and what the
content-key draw in front of either costs (rl_learn_draw, never measured before), for 1, 2 and 8 learners on FULL rings of 50,000 rows:

  learn   device-event time of ONE rl_learn call: 5 steps x batch 32, one launch, one workgroup per learner -- the baseline
  wide    device-event time of ONE rl_learn_wide call: 5 steps x batch 32 / 256 / 1024 / 2048, 2 x 5 + 3 = 13 launches, one workgroup per
          (learner, 32-row tile); the event pair includes the launches' host-side issue gaps
  draw    device-event time of ONE DeviceWorlds.draw_slots (rl_learn_draw: two launches, one workgroup per draw over the ring's keys) for
          the same 5 x batch tables

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls; the slot tables of the learn / wide figures are
drawn once, outside the clock.  The line to read is "us per sampled row": the call's median over 5 x batch rows.

    python tools/learn_wide_time.py [--out profiles/learn_wide.txt] [--reps 200]

No threshold is set: the figures are recorded.  Every learner count runs in a child process of its own under its own time limit, and
the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _report  # noqa: E402

LEARNERS = ("1", "2", "8")
BATCHES = (32, 256, 1024, 2048)
RING, N_STEPS = 50_000, 5
STEP_SECONDS = 240


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
    return [e[0].elapsed_time(e[1]) * 1e3 for e in ev]


def step(n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rng = np.random.RandomState(1)
    rings = [_ring(rng, dev) for _ in range(n)]
    base = None
    for entry, batch in [("rl_learn", 32)] + [("rl_learn_wide", b) for b in BATCHES]:
        wide = {"wide_batch": batch} if entry == "rl_learn_wide" else {}
        ls = [DeviceLearner(Models.DQN(), dev, ring=r, **wide) for r in rings]
        slots = dw.draw_slots(ls, N_STEPS)
        torch.cuda.synchronize()
        t = sorted(_time(lambda: dw.learn(ls, N_STEPS, slots=slots), reps))
        dw.check_error_flag()
        assert all(l.state.cpu().tolist() == [N_STEPS * (20 + reps), 20 + reps] for l in ls)
        what = "%s, %d steps x batch %d, %d learner(s), ring %d" % (entry, N_STEPS, batch, n, RING)
        _report(("learn  " if entry == "rl_learn" else "wide   ") + what, t, reps)
        per_row = t[reps // 2] / (N_STEPS * batch)
        base = per_row if entry == "rl_learn" else base
        print("row    %s | %8.4f us per sampled row = %6.2f x fewer than rl_learn's %.4f" % (what, per_row, base / per_row, base), flush=True)
        if entry == "rl_learn_wide":
            _report("draw   rl_learn_draw (DeviceWorlds.draw_slots), %d steps x batch %d, %d learner(s), ring %d" % (N_STEPS, batch, n, RING),
                    _time(lambda: dw.draw_slots(ls, N_STEPS), reps), reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # (a child process: one learner count)
    args = ap.parse_args()
    if args.step:
        step(int(args.step), max(args.reps, 200))
        return 0
    lines = []
    for st in LEARNERS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step", st]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_wide_time: step %s ran into its %d s limit; stopping" % (st, STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_wide_time: step %s failed (%d); stopping\n%s" % (st, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("learn", "wide", "row", "draw"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_wide_time.py on ONE MI355X: device events around one rl_learn (one launch), one rl_learn_wide (13 launches: the event pair\n"
                     "# includes their host-side issue gaps) and one rl_learn_draw (two launches), 20 warm-up + >= 200 repetitions per figure, full rings of\n"
                     "# 50,000 rows, slot tables drawn outside the clock.  NOT measured: a trainer() run with learn_batch, the 8-rank all-gather.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
