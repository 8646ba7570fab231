"""What the two uniform minibatch draws cost on ONE MI355X, side by side in one process per learner count: rl_learn_draw (DeviceWorlds.
draw_slots: two launches, one workgroup per draw over all of a ring's keys -- the yardstick, its kernels unchanged) and
rl_learn_draw_rank (DeviceWorlds.draw_slots_rank: six launches, the ring's rows sorted by content key once, one thread per draw), for 1
and 8 learners on FULL rings of 50,000 rows, 5 steps x batch 32 / 256 / 1024 / 2048.

  draw   device-event time of ONE DeviceWorlds.draw_slots call
  rank   device-event time of ONE DeviceWorlds.draw_slots_rank call for the same learners and table shape; the event pair includes the six
         launches' host-side issue gaps
  ratio  draw median / rank median

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls.  The expectation the figures confirm or refute:
the rank draw's time does not move with the batch and sits near its key pass -- 61 MB read per full ring plus a handful of short launches.

    python tools/learn_draw_time.py [--out profiles/learn_draw_rank.txt] [--reps 200]

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
from learn_wide_time import BATCHES, N_STEPS, RING, _ring, _time  # noqa: E402

LEARNERS = ("1", "8")
STEP_SECONDS = 240


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
    for batch in BATCHES:
        ls = [DeviceLearner(Models.DQN(), dev, ring=r, wide_batch=batch) for r in rings]
        what = "%d steps x batch %d, %d learner(s), ring %d" % (N_STEPS, batch, n, RING)
        draw = sorted(_time(lambda: dw.draw_slots(ls, N_STEPS), reps))
        rank = sorted(_time(lambda: dw.draw_slots_rank(ls, N_STEPS), reps))
        dw.check_error_flag()
        slots = dw.draw_slots_rank(ls, N_STEPS).cpu().numpy()
        for l, s in zip(ls, slots):   # the tables are what they should be: a permutation behind every draw, every slot inside the ring
            order = l.rank_order.cpu().numpy()
            assert np.array_equal(np.sort(order), np.arange(RING)) and s.min() >= 0 and s.max() < RING
        _report("draw   rl_learn_draw      (DeviceWorlds.draw_slots),      " + what, draw, reps)
        _report("rank   rl_learn_draw_rank (DeviceWorlds.draw_slots_rank), " + what, rank, reps)
        print("ratio  %s | rl_learn_draw / rl_learn_draw_rank = %6.2f" % (what, draw[reps // 2] / rank[reps // 2]), flush=True)


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
            print("learn_draw_time: step %s ran into its %d s limit; stopping" % (st, STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_draw_time: step %s failed (%d); stopping\n%s" % (st, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("draw", "rank", "ratio"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_draw_time.py on ONE MI355X: device events around one rl_learn_draw (two launches: the yardstick, its kernels unchanged) and one\n"
                     "# rl_learn_draw_rank (six launches: the event pair includes their host-side issue gaps) in the same process, 20 warm-up + >= 200\n"
                     "# repetitions per figure, full rings of 50,000 rows.  NOT measured: a trainer() run with learn_draw, hardware counters.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
