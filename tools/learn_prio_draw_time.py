"""What the two prioritised minibatch draws cost on ONE MI355X, alternating in one loop of one process per case: the exponential race
(rl_learn_prioritized_wide_draw / rl_learn_td_draw through DeviceWorlds.draw_prioritized / draw_td: two launches, one workgroup per draw,
each a pass over the ring -- the yardstick, its kernels unchanged) and the prefix sum over content-key rank
(rl_learn_prioritized_draw_rank / rl_learn_td_draw_rank through DeviceWorlds.draw_prioritized_rank / draw_td_rank: eight launches, one
sort, one cumulative sum, one thread per draw).

  PERD3QN  full rings of 10,000 rows, one step of batch 64 / 256 / 1024 / 2048, 1 and 8 learners; independent draws
  PERDQN   full rings of 20,000 rows, one step of batch 64, 1 / 2 / 8 learners; stratified draws

  race   device-event time of ONE race draw call
  rank   device-event time of ONE rank draw call for the same learners and table shape; the event pair includes the eight launches'
         host-side issue gaps
  ratio  race median / rank median

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls of each; race and rank calls alternate, so both see
the same clocks.  Nothing new is stamped in the timed calls (seen == count after the first).

    python tools/learn_prio_draw_time.py [--out profiles/learn_prio_draw_rank.txt] [--reps 200]

No threshold is set: the figures are recorded.  Every case runs in a child process of its own under its own time limit, and the first
step that fails ends the run."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _report  # noqa: E402

CASES = ("prio:1", "prio:8", "td:1", "td:2", "td:8")   # memory : learners
PRIO_BATCHES = (64, 256, 1024, 2048)
PRIO_RING, TD_RING = 10_000, 20_000
STEP_SECONDS = 240


def _ring(rng, dev, n):
    import numpy as np
    import torch

    def rows():
        x = (rng.random_sample((n, 153)) < 0.15) * rng.choice(np.array([1.0, -1.0, 0.5], np.float32), size=(n, 153))
        return torch.as_tensor(x.astype(np.float32), device=dev)
    return {"state": rows(), "state_prime": rows(), "action": torch.as_tensor(rng.randint(0, 8, size=n).astype(np.int8), device=dev),
            "reward": torch.as_tensor(rng.choice(np.array([0, 0.05, 0.3, -1, 5, -10], np.float32), size=n), device=dev),
            "done": torch.as_tensor((rng.random_sample(n) < 0.2).astype(np.uint8), device=dev), "prob": None,
            "age": torch.as_tensor(rng.randint(0, 200, size=n).astype(np.int32), device=dev),
            "count": torch.full((1,), n, dtype=torch.int64, device=dev)}


def _time_both(a, b, reps):
    """reps device-event times of a() and of b(), in microseconds, the calls alternating a b a b ..."""
    import torch
    for _ in range(20):
        a(); b()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(); a(); e[1].record(); b(); e[2].record()
    torch.cuda.synchronize()
    return sorted(e[0].elapsed_time(e[1]) * 1e3 for e in ev), sorted(e[1].elapsed_time(e[2]) * 1e3 for e in ev)


def step(case, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    memory, n = case.split(":")
    td, n = memory == "td", int(n)
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rng = np.random.RandomState(1)
    size = TD_RING if td else PRIO_RING
    rings = [_ring(rng, dev, size) for _ in range(n)]
    for batch in ((64,) if td else PRIO_BATCHES):
        if td:
            ls = [DeviceLearner(Models.PERDQN(), dev, ring=r, td_priority=True) for r in rings]
        else:
            ls = [DeviceLearner(Models.PERD3QN(), dev, ring=r, prioritized=True, prioritized_batch=batch) for r in rings]
        for l in ls:   # priorities over several orders of magnitude, as a memory under way holds them
            l.priority.copy_(torch.as_tensor((rng.random_sample(size) ** 3 * 4 + 1e-3).astype(np.float32), device=dev))
            l.seen.copy_(l.ring["count"])
        race_fn, rank_fn = (dw.draw_td, dw.draw_td_rank) if td else (dw.draw_prioritized, dw.draw_prioritized_rank)
        what = "1 step x batch %d, %d learner(s), ring %d" % (batch, n, size)
        race, rank = _time_both(lambda: race_fn(ls, 1), lambda: rank_fn(ls, 1), reps)
        dw.check_error_flag()
        slots = rank_fn(ls, 1).cpu().numpy()
        for l, s in zip(ls, slots):   # the tables are what they should be: a permutation and a rising sum behind every draw
            order, cum = l.rank_order.cpu().numpy(), l.rank_cum.cpu().numpy()
            assert np.array_equal(np.sort(order), np.arange(size)) and (np.diff(cum) >= 0).all() and s.min() >= 0 and s.max() < size
        names = ("rl_learn_td_draw", "rl_learn_td_draw_rank") if td else ("rl_learn_prioritized_wide_draw", "rl_learn_prioritized_draw_rank")
        _report("race   %-30s " % names[0] + what, race, reps)
        _report("rank   %-30s " % names[1] + what, rank, reps)
        print("ratio  %s | %s / %s = %6.2f" % (what, names[0], names[1], race[reps // 2] / rank[reps // 2]), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # (a child process: one case)
    args = ap.parse_args()
    if args.step:
        step(args.step, max(args.reps, 200))
        return 0
    lines = []
    for st in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step", st]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_prio_draw_time: step %s ran into its %d s limit; stopping" % (st, STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_prio_draw_time: step %s failed (%d); stopping\n%s" % (st, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("race", "rank", "ratio"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
