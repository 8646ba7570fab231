"""What a prioritised PERD3QN update on the device costs (rl_learn_prioritized_draw + rl_learn_prioritized, reinlife_amd/csrc/rl_learn_prio.hip
and rl_learn_dueling.hip), on an MI355X, next to the D3QN pair on the same rings in the same run:

  prio     device-event time of ONE rl_learn_prioritized_draw (1 step x batch 64: stamp + weights + keys of every ring row, then 64
           workgroups) and of ONE rl_learn_prioritized call (1 step) for N learners on rings of R transitions -- median, min and p90
           over >= 200 repetitions after 20 warm-up pairs; N in (1, 2, 8), R in (96, 10,000)
  d3qn     the same for rl_learn_draw (asked for [2][32]) + rl_learn_dueling with D3QN learners on the same rings

    python tools/learn_perd3qn_time.py [--out profiles/learn_perd3qn.txt] [--reps 200]

No threshold is set: the figures are recorded.  Every figure is taken in a child process of its own under its own time limit, and the
first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _report, _ring  # noqa: E402

STEPS = [(kind, str(n), str(ring)) for ring in (96, 10000) for n in (1, 2, 8) for kind in ("prio", "d3qn")]
STEP_SECONDS = 150


def pair(kind, n, ring_size, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    prio = kind == "prio"
    ls = [DeviceLearner(Models.PERD3QN(), dev, ring=_ring(torch, rng, dev, ring_size), prioritized=True) if prio else
          DeviceLearner(Models.D3QN(), dev, ring=_ring(torch, rng, dev, ring_size)) for _ in range(n)]
    draw = dw.draw_prioritized if prio else dw.draw_slots
    for _ in range(20):
        dw.learn(ls, 1, slots=draw(ls, 1))
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(); slots = draw(ls, 1); e[1].record(); dw.learn(ls, 1, slots=slots); e[2].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    assert ls[0].state.cpu().tolist() == [20 + reps, 20 + reps]
    names = ("rl_learn_prioritized_draw", "rl_learn_prioritized") if prio else ("rl_learn_draw", "rl_learn_dueling")
    what = "1 step x batch 64, %d learner(s), ring %d" % (n, ring_size)
    _report("%-5s draw   %s, %s" % (kind, names[0], what), [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)
    _report("%-5s learn  %s, %s" % (kind, names[1], what), [e[1].elapsed_time(e[2]) * 1e3 for e in ev], reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        pair(args.step[0], int(args.step[1]), int(args.step[2]), max(args.reps, 200))
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_perd3qn_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_perd3qn_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("prio", "d3qn"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_perd3qn_time.py on an MI355X: device events around the draw (two launches) and around the learn call (one launch,\n"
                     "# packer included), 20 warm-up + >= 200 repetitions per figure; the event pairs include the launches' host-side issue gaps\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
