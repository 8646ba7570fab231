"""What the device painter costs (rl_render, reinlife_amd/csrc/rl_render.hip), on an MI355X:

  paint    device-event time of DeviceWorlds.render() on N synthetic worlds of 30x30 at a grid size, against `out.fill_(0)` on the SAME
           tensor -- the write bandwidth a buffer of that size reaches on this box -- alternating the two in one process; prints both
           medians and their ratio (256 worlds at grid size 8, 16 worlds at grid size 24)
  tester   wall milliseconds per iteration of tester(n_steps=200, n_worlds=256, render="device") against render="host"

    python tools/render_time.py [--out profiles/render_frames.txt] [--reps 200]

Every figure is taken in a child process of its own under its own time limit, and the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("paint", "256", "8"), ("paint", "16", "24"), ("tester", "device"), ("tester", "host")]
STEP_SECONDS = 120


def paint(n_worlds, gs, reps):
    import random
    import torch
    from reinlife_amd.Helpers.render import Visualize
    from reinlife_amd.worlds import DeviceWorlds
    dw = DeviceWorlds(n_worlds=n_worlds, width=30, height=30, max_agents=100, seed=1)
    dw.reset_synthetic(100)
    random.seed(1)
    style = Visualize(30, 30, gs).style(dw.device)
    out = dw.render(style)
    nbytes = out.numel()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(reps)]
    for _ in range(20):   # warm-up of both
        dw.render(style, out=out)
        out.fill_(0)
    torch.cuda.synchronize()
    for e in ev:          # painter and yardstick take turns
        e[0].record(); dw.render(style, out=out); e[1].record()
        e[2].record(); out.fill_(0); e[3].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    tp = sorted(e[0].elapsed_time(e[1]) * 1e3 for e in ev)
    tf = sorted(e[2].elapsed_time(e[3]) * 1e3 for e in ev)
    mp, mf = tp[reps // 2], tf[reps // 2]
    print("paint  %3d worlds 30x30 gs %2d  %10d bytes  reps %d | rl_render median %8.2f us (min %8.2f, p90 %8.2f) = %6.0f GB/s | fill_(0) median %8.2f us "
          "(min %8.2f, p90 %8.2f) = %6.0f GB/s | ratio %.2f" % (n_worlds, gs, nbytes, reps, mp, tp[0], tp[reps * 9 // 10], nbytes / mp * 1e-3, mf, tf[0],
                                                                 tf[reps * 9 // 10], nbytes / mf * 1e-3, mp / mf), flush=True)


def tester_loop(how):
    import random
    import numpy as np
    import torch
    from reinlife_amd import Models, tester
    torch.manual_seed(1); random.seed(1); np.random.seed(1)
    brains = [Models.D3QN(training=False), Models.D3QN(training=False)]
    tester(brains, n_steps=20, n_worlds=256, seed=1, render=how)   # warm-up: code objects, weights, the painter's background
    random.seed(1); np.random.seed(1)
    t0 = time.perf_counter()
    tester(brains, n_steps=200, n_worlds=256, seed=1, render=how)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("tester n_steps=200 n_worlds=256 render=%-6s | %7.3f ms per iteration (tick + world 0's frame in env.frame; wall time of the whole call, %.3f s, over 200)"
          % (how, dt / 200 * 1e3, dt), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        if args.step[0] == "paint":
            paint(int(args.step[1]), int(args.step[2]), max(args.reps, 200))
        else:
            tester_loop(args.step[1])
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("render_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("render_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("paint", "tester"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/render_time.py on an MI355X: device events, 20 warm-up + >= 200 alternating repetitions per figure\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
