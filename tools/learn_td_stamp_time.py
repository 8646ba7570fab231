"""What rl_learn_td_stamp costs on ONE MI355X, in one process: device events around one stamp (DeviceWorlds.stamp_td: two launches, one
workgroup per learner and 64 window rows) alternating in the same loop with the PERDQN learning call it is queued in front of --
rl_learn_td_draw + rl_learn_td (DeviceWorlds.draw_td + learn: three launches, unchanged code, the yardstick).

  rings    full rings of 20,000 rows (count 60,000: they have wrapped), 1 / 2 / 8 learners
  windows  64, 1,024 and 20,000 fresh rows (seen = count - window, set again before every stamp, outside the timed pair)

  stamp  device-event time of ONE stamp call over that window
  call   device-event time of ONE draw_td + learn (one step of batch 64) behind it: the draw finds an empty window
  ratio  stamp median / call median

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up rounds; stamp and call alternate, so both see the same
clocks.  The learners train while the loop runs, so the stamp sees the parameters a run would show it: moving ones.

    python tools/learn_td_stamp_time.py [--out profiles/learn_td_stamp.txt] [--reps 200]

No threshold is set: the figures are recorded.  The comment lines at the head of an existing --out file (the expectations, written
before the run) are kept; the figures below them are replaced."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_prio_draw_time import _ring  # noqa: E402
from learn_time import _report  # noqa: E402

LEARNERS = (1, 2, 8)
WINDOWS = (64, 1024, 20_000)
RING, COUNT = 20_000, 60_000


def measure(reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rng = np.random.RandomState(1)
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    for n in LEARNERS:
        rings = [_ring(rng, dev, RING) for _ in range(n)]
        for r in rings:
            r["count"].fill_(COUNT)
        ls = [DeviceLearner(Models.PERDQN(), dev, ring=r, td_priority=True) for r in rings]
        for l in ls:
            l.priority.fill_(float(l.p_new))
            l.seen.copy_(l.ring["count"])
        for window in WINDOWS:
            def stamp():
                dw.stamp_td(ls)

            def call():
                dw.learn(ls, 1, slots=dw.draw_td(ls, 1))

            def open_window():
                for l in ls:
                    l.seen.fill_(COUNT - window)
            for _ in range(20):
                open_window(); stamp(); call()
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
            for e in ev:
                open_window(); e[0].record(); stamp(); e[1].record(); call(); e[2].record()
            torch.cuda.synchronize()
            dw.check_error_flag()
            a = sorted(e[0].elapsed_time(e[1]) * 1e3 for e in ev)
            b = sorted(e[1].elapsed_time(e[2]) * 1e3 for e in ev)
            for l in ls:   # the loop did what it times: every row of the last window is stamped, the window is closed, the learner trained
                pri = l.priority.cpu().numpy()
                assert np.isfinite(pri).all() and (pri > 0).all() and int(l.seen.item()) == COUNT and l.state.cpu().tolist()[0] > reps
                fresh = (np.arange(COUNT - window, COUNT) % RING)
                assert (pri[fresh].view(np.uint32) != np.float32(l.p_new).view(np.uint32)).all()
            what = "window %5d of ring %d, %d learner(s)" % (window, RING, n)
            _report("stamp  %-32s " % "rl_learn_td_stamp" + what, a, reps)
            _report("call   %-32s " % "rl_learn_td_draw + rl_learn_td" + what, b, reps)
            lines.append("stamp  %-32s %s | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions" % ("rl_learn_td_stamp", what, a[reps // 2], a[0], a[reps * 9 // 10], reps))
            lines.append("call   %-32s %s | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions" % ("rl_learn_td_draw + rl_learn_td", what, b[reps // 2], b[0], b[reps * 9 // 10], reps))
            say("ratio  %s | rl_learn_td_stamp / (rl_learn_td_draw + rl_learn_td) = %6.2f" % (what, a[reps // 2] / b[reps // 2]))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file, below the comment lines at its head")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    lines = measure(max(args.reps, 200))
    if args.out:
        head = []
        if os.path.exists(args.out):
            with open(args.out) as fh:
                for ln in fh:
                    if not ln.startswith("#"):
                        break
                    head.append(ln.rstrip("\n"))
        with open(args.out, "w") as fh:
            fh.write("\n".join(head + lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
