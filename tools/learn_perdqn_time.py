"""What a PERDQN update on the device costs (rl_learn_td_draw + rl_learn_td, reinlife_amd/csrc/rl_learn_prio.hip and rl_learn_td.hip), on
an MI355X, next to the same update made of eager torch ops on the same GPU:

  td       device-event time of ONE rl_learn_td_draw (1 step x batch 64: stamp + keys of every ring row, then 64 workgroups) and of ONE
           rl_learn_td call (1 step, packer included) for N learners on FULL rings of 20,000 transitions (PERDQNAgent's capacity) --
           median, min and p90 over >= 200 repetitions after 20 warm-up pairs; N in (1, 2, 8)
  torch    PERDQNAgent.train_model() for ONE brain as eager torch ops on the same GPU: 64 rows gathered from a ring of 20,000 by
           torch.multinomial on the priorities, both forward passes, the importance weights, the loss, backward, Adam (foreach=False),
           the priority write-back and the target copy; device events around the host-issued ops

    python tools/learn_perdqn_time.py [--out profiles/learn_perdqn.txt] [--reps 200]

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

RING = 20000
STEPS = [("td", "1"), ("td", "2"), ("td", "8"), ("torch",)]
STEP_SECONDS = 150


def pair(n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ls = [DeviceLearner(Models.PERDQN(), dev, ring=_ring(torch, rng, dev, RING), td_priority=True) for _ in range(n)]
    for _ in range(20):
        dw.learn(ls, 1, slots=dw.draw_td(ls, 1))
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(); slots = dw.draw_td(ls, 1); e[1].record(); dw.learn(ls, 1, slots=slots); e[2].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    assert ls[0].state.cpu().tolist() == [20 + reps, 20 + reps]
    what = "1 step x batch 64, %d learner(s), full ring %d" % (n, RING)
    _report("td    draw   rl_learn_td_draw, %s (incl. the slots tensor's allocation)" % what, [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)
    _report("td    learn  rl_learn_td, %s" % what, [e[1].elapsed_time(e[2]) * 1e3 for e in ev], reps)


def torch_steps(reps):
    import numpy as np
    import torch
    import torch.nn.functional as F
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ring = _ring(torch, rng, dev, RING)
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8)).to(dev)  # noqa: E731
    q, tgt = mk(), mk()
    tgt.load_state_dict(q.state_dict())
    opt = torch.optim.Adam(q.parameters(), lr=0.001, foreach=False)
    act, mask = ring["action"].long(), 1.0 - ring["done"].float()
    prio = torch.full((RING,), 0.0630957335, device=dev)
    beta = [0.4]

    def call():
        beta[0] = min(1.0, beta[0] + 0.001)
        idx = torch.multinomial(prio, 64, replacement=True)
        p = prio[idx]
        w = (p / p.min()) ** -beta[0]
        s, sp, a, r, dm = ring["state"][idx], ring["state_prime"][idx], act[idx].unsqueeze(1), ring["reward"][idx], mask[idx]
        with torch.no_grad():
            target = r + dm * 0.99 * tgt(sp).max(1)[0]
        pred = q(s).gather(1, a).squeeze(1)
        prio[idx] = (torch.abs(pred.detach() - target) + 0.01) ** 0.6
        loss = (w * F.mse_loss(pred, target)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        tgt.load_state_dict(q.state_dict())
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); call(); e[1].record()
    torch.cuda.synchronize()
    _report("torch eager torch ops, draw + 1 step x batch 64 + priorities + target copy, 1 brain, ring %d (device events around the host-issued ops)" % RING,
            [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        if args.step[0] == "td":
            pair(int(args.step[1]), max(args.reps, 200))
        else:
            torch_steps(max(args.reps, 200))
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_perdqn_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_perdqn_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("td", "torch"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_perdqn_time.py on an MI355X: device events around the draw (two launches) and around the learn call (one launch,\n"
                     "# packer included), 20 warm-up + >= 200 repetitions per figure; the event pairs include the launches' host-side issue gaps\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
