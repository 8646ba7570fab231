"""What a D3QN update on the device costs (rl_learn_dueling, reinlife_amd/csrc/rl_learn_dueling.hip), on an MI355X:

  duel     device-event time of ONE rl_learn_dueling call of 1 step (batch 64) for N learners on rings of 4,096 transitions -- median,
           min and p90 over >= 200 repetitions after 20 warm-up calls (1, 2 and 8 learners)
  dqn      ONE rl_learn call (5 steps x batch 32, one DQN learner) in the same run, as the yardstick: the ratio per multiply-add is
           (duel / 12.5 M) / (dqn / 5 / 3.0 M)
  torch    the same D3QN step as eager torch ops on the same GPU (index_select the minibatch, two forwards with the batch-wide advantage
           mean, MSE, backward, torch.optim.Adam(foreach=False)), one brain, same repetitions

    python tools/learn_d3qn_time.py [--out profiles/learn_d3qn.txt] [--reps 200]

Every figure is taken in a child process of its own under its own time limit, and the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import RING, _report, _ring  # noqa: E402

STEPS = [("duel", "1"), ("duel", "2"), ("duel", "8"), ("dqn", "1"), ("torch",)]
STEP_SECONDS = 150
MACS_D3QN, MACS_DQN = 12.5e6, 3.0e6   # multiply-adds of one update (two forwards, the backward pass, the weight gradients)


def device_learn(kind, n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    duel = kind == "duel"
    ls = [DeviceLearner(Models.D3QN() if duel else Models.DQN(), dev, ring=_ring(torch, rng, dev)) for _ in range(n)]
    n_steps = ls[0].n_steps_default
    for _ in range(20):
        dw.learn(ls, n_steps)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); dw.learn(ls, n_steps); e[1].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    assert ls[0].state.cpu().tolist() == [n_steps * (20 + reps), 20 + reps]
    _report("%-6s %s, %d step(s) x batch %d, %d learner(s), ring %d" % (kind, ls[0].entry, n_steps, ls[0].batch, n, RING),
            [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def torch_step(reps):
    import numpy as np
    import torch
    import torch.nn.functional as F
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ring = _ring(torch, rng, dev)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fc, self.a1, self.a2 = torch.nn.Linear(153, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 8)
            self.v1, self.v2 = torch.nn.Linear(128, 128), torch.nn.Linear(128, 1)

        def forward(self, x):
            f = F.relu(self.fc(x))
            adv = self.a2(F.relu(self.a1(f)))
            return adv + self.v2(F.relu(self.v1(f))) - adv.mean()
    q, tgt = Net().to(dev), Net().to(dev)
    tgt.load_state_dict(q.state_dict())
    opt = torch.optim.Adam(q.parameters(), lr=1e-3, foreach=False)
    act, mask = ring["action"].long(), 1.0 - ring["done"].float()

    def call():
        idx = torch.randint(0, RING, (64,), device=dev)
        s, sp, a, r, dm = ring["state"][idx], ring["state_prime"][idx], act[idx].unsqueeze(1), ring["reward"][idx], mask[idx]
        with torch.no_grad():
            target = r + 0.99 * dm * tgt(sp).max(1)[0]
        loss = F.mse_loss(q(s).gather(1, a).squeeze(1), target)
        opt.zero_grad()
        loss.backward()
        opt.step()
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); call(); e[1].record()
    torch.cuda.synchronize()
    _report("torch  eager torch ops, 1 D3QN step x batch 64, 1 brain (device events around the host-issued ops)", [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        reps = max(args.reps, 200)
        if args.step[0] in ("duel", "dqn"):
            device_learn(args.step[0], int(args.step[1]), reps)
        else:
            torch_step(reps)
        return 0
    lines, medians = [], {}
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_d3qn_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_d3qn_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("duel", "dqn", "torch"))]
        print("\n".join(got), flush=True)
        lines += got
        for ln in got:
            medians[" ".join(step)] = float(ln.split("median")[1].split("us")[0])
    if "duel 1" in medians and "dqn 1" in medians:
        per_update_dqn = medians["dqn 1"] / 5
        lines.append("ratio  one D3QN update %.1f us against one DQN update %.1f us (a fifth of the 5-step call): per multiply-add (%.1f M against %.1f M) "
                     "the D3QN kernel takes %.2f of the DQN kernel's time" % (medians["duel 1"], per_update_dqn, MACS_D3QN / 1e6, MACS_DQN / 1e6,
                                                                            (medians["duel 1"] / MACS_D3QN) / (per_update_dqn / MACS_DQN)))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_d3qn_time.py on an MI355X: device events, 20 warm-up + >= 200 repetitions per figure (each call includes the packer and its launch)\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
