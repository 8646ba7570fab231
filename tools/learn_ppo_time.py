"""What a PPO rollout on the device costs (rl_learn_rollout + rl_learn_ppo, reinlife_amd/csrc/rl_learn_ppo.hip), on an MI355X, next to the
same three epochs as eager torch operations on the same GPU, the D3QN pair on the same rings, and a trainer() loop with and without it:

  ppo      device-event time of ONE rl_learn_rollout (1 rollout x 32 rows: keys of the window's rows, then 32 workgroups) and of ONE
           rl_learn_ppo call (1 rollout, 3 epochs, packer included) for N learners on rings of R transitions of which the last 2,000 (or
           all 96) are fresh -- median, min and p90 over >= 200 repetitions after 20 warm-up pairs; N in (1, 2, 8), R in (96, 50,000)
  eager    the same three epochs (PPO.py:136-162) for ONE brain as eager torch float32 operations with torch.optim.Adam on the same GPU,
           rows already on the device, the GAE recursion on the host as the reference makes it
  d3qn     rl_learn_draw (asked for [2][32]) + rl_learn_dueling with D3QN learners on the same rings
  trainer  wall time of trainer([DQN, PPO], 200 episodes, 256 worlds, learn="device") with and without learn_rollout=True

    python tools/learn_ppo_time.py [--out profiles/learn_ppo.txt] [--reps 200]

No threshold is set: the figures are recorded.  Every figure is taken in a child process of its own under its own time limit, and the
first step that fails ends the run."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _report, _ring  # noqa: E402

STEPS = ([(kind, str(n), str(ring)) for ring in (96, 50000) for n in (1, 2, 8) for kind in ("ppo", "d3qn")]
         + [("eager", "1", "96"), ("trainer", "0", "256"), ("trainer", "1", "256")])
STEP_SECONDS = 150
KINDS = ("ppo", "d3qn", "eager", "trainer")


def _ppo_ring(torch, rng, dev, ring_size):
    r = _ring(torch, rng, dev, ring_size)
    r["prob"] = torch.as_tensor(rng.uniform(0.05, 0.5, size=ring_size).astype("float32"), device=dev)
    return r


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
    ppo = kind == "ppo"
    ls = [DeviceLearner(Models.PPO(), dev, ring=_ppo_ring(torch, rng, dev, ring_size), rollout=True) if ppo else
          DeviceLearner(Models.D3QN(), dev, ring=_ring(torch, rng, dev, ring_size)) for _ in range(n)]
    fresh = min(ring_size, 2000)

    def draw(ls, steps):
        if not ppo:
            return dw.draw_slots(ls, steps)
        for l in ls:   # every repetition sees the same window: the last `fresh` rows (a fill of one element, in stream order)
            l.seen.fill_(ring_size - fresh)
        return dw.draw_rollout(ls, steps)
    for _ in range(20):
        dw.learn(ls, 1, slots=draw(ls, 1))
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(); slots = draw(ls, 1); e[1].record(); dw.learn(ls, 1, slots=slots); e[2].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    per = 3 if ppo else 1
    assert ls[0].state.cpu().tolist() == [per * (20 + reps), 20 + reps]
    names = ("rl_learn_rollout", "rl_learn_ppo") if ppo else ("rl_learn_draw", "rl_learn_dueling")
    what = ("1 rollout x 32 rows x 3 epochs, %d learner(s), ring %d (%d fresh)" % (n, ring_size, fresh)) if ppo else \
        "1 step x batch 64, %d learner(s), ring %d" % (n, ring_size)
    _report("%-5s draw   %s, %s" % (kind, names[0], what), [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)
    _report("%-5s learn  %s, %s" % (kind, names[1], what), [e[1].elapsed_time(e[2]) * 1e3 for e in ev], reps)


def eager(reps):
    """PPO.py:136-162 as eager torch operations on the GPU, one brain, 32 rows."""
    import numpy as np
    import torch
    import torch.nn.functional as F
    from reinlife_amd import Models
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    net = Models.PPO().model.to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.0005)
    ring = _ppo_ring(torch, rng, dev, 96)
    idx = torch.as_tensor(rng.randint(0, 96, size=32), device=dev)
    s, sp, a = ring["state"][idx], ring["state_prime"][idx], ring["action"][idx].long().unsqueeze(1)
    r, mask, pa = (ring["reward"][idx] / 100.0).unsqueeze(1), (1.0 - ring["done"][idx].float()).unsqueeze(1), ring["prob"][idx].unsqueeze(1)
    trunk = lambda x: F.relu(net.fc2(F.relu(net.fc1(x))))  # noqa: E731

    def learn():
        for _ in range(3):
            td = r + 0.98 * net.fc_v(trunk(sp)) * mask
            h = trunk(s)
            v = net.fc_v(h)
            delta = (td - v).detach().cpu().numpy()
            adv, out = np.float32(0.0), []
            for d in delta[::-1]:
                adv = np.float32(0.98 * 0.95) * adv + d[0]
                out.append([adv])
            out.reverse()
            adv = torch.tensor(out, dtype=torch.float, device=dev)
            ratio = torch.exp(torch.log(torch.softmax(net.fc_pi(h), dim=1).gather(1, a)) - torch.log(pa))
            loss = -torch.min(ratio * adv, torch.clamp(ratio, 0.9, 1.1) * adv) + F.smooth_l1_loss(v, td.detach())
            opt.zero_grad()
            loss.mean().backward()
            opt.step()
    for _ in range(20):
        learn()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); learn(); e[1].record()
    torch.cuda.synchronize()
    _report("eager learn  torch float32 ops + torch.optim.Adam, 1 rollout x 32 rows x 3 epochs, 1 brain (a host round trip per epoch for the GAE)",
            [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def loop(with_rollout, n_worlds):
    import warnings
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(1)
    kw = {"learn_rollout": True} if with_rollout else {}
    for n_epi in (40, 200):   # (the first, short run loads the library and the kernels)
        brains = [Models.DQN(max_epi=200), Models.PPO()]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            env = trainer(brains, n_episodes=n_epi, n_worlds=n_worlds, synthetic_agents=100, refill_below=70, update_interval=100, learn="device",
                          save=False, print_results=False, **kw)
            wall = time.perf_counter() - t0
    st = env.learners[1].state.cpu().tolist() if with_rollout else None
    print("trainer %s learn_rollout: trainer([DQN, PPO], 200 episodes, %d worlds, learn='device'): loop %.1f ms (%.1f us per episode), call %.1f ms; PPO learner state %s"
          % ("with   " if with_rollout else "without", n_worlds, env.loop_seconds * 1e3, env.loop_seconds * 1e6 / 201, wall * 1e3, st))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        kind, n, size = args.step[0], int(args.step[1]), int(args.step[2])
        if kind == "eager":
            eager(max(args.reps, 200))
        elif kind == "trainer":
            loop(bool(n), size)
        else:
            pair(kind, n, size, max(args.reps, 200))
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_ppo_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_ppo_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(KINDS)]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_ppo_time.py on an MI355X: device events around the draw (two launches) and around the learn call (one launch,\n"
                     "# packer included), 20 warm-up + >= 200 repetitions per figure; the event pairs include the launches' host-side issue gaps\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
