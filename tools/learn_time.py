"""What learning on the device costs (rl_learn, reinlife_amd/csrc/rl_learn.hip), on an MI355X:

  learn    device-event time of ONE rl_learn call of 5 steps (batch 32) for N learners on rings of 4,096 transitions -- median, min and
           p90 over >= 200 repetitions after 20 warm-up calls (1, 2 and 8 learners)
  draw     device-event time of ONE rl_learn_draw call (5 x 32 draws by content key; two launches) on a FULL ring of 50,000 transitions,
           1 and 2 learners -- what Environment queues in front of every rl_learn
  torch    the same five steps as eager torch ops on the same GPU (index_select the minibatch, two forwards, smooth-L1, backward,
           torch.optim.Adam(foreach=False)), one brain, same repetitions
  trainer  wall seconds of the loop of trainer(n_worlds=256, n_episodes=2000, synthetic_agents=100, refill_below=70) with two DQN brains,
           learn="device" against learn=None (env.loop_seconds, after a 100-episode warm-up run)

    python tools/learn_time.py [--out profiles/learn_dqn.txt] [--reps 200]

Every figure is taken in a child process of its own under its own time limit, and the first step that fails ends the run."""
import argparse
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("learn", "1"), ("learn", "2"), ("learn", "8"), ("draw", "1"), ("draw", "2"), ("torch",), ("trainer", "device"), ("trainer", "none")]
STEP_SECONDS = 150
RING = 4096


def _ring(torch, rng, dev, RING=RING):
    import numpy as np
    x = lambda: torch.as_tensor((rng.random_sample((RING, 153)) < 0.15).astype(np.float32), device=dev)  # noqa: E731
    return {"state": x(), "state_prime": x(), "action": torch.as_tensor(rng.randint(0, 8, size=RING).astype(np.int8), device=dev),
            "reward": torch.as_tensor(rng.choice([0.0, 0.05, 0.3, -1.0, 5.0, -10.0], size=RING).astype(np.float32), device=dev),
            "done": torch.as_tensor((rng.random_sample(RING) < 0.2).astype(np.uint8), device=dev), "prob": None,
            "age": torch.zeros(RING, dtype=torch.int32, device=dev), "count": torch.full((1,), RING, dtype=torch.int64, device=dev)}


def _report(name, times, reps):
    t = sorted(times)
    print("%s | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions" % (name, t[reps // 2], t[0], t[reps * 9 // 10], reps), flush=True)


def learn(n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ls = [DeviceLearner(Models.DQN(), dev, ring=_ring(torch, rng, dev)) for _ in range(n)]
    for _ in range(20):
        dw.learn(ls, 5)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); dw.learn(ls, 5); e[1].record()
    torch.cuda.synchronize()
    dw.check_error_flag()
    assert ls[0].state.cpu().tolist() == [5 * (20 + reps), 20 + reps]
    _report("learn  rl_learn, 5 steps x batch 32, %d learner(s), ring %d" % (n, RING), [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def draw(n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import BUFFER_LIMIT, DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ls = [DeviceLearner(Models.DQN(), dev, ring=_ring(torch, rng, dev, BUFFER_LIMIT)) for _ in range(n)]
    for _ in range(20):
        dw.draw_slots(ls, 5)
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
    for e in ev:
        e[0].record(); slots = dw.draw_slots(ls, 5); e[1].record()
    torch.cuda.synchronize()
    assert 0 <= int(slots.min()) and int(slots.max()) < BUFFER_LIMIT
    _report("draw   rl_learn_draw, 5 x 32 draws, %d learner(s), full ring %d (incl. the slots tensor's allocation)" % (n, BUFFER_LIMIT), [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def torch_steps(reps):
    import numpy as np
    import torch
    import torch.nn.functional as F
    dev = "cuda:0"
    rng = np.random.RandomState(1)
    torch.manual_seed(1)
    ring = _ring(torch, rng, dev)
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(153, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8)).to(dev)  # noqa: E731
    q, tgt = mk(), mk()
    tgt.load_state_dict(q.state_dict())
    opt = torch.optim.Adam(q.parameters(), lr=0.0005, foreach=False)
    act, mask = ring["action"].long(), 1.0 - ring["done"].float()

    def call():
        for _ in range(5):
            idx = torch.randint(0, RING, (32,), device=dev)
            s, sp, a, r, dm = ring["state"][idx], ring["state_prime"][idx], act[idx].unsqueeze(1), ring["reward"][idx].unsqueeze(1), mask[idx].unsqueeze(1)
            with torch.no_grad():
                target = r + 0.98 * tgt(sp).max(1)[0].unsqueeze(1) * dm
            loss = F.smooth_l1_loss(q(s).gather(1, a), target)
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
    _report("torch  eager torch ops, 5 steps x batch 32 + target copy, 1 brain (device events around the host-issued ops)", [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def trainer_loop(how):
    import torch
    from reinlife_amd import Models, trainer
    learn_arg = "device" if how == "device" else None
    kw = dict(n_worlds=256, synthetic_agents=100, refill_below=70, seed=1, learn=learn_arg, save=False, print_results=False)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.manual_seed(1)
        trainer([Models.DQN(max_epi=100), Models.DQN(max_epi=100)], n_episodes=100, **kw)   # warm-up: code objects, pinned buffers
        torch.manual_seed(1)
        env = trainer([Models.DQN(max_epi=2000), Models.DQN(max_epi=2000)], n_episodes=2000, **kw)
    steps = [l.steps for l in env.learners.values()]
    print("trainer n_worlds=256 n_episodes=2000 two DQN brains learn=%-6s | loop %7.3f s = %7.1f us per tick, %d launches, Adam steps per brain %s"
          % (learn_arg, env.loop_seconds, env.loop_seconds / 2001 * 1e6, env.worlds.launches, steps), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one step)
    args = ap.parse_args()
    if args.step:
        reps = max(args.reps, 200)
        if args.step[0] == "learn":
            learn(int(args.step[1]), reps)
        elif args.step[0] == "draw":
            draw(int(args.step[1]), reps)
        elif args.step[0] == "torch":
            torch_steps(reps)
        else:
            trainer_loop(args.step[1])
        return 0
    lines = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(step)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_time: step %s ran into its %d s limit; stopping" % (" ".join(step), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_time: step %s failed (%d); stopping\n%s" % (" ".join(step), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("learn", "draw", "torch", "trainer"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_time.py on an MI355X: device events, 20 warm-up + >= 200 repetitions per figure; trainer: wall time of the loop\n" + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
