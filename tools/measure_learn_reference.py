"""Per-tick wall time of trainer(learn="reference") on the DQN fixture's configuration (tests/golden/learn_reference_dqn.npz: two
Models.DQN brains, 30 x 30, max_agents 100, the fixture's seeds), split into ticks with and without train() calls, beside the same loop
with learn=None.  The device is synchronised at the end of every tick, so a tick's time includes its learning launches.

    python tools/measure_learn_reference.py [ticks]          (default 700: the gate of 1000 rows opens around tick 320)
"""
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import learn_reference_cases as lrc  # noqa: E402


def run(learn, ticks):
    import torch
    from reinlife_amd import Environment, trainer
    g = lrc.load("dqn")
    case = lrc.CASES["dqn"]
    brains = lrc.product_brains("dqn", g)
    stamps = []
    update = Environment.update_env

    def timed(env, n_epi=0):
        r = update(env, n_epi)
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        return r

    Environment.update_env, Environment.log_reference_calls = timed, True
    try:
        lrc.seed_all(int(g["seed"]))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            env = trainer(brains, n_episodes=ticks - 1, width=case["width"], height=case["height"], max_agents=case["max_agents"],
                          print_results=False, save=False, learn=learn)
    finally:
        Environment.update_env, Environment.log_reference_calls = update, False
    dt = np.diff(np.array(stamps))            # tick t's time for t >= 1
    calls = np.zeros(ticks, np.int64)
    for n_epi, c in env.reference_calls:
        calls[n_epi] += c.kind != "sync"
    return dt, calls[1:], env


def main():
    ticks = int(sys.argv[1]) if len(sys.argv) > 1 else 700
    run(None, 50)                             # warm-up: library load, first launches
    base, _, _ = run(None, ticks)
    dt, calls, env = run("reference", ticks)
    us = lambda x: 1e6 * float(np.median(x)) if len(x) else float("nan")  # noqa: E731
    print("ticks %d; learn=None: median %.0f us per tick (mean %.0f)" % (ticks, us(base), 1e6 * base.mean()))
    print("learn='reference': median %.0f us per tick over all ticks (mean %.0f)" % (us(dt), 1e6 * dt.mean()))
    quiet, busy = dt[calls == 0], dt[calls > 0]
    print("  ticks without a train() call: %d, median %.0f us (mean %.0f)" % (len(quiet), us(quiet), 1e6 * quiet.mean() if len(quiet) else float("nan")))
    print("  ticks with train() calls:     %d, median %.0f us (mean %.0f), %.2f calls per such tick, at most %d"
          % (len(busy), us(busy), 1e6 * busy.mean() if len(busy) else float("nan"), calls[calls > 0].mean() if len(busy) else 0, calls.max()))
    if len(busy):
        per_call = (busy - us(quiet) * 1e-6) / calls[calls > 0]
        print("  time beyond a quiet tick, per train() call (five Adam steps, one launch): median %.0f us" % us(per_call))
    g = lrc.load("dqn")
    print("the reference's own loop on the generator's CPU, same seeds: median %.0f us per tick over the fixture's %d ticks; its ticks with "
          "train() calls: median %.0f us" % (us(g["tick_seconds"]), int(g["ticks"]),
                                            us(g["tick_seconds"][np.unique(g["call_tick"])])))
    print("Adam steps per learner:", {k: int(l.state[0].item()) for k, l in env.learners.items()})


if __name__ == "__main__":
    main()
