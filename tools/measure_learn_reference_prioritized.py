"""What learn_reference_prioritized=True costs on one MI355X (device events and medians where the device is timed, wall clock where the
host is part of the path):

  1. rl_learn_prioritized_store_ref and rl_learn_prioritized_choice alone, at n = 64 / 1,000 / 10,000 rows and 64 draws;
  2. the same work as it would run on the host -- the alternative design: the priorities read back, numpy's `**`, sum, cumsum and
     searchsorted, the slots uploaded;
  3. trainer() on the PERD3QN fixture's configuration and seeds (tests/golden/learn_reference_perd3qn.npz), with the keyword and with
     learn=None (a lone PERD3QN brain is refused by learn="reference" without the keyword: nothing would train), per tick, and the
     three launches of one train() -- store, choice, rl_learn_prioritized -- timed one by one on the run's learner afterwards.

    python tools/measure_learn_reference_prioritized.py [reps]          (default 200)
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
import learn_reference_prioritized_cases as pc  # noqa: E402


def device_us(fn, reps):
    """Median microseconds of fn() between two events on the current stream, after 10 warm-up calls."""
    import torch
    for _ in range(10):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return float(np.median(out))


def wall_us(fn, reps):
    import torch
    for _ in range(10):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0))
    return float(np.median(out))


def kernels_alone(reps):
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds
    w = DeviceWorlds(n_worlds=1, max_agents=10, n_brains=1, seed=3)
    for n in (64, 1000, 10_000):
        c = pc.choice_case(n, 3 * n - 1)
        C_, R = c["capacity"], c["ring_rows"]
        prio = torch.as_tensor(np.nan_to_num(c["by_slot"], nan=0.5), device=w.device)
        learners, sides = (_lib.Learner * 1)(), (_lib.Prio * 1)()
        learners[0].kind, sides[0].priority, sides[0].alpha = _lib.PERD3QN, prio.data_ptr(), 0.6
        group = (_lib.PrioStore * 1)(_lib.PrioStore(C_, R, c["stored"], pc.CHOICE_SLACK))
        u = torch.as_tensor(c["u"], device=w.device)
        idx = torch.zeros(64, dtype=torch.int32, device=w.device)
        slots = torch.zeros(64, dtype=torch.int32, device=w.device)
        work = torch.empty(int(w.lib.rl_learn_prioritized_choice_work_bytes(C_)), dtype=torch.uint8, device=w.device)
        draw = (_lib.PrioChoice * 1)(_lib.PrioChoice(C_, R, c["stored"], 64, u.data_ptr(), idx.data_ptr(), slots.data_ptr(), None, work.data_ptr()))
        store = lambda: _lib.check(w.lib.rl_learn_prioritized_store_ref(w.handle, learners, sides, group, 1, w._stream()), "store")  # noqa: E731
        choice = lambda: _lib.check(w.lib.rl_learn_prioritized_choice(w.handle, learners, sides, draw, 1, w._stream()), "choice")  # noqa: E731

        def upload():   # the host's part of the device path: the uniforms
            torch.as_tensor(c["u"], device=w.device)

        live = torch.as_tensor(np.flatnonzero(~np.isnan(c["by_slot"])), device=w.device)

        def host_path():   # the alternative design: priorities to the host, numpy's choice arithmetic, slots back
            p = prio[live].cpu().numpy()
            i, _ = pc.choice_indices(p, c["u"])
            torch.as_tensor(((i + C_ * ((c["stored"] - 1 - i) // C_)) % R).astype(np.int32), device=w.device)

        print("n = %5d, 64 draws: store %.1f us, choice %.1f us (device events); uniforms' upload %.1f us, the pair with the upload %.1f us, "
              "the host path (read back %d floats, numpy, upload 64 slots) %.1f us (wall clock, synchronised)"
              % (n, device_us(store, reps), device_us(choice, reps), wall_us(upload, reps), wall_us(lambda: (upload(), store(), choice()), reps),
                 n, wall_us(host_path, reps)))
        w.check_error_flag()


def run(ticks, **kw):
    import torch
    from reinlife_amd import Environment, trainer
    g = pc.load()
    brains = pc.product_brains(g)
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
            env = trainer(brains, n_episodes=ticks - 1, width=pc.CASE["width"], height=pc.CASE["height"], max_agents=pc.CASE["max_agents"],
                          print_results=False, save=False, **kw)
    finally:
        Environment.update_env, Environment.log_reference_calls = update, False
    calls = np.zeros(ticks, np.int64)
    for n_epi, c in env.reference_calls:
        calls[n_epi] += c.kind == "learn"
    return np.diff(np.array(stamps)), calls[1:], env


def the_run(reps):
    g = pc.load()
    ticks = int(g["ticks"])
    us = lambda x: 1e6 * float(np.median(x)) if len(x) else float("nan")  # noqa: E731
    run(30)
    base, _, _ = run(ticks)
    dt, calls, env = run(ticks, learn="reference", learn_reference_prioritized=True)
    quiet, busy = dt[calls == 0], dt[calls > 0]
    print("fixture configuration, %d ticks; learn=None: median %.0f us per tick" % (ticks, us(base)))
    print("learn='reference', learn_reference_prioritized=True: median %.0f us per tick; ticks without a train(): %d, median %.0f us (capture + "
          "one store launch); ticks with train(): %d, median %.0f us, %.2f calls per such tick"
          % (us(dt), len(quiet), us(quiet), len(busy), us(busy), calls[calls > 0].mean()))
    print("  time beyond a quiet tick, per train() (store, choice, rl_learn_prioritized: three launches and one upload): median %.0f us"
          % us((busy - us(quiet) * 1e-6) / calls[calls > 0]))
    l, w, s = env.learners[0], env.worlds, env.schedule
    C_, stored = s.specs[0].capacity, s.stored[0]
    u = np.random.RandomState(1).random_sample(l.batch)
    _, slots, _ = w.choose_prioritized_reference([l], [C_], [stored], [u])
    print("  one by one on the run's learner (device events): store %.1f us, choice with its upload %.1f us, rl_learn_prioritized %.1f us"
          % (device_us(lambda: w.store_prioritized_reference([l], [C_], [stored - 1], [1]), reps),
             device_us(lambda: w.choose_prioritized_reference([l], [C_], [stored], [u]), reps),
             device_us(lambda: w.learn([l], 1, slots=slots), reps)))
    print("the reference's own loop on the generator's CPU, same seeds: median %.0f us per tick; its ticks with train(): median %.0f us"
          % (us(g["tick_seconds"]), us(g["tick_seconds"][np.unique(g["call_tick"])])))
    w.check_error_flag()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    kernels_alone(reps)
    the_run(reps)
