"""What learn_reference_td=True costs on one MI355X (device events and medians where the device is timed, wall clock where the host is
part of the path).  Expectations, written before the first run: the three tree kernels are latency-bound one-workgroup launches of a few
microseconds each beside rl_learn_td's hundreds; the store of a full slot_cap group is the longest of them (its owner search is quadratic
in the group); a tick with a train_model() costs about what PERD3QN's does (profiles/learn_reference_prioritized.txt: 322 us per train());
the host-side alternative pays two synchronising copies and loses at every size.

  1. rl_learn_td_tree_store (groups of 1 and of slack rows), rl_learn_td_tree_sample and rl_learn_td_tree_update (64 entries) alone, at
     C = 64 (the fixture's) and C = 20,000, against rl_learn_td between them on the fixture's learner;
  2. the host-side alternative: the tree kept in numpy, the 64 rewritten priorities read back, the tree updated and walked on the host,
     the 64 slots uploaded -- synchronised wall clock against the device path's;
  3. trainer() on the fixture's configuration and seeds (tests/golden/learn_reference_perdqn.npz) with the keyword and with learn=None
     (a lone PERDQN brain is refused by learn="reference" without the keyword, so the frozen run is the inference-only one), per tick.

    python tools/measure_learn_reference_td.py [reps]          (default 200)
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import learn_reference_cases as lrc  # noqa: E402
import learn_reference_td_cases as tc  # noqa: E402
from measure_learn_reference_prioritized import device_us, wall_us  # noqa: E402


def kernels_alone(reps):
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds
    w = DeviceWorlds(n_worlds=1, max_agents=10, n_brains=1, seed=3)
    for C, slack in ((64, 64), (20_000, 256)):
        R = C + slack
        model = tc.TreeModel(C, R)
        rng = np.random.RandomState(C)
        model.store(C, tc.p_new())
        for j in range(C):   # priorities over six binades, as after many train_model() calls
            model.priority[model.slot_of(j + C - 1)] = np.float32(2.0 ** rng.uniform(-3, 3))
            model.update(j + C - 1, model.priority[model.slot_of(j + C - 1)])
        tree = torch.as_tensor(model.tree, device=w.device)
        prio = torch.as_tensor(model.priority, device=w.device)
        learners, sides = (_lib.Learner * 1)(), (_lib.TdPrio * 1)()
        learners[0].kind, sides[0].priority, sides[0].p_new = _lib.PERDQN, prio.data_ptr(), float(tc.p_new())
        u_host = rng.random_sample(64)
        u = torch.as_tensor(u_host, device=w.device)
        idxs = torch.zeros(64, dtype=torch.int32, device=w.device)
        slots = torch.zeros(64, dtype=torch.int32, device=w.device)
        one = (_lib.TdTreeStore * 1)(_lib.TdTreeStore(tree.data_ptr(), C, R, C, 1))
        full = (_lib.TdTreeStore * 1)(_lib.TdTreeStore(tree.data_ptr(), C, R, C, slack))
        draw = (_lib.TdTreeSample * 1)(_lib.TdTreeSample(tree.data_ptr(), C, R, C, 64, u.data_ptr(), idxs.data_ptr(), slots.data_ptr(), None, None))
        upd = (_lib.TdTreeUpdate * 1)(_lib.TdTreeUpdate(tree.data_ptr(), C, R, 64, idxs.data_ptr(), slots.data_ptr()))
        call = lambda name, a: (lambda: _lib.check(getattr(w.lib, name)(w.handle, learners, sides, a, 1, w._stream()), name))  # noqa: E731
        sample = call("rl_learn_td_tree_sample", draw)
        sample()

        def device_path():   # per train_model(): the uniforms up, sample, update (rl_learn_td between them is common to both designs)
            torch.as_tensor(u_host, device=w.device)
            sample()
            call("rl_learn_td_tree_update", upd)()

        def host_path():   # the alternative: the tree in numpy; 64 rewritten priorities read back, the slots uploaded
            got = model.sample(u_host)
            torch.as_tensor(np.array(got["slots"], np.int32), device=w.device)
            p = prio[slots.long()].cpu().numpy()
            for i, v in zip(got["idxs"], p):
                model.update(i, v)

        print("C = %5d: store of 1 row %.1f us, of %d rows %.1f us, sample of 64 %.1f us, update of 64 %.1f us (device events); per train_model() "
              "the device path (upload, sample, update) %.1f us against the host path (numpy tree, 64 priorities read back, slots uploaded) %.1f us "
              "(wall clock, synchronised)"
              % (C, device_us(call("rl_learn_td_tree_store", one), reps), slack, device_us(call("rl_learn_td_tree_store", full), reps),
                 device_us(sample, reps), device_us(call("rl_learn_td_tree_update", upd), reps), wall_us(device_path, reps), wall_us(host_path, reps)))
        w.check_error_flag()


def run(ticks, **kw):
    import time
    import torch
    from reinlife_amd import Environment, trainer
    g = tc.load()
    brains = tc.product_brains(g)
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
            env = trainer(brains, n_episodes=ticks - 1, width=tc.CASE["width"], height=tc.CASE["height"], max_agents=tc.CASE["max_agents"],
                          print_results=False, save=False, **kw)
    finally:
        Environment.update_env, Environment.log_reference_calls = update, False
    calls = np.zeros(ticks, np.int64)
    for n_epi, c in env.reference_calls:
        calls[n_epi] += c.kind == "learn"
    return np.diff(np.array(stamps)), calls[1:], env


def the_run(reps):
    g = tc.load()
    ticks = int(g["ticks"])
    us = lambda x: 1e6 * float(np.median(x)) if len(x) else float("nan")  # noqa: E731
    run(30)
    base, _, _ = run(ticks)
    dt, calls, env = run(ticks, learn="reference", learn_reference_td=True)
    quiet, busy = dt[calls == 0], dt[calls > 0]
    print("fixture configuration, %d ticks; learn=None (the PERDQN brain frozen): median %.0f us per tick" % (ticks, us(base)))
    print("learn='reference', learn_reference_td=True: median %.0f us per tick; ticks without a train_model(): %d, median %.0f us (capture + one "
          "store launch); ticks with one: %d, median %.0f us, %.2f calls per such tick"
          % (us(dt), len(quiet), us(quiet), len(busy), us(busy), calls[calls > 0].mean()))
    print("  time beyond a quiet tick, per train_model() (store, sample, rl_learn_td, update: four launches and one upload): median %.0f us"
          % us((busy - us(quiet) * 1e-6) / calls[calls > 0]))
    l, w, s = env.learners[0], env.worlds, env.schedule
    C, stored = s.specs[0].capacity, s.stored[0]
    u = np.random.RandomState(1).random_sample(l.batch)
    idxs, slots, _ = w.sample_td_reference([l], [C], [stored], [u])
    print("  one by one on the run's learner (device events): store %.1f us, sample with its upload %.1f us, rl_learn_td %.1f us, update %.1f us"
          % (device_us(lambda: w.store_td_reference([l], [C], [stored - 1], [1]), reps),
             device_us(lambda: w.sample_td_reference([l], [C], [stored], [u]), reps),
             device_us(lambda: w.learn([l], 1, slots=slots), reps),
             device_us(lambda: w.update_td_reference([l], [C], idxs, slots), reps)))
    print("the reference's own loop on the generator's CPU, same seeds: median %.0f us per tick; its ticks with train_model(): median %.0f us"
          % (us(g["tick_seconds"]), us(g["tick_seconds"][np.unique(g["call_tick"])])))
    w.check_error_flag()


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    kernels_alone(reps)
    the_run(reps)
