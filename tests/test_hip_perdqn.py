"""GPU: the PERDQN brain (ReinLife/Models/PERDQN.py, 153 -> 64 -> 64 -> 8) through its HIP tile (policy_pair_perdqn in k_policy_pair).

Fixtures: tests/golden/perdqn.npz and tests/golden/e2e_perdqn_mixed.npz, recorded from the real reference by tools/gen_golden_perdqn.py.
  * the three shipped checkpoints against the reference's torch outputs (|dq| <= 1e-5 * max(1, max|q| of the row), same first argmax);
  * >= 1e5 live observation rows of running worlds: per weight set no worse than 2x a torch-f32 nn.Sequential against a float64 forward;
  * ragged row counts, a mixed-kind rl_policy_act launch, the whole reference loop from seeds, the README's five-brain tester() call,
    trainer() through the two-launch fallback, and the Saver round trip.
"""
import copy
import ctypes as C
import glob
import json
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

import golden_io as gio

pytestmark = pytest.mark.gpu
PERDQN = 4
FIX = os.path.join(gio.GOLDEN_DIR, "perdqn.npz")
KEYS = [("fc.0.weight", (64, 153)), ("fc.0.bias", (64,)), ("fc.2.weight", (64, 64)), ("fc.2.bias", (64,)), ("fc.4.weight", (8, 64)),
        ("fc.4.bias", (8,))]


def _fix():
    d = np.load(FIX)
    return d, json.loads(bytes(d["meta"]).decode())


def _sd_of(flat):
    sd, off = OrderedDict(), 0
    for k, shape in KEYS:
        n = int(np.prod(shape))
        sd[k] = torch.from_numpy(np.asarray(flat[off:off + n], np.float32).reshape(shape).copy())
        off += n
    assert off == len(flat)
    return sd


def _set_flat(net, flat):
    sd, o = OrderedDict(), 0
    for k, v in net.state_dict().items():
        n = v.numel()
        sd[k] = torch.from_numpy(np.asarray(flat[o:o + n], np.float32).reshape(tuple(v.shape)).copy())
        o += n
    assert o == len(flat)
    net.load_state_dict(sd)


def _weight_sets():
    """name -> flat state dict: the three checkpoints and two freshly initialised nets."""
    from reinlife_amd.Models import PERDQN as P
    d, meta = _fix()
    sets = {name: d["ckpt_%s_weights" % name] for name in meta["ckpt"]}
    for s in (5, 6):
        torch.manual_seed(s)
        sets["fresh_%d" % s] = P().state_dict_flat()
    return sets


def _forward(flat, obs_dev):
    from reinlife_amd.worlds import pack_brain_weights, policy_forward
    return policy_forward(PERDQN, pack_brain_weights(PERDQN, flat), obs_dev)


def _f64(flat, x):
    sd = {k: v.numpy().astype(np.float64) for k, v in _sd_of(flat).items()}
    h = np.maximum(x.astype(np.float64) @ sd["fc.0.weight"].T + sd["fc.0.bias"], 0.0)
    h = np.maximum(h @ sd["fc.2.weight"].T + sd["fc.2.bias"], 0.0)
    return h @ sd["fc.4.weight"].T + sd["fc.4.bias"]


def _torch_f32(flat, x):
    net = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8))
    net.load_state_dict({"%d.%s" % (int(k.split(".")[1]), k.split(".")[2]): v for k, v in _sd_of(flat).items()})
    with torch.no_grad():
        return net(torch.from_numpy(np.ascontiguousarray(x, np.float32))).numpy()


def _scaled_err(q, ref):
    return np.abs(q.astype(np.float64) - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))


def test_checkpoints_match_the_reference_outputs():
    """The three shipped PERDQN checkpoints on the 96 fixture rows: |dq| <= 1e-5 * max(1, max|q| of the row), the same first argmax."""
    d, meta = _fix()
    obs = torch.as_tensor(d["obs"], device="cuda:0")
    for name in meta["ckpt"]:
        want = d["ckpt_%s_out" % name].astype(np.float64)
        got = _forward(d["ckpt_%s_weights" % name], obs).cpu().numpy()
        err = _scaled_err(got, want)
        print("%s: max scaled |dq| %.3g (bound 1e-5), max |q| %.1f" % (name, err.max(), np.abs(want).max()))
        assert err.max() <= 1e-5, name
        assert np.array_equal(got.argmax(axis=1), want.argmax(axis=1)), name


def _live_rows(min_rows=100_000):
    """Observation rows of running worlds: 256 synthetic worlds driven by two PERDQN brains through the two-launch loop."""
    from reinlife_amd.Models import PERDQN as P
    from reinlife_amd.worlds import DeviceWorlds
    torch.manual_seed(9)
    dw = DeviceWorlds(n_worlds=256, n_brains=2, max_agents=100, seed=17)
    brains = [P(training=False), P()]
    dw.set_brains([(PERDQN, b.epsilon, b.packed_weights()) for b in brains])
    dw.reset_synthetic(100)
    rows = []
    total = 0
    while total < min_rows:
        obs, n = dw.obs_state().cpu().numpy(), dw.s["n_agents"].cpu().numpy()
        live = np.arange(dw.cap)[None, :] < n[:, None]
        rows.append(obs[live])
        total += rows[-1].shape[0]
        dw.run(3, threshold=30, n_agents=100)
    assert not dw.run_supported()
    return np.concatenate(rows)


def test_live_rows_are_no_worse_than_torch_f32():
    """>= 1e5 rows of running worlds through each checkpoint and two fresh nets, against a float64 forward: the largest scaled error
    (|dq| / max(1, max|q| of the row)) is at most 2x that of a torch-f32 nn.Sequential with the same weights on the same rows; the first
    argmax equals the float64 one wherever the scaled top-2 gap is >= 1e-5, and rows below that gap may differ in at most 1e-3 of all rows."""
    x = _live_rows()
    assert x.shape[0] >= 100_000
    pad = torch.zeros((x.shape[0] + 1, 153), dtype=torch.float32, device="cuda:0")
    pad[:x.shape[0]] = torch.from_numpy(x)
    for name, flat in _weight_sets().items():
        ref = _f64(flat, x)
        got = _forward(flat, pad[:x.shape[0]]).cpu().numpy()
        e_hip, e_torch = _scaled_err(got, ref).max(), _scaled_err(_torch_f32(flat, x), ref).max()
        srt = np.sort(ref, axis=1)
        gap = (srt[:, -1] - srt[:, -2]) / np.maximum(1.0, np.abs(ref).max(axis=1))
        differ = got.argmax(axis=1) != ref.argmax(axis=1)
        print("%s: %d rows, max scaled err hip %.3g torch-f32 %.3g (ratio %.2f), argmax differs on %d rows (%d with gap >= 1e-5)"
              % (name, x.shape[0], e_hip, e_torch, e_hip / e_torch, int(differ.sum()), int((differ & (gap >= 1e-5)).sum())))
        assert e_hip <= 2.0 * e_torch, name
        assert not (differ & (gap >= 1e-5)).any(), name
        assert differ.sum() <= 1e-3 * x.shape[0], name


def test_ragged_row_counts_give_the_bits_of_a_larger_launch():
    d, meta = _fix()
    rng = np.random.RandomState(4)
    big = np.concatenate([d["obs"]] * 50)[rng.permutation(4800)][:4200]
    dev = torch.as_tensor(big, device="cuda:0")
    flat = d["ckpt_all_gene_2_weights"]
    full = _forward(flat, dev).cpu().numpy()
    for n in (1, 31, 32, 33, 4097):
        own = torch.zeros((n + 1, 153), dtype=torch.float32, device="cuda:0")
        own[:n] = dev[:n]
        got = _forward(flat, own[:n]).cpu().numpy()
        assert np.array_equal(got, full[:n]), n


def test_mixed_kind_launch():
    """One rl_policy_act over 256 worlds with brains [PERDQN eps 0, PERDQN eps 1, DQN, PPO, PERD3QN]."""
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights, policy_forward
    d, _ = _fix()
    p = np.load(gio.GOLDEN_DIR + "/pretrained.npz")
    pk = {"PERDQN0": pack_brain_weights(PERDQN, d["ckpt_all_gene_2_weights"]), "PERDQN1": pack_brain_weights(PERDQN, d["ckpt_perdqn_gene_1_weights"]),
          "DQN": pack_brain_weights(_lib.DQN, p["DQN_weights"]), "PPO": pack_brain_weights(_lib.PPO, p["PPO_weights"]),
          "PERD3QN": pack_brain_weights(_lib.PERD3QN, p["PERD3QN_weights"])}
    others = [(_lib.DQN, 0.3, pk["DQN"]), (_lib.PPO, 0.0, pk["PPO"]), (_lib.PERD3QN, 0.2, pk["PERD3QN"])]
    dw = DeviceWorlds(n_worlds=256, n_brains=5, max_agents=100, seed=23)
    dw.reset_synthetic(100)
    dw.tick(np.random.RandomState(1).randint(0, 8, size=(256, dw.cap)).astype(np.int8))   # (tick 1: draws keyed by a non-zero tick)
    dw.set_brains([(PERDQN, 0.0, pk["PERDQN0"]), (PERDQN, 1.0, pk["PERDQN1"])] + others)
    dw.act(want_q=True)
    act, q = dw.actions.cpu().numpy().copy(), dw.out_q.cpu().numpy().copy()
    dw.set_brains([(_lib.DQN, 0.0, pk["DQN"]), (_lib.DQN, 1.0, pk["DQN"])] + others)
    dw.act(want_q=True)
    act2, q2 = dw.actions.cpu().numpy(), dw.out_q.cpu().numpy()
    n, brain = dw.s["n_agents"].cpu().numpy(), dw.s["a_brain"].cpu().numpy()
    tick, epoch = dw.s["tick"].cpu().numpy(), dw.s["epoch"].cpu().numpy()
    obs = dw.obs_state()
    live = np.arange(dw.cap)[None, :] < n[:, None]
    for b in range(5):
        assert (live & (brain == b)).sum() > 100, b
    # PERDQN eps 0: the first argmax of its own rl_policy_forward outputs, bit for bit
    ws, ks = np.nonzero(live & (brain == 0))
    rows = obs[torch.as_tensor(ws, device=obs.device), torch.as_tensor(ks, device=obs.device)].contiguous()
    pad = torch.zeros((rows.shape[0] + 1, 153), dtype=torch.float32, device=obs.device)
    pad[:rows.shape[0]] = rows
    fwd = policy_forward(PERDQN, pk["PERDQN0"], pad[:rows.shape[0]]).cpu().numpy()
    assert np.array_equal(q[ws, ks], fwd)
    assert np.array_equal(act[ws, ks], fwd.argmax(axis=1))
    # PERDQN eps 1: every action is the Philox draw's
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    ws, ks = np.nonzero(live & (brain == 1))
    for w, k in zip(ws, ks):
        lib.rl_philox(dw.cfg.seed, int(epoch[w]), int(w), int(tick[w]), 5, int(k), C.byref(out))
        assert act[w, k] == out[1] >> 29, (w, k)
    # the other kinds: bit-identical to the launch in which the PERDQN brains are DQN brains with the same epsilon
    m = live & (brain >= 2)
    assert np.array_equal(act[m], act2[m]) and np.array_equal(q[m], q2[m])


def _e2e_brains(tr):
    from reinlife_amd import Models
    kinds = [int(k) for k in tr["kinds"]]
    assert kinds == [PERDQN, PERDQN, 2]
    brains = []
    for idx, (kind, training) in enumerate(zip(kinds, tr["training"])):
        if kind == PERDQN:
            b = Models.PERDQN(training=bool(training))
            _set_flat(b.model, tr["weights_%d" % idx])
        else:
            b = Models.PERD3QN(training=bool(training))
            _set_flat(b.eval_net, tr["weights_%d" % idx])
            _set_flat(b.target_net, tr["weights_%d" % idx])
        b.invalidate()
        brains.append(b)
    return brains


@pytest.mark.parametrize("batched", [False, True])
def test_whole_loop_from_seeds_matches_reference(batched):
    """e2e_perdqn_mixed: the reference's trainer loop body without learn() with [PERDQN greedy, PERDQN exploring, PERD3QN exploring],
    reproduced action for action and world for world (Environment with rng='reference', as tests/test_hip_e2e_seeds.py)."""
    from reinlife_amd import Environment
    name = "e2e_perdqn_mixed"
    tr = np.load(os.path.join(gio.GOLDEN_DIR, name + ".npz"))
    cfg, ticks = gio.trace_cfg(tr)
    brains = _e2e_brains(tr)
    seed = int(tr["seed"])
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)
    env = Environment(width=cfg["width"], height=cfg["height"], brains=brains, max_agents=cfg["max_agents"],
                      static_families=cfg["static_families"], training=False, print_results=False, n_worlds=1, rng="reference")
    env.reset()
    for t in range(ticks):
        n0 = int(tr["n0"][t])
        assert len(env.agents) == n0
        if batched:
            env.act(t)
        else:
            for agent in env.agents:
                agent.get_action(t)
        gio._eq("%s tick %d" % (name, t), "actions", [a.action for a in env.agents], tr["actions"][t][:n0])
        env.step()
        n1 = int(tr["step_n"][t])
        tag = "%s tick %d step" % (name, t)
        gio.check_world(tag, env.worlds.world(0), tr, "step", t, True)
        gio._cmp_obs(tag + " reward", [a.reward for a in env.agents], tr["step_reward"][t][:n1], True)
        env.update_env(t)
        gio.check_world("%s tick %d update" % (name, t), env.worlds.world(0), tr, "upd", t, cfg["static_families"])


def _pretrained_all(tmp_path):
    """The reference README's five pretrained/All brains (genes 0-4), rebuilt as .pt files from the fixtures and loaded with load_model=."""
    from reinlife_amd import Models
    p = np.load(gio.GOLDEN_DIR + "/pretrained.npz")
    meta = json.loads(bytes(p["meta"]).decode())
    d, _ = _fix()
    files = {}
    for name in ("DQN", "D3QN", "PERD3QN", "PPO"):
        sd, o = OrderedDict(), 0
        for key, shape in meta[name]["keys"]:
            k = int(np.prod(shape))
            sd[key] = torch.from_numpy(p[name + "_weights"][o:o + k].reshape(shape).copy())
            o += k
        files[name] = str(tmp_path / (name + ".pt"))
        torch.save(sd, files[name])
    files["PERDQN"] = str(tmp_path / "PERDQN.pt")
    torch.save(_sd_of(d["ckpt_all_gene_2_weights"]), files["PERDQN"])
    return [Models.DQN(load_model=files["DQN"], training=False), Models.D3QN(load_model=files["D3QN"], training=False),
            Models.PERDQN(load_model=files["PERDQN"], training=False), Models.PERD3QN(load_model=files["PERD3QN"], training=False),
            Models.PPO(load_model=files["PPO"])]


@pytest.mark.parametrize("rng", ["reference", "philox"])
def test_readme_tester_example_with_the_five_pretrained_brains(tmp_path, rng):
    from reinlife_amd import tester
    np.random.seed(5); random.seed(5)
    brains = _pretrained_all(tmp_path)
    frames = []
    env = tester(brains, width=30, height=30, max_agents=100, static_families=True, fps=10, n_steps=50, rng=rng,
                 on_frame=lambda e: frames.append(e.frame))
    assert len(frames) == 50 and frames[-1].shape == (30 * 24, 30 * 24, 3)
    methods = {"DQN", "D3QN", "PERDQN", "PERD3QN", "PPO"}
    for a in env.agents:
        assert a.brain.method in methods and a.brain.method == brains[a.gene].method


def test_trainer_falls_back_to_the_two_launch_loop_with_a_perdqn(tmp_path):
    """trainer(fused=True) with a PERDQN in the brains list: rl_run refuses the set (RL_E_UNSUPPORTED, naming PERDQN), DeviceWorlds.run
    takes the two-launch loop, and Tracker.results equal those of fused=False."""
    from reinlife_amd import Models, _lib
    from reinlife_amd.Helpers.trainer import trainer
    from reinlife_amd.worlds import _ptr
    torch.manual_seed(12)
    proto = [Models.PERDQN(), Models.DQN(max_epi=90), Models.PERDQN(training=False)]   # (DQN.py:67-69 divides by max_epi)
    envs = []
    for fused in (True, False):
        brains = copy.deepcopy(proto)
        np.random.seed(99)
        with pytest.warns(UserWarning):
            env = trainer(brains, n_episodes=90, update_interval=30, print_results=False, save=False, n_worlds=64, seed=31, fused=fused)
        envs.append(env)
    a, b = envs
    assert a.tracker.results == b.tracker.results or _results_equal(a.tracker.results, b.tracker.results)
    assert len(a.tracker.results["Avg Number of Populations"]) == 3
    assert np.array_equal(a.worlds.s["n_agents"].cpu().numpy(), b.worlds.s["n_agents"].cpu().numpy())
    dw = a.worlds
    assert not dw.run_supported()
    lib = _lib.lib()
    pair = (C.c_void_p * 2)(_ptr(dw._obs2[0]), _ptr(dw._obs2[1]))
    opts = _lib.RunOpts(-1, 0, None, None, 0, 0, None, None)
    rc = lib.rl_run_ex(dw.handle, dw._brains, dw.n_brains, 1, _ptr(dw.actions), C.byref(dw._step_out), pair, 0, None, C.byref(opts), None)
    err = lib.rl_last_error().decode()
    assert rc == _lib_status_unsupported() and "PERDQN" in err and "two-launch loop" in err, (rc, err)


def _lib_status_unsupported():
    return -4   # RL_E_UNSUPPORTED (include/reinlife_hip.h)


def _results_equal(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(_results_equal(x[k], y[k]) for k in x)
    return np.array_equal(np.asarray(x, np.float64), np.asarray(y, np.float64), equal_nan=True)


def test_saver_round_trip(tmp_path, monkeypatch):
    """trainer(save=True) writes PERDQN/brain_gene_<g>.pt with the reference's keys; a brain loaded from it gives bit-equal outputs."""
    from reinlife_amd import Models
    from reinlife_amd.Helpers.trainer import trainer
    monkeypatch.chdir(tmp_path)
    d, _ = _fix()
    torch.manual_seed(4)
    brains = [Models.PERDQN(training=False), Models.PERDQN(training=False)]
    with pytest.warns(UserWarning):
        trainer(brains, n_episodes=3, print_results=False, save=True, n_worlds=2, seed=3)
    files = sorted(glob.glob(str(tmp_path / "experiments" / "*" / "PERDQN" / "brain_gene_*.pt")))
    assert len(files) == 2
    for f in files:
        g = int(f.rsplit("_", 1)[1][:-3])
        sd = torch.load(f)
        assert [(k, tuple(v.shape)) for k, v in sd.items()] == KEYS
        fresh = Models.PERDQN(load_model=f, training=False)
        assert np.array_equal(fresh.forward_batch(d["obs"]).cpu().numpy(), brains[g].forward_batch(d["obs"]).cpu().numpy())
        assert os.path.exists(os.path.join(os.path.dirname(f), "parameters_gene_%d.json" % g))
