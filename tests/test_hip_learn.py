"""GPU: rl_learn / DeviceWorlds.learn / trainer(learn="device") -- the DQN update of ReinLife/Models/DQN.py:80-83, 142-153 on the device,
checked in pieces: gradients against torch float64 autograd, Adam against torch's formula replayed from the kernel's own gradients,
the five fixture steps against the reference's own train() (tests/golden/learn_dqn.npz), the device packer against the host packer
bit for bit, the size gate, the Philox sampler, independence of the learners of a launch, run-to-run determinism, the checked bad
slot, and the whole path through trainer().  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_cases as lc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = 0.0005, 0.98


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.DQN()
    with torch.no_grad():
        for p, v in zip(b.agent.parameters(), lc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, capacity=None, count=None):
    """A replay ring on the device from host rows (dict with ring_state, ...), as DeviceWorlds.enable_capture lays one out."""
    import torch
    n = rows["ring_state"].shape[0]
    capacity = capacity or n
    assert n == capacity
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": torch.zeros(capacity, dtype=torch.int32, device=DEV),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, ring, n_steps, batch=32, want_grad=True):
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring)
    l.batch = batch
    assert (l.lr, l.gamma, l.min_size, l.train_freq) == (LR, GAMMA, 1000, 20)
    l.min_size = 0   # (the fixture's ring holds 48 transitions; the gate has a test of its own)
    if want_grad:
        l.grad = torch.zeros((n_steps, lc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in ("params", "target", "adam_m", "adam_v", "state", "packed")}


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.DQN), np.float32)
    assert lib.rl_policy_pack_weights(_lib.DQN, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def _batch5(g):
    """Five rows of the first minibatch: its duplicated slot twice, a done row, one with |td| < 1 and one with |td| > 1."""
    net = lc.qnet(np.asarray(g["init"], np.float64))
    import torch
    s0 = g["slots"][0]
    td = lc.td_errors(net, net, g, s0, GAMMA, torch.float64).detach().abs().numpy().reshape(-1)
    done = g["ring_done"][s0]
    pick = [0, 1, int(np.nonzero(done == 1)[0][0]), int(np.nonzero((td < 1) & (done == 0))[0][-1]), int(np.nonzero((td > 1) & (done == 0) & (s0 != s0[0]))[0][0])]
    return s0[pick].astype(np.int32)


@pytest.mark.parametrize("batch", [32, 5])
def test_gradients_match_float64_autograd(worlds, batch):
    """One step on a wrapped ring (capacity 48, count 130) with explicit slots: every gradient tensor within 1e-5 of its largest
    magnitude of torch float64 autograd (the project's f32-grade bar), exact zeros where float64 has exact zeros, loss within 1e-5."""
    import torch
    g = lc.golden()
    slots = g["slots"][0] if batch == 32 else _batch5(g)
    assert len(slots) == batch and len(set(slots.tolist())) < batch                      # a duplicate
    td = lc.td_errors(lc.qnet(np.asarray(g["init"], np.float64)), lc.qnet(np.asarray(g["init"], np.float64)), g, slots, GAMMA, torch.float64).detach().abs()
    assert (td < 1).any() and (td > 1).any() and g["ring_done"][slots].any() and not g["ring_done"][slots].all()
    l = _learner(g["init"], _ring(g, count=130), 1, batch=batch)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    loss64, g64 = lc.grads64(g["init"], g["init"], g, slots, GAMMA)
    got = lc.split(l.grad[0].cpu().numpy())
    loss = float(l.loss[0].item())
    print("batch %d: loss %.9g (float64 %.9g, relative error %.3g)" % (batch, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(lc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("batch %d: %-10s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("batch %d: worst gradient error / max|g| = %.3g (torch float32 on the fixture: ref_grad_err %.3g)" % (batch, worst, float(g["ref_grad_err"])))
    for name, a, b in zip(lc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert (g64[3] == 0).any() and (g64[2] == 0).all(axis=1).any(), "no dead fc2 unit in the case"   # dead ReLU units
    assert (g64[4] == 0).all(axis=1).any()                                               # rows of fc3 for actions not taken
    assert (g64[0][:, 3::10] == 0).all()                                                 # input columns that are zero in every row
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert l.state.cpu().tolist() == [1, 1]


@pytest.fixture(scope="module")
def trained(worlds):
    """The five fixture steps, once: the kernel's gradients, losses and every buffer afterwards."""
    import torch
    g = lc.golden()
    l = _learner(g["init"], _ring(g), 5)
    worlds.learn([l], 5, slots=g["slots"].reshape(1, 5, 32))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    out = _np(l)
    out["grad"], out["loss"] = l.grad.cpu().numpy(), l.loss.cpu().numpy()
    out["learner"] = l
    return out


def test_adam_matches_torch_formula_on_the_kernels_own_gradients(trained):
    """torch.optim.Adam replayed in numpy float64 from the kernel's five gradients: every parameter within 1e-5 lr + 1 ulp.  The replay
    keeps its state as torch does -- parameters and moments are float32 tensors, so each step's results are rounded to float32 before
    the next step reads them; the arithmetic of a step is float64.  (The bound is a step's: a handful of f32 roundings of a quantity of
    order lr plus ONE final subtraction.  A replay that never rounds would be compared against five stacked subtractions; its figure
    is printed too.)"""
    g = lc.golden()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v = g["init"].astype(np.float64), np.zeros(lc.N_PARAMS), np.zeros(lc.N_PARAMS)
    pu, mu, vu = p, m, v
    for t in range(1, 6):
        gt = trained["grad"][t - 1].astype(np.float64)
        p, m, v = (f32(x) for x in lc.adam64(p, m, v, gt, t, LR))
        pu, mu, vu = lc.adam64(pu, mu, vu, gt, t, LR)
    err = np.abs(trained["params"].astype(np.float64) - p)
    bound = 1e-5 * LR + np.spacing(np.abs(trained["params"])).astype(np.float64)
    print("Adam: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative to their maxima); "
          "against a replay that never rounds to float32: worst error / bound %.3g"
          % (err.max(), 1e-5 * LR, (err / bound).max(), np.abs(trained["adam_m"] - m).max() / np.abs(m).max(), np.abs(trained["adam_v"] - v).max() / np.abs(v).max(),
             (np.abs(trained["params"].astype(np.float64) - pu) / bound).max()))
    assert (err <= bound).all()
    # ... and against the replay that never rounds: one final subtraction per step, so n_steps ulp + 1e-5 lr -- a drift that the
    # per-step rounding above could absorb shows here
    err_u = np.abs(trained["params"].astype(np.float64) - pu)
    assert (err_u <= 1e-5 * LR + 5 * np.spacing(np.abs(trained["params"])).astype(np.float64)).all()
    assert np.abs(trained["adam_m"] - m).max() <= 1e-5 * np.abs(m).max() and np.abs(trained["adam_v"] - v).max() <= 1e-5 * np.abs(v).max()
    assert trained["state"].tolist() == [5, 1]
    assert trained["target"].tobytes() == trained["params"].tobytes()
    assert np.isfinite(trained["loss"]).all() and (trained["loss"] > 0).all()


def test_five_steps_match_the_reference_end_to_end(trained):
    """Q values (float64, the 48 fixture states) of the kernel's final parameters against the reference's own train(): the difference,
    relative to what training changed, within the reference's own float32 spread scaled by how much looser the project's gradient
    bar (1e-5) is than torch's float32 gradient error."""
    g = lc.golden()
    q_ref, q_got, q_init = lc.q_values(g["final"], g["ring_state"]), lc.q_values(trained["params"], g["ring_state"]), lc.q_values(g["init"], g["ring_state"])
    effect = np.abs(q_ref - q_init).max()
    ratio = np.abs(q_got - q_ref).max() / effect
    bar = float(g["ref_q_spread"]) * (1e-5 / float(g["ref_grad_err"]))
    print("end to end: max|dQ| / training effect = %.3g (bar %.3g; torch float32 against float64: %.3g); effect %.3g; max |p - p_ref| %.3g"
          % (ratio, bar, float(g["ref_q_spread"]), effect, np.abs(trained["params"] - g["final"]).max()))
    assert ratio <= bar


def test_device_packing_is_the_host_packing_bit_for_bit(trained):
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import policy_forward
    host = _host_pack(trained["params"])
    assert trained["packed"].tobytes() == host.tobytes()
    g = lc.golden()
    obs = torch.zeros((49, 153), dtype=torch.float32, device=DEV)
    obs[:48] = torch.as_tensor(g["ring_state"], device=DEV)
    a = policy_forward(_lib.DQN, trained["learner"].packed, obs[:48]).cpu().numpy()
    b = policy_forward(_lib.DQN, torch.as_tensor(host, device=DEV), obs[:48]).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    assert np.abs(a - lc.q_values(trained["params"], g["ring_state"])).max() <= 1e-5 * np.abs(a).max()


def _big_ring_rows(n, seed):
    rng = np.random.RandomState(seed)
    def rows():
        x = (rng.random_sample((n, 153)) < 0.15) * rng.choice(np.array([1.0, -1.0, 0.5], np.float32), size=(n, 153))
        return x.astype(np.float32)
    return {"ring_state": rows(), "ring_state_prime": rows(), "ring_action": rng.randint(0, 8, size=n).astype(np.int8),
            "ring_reward": rng.choice(np.array([0, 0.05, 0.3, -1, 5, -10], np.float32), size=n), "ring_done": (rng.random_sample(n) < 0.2).astype(np.uint8)}


def test_size_gate_and_philox_sampler(worlds):
    """DQN.py:81: 1000 transitions train nothing (the target copy still happens, the call is counted); 1001 do, on the rows that
    rl_philox(seed, 0, brain, calls, RL_SITE_LEARN, s * batch + j) picks -- the same gradient as explicit slots computed on the host."""
    import torch
    from reinlife_amd.learn import philox_slots
    g = lc.golden()
    rows = _big_ring_rows(1100, 3)
    l = _learner(g["init"], _ring(rows, count=1000), 2)
    l.min_size = 1000
    l.target.mul_(0.5)
    before = _np(l)
    worlds.learn([l], 2)
    after = _np(l)
    for k in ("params", "adam_m", "adam_v", "packed"):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["state"].tolist() == [0, 1] and after["target"].tobytes() == before["params"].tobytes()
    assert not l.grad.any().item()
    # one more transition
    a = _learner(g["init"], _ring(rows, count=1001), 2)
    a.min_size = 1000
    worlds.learn([a], 2)
    slots = philox_slots(SEED, 0, 0, 2, 32, 1001)
    assert slots.max() < 1001 and len(np.unique(slots)) > 40
    b = _learner(g["init"], _ring(rows, count=1001), 2)
    b.min_size = 1000
    worlds.learn([b], 2, slots=slots.reshape(1, 2, 32))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [2, 1] and a.grad.any().item()
    assert a.grad.cpu().numpy().tobytes() == b.grad.cpu().numpy().tobytes()
    assert ra["params"].tobytes() == rb["params"].tobytes() and ra["params"].tobytes() != before["params"].tobytes()
    # the second call draws with calls = 1: other rows
    worlds.learn([a], 2)
    torch.cuda.synchronize()
    c = _learner(g["init"], _ring(rows, count=1001), 2)
    c.min_size = 1000
    worlds.learn([c], 2, slots=philox_slots(SEED, 0, 1, 2, 32, 1001).reshape(1, 2, 32))
    torch.cuda.synchronize()
    assert a.state.cpu().tolist() == [4, 2]
    assert not np.array_equal(philox_slots(SEED, 0, 1, 2, 32, 1001), slots)


def test_draws_by_content_do_not_depend_on_the_order_of_the_ring(worlds):
    """rl_learn_draw on a ring and on the same rows in another order: the draws name the same ROWS (other slots), training on them gives
    the same bits, and over 6,400 draws every one of the 48 rows is taken about equally often (uniform, with replacement)."""
    import torch
    g = lc.golden()
    perm = np.random.RandomState(4).permutation(48)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")}
    a, b = _learner(g["init"], _ring(g), 5, want_grad=False), _learner(g["init"], _ring(rows2), 5, want_grad=False)
    sa, sb = worlds.draw_slots([a], 5), worlds.draw_slots([b], 5)
    torch.cuda.synchronize()
    sa, sb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert sa.min() >= 0 and sa.max() < 48 and not np.array_equal(sa, sb)
    assert np.array_equal(perm[sb], sa)                                  # slot j of the permuted ring holds row perm[j]
    assert len(np.unique(sa)) > 40 and len(np.unique(sa)) < 160          # 160 draws of 48 rows: most rows, with repeats
    worlds.learn([a], 5, slots=torch.as_tensor(sa.reshape(1, 5, 32), device=DEV))
    worlds.learn([b], 5, slots=torch.as_tensor(sb.reshape(1, 5, 32), device=DEV))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    for k in ("params", "adam_m", "adam_v", "packed", "state"):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["state"].tolist() == [5, 1]
    # a later call (calls = 1) draws other rows; two learners in one call get tables of their own
    both = worlds.draw_slots([a, b], 5).cpu().numpy()
    assert both.shape == (2, 5, 32) and not np.array_equal(both[0].reshape(-1), sa) and both.min() >= 0 and both.max() < 48
    # uniform: 200 steps x 32 = 6,400 draws over 48 rows, 133 expected per row, standard deviation 11.4: within 5 of them
    c = _learner(g["init"], _ring(g), 1, want_grad=False)
    hist = np.bincount(worlds.draw_slots([c], 200).cpu().numpy().reshape(-1), minlength=48)
    print("draws per row over 6,400: min %d max %d (expected 133.3, sd 11.4)" % (hist.min(), hist.max()))
    assert hist.sum() == 6400 and abs(hist - 6400 / 48).max() <= 5 * 11.4


def _second_case(g):
    rows = {k: np.ascontiguousarray(g[k][::-1]) for k in ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")}
    rows["ring_reward"] = (rows["ring_reward"] * np.float32(0.5)).astype(np.float32)
    return (g["init"] * np.float32(0.75)).astype(np.float32), rows, np.ascontiguousarray(g["slots"][::-1])


def test_learners_of_a_launch_are_independent_and_runs_repeat(worlds):
    g = lc.golden()
    init2, rows2, slots2 = _second_case(g)
    both = np.stack([g["slots"], slots2]).astype(np.int32)

    def pair():
        return _learner(g["init"], _ring(g), 5, want_grad=False), _learner(init2, _ring(rows2), 5, want_grad=False)
    a, b = pair()
    worlds.learn([a, b], 5, slots=both)
    ra, rb = _np(a), _np(b)
    sa, sb = pair()
    worlds.learn([sa], 5, slots=both[0:1])
    worlds.learn([sb], 5, slots=both[1:2])
    rsa, rsb = _np(sa), _np(sb)
    a2, b2 = pair()
    worlds.learn([b2, a2], 5, slots=both[::-1].copy())   # (the other order, again from the same initial buffers)
    ra2, rb2 = _np(a2), _np(b2)
    worlds.check_error_flag()
    for k in ("params", "target", "adam_m", "adam_v", "state", "packed"):
        assert ra[k].tobytes() == rsa[k].tobytes() == ra2[k].tobytes(), k
        assert rb[k].tobytes() == rsb[k].tobytes() == rb2[k].tobytes(), k
    assert ra["params"].tobytes() != rb["params"].tobytes() and ra["state"].tolist() == [5, 1]


def test_a_bad_slot_is_flagged_and_that_brain_is_left_alone(worlds):
    """A slot equal to the ring's size: error-flag code 6 with the brain's index, the step and the value; nothing of that brain is
    written (and nothing is read out of bounds -- every slot is checked before the first row is fetched); the other learner trains."""
    import torch
    g = lc.golden()
    init2, rows2, slots2 = _second_case(g)
    bad = g["slots"].copy()
    bad[2, 3] = 48
    a, b = _learner(g["init"], _ring(g), 5), _learner(init2, _ring(rows2), 5)
    before = _np(a)
    worlds.learn([a, b], 5, slots=np.stack([bad, slots2]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 2, 48]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in ("params", "target", "adam_m", "adam_v", "state", "packed"):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item()
    solo = _learner(init2, _ring(rows2), 5)
    worlds.learn([solo], 5, slots=slots2.reshape(1, 5, 32).astype(np.int32))
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [5, 1] and rb["params"].tobytes() == rs["params"].tobytes()


def _train(learn, tmp=None, **kw):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.DQN(max_epi=60)]
    init = [b.state_dict_flat().copy() for b in brains]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=60, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn=learn,
                      save=tmp is not None, print_results=False, **kw)
    return env, brains, init


def test_trainer_learn_device_trains_and_saves(tmp_path, monkeypatch):
    import torch
    env, brains, init = _train("device")
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    for k, b in enumerate(brains):
        l = env.learners[k]
        assert int(env.worlds.replays[k]["count"].item()) > 1000
        steps, calls = l.state.cpu().tolist()
        assert steps > 0 and steps % 5 == 0 and calls == 3, (steps, calls)
        now = b.state_dict_flat()
        assert not np.array_equal(now, init[k]) and np.isfinite(now).all()
        assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes()             # what the worlds acted with
        assert np.array_equal(np.concatenate([p.detach().numpy().reshape(-1) for p in b.target.state_dict().values()]), l.target.cpu().numpy())
        assert env.worlds._brain_keep[k].data_ptr() == l.packed.data_ptr()
    # learn=None: nothing moves, and the run is what it is without the keyword
    env0, brains0, init0 = _train(None)
    for b, i in zip(brains0, init0):
        assert b.state_dict_flat().tobytes() == i.tobytes()
    assert env0.learners == {} and env0.worlds.replays is None
    env00, _, _ = _train(None)
    assert env0.tracker.results == env00.tracker.results
    # save=True writes the trained weights, and settings.json says which brains learned
    monkeypatch.chdir(tmp_path)
    env3, brains3, init3 = _train("device", tmp=tmp_path)
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "DQN", "brain_gene_*.pt")))
    assert len(files) == 2
    for f, b, i in zip(files, brains3, init3):
        flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(f).values()])
        assert flat.tobytes() == b.state_dict_flat().tobytes() and not np.array_equal(flat, i)
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "trained on the device" in settings and "inference only" not in settings


def test_a_second_identical_trainer_call_gives_the_same_parameters():
    """A second identical trainer(learn="device") call gives bit-identical parameters and Tracker results.  The replay rings are filled
    inside the multi-tick launch, where every world's workgroup reserves its slots with an atomic add on the ring's counter
    (include/reinlife_hip.h, rl_run_opts.replays: "worlds interleaved"): the SET of transitions repeats, their slots do not.  Drawn by
    slot, the two runs parted at the first update (measured: equal ring counts 10,196 / 10,747, ~19,700 of 28,488 parameters different
    by up to 9.6e-3); Environment therefore draws its minibatches by the rows' content (rl_learn_draw)."""
    env, brains, _ = _train("device")
    env2, brains2, _ = _train("device")
    for k, (b, b2) in enumerate(zip(brains, brains2)):
        p1, p2 = b.state_dict_flat(), b2.state_dict_flat()
        print("brain %d: ring counts %d / %d, parameters differing %d of %d, max |p1 - p2| %.3g" % (
            k, int(env.worlds.replays[k]["count"].item()), int(env2.worlds.replays[k]["count"].item()), int((p1 != p2).sum()), p1.size, np.abs(p1 - p2).max()))
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results


def test_brains_of_other_kinds_stay_frozen_and_the_warning_names_them():
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(5)
    brains = [Models.DQN(max_epi=40), Models.D3QN()]
    init = [b.state_dict_flat().copy() for b in brains]
    with pytest.warns(UserWarning, match=r"brains 1 \(D3QN\)"):
        env = trainer(brains, n_episodes=40, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device", save=False,
                      print_results=False)
    assert sorted(env.learners) == [0]
    assert not np.array_equal(brains[0].state_dict_flat(), init[0]) and np.array_equal(brains[1].state_dict_flat(), init[1])
