"""GPU: rl_learn_dueling / DeviceWorlds.learn / trainer(learn="device", learn_kinds=("DQN", "D3QN")) -- the D3QN update of
ReinLife/Models/D3QN.py:97-126, 148-165 on the device, checked in pieces: gradients against torch float64 autograd (batch-wide advantage
mean, full / 33-row / 5-row minibatches), Adam against torch's formula replayed from the kernel's own gradients, the three fixture steps
against the reference's own train() (tests/golden/learn_d3qn.npz), the device packer against the host packer bit for bit, sync_target,
the size gate, the Philox sampler, content draws at batch 64, independence of the learners of a launch, run-to-run determinism, the
checked bad slot, and the whole path through trainer().  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = 1e-3, 0.99
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")


def _brain(flat, **kw):
    import torch
    from reinlife_amd import Models
    b = Models.D3QN(**kw)
    with torch.no_grad():
        for p, v in zip(b.eval_net.parameters(), dc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, count=None):
    """A replay ring on the device from host rows (dict with ring_state, ...), as DeviceWorlds.enable_capture lays one out."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": torch.zeros(capacity, dtype=torch.int32, device=DEV),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, target_flat, ring, n_steps, batch=64, want_grad=True, sync_target=False):
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring)
    assert (l.lr, l.gamma, l.batch, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (LR, GAMMA, 64, 63, 20, 1, False)
    assert (l.exploration, l.soft_update_freq, l.entry) == (1000, 200, "rl_learn_dueling")
    l.batch, l.min_size, l.sync_target = batch, batch - 1, sync_target
    l.target.copy_(torch.as_tensor(np.array(target_flat, np.float32), device=DEV))
    if want_grad:
        l.grad = torch.zeros((n_steps, dc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS}


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.D3QN), np.float32)
    assert lib.rl_policy_pack_weights(_lib.D3QN, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def _batch5(g):
    """Five rows of the first minibatch: its duplicated slot twice, a done row, and one live row of each sign of the td error."""
    import torch
    s0 = g["slots"][0]
    td = dc.td_errors(dc.net_of(g["init"]), dc.net_of(g["target_init"]), g, s0, GAMMA, torch.float64).detach().numpy()
    done = g["ring_done"][s0]
    other = (done == 0) & (s0 != s0[0])
    pick = [0, 1, int(np.nonzero(done == 1)[0][0]), int(np.nonzero(other & (td > 1))[0][0]), int(np.nonzero(other & (td < -1))[0][0])]
    return s0[pick].astype(np.int32)


@pytest.mark.parametrize("batch", [64, 33, 5])
def test_gradients_match_float64_autograd(worlds, batch):
    """One step on a wrapped ring (capacity 96, count 250) with explicit slots: every gradient tensor within 1e-5 of its largest
    magnitude of torch float64 autograd (the project's f32-grade bar), exact zeros where float64 has exact zeros, loss within 1e-5.
    64 rows fill the minibatch, 33 cross a 32-row boundary, 5 leave padding rows that must stay out of the batch-wide mean."""
    import torch
    g = dc.golden()
    slots = g["slots"][0][:batch] if batch > 5 else _batch5(g)
    assert len(slots) == batch and len(set(slots.tolist())) < batch                      # a duplicate
    td = dc.td_errors(dc.net_of(g["init"]), dc.net_of(g["target_init"]), g, slots, GAMMA, torch.float64).detach()
    assert (td > 0).any() and (td < 0).any() and g["ring_done"][slots].any() and not g["ring_done"][slots].all()
    l = _learner(g["init"], g["target_init"], _ring(g, count=250), 1, batch=batch)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    loss64, g64 = dc.grads64(g["init"], g["target_init"], g, slots, GAMMA)
    got = dc.split(l.grad[0].cpu().numpy())
    loss = float(l.loss[0].item())
    print("batch %d: loss %.9g (float64 %.9g, relative error %.3g)" % (batch, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(dc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("batch %d: %-17s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("batch %d: worst gradient error / max|g| = %.3g (torch float32 on the fixture: ref_grad_err %.3g)" % (batch, worst, float(g["ref_grad_err"])))
    for name, a, b in zip(dc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    by = dict(zip(dc.NAMES, g64))
    assert (by["adv_fc1.bias"] == 0).any() and (by["value_fc1.bias"] == 0).any(), "no dead branch unit in the case"   # dead ReLU units
    assert (by["adv_fc1.weight"] == 0).all(axis=1).any() and (by["value_fc2.weight"] == 0).any()
    assert (by["fc.weight"][:, 3::10] == 0).all()                                        # input columns that are zero in every row
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert l.state.cpu().tolist() == [1, 1]


@pytest.fixture(scope="module")
def trained(worlds):
    """The three fixture steps, once: the kernel's gradients, losses and every buffer afterwards."""
    import torch
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), 3)
    worlds.learn([l], 3, slots=g["slots"].reshape(1, 3, 64))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    out = _np(l)
    out["grad"], out["loss"] = l.grad.cpu().numpy(), l.loss.cpu().numpy()
    out["learner"] = l
    return out


def test_adam_matches_torch_formula_on_the_kernels_own_gradients(trained):
    """torch.optim.Adam replayed in numpy float64 from the kernel's three gradients: every parameter within 1e-5 lr + 1 ulp.  The replay
    keeps its state as torch does -- parameters and moments are float32 tensors, so each step's results are rounded to float32 before
    the next step reads them; the arithmetic of a step is float64."""
    g = dc.golden()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v = g["init"].astype(np.float64), np.zeros(dc.N_PARAMS), np.zeros(dc.N_PARAMS)
    for t in range(1, 4):
        gt = trained["grad"][t - 1].astype(np.float64)
        p, m, v = (f32(x) for x in dc.adam64(p, m, v, gt, t, LR))
    err = np.abs(trained["params"].astype(np.float64) - p)
    bound = 1e-5 * LR + np.spacing(np.abs(trained["params"])).astype(np.float64)
    em, ev = np.abs(trained["adam_m"] - m).max() / np.abs(m).max(), np.abs(trained["adam_v"] - v).max() / np.abs(v).max()
    print("Adam: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative to their maxima)"
          % (err.max(), 1e-5 * LR, (err / bound).max(), em, ev))
    assert (err <= bound).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert trained["state"].tolist() == [3, 1]
    assert trained["target"].tobytes() == g["target_init"].tobytes()                     # sync_target = 0
    assert np.isfinite(trained["loss"]).all() and (trained["loss"] > 0).all()


def test_three_steps_match_the_reference_end_to_end(trained):
    """Q values (float64, the 96 fixture states as one batch) of the kernel's final parameters against the reference's own train(): the
    difference, relative to what training changed, within the reference's own float32 spread scaled by how much looser the project's
    gradient bar (1e-5) is than torch's float32 gradient error."""
    g = dc.golden()
    q_ref, q_got, q_init = dc.q_values(g["final"], g["ring_state"]), dc.q_values(trained["params"], g["ring_state"]), dc.q_values(g["init"], g["ring_state"])
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
    assert trained["packed"].tobytes() != _host_pack(dc.golden()["init"]).tobytes()
    obs = torch.as_tensor(dc.golden()["ring_state"], device=DEV).contiguous()
    a = policy_forward(_lib.D3QN, trained["learner"].packed, obs).cpu().numpy()
    b = policy_forward(_lib.D3QN, torch.as_tensor(host, device=DEV), obs).cpu().numpy()
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


def test_sync_target_copies_the_parameters_only_when_asked(worlds, trained):
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), 3, want_grad=False, sync_target=True)
    worlds.learn([l], 3, slots=g["slots"].reshape(1, 3, 64))
    r = _np(l)
    worlds.check_error_flag()
    assert r["params"].tobytes() == trained["params"].tobytes()                         # the same update as with sync_target = 0 ...
    assert r["target"].tobytes() == r["params"].tobytes() != g["target_init"].tobytes()  # ... and the copy afterwards
    assert trained["target"].tobytes() == g["target_init"].tobytes()


def test_size_gate_and_philox_sampler(worlds):
    """The reference's only gate is random.sample's need of `batch` rows (D3QN.py:98, 140): batch - 1 transitions train nothing (the call is
    counted, the target copied if asked); `batch` do, on the rows rl_philox(seed, 0, brain, calls, RL_SITE_LEARN, j) picks -- the same
    gradient as explicit slots computed on the host."""
    import torch
    from reinlife_amd.learn import philox_slots
    g = dc.golden()
    for sync in (False, True):
        l = _learner(g["init"], g["target_init"], _ring(g, count=63), 1, sync_target=sync)
        before = _np(l)
        worlds.learn([l], 1)
        after = _np(l)
        for k in ("params", "adam_m", "adam_v", "packed"):
            assert after[k].tobytes() == before[k].tobytes(), k
        assert after["state"].tolist() == [0, 1] and not l.grad.any().item()
        assert after["target"].tobytes() == (before["params"] if sync else before["target"]).tobytes()
    a = _learner(g["init"], g["target_init"], _ring(g, count=64), 1)
    worlds.learn([a], 1)
    slots = philox_slots(SEED, 0, 0, 1, 64, 64)
    assert slots.shape == (1, 64) and slots.max() < 64 and len(np.unique(slots)) > 30
    b = _learner(g["init"], g["target_init"], _ring(g, count=64), 1)
    worlds.learn([b], 1, slots=slots.reshape(1, 1, 64))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [1, 1] and a.grad.any().item()
    assert a.grad.cpu().numpy().tobytes() == b.grad.cpu().numpy().tobytes()
    assert ra["params"].tobytes() == rb["params"].tobytes() and ra["params"].tobytes() != g["init"].tobytes()
    torch.cuda.synchronize()


def test_draws_by_content_for_batch_64_do_not_depend_on_the_order_of_the_ring(worlds):
    """draw_slots for a batch-64 learner (rl_learn_draw asked for [2 n_steps][32]: the same flat table): [n, n_steps, 64] inside
    [0, size), the same ROWS on a permuted ring, and training on either gives the same bits."""
    import torch
    g = dc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in dc.RING_KEYS}
    a, b = _learner(g["init"], g["target_init"], _ring(g), 2, want_grad=False), _learner(g["init"], g["target_init"], _ring(rows2), 2, want_grad=False)
    sa, sb = worlds.draw_slots([a], 2), worlds.draw_slots([b], 2)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (1, 2, 64) and sa.dtype == torch.int32
    both = worlds.draw_slots([a, b], 2)
    assert tuple(both.shape) == (2, 2, 64) and int(both.min()) >= 0 and int(both.max()) < 96
    sa, sb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert sa.min() >= 0 and sa.max() < 96 and not np.array_equal(sa, sb)
    assert np.array_equal(perm[sb], sa)                                  # slot j of the permuted ring holds row perm[j]
    assert 50 < len(np.unique(sa)) < 128                                 # 128 draws of 96 rows: most rows, with repeats
    worlds.learn([a], 2, slots=torch.as_tensor(sa.reshape(1, 2, 64), device=DEV))
    worlds.learn([b], 2, slots=torch.as_tensor(sb.reshape(1, 2, 64), device=DEV))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    for k in BUFFERS:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["state"].tolist() == [2, 1]
    # a smaller ring: the draws stay inside its size
    c = _learner(g["init"], g["target_init"], _ring(g, count=70), 1, want_grad=False)
    sc = worlds.draw_slots([c], 1).cpu().numpy()
    assert sc.shape == (1, 1, 64) and sc.min() >= 0 and sc.max() < 70


def _second_case(g):
    rows = {k: np.ascontiguousarray(g[k][::-1]) for k in dc.RING_KEYS}
    rows["ring_reward"] = (rows["ring_reward"] * np.float32(0.5)).astype(np.float32)
    return (g["init"] * np.float32(0.75)).astype(np.float32), rows, np.ascontiguousarray(g["slots"][::-1])


def test_learners_of_a_launch_are_independent_and_runs_repeat(worlds):
    g = dc.golden()
    init2, rows2, slots2 = _second_case(g)
    both = np.stack([g["slots"], slots2]).astype(np.int32)

    def pair():
        return (_learner(g["init"], g["target_init"], _ring(g), 3, want_grad=False),
                _learner(init2, g["target_init"], _ring(rows2), 3, want_grad=False, sync_target=True))
    a, b = pair()
    worlds.learn([a, b], 3, slots=both)
    ra, rb = _np(a), _np(b)
    sa, sb = pair()
    worlds.learn([sa], 3, slots=both[0:1])
    worlds.learn([sb], 3, slots=both[1:2])
    rsa, rsb = _np(sa), _np(sb)
    a2, b2 = pair()
    worlds.learn([b2, a2], 3, slots=both[::-1].copy())   # (the other order, again from the same initial buffers)
    ra2, rb2 = _np(a2), _np(b2)
    a3, b3 = pair()
    worlds.learn([a3, b3], 3, slots=both)                 # (a second run)
    ra3, rb3 = _np(a3), _np(b3)
    worlds.check_error_flag()
    for k in BUFFERS:
        assert ra[k].tobytes() == rsa[k].tobytes() == ra2[k].tobytes() == ra3[k].tobytes(), k
        assert rb[k].tobytes() == rsb[k].tobytes() == rb2[k].tobytes() == rb3[k].tobytes(), k
    assert ra["params"].tobytes() != rb["params"].tobytes() and ra["state"].tolist() == [3, 1]


def test_a_bad_slot_is_flagged_and_that_brain_is_left_alone(worlds):
    """A slot equal to the ring's size: error-flag code 6 with the brain's index, the step and the value; nothing of that brain is
    written (and nothing is read out of bounds -- every slot is checked before the first row is fetched); the other learner trains."""
    import torch
    g = dc.golden()
    init2, rows2, slots2 = _second_case(g)
    bad = g["slots"].copy()
    bad[2, 40] = 96
    a, b = _learner(g["init"], g["target_init"], _ring(g), 3, sync_target=True), _learner(init2, g["target_init"], _ring(rows2), 3)
    before = _np(a)
    worlds.learn([a, b], 3, slots=np.stack([bad, slots2]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 2, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in BUFFERS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item()
    solo = _learner(init2, g["target_init"], _ring(rows2), 3)
    worlds.learn([solo], 3, slots=slots2.reshape(1, 3, 64).astype(np.int32))
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [3, 1] and rb["params"].tobytes() == rs["params"].tobytes()


def test_mixed_kinds_in_one_learn_call_are_refused(worlds):
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    g = dc.golden()
    d3 = _learner(g["init"], g["target_init"], _ring(g), 1, want_grad=False)
    dqn = DeviceLearner(Models.DQN(), DEV, ring=_ring(g))
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([dqn, d3], 1)


def _train(learn_kinds, **kw):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.D3QN(exploration=20, soft_update_freq=40)]
    init = [b.state_dict_flat().copy() for b in brains]
    if learn_kinds is not None:
        kw["learn_kinds"] = learn_kinds
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=60, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      save=False, print_results=False, **kw)
    return env, brains, init


def test_trainer_learn_kinds_trains_the_d3qn_on_its_schedule():
    """exploration 20, soft_update_freq 40, learn_every 20 (the smallest train_freq): the D3QN trains after episodes 40 and 60 (not 20:
    D3QN.py:121 asks n_epi > exploration) and its target is synced at 40 alone."""
    env, brains, init = _train(("DQN", "D3QN"))
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    l = env.learners[1]
    count = int(env.worlds.replays[1]["count"].item())
    print("D3QN: state %s, ring count %d of %d" % (l.state.cpu().tolist(), count, env.worlds.replays[1]["state"].shape[0]))
    assert l.state.cpu().tolist() == [2, 2]
    assert env.worlds.replays[1]["state"].shape[0] == brains[1].capacity == 10000 and 64 <= count < 10000   # (no wrap: the rows do not depend on append order)
    assert env.worlds.replays[0]["state"].shape[0] == 50000
    now, target = brains[1].state_dict_flat(), l.target.cpu().numpy()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1])
    assert now.tobytes() == l.params.cpu().numpy().tobytes()
    assert not np.array_equal(target, init[1]) and not np.array_equal(target, now)       # synced at 40, not at 60
    assert np.array_equal(np.concatenate([p.detach().numpy().reshape(-1) for p in brains[1].target_net.state_dict().values()]), target)
    assert env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()                    # what the worlds acted with
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes()
    assert not np.array_equal(brains[0].state_dict_flat(), init[0])                       # the DQN learned too
    assert "rl_learn_dueling" in env._weights_note() and "rl_learn:" in env._weights_note()
    # a second identical call: the same bits
    env2, brains2, _ = _train(("DQN", "D3QN"))
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    # without learn_kinds the D3QN stays as it was, and the DQN learner's run does not depend on the D3QN's learning call
    env0, brains0, init0 = _train(None)
    assert sorted(env0.learners) == [0] and brains0[1].state_dict_flat().tobytes() == init0[1].tobytes()
