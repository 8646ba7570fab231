"""GPU: rl_learn_ppo / rl_learn_rollout / DeviceWorlds.learn, draw_rollout / trainer(learn="device", learn_rollout=True) -- PPO.learn() of
ReinLife/Models/PPO.py:136-162 on the device, checked in pieces: every epoch's gradients against torch float64 autograd on the same
pre-epoch parameters (rollouts of 32, 17 and 1 rows), Adam against torch's formula replayed from the kernel's own gradients, the fixture's
three rollouts against the reference's own learn() (tests/golden/learn_ppo.npz), the device packer against the host packer bit for bit,
independence of the learners of a launch and run-to-run determinism, the on-policy draw (order independence, the window, uniformity, the
empty window), the checked bad slot and the refusals, and the whole path through trainer().  The ring has capacity 96 and is wrapped
(count 250).  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_ppo_cases as pc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
BUFFERS = ("params", "adam_m", "adam_v", "state", "packed")
RING_KEYS = ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")


def _brain(flat, **kw):
    import torch
    from reinlife_amd import Models
    b = Models.PPO(**kw)
    with torch.no_grad():
        for p, v in zip(b.model.parameters(), pc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, prob, count=250, age=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture(..., with_prob=True) lays one out."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None if prob is None else t(prob, torch.float32),
            "age": torch.zeros(capacity, dtype=torch.int32, device=DEV) if age is None else t(age, torch.int32),
            "count": torch.full((1,), count, dtype=torch.int64, device=DEV)}


def _learner(flat, ring, batch=32, n_grad=0, k_epoch=3):
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring, rollout=True)
    assert (l.entry, l.lr, l.gamma, l.lmbda, l.eps_clip, l.k_epoch, l.batch, l.train_freq) == ("rl_learn_ppo", pc.LR, pc.GAMMA, pc.LMBDA, pc.EPS_CLIP, 3, 32, 20)
    assert l.target is None and l.seen.item() == 0 and l.fresh.item() == 0
    l.batch, l.k_epoch = batch, k_epoch
    if n_grad:
        l.grad = torch.zeros((n_grad, pc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_grad, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS}


def _slots(s):
    return np.asarray(s, np.int32).reshape(1, 1, -1)


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.PPO), np.float32)
    assert lib.rl_policy_pack_weights(_lib.PPO, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


# ---- 1. gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_every_epochs_gradients_match_float64_autograd(worlds, which):
    """The fixture's rollouts of 32, 17 and 1 rows from the initial parameters, three epochs made as three calls of one epoch each so that
    the parameters in front of every epoch can be read: every gradient tensor within 1e-5 of its largest magnitude of torch float64
    autograd on those parameters (the project's f32-grade bar), exact zeros where float64 has them, each loss within 1e-5.  One call of
    three epochs then gives the same bits."""
    import torch
    g = pc.golden()
    slots = pc.rollouts(g)[which]
    n = len(slots)
    rows = pc.rows_of(g, g["prob"], slots)
    l = _learner(g["init"], _ring(g, g["prob"]), batch=n, n_grad=1, k_epoch=1)
    grads = []
    for ep in range(3):
        before = l.params.cpu().numpy().copy()
        worlds.learn([l], 1, slots=_slots(slots), gate=False)
        torch.cuda.synchronize()
        worlds.check_error_flag()
        loss64, g64, mid = pc.grads_autograd(before, rows)
        got, loss = pc.split(l.grad[0].cpu().numpy()), float(l.loss[0].item())
        grads.append(l.grad[0].cpu().numpy().copy())
        print("rows %d epoch %d: loss %.9g (float64 %.9g, relative error %.3g)" % (n, ep, loss, loss64, abs(loss - loss64) / abs(loss64)))
        worst = 0.0
        for name, a, b in zip(pc.NAMES, got, g64):
            err = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))   # (a tensor float64 has all zero: the error itself)
            worst = max(worst, err)
            print("rows %d epoch %d: %-13s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (n, ep, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
        print("rows %d epoch %d: worst gradient error / max|g| = %.3g (torch float32 on the fixture: ref_grad_err %.3g)" % (n, ep, worst, float(g["ref_grad_err"])))
        for name, a, b in zip(pc.NAMES, got, g64):
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (name, ep)
            assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
        assert abs(loss - loss64) <= 1e-5 * abs(loss64)
        by = dict(zip(pc.NAMES, g64))
        assert (by["fc1.weight"][:, 3::10] == 0).all()                                   # input columns that are zero in every row
        assert which != 2 or ((by["fc2.bias"] == 0).any() and (by["fc1.bias"] == 0).any())   # one row: dead units for certain
        if which == 0 and ep == 0:   # the fixture's float64 run starts on the same parameters
            np.testing.assert_allclose([np.abs(x).max() for x in g64], g["grad_max"][0, 0], rtol=1e-9)
    assert l.state.cpu().tolist() == [3, 3]
    one = _learner(g["init"], _ring(g, g["prob"]), batch=n, n_grad=3, k_epoch=3)
    worlds.learn([one], 1, slots=_slots(slots), gate=False)
    r1, r3 = _np(one), _np(l)
    worlds.check_error_flag()
    for k in ("params", "adam_m", "adam_v", "packed"):
        assert r1[k].tobytes() == r3[k].tobytes(), k
    assert r1["state"].tolist() == [3, 1] and one.grad.cpu().numpy().tobytes() == np.stack(grads).tobytes()


# ---- 2. the fixture's three rollouts -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained(worlds):
    """The fixture's rollouts of 32, 17 and 1 rows, three calls on one learner: the kernel's nine gradients and every buffer afterwards."""
    import torch
    g = pc.golden()
    l = _learner(g["init"], _ring(g, g["prob"]), n_grad=3)
    grads, losses = [], []
    for slots in pc.rollouts(g):
        l.batch = len(slots)
        worlds.learn([l], 1, slots=_slots(slots), gate=False)
        torch.cuda.synchronize()
        grads.append(l.grad.cpu().numpy().copy()); losses.append(l.loss.cpu().numpy().copy())
    worlds.check_error_flag()
    out = _np(l)
    out["grad"], out["loss"], out["learner"] = np.concatenate(grads), np.concatenate(losses), l
    return out


def test_adam_matches_torch_formula_on_the_kernels_own_gradients(trained):
    """torch.optim.Adam replayed in numpy float64 from the kernel's nine gradients (parameters and moments rounded to float32 after every
    step, as torch keeps them): every parameter within 1e-5 lr + 1 ulp, the moments within 1e-5 of their maxima."""
    g = pc.golden()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v = g["init"].astype(np.float64), np.zeros(pc.N_PARAMS), np.zeros(pc.N_PARAMS)
    for t in range(1, 10):
        p, m, v = (f32(x) for x in pc.adam64(p, m, v, trained["grad"][t - 1].astype(np.float64), t))
    err = np.abs(trained["params"].astype(np.float64) - p)
    bound = 1e-5 * pc.LR + np.spacing(np.abs(trained["params"])).astype(np.float64)
    em, ev = np.abs(trained["adam_m"] - m).max() / np.abs(m).max(), np.abs(trained["adam_v"] - v).max() / np.abs(v).max()
    print("Adam: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative to their maxima)"
          % (err.max(), 1e-5 * pc.LR, (err / bound).max(), em, ev))
    assert (err <= bound).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert trained["state"].tolist() == [9, 3]
    assert np.isfinite(trained["loss"]).all() and trained["loss"].shape == (9,)


def test_three_rollouts_match_the_reference_end_to_end(trained):
    """Outputs (probabilities and values in float64 over the 96 fixture states) of the kernel's final parameters against the reference's
    own learn(): the distance, relative to what training changed, within the reference's own float32 spread scaled by how much looser
    the project's gradient bar (1e-5) is than torch's float32 gradient error.  Parameters are not compared: Adam's m / sqrt(v) turns noise
    in near-zero gradients into lr-sized steps."""
    g = pc.golden()
    o_ref, o_got, o_init = pc.outputs(g["final"], g["ring_state"]), pc.outputs(trained["params"], g["ring_state"]), pc.outputs(g["init"], g["ring_state"])
    effect = np.abs(o_ref - o_init).max()
    ratio = np.abs(o_got - o_ref).max() / effect
    bar = float(g["ref_out_spread"]) * (1e-5 / float(g["ref_grad_err"]))
    print("end to end: max|d out| / training effect = %.3g (bar %.3g; torch float32 against float64: %.3g); effect %.3g; max |p - p_ref| %.3g"
          % (ratio, bar, float(g["ref_out_spread"]), effect, np.abs(trained["params"] - g["final"]).max()))
    assert ratio <= bar


def test_device_packing_is_the_host_packing_bit_for_bit(trained):
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import policy_forward
    host = _host_pack(trained["params"])
    assert trained["packed"].tobytes() == host.tobytes()
    assert trained["packed"].tobytes() != _host_pack(pc.golden()["init"]).tobytes()
    obs = torch.as_tensor(pc.golden()["ring_state"], device=DEV).contiguous()
    a = policy_forward(_lib.PPO, trained["learner"].packed, obs).cpu().numpy()
    b = policy_forward(_lib.PPO, torch.as_tensor(host, device=DEV), obs).cpu().numpy()
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


# ---- 3. independence and repeatability ---------------------------------------------------------------------------------------------
def _second_case(g):
    rows = {k: np.ascontiguousarray(g[k][::-1]) for k in RING_KEYS}
    rows["ring_reward"] = (rows["ring_reward"] * np.float32(0.5)).astype(np.float32)
    return (g["init"] * np.float32(0.75)).astype(np.float32), rows, np.ascontiguousarray(g["prob"][::-1]), np.ascontiguousarray(g["slots"][:2, :17][:, ::-1])


def test_learners_of_a_launch_are_independent_and_runs_repeat(worlds):
    """Two rollouts of 17 rows per brain in one call: two learners in one launch equal each alone, in either order, and a second run."""
    g = pc.golden()
    init2, rows2, prob2, slots2 = _second_case(g)
    slots1 = np.ascontiguousarray(g["slots"][:2, :17])
    both = np.stack([slots1, slots2]).astype(np.int32)

    def pair():
        return _learner(g["init"], _ring(g, g["prob"]), batch=17), _learner(init2, _ring(rows2, prob2), batch=17)
    a, b = pair()
    worlds.learn([a, b], 2, slots=both, gate=False)
    ra, rb = _np(a), _np(b)
    sa, sb = pair()
    worlds.learn([sa], 2, slots=both[0:1], gate=False)
    worlds.learn([sb], 2, slots=both[1:2], gate=False)
    rsa, rsb = _np(sa), _np(sb)
    a2, b2 = pair()
    worlds.learn([b2, a2], 2, slots=both[::-1].copy(), gate=False)
    ra2, rb2 = _np(a2), _np(b2)
    a3, b3 = pair()
    worlds.learn([a3, b3], 2, slots=both, gate=False)
    ra3, rb3 = _np(a3), _np(b3)
    worlds.check_error_flag()
    for k in BUFFERS:
        assert ra[k].tobytes() == rsa[k].tobytes() == ra2[k].tobytes() == ra3[k].tobytes(), k
        assert rb[k].tobytes() == rsb[k].tobytes() == rb2[k].tobytes() == rb3[k].tobytes(), k
    assert ra["params"].tobytes() != rb["params"].tobytes() and ra["state"].tolist() == [6, 1] == rb["state"].tolist()
    assert ra["params"].tobytes() != g["init"].tobytes()


# ---- 4. rollouts -------------------------------------------------------------------------------------------------------------------
def test_rollouts_do_not_depend_on_the_order_of_the_ring(worlds):
    """Two rings holding the same fresh rows in different slots draw rollouts with identical content, and train to the same bits."""
    import torch
    g = pc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in RING_KEYS}                     # slot j of the permuted ring holds row perm[j]
    a = _learner(g["init"], _ring(g, g["prob"], count=96))
    b = _learner(g["init"], _ring(rows2, g["prob"][perm], count=96))
    sa, sb = worlds.draw_rollout([a], 2), worlds.draw_rollout([b], 2)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (1, 2, 32) and sa.dtype == torch.int32
    assert a.fresh.item() == 96 == b.fresh.item() and a.seen.item() == 96 == b.seen.item()
    na, nb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert not np.array_equal(na, nb) and np.array_equal(perm[nb], na) and 20 < len(np.unique(na)) <= 64
    worlds.learn([a], 2, slots=sa)
    worlds.learn([b], 2, slots=sb)
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    for k in BUFFERS:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["state"].tolist() == [6, 1] and ra["params"].tobytes() != g["init"].tobytes()
    # the draw is the host model's: content keys, Philox words 0-1 of (seed, 0, brain 0, calls 0, RL_SITE_LEARN_ROLLOUT, d)
    from reinlife_amd import _lib
    keys = [pc.row_key(g, r) for r in range(96)]
    assert [int(x) & ((1 << 64) - 1) for x in a.keys.cpu().numpy().tolist()] == keys
    out = (C.c_uint32 * 4)()
    for d in range(64):
        _lib.lib().rl_philox(SEED, 0, 0, 0, _lib.SITE_LEARN_ROLLOUT, d, C.byref(out))
        assert pc.rollout_draw(keys, list(range(96)), (int(out[1]) << 32) | int(out[0])) == na[d], d
    # a later call (state[1] = 1) with nothing appended in between: an empty window
    sc = worlds.draw_rollout([a], 2)
    assert a.fresh.item() == 0 and not sc.any().item()


def test_draws_fall_only_on_the_window_and_are_uniform_over_it(worlds):
    """seen = 202, count = 250 on a ring of 96: the window is the 48 slots 10..57.  6,400 draws fall on it alone, every row's count within
    5 binomial standard deviations of 6400 / 48 (deterministic: this passes always or never)."""
    g = pc.golden()
    l = _learner(g["init"], _ring(g, g["prob"], count=250))
    l.seen.fill_(202)
    window = pc.window_slots(202, 250, 96)
    assert sorted(window) == list(range(10, 58))
    slots = worlds.draw_rollout([l], 200).cpu().numpy().reshape(-1)
    worlds.check_error_flag()
    assert l.fresh.item() == 48 and l.seen.item() == 250 and slots.size == 6400
    counts = np.bincount(slots, minlength=96)
    n, p = 6400, 1 / 48
    z = np.abs(counts[10:58] - n * p) / np.sqrt(n * p * (1 - p))
    print("rollout draws: %d of 6400 outside the window; counts %d..%d (expected %.1f); worst deviation %.2f sd"
          % (counts[:10].sum() + counts[58:].sum(), counts[10:58].min(), counts[10:58].max(), n * p, z.max()))
    assert not counts[:10].any() and not counts[58:].any()
    assert (z <= 5).all()
    # through the wrap, and a window of the whole ring
    l.seen.fill_(250); l.ring["count"].fill_(300)                                        # slots 58..95 and 0..11
    s2 = worlds.draw_rollout([l], 20).cpu().numpy().reshape(-1)
    assert l.fresh.item() == 50 and set(s2.tolist()) <= set(pc.window_slots(250, 300, 96)) and (s2 >= 58).any() and (s2 < 12).any()
    l.ring["count"].fill_(1000)
    s3 = worlds.draw_rollout([l], 20).cpu().numpy().reshape(-1)
    assert l.fresh.item() == 96 and l.seen.item() == 1000 and len(np.unique(s3)) > 60
    worlds.check_error_flag()


def test_an_empty_window_makes_no_update(worlds):
    import torch
    g = pc.golden()
    for count in (0, 250):   # an empty ring (slot 0 is not even a row), and a ring with nothing new
        l = _learner(g["init"], _ring(g, g["prob"], count=count), n_grad=3)
        l.seen.fill_(count)
        before = _np(l)
        slots = worlds.draw_rollout([l], 1)
        worlds.learn([l], 1, slots=slots)
        after = _np(l)
        worlds.check_error_flag()
        assert l.fresh.item() == 0 and not slots.any().item()
        for k in ("params", "adam_m", "adam_v", "packed"):
            assert after[k].tobytes() == before[k].tobytes(), k
        assert after["state"].tolist() == [0, 1] and not l.grad.any().item()
    l.ring["count"].fill_(260)   # ten new rows: the next pair trains
    worlds.learn([l], 1, slots=worlds.draw_rollout([l], 1))
    after = _np(l)
    worlds.check_error_flag()
    assert l.fresh.item() == 10 and after["state"].tolist() == [3, 2] and after["params"].tobytes() != before["params"].tobytes()


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_a_bad_slot_is_flagged_and_that_brain_is_left_alone(worlds):
    import torch
    g = pc.golden()
    init2, rows2, prob2, slots2 = _second_case(g)
    bad = np.ascontiguousarray(g["slots"][:2, :17]).copy()
    bad[1, 5] = 96
    a, b = _learner(g["init"], _ring(g, g["prob"]), batch=17, n_grad=6), _learner(init2, _ring(rows2, prob2), batch=17)
    before = _np(a)
    worlds.learn([a, b], 2, slots=np.stack([bad, slots2]).astype(np.int32), gate=False)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 1, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in BUFFERS:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item()
    solo = _learner(init2, _ring(rows2, prob2), batch=17)
    worlds.learn([solo], 2, slots=slots2.reshape(1, 2, 17).astype(np.int32), gate=False)
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [6, 1]
    for k in BUFFERS:
        assert rb[k].tobytes() == rs[k].tobytes(), k
    # a slot beyond a ring that is still filling (count 40 of 96)
    c = _learner(g["init"], _ring(g, g["prob"], count=40), batch=1)
    worlds.learn([c], 1, slots=_slots([40]), gate=False)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 0, 40] and c.state.cpu().tolist() == [0, 0]
    worlds.err.zero_()


def test_the_python_layer_and_the_entry_points_refuse_what_they_cannot_do(worlds):
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    g = pc.golden()
    l = _learner(g["init"], _ring(g, g["prob"]))
    with pytest.raises(_lib.ReinLifeHipError, match="slots must not be null"):
        worlds.learn([l], 1)                                                             # slots == NULL
    noprob = _learner(g["init"], _ring(g, None))
    with pytest.raises(_lib.ReinLifeHipError, match="prob"):
        worlds.learn([noprob], 1, slots=_slots(g["slots"][0]))                           # a ring without prob
    with pytest.raises(_lib.ReinLifeHipError, match="kind 0"):
        l.kind = _lib.DQN                                                                # a wrong kind
        worlds.learn([l], 1, slots=_slots(g["slots"][0]))
    l.kind = _lib.PPO
    with pytest.raises(ValueError, match="no entry point trains PPO"):
        DeviceLearner(Models.PPO(), DEV, ring=_ring(g, g["prob"]))                       # without rollout=True: what it always raised
    with pytest.raises(ValueError, match="rollout=True is for PPO"):
        DeviceLearner(Models.D3QN(), DEV, ring=_ring(g, g["prob"]), rollout=True)
    d3 = DeviceLearner(Models.D3QN(), DEV, ring=_ring(g, g["prob"]))
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([d3, l], 1, slots=np.zeros((2, 1, 32), np.int32))
    with pytest.raises(ValueError, match="PPO one"):
        worlds.draw_rollout([d3], 1)
    worlds.check_error_flag()


# ---- 6. trainer() ------------------------------------------------------------------------------------------------------------------
def _train(learn_rollout, n_episodes=60, save=False):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.PPO()]
    init = [b.state_dict_flat().copy() for b in brains]
    kw = {"learn_rollout": True} if learn_rollout else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=n_episodes, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      save=save, print_results=False, **kw)
    return env, brains, init


def test_trainer_learn_rollout_trains_the_ppo_and_saves_it(tmp_path, monkeypatch):
    import torch
    from reinlife_amd import Models, _lib
    monkeypatch.chdir(tmp_path)
    env, brains, init = _train(True, save=True)
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    l = env.learners[1]
    count = int(env.worlds.replays[1]["count"].item())
    print("PPO: state %s, ring count %d, seen %d, fresh %d" % (l.state.cpu().tolist(), count, int(l.seen.item()), int(l.fresh.item())))
    assert l.entry == "rl_learn_ppo" and l.state.cpu().tolist() == [9, 3]
    assert env.worlds.replays[1]["prob"] is not None and 0 < int(l.fresh.item()) <= int(l.seen.item()) <= count < 50000
    now = brains[1].state_dict_flat()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1]) and now.tobytes() == l.params.cpu().numpy().tobytes()
    assert env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()                    # what the worlds acted with
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes() != _host_pack(init[1]).tobytes()
    assert not np.array_equal(brains[0].state_dict_flat(), init[0])                       # the DQN learned too
    assert "rl_learn_ppo" in env._weights_note() and "rl_learn:" in env._weights_note()
    # a saved brain reloads with the trained weights
    files = glob.glob(os.path.join(str(tmp_path), "experiments", "*", "PPO", "brain_gene_*.pt"))
    assert len(files) == 1
    assert Models.PPO(load_model=files[0]).state_dict_flat().tobytes() == now.tobytes()
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_ppo" in settings
    # a second identical call: the same bits
    env2, brains2, _ = _train(True)
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    # without the keyword the PPO stays as it was, and its ring records no probabilities
    env0, brains0, init0 = _train(False)
    assert sorted(env0.learners) == [0] and brains0[1].state_dict_flat().tobytes() == init0[1].tobytes()
    assert env0.worlds.replays[1]["prob"] is None


def test_the_dqn_learner_is_bit_for_bit_what_it_is_without_the_keyword():
    """Up to and including episode 20 -- the DQN's first call, with the PPO's first call BEHIND it -- the runs with and without the keyword
    hold the same DQN learner bit for bit.  After that the trained PPO acts differently and the shared worlds part company."""
    env, brains, _ = _train(True, 20)
    env0, brains0, init0 = _train(False, 20)
    assert env.learn_every == env0.learn_every == 20 and env.learners[1].state.cpu().tolist() == [3, 1] and sorted(env0.learners) == [0]
    for k in ("params", "target", "adam_m", "adam_v", "state", "packed"):
        assert getattr(env.learners[0], k).cpu().numpy().tobytes() == getattr(env0.learners[0], k).cpu().numpy().tobytes(), k
    assert brains[0].state_dict_flat().tobytes() == brains0[0].state_dict_flat().tobytes()
    assert env.tracker.results == env0.tracker.results
    assert int(env.worlds.replays[0]["count"].item()) == int(env0.worlds.replays[0]["count"].item())
    st = env0.learners[0].state.cpu().tolist()
    assert st[1] == 1 and st[0] == 5 and not np.array_equal(brains0[0].state_dict_flat(), init0[0])
    assert not np.array_equal(brains[1].state_dict_flat(), brains0[1].state_dict_flat())   # (the PPO did train after episode 20)
