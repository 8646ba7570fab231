"""GPU: rl_learn_td / rl_learn_td_draw / DeviceWorlds.draw_td / trainer(learn="device", learn_td_priority=True) -- the PERDQN update of
ReinLife/Models/PERDQN.py (train_model, Memory) on the device, checked in pieces: gradients and loss -- with the mean(is_weight) factor --
against torch float64 autograd (full / 33-row / 5-row minibatches), Adam against torch's formula replayed from the kernel's own
gradients, three single-step calls against the reference's own train_model() (tests/golden/learn_perdqn.npz), the priorities, importance
weights and beta of every call, the stamp of new rows, the weighted draw (statistically, and slot for slot against the host
restatement), order independence, the checked bad slot, the size gate, independence of the learners of a launch, run-to-run
determinism, the device packer against the host packer bit for bit, and the whole path through trainer().  Every figure a bar is held
against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = 1e-3, 0.99
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
MEM = ("priority", "beta_is", "seen")


def _brain(flat, **kw):
    import torch
    from reinlife_amd import Models
    b = Models.PERDQN(**kw)
    with torch.no_grad():
        for p, v in zip(b.model.parameters(), tc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, count=None, capacity=None):
    """A replay ring on the device from host rows (dict with ring_state, ...), as DeviceWorlds.enable_capture lays one out."""
    import torch
    capacity = rows["ring_state"].shape[0] if capacity is None else capacity
    t = lambda a, dt: torch.as_tensor(np.array(a[:capacity]), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": torch.zeros(capacity, dtype=torch.int32, device=DEV),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, target_flat, ring, n_steps=1, batch=64, want_grad=True, sync_target=False, priority=None, min_size=0):
    """A PERDQN learner on the fixture's networks; the memory starts with the fixture's priorities (or `priority`), nothing new to stamp
    (seen = count) and beta 0.4.  The size gate is lowered to the 96-row rings unless the test sets it."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    p = tc.golden()
    l = DeviceLearner(_brain(flat), DEV, ring=ring, td_priority=True)
    assert (l.lr, l.gamma, l.batch, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (LR, GAMMA, 64, 999, 20, 1, True)
    assert (l.entry, l.train_start, l.memory_size, l.prio_e, l.prio_a, l.beta_increment) == ("rl_learn_td", 1000, 20000, 0.01, 0.6, 0.001)
    assert np.float32(l.p_new).tobytes() == p["p_new"].tobytes()
    capacity = ring["state"].shape[0]
    assert l.priority.numel() == l.keys.numel() == capacity and l.beta_is.item() == 0.4 and l.seen.item() == 0 and l.beta_is.dtype == torch.float64
    pri = p["prio_init"] if priority is None else priority
    l.priority.copy_(torch.as_tensor(np.array(pri[:capacity], np.float32), device=DEV))
    l.seen.copy_(ring["count"])
    l.batch, l.min_size, l.sync_target = batch, min_size, sync_target
    l.target.copy_(torch.as_tensor(np.array(target_flat, np.float32), device=DEV))
    l.is_weight = torch.zeros((n_steps, batch), dtype=torch.float32, device=DEV)
    if want_grad:
        l.grad = torch.zeros((n_steps, tc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS + MEM}


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.PERDQN), np.float32)
    assert lib.rl_policy_pack_weights(_lib.PERDQN, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def _batch5(g, p):
    """Five rows of the first minibatch: its duplicated slot twice, a done row, and one live row of each sign of the TD error."""
    import torch
    s0 = g["slots"][0]
    pred, target = tc.pred_target(tc.net_of(p["init"]), tc.net_of(p["target_init"]), g, s0, GAMMA, torch.float64)
    td = (pred - target).detach().numpy()
    done = g["ring_done"][s0]
    other = (done == 0) & (s0 != s0[0])
    pick = [0, 1, int(np.nonzero(done == 1)[0][0]), int(np.nonzero(other & (td > 1))[0][0]), int(np.nonzero(other & (td < -1))[0][0])]
    return s0[pick].astype(np.int32)


# ---- 1. one step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [64, 33, 5])
def test_gradients_and_loss_match_float64_autograd(worlds, batch):
    """One step on a wrapped ring (capacity 96, count 250) with explicit slots and the target scaled by 0.9: every gradient tensor
    within 1e-5 of its largest magnitude of torch float64 autograd on loss = mean(w) * mean((pred - target)^2), exact zeros where
    float64 has exact zeros, loss within 1e-5.  The priorities are unequal, so mean(w) != 1: a kernel without the factor fails."""
    import torch
    g, p = dc.golden(), tc.golden()
    slots = g["slots"][0][:batch] if batch > 5 else _batch5(g, p)
    pri = p["prio_init"].copy()
    if batch == 5:
        pri[slots[2]], pri[slots[3]] = np.float32(0.9), np.float32(2.5)                  # (whatever the five rows held: unequal)
    assert len(slots) == batch and len(set(slots.tolist())) < batch                      # a duplicate
    pred, target = tc.pred_target(tc.net_of(p["init"]), tc.net_of(p["target_init"]), g, slots, GAMMA, torch.float64)
    td = (pred - target).detach()
    assert (td > 0).any() and (td < 0).any() and g["ring_done"][slots].any() and not g["ring_done"][slots].all()
    beta = 0.4 + 0.001
    w = tc.is_weights(pri[slots], beta)
    assert len(set(pri[slots].tolist())) > 1 and w.mean() < 0.95
    l = _learner(p["init"], p["target_init"], _ring(g, count=250), batch=batch, priority=pri)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    loss64, g64, prio64, _, _ = tc.step(p["init"], p["target_init"], g, slots, w, GAMMA)
    got = tc.split(l.grad[0].cpu().numpy())
    loss = float(l.loss[0].item())
    print("batch %d: mean(w) %.6g, loss %.9g (float64 %.9g, relative error %.3g)" % (batch, w.mean(), loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(tc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("batch %d: %-12s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("batch %d: worst gradient error / max|g| = %.3g (torch float32 on the fixture: ref_grad_err %.3g)" % (batch, worst, float(p["ref_grad_err"])))
    for name, a, b in zip(tc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    by = dict(zip(tc.NAMES, g64))
    assert (by["fc.0.weight"][:, 3::10] == 0).all()                                      # input columns that are zero in every row
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    ww = l.is_weight[0].cpu().numpy()
    assert (np.abs(ww - w.astype(np.float32)) <= np.spacing(w.astype(np.float32))).all()
    assert l.state.cpu().tolist() == [1, 1] and l.beta_is.item() == beta
    assert l.target.cpu().numpy().tobytes() == p["target_init"].tobytes()                # (the helper switches sync_target off)


@pytest.fixture(scope="module")
def trained(worlds):
    """The fixture's three minibatches in ONE call of three steps (sync_target off: the reference's train_model() never copies), once:
    the kernel's gradients, losses and every buffer afterwards."""
    import torch
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g), 3)
    worlds.learn([l], 3, slots=g["slots"].reshape(1, 3, 64))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    out = _np(l)
    out["grad"], out["loss"], out["is_weight"] = l.grad.cpu().numpy(), l.loss.cpu().numpy(), l.is_weight.cpu().numpy()
    out["learner"] = l
    return out


# ---- 2. Adam -----------------------------------------------------------------------------------------------------------------------
def test_adam_matches_torch_formula_on_the_kernels_own_gradients(trained):
    """torch.optim.Adam replayed in numpy float64 from the kernel's three gradients: every parameter within 1e-5 lr + 1 ulp; parameters
    and moments are rounded to float32 between the steps, as torch keeps them."""
    p = tc.golden()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    q, m, v = p["init"].astype(np.float64), np.zeros(tc.N_PARAMS), np.zeros(tc.N_PARAMS)
    for t in range(1, 4):
        gt = trained["grad"][t - 1].astype(np.float64)
        q, m, v = (f32(x) for x in dc.adam64(q, m, v, gt, t, LR))
    err = np.abs(trained["params"].astype(np.float64) - q)
    bound = 1e-5 * LR + np.spacing(np.abs(trained["params"])).astype(np.float64)
    em, ev = np.abs(trained["adam_m"] - m).max() / np.abs(m).max(), np.abs(trained["adam_v"] - v).max() / np.abs(v).max()
    print("Adam: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative to their maxima)"
          % (err.max(), 1e-5 * LR, (err / bound).max(), em, ev))
    assert (err <= bound).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert trained["state"].tolist() == [3, 1]
    assert trained["target"].tobytes() == p["target_init"].tobytes()                     # sync_target = 0
    assert np.isfinite(trained["loss"]).all() and (trained["loss"] > 0).all()


# ---- 3. the reference's three calls ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_calls(worlds):
    """The fixture's three minibatches as three single-step calls, once: every buffer before and after each, and each call's weights.
    A second learner makes the same calls with its memory set, before each, to the priorities the REFERENCE's memory held at that point
    (the device's own differ from them within the priorities' bound): its weights are the ones to hold against the fixture's."""
    import torch
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g), want_grad=False)
    pinned = _learner(p["init"], p["target_init"], _ring(g), want_grad=False)
    out = {"before": [], "after": [], "is_weight": [], "is_weight_pinned": [], "learner": l}
    ref = p["prio_init"].copy()
    for s in range(3):
        out["before"].append(_np(l))
        worlds.learn([l], 1, slots=g["slots"][s].reshape(1, 1, 64))
        out["after"].append(_np(l))
        out["is_weight"].append(l.is_weight[0].cpu().numpy().copy())
        pinned.priority.copy_(torch.as_tensor(ref, device=DEV))
        worlds.learn([pinned], 1, slots=g["slots"][s].reshape(1, 1, 64))
        out["is_weight_pinned"].append(pinned.is_weight[0].cpu().numpy().copy())
        ref[g["slots"][s].astype(np.int64)] = p["priorities"][s]
    worlds.check_error_flag()
    return out


def test_three_single_step_calls_match_the_reference_end_to_end(trained, three_calls):
    """Q values (float64, the 96 fixture states) of the kernel's final parameters against the reference's own train_model() x 3: the
    difference, relative to what training changed, within the reference's own float32 spread scaled by how much looser the project's
    gradient bar (1e-5) is than torch's float32 gradient error.  One call of three steps ends on the same bits."""
    g, p = dc.golden(), tc.golden()
    got = three_calls["after"][2]
    q_ref, q_got, q_init = tc.q_values(p["final"], g["ring_state"]), tc.q_values(got["params"], g["ring_state"]), tc.q_values(p["init"], g["ring_state"])
    effect = np.abs(q_ref - q_init).max()
    ratio = np.abs(q_got - q_ref).max() / effect
    bar = float(p["ref_q_spread"]) * (1e-5 / float(p["ref_grad_err"]))
    print("end to end: max|dQ| / training effect = %.3g (bar %.3g; torch float32 against float64: %.3g); effect %.3g; max |p - p_ref| %.3g"
          % (ratio, bar, float(p["ref_q_spread"]), effect, np.abs(got["params"] - p["final"]).max()))
    assert ratio <= bar
    assert got["state"].tolist() == [3, 3]
    for k in ("params", "adam_m", "adam_v", "packed", "priority", "beta_is"):
        assert got[k].tobytes() == trained[k].tobytes(), k


# ---- 4. priorities and weights -----------------------------------------------------------------------------------------------------
def test_priorities_weights_and_beta_of_every_call(three_calls):
    """After each call the batch rows hold (|pred - target| + e) ** a within 3.8e-5 x scale + 4 ulp of the float64 formula on float64
    forward passes of the parameters the call started from (scale: the batch's largest |Q|; 3.8 = a e^(a - 1) bounds the formula's
    slope; 1e-5 is the project's forward bar), and of the fixture's recorded priorities; the other rows keep their bits; is_weight
    within 1 float32 ulp of the reference's on the reference's priorities, and of (p / p_min) ** -beta on the device's own (from the
    second call on they differ from the reference's within the bound above, and the weights with them); beta equals the fixture's double."""
    import torch
    g, p = dc.golden(), tc.golden()
    for s in range(3):
        before, after = three_calls["before"][s], three_calls["after"][s]
        idx = g["slots"][s].astype(np.int64)
        w_ref = p["is_weights"][s].astype(np.float32)
        _, _, prio64, pred, target = tc.step(before["params"], before["target"], g, idx, p["is_weights"][s], GAMMA)
        with torch.no_grad():
            scale = max(np.abs(tc.q_values(before["params"], g["ring_state"][idx])).max(), np.abs(tc.q_values(before["target"], g["ring_state_prime"][idx])).max(),
                        np.abs(target).max())
        got = after["priority"][idx]
        ulp = np.spacing(np.abs(got)).astype(np.float64)
        e64, eref = np.abs(got - prio64), np.abs(got.astype(np.float64) - p["priorities"][s])
        w_own = tc.is_weights(before["priority"][idx], p["beta"][s]).astype(np.float32)
        print("call %d: scale %.4g; max |priority - float64| %.3g, max |priority - recorded| %.3g (bound %.3g + 4 ulp); is_weight: worst %.3g ulp "
              "of the reference's, %.3g ulp of the formula on the device's own priorities; beta %.17g"
              % (s, scale, e64.max(), eref.max(), 3.8e-5 * scale, (np.abs(three_calls["is_weight_pinned"][s] - w_ref) / np.spacing(w_ref)).max(),
                 (np.abs(three_calls["is_weight"][s] - w_own) / np.spacing(w_own)).max(), after["beta_is"][0]))
        assert (e64 <= 3.8e-5 * scale + 4 * ulp).all() and (eref <= 3.8e-5 * scale + 4 * ulp).all(), s
        rest = np.setdiff1d(np.arange(96), idx)
        assert len(rest) > 10 and after["priority"][rest].tobytes() == before["priority"][rest].tobytes(), s
        assert (np.abs(three_calls["is_weight_pinned"][s] - w_ref) <= np.spacing(w_ref)).all(), s
        assert (np.abs(three_calls["is_weight"][s] - w_own) <= np.spacing(w_own)).all(), s
        assert after["beta_is"][0] == p["beta"][s], s
        assert after["seen"].tolist() == before["seen"].tolist()                         # the update does not move `seen`
    assert three_calls["after"][0]["priority"][g["slots"][0][0]] == three_calls["after"][0]["priority"][g["slots"][0][1]]


# ---- 5. stamping -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seen, count", [(2, 5), (6, 11), (3, 20), (7, 7), (0, 0), (13, 17)])
def test_new_rows_are_stamped_with_p_new(worlds, seen, count):
    """Capacity 8: a window without wrap, across the wrap, count - seen >= capacity, empty windows (also of an empty ring), and a window
    of a ring that has wrapped before.  The stamped rows hold p_new's bits, the others keep theirs, seen == count afterwards."""
    import torch
    g, p = dc.golden(), tc.golden()
    old = (np.arange(8) * 0.25 + 0.125).astype(np.float32)
    l = _learner(p["init"], p["target_init"], _ring(g, count=count, capacity=8), batch=4, want_grad=False, priority=old)
    l.seen.fill_(seen)
    before = _np(l)
    slots = worlds.draw_td([l], 2)
    r = _np(l)
    worlds.check_error_flag()
    size = min(count, 8)
    want = tc.stamp(old, seen, count, p["p_new"])
    assert r["priority"].tobytes() == want.tobytes() and int(r["seen"][0]) == count
    stamped = want != old
    assert (r["priority"][stamped].view(np.uint32) == p["p_new"].view(np.uint32)).all() and stamped.sum() == min(count - seen, 8)
    s = slots.cpu().numpy()
    assert s.shape == (1, 2, 4) and s.min() >= 0 and s.max() < max(size, 1)
    for k in BUFFERS + ("beta_is",):                                                     # the draw writes the memory's columns alone
        assert r[k].tobytes() == before[k].tobytes(), k
    torch.cuda.synchronize()


# ---- 6. the draw -------------------------------------------------------------------------------------------------------------------
def _counts(worlds, l, pri, calls=25):
    """6,400 draws (25 calls of 4 x 64) from the first 48 rows with the given priorities -> how often each row was drawn, and the rows."""
    import torch
    l.priority[:48] = torch.as_tensor(np.asarray(pri, np.float32), device=DEV)
    rows = []
    for c in range(calls):
        l.state[1] = c
        rows.append(worlds.draw_td([l], 4).cpu().numpy().reshape(-1))
    rows = np.concatenate(rows)
    return np.bincount(rows, minlength=48), rows


def test_draws_are_proportional_to_the_priorities_and_equal_the_host_restatement(worlds):
    """48 rows, priorities over several orders of magnitude with every 7th row at zero, 6,400 draws: no zero-priority row, every other
    count within 5 binomial standard deviations of 6400 p / sum p (a uniform draw fails by far); the draws of the first call equal the
    host restatement slot for slot.  One row with a priority: every draw takes it.  No priority anywhere: the uniform content-key draw."""
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g, count=48, capacity=48), want_grad=False)
    pri = pc.edge_priorities(48)
    n = 6400
    counts, rows = _counts(worlds, l, pri)
    prob = pri.astype(np.float64) / pri.astype(np.float64).sum()
    sd = np.sqrt(n * prob * (1 - prob))
    z = np.abs(counts - n * prob)[pri > 0] / sd[pri > 0]
    zu = np.abs(counts - n / 48) / np.sqrt(n * (1 / 48) * (47 / 48))
    print("weighted: worst deviation %.2f sd (from a uniform draw: %.1f sd)" % (z.max(), zu.max()))
    assert counts.sum() == n and not counts[pri == 0].any()
    assert (z <= 5).all() and zu.max() > 20
    keys = pc.content_keys(g, 48)
    host = np.concatenate([tc.host_draw(keys, pri, SEED, 0, c, 256) for c in range(2)])
    assert np.array_equal(rows[:512], host)
    one = np.zeros(48)
    one[29] = 0.003
    assert _counts(worlds, l, one, 4)[0][29] == 1024
    flat, rows0 = _counts(worlds, l, np.zeros(48))
    zf = np.abs(flat - n / 48) / np.sqrt(n * (1 / 48) * (47 / 48))
    print("all zero: worst deviation from uniform %.2f sd" % zf.max())
    from reinlife_amd import _lib
    assert flat.sum() == n and (zf <= 5).all()
    assert np.array_equal(rows0[:256], pc.host_uniform_draw(keys, SEED, 0, 0, 256, site=_lib.SITE_LEARN_TD))
    empty = _learner(p["init"], p["target_init"], _ring(g, count=0, capacity=48), want_grad=False)
    assert not worlds.draw_td([empty], 1).cpu().numpy().any()                            # an empty ring draws slot 0
    worlds.check_error_flag()


def test_draws_and_training_do_not_depend_on_the_order_of_the_ring(worlds):
    import torch
    g, p = dc.golden(), tc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in dc.RING_KEYS}
    pri = pc.edge_priorities(96)

    def pair():
        return (_learner(p["init"], p["target_init"], _ring(g), 2, want_grad=False, priority=pri),
                _learner(p["init"], p["target_init"], _ring(rows2), 2, want_grad=False, priority=pri[perm]))   # slot j of the permuted ring holds row perm[j]
    a, b = pair()
    sa, sb = worlds.draw_td([a], 2), worlds.draw_td([b], 2)
    both = worlds.draw_td([a, b], 2)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (1, 2, 64) and sa.dtype == torch.int32 and tuple(both.shape) == (2, 2, 64)
    assert torch.equal(both[0:1], sa) and not torch.equal(both[1:2], sb)                 # (the brain index salts the draw)
    sa, sb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert not np.array_equal(sa, sb) and np.array_equal(perm[sb], sa)
    assert (pri[sa] > 0).all() and 10 < len(np.unique(sa)) < 128
    worlds.learn([a], 2, slots=torch.as_tensor(sa.reshape(1, 2, 64), device=DEV))
    worlds.learn([b], 2, slots=torch.as_tensor(sb.reshape(1, 2, 64), device=DEV))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    for k in BUFFERS + ("beta_is",):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["priority"][perm].tobytes() == rb["priority"].tobytes() and ra["priority"].tobytes() != pri.tobytes()
    assert a.is_weight.cpu().numpy().tobytes() == b.is_weight.cpu().numpy().tobytes()
    assert ra["state"].tolist() == [2, 1]


# ---- 7. robustness -----------------------------------------------------------------------------------------------------------------
def _second_case(g, p):
    rows = {k: np.ascontiguousarray(g[k][::-1]) for k in dc.RING_KEYS}
    rows["ring_reward"] = (rows["ring_reward"] * np.float32(0.5)).astype(np.float32)
    return (p["init"] * np.float32(0.75)).astype(np.float32), rows, np.ascontiguousarray(g["slots"][::-1])


def test_learners_of_a_launch_are_independent_and_runs_repeat(worlds):
    g, p = dc.golden(), tc.golden()
    init2, rows2, slots2 = _second_case(g, p)
    both = np.stack([g["slots"], slots2]).astype(np.int32)

    def pair():
        return (_learner(p["init"], p["target_init"], _ring(g), 3, want_grad=False),
                _learner(init2, p["target_init"], _ring(rows2), 3, want_grad=False, sync_target=True, priority=p["prio_init"][::-1]))
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
    for k in BUFFERS + MEM:
        assert ra[k].tobytes() == rsa[k].tobytes() == ra2[k].tobytes() == ra3[k].tobytes(), k
        assert rb[k].tobytes() == rsb[k].tobytes() == rb2[k].tobytes() == rb3[k].tobytes(), k
    assert a.is_weight.cpu().numpy().tobytes() == sa.is_weight.cpu().numpy().tobytes() == a3.is_weight.cpu().numpy().tobytes()
    assert ra["params"].tobytes() != rb["params"].tobytes() and ra["state"].tolist() == [3, 1]
    assert ra["priority"].tobytes() != rb["priority"].tobytes() and rb["target"].tobytes() == rb["params"].tobytes()
    assert ra["target"].tobytes() == p["target_init"].tobytes()


def test_a_bad_slot_is_flagged_and_that_brain_is_left_alone(worlds):
    """A slot equal to the ring's size: error-flag code 6 with the brain's index, the step and the value; nothing of that brain -- its
    priorities, beta and packed weights included -- is written; the other learner trains."""
    import torch
    g, p = dc.golden(), tc.golden()
    init2, rows2, slots2 = _second_case(g, p)
    bad = g["slots"].copy()
    bad[2, 40] = 96
    a, b = _learner(p["init"], p["target_init"], _ring(g), 3, sync_target=True), _learner(init2, p["target_init"], _ring(rows2), 3)
    before = _np(a)
    worlds.learn([a, b], 3, slots=np.stack([bad, slots2]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 2, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in BUFFERS + MEM:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item() and not a.is_weight.any().item() and after["beta_is"][0] == 0.4
    solo = _learner(init2, p["target_init"], _ring(rows2), 3)
    worlds.learn([solo], 3, slots=slots2.reshape(1, 3, 64).astype(np.int32))
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [3, 1]
    for k in BUFFERS + MEM:
        assert rb[k].tobytes() == rs[k].tobytes(), k


def test_a_call_below_the_size_gate_only_syncs_the_target(worlds):
    """size <= min_size (train_start - 1; here 96 rows against a gate of 96): no update -- only target (synced: PERDQNAgent.learn calls
    update_target_model() after every trigger), state[1] and packed (rewritten, to the same bits) move.  One row more trains."""
    g, p = dc.golden(), tc.golden()
    for sync in (True, False):
        l = _learner(p["init"], p["target_init"], _ring(g), min_size=96, sync_target=sync)
        before = _np(l)
        worlds.learn([l], 1, slots=g["slots"][0].reshape(1, 1, 64))
        after = _np(l)
        worlds.check_error_flag()
        for k in ("params", "adam_m", "adam_v", "packed") + MEM:
            assert after[k].tobytes() == before[k].tobytes(), k
        assert after["state"].tolist() == [0, 1] and not l.grad.any().item() and not l.is_weight.any().item()
        assert after["target"].tobytes() == (before["params"] if sync else before["target"]).tobytes()
        assert after["packed"].tobytes() == _host_pack(p["init"]).tobytes()
    l = _learner(p["init"], p["target_init"], _ring(g), min_size=95)
    worlds.learn([l], 1, slots=g["slots"][0].reshape(1, 1, 64))
    assert _np(l)["state"].tolist() == [1, 1]
    worlds.check_error_flag()


def test_the_python_layer_refuses_what_the_entry_points_cannot_do(worlds):
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g), want_grad=False)
    d = DeviceLearner(Models.DQN(max_epi=60), DEV, ring=_ring(g))
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([d, l], 1)
    with pytest.raises(_lib.ReinLifeHipError, match="rl_learn_td_draw"):
        worlds.learn([l], 1)                                                             # no slots: the draw is draw_td()'s job
    with pytest.raises(ValueError, match="PERDQN"):
        worlds.draw_td([d], 1)
    with pytest.raises(_lib.ReinLifeHipError, match="PERDQN memory"):
        d.td_struct()
    with pytest.raises(_lib.ReinLifeHipError, match="kind 4"):
        d.kind = _lib.PERDQN                                                             # rl_learn still refuses the kind
        worlds.learn([d], 1, slots=g["slots"][:1, :32].reshape(1, 1, 32))
    worlds.check_error_flag()


# ---- 8. the packer -----------------------------------------------------------------------------------------------------------------
def test_device_packing_is_the_host_packing_bit_for_bit(trained):
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import policy_forward
    host = _host_pack(trained["params"])
    assert trained["packed"].tobytes() == host.tobytes()
    assert trained["packed"].tobytes() != _host_pack(tc.golden()["init"]).tobytes()
    obs = torch.as_tensor(dc.golden()["ring_state"], device=DEV).contiguous()
    a = policy_forward(_lib.PERDQN, trained["learner"].packed, obs).cpu().numpy()
    b = policy_forward(_lib.PERDQN, torch.as_tensor(host, device=DEV), obs).cpu().numpy()
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()


# ---- 9. trainer() ------------------------------------------------------------------------------------------------------------------
def _train(learn_td_priority, n_episodes=40, save=False, expect_warning=None):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.PERDQN(), Models.DQN(max_epi=60)]
    brains[0].train_start = 200                                                          # (so that the calls of a short run train)
    init = [b.state_dict_flat().copy() for b in brains]
    kw = {"learn_td_priority": True} if learn_td_priority else {}
    args = dict(n_episodes=n_episodes, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device", save=save,
                print_results=False, **kw)
    if expect_warning:
        with pytest.warns(UserWarning, match=expect_warning):
            env = trainer(brains, **args)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            env = trainer(brains, **args)
    return env, brains, init


def test_trainer_learn_td_priority_trains_the_perdqn(tmp_path, monkeypatch):
    """[PERDQN, DQN], 2 worlds, 40 episodes, learn_every 20 (the DQN's train_freq), train_start 200: the PERDQN trains after episodes
    20 and 40, one update each; its epsilon falls by epsilon_decay per update; save=True writes the trained weights."""
    import torch
    from reinlife_amd import _lib
    monkeypatch.chdir(tmp_path)
    env, brains, init = _train(True, save=True)
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    l = env.learners[0]
    count, capacity = int(env.worlds.replays[0]["count"].item()), env.worlds.replays[0]["state"].shape[0]
    pri, seen = l.priority.cpu().numpy(), int(l.seen.item())
    print("PERDQN: state %s, ring count %d of %d, seen %d, beta %.17g, epsilon %.17g, rows re-prioritised %d"
          % (l.state.cpu().tolist(), count, capacity, seen, l.beta_is.item(), brains[0].epsilon, int((pri[:seen] != np.float32(l.p_new)).sum())))
    assert l.entry == "rl_learn_td" and l.state.cpu().tolist() == [2, 2] and l.min_size == 199 and l.trained_from
    assert capacity == brains[0].memory_size == 20000 and 200 <= count < 20000 and env.worlds.replays[1]["state"].shape[0] == 50000
    assert 0 < seen <= count and (pri[:seen] > 0).all() and not pri[seen:].any() and 0 < (pri[:seen] != np.float32(l.p_new)).sum() <= 128
    assert l.beta_is.item() == (0.4 + 0.001) + 0.001
    assert brains[0].epsilon == (1.0 - brains[0].epsilon_decay) - brains[0].epsilon_decay
    now, target = brains[0].state_dict_flat(), l.target.cpu().numpy()
    assert np.isfinite(now).all() and not np.array_equal(now, init[0])
    assert now.tobytes() == l.params.cpu().numpy().tobytes() == target.tobytes()          # model -> target_model at every call
    assert np.array_equal(np.concatenate([t.detach().numpy().reshape(-1) for t in brains[0].target_model.state_dict().values()]), target)
    assert env.worlds._brain_keep[0].data_ptr() == l.packed.data_ptr()                    # what the worlds acted with
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes()
    assert not np.array_equal(brains[1].state_dict_flat(), init[1])                       # the DQN learned too
    note = env._weights_note()
    assert "rl_learn_td" in note and "rl_learn:" in note and "as loaded" not in note
    files = glob.glob(os.path.join(str(tmp_path), "experiments", "*", "PERDQN", "brain_gene_*.pt"))
    assert len(files) == 1
    flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(files[0]).values()])
    assert flat.tobytes() == now.tobytes()
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_td" in settings


def test_without_the_keyword_nothing_changes_and_the_dqn_learner_keeps_its_bits():
    """Without the keyword the PERDQN stays frozen and the warning is the one it was.  The DQN learner's call and draws do not depend on
    the keyword: in runs that end with the first learning call (episode 20: the PERDQN trains BEHIND the DQN's call, and acts on new
    weights and a new epsilon only afterwards) its buffers are bit for bit the same with and without it."""
    env0, brains0, init0 = _train(False, 20, expect_warning=r"brains 0 \(PERDQN\).*PERDQN brains do not learn yet")
    assert sorted(env0.learners) == [1] and brains0[0].state_dict_flat().tobytes() == init0[0].tobytes() and brains0[0].epsilon == 1.0
    assert env0.worlds.replays[0]["state"].shape[0] == 50000 and "their kinds do not learn in this build" in env0._weights_note()
    env, brains, _ = _train(True, 20)
    assert env.learn_every == env0.learn_every == 20 and env.learners[0].state.cpu().tolist() == [1, 1]
    for k in BUFFERS:
        assert getattr(env.learners[1], k).cpu().numpy().tobytes() == getattr(env0.learners[1], k).cpu().numpy().tobytes(), k
    assert brains[1].state_dict_flat().tobytes() == brains0[1].state_dict_flat().tobytes()
    assert env.tracker.results == env0.tracker.results
    st = env0.learners[1].state.cpu().tolist()
    assert st == [5, 1] and int(env0.worlds.replays[1]["count"].item()) > 1000 and not np.array_equal(brains0[1].state_dict_flat(), init0[1])
    assert not np.array_equal(brains[0].state_dict_flat(), brains0[0].state_dict_flat())   # (the PERDQN did train)
