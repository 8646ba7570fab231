"""GPU: rl_learn_td_wide / rl_learn_td_wide_draw / rl_learn_td_wide_draw_rank / DeviceLearner(td_priority=True, td_batch=) /
trainer(learn_td_priority=True, learn_batch={"PERDQN": B}) -- PERDQNAgent.train_model() (ReinLife/Models/PERDQN.py:130-186) on minibatches
of several 64-row tiles: one tile is rl_learn_td bit for bit (every learner buffer, the priorities, beta, the weights, loss and gradients);
several tiles against torch float64 autograd on mean(w) * mean((pred - target)^2) with w and both means over the WHOLE batch (the inputs
tell a per-tile p_min or mean apart 1,000 times over: tests/test_learn_td_wide_cpu.py); Adam replayed from the kernel's own gradients; the
priorities, weights and beta; slots duplicated across tiles; the checked bad slot, the size gate, sixteen learners, repeatability, the
packer; the two wide draws against the narrow ones and the host restatements; the refusals; and the whole path through trainer().  Every
figure a bar is held against is printed before it is asserted.
Measured on an MI355X: see docs/experiments.md, Part Z."""
import ctypes as C
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc
import learn_prio_rank_cases as rk
import learn_td_wide_cases as wc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
ALL = BUFFERS + ("priority", "beta_is", "is_weight", "loss", "grad")


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.PERDQN()
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


def _learner(n_steps, batch, wide=True, rows=None, priority=None, flat=None, sync_target=False, min_size=0, count=None):
    """wide: a PERDQN learner through rl_learn_td_wide; else through rl_learn_td.  On the fixture's networks with is_weight, grad and loss
    rows and an open gate unless min_size says otherwise; the memory starts with `priority` (learn_td_wide_cases.priorities of the ring),
    nothing new to stamp (seen = count) and beta 0.4."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    p = tc.golden()
    rows = dc.golden() if rows is None else rows
    ring = _ring(rows, count=count)
    capacity = ring["state"].shape[0]
    l = DeviceLearner(_brain(p["init"] if flat is None else flat), DEV, ring=ring, td_priority=True, **({"td_batch": batch} if wide else {}))
    assert l.entry == ("rl_learn_td_wide" if wide else "rl_learn_td")
    assert (l.lr, l.gamma, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (wc.LR, wc.GAMMA, 999, 20, 1, True)
    assert l.priority.numel() == l.keys.numel() == capacity and l.beta_is.item() == 0.4 and l.seen.item() == 0
    if wide:
        assert l.batch == batch and l.work.numel() == wc.work_bytes(batch) and l.work.data_ptr() % 16 == 0
        l.work.fill_(0xA5)   # the work buffer needs no initialisation
    else:
        assert l.work is None and l.batch == 64
    pri = wc.priorities(capacity) if priority is None else priority
    l.priority.copy_(torch.as_tensor(np.array(pri[:capacity], np.float32), device=DEV))
    l.seen.copy_(ring["count"])
    l.batch, l.min_size, l.sync_target = batch, min_size, sync_target
    l.target.copy_(torch.as_tensor(np.array(p["target_init"], np.float32), device=DEV))
    l.is_weight = torch.zeros((n_steps, batch), dtype=torch.float32, device=DEV)
    l.grad = torch.zeros((n_steps, tc.N_PARAMS), dtype=torch.float32, device=DEV)
    l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in ALL}


def _same(a, b, keys=ALL):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _learn(worlds, l, slots, n_steps=1):
    worlds.learn([l], n_steps, slots=np.ascontiguousarray(slots, np.int32).reshape(1, n_steps, l.batch))
    return _np(l)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.PERDQN), np.float32)
    assert lib.rl_policy_pack_weights(_lib.PERDQN, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


# ---- one tile is rl_learn_td, bit for bit ----

@pytest.mark.parametrize("n_steps", [1, 3])
@pytest.mark.parametrize("batch", wc.ONE_TILE_BATCHES)
def test_one_tile_is_rl_learn_td_bit_for_bit(worlds, batch, n_steps):
    """The fixture's slots on the wrapped fixture ring (capacity 96, count 250), unequal priorities, once with the target copy: params,
    target, adam_m, adam_v, state, packed, the whole priority array, beta, is_weight, loss and grad of rl_learn_td_wide are rl_learn_td's
    from the same start, and the launches are counted as the header counts them."""
    g = dc.golden()
    slots = np.ascontiguousarray(g["slots"][:n_steps, :batch]).astype(np.int32)
    mk = lambda wide: _learner(n_steps, batch, wide, count=250, sync_target=batch == 33)  # noqa: E731
    before = worlds.launches
    ra = _learn(worlds, mk(True), slots, n_steps)
    assert worlds.launches - before == wc.launches(n_steps)
    rb = _learn(worlds, mk(False), slots, n_steps)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [n_steps, 1] and rb["grad"].any() and (rb["loss"] > 0).all()
    assert rb["params"].tobytes() != np.asarray(tc.golden()["init"]).tobytes()
    assert (rb["target"].tobytes() == rb["params"].tobytes()) == (batch == 33)
    assert (rb["priority"] != wc.priorities(96)).sum() == len(np.unique(slots)) and rb["beta_is"][0] > 0.4
    assert batch == 1 or (rb["is_weight"] < 1).any()
    _same(ra, rb)


# ---- several tiles against float64 ----

@pytest.mark.parametrize("batch", wc.MULTI_TILE_BATCHES)
def test_gradients_and_loss_of_several_tiles_match_float64_autograd(worlds, batch):
    """One step on learn_td_wide_cases.inputs(batch) -- unequal priorities over a factor of 100 and more, the smallest in one row of the
    last tile; 2048 rows on a 300-row ring, so slots repeat across tiles: every gradient tensor within 1e-5 of its largest magnitude of
    torch float64 autograd on mean(w) * mean((pred - target)^2) with w and both means over the WHOLE batch, exact zeros where float64 has
    exact zeros, the loss within 1e-5: the bar tests/test_hip_learn_perdqn.py holds rl_learn_td to."""
    slots, pri, w, loss64, g64 = wc.case(batch)
    assert wc.tiles(batch) > 1 and abs(w.mean() - 1) > 0.05 and np.argmin(pri[slots]) >= wc.TILE * (wc.tiles(batch) - 1)
    l = _learner(1, batch, rows=wc.ring_of(batch), priority=pri)
    r = _learn(worlds, l, slots)
    worlds.check_error_flag()
    got = tc.split(r["grad"][0])
    loss = float(r["loss"][0])
    worst, per = wc.worst_relative_error(got, g64)
    print("batch %d (%d tiles): mean(w) %.6g, loss %.9g (float64 %.9g, relative error %.3g)"
          % (batch, wc.tiles(batch), w.mean(), loss, loss64, abs(loss - loss64) / abs(loss64)))
    for name, err, b in zip(tc.NAMES, per, g64):
        print("batch %d: %-12s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("batch %d: worst gradient error / max|g| = %.3g (bar %.0e)" % (batch, worst, wc.BAR))
    for name, a, b in zip(tc.NAMES, got, g64):
        assert np.abs(a - b).max() <= wc.BAR * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert abs(loss - loss64) <= wc.BAR * abs(loss64)
    ww = r["is_weight"][0]
    assert (np.abs(ww - w.astype(np.float32)) <= np.spacing(w.astype(np.float32))).all()
    assert r["state"].tolist() == [1, 1] and r["beta_is"][0] == wc.BETA1


# ---- Adam ----

@pytest.fixture(scope="module")
def three_steps(worlds):
    """Three steps of 130 rows in ONE call on the fixture ring, once: every buffer afterwards."""
    slots = wc.slots_of(130, 3)
    l = _learner(3, 130)
    out = _learn(worlds, l, slots, 3)
    worlds.check_error_flag()
    out["slots"], out["learner"] = slots, l
    return out


def test_adam_matches_torch_formula_on_the_kernels_own_gradients(three_steps):
    """torch.optim.Adam replayed in numpy float64 from the kernel's three gradients: every parameter within 1e-5 lr + 1 ulp, the moments
    within 1e-5 of their largest; parameters and moments are rounded to float32 between the steps, as torch keeps them."""
    p = tc.golden()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    q, m, v = p["init"].astype(np.float64), np.zeros(tc.N_PARAMS), np.zeros(tc.N_PARAMS)
    for t in range(1, 4):
        q, m, v = (f32(x) for x in dc.adam64(q, m, v, three_steps["grad"][t - 1].astype(np.float64), t, wc.LR))
    err = np.abs(three_steps["params"].astype(np.float64) - q)
    bound = 1e-5 * wc.LR + np.spacing(np.abs(three_steps["params"])).astype(np.float64)
    em, ev = np.abs(three_steps["adam_m"] - m).max() / np.abs(m).max(), np.abs(three_steps["adam_v"] - v).max() / np.abs(v).max()
    print("Adam: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative to their maxima)"
          % (err.max(), 1e-5 * wc.LR, (err / bound).max(), em, ev))
    assert (err <= bound).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert three_steps["state"].tolist() == [3, 1]
    assert three_steps["target"].tobytes() == p["target_init"].tobytes()                 # sync_target = 0
    assert np.isfinite(three_steps["loss"]).all() and (three_steps["loss"] > 0).all()


# ---- priorities, weights, beta ----

def test_priorities_of_every_batch_row_and_the_rows_outside_the_batch(worlds):
    """After one step of 130 rows every batch row holds (|pred - target| + e) ** a within 3.8e-5 x scale + 4 ulp of the float64 formula on
    float64 forward passes (tests/test_hip_learn_perdqn.py's bar: scale the batch's largest |Q|, 3.8 bounds the formula's slope, 1e-5 the
    forward bar); the rows outside the batch keep their bits; is_weight is the host restatement over the whole batch."""
    g, p = dc.golden(), tc.golden()
    slots, pri, w, _, _ = wc.case(130)
    idx = slots.astype(np.int64)
    r = _learn(worlds, _learner(1, 130, priority=pri), slots)
    worlds.check_error_flag()
    _, _, prio64, _, target = tc.step(p["init"], p["target_init"], g, idx, w, wc.GAMMA)
    scale = max(np.abs(tc.q_values(p["init"], g["ring_state"][idx])).max(), np.abs(tc.q_values(p["target_init"], g["ring_state_prime"][idx])).max(),
                np.abs(target).max())
    got = r["priority"][idx]
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    e64 = np.abs(got - prio64)
    print("130 rows: scale %.4g; max |priority - float64| %.3g (bound %.3g + 4 ulp)" % (scale, e64.max(), 3.8e-5 * scale))
    assert (e64 <= 3.8e-5 * scale + 4 * ulp).all()
    rest = np.setdiff1d(np.arange(96), idx)
    assert len(rest) > 10 and r["priority"][rest].tobytes() == pri[rest].tobytes()
    w32 = tc.is_weights(pri[idx], wc.BETA1).astype(np.float32)
    assert (np.abs(r["is_weight"][0] - w32) <= np.spacing(w32)).all() and r["is_weight"][0].min() < 0.2 and r["is_weight"][0].max() == 1


def test_beta_is_the_narrow_learners_and_later_steps_see_earlier_priority_writes(worlds, three_steps):
    """beta after three steps is rl_learn_td's double ((0.4 + 0.001) + 0.001) + 0.001.  One call of three steps is three calls of one step:
    step 2's weights are made from the priorities step 1 wrote -- every buffer but the call counter ends on the same bits, and the weights
    of steps 2 and 3 differ from what the initial priorities would give."""
    g = dc.golden()
    narrow = _learn(worlds, _learner(3, 64, wide=False), g["slots"], 3)
    assert three_steps["beta_is"].tobytes() == narrow["beta_is"].tobytes() and narrow["beta_is"][0] == ((0.4 + 0.001) + 0.001) + 0.001
    slots = three_steps["slots"]
    l = _learner(1, 130)
    weights, losses, grads = [], [], []
    for s in range(3):
        r = _learn(worlds, l, slots[s])
        weights.append(r["is_weight"][0]); losses.append(r["loss"][0]); grads.append(r["grad"][0])
    worlds.check_error_flag()
    assert r["state"].tolist() == [3, 3]
    _same(r, three_steps, ("params", "target", "adam_m", "adam_v", "packed", "priority", "beta_is"))
    assert np.stack(weights).tobytes() == three_steps["is_weight"].tobytes() and np.stack(grads).tobytes() == three_steps["grad"].tobytes()
    assert np.array(losses, np.float32).tobytes() == three_steps["loss"].tobytes()
    pri = wc.priorities(96)
    for s, beta in ((1, wc.BETA1 + 0.001), (2, (wc.BETA1 + 0.001) + 0.001)):
        stale = tc.is_weights(pri[slots[s]], beta).astype(np.float32)
        assert not np.array_equal(stale, three_steps["is_weight"][s])
    first = tc.is_weights(pri[slots[0]], wc.BETA1).astype(np.float32)
    assert (np.abs(three_steps["is_weight"][0] - first) <= np.spacing(first)).all()


# ---- duplicated slots ----

def test_slots_duplicated_across_tiles_carry_equal_bits_in_every_run(worlds):
    """A batch of 128 whose every slot sits in tiles 0 and 1: the same priority bytes in five runs, equal to the run where each slot
    appears once (a row's priority does not depend on the batch around it), and the other rows keep their bits."""
    twice, once = wc.every_slot_in_two_tiles()
    assert len(set(once.tolist())) == 64 and np.array_equal(twice[:64], twice[64:])
    runs = [_learn(worlds, _learner(1, 128), twice) for _ in range(5)]
    single = _learn(worlds, _learner(1, 64), once)
    worlds.check_error_flag()
    for r in runs[1:]:
        _same(r, runs[0])
    assert runs[0]["priority"].tobytes() == single["priority"].tobytes()
    pri = wc.priorities(96)
    rest = np.setdiff1d(np.arange(96), once)
    assert (runs[0]["priority"][once] != pri[once]).all() and runs[0]["priority"][rest].tobytes() == pri[rest].tobytes()


# ---- structure ----

def test_a_bad_slot_in_step_2_of_tile_3_is_flagged_and_that_brain_is_left_alone(worlds):
    """Learner 1 of two, batch 256, three steps, slot 96 (the ring's size) at row 200 of step 2: error-flag code 6 with the brain's index,
    the step and the value; nothing of that brain -- priorities, beta, is_weight and packed weights included -- is written; learner 0
    trains as it does alone."""
    import torch
    slots = np.stack([wc.slots_of(256, 3, seed=1), wc.slots_of(256, 3, seed=2)]).astype(np.int32)
    assert 200 // wc.TILE == 3
    slots[1, 2, 200] = 96
    a, b = _learner(3, 256), _learner(3, 256, sync_target=True, flat=(tc.golden()["init"] * np.float32(0.75)).astype(np.float32))
    before = _np(b)
    worlds.learn([a, b], 3, slots=slots)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 1, 2, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(b)
    _same(after, before)
    assert not after["grad"].any() and not after["is_weight"].any() and after["beta_is"][0] == 0.4 and after["state"].tolist() == [0, 0]
    ra = _np(a)
    solo = _learn(worlds, _learner(3, 256), slots[0], 3)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [3, 1]
    _same(ra, solo)


def test_a_call_below_the_size_gate_only_syncs_the_target(worlds):
    """size <= min_size (96 rows against a gate of 96): no update -- only target (synced), state[1] and packed (rewritten, to the same
    bits) move; priorities, beta and is_weight stay.  One row more trains."""
    p = tc.golden()
    slots = wc.slots_of(130)
    for sync in (True, False):
        l = _learner(1, 130, min_size=96, sync_target=sync)
        before = _np(l)
        after = _learn(worlds, l, slots)
        worlds.check_error_flag()
        _same(after, before, ("params", "adam_m", "adam_v", "packed", "priority", "beta_is", "is_weight", "loss", "grad"))
        assert after["state"].tolist() == [0, 1] and not after["grad"].any() and not after["is_weight"].any()
        assert after["target"].tobytes() == (before["params"] if sync else before["target"]).tobytes()
        assert after["packed"].tobytes() == _host_pack(p["init"]).tobytes()
    assert _learn(worlds, _learner(1, 130, min_size=95), slots)["state"].tolist() == [1, 1]
    worlds.check_error_flag()


def test_sixteen_learners_are_independent_and_runs_repeat(worlds):
    """Sixteen learners of one call, each with its own ring (the fixture rows rolled), parameters, priorities and slots, batch 96, two
    steps: every one ends as it does in a call of its own, and a second run repeats every byte."""
    g, p = dc.golden(), tc.golden()
    n = 16

    def make():
        out = []
        for i in range(n):
            rows = {k: np.ascontiguousarray(np.roll(g[k], 5 * i, axis=0)) for k in dc.RING_KEYS}
            out.append(_learner(2, 96, rows=rows, priority=wc.priorities(96, seed=20 + i), sync_target=i % 2 == 1,
                                flat=(p["init"] * np.float32(1 - i / 64)).astype(np.float32)))
        return out
    slots = np.stack([wc.slots_of(96, 2, seed=100 + i) for i in range(n)]).astype(np.int32)
    first, second = make(), make()
    worlds.learn(first, 2, slots=slots)
    worlds.learn(second, 2, slots=slots)
    ra, rb = [_np(l) for l in first], [_np(l) for l in second]
    worlds.check_error_flag()
    for i in (0, 7, 15):
        solo = _learn(worlds, make()[i], slots[i], 2)
        _same(ra[i], solo)
    worlds.check_error_flag()
    for i in range(n):
        _same(ra[i], rb[i])
        assert ra[i]["state"].tolist() == [2, 1] and (ra[i]["target"].tobytes() == ra[i]["params"].tobytes()) == (i % 2 == 1)
    assert len({r["params"].tobytes() for r in ra}) == n and len({r["priority"].tobytes() for r in ra}) == n


def test_device_packing_is_the_host_packing_bit_for_bit(three_steps):
    host = _host_pack(three_steps["params"])
    assert three_steps["packed"].tobytes() == host.tobytes() and host.tobytes() != _host_pack(tc.golden()["init"]).tobytes()


# ---- the draws ----

def _draw_learner(batch, wide, rows=48):
    """A learner on the first `rows` fixture rows with weights over several orders of magnitude, zeros included, rows to stamp (seen 20)
    and a call counter of 3."""
    l = _learner(1, batch, wide, count=rows, rows={k: dc.golden()[k][:rows] for k in dc.RING_KEYS}, priority=pc.edge_priorities(rows))
    l.seen.fill_(20)
    l.state[1] = 3
    return l


@pytest.mark.parametrize("ranked", [False, True], ids=["race", "rank"])
def test_the_wide_draws_at_batch_64_name_the_narrow_draws_slots(worlds, ranked):
    """Equal memories with rows to stamp: equal slot tables, priority, keys and seen -- the race draw, and the rank draw stratified and
    independent (also its order and cumulative sum)."""
    for stratified in ((True, False) if ranked else (None,)):
        out = []
        for wide in (True, False):
            l = _draw_learner(64, wide)
            before = worlds.launches
            slots = worlds.draw_td_rank([l], 2, stratified=stratified) if ranked else worlds.draw_td([l], 2)
            assert worlds.launches - before == (rk.PRIO_RANK_LAUNCHES if ranked else 2)
            out.append([slots.cpu().numpy(), l.priority.cpu().numpy(), l.keys.cpu().numpy(), l.seen.cpu().numpy()]
                       + ([l.rank_order.cpu().numpy(), l.rank_cum.cpu().numpy()] if ranked else []))
        worlds.check_error_flag()
        assert out[0][0].shape == (1, 2, 64) and int(out[0][3][0]) == 48
        for a, b in zip(*out):
            assert a.tobytes() == b.tobytes()
        assert (out[0][1][20:] == np.float32(tc.golden()["p_new"])).all()               # the fresh rows were stamped


@pytest.mark.parametrize("batch", [65, 2048])
def test_the_wide_race_draw_equals_the_host_restatement(worlds, batch):
    """Draw d = s * batch + j keeps its salt: the table of two steps is learn_perdqn_cases.host_draw's, slot for slot."""
    from reinlife_amd import _lib
    l = _draw_learner(batch, True)
    slots = worlds.draw_td([l], 2).cpu().numpy()
    worlds.check_error_flag()
    pri = tc.stamp(pc.edge_priorities(48), 20, 48, tc.golden()["p_new"])
    assert l.priority.cpu().numpy().tobytes() == pri.tobytes() and int(l.seen.item()) == 48
    keys = pc.content_keys(dc.golden(), 48)
    assert np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
    want, gaps = pc.host_draw64(keys, pri, SEED, 0, 3, 2 * batch, site=_lib.SITE_LEARN_TD)
    close = gaps < 1e-5                                                                  # (races logf's rounding could decide: none expected)
    print("wide race draw, batch %d: %d draws, %d with a relative gap below 1e-5" % (batch, 2 * batch, int(close.sum())))
    assert slots.shape == (1, 2, batch) and np.array_equal(slots.reshape(-1)[~close], want[~close]) and close.sum() <= 2
    assert np.array_equal(slots.reshape(-1), tc.host_draw(keys, pri, SEED, 0, 3, 2 * batch)) or close.any()


@pytest.mark.parametrize("stratified", [False, True], ids=["independent", "stratified"])
@pytest.mark.parametrize("batch", [65, 2048])
def test_the_wide_rank_draw_equals_the_host_restatement_and_keeps_its_strata(worlds, batch, stratified):
    """Order, cumulative sum (numpy's, in the header's association order) and every slot of two steps equal the host restatement; with
    stratified draws, draw j's target lies in segment j of `batch` segments of the total, exactly: the picked rank's interval of the
    cumulative sum meets [j, j + 1) * total / batch."""
    from reinlife_amd import _lib
    l = _draw_learner(batch, True)
    slots = worlds.draw_td_rank([l], 2, stratified=stratified).cpu().numpy()
    worlds.check_error_flag()
    pri = tc.stamp(pc.edge_priorities(48), 20, 48, tc.golden()["p_new"])
    keys = pc.content_keys(dc.golden(), 48)
    want, ranks, order, cum = rk.host_draw(keys, pri, SEED, 0, 3, _lib.SITE_LEARN_TD, 2, batch, stratified)
    assert l.rank_order.cpu().numpy()[:48].tobytes() == order.astype(np.int32).tobytes()
    assert l.rank_cum.cpu().numpy()[:48].tobytes() == cum.tobytes()
    assert slots.shape == (1, 2, batch) and np.array_equal(slots.reshape(-1), want) and (pri[want] > 0).all()
    if stratified:
        seg = cum[-1] / np.float64(batch)
        j = (np.arange(2 * batch) % batch).astype(np.float64)
        low = np.where(ranks > 0, cum[np.maximum(ranks - 1, 0)], 0.0)
        assert (cum[ranks] > j * seg).all() and (low <= (j + 1) * seg).all()
        assert (np.diff(ranks[:batch]) >= 0).all() and (np.diff(ranks[batch:]) >= 0).all()   # (the strata ascend with j)
    else:
        assert not (np.diff(ranks[:batch]) >= 0).all()


# ---- refusals ----

def test_the_c_abi_refuses_what_it_cannot_do(worlds):
    import torch
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    lib = _lib.lib()
    a, b, n = _learner(1, 130), _learner(1, 96), _learner(1, 64, wide=False)
    dev_slots = torch.zeros(2 * 2049, dtype=torch.int32, device=DEV)
    one = lambda l: ((_lib.Learner * 1)(l.struct()), (_lib.Replay * 1)(l.ring_struct()), (_lib.TdPrio * 1)(l.td_struct()))  # noqa: E731
    work = (C.c_void_p * 2)(a.work.data_ptr(), b.work.data_ptr())
    rank = lambda ls: [(C.c_void_p * len(ls))(*[t.data_ptr() for t in ts]) for ts in (  # noqa: E731
        [torch.zeros(96, dtype=torch.int32, device=DEV) for _ in ls], [torch.zeros(96, dtype=torch.float64, device=DEV) for _ in ls],
        [torch.empty(int(lib.rl_learn_prio_draw_rank_work_bytes(96)), dtype=torch.uint8, device=DEV) for _ in ls])]
    # batch 0 / 2049
    for batch in (0, 2049):
        a.batch = batch
        arr, rings, tds = one(a)
        assert lib.rl_learn_td_wide(worlds.handle, arr, rings, tds, 1, 1, dev_slots.data_ptr(), work, None) == -1
        assert b"rl_learn_td_wide: learner 0: batch must be in [1,2048] (got %d)" % batch in lib.rl_last_error()
        assert lib.rl_learn_td_wide_draw(worlds.handle, arr, rings, tds, 1, 1, dev_slots.data_ptr(), None) == -1
        assert b"rl_learn_td_wide_draw: learner 0: batch must be in [1,2048]" in lib.rl_last_error()
        assert lib.rl_learn_td_wide_draw_rank(worlds.handle, arr, rings, tds, 1, 1, 1, *rank([a]), dev_slots.data_ptr(), None) == -1
        assert b"rl_learn_td_wide_draw_rank: learner 0: batch must be in [1,2048]" in lib.rl_last_error()
    a.batch = 130
    # unequal batches in one call
    arr, rings = (_lib.Learner * 2)(a.struct(), b.struct()), (_lib.Replay * 2)(a.ring_struct(), b.ring_struct())
    tds = (_lib.TdPrio * 2)(a.td_struct(), b.td_struct())
    assert lib.rl_learn_td_wide(worlds.handle, arr, rings, tds, 2, 1, dev_slots.data_ptr(), work, None) == -1
    assert b"rl_learn_td_wide: learner 1: batch 96 differs from learner 0's 130" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw(worlds.handle, arr, rings, tds, 2, 1, dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_td_wide_draw: learner 1: batch 96 differs" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw_rank(worlds.handle, arr, rings, tds, 2, 1, 0, *rank([a, b]), dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_td_wide_draw_rank: learner 1: batch 96 differs" in lib.rl_last_error()
    # null work[i], null slots
    arr, rings, tds = one(a)
    assert lib.rl_learn_td_wide(worlds.handle, arr, rings, tds, 1, 1, dev_slots.data_ptr(), (C.c_void_p * 1)(), None) == -1
    assert b"work[0] must not be null (rl_learn_td_wide_work_bytes)" in lib.rl_last_error()
    assert lib.rl_learn_td_wide(worlds.handle, arr, rings, tds, 1, 1, None, work, None) == -1
    assert b"slots must not be null -- the minibatches of a prioritised memory are drawn by rl_learn_td_wide_draw" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw(worlds.handle, arr, rings, tds, 1, 1, None, None) == -1 and b"slots must not be null" in lib.rl_last_error()
    # a kind that is not RL_PERDQN
    d = DeviceLearner(Models.DQN(max_epi=60), DEV, ring=_ring(dc.golden()))
    darr, drings = (_lib.Learner * 1)(d.struct()), (_lib.Replay * 1)(d.ring_struct())
    assert lib.rl_learn_td_wide(worlds.handle, darr, drings, tds, 1, 1, dev_slots.data_ptr(), work, None) == -4
    assert b"kind %d" % _lib.DQN in lib.rl_last_error() and b"RL_PERDQN (4) only (rl_learn_td_wide_supported)" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw(worlds.handle, darr, drings, tds, 1, 1, dev_slots.data_ptr(), None) == -4 and b"kind %d" % _lib.DQN in lib.rl_last_error()
    # rl_learn_td and the narrow draws still refuse 65
    n.batch = 65
    arr, rings, tds = one(n)
    assert lib.rl_learn_td(worlds.handle, arr, rings, tds, 1, 1, dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_td: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    assert lib.rl_learn_td_draw(worlds.handle, arr, rings, tds, 1, 1, dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_td_draw: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    assert lib.rl_learn_td_draw_rank(worlds.handle, arr, rings, tds, 1, 1, 1, *rank([n]), dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_td_draw_rank: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    torch.cuda.synchronize()
    worlds.check_error_flag()


def test_the_python_layer_refuses_mixed_calls(worlds):
    from reinlife_amd import _lib
    a, b, n = _learner(1, 130), _learner(1, 96), _learner(1, 64, wide=False)
    table = np.zeros((2, 1, 130), np.int32)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([a, n], 1, slots=table)
    with pytest.raises(ValueError, match="one kind"):
        worlds.draw_td([_learner(1, 64), n], 1)
    with pytest.raises(ValueError, match="one kind"):
        worlds.draw_td_rank([_learner(1, 64), n], 1)
    with pytest.raises(ValueError, match="share one batch"):
        worlds.draw_td([a, b], 1)
    with pytest.raises(ValueError, match=r"slots must hold \[n_learners, n_steps, batch\]"):
        worlds.learn([a, b], 1, slots=table)                                             # (a table is rectangular: one batch)
    with pytest.raises(ValueError, match="share one batch size, got \\[96, 130\\]"):
        worlds.learn([a, b], 1)
    with pytest.raises(_lib.ReinLifeHipError, match="rl_learn_td_wide_draw"):
        worlds.learn([a], 1)                                                             # no slots: the draw is draw_td()'s job
    worlds.check_error_flag()


# ---- the whole path: trainer(learn="device", learn_td_priority=True, learn_batch={"PERDQN": B}) ----
_runs = {}


def _train(fresh=False, **kw):
    """trainer([PERDQN, DQN], 40 episodes, 2 worlds, train_start 200, learn_td_priority=True): tests/test_hip_learn_perdqn.py's run -- the
    PERDQN trains after episodes 20 and 40, one update each.  Made once per keyword set unless fresh."""
    import torch
    from reinlife_amd import Models, trainer
    key = tuple(sorted((k, str(v)) for k, v in kw.items()))
    if not fresh and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.PERDQN(), Models.DQN(max_epi=60)]
    brains[0].train_start = 200
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=40, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device", save=False,
                      print_results=False, learn_td_priority=True, **kw)
    count, capacity = int(env.worlds.replays[0]["count"].item()), int(env.worlds.replays[0]["state"].shape[0])
    assert 200 <= count < capacity == 20000, (count, capacity)   # (no wrap: the rows a draw sees do not depend on append order)
    if not fresh:
        _runs[key] = env
    return env


def _bits(env):
    """The learners' buffers as bytes; the priorities sorted (the rows' slots differ from run to run, their priorities do not)."""
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, l in env.learners.items():
        out[k] = {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS}
        if getattr(l, "priority", None) is not None:
            out[k]["priority"] = np.sort(l.priority.cpu().numpy()).tobytes()
            out[k]["beta_is"] = l.beta_is.cpu().numpy().tobytes()
            out[k]["seen"] = l.seen.cpu().numpy().tobytes()
    return out


def test_learn_batch_perdqn_needs_learn_td_priority_before_a_device_is_touched(monkeypatch):
    from reinlife_amd import Environment, Models, worlds as worlds_module
    monkeypatch.setattr(worlds_module, "DeviceWorlds", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=r"takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them, got \{'PERDQN': 96\}$"):
        Environment(brains=[Models.PERDQN(), Models.DQN(max_epi=60)], n_worlds=2, learn="device", learn_batch={"PERDQN": 96})


def test_learn_batch_perdqn_64_is_the_run_without_the_key():
    env, env64 = _train(), _train(learn_batch={"PERDQN": 64})
    assert [env.learners[k].entry for k in (0, 1)] == ["rl_learn_td", "rl_learn"]
    assert [env64.learners[k].entry for k in (0, 1)] == ["rl_learn_td_wide", "rl_learn"]
    assert env.learn_batch is None and env64.learn_batch == {"PERDQN": 64}
    assert env.learners[0].state.cpu().tolist() == env64.learners[0].state.cpu().tolist() == [2, 2]
    assert _bits(env) == _bits(env64) and env.tracker.results == env64.tracker.results
    assert env64.worlds.launches - env.worlds.launches == 2 * (wc.launches(1) - 1)
    assert env.brains[0].epsilon == env64.brains[0].epsilon < 1.0


def test_learn_batch_perdqn_96_trains_and_repeats():
    from reinlife_amd import _lib
    env = _train(learn_batch={"PERDQN": 96})
    l = env.learners[0]
    assert l.entry == "rl_learn_td_wide" and l.batch == 96 and l.min_size == 199 and l.state.cpu().tolist() == [2, 2] and l.trained_from
    seen, pri = int(l.seen.item()), l.priority.cpu().numpy()
    changed = int((pri[:seen] != np.float32(l.p_new)).sum())
    print("PERDQN at batch 96: seen %d, beta %.17g, rows re-prioritised %d" % (seen, l.beta_is.item(), changed))
    assert 96 < changed <= 192 and (pri[:seen] > 0).all() and not pri[seen:].any() and l.beta_is.item() == (0.4 + 0.001) + 0.001
    now = env.brains[0].state_dict_flat()
    assert np.isfinite(now).all() and now.tobytes() == l.params.cpu().numpy().tobytes() == l.target.cpu().numpy().tobytes()
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes() and env.worlds._brain_keep[0].data_ptr() == l.packed.data_ptr()
    assert _bits(env)[0]["params"] != _bits(_train(learn_batch={"PERDQN": 64}))[0]["params"]   # a wider batch is another update
    note = env._weights_note()
    assert "rl_learn_td_wide" in note and "batch 96" in note and "rl_learn:" in note and _lib.LEARN_TD_WIDE_MAX == 2048
    again = _train(fresh=True, learn_batch={"PERDQN": 96})
    assert _bits(env) == _bits(again) and env.tracker.results == again.tracker.results and env.worlds.launches == again.worlds.launches
    env.worlds.check_error_flag()


def test_with_the_stamp_and_the_rank_draw_the_queued_launches_are_the_notes(monkeypatch):
    """learn_batch={"PERDQN": 96} with learn_td_stamp="error" and learn_draw={"PERDQN": "rank"}: every PERDQN call is stamp_td (2 launches),
    draw_td_rank (8, through rl_learn_td_wide_draw_rank, stratified at 96) and learn (3 + 3); the DQN calls are what they were."""
    from reinlife_amd.worlds import DeviceWorlds
    log = []
    for name in ("stamp_td", "draw_td", "draw_td_rank", "draw_slots", "learn"):
        def wrap(original, name):
            def watched(self, learners, *a, **k):
                before = self.launches
                out = original(self, learners, *a, **k)
                log.append((name, [l.entry for l in learners], self.launches - before))
                return out
            return watched
        monkeypatch.setattr(DeviceWorlds, name, wrap(getattr(DeviceWorlds, name), name))
    kw = dict(learn_td_stamp="error", learn_draw={"PERDQN": "rank"})
    env = _train(fresh=True, learn_batch={"PERDQN": 96}, **kw)
    monkeypatch.undo()
    td = [c for c in log if c[1] == ["rl_learn_td_wide"]]
    assert td == [("stamp_td", ["rl_learn_td_wide"], 2), ("draw_td_rank", ["rl_learn_td_wide"], 8), ("learn", ["rl_learn_td_wide"], 6)] * 2
    assert [c for c in log if c[1] != ["rl_learn_td_wide"]] == [("draw_slots", ["rl_learn"], 2), ("learn", ["rl_learn"], 1)] * 2
    l = env.learners[0]
    assert l.state.cpu().tolist() == [2, 2] and l.rank_cum is not None
    assert not (l.priority.cpu().numpy().view(np.uint32) == np.float32(l.p_new).view(np.uint32)).any()   # the ring holds no p_new
    note = env._weights_note()
    assert "rl_learn_td_wide:" in note and "rl_learn_td_wide_draw_rank" in note and "rl_learn_td_stamp" in note and "learn_td_stamp='error'" in note
    narrow = _train(**kw)
    assert env.worlds.launches - narrow.worlds.launches == 2 * (wc.launches(1) - 1)
    env.worlds.check_error_flag()


def test_learn_batch_perdqn_96_under_the_identity_merge():
    """learn_ranks="average" on one rank without a process group: export, merge and repack after every learning episode change no bit."""
    env, envm = _train(learn_batch={"PERDQN": 96}), _train(learn_batch={"PERDQN": 96}, learn_ranks="average")
    assert envm.learn_ranks == "average" and envm.learn_now_calls == env.learn_now_calls == 2
    assert _bits(env) == _bits(envm) and env.tracker.results == envm.tracker.results
