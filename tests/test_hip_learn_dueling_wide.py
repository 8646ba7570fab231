"""GPU: rl_learn_dueling_wide / DeviceLearner(dueling_batch=) / trainer(learn_batch={"D3QN": B}) -- the D3QN update of
ReinLife/Models/D3QN.py:97-116, 148-165 on minibatches of several 64-row tiles with the advantage mean of the WHOLE batch: one tile is
rl_learn_dueling bit for bit, several tiles against torch float64 autograd (the test a per-tile mean fails:
tests/test_learn_dueling_wide_cpu.py shows by how much), Adam replayed from the kernel's own gradients, packing, sync_target, the gate,
repeatability, independence of the learners of a launch, the checked bad slot, and the whole path through trainer().  Every figure a bar
is held against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_dueling_wide_cases as wc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = wc.LR, wc.GAMMA
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
ALL = BUFFERS + ("grad", "loss")


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


def _learner(n_steps, batch, wide=True, ring=None, flat=None, sync_target=False, moments=False, min_size=0, steps_taken=0):
    """A D3QN learner on the fixture (wide: through rl_learn_dueling_wide) with grad and loss rows; the gate is open unless min_size says
    otherwise; moments=True starts from learn_d3qn_cases.adam_moments."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    g = dc.golden()
    l = DeviceLearner(_brain(g["init"] if flat is None else flat), DEV, ring=_ring(g) if ring is None else ring, **({"dueling_batch": batch} if wide else {}))
    assert l.entry == ("rl_learn_dueling_wide" if wide else "rl_learn_dueling")
    assert (l.lr, l.gamma, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (LR, GAMMA, 63, 20, 1, False)
    assert (l.exploration, l.soft_update_freq) == (1000, 200)
    if wide:
        assert l.batch == batch and l.work.numel() == wc.work_bytes(batch) and l.work.data_ptr() % 16 == 0
        l.work.fill_(0xA5)   # the work buffer needs no initialisation
    else:
        assert l.work is None
    l.batch, l.min_size, l.sync_target = batch, min_size, sync_target
    l.target.copy_(torch.as_tensor(np.array(g["target_init"], np.float32), device=DEV))
    if moments:
        m0, v0 = dc.adam_moments(dc.N_PARAMS)
        l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
        l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
    if steps_taken:
        l.state[0] = steps_taken
    l.grad = torch.zeros((n_steps, dc.N_PARAMS), dtype=torch.float32, device=DEV)
    l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    out = {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS}
    out["grad"], out["loss"] = l.grad.cpu().numpy().copy(), l.loss.cpu().numpy().copy()
    return out


def _same(a, b, keys=ALL):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


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


# ---- one tile is rl_learn_dueling, bit for bit ----

@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("batch", [1, 5, 33, 64])
def test_one_tile_is_rl_learn_dueling_bit_for_bit(worlds, batch, moments):
    """Three steps on the wrapped fixture ring (capacity 96, count 250), explicit slots, from fresh moments and from moments under way,
    once with the target copy: params, adam_m, adam_v, target, state, packed, loss and grad of rl_learn_dueling_wide are those of
    rl_learn_dueling from the same start."""
    g = dc.golden()
    slots = np.ascontiguousarray(g["slots"][:, :batch]).astype(np.int32).reshape(1, 3, batch)
    sync = batch == 33
    mk = lambda wide: _learner(3, batch, wide=wide, ring=_ring(g, count=250), moments=moments, sync_target=sync, min_size=batch - 1)  # noqa: E731
    a, b = mk(True), mk(False)
    worlds.learn([a], 3, slots=slots)
    worlds.learn([b], 3, slots=slots)
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [3, 1] and rb["grad"].any() and (rb["loss"] > 0).all()
    assert rb["params"].tobytes() != np.asarray(g["init"]).tobytes()
    assert (rb["target"].tobytes() == rb["params"].tobytes()) == sync
    _same(ra, rb)


def test_one_tile_with_the_philox_draw_is_rl_learn_dueling_bit_for_bit(worlds):
    """slots == NULL at batch 64, two steps: row j of step s takes draw index s * 64 + j, rl_learn_dueling's mapping."""
    from reinlife_amd.learn import philox_slots
    a, b, c = _learner(2, 64, wide=True), _learner(2, 64, wide=False), _learner(2, 64, wide=True)
    worlds.learn([a], 2)
    worlds.learn([b], 2)
    worlds.learn([c], 2, slots=philox_slots(SEED, 0, 0, 2, 64, 96).reshape(1, 2, 64))
    ra, rb, rc = _np(a), _np(b), _np(c)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [2, 1] and rb["grad"].any()
    _same(ra, rb)
    _same(ra, rc)


# ---- several tiles against float64 autograd ----

def _check_against_float64(tag, l, loss64, g64):
    got = dc.split(l.grad[0].cpu().numpy())
    loss = float(l.loss[0].item())
    print("%s: loss %.9g (float64 %.9g, relative error %.3g)" % (tag, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(dc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("%s: %-17s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (tag, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("%s: worst gradient error / max|g| = %.3g (bar 1e-5)" % (tag, worst))
    for name, a, b in zip(dc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


@pytest.mark.parametrize("batch", wc.MULTI_TILE_BATCHES)
def test_several_tiles_match_float64_autograd(worlds, batch):
    """One step on the 96-row fixture ring, rows drawn with replacement: a second tile with one live row (65), a half tile (96), full
    tiles (128), a ragged third tile (130) and 32 tiles (2048).  Every gradient tensor within 1e-5 of its largest magnitude of torch
    float64 autograd of the reference's loss -- the mean over the whole batch --, exact zeros where float64 has them, the loss within
    1e-5: rl_learn_dueling's bar.  Tiles that each take their own mean miss it 400 to 2000 times over (tests/test_learn_dueling_wide_cpu.py)."""
    import torch
    slots, loss64, g64 = wc.case(batch)
    assert len(slots) == batch and len(set(slots.tolist())) < batch
    by = dict(zip(dc.NAMES, g64))
    assert (by["fc.weight"][:, 3::10] == 0).all() and (by["adv_fc1.bias"] == 0).any()
    l = _learner(1, batch)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    _check_against_float64("batch %d" % batch, l, loss64, g64)
    assert l.state.cpu().tolist() == [1, 1]
    assert l.target.cpu().numpy().tobytes() == dc.golden()["target_init"].tobytes()
    assert l.packed.cpu().numpy().tobytes() == _host_pack(l.params.cpu().numpy()).tobytes()


# ---- Adam ----

def test_adam_over_three_wide_steps_matches_torch_formula_on_the_kernels_own_gradients(worlds):
    """Batch 130, three steps: torch.optim.Adam replayed in numpy float64 from the kernel's own gradient rows, parameters and moments
    rounded to float32 between the steps as torch keeps them -- every parameter within 1e-5 lr + 1 ulp, moments within 1e-5 of their
    maxima; the second and third steps read the parameters the steps before them left (their gradients are float64 autograd's at those
    parameters); the counters, the untouched target and the packed weights as rl_learn_dueling leaves them."""
    g = dc.golden()
    slots = wc.slots_of(130, 3, seed=7)
    l = _learner(3, 130)
    worlds.learn([l], 3, slots=slots.reshape(1, 3, 130))
    r = _np(l)
    worlds.check_error_flag()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v = g["init"].astype(np.float64), np.zeros(dc.N_PARAMS), np.zeros(dc.N_PARAMS)
    for t in range(1, 4):
        gt = r["grad"][t - 1].astype(np.float64)
        assert gt.any()
        if t == 2:   # n_steps = 2 and beyond: this step's gradient is taken at the parameters step 1 left, not at the initial ones
            loss64, g64 = dc.grads64(p.astype(np.float32), g["target_init"], g, slots[1], GAMMA)
            worst = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(dc.split(gt), g64))
            loss0, g0 = dc.grads64(g["init"], g["target_init"], g, slots[1], GAMMA)
            stale = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(dc.split(gt), g0))
            print("step 2 gradient: against float64 at step 1's parameters %.3g (bar 1e-5), at the initial parameters %.3g" % (worst, stale))
            assert worst <= 1e-5 < stale and abs(float(r["loss"][1]) - loss64) <= 1e-5 * loss64
        p, m, v = (f32(x) for x in dc.adam64(p, m, v, gt, t, LR))
    err = np.abs(r["params"].astype(np.float64) - p)
    bound = 1e-5 * LR + np.spacing(np.abs(r["params"])).astype(np.float64)
    em, ev = np.abs(r["adam_m"] - m).max() / np.abs(m).max(), np.abs(r["adam_v"] - v).max() / np.abs(v).max()
    print("Adam, batch 130 x 3: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g "
          "(relative to their maxima)" % (err.max(), 1e-5 * LR, (err / bound).max(), em, ev))
    assert (err <= bound).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert r["state"].tolist() == [3, 1]
    assert r["target"].tobytes() == g["target_init"].tobytes() and r["params"].tobytes() != g["init"].tobytes()
    assert r["packed"].tobytes() == _host_pack(r["params"]).tobytes() != _host_pack(g["init"]).tobytes()
    assert np.isfinite(r["loss"]).all() and (r["loss"] > 0).all()


def test_adam_at_step_ten_thousand_on_moments_that_are_not_zero(worlds):
    """Batch 130, state[0] = 9999, moments from learn_d3qn_cases.adam_moments, one step: every parameter within 1e-5 lr + 1 ulp of
    adam64(p, m, v, kernel_grad, t = 10000), m and v within 1e-5 of their maxima (and within 1 ulp), state [10000, 1]."""
    g = dc.golden()
    m0, v0 = dc.adam_moments(dc.N_PARAMS)
    slots = wc.case(130)[0]
    l = _learner(1, 130, moments=True, steps_taken=9999)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, 130))
    r = _np(l)
    worlds.check_error_flag()
    grad = r["grad"][0].astype(np.float64)
    p64, m64, v64 = dc.adam64(g["init"].astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), grad, 10000, LR)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    perr, bound = np.abs(r["params"] - p64), 1e-5 * LR + ulp(r["params"])
    merr, verr = np.abs(r["adam_m"] - m64) / ulp(m64), np.abs(r["adam_v"] - v64) / ulp(v64)
    print("wide D3QN Adam at t = 10000: worst |p - float64| / (1e-5 lr + 1 ulp) %.3g (largest step %.3g lr); m: worst %.3g ulp; v: worst %.3g ulp"
          % ((perr / bound).max(), (np.abs(p64 - g["init"]) / LR).max(), merr.max(), verr.max()))
    assert r["state"].tolist() == [10000, 1] and grad.any()
    assert (perr <= bound).all()
    assert np.abs(r["adam_m"] - m64).max() <= 1e-5 * np.abs(m64).max() and np.abs(r["adam_v"] - v64).max() <= 1e-5 * np.abs(v64).max()
    assert (merr <= 1).all() and (verr <= 1).all()


# ---- the rest of the contract ----

def test_sync_target_copies_the_parameters_only_when_asked(worlds):
    slots = wc.slots_of(130, 2, seed=5).reshape(1, 2, 130)
    off, on = _learner(2, 130), _learner(2, 130, sync_target=True)
    worlds.learn([off], 2, slots=slots)
    worlds.learn([on], 2, slots=slots)
    r0, r1 = _np(off), _np(on)
    worlds.check_error_flag()
    assert r0["target"].tobytes() == dc.golden()["target_init"].tobytes()
    assert r1["target"].tobytes() == r1["params"].tobytes() != dc.golden()["target_init"].tobytes()
    _same(r0, r1, keys=("params", "adam_m", "adam_v", "state", "packed", "grad", "loss"))   # the same update, and the copy afterwards


@pytest.mark.parametrize("sync", [False, True])
def test_below_the_size_gate_nothing_trains_but_the_call_is_counted(worlds, sync):
    """A ring of min_size rows trains nothing: every buffer but state[1] (and, where asked, the target) stays; one more row trains."""
    g = dc.golden()
    l = _learner(2, 130, ring=_ring(g, count=63), min_size=63, sync_target=sync)
    before = _np(l)
    worlds.learn([l], 2)
    after = _np(l)
    worlds.check_error_flag()
    assert worlds.err.cpu().tolist()[0] == 0
    for k in ("params", "adam_m", "adam_v", "packed", "grad", "loss"):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["state"].tolist() == [0, 1]
    assert after["target"].tobytes() == (before["params"] if sync else before["target"]).tobytes()
    from reinlife_amd.learn import philox_slots
    a = _learner(2, 130, ring=_ring(g, count=64), min_size=63)
    b = _learner(2, 130, ring=_ring(g, count=64), min_size=63)
    slots = philox_slots(SEED, 0, 0, 2, 130, 64)
    assert slots.shape == (2, 130) and slots.max() < 64
    worlds.learn([a], 2)
    worlds.learn([b], 2, slots=slots.reshape(1, 2, 130))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [2, 1] and ra["grad"].any()
    _same(ra, rb)


def test_runs_repeat_and_the_last_of_sixteen_learners_is_the_learner_alone(worlds):
    """The same call twice gives the same bits; the last learner of a 16-learner call (batch 130, two steps) ends as it does alone."""
    g = dc.golden()
    slots = wc.slots_of(130, 2, seed=21)
    a, b = _learner(2, 130), _learner(2, 130)
    worlds.learn([a], 2, slots=slots.reshape(1, 2, 130))
    worlds.learn([b], 2, slots=slots.reshape(1, 2, 130))
    ra, rb = _np(a), _np(b)
    _same(ra, rb)
    others = [_learner(2, 130, flat=(g["init"] * np.float32(1.0 - 0.01 * i)).astype(np.float32)) for i in range(1, 16)]
    c = _learner(2, 130)
    table = np.stack([wc.slots_of(130, 2, seed=30 + i) for i in range(15)] + [slots]).astype(np.int32)
    worlds.learn(others + [c], 2, slots=table)
    rc, r0 = _np(c), _np(others[0])
    worlds.check_error_flag()
    _same(ra, rc)
    assert ra["state"].tolist() == [2, 1] and r0["state"].tolist() == [2, 1] and r0["params"].tobytes() != ra["params"].tobytes()


def test_a_bad_slot_in_the_last_tile_of_the_last_step_is_flagged_and_that_brain_is_left_alone(worlds):
    """Batch 130, two steps, -1 at the very last table index (the third tile's second row, step 1): error-flag code 6 with the learner,
    the step and the value; none of that learner's buffers is written -- packed, which does not match its params here, included -- and
    the healthy learner of the same call trains as it does alone.  (The check pass reads the table's VALUES before any row is fetched.)"""
    import torch
    good = wc.slots_of(130, 2, seed=31)
    bad = good.copy()
    bad[1, 129] = -1
    healthy, broken = _learner(2, 130), _learner(2, 130, sync_target=True)
    broken.packed.mul_(0.5)
    broken.adam_m.fill_(0.25)
    before = _np(broken)
    worlds.err.zero_()
    worlds.learn([healthy, broken], 2, slots=np.stack([good, bad]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 1, 1, -1]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    _same(_np(broken), before)
    assert not broken.grad.any().item() and not broken.loss.any().item()
    solo = _learner(2, 130)
    worlds.learn([solo], 2, slots=good.reshape(1, 2, 130))
    rh, rs = _np(healthy), _np(solo)
    worlds.check_error_flag()
    assert rh["state"].tolist() == [2, 1] and rh["params"].tobytes() != dc.golden()["init"].tobytes()
    _same(rh, rs)


def test_mixed_batches_mixed_entries_and_perd3qn_are_refused(worlds):
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    g = dc.golden()
    a, b = _learner(1, 130), _learner(1, 96)
    with pytest.raises(ValueError, match="share one batch"):
        worlds.learn([a, b], 1)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([a, _learner(1, 64, wide=False)], 1)
    with pytest.raises(ValueError, match="dueling_batch is for D3QN brains"):
        DeviceLearner(Models.PERD3QN(), DEV, ring=_ring(g), dueling_batch=130)
    # ... and at the C entry point: a PERD3QN learner's structures with a work buffer
    p = DeviceLearner(Models.PERD3QN(), DEV, ring=_ring(g), prioritized=True)
    p.batch = 130
    arr, rings = (_lib.Learner * 1)(p.struct()), (_lib.Replay * 1)(p.ring_struct())
    work = (C.c_void_p * 1)(a.work.data_ptr())
    rc = _lib.lib().rl_learn_dueling_wide(worlds.handle, arr, rings, 1, 1, None, work, None)
    assert rc == -4 and b"kind %d" % _lib.PERD3QN in _lib.lib().rl_last_error()
    arr = (_lib.Learner * 2)(a.struct(), b.struct())
    rings = (_lib.Replay * 2)(a.ring_struct(), b.ring_struct())
    work = (C.c_void_p * 2)(a.work.data_ptr(), b.work.data_ptr())
    rc = _lib.lib().rl_learn_dueling_wide(worlds.handle, arr, rings, 2, 1, None, work, None)
    assert rc == -1 and b"batch 96 differs" in _lib.lib().rl_last_error()


def test_draws_take_a_wide_dueling_learners_batch(worlds):
    """draw_slots and draw_slots_rank for a batch-130 learner: [1, 2, 130] inside the ring, and training on them repeats."""
    import torch
    a, b = _learner(2, 130), _learner(2, 130)
    for draw in (worlds.draw_slots, worlds.draw_slots_rank):
        sa, sb = draw([a], 2), draw([b], 2)
        torch.cuda.synchronize()
        assert tuple(sa.shape) == (1, 2, 130) and sa.dtype == torch.int32 and int(sa.min()) >= 0 and int(sa.max()) < 96
        assert torch.equal(sa, sb)
    worlds.learn([a], 2, slots=sa)
    worlds.learn([b], 2, slots=sb)
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [2, 1]
    _same(ra, rb)


# ---- the whole path: trainer(learn="device", learn_kinds=("DQN", "D3QN"), learn_batch={...}) ----
_runs = {}


def _train(tmp=None, exploration=20, **kw):
    """One short trainer() run of a DQN and a D3QN brain on 2 synthetic worlds (exploration 20, soft_update_freq 40, learn_every 20: the
    D3QN trains after episodes 40 and 60, its target synced at 40); runs without a folder to save into are made once per keyword set."""
    import torch
    from reinlife_amd import Models, trainer
    key = tuple(sorted((k, tuple(sorted(v.items())) if isinstance(v, dict) else v) for k, v in kw.items())) + (exploration,)
    if tmp is None and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.D3QN(exploration=exploration, soft_update_freq=40)]
    init = [b.state_dict_flat().copy() for b in brains]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=60, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      learn_kinds=("DQN", "D3QN"), save=tmp is not None, print_results=False, **kw)
    count, capacity = int(env.worlds.replays[1]["count"].item()), int(env.worlds.replays[1]["state"].shape[0])
    assert 64 <= count < capacity == 10000, (count, capacity)   # (no wrap: the rows a draw sees do not depend on append order)
    out = (env, brains, init)
    if tmp is None:
        _runs[key] = out
    return out


def _learner_bits(env):
    import torch
    torch.cuda.synchronize()
    return {k: {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS} for k, l in env.learners.items()}


def _equal_learners(a, b, keys=None):
    ba, bb = _learner_bits(a), _learner_bits(b)
    assert sorted(ba) == sorted(bb) == [0, 1]
    for k in (keys or ba):
        for n in BUFFERS:
            assert ba[k][n] == bb[k][n], (k, n)


def test_learn_batch_d3qn_64_is_the_run_without_the_keyword():
    """The draw table is the same and a one-tile call is rl_learn_dueling: bit-identical learners and Tracker results."""
    env, _, _ = _train()
    env64, _, _ = _train(learn_batch={"D3QN": 64})
    assert [env.learners[k].entry for k in (0, 1)] == ["rl_learn", "rl_learn_dueling"]
    assert [env64.learners[k].entry for k in (0, 1)] == ["rl_learn", "rl_learn_dueling_wide"]
    assert env.learn_batch is None and env64.learn_batch == {"D3QN": 64} and type(env64.learn_batch) is dict
    assert env.learners[1].state.cpu().tolist() == env64.learners[1].state.cpu().tolist() == [2, 2]
    _equal_learners(env, env64)
    assert env.tracker.results == env64.tracker.results


def test_learn_batch_d3qn_130_trains_saves_and_repeats(tmp_path, monkeypatch):
    import torch
    env, brains, init = _train(learn_batch={"D3QN": 130})
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    l = env.learners[1]
    assert l.entry == "rl_learn_dueling_wide" and l.batch == 130 and l.min_size == 63 and l.state.cpu().tolist() == [2, 2]
    assert env.worlds.replays[1]["state"].shape[0] == brains[1].capacity == 10000 and env.worlds.replays[0]["state"].shape[0] == 50000
    now, target = brains[1].state_dict_flat(), l.target.cpu().numpy()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1]) and now.tobytes() == l.params.cpu().numpy().tobytes()
    assert not np.array_equal(target, init[1]) and not np.array_equal(target, now)       # synced at 40, not at 60
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes()                  # what the worlds acted with
    assert env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()
    env64, brains64, _ = _train(learn_batch={"D3QN": 64})
    assert brains64[1].state_dict_flat().tobytes() != now.tobytes()                       # a wider batch is another update
    note = env._weights_note()
    assert "rl_learn_dueling_wide" in note and "batch 130" in note and "rl_learn:" in note
    # a second identical call gives the same parameters
    monkeypatch.chdir(tmp_path)
    env2, brains2, init2 = _train(tmp=tmp_path, learn_batch={"D3QN": 130})
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    # save=True wrote the trained weights, and settings.json names the keyword and the entry point
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "D3QN", "brain_gene_*.pt")))
    assert len(files) == 1
    flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(files[0]).values()])
    assert flat.tobytes() == brains2[1].state_dict_flat().tobytes() and not np.array_equal(flat, init2[1])
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_dueling_wide" in settings and '"Learn batch": {"D3QN": 130}' in settings.replace("\n", "").replace("  ", "")


def test_learn_batch_d3qn_130_with_the_rank_draw_and_the_identity_merge():
    """learn_draw="rank": another sampler, so other parameters, and the same bits in a second run; learn_ranks="average" on one rank
    without a process group: export, merge and repack after every learning episode change no bit."""
    env, brains, _ = _train(learn_batch={"D3QN": 130})
    envr, brainsr, initr = _train(learn_batch={"D3QN": 130}, learn_draw="rank")
    assert envr.learners[1].entry == "rl_learn_dueling_wide" and envr.learners[1].state.cpu().tolist() == [2, 2]
    now = brainsr[1].state_dict_flat()
    assert np.isfinite(now).all() and not np.array_equal(now, initr[1]) and now.tobytes() != brains[1].state_dict_flat().tobytes()
    envr64, brainsr64, _ = _train(learn_batch={"D3QN": 64}, learn_draw="rank")
    assert brainsr64[1].state_dict_flat().tobytes() != now.tobytes()                     # ... and differs from batch 64 on the same sampler
    _runs.pop(next(k for k in _runs if ("learn_draw", "rank") in k and ("learn_batch", (("D3QN", 130),)) in k))   # (made again, not taken from the cache)
    envr2, _, _ = _train(learn_batch={"D3QN": 130}, learn_draw="rank")
    _equal_learners(envr, envr2)
    envm, _, _ = _train(learn_batch={"D3QN": 130}, learn_ranks="average")
    assert envm.learn_ranks == "average" and envm.learn_now_calls == env.learn_now_calls == 3
    _equal_learners(env, envm)
    assert env.tracker.results == envm.tracker.results


def test_learn_batch_by_kind_gives_the_dqn_learner_the_bits_of_the_int():
    """{"DQN": 96, "D3QN": 130} on the mixed list: the DQN learner ends with the bits learn_batch=96 gives it.  The agents of both
    brains share the worlds, so a D3QN that trains on another batch acts differently and changes the rows the DQN learner sees; the
    comparison is therefore made where the D3QN learner is built but not yet called (exploration 1000 > 60 episodes), so that the DQN
    learner's rows are the same in both runs.  With exploration 20 both learners train and are wide."""
    both, brains, init = _train(exploration=1000, learn_batch={"DQN": 96, "D3QN": 130})
    dqn, _, _ = _train(exploration=1000, learn_batch=96)
    assert [both.learners[k].entry for k in (0, 1)] == ["rl_learn_wide", "rl_learn_dueling_wide"]
    assert [dqn.learners[k].entry for k in (0, 1)] == ["rl_learn_wide", "rl_learn_dueling"] and dqn.learn_batch == 96
    assert both.learn_batch == {"DQN": 96, "D3QN": 130} and (both.learners[0].batch, both.learners[1].batch) == (96, 130)
    assert both.learners[0].state.cpu().tolist()[0] > 0 and both.learners[1].state.cpu().tolist() == [0, 0]
    assert not np.array_equal(brains[0].state_dict_flat(), init[0])
    _equal_learners(both, dqn)
    assert both.tracker.results == dqn.tracker.results
    trained, brains_t, init_t = _train(learn_batch={"DQN": 96, "D3QN": 130})
    assert trained.learners[1].state.cpu().tolist() == [2, 2] and trained.learners[0].state.cpu().tolist()[0] > 0
    for k in (0, 1):
        now = brains_t[k].state_dict_flat()
        assert np.isfinite(now).all() and not np.array_equal(now, init_t[k])
