"""GPU: rl_learn_td_draw and rl_learn_td beyond the 96-row fixture -- the weighted draw row for row against the float64 race on rings whose
256-stride loop takes a second pass and whose last group of four rows is partial (1 .. 1025 rows with real ages, size below the
capacity), stamping through the wrap of capacity 1001, learners of different batches in one draw call of the C ABI, one step on the
reference's TRAINED weights (tests/golden/perdqn.npz: |w| up to 2.05, |pred| and |target| in the hundreds) against float64, beta at its
cap, Adam at step 10,000 on moments that are not zero, the fixture's rows at the top of a ring of 10,000, a bad slot that only the second
pass of the 512-stride check reaches, and the sixteenth learner of a launch.  tests/test_learn_late_edges_cpu.py checks without a GPU that
these inputs satisfy what the comparisons rest on.  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = 1e-3, 0.99
SIZES = (1, 3, 255, 256, 257, 701, 1025)
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
MEM = ("priority", "beta_is", "seen")
SENTINEL = np.float32(2.0 ** -20)
GUARD = 64
_keys = {}


def _edge(n, seed=11):
    """(the first n of 1027 seeded rows with ages 0..199, their content keys)"""
    if seed not in _keys:
        rows = lc.edge_ring_rows(1027, seed)
        _keys[seed] = (rows, pc.content_keys(rows, 1027, rows["ring_age"]))
        assert len(set(_keys[seed][1].tolist())) == 1027
    rows, keys = _keys[seed]
    return {k: v[:n] for k, v in rows.items()}, keys[:n]


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.PERDQN()
    with torch.no_grad():
        for p, v in zip(b.model.parameters(), tc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, count=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture lays one out; the ages are the rows' ("ring_age") or 0."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    age = rows["ring_age"] if "ring_age" in rows else np.zeros(capacity, np.int32)
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": t(age, torch.int32),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, target_flat, ring, priority, n_steps=1, batch=64, want_grad=True, sync_target=False, fill_beyond=None):
    """A PERDQN learner whose size gate is open; the memory holds `priority` in its first rows (fill_beyond: the value of the rows
    after them), nothing new to stamp (seen = count) and beta 0.4."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring, td_priority=True)
    assert (l.entry, l.lr, l.gamma, l.batch, l.beta_increment, l.sync_target) == ("rl_learn_td", LR, GAMMA, 64, 0.001, True)
    assert np.float32(l.p_new).tobytes() == tc.golden()["p_new"].tobytes() and l.beta_is.item() == 0.4
    _prime(l, ring, priority, fill_beyond)
    l.batch, l.min_size, l.sync_target = batch, 0, sync_target
    l.target.copy_(torch.as_tensor(np.array(target_flat, np.float32), device=DEV))
    l.is_weight = torch.zeros((n_steps, batch), dtype=torch.float32, device=DEV)
    if want_grad:
        l.grad = torch.zeros((n_steps, tc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _prime(l, ring, priority, fill_beyond=None):
    """Give a learner `ring` and the priorities of its first len(priority) rows, with nothing new to stamp (seen = count)."""
    import torch
    l.ring = ring
    l._make_td()
    if fill_beyond is not None:      # rows beyond the ring's size: a loop bounded by the capacity would draw them
        l.priority.fill_(fill_beyond)
    l.priority[:len(priority)] = torch.as_tensor(np.array(priority, np.float32), device=DEV)
    l.seen.copy_(ring["count"])


def _np(l, names=BUFFERS + MEM):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in names}


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


@pytest.fixture(scope="module")
def drawer():
    """One PERDQN learner for the draw tests; every case gives it its own ring and memory."""
    g, p = dc.golden(), tc.golden()
    return _learner(p["init"], p["target_init"], _ring(g), p["prio_init"], want_grad=False)


# ---- 1. the draw, row for row ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_the_td_draw_is_the_host_models_row_for_row(worlds, drawer, n, slack):
    """rl_learn_td_draw on n rows (capacity n + slack; priorities random^3 * 4, every 7th row 0; the rows beyond the size hold 1e6: a loop
    bounded by the capacity would draw them), batch 64, two steps, at calls 0 and 3: every one of the 128 slots is the winner of the
    float64 race on the float32 priorities.  The race's smallest relative gap between first and second is at least 1e-4 on these inputs
    (asserted here, and without a GPU in tests/test_learn_late_edges_cpu.py), a hundred times what -logf(U) / p can be off by, so no draw
    is left out.  No drawn row has priority 0, the keys read back are the content keys WITH the ages, no priority changes, seen == n."""
    import torch
    rows, keys = _edge(n + slack)
    pri = pc.edge_priorities(n)
    l = drawer
    from reinlife_amd import _lib
    for calls in (0, 3):
        _prime(l, _ring(rows, count=n), pri, fill_beyond=1e6)
        l.state[1] = calls
        got = worlds.draw_td([l], 2)
        torch.cuda.synchronize()
        worlds.check_error_flag()
        assert tuple(got.shape) == (1, 2, 64) and got.dtype == torch.int32
        got, p_after = got.cpu().numpy().reshape(-1), l.priority.cpu().numpy()
        want, gaps = pc.host_draw64(keys[:n], pri, SEED, 0, calls, 128, site=_lib.SITE_LEARN_TD)
        print("n %d capacity %d calls %d: smallest gap %.3g; %d of 128 draws differ; %d distinct rows, %d beyond row 255, %d rows of priority 0"
              % (n, n + slack, calls, gaps.min(), int((got != want).sum()), len(np.unique(want)), int((want >= 256).sum()), int((pri == 0).sum())))
        assert gaps.min() >= 1e-4
        assert np.array_equal(got, want)
        assert (pri[got] > 0).all()
        assert np.array_equal(l.keys.cpu().numpy().view(np.uint64)[:n], keys[:n])
        assert p_after[:n].tobytes() == pri.tobytes() and (p_after[n:] == 1e6).all()      # nothing stamped, nothing beyond the size written
        assert int(l.seen.item()) == n


def test_stamping_through_the_wrap_of_a_capacity_that_is_no_multiple_of_four(worlds, drawer):
    """Capacity 1001: seen 990 -> count 1100 (slots 990..1000 and 0..98), then a whole capacity of new rows, then nothing new: priority
    is learn_perdqn_cases.stamp's byte for byte, seen == count afterwards."""
    import torch
    rows, _ = _edge(1001)
    l = drawer
    _prime(l, _ring(rows), np.full(1001, SENTINEL, np.float32))
    p_new = tc.golden()["p_new"]
    want = np.full(1001, SENTINEL, np.float32)
    for count, seen in ((1100, 990), (1100 + 1001, 1100), (1100 + 1001, 1100 + 1001)):
        l.ring["count"].fill_(count)
        assert seen == 990 or int(l.seen.item()) == seen                                 # (the draw before left it there)
        l.seen.fill_(seen)
        before = want
        want = tc.stamp(before, seen, count, p_new)
        slots = worlds.draw_td([l], 1)
        torch.cuda.synchronize()
        p = l.priority.cpu().numpy()
        print("seen %d count %d: %d rows stamped (host %d), seen afterwards %d" % (seen, count, int((p != before).sum()), int((want != before).sum()), int(l.seen.item())))
        assert p.tobytes() == want.tobytes()
        assert int(l.seen.item()) == count
        assert int(slots.min()) >= 0 and int(slots.max()) < 1001
    assert (want.view(np.uint32) == p_new.view(np.uint32)).all()
    worlds.check_error_flag()


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_learners_of_different_batches_in_one_td_draw_call(worlds, order):
    """rl_learn_td_draw through the C ABI with (batch 64, 257 rows) and (batch 7, 96 rows) in one call, two steps: the tables lie end to
    end in a buffer of exactly sum(n_steps * batch) entries, each the float64 race's at its learner's own position, with the 1e-4 gap
    asserted first; 64 guard entries on either side keep their -1."""
    import torch
    from reinlife_amd import _lib
    g, p = dc.golden(), tc.golden()
    cases = [(64, _edge(257), 3, 5), (7, _edge(96, seed=12), 1, 6)]
    cases = [cases[i] for i in order]
    learners = []
    for batch, (rows, keys), calls, pseed in cases:
        l = _learner(p["init"], p["target_init"], _ring(rows), pc.edge_priorities(len(keys), pseed), batch=batch, want_grad=False)
        l.state[1] = calls
        learners.append(l)
    n = len(learners)
    arr = (_lib.Learner * n)(*[l.struct() for l in learners])
    rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
    tds = (_lib.TdPrio * n)(*[l.td_struct() for l in learners])
    total = sum(2 * c[0] for c in cases)
    buf = torch.full((GUARD + total + GUARD,), -1, dtype=torch.int32, device=DEV)
    _lib.check(worlds.lib.rl_learn_td_draw(worlds.handle, arr, rings, tds, n, 2, C.c_void_p(buf.data_ptr() + 4 * GUARD), worlds._stream()), "rl_learn_td_draw")
    torch.cuda.synchronize()
    worlds.check_error_flag()
    got = buf.cpu().numpy()
    assert got.size == 2 * GUARD + total and (got[:GUARD] == -1).all() and (got[GUARD + total:] == -1).all()
    off = GUARD
    for i, (l, (batch, (rows, keys), calls, pseed)) in enumerate(zip(learners, cases)):
        want, gaps = pc.host_draw64(keys, pc.edge_priorities(len(keys), pseed), SEED, i, calls, 2 * batch, site=_lib.SITE_LEARN_TD)
        print("learner %d (batch %d, %d rows): smallest gap %.3g; %d of %d draws differ" % (i, batch, len(keys), gaps.min(), int((got[off:off + 2 * batch] != want).sum()), 2 * batch))
        assert gaps.min() >= 1e-4
        assert np.array_equal(got[off:off + 2 * batch], want), i
        assert int(l.seen.item()) == len(keys) and np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
        off += 2 * batch


# ---- 2. rl_learn_td beyond the fixture ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_one_step_on_trained_weights_matches_float64(worlds, which):
    """learn_perdqn_cases.edge_case(): a trained PERDQN network, the same times float32(0.96875) as the target, 1027 seeded rows with
    priorities over several orders of magnitude, minibatches of 64, 33 and 1 rows: every gradient tensor within 1e-5 of its largest
    magnitude of float64 autograd on loss = mean(w) * mean((pred - target)^2) with w = is_weights(priority, 0.401), the loss within
    relative 1e-5 (torch's own float32: 2.0e-7 to 3.3e-7, tests/test_learn_late_edges_cpu.py), is_weight within 1 float32 ulp, the
    batch rows' new priorities within 3.8e-5 x scale + 4 ulp of the float64 formula (test_priorities_weights_and_beta_of_every_call's
    bound and scale), every other row's priority unchanged, the packed weights byte for byte the host packer's."""
    import torch
    w, tgt, rows, pri, batches = tc.edge_case()
    slots = batches[which]
    batch = len(slots)
    l = _learner(w, tgt, _ring(rows), pri, batch=batch)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    r = _np(l)
    worlds.check_error_flag()
    isw = tc.is_weights(pri[slots], 0.4 + 0.001)
    loss64, g64, prio64, pred, target = tc.step(w, tgt, rows, slots, isw, GAMMA)
    got, loss = tc.split(l.grad[0].cpu().numpy()), float(l.loss[0].item())
    print("batch %d: mean(w) %.6g, loss %.9g (float64 %.9g, relative error %.3g); max |pred| %.4g, max |target| %.4g"
          % (batch, isw.mean(), loss, loss64, abs(loss - loss64) / abs(loss64), np.abs(pred).max(), np.abs(target).max()))
    worst = 0.0
    for name, a, b in zip(tc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("batch %d: %-12s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    ww = l.is_weight[0].cpu().numpy()
    w32 = isw.astype(np.float32)
    scale = max(np.abs(tc.q_values(w, rows["ring_state"][slots])).max(), np.abs(tc.q_values(tgt, rows["ring_state_prime"][slots])).max(), np.abs(target).max())
    new = r["priority"][slots]
    perr, ulp = np.abs(new - prio64), np.spacing(np.abs(new)).astype(np.float64)
    print("batch %d: worst gradient error / max|g| = %.3g; is_weight worst %.3g ulp; max |priority - float64| %.3g (bound %.3g + 4 ulp, scale %.4g)"
          % (batch, worst, (np.abs(ww - w32) / np.spacing(w32)).max(), perr.max(), 3.8e-5 * scale, scale))
    for name, a, b in zip(tc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert (np.abs(ww - w32) <= np.spacing(w32)).all()
    assert (perr <= 3.8e-5 * scale + 4 * ulp).all()
    rest = np.setdiff1d(np.arange(1027), slots)
    assert len(rest) >= 1027 - batch and r["priority"][rest].tobytes() == pri[rest].tobytes()
    assert r["state"].tolist() == [1, 1] and r["beta_is"][0] == 0.4 + 0.001 and r["params"].tobytes() != w.tobytes()
    assert r["target"].tobytes() == tgt.tobytes() and r["packed"].tobytes() == _host_pack(r["params"]).tobytes()


def test_beta_stops_at_its_cap(worlds):
    """beta_is = 0.9995, one call of two steps on the fixture: beta afterwards is min(1.0, min(1.0, 0.9995 + 0.001) + 0.001) == 1.0
    exactly; both steps' is_weight rows are (p / p_min) ** -1 within 1 float32 ulp on the priorities the device held before each
    step (a single-step call from the same start shows those of the second: the steps are deterministic); the step-0 gradient is
    within 1e-5 of float64 with those weights.  (Without the cap the weights would be thousands of ulp off:
    tests/test_learn_late_edges_cpu.py.)"""
    g, p = dc.golden(), tc.golden()
    out = {}
    for n_steps in (1, 2):
        l = _learner(p["init"], p["target_init"], _ring(g), p["prio_init"], n_steps=n_steps)
        l.beta_is.fill_(0.9995)
        worlds.learn([l], n_steps, slots=g["slots"][:n_steps].reshape(1, n_steps, 64))
        out[n_steps] = _np(l, BUFFERS + MEM + ("grad", "loss", "is_weight"))
    worlds.check_error_flag()
    one, two = out[1], out[2]
    want = min(1.0, min(1.0, 0.9995 + 0.001) + 0.001)
    print("beta after one step %.17g, after two %.17g (wanted %.17g)" % (one["beta_is"][0], two["beta_is"][0], want))
    assert want == 1.0 and two["beta_is"][0] == 1.0 and one["beta_is"][0] == 1.0
    assert two["is_weight"][0].tobytes() == one["is_weight"][0].tobytes() and two["grad"][0].tobytes() == one["grad"][0].tobytes()
    held = (p["prio_init"], one["priority"])                                             # before step 0, before step 1
    for s in range(2):
        w64 = tc.is_weights(held[s][g["slots"][s]], 1.0)
        w32 = w64.astype(np.float32)
        err = np.abs(two["is_weight"][s] - w32) / np.spacing(w32)
        print("step %d: is_weight worst %.3g ulp of (p / p_min) ** -1; mean %.6g" % (s, err.max(), w64.mean()))
        assert (err <= 1).all(), s
        assert len(set(held[s][g["slots"][s]].tolist())) > 1 and w64.mean() < 0.95
    loss64, g64, _, _, _ = tc.step(p["init"], p["target_init"], g, g["slots"][0], tc.is_weights(p["prio_init"][g["slots"][0]], 1.0), GAMMA)
    worst = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(tc.split(two["grad"][0]), g64))
    print("step 0 at beta 1: worst gradient error / max|g| = %.3g; loss relative error %.3g" % (worst, abs(two["loss"][0] - loss64) / loss64))
    for name, a, b in zip(tc.NAMES, tc.split(two["grad"][0]), g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
    assert abs(two["loss"][0] - loss64) <= 1e-5 * loss64
    assert two["state"].tolist() == [2, 1]


def test_adam_at_step_ten_thousand_on_moments_that_are_not_zero(worlds):
    """state[0] = 9999, adam_m ~ N(0, 1e-3), adam_v the squares of another such draw, the fixture's first minibatch, one step: every
    parameter within 1e-5 lr + 1 ulp of adam64(p, m, v, kernel_grad, t = 10000), m and v within 1 ulp of the float64 values, state
    [10000, 1].  (A replay at t = 3 misses the bar on most parameters.)"""
    import torch
    g, p = dc.golden(), tc.golden()
    m0, v0 = dc.adam_moments(tc.N_PARAMS)
    l = _learner(p["init"], p["target_init"], _ring(g), p["prio_init"])
    l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
    l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
    l.state[0] = 9999
    worlds.learn([l], 1, slots=g["slots"][0].reshape(1, 1, 64))
    r = _np(l)
    worlds.check_error_flag()
    grad = l.grad[0].cpu().numpy().astype(np.float64)
    f64 = lambda x: x.astype(np.float64)  # noqa: E731
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    p64, m64, v64 = dc.adam64(f64(p["init"]), f64(m0), f64(v0), grad, 10000, LR)
    p3 = dc.adam64(f64(p["init"]), f64(m0), f64(v0), grad, 3, LR)[0]
    perr, bound = np.abs(r["params"] - p64), 1e-5 * LR + ulp(r["params"])
    merr, verr = np.abs(r["adam_m"] - m64) / ulp(m64), np.abs(r["adam_v"] - v64) / ulp(v64)
    print("PERDQN Adam at t = 10000: worst |p - float64| / (1e-5 lr + 1 ulp) %.3g (%d of %d beyond the bound; largest step %.3g lr); m: worst %.3g ulp; v: worst %.3g ulp; "
          "a replay at t = 3 would leave %d parameters beyond the bound"
          % ((perr / bound).max(), int((perr > bound).sum()), perr.size, (np.abs(p64 - p["init"]) / LR).max(), merr.max(), verr.max(), int((np.abs(r["params"] - p3) > bound).sum())))
    assert r["state"].tolist() == [10000, 1] and grad.any()
    assert (perr <= bound).all()
    assert (merr <= 1).all() and (verr <= 1).all()
    assert (np.abs(r["params"] - p3) > bound).sum() > perr.size // 2


def test_rows_at_the_top_of_a_long_ring_train_like_the_fixture_ring(worlds):
    """The fixture's rows at the last slots of a ring of 10,000 zero rows, three steps on slots + offset: every buffer, gradient, loss,
    weight and beta byte for byte the short ring's run; the priorities of the top rows are the short run's, every row below keeps a
    sentinel."""
    g, p = dc.golden(), tc.golden()
    capacity, at = 10000, 10000 - 96
    pri_long = np.full(capacity, SENTINEL, np.float32)
    pri_long[at:] = p["prio_init"]
    names = BUFFERS + MEM + ("grad", "loss", "is_weight")
    out = []
    for rows, pri, off in ((g, p["prio_init"], 0), (lc.relocated(g, capacity, at), pri_long, at)):
        l = _learner(p["init"], p["target_init"], _ring(rows), pri, n_steps=3)
        worlds.learn([l], 3, slots=(g["slots"] + off).reshape(1, 3, 64))
        out.append(_np(l, names))
    worlds.check_error_flag()
    short, long_ = out
    for k in BUFFERS + ("grad", "loss", "is_weight", "beta_is"):
        assert short[k].tobytes() == long_[k].tobytes(), k
    assert short["state"].tolist() == [3, 1] and short["params"].tobytes() != p["init"].tobytes() and short["grad"].any()
    assert long_["priority"][at:].tobytes() == short["priority"].tobytes() != p["prio_init"].tobytes()
    assert (long_["priority"][:at] == SENTINEL).all() and int(long_["seen"][0]) == capacity


def test_a_bad_slot_late_in_the_table_is_flagged_and_that_learner_is_left_alone(worlds):
    """n_steps = 10 minibatches of 64 rows: 640 table entries, so the 512-stride check of k_learn_perdqn takes a second pass; the bad
    value (the ring's size) sits at index 600.  Error-flag code 6 with [learner, 600 // 64, value]; every buffer of that learner --
    priority and beta_is among them -- is untouched; the healthy learner of the same call equals itself alone."""
    import torch
    g, p = dc.golden(), tc.golden()
    good = np.random.RandomState(8).randint(0, 96, size=(10, 64)).astype(np.int32)
    bad = np.random.RandomState(9).randint(0, 96, size=(10, 64)).astype(np.int32)
    bad.reshape(-1)[600] = 96
    init2 = (p["init"] * np.float32(0.75)).astype(np.float32)
    a = _learner(p["init"], p["target_init"], _ring(g), p["prio_init"], n_steps=10, sync_target=True)
    b = _learner(init2, p["target_init"], _ring(g), p["prio_init"], n_steps=10, want_grad=False)
    a.packed.mul_(0.5)
    before = _np(a)
    worlds.err.zero_()
    worlds.learn([a, b], 10, slots=np.stack([bad, good]))
    torch.cuda.synchronize()
    print("error flag %s" % worlds.err.cpu().tolist())
    assert worlds.err.cpu().tolist() == [6, 0, 600 // 64, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in BUFFERS + MEM:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item() and not a.is_weight.any().item() and after["beta_is"][0] == 0.4
    solo = _learner(init2, p["target_init"], _ring(g), p["prio_init"], n_steps=10, want_grad=False)
    worlds.learn([solo], 10, slots=good.reshape(1, 10, 64))
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [10, 1] and rb["params"].tobytes() != init2.tobytes()
    for k in BUFFERS + MEM:
        assert rb[k].tobytes() == rs[k].tobytes(), k
    assert b.is_weight.cpu().numpy().tobytes() == solo.is_weight.cpu().numpy().tobytes()


def test_the_sixteenth_learner_of_a_launch_ends_on_the_bits_it_ends_on_alone(worlds):
    """RL_MAX_CAPTURE_BRAINS = 16 learners in one call, one step each: the learner at index 15 (the fixture's network; the others: a
    scaled one on the reversed ring) equals itself alone."""
    g, p = dc.golden(), tc.golden()
    rows2 = {k: np.ascontiguousarray(g[k][::-1]) for k in dc.RING_KEYS}
    init2 = (p["init"] * np.float32(0.75)).astype(np.float32)
    ring, ring2 = _ring(g), _ring(rows2)
    mine, other = g["slots"][1], np.ascontiguousarray(g["slots"][0][::-1])
    learners = [_learner(init2, p["target_init"], ring2, p["prio_init"][::-1], want_grad=False) for _ in range(15)]
    learners.append(_learner(p["init"], p["target_init"], ring, p["prio_init"], want_grad=False))
    worlds.learn(learners, 1, slots=np.stack([other] * 15 + [mine]).reshape(16, 1, 64).astype(np.int32))
    last, first = _np(learners[15]), _np(learners[0])
    solo = _learner(p["init"], p["target_init"], ring, p["prio_init"], want_grad=False)
    worlds.learn([solo], 1, slots=mine.reshape(1, 1, 64))
    rs = _np(solo)
    worlds.check_error_flag()
    for k in BUFFERS + MEM:
        assert last[k].tobytes() == rs[k].tobytes(), k
    assert learners[15].is_weight.cpu().numpy().tobytes() == solo.is_weight.cpu().numpy().tobytes()
    assert last["state"].tolist() == [1, 1] == first["state"].tolist() and last["params"].tobytes() != p["init"].tobytes()
    assert first["params"].tobytes() != last["params"].tobytes()
