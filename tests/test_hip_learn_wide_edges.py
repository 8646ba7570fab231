"""GPU: rl_learn_wide at its own sizes -- one step of 2048, 2017 and 1000 rows (64 tiles; 64 with a one-row last tile; 32 with a last tile
of 8) on the reference's trained weights against float64 autograd, the loss row against the double sum of the tile losses the call
left in its work buffer, Adam at steps 10,000 .. 10,002 over 64 tiles on moments that are not zero, a bad slot that only the second
pass of k_wide_check's 256-stride loop reaches and one in the last tile of batch 2048, the content-key draw of a 2048-row batch, and
the sixteenth learner of a launch.  tests/test_learn_late_edges_cpu.py checks without a GPU that these inputs satisfy what the
comparisons rest on.  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_wide_cases as wc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = wc.LR, wc.GAMMA
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
ROWS = 1027


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.DQN()
    with torch.no_grad():
        for p, v in zip(b.agent.parameters(), lc.split(flat)):
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


def _learner(flat, ring, n_steps, batch, target=None):
    """A wide DQN learner with grad and loss rows and an open size gate."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring, wide_batch=batch)
    assert l.entry == "rl_learn_wide" and l.batch == batch and (l.lr, l.gamma, l.sync_target) == (LR, GAMMA, True)
    assert l.work.numel() == wc.work_bytes(batch) and l.work.data_ptr() % 16 == 0
    l.min_size = 0
    if target is not None:
        l.target.copy_(torch.as_tensor(np.array(target), device=DEV))
    l.grad = torch.zeros((n_steps, lc.N_PARAMS), dtype=torch.float32, device=DEV)
    l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l):
    import torch
    torch.cuda.synchronize()
    out = {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS}
    out["grad"], out["loss"] = l.grad.cpu().numpy().copy(), l.loss.cpu().numpy().copy()
    return out


def _same(a, b, keys=BUFFERS + ("grad", "loss")):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.DQN), np.float32)
    assert lib.rl_policy_pack_weights(_lib.DQN, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


@pytest.fixture(scope="module")
def ring():
    """The 1027 seeded rows on the device, shared by the tests that only read them."""
    return _ring(lc.edge_ring_rows(ROWS))


# ---- 1. one step at the sizes the timing profile measures ---------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2048, 2017, 1000])
def test_one_wide_step_matches_float64_autograd(worlds, ring, batch):
    """learn_wide_cases.edge_case(batch, n_rows=1027): the reference's trained DQN weights on 1027 seeded rows, about 870 of the 2048 slots
    distinct.  Every gradient tensor within 1e-5 of its largest magnitude of float64 autograd, exact zeros where float64 has them
    (fc3.weight: 23 to 29), the loss within relative 1e-5 (torch's own float32: 2.4e-7 to 2.9e-7,
    tests/test_learn_late_edges_cpu.py); the work buffer is rl_learn_wide_work_bytes long (7,293,248 bytes at 2048) and the loss row is
    the double sum of the tile losses the call left behind `tiles * n_params` floats, and of their float64 model, within the same bar."""
    import torch
    w, tgt, rows, slots, loss64, g64 = wc.edge_case(batch, n_rows=ROWS)
    tiles = wc.tiles(batch)
    assert len(slots) == batch and (g64[4] == 0).any()
    l = _learner(w, ring, 1, batch, target=tgt)
    assert l.work.numel() == wc.work_bytes(batch) and (batch != 2048 or l.work.numel() == 7293248)
    l.work.fill_(0xff)                                                                   # (the buffer needs no initialisation: NaN patterns)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    got, loss = lc.split(l.grad[0].cpu().numpy()), float(l.loss[0].item())
    print("batch %d (%d tiles): loss %.9g (float64 %.9g, relative error %.3g)" % (batch, tiles, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(lc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("batch %d: %-10s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (batch, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    work = l.work.cpu().numpy()
    tile_loss = work[wc.HEADER_BYTES + tiles * lc.N_PARAMS * 4:][:tiles * 4].view(np.float32).astype(np.float64)
    model, per_tile = wc.tile_loss_model(w, tgt, rows, slots)
    summed = tile_loss.sum() / batch
    print("batch %d: worst gradient error / max|g| = %.3g (bar 1e-5); loss row against the double sum of the device's tile losses %.3g, against their float64 model %.3g; "
          "worst tile loss against its model %.3g" % (batch, worst, abs(loss - summed) / summed, abs(loss - model) / model, (np.abs(tile_loss - per_tile) / per_tile).max()))
    for name, a, b in zip(lc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert abs(loss - summed) <= 1e-5 * summed and abs(loss - model) <= 1e-5 * model
    assert tile_loss.shape == per_tile.shape == (tiles,) and np.isfinite(tile_loss).all()
    hdr = work[:wc.HEADER_BYTES].view(np.int64)
    assert hdr[:5].tolist() == [1, 0, 0, 0, ROWS]                                        # trains, no bad slot, steps and calls at entry, size
    assert l.state.cpu().tolist() == [1, 1]


# ---- 2. a late step over 64 tiles ---------------------------------------------------------------------------------------------------
def test_adam_at_step_ten_thousand_over_64_tiles(worlds, ring):
    """Batch 2048, three steps in one call, state[0] = 9999, moments from learn_d3qn_cases.adam_moments(28488).  A call of ONE step:
    every parameter within 1e-5 lr + 1 ulp of adam64(p, m, v, kernel_grad, t = 10000), m and v within 1 ulp, state [10000, 1].  The
    call of three: its first gradient row is that call's; Adam replayed from the kernel's own gradient rows at t = 10000 .. 10002
    with parameters and moments rounded to float32 between the steps, as the kernel keeps them: parameters within 1e-5 lr + 1 ulp,
    within 1e-5 lr + 3 ulp of a replay that never rounds (tests/test_hip_learn_wide.py's two bars), moments within 1e-5 of their
    maxima; state [10002, 1], target == params, packed the host packer's; the same call twice gives the same bits."""
    import torch
    w, tgt = lc.pretrained("DQN")
    slots = wc.slot_table(3, 2048, ROWS, 7)
    m0, v0 = dc.adam_moments(lc.N_PARAMS)

    def run(n_steps):
        l = _learner(w, ring, n_steps, 2048, target=tgt)
        l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
        l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
        l.state[0] = 9999
        worlds.learn([l], n_steps, slots=slots[:n_steps].reshape(1, n_steps, 2048))
        return _np(l)
    one, three, again = run(1), run(3), run(3)
    worlds.check_error_flag()
    _same(three, again)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    f64 = lambda x: x.astype(np.float64)  # noqa: E731
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p64, m64, v64 = lc.adam64(f64(w), f64(m0), f64(v0), f64(one["grad"][0]), 10000, LR)
    p3 = lc.adam64(f64(w), f64(m0), f64(v0), f64(one["grad"][0]), 3, LR)[0]
    perr, bound = np.abs(one["params"] - p64), 1e-5 * LR + ulp(one["params"])
    merr, verr = np.abs(one["adam_m"] - m64) / ulp(m64), np.abs(one["adam_v"] - v64) / ulp(v64)
    print("wide Adam at t = 10000: worst |p - float64| / (1e-5 lr + 1 ulp) %.3g (%d of %d beyond the bound; largest step %.3g lr); m: worst %.3g ulp; v: worst %.3g ulp; "
          "a replay at t = 3 would leave %d parameters beyond the bound"
          % ((perr / bound).max(), int((perr > bound).sum()), perr.size, (np.abs(p64 - w) / LR).max(), merr.max(), verr.max(), int((np.abs(one["params"] - p3) > bound).sum())))
    assert one["state"].tolist() == [10000, 1]
    assert (perr <= bound).all()
    assert (merr <= 1).all() and (verr <= 1).all()
    assert (np.abs(one["params"] - p3) > bound).sum() > perr.size // 2
    assert three["grad"][0].tobytes() == one["grad"][0].tobytes()
    p, m, v = f64(w), f64(m0), f64(v0)
    pu, mu, vu = p, m, v
    for s in range(3):
        assert three["grad"][s].any()
        p, m, v = (f32(x) for x in lc.adam64(p, m, v, f64(three["grad"][s]), 10000 + s, LR))
        pu, mu, vu = lc.adam64(pu, mu, vu, f64(three["grad"][s]), 10000 + s, LR)
    err, bound3 = np.abs(three["params"] - p), 1e-5 * LR + ulp(three["params"])
    err_u, bound_u = np.abs(three["params"] - pu), 1e-5 * LR + 3 * ulp(three["params"])
    em, ev = np.abs(three["adam_m"] - m).max() / np.abs(m).max(), np.abs(three["adam_v"] - v).max() / np.abs(v).max()
    print("wide Adam at t = 10000..10002: worst |p - replay| / (1e-5 lr + 1 ulp) %.3g; moments: m %.3g v %.3g (relative to their maxima); against a replay that never "
          "rounds to float32: worst error / (1e-5 lr + 3 ulp) %.3g" % ((err / bound3).max(), em, ev, (err_u / bound_u).max()))
    assert (err <= bound3).all()
    assert (err_u <= bound_u).all()
    assert em <= 1e-5 and ev <= 1e-5
    assert three["state"].tolist() == [10002, 1]
    assert three["target"].tobytes() == three["params"].tobytes() != w.tobytes()
    assert three["packed"].tobytes() == _host_pack(three["params"]).tobytes()
    assert np.isfinite(three["loss"]).all() and (three["loss"] > 0).all()


# ---- 3. bad slots late in the table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["second pass", "last tile"])
def test_a_bad_slot_late_in_the_table_is_flagged_and_that_learner_is_left_alone(worlds, ring, where):
    """Batch 160, two steps: a slot equal to the ring's size at table index 300, which only the second pass of k_wide_check's
    256-stride loop reaches.  Batch 2048, one step: the same at index 2047, the last row of the last tile.  Error-flag code 6 with the
    learner, the step and the value; none of that learner's buffers is written -- packed, which does not match its params here,
    included; the healthy learner of the same call trains as it does alone."""
    import torch
    w, tgt = lc.pretrained("DQN")
    batch, n_steps, at = (160, 2, 300) if where == "second pass" else (2048, 1, 2047)
    good = wc.slot_table(n_steps, batch, ROWS, 31)
    bad = wc.slot_table(n_steps, batch, ROWS, 32).copy()
    bad.reshape(-1)[at] = ROWS
    healthy, broken = _learner(w, ring, n_steps, batch, target=tgt), _learner(w, ring, n_steps, batch, target=tgt)
    broken.packed.mul_(0.5)
    broken.adam_m.fill_(0.25)
    before = _np(broken)
    worlds.err.zero_()
    worlds.learn([healthy, broken], n_steps, slots=np.stack([good, bad]).astype(np.int32))
    torch.cuda.synchronize()
    print("%s: error flag %s" % (where, worlds.err.cpu().tolist()))
    assert worlds.err.cpu().tolist() == [6, 1, at // batch, ROWS]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    _same(_np(broken), before)
    assert not broken.grad.any().item() and not broken.loss.any().item()
    solo = _learner(w, ring, n_steps, batch, target=tgt)
    worlds.learn([solo], n_steps, slots=good.reshape(1, n_steps, batch))
    rh, rs = _np(healthy), _np(solo)
    worlds.check_error_flag()
    assert rh["state"].tolist() == [n_steps, 1] and rh["params"].tobytes() != w.tobytes()
    _same(rh, rs)


# ---- 4. the draw at a wide batch ----------------------------------------------------------------------------------------------------
def test_the_content_key_draw_of_a_wide_batch_is_the_host_models(worlds):
    """DeviceWorlds.draw_slots for a wide learner of batch 2048, two steps, on 1025 rows with real ages: all 4,096 slots are
    learn_perd3qn_cases.host_uniform_draw's (the flat table rl_learn_draw makes as [128][32]); the wide call fed that table trains."""
    import torch
    rows = lc.edge_ring_rows(ROWS)
    n = 1025
    first = {k: v[:n] for k, v in rows.items()}
    keys = pc.content_keys(rows, ROWS, rows["ring_age"])[:n]
    w, tgt = lc.pretrained("DQN")
    l = _learner(w, _ring(first), 2, 2048, target=tgt)
    table = worlds.draw_slots([l], 2)
    torch.cuda.synchronize()
    assert tuple(table.shape) == (1, 2, 2048) and table.dtype == torch.int32
    got = table.cpu().numpy().reshape(-1)
    want = pc.host_uniform_draw(keys, SEED, 0, 0, 4096)
    print("wide draw: %d of 4096 draws differ; %d distinct rows, %d beyond row 255, %d beyond row 511" % (
        int((got != want).sum()), len(np.unique(want)), int((want >= 256).sum()), int((want >= 512).sum())))
    assert np.array_equal(got, want)
    assert np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
    worlds.learn([l], 2, slots=table)
    r = _np(l)
    worlds.check_error_flag()
    assert worlds.err.cpu().tolist()[0] == 0
    assert r["state"].tolist() == [2, 1] and r["params"].tobytes() != w.tobytes() and r["grad"].any() and (r["loss"] > 0).all()


# ---- 5. the last position of a launch -----------------------------------------------------------------------------------------------
def test_the_sixteenth_learner_of_a_launch_ends_on_the_bits_it_ends_on_alone(worlds, ring):
    """RL_MAX_CAPTURE_BRAINS = 16 learners in one call at batch 96, two steps: the learner at index 15 (the trained network; the
    others: the fixture's initial one on other slots) equals itself alone."""
    g = lc.golden()
    w, tgt = lc.pretrained("DQN")
    mine, other = wc.slot_table(2, 96, ROWS, 21), wc.slot_table(2, 96, ROWS, 22)
    learners = [_learner(g["init"], ring, 2, 96) for _ in range(15)] + [_learner(w, ring, 2, 96, target=tgt)]
    worlds.learn(learners, 2, slots=np.stack([other] * 15 + [mine]).astype(np.int32))
    last, first = _np(learners[15]), _np(learners[0])
    solo = _learner(w, ring, 2, 96, target=tgt)
    worlds.learn([solo], 2, slots=mine.reshape(1, 2, 96))
    rs = _np(solo)
    worlds.check_error_flag()
    _same(last, rs)
    assert last["state"].tolist() == [2, 1] == first["state"].tolist() and last["params"].tobytes() != w.tobytes()
    assert first["params"].tobytes() != last["params"].tobytes() and first["params"].tobytes() != np.asarray(g["init"]).tobytes()
