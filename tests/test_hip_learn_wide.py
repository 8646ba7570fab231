"""GPU: rl_learn_wide / DeviceLearner(wide_batch=) / trainer(learn_batch=) -- the DQN update of ReinLife/Models/DQN.py:80-83, 142-153 on
minibatches of several 32-row tiles: one tile is rl_learn bit for bit, several tiles against torch float64 autograd, Adam replayed from the
kernel's own gradients, repeatability and independence of the learners of a launch, the size gate and the checked bad slot, and the
whole path through trainer().  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_cases as lc
import learn_wide_cases as wc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = wc.LR, wc.GAMMA
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.DQN()
    with torch.no_grad():
        for p, v in zip(b.agent.parameters(), lc.split(flat)):
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


def _learner(flat, ring, n_steps, batch, wide=True, target=None, min_size=0):
    """A DQN learner (wide: through rl_learn_wide) with grad and loss rows; the rings of these tests are small, so the gate is open
    unless min_size says otherwise."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring, **({"wide_batch": batch} if wide else {}))
    assert l.entry == ("rl_learn_wide" if wide else "rl_learn")
    if wide:
        assert l.batch == batch and l.work.numel() == wc.work_bytes(batch) and l.work.data_ptr() % 16 == 0
    l.batch = batch
    assert (l.lr, l.gamma, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (LR, GAMMA, 1000, 20, 5, True)
    l.min_size = min_size
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


@pytest.mark.parametrize("batch", [32, 7])
@pytest.mark.parametrize("explicit", [True, False])
def test_one_tile_is_rl_learn_bit_for_bit(worlds, batch, explicit):
    """Two steps on the wrapped fixture ring (capacity 48, count 130), with explicit slots and with the Philox draw: every buffer,
    the losses and the gradients of rl_learn_wide are those of rl_learn from the same start."""
    g = lc.golden()
    slots = np.ascontiguousarray(g["slots"][:2, :batch]).astype(np.int32).reshape(1, 2, batch) if explicit else None
    a = _learner(g["init"], _ring(g, count=130), 2, batch, wide=True)
    b = _learner(g["init"], _ring(g, count=130), 2, batch, wide=False)
    worlds.learn([a], 2, slots=slots)
    worlds.learn([b], 2, slots=slots)
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [2, 1] and rb["grad"].any() and (rb["loss"] > 0).all()
    assert rb["params"].tobytes() != np.asarray(g["init"]).tobytes()
    _same(ra, rb)


def _check_against_float64(tag, l, case):
    w, tgt, rows, slots, loss64, g64 = case
    got = lc.split(l.grad[0].cpu().numpy())
    loss = float(l.loss[0].item())
    print("%s: loss %.9g (float64 %.9g, relative error %.3g)" % (tag, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(lc.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("%s: %-10s max|g| %.4g  error / max|g| %.3g  exact zeros %d of %d" % (tag, name, np.abs(b).max(), err, int((b == 0).sum()), b.size))
    print("%s: worst gradient error / max|g| = %.3g (bar 1e-5)" % (tag, worst))
    for name, a, b in zip(lc.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
        assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)


@pytest.mark.parametrize("batch", [33, 64, 96, 80])
def test_several_tiles_match_float64_autograd(worlds, batch):
    """One step of the reference's trained weights on seeded ring rows: a one-row last tile (33), full tiles (64, 96) and a ragged last
    tile (80).  Every gradient tensor within 1e-5 of its largest magnitude of torch float64 autograd, exact zeros where float64 has
    them, loss within 1e-5 relative -- rl_learn's bar, unchanged: a tile's arithmetic is rl_learn's and the cross-tile sum is double."""
    import torch
    case = wc.edge_case(batch)
    w, tgt, rows, slots, loss64, g64 = case
    assert len(slots) == batch and len(set(slots.tolist())) < batch and (g64[4] == 0).any()
    l = _learner(w, _ring(rows), 1, batch, target=tgt)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    _check_against_float64("batch %d" % batch, l, case)
    assert l.state.cpu().tolist() == [1, 1]


def test_adam_over_three_wide_steps_matches_torch_formula_on_the_kernels_own_gradients(worlds):
    """Batch 96, three steps: torch.optim.Adam replayed in numpy float64 from the kernel's own gradient rows -- every parameter within
    1e-5 lr + 1 ulp of a replay that keeps its state in float32 as torch does, within 1e-5 lr + 3 ulp of one that never rounds, moments
    within 1e-5 of their maxima; the counters, the target copy and the packed weights as rl_learn leaves them."""
    w, tgt = lc.pretrained("DQN")
    rows = lc.edge_ring_rows(wc.EDGE_ROWS)
    slots = wc.slot_table(3, 96, wc.EDGE_ROWS, 7)
    l = _learner(w, _ring(rows), 3, 96, target=tgt)
    worlds.learn([l], 3, slots=slots.reshape(1, 3, 96))
    r = _np(l)
    worlds.check_error_flag()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    p, m, v = w.astype(np.float64), np.zeros(lc.N_PARAMS), np.zeros(lc.N_PARAMS)
    pu, mu, vu = p, m, v
    for t in range(1, 4):
        gt = r["grad"][t - 1].astype(np.float64)
        assert gt.any()
        p, m, v = (f32(x) for x in lc.adam64(p, m, v, gt, t, LR))
        pu, mu, vu = lc.adam64(pu, mu, vu, gt, t, LR)
    err = np.abs(r["params"].astype(np.float64) - p)
    ulp = np.spacing(np.abs(r["params"])).astype(np.float64)
    bound = 1e-5 * LR + ulp
    err_u = np.abs(r["params"].astype(np.float64) - pu)
    print("Adam, batch 96 x 3: max |p - replay| %.3g (bound 1e-5 lr = %.3g + 1 ulp), worst error / bound %.3g; moments: m %.3g v %.3g (relative "
          "to their maxima); against a replay that never rounds to float32: worst error / (1e-5 lr + 3 ulp) %.3g"
          % (err.max(), 1e-5 * LR, (err / bound).max(), np.abs(r["adam_m"] - m).max() / np.abs(m).max(), np.abs(r["adam_v"] - v).max() / np.abs(v).max(),
             (err_u / (1e-5 * LR + 3 * ulp)).max()))
    assert (err <= bound).all()
    assert (err_u <= 1e-5 * LR + 3 * ulp).all()
    assert np.abs(r["adam_m"] - m).max() <= 1e-5 * np.abs(m).max() and np.abs(r["adam_v"] - v).max() <= 1e-5 * np.abs(v).max()
    assert r["state"].tolist() == [3, 1]
    assert r["target"].tobytes() == r["params"].tobytes() and r["params"].tobytes() != w.tobytes()
    assert r["packed"].tobytes() == _host_pack(r["params"]).tobytes()
    assert np.isfinite(r["loss"]).all() and (r["loss"] > 0).all()


def test_runs_repeat_and_the_learners_of_a_launch_are_independent(worlds):
    """The same call twice from the same start gives the same bits; a learner alone and the same learner as the middle one of three in
    a launch give the same bits (batch 96, two steps, explicit slots)."""
    g = lc.golden()
    w, tgt = lc.pretrained("DQN")
    rows = lc.edge_ring_rows(wc.EDGE_ROWS)
    slots = wc.slot_table(2, 96, wc.EDGE_ROWS, 21)
    other = wc.slot_table(2, 96, 48, 22)

    def mine():
        return _learner(w, _ring(rows), 2, 96, target=tgt)
    a, b = mine(), mine()
    worlds.learn([a], 2, slots=slots.reshape(1, 2, 96))
    worlds.learn([b], 2, slots=slots.reshape(1, 2, 96))
    ra, rb = _np(a), _np(b)
    _same(ra, rb)
    c = mine()
    x, y = _learner(g["init"], _ring(g), 2, 96), _learner((g["init"] * np.float32(0.75)).astype(np.float32), _ring(g), 2, 96)
    worlds.learn([x, c, y], 2, slots=np.stack([other, slots, other[::-1]]).astype(np.int32))
    rc, rx, ry = _np(c), _np(x), _np(y)
    worlds.check_error_flag()
    _same(ra, rc)
    assert ra["state"].tolist() == [2, 1] and rx["state"].tolist() == [2, 1] and ry["state"].tolist() == [2, 1]
    assert rx["params"].tobytes() != ry["params"].tobytes() != ra["params"].tobytes()


def test_a_tile_of_one_row_drawn_32_times_matches_float64(worlds):
    """Batch 96 where all of tile 1's slots are equal: duplicates count once each, as in rl_learn."""
    import torch
    case = wc.edge_case(96, equal_tile=1)
    w, tgt, rows, slots, loss64, g64 = case
    assert len(set(slots[32:64].tolist())) == 1 and len(set(slots[:32].tolist())) > 16
    l = _learner(w, _ring(rows), 1, 96, target=tgt)
    worlds.learn([l], 1, slots=slots.reshape(1, 1, 96))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    _check_against_float64("batch 96, tile 1 one row", l, case)


def test_below_the_size_gate_nothing_trains_but_the_call_is_counted(worlds):
    """DQN.py:81-83: a ring of 1000 rows trains nothing; the target copy still happens, the call is counted, packed is rewritten, and no
    error flag is raised; one more row and the call trains on the rows Philox names."""
    import torch
    from reinlife_amd.learn import philox_slots
    g = lc.golden()
    rows = lc.edge_ring_rows(1100, seed=3)
    l = _learner(g["init"], _ring(rows, count=1000), 2, 96, min_size=1000)
    l.target.mul_(0.5)
    l.packed.zero_()
    before = _np(l)
    worlds.learn([l], 2)
    after = _np(l)
    worlds.check_error_flag()
    assert worlds.err.cpu().tolist()[0] == 0
    for k in ("params", "adam_m", "adam_v", "grad", "loss"):
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["state"].tolist() == [0, 1] and after["target"].tobytes() == before["params"].tobytes()
    assert after["packed"].tobytes() == _host_pack(before["params"]).tobytes() and after["packed"].any()
    # one more transition: the gate opens, and slots=None draws rl_learn's rule with the wider batch
    a = _learner(g["init"], _ring(rows, count=1001), 2, 96, min_size=1000)
    b = _learner(g["init"], _ring(rows, count=1001), 2, 96, min_size=1000)
    slots = philox_slots(SEED, 0, 0, 2, 96, 1001)
    assert slots.max() < 1001 and len(np.unique(slots)) > 150
    worlds.learn([a], 2)
    worlds.learn([b], 2, slots=slots.reshape(1, 2, 96))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    assert ra["state"].tolist() == [2, 1] and ra["grad"].any()
    _same(ra, rb)


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_bad_slot_is_flagged_and_that_learner_is_left_alone(worlds, where):
    """Batch 96, two steps.  A slot equal to the ring's size at table index 0, or -1 at the very last index of the last tile of the last
    step: error-flag code 6 with the learner, the step and the value; none of that learner's buffers is written -- packed, which does
    not match its params here, included -- and the healthy learner of the same call trains as it does alone.  (The check pass reads
    the table's VALUES; no kernel forms an address from a slot of a learner it has marked bad.)"""
    import torch
    w, tgt = lc.pretrained("DQN")
    rows = lc.edge_ring_rows(wc.EDGE_ROWS)
    good = wc.slot_table(2, 96, wc.EDGE_ROWS, 31)
    bad = good.copy()
    if where == "first":
        bad[0, 0] = wc.EDGE_ROWS
        want = [6, 1, 0, wc.EDGE_ROWS]
    else:
        bad[1, 95] = -1
        want = [6, 1, 1, -1]
    healthy, broken = _learner(w, _ring(rows), 2, 96, target=tgt), _learner(w, _ring(rows), 2, 96, target=tgt)
    broken.packed.mul_(0.5)
    broken.adam_m.fill_(0.25)
    before = _np(broken)
    worlds.err.zero_()
    worlds.learn([healthy, broken], 2, slots=np.stack([good, bad]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == want
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    _same(_np(broken), before)
    assert not broken.grad.any().item() and not broken.loss.any().item()
    solo = _learner(w, _ring(rows), 2, 96, target=tgt)
    worlds.learn([solo], 2, slots=good.reshape(1, 2, 96))
    rh, rs = _np(healthy), _np(solo)
    worlds.check_error_flag()
    assert rh["state"].tolist() == [2, 1] and rh["params"].tobytes() != w.tobytes()
    _same(rh, rs)


# ---- the whole path: trainer(learn="device", learn_batch=...) ----
_runs = {}


def _train(tmp=None, **kw):
    """One short trainer() run of two DQN brains on 4 synthetic worlds (its learners pass the 1000-row gate within the run); runs
    without a folder to save into are made once per keyword set."""
    import torch
    from reinlife_amd import Models, trainer
    key = tuple(sorted(kw.items()))
    if tmp is None and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.DQN(max_epi=60)]
    init = [b.state_dict_flat().copy() for b in brains]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=60, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      save=tmp is not None, print_results=False, **kw)
    for k in env.learners:   # no chunk appended more than a ring holds: the set of rows a draw sees repeats from run to run
        count, capacity = int(env.worlds.replays[k]["count"].item()), int(env.worlds.replays[k]["state"].shape[0])
        assert 1000 < count <= capacity, (k, count, capacity)
    out = (env, brains, init)
    if tmp is None:
        _runs[key] = out
    return out


def _learner_bits(env):
    import torch
    torch.cuda.synchronize()
    return {k: {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS} for k, l in env.learners.items()}


def test_learn_batch_32_is_the_run_without_the_keyword():
    """The draw table is the same flat table and a one-tile call is rl_learn: bit-identical learners and Tracker results."""
    env, _, _ = _train()
    env32, _, _ = _train(learn_batch=32)
    assert {l.entry for l in env.learners.values()} == {"rl_learn"} and {l.entry for l in env32.learners.values()} == {"rl_learn_wide"}
    assert env.learn_batch is None and env32.learn_batch == 32
    a, b = _learner_bits(env), _learner_bits(env32)
    assert sorted(a) == sorted(b) == [0, 1]
    for k in a:
        for n in BUFFERS:
            assert a[k][n] == b[k][n], (k, n)
        assert env.learners[k].state.cpu().tolist()[0] > 0
    assert env.tracker.results == env32.tracker.results


def test_learn_batch_96_trains_saves_and_repeats(tmp_path, monkeypatch):
    import torch
    env, brains, init = _train(learn_batch=96)
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20 and env.learn_steps == 5
    for k, b in enumerate(brains):
        l = env.learners[k]
        assert l.entry == "rl_learn_wide" and l.batch == 96
        steps, calls = l.state.cpu().tolist()
        assert steps > 0 and steps % 5 == 0 and calls == 3, (steps, calls)
        now = b.state_dict_flat()
        assert not np.array_equal(now, init[k]) and np.isfinite(now).all()
        assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes()             # what the worlds acted with
        assert env.worlds._brain_keep[k].data_ptr() == l.packed.data_ptr()
    env32, brains32, _ = _train(learn_batch=32)
    assert brains32[0].state_dict_flat().tobytes() != brains[0].state_dict_flat().tobytes()   # a wider batch is another update
    # a second identical call gives the same parameters
    monkeypatch.chdir(tmp_path)
    env2, brains2, init2 = _train(tmp=tmp_path, learn_batch=96)
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    # save=True wrote the trained weights, and settings.json names the keyword
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "DQN", "brain_gene_*.pt")))
    assert len(files) == 2
    for f, b, i in zip(files, brains2, init2):
        flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(f).values()])
        assert flat.tobytes() == b.state_dict_flat().tobytes() and not np.array_equal(flat, i)
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_wide" in settings and '"Learn batch": 96' in settings and "inference only" not in settings


def test_the_merge_of_one_rank_is_the_identity_on_a_wide_learner():
    """learn_ranks="average" on one rank without a process group: export, merge and repack after every learning episode change no bit."""
    env, brains, _ = _train(learn_batch=96)
    envm, brainsm, _ = _train(learn_batch=96, learn_ranks="average")
    assert envm.learn_ranks == "average" and envm.learn_now_calls == env.learn_now_calls == 3
    a, b = _learner_bits(env), _learner_bits(envm)
    for k in a:
        for n in BUFFERS:
            assert a[k][n] == b[k][n], (k, n)
    assert env.tracker.results == envm.tracker.results
