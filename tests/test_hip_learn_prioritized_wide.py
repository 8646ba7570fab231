"""GPU: rl_learn_prioritized_wide / rl_learn_prioritized_wide_draw / DeviceLearner(prioritized=True, prioritized_batch=) /
trainer(learn_prioritized=True, learn_batch={"PERD3QN": B}) -- PERD3QNAgent.train() (ReinLife/Models/PERD3QN.py:94-115) on minibatches
of several 64-row tiles: one tile is rl_learn_prioritized bit for bit (update, priorities, prio_max, and the draw's table); at any batch
the update is rl_learn_dueling_wide's bit for bit; the priorities of ALL rows of a wide batch against float64 with the batch-wide means
(the test a per-tile mean fails 300 times over: tests/test_learn_prioritized_wide_cpu.py); duplicated slots across tiles and positions;
steps, short rings, the gate, the checked bad slot, independence, repeatability, order independence, the draw's statistics at width, the
refusals, and the whole path through trainer().  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_dueling_wide_cases as wc
import learn_perd3qn_cases as pc
import learn_prioritized_wide_cases as pw

pytestmark = pytest.mark.gpu

SEED = pw.DRAW_SEED
DEV = "cuda:0"
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
EIGHT = BUFFERS + ("loss", "grad")
PRIO = ("priority", "prio_max")
SENTINEL = np.float32(2.0 ** -20)    # below every priority of the fixture, so that prio_max is one of the kernel's own


def _brain(cls, flat, **kw):
    import torch
    b = cls(**kw)
    with torch.no_grad():
        for p, v in zip(b.eval_net.parameters(), dc.split(flat)):
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


def _learner(n_steps, batch, kind="wide", ring=None, flat=None, sync_target=False, moments=False, min_size=0, fill=SENTINEL):
    """kind "wide": a PERD3QN learner through rl_learn_prioritized_wide; "narrow": through rl_learn_prioritized; "d3qn": a D3QN learner
    through rl_learn_dueling_wide.  All on the fixture's networks with grad and loss rows and an open gate unless min_size says
    otherwise; a memory starts with every priority at `fill`, nothing new to stamp (seen = count) and a maximum of 1."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    g = dc.golden()
    ring = _ring(g) if ring is None else ring
    flat = g["init"] if flat is None else flat
    if kind == "d3qn":
        l = DeviceLearner(_brain(Models.D3QN, flat), DEV, ring=ring, dueling_batch=batch)
        assert l.entry == "rl_learn_dueling_wide"
    else:
        l = DeviceLearner(_brain(Models.PERD3QN, flat), DEV, ring=ring, prioritized=True, **({"prioritized_batch": batch} if kind == "wide" else {}))
        assert l.entry == ("rl_learn_prioritized_wide" if kind == "wide" else "rl_learn_prioritized")
        assert (l.lr, l.gamma, l.min_size, l.train_freq, l.n_steps_default, l.sync_target, l.alpha) == (wc.LR, wc.GAMMA, 0, 20, 1, False, 0.6)
        assert (l.exploration, l.soft_update_freq) == (1000, 200)
        capacity = ring["state"].shape[0]
        assert l.priority.numel() == l.weight.numel() == l.keys.numel() == capacity and l.prio_max.item() == 1.0 and l.seen.item() == 0
        l.priority.fill_(float(fill))
        l.seen.copy_(ring["count"])
    if kind == "narrow":
        assert l.work is None and l.batch == 64
    else:
        assert l.batch == batch and l.work.numel() == wc.work_bytes(batch) and l.work.data_ptr() % 16 == 0
        l.work.fill_(0xA5)   # the work buffer needs no initialisation
    l.batch, l.min_size, l.sync_target = batch, min_size, sync_target
    l.target.copy_(torch.as_tensor(np.array(g["target_init"], np.float32), device=DEV))
    if moments:
        m0, v0 = dc.adam_moments(dc.N_PARAMS)
        l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
        l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
    l.grad = torch.zeros((n_steps, dc.N_PARAMS), dtype=torch.float32, device=DEV)
    l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l, prio=True):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in EIGHT + (PRIO if prio else ())}


def _same(a, b, keys=EIGHT + PRIO):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _learn(worlds, l, slots, n_steps=1):
    worlds.learn([l], n_steps, slots=np.ascontiguousarray(slots, np.int32).reshape(1, n_steps, l.batch))
    return _np(l, prio=l.priority is not None)


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


# ---- one tile is rl_learn_prioritized, bit for bit ----

@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("batch", pw.ONE_TILE_BATCHES)
def test_one_tile_is_rl_learn_prioritized_bit_for_bit(worlds, batch, moments):
    """Three steps on the wrapped fixture ring (capacity 96, count 250), the same slots, from fresh moments and from moments under way,
    once with the target copy: all eight learner buffers, the whole priority array and prio_max of rl_learn_prioritized_wide are those
    of rl_learn_prioritized from the same start."""
    g = dc.golden()
    slots = np.ascontiguousarray(g["slots"][:, :batch]).astype(np.int32)
    mk = lambda kind: _learner(3, batch, kind, ring=_ring(g, count=250), moments=moments, sync_target=batch == 33)  # noqa: E731
    ra, rb = _learn(worlds, mk("wide"), slots, 3), _learn(worlds, mk("narrow"), slots, 3)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [3, 1] and rb["grad"].any() and (rb["loss"] > 0).all()
    assert rb["params"].tobytes() != np.asarray(g["init"]).tobytes()
    assert (rb["target"].tobytes() == rb["params"].tobytes()) == (batch == 33)
    assert rb["prio_max"][0] == rb["priority"].max() > SENTINEL and (rb["priority"] != SENTINEL).sum() == len(np.unique(slots))
    _same(ra, rb)


@pytest.mark.parametrize("batch", pw.ONE_TILE_BATCHES)
def test_the_draw_at_one_tile_is_rl_learn_prioritized_draws_bit_for_bit(worlds, batch):
    """Equal memories with rows to stamp (seen 50 of 96, maximum 2.5) and weights over several orders of magnitude, zeros included: equal
    slot tables, priority, weight, keys and seen."""
    import torch
    g = dc.golden()
    out = []
    for kind in ("wide", "narrow"):
        l = _learner(1, batch, kind)
        l.priority.copy_(torch.as_tensor(pc.edge_priorities(96), device=DEV))
        l.seen.fill_(50)
        l.prio_max.fill_(2.5)
        slots = worlds.draw_prioritized([l], 1)
        torch.cuda.synchronize()
        assert tuple(slots.shape) == (1, 1, batch) and slots.dtype == torch.int32
        out.append({"slots": slots.cpu().numpy(), **{k: getattr(l, k).cpu().numpy().copy() for k in ("priority", "weight", "keys", "seen", "prio_max")}})
    worlds.check_error_flag()
    a, b = out
    assert b["seen"].tolist() == [96] and (b["priority"][50:] == 2.5).all() and b["prio_max"].tolist() == [2.5]
    assert b["slots"].min() >= 0 and b["slots"].max() < 96 and (b["weight"][b["slots"].reshape(-1)] > 0).all()
    assert np.array_equal(b["keys"].view(np.uint64), pc.content_keys(g, 96))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- several tiles: the update is rl_learn_dueling_wide's, the priorities are float64's ----
_wide = {}


def _wide_case(worlds, batch):
    """One step at `batch` on pw.case(batch)'s slots, once per batch: the PERD3QN learner through rl_learn_prioritized_wide and a D3QN
    learner with the same parameters, ring and slots through rl_learn_dueling_wide."""
    if batch not in _wide:
        slots = pw.case(batch)[0]
        _wide[batch] = (_learn(worlds, _learner(1, batch, "wide"), slots), _learn(worlds, _learner(1, batch, "d3qn"), slots))
        worlds.check_error_flag()
    return _wide[batch]


@pytest.mark.parametrize("batch", pw.MULTI_TILE_BATCHES)
def test_the_update_is_rl_learn_dueling_wides_bit_for_bit(worlds, batch):
    rp, rd = _wide_case(worlds, batch)
    assert rd["state"].tolist() == [1, 1] and rd["grad"].any() and rd["loss"][0] > 0
    assert rd["params"].tobytes() != dc.golden()["init"].tobytes()
    _same(rp, rd, keys=EIGHT)


@pytest.mark.parametrize("batch", pw.MULTI_TILE_BATCHES)
def test_the_priorities_of_every_batch_row_are_float64s_with_the_batch_wide_means(worlds, batch):
    """Every batch row's priority within 1e-5 of float64, relative to the batch's largest |q|, |q'| (tests/test_hip_learn_perd3qn.py's
    bar); the float64 value comes from learn_perd3qn_cases.priorities over the WHOLE batch.  Rows outside the batch keep their bits and
    prio_max is the maximum over [0, size), exactly."""
    rp, _ = _wide_case(worlds, batch)
    slots, p64, q, qn = pw.case(batch)
    scale = max(np.abs(q).max(), np.abs(qn).max())
    got = rp["priority"][slots]
    err = np.abs(got - p64).max() / scale
    print("batch %d: max |priority - float64| / scale %.3g (bar %g; scale %.4g), prio_max %.6g, %d distinct rows of 96 drawn"
          % (batch, err, pw.BAR, scale, rp["prio_max"][0], len(np.unique(slots))))
    assert err <= pw.BAR
    assert np.isfinite(got).all() and (got >= 0).all()
    rest = np.setdiff1d(np.arange(96), slots)
    assert (rp["priority"][rest] == SENTINEL).all() and (len(rest) > 0 or batch == 2048)
    assert rp["prio_max"][0] == rp["priority"][:96].max() > SENTINEL


# ---- duplicates across tiles and positions ----

def _stash(l, tiles):
    """The tiles' stash blocks of a learner's work buffer (include/reinlife_hip.h: header | partial[T] | sums | stash[T][896]) -> uint32 [T, 896]."""
    raw = l.work.cpu().numpy()
    off = wc.HEADER_BYTES + tiles * dc.N_PARAMS * 4 + (2 * tiles * 4 + 15) // 16 * 16
    n = tiles * wc.TILE * wc.STASH_FLOATS
    assert off + 4 * n == raw.size == wc.work_bytes(tiles * wc.TILE)
    return raw[off:].view(np.uint32).reshape(tiles, wc.TILE * wc.STASH_FLOATS).copy()


def _stash_rows(block):
    """A tile's stash [896] as rows [64, 14]: adv'[8], val', adv[a], val, reward, mask, action."""
    adv = block[:512].reshape(64, 8)
    return np.concatenate([adv, block[512:].reshape(6, 64).T], axis=1)


def test_a_second_tile_that_repeats_the_first_leaves_the_same_stash_and_mirrored_rows_are_equal(worlds):
    """Position does not leak into a row's forward arithmetic: batch 128 whose second tile repeats the first tile's 64 slots leaves two
    equal stash blocks, bit for bit; within one tile with rows j and 63 - j on the same slot the two stash rows are equal."""
    l = _learner(1, 128)
    s2 = pw.second_tile_repeats_the_first()
    r = _learn(worlds, l, s2)
    worlds.check_error_flag()
    st = _stash(l, 2)
    assert st.any() and (st != 0xA5A5A5A5).all()
    assert st[0].tobytes() == st[1].tobytes()
    assert len(np.unique(r["priority"][s2[:64]])) > 10 and r["state"].tolist() == [1, 1]
    m = _learner(1, 64)
    _learn(worlds, m, pw.mirrored_tile())
    worlds.check_error_flag()
    rows = _stash_rows(_stash(m, 1)[0])
    assert rows[:32].tobytes() == rows[:31:-1].tobytes() and len(np.unique(rows[:32, 8])) > 10


def test_a_slot_in_three_tiles_ends_with_one_value_in_every_run(worlds):
    """Batch 130 with one slot at positions 3, 70 and 129 (tiles 0, 1, 2): the three writes carry equal bits, so two runs give the same
    priority array -- and the value is float64's within the bar."""
    slots = pw.duplicate_across_tiles()
    ra, rb = _learn(worlds, _learner(1, 130), slots), _learn(worlds, _learner(1, 130), slots)
    worlds.check_error_flag()
    _same(ra, rb)
    g = dc.golden()
    p64, q, qn = pc.priorities(g["init"], g["target_init"], g, slots)
    scale = max(np.abs(q).max(), np.abs(qn).max())
    err = np.abs(ra["priority"][slots] - p64).max() / scale
    print("batch 130, slot 17 at 3 / 70 / 129: priority %.9g (float64 %.9g), worst row error / scale %.3g" % (ra["priority"][17], p64[3], err))
    assert err <= pw.BAR and np.ptp(p64[[3, 70, 129]]) <= 1e-12 * scale              # (float64's own rounding by position in the host's matrix product)
    assert ra["priority"][17] == rb["priority"][17] > SENTINEL


# ---- steps and short rings ----

def test_later_steps_overwrite_earlier_ones_and_a_short_ring_keeps_its_tail(worlds):
    """Two steps of batch 130 in one call leave what two single-step calls leave: a slot drawn in both steps ends with step 2's value,
    taken from the parameters step 1 left.  With count 70 of 96 the maximum runs over rows [0, 70) only."""
    slots = wc.slots_of(130, 2, seed=7)
    assert len(np.intersect1d(slots[0], slots[1])) > 10
    one = _learn(worlds, _learner(2, 130), slots, 2)
    l = _learner(1, 130)
    first = _learn(worlds, l, slots[0])
    second = _learn(worlds, l, slots[1])
    worlds.check_error_flag()
    _same(one, second, keys=("params", "target", "adam_m", "adam_v", "packed") + PRIO)
    assert one["state"].tolist() == [2, 1] and second["state"].tolist() == [2, 2]
    both = np.intersect1d(slots[0], slots[1])
    moved = one["priority"][both] != first["priority"][both]
    print("batch 130 x 2 steps: %d slots in both steps, %d of them end with other bits than step 1 wrote" % (len(both), int(moved.sum())))
    assert moved.any()
    only0 = np.setdiff1d(slots[0], slots[1])
    assert one["priority"][only0].tobytes() == first["priority"][only0].tobytes()
    short = _learner(1, 130, ring=_ring(dc.golden(), count=70), fill=0.0)
    short.priority[70:] = 9.0                                                            # (beyond the ring's size: never read)
    rs = _learn(worlds, short, wc.slots_of(130)[0] % 70)
    worlds.check_error_flag()
    assert 0 < rs["prio_max"][0] == rs["priority"][:70].max() < 9.0 and (rs["priority"][70:] == 9.0).all()


# ---- gate, target and bad slots ----

@pytest.mark.parametrize("sync", [False, True])
def test_below_the_size_gate_the_memory_and_the_parameters_stay_and_the_call_is_counted(worlds, sync):
    l = _learner(1, 130, min_size=96, sync_target=sync)
    l.prio_max.fill_(3.5)
    before = _np(l)
    after = _learn(worlds, l, wc.slots_of(130)[0])
    worlds.check_error_flag()
    _same(after, before, keys=("params", "adam_m", "adam_v", "packed", "grad", "loss") + PRIO)
    assert after["state"].tolist() == [0, 1] and after["prio_max"][0] == 3.5
    assert after["target"].tobytes() == (before["params"] if sync else before["target"]).tobytes()


def test_a_bad_slot_in_the_last_tile_of_the_last_step_is_flagged_and_that_brain_is_left_alone(worlds):
    """Batch 130, two steps, 96 (the ring's size) at the very last table index: error-flag code 6 with the learner, the step and the
    value; none of that learner's buffers is written -- priority and prio_max included -- and the healthy learner of the same call
    trains as it does alone.  (The check pass reads the table's VALUES before any row is fetched or any priority indexed.)"""
    import torch
    good = wc.slots_of(130, 2, seed=31)
    bad = good.copy()
    bad[1, 129] = 96
    healthy, broken = _learner(2, 130), _learner(2, 130, sync_target=True)
    broken.packed.mul_(0.5)
    broken.adam_m.fill_(0.25)
    broken.prio_max.fill_(1.75)
    before = _np(broken)
    worlds.err.zero_()
    worlds.learn([healthy, broken], 2, slots=np.stack([good, bad]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 1, 1, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(broken)
    _same(after, before)
    assert not after["grad"].any() and after["prio_max"][0] == 1.75 and (after["priority"] == SENTINEL).all()
    rs, rh = _learn(worlds, _learner(2, 130), good, 2), _np(healthy)
    worlds.check_error_flag()
    assert rh["state"].tolist() == [2, 1] and rh["params"].tobytes() != dc.golden()["init"].tobytes()
    _same(rh, rs)


# ---- independence and repeatability ----

def test_runs_repeat_and_the_last_of_sixteen_learners_is_the_learner_alone(worlds):
    g = dc.golden()
    slots = wc.slots_of(130, 2, seed=21)
    ra, rb = _learn(worlds, _learner(2, 130), slots, 2), _learn(worlds, _learner(2, 130), slots, 2)
    _same(ra, rb)
    others = [_learner(2, 130, flat=(g["init"] * np.float32(1.0 - 0.01 * i)).astype(np.float32)) for i in range(1, 16)]
    c = _learner(2, 130)
    table = np.stack([wc.slots_of(130, 2, seed=30 + i) for i in range(15)] + [slots]).astype(np.int32)
    worlds.learn(others + [c], 2, slots=table)
    rc, r0 = _np(c), _np(others[0])
    worlds.check_error_flag()
    _same(ra, rc)
    assert ra["state"].tolist() == [2, 1] and r0["state"].tolist() == [2, 1]
    assert r0["params"].tobytes() != ra["params"].tobytes() and r0["priority"].tobytes() != ra["priority"].tobytes()


def test_draws_and_training_at_batch_130_do_not_depend_on_the_order_of_the_ring(worlds):
    """The ring's rows permuted, the priorities following: the draw names other slots holding the SAME rows, and training on them ends
    with the same parameters, the same maximum and the same priorities row for row."""
    import torch
    g = dc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in dc.RING_KEYS}
    pri = pc.edge_priorities(96)
    a, b = _learner(1, 130), _learner(1, 130, ring=_ring(rows2))
    a.priority.copy_(torch.as_tensor(pri, device=DEV))
    b.priority.copy_(torch.as_tensor(pri[perm], device=DEV))                              # slot j of the permuted ring holds row perm[j]
    sa, sb = worlds.draw_prioritized([a], 1), worlds.draw_prioritized([b], 1)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (1, 1, 130) and sa.dtype == torch.int32
    assert np.array_equal(a.keys.cpu().numpy()[perm], b.keys.cpu().numpy())               # the content keys follow the rows
    sa, sb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert not np.array_equal(sa, sb) and np.array_equal(perm[sb], sa)
    assert (pri[sa] > 0).all() and 10 < len(np.unique(sa)) < 130
    ra, rb = _learn(worlds, a, sa), _learn(worlds, b, sb)
    worlds.check_error_flag()
    _same(ra, rb, keys=EIGHT + ("prio_max",))
    assert ra["priority"][perm].tobytes() == rb["priority"].tobytes() and ra["priority"].tobytes() != pri.tobytes()
    assert ra["state"].tolist() == [1, 1]


# ---- the draw at width ----

def test_2048_draws_times_3_steps_follow_priority_to_the_alpha_over_the_sum(worlds):
    """48 rows, priorities cycling through {0, 0.25, 1, 4}, 2048 x 3 draws in ONE call: a zero-priority row is never drawn, every other
    row's count lies within 5 binomial standard deviations of n w / sum w, w = p^0.6 -- the bound of the 6,400-draw test of
    rl_learn_prioritized_draw at this draw count (deterministic: this passes always or never; the host model passes it with the same
    seed, tests/test_learn_prioritized_wide_cpu.py)."""
    import torch
    g = dc.golden()
    l = _learner(1, pw.DRAW_BATCH, ring=_ring(g, capacity=pw.DRAW_ROWS))
    pri = pw.draw_priorities()
    l.priority.copy_(torch.as_tensor(pri.astype(np.float32), device=DEV))
    slots = worlds.draw_prioritized([l], pw.DRAW_STEPS).cpu().numpy()
    worlds.check_error_flag()
    n = pw.DRAW_BATCH * pw.DRAW_STEPS
    assert slots.shape == (1, pw.DRAW_STEPS, pw.DRAW_BATCH) and slots.min() >= 0 and slots.max() < pw.DRAW_ROWS
    counts = np.bincount(slots.reshape(-1), minlength=pw.DRAW_ROWS)
    want, sd = pw.draw_bound(n)
    z = np.abs(counts - want)[pri > 0] / sd[pri > 0]
    print("wide draw: counts by class %s, expected %s, worst deviation %.2f sd (bound %d)" % (
        [int(counts[pri == v].sum()) for v in (0.0, 0.25, 1.0, 4.0)], [round(float(want[pri == v].sum()), 1) for v in (0.0, 0.25, 1.0, 4.0)], z.max(), pw.DRAW_SD))
    assert counts.sum() == n and not counts[pri == 0].any()
    assert (z <= pw.DRAW_SD).all()
    assert not np.array_equal(slots[0, 0], slots[0, 1]) and not np.array_equal(slots[0, 1], slots[0, 2])   # (draw d = s * batch + j: other salts per step)


# ---- refusals ----

def test_mixed_entries_mixed_batches_and_d3qn_learners_are_refused(worlds):
    from reinlife_amd import _lib
    lib = _lib.lib()
    a, b, n, d = _learner(1, 130), _learner(1, 96), _learner(1, 64, "narrow"), _learner(1, 130, "d3qn")
    table = np.zeros((2, 1, 130), np.int32)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([a, n], 1, slots=table)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([a, d], 1, slots=table)
    with pytest.raises(ValueError, match="one kind"):
        worlds.draw_prioritized([_learner(1, 64), n], 1)
    with pytest.raises(ValueError, match="share one batch"):
        worlds.draw_prioritized([a, b], 1)
    with pytest.raises(ValueError, match="prioritised"):
        worlds.draw_prioritized([d], 1)
    with pytest.raises(_lib.ReinLifeHipError, match="rl_learn_prioritized_wide_draw"):
        worlds.learn([a], 1)                                                             # no slots: the draw is draw_prioritized()'s job
    # ... and at the C entry points: unequal batches, and a D3QN learner's structures
    slots = np.zeros(260, np.int32)
    import torch
    dev_slots = torch.as_tensor(slots, device=DEV)
    arr, rings = (_lib.Learner * 2)(a.struct(), b.struct()), (_lib.Replay * 2)(a.ring_struct(), b.ring_struct())
    prios = (_lib.Prio * 2)(a.prio_struct(), b.prio_struct())
    work = (C.c_void_p * 2)(a.work.data_ptr(), b.work.data_ptr())
    assert lib.rl_learn_prioritized_wide(worlds.handle, arr, rings, prios, 2, 1, dev_slots.data_ptr(), work, None) == -1
    assert b"rl_learn_prioritized_wide: learner 1: batch 96 differs" in lib.rl_last_error()
    assert lib.rl_learn_prioritized_wide_draw(worlds.handle, arr, rings, prios, 2, 1, dev_slots.data_ptr(), None) == -1
    assert b"rl_learn_prioritized_wide_draw: learner 1: batch 96 differs" in lib.rl_last_error()
    arr, rings = (_lib.Learner * 1)(d.struct()), (_lib.Replay * 1)(d.ring_struct())
    assert lib.rl_learn_prioritized_wide(worlds.handle, arr, rings, prios, 1, 1, dev_slots.data_ptr(), work, None) == -4
    assert b"kind %d" % _lib.D3QN in lib.rl_last_error() and b"RL_PERD3QN" in lib.rl_last_error()
    assert lib.rl_learn_prioritized_wide_draw(worlds.handle, arr, rings, prios, 1, 1, dev_slots.data_ptr(), None) == -4
    assert b"kind %d" % _lib.D3QN in lib.rl_last_error()
    worlds.check_error_flag()


# ---- the whole path: trainer(learn="device", learn_prioritized=True, learn_batch={"PERD3QN": B}) ----
_runs = {}


def _train(tmp=None, three=False, **kw):
    """One short trainer() run on 4 synthetic worlds, 30 episodes, learn_every 10: a DQN and a PERD3QN brain (exploration 5,
    soft_update_freq 20: it trains after episodes 10, 20 and 30, its target synced at 20 alone); three=True adds a D3QN brain on the same
    schedule (learn_kinds DQN and D3QN).  Runs without a folder to save into are made once per keyword set."""
    import torch
    from reinlife_amd import Models, trainer
    key = tuple(sorted((k, tuple(sorted(v.items())) if isinstance(v, dict) else v) for k, v in kw.items())) + (three,)
    if tmp is None and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    sched = dict(exploration=5, soft_update_freq=20)
    brains = [Models.DQN(max_epi=30)] + ([Models.D3QN(**sched)] if three else []) + [Models.PERD3QN(**sched)]
    init = [b.state_dict_flat().copy() for b in brains]
    if three:
        kw = dict(kw, learn_kinds=("DQN", "D3QN"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=30, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      learn_every=10, learn_prioritized=True, save=tmp is not None, print_results=False, **kw)
    k = len(brains) - 1
    count, capacity = int(env.worlds.replays[k]["count"].item()), int(env.worlds.replays[k]["state"].shape[0])
    assert 130 <= count < capacity == 10000, (count, capacity)   # (no wrap: the rows a draw sees do not depend on append order)
    out = (env, brains, init)
    if tmp is None:
        _runs[key] = out
    return out


def _bits(l):
    """A learner's buffers as bytes; the priorities sorted (the rows' slots differ from run to run, their priorities do not)."""
    import torch
    torch.cuda.synchronize()
    out = {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS}
    if l.priority is not None:
        out["priority"] = np.sort(l.priority.cpu().numpy()).tobytes()
        out["prio_max"], out["seen"] = l.prio_max.cpu().numpy().tobytes(), l.seen.cpu().numpy().tobytes()
    return out


def _equal_envs(a, b):
    assert sorted(a.learners) == sorted(b.learners)
    for k in a.learners:
        ba, bb = _bits(a.learners[k]), _bits(b.learners[k])
        assert sorted(ba) == sorted(bb)
        for n in ba:
            assert ba[n] == bb[n], (k, n)
    assert a.tracker.results == b.tracker.results


def test_learn_batch_perd3qn_64_is_the_run_without_the_key():
    env, _, _ = _train()
    env64, _, _ = _train(learn_batch={"PERD3QN": 64})
    assert [env.learners[k].entry for k in (0, 1)] == ["rl_learn", "rl_learn_prioritized"]
    assert [env64.learners[k].entry for k in (0, 1)] == ["rl_learn", "rl_learn_prioritized_wide"]
    assert env.learn_batch is None and env64.learn_batch == {"PERD3QN": 64}
    assert env.learners[1].state.cpu().tolist() == env64.learners[1].state.cpu().tolist() == [3, 3]
    assert float(env.learners[1].prio_max.item()) > 0 and (env.learners[1].priority.cpu().numpy() > 0).any()
    _equal_envs(env, env64)


def test_learn_batch_perd3qn_130_trains_saves_and_repeats(tmp_path, monkeypatch):
    import torch
    from reinlife_amd import _lib
    env, brains, init = _train(learn_batch={"PERD3QN": 130})
    l = env.learners[1]
    assert l.entry == "rl_learn_prioritized_wide" and l.batch == 130 and l.min_size == 0 and l.state.cpu().tolist() == [3, 3]
    count = int(env.worlds.replays[1]["count"].item())
    pri, pmax, seen = l.priority.cpu().numpy(), float(l.prio_max.item()), int(l.seen.item())
    print("PERD3QN at batch 130: ring count %d, seen %d, prio_max %.6g, rows re-prioritised among the seen: %d" % (count, seen, pmax, int((pri[:seen] != pmax).sum())))
    assert 0 < seen <= count and pmax == pri[:count].max() > 0
    assert (pri[:seen] != pmax).any() and (pri[:seen] > 0).all() and not pri[count:].any()
    now, target = brains[1].state_dict_flat(), l.target.cpu().numpy()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1]) and now.tobytes() == l.params.cpu().numpy().tobytes()
    assert not np.array_equal(target, init[1]) and not np.array_equal(target, now)       # synced at 20, not at 30
    packed = np.zeros(_lib.lib().rl_policy_packed_floats(_lib.PERD3QN), np.float32)
    assert _lib.lib().rl_policy_pack_weights(_lib.PERD3QN, np.ascontiguousarray(now).ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    assert l.packed.cpu().numpy().tobytes() == packed.tobytes() and env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()
    env64, brains64, _ = _train(learn_batch={"PERD3QN": 64})
    assert brains64[1].state_dict_flat().tobytes() != now.tobytes()                       # a wider batch is another update
    note = env._weights_note()
    assert "rl_learn_prioritized_wide" in note and "batch 130" in note and "rl_learn:" in note
    # a second identical call gives the same bits, and save=True writes the trained weights
    monkeypatch.chdir(tmp_path)
    env2, brains2, init2 = _train(tmp=tmp_path, learn_batch={"PERD3QN": 130})
    _equal_envs(env, env2)
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "PERD3QN", "brain_gene_*.pt")))
    assert len(files) == 1
    flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(files[0]).values()])
    assert flat.tobytes() == brains2[1].state_dict_flat().tobytes() == now.tobytes() and not np.array_equal(flat, init2[1])
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_prioritized_wide" in settings and '"Learn batch": {"PERD3QN": 130}' in settings.replace("\n", "").replace("  ", "")


def test_learn_batch_perd3qn_130_under_the_identity_merge():
    """learn_ranks="average" on one rank without a process group: export, merge and repack after every learning episode change no bit."""
    env, _, _ = _train(learn_batch={"PERD3QN": 130})
    envm, _, _ = _train(learn_batch={"PERD3QN": 130}, learn_ranks="average")
    assert envm.learn_ranks == "average" and envm.learn_now_calls == env.learn_now_calls == 3
    _equal_envs(env, envm)


def test_beside_dqn_and_d3qn_learners_the_key_changes_nothing_of_theirs():
    """DQN, D3QN and PERD3QN brains learning in shared worlds: with {"PERD3QN": 64} the PERD3QN learner is a wide one and ends with the
    narrow one's bits, so the worlds stay the same and the DQN and D3QN learners end with the bits they have without the key; at 130 all
    three train."""
    env, _, _ = _train(three=True)
    env64, _, _ = _train(three=True, learn_batch={"PERD3QN": 64})
    assert [env.learners[k].entry for k in (0, 1, 2)] == ["rl_learn", "rl_learn_dueling", "rl_learn_prioritized"]
    assert [env64.learners[k].entry for k in (0, 1, 2)] == ["rl_learn", "rl_learn_dueling", "rl_learn_prioritized_wide"]
    assert env.learners[1].state.cpu().tolist() == [3, 3] == env.learners[2].state.cpu().tolist() and env.learners[0].state.cpu().tolist()[0] > 0
    _equal_envs(env, env64)
    wide, brains, init = _train(three=True, learn_batch={"PERD3QN": 130, "D3QN": 96})
    assert [wide.learners[k].entry for k in (0, 1, 2)] == ["rl_learn", "rl_learn_dueling_wide", "rl_learn_prioritized_wide"]
    assert (wide.learners[1].batch, wide.learners[2].batch) == (96, 130)
    assert wide.learners[1].state.cpu().tolist() == [3, 3] == wide.learners[2].state.cpu().tolist()
    for k in (0, 1, 2):
        now = brains[k].state_dict_flat()
        assert np.isfinite(now).all() and not np.array_equal(now, init[k])
