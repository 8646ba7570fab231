"""GPU: rl_learn_td_stamp / DeviceWorlds.stamp_td / trainer(learn_td_priority=True, learn_td_stamp="error") -- the TD-error priority
PERDQN.py:113-128 spells out for a stored row, made on the device for the rows appended since the last draw.  Checked against float64
forward passes through the formula (the bar tests/test_hip_learn_perdqn.py holds rl_learn_td's write-back to: 3.8e-5 x scale + 4 ulp),
bit for bit against what rl_learn_td writes for the same rows from the same parameters, window by window against the host rule
(learn_perdqn_cases.stamp) over a sentinel, on done rows, on a permuted ring, on rings of 1,025 and 20,000 rows, with 16 learners in
one call, twice in a row, in front of both draws, and through trainer().  Every figure a bar is held against is printed first."""
import warnings

import numpy as np
import pytest

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc
import learn_prio_rank_cases as prc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
GAMMA = 0.99
SENTINEL = np.float32(2.0 ** -20)
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.PERDQN()
    with torch.no_grad():
        for p, v in zip(b.model.parameters(), tc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, count=None, capacity=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture lays one out; the ages are the rows' ("ring_age") or 0."""
    import torch
    capacity = rows["ring_state"].shape[0] if capacity is None else capacity
    t = lambda a, dt: torch.as_tensor(np.array(a[:capacity]), device=DEV).to(dt)  # noqa: E731
    age = rows["ring_age"] if "ring_age" in rows else np.zeros(capacity, np.int32)
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": t(age, torch.int32),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, target_flat, ring, seen=0, fill=SENTINEL, batch=64):
    """A PERDQN learner on the given networks whose memory holds `fill` (an array: those priorities) and has seen `seen` rows; its size
    gate is open and its target stays where it is."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(_brain(flat), DEV, ring=ring, td_priority=True)
    assert (l.entry, l.gamma, l.prio_e, l.prio_a) == ("rl_learn_td", GAMMA, 0.01, 0.6)
    assert np.float32(l.p_new).tobytes() == tc.golden()["p_new"].tobytes() and l.priority.numel() == ring["state"].shape[0]
    if np.ndim(fill):
        l.priority.copy_(torch.as_tensor(np.array(fill, np.float32), device=DEV))
    else:
        l.priority.fill_(float(fill))
    l.seen.fill_(int(seen))
    l.batch, l.min_size, l.sync_target = batch, 0, False
    l.target.copy_(torch.as_tensor(np.array(target_flat, np.float32), device=DEV))
    return l


def _pri(l):
    import torch
    torch.cuda.synchronize()
    return l.priority.cpu().numpy().copy()


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


_ref = {}


def _float64(flat, target_flat, rows, tag):
    """(priorities, scale) in float64 through the formula, once per case: scale is the rows' largest |Q(s)|, |Q_target(s')| or |target|."""
    if tag not in _ref:
        import torch
        n = rows["ring_state"].shape[0]
        ring = {k: rows[k] for k in dc.RING_KEYS}
        pred, target = tc.pred_target(tc.net_of(flat), tc.net_of(target_flat), ring, np.arange(n), GAMMA, torch.float64)
        pri = (np.abs((pred - target).detach().numpy()) + 0.01) ** 0.6
        scale = max(np.abs(tc.q_values(flat, rows["ring_state"])).max(), np.abs(tc.q_values(target_flat, rows["ring_state_prime"])).max(),
                    np.abs(target.numpy()).max())
        pri.setflags(write=False)
        _ref[tag] = (pri, float(scale))
    return _ref[tag]


def _hold_to_float64(got, pri64, scale, tag):
    err = np.abs(got.astype(np.float64) - pri64)
    ulp = np.spacing(np.abs(got)).astype(np.float64)
    bound = 3.8e-5 * scale + 4 * ulp
    worst = int(np.argmax(err / bound))
    print("%s: %d rows, scale %.4g; max |priority - float64| %.3g; worst row %d: error %.3g against %.3g (3.8e-5 x scale + 4 ulp), priority %.6g"
          % (tag, len(got), scale, err.max(), worst, err[worst], bound[worst], got[worst]))
    assert np.isfinite(got).all() and (err <= bound).all(), tag


@pytest.fixture(scope="module")
def stamped(worlds):
    """The fixture's 96-row ring stamped whole (seen 0, count 96) over a sentinel, once: the priorities, and seen afterwards."""
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g))
    before = worlds.launches
    worlds.stamp_td([l])
    pri = _pri(l)
    worlds.check_error_flag()
    assert worlds.launches - before == 2
    pri.setflags(write=False)
    return {"priority": pri, "seen": int(l.seen.item()), "learner": l}


# ---- 1. the arithmetic -------------------------------------------------------------------------------------------------------------
def test_a_whole_ring_stamp_matches_float64_through_the_formula(stamped):
    g, p = dc.golden(), tc.golden()
    pri64, scale = _float64(p["init"], p["target_init"], g, "fixture")
    got = stamped["priority"]
    assert stamped["seen"] == 96 and not (got.view(np.uint32) == SENTINEL.view(np.uint32)).any()
    assert not (got.view(np.uint32) == p["p_new"].view(np.uint32)).any() and got.max() / got.min() > 10
    _hold_to_float64(got, pri64, scale, "fixture ring")
    st = stamped["learner"]
    assert st.state.cpu().tolist() == [0, 0] and st.beta_is.item() == 0.4           # the stamp is no learning call
    assert st.params.cpu().numpy().tobytes() == p["init"].tobytes() and st.target.cpu().numpy().tobytes() == p["target_init"].tobytes()


def test_a_stamped_priority_is_what_rl_learn_td_writes_for_the_row_bit_for_bit(worlds, stamped):
    """Fresh copies of the learner make one-step rl_learn_td calls on rows 0..63 and 32..95: priority[slot] of the batch rows has the
    stamp's bits -- the stamp's dot products are rl_learn_td's, term for term."""
    g, p = dc.golden(), tc.golden()
    for lo in (0, 32):
        slots = np.arange(lo, lo + 64, dtype=np.int32)
        l = _learner(p["init"], p["target_init"], _ring(g), seen=96, fill=p["prio_init"])
        worlds.learn([l], 1, slots=slots.reshape(1, 1, 64))
        got = _pri(l)
        worlds.check_error_flag()
        assert l.state.cpu().tolist() == [1, 1]
        diff = int((got[slots].view(np.uint32) != stamped["priority"][slots].view(np.uint32)).sum())
        print("rows %d..%d: %d of 64 priorities differ in bits from the stamp's" % (lo, lo + 63, diff))
        assert got[slots].tobytes() == stamped["priority"][slots].tobytes(), lo
        rest = np.setdiff1d(np.arange(96), slots)
        assert got[rest].tobytes() == p["prio_init"][rest].tobytes()


# ---- 2. windows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity, seen, count", [
    (96, 0, 1), (96, 5, 68), (96, 0, 64), (96, 10, 75),            # windows of 1, 63, 64 and 65 rows, no wrap
    (96, 90, 100), (96, 60, 125), (96, 95, 96 + 64),               # across the wrap: 10, 65 (two workgroups) and 65 rows
    (96, 3, 120), (96, 0, 96), (96, 0, 5000), (70, 10, 80),        # count - seen >= capacity: the whole ring
    (96, 7, 7), (96, 0, 0), (96, 300, 300), (96, 9, 4),            # empty windows (also of an empty ring, and seen ahead of count)
    (96, 200, 230), (96, 1000, 1063), (65, 130, 194),              # a ring that wrapped before
])
def test_exactly_the_window_is_stamped(worlds, stamped, capacity, seen, count):
    """Priorities pre-filled with a sentinel: exactly the slots the host rule of the draws' stamp names change -- to the bits the
    whole-ring stamp gave the row, which sits in the same slot here -- the rest keep theirs, and seen == count afterwards."""
    g, p = dc.golden(), tc.golden()
    l = _learner(p["init"], p["target_init"], _ring(g, count=count, capacity=capacity), seen=seen)
    worlds.stamp_td([l])
    got = _pri(l)
    worlds.check_error_flag()
    named = tc.stamp(np.full(capacity, SENTINEL, np.float32), seen, max(count, seen), np.float32(1.0)) == 1.0
    assert named.sum() == (min(count, capacity) if count - seen >= capacity else max(count - seen, 0))
    want = np.where(named, stamped["priority"][:capacity], SENTINEL)
    assert got.tobytes() == want.tobytes(), (np.nonzero(got != want)[0][:8], got[got != want][:8])
    assert int(l.seen.item()) == count


# ---- 3. rows -----------------------------------------------------------------------------------------------------------------------
def test_done_rows_take_the_reward_as_their_target(worlds):
    """Every row done: the priorities do not depend on s' at all (other s' rows give the same bits) and are the formula's with
    target == reward."""
    g, p = dc.golden(), tc.golden()
    rows = {k: np.array(g[k][:96]) for k in dc.RING_KEYS}
    rows["ring_done"] = np.ones(96, np.uint8)
    other = dict(rows, ring_state_prime=np.ascontiguousarray(rows["ring_state_prime"][::-1] * np.float32(3.0)))
    a, b = _learner(p["init"], p["target_init"], _ring(rows)), _learner(p["init"], p["target_init"], _ring(other))
    worlds.stamp_td([a]); worlds.stamp_td([b])
    pa, pb = _pri(a), _pri(b)
    worlds.check_error_flag()
    assert pa.tobytes() == pb.tobytes() and not (pa == SENTINEL).any()
    q = tc.q_values(p["init"], rows["ring_state"])[np.arange(96), rows["ring_action"].astype(np.int64)]
    pri64 = (np.abs(q - rows["ring_reward"].astype(np.float64)) + 0.01) ** 0.6
    scale = max(np.abs(tc.q_values(p["init"], rows["ring_state"])).max(), np.abs(rows["ring_reward"]).max())
    _hold_to_float64(pa, pri64, float(scale), "all rows done")


def test_a_permuted_ring_gives_every_row_the_same_bits(worlds, stamped):
    g, p = dc.golden(), tc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows = {k: np.ascontiguousarray(g[k][:96][perm]) for k in dc.RING_KEYS}       # slot j holds row perm[j]
    l = _learner(p["init"], p["target_init"], _ring(rows))
    worlds.stamp_td([l])
    got = _pri(l)
    worlds.check_error_flag()
    assert got.tobytes() == stamped["priority"][perm].tobytes() and got.tobytes() != stamped["priority"].tobytes()


def test_a_repeated_call_on_an_unchanged_ring_changes_nothing(worlds, stamped):
    import torch
    l = stamped["learner"]
    worlds.stamp_td([l])
    assert _pri(l).tobytes() == stamped["priority"].tobytes() and int(l.seen.item()) == 96
    l.priority.fill_(float(SENTINEL))                                               # (no window: not one row is written)
    worlds.stamp_td([l])
    assert (_pri(l) == SENTINEL).all() and int(l.seen.item()) == 96
    l.priority.copy_(torch.as_tensor(np.array(stamped["priority"]), device=DEV))
    worlds.check_error_flag()


# ---- 4. long rings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1025, 20000])
def test_long_rings_are_stamped_whole(worlds, n):
    """n seeded rows (learn_cases.edge_ring_rows) on the reference's trained weights: 17 workgroups with one row in the last, and 313
    with 32 in the last.  All rows meet the float64 bar; 64 random rows equal rl_learn_td's write-back bit for bit."""
    w, tgt, _, _, _ = tc.edge_case()
    rows = lc.edge_ring_rows(n, 5)
    l = _learner(w, tgt, _ring(rows))
    worlds.stamp_td([l])
    got = _pri(l)
    worlds.check_error_flag()
    assert int(l.seen.item()) == n and not (got == SENTINEL).any()
    pri64, scale = _float64(w, tgt, rows, "edge%d" % n)
    _hold_to_float64(got, pri64, scale, "ring of %d rows" % n)
    slots = np.random.RandomState(n).choice(n, 64, replace=False).astype(np.int32)
    slots[0], slots[1] = n - 1, 0
    t = _learner(w, tgt, _ring(rows), seen=n, fill=1.0)
    worlds.learn([t], 1, slots=slots.reshape(1, 1, 64))
    back = _pri(t)
    worlds.check_error_flag()
    assert t.state.cpu().tolist() == [1, 1]
    assert back[slots].tobytes() == got[slots].tobytes()


# ---- 5. many learners --------------------------------------------------------------------------------------------------------------
def test_sixteen_learners_of_one_call_each_equal_their_stamp_alone(worlds):
    """16 learners with different ring sizes, windows, networks and batches in ONE call: every priority array and seen are those of
    the learner's stamp alone; the grid is the largest ring's, so most workgroups of the small rings return at once."""
    w, tgt, _, _, _ = tc.edge_case()
    rows = lc.edge_ring_rows(1027, 11)
    cases = []
    for i in range(16):
        cap = (1, 63, 64, 65, 130, 257, 701, 1027)[i % 8]
        seen, count = ((0, cap), (cap // 2, cap + cap // 3), (0, cap // 2 + 1), (5 * cap, 5 * cap), (3, 3 + 2 * cap))[i % 5]
        flat = (w * np.float32(1.0 - 0.01 * i)).astype(np.float32)
        at = i if i + cap <= 1027 else 0
        cases.append((flat, {k: v[at:at + cap] for k, v in rows.items()}, seen, count, 1 + (i * 5) % 64))

    def make():
        return [_learner(flat, tgt, _ring(r, count=count), seen=seen, batch=batch) for flat, r, seen, count, batch in cases]
    together, alone = make(), make()
    worlds.stamp_td(together)
    for l in alone:
        worlds.stamp_td([l])
    worlds.check_error_flag()
    changed = 0
    for i, (a, b) in enumerate(zip(together, alone)):
        pa, pb = _pri(a), _pri(b)
        assert pa.tobytes() == pb.tobytes(), i
        assert int(a.seen.item()) == int(b.seen.item()) == cases[i][3], i
        named = tc.stamp(np.full(len(pa), SENTINEL, np.float32), cases[i][2], cases[i][3], np.float32(1.0)) == 1.0
        assert np.array_equal(pa != SENTINEL, named), i
        changed += int(named.sum())
    assert changed > 0
    with pytest.raises(ValueError, match="1 to 16 learners"):
        worlds.stamp_td(together + alone[:1])
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    with pytest.raises(ValueError, match="PERDQN"):
        worlds.stamp_td([DeviceLearner(Models.DQN(max_epi=60), DEV, ring=_ring(dc.golden()))])


# ---- 6. in front of the draws ------------------------------------------------------------------------------------------------------
def test_the_draws_behind_a_stamp_stamp_nothing_and_draw_by_the_priorities_found(worlds, stamped):
    """rl_learn_td_draw and rl_learn_td_draw_rank, unchanged code, behind a stamp: every priority keeps its bits (no row gets p_new)
    and the slots are the host rules' for these priorities."""
    from reinlife_amd import _lib
    g, p = dc.golden(), tc.golden()
    keys = pc.content_keys(g, 96)
    for ranked in (False, True):
        l = _learner(p["init"], p["target_init"], _ring(g, count=96 + 40), seen=70, fill=p["prio_init"])   # a window across the wrap
        l.state[1] = 3
        worlds.stamp_td([l])
        after_stamp = _pri(l)
        named = tc.stamp(np.zeros(96, np.float32), 70, 136, np.float32(1.0)) == 1.0
        assert after_stamp[named].tobytes() == stamped["priority"][named].tobytes() and after_stamp[~named].tobytes() == p["prio_init"][~named].tobytes()
        before = worlds.launches
        slots = (worlds.draw_td_rank if ranked else worlds.draw_td)([l], 2).cpu().numpy().reshape(-1)
        assert worlds.launches - before == (8 if ranked else 2)
        assert _pri(l).tobytes() == after_stamp.tobytes() and int(l.seen.item()) == 136
        assert np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
        if ranked:
            want = prc.host_draw(keys, after_stamp, SEED, 0, 3, _lib.SITE_LEARN_TD, 2, 64, True)[0]
        else:
            want = tc.host_draw(keys, after_stamp, SEED, 0, 3, 128)
        assert np.array_equal(slots, want), ranked
        worlds.check_error_flag()


# ---- 7. trainer() ------------------------------------------------------------------------------------------------------------------
_runs = {}


def _train(stamp, fresh=False, **kw):
    """trainer([PERDQN, DQN], 40 episodes, 2 worlds, train_start 200, learn_td_priority=True): tests/test_hip_learn_perdqn.py's run."""
    import torch
    from reinlife_amd import Models, trainer
    key = (stamp,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if not fresh and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.PERDQN(), Models.DQN(max_epi=60)]
    brains[0].train_start = 200
    more = {"learn_td_stamp": stamp} if stamp else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=40, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device", save=False,
                      print_results=False, learn_td_priority=True, **more, **kw)
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
    return out


def _watch(monkeypatch, log):
    from reinlife_amd.worlds import DeviceWorlds
    for name in ("stamp_td", "draw_td", "draw_td_rank", "draw_slots", "learn"):
        def wrap(original, name):
            def watched(self, learners, *a, **k):
                log.append((name, [l.entry for l in learners]))
                return original(self, learners, *a, **k)
            return watched
        monkeypatch.setattr(DeviceWorlds, name, wrap(getattr(DeviceWorlds, name), name))


@pytest.mark.parametrize("ranked", [False, True], ids=["race", "rank"])
def test_trainer_with_the_key_stamps_in_front_of_every_perdqn_draw_and_repeats(ranked, monkeypatch):
    kw = dict(learn_draw={"PERDQN": "rank"}) if ranked else {}
    log = []
    _watch(monkeypatch, log)
    env = _train("error", fresh=True, **kw)
    monkeypatch.undo()
    draw = "draw_td_rank" if ranked else "draw_td"
    td = [c for c in log if c[1] == ["rl_learn_td"]]
    assert [c[0] for c in td] == ["stamp_td", draw, "learn"] * 2 and env.learn_now_calls == 2 and env.learn_td_stamp == "error"
    assert [c for c in log if c[1] != ["rl_learn_td"]] == [("draw_slots", ["rl_learn"]), ("learn", ["rl_learn"])] * 2
    l = env.learners[0]
    count, seen, pri = int(env.worlds.replays[0]["count"].item()), int(l.seen.item()), l.priority.cpu().numpy()
    distinct = len(np.unique(pri[:seen]))
    print("%s draw: ring count %d, seen %d, state %s, %d distinct priorities among the %d rows seen, min %.4g max %.4g"
          % (draw, count, seen, l.state.cpu().tolist(), distinct, seen, pri[:seen].min(), pri[:seen].max()))
    assert 200 <= seen <= count < 20000 and l.state.cpu().tolist() == [2, 2]
    assert (pri[:seen] > 0).all() and np.isfinite(pri).all() and not pri[seen:].any()
    assert not (pri.view(np.uint32) == np.float32(l.p_new).view(np.uint32)).any()    # the ring holds no p_new
    assert distinct > 10                                                             # (and no other constant: that would be one value)
    env.worlds.check_error_flag()
    note = env._weights_note()
    assert "rl_learn_td_stamp" in note and "rl_learn_td" in note
    again = _train("error", fresh=True, **kw)
    assert _bits(env) == _bits(again) and env.tracker.results == again.tracker.results and env.worlds.launches == again.worlds.launches
    plain = _train(None, **kw)
    assert env.worlds.launches - plain.worlds.launches == 2 * 2                      # two launches per learning call
    assert _bits(env)[0]["params"] != _bits(plain)[0]["params"]                      # other priorities: other rows, other parameters


def test_trainer_without_the_key_makes_the_calls_it_made(monkeypatch):
    """The run without the key, watched: no stamp is ever queued, the PERDQN calls are draw_td then learn, every fresh row got p_new and
    only rows rl_learn_td trained on differ from it; it ends on the bits of the unwatched run and counts its launches."""
    log = []
    _watch(monkeypatch, log)
    env = _train(None, fresh=True)
    monkeypatch.undo()
    assert [c[0] for c in log if c[1] == ["rl_learn_td"]] == ["draw_td", "learn"] * 2 and not any(c[0] == "stamp_td" for c in log)
    assert env.learn_td_stamp is None and "rl_learn_td_stamp" not in env._weights_note()
    l = env.learners[0]
    seen, pri = int(l.seen.item()), l.priority.cpu().numpy()
    assert 0 < (pri[:seen] != np.float32(l.p_new)).sum() <= 128 and not pri[seen:].any()
    plain = _train(None)
    assert _bits(env) == _bits(plain) and env.worlds.launches == plain.worlds.launches and env.tracker.results == plain.tracker.results
