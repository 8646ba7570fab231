"""CPU: the host model of the replay rings (tests/capture_ring_cases.py) and the premises of tests/test_hip_capture_ring.py.  The one-world
rule is the reference's deque(maxlen=capacity); the block rule is shown on hand-made lists (a block that ends exactly at the ring's end,
one that straddles it, a start count of 2**32 - 100) and shown to notice what it is there to notice (a torn row, a run out of order, a
written slot outside the block); the table's rows, on the oracle alone under seeded random actions, reach what they are in the table for;
and both capture entry points refuse a ring below n_worlds * slot_cap by name before anything is launched."""
import collections
import ctypes as C

import numpy as np
import pytest

import capture_ring_cases as cr
from reinlife_amd import _lib


def _rows(rng, n, with_prob=False):
    """n distinct hand-made transitions as packed rows."""
    tx = dict(state=rng.randint(-1, 2, size=(n, cr.OBS)).astype(np.float32), state_prime=rng.randint(-1, 2, size=(n, cr.OBS)).astype(np.float32),
              reward=rng.choice([0.0, 0.3, -1.0, 5.0], size=n).astype(np.float32), age=rng.randint(2, 50, size=n).astype(np.int32),
              action=rng.randint(0, 8, size=n).astype(np.int8), done=(rng.random_sample(n) < 0.2).astype(np.uint8))
    return cr.pack_rows(tx, prob=rng.random_sample(n).astype(np.float32) if with_prob else None)


@pytest.mark.parametrize("capacity,count0", [(7, 0), (257, 0), (257, 200), (300, 2 ** 32 - 100), (64, 63), (1, 5)])
def test_the_one_world_rule_is_the_reference_deque(capacity, count0):
    """Rows fed in call order to collections.deque(maxlen=capacity) (DQN.py:15 / D3QN.py:62): what the deque holds, oldest first, is what
    the rule leaves in the slots behind the newest row, and count0 only turns the ring."""
    rng = np.random.RandomState(capacity)
    before = _rows(rng, capacity)
    for n in (0, 1, capacity - 1, capacity, capacity + 1, 3 * capacity + 2):
        rows = _rows(rng, n)
        dq = collections.deque((r.tobytes() for r in before[(count0 + np.arange(capacity)) % capacity]), maxlen=capacity)   # the ring, oldest first
        for r in rows:
            dq.append(r.tobytes())
        after = cr.expect_one_world(before, count0, rows)
        oldest_first = after[(count0 + n + np.arange(capacity)) % capacity]
        assert [r.tobytes() for r in oldest_first] == list(dq), (capacity, count0, n)
        assert cr.check_one_world(before, after, count0, count0 + n, rows)["rows"] == n
        if n:
            wrong = after.copy()
            wrong[(count0 + n - 1) % capacity, 0] ^= 1
            with pytest.raises(AssertionError, match="slots differ"):
                cr.check_one_world(before, wrong, count0, count0 + n, rows)
            with pytest.raises(AssertionError, match="count"):
                cr.check_one_world(before, after, count0, count0 + n + 1, rows)


def _fill(before, count0, runs, order):
    """The ring after the runs were appended in `order` from count0 on (what the atomics of a launch may produce)."""
    after, pos = before.copy(), count0
    for i in order:
        after[(pos + np.arange(len(runs[i]))) % len(before)] = runs[i]
        pos += len(runs[i])
    return after, pos


@pytest.mark.parametrize("capacity,count0,lens,why", [
    (100, 70, (10, 0, 15, 5), "a block that ends exactly at the ring's end"),
    (100, 70, (10, 17, 15, 5), "a block that straddles the ring's end, inside a run"),
    (127, 2 ** 32 - 100, (40, 43, 30), "a start count of 2**32 - 100: the block passes 2**32"),
    (64, 5, (64,), "one run that fills the whole ring"),
    (257, 0, (0, 0), "nothing appended"),
])
@pytest.mark.parametrize("with_prob", [False, True], ids=["rows", "rows+prob"])
def test_the_block_rule_on_hand_made_lists(capacity, count0, lens, why, with_prob):
    rng = np.random.RandomState(len(lens) + capacity)
    before = _rows(rng, capacity, with_prob)
    runs = [_rows(rng, n, with_prob) for n in lens]
    total = sum(lens)
    for order in (range(len(runs)), reversed(range(len(runs)))):           # worlds in any order
        after, count1 = _fill(before, count0, runs, list(order))
        got = cr.check_block(before, after, count0, count1, runs, why)
        assert got == dict(rows=total, runs=sum(1 for n in lens if n), placed=sum(1 for n in lens if n)), why
        if why.startswith("a block that ends exactly"):
            assert (count0 + total) % capacity == 0
        if why.startswith("a block that straddles"):
            assert count0 % capacity + total > capacity
        if why.startswith("a start count"):
            assert count0 < 2 ** 32 < count1
    if not total:
        return
    after, count1 = _fill(before, count0, runs, range(len(runs)))
    first = next(i for i, n in enumerate(lens) if n)
    last_slot = (count0 + total - 1) % capacity
    # a torn row: the state of one transition with the reward of another
    torn = after.copy()
    torn[last_slot, 2 * cr.OBS * 4] ^= 0x40
    with pytest.raises(AssertionError, match="not the launch's transitions: 1 rows of the oracle's list missing, 1 rows that are none"):
        cr.check_block(before, torn, count0, count1, runs)
    with pytest.raises(AssertionError, match="count"):
        cr.check_block(before, after, count0, count1 - 1, runs)
    if total < capacity:      # a slot outside the block was written
        out = after.copy()
        out[(count0 + total) % capacity, 3] ^= 1
        with pytest.raises(AssertionError, match="outside the launch's block"):
            cr.check_block(before, out, count0, count1, runs)
    if lens[first] >= 3:      # the rows of a run in another order: the same multiset, not the call order
        swapped = after.copy()
        a, b = (count0 + 1) % capacity, (count0 + 2) % capacity
        swapped[[a, b]] = swapped[[b, a]]
        with pytest.raises(AssertionError, match="not one contiguous stretch"):
            cr.check_block(before, swapped, count0, count1, runs)
    with pytest.raises(AssertionError, match="outside the rule"):
        cr.check_block(before[: total - 1], after[: total - 1], count0, count1, runs)


def test_a_run_whose_first_row_occurs_twice_is_checked_as_a_multiset_only():
    rng = np.random.RandomState(2)
    before = _rows(rng, 50)
    a = _rows(rng, 6)
    b = np.concatenate([a[:1], _rows(rng, 4)])             # begins with the row a begins with
    after, count1 = _fill(before, 45, [a, b], [1, 0])
    assert cr.check_block(before, after, 45, count1, [a, b]) == dict(rows=11, runs=2, placed=0)


def test_count_foreign_counts_the_rows_that_are_no_whole_transition():
    rng = np.random.RandomState(3)
    pool = _rows(rng, 200)
    ring = pool[rng.randint(0, 200, size=64)].copy()
    assert cr.count_foreign(ring, 1000, pool) == 0
    ring[5, 2 * cr.OBS * 4 + 1] ^= 1
    ring[9, 0] ^= 1
    assert cr.count_foreign(ring, 1000, pool) == 2 and cr.count_foreign(ring, 6, pool) == 1


def test_reach_counts_laps_straddles_and_crossings():
    # one world, capacity 10: ticks of 4 rows from count 7: [7,11) straddles, [11,15), [15,19), [19,23) straddles
    f = cr.reach(np.full((4, 1, 1), 4), (10,), 7, (1, 3))[0]
    assert f == dict(total=16, laps=2, straddles=2, crossings=2, most_tick=4, most_launch=12)
    # a reservation that ends exactly at the ring's end does not straddle it
    f = cr.reach(np.full((2, 1, 1), 5), (10,), 0, (1, 1))[0]
    assert f["straddles"] == 0 and f["crossings"] == 0 and f["laps"] == 1
    # several worlds: launches are counted, not reservations (their order within a tick is the atomics')
    f = cr.reach(np.full((4, 3, 1), 2), (10,), 2 ** 32 - 4, (2, 2))[0]
    assert f == dict(total=24, laps=2, straddles=0, crossings=2, most_tick=2, most_launch=12)


@pytest.mark.parametrize("row", cr.TABLE, ids=[r.name for r in cr.TABLE])
@pytest.mark.parametrize("n_brains", [2, 3])
def test_the_table_reaches_what_its_rows_are_for(row, n_brains):
    """Conditions on the inputs, on the oracle alone under seeded random actions: a seed that misses one is replaced, the floors stay.  Each
    wrapping ring laps at least 3 times; a reservation straddles the ring's end at least 3 times (one world: the order of the reservations is
    the ticks'; several worlds: a launch's block crosses the end that often -- which world's run the end falls into is the atomics' order);
    the crowded row appends more than 64 rows of its world to one ring in one tick; every multi-world launch stays within capacity.  The GPU
    file asserts the same floors on the trajectories the device's own actions give."""
    caps = cr.capacities(row, n_brains)
    assert len(caps) == n_brains and min(caps) >= cr.floor_rows(row.worlds, row.slot_cap)      # (no ring of the table is overfull)
    counts = cr.count_rows(cr.run_oracle_random(row, n_brains), n_brains)
    figures = cr.reach(counts, caps, row.count0, row.chunks)
    print(row.name, n_brains, "brains: rows per tick and brain", counts.sum(1).min(0).tolist(), "..", counts.sum(1).max(0).tolist(), figures)
    cr.assert_reach(row, caps, figures, row.name)
    if row.worlds > 1:
        assert max(row.chunks) <= 3 and len(row.chunks) >= 16
    if row.name == "one-world-2^32":
        assert row.count0 == 2 ** 32 - 100 and figures[1]["laps"] == 0 and figures[0]["laps"] >= 3


# ---------------------------------------------------------------------------------------------------------------------
# the floor: a ring holds at least what one tick of all worlds can append to it (n_worlds * slot_cap rows)
# ---------------------------------------------------------------------------------------------------------------------
def _bound_handle(n_worlds, slot_cap=256, n_brains=2):
    """A handle bound to host memory that no kernel will ever see: the checks below all end before a launch."""
    lib, h = _lib.lib(), C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, n_brains, slot_cap, n_worlds, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    backing = (C.c_uint8 * 64)()
    state = _lib.State(*[C.addressof(backing)] * len(_lib.STATE_FIELDS))
    assert lib.rl_bind_state(h, C.byref(state)) == 0
    return lib, h, backing


def _rings(capacities):
    p = C.c_void_p(0x1000)
    return (_lib.Replay * len(capacities))(*[_lib.Replay(p, p, p, p, p, None, p, p, c) for c in capacities])


@pytest.mark.parametrize("n_worlds,slot_cap", [(1, 256), (4, 256), (6, 512), (256, 256)])
def test_both_entry_points_refuse_a_ring_below_the_floor_by_name(n_worlds, slot_cap):
    """rl_run_ex (given replays) and rl_capture_transitions at floor - 1: RL_E_INVALID naming the ring, its capacity and the floor, decided
    on the host before anything is launched (there is no device here, and the pointers are dummies).  At the floor rl_run_ex passes its
    checks (n_ticks = 0 returns behind them); rl_capture_transitions at the floor launches, so that half is in tests/test_hip_capture_ring.py."""
    lib, h, backing = _bound_handle(n_worlds, slot_cap)
    floor = cr.floor_rows(n_worlds, slot_cap)
    p = C.c_void_p(0x1000)
    brains = (_lib.Brain * 2)(_lib.Brain(_lib.PERD3QN, 0.0, p), _lib.Brain(_lib.D3QN, 0.2, p))
    pair = (C.c_void_p * 2)(p, p)
    step = _lib.StepOut(*[p] * len(_lib.STEP_OUT_FIELDS))
    try:
        for caps, ring in (([floor, floor - 1], 1), ([floor - 1, 10 * floor], 0)):
            rings = _rings(caps)
            says = ("replay %d: capacity %d is below the floor of %d rows (n_worlds %d x slot_cap %d" % (ring, floor - 1, floor, n_worlds, slot_cap)).encode()
            opts = _lib.RunOpts(70, 100, None, None, 0, 0, C.cast(rings, C.c_void_p), None)
            for n_ticks in (0, 5):
                assert lib.rl_run_ex(h, brains, 2, n_ticks, p, C.byref(step), pair, 0, None, C.byref(opts), None) == -1
                assert lib.rl_last_error().startswith(b"rl_run: ") and says in lib.rl_last_error(), lib.rl_last_error()
            assert lib.rl_capture_transitions(h, p, p, None, C.byref(step), rings, 2, None) == -1
            assert lib.rl_last_error().startswith(b"rl_capture_transitions: ") and says in lib.rl_last_error(), lib.rl_last_error()
        rings = _rings([floor, floor])
        opts = _lib.RunOpts(70, 100, None, None, 0, 0, C.cast(rings, C.c_void_p), None)
        assert lib.rl_run_ex(h, brains, 2, 0, p, C.byref(step), pair, 0, None, C.byref(opts), None) == 0
        rings[0].capacity = 0           # (an incomplete ring is still named as such)
        assert lib.rl_run_ex(h, brains, 2, 0, p, C.byref(step), pair, 0, None, C.byref(opts), None) == -1 and b"replay 0 incomplete" in lib.rl_last_error()
        assert lib.rl_capture_transitions(h, p, p, None, C.byref(step), rings, 2, None) == -1 and b"replay 0 incomplete" in lib.rl_last_error()
    finally:
        lib.rl_destroy(h)


def test_the_existing_callers_stay_above_the_floor():
    """tests/test_hip_api.py captures into 700 rows at 1 world and 5,000 at 6 worlds, tests/test_hip_round3.py into 40,000 at 9 worlds (all
    30x30 with 100 agents: slot_cap 256); the reference's ring sizes at the world counts the training tests run."""
    cap = _lib.slot_cap_for(100)
    assert cap == 256
    assert cr.floor_rows(1, cap) == 256 <= 700 and cr.floor_rows(6, cap) == 1536 <= 5000 and cr.floor_rows(9, cap) == 2304 <= 40_000
    assert cr.floor_rows(2, cap) <= 10_000 and cr.floor_rows(2, _lib.slot_cap_for(50)) == 256      # trainer(n_worlds=2): D3QN / PERD3QN rings
    for row in cr.TABLE:
        assert row.slot_cap == _lib.slot_cap_for(row.max_agents)


def _recording_worlds():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("record_learner_layer", os.path.join(root, "tools", "record_learner_layer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool.RecordingWorlds


def test_environment_sizes_each_ring_to_its_rows_or_the_floor(monkeypatch):
    """Environment(learn="device"): each ring is max(its rows today, n_worlds * slot_cap), exposed as ring_rows / ring_floor; when nothing is
    below the floor the enable_capture call is the one it always was (a scalar BUFFER_LIMIT for DQN brains, the brains' capacities else)."""
    import warnings
    from reinlife_amd import Models
    from reinlife_amd.World import environment as envmod
    monkeypatch.setattr(envmod, "DeviceWorlds", _recording_worlds())

    def env(brains, n_worlds, **kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return envmod.Environment(brains=brains, n_worlds=n_worlds, max_agents=100, rng="philox", learn="device", print_results=False, **kw)
    e = env([Models.D3QN(capacity=300), Models.D3QN(capacity=300)], 4, learn_kinds="D3QN")
    assert e.ring_floor == 4 * 256 and e.ring_rows == [1024, 1024] and e.worlds.capture == [[1024, 1024], False]
    assert [int(l.ring["state"].shape[0]) for l in e.learners.values()] == [1024, 1024]
    e = env([Models.D3QN(), Models.D3QN(capacity=300)], 4, learn_kinds="D3QN")
    assert e.ring_rows == [10_000, 1024] and e.worlds.capture == [[10_000, 1024], False]
    e = env([Models.D3QN(), Models.D3QN(capacity=1024)], 4, learn_kinds="D3QN")          # at the floor: untouched
    assert e.ring_rows == [10_000, 1024] and e.worlds.capture == [[10_000, 1024], False]
    e = env([Models.DQN(), Models.DQN()], 4)                                              # DQN.py:15's 50,000, one number as before
    assert e.ring_rows == [50_000, 50_000] and e.worlds.capture == [50_000, False]
    e = env([Models.DQN(), Models.D3QN()], 256, learn_kinds=("DQN", "D3QN"))             # 256 worlds: 65,536 rows per tick at the most
    assert e.ring_floor == 65_536 and e.ring_rows == [65_536, 65_536] and e.worlds.capture == [[65_536, 65_536], False]
