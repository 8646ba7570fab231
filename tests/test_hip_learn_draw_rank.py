"""GPU: rl_learn_draw_rank / DeviceWorlds.draw_slots_rank / trainer(learn_draw="rank") -- uniform minibatch draws by content-key rank.
Everything is integers, so every comparison is exact: the keys are learn_perd3qn_cases.content_keys, the order numpy's lexsort by
(key, slot), and every slot the host rule's (learn_rank_cases.host_rank_draw)."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_cases as lc
import learn_perd3qn_cases as pc
import learn_rank_cases as rc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
BATCHES = (1, 32, 37, 64, 2048)
_edge = {}


def _rows(n, seed=11):
    """(n seeded rows with ages 0..199, their content keys)"""
    if (n, seed) not in _edge:
        rows = lc.edge_ring_rows(n, seed)
        _edge[(n, seed)] = (rows, pc.content_keys(rows, n, rows["ring_age"]))
    return _edge[(n, seed)]


def _take(rows, index):
    return {k: np.ascontiguousarray(v[index]) for k, v in rows.items()}


def _ring(rows, count=None):
    """A replay ring on the device from host rows with their ages, as DeviceWorlds.enable_capture lays one out."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": t(rows["ring_age"], torch.int32),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


_brain = []


def _learner(ring, batch, calls=0, wide=False):
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    if not _brain:
        torch.manual_seed(5)
        _brain.append(Models.DQN())
    l = DeviceLearner(_brain[0], DEV, ring=ring, **({"wide_batch": batch} if wide else {}))
    l.batch, l.min_size = batch, 0
    l.state[1] = calls
    return l


def _prefill(l, value=-1):
    """After a first draw has allocated the learner's rank buffers: overwrite keys / order so that what a call leaves alone shows."""
    l.keys.fill_(value)
    l.rank_order.fill_(value)
    l.rank_work.fill_(0xA5)      # the scratch needs no initialisation: start every call from garbage


def _draw(worlds, learners, n_steps):
    import torch
    got = worlds.draw_slots_rank(learners, n_steps)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _check_learner(l, keys, size, tag=""):
    """keys[:size] are the content keys and order[:size] the lexsort; both are left alone from `size` on (they hold -1 there)."""
    got_keys = l.keys.cpu().numpy().view(np.uint64)
    got_order = l.rank_order.cpu().numpy()
    assert np.array_equal(got_keys[:size], keys[:size]), tag
    assert np.array_equal(got_order[:size], rc.host_order(keys[:size])), tag
    assert (got_keys[size:] == np.uint64(2 ** 64 - 1)).all() and (got_order[size:] == -1).all(), tag


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


# (rows a ring holds, its capacity, its counter): full rings, count < capacity, and wrapped rings (count > capacity, size == capacity)
RINGS = [(1, 1, 1), (1, 3, 1), (2, 2, 2), (2, 2, 7), (31, 31, 31), (31, 40, 31), (1025, 1025, 1025), (1025, 1025, 5000), (1025, 1500, 1025),
         (10_000, 10_000, 10_000), (10_000, 10_000, 25_000), (10_000, 10_007, 10_000)]


@pytest.mark.parametrize("size, capacity, count", RINGS)
def test_keys_order_and_every_slot_are_the_host_rules(worlds, size, capacity, count):
    """Batches 1, 32, 37, 64 and 2048 with 1 and 5 steps each on one ring: keys == content_keys, order[:size] == lexsort((slot, key)), all
    n_steps x batch slots == order[(x_d * size) >> 32]; rows, keys and order beyond `size` take no part and are not written."""
    rows, keys = _rows(capacity)
    assert min(count, capacity) == size
    if size == 10_000:   # step 4 (the placement inside a bucket) works on natural data: many buckets of two or more rows
        shared = size - len(np.unique(keys[:size] >> np.uint64(48)))
        print("10,000 rows: %d rows share a bucket with an earlier one" % shared)
        assert shared >= 100 and len(np.unique(keys[:size])) == size
    l = _learner(_ring(rows, count=count), 1)
    _draw(worlds, [l], 1)
    for batch in BATCHES:
        for n_steps, calls in ((1, 0), (5, 3)):
            l.batch = batch
            l.state[1] = calls
            _prefill(l)
            got = _draw(worlds, [l], n_steps)
            assert got.shape == (1, n_steps, batch) and got.dtype == np.int32
            want = rc.host_rank_draw(keys[:size], SEED, 0, calls, n_steps * batch)
            assert np.array_equal(got.reshape(-1), want), (batch, n_steps)
            _check_learner(l, keys, size, (batch, n_steps))
    assert l.rank_work.numel() == rc.work_bytes(capacity) and l.rank_work.data_ptr() % 16 == 0
    worlds.check_error_flag()


def test_a_ring_of_identical_rows_is_one_bucket_and_keeps_slot_order(worlds):
    """1025 copies of one row: one bucket holds the ring, every comparison is a tie, order is 0 .. size - 1 and the draw is rl_learn's own."""
    from reinlife_amd.learn import philox_slots
    rows, _ = _rows(1025)
    same = _take(rows, np.zeros(1025, np.int64))
    keys = pc.content_keys(same, 1025, same["ring_age"])
    assert len(set(keys.tolist())) == 1
    l = _learner(_ring(same), 64)
    _draw(worlds, [l], 1)
    _prefill(l)
    got = _draw(worlds, [l], 5)
    assert np.array_equal(l.rank_order.cpu().numpy(), np.arange(1025, dtype=np.int32))
    assert np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(got[0], philox_slots(SEED, 0, 0, 5, 64, 1025))          # rank == slot here
    worlds.check_error_flag()


def test_rows_that_occur_twice_sit_side_by_side_lower_slot_first(worlds):
    """1025 rows: 513 distinct ones, 512 of them a second time, shuffled by a fixed permutation.  In `order` the two slots of a pair are
    neighbours, the lower slot first."""
    rows, _ = _rows(1025)
    perm = np.random.RandomState(3).permutation(1025)
    source = np.concatenate([np.arange(513), np.arange(512)])[perm]               # slot -> the distinct row it holds
    twice = _take(rows, source)
    keys = pc.content_keys(twice, 1025, twice["ring_age"])
    assert len(set(keys.tolist())) == 513
    l = _learner(_ring(twice), 37)
    _draw(worlds, [l], 1)
    _prefill(l)
    got = _draw(worlds, [l], 5)
    order = l.rank_order.cpu().numpy()
    assert np.array_equal(order, rc.host_order(keys))
    place = np.empty(1025, np.int64)
    place[order] = np.arange(1025)
    for r in range(512):
        a, b = np.nonzero(source == r)[0]
        assert a < b and place[b] == place[a] + 1, r
    assert np.array_equal(got.reshape(-1), rc.host_rank_draw(keys, SEED, 0, 0, 5 * 37))
    worlds.check_error_flag()


def _raw(worlds, learners, n_steps, slots):
    """rl_learn_draw_rank through the C ABI into the caller's own `slots` tensor."""
    import torch
    from reinlife_amd import _lib
    n = len(learners)
    arr = (_lib.Learner * n)(*[l.struct() for l in learners])
    rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
    keys, order, work = ((C.c_void_p * n)(*[getattr(l, name).data_ptr() for l in learners]) for name in ("keys", "rank_order", "rank_work"))
    _lib.check(worlds.lib.rl_learn_draw_rank(worlds.handle, arr, rings, n, n_steps, keys, order, work, C.c_void_p(slots.data_ptr()), worlds._stream()),
               "rl_learn_draw_rank")
    torch.cuda.synchronize()


def test_an_empty_ring_gives_slot_0_everywhere(worlds):
    """count == 0: every one of the n_steps x batch entries is WRITTEN with 0 (the table starts as -7), the guard entries behind it keep
    their -7, and keys and order are left alone."""
    import torch
    rows, _ = _rows(31)
    l = _learner(_ring(rows, count=0), 37)
    _draw(worlds, [l], 1)
    _prefill(l)
    slots = torch.full((5 * 37 + 64,), -7, dtype=torch.int32, device=DEV)
    _raw(worlds, [l], 5, slots)
    got = slots.cpu().numpy()
    assert (got[:5 * 37] == 0).all() and (got[5 * 37:] == -7).all()
    assert (l.rank_order.cpu().numpy() == -1).all() and (l.keys.cpu().numpy() == -1).all()
    worlds.check_error_flag()


def test_the_rows_drawn_do_not_depend_on_the_order_of_the_ring(worlds):
    """The same 1025 rows, ages included, in another order: other slots, the same rows -- keys_a[slots_a] == keys_b[slots_b] draw by draw."""
    rows, keys = _rows(1025)
    perm = np.random.RandomState(7).permutation(1025)
    moved = _take(rows, perm)
    a, b = _learner(_ring(rows), 64, calls=2), _learner(_ring(moved), 64, calls=2)
    sa, sb = _draw(worlds, [a], 5).reshape(-1), _draw(worlds, [b], 5).reshape(-1)
    ka, kb = a.keys.cpu().numpy().view(np.uint64), b.keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(ka, keys) and np.array_equal(kb, keys[perm])
    assert not np.array_equal(sa, sb) and len(np.unique(sa)) > 200
    assert np.array_equal(ka[sa], kb[sb])
    assert np.array_equal(perm[sb], sa)                                            # (distinct keys: the very same rows)
    worlds.check_error_flag()


@pytest.mark.parametrize("first", [0, 1])
def test_learners_of_different_batches_and_ring_sizes_in_one_call(worlds, first):
    """rl_learn_draw_rank through the C ABI with (batch 2048, 1025 rows of a ring of 1500) and (batch 37, 31 rows) in one call of 5 steps,
    in either order: the tables lie end to end in a buffer of exactly sum(n_steps * batch) entries plus 64 guard entries that keep their
    -7, each table the host rule's at its learner's own index (the index keys the Philox draw); keys and order are bit for bit what
    the learner gets in a call of its own."""
    import torch
    cases = [(2048, _rows(1500), 1025, 3), (37, _rows(31, seed=12), 31, 1)]
    cases = [cases[first], cases[1 - first]]
    together = [_learner(_ring(rows, count=size), batch, calls) for batch, (rows, _), size, calls in cases]
    alone = [_learner(_ring(rows, count=size), batch, calls) for batch, (rows, _), size, calls in cases]
    for l in together:
        _draw(worlds, [l], 1)      # (allocates the learner's keys, order and scratch)
        _prefill(l)
    slots = torch.full((5 * 2048 + 5 * 37 + 64,), -7, dtype=torch.int32, device=DEV)
    _raw(worlds, together, 5, slots)
    got = slots.cpu().numpy()
    assert (got[5 * 2048 + 5 * 37:] == -7).all()
    off = 0
    for i, (batch, (_, keys), size, calls) in enumerate(cases):
        assert np.array_equal(got[off:off + 5 * batch], rc.host_rank_draw(keys[:size], SEED, i, calls, 5 * batch)), i
        off += 5 * batch
        _draw(worlds, [alone[i]], 5)
        for name in ("keys", "rank_order"):
            assert getattr(together[i], name).cpu().numpy()[:size].tobytes() == getattr(alone[i], name).cpu().numpy()[:size].tobytes(), (i, name)
    with pytest.raises(ValueError, match="share one batch size"):
        worlds.draw_slots_rank(together, 5)
    worlds.check_error_flag()


def test_the_sixteenth_learner_of_a_call_draws_what_it_draws_alone(worlds):
    """RL_MAX_CAPTURE_BRAINS = 16 learners in one call (fifteen on a 31-row ring, the last on 1025 rows): the learner at index 15 gets
    the keys and the order it gets alone, and the host rule's slots at index 15; a seventeenth is refused."""
    small, _ = _rows(31, seed=12)
    rows, keys = _rows(1025)
    shared = _ring(small)
    learners = [_learner(shared, 32) for _ in range(15)] + [_learner(_ring(rows), 32, calls=4)]
    got = _draw(worlds, learners, 5)
    assert got.shape == (16, 5, 32)
    assert np.array_equal(got[15].reshape(-1), rc.host_rank_draw(keys, SEED, 15, 4, 160))
    solo = _learner(_ring(rows), 32, calls=4)
    alone = _draw(worlds, [solo], 5)
    assert np.array_equal(solo.rank_order.cpu().numpy(), learners[15].rank_order.cpu().numpy())
    assert np.array_equal(solo.keys.cpu().numpy(), learners[15].keys.cpu().numpy())
    assert np.array_equal(alone.reshape(-1), rc.host_rank_draw(keys, SEED, 0, 4, 160))
    with pytest.raises(ValueError, match="1 to 16 learners"):
        worlds.draw_slots_rank(learners + [solo], 5)
    worlds.check_error_flag()


def test_a_second_identical_call_gives_identical_order_and_slots(worlds):
    """10,000 rows, batch 2048, 5 steps, twice -- with the scratch overwritten in between: the same bits in order, keys and slots."""
    rows, keys = _rows(10_000)
    l = _learner(_ring(rows), 2048)
    a = _draw(worlds, [l], 5)
    oa, ka = l.rank_order.cpu().numpy().copy(), l.keys.cpu().numpy().copy()
    l.rank_work.fill_(0x3C)
    b = _draw(worlds, [l], 5)
    assert a.tobytes() == b.tobytes() and oa.tobytes() == l.rank_order.cpu().numpy().tobytes() and ka.tobytes() == l.keys.cpu().numpy().tobytes()
    assert worlds.launches >= 2 * rc.RANK_LAUNCHES
    before = worlds.launches
    _draw(worlds, [l], 1)
    assert worlds.launches - before == rc.RANK_LAUNCHES == 6


def test_rl_learn_wide_trains_on_the_table_and_the_next_draw_follows_the_call_counter(worlds):
    """A wide DQN learner (batch 96, 2 steps) fed the rank draw's table trains with error flag 0; the learning call advances state[1],
    and the next draw is the host rule's for calls = 1 -- other slots than the first."""
    import torch
    rows, keys = _rows(1025)
    l = _learner(_ring(rows), 96, wide=True)
    assert l.entry == "rl_learn_wide"
    before = l.params.cpu().numpy().copy()
    worlds.err.zero_()
    slots = worlds.draw_slots_rank([l], 2)
    worlds.learn([l], 2, slots=slots)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist()[0] == 0
    worlds.check_error_flag()
    first = slots.cpu().numpy().reshape(-1)
    assert np.array_equal(first, rc.host_rank_draw(keys, SEED, 0, 0, 192))
    assert l.state.cpu().tolist() == [2, 1] and not np.array_equal(l.params.cpu().numpy(), before) and np.isfinite(l.params.cpu().numpy()).all()
    second = _draw(worlds, [l], 2).reshape(-1)
    assert np.array_equal(second, rc.host_rank_draw(keys, SEED, 0, 1, 192)) and not np.array_equal(first, second)


# ---- the whole path: trainer(learn="device", learn_draw="rank", ...) ----
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
_runs = {}


def _train(tmp=None, d3qn=False, fresh=False, **kw):
    """One short trainer() run of two DQN brains on 4 synthetic worlds, as tests/test_hip_learn_wide.py's (d3qn: a DQN and a D3QN brain
    on 2 worlds, as tests/test_hip_learn_d3qn.py's -- the D3QN's ring of 10,000 rows does not wrap there); runs without a folder to save
    into are made once per keyword set unless `fresh`."""
    import torch
    from reinlife_amd import Models, trainer
    key = (d3qn,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if tmp is None and not fresh and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.D3QN(exploration=20, soft_update_freq=40) if d3qn else Models.DQN(max_epi=60)]
    init = [b.state_dict_flat().copy() for b in brains]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=60, n_worlds=2 if d3qn else 4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      save=tmp is not None, print_results=False, **kw)
    out = (env, brains, init)
    if tmp is None and not fresh:
        _runs[key] = out
    return out


def _bits(env):
    import torch
    torch.cuda.synchronize()
    return {k: {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS} for k, l in env.learners.items()}


def test_trainer_learn_draw_rank_with_learn_batch_96_trains_repeats_and_counts_its_launches(tmp_path, monkeypatch):
    env, brains, init = _train(learn_batch=96, learn_draw="rank")
    plain, _, _ = _train(learn_batch=96)
    assert env.learn_draw == "rank" and plain.learn_draw is None and env.learn_now_calls == plain.learn_now_calls == 3
    for k, b in enumerate(brains):
        l = env.learners[k]
        count, capacity = int(l.ring["count"].item()), int(l.ring["state"].shape[0])
        assert 1000 < count <= capacity                      # no chunk appended more than a ring holds: the rows repeat from run to run
        assert l.entry == "rl_learn_wide" and l.batch == 96 and l.rank_order is not None and l.rank_work.numel() == rc.work_bytes(capacity)
        steps, calls = l.state.cpu().tolist()
        assert steps > 0 and steps % 5 == 0 and calls == 3, (steps, calls)
        now = b.state_dict_flat()
        assert not np.array_equal(now, init[k]) and np.isfinite(now).all()
    env.worlds.check_error_flag()
    assert env.worlds.err.cpu().tolist()[0] == 0
    # another sampler: other parameters than the run without the keyword -- whose draw calls number one per learning episode here
    assert _bits(env)[0]["params"] != _bits(plain)[0]["params"]
    assert env.worlds.launches - plain.worlds.launches == (rc.RANK_LAUNCHES - 2) * env.learn_now_calls
    # a second identical call ends on the same bits
    monkeypatch.chdir(tmp_path)
    env2, brains2, _ = _train(tmp=tmp_path, learn_batch=96, learn_draw="rank")
    assert _bits(env) == _bits(env2) and env.tracker.results == env2.tracker.results and env.worlds.launches == env2.worlds.launches
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert '"Learn draw": "rank"' in settings and "rl_learn_draw_rank" in settings and '"Learn batch": 96' in settings
    # without the keyword the note on the weights says nothing of it
    assert "rl_learn_draw_rank" in env._weights_note() and "rl_learn_draw_rank" not in plain._weights_note()


def test_trainer_learn_draw_rank_with_dqn_and_d3qn_learners_trains_repeats_and_counts_its_launches():
    kw = dict(d3qn=True, learn_kinds=("DQN", "D3QN"))
    env, brains, init = _train(learn_draw="rank", **kw)
    plain, _, _ = _train(**kw)
    assert {l.entry for l in env.learners.values()} == {"rl_learn", "rl_learn_dueling"} and env.learn_now_calls == 3
    for k, b in enumerate(brains):
        l = env.learners[k]
        count, capacity = int(l.ring["count"].item()), int(l.ring["state"].shape[0])
        assert count <= capacity, (k, count, capacity)       # no ring wrapped: the rows repeat from run to run
        assert l.state.cpu().tolist()[0] > 0 and l.rank_order is not None, k
        now = b.state_dict_flat()
        assert not np.array_equal(now, init[k]) and np.isfinite(now).all()
    env.worlds.check_error_flag()
    assert env.worlds.err.cpu().tolist()[0] == 0
    draw_calls = sum(int(l.state[1].item()) for l in env.learners.values())      # one draw per learning call: a call per kind here
    assert draw_calls == sum(int(l.state[1].item()) for l in plain.learners.values()) == 5       # the DQN's three, the D3QN's after 40 and 60
    assert env.worlds.launches - plain.worlds.launches == (rc.RANK_LAUNCHES - 2) * draw_calls
    a = _bits(env)
    assert a[0]["params"] != _bits(plain)[0]["params"] and a[1]["params"] != _bits(plain)[1]["params"]
    env2, _, _ = _train(fresh=True, learn_draw="rank", **kw)
    assert env2 is not env and a == _bits(env2) and env.tracker.results == env2.tracker.results
