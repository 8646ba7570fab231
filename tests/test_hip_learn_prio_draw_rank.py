"""GPU: rl_learn_prioritized_draw_rank / rl_learn_td_draw_rank / DeviceWorlds.draw_prioritized_rank / draw_td_rank /
trainer(learn_draw={...}) -- prioritised minibatch draws by prefix sum over content-key rank.  Every comparison with the host rule
(learn_prio_rank_cases) is exact: the keys are integers, the cumulative sum has a fixed association order, and the targets are single
rounded float64 operations.  The weights are read back from the device (its powf is not numpy's)."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_cases as lc
import learn_perd3qn_cases as pc
import learn_prio_rank_cases as prc
import learn_rank_cases as rc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
_edge, _brains = {}, {}


def _rows(n, seed=11):
    """(n seeded rows with ages 0..199, their content keys)"""
    if (n, seed) not in _edge:
        rows = lc.edge_ring_rows(n, seed)
        _edge[(n, seed)] = (rows, pc.content_keys(rows, n, rows["ring_age"]))
    return _edge[(n, seed)]


def _golden48():
    """The first 48 rows of the DQN fixture ring (ages 0) and their keys: the rows of the counting tests."""
    if "g48" not in _edge:
        g = lc.golden()
        rows = {k: np.ascontiguousarray(g[k][:48]) for k in ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")}
        _edge["g48"] = (rows, pc.content_keys(rows, 48))
    return _edge["g48"]


def _take(rows, index):
    return {k: np.ascontiguousarray(v[index]) for k, v in rows.items()}


def _ring(rows, count=None):
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None,
            "age": t(rows["ring_age"], torch.int32) if "ring_age" in rows else torch.zeros(capacity, dtype=torch.int32, device=DEV),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(td, ring, batch, priority=None, calls=0, seen=None, wide=None):
    """A PERDQN (td) or wide PERD3QN learner on `ring` with an open gate; the memory holds `priority` (default: edge_priorities), and
    nothing is new to stamp (seen = count) unless `seen` says otherwise."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    if not _brains:
        torch.manual_seed(5)
        _brains.update(td=Models.PERDQN(), prio=Models.PERD3QN())
    if td:
        l = DeviceLearner(_brains["td"], DEV, ring=ring, td_priority=True)
        assert l.entry == "rl_learn_td"
    else:
        l = DeviceLearner(_brains["prio"], DEV, ring=ring, prioritized=True, prioritized_batch=wide or 64)
        assert l.entry == "rl_learn_prioritized_wide" and l.alpha == 0.6
    capacity = ring["state"].shape[0]
    l.batch, l.min_size = batch, 0
    l.state[1] = calls
    l.priority.copy_(torch.as_tensor(pc.edge_priorities(capacity) if priority is None else np.asarray(priority, np.float32), device=DEV))
    l.seen.copy_(ring["count"]) if seen is None else l.seen.fill_(seen)
    return l


def _site(td):
    from reinlife_amd import _lib
    return _lib.SITE_LEARN_TD if td else _lib.SITE_LEARN_PRIO


def _draw(worlds, td, learners, n_steps, stratified):
    import torch
    got = (worlds.draw_td_rank if td else worlds.draw_prioritized_rank)(learners, n_steps, stratified=stratified)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _weights(l, td):
    return (l.priority if td else l.weight).cpu().numpy()


def _check(l, td, keys, size, brain, calls, n_steps, batch, stratified, got, tag=""):
    """keys, order, cum and every slot are the host rule's, bit for bit, from the weights as the device left them."""
    got_keys = l.keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(got_keys[:size], keys[:size]), tag
    w32 = _weights(l, td)[:size]
    slots, ranks, order, cum = prc.host_draw(keys[:size], w32, SEED, brain, calls, _site(td), n_steps, batch, stratified)
    assert np.array_equal(l.rank_order.cpu().numpy()[:size], order), tag
    assert l.rank_cum.cpu().numpy()[:size].tobytes() == cum.tobytes(), tag
    assert np.array_equal(np.asarray(got).reshape(-1), slots), tag
    return slots, ranks, order, cum


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


# (rows a ring holds, its capacity, its counter): the sizes around the segment length, more than one block, and a wrapped ring
RINGS = [(1, 1, 1), (2, 2, 2), (63, 63, 63), (64, 64, 64), (65, 70, 65), (129, 129, 129), (1025, 1025, 5000), (10_000, 10_000, 10_000)]


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
@pytest.mark.parametrize("size, capacity, count", RINGS)
def test_keys_order_cum_and_every_slot_are_the_host_rules(worlds, size, capacity, count, td):
    """Batches 1, 64, 65 and 2048 (PERDQN: 1 and 64), independent and stratified, 1 and 3 steps: keys == content_keys, order ==
    lexsort((slot, key)), cum == the segment-of-64 rule on the device's own weights, every slot == searchsorted(cum, target, "right")
    with the clamp rule; order, cum and keys beyond `size` are not written; the weight column is powf(priority, alpha) to float32
    rounding and the priorities stay (nothing to stamp)."""
    rows, keys = _rows(capacity)
    assert min(count, capacity) == size
    l = _learner(td, _ring(rows, count=count), 1)
    pri = l.priority.cpu().numpy().copy()
    _draw(worlds, td, [l], 1, False)
    for batch in ((1, 64) if td else (1, 64, 65, 2048)):
        for stratified in (False, True):
            for n_steps, calls in ((1, 0), (3, 2)):
                l.batch = batch
                l.state[1] = calls
                l.rank_order.fill_(-1)
                l.rank_cum.fill_(-1.0)
                l.keys.fill_(-1)
                l.rank_work.fill_(0xA5)      # the scratch needs no initialisation
                got = _draw(worlds, td, [l], n_steps, stratified)
                assert got.shape == (1, n_steps, batch) and got.dtype == np.int32
                tag = (batch, stratified, n_steps)
                slots, ranks, order, cum = _check(l, td, keys, size, 0, calls, n_steps, batch, stratified, got, tag)
                assert (l.rank_order.cpu().numpy()[size:] == -1).all() and (l.rank_cum.cpu().numpy()[size:] == -1.0).all(), tag
                assert (l.keys.cpu().numpy()[size:] == -1).all(), tag
                assert (_weights(l, td)[slots] > 0).all(), tag
    assert np.array_equal(l.priority.cpu().numpy(), pri) and int(l.seen.item()) == count
    if not td:
        w = l.weight.cpu().numpy()[:size].astype(np.float64)
        assert np.allclose(w, pri[:size].astype(np.float64) ** 0.6, rtol=1e-6, atol=0)
    from reinlife_amd import _lib
    assert l.rank_work.numel() == prc.work_bytes(capacity) == _lib.lib().rl_learn_prio_draw_rank_work_bytes(capacity) and l.rank_work.data_ptr() % 16 == 0
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_the_stamp_is_the_race_draws(worlds, td):
    """A ring of 1001 rows: nothing seen; seen partway; a window that wraps; count - seen >= capacity; nothing new.  Afterwards *seen ==
    *count, and priority and weight are, bit for bit, what the race draw (rl_learn_prioritized_wide_draw / rl_learn_td_draw) leaves on
    a copy of the same memory."""
    import torch
    rows, keys = _rows(1001)
    for count, seen in ((700, 0), (1001, 400), (1100, 990), (1100 + 1001, 1100), (3000, 10), (1500, 1500)):
        out = []
        for rank in (True, False):
            l = _learner(td, _ring(rows, count=count), 64, seen=seen)
            if not td:
                l.prio_max.fill_(2.5)
                l.weight.fill_(-3.0)
            before = l.priority.cpu().numpy().copy()
            if rank:
                _draw(worlds, td, [l], 1, td)
            else:
                (worlds.draw_td if td else worlds.draw_prioritized)([l], 1)
                torch.cuda.synchronize()
            assert int(l.seen.item()) == count, (count, seen)
            out.append({k: getattr(l, k).cpu().numpy().copy() for k in (("priority",) if td else ("priority", "weight"))})
        size = min(count, 1001)
        stamped = out[0]["priority"] != before
        fresh = min(count - seen, 1001)
        print("count %d seen %d: %d rows stamped, %d fresh" % (count, seen, int(stamped.sum()), fresh))
        assert int(stamped[:size].sum()) <= fresh and not stamped[size:].any()
        value = np.float32(l.p_new) if td else np.float32(2.5)
        window = np.zeros(1001, bool) if fresh == 0 else np.ones(1001, bool) if fresh >= 1001 else np.isin(np.arange(1001), np.arange(seen, count) % 1001)
        assert (out[0]["priority"][window] == value).all() and np.array_equal(out[0]["priority"][~window], before[~window])
        for k in out[0]:
            assert out[0][k].tobytes() == out[1][k].tobytes(), (count, seen, k)
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_weight_edges(worlds, td):
    """200 rows.  All weights zero: the uniform rank rule.  One positive weight among zeros at the lowest rank, the highest rank and on
    both sides of a segment boundary: every draw takes it, in both modes (the stratified targets reach total: the clamp).  Priorities 0
    and NaN are never drawn.  Weights over sixty orders of magnitude: no error, and the largest takes all but a negligible share."""
    rows, keys = _rows(200)
    order = rc.host_order(keys)
    x, _ = prc.philox_words(SEED, 0, 0, _site(td), 64)
    uniform = order[((x * np.uint64(200)) >> np.uint64(32)).astype(np.int64)]
    for stratified in (False, True):
        l = _learner(td, _ring(rows), 64, priority=np.zeros(200, np.float32))
        got = _draw(worlds, td, [l], 1, stratified)
        assert np.array_equal(got.reshape(-1), uniform) and not l.rank_cum.cpu().numpy().any()
        for rank in (0, 63, 64, 199):
            for value in (1.0, 1e-30, 3e38):
                pri = np.zeros(200, np.float32)
                pri[order[rank]] = value
                l = _learner(td, _ring(rows), 64, priority=pri)
                got = _draw(worlds, td, [l], 2, stratified)
                assert (got == order[rank]).all(), (stratified, rank, value)
                _check(l, td, keys, 200, 0, 0, 2, 64, stratified, got)
        pri = np.where(np.arange(200) % 3 == 0, 0.0, np.where(np.arange(200) % 3 == 1, np.nan, 1.0)).astype(np.float32)
        l = _learner(td, _ring(rows), 64, priority=pri)
        got = _draw(worlds, td, [l], 4, stratified)
        assert (pri[got.reshape(-1)] == 1.0).all() and len(np.unique(got)) > 30
        _check(l, td, keys, 200, 0, 0, 4, 64, stratified, got)
        pri = (10.0 ** (-30.0 + 10 * (np.arange(200) % 6))).astype(np.float32)    # 1e-30 .. 1e20, and ONE row of 1e30
        pri[order[77]] = 1e30
        l = _learner(td, _ring(rows), 64, priority=pri)
        got = _draw(worlds, td, [l], 4, stratified)
        _check(l, td, keys, 200, 0, 0, 4, 64, stratified, got)
        w = _weights(l, td).astype(np.float64)
        assert np.isfinite(l.rank_cum.cpu().numpy()).all()
        share = w[order[77]] / w.sum()
        print("largest weight's share 1 - %.3g, drawn %d of 256" % (1 - share, int((got == order[77]).sum())))
        assert 1 - share < 1e-4 and (got == order[77]).sum() >= 255               # (256 draws miss it 0.03 times at the most, on average)
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_stratified_draws_stay_inside_their_strata(worlds, td):
    """48 rows, priorities cycling 0, 0.25, 1, 4, batch 64, three steps: for draw j with drawn rank r, cum[r] > j seg and cum[r - 1] <=
    (j + 1) seg; per row, the count in one batch lies in [floor(B w / sum) - 1, ceil(B w / sum) + 1]; zero rows are never drawn."""
    rows, keys = _golden48()
    pri = prc.cycle_priorities(48)
    l = _learner(td, _ring(rows), 64, priority=pri, calls=1)
    got = _draw(worlds, td, [l], 3, True)
    slots, ranks, order, cum = _check(l, td, keys, 48, 0, 1, 3, 64, True, got)
    dev_cum = l.rank_cum.cpu().numpy()
    place = np.empty(48, np.int64)
    place[l.rank_order.cpu().numpy()] = np.arange(48)
    w = _weights(l, td).astype(np.float64)
    share = 64 * w / w.sum()
    seg = dev_cum[47] / np.float64(64)
    for s in range(3):
        r = place[got[0, s]]
        j = np.arange(64, dtype=np.float64)
        before = np.where(r == 0, 0.0, dev_cum[np.maximum(r - 1, 0)])
        assert (dev_cum[r] > j * seg).all() and (before <= (j + 1) * seg).all(), s
        counts = np.bincount(got[0, s], minlength=48)
        assert (counts >= np.floor(share) - 1).all() and (counts <= np.ceil(share) + 1).all() and not counts[pri == 0].any(), s
    assert not np.array_equal(got[0, 0], got[0, 1])
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_6400_independent_draws_follow_the_weights(worlds, td):
    """tests/test_hip_learn_perd3qn.py's design: 48 rows, priorities cycling 0, 0.25, 1, 4, 100 steps of batch 64 in one call; zero rows
    are never drawn, every other count is within 5 binomial standard deviations of 6400 w_i / sum w.  Deterministic: the fixed seed
    passes on the host rule (tests/test_learn_prio_draw_rank_cpu.py)."""
    rows, keys = _golden48()
    pri = prc.cycle_priorities(48)
    l = _learner(td, _ring(rows), 64, priority=pri)
    got = _draw(worlds, td, [l], 100, False)
    _check(l, td, keys, 48, 0, 0, 100, 64, False, got)
    w = _weights(l, td).astype(np.float64)
    p = w / w.sum()
    counts = np.bincount(got.reshape(-1), minlength=48)
    sigma = np.sqrt(6400 * p * (1 - p))
    z = (counts - 6400 * p)[pri > 0] / sigma[pri > 0]
    print("z min %.2f max %.2f" % (z.min(), z.max()))
    assert counts.sum() == 6400 and not counts[pri == 0].any() and (np.abs(z) <= 5).all()
    worlds.check_error_flag()


@pytest.mark.parametrize("stratified", [False, True])
def test_the_rows_drawn_do_not_depend_on_the_order_of_the_ring(worlds, stratified):
    """The same 1025 rows with their priorities in another order: other slots, the same rows, and the same cumulative sum."""
    rows, keys = _rows(1025)
    pri = pc.edge_priorities(1025)
    perm = np.random.RandomState(7).permutation(1025)
    a = _learner(False, _ring(rows), 130, priority=pri, calls=2)
    b = _learner(False, _ring(_take(rows, perm)), 130, priority=pri[perm], calls=2)
    sa, sb = _draw(worlds, False, [a], 3, stratified).reshape(-1), _draw(worlds, False, [b], 3, stratified).reshape(-1)
    assert not np.array_equal(sa, sb) and len(np.unique(sa)) > 100
    assert np.array_equal(perm[sb], sa)                                            # (distinct keys: the very same rows)
    assert a.rank_cum.cpu().numpy().tobytes() == b.rank_cum.cpu().numpy().tobytes()
    worlds.check_error_flag()


def test_a_row_stored_twice_sits_at_adjacent_ranks_and_both_copies_carry_weight(worlds):
    """130 rows: 65 distinct ones, each a second time, shuffled.  In `order` the two slots of a pair are neighbours, the lower slot first;
    cum rises at both; over 50 steps of batch 64 both copies of the heaviest pair are drawn."""
    rows, _ = _rows(130)
    perm = np.random.RandomState(3).permutation(130)
    source = np.concatenate([np.arange(65), np.arange(65)])[perm]
    twice = _take(rows, source)
    keys = pc.content_keys(twice, 130, twice["ring_age"])
    assert len(set(keys.tolist())) == 65
    pri = (1.0 + source % 5).astype(np.float32)
    l = _learner(True, _ring(twice), 64, priority=pri)
    got = _draw(worlds, True, [l], 50, False)
    slots, ranks, order, cum = _check(l, True, keys, 130, 0, 0, 50, 64, False, got)
    place = np.empty(130, np.int64)
    place[order] = np.arange(130)
    for r in range(65):
        lo, hi = np.nonzero(source == r)[0]
        assert lo < hi and place[hi] == place[lo] + 1, r
    assert (np.diff(np.concatenate([[0.0], cum])) > 0).all()
    lo, hi = np.nonzero(source == 4)[0]
    assert (got == lo).any() and (got == hi).any()
    worlds.check_error_flag()


def _raw(worlds, td, learners, n_steps, stratified, slots):
    """The C entry point itself, into the caller's own `slots` tensor -> the status."""
    import torch
    from reinlife_amd import _lib
    n = len(learners)
    side = _lib.TdPrio if td else _lib.Prio
    arr = (_lib.Learner * n)(*[l.struct() for l in learners])
    rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
    sides = (side * n)(*[l.side_struct(side) for l in learners])
    order, cum, work = ((C.c_void_p * n)(*[getattr(l, name).data_ptr() for l in learners]) for name in ("rank_order", "rank_cum", "rank_work"))
    fn = worlds.lib.rl_learn_td_draw_rank if td else worlds.lib.rl_learn_prioritized_draw_rank
    status = fn(worlds.handle, arr, rings, sides, n, n_steps, int(stratified), order, cum, work, C.c_void_p(slots.data_ptr()), worlds._stream())
    torch.cuda.synchronize()
    return status


def test_sixteen_learners_of_different_ring_sizes_and_batches_in_one_call(worlds):
    """RL_MAX_CAPTURE_BRAINS = 16 PERD3QN learners in one call of 2 steps through the C ABI: ring sizes 1 .. 1025, batches 1 .. 2048.  The
    tables lie end to end (64 guard entries behind them keep their -7), each the host rule's at its learner's own index, and the
    sixteenth draws, index apart, from the order and cum it gets alone; a seventeenth is refused."""
    import torch
    sizes = [1, 2, 63, 64, 65, 129, 200, 31, 48, 1025, 7, 300, 64, 128, 500, 1025]
    batches = [1, 64, 65, 2048, 130, 7, 64, 1, 32, 96, 2048, 3, 64, 65, 640, 130]
    ls = []
    for i, (size, batch) in enumerate(zip(sizes, batches)):
        rows, keys = _rows(size + 3, seed=20 + i)
        l = _learner(False, _ring(rows, count=size), batch, calls=i % 3)
        _draw(worlds, False, [l], 1, False)              # (allocates the learner's order, cum and scratch)
        l.rank_order.fill_(-1), l.rank_cum.fill_(-1.0), l.rank_work.fill_(0xA5)
        ls.append((l, keys, size, batch, i % 3))
    total = 2 * sum(batches)
    slots = torch.full((total + 64,), -7, dtype=torch.int32, device=DEV)
    assert _raw(worlds, False, [l for l, *_ in ls], 2, False, slots) == 0
    got = slots.cpu().numpy()
    assert (got[total:] == -7).all()
    off = 0
    for i, (l, keys, size, batch, calls) in enumerate(ls):
        _check(l, False, keys, size, i, calls, 2, batch, False, got[off:off + 2 * batch], i)
        off += 2 * batch
    l, keys, size, batch, calls = ls[15]
    solo = _learner(False, l.ring, batch, calls=calls)
    alone = _draw(worlds, False, [solo], 2, False)
    _check(solo, False, keys, size, 0, calls, 2, batch, False, alone)
    assert solo.rank_order.cpu().numpy()[:size].tobytes() == l.rank_order.cpu().numpy()[:size].tobytes()
    assert solo.rank_cum.cpu().numpy()[:size].tobytes() == l.rank_cum.cpu().numpy()[:size].tobytes()
    with pytest.raises(ValueError, match="1 to 16 learners"):
        worlds.draw_prioritized_rank([l for l, *_ in ls] + [solo], 1)
    with pytest.raises(ValueError, match="share one batch size"):
        worlds.draw_prioritized_rank([ls[0][0], ls[1][0]], 1)
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_a_second_identical_call_gives_identical_order_cum_and_slots(worlds, td):
    """10,000 rows, 3 steps, twice -- with the scratch overwritten in between: the same bits; one call counts eight launches."""
    rows, keys = _rows(10_000)
    l = _learner(td, _ring(rows), 64 if td else 2048)
    a = _draw(worlds, td, [l], 3, td)
    oa, ca = l.rank_order.cpu().numpy().copy(), l.rank_cum.cpu().numpy().copy()
    l.rank_work.fill_(0x3C)
    before = worlds.launches
    b = _draw(worlds, td, [l], 3, td)
    assert worlds.launches - before == prc.PRIO_RANK_LAUNCHES == 8
    assert a.tobytes() == b.tobytes() and oa.tobytes() == l.rank_order.cpu().numpy().tobytes() and ca.tobytes() == l.rank_cum.cpu().numpy().tobytes()
    worlds.check_error_flag()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn-130", "perdqn-64"])
def test_the_learners_train_on_the_table_and_the_next_draw_follows_the_call_counter(worlds, td):
    """rl_learn_prioritized_wide at batch 130 and rl_learn_td at batch 64 fed the rank draw's table train with error flag 0, rewrite
    the priorities at exactly the drawn slots, and advance state[1]: the next draw is the host rule's for calls = 1."""
    import torch
    rows, keys = _rows(1025)
    batch = 64 if td else 130
    l = _learner(td, _ring(rows), batch, wide=None if td else 130)
    params = l.params.cpu().numpy().copy()
    worlds.err.zero_()
    slots = (worlds.draw_td_rank if td else worlds.draw_prioritized_rank)([l], 1)
    torch.cuda.synchronize()
    before = l.priority.cpu().numpy().copy()
    first = slots.cpu().numpy().reshape(-1)
    _check(l, td, keys, 1025, 0, 0, 1, batch, td, first)
    worlds.learn([l], 1, slots=slots)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist()[0] == 0
    worlds.check_error_flag()
    assert l.state.cpu().tolist() == [1, 1] and not np.array_equal(l.params.cpu().numpy(), params) and np.isfinite(l.params.cpu().numpy()).all()
    after = l.priority.cpu().numpy()
    drawn = np.zeros(1025, bool)
    drawn[first] = True
    assert np.array_equal(after[~drawn], before[~drawn]) and (after[drawn] != before[drawn]).all() and (after[drawn] > 0).all()
    second = _draw(worlds, td, [l], 1, td).reshape(-1)
    _check(l, td, keys, 1025, 0, 1, 1, batch, td, second)
    assert not np.array_equal(first, second)


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn", "perdqn"])
def test_bad_arguments_are_refused_and_nothing_is_launched(worlds, td):
    """On real buffers: a wrong kind (RL_E_UNSUPPORTED naming it), a null work entry, a batch out of range, n_steps 0 -- every table,
    order and cum keep their sentinels, and *seen stays."""
    import torch
    rows, _ = _rows(129)
    l = _learner(td, _ring(rows), 64, seen=5)
    other = _learner(not td, _ring(rows), 64)
    _draw(worlds, td, [l], 1, False)
    _draw(worlds, not td, [other], 1, False)
    l.seen.fill_(5)
    l.rank_order.fill_(-1), l.rank_cum.fill_(-1.0)
    slots = torch.full((256,), -7, dtype=torch.int32, device=DEV)
    who = b"rl_learn_td_draw_rank" if td else b"rl_learn_prioritized_draw_rank"

    def refused(status, *words):
        err = worlds.lib.rl_last_error()
        assert worlds.lib.rl_last_error().startswith(who + b":") and all(w in err for w in words), err
        assert (slots.cpu().numpy() == -7).all() and (l.rank_order.cpu().numpy() == -1).all() and (l.rank_cum.cpu().numpy() == -1.0).all()
        assert int(l.seen.item()) == 5
        return status
    kind = l.kind
    l.kind = other.kind
    assert refused(_raw(worlds, td, [l], 1, False, slots), b"learner 0", b"kind %d" % other.kind) == -4
    l.kind = kind
    work, l.rank_work = l.rank_work, torch.zeros(0, dtype=torch.uint8, device=DEV)
    assert l.rank_work.data_ptr() == 0
    assert refused(_raw(worlds, td, [l], 1, False, slots), b"work[0]") == -1
    l.rank_work = work
    for batch in (0, 65 if td else 2049):
        l.batch = batch
        assert refused(_raw(worlds, td, [l], 1, False, slots), b"batch") == -1
    l.batch = 64
    assert refused(_raw(worlds, td, [l], 0, False, slots), b"n_steps") == -1
    assert _raw(worlds, td, [l], 1, False, slots) == 0 and int(l.seen.item()) == 129 and (slots.cpu().numpy()[:64] >= 0).all()
    worlds.check_error_flag()


# ---- the whole path: trainer(learn="device", learn_draw={...}) ----
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
_runs = {}


def _train(td, tmp=None, fresh=False, spy=None, **kw):
    """One short trainer() run on 4 synthetic worlds, 30 episodes, learn_every 10 (three learning calls): a DQN brain and a PERD3QN brain
    (exploration 5: it trains after episodes 10, 20 and 30) under learn_prioritized=True, or (td) a DQN and a PERDQN brain (train_start 100)
    under learn_td_priority=True.  spy: called with the DeviceWorlds class before the run (to wrap a draw)."""
    import torch
    from reinlife_amd import Models, trainer
    key = (td,) + tuple(sorted((k, str(v)) for k, v in kw.items()))
    if tmp is None and not fresh and spy is None and key in _runs:
        return _runs[key]
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=30), Models.PERDQN() if td else Models.PERD3QN(exploration=5, soft_update_freq=20)]
    if td:
        brains[1].train_start = 100
    init = [b.state_dict_flat().copy() for b in brains]
    opt_in = dict(learn_td_priority=True) if td else dict(learn_prioritized=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=30, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      learn_every=10, save=tmp is not None, print_results=False, **opt_in, **kw)
    count, capacity = int(env.worlds.replays[1]["count"].item()), int(env.worlds.replays[1]["state"].shape[0])
    assert 130 <= count < capacity, (count, capacity)        # (no wrap: the rows a draw sees do not depend on append order)
    out = (env, brains, init)
    if tmp is None and not fresh and spy is None:
        _runs[key] = out
    return out


def _bits(env):
    """The learners' buffers as bytes; the priorities sorted (the rows' slots differ from run to run, their priorities do not)."""
    import torch
    torch.cuda.synchronize()
    out = {}
    for k, l in env.learners.items():
        out[k] = {n: getattr(l, n).cpu().numpy().tobytes() for n in BUFFERS}
        if l.priority is not None:
            out[k]["priority"] = np.sort(l.priority.cpu().numpy()).tobytes()
    return out


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn-96", "perdqn"])
def test_trainer_with_the_key_trains_repeats_and_counts_its_launches(td, tmp_path, monkeypatch):
    kind = "PERDQN" if td else "PERD3QN"
    kw = {} if td else dict(learn_batch={"PERD3QN": 96})
    env, brains, init = _train(td, learn_draw={kind: "rank"}, **kw)
    plain, _, _ = _train(td, **kw)
    assert env.learn_draw == {kind: "rank"} and plain.learn_draw is None and env.learn_now_calls == plain.learn_now_calls == 3
    l = env.learners[1]
    assert l.entry == ("rl_learn_td" if td else "rl_learn_prioritized_wide") and l.batch == (64 if td else 96)
    assert l.rank_cum is not None and l.rank_work.numel() == prc.work_bytes(l.ring["state"].shape[0]) and plain.learners[1].rank_cum is None
    assert l.state.cpu().tolist() == [3, 3] and int(l.seen.item()) == int(l.ring["count"].item())
    assert env.learners[0].rank_order is None                                     # the DQN learner's draw is what it was
    for k, b in enumerate(brains):
        now = b.state_dict_flat()
        assert not np.array_equal(now, init[k]) and np.isfinite(now).all()
    env.worlds.check_error_flag()
    assert env.worlds.err.cpu().tolist()[0] == 0
    a, p = _bits(env), _bits(plain)
    assert a[1]["params"] != p[1]["params"]                                       # another sampler: other rows, other parameters
    assert env.worlds.launches - plain.worlds.launches == (prc.PRIO_RANK_LAUNCHES - 2) * 3
    monkeypatch.chdir(tmp_path)
    env2, _, _ = _train(td, tmp=tmp_path, learn_draw={kind: "rank"}, **kw)
    assert a == _bits(env2) and env.tracker.results == env2.tracker.results and env.worlds.launches == env2.worlds.launches
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    entry = "rl_learn_td_draw_rank" if td else "rl_learn_prioritized_draw_rank"
    import json
    assert json.loads(settings)["Learn draw"] == {kind: "rank"} and entry in json.loads(settings)["Weights"]
    assert entry in env._weights_note() and "draw_rank" not in plain._weights_note()


@pytest.mark.parametrize("td", [False, True], ids=["perd3qn-96", "perdqn"])
def test_without_the_key_every_draw_is_the_race_entry_points(td, monkeypatch):
    """The run without the key, watched: every prioritised draw it makes is called again on a copy of the memory as it stood, through
    the race entry point itself (rl_learn_prioritized_wide_draw / rl_learn_td_draw) -- the same table, priorities and seen, bit for bit;
    no rank buffer is ever made; and the run ends on the bits of an unwatched run."""
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds
    name, entry, side = ("draw_td", "rl_learn_td_draw", _lib.TdPrio) if td else ("draw_prioritized", "rl_learn_prioritized_wide_draw", _lib.Prio)
    tensors = ("priority", "keys", "seen") if td else ("priority", "weight", "keys", "seen")
    original, seen_calls = getattr(DeviceWorlds, name), []

    def watched(self, learners, n_steps):
        torch.cuda.synchronize()
        kept = [{t: getattr(l, t).clone() for t in tensors} for l in learners]
        got = original(self, learners, n_steps)
        torch.cuda.synchronize()
        after = [{t: getattr(l, t).clone() for t in tensors} for l in learners]
        for l, k in zip(learners, kept):
            for t in tensors:
                getattr(l, t).copy_(k[t])
        n = len(learners)
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        sides = (side * n)(*[l.side_struct(side) for l in learners])
        again = torch.full_like(got, -1)
        assert getattr(self.lib, entry)(self.handle, arr, rings, sides, n, int(n_steps), C.c_void_p(again.data_ptr()), self._stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(again, got)
        for l, a in zip(learners, after):
            for t in tensors:
                assert getattr(l, t).cpu().numpy().tobytes() == a[t].cpu().numpy().tobytes(), t
        seen_calls.append(n_steps)
        return got
    kw = {} if td else dict(learn_batch={"PERD3QN": 96})
    monkeypatch.setattr(DeviceWorlds, name, watched)
    env, _, _ = _train(td, fresh=True, **kw)
    monkeypatch.undo()
    assert seen_calls == [1, 1, 1] and all(l.rank_cum is None and l.rank_order is None for l in env.learners.values())
    plain, _, _ = _train(td, **kw)
    assert _bits(env) == _bits(plain) and env.worlds.launches == plain.worlds.launches and env.tracker.results == plain.tracker.results
