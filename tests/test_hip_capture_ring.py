"""GPU: transition capture where the replay rings wrap, lap and overfill -- capture_reserve / capture_rows inside k_run (rl_run.hip, what
trainer(learn="device") runs) and k_capture (rl_world.hip, behind rl_capture_transitions and the two-launch loop) against the host model of
tests/capture_ring_cases.py, on the rows of its table, with the two brain sets of tests/test_hip_world_shapes.py.  One handle runs run(k)
in chunks, the other act / tick_refill / capture_transitions tick by tick; the oracle is fed the device's actions tick by tick, state is
compared first, then both handles' rings against the model: exact slots for one world, the block rule for several (a snapshot of the ring
before every launch for the untouched slots), `prob` from the tick-by-tick handle's policy outputs.  Rows are compared byte for byte: there
is no tolerance in this file.  The lap, straddle and capacity floors are asserted at run time from the oracle's counts, and every figure is
printed before it is asserted.  The last tests hold the floor of a ring (n_worlds * slot_cap rows) at the boundary."""
import time

import numpy as np
import pytest

import capture_ring_cases as cr

pytestmark = pytest.mark.gpu

DUELING = (("PERD3QN", "D3QN"), (0.0, 0.2), (7, 8))
MIXED = (("PPO", "DQN", "PERD3QN"), (0.0, 0.3, 0.05), (21, 22, 23))
KEYS = ("state", "state_prime", "action", "reward", "done", "age")


def _handles(row, brains, n):
    import bench
    from oracle import oracle as orc
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    names, eps, seeds = brains
    cfg = cr.config(row, len(names))
    wts = [bench.brain_weights(k, s) for k, s in zip(names, seeds)]
    out = []
    for _ in range(n):
        dw = DeviceWorlds(n_worlds=row.worlds, seed=cr.SEED, world_base=cr.WORLD_BASE, **cfg)
        dw.set_brains([(_lib.KIND_BY_METHOD[k], e, pack_brain_weights(_lib.KIND_BY_METHOD[k], w)) for k, e, w in zip(names, eps, wts)])
        dw.reset_synthetic(row.n_new)
        out.append(dw)
    ow = orc.OracleWorlds(n_worlds=row.worlds, seed=cr.SEED, world_base=cr.WORLD_BASE, **cfg)
    ow.reset_synthetic(row.n_new)
    return out, ow


def _ring(dw, b, with_prob):
    """-> (the ring's bytes [capacity, row], its count)"""
    r = dw.replays[b]
    host = {k: r[k].cpu().numpy() for k in KEYS + (("prob",) if with_prob else ())}
    return cr.ring_bytes(host, with_prob), int(r["count"].item())


def _cmp_state(dw, ow, tag):
    n = ow.s["n_agents"]
    for key in dw.s:
        got, want = dw.s[key].cpu().numpy(), ow.s[key]
        if key.startswith("a_"):
            for w in range(ow.R):
                assert np.array_equal(got[w, : n[w]], want[w, : n[w]]), (tag, key, w)
        else:
            assert np.array_equal(got.reshape(want.shape), want), (tag, key)
    obs = dw.obs_state().cpu().numpy()
    for w in range(ow.R):
        assert obs[w, : n[w]].tobytes() == ow.obs2[w, : n[w]].tobytes(), (tag, "obs2", w)


class _Follower:
    """One handle's rings followed launch by launch: the bytes and the count before the launch, the rule behind it."""

    def __init__(self, dw, nb, with_prob, one_world, name):
        self.dw, self.nb, self.with_prob, self.one, self.name = dw, nb, with_prob, one_world, name
        self.before = [_ring(dw, b, with_prob) for b in range(nb)]
        self.placed = self.runs = self.rows = 0

    def launch_done(self, ticks, probs, tag):
        """ticks: the launch's per-tick oracle transitions; probs: per tick per world the tick-by-tick handle's policy outputs (or None)."""
        for b in range(self.nb):
            runs = cr.brain_runs(ticks, b, probs if self.with_prob else None)
            after, count1 = _ring(self.dw, b, self.with_prob)
            before, count0 = self.before[b]
            where = "%s %s brain %d" % (self.name, tag, b)
            if self.one:
                width = before.shape[1]
                rows = np.concatenate(runs) if runs else np.zeros((0, width), np.uint8)
                got = cr.check_one_world(before, after, count0, count1, rows.reshape(-1, width), where)
            else:
                got = cr.check_block(before, after, count0, count1, runs, where)
                self.placed += got["placed"]; self.runs += got["runs"]
            self.rows += got["rows"]
            self.before[b] = (after, count1)


CASES = [(row, brains) for row in cr.TABLE for brains in (DUELING, MIXED)]


@pytest.mark.parametrize("row,brains", CASES, ids=["%s-%s" % (r.name, "dueling" if b is DUELING else "mixed") for r, b in CASES])
def test_rings_against_the_host_model_on_both_capture_paths(row, brains):
    import torch
    t_start = time.perf_counter()
    names = brains[0]
    nb, with_prob = len(names), brains is MIXED
    caps = cr.capacities(row, nb)
    (A, B), ow = _handles(row, brains, 2)
    assert A.cap == ow.cap == row.slot_cap
    for dw in (A, B):
        dw.enable_capture(list(caps), with_prob=with_prob)
        for r in dw.replays:
            r["count"].fill_(row.count0)
    # a slot capacity of 512 is outside what the mixed-kind launch supports: there run(k) is the loop (k_capture on both handles)
    assert A.run_supported() == (not (brains is MIXED and row.slot_cap == 512))
    fa = _Follower(A, nb, with_prob, row.worlds == 1, "run(k)")
    fb = _Follower(B, nb, with_prob, row.worlds == 1, "loop")
    thr, n_new, R = row.thr, row.n_new, row.worlds
    every, done = [], 0
    for chunk in row.chunks:
        A.run(chunk, thr, n_new)
        ticks, probs = [], []
        for _ in range(chunk):
            B.act(want_q=with_prob)
            torch.cuda.synchronize()
            acts = B.actions.cpu().numpy()
            q = B.out_q.cpu().numpy().copy() if with_prob else None
            n0 = ow.s["n_agents"].copy()
            full = np.zeros((R, B.cap), np.int8)
            for w in range(R):
                full[w, : n0[w]] = acts[w, : n0[w]]
            tx = cr.tick_transitions(ow, full, thr, n_new)
            B.tick_refill(thr, n_new)
            B.capture_transitions(with_policy_out=with_prob)
            B.check_error_flag()
            done += 1
            _cmp_state(B, ow, "loop, tick %d" % done)
            ticks.append(tx); probs.append(q)
            if R > 1:           # (several worlds: every tick of the loop is a launch of its own; one world: the rule composes over ticks)
                fb.launch_done([tx], [q], "tick %d" % done)
        A.check_error_flag()
        tag = "after %d ticks" % done
        _cmp_state(A, ow, "run(k), " + tag)
        if R == 1:
            fb.launch_done(ticks, probs, tag)
        fa.launch_done(ticks, probs, tag)
        every += ticks
    counts = cr.count_rows(every, nb)
    figures = cr.reach(counts, caps, row.count0, row.chunks)
    print("\n%s, %s: %d ticks in %d launches; rows per tick and brain %s .. %s" % (row.name, "+".join(names), done, len(row.chunks),
                                                                                 counts.sum(1).min(0).tolist(), counts.sum(1).max(0).tolist()))
    for b, (cap, f) in enumerate(zip(caps, figures)):
        print("  brain %d capacity %d count0 %d: %r" % (b, cap, row.count0, f))
    print("  run(k): %d rows checked, %d of %d runs placed; loop: %d rows checked, %d of %d runs placed; %.2f s"
          % (fa.rows, fa.placed, fa.runs, fb.rows, fb.placed, fb.runs, time.perf_counter() - t_start))
    cr.assert_reach(row, caps, figures, row.name)
    for b in range(nb):
        assert fa.rows == fb.rows == int(counts.sum()) and int(A.replays[b]["count"].item()) == row.count0 + figures[b]["total"]
    if R > 1:   # the run-by-run check is not vacuous: most runs begin with a row that occurs once in their block
        assert fa.placed >= 0.9 * fa.runs and fb.placed >= 0.9 * fb.runs, (fa.placed, fa.runs, fb.placed, fb.runs)


# ---------------------------------------------------------------------------------------------------------------------
# the floor: a ring holds at least what one tick of all worlds can append to it
# ---------------------------------------------------------------------------------------------------------------------
def _small(n_worlds=3):
    row = cr.Row("floor", n_worlds, 12, 9, 40, 128, 30, 20, True, None, 0, (), "")
    (dw,), ow = _handles(row, DUELING, 1)
    return row, dw, ow


def test_enable_capture_refuses_a_ring_below_the_floor_and_takes_one_at_it():
    row, dw, _ = _small()
    floor = dw.capture_floor()
    assert floor == cr.floor_rows(3, 128) == 384
    with pytest.raises(ValueError, match=r"ring 1: capacity 383 is below the floor of 384 rows \(n_worlds 3 x slot_cap 128"):
        dw.enable_capture([floor, floor - 1])
    with pytest.raises(ValueError, match=r"ring 0: capacity 383 is below the floor of 384"):
        dw.enable_capture(floor - 1)
    assert dw.replays is None
    dw.enable_capture(floor)
    assert [r["state"].shape[0] for r in dw.replays] == [floor, floor]


@pytest.mark.parametrize("path", ["run", "capture_transitions"])
def test_the_entry_points_refuse_a_ring_below_the_floor_before_anything_is_launched(path):
    """rl_run_ex (given replays) and rl_capture_transitions: RL_E_INVALID naming the ring, its capacity and the floor at floor - 1 -- the
    world has not moved and no count has changed -- and the same call runs at the floor."""
    import torch
    from reinlife_amd import _lib
    row, dw, _ = _small()
    floor = dw.capture_floor()
    dw.enable_capture(floor)
    assert dw.run_supported()
    if path == "capture_transitions":
        dw.act(); dw.tick_refill(row.thr, row.n_new)
    call = (lambda: dw.run(4, row.thr, row.n_new)) if path == "run" else dw.capture_transitions
    tick0 = dw.s["tick"].cpu().numpy().copy()
    dw._replay_arr[1].capacity = floor - 1           # (the library's own check: enable_capture would not have made this ring)
    with pytest.raises(_lib.ReinLifeHipError) as e:
        call()
    msg = str(e.value)
    print(msg)
    assert "(-1)" in msg and ("rl_run" if path == "run" else "rl_capture_transitions") in msg
    assert "replay 1: capacity 383 is below the floor of 384 rows (n_worlds 3 x slot_cap 128" in msg
    torch.cuda.synchronize()
    assert np.array_equal(dw.s["tick"].cpu().numpy(), tick0) and [int(r["count"].item()) for r in dw.replays] == [0, 0]
    dw._replay_arr[1].capacity = floor
    call()
    dw.check_error_flag()
    appended = [int(r["count"].item()) for r in dw.replays]
    print("appended at the floor:", appended)
    assert np.array_equal(dw.s["tick"].cpu().numpy(), tick0 + (4 if path == "run" else 0))
    if path == "run":
        assert min(appended) > 0


def test_a_ring_at_the_floor_holds_every_tick_whole():
    """3 worlds at capacity == floor: every tick's rows of all worlds are one block of whole transitions, on both paths."""
    import torch
    row, A, ow = _small()
    (B,), _ = _handles(row, DUELING, 1)
    floor = A.capture_floor()
    for dw in (A, B):
        dw.enable_capture(floor)
    fa, fb = _Follower(A, 2, False, False, "run(1)"), _Follower(B, 2, False, False, "loop")
    for t in range(30):
        A.run(1, row.thr, row.n_new)
        B.act()
        torch.cuda.synchronize()
        tx = cr.tick_transitions(ow, B.actions.cpu().numpy().copy(), row.thr, row.n_new)
        B.tick_refill(row.thr, row.n_new); B.capture_transitions()
        A.check_error_flag(); B.check_error_flag()
        _cmp_state(A, ow, "tick %d" % t)
        fa.launch_done([tx], None, "tick %d" % t); fb.launch_done([tx], None, "tick %d" % t)
    counts = [int(r["count"].item()) for r in A.replays]
    print("rows", fa.rows, "counts", counts, "floor", floor, "runs placed", fa.placed, "of", fa.runs)
    assert fa.rows == fb.rows == sum(counts) and min(counts) > floor           # both rings have wrapped


def test_environment_raises_a_small_ring_to_the_floor_and_says_so():
    """Models.D3QN(capacity=300) at 4 worlds: rings of 4 * slot_cap rows, exposed as ring_rows; at the reference's 10,000 nothing changes."""
    import warnings
    from reinlife_amd import Environment, Models, _lib
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw = dict(width=30, height=30, max_agents=100, n_worlds=4, static_families=True, training=True, seed=3, rng="philox", print_results=False,
                  synthetic_agents=100, refill_below=70, learn="device", learn_kinds=("D3QN",))
        env = Environment(brains=[Models.D3QN(capacity=300), Models.D3QN(capacity=300)], **kw)
        big = Environment(brains=[Models.D3QN(), Models.D3QN(capacity=1024)], **kw)
    floor = 4 * _lib.slot_cap_for(100)
    assert floor == 1024 == env.worlds.capture_floor() == env.ring_floor
    assert env.ring_rows == [floor, floor] and [r["state"].shape[0] for r in env.worlds.replays] == [floor, floor]
    assert [l.ring["state"].shape[0] for l in env.learners.values()] == [floor, floor]
    assert big.ring_rows == [10_000, 1024] and [r["state"].shape[0] for r in big.worlds.replays] == [10_000, 1024]
