"""GPU: the world kernels (rl_world.hip, rl_run.hip, rl_world_dev.h) on the narrowest, longest and fullest grids rl_create accepts -- the
table of tests/world_shape_cases.py -- against the CPU oracle, bit for bit: sides of 3 and of 255 (8-bit coordinates packed in one
unsigned short), both sides below the 7-wide window, widths whose padded plane stride equals the width, a shape whose padding is refused,
4,095 and 4,096 cells (cell / W by reciprocal), the fullest LDS.  tests/test_world_shapes_cpu.py shows without a GPU that these inputs
cross both seams, stand on coordinate 254 and see births, vanishes and refills.  There is no tolerance anywhere in this file."""
import numpy as np
import pytest

import world_shape_cases as wc

pytestmark = pytest.mark.gpu

INDEX = {wc.case_id(c): k for k, c in enumerate(wc.CASES)}
BY_ID = {wc.case_id(c): c for c in wc.CASES}
LONG = [c for c in wc.CASES if 255 in (c.width, c.height)]
DUELING = (("PERD3QN", "D3QN"), (0.0, 0.2), (7, 8))
MIXED = (("PPO", "DQN", "PERD3QN"), (0.0, 0.3, 0.05), (21, 22, 23))
# The greedy dueling brains of these weights attack in place (actions 5 and 6 in 85 % of their rows): on the 255-long rows the D3QN brain
# explores in every row instead, so that agents walk through the far seam under the launch's own actions (_launch_against_loop_and_oracle)
LONG_EPS = 1.0


def _weights(kind, seed):
    import bench
    return bench.brain_weights(kind, seed)


_static = wc.is_static      # non-static families on every second row
_seed = wc.world_seed


def _cmp_state(dw, ow, tag):
    n = ow.s["n_agents"]
    for key in dw.s:
        got, want = dw.s[key].cpu().numpy(), ow.s[key]
        if key.startswith("a_"):
            for w in range(ow.R):
                assert np.array_equal(got[w, : n[w]], want[w, : n[w]]), (tag, key, w)
        else:
            assert np.array_equal(got.reshape(want.shape), want), (tag, key)


def _cmp_rows(got, want, n, tag):
    got, want = np.asarray(got), np.asarray(want)
    for w in range(len(n)):
        assert got[w, : n[w]].tobytes() == want[w, : n[w]].tobytes(), (tag, w)


def _same_device_state(a, b, tag):
    n = a.s["n_agents"].cpu().numpy()
    assert np.array_equal(n, b.s["n_agents"].cpu().numpy()), tag
    for key in a.s:
        x, y = a.s[key].cpu().numpy(), b.s[key].cpu().numpy()
        if key.startswith("a_"):
            for w in range(a.R):
                assert np.array_equal(x[w, : n[w]], y[w, : n[w]]), (tag, key, w)
        else:
            assert np.array_equal(x, y), (tag, key)
    _cmp_rows(a.obs_state().cpu().numpy(), b.obs_state().cpu().numpy(), n, tag + " obs2")


# ---------------------------------------------------------------------------------------------------------------------
# a. reset, split step and update
# ---------------------------------------------------------------------------------------------------------------------
SPLIT = [(c, None) for c in wc.CASES] + [(c, 256) for c in wc.CASES if c.slot_cap <= 256]


@pytest.mark.parametrize("case,block", SPLIT, ids=["%s-%s" % (wc.case_id(c), "T%d" % b if b else "default") for c, b in SPLIT])
def test_reset_split_step_and_update_match_the_oracle(case, block, hip_option):
    """reset_synthetic, then 40 ticks of rl_step + rl_update under seeded random actions with a refill every 10 ticks (wc.SETTINGS["split"]):
    world state, every per-agent output of both launches and the Tracker arrays against the oracle, at the default workgroup size and at 256
    threads."""
    from hip_backend import HipBackend
    from oracle import oracle as orc
    if block:
        hip_option("world_block", block)
    R = wc.n_worlds(case)
    setting = wc.SETTINGS["split"]       # (the inputs tests/test_world_shapes_cpu.py asserts its preconditions on)
    cfg = wc.config(case, 3, _static(case), world_base=setting["world_base"])
    hb = HipBackend(R, seed=_seed(case), **cfg)
    ow = orc.OracleWorlds(n_worlds=R, seed=_seed(case), **cfg)
    assert hb.cap == ow.cap == case.slot_cap
    hb.dw.reset_synthetic(case.n_new)
    ow.reset_synthetic(case.n_new)
    hb.dw.check_error_flag()
    _cmp_state(hb.dw, ow, "reset")
    _cmp_rows(hb.obs2, ow.obs2, ow.s["n_agents"], "reset obs2")
    rng = np.random.RandomState(100 * case.width + case.height)
    refills = 0
    for t in range(wc.TICKS):
        acts = rng.randint(0, 8, size=(R, hb.cap)).astype(np.int8)
        n0 = ow.s["n_agents"].copy()
        ow.step(acts)
        hb.step(acts)
        _cmp_state(hb.dw, ow, "tick %d step" % t)
        n1 = ow.s["n_agents"].copy()
        assert np.array_equal(hb.n_acted, n0), "tick %d n_acted" % t
        _cmp_rows(hb.reward, ow.reward, n1, "tick %d reward" % t)
        _cmp_rows(hb.done, ow.done, n1, "tick %d done" % t)
        _cmp_rows(hb.src1, ow.src1, n1, "tick %d src1" % t)
        _cmp_rows(hb.obs1, ow.obs1, n1, "tick %d obs1" % t)
        assert np.array_equal(hb.trk_tick, ow.trk_tick) and np.array_equal(hb.trk_pop, ow.trk_pop), "tick %d tracker" % t
        assert np.array_equal(hb.trk_sum, ow.trk_sum) and np.array_equal(hb.trk_cnt, ow.trk_cnt), "tick %d tracker sums" % t
        ow.update()
        hb.update()
        _cmp_state(hb.dw, ow, "tick %d update" % t)
        _cmp_rows(hb.src2, ow.src2, ow.s["n_agents"], "tick %d src2" % t)
        _cmp_rows(hb.obs2, ow.obs2, ow.s["n_agents"], "tick %d obs2" % t)
        if t % setting["refill_every"] == setting["refill_every"] - 1:
            refills += ow.refill(case.thr, case.n_new)
            hb.dw.refill(case.thr, case.n_new)
            hb.dw.check_error_flag()
            _cmp_state(hb.dw, ow, "tick %d refill" % t)
            _cmp_rows(hb.obs2, ow.obs2, ow.s["n_agents"], "tick %d refill obs2" % t)
    assert refills > 0 and int(hb.dw.refill_count.item()) == refills


# ---------------------------------------------------------------------------------------------------------------------
# b. fused tick with refill
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_fused_tick_with_refill_matches_the_oracle(case):
    """rl_tick_refill == step + update_env + refill(thr, n_new) in one launch, 40 ticks of seeded random actions (wc.SETTINGS["fused"])."""
    from oracle import oracle as orc
    from reinlife_amd.worlds import DeviceWorlds
    R = wc.n_worlds(case)
    setting = wc.SETTINGS["fused"]       # (the inputs tests/test_world_shapes_cpu.py asserts its preconditions on)
    assert setting["refill_every"] == 1
    cfg = wc.config(case, 3, _static(case), world_base=setting["world_base"])
    dw = DeviceWorlds(n_worlds=R, seed=_seed(case), **cfg)
    ow = orc.OracleWorlds(n_worlds=R, seed=_seed(case), **cfg)
    dw.reset_synthetic(case.n_new); ow.reset_synthetic(case.n_new)
    rng = np.random.RandomState(100 * case.width + case.height)
    refills = 0
    for t in range(wc.TICKS):
        acts = rng.randint(0, 8, size=(R, dw.cap)).astype(np.int8)
        ow.step(acts); ow.update()
        refills += ow.refill(case.thr, case.n_new)
        dw.set_actions(acts)
        dw.tick_refill(case.thr, case.n_new)
        dw.check_error_flag()
        _cmp_state(dw, ow, "tick %d" % t)
        _cmp_rows(dw.obs_state().cpu().numpy(), ow.obs2, ow.s["n_agents"], "tick %d obs2" % t)
    assert refills > 0 and int(dw.refill_count.item()) == refills


# ---------------------------------------------------------------------------------------------------------------------
# c. Environment.reset on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["3x3", "255x3", "65x63"])
@pytest.mark.parametrize("n_brains", [2, 5])
def test_reset_families_matches_the_oracle(shape, n_brains):
    from oracle import oracle as orc
    from reinlife_amd.worlds import DeviceWorlds
    case = BY_ID[shape]
    R = 16
    cfg = wc.config(case, n_brains, True)
    dw = DeviceWorlds(n_worlds=R, seed=12, world_base=9, **cfg)
    ow = orc.OracleWorlds(n_worlds=R, seed=12, world_base=9, **cfg)
    dw.reset_families(); ow.reset_families()
    dw.check_error_flag()
    _cmp_state(dw, ow, "reset_families")
    _cmp_rows(dw.obs_state().cpu().numpy(), ow.obs2, ow.s["n_agents"], "obs")
    genes = dw.s["a_gene"].cpu().numpy()[:, :n_brains]
    assert (dw.s["n_agents"].cpu().numpy() == n_brains).all() and (np.sort(genes, axis=1) == np.arange(n_brains)).all()
    assert len({tuple(g) for g in genes}) > 1          # which brain lands where differs from world to world


# ---------------------------------------------------------------------------------------------------------------------
# d, e, g. the multi-tick launch
# ---------------------------------------------------------------------------------------------------------------------
def _handles(case, brains, n, static, **over):
    """-> n DeviceWorlds of the case with these brains (names, epsilons, weight seeds) from reset_synthetic, the oracle beside them, the weights."""
    from oracle import oracle as orc
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    names, eps, seeds = brains
    R = wc.n_worlds(case)
    cfg = wc.config(case, len(names), static, **over)
    wts = [_weights(k, s) for k, s in zip(names, seeds)]
    out = []
    for _ in range(n):
        dw = DeviceWorlds(n_worlds=R, seed=1299, world_base=3, **cfg)
        dw.set_brains([(_lib.KIND_BY_METHOD[k], e, pack_brain_weights(_lib.KIND_BY_METHOD[k], w)) for k, e, w in zip(names, eps, wts)])
        dw.reset_synthetic(case.n_new)
        out.append(dw)
    ow = orc.OracleWorlds(n_worlds=R, seed=1299, world_base=3, **cfg)
    ow.reset_synthetic(case.n_new)
    return out, ow


def _launch_against_loop_and_oracle(case, brains, expect_run):
    """One handle runs the multi-tick launch, the other rl_policy_act + rl_tick_refill tick by tick, the oracle is fed the actions: 40
    launches of one tick with state and Agent.state compared three ways every tick, then launches of 2, 7 and 20 ticks with every output of
    the last tick compared as well.  -> seam crossings (rows, columns) of the oracle's trajectory under these actions."""
    (fused, loop), ow = _handles(case, brains, 2, _static(case))
    assert fused.run_supported() == bool(expect_run), "rl_run_supported: the table says %d" % expect_run
    thr, n_new = case.thr, case.n_new
    crossings = np.zeros(2, np.int64)

    def oracle_tick(acts):
        before = wc.positions(ow)
        prev = ow.obs2.copy()
        n0 = ow.s["n_agents"].copy()
        ow.step(acts)
        n1 = ow.s["n_agents"].copy()
        post = {k: getattr(ow, k).copy() for k in ("reward", "done", "src1", "obs1")}
        ow.update()
        crossings[:] += wc.seam_crossings(before, wc.positions(ow), case.height, case.width)
        src2, n2, epoch = ow.src2.copy(), ow.s["n_agents"].copy(), ow.s["epoch"].copy()
        refills = ow.refill(thr, n_new)
        return dict(prev=prev, n0=n0, n1=n1, post=post, src2=src2, n2=n2, kept=ow.s["epoch"] == epoch, refills=refills)

    refills = acted = 0
    for t in range(wc.TICKS):
        fused.run(1, thr, n_new)
        loop.act(); loop.tick_refill(thr, n_new)
        acts = fused.actions.cpu().numpy().copy()
        o = oracle_tick(acts)
        refills += o["refills"]; acted += int(o["n0"].sum())
        fused.check_error_flag(); loop.check_error_flag()
        _same_device_state(fused, loop, "tick %d" % t)
        _cmp_state(fused, ow, "tick %d vs oracle" % t)
        _cmp_rows(fused.obs_state().cpu().numpy(), ow.obs2, ow.s["n_agents"], "tick %d obs2 vs oracle" % t)
    done = wc.TICKS
    for chunk in (2, 7, 20):
        fused.run(chunk, thr, n_new)
        for _ in range(chunk):
            loop.act(); loop.tick_refill(thr, n_new)
            o = oracle_tick(loop.actions.cpu().numpy().copy())
            refills += o["refills"]; acted += int(o["n0"].sum())
        done += chunk
        fused.check_error_flag(); loop.check_error_flag()
        tag = "after %d ticks" % done
        _same_device_state(fused, loop, tag)
        _cmp_state(fused, ow, tag + " vs oracle")
        _cmp_rows(fused.obs_state().cpu().numpy(), ow.obs2, ow.s["n_agents"], tag + " obs2 vs oracle")
        # the last tick's outputs: the policy's input and actions over the agents that acted, the post-step outputs over the post-step
        # list, the update's permutation over the post-update list of the worlds that were not refilled behind it
        assert np.array_equal(fused.n_acted.cpu().numpy(), o["n0"]) and np.array_equal(loop.n_acted.cpu().numpy(), o["n0"]), tag
        _cmp_rows(fused.actions.cpu().numpy(), loop.actions.cpu().numpy(), o["n0"], tag + " actions")
        _cmp_rows(fused.prev_state().cpu().numpy(), o["prev"], o["n0"], tag + " policy input of the last tick vs oracle")
        _cmp_rows(loop.prev_state().cpu().numpy(), o["prev"], o["n0"], tag + " policy input of the last tick, loop vs oracle")
        for name in ("reward", "done", "src1"):
            _cmp_rows(getattr(fused, name).cpu().numpy(), o["post"][name], o["n1"], tag + " " + name + " vs oracle")
            _cmp_rows(getattr(loop, name).cpu().numpy(), o["post"][name], o["n1"], tag + " " + name + ", loop vs oracle")
        _cmp_rows(fused.obs_state_prime().cpu().numpy(), o["post"]["obs1"], o["n1"], tag + " obs1 vs oracle")
        _cmp_rows(loop.obs_state_prime().cpu().numpy(), o["post"]["obs1"], o["n1"], tag + " obs1, loop vs oracle")
        n2 = np.where(o["kept"], o["n2"], 0)
        _cmp_rows(fused.src2.cpu().numpy(), o["src2"], n2, tag + " src2 vs oracle")
        _cmp_rows(loop.src2.cpu().numpy(), o["src2"], n2, tag + " src2, loop vs oracle")
        assert int(fused.acted_total.item()) == int(loop.acted_total.item()) == acted, tag
        assert int(fused.refill_count.item()) == int(loop.refill_count.item()) == refills, tag
    assert refills > 0
    return int(crossings[0]), int(crossings[1])


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_multi_tick_launch_dueling_pair(case):
    """k_run's dueling instantiation (PERD3QN at eps 0, D3QN at eps 0.2) at every shape of the table -- each of them claimed by
    rl_run_supported -- against the two-launch loop and the oracle; on the 255-long rows agents must have walked through both seams under the
    launch's own actions (the D3QN brain explores in every row there: LONG_EPS)."""
    names, eps, seeds = DUELING
    if case in LONG:
        eps = (eps[0], LONG_EPS)
    assert case.run_dueling == 1
    rows, cols = _launch_against_loop_and_oracle(case, (names, eps, seeds), case.run_dueling)
    if case in LONG:
        assert rows >= 1 and cols >= 1, "seam crossings under the launch's actions: %d over rows, %d over columns" % (rows, cols)


@pytest.mark.parametrize("case", [c for c in wc.CASES if c.run_mixed], ids=wc.case_id)
def test_multi_tick_launch_mixed_kinds(case):
    """The mixed-kind kernel (PPO, DQN, PERD3QN with eps 0, 0.3, 0.05) on the rows the table marks supported."""
    _launch_against_loop_and_oracle(case, MIXED, 1)


@pytest.mark.parametrize("case", [c for c in wc.CASES if not c.run_mixed], ids=wc.case_id)
def test_multi_tick_launch_mixed_kinds_fall_back_at_slot_cap_512(case):
    """Mixed kinds at slot_cap 512 are outside rl_run's scope (the tiles' exchange buffers do not fit beside the world): run(9) is nine
    rounds of the two launches."""
    assert case.slot_cap == 512
    (a, b), _ = _handles(case, MIXED, 2, _static(case))
    assert not a.run_supported()
    a.run(9, case.thr, case.n_new)
    for _ in range(9):
        b.act(); b.tick_refill(case.thr, case.n_new)
    a.check_error_flag(); b.check_error_flag()
    _same_device_state(a, b, "fallback")
    _cmp_rows(a.actions.cpu().numpy(), b.actions.cpu().numpy(), a.n_acted.cpu().numpy(), "fallback actions")
    assert int(a.refill_count.item()) == int(b.refill_count.item()) and int(a.acted_total.item()) == int(b.acted_total.item())


# ---------------------------------------------------------------------------------------------------------------------
# f. Tracker and transition capture inside the launch
# ---------------------------------------------------------------------------------------------------------------------
def _ring_rows(dw, b, lo, hi):
    """Transitions lo..hi-1 of brain b's ring as comparable rows (state | state_prime | reward | prob | action | done | age), sorted."""
    r = dw.replays[b]
    idx = np.arange(lo, hi) % r["state"].shape[0]
    cols = [r["state"][idx].cpu().numpy(), r["state_prime"][idx].cpu().numpy(), r["reward"][idx].cpu().numpy()[:, None], r["prob"][idx].cpu().numpy()[:, None]]
    cols += [r[k][idx].cpu().numpy()[:, None].astype(np.float32) for k in ("action", "done", "age")]
    rows = np.ascontiguousarray(np.concatenate(cols, axis=1))
    return rows[np.lexsort(rows.T[::-1])]


@pytest.mark.parametrize("shape", ["255x16", "16x255", "4x6"])
@pytest.mark.parametrize("brains", [DUELING, MIXED], ids=["dueling", "mixed"])
def test_tracker_and_capture_inside_the_launch(shape, brains):
    """Training launches (Tracker on, transition capture with the acting probability, a per-tick epsilon schedule) of 1, 3, 7 and 20 ticks
    against launches of one tick: state, rows, Tracker sums and the brains' replay rings (a launch's transitions as a sorted set: worlds
    interleave by atomics within a tick); the tick-by-tick handle's state and Tracker sums against the oracle fed its actions."""
    import torch
    case = BY_ID[shape]
    nb = len(brains[0])
    ticks = 1 + 3 + 7 + 20
    (A, B), ow = _handles(case, brains, 2, _static(case))
    for dw in (A, B):
        dw.enable_tracking(True)
        dw.enable_capture(capacity=A.R * A.cap * ticks + 1024, with_prob=True)
    assert A.run_supported()
    sched = np.random.RandomState(INDEX[shape]).uniform(0, 0.4, size=(ticks, nb)).astype(np.float32)
    t, seen = 0, [0] * nb
    for chunk in (1, 3, 7, 20):
        A.run(chunk, case.thr, case.n_new, eps_schedule=sched[t:t + chunk])
        for k in range(chunk):
            B.run(1, case.thr, case.n_new, eps_schedule=sched[t + k:t + k + 1])
            ow.step(B.actions.cpu().numpy().copy()); ow.update(); ow.refill(case.thr, case.n_new)
        t += chunk
        torch.cuda.synchronize()
        A.check_error_flag(); B.check_error_flag()
        tag = "after %d ticks" % t
        _cmp_state(B, ow, tag + " vs oracle")
        _cmp_rows(B.obs_state().cpu().numpy(), ow.obs2, ow.s["n_agents"], tag + " obs2 vs oracle")
        assert np.array_equal(B.trk_sum.cpu().numpy(), ow.trk_sum) and np.array_equal(B.trk_cnt.cpu().numpy(), ow.trk_cnt), tag + " tracker vs oracle"
        _same_device_state(A, B, tag)
        assert torch.equal(A.trk_sum, B.trk_sum) and torch.equal(A.trk_cnt, B.trk_cnt), tag + " tracker"
        for b in range(nb):
            ta, tb = int(A.replays[b]["count"].item()), int(B.replays[b]["count"].item())
            assert ta == tb >= seen[b], (tag, "ring count", b, ta, tb)
            assert _ring_rows(A, b, seen[b], ta).tobytes() == _ring_rows(B, b, seen[b], tb).tobytes(), (tag, "ring rows", b)
            seen[b] = ta
    assert min(seen) > 0, seen
