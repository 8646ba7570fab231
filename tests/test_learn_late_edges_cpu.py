"""CPU: the inputs of tests/test_hip_learn_ppo_edges.py, tests/test_hip_learn_perdqn_edges.py and tests/test_hip_learn_wide_edges.py satisfy
what their comparisons rest on -- the float64 race of rl_learn_td_draw has a gap of at least 1e-4 between first and second on every draw
of every size and call number (so a few float32 ulp of -logf(U) / p on the device cannot flip one); the rollout draws of the larger
rings reach rows that only a second pass of k_rollout_pick's loop sees; on the reference's trained weights the PPO rollouts take every
branch of min(), clamp() and smooth-L1, stay 1e-4 away from every kink, and torch's own float32 autograd sits inside every 1e-5 bar the
kernels are held to (PPO, PERDQN and the wide DQN update at 1000 .. 2048 rows); and the host models themselves disagree with a
deliberately wrong variant of each family the GPU tests are meant to catch.  Every figure a bar is held against is printed first."""
import numpy as np
import pytest
import torch

from reinlife_amd import _lib

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc
import learn_ppo_cases as oc
import learn_wide_cases as wc

SEED = 11
SIZES = (1, 3, 255, 256, 257, 701, 1025)
_cache = {}


def _edge(n, seed=11):
    if seed not in _cache:
        rows = lc.edge_ring_rows(1027, seed)
        _cache[seed] = (rows, pc.content_keys(rows, 1027, rows["ring_age"]))
    rows, keys = _cache[seed]
    return {k: v[:n] for k, v in rows.items()}, keys[:n]


# ---- 1. the draws ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("calls", [0, 3])
@pytest.mark.parametrize("n", SIZES)
def test_the_td_race_has_a_gap_and_float32_agrees_with_float64(n, calls):
    """128 draws per size and call number on learn_perd3qn_cases.edge_priorities (the priority itself is the race weight): the smallest
    relative gap between the first and second t is at least 1e-4 in float64; numpy's float32 race (learn_perdqn_cases.host_draw) names
    the float64 winner in every draw; no row of priority 0 is drawn; the keys are distinct."""
    _, keys = _edge(n)
    assert len(set(keys.tolist())) == n
    pri = pc.edge_priorities(n)
    assert (pri[::7] == 0).all() if n > 3 else (pri > 0).all()
    rows, gaps = pc.host_draw64(keys, pri, SEED, 0, calls, 128, site=_lib.SITE_LEARN_TD)
    rows32 = tc.host_draw(keys, pri, SEED, 0, calls, 128)
    print("n %d calls %d: smallest gap %.3g; float32 race differs in %d of 128 draws; %d distinct rows, %d beyond row 255, %d beyond row 511"
          % (n, calls, gaps.min(), int((rows32 != rows).sum()), len(np.unique(rows)), int((rows >= 256).sum()), int((rows >= 512).sum())))
    assert gaps.min() >= 1e-4
    assert np.array_equal(rows32, rows)
    assert (pri[rows] > 0).all()
    if n >= 701:
        assert (rows >= 256).sum() >= 10 and (rows >= 512).sum() >= 5
    if n == 1:
        assert np.isinf(gaps).all() and not rows.any()
    # the site salts the draw: the PERD3QN race on the same weights is another table
    assert n <= 3 or not np.array_equal(rows, pc.host_draw64(keys, pri, SEED, 0, calls, 128)[0])


@pytest.mark.parametrize("brain", [0, 1])
def test_the_mixed_td_learner_cases_have_the_gap_at_either_position(brain):
    """(batch 64, 257 rows, calls 3) and (batch 7, 96 rows of another ring, calls 1), each at brain index 0 and 1."""
    for batch, (_, keys), calls, pseed in ((64, _edge(257), 3, 5), (7, _edge(96, 12), 1, 6)):
        pri = pc.edge_priorities(len(keys), pseed)
        rows, gaps = pc.host_draw64(keys, pri, SEED, brain, calls, 2 * batch, site=_lib.SITE_LEARN_TD)
        print("brain %d batch %d: smallest gap %.3g" % (brain, batch, gaps.min()))
        assert gaps.min() >= 1e-4
        assert np.array_equal(tc.host_draw(keys, pri, SEED, brain, calls, 2 * batch), rows)


def test_a_td_race_bounded_at_256_rows_disagrees_on_the_larger_rings():
    """What the GPU comparison can catch: a host race that sees the first 256 rows only (a pick loop without its second pass) names
    other rows at 701 and 1025 rows, and one that runs to the capacity draws the 1e6 rows beyond the size."""
    for n in (701, 1025):
        _, keys = _edge(n)
        pri = pc.edge_priorities(n)
        rows = pc.host_draw64(keys, pri, SEED, 0, 3, 128, site=_lib.SITE_LEARN_TD)[0]
        short = pc.host_draw64(keys[:256], pri[:256], SEED, 0, 3, 128, site=_lib.SITE_LEARN_TD)[0]
        beyond = np.concatenate([pri, np.full(2, 1e6, np.float32)])
        long_ = pc.host_draw64(_edge(n + 2)[1], beyond, SEED, 0, 3, 128, site=_lib.SITE_LEARN_TD)[0]
        print("n %d: a 256-row race differs in %d of 128 draws, a race over the capacity in %d" % (n, int((short != rows).sum()), int((long_ != rows).sum())))
        assert (short != rows).sum() >= 64 and (long_ != rows).sum() >= 64


@pytest.mark.parametrize("n", SIZES)
def test_the_rollout_draws_of_the_edge_rings(n):
    """learn_ppo_cases.rollout_table is rollout_draw draw for draw (checked on the first four draws); on the rings of 701 and 1025
    rows the whole-ring window's tables reach rows beyond 255 and 511, and the window of the last 300 rows starts beyond slot 0 and
    is longer than one pass of the 256-thread loop."""
    rows, keys = _edge(n)
    as_int = [int(k) for k in keys]
    for calls in (0, 3):
        whole = oc.window_slots(0, n, n + 2)
        assert whole == list(range(n))
        table = oc.rollout_table(keys, whole, SEED, 0, calls, 64)
        assert table.min() >= 0 and table.max() < n
        for d, salt in enumerate(pc._salts(SEED, 0, calls, _lib.SITE_LEARN_ROLLOUT, 4)):
            assert oc.rollout_draw(as_int, whole, int(salt)) == table[d]
        print("n %d calls %d: %d distinct rows, %d beyond row 255, %d beyond row 511" % (n, calls, len(np.unique(table)), int((table >= 256).sum()), int((table >= 512).sum())))
        if n >= 701:
            assert (table >= 256).sum() >= 10 and (table >= 512).sum() >= 5
            last = oc.window_slots(n - 300, n, n + 2)
            assert last == list(range(n - 300, n))
            t300 = oc.rollout_table(keys, last, SEED, 0, calls, 64)
            assert t300.min() >= n - 300 and (t300 >= n - 300 + 256).sum() >= 3            # rows only the second pass reaches
            bounded = oc.rollout_table(keys, whole[:256], SEED, 0, calls, 64)              # a draw bounded at 256 rows must disagree
            assert (bounded != table).sum() >= 32
        one = oc.rollout_table(keys, oc.window_slots(n - 1, n, n), SEED, 0, calls, 64)
        assert (one == n - 1).all()
    assert oc.row_key(rows, n - 1, rows["ring_age"][n - 1]) == as_int[n - 1]               # (the two key models agree, ages included)
    assert not oc.rollout_table(keys, [], SEED, 0, 0, 8).any()


def test_the_wrapped_windows_and_stamps_of_capacity_1001():
    """seen 990 -> count 1100 on 1001 rows: slots 990..1000 and 0..98 -- the rollout's window and the rows rl_learn_td_draw stamps."""
    w = oc.window_slots(990, 1100, 1001)
    assert w == list(range(990, 1001)) + list(range(0, 99)) and len(w) == 110
    old = np.full(1001, 0.5, np.float32)
    st = tc.stamp(old, 990, 1100, np.float32(0.25))
    assert sorted(np.nonzero(st == 0.25)[0].tolist()) == sorted(w) and (st[99:990] == 0.5).all()
    assert (tc.stamp(st, 1100, 2101, np.float32(0.125)) == 0.125).all()                     # a whole capacity of new rows
    assert tc.stamp(st, 2101, 2101, np.float32(4.0)).tobytes() == st.tobytes()              # nothing new


# ---- 2. PPO on trained weights -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_the_ppo_rollouts_on_trained_weights_take_every_branch_and_keep_off_the_kinks(which):
    """Rollouts of 32, 31, 17 and 1 rows of learn_ppo_cases.edge_case(): rows in smooth-L1's linear region, rows whose clamp stops the
    gradient, rows outside the clip range on the side that passes (the one-row rollout excepted); every ratio at least 1e-4 from both
    clip bounds and every |v - td| at least 1e-4 from 1, so that a float32 kernel sits on the same side of every kink as float64; torch's
    float32 autograd within 1e-6 of float64 on the gradients (relative to each tensor's largest entry) and on the loss."""
    torch.set_num_threads(1)
    w, rows, prob, rollouts = oc.edge_case()
    slots = rollouts[which]
    assert len(slots) == oc.EDGE_ROLLOUT_ROWS[which] and prob.dtype == np.float32 and (prob > 0).all()
    batch = oc.rows_of(rows, prob, slots)
    loss64, g64, mid = oc.grads_autograd(w, batch)
    hand_loss, hand, hmid = oc.grads_by_hand(w, batch)
    ratio, adv, d = mid["ratio"], mid["adv"], mid["v"] - mid["td"]
    lo, hi = 1 - oc.EPS_CLIP, 1 + oc.EPS_CLIP
    linear = int((np.abs(d) > 1).sum())
    stopped = int((hmid["coef"] == 0).sum())
    passing = int((((ratio < lo) | (ratio > hi)) & (hmid["coef"] == 1)).sum())
    kink_ratio = float(np.minimum(np.abs(ratio - lo), np.abs(ratio - hi)).min())
    kink_v = float(np.abs(np.abs(d) - 1).min())
    loss32, g32, _ = oc.grads_autograd(w, oc.rows_of(rows, prob, slots, torch.float32), torch.float32)
    gerr = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g32, g64) if np.abs(b).max() > 0)
    herr = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(hand, g64) if np.abs(b).max() > 0)
    lerr = abs(loss32 - loss64) / abs(loss64)
    print("rows %d: %d in smooth-L1's linear region, %d stopped by the clamp, %d outside the clip range on the passing side; max |adv| %.3g; "
          "nearest ratio to a clip bound %.3g, nearest |v - td| to 1 %.3g; torch float32: gradients %.3g, loss %.3g; by hand against autograd %.3g"
          % (len(slots), linear, stopped, passing, np.abs(adv).max(), kink_ratio, kink_v, gerr, lerr, herr))
    assert kink_ratio >= 1e-4 and kink_v >= 1e-4
    assert gerr <= 1e-6 and lerr <= 1e-6 and herr <= 1e-12 and abs(hand_loss - loss64) <= 1e-12 * abs(loss64)
    if len(slots) > 1:
        assert linear >= 2 and stopped >= 5 and passing >= 5 and linear < len(slots)
        assert np.abs(adv).max() > 3 and all(np.abs(b).max() > 0 for b in g64)
    assert w.tobytes() != oc.golden()["init"].tobytes() and w.size == oc.N_PARAMS          # (the trained network, not the fixture's initial one)


def test_what_a_replay_at_the_wrong_step_makes_of_adam_at_step_ten_thousand():
    """What the late-step tests can catch: Adam replayed at t = 3 instead of t = 10000 on the PPO, PERDQN and DQN moments of
    learn_d3qn_cases.adam_moments misses the 1e-5 lr + 1 ulp bar on most parameters (the bias corrections 1 - 0.9^t and 1 - 0.999^t
    differ by 3.7 and 330 times), so a kernel that took its step number from the call alone (s + 1, without the steps taken before)
    cannot pass.  An off-by-one is NOT visible this late (0.999^10000 is 4.5e-5: t = 9999 moves no parameter beyond the bar, printed);
    that is what the fixtures' steps 1..9 are for."""
    for n, lr in ((oc.N_PARAMS, oc.LR), (tc.N_PARAMS, 1e-3), (lc.N_PARAMS, wc.LR)):
        m0, v0 = dc.adam_moments(n)
        g = np.random.RandomState(3).normal(0, 1e-3, n)
        p0 = np.random.RandomState(4).normal(0, 0.1, n).astype(np.float32).astype(np.float64)
        right = lc.adam64(p0, m0.astype(np.float64), v0.astype(np.float64), g, 10000, lr)[0]
        for t in (3, 9999):
            wrong = lc.adam64(p0, m0.astype(np.float64), v0.astype(np.float64), g, t, lr)[0]
            bound = 1e-5 * lr + np.spacing(np.abs(right).astype(np.float32)).astype(np.float64)
            missed = float((np.abs(wrong - right) > bound).mean())
            print("%d parameters, replay at t = %d: %.3g of them beyond 1e-5 lr + 1 ulp" % (n, t, missed))
            assert missed > 0.5 or t != 3


# ---- 3. PERDQN on trained weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_torch_float32_is_inside_the_bars_on_the_trained_perdqn_weights(which):
    """learn_perdqn_cases.edge_case(): |w| up to 2.05, |pred| and |target| in the hundreds, unequal importance weights; torch's float32
    autograd within 1e-6 of float64 on gradients and loss, a tenth of the bar the kernel is held to; the new priorities within the
    kernel's bound."""
    torch.set_num_threads(1)
    w, tgt, rows, pri, batches = tc.edge_case()
    slots = batches[which]
    assert len(slots) == tc.EDGE_BATCHES[which] and (pri > 0).all() and int((pri == tc.golden()["p_new"]).sum()) == 147
    assert np.array_equal(tgt, w * lc.TARGET_SCALE) and w.size == tc.N_PARAMS
    isw = tc.is_weights(pri[slots], 0.401)
    loss64, g64, prio64, pred, target = tc.step(w, tgt, rows, slots, isw, 0.99)
    loss32, g32, prio32, _, _ = tc.step(w, tgt, rows, slots, isw, 0.99, torch.float32)
    gerr = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g32, g64))
    lerr = abs(loss32 - loss64) / abs(loss64)
    scale = max(np.abs(tc.q_values(w, rows["ring_state"][slots])).max(), np.abs(tc.q_values(tgt, rows["ring_state_prime"][slots])).max(), np.abs(target).max())
    perr = float(np.abs(prio32 - prio64).max())
    print("batch %d: max |w| %.3g, max |pred| %.4g, max |target| %.4g, mean(w) %.3g, loss %.6g; torch float32: gradients %.3g, loss %.3g, priorities %.3g (bound %.3g)"
          % (len(slots), np.abs(w).max(), np.abs(pred).max(), np.abs(target).max(), isw.mean(), loss64, gerr, lerr, perr, 3.8e-5 * scale))
    assert gerr <= 1e-6 and lerr <= 1e-6 and perr <= 3.8e-5 * scale
    assert all(np.abs(b).max() > 0 for b in g64) and np.abs(w).max() > 2.0
    if len(slots) > 1:
        assert np.abs(pred).max() > 30 and np.abs(target).max() > 100 and isw.mean() < 0.5
    else:
        assert isw.tolist() == [1.0]


def test_the_beta_cap_changes_the_weights_it_is_tested_on():
    """What the beta test can catch: from 0.9995 both steps' beta is exactly 1.0; without the cap it would be 1.0005 and 1.0015, and
    the fixture's importance weights would differ from (p / p_min) ** -1 by far more than 1 float32 ulp."""
    g, p = dc.golden(), tc.golden()
    b1 = min(1.0, 0.9995 + 0.001)
    b2 = min(1.0, b1 + 0.001)
    assert b1 == 1.0 and b2 == 1.0 and 0.9995 + 0.001 > 1.0
    pri = p["prio_init"][g["slots"][0]]
    capped, free = tc.is_weights(pri, 1.0).astype(np.float32), tc.is_weights(pri, 0.9995 + 0.001).astype(np.float32)
    ulps = np.abs(capped - free) / np.spacing(capped)
    print("beta 1.0 against 1.0005: weights differ by up to %.3g ulp" % ulps.max())
    assert ulps.max() > 100 and len(set(pri.tolist())) > 1


# ---- 4. the wide update at its own sizes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2048, 2017, 1000])
def test_torch_float32_is_inside_the_bars_at_the_wide_batches(batch):
    """learn_wide_cases.edge_case(batch, n_rows=1027): 64 tiles, 64 tiles with a one-row last tile, 32 tiles with a last tile of 8; torch
    float32 within 1e-6 of float64; fc3.weight has exact zeros; the tile-by-tile loss model is the float64 loss; the work buffer's size."""
    torch.set_num_threads(1)
    w, tgt, rows, slots, loss64, g64 = wc.edge_case(batch, n_rows=1027)
    assert len(slots) == batch and slots.max() < 1027 and wc.tiles(batch) == {2048: 64, 2017: 64, 1000: 32}[batch]
    assert batch - (wc.tiles(batch) - 1) * 32 == {2048: 32, 2017: 1, 1000: 8}[batch]
    loss32, g32 = lc.grads64(w, tgt, rows, slots, wc.GAMMA, dtype=torch.float32)
    gerr = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g32, g64))
    lerr = abs(loss32 - loss64) / abs(loss64)
    model, per_tile = wc.tile_loss_model(w, tgt, rows, slots)
    print("batch %d: %d distinct slots, fc3.weight exact zeros %d; torch float32: gradients %.3g, loss %.3g; tile loss model against float64 %.3g"
          % (batch, len(np.unique(slots)), int((g64[4] == 0).sum()), gerr, lerr, abs(model - loss64) / loss64))
    assert gerr <= 1e-6 and lerr <= 1e-6 and abs(model - loss64) <= 1e-12 * loss64 and per_tile.shape == (wc.tiles(batch),)
    assert (g64[4] == 0).sum() >= 8 and len(np.unique(slots)) > 600
    assert wc.work_bytes(2048) == 7293248 and int(_lib.lib().rl_learn_wide_work_bytes(_lib.DQN, batch)) == wc.work_bytes(batch)


def test_a_sum_over_fewer_tiles_misses_the_bar():
    """What the 64-tile test can catch: the gradient of the first 63 tiles of batch 2048 (scaled by the whole batch, as a cross-tile
    sum that stopped one tile early would leave it) is far beyond 1e-5 of the full one, and so is a loss without the last tile."""
    w, tgt, rows, slots, loss64, g64 = wc.edge_case(2048, n_rows=1027)
    loss63, g63 = lc.grads64(w, tgt, rows, slots[:2016], wc.GAMMA)
    worst = min(float(np.abs(a * (2016 / 2048) - b).max() / np.abs(b).max()) for a, b in zip(g63, g64))
    model, per_tile = wc.tile_loss_model(w, tgt, rows, slots)
    short = per_tile[:63].sum() / 2048
    print("63 of 64 tiles: the least wrong gradient tensor is %.3g off, the loss %.3g" % (worst, abs(short - loss64) / loss64))
    assert worst > 1e-3 and abs(short - loss64) > 1e-4 * loss64


def test_the_wide_draw_table_and_the_late_bad_slots():
    """The content-key draw of 4,096 slots on 1025 rows names rows beyond 255 and 511; the bad-slot tables put their entry where only a
    later pass of the checks' strided loops (256 / 512 threads) reaches it."""
    _, keys = _edge(1025)
    table = pc.host_uniform_draw(keys, SEED, 0, 0, 4096)
    assert table.max() < 1025 and (table >= 512).sum() > 1000 and len(np.unique(table)) > 900
    assert 300 >= 256 and 2 * 160 > 300 and 300 // 160 == 1                               # wide: index 300 of 320, step 1
    assert 20 * 32 > 600 >= 512 and 600 // 32 == 18 and 10 * 64 > 600 and 600 // 64 == 9   # PPO and PERDQN: index 600 of 640
