"""CPU: the inputs of tests/test_hip_learn_edges.py satisfy what its comparisons rest on -- the seeded rings have distinct content keys
that carry their ages, the float64 race of the prioritised draw has a gap of at least 1e-4 between first and second on every draw of
every size (so a few float32 ulp on the device cannot flip one), numpy's float32 model of the race agrees with the float64 one on every
draw, the draws of the larger rings reach rows that only a second pass of the kernels' 256-thread loops sees, and torch's own float32
autograd sits well inside the 1e-5 bars on the reference's trained weights.  Every figure a bar is held against is printed first."""
import numpy as np
import pytest
import torch

from reinlife_amd import _lib

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc

SEED = 11
SIZES = (1, 3, 255, 256, 257, 701, 1025)
_cache = {}


def _edge(n, seed=11):
    if seed not in _cache:
        rows = lc.edge_ring_rows(1027, seed)
        _cache[seed] = (rows, pc.content_keys(rows, 1027, rows["ring_age"]))
    rows, keys = _cache[seed]
    return {k: v[:n] for k, v in rows.items()}, keys[:n]


@pytest.mark.parametrize("seed", [11, 12])
def test_the_seeded_rings_have_distinct_keys_that_carry_their_ages(seed):
    rows, keys = _edge(1027, seed)
    assert len(set(keys.tolist())) == 1027
    age = rows["ring_age"]
    assert age.dtype == np.int32 and age.min() == 0 and age.max() == 199 and len(np.unique(age)) > 190
    without = pc.content_keys(rows, 1027)
    assert np.array_equal(keys[age == 0], without[age == 0]) and (keys[age != 0] != without[age != 0]).all() and (age == 0).any()
    assert np.array_equal(pc.content_keys(rows, 1027, np.zeros(1027, np.int32)), without)                  # (the default is age 0)
    assert set(np.unique(rows["ring_state"]).tolist()) == set(np.unique(rows["ring_state_prime"]).tolist()) == {0.0, 0.5, -0.5, 1.0, -1.0}
    assert set(np.unique(rows["ring_action"]).tolist()) == set(range(8))
    assert set(np.unique(rows["ring_reward"]).tolist()) == {float(np.float32(x)) for x in (0, 0.05, 0.3, -1, 5, -10, 400)}
    assert 0.15 < rows["ring_done"].mean() < 0.25 and set(np.unique(rows["ring_done"]).tolist()) == {0, 1}
    # the fixture rings' keys are what they were (age 0)
    g = dc.golden()
    assert np.array_equal(pc.content_keys(g, 48), pc.content_keys(g, 48, np.zeros(48, np.int32)))


@pytest.mark.parametrize("n", SIZES)
def test_the_uniform_draws_of_the_edge_rings(n):
    """The host model picks rows inside the ring; on the rings of 701 and 1025 rows every table reaches rows beyond 255 (what only a
    second pass of k_learn_pick's loop sees) and beyond 511; the lower slot wins equal values."""
    _, keys = _edge(n)
    for batch in (32, 64):
        for calls in (0, 3):
            rows = pc.host_uniform_draw(keys, SEED, 0, calls, 2 * batch)
            assert rows.shape == (2 * batch,) and rows.min() >= 0 and rows.max() < n
            print("n %d batch %d calls %d: %d distinct rows, %d beyond row 255, %d beyond row 511" % (n, batch, calls, len(np.unique(rows)), int((rows >= 256).sum()), int((rows >= 512).sum())))
            if n >= 701:
                assert (rows >= 256).sum() >= 10 and (rows >= 512).sum() >= 5
    assert not np.array_equal(pc.host_uniform_draw(keys, SEED, 0, 0, 64), pc.host_uniform_draw(keys, SEED, 0, 3, 64)) or n == 1
    twice = np.concatenate([keys, keys])                                                                   # equal keys: the lower slot
    assert np.array_equal(pc.host_uniform_draw(twice, SEED, 0, 0, 64), pc.host_uniform_draw(keys, SEED, 0, 0, 64))


def _race(keys, pri, brain, calls, n_draws):
    w64 = pri.astype(np.float64) ** 0.6
    rows, gaps = pc.host_draw64(keys, w64, SEED, brain, calls, n_draws)
    rows32 = pc.host_draw(keys, pri, SEED, brain, calls, n_draws)
    w32 = (pri ** np.float32(0.6)).astype(np.float32)
    rows_w32, gaps_w32 = pc.host_draw64(keys, w32, SEED, brain, calls, n_draws)
    return rows, gaps, rows32, rows_w32, gaps_w32


@pytest.mark.parametrize("n", SIZES)
def test_the_prioritised_race_has_a_gap_and_float32_agrees_with_float64(n):
    """128 draws at calls 3 per size: the smallest relative gap between the first and second t is at least 1e-4 in float64 (and on
    numpy's float32 weights); numpy's float32 race names the float64 winner in every draw; no row of priority 0 is drawn."""
    _, keys = _edge(n)
    pri = pc.edge_priorities(n)
    assert (pri[::7] == 0).all() if n > 3 else (pri > 0).all()
    rows, gaps, rows32, rows_w32, gaps_w32 = _race(keys, pri, 0, 3, 128)
    print("n %d: smallest gap %.3g (on float32 weights %.3g); float32 race differs in %d of 128 draws; %d distinct rows, %d beyond row 255"
          % (n, gaps.min(), gaps_w32.min(), int((rows32 != rows).sum()), len(np.unique(rows)), int((rows >= 256).sum())))
    assert gaps.min() >= 1e-4 and gaps_w32.min() >= 1e-4
    assert np.array_equal(rows32, rows) and np.array_equal(rows_w32, rows)
    assert (pri[rows] > 0).all()
    if n >= 701:
        assert (rows >= 256).sum() >= 10 and (rows >= 512).sum() >= 5
    if n == 1:
        assert np.isinf(gaps).all() and not rows.any()


@pytest.mark.parametrize("brain", [0, 1])
def test_the_mixed_learner_cases_have_the_gap_at_either_position(brain):
    """(batch 64, 257 rows, calls 3) and (batch 7, 96 rows of another ring, calls 1), each at brain index 0 and 1."""
    for batch, (_, keys), calls, pseed in ((64, _edge(257), 3, 5), (7, _edge(96, 12), 1, 6)):
        pri = pc.edge_priorities(len(keys), pseed)
        rows, gaps, rows32, rows_w32, gaps_w32 = _race(keys, pri, brain, calls, 2 * batch)
        print("brain %d batch %d: smallest gap %.3g (on float32 weights %.3g)" % (brain, batch, gaps.min(), gaps_w32.min()))
        assert gaps.min() >= 1e-4 and gaps_w32.min() >= 1e-4
        assert np.array_equal(rows32, rows) and np.array_equal(rows_w32, rows)
    k257 = _edge(257)[1]
    assert not np.array_equal(pc.host_uniform_draw(k257, SEED, 0, 3, 64), pc.host_uniform_draw(k257, SEED, 1, 3, 64))   # the position salts the draw


def test_with_no_weight_the_race_is_the_uniform_draw_on_the_prioritised_site():
    _, keys = _edge(257)
    zero = np.zeros(257, np.float32)
    rows, gaps = pc.host_draw64(keys, zero, SEED, 0, 3, 128)
    uni = pc.host_uniform_draw(keys, SEED, 0, 3, 128, site=_lib.SITE_LEARN_PRIO)
    assert np.array_equal(rows, uni) and np.array_equal(pc.host_draw(keys, zero, SEED, 0, 3, 128), uni) and np.isinf(gaps).all()
    assert not np.array_equal(uni, pc.host_uniform_draw(keys, SEED, 0, 3, 128))


def test_torch_float32_is_well_inside_the_bars_on_the_trained_weights():
    """The reference's trained weights (target: the same times 0.96875) on the fixture rings: torch's own float32 autograd against
    float64 -- gradients relative to each tensor's largest entry, the loss, and PERD3QN's priorities relative to the largest |q|, |q'|
    -- all below 1e-6, a tenth of the bar the kernels are held to."""
    torch.set_num_threads(1)
    assert float(lc.TARGET_SCALE) == 0.96875
    worst_w, worst_q = 0.0, 0.0
    for method, mod, g, gamma, batches in (("DQN", lc, lc.golden(), 0.98, (32,)), ("D3QN", dc, dc.golden(), 0.99, (64, 33)), ("PERD3QN", dc, dc.golden(), 0.99, (64, 33))):
        w, tgt = lc.pretrained(method)
        assert w.size == mod.N_PARAMS and tgt.dtype == np.float32 and np.array_equal(tgt, w * np.float32(0.96875))
        q = mod.q_values(w, g["ring_state"])
        worst_w, worst_q = max(worst_w, float(np.abs(w).max())), max(worst_q, float(np.abs(q).max()))
        for batch in batches:
            slots = g["slots"][0][:batch]
            loss64, g64 = mod.grads64(w, tgt, g, slots, gamma)
            loss32, g32 = mod.grads64(w, tgt, g, slots, gamma, dtype=torch.float32)
            gerr = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(g32, g64))
            lerr = abs(loss32 - loss64) / abs(loss64)
            print("%s batch %d: max |w| %.3g, max |q| %.3g, loss %.6g; torch float32: gradients %.3g, loss %.3g" % (method, batch, np.abs(w).max(), np.abs(q).max(), loss64, gerr, lerr))
            assert all(np.abs(b).max() > 0 for b in g64) and gerr <= 1e-6 and lerr <= 1e-6
            if method == "PERD3QN":
                p64, qa, qn = pc.priorities(w, tgt, g, slots)
                p32 = pc.priorities(w, tgt, g, slots, torch.float32)[0]
                scale = max(np.abs(qa).max(), np.abs(qn).max())
                perr = float(np.abs(p32 - p64).max() / scale)
                print("PERD3QN batch %d: torch float32 priorities %.3g of the scale %.4g" % (batch, perr, scale))
                assert perr <= 1e-6 and scale > 30 and p64.min() > 0
    assert worst_w > 1.7 and worst_q > 30                                                                   # (a trained network, not torch's initial one)


@pytest.mark.parametrize("method", ["D3QN", "DQN"])
def test_what_float32_makes_of_adam_at_step_ten_thousand(method):
    """torch's Adam step made of float32 operations (learn_d3qn_cases.adam32) at t = 10000 on moments N(0, 1e-3) and the squares of
    another such draw, from torch's float32 gradient of the fixture's first minibatch: its distance from float64 in the units the GPU test
    asserts, printed.  Asserted: the steps reach hundreds of lr -- m / sqrt(v) of two independent normal draws has heavy tails -- so a float32
    rounding of the step is no longer small against 1e-5 lr; m + 0.1 (g - m) cancels where g is near -9 m, so a rounding of 0.1 (g - m) is
    many ulp of the sum; and float32 operations do miss the GPU test's bars on these inputs -- which is why adam_update
    (reinlife_amd/csrc/rl_learn_dev.h) takes double arithmetic and rounds each of p, m and v once: that meets them by construction
    (half an ulp each)."""
    mod, g = (lc, lc.golden()) if method == "DQN" else (dc, dc.golden())
    lr, gamma, tgt = (0.0005, 0.98, g["init"]) if method == "DQN" else (1e-3, 0.99, g["target_init"])
    m0, v0 = dc.adam_moments(mod.N_PARAMS)
    assert abs(m0.std() - 1e-3) < 2e-5 and (v0 >= 0).all() and abs(np.sqrt(v0.mean()) - 1e-3) < 2e-5
    torch.set_num_threads(1)
    grad = np.concatenate([x.reshape(-1) for x in mod.grads64(g["init"], tgt, g, g["slots"][0], gamma, dtype=torch.float32)[1]]).astype(np.float32)
    p32, m32, v32 = dc.adam32(g["init"], m0, v0, grad, 10000, lr)
    p64, m64, v64 = mod.adam64(g["init"].astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), grad.astype(np.float64), 10000, lr)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    assert p32.dtype == m32.dtype == v32.dtype == np.float32
    perr, bound, step = np.abs(p32 - p64), 1e-5 * lr + ulp(p32), np.abs(p64 - g["init"])
    merr, verr = np.abs(m32 - m64) / ulp(m64), np.abs(v32 - v64) / ulp(v64)
    print("%s: float32 operations against float64: parameters worst %.3g of (1e-5 lr + 1 ulp), %d of %d beyond it; largest step %.3g lr; m worst %.3g ulp (%d beyond 1); v worst %.3g ulp (%d beyond 1)"
          % (method, (perr / bound).max(), int((perr > bound).sum()), perr.size, step.max() / lr, merr.max(), int((merr > 1).sum()), verr.max(), int((verr > 1).sum())))
    assert step.max() > 100 * lr
    assert (perr > bound).any() and (merr > 1).any() and (verr > 1).any()
    once = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    assert (np.abs(once(p64) - p64) <= bound).all() and (np.abs(once(m64) - m64) <= ulp(m64)).all() and (np.abs(once(v64) - v64) <= ulp(v64)).all()
    assert (np.abs(m64) < 1e-3 * np.abs(0.1 * (grad.astype(np.float64) - m0))).any()
