"""CPU: what tests/test_hip_learn_ppo_wide.py rests on, in float64 over all three epochs (learn_ppo_cases.grads_by_hand + adam64) for the
rollouts of 33, 64, 65, 96, 130 and 2048 rows on learn_ppo_cases.edge_case(): no row's ratio within 1e-5 of a clip bound and no row's
|v - td| within 1e-3 of 1 (a float32 kernel and float64 autograd then sit on the same side of every kink), the hand-written gradients
equal to autograd, a per-tile restart of the GAE recursion far outside the GPU test's bar wherever a tile is full -- and the host side of
rl_learn_ppo_wide: the work buffer's size, the entry-point row, and the conditions of learn_batch={"PPO": B}.
Measured with exactly these inputs: the smallest ratio-to-bound distance over all batches and epochs is 1.6e-4 (2048 rows, epoch 3), the
smallest ||v - td| - 1| is 0.83, hand-written against autograd 1e-15; the restart moves the six trunk and policy-head gradients by 0.03 ..
0.6 of each tensor's largest at 64 rows and more, and by only 0.9e-4 .. 1.3e-4 at 33 rows (9 times the bar: 33 rows alone do not pin the
chain, so 64 and more are in the GPU list); fc_v's gradients do not depend on the advantage."""
import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_ppo_cases as pc
import learn_ppo_wide_cases as wc

BAR = 1e-5   # the GPU test's bar on a gradient tensor, relative to its largest magnitude


@pytest.mark.parametrize("batch", wc.MULTI_TILE)
def test_no_row_sits_at_a_kink_and_hand_written_gradients_are_autograds(batch):
    _, ring, prob, _ = pc.edge_case()
    rows = pc.rows_of(ring, prob, wc.wide_slots(batch))
    lo, hi = 1 - pc.EPS_CLIP, 1 + pc.EPS_CLIP
    for ep, (p, loss, grads, mid) in enumerate(wc.replay(batch)):
        to_bound = float(np.minimum(np.abs(mid["ratio"] - lo), np.abs(mid["ratio"] - hi)).min())
        to_one = float(np.abs(np.abs(mid["v"] - mid["td"]) - 1).min())
        loss_a, grads_a, _ = pc.grads_autograd(p, rows)
        err = max(float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(grads, grads_a))
        print("rows %d epoch %d: ratio to a clip bound >= %.3g, ||v - td| - 1| >= %.3g, hand-written against autograd %.3g, ratios %.3g .. %.3g"
              % (batch, ep + 1, to_bound, to_one, err, mid["ratio"].min(), mid["ratio"].max()))
        assert to_bound > 1e-5 and to_one > 1e-3
        assert err <= 1e-12 and abs(loss - loss_a) <= 1e-12 * abs(loss_a)
        assert (mid["ratio"] < lo).any() and (mid["ratio"] > hi).any() or batch < 64   # both clamp branches are taken


@pytest.mark.parametrize("batch", wc.MULTI_TILE)
def test_a_per_tile_restart_of_the_gae_chain_would_be_caught(batch):
    _, ring, prob, _ = pc.edge_case()
    rows = pc.rows_of(ring, prob, wc.wide_slots(batch))
    p, _, whole, mid = wc.replay(batch)[0]
    _, tiled, mid_t = wc.grads_by_hand_per_tile(p, rows)
    assert np.array_equal(mid_t["adv"][-(batch % 32 or 32):], mid["adv"][-(batch % 32 or 32):])   # the last tile's rows start the chain either way
    assert not np.array_equal(mid_t["adv"][:32], mid["adv"][:32])
    diff = {n: float(np.abs(a - b).max() / np.abs(b).max()) for n, a, b in zip(pc.NAMES, tiled, whole)}
    print("rows %d: a per-tile restart moves the gradients by %s of their largest" % (batch, ", ".join("%s %.3g" % kv for kv in diff.items())))
    assert diff["fc_v.weight"] == 0 and diff["fc_v.bias"] == 0          # dL/dv does not see the advantage
    moved = [diff[n] for n in pc.NAMES[:6]]
    assert min(moved) > (1000 * BAR if batch >= 64 else 5 * BAR)       # 33 rows: the restart costs one row of one tile its tail


def test_the_work_buffer_is_the_headers_formula():
    lib = _lib.lib()
    for batch in (1, 17, 32, 33, 64, 65, 96, 130, 2047, 2048):
        assert lib.rl_learn_ppo_wide_work_bytes(_lib.PPO, batch) == wc.work_bytes(batch), batch
    assert wc.work_bytes(32) == 64 + 430388 and wc.work_bytes(2048) == 27544896 and wc.work_bytes(33) == wc.work_bytes(64)
    for kind, batch, says in ((_lib.PPO, 0, b"[1,2048]"), (_lib.PPO, 2049, b"[1,2048]"), (_lib.DQN, 64, b"kind 0"), (_lib.PERDQN, 64, b"kind 4")):
        assert lib.rl_learn_ppo_wide_work_bytes(kind, batch) == 0 and says in lib.rl_last_error()
    assert [lib.rl_learn_ppo_wide_supported(k) for k in range(6)] == [0, 0, 0, 1, 0, 0]
    assert _lib.LEARN_PPO_WIDE_MAX == wc.WIDE_MAX == 2048


def test_the_entry_points_refuse_on_the_host_before_anything_is_launched():
    """Null arguments reach no device: RL_E_INVALID naming the argument."""
    import ctypes as C
    lib = _lib.lib()
    one = (_lib.Learner * 1)(); rings = (_lib.Replay * 1)(); ppos = (_lib.Ppo * 1)(); work = (C.c_void_p * 1)()
    assert lib.rl_learn_ppo_wide(None, one, rings, ppos, 1, 1, None, work, None) == -1 and b"null handle" in lib.rl_last_error()
    assert lib.rl_learn_rollout_wide(None, one, rings, ppos, 1, 1, None, None) == -1 and b"null handle" in lib.rl_last_error()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    try:
        slots = C.c_void_p(16)   # (never dereferenced: every call below is refused first)
        assert lib.rl_learn_ppo_wide(h, one, rings, ppos, 1, 1, slots, None, None) == -1 and b"null work" in lib.rl_last_error()
        assert lib.rl_learn_ppo_wide(h, None, rings, ppos, 1, 1, slots, work, None) == -1 and b"null learners" in lib.rl_last_error()
        assert lib.rl_learn_ppo_wide(h, one, rings, ppos, 0, 1, slots, work, None) == -1 and b"n_learners" in lib.rl_last_error()
        assert lib.rl_learn_ppo_wide(h, one, rings, ppos, 1, 0, slots, work, None) == -1 and b"n_steps" in lib.rl_last_error()
        assert lib.rl_learn_ppo_wide(h, one, rings, ppos, 1, 1, None, work, None) == -1 and b"rl_learn_rollout_wide" in lib.rl_last_error()
        assert lib.rl_learn_ppo_wide(h, one, rings, ppos, 1, 1, slots, work, None) == -4 and b"kind 0" in lib.rl_last_error()   # RL_DQN
        assert lib.rl_learn_rollout_wide(h, one, rings, ppos, 1, 1, slots, None) == -4 and b"rl_learn_ppo_wide_supported" in lib.rl_last_error()
    finally:
        lib.rl_destroy(h)


def test_the_table_row_and_its_launch_count():
    from reinlife_amd.learn import ALL_ENTRIES, ENTRIES, ENTRY, MORE_ENTRIES
    assert ALL_ENTRIES == ENTRIES + MORE_ENTRIES and len(ENTRIES) == 8 and set(ENTRY) == {x.name for x in ALL_ENTRIES}
    e = ALL_ENTRIES[-1]
    assert (e.name, e.method, e.family, e.has_target, e.keyword, e.needs, e.narrow, e.batch_max, e.one_batch, e.draw, e.side) == (
        "rl_learn_ppo_wide", "PPO", "ppo", False, "rollout_batch", "rollout", "rl_learn_ppo", "LEARN_PPO_WIDE_MAX", True, "rl_learn_rollout_wide", _lib.Ppo)
    assert e.side_tensors == ENTRY["rl_learn_ppo"].side_tensors and e.work_bytes == "rl_learn_ppo_wide_work_bytes"
    assert e.per_epoch and [e.launches(1, 3), e.launches(2, 3), e.launches(1, 8)] == [wc.launches(1, 3), wc.launches(2, 3), wc.launches(1, 8)] == [12, 21, 27]
    for other in ALL_ENTRIES[:-1]:   # what the existing rows answer is what they answered
        assert not other.per_epoch and other.launches(2) in (1, 7, 9)


P = dict(rollout=True)


@pytest.mark.parametrize("make, kwargs, says", [
    (Models.PPO, dict(rollout_batch=130), r"rollout_batch is for PPO brains with rollout=True \(rl_learn_ppo_wide\); got a PPO brain \(kind 3\) without rollout=True$"),
    (Models.D3QN, dict(rollout_batch=130, **P), r"rollout_batch is for PPO brains with rollout=True \(rl_learn_ppo_wide\); got a D3QN brain \(kind 1\)$"),
    (Models.PPO, dict(rollout_batch=130, wide_batch=64, **P), r"got a PPO brain \(kind 3\) with wide_batch$"),
    (Models.PPO, dict(rollout_batch=130, prioritized=True, **P), r"got a PPO brain \(kind 3\) with prioritized=True$"),
    (Models.PPO, dict(rollout_batch=0, **P), r"rollout_batch must be an int in \[1, 2048\] \(the rows of a minibatch of rl_learn_ppo_wide\)"),
    (Models.PPO, dict(rollout_batch=2049, **P), r"rollout_batch must be an int in \[1, 2048\]"),
    (Models.PPO, dict(rollout_batch=True, **P), r"rollout_batch must be an int in \[1, 2048\]"),
])
def test_device_learner_states_rollout_batchs_conditions_before_touching_a_gpu(make, kwargs, says, monkeypatch):
    import torch
    from reinlife_amd.learn import DeviceLearner
    brain = make()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(brain, "cuda:0", **kwargs)


def _brains():
    return [Models.DQN(max_epi=60), Models.PPO()]


DEVR = dict(learn="device", learn_rollout=True)
TAKES = (r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and, with learn_rollout=True, "
         r"'PPO' \(rl_learn_ppo_wide\), and at least one of them, got")


@pytest.mark.parametrize("kwargs, says", [
    # without learn_rollout=True the key stays unknown, with the text the other unknown keys get
    (dict(learn="device", learn_batch={"PPO": 130}),
     r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them, got"),
    (dict(learn_rollout=True, learn_batch={"PPO": 130}), "learn_rollout=True needs learn='device'"),
    (dict(learn_batch={}, **DEVR), TAKES),
    (dict(learn_batch={"PPO": 130, "PERD3QN": 64}, **DEVR), TAKES),
    (dict(learn_batch={"PPO": 0}, **DEVR), r"learn_batch\['PPO'\] must be an int in \[1, 2048\] \(the rows of a PPO minibatch, rl_learn_ppo_wide\)"),
    (dict(learn_batch={"PPO": 2049}, **DEVR), r"learn_batch\['PPO'\] must be an int in \[1, 2048\]"),
    (dict(learn_batch={"PPO": 64.0}, **DEVR), r"learn_batch\['PPO'\] must be an int in \[1, 2048\]"),
])
def test_learn_batch_ppo_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    with pytest.raises(ValueError, match=says):
        Environment(brains=_brains(), n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("kwargs", [dict(learn_batch={"PPO": 1}), dict(learn_batch={"PPO": 2048}, rollout_steps=2),
                                    dict(learn_batch={"PPO": np.int64(130), "DQN": 64}, learn_ranks="average")])
def test_learn_batch_ppo_passes_its_checks_where_a_learner_can_use_it(kwargs, monkeypatch):
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    with pytest.raises(Reached):
        trainer(_brains(), n_episodes=5, n_worlds=4, save=False, print_results=False, **DEVR, **kwargs)


def test_the_documents_say_what_runs():
    import reinlife_amd
    assert "rl_learn_ppo_wide" in reinlife_amd.Environment.learn_now.__doc__ and "rl_learn_ppo_wide" in reinlife_amd.trainer.__doc__
    assert "rl_learn_ppo_wide" in reinlife_amd.Environment._NOTES
