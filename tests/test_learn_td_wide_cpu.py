"""CPU: what tests/test_hip_learn_td_wide.py rests on, in float64 (learn_td_wide_cases.step64) on the GPU tests' own inputs at 65, 96 and
128 rows -- a p_min taken per tile and a mean(is_w) taken per tile each miss the GPU test's bar by far, so the inputs can tell the
prescribed computation from the two tilings that need no weights pass; the prescribed order of mean(is_w) (tile sums in f32, then double,
rounded once) stays within the bar -- and the host side of rl_learn_td_wide: the work buffer's size, the refusals that need no device,
the entry-point row, and the conditions of td_batch and learn_batch={"PERDQN": B}.
Measured with exactly these inputs (worst gradient tensor, relative to its largest magnitude; the bar is 1e-5): p_min per tile 0.934 /
0.637 / 0.518 at 65 / 96 / 128 rows (every tensor and the loss alike: the error is one common factor), mean(is_w) per tile 0.0452 / 0.0823 /
0.0327 (the least-moved tensor: 0.0446 / 0.047 / 0.0125), the prescribed order 5.4e-8 / 1.3e-7 / 2.5e-8."""
import ctypes as C
import inspect

import numpy as np
import pytest

from reinlife_amd import Models, _lib

import learn_perdqn_cases as tc
import learn_td_wide_cases as wc

CPU_BATCHES = (65, 96, 128)


@pytest.mark.parametrize("batch", CPU_BATCHES)
def test_per_tile_scalars_would_be_caught_and_the_prescribed_order_is_within_the_bar(batch):
    p = tc.golden()
    slots, pri, w, loss64, g64 = wc.case(batch)
    ring = wc.ring_of(batch)
    assert abs(w.mean() - 1) > 0.05 and np.argmin(pri[slots]) >= wc.TILE * (wc.tiles(batch) - 1)   # mean_w != 1; p_min in the last tile only
    wrong = {"p_min per tile": wc.per_tile_p_min_scale(pri[slots], wc.BETA1), "mean_w per tile": wc.per_tile_mean_w_scale(pri[slots], wc.BETA1)}
    for name, scale in wrong.items():
        loss, grads = wc.step64(p["init"], p["target_init"], ring, slots, scale)
        worst, per = wc.worst_relative_error(grads, g64)
        least = min(per)
        print("rows %d: %s moves the gradients by %.3g .. %.3g of their largest (bar %.0e), the loss by %.3g"
              % (batch, name, least, worst, wc.BAR, abs(loss - loss64) / abs(loss64)))
        assert worst >= 10 * wc.BAR, name
    mean_w, w32 = wc.prescribed_mean_w(pri[slots], wc.BETA1)
    loss, grads = wc.step64(p["init"], p["target_init"], ring, slots, np.float64(mean_w))
    worst, _ = wc.worst_relative_error(grads, g64)
    print("rows %d: the prescribed order gives mean_w %.9g (float64 %.17g): gradients within %.3g of their largest, loss within %.3g"
          % (batch, mean_w, w.mean(), worst, abs(loss - loss64) / abs(loss64)))
    assert worst <= wc.BAR and abs(loss - loss64) <= wc.BAR * abs(loss64)
    assert (np.abs(w32 - w.astype(np.float32)) <= np.spacing(w.astype(np.float32))).all()


def test_one_tile_of_the_prescribed_order_is_the_narrow_kernels_float():
    """With one tile the double sum from -0.0 hands the tile's f32 sum back: mean_w is sum * (1.0f / B), rl_learn_td's expression."""
    pri = wc.priorities(96)
    for batch in wc.ONE_TILE_BATCHES:
        rows = pri[wc.slots_of(batch, seed=7)[0] % 96]
        mean_w, w = wc.prescribed_mean_w(rows, wc.BETA1)
        s = np.float32(0.0)
        for x in w:
            s = np.float32(s + x)
        assert mean_w.tobytes() == np.float32(s * (np.float32(1.0) / np.float32(batch))).tobytes()


def test_the_work_buffer_is_the_headers_formula():
    lib = _lib.lib()
    for batch in (1, 17, 64, 65, 96, 128, 130, 2047, 2048):
        assert lib.rl_learn_td_wide_work_bytes(_lib.PERDQN, batch) == wc.work_bytes(batch), batch
    assert wc.work_bytes(64) == 64 + 58144 + 16 and wc.work_bytes(2048) == 64 + 32 * 58144 + 128 and wc.work_bytes(65) == wc.work_bytes(128)
    for kind, batch, says in ((_lib.PERDQN, 0, b"[1,2048]"), (_lib.PERDQN, 2049, b"[1,2048]"), (_lib.DQN, 64, b"kind 0"), (_lib.PERD3QN, 64, b"kind 2")):
        assert lib.rl_learn_td_wide_work_bytes(kind, batch) == 0 and says in lib.rl_last_error()
    assert [lib.rl_learn_td_wide_supported(k) for k in range(6)] == [0, 0, 0, 0, 1, 0]
    assert _lib.LEARN_TD_WIDE_MAX == wc.WIDE_MAX == 2048


def test_the_entry_points_refuse_on_the_host_before_anything_is_launched():
    """Null arguments reach no device: RL_E_INVALID naming the argument; another kind: RL_E_UNSUPPORTED naming it."""
    lib = _lib.lib()
    one = (_lib.Learner * 1)(); rings = (_lib.Replay * 1)(); tds = (_lib.TdPrio * 1)(); work = (C.c_void_p * 1)()
    assert lib.rl_learn_td_wide(None, one, rings, tds, 1, 1, None, work, None) == -1 and b"null handle" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw(None, one, rings, tds, 1, 1, None, None) == -1 and b"null handle" in lib.rl_last_error()
    assert lib.rl_learn_td_wide_draw_rank(None, one, rings, tds, 1, 1, 1, None, None, None, None, None) == -1 and b"null handle" in lib.rl_last_error()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    try:
        slots = C.c_void_p(16)   # (never dereferenced: every call below is refused first)
        assert lib.rl_learn_td_wide(h, one, rings, tds, 1, 1, slots, None, None) == -1 and b"null work" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, None, rings, tds, 1, 1, slots, work, None) == -1 and b"null learners" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, one, rings, tds, 0, 1, slots, work, None) == -1 and b"n_learners" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, one, rings, tds, 1, 0, slots, work, None) == -1 and b"n_steps" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, one, rings, tds, 1, 65537, slots, work, None) == -1 and b"[1,65536]" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, one, rings, tds, 1, 1, None, work, None) == -1 and b"drawn by rl_learn_td_wide_draw" in lib.rl_last_error()
        assert lib.rl_learn_td_wide(h, one, rings, tds, 1, 1, slots, work, None) == -4 and b"kind 0" in lib.rl_last_error()   # RL_DQN
        assert b"RL_PERDQN (4)" in lib.rl_last_error() and b"rl_learn_td_wide_supported" in lib.rl_last_error()
        assert lib.rl_learn_td_wide_draw(h, one, rings, tds, 1, 1, slots, None) == -4 and b"rl_learn_td_wide_supported" in lib.rl_last_error()
        assert lib.rl_learn_td_wide_draw_rank(h, one, rings, tds, 1, 1, 1, None, None, None, slots, None) == -1 and b"null order" in lib.rl_last_error()
        # the narrow entries' messages are what they were
        assert lib.rl_learn_td(h, one, rings, tds, 1, 1, None, None) == -1 and lib.rl_last_error().endswith(b"drawn by rl_learn_td_draw")
        assert lib.rl_learn_td(h, one, rings, tds, 1, 1, slots, None) == -4 and lib.rl_last_error().endswith(b"RL_PERDQN (4) only (rl_learn_td_supported)")
    finally:
        lib.rl_destroy(h)


def test_the_table_row_and_its_launch_count():
    from reinlife_amd.learn import ALL_ENTRIES, ENTRIES, ENTRY, MORE_ENTRIES
    assert ALL_ENTRIES == ENTRIES + MORE_ENTRIES and len(ENTRIES) == 8 and set(ENTRY) == {x.name for x in ALL_ENTRIES}
    e = ENTRY["rl_learn_td_wide"]
    assert e in MORE_ENTRIES and e not in ENTRIES
    assert (e.name, e.method, e.family, e.has_target, e.keyword, e.needs, e.narrow, e.batch_max, e.one_batch, e.draw, e.draw_rank, e.side) == (
        "rl_learn_td_wide", "PERDQN", "td", True, "td_batch", "td_priority", "rl_learn_td", "LEARN_TD_WIDE_MAX", True, "rl_learn_td_wide_draw",
        "rl_learn_td_wide_draw_rank", _lib.TdPrio)
    assert e.side_tensors == ENTRY["rl_learn_td"].side_tensors and e.ring_rows == ENTRY["rl_learn_td"].ring_rows == "memory_size"
    assert e.work_bytes == "rl_learn_td_wide_work_bytes" and e.supported == "rl_learn_td_wide_supported" and not e.per_epoch
    assert [e.launches(1), e.launches(2), e.launches(3)] == [wc.launches(1), wc.launches(2), wc.launches(3)] == [6, 9, 12]
    assert [x.draw_rank for x in ALL_ENTRIES if x is not e] == [None] * 9     # the other rows keep the family's rank draw
    assert [x.name for x in ALL_ENTRIES if x.keyword == "td_batch"] == ["rl_learn_td_wide"]
    assert "td_batch" in ENTRY["rl_learn_ppo_wide"].conflicts


def test_td_batch_is_keyword_only_and_the_pinned_names_keep_their_places():
    from reinlife_amd.learn import DeviceLearner
    params = inspect.signature(DeviceLearner.__init__).parameters
    assert list(params)[-2:] == ["wide_batch", "dueling_batch"]
    assert params["td_batch"].kind is inspect.Parameter.KEYWORD_ONLY and params["td_batch"].default is None


T = dict(td_priority=True)


@pytest.mark.parametrize("make, kwargs, says", [
    (Models.PERDQN, dict(td_batch=130), r"td_batch is for PERDQN brains with td_priority=True \(rl_learn_td_wide\); got a PERDQN brain \(kind 4\) without td_priority=True$"),
    (Models.D3QN, dict(td_batch=130, **T), r"td_batch is for PERDQN brains with td_priority=True \(rl_learn_td_wide\); got a D3QN brain \(kind 1\)$"),
    (Models.PERDQN, dict(td_batch=130, wide_batch=64, **T), r"got a PERDQN brain \(kind 4\) with wide_batch$"),
    (Models.PERDQN, dict(td_batch=130, dueling_batch=64, **T), r"got a PERDQN brain \(kind 4\) with dueling_batch$"),
    (Models.PERDQN, dict(td_batch=130, prioritized=True, **T), r"got a PERDQN brain \(kind 4\) with prioritized=True$"),
    (Models.PERDQN, dict(td_batch=130, rollout=True, **T), r"got a PERDQN brain \(kind 4\) with rollout=True$"),
    (Models.PERDQN, dict(td_batch=130, rollout_batch=64, **T), r"rollout_batch is for PPO brains with rollout=True \(rl_learn_ppo_wide\); got a PERDQN brain \(kind 4\)"),
    (Models.PERDQN, dict(td_batch=0, **T), r"td_batch must be an int in \[1, 2048\] \(the rows of a minibatch of rl_learn_td_wide\)"),
    (Models.PERDQN, dict(td_batch=2049, **T), r"td_batch must be an int in \[1, 2048\]"),
    (Models.PERDQN, dict(td_batch=True, **T), r"td_batch must be an int in \[1, 2048\]"),
    (Models.PERDQN, dict(td_batch=64.0, **T), r"td_batch must be an int in \[1, 2048\]"),
])
def test_device_learner_states_td_batchs_conditions_before_touching_a_gpu(make, kwargs, says, monkeypatch):
    import torch
    from reinlife_amd.learn import DeviceLearner
    brain = make()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(brain, "cuda:0", **kwargs)


def _brains():
    return [Models.DQN(max_epi=60), Models.PERDQN()]


DEVT = dict(learn="device", learn_td_priority=True)
TAKES = (r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and, with learn_td_priority=True, "
         r"'PERDQN' \(rl_learn_td_wide\), and at least one of them, got")


@pytest.mark.parametrize("kwargs, says", [
    # without learn_td_priority=True the key stays unknown, with the text the other unknown keys get
    (dict(learn="device", learn_batch={"PERDQN": 96}),
     r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them, got \{'PERDQN': 96\}$"),
    (dict(learn_td_priority=True, learn_batch={"PERDQN": 96}), "learn_td_priority=True needs learn='device'"),
    (dict(learn_batch={}, **DEVT), TAKES),
    (dict(learn_batch={"PERDQN": 96, "PPO": 64}, **DEVT), TAKES),
    (dict(learn_batch={"PERDQN": 0}, **DEVT), r"learn_batch\['PERDQN'\] must be an int in \[1, 2048\] \(the rows of a PERDQN minibatch, rl_learn_td_wide\)"),
    (dict(learn_batch={"PERDQN": 2049}, **DEVT), r"learn_batch\['PERDQN'\] must be an int in \[1, 2048\]"),
    (dict(learn_batch={"PERDQN": 64.0}, **DEVT), r"learn_batch\['PERDQN'\] must be an int in \[1, 2048\]"),
])
def test_learn_batch_perdqn_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds, "DeviceWorlds", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        Environment(brains=_brains(), n_worlds=2, **kwargs)


def test_the_note_of_the_new_entry_and_the_docstrings_name_it():
    from reinlife_amd import Environment, trainer
    from reinlife_amd.learn import ENTRY
    assert set(Environment._NOTES) == set(ENTRY)
    made, note = Environment._NOTES["rl_learn_td_wide"]
    assert made and "%(wide)d" in note and "whole batch" in note
    for doc in (trainer.__doc__, Environment.learn_now.__doc__):
        assert "rl_learn_td_wide" in doc and '"PERDQN"' in doc
