"""CPU: the host side of wide PERD3QN minibatches -- rl_learn_prioritized_wide / _draw / _supported / _work_bytes are declared, exported
and validate their arguments without a GPU; DeviceLearner(prioritized=True, prioritized_batch=) and Environment(learn_prioritized=True,
learn_batch={"PERD3QN": B}) state their conditions before a device is touched; and the premises of
tests/test_hip_learn_prioritized_wide.py hold on the host: a per-tile advantage mean misses the 1e-5 bar on the priorities, a slot drawn
in three tiles gets one value, and the host model of the draw passes the statistical bound the GPU test holds the device to."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc
import learn_dueling_wide_cases as wc
import learn_perd3qn_cases as pc
import learn_prioritized_wide_cases as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
INVALID, UNSUPPORTED = -1, -4   # RL_E_INVALID, RL_E_UNSUPPORTED
NAMES = ("rl_learn_prioritized_wide", "rl_learn_prioritized_wide_draw", "rl_learn_prioritized_wide_supported", "rl_learn_prioritized_wide_work_bytes")


def test_the_four_symbols_are_declared_exported_and_answer_for_perd3qn_alone():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
    assert "int rl_learn_prioritized_wide(" in hdr and "int rl_learn_prioritized_wide_draw(" in hdr
    assert "int rl_learn_prioritized_wide_supported(int kind);" in hdr
    assert "size_t rl_learn_prioritized_wide_work_bytes(int kind, int batch);" in hdr
    assert "#define RL_LEARN_PRIORITIZED_WIDE_MAX 2048" in hdr and _lib.LEARN_PRIORITIZED_WIDE_MAX == pw.WIDE_MAX == 2048
    assert {n for n, _, _ in _lib.ABI} >= set(NAMES)
    assert [lib.rl_learn_prioritized_wide_supported(k) for k in KINDS] == [0, 0, 1, 0, 0]
    assert lib.rl_learn_prioritized_wide_supported(-1) == 0 and lib.rl_learn_prioritized_wide_supported(9) == 0
    # the older answers are what they were
    assert [lib.rl_learn_prioritized_supported(k) for k in KINDS] == [0, 0, 1, 0, 0]
    assert [lib.rl_learn_dueling_wide_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    from reinlife_amd.learn import ENTRY_BY_METHOD, entry_of
    assert ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"} and entry_of(_lib.PERD3QN) is None


def test_work_bytes_are_rl_learn_dueling_wides():
    lib = _lib.lib()
    for batch in (1, 64, 65, 2048):
        got = lib.rl_learn_prioritized_wide_work_bytes(_lib.PERD3QN, batch)
        assert got == wc.work_bytes(batch) == lib.rl_learn_dueling_wide_work_bytes(_lib.D3QN, batch), (batch, got)
    for batch in (0, 2049, -1):
        assert lib.rl_learn_prioritized_wide_work_bytes(_lib.PERD3QN, batch) == 0
        err = lib.rl_last_error()
        assert err.startswith(b"rl_learn_prioritized_wide_work_bytes:") and b"batch" in err and b"[1,2048]" in err, (batch, err)
    for kind in (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERDQN, 7):
        assert lib.rl_learn_prioritized_wide_work_bytes(kind, 64) == 0
        err = lib.rl_last_error()
        assert ("kind %d" % kind).encode() in err and b"RL_PERD3QN" in err, (kind, err)


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, batch=130, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.PERD3QN, p, p, p, p, p, p, 1e-3, 0.99, 0.9, 0.999, 1e-8, batch, 0, 0, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    ps = (_lib.Prio * n)(*[_lib.Prio(p, p, p, p, p, 0.6) for _ in range(n)])
    work = (C.c_void_p * n)(*[0x1000] * n)
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls, rs, ps, work


SLOTS = C.c_void_p(0x1000)


def _learn(h, ls, rs, ps, n, n_steps, work, slots=SLOTS):
    lib = _lib.lib()
    return lib.rl_learn_prioritized_wide(h, ls, rs, ps, n, n_steps, slots, work, None), lib.rl_last_error()


def _draw(h, ls, rs, ps, n, n_steps, work=None, slots=SLOTS):
    lib = _lib.lib()
    return lib.rl_learn_prioritized_wide_draw(h, ls, rs, ps, n, n_steps, slots, None), lib.rl_last_error()


@pytest.mark.parametrize("call, who", [(_learn, b"rl_learn_prioritized_wide:"), (_draw, b"rl_learn_prioritized_wide_draw:")])
def test_both_entry_points_validate_on_the_host_and_name_the_argument(call, who):
    h = _handle()
    ls, rs, ps, work = _args()
    rc, err = call(None, ls, rs, ps, 1, 1, work)
    assert rc == INVALID and err.startswith(who) and b"null handle" in err
    rc, err = call(h, None, rs, ps, 1, 1, work)
    assert rc == INVALID and err.startswith(who) and b"learners" in err
    rc, err = call(h, ls, None, ps, 1, 1, work)
    assert rc == INVALID and err.startswith(who) and b"rings" in err
    rc, err = call(h, ls, rs, None, 1, 1, work)
    assert rc == INVALID and err.startswith(who) and b"prios" in err
    rc, err = call(h, ls, rs, ps, 1, 1, work, slots=None)
    assert rc == INVALID and err.startswith(who) and b"slots must not be null" in err
    if call is _learn:
        assert b"drawn by rl_learn_prioritized_wide_draw" in err
        rc, err = call(h, ls, rs, ps, 1, 1, None)
        assert rc == INVALID and b"rl_learn_prioritized_wide: null work" in err
        l2, r2, p2, w2 = _args(2)
        w2[1] = None
        rc, err = call(h, l2, r2, p2, 2, 1, w2)
        assert rc == INVALID and err.startswith(who) and b"work[1]" in err and b"null" in err
    rc, err = call(h, ls, rs, ps, 1, 0, work)
    assert rc == INVALID and b"n_steps" in err
    rc, err = call(h, ls, rs, ps, 0, 1, work)
    assert rc == INVALID and b"n_learners" in err
    for batch in (0, 2049, -1):
        ls, rs, ps, work = _args(batch=batch)
        rc, err = call(h, ls, rs, ps, 1, 1, work)
        assert rc == INVALID and err.startswith(who) and b"batch" in err and b"[1,2048]" in err, batch
    for batch in (1, 65, 2048):                                                  # the limits themselves pass the batch check
        ls, rs, ps, work = _args(batch=batch)
        rs[0].count = None
        rc, err = call(h, ls, rs, ps, 1, 1, work)
        assert rc == INVALID and b"replay 0" in err, batch
    ls, rs, ps, work = _args(3, batch=130)
    ls[1].batch = 64
    rc, err = call(h, ls, rs, ps, 3, 1, work)
    assert rc == INVALID and err.startswith(who) and b"learner 1" in err and b"batch 64 differs" in err and b"130" in err
    for kind in (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERDQN, 7):
        ls, rs, ps, work = _args(kind=kind)
        rc, err = call(h, ls, rs, ps, 1, 1, work)
        assert rc == UNSUPPORTED and err.startswith(who) and ("kind %d" % kind).encode() in err and b"RL_PERD3QN" in err, kind
    for alpha in (0.0, -0.5, float("nan")):
        ls, rs, ps, work = _args()
        ps[0].alpha = alpha
        rc, err = call(h, ls, rs, ps, 1, 1, work)
        assert rc == INVALID and err.startswith(who) and b"alpha must be > 0" in err, alpha
    for field in ("priority", "prio_max", "seen"):
        ls, rs, ps, work = _args(2)
        setattr(ps[1], field, None)
        rc, err = call(h, ls, rs, ps, 2, 1, work)
        assert rc == INVALID and err.startswith(who) and b"prio 1" in err and b"null" in err, field
    _lib.lib().rl_destroy(h)


def test_the_narrow_entry_points_keep_their_limit_and_messages():
    lib, h = _lib.lib(), _handle()
    ls, rs, ps, _ = _args(batch=65)
    assert lib.rl_learn_prioritized(h, ls, rs, ps, 1, 1, SLOTS, None) == INVALID
    assert b"rl_learn_prioritized: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    assert lib.rl_learn_prioritized_draw(h, ls, rs, ps, 1, 1, SLOTS, None) == INVALID
    assert b"rl_learn_prioritized_draw: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    ls, rs, ps, _ = _args(batch=64)
    assert lib.rl_learn_prioritized(h, ls, rs, ps, 1, 1, None, None) == INVALID
    assert lib.rl_last_error() == (b"rl_learn_prioritized: slots must not be null -- the minibatches of a prioritised memory are drawn by "
                                   b"rl_learn_prioritized_draw")
    ls, rs, ps, _ = _args(batch=64, kind=_lib.D3QN)
    assert lib.rl_learn_prioritized(h, ls, rs, ps, 1, 1, SLOTS, None) == UNSUPPORTED
    assert lib.rl_last_error().endswith(b"this entry point trains RL_PERD3QN (2) only (rl_learn_prioritized_supported)")
    ls, rs, ps, _ = _args(2, batch=64)                                           # unequal batches stay allowed there
    ls[0].batch = 32
    rs[1].count = None
    assert lib.rl_learn_prioritized_draw(h, ls, rs, ps, 2, 1, SLOTS, None) == INVALID and b"replay 1" in lib.rl_last_error()
    lib.rl_destroy(h)


P = dict(prioritized=True)


@pytest.mark.parametrize("make, kwargs, says", [
    (Models.PERD3QN, dict(prioritized_batch=128), r"prioritized_batch is for PERD3QN brains with prioritized=True \(rl_learn_prioritized_wide\); got a PERD3QN brain .* without prioritized=True"),
    (Models.D3QN, dict(prioritized_batch=128, **P), r"prioritized_batch is for PERD3QN brains .* got a D3QN brain"),
    (Models.DQN, dict(prioritized_batch=128, **P), r"prioritized_batch is for PERD3QN brains .* got a DQN brain"),
    (Models.PERDQN, dict(prioritized_batch=128, **P), r"prioritized_batch is for PERD3QN brains .* got a PERDQN brain"),
    (Models.PERD3QN, dict(prioritized_batch=128, wide_batch=64, **P), r"prioritized_batch is for PERD3QN brains .* with wide_batch"),
    (Models.PERD3QN, dict(prioritized_batch=128, dueling_batch=64, **P), r"prioritized_batch is for PERD3QN brains .* with dueling_batch"),
    (Models.PERD3QN, dict(prioritized_batch=128, rollout=True, **P), r"prioritized_batch is for PERD3QN brains .* with rollout=True"),
    (Models.PERD3QN, dict(prioritized_batch=128, td_priority=True, **P), r"prioritized_batch is for PERD3QN brains .* with td_priority=True"),
    (Models.PERD3QN, dict(prioritized_batch=0, **P), r"prioritized_batch must be an int in \[1, 2048\]"),
    (Models.PERD3QN, dict(prioritized_batch=2049, **P), r"prioritized_batch must be an int in \[1, 2048\]"),
    (Models.PERD3QN, dict(prioritized_batch=64.0, **P), r"prioritized_batch must be an int in \[1, 2048\]"),
    (Models.PERD3QN, dict(prioritized_batch=True, **P), r"prioritized_batch must be an int in \[1, 2048\]"),
    # what these always raised
    (Models.PERD3QN, dict(dueling_batch=128), r"dueling_batch is for D3QN brains \(rl_learn_dueling_wide\); got a PERD3QN brain \(kind 2\)$"),
    (Models.PERD3QN, dict(dueling_batch=128, **P), r"dueling_batch is for D3QN brains \(rl_learn_dueling_wide\); got a PERD3QN brain \(kind 2\) with prioritized=True$"),
    (Models.D3QN, dict(**P), r"prioritized=True is for PERD3QN brains \(rl_learn_prioritized\); got a D3QN brain"),
])
def test_device_learner_states_prioritized_batchs_conditions_before_touching_a_gpu(make, kwargs, says, monkeypatch):
    import torch
    from reinlife_amd.learn import DeviceLearner
    brain = make()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(brain, "cuda:0", **kwargs)


@pytest.mark.parametrize("batch", [1, 64, np.int64(130), 2048])
def test_device_learner_accepts_prioritized_batch_and_reaches_the_device(batch, monkeypatch):
    """The accepted spellings pass every check: the first thing DeviceLearner does on the device is torch.as_tensor of the parameters."""
    import torch
    from reinlife_amd.learn import DeviceLearner

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    brain = Models.PERD3QN()
    monkeypatch.setattr(torch, "as_tensor", stop)
    with pytest.raises(Reached):
        DeviceLearner(brain, "cuda:0", prioritized=True, prioritized_batch=batch)


def _brains(which):
    return {"perd3qn": [Models.PERD3QN(), Models.PERD3QN()], "d3qn": [Models.D3QN(), Models.D3QN()],
            "mixed": [Models.DQN(max_epi=60), Models.D3QN(), Models.PERD3QN()]}[which]


DEVP = dict(learn="device", learn_prioritized=True)
BOTH = ("DQN", "D3QN")
TAKES3 = (r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and, with learn_prioritized=True, "
          r"'PERD3QN' \(rl_learn_prioritized_wide\)")


@pytest.mark.parametrize("brains, kwargs, says", [
    # without learn_prioritized=True the key stays unknown, with today's text
    ("perd3qn", dict(learn="device", learn_batch={"PERD3QN": 128}),
     r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them, got"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"PERD3QN": 128}),
     r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them, got"),
    ("d3qn", dict(learn_prioritized=True, learn="device", learn_batch={"PERD3QN": 128}), "learn_prioritized=True needs at least one Models.PERD3QN"),
    ("perd3qn", dict(learn_prioritized=True, learn_batch={"PERD3QN": 128}), "learn_prioritized=True needs learn='device'"),
    # with it, the message names all three keys
    ("perd3qn", dict(learn_batch={}, **DEVP), TAKES3),
    ("perd3qn", dict(learn_batch={"PERD3QN": 128, "PPO": 32}, **DEVP), TAKES3),
    ("perd3qn", dict(learn_batch={"PERDQN": 128}, **DEVP), TAKES3),
    ("perd3qn", dict(learn_batch={"PERD3QN": 0}, **DEVP), r"learn_batch\['PERD3QN'\] must be an int in \[1, 2048\]"),
    ("perd3qn", dict(learn_batch={"PERD3QN": 2049}, **DEVP), r"learn_batch\['PERD3QN'\] must be an int in \[1, 2048\]"),
    ("perd3qn", dict(learn_batch={"PERD3QN": 128.0}, **DEVP), r"learn_batch\['PERD3QN'\] must be an int in \[1, 2048\]"),
    ("perd3qn", dict(learn_batch={"PERD3QN": True}, **DEVP), r"learn_batch\['PERD3QN'\] must be an int in \[1, 2048\] \(the rows of a PERD3QN minibatch, rl_learn_prioritized_wide\)"),
    ("perd3qn", dict(learn_batch={"PERD3QN": 128, "D3QN": 128}, learn_kinds=BOTH, **DEVP), "learn_batch names D3QN"),
    # an int keeps its meaning (DQN)
    ("perd3qn", dict(learn_batch=128, **DEVP), "learn_batch needs at least one Models.DQN brain"),
])
def test_learn_batch_perd3qn_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    with pytest.raises(ValueError, match=says):
        Environment(brains=_brains(brains), n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("brains, kwargs", [
    ("perd3qn", dict(learn_batch={"PERD3QN": 1}, **DEVP)),
    ("perd3qn", dict(learn_batch={"PERD3QN": 2048}, **DEVP)),
    ("perd3qn", dict(learn_batch={"PERD3QN": np.int64(130)}, learn_ranks="average", **DEVP)),
    ("mixed", dict(learn_batch={"PERD3QN": 130}, **DEVP)),
    ("mixed", dict(learn_batch={"PERD3QN": 130, "D3QN": 96, "DQN": 64}, learn_kinds=BOTH, **DEVP)),
    ("mixed", dict(learn_batch={"PERD3QN": 130}, learn_kinds=BOTH, learn_draw="rank", **DEVP)),
    ("mixed", dict(learn_batch=96, **DEVP)),
])
def test_learn_batch_perd3qn_passes_its_checks_where_a_learner_can_use_it(brains, kwargs, monkeypatch):
    """The accepted combinations get as far as the device: the first thing Environment builds there."""
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    with pytest.raises(Reached):
        trainer(_brains(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_trainer_and_environment_gain_no_keyword_and_say_what_runs():
    import reinlife_amd
    for f in (reinlife_amd.trainer, reinlife_amd.Environment.__init__):
        assert list(inspect.signature(f).parameters)[-2:] == ["learn_batch", "learn_draw"]
    from reinlife_amd.learn import DeviceLearner
    assert "prioritized_batch" in inspect.signature(DeviceLearner.__init__).parameters
    assert inspect.signature(DeviceLearner.__init__).parameters["prioritized_batch"].default is None
    doc = reinlife_amd.trainer.__doc__
    assert "rl_learn_prioritized_wide" in doc and '{"PERD3QN": 64}' in doc
    assert "rl_learn_prioritized_wide" in reinlife_amd.Environment.learn_now.__doc__


# ---- the premises of the GPU tests, on the host ----

def test_a_per_tile_mean_misses_the_bar_on_the_priorities_of_a_130_row_batch():
    """float64, batch 130 (tiles of 64, 64 and 2 rows): priorities taken with each tile's OWN advantage means differ from the batch-wide
    ones by far more than the GPU test's 1e-5 of the batch's largest |q|, |q'| -- so that test tells the two apart."""
    g = dc.golden()
    slots, p64, q, qn = pw.case(130)
    scale = max(np.abs(q).max(), np.abs(qn).max())
    tiled = pw.per_tile_priorities(g["init"], g["target_init"], g, slots)
    err = np.abs(tiled - p64) / scale
    print("batch 130: per-tile mean against the batch-wide mean: worst |priority error| / scale %.3g (bar %g), by tile %s"
          % (err.max(), pw.BAR, ["%.3g" % err[t:t + 64].max() for t in (0, 64, 128)]))
    assert tiled.shape == p64.shape == (130,)
    assert err.max() > 100 * pw.BAR
    whole = pc.priorities(g["init"], g["target_init"], g, slots)[0]
    assert np.array_equal(whole, p64)                                             # (the reference is left unchanged)


def test_a_slot_drawn_in_three_tiles_gets_one_value():
    g = dc.golden()
    slots = pw.duplicate_across_tiles()
    at = np.flatnonzero(slots == 17)
    assert at.tolist() == [3, 70, 129] and sorted({int(i) // 64 for i in at}) == [0, 1, 2]
    p64, q, qn = pc.priorities(g["init"], g["target_init"], g, slots)
    scale = max(np.abs(q).max(), np.abs(qn).max())
    tiled = pw.per_tile_priorities(g["init"], g["target_init"], g, slots)
    one, three = np.ptp(p64[at]) / scale, np.ptp(tiled[at]) / scale
    print("slot 17 at 3 / 70 / 129: spread / scale with the batch-wide mean %.3g (float64's own rounding), with per-tile means %.3g" % (one, three))
    assert one <= 1e-12                                                           # one value, up to the host matrix product's last bits
    assert three > 100 * pw.BAR                                                   # (position leaks in where the mean is the tile's)
    s2, m = pw.second_tile_repeats_the_first(), pw.mirrored_tile()
    assert s2.shape == (128,) and np.array_equal(s2[:64], s2[64:]) and m.shape == (64,) and np.array_equal(m, m[::-1])


def test_the_host_model_of_the_draw_passes_the_bound_at_the_wide_draw_count():
    """The seed, rows and priorities of the GPU test's 2048 x 3 draws on the host model (pc.host_draw): every row with a weight within
    5 binomial standard deviations of its expectation, no zero-priority row drawn -- the reference alone passes the bound."""
    g = dc.golden()
    n = pw.DRAW_BATCH * pw.DRAW_STEPS
    pri = pw.draw_priorities()
    keys = pc.content_keys(g, pw.DRAW_ROWS)
    rows = pc.host_draw(keys, pri, pw.DRAW_SEED, 0, 0, n)
    counts = np.bincount(rows, minlength=pw.DRAW_ROWS)
    want, sd = pw.draw_bound(n)
    z = np.abs(counts - want)[pri > 0] / sd[pri > 0]
    print("host model, %d draws over %d rows: worst deviation %.2f sd (bound %d)" % (n, pw.DRAW_ROWS, z.max(), pw.DRAW_SD))
    assert counts.sum() == n and not counts[pri == 0].any() and (z <= pw.DRAW_SD).all()
    assert want[3] - want[1] > 10 * (sd[1] + sd[3])                               # (the case tells a uniform draw apart)
