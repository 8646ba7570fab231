"""CPU: the host side of wide D3QN minibatches -- rl_learn_dueling_wide / _supported / _work_bytes are declared, exported and validate
their arguments without a GPU; DeviceLearner(dueling_batch=) and Environment(learn_batch={...}) state their conditions before a device is
touched; and the premises of tests/test_hip_learn_dueling_wide.py hold on the host: torch float32 stays inside the 1e-5 bar at the tested
batches, a per-tile advantage mean does not, and the host model of the tiled computation is float64 autograd."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc
import learn_dueling_wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
INVALID, UNSUPPORTED = -1, -4   # RL_E_INVALID, RL_E_UNSUPPORTED


def test_the_three_symbols_are_declared_exported_and_answer_for_d3qn_alone():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    for name in ("rl_learn_dueling_wide", "rl_learn_dueling_wide_supported", "rl_learn_dueling_wide_work_bytes"):
        assert hasattr(lib, name), name
    assert "int rl_learn_dueling_wide(" in hdr and "int rl_learn_dueling_wide_supported(int kind);" in hdr
    assert "size_t rl_learn_dueling_wide_work_bytes(int kind, int batch);" in hdr
    assert "#define RL_LEARN_DUELING_WIDE_MAX 2048" in hdr and _lib.LEARN_DUELING_WIDE_MAX == wc.WIDE_MAX == 2048
    assert "3 n_steps + 3 launches" in hdr and "2 n_steps + 3 launches" in hdr       # this entry point's count, and rl_learn_wide's as it was
    assert [lib.rl_learn_dueling_wide_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert lib.rl_learn_dueling_wide_supported(-1) == 0 and lib.rl_learn_dueling_wide_supported(9) == 0
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]     # (rl_learn_dueling's contract is what it was)
    assert [lib.rl_learn_wide_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]
    from reinlife_amd.learn import ENTRY_BY_METHOD, entry_of
    assert ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"} and entry_of(_lib.D3QN) == "rl_learn_dueling"
    src = open(os.path.join(ROOT, "reinlife_amd", "build.py")).read()
    assert '"rl_learn_dueling_wide.hip"' in src and os.path.exists(os.path.join(ROOT, "reinlife_amd", "csrc", "rl_learn_dueling_wide.hip"))


def test_work_bytes_grow_by_one_parameter_row_and_one_stash_per_started_tile():
    lib = _lib.lib()
    assert dc.N_PARAMS == lib.rl_policy_n_params(_lib.D3QN) == 53897
    got = {b: lib.rl_learn_dueling_wide_work_bytes(_lib.D3QN, b) for b in (1, 64, 65, 128, 130, 2048)}
    print(got)
    for b, n in got.items():
        assert n == wc.work_bytes(b), (b, n)
    tile = dc.N_PARAMS * 4 + wc.TILE * wc.STASH_FLOATS * 4
    assert got[1] == got[64] and got[65] == got[128] and got[130] > got[128]         # a started tile counts whole
    assert tile <= got[65] - got[64] <= tile + 16 and tile <= got[1] - wc.HEADER_BYTES <= tile + 16
    assert 30 * tile <= got[2048] - got[128] <= 30 * tile + 30 * 8 + 16
    for batch in (0, 2049, -1):
        assert lib.rl_learn_dueling_wide_work_bytes(_lib.D3QN, batch) == 0
        err = lib.rl_last_error()
        assert err.startswith(b"rl_learn_dueling_wide_work_bytes:") and b"batch" in err and b"[1,2048]" in err, (batch, err)
    for kind in (_lib.DQN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        assert lib.rl_learn_dueling_wide_work_bytes(kind, 64) == 0
        assert ("kind %d" % kind).encode() in lib.rl_last_error(), kind


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, batch=130, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.D3QN, p, p, p, p, p, p, 1e-3, 0.99, 0.9, 0.999, 1e-8, batch, 63, 0, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    work = (C.c_void_p * n)(*[0x1000] * n)
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls, rs, work


def _call(h, ls, rs, n, n_steps, work):
    lib = _lib.lib()
    return lib.rl_learn_dueling_wide(h, ls, rs, n, n_steps, None, work, None), lib.rl_last_error()


@pytest.mark.parametrize("field", ["params", "target", "adam_m", "adam_v", "state", "packed"])
def test_rl_learn_dueling_wide_rejects_null_learner_pointers(field):
    h = _handle()
    ls, rs, work = _args(2, **{field: None})
    rc, err = _call(h, ls, rs, 2, 1, work)
    assert rc == INVALID and err.startswith(b"rl_learn_dueling_wide:") and b"learner 1" in err and b"null" in err
    _lib.lib().rl_destroy(h)


def test_rl_learn_dueling_wide_rejects_bad_counts_kinds_batches_rings_and_work():
    lib, h = _lib.lib(), _handle()
    ls, rs, work = _args()
    rc, err = _call(None, ls, rs, 1, 1, work)
    assert rc == INVALID and b"rl_learn_dueling_wide: null handle" in err
    rc, err = _call(h, None, rs, 1, 1, work)
    assert rc == INVALID and b"null learners" in err
    rc, err = _call(h, ls, None, 1, 1, work)
    assert rc == INVALID and b"rings" in err
    rc, err = _call(h, ls, rs, 1, 1, None)
    assert rc == INVALID and b"rl_learn_dueling_wide: null work" in err
    rc, err = _call(h, ls, rs, 1, 0, work)
    assert rc == INVALID and b"n_steps" in err
    rc, err = _call(h, ls, rs, 0, 1, work)
    assert rc == INVALID and b"n_learners" in err
    l17, r17, w17 = _args(17)
    rc, err = _call(h, l17, r17, 17, 1, w17)
    assert rc == INVALID and b"n_learners" in err and b"16" in err
    for kind in (_lib.DQN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        ls, rs, work = _args(kind=kind)
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == UNSUPPORTED and ("kind %d" % kind).encode() in err and err.startswith(b"rl_learn_dueling_wide:") and b"RL_D3QN" in err, kind
    for batch in (0, 2049, -1):
        ls, rs, work = _args(batch=batch)
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == INVALID and b"batch" in err and b"[1,2048]" in err, batch
    for batch in (1, 65, 2048):                                                  # the limits themselves pass the batch check
        ls, rs, work = _args(batch=batch)
        rs[0].count = None
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == INVALID and b"replay 0" in err, batch
    ls, rs, work = _args(3, batch=130)
    ls[1].batch = 64
    rc, err = _call(h, ls, rs, 3, 1, work)
    assert rc == INVALID and b"learner 1" in err and b"batch 64 differs" in err and b"130" in err
    ls, rs, work = _args()
    rs[0].reward = None
    rc, err = _call(h, ls, rs, 1, 1, work)
    assert rc == INVALID and b"replay 0" in err
    ls, rs, work = _args()
    rs[0].capacity = 0
    rc, err = _call(h, ls, rs, 1, 1, work)
    assert rc == INVALID and b"replay 0" in err
    ls, rs, work = _args(2)
    work[1] = None
    rc, err = _call(h, ls, rs, 2, 1, work)
    assert rc == INVALID and b"work[1]" in err and b"null" in err
    # rl_learn_dueling's own limit and message are what they were
    ls, rs, _ = _args(batch=65)
    assert lib.rl_learn_dueling(h, ls, rs, 1, 1, None, None) == INVALID
    assert b"rl_learn_dueling: learner 0: batch must be in [1,64] (got 65)" in lib.rl_last_error()
    lib.rl_destroy(h)


@pytest.mark.parametrize("make, kwargs, says", [
    (Models.DQN, dict(dueling_batch=128), r"dueling_batch is for D3QN brains \(rl_learn_dueling_wide\); got a DQN brain"),
    (Models.PPO, dict(dueling_batch=128), r"dueling_batch is for D3QN brains \(rl_learn_dueling_wide\); got a PPO brain"),
    (Models.PERD3QN, dict(dueling_batch=128), r"dueling_batch is for D3QN brains \(rl_learn_dueling_wide\); got a PERD3QN brain"),
    (Models.PERD3QN, dict(dueling_batch=128, prioritized=True), r"dueling_batch is for D3QN brains .* with prioritized=True"),
    (Models.D3QN, dict(dueling_batch=128, wide_batch=64), r"dueling_batch is for D3QN brains .* with wide_batch"),
    (Models.D3QN, dict(dueling_batch=128, prioritized=True), r"dueling_batch is for D3QN brains .* with prioritized=True"),
    (Models.D3QN, dict(dueling_batch=128, rollout=True), r"dueling_batch is for D3QN brains .* with rollout=True"),
    (Models.D3QN, dict(dueling_batch=128, td_priority=True), r"dueling_batch is for D3QN brains .* with td_priority=True"),
    (Models.D3QN, dict(dueling_batch=0), r"dueling_batch must be an int in \[1, 2048\]"),
    (Models.D3QN, dict(dueling_batch=2049), r"dueling_batch must be an int in \[1, 2048\]"),
    (Models.D3QN, dict(dueling_batch=64.0), r"dueling_batch must be an int in \[1, 2048\]"),
    (Models.D3QN, dict(dueling_batch=True), r"dueling_batch must be an int in \[1, 2048\]"),
    (Models.D3QN, dict(wide_batch=64), r"wide_batch is for DQN brains \(rl_learn_wide\); got a D3QN brain"),   # (what it always raised)
])
def test_device_learner_states_dueling_batchs_conditions_before_touching_a_gpu(make, kwargs, says, monkeypatch):
    import torch
    from reinlife_amd.learn import DeviceLearner
    brain = make()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(brain, "cuda:0", **kwargs)


def _brains(which):
    return {"dqn": [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "d3qn": [Models.D3QN(), Models.D3QN()],
            "mixed": [Models.DQN(max_epi=60), Models.D3QN()], "perd3qn": [Models.PERD3QN(), Models.PERD3QN()]}[which]


BOTH = ("DQN", "D3QN")


@pytest.mark.parametrize("brains, kwargs, says", [
    ("d3qn", dict(learn_batch={"D3QN": 128}), "learn_batch needs learn='device'"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={}), "learn_batch as a dict takes the keys 'DQN' .* and 'D3QN'"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"PERD3QN": 128}), "learn_batch as a dict takes the keys"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": 128, "PPO": 32}), "learn_batch as a dict takes the keys"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": 0}), r"learn_batch\['D3QN'\] must be an int in \[1, 2048\]"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": 2049}), r"learn_batch\['D3QN'\] must be an int in \[1, 2048\]"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": 128.0}), r"learn_batch\['D3QN'\] must be an int in \[1, 2048\]"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": True}), r"learn_batch\['D3QN'\] must be an int in \[1, 2048\]"),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"DQN": 64.5, "D3QN": 128}), r"learn_batch\['DQN'\] must be an int in \[1, 2048\]"),
    ("d3qn", dict(learn="device", learn_batch={"D3QN": 128}), "learn_batch names D3QN: it needs at least one Models.D3QN brain among the learning kinds"),
    ("mixed", dict(learn="device", learn_batch={"D3QN": 128}), "learn_batch names D3QN"),                      # learn_kinds is ("DQN",)
    ("dqn", dict(learn="device", learn_kinds=BOTH, learn_batch={"D3QN": 128}), "learn_batch names D3QN"),      # no such brain
    ("d3qn", dict(learn="device", learn_kinds=BOTH, learn_batch={"DQN": 64, "D3QN": 128}), "learn_batch names DQN"),
    ("perd3qn", dict(learn="device", learn_prioritized=True, learn_kinds=BOTH, learn_batch={"D3QN": 128}), "learn_batch names D3QN"),
    # an int keeps today's meaning and today's messages
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch=64), "learn_batch needs at least one Models.DQN brain"),
    ("dqn", dict(learn="device", learn_batch=2049), r"learn_batch must be None or an int in \[1, 2048\] \(the rows of a DQN minibatch, rl_learn_wide\)"),
])
def test_learn_batch_by_kind_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    with pytest.raises(ValueError, match=says):
        Environment(brains=_brains(brains), n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("brains, kwargs", [
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch={"D3QN": 1})),
    ("d3qn", dict(learn="device", learn_kinds="D3QN", learn_batch={"D3QN": 2048})),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"D3QN": np.int64(130)})),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"DQN": 96})),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"DQN": 96, "D3QN": 130})),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"D3QN": 130}, learn_draw="rank")),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"D3QN": 130}, learn_ranks="average")),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch={"D3QN": 130}, learn_steps={"DQN": 5, "D3QN": 2})),
    ("mixed", dict(learn="device", learn_kinds=BOTH, learn_batch=96)),
])
def test_learn_batch_by_kind_passes_its_checks_where_a_learner_can_use_it(brains, kwargs, monkeypatch):
    """The accepted combinations get as far as the device: the first thing Environment builds there."""
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    with pytest.raises(Reached):
        trainer(_brains(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_signatures_gain_no_keyword():
    import reinlife_amd
    for f in (reinlife_amd.trainer, reinlife_amd.Environment.__init__):
        assert list(inspect.signature(f).parameters)[-2:] == ["learn_batch", "learn_draw"]
    from reinlife_amd.learn import DeviceLearner
    assert list(inspect.signature(DeviceLearner.__init__).parameters)[-2:] == ["wide_batch", "dueling_batch"]
    doc = reinlife_amd.trainer.__doc__
    assert "rl_learn_dueling_wide" in doc and '{"D3QN": 64}' in doc


# ---- the premises of the GPU tests, on the host ----

@pytest.mark.parametrize("batch", [65, 128, 130, 2048])
def test_torch_float32_autograd_stays_inside_the_bar_at_the_tested_batches(batch):
    """What float32 itself makes of these minibatches: torch float32 autograd against float64, every tensor within 1e-5 of its largest
    magnitude with room to spare (measured 3e-7 .. 6e-7) -- the bar of the GPU test is not tighter than the number format allows."""
    import torch
    g = dc.golden()
    slots, loss64, g64 = wc.case(batch)
    loss32, g32 = dc.grads64(g["init"], g["target_init"], g, slots, wc.GAMMA, dtype=torch.float32)
    worst, per = wc.worst_relative_error(g32, g64)
    print("batch %d: torch float32 against float64: worst error / max|g| %.3g; loss %.3g" % (batch, worst, abs(loss32 - loss64) / abs(loss64)))
    assert worst <= 1e-5 and abs(loss32 - loss64) <= 1e-5 * abs(loss64)


@pytest.mark.parametrize("batch", wc.MULTI_TILE_BATCHES)
def test_the_tiled_model_is_float64_autograd_and_a_per_tile_mean_is_not(batch):
    """The algebra of the kernels -- per-tile advantage sums, M' and M over the tiles, G over the tiles, dL/dadv = g_i [a = a_i] -
    G / (8 batch), the tiles' partial gradients added -- is the float64 autograd gradient of the reference's loss; the same tiles each
    with its OWN mean miss the GPU test's 1e-5 bar by at least a hundredfold on some tensor (other tensors move only ~3e-7: the
    assertion is on the maximum over tensors)."""
    g = dc.golden()
    slots, loss64, g64 = wc.case(batch)
    assert wc.tiles(batch) > 1 and len(slots) == batch and len(set(slots.tolist())) < batch
    loss, grads = wc.tiled_model(g["init"], g["target_init"], g, slots)
    worst, per = wc.worst_relative_error(grads, g64)
    print("batch %d: tiled model against autograd: worst error / max|g| %.3g, loss %.3g" % (batch, worst, abs(loss - loss64) / abs(loss64)))
    assert worst <= 1e-12 and abs(loss - loss64) <= 1e-12 * abs(loss64)
    for a, b in zip(grads, g64):
        assert not a[b == 0].any()
    loss_t, grads_t = wc.tiled_model(g["init"], g["target_init"], g, slots, per_tile_mean=True)
    worst_t, per_t = wc.worst_relative_error(grads_t, g64)
    print("batch %d: per-tile mean against autograd: per tensor %s; worst %.3g" % (batch, " ".join("%.2g" % e for e in per_t), worst_t))
    assert worst_t >= 1e-3


def test_one_tile_of_the_model_is_the_untiled_update():
    g = dc.golden()
    slots = g["slots"][0]
    loss64, g64 = dc.grads64(g["init"], g["target_init"], g, slots, wc.GAMMA)
    for per_tile in (False, True):
        loss, grads = wc.tiled_model(g["init"], g["target_init"], g, slots, per_tile_mean=per_tile)
        assert wc.worst_relative_error(grads, g64)[0] <= 1e-12 and abs(loss - loss64) <= 1e-12 * abs(loss64)
