"""CPU: the host side of wide DQN minibatches -- rl_learn_wide / rl_learn_wide_supported / rl_learn_wide_work_bytes are declared, exported
and validate their arguments without a GPU; DeviceLearner(wide_batch=) and Environment(learn_batch=) state their conditions before a
device is touched; trainer() forwards the keyword."""
import ctypes as C
import inspect
import os
import sys

import pytest

from reinlife_amd import Models, _lib, trainer

import learn_cases as lc
import learn_wide_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
INVALID = -1   # RL_E_INVALID


def test_the_three_symbols_are_declared_exported_and_answer_for_dqn_alone():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    for name in ("rl_learn_wide", "rl_learn_wide_supported", "rl_learn_wide_work_bytes"):
        assert hasattr(lib, name), name
    assert "int rl_learn_wide(" in hdr and "int rl_learn_wide_supported(int kind);" in hdr and "size_t rl_learn_wide_work_bytes(int kind, int batch);" in hdr
    assert "#define RL_LEARN_WIDE_MAX 2048" in hdr and "DQN.py:80-83, 142-153" in hdr and _lib.LEARN_WIDE_MAX == wc.WIDE_MAX == 2048
    assert [lib.rl_learn_wide_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]
    assert lib.rl_learn_wide_supported(-1) == 0 and lib.rl_learn_wide_supported(9) == 0
    assert [lib.rl_learn_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]            # (rl_learn's contract is what it was)
    from reinlife_amd.learn import ENTRY_BY_METHOD, entry_of
    assert ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"} and entry_of(_lib.DQN) == "rl_learn"
    src = open(os.path.join(ROOT, "reinlife_amd", "build.py")).read()
    assert '"rl_learn_wide.hip"' in src and os.path.exists(os.path.join(ROOT, "reinlife_amd", "csrc", "rl_learn_wide.hip"))


def test_work_bytes_grow_by_one_parameter_row_per_started_tile():
    lib = _lib.lib()
    assert lc.N_PARAMS == lib.rl_policy_n_params(_lib.DQN) == 28488
    got = {b: lib.rl_learn_wide_work_bytes(_lib.DQN, b) for b in (1, 32, 33, 64, 2048)}
    print(got)
    for b, n in got.items():
        assert n == wc.work_bytes(b) and n % 16 == 0, (b, n)
    row = lc.N_PARAMS * 4
    assert got[1] == got[32] and got[33] == got[64]                                  # a started tile counts whole
    assert row <= got[33] - got[32] <= row + 16 and row <= got[1] - wc.HEADER_BYTES <= row + 16
    assert 62 * row <= got[2048] - got[64] <= 62 * row + 62 * 4 + 16
    for batch in (0, 2049, -1):
        assert lib.rl_learn_wide_work_bytes(_lib.DQN, batch) == 0
        err = lib.rl_last_error()
        assert err.startswith(b"rl_learn_wide_work_bytes:") and b"batch" in err and b"[1,2048]" in err, (batch, err)
    for kind in (_lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        assert lib.rl_learn_wide_work_bytes(kind, 64) == 0
        assert ("kind %d" % kind).encode() in lib.rl_last_error(), kind


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, batch=96, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.DQN, p, p, p, p, p, p, 0.0005, 0.98, 0.9, 0.999, 1e-8, batch, 1000, 1, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    work = (C.c_void_p * n)(*[0x1000] * n)
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls, rs, work


def _call(h, ls, rs, n, n_steps, work):
    lib = _lib.lib()
    return lib.rl_learn_wide(h, ls, rs, n, n_steps, None, work, None), lib.rl_last_error()


@pytest.mark.parametrize("field", ["params", "target", "adam_m", "adam_v", "state", "packed"])
def test_rl_learn_wide_rejects_null_learner_pointers(field):
    h = _handle()
    ls, rs, work = _args(2, **{field: None})
    rc, err = _call(h, ls, rs, 2, 1, work)
    assert rc == INVALID and err.startswith(b"rl_learn_wide:") and b"learner 1" in err and b"null" in err
    _lib.lib().rl_destroy(h)


def test_rl_learn_wide_rejects_bad_counts_kinds_batches_rings_and_work():
    lib, h = _lib.lib(), _handle()
    ls, rs, work = _args()
    rc, err = _call(None, ls, rs, 1, 1, work)
    assert rc == INVALID and b"rl_learn_wide: null handle" in err
    rc, err = _call(h, None, rs, 1, 1, work)
    assert rc == INVALID and b"null learners" in err
    rc, err = _call(h, ls, None, 1, 1, work)
    assert rc == INVALID and b"rings" in err
    rc, err = _call(h, ls, rs, 1, 1, None)
    assert rc == INVALID and b"rl_learn_wide: null work" in err
    rc, err = _call(h, ls, rs, 1, 0, work)
    assert rc == INVALID and b"n_steps" in err
    rc, err = _call(h, ls, rs, 0, 1, work)
    assert rc == INVALID and b"n_learners" in err
    l17, r17, w17 = _args(17)
    rc, err = _call(h, l17, r17, 17, 1, w17)
    assert rc == INVALID and b"n_learners" in err and b"16" in err
    for kind in (_lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        ls, rs, work = _args(kind=kind)
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == INVALID and ("kind %d" % kind).encode() in err and err.startswith(b"rl_learn_wide:"), kind
    for batch in (0, 2049, -1):
        ls, rs, work = _args(batch=batch)
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == INVALID and b"batch" in err and b"[1,2048]" in err, batch
    for batch in (1, 33, 2048):                                                  # the limits themselves pass the batch check
        ls, rs, work = _args(batch=batch)
        rs[0].count = None
        rc, err = _call(h, ls, rs, 1, 1, work)
        assert rc == INVALID and b"replay 0" in err, batch
    ls, rs, work = _args(3, batch=96)
    ls[1].batch = 64
    rc, err = _call(h, ls, rs, 3, 1, work)
    assert rc == INVALID and b"learner 1" in err and b"batch 64 differs" in err and b"96" in err
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
    # rl_learn's own limit and message are what they were
    ls, rs, _ = _args(batch=33)
    assert lib.rl_learn(h, ls, rs, 1, 1, None, None) == INVALID and b"rl_learn: learner 0: batch must be in [1,32] (got 33)" in lib.rl_last_error()
    lib.rl_destroy(h)


@pytest.mark.parametrize("make, kwargs, says", [
    (Models.D3QN, dict(wide_batch=64), r"wide_batch is for DQN brains \(rl_learn_wide\); got a D3QN brain"),
    (Models.PPO, dict(wide_batch=64), r"wide_batch is for DQN brains \(rl_learn_wide\); got a PPO brain"),
    (Models.PERD3QN, dict(wide_batch=64, prioritized=True), r"wide_batch is for DQN brains .* with prioritized=True"),
    (Models.DQN, dict(wide_batch=64, prioritized=True), r"wide_batch is for DQN brains .* with prioritized=True"),
    (Models.DQN, dict(wide_batch=64, rollout=True), r"wide_batch is for DQN brains .* with rollout=True"),
    (Models.DQN, dict(wide_batch=64, td_priority=True), r"wide_batch is for DQN brains .* with td_priority=True"),
    (Models.DQN, dict(wide_batch=0), r"wide_batch must be an int in \[1, 2048\]"),
    (Models.DQN, dict(wide_batch=2049), r"wide_batch must be an int in \[1, 2048\]"),
    (Models.DQN, dict(wide_batch=64.0), r"wide_batch must be an int in \[1, 2048\]"),
    (Models.DQN, dict(wide_batch=True), r"wide_batch must be an int in \[1, 2048\]"),
])
def test_device_learner_states_wide_batchs_conditions_before_touching_a_gpu(make, kwargs, says, monkeypatch):
    import torch
    from reinlife_amd.learn import DeviceLearner
    brain = make()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(brain, "cuda:0", **kwargs)


@pytest.mark.parametrize("brains, kwargs, says", [
    ("dqn", dict(learn_batch=64), "learn_batch needs learn='device'"),
    ("dqn", dict(learn="device", learn_batch=0), r"learn_batch must be None or an int in \[1, 2048\]"),
    ("dqn", dict(learn="device", learn_batch=2049), r"learn_batch must be None or an int in \[1, 2048\]"),
    ("dqn", dict(learn="device", learn_batch=64.5), r"learn_batch must be None or an int in \[1, 2048\]"),
    ("dqn", dict(learn="device", learn_batch=True), r"learn_batch must be None or an int in \[1, 2048\]"),
    ("d3qn", dict(learn="device", learn_kinds=("D3QN",), learn_batch=64), "learn_batch needs at least one Models.DQN brain"),
    ("d3qn", dict(learn="device", learn_batch=64), "learn_batch needs at least one Models.DQN brain"),
    ("mixed", dict(learn="device", learn_kinds=("D3QN",), learn_batch=64), "learn_batch needs at least one Models.DQN brain among the learning kinds"),
])
def test_learn_batch_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    made = {"dqn": [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "d3qn": [Models.D3QN(), Models.D3QN()], "mixed": [Models.DQN(max_epi=60), Models.D3QN()]}[brains]
    with pytest.raises(ValueError, match=says):
        trainer(made, n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_trainer_accepts_and_forwards_learn_batch(monkeypatch):
    import reinlife_amd
    trainer_module = sys.modules["reinlife_amd.Helpers.trainer"]   # (the package attribute of that name is the function)
    for f in (reinlife_amd.trainer, reinlife_amd.Environment.__init__):
        p = inspect.signature(f).parameters["learn_batch"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    seen = {}

    class Stop(Exception):
        pass

    def fake(**kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(trainer_module, "Environment", fake)
    with pytest.raises(Stop):
        trainer([Models.DQN(max_epi=60)], n_episodes=5, learn="device", learn_batch=96, save=False, print_results=False)
    assert seen["learn_batch"] == 96 and seen["learn"] == "device"
    seen.clear()
    with pytest.raises(Stop):
        trainer([Models.DQN(max_epi=60)], n_episodes=5, save=False, print_results=False)
    assert seen["learn_batch"] is None
