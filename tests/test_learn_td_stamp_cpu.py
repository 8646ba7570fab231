"""No GPU: rl_learn_td_stamp's declaration, export and prototype, every validation case through the library without a device, the
learn_td_stamp keyword's conditions and messages before a device is touched, where Environment.learn_now queues the stamp, and the
premise of tests/test_hip_learn_td_stamp.py -- on the fixture the TD-error priorities of the 96 rows differ from p_new and from each other
by far more than any tolerance, so a stamp that did nothing or wrote a constant cannot pass there."""
import ctypes as C
import importlib.util
import inspect
import os
import re

import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc
import learn_perdqn_cases as tc

ROOT = dc.ROOT
INVALID, UNSUPPORTED = -1, -4
NAME = "rl_learn_td_stamp"


def test_error_codes_are_the_headers():
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert re.search(r"RL_E_INVALID\s*=\s*-1\b", hdr) and re.search(r"RL_E_UNSUPPORTED\s*=\s*-4\b", hdr)


# ---- the C ABI ----
def test_the_symbol_is_declared_exported_and_listed():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert ("int rl_learn_td_stamp(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, "
            "void* stream);") in flat
    assert "#define RL_LEARN_TD_STAMP_LAUNCHES 2" in hdr and _lib.LEARN_TD_STAMP_LAUNCHES == 2
    comment = flat[:flat.index("#define RL_LEARN_TD_STAMP_LAUNCHES")].rsplit("/*", 1)[1]
    assert comment.startswith(" THIS BUILD'S OWN") and "PERDQN.py:113-128" in comment and "BIT FOR BIT" in comment
    assert "global: rl_*;" in open(os.path.join(ROOT, "reinlife_amd", "csrc", "exports.map")).read()
    abi = {n: (res, args) for n, res, args in _lib.ABI}
    assert hasattr(lib, NAME) and NAME in abi
    assert abi[NAME][0] is C.c_int and len(abi[NAME][1]) == 6 and abi[NAME][1][4] is C.c_int
    assert abi[NAME][1][1:4] == [C.POINTER(_lib.Learner), C.POINTER(_lib.Replay), C.POINTER(_lib.TdPrio)]
    # the draws and the update are listed as they were, and the learner table gains no row: the stamp is a step of the draw
    assert len(abi["rl_learn_td_draw"][1]) == 8 and len(abi["rl_learn_td_draw_rank"][1]) == 12 and len(abi["rl_learn_td"][1]) == 8
    from reinlife_amd import learn
    assert len(learn.ENTRIES) == 8 and not any("stamp" in e.name for e in learn.ENTRIES)
    assert list(inspect.signature(learn.DeviceLearner.__init__).parameters)[-2:] == ["wide_batch", "dueling_batch"]


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


class _Args:
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced).  What
    the stamp does not read is null or out of range already: adam_m / adam_v / state / packed, batch, min_size, age, keys, beta, p_new."""

    def __init__(self, n=1):
        p = C.c_void_p(0x1000)
        self.n = n
        self.ls = (_lib.Learner * n)(*[_lib.Learner(_lib.PERDQN, p, p, None, None, None, None, 0.001, 0.99, 0.9, 0.999, 1e-8, 0, -7, 0, None, None) for _ in range(n)])
        self.rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, None, p, 96) for _ in range(n)])
        self.sides = (_lib.TdPrio * n)(*[_lib.TdPrio(p, None, p, None, float("nan"), 0.01, 0.6, 0.001, None) for _ in range(n)])

    def call(self, h):
        lib = _lib.lib()
        return lib.rl_learn_td_stamp(h, self.ls, self.rs, self.sides, self.n, None), lib.rl_last_error()


def test_the_dummy_arguments_are_laid_out_as_the_structs_are():
    """(the positional constructors above against the fields' names: a moved field would make the cases below test something else)"""
    a = _Args()
    assert a.ls[0].kind == _lib.PERDQN and a.ls[0].params == 0x1000 and a.ls[0].target == 0x1000 and a.ls[0].adam_m is None and a.ls[0].batch == 0
    assert a.rs[0].capacity == 96 and a.rs[0].count == 0x1000 and a.rs[0].age is None and a.rs[0].done == 0x1000
    assert a.sides[0].priority == 0x1000 and a.sides[0].keys is None and a.sides[0].seen == 0x1000 and a.sides[0].beta is None
    assert abs(a.sides[0].prio_a - 0.6) < 1e-6 and abs(a.sides[0].prio_e - 0.01) < 1e-6


def test_every_bad_argument_is_named():
    """Nothing is launched: every address here is a dummy, and this test runs without a GPU."""
    lib, h = _lib.lib(), _handle()
    who = NAME.encode()
    got, err = _Args().call(None)
    assert got == INVALID and err.startswith(who + b":") and b"null handle" in err
    for field, word in (("ls", b"learners"), ("rs", b"rings"), ("sides", b"tds")):
        a = _Args()
        setattr(a, field, None)
        got, err = a.call(h)
        assert got == INVALID and err.startswith(who + b":") and word in err and b"null" in err, (field, err)
    for n in (0, 17, -1):
        a = _Args(17)
        a.n = n
        got, err = a.call(h)
        assert got == INVALID and err.startswith(who + b":") and b"n_learners" in err and b"[1,16]" in err, n
    for kind in (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERD3QN):
        a = _Args(2)
        a.ls[1].kind = kind
        got, err = a.call(h)
        assert got == UNSUPPORTED and err.startswith(who + b":") and b"learner 1" in err and b"kind %d" % kind in err, (kind, err)
    for field in ("params", "target"):
        a = _Args(2)
        setattr(a.ls[1], field, None)
        got, err = a.call(h)
        assert got == INVALID and b"learner 1" in err and field.encode() in err and b"null" in err, (field, err)
    for field in ("state", "state_prime", "action", "reward", "done", "count"):
        a = _Args(2)
        setattr(a.rs[1], field, None)
        got, err = a.call(h)
        assert got == INVALID and b"replay 1" in err and b" %s must" % field.encode() in err, (field, err)
    for capacity in (0, -5):
        a = _Args()
        a.rs[0].capacity = capacity
        got, err = a.call(h)
        assert got == INVALID and b"replay 0" in err and b"capacity" in err, capacity
    for field in ("priority", "seen"):
        a = _Args(2)
        setattr(a.sides[1], field, None)
        got, err = a.call(h)
        assert got == INVALID and b"td 1" in err and field.encode() in err and b"null" in err, (field, err)
    for prio_a in (0.0, -0.6, float("nan")):
        a = _Args()
        a.sides[0].prio_a = prio_a
        got, err = a.call(h)
        assert got == INVALID and b"td 0" in err and b"prio_a" in err, prio_a
    lib.rl_destroy(h)


# ---- trainer(learn_td_stamp=...) / Environment(learn_td_stamp=...) ----
def _made(which):
    return {"dqn": lambda: [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "perdqn": lambda: [Models.PERDQN(), Models.DQN(max_epi=60)],
            "all": lambda: [Models.DQN(max_epi=60), Models.D3QN(), Models.PERD3QN(), Models.PERDQN()]}[which]()


MUST = r"learn_td_stamp must be None .* or 'error' .*rl_learn_td_stamp"
NEEDS = r"learn_td_stamp='error' needs learn_td_priority=True"


@pytest.mark.parametrize("brains, kwargs, says", [
    ("perdqn", dict(learn="device", learn_td_priority=True, learn_td_stamp=True), MUST),
    ("perdqn", dict(learn="device", learn_td_priority=True, learn_td_stamp="td"), MUST),
    ("perdqn", dict(learn="device", learn_td_priority=True, learn_td_stamp=1), MUST),
    ("perdqn", dict(learn="device", learn_td_priority=True, learn_td_stamp=["error"]), MUST),
    ("perdqn", dict(learn="device", learn_td_stamp="error"), NEEDS),
    ("perdqn", dict(learn_td_stamp="error"), NEEDS),
    ("all", dict(learn="device", learn_prioritized=True, learn_td_stamp="error"), NEEDS),
    ("perdqn", dict(learn_td_priority=True, learn_td_stamp="error"), r"learn_td_priority=True needs learn='device'"),   # (learn_td_priority's own complaints, as they were)
    ("dqn", dict(learn="device", learn_td_priority=True, learn_td_stamp="error"), r"learn_td_priority=True needs at least one Models.PERDQN brain"),
    ("perdqn", dict(learn="device", learn_td_priority="error"), r"learn_td_priority must be None or True"),
])
def test_the_keyword_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    made = _made(brains)
    with pytest.raises(ValueError, match=says):
        trainer(made, n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    with pytest.raises(ValueError, match=says):
        Environment(brains=made, n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("brains, kwargs", [
    ("perdqn", dict(learn_td_priority=True, learn_td_stamp="error")),
    ("perdqn", dict(learn_td_priority=True, learn_td_stamp="error", learn_draw={"PERDQN": "rank"})),
    ("all", dict(learn_kinds=("DQN", "D3QN"), learn_prioritized=True, learn_td_priority=True, learn_td_stamp="error")),
    ("perdqn", dict(learn_td_priority=True, learn_td_stamp=None)),
])
def test_the_keyword_passes_its_checks_with_learn_td_priority(brains, kwargs, monkeypatch):
    """The accepted combinations get as far as the device: the first thing Environment builds there."""
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    with pytest.raises(Reached):
        trainer(_made(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, learn="device", **kwargs)


def test_the_keyword_sits_with_learn_td_priority_and_defaults_to_none():
    import reinlife_amd
    for f in (reinlife_amd.trainer, reinlife_amd.Environment.__init__):
        params = inspect.signature(f).parameters
        p = params["learn_td_stamp"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
        names = list(params)
        assert names.index("learn_td_stamp") == names.index("learn_td_priority") + 1
    assert "learn_td_stamp" in reinlife_amd.trainer.__doc__ and "AS OF THE LEARNING CALL" in reinlife_amd.trainer.__doc__


def _recording_worlds():
    spec = importlib.util.spec_from_file_location("record_learner_layer", os.path.join(ROOT, "tools", "record_learner_layer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    class Worlds(tool.RecordingWorlds):
        draw_td_rank = tool.RecordingWorlds._draw("draw_td_rank")

        def stamp_td(self, learners):
            self._note("stamp_td", learners, None)
    return Worlds


def test_learn_now_queues_one_stamp_in_front_of_the_perdqn_draw_and_only_with_the_key():
    """Environment.learn_now over stand-in worlds: with the key one stamp_td directly in front of the PERDQN draw, the race draw and the
    rank draw alike, and every other call as it is without the key; without it the log of calls is what it was."""
    from reinlife_amd import Environment
    from reinlife_amd.World import environment as envmod
    every = dict(learn="device", learn_kinds=("DQN", "D3QN"), learn_prioritized=True, learn_rollout=True, learn_td_priority=True)
    logs = {}
    for stamp in (None, "error"):
        for draw in (None, {"PERDQN": "rank"}):
            mp = pytest.MonkeyPatch()
            mp.setattr(envmod, "DeviceWorlds", _recording_worlds())
            try:
                env = Environment(brains=_made("all") + [Models.PPO()], n_worlds=4, rng="philox", learn_draw=draw, learn_td_stamp=stamp, **every)
            finally:
                mp.undo()
            env.learn_now()
            env.learn_now(40)
            assert env.learn_td_stamp == stamp
            logs[stamp, draw is not None] = env.worlds.log
            note = env._weights_note()
            assert ("rl_learn_td_stamp" in note) == (stamp == "error") and "rl_learn_td" in note
            assert ("as of the learning call" in note) == (stamp == "error")
    for ranked in (False, True):
        plain, stamped = logs[None, ranked], logs["error", ranked]
        names = [r[0] for r in stamped]
        assert not any(r[0] == "stamp_td" for r in plain) and names.count("stamp_td") == 2
        for i, r in enumerate(stamped):
            if r[0] == "stamp_td":
                assert r[1] == ["rl_learn_td"] and stamped[i + 1][0] == ("draw_td_rank" if ranked else "draw_td") and stamped[i + 2][0] == "learn"
                assert stamped[i + 2][1] == ["rl_learn_td"]
        assert [r for r in stamped if r[0] != "stamp_td"] == plain


def test_the_signature_the_ranks_compare_grows_only_with_the_key(monkeypatch):
    from reinlife_amd import Environment, distributed
    from reinlife_amd.World import environment as envmod
    sigs = []
    monkeypatch.setattr(distributed, "check_learner_signature", lambda sig, dist, device=None: sigs.append(list(sig)))
    monkeypatch.setattr(distributed, "broadcast_from_rank0", lambda flat, dist: None)
    monkeypatch.setattr(envmod, "DeviceWorlds", _recording_worlds())
    for stamp in (None, "error"):
        env = Environment(brains=_made("perdqn"), n_worlds=4, rng="philox", learn="device", learn_td_priority=True, learn_td_stamp=stamp)
        env.dist = object()
        env._align_learners()
    assert len(sigs) == 2 and sigs[1][:-1] == sigs[0] and sigs[1][-1] == 1


# ---- the premise of the GPU tests ----
def test_the_fixtures_td_error_priorities_are_spread_and_none_is_p_new():
    import torch
    g, p = dc.golden(), tc.golden()
    gamma = float(p["gamma"])
    pred, target = tc.pred_target(tc.net_of(p["init"]), tc.net_of(p["target_init"]), g, np.arange(96), gamma, torch.float64)
    err = np.abs((pred - target).detach().numpy())
    pri = (err + float(p["prio_e"])) ** float(p["prio_a"])
    p_new = float(p["p_new"])
    order = np.sort(pri)
    print("float64 TD-error priorities of the 96 fixture rows: min %.6g, median %.6g, max %.6g (max / min %.4g); p_new %.8g; "
          "closest to p_new: %.3g away; smallest gap between two rows' priorities, relative: %.3g"
          % (pri.min(), np.median(pri), pri.max(), pri.max() / pri.min(), p_new, np.abs(pri - p_new).min(), (np.diff(order) / order[1:]).min()))
    assert pri.shape == (96,) and np.isfinite(pri).all()
    assert (pri.astype(np.float32) != np.float32(p_new)).all()   # a stamp that did nothing leaves p_new where the tests put it
    assert pri.max() / pri.min() > 10                            # no constant is close to all of them
    done = g["ring_done"][:96].astype(bool)
    assert done.any() and not done.all()
    assert np.array_equal(target.numpy()[done], g["ring_reward"][:96].astype(np.float64)[done])   # done: target == reward
