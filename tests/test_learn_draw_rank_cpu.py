"""CPU: the host side of the rank draw -- rl_learn_draw_rank / rl_learn_draw_rank_work_bytes are declared, exported and validate their
arguments without a GPU; Environment(learn_draw=) states its conditions before a device is touched; trainer() forwards the keyword; and
the draw's rule itself, restated on the host (learn_rank_cases), is uniform over the rows."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_cases as lc
import learn_perd3qn_cases as pc
import learn_rank_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1   # RL_E_INVALID


def test_both_symbols_are_declared_exported_and_listed():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "size_t rl_learn_draw_rank_work_bytes(long long capacity);" in hdr and "int rl_learn_draw_rank(rl_world* h," in hdr
    assert "#define RL_LEARN_DRAW_RANK_LAUNCHES 6" in hdr and _lib.LEARN_DRAW_RANK_LAUNCHES == rc.RANK_LAUNCHES == 6
    abi = {n: (res, args) for n, res, args in _lib.ABI}
    for name in ("rl_learn_draw_rank", "rl_learn_draw_rank_work_bytes"):
        assert hasattr(lib, name) and name in abi, name
    assert abi["rl_learn_draw_rank_work_bytes"] == (C.c_size_t, [C.c_longlong]) and len(abi["rl_learn_draw_rank"][1]) == 10
    src = open(os.path.join(ROOT, "reinlife_amd", "build.py")).read()
    assert '"rl_learn_rank.hip"' in src and os.path.exists(os.path.join(ROOT, "reinlife_amd", "csrc", "rl_learn_rank.hip"))
    # the contracts beside it are what they were
    kinds = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
    assert [lib.rl_learn_supported(k) for k in kinds] == [1, 0, 0, 0, 0] and [lib.rl_learn_wide_supported(k) for k in kinds] == [1, 0, 0, 0, 0]
    assert [lib.rl_learn_dueling_supported(k) for k in kinds] == [0, 1, 0, 0, 0]


def test_work_bytes_are_positive_monotone_and_multiples_of_16():
    lib = _lib.lib()
    caps = (1, 2, 3, 4, 5, 48, 1025, 10_000, 50_000, 2 ** 31 - 1)
    got = [lib.rl_learn_draw_rank_work_bytes(c) for c in caps]
    print(dict(zip(caps, got)))
    for c, n in zip(caps, got):
        assert n > 0 and n % 16 == 0 and n == rc.work_bytes(c) and n >= rc.TABLE_BYTES + 4 * c, (c, n)
    assert all(a <= b for a, b in zip(got, got[1:])) and got[0] < got[-1]
    for c in (0, -1, 2 ** 31):
        assert lib.rl_learn_draw_rank_work_bytes(c) == 0
        err = lib.rl_last_error()
        assert err.startswith(b"rl_learn_draw_rank_work_bytes:") and b"capacity" in err, (c, err)


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


class _Args:
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""

    def __init__(self, n=1, batch=96):
        p = C.c_void_p(0x1000)
        self.n, self.n_steps = n, 1
        self.ls = (_lib.Learner * n)(*[_lib.Learner(_lib.DQN, p, p, p, p, p, p, 0.0005, 0.98, 0.9, 0.999, 1e-8, batch, 1000, 1, None, None) for _ in range(n)])
        self.rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
        self.keys, self.order, self.work = ((C.c_void_p * n)(*[0x1000] * n) for _ in range(3))
        self.slots = p

    def call(self, h):
        lib = _lib.lib()
        return lib.rl_learn_draw_rank(h, self.ls, self.rs, self.n, self.n_steps, self.keys, self.order, self.work, self.slots, None), lib.rl_last_error()


def test_rl_learn_draw_rank_names_every_bad_argument():
    lib, h = _lib.lib(), _handle()
    rc_, err = _Args().call(None)
    assert rc_ == INVALID and err == b"rl_learn_draw_rank: null handle"
    for field, word in (("ls", b"learners"), ("rs", b"rings"), ("keys", b"keys"), ("order", b"order"), ("work", b"work"), ("slots", b"slots")):
        a = _Args()
        setattr(a, field, None)
        rc_, err = a.call(h)
        assert rc_ == INVALID and err == b"rl_learn_draw_rank: null " + word, (field, err)
    for field, says in (("keys", b"keys[1]"), ("order", b"order[1]"), ("work", b"work[1]")):
        a = _Args(2)
        getattr(a, field)[1] = None
        rc_, err = a.call(h)
        assert rc_ == INVALID and err.startswith(b"rl_learn_draw_rank:") and says in err and b"null" in err, (field, err)
    a = _Args(2)
    a.ls[1].state = None
    rc_, err = a.call(h)
    assert rc_ == INVALID and b"learner 1" in err and b"state" in err and b"null" in err
    for n in (0, 17, -1):
        a = _Args(17)
        a.n = n
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"n_learners" in err and b"[1,16]" in err, n
    for n_steps in (0, -3):
        a = _Args()
        a.n_steps = n_steps
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"n_steps" in err, n_steps
    for batch in (0, 2049, -1):
        a = _Args(2)
        a.ls[1].batch = batch
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"learner 1" in err and b"batch" in err and b"[1,2048]" in err, batch
    for field in ("state", "state_prime", "action", "reward", "done", "age", "count"):
        a = _Args(2)
        setattr(a.rs[1], field, None)
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"replay 1" in err and field.encode() in err, field
    for capacity in (0, -5, 2 ** 31):
        a = _Args()
        a.rs[0].capacity = capacity
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"replay 0" in err and b"capacity" in err, capacity
    for batch in (1, 33, 2048):            # the limits themselves pass the batch check (and so do different batches in one call)
        a = _Args(2, batch=batch)
        a.ls[0].batch = 7
        a.rs[1].count = None
        rc_, err = a.call(h)
        assert rc_ == INVALID and b"replay 1" in err, batch
    a = _Args(16, batch=2048)
    a.n_steps = 2 ** 16                    # 2^16 x 16 x 2048 = 2^31 draws: one more than an int32 index holds
    rc_, err = a.call(h)
    assert rc_ == INVALID and b"n_steps" in err and b"2^31" in err
    # rl_learn_draw's own limit and message are what they were
    a = _Args(batch=33)
    assert lib.rl_learn_draw(h, a.ls, a.rs, 1, 1, a.keys, a.slots, None) == INVALID
    assert b"rl_learn_draw: learner 0: batch must be in [1,32] (got 33)" in lib.rl_last_error()
    lib.rl_destroy(h)


@pytest.mark.parametrize("brains, kwargs, says", [
    ("dqn", dict(learn="device", learn_draw="sorted"), r"learn_draw must be None \(rl_learn_draw\) or 'rank'"),
    ("dqn", dict(learn="device", learn_draw=True), r"learn_draw must be None \(rl_learn_draw\) or 'rank'"),
    ("dqn", dict(learn_draw="key"), r"learn_draw must be None \(rl_learn_draw\) or 'rank'"),
    ("dqn", dict(learn_draw="rank"), "learn_draw='rank' needs learn='device'"),
    ("d3qn", dict(learn="device", learn_draw="rank"), "learn_draw='rank' needs at least one brain that rl_learn, rl_learn_wide or rl_learn_dueling trains"),
    ("dqn", dict(learn="device", learn_kinds=("D3QN",), learn_draw="rank"), "learn_draw='rank' needs at least one brain"),
    ("perd3qn", dict(learn="device", learn_prioritized=True, learn_draw="rank"), "learn_draw='rank' needs at least one brain"),
    ("ppo", dict(learn="device", learn_rollout=True, learn_draw="rank"), "learn_draw='rank' needs at least one brain"),
])
def test_learn_draw_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    made = {"dqn": [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "d3qn": [Models.D3QN(), Models.D3QN()],
            "perd3qn": [Models.PERD3QN(), Models.PERD3QN()], "ppo": [Models.PPO(), Models.PPO()]}[brains]
    with pytest.raises(ValueError, match=says):
        trainer(made, n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    from reinlife_amd import Environment
    with pytest.raises(ValueError, match=says):
        Environment(brains=made, n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("brains, kwargs", [
    ("dqn", dict(learn="device", learn_draw="rank")),
    ("dqn", dict(learn="device", learn_draw="rank", learn_batch=96)),
    ("mixed", dict(learn="device", learn_draw="rank", learn_kinds=("D3QN",))),
    ("mixed", dict(learn="device", learn_draw="rank", learn_kinds=("DQN", "D3QN"))),
])
def test_learn_draw_passes_its_checks_where_a_learner_can_use_it(brains, kwargs, monkeypatch):
    """The accepted combinations get as far as the device: the first thing Environment builds there."""
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    made = {"dqn": [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "mixed": [Models.DQN(max_epi=60), Models.D3QN()]}[brains]
    with pytest.raises(Reached):
        trainer(made, n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_trainer_accepts_and_forwards_learn_draw(monkeypatch):
    import reinlife_amd
    trainer_module = sys.modules["reinlife_amd.Helpers.trainer"]   # (the package attribute of that name is the function)
    for f in (reinlife_amd.trainer, reinlife_amd.Environment.__init__):
        params = inspect.signature(f).parameters
        p = params["learn_draw"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
        assert list(params)[-2:] == ["learn_batch", "learn_draw"]                 # behind the existing keywords
    seen = {}

    class Stop(Exception):
        pass

    def fake(**kw):
        seen.update(kw)
        raise Stop()
    monkeypatch.setattr(trainer_module, "Environment", fake)
    with pytest.raises(Stop):
        trainer([Models.DQN(max_epi=60)], n_episodes=5, learn="device", learn_draw="rank", save=False, print_results=False)
    assert seen["learn_draw"] == "rank" and seen["learn"] == "device"
    seen.clear()
    with pytest.raises(Stop):
        trainer([Models.DQN(max_epi=60)], n_episodes=5, save=False, print_results=False)
    assert seen["learn_draw"] is None


def test_the_host_rule_is_a_permutation_lookup_and_handles_ties_and_empty_rings():
    keys = np.array([5, 3, 5, 1, 3, 2 ** 64 - 1, 0], np.uint64)
    assert rc.host_order(keys).tolist() == [6, 3, 1, 4, 0, 2, 5]                  # equal keys: the lower slot first
    assert rc.host_order(np.full(9, 7, np.uint64)).tolist() == list(range(9))
    assert rc.host_rank_draw(keys[:0], 11, 0, 0, 5).tolist() == [0] * 5
    assert rc.host_rank_draw(keys[:1], 11, 3, 2, 5).tolist() == [0] * 5
    x = rc.philox_words(11, 2, 7, 64)
    want = rc.host_order(keys)[((x.astype(object) * 7) // 2 ** 32).astype(np.int64)]   # the multiply-shift in Python integers
    assert np.array_equal(rc.host_rank_draw(keys, 11, 2, 7, 64), want)
    from reinlife_amd.learn import philox_slots
    assert np.array_equal(((x * np.uint64(7)) >> np.uint64(32)).astype(np.int32), philox_slots(11, 2, 7, 2, 32, 7).reshape(-1))   # rl_learn's own mapping


def test_the_host_rule_is_uniform_over_48_rows():
    """6,400 draws (200 steps of batch 32) over the fixture ring's 48 rows: every row's count within 5 standard deviations of 6400 / 48
    = 133.3 (sigma = sqrt(6400 * (1 / 48) * (47 / 48)) = 11.4, so 76 .. 190).  A condition on the rule, checked on the host: the multiply-shift of a
    Philox word is uniform whatever the keys are, and the order is a permutation."""
    g = lc.golden()
    keys = pc.content_keys(g, 48)
    assert len(set(keys.tolist())) == 48
    rows = rc.host_rank_draw(keys, 11, 0, 0, 6400)
    counts = np.bincount(rows, minlength=48)
    sigma = np.sqrt(6400 * (1 / 48) * (47 / 48))
    print("counts min %d max %d (mean 133.3, sigma %.2f: %.2f .. %.2f sigma)" % (counts.min(), counts.max(), sigma, (counts.min() - 6400 / 48) / sigma,
                                                                                  (counts.max() - 6400 / 48) / sigma))
    assert counts.sum() == 6400 and len(counts) == 48
    assert (np.abs(counts - 6400 / 48) <= 5 * sigma).all()
