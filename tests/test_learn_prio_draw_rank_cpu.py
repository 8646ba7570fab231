"""CPU: the host side of the prioritised rank draws -- the numpy restatement the GPU test compares with (learn_prio_rank_cases) checked on
its own; rl_learn_prioritized_draw_rank / rl_learn_td_draw_rank / rl_learn_prio_draw_rank_work_bytes declared, exported, listed and
validating their arguments without a GPU; Environment(learn_draw={...}) stating its conditions before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from reinlife_amd import Models, _lib, trainer

import learn_cases as lc
import learn_perd3qn_cases as pc
import learn_prio_rank_cases as prc
import learn_rank_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -4


# ---- the host restatement ----
def test_the_cumulative_sum_is_the_segment_rule_and_close_to_the_exact_sum():
    """Sizes around the segment length: cum equals a plain Python restatement of the formula (float64 adds in the stated order), is
    nondecreasing, repeats its value at zero, negative and NaN weights, and differs from the exact rational sum by a few ulps."""
    from fractions import Fraction
    rng = np.random.RandomState(4)
    for n in (1, 2, 63, 64, 65, 129, 1025):
        w = (rng.random_sample(n) ** 3 * 4).astype(np.float32)
        w[::7] = 0.0
        if n > 10:
            w[3], w[5] = np.nan, -1.0
        cum = prc.host_cum(w)
        local, base, want = 0.0, 0.0, []
        for r in range(n):
            if r % 64 == 0:
                base, local = (base + local if r else 0.0), 0.0
            local = local + (float(w[r]) if w[r] > 0 else 0.0)
            want.append(base + local)
        assert cum.dtype == np.float64 and cum.tobytes() == np.array(want, np.float64).tobytes(), n
        assert (np.diff(cum) >= 0).all()
        dead = ~(w > 0)
        assert all(cum[r] == (cum[r - 1] if r else 0.0) for r in np.nonzero(dead)[0])
        exact = sum(Fraction(float(v)) for v in w if v > 0)
        assert abs(Fraction(float(cum[-1])) - exact) <= exact * Fraction(n + 64, 2 ** 52), n
    assert prc.host_cum(np.zeros(0, np.float32)).shape == (0,)


def test_the_pick_agrees_with_brute_force_on_small_cases():
    """Weights that are small integers over 8 (every partial sum exact in float64): the searchsorted pick is the exact rule's, in both
    modes, at the segment borders too."""
    rng = np.random.RandomState(9)
    for n in (1, 5, 64, 65, 130):
        w = (rng.randint(0, 5, n) / 8.0).astype(np.float32)
        w[rng.randint(n)] = 1.0
        cum = prc.host_cum(w)
        total = cum[-1]
        u = np.concatenate([rng.random_sample(200), [0.0, 1 - 2.0 ** -53]])
        for batch, stratified in ((1, False), (7, True), (64, True)):
            t = prc.targets(u, total, batch, stratified)
            got = prc.pick_ranks(cum, t)
            assert np.array_equal(got, prc.brute_force_ranks(w, t)), (n, batch, stratified)
            assert (w[got] > 0).all()
        # every partial sum itself as a target: the NEXT row of positive weight (cum > target is strict)
        got = prc.pick_ranks(cum, cum[:-1])
        assert np.array_equal(got, prc.brute_force_ranks(w, cum[:-1]))


def test_the_clamp_rule_takes_the_last_row_of_positive_weight():
    w = np.zeros(200, np.float32)
    w[[0, 63, 64, 130]] = (1.0, 2.0, 0.5, 3.0)
    cum = prc.host_cum(w)
    total = cum[-1]
    assert total == 6.5
    for t in (total, np.nextafter(total, np.inf), 1e300, np.inf):
        assert prc.pick_ranks(cum, np.array([t])).tolist() == [130]
    assert prc.pick_ranks(cum, np.array([np.nextafter(total, 0)])).tolist() == [130]
    assert prc.pick_ranks(cum, np.array([0.0, 0.999, 1.0, 2.999, 3.0, 3.499, 3.5])).tolist() == [0, 0, 63, 63, 64, 64, 130]
    # one positive weight among zeros: every target, 0 and total included, names it
    for at in (0, 63, 64, 199):
        one = np.zeros(200, np.float32)
        one[at] = 1e-30
        c = prc.host_cum(one)
        assert prc.pick_ranks(c, prc.targets(np.array([0.0, 0.5, 1 - 2.0 ** -53]), c[-1], 1, False)).tolist() == [at] * 3
        assert set(prc.pick_ranks(c, prc.targets(np.linspace(0, 1, 64, endpoint=False), c[-1], 64, True)).tolist()) == {at}
        assert prc.pick_ranks(c, np.array([c[-1]])).tolist() == [at]


def test_uniforms_are_53_bit_fractions_and_a_zero_total_is_the_uniform_rank_rule():
    x, y = prc.philox_words(11, 2, 7, _lib.SITE_LEARN_PRIO, 64)
    u = prc.uniforms(x, y)
    want = [((int(b) << 32 | int(a)) >> 11) / 2.0 ** 53 for a, b in zip(x, y)]
    assert u.tolist() == want and (u >= 0).all() and (u < 1).all() and len(set(u.tolist())) == 64
    a, _ = prc.philox_words(11, 2, 7, _lib.SITE_LEARN_TD, 64)
    assert not np.array_equal(a, x)                                               # the two memories' sites differ
    keys = np.arange(7, dtype=np.uint64)[::-1].copy()
    slots, ranks, order, cum = prc.host_draw(keys, np.zeros(7, np.float32), 11, 2, 7, _lib.SITE_LEARN_PRIO, 2, 32, False)
    assert np.array_equal(ranks, (x * np.uint64(7)) >> np.uint64(32)) and np.array_equal(slots, order[ranks]) and not cum.any()
    inf = np.full(7, np.inf, np.float32)
    assert np.array_equal(prc.host_draw(keys, inf, 11, 2, 7, _lib.SITE_LEARN_PRIO, 2, 32, True)[0], slots)
    assert prc.host_draw(keys[:0], inf[:0], 11, 2, 7, _lib.SITE_LEARN_PRIO, 2, 32, True)[0].tolist() == [0] * 64


def _cycle_case(stratified, n_steps, batch):
    g = lc.golden()
    keys = pc.content_keys(g, 48)
    pri = prc.cycle_priorities(48)
    w32 = (pri.astype(np.float64) ** 0.6).astype(np.float32)
    return (pri, w32) + prc.host_draw(keys, w32, 11, 0, 0, _lib.SITE_LEARN_PRIO, n_steps, batch, stratified)


def test_stratified_draws_stay_inside_their_strata():
    """48 rows with priorities cycling 0, 0.25, 1, 4, batch 64: draw j's row overlaps segment j -- cum[r] > j * seg and cum[r - 1] <=
    (j + 1) * seg -- and a row's count in the batch lies in [floor(B w / sum) - 1, ceil(B w / sum) + 1]."""
    pri, w32, slots, ranks, order, cum = _cycle_case(True, 1, 64)
    seg = cum[-1] / np.float64(64)
    j = np.arange(64, dtype=np.float64)
    before = np.where(ranks == 0, 0.0, cum[np.maximum(ranks - 1, 0)])
    assert (cum[ranks] > j * seg).all() and (before <= (j + 1) * seg).all()
    share = 64 * w32.astype(np.float64) / w32.astype(np.float64).sum()
    counts = np.bincount(slots, minlength=48)
    assert (counts >= np.floor(share) - 1).all() and (counts <= np.ceil(share) + 1).all() and not counts[pri == 0].any()
    assert (np.diff(ranks) >= 0).all()                                            # one uniform per segment: the ranks ascend with j


def test_6400_independent_draws_follow_the_weights():
    """tests/test_hip_learn_perd3qn.py's design on the host rule: 48 rows, priorities cycling 0, 0.25, 1, 4, 100 steps of batch 64; zero
    rows never drawn, every other count within 5 binomial standard deviations of 6400 p_i."""
    pri, w32, slots, ranks, order, cum = _cycle_case(False, 100, 64)
    p = w32.astype(np.float64) / w32.astype(np.float64).sum()
    counts = np.bincount(slots, minlength=48)
    sigma = np.sqrt(6400 * p * (1 - p))
    z = (counts - 6400 * p)[pri > 0] / sigma[pri > 0]
    print("z min %.2f max %.2f" % (z.min(), z.max()))
    assert counts.sum() == 6400 and not counts[pri == 0].any() and (np.abs(z) <= 5).all()


# ---- the C ABI ----
def test_the_symbols_are_declared_exported_and_listed():
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "size_t rl_learn_prio_draw_rank_work_bytes(long long capacity);" in flat
    assert ("int rl_learn_prioritized_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, "
            "int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream);") in flat
    assert ("int rl_learn_td_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps, "
            "int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream);") in flat
    assert "#define RL_LEARN_PRIO_DRAW_RANK_LAUNCHES 8" in hdr and _lib.LEARN_PRIO_DRAW_RANK_LAUNCHES == prc.PRIO_RANK_LAUNCHES == 8
    assert "global: rl_*;" in open(os.path.join(ROOT, "reinlife_amd", "csrc", "exports.map")).read()
    abi = {n: (res, args) for n, res, args in _lib.ABI}
    for name in ("rl_learn_prioritized_draw_rank", "rl_learn_td_draw_rank", "rl_learn_prio_draw_rank_work_bytes"):
        assert hasattr(lib, name) and name in abi, name
    assert abi["rl_learn_prio_draw_rank_work_bytes"] == (C.c_size_t, [C.c_longlong])
    assert len(abi["rl_learn_prioritized_draw_rank"][1]) == len(abi["rl_learn_td_draw_rank"][1]) == 12
    # the uniform rank draw and the race draws are listed as they were
    assert _lib.LEARN_DRAW_RANK_LAUNCHES == 6 and len(abi["rl_learn_draw_rank"][1]) == 10 and len(abi["rl_learn_td_draw"][1]) == 8
    from reinlife_amd import learn
    assert len(learn.ENTRIES) == 8 and not any("draw_rank" in e.name for e in learn.ENTRIES)   # a draw is no learning entry point


def test_work_bytes():
    lib = _lib.lib()
    for c in (1, 63, 64, 65, 10_000, 50_000, 2 ** 31 - 1):
        n = lib.rl_learn_prio_draw_rank_work_bytes(c)
        assert n == prc.work_bytes(c) and n % 16 == 0 and n >= lib.rl_learn_draw_rank_work_bytes(c) + 8 * ((c + 63) // 64), c
    for c in (0, -1, 2 ** 31):
        assert lib.rl_learn_prio_draw_rank_work_bytes(c) == 0
        err = lib.rl_last_error()
        assert err.startswith(b"rl_learn_prio_draw_rank_work_bytes:") and b"capacity" in err, (c, err)


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


class _Args:
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""

    def __init__(self, td, n=1, batch=64):
        p = C.c_void_p(0x1000)
        self.td, self.n, self.n_steps, self.stratified = td, n, 1, 0
        kind = _lib.PERDQN if td else _lib.PERD3QN
        self.ls = (_lib.Learner * n)(*[_lib.Learner(kind, p, p, p, p, p, p, 0.001, 0.99, 0.9, 0.999, 1e-8, batch, 0, 0, None, None) for _ in range(n)])
        self.rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
        if td:
            self.sides = (_lib.TdPrio * n)(*[_lib.TdPrio(p, p, p, p, 0.063, 0.01, 0.6, 0.001, None) for _ in range(n)])
        else:
            self.sides = (_lib.Prio * n)(*[_lib.Prio(p, p, p, p, p, 0.6) for _ in range(n)])
        self.order, self.cum, self.work = ((C.c_void_p * n)(*[0x1000] * n) for _ in range(3))
        self.slots = p
        self.name = "rl_learn_td_draw_rank" if td else "rl_learn_prioritized_draw_rank"

    def call(self, h):
        lib = _lib.lib()
        got = getattr(lib, self.name)(h, self.ls, self.rs, self.sides, self.n, self.n_steps, self.stratified, self.order, self.cum, self.work,
                                      self.slots, None)
        return got, lib.rl_last_error()


@pytest.mark.parametrize("td", [False, True])
def test_every_bad_argument_is_named(td):
    """Nothing is launched: every address here is a dummy, and this test runs without a GPU."""
    lib, h = _lib.lib(), _handle()
    who = _Args(td).name.encode()
    got, err = _Args(td).call(None)
    assert got == INVALID and err.startswith(who + b":") and b"null handle" in err
    for field, word in (("ls", b"learners"), ("rs", b"rings"), ("sides", b"tds" if td else b"prios"), ("order", b"order"), ("cum", b"cum"),
                        ("work", b"work"), ("slots", b"slots")):
        a = _Args(td)
        setattr(a, field, None)
        got, err = a.call(h)
        assert got == INVALID and err.startswith(who + b":") and word in err and b"null" in err, (field, err)
    for field, says in (("order", b"order[1]"), ("cum", b"cum[1]"), ("work", b"work[1]")):
        a = _Args(td, 2)
        getattr(a, field)[1] = None
        got, err = a.call(h)
        assert got == INVALID and err.startswith(who + b":") and says in err and b"null" in err, (field, err)
    for kind in (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERD3QN if td else _lib.PERDQN):
        a = _Args(td, 2)
        a.ls[1].kind = kind
        got, err = a.call(h)
        assert got == UNSUPPORTED and b"learner 1" in err and b"kind %d" % kind in err, (kind, err)
    a = _Args(td, 2)
    a.ls[1].state = None
    got, err = a.call(h)
    assert got == INVALID and b"learner 1" in err and b"state" in err
    for n in (0, 17, -1):
        a = _Args(td, 17)
        a.n = n
        got, err = a.call(h)
        assert got == INVALID and b"n_learners" in err and b"[1,16]" in err, n
    for n_steps in (0, -3):
        a = _Args(td)
        a.n_steps = n_steps
        got, err = a.call(h)
        assert got == INVALID and b"n_steps" in err, n_steps
    limit = 64 if td else 2048
    for batch in (0, limit + 1, -1):
        a = _Args(td, 2)
        a.ls[1].batch = batch
        got, err = a.call(h)
        assert got == INVALID and b"learner 1" in err and b"batch" in err and b"[1,%d]" % limit in err, batch
    for field in ("state", "state_prime", "action", "reward", "done", "age", "count"):
        a = _Args(td, 2)
        setattr(a.rs[1], field, None)
        got, err = a.call(h)
        assert got == INVALID and b"replay 1" in err and field.encode() in err, field
    for capacity in (0, -5, 2 ** 31):
        a = _Args(td)
        a.rs[0].capacity = capacity
        got, err = a.call(h)
        assert got == INVALID and b"replay 0" in err and b"capacity" in err, capacity
    for field in (("priority", "keys", "seen") if td else ("priority", "weight", "keys", "prio_max", "seen")):
        a = _Args(td, 2)
        setattr(a.sides[1], field, None)
        got, err = a.call(h)
        assert got == INVALID and (b"td 1" if td else b"prio 1") in err and field.encode() in err, field
    if not td:
        for alpha in (0.0, -1.0, float("nan")):
            a = _Args(td)
            a.sides[0].alpha = alpha
            got, err = a.call(h)
            assert got == INVALID and b"alpha" in err, alpha
    # the limits pass the batch check, and so do different batches in one call: the next complaint is about something else
    a = _Args(td, 2, batch=limit)
    a.ls[0].batch = 1
    a.rs[1].count = None
    got, err = a.call(h)
    assert got == INVALID and b"replay 1" in err
    lib.rl_destroy(h)


# ---- Environment(learn_draw={...}) ----
def _made(which):
    return {"dqn": lambda: [Models.DQN(max_epi=60), Models.DQN(max_epi=60)], "d3qn": lambda: [Models.D3QN(), Models.D3QN()],
            "perd3qn": lambda: [Models.PERD3QN(), Models.PERD3QN()], "perdqn": lambda: [Models.PERDQN(), Models.PERDQN()],
            "all": lambda: [Models.DQN(max_epi=60), Models.D3QN(), Models.PERD3QN(), Models.PERDQN()]}[which]()


MUST = r"learn_draw must be None \(rl_learn_draw\) or 'rank'"


@pytest.mark.parametrize("brains, kwargs, says", [
    ("dqn", dict(learn="device", learn_draw={}), MUST),
    ("dqn", dict(learn="device", learn_draw={"DQN": "sorted"}), MUST),
    ("dqn", dict(learn="device", learn_draw={"DQN": True}), MUST),
    ("dqn", dict(learn="device", learn_draw={"PPO": "rank"}), MUST),
    ("dqn", dict(learn="device", learn_draw={"DQN": "rank", "A2C": "rank"}), MUST),
    ("dqn", dict(learn="device", learn_draw=["rank"]), MUST),
    ("dqn", dict(learn_draw={"DQN": "rank"}), "needs learn='device'"),
    ("dqn", dict(learn="device", learn_draw={"D3QN": "rank"}), "learn_draw names D3QN: it needs at least one Models.D3QN brain"),
    ("d3qn", dict(learn="device", learn_draw={"D3QN": "rank"}), "learn_draw names D3QN: it needs at least one Models.D3QN brain among the learning kinds"),
    ("all", dict(learn="device", learn_draw={"PERD3QN": "rank"}), "learn_draw names PERD3QN: it needs learn_prioritized=True"),
    ("all", dict(learn="device", learn_prioritized=True, learn_draw={"PERDQN": "rank"}), "learn_draw names PERDQN: it needs learn_td_priority=True"),
    ("all", dict(learn="device", learn_td_priority=True, learn_draw={"PERDQN": "rank", "PERD3QN": "rank"}), "learn_draw names PERD3QN: it needs learn_prioritized=True"),
    ("dqn", dict(learn="device", learn_prioritized=True, learn_draw={"PERD3QN": "rank"}), "PERD3QN"),   # (learn_prioritized's own complaint: no such brain)
])
def test_the_dict_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import Environment, worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    made = _made(brains)
    with pytest.raises(ValueError, match=says):
        trainer(made, n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)
    with pytest.raises(ValueError, match=says):
        Environment(brains=made, n_worlds=4, rng="philox", **kwargs)


@pytest.mark.parametrize("brains, kwargs", [
    ("dqn", dict(learn_draw={"DQN": "rank"})),
    ("all", dict(learn_kinds=("DQN", "D3QN"), learn_draw={"D3QN": "rank"})),
    ("perd3qn", dict(learn_prioritized=True, learn_draw={"PERD3QN": "rank"})),
    ("perd3qn", dict(learn_prioritized=True, learn_batch={"PERD3QN": 96}, learn_draw={"PERD3QN": "rank"})),
    ("perdqn", dict(learn_td_priority=True, learn_draw={"PERDQN": "rank"})),
    ("all", dict(learn_kinds=("DQN", "D3QN"), learn_prioritized=True, learn_td_priority=True,
                 learn_draw={"DQN": "rank", "D3QN": "rank", "PERD3QN": "rank", "PERDQN": "rank"})),
])
def test_the_dict_passes_its_checks_where_its_kinds_have_learners(brains, kwargs, monkeypatch):
    """The accepted combinations get as far as the device: the first thing Environment builds there."""
    from reinlife_amd import worlds

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", stop)
    with pytest.raises(Reached):
        trainer(_made(brains), n_episodes=5, n_worlds=4, save=False, print_results=False, learn="device", **kwargs)


def test_learn_now_picks_the_draw_per_family():
    """Environment.learn_now over stand-in worlds: each family calls the draw its key names, and without a key the draw it always called."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("record_learner_layer", os.path.join(ROOT, "tools", "record_learner_layer.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    class Worlds(tool.RecordingWorlds):
        draw_prioritized_rank, draw_td_rank = tool.RecordingWorlds._draw("draw_prioritized_rank"), tool.RecordingWorlds._draw("draw_td_rank")

    from reinlife_amd import Environment
    from reinlife_amd.World import environment as envmod
    every = dict(learn="device", learn_kinds=("DQN", "D3QN"), learn_prioritized=True, learn_td_priority=True)
    plain = ["draw_slots", "draw_slots", "draw_prioritized", "draw_td"]
    for draw, want in ((None, plain), ("rank", ["draw_slots_rank", "draw_slots_rank", "draw_prioritized", "draw_td"]),
                       ({"PERD3QN": "rank"}, ["draw_slots", "draw_slots", "draw_prioritized_rank", "draw_td"]),
                       ({"PERDQN": "rank", "DQN": "rank"}, ["draw_slots_rank", "draw_slots", "draw_prioritized", "draw_td_rank"]),
                       ({"D3QN": "rank", "PERD3QN": "rank", "PERDQN": "rank"}, ["draw_slots", "draw_slots_rank", "draw_prioritized_rank", "draw_td_rank"])):
        mp = pytest.MonkeyPatch()
        mp.setattr(envmod, "DeviceWorlds", Worlds)
        try:
            env = Environment(brains=_made("all"), n_worlds=4, rng="philox", learn_draw=draw, **every)
        finally:
            mp.undo()
        env.learn_now()
        got = [r[0] for r in env.worlds.log if r[0].startswith("draw")]
        assert got == want, (draw, got)
        assert env.learn_draw == draw
        note = env._weights_note()
        assert ("rl_learn_prioritized_draw_rank" in note) == (isinstance(draw, dict) and "PERD3QN" in draw)
        assert ("rl_learn_td_draw_rank" in note) == (isinstance(draw, dict) and "PERDQN" in draw)
        assert ("rl_learn_draw_rank" in note) == (draw == "rank" or (isinstance(draw, dict) and bool({"DQN", "D3QN"} & set(draw))))
