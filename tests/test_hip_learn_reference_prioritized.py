"""GPU: learn="reference" with learn_reference_prioritized=True -- rl_learn_prioritized_store_ref and rl_learn_prioritized_choice against
the literal buffer model and numpy's np.random.choice arithmetic (tests/learn_reference_prioritized_cases.py), and the trainer() run of
tests/golden/learn_reference_perd3qn.npz from seeds alone: the reference's actions, both generators' digests, every train()'s indices, the
outputs within test_hip_learn_reference.py's bar and the final priorities within twice that bar of the largest |q|.  Every figure a bar
is held against is printed before it is asserted."""
import glob
import hashlib
import os
import random
import warnings

import numpy as np
import pytest

import learn_reference_cases as lrc
import learn_reference_prioritized_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def _worlds():
    from reinlife_amd.worlds import DeviceWorlds
    if "w" not in _cache:
        _cache["w"] = DeviceWorlds(n_worlds=1, max_agents=10, n_brains=1, seed=3)
    return _cache["w"]


def _common(prios, kinds=None):
    from reinlife_amd import _lib
    n = len(prios)
    learners, sides = (_lib.Learner * n)(), (_lib.Prio * n)()
    for i, p in enumerate(prios):
        learners[i].kind = _lib.PERD3QN if kinds is None else kinds[i]
        sides[i].priority, sides[i].alpha = p.data_ptr(), 0.6
    return n, learners, sides


def _store(prios, capacities, first_rows, n_rows, kinds=None):
    """rl_learn_prioritized_store_ref on device float32 tensors indexed by ring slot -> (return code, message)"""
    from reinlife_amd import _lib
    w = _worlds()
    n, learners, sides = _common(prios, kinds)
    groups = (_lib.PrioStore * n)(*[_lib.PrioStore(int(c), int(p.numel()), int(a), int(m)) for p, c, a, m in zip(prios, capacities, first_rows, n_rows)])
    rc = w.lib.rl_learn_prioritized_store_ref(w.handle, learners, sides, groups, n, w._stream())
    return rc, w.lib.rl_last_error().decode()


def _choice(prios, capacities, stored, uniforms, bracket=True, kinds=None, batch=None, ring_rows=None):
    """rl_learn_prioritized_choice -> (return code, message, indices [n][batch], slots, bracket or None) as numpy; bracket starts at -7."""
    import torch
    from reinlife_amd import _lib
    w = _worlds()
    n, learners, sides = _common(prios, kinds)
    keep, draws = [], (_lib.PrioChoice * n)()
    for i, (p, c, s, u) in enumerate(zip(prios, capacities, stored, uniforms)):
        u = torch.as_tensor(np.asarray(u, np.float64), device=DEV)
        b = int(u.numel()) if batch is None else batch
        t = dict(u=u, indices=torch.full((max(b, 1),), -1, dtype=torch.int32, device=DEV), slots=torch.full((max(b, 1),), -1, dtype=torch.int32, device=DEV),
                 bracket=torch.full((max(b, 1), 2), -7.0, dtype=torch.float64, device=DEV),
                 work=torch.empty(max(int(w.lib.rl_learn_prioritized_choice_work_bytes(int(c))), 256), dtype=torch.uint8, device=DEV))
        keep.append(t)
        draws[i] = _lib.PrioChoice(int(c), int(p.numel()) if ring_rows is None else ring_rows, int(s), b, u.data_ptr(), t["indices"].data_ptr(),
                                   t["slots"].data_ptr(), t["bracket"].data_ptr() if bracket else None, t["work"].data_ptr())
    rc = w.lib.rl_learn_prioritized_choice(w.handle, learners, sides, draws, n, w._stream())
    msg = w.lib.rl_last_error().decode()
    torch.cuda.synchronize()
    return (rc, msg, [t["indices"].cpu().numpy() for t in keep], [t["slots"].cpu().numpy() for t in keep],
            [t["bracket"].cpu().numpy() for t in keep])


def _dev(a):
    import torch
    return torch.as_tensor(np.asarray(a, np.float32), device=DEV)


def _write(prio, slots, values):
    """update_priorities on the device tensor: in order, so of several writes to one slot the last one stays"""
    import torch
    last = dict(zip([int(x) for x in slots], [float(v) for v in values]))
    prio[torch.as_tensor(list(last), device=DEV)] = _dev(list(last.values()))


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


# ---- the store kernel -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity,slack", [(1, 4), (5, 4), (64, 4), (10_000, 256)])
def test_store_stamps_what_the_literal_buffer_stamps_through_two_wraps(capacity, slack):
    """Interleaved store groups of 1..slack rows and hand-made priority writes (between groups, as train() falls), through two wraps of
    the ring: the priorities at the live rows' slots are the literal model's, bit for bit.  The first row gets 1.0; groups cross the
    ring's end."""
    import torch
    R = capacity + slack
    model = pc.BufferModel(capacity, R)
    prio = torch.zeros(R, dtype=torch.float32, device=DEV)
    rng = np.random.RandomState(capacity)
    crossed, checks = 0, 0
    while model.stored < 2 * R + slack:
        m = int(rng.randint(1, slack + 1)) if model.stored else 1
        a = model.stored
        for _ in range(m):
            model.store()
        rc, msg = _store([prio], [capacity], [a], [m])
        assert rc == 0, msg
        crossed += (a % R) + m > R
        if a == 0:
            assert prio.cpu().numpy()[0] == 1.0 and model.by_slot[0] == 1.0
        if rng.rand() < 0.6:                                  # update_priorities on three live indices, up or down
            idx = rng.randint(0, len(model.memory), size=3)
            p = (rng.rand(3) * 10.0 ** rng.randint(-3, 3, size=3)).astype(np.float32)
            model.update_priorities(idx, p)
            _write(prio, model.slots(idx), p)
        if model.stored % 7 == 0 or model.stored >= 2 * R:
            live = model.slots(range(len(model.memory)))
            assert _bits(prio.cpu().numpy()[live]) == _bits(model.by_slot[live]) == _bits(model.priorities[:len(live)])
            checks += 1
    assert crossed >= 1 and checks >= 2
    _worlds().check_error_flag()


def test_store_propagates_a_nan_and_counts_unreached_indices_as_zero():
    import torch
    C_, R = 5, 9
    model = pc.BufferModel(C_, R)
    prio = torch.zeros(R, dtype=torch.float32, device=DEV)
    for a in range(3):
        model.store()
        assert _store([prio], [C_], [a], [1])[0] == 0
    model.update_priorities([0, 1, 2], np.array([-2.0, -3.0, -0.5], np.float32))     # all negative while a < C: the unused zeros win
    prio[:3] = _dev([-2.0, -3.0, -0.5])
    model.store()
    assert _store([prio], [C_], [3], [1])[0] == 0
    assert _bits(prio.cpu().numpy()[:4]) == _bits(model.by_slot[:4]) and float(model.by_slot[3]) == 0.0
    for a in range(4, 12):
        model.store()
        assert _store([prio], [C_], [a], [1])[0] == 0
    model.update_priorities([1], np.array([np.nan], np.float32))
    prio[model.slots([1])[0]] = float("nan")
    a = model.stored
    for _ in range(3):
        model.store()
    assert _store([prio], [C_], [a], [3])[0] == 0
    live = model.slots(range(C_))
    got = prio.cpu().numpy()
    assert _bits(got[live]) == _bits(model.by_slot[live]) and np.isnan(got[[x % R for x in range(a, a + 3)]]).all()


def test_store_serves_sixteen_learners_of_different_sizes_in_one_call():
    import torch
    caps = [1, 2, 3, 5, 8, 13, 21, 34, 55, 64, 100, 129, 255, 256, 1000, 4097]
    slacks = [1 + i % 4 for i in range(16)]
    models = [pc.BufferModel(c, c + s) for c, s in zip(caps, slacks)]
    prios = [torch.zeros(c + s, dtype=torch.float32, device=DEV) for c, s in zip(caps, slacks)]
    rng = np.random.RandomState(16)
    for _ in range(40):
        first, count = [], []
        for mdl, s in zip(models, slacks):
            m = int(rng.randint(1, s + 1))
            first.append(mdl.stored); count.append(m)
            for _ in range(m):
                mdl.store()
        rc, msg = _store(prios, caps, first, count)
        assert rc == 0, msg
        for mdl, p in zip(models, prios):
            idx = rng.randint(0, len(mdl.memory), size=2)
            v = (rng.rand(2) * 4.0).astype(np.float32)
            mdl.update_priorities(idx, v)
            _write(p, mdl.slots(idx), v)
    for mdl, p in zip(models, prios):
        live = mdl.slots(range(len(mdl.memory)))
        assert _bits(p.cpu().numpy()[live]) == _bits(mdl.by_slot[live])


def test_both_entry_points_refuse_what_the_header_says():
    import torch
    from reinlife_amd import _lib
    prio = torch.zeros(9, dtype=torch.float32, device=DEV)
    for m in (0, 5, -1):
        rc, msg = _store([prio], [5], [0], [m])
        assert rc == -1 and "n_rows must be in [1, ring_rows - capacity] = [1, 4]" in msg
    assert _store([prio], [5], [0], [4])[0] == 0
    rc, msg = _store([prio], [5], [0], [1], kinds=[_lib.D3QN])
    assert rc == -4 and "brain kind 1" in msg and "RL_PERD3QN" in msg
    rc, msg = _store([prio] * 17, [5] * 17, [0] * 17, [1] * 17)
    assert rc == -1 and "n_learners must be in [1,16]" in msg
    rc, msg = _store([prio], [10], [0], [1])
    assert rc == -1 and "ring_rows must be in [capacity, 2^31)" in msg
    u = np.full(4, 0.5)
    rc, msg, *_ = _choice([prio], [5], [0], [u])
    assert rc == -1 and "stored must be >= 1" in msg
    rc, msg, *_ = _choice([prio], [5], [3], [np.full(65, 0.5)])
    assert rc == -1 and "batch must be in [1,64] (got 65)" in msg
    rc, msg, *_ = _choice([prio], [5], [3], [u], batch=0)
    assert rc == -1 and "batch must be in [1,64] (got 0)" in msg
    rc, msg, *_ = _choice([prio], [5], [3], [u], kinds=[_lib.PERDQN])
    assert rc == -4 and "brain kind 4" in msg
    rc, msg, *_ = _choice([prio], [2 ** 31], [3], [u], ring_rows=2 ** 31)
    assert rc == -1 and "capacity must be in [1, 2^31)" in msg
    assert int(_worlds().lib.rl_learn_prioritized_choice_work_bytes(2 ** 31)) == 0
    assert int(_worlds().lib.rl_learn_prioritized_choice_work_bytes(10_000)) >= 120_000


# ---- the choice kernel ------------------------------------------------------------------------------------------------------------

def _snapshot(g, k, R):
    """Call k of the fixture as a priority array by ring slot (every slot no live row sits in: a NaN)."""
    from reinlife_amd.learn_reference import memory_slots
    n, stored, Cc = int(g["call_size"][k]), int(g["call_stored"][k]), int(g["capacity"])
    by_slot = np.full(R, np.nan, np.float32)
    by_slot[memory_slots(stored, Cc, R, np.arange(n))] = g["call_prio"][k, :n]
    return by_slot


def test_choice_names_the_references_indices_from_the_fixtures_snapshots():
    """All train() calls of the run, sixteen learners per launch: the fixture's priorities and uniforms give the fixture's indices and
    their ring slots, every draw; the brackets lie within 2^-21 of numpy's; a call of batch 1 names the first index."""
    from reinlife_amd.learn_reference import memory_slots
    g = pc.load()
    Cc, R = int(g["capacity"]), int(g["capacity"]) + 64
    K = len(g["call_tick"])
    worst = 0.0
    for lo in range(0, K, 16):
        ks = list(range(lo, min(lo + 16, K)))
        prios = [_dev(_snapshot(g, k, R)) for k in ks]
        rc, msg, idx, slots, br = _choice(prios, [Cc] * len(ks), g["call_stored"][ks], g["call_uniforms"][ks])
        assert rc == 0, msg
        for j, k in enumerate(ks):
            assert idx[j].tolist() == g["call_indices"][k, 0].tolist(), k
            assert slots[j].tolist() == memory_slots(int(g["call_stored"][k]), Cc, R, g["call_indices"][k, 0]).tolist()
            worst = max(worst, float(np.abs(br[j] - g["call_bracket"][k]).max()))
        rc, msg, idx1, slots1, _ = _choice(prios[:1], [Cc], g["call_stored"][ks[:1]], [g["call_uniforms"][ks[0], :1]])
        assert rc == 0 and idx1[0].tolist() == [int(g["call_indices"][ks[0], 0, 0])] and slots1[0][0] == slots[0][0]
    print("largest |bracket - numpy's| over %d draws: %.3g (bar 2^-21 = %.3g)" % (K * int(g["batch"]), worst, 2.0 ** -21))
    assert K > 16 and worst <= 2.0 ** -21
    _worlds().check_error_flag()


def test_choice_resolves_exact_ties_to_the_next_row_and_skips_rows_of_weight_zero():
    prio = _dev(np.full(64 + 4, 0.37))
    u = np.arange(64) / 64.0
    rc, msg, idx, slots, br = _choice([prio], [64], [64], [u])
    assert rc == 0, msg
    assert idx[0].tolist() == list(range(64)) and slots[0].tolist() == list(range(64))      # side="right": u = k/64 = cdf[k-1] names row k
    assert np.array_equal(br[0][:, 1], (np.arange(64) + 1) / 64.0) and np.array_equal(br[0][:, 0], u)
    p = np.array([0, 0, 0, 0.5, 0, 2.0, 0, 0], np.float32)
    rc, msg, idx, _, br = _choice([_dev(np.concatenate([p, np.zeros(2, np.float32)]))], [8], [8], [[0.0, np.nextafter(1.0, 0.0), 0.3]])
    assert rc == 0 and idx[0].tolist()[:2] == [3, 5] and idx[0][2] in (3, 5)               # u = 0: the first row of nonzero weight
    assert br[0][0].tolist() == [0.0, br[0][0][1]] and br[0][1][1] == 1.0


@pytest.mark.parametrize("n", pc.CHOICE_SIZES)
def test_choice_names_numpys_indices_on_hand_made_memories(n):
    """n = C priorities over six binades with zeros, at stored = n, C + 5 and 3 C - 1 (three learners of one call), 64 uniforms each that
    numpy's arithmetic keeps 2^-20 from their brackets' ends: numpy's indices, every draw; no zero-weight row; no slot outside the live
    rows (they hold NaNs); a second identical call gives the same bits in all three outputs."""
    from reinlife_amd.learn_reference import memory_slots
    cases = [pc.choice_case(n, s) for s in (n, n + 5, 3 * n - 1)]
    prios = [_dev(c["by_slot"]) for c in cases]
    args = (prios, [n] * 3, [c["stored"] for c in cases], [c["u"] for c in cases])
    rc, msg, idx, slots, br = _choice(*args)
    assert rc == 0, msg
    worst = 0.0
    for c, i, s, b in zip(cases, idx, slots, br):
        assert i.tolist() == c["idx"].tolist(), (n, c["stored"])
        assert (c["prio"][i] > 0).all()
        assert s.tolist() == memory_slots(c["stored"], n, c["ring_rows"], c["idx"]).tolist()
        assert ((b[:, 0] <= c["u"]) & (c["u"] < b[:, 1])).all()
        worst = max(worst, float(np.abs(b - c["bracket"]).max()))
    print("n = %d: largest |bracket - numpy's| %.3g (2^-21 = %.3g)" % (n, worst, 2.0 ** -21))
    assert worst <= 2.0 ** -21
    rc, msg, idx2, slots2, br2 = _choice(*args)
    assert rc == 0
    for a, b in zip(idx + slots + br, idx2 + slots2 + br2):
        assert a.tobytes() == b.tobytes()
    _worlds().check_error_flag()


@pytest.mark.parametrize("what", ["zeros", "nan", "negative"])
def test_choice_refuses_priorities_np_random_choice_refuses(what):
    """All-zero, NaN and negative priorities: error-flag code 7 naming the learner, every draw index 0 and the slot of memory index 0,
    and the bracket is not written."""
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.learn_reference import memory_slots
    w = _worlds()
    Cc, R, stored = 8, 11, 21
    p = np.zeros(R, np.float32)
    live = memory_slots(stored, Cc, R, np.arange(Cc))
    if what != "zeros":
        p[live] = np.linspace(0.5, 2.0, Cc)
        p[live[3]] = np.nan if what == "nan" else -1.0
    good = np.zeros(R, np.float32)
    good[live] = 1.0
    w.err.zero_()
    rc, msg, idx, slots, br = _choice([_dev(good), _dev(p)], [Cc, Cc], [stored, stored], [np.linspace(0.05, 0.95, 6)] * 2)
    assert rc == 0, msg
    torch.cuda.synchronize()
    err = w.err.cpu().numpy().tolist()
    w.err.zero_()
    assert err == [_lib.ERR_NO_DISTRIBUTION, 1, Cc, 0]
    assert idx[1].tolist() == [0] * 6 and slots[1].tolist() == [int(live[0])] * 6 and (br[1] == -7.0).all()
    assert idx[0].tolist() == [0, 1, 3, 4, 6, 7] and (br[0] != -7.0).all()                 # the learner beside it drew


# ---- the run ----------------------------------------------------------------------------------------------------------------------

def _digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def _run(g, brains, ticks=None, save=False, **kw):
    """trainer() on the fixture's configuration and seeds, watched as tests/test_hip_learn_reference.py watches its runs: per tick the
    actions and both generators' digests, and a copy of each learner's parameters right behind its first update, in stream order."""
    from reinlife_amd import Environment, trainer
    from reinlife_amd.worlds import DeviceWorlds
    ticks = int(g["ticks"]) if ticks is None else ticks
    rec = dict(actions=[], digest=[], np_digest=[], entries=[], first={})
    mp = pytest.MonkeyPatch()
    step, update, dev_learn = Environment.step, Environment.update_env, DeviceWorlds.learn

    def w_step(env):
        m = env._mat(0)
        rec["actions"].append(np.array(m.actions[:m.n], np.int8))
        return step(env)

    def w_update(env, n_epi=0):
        r = update(env, n_epi)
        rec["digest"].append(_digest()); rec["np_digest"].append(pc.np_digest())
        return r

    def w_dev_learn(worlds, learners, n_steps, slots=None, gate=True):
        r = dev_learn(worlds, learners, n_steps, slots=slots, gate=gate)
        l = learners[0]
        rec["entries"].append((l.entry, int(l.batch), int(n_steps)))
        if id(l.params) not in rec["first"]:
            rec["first"][id(l.params)] = l.params.clone()
        return r

    mp.setattr(Environment, "step", w_step)
    mp.setattr(Environment, "update_env", w_update)
    mp.setattr(DeviceWorlds, "learn", w_dev_learn)
    mp.setattr(Environment, "log_reference_calls", True)
    try:
        lrc.seed_all(int(g["seed"]))   # after construction, like the recorder
        env = trainer(brains, n_episodes=ticks - 1, width=pc.CASE["width"], height=pc.CASE["height"], max_agents=pc.CASE["max_agents"],
                      print_results=False, save=save, learn="reference", **kw)
    finally:
        mp.undo()
    rec["env"] = env
    rec["first"] = {k: rec["first"][id(l.params)].cpu().numpy() for k, l in env.learners.items() if id(l.params) in rec["first"]}
    rec["final"] = {k: l.params.cpu().numpy() for k, l in env.learners.items()}
    return rec


def test_trainer_trains_the_perd3qn_brain_as_the_reference_does_from_seeds():
    from reinlife_amd.learn_reference import memory_slots
    g = pc.load()
    brains = pc.product_brains(g)
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # one PERD3QN brain, and it trains: nothing is frozen, nothing warns
        r = _run(g, brains, learn_reference_prioritized=True)
    env, T, Cc = r["env"], int(g["ticks"]), int(g["capacity"])
    assert env.ring_rows == [Cc + 64] and env.learners[0].entry == "rl_learn_prioritized" and env.learners[0].priority.numel() == Cc + 64
    # the actions, tick for tick, and both generators after every tick
    assert len(r["actions"]) == T
    for t in range(T):
        assert r["actions"][t].tolist() == g["actions"][t, :int(g["n0"][t])].tolist(), "actions of tick %d" % t
    assert r["digest"] == g["digest"].tolist() and r["np_digest"] == g["np_digest"].tolist()
    # the calls: tick, len(memory), target copy, uniforms -- and the indices the device chose
    made = [(t, c) for t, c in env.reference_calls if c.kind == "learn"]
    assert [t for t, _ in made] == g["call_tick"].tolist() and [c.size for _, c in made] == g["call_size"].tolist()
    assert [int(c.sync_target) for _, c in made] == g["call_sync"].tolist()
    assert [(t, c.brain) for t, c in env.reference_calls if c.kind == "sync"] == list(zip(g["sync_tick"].tolist(), g["sync_brain"].tolist()))
    assert r["entries"] == [("rl_learn_prioritized", int(g["batch"]), 1)] * len(made)
    assert len(env.reference_choices) == len(made)
    worst_br = 0.0
    for k, (t, b, idx, slots, bracket) in enumerate(env.reference_choices):
        assert (t, b) == (int(g["call_tick"][k]), 0)
        assert idx.cpu().numpy().tolist() == g["call_indices"][k, 0].tolist(), "indices of call %d" % k
        assert slots.cpu().numpy().tolist() == memory_slots(int(g["call_stored"][k]), Cc, Cc + 64, g["call_indices"][k, 0]).tolist()
        worst_br = max(worst_br, float(np.abs(bracket.cpu().numpy() - g["call_bracket"][k]).max()))
    print("largest |bracket - the reference's| over the run: %.3g (D of the fixture %.3g)" % (worst_br, float(g["cdf_err"])))
    # the bar: outputs in float64 on the fixture's states, after the first update and at the end
    bar = float(g["ref_q_spread"][0]) * (1e-5 / float(g["ref_grad_err"][0]))
    ratios = {}
    for when, got in (("first", r["first"][0]), ("final", r["final"][0])):
        ref, init = g["out_" + when][0], g["out_init"][0]
        ratios[when] = np.abs(lrc.outputs64(pc.KIND, got, g["states"]) - ref).max() / np.abs(ref - init).max()
        print("%s update: max|d out| / training effect = %.3g (bar %.3g; ratio / bar %.3g); effect %.3g"
              % (when, ratios[when], bar, ratios[when] / bar, np.abs(ref - init).max()))
    # the final priorities of the live rows: a priority is a difference of two outputs -> twice the bar, relative to the largest |q|
    qmax = max(float(np.abs(g["out_" + k][0]).max()) for k in ("init", "first", "final"))
    live = memory_slots(int(g["final_stored"]), Cc, Cc + 64, np.arange(Cc))
    got_prio = env.learners[0].priority.cpu().numpy()[live]
    prio_ratio = float(np.abs(got_prio.astype(np.float64) - g["final_prio"].astype(np.float64)).max()) / qmax
    print("final priorities: max|d p| / largest |q| = %.3g (bar %.3g; ratio / bar %.3g); largest |q| %.3g" % (prio_ratio, 2 * bar, prio_ratio / (2 * bar), qmax))
    assert int(env.learners[0].ring["count"].item()) == int(g["final_stored"]) == env.schedule.stored[0] == env.schedule.stamped[0]
    assert ratios["first"] <= bar and ratios["final"] <= bar
    assert prio_ratio <= 2 * bar
    # the acting weights are the learner's
    assert brains[0].state_dict_flat().tobytes() == r["final"][0].tobytes()
    assert not np.array_equal(r["final"][0], lrc.weights(pc.KIND, int(g["init_seeds"][0])))
    assert "learn_reference_prioritized=True" in env._weights_note() and "brains [0] trained" in env._weights_note()


def test_save_writes_the_trained_weights_and_the_run_without_the_keyword_is_what_it_was(tmp_path, monkeypatch):
    """save=True a dozen ticks past the first update: the saved PERD3QN file holds the learner's parameters.  Without the keyword the
    mode is what it was: a PERD3QN brain alone is refused (nothing trains), and beside a DQN brain -- the mode needs one brain it
    trains -- it is named by the warning as today, gets no learner and a ring of the floor's size, and keeps its weights."""
    import torch
    from reinlife_amd import Models
    g = pc.load()
    first = int(g["first_update_tick"].min())
    monkeypatch.chdir(tmp_path)
    r = _run(g, pc.product_brains(g), ticks=first + 12, save=True, learn_reference_prioritized=True)
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "PERD3QN", "brain_gene_*.pt")))
    assert len(files) == 1
    flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(files[0]).values()])
    assert flat.tobytes() == r["final"][0].tobytes() and not np.array_equal(flat, lrc.weights(pc.KIND, int(g["init_seeds"][0])))
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "learn_reference_prioritized=True" in settings and "inference only" not in settings
    for t in range(first + 12):
        assert r["actions"][t].tolist() == g["actions"][t, :int(g["n0"][t])].tolist(), t
    # without the keyword
    with pytest.raises(ValueError, match="none of the brains is of a kind that trains in this mode"):
        _run(g, pc.product_brains(g), ticks=2)
    brains = pc.product_brains(g) + [Models.DQN(max_epi=100)]
    before = brains[0].state_dict_flat().copy()
    with pytest.warns(UserWarning, match=r"learn='reference' trains the DQN, D3QN and PPO brains.*0 \(PERD3QN\).*NOT updated"):
        n = _run(g, brains, ticks=first + 12)
    env = n["env"]
    assert sorted(env.learners) == [1] and env.ring_rows == [64, 50_000 + 64] and env.schedule.specs[0] is None
    assert env.reference_choices == [] and all(c.brain == 1 for _, c in env.reference_calls)
    assert brains[0].state_dict_flat().tobytes() == before.tobytes()
    # with the keyword the warning names PERDQN brains only
    brains = pc.product_brains(g) + [Models.PERDQN()]
    with pytest.warns(UserWarning, match=r"learn_reference_prioritized=True trains the DQN, D3QN, PPO and PERD3QN brains.*brains 1 \(PERDQN\) are") as rec:
        from reinlife_amd import Environment
        Environment(brains=brains, max_agents=10, print_results=False, learn="reference", learn_reference_prioritized=True)
    assert not any("PERD3QN)" in str(x.message).split("are of")[0].split("brains of this run; brains")[1] for x in rec)
