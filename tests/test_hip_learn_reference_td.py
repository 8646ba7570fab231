"""GPU: learn="reference" with learn_reference_td=True -- rl_learn_td_tree_store, rl_learn_td_tree_sample and rl_learn_td_tree_update against
the literal sequential model of the reference's sum tree (tests/learn_reference_td_cases.py), bit for bit, and the trainer() run of
tests/golden/learn_reference_perdqn.npz from seeds alone: the reference's actions, both generators' digests, every train_model()'s tree
indices, beta and epsilon exactly, the outputs within test_hip_learn_reference.py's bar and the final leaf priorities within twice that
bar of the largest |q|.  Every figure a bar is held against is printed before it is asserted."""
import hashlib
import random
import warnings

import numpy as np
import pytest

import learn_reference_cases as lrc
import learn_reference_prioritized_cases as pc
import learn_reference_td_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def _worlds():
    from reinlife_amd.worlds import DeviceWorlds
    if "w" not in _cache:
        _cache["w"] = DeviceWorlds(n_worlds=1, max_agents=10, n_brains=1, seed=3)
    return _cache["w"]


class Mem:
    """One learner's device side: the tree, the priorities by ring slot, and the literal model beside them."""

    def __init__(self, capacity, slack):
        import torch
        self.C, self.R = capacity, capacity + slack
        self.tree = torch.zeros(2 * capacity - 1, dtype=torch.float64, device=DEV)
        self.priority = torch.zeros(self.R, dtype=torch.float32, device=DEV)
        self.model = tc.TreeModel(capacity, self.R)

    def same(self):
        return (self.tree.cpu().numpy().view(np.uint64).tolist() == self.model.tree.view(np.uint64).tolist()
                and self.priority.cpu().numpy().view(np.uint32).tolist() == self.model.priority.view(np.uint32).tolist())


def _common(mems, kinds=None):
    from reinlife_amd import _lib
    n = len(mems)
    learners, sides = (_lib.Learner * n)(), (_lib.TdPrio * n)()
    for i, m in enumerate(mems):
        learners[i].kind = _lib.PERDQN if kinds is None else kinds[i]
        sides[i].priority, sides[i].p_new = m.priority.data_ptr(), float(tc.p_new())
    return n, learners, sides


def _call(name, mems, args, kinds=None):
    w = _worlds()
    n, learners, sides = _common(mems, kinds)
    rc = getattr(w.lib, name)(w.handle, learners, sides, args, n, w._stream())
    return rc, w.lib.rl_last_error().decode()


def _store(mems, first_rows, n_rows, kinds=None, capacity=None, ring_rows=None, tree=True):
    from reinlife_amd import _lib
    args = (_lib.TdTreeStore * len(mems))(*[_lib.TdTreeStore(m.tree.data_ptr() if tree else None, m.C if capacity is None else capacity,
                                                              m.R if ring_rows is None else ring_rows, int(a), int(k))
                                            for m, a, k in zip(mems, first_rows, n_rows)])
    return _call("rl_learn_td_tree_store", mems, args, kinds)


def _update(mems, idxs, slots, kinds=None, n=None):
    import torch
    from reinlife_amd import _lib
    keep = [(torch.as_tensor(np.asarray(i, np.int32), device=DEV), torch.as_tensor(np.asarray(s, np.int32), device=DEV)) for i, s in zip(idxs, slots)]
    args = (_lib.TdTreeUpdate * len(mems))(*[_lib.TdTreeUpdate(m.tree.data_ptr(), m.C, m.R, int(i.numel()) if n is None else n, i.data_ptr(), s.data_ptr())
                                             for m, (i, s) in zip(mems, keep)])
    out = _call("rl_learn_td_tree_update", mems, args, kinds)
    torch.cuda.synchronize()
    return out


def _sample(mems, stored, uniforms, kinds=None, n=None):
    """-> (return code, message, idxs, slots, s, leaves) as lists of numpy arrays; s and leaves start at -7."""
    import torch
    from reinlife_amd import _lib
    keep, args = [], (_lib.TdTreeSample * len(mems))()
    for k, (m, st, u) in enumerate(zip(mems, stored, uniforms)):
        u = torch.as_tensor(np.asarray(u, np.float64), device=DEV)
        b = int(u.numel())
        t = dict(u=u, idxs=torch.full((b,), -1, dtype=torch.int32, device=DEV), slots=torch.full((b,), -1, dtype=torch.int32, device=DEV),
                 s=torch.full((b,), -7.0, dtype=torch.float64, device=DEV), leaves=torch.full((b,), -7.0, dtype=torch.float64, device=DEV))
        keep.append(t)
        args[k] = _lib.TdTreeSample(m.tree.data_ptr(), m.C, m.R, int(st), b if n is None else n, u.data_ptr(), t["idxs"].data_ptr(), t["slots"].data_ptr(),
                                    t["s"].data_ptr(), t["leaves"].data_ptr())
    rc, msg = _call("rl_learn_td_tree_sample", mems, args, kinds)
    torch.cuda.synchronize()
    return (rc, msg) + tuple([t[k].cpu().numpy() for t in keep] for k in ("idxs", "slots", "s", "leaves"))


def _dev_write(mem, values_by_leaf):
    """What rl_learn_td leaves behind for an update batch: the new priority of every distinct row, at its ring slot."""
    import torch
    slots = [mem.model.slot_of(leaf) for leaf in values_by_leaf]
    mem.priority[torch.as_tensor(slots, device=DEV)] = torch.as_tensor(np.array(list(values_by_leaf.values()), np.float32), device=DEV)


def _drive(mem, ops):
    """The script on the device and the model side by side -> the number of checks made (each: tree as uint64, priority as uint32)."""
    n = {"checks": 0, "crossed": 0}
    p = tc.p_new()

    def on_store(first, m):
        rc, msg = _store([mem], [first], [m])
        assert rc == 0, msg
        n["crossed"] += (first % mem.R) + m > mem.R

    def on_update(idxs, slots, vals):
        _dev_write(mem, vals)
        rc, msg = _update([mem], [idxs], [slots])
        assert rc == 0, msg

    def on_check():
        assert mem.same(), "after %d rows" % mem.model.stored
        n["checks"] += 1

    # (run_script applies an operation to the model first; slot_of() needs the model's row count as of the update, which a store has set)
    tc.run_script(mem.model, ops, p, on_store, on_update, on_check)
    return n


# ---- store and update -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("capacity,slack", tc.TREE_CASES)
def test_store_and_update_leave_the_sequential_references_bits(capacity, slack):
    """Store groups of 1 .. slack rows interleaved with update batches of 1 and 64 entries that name leaves twice, through two wraps of
    the ring: the tree and the priorities are the literal model's, bit for bit, at every check.  Then three samples on the tree that
    has grown: u = 0, u at its largest value below 1 and random u give the model's idxs, slots, s and leaves, bit for bit."""
    mem = Mem(capacity, slack)
    n = _drive(mem, tc.script(capacity, slack))
    assert n["checks"] >= 2 and n["crossed"] >= 1 and mem.model.stored >= 2 * mem.R
    rng = np.random.RandomState(capacity)
    for u in (np.zeros(64), np.full(64, np.nextafter(1.0, 0.0)), rng.random_sample(64), rng.random_sample(1), rng.random_sample(7)):
        want = mem.model.sample(u)
        rc, msg, idxs, slots, s, leaves = _sample([mem], [mem.model.stored], [u])
        assert rc == 0 and not want["bad"], msg
        assert idxs[0].tolist() == want["idxs"] and slots[0].tolist() == want["slots"]
        assert s[0].tobytes() == want["s"].tobytes() and leaves[0].tobytes() == want["leaves"].tobytes()
    _worlds().check_error_flag()


def test_sample_goes_left_where_s_equals_the_left_sum_and_follows_a_partly_filled_memory():
    import torch
    mem = Mem(4, 3)
    mem.model.tree[:] = [4, 2, 2, 1, 1, 1, 1]
    mem.model.stored = 4
    mem.tree.copy_(torch.as_tensor(mem.model.tree))
    rc, msg, idxs, slots, s, leaves = _sample([mem], [4], [np.zeros(4)])            # s_i = i exactly: 1 = tree[3], 2 = tree[1]
    assert rc == 0 and s[0].tolist() == [0.0, 1.0, 2.0, 3.0] and idxs[0].tolist() == [3, 3, 4, 5] == mem.model.sample(np.zeros(4))["idxs"]
    assert slots[0].tolist() == [0, 0, 1, 2]
    # a memory that is not full yet, leaves at two depths: the unreached leaves hold 0 and no draw with s > 0 ends there.  With C = 5
    # the two deepest leaves (memory indices 3 and 4) are the tree's leftmost: s = 0 walks `<=` down to index 3, which no row has
    # reached -- the reference would draw again there, the device says code 8 (random.random() gives 0.0 once in 2^53 draws)
    from reinlife_amd import _lib
    w = _worlds()
    part = Mem(5, 4)
    part.model.store(3, tc.p_new())
    assert _store([part], [0], [3])[0] == 0 and part.same()
    rng = np.random.RandomState(5)
    w.check_error_flag()
    for u in (np.full(64, np.nextafter(1.0, 0.0)), rng.random_sample(64), np.full(64, 2.0 ** -53)):
        want = part.model.sample(u)
        rc, msg, idxs, slots, s, leaves = _sample([part], [3], [u])
        assert rc == 0 and not want["bad"] and idxs[0].tolist() == want["idxs"] and slots[0].tolist() == want["slots"]
        assert s[0].tobytes() == want["s"].tobytes() and leaves[0].tobytes() == want["leaves"].tobytes()
        assert max(want["idxs"]) - 4 < 3
    w.check_error_flag()
    want = part.model.sample(np.zeros(3))
    rc, msg, idxs, slots, s, leaves = _sample([part], [3], [np.zeros(3)])
    err = w.err.cpu().numpy().tolist()
    w.err.zero_()
    assert rc == 0 and want["bad"] and err == [_lib.ERR_TREE_REDRAW, 0, 0, 3] and idxs[0].tolist() == want["idxs"] == [4, 4, 4]


# ---- code 8 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", ["unreached", "zeros"])
def test_sample_refuses_where_the_reference_would_draw_again(what):
    """A partly filled tree whose hand-made node values steer a draw onto a leaf no row has reached, and an all-zero tree: error-flag
    code 8 naming the learner, every draw of that learner leaf C - 1 and its slot, s and leaves not written; the learner beside it drew."""
    import torch
    from reinlife_amd import _lib
    w = _worlds()
    good, bad = Mem(8, 4), Mem(8, 4)
    for first, m in ((0, 4), (4, 4), (8, 3)):
        good.model.store(m, tc.p_new())
        assert _store([good], [first], [m])[0] == 0
    if what == "unreached":
        bad.model.store(3, tc.p_new())
        bad.model.tree[8 - 1 + 5] = 1.0
        for node in (5, 2, 0):
            bad.model.tree[node] += 1.0
        bad.tree.copy_(torch.as_tensor(bad.model.tree))
    stored = 3 if what == "unreached" else 1
    bad.model.stored = stored
    u = np.linspace(0.05, 0.95, 6)
    want_good, want_bad = good.model.sample(u), bad.model.sample(u)
    assert want_bad["bad"] and not want_good["bad"]
    w.err.zero_()
    rc, msg, idxs, slots, s, leaves = _sample([good, bad], [11, stored], [u, u])
    assert rc == 0, msg
    err = w.err.cpu().numpy().tolist()
    w.err.zero_()
    assert err[:2] == [_lib.ERR_TREE_REDRAW, 1] and (err[2:] == [-1, 0] if what == "zeros" else err[3] == 5)
    assert idxs[1].tolist() == [7] * 6 == want_bad["idxs"] and slots[1].tolist() == want_bad["slots"]
    assert (s[1] == -7.0).all() and (leaves[1] == -7.0).all()
    assert idxs[0].tolist() == want_good["idxs"] and slots[0].tolist() == want_good["slots"] and s[0].tobytes() == want_good["s"].tobytes()
    with pytest.raises(_lib.ReinLifeHipError, match="code 8.*rl_learn_td_tree_sample.*draws again"):
        w.raise_on_error_flag(np.array(err))


# ---- several learners -------------------------------------------------------------------------------------------------------------

def test_sixteen_learners_of_different_capacities_in_one_call():
    caps = [2, 3, 4, 5, 7, 8, 13, 21, 33, 64, 100, 129, 255, 256, 1000, 4097]
    mems = [Mem(c, 1 + i % 5) for i, c in enumerate(caps)]
    rng = np.random.RandomState(16)
    p = tc.p_new()
    for r in range(30):
        first, count = [], []
        for m in mems:
            k = int(rng.randint(1, m.R - m.C + 1))
            first.append(m.model.stored); count.append(k)
            m.model.store(k, p)
        rc, msg = _store(mems, first, count)
        assert rc == 0, msg
        idxs, slots = [], []
        for m in mems:
            i = rng.randint(0, min(m.model.stored, m.C), size=64) + m.C - 1
            vals = {int(x): np.float32(2.0 ** rng.uniform(-3, 3)) for x in set(i.tolist())}
            s = np.array([m.model.slot_of(x) for x in i], np.int32)
            _dev_write(m, vals)
            for leaf, v in vals.items():
                m.model.priority[m.model.slot_of(leaf)] = v
            m.model.update_batch(i, s)
            idxs.append(i); slots.append(s)
        rc, msg = _update(mems, idxs, slots)
        assert rc == 0, msg
        if r % 10 == 9:
            assert all(m.same() for m in mems)
            us = [rng.random_sample(64) for _ in mems]
            want = [m.model.sample(u) for m, u in zip(mems, us)]
            rc, msg, gi, gs, s, leaves = _sample(mems, [m.model.stored for m in mems], us)
            assert rc == 0, msg
            for k, wnt in enumerate(want):
                assert not wnt["bad"] and gi[k].tolist() == wnt["idxs"] and gs[k].tolist() == wnt["slots"] and s[k].tobytes() == wnt["s"].tobytes()
    _worlds().check_error_flag()


def test_update_skips_a_leaf_outside_the_tree_and_says_so():
    from reinlife_amd import _lib
    w = _worlds()
    mem = Mem(5, 4)
    mem.model.store(5, tc.p_new())
    assert _store([mem], [0], [4])[0] == 0 and _store([mem], [4], [1])[0] == 0
    _dev_write(mem, {4: np.float32(2.0), 5: np.float32(0.5)})
    mem.model.priority[:2] = [2.0, 0.5]
    w.err.zero_()
    assert _update([mem], [[4, 9, 3, 5]], [[0, 0, 0, 1]])[0] == 0            # 9 = 2 C - 1 and 3 = C - 2 lie outside the leaves
    err = w.err.cpu().numpy().tolist()
    w.err.zero_()
    assert err[0] == _lib.ERR_TREE_INDEX == 9 and err[1] == 0 and (err[2], err[3]) in ((1, 9), (2, 3))
    with pytest.raises(_lib.ReinLifeHipError, match="code 9.*rl_learn_td_tree_update.*outside"):
        w.raise_on_error_flag(np.array(err))
    mem.model.update_batch([4, 5], [0, 1])
    assert mem.same()


# ---- host refusals ----------------------------------------------------------------------------------------------------------------

def test_the_entry_points_refuse_what_the_header_says():
    from reinlife_amd import _lib
    mem = Mem(5, 4)
    for m in (0, 5, -1):
        rc, msg = _store([mem], [0], [m])
        assert rc == -1 and "n_rows must be in [1, ring_rows - capacity] = [1, 4]" in msg
    assert _store([mem], [0], [4])[0] == 0
    rc, msg = _store([mem], [-1], [1])
    assert rc == -1 and "first_row must be >= 0" in msg
    for name, call in (("rl_learn_td_tree_store", lambda **k: _store([mem], [0], [1], **k)),
                       ("rl_learn_td_tree_sample", lambda **k: _sample([mem], [3], [np.full(4, 0.5)], **k)[:2]),
                       ("rl_learn_td_tree_update", lambda **k: _update([mem], [[4]], [[0]], **k))):
        rc, msg = call(kinds=[_lib.PERD3QN])
        assert rc == -4 and name in msg and "brain kind 2" in msg and "RL_PERDQN" in msg
    rc, msg = _store([mem], [0], [1], capacity=1, ring_rows=5)
    assert rc == -1 and "capacity must be in [2, 2^30] (got 1)" in msg and "_propagate never ends" in msg
    rc, msg = _store([mem], [0], [1], capacity=2 ** 30 + 1, ring_rows=2 ** 31 - 1)
    assert rc == -1 and "capacity must be in [2, 2^30]" in msg
    rc, msg = _store([mem], [0], [1], ring_rows=4)
    assert rc == -1 and "ring_rows must be in [capacity, 2^31)" in msg
    rc, msg = _store([mem], [0], [1], tree=False)
    assert rc == -1 and "tree must not be null" in msg
    rc, msg = _store([mem] * 17, [0] * 17, [1] * 17)
    assert rc == -1 and "n_learners must be in [1,16]" in msg
    rc, msg, *_ = _sample([mem], [0], [np.full(4, 0.5)])
    assert rc == -1 and "stored must be >= 1" in msg
    rc, msg, *_ = _sample([mem], [3], [np.full(65, 0.5)])
    assert rc == -1 and "n must be in [1,64] (got 65)" in msg
    rc, msg, *_ = _sample([mem], [3], [np.full(4, 0.5)], n=0)
    assert rc == -1 and "n must be in [1,64] (got 0)" in msg
    rc, msg = _update([mem], [[4] * 65], [[0] * 65])
    assert rc == -1 and "n must be in [1,64] (got 65)" in msg
    rc, msg = _update([mem], [[4]], [[0]], n=0)
    assert rc == -1 and "n must be in [1,64] (got 0)" in msg
    _worlds().check_error_flag()


# ---- the run ----------------------------------------------------------------------------------------------------------------------

def _digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def _run(g, brains, ticks=None, **kw):
    """trainer() on the fixture's configuration and seeds, watched as tests/test_hip_learn_reference_prioritized.py watches its run."""
    from reinlife_amd import Environment, trainer
    from reinlife_amd.worlds import DeviceWorlds
    ticks = int(g["ticks"]) if ticks is None else ticks
    rec = dict(actions=[], digest=[], np_digest=[], entries=[], first={}, epsilon=[])
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
        rec["entries"].append((l.entry, int(l.batch), int(n_steps), int(l.min_size), bool(l.sync_target)))
        rec["epsilon"].append(float(l.brain.epsilon))
        if id(l.params) not in rec["first"]:
            rec["first"][id(l.params)] = l.params.clone()
        return r

    mp.setattr(Environment, "step", w_step)
    mp.setattr(Environment, "update_env", w_update)
    mp.setattr(DeviceWorlds, "learn", w_dev_learn)
    mp.setattr(Environment, "log_reference_calls", True)
    try:
        lrc.seed_all(int(g["seed"]))   # after construction, like the recorder
        env = trainer(brains, n_episodes=ticks - 1, width=tc.CASE["width"], height=tc.CASE["height"], max_agents=tc.CASE["max_agents"],
                      print_results=False, learn="reference", **kw)
    finally:
        mp.undo()
    rec["env"] = env
    rec["first"] = {k: rec["first"][id(l.params)].cpu().numpy() for k, l in env.learners.items() if id(l.params) in rec["first"]}
    rec["final"] = {k: l.params.cpu().numpy() for k, l in env.learners.items()}
    return rec


def test_trainer_trains_the_perdqn_brain_as_the_reference_does_from_seeds():
    """The final outputs and leaf priorities are held to the bars of test_hip_learn_reference_prioritized.py."""
    from reinlife_amd.learn_reference import memory_slots
    g = tc.load()
    brains = tc.product_brains(g)
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # one PERDQN brain, and it trains: nothing is frozen, nothing warns
        r = _run(g, brains, learn_reference_td=True)
    env, T, C = r["env"], int(g["ticks"]), int(g["capacity"])
    l = env.learners[0]
    assert env.ring_rows == [C + 64] and l.entry == "rl_learn_td" and l.priority.numel() == C + 64 and l.ref_tree.numel() == 2 * C - 1
    # the actions, tick for tick, and both generators after every tick
    assert len(r["actions"]) == T
    for t in range(T):
        assert r["actions"][t].tolist() == g["actions"][t, :int(g["n0"][t])].tolist(), "actions of tick %d" % t
    assert r["digest"] == g["digest"].tolist() and r["np_digest"] == g["np_digest"].tolist()
    # the calls: tick, size, uniforms -- and the tree indices the device found
    made = [(t, c) for t, c in env.reference_calls if c.kind == "learn"]
    assert [t for t, _ in made] == g["call_tick"].tolist() and [c.size for _, c in made] == g["call_size"].tolist()
    assert {c.kind for _, c in env.reference_calls} == {"learn", "store"}
    assert r["entries"] == [("rl_learn_td", int(g["batch"]), 1, 0, True)] * len(made)
    assert r["epsilon"] == g["call_epsilon"].tolist() and brains[0].epsilon == float(g["final_epsilon"])
    assert len(env.reference_choices) == len(made)
    worst_s = 0.0
    for k, (t, b, idxs, slots, points) in enumerate(env.reference_choices):
        assert (t, b) == (int(g["call_tick"][k]), 0)
        assert idxs.cpu().numpy().tolist() == g["call_idxs"][k].tolist(), "tree indices of call %d" % k
        assert slots.cpu().numpy().tolist() == memory_slots(int(g["call_stored"][k]), C, C + 64, g["call_idxs"][k] - (C - 1)).tolist()
        worst_s = max(worst_s, float(np.abs(points.cpu().numpy()[:, 0] - g["call_s"][k]).max() / g["call_total"][k]))
    print("largest |s - the reference's| / total over the run: %.3g (D of the fixture / smallest total %.3g)"
          % (worst_s, float(g["interval_err"]) / float(g["call_total"].min())))
    assert float(l.beta_is.item()) == float(g["final_beta"])
    # the bar: outputs in float64 on the fixture's states, after the first update and at the end
    bar = float(g["ref_q_spread"][0]) * (1e-5 / float(g["ref_grad_err"][0]))
    ratios = {}
    for when, got in (("first", r["first"][0]), ("final", r["final"][0])):
        ref, init = g["out_" + when][0], g["out_init"][0]
        ratios[when] = np.abs(tc.outputs64(got, g["states"]) - ref).max() / np.abs(ref - init).max()
        print("%s update: max|d out| / training effect = %.3g (bar %.3g; ratio / bar %.3g); effect %.3g"
              % (when, ratios[when], bar, ratios[when] / bar, np.abs(ref - init).max()))
    # the final leaf priorities: a priority comes from a difference of two outputs -> twice the bar, relative to the largest |q|
    qmax = max(float(np.abs(g["out_" + k][0]).max()) for k in ("init", "first", "final"))
    tree = l.ref_tree.cpu().numpy()
    live = memory_slots(int(g["final_stored"]), C, C + 64, np.arange(C))
    assert l.priority.cpu().numpy()[live].astype(np.float64).tobytes() == tree[C - 1:].tobytes()        # the invariant between calls
    prio_ratio = float(np.abs(tree[C - 1:] - g["final_leaves"]).max()) / qmax
    print("final leaf priorities: max|d p| / largest |q| = %.3g (bar %.3g; ratio / bar %.3g); largest |q| %.3g; total %.9g against %.9g"
          % (prio_ratio, 2 * bar, prio_ratio / (2 * bar), qmax, tree[0], g["final_tree"][0]))
    assert int(l.ring["count"].item()) == int(g["final_stored"]) == env.schedule.stored[0] == env.schedule.stamped[0]
    assert ratios["first"] <= bar and ratios["final"] <= bar
    assert prio_ratio <= 2 * bar
    # the acting weights are the learner's
    assert brains[0].state_dict_flat().tobytes() == r["final"][0].tobytes()
    assert not np.array_equal(r["final"][0], tc.weights(int(g["init_seeds"][0])))
    assert "learn_reference_td=True" in env._weights_note() and "brains [0] trained" in env._weights_note()
    # a memory keeps its capacity: another one on a learner that has a tree is refused, not answered with a fresh tree
    with pytest.raises(ValueError, match="built for a capacity of 64, not 65"):
        env.worlds.store_td_reference([l], [C + 1], [0], [1])
    assert l.ref_tree.cpu().numpy().tobytes() == tree.tobytes()


def test_the_run_without_the_keyword_is_what_it_was():
    """Without learn_reference_td a PERDQN brain alone is refused (nothing trains), with learn_reference_prioritized=True it stays frozen
    and named by that keyword's warning, byte for byte; with the new keyword a PERD3QN brain beside it is the one the warning names."""
    from reinlife_amd import Environment, Models
    g = tc.load()
    with pytest.raises(ValueError, match="none of the brains is of a kind that trains in this mode"):
        _run(g, tc.product_brains(g), ticks=2)
    brains = tc.product_brains(g) + [Models.PERD3QN()]
    before = brains[0].state_dict_flat().copy()
    with pytest.warns(UserWarning, match=r"learn_reference_prioritized=True trains the DQN, D3QN, PPO and PERD3QN brains.*brains 0 \(PERDQN\) are.*"
                                         r"PERDQN brains do not train in this mode yet"):
        n = _run(g, brains, ticks=int(g["first_update_tick"].min()) + 3, learn_reference_prioritized=True)
    env = n["env"]
    assert sorted(env.learners) == [1] and env.schedule.specs[0] is None and env.ring_rows[0] == 64
    assert all(c.brain == 1 for _, c in env.reference_calls) and brains[0].state_dict_flat().tobytes() == before.tobytes()
    assert brains[0].epsilon == 1.0 and not hasattr(env.learners[1], "ref_tree")
    with pytest.warns(UserWarning, match=r"learn_reference_td=True trains the DQN, D3QN, PPO and PERDQN brains.*brains 1 \(PERD3QN\) are.*"
                                         r"learn_reference_prioritized=True"):
        Environment(brains=tc.product_brains(g) + [Models.PERD3QN()], max_agents=10, print_results=False, learn="reference", learn_reference_td=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")       # both keywords: all five kinds train, nothing warns
        env = Environment(brains=tc.product_brains(g) + [Models.PERD3QN()], max_agents=10, print_results=False, learn="reference",
                          learn_reference_td=True, learn_reference_prioritized=True)
    assert [env.learners[k].entry for k in (0, 1)] == ["rl_learn_td", "rl_learn_prioritized"]
