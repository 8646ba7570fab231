"""GPU: rl_learn_prioritized / rl_learn_prioritized_draw / trainer(learn="device", learn_prioritized=True) -- PERD3QNAgent.train() and its
prioritised memory (ReinLife/Models/PERD3QN.py:94-115, 133-182) on the device, checked in pieces: the update is rl_learn_dueling's bit for
bit; the priorities it leaves are |max q'_target(s') - q(s)[a]| of float64 and of the reference's own train()
(tests/golden/learn_perd3qn.npz); rows appended since the last draw are stamped with the maximum from the `seen` counter; the draw takes
rows with probability priority^0.6 / sum, whatever slots they sit in; learners of a launch are independent and runs repeat; a bad slot is
flagged and that brain left alone; and the whole path through trainer().  Every figure a bar is held against is printed first."""
import ctypes as C
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
LR, GAMMA = 1e-3, 0.99
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
PRIO = ("priority", "prio_max")
SENTINEL = np.float32(2.0 ** -20)    # below every priority of the fixture, so that prio_max is one of the kernel's own


def _brain(cls, flat, **kw):
    import torch
    b = cls(**kw)
    with torch.no_grad():
        for p, v in zip(b.eval_net.parameters(), dc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, count=None, capacity=None):
    """A replay ring on the device from host rows (dict with ring_state, ...), as DeviceWorlds.enable_capture lays one out."""
    import torch
    capacity = rows["ring_state"].shape[0] if capacity is None else capacity
    t = lambda a, dt: torch.as_tensor(np.array(a[:capacity]), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": torch.zeros(capacity, dtype=torch.int32, device=DEV),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, target_flat, ring, n_steps=1, batch=64, want_grad=True, sync_target=False, prioritized=True, fill=SENTINEL):
    """A prioritised PERD3QN learner (or, prioritized=False, the D3QN learner it is compared with) on the fixture's networks; the
    memory starts with every priority at `fill`, nothing new to stamp (seen = count) and a maximum of 1."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    if prioritized:
        l = DeviceLearner(_brain(Models.PERD3QN, flat), DEV, ring=ring, prioritized=True)
        assert (l.lr, l.gamma, l.batch, l.min_size, l.train_freq, l.n_steps_default, l.sync_target) == (LR, GAMMA, 64, 0, 20, 1, False)
        assert (l.exploration, l.soft_update_freq, l.entry, l.alpha) == (1000, 200, "rl_learn_prioritized", 0.6)
        capacity = ring["state"].shape[0]
        assert l.priority.numel() == l.weight.numel() == l.keys.numel() == capacity and l.prio_max.item() == 1.0 and l.seen.item() == 0
        l.priority.fill_(float(fill))
        l.seen.copy_(ring["count"])
        l.batch = batch
    else:
        l = DeviceLearner(_brain(Models.D3QN, flat), DEV, ring=ring)
        l.batch, l.min_size = batch, batch - 1
    l.sync_target = sync_target
    l.target.copy_(torch.as_tensor(np.array(target_flat, np.float32), device=DEV))
    if want_grad:
        l.grad = torch.zeros((n_steps, dc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _np(l, prio=True):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in BUFFERS + (PRIO if prio else ())}


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _host_pack(flat, kind):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(kind), np.float32)
    assert lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def _batch5(g):
    """Five rows of the first minibatch: its duplicated slot twice and three others."""
    s0 = g["slots"][0]
    return s0[[0, 1, 7, 20, 41]].astype(np.int32)


# ---- 1. the same update ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [64, 33, 5])
def test_one_step_is_rl_learn_duelings_bit_for_bit(worlds, batch):
    """Explicit slots on a wrapped ring (capacity 96, count 250): gradient, loss, parameters, Adam's moments and the packed weights of
    rl_learn_prioritized are the bits rl_learn_dueling leaves on a D3QN learner with the same buffers."""
    import torch
    from reinlife_amd import _lib
    g = dc.golden()
    slots = g["slots"][0][:batch] if batch > 5 else _batch5(g)
    a = _learner(g["init"], g["target_init"], _ring(g, count=250), batch=batch)
    b = _learner(g["init"], g["target_init"], _ring(g, count=250), batch=batch, prioritized=False)
    worlds.learn([a], 1, slots=slots.reshape(1, 1, batch))
    worlds.learn([b], 1, slots=slots.reshape(1, 1, batch))
    ra, rb = _np(a), _np(b, prio=False)
    worlds.check_error_flag()
    for k in BUFFERS:
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert a.grad.cpu().numpy().tobytes() == b.grad.cpu().numpy().tobytes() and a.grad.any().item()
    assert a.loss.cpu().numpy().tobytes() == b.loss.cpu().numpy().tobytes()
    assert ra["state"].tolist() == [1, 1] and ra["params"].tobytes() != g["init"].tobytes()
    assert ra["packed"].tobytes() == _host_pack(ra["params"], _lib.PERD3QN).tobytes()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def three_calls(worlds):
    """The fixture's three minibatches as three single-step calls, once: the parameters every call started from, and the priorities,
    their maximum and every buffer after each."""
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), want_grad=False)
    out = {"before": [], "after": [], "learner": l}
    for s in range(3):
        out["before"].append(_np(l))
        worlds.learn([l], 1, slots=g["slots"][s].reshape(1, 1, 64))
        out["after"].append(_np(l))
    worlds.check_error_flag()
    return out


def test_three_single_step_calls_end_where_d3qns_three_steps_end(worlds, three_calls):
    from reinlife_amd import _lib
    g, p = dc.golden(), pc.golden()
    d = _learner(g["init"], g["target_init"], _ring(g), 3, want_grad=False, prioritized=False)
    worlds.learn([d], 3, slots=g["slots"].reshape(1, 3, 64))
    rd, last = _np(d, prio=False), three_calls["after"][2]
    worlds.check_error_flag()
    for k in ("params", "adam_m", "adam_v", "target", "packed"):
        assert last[k].tobytes() == rd[k].tobytes(), k
    assert last["state"].tolist() == [3, 3] and rd["state"].tolist() == [3, 1]
    assert last["target"].tobytes() == g["target_init"].tobytes()
    assert last["packed"].tobytes() == _host_pack(last["params"], _lib.PERD3QN).tobytes()
    print("max |params - reference final| %.3g" % np.abs(last["params"] - p["final"]).max())


# ---- 2. priorities -----------------------------------------------------------------------------------------------------------------
def test_priorities_are_the_references_expression(three_calls):
    """After each call priority[slots[s]] = |max_a q'_target(s') - q_eval(s)[a]| of the parameters the call started from: within the
    project's 1e-5 bar, relative to the largest |q|, |q'| of the batch, of float64 and of the reference's own train(); every other row
    keeps its bits; prio_max is the maximum over [0, size); the duplicated slot of step 0 holds one value."""
    g, p = dc.golden(), pc.golden()
    expect = np.full(96, SENTINEL, np.float32)
    for s in range(3):
        before, after = three_calls["before"][s], three_calls["after"][s]
        assert before["priority"].tobytes() == expect.tobytes()
        slots = g["slots"][s]
        p64, q, qn = pc.priorities(before["params"], before["target"], g, slots)
        scale = max(np.abs(q).max(), np.abs(qn).max())
        got = after["priority"][slots]
        e64, eref = np.abs(got - p64).max() / scale, np.abs(got.astype(np.float64) - p["priorities"][s]).max() / scale
        print("call %d: max |priority - float64| / scale %.3g, max |priority - reference| / scale %.3g (scale %.4g, torch float32: %.3g), prio_max %.6g"
              % (s, e64, eref, scale, float(p["ref_prio_err"]), after["prio_max"][0]))
        assert e64 <= 1e-5 and eref <= 1e-5
        expect[slots] = got
        assert after["priority"].tobytes() == expect.tobytes()                           # rows outside the batch keep their bits
        assert after["prio_max"][0] == after["priority"].max() > SENTINEL
        assert np.isfinite(got).all() and (got >= 0).all()
    assert g["slots"][0][1] == g["slots"][0][0]
    assert not np.array_equal(three_calls["after"][2]["priority"][g["slots"][0]], three_calls["after"][0]["priority"][g["slots"][0]])   # later steps overwrite


def test_later_steps_of_one_call_overwrite_earlier_ones_and_a_short_ring_keeps_its_tail(worlds, three_calls):
    """One call of three steps leaves, for every row, the priority of the LAST step that drew it (each from that step's pre-update
    parameters: the single-step calls' values); with count 70 of 96 the maximum is taken over rows [0, 70) only."""
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), 3, want_grad=False)
    worlds.learn([l], 3, slots=g["slots"].reshape(1, 3, 64))
    r = _np(l)
    worlds.check_error_flag()
    assert r["priority"].tobytes() == three_calls["after"][2]["priority"].tobytes()
    assert r["prio_max"].tobytes() == three_calls["after"][2]["prio_max"].tobytes() and r["state"].tolist() == [3, 1]
    short = _learner(g["init"], g["target_init"], _ring(g, count=70), want_grad=False, fill=0.0)
    short.priority[70:] = 9.0                                                            # (beyond the ring's size: never read)
    slots = (g["slots"][0] % 70).astype(np.int32)
    worlds.learn([short], 1, slots=slots.reshape(1, 1, 64))
    rs = _np(short)
    worlds.check_error_flag()
    assert rs["prio_max"][0] == rs["priority"][:70].max() < 9.0 and (rs["priority"][70:] == 9.0).all()


# ---- 3. stamping -------------------------------------------------------------------------------------------------------------------
def _stamp(worlds, l, count, seen=None, prio_max=None):
    import torch
    l.ring["count"].fill_(count)
    if seen is not None:
        l.seen.fill_(seen)
    if prio_max is not None:
        l.prio_max.fill_(prio_max)
    slots = worlds.draw_prioritized([l], 1)
    torch.cuda.synchronize()
    assert tuple(slots.shape) == (1, 1, 64) and int(slots.min()) >= 0 and int(slots.max()) < min(count, 96)
    return l.priority.cpu().numpy(), int(l.seen.item())


def test_rows_appended_since_the_last_draw_get_the_maximum(worlds):
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), want_grad=False)
    s = float(SENTINEL)
    p, seen = _stamp(worlds, l, count=40, seen=0)                                        # a ring that is filling: rows 0..39
    assert (p[:40] == 1.0).all() and (p[40:] == s).all() and seen == 40
    assert np.abs(l.weight.cpu().numpy()[:40] - 1.0).max() <= 1e-6
    p, seen = _stamp(worlds, l, count=70, prio_max=2.5)                                  # 30 more at another maximum
    assert (p[:40] == 1.0).all() and (p[40:70] == 2.5).all() and (p[70:] == s).all() and seen == 70
    w = l.weight.cpu().numpy()
    assert np.abs(w[40:70] - 2.5 ** 0.6).max() <= 1e-6 and np.abs(w[:40] - 1.0).max() <= 1e-6
    p, seen = _stamp(worlds, l, count=70)                                                # nothing new: nothing stamped
    assert (p[:40] == 1.0).all() and (p[40:70] == 2.5).all() and (p[70:] == s).all() and seen == 70
    m = _learner(g["init"], g["target_init"], _ring(g), want_grad=False)
    p, seen = _stamp(worlds, m, count=110, seen=90, prio_max=3.0)                        # through the wrap: slots 90..95 and 0..13
    assert (p[90:] == 3.0).all() and (p[:14] == 3.0).all() and (p[14:90] == s).all() and seen == 110
    p, seen = _stamp(worlds, m, count=110 + 96, prio_max=4.0)                            # a whole capacity of new rows: all of them
    assert (p == 4.0).all() and seen == 206
    p, seen = _stamp(worlds, m, count=1000, seen=10, prio_max=5.0)                       # more than a capacity
    assert (p == 5.0).all() and seen == 1000
    worlds.check_error_flag()
    assert m.prio_max.item() == 5.0                                                      # (the draw reads the maximum, never writes it)


# ---- 4. the weighted draw ----------------------------------------------------------------------------------------------------------
def _counts(worlds, l, pri, n_steps=100):
    import torch
    l.priority.copy_(torch.as_tensor(np.asarray(pri, np.float32), device=DEV))
    slots = worlds.draw_prioritized([l], n_steps).cpu().numpy()
    assert slots.shape == (1, n_steps, 64) and slots.min() >= 0 and slots.max() < len(pri)
    return np.bincount(slots.reshape(-1), minlength=len(pri))


def test_rows_are_drawn_with_probability_priority_to_the_alpha_over_the_sum(worlds):
    """48 rows, priorities cycling through {0, 0.25, 1, 4}, 6,400 draws: a zero-priority row is never drawn, every other row's count lies
    within 5 binomial standard deviations of 6400 w / sum w, w = p^0.6 (deterministic: this passes always or never).  A uniform draw
    fails: the 0.25 and 4 classes expect 62 and 328 draws a row."""
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g, capacity=48), want_grad=False)
    n = 6400
    pri = np.tile(np.array([0.0, 0.25, 1.0, 4.0]), 12)
    counts = _counts(worlds, l, pri)
    w = pri ** 0.6
    prob = w / w.sum()
    sd = np.sqrt(n * prob * (1 - prob))
    z = np.abs(counts - n * prob)[pri > 0] / sd[pri > 0]
    print("weighted: counts by class %s, expected %s, worst deviation %.2f sd" % (
        [int(counts[pri == v].sum()) for v in (0.0, 0.25, 1.0, 4.0)], [round(float(n * prob[pri == v].sum()), 1) for v in (0.0, 0.25, 1.0, 4.0)], z.max()))
    assert counts.sum() == n and not counts[pri == 0].any()
    assert (z <= 5).all()
    lo, hi = n * prob[1], n * prob[3]
    assert hi - lo > 10 * (sd[1] + sd[3])                                                # (the case tells a uniform draw apart)
    one = np.zeros(48)
    one[29] = 0.003
    assert _counts(worlds, l, one, 4)[29] == 256                                         # one row with a weight: every draw takes it
    flat = _counts(worlds, l, np.zeros(48))                                              # no weight anywhere: the uniform content-key draw
    zu = np.abs(flat - n / 48) / np.sqrt(n * (1 / 48) * (47 / 48))
    print("all zero: worst deviation from uniform %.2f sd" % zu.max())
    assert flat.sum() == n and (zu <= 5).all()
    worlds.check_error_flag()


# ---- 5. order independence ---------------------------------------------------------------------------------------------------------
def test_draws_and_training_do_not_depend_on_the_order_of_the_ring(worlds):
    import torch
    g = dc.golden()
    perm = np.random.RandomState(4).permutation(96)
    rows2 = {k: np.ascontiguousarray(g[k][perm]) for k in dc.RING_KEYS}
    pri = (np.random.RandomState(5).random_sample(96) ** 3 * 4).astype(np.float32)
    pri[::7] = 0.0

    def pair():
        a, b = _learner(g["init"], g["target_init"], _ring(g), 2, want_grad=False), _learner(g["init"], g["target_init"], _ring(rows2), 2, want_grad=False)
        a.priority.copy_(torch.as_tensor(pri, device=DEV))
        b.priority.copy_(torch.as_tensor(pri[perm], device=DEV))                          # slot j of the permuted ring holds row perm[j]
        return a, b
    a, b = pair()
    sa, sb = worlds.draw_prioritized([a], 2), worlds.draw_prioritized([b], 2)
    both = worlds.draw_prioritized([a, b], 2)
    torch.cuda.synchronize()
    assert tuple(sa.shape) == (1, 2, 64) and sa.dtype == torch.int32 and tuple(both.shape) == (2, 2, 64)
    assert torch.equal(both[0:1], sa) and not torch.equal(both[1:2], sb)                 # (the brain index salts the draw)
    sa, sb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert not np.array_equal(sa, sb) and np.array_equal(perm[sb], sa)
    assert (pri[sa] > 0).all() and 10 < len(np.unique(sa)) < 128
    worlds.learn([a], 2, slots=torch.as_tensor(sa.reshape(1, 2, 64), device=DEV))
    worlds.learn([b], 2, slots=torch.as_tensor(sb.reshape(1, 2, 64), device=DEV))
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    for k in BUFFERS + ("prio_max",):
        assert ra[k].tobytes() == rb[k].tobytes(), k
    assert ra["priority"][perm].tobytes() == rb["priority"].tobytes() and ra["priority"].tobytes() != pri.tobytes()
    assert ra["state"].tolist() == [2, 1]
    # a later call draws other rows from the same priorities
    c, _ = pair()
    c.state[1] = 1
    sc = worlds.draw_prioritized([c], 2).cpu().numpy().reshape(-1)
    assert not np.array_equal(sc, sa) and (pri[sc] > 0).all()


# ---- 6. independence and repeatability ---------------------------------------------------------------------------------------------
def _second_case(g):
    rows = {k: np.ascontiguousarray(g[k][::-1]) for k in dc.RING_KEYS}
    rows["ring_reward"] = (rows["ring_reward"] * np.float32(0.5)).astype(np.float32)
    return (g["init"] * np.float32(0.75)).astype(np.float32), rows, np.ascontiguousarray(g["slots"][::-1])


def test_learners_of_a_launch_are_independent_and_runs_repeat(worlds):
    g = dc.golden()
    init2, rows2, slots2 = _second_case(g)
    both = np.stack([g["slots"], slots2]).astype(np.int32)

    def pair():
        return (_learner(g["init"], g["target_init"], _ring(g), 3, want_grad=False),
                _learner(init2, g["target_init"], _ring(rows2), 3, want_grad=False, sync_target=True))
    a, b = pair()
    worlds.learn([a, b], 3, slots=both)
    ra, rb = _np(a), _np(b)
    sa, sb = pair()
    worlds.learn([sa], 3, slots=both[0:1])
    worlds.learn([sb], 3, slots=both[1:2])
    rsa, rsb = _np(sa), _np(sb)
    a2, b2 = pair()
    worlds.learn([b2, a2], 3, slots=both[::-1].copy())   # (the other order, again from the same initial buffers)
    ra2, rb2 = _np(a2), _np(b2)
    a3, b3 = pair()
    worlds.learn([a3, b3], 3, slots=both)                 # (a second run)
    ra3, rb3 = _np(a3), _np(b3)
    worlds.check_error_flag()
    for k in BUFFERS + PRIO:
        assert ra[k].tobytes() == rsa[k].tobytes() == ra2[k].tobytes() == ra3[k].tobytes(), k
        assert rb[k].tobytes() == rsb[k].tobytes() == rb2[k].tobytes() == rb3[k].tobytes(), k
    assert ra["params"].tobytes() != rb["params"].tobytes() and ra["state"].tolist() == [3, 1]
    assert ra["priority"].tobytes() != rb["priority"].tobytes() and rb["target"].tobytes() == rb["params"].tobytes()


# ---- 7. a bad slot -----------------------------------------------------------------------------------------------------------------
def test_a_bad_slot_is_flagged_and_that_brain_is_left_alone(worlds):
    """A slot equal to the ring's size: error-flag code 6 with the brain's index, the step and the value; nothing of that brain -- its
    priorities and prio_max included -- is written; the other learner trains."""
    import torch
    g = dc.golden()
    init2, rows2, slots2 = _second_case(g)
    bad = g["slots"].copy()
    bad[2, 40] = 96
    a, b = _learner(g["init"], g["target_init"], _ring(g), 3, sync_target=True), _learner(init2, g["target_init"], _ring(rows2), 3)
    before = _np(a)
    worlds.learn([a, b], 3, slots=np.stack([bad, slots2]).astype(np.int32))
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 2, 96]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    after = _np(a)
    for k in BUFFERS + PRIO:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert not a.grad.any().item() and after["prio_max"][0] == 1.0 and (after["priority"] == SENTINEL).all()
    solo = _learner(init2, g["target_init"], _ring(rows2), 3)
    worlds.learn([solo], 3, slots=slots2.reshape(1, 3, 64).astype(np.int32))
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [3, 1]
    for k in BUFFERS + PRIO:
        assert rb[k].tobytes() == rs[k].tobytes(), k


def test_the_python_layer_refuses_what_the_entry_points_cannot_do(worlds):
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    g = dc.golden()
    p = _learner(g["init"], g["target_init"], _ring(g), want_grad=False)
    d3 = _learner(g["init"], g["target_init"], _ring(g), want_grad=False, prioritized=False)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([d3, p], 1, slots=g["slots"][:1].reshape(1, 1, 64).repeat(2, 0))
    with pytest.raises(_lib.ReinLifeHipError, match="rl_learn_prioritized_draw"):
        worlds.learn([p], 1)                                                             # no slots: the draw is draw_prioritized()'s job
    with pytest.raises(ValueError, match="prioritised"):
        worlds.draw_prioritized([d3], 1)
    with pytest.raises(ValueError, match="no entry point trains PERD3QN"):
        DeviceLearner(Models.PERD3QN(), DEV, ring=_ring(g))                              # without prioritized=True: what it always raised
    with pytest.raises(ValueError, match="prioritized=True is for PERD3QN"):
        DeviceLearner(Models.D3QN(), DEV, ring=_ring(g), prioritized=True)
    with pytest.raises(_lib.ReinLifeHipError, match="kind 2"):
        d3.kind = _lib.PERD3QN                                                           # rl_learn_dueling still refuses the kind
        worlds.learn([d3], 1, slots=g["slots"][:1].reshape(1, 1, 64))
    worlds.check_error_flag()


# ---- 8. trainer() ------------------------------------------------------------------------------------------------------------------
def _train(learn_prioritized, n_episodes=60, **perd3qn):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.PERD3QN(exploration=20, soft_update_freq=40, **perd3qn)]
    init = [b.state_dict_flat().copy() for b in brains]
    kw = {"learn_prioritized": True} if learn_prioritized else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=n_episodes, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      save=False, print_results=False, **kw)
    return env, brains, init


def test_trainer_learn_prioritized_trains_the_perd3qn_on_its_schedule():
    """exploration 20, soft_update_freq 40, learn_every 20: the PERD3QN trains after episodes 40 and 60 (PERD3QN.py:120 asks
    n_epi > exploration) and its target is synced at 40 alone."""
    from reinlife_amd import _lib
    env, brains, init = _train(True)
    assert sorted(env.learners) == [0, 1] and env.learn_every == 20
    l = env.learners[1]
    count, capacity = int(env.worlds.replays[1]["count"].item()), env.worlds.replays[1]["state"].shape[0]
    pri, pmax, seen = l.priority.cpu().numpy(), float(l.prio_max.item()), int(l.seen.item())
    print("PERD3QN: state %s, ring count %d of %d, seen %d, prio_max %.6g, priorities below the maximum among the seen rows: %d"
          % (l.state.cpu().tolist(), count, capacity, seen, pmax, int((pri[:seen] != pmax).sum())))
    assert l.entry == "rl_learn_prioritized" and l.state.cpu().tolist() == [2, 2]
    assert capacity == brains[1].capacity == 10000 and 64 <= count < 10000              # (no wrap: the rows do not depend on append order)
    assert env.worlds.replays[0]["state"].shape[0] == 50000
    assert 0 < seen <= count and pmax == pri[:count].max()
    assert (pri[:seen] != pmax).any() and (pri[:seen] > 0).all() and not pri[count:].any()   # some rows were drawn and re-prioritised
    now, target = brains[1].state_dict_flat(), l.target.cpu().numpy()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1])
    assert now.tobytes() == l.params.cpu().numpy().tobytes()
    assert not np.array_equal(target, init[1]) and not np.array_equal(target, now)       # synced at 40, not at 60
    assert np.array_equal(np.concatenate([p.detach().numpy().reshape(-1) for p in brains[1].target_net.state_dict().values()]), target)
    assert env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()                    # what the worlds acted with
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now, _lib.PERD3QN).tobytes()
    assert not np.array_equal(brains[0].state_dict_flat(), init[0])                       # the DQN learned too
    assert "rl_learn_prioritized" in env._weights_note() and "rl_learn:" in env._weights_note()
    # a second identical call: the same bits
    env2, brains2, _ = _train(True)
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    assert np.sort(env2.learners[1].priority.cpu().numpy()).tobytes() == np.sort(pri).tobytes()   # (the rows' slots may differ, their priorities do not)
    # without the keyword the PERD3QN stays as it was
    env0, brains0, init0 = _train(False)
    assert sorted(env0.learners) == [0] and brains0[1].state_dict_flat().tobytes() == init0[1].tobytes()
    assert not np.array_equal(brains0[0].state_dict_flat(), init0[0])


def test_the_dqn_learner_is_bit_for_bit_what_it_is_without_the_keyword():
    """The DQN learner's calls and draws do not depend on the keyword: its Philox index, ring, period and steps are the same.  After the 60
    episodes of the test above the two runs cannot be compared -- the PERD3QN acts on its trained weights from episode 41 on, so the
    shared worlds, and with them the rows of the DQN's ring, part company.  Up to and including episode 40 they must agree: the DQN
    trains after episodes 20 and 40, the PERD3QN for the first time after 40 and BEHIND the DQN's call, so runs that end there hold the
    same DQN learner bit for bit, with and without the keyword -- also when the PERD3QN asks for a shorter train_freq, which does not
    set the period while other learners are there."""
    env, brains, _ = _train(True, 40)
    env0, brains0, init0 = _train(False, 40)
    env10, brains10, _ = _train(True, 40, train_freq=10)
    assert env.learn_every == env0.learn_every == env10.learn_every == 20
    assert env.learners[1].state.cpu().tolist() == [1, 1] == env10.learners[1].state.cpu().tolist() and sorted(env0.learners) == [0]
    for e, b in ((env, brains), (env10, brains10)):
        for k in BUFFERS:
            assert getattr(e.learners[0], k).cpu().numpy().tobytes() == getattr(env0.learners[0], k).cpu().numpy().tobytes(), k
        assert b[0].state_dict_flat().tobytes() == brains0[0].state_dict_flat().tobytes()
        assert e.tracker.results == env0.tracker.results
        assert int(e.worlds.replays[0]["count"].item()) == int(env0.worlds.replays[0]["count"].item())
    st = env0.learners[0].state.cpu().tolist()
    assert st[1] == 2 and st[0] >= 5 and not np.array_equal(brains0[0].state_dict_flat(), init0[0])
    assert not np.array_equal(brains[1].state_dict_flat(), brains0[1].state_dict_flat())   # (the PERD3QN did train after episode 40)


def test_a_call_below_the_size_gate_leaves_the_memory_alone(worlds):
    """size <= min_size (a caller's own gate; Python passes 0): the call is counted and nothing else changes -- no priority, and not the
    maximum, which is retaken only by a call that trained."""
    g = dc.golden()
    l = _learner(g["init"], g["target_init"], _ring(g), want_grad=False)
    l.min_size = 96
    l.prio_max.fill_(3.5)
    before = _np(l)
    worlds.learn([l], 1, slots=g["slots"][0].reshape(1, 1, 64))
    after = _np(l)
    worlds.check_error_flag()
    for k in ("params", "target", "adam_m", "adam_v", "packed") + PRIO:
        assert after[k].tobytes() == before[k].tobytes(), k
    assert after["state"].tolist() == [0, 1] and after["prio_max"][0] == 3.5
