"""CPU: the host side of on-device PERDQN learning -- rl_learn_td / rl_learn_td_draw / rl_learn_td_supported are exported and validate
their arguments without a GPU, the fixture tests/golden/learn_perdqn.npz (the reference's own train_model(), append_sample and Memory,
tools/gen_golden_learn_perdqn.py) is what a torch restatement of ReinLife/Models/PERDQN.py makes of its inputs (parameters, priorities,
importance weights, beta, epsilon), the reference's memory stores one priority whatever the row, and learn_td_priority /
DeviceLearner(td_priority=True) refuse what they cannot do before they touch a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc
import learn_perdqn_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
ENTRIES = ("rl_learn_td", "rl_learn_td_draw")


def test_the_three_symbols_are_exported_and_supported_for_perdqn_alone():
    lib = _lib.lib()
    for name in ENTRIES + ("rl_learn_td_supported",):
        assert hasattr(lib, name), name
    assert [lib.rl_learn_td_supported(k) for k in KINDS] == [0, 0, 0, 0, 1]
    assert lib.rl_learn_td_supported(-1) == 0 and lib.rl_learn_td_supported(9) == 0
    assert [lib.rl_learn_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]            # (the older contracts are what they were)
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert [lib.rl_learn_prioritized_supported(k) for k in KINDS] == [0, 0, 1, 0, 0]
    assert [lib.rl_learn_ppo_supported(k) for k in KINDS] == [0, 0, 0, 1, 0]
    assert (_lib.SITE_LEARN, _lib.SITE_LEARN_PRIO, _lib.SITE_LEARN_ROLLOUT, _lib.SITE_LEARN_TD) == (10, 11, 12, 13)
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "RL_SITE_LEARN_TD = 13" in hdr and "int rl_learn_td(" in hdr and "int rl_learn_td_draw(" in hdr and "} rl_tdprio;" in hdr
    assert C.sizeof(_lib.TdPrio) == 64                                                # four pointers, three floats + padding, a double, a pointer
    assert _lib.TdPrio.beta_increment.offset == 48 and _lib.TdPrio.p_new.offset == 32


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, td=None, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.PERDQN, p, p, p, p, p, p, 0.001, 0.99, 0.9, 0.999, 1e-8, 64, 999, 1, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    ts = (_lib.TdPrio * n)(*[_lib.TdPrio(p, p, p, p, 0.0630957335, 0.01, 0.6, 0.001, None) for _ in range(n)])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    for k, v in (td or {}).items():
        setattr(ts[n - 1], k, v)
    return ls, rs, ts


def _call(name, h, ls, rs, ts, n=1, n_steps=1, slots=C.c_void_p(0x1000)):
    lib = _lib.lib()
    rc = getattr(lib, name)(h, ls, rs, ts, n, n_steps, slots, None)
    return rc, lib.rl_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_handles_counts_kinds_and_rings_are_refused_by_name(name):
    lib, h = _lib.lib(), _handle()
    ls, rs, ts = _args()
    rc, err = _call(name, None, ls, rs, ts)
    assert rc == -1 and err == (name + ": null handle").encode()
    for bad in ((None, rs, ts), (ls, None, ts), (ls, rs, None)):
        rc, err = _call(name, h, *bad)
        assert rc == -1 and err.startswith(name.encode() + b":") and b"null learners / rings / tds" in err
    rc, err = _call(name, h, ls, rs, ts, n_steps=0)
    assert rc == -1 and b"n_steps" in err
    rc, err = _call(name, h, ls, rs, ts, n=0)
    assert rc == -1 and b"n_learners" in err
    rc, err = _call(name, h, *_args(17), n=17)
    assert rc == -1 and b"n_learners" in err and b"16" in err
    for batch in (0, 65):
        rc, err = _call(name, h, *_args(batch=batch))
        assert rc == -1 and b"batch" in err and b"[1,64]" in err, batch
    for kind in (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, 7):
        rc, err = _call(name, h, *_args(2, kind=kind), n=2)
        assert rc == -4, kind                                                          # RL_E_UNSUPPORTED
        assert ("kind %d" % kind).encode() in err and b"learner 1" in err and err.startswith(name.encode() + b":")
    rc, err = _call(name, h, ls, rs, ts, slots=None)
    assert rc == -1 and b"slots" in err and b"null" in err
    ls, rs, ts = _args()
    rs[0].reward = None
    rc, err = _call(name, h, ls, rs, ts)
    assert rc == -1 and b"replay 0" in err
    lib.rl_destroy(h)


def test_rl_learn_td_names_the_draw_when_it_is_given_no_slots_and_checks_the_learners_buffers():
    lib, h = _lib.lib(), _handle()
    rc, err = _call("rl_learn_td", h, *_args(), slots=None)
    assert rc == -1 and b"rl_learn_td_draw" in err
    for field in ("params", "target", "adam_m", "adam_v", "state", "packed"):
        rc, err = _call("rl_learn_td", h, *_args(**{field: None}))
        assert rc == -1 and b"learner 0" in err and b"null" in err, field
    rc, err = _call("rl_learn_td_draw", h, *_args(state=None))
    assert rc == -1 and b"state" in err
    lib.rl_destroy(h)


@pytest.mark.parametrize("name, fields", [("rl_learn_td", ("priority", "seen", "beta")), ("rl_learn_td_draw", ("priority", "keys", "seen"))])
def test_null_memory_buffers_are_refused(name, fields):
    lib, h = _lib.lib(), _handle()
    for field in fields:
        rc, err = _call(name, h, *_args(2, td={field: None}), n=2)
        assert rc == -1 and err.startswith(name.encode() + b":") and b"td 1" in err and b"null" in err and field.encode() in err, field
    if name == "rl_learn_td_draw":   # ... and the ring's age column, which the content keys read
        ls, rs, ts = _args()
        rs[0].age = None
        rc, err = _call(name, h, ls, rs, ts)
        assert rc == -1 and b"replay 0" in err and b"age" in err
    lib.rl_destroy(h)


@pytest.mark.parametrize("a", [0.0, -0.6, float("nan")])
def test_prio_a_must_be_positive(a):
    lib, h = _lib.lib(), _handle()
    rc, err = _call("rl_learn_td", h, *_args(td={"prio_a": a}))
    assert rc == -1 and b"prio_a" in err and b"td 0" in err
    lib.rl_destroy(h)


def test_the_fixture_is_what_the_torch_restatement_makes_of_its_inputs():
    """final under the bar of test_three_steps_match_the_reference_end_to_end (the reference's float32 spread scaled by how much looser
    the project's 1e-5 gradient bar is than torch's float32 gradient error), the priorities, the importance weights (equal after
    rounding to float32), beta and epsilon."""
    g, p = dc.golden(), tc.golden()
    assert p["init"].size == tc.N_PARAMS == 14536 and p["final"].size == tc.N_PARAMS and np.array_equal(p["slots"], g["slots"])
    assert p["priorities"].shape == p["errors"].shape == p["is_weights"].shape == (3, 64) and p["prio_init"].shape == (96,)
    assert float(p["p_new"]) == float((torch.zeros(()) + 0.01) ** 0.6) and p["p_new"].dtype == np.float32
    assert abs(float(p["p_new"]) - 0.06309573) < 1e-8
    assert (p["prio_init"] == p["p_new"]).sum() == 64 and len(set(p["prio_init"].tolist())) > 20     # unequal priorities
    assert (p["is_weights"].mean(1) < 0.9).all()                                                     # mean(w) != 1: the factor matters
    torch.set_num_threads(1)
    final, prios, ws, betas = tc.torch_steps(p, g)
    q_ref, q_got, q_init = tc.q_values(p["final"], g["ring_state"]), tc.q_values(final, g["ring_state"]), tc.q_values(p["init"], g["ring_state"])
    effect = np.abs(q_ref - q_init).max()
    ratio, bar = np.abs(q_got - q_ref).max() / effect, float(p["ref_q_spread"]) * (1e-5 / float(p["ref_grad_err"]))
    print("restatement: max|dQ| / training effect %.3g (bar %.3g); effect %.4g (recorded %.4g); max |p - final| %.3g"
          % (ratio, bar, effect, float(p["effect"]), np.abs(final - p["final"]).max()))
    assert 1e-9 < float(p["ref_grad_err"]) < 1e-6 and abs(effect - float(p["effect"])) <= 1e-9 and ratio <= bar
    # the mean(w) factor scales the loss and every gradient (Adam is nearly scale-free, so the end-to-end bar above cannot see it)
    loss_w, grads_w = tc.step(p["init"], p["target_init"], g, p["slots"][0], p["is_weights"][0], float(p["gamma"]))[:2]
    loss_1, grads_1 = tc.step(p["init"], p["target_init"], g, p["slots"][0], np.ones(64), float(p["gamma"]))[:2]
    mw = p["is_weights"][0].mean()
    assert abs(loss_w - mw * loss_1) <= 1e-12 * abs(loss_1) and all(np.abs(a - mw * b).max() <= 1e-12 * np.abs(b).max() for a, b in zip(grads_w, grads_1))
    # priorities: the float32 restatement reproduces the recorded ones to float32 rounding of the forward passes
    for s in range(3):
        scale = np.abs(p["errors"][s]).max()
        worst = np.abs(prios[s].astype(np.float64) - p["priorities"][s]).max()
        print("call %d: max |priority - recorded| %.3g (largest error %.4g)" % (s, worst, scale))
        assert worst <= 3.8e-5 * scale + 4 * np.spacing(np.float32(p["priorities"][s].max()))
        again = [(np.abs(x) + float(p["prio_e"])) ** float(p["prio_a"]) for x in p["errors"][s]]   # Memory._get_priority, scalar by scalar
        assert all(type(x) is np.float32 for x in again) and np.array(again).tobytes() == p["priorities"][s].tobytes()   # float32 arithmetic
    assert p["priorities"][0][1] == p["priorities"][0][0]                                            # slots[0][1] repeats slots[0][0]
    # is_weights: (p / p_min) ** -beta is the reference's (n p / total) ** -beta / max after rounding to float32 -- on the recorded priorities
    prio = p["prio_init"].copy()
    for s in range(3):
        idx = p["slots"][s].astype(np.int64)
        w = tc.is_weights(prio[idx], p["beta"][s])
        assert w.astype(np.float32).tobytes() == p["is_weights"][s].astype(np.float32).tobytes(), s
        prio[idx] = p["priorities"][s]
    # beta by repeated addition in double, epsilon by repeated subtraction
    b, e = float(p["beta0"]), 1.0
    assert e == p["epsilon"][0]
    for s in range(3):
        b = min(1.0, b + float(p["beta_increment"]))
        if e > float(p["epsilon_min"]):
            e -= float(p["epsilon_decay"])
        assert b == p["beta"][s] == betas[s] and e == p["epsilon"][s + 1], s


def test_the_reference_memory_stores_one_priority_whatever_the_row():
    """5 append_sample calls, update(1, 0.5), update(3, 2.0), 6 more append_sample calls through the wrap of a capacity-8 Memory: every
    store writes p_new; the host restatement of the device's stamp gives the same leaves; sample()'s is_weight is (p / p_min) ** -beta."""
    p = tc.golden()
    trace, (first, second) = p["mem_trace"], p["mem_stores"]
    cap = trace.shape[1]
    assert trace.shape == (first + 2 + second, 8) and first + second > cap
    p_new = p["p_new"]
    mine, seen, count = np.zeros(cap, np.float32), 0, 0
    e = 0
    for _ in range(first):
        count += 1
        mine = tc.stamp(mine, seen, count, p_new); seen = count
        assert mine.tobytes() == trace[e].tobytes() and trace[e][count - 1] == p_new, e
        e += 1
    for i, err in zip(p["mem_update_idx"], p["mem_update_err"]):
        mine[i] = (np.float32(err) + np.float32(p["prio_e"])) ** np.float32(p["prio_a"])
        assert mine.tobytes() == trace[e].tobytes(), e
        e += 1
    for _ in range(second):
        count += 1
        mine = tc.stamp(mine, seen, count, p_new); seen = count
        assert mine.tobytes() == trace[e].tobytes() and trace[e][(count - 1) % cap] == p_new, e
        e += 1
    assert (trace[-1] == p_new).sum() == cap - 1 and trace[-1][3] != p_new       # the wrap overwrote row 1's update, not row 3's
    # stamping once, after all six stores, gives what stamping after every store gave
    late = trace[first + 1].copy()
    assert tc.stamp(late, first, first + second, p_new).tobytes() == trace[-1].tobytes()
    assert (tc.stamp(late, 0, 3 * cap, p_new) == p_new).all()
    b = float(p["beta0"])
    for s in range(3):
        b = min(1.0, b + float(p["beta_increment"]))
        assert b == p["mem_beta"][s]
        w = tc.is_weights(p["mem_sample_prio"][s], b)
        assert w.astype(np.float32).tobytes() == p["mem_is_weight"][s].astype(np.float32).tobytes()
    assert len(set(p["mem_is_weight"].reshape(-1).tolist())) > 1


@pytest.mark.parametrize("brains, kwargs, says", [
    (lambda: [Models.DQN(max_epi=60), Models.PERDQN()], dict(learn_td_priority=True), "learn_td_priority=True needs learn='device'"),
    (lambda: [Models.DQN(max_epi=60), Models.D3QN()], dict(learn="device", learn_td_priority=True), "needs at least one Models.PERDQN"),
    (lambda: [Models.DQN(max_epi=60), Models.PERDQN()], dict(learn="device", learn_td_priority=False), "learn_td_priority must be None or True"),
])
def test_learn_td_priority_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(brains(), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


@pytest.mark.parametrize("brain, kwargs, says", [
    (lambda: Models.DQN(max_epi=60), dict(td_priority=True), "td_priority=True is for PERDQN brains"),
    (lambda: Models.PERD3QN(), dict(td_priority=True), "td_priority=True is for PERDQN brains"),
    (lambda: Models.PERDQN(), dict(td_priority=True, prioritized=True), "with prioritized=True"),
    (lambda: Models.PERDQN(), dict(td_priority=True, rollout=True), "with rollout=True"),
    (lambda: Models.PERDQN(), dict(), "no entry point trains PERDQN brains"),
])
def test_device_learner_refuses_what_td_priority_is_not_for(brain, kwargs, says, monkeypatch):
    from reinlife_amd.learn import DeviceLearner
    b = brain()
    monkeypatch.setattr(torch, "as_tensor", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        DeviceLearner(b, "cuda:0", **kwargs)


def test_the_older_switches_answer_what_they_answered():
    from reinlife_amd.learn import ENTRY_BY_METHOD, entry_of
    assert ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}
    assert entry_of(_lib.PERDQN) is None and entry_of(_lib.DQN) == "rl_learn"


def test_the_race_on_content_keys_draws_in_proportion_to_the_priorities():
    """rl_learn_td_draw's pick restated on the host with the seed and the priorities tests/test_hip_learn_perdqn.py uses on the device:
    48 fixture rows, edge_priorities-style weights (several orders of magnitude, every 7th row 0), 6,400 draws -- no zero-priority row,
    every other count within 5 binomial standard deviations of 6400 p / sum p; a uniform draw would fail."""
    g = dc.golden()
    keys = pc.content_keys(g, 48)
    n = 6400
    pri = pc.edge_priorities(48)
    counts = np.bincount(np.concatenate([tc.host_draw(keys, pri, 11, 0, c, 256) for c in range(25)]), minlength=48)   # the device test's 25 calls
    prob = pri.astype(np.float64) / pri.astype(np.float64).sum()
    sd = np.sqrt(n * prob * (1 - prob))
    z = np.abs(counts - n * prob)[pri > 0] / sd[pri > 0]
    print("weighted: worst deviation %.2f sd" % z.max())
    assert not counts[pri == 0].any() and (z <= 5).all()
    zu = np.abs(counts - n / 48) / np.sqrt(n * (1 / 48) * (47 / 48))
    assert zu.max() > 20                                                             # far from uniform
