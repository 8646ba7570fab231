"""CPU: the host side of on-device PERD3QN learning -- rl_learn_prioritized / rl_learn_prioritized_draw / rl_learn_prioritized_supported are
exported and validate their arguments without a GPU, the fixture tests/golden/learn_perd3qn.npz (the reference's own train() and
PrioritizedReplayBuffer, tools/gen_golden_learn_perd3qn.py) is what a torch restatement of ReinLife/Models/PERD3QN.py:94-115 makes of
its inputs, the host model of the memory the device keeps (stamping from a `seen` counter, the maximum, p = priority^alpha / sum)
reproduces the reference buffer's trace, and learn_prioritized refuses what it cannot do before it touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
ENTRIES = ("rl_learn_prioritized", "rl_learn_prioritized_draw")


def test_the_three_symbols_are_exported_and_supported_for_perd3qn_alone():
    lib = _lib.lib()
    for name in ENTRIES + ("rl_learn_prioritized_supported",):
        assert hasattr(lib, name), name
    assert [lib.rl_learn_prioritized_supported(k) for k in KINDS] == [0, 0, 1, 0, 0]
    assert lib.rl_learn_prioritized_supported(-1) == 0 and lib.rl_learn_prioritized_supported(9) == 0
    assert [lib.rl_learn_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]            # (the older contracts are what they were)
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert _lib.SITE_LEARN_PRIO == 11 and _lib.SITE_LEARN == 10
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "RL_SITE_LEARN_PRIO = 11" in hdr and "int rl_learn_prioritized(" in hdr and "int rl_learn_prioritized_draw(" in hdr
    assert "PERD3QN.py:94-115" in hdr and "PERD3QN.py:110-111" in hdr and "NO importance-weighted loss" in hdr
    assert "with an importance-weighted loss" not in hdr                            # (what the header used to say of the reference)
    assert C.sizeof(_lib.Prio) == 48                                                  # five pointers, a float, padding


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, prio=None, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.PERD3QN, p, p, p, p, p, p, 0.001, 0.99, 0.9, 0.999, 1e-8, 64, 0, 0, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    ps = (_lib.Prio * n)(*[_lib.Prio(p, p, p, p, p, 0.6) for _ in range(n)])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    for k, v in (prio or {}).items():
        setattr(ps[n - 1], k, v)
    return ls, rs, ps


def _call(name, h, ls, rs, ps, n=1, n_steps=1, slots=C.c_void_p(0x1000)):
    lib = _lib.lib()
    rc = getattr(lib, name)(h, ls, rs, ps, n, n_steps, slots, None)
    return rc, lib.rl_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_handles_counts_kinds_and_rings_are_refused_by_name(name):
    lib, h = _lib.lib(), _handle()
    ls, rs, ps = _args()
    rc, err = _call(name, None, ls, rs, ps)
    assert rc == -1 and err == (name + ": null handle").encode()
    for bad in ((None, rs, ps), (ls, None, ps), (ls, rs, None)):
        rc, err = _call(name, h, *bad)
        assert rc == -1 and err.startswith(name.encode() + b":") and b"null learners / rings / prios" in err
    rc, err = _call(name, h, ls, rs, ps, n_steps=0)
    assert rc == -1 and b"n_steps" in err
    rc, err = _call(name, h, ls, rs, ps, n=0)
    assert rc == -1 and b"n_learners" in err
    rc, err = _call(name, h, *_args(17), n=17)
    assert rc == -1 and b"n_learners" in err and b"16" in err
    for batch in (0, 65):
        rc, err = _call(name, h, *_args(batch=batch))
        assert rc == -1 and b"batch" in err and b"[1,64]" in err, batch
    for kind in (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERDQN, 7):
        rc, err = _call(name, h, *_args(2, kind=kind), n=2)
        assert rc == -4, kind                                                          # RL_E_UNSUPPORTED
        assert ("kind %d" % kind).encode() in err and b"learner 1" in err and err.startswith(name.encode() + b":")
    rc, err = _call(name, h, ls, rs, ps, slots=None)
    assert rc == -1 and b"slots" in err and b"null" in err
    ls, rs, ps = _args()
    rs[0].reward = None
    rc, err = _call(name, h, ls, rs, ps)
    assert rc == -1 and b"replay 0" in err
    lib.rl_destroy(h)


def test_rl_learn_prioritized_names_the_draw_when_it_is_given_no_slots():
    lib, h = _lib.lib(), _handle()
    rc, err = _call("rl_learn_prioritized", h, *_args(), slots=None)
    assert rc == -1 and b"rl_learn_prioritized_draw" in err
    lib.rl_destroy(h)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("field", ["priority", "prio_max", "seen"])
def test_null_priority_buffers_are_refused(name, field):
    lib, h = _lib.lib(), _handle()
    rc, err = _call(name, h, *_args(2, prio={field: None}), n=2)
    assert rc == -1 and err.startswith(name.encode() + b":") and b"prio 1" in err and b"null" in err and field.encode() in err
    lib.rl_destroy(h)


@pytest.mark.parametrize("field", ["weight", "keys"])
def test_the_draw_needs_its_scratch_columns_and_the_update_does_not_read_them(field):
    lib, h = _lib.lib(), _handle()
    rc, err = _call("rl_learn_prioritized_draw", h, *_args(prio={field: None}))
    assert rc == -1 and b"prio 0" in err and field.encode() in err
    ls, rs, ps = _args()
    rs[0].age = None
    rc, err = _call("rl_learn_prioritized_draw", h, ls, rs, ps)
    assert rc == -1 and b"replay 0" in err and b"age" in err
    lib.rl_destroy(h)


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("alpha", [0.0, -0.6, float("nan")])
def test_alpha_must_be_positive(name, alpha):
    lib, h = _lib.lib(), _handle()
    rc, err = _call(name, h, *_args(prio={"alpha": alpha}))
    assert rc == -1 and b"alpha" in err and b"prio 0" in err
    lib.rl_destroy(h)


def test_the_fixture_is_what_the_torch_restatement_makes_of_its_inputs():
    g, p = dc.golden(), pc.golden()
    assert p["priorities"].shape == (3, 64) and p["priorities"].dtype == np.float32 and np.array_equal(p["indices"], g["slots"])
    assert p["final"].size == dc.N_PARAMS and (p["priorities"] >= 0).all() and p["priorities"].max() > 10 * p["priorities"].min()
    torch.set_num_threads(1)
    # the same update as D3QN's: the same torch restatement ends on the same parameters
    mine = dc.torch_steps(g)
    print("max |restatement - final| %.3g; max |final - learn_d3qn.final| %.3g" % (np.abs(mine - p["final"]).max(), np.abs(p["final"] - g["final"]).max()))
    assert np.abs(mine - p["final"]).max() <= 1e-6
    # the priorities: |max q' - q[a]| in float64 on the parameters each step started from, within twice torch's own float32 error
    err = float(p["ref_prio_err"])
    assert 1e-9 < err < 1e-6
    again = 0.0
    for s, flat in enumerate(pc.step_params()):
        p64, q, qn = pc.priorities(flat, g["target_init"], g, g["slots"][s])
        p32 = pc.priorities(flat, g["target_init"], g, g["slots"][s], torch.float32)[0]
        scale = max(np.abs(q).max(), np.abs(qn).max())
        worst = np.abs(p["priorities"][s] - p64).max()
        again = max(again, np.abs(p32 - p64).max() / scale)
        print("step %d: max |priority - float64| %.3g, bound %.3g (scale %.4g)" % (s, worst, 2 * err * scale, scale))
        assert worst <= 2 * err * scale, s
        # not the TD error: the reference leaves reward, gamma and the done mask out (PERD3QN.py:110)
        td = np.abs(dc.td_errors(dc.net_of(flat), dc.net_of(g["target_init"]), g, g["slots"][s], float(g["gamma"]), torch.float64).detach().numpy())
        assert np.abs(td - p64).max() > 1.0
    print("ref_prio_err recorded %.4g, recomputed %.4g" % (err, again))
    assert 0.5 * err <= again <= 2 * err
    # slots[0][1] repeats slots[0][0]: equal rows, equal priorities
    assert p["priorities"][0][1] == p["priorities"][0][0]


def test_the_host_model_of_the_memory_reproduces_the_reference_buffers_trace():
    """Stamping after the fact is what store() does one row at a time: 5 stores, update_priorities([1, 3], [0.5, 2.0]), 6 more stores
    through the wrap of a capacity-8 buffer -- the priorities after every event, exactly, and sample()'s p to 1e-7."""
    p = pc.golden()
    trace, (first, second) = p["buf_prio_trace"], p["buf_stores"]
    assert trace.shape == (first + 1 + second, int(p["buf_capacity"])) and first + second > int(p["buf_capacity"])
    m = pc.HostMemory(int(p["buf_capacity"]), float(p["buf_alpha"]))
    e = 0
    for _ in range(first):
        m.store()
        assert m.stamp().tobytes() == trace[e].tobytes(), e
        e += 1
    m.update(p["buf_update_idx"], p["buf_update_prio"])
    assert m.stamp().tobytes() == trace[e].tobytes() and m.prio_max == 2.0
    e += 1
    for _ in range(second):
        m.store()
        assert m.stamp().tobytes() == trace[e].tobytes(), e
        e += 1
    assert len(set(trace[-1].tolist())) > 1                                           # (a row that kept an older maximum)
    assert np.abs(m.probs() - p["buf_probs"]).max() <= 1e-7 and abs(p["buf_probs"].sum() - 1) < 1e-6
    # stamping once, after all six stores, gives what stamping after every store gave (the maximum does not move in between)
    late = pc.HostMemory(int(p["buf_capacity"]), float(p["buf_alpha"]))
    late.store(first)
    late.update(p["buf_update_idx"], p["buf_update_prio"])
    late.store(second)
    assert late.stamp().tobytes() == trace[-1].tobytes()
    # more than a capacity of rows between two looks: every row
    late.store(20)
    assert (late.stamp() == late.prio_max).all()


@pytest.mark.parametrize("brains, kwargs, says", [
    (lambda: [Models.DQN(max_epi=60), Models.PERD3QN()], dict(learn_prioritized=True), "learn_prioritized=True needs learn='device'"),
    (lambda: [Models.DQN(max_epi=60), Models.D3QN()], dict(learn="device", learn_prioritized=True), "needs at least one Models.PERD3QN"),
    (lambda: [Models.DQN(max_epi=60), Models.PERD3QN()], dict(learn="device", learn_prioritized=False), "learn_prioritized must be None or True"),
])
def test_learn_prioritized_states_its_conditions_before_touching_a_gpu(brains, kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(brains(), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_the_older_switches_answer_what_they_answered():
    from reinlife_amd.learn import ENTRY_BY_METHOD, entry_of
    assert ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}
    assert entry_of(_lib.PERD3QN) is None and entry_of(_lib.D3QN) == "rl_learn_dueling"


def test_the_exponential_race_on_content_keys_draws_in_proportion_to_the_weights():
    """The draw of rl_learn_prioritized_draw restated on the host (learn_perd3qn_cases.host_draw: the kernel's integer code and the
    library's rl_philox; numpy's log and power): 48 fixture rows with priorities cycling through {0, 0.25, 1, 4}, 6,400 draws -- no
    zero-priority row, every other count within 5 binomial standard deviations of 6400 w / sum w; all weights zero: uniform."""
    g = dc.golden()
    keys = pc.content_keys(g, 48)
    assert len(set(keys.tolist())) == 48
    n = 6400
    pri = np.tile(np.array([0.0, 0.25, 1.0, 4.0]), 12)
    counts = np.bincount(pc.host_draw(keys, pri, 11, 0, 0, n), minlength=48)
    w = pri ** 0.6
    prob = w / w.sum()
    sd = np.sqrt(n * prob * (1 - prob))
    z = np.abs(counts - n * prob)[pri > 0] / sd[pri > 0]
    print("weighted: worst deviation %.2f sd" % z.max())
    assert not counts[pri == 0].any() and (z <= 5).all()
    flat = np.bincount(pc.host_draw(keys, np.zeros(48), 11, 0, 0, n), minlength=48)
    zu = np.abs(flat - n / 48) / np.sqrt(n * (1 / 48) * (47 / 48))
    print("all zero: worst deviation from uniform %.2f sd" % zu.max())
    assert (zu <= 5).all()
