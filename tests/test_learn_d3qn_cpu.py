"""CPU: the host side of on-device D3QN learning -- rl_learn_dueling / rl_learn_dueling_supported are exported and validate their
arguments without a GPU, learn_kinds refuses what it cannot do before it touches a device, Models.D3QN keeps its learning rate and
capacity without another generator draw, and the fixture tests/golden/learn_d3qn.npz (the reference's own train(),
tools/gen_golden_learn_d3qn.py) is reproduced by a torch restatement of ReinLife/Models/D3QN.py:97-116, 148-165 written in
tests/learn_d3qn_cases.py -- whose batch-wide advantage mean the fixture tells apart from a per-row mean."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_d3qn_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)


def test_rl_learn_dueling_is_exported_and_supported_for_d3qn_alone():
    lib = _lib.lib()
    assert hasattr(lib, "rl_learn_dueling") and hasattr(lib, "rl_learn_dueling_supported")
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert lib.rl_learn_dueling_supported(-1) == 0 and lib.rl_learn_dueling_supported(9) == 0
    assert [lib.rl_learn_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]            # (rl_learn's contract is what it was)
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "int rl_learn_dueling(" in hdr and "D3QN.py:97-116" in hdr and "D3QN.py:165" in hdr


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.D3QN, p, p, p, p, p, p, 0.001, 0.99, 0.9, 0.999, 1e-8, 64, 63, 0, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 96) for _ in range(n)])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls, rs


@pytest.mark.parametrize("field", ["params", "target", "adam_m", "adam_v", "state", "packed"])
def test_rl_learn_dueling_rejects_null_learner_pointers(field):
    lib, h = _lib.lib(), _handle()
    ls, rs = _args(2, **{field: None})
    assert lib.rl_learn_dueling(h, ls, rs, 2, 1, None, None) == -1
    err = lib.rl_last_error()
    assert err.startswith(b"rl_learn_dueling:") and b"learner 1" in err and b"null" in err
    lib.rl_destroy(h)


def test_rl_learn_dueling_rejects_bad_counts_kinds_and_rings():
    lib, h = _lib.lib(), _handle()
    ls, rs = _args()
    assert lib.rl_learn_dueling(None, ls, rs, 1, 1, None, None) == -1 and b"rl_learn_dueling: null handle" in lib.rl_last_error()
    assert lib.rl_learn_dueling(h, None, rs, 1, 1, None, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn_dueling(h, ls, None, 1, 1, None, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn_dueling(h, ls, rs, 1, 0, None, None) == -1 and b"n_steps" in lib.rl_last_error()
    assert lib.rl_learn_dueling(h, ls, rs, 0, 1, None, None) == -1 and b"n_learners" in lib.rl_last_error()
    l17, r17 = _args(17)
    assert lib.rl_learn_dueling(h, l17, r17, 17, 1, None, None) == -1 and b"n_learners" in lib.rl_last_error() and b"16" in lib.rl_last_error()
    for batch in (0, 65, -1):
        ls, rs = _args(batch=batch)
        assert lib.rl_learn_dueling(h, ls, rs, 1, 1, None, None) == -1 and b"batch" in lib.rl_last_error() and b"[1,64]" in lib.rl_last_error(), batch
    for kind in (_lib.DQN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        ls, rs = _args(kind=kind)
        assert lib.rl_learn_dueling(h, ls, rs, 1, 1, None, None) == -4, kind          # RL_E_UNSUPPORTED
        assert ("kind %d" % kind).encode() in lib.rl_last_error() and lib.rl_last_error().startswith(b"rl_learn_dueling:")
    ls, rs = _args()
    rs[0].reward = None
    assert lib.rl_learn_dueling(h, ls, rs, 1, 1, None, None) == -1 and b"replay 0" in lib.rl_last_error()
    ls, rs = _args()
    rs[0].capacity = 0
    assert lib.rl_learn_dueling(h, ls, rs, 1, 1, None, None) == -1 and b"replay 0" in lib.rl_last_error()
    lib.rl_destroy(h)


def test_the_fixture_is_what_three_torch_steps_make_of_its_inputs():
    g = dc.golden()
    assert g["slots"].shape == (3, 64) and g["slots"][0, 1] == g["slots"][0, 0] and g["ring_state"].shape == (96, 153)
    assert g["slots"].min() >= 0 and g["slots"].max() < 96
    assert 0.1 < g["ring_done"].mean() < 0.35 and set(np.unique(g["ring_reward"])) <= {0.0, np.float32(0.05), np.float32(0.3), -1.0, 5.0, -10.0, 400.0, -400.0}
    assert not g["ring_state"][:, 3::10].any()
    assert g["init"].size == _lib.lib().rl_policy_n_params(_lib.D3QN) == g["final"].size == g["target_init"].size == dc.N_PARAMS == 53897
    assert np.array_equal(g["target_init"], g["init"] * np.float32(0.9)) and (float(g["lr"]), float(g["gamma"])) == (1e-3, 0.99)
    torch.set_num_threads(1)
    mine = dc.torch_steps(g)
    # the same torch, the same operations: equal up to the order of float32 sums inside torch's kernels
    print("max |restatement - final| %.3g" % np.abs(mine - g["final"]).max())
    assert np.abs(mine - g["final"]).max() <= 1e-6, np.abs(mine - g["final"]).max()
    assert np.abs(g["final"] - g["init"]).max() > 1e-3                       # three steps of lr 1e-3 moved the parameters
    # the recorded spreads of torch itself are what the float64 restatement gives
    f64 = dc.torch_steps(g, torch.float64)
    q = lambda p: dc.q_values(p, g["ring_state"])  # noqa: E731
    effect = np.abs(q(g["final"]) - q(g["init"])).max()
    assert abs(effect - float(g["effect"])) <= 1e-9 * effect
    assert abs(np.abs(q(g["final"]) - q(f64)).max() / effect - float(g["ref_q_spread"])) <= 1e-3 * float(g["ref_q_spread"])
    assert 1e-9 < float(g["ref_grad_err"]) < 1e-6 and 1e-9 < float(g["ref_q_spread"]) < 1e-5
    # ref_grad_err sets the bar of the GPU end-to-end test: torch float32 autograd of step 1 against float64, over all parameters.  It is
    # rounding noise of torch's float32 kernels, so another torch build may sum in another order: the same size, not the same digits.
    flat = lambda ts: np.concatenate([t.reshape(-1).astype(np.float64) for t in ts])  # noqa: E731
    g64 = flat(dc.grads64(g["init"], g["target_init"], g, g["slots"][0], float(g["gamma"]))[1])
    g32 = flat(dc.grads64(g["init"], g["target_init"], g, g["slots"][0], float(g["gamma"]), dtype=torch.float32)[1])
    again = np.abs(g32 - g64).max() / np.abs(g64).max()
    print("ref_grad_err recorded %.4g, recomputed %.4g" % (float(g["ref_grad_err"]), again))
    assert 0.5 * float(g["ref_grad_err"]) <= again <= 2 * float(g["ref_grad_err"])


def test_the_fixture_tells_the_batch_wide_mean_from_a_per_row_mean():
    """D3QN.py:165 subtracts advantage.mean() -- over the whole minibatch.  A per-row mean gives another step-1 gradient: by far more
    than the 1e-5 of max |g| the GPU test allows."""
    g = dc.golden()
    _, batch_wide = dc.grads64(g["init"], g["target_init"], g, g["slots"][0], float(g["gamma"]))
    _, per_row = dc.grads64(g["init"], g["target_init"], g, g["slots"][0], float(g["gamma"]), row_mean=True)
    for name, a, b in zip(dc.NAMES, batch_wide, per_row):
        print("%-18s max |g_row_mean - g| / max |g| = %.3g" % (name, np.abs(a - b).max() / np.abs(a).max()))
    assert np.abs(batch_wide[0] - per_row[0]).max() > 1e-2 * np.abs(batch_wide[0]).max()


def _brains():
    return [Models.DQN(max_epi=60), Models.D3QN()]


@pytest.mark.parametrize("kwargs, says", [
    (dict(learn="device", learn_kinds=("DQN", "PERD3QN")), "no entry point trains PERD3QN"),
    (dict(learn="device", learn_kinds=("PPO",)), "no entry point trains PPO"),
    (dict(learn="device", learn_kinds=("DQN", "D4QN")), "no entry point trains D4QN"),
    (dict(learn="device", learn_kinds=("DQN", "D3QN"), learn_steps={"PPO": 2}), "learn_steps"),
    (dict(learn="device", learn_kinds=("DQN", "D3QN"), learn_steps={"D3QN": 0}), "learn_steps"),
    (dict(learn_kinds=("DQN", "D3QN")), "learn_kinds needs learn='device'"),
    (dict(learn_kinds=("DQN",)), "learn_kinds needs learn='device'"),
])
def test_learn_kinds_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(), n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


@pytest.mark.parametrize("cls", [Models.D3QN, Models.PERD3QN])
def test_the_dueling_brains_keep_their_learning_rate_and_capacity_and_draw_what_they_drew(cls):
    torch.manual_seed(5)
    b = cls()
    after = torch.rand(1).item()
    torch.manual_seed(5)
    sizes = [(153, 128), (128, 128), (128, 8), (128, 128), (128, 1)]
    ref = [torch.nn.Linear(i, o) for i, o in sizes], [torch.nn.Linear(i, o) for i, o in sizes]   # target_net, then eval_net: nothing else drawn
    assert after == torch.rand(1).item()
    assert all(torch.equal(p, q) for p, q in zip(b.target_net.parameters(), [t for l in ref[0] for t in (l.weight, l.bias)]))
    assert b.learning_rate == 1e-3 and b.capacity == 10000 and b.batch_size == 64 and b.gamma == 0.99
    c = cls(learning_rate=3e-4, capacity=777)
    assert c.learning_rate == 3e-4 and c.capacity == 777
