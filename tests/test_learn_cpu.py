"""CPU: the host side of on-device DQN learning -- rl_learn / rl_learn_supported are exported and validate their arguments without a
GPU, trainer(learn="device") refuses what it cannot do before it touches a device, learn=None changes nothing, and the fixture
tests/golden/learn_dqn.npz (the reference's own train(), tools/gen_golden_learn.py) is reproduced by a torch restatement of
ReinLife/Models/DQN.py:142-153 written here."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rl_learn_is_exported_and_supported_for_dqn_alone():
    lib = _lib.lib()
    assert hasattr(lib, "rl_learn") and hasattr(lib, "rl_learn_supported")
    assert [lib.rl_learn_supported(k) for k in (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)] == [1, 0, 0, 0, 0]
    assert lib.rl_learn_supported(-1) == 0 and lib.rl_learn_supported(9) == 0
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "RL_SITE_LEARN = 10" in hdr and "6  rl_learn" in hdr and "DQN.py:80-83" in hdr


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.DQN, p, p, p, p, p, p, 0.0005, 0.98, 0.9, 0.999, 1e-8, 32, 1000, 1, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, None, p, p, 48) for _ in range(n)])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls, rs


@pytest.mark.parametrize("field", ["params", "target", "adam_m", "adam_v", "state", "packed"])
def test_rl_learn_rejects_null_learner_pointers(field):
    lib, h = _lib.lib(), _handle()
    ls, rs = _args(2, **{field: None})
    assert lib.rl_learn(h, ls, rs, 2, 5, None, None) == -1
    assert b"learner 1" in lib.rl_last_error() and b"null" in lib.rl_last_error()
    lib.rl_destroy(h)


def test_rl_learn_rejects_bad_counts_kinds_and_rings():
    lib, h = _lib.lib(), _handle()
    ls, rs = _args()
    assert lib.rl_learn(None, ls, rs, 1, 5, None, None) == -1 and b"null handle" in lib.rl_last_error()
    assert lib.rl_learn(h, None, rs, 1, 5, None, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn(h, ls, None, 1, 5, None, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn(h, ls, rs, 1, 0, None, None) == -1 and b"n_steps" in lib.rl_last_error()
    assert lib.rl_learn(h, ls, rs, 0, 5, None, None) == -1 and b"n_learners" in lib.rl_last_error()
    l17, r17 = _args(17)
    assert lib.rl_learn(h, l17, r17, 17, 5, None, None) == -1 and b"n_learners" in lib.rl_last_error() and b"16" in lib.rl_last_error()
    for batch in (0, 33, -1):
        ls, rs = _args(batch=batch)
        assert lib.rl_learn(h, ls, rs, 1, 5, None, None) == -1 and b"batch" in lib.rl_last_error(), batch
    for kind in (_lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN, 7):
        ls, rs = _args(kind=kind)
        assert lib.rl_learn(h, ls, rs, 1, 5, None, None) == -4, kind          # RL_E_UNSUPPORTED
        assert ("kind %d" % kind).encode() in lib.rl_last_error()
    ls, rs = _args()
    rs[0].reward = None
    assert lib.rl_learn(h, ls, rs, 1, 5, None, None) == -1 and b"replay 0" in lib.rl_last_error()
    ls, rs = _args()
    rs[0].capacity = 0
    assert lib.rl_learn(h, ls, rs, 1, 5, None, None) == -1 and b"replay 0" in lib.rl_last_error()
    lib.rl_destroy(h)


def test_rl_learn_draw_validates_its_arguments():
    lib, h = _lib.lib(), _handle()
    ls, rs = _args()
    p = C.c_void_p(0x1000)
    keys = (C.c_void_p * 1)(p)
    assert lib.rl_learn_draw(None, ls, rs, 1, 5, keys, p, None) == -1 and b"null handle" in lib.rl_last_error()
    assert lib.rl_learn_draw(h, ls, rs, 1, 5, None, p, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn_draw(h, ls, rs, 1, 5, keys, None, None) == -1 and b"null" in lib.rl_last_error()
    assert lib.rl_learn_draw(h, ls, rs, 1, 0, keys, p, None) == -1 and b"n_steps" in lib.rl_last_error()
    assert lib.rl_learn_draw(h, ls, rs, 17, 5, keys, p, None) == -1 and b"n_learners" in lib.rl_last_error()
    assert lib.rl_learn_draw(h, ls, rs, 1, 5, (C.c_void_p * 1)(None), p, None) == -1 and b"keys" in lib.rl_last_error()
    ls, rs = _args(batch=33)
    assert lib.rl_learn_draw(h, ls, rs, 1, 5, keys, p, None) == -1 and b"batch" in lib.rl_last_error()
    ls, rs = _args()
    rs[0].age = None
    assert lib.rl_learn_draw(h, ls, rs, 1, 5, keys, p, None) == -1 and b"replay 0" in lib.rl_last_error()
    lib.rl_destroy(h)


class _FakeDist:
    """A process group of four ranks, as far as resolve_dist looks."""

    def is_initialized(self):
        return True

    def get_rank(self):
        return 1

    def get_world_size(self):
        return 4


def _brains():
    return [Models.DQN(max_epi=60), Models.DQN(max_epi=60)]


@pytest.mark.parametrize("kwargs, says", [
    (dict(rng="reference", n_worlds=1), "rng='philox'"),
    (dict(n_worlds=1), "rng='philox'"),                                    # (a single world defaults to the reference's generators)
    (dict(n_worlds=4, static_families=False), "static_families=True"),
    (dict(n_worlds=4, training=False), "training=True"),
    (dict(n_worlds=4, dist=_FakeDist()), "single rank"),
    (dict(n_worlds=4, per_agent_api=True), "fused"),
    (dict(n_worlds=4, fused=False), "fused"),
    (dict(n_worlds=4, learn_steps=0), "learn_steps"),
])
def test_trainer_learn_device_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer(_brains(), n_episodes=5, learn="device", save=False, print_results=False, **kwargs)


def test_trainer_rejects_an_unknown_learn_mode():
    with pytest.raises(ValueError, match="learn must be"):
        trainer(_brains(), n_episodes=5, learn="host", n_worlds=4, save=False, print_results=False)


def test_learn_none_constructs_what_it_always_did(monkeypatch):
    """The default: same brains (no extra generator draw, no target module), the same inference-only warning, no learners, no capture."""
    from reinlife_amd.World import environment as envmod
    torch.manual_seed(5)
    a = Models.DQN(max_epi=60)
    after = torch.rand(1).item()
    torch.manual_seed(5)
    ref = torch.nn.Linear(153, 128), torch.nn.Linear(128, 64), torch.nn.Linear(64, 8)    # _Qnet's three layers, nothing else drawn
    assert after == torch.rand(1).item()
    assert all(torch.equal(p, q) for p, q in zip(a.agent.parameters(), [t for l in ref for t in (l.weight, l.bias)]))
    assert not hasattr(a, "target") and a.learning_rate == 0.0005

    class Stub:   # a DeviceWorlds that records what Environment asks of it
        def __init__(self, **k):
            self.calls, self.device = [], k["device"]

        def enable_tracking(self, on=True):
            pass

        def enable_capture(self, *a, **k):
            self.calls.append("enable_capture")
    monkeypatch.setattr(envmod, "DeviceWorlds", Stub)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        env = envmod.Environment(brains=_brains(), n_worlds=4, print_results=False)
    assert [str(x.message) for x in w if "brain.learn() is a no-op" in str(x.message)], "the inference-only warning is gone"
    assert env.learn is None and env.learners == {} and env.learn_every is None and env.worlds.calls == []
    assert "inference only" in env._weights_note()


def _torch_five_steps(g, dtype=torch.float32):
    """DQN.py:142-153 restated: five times smooth-L1 of Q(s)[a] against r + gamma max Q_target(s') done_mask, one Adam step each."""
    net, tgt = lc.qnet(g["init"], dtype), lc.qnet(g["init"], dtype)
    opt = torch.optim.Adam(net.parameters(), lr=float(g["lr"]))
    for s in range(g["slots"].shape[0]):
        loss = lc.dqn_loss(net, tgt, g, g["slots"][s], float(g["gamma"]), dtype)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return lc.flat_of(net)


def test_the_fixture_is_what_five_torch_steps_make_of_its_inputs():
    g = lc.golden()
    assert g["slots"].shape == (5, 32) and g["slots"][0, 1] == g["slots"][0, 0] and g["ring_state"].shape == (48, 153)
    assert g["slots"].min() >= 0 and g["slots"].max() < 48
    assert 0.1 < g["ring_done"].mean() < 0.35 and set(np.unique(g["ring_reward"])) <= {0.0, np.float32(0.05), np.float32(0.3), -1.0, 5.0, -10.0, 400.0, -400.0}
    assert not g["ring_state"][:, 3::10].any() and g["init"].size == _lib.lib().rl_policy_n_params(_lib.DQN) == g["final"].size
    torch.set_num_threads(1)
    mine = _torch_five_steps(g)
    # the same torch, the same operations: equal up to the order of float32 sums inside torch's kernels
    assert np.abs(mine - g["final"]).max() <= 1e-6, np.abs(mine - g["final"]).max()
    assert np.abs(g["final"] - g["init"]).max() > 1e-3                       # five steps of lr 5e-4 moved the parameters
    # the recorded spreads of torch itself are what the float64 restatement gives
    f64 = _torch_five_steps(g, torch.float64)
    q = lambda p: lc.q_values(p, g["ring_state"])  # noqa: E731
    effect = np.abs(q(g["final"]) - q(g["init"])).max()
    assert abs(effect - float(g["effect"])) <= 1e-9 * effect
    assert abs(np.abs(q(g["final"]) - q(f64)).max() / effect - float(g["ref_q_spread"])) <= 1e-3 * float(g["ref_q_spread"])
    assert 1e-9 < float(g["ref_grad_err"]) < 1e-6 and 1e-9 < float(g["ref_q_spread"]) < 1e-5
    # both smooth-L1 branches occur in the first minibatch
    net, tgt = lc.qnet(g["init"], torch.float64), lc.qnet(g["init"], torch.float64)
    td = lc.td_errors(net, tgt, g, g["slots"][0], float(g["gamma"]), torch.float64).abs()
    assert (td < 1).any() and (td > 1).any()


def test_philox_slots_follow_the_documented_mapping():
    from reinlife_amd import learn
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    s = learn.philox_slots(7, 1, 3, 2, 5, 1001)
    assert s.shape == (2, 5) and s.dtype == np.int32 and s.min() >= 0 and s.max() < 1001
    lib.rl_philox(7, 0, 1, 3, 10, 1 * 5 + 2, C.byref(out))
    assert s[1, 2] == (int(out[0]) * 1001) >> 32
