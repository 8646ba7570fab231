"""CPU: the host side of on-device PPO learning -- rl_learn_ppo / rl_learn_rollout / rl_learn_ppo_supported are exported and validate
their arguments without a GPU; the hand-written float64 model of PPO.learn() (tests/learn_ppo_cases.py: the gradients at the kinks of
min() and clamp() spelled out) equals torch autograd and reproduces the fixture tests/golden/learn_ppo.npz (the reference's own learn(),
tools/gen_golden_learn_ppo.py) within the fixture's own float32 spread; the float32 form of the GAE recursion gives the reference's
advantages bit for bit; the host model of the rollout window; and learn_rollout refuses what it cannot do before it touches a device."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_ppo_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PPO, _lib.PERDQN)
ENTRIES = ("rl_learn_ppo", "rl_learn_rollout")


def test_the_three_symbols_are_exported_and_supported_for_ppo_alone():
    lib = _lib.lib()
    for name in ENTRIES + ("rl_learn_ppo_supported",):
        assert hasattr(lib, name), name
    assert [lib.rl_learn_ppo_supported(k) for k in KINDS] == [0, 0, 0, 1, 0]
    assert lib.rl_learn_ppo_supported(-1) == 0 and lib.rl_learn_ppo_supported(9) == 0
    assert [lib.rl_learn_supported(k) for k in KINDS] == [1, 0, 0, 0, 0]            # (the older contracts are what they were)
    assert [lib.rl_learn_dueling_supported(k) for k in KINDS] == [0, 1, 0, 0, 0]
    assert [lib.rl_learn_prioritized_supported(k) for k in KINDS] == [0, 0, 1, 0, 0]
    assert (_lib.SITE_LEARN, _lib.SITE_LEARN_PRIO, _lib.SITE_LEARN_ROLLOUT, _lib.PPO_ROLLOUT_MAX) == (10, 11, 12, 32)
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "RL_SITE_LEARN_ROLLOUT = 12" in hdr and "#define RL_PPO_ROLLOUT_MAX 32" in hdr
    assert "int rl_learn_ppo(" in hdr and "int rl_learn_rollout(" in hdr and "int rl_learn_ppo_supported(" in hdr
    assert C.sizeof(_lib.Ppo) == 40                                                   # two floats, an int, padding, three pointers
    assert int(lib.rl_policy_n_params(_lib.PPO)) == pc.N_PARAMS == 107529


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


def _args(n=1, ppo=None, **over):
    """A well-formed argument set over dummy non-null addresses (validation happens before anything is launched or dereferenced)."""
    p = C.c_void_p(0x1000)
    ls = (_lib.Learner * n)(*[_lib.Learner(_lib.PPO, p, None, p, p, p, p, 0.0005, 0.98, 0.9, 0.999, 1e-8, 32, 0, 0, None, None) for _ in range(n)])
    rs = (_lib.Replay * n)(*[_lib.Replay(p, p, p, p, p, p, p, p, 96) for _ in range(n)])
    ps = (_lib.Ppo * n)(*[_lib.Ppo(0.95, 0.1, 3, p, p, p) for _ in range(n)])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    for k, v in (ppo or {}).items():
        setattr(ps[n - 1], k, v)
    return ls, rs, ps


def _call(name, h, ls, rs, ps, n=1, n_steps=1, slots=C.c_void_p(0x1000)):
    lib = _lib.lib()
    rc = getattr(lib, name)(h, ls, rs, ps, n, n_steps, slots, None)
    return rc, lib.rl_last_error()


@pytest.mark.parametrize("name", ENTRIES)
def test_bad_handles_counts_kinds_batches_and_rings_are_refused_by_name(name):
    lib, h = _lib.lib(), _handle()
    ls, rs, ps = _args()
    rc, err = _call(name, None, ls, rs, ps)
    assert rc == -1 and err == (name + ": null handle").encode()
    for bad in ((None, rs, ps), (ls, None, ps), (ls, rs, None)):
        rc, err = _call(name, h, *bad)
        assert rc == -1 and err.startswith(name.encode() + b":") and b"null learners / rings / ppos" in err
    rc, err = _call(name, h, ls, rs, ps, n_steps=0)
    assert rc == -1 and b"n_steps" in err
    rc, err = _call(name, h, ls, rs, ps, n=0)
    assert rc == -1 and b"n_learners" in err
    rc, err = _call(name, h, *_args(17), n=17)
    assert rc == -1 and b"n_learners" in err and b"16" in err                          # RL_MAX_CAPTURE_BRAINS
    for batch in (0, 33, 64):
        rc, err = _call(name, h, *_args(batch=batch))
        assert rc == -1 and b"batch" in err and b"[1,32]" in err, batch
    for kind in (_lib.DQN, _lib.D3QN, _lib.PERD3QN, _lib.PERDQN, 7):
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


def test_rl_learn_ppo_refuses_its_own_arguments():
    lib, h = _lib.lib(), _handle()
    rc, err = _call("rl_learn_ppo", h, *_args(), slots=None)
    assert rc == -1 and b"rl_learn_rollout" in err                                     # names where slots come from
    for k in (0, 9, -1):
        rc, err = _call("rl_learn_ppo", h, *_args(2, ppo={"k_epoch": k}), n=2)
        assert rc == -1 and b"k_epoch" in err and b"[1,8]" in err and b"ppo 1" in err, k
    ls, rs, ps = _args()
    rs[0].prob = None
    rc, err = _call("rl_learn_ppo", h, ls, rs, ps)
    assert rc == -1 and b"replay 0" in err and b"prob" in err                          # a ring without prob
    for field in ("params", "adam_m", "adam_v", "state", "packed"):
        rc, err = _call("rl_learn_ppo", h, *_args(**{field: None}))
        assert rc == -1 and b"learner 0" in err and field.encode() in err, field
    # target (NULL in _args), min_size and sync_target are ignored, fresh may be NULL: what is left is valid up to the launch itself, which
    # a machine without a GPU cannot make -- so only the draw's own demands are shown here
    for field in ("seen", "fresh", "keys"):
        rc, err = _call("rl_learn_rollout", h, *_args(ppo={field: None}))
        assert rc == -1 and b"ppo 0" in err and field.encode() in err, field
    ls, rs, ps = _args()
    rs[0].age = None
    rc, err = _call("rl_learn_rollout", h, ls, rs, ps)
    assert rc == -1 and b"replay 0" in err and b"age" in err
    lib.rl_destroy(h)


# ---- the host model against the fixture ----
def test_the_fixture_meets_the_conditions_its_generator_asserts():
    g = pc.golden()
    assert g["rows"].tolist() == [32, 17, 1] and g["slots"].shape == (3, 32) and (g["slots"][1][17:] == -1).all()
    assert g["final"].size == pc.N_PARAMS and g["final"].dtype == np.float32 and g["prob"].shape == (96,)
    assert (float(g["lr"]), float(g["gamma"]), float(g["lmbda"]), float(g["eps_clip"]), int(g["k_epoch"])) == (pc.LR, pc.GAMMA, pc.LMBDA, pc.EPS_CLIP, pc.K_EPOCH)
    assert (g["factor"] >= 0.8).all() and (g["factor"] <= 1.25).all() and (g["prob"] > 0).all() and (g["prob"] <= 1).all()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "learn_ppo.npz")) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "models.npz"))
    for slots in pc.rollouts(g)[:2]:
        _, _, mid = pc.grads_by_hand(g["init"], pc.rows_of(g, g["prob"], slots))
        ratio, adv, d = mid["ratio"], mid["adv"], mid["v"] - mid["td"]
        lo, hi = 1 - pc.EPS_CLIP, 1 + pc.EPS_CLIP
        assert ((adv > 0) & (ratio > hi)).any() and ((adv > 0) & (ratio < lo)).any() and ((adv < 0) & (ratio > hi)).any()
        assert ((adv < 0) & (ratio >= lo) & (ratio <= hi)).any()
        assert (np.abs(d) < 1).any() and (np.abs(d) > 1).any()
        assert np.abs(ratio - lo).min() > 1e-4 and np.abs(ratio - hi).min() > 1e-4 and np.abs(np.abs(d) - 1).min() > 1e-4


@pytest.mark.parametrize("which", [0, 1, 2])
def test_hand_written_gradients_equal_autograd(which):
    """float64, on the initial parameters, the fixture's rollouts of 32, 17 and 1 rows."""
    g = pc.golden()
    rows = pc.rows_of(g, g["prob"], pc.rollouts(g)[which])
    loss_a, ga, mid_a = pc.grads_autograd(g["init"], rows)
    loss_h, gh, mid_h = pc.grads_by_hand(g["init"], rows)
    assert abs(loss_a - loss_h) <= 1e-13 * max(1.0, abs(loss_a))
    for name, a, b in zip(pc.NAMES, ga, gh):
        err = np.abs(a - b).max() / np.abs(a).max()
        print("rollout %d: %-13s max|g| %.4g  |hand - autograd| / max|g| %.3g" % (which, name, np.abs(a).max(), err))
        assert err <= 1e-12, name
        assert not b[a == 0].any(), name
    assert np.array_equal(mid_a["adv"], mid_h["adv"])
    if which == 0:   # the generator's float64 run starts here too (its later rollouts run on trained parameters)
        np.testing.assert_allclose([np.abs(x).max() for x in ga], g["grad_max"][0, 0], rtol=1e-9)


def test_the_float32_recursion_gives_the_references_advantages_bit_for_bit():
    g = pc.golden()
    assert g["adv"].dtype == np.float32 and g["delta"].dtype == np.float32
    for i, n in enumerate(g["rows"]):
        for ep in range(int(g["k_epoch"])):
            mine = pc.gae32(g["delta"][i, ep, :n])
            assert mine.tobytes() == g["adv"][i, ep, :n].tobytes(), (i, ep)
    # what a double recursion (numpy 1.x) would have made differs in the last bits somewhere: the form matters
    d = g["delta"][0, 0].astype(np.float64)
    adv, out = 0.0, np.zeros(32)
    for t in range(31, -1, -1):
        adv = pc.GAMMA * pc.LMBDA * adv + d[t]
        out[t] = adv
    assert out.astype(np.float32).tobytes() != g["adv"][0, 0].tobytes()


def test_final_parameters_of_the_host_model_lie_within_the_fixtures_own_spread():
    """The hand-written model runs the nine epochs in float64; the reference ran them in float32.  Their outputs (probabilities and
    values over the 96 ring states) differ by what the fixture itself records for torch float32 against float64, ref_out_spread."""
    g = pc.golden()
    final = pc.learn_by_hand(g["init"], g, g["prob"], pc.rollouts(g))
    o_ref, o_mine, o_init = pc.outputs(g["final"], g["ring_state"]), pc.outputs(final, g["ring_state"]), pc.outputs(g["init"], g["ring_state"])
    effect = np.abs(o_ref - o_init).max()
    ratio = np.abs(o_mine - o_ref).max() / effect
    print("host model: max|d out| / effect %.3g (ref_out_spread %.3g), effect %.3g (fixture %.3g), max |p - final| %.3g"
          % (ratio, float(g["ref_out_spread"]), effect, float(g["effect"]), np.abs(final - g["final"]).max()))
    np.testing.assert_allclose(effect, float(g["effect"]), rtol=1e-9)
    assert ratio <= float(g["ref_out_spread"]) * (1 + 1e-3)
    assert effect > 1e4 * float(g["ref_out_spread"]) * effect                        # training moved the outputs far more than rounding does


def _case(ratio_factor, adv_sign):
    """One row whose ratio is exactly ratio_factor: prob_a = pi(s)[a] / ratio_factor in float64, reward chosen for the sign of delta."""
    g = pc.golden()
    slot = int(g["slots"][0][0])
    rows = pc.rows_of(g, g["prob"], [slot])
    net = pc.net_of(g["init"])
    with torch.no_grad():
        pi_a = net.pi(rows["s"]).gather(1, rows["a"])
    rows["prob"] = pi_a / ratio_factor
    rows["r"] = torch.full_like(rows["r"], 0.5 * adv_sign)
    return g, rows


@pytest.mark.parametrize("adv_sign", [1.0, -1.0])
def test_a_ratio_of_exactly_one_takes_the_tie_rule(adv_sign):
    """On-policy rows in their first epoch: surr1 == surr2 exactly, min() gives each side half, the clamp passes its half: coefficient 1."""
    g, rows = _case(1.0, adv_sign)
    loss_h, gh, mid = pc.grads_by_hand(g["init"], rows)
    assert mid["ratio"][0] == 1.0 and mid["coef"][0] == 1.0 and np.sign(mid["adv"][0]) == adv_sign
    loss_a, ga, _ = pc.grads_autograd(g["init"], rows)
    for name, a, b in zip(pc.NAMES, ga, gh):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), name
    assert np.abs(ga[4]).max() > 0                                                    # the policy head does get a gradient


@pytest.mark.parametrize("bound", ["lo", "hi"])
@pytest.mark.parametrize("adv_sign", [1.0, -1.0])
def test_a_ratio_exactly_on_a_clip_bound_passes_the_clamps_gradient(bound, adv_sign):
    """clamp(ratio) == ratio on the bound, so again surr1 == surr2, and the bound is inside the clamp's closed interval: coefficient 1,
    not 1/2 -- as torch makes it."""
    g, rows = _case(0.9 if bound == "lo" else 1.1, adv_sign)
    ratio = float(pc.grads_by_hand(g["init"], rows)[2]["ratio"][0])                   # about 0.9 / 1.1; the bound is put exactly on it
    eps = 1.0 - ratio if bound == "lo" else ratio - 1.0                               # (both subtractions, and 1 -+ eps again, are exact)
    assert (1.0 - eps if bound == "lo" else 1.0 + eps) == ratio and abs(eps - 0.1) < 1e-9
    loss_h, gh, mid = pc.grads_by_hand(g["init"], rows, eps_clip=eps)
    assert mid["ratio"][0] == ratio and mid["coef"][0] == 1.0
    loss_a, ga, _ = pc.grads_autograd(g["init"], rows, eps_clip=eps)
    for name, a, b in zip(pc.NAMES, ga, gh):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), name
    assert np.abs(ga[4]).max() > 0
    # just outside the bound the clamp stops it: coefficient 1 where the unclipped side is the smaller one, else 0
    rows["prob"] = rows["prob"] * (1.001 if bound == "lo" else 1 / 1.001)
    _, gh2, mid2 = pc.grads_by_hand(g["init"], rows, eps_clip=eps)
    want = 1.0 if (adv_sign > 0) == (bound == "lo") else 0.0
    assert mid2["coef"][0] == want
    _, ga2, _ = pc.grads_autograd(g["init"], rows, eps_clip=eps)
    assert np.abs(ga2[4] - gh2[4]).max() <= 1e-12 * max(np.abs(ga2[4]).max(), 1e-30)
    assert (np.abs(ga2[4]).max() > 0) == (want == 1.0)


# ---- the rollout window ----
def test_window_bookkeeping():
    w = pc.window_slots
    assert w(0, 0, 96) == []                                                           # nothing appended: an empty window
    assert w(0, 5, 96) == [0, 1, 2, 3, 4]
    assert w(5, 5, 96) == []                                                           # nothing since the last call
    assert w(90, 100, 96) == [90, 91, 92, 93, 94, 95, 0, 1, 2, 3]                      # the window wraps
    assert w(200, 250, 96) == [(200 + j) % 96 for j in range(50)]                      # seen in the middle of a wrapped ring
    assert sorted(w(100, 196, 96)) == list(range(96))                                  # count - seen == capacity: the whole ring
    assert sorted(w(3, 1000, 96)) == list(range(96))                                   # ... and beyond
    assert w(7, 3, 96) == []                                                           # a counter that went back (a fresh ring): empty, not negative
    # a draw names a window row, whatever the slots: the same rows under a rotation of the ring
    g = pc.golden()
    keys = [pc.row_key(g, r) for r in range(96)]
    rot = 37
    keys_rot = [keys[(i - rot) % 96] for i in range(96)]                               # row r sits in slot (r + rot) % 96
    for d, salt in enumerate((0x0123456789abcdef, 0xfedcba9876543210, 42)):
        a = pc.rollout_draw(keys, w(10, 40, 96), salt)
        b = pc.rollout_draw(keys_rot, w(10 + rot, 40 + rot, 96), salt)
        assert 10 <= a < 40 and (a + rot) % 96 == b, d
    assert pc.rollout_draw(keys, [], 1) == 0


# ---- Python: the brain's attributes and the keyword's refusals ----
def test_ppo_brain_keeps_its_hyperparameters():
    b = Models.PPO()
    assert (b.learning_rate, b.gamma, b.lmbda, b.eps_clip, b.k_epoch, b.train_freq) == (0.0005, 0.98, 0.95, 0.1, 3, 20)
    b = Models.PPO(learning_rate=1e-4, gamma=0.9, lmbda=0.8, eps_clip=0.2, k_epoch=5, train_freq=7)
    assert (b.learning_rate, b.gamma, b.lmbda, b.eps_clip, b.k_epoch, b.train_freq) == (1e-4, 0.9, 0.8, 0.2, 5, 7)


def test_learn_rollout_is_refused_before_a_device_is_touched():
    from reinlife_amd.World.environment import Environment
    from reinlife_amd import learn
    with pytest.raises(ValueError, match="learn_rollout=True needs learn='device'"):
        Environment(brains=[Models.PPO()], learn_rollout=True, device="cuda:99")
    with pytest.raises(ValueError, match="learn_rollout=True needs at least one Models.PPO"):
        Environment(brains=[Models.DQN(), Models.D3QN()], learn="device", learn_rollout=True, n_worlds=2, device="cuda:99")
    with pytest.raises(ValueError, match="learn_rollout must be None or True"):
        Environment(brains=[Models.PPO()], learn="device", learn_rollout=False, n_worlds=2, device="cuda:99")
    with pytest.raises(ValueError, match="rollout_steps needs learn_rollout=True"):
        Environment(brains=[Models.PPO()], learn="device", rollout_steps=2, n_worlds=2, device="cuda:99")
    with pytest.raises(ValueError, match="rollout_steps must be >= 1"):
        Environment(brains=[Models.PPO()], learn="device", learn_rollout=True, rollout_steps=0, n_worlds=2, device="cuda:99")
    with pytest.raises(ValueError, match="learn_rollout=True needs learn='device'"):
        trainer([Models.PPO()], n_episodes=1, learn_rollout=True, device="cuda:99", print_results=False, save=False)
    assert learn.ENTRY_BY_METHOD == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}   # (what learn_kinds offers is what it was)
    with pytest.raises(ValueError, match="rollout=True is for PPO brains"):
        learn.DeviceLearner(Models.DQN(), "cpu", rollout=True)
