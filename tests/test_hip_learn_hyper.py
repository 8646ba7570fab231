"""GPU: the learning kernels at hyperparameters other than the reference's defaults.  Every other GPU test of a learner runs it at the
defaults, so a kernel with a baked-in 0.99f, swapped betas, 0.6 where alpha belongs, or learner 0's values for every workgroup of a launch
would pass them.  Here, for the ten update entry points (rl_learn, rl_learn_dueling, rl_learn_prioritized, rl_learn_ppo, rl_learn_td and
their wide entries) on their smallest batches: one update against float64 at other gamma / lmbda / eps_clip / prio_e / prio_a / beta,
Adam at step 10,000 at other lr / beta1 / beta2 / eps, the exact properties of gamma = 0, lr = 0, beta1 = 0 and beta2 = 0, three learners
of pairwise different values in one call against their solo calls, alpha in the three samplers, rl_learn_td_stamp against rl_learn_td,
and the values' way from the public constructors through DeviceLearner and trainer().  tests/test_learn_hyper_cpu.py checks without a
GPU that every value moves the float64 model at least a hundred bars from the default's.  Every figure a bar is held against is
printed before it is asserted, with the entry point's name in front."""
import ctypes as C
import warnings

import numpy as np
import pytest

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_hyper_cases as hc
import learn_perd3qn_cases as kc
import learn_perdqn_cases as tc
import learn_prio_rank_cases as prc
import learn_reference_prioritized_cases as rpc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
ENTRIES = sorted(hc.ENTRIES)
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed", "grad", "loss")
SIDE = {"prioritized": ("priority", "prio_max"), "td": ("priority", "beta_is", "is_weight")}
_rings = {}


def _ring(rows, prob=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture lays one out (count = capacity, ages the rows' or 0)."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    age = rows["ring_age"] if "ring_age" in rows else np.zeros(capacity, np.int32)
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None if prob is None else t(prob, torch.float32), "age": t(age, torch.int32),
            "count": torch.full((1,), capacity, dtype=torch.int64, device=DEV)}


def _ring_of(entry, adam=False):
    """The entry's ring on the device, made once (the update kernels only read it)."""
    key = (hc.ENTRIES[entry][0], adam)
    if key not in _rings:
        i = hc.inputs(entry, adam)
        _rings[key] = _ring(i["rows"], i["prob"])
    return _rings[key]


def _host_pack(flat, kind):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(kind), np.float32)
    assert lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def _set(l, hyper):
    """The hyperparameters as attributes of the learner: struct() and side_struct() pass them on by name."""
    for k, v in hyper.items():
        if k == "beta_is":
            l.beta_is.fill_(v)
        else:
            assert hasattr(l, k), k
            setattr(l, k, v)


def _make(entry, hyper=None, adam=False, n_steps=1, ring=None, target=None, brain=None, batch=None):
    """A DeviceLearner of `entry` on the entry's inputs (learn_hyper_cases.inputs) with an open size gate, gradient and loss rows for
    every Adam step of a call of n_steps, and `hyper` set.  It is made from a brain without arguments, whose values must be the
    defaults the other test files assert (brain: another one)."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    family, keyword, rows = hc.ENTRIES[entry]
    i = hc.inputs(entry, adam)
    kw = {"prioritized": dict(prioritized=True), "ppo": dict(rollout=True), "td": dict(td_priority=True)}.get(family, {})
    if keyword:
        kw[keyword] = rows if batch is None else batch
    l = DeviceLearner(getattr(Models, hc.METHOD[family])() if brain is None else brain, DEV, ring=_ring_of(entry, adam) if ring is None else ring, **kw)
    assert l.entry == entry
    if brain is None:
        for k, v in hc.DEFAULTS[family].items():
            assert (l.beta_is.item() if k == "beta_is" else getattr(l, k)) == v, (entry, k)
        assert l.alpha == 0.6
    if not keyword and brain is None:
        l.batch = rows
    l.min_size = 0
    dev = lambda a: torch.as_tensor(np.array(a, np.float32), device=DEV)  # noqa: E731
    l.params.copy_(dev(i["params"]))
    l.packed.copy_(dev(_host_pack(i["params"], l.kind)))
    if l.target is not None:
        l.target.copy_(dev(i["target"] if target is None else target))
    if family in SIDE:
        l.priority.copy_(dev(i["priority"]))
        l.seen.copy_(l.ring["count"])
    _set(l, hyper or {})
    n_rows = n_steps * (l.k_epoch if family == "ppo" else 1)
    l.grad = torch.zeros((n_rows, l.n_params), dtype=torch.float32, device=DEV)
    l.loss = torch.zeros(n_rows, dtype=torch.float32, device=DEV)
    if family == "td":
        l.is_weight = torch.zeros((n_steps, l.batch), dtype=torch.float32, device=DEV)
    return l


def _learn(worlds, learners, slots, n_steps=1):
    """One call for the learners (all of one entry point) on `slots` ([n_steps][batch], the same table for every learner) -> what each ends on."""
    import torch
    family = learners[0].spec.family
    table = np.stack([np.asarray(slots, np.int32).reshape(n_steps, -1)] * len(learners))
    worlds.learn(learners, n_steps, slots=table, **(dict(gate=False) if family == "ppo" else {}))
    torch.cuda.synchronize()
    worlds.check_error_flag()
    names = tuple(n for n in BUFFERS if n != "target" or family != "ppo") + SIDE.get(family, ())
    return [{k: getattr(l, k).cpu().numpy().copy() for k in names} for l in learners]


def _run(worlds, entry, hyper=None, adam=False, n_steps=1, slots=None, **make):
    l = _make(entry, hyper, adam, n_steps, **make)
    return _learn(worlds, [l], hc.inputs(entry, adam)["slots"] if slots is None else slots, n_steps)[0], l


def _same(a, b, keys, tag):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s" % (tag, k)


def _hold_to_model(entry, r, m, slots, tag, row=0, pri_before=None):
    """The project's bars: every gradient tensor of row `row` within 1e-5 of its largest float64 entry, the loss within relative 1e-5;
    PERD3QN / PERDQN: the batch rows' priorities within 1e-5 of float64 relative to the scale (the largest |q|, |q'| or target), every
    other row's priority unchanged; PERDQN: the importance weights within 1 float32 ulp."""
    family = hc.ENTRIES[entry][0]
    mod = hc.CASES_OF[family]
    got, loss, loss64 = mod.split(r["grad"][row]), float(r["loss"][row]), m["loss"]
    worst = 0.0
    for name, a, b in zip(mod.NAMES, got, m["grads"]):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("%s %s: %-17s max|g| %.4g  error / max|g| %.3g" % (entry, tag, name, np.abs(b).max(), err))
    print("%s %s: worst gradient error / max|g| %.3g (bar 1e-5); loss %.9g (float64 %.9g, relative error %.3g, bar 1e-5)"
          % (entry, tag, worst, loss, loss64, abs(loss - loss64) / abs(loss64)))
    if "prio64" in m:
        perr = float(np.abs(r["priority"][slots] - m["prio64"]).max() / m["scale"])
        print("%s %s: max |priority - float64| / scale %.3g (bar 1e-5; scale %.4g)" % (entry, tag, perr, m["scale"]))
    if "isw" in m:
        w32 = m["isw"].astype(np.float32)
        werr = float((np.abs(r["is_weight"][row] - w32) / np.spacing(w32)).max())
        print("%s %s: importance weights worst %.3g ulp (bar 1); mean %.6g" % (entry, tag, werr, m["isw"].mean()))
    for name, a, b in zip(mod.NAMES, got, m["grads"]):
        assert np.abs(a - b).max() <= hc.BAR * np.abs(b).max(), "%s %s: %s" % (entry, tag, name)
    assert abs(loss - loss64) <= hc.BAR * abs(loss64), "%s %s: loss" % (entry, tag)
    if "prio64" in m:
        assert perr <= hc.BAR, "%s %s: priorities" % (entry, tag)
        if pri_before is not None:
            rest = np.setdiff1d(np.arange(len(pri_before)), slots)
            assert r["priority"][rest].tobytes() == np.asarray(pri_before, np.float32)[rest].tobytes(), "%s %s: a row outside the batch was written" % (entry, tag)
    if "isw" in m:
        assert werr <= 1, "%s %s: importance weights" % (entry, tag)


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


def _values(family):
    return list(hc.GAMMAS[family]) + (list(hc.PPO_VALUES) if family == "ppo" else [])


# ---- 1. one update against float64 at other values ---------------------------------------------------------------------------------
@pytest.mark.parametrize("entry, which", [(e, n) for e in ENTRIES for n in range(len(_values(hc.ENTRIES[e][0])))])
def test_one_update_at_other_values_matches_float64(worlds, entry, which):
    """Trained weights, the float32(0.96875) target, the entry's smallest batch (wide: one row in a second tile), one update at gamma
    0.9 and 1.0 (the two D3QN entries: 0.5 -- from their default 0.99 the step to 1.0 moves their gradient too little to be told from no
    step, tests/test_learn_hyper_cpu.py), PPO also
    at (lmbda, eps_clip) = (0.8, 0.3) and at lmbda = 0, where gl = 0 and the advantage is delta itself, on the wide entry across the
    tile seam: the project's bars against the float64 model at those values; packed is the host packer's of the parameters read back."""
    family = hc.ENTRIES[entry][0]
    values = _values(family)
    v = dict(values[which], **(dict(k_epoch=1) if family == "ppo" else {}))
    hyper = hc.hyper_of(family, **v)
    i = hc.inputs(entry)
    r, l = _run(worlds, entry, hyper)
    tag = " ".join("%s=%g" % kv for kv in sorted(values[which].items()))
    _hold_to_model(entry, r, hc.model(entry, hyper), i["slots"], tag, pri_before=i["priority"])
    assert r["state"].tolist() == [1, 1] and r["params"].tobytes() != i["params"].tobytes()
    assert r["packed"].tobytes() == _host_pack(r["params"], l.kind).tobytes(), entry
    if family == "prioritized":
        assert r["prio_max"][0] == r["priority"].max() > hc.SENTINEL
    if family == "td":
        assert r["beta_is"][0] == 0.4 + 0.001


@pytest.mark.parametrize("entry", ["rl_learn_td", "rl_learn_td_wide"])
def test_two_perdqn_steps_at_other_memory_values_match_float64(worlds, entry):
    """(prio_e, prio_a) = (2.0, 0.4; 0.05 would move the priorities by 4 to 11 bars only), beta_is = 0.7, beta_increment = 0.05, two steps in one call, the second on the first's rows in
    another order: step 0 at beta 0.75 against float64; step 1 at beta 0.8 against float64 from the parameters and priorities a
    one-step call from the same start leaves (the steps are deterministic: its gradient, weights and loss are step 0's bit for bit),
    so its importance weights come from the priorities step 0 wrote at these prio_e and prio_a; beta ends on 0.8 exactly."""
    hyper = hc.hyper_of("td", **hc.TD_VALUES)
    i = hc.inputs(entry)
    s0, s1 = i["slots"], hc.td_second_slots(entry)
    one, _ = _run(worlds, entry, hyper)
    two, l = _run(worlds, entry, hyper, n_steps=2, slots=np.stack([s0, s1]))
    assert two["grad"][0].tobytes() == one["grad"][0].tobytes() and two["is_weight"][0].tobytes() == one["is_weight"][0].tobytes()
    assert two["loss"][0].tobytes() == one["loss"][0].tobytes(), entry
    m0 = hc.model(entry, hyper)
    assert m0["beta"] == 0.75
    _hold_to_model(entry, one, m0, s0, "step 0 (beta 0.75)", pri_before=i["priority"])
    m1 = hc.model(entry, dict(hyper, beta_is=0.75), params=one["params"], priority=one["priority"], slots=s1)
    _hold_to_model(entry, two, m1, s1, "step 1 (beta 0.8)", row=1, pri_before=i["priority"])
    print("%s: beta after one step %.17g, after two %.17g" % (entry, one["beta_is"][0], two["beta_is"][0]))
    assert one["beta_is"][0] == 0.75 and two["beta_is"][0] == min(1.0, 0.75 + 0.05) == 0.8, entry
    assert len(set(one["priority"][s1].tolist())) > 8 and m1["isw"].mean() < 0.95     # (weights that are not all 1)
    assert two["state"].tolist() == [2, 1] and two["packed"].tobytes() == _host_pack(two["params"], l.kind).tobytes()


def test_a_stamped_priority_is_what_rl_learn_td_writes_at_the_same_values(worlds):
    """rl_learn_td_stamp on the whole 1027-row ring at gamma 0.9, prio_e 2.0, prio_a 0.4: the batch rows' stamps equal, bit for bit,
    what rl_learn_td writes for them from the same parameters at the same values (the rule of tests/test_hip_learn_td_stamp.py), lie
    within 1e-5 of float64 relative to the scale, and are not the stamps at the default values."""
    entry = "rl_learn_td"
    hyper = hc.hyper_of("td", gamma=0.9, prio_e=hc.TD_VALUES["prio_e"], prio_a=hc.TD_VALUES["prio_a"])
    i = hc.inputs(entry)
    out = {}
    for tag, h in (("at", hyper), ("default", hc.DEFAULTS["td"])):
        l = _make(entry, h)
        l.priority.fill_(float(hc.SENTINEL))
        l.seen.fill_(0)
        worlds.stamp_td([l])
        out[tag] = l.priority.cpu().numpy().copy()
        worlds.check_error_flag()
        assert int(l.seen.item()) == 1027 and not (out[tag] == hc.SENTINEL).any()
    r, _ = _run(worlds, entry, hyper)
    slots = i["slots"]
    m = hc.model(entry, hyper)
    diff = int((r["priority"][slots].view(np.uint32) != out["at"][slots].view(np.uint32)).sum())
    perr = float(np.abs(out["at"][slots] - m["prio64"]).max() / m["scale"])
    moved = int((out["at"] != out["default"]).sum())
    print("rl_learn_td_stamp: %d of 64 stamps differ in bits from rl_learn_td's write; max |stamp - float64| / scale %.3g (bar 1e-5); %d of 1027 stamps differ from "
          "the default values'" % (diff, perr, moved))
    assert r["priority"][slots].tobytes() == out["at"][slots].tobytes(), "rl_learn_td_stamp"
    assert perr <= hc.BAR and moved >= 1000, "rl_learn_td_stamp"


# ---- 2. Adam at other lr, beta1, beta2, eps ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_adam_at_step_ten_thousand_at_other_values(worlds, entry):
    """state[0] = 9999, learn_d3qn_cases.adam_moments, the fixtures' initial parameters, one step at (lr, beta1, beta2, eps) = (0.002,
    0.8, 0.99, 1e-4): every parameter within 1e-5 lr + 1 ulp of adam64 on the kernel's own gradient with the decimals the float32
    values stand for, m and v within 1 ulp.  The same replay with any one value at its default misses the bound on at least 1 % of the parameters (printed: on most)."""
    import torch
    family = hc.ENTRIES[entry][0]
    hyper = hc.hyper_of(family, **hc.ADAM_VALUES, **(dict(k_epoch=1) if family == "ppo" else {}))
    i = hc.inputs(entry, adam=True)
    m0, v0 = dc.adam_moments(hc.CASES_OF[family].N_PARAMS)
    l = _make(entry, hyper, adam=True)
    l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
    l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
    l.state[0] = 9999
    r = _learn(worlds, [l], i["slots"])[0]
    f64 = lambda x: np.asarray(x, np.float64)  # noqa: E731
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    grad = f64(r["grad"][0])
    d = {k: hc.decimal(np.float32(hyper[k])) for k in hc.ADAM_VALUES}
    assert d == hc.ADAM_VALUES
    p64, m64, v64 = lc.adam64(f64(i["params"]), f64(m0), f64(v0), grad, 10000, d["lr"], d["beta1"], d["beta2"], d["eps"])
    perr, bound = np.abs(r["params"] - p64), hc.adam_bound(r["params"], d["lr"])
    merr, verr = np.abs(r["adam_m"] - m64) / ulp(m64), np.abs(r["adam_v"] - v64) / ulp(v64)
    missed = {}
    for name in sorted(hc.ADAM_VALUES):
        e = dict(d, **{name: hc.DEFAULTS[family][name]})
        missed[name] = int((np.abs(r["params"] - lc.adam64(f64(i["params"]), f64(m0), f64(v0), grad, 10000, e["lr"], e["beta1"], e["beta2"], e["eps"])[0]) > bound).sum())
    print("%s Adam at t = 10000, lr 0.002 beta1 0.8 beta2 0.99 eps 1e-4: worst |p - float64| / (1e-5 lr + 1 ulp) %.3g (%d of %d beyond the bound; largest step %.3g lr); "
          "m: worst %.3g ulp; v: worst %.3g ulp; with one value at its default the parameters beyond the bound: %s"
          % (entry, (perr / bound).max(), int((perr > bound).sum()), perr.size, (np.abs(p64 - i["params"]) / d["lr"]).max(), merr.max(), verr.max(), missed))
    assert r["state"].tolist() == [10000, 1] and grad.any(), entry
    assert (perr <= bound).all(), entry
    assert (merr <= 1).all() and (verr <= 1).all(), entry
    assert min(missed.values()) >= perr.size // 100, entry                               # (the CPU file's criterion: at least 1 %)


# ---- 3. exact properties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_at_gamma_zero_nothing_depends_on_the_next_state(worlds, entry):
    """gamma = 0: a second call whose ring has other (finite) state_prime rows and the opposite done column, and whose target network is
    another one, ends on the same bits in grad, loss, params, adam_m, adam_v, packed and -- PERDQN -- the priorities, weights and beta.
    (PPO has no target; at gamma = 0 gl is 0 too, so done gates nothing.)  PERD3QN's priority is |max_a q'_target(s') - q(s)[a]|
    (PERD3QN.py:110), which holds no gamma: there the second call's priorities must be float64's of ITS inputs, and differ from the
    first's.  At the default gamma the same two calls differ: the changed inputs are read."""
    family = hc.ENTRIES[entry][0]
    i = hc.inputs(entry)
    rows2 = {k: np.array(i["rows"][k]) for k in lc.RING_KEYS + (("ring_age",) if "ring_age" in i["rows"] else ())}
    rows2["ring_state_prime"] = np.ascontiguousarray(rows2["ring_state_prime"][::-1] * np.float32(3.0))
    rows2["ring_done"] = (1 - rows2["ring_done"]).astype(np.uint8)
    ring2 = _ring(rows2, i["prob"])
    target2 = None if i["target"] is None else (i["target"] * np.float32(0.5)).astype(np.float32)
    keys = ("grad", "loss", "params", "adam_m", "adam_v", "packed") + {"td": ("priority", "beta_is", "is_weight")}.get(family, ())
    out = {}
    for gamma in (0.0, hc.DEFAULTS[family]["gamma"]):
        hyper = hc.hyper_of(family, gamma=gamma)
        a, _ = _run(worlds, entry, hyper)
        b, _ = _run(worlds, entry, hyper, ring=ring2, target=target2)
        out[gamma] = (a, b)
    a, b = out[0.0]
    differ = [k for k in keys if a[k].tobytes() != b[k].tobytes()]
    a9, b9 = out[hc.DEFAULTS[family]["gamma"]]
    print("%s gamma 0: buffers that differ between the two calls: %s; at the default gamma: %s" % (entry, differ, [k for k in keys if a9[k].tobytes() != b9[k].tobytes()]))
    assert not differ, "%s: %s" % (entry, differ)
    assert a["grad"].any() and a["params"].tobytes() != i["params"].tobytes()
    assert a9["grad"].tobytes() != b9["grad"].tobytes() and a9["params"].tobytes() != b9["params"].tobytes(), entry
    if family == "prioritized":
        m = hc.model(entry, hc.hyper_of(family, gamma=0.0), rows=rows2, target=target2)
        perr = float(np.abs(b["priority"][i["slots"]] - m["prio64"]).max() / m["scale"])
        print("%s gamma 0: the second call's priorities against float64 of its own inputs: %.3g of the scale (bar 1e-5)" % (entry, perr))
        assert perr <= hc.BAR and a["priority"].tobytes() != b["priority"].tobytes(), entry


@pytest.mark.parametrize("entry", ENTRIES)
def test_at_lr_zero_the_parameters_keep_their_bits(worlds, entry):
    """lr = 0: params and packed keep their bits; adam_m, adam_v, state and grad are those of the same call at the default lr."""
    family = hc.ENTRIES[entry][0]
    i = hc.inputs(entry)
    more = dict(k_epoch=1) if family == "ppo" else {}
    zero, l = _run(worlds, entry, hc.hyper_of(family, lr=0.0, **more))
    base, _ = _run(worlds, entry, hc.hyper_of(family, **more))
    assert zero["params"].tobytes() == np.asarray(i["params"], np.float32).tobytes(), entry
    assert zero["packed"].tobytes() == _host_pack(i["params"], l.kind).tobytes(), entry
    _same(zero, base, ("adam_m", "adam_v", "state", "grad", "loss"), entry)
    assert base["params"].tobytes() != zero["params"].tobytes() and zero["adam_m"].any() and zero["adam_v"].any() and zero["state"].tolist() == [1, 1]


@pytest.mark.parametrize("entry", ENTRIES)
def test_at_beta_zero_the_moments_are_the_gradient_and_its_square(worlds, entry):
    """From zero moments, beta1 = 0: adam_m equals grad bit for bit; beta2 = 0: adam_v equals float32(float64(grad) ** 2) bit for bit."""
    family = hc.ENTRIES[entry][0]
    more = dict(k_epoch=1) if family == "ppo" else {}
    r1, _ = _run(worlds, entry, hc.hyper_of(family, beta1=0.0, **more))
    r2, _ = _run(worlds, entry, hc.hyper_of(family, beta2=0.0, **more))
    want_v = (r2["grad"][0].astype(np.float64) ** 2).astype(np.float32)
    print("%s: beta1 = 0: %d of %d adam_m differ in bits from grad; beta2 = 0: %d adam_v differ from float32(float64(grad)^2)"
          % (entry, int((r1["adam_m"].view(np.uint32) != r1["grad"][0].view(np.uint32)).sum()), r1["adam_m"].size,
             int((r2["adam_v"].view(np.uint32) != want_v.view(np.uint32)).sum())))
    assert r1["grad"][0].any() and r1["grad"].tobytes() == r2["grad"].tobytes()
    assert r1["adam_m"].tobytes() == r1["grad"][0].tobytes(), "%s: beta1 = 0" % entry
    assert r2["adam_v"].tobytes() == want_v.tobytes(), "%s: beta2 = 0" % entry
    assert r1["adam_v"].tobytes() != r2["adam_v"].tobytes() and r1["adam_m"].tobytes() != r2["adam_m"].tobytes()   # (at step 1 the betas cancel in the parameters)


# ---- 4. hyperparameters are per learner --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_three_learners_of_different_values_each_end_on_the_bits_of_their_solo_call(worlds, entry):
    """One call with three learners on the same inputs whose (lr, gamma, beta1, beta2, eps) -- PPO: lmbda, eps_clip, k_epoch too; PERDQN:
    prio_e, prio_a, beta_increment too -- differ pairwise, the default set last: each ends on the bits of its solo call in every buffer,
    the gradient rows, the loss and the memory's tensors; the three results differ from each other."""
    family = hc.ENTRIES[entry][0]
    sets = hc.learners_of_one_call(family)
    slots = hc.inputs(entry)["slots"]
    together = _learn(worlds, [_make(entry, h) for h in sets], slots)
    alone = [_learn(worlds, [_make(entry, h)], slots)[0] for h in sets]
    for n, (a, b) in enumerate(zip(together, alone)):
        differ = [k for k in a if a[k].tobytes() != b[k].tobytes()]
        print("%s learner %d of 3: buffers that differ from its solo call: %s" % (entry, n, differ))
    for n, (a, b) in enumerate(zip(together, alone)):
        _same(a, b, tuple(a), "%s learner %d" % (entry, n))
        assert a["grad"].shape[0] == (sets[n]["k_epoch"] if family == "ppo" else 1) and a["grad"][-1].any()
    for x, y in ((0, 1), (0, 2), (1, 2)):
        assert alone[x]["params"].tobytes() != alone[y]["params"].tobytes() and alone[x]["adam_v"].tobytes() != alone[y]["adam_v"].tobytes()
        assert alone[x]["grad"][0].tobytes() != alone[y]["grad"][0].tobytes(), entry    # (gamma)


def _drawer(alpha, calls=hc.DRAW_CALLS):
    """A narrow PERD3QN learner on the 257-row edge ring with its priorities, nothing new to stamp, at call `calls`."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    rows, keys, pri = hc.draw_case()
    if "draw" not in _rings:
        _rings["draw"] = _ring(rows)
    l = DeviceLearner(Models.PERD3QN(), DEV, ring=_rings["draw"], prioritized=True)
    assert l.entry == "rl_learn_prioritized" and l.alpha == 0.6 and l.batch == 64
    l.min_size = 0
    l.priority.copy_(torch.as_tensor(pri, device=DEV))
    l.seen.copy_(l.ring["count"])
    l.state[1] = calls
    l.alpha = alpha
    return l


def _draw(worlds, learners, rank):
    import torch
    got = (worlds.draw_prioritized_rank if rank else worlds.draw_prioritized)(learners, hc.DRAW_STEPS)
    torch.cuda.synchronize()
    worlds.check_error_flag()
    assert tuple(got.shape) == (len(learners), hc.DRAW_STEPS, 64)
    return got.cpu().numpy().reshape(len(learners), -1), [l.weight.cpu().numpy().copy() for l in learners]


def _hold_draw(name, l, brain, got, w, alpha, rank):
    """One learner's table and weights against the host rules at `alpha`, at position `brain` of its call."""
    from reinlife_amd import _lib
    rows, keys, pri = hc.draw_case()
    w64 = hc.draw_weights64(alpha)
    live = pri > 0
    werr = float((np.abs(w[live] - w64[live]) / w64[live]).max())
    if rank:
        want, _, order, cum = prc.host_draw(keys, w, SEED, brain, hc.DRAW_CALLS, _lib.SITE_LEARN_PRIO, hc.DRAW_STEPS, 64, False)
        print("%s alpha %.1f position %d: max relative weight error %.3g (bar 1e-6); %d of 128 draws differ from the rank rule on the device's weights"
              % (name, alpha, brain, werr, int((got != want).sum())))
        assert np.array_equal(l.rank_order.cpu().numpy(), order) and l.rank_cum.cpu().numpy().tobytes() == cum.tobytes(), name
    else:
        want, gaps = kc.host_draw64(keys, w, SEED, brain, hc.DRAW_CALLS, 128)
        host = kc.host_draw(keys, pri, SEED, brain, hc.DRAW_CALLS, 128, alpha=alpha)
        print("%s alpha %.1f position %d: max relative weight error %.3g (bar 1e-6); smallest gap %.3g; %d of 128 draws differ from the float64 race on the device's "
              "weights, %d from the float32 host model" % (name, alpha, brain, werr, gaps.min(), int((got != want).sum()), int((got != host).sum())))
        assert gaps.min() >= 1e-4, name
        assert np.array_equal(got, host), "%s: learn_perd3qn_cases.host_draw(..., alpha=%g)" % (name, alpha)
    assert werr <= 1e-6 and not w[~live].any(), name
    if alpha == 1.0:
        assert w.tobytes() == pri.tobytes(), "%s: at alpha 1 the weight is the priority" % name
    assert np.array_equal(got, want), name
    assert live[got].all() and np.array_equal(l.keys.cpu().numpy().view(np.uint64), keys)
    assert l.priority.cpu().numpy().tobytes() == pri.tobytes()


@pytest.mark.parametrize("rank", [False, True], ids=["rl_learn_prioritized_draw", "rl_learn_prioritized_draw_rank"])
def test_three_alphas_in_one_draw_call(worlds, rank):
    """alpha = 0.3, 1.0 and 0.6 in one call: every learner's weights are those of its solo call bit for bit, its slot table that of the
    call in which all three learners have ITS alpha (a table depends on the learner's position in the call), and both are the host
    rules' at its alpha and position."""
    name = "rl_learn_prioritized_draw_rank" if rank else "rl_learn_prioritized_draw"
    learners = [_drawer(a) for a in hc.ALPHAS]
    got, w = _draw(worlds, learners, rank)
    for n, alpha in enumerate(hc.ALPHAS):
        _hold_draw(name, learners[n], n, got[n], w[n], alpha, rank)
        same = [_drawer(alpha) for _ in hc.ALPHAS]
        got_same, w_same = _draw(worlds, same, rank)
        solo_w = _draw(worlds, [_drawer(alpha)], rank)[1][0]
        print("%s learner %d (alpha %.1f): %d of 128 slots differ from the call of three at its alpha; %d weights differ in bits from its solo call"
              % (name, n, alpha, int((got[n] != got_same[n]).sum()), int((w[n].view(np.uint32) != solo_w.view(np.uint32)).sum())))
        assert np.array_equal(got[n], got_same[n]) and w[n].tobytes() == w_same[n].tobytes() == solo_w.tobytes(), "%s learner %d" % (name, n)
    assert w[0].tobytes() != w[1].tobytes() != w[2].tobytes() and not np.array_equal(got[0], got[1])


# ---- 5. alpha in the three samplers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [1.0, 0.3])
@pytest.mark.parametrize("rank", [False, True], ids=["rl_learn_prioritized_draw", "rl_learn_prioritized_draw_rank"])
def test_the_draws_take_alpha_from_the_learner(worlds, rank, alpha):
    """The 257-row edge ring at call 3, two steps of 64: weight = priority^alpha within relative 1e-6 of float64 (alpha = 1: the
    priority's bits), exactly 0 for a zero priority; the race draw's slots are the float64 race's on the device's own weights, with
    the 1e-4 gap asserted first (tests/test_hip_learn_edges.py's rule, and without a GPU in tests/test_learn_hyper_cpu.py); the rank
    draw's order, cumulative sums and slots are learn_prio_rank_cases.host_draw's bit for bit.  The table is not the one at 0.6."""
    name = "rl_learn_prioritized_draw_rank" if rank else "rl_learn_prioritized_draw"
    l = _drawer(alpha)
    got, w = _draw(worlds, [l], rank)
    _hold_draw(name, l, 0, got[0], w[0], alpha, rank)
    at_default, _ = _draw(worlds, [_drawer(0.6)], rank)
    print("%s alpha %.1f: %d of 128 slots differ from the table at alpha 0.6" % (name, alpha, int((got[0] != at_default[0]).sum())))
    assert (got[0] != at_default[0]).sum() >= 5, name


@pytest.mark.parametrize("n", hc.CHOICE_SIZES)
def test_the_choice_takes_alpha_from_the_learner(worlds, n):
    """rl_learn_prioritized_choice with three learners of alpha 1.0, 0.25 and 0.6 in one call on memories of n = 65 and 1000 rows (stored
    n + 5, a ring of n + 7): numpy's indices at each learner's alpha for 64 uniforms that numpy's arithmetic keeps SNAPSHOT_MARGIN
    inside their brackets, the ring slots of those indices, the brackets within 2^-21 of numpy's."""
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.learn_reference import memory_slots
    alphas = hc.CHOICE_ALPHAS + (float(rpc.ALPHA),)
    cases = [hc.choice_case(n, n + 5, a) for a in alphas]
    k = len(cases)
    learners, sides, draws, keep = (_lib.Learner * k)(), (_lib.Prio * k)(), (_lib.PrioChoice * k)(), []
    for j, c in enumerate(cases):
        t = dict(prio=torch.as_tensor(c["by_slot"], device=DEV), u=torch.as_tensor(c["u"], device=DEV),
                 indices=torch.full((64,), -1, dtype=torch.int32, device=DEV), slots=torch.full((64,), -1, dtype=torch.int32, device=DEV),
                 bracket=torch.full((64, 2), -7.0, dtype=torch.float64, device=DEV),
                 work=torch.empty(max(int(worlds.lib.rl_learn_prioritized_choice_work_bytes(n)), 256), dtype=torch.uint8, device=DEV))
        keep.append(t)
        learners[j].kind = _lib.PERD3QN
        sides[j].priority, sides[j].alpha = t["prio"].data_ptr(), c["alpha"]
        draws[j] = _lib.PrioChoice(n, c["ring_rows"], c["stored"], 64, t["u"].data_ptr(), t["indices"].data_ptr(), t["slots"].data_ptr(),
                                   t["bracket"].data_ptr(), t["work"].data_ptr())
    _lib.check(worlds.lib.rl_learn_prioritized_choice(worlds.handle, learners, sides, draws, k, worlds._stream()), "rl_learn_prioritized_choice")
    torch.cuda.synchronize()
    worlds.check_error_flag()
    for c, t in zip(cases, keep):
        idx, slots, br = t["indices"].cpu().numpy(), t["slots"].cpu().numpy(), t["bracket"].cpu().numpy()
        worst = float(np.abs(br - c["bracket"]).max())
        print("rl_learn_prioritized_choice n %d alpha %.2f: %d of 64 indices differ from numpy's; largest |bracket - numpy's| %.3g (bar 2^-21 = %.3g)"
              % (n, c["alpha"], int((idx != c["idx"]).sum()), worst, 2.0 ** -21))
        assert idx.tolist() == c["idx"].tolist(), "rl_learn_prioritized_choice alpha %g" % c["alpha"]
        assert slots.tolist() == memory_slots(c["stored"], n, c["ring_rows"], c["idx"]).tolist()
        assert (c["prio"][idx] > 0).all() and worst <= 2.0 ** -21, "rl_learn_prioritized_choice alpha %g" % c["alpha"]
    assert cases[0]["idx"].tolist() != cases[1]["idx"].tolist() != cases[2]["idx"].tolist()


# ---- 6. the Python layer -----------------------------------------------------------------------------------------------------------
LAYER = [
    ("rl_learn", "DQN", dict(learning_rate=3e-4), dict(lr=3e-4), 32),
    ("rl_learn_dueling", "D3QN", dict(gamma=0.9, learning_rate=3e-4, batch_size=48), dict(lr=3e-4, gamma=0.9), 48),
    ("rl_learn_prioritized", "PERD3QN", dict(gamma=0.9, learning_rate=3e-4, batch_size=48), dict(lr=3e-4, gamma=0.9), 48),
    ("rl_learn_ppo", "PPO", dict(learning_rate=1e-4, gamma=0.9, lmbda=0.8, eps_clip=0.3, k_epoch=5), dict(lr=1e-4, gamma=0.9, lmbda=0.8, eps_clip=0.3, k_epoch=5), 32),
    ("rl_learn_td", "PERDQN", dict(gamma=0.9, learning_rate=3e-4, batch_size=48), dict(lr=3e-4, gamma=0.9), 48),
]


@pytest.mark.parametrize("entry, method, ctor, changed, batch", LAYER, ids=[c[1] for c in LAYER])
def test_the_constructors_values_reach_the_structs_and_the_kernel(worlds, entry, method, ctor, changed, batch):
    """A DeviceLearner made from the public constructor with other values: struct() and the side struct carry them as float32, and one
    update through DeviceWorlds.learn on the entry's trained-weight inputs meets the bars against float64 at those values (PPO: the
    first of its five epochs; its loss and gradient rows are one per epoch)."""
    from reinlife_amd import Models, _lib
    family = hc.ENTRIES[entry][0]
    hyper = hc.hyper_of(family, **changed)
    brain = getattr(Models, method)(**ctor)
    l = _make(entry, brain=brain, batch=batch, n_steps=1)
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    s = l.struct()
    got = dict(lr=s.lr, gamma=s.gamma, beta1=s.beta1, beta2=s.beta2, eps=s.eps, batch=s.batch)
    want = dict(lr=f32(hyper["lr"]), gamma=f32(hyper["gamma"]), beta1=f32(0.9), beta2=f32(0.999), eps=f32(1e-8), batch=batch)
    if family == "ppo":
        side = l.ppo_struct()
        got.update(lmbda=side.lmbda, eps_clip=side.eps_clip, k_epoch=side.k_epoch)
        want.update(lmbda=f32(0.8), eps_clip=f32(0.3), k_epoch=5)
    elif family == "td":
        side = l.td_struct()
        got.update(prio_e=side.prio_e, prio_a=side.prio_a, beta_increment=side.beta_increment, p_new=side.p_new)
        want.update(prio_e=f32(0.01), prio_a=f32(0.6), beta_increment=0.001, p_new=float(tc.golden()["p_new"]))
    elif family == "prioritized":
        got.update(alpha=l.prio_struct().alpha)
        want.update(alpha=f32(0.6))
    print("%s from Models.%s(%s): struct fields %s" % (entry, method, ", ".join("%s=%g" % kv for kv in ctor.items()), got))
    assert got == want, entry
    assert s.kind == getattr(_lib, method) and l.batch == batch
    i = hc.inputs(entry)
    slots = np.ascontiguousarray(i["slots"][:batch])
    r = _learn(worlds, [l], slots)[0]
    _hold_to_model(entry, r, hc.model(entry, hyper, slots=slots), slots, "from Models.%s(...)" % method, pri_before=i["priority"])
    steps = 5 if family == "ppo" else 1
    assert r["state"].tolist() == [steps, 1] and r["grad"].shape[0] == steps and r["grad"][-1].any()
    assert r["packed"].tobytes() == _host_pack(r["params"], l.kind).tobytes()


def _train(**d3qn):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.D3QN(exploration=20, soft_update_freq=40, **d3qn)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return trainer(brains, n_episodes=60, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device", save=False,
                       print_results=False, learn_kinds=("DQN", "D3QN"))


def test_trainer_trains_the_d3qn_brain_at_its_constructors_values():
    """tests/test_hip_learn_d3qn.py's run of 60 episodes with Models.D3QN(gamma=0.9, learning_rate=3e-4, batch_size=48): the learner
    carries those values, trains, and ends elsewhere than the same run with Models.D3QN()'s defaults (same seed, same initial weights)."""
    env = _train(gamma=0.9, learning_rate=3e-4, batch_size=48)
    l = env.learners[1]
    print("trainer: D3QN learner gamma %g lr %g batch %d, state %s" % (l.gamma, l.lr, l.batch, l.state.cpu().tolist()))
    assert (l.entry, l.gamma, l.lr, l.batch) == ("rl_learn_dueling", 0.9, 3e-4, 48)
    assert int(l.state[0].item()) > 0
    env.worlds.check_error_flag()
    base = _train()
    b = base.learners[1]
    assert (b.gamma, b.lr, b.batch) == (0.99, 1e-3, 64) and b.state.cpu().tolist() == l.state.cpu().tolist()
    assert l.params.cpu().numpy().tobytes() != b.params.cpu().numpy().tobytes()
    assert np.isfinite(l.params.cpu().numpy()).all()
