"""Shared by tests/test_learn_hyper_cpu.py and tests/test_hip_learn_hyper.py: the ten update entry points at hyperparameters other than
the reference's defaults -- per entry point its smallest batch (narrow: 32 or 64 rows; wide: one batch with a one-row second tile), the
trained-weight inputs the edge tests use, the float64 models of the suite with the hyperparameters passed through by name, the values
tested, and the sensitivity of every comparison to every single value (a comparison has power only if the default would fail it).
Nothing here needs a GPU."""
import numpy as np

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as kc
import learn_perdqn_cases as tc
import learn_ppo_cases as pc
import learn_reference_prioritized_cases as rpc

# entry point -> (family, the DeviceLearner keyword of its batch or None, rows of the batch)
ENTRIES = {
    "rl_learn": ("dqn", None, 32), "rl_learn_wide": ("dqn", "wide_batch", 33),
    "rl_learn_dueling": ("dueling", None, 64), "rl_learn_dueling_wide": ("dueling", "dueling_batch", 65),
    "rl_learn_prioritized": ("prioritized", None, 64), "rl_learn_prioritized_wide": ("prioritized", "prioritized_batch", 65),
    "rl_learn_ppo": ("ppo", None, 32), "rl_learn_ppo_wide": ("ppo", "rollout_batch", 33),
    "rl_learn_td": ("td", None, 64), "rl_learn_td_wide": ("td", "td_batch", 65),
}
METHOD = {"dqn": "DQN", "dueling": "D3QN", "prioritized": "PERD3QN", "ppo": "PPO", "td": "PERDQN"}
CASES_OF = {"dqn": lc, "dueling": dc, "prioritized": dc, "ppo": pc, "td": tc}
ADAM_DEFAULT = dict(beta1=0.9, beta2=0.999, eps=1e-8)
DEFAULTS = {   # what DeviceLearner gives a brain made without arguments (reinlife_amd/learn.py)
    "dqn": dict(lr=0.0005, gamma=0.98, **ADAM_DEFAULT), "dueling": dict(lr=1e-3, gamma=0.99, **ADAM_DEFAULT),
    "prioritized": dict(lr=1e-3, gamma=0.99, **ADAM_DEFAULT),
    "ppo": dict(lr=0.0005, gamma=0.98, lmbda=0.95, eps_clip=0.1, k_epoch=3, **ADAM_DEFAULT),
    "td": dict(lr=1e-3, gamma=0.99, prio_e=0.01, prio_a=0.6, beta_is=0.4, beta_increment=0.001, **ADAM_DEFAULT),
}
# gamma 0.9 and 1.0 everywhere but on the two D3QN entry points: from their default 0.99 the step to 1.0 moves the trained D3QN gradient by
# 2.6e-4 (rl_learn_dueling) and 1.6e-4 (rl_learn_dueling_wide) of its largest entry, under the 1e-3 a value needs to be worth testing
# (tests/test_learn_hyper_cpu.py), so D3QN takes 0.5 in 1.0's place.  PERD3QN (3.1e-3, wide 1.3e-3) and PERDQN (7.1e-3, wide 3.6e-3) keep 1.0.
GAMMAS = {"dqn": (dict(gamma=0.9), dict(gamma=1.0)), "ppo": (dict(gamma=0.9), dict(gamma=1.0)),
          "dueling": (dict(gamma=0.9), dict(gamma=0.5)), "prioritized": (dict(gamma=0.9), dict(gamma=1.0)), "td": (dict(gamma=0.9), dict(gamma=1.0))}
PPO_VALUES = (dict(lmbda=0.8, eps_clip=0.3), dict(lmbda=0.0))
# over two steps of one call.  prio_e is 2.0, not 0.05: from 0.01 the step to 0.05 moves the written priorities by 4 to 11 bars
# only, and the priorities are the one figure held to a float64 model that sees prio_e; 2.0 moves them by 167 (wide: 196) bars.
TD_VALUES = dict(prio_e=2.0, prio_a=0.4, beta_is=0.7, beta_increment=0.05)
ADAM_VALUES = dict(lr=0.002, beta1=0.8, beta2=0.99, eps=1e-4)
# three learners of one call, pairwise different, the default set LAST (the family's own values are added by learners_of_one_call)
PER_LEARNER = (dict(lr=0.002, gamma=0.9, beta1=0.8, beta2=0.99, eps=1e-4), dict(lr=3e-4, gamma=0.95, beta1=0.85, beta2=0.995, eps=1e-6), dict())
PER_LEARNER_PPO = (dict(lmbda=0.8, eps_clip=0.3, k_epoch=2), dict(lmbda=0.5, eps_clip=0.35, k_epoch=1), dict())   # (no bound on a ratio of the rollout)
PER_LEARNER_TD = (dict(prio_e=2.0, prio_a=0.4, beta_increment=0.05), dict(prio_e=0.02, prio_a=0.8, beta_increment=0.01), dict())
ALPHAS = (0.3, 1.0, 0.6)            # the three draws' learners of one call, the default last
BAR = 1e-5                          # the project's bar on a gradient tensor (of its largest float64 entry), a loss (relative) and a priority (of the scale)
POWER = 100.0                       # a value is tested only where the default would miss the bar by this factor
SENTINEL = np.float32(2.0 ** -20)   # the priority of every row of a PERD3QN memory before the call
DRAW_ROWS, DRAW_CALLS, DRAW_STEPS = 257, 3, 2   # the 257-row edge ring of tests/test_hip_learn_edges.py, at call 3, two steps of 64
_inputs, _models = {}, {}


def hyper_of(family, **changed):
    h = dict(DEFAULTS[family])
    assert set(changed) <= set(h), (family, changed)
    h.update(changed)
    return h


def decimal(x):
    """The decimal a float32 hyperparameter stands for (include/reinlife_hip.h, learn_decimal): what Adam's model takes."""
    return float("%.7g" % np.float32(x))


def learners_of_one_call(family):
    """The three hyperparameter sets of one call: pairwise different in every value the family has, the default set last."""
    more = {"ppo": PER_LEARNER_PPO, "td": PER_LEARNER_TD}.get(family, (dict(), dict(), dict()))
    sets = [hyper_of(family, **a, **b) for a, b in zip(PER_LEARNER, more)]
    assert sets[2] == DEFAULTS[family]
    for k in sets[0]:
        if k != "beta_is":
            assert len({s[k] for s in sets}) == 3, k
    return sets


def inputs(entry, adam=False):
    """The inputs of `entry`'s one batch: dict(params, target, rows (the host ring), prob, priority, slots).  adam=False: the
    trained-weight cases of the edge tests (learn_cases.pretrained with the float32(0.96875) target, learn_ppo_cases.edge_case(),
    learn_perdqn_cases.edge_case(); DQN, D3QN, PERD3QN on their fixtures' rings).  adam=True: the fixtures' initial parameters on the
    fixtures' rings, the setting of test_adam_at_step_ten_thousand_on_moments_that_are_not_zero.  The narrow slots are the fixtures' /
    the edge cases' first batch, the wide ones RandomState(batch) draws from the same ring.  Made once, read-only."""
    key = (entry, adam)
    if key in _inputs:
        return _inputs[key]
    family, _, batch = ENTRIES[entry]
    wide = ENTRIES[entry][1] is not None
    out = dict(prob=None, priority=None, target=None)
    if family in ("dqn", "dueling", "prioritized"):
        mod = CASES_OF[family]
        g = mod.golden()
        out["rows"] = g
        if adam:
            out["params"], out["target"] = g["init"], (g["init"] if family == "dqn" else g["target_init"])
        else:
            out["params"], out["target"] = lc.pretrained(METHOD[family])
        rows = g["ring_state"].shape[0]
        out["slots"] = np.random.RandomState(batch).randint(0, rows, batch).astype(np.int32) if wide else g["slots"][0][:batch].astype(np.int32)
        if family == "prioritized":
            out["priority"] = np.full(rows, SENTINEL, np.float32)
    elif family == "ppo":
        if adam:
            g = pc.golden()
            out.update(params=g["init"], rows=g, prob=g["prob"])
            first = pc.rollouts(g)[0]
            out["slots"] = np.concatenate([first, first[:1]]) if wide else first
        else:
            w, rows, prob, rollouts = pc.edge_case()
            out.update(params=w, rows=rows, prob=prob)
            out["slots"] = np.random.RandomState(100 + batch).randint(0, 1027, batch).astype(np.int32) if wide else rollouts[0]
    else:
        if adam:
            g, p = dc.golden(), tc.golden()
            out.update(params=p["init"], target=p["target_init"], rows=g, priority=p["prio_init"])
            out["slots"] = np.random.RandomState(batch).randint(0, 96, batch).astype(np.int32) if wide else g["slots"][0].astype(np.int32)
        else:
            w, tgt, rows, pri, batches = tc.edge_case()
            out.update(params=w, target=tgt, rows=rows, priority=pri)
            out["slots"] = np.random.RandomState(batch).randint(0, 1027, batch).astype(np.int32) if wide else batches[0]
    assert len(out["slots"]) == batch
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _inputs[key] = out
    return out


def model(entry, hyper, adam=False, params=None, target=None, priority=None, slots=None, rows=None):
    """One update of `entry` in float64 at `hyper` -> dict(loss, grads, names, and per family prio64 (the batch rows' new priorities),
    scale (what a priority's error is relative to), isw (PERDQN's importance weights), beta (after the step), mid (PPO's intermediates)).
    params / target / priority / slots / rows: instead of inputs(entry)'s.  The models are the suite's own (learn_cases.grads64,
    learn_d3qn_cases.grads64, learn_perd3qn_cases.priorities, learn_ppo_cases.grads_by_hand, learn_perdqn_cases.step / is_weights)."""
    family = ENTRIES[entry][0]
    i = inputs(entry, adam)
    memo = None
    if all(x is None for x in (params, target, priority, slots, rows)):
        memo = (entry, adam, tuple(sorted(hyper.items())))
        if memo in _models:
            return _models[memo]
    w = i["params"] if params is None else params
    tgt = i["target"] if target is None else target
    pri = i["priority"] if priority is None else priority
    slots = i["slots"] if slots is None else slots
    rows = i["rows"] if rows is None else rows
    mod = CASES_OF[family]
    out = dict(names=mod.NAMES)
    if family in ("dqn", "dueling", "prioritized"):
        out["loss"], out["grads"] = mod.grads64(w, tgt, rows, slots, hyper["gamma"])
        if family == "prioritized":
            p64, q, qn = kc.priorities(w, tgt, rows, slots)
            out["prio64"], out["scale"] = p64, float(max(np.abs(q).max(), np.abs(qn).max()))
    elif family == "ppo":
        out["loss"], out["grads"], out["mid"] = pc.grads_by_hand(w, pc.rows_of(rows, i["prob"], slots), hyper["gamma"], hyper["lmbda"], hyper["eps_clip"])
    else:
        beta = min(1.0, hyper["beta_is"] + hyper["beta_increment"])
        isw = tc.is_weights(pri[slots], beta)
        out["loss"], out["grads"], out["prio64"], pred, tq = tc.step(w, tgt, rows, slots, isw, hyper["gamma"], prio_e=hyper["prio_e"], prio_a=hyper["prio_a"])
        out["isw"], out["beta"] = isw, beta
        out["scale"] = float(max(np.abs(tc.q_values(w, rows["ring_state"][slots])).max(), np.abs(tc.q_values(tgt, rows["ring_state_prime"][slots])).max(),
                                 np.abs(tq).max()))
    if memo is not None:
        _models[memo] = out
    return out


def flat(grads):
    return np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in grads])


def gradient_difference(a, b):
    """The largest, over the tensors, of max |a - b| / max |b|: what the bar of a gradient comparison is held against."""
    return max(float(np.abs(x - y).max() / np.abs(y).max()) for x, y in zip(a["grads"], b["grads"]))


def td_second_slots(entry):
    """The second step's minibatch of the two-step PERDQN call: the first step's rows in another order, so that every importance weight
    of the second step comes from a priority the first step wrote."""
    return np.ascontiguousarray(np.roll(inputs(entry)["slots"], 7))


def td_two_steps64(entry, hyper):
    """The two steps of one rl_learn_td call in float64 (Adam by adam64 between them, the target left alone) -> the two model dicts."""
    i = inputs(entry)
    one = model(entry, hyper)
    g = flat(one["grads"])
    p1 = lc.adam64(np.asarray(i["params"], np.float64), np.zeros_like(g), np.zeros_like(g), g, 1, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"])[0]
    two = model(entry, dict(hyper, beta_is=one["beta"]), params=p1, priority=_written(i, one), slots=td_second_slots(entry))
    return one, two


def _written(i, one):
    pri = np.array(i["priority"], np.float64)
    pri[i["slots"]] = one["prio64"]
    return pri


def td_power(entry, name, value):
    """How far the default of ONE PERDQN value leaves the figures the GPU test of the two-step call compares from their models at
    `value`, each in units of its bar: gradients (1e-5 of a tensor's largest entry), priorities (1e-5 of the scale), importance weights
    (1 float32 ulp) -> dict(grad, priority, is_weight).  Only what that test holds a kernel to counts: step 0 against its float64
    model; step 1 against the float64 model of the parameters and priorities THE DEVICE holds after step 0 at beta 0.75 -- so both of
    step 1's models here start from the same state (the float64 chain's at `value`) and differ in the one value alone, and what a
    wrong value does to step 1 THROUGH the priorities step 0 wrote is not counted: the kernel's own priorities would feed the model."""
    at = hyper_of("td", **TD_VALUES)
    was = dict(at, **{name: DEFAULTS["td"][name]})
    i = inputs(entry)
    one, two = td_two_steps64(entry, at)
    state = dict(params=lc.adam64(np.asarray(i["params"], np.float64), 0.0, 0.0, flat(one["grads"]), 1, at["lr"], at["beta1"], at["beta2"], at["eps"])[0],
                 priority=_written(i, one), slots=td_second_slots(entry))
    pairs = [(one, model(entry, was)), (two, model(entry, dict(was, beta_is=one["beta"]), **state))]
    out = dict(grad=0.0, priority=0.0, is_weight=0.0)
    for a, b in pairs:
        out["grad"] = max(out["grad"], gradient_difference(b, a) / BAR)
        out["priority"] = max(out["priority"], float(np.abs(a["prio64"] - b["prio64"]).max() / (BAR * a["scale"])))
        out["is_weight"] = max(out["is_weight"], float((np.abs(a["isw"] - b["isw"]) / np.spacing(a["isw"].astype(np.float32)).astype(np.float64)).max()))
    return out


def adam_case(entry):
    """Adam's inputs at step 10,000: (p, m, v as float64 from the fixtures' initial parameters and learn_d3qn_cases.adam_moments, the
    float64 gradient of the batch at the default hyperparameters -- on the device the kernel's own gradient takes its place)."""
    i = inputs(entry, adam=True)
    family = ENTRIES[entry][0]
    m0, v0 = dc.adam_moments(CASES_OF[family].N_PARAMS)
    g = flat(model(entry, DEFAULTS[family], adam=True)["grads"])
    return np.asarray(i["params"], np.float64), m0.astype(np.float64), v0.astype(np.float64), g


def adam_bound(p32, lr):
    """1e-5 lr + 1 float32 ulp of the parameter."""
    return 1e-5 * lr + np.spacing(np.abs(np.asarray(p32, np.float32))).astype(np.float64)


def adam_at(entry, hyper, t=10000):
    p, m, v, g = adam_case(entry)
    return lc.adam64(p, m, v, g, t, decimal(hyper["lr"]), decimal(hyper["beta1"]), decimal(hyper["beta2"]), decimal(hyper["eps"]))


def adam_power(entry, name):
    """The share of the parameters that the default of ONE of Adam's four values leaves at least 100 bounds from the step at ADAM_VALUES."""
    family = ENTRIES[entry][0]
    at = hyper_of(family, **ADAM_VALUES)
    p_at = adam_at(entry, at)[0]
    p_was = adam_at(entry, dict(at, **{name: DEFAULTS[family][name]}))[0]
    return float((np.abs(p_at - p_was) >= POWER * adam_bound(p_at, ADAM_VALUES["lr"])).mean())


# ---- the draws ----
def draw_case():
    """(rows, content keys, priorities) of the 257-row edge ring: learn_cases.edge_ring_rows(1027)[:257] with its ages, priorities
    learn_perd3qn_cases.edge_priorities(257) (random^3 * 4, every 7th row 0)."""
    if "draw" not in _inputs:
        rows = lc.edge_ring_rows(1027, 11)
        keys = kc.content_keys(rows, 1027, rows["ring_age"])[:DRAW_ROWS]
        _inputs["draw"] = ({k: v[:DRAW_ROWS] for k, v in rows.items()}, keys, kc.edge_priorities(DRAW_ROWS))
    return _inputs["draw"]


def draw_weights64(alpha):
    return draw_case()[2].astype(np.float64) ** float(alpha)


# ---- rl_learn_prioritized_choice ----
CHOICE_SIZES = (65, 1000)
CHOICE_ALPHAS = (1.0, 0.25)


def choice_case(n, stored, alpha=rpc.ALPHA):
    """learn_reference_prioritized_cases.choice_case's recipe with the exponent as an argument: the same seeded priorities, layout by
    ring slot and stream of uniforms, keeping the uniforms that numpy's own arithmetic AT THIS ALPHA holds at least SNAPSHOT_MARGIN from
    both ends of their bracket.  At the default alpha it is that function's case byte for byte (tests/test_learn_hyper_cpu.py)."""
    C, R = int(n), int(n) + rpc.CHOICE_SLACK
    rng = np.random.RandomState(7919 * C + int(stored))
    prio = (2.0 ** rng.uniform(-3.0, 3.0, size=C)).astype(np.float32)
    prio[rng.rand(C) < 0.1] = 0.0
    if C > 1:
        prio[0] = 0.0
    prio[-1] = max(prio[-1], np.float32(0.25))
    by_slot = np.full(R, np.nan, np.float32)
    i = np.arange(C, dtype=np.int64)
    by_slot[(i + C * ((int(stored) - 1 - i) // C)) % R] = prio
    u, tried = [], 0
    while len(u) < rpc.CHOICE_BATCH and tried < 100 * rpc.CHOICE_BATCH:
        x = rng.random_sample()
        tried += 1
        _, br = rpc.choice_indices(prio, [x], alpha)
        if rpc.margins(x, br)[0] >= rpc.SNAPSHOT_MARGIN:
            u.append(x)
    u = np.array(u, np.float64)
    idx, bracket = rpc.choice_indices(prio, u, alpha)
    return dict(prio=prio, by_slot=by_slot, u=u, idx=idx, bracket=bracket, tried=tried, capacity=C, ring_rows=R, stored=int(stored), alpha=float(alpha))
