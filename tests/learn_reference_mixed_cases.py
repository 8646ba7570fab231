"""What tools/gen_golden_learn_reference_mixed.py and the learn="reference" tests of a run with several opt-in brains share: the run's
configuration, the fixture's premises as one function of the data, the replay of a run's two process-global streams around the host
schedule, and the product-side brains of the fixture.

tests/golden/learn_reference_pairs.npz  brains PERD3QN, PERDQN, PERD3QN, PERDQN in one world: two opt-in brains of each kind, training in
                                        the same ticks, no PERDQN learner at index 0 alone and a PERD3QN learner at index 2

(A run with one brain of each of the five kinds is NOT among the fixtures: docs/experiments.md says what was tried.)

It is a run of the real reference's trainer loop, learn() included, from seeds, and holds what learn_reference_perdqn.npz holds
up to the calls (tests/learn_reference_cases.py, learn_reference_prioritized_cases.py, learn_reference_td_cases.py: the actions, the
post-step lists, both generators' digests, the environment's draws, the decisions' gaps, 64 states) and:
    pre_brain [T, maxn]                      the brain of every agent of the pre-step list (whose coin a decision's draws are)
    call_tick, call_brain, call_kind, call_size, call_sync, call_stored [n_calls], call_store [n_calls, 2]
                                             call_order: EVERY call of the run in the order made -- kind as an index into CALL_KINDS
                                             ("learn": a train() that updated; "sync": a D3QN / PERD3QN target copy without an update; "ppo";
                                             "store": the rows an opt-in brain stored behind its tick's last train(), brains ascending at the
                                             end of the tick), len(deque / list / memory) at the call, target copy, the rows the brain had
                                             stored as of the call and, for the opt-in brains, the store group (first row, rows; else -1)
    out_init_<b>, out_first_<b>, out_final_<b> [64, 8 or 9] float64      the reference's float32 parameters of brain b evaluated in float64
                                             on `states`: initial, after its first update, at the end.  No parameter sets are kept.
    first_update_tick, ref_grad_err, ref_q_spread, effect, final_stored [n_brains]
and per brain b, one row per "learn" call of that brain in order:
    DQN, D3QN       indices_<b> [n, steps, batch]                       what random.sample drew, as deque indices
    PERD3QN         uniforms_<b>, indices_<b> [n, batch], prio_<b> [n, capacity], bracket_<b> [n, batch, 2], new_prio_<b> [n, batch] (what
                    update_priorities left at the drawn indices), final_prio_<b>, cdf_err[b]
    PERDQN          uniforms_<b>, idxs_<b>, s_<b>, leaves_<b>, lo_<b>, is_weight_<b>, errors_<b> [n, batch], total_<b>, epsilon_<b> [n],
                    final_tree_<b>, final_beta[b], final_epsilon[b], interval_err[b]
with the meanings their own fixtures give them."""
import hashlib
import os
import random

import numpy as np

import learn_reference_cases as lrc
import learn_reference_prioritized_cases as pc
import learn_reference_td_cases as tc

CALL_KINDS = ("learn", "sync", "ppo", "store")
OPT_IN = ("PERD3QN", "PERDQN")
# Constructor arguments: the single-kind cases', but for train_freq.  The reference's world starts with one agent per brain and holds
# ten to twenty agents after a hundred ticks, so at the default of 20 a brain trains in about one tick of ten and two brains of a kind
# hardly ever in the same tick: with the single-kind arguments no seed of 1..200 met the premises in runs of 140, 220, 300 or 400 ticks
# (docs/experiments.md has the counts).  At TRAIN_FREQ the triggers fall twice as often and the premises can be met in 140 ticks.  The
# schedule's rule is the same (age % train_freq == 0 or dead); the bars and margins are taken from THIS run's own yardsticks.
TRAIN_FREQ = 10
ARGS = {"PERD3QN": dict(pc.CASE["args"], train_freq=TRAIN_FREQ), "PERDQN": dict(tc.CASE["args"], train_freq=TRAIN_FREQ)}
NETS = {"PERD3QN": ["eval_net", "target_net"], "PERDQN": ["model", "target_model"]}
CASES = {"pairs": dict(kinds=("PERD3QN", "PERDQN", "PERD3QN", "PERDQN"), width=30, height=30, max_agents=21, max_ticks=140)}
NAMES = tuple(CASES)


def path(name):
    return os.path.join(lrc.GOLDEN_DIR, "learn_reference_%s.npz" % name)


def load(name):
    with np.load(path(name)) as z:
        return {k: z[k] for k in z.files}


def slack(name):
    """slot_cap_for(max_agents) of the run: the rows a ring holds beyond its deque's maxlen."""
    return ((2 * CASES[name]["max_agents"] + 2 + 63) // 64) * 64


def weights(kind, seed):
    return tc.weights(seed) if kind == "PERDQN" else lrc.weights(pc.KIND, seed)


def outputs64(kind, flat, states):
    """A brain's outputs on `states` in float64, by its kind's own cases module."""
    return tc.outputs64(flat, states) if kind == "PERDQN" else lrc.outputs64(pc.KIND, flat, states)


def product_brains(name, g):
    """The product's brains of a fixture, carrying its initial weights (before any seeding: the constructors draw from torch)."""
    import torch
    from reinlife_amd import Models
    brains = []
    for b, kind in enumerate(CASES[name]["kinds"]):
        brain = getattr(Models, kind)(**ARGS[kind])
        if kind == "PERDQN":
            brain.train_start = int(tc.CASE["train_start"])
        flat = weights(kind, int(g["init_seeds"][b]))
        for net in NETS[kind]:
            off = 0
            with torch.no_grad():
                for t in getattr(brain, net).state_dict().values():
                    t.copy_(torch.from_numpy(flat[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                    off += t.numel()
            assert off == flat.size
        brain.invalidate()
        brains.append(brain)
    return brains


def specs(name):
    """The BrainSpecs of the run's brains, from the constructor arguments (the CPU test holds them against BrainSpec.of)."""
    from reinlife_amd.learn_reference import BrainSpec
    out = []
    for kind in CASES[name]["kinds"]:
        a = ARGS[kind]
        if kind == "PERDQN":
            out.append(BrainSpec("PERDQN", a["train_freq"], a["capacity"], 64, train_start=tc.CASE["train_start"]))
        else:
            out.append(BrainSpec(kind, a["train_freq"], a["capacity"], a["batch_size"], a["exploration"], a["soft_update_freq"]))
    return out


def digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def replay_draws(py, npd):
    """The environment's recorded draws, as codes (learn_reference_prioritized_cases' docstring), on both generators."""
    for c in py:
        if c == 0:
            random.random()
        elif c > 0:
            random.choice(range(int(c)))
    for c in npd:
        if c == 0:
            np.random.random()
        elif c > 0:
            np.random.randint(0, int(c))


def host_loop(name, g, by_brain=False, on_tick=None):
    """The run's whole `random` and np.random streams without a world: seeded as the run was, then per tick every agent's coin in act()'s
    order by its brain's kind (PERD3QN.py:204-210, PERDQN.py:104-105), the draws the environment made in step(), the schedule's draws, and update_env()'s draws.  by_brain=True hands the
    schedule each tick's agents sorted by brain (stable) instead of in list order: the WRONG interleaving, which the fixture must tell
    from the right one.  Returns the schedule, every (tick, Call) and (random digest, np.random digest) after every tick."""
    from reinlife_amd.learn_reference import ReferenceSchedule
    kinds = CASES[name]["kinds"]
    sched = ReferenceSchedule(specs(name), slack(name))
    random.seed(int(g["seed"]))
    replay_draws(g["reset_draws"], [])
    np.random.set_state(("MT19937", g["np_state0"], int(g["np_pos0"]), 0, 0.0))
    assert digest() == int(g["digest0"]) and pc.np_digest() == int(g["np_digest0"])
    out, digests = [], []
    for t in range(int(g["ticks"])):
        for k in range(int(g["n0"][t])):
            kind, greedy = kinds[int(g["pre_brain"][t, k])], bool(g["greedy"][t, k])
            if kind == "PERD3QN":
                random.random()
                if not greedy:
                    random.choice(list(range(8)))
            else:
                np.random.rand()
                if not greedy:
                    random.randrange(8)
        replay_draws(g["step_draws"][t], g["np_step_draws"][t])
        n1 = int(g["n1"][t])
        agents = list(zip(g["post_brain"][t, :n1].tolist(), g["post_age"][t, :n1].tolist(), g["post_dead"][t, :n1].tolist()))
        if by_brain:
            agents.sort(key=lambda a: a[0])
        calls = sched.tick(t, agents)
        out += [(t, c) for c in calls]
        replay_draws(g["upd_draws"][t], g["np_upd_draws"][t])
        digests.append((digest(), pc.np_digest()))
        if on_tick:
            on_tick(t, sched, calls)
    return sched, out, digests


def calls_of(g, b, kind="learn"):
    """The positions in call_order of brain b's calls of one kind."""
    return np.flatnonzero((g["call_brain"] == b) & (g["call_kind"] == CALL_KINDS.index(kind)))


def bars(g):
    """Per brain, the bar of its own single-kind test: ref_q_spread * (1e-5 / ref_grad_err), relative to what training changed."""
    return g["ref_q_spread"] * (1e-5 / g["ref_grad_err"])


def perd3qn_margins(g, b):
    return pc.margins(g["uniforms_%d" % b], g["bracket_%d" % b])


def perdqn_margins(g, b):
    s, lo, leaves = g["s_%d" % b], g["lo_%d" % b], g["leaves_%d" % b]
    return np.minimum(s - lo, lo + leaves - s)


def premises(name, g):
    """What the run was chosen for, from the data alone -> the premises a fixture misses, as sentences (none: it is kept).  The
    generator asserts this at the end of run() and the CPU test again.  (That the fixture tells list order from brain order needs the
    replay: sensitive().)"""
    kinds, T = CASES[name]["kinds"], int(g["ticks"])
    nb, miss = len(kinds), []
    tick, brain, ckind = g["call_tick"], g["call_brain"], g["call_kind"]
    per = np.bincount(brain[ckind == CALL_KINDS.index("learn")], minlength=nb)
    if per.min() < 3:
        miss.append("a brain with fewer than 3 updating calls: %s" % per.tolist())
    for b, kind in enumerate(kinds):
        if int(g["final_stored"][b]) < 2 * ARGS[kind]["capacity"]:
            miss.append("brain %d (%s): the memory does not wrap: %d rows" % (b, kind, int(g["final_stored"][b])))
    by_tick = {}
    for k in np.flatnonzero(ckind == CALL_KINDS.index("learn")):
        by_tick.setdefault(int(tick[k]), set()).add(int(brain[k]))
    for kind in OPT_IN:
        both = {b for b, k in enumerate(kinds) if k == kind}
        n = sum(1 for trained in by_tick.values() if trained >= both)
        if n < 5:
            miss.append("both %s brains train in %d ticks only" % (kind, n))
    ends = [k for k in range(len(tick)) if ckind[k] == CALL_KINDS.index("store")]
    if not any(tick[a] == tick[c] and brain[a] != brain[c] for a, c in zip(ends, ends[1:])):
        miss.append("no tick ends with store calls for two brains")
    # The greedy decisions: no near-tie.  tests/test_learn_reference_cpu.py::test_fixture_premises' rule, applied per brain.  There the
    # brains are of one kind and one scale, and one pair of figures serves them all: up to the run's first update a relative gap of 1e-5,
    # after it 10 x the largest absolute bar.  Here a decision of brain b is an argmax over brain b's outputs alone.  Up to b's OWN
    # first update these come from its initial weights, bit for bit the reference's, whatever other brains have trained: the relative
    # rule's premise holds until then.  After it they differ from the reference's by at most b's own bar times b's own effect: another
    # brain's bar, taken on another network's outputs of another scale, bounds nothing about them.
    greedy = g["greedy"] == 1
    valid = np.arange(g["greedy"].shape[1])[None] < g["n0"][:, None]
    rel = np.where(greedy, g["gap"] / np.maximum(g["qmax"], 1e-30), np.inf)
    absg = np.where(greedy, g["gap"], np.inf)
    for b in range(nb):
        mine, first = valid & (g["pre_brain"] == b), int(g["first_update_tick"][b])
        bar_abs = float(bars(g)[b] * g["effect"][b])
        before, after = np.where(mine, rel, np.inf)[:first + 1], np.where(mine, absg, np.inf)[first + 1:]
        if not (mine & greedy).any():
            miss.append("brain %d: no greedy decision" % b)
        if before.min() < 1e-5:
            miss.append("brain %d: a greedy decision up to its first update with a relative gap of %.3g" % (b, before.min()))
        if not first + 1 < T or after.min() < 10 * bar_abs:
            miss.append("brain %d: a greedy decision after its first update with a gap of %.3g < 10 x its absolute bar %.3g" % (b, after.min(), bar_abs))
    if not (((1e-9 < g["ref_grad_err"]) & (g["ref_grad_err"] < 1e-5)).all() and (g["ref_q_spread"] > 0).all() and (g["effect"] > 0).all()):
        miss.append("a yardstick out of its range: ref_grad_err %s ref_q_spread %s effect %s" % (g["ref_grad_err"], g["ref_q_spread"], g["effect"]))
    # the draws: EVERY one, from both ends of its bracket / its leaf's interval
    for b, kind in enumerate(kinds):
        if kind == "PERD3QN":
            m, D = perd3qn_margins(g, b), float(g["cdf_err"][b])
            if m.min() < pc.SNAPSHOT_MARGIN or m.min() < pc.RUN_MARGIN_FACTOR * D or not D > 0:
                miss.append("brain %d: a PERD3QN draw %.3g from an end of its bracket (2^-20 = %.3g, 8 D = %.3g)" % (b, m.min(), pc.SNAPSHOT_MARGIN, 8 * D))
        if kind == "PERDQN":
            m, D = perdqn_margins(g, b), float(g["interval_err"][b])
            relm = (m / g["total_%d" % b][:, None]).min()
            if relm < tc.REL_MARGIN or m.min() < tc.RUN_MARGIN_FACTOR * D or not D > 0:
                miss.append("brain %d: a PERDQN draw %.3g (%.3g of the total) from an end of its leaf's interval (8 D = %.3g)" % (b, m.min(), relm, 8 * D))
            C = ARGS[kind]["capacity"]
            mem = g["idxs_%d" % b] - (C - 1)
            stored = g["call_stored"][calls_of(g, b)]
            if not ((mem >= 0) & (mem < np.minimum(stored, C)[:, None])).all():
                miss.append("brain %d: a PERDQN draw on a leaf no row has reached (the reference draws again there)" % b)
    return miss


def sensitive(name, g):
    """Can the fixture tell a wrong order of the brains' draws from the right one?  Replayed with each tick's agents handed to the
    schedule sorted by brain, every brain must be handed other uniforms than the reference consumed at some call.  (The streams'
    digests after a tick cannot show it in this run: a PERD3QN call always takes 16 doubles of np.random and a PERDQN call 64 of
    `random`, so a tick leaves both generators where it left them whatever the order -- it is the uniforms per call that differ.)
    -> the brains whose uniforms all stayed the same (none: sensitive)."""
    _, wrong, _ = host_loop(name, g, by_brain=True)
    same = []
    for b in range(len(CASES[name]["kinds"])):
        got = [c.uniforms for _, c in wrong if c.brain == b and c.kind == "learn"]
        if len(got) == len(g["uniforms_%d" % b]) and np.array_equal(np.stack(got), g["uniforms_%d" % b]):
            same.append(b)
    return same
