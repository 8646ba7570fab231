"""GPU: trainer(learn="reference") -- the reference's own training schedule and draws on one world, from seeds alone.

tests/golden/learn_reference_{dqn,d3qn,ppo}.npz (tools/gen_golden_learn_reference.py) hold runs of the real reference's trainer loop,
learn() included.  Here the product's brains get the same initial weights, `random` / `np.random` / torch the same seeds, and
trainer(..., learn="reference") must make the same actions tick for tick, leave `random` in the same state after every tick, make the
same train() calls on the same sampled rows, and end -- after each brain's first update and at the end of the run -- with outputs on the
fixture's states that differ from the reference's by no more than test_five_steps_match_the_reference_end_to_end's bar:
ref_q_spread * (1e-5 / ref_grad_err) of what training changed.  Every figure a bar is held against is printed before it is asserted."""
import collections
import glob
import hashlib
import os
import random

import numpy as np
import pytest

import learn_reference_cases as lrc

pytestmark = pytest.mark.gpu

_RUNS = {}


def _digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def _run(name, learn, ticks=None, save=False, rows=False):
    """trainer() on a fixture's configuration and seeds, watched: per tick the actions and the `random` digest; per learning call the
    entry point, the batch and -- right behind each brain's first update, in stream order -- a copy of its parameters; rows=True also
    keeps every captured transition on the host and reads the ring back at every call's slots."""
    import torch
    from reinlife_amd import Environment, trainer
    from reinlife_amd.worlds import DeviceWorlds
    g = lrc.load(name)
    case = lrc.CASES[name]
    brains = lrc.product_brains(name, g)
    ticks = int(g["ticks"]) if ticks is None else ticks
    rec = dict(g=g, brains=brains, actions=[], digest=[], entries=[], first={}, history=collections.defaultdict(list), ring_checks=[])
    mp = pytest.MonkeyPatch()
    step, update, learn_ref, dev_learn = Environment.step, Environment.update_env, Environment.learn_reference, DeviceWorlds.learn

    def w_step(env):
        m = env._mat(0)
        rec["actions"].append(np.array(m.actions[:m.n], np.int8))
        return step(env)

    def w_update(env, n_epi=0):
        r = update(env, n_epi)
        rec["digest"].append(_digest())
        return r

    def w_dev_learn(worlds, learners, n_steps, slots=None, gate=True):
        r = dev_learn(worlds, learners, n_steps, slots=slots, gate=gate)
        l = learners[0]
        rec["entries"].append((l.entry, int(l.batch), int(n_steps)))
        if id(l.params) not in rec["first"]:
            rec["first"][id(l.params)] = l.params.clone()
        return r

    def w_learn_ref(env, n_epi=0):
        if not rows:
            return learn_ref(env, n_epi)
        agents = env.agents
        post = [(int(a._f("brain")), a.age, a.dead, np.array(a.state, np.float32), np.array(a.state_prime, np.float32), a.action,
                 np.float32(a.reward), a.done) for a in agents]
        calls = learn_ref(env, n_epi)
        pending = collections.defaultdict(list)
        for c in calls:
            if c.kind == "learn":
                pending[c.brain].append(c)
        for b, age, dead, *row in post:          # the deque of the reference, agent by agent (D3QN.py:118-126)
            if age <= 1:
                continue
            brain = env.brains[b]
            dq = rec.setdefault("deque_%d" % b, collections.deque(maxlen=brain.capacity))
            rec["history"][b].append(row)
            dq.append(len(rec["history"][b]) - 1)
            if n_epi > brain.exploration and (age % brain.train_freq == 0 or dead):
                c = pending[b].pop(0)
                assert c.size == len(dq)
                ring = env.learners[b].ring
                sl = torch.as_tensor(c.slots[0].astype(np.int64), device=ring["state"].device)
                got = [ring[k][sl].cpu().numpy() for k in ("state", "state_prime", "action", "reward", "done")]
                rec["ring_checks"].append((n_epi, b, [dq[i] for i in c.indices[0]], got))
        assert not any(pending.values())
        return calls

    mp.setattr(Environment, "step", w_step)
    mp.setattr(Environment, "update_env", w_update)
    mp.setattr(Environment, "learn_reference", w_learn_ref)
    mp.setattr(DeviceWorlds, "learn", w_dev_learn)
    mp.setattr(Environment, "log_reference_calls", True)
    try:
        lrc.seed_all(int(g["seed"]))   # after construction, like the recorder
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            env = trainer(brains, n_episodes=ticks - 1, width=case["width"], height=case["height"], max_agents=case["max_agents"],
                          print_results=False, save=save, learn=learn)
    finally:
        mp.undo()
    rec["env"] = env
    rec["first"] = {k: rec["first"][id(l.params)].cpu().numpy() for k, l in env.learners.items() if id(l.params) in rec["first"]}
    rec["final"] = {k: l.params.cpu().numpy() for k, l in env.learners.items()}
    return rec


def _reference_run(name):
    if name not in _RUNS:
        _RUNS[name] = _run(name, "reference", rows=name == "d3qn")
    return _RUNS[name]


@pytest.mark.parametrize("name", ["dqn", "d3qn", "ppo"])
def test_trainer_trains_as_the_reference_does_from_seeds(name):
    r = _reference_run(name)
    g, env = r["g"], r["env"]
    kind, nb, T = lrc.CASES[name]["kind"], lrc.CASES[name]["n_brains"], int(g["ticks"])
    # the actions, tick for tick, and the `random` stream after every tick
    assert len(r["actions"]) == T
    for t in range(T):
        n0 = int(g["n0"][t])
        assert r["actions"][t].tolist() == g["actions"][t, :n0].tolist(), "%s: actions of tick %d" % (name, t)
    assert r["digest"] == g["digest"].tolist()
    # the calls: tick, brain, deque length, sampled indices (PPO: list length and the entry it went to)
    made = [(t, c) for t, c in env.reference_calls if c.kind != "sync"]
    assert [t for t, _ in made] == g["call_tick"].tolist() and [c.brain for _, c in made] == g["call_brain"].tolist()
    assert [c.size for _, c in made] == g["call_size"].tolist()
    if kind == "PPO":
        assert r["entries"] == [("rl_learn_ppo_wide" if n > 32 else "rl_learn_ppo", int(n), 1) for n in g["call_size"]]
        assert (g["call_size"] > 32).any() and (g["call_size"] <= 32).any()
    else:
        assert np.array_equal(np.stack([c.indices for _, c in made]), g["call_indices"])
        assert [e[0] for e in r["entries"]] == [{"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}[kind]] * len(made)
        assert [(t, c.brain) for t, c in env.reference_calls if c.kind == "sync"] == list(zip(g["sync_tick"].tolist(), g["sync_brain"].tolist()))
    assert sorted(env.learners) == list(range(nb)) and all(int(l.state[0].item()) > 0 for l in env.learners.values())
    # the bar: outputs in float64 on the fixture's states, after the first update and at the end
    worst = 0.0
    for b in range(nb):
        bar = float(g["ref_q_spread"][b]) * (1e-5 / float(g["ref_grad_err"][b]))
        for when, got in (("first", r["first"][b]), ("final", r["final"][b])):
            ref, init = g["out_" + when][b], g["out_init"][b]
            effect = np.abs(ref - init).max()
            ratio = np.abs(lrc.outputs64(kind, got, g["states"]) - ref).max() / effect
            worst = max(worst, ratio / bar)
            print("%s brain %d, %s update: max|d out| / training effect = %.3g (bar %.3g; torch float32 against float64: %.3g); effect %.3g"
                  % (name, b, when, ratio, bar, float(g["ref_q_spread"][b]), effect))
    print("%s: worst ratio / bar = %.3g" % (name, worst))
    for b in range(nb):
        bar = float(g["ref_q_spread"][b]) * (1e-5 / float(g["ref_grad_err"][b]))
        for when, got in (("first", r["first"][b]), ("final", r["final"][b])):
            ref, init = g["out_" + when][b], g["out_init"][b]
            assert np.abs(lrc.outputs64(kind, got, g["states"]) - ref).max() / np.abs(ref - init).max() <= bar, (name, b, when)
    # the acting weights are the learners': sync_learners() has put the trained parameters into the brains' modules
    for b, brain in enumerate(r["brains"]):
        assert brain.state_dict_flat().tobytes() == r["final"][b].tobytes()
        assert not np.array_equal(r["final"][b], lrc.weights(kind, int(g["init_seeds"][b])))


def test_ring_rows_at_the_named_slots_are_the_deques_after_it_has_lapped():
    """The D3QN run: a deque of 80 in a ring of 144 that 300-odd rows pass through.  For every train() call the rows read back from the
    ring at the call's slots are the transitions a host-side deque(maxlen=80) of the captured transitions holds at the sampled indices."""
    r = _reference_run("d3qn")
    g, env = r["g"], r["env"]
    assert len(r["ring_checks"]) == len(g["call_tick"]) > 0
    ring = int(env.learners[0].ring["state"].shape[0])
    stored = len(r["history"][0])
    assert ring == 80 + 64 and stored > 2 * ring and int(env.learners[0].ring["count"].item()) == stored == env.schedule.stored[0]
    for n_epi, b, ids, (state, state_prime, action, reward, done) in r["ring_checks"]:
        want = [r["history"][b][i] for i in ids]
        assert np.array_equal(state, np.stack([w[0] for w in want])), n_epi
        assert np.array_equal(state_prime, np.stack([w[1] for w in want])), n_epi
        assert action.tolist() == [w[2] for w in want] and reward.tolist() == [float(w[3]) for w in want]
        assert done.astype(bool).tolist() == [bool(w[4]) for w in want]
    late = [c for c in r["ring_checks"] if c[0] >= int(g["call_tick"][-1])]
    assert late and max(max(c[2]) for c in late) >= ring          # rows beyond the first lap were sampled


def test_a_list_of_32_rows_ends_with_the_same_bytes_through_either_ppo_entry():
    """The narrow and the wide PPO learner of learn="reference" share every tensor; on a list of exactly 32 captured rows rl_learn_ppo and
    rl_learn_ppo_wide leave the same parameters, moments, counters and acting weights.  (Lists of more than 32 rows go to the wide entry
    in the fixture's run, which ends within the bar: test_trainer_trains_as_the_reference_does_from_seeds.)"""
    import torch
    import warnings
    from reinlife_amd import Environment
    g = lrc.load("ppo")
    brains = lrc.product_brains("ppo", g)
    lrc.seed_all(7)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = Environment(brains=brains, max_agents=100, print_results=False, learn="reference")
    env.reset()
    l, narrow = env.learners[0], env._ppo_narrow[0]
    assert (l.entry, narrow.entry) == ("rl_learn_ppo_wide", "rl_learn_ppo") and narrow.params is l.params and narrow.packed is l.packed
    for t in range(400):
        env.act(t); env.step()
        env.worlds.capture_transitions(with_policy_out=True)     # the rows without the schedule: nothing trains yet
        env.update_env(t)
        if t % 8 == 7 and int(l.ring["count"].item()) >= 32:
            break
    assert int(l.ring["count"].item()) >= 32
    names = ("params", "adam_m", "adam_v", "state", "packed")
    before = {k: getattr(l, k).clone() for k in names}
    slots = np.arange(32, dtype=np.int32).reshape(1, 32)
    out = {}
    for wide in (False, True):
        for k in names:
            getattr(l, k).copy_(before[k])
        env._learn_ppo(0, slots, wide)
        torch.cuda.synchronize()
        env.worlds.check_error_flag()
        out[wide] = {k: getattr(l, k).cpu().numpy().copy() for k in names}
    assert out[True]["state"].tolist() == [l.k_epoch, 1] and not np.array_equal(out[True]["params"], before["params"].cpu().numpy())
    for k in names:
        assert out[False][k].tobytes() == out[True][k].tobytes(), k


def test_frozen_kinds_are_named_and_stay_frozen():
    """A PERD3QN brain beside a DQN brain: the warning names it, it gets no learner and a ring of the floor's size that the capture
    fills all the same, a caller's own loop runs, and its weights stay what they were."""
    from reinlife_amd import Environment, Models
    brains = [Models.DQN(max_epi=100), Models.PERD3QN()]
    before = brains[1].state_dict_flat().copy()
    lrc.seed_all(9)
    with pytest.warns(UserWarning, match=r"learn='reference' trains the DQN, D3QN and PPO brains.*1 \(PERD3QN\).*NOT updated"):
        env = Environment(brains=brains, max_agents=100, print_results=False, learn="reference")
    assert sorted(env.learners) == [0] and env.ring_rows == [50_000 + 256, 256] and env.schedule.specs[1] is None
    env.reset()
    with pytest.raises(RuntimeError, match="between step"):
        env.learn_reference(0)
    for t in range(30):
        env.act(t); env.step()
        assert env.learn_reference(t) == []              # (a DQN deque of a few dozen rows: below the gate)
        with pytest.raises(RuntimeError, match="once per tick"):
            env.learn_reference(t)
        env.update_env(t)
    env._sync()
    counts = [int(r["count"].item()) for r in env.worlds.replays]
    assert counts[0] == env.schedule.stored[0] > 0 and counts[1] > 0 and env.schedule.stored[1] == 0
    env.sync_learners()
    assert brains[1].state_dict_flat().tobytes() == before.tobytes()
    assert "brains [1] as loaded / initialised" in env._weights_note()


def test_save_writes_the_trained_weights_and_learn_none_is_what_it_was(tmp_path, monkeypatch):
    import torch
    g = lrc.load("d3qn")
    first = int(g["first_update_tick"].min())
    monkeypatch.chdir(tmp_path)
    r = _run("d3qn", "reference", ticks=first + 12, save=True)
    files = sorted(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "D3QN", "brain_gene_*.pt")))
    assert len(files) == 1
    flat = np.concatenate([v.numpy().reshape(-1) for v in torch.load(files[0]).values()])
    assert flat.tobytes() == r["final"][0].tobytes() and not np.array_equal(flat, lrc.weights("D3QN", int(g["init_seeds"][0])))
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "learn='reference'" in settings and "inference only" not in settings
    # learn=None on the same seeds: the same actions up to the first update, no learner, no ring, no learning or capture launch
    n = _run("d3qn", None, ticks=first + 1)
    env = n["env"]
    for t in range(first + 1):
        assert n["actions"][t].tolist() == g["actions"][t, :int(g["n0"][t])].tolist(), t
    assert n["digest"][:first] == g["digest"][:first].tolist() and n["digest"][first] != int(g["digest"][first])   # (tick `first` samples)
    assert env.learners == {} and env.worlds.replays is None and env.worlds.launches == 0 and n["entries"] == [] and env.schedule is None
    assert r["env"].worlds.launches > 0
    assert n["brains"][0].state_dict_flat().tobytes() == lrc.weights("D3QN", int(g["init_seeds"][0])).tobytes()
