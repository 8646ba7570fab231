"""The learn_reference_prioritized=True fixture from the real reference (build container only; data in, data out -- no reference source is
copied).

Runs the reference's own trainer loop body (ReinLife/Helpers/trainer.py:85-99) with one real PERD3QN brain carrying repo-generated
weights, as tools/gen_golden_learn_reference.py runs its D3QN brain -- the same recorders, seeding, decisions' gaps and yardsticks, taken
from that module -- and records beside them what tests/learn_reference_prioritized_cases.py lists: a digest of np.random's state per tick
and, per train() call, the uniforms np.random.choice consumed, the indices it answered, the priorities as they stood and each draw's
bracket of the cdf.  The reference's files are not modified: train(), buffer.store and buffer.sample are wrapped on the brain instance.

Every call checks, before it lets train() run, that np.random.choice is what the cases module states: the indices are
cdf.searchsorted(u, side="right") for u = np.random.random_sample(batch) from the state before the call, and np.random is left in the state
those draws leave it in.

A float64 twin follows the run on the recorded batches (Shadow of tools/gen_golden_learn_reference.py) and keeps float64 priorities by
the same store / update rules; at every call the cdf of those is compared with the float32 run's: D is the largest difference.

Seeds are searched until the premises hold (the end of run()): the memory wraps at least twice, at least 20 train() calls, a target copy
on an update, the greedy decisions' gaps as for the other fixtures, and EVERY draw at least 2^-20 and at least 8 D from both ends of its
bracket -- no draw is exempt.

    python tools/gen_golden_learn_reference_prioritized.py [first:last]
"""
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_learn_reference as base  # noqa: E402  (puts the repository root and tests/ on sys.path)
from oracle import ref_harness as rh  # noqa: E402
import learn_reference_cases as lrc  # noqa: E402
import learn_reference_prioritized_cases as pc  # noqa: E402

FIRST_SEED = 1   # the seed range the committed fixture was searched from


def env_draws():
    """The draws the reference's environment made since the log was cleared, as codes in order -- from `random`: 0 = random.random(),
    n > 0 = random.choice of n elements; from np.random: 0 = np.random.random(), n > 0 = np.random.randint(0, n) (grid.py:75-77,
    environment.py:760)."""
    py, npd = [], []
    for _, _, kind, _, extra in rh.LOG.entries:
        if kind == "py.random":
            py.append(0)
        elif kind == "py.choice":
            py.append(int(extra))
        elif kind == "np.randint":
            npd.append(int(extra))
        else:
            assert kind == "np.random", "a draw of the environment this recorder does not know: %s" % kind
            npd.append(0)
    rh.LOG.clear()
    return py, npd


def run(seed):
    case, kind, nb = pc.CASE, pc.KIND, 1
    ref = rh.load_reference()
    torch = ref.torch
    init_seed = 1000 + 10 * seed
    brain = ref.PERD3QN(**case["args"])
    w = lrc.weights(kind, init_seed)
    for net in ("eval_net", "target_net"):
        off = 0
        with torch.no_grad():
            for t in getattr(brain, net).state_dict().values():
                t.copy_(torch.from_numpy(w[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                off += t.numel()
    sh = base.Shadow(torch, kind, brain)
    params = lambda: base.flat(brain.eval_net.state_dict()).astype(np.float32)  # noqa: E731
    C, B = brain.buffer.capacity, brain.batch_size
    alpha64 = float(pc.ALPHA)
    prio64 = np.zeros(C, np.float64)          # the float64 twin's priorities, by memory index
    cur = {"tick": 0, "trained": None, "stored": 0, "D": 0.0}
    calls, syncs, first, first_tick = [], [], [None], [-1]

    buf = brain.buffer
    orig_store, orig_sample, orig_train = buf.store, buf.sample, brain.train

    def store(*a, **k):
        prio64[buf.pos] = prio64.max() if buf.memory else 1.0     # PERD3QN.py:147, 153 in float64
        cur["stored"] += 1
        return orig_store(*a, **k)

    def sample(batch_size):
        out = orig_sample(batch_size)
        cur["indices"] = np.array(out[5], np.int64)
        return out

    def train():
        n = len(buf.memory)
        prio = buf.priorities[:n].copy()
        state = np.random.get_state()
        u = np.random.random_sample(B)
        drawn = np.random.get_state()
        np.random.set_state(state)
        idx, bracket = pc.choice_indices(prio, u)
        batch = [buf.memory[i] for i in idx]
        sh.before([batch], brain.target_net)
        cdf64 = (prio64[:n] ** alpha64) / (prio64[:n] ** alpha64).sum()
        cdf64 = cdf64.cumsum()
        cur["D"] = max(cur["D"], float(np.abs(cdf64 / cdf64[-1] - pc.choice_cdf(prio)).max()))
        orig_train()
        after = np.random.get_state()
        assert np.array_equal(cur["indices"], idx), "np.random.choice is not cdf.searchsorted(random_sample(batch), side='right')"
        assert after[2] == drawn[2] and np.array_equal(after[1], drawn[1]), "np.random.choice consumed other draws than random_sample(batch)"
        with torch.no_grad():   # update_priorities (PERD3QN.py:110-111) by the float64 twin, before its step
            s = torch.tensor(np.concatenate([x[0] for x in batch], 0), dtype=torch.float64)
            a = torch.tensor([int(x[1]) for x in batch])
            sp = torch.tensor(np.concatenate([x[3] for x in batch], 0), dtype=torch.float64)
            p64 = (sh.t.forward(sp).max(1)[0] - sh.q.forward(s).gather(1, a.unsqueeze(1)).squeeze(1)).abs().numpy()
        for i, p in zip(idx, p64):
            prio64[i] = p
        sh.step([batch])
        cur["trained"] = dict(size=n, stored=cur["stored"], u=u, idx=idx, prio=prio, bracket=bracket)

    buf.store, buf.sample, brain.train = store, sample, train

    rh.seed_all(seed)   # after construction: the constructors consume torch's generator
    rh.LOG.clear()
    env = rh.make_env(brains=[brain], width=case["width"], height=case["height"], max_agents=case["max_agents"], static_families=True)
    env.reset()
    reset_draws, digest0, np_digest0, np_state0 = env_draws()[0], base.digest(), pc.np_digest(), np.random.get_state()
    assert np_state0[3] == 0, "np.random holds a cached gaussian after reset()"
    rec = {k: [] for k in ("actions", "post", "digest", "np_digest", "dec", "seconds", "step_draws", "upd_draws", "np_step_draws", "np_upd_draws")}
    pool, stale = [], False
    for t in range(case["max_ticks"]):
        t0 = time.perf_counter()
        cur["tick"] = t
        dec, acts = [], []
        for agent in env.agents:
            with torch.no_grad():
                out = brain.eval_net(torch.from_numpy(agent.state).float()[None])[0].numpy()
            state = random.getstate()
            agent.get_action(t)
            after = random.getstate()
            random.setstate(state)
            coin = random.random()
            random.setstate(after)
            greedy = coin > brain.epsilon
            top = np.sort(out)[::-1]
            dec.append((int(greedy), float(top[0] - top[1]), float(np.abs(out).max()), float(out[agent.action])))
            if greedy:
                assert int(agent.action) == int(out.argmax())
            acts.append(int(agent.action))
            pool.append((t, np.asarray(agent.state, np.float32)))
        rh.LOG.clear()
        env.step()
        py, npd = env_draws()
        rec["step_draws"].append(py); rec["np_step_draws"].append(npd)
        rec["post"].append([(0, a.age, int(a.dead)) for a in env.agents])
        for agent in env.agents:
            cur["trained"] = None
            agent.learn(n_epi=t)
            if agent.age > 1 and t > brain.exploration:
                sync = t % brain.soft_update_freq == 0
                if cur["trained"]:
                    calls.append(dict(cur["trained"], tick=t, sync=int(sync)))
                    if first[0] is None:
                        first[0], first_tick[0] = params(), t
                    stale = not sync
                    if sync:
                        sh.sync()
                elif sync and stale:
                    syncs.append((t, 0))
                    stale = False
                    sh.sync()
        assert env_draws() == ([], []), "learn() drew through the environment's module"
        env.update_env(t)
        py, npd = env_draws()
        rec["upd_draws"].append(py); rec["np_upd_draws"].append(npd)
        rec["actions"].append(acts); rec["dec"].append(dec)
        rec["digest"].append(base.digest()); rec["np_digest"].append(pc.np_digest())
        rec["seconds"].append(time.perf_counter() - t0)
    T = len(rec["actions"])
    if first[0] is None:
        return None, "seed %d: the brain never trained in %d ticks" % (seed, T)
    inits, firsts, finals = [w], [first[0]], [params()]
    later = [s for tt, s in pool if tt >= T // 2]
    states = np.stack([later[i] for i in np.linspace(0, len(later) - 1, lrc.N_STATES).astype(int)])
    o = lambda x: lrc.outputs64(kind, x, states)  # noqa: E731
    out_init, out_first, out_final = (np.stack([o(x) for x in ws]) for ws in (inits, firsts, finals))
    out64 = np.stack([o(base.flat(sh.q.state_dict()))])
    effect = np.array([np.abs(out_final[0] - out_init[0]).max()])
    spread = np.array([np.abs(out_final[0] - out64[0]).max() / effect[0]])
    grad_err = np.array([sh.grad_err])
    bar_abs = float((spread * (1e-5 / grad_err) * effect).max())

    maxn = max(max(len(a) for a in rec["actions"]), max(len(p) for p in rec["post"]), 1)
    pad = lambda rows, dt, fill=0: np.stack([np.concatenate([np.asarray(r, dt).reshape(-1), np.full(maxn - len(r), fill, dt)]) for r in rows])  # noqa: E731
    d = {"seed": np.int64(seed), "ticks": np.int64(T), "max_epi": np.int64(case["max_ticks"]), "init_seeds": np.array([init_seed], np.int64),
         "cfg": np.array([case["width"], case["height"], case["max_agents"], nb], np.int64),
         "n0": np.array([len(a) for a in rec["actions"]], np.int32), "actions": pad(rec["actions"], np.int8, -1),
         "n1": np.array([len(p) for p in rec["post"]], np.int32)}
    for i, key in enumerate(("post_brain", "post_age", "post_dead")):
        d[key] = pad([[x[i] for x in p] for p in rec["post"]], np.int32)
    d["digest"], d["digest0"] = np.array(rec["digest"], np.uint64), np.uint64(digest0)
    d["np_digest"], d["np_digest0"] = np.array(rec["np_digest"], np.uint64), np.uint64(np_digest0)
    wide = lambda rows: np.stack([np.concatenate([np.asarray(r, np.int32), np.full(max(map(len, rows)) - len(r), -1, np.int32)]) for r in rows])  # noqa: E731
    d["reset_draws"], d["step_draws"], d["upd_draws"] = np.array(reset_draws, np.int32), wide(rec["step_draws"]), wide(rec["upd_draws"])
    d["np_step_draws"], d["np_upd_draws"] = wide(rec["np_step_draws"]), wide(rec["np_upd_draws"])
    d["np_state0"], d["np_pos0"] = np.asarray(np_state0[1], np.uint32), np.int64(np_state0[2])
    d["greedy"] = pad([[x[0] for x in r] for r in rec["dec"]], np.uint8)
    for i, key in ((1, "gap"), (2, "qmax"), (3, "chosen")):
        d[key] = pad([[x[i] for x in r] for r in rec["dec"]], np.float32)
    d["capacity"], d["batch"] = np.int64(C), np.int64(B)
    d["call_tick"], d["call_size"], d["call_stored"], d["call_sync"] = (np.array([c[k] for c in calls], np.int32) for k in ("tick", "size", "stored", "sync"))
    d["call_brain"] = np.zeros(len(calls), np.int32)
    d["call_uniforms"] = np.stack([c["u"] for c in calls]).astype(np.float64)
    d["call_indices"] = np.stack([c["idx"] for c in calls]).astype(np.int32)[:, None, :]
    d["call_prio"] = np.stack([np.concatenate([c["prio"], np.zeros(C - len(c["prio"]), np.float32)]) for c in calls]).astype(np.float32)
    d["call_bracket"] = np.stack([c["bracket"] for c in calls]).astype(np.float64)
    d["final_prio"], d["final_stored"] = buf.priorities.astype(np.float32).copy(), np.int64(cur["stored"])
    d["sync_tick"], d["sync_brain"] = (np.array([s[i] for s in syncs], np.int32) for i in range(2))
    d["states"], d["out_init"], d["out_first"], d["out_final"] = states, out_init, out_first, out_final
    d["final_0"] = finals[0]
    d["first_update_tick"] = np.array(first_tick, np.int32)
    d["ref_grad_err"], d["ref_q_spread"], d["effect"] = grad_err, spread, effect
    margin = pc.margins(d["call_uniforms"], d["call_bracket"])
    d["cdf_err"], d["min_margin"] = np.float64(cur["D"]), np.float64(margin.min())
    d["tick_seconds"] = np.array(rec["seconds"], np.float64)

    # ---- the premises: keep this seed? ----
    ft = first_tick[0]
    rel = np.where(d["greedy"] == 1, d["gap"] / np.maximum(d["qmax"], 1e-30), np.inf)
    absg = np.where(d["greedy"] == 1, d["gap"], np.inf)
    why = None
    if rel[:ft + 1].min() < 1e-5:
        why = "a greedy decision before the first update with a relative gap of %.3g" % rel[:ft + 1].min()
    elif ft + 1 < T and absg[ft + 1:].min() < 10 * bar_abs:
        why = "a greedy decision after the first update with a gap of %.3g < 10 x the bar %.3g" % (absg[ft + 1:].min(), bar_abs)
    elif cur["stored"] < 2 * C:
        why = "the memory does not wrap twice: %d rows through a capacity of %d" % (cur["stored"], C)
    elif len(calls) < 20:
        why = "%d train() calls, fewer than 20" % len(calls)
    elif not d["call_sync"].any():
        why = "no target copy rides on an update"
    elif margin.min() < pc.SNAPSHOT_MARGIN:
        why = "a draw %.3g from an end of its bracket, closer than 2^-20" % margin.min()
    elif margin.min() < pc.RUN_MARGIN_FACTOR * cur["D"]:
        why = "a draw %.3g from an end of its bracket, closer than 8 D = %.3g" % (margin.min(), pc.RUN_MARGIN_FACTOR * cur["D"])
    info = ("seed %d: %d ticks, %d rows stored, %d calls (len %d..%d), %d on a target copy, %d bare syncs, first update at tick %d, "
            "ref_grad_err %s ref_q_spread %s effect %s, absolute bar %.3g, D %.3g, smallest margin %.3g, %.1f ms per tick"
            % (seed, T, cur["stored"], len(calls), d["call_size"].min(), d["call_size"].max(), int(d["call_sync"].sum()), len(syncs), ft,
               grad_err, spread, effect, bar_abs, cur["D"], margin.min(), 1e3 * np.mean(rec["seconds"])))
    return (d if why is None else None), (info if why is None else "seed %d: %s" % (seed, why))


def main():
    span = next((tuple(int(x) for x in a.split(":")) for a in sys.argv[1:] if ":" in a), (FIRST_SEED, FIRST_SEED + 200))
    for seed in range(*span):
        d, info = run(seed)
        print(info, flush=True)
        if d is not None:
            np.savez_compressed(pc.path(), **d)
            print("wrote %s (%.0f KB)" % (pc.path(), os.path.getsize(pc.path()) / 1024))
            return
    raise SystemExit("no seed met the premises")


if __name__ == "__main__":
    main()
