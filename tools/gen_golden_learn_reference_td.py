"""The learn_reference_td=True fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Runs the reference's own trainer loop body (ReinLife/Helpers/trainer.py:85-99) with one real PERDQN brain carrying repo-generated weights
(capacity 64, explore_step 20, train_start set to 48), as tools/gen_golden_learn_reference_prioritized.py runs its PERD3QN brain -- the
same recorders, seeding, decisions' gaps and yardsticks -- and records what tests/learn_reference_td_cases.py lists: both generators'
digests per tick and, per train_model(), the uniforms Memory.sample's random.uniform calls consumed, the tree indices it answered, the
leaves it read, is_weight, the errors handed to update() and tree[0].  The reference's files are not modified: train_model, memory.sample
and memory.update are wrapped on the brain instance, and the module gets the ragged-np.array stand-in of tools/gen_golden_learn_perdqn.py.

Every call checks that Memory.sample is what the cases module states: from u = [random.random() for _ in range(batch)] drawn at the state
before the call, the literal model's walk names the indices the reference named, and `random` is left in the state those draws leave it in
-- a draw that the reference repeated (a leaf no row has reached) shows as another state, and the seed is dropped.

A float64 twin follows the run on the recorded batches with the recorded importance weights and keeps float64 leaves by the same add /
update rules; at every call the cumulative sums of its leaves are compared with the run's: D is the largest difference.

Seeds are searched until the premises hold (the end of run()): the memory wraps at least twice, at least 20 train_model() calls, a batch
that names a leaf twice, no draw repeated, the greedy decisions' gaps as for the other fixtures, and EVERY draw at least 8 D and at least
2^-20 of the total from both ends of its leaf's interval.

    python tools/gen_golden_learn_reference_td.py [first:last]
"""
import copy
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_learn_reference as base  # noqa: E402  (puts the repository root and tests/ on sys.path)
import gen_golden_learn_reference_prioritized as gp  # noqa: E402
from gen_golden_learn_perdqn import NpCompat  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
import learn_reference_cases as lrc  # noqa: E402
import learn_reference_prioritized_cases as pc  # noqa: E402
import learn_reference_td_cases as tc  # noqa: E402

FIRST_SEED = 1   # the seed range the committed fixture was searched from


class Retried(Exception):
    pass


def run(seed):
    case = tc.CASE
    ref = rh.load_reference()
    torch = ref.torch
    import ReinLife.Models.PERDQN  # noqa: F401
    mod = sys.modules["ReinLife.Models.PERDQN"]
    mod.np = NpCompat()
    init_seed = 1000 + 10 * seed
    brain = mod.PERDQNAgent(**case["args"])
    brain.train_start = case["train_start"]
    w = tc.weights(init_seed)
    for net in ("model", "target_model"):
        off = 0
        with torch.no_grad():
            for t in getattr(brain, net).state_dict().values():
                t.copy_(torch.from_numpy(w[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                off += t.numel()
    params = lambda: base.flat(brain.model.state_dict()).astype(np.float32)  # noqa: E731
    mem, C, B = brain.memory, brain.memory_size, brain.batch_size
    gamma, lr = brain.discount_factor, brain.optimizer.param_groups[0]["lr"]
    q64, t64 = copy.deepcopy(brain.model).double(), copy.deepcopy(brain.target_model).double()
    opt64 = torch.optim.Adam(q64.parameters(), lr=lr)
    leaves64 = np.zeros(C, np.float64)        # the float64 twin's leaves, by memory index
    twin = {"grad_err": None}
    cur = {"stored": 0, "D": 0.0, "trained": None}
    calls, first, first_tick = [], [None], [-1]
    orig_sample, orig_update, orig_train, orig_add = mem.sample, mem.update, brain.train_model, mem.add

    def add(error, sample):
        assert float(error) == 0.0, "append_sample's error is no longer exactly 0"
        leaves64[cur["stored"] % C] = (0.0 + mem.e) ** mem.a
        cur["stored"] += 1
        return orig_add(error, sample)

    def sample(n):
        total = float(mem.tree.tree[0])
        batch, idxs, w_is = orig_sample(n)
        cur["sample"] = dict(batch=batch, idxs=np.array(idxs, np.int64), is_weight=np.array(w_is, np.float64), total=total,
                             leaves=mem.tree.tree[np.array(idxs)].copy(), beta=float(mem.beta))
        return batch, idxs, w_is

    def update(idx, error):
        cur["errors"].append((int(idx), error))
        return orig_update(idx, error)

    def loss_of(q, t, batch, w_is, dtype):
        s = torch.tensor(np.vstack([x[0] for x in batch]), dtype=dtype)
        a = torch.tensor([int(x[1]) for x in batch])
        r = torch.tensor([float(x[2]) for x in batch], dtype=dtype)
        sp = torch.tensor(np.vstack([x[3] for x in batch]), dtype=dtype)
        d = torch.tensor([float(int(x[4])) for x in batch], dtype=dtype)
        pred = q(s).gather(1, a.unsqueeze(1)).squeeze(1)
        target = r + (1 - d) * gamma * t(sp).max(1)[0].detach()
        return (torch.tensor(w_is, dtype=dtype) * torch.nn.functional.mse_loss(pred, target)).mean(), (pred - target).abs().detach()

    def train_model():
        n = min(cur["stored"], C)
        model = tc.TreeModel(C, C)             # the literal model on the reference's own tree, for the walk
        model.tree[:] = mem.tree.tree
        model.stored = cur["stored"]
        state = random.getstate()
        u = np.array([random.random() for _ in range(B)], np.float64)
        drawn = random.getstate()
        random.setstate(state)
        want = model.sample(u)
        lo = np.array([model.leaf_lo(i) for i in want["idxs"]], np.float64)
        cum32, cum64 = np.cumsum(mem.tree.tree[C - 1:]), np.cumsum(leaves64)
        cur["D"] = max(cur["D"], float(np.abs(cum32 - cum64).max()))
        cur["errors"] = []
        target32 = copy.deepcopy(brain.target_model)
        net32 = copy.deepcopy(brain.model)
        orig_train()
        if random.getstate() != drawn:
            raise Retried()
        sm = cur["sample"]
        assert not want["bad"] and np.array_equal(sm["idxs"], want["idxs"]), "Memory.sample is not the walk from a + (b - a) * random.random()"
        assert np.array_equal(sm["leaves"], want["leaves"])
        assert [i for i, _ in cur["errors"]] == sm["idxs"].tolist()
        errors = np.array([e for _, e in cur["errors"]])
        assert errors.dtype == np.float32
        if twin["grad_err"] is None:
            g32 = torch.autograd.grad(loss_of(net32, target32, sm["batch"], sm["is_weight"], torch.float32)[0], list(net32.parameters()))
            g64 = torch.autograd.grad(loss_of(q64, t64, sm["batch"], sm["is_weight"], torch.float64)[0], list(q64.parameters()))
            g32, g64 = (np.concatenate([x.numpy().reshape(-1) for x in g]) for g in (g32, g64))
            twin["grad_err"] = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        loss, err64 = loss_of(q64, t64, sm["batch"], sm["is_weight"], torch.float64)
        for i, e in zip(sm["idxs"], err64.numpy()):      # train_model's update loop by the twin, before its step
            leaves64[i - (C - 1)] = (abs(e) + mem.e) ** mem.a
        opt64.zero_grad()
        loss.backward()
        opt64.step()
        cur["trained"] = dict(size=n, stored=cur["stored"], u=u, idxs=sm["idxs"], s=want["s"], leaves=sm["leaves"], lo=lo, total=sm["total"],
                              is_weight=sm["is_weight"], errors=errors, epsilon=float(brain.epsilon))

    mem.add, mem.sample, mem.update, brain.train_model = add, sample, update, train_model

    rh.seed_all(seed)   # after construction: the constructors consume torch's generator
    rh.LOG.clear()
    env = rh.make_env(brains=[brain], width=case["width"], height=case["height"], max_agents=case["max_agents"], static_families=True)
    env.reset()
    reset_draws, digest0, np_digest0, np_state0 = gp.env_draws()[0], base.digest(), pc.np_digest(), np.random.get_state()
    assert np_state0[3] == 0, "np.random holds a cached gaussian after reset()"
    rec = {k: [] for k in ("actions", "post", "digest", "np_digest", "dec", "seconds", "step_draws", "upd_draws", "np_step_draws", "np_upd_draws")}
    pool = []
    for t in range(case["max_ticks"]):
        t0 = time.perf_counter()
        dec, acts = [], []
        for agent in env.agents:
            with torch.no_grad():
                out = brain.model(torch.from_numpy(np.asarray(agent.state)).float()[None])[0].numpy()
            state = np.random.get_state()
            agent.get_action(t)
            after = np.random.get_state()
            np.random.set_state(state)
            coin = np.random.rand()
            np.random.set_state(after)
            greedy = not coin <= brain.epsilon           # PERDQN.py:104
            top = np.sort(out)[::-1]
            dec.append((int(greedy), float(top[0] - top[1]), float(np.abs(out).max()), float(out[agent.action])))
            if greedy:
                assert int(agent.action) == int(out.argmax())
            acts.append(int(agent.action))
            pool.append((t, np.asarray(agent.state, np.float32)))
        rh.LOG.clear()
        env.step()
        py, npd = gp.env_draws()
        rec["step_draws"].append(py); rec["np_step_draws"].append(npd)
        rec["post"].append([(0, a.age, int(a.dead)) for a in env.agents])
        for agent in env.agents:
            cur["trained"] = None
            try:
                agent.learn()
            except Retried:
                return None, "seed %d: Memory.sample repeated a draw at tick %d" % (seed, t)
            if agent.age > 1 and (agent.age % brain.train_freq == 0 or agent.dead):
                t64.load_state_dict(q64.state_dict())    # learn(): update_target_model() after every trigger
                if cur["trained"]:
                    calls.append(dict(cur["trained"], tick=t))
                    if first[0] is None:
                        first[0], first_tick[0] = params(), t
        assert gp.env_draws() == ([], []), "learn() drew through the environment's module"
        env.update_env(t)
        py, npd = gp.env_draws()
        rec["upd_draws"].append(py); rec["np_upd_draws"].append(npd)
        rec["actions"].append(acts); rec["dec"].append(dec)
        rec["digest"].append(base.digest()); rec["np_digest"].append(pc.np_digest())
        rec["seconds"].append(time.perf_counter() - t0)
    T = len(rec["actions"])
    if first[0] is None or len(calls) < 2:
        return None, "seed %d: the brain trained %d times in %d ticks (%d rows)" % (seed, len(calls), T, cur["stored"])
    later = [s for tt, s in pool if tt >= T // 2]
    states = np.stack([later[i] for i in np.linspace(0, len(later) - 1, lrc.N_STATES).astype(int)])
    o = lambda x: tc.outputs64(x, states)  # noqa: E731
    out_init, out_first, out_final = (np.stack([o(x)]) for x in (w, first[0], params()))
    out64 = np.stack([o(base.flat(q64.state_dict()))])
    effect = np.array([np.abs(out_final[0] - out_init[0]).max()])
    spread = np.array([np.abs(out_final[0] - out64[0]).max() / effect[0]])
    grad_err = np.array([twin["grad_err"]])
    bar_abs = float((spread * (1e-5 / grad_err) * effect).max())

    maxn = max(max(len(a) for a in rec["actions"]), max(len(p) for p in rec["post"]), 1)
    pad = lambda rows, dt, fill=0: np.stack([np.concatenate([np.asarray(r, dt).reshape(-1), np.full(maxn - len(r), fill, dt)]) for r in rows])  # noqa: E731
    d = {"seed": np.int64(seed), "ticks": np.int64(T), "max_epi": np.int64(case["max_ticks"]), "init_seeds": np.array([init_seed], np.int64),
         "cfg": np.array([case["width"], case["height"], case["max_agents"], 1], np.int64),
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
    d["capacity"], d["batch"], d["train_start"] = np.int64(C), np.int64(B), np.int64(brain.train_start)
    d["epsilon_decay"], d["epsilon_min"] = np.float64(brain.epsilon_decay), np.float64(brain.epsilon_min)
    d["call_tick"], d["call_size"], d["call_stored"] = (np.array([c[k] for c in calls], np.int32) for k in ("tick", "size", "stored"))
    d["call_uniforms"] = np.stack([c["u"] for c in calls]).astype(np.float64)
    d["call_idxs"] = np.stack([c["idxs"] for c in calls]).astype(np.int32)
    for key, name in (("s", "call_s"), ("leaves", "call_leaves"), ("lo", "call_lo"), ("is_weight", "call_is_weight")):
        d[name] = np.stack([c[key] for c in calls]).astype(np.float64)
    d["call_errors"] = np.stack([c["errors"] for c in calls]).astype(np.float32)
    d["call_total"], d["call_epsilon"] = (np.array([c[k] for c in calls], np.float64) for k in ("total", "epsilon"))
    d["duplicates"] = np.array([B - len(set(c["idxs"].tolist())) for c in calls], np.int32)
    d["final_tree"], d["final_leaves"] = mem.tree.tree.astype(np.float64).copy(), mem.tree.tree[C - 1:].astype(np.float64).copy()
    d["final_beta"], d["final_epsilon"], d["final_stored"] = np.float64(mem.beta), np.float64(brain.epsilon), np.int64(cur["stored"])
    d["states"], d["out_init"], d["out_first"], d["out_final"] = states, out_init, out_first, out_final
    d["final_0"] = params()
    d["first_update_tick"] = np.array(first_tick, np.int32)
    d["ref_grad_err"], d["ref_q_spread"], d["effect"] = grad_err, spread, effect
    margin = np.minimum(d["call_s"] - d["call_lo"], d["call_lo"] + d["call_leaves"] - d["call_s"])
    d["interval_err"], d["min_margin"] = np.float64(cur["D"]), np.float64(margin.min())
    d["min_margin_rel"] = np.float64((margin / d["call_total"][:, None]).min())
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
    elif not (d["greedy"][ft + 1:] == 1).any():
        why = "no greedy decision after the first update"
    elif cur["stored"] < 2 * C:
        why = "the memory does not wrap twice: %d rows through a capacity of %d" % (cur["stored"], C)
    elif len(calls) < 20:
        why = "%d train_model() calls, fewer than 20" % len(calls)
    elif not d["duplicates"].any():
        why = "no batch names a leaf twice"
    elif d["min_margin_rel"] < tc.REL_MARGIN:
        why = "a draw %.3g of the total from an end of its interval, closer than 2^-20" % d["min_margin_rel"]
    elif margin.min() < tc.RUN_MARGIN_FACTOR * cur["D"]:
        why = "a draw %.3g from an end of its interval, closer than 8 D = %.3g" % (margin.min(), tc.RUN_MARGIN_FACTOR * cur["D"])
    info = ("seed %d: %d ticks, %d rows stored, %d calls (size %d..%d), %d duplicated leaves, first update at tick %d, epsilon %.3g, "
            "ref_grad_err %s ref_q_spread %s effect %s, absolute bar %.3g, D %.3g, smallest margin %.3g (%.3g of the total), %.1f ms per tick"
            % (seed, T, cur["stored"], len(calls), d["call_size"].min(), d["call_size"].max(), int(d["duplicates"].sum()), ft, brain.epsilon,
               grad_err, spread, effect, bar_abs, cur["D"], margin.min(), d["min_margin_rel"], 1e3 * np.mean(rec["seconds"])))
    return (d if why is None else None), (info if why is None else "seed %d: %s" % (seed, why))


def main():
    span = next((tuple(int(x) for x in a.split(":")) for a in sys.argv[1:] if ":" in a), (FIRST_SEED, FIRST_SEED + 200))
    for seed in range(*span):
        d, info = run(seed)
        print(info, flush=True)
        if d is not None:
            np.savez_compressed(tc.path(), **d)
            print("wrote %s (%.0f KB)" % (tc.path(), os.path.getsize(tc.path()) / 1024))
            return
    raise SystemExit("no seed met the premises")


if __name__ == "__main__":
    main()
