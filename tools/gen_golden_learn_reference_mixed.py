"""The learn="reference" fixture with several opt-in brains from the real reference (build container only; data in, data out -- no
reference source is copied).

Runs the reference's own trainer loop body (ReinLife/Helpers/trainer.py:85-99) with two real PERD3QN and two real PERDQN brains in one
world (PERD3QN, PERDQN, PERD3QN, PERDQN), each carrying repo-generated weights and the constructor arguments of its single-kind
fixture, and records what tests/learn_reference_mixed_cases.py lists.  The recorders, the seeding, the decisions' gaps and the
yardsticks are those of tools/gen_golden_learn_reference.py (Shadow, digest, flat), ..._prioritized.py (env_draws) and ..._td.py /
gen_golden_learn_perdqn.py (NpCompat), imported from there; what is new is that every brain's train() / store / sample is wrapped on ITS
instance, that every call of the run is noted in one list in the order made (call_order), and that each brain's float64 twin follows
its own calls only.  The reference's files are not modified.

Seeds are searched until learn_reference_mixed_cases.premises() names nothing and sensitive() names no brain: replayed with each tick's
agents handed to the schedule sorted by brain, every brain gets other uniforms than it consumed.  A run in which Memory.sample
repeated a draw is dropped.

    python tools/gen_golden_learn_reference_mixed.py [first:last]

SEED is the seed the committed fixture was made from (the first of 1..200 that met the premises); first:last searches another range.
The file holds no timings and its members carry no dates, so the seed reproduces it byte for byte.
"""
import copy
import os
import random
import sys
import zipfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden_learn_reference as base  # noqa: E402  (puts the repository root and tests/ on sys.path)
import gen_golden_learn_reference_prioritized as gp  # noqa: E402
from gen_golden_learn_perdqn import NpCompat  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402
import learn_reference_cases as lrc  # noqa: E402
import learn_reference_mixed_cases as mc  # noqa: E402
import learn_reference_prioritized_cases as pc  # noqa: E402
import learn_reference_td_cases as tc  # noqa: E402

SEED = 88
NAME = "pairs"
NETS = mc.NETS


class Retried(Exception):
    pass


class TdTwin:
    """A PERDQN brain's float64 twin (tools/gen_golden_learn_reference_td.py's, as an object): the same updates on the recorded batches
    with the recorded importance weights, float64 leaves by the same add / update rules, and the first step's gradients in both types."""

    def __init__(self, torch, brain):
        self.torch, self.brain = torch, brain
        self.q, self.t = copy.deepcopy(brain.model).double(), copy.deepcopy(brain.target_model).double()
        self.opt = torch.optim.Adam(self.q.parameters(), lr=brain.optimizer.param_groups[0]["lr"])
        self.leaves = np.zeros(brain.memory_size, np.float64)
        self.grad_err = None

    def loss(self, q, t, batch, w_is, dtype):
        torch = self.torch
        s = torch.tensor(np.vstack([x[0] for x in batch]), dtype=dtype)
        a = torch.tensor([int(x[1]) for x in batch])
        r = torch.tensor([float(x[2]) for x in batch], dtype=dtype)
        sp = torch.tensor(np.vstack([x[3] for x in batch]), dtype=dtype)
        d = torch.tensor([float(int(x[4])) for x in batch], dtype=dtype)
        pred = q(s).gather(1, a.unsqueeze(1)).squeeze(1)
        target = r + (1 - d) * self.brain.discount_factor * t(sp).max(1)[0].detach()
        return (torch.tensor(w_is, dtype=dtype) * torch.nn.functional.mse_loss(pred, target)).mean(), (pred - target).abs().detach()

    def follow(self, net32, target32, batch, w_is, idxs):
        torch, mem, C = self.torch, self.brain.memory, self.brain.memory_size
        if self.grad_err is None:
            g32 = torch.autograd.grad(self.loss(net32, target32, batch, w_is, torch.float32)[0], list(net32.parameters()))
            g64 = torch.autograd.grad(self.loss(self.q, self.t, batch, w_is, torch.float64)[0], list(self.q.parameters()))
            g32, g64 = (np.concatenate([x.numpy().reshape(-1) for x in g]) for g in (g32, g64))
            self.grad_err = float(np.abs(g32 - g64).max() / np.abs(g64).max())
        loss, err64 = self.loss(self.q, self.t, batch, w_is, torch.float64)
        for i, e in zip(idxs, err64.numpy()):      # train_model's update loop by the twin, before its step
            self.leaves[i - (C - 1)] = (abs(e) + mem.e) ** mem.a
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()

    def sync(self):
        self.t.load_state_dict(self.q.state_dict())


def build(ref, torch, kind, seed):
    kw = dict(mc.ARGS[kind])
    if kind == "PERDQN":
        brain = sys.modules["ReinLife.Models.PERDQN"].PERDQNAgent(**kw)
        brain.train_start = tc.CASE["train_start"]
    else:
        brain = getattr(ref, kind)(**kw)
    w = mc.weights(kind, seed)
    for net in NETS[kind]:
        off = 0
        with torch.no_grad():
            for t in getattr(brain, net).state_dict().values():
                t.copy_(torch.from_numpy(w[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                off += t.numel()
        assert off == w.size
    return brain, w


def run(name, seed):
    case = mc.CASES[name]
    kinds, nb = case["kinds"], len(case["kinds"])
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.PERDQN  # noqa: F401
    sys.modules["ReinLife.Models.PERDQN"].np = NpCompat()
    init_seeds = [1000 + 10 * seed + b for b in range(nb)]
    brains, inits = zip(*[build(ref, torch, kinds[b], init_seeds[b]) for b in range(nb)])
    net_of = lambda b: getattr(brains[b], NETS[kinds[b]][0])  # noqa: E731
    params = lambda b: base.flat(net_of(b).state_dict()).astype(np.float32)  # noqa: E731
    shadows = [TdTwin(torch, brains[b]) if kinds[b] == "PERDQN" else base.Shadow(torch, pc.KIND, brains[b])
               for b in range(nb)]
    prio64 = {b: np.zeros(brains[b].buffer.capacity, np.float64) for b in range(nb) if kinds[b] == "PERD3QN"}
    cur = {"tick": 0, "trained": None}
    stored, stamped, stale, D = [0] * nb, [0] * nb, [False] * nb, [0.0] * nb
    calls, firsts, first_tick = [], [None] * nb, [-1] * nb
    detail = [[] for _ in range(nb)]           # per brain, per "learn" call: what its own fixture records

    def note(b, kind, size=0, sync=False, group=None, **more):
        calls.append((cur["tick"], b, mc.CALL_KINDS.index(kind), int(size), int(sync), stored[b], group or (-1, -1)))
        if kind in ("learn", "ppo"):
            detail[b].append(more)
            if firsts[b] is None:
                firsts[b], first_tick[b] = params(b), cur["tick"]

    def group_of(b):
        first, stamped[b] = stamped[b], stored[b]
        return (first, stored[b] - first)

    def wrap_perd3qn(b, brain):
        sh, buf, p64 = shadows[b], brain.buffer, prio64[b]
        orig_store, orig_sample, orig_train = buf.store, buf.sample, brain.train
        B, alpha64 = brain.batch_size, float(pc.ALPHA)

        def store(*a, **k):
            p64[buf.pos] = p64.max() if buf.memory else 1.0     # PERD3QN.py:147, 153 in float64
            stored[b] += 1
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
            cdf64 = ((p64[:n] ** alpha64) / (p64[:n] ** alpha64).sum()).cumsum()
            D[b] = max(D[b], float(np.abs(cdf64 / cdf64[-1] - pc.choice_cdf(prio)).max()))
            orig_train()
            after = np.random.get_state()
            assert np.array_equal(cur["indices"], idx), "np.random.choice is not cdf.searchsorted(random_sample(batch), side='right')"
            assert after[2] == drawn[2] and np.array_equal(after[1], drawn[1]), "np.random.choice consumed other draws than random_sample(batch)"
            with torch.no_grad():   # update_priorities (PERD3QN.py:110-111) by the float64 twin, before its step
                s = torch.tensor(np.concatenate([x[0] for x in batch], 0), dtype=torch.float64)
                a = torch.tensor([int(x[1]) for x in batch])
                sp = torch.tensor(np.concatenate([x[3] for x in batch], 0), dtype=torch.float64)
                new = (sh.t.forward(sp).max(1)[0] - sh.q.forward(s).gather(1, a.unsqueeze(1)).squeeze(1)).abs().numpy()
            for i, p in zip(idx, new):
                p64[i] = p
            sh.step([batch])
            cur["trained"] = dict(size=n, uniforms=u, indices=idx.astype(np.int32), prio=np.concatenate([prio, np.zeros(buf.capacity - n, np.float32)]),
                                  bracket=bracket, new_prio=buf.priorities[idx].copy())
        buf.store, buf.sample, brain.train = store, sample, train

    def wrap_perdqn(b, brain):
        tw, mem, C, B = shadows[b], brain.memory, brain.memory_size, brain.batch_size
        orig_sample, orig_update, orig_train, orig_add = mem.sample, mem.update, brain.train_model, mem.add

        def add(error, sample):
            assert float(error) == 0.0, "append_sample's error is no longer exactly 0"
            tw.leaves[stored[b] % C] = (0.0 + mem.e) ** mem.a
            stored[b] += 1
            return orig_add(error, sample)

        def sample(n):
            total = float(mem.tree.tree[0])
            batch, idxs, w_is = orig_sample(n)
            cur["sample"] = dict(batch=batch, idxs=np.array(idxs, np.int64), is_weight=np.array(w_is, np.float64), total=total,
                                 leaves=mem.tree.tree[np.array(idxs)].copy())
            return batch, idxs, w_is

        def update(idx, error):
            cur["errors"].append((int(idx), error))
            return orig_update(idx, error)

        def train_model():
            model = tc.TreeModel(C, C)             # the literal model on the reference's own tree, for the walk
            model.tree[:] = mem.tree.tree
            model.stored = stored[b]
            state = random.getstate()
            u = np.array([random.random() for _ in range(B)], np.float64)
            drawn = random.getstate()
            random.setstate(state)
            want = model.sample(u)
            lo = np.array([model.leaf_lo(i) for i in want["idxs"]], np.float64)
            D[b] = max(D[b], float(np.abs(np.cumsum(mem.tree.tree[C - 1:]) - np.cumsum(tw.leaves)).max()))
            cur["errors"] = []
            target32, net32 = copy.deepcopy(brain.target_model), copy.deepcopy(brain.model)
            orig_train()
            if random.getstate() != drawn:
                raise Retried()
            sm = cur["sample"]
            assert not want["bad"] and np.array_equal(sm["idxs"], want["idxs"]), "Memory.sample is not the walk from a + (b - a) * random.random()"
            assert np.array_equal(sm["leaves"], want["leaves"]) and [i for i, _ in cur["errors"]] == sm["idxs"].tolist()
            errors = np.array([e for _, e in cur["errors"]])
            assert errors.dtype == np.float32
            tw.follow(net32, target32, sm["batch"], sm["is_weight"], sm["idxs"])
            cur["trained"] = dict(size=min(stored[b], C), uniforms=u, idxs=sm["idxs"].astype(np.int32), s=want["s"], leaves=sm["leaves"], lo=lo,
                                  total=sm["total"], is_weight=sm["is_weight"], errors=errors, epsilon=float(brain.epsilon))
        mem.add, mem.sample, mem.update, brain.train_model = add, sample, update, train_model

    for b, brain in enumerate(brains):
        {"PERD3QN": wrap_perd3qn, "PERDQN": wrap_perdqn}[kinds[b]](b, brain)

    rh.seed_all(seed)   # after construction: the constructors consume torch's generator
    rh.LOG.clear()
    env = rh.make_env(brains=list(brains), width=case["width"], height=case["height"], max_agents=case["max_agents"], static_families=True)
    env.reset()
    reset_draws, digest0, np_digest0, np_state0 = gp.env_draws()[0], base.digest(), pc.np_digest(), np.random.get_state()
    assert np_state0[3] == 0, "np.random holds a cached gaussian after reset()"
    rec = {k: [] for k in ("actions", "pre", "post", "digest", "np_digest", "dec", "step_draws", "upd_draws", "np_step_draws", "np_upd_draws")}
    pool = [[] for _ in range(nb)]
    for t in range(case["max_ticks"]):
        cur["tick"] = t
        dec, acts, pre = [], [], []
        for agent in env.agents:
            b = agent.brain._tmpl
            kind = kinds[b]
            x = torch.from_numpy(np.asarray(agent.state)).float()
            with torch.no_grad():
                out = (brains[b].eval_net(x[None])[0] if kind == "PERD3QN" else brains[b].model(x[None])[0]).numpy()
            py, npy = random.getstate(), np.random.get_state()
            agent.get_action(t)
            py_after, np_after = random.getstate(), np.random.get_state()
            random.setstate(py); np.random.set_state(npy)
            coin, np_coin = random.random(), np.random.rand()
            random.setstate(py_after); np.random.set_state(np_after)
            eps = brains[b].epsilon
            greedy = coin > eps if kind == "PERD3QN" else not np_coin <= eps        # PERD3QN.py:204-210, PERDQN.py:104
            top = np.sort(out)[::-1]
            dec.append((int(greedy), float(top[0] - top[1]), float(np.abs(out).max()), float(out[agent.action])))
            if greedy:
                assert int(agent.action) == int(out.argmax())
            acts.append(int(agent.action)); pre.append(b)
            pool[b].append((t, np.asarray(agent.state, np.float32)))
        rh.LOG.clear()
        env.step()
        py, npd = gp.env_draws()
        rec["step_draws"].append(py); rec["np_step_draws"].append(npd)
        rec["post"].append([(a.brain._tmpl, a.age, int(a.dead)) for a in env.agents])
        for agent in env.agents:
            b = agent.brain._tmpl
            kind, brain = kinds[b], brains[b]
            cur["trained"] = None
            try:
                agent.learn(n_epi=t)
            except Retried:
                return None, "%s seed %d: Memory.sample repeated a draw at tick %d" % (name, seed, t)
            if kind == "PERD3QN" and agent.age > 1 and t > brain.exploration:
                sync = t % brain.soft_update_freq == 0
                if cur["trained"]:
                    tr = dict(cur["trained"])
                    note(b, "learn", tr.pop("size"), sync, group_of(b), **tr)
                    stale[b] = not sync
                    if sync:
                        shadows[b].sync()
                elif sync and stale[b]:
                    note(b, "sync")
                    stale[b] = False
                    shadows[b].sync()
            if kind == "PERDQN" and agent.age > 1 and (agent.age % brain.train_freq == 0 or agent.dead):
                shadows[b].sync()                        # learn(): update_target_model() after every trigger
                if cur["trained"]:
                    tr = dict(cur["trained"])
                    note(b, "learn", tr.pop("size"), True, group_of(b), **tr)
        for b in range(nb):                              # the rows a brain stored behind its tick's last train()
            if stamped[b] < stored[b]:
                note(b, "store", group=group_of(b))
        assert gp.env_draws() == ([], []), "learn() drew through the environment's module"
        env.update_env(t)
        py, npd = gp.env_draws()
        rec["upd_draws"].append(py); rec["np_upd_draws"].append(npd)
        rec["actions"].append(acts); rec["dec"].append(dec); rec["pre"].append(pre)
        rec["digest"].append(base.digest()); rec["np_digest"].append(pc.np_digest())
    T = len(rec["actions"])
    if any(f is None for f in firsts):
        return None, "%s seed %d: a brain never trained in %d ticks (rows stored per brain: %s)" % (name, seed, T, stored)
    finals = [params(b) for b in range(nb)]
    every = sorted((tt, i, b) for b in range(nb) for i, (tt, _) in enumerate(pool[b]) if tt >= T // 2)
    states = np.stack([pool[b][i][1] for _, i, b in [every[j] for j in np.linspace(0, len(every) - 1, lrc.N_STATES).astype(int)]])
    o = lambda b, w: mc.outputs64(kinds[b], w, states)  # noqa: E731
    maxn = max(max(len(a) for a in rec["actions"]), max(len(p) for p in rec["post"]), 1)
    pad = lambda rows, dt, fill=0: np.stack([np.concatenate([np.asarray(r, dt).reshape(-1), np.full(maxn - len(r), fill, dt)]) for r in rows])  # noqa: E731
    d = {"seed": np.int64(seed), "ticks": np.int64(T), "max_epi": np.int64(case["max_ticks"]), "init_seeds": np.array(init_seeds, np.int64),
         "cfg": np.array([case["width"], case["height"], case["max_agents"], nb], np.int64),
         "n0": np.array([len(a) for a in rec["actions"]], np.int32), "actions": pad(rec["actions"], np.int8, -1),
         "pre_brain": pad(rec["pre"], np.int32), "n1": np.array([len(p) for p in rec["post"]], np.int32)}
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
    for i, key in enumerate(("call_tick", "call_brain", "call_kind", "call_size", "call_sync", "call_stored")):
        d[key] = np.array([c[i] for c in calls], np.int32)
    d["call_store"] = np.array([c[6] for c in calls], np.int32).reshape(-1, 2)
    d["states"] = states
    effect, spread, grad_err = np.zeros(nb), np.zeros(nb), np.zeros(nb)
    for b in range(nb):
        d["out_init_%d" % b], d["out_first_%d" % b], d["out_final_%d" % b] = o(b, inits[b]), o(b, firsts[b]), o(b, finals[b])
        out64 = o(b, base.flat(shadows[b].q.state_dict()))
        effect[b] = np.abs(d["out_final_%d" % b] - d["out_init_%d" % b]).max()
        spread[b] = np.abs(d["out_final_%d" % b] - out64).max() / effect[b]
        grad_err[b] = shadows[b].grad_err
        stack = lambda key, dt: np.stack([c[key] for c in detail[b]]).astype(dt)  # noqa: E731
        if kinds[b] == "PERD3QN":
            d["uniforms_%d" % b], d["indices_%d" % b] = stack("uniforms", np.float64), stack("indices", np.int32)
            d["prio_%d" % b], d["bracket_%d" % b] = stack("prio", np.float32), stack("bracket", np.float64)
            d["new_prio_%d" % b] = stack("new_prio", np.float32)
            d["final_prio_%d" % b] = brains[b].buffer.priorities.astype(np.float32).copy()
        if kinds[b] == "PERDQN":
            d["uniforms_%d" % b], d["idxs_%d" % b] = stack("uniforms", np.float64), stack("idxs", np.int32)
            for key in ("s", "leaves", "lo", "is_weight"):
                d["%s_%d" % (key, b)] = stack(key, np.float64)
            d["errors_%d" % b] = stack("errors", np.float32)
            d["total_%d" % b], d["epsilon_%d" % b] = (np.array([c[k] for c in detail[b]], np.float64) for k in ("total", "epsilon"))
            d["final_tree_%d" % b] = brains[b].memory.tree.tree.astype(np.float64).copy()
    td = lambda f: np.array([f(b) if kinds[b] == "PERDQN" else 0.0 for b in range(nb)], np.float64)  # noqa: E731
    d["final_beta"], d["final_epsilon"] = td(lambda b: brains[b].memory.beta), td(lambda b: brains[b].epsilon)
    d["interval_err"] = td(lambda b: D[b])
    d["cdf_err"] = np.array([D[b] if kinds[b] == "PERD3QN" else 0.0 for b in range(nb)], np.float64)
    d["first_update_tick"], d["final_stored"] = np.array(first_tick, np.int32), np.array(stored, np.int64)
    d["ref_grad_err"], d["ref_q_spread"], d["effect"] = grad_err, spread, effect

    # ---- the premises: keep this seed? ----
    miss = mc.premises(name, d)
    if not miss and mc.sensitive(name, d):
        miss = ["replayed with the agents sorted by brain, brains %s draw the uniforms they drew" % mc.sensitive(name, d)]
    per = np.bincount(d["call_brain"][d["call_kind"] != 3], minlength=nb)
    info = "%s seed %d: %d ticks, rows stored %s, calls per brain %s, first updates at %s, bars %s, D %s" % (
        name, seed, T, stored, per.tolist(), first_tick, mc.bars(d), [float("%.3g" % x) for x in D])
    return (d if not miss else None), info + ("" if not miss else "\n    dropped: " + "; ".join(miss))


def save(path, d):
    """np.savez_compressed without the clock: every member dated 1980-01-01, so that a seed reproduces its file byte for byte."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key, value in d.items():
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(value), allow_pickle=False)


def main():
    span = next((tuple(int(x) for x in a.split(":")) for a in sys.argv[1:] if ":" in a), (SEED, SEED + 1))
    for seed in range(*span):
        d, info = run(NAME, seed)
        print(info, flush=True)
        if d is not None:
            save(mc.path(NAME), d)
            print("wrote %s (%.0f KB)" % (mc.path(NAME), os.path.getsize(mc.path(NAME)) / 1024))
            return
    raise SystemExit("no seed of %d..%d met the premises" % (span[0], span[1] - 1))


if __name__ == "__main__":
    main()
