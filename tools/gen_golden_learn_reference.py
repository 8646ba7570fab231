"""The learn="reference" fixtures from the real reference (build container only; data in, data out -- no reference source is copied).

Runs the reference's own trainer loop body (ReinLife/Helpers/trainer.py:85-99: get_action for every agent, step(), learn() for every
agent, update_env()) with its real DQN / D3QN / PPO brains carrying repo-generated weights, seeded as oracle/gen_golden_e2e.py seeds its
runs (brains first, then random / np.random / torch), and records what tests/learn_reference_cases.py lists: the post-step lists, the
actions, every train() call with the indices random.sample drew, a digest of the `random` stream per tick, the decisions' top-2 gaps, the
reference's outputs on 64 of the run's states and -- from a float64 replay of the recorded batches beside the float32 run -- the two
yardsticks ref_grad_err and ref_q_spread.  The reference's files are not modified: the `random` attribute of its DQN / D3QN modules is
replaced by a recording proxy and train() / learn() are wrapped per brain instance.

Closed-loop reproduction is only possible where no decision is a near-tie, so seeds are searched: a run is kept when every greedy
decision before the first update has a top-2 gap of at least 1e-5 of the row's largest |q| and every later one a gap of at least ten
times the fixture's absolute Q bar (ref_q_spread * 1e-5 / ref_grad_err * effect, the largest over the brains), and when it shows what
the case is there to show (the end of run()).  PPO's decisions are samples: their probabilities are recorded, no gap applies.

    python tools/gen_golden_learn_reference.py [dqn] [d3qn] [ppo] [first:last]

FIRST_SEED holds the seeds the committed fixtures were made from (the first of each search that met the premises); first:last searches
another range.
"""
import copy
import hashlib
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness as rh  # noqa: E402
import learn_reference_cases as lrc  # noqa: E402

FIRST_SEED = {"dqn": 170, "d3qn": 53, "ppo": 61}
SAMPLES = []   # what the proxy saw: (len(population), indices, the drawn elements)


class RandomProxy:
    """Stands in for `random` inside the reference's DQN / D3QN modules: sample() also notes which indices were drawn."""

    def sample(self, population, k):
        state = random.getstate()
        idx = random.sample(range(len(population)), k)
        random.setstate(state)
        got = random.sample(population, k)
        assert all(a is population[i] for a, i in zip(got, idx)), "random.sample(range(n), k) does not name random.sample(deque, k)'s elements"
        SAMPLES.append((len(population), idx, got))
        return got

    def __getattr__(self, name):
        return getattr(random, name)


def digest():
    return int.from_bytes(hashlib.sha256(repr(random.getstate()).encode()).digest()[:8], "little")


def env_draws():
    """The draws the reference's environment made from `random` since the log was cleared (oracle/ref_harness.py records them), as codes:
    0 = random.random(), n > 0 = random.choice of a sequence of n."""
    out = []
    for _, _, kind, _, extra in rh.LOG.entries:
        if kind == "py.random":
            out.append(0)
        elif kind == "py.choice":
            out.append(int(extra))
        else:
            assert kind.startswith("np."), "a draw of the environment this recorder does not know: %s" % kind
    rh.LOG.clear()
    return out


def flat(sd):
    return np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])


def gae32(delta, gl):
    adv, out = np.float32(0.0), np.zeros(len(delta), np.float32)
    for t in range(len(delta) - 1, -1, -1):
        adv = np.float32(np.float32(np.float32(gl) * adv) + np.float32(delta[t]))
        out[t] = adv
    return out


class Shadow:
    """One brain's float64 twin: the same updates on the same recorded batches, and the float32 / float64 gradients of the first."""

    def __init__(self, torch, kind, brain):
        self.torch, self.kind, self.brain = torch, kind, brain
        net = {"DQN": "agent", "D3QN": "eval_net", "PPO": "model"}[kind]
        self.net32 = getattr(brain, net)
        self.q = copy.deepcopy(self.net32).double()
        if kind == "PPO":
            self.q.optimizer = None
        self.t = copy.deepcopy(self.q) if kind != "PPO" else None
        lr = (brain.model.optimizer if kind == "PPO" else brain.optimizer).param_groups[0]["lr"]
        self.opt = torch.optim.Adam(self.q.parameters(), lr=lr)
        self.grad_err = None

    def _loss(self, q, t, batch, dtype):
        torch, F = self.torch, self.torch.nn.functional
        if self.kind == "DQN":   # DQN.py:144-149
            s = torch.tensor(np.array([x[0] for x in batch]), dtype=dtype)
            a = torch.tensor([[int(x[1])] for x in batch])
            r = torch.tensor([[float(x[2])] for x in batch], dtype=dtype)
            sp = torch.tensor(np.array([x[3] for x in batch]), dtype=dtype)
            dm = torch.tensor([[float(x[4])] for x in batch], dtype=dtype)
            return F.smooth_l1_loss(q(s).gather(1, a), r + 0.98 * t(sp).max(1)[0].unsqueeze(1) * dm)
        if self.kind == "D3QN":   # D3QN.py:100-113
            s = torch.tensor(np.concatenate([x[0] for x in batch], 0), dtype=dtype)
            a = torch.tensor([int(x[1]) for x in batch])
            r = torch.tensor([float(x[2]) for x in batch], dtype=dtype)
            sp = torch.tensor(np.concatenate([x[3] for x in batch], 0), dtype=dtype)
            d = torch.tensor([float(x[4]) for x in batch], dtype=dtype)
            nq = t.forward(sp).max(1)[0].detach()
            return F.mse_loss(q.forward(s).gather(1, a.unsqueeze(1)).squeeze(1), r + self.brain.gamma * (1 - d) * nq)
        m = self.brain.model   # PPO.py:140-158
        col = lambda v: torch.tensor(np.asarray(v, np.float64), dtype=dtype).unsqueeze(1)  # noqa: E731
        s = torch.tensor(np.array([x[0] for x in batch]), dtype=dtype)
        a = torch.tensor([[int(x[1])] for x in batch])
        r = col(np.array([x[2] for x in batch], np.float64).astype(np.float32))
        sp = torch.tensor(np.array([x[3] for x in batch]), dtype=dtype)
        pa = col(np.array([x[4] for x in batch], np.float64).astype(np.float32))
        mask = col([0.0 if x[5] else 1.0 for x in batch])
        td = r + m.gamma * q.v(sp) * mask
        v = q.v(s)
        delta = (td - v).detach().numpy()[:, 0]
        adv = torch.tensor(gae32(delta.astype(np.float32), m.gamma * m.lmbda).astype(np.float64), dtype=dtype).unsqueeze(1)
        ratio = torch.exp(torch.log(q.pi(s, softmax_dim=1).gather(1, a)) - torch.log(pa))
        surr1, surr2 = ratio * adv, torch.clamp(ratio, 1 - m.eps_clip, 1 + m.eps_clip) * adv
        return (-torch.min(surr1, surr2) + F.smooth_l1_loss(v, td.detach())).mean()

    def before(self, batches, target32=None):
        """The float32 gradient of the first step of the first update, by the reference's module, before anything changes."""
        if self.grad_err is not None:
            return
        torch = self.torch
        g32 = torch.autograd.grad(self._loss(self.net32, target32, batches[0], torch.float32), list(self.net32.parameters()))
        g64 = torch.autograd.grad(self._loss(self.q, self.t, batches[0], torch.float64), list(self.q.parameters()))
        g32, g64 = (np.concatenate([x.numpy().reshape(-1) for x in g]) for g in (g32, g64))
        self.grad_err = float(np.abs(g32 - g64).max() / np.abs(g64).max())

    def step(self, batches, epochs=1):
        for batch in batches:
            for _ in range(epochs):
                loss = self._loss(self.q, self.t, batch, self.torch.float64)
                self.opt.zero_grad()
                loss.backward()
                self.opt.step()

    def sync(self):
        self.t.load_state_dict(self.q.state_dict())


def run(name, seed, verbose=False):
    case = lrc.CASES[name]
    kind, nb = case["kind"], case["n_brains"]
    ref = rh.load_reference()
    torch = ref.torch
    mods = {}
    for k in ("DQN", "D3QN", "PPO"):
        __import__("ReinLife.Models." + k)
        mods[k] = sys.modules["ReinLife.Models." + k]
    mods["DQN"].random = mods["D3QN"].random = RandomProxy()
    max_epi = case["max_ticks"]
    init_seeds = [1000 + 10 * seed + b for b in range(nb)]
    brains, inits = [], []
    for b in range(nb):
        kw = dict(case["args"])
        if kind == "DQN":
            kw["max_epi"] = max_epi
        brain = getattr(ref, kind)(**kw)
        w = lrc.weights(kind, init_seeds[b])
        for net in {"DQN": ["agent", "target"], "D3QN": ["eval_net", "target_net"], "PPO": ["model"]}[kind]:
            off = 0
            with torch.no_grad():
                for t in getattr(brain, net).state_dict().values():
                    t.copy_(torch.from_numpy(w[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                    off += t.numel()
        brains.append(brain)
        inits.append(w)
    shadows = [Shadow(torch, kind, b) for b in brains]
    net_of = lambda b: {"DQN": "agent", "D3QN": "eval_net", "PPO": "model"}[kind]  # noqa: E731
    params = lambda b: flat(getattr(brains[b], net_of(b)).state_dict()).astype(np.float32)  # noqa: E731

    cur = {"tick": 0}
    calls, syncs, firsts, first_tick = [], [], [None] * nb, [-1] * nb

    def note(b, size, sync, indices):
        calls.append((cur["tick"], b, size, int(sync), indices))
        if firsts[b] is None:
            firsts[b], first_tick[b] = params(b), cur["tick"]

    def wrap(b, brain):
        sh = shadows[b]
        if kind == "DQN":
            orig = brain.train

            def train():
                n0 = len(SAMPLES)
                if brain.memory.size() > 1000:
                    # (the batches are not known before train() draws them: draw them once ahead on a saved stream, then let train() draw)
                    state = random.getstate()
                    ahead = [random.sample(brain.memory.buffer, 32) for _ in range(5)]
                    random.setstate(state)
                    sh.before(ahead, brain.target)
                orig()
                got = SAMPLES[n0:]
                if got:
                    assert len(got) == 5 and all(s[0] == got[0][0] for s in got)
                    sh.step([s[2] for s in got]); sh.sync()
                    note(b, got[0][0], True, np.array([s[1] for s in got], np.int32))
            brain.train = train
        elif kind == "D3QN":
            orig = brain.train

            def train():
                n0 = len(SAMPLES)
                state = random.getstate()
                ahead = [random.sample(brain.buffer.memory, brain.batch_size)]
                random.setstate(state)
                sh.before(ahead, brain.target_net)
                orig()
                got = SAMPLES[n0:]
                assert len(got) == 1
                sh.step([got[0][2]])
                cur["trained"] = (got[0][0], np.array([got[0][1]], np.int32))
            brain.train = train
        else:
            orig = brain.model.learn

            def learn():
                data = list(brain.model.data)
                sh.before([data])
                orig()
                sh.step([data], epochs=brain.model.k_epoch)
                note(b, len(data), False, None)
            brain.model.learn = learn

    for b, brain in enumerate(brains):
        wrap(b, brain)

    rh.seed_all(seed)   # after construction: the constructors consume torch's generator
    rh.LOG.clear()
    env = rh.make_env(brains=brains, width=case["width"], height=case["height"], max_agents=case["max_agents"], static_families=True)
    env.reset()
    reset_draws, digest0 = env_draws(), digest()
    rec = {k: [] for k in ("actions", "post", "digest", "dec", "seconds", "step_draws", "upd_draws")}
    pool = []
    stale = [False] * nb
    done_at = None
    for t in range(case["max_ticks"]):
        t0 = time.perf_counter()
        cur["tick"] = t
        dec, acts = [], []
        for agent in env.agents:
            b = agent.brain._tmpl
            with torch.no_grad():
                x = torch.from_numpy(agent.state).float()
                out = {"DQN": lambda: brains[b].agent(x), "D3QN": lambda: brains[b].eval_net(x[None])[0], "PPO": lambda: brains[b].model.pi(x)}[kind]().numpy()
            state = random.getstate()
            agent.get_action(t)
            after = random.getstate()
            random.setstate(state)
            coin = random.random()
            random.setstate(after)
            eps = getattr(brains[b], "epsilon", 0.0)
            greedy = {"DQN": coin >= eps, "D3QN": coin > eps, "PPO": False}[kind]
            top = np.sort(out)[::-1]
            dec.append((int(greedy), float(top[0] - top[1]), float(np.abs(out).max()), float(out[agent.action])))
            if greedy:
                assert int(agent.action) == int(out.argmax())
            acts.append(int(agent.action))
            pool.append((t, np.asarray(agent.state, np.float32)))
        rh.LOG.clear()
        env.step()
        rec["step_draws"].append(env_draws())
        rec["post"].append([(a.brain._tmpl, a.age, int(a.dead)) for a in env.agents])
        for agent in env.agents:
            b = agent.brain._tmpl
            cur["trained"] = None
            agent.learn(n_epi=t)
            if kind == "D3QN" and agent.age > 1 and t > brains[b].exploration:
                sync = t % brains[b].soft_update_freq == 0
                if cur["trained"]:
                    note(b, cur["trained"][0], sync, cur["trained"][1])
                    stale[b] = not sync
                    if sync:
                        shadows[b].sync()
                elif sync and stale[b]:
                    syncs.append((t, b))
                    stale[b] = False
                    shadows[b].sync()
        assert not env_draws(), "learn() drew through the environment's module"
        env.update_env(t)
        rec["upd_draws"].append(env_draws())
        rec["actions"].append(acts); rec["dec"].append(dec)
        rec["digest"].append(digest())
        rec["seconds"].append(time.perf_counter() - t0)
        per = [sum(1 for c in calls if c[1] == b) for b in range(nb)]
        if kind == "DQN" and min(per) >= 3:
            done_at = t
            break
        if kind == "DQN" and calls and t - calls[0][0] >= 12:   # (a dozen ticks after the first update and not done: another seed)
            break
    T = len(rec["actions"])
    finals = [params(b) for b in range(nb)]
    if any(f is None for f in firsts):
        return None, "%s seed %d: a brain never trained in %d ticks (rows stored per brain: %s)" % (
            name, seed, T, [sum(1 for p in rec["post"] for x in p if x[0] == b and x[1] > 1) for b in range(nb)])
    later = [s for tt, s in pool if tt >= T // 2]
    states = np.stack([later[i] for i in np.linspace(0, len(later) - 1, lrc.N_STATES).astype(int)])
    o = lambda w: lrc.outputs64(kind, w, states)  # noqa: E731
    out_init, out_first, out_final = (np.stack([o(w) for w in ws]) for ws in (inits, firsts, finals))
    out64 = np.stack([o(flat(sh.q.state_dict())) for sh in shadows])
    effect = np.array([np.abs(out_final[b] - out_init[b]).max() for b in range(nb)])
    spread = np.array([np.abs(out_final[b] - out64[b]).max() / effect[b] for b in range(nb)])
    grad_err = np.array([sh.grad_err for sh in shadows])
    bar_abs = float((spread * (1e-5 / grad_err) * effect).max())

    maxn = max(max(len(a) for a in rec["actions"]), max(len(p) for p in rec["post"]), 1)
    pad = lambda rows, dt, fill=0: np.stack([np.concatenate([np.asarray(r, dt).reshape(-1), np.full(maxn - len(r), fill, dt)]) for r in rows])  # noqa: E731
    d = {"seed": np.int64(seed), "ticks": np.int64(T), "max_epi": np.int64(max_epi), "init_seeds": np.array(init_seeds, np.int64),
         "cfg": np.array([case["width"], case["height"], case["max_agents"], nb], np.int64),
         "n0": np.array([len(a) for a in rec["actions"]], np.int32), "actions": pad(rec["actions"], np.int8, -1),
         "n1": np.array([len(p) for p in rec["post"]], np.int32)}
    for i, key in enumerate(("post_brain", "post_age", "post_dead")):
        d[key] = pad([[x[i] for x in p] for p in rec["post"]], np.int32)
    d["digest"], d["digest0"] = np.array(rec["digest"], np.uint64), np.uint64(digest0)
    wide = lambda rows: np.stack([np.concatenate([np.asarray(r, np.int32), np.full(max(map(len, rows)) - len(r), -1, np.int32)]) for r in rows])  # noqa: E731
    d["reset_draws"], d["step_draws"], d["upd_draws"] = np.array(reset_draws, np.int32), wide(rec["step_draws"]), wide(rec["upd_draws"])
    d["greedy"] = pad([[x[0] for x in r] for r in rec["dec"]], np.uint8)
    for i, key in ((1, "gap"), (2, "qmax"), (3, "chosen")):
        d[key] = pad([[x[i] for x in r] for r in rec["dec"]], np.float32)
    d["call_tick"], d["call_brain"], d["call_size"], d["call_sync"] = (np.array([c[i] for c in calls], np.int32) for i in range(4))
    if kind != "PPO":
        d["call_indices"] = np.stack([c[4] for c in calls]).astype(np.int32)
    d["sync_tick"], d["sync_brain"] = (np.array([s[i] for s in syncs], np.int32) for i in range(2))
    d["states"], d["out_init"], d["out_first"], d["out_final"] = states, out_init, out_first, out_final
    for b in range(nb):
        if kind != "PPO":
            d["init_%d" % b], d["first_%d" % b] = inits[b], firsts[b]
        if kind != "PPO" or b == 0:
            d["final_%d" % b] = finals[b]
    d["first_update_tick"] = np.array(first_tick, np.int32)
    d["ref_grad_err"], d["ref_q_spread"], d["effect"] = grad_err, spread, effect
    d["tick_seconds"] = np.array(rec["seconds"], np.float64)

    # ---- the premises: keep this seed? ----
    first = min(first_tick)
    rel = np.where(d["greedy"] == 1, d["gap"] / np.maximum(d["qmax"], 1e-30), np.inf)
    absg = np.where(d["greedy"] == 1, d["gap"], np.inf)
    why = None
    if kind != "PPO":
        if rel[:first + 1].min() < 1e-5:
            why = "a greedy decision before the first update with a relative gap of %.3g" % rel[:first + 1].min()
        elif first + 1 < T and absg[first + 1:].min() < 10 * bar_abs:
            why = "a greedy decision after the first update with a gap of %.3g < 10 x the bar %.3g" % (absg[first + 1:].min(), bar_abs)
    sizes = d["call_size"]
    if why is None and kind == "DQN":
        if done_at is None:
            why = "the brains did not both make three train() calls in %d ticks" % T
        elif done_at - first > 12:
            why = "the run ends %d ticks after the first update" % (done_at - first)
    if why is None and kind == "D3QN":
        stored = sum(1 for p in rec["post"] for x in p if x[1] > 1)
        ring = case["args"]["capacity"] + 64
        with_update = {int(tt) for tt, s in zip(d["call_tick"], d["call_sync"]) if s}
        if stored <= 2 * ring:
            why = "the ring does not lap: %d rows in a ring of %d" % (stored, ring)
        elif not with_update or not len(syncs) or not (set(int(s[0]) for s in syncs) - with_update):
            why = "no target copy on a tick with an update, or none on a tick without"
        elif sizes.max() < case["args"]["capacity"]:
            why = "the deque never fills"
    if why is None and kind == "PPO":
        if not ((sizes == 1).any() and ((sizes >= 2) & (sizes <= 32)).any()):
            why = "no list of one row, or none of 2..32 rows"
        elif min(sum(1 for c in calls if c[1] == b) for b in range(nb)) < 3:
            why = "a brain with fewer than three learn() calls"
    info = ("%s seed %d: %d ticks, %d calls (sizes %d..%d), %d bare syncs, first update at tick %s, ref_grad_err %s ref_q_spread %s effect %s, "
            "absolute bar %.3g, smallest greedy gap before / after the first update %.3g (relative) / %.3g, %.1f ms per tick"
            % (name, seed, T, len(calls), sizes.min(), sizes.max(), len(syncs), first_tick, grad_err, spread, effect, bar_abs,
               rel[:first + 1].min(), absg[first + 1:].min() if first + 1 < T else np.inf, 1e3 * np.mean(rec["seconds"])))
    if kind == "PPO":
        info += "; lists longer than 32 rows: %d (longest %d)" % ((sizes > 32).sum(), sizes.max())
    return (d if why is None else None), (info if why is None else "%s seed %d: %s" % (name, seed, why))


def main():
    args = [a for a in sys.argv[1:] if ":" not in a]
    span = next((tuple(int(x) for x in a.split(":")) for a in sys.argv[1:] if ":" in a), None)   # first:last, a seed range to search instead
    for name in (args or sorted(lrc.CASES)):
        for seed in range(*(span or (FIRST_SEED[name], FIRST_SEED[name] + 40))):
            try:
                d, info = run(name, seed)
            except ValueError as e:   # (D3QN: random.sample on a deque shorter than the batch)
                d, info = None, "%s seed %d: ValueError: %s" % (name, seed, e)
            print(info, flush=True)
            if d is not None:
                np.savez_compressed(lrc.path(name), **d)
                print("wrote %s (%.0f KB)" % (lrc.path(name), os.path.getsize(lrc.path(name)) / 1024))
                break
        else:
            raise SystemExit("no seed of %s met the premises" % name)


if __name__ == "__main__":
    main()
