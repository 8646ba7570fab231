"""The PERDQN learning fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Training.  Builds the reference's PERDQNAgent (ReinLife/Models/PERDQN.py) under a fixed torch seed with a memory of 96 rows and scales its
target net by 0.9.  The memory is a subclass of the reference's real Memory: the 96 ring rows of tests/golden/learn_d3qn.npz are stored
through the agent's OWN append_sample (every leaf then holds (0 + e) ** a: the view quirk), a third of the rows is then given another
priority through the real update(), so that the importance weights of the first call are unequal.  Its sample() feeds the real
Memory.sample the uniforms that make it visit the slots of a recorded table (three tables, the first with a duplicated slot) -- the
is_weight values, beta and the batch are therefore the REAL sample()'s; its update() records what it is handed and passes it on to the
real one.  The reference's own train_model() is called three times.
  numpy: train_model's np.array(mini_batch) is ragged and raises under numpy >= 1.24.  The module is handed an `np` stand-in whose
  array() retries with dtype=object -- what numpy < 1.24 did with a warning.  Everything else of numpy is the installed one (2.x: the
  priorities (|error| + e) ** a of float32 errors are float32 arithmetic).

Memory.  A second PERDQNAgent(capacity=8): 5 append_sample calls, two update()s, 6 more append_sample calls (the ring wraps); the leaf
priorities after every event.  Then three sample(4) calls of the real Memory under a fixed seed: the drawn rows' priorities, is_weight, beta.

  tests/golden/learn_perdqn.npz
    init, target_init   flat float32 state dicts (fc.0.w fc.0.b fc.2.w fc.2.b fc.4.w fc.4.b) of model and target_model before training
    final               flat float32 parameters of model after the three train_model() calls
    slots               int32 [3][64] ring slots of the three minibatches (slots[0][1] repeats slots[0][0])
    prio_init           float32 [96] the leaves before the first call
    errors, priorities  float32 [3][64]: what train_model handed to update() in each call, and the leaf each batch row held afterwards
    is_weights          float64 [3][64] as Memory.sample returned them;  beta float64 [3] after each sample()
    epsilon             float64 [4]: before the first call and after each call;  epsilon_decay, epsilon_min
    p_new, prio_e, prio_a, beta0, beta_increment, lr, gamma
    ref_grad_err        torch's own float32 error: max |g32 - g64| / max |g64| over all parameters at step 1 (g64: the same step in float64)
    ref_q_spread        max |Q(final32) - Q(final64)| over the 96 ring states / effect, final64 = the same three steps in float64
    effect              max |Q(final32) - Q(init)| over the 96 ring states (all Q values evaluated in float64)
    mem_trace           float32 [13][8]: the leaves of the capacity-8 memory after each of the 13 events
    mem_update_idx, mem_update_err, mem_stores      the trace's parameters
    mem_sample_prio, mem_is_weight  float64 [3][4];  mem_beta float64 [3]

    python tools/gen_golden_learn_perdqn.py
"""
import copy
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learn_perdqn.npz")
D3QN = os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")
SEED, RING, STEPS, BATCH = 21, 96, 3, 64
CAPACITY, STORES, UPDATE_IDX, UPDATE_ERR = 8, (5, 6), [1, 3], [0.5, 2.0]


def flat(sd):
    return np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])


class NpCompat:
    """numpy, with array() retrying a ragged input as dtype=object (numpy < 1.24's behaviour)."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *a, **k):
        try:
            return np.array(obj, *a, **k)
        except ValueError:
            return np.array(obj, *a, dtype=object, **k)


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.PERDQN  # noqa: F401  (the module; ReinLife.Models.PERDQN the attribute may be the class)
    mod = sys.modules["ReinLife.Models.PERDQN"]
    mod.np = NpCompat()
    real_random = mod.random
    with np.load(D3QN) as z:
        g = {k: z[k] for k in z.files}
    slots = g["slots"]
    assert slots.shape == (STEPS, BATCH) and slots[0, 1] == slots[0, 0] and g["ring_state"].shape[0] == RING

    queue = []   # the uniforms the next Memory.sample is to draw

    class Memory(mod.Memory):
        def __init__(self, capacity):
            super().__init__(capacity)
            self.calls, self.errors, self.idxs, self.is_weights, self.betas = 0, [], [], [], []

        def leaf_point(self, slot):
            """A point of the tree's [0, total) that SumTree.get maps to `slot`: the middle of its leaf's interval."""
            t = self.tree.tree
            node = slot + self.capacity - 1
            s = t[node] / 2
            while node != 0:
                parent = (node - 1) // 2
                if node == 2 * parent + 2:
                    s += t[2 * parent + 1]
                node = parent
            return s

        def sample(self, n):
            assert n == BATCH
            queue[:] = [self.leaf_point(int(s)) for s in slots[self.calls]]
            self.calls += 1
            self.errors.append({})
            batch, idxs, w = super().sample(n)   # the real sample(): the real is_weight and beta
            assert not queue and [i - self.capacity + 1 for i in idxs] == [int(s) for s in slots[self.calls - 1]]
            self.idxs.append(np.array(idxs, np.int64)); self.is_weights.append(np.array(w, np.float64)); self.betas.append(float(self.beta))
            return batch, idxs, w

        def update(self, idx, error):
            if self.errors:
                self.errors[-1][int(idx)] = error
            super().update(idx, error)

        def leaves(self):
            return self.tree.tree[self.capacity - 1:].copy()

    mod.random = types.SimpleNamespace(uniform=lambda a, b: queue.pop(0))
    try:
        torch.manual_seed(SEED)
        brain = mod.PERDQNAgent(capacity=RING)
        with torch.no_grad():
            for p in brain.target_model.parameters():
                p.mul_(0.9)
        init = flat(brain.model.state_dict()).astype(np.float32)
        target_init = flat(brain.target_model.state_dict()).astype(np.float32)
        lr, gamma = brain.optimizer.param_groups[0]["lr"], brain.discount_factor
        assert brain.batch_size == BATCH and init.size == 14536
        brain.memory = Memory(RING)
        for i in range(RING):   # the agent's own append_sample
            brain.append_sample(g["ring_state"][i], int(g["ring_action"][i]), float(g["ring_reward"][i]), g["ring_state_prime"][i], bool(g["ring_done"][i]))
        p_new = brain.memory.leaves()
        assert len(set(p_new.tolist())) == 1, "append_sample no longer gives every row one priority"
        p_new = np.float32(p_new[0])
        assert float(p_new) == float((torch.zeros(()) + brain.memory.e) ** brain.memory.a)
        rng = np.random.RandomState(SEED)
        for i in range(0, RING, 3):   # unequal priorities: every third row through the real update()
            brain.memory.update(i + RING - 1, np.float32(rng.choice([0.02, 0.3, 1.5, 7.0, 40.0]) * rng.random_sample()))
        prio_init = brain.memory.leaves().astype(np.float32)
        assert np.array_equal(prio_init.astype(np.float64), brain.memory.leaves())
        q0, t0 = copy.deepcopy(brain.model), copy.deepcopy(brain.target_model)

        epsilon = [brain.epsilon]
        prios = []
        for s in range(STEPS):
            brain.train_model()   # the reference's own update
            epsilon.append(brain.epsilon)
            prios.append(brain.memory.leaves()[slots[s].astype(np.int64)].astype(np.float32))
        mem = brain.memory
        assert mem.calls == STEPS
        errors = np.stack([np.array([mem.errors[s][int(i)] for i in mem.idxs[s]], np.float32) for s in range(STEPS)])
        assert all(type(v) is np.float32 for v in mem.errors[0].values())
        final = flat(brain.model.state_dict()).astype(np.float32)
        assert np.array_equal(flat(brain.target_model.state_dict()).astype(np.float32), target_init)
    finally:
        mod.random = real_random
    is_weights = np.stack(mem.is_weights)

    def loss_of(net, tgt, step, dtype):
        idx = slots[step].astype(np.int64)
        s, sp = torch.tensor(g["ring_state"][idx], dtype=dtype), torch.tensor(g["ring_state_prime"][idx], dtype=dtype)
        a = torch.tensor(g["ring_action"][idx].astype(np.int64))
        r, d = torch.tensor(g["ring_reward"][idx], dtype=dtype), torch.tensor(g["ring_done"][idx].astype(np.float64), dtype=dtype)
        q = net.forward(s).gather(1, a.unsqueeze(1)).squeeze(1)
        w = torch.tensor(is_weights[step], dtype=dtype)
        return (w * torch.nn.functional.mse_loss(q, r + (1 - d) * gamma * tgt.forward(sp).max(1)[0].detach())).mean()

    g32 = np.concatenate([x.numpy().reshape(-1) for x in torch.autograd.grad(loss_of(q0, t0, 0, torch.float32), list(q0.parameters()))])
    q64, t64 = copy.deepcopy(q0).double(), copy.deepcopy(t0).double()
    opt64 = torch.optim.Adam(q64.parameters(), lr=lr)
    g64 = None
    for step in range(STEPS):
        loss = loss_of(q64, t64, step, torch.float64)
        opt64.zero_grad()
        loss.backward()
        if g64 is None:
            g64 = np.concatenate([p.grad.numpy().reshape(-1) for p in q64.parameters()])
        opt64.step()

    def q_of(flat_params):
        net = copy.deepcopy(q64)
        off = 0
        with torch.no_grad():
            for t in net.state_dict().values():
                t.copy_(torch.from_numpy(np.asarray(flat_params[off:off + t.numel()], np.float64).reshape(tuple(t.shape))))
                off += t.numel()
            return net.forward(torch.tensor(g["ring_state"], dtype=torch.float64)).numpy()

    effect = float(np.abs(q_of(final) - q_of(init)).max())

    # the reference's real memory, fed by the reference's own append_sample
    torch.manual_seed(SEED)
    small = mod.PERDQNAgent(capacity=CAPACITY)
    leaves = lambda: small.memory.tree.tree[CAPACITY - 1:].copy()  # noqa: E731
    trace = []
    rs = np.random.RandomState(SEED + 1)
    n = 0

    def store():
        small.append_sample(rs.random_sample(153).astype(np.float32), int(rs.randint(8)), float(rs.choice([0.0, 5.0, -10.0, 400.0])),
                            rs.random_sample(153).astype(np.float32), bool(rs.randint(2)))
        trace.append(leaves())
    for _ in range(STORES[0]):
        store(); n += 1
    for i, e in zip(UPDATE_IDX, UPDATE_ERR):
        small.memory.update(i + CAPACITY - 1, np.float32(e))
        trace.append(leaves())
    for _ in range(STORES[1]):
        store(); n += 1
    real_random.seed(SEED)
    mem_prio, mem_w, mem_beta = [], [], []
    for _ in range(3):
        _, idxs, w = small.memory.sample(4)
        mem_prio.append(small.memory.tree.tree[np.array(idxs)].copy()); mem_w.append(np.array(w, np.float64)); mem_beta.append(float(small.memory.beta))

    out = dict(init=init, target_init=target_init, final=final, slots=slots, prio_init=prio_init, errors=errors, priorities=np.stack(prios),
               is_weights=is_weights, beta=np.array(mem.betas, np.float64), epsilon=np.array(epsilon, np.float64),
               epsilon_decay=np.float64(brain.epsilon_decay), epsilon_min=np.float64(brain.epsilon_min),
               p_new=p_new, prio_e=np.float64(mod.Memory.e), prio_a=np.float64(mod.Memory.a), beta0=np.float64(mod.Memory.beta),
               beta_increment=np.float64(mod.Memory.beta_increment_per_sampling), lr=np.float64(lr), gamma=np.float64(gamma),
               effect=np.float64(effect), ref_grad_err=np.float64(np.abs(g32 - g64).max() / np.abs(g64).max()),
               ref_q_spread=np.float64(np.abs(q_of(final) - q_of(flat(q64.state_dict()))).max() / effect),
               mem_trace=np.stack(trace).astype(np.float32), mem_update_idx=np.array(UPDATE_IDX, np.int64), mem_update_err=np.array(UPDATE_ERR, np.float32),
               mem_stores=np.array(STORES, np.int64), mem_sample_prio=np.stack(mem_prio), mem_is_weight=np.stack(mem_w), mem_beta=np.array(mem_beta, np.float64))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB): ref_grad_err %.3g ref_q_spread %.3g effect %.3g p_new %.9g mean(w) %s" % (
        OUT, os.path.getsize(OUT) / 1024, out["ref_grad_err"], out["ref_q_spread"], effect, p_new, is_weights.mean(1)))
    print("beta", mem.betas, "epsilon", epsilon)
    print("mem_trace[-1]", trace[-1], "mem_is_weight[0]", mem_w[0])


if __name__ == "__main__":
    main()
