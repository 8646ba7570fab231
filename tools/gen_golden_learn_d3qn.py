"""The D3QN learning fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Builds the reference's D3QNAgent (ReinLife/Models/D3QN.py) under a fixed torch seed, scales its target net by 0.9 (so that target != eval),
replaces buffer.sample with a replay of recorded minibatches and calls the reference's OWN train() three times -- one Adam step on the
MSE loss each (D3QN.py:97-116), with the reference's batch-wide advantage mean (D3QN.py:165).

  tests/golden/learn_d3qn.npz
    init, target_init   flat float32 state dicts (registration order) of eval_net and target_net before training
    ring_state / ring_state_prime / ring_action / ring_reward / ring_done   a 96-slot replay ring: sparse observation-like rows (every
                    tenth column zero in all rows), rewards from {0, 0.05, 0.3, -1, 5, -10, +-400}, a fifth of the rows done
    slots           int32 [3][64] ring slots of the three minibatches (slots[0][1] repeats slots[0][0])
    final           flat float32 parameters of eval_net after the three train() calls
    ref_grad_err    torch's own float32 error: max |g32 - g64| / max |g64| over all parameters at step 1 (g64: the same step in float64)
    ref_q_spread    max |Q(final32) - Q(final64)| over the 96 ring states / effect, final64 = the same three steps in float64
    effect          max |Q(final32) - Q(init)| over the 96 ring states (all Q values evaluated in float64, the 96 rows as one batch)
    lr, gamma       the hyperparameters the reference used (D3QN.py:54-55)

    python tools/gen_golden_learn_d3qn.py
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")
SEED, RING, STEPS, BATCH = 21, 96, 3, 64
REWARDS = np.array([0.0, 0.05, 0.3, -1.0, 5.0, -10.0, 400.0, -400.0], np.float32)


def flat(sd):
    return np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])


def make_ring(rng):
    def rows():
        x = np.zeros((RING, 153), np.float32)
        on = rng.random_sample((RING, 153)) < 0.15
        vals = rng.choice(np.array([1.0, -1.0, 0.5, 0.25], np.float32), size=(RING, 153))
        frac = rng.random_sample((RING, 153)).astype(np.float32)
        x[on] = np.where(rng.random_sample((RING, 153)) < 0.6, vals, frac)[on]
        x[:, 3::10] = 0.0   # columns no row ever uses: their fc gradients are exactly zero
        return x
    return {"ring_state": rows(), "ring_state_prime": rows(), "ring_action": rng.randint(0, 8, size=RING).astype(np.int8),
            "ring_reward": rng.choice(REWARDS, size=RING).astype(np.float32), "ring_done": np.isin(np.arange(RING), rng.choice(RING, size=RING // 5, replace=False)).astype(np.uint8)}


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.D3QN  # noqa: F401  (the module; ReinLife.Models.D3QN the attribute is the class)
    mod = sys.modules["ReinLife.Models.D3QN"]
    rng = np.random.RandomState(SEED)
    ring = make_ring(rng)
    slots = rng.randint(0, RING, size=(STEPS, BATCH)).astype(np.int32)
    slots[0, 1] = slots[0, 0]

    torch.manual_seed(SEED)
    brain = mod.D3QNAgent()
    with torch.no_grad():
        for p in brain.target_net.parameters():
            p.mul_(0.9)
    init = flat(brain.eval_net.state_dict()).astype(np.float32)
    target_init = flat(brain.target_net.state_dict()).astype(np.float32)
    lr, gamma = brain.optimizer.param_groups[0]["lr"], brain.gamma
    assert brain.batch_size == BATCH

    class Replay:   # buffer.sample(n) -> the recorded minibatches, in replay_buffer.sample's shapes (D3QN.py:139-142)
        calls = 0

        def sample(self, n):
            assert n == BATCH
            idx = slots[self.calls].astype(np.int64)
            self.calls += 1
            return (ring["ring_state"][idx], tuple(int(a) for a in ring["ring_action"][idx]), tuple(float(r) for r in ring["ring_reward"][idx]),
                    ring["ring_state_prime"][idx], tuple(float(d) for d in ring["ring_done"][idx]))

    def loss_of(net, tgt, step, dtype):
        idx = slots[step].astype(np.int64)
        s, sp = torch.tensor(ring["ring_state"][idx], dtype=dtype), torch.tensor(ring["ring_state_prime"][idx], dtype=dtype)
        a = torch.tensor(ring["ring_action"][idx].astype(np.int64))
        r, d = torch.tensor(ring["ring_reward"][idx], dtype=dtype), torch.tensor(ring["ring_done"][idx].astype(np.float64), dtype=dtype)
        q = net.forward(s).gather(1, a.unsqueeze(1)).squeeze(1)
        return torch.nn.functional.mse_loss(q, r + gamma * (1 - d) * tgt.forward(sp).max(1)[0].detach())

    # the float32 gradient of step 1, by the reference's modules, before anything changes
    g32 = np.concatenate([g.numpy().reshape(-1) for g in torch.autograd.grad(loss_of(brain.eval_net, brain.target_net, 0, torch.float32), list(brain.eval_net.parameters()))])

    # the same three steps in float64 (copies of the reference's modules)
    q64, t64 = copy.deepcopy(brain.eval_net).double(), copy.deepcopy(brain.target_net).double()
    opt64 = torch.optim.Adam(q64.parameters(), lr=lr)
    g64 = None
    for step in range(STEPS):
        loss = loss_of(q64, t64, step, torch.float64)
        opt64.zero_grad()
        loss.backward()
        if g64 is None:
            g64 = np.concatenate([p.grad.numpy().reshape(-1) for p in q64.parameters()])
        opt64.step()

    brain.buffer = Replay()
    for _ in range(STEPS):
        brain.train()   # the reference's own update
    assert brain.buffer.calls == STEPS
    final = flat(brain.eval_net.state_dict()).astype(np.float32)
    assert np.array_equal(flat(brain.target_net.state_dict()).astype(np.float32), target_init)

    def q_of(flat_params):
        net = copy.deepcopy(q64)
        off = 0
        with torch.no_grad():
            for t in net.state_dict().values():
                t.copy_(torch.from_numpy(np.asarray(flat_params[off:off + t.numel()], np.float64).reshape(tuple(t.shape))))
                off += t.numel()
            return net.forward(torch.tensor(ring["ring_state"], dtype=torch.float64)).numpy()

    effect = float(np.abs(q_of(final) - q_of(init)).max())
    out = dict(ring)
    out.update(init=init, target_init=target_init, final=final, slots=slots, lr=np.float64(lr), gamma=np.float64(gamma), effect=np.float64(effect),
               ref_grad_err=np.float64(np.abs(g32 - g64).max() / np.abs(g64).max()),
               ref_q_spread=np.float64(np.abs(q_of(final) - q_of(flat(q64.state_dict()))).max() / effect))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB): ref_grad_err %.3g ref_q_spread %.3g effect %.3g max|final - final64| %.3g" % (
        OUT, os.path.getsize(OUT) / 1024, out["ref_grad_err"], out["ref_q_spread"], effect, np.abs(final - flat(q64.state_dict())).max()))


if __name__ == "__main__":
    main()
