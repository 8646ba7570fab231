"""The DQN learning fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Builds the reference's DQNAgent (ReinLife/Models/DQN.py) under a fixed torch seed, replaces memory.sample with a replay of recorded
minibatches and calls the reference's OWN train(q, q_target, memory, optimizer) once -- five Adam steps on smooth-L1 (DQN.py:142-153).

  tests/golden/learn_dqn.npz
    init            flat float32 state dict (registration order) before training
    ring_state / ring_state_prime / ring_action / ring_reward / ring_done   a 48-slot replay ring: sparse observation-like rows (every
                    tenth column zero in all rows), rewards from {0, 0.05, 0.3, -1, 5, -10, +-400} (both smooth-L1 branches), 9 of 48 done
    slots           int32 [5][32] ring slots of the five minibatches (slots[0][1] repeats slots[0][0]; slots[0][2:4] are done rows)
    final           flat float32 parameters after train()
    ref_grad_err    torch's own float32 error: max |g32 - g64| / max |g64| over all parameters at step 1 (g64: the same step in float64)
    ref_q_spread    max |Q(final32) - Q(final64)| over the 48 ring states / effect, final64 = the same five steps in float64
    effect          max |Q(final32) - Q(init)| over the 48 ring states (all Q values evaluated in float64)
    lr, gamma       the hyperparameters the reference used (DQN.py:14, 45)

    python tools/gen_golden_learn.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learn_dqn.npz")
SEED, RING, STEPS, BATCH = 20, 48, 5, 32
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
        x[:, 3::10] = 0.0   # columns no row ever uses: their fc1 gradients are exactly zero
        return x
    return {"ring_state": rows(), "ring_state_prime": rows(), "ring_action": rng.randint(0, 8, size=RING).astype(np.int8),
            "ring_reward": rng.choice(REWARDS, size=RING).astype(np.float32), "ring_done": np.isin(np.arange(RING), rng.choice(RING, size=RING // 5, replace=False)).astype(np.uint8)}


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.DQN  # noqa: F401  (the module; ReinLife.Models.DQN the attribute is the class)
    mod = sys.modules["ReinLife.Models.DQN"]
    rng = np.random.RandomState(SEED)
    ring = make_ring(rng)
    slots = rng.randint(0, RING, size=(STEPS, BATCH)).astype(np.int32)
    slots[0, 1] = slots[0, 0]
    slots[0, 2:4] = np.nonzero(ring["ring_done"])[0][:2]   # the first minibatch holds done rows too

    torch.manual_seed(SEED)
    brain = mod.DQNAgent()
    init = flat(brain.agent.state_dict()).astype(np.float32)
    lr = brain.optimizer.param_groups[0]["lr"]

    def batch_of(s, dtype):
        idx = slots[s].astype(np.int64)
        return (torch.tensor(ring["ring_state"][idx], dtype=dtype), torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1),
                torch.tensor(ring["ring_reward"][idx], dtype=dtype).unsqueeze(1), torch.tensor(ring["ring_state_prime"][idx], dtype=dtype),
                torch.tensor(1.0 - ring["ring_done"][idx], dtype=dtype).unsqueeze(1))

    class Replay:   # memory.sample(n) -> the recorded minibatches, in ReplayBuffer.sample's dtypes (DQN.py:111-113)
        calls = 0

        def sample(self, n):
            assert n == BATCH
            b = batch_of(self.calls, torch.float32)
            self.calls += 1
            return b

    # the float32 gradient of step 1, by the reference's modules, before anything changes
    s, a, r, sp, dm = batch_of(0, torch.float32)
    loss = torch.nn.functional.smooth_l1_loss(brain.agent(s).gather(1, a), r + mod.gamma * brain.target(sp).max(1)[0].unsqueeze(1) * dm)
    g32 = np.concatenate([g.numpy().reshape(-1) for g in torch.autograd.grad(loss, list(brain.agent.parameters()))])

    # the same five steps in float64 (copies of the reference's modules)
    import copy
    q64, t64 = copy.deepcopy(brain.agent).double(), copy.deepcopy(brain.target).double()
    opt64 = torch.optim.Adam(q64.parameters(), lr=lr)
    g64 = None
    for step in range(STEPS):
        s, a, r, sp, dm = batch_of(step, torch.float64)
        loss = torch.nn.functional.smooth_l1_loss(q64(s).gather(1, a), r + mod.gamma * t64(sp).max(1)[0].unsqueeze(1) * dm)
        opt64.zero_grad()
        loss.backward()
        if g64 is None:
            g64 = np.concatenate([p.grad.numpy().reshape(-1) for p in q64.parameters()])
        opt64.step()

    memory = Replay()
    mod.train(brain.agent, brain.target, memory, brain.optimizer)   # the reference's own five steps
    assert memory.calls == STEPS
    final = flat(brain.agent.state_dict()).astype(np.float32)

    def q_of(flat_params):
        net = copy.deepcopy(q64)
        off = 0
        with torch.no_grad():
            for t in net.state_dict().values():
                t.copy_(torch.from_numpy(np.asarray(flat_params[off:off + t.numel()], np.float64).reshape(tuple(t.shape))))
                off += t.numel()
            return net(torch.tensor(ring["ring_state"], dtype=torch.float64)).numpy()

    effect = float(np.abs(q_of(final) - q_of(init)).max())
    out = dict(ring)
    out.update(init=init, final=final, slots=slots, lr=np.float64(lr), gamma=np.float64(mod.gamma), effect=np.float64(effect),
               ref_grad_err=np.float64(np.abs(g32 - g64).max() / np.abs(g64).max()),
               ref_q_spread=np.float64(np.abs(q_of(final) - q_of(flat(q64.state_dict()))).max() / effect))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB): ref_grad_err %.3g ref_q_spread %.3g effect %.3g max|final - final64| %.3g" % (
        OUT, os.path.getsize(OUT) / 1024, out["ref_grad_err"], out["ref_q_spread"], effect, np.abs(final - flat(q64.state_dict())).max()))


if __name__ == "__main__":
    main()
