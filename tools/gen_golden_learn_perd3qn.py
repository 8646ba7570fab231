"""The PERD3QN learning fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Training.  Builds the reference's PERD3QNAgent (ReinLife/Models/PERD3QN.py) under the torch seed of tests/golden/learn_d3qn.npz, scales its
target net by 0.9 and checks that both networks are bit for bit that fixture's init / target_init (DuelingDDQN is the D3QN network, built
in the same order).  brain.buffer is replaced by a stand-in whose sample() replays learn_d3qn.npz's ring and slots (plus the indices and
dummy importance weights -- train() never reads the weights) and whose update_priorities() records its arguments; the reference's OWN
train() (PERD3QN.py:94-115) is called three times.

Memory.  The reference's real PrioritizedReplayBuffer(capacity=8): 5 stores; update_priorities([1, 3], [0.5, 2.0]); 6 more stores (the
ring wraps).  After every event the priorities array is recorded; at the end sample() is called with np.random.choice patched to record
the `p` it is handed.

  tests/golden/learn_perd3qn.npz
    priorities      float32 [3][64]: what train() handed to update_priorities in each of the three calls, |max q'_target(s') - q(s)[a]|
    indices         int64 [3][64]: the indices it handed over with them (= learn_d3qn.npz's slots)
    final           flat float32 parameters of eval_net after the three train() calls
    ref_prio_err    torch's own float32 error of the priorities: max over the three steps of max |p32 - p64| / max(|q|, |q'|), p64 / q / q'
                    from the same step made in float64 on the float32 run's parameters of that step
    buf_prio_trace  float32 [12][8]: the buffer's priorities after each of the 12 events (5 stores, 1 update, 6 stores)
    buf_probs       float64 [8]: the p of np.random.choice in sample() after the last event
    buf_capacity, buf_alpha, buf_stores, buf_update_idx, buf_update_prio   the trace's parameters

    python tools/gen_golden_learn_perd3qn.py
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learn_perd3qn.npz")
D3QN = os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")
SEED, STEPS, BATCH = 21, 3, 64
CAPACITY, STORES, UPDATE_IDX, UPDATE_PRIO = 8, (5, 6), [1, 3], [0.5, 2.0]


def flat(sd):
    return np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.PERD3QN  # noqa: F401  (the module; ReinLife.Models.PERD3QN the attribute is the class)
    mod = sys.modules["ReinLife.Models.PERD3QN"]
    with np.load(D3QN) as z:
        g = {k: z[k] for k in z.files}
    slots = g["slots"]
    assert slots.shape == (STEPS, BATCH)

    torch.manual_seed(SEED)
    brain = mod.PERD3QNAgent()
    with torch.no_grad():
        for p in brain.target_net.parameters():
            p.mul_(0.9)
    init = flat(brain.eval_net.state_dict()).astype(np.float32)
    target_init = flat(brain.target_net.state_dict()).astype(np.float32)
    assert init.tobytes() == g["init"].tobytes() and target_init.tobytes() == g["target_init"].tobytes(), "not learn_d3qn.npz's networks"
    assert brain.batch_size == BATCH and brain.gamma == float(g["gamma"]) and brain.optimizer.param_groups[0]["lr"] == float(g["lr"])

    class Replay:   # buffer.sample(n) -> the recorded minibatches in PrioritizedReplayBuffer.sample's shapes; update_priorities records
        def __init__(self):
            self.calls, self.indices, self.priorities, self.params = 0, [], [], []

        def sample(self, n):
            assert n == BATCH
            idx = slots[self.calls].astype(np.int64)
            self.calls += 1
            self.params.append((copy.deepcopy(brain.eval_net), copy.deepcopy(brain.target_net)))   # this step's pre-update networks
            return (g["ring_state"][idx], tuple(int(a) for a in g["ring_action"][idx]), tuple(float(r) for r in g["ring_reward"][idx]),
                    g["ring_state_prime"][idx], tuple(float(d) for d in g["ring_done"][idx]), idx, np.ones(BATCH, np.float32))

        def update_priorities(self, indices, priorities):
            self.indices.append(np.array(indices, np.int64))
            self.priorities.append(np.array(priorities, np.float32))

    brain.buffer = Replay()
    for _ in range(STEPS):
        brain.train()   # the reference's own update
    assert brain.buffer.calls == STEPS and len(brain.buffer.priorities) == STEPS
    final = flat(brain.eval_net.state_dict()).astype(np.float32)
    assert np.array_equal(flat(brain.target_net.state_dict()).astype(np.float32), target_init)
    priorities, indices = np.stack(brain.buffer.priorities), np.stack(brain.buffer.indices)
    assert np.array_equal(indices, slots.astype(np.int64))

    # torch's own float32 error: the same expression in float64 on the same (float32) parameters of every step
    ref_prio_err = 0.0
    for s, (q_net, t_net) in enumerate(brain.buffer.params):
        idx = slots[s].astype(np.int64)
        q64, t64 = q_net.double(), t_net.double()
        with torch.no_grad():
            q = q64.forward(torch.tensor(g["ring_state"][idx], dtype=torch.float64)).gather(1, torch.tensor(g["ring_action"][idx].astype(np.int64)).unsqueeze(1)).squeeze(1).numpy()
            qn = t64.forward(torch.tensor(g["ring_state_prime"][idx], dtype=torch.float64)).max(1)[0].numpy()
        ref_prio_err = max(ref_prio_err, float(np.abs(priorities[s].astype(np.float64) - np.abs(qn - q)).max() / max(np.abs(q).max(), np.abs(qn).max())))

    # the reference's real memory
    buf = mod.PrioritizedReplayBuffer(capacity=CAPACITY)
    trace = []
    row = lambda i: (np.full(3, i, np.float32), i % 8, float(i), np.full(3, i + 1, np.float32), 0.0)  # noqa: E731
    n = 0
    for _ in range(STORES[0]):
        buf.store(*row(n)); n += 1
        trace.append(buf.priorities.copy())
    buf.update_priorities(UPDATE_IDX, UPDATE_PRIO)
    trace.append(buf.priorities.copy())
    for _ in range(STORES[1]):
        buf.store(*row(n)); n += 1
        trace.append(buf.priorities.copy())
    seen = {}
    real_choice = np.random.choice

    def choice(a, size=None, replace=True, p=None):
        seen["p"] = np.array(p, np.float64)
        return real_choice(a, size, replace, p)
    np.random.choice = choice
    try:
        np.random.seed(SEED)
        buf.sample(4)
    finally:
        np.random.choice = real_choice
    assert len(buf) == CAPACITY and seen["p"].shape == (CAPACITY,)

    out = dict(priorities=priorities, indices=indices, final=final, ref_prio_err=np.float64(ref_prio_err),
               buf_prio_trace=np.stack(trace).astype(np.float32), buf_probs=seen["p"], buf_capacity=np.int64(CAPACITY), buf_alpha=np.float64(buf.alpha),
               buf_stores=np.array(STORES, np.int64), buf_update_idx=np.array(UPDATE_IDX, np.int64), buf_update_prio=np.array(UPDATE_PRIO, np.float32))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB): ref_prio_err %.3g, max priority %.4g, max |final - learn_d3qn.final| %.3g" % (
        OUT, os.path.getsize(OUT) / 1024, ref_prio_err, priorities.max(), np.abs(final - g["final"]).max()))
    print("buf_probs", seen["p"])
    print("buf_prio_trace[-1]", trace[-1])


if __name__ == "__main__":
    main()
