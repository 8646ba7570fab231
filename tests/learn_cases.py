"""Shared by tests/test_learn_cpu.py and tests/test_hip_learn.py: the fixture tests/golden/learn_dqn.npz and a torch restatement of the
DQN update (ReinLife/Models/DQN.py:126-130, 142-153) in any dtype."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 153), (128,), (64, 128), (64,), (8, 64), (8,)]   # fc1.w fc1.b fc2.w fc2.b fc3.w fc3.b
NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_dqn.npz")) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def split(flat):
    out, off = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(np.asarray(flat[off:off + n]).reshape(s))
        off += n
    return out


def qnet(flat, dtype=torch.float64):
    net = torch.nn.Sequential(torch.nn.Linear(153, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8)).to(dtype)
    with torch.no_grad():
        for p, v in zip(net.parameters(), split(flat)):
            p.copy_(torch.from_numpy(np.array(v)).to(dtype))
    return net


def flat_of(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])


def q_values(flat, states):
    """float64 Q values of float32 (or float64) parameters on the given rows."""
    with torch.no_grad():
        return qnet(np.asarray(flat, np.float64)).forward(torch.tensor(np.asarray(states), dtype=torch.float64)).numpy()


def td_errors(net, tgt, ring, slots, gamma, dtype):
    idx = np.asarray(slots, np.int64)
    s = torch.tensor(ring["ring_state"][idx], dtype=dtype)
    sp = torch.tensor(ring["ring_state_prime"][idx], dtype=dtype)
    a = torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1)
    r = torch.tensor(ring["ring_reward"][idx], dtype=dtype).unsqueeze(1)
    mask = torch.tensor(1.0 - ring["ring_done"][idx].astype(np.float64), dtype=dtype).unsqueeze(1)
    target = r + gamma * tgt(sp).max(1)[0].unsqueeze(1).detach() * mask
    return net(s).gather(1, a) - target


def dqn_loss(net, tgt, ring, slots, gamma, dtype):
    td = td_errors(net, tgt, ring, slots, gamma, dtype)
    return torch.nn.functional.smooth_l1_loss(td, torch.zeros_like(td))


def grads64(flat, target_flat, ring, slots, gamma, dtype=torch.float64):
    """(loss, the six gradient tensors) of one minibatch in float64 autograd (dtype=torch.float32: what torch itself makes of it)."""
    net, tgt = qnet(np.asarray(flat, np.float64), dtype), qnet(np.asarray(target_flat, np.float64), dtype)
    loss = dqn_loss(net, tgt, ring, slots, gamma, dtype)
    g = torch.autograd.grad(loss, list(net.parameters()))
    return float(loss.detach()), [x.numpy() for x in g]


def adam64(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in numpy float64 -> (p, m, v)."""
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


# ---- inputs beyond the fixtures (tests/test_learn_edges_cpu.py, tests/test_hip_learn_edges.py) ----
RING_KEYS = ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")
TARGET_SCALE = np.float32(0.96875)   # trained eval weights times this are the target network of the trained-weight cases: q' differs from q
_pretrained = None
_edge_rows = {}


def pretrained(method):
    """The reference's trained weights of `method` ("DQN", "D3QN", "PERD3QN"; tests/golden/pretrained.npz) as the eval network, and the
    same weights times float32(0.96875) as the target -> (eval, target), flat float32."""
    global _pretrained
    if _pretrained is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "pretrained.npz")) as z:
            _pretrained = {k: z[k] for k in z.files if k.endswith("_weights")}
        for v in _pretrained.values():
            v.setflags(write=False)
    w = _pretrained[method + "_weights"]
    return w, (w * TARGET_SCALE).astype(np.float32)


def edge_ring_rows(n, seed=11):
    """n seeded ring rows as the worlds write them: observation planes from {0, +-0.5, +-1} (about 15 % non-zero), actions 0..7, rewards
    from {0, 0.05, 0.3, -1, 5, -10, 400}, about 20 % done, and ages 0..199 ("ring_age", int32).  Generated once per (n, seed), read-only."""
    if (n, seed) not in _edge_rows:
        rng = np.random.RandomState(seed)

        def rows():
            x = (rng.random_sample((n, 153)) < 0.15) * rng.choice(np.array([1.0, -1.0, 0.5, -0.5], np.float32), size=(n, 153))
            return x.astype(np.float32)
        r = {"ring_state": rows(), "ring_state_prime": rows(), "ring_action": rng.randint(0, 8, size=n).astype(np.int8),
             "ring_reward": rng.choice(np.array([0, 0.05, 0.3, -1, 5, -10, 400], np.float32), size=n),
             "ring_done": (rng.random_sample(n) < 0.2).astype(np.uint8), "ring_age": rng.randint(0, 200, size=n).astype(np.int32)}
        for v in r.values():
            v.setflags(write=False)
        _edge_rows[(n, seed)] = r
    return _edge_rows[(n, seed)]


def relocated(rows, capacity, at):
    """A ring of `capacity` rows, all zero but for `rows` at slots at .. at + len(rows) - 1."""
    n = rows["ring_state"].shape[0]
    assert 0 <= at and at + n <= capacity
    out = {}
    for k in RING_KEYS:
        a = np.zeros((capacity,) + rows[k].shape[1:], rows[k].dtype)
        a[at:at + n] = rows[k]
        out[k] = a
    return out
