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


def grads64(flat, target_flat, ring, slots, gamma):
    """(loss, the six gradient tensors) of one minibatch in float64 autograd."""
    net, tgt = qnet(np.asarray(flat, np.float64)), qnet(np.asarray(target_flat, np.float64))
    loss = dqn_loss(net, tgt, ring, slots, gamma, torch.float64)
    g = torch.autograd.grad(loss, list(net.parameters()))
    return float(loss.detach()), [x.numpy() for x in g]


def adam64(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in numpy float64 -> (p, m, v)."""
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v
