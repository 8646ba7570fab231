"""Shared by tests/test_learn_d3qn_cpu.py and tests/test_hip_learn_d3qn.py: the fixture tests/golden/learn_d3qn.npz and a torch
restatement of the D3QN update (ReinLife/Models/D3QN.py:97-116, 148-165) in any dtype -- with the reference's batch-wide advantage
mean, and with a per-row mean for comparison."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 153), (128,), (128, 128), (128,), (8, 128), (8,), (128, 128), (128,), (1, 128), (1,)]
NAMES = ["fc.weight", "fc.bias", "adv_fc1.weight", "adv_fc1.bias", "adv_fc2.weight", "adv_fc2.bias", "value_fc1.weight", "value_fc1.bias",
         "value_fc2.weight", "value_fc2.bias"]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)
RING_KEYS = ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")) as z:
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


class Dueling(torch.nn.Module):
    """D3QN.py:148-165; row_mean=True takes the advantage mean per row instead (what the reference does NOT do)."""

    def __init__(self, row_mean=False):
        super().__init__()
        self.fc = torch.nn.Linear(153, 128)
        self.adv_fc1 = torch.nn.Linear(128, 128)
        self.adv_fc2 = torch.nn.Linear(128, 8)
        self.value_fc1 = torch.nn.Linear(128, 128)
        self.value_fc2 = torch.nn.Linear(128, 1)
        self.row_mean = row_mean

    def forward(self, x):
        f = torch.relu(self.fc(x))
        adv = self.adv_fc2(torch.relu(self.adv_fc1(f)))
        val = self.value_fc2(torch.relu(self.value_fc1(f)))
        return adv + val - (adv.mean(1, keepdim=True) if self.row_mean else adv.mean())


def net_of(flat, dtype=torch.float64, row_mean=False):
    net = Dueling(row_mean).to(dtype)
    with torch.no_grad():
        for p, v in zip(net.parameters(), split(flat)):
            p.copy_(torch.from_numpy(np.array(v)).to(dtype))
    return net


def flat_of(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])


def q_values(flat, states):
    """float64 Q values of float32 (or float64) parameters on the given rows taken as ONE batch (the mean is the batch's)."""
    with torch.no_grad():
        return net_of(np.asarray(flat, np.float64)).forward(torch.tensor(np.asarray(states), dtype=torch.float64)).numpy()


def td_errors(net, tgt, ring, slots, gamma, dtype):
    idx = np.asarray(slots, np.int64)
    s = torch.tensor(ring["ring_state"][idx], dtype=dtype)
    sp = torch.tensor(ring["ring_state_prime"][idx], dtype=dtype)
    a = torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1)
    r = torch.tensor(ring["ring_reward"][idx], dtype=dtype)
    done = torch.tensor(ring["ring_done"][idx].astype(np.float64), dtype=dtype)
    y = r + gamma * (1 - done) * tgt(sp).max(1)[0].detach()
    return net(s).gather(1, a).squeeze(1) - y


def d3qn_loss(net, tgt, ring, slots, gamma, dtype):
    td = td_errors(net, tgt, ring, slots, gamma, dtype)
    return torch.nn.functional.mse_loss(td, torch.zeros_like(td))


def grads64(flat, target_flat, ring, slots, gamma, row_mean=False, dtype=torch.float64):
    """(loss, the ten gradient tensors) of one minibatch in float64 autograd (dtype=torch.float32: what torch itself makes of it)."""
    net, tgt = net_of(np.asarray(flat, np.float64), dtype, row_mean), net_of(np.asarray(target_flat, np.float64), dtype, row_mean)
    loss = d3qn_loss(net, tgt, ring, slots, gamma, dtype)
    g = torch.autograd.grad(loss, list(net.parameters()))
    return float(loss.detach()), [x.numpy() for x in g]


def torch_steps(g, dtype=torch.float32):
    """D3QN.py:97-116 restated: per recorded minibatch MSE of q[a] against r + gamma (1 - done) max q'_target(s'), one Adam step."""
    net, tgt = net_of(g["init"], dtype), net_of(g["target_init"], dtype)
    opt = torch.optim.Adam(net.parameters(), lr=float(g["lr"]))
    for s in range(g["slots"].shape[0]):
        loss = d3qn_loss(net, tgt, g, g["slots"][s], float(g["gamma"]), dtype)
        opt.zero_grad()
        loss.backward()
        opt.step()
    return flat_of(net)


def adam64(p, m, v, g, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in numpy float64 -> (p, m, v)."""
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


def adam32(p, m, v, g, t, lr):
    """torch.optim.Adam's update made of float32 operations, in numpy, from bias corrections made in double -> (p, m, v): what float32
    itself makes of a step (the kernels' adam_update takes double arithmetic and rounds p, m and v once)."""
    f = np.float32
    p, m, v, g = (np.asarray(x, f) for x in (p, m, v, g))
    w1, w2, b2 = f(1.0 - 0.9), f(1.0 - 0.999), f(0.999)
    bc2, neg = f(np.sqrt(1.0 - 0.999 ** t)), f(-(lr / (1.0 - 0.9 ** t)))
    m2 = m + w1 * (g - m)
    v2 = v * b2 + (w2 * g) * g
    return p + (neg * m2) / (np.sqrt(v2) / bc2 + f(1e-8)), m2, v2


def adam_moments(n, seed=7):
    """Moments of a run that is under way: adam_m ~ N(0, 1e-3), adam_v the squares of another N(0, 1e-3) draw -> (m, v), float32."""
    rng = np.random.RandomState(seed)
    m = rng.normal(0, 1e-3, n).astype(np.float32)
    return m, (rng.normal(0, 1e-3, n) ** 2).astype(np.float32)
