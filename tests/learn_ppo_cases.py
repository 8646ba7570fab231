"""Shared by tests/test_learn_ppo_cpu.py and tests/test_hip_learn_ppo.py: the fixture tests/golden/learn_ppo.npz (with the ring of
learn_d3qn.npz and the initial parameters of models.npz it builds on), a torch restatement of PPO.learn() (ReinLife/Models/PPO.py:136-162)
for autograd in any dtype, a HAND-WRITTEN float64 model of the same update -- the gradients at the kinks of min() and clamp() spelled out,
no autograd -- and a host model of rl_learn_rollout's window bookkeeping."""
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 153), (256,), (256, 256), (256,), (8, 256), (8,), (1, 256), (1,)]
NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc_pi.weight", "fc_pi.bias", "fc_v.weight", "fc_v.bias"]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)
LR, GAMMA, LMBDA, EPS_CLIP, K_EPOCH = 0.0005, 0.98, 0.95, 0.1, 3   # PPO.py:42-43
_golden = None


def golden():
    """learn_ppo.npz, plus ring_* of learn_d3qn.npz and init = PPO_weights of models.npz (stored once, there)."""
    global _golden
    if _golden is None:
        g = {}
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")) as z:
            g.update({k: z[k] for k in z.files if k.startswith("ring_")})
        with np.load(os.path.join(ROOT, "tests", "golden", "models.npz")) as z:
            g["init"] = z["PPO_weights"]
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_ppo.npz")) as z:
            g.update({k: z[k] for k in z.files})
        g["ring_reward"] = (g["ring_reward"] * g["reward_scale"]).astype(np.float32)
        for v in g.values():
            v.setflags(write=False)
        _golden = g
    return _golden


def rollouts(g):
    """The fixture's three slot lists (32, 17 and 1 rows)."""
    return [g["slots"][i][:int(n)].astype(np.int32) for i, n in enumerate(g["rows"])]


def split(flat):
    out, off = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(np.asarray(flat[off:off + n]).reshape(s))
        off += n
    return out


class Net(torch.nn.Module):   # PPO.py:95-112
    def __init__(self):
        super().__init__()
        self.fc1 = torch.nn.Linear(153, 256)
        self.fc2 = torch.nn.Linear(256, 256)
        self.fc_pi = torch.nn.Linear(256, 8)
        self.fc_v = torch.nn.Linear(256, 1)

    def trunk(self, x):
        return torch.relu(self.fc2(torch.relu(self.fc1(x))))

    def pi(self, x):
        return torch.softmax(self.fc_pi(self.trunk(x)), dim=1)

    def v(self, x):
        return self.fc_v(self.trunk(x))


def net_of(flat, dtype=torch.float64):
    net = Net().to(dtype)
    with torch.no_grad():
        for p, v in zip(net.parameters(), split(flat)):
            p.copy_(torch.from_numpy(np.array(v)).to(dtype))
    return net


def flat_of(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])


def outputs(flat, states):
    """float64 [rows][9]: the eight probabilities and the value of float32 (or float64) parameters on the given rows."""
    with torch.no_grad():
        net, x = net_of(np.asarray(flat, np.float64)), torch.tensor(np.asarray(states), dtype=torch.float64)
        return torch.cat([net.pi(x), net.v(x)], dim=1).numpy()


def rows_of(ring, prob, slots, dtype=torch.float64):
    """What make_batch (PPO.py:117-134) hands learn(): s, a, r = reward / 100 (in double, then float32: the list holds Python floats and
    torch.tensor makes float32 of them), s', done_mask, prob_a."""
    idx = np.asarray(slots, np.int64)
    r = np.array([float(x) / 100.0 for x in ring["ring_reward"][idx]], np.float64).astype(np.float32)
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype).unsqueeze(1)  # noqa: E731
    return dict(s=torch.tensor(ring["ring_state"][idx], dtype=dtype), sp=torch.tensor(ring["ring_state_prime"][idx], dtype=dtype),
                a=torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1), r=t(r), mask=t(1.0 - ring["ring_done"][idx]),
                prob=t(np.asarray(prob)[idx]))


def gae32(delta, gamma=GAMMA, lmbda=LMBDA):
    """PPO.py:144-150 as numpy 2 makes it: delta is float32, the Python double gamma * lmbda becomes ONE float32, and every step is one
    float32 multiply and one float32 add, backwards, with no reset at done."""
    gl = np.float32(gamma * lmbda)
    adv, out = np.float32(0.0), np.zeros(len(delta), np.float32)
    for t in range(len(delta) - 1, -1, -1):
        adv = np.float32(np.float32(gl * adv) + np.float32(delta[t]))
        out[t] = adv
    return out


def ppo_loss(net, rows, dtype, gamma=GAMMA, lmbda=LMBDA, eps_clip=EPS_CLIP):
    """PPO.py:140-158 restated with torch operations, for autograd -> (loss, dict of the intermediate values)."""
    td = rows["r"] + gamma * net.v(rows["sp"]) * rows["mask"]
    v = net.v(rows["s"])
    delta = (td - v).detach()
    adv = torch.tensor(gae32(delta.numpy()[:, 0].astype(np.float32), gamma, lmbda).astype(np.float64), dtype=dtype).unsqueeze(1)
    pi_a = net.pi(rows["s"]).gather(1, rows["a"])
    ratio = torch.exp(torch.log(pi_a) - torch.log(rows["prob"]))
    surr1, surr2 = ratio * adv, torch.clamp(ratio, 1 - eps_clip, 1 + eps_clip) * adv
    loss = (-torch.min(surr1, surr2) + torch.nn.functional.smooth_l1_loss(v, td.detach())).mean()
    return loss, dict(td=td.detach(), v=v.detach(), delta=delta, adv=adv, ratio=ratio.detach())


def grads_autograd(flat, rows, dtype=torch.float64, **hyper):
    """(loss, the eight gradient tensors, intermediates) of one epoch by torch autograd."""
    net = net_of(np.asarray(flat, np.float64), dtype)
    loss, mid = ppo_loss(net, rows, dtype, **hyper)
    g = torch.autograd.grad(loss, list(net.parameters()))
    return float(loss.detach()), [x.numpy() for x in g], {k: v.numpy()[:, 0] for k, v in mid.items()}


def grads_by_hand(flat, rows, gamma=GAMMA, lmbda=LMBDA, eps_clip=EPS_CLIP):
    """The same epoch in float64 WITHOUT autograd: the forward pass as matrix products, then
        dL/dv_i     = clamp(v_i - td_i, -1, 1) / T                       (smooth-L1, beta 1; nothing through td or the advantage)
        dL/dratio_i = -(adv_i / T) ([s1 < s2] + 1/2 [s1 == s2] + in_i ([s2 < s1] + 1/2 [s1 == s2])),  in_i = [1 - eps <= ratio_i <= 1 + eps]
                      (min: the smaller side takes it all, each side half at a tie; clamp: passes on the closed interval)
        dL/dlogit_ij = dL/dratio_i ratio_i ([j == a_i] - pi_ij)
    and the chain rule through the layers -> (loss, the eight gradient tensors, intermediates)."""
    W1, b1, W2, b2, Wp, bp, Wv, bv = [torch.tensor(np.asarray(x, np.float64)) for x in split(np.asarray(flat, np.float64))]

    def trunk(x):
        h1 = torch.relu(x @ W1.T + b1)
        return h1, torch.relu(h1 @ W2.T + b2)
    s, sp, a = rows["s"].double(), rows["sp"].double(), rows["a"]
    T = s.shape[0]
    vp = trunk(sp)[1] @ Wv.T + bv
    h1, h2 = trunk(s)
    v = h2 @ Wv.T + bv
    pi = torch.softmax(h2 @ Wp.T + bp, dim=1)
    td = rows["r"].double() + gamma * vp * rows["mask"].double()
    delta = td - v
    adv = torch.tensor(gae32(delta.numpy()[:, 0].astype(np.float32), gamma, lmbda).astype(np.float64)).unsqueeze(1)
    ratio = torch.exp(torch.log(pi.gather(1, a)) - torch.log(rows["prob"].double()))
    lo, hi = 1 - eps_clip, 1 + eps_clip
    s1, s2 = ratio * adv, torch.clamp(ratio, lo, hi) * adv
    d = v - td
    huber = torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)
    loss = float((-torch.min(s1, s2)).mean() + huber.mean())
    inside = ((ratio >= lo) & (ratio <= hi)).double()
    tie = (s1 == s2).double()
    coef = (s1 < s2).double() + 0.5 * tie + inside * ((s2 < s1).double() + 0.5 * tie)
    g_ratio = -(adv / T) * coef
    onehot = torch.zeros_like(pi).scatter_(1, a, 1.0)
    d_logit = g_ratio * ratio * (onehot - pi)
    d_v = torch.clamp(d, -1, 1) / T
    d2 = (d_logit @ Wp + d_v @ Wv) * (h2 > 0).double()
    d1 = (d2 @ W2) * (h1 > 0).double()
    grads = [d1.T @ s, d1.sum(0), d2.T @ h1, d2.sum(0), d_logit.T @ h2, d_logit.sum(0), d_v.T @ h2, d_v.sum(0)]
    mid = dict(td=td, v=v, delta=delta, adv=adv, ratio=ratio, coef=coef)
    return loss, [x.numpy() for x in grads], {k: x.numpy()[:, 0] for k, x in mid.items()}


def adam64(p, m, v, g, t, lr=LR, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in numpy float64 -> (p, m, v)."""
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * m / denom, m, v


def learn_by_hand(flat, ring, prob, slot_lists, k_epoch=K_EPOCH, lr=LR, **hyper):
    """PPO.learn() on each slot list in turn, in float64 from grads_by_hand and adam64 -> the final flat parameters (float64)."""
    p = np.asarray(flat, np.float64).copy()
    m, v, t = np.zeros_like(p), np.zeros_like(p), 0
    for slots in slot_lists:
        rows = rows_of(ring, prob, slots)
        for _ in range(k_epoch):
            _, grads, _ = grads_by_hand(p, rows, **hyper)
            t += 1
            p, m, v = adam64(p, m, v, np.concatenate([x.reshape(-1) for x in grads]), t, lr)
    return p


# ---- rl_learn_rollout's window (include/reinlife_hip.h) ----
def window_slots(seen, count, capacity):
    """The slots of the rows appended since `seen`: [seen, count) mod capacity, or the whole ring once count - seen >= capacity."""
    fresh = min(max(count - seen, 0), capacity)
    return [(count - fresh + j) % capacity for j in range(fresh)]


def mix64(z):   # splitmix64's finalizer (rl_learn_dev.h: learn_mix64)
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def row_key(ring, row, age=0):
    """The content key of a ring row (rl_learn_dev.h: learn_row_key): a sum mod 2^64 of mixed (position, bits) terms."""
    M = (1 << 64) - 1
    term = lambda pos, bits: mix64(((pos + 1) << 32) | int(bits))  # noqa: E731
    k = 0
    for f, b in enumerate(np.asarray(ring["ring_state"][row], np.float32).view(np.uint32)):
        k += term(f, b)
    for f, b in enumerate(np.asarray(ring["ring_state_prime"][row], np.float32).view(np.uint32)):
        k += term(153 + f, b)
    k += term(306, int(ring["ring_action"][row]) & 0xff) + term(307, np.float32(ring["ring_reward"][row]).view(np.uint32))
    k += term(308, int(ring["ring_done"][row])) + term(309, int(age) & 0xffffffff)
    return k & M


def rollout_draw(keys_by_slot, window, salt):
    """One draw: the window slot whose mixed key is smallest (ties: the lower slot); slot 0 from an empty window."""
    if not window:
        return 0
    return min(window, key=lambda i: (mix64(keys_by_slot[i] ^ salt), i))


def rollout_table(keys, window, seed, brain, calls, n_draws):
    """rollout_draw for every draw of a call at once, in numpy's integers: draw d takes the window slot with the smallest
    (mix64(key ^ salt_d), slot), salt_d = words 0-1 of rl_philox(seed, 0, brain, calls, RL_SITE_LEARN_ROLLOUT, d); slot 0 from an empty
    window -> int64 [n_draws].  keys: uint64 by slot."""
    from reinlife_amd import _lib
    import learn_perd3qn_cases as prio
    if not len(window):
        return np.zeros(n_draws, np.int64)
    window = np.asarray(window, np.int64)
    k = np.asarray(keys, np.uint64)[window]
    out = np.zeros(n_draws, np.int64)
    for d, salt in enumerate(prio._salts(seed, brain, calls, _lib.SITE_LEARN_ROLLOUT, n_draws)):
        out[d] = window[np.lexsort((window, prio._mix64(k ^ salt)))[0]]
    return out


# ---- inputs beyond the fixture (tests/test_learn_late_edges_cpu.py, tests/test_hip_learn_ppo_edges.py) ----
EDGE_FACTORS = np.array([1, 0.8, 1.25, 0.95, 1.05, 0.5, 2], np.float64)
EDGE_ROLLOUT_ROWS = (32, 31, 17, 1)
_edge = None


def edge_case():
    """One epoch on the reference's TRAINED weights: (PPO_weights of tests/golden/pretrained.npz, learn_cases.edge_ring_rows(1027), the
    prob column float32(pi64(s)[a] / factor) with factor drawn by RandomState(5) from EDGE_FACTORS, the rollouts of 32, 31, 17 and 1
    rows RandomState(1..4).randint(0, 1027, n)).  Made once, read-only."""
    global _edge
    if _edge is None:
        import learn_cases as lc
        w = lc.pretrained("PPO")[0]
        rows = lc.edge_ring_rows(1027)
        factor = np.random.RandomState(5).choice(EDGE_FACTORS, size=1027)
        pi = outputs(w, rows["ring_state"])[np.arange(1027), rows["ring_action"].astype(np.int64)]
        prob = (pi / factor).astype(np.float32)
        rollouts = [np.random.RandomState(1 + i).randint(0, 1027, n).astype(np.int32) for i, n in enumerate(EDGE_ROLLOUT_ROWS)]
        for a in [prob] + rollouts:
            a.setflags(write=False)
        _edge = (w, rows, prob, rollouts)
    return _edge
