"""Shared by tests/test_learn_perdqn_cpu.py and tests/test_hip_learn_perdqn.py: the fixture tests/golden/learn_perdqn.npz (the reference's
own PERDQNAgent.train_model(), append_sample and Memory, tools/gen_golden_learn_perdqn.py), a torch restatement of one train_model()
step in any dtype -- the loss with its mean(is_weight) factor, its gradients, the batch rows' new priorities and the importance weights
as rl_learn_td makes them -- and the host restatement of rl_learn_td_draw's race.  The ring and slots are tests/golden/learn_d3qn.npz's."""
import os

import numpy as np
import torch

import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc

ROOT = dc.ROOT
SHAPES = [(64, 153), (64,), (64, 64), (64,), (8, 64), (8,)]
NAMES = ["fc.0.weight", "fc.0.bias", "fc.2.weight", "fc.2.bias", "fc.4.weight", "fc.4.bias"]
N_PARAMS = sum(int(np.prod(s)) for s in SHAPES)
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_perdqn.npz")) as z:
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


def net_of(flat, dtype=torch.float64):
    """PERDQN.py's DQN module: fc.0 153 -> 64, fc.2 64 -> 64, fc.4 64 -> 8, ReLU between."""
    net = torch.nn.Sequential(torch.nn.Linear(153, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 8)).to(dtype)
    with torch.no_grad():
        for p, v in zip(net.parameters(), split(flat)):
            p.copy_(torch.from_numpy(np.array(v)).to(dtype))
    return net


def flat_of(net):
    return np.concatenate([p.detach().numpy().reshape(-1) for p in net.parameters()])


def q_values(flat, states):
    with torch.no_grad():
        return net_of(np.asarray(flat, np.float64))(torch.tensor(np.asarray(states), dtype=torch.float64)).numpy()


def is_weights(prio, beta):
    """rl_learn_td's importance weights of a batch: (p_i / min_j p_j) ** -beta in float64 (the reference's
    (n p_i / total) ** -beta / max, with n and total cancelled)."""
    p = np.asarray(prio, np.float64)
    return (p / p.min()) ** -float(beta)


def pred_target(net, tgt, ring, slots, gamma, dtype):
    idx = np.asarray(slots, np.int64)
    s, sp = torch.tensor(ring["ring_state"][idx], dtype=dtype), torch.tensor(ring["ring_state_prime"][idx], dtype=dtype)
    a = torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1)
    r, done = torch.tensor(ring["ring_reward"][idx], dtype=dtype), torch.tensor(ring["ring_done"][idx].astype(np.float64), dtype=dtype)
    return net(s).gather(1, a).squeeze(1), r + (1 - done) * gamma * tgt(sp).max(1)[0].detach()


def step(flat, target_flat, ring, slots, w, gamma, dtype=torch.float64, prio_e=0.01, prio_a=0.6):
    """One train_model() in `dtype` -> (loss = mean(w) * mean((pred - target)^2), the six gradient tensors, the batch rows' new priorities
    (|pred - target| + e) ** a, pred, target), float64 arrays."""
    net, tgt = net_of(np.asarray(flat, np.float64), dtype), net_of(np.asarray(target_flat, np.float64), dtype)
    pred, target = pred_target(net, tgt, ring, slots, gamma, dtype)
    loss = (torch.tensor(np.asarray(w), dtype=dtype) * torch.nn.functional.mse_loss(pred, target)).mean()
    g = torch.autograd.grad(loss, list(net.parameters()))
    err = torch.abs(pred - target).detach().double().numpy()
    return float(loss.detach()), [x.double().numpy() for x in g], (err + prio_e) ** prio_a, pred.detach().double().numpy(), target.double().numpy()


def torch_steps(p, g, dtype=torch.float32):
    """The fixture's three train_model() calls restated: the memory's priorities and beta, the weights, the loss, one Adam step each ->
    (final flat parameters, priorities [3][64], is_weights [3][64] float64, beta [3])."""
    net, tgt = net_of(p["init"], dtype), net_of(p["target_init"], dtype)
    opt = torch.optim.Adam(net.parameters(), lr=float(p["lr"]))
    prio = p["prio_init"].astype(np.float32).copy()
    beta, e, a = float(p["beta0"]), np.float32(p["prio_e"]), np.float32(p["prio_a"])
    prios, ws, betas = [], [], []
    for s in range(p["slots"].shape[0]):
        idx = p["slots"][s].astype(np.int64)
        beta = min(1.0, beta + float(p["beta_increment"]))
        w = is_weights(prio[idx], beta)
        pred, target = pred_target(net, tgt, g, idx, float(p["gamma"]), dtype)
        err = torch.abs(pred - target).detach().numpy().astype(np.float32)
        prio[idx] = (err + e) ** a   # float32 arithmetic, as numpy 2 makes it of float32 errors and Python floats
        loss = (torch.tensor(w, dtype=dtype) * torch.nn.functional.mse_loss(pred, target)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        prios.append(prio[idx].copy()); ws.append(w); betas.append(beta)
    return flat_of(net), np.stack(prios), np.stack(ws), np.array(betas)


def host_draw(keys, priority, seed, brain, calls, n_draws):
    """rl_learn_td_draw's pick restated (learn_perd3qn_cases.host_draw with RL_SITE_LEARN_TD and the priority itself as the weight):
    draw d takes the row with the smallest (t, v, slot): v = mix64(key ^ salt_d), U = ((v >> 41) + 0.5) / 2^23, t = -log(U) / p."""
    from reinlife_amd import _lib
    keys = np.asarray(keys, np.uint64)
    w = np.asarray(priority, np.float32)
    rows = np.zeros(n_draws, np.int64)
    for d, salt in enumerate(pc._salts(seed, brain, calls, _lib.SITE_LEARN_TD, n_draws)):
        v = pc._mix64(keys ^ salt)
        u = ((v >> np.uint64(41)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(w > 0, -np.log(u) / w, np.inf).astype(np.float32)
        rows[d] = np.lexsort((np.arange(len(keys)), v, t))[0]
    return rows


def stamp(priority, seen, count, p_new):
    """k_prio_prepare<TD>'s stamp on the host: slots [seen, count) mod capacity (all once count - seen >= capacity) get p_new."""
    out = np.array(priority, np.float32)
    cap = len(out)
    if count - seen >= cap:
        out[:min(count, cap)] = p_new
    else:
        for c in range(seen, count):
            out[c % cap] = p_new
    return out


# ---- inputs beyond the fixture (tests/test_learn_late_edges_cpu.py, tests/test_hip_learn_perdqn_edges.py) ----
EDGE_BATCHES = (64, 33, 1)
_edge = None


def edge_case():
    """One step on the reference's TRAINED weights: (ckpt_perdqn_gene_1_weights of tests/golden/perdqn.npz, the same times
    learn_cases.TARGET_SCALE as the target, learn_cases.edge_ring_rows(1027), the priorities learn_perd3qn_cases.edge_priorities(1027)
    with their zeros replaced by p_new, the minibatches of 64, 33 and 1 rows RandomState(1..3).randint(0, 1027, n)).  Made once, read-only."""
    global _edge
    if _edge is None:
        import learn_cases as lc
        with np.load(os.path.join(ROOT, "tests", "golden", "perdqn.npz")) as z:
            w = z["ckpt_perdqn_gene_1_weights"]
        tgt = (w * lc.TARGET_SCALE).astype(np.float32)
        rows = lc.edge_ring_rows(1027)
        pri = pc.edge_priorities(1027).copy()
        pri[pri == 0] = golden()["p_new"]
        batches = [np.random.RandomState(1 + i).randint(0, 1027, n).astype(np.int32) for i, n in enumerate(EDGE_BATCHES)]
        for a in [w, tgt, pri] + batches:
            a.setflags(write=False)
        _edge = (w, tgt, rows, pri, batches)
    return _edge
