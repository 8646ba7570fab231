"""Shared by tests/test_learn_td_wide_cpu.py and tests/test_hip_learn_td_wide.py: the shapes of rl_learn_td_wide's work buffer, the rings
(the 96-row fixture ring of tests/learn_d3qn_cases.py; learn_cases.edge_ring_rows(300) for the 2048-row batch, whose slots therefore repeat
across tiles), seeded slot tables and priorities -- unequal, spanning a factor of 100, the batch's smallest in ONE row of the last tile --
the float64 autograd reference of one wide train_model() step (computed once per batch and left unchanged), the host restatement of the
prescribed order of mean(is_w), and the two plausible-but-wrong tilings: p_min per tile, mean(is_w) per tile."""
import numpy as np
import torch

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perdqn_cases as tc

TILE = 64                 # rows of a tile
HEADER_BYTES = 64         # include/reinlife_hip.h, rl_learn_td_wide_work_bytes
WIDE_MAX = 2048           # RL_LEARN_TD_WIDE_MAX
LR, GAMMA = 1e-3, 0.99
BETA1 = 0.4 + 0.001       # Memory.beta after the first sample()
ONE_TILE_BATCHES = (1, 5, 33, 64)
MULTI_TILE_BATCHES = (65, 96, 128, 130, 2048)
BIG_RING = 300            # rows of the 2048-row batch's ring
BAR = 1e-5                # the project's bar on a gradient tensor, relative to its largest magnitude (tests/test_hip_learn_perdqn.py)
_ref = {}
_prio = {}


def tiles(batch):
    return (batch + TILE - 1) // TILE


def launches(n_steps):
    """RL_LEARN_TD_WIDE_LAUNCHES: check | weights, tiles, update per step | target / counters / beta | pack."""
    return 3 * n_steps + 3


def work_bytes(batch):
    """What rl_learn_td_wide_work_bytes must answer: header, one parameter row per started tile, the tiles' sums of td^2 rounded up to 16 bytes."""
    t = tiles(batch)
    return HEADER_BYTES + t * tc.N_PARAMS * 4 + (t * 4 + 15) // 16 * 16


def ring_of(batch):
    """The host rows a batch is drawn from: the 96-row fixture ring, or 300 seeded rows for the 2048-row batch."""
    return lc.edge_ring_rows(BIG_RING) if batch > 1024 else dc.golden()


def ring_rows(batch):
    return ring_of(batch)["ring_state"].shape[0]


def priorities(rows, seed=3):
    """float32 priorities of a ring of `rows` rows: 0.05 * 100 ** u, u uniform -- unequal, positive, a factor of 100 wide."""
    if (rows, seed) not in _prio:
        p = (0.05 * 100.0 ** np.random.RandomState(seed).random_sample(rows)).astype(np.float32)
        p.setflags(write=False)
        _prio[(rows, seed)] = p
    return _prio[(rows, seed)]


def slots_of(batch, n_steps=1, seed=None):
    """int32 [n_steps, batch] slots of ring_of(batch), with replacement: RandomState(batch).randint(0, rows, ...)."""
    s = np.random.RandomState(batch if seed is None else seed).randint(0, ring_rows(batch), (n_steps, batch)).astype(np.int32)
    s.setflags(write=False)
    return s


def inputs(batch):
    """(slots [batch], priorities of the whole ring): slots_of(batch) with ONE row of the last tile, and no other row of the batch, on the
    slot that holds the ring's smallest priority (0.01) -- p_min sits in one tile only."""
    rows = ring_rows(batch)
    s = slots_of(batch)[0].copy()
    pri = priorities(rows).copy()
    m = int(s[-1])
    s[s == m] = (m + 1) % rows
    s[-1] = m
    pri[m] = np.float32(0.01)
    assert (s == m).sum() == 1 and pri[s].min() == pri[m] and (pri[s] == pri[m]).sum() == 1 and pri[s].max() / pri[s].min() >= 10
    return s, pri


def step64(flat, target_flat, ring, slots, row_scale, gamma=GAMMA):
    """float64 autograd of sum_i row_scale_i * (pred_i - target_i)^2 / B -> (loss, the six gradient tensors).  With row_scale = mean(w) in
    every row this is train_model()'s mean(w) * mean((pred - target)^2)."""
    net, tgt = tc.net_of(np.asarray(flat, np.float64)), tc.net_of(np.asarray(target_flat, np.float64))
    pred, target = tc.pred_target(net, tgt, ring, slots, gamma, torch.float64)
    c = torch.tensor(np.broadcast_to(np.asarray(row_scale, np.float64), (len(slots),)).copy(), dtype=torch.float64)
    loss = (c * (pred - target) ** 2).sum() / len(slots)
    g = torch.autograd.grad(loss, list(net.parameters()))
    return float(loss.detach()), [x.numpy() for x in g]


def case(batch):
    """One step from the fixture's parameters on inputs(batch) with beta = BETA1: (slots, priorities, w float64 [batch] over the WHOLE
    batch, float64 loss, the six float64 gradient tensors)."""
    if batch not in _ref:
        p = tc.golden()
        slots, pri = inputs(batch)
        w = tc.is_weights(pri[slots], BETA1)
        loss64, g64 = step64(p["init"], p["target_init"], ring_of(batch), slots, w.mean())
        out = (slots, pri, w, loss64, g64)
        for a in (slots, pri, w) + tuple(g64):
            a.setflags(write=False)
        _ref[batch] = out
    return _ref[batch]


def prescribed_mean_w(prio_rows, beta):
    """mean(is_w) in the order include/reinlife_hip.h prescribes: w_i = (float)pow((double)p_i / (double)p_min, -beta); per tile the f32 sum,
    rows ascending; the tile sums added in double in tile order and rounded to float once; times 1.0f / B -> (float32 mean_w, float32 w)."""
    p = np.asarray(prio_rows, np.float32)
    w = ((p.astype(np.float64) / np.float64(p.min())) ** -float(beta)).astype(np.float32)
    total = np.float64(-0.0)
    for t in range(0, len(w), TILE):
        s = np.float32(0.0)
        for x in w[t:t + TILE]:
            s = np.float32(s + x)
        total = total + np.float64(s)
    return np.float32(np.float32(total) * (np.float32(1.0) / np.float32(len(w)))), w


def per_tile_p_min_scale(prio_rows, beta):
    """What tiles side by side without the weights pass would use if each took p_min over its OWN rows: the mean of those weights."""
    p = np.asarray(prio_rows, np.float64)
    w = np.concatenate([tc.is_weights(p[t:t + TILE], beta) for t in range(0, len(p), TILE)])
    return np.full(len(p), w.mean())


def per_tile_mean_w_scale(prio_rows, beta):
    """... and if each took mean(is_w) over its own rows (p_min over the whole batch): one scale per tile."""
    w = tc.is_weights(prio_rows, beta)
    return np.concatenate([np.full(len(w[t:t + TILE]), w[t:t + TILE].mean()) for t in range(0, len(w), TILE)])


def worst_relative_error(got, want):
    """max over the tensors of max|got - want| / max|want|, and the per-tensor figures."""
    per = [float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    return max(per), per


def every_slot_in_two_tiles(rows=96):
    """(batch 128 whose rows 64 .. 127 are rows 0 .. 63 again, those 64 distinct slots): every slot of the batch sits in tiles 0 and 1."""
    once = np.random.RandomState(128).permutation(rows)[:TILE].astype(np.int32)
    return np.concatenate([once, once]).astype(np.int32), once
