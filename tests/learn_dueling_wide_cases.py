"""Shared by tests/test_learn_dueling_wide_cpu.py and tests/test_hip_learn_dueling_wide.py: the shapes of rl_learn_dueling_wide's work
buffer, seeded slot tables on the 96-row fixture ring of tests/learn_d3qn_cases.py, the float64 autograd references of the wide D3QN
update (computed once per batch and left unchanged), a host model of the TILED computation in the kernels' orders of summation, and the
plausible-but-wrong model that takes the advantage mean per tile."""
import numpy as np

import learn_d3qn_cases as dc

TILE = 64                 # rows of a tile
HEADER_BYTES = 64         # include/reinlife_hip.h, rl_learn_dueling_wide_work_bytes
STASH_FLOATS = 14         # per row: adv'[8], val', adv[a], val, reward, mask, action
WIDE_MAX = 2048           # RL_LEARN_DUELING_WIDE_MAX
LR, GAMMA = 1e-3, 0.99
RING_ROWS = 96
MULTI_TILE_BATCHES = (65, 96, 128, 130, 2048)
_ref = {}


def tiles(batch):
    return (batch + TILE - 1) // TILE


def work_bytes(batch):
    """What rl_learn_dueling_wide_work_bytes must answer: header, one parameter row per started tile, the tiles' two advantage sums
    rounded up to 16 bytes, the per-row stash."""
    t = tiles(batch)
    return HEADER_BYTES + t * dc.N_PARAMS * 4 + (2 * t * 4 + 15) // 16 * 16 + t * TILE * STASH_FLOATS * 4


def slots_of(batch, n_steps=1, seed=None):
    """int32 [n_steps, batch] slots of the fixture ring, with replacement: RandomState(batch).randint(0, 96, ...)."""
    s = np.random.RandomState(batch if seed is None else seed).randint(0, RING_ROWS, (n_steps, batch)).astype(np.int32)
    s.setflags(write=False)
    return s


def case(batch):
    """One step from the fixture's parameters on slots_of(batch): (slots [batch], float64 loss, the ten float64 gradient tensors)."""
    if batch not in _ref:
        g = dc.golden()
        slots = slots_of(batch)[0]
        loss64, g64 = dc.grads64(g["init"], g["target_init"], g, slots, GAMMA)
        for a in g64:
            a.setflags(write=False)
        _ref[batch] = (slots, loss64, g64)
    return _ref[batch]


def _forward(flat, x):
    """float64 forward of the dueling network without the mean -> (f, ha, hv, adv [n][8], val [n])."""
    w0, b0, wa1, ba1, wa2, ba2, wv1, bv1, wv2, bv2 = [np.asarray(a, np.float64) for a in dc.split(flat)]
    f = np.maximum(x @ w0.T + b0, 0)
    ha = np.maximum(f @ wa1.T + ba1, 0)
    hv = np.maximum(f @ wv1.T + bv1, 0)
    return f, ha, hv, ha @ wa2.T + ba2, (hv @ wv2.T + bv2)[:, 0]


def tiled_model(flat, target_flat, ring, slots, gamma=GAMMA, per_tile_mean=False):
    """The kernels' computation in float64, tile by tile in their orders: per-tile advantage sums -> M' and M over the tiles (or, with
    per_tile_mean=True, each tile's OWN means and its own G over its own rows: what tiles running side by side without the three
    scalars would compute), g_i = 2 td / batch, G over the tiles, dL/dadv = g_i [a = a_i] - G / (8 batch), the backward pass per
    tile, the tiles' partial gradients added in tile order -> (loss, the ten gradient tensors)."""
    slots = np.asarray(slots, np.int64)
    batch, T = len(slots), tiles(len(slots))
    w0, b0, wa1, ba1, wa2, ba2, wv1, bv1, wv2, bv2 = [np.asarray(a, np.float64) for a in dc.split(flat)]
    s, sp = ring["ring_state"][slots].astype(np.float64), ring["ring_state_prime"][slots].astype(np.float64)
    a_i, r = ring["ring_action"][slots].astype(np.int64) & 7, ring["ring_reward"][slots].astype(np.float64)
    mask = 1.0 - ring["ring_done"][slots].astype(np.float64)
    part = [slice(TILE * t, min(TILE * (t + 1), batch)) for t in range(T)]
    fwd_p = [_forward(target_flat, sp[p]) for p in part]
    fwd_e = [_forward(flat, s[p]) for p in part]
    if per_tile_mean:
        m_p = [fw[3].sum() / (8 * fw[3].shape[0]) for fw in fwd_p]
        m_e = [fw[3].sum() / (8 * fw[3].shape[0]) for fw in fwd_e]
    else:
        sum_p = sum_e = 0.0
        for t in range(T):                      # tile ascending
            sum_p += fwd_p[t][3].sum(1).sum()
            sum_e += fwd_e[t][3].sum(1).sum()
        m_p, m_e = [sum_p / (8 * batch)] * T, [sum_e / (8 * batch)] * T
    g_rows, tile_g, tile_l = [], [], []
    for t, p in enumerate(part):
        mx = ((fwd_p[t][3] + fwd_p[t][4][:, None]) - m_p[t]).max(1)
        y = r[p] + (gamma * mask[p]) * mx
        q = (fwd_e[t][3][np.arange(len(mx)), a_i[p]] + fwd_e[t][4]) - m_e[t]
        td = q - y
        g_rows.append(2 * td / batch)
        tile_g.append(g_rows[-1].sum())
        tile_l.append((td * td).sum())
    loss = sum(tile_l) / batch
    G = sum(tile_g)
    grads = [np.zeros(sh) for sh in dc.SHAPES]
    for t, p in enumerate(part):
        f, ha, hv, adv, _ = fwd_e[t]
        n = adv.shape[0]
        mean_term = tile_g[t] / (8 * n) if per_tile_mean else G / (8 * batch)
        dadv = -mean_term * np.ones((n, 8))
        dadv[np.arange(n), a_i[p]] += g_rows[t]
        dval = g_rows[t][:, None]
        da = (dadv @ wa2) * (ha > 0)
        dv = (dval @ wv2) * (hv > 0)
        df = (da @ wa1 + dv @ wv1) * (f > 0)
        for acc, add in zip(grads, [df.T @ s[p], df.sum(0), da.T @ f, da.sum(0), dadv.T @ ha, dadv.sum(0), dv.T @ f, dv.sum(0), dval.T @ hv, dval.sum(0)]):
            acc += add
    return float(loss), grads


def worst_relative_error(got, want):
    """max over the tensors of max|got - want| / max|want|, and the per-tensor figures."""
    per = [float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    return max(per), per
