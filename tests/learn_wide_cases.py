"""Shared by tests/test_learn_wide_cpu.py and tests/test_hip_learn_wide.py: the shapes of rl_learn_wide's work buffer, seeded slot tables
and the float64 references of the wide DQN update, computed once per case from tests/learn_cases.py (the torch restatement of
ReinLife/Models/DQN.py:126-130, 142-153) and left unchanged."""
import numpy as np

import learn_cases as lc

TILE = 32                 # rows of a tile
HEADER_BYTES = 64         # include/reinlife_hip.h, rl_learn_wide_work_bytes
WIDE_MAX = 2048           # RL_LEARN_WIDE_MAX
LR, GAMMA = 0.0005, 0.98
EDGE_ROWS = 200           # rows of the trained-weight cases' ring (lc.edge_ring_rows)
_ref = {}


def tiles(batch):
    return (batch + TILE - 1) // TILE


def work_bytes(batch):
    """What rl_learn_wide_work_bytes must answer: header, one parameter row per started tile, the tile losses rounded up to 16 bytes."""
    t = tiles(batch)
    return HEADER_BYTES + t * lc.N_PARAMS * 4 + (t * 4 + 15) // 16 * 16


def slot_table(n_steps, batch, size, seed, equal_tile=None):
    """int32 [n_steps, batch] slots in [0, size), seeded, with a duplicate in every step; equal_tile=t makes all rows of tile t of
    every step the same slot (one row drawn 32 times)."""
    rng = np.random.RandomState(seed)
    s = rng.randint(0, size, size=(n_steps, batch)).astype(np.int32)
    if batch > 1:
        s[:, batch - 1] = s[:, 0]
    if equal_tile is not None:
        s[:, TILE * equal_tile:TILE * (equal_tile + 1)] = s[:, TILE * equal_tile:TILE * equal_tile + 1]
    s.setflags(write=False)
    return s


def edge_case(batch, equal_tile=None, n_rows=EDGE_ROWS):
    """One step of the reference's trained DQN weights (target = weights * 0.96875) on lc.edge_ring_rows(n_rows): (eval, target, rows,
    slots [batch], float64 loss, the six float64 gradient tensors).  Computed once per case."""
    key = (batch, equal_tile) if n_rows == EDGE_ROWS else (batch, equal_tile, n_rows)
    if key not in _ref:
        w, tgt = lc.pretrained("DQN")
        rows = lc.edge_ring_rows(n_rows)
        slots = slot_table(1, batch, n_rows, 100 + batch, equal_tile)[0]
        loss64, g64 = lc.grads64(w, tgt, rows, slots, GAMMA)
        for a in g64:
            a.setflags(write=False)
        _ref[key] = (w, tgt, rows, slots, loss64, g64)
    return _ref[key]


def tile_loss_model(w, tgt, rows, slots, dtype=None):
    """k_wide_tile's loss bookkeeping on the host: the smooth-L1 term of every batch row in float64, summed per 32-row tile, the tiles
    summed in double and divided by the batch (k_wide_apply) -> (the loss, the tile sums [tiles])."""
    import torch
    with torch.no_grad():
        td = lc.td_errors(lc.qnet(np.asarray(w, np.float64)), lc.qnet(np.asarray(tgt, np.float64)), rows, slots, GAMMA, torch.float64).numpy()[:, 0]
    term = np.where(np.abs(td) < 1, 0.5 * td * td, np.abs(td) - 0.5)
    pad = np.zeros(tiles(len(slots)) * TILE)
    pad[:len(slots)] = term
    per_tile = pad.reshape(-1, TILE).sum(1)
    return float(per_tile.sum() / len(slots)), per_tile
