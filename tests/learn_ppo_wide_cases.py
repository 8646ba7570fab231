"""Shared by tests/test_learn_ppo_wide_cpu.py and tests/test_hip_learn_ppo_wide.py: the slot tables of the wide rollouts on
learn_ppo_cases.edge_case() (the reference's trained PPO weights, 1,027 ring rows, a prob column with ratios 0.5 .. 2), the GAE recursion
restarted at every 32-row tile -- what rl_learn_ppo_wide must NOT compute --, a host model of the work buffer's size, and the float64
replay of three epochs (made once per batch, read-only)."""
import numpy as np

import learn_ppo_cases as pc

TILE = 32
MULTI_TILE = (33, 64, 65, 96, 130, 2048)     # one row into a second tile; whole tiles; an odd tail; more tiles than one wave's lanes
ONE_TILE = (1, 17, 32)
WIDE_MAX = 2048
_replays = {}
_gae32 = pc.gae32                            # (the whole-rollout recursion: grads_by_hand_per_tile rebinds the module's name for one call)


def wide_slots(batch):
    """The rollout of `batch` rows on the 1,027-row edge ring."""
    s = np.random.RandomState(100 + batch).randint(0, 1027, batch).astype(np.int32)
    s.setflags(write=False)
    return s


def work_bytes(batch):
    """include/reinlife_hip.h, rl_learn_ppo_wide_work_bytes: header | lsum[T][2] float64 | td[32 T] | delta[32 T] | partial[T][n_params]."""
    tiles = (batch + TILE - 1) // TILE
    return 64 + tiles * (2 * 8 + 2 * TILE * 4 + 4 * pc.N_PARAMS)


def launches(n_steps, k_epoch):
    """The launches of one rl_learn_ppo_wide call: check | two tile passes and the update per rollout and epoch | counters | pack."""
    return 3 * n_steps * k_epoch + 3


def gae32_per_tile(delta, gamma=pc.GAMMA, lmbda=pc.LMBDA):
    """gae32 restarted from zero at the end of every 32-row tile: the recursion a tiled kernel makes when it forgets the other tiles."""
    delta = np.asarray(delta, np.float32)
    return np.concatenate([_gae32(delta[i:i + TILE], gamma, lmbda) for i in range(0, len(delta), TILE)])


def grads_by_hand_per_tile(flat, rows):
    """learn_ppo_cases.grads_by_hand with the per-tile recursion in gae32's place (the function looks its recursion up when called)."""
    pc.gae32 = gae32_per_tile
    try:
        return pc.grads_by_hand(flat, rows)
    finally:
        pc.gae32 = _gae32


def replay(batch, k_epoch=pc.K_EPOCH):
    """Three epochs on wide_slots(batch) from the edge case's weights in float64 (grads_by_hand + adam64) -> a list, per epoch, of
    (parameters in front of the epoch, loss, gradients, intermediates)."""
    if batch not in _replays:
        w, ring, prob, _ = pc.edge_case()
        rows = pc.rows_of(ring, prob, wide_slots(batch))
        p = np.asarray(w, np.float64).copy()
        m, v = np.zeros_like(p), np.zeros_like(p)
        out = []
        for ep in range(k_epoch):
            loss, grads, mid = pc.grads_by_hand(p, rows)
            out.append((p.copy(), loss, grads, mid))
            p, m, v = pc.adam64(p, m, v, np.concatenate([x.reshape(-1) for x in grads]), ep + 1)
        _replays[batch] = out
    return _replays[batch]
