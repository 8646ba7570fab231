"""Shared by tests/test_learn_prio_draw_rank_cpu.py and tests/test_hip_learn_prio_draw_rank.py: rl_learn_prioritized_draw_rank /
rl_learn_td_draw_rank restated on the host, bit for bit -- the order is learn_rank_cases.host_order, the cumulative sum float64 in
segments of 64 ranks (np.cumsum inside a segment, a sequential sum of the segments' totals, one add), the target one or three rounded
float64 operations on the draw's Philox words, and the pick numpy's searchsorted with the clamp rule.  The weights are float32 as the
device left them (its powf is not numpy's)."""
import ctypes as C

import numpy as np

import learn_rank_cases as rc

PRIO_RANK_LAUNCHES = 8   # RL_LEARN_PRIO_DRAW_RANK_LAUNCHES
SEG = 64                 # ranks per segment of the cumulative sum


def work_bytes(capacity):
    """rl_learn_prio_draw_rank_work_bytes: rl_learn_draw_rank's buffer, then one float64 per segment of 64 rows, rounded up to 16 bytes."""
    return rc.work_bytes(capacity) + (8 * ((int(capacity) + SEG - 1) // SEG) + 15) // 16 * 16


def host_cum(weight32_in_rank_order):
    """cum[r] = base[r // 64] + local[r]: w = the float32 weights as float64 where > 0, else 0 (NaN too); local the inclusive
    left-to-right sum inside r's segment, base the exclusive left-to-right sum of the segments' totals -> float64 [size]."""
    w32 = np.asarray(weight32_in_rank_order, np.float32)
    n = len(w32)
    if n == 0:
        return np.zeros(0, np.float64)
    with np.errstate(invalid="ignore"):
        w = np.where(w32 > 0, w32.astype(np.float64), 0.0)
    n_seg = (n + SEG - 1) // SEG
    padded = np.zeros(n_seg * SEG, np.float64)
    padded[:n] = w
    local = np.cumsum(padded.reshape(n_seg, SEG), axis=1, dtype=np.float64)   # (accumulate: strictly left to right)
    base, run = np.zeros(n_seg, np.float64), np.float64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(n_seg):
            base[s] = run
            run = run + local[s, SEG - 1]
        return (base[:, None] + local).reshape(-1)[:n]


def philox_words(seed, brain, calls, site, n_draws):
    """Words 0 and 1 of rl_philox(seed, 0, brain, (uint32)calls, site, d), d = 0 .. n_draws - 1 -> two uint64 [n_draws]."""
    from reinlife_amd import _lib
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    x, y = np.zeros(n_draws, np.uint64), np.zeros(n_draws, np.uint64)
    for d in range(n_draws):
        lib.rl_philox(seed, 0, brain, calls & 0xffffffff, site, d, C.byref(out))
        x[d], y[d] = int(out[0]), int(out[1])
    return x, y


def uniforms(x, y):
    """u = (double)(((y << 32) | x) >> 11) * 2^-53: exact, in [0, 1)."""
    return (((y << np.uint64(32)) | x) >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)


def targets(u, total, batch, stratified):
    """Independent: u * total.  Stratified: ((double)j + u) * (total / batch), j = d % batch -- every operation rounded on its own."""
    u, total = np.asarray(u, np.float64), np.float64(total)
    if not stratified:
        return u * total
    seg = total / np.float64(batch)
    return ((np.arange(len(u)) % batch).astype(np.float64) + u) * seg


def pick_ranks(cum, target):
    """The smallest rank with cum > target; none (target >= total): the smallest rank with cum == total."""
    cum = np.asarray(cum, np.float64)
    r = np.searchsorted(cum, target, side="right")
    return np.where(r >= len(cum), np.searchsorted(cum, cum[-1], side="left"), r).astype(np.int64)


def host_ranks(cum, x, y, batch, stratified):
    """The rank of every draw from its Philox words, the uniform rank rule where the total is zero or not finite -> int64 [n_draws]."""
    size = len(cum)
    total = cum[-1]
    if not (total > 0) or not np.isfinite(total):
        return ((x * np.uint64(size)) >> np.uint64(32)).astype(np.int64)
    return pick_ranks(cum, targets(uniforms(x, y), total, batch, stratified))


def host_draw(keys, weight32, seed, brain, calls, site, n_steps, batch, stratified):
    """(slots int32 [n_steps * batch], ranks, order, cum) for one learner: keys and float32 weights by slot, rows [0, size)."""
    n_draws = n_steps * batch
    size = len(keys)
    if size == 0:
        return np.zeros(n_draws, np.int32), np.zeros(n_draws, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
    order = rc.host_order(keys)
    cum = host_cum(np.asarray(weight32, np.float32)[order])
    x, y = philox_words(seed, brain, calls, site, n_draws)
    ranks = host_ranks(cum, x, y, batch, stratified)
    return order[ranks].astype(np.int32), ranks, order, cum


def brute_force_ranks(weights, target):
    """Exact: Python fractions of the float64 weights -- the smallest rank whose exact cumulative sum exceeds the target."""
    from fractions import Fraction
    out = []
    for t in np.atleast_1d(target):
        run, t = Fraction(0), Fraction(float(t))
        for r, w in enumerate(weights):
            run += Fraction(float(w)) if w > 0 else 0
            if run > t:
                out.append(r)
                break
        else:
            out.append(max(r for r, w in enumerate(weights) if w > 0))
    return np.array(out, np.int64)


def cycle_priorities(n=48):
    """The priorities of the counting tests: cycling 0, 0.25, 1, 4."""
    return np.tile(np.array([0.0, 0.25, 1.0, 4.0], np.float32), (n + 3) // 4)[:n]
