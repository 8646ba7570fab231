"""What the CPU and GPU tests of rl_learn_merge / rl_learn_export / rl_policy_pack_device share: the float64 reference of the merge (an
explicit loop over the participants in rank order, then one division, then astype(float32)), the synthetic all-gather tables, and the
packer's edge-case parameters.  Every comparison made against these is bit for bit."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DQN, D3QN, PERD3QN, PPO, PERDQN = range(5)
KINDS = (DQN, D3QN, PERD3QN, PPO, PERDQN)
N_PARAMS = {DQN: 28488, D3QN: 53897, PERD3QN: 53897, PPO: 107529, PERDQN: 14536}
FIXTURE = {DQN: "learn_dqn", D3QN: "learn_d3qn", PERD3QN: "learn_perd3qn", PPO: "learn_ppo", PERDQN: "learn_perdqn"}
# first-layer width and the state-dict offset of the second weight matrix (its rows: the first layer's width)
L1_WIDTH = {DQN: 128, D3QN: 128, PERD3QN: 128, PPO: 256, PERDQN: 64}
SENTINEL = 0x7fc12345   # a NaN with a payload: no packer writes it
PATTERNS = ("all_equal", "all_zero", "one_behind", "one_ahead", "high_word")


def merge_floats(kind):
    return 3 * N_PARAMS[kind] + 2


def segments(kinds):
    """[(first float, n_params)] of the learners' segments in a row, and the floats of the whole row."""
    segs, off = [], 0
    for k in kinds:
        segs.append((off, N_PARAMS[k]))
        off += merge_floats(k)
    return segs, off


def steps_of(pattern, n_ranks, shift=0):
    """The Adam step counts of the ranks' rows for one learner.  `shift` moves the odd rank out, so that the learners of one call hold
    different masks."""
    odd = shift % n_ranks
    if pattern == "all_equal":
        return [7] * n_ranks
    if pattern == "all_zero":
        return [0] * n_ranks
    if pattern == "one_behind":
        return [5 if r == odd else 7 for r in range(n_ranks)]
    if pattern == "one_ahead":
        return [9 if r == odd else 7 for r in range(n_ranks)]
    if pattern == "high_word":   # the low words are equal: only the high word tells the rows apart
        return [(1 << 32) + 3 if r == odd else 3 for r in range(n_ranks)]
    raise KeyError(pattern)


def make_rows(kinds, n_ranks, patterns, seed, pad=0):
    """A synthetic all-gather: float32 [n_ranks, stride] with every learner's params | adam_m | adam_v | step words, stride = the segments
    + pad.  patterns: one name per learner.  The values carry what a float mean can get wrong: both signs, zeros of both signs,
    denormals, magnitudes from 1e-30 to 1e3."""
    segs, total = segments(kinds)
    rng = np.random.RandomState(seed)
    rows = np.zeros((n_ranks, total + pad), np.float32)
    rows[:, total:] = np.float32(-77.0)
    for i, ((off, n), pat) in enumerate(zip(segs, patterns)):
        steps = steps_of(pat, n_ranks, shift=i + 1)
        for r in range(n_ranks):
            p = (rng.uniform(-0.1, 0.1, n) * 10.0 ** rng.randint(-3, 2, n)).astype(np.float32)
            m = (rng.standard_normal(n) * 1e-3).astype(np.float32)
            v = (rng.uniform(0, 1, n) ** 4 * 1e-4).astype(np.float32)
            for a in (p, m, v):
                a[rng.randint(0, n, 40)] = np.float32(0.0)
                a[rng.randint(0, n, 40)] = np.float32(-0.0) if a is not v else np.float32(0.0)
                a[rng.randint(0, n, 40)] = np.float32(1e-30)
                a[rng.randint(0, n, 40)] = np.float32(1e-41)          # denormal
                a[rng.randint(0, n, 40)] = np.float32(1234.5678)
            p[:8] = np.float32(-0.0)                                   # -0.0 on EVERY rank: the mean keeps the sign
            rows[r, off:off + n], rows[r, off + n:off + 2 * n], rows[r, off + 2 * n:off + 3 * n] = p, m, v
            rows[r, off + 3 * n:off + 3 * n + 2] = np.array([steps[r] & 0xffffffff, steps[r] >> 32], np.uint32).view(np.float32)
    return rows


def row_steps(rows, off, n):
    words = np.ascontiguousarray(rows[:, off + 3 * n:off + 3 * n + 2]).view(np.uint32)
    return [int(np.array([int(lo) | (int(hi) << 32)], np.uint64).view(np.int64)[0]) for lo, hi in words]


def merge_reference(rows, kinds):
    """Per learner (params, adam_m, adam_v, step count) as rl_learn_merge defines them: the participants are the ranks whose step count is
    the maximum; every element is their sum IN RANK ORDER in float64 -- an explicit loop, started from -0.0, the additive identity, so
    that one participant gives its own bits -- divided by their number in float64, rounded to float32 once."""
    segs, _ = segments(kinds)
    out = []
    for off, n in segs:
        steps = row_steps(rows, off, n)
        mx = max(steps)
        part = [r for r in range(rows.shape[0]) if steps[r] == mx]
        merged = []
        for a in range(3):
            acc = np.full(n, -0.0, np.float64)
            for r in part:
                acc = acc + rows[r, off + a * n:off + (a + 1) * n].astype(np.float64)
            merged.append((acc / np.float64(len(part))).astype(np.float32))
        out.append((merged[0], merged[1], merged[2], mx, part))
    return out


def host_pack(kind, flat, prefill=None):
    """rl_policy_pack_weights(kind, flat) into a buffer pre-filled with the sentinel's bits (or `prefill`)."""
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    assert flat.size == N_PARAMS[kind] == lib.rl_policy_n_params(kind)
    packed = np.full(lib.rl_policy_packed_floats(kind), SENTINEL, np.uint32).view(np.float32) if prefill is None else prefill.copy()
    assert lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


def trained_params(kind):
    """The `final` parameters of the kind's learning fixture (tests/golden/learn_*.npz): a trained state."""
    with np.load(os.path.join(ROOT, "tests", "golden", FIXTURE[kind] + ".npz")) as z:
        return np.array(z["final"], np.float32)


def edge_params(kind, seed):
    """Seeded random parameters with the rows the packer's scale rule can get wrong: feature 3 of the first layer all zero, feature 5's
    largest magnitude exactly a power of two (and the rest below it), feature 7 of magnitudes near 1e-30 (below the clamp of the scale's
    exponent), feature 9 near 1e30; the same four in the second weight matrix."""
    rng = np.random.RandomState(seed)
    n = N_PARAMS[kind]
    flat = (rng.uniform(0.25, 1.0, n) * rng.choice([-1.0, 1.0], n) * 2.0 ** rng.randint(-9, 2, n)).astype(np.float32)
    w = L1_WIDTH[kind]
    second = 153 * w + w                                               # the second weight matrix: rows of w inputs
    for base, n_in in ((0, 153), (second, w)):
        row = lambda o: slice(base + o * n_in, base + (o + 1) * n_in)   # noqa: E731
        flat[row(3)] = 0.0
        flat[row(5)] = (rng.uniform(-0.24, 0.24, n_in)).astype(np.float32)
        flat[base + 5 * n_in + 11] = np.float32(-0.25)
        flat[row(7)] = (rng.uniform(0.5, 2.0, n_in) * 1e-30 * rng.choice([-1.0, 1.0], n_in)).astype(np.float32)
        flat[row(9)] = (rng.uniform(0.5, 2.0, n_in) * 1e30 * rng.choice([-1.0, 1.0], n_in)).astype(np.float32)
    return flat
