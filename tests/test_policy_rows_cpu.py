"""CPU: the builders, references and premises of tests/test_hip_policy_rows.py (mixed-magnitude rows, exact ties, degenerate rows,
within-row spread below the input layer), so that what the GPU tests assume is itself asserted where no GPU is needed:

  * the f64 reference (oracle/cpu_bench.forward on float64 layers; the same for PERDQN) and how far a plain numpy f32 forward is from it on
    the very rows the GPU tests feed -- the per-row bar 1e-5 * max_j |ref_ij| is only a fair demand where f32 itself stays ~10x inside it;
  * power-of-two equivariance of an f32 forward with zeroed biases on those rows, bit for bit (so that nothing but a wrong row scale can
    break it in the kernels), and of the host packing: a first layer scaled by 2^k packs to the SAME f16 planes and a different unscale;
  * the tied heads: every row's maximum lies in a tied group, and the expected answers cover 0 .. 6;
  * a numpy emulation of the 2 x f16 block-scaled layer (row scale, hi / lo split, three partial products) that meets every identity --
    and stops meeting them under the faults the GPU tests target (a neighbour's row maximum; `>=` in the argmax), which is the argument
    that those tests would fail on such a kernel.
"""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
KINDS = ["DQN", "D3QN", "PERD3QN", "PPO", "PERDQN"]
Q_KINDS = ["DQN", "D3QN", "PERD3QN", "PERDQN"]
DUELING = ("D3QN", "PERD3QN")
SHAPES = {"DQN": [(128, 153), (64, 128), (8, 64)],
          "D3QN": [(128, 153), (128, 128), (8, 128), (128, 128), (1, 128)],
          "PERD3QN": [(128, 153), (128, 128), (8, 128), (128, 128), (1, 128)],
          "PPO": [(256, 153), (256, 256), (8, 256), (1, 256)],
          "PERDQN": [(64, 153), (64, 64), (8, 64)]}
HEAD = {"DQN": 2, "D3QN": 2, "PERD3QN": 2, "PPO": 2, "PERDQN": 2}   # index of the layer whose 8 outputs are argmax'ed / softmax'ed
ROW_BAR = 1e-5        # the project's bar, per row: |out - ref64| <= ROW_BAR * max_j |ref64_ij|  (PPO: atol on the probabilities)
F32_MARGIN = 1e-6     # what a numpy f32 forward of the same rows must stay within for the bar to be a fair demand
K_RANGE = {"DQN": (-40, 40), "D3QN": (-40, 40), "PERD3QN": (-40, 40), "PERDQN": (-40, 40), "PPO": (-40, 6)}
# supported magnitude of a row's largest element: row_scale() clamps the biased exponent to [32, 230] (rl_policy_dev.h)
CLAMP_LO, CLAMP_HI = -95, 103
# pattern[i] = which distinct row output i copies; every group has at least two members, so every row's maximum is tied.  The first
# indices of the groups are 0,1,2 / 0,3,4 / 0,5 / 0,6: the expected answer takes every value 0 .. 6 over the arrangements.
TIE_PATTERNS = {"012": [0, 1, 2, 0, 1, 2, 0, 1], "034": [0, 0, 0, 1, 2, 1, 2, 1], "05": [0, 0, 0, 0, 0, 1, 0, 1], "06": [0, 0, 0, 0, 0, 0, 1, 1]}


# ---------------------------------------------------------------------------------------------------------------------
# builders (imported by the GPU module)
# ---------------------------------------------------------------------------------------------------------------------
def golden_rows():
    return np.load(os.path.join(GOLDEN, "models.npz"))["obs"].astype(np.float32)


def golden_weights(name):
    """The reference's seeded networks (tests/golden/models.npz); PERDQN: the seed-0 initial weights of tests/golden/perdqn.npz."""
    if name == "PERDQN":
        return np.load(os.path.join(GOLDEN, "perdqn.npz"))["init_0_greedy"].astype(np.float32).copy()
    return np.load(os.path.join(GOLDEN, "models.npz"))[name + "_weights"].astype(np.float32).copy()


def offsets(name):
    """[(weight offset, bias offset, n_out, n_in)] of the flat state dict."""
    out, o = [], 0
    for n_out, n_in in SHAPES[name]:
        out.append((o, o + n_out * n_in, n_out, n_in))
        o += n_out * n_in + n_out
    return out, o


def unpack(name, flat, dtype=np.float64):
    """flat state dict -> [(W.T, b)] in `dtype` (the layout of oracle/cpu_bench.unpack)."""
    offs, total = offsets(name)
    assert total == len(flat), (name, total, len(flat))
    return [(np.ascontiguousarray(flat[w:w + n_out * n_in].reshape(n_out, n_in).T.astype(dtype)), flat[b:b + n_out].astype(dtype))
            for w, b, n_out, n_in in offs]


def forward(name, flat, x, dtype=np.float64):
    """The reference networks in `dtype`: oracle/cpu_bench.forward on layers cast to it (PERDQN: the three-layer MLP, PERDQN.py:311-323)."""
    from oracle import cpu_bench
    layers = unpack(name, flat, dtype)
    x = np.ascontiguousarray(x, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        if name == "PERDQN":
            return cpu_bench.forward("DQN", layers, x)
        return cpu_bench.forward(name, layers, x)


def row_err(out, ref):
    """Per row: max_j |out - ref| / max_j |ref| (0 where the reference row is all zero and so is the output)."""
    d = np.abs(out.astype(np.float64) - ref).max(axis=1)
    m = np.abs(ref).max(axis=1)
    return np.where(m > 0, d / np.where(m > 0, m, 1.0), np.where(d > 0, np.inf, 0.0))


def err_of(name, out, ref):
    """The figure the bar applies to: per-row relative for the Q kinds, absolute on the probabilities for PPO."""
    return np.abs(out.astype(np.float64) - ref).max(axis=1) if name == "PPO" else row_err(out, ref)


def zero_biases(name, flat):
    flat = flat.copy()
    for w, b, n_out, n_in in offsets(name)[0]:
        flat[b:b + n_out] = 0.0
    return flat


def scale_layer1(name, flat, k):
    """Brain B of brain A: the first layer's weights times 2^k (exact in f32)."""
    flat = flat.copy()
    w, b, n_out, n_in = offsets(name)[0][0]
    flat[w:b] = np.ldexp(flat[w:b], k)
    return flat


def mixed_exponents(n, lo, hi, seed):
    """k_i per row: even rows from the lowest third of [lo, hi], odd rows from the highest third (the parity flips per 32-row tile so that
    both halves of a tile see both) -- neighbouring rows differ by at least (hi - lo) / 3 binades."""
    rng = np.random.RandomState(seed)
    third = (hi - lo) // 3
    low = rng.randint(lo, lo + third + 1, size=n)
    high = rng.randint(hi - third, hi + 1, size=n)
    i = np.arange(n)
    return np.where(((i + i // 32) & 1) == 0, low, high).astype(np.int32)


def scaled(x, k):
    """Row i of x times 2^k_i, exactly (float32; the golden rows' smallest non-zero magnitude is far from the subnormals)."""
    return np.ldexp(x.astype(np.float32), np.asarray(k, np.int32)[:, None]).astype(np.float32)


def mixed_rows(name, n, seed=1):
    """n rows for brain kind `name`: the 640 golden rows, cycled, row i times 2^k_i.  Returns (rows, base rows, k)."""
    base = golden_rows()
    base = base[np.arange(n) % base.shape[0]]
    k = mixed_exponents(n, *K_RANGE[name], seed=seed)
    return scaled(base, k), base, k


def tied_weights(name, pattern, seed, all_equal=False):
    """golden_weights(name) with the argmax'ed head (advantage head of the dueling kinds) rebuilt: output i carries distinct row
    pattern[i] -- weights and bias.  The distinct rows are fresh draws of the head's own magnitude (copying rows of the golden head in
    place leaves one action winning 639 of 640 rows), made orthogonal to the mean of the head's input over the golden rows.  all_equal: zero weights and one bias for all eight outputs."""
    flat = golden_weights(name)
    w, b, n_out, n_in = offsets(name)[0][HEAD[name]]
    assert n_out == 8
    if all_equal:
        flat[w:b] = 0.0
        flat[b:b + 8] = np.float32(0.37)
        return flat
    rng = np.random.RandomState(seed)
    amp = float(np.abs(flat[w:b]).max())
    L = unpack(name, flat)
    h = np.maximum(np.maximum(golden_rows().astype(np.float64) @ L[0][0] + L[0][1], 0) @ L[1][0] + L[1][1], 0)   # the head's input rows
    hbar = h.mean(axis=0)
    rows = rng.uniform(-1.0, 1.0, size=(3, n_in))
    rows -= np.outer(rows @ hbar / (hbar @ hbar), hbar)      # blind to the mean hidden row: which group wins is decided row by row
    rows = (rows * (amp / np.abs(rows).max())).astype(np.float32)
    bias = (rng.uniform(-1.0, 1.0, size=3) * 0.01 * amp).astype(np.float32)
    pattern = np.asarray(pattern)
    flat[w:b] = rows[pattern].reshape(-1)
    flat[b:b + 8] = bias[pattern]
    return flat


def group_firsts(pattern):
    """first output index of every tied group, ascending"""
    return sorted({g: i for i, g in reversed(list(enumerate(pattern)))}.values())


def tie_expected(ref, pattern):
    """(expected action, gap between DISTINCT groups) of reference outputs whose duplicated outputs are bit-equal: the first index of the
    group that holds the maximum -- np.argmax's and rl_oracle.c's first-maximum rule."""
    firsts = group_firsts(pattern)
    assert all(np.array_equal(ref[:, i], ref[:, firsts[sorted(set(pattern)).index(g)]]) for i, g in enumerate(pattern)), "duplicates differ"
    sub = ref[:, firsts]
    want = np.asarray(firsts)[sub.argmax(axis=1)]
    if len(firsts) == 1:
        return want, np.full(ref.shape[0], np.inf)
    srt = np.sort(sub, axis=1)
    return want, srt[:, -1] - srt[:, -2]


def argmax_first(q):
    """the reference's rule: `>` keeps the first maximum (tile1_finish, rl_oracle.c)"""
    a = np.zeros(q.shape[0], np.int64)
    best = q[:, 0].copy()
    for i in range(1, q.shape[1]):
        gt = q[:, i] > best
        a = np.where(gt, i, a); best = np.where(gt, q[:, i], best)
    return a


def argmax_last(q):
    """the fault the tie tests target: `>=` keeps the LAST maximum"""
    a = np.zeros(q.shape[0], np.int64)
    best = q[:, 0].copy()
    for i in range(1, q.shape[1]):
        ge = q[:, i] >= best
        a = np.where(ge, i, a); best = np.where(ge, q[:, i], best)
    return a


def saturated_ppo(seed=3):
    """PPO weights whose head is scaled until every golden row's top-2 logit gap exceeds 200: exp(-200) < 2^-288, so the softmax is one-hot
    in f64 and in f32.  Returns (flat, hot index per golden row)."""
    flat = golden_weights("PPO")
    w, b, n_out, n_in = offsets("PPO")[0][2]
    rng = np.random.RandomState(seed)
    flat[w:b] = rng.uniform(-0.08, 0.08, size=b - w).astype(np.float32)
    x = golden_rows().astype(np.float64)
    L = unpack("PPO", flat)
    h = np.maximum(np.maximum(x @ L[0][0] + L[0][1], 0) @ L[1][0] + L[1][1], 0)
    lg = h @ L[2][0] + L[2][1]
    srt = np.sort(lg, axis=1)
    gap = float((srt[:, -1] - srt[:, -2]).min())
    assert gap > 0
    mult = np.float32(2.0 ** np.ceil(np.log2(400.0 / gap)))
    flat[w:b + 8] *= mult
    return flat, lg.argmax(axis=1)


def degenerate_tile(seed=7):
    """One 32-row tile: ordinary golden rows with the degenerate ones between them.  Returns (rows, {label: row index}).  `checked` rows
    lie inside the clamp range [2^-95, 2^103] (or are zero) and must meet the f64 reference; `outside` ones only have to stay harmless."""
    g = golden_rows()
    x = g[:32].copy()
    idx = {"zero": 3, "negzero": 6, "one-element": 9, "min-2^-94": 12, "max-2^102": 15, "subnormal": 18, "tiny-2^-110": 21, "huge-2^110": 24}
    x[3] = 0.0
    x[6] = -0.0
    x[9] = 0.0; x[9, 100] = -0.75
    x[12] = np.ldexp(g[40], -94)
    x[15] = np.ldexp(g[41], 102)
    x[18] = np.float32(1e-41) * np.sign(g[42])
    x[21] = np.ldexp(g[43], -110)
    x[24] = np.ldexp(g[44], 110)
    return x.astype(np.float32), idx


DEGENERATE_CHECKED = ("zero", "negzero", "one-element", "min-2^-94", "max-2^102")
DEGENERATE_OUTSIDE = ("subnormal", "tiny-2^-110", "huge-2^110")


def dead_hidden_weights(name):
    """First layer all-negative with a negative bias: on non-negative inputs every hidden row is zero (here: on |x|, which the tests feed)."""
    flat = golden_weights(name)
    w, b, n_out, n_in = offsets(name)[0][0]
    flat[w:b] = -np.abs(flat[w:b]) - np.float32(1e-3)
    flat[b:b + n_out] = -np.abs(flat[b:b + n_out]) - np.float32(1e-3)
    return flat


def h1_zero_reference(name, flat):
    """f64 outputs of a row whose first hidden row is zero: the later layers' biases alone"""
    z = flat.copy()
    w, b, n_out, n_in = offsets(name)[0][0]
    z[w:b + n_out] = 0.0
    return forward(name, z, np.zeros((1, 153)))[0]


# ---- part D: a layer below the input layer under a 2^0 .. 2^-S spread ------------------------------------------------
SPREAD_CASES = ("DQN-l2", "DQN-head", "D3QN-value-l2", "D3QN-value-head")
SPREAD_N = {"DQN-l2": 64, "DQN-head": 32, "D3QN-value-l2": 64, "D3QN-value-head": 64}   # signed terms per output of the layer under test
SPREAD_BEFORE_AFTER = {"DQN-l2": (1, 1), "DQN-head": (2, 0), "D3QN-value-l2": (1, 1), "D3QN-value-head": (2, 0)}


def spread_problem(n_terms, S, seed=11, n_rows=512):
    """x [n_rows, n_terms] whose elements span 2^0 .. 2^-S (element 0 full scale), eight weight rows: four with an independent spread,
    four adversarial against rows 1..4 (|w_k| = 2^-S / 2^-expo_k with matched signs: every product ~2^-S max|x| max|w|).  The
    construction of test_policy_split_precision_within_row_dynamic_range."""
    rng = np.random.RandomState(seed)
    expo = rng.randint(0, S + 1, size=(n_rows, n_terms)); expo[:, 0] = 0
    sign = rng.choice([-1.0, 1.0], size=(n_rows, n_terms))
    x = (rng.uniform(1.0, 2.0, size=(n_rows, n_terms)) * np.exp2(-expo.astype(np.float64)) * sign).astype(np.float32)
    w = np.zeros((8, n_terms), np.float64)
    wexp = rng.randint(0, S + 1, size=(4, n_terms)); wexp[:, 0] = 0
    w[:4] = rng.uniform(1.0, 2.0, size=(4, n_terms)) * np.exp2(-wexp.astype(np.float64)) * rng.choice([-1.0, 1.0], size=(4, n_terms))
    for o, r in ((4, 1), (5, 2), (6, 3), (7, 4)):
        w[o] = np.exp2((expo[r] - S).astype(np.float64)) * rng.uniform(1.0, 1.25, size=n_terms) * sign[r]
    return x, w.astype(np.float32)


def _assemble(name, mats):
    flat = np.concatenate([np.concatenate([W.reshape(-1), np.zeros(W.shape[0], np.float32)]) for W in mats]).astype(np.float32)
    assert len(flat) == offsets(name)[1]
    return flat


def spread_brains(case, x, w):
    """[(kind name, flat weights, output column)] and the 153-wide observation rows that put the n signed values x[r] and the weight rows w
    on the layer under test.  Pass-through layers carry a signed value v as the pair relu(+v), relu(-v) (unit weights, zero biases: exact
    up to their own split of the row) and the layer after it recombines them.  Output o of brain b estimates  sum_k x[r, k] w[o', k]."""
    n = x.shape[1]
    obs = np.zeros((x.shape[0], 153), np.float32); obs[:, :n] = x
    eye = np.arange(n)
    if case in ("DQN-l2", "DQN-head"):
        W1 = np.zeros((128, 153), np.float32); W2 = np.zeros((64, 128), np.float32); W3 = np.zeros((8, 64), np.float32)
        if case == "DQN-l2":                      # h1 = [relu(x) | relu(-x)] (64 + 64); layer 2 under test: rows 0..7 = +w, 8..15 = -w
            W1[eye, eye] = 1.0; W1[64 + eye, eye] = -1.0
            W2[:8, :64] = w; W2[:8, 64:] = -w; W2[8:16] = -W2[:8]
            W3[np.arange(8), np.arange(8)] = 1.0; W3[np.arange(8), 8 + np.arange(8)] = -1.0
        else:                                     # h1, h2 = [relu(x) | relu(-x)] (32 + 32); the head under test
            W1[eye, eye] = 1.0; W1[32 + eye, eye] = -1.0
            W2[np.arange(64), np.arange(64)] = 1.0
            W3[:, :32] = w; W3[:, 32:] = -w
        return [("DQN", _assemble("DQN", [W1, W2, W3]), None)], obs   # (None: all eight outputs are outputs of the layer under test)
    # dueling, value branch (the advantage head is zero: q_i = (0 + v) - 0 = v exactly).  One weight row per brain: the value is one number.
    brains = []
    for o in range(8):
        W1 = np.zeros((128, 153), np.float32); W1[eye, eye] = 1.0; W1[64 + eye, eye] = -1.0
        A1 = np.zeros((128, 128), np.float32); A2 = np.zeros((8, 128), np.float32)
        V1 = np.zeros((128, 128), np.float32); V2 = np.zeros((1, 128), np.float32)
        if case == "D3QN-value-l2":
            V1[0, :64] = w[o]; V1[0, 64:] = -w[o]; V1[1] = -V1[0]
            V2[0, 0] = 1.0; V2[0, 1] = -1.0
        else:
            V1[np.arange(128), np.arange(128)] = 1.0
            V2[0, :64] = w[o]; V2[0, 64:] = -w[o]
        brains.append(("D3QN", _assemble("D3QN", [W1, A1, A2, V1, V2]), o))
    return brains, obs


def spread_bound(case, x, w):
    """(exact, bound, sum|x w|, max|x| max|w|) per (row, output) -- the bound of test_policy_split_precision_within_row_dynamic_range's
    docstring for the layer under test,
        2^-19 sum_k |x_k w_ok|  +  n 2^-31 max|x| max|w_o|,
    plus what the pass-through layers add by splitting the row again.  A pass-through BEFORE the layer hands it x_k' with
    |x_k' - x_k| <= 2^-21 |x_k| + 2^-31 max|x| (22 bits of the element, bottoming out at the f16 subnormal step against the scaled row
    maximum), which the layer turns into at most 2^-21 sum|x w| + n 2^-31 max|x| max|w_o|; one AFTER it does the same to the result y:
    2^-21 |y| + 2^-31 max_o |y_o|.  Derived from the scheme, not measured."""
    before, after = SPREAD_BEFORE_AFTER[case]
    n = x.shape[1]
    xd, wd = x.astype(np.float64), w.astype(np.float64)
    exact = xd @ wd.T
    mag = np.abs(xd) @ np.abs(wd).T
    scale = np.abs(xd).max(1, keepdims=True) * np.abs(wd).max(1)[None, :]
    own = 2.0 ** -19 * mag + n * 2.0 ** -31 * scale
    if case.endswith("value-l2") or case.endswith("value-head"):
        ymax = np.abs(exact)                       # (one output per brain: the row of the layer behind it holds +-y alone)
    else:
        ymax = np.abs(exact).max(1, keepdims=True)
    bound = own + before * (2.0 ** -21 * mag + n * 2.0 ** -31 * scale) + after * (2.0 ** -21 * np.abs(exact) + 2.0 ** -31 * ymax)
    return exact, bound, mag, scale


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulation of the block-scaled 2 x f16 layer (rl_policy_dev.h: row_scale, split_pair, hi.lo + hi.hi + lo.hi)
# ---------------------------------------------------------------------------------------------------------------------
def _row_scale(mx):
    """2^(10 - exponent(mx)) with the biased exponent clamped to [32, 230], and its inverse (float64 holds both exactly)"""
    mx = np.asarray(mx, np.float32)
    eb = (mx.view(np.int32) >> 23) & 0xff
    eb = np.clip(eb, 32, 230)
    return np.exp2((127 + 10 - eb).astype(np.float64)), np.exp2((eb - 127 - 10).astype(np.float64))


def _split(v, s):
    """v [rows, k] times the per-row power of two s -> (hi, lo) as float64 holding f16 values (both rounded to nearest even)"""
    with np.errstate(over="ignore", invalid="ignore"):
        t = v.astype(np.float64) * s[:, None]
        hi = t.astype(np.float16).astype(np.float64)
        lo = (t - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def emu_layer(x, Wt, b, relu, row_max=None):
    """One layer as the kernels compute it, up to the summation order (products summed in float64, then one rounding to float32).
    row_max(m): hook that replaces the vector of row maxima -- the fault injection."""
    m = np.abs(x).max(axis=1).astype(np.float32)
    if row_max is not None:
        m = row_max(m)
    sx, ux = _row_scale(m)
    xh, xl = _split(x, sx)
    W = np.ascontiguousarray(Wt.T)
    sw, uw = _row_scale(np.abs(W).max(axis=1))
    wh, wl = _split(W, sw)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = (xh @ wh.T + xl @ wh.T + xh @ wl.T).astype(np.float32)
        y = (acc.astype(np.float64) * (uw[None, :] * ux[:, None]) + b.astype(np.float64)[None, :]).astype(np.float32)
    return np.maximum(y, np.float32(0)) if relu else y


def emu_forward(name, flat, x, row_max=None):
    """The Q kinds through emu_layer (PPO's softmax is not needed by any identity)."""
    L = unpack(name, flat, np.float32)
    x = np.ascontiguousarray(x, np.float32)
    if name in ("DQN", "PERDQN"):
        h = emu_layer(x, *L[0], True, row_max)
        h = emu_layer(h, *L[1], True, row_max)
        return emu_layer(h, *L[2], False, row_max)
    f = emu_layer(x, *L[0], True, row_max)
    adv = emu_layer(emu_layer(f, *L[1], True, row_max), *L[2], False, row_max)
    val = emu_layer(emu_layer(f, *L[3], True, row_max), *L[4], False, row_max)
    mean = adv[:, 0].copy()
    for i in range(1, 8):
        mean = mean + adv[:, i]
    mean = mean * np.float32(0.125)
    return (adv + val) - mean[:, None]


def neighbours_maximum(m):
    """the fault of part A: a row scales itself by the larger of its own maximum and its neighbour's in the tile (rows i and i ^ 1)"""
    m = m.copy()
    n = len(m) // 2 * 2
    pair = np.maximum(m[0:n:2], m[1:n:2])
    m[0:n:2] = pair; m[1:n:2] = pair
    return m


# ---------------------------------------------------------------------------------------------------------------------
# the premises, asserted
# ---------------------------------------------------------------------------------------------------------------------
def test_every_golden_row_has_the_same_magnitude_and_the_mixed_rows_do_not():
    g = golden_rows()
    assert g.shape == (640, 153) and np.all(np.abs(g).max(axis=1) == 1.0)       # the blind spot: one magnitude for all 640 rows
    for name in KINDS:
        x, base, k = mixed_rows(name, 640)
        lo, hi = K_RANGE[name]
        assert k.min() >= lo and k.max() <= hi and np.array_equal(x, scaled(base, k))
        assert np.array_equal(np.abs(x).max(axis=1), np.exp2(k.astype(np.float64)))
        for t in range(20):                                                       # neighbouring rows of a tile: dozens of binades apart
            step = np.abs(np.diff(k[32 * t:32 * t + 32]))
            assert step.min() >= (hi - lo) // 3 >= 15, (name, t, step.min())


@pytest.mark.parametrize("name", KINDS)
def test_f32_forward_of_the_mixed_rows_stays_ten_times_inside_the_bar(name, capsys):
    """The condition of the per-row bar (Q kinds: 1e-5 * max_j |ref_ij|; PPO: 1e-5 on the probabilities): a plain numpy f32 forward of the
    same rows is within 1e-6 of the f64 one by the same measure.  PPO's range stops at +6: scaled up further f32 itself leaves the bar."""
    flat = golden_weights(name)
    x, base, k = mixed_rows(name, 640)
    ref = forward(name, flat, x)
    e = err_of(name, forward(name, flat, x, np.float32), ref)
    with capsys.disabled():
        print("\n[mixed rows, f32 numpy vs f64] %s k in [%d, %d]: max %.3g" % ((name,) + K_RANGE[name] + (float(e.max()),)))
    assert np.isfinite(ref).all() and e.max() <= F32_MARGIN, (name, float(e.max()))


def test_ppo_scaled_up_is_where_f32_itself_leaves_the_bar():
    """Why PPO's exponents stop at +6: at +-12 the f32 forward is already further than 1e-6 from f64 (so the GPU bar would not be fair)."""
    flat = golden_weights("PPO")
    base = golden_rows()
    x = scaled(base, mixed_exponents(640, -12, 12, seed=1))
    e = err_of("PPO", forward("PPO", flat, x, np.float32), forward("PPO", flat, x))
    assert e.max() > F32_MARGIN


@pytest.mark.parametrize("name", Q_KINDS)
def test_power_of_two_equivariance_holds_bit_for_bit_in_f32_and_in_the_emulated_scheme(name):
    """Zero biases: forward(2^k_i x_i) == 2^k_i forward(x_i) exactly -- for the numpy f32 forward (every scale is a power of two and
    nothing goes subnormal: min |q| of the unscaled rows is ~2e-6 > 2^-126 * 2^40) and for the emulation of the 2 x f16 scheme.  Fed a
    neighbour's row maximum the emulation breaks the identity AND the per-row bar, while on the unscaled golden rows (all maxima 1.0) the
    same fault changes nothing: the suite could not see it before."""
    flat = zero_biases(name, golden_weights(name))
    x, base, k = mixed_rows(name, 640)
    q0 = forward(name, flat, base, np.float32)
    assert np.abs(q0).min() > 1e-7
    # (numpy's sgemm sums a row's products in an order that depends on the row's position in the batch, not on its values: same batch shape)
    assert np.array_equal(forward(name, flat, x, np.float32), scaled(q0, k))
    e0 = emu_forward(name, flat, base)
    ex = emu_forward(name, flat, x)
    assert np.array_equal(ex, scaled(e0, k))
    ref = forward(name, flat, x)
    assert row_err(ex, ref).max() <= ROW_BAR
    # the fault: invisible on rows of one magnitude, visible on mixed rows both ways
    assert np.array_equal(emu_forward(name, flat, base, neighbours_maximum), e0)
    bad = emu_forward(name, flat, x, neighbours_maximum)
    assert not np.array_equal(bad, scaled(e0, k))
    assert row_err(bad, ref).max() > ROW_BAR


@pytest.mark.parametrize("over", [5, 8])
def test_an_overestimated_row_maximum_passes_the_bar_but_not_the_identity(over):
    """A row maximum too large by 2^5 or 2^8 (a partial maximum of another row out of the LDS exchange) only pushes the low parts of the
    smaller elements under the f16 subnormal step: the 1e-5 bar does not see it -- the blind spot -- but the bit-exact identities do, once
    rows differ: here every ODD row overestimates.  (Too large by 2^1 changes nothing at all: f16 is a floating-point format.)"""
    name = "DQN"
    flat = zero_biases(name, golden_weights(name))
    x, base, k = mixed_rows(name, 640)

    def fault(m):
        m = m.copy(); m[1::2] = np.ldexp(m[1::2], over); return m
    good, bad = emu_forward(name, flat, x), emu_forward(name, flat, x, fault)
    assert row_err(bad, forward(name, flat, x)).max() <= ROW_BAR
    assert not np.array_equal(good, bad)


@pytest.mark.parametrize("name", KINDS)
@pytest.mark.parametrize("k", [-30, 30])
def test_a_first_layer_scaled_by_a_power_of_two_packs_to_the_same_planes(name, k):
    """Brain B = brain A with layer 1 times 2^k, biases zeroed in both: rl_policy_pack_weights gives B the f16 planes of A everywhere, the
    unscale constants of layer 1 times 2^k, and nothing else differs."""
    from reinlife_amd import _lib
    lib = _lib.lib()
    kind = _lib.KIND_BY_METHOD[name]
    A = zero_biases(name, golden_weights(name))
    B = scale_layer1(name, A, k)
    packs = []
    for flat in (A, B):
        p = np.zeros(lib.rl_policy_packed_floats(kind), np.float32)
        assert lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)) == 0
        packs.append(p)
    pa, pb = packs
    tout = SHAPES[name][0][0] // 32
    frag = 10 * tout * 2 * 64 * 4                                   # frag_floats(kInChunks, tout)
    assert np.array_equal(pa[:frag].view(np.uint32), pb[:frag].view(np.uint32)) and np.any(pa[:frag].view(np.uint32))
    ca, cb = pa[frag:frag + tout * 64].reshape(tout * 2, 2, 16), pb[frag:frag + tout * 64].reshape(tout * 2, 2, 16)
    assert np.array_equal(cb[:, 0], np.ldexp(ca[:, 0], k)) and np.all(ca[:, 0] > 0)      # unscale
    assert np.all(ca[:, 1] == 0) and np.all(cb[:, 1] == 0)                               # bias
    assert np.array_equal(pa[frag + tout * 64:].view(np.uint32), pb[frag + tout * 64:].view(np.uint32))
    # the f32 forward of B is 2^k times that of A, bit for bit (PPO: the same probabilities only where the logits are; not claimed)
    if name != "PPO":
        x = golden_rows()
        assert np.array_equal(forward(name, B, x, np.float32), np.ldexp(forward(name, A, x, np.float32), k))


@pytest.mark.parametrize("name", ["DQN", "D3QN", "PERD3QN", "PERDQN"])
def test_tied_heads_tie_every_row_and_cover_the_answers(name):
    """Per arrangement every one of the 640 rows has its maximum in a tied group (>= 200 is what the GPU test needs), the f32 forwards
    (numpy sgemm and the C oracle's scalar one) give bit-equal duplicates, the expected answers cover 0 .. 6 over the arrangements, and
    an argmax written with `>=` gets every one of those rows wrong."""
    from oracle import oracle as orc
    x = golden_rows()
    seen = set()
    for p, pattern in TIE_PATTERNS.items():
        flat = tied_weights(name, pattern, seed=5)
        ref = forward(name, flat, x, np.float32)
        want, gap = tie_expected(ref, pattern)
        if name in orc.KIND_BY_NAME:
            ora = orc.policy_forward(orc.KIND_BY_NAME[name], flat, x)
            tie_expected(ora, pattern)                               # (asserts the duplicates are bit-equal)
        tied = (ref == ref.max(axis=1, keepdims=True)).sum(axis=1) >= 2
        assert tied.sum() >= 200 and tied.all()
        clear = gap >= 1e-5
        assert clear.sum() >= 600
        assert np.array_equal(argmax_first(ref), want) and np.array_equal(ref.argmax(axis=1), want)
        assert (argmax_last(ref) != want).all()
        seen |= set(want[clear].tolist())
        for v in group_firsts(pattern):
            assert (want[clear] == v).sum() >= 20, (p, v)            # every group wins on some rows
    assert seen == set(range(7)), seen
    flat = tied_weights(name, None, seed=5, all_equal=True)
    ref = forward(name, flat, x, np.float32)
    assert np.all(ref == ref[:, :1]) and np.all(argmax_first(ref) == 0) and np.all(argmax_last(ref) == 7)


def test_the_golden_heads_copied_in_place_would_not_do():
    """Why the tied rows are fresh draws: with rows of the golden DQN head copied in place one action wins nearly every row."""
    flat = golden_weights("DQN")
    w, b, n_out, n_in = offsets("DQN")[0][2]
    W = flat[w:b].reshape(8, 64).copy(); bias = flat[b:b + 8].copy()
    pat = [0, 1, 1, 3, 3, 3, 0, 7]
    flat[w:b] = W[pat].reshape(-1); flat[b:b + 8] = bias[pat]
    hist = np.bincount(forward("DQN", flat, golden_rows(), np.float32).argmax(axis=1), minlength=8)
    assert hist.max() >= 630


def test_saturated_ppo_is_one_hot_in_f64():
    flat, hot = saturated_ppo()
    p = forward("PPO", flat, golden_rows())
    assert np.all(p[np.arange(640), hot] == 1.0) and np.all(np.delete(p, 0, axis=1).shape == (640, 7))
    assert np.all(np.sort(p, axis=1)[:, :7] == 0.0)
    assert len(set(hot.tolist())) >= 3


def test_degenerate_tile_premises():
    x, idx = degenerate_tile()
    mx = np.abs(x).max(axis=1)
    assert mx[idx["zero"]] == 0 and mx[idx["negzero"]] == 0 and np.all(np.signbit(x[idx["negzero"]]))
    assert np.count_nonzero(x[idx["one-element"]]) == 1
    assert mx[idx["min-2^-94"]] == 2.0 ** -94 and mx[idx["max-2^102"]] == 2.0 ** 102
    assert 2.0 ** CLAMP_LO <= mx[idx["min-2^-94"]] and mx[idx["max-2^102"]] < 2.0 ** (CLAMP_HI + 1)
    assert 0 < mx[idx["subnormal"]] < 2.0 ** -126 and mx[idx["tiny-2^-110"]] < 2.0 ** CLAMP_LO and mx[idx["huge-2^110"]] > 2.0 ** CLAMP_HI
    # the clamp of row_scale: biased exponents 32 and 230 are 2^-95 and 2^103
    s, u = _row_scale(np.array([0.0, 2.0 ** -95, 2.0 ** -120, 2.0 ** 103, 2.0 ** 120], np.float32))
    assert np.array_equal(s, np.exp2([105.0, 105.0, 105.0, -93.0, -93.0])) and np.array_equal(s * u, np.ones(5))
    for name in KINDS:
        flat = golden_weights(name)
        ref = forward(name, flat, x)
        assert np.isfinite(ref[[idx[k] for k in DEGENERATE_CHECKED]]).all()
        # zero inputs: the biases alone
        L = unpack(name, flat)
        h = np.maximum(L[0][1], 0.0)
        if name in ("DQN", "PERDQN"):
            want = np.maximum(h @ L[1][0] + L[1][1], 0) @ L[2][0] + L[2][1]
            assert np.allclose(ref[idx["zero"]], want, rtol=1e-12, atol=0) and np.array_equal(ref[idx["zero"]], ref[idx["negzero"]])
        # dead hidden rows: what is left does not depend on the input
        dead = dead_hidden_weights(name)
        out = forward(name, dead, np.abs(x[:3]))
        assert np.array_equal(out[0], out[1]) and np.allclose(out[0], h1_zero_reference(name, dead), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("case", SPREAD_CASES)
def test_spread_brains_compute_the_layer_under_test(case):
    """The pass-through construction of part D in float64: the brains' outputs ARE sum_k x_k w_ok of the layer under test."""
    x, w = spread_problem(SPREAD_N[case], 20)
    brains, obs = spread_brains(case, x, w)
    exact, bound, mag, scale = spread_bound(case, x, w)
    for name, flat, o in brains:
        out = forward(name, flat, obs)
        got = out if o is None else out[:, o:o + 1]
        want = exact if o is None else exact[:, o:o + 1]
        assert np.abs(got - want).max() <= 1e-12 * np.abs(scale).max(), case
        if o is not None:
            assert np.all(out == out[:, :1])                       # q_i = v for every action
    adv = np.abs(exact[[1, 2, 3, 4], [4, 5, 6, 7]])
    assert adv.max() < SPREAD_N[case] * 2.5 * 2.0 ** -20 and scale.min() >= 2.0 ** -20   # the adversarial outputs: every product < 2.5 * 2^-20


def test_policy_check_tie_groups_only_tightens():
    """tests/policy_check.PolicyCheck(tie_groups=...): a flip between members of one tied group is no longer excused by the zero top-2 gap
    (the gap that counts is the one between distinct groups); without the argument the helper accepts what it accepted."""
    from oracle import oracle as orc
    from policy_check import PolicyCheck
    pattern = TIE_PATTERNS["034"]
    flat = tied_weights("DQN", pattern, seed=5)

    class FakeWorlds:
        pass
    ow = FakeWorlds()
    x = golden_rows()[:96]
    ow.obs2 = x.reshape(1, 96, 153).copy()
    ow.s = dict(n_agents=np.array([96], np.int32), a_brain=np.zeros((1, 96), np.int8), tick=np.zeros(1, np.int32), epoch=np.zeros(1, np.int32))
    ow.cfg = orc.OracleWorlds(n_worlds=1, width=5, height=5, max_agents=4, n_brains=1).cfg
    ref = forward("DQN", flat, x, np.float32)
    good = argmax_first(ref).astype(np.int8).reshape(1, 96)
    last = argmax_last(ref).astype(np.int8).reshape(1, 96)
    for groups, acts, ok in ((None, good, True), ([pattern], good, True), (None, last, True), ([pattern], last, False)):
        pc = PolicyCheck(["DQN"], [flat], [0.0], tie_groups=groups) if groups else PolicyCheck(["DQN"], [flat], [0.0])
        pc.before(ow)
        if ok:
            pc.after(acts)
        else:
            with pytest.raises(AssertionError):
                pc.after(acts)
