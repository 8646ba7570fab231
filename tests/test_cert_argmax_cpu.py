"""The certified argmax of the dueling finish (rl_policy_dev.h tile1_finish_cert), emulated in numpy float32 in the kernel's
order of operations: wherever the certificate holds, the first argmax of the advantages is the first argmax of q = fl(fl(a + v) - m) --
over millions of rows, values of v across many decades, near-ties built with nextafter, and the NaN / Inf rows."""
import numpy as np

F = np.float32


def full_action(a, v):
    """tile1_finish: m = (((a0 + a1) + ...) + a7) * 0.125, q_i = (a_i + v) - m, first maximum (q[i] > best)."""
    m = a[:, 0].copy()
    for i in range(1, 8):
        m = m + a[:, i]
    m = m * F(0.125)
    q = (a + v[:, None]) - m[:, None]
    return first_max(q)


def first_max(x):
    best = x[:, 0].copy()
    idx = np.zeros(len(x), np.int64)
    for i in range(1, 8):
        gt = x[:, i] > best
        idx = np.where(gt, i, idx)
        best = np.where(gt, x[:, i], best)
    return idx, best


def certify(a, vbar):
    """tile1_finish_cert: i* = first argmax of a; certified when every j < i* has fl(a_i* - a_j) > thr."""
    istar, best = first_max(a)
    amax = np.abs(a[:, 0])
    s = a[:, 0].copy()
    for i in range(1, 8):
        amax = np.fmax(amax, np.abs(a[:, i]))
        s = s + a[:, i]
    thr = F(2.0 ** -20) * (((amax + amax) + vbar) + F(2.0 ** -80)) + (s - s)
    ok = np.ones(len(a), bool)
    for j in range(7):
        ok &= (j >= istar) | ((best - a[:, j]) > thr)
    return istar, ok


def check(a, v, vbar):
    with np.errstate(all="ignore"):
        want, _ = full_action(a, v)
        istar, ok = certify(a, vbar)
    bad = ok & (istar != want)
    assert not bad.any(), (a[bad][:3], v[bad][:3], istar[bad][:3], want[bad][:3])
    return ok


def rows(rng, n, scale):
    return (rng.standard_normal((n, 8)) * scale).astype(F)


def test_certified_rows_pick_the_full_paths_action():
    rng = np.random.default_rng(5)
    total = certified = 0
    for it in range(40):
        n = 100_000
        a = rows(rng, n, F(10.0) ** rng.uniform(-6, 4, (n, 1)).astype(F))
        v = (rng.standard_normal(n) * F(10.0) ** rng.uniform(-8, 8, n)).astype(F)
        for vbar in (np.abs(v), (np.abs(v) * F(1.0 + 2.0 ** -8)).astype(F), (np.abs(v) * F(3.0)).astype(F)):
            ok = check(a, v, vbar)
            total += n
            certified += int(ok.sum())
    assert certified > 0.5 * total   # (v up to 1e8 against advantages down to 1e-6: many rows honestly fall back)


def test_near_ties_merged_by_a_large_value():
    """Advantages a few ulps apart: a large v merges them in q, and the certificate must refuse exactly those rows (or be right)."""
    rng = np.random.default_rng(6)
    fell_back = 0
    for it in range(30):
        n = 100_000
        a = rows(rng, n, F(1.0))
        j = rng.integers(0, 7, n)
        k = rng.integers(1, 8, n)
        k = np.where(k <= j, j + 1, k)
        k = np.minimum(k, 7)
        top = np.max(np.abs(a), axis=1) + F(1.0)
        a[np.arange(n), k] = top
        steps = rng.integers(0, 6, n)
        lo = top.copy()
        for s in range(6):
            lo = np.where(steps > s, np.nextafter(lo, F(-np.inf)), lo)
        a[np.arange(n), j] = lo   # a_j <= a_k, a few ulps apart, j < k
        v = (rng.choice([-1, 1], n) * F(10.0) ** rng.uniform(-3, 6, n)).astype(F)
        ok = check(a, v, np.abs(v))
        fell_back += int((~ok).sum())
    assert fell_back > 0   # the rule did have to refuse some rows


def test_first_argmax_at_zero_is_always_certified_and_nan_inf_fall_back():
    a = np.zeros((8, 8), F)
    v = np.zeros(8, F)
    a[0] = [5, 1, 2, 3, 4, 0, 0, 0]                          # i* == 0: certified whatever the bound
    a[1] = [np.nan, 1, 2, 3, 4, 0, 0, 0]                     # NaN at 0: i* == 0, the full path picks 0 too
    a[2] = [5, 1, np.nan, 3, 4, 0, 0, 0]                     # i* == 0 again (the full path: every q NaN -> 0)
    a[3] = [1, 2, np.nan, 3, 4, 0, 0, 0]                     # NaN elsewhere, i* > 0: must fall back
    a[4] = [1, 2, np.inf, 3, 4, 0, 0, 0]                     # +Inf: falls back
    a[5] = [1, -np.inf, 2, 3, 4, 0, 0, 0]                    # -Inf: falls back
    a[6] = [1, 2, 3, 4, 5, 0, 0, 0]                          # ordinary row
    a[7] = [1, 2, 3, 4, 5, 0, 0, 0]
    vbar = np.array([np.nan, 0, 0, 0, 0, 0, np.nan, np.inf], F)   # NaN / Inf bounds fall back unless i* == 0
    ok = check(a, v, vbar)
    assert list(ok) == [True, True, True, False, False, False, False, False]
    ok = check(a, v, np.zeros(8, F))
    assert ok[0] and ok[1] and ok[2] and not ok[3] and not ok[4] and not ok[5] and ok[6] and ok[7]

