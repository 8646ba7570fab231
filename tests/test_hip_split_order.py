"""GPU: the f16 hi / lo split dealt stage by stage, the weight ring requested in reverse and the epilogue constants requested bias first
(k_run's certified one-wave dueling tile).  The new order issues the same instructions on the same operands, so every
comparison here is exact.

Stand-alone policy (rl_policy_forward, the tiles that keep the pair-by-pair order), one brain of each dueling kind, at 1 / 32 / 33 rows:
the three variants agree by np.array_equal and every row is within the project's bar of a float64 forward (oracle/cpu_bench.forward, as
tests/test_hip_policy_rows.py).  Rows: mixed magnitudes inside one tile, exact ties (a head whose outputs are tied), all-zero and
single-nonzero rows, and brains whose first input-layer unit is scaled by 2^16 / 2^40 -- a power-of-two scaling of the ROW moves every
activation alike (the scheme is exactly equivariant), so what puts the other 127 activations of a row 2^-16 / 2^-40 below the row's maximum
is the unit's weights: scaled by the row's scale 2^10 / max they lie below 2^-3, where the `lo` half of the hidden layer's split is an f16
subnormal (below 2^-14), and below 2^-25, where both halves are exactly zero.  The premises are asserted on a float64 forward.

k_run: 3 worlds of 8 x 8 cells, max_agents 40, two PERD3QN brains -- world 0 gives brain 0 exactly 33 agents (two tiles of one brain, the
second with one valid row), world 2 gives brain 1 none.  12 ticks in launches of 1, 5 and 6: TRAIN 0 and TRAIN 1 against the two-launch
loop (states, actions, rewards, done flags, Agent.state rows), TRAIN 2's policy_out against rl_policy_forward of the rows the tick read,
all by np.array_equal; once more with adversarial brains, whose certified tiles fail their certificate, so that the cold full tile runs
between hot ones.  On the product library and on the tuning library, whose counters show that the certified finish ran / fell back.
World, brain and comparison helpers: tests/test_hip_weight_lookahead.py (its script text up to `case`), builders: tests/test_policy_rows_cpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_hip_weight_lookahead as wl
import test_policy_rows_cpu as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 32, 33)
VARIANTS = ("pair", "dense", "wave")


# ---------------------------------------------------------------------------------------------------------------------
# stand-alone policy
# ---------------------------------------------------------------------------------------------------------------------
def _rows33(name):
    """33 rows: mixed magnitudes (neighbours dozens of binades apart), an all-zero row, a -0 row and a single-nonzero row among them;
    row 32 (the one valid row of the second tile) is an ordinary scaled row."""
    x, _, _ = pr.mixed_rows(name, 33, seed=33)
    x[3] = 0.0
    x[6] = -0.0
    x[9] = 0.0; x[9, 100] = -0.75
    x[20] = 0.0; x[20, 152] = np.float32(2.0 ** -30)
    return x


def _hidden(name, flat, x):
    L = pr.unpack(name, flat)
    return np.maximum(x.astype(np.float64) @ L[0][0] + L[0][1], 0)


def _spread_brain(name, K):
    """golden weights with input-layer unit j0 (weights and bias) times 2^K, j0 = the unit whose smallest activation over the first 33
    golden rows is largest.  Returns (flat, rows, j0)."""
    flat = pr.golden_weights(name)
    x = pr.golden_rows()[:33].copy()
    h = _hidden(name, flat, x)
    j0 = int(h.min(axis=0).argmax())
    assert h[:, j0].min() > 0
    w, b, n_out, n_in = pr.offsets(name)[0][0]
    flat[w + j0 * n_in:w + (j0 + 1) * n_in] = np.ldexp(flat[w + j0 * n_in:w + (j0 + 1) * n_in], K)
    flat[b + j0] = np.ldexp(flat[b + j0], K)
    return flat, x, j0


def _scaled_activations(name, flat, x):
    """the hidden layer's input as the split sees it: activation times 2^(10 - exponent of the row's maximum)"""
    h = _hidden(name, flat, x)
    return h * np.ldexp(1.0, 10 - np.floor(np.log2(h.max(axis=1))).astype(np.int64))[:, None]


def _check(name, flat, x, hip_option, tied=None):
    from test_hip_policy_rows import _Fwd, _same
    f = _Fwd(name, flat, hip_option)
    worst = 0.0
    for n in SIZES:
        xs = x[:n]
        ref = pr.forward(name, flat, xs)
        outs = [f(xs, v) for v in VARIANTS]
        for v, out in zip(VARIANTS[1:], outs[1:]):
            assert _same(out, outs[0]), (name, n, v)
        e = pr.err_of(name, outs[0], ref)
        worst = max(worst, float(e.max()))
        assert np.isfinite(outs[0]).all() and e.max() <= pr.ROW_BAR, (name, n, float(e.max()), int(e.argmax()))
        if tied is not None:
            for i, g in enumerate(tied):
                assert _same(outs[0][:, i], outs[0][:, tied.index(g)]), (name, n, i)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", pr.DUELING)
def test_standalone_variants_agree_on_mixed_zero_and_single_nonzero_rows(name, hip_option, capsys):
    worst = _check(name, pr.golden_weights(name), _rows33(name), hip_option)
    with capsys.disabled():
        print("\n[split order] %s mixed / zero / single-nonzero rows: max per-row error vs f64 %.3g (bar 1e-5)" % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", pr.DUELING)
def test_standalone_variants_agree_on_exact_ties(name, hip_option):
    """A head whose eight outputs copy three distinct rows (pattern 0 1 2 0 1 2 0 1): every row's maximum is tied, the tied outputs are the
    same bits in every variant."""
    pattern = pr.TIE_PATTERNS["012"]
    _check(name, pr.tied_weights(name, pattern, seed=5), _rows33(name), hip_option, tied=list(pattern))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [16, 40], ids=["lo-subnormal", "halves-zero"])
@pytest.mark.parametrize("name", pr.DUELING)
def test_standalone_variants_agree_where_the_hidden_split_leaves_the_normal_range(name, K, hip_option, capsys):
    flat, x, j0 = _spread_brain(name, K)
    s = _scaled_activations(name, flat, x)
    others = np.delete(s, j0, axis=1)
    assert (s.argmax(axis=1) == j0).all() and ((s[:, j0] >= 2.0 ** 10) & (s[:, j0] < 2.0 ** 11)).all()
    live = others > 0
    assert live.sum() > 33 * 20                                       # (a fair share of the 127 other units is active in every batch)
    if K == 16:   # scaled value in [2^-14, 2^-3): hi is a normal f16, lo (at most half an ulp of hi: below 2^-14) a subnormal one or zero
        assert (live & (others < 2.0 ** -3) & (others >= 2.0 ** -14)).sum() > 33 * 20 and (others < 2.0 ** -3).all()
    else:         # scaled value below 2^-25: half the smallest f16 subnormal -- hi and lo are exactly zero
        assert (others < 2.0 ** -25).all()
    worst = _check(name, flat, x, hip_option)
    with capsys.disabled():
        print("\n[split order] %s unit %d x 2^%d: max per-row error vs f64 %.3g (bar 1e-5)" % (name, j0, K, worst))


# ---------------------------------------------------------------------------------------------------------------------
# k_run
# ---------------------------------------------------------------------------------------------------------------------
CASE = r'''
THR, N_NEW, EPS, CHUNKS = 30, 36, [0.0, 0.05], (1, 5, 6)

def make2(adv):
    dw = DeviceWorlds(n_worlds=3, width=8, height=8, max_agents=40, n_brains=2, static_families=True, limit_reproduction=False,
                      incentivize_killing=True, seed=53, world_base=3, device="cuda:0")
    flats = [adversarial(300 + k) if k in adv else bench.brain_weights("PERD3QN", 900 + k).astype(np.float32) for k in range(2)]
    packed = [pack_brain_weights(_lib.PERD3QN, w, "cuda:0") for w in flats]
    dw.set_brains([(_lib.PERD3QN, EPS[k], packed[k]) for k in range(2)])
    dw.reset_synthetic(N_NEW)
    torch.cuda.synchronize()
    n = dw.s["n_agents"].cpu().numpy()
    br = dw.s["a_brain"].cpu().numpy().copy()
    assert n.min() >= 34
    br[0, :n[0]] = 1; br[0, :33] = 0        # brain 0: 33 agents = two tiles, the second with ONE valid row
    br[2, :n[2]] = 0                        # brain 1 has no agents
    dw.s["a_brain"].copy_(torch.as_tensor(br, device="cuda:0"))
    torch.cuda.synchronize()
    _lib.check(lib.rl_bind_state(dw.handle, ctypes.byref(dw._state)), "rl_bind_state")
    dw.packed2 = packed
    return dw

def run2(adv):
    have_counters = hasattr(lib, "rl_debug_cert_counters")
    res = dict(adv=adv, have_counters=have_counters, diff={}, q_rows=0, q_diff=[], first_rows=None, ticks=0)
    sched = lambda n: np.ascontiguousarray(np.array(EPS, np.float32)[None, :].repeat(n, 0))   # noqa: E731
    t0, t1, t2, loop = make2(adv), make2(adv), make2(adv), make2(adv)
    assert t0.run_supported()
    t1.enable_tracking(True)
    res["first_rows"] = rows(loop).tolist()
    got = [0, 0, 0]
    if have_counters:
        counters()
    for n in CHUNKS:
        t0.run(n, THR, N_NEW)
        a0 = snap(t0)
        if have_counters:
            got = [x + y for x, y in zip(got, counters())]
        t1.run(n, THR, N_NEW, eps_schedule=sched(n), trk_skip=1)
        a1 = snap(t1)
        t2.run(n, THR, N_NEW, want_q=True)
        torch.cuda.synchronize()
        t2.check_error_flag()
        for i in range(n):
            if i == n - 1:   # what the chunk's last policy half reads
                torch.cuda.synchronize()
                obs = loop.obs_state().cpu().numpy().copy()
                cnt = loop.s["n_agents"].cpu().numpy().copy()
                br = loop.s["a_brain"].cpu().numpy().copy()
            loop._set_epsilons(EPS)
            loop.act(); loop.tick_refill(THR, N_NEW)
        l = snap(loop)
        res["diff"]["%%d:train0" %% res["ticks"]] = differ(a0, l)
        res["diff"]["%%d:train1" %% res["ticks"]] = differ(a1, l)
        q = t2.out_q.cpu().numpy()
        for w in range(3):
            for b in range(2):
                ks = np.nonzero(br[w, :cnt[w]] == b)[0]
                if len(ks) == 0:
                    continue
                x = torch.zeros((len(ks) + 1, 153), dtype=torch.float32, device="cuda:0")
                x[:len(ks)] = torch.from_numpy(np.ascontiguousarray(obs[w, ks, :153], np.float32))
                out = torch.full((len(ks), 8), float("nan"), device="cuda:0")
                policy_forward(_lib.PERD3QN, t2.packed2[b], x[:len(ks)], out)
                torch.cuda.synchronize()
                res["q_rows"] += len(ks)
                if not np.array_equal(out.cpu().numpy().view(np.uint32), np.ascontiguousarray(q[w, ks]).view(np.uint32)):
                    res["q_diff"].append("%%d:w%%d:b%%d" %% (res["ticks"], w, b))
        res["ticks"] += n
    res["counters"] = got
    print("RESULT " + json.dumps(res), flush=True)

from reinlife_amd.worlds import policy_forward
run2(%(adv)r)
'''


def _k_run(which, adv):
    from reinlife_amd import build
    env = dict(os.environ)
    env.pop("RL_TUNE", None)
    if which == "tuning":
        if not os.path.exists(build.TUNE_LIB_PATH):
            pytest.skip("the tuning library is not built (RL_TUNE=1 python reinlife_amd/build.py; __graft_entry__.build() builds it)")
        env["REINLIFE_HIP_LIB"] = build.TUNE_LIB_PATH
    else:
        env.pop("REINLIFE_HIP_LIB", None)
    script = (wl.SCRIPT.split("def case(")[0] + CASE) % dict(root=ROOT, adv=adv)
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = [json.loads(line[len("RESULT "):]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    assert len(res) == 1
    r = res[0]
    print(r)
    assert r["ticks"] == 12, r
    assert r["first_rows"][0] == [33, r["first_rows"][0][1]] and r["first_rows"][0][1] >= 1 and r["first_rows"][2][1] == 0, r
    assert all(v == [] for v in r["diff"].values()) and len(r["diff"]) == 6, r   # TRAIN 0 / TRAIN 1 against act + tick_refill
    assert r["q_diff"] == [] and r["q_rows"] >= 3 * 34, r                        # TRAIN 2 against rl_policy_forward
    assert r["have_counters"] == (which == "tuning"), r
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["product", "tuning"])
def test_k_run_equals_the_two_launch_loop_and_the_standalone_policy(which):
    r = _k_run(which, [])
    if which == "tuning":
        assert r["counters"][1] > 0, r    # rows were certified: the hot tile finished them


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["product", "tuning"])
def test_k_run_with_adversarial_brains_runs_the_cold_tile_between_hot_ones(which):
    """Brain 0 adversarial and greedy (advantages one ulp apart, b_v = 300): its tiles store nothing and are run again as the full tile,
    brain 1's tiles stay hot."""
    r = _k_run(which, [0])
    if which == "tuning":
        assert r["counters"][2] > 0 and r["counters"][1] > 0, r
