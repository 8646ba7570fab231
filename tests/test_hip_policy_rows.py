"""GPU: the policy tiles on rows the rest of the suite never feeds them -- rows of different magnitude inside one 32-row tile, exact ties,
degenerate rows, and a within-row spread below the input layer.  Builders, references and every premise: tests/test_policy_rows_cpu.py.

Every numeric check is against a float64 forward (oracle/cpu_bench.forward on float64 layers), per row:
    Q kinds  |out - ref64| <= 1e-5 * max_j |ref64_ij|        PPO  |p - p64| <= 1e-5
(the project's bar, applied per row; a numpy f32 forward of the same rows stays within 1e-6, asserted on the CPU).  Every identity that the
scheme makes exact -- row permutation, position in the batch, tile variant, power-of-two scaling of a row or of a weight layer, duplicated
outputs -- is asserted with np.array_equal.  Each docstring says which fault the test would catch; the CPU companion demonstrates the two
cheap ones on an emulation of the scheme (a neighbour's row maximum; `>=` in the argmax)."""
import ctypes as C

import numpy as np
import pytest

import test_policy_rows_cpu as pr

pytestmark = pytest.mark.gpu
AUTO_ROWS = 1536 * 32 + 128          # from 1,536 tiles on `auto` picks k_policy_dense for the dueling kinds


def _kind(name):
    from reinlife_amd import _lib
    return _lib.KIND_BY_METHOD[name]


def _variants(name):
    return ["pair", "dense", "wave"] if name in pr.DUELING else ["pair"]


class _Fwd:
    """rl_policy_forward of one brain under a policy_variant; the rows live in a buffer one row longer than the batch (the kernels read
    16 bytes at a time)."""
    def __init__(self, name, flat, hip_option):
        from reinlife_amd.worlds import pack_brain_weights
        self.name, self.kind, self.opt = name, _kind(name), hip_option
        self.packed = pack_brain_weights(self.kind, flat)

    def __call__(self, x, variant="pair"):
        import torch
        from reinlife_amd.worlds import policy_forward
        self.opt("policy_variant", variant)
        n = x.shape[0]
        buf = torch.zeros((n + 1, 153), dtype=torch.float32, device="cuda:0")
        buf[:n] = torch.from_numpy(np.ascontiguousarray(x, np.float32))
        out = torch.full((n, 8), float("nan"), device="cuda:0")
        policy_forward(self.kind, self.packed, buf[:n], out)
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# A. rows of different magnitude in one tile
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.KINDS)
def test_mixed_magnitude_rows_meet_the_bar_per_row(name, hip_option, capsys):
    """Golden rows times 2^k_i, k_i in [-40, 40] (PPO: [-40, 6]), neighbours dozens of binades apart, at 1 / 31 / 32 / 33 / 640 rows, a
    shuffled 4,480 (35 workgroups of the pair kernel) and, under `auto`, 49,280 rows (the dense kernel) -- against float64, PER ROW.
    Fault: a row scaled by anything but its own maximum (a partial maximum of another row from the LDS exchange, a tile-wide maximum): it
    costs the smaller row its bits or overflows f16 -- the CPU companion shows the per-row error of such a kernel far beyond 1e-5, while
    the same fault is invisible on the unscaled golden rows."""
    flat = pr.golden_weights(name)
    f = _Fwd(name, flat, hip_option)
    rng = np.random.RandomState(3)
    worst = 0.0
    for n, variants in [(n, _variants(name)) for n in (1, 31, 32, 33, 640, 4480)] + [(AUTO_ROWS, ["auto"])]:
        x, _, k = pr.mixed_rows(name, n, seed=n)
        if n > 640:
            x = x[rng.permutation(n)]
        ref = pr.forward(name, flat, x)
        for v in variants:
            out = f(x, v)
            e = pr.err_of(name, out, ref)
            worst = max(worst, float(e.max()))
            assert np.isfinite(out).all() and e.max() <= pr.ROW_BAR, (name, n, v, float(e.max()), int(e.argmax()))
    with capsys.disabled():
        print("\n[mixed rows] %s: max per-row error vs f64 %.3g (bar 1e-5)" % (name, worst))


@pytest.mark.parametrize("name", pr.KINDS)
def test_a_rows_result_depends_on_nothing_but_the_row(name, hip_option):
    """forward(P X) == P forward(X) for a random permutation of 4,480 mixed-magnitude rows; the same 640 rows at offsets 0, 7 and 1,003 of
    a larger batch (another tile, another lane, another workgroup); every variant, and `auto` on a batch large enough for the dense
    kernel: the same bits.  Fault: anything a row inherits from its tile -- a shared scale, a neighbour's exchange slot, a lane-dependent
    summation order."""
    flat = pr.golden_weights(name)
    f = _Fwd(name, flat, hip_option)
    x, _, _ = pr.mixed_rows(name, 4480, seed=9)
    base = f(x, "pair")
    perm = np.random.RandomState(4).permutation(len(x))
    for v in _variants(name):
        assert _same(f(x[perm], v), base[perm]), (name, v, "permutation")
        assert _same(f(x, v), base), (name, v, "variant")
    other, _, _ = pr.mixed_rows(name, 2000, seed=10)
    big = np.concatenate([other[:7], x[:640], other[7:7 + 1003 - 647], x[:640], other[400:437]])
    assert np.array_equal(big[7:647], x[:640]) and np.array_equal(big[1003:1643], x[:640])
    for v in _variants(name):
        out = f(big, v)
        assert _same(out[7:647], base[:640]) and _same(out[1003:1643], base[:640]), (name, v, "offset")
    huge = np.concatenate([x] * (AUTO_ROWS // len(x) + 1))
    out = f(huge, "auto")
    for r in range(len(huge) // len(x)):
        assert _same(out[r * len(x):(r + 1) * len(x)], base), (name, "auto", r)


@pytest.mark.parametrize("name", pr.Q_KINDS)
def test_scaling_a_row_by_a_power_of_two_scales_its_outputs_bit_for_bit(name, hip_option):
    """Biases zeroed: forward(2^k_i x_i) == 2^k_i forward(x_i) exactly, k_i in [-40, 40] per row.  Every scale in the scheme is a power of
    two and the split sees the same scaled values, so nothing but a wrong row maximum can break this (the numpy f32 forward and the
    emulated scheme satisfy it on these rows: CPU companion, which also shows a maximum overestimated by 2^5 -- invisible to the 1e-5
    bar -- breaking it)."""
    flat = pr.zero_biases(name, pr.golden_weights(name))
    f = _Fwd(name, flat, hip_option)
    x, base, k = pr.mixed_rows(name, 4480, seed=21)
    for v in _variants(name):
        q0, q = f(base, v), f(x, v)
        assert np.abs(q0).min() > 1e-7
        assert _same(q, pr.scaled(q0, k)), (name, v)
    reps = AUTO_ROWS // len(x) + 1
    q0, q = f(np.concatenate([base] * reps), "auto"), f(np.concatenate([x] * reps), "auto")
    assert _same(q, pr.scaled(q0, np.concatenate([k] * reps))), (name, "auto")


def _act_worlds(names, flats, eps, n_worlds=48, seed=5):
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    dw = DeviceWorlds(n_worlds=n_worlds, width=30, height=30, max_agents=100, n_brains=len(names), static_families=True, seed=seed)
    dw.set_brains([(_kind(n), e, pack_brain_weights(_kind(n), w)) for n, w, e in zip(names, flats, eps)])
    dw.reset_synthetic(100)
    return dw


def _write_rows(dw, names, seed):
    """Overwrite Agent.state of every live agent with a golden row times 2^k (k from the range of the row's brain kind).  Returns the
    host copy of the rows, the live mask and the brain index per slot."""
    import torch
    n, brain = dw.s["n_agents"].cpu().numpy(), dw.s["a_brain"].cpu().numpy().astype(np.int64)
    live = np.arange(dw.cap)[None, :] < n[:, None]
    g = pr.golden_rows()
    rows = np.zeros((dw.R, dw.cap, 153), np.float32)
    slot = np.arange(dw.R * dw.cap).reshape(dw.R, dw.cap)
    for b, name in enumerate(names):
        m = live & (brain == b)
        cnt = int(m.sum())
        k = pr.mixed_exponents(cnt, *pr.K_RANGE[name], seed=seed + b)
        rows[m] = pr.scaled(g[slot[m] % len(g)], k)
    dw.obs_state().copy_(torch.from_numpy(rows).to(dw.device))
    return rows, live, brain


def test_policy_act_with_five_kinds_on_mixed_magnitude_rows(hip_option, capsys):
    """rl_policy_act over 48 worlds whose live rows a caller has overwritten with mixed-magnitude rows, brains [DQN, D3QN, PERD3QN, PPO,
    PERDQN] in one launch (rows bucketed by brain: a tile's rows come from different worlds): outputs per row against float64, the bits
    of rl_policy_forward on the gathered rows, actions = the oracle's selection rule on the launch's own outputs."""
    import torch
    from oracle import oracle as orc
    names, eps = list(pr.KINDS), [0.0, 0.3, 0.0, 0.0, 0.0]
    flats = [pr.golden_weights(n) for n in names]
    for variant in ("pair", "auto"):
        hip_option("policy_variant", variant)
        dw = _act_worlds(names, flats, eps)
        rows, live, brain = _write_rows(dw, names, seed=31)
        dw.act(want_q=True)
        torch.cuda.synchronize()
        dw.check_error_flag()
        act, q = dw.actions.cpu().numpy(), dw.out_q.cpu().numpy()
        tick, epoch = dw.s["tick"].cpu().numpy(), dw.s["epoch"].cpu().numpy()
        ocfg = orc.OracleWorlds(n_worlds=1, width=30, height=30, max_agents=100, n_brains=5, static_families=True, seed=5).cfg
        for b, name in enumerate(names):
            ws, ks = np.nonzero(live & (brain == b))
            assert len(ws) > 300, name
            x = rows[ws, ks]
            span = np.log2(np.abs(x).max(axis=1))
            assert span.max() - span.min() >= 40
            e = pr.err_of(name, q[ws, ks], pr.forward(name, flats[b], x))
            with capsys.disabled():
                print("\n[rl_policy_act, mixed rows, %s] %s: %d rows, max per-row error %.3g" % (variant, name, len(ws), float(e.max())))
            assert e.max() <= pr.ROW_BAR, (name, float(e.max()))
            assert _same(q[ws, ks], _Fwd(name, flats[b], hip_option)(x, variant)), name
            hip_option("policy_variant", variant)
            if name == "PERDQN":
                want = pr.argmax_first(q[ws, ks])
            else:
                want = orc.select_actions(ocfg, orc.KIND_BY_NAME[name], q[ws, ks], ws, ks, tick, epoch, eps[b])
            assert np.array_equal(act[ws, ks], want), name


def _run_worlds(names, flats, eps, shape, seed=31):
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    dw = DeviceWorlds(n_worlds=12, width=30, height=30, max_agents=shape["max_agents"], n_brains=len(names), static_families=True,
                      limit_reproduction=False, incentivize_killing=True, seed=seed, world_base=3)
    dw.set_brains([(_kind(n), e, pack_brain_weights(_kind(n), w)) for n, w, e in zip(names, flats, eps)])
    dw.reset_synthetic(shape["n_new"])
    assert dw.run_supported()
    return dw


RUN_SHAPES = {"one-wave": dict(max_agents=150, n_new=140, thr=130, names=["PERD3QN", "D3QN", "PERD3QN"]),   # 5+ tiles: the certified one-wave tile
              "pair": dict(max_agents=100, n_new=100, thr=70, names=["PERD3QN", "D3QN", "PERD3QN"]),       # <= 4 tiles: two waves per tile
              "mixed-kinds": dict(max_agents=100, n_new=100, thr=70, names=["DQN", "PERD3QN", "DQN"])}      # the kernel that picks the tile code per tile


@pytest.mark.parametrize("shape", list(RUN_SHAPES))
def test_a_weight_layer_scaled_by_a_power_of_two_changes_nothing_in_k_run(shape):
    """Brains A: golden weights, biases zeroed.  Brains B: the same with layer 1 times 2^+30 (brain 0) / 2^-30 (brain 2), brain 1 left
    as it is -- A-type and B-type brains in one world.  Host packing gives B the f16 planes of A and another unscale (CPU companion), so
    two worlds driven by A and by B must stay identical through 25 ticks of rl_run: one TRAIN 0 launch without outputs (certified
    finish: the argmax from the advantages alone, its bound from the packed weights) and 25 one-tick launches with want_q, whose out_q
    of B's rows is 2^k times A's.  Fault: a scale that enters anything but the epilogue multiply -- the certificate's value bound, the
    known-row-structure shortcut, a clamp."""
    from test_hip_round2 import _cmp_rows, _same_device_state
    sh = RUN_SHAPES[shape]
    names, eps, ks = sh["names"], [0.0, 0.2, 0.0], [30, 0, -30]
    A = [pr.zero_biases(n, pr.golden_weights(n)) for n in names]
    B = [pr.scale_layer1(n, w, k) for n, w, k in zip(names, A, ks)]
    # one launch of 25 ticks, no outputs
    a, b = _run_worlds(names, A, eps, sh), _run_worlds(names, B, eps, sh)
    a.run(25, sh["thr"], sh["n_new"]); b.run(25, sh["thr"], sh["n_new"])
    a.check_error_flag(); b.check_error_flag()
    _same_device_state(a, b, shape + " 25 ticks")
    acted = a.n_acted.cpu().numpy()
    assert acted.min() >= sh["thr"] and int(a.refill_count.item()) == int(b.refill_count.item())
    _cmp_rows(a.actions.cpu().numpy(), b.actions.cpu().numpy(), acted, "actions")
    post = a.n_post.cpu().numpy()
    _cmp_rows(a.reward.cpu().numpy(), b.reward.cpu().numpy(), post, "reward")
    # 25 launches of one tick with outputs
    a, b = _run_worlds(names, A, eps, sh, seed=32), _run_worlds(names, B, eps, sh, seed=32)
    scaled_rows = 0
    for t in range(25):
        brain = a.s["a_brain"].cpu().numpy().astype(np.int64)
        a.run(1, sh["thr"], sh["n_new"], want_q=True); b.run(1, sh["thr"], sh["n_new"], want_q=True)
        acted = a.n_acted.cpu().numpy()
        qa, qb = a.out_q.cpu().numpy(), b.out_q.cpu().numpy()
        kk = np.asarray(ks)[brain]
        for w in range(a.R):
            n = acted[w]
            assert _same(qb[w, :n], np.ldexp(qa[w, :n], kk[w, :n, None])), (shape, t, w)
            assert np.isfinite(qa[w, :n]).all() and np.abs(qa[w, :n]).max() > 0
            scaled_rows += int((kk[w, :n] != 0).sum())
        _cmp_rows(a.actions.cpu().numpy(), b.actions.cpu().numpy(), acted, "tick %d actions" % t)
        _cmp_rows(a.reward.cpu().numpy(), b.reward.cpu().numpy(), a.n_post.cpu().numpy(), "tick %d reward" % t)
        _same_device_state(a, b, "%s tick %d" % (shape, t))
    a.check_error_flag(); b.check_error_flag()
    assert scaled_rows > 10_000


@pytest.mark.parametrize("names", [["PPO", "PERD3QN", "DQN"], ["PERD3QN", "D3QN", "PERD3QN"]], ids=["mixed-kinds", "dueling"])
def test_k_run_on_rows_whose_maxima_span_twenty_binades_in_a_tile(names, capsys):
    """a_health is int32 and a caller may write it: every fourth agent gets a health of +-2^8 .. +-2^30 (health / 200 is a feature of the
    agent's row: 2^8 .. 2^27 alone would span 19.4 binades against the ordinary rows' [1, 2), 2^29 and 2^30 make it more than 20), rl_bind_state + observe() as
    test_known_row_structure_is_only_used_where_it_holds does.  Premise: within single tiles (the rows of one brain of one world, 32 at a
    time) the row maxima span more than 20 binades.  One fused tick with want_q equals the two-launch loop bit for bit, and the loop's
    outputs meet the per-row bar against float64 on the rows read back.  Fault: k_run's tiles taking a row scale from the world's known
    structure (or from a neighbour) where the rows do not have it."""
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    from test_hip_round2 import _cmp_rows, _same_device_state
    flats = [pr.golden_weights(n) for n in names]
    pair = []
    for _ in range(2):
        dw = DeviceWorlds(n_worlds=24, seed=17, static_families=False, width=30, height=30, max_agents=100, n_brains=3)
        dw.set_brains([(_kind(n), 0.0, pack_brain_weights(_kind(n), w)) for n, w in zip(names, flats)])
        dw.reset_synthetic(100)
        k = np.arange(dw.cap)
        h = (2.0 ** np.array([30, 8, 29, 14, 30, 20, 29, 27])[(k // 4) % 8]).astype(np.int64) * np.where((k // 8) % 2 == 0, 1, -1)
        sel = torch.from_numpy((k % 4 == 0)).to(dw.device)   # (every fourth: the others keep rows in [1, 2) unless a neighbour's health shows in their plane)
        hv = torch.from_numpy(h.astype(np.int32)).to(dw.device)
        dw.s["a_health"][:, sel] = hv[sel]
        dw.s["a_flags"][:, sel] = 0
        _lib.check(dw.lib.rl_bind_state(dw.handle, C.byref(dw._state)), "rl_bind_state")
        dw.observe()
        pair.append(dw)
    fused, loop = pair
    assert fused.run_supported()
    obs = fused.obs_state().cpu().numpy()
    n, brain = fused.s["n_agents"].cpu().numpy(), fused.s["a_brain"].cpu().numpy().astype(np.int64)
    tiles = full = wide = 0
    for w in range(fused.R):
        for b in range(3):
            ks = np.nonzero(brain[w, :n[w]] == b)[0]
            for t0 in range(0, len(ks), 32):
                e = np.floor(np.log2(np.abs(obs[w, ks[t0:t0 + 32]]).max(axis=1)))
                tiles += 1
                full += int(len(ks) - t0 >= 32)
                wide += int(len(ks) - t0 >= 32 and e.max() - e.min() > 20)
    with capsys.disabled():
        print("\n[k_run, caller-written healths] %d tiles, %d of them full; %d full tiles hold row maxima more than 20 binades apart" % (tiles, full, wide))
    assert full >= 36 and wide == full          # (a brain's last tile in a world holds what is left over: a handful of rows)
    fused.run(1, 70, 100, want_q=True)
    loop.act(want_q=True); loop.tick_refill(70, 100)
    fused.check_error_flag(); loop.check_error_flag()
    acted = fused.n_acted.cpu().numpy()
    assert np.array_equal(acted, n)
    qf, ql = fused.out_q.cpu().numpy(), loop.out_q.cpu().numpy()
    for w in range(fused.R):
        assert _same(qf[w, :n[w]], ql[w, :n[w]]), w
    _cmp_rows(fused.actions.cpu().numpy(), loop.actions.cpu().numpy(), acted, "actions")
    _same_device_state(fused, loop, "after the tick")
    live = np.arange(fused.cap)[None, :] < n[:, None]
    for b, name in enumerate(names):
        ws, ks = np.nonzero(live & (brain == b))
        x = obs[ws, ks]
        ref = pr.forward(name, flats[b], x)
        if name == "PPO":   # (scaled up, f32 itself leaves 1e-5 on the probabilities: the bar holds where the numpy f32 forward keeps its margin)
            fair = pr.err_of(name, pr.forward(name, flats[b], x, np.float32), ref) <= pr.F32_MARGIN
            assert fair.sum() > 100
        else:
            fair = np.ones(len(ws), bool)
        e = pr.err_of(name, ql[ws, ks], ref)
        with capsys.disabled():
            print("[k_run, caller-written healths] %s: %d rows (%d checked), max per-row error %.3g" % (name, len(ws), int(fair.sum()), float(e[fair].max())))
        assert e[fair].max() <= pr.ROW_BAR, (name, float(e[fair].max()))


# ---------------------------------------------------------------------------------------------------------------------
# B. exact ties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.KINDS)
def test_tied_outputs_are_bit_equal_and_the_first_maximum_wins(name, hip_option):
    """Heads whose eight rows are copies of two or three distinct rows (advantage head of the dueling kinds), four arrangements whose
    expected answers cover 0 .. 6, and the all-equal head (action 0).  With epsilon 0 and NO tolerance: duplicated outputs carry the same
    bits in every variant; the action of rl_policy_act is the oracle's rule on the kernel's own outputs, and the first index of the
    maximal group of the f32 reference wherever the gap between DISTINCT groups is >= 1e-5.  Fault: `>=` in the argmax (the CPU companion:
    then every one of these rows is wrong), a tree reduction that prefers the later lane, duplicated features summed in different orders."""
    import torch
    from oracle import oracle as orc
    x = pr.golden_rows()
    cases = [(p, pat, pr.tied_weights(name, pat, seed=5)) for p, pat in pr.TIE_PATTERNS.items()]
    cases.append(("all-equal", [0] * 8, pr.tied_weights(name, None, seed=5, all_equal=True)))
    seen = set()
    for label, pattern, flat in cases:
        ref = pr.forward(name, flat, x, np.float32)
        want, gap = pr.tie_expected(ref, pattern) if name != "PPO" else (None, None)
        f = _Fwd(name, flat, hip_option)
        outs = {v: f(x, v) for v in _variants(name)}
        outs["auto"] = f(np.concatenate([x] * (AUTO_ROWS // 640 + 1)), "auto")[:640]
        for v, out in outs.items():
            assert _same(out, outs["pair"]), (name, label, v)
            for i, g in enumerate(pattern):
                assert np.array_equal(_bits(out[:, i]), _bits(out[:, pattern.index(g)])), (name, label, v, i)
            tied = (out == out.max(axis=1, keepdims=True)).sum(axis=1) >= 2
            assert tied.sum() >= 200 and tied.all(), (name, label, v)
        # the action: rl_policy_act over worlds whose rows are the golden rows
        hip_option("policy_variant", "pair")
        dw = _act_worlds([name, name], [flat, flat], [0.0, 0.0], n_worlds=8)
        n, brain = dw.s["n_agents"].cpu().numpy(), dw.s["a_brain"].cpu().numpy()
        live = np.arange(dw.cap)[None, :] < n[:, None]
        rows = np.zeros((dw.R, dw.cap, 153), np.float32)
        ws, ks = np.nonzero(live)
        rows[ws, ks] = x[np.arange(len(ws)) % 640]
        dw.obs_state().copy_(torch.from_numpy(rows).to(dw.device))
        dw.act(want_q=True)
        torch.cuda.synchronize()
        act, q = dw.actions.cpu().numpy()[ws, ks], dw.out_q.cpu().numpy()[ws, ks]
        assert _same(q, outs["pair"][np.arange(len(ws)) % 640]) and len(ws) >= 640
        tick, epoch = dw.s["tick"].cpu().numpy(), dw.s["epoch"].cpu().numpy()
        if name == "PERDQN":
            assert np.array_equal(act, pr.argmax_first(q))
        else:
            ocfg = orc.OracleWorlds(n_worlds=1, width=30, height=30, max_agents=100, n_brains=2, static_families=True, seed=5).cfg
            assert np.array_equal(act, orc.select_actions(ocfg, orc.KIND_BY_NAME[name], q, ws, ks, tick, epoch, 0.0)), (name, label)
        if name != "PPO":
            idx = np.arange(len(ws)) % 640
            clear = gap[idx] >= 1e-5
            assert clear.sum() >= 600 or label == "all-equal"
            assert np.array_equal(act[clear], want[idx][clear]), (name, label)
            seen |= set(act[clear].tolist())
    if name != "PPO":
        assert seen == set(range(7)), seen


def test_saturated_ppo_head_gives_finite_one_hot_probabilities(hip_option):
    """Logit gaps beyond 200: the float64 softmax is exactly one-hot.  The probabilities are finite, within 1e-5 of it, and the sampled
    action of rl_policy_act is the hot index whatever the draw.  Fault: exp of an unshifted logit (Inf / Inf), a CDF walk that falls off the
    end when seven probabilities are zero."""
    import torch
    flat, hot = pr.saturated_ppo()
    x = pr.golden_rows()
    ref = pr.forward("PPO", flat, x)
    f = _Fwd("PPO", flat, hip_option)
    for v, rows in (("pair", x), ("auto", np.concatenate([x] * (AUTO_ROWS // 640 + 1)))):
        out = f(rows, v)[:640]
        assert np.isfinite(out).all() and np.abs(out - ref).max() <= 1e-5
        assert np.array_equal(out.argmax(axis=1), hot)
    hip_option("policy_variant", "pair")
    dw = _act_worlds(["PPO", "PPO"], [flat, flat], [0.0, 0.0], n_worlds=8)
    n = dw.s["n_agents"].cpu().numpy()
    ws, ks = np.nonzero(np.arange(dw.cap)[None, :] < n[:, None])
    rows = np.zeros((dw.R, dw.cap, 153), np.float32)
    rows[ws, ks] = x[np.arange(len(ws)) % 640]
    dw.obs_state().copy_(torch.from_numpy(rows).to(dw.device))
    dw.act(want_q=True)
    torch.cuda.synchronize()
    assert np.array_equal(dw.actions.cpu().numpy()[ws, ks], hot[np.arange(len(ws)) % 640])


def test_tied_heads_in_k_run_follow_the_oracles_rule():
    """OracleWorlds fed the launch's actions + PolicyCheck(tie_groups=...) for 50 ticks of TRAIN 0 WITHOUT outputs, in worlds of five or
    more tiles (the certified one-wave finish decides from the advantages alone): every greedy action is the first index of the maximal
    group of the f32 forward of the ORACLE's rows wherever distinct groups are >= 1e-5 apart -- the reference's rule, not only agreement of
    the launch with itself.  Every 10th tick a launch with outputs checks the duplicates' bits and the rule on the launch's own outputs."""
    from oracle import oracle as orc
    from policy_check import PolicyCheck
    from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
    names = ["PERD3QN", "D3QN", "PERD3QN"]
    pats = [pr.TIE_PATTERNS["034"], pr.TIE_PATTERNS["012"], pr.TIE_PATTERNS["06"]]
    flats = [pr.tied_weights(n, p, seed=40 + i) for i, (n, p) in enumerate(zip(names, pats))]
    cfg = dict(width=30, height=30, max_agents=150, n_brains=3, static_families=True, limit_reproduction=False, incentivize_killing=True)
    dw = DeviceWorlds(n_worlds=12, seed=31, **cfg)
    ow = orc.OracleWorlds(n_worlds=12, seed=31, **cfg)
    dw.set_brains([(_kind(n), 0.0, pack_brain_weights(_kind(n), w)) for n, w in zip(names, flats)])
    dw.reset_synthetic(140); ow.reset_synthetic(140)
    assert dw.run_supported()
    pc = PolicyCheck(names, flats, [0.0] * 3, tie_groups=pats)
    hist = np.zeros(8, np.int64)
    for t in range(50):
        n0 = ow.s["n_agents"].copy()
        assert n0.min() >= 130                                       # five tiles or more: the one-wave certified tile
        with_q = t % 10 == 9
        pc.before(ow)
        dw.run(1, 130, 140, want_q=with_q)
        acts = dw.actions.cpu().numpy()
        q = dw.out_q.cpu().numpy() if with_q else None
        pc.after(acts, q, "tick %d" % t)
        if with_q:
            for w in range(12):
                br = ow.s["a_brain"][w, :n0[w]]
                for b, pat in enumerate(pats):
                    rows = q[w, :n0[w]][br == b]
                    for i, g in enumerate(pat):
                        assert np.array_equal(_bits(rows[:, i]), _bits(rows[:, pat.index(g)])), (t, w, b, i)
        for w in range(12):
            hist += np.bincount(acts[w, :n0[w]].astype(np.int64), minlength=8)
        ow.step(acts); ow.update(); ow.refill(130, 140)
        assert np.array_equal(dw.n_acted.cpu().numpy(), n0)
        for key in ("cell_type", "n_agents", "tick", "epoch"):
            assert np.array_equal(dw.s[key].cpu().numpy().reshape(ow.s[key].shape), ow.s[key]), (t, key)
    dw.check_error_flag()
    print("tied heads in k_run: %d rows checked, action histogram %s" % (pc.rows, hist.tolist()))
    assert pc.rows > 50 * 12 * 130 and pc.q_rows > 5 * 12 * 130
    assert hist[5] == 0 and hist[7] == 0 and (hist > 0).sum() >= 4, hist     # only first indices of groups are ever chosen


# ---------------------------------------------------------------------------------------------------------------------
# C. degenerate rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pr.KINDS)
def test_degenerate_rows_inside_a_tile(name, hip_option, capsys):
    """One 32-row tile mixing ordinary rows with an all-zero row, a row of -0.0, a row with one non-zero element, rows whose maximum is
    2^-94 and 2^102 (inside row_scale's clamp range 2^-95 .. 2^103) -- all against float64 by the per-row bar (zero input: the biases alone)
    -- and rows outside the range (f32 subnormals, 2^-110, 2^110), which only have to be harmless: every OTHER row keeps the bits it has
    in a launch where those rows are zeros.  Plus a brain whose first layer is all-negative with a negative bias, on |x|: every hidden
    row is zero (row maximum 0 at a hidden layer).  Fault: a scale of Inf / NaN from a zero maximum, 0 * Inf in the epilogue, a clamp
    that lets 2^102 overflow f16."""
    import torch
    x, idx = pr.degenerate_tile()
    flat = pr.golden_weights(name)
    f = _Fwd(name, flat, hip_option)
    ref = pr.forward(name, flat, x)
    inside = np.ones(32, bool)
    inside[[idx[k] for k in pr.DEGENERATE_OUTSIDE]] = False
    if name == "PPO":            # (2^102 saturates the softmax: one-hot in float64 as well; the bar is absolute there)
        assert np.isfinite(ref[inside]).all()
    clean = x.copy(); clean[~inside] = 0.0
    for v in _variants(name) + ["auto"]:
        reps = AUTO_ROWS // 32 + 1 if v == "auto" else 1
        out = f(np.concatenate([x] * reps), v)[:32]
        base = f(np.concatenate([clean] * reps), v)[:32]
        e = pr.err_of(name, out[inside], ref[inside])
        with capsys.disabled():
            print("\n[degenerate tile] %s %s: max per-row error of the %d rows inside the range %.3g" % (name, v, int(inside.sum()), float(e.max())))
        assert np.isfinite(out[inside]).all() and e.max() <= pr.ROW_BAR, (name, v, float(e.max()), int(np.nonzero(inside)[0][e.argmax()]))
        assert _same(out[inside], base[inside]), (name, v, "rows outside the range disturbed their tile")
        assert _same(out[idx["zero"]], out[idx["negzero"]])
    dead = pr.dead_hidden_weights(name)
    fd = _Fwd(name, dead, hip_option)
    want = pr.h1_zero_reference(name, dead)
    for v in _variants(name):
        out = fd(np.abs(x[inside]), v)
        e = pr.err_of(name, out, np.broadcast_to(want, out.shape))
        assert e.max() <= pr.ROW_BAR and _same(out, np.broadcast_to(out[:1], out.shape)), (name, v, float(e.max()))
    # rl_policy_act: rows outside the range yield an action in 0 .. 7 and no error flag
    hip_option("policy_variant", "pair")
    dw = _act_worlds([name, name], [flat, flat], [0.0, 0.0], n_worlds=4)
    n = dw.s["n_agents"].cpu().numpy()
    ws, ks = np.nonzero(np.arange(dw.cap)[None, :] < n[:, None])
    rows = np.zeros((dw.R, dw.cap, 153), np.float32)
    rows[ws, ks] = x[np.arange(len(ws)) % 32]
    dw.obs_state().copy_(torch.from_numpy(rows).to(dw.device))
    dw.actions.fill_(-1)
    dw.act(want_q=True)
    torch.cuda.synchronize()
    dw.check_error_flag()
    act = dw.actions.cpu().numpy()[ws, ks]
    assert act.min() >= 0 and act.max() <= 7
    if name != "PPO":
        q = dw.out_q.cpu().numpy()[ws, ks]
        ok = inside[np.arange(len(ws)) % 32]
        assert np.array_equal(act[ok], pr.argmax_first(q[ok]))


BAD_ROWS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


@pytest.mark.parametrize("name", pr.KINDS)
def test_a_non_finite_row_leaves_its_tile_alone_and_reads_as_a_dead_hidden_row(name, hip_option):
    """A row holding NaN, +Inf or -Inf (one element, or all of them) between ordinary rows.
    Isolation: every other row's outputs AND action are bit-identical to a launch in which the bad row is zeros.
    The bad row itself -- the maintainers' choice, README "Limits": the kernels keep fmaxf's behaviour.  The row maximum and the ReLU are
    built from fmaxf / v_max, which return the operand that is a number, so the NaN the bad element puts into every feature of the first
    layer (0 * NaN included) ends at that layer's ReLU: the row comes out as a row whose first hidden layer is zero -- FINITE outputs, the
    later layers' biases alone -- where the reference propagates NaN (and argmax then answers 0).  Pinned here: finite, within the bar of
    that float64 value, action = first maximum of those outputs."""
    import torch
    g = pr.golden_rows()
    flat = pr.golden_weights(name)
    want = pr.h1_zero_reference(name, flat)
    f = _Fwd(name, flat, hip_option)
    x = g[64:128].copy()
    bad = {5: ("nan", False), 17: ("+inf", False), 38: ("-inf", False), 44: ("nan", True), 63: ("+inf", True)}
    clean = x.copy()
    for r, (what, whole) in bad.items():
        if whole:
            x[r] = BAD_ROWS[what]
        else:
            x[r, 11 + r] = BAD_ROWS[what]
        clean[r] = 0.0
    good = np.ones(64, bool); good[list(bad)] = False
    for v in _variants(name) + ["auto"]:
        reps = AUTO_ROWS // 64 + 1 if v == "auto" else 1
        out = f(np.concatenate([x] * reps), v)[:64]
        base = f(np.concatenate([clean] * reps), v)[:64]
        assert _same(out[good], base[good]), (name, v, "isolation")
        assert np.isfinite(out[~good]).all(), (name, v, out[~good])
        e = pr.err_of(name, out[~good], np.broadcast_to(want, out[~good].shape))
        assert e.max() <= pr.ROW_BAR, (name, v, float(e.max()))
    # actions through rl_policy_act: isolation of the other rows' actions, the bad rows' action from their own (finite) outputs
    hip_option("policy_variant", "pair")
    res = []
    for rows_of in (x, clean):
        dw = _act_worlds([name, name], [flat, flat], [0.0, 0.0], n_worlds=4)
        n = dw.s["n_agents"].cpu().numpy()
        ws, ks = np.nonzero(np.arange(dw.cap)[None, :] < n[:, None])
        rows = np.zeros((dw.R, dw.cap, 153), np.float32)
        rows[ws, ks] = rows_of[np.arange(len(ws)) % 64]
        dw.obs_state().copy_(torch.from_numpy(rows).to(dw.device))
        dw.act(want_q=True)
        torch.cuda.synchronize()
        dw.check_error_flag()
        res.append((dw.actions.cpu().numpy()[ws, ks], dw.out_q.cpu().numpy()[ws, ks], good[np.arange(len(ws)) % 64]))
    (a1, q1, ok), (a0, q0, _) = res
    assert np.array_equal(a1[ok], a0[ok]) and _same(q1[ok], q0[ok])
    assert np.isfinite(q1[~ok]).all() and a1.min() >= 0 and a1.max() <= 7
    if name != "PPO":
        assert np.array_equal(a1[~ok], pr.argmax_first(q1[~ok]))


# ---------------------------------------------------------------------------------------------------------------------
# D. within-row spread below the input layer
# ---------------------------------------------------------------------------------------------------------------------
def _spread_run(case, S, hip_option):
    x, w = pr.spread_problem(pr.SPREAD_N[case], S)
    brains, obs = pr.spread_brains(case, x, w)
    exact, bound, mag, scale = pr.spread_bound(case, x, w)
    out = np.zeros_like(exact)
    for name, flat, o in brains:
        got = _Fwd(name, flat, hip_option)(obs, "pair").astype(np.float64)
        if o is None:
            out = got
        else:
            assert np.all(got == got[:, :1])
            out[:, o] = got[:, 0]
    return np.abs(out - exact), exact, bound, mag, scale


@pytest.mark.parametrize("case", pr.SPREAD_CASES)
def test_within_row_spread_below_the_input_layer(case, hip_option, capsys):
    """test_policy_split_precision_within_row_dynamic_range one and two layers further down: activations AND weights of a hidden layer /
    a head spread over 2^0 .. 2^-S, arranged adversarially (a loaded brain with badly scaled hidden features).  Layer 1 (and 2) pass the
    signed values through as relu(+x), relu(-x); the layers behind the one under test recombine.  Asserted for S = 20: that docstring's
    bound for the layer under test, 2^-19 sum|x w| + n 2^-31 max|x| max|w_o|, plus the pass-through layers' own splits
    (test_policy_rows_cpu.spread_bound: derived from the scheme, not measured).  Swept and printed for S = 0 .. 32: the largest error
    relative to max|x| max|w_o|, to sum|x w|, and -- for the adversarial pairs, whose true value is ~n 2^-S of max|x| max|w| -- to |y|
    itself (docs/experiments.md records the table).  Fault: a hidden layer or head that splits against anything coarser than its own
    row's maximum, or drops the lo.hi / hi.lo product there."""
    rows = []
    for S in (0, 4, 8, 12, 16, 20, 24, 28, 32):
        err, exact, bound, mag, scale = _spread_run(case, S, hip_option)
        pairs = ([1, 2, 3, 4], [4, 5, 6, 7])
        rows.append((S, float((err / scale).max()), float((err / mag).max()), float((err[pairs] / np.abs(exact[pairs])).max()), float((err / bound).max())))
        if S == 20:
            assert (err <= bound).all(), (case, float((err / bound).max()))
            assert float((err[:, :4] / mag[:, :4]).max()) < 3e-6       # rows without an adversarial partner: f32-grade against the terms
    with capsys.disabled():
        print("\n[spread below the input layer] %s:  S | err / (max|x| max|w|) | err / sum|x w| | adversarial err / |y| | err / bound" % case)
        for r in rows:
            print("    %2d | %.3g | %.3g | %.3g | %.3f" % r)
