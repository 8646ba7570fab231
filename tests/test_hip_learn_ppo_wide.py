"""GPU: rl_learn_ppo_wide / rl_learn_rollout_wide / DeviceLearner(rollout=True, rollout_batch=B) / trainer(learn_batch={"PPO": B}) --
PPO.learn() (ReinLife/Models/PPO.py:136-162) on rollouts of up to 2048 rows in 32-row tiles with ONE GAE recursion over the whole rollout.
One tile against rl_learn_ppo bit for bit (every buffer, loss and grad; the draw against rl_learn_rollout); several tiles against torch
float64 autograd on the kernel's own parameters in front of each epoch (33, 64, 65, 96, 130 and 2048 rows: tests/test_learn_ppo_wide_cpu.py
shows without a GPU that no row sits at a kink and that a per-tile restart of the recursion is 3,000 bars away at 64 rows and more); Adam
replayed in float64 from the kernel's own gradients; the device packer; the gate, bad slots and refusals; repeatability and independence;
the draw at 2048 rows on a wrapped ring; trainer().  Inputs: learn_ppo_cases.edge_case() -- the reference's trained weights, 1,027 ring
rows, ratios 0.5 .. 2.  Every figure a bar is held against is printed before it is asserted.
Measured (MI355X): see DESIGN.md 5.30."""
import ctypes as C
import glob
import os
import warnings

import numpy as np
import pytest

import learn_d3qn_cases as dc
import learn_ppo_cases as pc
import learn_ppo_wide_cases as wc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
BUFFERS = ("params", "adam_m", "adam_v", "state", "packed")
RING_KEYS = ("ring_state", "ring_state_prime", "ring_action", "ring_reward", "ring_done")


def _brain(flat):
    import torch
    from reinlife_amd import Models
    b = Models.PPO()
    with torch.no_grad():
        for p, v in zip(b.model.parameters(), pc.split(flat)):
            p.copy_(torch.from_numpy(np.array(v, np.float32)))
    return b


def _ring(rows, prob, count=None, age=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture(..., with_prob=True) lays one out (full by default)."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None if prob is None else t(prob, torch.float32),
            "age": torch.zeros(capacity, dtype=torch.int32, device=DEV) if age is None else t(age, torch.int32),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(flat, ring, batch, n_grad=0, k_epoch=3, wide=True):
    """A wide learner of `batch` rows, or (wide=False) the narrow one on the same brain and ring."""
    import torch
    from reinlife_amd.learn import DeviceLearner
    if wide:
        l = DeviceLearner(_brain(flat), DEV, ring=ring, rollout=True, rollout_batch=batch)
        assert (l.entry, l.batch, l.lr, l.gamma, l.lmbda, l.eps_clip, l.k_epoch) == ("rl_learn_ppo_wide", batch, pc.LR, pc.GAMMA, pc.LMBDA, pc.EPS_CLIP, 3)
        assert l.target is None and l.work.numel() == wc.work_bytes(batch) and l.seen.item() == 0 and l.fresh.item() == 0
    else:
        l = DeviceLearner(_brain(flat), DEV, ring=ring, rollout=True)
        l.batch = batch
    l.k_epoch = k_epoch
    if n_grad:
        l.grad = torch.zeros((n_grad, pc.N_PARAMS), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_grad, dtype=torch.float32, device=DEV)
    return l


def _np(l, keys=BUFFERS):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in keys}


def _slots(s):
    return np.asarray(s, np.int32).reshape(1, 1, -1)


def _same(a, b, keys=BUFFERS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


@pytest.fixture(scope="module")
def edge():
    """(weights, ring rows, prob, one ring on the device shared by the tests that only read it)."""
    w, rows, prob, _ = pc.edge_case()
    return w, rows, prob, _ring(rows, prob)


def _host_pack(flat):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(_lib.PPO), np.float32)
    assert lib.rl_policy_pack_weights(_lib.PPO, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


# ---- 1. one tile is rl_learn_ppo ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True])
@pytest.mark.parametrize("batch", wc.ONE_TILE)
def test_one_tile_is_rl_learn_ppo_bit_for_bit(worlds, edge, batch, moments):
    """Rollouts of 1, 17 and 32 rows, k_epoch 3, two rollouts per call, from zero moments and from moments that are not zero at step
    9,999: params, adam_m, adam_v, state, packed, loss and grad of rl_learn_ppo_wide are rl_learn_ppo's, byte for byte."""
    import torch
    w, rows, prob, ring = edge
    slots = np.stack([wc.wide_slots(batch), wc.wide_slots(batch)[::-1]]).reshape(1, 2, batch).astype(np.int32)
    out = []
    for wide in (False, True):
        l = _learner(w, ring, batch, n_grad=6, wide=wide)
        if moments:
            m0, v0 = dc.adam_moments(pc.N_PARAMS)
            l.adam_m.copy_(torch.as_tensor(m0, device=DEV)); l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
            l.state[0] = 9999
        before = worlds.launches
        worlds.learn([l], 2, slots=slots, gate=False)
        assert worlds.launches - before == (wc.launches(2, 3) if wide else 1)
        out.append(_np(l, BUFFERS + ("loss", "grad")))
    worlds.check_error_flag()
    _same(out[0], out[1], BUFFERS + ("loss", "grad"))
    assert out[1]["state"].tolist() == [(9999 if moments else 0) + 6, 1] and out[1]["grad"].any(axis=1).all() and np.isfinite(out[1]["loss"]).all()
    assert out[1]["params"].tobytes() != np.asarray(w, np.float32).tobytes()


@pytest.mark.parametrize("batch", wc.ONE_TILE)
def test_the_one_tile_draw_is_rl_learn_rollout_bit_for_bit(worlds, edge, batch):
    """rl_learn_rollout_wide against rl_learn_rollout on a wrapped ring (count 1,500 of 1,027, 300 fresh rows): slots, keys, fresh, seen."""
    w, rows, prob, _ = edge
    out = []
    for wide in (False, True):
        l = _learner(w, _ring(rows, prob, count=1500), batch, wide=wide)
        l.seen.fill_(1200)
        s = worlds.draw_rollout([l], 2)
        assert tuple(s.shape) == (1, 2, batch)
        out.append((s.cpu().numpy(), l.keys.cpu().numpy(), int(l.fresh.item()), int(l.seen.item())))
    worlds.check_error_flag()
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()
    assert out[0][2:] == out[1][2:] == (300, 1500)
    assert set(out[1][0].reshape(-1).tolist()) <= set(pc.window_slots(1200, 1500, 1027))


# ---- 2. several tiles against float64 autograd -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def epochs(worlds, edge):
    """Per batch: three calls of ONE epoch each (parameters read in front of every epoch), then one call of three epochs."""
    cache = {}

    def run(batch):
        if batch not in cache:
            import torch
            w, rows, prob, ring = edge
            slots = _slots(wc.wide_slots(batch))
            l = _learner(w, ring, batch, n_grad=1, k_epoch=1)
            steps = []
            for ep in range(3):
                before = l.params.cpu().numpy().copy()
                worlds.learn([l], 1, slots=slots, gate=False)
                torch.cuda.synchronize()
                steps.append((before, l.grad[0].cpu().numpy().copy(), float(l.loss[0].item())))
            one = _learner(w, ring, batch, n_grad=3, k_epoch=3)
            worlds.learn([one], 1, slots=slots, gate=False)
            worlds.check_error_flag()
            cache[batch] = (steps, _np(l), _np(one, BUFFERS + ("grad", "loss")))
        return cache[batch]
    return run


@pytest.mark.parametrize("batch", wc.MULTI_TILE)
def test_every_epochs_gradients_match_float64_autograd(epochs, edge, batch):
    """tests/test_hip_learn_ppo.py's method on rollouts of several tiles: every gradient tensor within 1e-5 of its largest magnitude of
    torch float64 autograd on the kernel's own pre-epoch parameters, exact zeros where float64 has them, each loss within 1e-5.  One call
    of three epochs gives the bits of three calls of one."""
    w, rows, prob, _ = edge
    steps, three_calls, one_call = epochs(batch)
    r = pc.rows_of(rows, prob, wc.wide_slots(batch))
    for ep, (before, grad, loss) in enumerate(steps):
        loss64, g64, mid = pc.grads_autograd(before, r)
        got = pc.split(grad)
        errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, g64)]
        print("rows %d epoch %d: loss %.9g (float64 %.9g, relative error %.3g); gradient error / max|g|: %s; max |adv| %.3g"
              % (batch, ep + 1, loss, loss64, abs(loss - loss64) / abs(loss64), ", ".join("%s %.3g" % kv for kv in zip(pc.NAMES, errs)), np.abs(mid["adv"]).max()))
        for name, a, b in zip(pc.NAMES, got, g64):
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), (name, ep)
            assert not a[b == 0].any(), "%s: non-zero where float64 is exactly zero" % name
        assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    assert three_calls["state"].tolist() == [3, 3] and one_call["state"].tolist() == [3, 1]
    _same(three_calls, one_call, ("params", "adam_m", "adam_v", "packed"))
    assert one_call["grad"].tobytes() == np.stack([g for _, g, _ in steps]).tobytes()
    assert one_call["loss"].tobytes() == np.array([x for _, _, x in steps], np.float32).tobytes()


# ---- 3. Adam -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step0", [0, 10000])
def test_adam_matches_torch_formula_on_the_kernels_own_gradients(worlds, edge, step0):
    """130 rows, three epochs in one call, from step 0 with zero moments and from step 10,000 with moments that are not zero:
    torch.optim.Adam replayed in numpy float64 from the kernel's three gradients (parameters and moments rounded to float32 between the
    steps, as the kernel keeps them): every parameter within 1e-5 lr + 1 ulp, the moments within 1e-5 of their maxima."""
    import torch
    w, rows, prob, ring = edge
    l = _learner(w, ring, 130, n_grad=3)
    p, m, v = np.asarray(w, np.float64), np.zeros(pc.N_PARAMS), np.zeros(pc.N_PARAMS)
    if step0:
        m0, v0 = dc.adam_moments(pc.N_PARAMS)
        l.adam_m.copy_(torch.as_tensor(m0, device=DEV)); l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
        l.state[0] = step0
        m, v = m0.astype(np.float64), v0.astype(np.float64)
    worlds.learn([l], 1, slots=_slots(wc.wide_slots(130)), gate=False)
    r = _np(l, BUFFERS + ("grad",))
    worlds.check_error_flag()
    f32 = lambda x: x.astype(np.float32).astype(np.float64)  # noqa: E731
    for ep in range(3):
        assert r["grad"][ep].any()
        p, m, v = (f32(x) for x in pc.adam64(p, m, v, r["grad"][ep].astype(np.float64), step0 + ep + 1))
    err = np.abs(r["params"].astype(np.float64) - p)
    bound = 1e-5 * pc.LR + np.spacing(np.abs(r["params"])).astype(np.float64)
    em, ev = np.abs(r["adam_m"] - m).max() / np.abs(m).max(), np.abs(r["adam_v"] - v).max() / np.abs(v).max()
    print("Adam from step %d: worst |p - replay| / (1e-5 lr + 1 ulp) %.3g; moments: m %.3g v %.3g (relative to their maxima)" % (step0, (err / bound).max(), em, ev))
    assert (err <= bound).all() and em <= 1e-5 and ev <= 1e-5
    assert r["state"].tolist() == [step0 + 3, 1]


# ---- 4. the packer -----------------------------------------------------------------------------------------------------------------
def test_device_packing_is_the_host_packing_bit_for_bit(epochs, edge):
    _, _, one_call = epochs(130)
    assert one_call["packed"].tobytes() == _host_pack(one_call["params"]).tobytes() != _host_pack(edge[0]).tobytes()


# ---- 5. the gate, bad slots, refusals ----------------------------------------------------------------------------------------------
def test_an_empty_window_moves_only_the_call_counter(worlds, edge):
    w, rows, prob, _ = edge
    l = _learner(w, _ring(rows, prob, count=1500), 130, n_grad=3)
    l.seen.fill_(1500)
    before = _np(l)
    slots = worlds.draw_rollout([l], 1)
    slots.fill_(5000)   # (no slot check either: the table of a call that does not train is not read)
    worlds.learn([l], 1, slots=slots)
    after = _np(l)
    worlds.check_error_flag()
    assert l.fresh.item() == 0
    _same(before, after, ("params", "adam_m", "adam_v", "packed"))
    assert after["state"].tolist() == [0, 1] and not l.grad.any().item()
    l.ring["count"].fill_(1510)   # ten new rows: the next pair trains
    worlds.learn([l], 1, slots=worlds.draw_rollout([l], 1))
    after = _np(l)
    worlds.check_error_flag()
    assert l.fresh.item() == 10 and after["state"].tolist() == [3, 2] and after["params"].tobytes() != before["params"].tobytes()


def test_a_bad_slot_in_the_last_tile_is_flagged_and_that_learner_is_left_alone(worlds, edge):
    """Learner 0's table holds 1027 (one past the ring) in the last row of the last tile of the last rollout: code 6, learner 0, step 1,
    the value; none of its buffers is written.  Learner 1 of the same call ends with the bits of its solo call."""
    import torch
    w, rows, prob, ring = edge
    good = np.stack([wc.wide_slots(65), wc.wide_slots(65)[::-1]]).astype(np.int32)
    bad = good.copy()
    bad[1, 64] = 1027
    a, b = _learner(w, ring, 65, n_grad=6), _learner((np.asarray(w) * np.float32(0.75)).astype(np.float32), ring, 65)
    before = _np(a)
    worlds.learn([a, b], 2, slots=np.stack([bad, good]), gate=False)
    torch.cuda.synchronize()
    assert worlds.err.cpu().tolist() == [6, 0, 1, 1027]
    with pytest.raises(Exception, match="code 6"):
        worlds.check_error_flag()
    worlds.err.zero_()
    _same(before, _np(a))
    assert not a.grad.any().item()
    solo = _learner((np.asarray(w) * np.float32(0.75)).astype(np.float32), ring, 65)
    worlds.learn([solo], 2, slots=good.reshape(1, 2, 65), gate=False)
    rb, rs = _np(b), _np(solo)
    worlds.check_error_flag()
    assert rb["state"].tolist() == [6, 1]
    _same(rb, rs)


def test_the_entry_points_refuse_what_they_cannot_do(worlds, edge):
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    w, rows, prob, ring = edge
    lib = _lib.lib()
    l = _learner(w, ring, 130)
    table = np.zeros((1, 1, 130), np.int32)

    def call(learners, slots, work="own", n_steps=1):
        n = len(learners)
        arr = (_lib.Learner * n)(*[x.struct() for x in learners])
        rings = (_lib.Replay * n)(*[x.ring_struct() for x in learners])
        ppos = (_lib.Ppo * n)(*[x.ppo_struct(gate=False) for x in learners])
        wk = (C.c_void_p * n)(*[x.work.data_ptr() if x.work is not None else None for x in learners]) if work == "own" else work
        rc = lib.rl_learn_ppo_wide(worlds.handle, arr, rings, ppos, n, n_steps, None if slots is None else slots.data_ptr(), wk, worlds._stream())
        return rc, lib.rl_last_error().decode()
    import torch
    dev = torch.as_tensor(table, device=DEV)
    before = _np(l)
    rc, err = call([l], None)
    assert rc == -1 and "slots must not be null" in err and "rl_learn_rollout_wide" in err
    rc, err = call([l], dev, work=None)
    assert rc == -1 and "null work" in err
    rc, err = call([l], dev, work=(C.c_void_p * 1)(None))
    assert rc == -1 and "work[0]" in err
    for bad in (0, 2049):
        l.batch = bad
        rc, err = call([l], dev)
        assert rc == -1 and "[1,2048]" in err and "(got %d)" % bad in err
    l.batch = 130
    other = _learner(w, ring, 65)
    rc, err = call([l, other], dev)
    assert rc == -1 and "batch 65 differs from learner 0's 130" in err
    with pytest.raises(ValueError, match="must share one batch size"):
        worlds.learn([l, other], 1)
    l.kind = _lib.DQN
    rc, err = call([l], dev)
    assert rc == -4 and "kind 0" in err and "rl_learn_ppo_wide_supported" in err
    l.kind = _lib.PPO
    l.k_epoch = 9
    rc, err = call([l], dev)
    assert rc == -1 and "k_epoch" in err
    l.k_epoch = 3
    noprob = _learner(w, _ring(rows, None), 130)
    rc, err = call([noprob], dev)
    assert rc == -1 and "prob" in err
    narrow = _learner(w, ring, 32, wide=False)
    with pytest.raises(ValueError, match="one kind"):
        worlds.learn([narrow, l], 1, slots=np.zeros((2, 1, 32), np.int32))
    with pytest.raises(ValueError, match="one kind"):
        worlds.draw_rollout([narrow, _learner(w, ring, 32)], 1)
    with pytest.raises(ValueError, match=r"rollout_batch is for PPO brains with rollout=True \(rl_learn_ppo_wide\); got a PPO brain \(kind 3\) without rollout=True"):
        DeviceLearner(Models.PPO(), DEV, ring=ring, rollout_batch=130)
    _same(before, _np(l))
    worlds.check_error_flag()


# ---- 6. repeatability and independence ---------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits(worlds, edge, epochs):
    w, rows, prob, ring = edge
    again = _learner(w, ring, 2048, n_grad=3)
    worlds.learn([again], 1, slots=_slots(wc.wide_slots(2048)), gate=False)
    r = _np(again, BUFFERS + ("grad", "loss"))
    worlds.check_error_flag()
    _same(r, epochs(2048)[2], BUFFERS + ("grad", "loss"))


def test_the_last_of_sixteen_learners_is_the_learner_alone(worlds, edge):
    w, rows, prob, ring = edge
    scale = lambda i: (np.asarray(w) * np.float32(1 - 0.01 * i)).astype(np.float32)  # noqa: E731
    ls = [_learner(scale(i), ring, 65) for i in range(16)]
    table = np.stack([np.roll(wc.wide_slots(65), i) for i in range(16)]).reshape(16, 1, 65).astype(np.int32)
    worlds.learn(ls, 1, slots=table, gate=False)
    solo = _learner(scale(15), ring, 65)
    worlds.learn([solo], 1, slots=table[15:16], gate=False)
    r, rs, r0 = _np(ls[15]), _np(solo), _np(ls[0])
    worlds.check_error_flag()
    _same(r, rs)
    assert r["state"].tolist() == [3, 1] and r["params"].tobytes() != r0["params"].tobytes()


def test_rollouts_do_not_depend_on_the_order_of_the_ring(worlds, edge):
    """Two rings holding the same rows in different slots draw rollouts of 130 rows with identical content, and train to the same bits."""
    w, rows, prob, _ = edge
    perm = np.random.RandomState(4).permutation(1027)
    rows2 = {k: np.ascontiguousarray(rows[k][perm]) for k in RING_KEYS}   # slot j of the permuted ring holds row perm[j]
    a, b = _learner(w, _ring(rows, prob), 130), _learner(w, _ring(rows2, prob[perm]), 130)
    sa, sb = worlds.draw_rollout([a], 2), worlds.draw_rollout([b], 2)
    na, nb = sa.cpu().numpy().reshape(-1), sb.cpu().numpy().reshape(-1)
    assert a.fresh.item() == 1027 == b.fresh.item() and not np.array_equal(na, nb) and np.array_equal(perm[nb], na) and len(np.unique(na)) > 200
    worlds.learn([a], 2, slots=sa)
    worlds.learn([b], 2, slots=sb)
    ra, rb = _np(a), _np(b)
    worlds.check_error_flag()
    _same(ra, rb)
    assert ra["state"].tolist() == [6, 1]
    # the table is the host model's: content keys, Philox words 0-1 of (seed, 0, brain 0, calls 0, RL_SITE_LEARN_ROLLOUT, d = s * batch + j)
    keys = a.keys.cpu().numpy().view(np.uint64)
    assert np.array_equal(pc.rollout_table(keys, np.arange(1027), SEED, 0, 0, 260), na)


def test_learners_with_different_k_epoch_in_one_call_equal_their_solo_calls(worlds, edge):
    w, rows, prob, ring = edge
    slots = np.stack([wc.wide_slots(96), wc.wide_slots(96)[::-1]]).reshape(2, 1, 96).astype(np.int32)

    def pair():
        return _learner(w, ring, 96, n_grad=1, k_epoch=1), _learner(w, ring, 96, n_grad=3, k_epoch=3)
    a, b = pair()
    before = worlds.launches
    worlds.learn([a, b], 1, slots=slots, gate=False)
    assert worlds.launches - before == wc.launches(1, 3)
    sa, sb = pair()
    worlds.learn([sa], 1, slots=slots[0:1], gate=False)
    worlds.learn([sb], 1, slots=slots[1:2], gate=False)
    keys = BUFFERS + ("grad", "loss")
    ra, rb, rsa, rsb = _np(a, keys), _np(b, keys), _np(sa, keys), _np(sb, keys)
    worlds.check_error_flag()
    _same(ra, rsa, keys)
    _same(rb, rsb, keys)
    assert ra["state"].tolist() == [1, 1] and rb["state"].tolist() == [3, 1]


# ---- 7. the draw at 2048 rows ------------------------------------------------------------------------------------------------------
def test_wide_draws_fall_only_on_the_window_and_are_uniform_over_it(worlds, edge):
    """seen = count - 48 on a wrapped ring of 1,027 (count 2,070: the window is slots 995 .. 1026 and 0 .. 15).  6,400 draws of a
    2048-row call (the first 6,400 of its 3 x 2048) fall on the window alone, every row's count within 5 binomial standard deviations of
    6400 / 48 (deterministic: this passes always or never)."""
    w, rows, prob, _ = edge
    l = _learner(w, _ring(rows, prob, count=2070), 2048)
    l.seen.fill_(2022)
    window = pc.window_slots(2022, 2070, 1027)
    assert sorted(window) == list(range(0, 16)) + list(range(995, 1027))
    all_slots = worlds.draw_rollout([l], 4).cpu().numpy().reshape(-1)
    worlds.check_error_flag()
    assert l.fresh.item() == 48 and l.seen.item() == 2070 and all_slots.size == 8192
    assert set(all_slots.tolist()) <= set(window)
    counts = np.bincount(all_slots[:6400], minlength=1027)
    n, p = 6400, 1 / 48
    z = np.abs(counts[window] - n * p) / np.sqrt(n * p * (1 - p))
    print("wide rollout draws: counts %d..%d (expected %.1f); worst deviation %.2f sd" % (counts[window].min(), counts[window].max(), n * p, z.max()))
    assert counts.sum() == counts[window].sum() == 6400 and (z <= 5).all()


# ---- 8. trainer() ------------------------------------------------------------------------------------------------------------------
def _train(learn_batch, n_episodes=40, save=False, **more):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=60), Models.PPO()]
    init = [b.state_dict_flat().copy() for b in brains]
    kw = {"learn_batch": learn_batch} if learn_batch is not None else {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=n_episodes, n_worlds=2, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      learn_rollout=True, save=save, print_results=False, **kw, **more)
    return env, brains, init


def _learner_bytes(l):
    return {k: getattr(l, k).cpu().numpy().tobytes() for k in BUFFERS + (("target",) if l.target is not None else ())}


def test_trainer_learn_batch_ppo_32_is_the_run_without_the_key():
    env, brains, _ = _train({"PPO": 32})
    env0, brains0, _ = _train(None)
    assert env.learners[1].entry == "rl_learn_ppo_wide" and env0.learners[1].entry == "rl_learn_ppo"
    assert env.learners[1].state.cpu().tolist() == [6, 2] == env0.learners[1].state.cpu().tolist()
    for k in (0, 1):
        assert _learner_bytes(env.learners[k]) == _learner_bytes(env0.learners[k]), k
        assert brains[k].state_dict_flat().tobytes() == brains0[k].state_dict_flat().tobytes()
    assert env.tracker.results == env0.tracker.results
    assert env.worlds.launches - env0.worlds.launches == 2 * (wc.launches(1, 3) - 1)


def test_trainer_learn_batch_ppo_130_trains_saves_and_repeats(tmp_path, monkeypatch):
    """{"PPO": 130} over 40 episodes (two learning calls): trains, saves loadable weights, names the entry point and the key, repeats bit
    for bit, and is the identity under learn_ranks="average" on one rank.  "The DQN learner beside it is the run's without the key" is
    asserted in its reachable form, as tests/test_hip_learn_ppo.py does for the keyword itself: over a 20-episode run, up to and including
    the DQN's first learning call with the PPO's first call BEHIND it.  After that the PPO acts with other weights than in the run
    without the key, the worlds both brains share part company, and so do the rows the DQN learner sees: no equality exists to assert
    for the 40-episode run."""
    from reinlife_amd import Models
    monkeypatch.chdir(tmp_path)
    env, brains, init = _train({"PPO": 130}, save=True)
    l = env.learners[1]
    assert l.entry == "rl_learn_ppo_wide" and l.batch == 130 and l.state.cpu().tolist() == [6, 2] and env.learn_batch == {"PPO": 130}
    now = brains[1].state_dict_flat()
    assert np.isfinite(now).all() and not np.array_equal(now, init[1]) and now.tobytes() == l.params.cpu().numpy().tobytes()
    assert env.worlds._brain_keep[1].data_ptr() == l.packed.data_ptr()
    assert l.packed.cpu().numpy().tobytes() == _host_pack(now).tobytes() != _host_pack(init[1]).tobytes()
    note = env._weights_note()
    assert "rl_learn_ppo_wide" in note and "130 rows" in note and "rl_learn:" in note
    files = glob.glob(os.path.join(str(tmp_path), "experiments", "*", "PPO", "brain_gene_*.pt"))
    assert len(files) == 1 and Models.PPO(load_model=files[0]).state_dict_flat().tobytes() == now.tobytes()
    settings = open(glob.glob(os.path.join(str(tmp_path), "experiments", "*", "settings.json"))[0]).read()
    assert "rl_learn_ppo_wide" in settings and '"Learn batch"' in settings
    env2, brains2, _ = _train({"PPO": 130})
    for b, b2 in zip(brains, brains2):
        assert b.state_dict_flat().tobytes() == b2.state_dict_flat().tobytes()
    assert env.tracker.results == env2.tracker.results
    # one rank with learn_ranks="average": the identity merge
    env3, brains3, _ = _train({"PPO": 130}, learn_ranks="average")
    for k in (0, 1):
        assert _learner_bytes(env.learners[k]) == _learner_bytes(env3.learners[k]), k
    # up to and including episode 20 -- the DQN's first call, with the PPO's first call BEHIND it -- the DQN learner is the run's without the key
    enva, _, _ = _train({"PPO": 130}, 20)
    envb, _, _ = _train(None, 20)
    assert _learner_bytes(enva.learners[0]) == _learner_bytes(envb.learners[0]) and enva.tracker.results == envb.tracker.results
    assert _learner_bytes(enva.learners[1])["params"] != _learner_bytes(envb.learners[1])["params"]


def test_the_key_without_learn_rollout_is_refused_before_a_device_is_touched(monkeypatch):
    from reinlife_amd import Models, trainer, worlds as wmod
    monkeypatch.setattr(wmod.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=r"learn_batch as a dict takes the keys 'DQN' \(rl_learn_wide\) and 'D3QN' \(rl_learn_dueling_wide\) and at least one of them"):
        trainer([Models.DQN(max_epi=60), Models.PPO()], n_episodes=5, n_worlds=2, learn="device", learn_batch={"PPO": 130}, save=False, print_results=False)
