"""GPU: the learners' draws and updates beyond the 96-row fixtures -- rl_learn_draw and rl_learn_prioritized_draw row for row against exact
host models on rings whose strided loops take a second pass and whose last group of four rows is partial (1 .. 1025 rows, with real
ages, size below capacity), stamping through the wrap of a capacity that is no multiple of four, learners of different batches and
capacities in one draw call of the C ABI, one update of rl_learn / rl_learn_dueling / rl_learn_prioritized on the reference's TRAINED
weights (tests/golden/pretrained.npz: |w| up to 1.75, |q| up to 40) against float64, Adam at step 10,000 on moments that are not zero,
and the update kernels on rings of 5,000 and 10,000 rows.  tests/test_learn_edges_cpu.py checks without a GPU that these inputs satisfy
what the comparisons rest on.  Every figure a bar is held against is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import learn_cases as lc
import learn_d3qn_cases as dc
import learn_perd3qn_cases as pc

pytestmark = pytest.mark.gpu

SEED = 11
DEV = "cuda:0"
SIZES = (1, 3, 255, 256, 257, 701, 1025)
BUFFERS = ("params", "target", "adam_m", "adam_v", "state", "packed")
SENTINEL = np.float32(2.0 ** -20)
GUARD = 64
_keys = {}


def _edge(n, seed=11):
    """(the first n of 1027 seeded rows with ages 0..199, their content keys)"""
    if seed not in _keys:
        rows = lc.edge_ring_rows(1027, seed)
        _keys[seed] = (rows, pc.content_keys(rows, 1027, rows["ring_age"]))
        assert len(set(_keys[seed][1].tolist())) == 1027
    rows, keys = _keys[seed]
    return {k: v[:n] for k, v in rows.items()}, keys[:n]


def _ring(rows, count=None):
    """A replay ring on the device from host rows, as DeviceWorlds.enable_capture lays one out; the ages are the rows' ("ring_age") or 0."""
    import torch
    capacity = rows["ring_state"].shape[0]
    t = lambda a, dt: torch.as_tensor(np.array(a), device=DEV).to(dt)  # noqa: E731
    age = rows["ring_age"] if "ring_age" in rows else np.zeros(capacity, np.int32)
    return {"state": t(rows["ring_state"], torch.float32), "state_prime": t(rows["ring_state_prime"], torch.float32),
            "action": t(rows["ring_action"], torch.int8), "reward": t(rows["ring_reward"], torch.float32),
            "done": t(rows["ring_done"], torch.uint8), "prob": None, "age": t(age, torch.int32),
            "count": torch.full((1,), capacity if count is None else count, dtype=torch.int64, device=DEV)}


def _learner(method, ring=None, batch=None, params=None, target=None, want_grad=False, n_steps=1):
    """A DeviceLearner of `method` ("DQN", "D3QN", "PERD3QN": the prioritised one) whose size gate is open; params / target: flat float32
    written over the brain's own (the update kernels read nothing else of the networks)."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    l = DeviceLearner(getattr(Models, method)(), DEV, ring=ring, prioritized=method == "PERD3QN")
    assert l.entry == {"DQN": "rl_learn", "D3QN": "rl_learn_dueling", "PERD3QN": "rl_learn_prioritized"}[method]
    if batch is not None:
        l.batch = batch
    l.min_size = 0
    if params is not None:
        l.params.copy_(torch.as_tensor(np.array(params, np.float32), device=DEV))
        l.target.copy_(torch.as_tensor(np.array(params if target is None else target, np.float32), device=DEV))
    if want_grad:
        l.grad = torch.zeros((n_steps, l.n_params), dtype=torch.float32, device=DEV)
        l.loss = torch.zeros(n_steps, dtype=torch.float32, device=DEV)
    return l


def _prime(l, ring, priority, fill_beyond=None):
    """Give a prioritised learner `ring` and the priorities of its first len(priority) rows, with nothing new to stamp (seen = count)."""
    import torch
    l.ring = ring
    l._make_prio()
    n = len(priority)
    if fill_beyond is not None:      # rows beyond the ring's size: a kernel that read them would draw them
        l.priority.fill_(fill_beyond)
        l.weight.fill_(fill_beyond)
    l.priority[:n] = torch.as_tensor(np.asarray(priority, np.float32), device=DEV)
    l.seen.copy_(ring["count"])


def _np(l, names=BUFFERS):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(l, k).cpu().numpy().copy() for k in names}


def _host_pack(flat, kind):
    from reinlife_amd import _lib
    lib = _lib.lib()
    flat = np.ascontiguousarray(flat, np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(kind), np.float32)
    assert lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    return packed


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=SEED, device=DEV)


@pytest.fixture(scope="module")
def drawers():
    """One learner of each kind for the draw tests; every case gives them its own ring."""
    return {"DQN": _learner("DQN", batch=32), "D3QN": _learner("D3QN", batch=64), "PERD3QN": _learner("PERD3QN", batch=64)}


# ---- 2. both draws, row for row ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_the_uniform_draw_is_the_host_models_row_for_row(worlds, drawers, n, slack):
    """rl_learn_draw on n rows of a ring of capacity n + slack: every slot of a batch-32 DQN learner's and a batch-64 D3QN learner's two
    steps, at calls 0 and 3, is argmin_i mix64(key_i ^ salt_d) of the host; the keys read back are the content keys WITH the ages."""
    import torch
    rows, keys = _edge(n + slack)
    ring = _ring(rows, count=n)
    for method, batch in (("DQN", 32), ("D3QN", 64)):
        l = drawers[method]
        l.ring = ring
        for calls in (0, 3):
            l.state[1] = calls
            got = worlds.draw_slots([l], 2)
            torch.cuda.synchronize()
            assert tuple(got.shape) == (1, 2, batch) and got.dtype == torch.int32
            got = got.cpu().numpy().reshape(-1)
            want = pc.host_uniform_draw(keys[:n], SEED, 0, calls, 2 * batch)
            print("n %d capacity %d %s calls %d: %d of %d draws differ; %d distinct rows, %d beyond row 255" % (
                n, n + slack, method, calls, int((got != want).sum()), got.size, len(np.unique(want)), int((want >= 256).sum())))
            assert np.array_equal(got, want)
        assert l.keys.numel() == n + slack
        assert np.array_equal(l.keys.cpu().numpy().view(np.uint64)[:n], keys[:n])
    worlds.check_error_flag()


@pytest.mark.parametrize("slack", [0, 2])
@pytest.mark.parametrize("n", SIZES)
def test_the_prioritised_draw_is_the_host_models_row_for_row(worlds, drawers, n, slack):
    """rl_learn_prioritized_draw on n rows (capacity n + slack; priorities random^3 * 4, every 7th row 0): weight = priority^0.6 within
    relative 1e-6 of float64 and exactly 0 for a zero priority; every one of the 128 slots is the winner of the float64 race run on the
    device's own float32 weights.  The race's smallest relative gap between first and second is at least 1e-4 on these inputs (asserted
    here from the device's weights, and without a GPU in tests/test_learn_edges_cpu.py), a hundred times what -logf(U) / w can be off by,
    so no draw is left out.  Rows beyond the size hold a weight and a priority of 1e6: a loop bounded by the capacity would draw them."""
    import torch
    rows, keys = _edge(n + slack)
    ring = _ring(rows, count=n)
    l = drawers["PERD3QN"]
    pri = pc.edge_priorities(n)
    _prime(l, ring, pri, fill_beyond=1e6)
    l.state[1] = 3
    got = worlds.draw_prioritized([l], 2)
    torch.cuda.synchronize()
    worlds.check_error_flag()
    assert tuple(got.shape) == (1, 2, 64) and got.dtype == torch.int32
    got, w, p_after = got.cpu().numpy().reshape(-1), l.weight.cpu().numpy(), l.priority.cpu().numpy()
    w64 = pri.astype(np.float64) ** 0.6
    live = pri > 0
    werr = float((np.abs(w[:n][live] - w64[live]) / w64[live]).max())
    want, gaps = pc.host_draw64(keys[:n], w[:n], SEED, 0, 3, 128)
    print("n %d capacity %d: max relative weight error %.3g; smallest gap %.3g; %d of 128 draws differ; %d distinct rows, %d beyond row 255, %d rows of priority 0"
          % (n, n + slack, werr, gaps.min(), int((got != want).sum()), len(np.unique(want)), int((want >= 256).sum()), int((~live).sum())))
    assert werr <= 1e-6 and not w[:n][~live].any()
    assert gaps.min() >= 1e-4
    assert np.array_equal(got, want)
    assert live[got].all()
    assert np.array_equal(l.keys.cpu().numpy().view(np.uint64)[:n], keys[:n])
    assert p_after[:n].tobytes() == pri.tobytes() and (p_after[n:] == 1e6).all() and (w[n:] == 1e6).all()   # nothing stamped, nothing beyond the size written
    assert int(l.seen.item()) == n


def test_with_no_weight_anywhere_the_prioritised_draw_is_the_uniform_one_on_its_own_site(worlds, drawers):
    """257 rows, every priority 0: t = +inf everywhere, v alone orders the race -- host_uniform_draw with RL_SITE_LEARN_PRIO's salt."""
    import torch
    from reinlife_amd import _lib
    rows, keys = _edge(257)
    l = drawers["PERD3QN"]
    _prime(l, _ring(rows), np.zeros(257, np.float32))
    l.state[1] = 3
    got = worlds.draw_prioritized([l], 2).cpu().numpy().reshape(-1)
    torch.cuda.synchronize()
    worlds.check_error_flag()
    want = pc.host_uniform_draw(keys, SEED, 0, 3, 128, site=_lib.SITE_LEARN_PRIO)
    print("all zero: %d of 128 draws differ; %d distinct rows, %d beyond row 255" % (int((got != want).sum()), len(np.unique(want)), int((want >= 256).sum())))
    assert np.array_equal(got, want) and not l.weight.any().item()
    assert not np.array_equal(want, pc.host_uniform_draw(keys, SEED, 0, 3, 128))         # (the site salts the draw)


def test_stamping_through_the_wrap_of_a_capacity_that_is_no_multiple_of_four(worlds, drawers):
    """Capacity 1001: seen 990 -> count 1100 at maximum 3 (slots 990..1000 and 0..98), then a whole capacity of new rows, then nothing
    new: priority and seen are HostMemory's exactly, weight = priority^0.6 within relative 1e-6."""
    import torch
    rows, _ = _edge(1001)
    l = drawers["PERD3QN"]
    _prime(l, _ring(rows), np.full(1001, SENTINEL, np.float32))
    host = pc.HostMemory(1001)
    host.priority[:] = SENTINEL
    for count, seen, prio_max in ((1100, 990, 3.0), (1100 + 1001, None, 4.0), (1100 + 1001, None, 5.0)):
        l.ring["count"].fill_(count)
        host.count = count
        if seen is not None:
            l.seen.fill_(seen)
            host.seen = seen
        l.prio_max.fill_(prio_max)
        host.prio_max = np.float32(prio_max)
        want = host.stamp().copy()
        slots = worlds.draw_prioritized([l], 1)
        torch.cuda.synchronize()
        p, w = l.priority.cpu().numpy(), l.weight.cpu().numpy()
        werr = float((np.abs(w - p.astype(np.float64) ** 0.6) / p.astype(np.float64) ** 0.6).max())
        print("count %d: %d rows at %.1f (host %d), seen %d, max relative weight error %.3g" % (
            count, int((p == prio_max).sum()), prio_max, int((want == prio_max).sum()), int(l.seen.item()), werr))
        assert p.tobytes() == want.tobytes()
        assert int(l.seen.item()) == host.seen == count and l.prio_max.item() == prio_max
        assert werr <= 1e-6
        assert int(slots.min()) >= 0 and int(slots.max()) < 1001
    assert (want[990:] == 4.0).all() and (want == 4.0).all()                             # (the last look stamped nothing at 5.0)
    worlds.check_error_flag()


def _slot_buffer(total):
    import torch
    buf = torch.full((GUARD + total + GUARD,), -1, dtype=torch.int32, device=DEV)
    return buf, C.c_void_p(buf.data_ptr() + 4 * GUARD)


def _check_tables(buf, tables):
    """The learners' tables end to end between two rows of guards: each equal to its host model, the guards untouched."""
    got = buf.cpu().numpy()
    total = sum(len(t) for t in tables)
    assert got.size == 2 * GUARD + total
    assert (got[:GUARD] == -1).all() and (got[GUARD + total:] == -1).all()
    off = GUARD
    for i, t in enumerate(tables):
        print("learner %d: %d of %d draws differ" % (i, int((got[off:off + len(t)] != t).sum()), len(t)))
        assert np.array_equal(got[off:off + len(t)], t), i
        off += len(t)


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_learners_of_different_batches_in_one_uniform_draw_call(worlds, drawers, order):
    """rl_learn_draw through the C ABI with (batch 32, 257 rows) and (batch 5, 96 rows) in one call, two steps: the tables lie end to end
    in a buffer of exactly sum(n_steps * batch) entries, each the host model's at its learner's own position; 64 guard entries on either
    side keep their -1."""
    import torch
    from reinlife_amd import _lib
    cases = [("DQN", 32, _edge(257), 3), ("DQN", 5, _edge(96, seed=12), 1)]
    cases = [cases[i] for i in order]
    learners = []
    for method, batch, (rows, keys), calls in cases:
        l = _learner(method, ring=_ring(rows), batch=batch)
        l.state[1] = calls
        l.keys = torch.zeros(len(keys), dtype=torch.int64, device=DEV)
        learners.append(l)
    n = len(learners)
    arr = (_lib.Learner * n)(*[l.struct() for l in learners])
    rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
    keyp = (C.c_void_p * n)(*[l.keys.data_ptr() for l in learners])
    buf, ptr = _slot_buffer(sum(2 * c[1] for c in cases))
    _lib.check(worlds.lib.rl_learn_draw(worlds.handle, arr, rings, n, 2, keyp, ptr, worlds._stream()), "rl_learn_draw")
    torch.cuda.synchronize()
    worlds.check_error_flag()
    _check_tables(buf, [pc.host_uniform_draw(c[2][1], SEED, i, c[3], 2 * c[1]) for i, c in enumerate(cases)])
    for l, c in zip(learners, cases):
        assert np.array_equal(l.keys.cpu().numpy().view(np.uint64), c[2][1])


@pytest.mark.parametrize("order", [(0, 1), (1, 0)])
def test_learners_of_different_batches_in_one_prioritised_draw_call(worlds, order):
    """rl_learn_prioritized_draw through the C ABI with (batch 64, 257 rows) and (batch 7, 96 rows) in one call, two steps: as above, each
    table the float64 race's on that learner's own weights, with the 1e-4 gap asserted first."""
    import torch
    from reinlife_amd import _lib
    cases = [(64, _edge(257), 3, 5), (7, _edge(96, seed=12), 1, 6)]
    cases = [cases[i] for i in order]
    learners = []
    for batch, (rows, keys), calls, pseed in cases:
        l = _learner("PERD3QN", batch=batch)
        _prime(l, _ring(rows), pc.edge_priorities(len(keys), pseed))
        l.state[1] = calls
        learners.append(l)
    n = len(learners)
    arr = (_lib.Learner * n)(*[l.struct() for l in learners])
    rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
    prios = (_lib.Prio * n)(*[l.prio_struct() for l in learners])
    buf, ptr = _slot_buffer(sum(2 * c[0] for c in cases))
    _lib.check(worlds.lib.rl_learn_prioritized_draw(worlds.handle, arr, rings, prios, n, 2, ptr, worlds._stream()), "rl_learn_prioritized_draw")
    torch.cuda.synchronize()
    worlds.check_error_flag()
    tables = []
    for i, (l, c) in enumerate(zip(learners, cases)):
        want, gaps = pc.host_draw64(c[1][1], l.weight.cpu().numpy(), SEED, i, c[2], 2 * c[0])
        print("learner %d (batch %d, %d rows): smallest gap %.3g" % (i, c[0], len(c[1][1]), gaps.min()))
        assert gaps.min() >= 1e-4
        tables.append(want)
        assert int(l.seen.item()) == len(c[1][1])
    _check_tables(buf, tables)


# ---- 3. updates on trained weights -------------------------------------------------------------------------------------------------
def _fixture_of(method):
    return (lc, lc.golden()) if method == "DQN" else (dc, dc.golden())


@pytest.mark.parametrize("method, batch", [("DQN", 32), ("D3QN", 64), ("D3QN", 33), ("PERD3QN", 64), ("PERD3QN", 33)])
def test_one_step_on_trained_weights_matches_float64(worlds, method, batch):
    """The reference's trained weights as the eval network, the same times float32(0.96875) as the target, the fixture's ring and first
    minibatch: every gradient tensor within 1e-5 of its largest float64 entry, the loss within relative 1e-5 (torch's own float32
    autograd: 1.9e-7 to 3.2e-7 on these inputs, tests/test_learn_edges_cpu.py); PERD3QN: the batch rows' priorities within 1e-5 of float64,
    relative to the largest |q|, |q'|; the packed weights byte for byte the host packer's of the parameters read back."""
    import torch
    from reinlife_amd import _lib
    mod, g = _fixture_of(method)
    w, tgt = lc.pretrained(method)
    slots = g["slots"][0][:batch].astype(np.int32)
    l = _learner(method, ring=_ring(g), batch=batch, params=w, target=tgt, want_grad=True)
    if method == "PERD3QN":
        _prime(l, l.ring, np.full(96, SENTINEL, np.float32))
    worlds.learn([l], 1, slots=slots.reshape(1, 1, batch))
    r = _np(l)
    worlds.check_error_flag()
    loss64, g64 = mod.grads64(w, tgt, g, slots, l.gamma)
    got, loss = mod.split(l.grad[0].cpu().numpy()), float(l.loss[0].item())
    print("%s batch %d: loss %.9g (float64 %.9g, relative error %.3g)" % (method, batch, loss, loss64, abs(loss - loss64) / abs(loss64)))
    worst = 0.0
    for name, a, b in zip(mod.NAMES, got, g64):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        worst = max(worst, err)
        print("%s batch %d: %-17s max|g| %.4g  error / max|g| %.3g" % (method, batch, name, np.abs(b).max(), err))
    print("%s batch %d: worst gradient error / max|g| = %.3g; max |w| %.3g" % (method, batch, worst, np.abs(w).max()))
    if method == "PERD3QN":
        p64, q, qn = pc.priorities(w, tgt, g, slots)
        scale = max(np.abs(q).max(), np.abs(qn).max())
        perr = float(np.abs(l.priority.cpu().numpy()[slots] - p64).max() / scale)
        print("PERD3QN batch %d: max |priority - float64| / scale %.3g (scale %.4g), prio_max %.6g" % (batch, perr, scale, l.prio_max.item()))
    for name, a, b in zip(mod.NAMES, got, g64):
        assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max(), name
    assert abs(loss - loss64) <= 1e-5 * abs(loss64)
    if method == "PERD3QN":
        assert perr <= 1e-5
        pri = l.priority.cpu().numpy()
        assert l.prio_max.item() == pri.max() > SENTINEL and (np.delete(pri, slots) == SENTINEL).all()
    assert r["state"].tolist() == [1, 1] and r["params"].tobytes() != w.tobytes() and r["target"].tobytes() == (r["params"] if method == "DQN" else tgt).tobytes()
    assert r["packed"].tobytes() == _host_pack(r["params"], getattr(_lib, method)).tobytes()


@pytest.mark.parametrize("method", ["D3QN", "DQN"])
def test_adam_at_step_ten_thousand_on_moments_that_are_not_zero(worlds, method):
    """state[0] = 9999, adam_m ~ N(0, 1e-3), adam_v the squares of another N(0, 1e-3) draw, the fixture's initial parameters, one step:
    every parameter within 1e-5 lr + 1 ulp of adam64(p, m, v, kernel_grad, t = 10000), m and v within 1 ulp of the float64 values,
    state [10000, 1].  With these moments m / sqrt(v) has heavy tails -- the largest step is 8,120 lr (D3QN) and 2,140 lr (DQN) -- and
    m + 0.1 (g - m) cancels where g is near -9 m.  An update made of float32 operations (torch's own, learn_d3qn_cases.adam32; the
    kernels' until adam_update took double arithmetic) misses these bars: measured on an MI355X, parameters 2.2 / 3.52 times the bound,
    m up to 19,700 ulp, v up to 2.31 ulp.  Its distance from the kernel is printed."""
    import torch
    mod, g = _fixture_of(method)
    m0, v0 = dc.adam_moments(mod.N_PARAMS)
    batch = 32 if method == "DQN" else 64
    l = _learner(method, ring=_ring(g), batch=batch, params=g["init"], target=g["init"] if method == "DQN" else g["target_init"], want_grad=True)
    l.adam_m.copy_(torch.as_tensor(m0, device=DEV))
    l.adam_v.copy_(torch.as_tensor(v0, device=DEV))
    l.state[0] = 9999
    worlds.learn([l], 1, slots=g["slots"][0].reshape(1, 1, batch))
    r = _np(l)
    worlds.check_error_flag()
    grad = l.grad[0].cpu().numpy()
    p64, m64, v64 = mod.adam64(g["init"].astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), grad.astype(np.float64), 10000, l.lr)
    ulp = lambda x: np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)  # noqa: E731
    perr, bound = np.abs(r["params"] - p64), 1e-5 * l.lr + ulp(r["params"])
    merr, verr = np.abs(r["adam_m"] - m64) / ulp(m64), np.abs(r["adam_v"] - v64) / ulp(v64)
    p32, m32, v32 = dc.adam32(g["init"], m0, v0, grad, 10000, l.lr)
    step = np.abs(p64 - g["init"]) / l.lr
    print("%s Adam at t = 10000: worst |p - float64| / (1e-5 lr + 1 ulp) %.3g (%d of %d beyond the bound; largest step %.3g lr); m: worst %.3g ulp (%d beyond 1); "
          "v: worst %.3g ulp (%d beyond 1); against a float32 update: %d parameters, %d m, %d v differ in bits"
          % (method, (perr / bound).max(), int((perr > bound).sum()), perr.size, step.max(), merr.max(), int((merr > 1).sum()), verr.max(), int((verr > 1).sum()),
             int((r["params"] != p32).sum()), int((r["adam_m"] != m32).sum()), int((r["adam_v"] != v32).sum())))
    assert r["state"].tolist() == [10000, 1]
    assert (perr <= bound).all()
    assert (merr <= 1).all() and (verr <= 1).all()


# ---- 4. long rings under the update kernels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("method, capacity", [("D3QN", 10000), ("PERD3QN", 10000), ("DQN", 5000)])
def test_rows_at_the_top_of_a_long_ring_train_like_the_fixture_ring(worlds, method, capacity):
    """The fixture's rows at the last slots of a long ring of zero rows (count = capacity), three steps on slots + offset: every buffer,
    gradient and loss byte for byte the short ring's run; PERD3QN: the priorities of the top rows are the short run's, every row
    below keeps its fill, and so does the maximum."""
    mod, g = _fixture_of(method)
    n = g["ring_state"].shape[0]
    at = capacity - n
    batch = g["slots"].shape[1]
    slots = g["slots"][:3].astype(np.int32)
    names = BUFFERS + ("grad", "loss") + (("priority", "prio_max") if method == "PERD3QN" else ())
    out = []
    for rows, off in ((g, 0), (lc.relocated(g, capacity, at), at)):
        l = _learner(method, ring=_ring(rows), batch=batch, params=g["init"], target=g["init"] if method == "DQN" else g["target_init"],
                     want_grad=True, n_steps=3)
        if method == "PERD3QN":
            _prime(l, l.ring, np.full(rows["ring_state"].shape[0], SENTINEL, np.float32))
        worlds.learn([l], 3, slots=(slots + off).reshape(1, 3, batch))
        out.append(_np(l, names))
    worlds.check_error_flag()
    short, long_ = out
    for k in BUFFERS + ("grad", "loss"):
        assert short[k].tobytes() == long_[k].tobytes(), k
    assert short["state"].tolist() == [3, 1] and short["params"].tobytes() != g["init"].tobytes() and short["grad"].any()
    if method == "PERD3QN":
        assert long_["priority"][at:].tobytes() == short["priority"].tobytes() and (long_["priority"][:at] == SENTINEL).all()
        assert long_["prio_max"].tobytes() == short["prio_max"].tobytes() and short["prio_max"][0] == short["priority"].max() > SENTINEL


def test_the_maximum_is_retaken_over_every_row_of_a_long_ring(worlds):
    """10,000 rows at the sentinel priority and one row at 9.0, first, at the seams of the 512-thread loop, in the middle and last:
    after a one-step call prio_max is priority[:size].max() exactly -- 9.0; with count 9000 and the 9.0 at row 9500, beyond the size,
    it is the batch's own largest priority."""
    g = dc.golden()
    at = 2000
    rows = lc.relocated(g, 10000, at)
    slots = (g["slots"][0].astype(np.int32) + at).reshape(1, 1, 64)
    l = _learner("PERD3QN", ring=_ring(rows), batch=64, params=g["init"], target=g["target_init"])
    for count, r in ((10000, 0), (10000, 511), (10000, 512), (10000, 5000), (10000, 9999), (9000, 9500)):
        l.ring["count"].fill_(count)
        pri = np.full(10000, SENTINEL, np.float32)
        pri[r] = 9.0
        _prime(l, l.ring, pri)
        l.prio_max.fill_(1.0)
        worlds.learn([l], 1, slots=slots)
        got = _np(l, ("priority", "prio_max"))
        size = min(count, 10000)
        print("count %d, 9.0 at row %d: prio_max %.6g, priority[:size].max() %.6g" % (count, r, got["prio_max"][0], got["priority"][:size].max()))
        assert got["prio_max"][0] == got["priority"][:size].max()
        assert got["priority"][r] == 9.0 and (got["prio_max"][0] == 9.0) == (r < size)
        if r >= size:
            assert SENTINEL < got["prio_max"][0] == got["priority"][slots.reshape(-1)].max() < 9.0
    worlds.check_error_flag()
