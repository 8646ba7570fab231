"""GPU: rl_render / DeviceWorlds.render / Environment.frames / Environment.record / tester(render="device") paint byte for byte what the
CPU painter paints from the same state: every comparison is np.array_equal against Visualize.frame(RenderFeed.from_world(...)), which
tests/test_render_cpu.py pins to the reference's rectangles (and tests/test_render_device_cpu.py to the kernel's per-pixel rule)."""
import ctypes as C
import random

import numpy as np
import pytest

import render_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 64


def _cap_for(n):
    cap = max(64, (n + 63) // 64 * 64)
    return cap, (cap - 2) // 2


def _worlds(width, height, snaps, cap=None):
    """One handle with one world per snapshot."""
    from reinlife_amd.worlds import DeviceWorlds
    cap, max_agents = _cap_for(max([len(s["i"]) for s in snaps] + [cap or 0]))
    dw = DeviceWorlds(n_worlds=len(snaps), width=width, height=height, max_agents=max_agents, slot_cap=cap)
    for w, s in enumerate(snaps):
        dw.load_world(w, s)
    return dw


def _cpu(viz, snap):
    from reinlife_amd.Helpers.render import RenderFeed
    return viz.frame(RenderFeed.from_world(viz.width, viz.height, snap))


def _guarded(dw, gs, n, lead=GUARD):
    """A frame buffer for n frames inside a larger one: `lead` (>= 64) bytes of 0xA5 before it and 64 behind."""
    import torch
    shape = (n, dw.H * gs, dw.W * gs, 3)
    nbytes = int(np.prod(shape))
    big = torch.full((lead + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=dw.device)
    return big, big[lead:lead + nbytes].view(shape)


def _guards_intact(big, lead=GUARD):
    return bool((big[:lead] == 0xA5).all()) and bool((big[-GUARD:] == 0xA5).all())


@pytest.mark.parametrize("name", rc.GOLDEN)
def test_golden_frames(name):
    from reinlife_amd.Helpers.render import Visualize
    meta, snaps = rc.golden_frames(name)
    random.seed(meta["seed"])   # like tests/test_render_cpu.py: the painter's colours and tiles come from `random`
    np.random.seed(meta["seed"])
    viz = Visualize(meta["width"], meta["height"], meta["gs"], pastel=meta["pastel"])
    dw = _worlds(meta["width"], meta["height"], snaps)
    got = dw.render(viz.style(dw.device)).cpu().numpy()   # every recorded frame in ONE call
    assert got.shape == (len(snaps), meta["height"] * meta["gs"], meta["width"] * meta["gs"], 3) and got.dtype == np.uint8
    for w, s in enumerate(snaps):
        assert np.array_equal(got[w], _cpu(viz, s)), (name, w)
    dw.check_error_flag()


@pytest.mark.parametrize("lead", [64, 67])
@pytest.mark.parametrize("width,height,gs,n", [(3, 3, 1, 4), (5, 4, 7, 3), (7, 5, 3, 3), (255, 10, 3, 2), (10, 255, 3, 2), (64, 64, 5, 2),
                                               (30, 30, 33, 2), (40, 3, 64, 2), (50, 3, 64, 2)])
def test_smallest_shapes_at_which_the_stores_can_go_wrong(width, height, gs, n, lead):
    """27-byte frames, 105-byte rows, odd row lengths, one column / one row of bands, a whole world per band and many bands per world,
    and the two widest: 40 cells of 64 pixels are the last whose scanlines fit into the kernel's LDS lines, 50 take its direct form:
    every frame right, and not a byte outside frames[0 : n * frame_bytes] touched (64 guard bytes on each side; lead = 67 also puts the
    buffer itself off every alignment)."""
    from reinlife_amd.Helpers.render import Visualize
    rng = np.random.RandomState(width * 1000 + height * 10 + gs)
    random.seed(gs)
    viz = Visualize(width, height, gs, pastel=bool(gs & 1))
    snaps = [rc.random_state(rng, width, height, int(rng.randint(1, 60)), consistent=(w == 0)) for w in range(n)]
    dw = _worlds(width, height, snaps)
    big, out = _guarded(dw, gs, n, lead)
    got = dw.render(viz.style(dw.device), out=out)
    assert got is out
    host = got.cpu().numpy()
    for w, s in enumerate(snaps):
        assert np.array_equal(host[w], _cpu(viz, s)), (width, height, gs, w)
    assert _guards_intact(big, lead)
    dw.check_error_flag()


@pytest.mark.parametrize("pastel", [False, True])
def test_inconsistent_states(pastel):
    """Whatever load_world accepts, the CPU painter defines the frame."""
    from reinlife_amd import _lib
    from reinlife_amd.Helpers.render import Visualize
    width, height, gs, cap = 6, 5, 8, 64
    random.seed(77)
    viz = Visualize(width, height, gs, pastel=pastel)
    nc = len(viz.colors)
    empty = np.zeros(width * height, np.uint8)
    food = empty.copy()
    food[1 * width + 2], food[3 * width + 4], food[0] = _lib.FOOD, _lib.POISON, _lib.SUPER_FOOD
    D, K = _lib.F_DEAD, _lib.F_KILLED
    rng = np.random.RandomState(9)
    snaps = [
        rc.full_snap([2, 4, 2], [3, 1, 3], [1, 2, 5], [200, 100, 40], [0, 0, 0], empty),                 # 0 two live agents on (2, 3): the later wins
        rc.full_snap([2, 2, 2], [3, 3, 3], [1, 5, 2], [200, 40, 90], [0, 0, D], empty),                  # 1 ... the later LIVE one: a dead entry behind it does not
        rc.full_snap([1, 3, 0], [2, 4, 0], [0, 1, 2], [150, 60, 10], [0, K, 0], food),                   # 2 agents on food cells
        rc.full_snap([height, 2, 255, 1], [1, width, 255, 1], [0, 1, 2, 3], [100] * 4, [0] * 4, empty),  # 3 a_i >= height, a_j >= width
        rc.full_snap([0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], [120] * 4, [D, K, D | K, 0], empty),      # 4 dead, killed, dead + killed
        rc.full_snap([0, 1, 2, 3], [1, 2, 3, 4], [3, 3, 3, 3], [-50, 0, 205, 400], [0] * 4, empty),      # 5 health below 0, 0, 205, above 205
        rc.full_snap([0, 1, 2, 3], [1, 2, 3, 4], [nc, nc + 1, 7 * nc + 3, 2 ** 31 - 1], [90] * 4, [0] * 4, empty),   # 6 genes beyond n_colors
        rc.full_snap([], [], [], [], [], food),                                                          # 7 n_agents == 0
        rc.random_state(rng, width, height, cap, consistent=False),                                      # 8 n_agents == slot_cap
    ]
    dw = _worlds(width, height, snaps, cap=cap)
    assert dw.cap == cap and len(snaps[8]["i"]) == cap
    # beyond n_agents the arrays hold live agents that are NOT in the list: they must not be painted
    dw.s["a_i"][7, :] = 2; dw.s["a_j"][7, :] = 2; dw.s["a_flags"][7, :] = 0
    got = dw.render(viz.style(dw.device)).cpu().numpy()
    for w, s in enumerate(snaps):
        assert np.array_equal(got[w], _cpu(viz, s)), w
    inside = (2 * gs + 4, 3 * gs + 3)   # a body pixel of cell (2, 3), off the border and the eyes
    for w in (0, 1):
        assert np.array_equal(got[w][inside], np.clip(np.asarray(viz.colors[5 % nc]), 0, 255).astype(np.uint8)), w
    dw.check_error_flag()


def test_world_selection_out_reuse_and_bad_ids():
    import torch
    from reinlife_amd import _lib
    from reinlife_amd.Helpers.render import Visualize
    width, height, gs = 7, 5, 6
    rng = np.random.RandomState(4)
    random.seed(4)
    viz = Visualize(width, height, gs)
    snaps = [rc.random_state(rng, width, height, 12, consistent=True) for _ in range(6)]
    dw = _worlds(width, height, snaps)
    style = viz.style(dw.device)
    want = np.stack([_cpu(viz, s) for s in snaps])
    for ids in ([1, 4], [5, 4, 3, 2, 1, 0], [2, 2, 0, 2, 5, 5, 5], (3,), np.array([4, 0]), torch.tensor([1, 1, 2]),
                torch.tensor([5, 0], dtype=torch.int32, device=dw.device)):
        got = dw.render(style, ids)
        index = [int(x) for x in ids]
        assert tuple(got.shape) == (len(index), height * gs, width * gs, 3) and got.dtype == torch.uint8 and got.device == dw.s["tick"].device
        assert np.array_equal(got.cpu().numpy(), want[index]), ids
    assert np.array_equal(dw.render(style, None).cpu().numpy(), want)
    out = torch.zeros((2, height * gs, width * gs, 3), dtype=torch.uint8, device=dw.device)
    again = dw.render(style, [0, 1], out=out)
    assert again is out and again.data_ptr() == out.data_ptr() and np.array_equal(out.cpu().numpy(), want[:2])
    assert dw.render(style, [3, 2], out=out) is out and np.array_equal(out.cpu().numpy(), want[[3, 2]])
    for bad in ([0, 6], [-1], [2, 10 ** 6]):
        with pytest.raises(IndexError):
            dw.render(style, bad)
    with pytest.raises(ValueError):
        dw.render(style, [0, 1, 2], out=out)            # wrong shape
    with pytest.raises(ValueError):
        dw.render(style, [])
    dw.check_error_flag()
    # the raw C call: a bad id leaves ITS frame as it was, sets the error flag (code 5, the id, the frame), and the other frames are painted
    ids = torch.tensor([0, 99, 1, -7], dtype=torch.int32, device=dw.device)
    raw = torch.full((4, height * gs, width * gs, 3), 0x5A, dtype=torch.uint8, device=dw.device)
    stream = C.c_void_p(torch.cuda.current_stream(dw.device).cuda_stream)
    assert dw.lib.rl_render(dw.handle, C.byref(style), C.c_void_p(ids.data_ptr()), 4, C.c_void_p(raw.data_ptr()), stream) == 0
    host = raw.cpu().numpy()
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[2], want[1])
    assert np.all(host[1] == 0x5A) and np.all(host[3] == 0x5A)
    err = dw.err.cpu().numpy()
    assert err[0] == 5 and (int(err[1]), int(err[2])) in ((99, 1), (-7, 3))
    with pytest.raises(_lib.ReinLifeHipError):
        dw.check_error_flag()
    dw.err.zero_()
    # NULL worlds with more frames than worlds: refused on the host
    assert dw.lib.rl_render(dw.handle, C.byref(style), None, 7, C.c_void_p(raw.data_ptr()), stream) == -1
    assert b"n_frames" in dw.lib.rl_last_error()


def test_rendering_leaves_the_state_untouched():
    import torch
    from reinlife_amd.Helpers.render import Visualize
    rng = np.random.RandomState(12)
    random.seed(12)
    viz = Visualize(9, 8, 5, pastel=True)
    dw = _worlds(9, 8, [rc.random_state(rng, 9, 8, 20, consistent=bool(w & 1)) for w in range(5)])
    before = dw._arena.clone()
    dw.render(viz.style(dw.device))
    dw.render(viz.style(dw.device), [4, 0, 4])
    torch.cuda.synchronize()
    assert torch.equal(dw._arena, before)


def test_byte_offsets_beyond_two_to_the_31():
    """2,048 frames of 30x30 at grid_size 24 are 3.2e9 bytes: the frames behind byte 2^31 are those of the worlds they name."""
    import torch
    from reinlife_amd.Helpers.render import Visualize
    width = height = 30
    gs, n = 24, 2048
    rng = np.random.RandomState(24)
    random.seed(24)
    viz = Visualize(width, height, gs)
    snaps = [rc.random_state(rng, width, height, 60, consistent=True) for _ in range(4)]
    dw = _worlds(width, height, snaps)
    ids = torch.arange(n, dtype=torch.int32, device=dw.device) % 4
    out = dw.render(viz.style(dw.device), ids)
    assert out.numel() > 2 ** 31
    first = out[:4].reshape(1, 4, -1)
    for c in range(0, n, 256):
        assert bool((out[c:c + 256].reshape(64, 4, -1) == first).all()), c
    host = out[n - 4:].cpu().numpy()
    for w, s in enumerate(snaps):
        assert np.array_equal(host[w], _cpu(viz, s)), w
    del out, first
    torch.cuda.empty_cache()


def _env(brains, **kw):
    from reinlife_amd import Environment
    return Environment(width=12, height=9, brains=brains, grid_size=8, max_agents=40, training=False, n_worlds=8, rng="philox",
                       seed=5, synthetic_agents=14, **kw)


def _brains():
    from reinlife_amd import Models
    return [Models.DQN(training=False), Models.D3QN(training=False)]


def test_live_worlds_frames_equal_the_cpu_painter():
    import torch
    brains = _brains()
    random.seed(21)
    env = _env(brains)
    env.reset()
    n_epi = 0
    for ticks in (1, 4, 7, 8, 10):   # 30 ticks, looked at five times
        env.run(n_epi, ticks)
        n_epi += ticks
        got = env.frames()
        assert tuple(got.shape) == (8, 9 * 8, 12 * 8, 3) and got.dtype == torch.uint8 and got.is_cuda
        host = got.cpu().numpy()
        for w in range(8):
            assert np.array_equal(host[w], env.viz.frame(env.render_feed(w))), (n_epi, w)
    assert env.frame is None   # frames() is not render(): env.frame stays what render() left


def test_record_equals_the_loop_of_run_and_frames():
    import torch
    from reinlife_amd import Environment
    brains = _brains()
    random.seed(22)
    a = _env(brains)
    a.reset()
    a.run(0, 3)
    before = a.frames((0, 3, 7)).clone()
    film = a.record(12, worlds=(0, 3, 7), every=4, n_epi=3)
    assert tuple(film.shape) == (4, 3, 9 * 8, 12 * 8, 3) and film.dtype == torch.uint8
    assert torch.equal(film[0], before)                      # frame 0: the state at the call
    random.seed(22)
    b = _env(brains)
    b.reset()
    b.run(0, 3)
    loop, n_epi = [b.frames((0, 3, 7)).clone()], 3
    for _ in range(3):
        b.run(n_epi, 4)
        n_epi += 4
        loop.append(b.frames((0, 3, 7)).clone())
    assert torch.equal(film, torch.stack(loop))
    assert not torch.equal(film[0], film[3])                 # (the worlds moved)
    out = torch.empty_like(film)
    assert a.record(0, worlds=(0, 3, 7), out=out[:1]).data_ptr() == out.data_ptr() and torch.equal(out[0], film[3])
    with pytest.raises(ValueError, match="philox"):
        Environment(width=12, height=9, brains=brains, grid_size=8, training=False).record(4)


def test_tester_paints_the_same_frames_with_either_painter():
    from reinlife_amd import tester
    brains = _brains()
    films = {}
    for how in ("device", "host"):
        random.seed(3)   # the background tiles come from `random`, world 0 of reset() from np.random
        np.random.seed(3)
        seen = []
        env = tester(brains, n_steps=5, n_worlds=2, seed=3, render=how, on_frame=lambda e: seen.append(e.frame.copy()))
        assert len(seen) == 5 and isinstance(env.frame, np.ndarray) and env.frame.dtype == np.uint8 and env.frame.shape == (720, 720, 3)
        films[how] = np.stack(seen)
    assert np.array_equal(films["device"], films["host"])
    assert not np.array_equal(films["host"][0], films["host"][4])
    with pytest.raises(ValueError):
        tester(brains, n_steps=1, render="gpu")
