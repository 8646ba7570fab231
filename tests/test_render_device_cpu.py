"""CPU: everything of the device painter (rl_render, include/reinlife_hip.h) that needs no GPU -- the ABI entry and its host-side
validation, Visualize.geometry() / style() / mosaic() -- and the PREMISE of tests/test_hip_render.py: a frame is a pure function of each
pixel's cell.  A numpy restatement of the kernel's five-step rule equals the rectangle painter (Visualize.frame, pinned to the reference's
rectangles by tests/test_render_cpu.py) on the recorded fixtures and on seeded random states, consistent and inconsistent."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from reinlife_amd import _lib
from reinlife_amd.Helpers.render import RenderFeed, Visualize, mosaic
from reinlife_amd.World.utils import EntityTypes

import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rule_frame(viz, snap):
    """The five-step rule of rl_render.hip, per pixel, in numpy.  `viz` has its background."""
    geo, gs, H, W = viz.geometry(), viz.grid_size, viz.height, viz.width
    ct = np.asarray(snap["cell_type"]).reshape(H, W)
    win = np.full((H, W), -1, np.int64)
    for k in range(len(snap["i"])):   # the LAST live entry on the grid wins its cell
        i, j = int(snap["i"][k]), int(snap["j"][k])
        if not (int(snap["flags"][k]) & _lib.F_DEAD) and i < H and j < W:
            win[i, j] = k
    body = np.zeros((H, W, 3), np.uint8)
    border = np.zeros((H, W, 3), np.uint8)
    for i, j in zip(*np.nonzero(win >= 0)):
        k = win[i, j]
        col = np.asarray(viz.colors[int(snap["gene"][k]) % len(viz.colors)], np.float64)
        body[i, j] = np.clip(col, 0, 255).astype(np.uint8)
        if int(snap["flags"][k]) & _lib.F_KILLED:
            border[i, j] = (255, 0, 0)
        else:
            border[i, j] = np.clip(col * (1 - int(snap["health"][k]) / 205), 0, 255).astype(np.uint8)
    p = np.arange(gs)

    def square(x0, y0, side):
        m = np.zeros((gs, gs), bool)   # [py, px]
        if side > 0:
            m[np.ix_((p >= y0) & (p < y0 + side), (p >= x0) & (p < x0 + side))] = True
        return m

    bo, bs, bw = geo["body_off"], geo["body_size"], geo["border"]
    body_m = square(bo, bo, bs)
    inner = square(bo + bw, bo + bw, bs - 2 * bw) if 2 * bw < bs else np.zeros((gs, gs), bool)
    border_m = body_m & ~inner
    eye_m = square(geo["eye_x0"], geo["eye_y"], geo["eye_size"]) | square(geo["eye_x1"], geo["eye_y"], geo["eye_size"])
    food_m = square(geo["food_off"], geo["food_off"], geo["food_size"])
    I, J = np.arange(H * gs) // gs, np.arange(W * gs) // gs
    PY, PX = np.arange(H * gs) % gs, np.arange(W * gs) % gs

    def px(mask):   # [gs, gs] -> [Hpx, Wpx]
        return mask[np.ix_(PY, PX)]

    def cells(a):   # [H, W, ...] -> [Hpx, Wpx, ...]
        return a[np.ix_(I, J)]

    img = cells(viz.background[::gs, ::gs]).copy()                            # 5 background
    has = cells(win >= 0)
    img[has & px(body_m)] = cells(body)[has & px(body_m)]                    # 4 body
    img[has & px(border_m)] = cells(border)[has & px(border_m)]              # 3 border
    img[has & px(eye_m)] = 0                                                  # 2 eyes
    for kind, color in ((EntityTypes.food, (255, 255, 255)), (EntityTypes.poison, (0, 0, 0)), (EntityTypes.super_food, (255, 0, 0))):
        img[cells(ct == int(kind)) & px(food_m)] = color                      # 1 food square
    return img


def _cpu_frame(viz, width, height, snap):
    return viz.frame(RenderFeed.from_world(width, height, snap))


def test_the_header_declares_rl_render_and_the_ctypes_table_lists_it():
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "rl_render          " in hdr[:hdr.index("#ifndef")] and "Helpers/render.py:51-239" in hdr[:hdr.index("#ifndef")]
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int rl_render\(rl_world\* h, const rl_render_style\* \w+, const int32_t\* \w+, int \w+, uint8_t\* \w+, void\* stream\);", code)
    assert "} rl_render_style;" in code
    entry = [e for e in _lib.ABI if e[0] == "rl_render"]
    assert len(entry) == 1 and entry[0][1] is C.c_int and len(entry[0][2]) == 6
    assert hasattr(_lib.lib(), "rl_render")
    # the struct mirrors the header: eleven int32, two pointers
    names = re.findall(r"\b(\w+)\s*[,;]", code[code.index("typedef struct {\n    int32_t grid_size"):code.index("} rl_render_style;")])
    assert names == [n for n, _ in _lib.RenderStyle._fields_]
    assert "5  rl_render" in hdr   # the new error-flag code is documented beside the others


def _handle(n_worlds=4):
    lib = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.Config(30, 30, 100, 2, 256, n_worlds, 1, 0, 1, 0, 0)
    assert lib.rl_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def test_rl_render_validates_on_the_host_and_names_the_argument():
    """None of these calls reaches a launch: an unbound handle, then (bound to host memory that no kernel will ever see) every bad argument."""
    lib, h = _handle()
    colors, tiles, frames = (C.c_double * 24)(), (C.c_uint8 * (30 * 30 * 3))(), (C.c_uint8 * 64)()

    def style(**kw):
        geo = Visualize(30, 30, 8).geometry()
        st = _lib.RenderStyle(**geo, n_colors=8, colors=C.addressof(colors), tiles=C.addressof(tiles))
        for k, v in kw.items():
            setattr(st, k, v)
        return st

    def call(st, worlds, n, fr):
        rc_ = lib.rl_render(h, C.byref(st) if st is not None else None, worlds, n, fr, None)
        return rc_, lib.rl_last_error().decode()

    try:
        rc_, err = call(style(), None, 1, frames)
        assert rc_ == -2 and "rl_render" in err and "rl_bind_state" in err            # RL_E_UNBOUND
        assert lib.rl_render(None, C.byref(style()), None, 1, frames, None) == -1
        backing = (C.c_uint8 * 64)()
        state = _lib.State(*[C.addressof(backing)] * len(_lib.STATE_FIELDS))
        assert lib.rl_bind_state(h, C.byref(state)) == 0
        for st, worlds, n, fr, word in ((None, None, 1, frames, "style"), (style(), None, 1, None, "frames"),
                                        (style(colors=None), None, 1, frames, "colors"), (style(tiles=None), None, 1, frames, "tiles"),
                                        (style(grid_size=0), None, 1, frames, "grid_size"), (style(grid_size=65), None, 1, frames, "grid_size"),
                                        (style(n_colors=0), None, 1, frames, "n_colors"), (style(), None, 0, frames, "n_frames"),
                                        (style(), None, -3, frames, "n_frames"), (style(), None, 5, frames, "n_worlds")):
            rc_, err = call(st, worlds, n, fr)
            assert rc_ == -1 and err.startswith("rl_render:") and word in err, (word, rc_, err)   # RL_E_INVALID
    finally:
        lib.rl_destroy(h)


@pytest.mark.parametrize("gs", range(1, 65))
def test_geometry_is_the_painters_expressions_and_stays_inside_the_cell(gs):
    geo = Visualize(4, 3, gs).geometry()
    assert geo == {"grid_size": gs, "body_off": max(1, int(gs / 8)), "body_size": gs - max(1, int(gs / 8) * 2), "border": 2,
                   "eye_size": gs - max(1, int(gs * .9)), "eye_y": max(1, int(gs / 3)), "eye_x0": max(1, int(gs / 3)),
                   "eye_x1": max(1, int(gs / 1.8)), "food_off": int(gs / 2.5), "food_size": gs - int(gs / 2.5) * 2}
    assert all(isinstance(v, int) for v in geo.values())
    # what makes a frame a function of each pixel's own cell: no rectangle reaches into a neighbour
    for off, size in ((geo["body_off"], geo["body_size"]), (geo["eye_x0"], geo["eye_size"]), (geo["eye_x1"], geo["eye_size"]),
                      (geo["eye_y"], geo["eye_size"]), (geo["food_off"], geo["food_size"])):
        assert off >= 0 and (size <= 0 or off + size <= gs), (gs, off, size)
    # and draw_list asks for exactly these rectangles
    snap = rc.full_snap([1], [2], [0], [100], [0], np.array([0] * 5 + [1] + [0] * 6))
    draws = Visualize(4, 3, gs).draw_list(RenderFeed.from_world(4, 3, snap))
    x, y = 2 * gs, 1 * gs
    assert [d[1:] for d in draws] == [
        ((x + geo["body_off"], y + geo["body_off"], geo["body_size"], geo["body_size"]), 0),
        ((x + geo["body_off"], y + geo["body_off"], geo["body_size"], geo["body_size"]), 2),
        ((x + geo["eye_x0"], y + geo["eye_y"], geo["eye_size"], geo["eye_size"]), 0),
        ((x + geo["eye_x1"], y + geo["eye_y"], geo["eye_size"], geo["eye_size"]), 0),
        ((1 * gs + geo["food_off"], 1 * gs + geo["food_off"], geo["food_size"], geo["food_size"]), 0)]


@pytest.mark.parametrize("pastel", [False, True])
def test_style_fields(pastel):
    random.seed(11)
    viz = Visualize(7, 5, 9, pastel=pastel)
    st = viz.style("cpu")
    assert viz.style("cpu") is st                                     # cached
    for k, v in viz.geometry().items():
        assert getattr(st, k) == v
    assert st.n_colors == len(viz.colors) == (100 if pastel else 8)
    colors, tiles = st._keep
    assert colors.dtype == torch.float64 and colors.data_ptr() == st.colors and tiles.dtype == torch.uint8 and tiles.data_ptr() == st.tiles
    assert colors.is_contiguous() and tiles.is_contiguous()
    assert np.array_equal(colors.numpy(), np.asarray(viz.colors, np.float64))
    assert tuple(tiles.shape) == (5, 7, 3)                             # [height][width][3]
    for i in range(5):
        for j in range(7):
            assert np.all(viz.background[i * 9:(i + 1) * 9, j * 9:(j + 1) * 9] == tiles.numpy()[i, j])


def test_building_the_style_first_takes_the_draws_the_first_frame_would_have_taken():
    snap = rc.full_snap([1], [2], [3], [100], [0], np.zeros(20))
    random.seed(5)
    a = Visualize(5, 4, 6, pastel=True)
    first = _cpu_frame(a, 5, 4, snap)
    after_frame = random.random()
    random.seed(5)
    b = Visualize(5, 4, 6, pastel=True)
    b.style("cpu")
    assert random.random() == after_frame
    assert np.array_equal(b.background, a.background)
    state = random.getstate()
    assert np.array_equal(_cpu_frame(b, 5, 4, snap), first) and b.style("cpu") is not None
    assert random.getstate() == state                                  # the background is built once


@pytest.mark.parametrize("name", rc.GOLDEN)
def test_the_rule_equals_the_rectangle_painter_on_the_golden_fixtures(name):
    meta, snaps = rc.golden_frames(name)
    random.seed(meta["seed"])
    viz = Visualize(meta["width"], meta["height"], meta["gs"], pastel=meta["pastel"])
    for snap in snaps:
        want = _cpu_frame(viz, meta["width"], meta["height"], snap)
        assert np.array_equal(rule_frame(viz, snap), want)


@pytest.mark.parametrize("gs", [1, 2, 3, 5, 7, 8, 9, 16, 24, 33])
def test_the_rule_equals_the_rectangle_painter_on_random_states(gs):
    rng = np.random.RandomState(1000 + gs)
    for case in range(6):
        width, height = int(rng.randint(3, 9)), int(rng.randint(3, 8))
        random.seed(case)
        viz = Visualize(width, height, gs, pastel=bool(case & 1))
        snap = rc.random_state(rng, width, height, int(rng.randint(0, 14)), consistent=case < 2)
        want = _cpu_frame(viz, width, height, snap)
        assert np.array_equal(rule_frame(viz, snap), want), (gs, case)


def test_mosaic():
    f = torch.arange(3 * 2 * 2 * 3, dtype=torch.uint8).reshape(3, 2, 2, 3) + 1   # three 2x2 frames, no zero byte
    m = mosaic(f, 2)
    assert tuple(m.shape) == (4, 4, 3) and m.dtype == torch.uint8
    assert torch.equal(m[0:2, 0:2], f[0]) and torch.equal(m[0:2, 2:4], f[1]) and torch.equal(m[2:4, 0:2], f[2])
    assert int(m[2:4, 2:4].abs().sum()) == 0                           # the missing tile is black
    assert torch.equal(mosaic(f, 3), torch.cat([f[0], f[1], f[2]], dim=1))
    assert torch.equal(mosaic(f, 1), torch.cat([f[0], f[1], f[2]], dim=0))
    assert tuple(mosaic(f, 5).shape) == (2, 10, 3)
    with pytest.raises(ValueError):
        mosaic(f, 0)
