"""World states for the painter tests (tests/test_render_device_cpu.py, tests/test_hip_render.py): seeded random ones, consistent (one
live agent per agent cell, as the kernels leave a world) and deliberately inconsistent (what load_world accepts: several agents on a
cell, agents on food, off-grid coordinates, any flags / health / gene), and the recorded frames of the render fixtures."""
import os

import numpy as np

from reinlife_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = ["render_30x30_gs24", "render_12x9_gs16_pastel", "render_20x20_gs7_genes"]
_FOODS = (_lib.FOOD, _lib.POISON, _lib.SUPER_FOOD)


def full_snap(i, j, gene, health, flags, cell_type):
    """A DeviceWorlds.load_world snapshot: the six arrays a frame depends on, zeros for the rest."""
    n = len(i)
    z = np.zeros(n, np.int32)
    return {"i": np.asarray(i, np.uint8), "j": np.asarray(j, np.uint8), "gene": np.asarray(gene, np.int32),
            "health": np.asarray(health, np.int32), "flags": np.asarray(flags, np.uint8),
            "cell_type": np.asarray(cell_type, np.uint8).reshape(-1),
            "age": z, "max_age": z, "brain": z, "uid": np.arange(n, dtype=np.int32), "action": np.zeros(n, np.int8),
            "fitness": np.zeros(n, np.float64)}


def random_state(rng, width, height, n, consistent):
    cells = width * height
    ct = np.zeros(cells, np.uint8)
    food = rng.rand(cells) < 0.25
    ct[food] = rng.choice(_FOODS, size=int(food.sum()))
    if consistent:
        n = min(n, cells)
        where = rng.choice(cells, size=n, replace=False)
        where.sort()
        ct[where] = _lib.AGENT
        i, j = where // width, where % width
        flags = np.where(rng.rand(n) < 0.2, _lib.F_KILLED, 0) | np.where(rng.rand(n) < 0.3, _lib.F_REPRODUCED, 0)
        health = rng.randint(1, 201, size=n)
        gene = rng.randint(0, 12, size=n)
    else:
        i = rng.randint(0, min(height + 2, 256), size=n)      # some below the grid
        j = rng.randint(0, min(width + 2, 256), size=n)       # some right of it
        if n > 3:                                              # several agents on one cell, whatever the cell holds
            i[n // 2:n // 2 + 2], j[n // 2:n // 2 + 2] = i[0], j[0]
        flags = rng.randint(0, 64, size=n)                     # dead, killed, dead + killed, ...
        health = rng.choice([-50, 0, 1, 41, 100, 200, 205, 400], size=n)
        gene = rng.randint(0, 300, size=n)
    return full_snap(i, j, gene, health, flags, ct)


def golden_frames(name):
    """(meta dict, [snap per recorded frame]) of a render fixture."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    seed, width, height, gs, pastel, n_brains, frames = [int(v) for v in g["meta"]]
    snaps = [full_snap(*[g["frame%d_%s" % (f, k)] for k in ("i", "j", "gene", "health", "flags", "cell_type")]) for f in range(frames)]
    return dict(seed=seed, width=width, height=height, gs=gs, pastel=bool(pastel)), snaps
