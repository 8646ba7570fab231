"""The world shapes at which the world kernels are most likely to go wrong (shared by tests/test_world_shapes_cpu.py and
tests/test_hip_world_shapes.py): the narrowest, the longest and the fullest grids rl_create accepts (sides 3 .. 255, at most 4,096 cells).

width = number of columns (a_j < width), height = number of rows (a_i < height).  Every row carries what the library is expected to answer
for it: the slot capacity rl_create is given, rl_run_supported for the dueling pair (PERD3QN + D3QN) and for mixed kinds (PPO + DQN), and the
row stride the multi-tick kernel lays its observation planes out with -- restated here from plane_stride (reinlife_amd/csrc/rl_world_dev.h):
the next S = 7 (mod 32) at or above the width, unless the padding of the three float planes would cost more than 16 KB.  The launch also
falls back to row-major planes when the padded carve-out would exceed 160 KB of LDS (host_plane_stride, rl_run.hip); run_lds_bytes below
restates that arithmetic, and tests/test_world_shapes_cpu.py shows with it that every row keeps its padded stride (64x64 at slot_cap 512 with
the dueling pair: 135 KB)."""
import collections

import numpy as np

Case = collections.namedtuple("Case", "width height max_agents n_new thr slot_cap run_dueling run_mixed stride why")

CASES = [
    Case(3, 3, 4, 4, 3, 64, 1, 1, 7, "minimum; planes of stride 7 on a width of 3"),
    Case(4, 6, 8, 8, 6, 64, 1, 1, 7, "both sides below the 7-wide window: every window sees cells twice"),
    Case(6, 4, 8, 8, 6, 64, 1, 1, 7, "the same, transposed"),
    Case(7, 7, 12, 12, 9, 64, 1, 1, 7, "W & 31 == 7: padded stride == width"),
    Case(39, 39, 100, 100, 92, 256, 1, 1, 39, "W & 31 == 7 at a size with several policy tiles"),
    Case(255, 3, 60, 60, 55, 128, 1, 1, 263, "8-bit coordinate maximum on the column axis, minimum on the row axis"),
    Case(3, 255, 60, 60, 55, 128, 1, 1, 7, "8-bit coordinate maximum on the row axis, minimum on the column axis"),
    Case(255, 16, 100, 100, 92, 256, 1, 1, 263, "4,080 cells (not a multiple of 64); stride 263"),
    Case(16, 255, 100, 100, 92, 256, 1, 1, 16, "4,080 cells; padding refused: row-major planes"),
    Case(128, 32, 100, 100, 92, 256, 1, 1, 135, "4,096 cells, stride 135"),
    Case(65, 63, 250, 250, 235, 512, 1, 0, 71, "4,095 cells: cell / W by reciprocal at its largest argument with an odd width; six and more policy tiles"),
    Case(64, 64, 250, 250, 235, 512, 1, 0, 71, "the fullest LDS: dueling kinds run the multi-tick kernel, mixed kinds fall back"),
]
STRIDES = [7, 7, 7, 7, 39, 263, 7, 263, 16, 135, 71, 71]   # (CASES' stride column, as the issue of this table lists it)
TICKS = 40


def case_id(c):
    return "%dx%d" % (c.width, c.height)


def n_worlds(c):
    return 4 if c.max_agents >= 250 else 6


def plane_stride(width, height):
    """plane_stride(W, H) of rl_world_dev.h."""
    s = width
    while (s & 31) != 7:
        s += 1
    return s if (s - width) * height * 12 <= 16 * 1024 else width


def slot_cap_for(max_agents):
    """The capacity DeviceWorlds and OracleWorlds pick by themselves: births can overshoot max_agents up to 2n + 1."""
    return (2 * max_agents + 2 + 63) // 64 * 64


def world_seed(c):
    return 1000 * c.width + c.height


def is_static(c):
    """Static families on the even rows of the table, non-static on every second row."""
    return CASES.index(c) % 2 == 0


# The two input settings under which tests/test_hip_world_shapes.py steps worlds with seeded random actions -- the split step + update (a refill
# every 10 ticks) and the fused tick with refill (a refill behind every tick): keyword arguments of run_oracle, which the GPU tests read from
# here as well, so that tests/test_world_shapes_cpu.py asserts its preconditions on the very trajectories the kernels are stepped through
SETTINGS = {"split": dict(world_base=0, refill_every=10), "fused": dict(world_base=0, refill_every=1)}

LDS_BYTES = 160 * 1024


def _a16(x):
    return (x + 15) & ~15


def world_lds_bytes(c, stride):
    """carve() of rl_world_dev.h restated: the LDS of one world of shape c with observation planes of row stride `stride`."""
    cap, cells = c.slot_cap, c.width * c.height
    cp = (cells + 63) & ~63
    hs = 64
    while hs < 2 * cap:
        hs <<= 1
    pp = max((stride * c.height + 63) & ~63, cp)
    sizes = [8 * 64] * 3 + [8 * 16] * 2 + [8 * cap] * 3 + [4 * 64] * 2 + [4 * 24] + [4 * 16] * 3 + [4 * 64] + [4 * hs] * 2 + [4 * pp] * 3 + [4 * cap] * 6 + \
            [2 * cp] + [2 * cap] * 7 + [2 * cp] + [cp] + [cap] * 3
    return sum(_a16(n) for n in sizes)


def run_lds_bytes(c, stride, n_brains, mixed=False):
    """Upper bound of the multi-tick launch's LDS at 512 threads (carve_policy of rl_run.hip: the Agent.state mirror takes only what is left below
    160 KB, so the world and `tail` decide): the world, the row lists, tile descriptors and Tracker scratch (10 * cap + 5120), the tiles' small
    exchanges (4 tiles x 160 floats, 384 for mixed kinds) and the brains' epilogue constants (804 floats per brain, 1040 for mixed kinds)."""
    tail = 10 * c.slot_cap + 5120 + 4 * 4 * (384 if mixed else 160) + 4 * (1040 if mixed else 804) * n_brains
    return _a16(world_lds_bytes(c, stride)) + tail


def config(c, n_brains=3, static=True, **over):
    cfg = dict(width=c.width, height=c.height, max_agents=c.max_agents, n_brains=n_brains, static_families=static, limit_reproduction=False,
               incentivize_killing=True, slot_cap=c.slot_cap)
    cfg.update(over)
    return cfg


def positions(ow):
    """-> per world {uid: (a_i, a_j)} of an OracleWorlds' agents."""
    out = []
    for w in range(ow.R):
        n = int(ow.s["n_agents"][w])
        out.append({int(u): (int(i), int(j)) for u, i, j in zip(ow.s["a_uid"][w, :n], ow.s["a_i"][w, :n], ow.s["a_j"][w, :n])})
    return out


def seam_crossings(before, after, height, width):
    """before, after: positions() of two oracle states one tick apart (same epoch) -> (row-seam crossings, column-seam crossings): the agents,
    matched by uid, whose a_i changed by height - 1 resp. whose a_j changed by width - 1 (a move is one cell: only a wrap gives that)."""
    rows = cols = 0
    for b, a in zip(before, after):
        for uid, (i0, j0) in b.items():
            if uid in a:
                rows += abs(a[uid][0] - i0) == height - 1
                cols += abs(a[uid][1] - j0) == width - 1
    return rows, cols


def run_oracle(c, ticks=TICKS, n_brains=3, static=True, seed=None, actions=None, world_base=0, refill_every=1):
    """The loop of the CPU preconditions: n_worlds(c) oracle worlds of shape c from reset_synthetic(c.n_new), `ticks` ticks of seeded random
    actions (RandomState(100 * W + H), or actions(t, ow) -> [R, cap] int8), a refill at c.thr behind every refill_every-th tick.
    -> dict(rows, cols: seam crossings; max_i, max_j: the largest coordinates an agent stood on; births, vanished, refills)."""
    from oracle import oracle as orc
    R = n_worlds(c)
    ow = orc.OracleWorlds(n_worlds=R, seed=world_seed(c) if seed is None else seed, world_base=world_base, **config(c, n_brains, static))
    ow.reset_synthetic(c.n_new)
    rng = np.random.RandomState(100 * c.width + c.height)
    st = dict(rows=0, cols=0, max_i=0, max_j=0, births=0, vanished=0, refills=0)

    def stood(ow):
        for w in range(R):
            n = int(ow.s["n_agents"][w])
            if n:
                st["max_i"] = max(st["max_i"], int(ow.s["a_i"][w, :n].max()))
                st["max_j"] = max(st["max_j"], int(ow.s["a_j"][w, :n].max()))
    stood(ow)
    for t in range(ticks):
        acts = rng.randint(0, 8, size=(R, ow.cap)).astype(np.int8) if actions is None else actions(t, ow)
        before = positions(ow)
        n0 = ow.s["n_agents"].copy()
        ow.step(acts)
        n1 = ow.s["n_agents"].copy()
        ow.update()
        r, k = seam_crossings(before, positions(ow), c.height, c.width)
        st["rows"] += r; st["cols"] += k
        st["vanished"] += int((n0 - n1).sum())
        st["births"] += int(sum((ow.src2[w, : ow.s["n_agents"][w]] < 0).sum() for w in range(R)))
        stood(ow)
        if t % refill_every == refill_every - 1:
            st["refills"] += ow.refill(c.thr, c.n_new)
            stood(ow)
    return st
