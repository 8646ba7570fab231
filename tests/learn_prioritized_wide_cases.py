"""Shared by tests/test_learn_prioritized_wide_cpu.py and tests/test_hip_learn_prioritized_wide.py: seeded slot tables on the 96-row
fixture ring (tests/learn_dueling_wide_cases.py's), the float64 priorities of a WHOLE wide minibatch (learn_perd3qn_cases.priorities,
computed once per batch and left unchanged), the plausible-but-wrong model that takes the advantage mean per 64-row tile, the slot
tables of the duplicate tests, and the case of the wide draw's statistics."""
import numpy as np

import learn_d3qn_cases as dc
import learn_dueling_wide_cases as wc
import learn_perd3qn_cases as pc

WIDE_MAX = 2048           # RL_LEARN_PRIORITIZED_WIDE_MAX
TILE = wc.TILE
ONE_TILE_BATCHES = (1, 5, 33, 64)
MULTI_TILE_BATCHES = wc.MULTI_TILE_BATCHES      # 65, 96, 128, 130, 2048
BAR = 1e-5                # the project's bar, relative to the batch's largest |q|, |q'| (tests/test_hip_learn_perd3qn.py)
_ref = {}

# the wide draw's statistics: 2048 draws x 3 steps over 48 rows, priorities cycling through {0, 0.25, 1, 4} (the existing 6,400-draw
# test's case at this draw count); checked on the host model (pc.host_draw) in the CPU tests before the GPU test relies on it
DRAW_SEED, DRAW_ROWS, DRAW_BATCH, DRAW_STEPS = 11, 48, 2048, 3
DRAW_SD = 5               # binomial standard deviations, as the 6,400-draw test


def draw_priorities():
    return np.tile(np.array([0.0, 0.25, 1.0, 4.0]), DRAW_ROWS // 4)


def draw_bound(n):
    """(expected count per row, its binomial standard deviation) of n draws with probability p^0.6 / sum."""
    w = draw_priorities() ** 0.6
    prob = w / w.sum()
    return n * prob, np.sqrt(n * prob * (1 - prob))


def case(batch):
    """One wide minibatch from the fixture's parameters on wc.slots_of(batch): (slots [batch], float64 |q' - q| [batch], q, q')
    with the advantage means of the WHOLE batch."""
    if batch not in _ref:
        g = dc.golden()
        slots = wc.slots_of(batch)[0]
        out = (slots,) + pc.priorities(g["init"], g["target_init"], g, slots)
        for a in out:
            a.setflags(write=False)
        _ref[batch] = out
    return _ref[batch]


def per_tile_priorities(flat, target_flat, ring, slots):
    """The priorities 64-row tiles would write if each took the advantage mean over its OWN rows: pc.priorities tile by tile."""
    slots = np.asarray(slots)
    return np.concatenate([pc.priorities(flat, target_flat, ring, slots[t:t + TILE])[0] for t in range(0, len(slots), TILE)])


def duplicate_across_tiles(batch=130, slot=17, at=(3, 70, 129)):
    """wc.slots_of(batch) with `slot` at the positions `at` (tiles 0, 1 and 2 at batch 130) and nowhere else."""
    s = wc.slots_of(batch)[0].copy()
    s[s == slot] = (slot + 1) % wc.RING_ROWS
    s[list(at)] = slot
    return s


def second_tile_repeats_the_first():
    """Batch 128 whose rows 64 .. 127 are rows 0 .. 63 again."""
    s = wc.slots_of(64, seed=128)[0]
    return np.concatenate([s, s]).astype(np.int32)


def mirrored_tile():
    """Batch 64 whose rows j and 63 - j hold the same slot."""
    s = wc.slots_of(32, seed=64)[0]
    return np.concatenate([s, s[::-1]]).astype(np.int32)
