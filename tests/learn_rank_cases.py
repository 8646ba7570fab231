"""Shared by tests/test_learn_draw_rank_cpu.py and tests/test_hip_learn_draw_rank.py: rl_learn_draw_rank's draw restated on the host, all
in integers -- the content keys are learn_perd3qn_cases.content_keys, the order numpy's lexsort by (key, slot), and draw d the row at rank
((uint64)x_d * size) >> 32, x_d = word 0 of rl_philox(seed, 0, brain, calls, RL_SITE_LEARN, d)."""
import ctypes as C

import numpy as np

RANK_LAUNCHES = 6   # RL_LEARN_DRAW_RANK_LAUNCHES
TABLE_BYTES = 2 * 65536 * 4   # the two counter tables of a work buffer


def work_bytes(capacity):
    """rl_learn_draw_rank_work_bytes: two tables of 65,536 uint32 counters and one int32 per ring row, rounded up to 16 bytes."""
    return TABLE_BYTES + (4 * int(capacity) + 15) // 16 * 16


def host_order(keys):
    """The slots 0 .. len(keys) - 1 ascending by (key, slot) -> int32."""
    keys = np.asarray(keys, np.uint64)
    return np.lexsort((np.arange(len(keys)), keys)).astype(np.int32)


def philox_words(seed, brain, calls, n_draws):
    """Word 0 of rl_philox(seed, 0, brain, (uint32)calls, RL_SITE_LEARN, d), d = 0 .. n_draws - 1 -> uint64 [n_draws]."""
    from reinlife_amd import _lib
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    x = np.zeros(n_draws, np.uint64)
    for d in range(n_draws):
        lib.rl_philox(seed, 0, brain, calls & 0xffffffff, _lib.SITE_LEARN, d, C.byref(out))
        x[d] = int(out[0])
    return x


def host_rank_draw(keys, seed, brain, calls, n_draws):
    """The slots rl_learn_draw_rank writes for one learner -> int32 [n_draws]; an empty ring: slot 0 for every draw."""
    size = len(keys)
    if size == 0:
        return np.zeros(n_draws, np.int32)
    t = (philox_words(seed, brain, calls, n_draws) * np.uint64(size)) >> np.uint64(32)   # (x < 2^32 and size < 2^31: no overflow)
    return host_order(keys)[t.astype(np.int64)]
