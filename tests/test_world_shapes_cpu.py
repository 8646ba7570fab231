"""CPU: the premises of tests/test_hip_world_shapes.py.  The inputs that file steps the world kernels with -- the shapes of
tests/world_shape_cases.py under seeded random actions -- do reach what the shapes are in the table for (both seams crossed, coordinate 254
stood on, births, vanishes and refills), shown on the oracle alone; and the host side of the library answers for every row what the table
says: rl_create accepts it, rl_run_supported claims (or refuses) it, and the plane stride restated in Python is the table's."""
import ctypes as C

import pytest

import world_shape_cases as wc
from reinlife_amd import _lib


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
@pytest.mark.parametrize("static", [True, False], ids=["static", "nonstatic"])
@pytest.mark.parametrize("setting", sorted(wc.SETTINGS))
def test_the_seeded_inputs_reach_the_seams_and_the_edges(case, static, setting):
    """Conditions on the inputs, not measurements: a seed that misses one is replaced, the floors stay.  Asserted once per input setting of
    the GPU file -- "fused": a refill at the row's threshold behind every tick (test_fused_tick_with_refill_matches_the_oracle), "split": one
    every 10 ticks (test_reset_split_step_and_update_match_the_oracle) -- with the constructor arguments those tests read from
    wc.SETTINGS, wc.world_seed and wc.config: 40 ticks of RandomState(100 * W + H) actions on 6 worlds (4 on the 250-agent rows, as on the
    GPU: fewer worlds make the floors harder to reach, not easier), with static and with non-static families (the GPU file runs the one
    wc.is_static names)."""
    st = wc.run_oracle(case, static=static, **wc.SETTINGS[setting])
    assert st["rows"] >= 5 and st["cols"] >= 5, "fewer than 5 crossings of a seam: %r" % st
    assert st["max_i"] == case.height - 1 and st["max_j"] == case.width - 1, "no agent stood on the last row / column: %r" % st
    if case.height == 255:
        assert st["max_i"] == 254
    if case.width == 255:
        assert st["max_j"] == 254
    assert st["births"] >= 1 and st["vanished"] >= 1 and st["refills"] >= 1, st


def test_seam_crossings_counts_wraps_only():
    before = [{1: (0, 0), 2: (2, 254), 3: (1, 7), 4: (0, 100)}, {1: (0, 0)}]
    after = [{1: (2, 0), 2: (2, 0), 3: (1, 8), 5: (0, 100)}, {1: (0, 0)}]      # 1: up through the row seam, 2: right through the column seam
    assert wc.seam_crossings(before, after, 3, 255) == (1, 1)
    assert wc.seam_crossings(before, before, 3, 255) == (0, 0)


def test_the_stride_rule_restated_in_python():
    assert [wc.plane_stride(c.width, c.height) for c in wc.CASES] == wc.STRIDES == [c.stride for c in wc.CASES]
    assert wc.STRIDES == [7, 7, 7, 7, 39, 263, 7, 263, 16, 135, 71, 71]
    assert wc.plane_stride(30, 30) == 39                       # (the shape bench.py times: DESIGN.md 5.8)
    assert wc.plane_stride(16, 255) == 16 and (39 - 16) * 255 * 12 > 16 * 1024      # the one row whose padding plane_stride refuses
    for c in wc.CASES:
        assert c.stride == c.width or c.stride & 31 == 7
        assert c.slot_cap == wc.slot_cap_for(c.max_agents) == _lib.slot_cap_for(c.max_agents)
        assert 3 <= min(c.width, c.height) and max(c.width, c.height) <= 255 and c.width * c.height <= 4096


def _handle(c, n_brains=2):
    cfg = _lib.Config(c.width, c.height, c.max_agents, n_brains, c.slot_cap, wc.n_worlds(c), 1, 0, 1, 0, 7)
    h = C.c_void_p()
    rc = _lib.lib().rl_create(C.byref(cfg), C.byref(h))
    assert rc == 0, "rl_create refused %s: %s" % (wc.case_id(c), _lib.lib().rl_last_error().decode())
    return h


@pytest.mark.parametrize("case", wc.CASES, ids=wc.case_id)
def test_rl_create_accepts_the_row_and_rl_run_supported_answers_as_the_table_says(case):
    lib = _lib.lib()
    h = _handle(case)
    try:
        duel = (_lib.Brain * 2)(_lib.Brain(_lib.PERD3QN, 0.0, None), _lib.Brain(_lib.D3QN, 0.2, None))
        mixed = (_lib.Brain * 2)(_lib.Brain(_lib.PPO, 0.0, None), _lib.Brain(_lib.DQN, 0.3, None))
        assert lib.rl_run_supported(h, duel, 2) == case.run_dueling
        assert lib.rl_run_supported(h, mixed, 2) == case.run_mixed
        assert case.run_mixed == (1 if case.slot_cap <= 256 else 0)
    finally:
        lib.rl_destroy(h)
    # ... and with the three brains of tests/test_hip_world_shapes.py's mixed-kind launches (PPO, DQN, PERD3QN)
    h = _handle(case, 3)
    try:
        three = (_lib.Brain * 3)(_lib.Brain(_lib.PPO, 0.0, None), _lib.Brain(_lib.DQN, 0.3, None), _lib.Brain(_lib.PERD3QN, 0.05, None))
        assert lib.rl_run_supported(h, three, 3) == case.run_mixed
    finally:
        lib.rl_destroy(h)


def test_no_row_loses_its_padding_to_the_lds_limit():
    """host_plane_stride (rl_run.hip) drops the padding when the launch's carve-out with padded planes exceeds 160 KB.  The carve arithmetic
    restated (wc.world_lds_bytes: carve() of rl_world_dev.h; wc.run_lds_bytes: + carve_policy's tail, the mirror taking only what is left)
    stays below that on every row at its table stride -- for the dueling kernel with the 2 brains of the GPU tests and with 8, the most
    rl_run takes, and for the mixed-kind kernel with 3 brains on the rows it supports -- so the stride column is what the launches run with."""
    full = wc.CASES[-1]
    assert (full.width, full.height, full.slot_cap) == (64, 64, 512)
    assert wc.world_lds_bytes(full, 64) == 113952 and wc.world_lds_bytes(full, 71) == 113952 + 7 * 64 * 12
    assert wc.run_lds_bytes(full, 71, 2) == 138560                      # 135 KB: the fullest row keeps stride 71
    for c in wc.CASES:
        assert wc.world_lds_bytes(c, c.width) <= wc.LDS_BYTES             # (what rl_create checks)
        assert wc.run_lds_bytes(c, c.stride, 2) <= wc.run_lds_bytes(c, c.stride, 8) <= wc.LDS_BYTES, wc.case_id(c)
        if c.run_mixed:
            assert wc.run_lds_bytes(c, c.stride, 3, mixed=True) <= wc.LDS_BYTES, wc.case_id(c)
