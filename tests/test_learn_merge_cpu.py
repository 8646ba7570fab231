"""CPU: the host side of training on several ranks -- rl_learn_merge_floats / rl_learn_export / rl_learn_merge / rl_policy_pack_device are
exported and refuse bad arguments by name before a device is touched, trainer(learn_ranks=...) states its conditions before it touches
one, the float64 reference of the merge (tests/learn_merge_cases.py) does what the contract says on hand-made rows, and the three
collectives of reinlife_amd/distributed.py (one all-gather of the learner rows, one broadcast, one signature gather) work between two
gloo processes on CPU tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from reinlife_amd import Models, _lib, trainer

import learn_merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_exported_and_the_segment_is_three_arrays_and_two_words():
    lib = _lib.lib()
    for name in ("rl_learn_merge_floats", "rl_learn_export", "rl_learn_merge", "rl_policy_pack_device"):
        assert hasattr(lib, name), name
    for kind in mc.KINDS:
        assert lib.rl_learn_merge_floats(kind) == 3 * lib.rl_policy_n_params(kind) + 2 == mc.merge_floats(kind)
    assert (3 * lib.rl_policy_n_params(_lib.D3QN)) % 2 == 1            # why the step count travels as two 32-bit words
    for kind in (-1, 5, 9):
        assert lib.rl_learn_merge_floats(kind) == -1
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    for decl in ("int64_t rl_learn_merge_floats(int kind);", "int rl_learn_export(", "int rl_learn_merge(", "int rl_policy_pack_device("):
        assert decl in hdr, decl
    assert _lib.MAX_MERGE_RANKS == 64


def _handle():
    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.rl_create(C.byref(_lib.Config(30, 30, 100, 2, 256, 1, 1, 0, 1, 0, 0)), C.byref(h)) == 0
    return h


P = C.c_void_p(0x1000)   # a dummy non-null address: validation happens before anything is launched or dereferenced


def _learners(kinds=(_lib.DQN,), **over):
    n = len(kinds)
    ls = (_lib.Learner * n)(*[_lib.Learner(k, P, None if k == _lib.PPO else P, P, P, P, P, 0.001, 0.99, 0.9, 0.999, 1e-8, 32, 0, 1, None, None)
                              for k in kinds])
    for k, v in over.items():
        setattr(ls[n - 1], k, v)
    return ls


def _merge(h, ls, rows=P, n_ranks=2, stride=None):
    lib = _lib.lib()
    if stride is None:
        stride = sum(max(lib.rl_learn_merge_floats(l.kind), 0) for l in ls)
    rc = lib.rl_learn_merge(h, ls, len(ls), rows, n_ranks, stride, None)
    return rc, lib.rl_last_error()


def _export(h, ls, row=P):
    lib = _lib.lib()
    rc = lib.rl_learn_export(h, ls, len(ls), row, None)
    return rc, lib.rl_last_error()


def test_merge_refuses_bad_arguments_by_name_before_touching_a_device():
    lib, h = _lib.lib(), _handle()
    mixed = (_lib.DQN, _lib.D3QN, _lib.PPO, _lib.PERDQN)
    rc, err = _merge(None, _learners())
    assert rc == -1 and err == b"rl_learn_merge: null handle"
    rc = lib.rl_learn_merge(h, None, 1, P, 2, 10 ** 6, None)
    assert rc == -1 and b"null learners" in lib.rl_last_error()
    rc, err = _merge(h, _learners(mixed), rows=None)
    assert rc == -1 and err.startswith(b"rl_learn_merge:") and b"null rows" in err and b"learners 0..3" in err
    for n_ranks in (0, 65, -1):
        rc, err = _merge(h, _learners(mixed), n_ranks=n_ranks)
        assert rc == -1 and b"n_ranks must be in [1,64]" in err and ("got %d" % n_ranks).encode() in err, n_ranks
    total = sum(mc.merge_floats(k) for k in mixed)
    rc, err = _merge(h, _learners(mixed), stride=total - 1)
    assert rc == -1 and b"row_stride_floats" in err and b"shorter" in err and b"learner 3" in err and str(total).encode() in err
    for field in ("params", "adam_m", "adam_v", "state", "packed", "target"):
        rc, err = _merge(h, _learners((_lib.PPO, _lib.D3QN), **{field: None}))
        assert rc == -1 and b"learner 1" in err and b"null" in err and field.encode() in err, field
    for kind in (-1, 5, 7):
        rc, err = _merge(h, _learners((_lib.DQN, kind)))
        assert rc == -4 and ("kind %d" % kind).encode() in err and b"learner 1" in err, kind      # RL_E_UNSUPPORTED
    for n in (0, 17):
        ls = _learners((_lib.DQN,) * max(n, 1))
        rc = lib.rl_learn_merge(h, ls, n, P, 2, 10 ** 7, None)
        assert rc == -1 and b"n_learners must be in [1,16]" in lib.rl_last_error() and ("got %d" % n).encode() in lib.rl_last_error()
    lib.rl_destroy(h)


def test_export_and_pack_device_refuse_bad_arguments_by_name_before_touching_a_device():
    lib, h = _lib.lib(), _handle()
    rc, err = _export(None, _learners())
    assert rc == -1 and err == b"rl_learn_export: null handle"
    rc, err = _export(h, _learners((_lib.DQN, _lib.PPO)), row=None)
    assert rc == -1 and b"null row" in err and b"learners 0..1" in err
    for field in ("params", "adam_m", "adam_v", "state"):
        rc, err = _export(h, _learners((_lib.DQN, _lib.PERD3QN), **{field: None}))
        assert rc == -1 and err.startswith(b"rl_learn_export:") and b"learner 1" in err and field.encode() in err, field
    rc, err = _export(h, _learners((_lib.DQN, 6)))
    assert rc == -4 and b"kind 6" in err and b"learner 1" in err
    ls = _learners((_lib.DQN,) * 17)
    assert lib.rl_learn_export(h, ls, 17, P, None) == -1 and b"n_learners" in lib.rl_last_error() and b"16" in lib.rl_last_error()
    lib.rl_destroy(h)
    for kind in (-1, 5):
        assert lib.rl_policy_pack_device(kind, P, P, None) == -1 and ("kind %d" % kind).encode() in lib.rl_last_error()
    for args in ((None, P), (P, None)):
        assert lib.rl_policy_pack_device(_lib.PERDQN, *args, None) == -1
        assert b"rl_policy_pack_device: kind 4" in lib.rl_last_error() and b"null" in lib.rl_last_error()


@pytest.mark.parametrize("kwargs, says", [
    (dict(learn="device", learn_ranks="bogus"), "learn_ranks must be"),
    (dict(learn="device", learn_ranks=True), "learn_ranks must be"),
    (dict(learn_ranks="average"), "learn_ranks='average' needs learn='device'"),
])
def test_learn_ranks_states_its_conditions_before_touching_a_gpu(kwargs, says, monkeypatch):
    from reinlife_amd import worlds
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match=says):
        trainer([Models.DQN(max_epi=60), Models.D3QN()], n_episodes=5, n_worlds=4, save=False, print_results=False, **kwargs)


def test_a_second_rank_without_the_keyword_is_still_refused_and_the_message_names_it(monkeypatch):
    from reinlife_amd import worlds

    class TwoRanks:
        def is_initialized(self): return True          # noqa: E704
        def get_rank(self): return 0                   # noqa: E704
        def get_world_size(self): return 2             # noqa: E704
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="single rank") as e:
        trainer([Models.DQN(max_epi=60)], n_episodes=5, n_worlds=4, save=False, print_results=False, learn="device", dist=TwoRanks())
    assert 'learn_ranks="average"' in str(e.value)


def test_more_than_64_ranks_are_refused_before_a_device_or_a_collective(monkeypatch):
    from reinlife_amd import worlds

    class ManyRanks:
        def is_initialized(self): return True          # noqa: E704
        def get_rank(self): return 0                   # noqa: E704
        def get_world_size(self): return 65            # noqa: E704
        def all_gather_into_tensor(self, *a): pytest.fail("a collective was issued")   # noqa: E704
    monkeypatch.setattr(worlds.DeviceWorlds, "__init__", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="at most 64 ranks"):
        trainer([Models.DQN(max_epi=60)], n_episodes=5, n_worlds=4, save=False, print_results=False, learn="device", learn_ranks="average", dist=ManyRanks())


def test_the_reference_merge_on_hand_made_rows():
    """A self-check of the tests' own reference (tests/learn_merge_cases.py), not of the library: it holds on any commit.  The GPU tests
    compare rl_learn_merge against this reference, so it has to do what the contract says.
    Three ranks, one DQN learner: steps (7, 9, 9) -> ranks 1 and 2 take part; the mean of 1 and 2 is 1.5, of 1e-30 and 3e-30 2e-30, rank
    0's values do not count; equal counts -> all three; one participant -> its own bits, a -0.0 included."""
    kinds = (mc.DQN,)
    n = mc.N_PARAMS[mc.DQN]
    rows = np.zeros((3, mc.merge_floats(mc.DQN)), np.float32)
    rows[0, :n], rows[1, :n], rows[2, :n] = 100.0, 1.0, 2.0
    rows[0, n:2 * n], rows[1, n:2 * n], rows[2, n:2 * n] = -5.0, 1e-30, 3e-30
    for r, s in enumerate((7, 9, 9)):
        rows[r, 3 * n:] = np.array([s, 0], np.uint32).view(np.float32)
    (p, m, v, mx, part), = mc.merge_reference(rows, kinds)
    assert part == [1, 2] and mx == 9 and (p == 1.5).all() and (m == np.float32(np.float64(np.float32(1e-30)) / 2 + np.float64(np.float32(3e-30)) / 2)).all() and (v == 0).all()
    rows[0, 3 * n] = np.array([9], np.uint32).view(np.float32)[0]
    (p, m, v, mx, part), = mc.merge_reference(rows, kinds)
    assert part == [0, 1, 2] and (p == np.float32(103.0 / 3.0)).all()
    rows[2, 3 * n + 1] = np.array([1], np.uint32).view(np.float32)[0]                  # the high word: 2^32 + 9
    rows[2, :4] = -0.0
    (p, m, v, mx, part), = mc.merge_reference(rows, kinds)
    assert part == [2] and mx == (1 << 32) + 9 and p.tobytes() == rows[2, :n].tobytes() and np.signbit(p[:4]).all()
    assert mc.row_steps(rows, 0, n) == [9, 9, (1 << 32) + 9]
    # ... and the synthetic tables hold what they say
    for pat in mc.PATTERNS:
        t = mc.make_rows((mc.PERDQN, mc.DQN), 3, (pat, pat), seed=1, pad=5)
        segs, total = mc.segments((mc.PERDQN, mc.DQN))
        assert t.shape == (3, total + 5) and [mc.row_steps(t, o, k) for o, k in segs] == [mc.steps_of(pat, 3, 1), mc.steps_of(pat, 3, 2)]
    assert mc.steps_of("high_word", 3, 1) == [3, (1 << 32) + 3, 3] and mc.steps_of("one_behind", 1, 1) == [5]


def _worker(rank, world_size, port, q):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from reinlife_amd import distributed as rd
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    out = {"rank": rank}
    row = torch.arange(7, dtype=torch.float32) + 100 * rank
    row[3] = torch.tensor([0x7fc00001 + rank], dtype=torch.int32).view(torch.float32)[0]   # bits travel as they are (a NaN's payload)
    table = rd.gather_learner_rows(row, dist)
    out["table"], out["after_gather"] = table.numpy().view(np.uint32).copy(), rd.learn_collectives_executed
    t = torch.full((5,), float(rank + 1))
    same = rd.broadcast_from_rank0(t, dist)
    out["broadcast"], out["in_place"], out["after_broadcast"] = t.tolist(), same is t, rd.learn_collectives_executed
    out["sig_ok"] = rd.check_learner_signature([2, 0, 0, 0, 1, 1, 1, 20, 5, 1, 1, 1], dist).shape
    try:
        rd.check_learner_signature([2, 0, 0, 0, 1, 1, 1, 20 + 10 * rank, 5, 1, 1, 1], dist)
        out["sig_bad"] = None
    except ValueError as e:
        out["sig_bad"] = str(e)
    try:   # learners of different counts: rows of one length all the same, so nobody hangs
        rd.check_learner_signature([1, 0, 0, 0, 20, 5, 1, 1, 1] if rank else [2, 0, 0, 0, 1, 1, 1, 20, 5, 1, 1, 1], dist)
        out["sig_len"] = None
    except ValueError as e:
        out["sig_len"] = str(e)
    out["learn_collectives"], out["collectives"] = rd.learn_collectives_executed, rd.collectives_executed
    q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_gather_broadcast_and_refuse_a_signature_mismatch_together():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=180) for _ in procs], key=lambda o: o["rank"])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = np.stack([(np.arange(7, dtype=np.float32) + 100 * r) for r in range(2)]).view(np.uint32).copy()
    want[0, 3], want[1, 3] = 0x7fc00001, 0x7fc00002
    for o in res:
        assert o["table"].shape == (2, 7) and np.array_equal(o["table"], want)            # the same [2, n] table on both ranks
        assert o["after_gather"] == 1                                                    # one collective counted
        assert o["broadcast"] == [1.0] * 5 and o["in_place"] and o["after_broadcast"] == 2   # rank 0's values
        assert tuple(o["sig_ok"]) == (2, 129)
        assert o["sig_bad"] is not None and "same learners on the same schedule" in o["sig_bad"] and "20" in o["sig_bad"] and "30" in o["sig_bad"]
        assert o["sig_len"] is not None and "same learners" in o["sig_len"]
        assert o["learn_collectives"] == 5 and o["collectives"] == 0                     # counted apart from the Tracker's / bench's collectives
    assert res[0]["sig_bad"] == res[1]["sig_bad"] and res[0]["sig_len"] == res[1]["sig_len"]    # the same error on every rank
