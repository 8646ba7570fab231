"""GPU: training on several ranks -- rl_policy_pack_device against the host packer for all five kinds, rl_learn_merge against the float64
reference of tests/learn_merge_cases.py at 1, 2, 3 and 8 ranks (a mixed-kind call and a 16-learner call, every step pattern), the
export / merge round trip of a learner that has made real updates, trainer(learn_ranks="average") in one process against the same run
without the keyword, and two ranks that share the one GPU over gloo.  Every comparison is bit for bit."""
import ctypes as C
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import learn_merge_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
BUFFERS = ("params", "adam_m", "adam_v", "target", "packed", "state")


@pytest.fixture(scope="module")
def worlds():
    from reinlife_amd.worlds import DeviceWorlds
    return DeviceWorlds(n_worlds=1, seed=11, device=DEV)


def _bits(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind", mc.KINDS)
def test_the_device_packer_is_the_host_packer_bit_for_bit(worlds, kind):
    """Edge rows (all zero, a power-of-two maximum, magnitudes near 1e-30 and 1e30), plain random parameters and the trained state of the
    kind's fixture; both destinations pre-filled with a sentinel, so floats neither packer writes are compared too."""
    import torch
    from reinlife_amd import _lib
    n_packed = _lib.lib().rl_policy_packed_floats(kind)
    cases = [("edge", mc.edge_params(kind, 7 + kind)), ("random", np.random.RandomState(kind).uniform(-0.08, 0.08, mc.N_PARAMS[kind]).astype(np.float32)),
             ("trained", mc.trained_params(kind)), ("zero", np.zeros(mc.N_PARAMS[kind], np.float32))]
    for name, flat in cases:
        host = mc.host_pack(kind, flat)
        packed = torch.as_tensor(np.full(n_packed, mc.SENTINEL, np.uint32).view(np.float32), device=DEV)
        worlds.pack_device(kind, torch.as_tensor(flat, device=DEV), packed)
        got = np.frombuffer(_bits(packed), np.uint32)
        bad = np.nonzero(got != host.view(np.uint32))[0]
        print("kind %d %s: %d of %d packed words differ; %d sentinel words left on the host, %d on the device"
              % (kind, name, bad.size, n_packed, (host.view(np.uint32) == mc.SENTINEL).sum(), (got == mc.SENTINEL).sum()))
        assert bad.size == 0, (name, bad[:8])
    worlds.check_error_flag()


class _Learner:
    """The six device buffers of a learner and nothing else (what rl_learn_export / rl_learn_merge read of rl_learner)."""

    def __init__(self, kind, seed, sync_target):
        import torch
        from reinlife_amd import _lib
        rng = np.random.RandomState(seed)
        n = mc.N_PARAMS[kind]
        t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
        self.kind, self.n_params, self.merge_floats, self.sync_target = kind, n, mc.merge_floats(kind), sync_target
        self.params, self.adam_m, self.adam_v = (t(rng.uniform(-9, 9, n).astype(np.float32)) for _ in range(3))   # garbage: all overwritten
        self.old_target = rng.uniform(-1, 1, n).astype(np.float32)
        self.target = None if kind == _lib.PPO else t(self.old_target)
        self.state = t(np.array([-1, 11 + seed], np.int64))
        self.packed = t(np.full(_lib.lib().rl_policy_packed_floats(kind), mc.SENTINEL, np.uint32).view(np.float32))

    def struct(self, sync_target=None):
        from reinlife_amd import _lib
        p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
        return _lib.Learner(self.kind, p(self.params), p(self.target), p(self.adam_m), p(self.adam_v), p(self.state), p(self.packed),
                            1e-3, 0.99, 0.9, 0.999, 1e-8, 32, 0, int(self.sync_target if sync_target is None else sync_target), None, None)


CALLS = {"mixed": (mc.DQN, mc.D3QN, mc.PPO, mc.PERDQN), "sixteen": (mc.DQN, mc.PERDQN) * 8}


@pytest.mark.parametrize("n_ranks", [1, 2, 3, 8])
@pytest.mark.parametrize("call", sorted(CALLS))
def test_merge_is_the_float64_mean_of_the_participants_in_rank_order(worlds, call, n_ranks):
    import torch
    kinds = CALLS[call]
    learners = [_Learner(k, 100 + i, sync_target=(i % 2 == 0)) for i, k in enumerate(kinds)]
    for p, first in enumerate(mc.PATTERNS):
        # learner i holds pattern (p + i) mod 5 with its own odd rank out: every call mixes masks; the rows are longer than the segments
        patterns = [mc.PATTERNS[(p + i) % len(mc.PATTERNS)] for i in range(len(kinds))]
        rows = mc.make_rows(kinds, n_ranks, patterns, seed=31 * p + n_ranks, pad=3)
        want = mc.merge_reference(rows, kinds)
        dev_rows = torch.as_tensor(rows, device=DEV)
        old_targets = [None if l.target is None else l.target.cpu().numpy().copy() for l in learners]
        worlds.merge_learners(learners, dev_rows, n_ranks)
        first_bits = []
        for i, (l, (wp, wm, wv, mx, part)) in enumerate(zip(learners, want)):
            where = "%s, %d ranks, %s, learner %d (kind %d, participants %s)" % (call, n_ranks, first, i, l.kind, part)
            assert _bits(l.params) == wp.tobytes(), where
            assert _bits(l.adam_m) == wm.tobytes() and _bits(l.adam_v) == wv.tobytes(), where
            assert l.state.cpu().tolist() == [mx, 11 + 100 + i], where                              # the maximum; state[1] untouched
            if l.target is None:
                assert l.kind == mc.PPO                                                          # a NULL target is accepted for PPO
            else:
                assert _bits(l.target) == (wp if l.sync_target else old_targets[i]).tobytes(), where
            assert _bits(l.packed) == mc.host_pack(l.kind, wp).tobytes(), where
            first_bits.append([_bits(getattr(l, b)) for b in BUFFERS if getattr(l, b) is not None])
        assert _bits(dev_rows) == rows.tobytes()                                                 # the table is only read
        worlds.merge_learners(learners, dev_rows, n_ranks)                                       # a second identical call: identical bits
        for l, fb in zip(learners, first_bits):
            assert [_bits(getattr(l, b)) for b in BUFFERS if getattr(l, b) is not None] == fb
    worlds.check_error_flag()


def test_this_calls_sync_flags_can_replace_the_learners_own(worlds):
    import torch
    kinds = (mc.DQN, mc.PERDQN)
    learners = [_Learner(k, 50 + i, sync_target=True) for i, k in enumerate(kinds)]
    rows = mc.make_rows(kinds, 2, ("all_equal", "one_ahead"), seed=3)
    want = mc.merge_reference(rows, kinds)
    worlds.merge_learners(learners, torch.as_tensor(rows, device=DEV), 2, sync_target=[False, True])
    assert _bits(learners[0].target) == learners[0].old_target.tobytes() and _bits(learners[1].target) == want[1][0].tobytes()
    with pytest.raises(ValueError, match="multiple of n_ranks"):
        worlds.merge_learners(learners, torch.zeros(7, device=DEV), 2)


def _trained_dqn(worlds):
    """A DQN learner that has made real updates through rl_learn on a small synthetic ring (as smoke() makes one)."""
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    rng = np.random.RandomState(0)
    torch.manual_seed(3)
    n = 64
    x = lambda: torch.as_tensor((rng.random_sample((n, 153)) < 0.15).astype(np.float32), device=DEV)  # noqa: E731
    ring = {"state": x(), "state_prime": x(), "action": torch.as_tensor(rng.randint(0, 8, size=n).astype(np.int8), device=DEV),
            "reward": torch.as_tensor(rng.choice([0.0, 0.3, -1.0, 5.0], size=n).astype(np.float32), device=DEV),
            "done": torch.as_tensor((rng.random_sample(n) < 0.2).astype(np.uint8), device=DEV), "prob": None,
            "age": torch.zeros(n, dtype=torch.int32, device=DEV), "count": torch.full((1,), n, dtype=torch.int64, device=DEV)}
    l = DeviceLearner(Models.DQN(), DEV, ring=ring)
    l.min_size = 0
    worlds.learn([l], 3)
    worlds.learn([l], 2)
    return l


def test_export_then_merge_with_one_rank_leaves_a_trained_learner_bit_identical(worlds):
    l = _trained_dqn(worlds)
    assert l.state.cpu().tolist() == [5, 2] and l.merge_floats == mc.merge_floats(mc.DQN)
    before = {b: _bits(getattr(l, b)) for b in BUFFERS}
    assert np.frombuffer(before["adam_v"], np.float32).max() > 0
    row = worlds.export_learners([l])
    n = l.n_params
    got = np.frombuffer(_bits(row), np.float32)
    assert got.size == 3 * n + 2
    assert got[:n].tobytes() == before["params"] and got[n:2 * n].tobytes() == before["adam_m"] and got[2 * n:3 * n].tobytes() == before["adam_v"]
    assert got[3 * n:].view(np.uint32).tolist() == [5, 0]                                         # the step count: low word, high word
    launches = worlds.launches
    worlds.merge_learners([l], row, 1)
    assert worlds.launches == launches + 2                                                       # mean, pack
    assert {b: _bits(getattr(l, b)) for b in BUFFERS} == before
    # ... and a second learner behind it lands where the first one's segment ends
    both = worlds.export_learners([l, l])
    got2 = np.frombuffer(_bits(both), np.float32)
    assert got2[:3 * n + 2].tobytes() == got.tobytes() and got2[3 * n + 2:].tobytes() == got.tobytes()
    worlds.check_error_flag()


def _train(**kw):
    import torch
    from reinlife_amd import Models, trainer
    torch.manual_seed(123)
    brains = [Models.DQN(max_epi=40), Models.D3QN(exploration=10, soft_update_freq=40)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        env = trainer(brains, n_episodes=40, n_worlds=4, synthetic_agents=100, refill_below=70, update_interval=20, learn="device",
                      learn_kinds=("DQN", "D3QN"), save=False, print_results=False, **kw)
    return env, brains


def test_one_process_without_a_process_group_trains_to_the_same_bits_as_without_the_keyword():
    """Learning calls behind episodes 20 and 40, both of which train both learners (the DQN's ring holds more than 1000 rows by episode 20,
    the D3QN is past its exploration of 10; no ring wraps).  With learn_ranks="average" every call ends with export + merge at n_ranks = 1
    -- the identity -- so every buffer ends as it does without the keyword, and `launches` differs by three per learning call."""
    import torch
    env, brains = _train(learn_ranks="average")
    ref, ref_brains = _train()
    torch.cuda.synchronize()
    assert env.learn_ranks == "average" and ref.learn_ranks is None and env.learn_now_calls == ref.learn_now_calls == 2
    for k in (0, 1):
        l, r = env.learners[k], ref.learners[k]
        print("learner %d (%s): state %s, ring count %d of %d" % (k, l.entry, l.state.cpu().tolist(), int(l.ring["count"].item()), l.ring["state"].shape[0]))
        assert int(l.ring["count"].item()) < l.ring["state"].shape[0]
        for b in BUFFERS:
            assert _bits(getattr(l, b)) == _bits(getattr(r, b)), (k, b)
        assert brains[k].state_dict_flat().tobytes() == ref_brains[k].state_dict_flat().tobytes()
    assert env.learners[0].state.cpu().tolist() == [10, 2] and env.learners[1].state.cpu().tolist() == [2, 2]
    assert env.worlds.launches == ref.worlds.launches + 3 * env.learn_now_calls
    assert env.tracker.results == ref.tracker.results
    assert "learn_ranks='average'" in env._weights_note() and "learn_ranks" not in ref._weights_note()


def test_two_ranks_on_one_gpu_end_with_the_same_learners(tmp_path):
    """Two fresh child processes, both on cuda:0, gloo (tests/learn_merge_rank.py): the same small trainer() on each rank over its own two
    worlds, torch seeded differently per rank.  A gloo dry run on one GPU: it shows structure -- the ranks start from rank 0's weights,
    end with the same bits, and talk once per learning episode -- not RCCL speed."""
    port = str(33500 + os.getpid() % 2000)
    outs = [str(tmp_path / ("rank%d.npz" % r)) for r in range(2)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "learn_merge_rank.py"), str(r), "2", port, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(2)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=240)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert [p.returncode for p in procs] == [0, 0], "\n".join(l[-3000:] for l in logs)
    r0, r1 = (dict(np.load(o)) for o in outs)
    assert not np.array_equal(r0["init0"], r1["init0"]) and not np.array_equal(r0["init1"], r1["init1"])   # the ranks' own initial weights differ
    for k in (0, 1):
        for b in BUFFERS:
            assert r0["%s%d" % (b, k)].tobytes() == r1["%s%d" % (b, k)].tobytes(), (k, b)
        p = r0["params%d" % k]
        assert np.isfinite(p).all() and not np.array_equal(p, r0["init%d" % k])
        assert r0["module%d" % k].tobytes() == p.tobytes() == r1["module%d" % k].tobytes()       # what Saver would write, on both ranks
        assert r0["packed%d" % k].tobytes() == mc.host_pack(k, p).tobytes()                      # (brain k is of kind k here: DQN 0, D3QN 1)
    print("states: DQN %s, D3QN %s; learn collectives %d for %d learn_now calls; tracker collectives %d (plain run %d)"
          % (r0["state0"].tolist(), r0["state1"].tolist(), r0["learn_collectives"], r0["learn_now_calls"], r0["tracker_collectives"], r0["tracker_collectives_plain"]))
    assert r0["state0"].tolist() == [10, 2] and r0["state1"].tolist() == [2, 2]
    for r in (r0, r1):
        assert r["learn_now_calls"] == 2
        assert r["learn_collectives"] == r["learn_now_calls"] + 2                                 # + the set-up's signature gather and broadcast
        assert r["learn_collectives_end"] == r["learn_collectives"]                               # a run without learning adds none
        assert r["tracker_collectives"] == r["tracker_collectives_plain"] == 2                    # one per closed interval, as without learning
        assert "2 rank(s)" in str(r["note"])


def test_nccl_at_world_size_one_runs_the_set_up_and_one_merge_on_the_device():
    """The collectives as a real multi-GPU job issues them -- a process group made with init_process_group("nccl"), which serves device
    tensors only -- at world size 1, as tests/test_hip_round4.py covers the Tracker's: the signature gather and the broadcast at
    construction, one all-gather for the one learn_now, everything on the device; the learners end on the bits of the same run without a
    process group and without the keyword."""
    import json
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    code = r'''
import hashlib, json, sys, warnings
sys.path.insert(0, %r)
import torch
import torch.distributed as dist
from reinlife_amd import Models, distributed as rd, trainer
use_dist = sys.argv[1] == "dist"
if use_dist:
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
torch.manual_seed(3)
brains = [Models.DQN(max_epi=20), Models.D3QN(exploration=10, soft_update_freq=20)]
kw = dict(learn_ranks="average") if use_dist else {}
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    env = trainer(brains, n_episodes=20, update_interval=20, n_worlds=4, save=False, print_results=False, seed=77, synthetic_agents=100,
                  refill_below=70, learn="device", learn_kinds=("DQN", "D3QN"), **kw)
torch.cuda.synchronize()
sha = {k: {b: hashlib.sha256(getattr(l, b).cpu().numpy().tobytes()).hexdigest() for b in ("params", "adam_m", "adam_v", "target", "packed", "state")}
       for k, l in env.learners.items()}
print(json.dumps({"sha": sha, "states": [env.learners[k].state.cpu().tolist() for k in (0, 1)], "learn_collectives": rd.learn_collectives_executed,
                  "learn_now_calls": env.learn_now_calls, "tracker": env.tracker.collectives_executed, "has_dist": env.dist is not None,
                  "backend": rd.backend_of(dist) if use_dist else ""}))
if use_dist:
    dist.barrier(); dist.destroy_process_group()
''' % ROOT
    outs = {}
    for mode in ("plain", "dist"):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        out = subprocess.run([sys.executable, "-c", code, mode], env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        outs[mode] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    p, d = outs["plain"], outs["dist"]
    print("nccl, one rank: states %s, learn collectives %d, tracker collectives %d" % (d["states"], d["learn_collectives"], d["tracker"]))
    assert d["has_dist"] and d["backend"] == "nccl" and not p["has_dist"]
    assert d["learn_now_calls"] == p["learn_now_calls"] == 1 and d["states"] == p["states"] == [[5, 1], [1, 1]]
    assert d["learn_collectives"] == 3 and p["learn_collectives"] == 0                # signature gather + broadcast + one all-gather
    assert d["tracker"] == 1 and p["tracker"] == 0
    assert d["sha"] == p["sha"]
