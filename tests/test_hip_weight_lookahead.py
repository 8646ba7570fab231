"""The prologue of k_run's certified one-wave dueling tile ("the row read without the false wait") on the GPU, through the
tuning library.  The tile reads its rows behind ONE wave-uniform branch: every row of the tile mirrored in LDS -> twenty ds_read_b128 (chunk
9 of the upper half as the 16-byte unit at float 152); any row beyond the mirror -> EVERY lane reads its row from memory.  These cases walk
both arms and the seam between them: one tile per brain, two tiles per brain (the benchmark's shape), six tiles (on six of the eight waves: no wave runs two -- two
tiles per wave occur in the cases with nine and more tiles), a brain without agents, tiles with one valid row, an adversarial brain whose tiles are redone by the full
tile between hot tiles on the same wave, and worlds with more agents than the mirror has rows (30 x 30 and 64 x 64, max_agents raised), whose
tiles hold mirrored rows next to rows from memory.  Every case compares states, actions, rewards, done flags and Agent.state rows exactly
with the forced full path (run mask 64), with the two-launch loop and with the same ticks as one-tick launches, for TRAIN 0 and TRAIN 1."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# bytes of one mirrored row (kXStride floats, rl_world_dev.h) and the LDS a workgroup can have: a world with more agents than
# LDS_BYTES / ROW_BYTES has rows beyond the mirror whatever else the kernel keeps in LDS
ROW_BYTES, LDS_BYTES = 164 * 4, 160 * 1024

SCRIPT = r'''
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch, bench
from reinlife_amd import _lib
from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
lib = _lib.lib()

def counters():
    a = (ctypes.c_ulonglong * 4)()
    assert lib.rl_debug_cert_counters(a) == 0
    return [int(a[i]) for i in range(3)]

def adversarial(seed):
    # advantage head weights zero: every row's advantages are the head's biases, a_1 and a_3 one ulp apart; a value bias of 300 merges them
    # in q = (a + v) - m, so the full path picks 1 where the advantages alone say 3 (tests/test_hip_cert_argmax.py)
    w = bench.brain_weights("PERD3QN", seed).astype(np.float32).copy()
    o = 153 * 128 + 128 + 128 * 128 + 128
    w[o:o + 8 * 128] = 0.0
    w[o + 8 * 128:o + 8 * 128 + 8] = np.array([0, 1, 0, np.nextafter(np.float32(1), np.float32(2)), 0, 0, 0, 0], np.float32)
    w[-1] = 300.0
    return w

# deal: the brains are dealt round-robin at reset (else the synthetic reset draws them); adv: the adversarial brains
SHAPES = {"one-tile": dict(R=6, size=30, n_brains=2, max_agents=64, n_new=56, thr=40, adv=[], eps=[0.0, 0.1], deal=True, chunks=(1, 7, 12)),
          "two-tiles": dict(R=8, size=30, n_brains=2, max_agents=100, n_new=100, thr=70, adv=[], eps=[0.0, 0.05], deal=True, chunks=(1, 7, 12)),
          "six-tiles": dict(R=4, size=30, n_brains=6, max_agents=128, n_new=120, thr=100, adv=[], eps=[0.0] * 6, deal=True, chunks=(1, 7, 12)),
          "edges": dict(R=6, size=30, n_brains=3, max_agents=100, n_new=96, thr=70, adv=[1], eps=[0.0, 0.0, 0.05], deal=False, chunks=(1, 7, 12)),
          "adversarial": dict(R=6, size=30, n_brains=8, max_agents=128, n_new=120, thr=100, adv=[1, 4], eps=[0.0] * 8, deal=True, chunks=(1, 7, 12)),
          "beyond-mirror": dict(R=4, size=30, n_brains=8, max_agents=250, n_new=272, thr=256, adv=[3], eps=[0.0] * 8, deal=True, chunks=(1, 7, 12)),
          "big-grid": dict(R=4, size=64, n_brains=8, max_agents=250, n_new=272, thr=256, adv=[], eps=[0.0] * 7 + [0.1], deal=True, chunks=(1, 7, 12))}

def make(shape):
    sh = SHAPES[shape]
    dw = DeviceWorlds(n_worlds=sh["R"], width=sh["size"], height=sh["size"], max_agents=sh["max_agents"], n_brains=sh["n_brains"],
                      static_families=True, limit_reproduction=False, incentivize_killing=True, seed=53, world_base=3, device="cuda:0")
    assert dw.cap <= 512
    brains = []
    for k in range(sh["n_brains"]):
        w = adversarial(300 + k) if k in sh["adv"] else bench.brain_weights("PERD3QN" if k %% 2 == 0 else "D3QN", 900 + k)
        kind = _lib.PERD3QN if k in sh["adv"] or k %% 2 == 0 else _lib.D3QN
        brains.append((kind, sh["eps"][k], pack_brain_weights(kind, w, "cuda:0")))
    dw.set_brains(brains)
    dw.reset_synthetic(sh["n_new"])
    if sh["deal"] or shape == "edges":
        torch.cuda.synchronize()
        n = dw.s["n_agents"].cpu().numpy()
        br = dw.s["a_brain"].cpu().numpy().copy()
        if sh["deal"]:
            br[:, :] = np.arange(br.shape[1])[None, :] %% sh["n_brains"]
        else:
            # world 0: brain 2 has no live agent; world 1: the adversarial brain 1 keeps ONE agent (a redone tile with a single valid row);
            # world 2: brain 0 holds exactly 33 agents (its second tile has a single valid row), the others go to brain 2
            b0 = br[0, :n[0]]; b0[b0 == 2] = 0
            b1 = br[1, :n[1]]; idx = np.nonzero(b1 == 1)[0]; b1[idx[1:]] = 0
            b2 = br[2, :n[2]]; b2[:] = 2; b2[:33] = 0
        dw.s["a_brain"].copy_(torch.as_tensor(br, device="cuda:0"))
        torch.cuda.synchronize()
        _lib.check(lib.rl_bind_state(dw.handle, ctypes.byref(dw._state)), "rl_bind_state")   # (state rewritten by the host, as load_world does)
    return dw

def rows(dw):   # [world][brain] row counts of the state the next policy half reads
    n = dw.s["n_agents"].cpu().numpy()
    br = dw.s["a_brain"].cpu().numpy()
    return np.stack([np.bincount(br[w, :n[w]].astype(np.int64), minlength=dw.n_brains) for w in range(dw.R)])

def snap(dw):
    torch.cuda.synchronize()
    dw.check_error_flag()
    R = dw.R
    n = dw.s["n_agents"].cpu().numpy()
    acted = dw.n_acted.cpu().numpy()
    d = {}
    for k, v in dw.s.items():
        x = v.cpu().numpy()
        d[k] = [x[w, :n[w]].copy() for w in range(R)] if k.startswith("a_") else x.copy()
    d["obs"] = [dw.obs_state().cpu().numpy()[w, :n[w]].copy() for w in range(R)]
    d["actions"] = [dw.actions.cpu().numpy()[w, :acted[w]].copy() for w in range(R)]
    post = dw.n_post.cpu().numpy()
    for k in ("reward", "done"):
        d[k] = [getattr(dw, k).cpu().numpy()[w, :post[w]].copy() for w in range(R)]   # (the last tick's rows: the slots after Environment.step)
    for k in ("n_acted", "n_post", "acted_total", "refill_count"):
        d[k] = getattr(dw, k).cpu().numpy().copy()
    return d

def differ(a, b):
    bad = []
    for k in a:
        if isinstance(a[k], list):
            same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[k], b[k]))
        else:
            same = np.array_equal(a[k], b[k], equal_nan=True)
        if not same:
            bad.append(k)
    return bad

def case(shape, train):
    sh = SHAPES[shape]
    thr, n_new, adv = sh["thr"], sh["n_new"], sh["adv"]
    sched = lambda n: np.ascontiguousarray(np.array(sh["eps"], np.float32)[None, :].repeat(n, 0))   # noqa: E731
    res = dict(shape=shape, train=train, diff_full=[], diff_loop=[], diff_single=[], tiles_adv=0, tiles_all=0, tiles_max=0, tiles_min=99,
               agents_max=0, agents_min=1 << 30, empty_brain=0, single_row_tiles=0, ticks=0)
    def run(dw, n):
        kw = dict(eps_schedule=sched(n), trk_skip=1) if train else {}
        dw.run(n, thr, n_new, **kw)
    lib.rl_debug_set_run_mask(0)
    cert, single, loop = make(shape), make(shape), make(shape)
    lib.rl_debug_set_run_mask(64)
    full = make(shape)
    for dw in (cert, single, full):
        assert dw.run_supported()
        if train:
            dw.enable_tracking(True)
    counters()
    got, forced = [0, 0, 0], [0, 0, 0]
    for n in sh["chunks"]:
        lib.rl_debug_set_run_mask(0)
        run(cert, n)
        a = snap(cert)
        got = [x + y for x, y in zip(got, counters())]
        for i in range(n):
            c = rows(single)   # what this tick's policy half reads: its tiles are ceil(rows / 32) per brain
            t = (c + 31) // 32
            res["tiles_adv"] += int(t[:, adv].sum()); res["tiles_all"] += int(t.sum())
            res["tiles_max"] = max(res["tiles_max"], int(t.sum(1).max())); res["tiles_min"] = min(res["tiles_min"], int(t.sum(1).min()))
            res["agents_max"] = max(res["agents_max"], int(c.sum(1).max())); res["agents_min"] = min(res["agents_min"], int(c.sum(1).min()))
            res["empty_brain"] += int((c == 0).sum()); res["single_row_tiles"] += int((c %% 32 == 1).sum())
            run(single, 1)
        s1 = snap(single)
        counters()
        lib.rl_debug_set_run_mask(64)
        run(full, n)
        f = snap(full)
        forced = [x + y for x, y in zip(forced, counters())]
        lib.rl_debug_set_run_mask(0)
        for i in range(n):
            if train:
                loop._set_epsilons(sh["eps"])
            loop.act(); loop.tick_refill(thr, n_new)
        l = snap(loop)
        res["diff_full"] += ["%%d:%%s" %% (res["ticks"], k) for k in differ(a, f)]
        res["diff_loop"] += ["%%d:%%s" %% (res["ticks"], k) for k in differ(a, l)]
        res["diff_single"] += ["%%d:%%s" %% (res["ticks"], k) for k in differ(a, s1)]
        res["ticks"] += n
    res["counters"] = got; res["forced"] = forced
    res["acted"] = int(cert.acted_total.item())
    print("RESULT " + json.dumps(res), flush=True)

case(%(shape)r, %(train)d)
'''


def _run(shape, train):
    from reinlife_amd import build
    tune = build.TUNE_LIB_PATH
    if not os.path.exists(tune):
        pytest.skip("the tuning library is not built (RL_TUNE=1 python reinlife_amd/build.py; __graft_entry__.build() builds it)")
    env = dict(os.environ, REINLIFE_HIP_LIB=tune)
    env.pop("RL_TUNE", None)
    out = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, shape=shape, train=train)], env=env, capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = [json.loads(line[len("RESULT "):]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    assert len(res) == 1
    print(res[0])
    r = res[0]
    assert r["ticks"] == 20, r
    assert r["diff_full"] == [], r       # against run mask 64: the full tile
    assert r["diff_loop"] == [], r       # against rl_policy_act + rl_tick_refill
    assert r["diff_single"] == [], r     # one launch of N ticks against N launches of one tick
    assert r["forced"] == [0, 0, 0], r   # the forced full path never enters the certified finish
    assert r["counters"][1] > 0, r       # ... and the launches under test did, and certified rows
    return r


TRAIN = pytest.mark.parametrize("train", [0, 1], ids=["TRAIN0", "TRAIN1"])


@pytest.mark.gpu
@TRAIN
def test_one_tile_per_brain(train):
    """Two brains of 28 agents at reset: two tiles per world, on waves 0 and 1; every row mirrored."""
    r = _run("one-tile", train)
    assert r["tiles_min"] == 2, r
    assert r["agents_max"] * ROW_BYTES < 64 * 1024, r   # (far inside any mirror)


@pytest.mark.gpu
@TRAIN
def test_two_tiles_per_brain(train):
    """The benchmark's shape: two brains of 50 agents, four tiles, one per SIMD; every row mirrored."""
    r = _run("two-tiles", train)
    assert r["tiles_max"] >= 4, r


@pytest.mark.gpu
@TRAIN
def test_six_tiles(train):
    """Six brains of 20 agents: six tiles on six of the eight waves, two SIMDs with two streaming tiles each."""
    r = _run("six-tiles", train)
    assert 5 <= r["tiles_max"] <= 8, r


@pytest.mark.gpu
@TRAIN
def test_brain_without_agents_and_tiles_with_one_valid_row(train):
    """A world one of whose brains has no live agent, the adversarial brain with ONE agent (a redone tile with a single valid row) and a brain
    of 33 agents (a hot tile with a single valid row: 31 padding lanes read list entry 0)."""
    r = _run("edges", train)
    assert r["empty_brain"] > 0 and r["single_row_tiles"] > 0, r
    assert r["counters"][2] > 0, r   # redone tiles


@pytest.mark.gpu
@TRAIN
def test_redone_tiles_between_hot_tiles(train):
    """Eight brains, two of them adversarial (advantages one ulp apart, b_v = 300) and greedy: every tile of theirs stores nothing and is run
    again as the full tile, between the hot tiles of the neighbouring waves."""
    r = _run("adversarial", train)
    assert r["tiles_max"] >= 8, r
    assert r["tiles_adv"] > 0 and r["counters"][2] >= r["tiles_adv"], r


@pytest.mark.gpu
@TRAIN
def test_more_agents_than_mirror_rows(train):
    """At least 256 agents of eight brains in a 30 x 30 world: more rows than the LDS can mirror, and the brains' rows interleave, so every
    tile holds mirrored rows next to rows beyond the mirror -- the whole tile reads from memory; two tiles per wave, one brain adversarial."""
    r = _run("beyond-mirror", train)
    assert r["agents_min"] * ROW_BYTES > LDS_BYTES, r
    assert r["tiles_max"] >= 9 and r["counters"][2] > 0, r


@pytest.mark.gpu
@TRAIN
def test_big_grid_rows_from_memory(train):
    """The same population on a 64 x 64 grid, whose planes leave the mirror still fewer rows."""
    r = _run("big-grid", train)
    assert r["agents_min"] * ROW_BYTES > LDS_BYTES, r
    assert r["tiles_max"] >= 9, r
