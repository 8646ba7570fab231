"""The redo of k_run's certified one-wave dueling tile on the GPU, through the tuning library.  The certified tile keeps no
tile descriptor: its per-lane operands come from the tile row's list entry where they are used, and a tile with a greedy row that fails the
certificate stores nothing and reports it -- the caller then builds a descriptor from the tile index and runs the full tile in the same loop
iteration.  These cases put that redo next to hot tiles: a world whose brain 0 is the adversarial brain of tests/test_hip_onewave_cert.py
(every tile of it is redone) and whose brain 1 is ordinary; the adversarial brain exploring (the redo's recomputed Philox draw must give the
full path's actions); eight brains with two tiles per wave (hot tile, redo, next hot tile on one wave); a brain without a live agent and a
tile with a single valid row.  Every case compares states, actions, rewards, done flags and Agent.state rows with the forced full path (run
mask 64) and with the two-launch loop, in launches of 1, 7 and the remaining ticks, for TRAIN 0 and TRAIN 1.  Tile counts come from the
brains' row counts, sampled before every tick on a handle that runs one-tick launches (whose states are compared too)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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

# adv: the adversarial brains; eps: the brains' exploration rates (TRAIN 0: fixed; TRAIN 1: every row of the schedule)
SHAPES = {"mixed": dict(R=8, n_brains=2, max_agents=100, n_new=90, thr=70, adv=[0], eps=[0.0, 0.1], chunks=(1, 7, 22)),
          "exploring": dict(R=8, n_brains=2, max_agents=100, n_new=90, thr=70, adv=[0], eps=[0.3, 0.0], chunks=(1, 7, 22)),
          "two-tiles": dict(R=4, n_brains=8, max_agents=250, n_new=272, thr=240, adv=[1, 3, 5, 7], eps=[0.0] * 8, chunks=(1, 7, 12)),
          "edges": dict(R=6, n_brains=3, max_agents=100, n_new=96, thr=70, adv=[1], eps=[0.0, 0.0, 0.05], chunks=(1, 7, 12))}

def make(shape):
    sh = SHAPES[shape]
    dw = DeviceWorlds(n_worlds=sh["R"], width=30, height=30, max_agents=sh["max_agents"], n_brains=sh["n_brains"], static_families=True,
                      limit_reproduction=False, incentivize_killing=True, seed=47, world_base=5, device="cuda:0")
    assert dw.cap <= 512
    brains = []
    for k in range(sh["n_brains"]):
        w = adversarial(200 + k) if k in sh["adv"] else bench.brain_weights("PERD3QN" if k %% 2 == 0 else "D3QN", 700 + k)
        kind = _lib.PERD3QN if k in sh["adv"] or k %% 2 == 0 else _lib.D3QN
        brains.append((kind, sh["eps"][k], pack_brain_weights(kind, w, "cuda:0")))
    dw.set_brains(brains)
    dw.reset_synthetic(sh["n_new"])
    if shape == "two-tiles":
        # an even deal at reset (the synthetic reset draws the brains: 20 to 50 agents each): 34 agents = two tiles per brain, sixteen per world
        torch.cuda.synchronize()
        br = dw.s["a_brain"].cpu().numpy().copy()
        br[:, :] = np.arange(br.shape[1])[None, :] %% sh["n_brains"]
        dw.s["a_brain"].copy_(torch.as_tensor(br, device="cuda:0"))
        torch.cuda.synchronize()
        _lib.check(lib.rl_bind_state(dw.handle, ctypes.byref(dw._state)), "rl_bind_state")   # (state rewritten by the host, as load_world does)
    if shape == "edges":
        # world 0: brain 2 has no live agent; world 1: the adversarial brain 1 keeps ONE agent (a tile with a single valid row, redone);
        # world 2: brain 0 holds exactly 33 agents (its second tile has a single valid row), the others go to brain 2
        torch.cuda.synchronize()
        n = dw.s["n_agents"].cpu().numpy()
        br = dw.s["a_brain"].cpu().numpy().copy()
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
    nb, thr, n_new, adv = sh["n_brains"], sh["thr"], sh["n_new"], sh["adv"]
    sched = lambda n: np.ascontiguousarray(np.array(sh["eps"], np.float32)[None, :].repeat(n, 0))   # noqa: E731
    res = dict(shape=shape, train=train, diff_full=[], diff_loop=[], diff_single=[], tiles_adv=0, tiles_all=0, tiles_max=0, tiles_min=99,
               rows_min_reset=0, rows_adv=0, empty_brain=0, single_row_tiles=0, single_row_adv=0, ticks=0)
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
    res["rows_min_reset"] = int(rows(cert).min())
    counters()
    got, one, forced = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    for n in sh["chunks"]:
        lib.rl_debug_set_run_mask(0)
        run(cert, n)
        a = snap(cert)
        got = [x + y for x, y in zip(got, counters())]
        for i in range(n):
            c = rows(single)   # what this tick's policy half reads: its tiles are ceil(rows / 32) per brain
            t = (c + 31) // 32
            res["tiles_adv"] += int(t[:, adv].sum()); res["tiles_all"] += int(t.sum()); res["rows_adv"] += int(c[:, adv].sum())
            res["tiles_max"] = max(res["tiles_max"], int(t.sum(1).max())); res["tiles_min"] = min(res["tiles_min"], int(t.sum(1).min()))
            res["empty_brain"] += int((c == 0).sum()); res["single_row_tiles"] += int((c %% 32 == 1).sum())
            res["single_row_adv"] += int((c[:, adv] %% 32 == 1).sum())
            run(single, 1)
        s1 = snap(single)
        one = [x + y for x, y in zip(one, counters())]
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
    res["counters"] = got; res["single"] = one; res["forced"] = forced
    res["acted"] = int(cert.acted_total.item()); res["refills"] = int(cert.refill_count.item())
    print("RESULT " + json.dumps(res), flush=True)

for shape, train in (%(cases)s):
    case(shape, train)
'''


def _run(shape, train):
    from reinlife_amd import build
    tune = build.TUNE_LIB_PATH
    if not os.path.exists(tune):
        pytest.skip("the tuning library is not built (RL_TUNE=1 python reinlife_amd/build.py; __graft_entry__.build() builds it)")
    env = dict(os.environ, REINLIFE_HIP_LIB=tune)
    env.pop("RL_TUNE", None)
    out = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, cases='("%s", %d),' % (shape, train))], env=env, capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = [json.loads(line[len("RESULT "):]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    assert len(res) == 1
    print(res[0])
    return res[0]


def _same(r):
    assert r["ticks"] <= 60, r
    assert r["diff_full"] == [], r       # against run mask 64: the full pair finish / the full one-wave tile
    assert r["diff_loop"] == [], r       # against rl_policy_act + rl_tick_refill
    assert r["diff_single"] == [], r     # one launch of N ticks against N launches of one tick
    assert r["forced"] == [0, 0, 0], r   # the forced full path never enters the certified finish
    assert r["counters"] == r["single"], r


def _redone_tiles_are_the_adversarial_brains(r):
    """Greedy adversarial brains: every row of theirs fails the certificate, so every tile of theirs is redone -- tiles_adv of them, from the
    row counts.  An ORDINARY row fails it too now and then (2.7e-4 of rows), and its tile is redone as well: those rows are
    counted exactly (greedy - certified - the adversarial brains' rows), each adds at most one tile, and they stay below 1e-3 of the rows."""
    greedy, certified, fell_back = r["counters"]
    ordinary_failed = greedy - certified - r["rows_adv"]
    assert 0 <= ordinary_failed <= 1e-3 * greedy, r
    assert r["tiles_adv"] > 0 and r["tiles_all"] > r["tiles_adv"], r
    assert r["tiles_adv"] <= fell_back <= r["tiles_adv"] + ordinary_failed, r
    assert certified > 0, r


TRAIN = pytest.mark.parametrize("train", [0, 1], ids=["TRAIN0", "TRAIN1"])


@pytest.mark.gpu
@TRAIN
def test_one_wave_redoes_its_tile_next_to_hot_tiles(train):
    """Brain 0 adversarial and greedy, brain 1 ordinary: every tile of brain 0 is redone while brain 1's tiles finish hot on the neighbouring
    waves.  The fallback-tile counter is brain 0's tile count, summed over worlds and ticks from the row counts -- plus the tiles of the few
    ordinary rows that fail the certificate, which the counters give exactly."""
    r = _run("mixed", train)
    _same(r)
    _redone_tiles_are_the_adversarial_brains(r)


@pytest.mark.gpu
@TRAIN
def test_redo_of_an_exploring_brain_draws_the_full_paths_actions(train):
    """The adversarial brain with eps 0.3 (fixed in TRAIN 0, from the schedule in TRAIN 1): its tiles are redone for their greedy rows, and the
    redo's recomputed Philox draw gives the exploring rows the actions of the full path and of the two-launch loop."""
    r = _run("exploring", train)
    _same(r)
    greedy, certified, fell_back = r["counters"]
    assert 0 < greedy < r["acted"], r    # some rows explored
    assert fell_back > 0 and fell_back <= r["tiles_adv"], r   # (a tile whose valid rows ALL explore is not redone)


@pytest.mark.gpu
@TRAIN
def test_two_tiles_per_wave_hot_redo_hot(train):
    """Eight brains of at least 33 agents each: at least nine tiles, so a wave runs tile t and tile t + 8 -- hot tile, redo (odd brains are
    adversarial), next hot tile."""
    r = _run("two-tiles", train)
    _same(r)
    assert r["rows_min_reset"] >= 33, r
    assert r["tiles_max"] >= 9, r
    _redone_tiles_are_the_adversarial_brains(r)


@pytest.mark.gpu
@TRAIN
def test_brain_without_agents_and_tiles_with_one_valid_row(train):
    """A world one of whose brains has no live agent (no tile for it), the adversarial brain with ONE agent (a redone tile with a single valid
    row) and a brain of 33 agents (a hot tile with a single valid row)."""
    r = _run("edges", train)
    _same(r)
    assert r["empty_brain"] > 0 and r["single_row_tiles"] > r["single_row_adv"] > 0, r
    _redone_tiles_are_the_adversarial_brains(r)
