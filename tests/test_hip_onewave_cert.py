"""k_run's certified ONE-WAVE dueling tile on the GPU, through the tuning library, in worlds of five to eight tiles -- three
dueling brains with an uneven split, and more than 128 agents of two brains.  Before 5.15 such worlds ran the full tile (V computed); now
every tile of a TRAIN 0 / 1 launch certifies its argmax.  Run mask 64 forces the full path, so the same launch is compared with itself and
with the two-launch loop: states, actions, rewards and rows must be identical.  The tile count is asserted, not trusted: a refill threshold
above 128 agents keeps every policy half at five tiles or more (the tiles of a world are at least ceil(n / 32)), and the count is sampled
from the brains' row counts at every launch boundary."""
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
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch, bench
from reinlife_amd import _lib
from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
lib = _lib.lib()
R = 12

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

SHAPES = {"three-brains": dict(n_brains=3, max_agents=150, n_new=140, thr=130, names=["PERD3QN", "D3QN", "PERD3QN"]),
          "crowded-two": dict(n_brains=2, max_agents=200, n_new=190, thr=170, names=["PERD3QN", "PERD3QN"]),
          "adversarial": dict(n_brains=3, max_agents=150, n_new=140, thr=130, names=["PERD3QN"] * 3),
          "tied": dict(n_brains=3, max_agents=150, n_new=140, thr=130, names=["PERD3QN", "D3QN", "PERD3QN"])}

def tied(name, k):
    # advantage heads whose eight rows are copies of two or three distinct rows: every row's maximum is an EXACT tie (tests/test_policy_rows_cpu.py)
    import test_policy_rows_cpu as pr
    return pr.tied_weights(name, list(pr.TIE_PATTERNS.values())[k], seed=60 + k)

def make(shape, eps):
    sh = SHAPES[shape]
    dw = DeviceWorlds(n_worlds=R, width=30, height=30, max_agents=sh["max_agents"], n_brains=sh["n_brains"], static_families=True,
                      limit_reproduction=False, incentivize_killing=True, seed=31, world_base=3, device="cuda:0")
    brains = []
    for k, name in enumerate(sh["names"]):
        kind = _lib.KIND_BY_METHOD[name]
        w = adversarial(100 + k) if shape == "adversarial" else tied(name, k) if shape == "tied" else bench.brain_weights(name, 900 + k)
        brains.append((kind, eps[k], pack_brain_weights(kind, w, "cuda:0")))
    dw.set_brains(brains)
    dw.reset_synthetic(sh["n_new"])
    return dw

def tiles(dw):
    n = dw.s["n_agents"].cpu().numpy()
    br = dw.s["a_brain"].cpu().numpy()
    out = []
    for w in range(R):
        cnt = np.bincount(br[w, :n[w]].astype(np.int64), minlength=dw.n_brains)
        out.append(int(sum((int(c) + 31) // 32 for c in cnt)))
    return out, [int(x) for x in n]

def snap(dw):
    torch.cuda.synchronize()
    dw.check_error_flag()
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

def schedule(n_brains, train, t0, n):   # TRAIN 1: a per-tick epsilon schedule (rows t0 .. t0 + n of one fixed table)
    tab = np.linspace(0.3, 0.0, 64, dtype=np.float32)[:, None].repeat(n_brains, 1)
    return np.ascontiguousarray(tab[t0:t0 + n])

def case(shape, train, chunks):
    sh = SHAPES[shape]
    nb, thr, n_new = sh["n_brains"], sh["thr"], sh["n_new"]
    eps = [0.0] * nb if shape in ("adversarial", "tied") else [0.2 * (k %% 2) for k in range(nb)]
    res = dict(shape=shape, train=train, thr=thr, tiles_min=99, tiles_max=0, agents_min=9999, agents_max=0, diff_full=[], diff_loop=[], diff_single=[])
    def note(dw):
        t, n = tiles(dw)
        res["tiles_min"] = min(res["tiles_min"], min(t)); res["tiles_max"] = max(res["tiles_max"], max(t))
        res["agents_min"] = min(res["agents_min"], min(n)); res["agents_max"] = max(res["agents_max"], max(n))
    def run(dw, t0, n):
        kw = dict(eps_schedule=schedule(nb, train, t0, n), trk_skip=1) if train else {}
        dw.run(n, thr, n_new, **kw)
    # product path (certified one-wave tiles) / forced full path / one-tick launches on the product path / the two-launch loop
    lib.rl_debug_set_run_mask(0)
    cert, single, loop = make(shape, eps), make(shape, eps), make(shape, eps)
    lib.rl_debug_set_run_mask(64)
    full = make(shape, eps)
    for dw in (cert, single, full):
        assert dw.run_supported()
        if train:
            dw.enable_tracking(True)
    counters()
    t0 = 0
    got = [0, 0, 0]
    forced = [0, 0, 0]
    for n in chunks:
        note(cert)
        lib.rl_debug_set_run_mask(0)
        run(cert, t0, n)
        a = snap(cert)
        got = [x + y for x, y in zip(got, counters())]
        for i in range(n):
            run(single, t0 + i, 1)
        s1 = snap(single)
        counters()
        lib.rl_debug_set_run_mask(64)
        run(full, t0, n)
        f = snap(full)
        forced = [x + y for x, y in zip(forced, counters())]
        lib.rl_debug_set_run_mask(0)
        for i in range(n):
            if train:
                loop._set_epsilons(schedule(nb, train, t0 + i, 1)[0].tolist())
            loop.act(); loop.tick_refill(thr, n_new)
        l = snap(loop)
        res["diff_full"] += ["%%d:%%s" %% (t0, k) for k in differ(a, f)]
        res["diff_loop"] += ["%%d:%%s" %% (t0, k) for k in differ(a, l)]
        res["diff_single"] += ["%%d:%%s" %% (t0, k) for k in differ(a, s1)]
        t0 += n
    note(cert)
    res["counters"] = got; res["forced"] = forced; res["refills"] = int(cert.refill_count.item())
    print("RESULT " + json.dumps(res), flush=True)

for shape, train, chunks in (%(cases)s):
    case(shape, train, chunks)
'''


def _run(cases):
    from reinlife_amd import build
    tune = build.TUNE_LIB_PATH
    if not os.path.exists(tune):
        pytest.skip("the tuning library is not built (RL_TUNE=1 python reinlife_amd/build.py; __graft_entry__.build() builds it)")
    env = dict(os.environ, REINLIFE_HIP_LIB=tune)
    env.pop("RL_TUNE", None)
    out = subprocess.run([sys.executable, "-c", SCRIPT % dict(root=ROOT, cases=cases)], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    res = [json.loads(line[len("RESULT "):]) for line in out.stdout.splitlines() if line.startswith("RESULT ")]
    for r in res:
        print(r)
    return res


def _check_tiles(r):
    assert r["thr"] > 128 and r["agents_min"] >= r["thr"], r           # every policy half: at least thr agents = five tiles or more
    assert 5 <= r["tiles_min"] and r["tiles_max"] <= 8, r              # ... and the sampled worlds: five to eight
    assert r["refills"] > 0, r


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["three-brains", "crowded-two"])
@pytest.mark.parametrize("train", [0, 1], ids=["TRAIN0", "TRAIN1"])
def test_certified_one_wave_tile_in_worlds_of_five_to_eight_tiles(shape, train):
    """Product path against the forced full path (run mask 64), against the two-launch loop, and one launch of N ticks against N launches of
    one tick (N = 1, 7, 10, 25: odd and even, the Agent.state ping-pong): identical states, actions, rewards and rows."""
    res = _run('("%s", %d, (1, 7, 10, 25)),' % (shape, train))
    assert len(res) == 1
    r = res[0]
    _check_tiles(r)
    if shape == "crowded-two":
        assert r["agents_max"] > 128, r
    assert r["diff_full"] == [], r
    assert r["diff_loop"] == [], r
    assert r["diff_single"] == [], r
    greedy, certified, fell_back = r["counters"]
    assert greedy > 10_000 and certified > 0.9 * greedy, r             # these worlds were on the full path before: certified now
    assert r["forced"] == [0, 0, 0], r                                 # the forced full path never enters the certified finish


@pytest.mark.gpu
def test_adversarial_brains_fall_back_on_the_one_wave_tile():
    """Advantages one ulp apart and a value bias of 300 (tests/test_hip_cert_argmax.py) in a six-tile world: no row is certified, every tile
    runs the full tile after all, and the results equal the forced full path and the two-launch loop."""
    res = _run('("adversarial", 0, (1, 8, 15)),')
    assert len(res) == 1
    r = res[0]
    _check_tiles(r)
    assert r["diff_full"] == [] and r["diff_loop"] == [] and r["diff_single"] == [], r
    greedy, certified, fell_back = r["counters"]
    assert greedy > 0 and certified == 0 and fell_back > 0, r


@pytest.mark.gpu
def test_exactly_tied_advantages_on_the_one_wave_tile():
    """Advantage heads whose rows are copies of two or three distinct rows (every row's maximum is an exact tie, all brains greedy) in a
    six-tile world: whether a row certifies or falls back, the product path, the forced full path, one-tick launches and the two-launch
    loop choose the same (first) maximum.  The counters are reported, not asserted: a tie between the top two advantages cannot be certified
    unless the first of them is action 0."""
    res = _run('("tied", 0, (1, 8, 15)),')
    assert len(res) == 1
    r = res[0]
    _check_tiles(r)
    assert r["diff_full"] == [] and r["diff_loop"] == [] and r["diff_single"] == [], r
    greedy, certified, fell_back = r["counters"]
    print("tied: greedy rows %d, certified %d, fallback tiles %d" % (greedy, certified, fell_back))
    assert greedy > 0 and r["forced"] == [0, 0, 0], r
