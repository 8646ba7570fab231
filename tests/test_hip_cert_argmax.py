"""The certified argmax of k_run's dueling pair tiles on the GPU, through the tuning library: run mask 64 forces the full
finish (V computed), so the same launch can be compared with itself -- states, actions and rewards must be identical -- and the tuning
build's counters show how often the certificate held and how often the value branch ran after all."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r'''
import argparse, ctypes, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch, bench
from reinlife_amd import _lib
from reinlife_amd.worlds import DeviceWorlds, pack_brain_weights
lib = _lib.lib()

def counters():
    a, b = (ctypes.c_ulonglong * 4)(), (ctypes.c_ulonglong * 4)()
    assert lib.rl_debug_cert_counters(a) == 0 and lib.rl_debug_cert_counters_all(b) == 0
    return [a[i] + b[i] for i in range(3)]

def adversarial(seed):
    # advantage head weights zero: every row's advantages are the head's biases, a_1 and a_3 one ulp apart; a value bias of 300 merges them
    # in q = (a + v) - m, so the full path picks 1 where the advantages alone say 3
    w = bench.brain_weights("PERD3QN", seed).astype(np.float32).copy()
    o = 153 * 128 + 128 + 128 * 128 + 128
    w[o:o + 8 * 128] = 0.0
    w[o + 8 * 128:o + 8 * 128 + 8] = np.array([0, 1, 0, np.nextafter(np.float32(1), np.float32(2)), 0, 0, 0, 0], np.float32)
    w[-1] = 300.0
    return w

def make(wl, adv):
    if adv:
        dw = DeviceWorlds(n_worlds=256, width=30, height=30, max_agents=100, n_brains=2, static_families=True, seed=1, device="cuda:0")
        dw.set_brains([(_lib.PERD3QN, 0.0, pack_brain_weights(_lib.PERD3QN, adversarial(100 + k), "cuda:0")) for k in range(2)])
        dw.reset_synthetic(100)
        return dw
    return bench.make_worlds(argparse.Namespace(worlds=256, workload=wl, seed=1), 0, "cuda:0")

def run(wl, train, adv, mask, ticks):
    lib.rl_debug_set_run_mask(mask)
    dw = make(wl, adv)
    kw = {}
    if train:
        dw.enable_tracking(True)
        kw = dict(eps_schedule=np.linspace(0.3, 0.0, ticks, dtype=np.float32)[:, None].repeat(2, 1).copy(), trk_skip=1)
    counters()
    dw.run(ticks, 70, 100, **kw)
    torch.cuda.synchronize()
    c = counters()
    snap = {k: v.cpu().numpy().copy() for k, v in dw.s.items()}
    for k in ("actions", "reward", "done", "n_acted", "acted_total", "refill_count"):
        snap[k] = getattr(dw, k).cpu().numpy().copy()
    snap["obs"] = dw.obs_state().cpu().numpy().copy()
    lib.rl_debug_set_run_mask(0)
    return snap, c

for wl, train, adv, ticks in ((%(cases)s)):
    full, cf = run(wl, train, adv, 64, ticks)
    cert, cc = run(wl, train, adv, 0, ticks)
    diff = [k for k in full if not np.array_equal(full[k], cert[k], equal_nan=True)]
    print("CASE", wl, train, adv, "diff", diff, "counters", cc, "forced", cf, flush=True)
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
    res = []
    for line in out.stdout.splitlines():
        if line.startswith("CASE"):
            head, rest = line.split(" diff ")
            diff, cnt = rest.split(" counters ")
            cc, cf = cnt.split(" forced ")
            res.append((head, eval(diff), eval(cc), eval(cf)))
    return res


@pytest.mark.gpu
def test_certified_argmax_matches_the_full_finish_on_the_bench_workloads():
    """configs[3] (TRAIN 0 and TRAIN 1 with an epsilon schedule) and configs[4], 256 worlds x 300 ticks: identical to the forced full finish."""
    res = _run('("c4", 0, False, 300), ("c4", 1, False, 300), ("c5", 0, False, 300)')
    assert len(res) == 3
    for head, diff, (greedy, certified, fell_back), forced in res:
        assert diff == [], (head, diff)
        assert forced == [0, 0, 0], head        # the forced full finish never enters the certified one
    (_, _, c4, _), (_, _, c4t, _), (_, _, c5, _) = res
    assert c4[0] > 1_000_000 and c4[0] - c4[1] < 0.01 * c4[0], c4   # the bench workload: well under 1 % of greedy rows fall back
    assert c4t[0] > 0 and c4t[1] > 0


@pytest.mark.gpu
def test_adversarial_brain_falls_back_and_keeps_the_full_paths_action():
    """Advantages one ulp apart and a value bias of 300: q rounds them together, the first of them wins in the full path.  The certificate must
    refuse those rows, the value branch must run (counters), and the results must equal the forced full finish."""
    res = _run('("adv", 0, True, 40),')
    assert len(res) == 1
    head, diff, (greedy, certified, fell_back), forced = res[0]
    assert diff == [], (head, diff)
    assert greedy > 0 and certified == 0 and fell_back > 0, (greedy, certified, fell_back)
