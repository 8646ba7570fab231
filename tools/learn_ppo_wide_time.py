"""What a wide PPO rollout costs on ONE MI355X (rl_learn_rollout_wide + rl_learn_ppo_wide, reinlife_amd/csrc/rl_learn_ppo_wide.hip) next to
rl_learn_rollout + rl_learn_ppo, for 1 and 8 learners on FULL rings of 50,000 rows whose window is the whole ring, ONE rollout of
k_epoch = 3 epochs per call:

  ppo     device-event times of ONE rl_learn_rollout (two launches) and ONE rl_learn_ppo call (one launch, one 512-thread workgroup per
          learner): 1 rollout x 32 rows -- the yardstick, unchanged code, ALTERNATING with the wide pair in the same process
  wide    device-event times of ONE rl_learn_rollout_wide (two launches) and ONE rl_learn_ppo_wide call: 1 rollout x 32 / 256 / 1024 /
          2048 rows, 3 x 3 + 3 = 12 launches, one workgroup per (learner, 32-row tile) in the two tile passes; the event pairs include
          the launches' host-side issue gaps

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls in one process.  The line to read is "us per
sampled row": draw + update of a call over its rollout's rows.

EXPECTATIONS, written down before the first measurement and derived from the code alone:
  E1  the one-tile wide call is NOT slower than rl_learn_ppo: per epoch it makes three trunk passes where k_learn_ppo makes two (the s
      forward is made again in the second tile pass) and it crosses eleven launch boundaries, but Adam on 107,529 parameters and the
      packer move off ONE workgroup onto 421 and 17 -- the other wide learners' finding, a supposition here.  CONFIRMED when the
      measured one-tile update takes at most 1.0 x rl_learn_ppo's, REFUTED otherwise.
  E2  the cost per sampled row falls about with the tile count while learners x tiles <= 256 CUs: 125 KB of LDS let one workgroup onto a
      CU, so every tile of such a call runs at once.  What grows with the rollout: the chain (E3) and the update's read of T partial
      gradients (T x 430 KB per learner and epoch: 27.5 MB at 2048 rows, microseconds at HBM speed).  8 learners x 1024 rows = 256 tiles
      is the edge; 8 x 2048 queues two rounds.  CONFIRMED when every call with learners x tiles <= 256 takes at most 1.25 x the one-tile
      call of the same learner count plus E3's upper estimate for its rows.  (That allowance is generous -- E3's interval is wide -- so
      the tool also prints the ratio WITHOUT it; read a CONFIRMED with both figures.)
  E3  the serial GAE chain: one thread, per row one LDS read, one multiply and one dependent add.  If the reads are pipelined in front of
      the arithmetic a row costs two dependent VALU operations, about 16 clocks: 2,048 rows = 33 k clocks = 14 us at 2.4 GHz per epoch;
      if every row waits for its own LDS round trip (about 100 clocks) it is 85 us per epoch.  Nobody has measured it.  TIMED HERE BY
      DIFFERENCE, not by stamps: (update at 2048 rows - update at 32 rows) / 3 epochs for ONE learner, where all 64 tiles run at once
      (E2), minus 8 us per epoch for the update's 27.5 MB of partial gradients at 3.5 TB/s -- an estimate that charges the chain with
      everything else that grows.  CONFIRMED when that lies in [14, 85] us per epoch, REFUTED otherwise.

    python tools/learn_ppo_wide_time.py [--out profiles/learn_ppo_wide.txt] [--reps 200]

No performance threshold is set: the figures are recorded and the three expectations judged.  NOT measured here: a trainer() run with
learn_batch={"PPO": B}, hardware counters, several GPUs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _ring  # noqa: E402

LEARNERS = (1, 8)
BATCHES = (32, 256, 1024, 2048)
RING, TILE, CUS, K_EPOCH = 50_000, 32, 256, 3
CHAIN_LO_US, CHAIN_HI_US, APPLY_US = 14.0, 85.0, 8.0   # per epoch at 2048 rows (E3)


def _ppo_ring(torch, rng, dev):
    r = _ring(torch, rng, dev, RING)
    r["prob"] = torch.as_tensor(rng.uniform(0.05, 0.5, size=RING).astype("float32"), device=dev)
    return r


def _stats(t, reps):
    t = sorted(t)
    return t[reps // 2], t[0], t[reps * 9 // 10]


def measure(reps, say):
    import numpy as np
    import torch
    from reinlife_amd import Models
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rng = np.random.RandomState(1)
    rings = [_ppo_ring(torch, rng, dev) for _ in range(max(LEARNERS))]
    med = {}

    def pair(ls):   # every repetition sees the same window: the whole ring (a fill of one element, in stream order)
        for l in ls:
            l.seen.fill_(0)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(); slots = dw.draw_rollout(ls, 1); e[1].record(); dw.learn(ls, 1, slots=slots); e[2].record()
        return e
    for n in LEARNERS:
        for batch in BATCHES:
            narrow = [DeviceLearner(Models.PPO(), dev, ring=r, rollout=True) for r in rings[:n]]
            wide = [DeviceLearner(Models.PPO(), dev, ring=r, rollout=True, rollout_batch=batch) for r in rings[:n]]
            for _ in range(20):
                pair(narrow); pair(wide)
            torch.cuda.synchronize()
            ev = [(pair(narrow), pair(wide)) for _ in range(reps)]   # alternating: both see the same clocks and the same neighbours
            torch.cuda.synchronize()
            dw.check_error_flag()
            assert all(l.state.cpu().tolist() == [K_EPOCH * (20 + reps), 20 + reps] for l in narrow + wide)
            for which, tag, rows, names in ((0, "ppo", 32, ("rl_learn_rollout", "rl_learn_ppo")), (1, "wide", batch, ("rl_learn_rollout_wide", "rl_learn_ppo_wide"))):
                what = "1 rollout x %d rows x %d epochs, %d learner(s), ring %d (all fresh)" % (rows, K_EPOCH, n, RING)
                draw = _stats([e[which][0].elapsed_time(e[which][1]) * 1e3 for e in ev], reps)
                learn = _stats([e[which][1].elapsed_time(e[which][2]) * 1e3 for e in ev], reps)
                say("%-5s draw   %s, %s | median %9.2f us (min %9.2f, p90 %9.2f) over %d repetitions" % ((tag, names[0], what) + draw + (reps,)))
                say("%-5s learn  %s, %s | median %9.2f us (min %9.2f, p90 %9.2f) over %d repetitions" % ((tag, names[1], what) + learn + (reps,)))
                med[(tag, n, batch)] = (draw[0], learn[0])
            (nd, nl), (wd, wl) = med[("ppo", n, batch)], med[("wide", n, batch)]
            per_row, base = (wd + wl) / batch, (nd + nl) / 32
            say("row   %d learner(s), %d rows | draw + update %8.4f us per sampled row = %6.2f x fewer than rl_learn_rollout + rl_learn_ppo's %.4f "
                "(update alone: %.4f against %.4f)" % (n, batch, per_row, base / per_row, base, wl / batch, nl / 32))
    return med


def judge(med, say):
    for n in LEARNERS:
        narrow, one = med[("ppo", n, 32)][1], med[("wide", n, 32)][1]
        say("E1    %d learner(s): one-tile wide update %.2f us, rl_learn_ppo %.2f us in the same process (%.2f x): %s"
            % (n, one, narrow, one / narrow, "CONFIRMED" if one <= narrow else "REFUTED: the one-tile wide call is SLOWER than rl_learn_ppo"))
        inside = [b for b in BATCHES if n * ((b + TILE - 1) // TILE) <= CUS]
        worst = max((med[("wide", n, b)][1] - K_EPOCH * CHAIN_HI_US * b / 2048) / one for b in inside)
        falls = all((sum(med[("wide", n, b)])) / b < (sum(med[("wide", n, a)])) / a for a, b in zip(BATCHES, BATCHES[1:]))
        raw = max(med[("wide", n, b)][1] / one for b in inside)
        say("E2    %d learner(s): rollouts %s keep learners x tiles <= %d; less E3's upper estimate the slowest of their updates takes %.2f x the "
            "one-tile update (<= 1.25 expected): %s (without that allowance: %.2f x); draw + update per sampled row %s with every widening"
            % (n, list(inside), CUS, worst, "CONFIRMED" if worst <= 1.25 else "REFUTED", raw, "falls" if falls else "DOES NOT fall"))
    chain = (med[("wide", 1, 2048)][1] - med[("wide", 1, 32)][1]) / K_EPOCH - APPLY_US
    say("E3    the GAE chain of 2,048 rows BY DIFFERENCE (no stamps): (update at 2048 rows %.2f us - at 32 rows %.2f us) / %d epochs - %.0f us for the "
        "partial gradients' read = %.2f us per epoch = %.1f ns per row (expected 14 .. 85 us): %s"
        % (med[("wide", 1, 2048)][1], med[("wide", 1, 32)][1], K_EPOCH, APPLY_US, chain, chain * 1e3 / 2048,
           "CONFIRMED" if CHAIN_LO_US <= chain <= CHAIN_HI_US else "REFUTED"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    judge(measure(max(args.reps, 200), say), say)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_ppo_wide_time.py on ONE MI355X, one process: device events around the draw (two launches) and around the update (rl_learn_ppo:\n"
                     "# one launch; rl_learn_ppo_wide: 12 launches -- the event pair includes their host-side issue gaps), ONE rollout of 3 epochs per call,\n"
                     "# the narrow and the wide pair ALTERNATING, 20 warm-up + >= 200 repetitions per figure, full rings of 50,000 rows, all rows fresh.\n"
                     "# Expected BEFORE measuring (the tool's docstring has the derivation): E1 the one-tile wide update is not slower than rl_learn_ppo;\n"
                     "# E2 updates with learners x tiles <= 256 take at most 1.25 x the one-tile update plus the chain; E3 the GAE chain of 2,048 rows takes\n"
                     "# 14 .. 85 us per epoch, timed by difference.\n"
                     "# NOT measured: a trainer() run with learn_batch={\"PPO\": B}, hardware counters, several GPUs.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
