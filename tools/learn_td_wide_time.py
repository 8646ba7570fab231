"""What a wide PERDQN minibatch costs on ONE MI355X (rl_learn_td_wide, rl_learn_td_wide_draw, rl_learn_td_wide_draw_rank and the stamp in
front, reinlife_amd/csrc/rl_learn_td_wide.hip, rl_learn_prio.hip, rl_learn_rank.hip, rl_learn_td.hip) for 1 and 8 learners on FULL rings of
20,000 rows (a PERDQN brain's memory_size), ONE update per call as PERDQNAgent.train_model() makes, every piece timed on its own:

  td      device-event times of ONE rl_learn_td_draw (2 launches) and ONE rl_learn_td (1 launch) at batch 64 -- the yardsticks, unchanged
          code, ALTERNATING with the wide calls, repetition by repetition, in the same loop
  tdwide  device-event times, at batch 64 / 256 / 1024 / 2048, of ONE rl_learn_td_stamp over a window of the WHOLE ring (2 launches; seen
          is set back to 0 outside the clock), ONE rl_learn_td_wide_draw (2 launches), ONE rl_learn_td_wide_draw_rank (8 launches,
          stratified) and ONE rl_learn_td_wide (6 launches) on the race draw's table

Every figure is the median (min, p90) over >= 200 repetitions after 20 warm-up calls in one process; the event pairs include the
launches' host-side issue gaps.

EXPECTATIONS, written down before the first measurement (DESIGN.md 5.32 has the derivations):
  E1  the one-tile call (batch 64, one learner) costs about what rl_learn_td costs (146 us when last measured): the tile pass is
      k_learn_perdqn's step without Adam and the packer, which move to 57 and 17 workgroups; against that stand five more launch gaps and
      the weights pass.  Expected: within 25 % of rl_learn_td's median of the same loop, either side.
  E2  the update is flat in the batch while learners x tiles <= 256 CUs at one 110 KB workgroup per CU: one learner from batch 64 (1 tile)
      to 2048 (32 tiles), and eight learners up to 2048 (256 tiles), grow by less than 40 % -- the weights pass' 2048 pow() calls and the
      update's 32 partials per parameter are what grows.
  E3  the rank draw is flat in the batch (a sort and a prefix sum of the ring, then one thread per draw): batch 2048 costs less than
      1.15 x batch 64.
  E4  the race draw is one workgroup per draw over all 20,000 rows: it grows with the batch, by 1.3 x to 4 x from batch 64 to 2048 for
      one learner (rl_learn_prioritized_wide_draw on 10,000 rows: 38.4 -> 57.9 us), and the rank draw is the cheaper one at 2048.
  E5  the stamp of a whole ring is 313 workgroups per learner, two to a CU: one round for one learner -- about one tile pass' forward
      half, 50 .. 200 us -- and about five rounds for eight learners.

    python tools/learn_td_wide_time.py [--out profiles/learn_td_wide.txt] [--reps 200]

No performance threshold is set: the figures are recorded and the expectations judged.  NOT measured here: a trainer() run with
learn_batch={"PERDQN": B}, hardware counters, several GPUs."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEARNERS = (1, 8)
BATCHES = (64, 256, 1024, 2048)
RING, N_STEPS, WARM = 20_000, 1, 20


def _ring(rng, dev):
    import numpy as np
    import torch

    def rows():
        x = (rng.random_sample((RING, 153)) < 0.15) * rng.choice(np.array([1.0, -1.0, 0.5], np.float32), size=(RING, 153))
        return torch.as_tensor(x.astype(np.float32), device=dev)
    return {"state": rows(), "state_prime": rows(), "action": torch.as_tensor(rng.randint(0, 8, size=RING).astype(np.int8), device=dev),
            "reward": torch.as_tensor(rng.choice(np.array([0, 0.05, 0.3, -1, 5, -10], np.float32), size=RING), device=dev),
            "done": torch.as_tensor((rng.random_sample(RING) < 0.2).astype(np.uint8), device=dev), "prob": None,
            "age": torch.as_tensor(rng.randint(0, 200, size=RING).astype(np.int32), device=dev),
            "count": torch.full((1,), RING, dtype=torch.int64, device=dev)}


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
    rings = [_ring(rng, dev) for _ in range(max(LEARNERS))]
    med = {}

    def line(tag, part, entry, batch, n, t):
        m, lo, p90 = _stats(t, reps)
        say("%-6s %-5s %s, %d step x batch %d, %d learner(s), ring %d | median %8.2f us (min %8.2f, p90 %8.2f) over %d repetitions"
            % (tag, part, entry, N_STEPS, batch, n, RING, m, lo, p90, reps))
        med[(tag, part, n, batch)] = m

    for n in LEARNERS:
        for batch in BATCHES:
            nl = [DeviceLearner(Models.PERDQN(), dev, ring=r, td_priority=True) for r in rings[:n]]
            wl = [DeviceLearner(Models.PERDQN(), dev, ring=r, td_priority=True, td_batch=batch) for r in rings[:n]]

            def once(e):   # the wide pieces and the narrow pair alternate, repetition by repetition
                mark = (lambda i: e[i].record()) if e else (lambda i: None)
                for l in wl:
                    l.seen.zero_()   # (outside the clock: the stamp's window is the whole ring)
                mark(0)
                dw.stamp_td(wl)
                mark(1)
                slots = dw.draw_td(wl, N_STEPS)
                mark(2)
                dw.draw_td_rank(wl, N_STEPS)
                mark(3)
                dw.learn(wl, N_STEPS, slots=slots)
                mark(4)
                narrow = dw.draw_td(nl, N_STEPS)
                mark(5)
                dw.learn(nl, N_STEPS, slots=narrow)
                mark(6)
            for _ in range(WARM):
                once(None)
            torch.cuda.synchronize()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(7)] for _ in range(reps)]
            for e in ev:
                once(e)
            torch.cuda.synchronize()
            dw.check_error_flag()
            assert all(l.state.cpu().tolist() == [N_STEPS * (WARM + reps), WARM + reps] for l in nl + wl)
            us = lambda a, b: [e[a].elapsed_time(e[b]) * 1e3 for e in ev]  # noqa: E731
            line("tdwide", "stamp", "rl_learn_td_stamp (whole ring)", batch, n, us(0, 1))
            line("tdwide", "draw", "rl_learn_td_wide_draw", batch, n, us(1, 2))
            line("tdwide", "rank", "rl_learn_td_wide_draw_rank", batch, n, us(2, 3))
            line("tdwide", "learn", "rl_learn_td_wide", batch, n, us(3, 4))
            line("td", "draw", "rl_learn_td_draw", 64, n, us(4, 5))
            line("td", "learn", "rl_learn_td", 64, n, us(5, 6))
            med[("td", "draw", n, batch)], med[("td", "learn", n, batch)] = med[("td", "draw", n, 64)], med[("td", "learn", n, 64)]
            d, r, p = med[("tdwide", "draw", n, batch)], med[("tdwide", "rank", n, batch)], med[("tdwide", "learn", n, batch)]
            yard = (med[("td", "draw", n, batch)] + med[("td", "learn", n, batch)]) / (N_STEPS * 64)
            say("row    %d learner(s), batch %d | race draw + update %.2f us = %.4f us per sampled row and learner, rank draw + update %.2f us = %.4f "
                "(rl_learn_td pair in the same loop: %.4f); update alone %.4f us per row (rl_learn_td: %.4f)"
                % (n, batch, d + p, (d + p) / (N_STEPS * batch * n), r + p, (r + p) / (N_STEPS * batch * n), yard / n, p / (N_STEPS * batch * n),
                   med[("td", "learn", n, batch)] / (N_STEPS * 64 * n)))
    return med


def judge(med, say):
    verdict = lambda ok: "CONFIRMED" if ok else "REFUTED"  # noqa: E731
    one, yard = med[("tdwide", "learn", 1, 64)], med[("td", "learn", 1, 64)]
    say("E1     one tile, one learner: rl_learn_td_wide %.1f us against rl_learn_td %.1f us in the same loop = %.2f x (expected within 25 %%): %s"
        % (one, yard, one / yard, verdict(0.75 <= one / yard <= 1.25)))
    for n in LEARNERS:
        t = [med[("tdwide", "learn", n, b)] for b in BATCHES]
        say("E2     %d learner(s): update at batch %s = %s us; batch 2048 / batch 64 = %.2f x (expected below 1.40 x while learners x tiles <= 256): %s"
            % (n, "/".join(map(str, BATCHES)), " / ".join("%.1f" % x for x in t), t[-1] / t[0], verdict(t[-1] / t[0] < 1.4)))
        r = [med[("tdwide", "rank", n, b)] for b in BATCHES]
        say("E3     %d learner(s): rank draw at batch %s = %s us; batch 2048 / batch 64 = %.2f x (expected below 1.15 x): %s"
            % (n, "/".join(map(str, BATCHES)), " / ".join("%.1f" % x for x in r), r[-1] / r[0], verdict(r[-1] / r[0] < 1.15)))
        d = [med[("tdwide", "draw", n, b)] for b in BATCHES]
        say("E4     %d learner(s): race draw at batch %s = %s us; batch 2048 / batch 64 = %.2f x%s; at 2048 the rank draw costs %.2f x the race draw%s"
            % (n, "/".join(map(str, BATCHES)), " / ".join("%.1f" % x for x in d), d[-1] / d[0],
               " (expected 1.3 x .. 4 x): %s" % verdict(1.3 <= d[-1] / d[0] <= 4) if n == 1 else "", r[-1] / d[-1],
               " (expected below 1): %s" % verdict(r[-1] < d[-1]) if n == 1 else ""))
    s1 = sorted(med[("tdwide", "stamp", 1, b)] for b in BATCHES)[len(BATCHES) // 2]
    s8 = sorted(med[("tdwide", "stamp", 8, b)] for b in BATCHES)[len(BATCHES) // 2]
    say("E5     the stamp of a whole ring of %d rows: one learner %.1f us (expected 50 .. 200 us): %s; eight learners %.1f us = %.1f x (expected about "
        "5 x, 3 .. 8): %s" % (RING, s1, verdict(50 <= s1 <= 200), s8, s8 / s1, verdict(3 <= s8 / s1 <= 8)))


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
            fh.write("# tools/learn_td_wide_time.py on ONE MI355X, one process: device events around one stamp of a whole ring (2 launches), one race draw\n"
                     "# (2 launches), one stratified rank draw (8 launches) and one learning call (rl_learn_td: 1 launch; rl_learn_td_wide: 6 launches; the\n"
                     "# event pairs include their host-side issue gaps), ONE step per call, 20 warm-up + >= 200 repetitions per figure, full rings of\n"
                     "# 20,000 rows.  The wide pieces and the rl_learn_td pair alternate in the same loop.  Expected BEFORE measuring (the tool's\n"
                     "# docstring, DESIGN.md 5.32): E1 the one-tile call within 25 % of rl_learn_td; E2 the update flat (< 1.40 x) while learners x tiles\n"
                     "# <= 256; E3 the rank draw flat in the batch (< 1.15 x); E4 the race draw 1.3 x .. 4 x from batch 64 to 2048, dearer than the rank\n"
                     "# draw at 2048; E5 the whole-ring stamp 50 .. 200 us for one learner, about 5 x for eight.\n"
                     "# NOT measured: a trainer() run with learn_batch={\"PERDQN\": B}, hardware counters, several GPUs.\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
