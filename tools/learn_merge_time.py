"""What the learners' merge over ranks costs on ONE MI355X (rl_learn_export + rl_learn_merge, reinlife_amd/csrc/rl_learn_merge.hip), next to
the same work made of eager torch ops and the host packer on the same GPU:

  merge    device-event time of ONE rl_learn_export (one launch) followed by ONE rl_learn_merge (two launches: mean, pack) for the
           learners of a call against a SYNTHETIC gather of n_ranks rows that already sits on the device -- median, min and p90 over
           >= 200 repetitions after 20 warm-up pairs; 1, 2 and 8 DQN learners and one PPO learner at n_ranks 1, 2 and 8
  torch    per learner: the rows' mean in double on the device (sum over the ranks, divide, to float32), the three copies into the
           learner's buffers, the parameters to the host, rl_policy_pack_weights there, and the packed weights' upload; device events
           around the host-issued ops

NOT measured here: the all-gather itself.  Between real GPUs it moves n_ranks x 4 x (3 n_params + 2) bytes per learner over xGMI (RCCL);
this tool runs on one GPU and never issues a collective.

    python tools/learn_merge_time.py [--out profiles/learn_merge.txt] [--reps 200]

No threshold is set: the figures are recorded.  Every configuration runs in a child process of its own under its own time limit, and the
first step that fails ends the run."""
import argparse
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_time import _report  # noqa: E402

STEPS = [("DQN", "1"), ("DQN", "2"), ("DQN", "8"), ("PPO", "1")]
RANKS = (1, 2, 8)
STEP_SECONDS = 150


def step(method, n, reps):
    import numpy as np
    import torch
    from reinlife_amd import Models, _lib
    from reinlife_amd.learn import DeviceLearner
    from reinlife_amd.worlds import DeviceWorlds
    dev = "cuda:0"
    lib = _lib.lib()
    dw = DeviceWorlds(n_worlds=1, seed=1, device=dev)
    torch.manual_seed(1)
    rollout = {"rollout": True} if method == "PPO" else {}
    ls = [DeviceLearner(getattr(Models, method)(), dev, **rollout) for _ in range(n)]
    total = sum(l.merge_floats for l in ls)
    row = torch.empty(total, dtype=torch.float32, device=dev)
    for n_ranks in RANKS:
        dw.export_learners(ls, out=row)
        rows = row.repeat(n_ranks, 1).contiguous()      # every rank at the same step count: all take part
        rows[:, : ls[0].n_params] += 1e-3 * torch.arange(n_ranks, device=dev, dtype=torch.float32)[:, None]
        for _ in range(20):
            dw.export_learners(ls, out=row); dw.merge_learners(ls, rows, n_ranks)
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
        for e in ev:
            e[0].record(); dw.export_learners(ls, out=row); e[1].record(); dw.merge_learners(ls, rows, n_ranks); e[2].record()
        torch.cuda.synchronize()
        dw.check_error_flag()
        what = "%d %s learner(s), n_ranks %d, %d floats per row" % (n, method, n_ranks, total)
        _report("merge export rl_learn_export, %s" % what, [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)
        _report("merge merge  rl_learn_merge (mean + pack), %s" % what, [e[1].elapsed_time(e[2]) * 1e3 for e in ev], reps)
        _report("merge both   rl_learn_export + rl_learn_merge, %s" % what, [e[0].elapsed_time(e[2]) * 1e3 for e in ev], reps)

        def eager():
            off = 0
            for l in ls:
                k = l.n_params
                mean = (rows[:, off:off + 3 * k].double().sum(0) / n_ranks).float()
                l.params.copy_(mean[:k]); l.adam_m.copy_(mean[k:2 * k]); l.adam_v.copy_(mean[2 * k:])
                host = l.params.cpu().numpy()
                packed = np.empty(l.packed.numel(), np.float32)
                _lib.check(lib.rl_policy_pack_weights(l.kind, host.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)), "rl_policy_pack_weights")
                l.packed.copy_(torch.from_numpy(packed))
                off += l.merge_floats
        for _ in range(5):
            eager()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(reps)]
        for e in ev:
            e[0].record(); eager(); e[1].record()
        torch.cuda.synchronize()
        _report("torch        eager mean in double + host pack + upload, %s (device events around the host-issued ops)" % what,
                [e[0].elapsed_time(e[1]) * 1e3 for e in ev], reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the figures to this file")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--step", nargs="+", default=None, help=argparse.SUPPRESS)   # (a child process: one configuration)
    args = ap.parse_args()
    if args.step:
        step(args.step[0], int(args.step[1]), max(args.reps, 200))
        return 0
    lines = []
    for st in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--step"] + list(st)
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_SECONDS, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("learn_merge_time: step %s ran into its %d s limit; stopping" % (" ".join(st), STEP_SECONDS), file=sys.stderr)
            return 1
        if r.returncode != 0:
            print("learn_merge_time: step %s failed (%d); stopping\n%s" % (" ".join(st), r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        got = [ln for ln in r.stdout.splitlines() if ln.startswith(("merge", "torch"))]
        print("\n".join(got), flush=True)
        lines += got
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/learn_merge_time.py on ONE MI355X: device events around rl_learn_export (one launch) and rl_learn_merge (two launches) against a\n"
                     "# synthetic gather that already sits on the device, 20 warm-up + >= 200 repetitions per figure; the event pairs include the launches'\n"
                     "# host-side issue gaps.  NOT measured: the all-gather of the rows over xGMI between real GPUs (no collective is issued here).\n"
                     + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
