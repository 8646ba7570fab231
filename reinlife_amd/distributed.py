"""Replica sharding across the GPUs of a node: worlds are independent, so each rank owns a contiguous
block of global replica ids and the only collective of a job is ONE all-gather of the metric counters (a row per rank).
Training on several ranks (learn_ranks="average", this build's own -- the reference has no multi-process training) adds the learners'
collectives, counted apart: one all-gather of the exported learner rows per learning episode (gather_learner_rows), and at set-up one
signature gather (check_learner_signature) and one broadcast of rank 0's parameters (broadcast_from_rank0)."""
import torch

collectives_executed = 0   # collectives this module has issued in this process (bench.py reports it; tests assert it)
learn_collectives_executed = 0   # the learners' collectives (gather_learner_rows, broadcast_from_rank0, check_learner_signature), apart


def shard(n_worlds_total, rank, world_size):
    """(first global replica id, number of replicas) of this rank: contiguous blocks, remainder to the low ranks."""
    base, rem = divmod(n_worlds_total, world_size)
    count = base + (1 if rank < rem else 0)
    first = rank * base + min(rank, rem)
    return first, count


def backend_of(dist):
    """Name of the process group's backend ("nccl" = RCCL on ROCm, "gloo", ...); "" for a stand-in without get_backend."""
    try:
        return str(dist.get_backend())
    except Exception:  # noqa: BLE001
        return ""


def gather_rows(row, dist):
    """ONE all-gather of a flat float64 tensor per rank -> [world_size, row.numel()], identical on every rank.  Under a CPU-only
    backend (gloo) with device tensors the few hundred bytes hop through the host (the 2-rank dry runs that share one GPU:
    tests/test_hip_round5.py; the result then stays on the host); under nccl (= RCCL) the gather runs on the device over xGMI."""
    row = row.reshape(-1).contiguous()
    if row.is_cuda and backend_of(dist) == "gloo":
        row = row.cpu()
    flat = torch.empty(dist.get_world_size() * row.numel(), dtype=row.dtype, device=row.device)
    dist.all_gather_into_tensor(flat, row)   # (flat output: the shape every backend accepts)
    return flat.view(dist.get_world_size(), row.numel())


def reduce_counters(counters, elapsed_s, dist=None):
    """counters: 1-D float64 tensor of additive metrics; returns (summed counters, max elapsed, per-rank table) over all ranks.

    ONE collective: every rank contributes a row [counters..., elapsed] to an all-gather of O(100 B) per rank (pure latency
    over xGMI, never per step); sums, the maximum of the elapsed times and the per-rank table (straggler diagnosis: bench.py
    prints min / max of the per-rank rates) all come out of it.  Runs whenever a process group exists -- also at world size 1,
    where RCCL executes the same call."""
    row = torch.cat([counters.to(torch.float64), torch.tensor([elapsed_s], dtype=torch.float64, device=counters.device)])
    if dist is not None and dist.is_initialized():
        global collectives_executed
        collectives_executed += 1
        table = gather_rows(row, dist)
    else:
        table = row[None, :].clone()
    return table[:, :-1].sum(0), float(table[:, -1].max().item()), table.cpu()


def gather_learner_rows(row, dist):
    """ONE all-gather of a rank's exported learner row (DeviceWorlds.export_learners: flat float32) -> [world_size, row.numel()], the
    same table on every rank, in rank order: what rl_learn_merge takes.  Like gather_rows, a device row hops through the host under gloo
    (the result is then a host tensor) and stays on the device under nccl (= RCCL, over xGMI)."""
    global learn_collectives_executed
    learn_collectives_executed += 1
    return gather_rows(row, dist)


def broadcast_from_rank0(tensor, dist):
    """ONE broadcast: `tensor` (contiguous) is overwritten in place with rank 0's values and returned.  A device tensor hops through
    the host under gloo and stays on the device under nccl."""
    global learn_collectives_executed
    learn_collectives_executed += 1
    if tensor.is_cuda and backend_of(dist) == "gloo":
        host = tensor.cpu()
        dist.broadcast(host, 0)
        tensor.copy_(host)
    else:
        dist.broadcast(tensor, 0)
    return tensor


SIGNATURE_LEN = 128   # numbers of a learner signature at most: every rank gathers a row of this length whatever it holds


def check_learner_signature(signature, dist, device=None):
    """Set-up of learn_ranks="average": every rank must hold the same learners on the same schedule, or the per-episode all-gather of
    their rows would hang or average unlike things.  `signature`: a flat list of at most SIGNATURE_LEN numbers (Environment: per learner
    its brain index, kind, entry point, exploration and soft_update_freq -- a wide DQN or wide D3QN learner also its batch --, then learn_every, the learn_steps per kind and rollout_steps).
    `device`: where the row is made -- the worlds' device under nccl (= RCCL), whose process group serves device tensors only, as the
    Tracker makes its layout row; under gloo gather_rows takes a device row through the host.  ONE all-gather of a
    fixed-length row [length, numbers..., zero padding]; a mismatch raises the same ValueError on EVERY rank, with the table in the
    message, before any rank can wait in a later collective -- as Tracker refuses unequal shards."""
    sig = [float(x) for x in signature]
    if len(sig) > SIGNATURE_LEN:
        raise ValueError("a learner signature holds at most %d numbers (got %d)" % (SIGNATURE_LEN, len(sig)))
    global learn_collectives_executed
    learn_collectives_executed += 1
    mine = torch.tensor([float(len(sig))] + sig + [0.0] * (SIGNATURE_LEN - len(sig)), dtype=torch.float64, device=device)
    table = gather_rows(mine, dist).cpu()
    if not bool((table == table[0]).all()):
        raise ValueError("learn_ranks='average' needs the same learners on the same schedule on every rank (kinds, entry points, exploration, soft_update_freq, "
                         "learn_every, learn_steps, rollout_steps); signatures per rank: %s"
                         % [[int(v) if v == int(v) else v for v in r[1:1 + int(r[0])].tolist()] for r in table])
    return table
