"""One rank of the two-rank dry run of tests/test_hip_learn_merge.py: python learn_merge_rank.py RANK WORLD_SIZE PORT OUT.npz.  Every rank
sits on cuda:0 and the collectives hop through the host and gloo -- this shows the structure of learn_ranks="average" (who talks when,
and that the ranks end with the same bits), not RCCL speed."""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_EPISODES, N_WORLDS = 40, 2


def brains_of(rank):
    import torch
    from reinlife_amd import Models
    torch.manual_seed(1000 + rank)          # another generator state per rank: the initial weights differ
    return [Models.DQN(max_epi=N_EPISODES), Models.D3QN(exploration=10, soft_update_freq=40)]


def run(brains, **kw):
    from reinlife_amd import trainer
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return trainer(brains, n_episodes=N_EPISODES, n_worlds=N_WORLDS, synthetic_agents=100, refill_below=70, update_interval=20, save=False,
                       print_results=False, device="cuda:0", seed=5, **kw)


def main():
    rank, world_size, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import torch
    import torch.distributed as dist
    from reinlife_amd import distributed as rd
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    brains = brains_of(rank)
    res = {"init%d" % k: b.state_dict_flat().copy() for k, b in enumerate(brains)}
    env = run(brains, learn="device", learn_kinds=("DQN", "D3QN"), learn_ranks="average")
    torch.cuda.synchronize()
    for k, l in sorted(env.learners.items()):
        for name in ("params", "adam_m", "adam_v", "target", "packed", "state"):
            res["%s%d" % (name, k)] = getattr(l, name).cpu().numpy()
        res["module%d" % k] = brains[k].state_dict_flat()
    res["learn_collectives"] = np.int64(rd.learn_collectives_executed)
    res["learn_now_calls"] = np.int64(env.learn_now_calls)
    res["tracker_collectives"] = np.int64(env.tracker.collectives_executed)
    res["note"] = np.array(env._weights_note())
    plain = run(brains_of(rank))            # the same run without learning: what the Tracker's collectives are on their own
    res["tracker_collectives_plain"] = np.int64(plain.tracker.collectives_executed)
    res["learn_collectives_end"] = np.int64(rd.learn_collectives_executed)
    np.savez(out, **res)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
