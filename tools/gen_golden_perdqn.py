"""PERDQN fixtures from the real reference (build container only; data in, data out -- no reference source is copied).

Runs the reference's own PERDQNAgent (ReinLife/Models/PERDQN.py) on CPU and records

  tests/golden/perdqn.npz
    ckpt_<name>_weights / _out   the three shipped PERDQN checkpoints as flat float32 state dicts (registration order) and the reference
                                 module's Q values on the 96 observation rows of tests/golden/pretrained.npz (meta: keys, shapes, files)
    init_<s>_train / init_<s>_greedy   the flat state dict of PERDQN() / PERDQN(training=False) after torch.manual_seed(s)
    act_<mode>_q / _actions      get_action(state) of a training=True ("explore") and a training=False ("greedy") brain over recorded
                                 rows, after random.seed / np.random.seed(ACT_SEED): the Q values the greedy brain saw and every action
  tests/golden/e2e_perdqn_mixed.npz
    the whole trainer loop body without learn() (Helpers/trainer.py:85-99) from seeds alone, in oracle/gen_golden_e2e.py's format:
    brains [PERDQN greedy (fresh weights), PERDQN exploring, PERD3QN exploring].  Every greedy PERDQN row of the run must have a top-2
    Q gap of at least 1e-4 * max(1, max|q|) (a near-tie of the reference alone must not decide the fixture); otherwise the next seed.

    python tools/gen_golden_perdqn.py
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as gg  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "perdqn.npz")
OUT_E2E = os.path.join(ROOT, "tests", "golden", "e2e_perdqn_mixed.npz")
CKPTS = {"all_gene_2": "pretrained/All/PERDQN/brain_gene_2.pt", "perdqn_gene_0": "pretrained/PERDQN/PERDQN/brain_gene_0.pt",
         "perdqn_gene_1": "pretrained/PERDQN/PERDQN/brain_gene_1.pt"}
INIT_SEEDS = (0, 1, 7)
ACT_SEED, ACT_CALLS = 11, 400
N_ROWS = 96
PERDQN_KIND, PERD3QN_KIND = 4, 2
E2E_SEEDS = range(31, 60)
E2E_TICKS, E2E_W, E2E_H, E2E_MAX = 150, 30, 30, 100


def flat(sd):
    return np.concatenate([v.detach().numpy().astype(np.float32).reshape(-1) for v in sd.values()])


def gap_ok(q):
    s = np.sort(q)
    return s[-1] - s[-2] >= 1e-4 * max(1.0, float(np.abs(q).max()))


def record_e2e(ref, PERDQN, seed):
    torch = ref.torch
    torch.manual_seed(1000 + seed)
    greedy = PERDQN(training=False)                  # fresh weights (xavier): not a checkpoint
    explore = PERDQN()                               # epsilon 1.0: every action from random.randrange
    perd3qn = ref.PERD3QN(training=True)
    sd3 = gg.model_weights("PERD3QN", 300 + seed)
    perd3qn.eval_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd3.items()})
    perd3qn.target_net.load_state_dict({k: torch.from_numpy(v) for k, v in sd3.items()})
    brains = [greedy, explore, perd3qn]
    flats = [flat(greedy.model.state_dict()), flat(explore.model.state_dict()), np.concatenate([sd3[k].reshape(-1) for k in sd3]).astype(np.float32)]
    rh.seed_all(seed)   # after construction: the constructors consume torch's generator
    env = rh.make_env(brains=brains, width=E2E_W, height=E2E_H, max_agents=E2E_MAX, static_families=True)
    env.reset()
    cap = orc.slot_cap_for(E2E_MAX, E2E_W * E2E_H)
    d = {"cfg": np.array([E2E_W, E2E_H, E2E_MAX, len(brains), 1, 0, 1, cap, E2E_TICKS], np.int64), "seed": np.int64(seed),
         "kinds": np.array([PERDQN_KIND, PERDQN_KIND, PERD3QN_KIND], np.int32), "training": np.array([0, 1, 1], np.int32)}
    for idx, f in enumerate(flats):
        d["weights_%d" % idx] = f
    snaps = {"step": [], "upd": []}
    actions, rewards = [], []
    greedy_rows = 0
    for t in range(E2E_TICKS):
        for agent in env.agents:
            b = agent.brain
            if b.method == "PERDQN" and b.epsilon == 0:   # (a forward pass draws nothing)
                with torch.no_grad():
                    q = b.model(torch.from_numpy(np.asarray(agent.state, np.float32).reshape(1, -1)))[0].numpy()
                if not gap_ok(q):
                    return None
                greedy_rows += 1
            agent.get_action(t)   # (entities.py:215-222: PERDQN is asked without n_epi)
        actions.append(np.array([int(a.action) for a in env.agents], np.int8))
        env.step()
        s, ags = rh.snapshot_world(env)
        rewards.append(np.array([float(a.reward) for a in ags], np.float32))
        snaps["step"].append(s)
        env.update_env(t)
        snaps["upd"].append(rh.snapshot_world(env)[0])
    maxn = max(1, max(len(s["i"]) for ph in snaps.values() for s in ph), max(len(a) for a in actions))
    d["n0"] = np.array([len(a) for a in actions], np.int32)
    d["actions"] = np.stack([gg._pad(a, maxn) for a in actions])
    d["step_reward"] = np.stack([gg._pad(r, maxn) for r in rewards])
    for ph, lst in snaps.items():
        d[ph + "_n"] = np.array([len(s["i"]) for s in lst], np.int32)
        d[ph + "_cell_type"] = np.stack([s["cell_type"] for s in lst])
        for k in gg.AGENT_KEYS:
            d[ph + "_" + k] = np.stack([gg._pad(s[k], maxn) for s in lst])
        d[ph + "_max_gene"] = np.array([s["max_gene"] for s in lst], np.int32)
        for k in ("best_uid", "best_fit", "best_brain"):
            d[ph + "_" + k] = np.stack([s[k] for s in lst])
    d["greedy_rows"] = np.int64(greedy_rows)
    return d


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    from ReinLife.Models import PERDQN   # (the reference package is on sys.path once load_reference() ran)
    obs = np.load(os.path.join(ROOT, "tests", "golden", "pretrained.npz"))["obs"][:N_ROWS].astype(np.float32)
    out = {"obs": obs}
    meta = {"ckpt": {}, "init_seeds": list(INIT_SEEDS), "act_seed": ACT_SEED}
    for name, rel in CKPTS.items():
        b = PERDQN(load_model=os.path.join(rh.REFERENCE_ROOT, rel), training=False)
        sd = b.model.state_dict()
        with torch.no_grad():
            out["ckpt_%s_out" % name] = b.model(torch.from_numpy(obs)).numpy().astype(np.float32)
        out["ckpt_%s_weights" % name] = flat(sd)
        meta["ckpt"][name] = {"file": rel, "keys": [[k, list(v.shape)] for k, v in sd.items()]}
        print(name, float(np.abs(out["ckpt_%s_out" % name]).max()))
    for s in INIT_SEEDS:
        torch.manual_seed(s)
        out["init_%d_train" % s] = flat(PERDQN().model.state_dict())
        torch.manual_seed(s)
        out["init_%d_greedy" % s] = flat(PERDQN(training=False).model.state_dict())
    # get_action sequences: rows cycle through the 96 observations, the greedy brain carries checkpoint all_gene_2
    rows = np.arange(ACT_CALLS) % N_ROWS
    for mode, training in (("explore", True), ("greedy", False)):
        b = PERDQN(load_model=os.path.join(rh.REFERENCE_ROOT, CKPTS["all_gene_2"]), training=training)
        random.seed(ACT_SEED)
        np.random.seed(ACT_SEED)
        acts = [b.get_action(obs[r]) for r in rows]
        out["act_%s_actions" % mode] = np.array(acts, np.int8)
        out["act_%s_rows" % mode] = rows.astype(np.int32)
    out["act_q"] = out["ckpt_all_gene_2_out"]
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT))
    for seed in E2E_SEEDS:
        d = record_e2e(ref, PERDQN, seed)
        if d is None:
            print("seed %d: a greedy PERDQN row has a top-2 gap below 1e-4 * max(1, max|q|); next seed" % seed)
            continue
        np.savez_compressed(OUT_E2E, **d)
        print("wrote %s (%.0f KB): seed %d, %d agent-steps, %d greedy PERDQN rows, population %d..%d" % (
            OUT_E2E, os.path.getsize(OUT_E2E) / 1024, seed, int(d["n0"].sum()), int(d["greedy_rows"]), d["upd_n"].min(), d["upd_n"].max()))
        return
    raise SystemExit("no seed in %s gave a whole-loop case without near-ties" % (E2E_SEEDS,))


if __name__ == "__main__":
    main()
