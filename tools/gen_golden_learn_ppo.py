"""The PPO learning fixture from the real reference (build container only; data in, data out -- no reference source is copied).

Builds the reference's PPOAgent (ReinLife/Models/PPO.py), loads PPO_weights of tests/golden/models.npz into its module (so the initial
parameters are not stored again) and feeds the reference's OWN learn() (PPO.py:136-162) three rollouts of 32, 17 and 1 rows through
put_data(), exactly as PPOAgent.learn (PPO.py:71-77) fills the list: (state, action, reward / 100.0, state_prime, prob_a, done).  The rows
are slots of learn_d3qn.npz's 96-row ring; prob_a = pi_init(s)[a] times a recorded factor in [0.8, 1.25], capped at 1, so that rows fall
on every side of the clip.  The ring's rewards are used as they are (reward_scale 1): +-400 / 100 gives |v - td| > 1 and the small
rewards |v - td| < 1, both smooth-L1 branches.

While learn() runs, optimizer.step is wrapped to snapshot the parameters in front of every epoch, and the module's `torch.tensor` is
watched for the advantage list (the one call with dtype=torch.float and a list of one-element lists of numpy scalars): the reference's own
advantages.

  tests/golden/learn_ppo.npz
    slots           int32 [3][32] ring slots of the three rollouts, -1 beyond a rollout's rows; rows int64 [3] = 32, 17, 1
    prob, factor    float32 [96] per ring row: the acting probability handed to learn(), and the factor it was made with
    reward_scale    what ring_reward of learn_d3qn.npz is multiplied by (1.0)
    final           flat float32 parameters after the three learn() calls
    delta, adv      float32 [3][3][32]: per rollout and epoch, the float32 delta made from that epoch's parameters (zero beyond the rows)
                    and the advantages the reference made of it
    grad_max        float64 [3][3][8]: per rollout, epoch and parameter tensor the largest gradient magnitude of the float64 run
    ref_grad_err    torch's own float32 error: max over the tensors of max |g32 - g64| / max |g64| in epoch 1 of rollout 1
    ref_out_spread  max |out(final32) - out(final64)| / effect over the 96 ring states, out = the 8 probabilities and the value in float64,
                    final64 = the same nine epochs in float64 (advantages in the float32 form, from float64 deltas)
    effect          max |out(final32) - out(init)|
    lr, gamma, lmbda, eps_clip, k_epoch   the hyperparameters the reference used

The float64 run is asserted to stay clear of branch flips: every rollout of 17 or more rows has a row in each of (adv > 0, ratio > 1 + eps),
(adv > 0, ratio < 1 - eps), (adv < 0, ratio > 1 + eps), (adv < 0, inside the clip) and rows on both sides of |v - td| = 1; no row of any
epoch has its ratio within 1e-4 of a clip bound or |v - td| within 1e-4 of 1.

    python tools/gen_golden_learn_ppo.py
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_harness as rh  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "learn_ppo.npz")
D3QN = os.path.join(ROOT, "tests", "golden", "learn_d3qn.npz")
MODELS = os.path.join(ROOT, "tests", "golden", "models.npz")
SEED, ROWS, RING = 35, (32, 17, 1), 96
FACTORS = np.array([0.8, 0.84, 0.88, 0.97, 1.0, 1.03, 1.16, 1.2, 1.25], np.float32)
REWARD_SCALE = 1.0


def flat(sd):
    return np.concatenate([v.detach().numpy().reshape(-1) for v in sd.values()])


def gae32(delta, gl):
    adv, out = np.float32(0.0), np.zeros(len(delta), np.float32)
    for t in range(len(delta) - 1, -1, -1):
        adv = np.float32(np.float32(np.float32(gl) * adv) + np.float32(delta[t]))
        out[t] = adv
    return out


def main():
    ref = rh.load_reference()
    torch = ref.torch
    torch.set_num_threads(1)
    import ReinLife.Models.PPO  # noqa: F401  (the module; ReinLife.Models.PPO the attribute may be the class)
    mod = sys.modules["ReinLife.Models.PPO"]
    with np.load(D3QN) as z:
        ring = {k: z[k] for k in z.files if k.startswith("ring_")}
    ring["ring_reward"] = (ring["ring_reward"] * np.float32(REWARD_SCALE)).astype(np.float32)
    with np.load(MODELS) as z:
        init = z["PPO_weights"].astype(np.float32)
    rng = np.random.RandomState(SEED)
    slots = np.full((len(ROWS), max(ROWS)), -1, np.int32)
    for i, n in enumerate(ROWS):
        slots[i, :n] = rng.choice(RING, size=n, replace=False)
    slots[0, 1] = slots[0, 0]   # a row that counts twice

    brain = mod.PPOAgent()
    model = brain.model
    off = 0
    with torch.no_grad():
        for t in model.state_dict().values():
            t.copy_(torch.from_numpy(init[off:off + t.numel()].reshape(tuple(t.shape))))
            off += t.numel()
    assert off == init.size and flat(model.state_dict()).astype(np.float32).tobytes() == init.tobytes()
    lr, gamma, lmbda, eps_clip, k_epoch = model.learning_rate, model.gamma, model.lmbda, model.eps_clip, model.k_epoch
    gl = gamma * lmbda

    factor = rng.choice(FACTORS, size=RING).astype(np.float32)
    with torch.no_grad():
        pi_init = model.pi(torch.tensor(ring["ring_state"]), softmax_dim=1).numpy()
    prob = np.minimum(pi_init[np.arange(RING), ring["ring_action"].astype(np.int64)] * factor, np.float32(1.0)).astype(np.float32)

    def batch(i, dtype):
        idx = slots[i, :ROWS[i]].astype(np.int64)
        r = np.array([float(x) / 100.0 for x in ring["ring_reward"][idx]], np.float64).astype(np.float32)
        col = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype).unsqueeze(1)  # noqa: E731
        return (torch.tensor(ring["ring_state"][idx], dtype=dtype), torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1), col(r),
                torch.tensor(ring["ring_state_prime"][idx], dtype=dtype), col(1.0 - ring["ring_done"][idx]), col(prob[idx]))

    def loss_of(net, i, dtype):   # PPO.py:140-158 with torch operations on a copy of the reference's module
        s, a, r, sp, mask, pa = batch(i, dtype)
        td = r + gamma * net.v(sp) * mask
        v = net.v(s)
        delta = (td - v).detach().numpy()[:, 0]
        adv = torch.tensor(gae32(delta.astype(np.float32), gl).astype(np.float64), dtype=dtype).unsqueeze(1)
        ratio = torch.exp(torch.log(net.pi(s, softmax_dim=1).gather(1, a)) - torch.log(pa))
        surr1, surr2 = ratio * adv, torch.clamp(ratio, 1 - eps_clip, 1 + eps_clip) * adv
        loss = (-torch.min(surr1, surr2) + torch.nn.functional.smooth_l1_loss(v, td.detach())).mean()
        return loss, dict(delta=delta, adv=adv.detach().numpy()[:, 0], ratio=ratio.detach().numpy()[:, 0], d=(v - td).detach().numpy()[:, 0])

    # ---- the same nine epochs in float64 (a copy of the reference's module), with the conditions that keep it clear of branch flips ----
    m64 = copy.deepcopy(model).double()
    m64.optimizer = None
    opt64 = torch.optim.Adam(m64.parameters(), lr=lr)
    grad_max = np.zeros((len(ROWS), k_epoch, 8))
    g64_first = None
    for i, n in enumerate(ROWS):
        for ep in range(k_epoch):
            loss, mid = loss_of(m64, i, torch.float64)
            opt64.zero_grad()
            loss.backward()
            gs = [p.grad.numpy().copy() for p in m64.parameters()]
            grad_max[i, ep] = [np.abs(x).max() for x in gs]
            if g64_first is None:
                g64_first = gs
            ratio, adv, d = mid["ratio"], mid["adv"], mid["d"]
            assert np.abs(ratio - (1 + eps_clip)).min() > 1e-4 and np.abs(ratio - (1 - eps_clip)).min() > 1e-4, "a ratio within 1e-4 of a clip bound"
            assert np.abs(np.abs(d) - 1).min() > 1e-4, "|v - td| within 1e-4 of 1"
            if n >= 17 and ep == 0:
                inside = (ratio >= 1 - eps_clip) & (ratio <= 1 + eps_clip)
                cases = [((adv > 0) & (ratio > 1 + eps_clip)).sum(), ((adv > 0) & (ratio < 1 - eps_clip)).sum(),
                         ((adv < 0) & (ratio > 1 + eps_clip)).sum(), ((adv < 0) & inside).sum()]
                print("rollout %d: rows per clip case %s; |v - td| < 1: %d, > 1: %d" % (i, cases, (np.abs(d) < 1).sum(), (np.abs(d) > 1).sum()))
                assert min(cases) >= 1, "a clip case without a row"
                assert (np.abs(d) < 1).any() and (np.abs(d) > 1).any(), "one smooth-L1 branch without a row"
            opt64.step()
    final64 = flat(m64.state_dict())

    # ---- torch's own float32 gradient error, epoch 1 of rollout 1, before anything changes ----
    loss32, _ = loss_of(model, 0, torch.float32)
    g32 = torch.autograd.grad(loss32, list(model.parameters()))
    ref_grad_err = max(float(np.abs(a.numpy() - b).max() / np.abs(b).max()) for a, b in zip(g32, g64_first))

    # ---- the reference's own learn(), watched ----
    snaps, advs = [], []
    real_step = model.optimizer.step

    def step(*a, **kw):
        snaps.append(copy.deepcopy(model.state_dict()))   # this epoch's pre-update parameters
        return real_step(*a, **kw)
    model.optimizer.step = step

    class TorchProxy:
        def __getattr__(self, name):
            return getattr(torch, name)

        def tensor(self, data, *a, **kw):
            if kw.get("dtype") is torch.float and isinstance(data, list) and data and isinstance(data[0], list) and len(data[0]) == 1 and isinstance(data[0][0], np.floating) and not a:
                advs.append(np.array([x[0] for x in data]))
            return torch.tensor(data, *a, **kw)
    real_torch = mod.torch
    mod.torch = TorchProxy()
    try:
        for i, n in enumerate(ROWS):
            for slot in slots[i, :n]:
                brain.put_data((ring["ring_state"][slot], int(ring["ring_action"][slot]), float(ring["ring_reward"][slot]) / 100.0,
                                ring["ring_state_prime"][slot], float(prob[slot]), bool(ring["ring_done"][slot])))
            brain.train()
    finally:
        mod.torch = real_torch
        model.optimizer.step = real_step
    assert len(snaps) == len(ROWS) * k_epoch and len(advs) == len(snaps), (len(snaps), len(advs))
    final = flat(model.state_dict()).astype(np.float32)

    delta_rec = np.zeros((len(ROWS), k_epoch, max(ROWS)), np.float32)
    adv_rec = np.zeros_like(delta_rec)
    for i, n in enumerate(ROWS):
        for ep in range(k_epoch):
            net = copy.deepcopy(model)
            net.load_state_dict(snaps[i * k_epoch + ep])
            s, a, r, sp, mask, pa = batch(i, torch.float32)
            with torch.no_grad():
                delta = ((r + gamma * net.v(sp) * mask) - net.v(s)).numpy()[:, 0]
            a_ref = advs[i * k_epoch + ep]
            assert a_ref.dtype == np.float32, "the reference's advantages are %s: not numpy 2's float32 recursion" % a_ref.dtype
            assert gae32(delta, gl).tobytes() == a_ref.tobytes(), "the float32 recursion does not give the reference's advantages"
            delta_rec[i, ep, :n], adv_rec[i, ep, :n] = delta, a_ref

    def out_of(flat_params):
        net = copy.deepcopy(m64)
        o = 0
        with torch.no_grad():
            for t in net.state_dict().values():
                t.copy_(torch.from_numpy(np.asarray(flat_params[o:o + t.numel()], np.float64).reshape(tuple(t.shape))))
                o += t.numel()
            x = torch.tensor(ring["ring_state"], dtype=torch.float64)
            return torch.cat([net.pi(x, softmax_dim=1), net.v(x)], dim=1).numpy()

    effect = float(np.abs(out_of(final) - out_of(init)).max())
    out = dict(slots=slots, rows=np.array(ROWS, np.int64), prob=prob, factor=factor, reward_scale=np.float32(REWARD_SCALE), final=final,
               delta=delta_rec, adv=adv_rec, grad_max=grad_max, ref_grad_err=np.float64(ref_grad_err), effect=np.float64(effect),
               ref_out_spread=np.float64(np.abs(out_of(final) - out_of(final64)).max() / effect),
               lr=np.float64(lr), gamma=np.float64(gamma), lmbda=np.float64(lmbda), eps_clip=np.float64(eps_clip), k_epoch=np.int64(k_epoch))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.0f KB): ref_grad_err %.3g ref_out_spread %.3g effect %.3g max|final - final64| %.3g" % (
        OUT, os.path.getsize(OUT) / 1024, ref_grad_err, out["ref_out_spread"], effect, np.abs(final - final64).max()))


if __name__ == "__main__":
    main()
