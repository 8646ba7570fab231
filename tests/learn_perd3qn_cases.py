"""Shared by tests/test_learn_perd3qn_cpu.py and tests/test_hip_learn_perd3qn.py: the fixture tests/golden/learn_perd3qn.npz (the
reference's own PERD3QNAgent.train() and PrioritizedReplayBuffer, tools/gen_golden_learn_perd3qn.py), a torch restatement of the
priorities train() hands to update_priorities (ReinLife/Models/PERD3QN.py:103-111) in any dtype, and a small host model of the
prioritised memory as the device keeps it: rows stamped after the fact from a `seen` counter, the maximum taken at every update, and
sample()'s p = priority^alpha / sum (PERD3QN.py:143-165, 177-179).  The ring, slots and networks are tests/golden/learn_d3qn.npz's."""
import os

import numpy as np
import torch

import learn_d3qn_cases as dc

ROOT = dc.ROOT
_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(os.path.join(ROOT, "tests", "golden", "learn_perd3qn.npz")) as z:
            _golden = {k: z[k] for k in z.files}
        for v in _golden.values():
            v.setflags(write=False)
    return _golden


def priorities(flat, target_flat, ring, slots, dtype=torch.float64):
    """(|max_a q'_target(s') - q_eval(s)[a]|, q_eval(s)[a], max_a q'_target(s')) of one minibatch, each with its batch-wide advantage
    mean, computed in `dtype` from the given flat parameters; returned as float64 arrays."""
    idx = np.asarray(slots, np.int64)
    net, tgt = dc.net_of(np.asarray(flat, np.float64), dtype), dc.net_of(np.asarray(target_flat, np.float64), dtype)
    with torch.no_grad():
        a = torch.tensor(ring["ring_action"][idx].astype(np.int64)).unsqueeze(1)
        q = net(torch.tensor(ring["ring_state"][idx], dtype=dtype)).gather(1, a).squeeze(1)
        qn = tgt(torch.tensor(ring["ring_state_prime"][idx], dtype=dtype)).max(1)[0]
        return tuple(x.double().numpy() for x in (torch.abs(qn - q), q, qn))


_step_params = None


def step_params():
    """The flat float32 parameters before each of the fixture's three steps: learn_d3qn_cases.torch_steps, recording as it goes."""
    global _step_params
    if _step_params is None:
        g = dc.golden()
        net, tgt = dc.net_of(g["init"], torch.float32), dc.net_of(g["target_init"], torch.float32)
        opt = torch.optim.Adam(net.parameters(), lr=float(g["lr"]))
        out = []
        for s in range(g["slots"].shape[0]):
            out.append(dc.flat_of(net).copy())
            loss = dc.d3qn_loss(net, tgt, g, g["slots"][s], float(g["gamma"]), torch.float32)
            opt.zero_grad()
            loss.backward()
            opt.step()
        _step_params = out
    return _step_params


class HostMemory:
    """The prioritised memory as rl_learn_prioritized_draw / rl_learn_prioritized keep it, on the host: store() only counts; the rows
    appended since the last look are stamped with the maximum after the fact (slots [seen, count) mod capacity, all of them once
    count - seen >= capacity); the maximum is retaken over [0, size) at every update."""

    def __init__(self, capacity, alpha=0.6):
        self.capacity, self.alpha = int(capacity), float(alpha)
        self.priority = np.zeros(self.capacity, np.float32)
        self.prio_max, self.seen, self.count = np.float32(1.0), 0, 0

    @property
    def size(self):
        return min(self.count, self.capacity)

    def store(self, n=1):
        self.count += n

    def stamp(self):
        fresh = self.count - self.seen
        if fresh >= self.capacity:
            self.priority[:] = self.prio_max
        else:
            for c in range(self.seen, self.count):
                self.priority[c % self.capacity] = self.prio_max
        self.seen = self.count
        return self.priority

    def update(self, indices, values):
        self.stamp()
        for i, v in zip(indices, values):
            self.priority[i] = v
        self.prio_max = self.priority[:self.size].max()

    def probs(self):
        w = self.stamp()[:self.size].astype(np.float64) ** self.alpha
        return w / w.sum()


# ---- the weighted draw of rl_learn_prioritized_draw, restated on the host (integer code and rl_philox exactly; logf / powf as numpy's) ----
def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _term(position, bits):
    return _mix64((np.uint64(position + 1) << np.uint64(32)) | np.asarray(bits, np.uint64))


def content_keys(ring, n, age=None):
    """The 64-bit content keys of the first n rows, as learn_row_key sums them; age: the rows' int32 ages (None: age 0)."""
    age = np.zeros(n, np.int32) if age is None else np.ascontiguousarray(np.asarray(age)[:n], np.int32)
    k = np.zeros(n, np.uint64)
    s, sp = np.ascontiguousarray(ring["ring_state"][:n]).view(np.uint32), np.ascontiguousarray(ring["ring_state_prime"][:n]).view(np.uint32)
    with np.errstate(over="ignore"):
        for f in range(153):
            k += _term(f, s[:, f])
            k += _term(153 + f, sp[:, f])
        k += _term(306, ring["ring_action"][:n].astype(np.uint8))
        k += _term(307, np.ascontiguousarray(ring["ring_reward"][:n]).view(np.uint32))
        k += _term(308, ring["ring_done"][:n])
        k += _term(309, age.view(np.uint32))
    return k


def host_draw(keys, priority, seed, brain, calls, n_draws, alpha=0.6):
    """Draw d takes the row with the smallest (t, v, slot): v = mix64(key ^ salt_d), U = ((v >> 41) + 0.5) / 2^23, t = -log(U) / p^alpha."""
    import ctypes as C
    from reinlife_amd import _lib
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    w = (np.asarray(priority, np.float32) ** np.float32(alpha)).astype(np.float32)
    rows = np.zeros(n_draws, np.int64)
    for d in range(n_draws):
        lib.rl_philox(seed, 0, brain, calls, _lib.SITE_LEARN_PRIO, d, C.byref(out))
        v = _mix64(keys ^ np.uint64((int(out[1]) << 32) | int(out[0])))
        u = ((v >> np.uint64(41)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(w > 0, -np.log(u) / w, np.inf).astype(np.float32)
        rows[d] = np.lexsort((np.arange(len(keys)), v, t))[0]
    return rows


def _salts(seed, brain, calls, site, n_draws):
    """salt_d = words 0-1 of rl_philox(seed, 0, brain, calls, site, d), d = 0 .. n_draws - 1 -> uint64 [n_draws]."""
    import ctypes as C
    from reinlife_amd import _lib
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    salts = np.zeros(n_draws, np.uint64)
    for d in range(n_draws):
        lib.rl_philox(seed, 0, brain, calls & 0xffffffff, site, d, C.byref(out))
        salts[d] = (int(out[1]) << 32) | int(out[0])
    return salts


def host_uniform_draw(keys, seed, brain, calls, n_draws, site=None):
    """k_learn_pick restated, all in integers: draw d takes argmin_i mix64(keys[i] ^ salt_d), the lower slot winning equal values;
    salt_d from RL_SITE_LEARN (site: another Philox site -- RL_SITE_LEARN_PRIO for the prioritised draw with no weight anywhere)."""
    from reinlife_amd import _lib
    keys = np.asarray(keys, np.uint64)
    salts = _salts(seed, brain, calls, _lib.SITE_LEARN if site is None else site, n_draws)
    return np.array([int(np.argmin(_mix64(keys ^ s))) for s in salts], np.int64)   # (argmin: the first of equal values)


def host_draw64(keys, weight32, seed, brain, calls, n_draws, site=None):
    """host_draw's integer part with t = -log(U) / weight in float64, from the float32 weights the device itself made (learner.weight
    read back), so that powf's rounding stays out of the comparison -> (the winner of every draw by (t, v, slot), the relative gap
    (t_second - t_first) / t_first of every draw: +inf where no second row has a weight).  site: another Philox site than
    RL_SITE_LEARN_PRIO -- RL_SITE_LEARN_TD for rl_learn_td_draw, whose race weight is the stored priority itself."""
    from reinlife_amd import _lib
    keys, w = np.asarray(keys, np.uint64), np.asarray(weight32).astype(np.float64)
    slot = np.arange(len(keys))
    rows, gaps = np.zeros(n_draws, np.int64), np.zeros(n_draws)
    for d, s in enumerate(_salts(seed, brain, calls, _lib.SITE_LEARN_PRIO if site is None else site, n_draws)):
        v = _mix64(keys ^ s)
        u = ((v >> np.uint64(41)).astype(np.float64) + 0.5) / 8388608.0
        t = np.full(len(keys), np.inf)
        t[w > 0] = -np.log(u[w > 0]) / w[w > 0]
        order = np.lexsort((slot, v, t))
        rows[d] = order[0]
        first, second = t[order[0]], (t[order[1]] if len(keys) > 1 else np.inf)
        gaps[d] = (second - first) / first if np.isfinite(second) else np.inf
    return rows, gaps


def edge_priorities(n, seed=5):
    """The priorities of the row-for-row draw tests: random^3 * 4 (weights over several orders of magnitude), every 7th row 0 -- no
    zeros on a ring of at most three rows."""
    pri = (np.random.RandomState(seed).random_sample(n) ** 3 * 4).astype(np.float32)
    if n > 3:
        pri[::7] = 0.0
    return pri
