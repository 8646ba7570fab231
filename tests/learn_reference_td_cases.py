"""What tools/gen_golden_learn_reference_td.py and the learn_reference_td=True tests share: the run's configuration, a literal sequential
model of the reference's sum tree written from the formulae of include/reinlife_hip.h (rl_learn_td_tree_store / _sample / _update), the
same updates in the per-node form the kernel computes them in, the case tables of the device tests and the product-side brain of the
fixture.

tests/golden/learn_reference_perdqn.npz (a run of the real reference's trainer loop with one PERDQN brain, learn() included, from seeds)
holds what learn_reference_perd3qn.npz holds up to the calls (tests/learn_reference_cases.py, tests/learn_reference_prioritized_cases.py:
the actions, the post-step lists, both generators' digests, the environment's draws, the decisions' gaps, the outputs on 64 states, the
yardsticks; the initial parameters are weights(init_seeds[0]) of THIS module) and:
    capacity, batch, train_start             the brain's memory size, batch size and gate
    call_tick, call_size, call_stored [n_calls]      per train_model(): the tick, min(rows stored, capacity) and the rows stored at the call
    call_uniforms [n_calls, batch] float64   the doubles Memory.sample's random.uniform calls consumed: random.random() from the state before
    call_idxs [n_calls, batch] int32         the TREE indices Memory.sample answered
    call_s, call_leaves [n_calls, batch] float64     each draw's point s and the leaf value it read
    call_lo [n_calls, batch] float64         the sum of the leaves left of each draw's leaf: the draw lies in (lo, lo + leaf]
    call_total [n_calls] float64             tree[0] at the call
    call_is_weight [n_calls, batch] float64, call_errors [n_calls, batch] float32    what sample() returned and what update() was handed
    call_epsilon [n_calls] float64           brain.epsilon behind each train_model()
    final_leaves [capacity] float64, final_tree [2 capacity - 1] float64, final_beta, final_epsilon, final_stored
    interval_err                             D: the largest |cumulative leaf sum of a float64 replay's tree - the run's| over all calls
    min_margin, min_margin_rel               the smallest distance of a draw from the ends of its leaf's interval, absolute and / total
    duplicates [n_calls]                     leaves named more than once per batch"""
import os

import numpy as np

import learn_reference_cases as lrc

NAME = "perdqn"
SHAPES = [("fc.0", 64, 153), ("fc.2", 64, 64), ("fc.4", 8, 64)]   # PERDQN.py:311-320
CASE = dict(args=dict(capacity=64, explore_step=20), train_start=48, n_brains=1, width=30, height=30, max_agents=10, max_ticks=130)
PRIO_E, PRIO_A = 0.01, 0.6
REL_MARGIN = 2.0 ** -20        # every draw at least this fraction of the total from both ends of its leaf's interval
RUN_MARGIN_FACTOR = 8.0        # ... and at least 8 D


def path():
    return os.path.join(lrc.GOLDEN_DIR, "learn_reference_%s.npz" % NAME)


def load():
    with np.load(path()) as z:
        return {k: z[k] for k in z.files}


def weights(seed):
    """Repo-generated initial parameters, flat float32 in state-dict order, nn.Linear-like scale (learn_reference_cases.weights' rule)."""
    rng = np.random.RandomState(seed)
    out = []
    for _, n_out, n_in in SHAPES:
        b = 1.0 / np.sqrt(n_in)
        out.append(rng.uniform(-b, b, size=(n_out, n_in)).astype(np.float32).reshape(-1))
        out.append(rng.uniform(-b, b, size=(n_out,)).astype(np.float32))
    return np.concatenate(out)


def outputs64(flat, states):
    """The network's Q values on `states` in float64."""
    x, off = np.asarray(states, np.float64), 0
    for k, (_, n_out, n_in) in enumerate(SHAPES):
        w = np.asarray(flat[off:off + n_out * n_in], np.float64).reshape(n_out, n_in); off += n_out * n_in
        b = np.asarray(flat[off:off + n_out], np.float64); off += n_out
        x = x @ w.T + b
        if k < len(SHAPES) - 1:
            x = np.maximum(x, 0.0)
    assert off == len(flat)
    return x


def p_new():
    """append_sample's priority: the float32 (0 + e) ** a as torch makes it (DeviceLearner.p_new)."""
    import torch
    return np.float32(float((torch.zeros(()) + PRIO_E) ** PRIO_A))


class TreeModel:
    """Memory / SumTree (PERDQN.py:198-308) kept literally, one operation at a time: `tree` float64 [2 C - 1], beside a ring of R slots
    that row a enters at a % R and `priority`, float32 by ring slot."""

    def __init__(self, capacity, ring_rows):
        self.C, self.R = int(capacity), int(ring_rows)
        self.tree = np.zeros(2 * self.C - 1, np.float64)
        self.priority = np.zeros(self.R, np.float32)
        self.stored = 0

    def update(self, idx, p, single=False):
        """SumTree.update.  single: as the reference runs it for a float32 torch scalar p (Memory.add from append_sample): the change
        and every sum are float32 operations on the float64 nodes rounded to float32."""
        if single:
            change = np.float32(p) - np.float32(self.tree[idx])
            self.tree[idx] = np.float64(np.float32(p))
            while idx != 0:
                idx = (idx - 1) // 2
                self.tree[idx] = np.float64(np.float32(self.tree[idx]) + change)
            return
        p = np.float64(p)
        change = p - self.tree[idx]
        self.tree[idx] = p
        while idx != 0:
            idx = (idx - 1) // 2
            self.tree[idx] = self.tree[idx] + change

    def store(self, m, p):
        """Memory.add for the next m rows, each with the float32 priority p."""
        for _ in range(int(m)):
            self.update(self.stored % self.C + self.C - 1, np.float32(p), single=True)
            self.priority[self.stored % self.R] = np.float32(p)
            self.stored += 1

    def slot_of(self, idx):
        """The ring slot of the row the leaf `idx` holds (learn_reference.memory_slots' formula)."""
        j = int(idx) - (self.C - 1)
        return (j + self.C * ((self.stored - 1 - j) // self.C)) % self.R

    def update_batch(self, idxs, slots):
        """train_model's loop: update(idxs[i], priority[slots[i]]) in order."""
        for i, s in zip(idxs, slots):
            self.update(int(i), self.priority[int(s)])

    def retrieve(self, s):
        idx, s = 0, np.float64(s)
        while 2 * idx + 1 < len(self.tree):
            left = 2 * idx + 1
            if s <= self.tree[left]:
                idx = left
            else:
                s = s - self.tree[left]
                idx = left + 1
        return idx, s

    def sample(self, u):
        """Memory.sample's draw from the uniforms u -> dict(idxs, slots, s, leaves, bad): bad where the reference would draw again (a leaf
        no row has reached) or the total is no positive finite number; idxs and slots then name memory index 0 throughout."""
        u = np.asarray(u, np.float64)
        n, total = len(u), self.tree[0]
        filled = min(self.stored, self.C)
        if not (total > 0 and np.isfinite(total)):
            return dict(bad=True, idxs=[self.C - 1] * n, slots=[self.slot_of(self.C - 1)] * n)
        segment = total / np.float64(n)
        idxs, ss = [], []
        for i in range(n):
            a, b = segment * np.float64(i), segment * np.float64(i + 1)
            s = a + (b - a) * u[i]
            idxs.append(self.retrieve(s)[0]); ss.append(s)
        if any(i - (self.C - 1) >= filled for i in idxs):
            return dict(bad=True, idxs=[self.C - 1] * n, slots=[self.slot_of(self.C - 1)] * n)
        return dict(bad=False, idxs=idxs, slots=[self.slot_of(i) for i in idxs], s=np.array(ss, np.float64), leaves=self.tree[idxs].copy())

    def leaf_lo(self, idx):
        """The sum of the leaves left of leaf `idx` as the walk sees it: what a draw that ends there has had subtracted."""
        lo = np.float64(0.0)
        path = []
        while idx != 0:
            path.append(idx); idx = (idx - 1) // 2
        for node in reversed(path):
            if node % 2 == 0:          # a right child: the walk subtracted its left sibling
                lo = lo + self.tree[node - 1]
        return lo


def apply_per_node(tree, updates, single=False):
    """The list of (leaf, value) applied to `tree` in place the way rl_learn_td_ref.hip's kernel computes it: the changes from each
    leaf's own earlier updates, then every touched inner node's value by ONE chain over the node's own subsequence of the list.  No node
    is read after another node of the list has been written.  single: a store group (TreeModel.update's float32 form)."""
    leaves = [int(l) for l, _ in updates]
    vals = [np.float64(v) for _, v in updates]
    old = tree.copy()
    change = []
    for i, leaf in enumerate(leaves):
        prev = next((vals[j] for j in range(i - 1, -1, -1) if leaves[j] == leaf), old[leaf])
        change.append(np.float32(vals[i]) - np.float32(prev) if single else vals[i] - prev)
    for i, leaf in enumerate(leaves):
        if leaf not in leaves[i + 1:]:
            tree[leaf] = vals[i]
    depth = [int(np.log2(l + 1)) for l in leaves]
    for d in range(max(depth, default=0)):
        seen = set()
        for i, leaf in enumerate(leaves):
            if depth[i] <= d:
                continue
            node = (leaf + 1) >> (depth[i] - d)
            if node in seen:
                continue
            seen.add(node)
            v = old[node - 1]
            for j in range(i, len(leaves)):
                if depth[j] > d and (leaves[j] + 1) >> (depth[j] - d) == node:
                    v = np.float64(np.float32(v) + change[j]) if single else v + change[j]
            tree[node - 1] = v


# ---- the case tables of the device tests ------------------------------------------------------------------------------------------
TREE_CASES = ((2, 3), (3, 4), (5, 4), (64, 64), (96, 7), (20_000, 300))   # (capacity, slack): 5 and 96 have leaves at two depths; 300 > one LDS chunk


def script(capacity, slack, seed=0):
    """The operations of one store-and-update run through two wraps of the ring, as a list of
        ("store", first_row, m)  |  ("update", idxs, values)  |  ("check",)
    store groups of 1 .. slack rows (the first of one row), update batches of 1 and 64 entries over live leaves with duplicates inside a
    batch, the values float32 priorities over six binades, one per DISTINCT leaf (a row has one priority)."""
    C, R = int(capacity), int(capacity) + int(slack)
    rng = np.random.RandomState(1000 * C + seed)
    ops, stored, k = [], 0, 0
    while stored < 2 * R + slack:
        m = 1 if not stored else int(rng.randint(max(1, slack // 2) if C > 1000 else 1, slack + 1))
        ops.append(("store", stored, m))
        stored += m
        filled = min(stored, C)
        if rng.rand() < 0.7:
            n = 1 if k % 3 == 2 else 64
            idxs = rng.randint(0, filled, size=n) + C - 1
            if n > 1:
                idxs[1] = idxs[0]                      # a duplicate, adjacent ...
                idxs[-1] = idxs[n // 2]                # ... and one far apart
            distinct = sorted(set(idxs.tolist()))
            vals = dict(zip(distinct, (2.0 ** rng.uniform(-3.0, 3.0, size=len(distinct))).astype(np.float32)))
            ops.append(("update", idxs.astype(np.int32), vals))
            k += 1
        if C <= 1000 or len(ops) % 40 == 0:
            ops.append(("check",))
    ops.append(("check",))
    return ops


def run_script(model, ops, p, on_store=None, on_update=None, on_check=None):
    """The script on the literal model; the callbacks see every operation AFTER the model has taken it."""
    for op in ops:
        if op[0] == "store":
            model.store(op[2], p)
            if on_store:
                on_store(op[1], op[2])
        elif op[0] == "update":
            slots = np.array([model.slot_of(i) for i in op[1]], np.int32)
            for leaf, v in op[2].items():
                model.priority[model.slot_of(leaf)] = v
            model.update_batch(op[1], slots)
            if on_update:
                on_update(op[1], slots, op[2])
        elif on_check:
            on_check()


def product_brains(g):
    """The product's PERDQN brain of the fixture, carrying its initial weights (before any seeding: the constructors draw from torch)."""
    import torch
    from reinlife_amd import Models
    brain = Models.PERDQN(**CASE["args"])
    brain.train_start = int(CASE["train_start"])
    flat = weights(int(g["init_seeds"][0]))
    for net in ("model", "target_model"):
        off = 0
        with torch.no_grad():
            for t in getattr(brain, net).state_dict().values():
                t.copy_(torch.from_numpy(flat[off:off + t.numel()].reshape(tuple(t.shape)).copy()))
                off += t.numel()
        assert off == flat.size
    brain.invalidate()
    return [brain]
