"""ReferenceSchedule: when the reference's brains train and on which rows, as a host object that never touches a device.

trainer.py:95-96 calls Agent.learn() for every agent of the post-step list, in list order, between step() and update_env(); only
agents with age > 1 reach their brain (entities.py:196).  A brain's learn() stores the row and, when `age % train_freq == 0 or dead`,
trains -- and its minibatches come from random.sample over the replay deque, that is from the process-global `random` stream, between
the coins of act() and the draws of update_env().  This class is given, per tick, n_epi and the post-step agents' (brain, age, dead) in
list order; it makes those draws in that order and returns the tick's device calls, in order, as `Call`s:

  DQN  (DQN.py:80-89, 99-100, 142-153)   store; on the trigger train(): with more than 1000 rows five minibatches of
       random.sample(deque, 32) -> one Call of five steps, target copy included.  Below the gate train() only copies agent ->
       target, which changes nothing (the two are equal since the last update): no call.
  D3QN (D3QN.py:97-126, 139-140)         store; once n_epi > exploration: on the trigger one update on random.sample(deque, batch_size)
       (ValueError when the deque is shorter, as random.sample raises it, before anything is queued); then, if n_epi is a multiple of
       soft_update_freq, eval -> target -- after every such agent call, trained or not.  A copy that follows an update rides on that
       update's Call (sync_target); one without an update is a Call of its own (kind "sync"), left out where no update was made since the
       last copy.
  PPO  (PPO.py:71-77, 117-162)           store with the acting probability; on the trigger, if the list is not empty, one learn() over
       all rows stored since the last learn(), in storage order.  No draws.

Rows and slots.  A brain's rows are numbered from 0 in the order they are stored; the device ring (rl_capture_transitions) writes row a
to slot a % ring_rows, all rows of a tick in one launch BEFORE the tick's calls.  With a ring of exactly the deque's maxlen C the later
agents of a tick would overwrite rows an earlier agent's train() may still sample, so a ring here holds C + slack rows, slack >= the
most rows one tick appends (slot_cap).  At an agent's call with c rows stored, len = min(c, C), deque index i is row c - len + i and its
slot (c - len + i) % (C + slack) (deque_slots): every such row is still in the ring at the end of the tick.  A PPO list lives in a ring
of PPO_LIST_MAX + slack rows and may not grow beyond PPO_LIST_MAX rows (ValueError).

  PERD3QN (PERD3QN.py:117-125, 143-165; only where the caller opts in, BrainSpec.of(brain, prioritized=True))   D3QN's shape: store; once
       n_epi > exploration: on the trigger one update on np.random.choice(len, batch_size, p=probs) -- WITH replacement, so one row is
       enough and no size error is raised -- then the same target copies.  np.random.choice consumes exactly batch_size doubles of
       np.random.random_sample whatever p is: the Call carries u = np.random.random_sample(batch_size), the only draw made here (nothing
       comes from `random`), and the device walks the cdf of the priorities it keeps (rl_learn_prioritized_choice): `slots` and `indices`
       are None, they are the device's.  store() gives a new row the priorities' maximum AS OF THAT STORE and only train() changes the
       maximum, so the rows stored since the last stamp are stamped as one group in front of every train() (`store`, rows
       [first, first + count)), and a tick that stored rows ends with a Call of kind "store" for those not yet stamped: no group spans a
       train() and none exceeds the rows of one tick, that is `slack` rows.

  PERDQN (PERDQN.py:130-133, 188-195, 280-298; only where the caller opts in, BrainSpec.of(brain, td=True))   store (append_sample: the
       row enters the sum tree with the constant priority, no draw); on the trigger, if min(stored, memory_size) >= train_start, one
       train_model() and then model -> target_model (sync_target on every such Call).  Memory.sample(batch_size) calls random.uniform once
       per segment -- random.uniform(a, b) is a + (b - a) * random.random() -- as long as no draw lands on a leaf no row has reached: the
       Call carries u = [random.random() for _ in range(batch_size)], drawn HERE from the process-global `random` stream where the
       reference's calls fall, and the device keeps the tree and walks it (rl_learn_td_tree_sample): `slots` and `indices` are None.  The
       rows stored since the last group enter the tree in front of every train_model() (`store`), and a tick ends with a Call of kind
       "store" for the rest: PERD3QN's rules.  Below the gate the trigger's target copy changes nothing (the two are equal since the last
       update): no call.

Brains of other kinds are not scheduled: their rows are counted by nobody here and they make no draws."""
import random
from typing import NamedTuple

import numpy as np

DQN_CAPACITY, DQN_BATCH, DQN_STEPS, DQN_GATE = 50_000, 32, 5, 1000   # DQN.py:15, 16, 143, 81
PPO_LIST_MAX = 2048      # the rows of the longest PPO list a call can train on (rl_learn_ppo_wide's batch limit)
PPO_NARROW_MAX = 32      # up to here a list goes to rl_learn_ppo, beyond to rl_learn_ppo_wide
KINDS = ("DQN", "D3QN", "PPO")   # the brain methods this schedule trains
OPT_IN_KINDS = ("PERD3QN", "PERDQN")   # ... and those it trains where the caller asks for it (BrainSpec.of(brain, prioritized=True) / td=True)


class Call(NamedTuple):
    """One device call of a tick.  kind "learn": n_steps minibatch updates (DQN 5, D3QN 1) on the ring slots `slots` [n_steps][batch],
    then the target copy iff sync_target.  kind "sync": params -> target, no update (D3QN).  kind "ppo": one PPO.learn() on the rows at
    `slots` [1][length], wide iff the list is longer than PPO_NARROW_MAX.  `size` is the deque's (list's) length at the call and
    `indices` what random.sample drew, as deque indices [n_steps][batch] (PPO, sync: None).
    PERD3QN: kind "learn" carries `uniforms` [batch] float64 -- np.random.choice's doubles, for the device's cdf walk; slots and indices
    are None -- and `store` = (first row, rows): the group store() stamps in front of that train(); `size` is len(memory).  kind
    "store": the stamp alone, of the rows a tick stored behind its last train().
    PERDQN: the same two kinds; `uniforms` are random.random()'s doubles for Memory.sample's stratified walk, `store` the rows that enter
    the sum tree in front of that train_model(), sync_target is always on."""
    kind: str
    brain: int
    slots: np.ndarray = None
    sync_target: bool = False
    size: int = 0
    indices: np.ndarray = None
    wide: bool = False
    uniforms: np.ndarray = None
    store: tuple = None


class BrainSpec(NamedTuple):
    method: str
    train_freq: int = 20
    capacity: int = DQN_CAPACITY     # the deque's maxlen (PPO: the longest list)
    batch: int = DQN_BATCH
    exploration: int = 0
    soft_update_freq: int = 1
    train_start: int = 0             # PERDQN: the rows the memory must hold before train_model() runs (PERDQN.py:192)

    @classmethod
    def of(cls, brain, prioritized=False, td=False):
        """The spec of a brain object by its own attributes, or None for a kind this schedule does not train.  prioritized=True: a
        PERD3QN brain gets a spec too (Environment's learn_reference_prioritized=True); td=True: a PERDQN brain does
        (learn_reference_td=True)."""
        method, freq = getattr(brain, "method", None), int(getattr(brain, "train_freq", 20))
        if method == "DQN":
            return cls("DQN", freq)
        if method == "D3QN":
            return cls("D3QN", freq, int(brain.capacity), int(brain.batch_size), int(brain.exploration), int(brain.soft_update_freq))
        if method == "PPO":
            return cls("PPO", freq, PPO_LIST_MAX, 0)
        if method == "PERD3QN" and prioritized:
            return cls("PERD3QN", freq, int(brain.capacity), int(brain.batch_size), int(brain.exploration), int(brain.soft_update_freq))
        if method == "PERDQN" and td:
            return cls("PERDQN", freq, int(brain.memory_size), int(brain.batch_size), train_start=int(brain.train_start))
        return None


def memory_rows(stored, capacity, indices):
    """The rows PrioritizedReplayBuffer.memory holds at `indices` once `stored` rows were stored (PERD3QN.py:149-155: row a is written to
    index a % capacity): index i holds the latest such row, i + capacity * ((stored - 1 - i) // capacity)."""
    i = np.asarray(indices, np.int64)
    return i + int(capacity) * ((int(stored) - 1 - i) // int(capacity))


def memory_slots(stored, capacity, ring_rows, indices):
    """... and the ring slots they sit in: row a is in slot a % ring_rows (rl_learn_prioritized_choice's `slots`)."""
    return (memory_rows(stored, capacity, indices) % int(ring_rows)).astype(np.int32)


def deque_slots(stored, capacity, ring_rows, indices):
    """The ring slots of the deque's elements `indices` at a call with `stored` rows stored so far: deque(maxlen=capacity) then holds
    rows stored - len .. stored - 1, len = min(stored, capacity), and row a sits in slot a % ring_rows."""
    size = min(int(stored), int(capacity))
    return ((int(stored) - size + np.asarray(indices, np.int64)) % int(ring_rows)).astype(np.int32)


class ReferenceSchedule:
    def __init__(self, specs, slack):
        """specs: one BrainSpec (or None: not trained) per brain; slack: the rows a ring holds beyond its deque's maxlen -- at least the
        most rows one tick can append to it."""
        self.specs, self.slack = list(specs), int(slack)
        if self.slack < 1:
            raise ValueError("ReferenceSchedule: slack must be >= 1 (the most rows one tick appends to a ring), got %r" % (slack,))
        for s in self.specs:
            if s is not None and s.method not in KINDS + OPT_IN_KINDS:
                raise ValueError("ReferenceSchedule trains %s brains, not %s" % (", ".join(KINDS), s.method))
        n = len(self.specs)
        self.stored = [0] * n        # rows stored so far, per brain
        self.listed = [0] * n        # PPO: the row the current list starts at
        self.stale = [False] * n     # D3QN, PERD3QN: an update was made since the last eval -> target copy
        self.stamped = [0] * n       # PERD3QN, PERDQN: the rows whose priority store() / Memory.add has been queued for
        self.calls = 0               # Calls handed out so far

    def ring_rows(self, brain):
        """The rows the device ring of `brain` must hold: its deque's maxlen (PPO: the longest list) + slack."""
        return self.specs[brain].capacity + self.slack

    def size(self, brain):
        """len(deque) of `brain` (PPO: of its list) as of now."""
        s = self.specs[brain]
        return self.stored[brain] - self.listed[brain] if s.method == "PPO" else min(self.stored[brain], s.capacity)

    def tick(self, n_epi, agents):
        """agents: the post-step list's (brain, age, dead) in list order -> the tick's Calls in order.  Draws from `random`."""
        agents = [(int(b), int(age), bool(dead)) for b, age, dead in agents]
        learning = [a for a in agents if a[1] > 1 and self.specs[a[0]] is not None]   # entities.py:196
        per_brain = {}
        for b, _, _ in learning:
            per_brain[b] = per_brain.get(b, 0) + 1
        over = [b for b, n in per_brain.items() if n > self.slack]
        if over:
            raise ValueError("ReferenceSchedule: brain %d stores %d rows in one tick, more than the rings' slack of %d rows"
                             % (over[0], per_brain[over[0]], self.slack))
        out = []
        for b, age, dead in learning:
            s = self.specs[b]
            self.stored[b] += 1                                   # memorize() / put_data()
            trigger = age % s.train_freq == 0 or dead
            out += getattr(self, "_" + s.method.lower())(b, s, n_epi, trigger)
        for b in sorted(per_brain):                               # PERD3QN, PERDQN: the rows stored behind the tick's last train()
            if self.specs[b].method in OPT_IN_KINDS and self.stamped[b] < self.stored[b]:
                out.append(Call("store", b, store=self._store_group(b)))
        self.calls += len(out)
        return out

    def _sample(self, b, s, n_steps):
        size = self.size(b)
        idx = np.array([random.sample(range(size), s.batch) for _ in range(n_steps)], np.int64)
        return size, idx, deque_slots(self.stored[b], s.capacity, self.ring_rows(b), idx)

    def _dqn(self, b, s, n_epi, trigger):
        if not trigger or self.size(b) <= DQN_GATE:               # DQN.py:81: the copy below the gate changes nothing
            return []
        size, idx, slots = self._sample(b, s, DQN_STEPS)
        return [Call("learn", b, slots, True, size, idx)]

    def _d3qn(self, b, s, n_epi, trigger):
        if n_epi <= s.exploration:                                # D3QN.py:121
            return []
        sync = n_epi % s.soft_update_freq == 0                    # D3QN.py:125-126: after every such agent call
        if trigger:
            if self.size(b) < s.batch:                            # random.sample's own refusal, before anything is drawn or queued
                raise ValueError("Sample larger than population or is negative (brain %d: D3QN.train() at n_epi %d samples %d rows of a "
                                 "replay buffer of %d)" % (b, n_epi, s.batch, self.size(b)))
            size, idx, slots = self._sample(b, s, 1)
            self.stale[b] = not sync
            return [Call("learn", b, slots, sync, size, idx)]
        if sync and self.stale[b]:
            self.stale[b] = False
            return [Call("sync", b)]
        return []

    def _store_group(self, b):
        first, self.stamped[b] = self.stamped[b], self.stored[b]
        return (first, self.stored[b] - first)

    def _perd3qn(self, b, s, n_epi, trigger):
        if n_epi <= s.exploration:                                # PERD3QN.py:120
            return []
        sync = n_epi % s.soft_update_freq == 0                    # PERD3QN.py:124-125: after every such agent call
        if trigger:
            u = np.random.random_sample(s.batch)                  # np.random.choice(len, batch, p=probs): these doubles, nothing else
            self.stale[b] = not sync
            return [Call("learn", b, None, sync, self.size(b), None, False, u, self._store_group(b))]
        if sync and self.stale[b]:
            self.stale[b] = False
            return [Call("sync", b)]
        return []

    def _perdqn(self, b, s, n_epi, trigger):
        if not trigger or self.size(b) < s.train_start:           # PERDQN.py:191-192: below the gate the copy changes nothing
            return []
        u = np.array([random.random() for _ in range(s.batch)], np.float64)   # Memory.sample: one random.uniform per segment
        return [Call("learn", b, None, True, self.size(b), None, False, u, self._store_group(b))]

    def _ppo(self, b, s, n_epi, trigger):
        n = self.size(b)
        if n > PPO_LIST_MAX:
            raise ValueError("brain %d: the PPO list holds %d rows, more than the %d rows a learning call takes (rl_learn_ppo_wide's limit)"
                             % (b, n, PPO_LIST_MAX))
        if not trigger or n == 0:
            return []
        slots = ((self.listed[b] + np.arange(n, dtype=np.int64)) % self.ring_rows(b)).astype(np.int32).reshape(1, n)
        self.listed[b] = self.stored[b]
        return [Call("ppo", b, slots, False, n, None, n > PPO_NARROW_MAX)]
