"""DeviceLearner: what a DQN (also on wide minibatches: wide_batch=, rl_learn_wide), D3QN (also on wide minibatches: dueling_batch=, rl_learn_dueling_wide), (prioritized=True) PERD3QN, (rollout=True) PPO (also on wide rollouts: rollout_batch=, rl_learn_ppo_wide) or (td_priority=True) PERDQN (also on wide minibatches: td_batch=, rl_learn_td_wide) brain needs to learn on
the device (rl_learn / rl_learn_dueling / rl_learn_prioritized / rl_learn_ppo / rl_learn_td, include/reinlife_hip.h) -- the flat f32 master parameters,
the target network, Adam's moments, the step / call counters and the packed weights the acting kernels read, all as device tensors.

Reference: DQNAgent owns `agent`, `target`, `memory` and `optimizer` (ReinLife/Models/DQN.py:48-52); train() (DQN.py:80-83, 142-153)
samples 5 minibatches of 32 and makes one Adam step on each, then copies agent -> target.  Here the replay memory is the brain's
rl_replay ring (DeviceWorlds.enable_capture) and the five steps are ONE launch (DeviceWorlds.learn).  Two deviations, stated wherever
this is documented: minibatches are drawn WITH replacement (the reference's random.sample draws without), and the schedule of train()
calls is the caller's (Environment: once per `learn_every` episodes), not "whenever an agent's age is a multiple of train_freq".

D3QNAgent owns `eval_net`, `target_net`, `buffer` and `optimizer` (ReinLife/Models/D3QN.py:58-62); train() (D3QN.py:97-116) samples ONE
minibatch of 64 and makes one Adam step on its MSE loss; learn() (D3QN.py:118-126) trains only once n_epi > exploration and copies eval ->
target every soft_update_freq episodes.  The learner takes lr, gamma, batch, train_freq, exploration and soft_update_freq from the
brain; its only size gate is random.sample's need of `batch` rows (min_size = batch - 1); the same two deviations apply.

PERD3QNAgent (ReinLife/Models/PERD3QN.py:48-66) is the D3QN agent with a prioritised memory: train() (PERD3QN.py:94-115) makes the same
update on the same plain MSE loss -- sample()'s importance weights are computed and never used -- and then sets the priority of every
batch row to |max_a q'_target(s') - q_eval(s)[a]| (PERD3QN.py:110-111).  DeviceLearner(brain, device, ring, prioritized=True) is that
agent's learner (rl_learn_prioritized): besides the D3QN learner's tensors it owns the memory's priorities (one per ring row), their
maximum, the ring count as of the last draw, and two scratch columns of the draw (DeviceWorlds.draw_prioritized: probability
priority^0.6 / sum, with replacement, by content key).  Its only size gate is np.random.choice's need of one row (min_size = 0).  The
same two deviations apply, and one more follows from the first: every row appended between two learning calls gets the priority
maximum as of the earlier call.  DeviceLearner(brain, device, ring, prioritized=True, prioritized_batch=B) is the same learner on wide
minibatches of B <= 2048 rows (rl_learn_prioritized_wide, this build's own: rl_learn_dueling_wide's tiled update with the priorities of
all B rows written and their maximum kept); it also owns that entry point's work buffer.

PPOAgent (ReinLife/Models/PPO.py:10-77) owns one module, `model`, with its own Adam (PPO.py:99) and the list of transitions gathered since
the last learn() (PPO.py:88, 114-115); learn() (PPO.py:136-162) makes k_epoch full-batch Adam steps on that list and empties it.
DeviceLearner(brain, device, ring, rollout=True) is that agent's learner (rl_learn_ppo): the parameters, Adam's moments, the counters and
the packed weights as above (no target network), lr / gamma / lmbda / eps_clip / k_epoch from the brain, and beside the ring -- which must
carry the acting probability (enable_capture(..., with_prob=True)) -- the bookkeeping of the on-policy window: the ring count as of the last
rollout, the rows the last window held, and the draw's scratch keys (DeviceWorlds.draw_rollout: `batch` = 32 rows per rollout, drawn
uniformly with replacement by content key from the rows appended since the last call).  Deviations: the schedule is the caller's; a rollout
is 32 independent draws, so the GAE recursion's neighbours are unrelated rows (in the reference: unrelated agents of one tick); the fresh
rows not drawn go unused.  DeviceLearner(brain, device, ring, rollout=True, rollout_batch=B) is the same learner on wide rollouts of
B <= 2048 rows (rl_learn_ppo_wide: 32-row tiles side by side with ONE GAE recursion over the whole rollout, both means over all B rows;
the tiling is this build's own, the length is not -- PPO.learn() trains on the whole list, however long); it also owns that entry
point's work buffer, and its draw is rl_learn_rollout_wide.

PERDQNAgent (ReinLife/Models/PERDQN.py) owns `model`, `target_model`, `memory` (a sum tree of priorities) and `optimizer`; train_model()
makes one Adam step on a minibatch of 64 drawn by priority.  DeviceLearner(brain, device, ring, td_priority=True) is that agent's learner
(rl_learn_td): lr, gamma, batch, train_start, train_freq and the memory's size from the brain; beside the D3QN learner's tensors the
memory's priorities (one per ring row), the ring count as of the last draw, the draw's scratch keys and beta (a device double, 0.4 -> 1 by
0.001 per update).  Three quirks of the reference are reproduced, not repaired: append_sample gives EVERY new row the priority
(0 + 0.01) ** 0.6 (its error is taken against a view of the tensor it has just overwritten; `p_new` is that float32, made with torch as
the reference makes it); the loss is mean(is_weight) * mean((pred - target)^2), not weighted per row; is_weight is
(p_i / min_j p_j) ** -beta over the batch.  learn() copies model -> target_model after every trigger, so sync_target is always on.
Deviations: Memory.sample is stratified through the sum tree -- here every draw is independent with probability p_i / sum p, by content
key, with replacement (DeviceWorlds.draw_td); the schedule is the caller's (once per `learn_every` episodes), so epsilon decays once per
update made, not once per agent trigger -- a smaller explore_step restores the reference's rate in wall-clock terms.
DeviceLearner(brain, device, ring, td_priority=True, td_batch=B) is the same learner on wide minibatches of B <= 2048 rows (rl_learn_td_wide,
this build's own: 64-row tiles side by side, the importance weights' minimum and mean taken over the whole batch by a pass of their own in
front of every step's tiles, the priorities of all B rows rewritten); it also owns that entry point's work buffer, and its draws are
rl_learn_td_wide_draw and rl_learn_td_wide_draw_rank."""
import copy
import ctypes as C
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib

GAMMA, BATCH, MIN_SIZE, BUFFER_LIMIT = 0.98, 32, 1000, 50_000   # DQN.py:14-16, 81
FAMILIES = ("dqn", "dueling", "prioritized", "ppo", "td")   # in Environment.learn_now's order of calls
# what sync_to_module writes: the module of the parameters and the module of the target network (None: none), per family
MODULES = {"dqn": ("agent", "target"), "dueling": ("eval_net", "target_net"), "prioritized": ("eval_net", "target_net"),
           "ppo": ("model", None), "td": ("model", "target_model")}
# the learner tensors a side struct is made of: (one per ring row?, dtype, what a fresh one holds)
SIDE_TENSORS = {"priority": (True, torch.float32, 0), "weight": (True, torch.float32, 0), "keys": (True, torch.int64, 0),
                "prio_max": (False, torch.float32, 1.0),   # PERD3QN.py:147
                "seen": (False, torch.int64, 0), "fresh": (False, torch.int64, 0), "beta_is": (False, torch.float64, 0.4)}   # Memory.beta


class Entry(NamedTuple):
    """One C entry point that trains brains, and all the Python layer knows about it: DeviceLearner, DeviceWorlds.learn / draw_* and
    Environment read these rows and compare no entry names."""
    name: str
    method: str                      # the brain method it trains
    family: str                      # one of FAMILIES: hyperparameters, gates, Environment.learn_now's schedule, sync_to_module's modules
    has_target: bool = True
    ring_rows: str = None            # the brain attribute that sizes its replay ring (None: BUFFER_LIMIT)
    keyword: str = None              # the DeviceLearner keyword that selects it (None: entry_of() does); Environment's is "learn_" + keyword
    conflicts: tuple = ()            # the keywords that keyword excludes, in the order its message names them
    needs: str = None                # the keyword that keyword goes on top of
    narrow: str = None               # a wide entry: the entry it stands in for (the keyword is then the batch, Environment's learn_batch)
    batch_max: str = None            # ... and the name of its batch limit in _lib
    one_batch: bool = False          # DeviceWorlds.learn refuses unequal batches itself (elsewhere the C library answers)
    side: type = None                # the struct it passes beside the rings: _lib.Prio, _lib.Ppo or _lib.TdPrio
    side_tensors: tuple = ()         # ... and the learner tensors that struct is made of (SIDE_TENSORS)
    draw: str = None                 # its own draw entry (None: the uniform draws, draw_slots / draw_slots_rank)
    launches: Callable = lambda n_steps: 1   # what one call of n_steps counts as
    per_epoch: bool = False          # launches takes (n_steps, k_epoch): the count depends on the largest k_epoch among the call's learners
    draw_rank: str = None            # its own prefix-sum draw entry (None: the family's, as DeviceWorlds.draw_*_rank names it)

    supported = property(lambda e: e.name + "_supported")
    work_bytes = property(lambda e: e.name + "_work_bytes" if e.narrow else None)


_PRIO = dict(side=_lib.Prio, side_tensors=("priority", "weight", "keys", "prio_max", "seen"))
# A row's index is part of the learner signature the ranks compare (Environment._align_learners): new entries go to the END.  The keyword
# rows are tried last to first (DeviceLearner), so a new opt-in is checked before the older ones it names as conflicts.
ENTRIES = (
    Entry("rl_learn", "DQN", "dqn"),
    Entry("rl_learn_dueling", "D3QN", "dueling", ring_rows="capacity"),
    Entry("rl_learn_prioritized", "PERD3QN", "prioritized", ring_rows="capacity", keyword="prioritized", draw="rl_learn_prioritized_draw", **_PRIO),
    Entry("rl_learn_ppo", "PPO", "ppo", has_target=False, keyword="rollout", conflicts=("prioritized",),
          side=_lib.Ppo, side_tensors=("keys", "seen", "fresh"), draw="rl_learn_rollout"),
    Entry("rl_learn_td", "PERDQN", "td", ring_rows="memory_size", keyword="td_priority", conflicts=("prioritized", "rollout"),
          side=_lib.TdPrio, side_tensors=("priority", "keys", "seen", "beta_is"), draw="rl_learn_td_draw"),
    Entry("rl_learn_wide", "DQN", "dqn", keyword="wide_batch", conflicts=("prioritized", "rollout", "td_priority"),
          narrow="rl_learn", batch_max="LEARN_WIDE_MAX", launches=lambda n_steps: 2 * n_steps + 3),   # check, tiles and update per step, target / counters, pack
    Entry("rl_learn_dueling_wide", "D3QN", "dueling", ring_rows="capacity", keyword="dueling_batch",
          conflicts=("wide_batch", "prioritized", "rollout", "td_priority"), narrow="rl_learn_dueling", batch_max="LEARN_DUELING_WIDE_MAX",
          one_batch=True, launches=lambda n_steps: 3 * n_steps + 3),   # check, the two tile passes and the update per step, target / counters, pack
    Entry("rl_learn_prioritized_wide", "PERD3QN", "prioritized", ring_rows="capacity", keyword="prioritized_batch", needs="prioritized",
          conflicts=("wide_batch", "dueling_batch", "rollout", "td_priority"), narrow="rl_learn_prioritized",
          batch_max="LEARN_PRIORITIZED_WIDE_MAX", one_batch=True, draw="rl_learn_prioritized_wide_draw",
          launches=lambda n_steps: 3 * n_steps + 3, **_PRIO),   # as rl_learn_dueling_wide
)
# ENTRIES stays these eight rows: tests count them (tests/test_learn_td_stamp_cpu.py, tests/test_learn_prio_draw_rank_cpu.py).  The rows added
# since stand in MORE_ENTRIES, and the layer reads ALL_ENTRIES = ENTRIES + MORE_ENTRIES: what is said above of a row's index and of the order
# the keyword rows are tried in holds for that table, and a new row goes to the END of MORE_ENTRIES.
# The one exception to "the END": rl_learn_td_wide stands IN FRONT of rl_learn_ppo_wide, because tests/test_learn_ppo_wide_cpu.py pins
# ALL_ENTRIES[-1] to that row.  The index is compared between the ranks of ONE run (Environment._align_learners), never stored, so
# rl_learn_ppo_wide's moving from 8 to 9 changes no run; rollout_batch names td_batch as a conflict, since it is now tried first.
MORE_ENTRIES = (
    Entry("rl_learn_td_wide", "PERDQN", "td", ring_rows="memory_size", keyword="td_batch", needs="td_priority",
          conflicts=("wide_batch", "dueling_batch", "prioritized", "prioritized_batch", "rollout", "rollout_batch"), narrow="rl_learn_td",
          batch_max="LEARN_TD_WIDE_MAX", one_batch=True, side=_lib.TdPrio, side_tensors=("priority", "keys", "seen", "beta_is"),
          draw="rl_learn_td_wide_draw", draw_rank="rl_learn_td_wide_draw_rank",
          launches=lambda n_steps: 3 * n_steps + 3),   # check, the weights pass, the tiles and the update per step, target / counters / beta, pack
    Entry("rl_learn_ppo_wide", "PPO", "ppo", has_target=False, keyword="rollout_batch", needs="rollout",
          conflicts=("wide_batch", "dueling_batch", "prioritized", "prioritized_batch", "td_priority", "td_batch"), narrow="rl_learn_ppo",
          batch_max="LEARN_PPO_WIDE_MAX", one_batch=True, side=_lib.Ppo, side_tensors=("keys", "seen", "fresh"), draw="rl_learn_rollout_wide",
          launches=lambda n_steps, k_epoch: 3 * n_steps * k_epoch + 3, per_epoch=True),   # check, the two tile passes and the update per rollout and epoch, counters, pack
)
ALL_ENTRIES = ENTRIES + MORE_ENTRIES
ENTRY = {e.name: e for e in ALL_ENTRIES}
ENTRY_BY_METHOD = {e.method: e.name for e in ALL_ENTRIES if not e.keyword}   # the brain kinds an entry point trains without a keyword (Environment's learn_kinds)
assert all(e.family in FAMILIES and set(e.side_tensors) <= set(SIDE_TENSORS) for e in ALL_ENTRIES) and set(ENTRY_BY_METHOD.values()) <= set(ENTRY)


def entry_of(kind):
    """The name of the C entry point that trains brains of `kind`, or None."""
    lib = _lib.lib()
    return next((name for name in ENTRY_BY_METHOD.values() if getattr(lib, ENTRY[name].supported)(kind)), None)


def _spelled(keyword):
    return keyword if keyword.endswith("_batch") else keyword + "=True"


class DeviceLearner:
    def __init__(self, brain, device="cuda:0", ring=None, prioritized=False, rollout=False, td_priority=False, prioritized_batch=None, *,
                 td_batch=None, rollout_batch=None, wide_batch=None, dueling_batch=None):
        # (the keywords behind `*` are keyword-only: td_batch and rollout_batch stand in front of wide_batch and dueling_batch, whose place
        # as the signature's last two names is pinned, and a caller that passed those two by position must get a TypeError, not another keyword)
        lib = _lib.lib()
        given = dict(prioritized=prioritized, rollout=rollout, td_priority=td_priority, prioritized_batch=prioritized_batch, wide_batch=wide_batch,
                     dueling_batch=dueling_batch, rollout_batch=rollout_batch, td_batch=td_batch)
        given = {k: v for k, v in given.items() if (v is not None if k.endswith("_batch") else v)}
        # every keyword is an explicit opt-in: entry_of() and ENTRY_BY_METHOD keep answering what they answered
        spec = next((e for e in reversed(ALL_ENTRIES) if e.keyword in given), None)
        if spec is None:
            spec = ENTRY.get(entry_of(brain.kind))
            if spec is None:
                raise ValueError("no entry point trains %s brains (kind %d): only DQN (rl_learn) and D3QN (rl_learn_dueling) learn on the device"
                                 % (brain.method, brain.kind))
        else:
            other = next((" with " + _spelled(k) for k in spec.conflicts if k in given), "")
            if not other and spec.needs and spec.needs not in given:
                other = " without " + _spelled(spec.needs)
            if other or not getattr(lib, spec.supported)(brain.kind):
                raise ValueError("%s is for %s brains%s (%s); got a %s brain (kind %d)%s" % (
                    _spelled(spec.keyword), spec.method, " with " + _spelled(spec.needs) if spec.needs else "", spec.name, brain.method, brain.kind, other))
            if spec.narrow:   # a wide entry: the narrow entry's learner with its own batch
                batch, limit = given[spec.keyword], getattr(_lib, spec.batch_max)
                if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or not 1 <= batch <= limit:
                    raise ValueError("%s must be an int in [1, %d] (the rows of a minibatch of %s), got %r" % (spec.keyword, limit, spec.name, batch))
        self.spec, self.entry = spec, spec.name
        from .worlds import pack_brain_weights
        self.brain, self.kind, self.device = brain, brain.kind, torch.device(device)
        flat = brain.state_dict_flat()
        self.n_params = int(lib.rl_policy_n_params(self.kind))
        self.merge_floats = int(lib.rl_learn_merge_floats(self.kind))   # this learner's segment of an exported row: params | adam_m | adam_v | step count
        self.params = torch.as_tensor(flat, device=self.device)
        self.target = self.params.clone() if spec.has_target else None  # DQN.py:50 / D3QN.py:60 (PPO has no target network)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)   # [Adam steps taken, rl_learn calls made]
        self.packed = pack_brain_weights(self.kind, flat, self.device)
        self.train_freq = int(getattr(brain, "train_freq", 20))
        if spec.family == "ppo":   # PPO.py:42-43: the brain's own hyperparameters
            self.lr, self.gamma = float(getattr(brain, "learning_rate", 0.0005)), float(getattr(brain, "gamma", 0.98))
            self.lmbda, self.eps_clip, self.k_epoch = float(getattr(brain, "lmbda", 0.95)), float(getattr(brain, "eps_clip", 0.1)), int(getattr(brain, "k_epoch", 3))
            self.batch, self.min_size = _lib.PPO_ROLLOUT_MAX, 0  # the rows of a rollout; no size gate (an empty window makes no update)
            self.n_steps_default = 1                             # one PPO.learn() per call
            self.sync_target = False
        elif spec.family == "td":   # PERDQNAgent.__init__: the brain's own hyperparameters
            self.lr, self.gamma = float(getattr(brain, "learning_rate", 1e-3)), float(getattr(brain, "discount_factor", 0.99))
            self.batch = int(getattr(brain, "batch_size", 64))
            self.train_start, self.memory_size = int(getattr(brain, "train_start", 1000)), int(getattr(brain, "memory_size", 20000))
            self.min_size = self.train_start - 1                 # learn(): n_entries >= train_start
            self.n_steps_default = 1                             # train_model() makes one update
            self.sync_target = True                              # learn(): update_target_model() after every trigger
        elif spec.family == "dqn":
            self.lr = float(getattr(brain, "learning_rate", 0.0005))
            self.gamma, self.batch, self.min_size = GAMMA, BATCH, MIN_SIZE
            self.n_steps_default = 5                             # DQN.py:143
            self.sync_target = True                              # DQN.py:83
        else:   # D3QN.py:54-72: the brain's own hyperparameters
            self.lr = float(getattr(brain, "learning_rate", 1e-3))
            self.gamma, self.batch = float(getattr(brain, "gamma", 0.99)), int(getattr(brain, "batch_size", 64))
            # random.sample needs `batch` rows (D3QN.py:98, 140): the only gate; np.random.choice (PERD3QN.py:165) needs one
            self.min_size = 0 if spec.family == "prioritized" else self.batch - 1
            self.exploration, self.soft_update_freq = int(getattr(brain, "exploration", 1000)), int(getattr(brain, "soft_update_freq", 200))
            self.n_steps_default = 1                             # D3QNAgent.train() makes one update
            self.sync_target = False                             # the schedule's (D3QN.py:125-126, Environment.learn_now)
        if spec.narrow:   # the wide learner's own batch: the gate stays the brain's (rows are drawn with replacement)
            self.batch = int(given[spec.keyword])
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8      # torch.optim.Adam's defaults (DQN.py:52, D3QN.py:61)
        self.ring = ring          # the brain's replay ring: a dict of device tensors as DeviceWorlds.enable_capture() makes them
        self.alpha = 0.6          # PERD3QN.py:134
        self.prio_e, self.prio_a, self.beta_increment = 0.01, 0.6, 0.001   # Memory.e, Memory.a, Memory.beta_increment_per_sampling
        self.p_new = float((torch.zeros(()) + self.prio_e) ** self.prio_a)  # append_sample's priority: float32 (0 + e) ** a, as torch makes it
        # the side struct's tensors (SIDE_TENSORS): prioritized=True the memory's priorities, their maximum and the draw's scratch;
        # rollout=True the window's bookkeeping; td_priority=True the memory's priorities and beta_is (Memory.beta, a device double)
        self.priority = self.weight = self.keys = self.prio_max = self.seen = self.fresh = self.beta_is = None
        self.is_weight = None     # optional device float32 [n_steps, batch]: rl_learn_td's importance weights (tests, diagnostics)
        self.trained_from = False  # td_priority=True: the ring has reached train_start (Environment.learn_now reads it back until then)
        if spec.side and ring is not None:
            self._make_side()
        # a wide entry's scratch (header, the tiles' partial gradients and sums, rl_learn_dueling_wide's per-row stash); needs no initialisation
        self.work = torch.empty(int(getattr(lib, spec.work_bytes)(self.kind, self.batch)), dtype=torch.uint8, device=self.device) if spec.narrow else None
        self.rank_order = self.rank_work = None   # DeviceWorlds.draw_slots_rank: the ring's slots in key order, and rl_learn_draw_rank's scratch
        self.rank_cum = None      # DeviceWorlds.draw_prioritized_rank / draw_td_rank: the weights' cumulative sum in key order (float64)
        self.loss = None          # optional device float32 [n_steps]
        self.grad = None          # optional device float32 [n_steps, n_params] (tests, diagnostics)

    def struct(self, sync_target=None):
        """rl_learner.  sync_target: this call's flag instead of the learner's own (DeviceWorlds.merge_learners)."""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return _lib.Learner(self.kind, p(self.params), p(self.target), p(self.adam_m), p(self.adam_v), p(self.state), p(self.packed),
                            self.lr, self.gamma, self.beta1, self.beta2, self.eps, self.batch, self.min_size,
                            int(self.sync_target if sync_target is None else sync_target),
                            p(self.loss), p(self.grad))

    def ring_struct(self):
        r = self.ring
        if r is None:
            raise _lib.ReinLifeHipError("this DeviceLearner has no replay ring (DeviceLearner.ring)")
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return _lib.Replay(*[p(r.get(n)) for n in ("state", "state_prime", "action", "reward", "done", "prob", "age", "count")],
                           int(r["state"].shape[0]))

    def _make_side(self):
        """The memory beside the ring, sized to it -- rl_prio: no priorities yet, maximum 1.0, nothing seen; rl_tdprio: no priorities yet,
        nothing seen, beta 0.4; rl_ppo, the on-policy window's bookkeeping: nothing seen, no fresh rows."""
        capacity = int(self.ring["state"].shape[0])
        for name in self.spec.side_tensors:
            per_row, dtype, fresh = SIDE_TENSORS[name]
            setattr(self, name, torch.full((capacity if per_row else 1,), fresh, dtype=dtype, device=self.device))

    _make_prio = _make_td = _make_ppo = _make_side   # (one implementation; the names it had per struct)

    def side_struct(self, kind, gate=True):
        """The struct of type `kind` that this learner's entry point takes beside the rings (Entry.side), its tensors made or re-made
        to the ring's size."""
        if self.spec.side is not kind:
            raise _lib.ReinLifeHipError({_lib.Prio: "this DeviceLearner has no prioritised memory (DeviceLearner(..., prioritized=True))",
                                         _lib.TdPrio: "this DeviceLearner has no PERDQN memory (DeviceLearner(..., td_priority=True))",
                                         _lib.Ppo: "this DeviceLearner is no PPO learner (DeviceLearner(..., rollout=True))"}[kind])
        if self.ring is None:
            raise _lib.ReinLifeHipError("this DeviceLearner has no replay ring (DeviceLearner.ring)")
        capacity = self.ring["state"].shape[0]
        tensors = [(getattr(self, n), SIDE_TENSORS[n][0]) for n in self.spec.side_tensors]
        if any(t is None or (per_row and t.numel() != capacity) for t, per_row in tensors):
            self._make_side()
        # a field is the learner attribute of its name (rl_tdprio's beta: beta_is); gate=False leaves rl_ppo's `fresh` out
        field = lambda n: None if n == "fresh" and not gate else getattr(self, "beta_is" if n == "beta" else n)  # noqa: E731
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return kind(*[p(field(n)) if ctype is C.c_void_p else field(n) for n, ctype in kind._fields_])

    def prio_struct(self):
        return self.side_struct(_lib.Prio)

    def td_struct(self):
        return self.side_struct(_lib.TdPrio)

    def ppo_struct(self, gate=True):
        """rl_ppo.  gate=False leaves `fresh` out: rl_learn_ppo then trains on the slots it is given whatever the last rollout's window held."""
        return self.side_struct(_lib.Ppo, gate=gate)

    @property
    def steps(self):
        """Adam steps taken so far (reads the device counter: synchronises)."""
        return int(self.state[0].item())

    def _load(self, module, flat):
        off = 0
        with torch.no_grad():
            for t in module.state_dict().values():
                n = t.numel()
                t.copy_(torch.from_numpy(flat[off:off + n].reshape(tuple(t.shape))))
                off += n
        assert off == flat.size

    def sync_to_module(self):
        """The trained parameters into brain.agent and the target network's into brain.target (made on first use: a copy, no
        generator draw), so that Saver and state_dict() see them.  D3QN and PERD3QN: into brain.eval_net and brain.target_net; PERDQN: into
        brain.model and brain.target_model."""
        module, target = MODULES[self.spec.family]   # (PPO.py:46: one module, no target; PERDQNAgent: Saver reads model)
        self._load(getattr(self.brain, module), self.params.cpu().numpy())
        if target is None:
            return
        if getattr(self.brain, target, None) is None:
            setattr(self.brain, target, copy.deepcopy(getattr(self.brain, module)))
        self._load(getattr(self.brain, target), self.target.cpu().numpy())


def philox_slots(seed, brain_index, calls, n_steps, batch, size):
    """The ring slots rl_learn draws when it is given none: word 0 of rl_philox(seed, 0, brain_index, calls, RL_SITE_LEARN, s * batch + j)
    mapped to [0, size) by ((uint64)x * size) >> 32 -> int32 [n_steps, batch]."""
    lib = _lib.lib()
    out = (C.c_uint32 * 4)()
    slots = np.zeros((n_steps, batch), np.int32)
    for s in range(n_steps):
        for j in range(batch):
            lib.rl_philox(seed, 0, brain_index, calls & 0xffffffff, _lib.SITE_LEARN, s * batch + j, C.byref(out))
            slots[s, j] = (int(out[0]) * int(size)) >> 32
    return slots
