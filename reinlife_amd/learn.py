"""DeviceLearner: what a DQN (also on wide minibatches: wide_batch=, rl_learn_wide), D3QN (also on wide minibatches: dueling_batch=, rl_learn_dueling_wide), (prioritized=True) PERD3QN, (rollout=True) PPO or (td_priority=True) PERDQN brain needs to learn on
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
rows not drawn go unused.

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
update made, not once per agent trigger -- a smaller explore_step restores the reference's rate in wall-clock terms."""
import copy
import ctypes as C

import numpy as np
import torch

from . import _lib

GAMMA, BATCH, MIN_SIZE, BUFFER_LIMIT = 0.98, 32, 1000, 50_000   # DQN.py:14-16, 81
ENTRY_BY_METHOD = {"DQN": "rl_learn", "D3QN": "rl_learn_dueling"}   # the brain kinds an entry point trains (Environment's learn_kinds)


def entry_of(kind):
    """The name of the C entry point that trains brains of `kind`, or None."""
    lib = _lib.lib()
    return "rl_learn" if lib.rl_learn_supported(kind) else "rl_learn_dueling" if lib.rl_learn_dueling_supported(kind) else None


class DeviceLearner:
    def __init__(self, brain, device="cuda:0", ring=None, prioritized=False, rollout=False, td_priority=False, prioritized_batch=None, wide_batch=None, dueling_batch=None):
        lib = _lib.lib()
        if prioritized_batch is not None:   # an explicit opt-in on top of prioritized=True: the prioritised learner on wide minibatches
            other = (" with wide_batch" if wide_batch is not None else " with dueling_batch" if dueling_batch is not None else " with rollout=True" if rollout
                     else " with td_priority=True" if td_priority else "" if prioritized else " without prioritized=True")
            if other or not lib.rl_learn_prioritized_wide_supported(brain.kind):
                raise ValueError("prioritized_batch is for PERD3QN brains with prioritized=True (rl_learn_prioritized_wide); got a %s brain (kind %d)%s"
                                 % (brain.method, brain.kind, other))
            if (isinstance(prioritized_batch, bool) or not isinstance(prioritized_batch, (int, np.integer))
                    or not 1 <= prioritized_batch <= _lib.LEARN_PRIORITIZED_WIDE_MAX):
                raise ValueError("prioritized_batch must be an int in [1, %d] (the rows of a minibatch of rl_learn_prioritized_wide), got %r"
                                 % (_lib.LEARN_PRIORITIZED_WIDE_MAX, prioritized_batch))
            self.entry = "rl_learn_prioritized_wide"
        elif dueling_batch is not None:   # an explicit opt-in, like the four below: entry_of() and ENTRY_BY_METHOD keep answering what they answered
            other = (" with wide_batch" if wide_batch is not None else " with prioritized=True" if prioritized else " with rollout=True" if rollout
                     else " with td_priority=True" if td_priority else "")
            if other or not lib.rl_learn_dueling_wide_supported(brain.kind):
                raise ValueError("dueling_batch is for D3QN brains (rl_learn_dueling_wide); got a %s brain (kind %d)%s" % (brain.method, brain.kind, other))
            if isinstance(dueling_batch, bool) or not isinstance(dueling_batch, (int, np.integer)) or not 1 <= dueling_batch <= _lib.LEARN_DUELING_WIDE_MAX:
                raise ValueError("dueling_batch must be an int in [1, %d] (the rows of a minibatch of rl_learn_dueling_wide), got %r"
                                 % (_lib.LEARN_DUELING_WIDE_MAX, dueling_batch))
            self.entry = "rl_learn_dueling_wide"
        elif wide_batch is not None:   # an explicit opt-in, like the three below: entry_of() and ENTRY_BY_METHOD keep answering what they answered
            other = " with prioritized=True" if prioritized else " with rollout=True" if rollout else " with td_priority=True" if td_priority else ""
            if other or not lib.rl_learn_wide_supported(brain.kind):
                raise ValueError("wide_batch is for DQN brains (rl_learn_wide); got a %s brain (kind %d)%s" % (brain.method, brain.kind, other))
            if isinstance(wide_batch, bool) or not isinstance(wide_batch, (int, np.integer)) or not 1 <= wide_batch <= _lib.LEARN_WIDE_MAX:
                raise ValueError("wide_batch must be an int in [1, %d] (the rows of a minibatch of rl_learn_wide), got %r" % (_lib.LEARN_WIDE_MAX, wide_batch))
            self.entry = "rl_learn_wide"
        elif td_priority:   # an explicit opt-in, like prioritized and rollout: entry_of() and ENTRY_BY_METHOD keep answering what they answered
            if prioritized or rollout or not lib.rl_learn_td_supported(brain.kind):
                raise ValueError("td_priority=True is for PERDQN brains (rl_learn_td); got a %s brain (kind %d)%s"
                                 % (brain.method, brain.kind, " with prioritized=True" if prioritized else " with rollout=True" if rollout else ""))
            self.entry = "rl_learn_td"
        elif rollout:   # an explicit opt-in, like prioritized: entry_of() and ENTRY_BY_METHOD keep answering what they answered
            if prioritized or not lib.rl_learn_ppo_supported(brain.kind):
                raise ValueError("rollout=True is for PPO brains (rl_learn_ppo); got a %s brain (kind %d)%s"
                                 % (brain.method, brain.kind, " with prioritized=True" if prioritized else ""))
            self.entry = "rl_learn_ppo"
        elif prioritized:   # an explicit opt-in: entry_of() and ENTRY_BY_METHOD keep answering what they answered
            if not lib.rl_learn_prioritized_supported(brain.kind):
                raise ValueError("prioritized=True is for PERD3QN brains (rl_learn_prioritized); got a %s brain (kind %d)" % (brain.method, brain.kind))
            self.entry = "rl_learn_prioritized"
        else:
            self.entry = entry_of(brain.kind)
        if self.entry is None:
            raise ValueError("no entry point trains %s brains (kind %d): only DQN (rl_learn) and D3QN (rl_learn_dueling) learn on the device"
                             % (brain.method, brain.kind))
        from .worlds import pack_brain_weights
        self.brain, self.kind, self.device = brain, brain.kind, torch.device(device)
        flat = brain.state_dict_flat()
        self.n_params = int(lib.rl_policy_n_params(self.kind))
        self.merge_floats = int(lib.rl_learn_merge_floats(self.kind))   # this learner's segment of an exported row: params | adam_m | adam_v | step count
        self.params = torch.as_tensor(flat, device=self.device)
        self.target = None if rollout else self.params.clone()  # DQN.py:50 / D3QN.py:60 (PPO has no target network)
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)   # [Adam steps taken, rl_learn calls made]
        self.packed = pack_brain_weights(self.kind, flat, self.device)
        self.train_freq = int(getattr(brain, "train_freq", 20))
        if self.entry == "rl_learn_ppo":   # PPO.py:42-43: the brain's own hyperparameters
            self.lr, self.gamma = float(getattr(brain, "learning_rate", 0.0005)), float(getattr(brain, "gamma", 0.98))
            self.lmbda, self.eps_clip, self.k_epoch = float(getattr(brain, "lmbda", 0.95)), float(getattr(brain, "eps_clip", 0.1)), int(getattr(brain, "k_epoch", 3))
            self.batch, self.min_size = _lib.PPO_ROLLOUT_MAX, 0  # the rows of a rollout; no size gate (an empty window makes no update)
            self.n_steps_default = 1                             # one PPO.learn() per call
            self.sync_target = False
        elif self.entry == "rl_learn_td":   # PERDQNAgent.__init__: the brain's own hyperparameters
            self.lr, self.gamma = float(getattr(brain, "learning_rate", 1e-3)), float(getattr(brain, "discount_factor", 0.99))
            self.batch = int(getattr(brain, "batch_size", 64))
            self.train_start, self.memory_size = int(getattr(brain, "train_start", 1000)), int(getattr(brain, "memory_size", 20000))
            self.min_size = self.train_start - 1                 # learn(): n_entries >= train_start
            self.n_steps_default = 1                             # train_model() makes one update
            self.sync_target = True                              # learn(): update_target_model() after every trigger
        elif self.entry in ("rl_learn", "rl_learn_wide"):   # the wide learner is the DQN learner with its own batch
            self.lr = float(getattr(brain, "learning_rate", 0.0005))
            self.gamma, self.batch, self.min_size = GAMMA, BATCH if wide_batch is None else int(wide_batch), MIN_SIZE
            self.n_steps_default = 5                             # DQN.py:143
            self.sync_target = True                              # DQN.py:83
        else:   # D3QN.py:54-72: the brain's own hyperparameters
            self.lr = float(getattr(brain, "learning_rate", 1e-3))
            self.gamma, self.batch = float(getattr(brain, "gamma", 0.99)), int(getattr(brain, "batch_size", 64))
            # random.sample needs `batch` rows (D3QN.py:98, 140): the only gate; np.random.choice (PERD3QN.py:165) needs one
            self.min_size = 0 if prioritized else self.batch - 1
            if dueling_batch is not None:   # the wide learner is the D3QN learner with its own batch: the gate stays the brain's (rows are drawn with replacement)
                self.batch = int(dueling_batch)
            if prioritized_batch is not None:   # likewise the prioritised learner: np.random.choice's gate (one row) stays
                self.batch = int(prioritized_batch)
            self.exploration, self.soft_update_freq = int(getattr(brain, "exploration", 1000)), int(getattr(brain, "soft_update_freq", 200))
            self.n_steps_default = 1                             # D3QNAgent.train() makes one update
            self.sync_target = False                             # the schedule's (D3QN.py:125-126, Environment.learn_now)
        self.beta1, self.beta2, self.eps = 0.9, 0.999, 1e-8      # torch.optim.Adam's defaults (DQN.py:52, D3QN.py:61)
        self.ring = ring          # the brain's replay ring: a dict of device tensors as DeviceWorlds.enable_capture() makes them
        self.alpha = 0.6          # PERD3QN.py:134
        self.priority = self.weight = self.keys = self.prio_max = self.seen = None
        if prioritized and ring is not None:
            self._make_prio()
        self.fresh = None         # rollout=True: the window's bookkeeping (seen and keys above, fresh here)
        if rollout and ring is not None:
            self._make_ppo()
        self.prio_e, self.prio_a, self.beta_increment = 0.01, 0.6, 0.001   # Memory.e, Memory.a, Memory.beta_increment_per_sampling
        self.p_new = float((torch.zeros(()) + self.prio_e) ** self.prio_a)  # append_sample's priority: float32 (0 + e) ** a, as torch makes it
        self.beta_is = None       # td_priority=True: Memory.beta, a device double
        self.is_weight = None     # optional device float32 [n_steps, batch]: rl_learn_td's importance weights (tests, diagnostics)
        self.trained_from = False  # td_priority=True: the ring has reached train_start (Environment.learn_now reads it back until then)
        if td_priority and ring is not None:
            self._make_td()
        self.work = None          # wide_batch: rl_learn_wide's scratch (header, the tiles' partial gradients and loss sums); needs no initialisation
        if self.entry == "rl_learn_wide":
            self.work = torch.empty(int(lib.rl_learn_wide_work_bytes(self.kind, self.batch)), dtype=torch.uint8, device=self.device)
        if self.entry == "rl_learn_dueling_wide":   # dueling_batch: rl_learn_dueling_wide's scratch (header, partial gradients, advantage sums, per-row stash)
            self.work = torch.empty(int(lib.rl_learn_dueling_wide_work_bytes(self.kind, self.batch)), dtype=torch.uint8, device=self.device)
        if self.entry == "rl_learn_prioritized_wide":   # prioritized_batch: rl_learn_prioritized_wide's scratch (rl_learn_dueling_wide's layout)
            self.work = torch.empty(int(lib.rl_learn_prioritized_wide_work_bytes(self.kind, self.batch)), dtype=torch.uint8, device=self.device)
        self.rank_order = self.rank_work = None   # DeviceWorlds.draw_slots_rank: the ring's slots in key order, and rl_learn_draw_rank's scratch
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

    def _make_prio(self):
        """The prioritised memory beside the ring (rl_prio), sized to it: no priorities yet, maximum 1.0 (PERD3QN.py:147), nothing seen."""
        capacity = int(self.ring["state"].shape[0])
        self.priority = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.keys = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self.prio_max = torch.ones(1, dtype=torch.float32, device=self.device)
        self.seen = torch.zeros(1, dtype=torch.int64, device=self.device)

    def prio_struct(self):
        if self.entry not in ("rl_learn_prioritized", "rl_learn_prioritized_wide"):
            raise _lib.ReinLifeHipError("this DeviceLearner has no prioritised memory (DeviceLearner(..., prioritized=True))")
        if self.ring is None:
            raise _lib.ReinLifeHipError("this DeviceLearner has no replay ring (DeviceLearner.ring)")
        if self.priority is None or self.priority.numel() != self.ring["state"].shape[0]:
            self._make_prio()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        return _lib.Prio(p(self.priority), p(self.weight), p(self.keys), p(self.prio_max), p(self.seen), self.alpha)

    def _make_td(self):
        """The PERDQN memory beside the ring (rl_tdprio), sized to it: no priorities yet, nothing seen, beta 0.4 (Memory.beta)."""
        capacity = int(self.ring["state"].shape[0])
        self.priority = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.keys = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self.seen = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.beta_is = torch.full((1,), 0.4, dtype=torch.float64, device=self.device)

    def td_struct(self):
        if self.entry != "rl_learn_td":
            raise _lib.ReinLifeHipError("this DeviceLearner has no PERDQN memory (DeviceLearner(..., td_priority=True))")
        if self.ring is None:
            raise _lib.ReinLifeHipError("this DeviceLearner has no replay ring (DeviceLearner.ring)")
        if self.priority is None or self.priority.numel() != self.ring["state"].shape[0]:
            self._make_td()
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return _lib.TdPrio(p(self.priority), p(self.keys), p(self.seen), p(self.beta_is), self.p_new, self.prio_e, self.prio_a,
                           self.beta_increment, p(self.is_weight))

    def _make_ppo(self):
        """The on-policy window's bookkeeping beside the ring (rl_ppo), sized to it: nothing seen, no fresh rows."""
        capacity = int(self.ring["state"].shape[0])
        self.keys = torch.zeros(capacity, dtype=torch.int64, device=self.device)
        self.seen = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.fresh = torch.zeros(1, dtype=torch.int64, device=self.device)

    def ppo_struct(self, gate=True):
        """rl_ppo.  gate=False leaves `fresh` out: rl_learn_ppo then trains on the slots it is given whatever the last rollout's window held."""
        if self.entry != "rl_learn_ppo":
            raise _lib.ReinLifeHipError("this DeviceLearner is no PPO learner (DeviceLearner(..., rollout=True))")
        if self.ring is None:
            raise _lib.ReinLifeHipError("this DeviceLearner has no replay ring (DeviceLearner.ring)")
        if self.fresh is None or self.keys.numel() != self.ring["state"].shape[0]:
            self._make_ppo()
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        return _lib.Ppo(self.lmbda, self.eps_clip, self.k_epoch, p(self.seen), p(self.fresh) if gate else None, p(self.keys))

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
        if self.entry == "rl_learn_ppo":   # PPO.py:46: one module, no target
            self._load(self.brain.model, self.params.cpu().numpy())
            return
        if self.entry == "rl_learn_td":    # PERDQNAgent: model and target_model (Saver reads model)
            self._load(self.brain.model, self.params.cpu().numpy())
            self._load(self.brain.target_model, self.target.cpu().numpy())
            return
        if self.entry in ("rl_learn_dueling", "rl_learn_prioritized", "rl_learn_dueling_wide", "rl_learn_prioritized_wide"):
            self._load(self.brain.eval_net, self.params.cpu().numpy())
            self._load(self.brain.target_net, self.target.cpu().numpy())
            return
        self._load(self.brain.agent, self.params.cpu().numpy())
        if getattr(self.brain, "target", None) is None:
            self.brain.target = copy.deepcopy(self.brain.agent)
        self._load(self.brain.target, self.target.cpu().numpy())


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
