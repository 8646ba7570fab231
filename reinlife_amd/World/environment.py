"""Environment: the reference's protocol (ReinLife/World/environment.py:16-215) over the HIP world kernels.

Same constructor keywords, `reset() / step() / update_env(n_epi)`, `agents` (row-major list), `brains`, `max_gene`,
`action_space = 8`, `observation_space = 153`.  Extras (keyword-only): `n_worlds` independent replicas on the device,
`device`, `seed`.  `env.agents` are lightweight views of world 0, built from the device state when they are first read after a change (a loop
that never reads them never synchronises); the batched fast paths are `env.act(n_epi)` (Agent.get_action for every agent of every
world on the GPU) and `env.run(n_epi, n_ticks)` (whole chunks of the trainer loop in one launch each).

Random numbers.  `rng="reference"` (the default for a single world) makes the SAME draws from Python's `random`,
`np.random` and torch's global generator, in the same order and with the same arguments, as the reference's
reset() / step() / update_env() (environment.py:133-158, 488-547, 741-776; grid.py:69-83): seed the three generators as
you would for the reference and the world follows the reference's trajectory bit for bit (tests/test_hip_seed_compat.py
replays the golden traces from their seeds alone).  The draws of _add_food depend on the grid after movement, so a step
is two launches (rl_step_split -> host draws -> rl_step_food).  `rng="philox"` (the default and only choice for
n_worlds > 1) draws inside the kernels from counter-based Philox streams keyed by `seed`.  The Tracker's statistics are accumulated in the step kernel (Helpers/tracker.py); Saver and a headless painter (Helpers/render.py) mirror the reference's; pygame windows are out of scope.
"""
import os

import numpy as np
import torch

from .. import _lib
from ..learn import ALL_ENTRIES as ENTRIES, BUFFER_LIMIT, ENTRY, ENTRY_BY_METHOD, FAMILIES, DeviceLearner, entry_of
from ..worlds import DeviceWorlds
from .utils import Actions, EntityTypes


_A_FIELDS = tuple(n for n in _lib.STATE_FIELDS if n.startswith("a_"))


class _WorldMirror:
    """Host copy of ONE world's agent list and per-agent outputs, in env.agents order.  Built on first use after a step() /
    update_env() / run() (Environment._mat): a loop that never looks at env.agents never pays for it.  The small arrays come with
    the state snapshot; the observation rows (Agent.state / state_prime: 612 B per agent) are fetched only when somebody reads them."""

    def __init__(self, env, world, phase):
        self.env, self.world, self.phase = env, world, phase
        self.stamp = env._stamp     # the device state this mirror describes (Environment._refresh moves on)
        self.n = 0
        self.host = None            # {"a_i": ..., ...}
        self._state = None          # [n,153] float64: Agent.state
        self._state_prime = None    # [n,153] or None (between update_env and the next step)
        self.reward = self.done = self.src1 = None
        self.actions = None         # [cap] int8
        self.q = None               # [cap,8] float32: the policy's outputs for this tick (Environment.act, rng="reference")
        self.dirty = False          # actions were set through AgentView.action and are not on the device yet
        self.views = None           # the AgentView list handed out by agents_of()

    def _rows(self, t):
        if self.stamp != self.env._stamp:
            raise RuntimeError("this AgentView describes an earlier tick: Agent.state / state_prime must be read before the next "
                               "step() / update_env() / run() (take env.agents again)")
        return t.cpu().numpy().astype(np.float64)

    @property
    def state(self):
        if self._state is None:
            w, n = self.env.worlds, self.n
            if self.phase == "step":   # Agent.state is still the observation the policy read, in the pre-step order
                self._state = self._rows(w.obs_state()[self.world])[self.src1[:n].astype(np.int64)]
            else:
                self._state = self._rows(w.obs_state()[self.world, :n])
        return self._state

    @property
    def state_prime(self):
        if self._state_prime is None and self.phase == "step":
            self._state_prime = self._rows(self.env.worlds.obs_state_prime()[self.world, :self.n])
        return self._state_prime


class AgentView:
    """One entry of env.agents / env.agents_of(world): the reference's Agent attributes (entities.py:131-170) read from the
    device state of that world."""

    def __init__(self, env, k, mirror=None):
        self._env, self._k = env, k
        self._m = mirror if mirror is not None else env._mat(0)
        self.prob = None
        self.info = ""

    def _f(self, name):
        return self._m.host["a_" + name][self._k]

    i = property(lambda s: int(s._f("i")))
    j = property(lambda s: int(s._f("j")))
    coordinates = property(lambda s: [s.i, s.j])
    health = property(lambda s: int(s._f("health")))
    max_health = 200
    age = property(lambda s: int(s._f("age")))
    max_age = property(lambda s: int(s._f("max_age")))
    gene = property(lambda s: int(s._f("gene")))
    fitness = property(lambda s: float(s._f("fitness")))
    dead = property(lambda s: bool(s._f("flags") & _lib.F_DEAD))
    reproduced = property(lambda s: bool(s._f("flags") & _lib.F_REPRODUCED))
    killed = property(lambda s: int(bool(s._f("flags") & _lib.F_KILLED)))
    ate_super_food = property(lambda s: 1.0 if s._f("flags") & _lib.F_ATE_SUPER else -1)
    brain = property(lambda s: s._env.brains[int(s._f("brain"))])
    entity_type = EntityTypes.agent

    @property
    def action(self):
        if self._m.actions is None:   # act() ran after this view was built: the policy's choice is fetched on first use
            self._env._mat(self._m.world)
        return int(self._m.actions[self._k])

    @action.setter
    def action(self, a):
        if self._m.actions is None:
            self._env._mat(self._m.world)
        self._m.actions[self._k] = int(a)
        self._m.dirty = True

    @property
    def state(self):
        return self._m.state[self._k]

    @property
    def state_prime(self):
        return self._m.state_prime[self._k] if self._m.state_prime is not None else self.state

    @property
    def reward(self):
        return float(self._m.reward[self._k]) if self._m.reward is not None else None

    @property
    def done(self):
        return bool(self._m.done[self._k]) if self._m.done is not None else False

    def get_action(self, n_epi, out=None):  # entities.py:215-222
        b = self.brain
        state = self.state if out is None else None   # (with the outputs at hand the brain does not look at the row: no fetch)
        if b.method == "PPO":
            r = b.get_action(state, out=out)
            self.action, self.prob = r if isinstance(r, tuple) else (r, None)
        elif b.method == "PERDQN":   # (its get_action takes no n_epi: entities.py:219-220)
            self.action = b.get_action(state, out=out)
        else:
            self.action = b.get_action(state, n_epi, out=out)

    def learn(self, **kwargs):
        """entities.py:194-208: the keyword set the reference hands to brain.learn, per brain method (caller kwargs such as
        n_epi only reach the brains the reference forwards them to).  The brains of this build ignore learn() (training is
        outside its scope); a subclass that overrides learn() receives the reference's arguments."""
        if self.age > 1:
            common = dict(age=self.age, dead=self.dead, action=self.action, state=self.state, reward=self.reward,
                          state_prime=self.state_prime, done=self.done)
            method = self.brain.method
            if method == "PPO":
                self.brain.learn(prob=self.prob, **common)
            elif method in ("DQN", "A2C", "PERDQN"):
                self.brain.learn(**common)
            else:  # DRQN, D3QN, PERD3QN, ...
                self.brain.learn(**common, **kwargs)


class Environment:
    _DRAW_KINDS = ("DQN", "D3QN", "PERD3QN", "PERDQN")   # the keys of learn_draw as a dict: the brain methods whose draw has a rank variant
    _DRAW_FAMILY = {"dqn": "DQN", "dueling": "D3QN", "prioritized": "PERD3QN", "td": "PERDQN"}   # ... per family of learn.FAMILIES
    log_reference_calls = False   # learn="reference": keep every Call in self.reference_calls (a class attribute: trainer() builds its own environment)

    def __init__(self, width=30, height=30, brains=None, grid_size=16, max_agents=50, update_interval=500, print_results=True,
                 static_families=True, interactive_results=False, google_colab=False, training=True, save=False,
                 pastel_colors=False, limit_reproduction=False, incentivize_killing=True, *, n_worlds=1, device=None,
                 seed=0, rng=None, synthetic_agents=None, refill_below=None, dist=None, world_base=None, learn=None, learn_every=None,
                 learn_steps=5, learn_kinds=None, learn_prioritized=None, learn_rollout=None, rollout_steps=1,
                 learn_td_priority=None, learn_td_stamp=None, learn_ranks=None, learn_reference_prioritized=None,
                 learn_reference_td=None, learn_batch=None, learn_draw=None):
        if not brains:
            raise ValueError("Environment needs a non-empty list of brains")
        if learn not in (None, "device", "reference"):
            raise ValueError("learn must be None (the brains stay as they are), 'device' (DQN brains train through rl_learn) or 'reference' (one world, "
                             "the reference's own schedule and draws: DQN, D3QN and PPO brains train), got %r" % (learn,))
        # learn_kinds: the brain methods that train under learn="device".  None = ("DQN",): what learn="device" always did; "D3QN" is an
        # explicit opt-in (rl_learn_dueling).  Checked here, before a device is touched.
        if learn_kinds is not None and learn != "device":
            raise ValueError("learn_kinds needs learn='device' (got learn=%r)" % (learn,))
        self.learn_kinds = ("DQN",) if learn_kinds is None else ((learn_kinds,) if isinstance(learn_kinds, str) else tuple(learn_kinds))
        unknown = [k for k in self.learn_kinds if k not in ENTRY_BY_METHOD]
        if unknown or not self.learn_kinds:
            raise ValueError("learn_kinds: no entry point trains %s brains; the kinds that learn on the device are %s"
                             % (", ".join(map(str, unknown)) or "()", ", ".join(sorted(ENTRY_BY_METHOD))))
        # learn_prioritized=True: every PERD3QN brain trains through rl_learn_prioritized on a prioritised memory (PERD3QN.py:94-115,
        # 133-182).  A keyword of its own: learn_kinds and ENTRY_BY_METHOD answer what they answered.  Checked before a device is touched.
        self._opt_in("prioritized", learn_prioritized, learn, brains)
        # learn_reference_prioritized=True: under learn="reference" every PERD3QN brain trains too -- its priorities stay on the device, the
        # host draws np.random.choice's uniforms (rl_learn_prioritized_store_ref, rl_learn_prioritized_choice, then rl_learn_prioritized).
        # A keyword of its own: without it learn="reference" is what it was.  Checked before a device is touched.
        if learn_reference_prioritized not in (None, True):
            raise ValueError("learn_reference_prioritized must be None or True, got %r" % (learn_reference_prioritized,))
        if learn_reference_prioritized and learn != "reference":
            raise ValueError("learn_reference_prioritized=True needs learn='reference' (got learn=%r)" % (learn,))
        if learn_reference_prioritized and not any(getattr(b, "method", None) == "PERD3QN" for b in brains):
            raise ValueError("learn_reference_prioritized=True needs at least one Models.PERD3QN brain (got %s)"
                             % ", ".join(str(getattr(b, "method", b)) for b in brains))
        self.learn_reference_prioritized = bool(learn_reference_prioritized)
        # learn_reference_td=True: under learn="reference" every PERDQN brain trains too -- its sum tree stays on the device in float64 with
        # the reference's rounding order, the host draws Memory.sample's uniforms (rl_learn_td_tree_store, rl_learn_td_tree_sample,
        # rl_learn_td, rl_learn_td_tree_update).  A keyword of its own: learn_reference_prioritized=True leaves PERDQN brains frozen, as it
        # did.  Checked before a device is touched.
        if learn_reference_td not in (None, True):
            raise ValueError("learn_reference_td must be None or True, got %r" % (learn_reference_td,))
        if learn_reference_td and learn != "reference":
            raise ValueError("learn_reference_td=True needs learn='reference' (got learn=%r)" % (learn,))
        if learn_reference_td and not any(getattr(b, "method", None) == "PERDQN" for b in brains):
            raise ValueError("learn_reference_td=True needs at least one Models.PERDQN brain (got %s)"
                             % ", ".join(str(getattr(b, "method", b)) for b in brains))
        if learn_reference_td:
            small = [int(b.memory_size) for b in brains if getattr(b, "method", None) == "PERDQN" and int(b.memory_size) < 2]
            if small:
                raise ValueError("learn_reference_td=True: a PERDQN memory needs a capacity of at least 2 (got %d): the reference's "
                                 "SumTree._propagate never ends for a tree of one leaf" % small[0])
        self.learn_reference_td = bool(learn_reference_td)
        # learn_rollout=True: every PPO brain trains through rl_learn_ppo on rollouts drawn from the rows its current weights made
        # (PPO.py:71-77, 136-162).  A keyword of its own, like learn_prioritized.  Checked before a device is touched.
        self._opt_in("rollout", learn_rollout, learn, brains)
        if rollout_steps != 1 and not learn_rollout:
            raise ValueError("rollout_steps needs learn_rollout=True")
        if int(rollout_steps) < 1:
            raise ValueError("rollout_steps must be >= 1 (got %r)" % (rollout_steps,))
        self.rollout_steps = int(rollout_steps)
        # learn_td_priority=True: every PERDQN brain trains through rl_learn_td on the reference's prioritised memory with importance
        # weights (PERDQN.py: train_model, Memory).  A keyword of its own, like learn_prioritized.  Checked before a device is touched.
        self._opt_in("td_priority", learn_td_priority, learn, brains)
        # learn_td_stamp="error": every learning call queues one rl_learn_td_stamp in front of the PERDQN draw -- the rows appended since
        # the last draw get the TD-error priority append_sample spells out, not its constant (this build's own; PERDQN.py:113-128).  It
        # rides on learn_td_priority=True, which has made sure of learn="device" and a Models.PERDQN.  Checked before a device is touched.
        if learn_td_stamp not in (None, "error"):
            raise ValueError("learn_td_stamp must be None (fresh PERDQN rows get the reference's constant (0 + e) ** a) or 'error' (they get "
                             "their TD error's priority, rl_learn_td_stamp), got %r" % (learn_td_stamp,))
        if learn_td_stamp and not self.learn_td_priority:
            raise ValueError("learn_td_stamp=%r needs learn_td_priority=True (it stamps the PERDQN learners' memories; with it learn='device' "
                             "and at least one Models.PERDQN)" % (learn_td_stamp,))
        self.learn_td_stamp = learn_td_stamp
        # learn_batch=B: every DQN learner trains through rl_learn_wide on minibatches of B rows (1 .. 2048) in 32-row tiles side by side
        # (this build's own: the reference's minibatch is 32, DQN.py:16).  None: rl_learn, as always.  Checked before a device is touched.
        # A dict by kind, like learn_steps: {"DQN": B}, {"D3QN": B} or both -- "D3QN": every D3QN learner trains through rl_learn_dueling_wide
        # on minibatches of B rows in 64-row tiles, the advantage mean taken over the whole batch (the reference's minibatch is 64, D3QN.py:98).
        # With learn_prioritized=True the dict also takes "PERD3QN": every PERD3QN learner trains through rl_learn_prioritized_wide on
        # minibatches of B rows (the prioritised draw at that width, the priorities of all B rows written); without it the key stays unknown.
        # With learn_rollout=True the dict also takes "PPO": every PPO learner trains through rl_learn_ppo_wide on rollouts of B rows (1 ..
        # 2048) in 32-row tiles, ONE GAE recursion over the whole rollout (the on-policy draw at that width); without it the key stays unknown.
        # With learn_td_priority=True the dict also takes "PERDQN": every PERDQN learner trains through rl_learn_td_wide on minibatches of B
        # rows (1 .. 2048) in 64-row tiles, the importance weights' minimum and mean taken over the whole batch (the reference's minibatch
        # is 64, PERDQN.py); without it the key stays unknown.
        wide = {e.method: e for e in ENTRIES if e.narrow}   # the wide entry per brain method, a key of the dict only where its narrow entry is on
        self.learn_batch_of = dict.fromkeys(wide)
        if isinstance(learn_batch, dict):
            on = {k: e for k, e in wide.items() if not ENTRY[e.narrow].keyword or getattr(self, "learn_" + ENTRY[e.narrow].keyword)}
            unknown = [k for k in learn_batch if k not in on]
            if unknown or not learn_batch:
                raise ValueError("learn_batch as a dict takes the keys 'DQN' (rl_learn_wide) and 'D3QN' (rl_learn_dueling_wide)%s and at least one of them, got %r"
                                 % ((" and, with learn_prioritized=True, 'PERD3QN' (rl_learn_prioritized_wide)," if self.learn_prioritized else "")
                                    + (" and, with learn_rollout=True, 'PPO' (rl_learn_ppo_wide)," if self.learn_rollout else "")
                                    + (" and, with learn_td_priority=True, 'PERDQN' (rl_learn_td_wide)," if self.learn_td_priority else ""), learn_batch))
            for k, v in learn_batch.items():
                limit = getattr(_lib, on[k].batch_max)
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= limit:
                    raise ValueError("learn_batch[%r] must be an int in [1, %d] (the rows of a %s minibatch, %s), got %r" % (k, limit, k, on[k].name, v))
            if learn != "device":
                raise ValueError("learn_batch needs learn='device' (got learn=%r)" % (learn,))
            for k in learn_batch:
                if ENTRY[on[k].narrow].keyword:   # (learn_prioritized=True has made sure of a Models.PERD3QN brain; learn_kinds does not name this kind)
                    continue
                if k not in self.learn_kinds or not any(getattr(b, "method", None) == k for b in brains):
                    raise ValueError("learn_batch names %s: it needs at least one Models.%s brain among the learning kinds %r (got %s)"
                                     % (k, k, self.learn_kinds, ", ".join(str(getattr(b, "method", b)) for b in brains)))
            self.learn_batch_of.update({k: int(v) for k, v in learn_batch.items()})
        elif learn_batch is not None:   # an int is the DQN learners' batch
            limit = getattr(_lib, wide["DQN"].batch_max)
            if isinstance(learn_batch, bool) or not isinstance(learn_batch, (int, np.integer)) or not 1 <= learn_batch <= limit:
                raise ValueError("learn_batch must be None or an int in [1, %d] (the rows of a DQN minibatch, %s), got %r" % (limit, wide["DQN"].name, learn_batch))
            if learn != "device":
                raise ValueError("learn_batch needs learn='device' (got learn=%r)" % (learn,))
            if "DQN" not in self.learn_kinds or not any(getattr(b, "method", None) == "DQN" for b in brains):
                raise ValueError("learn_batch needs at least one Models.DQN brain among the learning kinds %r (got %s)"
                                 % (self.learn_kinds, ", ".join(str(getattr(b, "method", b)) for b in brains)))
            self.learn_batch_of["DQN"] = int(learn_batch)
        # (what the caller gave: the int it always was, None, or a plain dict copy; learn_batch_of is what the learners are built from)
        self.learn_batch = {k: int(v) for k, v in learn_batch.items()} if isinstance(learn_batch, dict) else None if learn_batch is None else int(learn_batch)
        # learn_draw="rank": the DQN, wide DQN and D3QN learners' minibatches are drawn by content-key rank (rl_learn_draw_rank: one sort
        # per call, one thread per draw) instead of rl_learn_draw's minimum over all keys per draw -- another uniform sampler, so other
        # rows: this build's own, an explicit opt-in.  None: rl_learn_draw, as always.  Checked before a device is touched.
        # A dict by kind, like learn_batch: {"DQN": "rank"}, {"D3QN": "rank"} (the string, for that kind alone) and, with their opt-ins,
        # {"PERD3QN": "rank"} -- the prioritised draw by prefix sum over content-key rank, independent draws (rl_learn_prioritized_draw_rank)
        # -- and {"PERDQN": "rank"} -- the same, stratified: the reference's Memory.sample() (rl_learn_td_draw_rank).  Every key must name
        # a kind that has a learner in this run.  The string keeps its meaning: the DQN and D3QN families only.
        self.learn_draw_of = dict.fromkeys(self._DRAW_KINDS)
        if isinstance(learn_draw, dict):
            if not learn_draw or any(k not in self._DRAW_KINDS or v != "rank" for k, v in learn_draw.items()):
                raise ValueError("learn_draw must be None (rl_learn_draw) or 'rank' (uniform draws by content-key rank, rl_learn_draw_rank), or a "
                                 "dict by kind with the keys %s, the value 'rank' and at least one of them, got %r"
                                 % (", ".join(repr(k) for k in self._DRAW_KINDS), learn_draw))
            if learn != "device":
                raise ValueError("learn_draw=%r needs learn='device' (got learn=%r)" % (learn_draw, learn))
            for k in learn_draw:
                opt_in = {"PERD3QN": "learn_prioritized", "PERDQN": "learn_td_priority"}.get(k)
                if opt_in:   # (the opt-in has made sure of a brain of the kind)
                    if not getattr(self, opt_in):
                        raise ValueError("learn_draw names %s: it needs %s=True (its learners are that keyword's)" % (k, opt_in))
                elif k not in self.learn_kinds or not any(getattr(b, "method", None) == k for b in brains):
                    raise ValueError("learn_draw names %s: it needs at least one Models.%s brain among the learning kinds %r (got %s)"
                                     % (k, k, self.learn_kinds, ", ".join(str(getattr(b, "method", b)) for b in brains)))
            learn_draw = dict(learn_draw)   # (the caller's dict stays the caller's)
            self.learn_draw_of.update(learn_draw)
        else:
            if learn_draw not in (None, "rank"):
                raise ValueError("learn_draw must be None (rl_learn_draw) or 'rank' (uniform draws by content-key rank, rl_learn_draw_rank), got %r" % (learn_draw,))
            if learn_draw and learn != "device":
                raise ValueError("learn_draw=%r needs learn='device' (got learn=%r)" % (learn_draw, learn))
            if learn_draw and not any(getattr(b, "method", None) in self.learn_kinds for b in brains):
                raise ValueError("learn_draw=%r needs at least one brain that rl_learn, rl_learn_wide or rl_learn_dueling trains: a brain of the "
                                 "learning kinds %r (got %s)" % (learn_draw, self.learn_kinds, ", ".join(str(getattr(b, "method", b)) for b in brains)))
            if learn_draw:
                self.learn_draw_of.update(DQN="rank", D3QN="rank")
        self.learn_draw = learn_draw
        # learn_ranks="average": the ranks of a process group train independently and merge their learners at the end of every learn_now
        # (periodic parameter averaging; this build's own, the reference has no multi-process training).  Checked before a device is touched.
        if learn_ranks not in (None, "average"):
            raise ValueError("learn_ranks must be None (learning runs on a single rank) or 'average' (every rank trains on its own rings and the "
                             "ranks average their learners after every learning episode), got %r" % (learn_ranks,))
        if learn_ranks and learn != "device":
            raise ValueError("learn_ranks='average' needs learn='device' (got learn=%r)" % (learn,))
        self.learn_ranks = learn_ranks
        # learn_steps: minibatch updates per call -- an int is the DQN learners' (as always), a dict by method name sets it per kind;
        # D3QN defaults to 1 (D3QNAgent.train() makes one update), and so does PERDQN (train_model())
        self.learn_steps_of = {"DQN": 5, "D3QN": 1, "PERDQN": 1}
        steps_given = learn_steps   # (as the caller spelled it: learn="reference" takes none)
        if isinstance(learn_steps, dict):
            bad = [k for k in learn_steps if k not in ENTRY_BY_METHOD and k != "PERDQN"]
            if bad:
                raise ValueError("learn_steps: no entry point trains %s brains" % ", ".join(map(str, bad)))
            self.learn_steps_of.update({k: int(v) for k, v in learn_steps.items()})
        else:
            self.learn_steps_of["DQN"] = int(learn_steps)
        learn_steps = self.learn_steps_of["DQN"]
        self.width, self.height = width, height
        self.actions, self.entities = Actions, EntityTypes
        self.brains = brains
        self.max_agents = max_agents
        self.max_gene = len(brains)
        self.static_families = static_families
        self.training = training
        self.save = save
        self.google_colab = google_colab
        self.limit_reproduction = limit_reproduction
        self.incentivize_killing = incentivize_killing
        self.action_space = 8
        self.observation_space = 153
        self.n_worlds = n_worlds
        # Replica sharding: under an initialised torch.distributed process group (passed as `dist`, or found) this
        # process is ONE rank of a job whose replicas are `n_worlds` per rank -- global replica ids rank * n_worlds .. + n_worlds - 1
        # key the Philox streams (results do not depend on the number of ranks), the device defaults to cuda:LOCAL_RANK, and the
        # Tracker pools its per-interval statistics over all ranks with ONE all-gather per closed interval (+ one layout check when it is built).
        self.dist, self.rank, self.world_size = resolve_dist(dist)
        self.world_base = int(world_base) if world_base is not None else self.rank * n_worlds
        if device is None:
            device = "cuda:%d" % (int(os.environ.get("LOCAL_RANK", "0")) if self.dist is not None else 0)
        self.device = device
        # rng="reference" means "this process's one world consumes the process-global generators like the reference does": that cannot
        # be a shard of a replicated job (every rank would build the same world from the same seeds and the Tracker would pool
        # duplicates), so under a process group of several ranks, or at a non-zero world_base, the default is the keyed Philox streams
        sharded = self.world_size > 1 or self.world_base != 0
        self.rng = rng or ("reference" if (n_worlds == 1 and not sharded) else "philox")
        if self.rng not in ("reference", "philox") or (self.rng == "reference" and n_worlds != 1):
            raise ValueError("rng must be 'reference' (single world only) or 'philox'")
        if self.rng == "reference" and sharded:
            raise ValueError("rng='reference' draws from the process-global generators and ignores world_base: it cannot be one shard of "
                             "a replicated job (world_size %d, world_base %d) -- use rng='philox'" % (self.world_size, self.world_base))
        # SURVEY.md 8d's synthetic benchmark worlds through this API (keyword-only extras, rng="philox"): reset() fills every world with
        # `synthetic_agents` agents at random cells (gene / brain uniform over the brains) instead of one agent per brain, and a world
        # whose population drops below `refill_below` after update_env is re-generated (what bench.py times: 100 / 70)
        self.synthetic_agents, self.refill_below = synthetic_agents, refill_below
        if (synthetic_agents is not None or refill_below is not None) and self.rng != "philox":
            raise ValueError("synthetic_agents / refill_below need rng='philox'")
        if refill_below is not None and synthetic_agents is None:
            raise ValueError("refill_below needs synthetic_agents (the population a re-generated world starts with)")
        self.learn, self.learn_steps, self.learners = learn, int(learn_steps), {}
        if learn == "device":   # every condition is checked before a device is touched
            if self.rng != "philox":
                raise ValueError("learn='device' needs rng='philox' (the multi-tick launches that fill the replay rings); this environment has rng=%r" % self.rng)
            if not static_families:
                raise ValueError("learn='device' needs static_families=True: per-gene brain copies (non-static families) do not learn yet")
            if not training:
                raise ValueError("learn='device' needs training=True")
            if self.world_size > 1 and not learn_ranks:
                raise ValueError("learn='device' runs on a single rank: multi-rank training needs a weight collective (world size %d) -- "
                                 "learn_ranks=\"average\" is it: the ranks then average their learners after every learning episode" % self.world_size)
            if learn_ranks and self.world_size > _lib.MAX_MERGE_RANKS:
                raise ValueError("learn_ranks='average' merges the learners of at most %d ranks (world size %d)" % (_lib.MAX_MERGE_RANKS, self.world_size))
            if len(brains) > _lib.MAX_CAPTURE_BRAINS:
                raise ValueError("learn='device' captures transitions for at most %d brains (got %d)" % (_lib.MAX_CAPTURE_BRAINS, len(brains)))
            if min(self.learn_steps_of.values()) < 1 or (learn_every is not None and int(learn_every) < 1):
                raise ValueError("learn_steps and learn_every must be >= 1")
        self.schedule = None        # learn="reference": the host schedule (learn_reference.ReferenceSchedule)
        self._ppo_narrow = {}       # ... and per PPO brain the rl_learn_ppo learner over the wide learner's tensors
        self._learned = False       # ... learn_reference() ran since the last step()
        self.reference_calls = []   # ... every Call made so far as (n_epi, Call), while log_reference_calls is on (tests, diagnostics)
        self.reference_choices = []  # ... and per PERD3QN train() (n_epi, brain, indices, slots, bracket) as device tensors, likewise
        #                              (per PERDQN train_model(): (n_epi, brain, idxs, slots, points), idxs the reference's TREE indices)
        if learn == "reference":    # every condition is checked before a device is touched
            self._check_reference(brains, n_worlds, static_families, training, learn_every, steps_given)
        self.best_agents = []
        # environment.py:118: the painter is built first (pastel colours draw from `random` here, its background tiles at
        # the first render() -- both matter for same-seed runs)
        from ..Helpers.render import Visualize
        self.viz = Visualize(self.width, self.height, grid_size, pastel=pastel_colors)
        self.frame = None
        self.worlds = DeviceWorlds(n_worlds=n_worlds, width=width, height=height, max_agents=max_agents,
                                   n_brains=len(brains), static_families=static_families,
                                   limit_reproduction=limit_reproduction, incentivize_killing=incentivize_killing, seed=seed,
                                   device=device, world_base=self.world_base)
        # results tracker (environment.py:125-131); numeric part only, fed by the step kernel
        from ..Helpers.tracker import Tracker
        self.tracker = Tracker(update_interval=update_interval, interactive=False, print_results=print_results, nr_genes=len(brains),
                               static_families=static_families, brains=brains, worlds=self.worlds if training else None,
                               dist=self.dist)
        self._mirrors = {}          # world -> _WorldMirror, built on demand (_mat): env.agents is world 0's
        self._stamp = 0             # counts the changes of the device state (_refresh)
        self._n_empty = None        # rng="reference": empty cells after this tick's _add_food, as far as the host's draws say
        self._grid = self._max_gene = None
        self._phase = "update"
        self._acted = False         # act() ran since the last step() / update_env(): worlds.actions holds the policy's choice
        self._empty = True          # no world has been built yet (before reset())
        self._brains_bound, self._bound_key = False, None
        self._ticks_since_check = 0
        self.loop_seconds = None    # wall time of the last trainer() / tester() loop on this environment (set by them)
        self.learn_every = None
        self.learn_now_calls = 0    # learn_now() calls so far (learn_ranks="average": one collective each under a process group)
        self._merge_row = None      # learn_ranks="average": the row this rank's learners are exported into
        if learn == "device":
            # the replay rings of DQN.py:15 (buffer_limit), filled inside the multi-tick launches; one learner per brain rl_learn trains,
            # whose packed tensor IS that brain's acting weights from here on (rl_learn rewrites it in place)
            plan = {k: ENTRY[entry_of(b.kind)] for k, b in enumerate(brains) if b.method in self.learn_kinds and entry_of(b.kind)}
            for e in ENTRIES:   # ... and the explicit opt-ins (learn_prioritized, learn_rollout, learn_td_priority), in the table's order
                if e.keyword and not e.narrow and getattr(self, "learn_" + e.keyword):
                    plan.update({k: e for k, b in enumerate(brains) if b.method == e.method})
            prob = {"with_prob": True} if any(e.family == "ppo" for e in plan.values()) else {}   # the acting probability of every row (PPO.py:73): only where a PPO brain learns
            # a D3QN or prioritised PERD3QN learner's ring holds its brain's `capacity` rows (D3QN.py:62, PERD3QN.py:49, 55: 10,000), a
            # PERDQN learner's its brain's memory_size (20,000); every other ring stays DQN.py:15's
            rows = [int(getattr(b, plan[k].ring_rows)) if k in plan and plan[k].ring_rows else BUFFER_LIMIT for k, b in enumerate(brains)]
            # ... and none is smaller than what one tick of all worlds can append to it (n_worlds * slot_cap, the floor of rl_replay: below it
            # two rows of one tick would share a slot, written in no order): a ring below the floor is raised to it, and the learner's
            # size gate and draws then see that many rows.  ring_rows says what was chosen; with nothing below the floor the call is the
            # one it always was
            floor = int(n_worlds) * _lib.slot_cap_for(max_agents)
            self.ring_floor, self.ring_rows = floor, [max(r, floor) for r in rows]
            if self.ring_rows != rows:
                self.worlds.enable_capture(self.ring_rows, **prob)
            else:
                self.worlds.enable_capture(rows if any(e.ring_rows for e in plan.values()) else BUFFER_LIMIT, **prob)
            for k, e in plan.items():   # (learn_batch: the wide entry in the narrow one's place, through its own keyword on top)
                kw = {e.keyword: True} if e.keyword else {}
                if self.learn_batch_of.get(e.method) is not None:
                    kw[wide[e.method].keyword] = self.learn_batch_of[e.method]
                self.learners[k] = DeviceLearner(brains[k], self.worlds.device, ring=self.worlds.replays[k], **kw)
            if not self.learners:
                raise ValueError("learn='device': none of the brains is of a kind rl_learn trains (DQN)" if self.learn_kinds == ("DQN",) else
                                 "learn='device': none of the brains is of a kind in learn_kinds %r" % (self.learn_kinds,))
            # the default period is the smallest train_freq of the learners a run has WITHOUT learn_prioritized, so that the keyword does
            # not move their schedule; the prioritised learners' own train_freq counts only where they are the only learners -- and
            # likewise learn_rollout and the PPO learners', and learn_td_priority and the PERDQN learners'
            timed = next(t for t in ([l for l in self.learners.values() if l.spec.family in FAMILIES[:i]] for i in range(2, len(FAMILIES) + 1)) if t)
            self.learn_every = int(learn_every) if learn_every is not None else min(l.train_freq for l in timed)
            frozen = ["%d (%s)" % (k, b.method) for k, b in enumerate(brains) if k not in self.learners]
            if frozen:
                warn_inference_only(frozen, self.learn_kinds + (("PERD3QN (prioritised)",) if self.learn_prioritized else ())
                                    + (("PPO (rollouts)",) if self.learn_rollout else ())
                                    + (("PERDQN (TD priorities)",) if self.learn_td_priority else ()), draw=self.learn_draw)
            if self.learn_ranks:
                self._align_learners()
        elif learn == "reference":
            self._build_reference(brains, max_agents)
        elif training:
            warn_inference_only()

    def _check_reference(self, brains, n_worlds, static_families, training, learn_every, learn_steps):
        """The conditions of learn="reference", each a ValueError that names it.  (The other learn_* keywords have refused a learn that
        is not 'device' by now, each in its own words.)"""
        if n_worlds != 1:
            raise ValueError("learn='reference' needs n_worlds=1: it is the reference's own per-agent schedule for its one world (got n_worlds=%r); "
                             "learn='device' trains many worlds" % (n_worlds,))
        if self.world_size > 1:
            raise ValueError("learn='reference' runs on a single rank (world size %d)" % self.world_size)
        if self.rng != "reference":
            raise ValueError("learn='reference' needs rng='reference' (random.sample's draws interleave with the coins of act() and the draws of "
                             "update_env() on the process-global generators); this environment has rng=%r" % self.rng)
        if not static_families:
            raise ValueError("learn='reference' needs static_families=True: per-gene brain copies (non-static families) do not learn yet")
        if not training:
            raise ValueError("learn='reference' needs training=True")
        if learn_every is not None:
            raise ValueError("learn='reference' takes no learn_every: a brain trains when an agent's age is a multiple of its train_freq or the agent died")
        if isinstance(learn_steps, dict) or learn_steps != 5:
            raise ValueError("learn='reference' takes no learn_steps: the brains' own train() sets the updates per call (DQN 5, D3QN 1)")
        if len(brains) > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("learn='reference' captures transitions for at most %d brains (got %d)" % (_lib.MAX_CAPTURE_BRAINS, len(brains)))

    def _build_reference(self, brains, max_agents):
        """The learners, rings and schedule of learn="reference" (learn_reference.py): a ring of the deque's maxlen + slot_cap rows per
        learning brain (the floor for the others, whose rows nobody reads), one DeviceLearner per DQN / D3QN / PPO brain whose packed
        tensor is the brain's acting weights from here on.  A PPO brain's learner is the wide one, built once for PPO_LIST_MAX rows; the
        narrow entry's learner shares every tensor with it.  With learn_reference_prioritized=True a PERD3QN brain gets a prioritised
        learner (DeviceLearner(prioritized=True)) whose priorities, one per ring row, stay on the device."""
        from ..learn_reference import KINDS, PPO_LIST_MAX, BrainSpec, ReferenceSchedule
        slack = _lib.slot_cap_for(max_agents)
        opt = dict(prioritized=True) if self.learn_reference_prioritized else {}
        if self.learn_reference_td:   # (the keyword is only passed where it is given: every other run builds the specs it built)
            opt["td"] = True
        self.schedule = ReferenceSchedule([BrainSpec.of(b, **opt) for b in brains], slack)
        specs = self.schedule.specs
        self.ring_floor = slack
        self.ring_rows = [self.schedule.ring_rows(k) if specs[k] else slack for k in range(len(brains))]
        ppo = any(s is not None and s.method == "PPO" for s in specs)
        self.worlds.enable_capture(self.ring_rows, **({"with_prob": True} if ppo else {}))
        for k, s in enumerate(specs):
            if s is None:
                continue
            ring = self.worlds.replays[k]
            if s.method == "PPO":
                wide = self.learners[k] = DeviceLearner(brains[k], self.worlds.device, ring=ring, rollout=True, rollout_batch=PPO_LIST_MAX)
                narrow = self._ppo_narrow[k] = DeviceLearner(brains[k], self.worlds.device, ring=ring, rollout=True)
                for name in ("params", "adam_m", "adam_v", "state", "packed") + wide.spec.side_tensors:
                    setattr(narrow, name, getattr(wide, name))
            elif s.method == "PERD3QN":
                self.learners[k] = DeviceLearner(brains[k], self.worlds.device, ring=ring, prioritized=True)
            elif s.method == "PERDQN":   # rl_learn_td on the slots the tree walk names; the gate is the schedule's (train_start)
                l = self.learners[k] = DeviceLearner(brains[k], self.worlds.device, ring=ring, td_priority=True)
                l.min_size = 0
            else:
                self.learners[k] = DeviceLearner(brains[k], self.worlds.device, ring=ring)
        frozen = ["%d (%s)" % (k, b.method) for k, b in enumerate(brains) if k not in self.learners]
        if frozen:
            if self.learn_reference_td:   # (with it only PERD3QN brains without their own keyword can be left)
                warn_inference_only(frozen, KINDS + (("PERD3QN",) if self.learn_reference_prioritized else ()) + ("PERDQN",), mode="reference_td")
            else:
                warn_inference_only(frozen, KINDS, mode="reference_prioritized" if self.learn_reference_prioritized else "reference")
        if not self.learners:
            raise ValueError("learn='reference': none of the brains is of a kind that trains in this mode (DQN, D3QN, PPO)")

    def learn_reference(self, n_epi=0):
        """trainer.py:95-96 -- Agent.learn() for every agent of the post-step list -- between step() and update_env(n_epi): one
        capture of the tick's transitions (rl_capture_transitions), then the calls the schedule names, in its order, each one
        DeviceWorlds.learn with one learner and the slots of the rows random.sample drew (learn_reference.ReferenceSchedule).  The
        schedule reads the host mirror step() has built; nothing is read back.  Returns the tick's Calls."""
        if self.learn != "reference":
            raise ValueError("learn_reference() needs learn='reference' (this environment has learn=%r)" % (self.learn,))
        if self._phase != "step" or self._learned:
            raise RuntimeError("learn_reference() belongs between step() and update_env(), once per tick")
        h = self._host
        calls = self.schedule.tick(n_epi, zip(h["a_brain"], h["a_age"], h["a_flags"] & _lib.F_DEAD))
        self._learned = True
        self.worlds.capture_transitions(with_policy_out=bool(self._ppo_narrow))
        self.worlds.launches += 1
        for c in calls:
            l = self.learners[c.brain]
            if c.kind == "sync":    # eval -> target without an update: on the same stream, behind the last update
                l.target.copy_(l.params)
                self.worlds.launches += 1
            elif c.kind == "ppo":
                self._learn_ppo(c.brain, c.slots, c.wide)
            elif c.kind == "store" and l.spec.family == "td":   # PERDQN: Memory.add for the rows behind the tick's last train_model()
                self.worlds.store_td_reference([l], [self.schedule.specs[c.brain].capacity], [c.store[0]], [c.store[1]])
            elif c.kind == "store":   # PERD3QN: store()'s priority for the rows behind the tick's last train()
                self.worlds.store_prioritized_reference([l], [self.schedule.specs[c.brain].capacity], [c.store[0]], [c.store[1]])
            elif c.uniforms is not None and l.spec.family == "td":
                self._learn_td_reference(n_epi, c)
            elif c.uniforms is not None:
                self._learn_prioritized_reference(n_epi, c)
            else:
                l.sync_target = bool(c.sync_target)
                self.worlds.learn([l], c.slots.shape[0], slots=c.slots[None])
        if self.log_reference_calls:
            self.reference_calls += [(n_epi, c) for c in calls]
        return calls

    def _learn_ppo(self, brain, slots, wide):
        """One PPO.learn() on the rows at `slots` ([1][length], storage order) through rl_learn_ppo_wide (wide) or rl_learn_ppo; the
        batch of the call is the list's length."""
        l = self.learners[brain] if wide else self._ppo_narrow[brain]
        l.batch = int(np.asarray(slots).shape[-1])
        self.worlds.learn([l], 1, slots=np.asarray(slots, np.int32).reshape(1, 1, -1), gate=False)

    def _learn_prioritized_reference(self, n_epi, c):
        """One PERD3QNAgent.train() of learn_reference_prioritized=True: the stamp of the rows stored since the last one, the cdf walk on
        the call's uniforms, and rl_learn_prioritized on the slots it leaves on the device -- three launches, nothing read back."""
        l, capacity = self.learners[c.brain], self.schedule.specs[c.brain].capacity
        self.worlds.store_prioritized_reference([l], [capacity], [c.store[0]], [c.store[1]])
        indices, slots, bracket = self.worlds.choose_prioritized_reference([l], [capacity], [c.store[0] + c.store[1]], [c.uniforms],   # (the rows stored as of THIS call)
                                                                           with_bracket=self.log_reference_calls)
        l.sync_target = bool(c.sync_target)
        self.worlds.learn([l], 1, slots=slots)
        if self.log_reference_calls:
            self.reference_choices.append((n_epi, c.brain, indices[0], slots[0, 0], bracket[0]))

    def _learn_td_reference(self, n_epi, c):
        """One PERDQNAgent.train_model() of learn_reference_td=True: epsilon's decay on the host (PERDQN.py:132-133, a Python double, in
        front of the draw), then Memory.add for the rows stored since the last group, the stratified walk on the call's uniforms,
        rl_learn_td on the slots it leaves on the device, and the tree's update from the priorities that has written -- four launches,
        nothing read back."""
        l, capacity = self.learners[c.brain], self.schedule.specs[c.brain].capacity
        if l.brain.epsilon > l.brain.epsilon_min:
            l.brain.epsilon -= l.brain.epsilon_decay
        self.worlds.store_td_reference([l], [capacity], [c.store[0]], [c.store[1]])
        idxs, slots, points = self.worlds.sample_td_reference([l], [capacity], [c.store[0] + c.store[1]], [c.uniforms],   # (the rows stored as of THIS call)
                                                              with_points=self.log_reference_calls)
        l.sync_target = bool(c.sync_target)
        self.worlds.learn([l], 1, slots=slots)
        self.worlds.update_td_reference([l], [capacity], idxs, slots)
        if self.log_reference_calls:
            self.reference_choices.append((n_epi, c.brain, idxs[0], slots[0, 0], points[0]))

    def _opt_in(self, keyword, value, learn, brains):
        """learn_<keyword>=True, the environment's spelling of DeviceLearner(..., <keyword>=True): None or True, with learn='device' and
        at least one brain of the method that entry point trains."""
        name, method = "learn_" + keyword, next(e.method for e in ENTRIES if e.keyword == keyword)
        if value not in (None, True):
            raise ValueError("%s must be None or True, got %r" % (name, value))
        if value and learn != "device":
            raise ValueError("%s=True needs learn='device' (got learn=%r)" % (name, learn))
        if value and not any(getattr(b, "method", None) == method for b in brains):
            raise ValueError("%s=True needs at least one Models.%s brain (got %s)" % (name, method, ", ".join(str(getattr(b, "method", b)) for b in brains)))
        setattr(self, name, bool(value))

    def _align_learners(self):
        """Set-up of learn_ranks="average": the ranks build their brains from their own torch generators, so they start from rank 0's
        parameters -- one signature gather (the same learners, with the same exploration and soft_update_freq, on the same schedule everywhere,
        or the same ValueError on every rank) and
        ONE broadcast of all learners' params; then target = params (PPO has none), Adam's moments zero, and the acting weights repacked
        on the device (rl_policy_pack_device).  Without a process group there is nothing to align: a fresh learner is in that state already."""
        if self.dist is None:
            return
        from ..distributed import broadcast_from_rank0, check_learner_signature
        ls = [self.learners[k] for k in sorted(self.learners)]
        sig = [len(ls)]
        for k in sorted(self.learners):
            l = self.learners[k]   # (exploration and soft_update_freq decide whether a learner is called and when its target is synced)
            sig += [k, l.kind, ENTRIES.index(l.spec), getattr(l, "exploration", 0), getattr(l, "soft_update_freq", 0)]
            if l.spec.narrow:   # (the other entry points' batches come from the brains' classes: the signatures of runs without learn_batch stay what they were)
                sig += [l.batch]
        sig += [self.learn_every, self.learn_steps_of["DQN"], self.learn_steps_of["D3QN"], self.learn_steps_of["PERDQN"], self.rollout_steps]
        if self.learn_td_stamp:   # (appended, and only when given: every other run's signature stays what it was)
            sig += [1]
        check_learner_signature(sig, self.dist, device=self.worlds.device)
        flat = torch.cat([l.params for l in ls])
        broadcast_from_rank0(flat, self.dist)
        for l, part in zip(ls, flat.split([l.n_params for l in ls])):
            l.params.copy_(part)
            if l.target is not None:
                l.target.copy_(l.params)
            l.adam_m.zero_(); l.adam_v.zero_()
            self.worlds.pack_device(l.kind, l.params, l.packed)

    def _merge_learners(self, called):
        """The end of a learning episode under learn_ranks="average": export -> ONE all-gather -> merge, for all learners at once
        (DeviceWorlds.export_learners / merge_learners).  `called`: the learners this episode's calls were made for -- only their
        sync_target flags count (a D3QN learner still below its exploration keeps its target).  Without a process group the merge runs
        straight from the exported row (n_ranks = 1: the identity), so the path is the same in one process."""
        ls = [self.learners[k] for k in sorted(self.learners)]
        if self._merge_row is None:
            self._merge_row = torch.empty(sum(l.merge_floats for l in ls), dtype=torch.float32, device=self.worlds.device)
        row = self.worlds.export_learners(ls, out=self._merge_row)
        rows, n_ranks = row, 1
        if self.dist is not None:
            from ..distributed import gather_learner_rows
            rows = gather_learner_rows(row, self.dist).to(self.worlds.device)   # (under gloo the table arrives on the host)
            n_ranks = self.world_size
        self.worlds.merge_learners(ls, rows, n_ranks, sync_target=[bool(l.sync_target) and any(l is c for c in called) for l in ls])

    # -- the host view of the device state: materialised on first read after every state change ------------------------------
    @property
    def agents(self):
        """env.agents (environment.py:186, 214): world 0's agents in row-major order, as AgentView objects."""
        return [] if self._empty else self._mat(0).views

    @property
    def grid(self):
        """Grid.get_numpy() of world 0 (grid.py:49-57): [height, width] uint8 cell codes."""
        if self._grid is None and not self._empty:
            self._sync()
            self._grid = self.worlds.s["cell_type"][0].cpu().numpy().reshape(self.height, self.width)
        return self._grid

    @property
    def max_gene(self):
        if self._max_gene is None:
            self._sync()
            self._max_gene = int(self.worlds.s["max_gene"][0].item())
        return self._max_gene

    @max_gene.setter
    def max_gene(self, v):
        self._max_gene = int(v)

    # world 0's mirror under the names the rest of this class uses
    _mirror0 = property(lambda s: s._mat(0))
    _host = property(lambda s: s._mat(0).host)
    _state_host = property(lambda s: s._mat(0).state)

    # -- brains -------------------------------------------------------------------------------------------------
    def _bind_brains(self):
        """The brains' packed weights and current exploration rates on the device.  Weights are packed and uploaded when they have
        changed (packed_weights() keys its cache on the parameters' storage and version counters); otherwise only the rates move."""
        packed = [self.learners[k].packed if k in self.learners else b.packed_weights(self.device) for k, b in enumerate(self.brains)]
        key = tuple((b.kind, id(p)) for b, p in zip(self.brains, packed))   # (a repack makes a new tensor object)
        eps = [float(getattr(b, "epsilon", 0.0)) for b in self.brains]
        if self._brains_bound and key == self._bound_key:
            self.worlds._set_epsilons(eps)
            return
        self.worlds.set_brains([(b.kind, e, p) for b, e, p in zip(self.brains, eps, packed)])
        self._brains_bound, self._bound_key = True, key

    def _epsilon_schedule(self, n_epi, k):
        """[k, n_brains] float32: the brains' exploration rates in episodes n_epi .. n_epi + k - 1 (their own update rules:
        DQN.py:67-69, D3QN.py:84-89); leaves every brain in the state it has after episode n_epi + k - 1."""
        eps = np.empty((k, len(self.brains)), np.float32)
        for b, brain in enumerate(self.brains):
            sched = getattr(brain, "epsilon_schedule", None)
            if sched is not None:
                eps[:, b] = sched(n_epi, k)
            else:   # a brain class of the caller's: its own update rule, episode by episode
                for t in range(k):
                    brain.update_epsilon(n_epi + t)
                    eps[t, b] = getattr(brain, "epsilon", 0.0)
        return eps

    # -- reference protocol ---------------------------------------------------------------------------------------
    def reset(self):
        """environment.py:133-158.  World 0 follows the reference's np.random draw order exactly; further replicas are built
        by the same rule on the device (rl_reset_families)."""
        if self.synthetic_agents is not None:
            self.worlds.reset_synthetic(self.synthetic_agents)
            self._empty = False
            self._refresh(after="update")
            return
        # replicas: the same construction (one agent per brain, gene = its index; environment.py:147-149) on the device, from the
        # Philox streams keyed by (seed, global replica id): ONE launch for any number of worlds ...
        if self.rng == "philox" and (self.n_worlds > 1 or self.world_base != 0):
            self.worlds.reset_families()
        # ... and the job's replica 0 alone (world 0 of the rank with world_base 0) consumes the process-global np.random, in the
        # reference's order: a sharded job builds the same replicas whatever the number of ranks.  (rng="reference" -- one world per
        # process, the reference's own generator calls -- always does.)
        if self.world_base == 0 or self.rng == "reference":
            snap = host_reset(self.width, self.height, len(self.brains))
            self.worlds.load_world(0, snap)
            self.worlds.observe()
        self._empty = False
        self._refresh(after="update")

    def act(self, n_epi=0):
        """Agent.get_action for every agent of every world, batched on the GPU (trainer.py:88-89).

        rng="reference": one batched forward pass per brain, then the brains' own get_action rules agent by agent in
        list order, so the epsilon-greedy coins / categorical samples are the reference's generator calls in the
        reference's order (the forward pass draws nothing, so batching it changes no draw).
        rng="philox": forward pass, epsilon-greedy / categorical selection and the draws all happen in the kernel."""
        if self.rng == "reference":
            # ONE policy launch for all agents (rl_policy_act: per-brain row lists built on the device, every brain kind side by side),
            # queued before the host has looked at anything; its outputs travel with the state snapshot (one copy, one wait).  The
            # kernel's own action choice is overwritten below: the brains' rules run on the host, in list order, on these outputs.
            self._bind_brains()
            self.worlds.act(want_q=True)
            self._acted = True
            m = self._mat(0)
            if m.q is None:   # (the mirror was built before this call: somebody read env.agents first)
                m.q = self.worlds.out_q[0].cpu().numpy()
            q, qt = m.q, None
            for k, agent in enumerate(m.views):
                if agent.brain.method == "PPO":   # (Categorical(prob).sample() wants a tensor; argmax rules take the numpy row)
                    qt = torch.from_numpy(q) if qt is None else qt
                    agent.get_action(n_epi, out=qt[k])
                else:
                    agent.get_action(n_epi, out=q[k])
            return
        for b in self.brains:
            b.update_epsilon(n_epi)
        self._bind_brains()
        self.worlds.act()
        self._acted = True
        for m in self._mirrors.values():   # mirrors built before this call: their actions are the policy's choice now
            m.actions = None               # (fetched on first use: AgentView.action)
            m.dirty = False

    def step(self):
        """environment.py:160-186"""
        dirty = [m for m in self._mirrors.values() if m.dirty]
        if dirty:
            if self.n_worlds == 1:   # (the mirror holds the whole row: nothing to read back)
                full = dirty[0].actions[None]
            else:
                full = self.worlds.actions.cpu().numpy()
                for m in dirty:
                    full[m.world] = m.actions
            for m in dirty:
                m.dirty = False
            self.worlds.set_actions(full)
        if self.rng == "reference":
            # the draws of _add_food need the grid after movement: first half, ONE snapshot (the counts AND the post-step agent list --
            # update_env's draws are made from it without another look at the device), host draws, second half
            self.worlds.step_split()
            snap = self._snapshot()
            nf, npo, ns, ne = (int(x) for x in snap["pre_counts"][0])
            tape, self._n_empty = self._draw_add_food(nf, npo, ns, ne)
            self.worlds.step_food(self.worlds.make_tape([tape]))
            self._refresh(after="step")
            self._learned = False
            self._mirrors[0] = self._build_mirror(0, snap)   # (its cell_type predates the food: env.grid fetches its own)
        else:
            self.worlds.step()
            self._refresh(after="step")

    def update_env(self, n_epi=0):
        """environment.py:188-215"""
        if self.training:
            if self.tracker.update_results(None, n_epi):   # (the per-tick statistics were accumulated inside the step launch)
                self._ticks_since_check = 0                # an interval closed: the error flag came back with its sums (Tracker.resolve)
        self._ticks_since_check += 1
        if self._ticks_since_check >= 256:   # a loop that never reads env.agents / env.grid still learns of a device error
            self._sync()
            self._ticks_since_check = 0
        if self.rng == "reference":
            tape, produced = self._draw_update()
            self.worlds.update(self.worlds.make_tape([tape]))
            self._refresh(after="update")
            if produced and not self.static_families:  # Agent.mutate_brain (entities.py:210-213) draws torch.randn
                new = np.nonzero(self._host["a_gene"] == self.max_gene)[0]
                if len(new) and self.brains[int(self._host["a_brain"][new[0]])].method == "PERD3QN":
                    torch.randn((128, 153))  # PERD3QN.py:127-130; brains are shared by index here, only the stream advances
        else:
            self.worlds.update()
            if self.refill_below is not None:
                self.worlds.refill(self.refill_below, self.synthetic_agents)
            self._refresh(after="update")

    # -- the reference's random draws, made on the host from the global generators (rng="reference") -----------
    def _draw_add_food(self, n_food, n_poison, n_super, n_empty):
        """_add_food (environment.py:763-776) -> Grid.set_random (grid.py:69-83): randint(0, #empty) then random(), nothing
        when the grid is full (randint raises before drawing)."""
        C = self.width * self.height
        k = np.zeros(_lib.FOOD_TRIES, np.int32)
        u = np.full(_lib.FOOD_TRIES, 2.0)
        for tries, enabled, p in (((0, 1, 2), n_food <= C / 10, 0.2), ((3, 4, 5), n_poison <= C / 20, 0.2), ((6,), n_super == 0, 1.0)):
            if not enabled:
                continue
            for t in tries:
                if n_empty == 0:
                    continue
                k[t] = np.random.randint(0, n_empty)
                u[t] = np.random.random()
                n_empty -= u[t] < p
        return {"food_k": k, "food_u": u, "repro_u": [], "birth_k": [], "produce_u": 0.0, "produce_choice": 0}, n_empty

    def _draw_update(self):
        """_reproduce / _produce (environment.py:488-547) over the post-step agent list (host mirror)."""
        import random
        h = self._host
        n1 = len(h["a_age"])
        # (empty cells after _add_food: known from step()'s own draws; a caller who changed the world in between reads the grid)
        n_empty = self._n_empty if self._n_empty is not None else int((self.grid == _lib.EMPTY).sum())
        repro_u, birth_k = [], []
        produce_u, choice, produced = 0.0, 0, False

        def place():
            nonlocal n_empty
            if n_empty == 0:
                return False
            birth_k.append(np.random.randint(0, n_empty))
            np.random.random()  # the p=1 coin
            n_empty -= 1
            return True

        if n1 <= self.max_agents:
            for a in range(n1):
                if (h["a_flags"][a] & (_lib.F_DEAD | _lib.F_REPRODUCED)) or h["a_age"][a] <= 5:
                    continue
                r = random.random()
                repro_u.append(r)
                if r > 0.95:
                    place()
            produce_u = random.random()
            if produce_u > 0.95:
                if self.static_families:
                    genes = set([int(g) for g in h["a_gene"]])
                    not_alive = list(set(range(len(self.brains))).difference(genes))
                    choice = random.choice(not_alive) if not_alive else random.choice([x for x in range(len(self.brains))])
                else:
                    choice = random.choice(range(_lib.N_BEST))
                produced = place()
        return ({"food_k": np.zeros(_lib.FOOD_TRIES, np.int32), "food_u": np.zeros(_lib.FOOD_TRIES), "repro_u": repro_u,
                 "birth_k": birth_k, "produce_u": produce_u, "produce_choice": choice}, produced)

    def render_feed(self, world=0):
        """What the reference's painter reads (render.py:90-200) for one world: agents i/j/gene/health/killed/dead + food cells."""
        from ..Helpers.render import RenderFeed
        return RenderFeed.from_world(self.width, self.height, self.worlds.world(world))

    def render(self, fps=10, world=0):
        """environment.py:217-231.  No pygame window here: the frame is painted into `self.frame` (uint8 RGB,
        [height*grid_size, width*grid_size, 3]); returns True = keep going, like an open pygame window does."""
        self.frame = self.viz.frame(self.render_feed(world))
        return True

    def frames(self, worlds=None, out=None):
        """The frames render() would paint for `worlds` (ids in any order, repeats allowed; None = all worlds), painted on the device by
        rl_render: a uint8 tensor [n, height*grid_size, width*grid_size, 3] on the environment's device, byte for byte what
        Visualize.frame gives for each world.  Queued behind the ticks launched so far, without a host round trip; `out` is painted
        into and returned when given.  (`Helpers.render.mosaic` lays the frames out as one contact sheet.)"""
        return self.worlds.render(self.viz.style(self.worlds.device), worlds, out)

    def record(self, n_ticks, worlds=(0,), every=1, n_epi=0, out=None):
        """A film of `worlds` over `n_ticks` ticks of run(): uint8 [1 + n_ticks // every, n, Hpx, Wpx, 3] on the device.  Frame 0 is the
        state at the call, frame k the state after k * `every` more ticks starting at episode `n_epi`; ticks and painting are queued
        on one stream with no host wait between them.  Equal to a loop of run(n_epi, every) + frames(worlds)."""
        if self.rng != "philox":
            raise ValueError("record() needs rng='philox' (the multi-tick launches of run()); this environment has rng=%r" % self.rng)
        if every < 1 or n_ticks < 0:
            raise ValueError("record(): every must be >= 1 and n_ticks >= 0")
        n_shots = 1 + n_ticks // every
        n = self.n_worlds if worlds is None else len(worlds)
        gs = self.viz.grid_size
        shape = (n_shots, n, self.height * gs, self.width * gs, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.worlds.device)
        elif tuple(out.shape) != shape:
            raise ValueError("record(): out must have shape %s" % (shape,))
        self.frames(worlds, out=out[0])
        for k in range(1, n_shots):
            self.run(n_epi, every)
            n_epi += every
            self.frames(worlds, out=out[k])
        return out

    def save_results(self, main_folder="experiments"):
        """environment.py:233-256: brains + parameters + results.json + settings.json in the reference's layout."""
        from ..Helpers.saver import SavedAgent, Saver
        settings = {"Update interval": self.tracker.update_interval, "Width": self.width, "Height": self.height,
                    "Max agents": self.max_agents, "Families": self.static_families,
                    # (extra key, not in the reference's file) which weights were updated: say so next to them
                    "Weights": self._weights_note()}
        if self.learn_batch is not None:   # (extra key, only where the keyword was given)
            settings["Learn batch"] = self.learn_batch
        if self.learn_draw is not None:    # (likewise)
            settings["Learn draw"] = self.learn_draw
        if self.learn_td_stamp is not None:   # (likewise)
            settings["Learn td stamp"] = self.learn_td_stamp
        if self.static_families:
            agents = [SavedAgent(g, b) for g, b in enumerate(self.brains)]
        else:  # the brains the best agents descend from (inference-time copies share their weights)
            bb = self.worlds.s["best_brain"][0].cpu().numpy()
            agents = [SavedAgent(int(self.max_gene), self.brains[int(b)]) for b in bb]
        return Saver(main_folder, google_colab=self.google_colab).save(agents, self.static_families, self.tracker.results, settings)

    # _weights_note: per entry point, in the notes' order, its note and whether it makes the frozen brains' note say "in this run"
    _NOTES = {
        "rl_learn_wide": (False, "%(steps)d minibatch updates of batch %(wide)d (learn_batch) every %(every)d episodes, rows drawn by content key with replacement"),
        "rl_learn_dueling_wide": (False, "%(steps)d minibatch update(s) of batch %(wide)d (learn_batch) in 64-row tiles, the "
                                  "advantage mean taken over the whole batch, every %(every)d episodes once past the brain's exploration, target synced every "
                                  "soft_update_freq episodes, rows drawn by content key with replacement"),
        "rl_learn": (False, "%(steps)d minibatch updates every %(every)d episodes, rows drawn by content key with replacement"),
        "rl_learn_dueling": (True, "%(steps)d minibatch update(s) of batch %(batch)s every %(every)d episodes once past the brain's "
                             "exploration, target synced every soft_update_freq episodes, rows drawn by content key with replacement"),
        "rl_learn_prioritized": (True, "one minibatch update of batch %(batch)s every %(every)d episodes once past the brain's "
                                 "exploration, target synced every soft_update_freq episodes, rows drawn with probability priority^0.6 / sum by content key "
                                 "with replacement; rows appended between two calls get the priority maximum as of the earlier call"),
        "rl_learn_prioritized_wide": (True, "one minibatch update of batch %(wide)d (learn_batch) in 64-row tiles, the "
                                      "advantage mean taken over the whole batch and the priorities of all its rows rewritten, every %(every)d episodes once past the "
                                      "brain's exploration, target synced every soft_update_freq episodes, rows drawn with probability priority^0.6 / sum by "
                                      "content key with replacement; rows appended between two calls get the priority maximum as of the earlier call"),
        "rl_learn_ppo": (True, "%(steps)d rollout(s) of %(batch)s rows, %(k_epoch)s Adam steps each, every %(every)d episodes; the rows are "
                         "drawn by content key with replacement from those appended since the last call, so the GAE's neighbours are unrelated rows "
                         "and the other fresh rows go unused"),
        "rl_learn_ppo_wide": (True, "%(steps)d rollout(s) of %(wide)d rows (learn_batch) in 32-row tiles, one GAE recursion over the whole "
                              "rollout, %(k_epoch)s Adam steps each, every %(every)d episodes; the rows are drawn by content key with replacement "
                              "from those appended since the last call, so the GAE's neighbours are unrelated rows and the other fresh rows go unused"),
        "rl_learn_td": (True, "%(steps)d minibatch update(s) of batch %(batch)s every %(every)d episodes once the ring holds the "
                        "brain's train_start rows, loss scaled by the mean importance weight, target synced at every call, rows drawn with "
                        "probability priority / sum by content key with replacement -- independent draws, not the reference's stratified ones; "
                        "every new row gets the reference's one priority (0 + 0.01) ** 0.6; epsilon decays once per update"),
        "rl_learn_td_wide": (True, "%(steps)d minibatch update(s) of batch %(wide)d (learn_batch) in 64-row tiles, the importance weights' "
                             "minimum and mean taken over the whole batch and the priorities of all its rows rewritten, every %(every)d episodes "
                             "once the ring holds the brain's train_start rows, loss scaled by the mean importance weight, target synced at every "
                             "call, rows drawn with probability priority / sum by content key with replacement -- independent draws, not the "
                             "reference's stratified ones; every new row gets the reference's one priority (0 + 0.01) ** 0.6; epsilon decays "
                             "once per update"),
    }
    assert set(_NOTES) == set(ENTRY), "every row of learn.ALL_ENTRIES needs its note"

    def _steps(self, family):
        """The updates (PPO: rollouts) one learning call makes for the learners of `family`."""
        return {"dqn": self.learn_steps, "dueling": self.learn_steps_of["D3QN"], "prioritized": 1, "ppo": self.rollout_steps,
                "td": self.learn_steps_of["PERDQN"]}[family]

    def _weights_note(self):
        if not self.learners:
            return "as loaded / initialised -- reinlife_amd runs inference only, learn() is a no-op"
        if self.learn == "reference":
            frozen = [k for k in range(len(self.brains)) if k not in self.learners]
            prio = [k for k in sorted(self.learners) if self.learners[k].spec.family == "prioritized"]
            td = [k for k in sorted(self.learners) if self.learners[k].spec.family == "td"]
            return ("brains %s trained on the device on the reference's own schedule and draws (learn='reference': per agent of the post-step "
                    "list, when its age is a multiple of train_freq or it died; minibatches by random.sample over the replay deque)"
                    % sorted(self.learners)
                    + ("; the minibatches of brains %s by np.random.choice's rule on np.random's uniforms, the priorities kept and the cdf "
                       "walked on the device (learn_reference_prioritized=True: rl_learn_prioritized_store_ref, rl_learn_prioritized_choice; a "
                       "uniform within about 2^-21 of a cdf boundary may name the neighbouring row)" % prio if prio else "")
                    + ("; the minibatches of brains %s by Memory.sample's stratified walk on random.random()'s uniforms, the sum tree kept on the "
                       "device in float64 with the reference's rounding order (learn_reference_td=True: rl_learn_td_tree_store, "
                       "rl_learn_td_tree_sample, rl_learn_td_tree_update; a draw that the reference would repeat ends the run)" % td if td else "")
                    + ("; brains %s as loaded / initialised (their kinds do not learn in this mode)" % frozen if frozen else ""))
        frozen = [k for k in range(len(self.brains)) if k not in self.learners]
        by = {name: [k for k in sorted(self.learners) if self.learners[k].spec is ENTRY[name]] for name in self._NOTES}
        note = []
        for name, ks in by.items():
            if ks:
                ls = [self.learners[k] for k in ks]
                note.append("brains %s trained on the device (%s: %s)" % (ks, name, self._NOTES[name][1] % dict(
                    steps=self._steps(ENTRY[name].family), batch=sorted({l.batch for l in ls}), wide=self.learn_batch_of.get(ENTRY[name].method),
                    k_epoch=sorted({getattr(l, "k_epoch", None) for l in ls}), every=self.learn_every)))
        if frozen:
            note.append("brains %s as loaded / initialised (their kinds do not learn in this %s)"
                        % (frozen, "run" if any(ks and self._NOTES[name][0] for name, ks in by.items()) else "build"))
        uniform = sorted(k for name, ks in by.items() if not ENTRY[name].draw for k in ks)
        uniform = [k for k in uniform if self.learn_draw_of.get(self.learners[k].spec.method) == "rank"]
        if uniform:
            note.append("the minibatches of brains %s drawn by content-key rank (learn_draw=%r, rl_learn_draw_rank: the ring's rows sorted by "
                        "content key, draw d the row at rank (x_d * size) >> 32 -- uniform with replacement, other rows than rl_learn_draw names)"
                        % (uniform, self.learn_draw))
        for method, entry, how in (("PERD3QN", "rl_learn_prioritized_draw_rank", "independent draws u_d * total, as np.random.choice's"),
                                   ("PERDQN", "rl_learn_td_draw_rank", "stratified, draw j at (j + u_j) * total / batch: the reference's Memory.sample(), "
                                    "not the independent draws the note above states")):
            ks = [k for k in sorted(self.learners) if self.learners[k].spec.method == method]
            entry = next((self.learners[k].spec.draw_rank for k in ks if self.learners[k].spec.draw_rank), entry)   # (a wide learner's own)
            if ks and self.learn_draw_of.get(method) == "rank":
                note.append("the minibatches of brains %s drawn by prefix sum over content-key rank (learn_draw=%r, %s: the ring's rows sorted by "
                            "content key, their weights summed in that order in float64, every draw the smallest rank whose sum exceeds its target -- "
                            "%s; other rows than the race draw names)" % (ks, self.learn_draw, entry, how))
        if self.learn_td_stamp:   # (a clause more only where the keyword was given: every other run's note is what it was)
            note.append("the new rows of brains %s get (|Q(s)[a] - (r + (1 - done) gamma max_a Q_target(s'))| + 0.01) ** 0.6, their TD error's "
                        "priority from the parameters as of the learning call that first draws them, not the one priority the note above states "
                        "(learn_td_stamp=%r, rl_learn_td_stamp: this build's own, a departure from PERDQN.py:113-128 on purpose)"
                        % ([k for k in sorted(self.learners) if self.learners[k].spec.family == "td"], self.learn_td_stamp))
        if self.learn_ranks:
            note.append("%d rank(s) trained independently on their own rings and averaged params, adam_m and adam_v over the ranks with the "
                        "highest step count after every learning episode (learn_ranks='average': periodic parameter averaging, this build's own)"
                        % self.world_size)
        return "; ".join(note)

    def _decay_epsilon(self, ls, n):
        """train_model()'s epsilon decay on the host, once per update the PERDQN learners `ls` made in a call of `n` steps."""
        for l in ls:
            if not l.trained_from:   # (a read-back: only until the ring first holds train_start rows)
                l.trained_from = min(int(l.ring["count"].item()), int(l.ring["state"].shape[0])) >= l.train_start
            if l.trained_from:       # train_model(): epsilon loses epsilon_decay at the start of every update while above epsilon_min
                for _ in range(n):
                    if l.brain.epsilon > l.brain.epsilon_min:
                        l.brain.epsilon -= l.brain.epsilon_decay

    # learn_now, per family in learn.FAMILIES' order: D3QNAgent.learn's schedule (the exploration gate and the target rule)?  the draw
    # (None: the uniform draws, draw_slots or draw_slots_rank); one call per batch size (else ONE call)?  what follows a call
    _SCHEDULE = (("dqn", False, None, False, None), ("dueling", True, None, True, None), ("prioritized", True, "draw_prioritized", True, None),
                 ("ppo", False, "draw_rollout", False, None), ("td", False, "draw_td", True, _decay_epsilon))
    assert tuple(s[0] for s in _SCHEDULE) == FAMILIES

    def learn_now(self, last=None):
        """One DQNAgent.train() (DQN.py:80-83) for every DQN learner, queued behind the ticks launched so far (DeviceWorlds.learn).  The
        minibatches are drawn by the rows' content (DeviceWorlds.draw_slots): the rings' order differs from run to run, the run does not.
        D3QN learners (learn_kinds) train in a call of their own behind it -- the DQN learners' call and draws are what they are without
        them: D3QNAgent.learn's schedule (D3QN.py:118-126) at this build's granularity.  `last` is the episode just finished: a learner
        trains only once last > brain.exploration, and its target is synced in this call iff a multiple of brain.soft_update_freq lies
        in (last - learn_every, last].  last=None: every D3QN learner trains, sync_target as the learner holds it.
        Prioritised PERD3QN learners (learn_prioritized=True) follow on the same schedule (PERD3QN.py:117-125 is D3QN.py:118-126), behind
        the DQN and D3QN calls, which stay what they are without them: one prioritised draw (DeviceWorlds.draw_prioritized, two launches)
        and one rl_learn_prioritized, ONE update per call as PERD3QNAgent.train() makes.
        PPO learners (learn_rollout=True) come last, behind those calls, which again stay what they are without them: one on-policy draw
        (DeviceWorlds.draw_rollout, two launches) and one rl_learn_ppo of `rollout_steps` rollouts (PPO.learn(), PPO.py:136-162), on
        every call -- PPO has no exploration gate; a window without fresh rows makes no update.
        PERDQN learners (learn_td_priority=True) come behind the PPO call, and all earlier calls stay what they are without them: one draw
        (DeviceWorlds.draw_td, two launches) and one rl_learn_td of learn_steps["PERDQN"] (1) updates, on every call -- the reference has no
        exploration gate; below brain.train_start rows the call only copies model -> target_model (PERDQNAgent.learn).  train_model()'s
        epsilon decay follows on the host: once per update made.  Whether a call trained depends on the ring's count, which lives on the
        device: it is read back once per call until it first reaches train_start (it never falls again) -- these early calls SYNCHRONISE
        with the device; later ones do not.
        learn_batch=B: the DQN learners are wide ones (rl_learn_wide, minibatches of B rows in 32-row tiles side by side) and are called in
        the DQN learners' place, the same way: draw (draw_slots: the same flat table, so B = 32 trains on rl_learn's rows), then learn,
        learn_steps steps -- 2 learn_steps + 3 launches instead of one.
        learn_batch={"D3QN": B}: the D3QN learners are wide ones (rl_learn_dueling_wide, minibatches of B rows in 64-row tiles side by side,
        the advantage mean of the whole batch) and are called in the D3QN learners' place, the same way -- schedule, gate, draw, target
        rule --, 3 learn_steps["D3QN"] + 3 launches instead of one; B = 64 trains on rl_learn_dueling's rows and ends with its bits.
        learn_batch={"PERD3QN": B} (with learn_prioritized=True): the PERD3QN learners are wide ones (rl_learn_prioritized_wide, minibatches
        of B rows in 64-row tiles, the priorities of all B rows rewritten and their maximum kept) and are called in the PERD3QN learners'
        place, the same way -- gate, target rule, ONE step, draw (rl_learn_prioritized_wide_draw, two launches) then learn (6 launches
        instead of one) --, behind the DQN and D3QN calls; B = 64 draws rl_learn_prioritized's rows and ends with its bits, priorities and
        prio_max included.
        learn_batch={"PPO": B} (with learn_rollout=True): the PPO learners are wide ones (rl_learn_ppo_wide, rollouts of B rows in 32-row
        tiles, one GAE recursion over the whole rollout) and are called in the PPO learners' place, the same way -- no gate but the empty
        window, `rollout_steps` rollouts, draw (rl_learn_rollout_wide, two launches) then learn (3 rollout_steps k_epoch + 3 launches
        instead of one) --; B = 32 draws rl_learn_rollout's rows and ends with rl_learn_ppo's bits.
        learn_batch={"PERDQN": B} (with learn_td_priority=True): the PERDQN learners are wide ones (rl_learn_td_wide, minibatches of B rows
        in 64-row tiles, the importance weights' minimum and mean over the whole batch from a pass in front of every step's tiles, the
        priorities of all B rows rewritten) and are called in the PERDQN learners' place, the same way -- the train_start gate, the target
        copy at every call, learn_steps["PERDQN"] steps, the stamp in front where learn_td_stamp asks for it, draw (rl_learn_td_wide_draw,
        two launches, or with learn_draw={"PERDQN": "rank"} rl_learn_td_wide_draw_rank, eight launches, stratified at B) then learn
        (3 learn_steps["PERDQN"] + 3 launches instead of one), the epsilon decay --; B = 64 draws rl_learn_td's rows and ends with its
        bits, priorities and beta included.
        learn_draw="rank": the draw_slots calls above -- the DQN, wide DQN and D3QN learners' -- are draw_slots_rank calls (rl_learn_draw_rank,
        six launches instead of two: the rings' rows sorted by content key once, every draw an index into that order); the prioritised,
        rollout and PERDQN draws are what they are.
        learn_draw={"PERD3QN": "rank"}: the prioritised draw is a draw_prioritized_rank call (rl_learn_prioritized_draw_rank, eight launches
        instead of two: the same stamp, the sort, the weights' cumulative sum in rank order, one search per draw -- independent draws, as
        np.random.choice's) at any learn_batch["PERD3QN"]; learn_draw={"PERDQN": "rank"}: the PERDQN draw is a draw_td_rank call
        (rl_learn_td_draw_rank, eight launches, STRATIFIED: the reference's Memory.sample()).  {"DQN": "rank"} / {"D3QN": "rank"}: the string,
        for that kind alone.  Other rows than the race draws name; without the key every call is what it was.
        learn_td_stamp="error": one DeviceWorlds.stamp_td (rl_learn_td_stamp, two launches) is queued in front of the PERDQN draw, the race
        draw and the rank draw alike: the rows appended since the last draw get their TD error's priority from the parameters as they
        stand at this call, the draw stamps nothing.  Without the key every call is what it was.
        learn_ranks="average": all of the above is rank-local and unchanged; the call then ends with the merge of ALL learners over the
        ranks (_merge_learners: one launch to export, ONE all-gather, two launches to merge) -- this build's own, periodic parameter
        averaging: D3QN, PERD3QN and PERDQN learners make one update per call from identical parameters and moments, so the merged
        result is the mean of the ranks' one-step Adam updates; DQN makes learn_steps local steps and PPO k_epoch per rollout in between."""
        self.learn_now_calls += 1
        called = []
        for family, scheduled, draw, per_batch, after in self._SCHEDULE:   # (learn_batch: a family's learners are all wide, or none is)
            ls = [self.learners[k] for k in sorted(self.learners) if self.learners[k].spec.family == family
                  and (not scheduled or last is None or last > self.learners[k].exploration)]
            n = self._steps(family)
            # (one call per batch size: a call's slot table is rectangular)
            for ls in ([[l for l in ls if l.batch == batch] for batch in sorted({l.batch for l in ls})] if per_batch else [ls] if ls else []):
                if scheduled and last is not None:
                    for l in ls:
                        l.sync_target = last // l.soft_update_freq > max(last - self.learn_every, 0) // l.soft_update_freq
                ranked = "_rank" if self.learn_draw_of.get(self._DRAW_FAMILY.get(family)) == "rank" else ""   # (draw_td_rank: stratified by default)
                if family == "td" and self.learn_td_stamp:   # (the draw behind it, whichever it is, then finds no fresh row)
                    self.worlds.stamp_td(ls)
                self.worlds.learn(ls, n, slots=getattr(self.worlds, (draw or "draw_slots") + ranked)(ls, n))
                called += ls
                if after:
                    after(self, ls, n)
        if self.learn_ranks:
            self._merge_learners(called)

    def sync_learners(self):
        """The trained parameters into the brains' modules (DeviceLearner.sync_to_module): what Saver and state_dict() read."""
        for l in self.learners.values():
            l.sync_to_module()

    # -- fused loop ----------------------------------------------------------------------------------------------------
    def run(self, n_epi=0, n_ticks=1, max_chunk=4096):
        """`n_ticks` iterations of the trainer loop (trainer.py:85-99: get_action for every agent -> step -> update_env) starting at
        episode `n_epi`, with as few launches as the configuration allows: rng="philox" runs whole chunks in ONE launch each
        (rl_run_ex: worlds resident in LDS, the brains' per-episode epsilon as a schedule, the Tracker's statistics accumulated in the
        launch); chunks end where the reference's Tracker closes an interval (n_epi % update_interval == 0, tracker.py:107-121); episode
        0's statistics never reach an aggregate (tracker.py:279-282) and are left out inside the launch.  Same results as calling
        act() / step() / update_env() tick by tick (tests/test_hip_round3.py).
        learn="device": chunks also end at the episodes that are multiples of learn_every, and behind each such chunk the minibatch draw (two launches)
        and ONE rl_learn for all learners are queued on the same stream (learn_now) -- this build's schedule, not the reference's per-agent one."""
        if self.rng != "philox":
            for t in range(n_ticks):
                self.act(n_epi + t); self.step()
                if self.learn == "reference":
                    self.learn_reference(n_epi + t)
                self.update_env(n_epi + t)
            return
        interval = self.tracker.update_interval
        thr = -1 if self.refill_below is None else self.refill_below
        while n_ticks > 0:
            k = min(n_ticks, max_chunk)
            if self.training and n_epi + k - 1 >= interval:   # up to and including the next episode that closes a Tracker interval
                k = min(k, (max(n_epi, 1) + interval - 1) // interval * interval - n_epi + 1)
            if self.learners:   # ... and the next episode after which the brains train
                k = min(k, (max(n_epi, 1) + self.learn_every - 1) // self.learn_every * self.learn_every - n_epi + 1)
            eps = self._epsilon_schedule(n_epi, k)
            self._bind_brains()   # (the brains' current epsilon = the last row; weights are uploaded only when they changed)
            if self.training and n_epi == 0:
                # Tracker.update_results(n_epi=0) zeroes the running sums (tracker.py:279-282): whatever an earlier loop on this
                # environment left in them goes, and episode 0 itself stays out of them inside the launch (trk_skip)
                self.worlds.reset_tracking()
            self.worlds.run(k, thr, self.synthetic_agents or 0, eps_schedule=None if (eps == eps[-1]).all() else eps,
                            trk_skip=1 if (self.training and n_epi == 0) else 0)
            # The interval the PREVIOUS chunk closed: its sums (and the error flag) were copied out behind that chunk; the host
            # reads, divides and prints them now, with this chunk queued -- the device does not wait for any of it.
            self.tracker.resolve()
            self._refresh(after="update")
            last = n_epi + k - 1
            if self.learners and last > 0 and last % self.learn_every == 0:
                self.learn_now(last)
            if self.training and last > 0 and last % interval == 0:
                self.tracker.update_results(None, last, defer=True)   # the device half of the close: queued behind the chunk
            n_epi += k
            n_ticks -= k
        self.tracker.resolve()   # (a close behind the last chunk: a corrupted world stops the loop here at the latest)

    # -- host mirrors ----------------------------------------------------------------------------------------------------
    def agents_of(self, world):
        """env.agents of replica `world` (row-major list of AgentView): the same protocol as env.agents, which is world 0's.
        Views are valid until the next step() / update_env() / run()."""
        if not 0 <= world < self.n_worlds:
            raise IndexError("world %d of %d" % (world, self.n_worlds))
        return self._mat(world).views

    def _sync(self):
        torch.cuda.synchronize(self.worlds.device)
        self.worlds.check_error_flag()

    def _snapshot(self):
        """The device state on the host behind everything queued so far: ONE copy and ONE wait for a small handle (DeviceWorlds.snapshot);
        the error flag comes with it."""
        snap = self.worlds.snapshot()
        self.worlds.raise_on_error_flag(snap["err"])
        self._ticks_since_check = 0
        return snap

    def _build_mirror(self, world, snap):
        m = _WorldMirror(self, world, self._phase)
        n = m.n = int(snap["n_agents"][world])
        if world == 0 and "max_gene" in snap:
            self._max_gene = int(snap["max_gene"][0])
        m.host = {k: snap[k][world, :n] for k in _A_FIELDS}
        if self._phase == "step":
            m.src1, m.reward, m.done = snap["src1"][world], snap["reward"][world, :n], snap["done"][world, :n]
        if self._phase == "update" and self._acted:   # act() has run: what the policy chose for this tick (and what it computed)
            m.actions = snap["actions"][world].copy()
            m.q = snap["out_q"][world]
        else:                                          # Agent.action: the action last taken (-1 for newborns)
            m.actions = np.concatenate([m.host["a_action"], np.full(self.worlds.cap - n, -1, np.int8)])
        self._mirrors[world] = m   # (before the views: AgentView looks its mirror up)
        m.views = [AgentView(self, k, m) for k in range(n)]
        return m

    def _mat(self, world):
        """The host mirror of one world, built from the device state on first use."""
        m = self._mirrors.get(world)
        if m is None:
            w = self.worlds
            if hasattr(w, "snapshot") and w._arena.numel() <= w.SNAPSHOT_MAX_BYTES:
                m = self._build_mirror(world, self._snapshot())
            else:   # a big handle: this world's rows only
                self._sync()
                n = int(w.s["n_agents"][world].item())
                snap = {k: w.s[k][world:world + 1, :n].cpu().numpy() for k in w.s if k.startswith("a_")}
                snap["n_agents"] = np.array([n])
                for k in ("src1", "reward", "done", "actions", "out_q"):
                    snap[k] = getattr(w, k)[world:world + 1].cpu().numpy()
                snap = {k: _Shift(v, world) for k, v in snap.items()}   # (a plain dict: keys() / [] like a snapshot)
                m = self._build_mirror(world, snap)
        if m.actions is None:          # act() ran after this mirror was built: what the policy chose for this tick
            m.actions = self.worlds.actions[world].cpu().numpy().copy()
        return m

    def _refresh(self, after):
        """The device state changed: drop every host copy (they are rebuilt on first read -- no synchronisation here)."""
        self._phase = after
        self._acted = False
        self._mirrors = {}
        self._grid = self._max_gene = None
        self._stamp += 1
        if after != "step":
            self._n_empty = None


class _Shift:
    """A one-world slice that answers to the world's index in the full array (big handles: Environment._mat)."""

    def __init__(self, a, world):
        self.a, self.world = a, world

    def __getitem__(self, key):
        if isinstance(key, tuple):
            assert key[0] == self.world
            return self.a[(0,) + key[1:]]
        assert key == self.world
        return self.a[0]


def resolve_dist(dist=None):
    """(process-group module or None, rank, world size): `dist` as given (torch.distributed or a stand-in with the same calls), else
    torch.distributed when a default process group is initialised, else a single-process job."""
    if dist is None:
        import torch.distributed as td
        if td.is_available() and td.is_initialized():
            dist = td
    if dist is not None and dist.is_initialized():
        return dist, int(dist.get_rank()), int(dist.get_world_size())
    return None, 0, 1


def warn_inference_only(frozen=None, kinds=("DQN",), draw=None, mode="device"):
    import warnings
    if frozen is not None and mode == "reference_prioritized":
        warnings.warn("learn='reference' with learn_reference_prioritized=True trains the %s and PERD3QN brains of this run; brains %s are of "
                      "other kinds: they stay inference only -- brain.learn() is a no-op for them and their weights are NOT updated (a PERDQN "
                      "memory's sum tree accumulates rounding in update order and append_sample makes forward passes per store: PERDQN brains do "
                      "not train in this mode yet; learn='device' trains them on its own schedule)."
                      % (", ".join(kinds), ", ".join(frozen)), stacklevel=4)
        return
    if frozen is not None and mode == "reference_td":
        warnings.warn("learn='reference' with learn_reference_td=True trains the %s brains of this run; brains %s are of other kinds: they "
                      "stay inference only -- brain.learn() is a no-op for them and their weights are NOT updated (PERD3QN brains train in this "
                      "mode with learn_reference_prioritized=True; learn='device' trains them on its own schedule)."
                      % (", ".join(kinds[:-1]) + " and " + kinds[-1], ", ".join(frozen)), stacklevel=4)
        return
    if frozen is not None and mode == "reference":
        warnings.warn("learn='reference' trains the %s brains of this run; brains %s are of other kinds: they stay inference only -- "
                      "brain.learn() is a no-op for them and their weights are NOT updated (PERD3QN and PERDQN memories need their priorities on "
                      "the host for the reference's draws: they do not train in this mode yet; learn='device' trains them on its own schedule)."
                      % (", ".join(kinds[:-1]) + " and " + kinds[-1], ", ".join(frozen)), stacklevel=4)
        return
    if frozen is not None:
        # (a line more only where learn_draw was given: every other run's message is what it was)
        drawn = "" if draw is None else "\nlearn_draw=%r draws the DQN / D3QN learners' minibatches by content-key rank (rl_learn_draw_rank)." % (draw,)
        if isinstance(draw, dict):
            how = {"DQN": "DQN learners' uniformly by content-key rank (rl_learn_draw_rank)", "D3QN": "D3QN learners' uniformly by content-key rank (rl_learn_draw_rank)",
                   "PERD3QN": "PERD3QN learners' by priority through a prefix sum over content-key rank, independent draws (rl_learn_prioritized_draw_rank)",
                   "PERDQN": "PERDQN learners' by priority through a prefix sum over content-key rank, stratified (rl_learn_td_draw_rank)"}
            drawn = "\nlearn_draw=%r draws the minibatches: the %s." % (draw, "; the ".join(how[k] for k in how if k in draw))
        if tuple(kinds) == ("DQN",):
            warnings.warn("learn='device' trains the DQN brains of this run; brains %s are of kinds rl_learn does not train yet: they stay "
                          "inference only -- brain.learn() is a no-op for them and their weights are NOT updated (D3QN brains learn with "
                          "learn_kinds=('DQN', 'D3QN'), PERD3QN brains with learn_prioritized=True, PPO brains with learn_rollout=True; PERDQN brains do "
                          "not learn yet)." % ", ".join(frozen) + drawn, stacklevel=3)
        else:
            warnings.warn("learn='device' trains the %s brains of this run; brains %s are of other kinds (or of kinds no entry point trains): they stay "
                          "inference only -- brain.learn() is a no-op for them and their weights are NOT updated." % (" and ".join(kinds), ", ".join(frozen)) + drawn,
                          stacklevel=3)
        return
    warnings.warn("reinlife_amd runs ReinLife's per-tick path (world tick + policy inference) only: training=True keeps the "
                  "reference's loop, epsilon schedules and Tracker, but brain.learn() is a no-op and the brains' weights are NOT "
                  "updated; results saved from such a run hold the initial (untrained) weights.  Train with the reference, or feed "
                  "DeviceWorlds.enable_capture() / capture_transitions() to your own learner.", stacklevel=3)


def host_reset(width, height, n_brains, rng=None):
    """Environment.reset's world construction with the reference's exact global-np.random draw order
    (environment.py:147-154 -> _add_agent :483-484 -> Grid.set_random grid.py:69-83; _init_food :741-761).  `rng`: a
    np.random.RandomState to draw from instead of the process-global generator (replicas other than world 0)."""
    rnd = rng if rng is not None else np.random
    C = width * height
    grid = np.zeros(C, np.uint8)
    agents = []

    def set_random(kind, p):
        empties = np.nonzero(grid == _lib.EMPTY)[0]  # row-major, like np.where on the 2-D grid
        if len(empties) == 0:
            return None
        k = rnd.randint(0, len(empties))
        if rnd.random_sample() < p:
            grid[empties[k]] = kind
            return int(empties[k])
        return None

    for g in range(n_brains):
        cell = set_random(_lib.AGENT, 1.0)
        if cell is not None:
            agents.append((cell, g))
    for kind, prob in ((_lib.FOOD, 0.1), (_lib.POISON, 0.05)):
        for _ in range(C):
            if rnd.random_sample() < prob:
                set_random(kind, 1)
    set_random(_lib.SUPER_FOOD, 1)
    order = sorted(range(len(agents)), key=lambda a: agents[a][0])
    n = len(agents)
    cells = np.array([agents[a][0] for a in order], dtype=np.int64).reshape(n)
    snap = {"cell_type": grid,
            "i": (cells // width).astype(np.uint8), "j": (cells % width).astype(np.uint8),
            "health": np.full(n, 200, np.int32), "age": np.zeros(n, np.int32), "max_age": np.full(n, 50, np.int32),
            "gene": np.array([agents[a][1] for a in order], np.int32).reshape(n),
            "brain": np.array([agents[a][1] for a in order], np.int32).reshape(n),
            "uid": np.array(order, np.int32).reshape(n), "flags": np.zeros(n, np.uint8), "action": np.full(n, -1, np.int8),
            "fitness": np.zeros(n, np.float64), "max_gene": n_brains, "next_uid": n,
            "best_uid": np.full(_lib.N_BEST, -1, np.int32), "best_fit": np.zeros(_lib.N_BEST), "best_brain": np.zeros(_lib.N_BEST, np.int32)}
    return snap
