/* reinlife_hip.h -- C ABI of libreinlife_hip.so: the MI355X (gfx950) implementation of ReinLife's hot path.
 *
 * The reference (MaartenGr/ReinLife v1.0.1) is pure Python and has no FFI; this ABI is what a binding for its
 * per-tick path would call.  Each entry point names the reference code it replaces (paths under ReinLife/):
 *
 *   rl_step            Environment.step()                         World/environment.py:160-186
 *   rl_update          Environment.update_env() minus the Tracker World/environment.py:188-215
 *   rl_tick            step() + update_env() of one trainer-loop iteration, fused (Helpers/trainer.py:92,99)
 *   rl_observe         Environment._get_observations()            World/environment.py:313-375
 *   rl_reset_synthetic Environment.reset()-style world generator  World/environment.py:133-158, 741-761
 *   rl_reset_families  Environment.reset() itself (one agent per brain) World/environment.py:133-158
 *   rl_policy_act      Agent.get_action() over all agents         World/entities.py:215-222 ->
 *                      DQN.py:126-139, D3QN.py:161-173, PERD3QN.py:198-210, PPO.py:101-106,164-169,
 *                      PERDQN.py:101-111,311-323
 *   rl_policy_forward  the bare network forward of one brain on a dense batch of observation rows
 *   rl_render          Visualize.render()'s drawing of one frame, for any set of worlds     Helpers/render.py:51-239
 *   rl_learn           DQNAgent.train(): the size gate, 5 minibatch updates (smooth-L1, Adam) and the target copy
 *                      Models/DQN.py:80-83, 142-153 (sampling: :99-113, with replacement here)
 *   rl_learn_wide      the same update on minibatches of up to 2048 rows, 32-row tiles side by side (DQN.py:80-83, 142-153)
 *   rl_learn_dueling_wide  D3QNAgent.train() on minibatches of up to 2048 rows, 64-row tiles side by side, the batch-wide mean kept
 *   rl_learn_draw_rank this build's own: the minibatch tables of rl_learn / rl_learn_wide / rl_learn_dueling drawn uniformly by the
 *                      rows' content-key rank (one sort per call, one thread per draw)
 *   rl_learn_prioritized_draw_rank / rl_learn_td_draw_rank  this build's own: the prioritised minibatch tables of PERD3QN.py:157-165 and
 *                      PERDQN.py:280-304 (stratified) drawn by a prefix sum of the weights in content-key rank order, one search per draw
 *   rl_learn_td_stamp  this build's own: the rows appended since the last draw get the TD-error priority PERDQN.py:113-128 spells out
 *                      and does not compute (a forward pass of both networks per fresh row)
 *   rl_learn_ppo       PPO.learn(): k_epoch full-batch Adam steps on a rollout of at most 32 rows (rl_learn_rollout draws it)
 *   rl_learn_ppo_wide  PPO.learn() on a rollout of up to 2048 rows, 32-row tiles side by side, ONE GAE recursion over the whole rollout
 *                      (rl_learn_rollout_wide draws it)
 *   rl_learn_td_wide   PERDQNAgent.train_model() on a minibatch of up to 2048 rows, 64-row tiles side by side, the importance weights'
 *                      minimum and mean over the whole batch from a pass of its own in front of every step's tiles
 *   rl_learn_dueling   D3QNAgent.train(): one minibatch update of the dueling network (MSE, Adam), batch up to 64
 *                      Models/D3QN.py:97-116, 148-165 (schedule and target copy of :118-126: the caller's)
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types.  `stream` is a hipStream_t passed as void*.
 *   - The CALLER owns every device buffer (e.g. torch tensors) and the stream; the library allocates no device
 *     memory, starts no threads and never synchronises the device.  A handle is not thread-safe; distinct handles
 *     are independent.
 *   - Every function returns 0 on success or a negative rl_status; rl_last_error() gives the message (thread-local).
 *   - World state is struct-of-arrays over `n_worlds` independent worlds.  A world's agent list is ALWAYS its
 *     on-grid agents in row-major cell order (= Grid.get_entities order, World/grid.py:60-67), so index k is index
 *     k of the reference's env.agents.
 *   - Randomness: either a recorded tape of the reference's draws (parity mode) or Philox4x32-10 keyed
 *     (seed, epoch, world, tick, site, index) generated in-kernel (performance mode).  See DESIGN.md.
 */
#ifndef REINLIFE_HIP_H
#define REINLIFE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libreinlife_hip.so is built with -fvisibility=hidden: the declarations between this push and the pop at the end of the file ARE its
 * export list (tests/test_abi_cpu.py compares the library's dynamic symbol table with them). */
#pragma GCC visibility push(default)

#define RL_OBS_DIM 153   /* Environment.observation_space, environment.py:119 */
#define RL_N_ACTIONS 8   /* Environment.action_space, environment.py:118; World/utils.py:4-17 */
#define RL_N_BEST 10     /* len(best_agents), environment.py:149 */
#define RL_FOOD_TRIES 7  /* 3 Food + 3 Poison + 1 SuperFood set_random calls, environment.py:763-776 */
#define RL_MAX_CELLS 4096
#define RL_MAX_BRAINS 64
#define RL_TRK_VARS 7

typedef enum {
    RL_OK = 0, RL_E_INVALID = -1, RL_E_UNBOUND = -2, RL_E_LAUNCH = -3, RL_E_UNSUPPORTED = -4
} rl_status;

/* cell codes: World/utils.py:20-33 (kin = 4 is never placed on the grid) */
enum { RL_EMPTY = 0, RL_FOOD = 1, RL_POISON = 2, RL_AGENT = 3, RL_KIN = 4, RL_SUPER_FOOD = 5 };
/* a_flags bits (Agent booleans, World/entities.py:150-159) */
enum { RL_F_DEAD = 1, RL_F_REPRODUCED = 2, RL_F_KILLED = 4, RL_F_ATE_SUPER = 8, RL_F_INTER_KILLED = 16,
       RL_F_INTRA_KILLED = 32 };
/* brain kinds (BasicBrain.method, Models/utils.py:1-14) */
enum { RL_DQN = 0, RL_D3QN = 1, RL_PERD3QN = 2, RL_PPO = 3, RL_PERDQN = 4 };
/* Philox draw sites */
enum { RL_SITE_FOOD = 1, RL_SITE_REPRO = 2, RL_SITE_BIRTH = 3, RL_SITE_PRODUCE = 4, RL_SITE_ACT = 5,
       RL_SITE_RESET_AGENT = 6, RL_SITE_RESET_FOOD = 7, RL_SITE_RESET_POISON = 8, RL_SITE_RESET_SUPER = 9, RL_SITE_LEARN = 10,
       RL_SITE_LEARN_PRIO = 11, RL_SITE_LEARN_ROLLOUT = 12, RL_SITE_LEARN_TD = 13 };

/* keyword arguments of Environment(...) that matter on the path (environment.py:74-89) */
typedef struct {
    int32_t width, height;
    int32_t max_agents;
    int32_t n_brains;            /* len(brains) */
    int32_t slot_cap;            /* capacity of the per-world agent arrays; multiple of 64, >= 2*max_agents+2, <= 4096 */
    int32_t n_worlds;            /* independent replicas on this GPU, < 2^19 */
    int32_t static_families, limit_reproduction, incentivize_killing;
    int32_t world_base;          /* global id of world 0 (replica sharding across GPUs): Philox uses world_base + w */
    uint64_t seed;               /* Philox key */
} rl_config;

/* Device pointers, all caller-owned.  Shapes: R = n_worlds, C = width*height, cap = slot_cap. */
typedef struct {
    uint8_t* cell_type;   /* [R][C]   Grid.get_numpy() */
    int32_t* n_agents;    /* [R]      len(env.agents) */
    uint8_t* a_i;         /* [R][cap] Agent.i */
    uint8_t* a_j;         /* [R][cap] Agent.j */
    int32_t* a_health;    /* [R][cap] */
    int32_t* a_age;
    int32_t* a_max_age;
    int32_t* a_gene;
    int32_t* a_brain;     /* index into the brains list the agent's brain descends from */
    int32_t* a_uid;       /* creation-order id within the world (object identity in the reference) */
    uint8_t* a_flags;
    int8_t* a_action;     /* last action taken, -1 for newborns (entities.py:153) */
    double* a_fitness;    /* Agent.fitness (float64 sum of rewards, entities.py:189) */
    int32_t* max_gene;    /* [R] Environment.max_gene */
    int32_t* next_uid;    /* [R] */
    int32_t* tick;        /* [R] ticks since the last reset (Philox counter) */
    int32_t* epoch;       /* [R] resets so far (Philox key) */
    int32_t* best_uid;    /* [R][10] Environment.best_agents (non-static families) */
    double* best_fit;     /* [R][10] */
    int32_t* best_brain;  /* [R][10] */
} rl_state;

/* One tick of recorded reference draws (device pointers).  food_k == NULL => Philox. */
typedef struct {
    const int32_t* food_k;         /* [R][7]     np.random.randint results of _add_food's set_random calls */
    const double* food_u;          /* [R][7]     their np.random.random coins */
    const double* repro_u;         /* [R][cap]   random.random() gate of the k-th eligible agent (env.py:501) */
    const int32_t* birth_k;        /* [R][cap+1] np.random.randint result of the b-th birth placement */
    const double* produce_u;       /* [R]        random.random() gate of _produce (env.py:528) */
    const int32_t* produce_choice; /* [R]        static: chosen gene (env.py:536/538); else best_agents index (:544) */
} rl_tape;

/* Outputs of a step, indexed in the POST-step env.agents order.  Any pointer may be NULL. */
typedef struct {
    int32_t* n_acted;   /* [R]       agents that acted = agent-steps of this tick */
    float* reward;      /* [R][cap]  Agent.reward */
    uint8_t* done;      /* [R][cap]  Agent.done */
    int16_t* src;       /* [R][cap]  index of the agent in the PRE-step list (its state/action live there) */
    float* obs;         /* [R][cap][153] Agent.state_prime */
    unsigned long long* acted_total; /* [1] running sum of n_acted over worlds and calls (metric counter) */
    /* Tracker accumulators (Helpers/tracker.py:178-282), all or none.  G = n_brains (static families) or 1 groups x
     * RL_TRK_VARS variables [size, age, fitness, best age, attacks, kills, intra kills] over the post-step env.agents;
     * a per-tick value enters sum/cnt iff it is > -1, exactly like Tracker._aggregate. */
    double* trk_tick;   /* [R][G][7] this tick's values (-1 = no result) */
    double* trk_sum;    /* [R][G][7] running sum of valid values (caller zeroes it at interval boundaries) */
    int32_t* trk_cnt;   /* [R][G][7] number of valid ticks */
    double* trk_pop;    /* [R][3]    "Avg Number of Populations": this tick, running sum, running count */
    /* post-step list attributes that a fused rl_tick would otherwise lose (needed by rl_capture_transitions) */
    int32_t* n_post;    /* [R]       length of the post-step list (len(env.agents) after step()) */
    int32_t* age;       /* [R][cap]  Agent.age after the step */
    int32_t* brain;     /* [R][cap]  brains-list index of the agent's brain */
} rl_step_out;

/* Outputs of an update, indexed in the POST-update env.agents order. */
typedef struct {
    int16_t* src;       /* [R][cap]  index in the post-step list, -1 for newborns */
    float* obs;         /* [R][cap][153] Agent.state (what the policy reads next tick) */
} rl_update_out;

/* Replay ring of ONE brain (caller-owned device buffers): what Agent.learn hands to brain.learn each tick
 * (World/entities.py:194-208 -> DQN.py:73-84, D3QN.py:94-96, PERD3QN.py:91-92,117-125, PPO.py:69-76), stored in
 * slot (count % capacity) in Agent.learn call order per world.
 *   The contract of the two writers (rl_capture_transitions, and rl_run_ex with `replays`):
 *   count     *count after a launch == *count before + the rows appended.  It only grows (64 bits); the slot is count mod capacity.
 *   one world row n of a launch's call-order list sits in slot (count0 + n) % capacity, later rows over earlier ones: the reference's
 *             deque(maxlen=capacity).
 *   worlds    every (world, tick) list is reserved by ONE atomic on *count and is one contiguous run of slots in call order; the worlds'
 *             runs of a tick follow each other in the order their workgroups reach the counter.  A launch that appends at most
 *             `capacity` rows leaves every slot outside [count0, count0 + rows) % capacity untouched.
 *   floor     capacity >= n_worlds * slot_cap, the most rows ONE tick of all worlds can append to one ring: both entry points refuse a
 *             smaller ring (RL_E_INVALID naming the ring, its capacity and the floor) before anything is launched.  Below the floor two
 *             rows of one tick map to the same slot; they are written by different threads (across worlds: different workgroups), each
 *             row in parts, and nothing orders those writes -- the slot could end as the state of one transition with the reward or
 *             state_prime of another.
 *   assumed   the floor keeps the rows of ONE tick apart, not those of different ticks: inside a multi-tick launch the worlds are not in
 *             lockstep, and a world that has reserved its slots must finish writing that tick's rows before the other worlds have
 *             appended a whole further ring's worth of rows (capacity rows beyond its reservation) and reach the same slots again.  The
 *             kernel does not guarantee that; a ring of several ticks' rows (the reference's sizes: 10,000 and up) makes it a matter of
 *             one world stalling for that many ticks of all the others. */
typedef struct {
    float* state;                /* [capacity][153] observation the policy read before the step */
    float* state_prime;          /* [capacity][153] post-step observation */
    int8_t* action;              /* [capacity] */
    float* reward;               /* [capacity] raw Agent.reward (the PPO brain divides by 100 itself, PPO.py:71) */
    uint8_t* done;               /* [capacity] */
    float* prob;                 /* [capacity] policy output of the taken action (PPO: prob[action]) if outputs are given */
    int32_t* age;                /* [capacity] post-step age (train_freq logic, e.g. DQN.py:86) */
    unsigned long long* count;   /* [1] transitions stored so far */
    int64_t capacity;
} rl_replay;
#define RL_MAX_CAPTURE_BRAINS 16

/* One brain of the brains list. */
typedef struct {
    int32_t kind;            /* RL_DQN .. RL_PERDQN */
    float epsilon;           /* exploration rate (0 = greedy, training=False); ignored for PPO (always samples) */
    const float* packed;     /* device: weights in the layout produced by rl_policy_pack_weights */
} rl_brain;

typedef struct rl_world rl_world;

const char* rl_last_error(void);
const char* rl_version(void);

int rl_create(const rl_config* cfg, rl_world** out);
void rl_destroy(rl_world* h);
int rl_bind_state(rl_world* h, const rl_state* device_ptrs);
/* optional device int32[4] that kernels set on inconsistencies: [0] code, [1] world, [2..3] detail.  The first error stays.  Codes:
 *   1  a taped _add_food draw (food_k) outside [0, #empty cells)             detail: try, value
 *   2  a taped birth placement (birth_k) outside [0, #empty cells)           detail: site, value
 *   3  a world's agent list outgrew slot_cap                                 detail: slots
 *   4  a taped produce_choice outside [0, RL_N_BEST)                         detail: value
 *   5  rl_render: a world id outside [0, n_worlds) ([1] = the id)            detail: frame index
 *   6  rl_learn / rl_learn_dueling / rl_learn_prioritized / rl_learn_ppo / rl_learn_td / rl_learn_td_wide: a minibatch slot outside [0, ring size) ([1] = brain index) detail: step, value
 *   7  rl_learn_prioritized_choice: the priorities give no distribution -- all zero, a NaN or a negative one: where np.random.choice
 *      raises ValueError ([1] = learner index)                               detail: rows of the memory, 0
 *   8  rl_learn_td_tree_sample: a draw ended on a leaf no row has reached, where Memory.sample draws again -- detail: the draw, the
 *      leaf's memory index; or the tree's total is not a positive finite number -- detail: -1, 0 ([1] = learner index)
 *   9  rl_learn_td_tree_update: a leaf index outside the tree's leaves or a slot outside the ring ([1] = learner index)
 *                                                                             detail: position in the batch, the leaf index */
int rl_bind_error_flag(rl_world* h, int32_t* device_flag);

/* tuning aid: device int64[32] receiving shader-clock stamps at the phase boundaries of world `world` (NULL = off) */
int rl_bind_phase_profile(rl_world* h, long long* device_stamps, int world);

int rl_reset_synthetic(rl_world* h, int n_agents, float* obs, void* stream);
/* Environment.reset() for every world (environment.py:133-158): one agent per brain -- gene = brain = its index, each at a
 * uniformly random cell (:147-149) -- and _init_food's Binomial food / poison counts + one super food (:741-761), from the
 * Philox streams (epoch as found in the state); obs as in rl_reset_synthetic */
int rl_reset_families(rl_world* h, float* obs, void* stream);
/* worlds with n_agents < threshold are re-generated (epoch+1); refill_count: optional device int32 accumulator */
int rl_refill(rl_world* h, int threshold, int n_agents, float* obs, int32_t* refill_count, void* stream);
int rl_observe(rl_world* h, float* obs, void* stream);
int rl_step(rl_world* h, const int8_t* actions, const rl_tape* tape, const rl_step_out* out, void* stream);
/* Environment.step() in two launches, for callers that draw _add_food's random numbers themselves from the reference's
 * own np.random stream (their count and arguments depend on the post-movement grid, environment.py:763-776):
 *   rl_step_split  everything up to and including _get_rewards; pre_counts [R][4] = food, poison, super food and empty
 *                  cells after movement; the outputs except `obs` are produced here
 *   rl_step_food   _add_food driven by tape->food_k / food_u, then the observation pass into `obs` (state_prime) */
int rl_step_split(rl_world* h, const int8_t* actions, const rl_step_out* out, int32_t* pre_counts, void* stream);
int rl_step_food(rl_world* h, const rl_tape* tape, float* obs, void* stream);
int rl_update(rl_world* h, const rl_tape* tape, const rl_update_out* out, void* stream);
int rl_tick(rl_world* h, const int8_t* actions, const rl_tape* tape, const rl_step_out* sout,
            const rl_update_out* uout, void* stream);
/* rl_tick (Philox draws) followed, in the same launch, by rl_refill(threshold, n_agents) of every world */
int rl_tick_refill(rl_world* h, const int8_t* actions, const rl_step_out* sout, const rl_update_out* uout,
                   int threshold, int n_agents, int32_t* refill_count, void* stream);

/* n_ticks iterations of the inference loop of Helpers/trainer.py:85-99 (minus learn) in ONE launch:
 *     for agent in env.agents: agent.get_action(n_epi)   (= rl_policy_act)      trainer.py:88-89
 *     env.step(); env.update_env(n_epi)                  (= rl_tick_refill)     trainer.py:92,99
 * Every world stays in its workgroup's LDS for the whole launch; the results are those of n_ticks calls of rl_policy_act +
 * rl_tick_refill (same Philox streams), and every per-tick output is written every tick, so after the call the buffers hold
 * the LAST tick's values:
 *   actions     [R][cap]      the actions chosen in the last tick (its pre-step list order)
 *   sout        reward / done / src / obs (state_prime) / n_acted / acted_total and the Tracker accumulators as in rl_tick (n_post / age /
 *               brain, the inputs of rl_capture_transitions, are not written here: rl_run_ex captures inside the launch instead)
 *   obs[2]      Agent.state ping-pong pair: tick i READS obs[(first_obs + i) & 1] (the policy's input; for i = 0 it must hold
 *               the current Agent.state rows) and WRITES the other one; after the call the current rows are in
 *               obs[(first_obs + n_ticks) & 1] and the rows the policy read for the last tick in the other buffer
 *   update_src  [R][cap] or NULL: rl_update_out.src of the last tick
 *   threshold   < 0: no re-generation; else worlds below `threshold` agents are re-generated with n_agents (rl_refill)
 * Supported (rl_run_supported() != 0) in THIS library (libreinlife_hip.so): n_brains <= 8, slot_cap <= 512 (the workgroup: 512 threads,
 * one world per workgroup), brains of any kinds, and n_worlds <= 768 -- or any n_worlds with the "run_always" option set (several
 * workgroups per CU then take turns; the two-launch loop is faster there, which is why it is not the default).
 * Not in this library: the 256- and 1024-thread instantiations ("world_block" = 256 / 1024, dueling kinds only) exist in the tuning
 * build alone (libreinlife_hip_tune.so, RL_TUNE=1 python reinlife_amd/build.py); here they answer 0 / RL_E_UNSUPPORTED.
 * A brains list that holds a PERDQN brain is not run here (k_run has no PERDQN tile): rl_run_supported() answers 0 and rl_run / rl_run_ex
 * return RL_E_UNSUPPORTED, both naming PERDQN and the two-launch loop.
 * Otherwise RL_E_UNSUPPORTED: loop over rl_policy_act + rl_tick_refill. */
/* rl_run_ex: rl_run with the options a TRAINING loop needs (Helpers/trainer.py:85-99 with training=True):
 *   eps_schedule  device [n_ticks][n_brains] or NULL: the brains' exploration rate in every tick of the launch -- the reference's brains
 *                 change epsilon from episode to episode (D3QN.py:84-89 / PERD3QN.py:82-86: x 0.99 per new n_epi; DQN.py:67-69);
 *                 NULL = brains[b].epsilon throughout
 *   sout->trk_*   the Tracker accumulators of rl_step_out are maintained every tick (environment.py:206-207 -> tracker.py:107-121):
 *                 trk_tick holds the last tick's values, trk_sum / trk_cnt / trk_pop[1..2] are read at the start of the launch and
 *                 written back at its end (running sums over as many launches as the caller likes; it zeroes them at interval ends) */
#define RL_EPS_INLINE_MAX 256
typedef struct {
    int32_t threshold, n_agents;     /* refill rule as in rl_run (threshold < 0: none) */
    int32_t* refill_count;
    const float* eps_schedule;
    int32_t trk_skip_ticks;          /* the first trk_skip_ticks ticks of the launch write trk_tick but stay out of the running sums:
                                      * episode 0 of a training run never reaches an aggregate (tracker.py:279-282 keeps the last
                                      * update_interval entries of update_interval + 1) */
    int32_t eps_schedule_on_host;    /* != 0: eps_schedule is a HOST pointer and n_ticks * n_brains <= RL_EPS_INLINE_MAX: the table travels
                                      * inside the kernel arguments (copied during the call) -- a short launch then waits for no upload */
    const rl_replay* replays;        /* host array [n_brains] or NULL: every tick's transitions are appended to the brains' replay rings
                                      * inside the launch -- what rl_capture_transitions does after a stand-alone tick (trainer.py:95-96,
                                      * entities.py:194-208); the rings' order is Agent.learn call order per world, worlds interleaved;
                                      * a ring below n_worlds * slot_cap rows is RL_E_INVALID (rl_replay: floor) */
    float* policy_out;               /* device [R][cap][8] or NULL: the policy's outputs (Q values / PPO probabilities) of the LAST tick,
                                      * indexed like `actions`; with `replays`, rl_replay.prob gets the taken action's entry every tick */
} rl_run_opts;
int rl_run_supported(const rl_world* h, const rl_brain* brains, int n_brains);
int rl_run(rl_world* h, const rl_brain* brains, int n_brains, int n_ticks, int8_t* actions, const rl_step_out* sout,
           float* const obs[2], int first_obs, int16_t* update_src, int threshold, int n_agents, int32_t* refill_count,
           void* stream);
int rl_run_ex(rl_world* h, const rl_brain* brains, int n_brains, int n_ticks, int8_t* actions, const rl_step_out* sout,
              float* const obs[2], int first_obs, int16_t* update_src, const rl_run_opts* opts, void* stream);

/* trainer.py:95-96 for every world: agents of the post-step list with age > 1 append (state, action, reward,
 * state_prime, done[, prob]) to the replay ring of their brain.
 *   state      [R][cap][153] the observation buffer the policy read for this tick (keep it: ping-pong rl_update_out.obs)
 *   actions    [R][cap]      this tick's actions (pre-step list order)
 *   policy_out [R][cap][8]   optional rl_policy_act outputs of this tick
 *   step       outputs of this tick's rl_step / rl_tick; needs reward, done, src, obs, n_post, age, brain
 *   replays    host array of n_brains rings (n_brains <= RL_MAX_CAPTURE_BRAINS), each of at least n_worlds * slot_cap rows (rl_replay:
 *              floor; a smaller one is RL_E_INVALID naming it) */
int rl_capture_transitions(rl_world* h, const float* state, const int8_t* actions, const float* policy_out,
                           const rl_step_out* step, const rl_replay* replays, int n_brains, void* stream);

/* ---- policy ------------------------------------------------------------------------------------------------- */
/* number of floats in a brain's state dict (flat, registration order) / in its packed MFMA layout */
int64_t rl_policy_n_params(int kind);
int64_t rl_policy_packed_floats(int kind);
/* host -> host: state-dict order  (DQN: fc1.w fc1.b fc2.w fc2.b fc3.w fc3.b;  D3QN/PERD3QN: fc.w fc.b adv_fc1.w
 * adv_fc1.b adv_fc2.w adv_fc2.b value_fc1.w value_fc1.b value_fc2.w value_fc2.b;  PPO: fc1.w fc1.b fc2.w fc2.b
 * fc_pi.w fc_pi.b fc_v.w fc_v.b;  PERDQN: fc.0.w fc.0.b fc.2.w fc.2.b fc.4.w fc.4.b)  ->  MFMA-fragment-major layout read by the kernels */
int rl_policy_pack_weights(int kind, const float* state_dict_flat, float* packed);
/* dense batch: obs [n_rows][153] (device) -> out [n_rows][8]: Q values (per-row dueling mean) or PPO probabilities.
 * Every row is computed from that row alone (its own power-of-two scale): its outputs do not depend on the other rows of the
 * batch, on its position in it, or on the policy_variant.
 * Supported magnitudes: a row (and every hidden activation row it produces) whose largest |element| is 0 or lies in
 * [2^-95, 2^103] gets f32-grade results (|error| <= 1e-5 of the row's largest |output|; scaling a row by 2^k scales the outputs
 * of a bias-free Q network by exactly 2^k).  Outside that range the row scale is clamped: smaller rows lose precision down to
 * all-zero inputs, larger ones overflow the f16 operands; such a row still yields an action in 0..7, sets no error flag and
 * does not disturb the other rows.
 * Non-finite inputs: the reference propagates NaN; these kernels do not.  Row maximum and ReLU are fmaxf, which returns the
 * operand that is a number, so a row holding a NaN or +-Inf element leaves the first layer as an all-zero hidden row: its
 * outputs are FINITE (the later layers' biases alone) and its action is chosen from them.  Other rows are unaffected.
 * The same holds for rl_policy_act and the policy half of rl_run. */
int rl_policy_forward(int kind, const float* packed, const float* obs, int64_t n_rows, float* out, void* stream);
/* all agents of all worlds: row (w,k) uses brains[a_brain[w][k]].
 *   obs     [R][cap][153]   actions [R][cap] (written for k < n_agents[w])   out_q [R][cap][8] or NULL
 *   work    device scratch of rl_policy_work_bytes(h) bytes, zero-initialised ONCE by the caller before the first
 *           call and owned by this handle afterwards (it carries double-buffered counters between calls)
 *   tape_actions: optional [R][cap] recorded actions (parity mode) that override the selected ones */
size_t rl_policy_work_bytes(const rl_world* h);
/* optional: hand the work buffer to the handle so that rl_tick / rl_update / rl_reset_synthetic / rl_refill also emit
 * the per-brain row lists rl_policy_act needs (saves its bucket launch).  All launches of a handle must be issued in
 * stream order.  rl_bind_state (call it again after rewriting state buffers yourself) invalidates the lists. */
int rl_bind_policy_work(rl_world* h, void* work);
int rl_policy_act(rl_world* h, const rl_brain* brains, int n_brains, const float* obs, int8_t* actions, float* out_q,
                  void* work, void* stream);

/* ---- learning -------------------------------------------------------------------------------------------------- */
/* One learning brain of an rl_learn call: what DQNAgent owns besides its replay memory (Models/DQN.py:48-55 -- agent, target, optimizer)
 * as caller-owned device buffers, all in state-dict-flat order (rl_policy_pack_weights), plus the hyperparameters of DQN.py:14-16, 52. */
typedef struct {
    int32_t kind;                 /* RL_DQN; anything else: RL_E_UNSUPPORTED naming the kind */
    float *params, *target;       /* device [rl_policy_n_params(kind)], state-dict order */
    float *adam_m, *adam_v;       /* device, same size, zeroed once by the caller */
    int64_t* state;               /* device [2]: Adam steps taken, rl_learn calls made */
    float* packed;                /* device [rl_policy_packed_floats(kind)]: rewritten at the end of every call */
    float lr, gamma, beta1, beta2, eps;
    int32_t batch, min_size, sync_target;
    float* loss;                  /* device [n_steps] or NULL */
    float* grad;                  /* device [n_steps][n_params] or NULL (tests, diagnostics) */
} rl_learner;
/* 1 for the brain kinds rl_learn trains (RL_DQN), 0 for the others */
int rl_learn_supported(int kind);
/* DQNAgent.train() (DQN.py:80-83 -> train(), :142-153) for n_learners brains in ONE stream-ordered launch, one workgroup per brain:
 * learner i trains on rings[i] (n_learners <= RL_MAX_CAPTURE_BRAINS; both are host arrays, copied during the call).
 *   size gate   size = min(*ring.count, ring.capacity), read on the device; size <= min_size: no update (DQN.py:81)
 *   n_steps     sequential minibatch updates (the reference: 5), each: batch rows (1..32) of the ring -> q = Q_eval(state),
 *               target = reward + gamma * max_a Q_target(state_prime) * (1 - done), loss = mean smooth_l1(q[action] - target) (beta 1),
 *               its gradient through the network, and torch.optim.Adam's update (no weight decay, no amsgrad; bias corrections in
 *               double from the step count state[0]; lr, beta1, beta2 are re-read as the decimal that "%.7g" prints for them --
 *               0.999f means 0.999, as torch's Python floats do; a float that is NOT a decimal of at most 7 digits is rounded to one)
 *               of params / adam_m / adam_v.  loss[s] and grad[s][n_params] are written when given.
 *   rows        slots != NULL: device int32 [n_learners][n_steps][batch] ring slots, duplicates allowed (they count twice).  A slot
 *               outside [0, size) of a ring above the size gate sets error-flag code 6 and that brain leaves the call with NONE of its buffers touched (the others
 *               train).  slots == NULL: slot = ((uint64)x * size) >> 32, x = word 0 of rl_philox(seed, 0, i, (uint32)state[1],
 *               RL_SITE_LEARN, s * batch + j): uniform WITH replacement -- the reference's random.sample (DQN.py:100) draws without.
 *   afterwards  sync_target != 0: target <- params (DQN.py:83, also below the size gate); state[0] += updates made; state[1] += 1;
 *               `packed` is rewritten from the final params, bit for bit what rl_policy_pack_weights makes of them -- the acting
 *               kernels that hold this pointer (rl_brain.packed) act on the new weights from the next launch of the stream on.
 * Deterministic: the same buffers give the same bits in every run and whatever else is in the launch.  The handle supplies the Philox
 * seed and the error flag; it need not be bound. */
int rl_learn(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
             void* stream);

/* 1 for the brain kinds rl_learn_dueling trains (RL_D3QN), 0 for the others.  RL_PERD3QN has the same network and the same plain MSE
 * loss but learns from a prioritised memory (PERD3QN.py:110-111, 133-182), which this entry point does not keep: 0
 * (rl_learn_prioritized trains it). */
int rl_learn_dueling_supported(int kind);
/* D3QNAgent.train() (Models/D3QN.py:97-116) for n_learners brains in ONE stream-ordered launch, one workgroup per brain, on the same
 * rl_learner / rl_replay structures as rl_learn (kind must be RL_D3QN: anything else is RL_E_UNSUPPORTED naming the kind; batch in
 * [1,64]; every other validation is rl_learn's).  rl_learn, rl_learn_supported and rl_learn_draw are unchanged by it.
 *   network     dueling_ddqn (D3QN.py:148-165), state-dict order fc 153->128, adv_fc1 128->128, adv_fc2 128->8, value_fc1 128->128,
 *               value_fc2 128->1: 53,897 parameters.  q[i][a] = adv[i][a] + val[i] - M with M the mean of adv over ALL rows and actions
 *               of the minibatch (D3QN.py:165 writes advantage.mean(), not a per-row mean; the acting kernels' per-row mean is the same
 *               expression at batch 1).  The target network's q' takes its own M' over the batch's state_prime rows.
 *   size gate   size = min(*ring.count, ring.capacity), read on the device; size <= min_size: no update.  The reference has no gate but
 *               random.sample's need of batch rows (D3QN.py:98, 140): min_size = batch - 1.
 *   n_steps     sequential minibatch updates (the reference: 1 per train()), each: y_i = reward_i + gamma (1 - done_i) max_a q'_target
 *               (D3QN.py:107-110), loss = mean_i (q[i][a_i] - y_i)^2 (nn.MSELoss, D3QN.py:63, 112), its gradient through both branches
 *               and the shared fc, and torch.optim.Adam's update exactly as rl_learn makes it (bias corrections in double from
 *               state[0]; lr, beta1, beta2 re-read as decimals).  loss[s] and grad[s][n_params] are written when given.
 *   rows        as rl_learn: slots != NULL is device int32 [n_learners][n_steps][batch], all range-checked before the first row is
 *               fetched (a bad one: error-flag code 6, that brain leaves with NONE of its buffers written, the others train);
 *               slots == NULL draws with the same Philox mapping and RL_SITE_LEARN.
 *   afterwards  sync_target != 0: target <- params (the caller's schedule: D3QN.py:125-126 copies every soft_update_freq episodes, and
 *               D3QN.py:121 trains only once n_epi > exploration); state[0] += updates made; state[1] += 1; `packed` is rewritten from the
 *               final params, bit for bit what rl_policy_pack_weights(RL_D3QN, ...) makes of them.
 * Deterministic like rl_learn: plain f32 FMA, every sum by one thread in a fixed order, no float atomics. */
int rl_learn_dueling(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                     void* stream);

/* The `slots` of an rl_learn call drawn so that they do not depend on the ORDER of a ring's rows: rl_run_ex / rl_capture_transitions
 * append every world's transitions with an atomic add on the ring's counter, so two identical runs hold the same transitions in other
 * slots, and rl_learn's own draw (slots == NULL), which names slots, would train them differently.  Here every row gets a 64-bit key of
 * its content (state, state_prime, action, reward, done, age) and draw d = s * batch + j takes the row whose key, mixed with words 0-1 of
 * rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN, d), is smallest: empirically uniform over the rows (as good as the mixing function), WITH replacement, the same rows
 * whatever slots they sit in (equal rows are interchangeable; distinct rows with equal keys: 2^-64).
 *   keys    host array [n_learners] of device uint64 [ring capacity] scratch, rewritten by every call
 *   slots   device int32, the learners' [n_steps][batch] tables laid end to end (what rl_learn takes when all batches are equal)
 *           The table is FLAT (draw d = s * batch + j), and batch is at most 32 here: a batch-64 table for rl_learn_dueling,
 *           [n_steps][64], is the same table as [2 n_steps][32] -- ask with batch = the largest divisor of the real batch that is
 *           <= 32 and n_steps scaled to match (DeviceWorlds.draw_slots does).
 * Two launches (keys of the rows a ring holds, then one workgroup per draw); call it in front of rl_learn on the same stream.  What it
 * cannot mend: a launch that appends MORE than a ring's capacity overwrites its own rows in append order -- which rows survive then
 * differs from run to run. */
int rl_learn_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                  unsigned long long* const* keys, int32_t* slots, void* stream);

/* THIS BUILD'S OWN -- rl_learn_draw's table by another sampler: uniform draws by content-key RANK.  rl_learn_draw visits every key of a
 * ring once per draw, so its cost grows with n_steps x batch x size; here the rows a ring holds are sorted by content key once per
 * call and every draw is an index into that order, so the cost of a call does not depend on n_steps or the batches.  For learner i:
 *   size     min(*ring.count, ring.capacity), read on the device
 *   keys     host array [n_learners] of device uint64 [capacity]: keys[i][r], r < size, are the content keys exactly as rl_learn_draw
 *            makes them, rewritten by every call
 *   order    host array [n_learners] of device int32 [capacity]: after the call order[i][0 .. size) holds the slots 0 .. size - 1
 *            ascending by (keys[slot], slot) -- numpy's lexsort((arange(size), keys[:size])).  Equal keys are equal rows up to a 2^-64
 *            collision; the lower slot first makes the table a function of the ring's contents and layout, and the rows a draw names a
 *            function of the contents alone.  Entries from `size` on are left as they were.
 *   work     host array [n_learners] of device scratch of at least rl_learn_draw_rank_work_bytes(capacity) bytes each, 16-byte
 *            aligned: two tables of 65,536 counters (the keys' top 16 bits name a bucket) and one int32 per ring row.  It needs no
 *            initialisation and holds nothing between calls.
 *   slots    device int32, the learners' flat [n_steps][batch] tables laid end to end, as for rl_learn_draw: draw d = s * batch + j,
 *            d < n_steps * batch, takes x = word 0 of rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN, d), t = ((uint64)x * size)
 *            >> 32 and slots[d] = order[t] -- rl_learn's own slots == NULL mapping, applied to the rank instead of the slot: uniform up
 *            to the multiply-shift's size / 2^32, WITH replacement.  size == 0 writes slot 0 for every draw.  batch is in
 *            [1, RL_LEARN_WIDE_MAX] (the table is flat: no limit of 32 and no divisor trick), and the learners of a call may have
 *            different batches.
 * It is a DIFFERENT sampler from rl_learn_draw: the same distribution, other rows.  rl_learn_draw, rl_learn, rl_learn_wide and every
 * *_supported answer are unchanged by it.
 * RL_LEARN_DRAW_RANK_LAUNCHES (6) launches whatever n_steps, the batches and the rings hold, all queued on `stream`: clear the
 * counters, keys and histogram (one wave per row), the prefix sum (one workgroup per learner), the scatter into buckets, the placement
 * inside every bucket (a member's place is the number of members with a smaller (key, slot): the sum of the squared bucket sizes in all,
 * about two visits per row on mixed keys, size^2 -- bounded, still exact -- where every row of a ring is the same), and one thread per
 * draw.  No host read-back, no allocation.  The only atomics are integer adds and nothing the caller sees depends on the order they
 * arrive in: keys, order and slots have the same bits in every run.
 * Validated on the host before anything is launched, RL_E_INVALID naming the argument: a null handle, learners, rings, keys, order,
 * work or slots; a null learner state, keys[i], order[i] or work[i]; n_learners in [1, RL_MAX_CAPTURE_BRAINS]; n_steps >= 1 (and
 * n_steps times the batches below 2^31 draws); the batch range; rl_learn_draw's ring checks (the age column included). */
#define RL_LEARN_DRAW_RANK_LAUNCHES 6
/* The bytes of one learner's work buffer for a ring of `capacity` rows (a multiple of 16); 0, with rl_last_error set, for a capacity
 * outside [1, 2^31). */
size_t rl_learn_draw_rank_work_bytes(long long capacity);
int rl_learn_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                       unsigned long long* const* keys, int32_t* const* order, void* const* work, int32_t* slots, void* stream);

/* ---- wide minibatches (DQN)-------------------------------------------------------------------------------------- */
/* THIS BUILD'S OWN -- the reference trains one world on minibatches of 32 (DQN.py:80-83, 142-153).  rl_learn_wide is that update on a
 * minibatch of 1 .. RL_LEARN_WIDE_MAX rows, split into 32-row tiles that run side by side, one workgroup per (learner, tile): a run of
 * many worlds appends far more rows per learning episode than 5 x 32, and rl_learn keeps one CU busy.  A call whose batch is at most 32
 * (one tile) leaves every buffer bit for bit as rl_learn leaves it.  rl_learn, rl_learn_draw and rl_learn_supported are unchanged by it. */
#define RL_LEARN_WIDE_MAX 2048
/* 1 for the brain kinds rl_learn_wide trains (RL_DQN), 0 for the others */
int rl_learn_wide_supported(int kind);
/* The bytes of one learner's work buffer for a minibatch of `batch` rows: a 64-byte header, ceil(batch / 32) rows of
 * rl_policy_n_params(kind) floats (the tiles' partial gradients), and the tiles' loss sums, rounded up to 16 bytes.  0, with
 * rl_last_error set, for a kind rl_learn_wide does not train or a batch outside [1, RL_LEARN_WIDE_MAX]. */
size_t rl_learn_wide_work_bytes(int kind, int batch);
/* DQNAgent.train() (DQN.py:80-83 -> train(), :142-153) on wide minibatches for n_learners brains, on the rl_learner / rl_replay
 * structures of rl_learn (kind must be RL_DQN; batch in [1, RL_LEARN_WIDE_MAX], ONE batch for all learners of a call).
 *   work        host array [n_learners] of device buffers of at least rl_learn_wide_work_bytes(kind, batch) bytes each, 16-byte aligned;
 *               they need no initialisation and hold nothing between calls
 *   size gate   as rl_learn: size = min(*ring.count, ring.capacity), read on the device; size <= min_size: no update
 *   rows        slots != NULL: device int32 [n_learners][n_steps][batch]; every entry of a learner that trains is range-checked
 *               before a row is fetched -- a bad one sets error-flag code 6 ([1] = learner, [2] = step, [3] = the value; the first in
 *               table order) and that learner leaves the call with NONE of its buffers touched (the others train).  slots == NULL:
 *               rl_learn's draw with the wider batch: slot = ((uint64)x * size) >> 32, x = word 0 of rl_philox(seed, 0, i,
 *               (uint32)state[1], RL_SITE_LEARN, s * batch + j).  Tile t of a step holds batch rows 32 t .. min(32 t + 31, batch - 1).
 *   a step      every tile runs rl_learn's forward, smooth-L1 and backward arithmetic on its rows, with the loss gradient scaled by
 *               1.0f / batch of the WHOLE batch, and writes its partial gradient (per parameter the f32 sum over the tile's rows,
 *               ascending: what rl_learn hands to Adam) and its loss sum to `work`.  Then one thread per parameter adds the tiles'
 *               partials in tile order in double, rounds to float once -- with one tile: the partial itself -- and makes rl_learn's Adam
 *               update with it.  loss[s] = (float)(sum of the tiles' loss sums in double) * (1.0f / batch); grad[s] = the summed gradient.
 *   afterwards  as rl_learn: sync_target != 0: target <- params (also below the size gate); state[0] += updates made; state[1] += 1;
 *               `packed` rewritten from the final params, bit for bit what rl_policy_pack_weights(RL_DQN, ...) makes of them.
 * 2 n_steps + 3 launches, all queued on `stream`: one check pass (gate, slots, header), per step the tiles and the update, one pass for
 * target and counters, one for `packed`.  No host read-back, no cooperative launch, no allocation.  Deterministic: every sum has a fixed
 * order and no float atomics exist, so the same buffers give the same bits in every run and whatever else is in the launch.
 * Validated on the host before anything is launched, RL_E_INVALID naming the argument (here also for a kind that is not RL_DQN):
 * null handle / learners / rings / work, n_learners in [1, RL_MAX_CAPTURE_BRAINS], n_steps >= 1, batch in [1, RL_LEARN_WIDE_MAX] and
 * equal for all learners, rl_learn's null-pointer and capacity checks, a null work[i]. */
int rl_learn_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps, const int32_t* slots,
                  void* const* work, void* stream);

/* ---- wide minibatches (D3QN) ------------------------------------------------------------------------------------- */
/* THIS BUILD'S OWN -- the reference trains one world on ONE minibatch of 64 per train() (D3QN.py:97-116).  rl_learn_dueling_wide is that
 * update on a minibatch of 1 .. RL_LEARN_DUELING_WIDE_MAX rows, split into 64-row tiles that run side by side, one workgroup per (learner,
 * tile), with dueling_ddqn.forward's advantage mean (D3QN.py:165) taken over the WHOLE minibatch as the reference takes it: the tiles
 * meet in three scalars per step (the two means and the sum of the rows' loss gradients), each a sum of per-tile sums in tile order.  A
 * call whose batch is at most 64 (one tile) leaves every buffer bit for bit as rl_learn_dueling leaves it.  rl_learn_dueling and every
 * other entry point are unchanged by it. */
#define RL_LEARN_DUELING_WIDE_MAX 2048
/* 1 for the brain kinds rl_learn_dueling_wide trains (RL_D3QN), 0 for the others (RL_PERD3QN: its prioritised memory is not kept here) */
int rl_learn_dueling_wide_supported(int kind);
/* The bytes of one learner's work buffer for a minibatch of `batch` rows, T = ceil(batch / 64): a 64-byte header, T rows of
 * rl_policy_n_params(kind) floats (the tiles' partial gradients), 2 T floats rounded up to 16 bytes (the tiles' advantage sums) and
 * T x 64 rows of 14 floats (per row adv'[8], val', adv[a], val, reward, mask, action).  0, with rl_last_error set, for a kind
 * rl_learn_dueling_wide does not train or a batch outside [1, RL_LEARN_DUELING_WIDE_MAX]. */
size_t rl_learn_dueling_wide_work_bytes(int kind, int batch);
/* D3QNAgent.train() (D3QN.py:97-116) on wide minibatches for n_learners brains, on the rl_learner / rl_replay structures of
 * rl_learn_dueling (kind must be RL_D3QN: anything else is RL_E_UNSUPPORTED naming the kind; batch in [1, RL_LEARN_DUELING_WIDE_MAX],
 * ONE batch for all learners of a call).
 *   work        host array [n_learners] of device buffers of at least rl_learn_dueling_wide_work_bytes(kind, batch) bytes each, 16-byte
 *               aligned; they need no initialisation and hold nothing between calls
 *   size gate   as rl_learn_dueling: size = min(*ring.count, ring.capacity), read on the device; size <= min_size: no update
 *   rows        slots != NULL: device int32 [n_learners][n_steps][batch]; every entry of a learner that trains is range-checked
 *               before a row is fetched -- a bad one sets error-flag code 6 ([1] = learner, [2] = step, [3] = the value; the first in
 *               table order) and that learner leaves the call with NONE of its buffers touched (the others train).  slots == NULL:
 *               rl_learn_dueling's draw with the wider batch: slot = ((uint64)x * size) >> 32, x = word 0 of rl_philox(seed, 0, i,
 *               (uint32)state[1], RL_SITE_LEARN, s * batch + j).  Tile t of a step holds batch rows 64 t .. min(64 t + 63, batch - 1).
 *   a step      first pass, every tile: rl_learn_dueling's target forward on s' and eval forward on s; per tile the f32 sums of its live
 *               rows' advantage sums (row ascending), per row a few numbers, to `work`.  Second pass, every tile, identically: M' and M =
 *               (float)(the tiles' sums added in double, tile ascending) / (float)(8 batch); rl_learn_dueling's td and g_i = (2 td) *
 *               (1.0f / batch) for every row of the batch; G and the loss from per-tile f32 sums (row ascending) added in double in tile
 *               order and rounded once; then the tile's eval forward again and rl_learn_dueling's backward pass with G / (float)(8 batch),
 *               its partial gradient (per parameter the f32 sum over the tile's rows, ascending) to `work`.  Then one thread per
 *               parameter adds the tiles' partials in tile order in double, rounds to float once -- with one tile: the partial itself --
 *               and makes rl_learn_dueling's Adam update.  loss[s] = (float)(that double sum of td^2) * (1.0f / batch); grad[s] = the
 *               summed gradient.
 *   afterwards  as rl_learn_dueling: sync_target != 0: target <- params (also below the size gate); state[0] += updates made;
 *               state[1] += 1; `packed` rewritten from the final params, bit for bit what rl_policy_pack_weights(RL_D3QN, ...) makes.
 * 3 n_steps + 3 launches, all queued on `stream`: one check pass (gate, slots, header), per step the two tile passes and the update, one
 * pass for target and counters, one for `packed`.  No host read-back, no cooperative launch, no workgroup waits for another, no
 * allocation.  Deterministic: every sum has a fixed order and no float atomics exist, so the same buffers give the same bits in every
 * run and whatever else is in the launch.
 * Validated on the host before anything is launched, RL_E_INVALID naming the argument: null handle / learners / rings / work,
 * n_learners in [1, RL_MAX_CAPTURE_BRAINS], n_steps >= 1, batch in [1, RL_LEARN_DUELING_WIDE_MAX] and equal for all learners,
 * rl_learn's null-pointer and capacity checks, a null work[i]. */
int rl_learn_dueling_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, int n_learners, int n_steps,
                          const int32_t* slots, void* const* work, void* stream);

/* ---- prioritised replay (PERD3QN) ------------------------------------------------------------------------------- */
/* The prioritised memory of one learning PERD3QN brain (PrioritizedReplayBuffer, Models/PERD3QN.py:133-182) beside its rl_replay ring:
 * caller-owned device buffers.  The ring itself, rl_run_ex and rl_capture_transitions know nothing of priorities: store() gives a new
 * row max(priorities) (PERD3QN.py:147, 153) and never lowers that maximum (a row overwritten with the maximum keeps it), so between two
 * learning calls the maximum is a constant and "every row appended since the last draw gets the current maximum" is done after the
 * fact, from `seen` and the ring's counter (slot = count mod capacity). */
typedef struct {
    float* priority;            /* [capacity] */
    float* weight;              /* [capacity] scratch: priority^alpha, rewritten by every draw */
    unsigned long long* keys;   /* [capacity] scratch: content keys as rl_learn_draw makes them */
    float* prio_max;            /* [1] initialise to 1.0 (PERD3QN.py:147: the priority of the first row of an empty memory) */
    unsigned long long* seen;   /* [1] initialise to 0: ring.count as of the last draw */
    float alpha;                /* 0.6 (PERD3QN.py:134); must be > 0 */
} rl_prio;
/* PrioritizedReplayBuffer.sample's draw (PERD3QN.py:157-165: np.random.choice(len, batch, p = priorities^alpha / sum), WITH replacement)
 * for n_learners PERD3QN brains, stream-ordered, no host round trip, no allocation; like rl_learn_draw it does not depend on the slots
 * the rings' rows sit in.  Two launches:
 *   prepare   per row of [0, size): the slots in [*seen, *ring.count) mod capacity (all of them when count - seen >= capacity) get
 *             priority = *prio_max; weight = powf(priority, alpha) (alpha == 1: the priority itself, bit for bit); keys[row] = the
 *             row's content key exactly as rl_learn_draw makes it
 *   pick      one workgroup per draw d = s * batch + j (batch in [1,64] directly): v = mix64(key ^ salt_d), salt_d = words 0-1 of
 *             rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN_PRIO, d); U = ((v >> 41) + 0.5) / 2^23, a uniform in (0,1);
 *             t = -logf(U) / weight; the draw takes the row with the smallest (t, v, slot), compared lexicographically.  An exponential
 *             race: row i wins with probability w_i / sum w, the same rows whatever slots they sit in (U has 23 bits: rows whose t tie
 *             are told apart by v, and on a ring of N rows the probabilities are those of the exact race up to about N / 2^23 of
 *             themselves).  A row of weight 0 (or NaN) has t = +inf and loses to every finite t; so does a row whose positive weight is so
 *             small that -logf(U) / weight overflows (weight below about 4.9e-38: it ranks with the zero-weight rows; with alpha =
 *             0.6 no float priority is that small, an alpha above about 0.84 reaches it with denormal priorities).  If EVERY weight is zero the tie-break on
 *             v makes the draw rl_learn_draw's uniform content-key draw -- the reference would raise there (np.random.choice refuses a p
 *             of NaNs).  An empty ring draws slot 0.  This launch also advances *seen to *ring.count (the prepare launch is its only reader).
 *   slots     device int32, the learners' [n_steps][batch] tables laid end to end ([n_learners][n_steps][batch] when all batches are equal)
 * All n_steps of a call are drawn from the priorities as they stand at the draw: with n_steps = 1 -- the reference's train(), and what
 * Environment uses -- this is the reference's order exactly; with more, steps 2.. do not see the priorities step 1 will write.
 * Every learner's kind must be RL_PERD3QN (anything else: RL_E_UNSUPPORTED naming the kind); rings need state / state_prime / action /
 * reward / done / age / count; every pointer of rl_prio must be set and alpha > 0.
 * Two deviations from the reference, as for rl_learn_draw: rows appended between two draws all get the maximum as of the earlier
 * learning call (the reference recomputes it at every store(), but nothing changes it in between), and a launch that appends MORE than a
 * ring's capacity overwrites its own rows in append order -- which rows survive then differs from run to run. */
int rl_learn_prioritized_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                              int n_steps, int32_t* slots, void* stream);
/* 1 for the brain kinds rl_learn_prioritized trains (RL_PERD3QN), 0 for the others */
int rl_learn_prioritized_supported(int kind);
/* PERD3QNAgent.train() (Models/PERD3QN.py:94-115) for n_learners brains in ONE stream-ordered launch: rl_learn_dueling's update, the
 * same arithmetic in the same order (DuelingDDQN, PERD3QN.py:185-202, is the D3QN network; the advantage mean is the minibatch's), plus
 * the prioritised memory's upkeep.  What the reference does, stated exactly:
 *   loss        plain nn.MSELoss (PERD3QN.py:56, 109).  sample() computes importance weights (PERD3QN.py:168-172) but train() never uses
 *               them, so they -- and beta / beta_increment -- have no effect, there or here.  There is NO importance-weighted loss.
 *   priorities  after the forward passes, update_priorities(indices, |next_q_value - q_value|) (PERD3QN.py:110-111) with next_q_value =
 *               max_a q'_target(s') and q_value = q_eval(s)[a], each with its batch-wide mean: the reference's expression, not the TD
 *               error (no reward, no gamma, no done mask).  Here: right where a step forms td, every batch row writes priority[slot]
 *               from that step's pre-update parameters; duplicated slots write equal bits; later steps overwrite earlier ones.
 *   afterwards  as rl_learn_dueling, and, in a call that trained (size > min_size), *prio_max = max(priority[0 .. size)) (what store()
 *               hands the next new rows, PERD3QN.py:147); a call below the size gate leaves priorities and prio_max alone.
 *   order       PRECONDITION: rl_learn_prioritized_draw has run on these rings since the last row was appended (the `slots` of this
 *               call are its output).  The maximum is taken over the rows as they stand: rows the draw has not stamped yet still hold
 *               stale priorities (zero in a fresh buffer) and would lower it.
 * Validation is rl_learn_dueling's with these differences: kind must be RL_PERD3QN (anything else: RL_E_UNSUPPORTED naming the kind);
 * slots == NULL is refused with RL_E_INVALID -- the draw is rl_learn_prioritized_draw's job; prios[i].priority / prio_max / seen must
 * not be null and alpha > 0.  batch in [1,64].  min_size as before: the reference needs one row only (np.random.choice), min_size = 0.
 * A slot outside [0, size): error-flag code 6, and NONE of that brain's buffers -- priorities and prio_max included -- is written.
 * rl_learn, rl_learn_draw, rl_learn_dueling and the two older *_supported answers are unchanged by it. */
int rl_learn_prioritized(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners, int n_steps,
                         const int32_t* slots, void* stream);

/* ---- the prioritised memory as the reference keeps it: store() and np.random.choice (PERD3QN, learn="reference") ------------------- */
/* Two stream-ordered entry points, one launch of one workgroup per learner each, no allocation, no host round trip, at most
 * RL_MAX_CAPTURE_BRAINS learners per call, kind RL_PERD3QN only (anything else: RL_E_UNSUPPORTED naming the kind).  They are draws, not
 * learners: the update is rl_learn_prioritized, unchanged, on the slots rl_learn_prioritized_choice names.  In this use *prio_max and
 * *seen of rl_prio are written by rl_learn_prioritized and read by nobody: the store takes its own maximum, over the live window.
 *
 * Notation.  C = the memory's capacity (PERD3QN.py:135); R >= C = the rows the ring holds (a caller that captures a whole tick's rows in
 * front of the tick's train() calls needs R = C + slack, slack >= the rows of one tick).  Rows are numbered from 0 in storage order; row a
 * sits in ring slot a % R and at the reference's memory index a % C.  rl_prio.priority is indexed by RING SLOT and holds R floats,
 * zero-initialised.  Of rl_prio only `priority` (and, for the choice, `alpha`) is read. */
typedef struct {
    long long capacity;         /* C, in [1, 2^31) */
    long long ring_rows;        /* R, in [C, 2^31) */
    long long first_row;        /* a >= 0: the first row of the group */
    long long n_rows;           /* m in [1, R - C]; anything else is RL_E_INVALID */
} rl_prio_store;
/* PrioritizedReplayBuffer.store (PERD3QN.py:143-155) for rows [a, a + m) of each learner:
 *   M = 1.0f                                            when a == 0 (the first row of an empty memory)
 *   M = max over rows r in [max(0, a - C), a) of priority[r % R]   otherwise, and, when a < C, of 0 (the memory indices no row has reached
 *       yet count as np.max counts the array's unused zeros); a NaN in the window propagates, as np.max propagates it
 *   priority[(a + j) % R] = M  for j < m
 * A group gets ONE M.  That is the reference's result exactly when no train() lies inside the group: storing M never lowers the maximum
 * (a row overwritten with the maximum keeps it), and only update_priorities changes it.  The caller cuts its groups at every train(). */
int rl_learn_prioritized_store_ref(rl_world* h, const rl_learner* learners, const rl_prio* prios, const rl_prio_store* groups, int n_learners,
                                   void* stream);
#define RL_LEARN_CHOICE_MAX 64  /* the draws of one rl_learn_prioritized_choice call per learner at most */
typedef struct {
    long long capacity;         /* C, in [1, 2^31): slots and indices are int32 (a larger one is RL_E_INVALID naming this limit) */
    long long ring_rows;        /* R, in [C, 2^31) */
    long long stored;           /* rows stored so far, >= 1 (np.random.choice needs one row) */
    int32_t batch;              /* in [1, RL_LEARN_CHOICE_MAX] */
    const double* u;            /* device [batch]: the host's np.random.random_sample(batch), in [0,1) */
    int32_t* indices;           /* device [batch]: the reference's memory indices */
    int32_t* slots;             /* device [batch]: their ring slots, what rl_learn_prioritized takes */
    double* bracket;            /* device [batch][2] or NULL: each draw's cdf[idx - 1] (0 for idx = 0) and cdf[idx] (tests, diagnostics) */
    void* work;                 /* device, rl_learn_prioritized_choice_work_bytes(C) bytes of scratch: the cdf and the weights */
} rl_prio_choice;
/* the bytes of rl_prio_choice.work for a memory of `capacity` rows (0 for a capacity outside [1, 2^31)) */
size_t rl_learn_prioritized_choice_work_bytes(long long capacity);
/* PrioritizedReplayBuffer.sample's draw (PERD3QN.py:157-165) from host-drawn uniforms: np.random.choice(len, batch, p=probs) consumes
 * exactly `batch` doubles of random_sample() and answers cdf.searchsorted(u, side="right"), cdf = probs.cumsum() in float64 divided by its
 * last element.  Per learner, with T = 1024 and all sums taken left to right:
 *   n       = min(stored, C)
 *   a_i     = i + C * ((stored - 1 - i) / C)            (integer division) the row memory index i < n holds
 *   p_i     = priority[a_i % R]
 *   w_i     = (float)pow((double)p_i, (double)alpha)    alpha = 0.6f: probs ** self.alpha on a float32 array stays float32 under numpy 2
 *   L       = ceil(n / T); chunk t = the indices [t L, min(n, (t + 1) L))
 *   S       = (float)(sum over t = 0 .. T-1 of (sum over i in chunk t of (double)w_i))        both sums in double, rounded to float once
 *   q_i     = w_i / S                                   in float
 *   c_i     = sum over k in i's chunk, k <= i, of (double)q_k;    o_t = sum over t' < t of c_(last index of chunk t')
 *   cdf_i   = (o_t + c_i) / (o_t + c_i at i = n - 1)    nondecreasing, cdf_(n-1) = 1.0
 *   idx_j   = #{i : cdf_i <= u_j}                       side="right": a u on a boundary goes to the next row; a row of weight zero is never drawn
 *   indices[j] = idx_j;  slots[j] = a_(idx_j) % R;  bracket[j] = {idx_j > 0 ? cdf_(idx_j - 1) : 0, cdf_(idx_j)}
 * numpy's float32 power is within 1 ulp of w_i, not always equal to it, and its cumsum is sequential: the probabilities agree to a few
 * float32 ulps and the cdf to about 2^-21, so a u that close to a boundary may name the neighbouring row.  The bits of indices, slots and
 * bracket are the same in every run (no atomics, fixed association order).
 * Refused on the device: where np.random.choice raises ValueError -- the weights sum to zero, or a priority is NaN or negative (or the sum
 * overflows) -- the bound error flag gets code 7 and EVERY draw of that learner gets index 0 and slot a_0 % R; bracket is not written.
 * Refused on the host (RL_E_INVALID naming the argument): stored < 1, batch outside [1, RL_LEARN_CHOICE_MAX], a null u / indices / slots /
 * work, alpha <= 0, C or R outside their ranges. */
int rl_learn_prioritized_choice(rl_world* h, const rl_learner* learners, const rl_prio* prios, const rl_prio_choice* draws, int n_learners,
                                void* stream);

/* ---- prioritised replay on wide minibatches (PERD3QN) ------------------------------------------------------------ */
/* THIS BUILD'S OWN -- the reference trains one world on ONE minibatch of 64 per train() (PERD3QN.py:94-115).  rl_learn_prioritized_wide
 * is rl_learn_prioritized on a minibatch of 1 .. RL_LEARN_PRIORITIZED_WIDE_MAX rows: rl_learn_dueling_wide's update (64-row tiles side by
 * side, the advantage mean taken over the WHOLE minibatch) on an RL_PERD3QN learner, plus the prioritised memory's upkeep.  A call whose
 * batch is at most 64 (one tile), given the same slots, leaves every buffer rl_learn_prioritized writes -- params, target, adam_m,
 * adam_v, state, packed, loss, grad, priority[0 .. capacity) and *prio_max -- with rl_learn_prioritized's bits.  rl_learn_prioritized,
 * rl_learn_prioritized_draw, rl_learn_dueling, rl_learn_dueling_wide and every *_supported answer are unchanged by it. */
#define RL_LEARN_PRIORITIZED_WIDE_MAX 2048
/* 1 for the brain kinds rl_learn_prioritized_wide trains (RL_PERD3QN), 0 for the others */
int rl_learn_prioritized_wide_supported(int kind);
/* The bytes of one learner's work buffer for a minibatch of `batch` rows: rl_learn_dueling_wide_work_bytes' formula (the layout is
 * rl_learn_dueling_wide's: header | partial[T] | sumA'[T] sumA[T] | stash[T], T = ceil(batch / 64)).  0, with rl_last_error set, for a
 * kind rl_learn_prioritized_wide does not train or a batch outside [1, RL_LEARN_PRIORITIZED_WIDE_MAX]. */
size_t rl_learn_prioritized_wide_work_bytes(int kind, int batch);
/* rl_learn_prioritized_draw for wide minibatches: the same two launches (prepare, pick) with the same arithmetic, batch in
 * [1, RL_LEARN_PRIORITIZED_WIDE_MAX] and ONE batch for all learners of a call.  Draw d = s * batch + j keeps its salt -- words 0-1 of
 * rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN_PRIO, d) -- so with batch <= 64 and n_steps = 1 the table is
 * rl_learn_prioritized_draw's, bit for bit, and so are weight, keys and *seen.  n_steps x batch workgroups per learner, each a pass over
 * the ring's rows.
 *   slots     device int32 [n_learners][n_steps][batch]
 * Everything else -- the stamp of the rows appended since the last draw, kind RL_PERD3QN (anything else: RL_E_UNSUPPORTED naming the
 * kind), the rings' columns (age included), every pointer of rl_prio set, alpha > 0, n_steps in [1,65536], the two deviations -- is as
 * rl_learn_prioritized_draw states it. */
int rl_learn_prioritized_wide_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                   int n_steps, int32_t* slots, void* stream);
/* PERD3QNAgent.train() (PERD3QN.py:94-115) on wide minibatches for n_learners brains, on the rl_learner / rl_replay / rl_prio structures
 * of rl_learn_prioritized and the work buffers of rl_learn_dueling_wide.
 *   update      rl_learn_dueling_wide's, launch for launch and instruction for instruction (the size gate, the range check of every slot
 *               before a row is fetched, the two tile passes, the update, `afterwards`): at any batch the eight learner buffers end with
 *               the bits rl_learn_dueling_wide leaves on an RL_D3QN learner with the same parameters, ring and slots.
 *   priorities  in the second tile pass of every step, where td is formed for every row of the batch: the thread that handles batch row
 *               i = 64 t + r of its OWN tile t writes priority[slot_i] = |max_a q'_target(s'_i) - q_eval(s_i)[a_i]| (PERD3QN.py:110-111:
 *               the reference's expression, not the TD error), each q with the mean of the WHOLE minibatch's advantages, from this
 *               step's pre-update parameters.  The value depends only on the row's contents, the parameters and the two batch-wide
 *               means, which every tile forms identically, and a row's forward arithmetic does not depend on its place in a tile: a slot
 *               drawn several times, in one tile or in several, is written with equal bits -- there is no winner rule.  Later steps of a
 *               call overwrite earlier ones (stream order).  Rows of a tile beyond the batch carry no slot and write nothing.
 *   afterwards  as rl_learn_dueling_wide, and, in a call that trained (size > min_size, no bad slot), *prio_max = max(priority[0 ..
 *               size)), size = min(*ring.count, capacity) as read at entry.  A call below the size gate leaves priority and prio_max
 *               alone (state[1] is counted and sync_target honoured as always).
 *   bad slots   a slot outside [0, size): error-flag code 6 ([1] = learner, [2] = step, [3] = the value; the first in table order), and
 *               NONE of that learner's buffers -- priority and prio_max included -- is written; the other learners train.
 *   order       PRECONDITION as rl_learn_prioritized: rl_learn_prioritized_wide_draw has run on these rings since the last row was
 *               appended (the `slots` of this call are its output).
 * 3 n_steps + 3 launches, all queued on `stream` (the count and the grids of rl_learn_dueling_wide).  No host read-back, no cooperative
 * launch, no workgroup waits for another, no allocation, no float atomics: the same buffers give the same bits in every run and
 * whatever else is in the launch.
 * Validated on the host before anything is launched: kind must be RL_PERD3QN (anything else: RL_E_UNSUPPORTED naming the kind);
 * otherwise RL_E_INVALID naming the argument: null handle / learners / rings / prios / work, slots == NULL (the draw is
 * rl_learn_prioritized_wide_draw's job), n_learners in [1, RL_MAX_CAPTURE_BRAINS], n_steps in [1,65536], batch in
 * [1, RL_LEARN_PRIORITIZED_WIDE_MAX] and equal for all learners, rl_learn_prioritized's null-pointer and capacity checks,
 * prios[i].priority / prio_max / seen not null and alpha > 0, a null work[i]. */
int rl_learn_prioritized_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                              int n_steps, const int32_t* slots, void* const* work, void* stream);

/* ---- prioritised draws by prefix sum over content-key rank (PERD3QN, PERDQN) --------------------------------------- */
/* THIS BUILD'S OWN -- the prioritised draws' tables by another sampler.  rl_learn_prioritized_draw / _wide_draw / rl_learn_td_draw race
 * exponentials: one workgroup per draw, each a pass over the ring, probabilities w_i / sum w up to about size / 2^23, and no way to
 * stratify.  Here the rows a ring holds are sorted by content key once per call (rl_learn_draw_rank's sort, kernel for kernel), the
 * weights are summed in that order, and every draw is one binary search: the cost of a call does not depend on n_steps or the batches,
 * the probabilities are w_i / sum w up to the rounding of a float64 sum, and with one uniform per segment of total / batch the draw is
 * the reference's stratified Memory.sample() (PERDQN.py:280-304).  rl_learn_prioritized_draw_rank serves RL_PERD3QN learners on rl_prio,
 * rl_learn_td_draw_rank RL_PERDQN learners on rl_tdprio.  For learner i, size = min(*ring.count, ring.capacity) read on the device:
 *   prepare   rl_learn_prioritized_draw's (rl_learn_td_draw's) prepare step, unchanged: the slots in [*seen, *count) mod capacity (all
 *             rows once count - seen >= capacity) get priority = *prio_max (TD: p_new); weight[row] = powf(priority[row], alpha) (TD: no
 *             weight column, the weight of a row is its stored priority); keys[row] = the content key, rows < size.
 *   order     host array [n_learners] of device int32 [capacity]: order[i][0 .. size) = the slots ascending by (keys[slot], slot) --
 *             numpy's lexsort((arange(size), keys[:size])), as rl_learn_draw_rank leaves it.  Entries from `size` on are left alone.
 *   cum       host array [n_learners] of device float64 [capacity], written for ranks r < size.  With w_r = (double)weight[order[r]]
 *             where that float is > 0 and w_r = 0 otherwise (a zero, a negative or a NaN weight is never drawn -- the race's rule), in
 *             IEEE float64, every + one rounded addition:
 *               local[r] = w_(64 s) + w_(64 s + 1) + ... + w_r, s = r / 64, added left to right starting from 0.0
 *               tot[s]   = local[min(64 s + 63, size - 1)]
 *               base[0]  = 0.0, base[s + 1] = base[s] + tot[s]
 *               cum[r]   = base[r / 64] + local[r],    total = cum[size - 1]
 *             numpy: np.cumsum over the rows of w padded with zeros to [n_seg][64], a sequential sum of the last column, one add.
 *             cum is nondecreasing, and a row of weight 0 has cum[r] == cum[r - 1] (rank 0: cum[0] == 0).
 *   work      host array [n_learners] of device scratch of at least rl_learn_prio_draw_rank_work_bytes(capacity) bytes each, 16-byte
 *             aligned: rl_learn_draw_rank's two tables of 65,536 counters and one int32 per row, then one float64 per segment of 64
 *             rows.  It needs no initialisation and holds nothing between calls.
 *   slots     device int32, the learners' flat [n_steps][batch] tables laid end to end.  Draw d = s * batch + j of learner i:
 *               r4 = rl_philox(seed, 0, i, (uint32)state[1], SITE, d), SITE = RL_SITE_LEARN_PRIO (PERD3QN) or RL_SITE_LEARN_TD (PERDQN)
 *                    -- the race draws' own sites: the two samplers are alternatives and never share a call
 *               x = (((uint64)r4[1] << 32) | r4[0]) >> 11,  u = (double)x * 2^-53          (exact; u in [0, 1))
 *               stratified == 0:  target = u * total                                      (one multiply)
 *               stratified != 0:  seg = total / (double)batch,  target = ((double)j + u) * seg   (one divide; one add, then one multiply)
 *               slots[d] = order[r], r the smallest rank with cum[r] > target; if there is none (rounding gave target >= total), the
 *               smallest r with cum[r] == total: the last row of positive weight in rank order
 *             No fused multiply-add anywhere.  A zero-weight row is never the smallest such rank.  total == 0, or a total that is not
 *             finite: the uniform rank draw slots[d] = order[((uint64)r4[0] * size) >> 32] -- the race's "every weight zero means
 *             uniform".  size == 0: slot 0 for every draw.  WITH replacement; independent mode is np.random.choice(p = w / sum w)
 *             (PERD3QN.py:165), stratified mode Memory.sample()'s one random.uniform(a, b) per segment.
 *   seen      the last launch advances *seen to *ring.count, as the race draws' pick launch does.
 * batch is in [1, RL_LEARN_PRIORITIZED_WIDE_MAX] (PERD3QN) or [1, 64] (PERDQN); the learners of a call may have different batches.  The
 * tables feed rl_learn_prioritized, rl_learn_prioritized_wide and rl_learn_td unchanged: their precondition -- a draw has stamped the
 * fresh rows -- is met, the stamp being the same rule.  All n_steps are drawn from the priorities as they stand at the draw.
 * RL_LEARN_PRIO_DRAW_RANK_LAUNCHES (8) launches whatever n_steps, the batches and the rings hold, all queued on `stream`: the sort's
 * five (its key pass also stamps, weighs and counts), the segments' sums (one wave per segment), the bases (one workgroup per learner)
 * and one thread per draw.  No host read-back, no allocation, integer atomics only: keys, priority, weight, order, cum and slots have
 * the same bits in every run.  The race draws, rl_learn_draw_rank and every *_supported answer are unchanged by it.
 * Validated on the host before anything is launched: the race draws' checks -- kind (anything else: RL_E_UNSUPPORTED naming the kind),
 * the rings' columns (age included), every pointer of rl_prio and alpha > 0 (rl_tdprio: priority, keys, seen), n_learners in
 * [1, RL_MAX_CAPTURE_BRAINS], n_steps (PERD3QN: [1,65536]; PERDQN: >= 1), the batch range, slots -- and, RL_E_INVALID naming the argument, a
 * null order, cum or work, a null order[i], cum[i] or work[i], and n_steps times the batches below 2^31 draws. */
#define RL_LEARN_PRIO_DRAW_RANK_LAUNCHES 8
/* The bytes of one learner's work buffer for a ring of `capacity` rows (a multiple of 16): hist | start | tmp | segment sums.  0, with
 * rl_last_error set, for a capacity outside [1, 2^31). */
size_t rl_learn_prio_draw_rank_work_bytes(long long capacity);
int rl_learn_prioritized_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_prio* prios, int n_learners,
                                   int n_steps, int stratified, int32_t* const* order, double* const* cum, void* const* work,
                                   int32_t* slots, void* stream);

/* ---- on-policy learning (PPO) ------------------------------------------------------------------------------------ */
#define RL_PPO_ROLLOUT_MAX 32
/* What a learning PPO brain needs beside its rl_learner and its rl_replay ring (which must carry `prob`): the hyperparameters of
 * Models/PPO.py:42-43 and the bookkeeping of the on-policy window, as caller-owned device buffers. */
typedef struct {
    float lmbda, eps_clip;      /* 0.95, 0.1 (PPO.py:42) */
    int32_t k_epoch;            /* Adam steps per rollout, 1..8 (PPO.py:43: 3) */
    unsigned long long* seen;   /* [1] initialise to 0: ring.count as of the last rl_learn_rollout */
    unsigned long long* fresh;  /* [1] written by rl_learn_rollout: the rows of its window; rl_learn_ppo: may be NULL (always train) */
    unsigned long long* keys;   /* [capacity] scratch of rl_learn_rollout: content keys as rl_learn_draw makes them */
} rl_ppo;
/* 1 for the brain kinds rl_learn_ppo trains (RL_PPO), 0 for the others */
int rl_learn_ppo_supported(int kind);
/* PPO.learn() (Models/PPO.py:136-162) for n_learners brains in ONE stream-ordered launch, one workgroup per brain: n_steps rollouts per
 * brain, one after the other, each the reference's learn() on the rows slots[i][s][0 .. batch) IN THAT ORDER (the GAE's order).
 * rl_learner is reused: kind = RL_PPO; params, adam_m, adam_v, state, packed; lr, gamma, beta1, beta2, eps; batch = the rows of a
 * rollout, in [1, RL_PPO_ROLLOUT_MAX]; target, min_size and sync_target are ignored (target may be NULL).
 *   network     fc1 153->256, fc2 256->256, fc_pi 256->8, fc_v 256->1, ReLU after fc1 and fc2: 107,529 parameters, state-dict order
 *   a rollout   k_epoch full-batch Adam steps, each from the current parameters: reward / 100 (in double, rounded to float, PPO.py:73);
 *               td = r + gamma v(s') (1 - done); delta = td - v(s); adv_t = gamma lmbda adv_(t+1) + delta_t backwards over the rows with
 *               no reset at done, in float32 ((float)(gamma * lmbda), one multiply, one add, no fma: what numpy 2 makes of PPO.py:144-150;
 *               numpy 1 would make it double); ratio = exp(log pi(s)[a] - log prob_a); surr1 = ratio adv, surr2 = clamp(ratio, 1 - eps_clip,
 *               1 + eps_clip) adv; loss = mean(-min(surr1, surr2)) + smooth_l1(v(s), td) (beta 1).  Nothing flows through v(s') or the
 *               advantage.  At the kinks the gradient is torch's: min gives the smaller side all of it and each side half at a tie,
 *               clamp passes it on [1 - eps_clip, 1 + eps_clip], bounds included.  Adam exactly as rl_learn_dueling makes it (double
 *               update, bias corrections in double from state[0], lr / betas / eps -- and here gamma, lmbda, eps_clip -- re-read as decimals).
 *   rows        slots: device int32 [n_learners][n_steps][batch]; NULL is refused (RL_E_INVALID): rl_learn_rollout draws them.  All are
 *               range-checked against [0, min(count, capacity)) before the first row is fetched: a bad one sets error-flag code 6 and
 *               that brain leaves with NONE of its buffers written (the others train).
 *   fresh       ppos[i].fresh given and *fresh == 0: no update and no slot check (`if self.data()`, PPO.py:76); only state[1] moves.
 *   afterwards  state[0] += k_epoch per rollout trained; state[1] += 1; `packed` is rewritten from the final params, bit for bit what
 *               rl_policy_pack_weights(RL_PPO, ...) makes.  loss [n_steps][k_epoch] and grad [n_steps * k_epoch][n_params] are written when given.
 * Validation: kind must be RL_PPO (anything else: RL_E_UNSUPPORTED naming the kind); batch in [1,32]; k_epoch in [1,8]; at most
 * RL_MAX_CAPTURE_BRAINS learners; the ring must carry `prob`.  Deterministic like rl_learn_dueling: plain f32 FMA, every sum by one thread in
 * a fixed order, no float atomics.  rl_learn, rl_learn_dueling, rl_learn_prioritized and their *_supported answers are unchanged by it. */
int rl_learn_ppo(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                 const int32_t* slots, void* stream);
/* The on-policy counterpart of rl_learn_draw: the `slots` of an rl_learn_ppo call, drawn from the rows appended since the last call --
 * PPO trains on rows its current weights made -- and, like rl_learn_draw, without depending on the slots the rows sit in.
 *   window   slots [*seen, *count) mod capacity, or the whole ring once count - seen >= capacity
 *   draws    each of the n_steps * batch draws d takes the window row whose content key (rl_learn_draw's, unchanged), mixed with words
 *            0-1 of rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN_ROLLOUT, d), is smallest: uniform over the fresh rows, WITH
 *            replacement, the same rows whatever slots they sit in.  An empty window draws slot 0.
 *   writes   keys of the window's rows, slots (the learners' [n_steps][batch] tables laid end to end), *fresh = the rows of the window,
 *            then *seen = *count.
 * Two launches, no allocation.  kind must be RL_PPO; rings need state / state_prime / action / reward / done / age / count; seen, fresh
 * and keys of every rl_ppo must be set; batch in [1,32].  Deviations from the reference: a rollout is `batch` independent draws, so the
 * GAE's neighbours are unrelated rows (in the reference: unrelated agents of one tick); all but n_steps * batch of the fresh rows go
 * unused; a launch that appends more than a ring holds keeps rows by append order. */
int rl_learn_rollout(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                     int32_t* slots, void* stream);

/* ---- on-policy learning on wide rollouts (PPO) ------------------------------------------------------------------- */
/* The TILING is this build's own; the length is not: PPO.learn() (PPO.py:136-162) trains on the WHOLE list gathered since the last call,
 * which rl_learn_ppo cannot express once it passes 32 rows.  rl_learn_ppo_wide is rl_learn_ppo on a rollout of 1 ..
 * RL_LEARN_PPO_WIDE_MAX rows, computed in 32-row tiles with one workgroup per (learner, tile), with ONE GAE recursion over the whole
 * rollout.  A call whose batch is at most 32 (one tile), given the same slots, leaves every buffer rl_learn_ppo writes -- params,
 * adam_m, adam_v, state, packed, loss, grad -- with rl_learn_ppo's bits.  rl_learn_ppo, rl_learn_rollout and every *_supported answer
 * are unchanged by it. */
#define RL_LEARN_PPO_WIDE_MAX 2048
/* 1 for the brain kinds rl_learn_ppo_wide trains (RL_PPO), 0 for the others */
int rl_learn_ppo_wide_supported(int kind);
/* The bytes of one learner's work buffer for a rollout of `batch` rows, T = ceil(batch / 32) tiles:
 *   64 + T * (16 + 256 + 4 * 107,529) = 64 + 430,388 T          (27,544,896 bytes at 2048 rows)
 *   a 64-byte header | lsum[T][2] float64: the tiles' sums of the two loss terms | td[32 T] | delta[32 T] float32: what the two tile
 *   passes exchange | partial[T][107,529] float32: the tiles' gradients.
 * 0, with rl_last_error set, for a kind rl_learn_ppo_wide does not train or a batch outside [1, RL_LEARN_PPO_WIDE_MAX]. */
size_t rl_learn_ppo_wide_work_bytes(int kind, int batch);
/* rl_learn_rollout for wide rollouts: the same two launches (prepare, pick) with the same arithmetic, batch in
 * [1, RL_LEARN_PPO_WIDE_MAX] and ONE batch for all learners of a call.  Draw d = s * batch + j keeps its salt -- words 0-1 of
 * rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN_ROLLOUT, d) -- so with batch <= 32 the table, keys, *fresh and *seen are
 * rl_learn_rollout's, bit for bit.  n_steps x batch workgroups per learner, each a pass over the window's rows.
 *   slots     device int32 [n_learners][n_steps][batch]
 * Everything else -- the window, kind RL_PPO (anything else: RL_E_UNSUPPORTED naming the kind), the rings' columns (age included), seen /
 * fresh / keys of every rl_ppo, n_steps in [1,65536], the deviations (with replacement, by content key) -- is as rl_learn_rollout states it. */
int rl_learn_rollout_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                          int32_t* slots, void* stream);
/* PPO.learn() (PPO.py:136-162) on wide rollouts for n_learners brains, on the rl_learner / rl_replay / rl_ppo structures of rl_learn_ppo.
 *   batch       learners[i].batch in [1, RL_LEARN_PPO_WIDE_MAX], ONE batch for all learners of a call; slots is device int32
 *               [n_learners][n_steps][batch].  Tile t of a rollout holds its rows 32 t .. min(32 t + 31, batch - 1).
 *   work        host array [n_learners] of caller-owned device scratch of rl_learn_ppo_wide_work_bytes bytes each, 16-byte aligned.  It
 *               needs no initialisation and carries nothing between calls.
 *   a rollout   per epoch rl_learn_ppo's arithmetic on every row -- the forward passes, the per-row scalars formed in double and rounded
 *               once, the tie and clamp rules of the gradients, reward / 100 in double -- with three rules in place of its one-workgroup ones:
 *               1. ONE GAE chain over the whole rollout: adv_t = fl(fl(gl adv_(t+1)) + delta_t), gl = (float)(gamma * lmbda), backwards from
 *                  row batch - 1 to row 0 in float32, one multiply and one add, no fma, no reset at done, whatever tile a row sits in.  A
 *                  row's delta = td - v(s) does not depend on its place in a tile (its forward arithmetic is k ascending everywhere).
 *               2. means over the whole rollout: both loss terms and their gradients are scaled by 1 / (float)batch of the WHOLE batch.
 *                  Rows of the last tile beyond the batch are zero rows with zero loss gradients and stay out of the chain.
 *               3. a tile stores its partial gradient, each parameter summed in rl_learn_ppo's order over the tile's rows; one thread per
 *                  parameter adds the tiles' partials in tile order in double, rounds to float once and makes rl_learn_ppo's Adam update
 *                  with the bias corrections of step state[0] as read at entry + the epochs made so far in the call + 1.
 *               loss[s][ep] = (float)(L1 / (double)batch + L2 / (double)batch), L1 and L2 the per-tile double sums of the rows' two loss
 *               terms (rows ascending) added in tile order from 0.0; grad[s * k_epoch + ep][n_params] is the summed, rounded gradient.
 *   fresh       ppos[i].fresh given and *fresh == 0: no update and no slot check; only state[1] moves.
 *   bad slots   every slot of a call that trains is range-checked against [0, min(count, capacity)) in a pass of its own before a row is
 *               fetched: a bad one sets error-flag code 6 ([1] = learner, [2] = step, [3] = the value; the first in table order) and
 *               NONE of that learner's buffers is written; the other learners train.
 *   afterwards  state[0] += k_epoch per rollout trained; state[1] += 1; `packed` is rewritten from the final params (rl_policy_pack_device's
 *               kernel: bit for bit what rl_policy_pack_weights(RL_PPO, ...) makes).
 * 3 n_steps K + 3 launches, K = the largest k_epoch among the call's learners, all queued on `stream`: the check; per rollout and epoch
 * the two tile passes (grid T x n_learners) and the update; the counters; the packer.  A learner with a smaller k_epoch sits out the
 * later epochs.  No host read-back, no cooperative launch, no workgroup waits for another, no allocation, no float atomics: the same
 * buffers give the same bits in every run and whatever else is in the launch.
 * Validated on the host before anything is launched: kind must be RL_PPO (anything else: RL_E_UNSUPPORTED naming the kind); otherwise
 * RL_E_INVALID naming the argument: null handle / learners / rings / ppos / work, a null work[i], slots == NULL (the draw is
 * rl_learn_rollout_wide's job), n_learners in [1, RL_MAX_CAPTURE_BRAINS], n_steps in [1,65536], batch in [1, RL_LEARN_PPO_WIDE_MAX] and
 * equal for all learners, k_epoch in [1,8], lmbda and eps_clip >= 0, rl_learn_ppo's null-pointer and capacity checks, a ring without `prob`. */
int rl_learn_ppo_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_ppo* ppos, int n_learners, int n_steps,
                      const int32_t* slots, void* const* work, void* stream);

/* ---- prioritised replay with importance weights (PERDQN) ---------------------------------------------------------- */
/* The prioritised memory of one learning PERDQN brain (Memory / SumTree, Models/PERDQN.py) beside its rl_replay ring: caller-owned
 * device buffers.  Three things the reference does are reproduced as they are (the rule of rl_learn_prioritized):
 *   1. append_sample's error is |old_val - target[0][action]| with old_val a view of the tensor the line before overwrote: exactly 0.
 *      EVERY stored row gets (0 + e) ** a as a float32 torch scalar (0.06309573), whatever the row: no forward pass is needed to store
 *      one, and p_new is that number, made by the caller.
 *   2. train_model's loss is (FloatTensor(is_weights) * F.mse_loss(pred, target)).mean(), and mse_loss is already the scalar mean:
 *      loss = mean(is_w) * mean((pred - target)^2).  The importance weights scale the whole batch, not its rows.
 *   3. Memory.sample's is_weight, (n_entries p_i / total) ** -beta divided by its maximum over the batch, is (p_i / min_j p_j) ** -beta
 *      over the batch rows: total and n_entries cancel, so the device keeps no sum tree and no total.  beta = min(1, beta + increment),
 *      in double, at every sample(). */
typedef struct {
    float* priority;            /* [capacity] */
    unsigned long long* keys;   /* [capacity] scratch: content keys as rl_learn_draw makes them */
    unsigned long long* seen;   /* [1] initialise to 0: ring.count as of the last draw */
    double* beta;               /* [1] initialise to 0.4 (Memory.beta) */
    float p_new;                /* priority of a newly stored row: the reference's float32 (0 + e) ** a, made with torch on the host */
    float prio_e, prio_a;       /* 0.01, 0.6 (Memory.e, Memory.a); prio_a must be > 0 */
    double beta_increment;      /* 0.001 (Memory.beta_increment_per_sampling) */
    float* is_weight;           /* [n_steps][batch] or NULL: the importance weights of every step (tests, diagnostics) */
} rl_tdprio;
/* 1 for the brain kinds rl_learn_td trains (RL_PERDQN), 0 for the others */
int rl_learn_td_supported(int kind);
/* The draw of that memory for n_learners PERDQN brains: rl_learn_prioritized_draw's two launches (no allocation, no host round trip,
 * independent of the slots the rows sit in) with these differences:
 *   prepare   the slots in [*seen, *ring.count) mod capacity (all of them when count - seen >= capacity) get priority = p_new, not a
 *             running maximum; keys[row] as before; there is no weight column
 *   pick      the race weight is the stored priority itself -- the reference samples in proportion to p, which already carries ** a:
 *             no powf.  salt_d = words 0-1 of rl_philox(seed, 0, i, (uint32)state[1], RL_SITE_LEARN_TD, d).  t = -logf(U) / priority;
 *             the smallest (t, v, slot) wins.  A priority of 0 or NaN loses; if every one is zero the draw is rl_learn_draw's uniform
 *             content-key draw; an empty ring draws slot 0; rows whose t tie are told apart by v.  *seen advances to *ring.count here.
 * batch in [1,64] directly.  Every learner's kind must be RL_PERDQN (anything else: RL_E_UNSUPPORTED naming the kind); rings need state /
 * state_prime / action / reward / done / age / count; priority, keys and seen must be set.
 * Deviation from the reference: Memory.sample is stratified -- one uniform per segment of total / n, found through the sum tree, which
 * names slots (and the rings' slot order differs from run to run).  Here every draw is independent with probability p_i / sum p, each
 * stratified draw's marginal without its variance reduction, by content key, WITH replacement. */
int rl_learn_td_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                     int32_t* slots, void* stream);
/* THIS BUILD'S OWN -- that draw by prefix sum over content-key rank: rl_learn_prioritized_draw_rank (above: order, cum, work, the
 * formulas, RL_LEARN_PRIO_DRAW_RANK_LAUNCHES launches and rl_learn_prio_draw_rank_work_bytes) on this memory -- fresh rows get p_new, a
 * row's weight is its stored priority, SITE = RL_SITE_LEARN_TD, batch in [1,64].  stratified != 0 is Memory.sample() itself: the total is
 * cut into `batch` segments and draw j takes one uniform in segment j -- the deviation rl_learn_td_draw states does not apply; what
 * remains is that the cumulative sum runs over the rows in content-key order, not in the sum tree's slot order.  stratified == 0: independent
 * draws with probability p_i / sum p, rl_learn_td_draw's distribution (other rows). */
int rl_learn_td_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                          int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream);
/* THIS BUILD'S OWN -- the TD error at append.  PERDQNAgent.append_sample (PERDQN.py:113-128) means to store a row with
 * (|Q(s)[a] - (r + (1 - done) gamma max_a Q_target(s'))| + e) ** a and stores it with (0 + e) ** a, because old_val (:119) is a view of
 * the tensor :121-124 overwrite (point 1 above).  The draws reproduce that constant (p_new); this call, queued IN FRONT of a draw, gives
 * the rows of the draw's window the priority the code spells out -- a departure from PERDQN.py:119-126 on purpose, opt-in, and
 * with a schedule of our own: the error is taken with params / target AS OF THIS CALL, not as of the tick that stored the row.
 *   window     the slots of [*seen, *ring.count) mod capacity, or all min(count, capacity) rows once count - seen >= capacity: exactly
 *              the rows the following draw would have stamped with p_new
 *   launch 1   one workgroup per (learner, 64 window rows), workgroups beyond the window return at once: `target` on the s' rows and
 *              max_a, `params` on the s rows, priority[slot] = powf(fabsf(q[a] - (r + mask * (gamma * max))) + prio_e, prio_a).  Every
 *              dot product is rl_learn_td's chain (from the bias, fmaf with k ascending): a stamped priority is, BIT FOR BIT, what
 *              rl_learn_td would write for that row from the same params and target.  Reads seen and count; writes priority of window
 *              rows and nothing else; no float atomics; no workgroup waits for another
 *   launch 2   one thread per learner: *seen = *ring.count (launch 1 is seen's reader)
 * A following rl_learn_td_draw / rl_learn_td_draw_rank, unchanged, finds an empty window, stamps nothing and draws by the priorities it
 * finds.  keys, beta, p_new, batch and min_size are not read; the stamp also runs below rl_learn_td's size gate.  No allocation, no host
 * round trip.  RL_E_INVALID naming the argument for: a null handle, learners, rings or tds; n_learners outside
 * [1, RL_MAX_CAPTURE_BRAINS]; null params, target, priority or seen; a null ring column among state / state_prime / action / reward /
 * done / count; capacity outside [1, 2^31); prio_a <= 0.  A kind that is not RL_PERDQN: RL_E_UNSUPPORTED naming the kind. */
#define RL_LEARN_TD_STAMP_LAUNCHES 2
int rl_learn_td_stamp(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds,
                      int n_learners, void* stream);
/* PERDQNAgent.train_model() for n_learners brains in ONE stream-ordered launch, one workgroup per brain.  rl_learner / rl_replay as for
 * rl_learn_dueling; kind = RL_PERDQN: fc.0 153->64, fc.2 64->64, fc.4 64->8, ReLU between, 14,536 parameters in state-dict order.
 *   size gate   size = min(*count, capacity); size <= min_size: no update (the caller passes train_start - 1)
 *   rows        slots: device int32 [n_learners][n_steps][batch], from rl_learn_td_draw; all are range-checked against [0, size) before
 *               the first row is fetched: a bad one sets error-flag code 6 and that brain leaves with NONE of its buffers written --
 *               priority and beta included (the others train)
 *   each step   beta = min(1, beta + beta_increment) in double; w_i = (float)pow((double)p_i / (double)p_min, -beta) over the batch
 *               rows' priorities as they stand at this step (written to is_weight when given); target_i = r_i + (1 - done_i) gamma
 *               max_a Q_target(s'_i); pred_i = Q(s_i)[a_i]; loss = mean(w) * mean((pred - target)^2); Adam exactly as rl_learn_dueling
 *               makes it; every batch row writes priority[slot] = powf(fabsf(pred - target) + prio_e, prio_a) from this step's
 *               pre-update values (duplicated slots write equal bits, later steps overwrite earlier ones); loss[s] and
 *               grad[s][n_params] are written when given
 *   afterwards  sync_target != 0: target <- params, also below the size gate (PERDQNAgent.learn calls update_target_model() after every
 *               trigger); state[0] += updates made; state[1] += 1; `packed` is rewritten from the final params, bit for bit what
 *               rl_policy_pack_weights(RL_PERDQN, ...) makes (split to the nearest f16)
 * Validation is rl_learn_dueling's with these differences: kind must be RL_PERDQN (anything else: RL_E_UNSUPPORTED naming the kind);
 * slots == NULL is RL_E_INVALID; priority, seen and beta must not be null; prio_a > 0; batch in [1,64]; at most RL_MAX_CAPTURE_BRAINS
 * learners.  Deterministic like the other learners: plain f32 FMA, every sum by one thread in a fixed order, no float atomics.
 * Every older entry point and *_supported answer is unchanged by it (they refuse RL_PERDQN). */
int rl_learn_td(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                const int32_t* slots, void* stream);

/* ---- the sum tree as the reference keeps it: Memory.add, Memory.sample, Memory.update (PERDQN, learn="reference") ------------------ */
/* Three stream-ordered entry points, one launch of one workgroup per learner each, no allocation, no host round trip, no float atomics,
 * at most RL_MAX_CAPTURE_BRAINS learners per call, kind RL_PERDQN only (anything else: RL_E_UNSUPPORTED naming the kind).  They keep the
 * memory, not the network: the update is rl_learn_td, unchanged, on the slots rl_learn_td_tree_sample names (min_size = 0: the caller
 * gates at train_start), and rl_learn_td_tree_update follows it.  Of rl_tdprio only `priority` and `p_new` are read.
 *
 * Notation.  C = the memory's capacity (Memory.capacity, PERDQN.py:269-271), in [2, 2^30]: SumTree._propagate (:209-215) never ends for
 * C = 1, whose only leaf is the root, and tree indices are int32 (anything else: RL_E_INVALID naming the capacity).  R >= C = the rows
 * the ring holds, R < 2^31 (a caller that captures a whole tick's rows in front of the tick's train_model() calls needs R = C + slack,
 * slack >= the rows of one tick).  Rows are numbered from 0 in storage order; row a sits in ring slot a % R and at the reference's memory
 * index a % C.  rl_tdprio.priority is indexed by RING SLOT and holds R floats.  `tree` is a caller-owned device double[2 C - 1] per
 * learner, zero-initialised, in the reference's layout: the leaf of memory index j at j + C - 1, the parent of node i at (i - 1) / 2.
 * update(i, p) below is SumTree.update (:248-252): change = p - tree[i]; tree[i] = p; then tree[k] = tree[k] + change for every proper
 * ancestor k of i, up to the root -- each a separately rounded double operation.  update32(i, p) is the same loop as the reference runs
 * it when p is a float32 torch scalar, which is how append_sample's priority arrives (PERDQN.py:126-128, 273-278): change =
 * (float)p - (float)tree[i] in float; tree[i] = p; tree[k] = (double)((float)tree[k] + change), the node rounded to float, the sum taken
 * in float.  Inner nodes on the path of a stored row therefore hold float32 values until an update batch touches them.
 * Between calls, for every row the memory holds: priority[row % R] == (float)tree[its leaf]; leaves only ever hold float32 values.
 * The bits of `tree` and `priority` are those of the reference's sequential loop over the same updates, in every run: change depends
 * only on the earlier updates of the same leaf and every inner node receives its changes in update order, so each node's final value
 * is computed by one thread walking the node's own subsequence of the list (rl_learn_td_ref.hip). */
typedef struct {
    double* tree;               /* device [2 C - 1] */
    long long capacity;         /* C, in [2, 2^30] */
    long long ring_rows;        /* R, in [C, 2^31) */
    long long first_row;        /* a >= 0: the first row of the group */
    long long n_rows;           /* m in [1, R - C]; anything else is RL_E_INVALID */
} rl_td_tree_store;
/* Memory.add (PERDQN.py:276-278, 234-245) for rows [a, a + m) of each learner, in row order: update32((a + j) % C + C - 1, p_new)
 * and priority[(a + j) % R] = p_new.  append_sample's error is exactly 0 (rl_tdprio, point 1), so p_new is every stored row's priority
 * and storing a row needs no forward pass. */
int rl_learn_td_tree_store(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_store* groups, int n_learners,
                           void* stream);
#define RL_LEARN_TD_TREE_BATCH_MAX 64  /* the draws of one rl_learn_td_tree_sample call, the updates of one rl_learn_td_tree_update call, per learner at most */
typedef struct {
    const double* tree;         /* device [2 C - 1] */
    long long capacity;         /* C, in [2, 2^30] */
    long long ring_rows;        /* R, in [C, 2^31) */
    long long stored;           /* rows stored so far, >= 1 */
    int32_t n;                  /* the draws, in [1, RL_LEARN_TD_TREE_BATCH_MAX] */
    const double* u;            /* device [n]: the host's random.random() draws, in [0,1) */
    int32_t* idxs;              /* device [n]: TREE indices (the reference's idxs), in [C - 1, 2 C - 1) */
    int32_t* slots;             /* device [n]: the ring slots of the rows those leaves hold, what rl_learn_td takes */
    double* s;                  /* device [n] or NULL: each draw's point s_i (tests, diagnostics) */
    double* leaves;             /* device [n] or NULL: tree[idxs[i]] (tests, diagnostics) */
} rl_td_tree_sample;
/* Memory.sample(n)'s draw (PERDQN.py:280-298) from host-drawn uniforms, random.uniform(a, b) being a + (b - a) * random.random().  Per
 * learner, one thread per draw i, every operation a separately rounded double:
 *   segment = tree[0] / n;  a_i = segment * i;  b_i = segment * (i + 1);  s_i = a_i + (b_i - a_i) * u_i
 *   _retrieve: k = 0; while 2 k + 1 < 2 C - 1: left = 2 k + 1; if s <= tree[left]: k = left, else: s = s - tree[left], k = left + 1
 *   idxs[i] = k;  j = k - (C - 1);  slots[i] = (j + C * ((stored - 1 - j) / C)) % R  (integer division: the latest row at memory index j)
 *   s[i] = s_i (as drawn, before the walk) and leaves[i] = tree[k], where given
 * Refused on the device with error-flag code 8: a draw with j >= min(stored, C) -- a leaf no row has reached, where the reference's
 * `while True` (:291-295) draws again from a generator the device does not have -- or a total that is not a positive finite number.
 * EVERY draw of that learner then gets idxs = C - 1 and the slot of memory index 0; s and leaves are not written; the other learners of
 * the call are untouched.  The run has then left the reference's draw order.
 * Refused on the host (RL_E_INVALID naming the argument): stored < 1, n outside its range, a null tree / u / idxs / slots, C or R
 * outside their ranges. */
int rl_learn_td_tree_sample(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_sample* draws, int n_learners,
                            void* stream);
typedef struct {
    double* tree;               /* device [2 C - 1] */
    long long capacity;         /* C, in [2, 2^30] */
    long long ring_rows;        /* R, in [C, 2^31) */
    int32_t n;                  /* the updates, in [1, RL_LEARN_TD_TREE_BATCH_MAX] */
    const int32_t* idxs;        /* device [n]: tree indices, as rl_learn_td_tree_sample wrote them */
    const int32_t* slots;       /* device [n]: their ring slots */
} rl_td_tree_update;
/* train_model's loop (PERDQN.py:175-177) behind rl_learn_td, which has rewritten priority[slots[i]]: for i = 0 .. n - 1 in order,
 * update(idxs[i], (double)priority[slots[i]]).  A leaf named twice gets equal bits twice: its second change is 0.  An idxs[i] outside
 * [C - 1, 2 C - 1) or a slots[i] outside [0, R) is skipped and sets error-flag code 9. */
int rl_learn_td_tree_update(rl_world* h, const rl_learner* learners, const rl_tdprio* tds, const rl_td_tree_update* batches, int n_learners,
                            void* stream);

/* THIS BUILD'S OWN -- the reference trains one world on ONE minibatch of 64 per train_model() (PERDQN.py:130-186).  rl_learn_td_wide is
 * rl_learn_td on a minibatch of 1 .. RL_LEARN_TD_WIDE_MAX rows, computed in 64-row tiles with one 512-thread workgroup per (learner,
 * tile).  The rows of a step meet in two scalars, p_min and mean(is_w), both over the WHOLE batch, and the tiles rewrite the priorities
 * those are read from: so every step has a weights pass of its own in front of its tiles, and no workgroup reads a priority that a
 * workgroup of the same launch can write. */
#define RL_LEARN_TD_WIDE_MAX 2048
/* the launches one rl_learn_td_wide call queues: check | per step: weights, tiles, update | target / counters / beta | pack */
#define RL_LEARN_TD_WIDE_LAUNCHES(n_steps) (3 * (n_steps) + 3)
/* 1 for the brain kinds rl_learn_td_wide trains (RL_PERDQN), 0 for the others */
int rl_learn_td_wide_supported(int kind);
/* The bytes of one learner's work buffer at `batch`: a 64-byte header, one partial gradient row of rl_policy_n_params floats per tile
 * and the tiles' sums of td^2, T = ceil(batch / 64) tiles.  0, with rl_last_error set, for a kind rl_learn_td_wide does not train or a
 * batch outside [1, RL_LEARN_TD_WIDE_MAX]. */
size_t rl_learn_td_wide_work_bytes(int kind, int batch);
/* rl_learn_td_draw (two launches) and rl_learn_td_draw_rank (RL_LEARN_PRIO_DRAW_RANK_LAUNCHES launches; stratified != 0 cuts the total
 * into `batch` segments) for these learners: the same kernels and arithmetic with batch in [1, RL_LEARN_TD_WIDE_MAX], ONE batch for all
 * learners of a call and n_steps in [1,65536].  Draw d = s * batch + j keeps its salt -- words 0-1 of rl_philox(seed, 0, i,
 * (uint32)state[1], RL_SITE_LEARN_TD, d) -- so with batch <= 64 the tables are rl_learn_td_draw's and rl_learn_td_draw_rank's, slot for
 * slot.  Validation is theirs with the batch limit and the one-batch rule (RL_E_INVALID naming both batches); rl_learn_td_draw and
 * rl_learn_td_draw_rank keep their limit of 64 and their messages. */
int rl_learn_td_wide_draw(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                          int32_t* slots, void* stream);
int rl_learn_td_wide_draw_rank(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                               int stratified, int32_t* const* order, double* const* cum, void* const* work, int32_t* slots, void* stream);
/* PERDQNAgent.train_model() on wide minibatches for n_learners brains: RL_LEARN_TD_WIDE_LAUNCHES(n_steps) stream-ordered launches, no
 * allocation, no host round trip, no cooperative launch, no float atomics, no workgroup that waits for another.
 *   batch       learners[i].batch in [1, RL_LEARN_TD_WIDE_MAX], ONE batch B for all learners of a call; slots is device int32
 *               [n_learners][n_steps][B], from rl_learn_td_wide_draw / rl_learn_td_wide_draw_rank (or the caller's)
 *   work        host array [n_learners] of caller-owned device scratch of rl_learn_td_wide_work_bytes bytes each, 16-byte aligned.  It
 *               needs no initialisation and holds nothing between calls
 *   check       once: the size gate min(*count, capacity) > min_size; every slot of every step of a learner that trains is
 *               range-checked against [0, size) before anything is written -- a bad one sets error-flag code 6 as rl_learn_td does
 *               ([1] = brain index, [2] = step, [3] = the slot) and that learner leaves with NONE of its buffers written, priority and
 *               beta included, while the others train; the counters as read at entry go into the work buffer's header
 *   weights     per step, one workgroup per learner, finished before any tile of the step starts and started after every tile of the
 *               previous step: beta = min(1, beta + beta_increment) in double; the step's B priorities as they stand; p_min by fminf
 *               over the rows ascending; w_i = (float)pow((double)p_i / (double)p_min, -beta), each by its own thread, to
 *               is_weight[s][0..B) when given; per tile the f32 sum of w, rows ascending; the tile sums added in double in tile order
 *               from the additive identity (-0.0) and rounded to float once; mean_w = that * (1.0f / B)
 *   tiles       per step, one workgroup per (learner, 64 rows): rl_learn_td's arithmetic thread for thread -- the target forward on s',
 *               the eval forward on s, td = pred - target, row_g = mean_w * ((2 td) * (1 / B)) with B the whole batch; the row's own
 *               tile writes priority[slot] = powf(fabsf(td) + prio_e, prio_a) (duplicated slots, also across tiles, carry equal bits:
 *               no winner rule); the tile's f32 sum of td^2 and its partial gradient of all 14,536 parameters (f32 sums over the
 *               tile's rows, ascending) go to the work buffer
 *   update      per step, one thread per parameter: the tiles' partials added in tile order in double (from -0.0), rounded once, then
 *               rl_learn_td's Adam update; grad[s] and loss[s] = mean_w * (sum_sq * (1 / B)) are written when given, sum_sq formed from
 *               the tile sums as mean_w's sum is
 *   afterwards  sync_target != 0: target <- params, also below the size gate; state[0] += updates made; state[1] += 1; *beta is written
 *               iff the learner trained; `packed` is rewritten from the final params by rl_policy_pack_device's kernel
 * With one tile (B <= 64) and the same slots every buffer -- params, target, adam_m, adam_v, state, packed, priority, beta, is_weight,
 * loss, grad -- ends with rl_learn_td's bits: float -> double -> float is the identity.  Deterministic: the same bits in every run,
 * whatever else is in the launch.  Validation is rl_learn_td's with these differences: batch in [1, RL_LEARN_TD_WIDE_MAX] and equal for
 * all learners, n_steps in [1,65536], work and every work[i] non-null (RL_E_INVALID naming the argument); a kind that is not RL_PERDQN:
 * RL_E_UNSUPPORTED naming the kind.  rl_learn_td keeps its limit of 64 and its messages. */
int rl_learn_td_wide(rl_world* h, const rl_learner* learners, const rl_replay* rings, const rl_tdprio* tds, int n_learners, int n_steps,
                     const int32_t* slots, void* const* work, void* stream);

/* ---- learning on several ranks: one merge of the learners per learning episode ------------------------------------- */
/* THIS BUILD'S OWN -- the reference has no multi-process training.  Every rank trains its learners on its own rings exactly as a single
 * rank does; at the end of a learning episode the ranks export their learners into one row each, all-gather the rows (the caller's
 * collective) and merge: periodic PARAMETER averaging, not gradient averaging.  Memory-side state (rings, priorities, windows, beta,
 * state[1]) stays rank-local.
 * The floats of one rank's row segment for a learner of `kind`: 3 * rl_policy_n_params(kind) + 2, laid out params | adam_m | adam_v |
 * state[0], the step count as two 32-bit words, low then high, in the bytes of two floats (3 * 53,897 is odd: nothing may assume 8-byte
 * alignment).  -1 for an unknown kind. */
int64_t rl_learn_merge_floats(int kind);
/* ONE launch: learner i's segment, which starts at the sum of the earlier learners' rl_learn_merge_floats, is filled from its buffers
 * (params, adam_m, adam_v, state; target and packed are not read and may be NULL).  row: device, at least the sum of all segments. */
int rl_learn_export(rl_world* h, const rl_learner* learners, int n_learners, float* row, void* stream);
/* The merge.  rows: device [n_ranks][row_stride_floats], as an all-gather of the exported rows lays them out; it must not overlap a
 * learner's buffer.  Per learner, with s_r the step count of rank r's row:
 *   participants  the ranks with s_r == max_r s_r (all of them when the counts are equal, which covers "nobody trained"); decided on
 *                 the device from the rows' step words, no read-back
 *   the mean      every element of params, adam_m and adam_v becomes the participants' mean: summed in rank order in double (from
 *                 -0.0, the additive identity), divided by their number in double, rounded to float ONCE -- the same bits on every
 *                 rank, in every run, whatever else is in the launch; one participant: its values, bit for bit
 *   state         state[0] <- max_r s_r (a rank that is behind adopts the result); state[1] is untouched
 *   target        sync_target != 0: target <- the merged params; otherwise left alone.  RL_PPO: target may be NULL
 *   packed        rewritten from the merged params, bit for bit what rl_policy_pack_weights(kind, ...) makes of them
 * Kinds may be mixed within a call (n_learners in [1, RL_MAX_CAPTURE_BRAINS], n_ranks in [1, 64]); of rl_learner only kind, the six
 * buffers and sync_target are read.  Two launches (mean, pack), stream-ordered, no allocation, no host read-back.  Validated on the host
 * before anything is launched: a null buffer, a bad count or a stride shorter than the learners' segments is RL_E_INVALID, a kind no
 * learner has is RL_E_UNSUPPORTED, each naming the learner.  The handle supplies nothing but its presence; it need not be bound. */
int rl_learn_merge(rl_world* h, const rl_learner* learners, int n_learners, const float* rows, int n_ranks, int64_t row_stride_floats,
                   void* stream);
/* rl_policy_pack_weights on the device, all five kinds, ONE launch: params device [rl_policy_n_params(kind)] -> packed device
 * [rl_policy_packed_floats(kind)], 16-byte aligned.  Every float the host packer writes gets the same bits. */
int rl_policy_pack_device(int kind, const float* params, float* packed, void* stream);

/* ---- frames ---------------------------------------------------------------------------------------------------- */
/* What the painter of Helpers/render.py:51-239 draws, as integers: pixels per cell, the body square (offset, side, border width), the
 * two eye squares (side, y offset, x offsets) and the food square (offset, side) inside a cell -- computed by the host with the
 * reference's own expressions; a square whose side is <= 0 is not drawn. */
typedef struct {
    int32_t grid_size;                          /* pixels per cell, 1..64 */
    int32_t body_off, body_size, border;        /* border = 2 (render.py:153) */
    int32_t eye_size, eye_y, eye_x0, eye_x1;
    int32_t food_off, food_size;
    int32_t n_colors;                           /* >= 1 */
    const double* colors;                       /* device [n_colors][3]: Visualize.colors (a gene's colour is colors[gene mod n_colors]) */
    const uint8_t* tiles;                       /* device [height][width][3]: every cell's background colour */
} rl_render_style;
/* Paints n_frames frames from the bound rl_state (read only) into frames [n_frames][height*gs][width*gs][3] (uint8 RGB, screen x = j,
 * screen y = i; any alignment), stream-ordered, no host round trip.  Per pixel of cell (i, j), the first that applies: the food square
 * (cell_type food white, poison black, super food red), an eye (black), the border of the body square (red with RL_F_KILLED, else
 * body * (1 - health / 205) in float64), the body (colors[gene mod n_colors]), the tile.  Colours are clipped to [0, 255] and
 * truncated.  The agent of a cell is the LAST entry k < n_agents with RL_F_DEAD clear and (a_i, a_j) = (i, j) on the grid.
 *   worlds  device int32 [n_frames]: the world of every frame (any order, repeats allowed), or NULL = worlds 0 .. n_frames-1.
 *           An id outside [0, n_worlds) leaves that frame untouched and sets the bound error flag (code 5).
 * Nothing but `frames` (and the error flag) is written. */
int rl_render(rl_world* h, const rl_render_style* style, const int32_t* worlds, int n_frames, uint8_t* frames, void* stream);

/* ---- options -------------------------------------------------------------------------------------------------- */
/* Tuning / test switches (nothing like them in the reference).  Process-level values start from the environment, read ONCE
 * (RL_WORLD_BLOCK, RL_WORLD_GENERIC, RL_POLICY_VARIANT, RL_RUN_ALWAYS), and change only through rl_set_option;
 * rl_create copies them into the handle, so a handle's kernels never change under it and no launch reads the environment.
 *   "world_block"      "0" (by world count) | "256" | "512" | "1024": workgroup size of the world kernels and of rl_run
 *   "world_generic"    "1": the generic world code also for the default 30x30 / 100-agent shape
 *   "policy_variant"   "auto" (default: the tiles of rl_run's policy half -- ONE arithmetic on every path: `pair`, or `dense` for
 *                      dueling brains from 1,536 tiles on, bit-identical to each other) | "pair" | "dense" | "wave" (one wave per
 *                      tile, dueling kinds; the same bits).  Every variant computes the same Q values bit for bit.
 *   "run_always"       "1": callers that choose between rl_run and the two-launch loop by world count take rl_run
 * value NULL restores what the environment says.  rl_get_option: the handle's snapshot (h != NULL) or the process level (h == NULL);
 * policy_variant as 0 auto, 2 wave, 3 dense, 4 pair; -1 for an unknown name. */
int rl_set_option(const char* name, const char* value);
int rl_get_option(const rl_world* h, const char* name);

/* Philox4x32-10 exactly as the kernels use it (host helper for tests / tools) */
void rl_philox(uint64_t seed, uint32_t epoch, uint32_t world, uint32_t tick, uint32_t site, uint32_t index,
               uint32_t out[4]);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
