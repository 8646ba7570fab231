"""trainer(): same signature, defaults and return value as ReinLife/Helpers/trainer.py:7-107.

The loop is the reference's (get_action -> step -> learn -> update_env, trainer.py:85-99) with get_action batched on the
GPU through env.act().  A single world (rng="reference", the default for n_worlds == 1 outside a multi-rank job) makes every random draw of the
loop exactly as the reference does, so the same seeds give the same run; replicated worlds draw in-kernel.

By default (learn=None) the run is INFERENCE ONLY: training=True (the reference's default) keeps the loop, the epsilon schedules and
the Tracker, but the brains do not learn -- Environment warns about it, and save=True writes the weights as they were loaded /
initialised (settings.json says so).  learn="device" trains the DQN brains on the GPU (rl_learn); see trainer()'s docstring for how
its schedule and sampling differ from the reference's."""
import time

import torch

from ..World.environment import Environment


def trainer(brains, n_episodes=10_000, width=30, height=30, visualize_results=False, google_colab=False, update_interval=500,
            print_results=True, max_agents=100, render=False, static_families=True, training=True, save=True,
            limit_reproduction=False, incentivize_killing=True, *, n_worlds=1, device=None, seed=0, rng=None, per_agent_api=False,
            fused=None, synthetic_agents=None, refill_below=None, dist=None, world_base=None, learn=None, learn_every=None,
            learn_steps=5, learn_kinds=None, learn_prioritized=None, learn_rollout=None, rollout_steps=1,
            learn_td_priority=None, learn_td_stamp=None, learn_ranks=None, learn_reference_prioritized=None,
            learn_reference_td=None, learn_batch=None, learn_draw=None):
    """Extra keyword-only arguments: n_worlds / device / seed / rng / synthetic_agents / refill_below (Environment); per_agent_api=True makes the reference's literal
    per-agent get_action / learn calls; fused (default: True for rng="philox" without per_agent_api) runs the loop through
    Environment.run -- whole chunks of ticks per launch, ending where the Tracker closes an interval -- instead of three launches
    and a host round trip per tick; fused=False keeps the tick-by-tick loop (same results, tests/test_hip_round3.py).
    The wall time of the loop itself is left in env.loop_seconds.
    Several GPUs: start one process per GPU (torchrun) and initialise torch.distributed (backend "nccl" = RCCL) before the
    call -- or pass the process-group module as `dist`.  Every rank then owns `n_worlds` replicas (global ids rank * n_worlds ...: the
    worlds are the same whatever the number of ranks), runs on cuda:LOCAL_RANK unless `device` says otherwise, and the Tracker's
    per-interval statistics (tracker.py:107-121) are pooled over ALL ranks' worlds by one all-gather of the ranks' per-world sums per closed interval --
    the only collective of the loop; every rank returns the same `env.tracker.results`.
    learn="device" (default None: nothing learns, as before): every DQN brain of `brains` trains on the GPU.  The multi-tick launches
    append each tick's transitions to per-brain replay rings of 50,000 (DQN.py:15); after every episode that is a multiple of
    `learn_every` (default: the brains' train_freq, 20) three launches follow the chunk -- two that draw the minibatches (rl_learn_draw) and
    ONE rl_learn that makes `learn_steps` (default 5, DQN.py:143) minibatch updates per brain -- batch 32, gamma 0.98, smooth-L1, Adam, only once a ring holds more than 1000 transitions -- copies agent ->
    target (DQN.py:83) and rewrites the packed weights the worlds act with, all on the same stream with no host round trip; after the
    loop the trained parameters are copied into the brains' modules, so save=True writes them.  Brains of other kinds stay frozen (a
    warning names them).  Needs rng="philox", the fused path, static_families=True, training=True and a single rank -- or several with learn_ranks="average", below --
    (ValueError otherwise).  TWO DEVIATIONS from the reference: (1) the schedule -- the reference calls train() per agent whenever its age is a
    multiple of train_freq or it died (DQN.py:85-89: over a thousand dependent train() calls per tick at 256 worlds); here a brain
    trains once per `learn_every` ticks of world time, as a single long-lived agent would cause; (2) minibatches are drawn uniformly
    WITH replacement, where the reference's random.sample (DQN.py:100) draws without -- and by a key of the rows' content mixed with
    Philox bits rather than by slot, because the worlds append to a ring in a timing-dependent order: a second identical call gives the
    same parameters bit for bit unless one chunk appends more than a ring holds.
    learn="reference": the call a ReinLife user already has -- trainer([DQN(), DQN()]) -- trains, and from the same seeds it trains the
    way the reference does.  One world, rng="reference", static_families=True, training=True, per_agent_api=False, fused None or False,
    a single rank, and none of the learn_* keywords below (ValueError otherwise, before a device is touched): the brains' own attributes
    set the hyperparameters.  The loop is act -> step -> env.learn_reference(n_epi) -> update_env: one capture of the tick's transitions,
    then, per agent of the post-step list with age > 1, in list order, what its brain's learn() does when `age % train_freq == 0 or dead`
    -- DQN: five minibatches of random.sample(deque, 32) once the deque holds more than 1000 rows, target copy (rl_learn, one launch);
    D3QN: once n_epi > exploration one update on random.sample(deque, batch_size), eval -> target when n_epi is a multiple of
    soft_update_freq (rl_learn_dueling); PPO: one learn() over all rows stored since the last one, k_epoch epochs (rl_learn_ppo up to 32
    rows, rl_learn_ppo_wide up to 2048; a longer list is a ValueError).  random.sample consumes the process-global `random` stream as in
    the reference, so the run's draws stay the reference's.  PERD3QN and PERDQN brains stay frozen in this mode (a warning names them).
    learn_kinds (default None = ("DQN",): exactly the above): the brain methods that train.  learn_kinds=("DQN", "D3QN") also trains every
    D3QN brain, through rl_learn_dueling: its ring holds brain.capacity rows (10,000, D3QN.py:62); after an episode `last` that is a
    multiple of `learn_every` (default: the smallest train_freq of all learners) and greater than brain.exploration (D3QN.py:121) one
    launch makes ONE minibatch update (D3QNAgent.train(), D3QN.py:97-116: batch 64, gamma 0.99, lr 1e-3, MSE with the reference's
    batch-wide advantage mean, Adam) as soon as the ring holds 64 rows; the target network is synced in that launch iff a multiple of
    brain.soft_update_freq lies in (last - learn_every, last] (D3QN.py:125-126).  The DQN learners' call is a separate launch and draws
    what it draws without D3QN learners.  The same two deviations apply.  learn_steps: an int is the DQN learners' count; a dict by
    method name ({"DQN": 5, "D3QN": 1, "PERDQN": 1}) sets it per kind.  A learn_kinds name no entry point trains (PERD3QN, PPO, PERDQN), or learn_kinds without
    learn="device", is a ValueError before a device is touched.
    learn_prioritized (default None: every run is what it was; True needs learn="device" and at least one Models.PERD3QN, ValueError
    otherwise, before a device is touched; it needs no learn_kinds; the default `learn_every` stays the smallest train_freq of the DQN /
    D3QN learners -- a PERD3QN's train_freq sets it only where PERD3QN brains are the only learners): every PERD3QN brain trains through rl_learn_prioritized on a
    prioritised memory beside a ring of brain.capacity rows (10,000, PERD3QN.py:49).  The schedule is the D3QN learners': after an
    episode `last` that is a multiple of `learn_every` and greater than brain.exploration (PERD3QN.py:120), behind the DQN and D3QN
    calls (which stay bit for bit what they are without the keyword), one prioritised draw (rl_learn_prioritized_draw: rows appended
    since the last draw get the priority maximum, PERD3QN.py:147; then 64 draws with probability priority^0.6 / sum, with replacement,
    PERD3QN.py:157-165) and ONE update (PERD3QNAgent.train(), PERD3QN.py:94-115: the D3QN update on the plain MSE loss -- the reference
    computes importance weights and never uses them -- then priority = |max_a q'_target(s') - q_eval(s)[a]| for the batch rows); the
    target is synced iff a multiple of brain.soft_update_freq lies in (last - learn_every, last].  The same two deviations apply: a
    brain trains once per `learn_every` episodes, so ALL rows appended between two calls get the maximum as of the earlier call (the
    reference's per-agent train() calls change it in between); draws are by content key.  The run-to-run caveat is sharper here: a ring
    holds only 10,000 rows and a chunk of 256 worlds appends far more than that, so which rows survive depends on append order --
    a second identical call repeats bit for bit only while no chunk appends more than the ring holds.
    learn_rollout (default None: every run is what it was; True needs learn="device" and at least one Models.PPO, ValueError otherwise,
    before a device is touched; it needs no learn_kinds; a PPO's train_freq sets the default `learn_every` only where PPO brains are
    the only learners): every PPO brain trains through rl_learn_ppo.  The rings then also record the acting probability of every row
    (PPO.py:73).  After every episode that is a multiple of `learn_every`, behind the DQN, D3QN and PERD3QN calls (which stay bit for
    bit what they are without the keyword), one on-policy draw (rl_learn_rollout, two launches) names `rollout_steps` (default 1)
    rollouts of 32 rows among the rows appended since the last call, and ONE rl_learn_ppo makes PPO.learn() (PPO.py:136-162) on each:
    k_epoch (3) full-batch Adam steps on the clipped surrogate plus the smooth-L1 value loss, GAE backwards over the rollout's rows.
    DEVIATIONS: the schedule (once per `learn_every` episodes, not per agent); a rollout is 32 independent draws with replacement, so
    the GAE's neighbours are unrelated rows -- in the reference they are unrelated agents of one tick; all but rollout_steps * 32 of the
    fresh rows go unused; a chunk that appends more than a ring holds keeps rows by append order.
    learn_td_priority (default None: every run and every message is what it was; True needs learn="device" and at least one Models.PERDQN,
    ValueError otherwise, before a device is touched; it needs no learn_kinds; a PERDQN's train_freq sets the default `learn_every` only
    where PERDQN brains are the only learners): every PERDQN brain trains through rl_learn_td beside a ring of brain.memory_size rows
    (20,000).  A brains list with a PERDQN runs in the two-launch loop, which captures every tick's transitions into the rings.  After
    every episode that is a multiple of `learn_every`, behind all the other learners' calls (which stay bit for bit what they are
    without the keyword), one draw (rl_learn_td_draw, two launches) and ONE rl_learn_td make learn_steps["PERDQN"] (default 1)
    train_model() updates once the ring holds brain.train_start rows: batch 64, gamma 0.99, lr 1e-3, Adam; model -> target_model at
    every call.  Three quirks of the reference are reproduced, not repaired: every stored row gets the one priority (0 + 0.01) ** 0.6
    (append_sample's error is taken against a view of the tensor it has just overwritten); the loss is mean(is_weight) *
    mean((pred - target)^2), not weighted per row; is_weight = (p_i / min_j p_j) ** -beta over the batch, beta 0.4 -> 1 by 0.001 per
    update.  DEVIATIONS: the reference's sample() is stratified through its sum tree -- here the 64 draws are independent with
    probability p_i / sum p, by content key, with replacement; the schedule is per `learn_every` episodes, so brain.epsilon decays
    once per update made, not once per agent trigger (pass a smaller explore_step for the reference's rate in wall-clock terms).  Until a
    ring first holds train_start rows each learning call reads its count back (a synchronisation); afterwards none does.
    learn_td_stamp (default None: every run is launch for launch and bit for bit what it was; "error" needs learn_td_priority=True, and
    with it learn="device" and a Models.PERDQN; anything else is a ValueError before a device is touched): THIS BUILD'S OWN, a departure
    from the first of those three quirks on purpose.  Every learning call then queues one rl_learn_td_stamp (two launches) in front of
    the PERDQN draw -- the race draw and learn_draw={"PERDQN": "rank"} alike: every row appended since the last draw gets
    (|Q(s)[a] - (r + (1 - done) gamma max_a Q_target(s'))| + 0.01) ** 0.6, the priority append_sample's code spells out, from a forward
    pass of both networks over the fresh rows, and the draw that follows finds no fresh row and draws by these priorities.  The error
    is taken with the parameters AS OF THE LEARNING CALL, not as of the tick that stored the row (the reference's append_sample runs per
    stored row, between its per-agent train_model() calls): the schedule is ours.  Count read-back, epsilon's decay, the other
    families and learn_ranks="average" are untouched; priorities stay rank-local.
    learn_ranks (default None: learning needs a single rank, as before; "average" needs learn="device", anything else is a ValueError
    before a device is touched): training on several ranks, THIS BUILD'S OWN -- the reference has no multi-process training.  Every
    rank trains its learners on its own rings exactly as above (draws, calls, priorities and PPO windows are rank-local and unchanged).
    At set-up the ranks compare a signature of their learners and schedule (a mismatch raises on every rank), take rank 0's parameters
    by one broadcast, zero Adam's moments and repack on the device.  Every learning episode then ends with one launch that exports the
    learners into a row, ONE all-gather of the rows, and two launches that merge them (rl_learn_merge): per learner the ranks with the
    highest Adam step count take part, params / adam_m / adam_v become their mean -- summed in rank order in double, rounded once, the
    same bits on every rank -- the step count the maximum, the target the merged params where it was synced in this episode, and the
    packed acting weights are rewritten from the merged params.  This is periodic PARAMETER averaging, not gradient averaging: D3QN,
    PERD3QN and PERDQN make one update per episode from identical parameters and moments (the mean of R one-step Adam updates); DQN
    makes learn_steps local steps and PPO k_epoch per rollout before the ranks meet.  Rings, priorities, windows, beta and a PERDQN's
    host-side epsilon stay rank-local.  The merge also runs on one rank and without a process group (the identity, three launches).
    learn_batch (default None: every run is bit for bit what it was; an int in [1, 2048] needs learn="device" and at least one Models.DQN
    among the learning kinds, ValueError otherwise, before a device is touched): THIS BUILD'S OWN -- the reference's minibatch is 32 rows
    (DQN.py:16), sized for one world.  Every DQN learner then trains through rl_learn_wide: each of the `learn_steps` updates is one Adam
    step on a minibatch of learn_batch rows, computed in 32-row tiles that run side by side (one workgroup per brain and tile) and
    summed in tile order in double -- the same bits in every run.  Draw, schedule, gate (1000 rows), gamma, loss and target copy are the
    DQN learners'; a call is 2 learn_steps + 3 launches instead of one.  learn_batch=32 gives the parameters learn_batch=None gives, bit
    for bit.  The learning rate stays the brain's: a wider batch averages more rows per step, it does not take more steps.
    learn_batch also takes a dict by kind, like learn_steps: {"DQN": B}, {"D3QN": B} or both (keys from these two, at least one; ints in
    [1, 2048]; a named kind must be among learn_kinds and have a brain in the list: ValueError otherwise, before a device is touched).
    "D3QN" (this build's own -- the reference's minibatch is 64 rows, D3QN.py:98): every D3QN learner trains through
    rl_learn_dueling_wide, each update one Adam step on a minibatch of B rows computed in 64-row tiles side by side, with
    dueling_ddqn.forward's advantage mean (D3QN.py:165) taken over the WHOLE minibatch as the reference takes it -- the tiles meet in
    three scalars per step, summed in tile order in double, the same bits in every run.  Schedule, gate (exploration, a ring of at least
    batch_size rows), learn_steps per kind, target sync rule, learning rate, learn_draw and learn_ranks are the D3QN learners'; a call is
    3 learn_steps["D3QN"] + 3 launches instead of one.  {"D3QN": 64} gives the learners that learn_kinds alone gives, bit for bit.
    With learn_prioritized=True (and only then: without it the key stays unknown) the dict also takes "PERD3QN" (this build's own -- the
    reference's minibatch is 64 rows, PERD3QN.py:49, 95): every PERD3QN learner trains through rl_learn_prioritized_wide, rl_learn_dueling_wide's
    tiled update on a minibatch of B rows drawn by priority (rl_learn_prioritized_wide_draw: the prioritised draw at that width), with the
    priority of every one of the B rows rewritten from the whole batch's means and the maximum kept for the rows appended next.  Schedule,
    gate (exploration, one row), ONE update per call, target sync rule, learning rate and learn_ranks are the PERD3QN learners'; a call
    is 2 + 6 launches instead of 2 + 1.  {"PERD3QN": 64} gives the learners that learn_prioritized=True alone gives, bit for bit,
    priorities and prio_max included.
    With learn_rollout=True (and only then: without it the key stays unknown) the dict also takes "PPO": every PPO learner trains through
    rl_learn_ppo_wide on rollouts of B rows in [1, 2048] -- PPO.learn() (PPO.py:136-162) trains on the whole list gathered since the last
    call, which rl_learn_ppo's 32 rows cannot express; the tiling is this build's own: 32-row tiles side by side, ONE GAE recursion over
    the whole rollout across the tiles, both means over all B rows, the tiles' gradients summed in tile order in double -- the same bits
    in every run.  The draw is rl_learn_rollout_wide (the on-policy draw at that width: with replacement, by content key);
    rollout_steps, schedule, the empty-window gate, k_epoch, learning rate and learn_ranks are the PPO learners'; a call is
    2 + 3 rollout_steps k_epoch + 3 launches instead of 2 + 1.  {"PPO": 32} gives the learners that learn_rollout=True alone gives, bit for bit.
    With learn_td_priority=True (and only then: without it the key stays unknown) the dict also takes "PERDQN" (this build's own -- the
    reference's minibatch is 64 rows, PERDQN.py:130-186): every PERDQN learner trains through rl_learn_td_wide, train_model()'s update on a
    minibatch of B rows in [1, 2048] computed in 64-row tiles side by side.  The importance weights (p_i / min_j p_j) ** -beta and their
    mean run over the WHOLE batch, as Memory.sample() makes them: a pass of its own in front of every step's tiles takes the minimum and
    the mean from the priorities as they stand, the tiles then rewrite the priority of every one of the B rows, and the tiles' gradients
    are summed in tile order in double -- the same bits in every run.  The draw is rl_learn_td_wide_draw (the race draw at that width) or,
    with learn_draw={"PERDQN": "rank"}, rl_learn_td_wide_draw_rank, stratified into B segments; learn_steps["PERDQN"], the train_start
    gate, the target copy at every call, the epsilon decay, learn_td_stamp and learn_ranks are the PERDQN learners'; a call is
    3 learn_steps["PERDQN"] + 3 launches instead of one.  {"PERDQN": 64} gives the learners that learn_td_priority=True alone gives, bit
    for bit, priorities and beta included.
    learn_draw (default None: every run is launch for launch and bit for bit what it was; "rank" needs learn="device" and at least one
    brain of the learning kinds -- one that rl_learn, rl_learn_wide or rl_learn_dueling trains -- anything else is a ValueError before a
    device is touched): THIS BUILD'S OWN.  The DQN, wide DQN and D3QN learners' minibatches are then drawn by rl_learn_draw_rank instead of
    rl_learn_draw: the rows a ring holds are sorted by content key once per call (ties: the lower slot) and draw d takes the row at rank
    ((uint64)x_d * size) >> 32, x_d the draw's Philox word -- uniform with replacement and independent of the order the worlds appended
    the rows in, as before, but ANOTHER sampler: other rows, other parameters.  Six launches per draw instead of two, at a cost that does
    not grow with learn_steps x learn_batch (rl_learn_draw visits every key of a ring once per draw).  The prioritised, rollout and
    PERDQN draws are untouched; learn_ranks="average" needs nothing (draws are rank-local).
    learn_draw as a dict by kind, like learn_batch -- keys from "DQN", "D3QN", "PERD3QN", "PERDQN", the only value "rank", every key a kind
    that has a learner in this run ("PERD3QN" needs learn_prioritized=True, "PERDQN" learn_td_priority=True), checked before a device is
    touched.  {"DQN": "rank"} / {"D3QN": "rank"} is the string for that kind alone.  {"PERD3QN": "rank"}: the prioritised draw is
    rl_learn_prioritized_draw_rank -- the same stamp of the fresh rows, the sort above, the weights priority^0.6 summed in rank order in
    float64 and one binary search per draw: independent draws with probability weight / sum, as the reference's np.random.choice(p=...),
    at any learn_batch["PERD3QN"], eight launches instead of two at a cost that does not grow with the batch.  {"PERDQN": "rank"}:
    rl_learn_td_draw_rank, the same STRATIFIED -- the total cut into 64 segments, one uniform per segment: the reference's Memory.sample(),
    which the race draw cannot do.  Both are other samplers than the race draws: other rows, other parameters.

    learn_reference_prioritized (default None: learn="reference" is what it was, PERD3QN brains stay frozen and are named by its warning;
    True needs learn="reference" and at least one Models.PERD3QN, ValueError before a device is touched): every PERD3QN brain trains on
    the reference's schedule too -- PERD3QNAgent.learn (PERD3QN.py:117-125) has D3QNAgent.learn's shape.  Its priorities stay on the device,
    one per row of a ring of capacity + slot_cap rows: the host draws np.random.random_sample(batch_size), exactly the doubles
    np.random.choice(len, batch_size, p=probs) consumes, and three launches follow per train(): rl_learn_prioritized_store_ref (store()'s
    maximum for the rows stored since the last stamp), rl_learn_prioritized_choice (the cdf walk, indices and slots staying on the device)
    and rl_learn_prioritized on those slots.  np.random ends every tick in the reference's state.  The device's probabilities agree with
    numpy's to a few float32 ulps, so a uniform within about 2^-21 of a cdf boundary may name the neighbouring row: with capacity=10000
    that happens about once in some tens of train() calls, and a long run then leaves the reference's row choices while sampling the same
    distribution.  PERDQN brains stay frozen and the warning names them.

    learn_reference_td (default None: learn="reference" is what it was, with or without learn_reference_prioritized, and PERDQN brains stay
    frozen; True needs learn="reference" and at least one Models.PERDQN, ValueError before a device is touched): every PERDQN brain trains
    on the reference's schedule too -- PERDQNAgent.learn (PERDQN.py:188-195): store; on the trigger, once the memory holds train_start
    rows, one train_model() and the target copy.  The memory's sum tree stays on the device as float64 [2 capacity - 1] in the
    reference's layout and with the reference's rounding: every node ends with the bits the reference's sequential update loop gives it.
    The host draws [random.random() for _ in range(batch_size)], the doubles Memory.sample's random.uniform calls consume, and four
    launches follow per train_model(): rl_learn_td_tree_store (the rows stored since the last group, each with append_sample's constant
    priority), rl_learn_td_tree_sample (the stratified walk; tree indices and ring slots stay on the device), rl_learn_td on those slots,
    rl_learn_td_tree_update.  brain.epsilon loses epsilon_decay per train_model() while above epsilon_min, on the host, so act()'s coins
    follow the reference.  `random` ends every tick in the reference's state as long as no draw lands on a leaf no row has reached --
    there the reference draws again, which the host cannot know: the device sets error-flag code 8 and trainer() raises at the end of the
    loop."""
    if learn == "device" and (per_agent_api or fused is False):
        raise ValueError("trainer(learn='device') needs the fused path (fused=True, per_agent_api=False): the replay rings are filled "
                         "inside the multi-tick launches")
    if learn == "reference" and per_agent_api:
        raise ValueError("trainer(learn='reference') needs per_agent_api=False: the brains' own learn() stays a no-op, the tick's learning "
                         "calls are made by env.learn_reference(n_epi)")
    if learn == "reference" and fused:
        raise ValueError("trainer(learn='reference') needs fused=None or fused=False: it is the tick-by-tick loop of one world with "
                         "rng='reference' (the fused path is learn='device')")
    env = Environment(width=width, height=height, max_agents=max_agents, brains=brains, grid_size=24,
                      static_families=static_families, update_interval=update_interval, print_results=print_results,
                      interactive_results=visualize_results, google_colab=google_colab, training=training,
                      limit_reproduction=limit_reproduction, incentivize_killing=incentivize_killing, n_worlds=n_worlds,
                      device=device, seed=seed, rng=rng, synthetic_agents=synthetic_agents, refill_below=refill_below, dist=dist,
                      world_base=world_base, learn=learn, learn_every=learn_every, learn_steps=learn_steps, learn_kinds=learn_kinds,
                      learn_prioritized=learn_prioritized, learn_rollout=learn_rollout, rollout_steps=rollout_steps,
                      learn_td_priority=learn_td_priority, learn_td_stamp=learn_td_stamp, learn_ranks=learn_ranks, learn_batch=learn_batch, learn_draw=learn_draw,
                      learn_reference_prioritized=learn_reference_prioritized, learn_reference_td=learn_reference_td)
    env.reset()
    if fused is None:
        fused = env.rng == "philox" and not per_agent_api
    if fused and (env.rng != "philox" or per_agent_api):
        raise ValueError("trainer(fused=True) needs rng='philox' and per_agent_api=False")
    if env.rng == "philox":
        env._bind_brains()   # set-up like reset(): the brains' weights are packed for the matrix cores and uploaded once
    env._sync()
    t0 = time.perf_counter()
    if fused and not render:
        env.run(0, n_episodes + 1)      # trainer.py:85-99, n_episodes + 1 iterations
    else:
        for n_epi in range(n_episodes + 1):
            if fused:
                env.run(n_epi, 1)
            elif per_agent_api:  # the reference's literal per-agent calls (slow; API compatibility)
                for agent in env.agents:
                    agent.get_action(n_epi)
                env.step()
                if training:
                    for agent in env.agents:
                        agent.learn(n_epi=n_epi)
                env.update_env(n_epi)
            else:
                env.act(n_epi)
                env.step()
                if learn == "reference":       # trainer.py:95-96: every agent's learn(), as one capture and the schedule's calls
                    env.learn_reference(n_epi)
                env.update_env(n_epi)
            if render:  # trainer.py:101-102
                env.render(fps=120)
    torch.cuda.synchronize(env.worlds.device)      # the loop is over when the device is
    env.loop_seconds = time.perf_counter() - t0
    env.worlds.check_error_flag()                  # (a read-back of its own: after the clock)
    env.sync_learners()                            # learn="device": the trained parameters into the brains' modules
    if save:
        env.save_results()
    return env
