"""The host model of the replay rings that transition capture fills (shared by tests/test_capture_ring_cpu.py and
tests/test_hip_capture_ring.py): what k_capture (rl_world.hip, behind rl_capture_transitions) and capture_reserve / capture_rows inside
k_run (rl_run.hip, behind rl_run_ex with `replays`) must leave in a brain's ring, stated from the oracle's per-tick, per-world transitions
(oracle/capture_np.py on OracleWorlds state), the ring's capacity and its count before the launch.

The rules (include/reinlife_hip.h, rl_replay: "slot (count % capacity) in Agent.learn call order per world"):
  count        count after a launch == count before + the rows appended, exactly.
  one world    row n of a brain's call-order list sits in slot (count0 + n) % capacity; later rows overwrite earlier ones -- the
               reference's deque(maxlen=capacity) (expect_one_world).
  many worlds  when the launch appends at most `capacity` rows to the ring (check_block): the slot block [count0, count0 + total) %
               capacity holds the launch's transitions as a multiset of whole rows, compared byte-wise; every (world, tick) list is one
               contiguous run of the block in call order (ONE atomic reserves it) -- checked run by run wherever the run's first row occurs
               once in the block, so that its place is known; every slot outside the block keeps the bytes it had before the launch.
  prob         the taken action's entry of the policy outputs of the tick-by-tick handle, gathered by src and action (tick_transitions'
               "src"), rides in the row as four more bytes.

A row is the bytes of (state[153] f32 | state_prime[153] f32 | reward f32 | age i32 | action i8 | done u8 [| prob f32]): nothing is
compared with a tolerance anywhere."""
import collections

import numpy as np

OBS = 153
ROW_BYTES = 2 * OBS * 4 + 4 + 4 + 1 + 1
WRAPS_BELOW = 4096          # a ring of the table with a capacity below this is there to wrap (the lap floor applies to it)
LAP_FLOOR = STRADDLE_FLOOR = 3

Row = collections.namedtuple("Row", "name worlds width height max_agents slot_cap n_new thr static capacities count0 chunks why")

_ONE = (1, 1, 3, 12, 24, 19, 24, 16)               # 100 ticks; launches of 1 .. 24 ticks
_SIX = (1, 2, 3) + (3,) * 29                       # 32 launches of at most 3 ticks, 93 ticks
# (100 ticks on the one-world rows: under the device's own actions the mixed set's DQN brain appended 997 rows in 60 ticks -- 3 laps of its
# 300 rows and 2 straddles, below the floor of 3; the floors are asserted on the oracle's counts at run time)
# capacities: (the two of the dueling pair's brains, the three of the mixed set's)
TABLE = [
    Row("one-world", 1, 30, 30, 100, 256, 100, 70, True, ((257, 300), (257, 300, 283)), 0, _ONE,
        "exact slots, several laps, a prime capacity"),
    Row("one-world-2^32", 1, 30, 30, 100, 256, 100, 70, True, ((257, 40_000), (257, 40_000, 300)), 2 ** 32 - 100, _ONE,
        "counts preset to 2**32 - 100; one ring that never wraps beside one that does"),
    Row("crowded", 1, 64, 64, 250, 512, 250, 150, True, ((512, 613), (512, 613, 521)), 0, _ONE,
        "more than 64 rows per brain and tick: several 64-lane passes, the wrap inside a pass"),
    Row("six-worlds", 6, 30, 30, 100, 256, 100, 70, True, ((2048, 1999), (2048, 1999, 2003)), 0, _SIX,
        "the multi-world block rule; launches of at most 3 ticks stay within capacity; every ring crosses its end 3 times or more"),
    Row("non-static", 6, 30, 30, 100, 256, 100, 70, False, ((2048, 2048), (2048, 2048, 2048)), 0, _SIX,
        "brains follow genes"),
]
BY_NAME = {r.name: r for r in TABLE}
SEED, WORLD_BASE = 31, 0


def config(row, n_brains):
    return dict(width=row.width, height=row.height, max_agents=row.max_agents, n_brains=n_brains, static_families=row.static,
                limit_reproduction=False, incentivize_killing=True, slot_cap=row.slot_cap)


def capacities(row, n_brains):
    return row.capacities[n_brains - 2]


def floor_rows(n_worlds, slot_cap):
    """The smallest ring both capture entry points accept: the most rows one tick of all worlds can append to one ring."""
    return n_worlds * slot_cap


# ---------------------------------------------------------------------------------------------------------------------
# the oracle's transitions
# ---------------------------------------------------------------------------------------------------------------------
def tick_transitions(ow, acts, thr, n_new):
    """One tick of the trainer loop on an OracleWorlds (step, update_env, refill) under `acts` [R, cap] -> per world the dict of
    capture_np.transitions (Agent.learn call order) plus "src": the pre-step list index of every row's agent (where its policy output is)."""
    from oracle import capture_np
    prev = ow.obs2.copy()
    ow.step(acts)
    n1 = ow.s["n_agents"].copy()
    out = []
    for w in range(ow.R):
        n = int(n1[w])
        tx = capture_np.transitions(prev[w], acts[w], ow.src1[w, :n], ow.s["a_age"][w, :n], ow.s["a_flags"][w, :n], ow.reward[w, :n],
                                    ow.done[w, :n], ow.obs1[w, :n], ow.s["a_brain"][w, :n])
        tx["src"] = ow.src1[w, :n][tx["k"]].astype(np.int64)
        out.append(tx)
    ow.update()
    ow.refill(thr, n_new)
    return out


def pack_rows(tx, sel=None, prob=None):
    """The transitions tx[sel] (a dict of arrays keyed like capture_np.transitions / a ring) -> uint8 [n, ROW_BYTES (+ 4 with prob)]."""
    pick = (lambda a: np.asarray(a)) if sel is None else (lambda a: np.asarray(a)[sel])
    n = len(pick(tx["action"]))
    cols = [np.ascontiguousarray(pick(tx["state"]), np.float32).reshape(n, OBS).view(np.uint8).reshape(n, OBS * 4),
            np.ascontiguousarray(pick(tx["state_prime"]), np.float32).reshape(n, OBS).view(np.uint8).reshape(n, OBS * 4),
            np.ascontiguousarray(pick(tx["reward"]), np.float32).view(np.uint8).reshape(n, 4),
            np.ascontiguousarray(pick(tx["age"]), np.int32).view(np.uint8).reshape(n, 4),
            np.ascontiguousarray(pick(tx["action"]), np.int8).view(np.uint8).reshape(n, 1),
            np.ascontiguousarray(pick(tx["done"]), np.uint8).reshape(n, 1)]
    if prob is not None:
        cols.append(np.ascontiguousarray(prob if sel is None else np.asarray(prob)[sel], np.float32).view(np.uint8).reshape(n, 4))
    return np.ascontiguousarray(np.concatenate(cols, axis=1))


def ring_bytes(ring, with_prob=False):
    """A ring as host arrays (a dict with state, state_prime, action, reward, done, age[, prob], each [capacity, ...]) -> uint8 [capacity, row]."""
    return pack_rows(ring, prob=ring["prob"] if with_prob else None)


def brain_runs(ticks, brain, probs=None):
    """ticks: a launch's list (per tick) of tick_transitions results -> the launch's (world, tick) call-order lists for `brain`, tick by
    tick and world by world, each as packed rows.  probs: per tick per world the policy outputs [cap, 8] of that tick, or None."""
    runs = []
    for t, worlds in enumerate(ticks):
        for w, tx in enumerate(worlds):
            sel = tx["brain"] == brain
            prob = None if probs is None else probs[t][w][tx["src"], tx["action"].astype(np.int64)]
            runs.append(pack_rows(tx, sel, prob))
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# the ring's rules
# ---------------------------------------------------------------------------------------------------------------------
def expect_one_world(before, count0, rows):
    """before: the ring's bytes [capacity, row]; rows [n, row] in call order -> the bytes the ring must hold after they were appended from
    count0 on: row n in slot (count0 + n) % capacity, a later row over an earlier one."""
    cap = before.shape[0]
    after = before.copy()
    n = len(rows)
    keep = np.arange(max(0, n - cap), n)        # (the last `capacity` rows: every earlier one has been overwritten)
    after[(count0 + keep) % cap] = rows[keep]
    return after


def check_one_world(before, after, count0, count1, rows, tag=""):
    """The one-world rule, slot by slot over the whole ring (the untouched slots included)."""
    assert count1 == count0 + len(rows), "%s: count %d != %d + %d rows" % (tag, count1, count0, len(rows))
    want = expect_one_world(before, count0, rows)
    if after.tobytes() != want.tobytes():
        bad = np.nonzero((after != want).any(axis=1))[0]
        raise AssertionError("%s: %d of %d slots differ from the call-order rule, first %s" % (tag, len(bad), len(want), bad[:8].tolist()))
    return dict(rows=len(rows))


def _key(row):
    return row.tobytes()


def check_block(before, after, count0, count1, runs, tag=""):
    """The several-worlds rule for one launch.  runs: the launch's (world, tick) call-order lists (packed rows, empty ones allowed).
    -> dict(rows, runs, placed: runs whose place was known and checked, torn: always 0 here)."""
    cap = before.shape[0]
    total = sum(len(r) for r in runs)
    assert count1 == count0 + total, "%s: count %d != %d + %d rows" % (tag, count1, count0, total)
    assert total <= cap, "%s: the launch appends %d rows to a ring of %d: outside the rule (a condition on the inputs)" % (tag, total, cap)
    slots = (count0 + np.arange(total)) % cap
    block = after[slots]
    outside = np.ones(cap, bool)
    outside[slots] = False
    if after[outside].tobytes() != before[outside].tobytes():
        bad = np.nonzero(outside)[0][(after[outside] != before[outside]).any(axis=1)]
        raise AssertionError("%s: %d slots outside the launch's block changed, first %s" % (tag, len(bad), bad[:8].tolist()))
    where = collections.defaultdict(list)
    for i in range(total):
        where[_key(block[i])].append(i)
    want = collections.Counter(_key(r) for run in runs for r in run)
    got = collections.Counter({k: len(v) for k, v in where.items()})
    if want != got:
        missing, extra = sum((want - got).values()), sum((got - want).values())
        raise AssertionError("%s: the block is not the launch's transitions: %d rows of the oracle's list missing, %d rows that are none of "
                             "its transitions" % (tag, missing, extra))
    placed = 0
    for i, run in enumerate(runs):
        if len(run) and len(where[_key(run[0])]) == 1:
            at = where[_key(run[0])][0]
            assert at + len(run) <= total and block[at:at + len(run)].tobytes() == run.tobytes(), \
                "%s: run %d (%d rows) is not one contiguous stretch of the block in call order (its first row is at %d)" % (tag, i, len(run), at)
            placed += 1
    return dict(rows=total, runs=sum(1 for r in runs if len(r)), placed=placed)


def count_foreign(ring, count, pool):
    """How many of the ring's filled slots hold bytes that are not one whole transition of `pool` (an iterable of packed rows): the
    characterisation count of the overfull ring."""
    known = {_key(r) for r in pool}
    filled = min(int(count), ring.shape[0])
    return sum(1 for i in range(filled) if _key(ring[i]) not in known)


# ---------------------------------------------------------------------------------------------------------------------
# what a trajectory reaches (conditions on the inputs)
# ---------------------------------------------------------------------------------------------------------------------
def reach(counts, caps, count0, chunks):
    """counts [ticks, worlds, brains]: rows appended per tick, world and brain (the oracle's); chunks: ticks per launch -> per brain
    dict(total, laps: times the count passed a multiple of capacity, straddles: one-world reservations (a tick's rows) that begin before
    the ring's end and finish behind it, crossings: launches whose block does, most_tick: most rows one world appends in a tick,
    most_launch: most rows one launch appends)."""
    counts = np.asarray(counts, np.int64)
    out = []
    for b, cap in enumerate(caps):
        c = counts[:, :, b]
        pos, t0 = int(count0), 0
        straddles = crossings = most_launch = 0
        one = counts.shape[1] == 1
        for k in chunks:
            start = pos
            for t in range(t0, t0 + k):
                for w in range(counts.shape[1]):
                    n = int(c[t, w])
                    if one and n and pos % cap + n > cap:
                        straddles += 1
                    pos += n
            if pos > start and start % cap + (pos - start) > cap:
                crossings += 1
            most_launch = max(most_launch, pos - start)
            t0 += k
        out.append(dict(total=pos - int(count0), laps=pos // cap - int(count0) // cap, straddles=straddles, crossings=crossings,
                        most_tick=int(c.max()) if c.size else 0, most_launch=most_launch))
    return out


def assert_reach(row, caps, figures, tag=""):
    """The floors of the table, from reach()'s figures (printed by the caller first)."""
    for b, (cap, f) in enumerate(zip(caps, figures)):
        if cap < WRAPS_BELOW:
            assert f["laps"] >= LAP_FLOOR, "%s brain %d: %d laps of a ring of %d (floor %d)" % (tag, b, f["laps"], cap, LAP_FLOOR)
            if row.worlds == 1:
                assert f["straddles"] >= STRADDLE_FLOOR, "%s brain %d: %d reservations straddle the ring's end (floor %d)" % (tag, b, f["straddles"], STRADDLE_FLOOR)
            else:
                assert f["crossings"] >= STRADDLE_FLOOR, "%s brain %d: %d launches cross the ring's end (floor %d)" % (tag, b, f["crossings"], STRADDLE_FLOOR)
        if row.worlds > 1:
            assert f["most_launch"] <= cap, "%s brain %d: a launch appends %d rows to a ring of %d" % (tag, b, f["most_launch"], cap)
    if row.name == "crowded":
        assert max(f["most_tick"] for f in figures) > 64, "%s: no ring takes more than 64 rows of the world in one tick" % tag


def count_rows(ticks, n_brains):
    """ticks: per tick the tick_transitions result -> counts [ticks, worlds, brains]."""
    return np.array([[[int((tx["brain"] == b).sum()) for b in range(n_brains)] for tx in worlds] for worlds in ticks], np.int64)


def run_oracle_random(row, n_brains, seed=SEED):
    """The row's worlds from reset_synthetic under seeded random actions for sum(row.chunks) ticks -> per tick the tick_transitions result."""
    from oracle import oracle as orc
    ow = orc.OracleWorlds(n_worlds=row.worlds, seed=seed, world_base=WORLD_BASE, **config(row, n_brains))
    ow.reset_synthetic(row.n_new)
    rng = np.random.RandomState(seed)
    return [tick_transitions(ow, rng.randint(0, 8, size=(row.worlds, ow.cap)).astype(np.int8), row.thr, row.n_new)
            for _ in range(sum(row.chunks))]
