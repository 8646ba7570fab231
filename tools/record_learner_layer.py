#!/usr/bin/env python3
"""Record what the Python learner layer does, on the CPU: DeviceLearner's keyword resolution and tensors, the C calls DeviceWorlds.learn
and the draw_* methods make, and the calls Environment.learn_now queues -- as one JSON document (tests/learner_layer_recorded.json).
tests/test_learner_layer_cpu.py derives the same document from the code under test and compares it for equality.

No device is touched: learners are built on "cpu" over rings of CPU tensors; DeviceWorlds is made with __new__ over a library stand-in
that records every launching call and passes the pure queries (*_supported, *_bytes, rl_policy_*, rl_learn_merge_floats) through to the
real library; Environment is built over a recording stand-in for DeviceWorlds.

    python tools/record_learner_layer.py            # writes tests/learner_layer_recorded.json
    python tools/record_learner_layer.py --check    # compares instead, exit status 1 on a difference

Every distinct message (an entry name, an error's type and text, a call's description, the brains' epsilons) is stored once, in
"messages"; the cases refer to it by index.  A learn_now record is [last, rings full?, its list of calls, the brains' epsilon, the learners' trained_from]."""
import ctypes as C
import itertools
import json
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reinlife_amd import Models, _lib, distributed, learn, worlds   # noqa: E402
from reinlife_amd.World import environment                          # noqa: E402

OUT = os.path.join(ROOT, "tests", "learner_layer_recorded.json")
ENTRIES = ("rl_learn", "rl_learn_dueling", "rl_learn_prioritized", "rl_learn_ppo", "rl_learn_td", "rl_learn_wide", "rl_learn_dueling_wide",
           "rl_learn_prioritized_wide")
BRAINS = ("DQN", "D3QN", "PERD3QN", "PPO", "PERDQN")
# (a): the cross product, in this order of the axes
AXES = (("brain", BRAINS), ("prioritized", (False, True)), ("rollout", (False, True)), ("td_priority", (False, True)),
        ("prioritized_batch", (None, 64, 0, True)), ("wide_batch", (None, 96, 0)), ("dueling_batch", (None, 130, 0)))
# how to build a learner of each entry
HOW = {"rl_learn": ("DQN", {}), "rl_learn_dueling": ("D3QN", {}), "rl_learn_prioritized": ("PERD3QN", dict(prioritized=True)),
       "rl_learn_ppo": ("PPO", dict(rollout=True)), "rl_learn_td": ("PERDQN", dict(td_priority=True)),
       "rl_learn_wide": ("DQN", dict(wide_batch=96)), "rl_learn_dueling_wide": ("D3QN", dict(dueling_batch=130)),
       "rl_learn_prioritized_wide": ("PERD3QN", dict(prioritized=True, prioritized_batch=130))}
DRAWS = {"draw_slots": ("rl_learn", "rl_learn_wide", "rl_learn_dueling", "rl_learn_dueling_wide"),
         "draw_slots_rank": ("rl_learn", "rl_learn_wide", "rl_learn_dueling", "rl_learn_dueling_wide"),
         "draw_prioritized": ("rl_learn_prioritized", "rl_learn_prioritized_wide"), "draw_rollout": ("rl_learn_ppo",), "draw_td": ("rl_learn_td",)}
TENSORS = ("target", "work", "priority", "weight", "keys", "prio_max", "seen", "fresh", "beta_is")
SCALARS = ("batch", "min_size", "n_steps_default", "sync_target", "lr", "gamma", "train_freq", "exploration", "soft_update_freq", "lmbda",
           "eps_clip", "k_epoch", "train_start", "memory_size", "alpha", "p_new", "trained_from")


class Messages:
    def __init__(self):
        self.list, self.index = [], {}

    def __call__(self, value):
        key = json.dumps(value)
        if key not in self.index:
            self.index[key] = len(self.list)
            self.list.append(value)
        return self.index[key]

    def error(self, e):
        return self("%s: %s" % (type(e).__name__, e))


class _Reached(Exception):
    pass


def _stop(*a, **k):
    raise _Reached()


def _ring(capacity=96, count=0):
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    return {"state": torch.empty((capacity, _lib.OBS_DIM)), "state_prime": torch.empty((capacity, _lib.OBS_DIM)), "action": z(capacity, dtype=torch.int8),
            "reward": z(capacity), "done": z(capacity, dtype=torch.uint8), "prob": z(capacity), "age": z(capacity, dtype=torch.int32),
            "count": torch.full((1,), count, dtype=torch.int64)}


def _learner(entry, ring=True, **brain_kw):
    torch.manual_seed(1)
    method, kw = HOW[entry]
    return learn.DeviceLearner(getattr(Models, method)(**brain_kw), "cpu", ring=_ring() if ring else None, **kw)


def _outcome(msg, call):
    try:
        call()
        return "ok"
    except Exception as e:  # noqa: BLE001
        return msg.error(e)


# ---- (a) ----
def record_resolution(msg):
    brains = {m: getattr(Models, m)() for m in BRAINS}
    out, real = [], torch.as_tensor
    torch.as_tensor = _stop
    try:
        for case in itertools.product(*[values for _, values in AXES]):
            kw = dict(zip([n for n, _ in AXES], case))
            l = learn.DeviceLearner.__new__(learn.DeviceLearner)
            try:
                l.__init__(brains[kw.pop("brain")], "cuda:0", **kw)
                raise AssertionError("the constructor was not stopped")
            except _Reached:
                out.append(msg(l.entry))
            except ValueError as e:
                out.append(msg.error(e))
    finally:
        torch.as_tensor = real
    return out


# ---- (b) ----
def record_learners(msg):
    out = {}
    for entry in ENTRIES:
        l, bare = _learner(entry), _learner(entry, ring=False)
        rec = {"entry": l.entry, "merge_floats": l.merge_floats, "scalars": {n: getattr(l, n) for n in SCALARS if hasattr(l, n)},
               "tensors": {n: [list(getattr(l, n).shape), str(getattr(l, n).dtype)] for n in TENSORS if getattr(l, n, None) is not None},
               "bare_tensors": sorted(n for n in TENSORS if getattr(bare, n, None) is not None)}
        for name in ("ring_struct", "prio_struct", "td_struct", "ppo_struct"):
            rec[name] = [_outcome(msg, getattr(l, name)), _outcome(msg, getattr(bare, name))]
        rec["tensors_after_structs"] = sorted(n for n in TENSORS if getattr(l, n, None) is not None)
        if entry == "rl_learn_ppo":
            rec["fresh_null"] = [not l.ppo_struct().fresh, not l.ppo_struct(gate=False).fresh]
        out[entry] = rec
    return out


# ---- (c) ----
class RecordingLib:
    """The library's pure queries pass through; every other call is noted and answers 0."""

    def __init__(self):
        self.real, self.calls = _lib.lib(), []

    def __getattr__(self, name):
        if name.endswith(("_supported", "_bytes", "_floats")) or name.startswith("rl_policy_") or name == "rl_last_error":
            return getattr(self.real, name)
        return lambda *args: self.calls.append(_describe(name, args)) or 0


def _describe(name, args):
    """[function, argument count, the arguments' kinds, n, n_steps, per rl_learner (kind, batch, min_size, sync_target), per rl_ppo its gate]"""
    def tag(a):
        if a is None or (isinstance(a, C.c_void_p) and not a.value):
            return "null"
        if isinstance(a, C.Array):
            return "%s[%d]" % (a._type_.__name__, len(a))
        return "int" if isinstance(a, int) else "ptr"
    ints = [a for a in args if isinstance(a, int)]
    rec = [name, len(args), " ".join(tag(a) for a in args), ints[0], ints[1]]
    for a in args:
        if isinstance(a, C.Array) and a._type_ is _lib.Learner:
            rec.append([[s.kind, s.batch, s.min_size, s.sync_target] for s in a])
        if isinstance(a, C.Array) and a._type_ is _lib.Ppo:
            rec.append(["fresh null" if not s.fresh else "fresh" for s in a])
    return rec


def _device_worlds():
    dw = worlds.DeviceWorlds.__new__(worlds.DeviceWorlds)
    dw.lib, dw.handle, dw.device, dw.launches = RecordingLib(), C.c_void_p(0x1000), torch.device("cpu"), 0
    dw._stream = lambda: None
    return dw


def _call(msg, dw, what, method, learners, *args, **kw):
    """[case, the library calls made, launches counted, the shape returned or None, the error or None]"""
    dw.lib.calls, before = [], dw.launches
    returns = error = None
    try:
        got = getattr(dw, method)(learners, *args, **kw)
        returns = None if got is None else list(got.shape)
    except Exception as e:  # noqa: BLE001
        error = msg.error(e)
    return [what, [msg(c) for c in dw.lib.calls], dw.launches - before, returns, error]


def record_worlds(msg):
    dw, out = _device_worlds(), []
    ls = {e: [_learner(e) for _ in range(3)] for e in ENTRIES}
    out.append(_call(msg, dw, "learn: no learners", "learn", [], 1))
    for entry in ENTRIES:
        for n, n_steps in itertools.product((1, 3), (1, 3)):
            out.append(_call(msg, dw, "learn %s n=%d n_steps=%d" % (entry, n, n_steps), "learn", ls[entry][:n], n_steps))
        batch = ls[entry][0].batch
        out.append(_call(msg, dw, "learn %s: host slots" % entry, "learn", ls[entry][:2], 3, slots=np.zeros((2, 3, batch), np.int64)))
        out.append(_call(msg, dw, "learn %s: wrong-shaped slots" % entry, "learn", ls[entry][:2], 3, slots=np.zeros((2, 2, batch), np.int32)))
        out.append(_call(msg, dw, "learn %s: gate=False" % entry, "learn", ls[entry][:2], 1, gate=False))
        out.append(_call(msg, dw, "learn %s: too many learners" % entry, "learn", ls[entry][:1] * (_lib.MAX_CAPTURE_BRAINS + 1), 1))
        ls[entry][1].batch = batch // 2
        out.append(_call(msg, dw, "learn %s: mixed batches" % entry, "learn", ls[entry], 1))
        out.append(_call(msg, dw, "learn %s: mixed batches, slots given" % entry, "learn", ls[entry], 1, slots=np.zeros((3, 1, batch), np.int32)))
        for draw, takes in DRAWS.items():
            if entry in takes:
                out.append(_call(msg, dw, "%s %s: mixed batches" % (draw, entry), draw, ls[entry], 1))
        ls[entry][1].batch = batch
    for a, b in itertools.combinations(ENTRIES, 2):
        out.append(_call(msg, dw, "learn: mixed entries %s + %s" % (a, b), "learn", [ls[a][0], ls[b][0], ls[a][1]], 1))
    out.append(_call(msg, dw, "learn: mixed entries, too many", "learn", ls["rl_learn"][:1] * _lib.MAX_CAPTURE_BRAINS + ls["rl_learn_td"][:1], 1))
    for draw, takes in DRAWS.items():
        for entry in ENTRIES:
            if entry in takes:
                for n, n_steps in itertools.product((1, 3), (1, 3)):
                    out.append(_call(msg, dw, "%s %s n=%d n_steps=%d" % (draw, entry, n, n_steps), draw, ls[entry][:n], n_steps))
                out.append(_call(msg, dw, "%s %s: too many learners" % (draw, entry), draw, ls[entry][:1] * (_lib.MAX_CAPTURE_BRAINS + 1), 1))
            elif draw not in ("draw_slots", "draw_slots_rank"):   # (the uniform draws do not ask what they are given)
                out.append(_call(msg, dw, "%s: given %s" % (draw, entry), draw, ls[entry][:2], 1))
        if draw not in ("draw_slots", "draw_slots_rank"):
            out.append(_call(msg, dw, "%s: no learners" % draw, draw, [], 1))
    out.append(_call(msg, dw, "draw_prioritized: narrow and wide", "draw_prioritized", [ls["rl_learn_prioritized"][0], ls["rl_learn_prioritized_wide"][0]], 1))
    wide64 = learn.DeviceLearner(Models.PERD3QN(), "cpu", ring=_ring(), prioritized=True, prioritized_batch=64)
    out.append(_call(msg, dw, "draw_prioritized: narrow and wide of one batch", "draw_prioritized", [ls["rl_learn_prioritized"][0], wide64], 1))
    return out


# ---- (d) ----
class RecordingWorlds:
    """Stands in for DeviceWorlds under Environment: rings of CPU tensors, and a note of every draw and learning call."""

    def __init__(self, **kw):
        self.device, self.n_brains, self.log, self.capture, self.launches = torch.device("cpu"), kw["n_brains"], [], None, 0

    def enable_tracking(self, on=True):
        pass

    def enable_capture(self, capacity, with_prob=False):
        self.capture = [capacity if np.isscalar(capacity) else list(capacity), bool(with_prob)]
        caps = [int(capacity)] * self.n_brains if np.isscalar(capacity) else [int(c) for c in capacity]
        self.replays = [_ring(c) for c in caps]

    def _note(self, method, learners, n_steps, *more):
        self.log.append([method, [l.entry for l in learners], [l.batch for l in learners], [bool(l.sync_target) for l in learners], n_steps, *more])

    def _draw(method):   # noqa: N805
        def draw(self, learners, n_steps):
            self._note(method, learners, n_steps)
            return method
        return draw

    draw_slots, draw_slots_rank, draw_prioritized = _draw("draw_slots"), _draw("draw_slots_rank"), _draw("draw_prioritized")
    draw_rollout, draw_td = _draw("draw_rollout"), _draw("draw_td")

    def learn(self, learners, n_steps, slots=None, gate=True):
        self._note("learn", learners, n_steps, slots, gate)

    def export_learners(self, learners, out=None):
        self._note("export_learners", learners, None)
        return out

    def merge_learners(self, learners, rows, n_ranks, sync_target=None):
        self._note("merge_learners", learners, None, n_ranks, sync_target)

    def pack_device(self, kind, params, packed):
        pass


def _brains(which):
    make = {"DQN": lambda: Models.DQN(train_freq=20), "D3QN": lambda: Models.D3QN(train_freq=16), "PERD3QN": lambda: Models.PERD3QN(train_freq=12),
            "PPO": lambda: Models.PPO(train_freq=8), "PERDQN": lambda: Models.PERDQN(train_freq=4),
            "D3QN'": lambda: Models.D3QN(train_freq=18, batch_size=32, exploration=100, soft_update_freq=50),
            "PERD3QN'": lambda: Models.PERD3QN(train_freq=14, batch_size=32, exploration=100, soft_update_freq=50),
            "PERDQN'": lambda: Models.PERDQN(train_freq=6, batch_size=32)}
    torch.manual_seed(2)
    return [make[w]() for w in which]


ALL = ("DQN", "D3QN", "PERD3QN", "PPO", "PERDQN", "D3QN'")
EVERY = dict(learn_kinds=("DQN", "D3QN"), learn_prioritized=True, learn_rollout=True, learn_td_priority=True)
ENVIRONMENTS = [
    ("all kinds", ALL, EVERY),
    ("all kinds twice", ALL + ("PERD3QN'", "PERDQN'", "DQN"), EVERY),
    ("DQN alone", ("DQN",), {}),
    ("D3QN alone", ("D3QN",), dict(learn_kinds="D3QN")),
    ("PERD3QN alone", ("PERD3QN",), dict(learn_prioritized=True)),
    ("PPO alone", ("PPO",), dict(learn_rollout=True)),
    ("PERDQN alone", ("PERDQN",), dict(learn_td_priority=True)),
    ("the opt-ins alone", ("PERD3QN", "PPO", "PERDQN"), dict(learn_prioritized=True, learn_rollout=True, learn_td_priority=True)),
    ("PPO and PERDQN", ("PPO", "PERDQN"), dict(learn_rollout=True, learn_td_priority=True)),
    ("default kinds, the rest frozen", ALL, {}),
    ("both kinds, the rest frozen", ALL, dict(learn_kinds=("DQN", "D3QN"))),
    ("D3QN and rollouts, the rest frozen", ALL, dict(learn_kinds=("D3QN",), learn_rollout=True, learn_draw="rank")),
    ("learn_batch as an int", ALL, dict(EVERY, learn_batch=96)),
    ("learn_batch DQN", ALL, dict(EVERY, learn_batch={"DQN": 96})),
    ("learn_batch D3QN", ALL, dict(EVERY, learn_batch={"D3QN": 130})),
    ("learn_batch PERD3QN", ALL, dict(EVERY, learn_batch={"PERD3QN": 130})),
    ("learn_batch all three", ALL + ("PERD3QN'",), dict(EVERY, learn_batch={"DQN": 96, "D3QN": 130, "PERD3QN": 72})),
    ("learn_draw rank", ALL, dict(EVERY, learn_draw="rank")),
    ("learn_draw rank, wide", ALL, dict(EVERY, learn_draw="rank", learn_batch={"DQN": 96, "D3QN": 130, "PERD3QN": 72})),
    ("learn_ranks average", ALL, dict(EVERY, learn_ranks="average")),
    ("learn_ranks average, wide", ALL, dict(EVERY, learn_ranks="average", learn_batch={"DQN": 96, "D3QN": 130, "PERD3QN": 72})),
    ("wide D3QN, a DQN frozen", ("D3QN", "DQN"), dict(learn_kinds="D3QN", learn_batch={"D3QN": 130})),
    ("D3QN, a DQN frozen", ("D3QN", "DQN"), dict(learn_kinds="D3QN")),
    ("wide DQN, a D3QN frozen", ("D3QN", "DQN"), dict(learn_batch=64, learn_draw="rank")),
    ("steps per kind", ALL, dict(EVERY, learn_steps={"DQN": 3, "D3QN": 2, "PERDQN": 2}, rollout_steps=2, learn_every=7)),
]
LASTS = (None, 80, 500, 1090, 1200, None)   # no gate; between the two explorations; crossing 50 but not 200; past both, no multiple of 200; crossing 200


class _Captured(Exception):
    pass


def _signature(env):
    got = []

    def capture(sig, dist, device=None):
        got.extend(sig)
        raise _Captured()
    real, env.dist = distributed.check_learner_signature, object()
    distributed.check_learner_signature = capture
    try:
        env._align_learners()
    except _Captured:
        pass
    finally:
        distributed.check_learner_signature, env.dist = real, None
    return got


def record_learn_now(msg):
    out, real = [], environment.DeviceWorlds
    environment.DeviceWorlds = RecordingWorlds
    try:
        for name, which, kw in ENVIRONMENTS:
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                env = environment.Environment(brains=_brains(which), n_worlds=2, rng="philox", learn="device", print_results=False, **kw)
            rec = {"name": name, "brains": list(which), "entries": {str(k): msg(l.entry) for k, l in sorted(env.learners.items())},
                   "enable_capture": env.worlds.capture, "learn_every": env.learn_every, "weights_note": [msg(part) for part in env._weights_note().split("; ")],
                   "warnings": [msg(str(w.message)) for w in caught], "signature": _signature(env), "learn_now": []}
            for full in (False, True):
                for r in env.worlds.replays:
                    r["count"].fill_(int(r["state"].shape[0]) if full else 0)
                for last in LASTS[-2:] if full else LASTS:   # (full rings move the PERDQN learners alone, and they do not look at `last`)
                    env.worlds.log = []
                    env.learn_now(last)
                    rec["learn_now"].append([last, full, msg([msg(c) for c in env.worlds.log]), msg([getattr(b, "epsilon", None) for b in env.brains]),
                                             "".join("01"[bool(l.trained_from)] for _, l in sorted(env.learners.items()))])
            rec["learn_now_calls"] = env.learn_now_calls
            out.append(rec)
    finally:
        environment.DeviceWorlds = real
    return out


def record():
    msg = Messages()
    doc = {"axes": [[n, list(v)] for n, v in AXES], "resolution": record_resolution(msg), "learners": record_learners(msg),
           "worlds": record_worlds(msg), "learn_now": record_learn_now(msg)}
    doc["messages"] = msg.list
    return json.loads(json.dumps(doc))   # (what a reader of the file gets: tuples are lists, keys are strings)


def dumps(doc):
    return json.dumps(doc, separators=(",", ":"), sort_keys=True) + "\n"


if __name__ == "__main__":
    text = dumps(record())
    if "--check" in sys.argv[1:]:
        same = open(OUT).read() == text
        print("%s: %s" % (OUT, "reproduced byte for byte" if same else "DIFFERS from what this tree records"))
        sys.exit(0 if same else 1)
    with open(OUT, "w") as f:
        f.write(text)
    print("wrote %s: %d bytes, %d messages" % (OUT, len(text), len(json.loads(text)["messages"])))
