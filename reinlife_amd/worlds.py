"""DeviceWorlds: R independent ReinLife worlds resident in HBM, driven through the C ABI (include/reinlife_hip.h).

PyTorch is plumbing only: it owns the device buffers and the stream; all compute is libreinlife_hip.so.
Layout = `rl_state` (struct-of-arrays over worlds; a world's agent list is its on-grid agents in row-major cell
order, i.e. the reference's env.agents order -- World/grid.py:60-67).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_STATE_SPEC = [  # name, torch dtype, shape suffix
    ("cell_type", torch.uint8, "C"), ("n_agents", torch.int32, ""), ("a_i", torch.uint8, "cap"),
    ("a_j", torch.uint8, "cap"), ("a_health", torch.int32, "cap"), ("a_age", torch.int32, "cap"),
    ("a_max_age", torch.int32, "cap"), ("a_gene", torch.int32, "cap"), ("a_brain", torch.int32, "cap"),
    ("a_uid", torch.int32, "cap"), ("a_flags", torch.uint8, "cap"), ("a_action", torch.int8, "cap"),
    ("a_fitness", torch.float64, "cap"), ("max_gene", torch.int32, ""), ("next_uid", torch.int32, ""),
    ("tick", torch.int32, ""), ("epoch", torch.int32, ""), ("best_uid", torch.int32, "best"),
    ("best_fit", torch.float64, "best"), ("best_brain", torch.int32, "best")]


# Pinned staging buffers for run()'s epsilon schedules, one small ring per device for the whole process: pinning a fresh buffer per
# launch (or per Environment: trainer() builds a new one on every call) costs more than a short launch's kernel.  A slot is
# [pinned host buffer, device buffer, event recorded behind the slot's last upload].
_EPS_RING = {}


_NP = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.int32: np.int32, torch.float32: np.float32,
       torch.float64: np.float64}


def _public_raw_stream(device_index):
    return torch.cuda.current_stream(device_index).cuda_stream


# the current stream's handle for the C ABI, once per launch: torch's private accessor where this build has it (no Stream object per call,
# ~1 us), the public torch.cuda.current_stream(...).cuda_stream otherwise (a CPU-only wheel, a renamed symbol) -- same handle either way
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or _public_raw_stream


class _Snapshot:
    """DeviceWorlds.snapshot(): name -> numpy array over one host copy of the state arena; the typed views are made on first use."""

    def __init__(self, buf, layout):
        self._buf, self._layout, self._views = buf, layout, {}

    def __getitem__(self, name):
        v = self._views.get(name)
        if v is None:
            o, nb, dt, shape = self._layout[name]
            v = self._views[name] = self._buf[o:o + nb].view(_NP[dt]).reshape(shape)
        return v

    def __contains__(self, name):
        return name in self._layout

    def keys(self):
        return self._layout.keys()


class TapeRing:
    """The draws a host makes for a tick (Tape: food_k, food_u, repro_u, birth_k, produce_u, produce_choice), staged for the device.  The six
    arrays of a tape are carved out of ONE pinned host buffer and ONE device buffer -- one host-to-device copy per tape (a host that draws
    every tick uploads two tapes per tick) -- and there is a ring of SLOTS such pairs: every make() returns a FRESH Tape struct over the next
    slot's device buffer, so a caller may prepare the step's and the update's tape before launching either (until round 6 every tape aliased
    one device buffer and the second make() silently replaced the first one's draws).  A tape stays valid until the SLOTS-th make() after
    it; its slot's buffers are then rewritten in stream order -- behind every launch queued so far -- and the pinned buffer only once its
    last upload has executed.  With a CPU device (tests/test_host_api_cpu.py) the "upload" is a plain copy and nothing is pinned."""
    SLOTS = 4

    def __init__(self, n_worlds, cap, device, cur_stream=None):
        self.R, self.cap, self.device = n_worlds, cap, torch.device(device)
        self._cur_stream = cur_stream
        R = n_worlds
        spec = [("food_k", np.int32, (R, _lib.FOOD_TRIES)), ("food_u", np.float64, (R, _lib.FOOD_TRIES)), ("repro_u", np.float64, (R, cap)),
                ("birth_k", np.int32, (R, cap + 1)), ("produce_u", np.float64, (R,)), ("produce_choice", np.int32, (R,))]
        lay, off = {}, 0
        for name, dt, shape in spec:
            nb = int(np.prod(shape)) * np.dtype(dt).itemsize
            lay[name] = (off, nb, dt, shape)
            off += (nb + 255) // 256 * 256
        self.layout, self.nbytes = lay, off
        on_gpu = self.device.type == "cuda"
        self.slots = []
        for _ in range(self.SLOTS):
            host = torch.zeros(off, dtype=torch.uint8)
            if on_gpu:
                host = host.pin_memory()
            buf = host.numpy()
            dev = torch.zeros(off, dtype=torch.uint8, device=self.device)
            self.slots.append({"host": host, "dev": dev, "event": None,
                               "views": {n: buf[o:o + nb].view(dt).reshape(shape) for n, (o, nb, dt, shape) in lay.items()}})
        self.made = 0

    def make(self, tapes):
        R, cap = self.R, self.cap
        slot = self.slots[self.made % self.SLOTS]
        self.made += 1
        if slot["event"] is not None:
            slot["event"].synchronize()
        host = slot["views"]
        for w, t in enumerate(tapes):
            host["food_k"][w] = t["food_k"]
            host["food_u"][w] = t["food_u"]
            m = min(cap, len(t["repro_u"]))
            host["repro_u"][w, :m] = t["repro_u"][:m]
            host["repro_u"][w, m:] = 0
            m = min(cap + 1, len(t["birth_k"]))
            host["birth_k"][w, :m] = t["birth_k"][:m]
            host["birth_k"][w, m:] = 0
            host["produce_u"][w] = t["produce_u"]
            host["produce_choice"][w] = t["produce_choice"]
        if len(tapes) < R:   # (worlds beyond the list: zeros)
            for name in _lib.TAPE_FIELDS:
                host[name][len(tapes):] = 0
        slot["dev"].copy_(slot["host"], non_blocking=True)
        if self.device.type == "cuda":
            if slot["event"] is None:
                slot["event"] = torch.cuda.Event()
            slot["event"].record(self._cur_stream() if self._cur_stream else torch.cuda.current_stream(self.device))
        base = slot["dev"].data_ptr()
        tape = _lib.Tape(*[C.c_void_p(base + self.layout[n][0]) for n in _lib.TAPE_FIELDS])
        tape._keep = slot["dev"]   # (the struct keeps its buffer alive)
        return tape


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _Readback:
    """Host copies in flight (DeviceWorlds.readback): wait() blocks until THEY have arrived, not until the stream is idle."""

    def __init__(self, host, done):
        self.host, self.done = host, done

    def wait(self):
        self.done.synchronize()
        return [h.numpy() for h in self.host]


class DeviceWorlds:
    def __init__(self, n_worlds=1, width=30, height=30, max_agents=100, n_brains=2, static_families=True,
                 limit_reproduction=False, incentivize_killing=True, seed=0, slot_cap=None, device="cuda:0",
                 world_base=0):
        if not torch.cuda.is_available():
            raise _lib.ReinLifeHipError("DeviceWorlds needs an MI355X: torch.cuda.is_available() is False "
                                        "(there is no CPU fallback)")
        self.lib = _lib.lib()
        self.device = torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.R, self.W, self.H, self.C = n_worlds, width, height, width * height
        self.cap = slot_cap or _lib.slot_cap_for(max_agents)
        self.max_agents, self.n_brains = max_agents, n_brains
        self.world_base = int(world_base)   # global replica id of world 0 of this handle (keys the Philox streams)
        self.cfg = _lib.Config(width, height, max_agents, n_brains, self.cap, n_worlds, int(static_families),
                               int(limit_reproduction), int(incentivize_killing), world_base, seed)
        self.handle = C.c_void_p()
        _lib.check(self.lib.rl_create(C.byref(self.cfg), C.byref(self.handle)), "rl_create")
        dims = {"C": (self.C,), "cap": (self.cap,), "best": (_lib.N_BEST,), "": ()}
        with torch.cuda.device(self.device):
            R, cap = self.R, self.cap
            # The world state and every small per-tick output live in ONE allocation (`_arena`, each array 256-byte aligned inside it), so
            # that a host which has to look at a world every tick -- Environment(rng="reference"): the reference's generator draws are
            # made on the host -- fetches all of it with ONE copy (snapshot()) instead of one small copy per array.  The kernels see
            # plain pointers, as before.
            spec = [(n, dt, (R,) + dims[suf]) for n, dt, suf in _STATE_SPEC]
            spec += [("actions", torch.int8, (R, cap)), ("n_acted", torch.int32, (R,)), ("reward", torch.float32, (R, cap)),
                     ("done", torch.uint8, (R, cap)), ("src1", torch.int16, (R, cap)), ("src2", torch.int16, (R, cap)),
                     ("n_post", torch.int32, (R,)), ("pre_counts", torch.int32, (R, 4)), ("err", torch.int32, (4,)),
                     ("out_q", torch.float32, (R, cap, 8))]
            self._layout, off = {}, 0
            for name, dt, shape in spec:
                nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
                self._layout[name] = (off, nbytes, dt, shape)
                off += (nbytes + 255) // 256 * 256
            self._arena = torch.zeros(off, dtype=torch.uint8, device=self.device)
            self._arena_host = None
            carve = {name: self._arena[o:o + nb].view(dt).view(shape) for name, (o, nb, dt, shape) in self._layout.items()}
            self.s = {n: carve[n] for n, _, _ in _STATE_SPEC}
            self.s["best_uid"].fill_(-1)
            self.s["max_gene"].fill_(n_brains)
            self.actions, self.n_acted, self.reward, self.done = carve["actions"], carve["n_acted"], carve["reward"], carve["done"]
            self.src1, self.src2 = carve["src1"].fill_(-1), carve["src2"].fill_(-1)
            self.n_post, self.pre_counts, self.err, self.out_q = carve["n_post"], carve["pre_counts"], carve["err"], carve["out_q"]
            # +1 row of padding keeps 16-byte row reads of the policy kernel inside the allocation
            self.obs1 = torch.zeros((R * cap + 1, _lib.OBS_DIM), dtype=torch.float32, device=self.device)
            # Agent.state lives in a ping-pong pair: a tick writes the new observations into the other buffer, so the
            # observations the policy read for that tick stay available for transition capture
            self._obs2 = [torch.zeros((R * cap + 1, _lib.OBS_DIM), dtype=torch.float32, device=self.device) for _ in range(2)]
            self._cur = 0
            self.age1 = torch.zeros((R, cap), dtype=torch.int32, device=self.device)
            self.brain1 = torch.zeros((R, cap), dtype=torch.int32, device=self.device)
            self.refill_count = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.acted_total = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.G = n_brains if static_families else 1
            self.trk_tick = torch.zeros((R, self.G, _lib.TRK_VARS), dtype=torch.float64, device=self.device)
            self.trk_sum = torch.zeros((R, self.G, _lib.TRK_VARS), dtype=torch.float64, device=self.device)
            self.trk_cnt = torch.zeros((R, self.G, _lib.TRK_VARS), dtype=torch.int32, device=self.device)
            self.trk_pop = torch.zeros((R, 3), dtype=torch.float64, device=self.device)
        self._state = _lib.State(*[_ptr(self.s[n]) for n in _lib.STATE_FIELDS])
        _lib.check(self.lib.rl_bind_state(self.handle, C.byref(self._state)), "rl_bind_state")
        _lib.check(self.lib.rl_bind_error_flag(self.handle, _ptr(self.err)), "rl_bind_error_flag")
        self.tracking = False
        self._trk_dirty = False     # a launch has added to trk_sum / trk_cnt / trk_pop since they were last zeroed
        self.replays = None
        self._build_step_out()
        self._work = None
        self._ticked = False
        self._brains = None
        self._tape_keep = None
        self._run_pair = None
        self._eps_keep = None
        self._capture_prob = False
        self._fused_key = self._fused = None
        self.launches = 0                        # kernel-launching C-ABI calls made by run() so far (bench.py reports it)
        self._side = None                        # side stream of readback()

    def __del__(self):
        try:
            if getattr(self, "handle", None) and self.handle.value:
                self.lib.rl_destroy(self.handle)
                self.handle = C.c_void_p()
        except Exception:  # noqa: BLE001
            pass

    # -- helpers ------------------------------------------------------------------------------------------------
    def _stream(self):
        # (the raw handle of torch's current stream on this device: ~0.3 us, where torch.cuda.current_stream() builds a Stream object
        # in ~5 us -- eight launches per tick of a host-driven loop)
        return C.c_void_p(_raw_stream(self._dev_index))

    def _cur_stream(self):
        """torch's current stream on this device as a Stream object (for Event.record), rebuilt only when the raw handle has changed."""
        raw = _raw_stream(self._dev_index)
        if getattr(self, "_cs_raw", None) != raw:
            self._cs_raw, self._cs = raw, torch.cuda.current_stream(self.device)
        return self._cs

    def obs_state(self):
        """[R, cap, 153] view of Agent.state (post-update observation)."""
        return self.obs2[: self.R * self.cap].view(self.R, self.cap, _lib.OBS_DIM)

    def obs_state_prime(self):
        """[R, cap, 153] view of Agent.state_prime (post-step observation)."""
        return self.obs1[: self.R * self.cap].view(self.R, self.cap, _lib.OBS_DIM)

    def check_error_flag(self):
        self.raise_on_error_flag(self.err.cpu().numpy())

    @staticmethod
    def raise_on_error_flag(e):
        if e[0] != 0:
            hint = (" -- rl_learn_prioritized_choice: the priorities of learner [world] give no distribution (all zero, a NaN or a negative "
                    "one), where np.random.choice raises ValueError") if int(e[0]) == _lib.ERR_NO_DISTRIBUTION else ""
            if int(e[0]) == _lib.ERR_TREE_REDRAW:
                hint = (" -- rl_learn_td_tree_sample: a draw of learner [world] ended on a leaf of the sum tree no row has reached (or the "
                        "tree's total is no positive finite number), where the reference's Memory.sample draws again: the run has left the "
                        "reference's draw order")
            if int(e[0]) == _lib.ERR_TREE_INDEX:
                hint = (" -- rl_learn_td_tree_update: entry [detail 0] of learner [world]'s batch names a leaf index ([detail 1]) outside the "
                        "tree's leaves, or a slot outside the ring: the entry was skipped")
            raise _lib.ReinLifeHipError("device error flag: code %d world %d detail (%d, %d)" % tuple(int(x) for x in e) + hint)

    def readback(self, tensors):
        """Small device tensors on their way to pinned host memory BEHIND everything queued on the current stream so far and NEXT TO
        whatever is queued afterwards: the copies run on a side stream that waits for an event recorded here, so a caller can queue
        the next multi-tick launch first and collect the values while it runs (`.wait()` -> list of numpy arrays).  The Tracker
        closes its intervals this way (Helpers/tracker.py): the device does not idle for the host's read-back, the statistics'
        arithmetic and the next launch's set-up."""
        cur = torch.cuda.current_stream(self.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.device)
        ready = torch.cuda.Event()
        ready.record(cur)
        self._side.wait_event(ready)
        host = []
        with torch.cuda.stream(self._side):
            for t in tensors:
                h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
                h.copy_(t, non_blocking=True)
                t.record_stream(self._side)
                host.append(h)
            done = torch.cuda.Event()
            done.record(self._side)
        return _Readback(host, done)

    SNAPSHOT_MAX_BYTES = 1 << 20

    def snapshot(self):
        """Host copy of the whole state arena (every rl_state array, actions, n_acted, reward, done, src1 / src2, step_split's counts, the
        error flag, the policy outputs) behind everything queued on the current stream: ONE device-to-host copy and ONE wait, whatever
        the number of arrays -> {name: numpy array}.  For hosts that look at their worlds every tick (a single world driven by the
        reference's generators); refused for big handles, whose callers read single worlds (world())."""
        nbytes = self._arena.numel()
        if nbytes > self.SNAPSHOT_MAX_BYTES:
            raise _lib.ReinLifeHipError("snapshot(): %d bytes of state; read single worlds of a handle this large with world()" % nbytes)
        if self._arena_host is None:
            self._arena_host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
            self._arena_np = self._arena_host.numpy()
            self._arena_done = torch.cuda.Event()
        self._arena_host.copy_(self._arena, non_blocking=True)
        self._arena_done.record(self._cur_stream())
        self._arena_done.synchronize()
        return _Snapshot(self._arena_np.copy(), self._layout)   # (a copy: the pinned buffer is reused by the next snapshot)

    # -- host <-> device state (parity I/O) ----------------------------------------------------------------------
    def load_world(self, w, snap):
        n = len(snap["i"])
        assert n <= self.cap
        dev = self.device
        self.s["cell_type"][w] = torch.as_tensor(np.asarray(snap["cell_type"], np.uint8), device=dev)
        self.s["n_agents"][w] = n
        for key in ("i", "j", "health", "age", "max_age", "gene", "brain", "uid", "flags", "action", "fitness"):
            t = self.s["a_" + key]
            t[w, :n] = torch.as_tensor(np.ascontiguousarray(snap[key]), device=dev).to(t.dtype)
        self.s["max_gene"][w] = int(snap.get("max_gene", self.n_brains))
        self.s["next_uid"][w] = int(snap.get("next_uid", (int(np.max(snap["uid"])) + 1) if n else 0))
        for key in ("best_uid", "best_fit", "best_brain"):
            if key in snap:
                self.s[key][w] = torch.as_tensor(np.asarray(snap[key]), device=dev).to(self.s[key].dtype)
        _lib.check(self.lib.rl_bind_state(self.handle, C.byref(self._state)), "rl_bind_state")  # state rewritten by the host

    def world(self, w):
        n = int(self.s["n_agents"][w].item())
        d = {k[2:]: self.s[k][w, :n].cpu().numpy() for k in self.s if k.startswith("a_")}
        d["cell_type"] = self.s["cell_type"][w].cpu().numpy()
        for key in ("max_gene", "next_uid", "tick", "epoch"):
            d[key] = int(self.s[key][w].item())
        for key in ("best_uid", "best_fit", "best_brain"):
            d[key] = self.s[key][w].cpu().numpy()
        return d

    def render(self, style, worlds=None, out=None):
        """Frames of `worlds` (a sequence of world ids in any order, repeats allowed, or a device int32 tensor of them; None = every
        world) painted on the device from the current state (rl_render): uint8 [n, height*gs, width*gs, 3] on this device.  `style` is
        Visualize.style(device) (Helpers/render.py).  `out`: a contiguous uint8 tensor of that shape to paint into (it is returned).
        Queued on torch's current stream behind everything queued so far; nothing is synchronised and the state is not touched."""
        if worlds is None:
            ids, n = None, self.R
        elif torch.is_tensor(worlds) and worlds.is_cuda:   # a caller's device list: its ids are checked by the kernel (error flag)
            ids = worlds.to(device=self.device, dtype=torch.int32).contiguous().view(-1)
            n = ids.numel()
        else:
            host = np.asarray(worlds.cpu() if torch.is_tensor(worlds) else worlds, dtype=np.int64).reshape(-1)
            if host.size and (host.min() < 0 or host.max() >= self.R):
                raise IndexError("render(): world ids must lie in [0, %d), got %s" % (self.R, host[(host < 0) | (host >= self.R)][:4].tolist()))
            key = host.tobytes()
            if getattr(self, "_render_ids_key", None) != key:   # (the id list of a loop that paints the same worlds every tick is uploaded once)
                self._render_ids_key, self._render_ids = key, torch.as_tensor(host.astype(np.int32), device=self.device)
            ids, n = self._render_ids, host.size
        if n < 1:
            raise ValueError("render(): no worlds to paint")
        gs = int(style.grid_size)
        shape = (n, self.H * gs, self.W * gs, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif (out.dtype != torch.uint8 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != self._arena.device):
            raise ValueError("render(): out must be a contiguous uint8 tensor of shape %s on %s" % (shape, self.device))
        _lib.check(self.lib.rl_render(self.handle, C.byref(style), _ptr(ids), n, _ptr(out), self._stream()), "rl_render")
        return out

    def make_tape(self, tapes):
        """tapes: one dict per world (food_k, food_u, repro_u, birth_k, produce_u, produce_choice) -> device Tape (TapeRing.make): a FRESH
        struct over its own device buffer per call, valid until the fourth make_tape() after it."""
        if getattr(self, "_tape_ring", None) is None:
            self._tape_ring = TapeRing(self.R, self.cap, self.device, self._cur_stream)
        return self._tape_ring.make(tapes)

    # -- the path -----------------------------------------------------------------------------------------------
    @property
    def obs2(self):
        return self._obs2[self._cur]

    def _build_step_out(self):
        t = (self.trk_tick, self.trk_sum, self.trk_cnt, self.trk_pop) if self.tracking else (None, None, None, None)
        c = (self.n_post, self.age1, self.brain1) if self.replays is not None else (None, None, None)
        self._step_out = _lib.StepOut(_ptr(self.n_acted), _ptr(self.reward), _ptr(self.done), _ptr(self.src1), _ptr(self.obs1),
                                      _ptr(self.acted_total), *[_ptr(x) for x in t], *[_ptr(x) for x in c])

    def _next_upd_out(self):
        """update_env writes Agent.state into the OTHER buffer of the ping-pong pair, which then becomes current."""
        self._cur ^= 1
        return _lib.UpdateOut(_ptr(self.src2), _ptr(self._obs2[self._cur]))

    def prev_state(self):
        """[R, cap, 153] observations the policy read for the last tick (valid between a tick/update and the next one)."""
        return self._obs2[self._cur ^ 1][: self.R * self.cap].view(self.R, self.cap, _lib.OBS_DIM)

    def enable_tracking(self, on=True):
        """Accumulate the Tracker statistics (Helpers/tracker.py) inside step()/tick() launches."""
        self.tracking = bool(on)
        self._build_step_out()

    def capture_floor(self):
        """The smallest replay ring transition capture accepts for this handle: n_worlds * slot_cap rows."""
        return self.R * self.cap

    def enable_capture(self, capacity, with_prob=False):
        """Allocate one replay ring per brain (rl_replay): filled by capture_transitions() after a stand-alone tick, or by run() inside
        the multi-tick launch (every tick of it).  capacity: one number for all rings, or one per brain -- each at least capture_floor(),
        n_worlds * slot_cap rows: what one tick of all worlds can append to one ring (rl_replay in include/reinlife_hip.h; a smaller ring
        would take two rows of one tick in one slot, and nothing orders their writes)."""
        caps = [int(capacity)] * self.n_brains if np.isscalar(capacity) else [int(c) for c in capacity]
        if len(caps) != self.n_brains or min(caps) < 1:
            raise ValueError("enable_capture(): capacity must be one positive number or one per brain (%d brains), got %r" % (self.n_brains, capacity))
        floor = self.capture_floor()
        for b, c in enumerate(caps):
            if c < floor:
                raise ValueError("enable_capture(): ring %d: capacity %d is below the floor of %d rows (n_worlds %d x slot_cap %d, the most rows one "
                                 "tick of all worlds can append to one ring)" % (b, c, floor, self.R, self.cap))
        self._capture_prob = bool(with_prob)
        self.replays = []
        arr = (_lib.Replay * self.n_brains)()
        for b, capacity in enumerate(caps):
            r = {"state": torch.zeros((capacity, _lib.OBS_DIM), dtype=torch.float32, device=self.device),
                 "state_prime": torch.zeros((capacity, _lib.OBS_DIM), dtype=torch.float32, device=self.device),
                 "action": torch.zeros(capacity, dtype=torch.int8, device=self.device),
                 "reward": torch.zeros(capacity, dtype=torch.float32, device=self.device),
                 "done": torch.zeros(capacity, dtype=torch.uint8, device=self.device),
                 "prob": torch.zeros(capacity, dtype=torch.float32, device=self.device) if with_prob else None,
                 "age": torch.zeros(capacity, dtype=torch.int32, device=self.device),
                 "count": torch.zeros(1, dtype=torch.int64, device=self.device)}
            self.replays.append(r)
            arr[b] = _lib.Replay(*[_ptr(r[n]) for n in ("state", "state_prime", "action", "reward", "done", "prob", "age", "count")], capacity)
        self._replay_arr = arr
        self._build_step_out()  # the step launches now also emit n_post / age / brain of the post-step list

    def capture_transitions(self, with_policy_out=False):
        """trainer.py:95-96 on the device: call after step()/tick() of a tick whose actions are still in self.actions."""
        if self.replays is None:
            raise _lib.ReinLifeHipError("enable_capture() was not called")
        _lib.check(self.lib.rl_capture_transitions(self.handle, _ptr(self._obs2[self._cur ^ 1] if self._ticked else self._obs2[self._cur]),
                                                   _ptr(self.actions), _ptr(self.out_q) if with_policy_out else None,
                                                   C.byref(self._step_out), self._replay_arr, self.n_brains, self._stream()),
                   "rl_capture_transitions")

    def draw_slots(self, learners, n_steps):
        """Ring slots for learn(learners, n_steps, slots=...) that do not depend on the ORDER of the rings' rows (rl_learn_draw): the
        multi-tick launch appends the worlds' transitions in the order their workgroups reach an atomic counter, so two identical
        runs hold the same transitions in other slots; these draws pick rows by a key of their content -- uniform, with replacement,
        the same rows in every run.  Device int32 [len(learners), n_steps, batch], queued on the current stream.
        rl_learn_draw's table is flat (draw d = s * batch + j) and its batch is at most 32, so for a larger batch (D3QN: 64, wide DQN: up to 2048) the same
        table is asked for as [n_steps * batch / b][b], b the largest divisor of batch that is <= 32 ([n_steps][64] = [2 n_steps][32])."""
        n = len(learners)
        if len({l.batch for l in learners}) != 1:
            raise ValueError("draw_slots(): the learners of a call must share one batch size")
        batch = int(learners[0].batch)
        # any batch works (rl_learn_wide: up to 2048): a prime one such as 37 draws as [37 n_steps][1] -- more steps of one draw, the same flat table
        draw_batch = max(b for b in range(1, min(batch, 32) + 1) if batch % b == 0)
        draw_steps = int(n_steps) * (batch // draw_batch)
        for l in learners:
            if getattr(l, "keys", None) is None or l.keys.numel() != l.ring["state"].shape[0]:
                l.keys = torch.zeros(l.ring["state"].shape[0], dtype=torch.int64, device=self.device)
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        for a in arr:
            a.batch = draw_batch
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        keys = (C.c_void_p * n)(*[l.keys.data_ptr() for l in learners])
        slots = torch.zeros((n, int(n_steps), batch), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.rl_learn_draw(self.handle, arr, rings, n, draw_steps, keys, _ptr(slots), self._stream()), "rl_learn_draw")
        self.launches += 2
        return slots

    def draw_slots_rank(self, learners, n_steps):
        """draw_slots() by another sampler (rl_learn_draw_rank, this build's own): every ring's rows are sorted by content key once and
        draw d takes the row at rank ((uint64)x * size) >> 32, x = word 0 of rl_philox(seed, 0, i, calls, RL_SITE_LEARN, d) -- uniform,
        with replacement, the same rows whatever slots they sit in, at a cost that does not depend on n_steps or the batch (draw_slots
        visits every key of a ring once per draw).  Other rows than draw_slots names.  Device int32 [len(learners), n_steps, batch]
        (batch 1 .. 2048, asked for as it is), queued on the current stream.  Keeps learner.keys, learner.rank_order (the slots in key
        order, [0, size) defined) and learner.rank_work (scratch) on the learners, allocated once per ring size."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("draw_slots_rank(): 1 to %d learners per call (got %d)" % (_lib.MAX_CAPTURE_BRAINS, n))
        if len({l.batch for l in learners}) != 1:
            raise ValueError("draw_slots_rank(): the learners of a call must share one batch size")
        for l in learners:
            capacity = int(l.ring["state"].shape[0])
            if getattr(l, "keys", None) is None or l.keys.numel() != capacity:
                l.keys = torch.zeros(capacity, dtype=torch.int64, device=self.device)
            if getattr(l, "rank_order", None) is None or l.rank_order.numel() != capacity:
                l.rank_order = torch.zeros(capacity, dtype=torch.int32, device=self.device)
                l.rank_work = torch.empty(int(self.lib.rl_learn_draw_rank_work_bytes(capacity)), dtype=torch.uint8, device=self.device)
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        keys = (C.c_void_p * n)(*[l.keys.data_ptr() for l in learners])
        order = (C.c_void_p * n)(*[l.rank_order.data_ptr() for l in learners])
        work = (C.c_void_p * n)(*[l.rank_work.data_ptr() for l in learners])
        slots = torch.zeros((n, int(n_steps), int(learners[0].batch)), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.rl_learn_draw_rank(self.handle, arr, rings, n, int(n_steps), keys, order, work, _ptr(slots), self._stream()),
                   "rl_learn_draw_rank")
        self.launches += _lib.LEARN_DRAW_RANK_LAUNCHES
        return slots

    def draw_prioritized(self, learners, n_steps):
        """The minibatches of prioritised learners (DeviceLearner(..., prioritized=True)) for learn(learners, n_steps, slots=...):
        PrioritizedReplayBuffer.sample's draw (PERD3QN.py:157-165) on the device (rl_learn_prioritized_draw) -- first every row appended
        since the last draw gets the priority maximum (store(), PERD3QN.py:147-153), then each draw takes a row with probability
        priority^alpha / sum, with replacement, by a key of the rows' content: the same rows whatever slots they sit in.  All n_steps
        are drawn from the priorities as they stand now.  Device int32 [len(learners), n_steps, batch], queued on the current stream.
        A list of wide prioritised learners (DeviceLearner(..., prioritized=True, prioritized_batch=B)) goes to
        rl_learn_prioritized_wide_draw: the same two launches and the same arithmetic for batches up to 2048 (B <= 64 with n_steps = 1:
        rl_learn_prioritized_draw's table).  The learners of a call are all of the one kind or all of the other."""
        return self._draw_side("draw_prioritized", learners, n_steps, _lib.Prio, "a prioritised one (DeviceLearner(..., prioritized=True))")

    def draw_rollout(self, learners, n_steps):
        """The rollouts of PPO learners (DeviceLearner(..., rollout=True)) for learn(learners, n_steps, slots=...): the on-policy draw
        (rl_learn_rollout) -- the window is the rows appended to a ring since the last call (the whole ring once that is more than it
        holds); each of the n_steps * batch draws takes a window row uniformly, with replacement, by a key of the rows' content: the same
        rows whatever slots they sit in.  Leaves the number of rows of the window in learner.fresh (an empty one: the following learn()
        makes no update) and moves learner.seen up.  Device int32 [len(learners), n_steps, batch], queued on the current stream.
        A list of wide PPO learners (DeviceLearner(..., rollout=True, rollout_batch=B)) goes to rl_learn_rollout_wide: the same two launches
        and the same arithmetic for rollouts of up to 2048 rows (B <= 32: rl_learn_rollout's table).  The learners of a call are all of the
        one kind or all of the other."""
        return self._draw_side("draw_rollout", learners, n_steps, _lib.Ppo, "a PPO one (DeviceLearner(..., rollout=True))")

    def draw_td(self, learners, n_steps):
        """The minibatches of PERDQN learners (DeviceLearner(..., td_priority=True)) for learn(learners, n_steps, slots=...): the draw of
        the reference's Memory on the device (rl_learn_td_draw) -- first every row appended since the last draw gets the one priority
        append_sample gives (learner.p_new), then each draw takes a row with probability priority / sum, with replacement, by a key of the
        rows' content: the same rows whatever slots they sit in (the reference's sample() is stratified through its sum tree; here the
        draws are independent).  Device int32 [len(learners), n_steps, batch], queued on the current stream.
        A list of wide PERDQN learners (DeviceLearner(..., td_priority=True, td_batch=B)) goes to rl_learn_td_wide_draw: the same two
        launches and the same arithmetic for batches up to 2048 (B <= 64: rl_learn_td_draw's table).  The learners of a call are all of
        the one kind or all of the other."""
        return self._draw_side("draw_td", learners, n_steps, _lib.TdPrio, "a PERDQN one (DeviceLearner(..., td_priority=True))")

    def draw_prioritized_rank(self, learners, n_steps, stratified=False):
        """draw_prioritized() by another sampler (rl_learn_prioritized_draw_rank, this build's own): the same stamp of the rows appended
        since the last draw, then every ring's rows sorted by content key once, their weights priority^alpha summed in that order in
        float64 (segments of 64, a fixed association order), and draw d the row at the smallest rank whose cumulative sum exceeds
        u_d * total -- probability weight / sum exactly, with replacement, the same rows whatever slots they sit in, at a cost that does
        not depend on n_steps or the batch (draw_prioritized makes a pass over the ring per draw).  stratified=True cuts the total into
        `batch` segments and takes draw j inside segment j.  Other rows than draw_prioritized names.  Narrow and wide prioritised
        learners alike (batch 1 .. 2048; one batch per call, the table being one tensor -- the C entry allows a batch per learner).
        Device int32 [len(learners), n_steps, batch], queued on the current stream.  Keeps
        learner.rank_order, learner.rank_cum (float64, [0, size) defined) and learner.rank_work on the learners, allocated once per ring size."""
        return self._draw_side_rank("draw_prioritized_rank", "rl_learn_prioritized_draw_rank", learners, n_steps, stratified, _lib.Prio,
                                    "a prioritised one (DeviceLearner(..., prioritized=True))")

    def draw_td_rank(self, learners, n_steps, stratified=True):
        """draw_td() by that sampler (rl_learn_td_draw_rank): fresh rows get learner.p_new, a row's weight is its stored priority.
        stratified=True (the default) is the reference's Memory.sample(): the total is cut into `batch` segments and draw j takes one
        uniform in segment j -- over the rows in content-key order, so the same rows whatever slots they sit in.  Device int32
        [len(learners), n_steps, batch], queued on the current stream.
        A list of wide PERDQN learners (DeviceLearner(..., td_priority=True, td_batch=B)) goes to rl_learn_td_wide_draw_rank (Entry.draw_rank):
        the same eight launches for batches up to 2048, stratified at B (B <= 64: rl_learn_td_draw_rank's table).  The learners of a call
        are all of the one kind or all of the other."""
        entries = {l.entry for l in learners}
        if len(entries) > 1:
            raise ValueError("draw_td_rank(): the learners of a call must be of one kind (one entry point), got %s" % sorted(entries))
        draw = (learners[0].spec.draw_rank if learners else None) or "rl_learn_td_draw_rank"
        return self._draw_side_rank("draw_td_rank", draw, learners, n_steps, stratified, _lib.TdPrio,
                                    "a PERDQN one (DeviceLearner(..., td_priority=True))")

    def stamp_td(self, learners):
        """This build's own, in front of draw_td() / draw_td_rank() (rl_learn_td_stamp, two launches): every row appended since the last
        draw gets the priority append_sample spells out and does not compute, (|Q(s)[a] - (r + (1 - done) gamma max_a Q_target(s'))| +
        e) ** a, from a forward pass of learner.target and learner.params as they stand now -- bit for bit what learn() would write for
        the row from the same parameters -- and learner.seen moves up to the ring's count, so the draw that follows stamps nothing.
        The learners may differ in batch (it is not read).  Returns nothing; queued on the current stream."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("stamp_td(): 1 to %d learners per call (got %d)" % (_lib.MAX_CAPTURE_BRAINS, n))
        if any(l.spec.side is not _lib.TdPrio for l in learners):
            raise ValueError("stamp_td(): every learner must be a PERDQN one (DeviceLearner(..., td_priority=True))")
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        sides = (_lib.TdPrio * n)(*[l.side_struct(_lib.TdPrio) for l in learners])
        _lib.check(self.lib.rl_learn_td_stamp(self.handle, arr, rings, sides, n, self._stream()), "rl_learn_td_stamp")
        self.launches += _lib.LEARN_TD_STAMP_LAUNCHES

    def _reference_prio_args(self, who, learners):
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("%s(): 1 to %d learners per call (got %d)" % (who, _lib.MAX_CAPTURE_BRAINS, n))
        if any(l.spec.side is not _lib.Prio for l in learners):
            raise ValueError("%s(): every learner must be a prioritised one (DeviceLearner(..., prioritized=True))" % who)
        return n, (_lib.Learner * n)(*[l.struct() for l in learners]), (_lib.Prio * n)(*[l.side_struct(_lib.Prio) for l in learners])

    def store_prioritized_reference(self, learners, capacities, first_rows, n_rows):
        """PrioritizedReplayBuffer.store's priority rule (PERD3QN.py:143-155) as learn="reference" uses it (rl_learn_prioritized_store_ref,
        one launch, queued on the current stream): for learner i the rows [first_rows[i], first_rows[i] + n_rows[i]) -- numbered from 0 in
        storage order, row a in slot a % ring rows of learner.priority -- get the maximum of the priorities of the capacities[i] rows in
        front of them (1.0 into an empty memory).  One maximum per group: the reference's result where no train() lies inside it.
        n_rows[i] at most ring rows - capacities[i]."""
        n, arr, sides = self._reference_prio_args("store_prioritized_reference", learners)
        groups = (_lib.PrioStore * n)(*[_lib.PrioStore(int(c), int(l.ring["state"].shape[0]), int(a), int(m))
                                        for l, c, a, m in zip(learners, capacities, first_rows, n_rows)])
        _lib.check(self.lib.rl_learn_prioritized_store_ref(self.handle, arr, sides, groups, n, self._stream()), "rl_learn_prioritized_store_ref")
        self.launches += 1

    def choose_prioritized_reference(self, learners, capacities, stored, uniforms, with_bracket=False):
        """PrioritizedReplayBuffer.sample's np.random.choice (PERD3QN.py:157-165) from uniforms the host has drawn
        (rl_learn_prioritized_choice, one launch, queued on the current stream): learner i's memory of capacities[i] rows, stored[i] rows
        stored so far, priorities in learner.priority by ring slot; uniforms[i] = np.random.random_sample(batch), all of one batch <= 64.
        Returns device tensors: indices int32 [n, batch] (the reference's memory indices), slots int32 [n, 1, batch] (what
        learn(learners, 1, slots=...) takes) and, with_bracket=True, each draw's cdf[idx - 1] and cdf[idx] as float64 [n, batch, 2] (else
        None).  Priorities np.random.choice would refuse (all zero, a NaN) set the error flag, code _lib.ERR_NO_DISTRIBUTION.  Keeps
        learner.choice_work (scratch) on the learners, allocated once per capacity."""
        n, arr, sides = self._reference_prio_args("choose_prioritized_reference", learners)
        u = np.ascontiguousarray(np.asarray(uniforms, np.float64).reshape(n, -1))
        batch = u.shape[1]
        if not 1 <= batch <= _lib.LEARN_CHOICE_MAX:
            raise ValueError("choose_prioritized_reference(): 1 to %d uniforms per learner (got %d)" % (_lib.LEARN_CHOICE_MAX, batch))
        for l, c in zip(learners, capacities):
            need = int(self.lib.rl_learn_prioritized_choice_work_bytes(int(c)))
            if need < 1:
                raise ValueError("choose_prioritized_reference(): capacity must be in [1, 2^31) (got %r)" % (c,))
            if getattr(l, "choice_work", None) is None or l.choice_work.numel() != need:
                l.choice_work = torch.empty(need, dtype=torch.uint8, device=self.device)
        u_dev = torch.as_tensor(u, device=self.device)
        indices = torch.zeros((n, batch), dtype=torch.int32, device=self.device)
        slots = torch.zeros((n, 1, batch), dtype=torch.int32, device=self.device)
        bracket = torch.zeros((n, batch, 2), dtype=torch.float64, device=self.device) if with_bracket else None
        draws = (_lib.PrioChoice * n)(*[_lib.PrioChoice(int(c), int(l.ring["state"].shape[0]), int(s), batch, _ptr(u_dev[i]), _ptr(indices[i]),
                                                        _ptr(slots[i]), _ptr(bracket[i]) if with_bracket else None, _ptr(l.choice_work))
                                        for i, (l, c, s) in enumerate(zip(learners, capacities, stored))])
        _lib.check(self.lib.rl_learn_prioritized_choice(self.handle, arr, sides, draws, n, self._stream()), "rl_learn_prioritized_choice")
        self._choice_keep = u_dev   # (the launch reads the uniforms asynchronously)
        self.launches += 1
        return indices, slots, bracket

    def _reference_tree_args(self, who, learners, capacities):
        """The common arguments of the three sum-tree calls; keeps learner.ref_tree, the reference's SumTree.tree as a zeroed device
        float64 [2 C - 1], on the learners, made at a learner's first call; another capacity later is refused."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("%s(): 1 to %d learners per call (got %d)" % (who, _lib.MAX_CAPTURE_BRAINS, n))
        if any(l.spec.side is not _lib.TdPrio for l in learners):
            raise ValueError("%s(): every learner must be a PERDQN one (DeviceLearner(..., td_priority=True))" % who)
        for l, c in zip(learners, capacities):
            if not 2 <= int(c) <= 2 ** 30:
                raise ValueError("%s(): capacity must be in [2, 2^30] (got %r): the reference's SumTree._propagate never ends for a tree of one leaf" % (who, c))
            if getattr(l, "ref_tree", None) is None:   # (once per learner, at its first call: no later call allocates)
                l.ref_tree = torch.zeros(2 * int(c) - 1, dtype=torch.float64, device=self.device)
            elif l.ref_tree.numel() != 2 * int(c) - 1:
                raise ValueError("%s(): this learner's tree was built for a capacity of %d, not %d: a memory keeps its capacity (a new tree "
                                 "would lose its priorities)" % (who, (l.ref_tree.numel() + 1) // 2, int(c)))
        return n, (_lib.Learner * n)(*[l.struct() for l in learners]), (_lib.TdPrio * n)(*[l.side_struct(_lib.TdPrio) for l in learners])

    def store_td_reference(self, learners, capacities, first_rows, n_rows):
        """Memory.add (PERDQN.py:276-278) as learn="reference" uses it (rl_learn_td_tree_store, one launch, queued on the current stream):
        for learner i the rows [first_rows[i], first_rows[i] + n_rows[i]) -- numbered from 0 in storage order, row a at memory index
        a % capacities[i] and in slot a % ring rows of learner.priority -- enter learner.ref_tree in row order with append_sample's
        constant priority, learner.p_new.  n_rows[i] at most ring rows - capacities[i]."""
        n, arr, sides = self._reference_tree_args("store_td_reference", learners, capacities)
        groups = (_lib.TdTreeStore * n)(*[_lib.TdTreeStore(_ptr(l.ref_tree), int(c), int(l.ring["state"].shape[0]), int(a), int(m))
                                          for l, c, a, m in zip(learners, capacities, first_rows, n_rows)])
        _lib.check(self.lib.rl_learn_td_tree_store(self.handle, arr, sides, groups, n, self._stream()), "rl_learn_td_tree_store")
        self.launches += 1

    def sample_td_reference(self, learners, capacities, stored, uniforms, with_points=False):
        """Memory.sample's stratified draw (PERDQN.py:280-298) from uniforms the host has drawn (rl_learn_td_tree_sample, one launch, queued
        on the current stream): learner i's tree of capacities[i] leaves with stored[i] rows stored so far; uniforms[i] =
        [random.random() for _ in range(batch)], all of one batch <= 64.  Returns device tensors: idxs int32 [n, batch] (the reference's
        TREE indices), slots int32 [n, 1, batch] (what learn(learners, 1, slots=...) takes) and, with_points=True, each draw's s and the
        leaf it found as float64 [n, batch, 2] (else None).  A draw that lands on a leaf no row has reached, where the reference draws
        again, sets the error flag, code _lib.ERR_TREE_REDRAW."""
        n, arr, sides = self._reference_tree_args("sample_td_reference", learners, capacities)
        u = np.ascontiguousarray(np.asarray(uniforms, np.float64).reshape(n, -1))
        batch = u.shape[1]
        if not 1 <= batch <= _lib.LEARN_TD_TREE_BATCH_MAX:
            raise ValueError("sample_td_reference(): 1 to %d uniforms per learner (got %d)" % (_lib.LEARN_TD_TREE_BATCH_MAX, batch))
        u_dev = torch.as_tensor(u, device=self.device)
        idxs = torch.zeros((n, batch), dtype=torch.int32, device=self.device)
        slots = torch.zeros((n, 1, batch), dtype=torch.int32, device=self.device)
        points = torch.zeros((2, n, batch), dtype=torch.float64, device=self.device) if with_points else None
        draws = (_lib.TdTreeSample * n)(*[_lib.TdTreeSample(_ptr(l.ref_tree), int(c), int(l.ring["state"].shape[0]), int(s), batch, _ptr(u_dev[i]),
                                                            _ptr(idxs[i]), _ptr(slots[i]), _ptr(points[0, i]) if with_points else None,
                                                            _ptr(points[1, i]) if with_points else None)
                                          for i, (l, c, s) in enumerate(zip(learners, capacities, stored))])
        _lib.check(self.lib.rl_learn_td_tree_sample(self.handle, arr, sides, draws, n, self._stream()), "rl_learn_td_tree_sample")
        self._choice_keep = u_dev   # (the launch reads the uniforms asynchronously)
        self.launches += 1
        return idxs, slots, points.permute(1, 2, 0) if with_points else None

    def update_td_reference(self, learners, capacities, idxs, slots):
        """train_model's priority loop (PERDQN.py:175-177) behind learn() (rl_learn_td_tree_update, one launch, queued on the current
        stream): for learner i, in order, the leaf idxs[i][j] of learner.ref_tree gets the priority rl_learn_td has just written to
        learner.priority[slots[i][j]].  idxs and slots: the device tensors sample_td_reference() returned."""
        n, arr, sides = self._reference_tree_args("update_td_reference", learners, capacities)
        idxs, slots = idxs.reshape(n, -1), slots.reshape(n, -1)
        if idxs.dtype != torch.int32 or slots.dtype != torch.int32 or idxs.shape != slots.shape or not idxs.is_contiguous() or not slots.is_contiguous():
            raise ValueError("update_td_reference(): idxs and slots must be contiguous int32 device tensors of one shape")
        batches = (_lib.TdTreeUpdate * n)(*[_lib.TdTreeUpdate(_ptr(l.ref_tree), int(c), int(l.ring["state"].shape[0]), int(idxs.shape[1]),
                                                              _ptr(idxs[i]), _ptr(slots[i])) for i, (l, c) in enumerate(zip(learners, capacities))])
        _lib.check(self.lib.rl_learn_td_tree_update(self.handle, arr, sides, batches, n, self._stream()), "rl_learn_td_tree_update")
        self._tree_keep = (idxs, slots)   # (the launch reads them asynchronously)
        self.launches += 1

    def _draw_side_rank(self, who, draw, learners, n_steps, stratified, side, one_of):
        """draw_prioritized_rank / draw_td_rank: the C entry `draw`, fed the learners' side structs and their order / cum / work buffers.
        The learners of a call must share one batch -- deliberately, as for every draw_* here: the table comes back as ONE tensor
        [n, n_steps, batch], which DeviceWorlds.learn takes as it is (Environment.learn_now makes one call per batch size).  The C entry
        itself lays the learners' tables end to end and allows a batch per learner."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("%s(): 1 to %d learners per call (got %d)" % (who, _lib.MAX_CAPTURE_BRAINS, n))
        if len({l.batch for l in learners}) != 1:
            raise ValueError("%s(): the learners of a call must share one batch size" % who)
        if any(l.spec.side is not side for l in learners):
            raise ValueError("%s(): every learner must be %s" % (who, one_of))
        for l in learners:
            capacity = int(l.ring["state"].shape[0])
            if getattr(l, "rank_cum", None) is None or l.rank_cum.numel() != capacity:
                l.rank_order = torch.zeros(capacity, dtype=torch.int32, device=self.device)
                l.rank_cum = torch.zeros(capacity, dtype=torch.float64, device=self.device)
                l.rank_work = torch.empty(int(self.lib.rl_learn_prio_draw_rank_work_bytes(capacity)), dtype=torch.uint8, device=self.device)
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        sides = (side * n)(*[l.side_struct(side) for l in learners])
        order = (C.c_void_p * n)(*[l.rank_order.data_ptr() for l in learners])
        cum = (C.c_void_p * n)(*[l.rank_cum.data_ptr() for l in learners])
        work = (C.c_void_p * n)(*[l.rank_work.data_ptr() for l in learners])
        slots = torch.zeros((n, int(n_steps), int(learners[0].batch)), dtype=torch.int32, device=self.device)
        _lib.check(getattr(self.lib, draw)(self.handle, arr, rings, sides, n, int(n_steps), int(bool(stratified)), order, cum, work, _ptr(slots),
                                           self._stream()), draw)
        self.launches += _lib.LEARN_PRIO_DRAW_RANK_LAUNCHES
        return slots

    def _draw_side(self, who, learners, n_steps, side, one_of):
        """draw_prioritized / draw_rollout / draw_td: the draw entry of the learners' own (Entry.draw), fed their side structs of type `side`."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("%s(): 1 to %d learners per call (got %d)" % (who, _lib.MAX_CAPTURE_BRAINS, n))
        if len({l.batch for l in learners}) != 1:
            raise ValueError("%s(): the learners of a call must share one batch size" % who)
        if any(l.spec.side is not side for l in learners):
            raise ValueError("%s(): every learner must be %s" % (who, one_of))
        entries = {l.entry for l in learners}
        if len(entries) != 1:
            raise ValueError("%s(): the learners of a call must be of one kind (one entry point), got %s" % (who, sorted(entries)))
        draw = learners[0].spec.draw
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        sides = (side * n)(*[l.side_struct(side) for l in learners])
        slots = torch.zeros((n, int(n_steps), int(learners[0].batch)), dtype=torch.int32, device=self.device)
        _lib.check(getattr(self.lib, draw)(self.handle, arr, rings, sides, n, int(n_steps), _ptr(slots), self._stream()), draw)
        self.launches += 2
        return slots

    def learn(self, learners, n_steps, slots=None, gate=True):
        """DQNAgent.train() (DQN.py:80-83, 142-153) for every DeviceLearner of `learners` in ONE launch (rl_learn), queued on the current
        stream behind the ticks launched so far: `n_steps` minibatch updates per brain on its replay ring (learner.ring), then the
        target copy, and the learner's packed weights rewritten in place -- brains bound with that tensor act on the new weights
        from the next launch on.  slots: optional int32 [len(learners), n_steps, batch] ring slots (host array or device tensor);
        None = drawn on the device, uniformly WITH replacement (learn.philox_slots gives the same numbers on the host; the
        brain index of the draw is the learner's position in `learners`).
        A list of D3QN learners goes to rl_learn_dueling instead (D3QNAgent.train(), D3QN.py:97-116: batch up to 64, MSE, the target copy
        only when learner.sync_target says so), a list of prioritised PERD3QN learners to rl_learn_prioritized (PERD3QNAgent.train(),
        PERD3QN.py:94-115: the same update, and the batch rows' priorities rewritten; `slots` must come from draw_prioritized()), a list of
        PPO learners to rl_learn_ppo (PPO.learn(), PPO.py:136-162: n_steps rollouts of `batch` rows, k_epoch Adam steps each; `slots` from
        draw_rollout(), or the caller's own rows with gate=False, which leaves the empty-window gate out), a list of PERDQN learners to
        rl_learn_td (PERDQNAgent.train_model(): the loss scaled by the mean importance weight, the batch rows' priorities rewritten;
        `slots` from draw_td()), a list of wide DQN learners (DeviceLearner(..., wide_batch=B)) to rl_learn_wide (the DQN update on
        minibatches of B <= 2048 rows, 32-row tiles side by side, 2 n_steps + 3 launches; `slots` from draw_slots() or None), a list of
        wide D3QN learners (DeviceLearner(..., dueling_batch=B)) to rl_learn_dueling_wide (the D3QN update on minibatches of B <= 2048
        rows, 64-row tiles side by side with the advantage mean of the whole batch, 3 n_steps + 3 launches; one batch per call; `slots`
        from draw_slots() / draw_slots_rank() or None), a list of wide prioritised PERD3QN learners (DeviceLearner(..., prioritized=True,
        prioritized_batch=B)) to rl_learn_prioritized_wide (that tiled update plus the priorities of all B rows and their maximum, 3 n_steps
        + 3 launches; one batch per call; `slots` must come from draw_prioritized()), a list of wide PPO learners (DeviceLearner(...,
        rollout=True, rollout_batch=B)) to rl_learn_ppo_wide (PPO.learn() on rollouts of B <= 2048 rows, 32-row tiles side by side with one
        GAE recursion over the whole rollout, 3 n_steps k_epoch + 3 launches with the largest k_epoch of the call; one batch per call;
        `slots` from draw_rollout(), or the caller's own rows with gate=False), a list of wide PERDQN learners (DeviceLearner(...,
        td_priority=True, td_batch=B)) to rl_learn_td_wide (train_model() on minibatches of B <= 2048 rows, 64-row tiles side by side, the
        importance weights' minimum and mean over the whole batch from a pass in front of every step's tiles, 3 n_steps + 3 launches; one
        batch per call; `slots` must come from draw_td() / draw_td_rank()).  The
        learners of one call must all belong to one entry point: ValueError otherwise."""
        if not learners:
            return
        n = len(learners)
        entries = {l.entry for l in learners}
        if len(entries) != 1:
            raise ValueError("learn(): the learners of a call must be of one kind (one entry point), got %s" % sorted(entries))
        spec = learners[0].spec   # (the row of learn.ALL_ENTRIES: every C signature is handle, learners, rings, [side structs], n, n_steps, slots, [work], stream)
        if n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("learn(): at most %d learners per call (got %d)" % (_lib.MAX_CAPTURE_BRAINS, n))
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        rings = (_lib.Replay * n)(*[l.ring_struct() for l in learners])
        if slots is not None:
            if not (torch.is_tensor(slots) and slots.is_cuda):
                slots = torch.as_tensor(np.array(slots.cpu().numpy() if torch.is_tensor(slots) else slots, dtype=np.int32), device=self.device)
            slots = slots.to(device=self.device, dtype=torch.int32).contiguous()
            if slots.numel() != n * n_steps * learners[0].batch or len({l.batch for l in learners}) != 1:
                raise ValueError("learn(): slots must hold [n_learners, n_steps, batch] = [%d, %d, %d] entries" % (n, n_steps, learners[0].batch))
        if spec.one_batch and len({l.batch for l in learners}) != 1:
            raise ValueError("learn(): the %s learners of a call must share one batch size, got %s" % (spec.name, sorted({l.batch for l in learners})))
        sides = [(spec.side * n)(*[l.side_struct(spec.side, gate=gate) for l in learners])] if spec.side else []
        work = [(C.c_void_p * n)(*[l.work.data_ptr() for l in learners])] if spec.narrow else []
        _lib.check(getattr(self.lib, spec.name)(self.handle, arr, rings, *sides, n, int(n_steps), _ptr(slots), *work, self._stream()), spec.name)
        self._learn_keep = slots   # (the launch reads the table asynchronously)
        self.launches += spec.launches(int(n_steps), max(l.k_epoch for l in learners)) if spec.per_epoch else spec.launches(int(n_steps))

    def export_learners(self, learners, out=None):
        """The learners' state as ONE flat float32 row on the device (rl_learn_export, one launch, queued on the current stream): learner i's
        segment -- params | adam_m | adam_v | its Adam step count as two 32-bit words -- starts where learner i - 1's ends
        (DeviceLearner.merge_floats each).  What the ranks of a job all-gather before merge_learners().  out: a row to fill."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("export_learners(): 1 to %d learners per call (got %d)" % (_lib.MAX_CAPTURE_BRAINS, n))
        total = sum(l.merge_floats for l in learners)
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=self.device)
        elif out.numel() < total or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
            raise ValueError("export_learners(): out must be a contiguous float32 device tensor of at least %d elements" % total)
        arr = (_lib.Learner * n)(*[l.struct() for l in learners])
        _lib.check(self.lib.rl_learn_export(self.handle, arr, n, _ptr(out), self._stream()), "rl_learn_export")
        self.launches += 1
        return out

    def merge_learners(self, learners, rows, n_ranks, sync_target=None):
        """The end of a learning episode on several ranks (rl_learn_merge, two launches, queued on the current stream): `rows` is the
        all-gather of the ranks' exported rows, a float32 device tensor [n_ranks, floats] (a flat row when n_ranks == 1).  Per learner the
        ranks with the highest Adam step count take part; params, adam_m and adam_v become their mean (summed in rank order in double,
        rounded once: the same bits on every rank), the step count the maximum, target the merged params where the learner's sync_target
        is set (sync_target: a list of flags for THIS call instead), and packed is rewritten from the merged params like the host packer
        does.  This build's own: periodic parameter averaging, not gradient averaging; the reference has no multi-process training."""
        n = len(learners)
        if n < 1 or n > _lib.MAX_CAPTURE_BRAINS:
            raise ValueError("merge_learners(): 1 to %d learners per call (got %d)" % (_lib.MAX_CAPTURE_BRAINS, n))
        n_ranks = int(n_ranks)
        if n_ranks < 1 or n_ranks > _lib.MAX_MERGE_RANKS:
            raise ValueError("merge_learners(): 1 to %d ranks (got %d)" % (_lib.MAX_MERGE_RANKS, n_ranks))
        if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous()):
            raise ValueError("merge_learners(): rows must be a contiguous float32 device tensor")
        if rows.numel() % n_ranks:
            raise ValueError("merge_learners(): rows holds %d floats, no multiple of n_ranks %d" % (rows.numel(), n_ranks))
        flags = [None] * n if sync_target is None else list(sync_target)
        arr = (_lib.Learner * n)(*[l.struct(sync_target=f) for l, f in zip(learners, flags)])
        _lib.check(self.lib.rl_learn_merge(self.handle, arr, n, _ptr(rows), n_ranks, rows.numel() // n_ranks, self._stream()), "rl_learn_merge")
        self._merge_keep = rows   # (the launches read the table asynchronously)
        self.launches += 2

    def pack_device(self, kind, params, packed):
        """rl_policy_pack_weights on the device (rl_policy_pack_device, one launch on the current stream): `params` (device float32, state-dict
        order) -> `packed` (device float32 [rl_policy_packed_floats(kind)]), the host packer's bits."""
        if params.numel() != self.lib.rl_policy_n_params(kind) or packed.numel() != self.lib.rl_policy_packed_floats(kind):
            raise ValueError("pack_device(): brain kind %d takes %d parameters and %d packed floats (got %d, %d)"
                             % (kind, self.lib.rl_policy_n_params(kind), self.lib.rl_policy_packed_floats(kind), params.numel(), packed.numel()))
        if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (params, packed)):
            raise ValueError("pack_device(): params and packed must be contiguous float32 device tensors")
        _lib.check(self.lib.rl_policy_pack_device(int(kind), _ptr(params), _ptr(packed), self._stream()), "rl_policy_pack_device")
        self.launches += 1

    def reset_tracking(self):
        if self._trk_dirty:   # (fresh accumulators are zero: a new Environment's first launch is not preceded by three memsets)
            self.trk_sum.zero_(); self.trk_cnt.zero_(); self.trk_pop[:, 1:].zero_()
            self._trk_dirty = False

    def set_actions(self, actions):
        if torch.is_tensor(actions):
            a = actions.to(device=self.device, dtype=torch.int8)
            assert tuple(a.shape) == (self.R, self.cap)
            self.actions.copy_(a)
            return
        # a host array: through a pinned staging buffer (two, alternating; each reused only once its last upload has executed)
        if getattr(self, "_act_ring", None) is None:
            self._act_ring = [[torch.zeros((self.R, self.cap), dtype=torch.int8).pin_memory(), None] for _ in range(2)]
            self._act_next = 0
        slot = self._act_ring[self._act_next & 1]
        self._act_next += 1
        if slot[1] is not None:
            slot[1].synchronize()
        a = np.asarray(actions)
        assert a.shape == (self.R, self.cap)
        slot[0].numpy()[...] = a      # (casts to int8 like the former as_tensor(...).to(int8))
        self.actions.copy_(slot[0], non_blocking=True)
        if slot[1] is None:
            slot[1] = torch.cuda.Event()
        slot[1].record(self._cur_stream())

    def step(self, actions=None, tape=None):
        if actions is not None:
            self.set_actions(actions)
        self._trk_dirty = self._trk_dirty or self.tracking
        _lib.check(self.lib.rl_step(self.handle, _ptr(self.actions), C.byref(tape) if tape is not None else None,
                                    C.byref(self._step_out), self._stream()), "rl_step")
        self._ticked = False  # Agent.state of this tick is still the current buffer

    def step_split(self, actions=None):
        """First half of a split step; returns the device tensor [R,4] (food, poison, super food, empty cells after movement)."""
        if actions is not None:
            self.set_actions(actions)
        self._trk_dirty = self._trk_dirty or self.tracking
        _lib.check(self.lib.rl_step_split(self.handle, _ptr(self.actions), C.byref(self._step_out), _ptr(self.pre_counts),
                                          self._stream()), "rl_step_split")
        self._ticked = False
        return self.pre_counts

    def step_food(self, tape):
        _lib.check(self.lib.rl_step_food(self.handle, C.byref(tape), _ptr(self.obs1), self._stream()), "rl_step_food")

    def update(self, tape=None):
        uo = self._next_upd_out()
        _lib.check(self.lib.rl_update(self.handle, C.byref(tape) if tape is not None else None, C.byref(uo), self._stream()),
                   "rl_update")
        self._ticked = True

    def tick(self, actions=None, tape=None):
        """step() + update_env() of one trainer-loop iteration in ONE kernel launch."""
        if actions is not None:
            self.set_actions(actions)
        uo = self._next_upd_out()
        self._trk_dirty = self._trk_dirty or self.tracking
        _lib.check(self.lib.rl_tick(self.handle, _ptr(self.actions), C.byref(tape) if tape is not None else None,
                                    C.byref(self._step_out), C.byref(uo), self._stream()), "rl_tick")
        self._ticked = True

    def tick_refill(self, threshold, n_agents):
        """tick() + refill(threshold, n_agents) in one launch (Philox draws)."""
        uo = self._next_upd_out()
        self._trk_dirty = self._trk_dirty or self.tracking
        _lib.check(self.lib.rl_tick_refill(self.handle, _ptr(self.actions), C.byref(self._step_out), C.byref(uo),
                                           threshold, n_agents, _ptr(self.refill_count), self._stream()), "rl_tick_refill")
        self._ticked = True

    def run_supported(self):
        return self._brains is not None and bool(self.lib.rl_run_supported(self.handle, self._brains, self.n_brains))

    def run(self, n_ticks, threshold=-1, n_agents=0, eps_schedule=None, trk_skip=0, want_q=False):
        """n_ticks x (act() + tick_refill(threshold, n_agents)) -- or + tick() when threshold < 0 -- in ONE launch when the
        configuration allows it (rl_run_ex: every world stays in LDS between ticks; the Tracker accumulators are maintained in
        the launch when tracking is on), else the same loop over the two launches.  Either way the buffers afterwards hold the
        last tick's outputs.
        eps_schedule: optional [n_ticks, n_brains] float32 (host array or device tensor) -- the brains' exploration rate in every
        tick (the reference's brains decay epsilon per episode); None = the rates given to set_brains().
        trk_skip: the Tracker's running sums leave out the first trk_skip ticks (episode 0, tracker.py:279-282).
        want_q: the policy's outputs of the LAST tick (Q values / PPO probabilities) are left in self.out_q (rl_run_opts.policy_out)."""
        if self._brains is None:
            raise _lib.ReinLifeHipError("set_brains() was not called")
        if n_ticks <= 0:
            return
        eps_host = None
        if eps_schedule is not None:
            if not torch.is_tensor(eps_schedule) or not eps_schedule.is_cuda:
                eps_host = np.ascontiguousarray(eps_schedule.cpu().numpy() if torch.is_tensor(eps_schedule) else eps_schedule, dtype=np.float32)
                assert eps_host.shape == (n_ticks, self.n_brains)
            else:
                eps_schedule = eps_schedule.to(torch.float32).contiguous()
                assert tuple(eps_schedule.shape) == (n_ticks, self.n_brains)
        # (with many worlds per GPU -- several per CU -- the two stand-alone launches are faster: 8.0e8 against 6.1e8 agent-steps/s
        # at 1024 worlds, the cross-world policy tiles waste fewer rows; the run_always option forces the single launch)
        # (what the decision depends on: the brains' kinds -- set_brains() drops the cached answer -- and the handle's option snapshot)
        if self._fused_key is None:
            self._fused_key = True
            self._fused = self.run_supported() and (self.R <= 768 or self.lib.rl_get_option(self.handle, b"run_always") == 1)
        fused = self._fused
        if not fused:
            if eps_schedule is not None and eps_host is None:
                eps_host = eps_schedule.cpu().numpy()   # ONE read-back, not one per tick
            keep = None
            if self.tracking and trk_skip > 0:   # like the kernel: the first trk_skip ticks stay out of the running sums, earlier sums stay
                keep = (self.trk_sum.clone(), self.trk_cnt.clone(), self.trk_pop[:, 1:].clone())
            for t in range(n_ticks):
                if eps_host is not None:
                    self._set_epsilons(eps_host[t].tolist())
                self.act(want_q=want_q or (self.replays is not None and self._capture_prob))
                if threshold >= 0:
                    self.tick_refill(threshold, n_agents)
                else:
                    self.tick()
                self.launches += 2
                if self.replays is not None:
                    self.capture_transitions(with_policy_out=self._capture_prob)
                if keep is not None and t + 1 == trk_skip:
                    self.trk_sum.copy_(keep[0]); self.trk_cnt.copy_(keep[1]); self.trk_pop[:, 1:].copy_(keep[2])
            return
        inline = eps_host is not None and eps_host.size <= _lib.EPS_INLINE_MAX
        if eps_host is not None and not inline:
            eps_schedule = self._stage_schedule(eps_host)
        if self._run_pair is None:
            self._run_pair = (C.c_void_p * 2)(_ptr(self._obs2[0]), _ptr(self._obs2[1]))
        cap = self.replays is not None
        # (a short schedule rides in the kernel arguments -- rl_run_opts.eps_schedule_on_host: the launch waits for no upload)
        eps_arg = C.c_void_p(eps_host.ctypes.data) if inline else _ptr(eps_schedule)
        opts = _lib.RunOpts(threshold, n_agents, _ptr(self.refill_count), eps_arg, trk_skip, 1 if inline else 0,
                            C.cast(self._replay_arr, C.c_void_p) if cap else None, _ptr(self.out_q) if (want_q or (cap and self._capture_prob)) else None)
        self._trk_dirty = self._trk_dirty or self.tracking
        _lib.check(self.lib.rl_run_ex(self.handle, self._brains, self.n_brains, n_ticks, _ptr(self.actions), C.byref(self._step_out),
                                      self._run_pair, self._cur, _ptr(self.src2), C.byref(opts), self._stream()), "rl_run_ex")
        self._eps_keep = None if inline else eps_schedule   # the launch reads a device table asynchronously
        self.launches += 1
        self._cur = (self._cur + n_ticks) & 1
        self._ticked = True

    def _stage_schedule(self, host):
        """A host [n_ticks, n_brains] float32 schedule -> device through the process-wide ring of pinned buffers (_EPS_RING).  A slot's
        host buffer is rewritten only once its previous upload has executed (its event); its device buffer is rewritten by a copy
        queued on this stream, i.e. behind the launch that read it when that launch was on this stream -- and eight further uploads
        lie between two uses of a slot."""
        n = host.size
        ring = _EPS_RING.setdefault(str(self.device), {"slots": [], "next": 0})
        if len(ring["slots"]) < 8:
            cap = max(8192, 1 << int(n - 1).bit_length())
            slot = [torch.empty(cap, dtype=torch.float32).pin_memory(), torch.empty(cap, dtype=torch.float32, device=self.device),
                    torch.cuda.Event()]
            ring["slots"].append(slot)
        else:
            slot = ring["slots"][ring["next"] % 8]
            ring["next"] += 1
            slot[2].synchronize()
            if slot[0].numel() < n:
                cap = 1 << int(n - 1).bit_length()
                slot[0], slot[1] = torch.empty(cap, dtype=torch.float32).pin_memory(), torch.empty(cap, dtype=torch.float32, device=self.device)
        slot[0][:n].copy_(torch.from_numpy(host.reshape(-1)))
        dev = slot[1][:n]
        dev.copy_(slot[0][:n], non_blocking=True)
        slot[2].record(torch.cuda.current_stream(self.device))
        return dev.view(host.shape)

    def _set_epsilons(self, eps):
        for b, e in enumerate(eps):
            self._brains[b].epsilon = float(e)

    def observe(self):
        _lib.check(self.lib.rl_observe(self.handle, _ptr(self.obs2), self._stream()), "rl_observe")
        return self.obs_state()

    def reset_synthetic(self, n_agents):
        _lib.check(self.lib.rl_reset_synthetic(self.handle, n_agents, _ptr(self.obs2), self._stream()),
                   "rl_reset_synthetic")

    def reset_families(self):
        """Environment.reset() for every world on the device: one agent per brain (gene = its index) at random cells."""
        _lib.check(self.lib.rl_reset_families(self.handle, _ptr(self.obs2), self._stream()), "rl_reset_families")

    def refill(self, threshold, n_agents):
        _lib.check(self.lib.rl_refill(self.handle, threshold, n_agents, _ptr(self.obs2), _ptr(self.refill_count),
                                      self._stream()), "rl_refill")

    # -- policy -------------------------------------------------------------------------------------------------
    def set_brains(self, brains):
        """brains: list of (kind:int, epsilon:float, packed: device float32 tensor)."""
        assert len(brains) == self.n_brains
        self._brain_keep = [b[2] for b in brains]
        arr = (_lib.Brain * len(brains))()
        for k, (kind, eps, packed) in enumerate(brains):
            assert packed.is_cuda and packed.dtype == torch.float32 and packed.is_contiguous()
            assert packed.numel() == self.lib.rl_policy_packed_floats(kind)
            arr[k] = _lib.Brain(kind, float(eps), packed.data_ptr())
        self._brains = arr
        self._fused_key = None   # (the fused / two-launch decision depends on the brains' kinds)
        if self._work is None:
            nbytes = self.lib.rl_policy_work_bytes(self.handle)
            self._work = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.rl_bind_policy_work(self.handle, _ptr(self._work)), "rl_bind_policy_work")

    def act(self, want_q=False):
        """Agent.get_action for every agent of every world: obs_state -> self.actions (and self.out_q)."""
        if self._brains is None:
            raise _lib.ReinLifeHipError("set_brains() was not called")
        _lib.check(self.lib.rl_policy_act(self.handle, self._brains, self.n_brains, _ptr(self.obs2), _ptr(self.actions),
                                          _ptr(self.out_q) if want_q else None, _ptr(self._work), self._stream()),
                   "rl_policy_act")


def pack_brain_weights(kind, state_dict_flat, device="cuda:0"):
    """state-dict-order float32 vector (host) -> packed MFMA layout on the device."""
    lib = _lib.lib()
    flat = np.ascontiguousarray(state_dict_flat, dtype=np.float32)
    if flat.size != lib.rl_policy_n_params(kind):
        raise ValueError("brain kind %d expects %d parameters, got %d" % (kind, lib.rl_policy_n_params(kind), flat.size))
    packed = np.zeros(lib.rl_policy_packed_floats(kind), np.float32)
    _lib.check(lib.rl_policy_pack_weights(kind, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)),
               "rl_policy_pack_weights")
    return torch.as_tensor(packed, device=device)


def policy_forward(kind, packed, obs, out=None):
    """Dense batch: obs [n,153] device float32 (allocation must extend >= 12 bytes past the last row, or n rows of a
    larger buffer) -> [n,8]."""
    lib = _lib.lib()
    n = obs.shape[0]
    if out is None:
        out = torch.empty((n, 8), dtype=torch.float32, device=obs.device)
    stream = C.c_void_p(torch.cuda.current_stream(obs.device).cuda_stream)
    _lib.check(lib.rl_policy_forward(kind, _ptr(packed), _ptr(obs), n, _ptr(out), stream), "rl_policy_forward")
    return out
