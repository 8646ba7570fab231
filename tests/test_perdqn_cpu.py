"""CPU: the PERDQN brain (ReinLife/Models/PERDQN.py) -- its C ABI kind, packed layout and rl_run answer, and the Python class against
fixtures of the real reference (tests/golden/perdqn.npz, tools/gen_golden_perdqn.py): seeded initial weights, `load_model=`, the
np.random / random draw order of get_action, and the Saver's attribute name.  No compute call is made (no GPU here)."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from reinlife_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "perdqn.npz")
KEYS = [("fc.0.weight", [64, 153]), ("fc.0.bias", [64]), ("fc.2.weight", [64, 64]), ("fc.2.bias", [64]), ("fc.4.weight", [8, 64]),
        ("fc.4.bias", [8])]


def _fix():
    d = np.load(FIX)
    return d, json.loads(bytes(d["meta"]).decode())


def _flat(net):
    return np.concatenate([v.detach().numpy().astype(np.float32).reshape(-1) for v in net.state_dict().values()])


def _sd_of(flat):
    sd, off = {}, 0
    for k, shape in KEYS:
        n = int(np.prod(shape))
        sd[k] = torch.from_numpy(flat[off:off + n].reshape(shape).copy())
        off += n
    assert off == len(flat)
    return sd


def test_the_reference_readme_import_line_works():
    """README.md:100-107 / test.py:2 of the reference."""
    from reinlife_amd.Models import DQN, D3QN, PERD3QN, PPO, PERDQN  # noqa: F401
    from reinlife_amd import Models
    assert "PERDQN" in Models.__all__ and PERDQN().method == "PERDQN"


def test_abi_kind_params_and_packed_layout():
    lib = _lib.lib()
    assert _lib.PERDQN == 4 and _lib.KIND_BY_METHOD["PERDQN"] == 4
    hdr = open(os.path.join(ROOT, "include", "reinlife_hip.h")).read()
    assert "RL_PPO = 3, RL_PERDQN = 4" in hdr
    assert lib.rl_policy_n_params(4) == 14536 == sum(int(np.prod(s)) for _, s in KEYS)

    def frag(chunks, tout):
        return chunks * tout * 2 * 64 * 4
    in_layer, hid, head = frag(10, 2) + 2 * 64, frag(4, 2) + 2 * 64, frag(4, 1) + 16   # in_layer_floats(2), hid_layer_floats(2, 2), head_floats(2, 8)
    assert lib.rl_policy_packed_floats(4) == in_layer + hid + head == 16656
    assert lib.rl_policy_n_params(5) < 0 and lib.rl_policy_packed_floats(5) < 0


def test_weight_packing_keeps_every_perdqn_weight_to_22_bits():
    """rl_policy_pack_weights(PERDQN): three MFMA layers in the layout of every kind (f16 hi / lo planes of the weight scaled by a power of
    two per output feature, fragment order, then unscale / bias in accumulator order): every parameter is recovered to 22 bits of its row,
    and both planes are rounded to the nearest f16 (not toward zero, as for the four kinds of the multi-tick kernel)."""
    lib = _lib.lib()
    n = lib.rl_policy_n_params(4)
    rng = np.random.RandomState(5)
    flat = (rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n) * 2.0 ** rng.randint(-6, 3, size=n)).astype(np.float32)
    packed = np.zeros(lib.rl_policy_packed_floats(4), np.float32)
    assert lib.rl_policy_pack_weights(4, flat.ctypes.data_as(C.c_void_p), packed.ctypes.data_as(C.c_void_p)) == 0
    u16 = packed.view(np.uint16)
    off, par = [0], [0]

    def take(count):
        v = flat[par[0]:par[0] + count].astype(np.float64)
        par[0] += count
        return v

    def planes(chunks, tout):
        cnt = chunks * tout * 2 * 64 * 4
        p = u16[off[0] * 2:(off[0] + cnt) * 2].view(np.float16).reshape(chunks, tout, 2, 64, 8).astype(np.float64)
        off[0] += cnt
        return p[:, :, 0] + p[:, :, 1], p[:, :, 0]

    def nearest_hi(W, o, k):
        """PERDQN's split is to the nearest f16 (ties to even): hi = f16(s w), s = 2^(10 - exponent(row max)); lo = f16(s w - hi)."""
        x = np.float64(np.float32(W[o, k]) * np.float32(2.0 ** (10 - np.floor(np.log2(np.abs(W[o]).max())))))
        hi = np.float64(np.float16(x))
        return hi, hi + np.float64(np.float16(x - hi))

    def feature(t2, hh, r):
        return 32 * t2 + (r & 3) + 8 * (r >> 2) + 4 * hh

    def k_hidden(c, hh, e):
        t, cc = divmod(c, 2)
        r = 8 * cc + e
        return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * hh

    for n_in, chunks, k_of in ((153, 10, lambda c, hh, e: 16 * c + 8 * hh + e), (64, 4, k_hidden)):
        W = take(64 * n_in).reshape(64, n_in)
        b = take(64)
        val, hip = planes(chunks, 2)
        consts = packed[off[0]:off[0] + 128].reshape(2, 2, 2, 16).astype(np.float64)
        off[0] += 128
        un, bias = np.zeros(64), np.zeros(64)
        for t2 in range(2):
            for hh in range(2):
                for r in range(16):
                    un[feature(t2, hh, r)], bias[feature(t2, hh, r)] = consts[t2, hh, 0, r], consts[t2, hh, 1, r]
        assert np.array_equal(bias, b) and np.all(np.log2(un) == np.round(np.log2(un)))
        seen = np.zeros(W.shape, bool)
        for c in range(chunks):
            for t2 in range(2):
                for lane in range(64):
                    o = 32 * t2 + (lane & 31)
                    for e in range(8):
                        k = k_of(c, lane >> 5, e)
                        if k >= n_in:
                            assert val[c, t2, lane, e] == 0
                            continue
                        assert not seen[o, k]
                        seen[o, k] = True
                        assert abs(val[c, t2, lane, e] * un[o] - W[o, k]) <= np.abs(W[o]).max() * 2.0 ** -21
                        assert (hip[c, t2, lane, e], val[c, t2, lane, e]) == nearest_hi(W, o, k)
        assert seen.all()
    W = take(8 * 64).reshape(8, 64)
    b = take(8)
    val, hip = planes(4, 1)
    val, hip = val[:, 0], hip[:, 0]
    un, bias = packed[off[0]:off[0] + 8].astype(np.float64), packed[off[0] + 8:off[0] + 16].astype(np.float64)
    off[0] += 16
    assert np.array_equal(bias, b)
    for c in range(4):
        for lane in range(64):
            o = lane & 31
            for e in range(8):
                if o >= 8:
                    assert val[c, lane, e] == 0
                else:
                    assert abs(val[c, lane, e] * un[o] - W[o, k_hidden(c, lane >> 5, e)]) <= np.abs(W[o]).max() * 2.0 ** -21
                    assert (hip[c, lane, e], val[c, lane, e]) == nearest_hi(W, o, k_hidden(c, lane >> 5, e))
    assert off[0] == len(packed) and par[0] == n


def test_rl_run_supported_answers_0_for_a_perdqn_set_and_names_the_two_launch_loop():
    lib = _lib.lib()
    cfg = _lib.Config(30, 30, 100, 2, 256, 256, 1, 0, 1, 0, 7)
    h = C.c_void_p()
    assert lib.rl_create(C.byref(cfg), C.byref(h)) == 0
    try:
        for kinds in ((_lib.PERDQN, _lib.DQN), (_lib.PERD3QN, _lib.PERDQN)):
            brains = (_lib.Brain * 2)(*[_lib.Brain(k, 0.0, None) for k in kinds])
            assert lib.rl_run_supported(h, brains, 2) == 0
            err = lib.rl_last_error().decode()
            assert "PERDQN" in err and "two-launch loop" in err, err
        brains = (_lib.Brain * 2)(_lib.Brain(_lib.PPO, 0.0, None), _lib.Brain(_lib.PERD3QN, 0.0, None))
        assert lib.rl_run_supported(h, brains, 2) == 1     # (the other kinds keep their answer)
    finally:
        lib.rl_destroy(h)


@pytest.mark.parametrize("training", [True, False])
def test_seeded_construction_gives_the_reference_initial_weights(training):
    """PERDQN.py:74-76: DQN(), model.apply(xavier_uniform on every Linear weight), target DQN() -- the same draws on torch's generator."""
    from reinlife_amd.Models import PERDQN
    d, meta = _fix()
    for s in meta["init_seeds"]:
        torch.manual_seed(s)
        b = PERDQN(training=training)
        assert [[k, list(v.shape)] for k, v in b.model.state_dict().items()] == [list(x) for x in KEYS]
        want = d["init_%d_%s" % (s, "train" if training else "greedy")]
        assert np.array_equal(_flat(b.model), want)
        assert np.array_equal(_flat(b.target_model), want)
        assert b.epsilon == (1.0 if training else 0)


def test_load_model_reads_a_pt_file_of_the_reference_keys(tmp_path):
    from reinlife_amd.Models import PERDQN
    d, meta = _fix()
    for name, m in meta["ckpt"].items():
        assert m["keys"] == [list(x) for x in KEYS]
        path = str(tmp_path / ("%s.pt" % name))
        torch.save(_sd_of(d["ckpt_%s_weights" % name]), path)
        b = PERDQN(load_model=path, training=False)
        assert np.array_equal(_flat(b.model), d["ckpt_%s_weights" % name]) and not b.model.training


@pytest.mark.parametrize("mode", ["explore", "greedy"])
def test_get_action_reproduces_the_reference_draw_for_draw(mode):
    """PERDQN.py:101-111: np.random.rand() first; <= epsilon -> random.randrange(8), else the first argmax of Q.  The Q rows are handed in
    (`out=`, as Environment.act does); afterwards both generators stand where an independent replay of the same calls leaves them."""
    from reinlife_amd.Models import PERDQN
    d, meta = _fix()
    b = PERDQN(training=(mode == "explore"))
    q, rows, want = d["act_q"], d["act_%s_rows" % mode], d["act_%s_actions" % mode]
    random.seed(meta["act_seed"]); np.random.seed(meta["act_seed"])
    got = [b.get_action(d["obs"][r], out=q[r]) for r in rows]
    assert np.array_equal(np.array(got, np.int8), want)
    py_state, np_state = random.getstate(), np.random.get_state()
    random.seed(meta["act_seed"]); np.random.seed(meta["act_seed"])
    for _ in rows:
        if np.random.rand() <= b.epsilon:
            random.randrange(8)
    assert random.getstate() == py_state
    replay = np.random.get_state()
    assert np.array_equal(replay[1], np_state[1]) and replay[2:] == np_state[2:]
    b.update_epsilon(123)
    assert b.epsilon == (1.0 if mode == "explore" else 0) and np.all(b.epsilon_schedule(5, 4) == b.epsilon)


def test_saver_writes_the_model_attribute(tmp_path):
    """entities.py:235-236: save_brain writes brain.model.state_dict() for PERDQN."""
    from reinlife_amd.Helpers.saver import SavedAgent
    from reinlife_amd.Models import PERDQN
    torch.manual_seed(3)
    b = PERDQN()
    SavedAgent(2, b).save_brain(str(tmp_path / "brain_gene_2"))
    sd = torch.load(str(tmp_path / "brain_gene_2.pt"))
    assert list(sd.keys()) == [k for k, _ in KEYS]
    assert np.array_equal(np.concatenate([v.numpy().reshape(-1) for v in sd.values()]), _flat(b.model))
