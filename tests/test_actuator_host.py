"""Host-side checks of the actuator models (csrc/shf_actuator.hip: shf_actuator_step; units/actuators.py), no GPU: the entry is
declared, bound and additive (SHF_ABI_VERSION stays 22) and refuses what it cannot compute; the torch fallback equals the NumPy
twin (tests/actuator_ref.py); the delay and the DC-motor clip have the properties their definitions claim; Actuator.network takes
and refuses what it should; a Robot without an actuator is as it was."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from shifu_amd import _abi
from tests import actuator_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["target", "dof_state", "dof_elem_stride", "kp_or_null", "kd_or_null", "gain_env_stride", "delay_or_null", "delay_scalar",
         "strength_or_null", "saturation_or_null", "velocity_limit_or_null", "effort_limit_or_null", "reset_or_null", "mode", "net_or_null",
         "weights_or_null", "weights_count", "cmd_hist", "cmd_slots", "err_hist_or_null", "vel_hist_or_null", "hist_slots", "n", "num_dof",
         "applied_target_out_or_null", "efforts_out", "stream"]
KERNELS = ("_ZN12_GLOBAL__N_113k_actuator_pd", "_ZN12_GLOBAL__N_114k_actuator_netILi32E", "_ZN12_GLOBAL__N_114k_actuator_netILi64E")
SAT, VLIM, LIM = 33.5, 21.0, 33.5


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---------------------------------------------------------------------------------------------------------- plumbing --
def test_header_declares_the_entry_and_the_build_guards_its_kernels():
    m = re.search(r"\bint\s+shf_actuator_step\s*\(([^;]*)\)\s*;", _header())
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(NAMES)
    for a, nm in zip(args, NAMES):
        assert re.search(r"\b" + nm + r"$", a), (a, nm)
    from shifu_amd import build
    assert "shf_actuator.hip" in build.UNITY_SOURCES and "shf_actuator.hip" in build.SOURCES
    guarded = {p: (v, s) for p, v, s in build.BUDGETS}
    for k in KERNELS:
        assert guarded[k][1] == 0, "no scratch"


def test_binding_struct_and_version(lib, tmp_path):
    import json
    import subprocess
    from shifu_amd import _lib, build, glue
    assert "shf_actuator_step" in _lib.EXPORTS and len(_lib._SIGS["shf_actuator_step"][0]) == len(NAMES)
    assert callable(glue.actuator_step)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "shifu_amd.h"\nint main(){printf("%zu %d %d %d %d %d %d\\n",sizeof(ShfActuatorNet),'
                   'SHF_ACTUATOR_PD,SHF_ACTUATOR_NET,SHF_ACTUATOR_SOFTSIGN,SHF_ACTUATOR_RELU,SHF_ACTUATOR_TANH,SHF_ACTUATOR_ELU);'
                   'printf("%d %d %d %d\\n",SHF_ACTUATOR_MAX_SLOTS,SHF_ACTUATOR_MAX_TAPS,SHF_ACTUATOR_MAX_LAYERS,SHF_ACTUATOR_MAX_WIDTH);}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    A = _abi.ACTUATOR_ACTIVATIONS
    assert got == [ctypes.sizeof(_abi.ShfActuatorNet), _abi.ACTUATOR_PD, _abi.ACTUATOR_NET, A["softsign"], A["relu"], A["tanh"], A["elu"],
                   _abi.ACTUATOR_MAX_SLOTS, _abi.ACTUATOR_MAX_TAPS, _abi.ACTUATOR_MAX_LAYERS, _abi.ACTUATOR_MAX_WIDTH]
    assert got[0] == 60
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header()) and lib.shf_abi_version() == 22 and _abi.SHF_ABI_VERSION == 22
    res = json.load(open(build.RESOURCES))
    for prefix, vg, sc in build.BUDGETS:
        if prefix in KERNELS:
            hits = [v for k, v in res.items() if k.startswith(prefix)]
            assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["vgprs"] + hits[0]["agprs"] <= vg


def _net_struct(widths=(6, 32, 32, 32, 1), taps=(0, 1, 2), activation=0):
    s = _abi.ShfActuatorNet()
    s.activation, s.num_layers, s.num_taps = activation, len(widths) - 1, len(taps)
    for i, w in enumerate(widths[:5]):
        s.widths[i] = w
    for i, k in enumerate(taps[:4]):
        s.taps[i] = k
    s.err_scale = s.vel_scale = s.out_scale = 1.0
    return s


def test_library_refuses_what_it_cannot_compute(lib):
    """Every refusal is decided on the host, before any launch: the device pointers below are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    count = 9 * 32 + 2 * (32 * 32 + 32) + 33 + 3                  # 6-32-32-32-1, padded: 2436 floats
    pd = dict(zip(NAMES, [p, p, 2, p, p, 0, None, 0, None, None, None, None, None, _abi.ACTUATOR_PD, None, None, 0, p, 4, None, None, 1, 1, 12,
                          None, p, None]))
    net = dict(pd, mode=_abi.ACTUATOR_NET, net_or_null=ctypes.pointer(_net_struct()), weights_or_null=p, weights_count=count,
               err_hist_or_null=p, vel_hist_or_null=p, hist_slots=3, kp_or_null=None, kd_or_null=None)

    def refused(base, text, **kw):
        a = dict(base, **kw)
        assert lib.shf_actuator_step(*[a[k] for k in NAMES]) != 0, kw
        msg = lib.shf_last_error()
        assert b"shf_actuator_step" in msg and text in msg, (kw, msg)

    for name in ("target", "dof_state", "cmd_hist", "efforts_out", "kp_or_null", "kd_or_null"):
        refused(pd, b"null tensor", **{name: None})
    for nd in (0, 33):
        refused(pd, b"num_dof", num_dof=nd)
    for n in (0, -1):
        refused(pd, b"n must be at least 1", n=n)
    for L in (0, 9):
        refused(pd, b"cmd_slots", cmd_slots=L)
    for d in (-1, 4):
        refused(pd, b"delay_scalar", delay_scalar=d)
    for g in (1, 24, -12):
        refused(pd, b"gain_env_stride", gain_env_stride=g)
    refused(pd, b"saturation and velocity_limit", saturation_or_null=p)
    refused(pd, b"saturation and velocity_limit", velocity_limit_or_null=p)
    for mode in (-1, 2):
        refused(pd, b"unknown mode", mode=mode)
    refused(pd, b"dof_elem_stride", dof_elem_stride=1)
    refused(net, b"without weights", weights_or_null=None)
    refused(net, b"without weights", net_or_null=None)
    refused(net, b"without histories", err_hist_or_null=None)
    refused(net, b"without histories", vel_hist_or_null=None)
    for H in (0, 9):
        refused(net, b"hist_slots", hist_slots=H)
    refused(net, b"tap outside", net_or_null=ctypes.pointer(_net_struct(taps=(0, 1, 3))))
    refused(net, b"tap outside", net_or_null=ctypes.pointer(_net_struct(taps=(0, -1, 2))))
    s = _net_struct()
    s.num_taps = 0
    refused(net, b"num_taps", net_or_null=ctypes.pointer(s))
    s.num_taps = 5
    refused(net, b"num_taps", net_or_null=ctypes.pointer(s))
    s = _net_struct()
    s.num_layers = 5
    refused(net, b"more than 4 layers", net_or_null=ctypes.pointer(s))
    s.num_layers = 0
    refused(net, b"at least one layer", net_or_null=ctypes.pointer(s))
    refused(net, b"width outside 1..64", net_or_null=ctypes.pointer(_net_struct(widths=(6, 65, 32, 32, 1))))
    refused(net, b"width outside 1..64", net_or_null=ctypes.pointer(_net_struct(widths=(6, 32, 0, 32, 1))))
    refused(net, b"first width", net_or_null=ctypes.pointer(_net_struct(widths=(4, 32, 32, 32, 1))))
    refused(net, b"last width", net_or_null=ctypes.pointer(_net_struct(widths=(6, 32, 32, 32, 2))))
    for act in (-1, 4):
        refused(net, b"unknown activation", net_or_null=ctypes.pointer(_net_struct(activation=act)))
    refused(net, b"weights_count", weights_count=count - 4)
    refused(net, b"weights_count", net_or_null=ctypes.pointer(_net_struct(widths=(6, 33, 32, 32, 1))))     # P = 64: another layout
    refused(net, b"16-byte aligned", weights_or_null=ctypes.c_void_p(p.value + 4))


# ----------------------------------------------------------------------------------------------------- torch fallback --
def _run_both(n, nd, calls, L, net=None, dc=False, seed=0):
    """`calls` consecutive calls of the CPU torch fallback (through an Actuator) and of step32 / step64 with the state carried
    on each side: per-env delays, strengths and gains; resets on calls 0, 5 and 11.  Yields per call (fallback efforts, the
    Actuator, step32's output and state, step64's output, the float64 network inputs)."""
    from shifu_amd.units import Actuator, ActuatorNet
    rng = np.random.default_rng(seed)
    delay = (np.arange(n) % L).astype(np.int32)
    strength = rng.uniform(0.8, 1.2, (n, nd)).astype(np.float32)
    kp, kd = rng.uniform(30, 50, (n, nd)).astype(np.float32), rng.uniform(0.5, 1.5, (n, nd)).astype(np.float32)
    lims = dict(saturation=np.full(nd, SAT, np.float32), velocity_limit=np.full(nd, VLIM, np.float32)) if dc else {}
    lim = np.full(nd, LIM, np.float32)
    kw = dict(saturation_effort=t(lims["saturation"]), velocity_limit=t(lims["velocity_limit"])) if dc else {}
    if net is None:
        act = Actuator(kp=t(kp), kd=t(kd), effort_limit=t(lim), max_delay=L - 1, **kw)
    else:
        act = Actuator.network(ActuatorNet(net["layers"], net["activation"]), taps=net["taps"], err_scale=net["err_scale"], vel_scale=net["vel_scale"],
                               out_scale=net["out_scale"], effort_limit=t(lim), max_delay=L - 1, **kw)
    act.bind(n, nd, "cpu")
    act.set_delay(t(delay))
    act.set_strength(t(strength))
    H = None if net is None else max(net["taps"]) + 1
    s32, s64 = R.new_state(n, nd, L, H), R.new_state(n, nd, L, H, np.float64)
    for c in range(calls):
        X = R.seeded_call(rng, n, nd)
        reset = None
        if c in (0, 5, 11):
            reset = np.ones(n, np.uint8) if c == 0 else (rng.uniform(size=n) < 0.4).astype(np.uint8)
            reset[0] = 1
            act.reset(torch.nonzero(t(reset)).reshape(-1))
        got = act.efforts(t(X["target"]), t(np.stack([X["q"], X["qd"]], -1)))
        args = dict(kp=kp, kd=kd, delay=delay, strength=strength, effort_limit=lim, reset=reset, net=net, **lims)
        o32 = R.step32(s32, X["target"], X["q"], X["qd"], **args)
        o64 = R.step64(s64, X["target"], X["q"], X["qd"], **args)
        x64 = None
        if net is not None:
            taps = list(net["taps"])
            x64 = np.concatenate([net["err_scale"] * s64["err"][:, taps], net["vel_scale"] * s64["vel"][:, taps]], 1).transpose(0, 2, 1).reshape(n * nd, -1)
        yield got.numpy().copy(), act, o32, s32, o64, x64, strength


@pytest.mark.parametrize("dc", [False, True], ids=["pd", "dc-motor"])
def test_torch_fallback_equals_the_twin_bit_for_bit(dc):
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.int32)
    for got, act, o32, s32, _, _, _ in _run_both(65, 5, 14, 4, dc=dc):
        assert np.array_equal(bits(got), bits(o32["efforts"]))
        assert np.array_equal(bits(act.applied_target.numpy()), bits(o32["applied"])) and np.array_equal(bits(act.cmd_hist.numpy()), bits(s32["cmd"]))


@pytest.mark.parametrize("activation", R.ACTIVATIONS)
def test_torch_fallback_network_is_within_the_bound(activation):
    """A CPU matmul sums in another order than step 5 states, so the network's fallback is held to the worst-case forward error
    of that sum (actuator_ref.bound); the states do not pass through the network and stay bit-equal."""
    net = R.make_net([6, 32, 32, 32, 1], activation, err_scale=2.0, vel_scale=0.1, out_scale=20.0, seed=3)
    worst = 0.0
    for got, act, o32, s32, o64, x64, strength in _run_both(33, 12, 14, 3, net=net, dc=True):
        b = R.bound(net, x64, strength).reshape(got.shape)
        for a in (got, o32["efforts"]):
            d = np.abs(a.astype(np.float64) - o64["efforts"])
            assert (d <= b).all(), (activation, float((d - b).max()))
            worst = max(worst, float((d / b).max()))
        for k, h in (("cmd", act.cmd_hist), ("err", act.err_hist), ("vel", act.vel_hist)):
            assert np.array_equal(h.numpy(), s32[k]), k
    print(f"[actuator host] {activation}: worst error / bound {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- delay --
@pytest.mark.parametrize("form", ["twin", "fallback"])
def test_delay_on_integers(form):
    """Targets 0, 1, 2, ... over 12 calls, per-env delays 0..3 with L = 4, envs 1, 2, 5 and 6 reset at call 6: the applied target
    is the target of `delay` calls ago, but never older than the env's last reset."""
    from shifu_amd.utils import torch_utils as TU
    n, nd, L = 8, 3, 4
    delay = (np.arange(n) % 4).astype(np.int32)
    st = R.new_state(n, nd, L)
    cmd, applied = torch.zeros(n, L, nd), torch.zeros(n, nd)
    last = np.zeros(n)
    for c in range(12):
        target = np.full((n, nd), float(c), np.float32)
        reset = np.ones(n, np.uint8) if c == 0 else np.zeros(n, np.uint8)
        if c == 6:
            reset[[1, 2, 5, 6]] = 1
        last[reset != 0] = c
        zero = np.zeros((n, nd), np.float32)
        if form == "twin":
            a = R.step32(st, target, zero, zero, kp=np.ones(nd), kd=np.ones(nd), delay=delay, reset=reset)["applied"]
        else:
            TU.actuator_step(t(target), t(np.stack([zero, zero], -1)), cmd, kp=torch.ones(nd), kd=torch.ones(nd), delay=t(delay), reset=t(reset),
                             applied_out=applied)
            a = applied.numpy()
        want = np.maximum(c - delay, last)[:, None].repeat(nd, 1)
        assert np.array_equal(a, want), (c, a[:, 0], want[:, 0])
    # a scalar delay is the same delay for every env; one beyond the history is refused
    st = R.new_state(n, nd, L)
    for c in range(5):
        a = R.step32(st, np.full((n, nd), float(c), np.float32), zero, zero, kp=np.ones(nd), kd=np.ones(nd), delay=2,
                     reset=np.ones(n) if c == 0 else None)["applied"]
        assert (a == max(c - 2, 0)).all()
    with pytest.raises(AssertionError):
        TU.actuator_step(t(target), t(np.stack([zero, zero], -1)), cmd, kp=torch.ones(nd), kd=torch.ones(nd), delay=4)


# -------------------------------------------------------------------------------------------------------------- DC clip --
@pytest.mark.parametrize("form", ["twin", "fallback"])
def test_dc_clip_in_closed_form(form):
    """sat = 30 with lim = 40, 30 and 20.  At qd = vlim a positive torque gives 0; at qd = 0 the cap is min(sat, lim); at
    qd = -vlim the positive cap is min(2 sat, lim); the same mirrored by sign; a small torque passes where it may."""
    from shifu_amd.utils import torch_utils as TU
    sat, vlim = 30.0, 21.0
    lims = np.array([40.0, 30.0, 20.0], np.float32)
    nd = 3

    def run(tau, qd):
        n = 1
        target = np.full((n, nd), tau, np.float32)                 # kp = 1, q = 0, kd = 0: the pre-clip torque is the target
        q, v = np.zeros((n, nd), np.float32), np.full((n, nd), qd, np.float32)
        kw = dict(saturation=np.full(nd, sat, np.float32), velocity_limit=np.full(nd, vlim, np.float32), effort_limit=lims)
        if form == "twin":
            return R.step32(R.new_state(n, nd, 1), target, q, v, kp=np.ones(nd), kd=np.zeros(nd), reset=np.ones(n), **kw)["efforts"][0]
        return TU.actuator_step(t(target), t(np.stack([q, v], -1)), torch.zeros(n, 1, nd), kp=torch.ones(nd), kd=torch.zeros(nd),
                                reset=torch.ones(n, dtype=torch.uint8), saturation=t(kw["saturation"]), velocity_limit=t(kw["velocity_limit"]),
                                effort_limit=t(lims)).numpy()[0]

    for sign in (1.0, -1.0):
        assert (run(sign * 100.0, sign * vlim) == 0.0).all()
        assert np.array_equal(run(sign * 100.0, 0.0), sign * np.minimum(sat, lims))
        assert np.array_equal(run(sign * 100.0, -sign * vlim), sign * np.minimum(2 * sat, lims))
        assert np.array_equal(run(-sign * 100.0, sign * vlim), -sign * np.minimum(2 * sat, lims)), "braking torque is available at speed"
        assert np.array_equal(run(sign * 5.0, 0.0), np.full(nd, sign * 5.0, np.float32))
        assert np.array_equal(run(sign * 100.0, sign * 2 * vlim), np.zeros(nd, np.float32)), "beyond the no-load speed: nothing"
    # without an effort limit (or entries <= 0) only the speed line binds
    no = R.step32(R.new_state(1, nd, 1), np.full((1, nd), 100.0, np.float32), np.zeros((1, nd)), np.full((1, nd), -vlim), kp=np.ones(nd), kd=np.zeros(nd),
                  saturation=np.full(nd, sat), velocity_limit=np.full(nd, vlim), effort_limit=np.array([0.0, -1.0, 50.0]))["efforts"][0]
    assert np.array_equal(no, [60.0, 60.0, 50.0])


def test_dc_case_of_the_gpu_test_reaches_every_branch():
    """The inputs tests/test_gpu_actuator.py uses for the DC motor (qd ~ N(0, 8^2), pre-clip torque of sigma about 25 N m, sat =
    lim = 33.5, vlim = 21): each of clipped from above, clipped from below, left alone and speed-limited ceiling is at least 5 %."""
    shares = dc_shares(257, 12, 3)
    print("[actuator host] DC shares", {k: round(v, 3) for k, v in shares.items()})
    assert 20.0 <= shares.pop("sigma") <= 30.0
    assert all(v >= 0.05 for v in shares.values()), shares


def dc_shares(n, nd, calls, seed=1):
    rng = np.random.default_rng(seed)
    st = R.new_state(n, nd, 1, dtype=np.float64)
    above = below = alone = speed = total = 0
    pre = []
    for c in range(calls):
        X = R.seeded_call(rng, n, nd)
        o = R.step64(st, X["target"], X["q"], X["qd"], kp=np.full(nd, 40.0), kd=np.full(nd, 1.0), saturation=np.full(nd, SAT),
                     velocity_limit=np.full(nd, VLIM), effort_limit=np.full(nd, LIM), reset=np.ones(n) if c == 0 else None)
        above += int((o["pre"] > o["hi"]).sum())
        below += int((o["pre"] < o["lo"]).sum())
        alone += int(((o["pre"] <= o["hi"]) & (o["pre"] >= o["lo"])).sum())
        speed += int((o["hi"] < o["cap"]).sum())
        total += o["pre"].size
        pre.append(o["pre"])
    return {"above": above / total, "below": below / total, "alone": alone / total, "speed_limited": speed / total,
            "sigma": float(np.concatenate(pre).std())}


# ------------------------------------------------------------------------------------------------------ Actuator.network --
def test_network_sources_round_trip_and_limits(tmp_path):
    from shifu_amd.units import Actuator, ActuatorNet
    nn = torch.nn
    torch.manual_seed(0)
    seq = nn.Sequential(nn.Linear(6, 32), nn.Softsign(), nn.Linear(32, 32), nn.Softsign(), nn.Linear(32, 32), nn.Softsign(), nn.Linear(32, 1))
    a = ActuatorNet.of(seq)
    assert a.widths == [6, 32, 32, 32, 1] and a.activation == "softsign" and a.padded_width == 32 and a.pack().numel() == 2436
    path = str(tmp_path / "net.npz")
    a.save_npz(path)
    z = np.load(path)
    assert sorted(z.files) == ["activation", "b0", "b1", "b2", "b3", "w0", "w1", "w2", "w3"]
    b = ActuatorNet.of(path)
    c = ActuatorNet.of(seq.state_dict(), activation="softsign")
    for other in (b, c):
        assert other.activation == "softsign" and all(torch.equal(W, V) and torch.equal(p, q) for (W, p), (V, q) in zip(a.layers, other.layers))
    x = torch.randn(9, 6)
    assert torch.equal(b.module()(x), seq(x))
    assert ActuatorNet.of(nn.Sequential(nn.Linear(4, 8), nn.ELU(), nn.Linear(8, 1))).activation == "elu"
    # through an Actuator on the CPU: the fallback gives the module's output on the taps
    act = Actuator.network(path, out_scale=2.0)
    q, qd, tg = torch.randn(3, 2), torch.randn(3, 2), torch.randn(3, 2)
    got = act.efforts(tg, torch.stack([q, qd], -1))
    feats = torch.stack([tg - q, torch.zeros(3, 2), torch.zeros(3, 2), qd, torch.zeros(3, 2), torch.zeros(3, 2)], -1).reshape(6, 6)
    assert torch.allclose(got.reshape(-1), 2.0 * seq(feats).reshape(-1), atol=1e-6)
    # outside the kernel's limits: refused, the limit named
    wide = nn.Sequential(nn.Linear(6, 65), nn.ReLU(), nn.Linear(65, 1))
    with pytest.raises(ValueError, match="width 65.*1 to 64"):
        Actuator.network(wide)
    deep = nn.Sequential(*[m for k in range(4) for m in (nn.Linear(6 if k == 0 else 8, 8), nn.Tanh())], nn.Linear(8, 1))
    with pytest.raises(ValueError, match="5 linear layers.*1 to 4"):
        Actuator.network(deep)
    with pytest.raises(ValueError, match="2 x the taps"):
        Actuator.network(seq, taps=(0, 1))
    with pytest.raises(ValueError, match="last width of 1"):
        Actuator.network(nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 2)))
    with pytest.raises(ValueError, match="lags of 0 to 7"):
        Actuator.network(seq, taps=(0, 1, 8))
    with pytest.raises(ValueError, match="one kind of activation"):
        Actuator.network(nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Linear(8, 8), nn.Tanh(), nn.Linear(8, 1)))
    with pytest.raises(ValueError, match="neither a Linear"):
        Actuator.network(nn.Sequential(nn.Linear(6, 8), nn.Sigmoid(), nn.Linear(8, 1)))
    with pytest.raises(ValueError, match="max_delay 8"):
        Actuator.pd(1.0, 1.0, delay=8)
    with pytest.raises(ValueError, match="together"):
        Actuator.dc_motor(1.0, 1.0, 30.0, None)


@pytest.mark.parametrize("widths", [[6, 33, 5, 1], [6, 32, 32, 32, 1], [2, 8, 1], [8, 64, 64, 1], [6, 1]])
@pytest.mark.parametrize("activation", ["softsign", "relu"])
def test_zero_padding_leaves_step32_unchanged(widths, activation):
    """The kernel is handed the net padded to hidden widths of 32 or 64; the padded net's step32 is the unpadded net's, bit for
    bit, and ActuatorNet.pack() is that padded net in the layout the header states."""
    from shifu_amd.units import ActuatorNet
    T = widths[0] // 2
    net = R.make_net(widths, activation, taps=tuple(range(T)), err_scale=1.5, vel_scale=0.2, out_scale=10.0, seed=5)
    rng = np.random.default_rng(2)
    n, nd = 19, 5
    for P in (32, 64):
        if max(widths[1:-1], default=1) > P:
            continue
        pn = R.pad_net(net, P)
        sa, sb = R.new_state(n, nd, 2, T), R.new_state(n, nd, 2, T)
        for c in range(4):
            X = R.seeded_call(rng, n, nd)
            kw = dict(delay=1, reset=np.ones(n) if c == 0 else None)
            a = R.step32(sa, X["target"], X["q"], X["qd"], net=net, **kw)["efforts"]
            b = R.step32(sb, X["target"], X["q"], X["qd"], net=pn, **kw)["efforts"]
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    an = ActuatorNet(net["layers"], activation)
    pn = R.pad_net(net, an.padded_width)
    flat = np.concatenate([np.concatenate([W.reshape(-1), b]) for W, b in pn["layers"]])
    packed = an.pack().numpy()
    assert packed.size % 4 == 0 and packed.size - flat.size < 4 and np.array_equal(packed[:flat.size], flat) and (packed[flat.size:] == 0).all()


# ------------------------------------------------------------------------------------------------------ Actuator, Robot --
def test_actuator_options_on_the_cpu():
    from shifu_amd.units import Actuator
    n, nd = 6, 4
    act = Actuator.pd(40.0, [1.0, 2.0, 3.0, 4.0], effort_limit=20.0, delay=1, max_delay=3).bind(n, nd, "cpu")
    assert tuple(act.cmd_hist.shape) == (n, 4, nd) and act.kp.tolist() == [40.0] * 4 and act.delay == 1 and act.err_hist is None
    g = torch.Generator().manual_seed(0)
    act.randomize(torch.tensor([1, 3]), delay=(2, 3), strength=(0.8, 1.2), kp_scale=(0.9, 1.1), kd_scale=(0.5, 0.6), generator=g)
    assert act.delay.dtype == torch.int32 and act.delay[[0, 2, 4, 5]].tolist() == [1] * 4 and all(2 <= d <= 3 for d in act.delay[[1, 3]].tolist())
    assert tuple(act.kp.shape) == (n, nd) and torch.equal(act.kp[0], torch.full((nd,), 40.0)) and bool(((act.kp[1] >= 36) & (act.kp[1] <= 44)).all())
    assert torch.equal(act.kd[2], torch.tensor([1.0, 2.0, 3.0, 4.0])) and bool((act.kd[3] <= torch.tensor([0.6, 1.2, 1.8, 2.4]) + 1e-6).all())
    assert torch.equal(act.strength[0], torch.ones(nd)) and 0.8 <= float(act.strength[1, 0]) <= 1.2 and bool((act.strength[1] == act.strength[1, 0]).all())
    with pytest.raises(ValueError, match="max_delay = 3"):
        act.set_delay(4)
    with pytest.raises(ValueError, match="max_delay = 3"):
        act.randomize(delay=(0, 4))
    # reset flags are consumed by the next call
    tg = torch.arange(n * nd, dtype=torch.float32).reshape(n, nd)
    ds = torch.zeros(n, nd, 2)
    assert act.any_pending
    e = act.efforts(tg, ds)
    assert not act.any_pending and int(act.pending.sum()) == 0 and e is act.efforts_buf
    assert torch.equal(act.cmd_hist, tg.unsqueeze(1).expand(n, 4, nd)) and torch.equal(act.applied_target, tg)
    assert bool((e.abs() <= 20.0).all()) and float(e[0, 1]) == 20.0
    act.efforts(tg + 100.0, ds)
    act.reset(torch.tensor([2]))
    act.efforts(tg + 200.0, ds.view(n * nd, 2))                    # the flat dof-state tensor is taken too
    assert torch.equal(act.cmd_hist[2], (tg[2] + 200.0).expand(4, nd)) and torch.equal(act.cmd_hist[0, :, 0], torch.tensor([200.0, 100.0, 0.0, 0.0]))
    with pytest.raises(RuntimeError, match="not bound"):
        Actuator.pd(1.0, 1.0).reset()


def test_robot_without_an_actuator_is_as_it_was():
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.units import Actuator, Robot
    r = Robot.__new__(Robot)
    calls = []
    r._reset_dof_state = lambda ids: calls.append(("dof", ids))
    r._reset_root_state = lambda ids: calls.append(("root", ids))
    r.reset_idx([1, 2])
    assert calls == [("dof", [1, 2]), ("root", [1, 2])] and not hasattr(r, "actuator")
    with pytest.raises(RuntimeError, match="no actuator"):
        r.apply_actuator_targets(torch.zeros(2, 3))
    r.asset_options = SimpleNamespace(default_dof_drive_mode=gymapi.DOF_MODE_POS)
    with pytest.raises(RuntimeError, match="DOF_MODE_EFFORT"):
        r.set_actuator(Actuator.pd(1.0, 1.0))
    r.asset_options = SimpleNamespace(default_dof_drive_mode=gymapi.DOF_MODE_EFFORT)
    r.env, r.num_dof, r.device = SimpleNamespace(num_envs=4), 3, "cpu"
    act = Actuator.pd(1.0, 1.0)
    r.set_actuator(act)
    act.efforts(torch.zeros(4, 3), torch.zeros(4, 3, 2))
    r.reset_idx(torch.tensor([1, 2]))
    assert act.pending.tolist() == [0, 1, 1, 0] and act.any_pending
    r.set_actuator(None)
    assert r.actuator is None
