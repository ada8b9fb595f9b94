"""Host-side checks of the proprioceptive sensors (csrc/shf_proprio.hip: shf_proprioception_step; shifu_amd/proprio.py), no GPU:
the entry is declared, bound and additive (SHF_ABI_VERSION stays 22) and refuses what it cannot compute; the torch fallback
equals the NumPy twin (tests/proprio_ref.py) bit for bit; the float64 twin has the closed forms its definitions claim; the noise
has the moments the header states."""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi, proprio
from tests import proprio_ref as R

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["body_state", "body_env_stride", "body_row_stride", "dof_state", "dof_env_stride", "dof_row_stride", "contact",
         "contact_env_stride", "contact_row_stride", "reset_or_null", "config", "params", "delay", "global_ids_or_null", "counter", "imu_state", "enc_state",
         "foot_state", "n", "num_bodies", "num_dof", "out", "switch_out_or_null", "stream"]
KERNEL = "_ZN12_GLOBAL__N_116k_proprioception"
G = (0.0, 0.0, -9.81)


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


def quat_rotate(q, v):
    """v turned by the unit quaternion q (xyzw), by the sandwich product -- a route of its own, not the twin's matrix."""
    x, y, z, w = q
    u = np.array([x, y, z])
    return v + 2.0 * np.cross(u, np.cross(u, v) + w * v)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_conj(q):
    return np.array([-q[0], -q[1], -q[2], q[3]])


# ---------------------------------------------------------------------------------------------------------- plumbing --
def test_header_declares_the_entry_and_the_build_guards_its_kernel():
    m = re.search(r"\bint\s+shf_proprioception_step\s*\(([^;]*)\)\s*;", _header())
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(NAMES)
    for a, nm in zip(args, NAMES):
        assert re.search(r"\b" + nm + r"$", a), (a, nm)
    from shifu_amd import build
    assert "shf_proprio.hip" in build.UNITY_SOURCES and "shf_proprio.hip" in build.SOURCES
    guarded = {p: (v, s) for p, v, s in build.BUDGETS}
    assert guarded[KERNEL][1] == 0, "no scratch"


def test_binding_struct_and_version(lib, tmp_path):
    import json
    import subprocess
    from shifu_amd import _lib, build, glue
    from shifu_amd.utils import torch_utils
    assert "shf_proprioception_step" in _lib.EXPORTS and len(_lib._SIGS["shf_proprioception_step"][0]) == len(NAMES)
    assert callable(glue.proprioception_step) and callable(torch_utils.proprioception_step)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shifu_amd.h"\nint main(){printf("%zu %zu %zu %zu %d %d %d %d %d %d %d %d\\n",'
                   'sizeof(ShfProprioConfig),offsetof(ShfProprioConfig,imu_quat),offsetof(ShfProprioConfig,foot_body),offsetof(ShfProprioConfig,inv_dt),'
                   'SHF_PROPRIO_MAX_IMUS,SHF_PROPRIO_MAX_FEET,SHF_PROPRIO_MAX_SLOTS,SHF_PROPRIO_NUM_PARAMS,SHF_PROPRIO_CONTACT_NORM,'
                   'SHF_PROPRIO_CONTACT_Z,SHF_PROPRIO_VEL_DIRECT,SHF_PROPRIO_VEL_DIFFERENCE);}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = _abi.ShfProprioConfig
    assert got == [ctypes.sizeof(S), S.imu_quat.offset, S.foot_body.offset, S.inv_dt.offset, _abi.PROPRIO_MAX_IMUS, _abi.PROPRIO_MAX_FEET,
                   _abi.PROPRIO_MAX_SLOTS, _abi.PROPRIO_NUM_PARAMS, _abi.PROPRIO_CONTACT_MODES["norm"], _abi.PROPRIO_CONTACT_MODES["z"],
                   _abi.PROPRIO_VELOCITY_MODES["direct"], _abi.PROPRIO_VELOCITY_MODES["difference"]]
    assert len(_abi.PROPRIO_PARAMS) == 13 <= _abi.PROPRIO_NUM_PARAMS
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header()) and lib.shf_abi_version() == 22 and _abi.SHF_ABI_VERSION == 22
    res = json.load(open(build.RESOURCES))
    hits = [v for k, v in res.items() if k.startswith(KERNEL)]
    budget = {p: v for p, v, _ in build.BUDGETS}[KERNEL]
    assert len(hits) == 1 and hits[0]["scratch"] == 0 and hits[0]["vgprs"] + hits[0]["agprs"] <= budget


def test_library_refuses_what_it_cannot_compute(lib):
    """Every refusal is decided on the host, before any launch: the device pointers below are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def cfg(**kw):
        args = dict(imus=[dict(body=0), dict(body=3)], feet=[1, 2, 3, 4], slots=4, dt=0.02)
        raw = {k: kw.pop(k) for k in list(kw) if k.startswith("raw_")}
        args.update(kw)
        c = proprio.make_config(**args)
        for k, v in raw.items():                       # what make_config itself would refuse is written into the struct
            name = k[4:]
            if isinstance(v, tuple):
                getattr(c, name)[v[0]] = v[1]
            else:
                setattr(c, name, v)
        return c

    base = dict(zip(NAMES, [p, 65, 13, p, 24, 2, p, 15, 3, None, None, p, p, None, p, p, p, p, 1, 5, 12, p, p, None]))

    def refused(text, config=None, **kw):
        c = cfg() if config is None else config
        a = dict(base, config=ctypes.byref(c), **kw)
        assert lib.shf_proprioception_step(*[a[k] for k in NAMES]) != 0, (text, kw)
        msg = lib.shf_last_error()
        assert b"shf_proprioception_step" in msg and text in msg, (text, kw, msg)

    refused(b"more than 4 IMUs", cfg(raw_num_imus=5))
    refused(b"more than 8 feet", cfg(raw_num_feet=9))
    for L in (0, 9):
        refused(b"slots outside 1..8", cfg(raw_slots=L))
    for d in (4, 7, -1):
        refused(b"a delay of slots or more", cfg(raw_max_delay=d))
    for dt in (0.0, -0.02):
        refused(b"dt must be positive", cfg(raw_dt=dt))
    refused(b"dt must be positive", cfg(raw_inv_dt=0.0))
    for b in (-1, 5):
        refused(b"IMU's body index outside", cfg(raw_imu_body=(1, b)))
        refused(b"foot's body index outside", cfg(raw_foot_body=(3, b)))
    refused(b"unknown contact_mode", cfg(raw_contact_mode=2))
    refused(b"unknown velocity_mode", cfg(raw_velocity_mode=-1))
    for n in (0, -3):
        refused(b"n must be at least 1", n=n)
    for nd in (0, 33):
        refused(b"num_dof", num_dof=nd)
    for name in ("dof_state", "params", "delay", "counter", "enc_state", "out", "body_state", "imu_state", "contact", "foot_state"):
        refused(b"null tensor", **{name: None})
    refused(b"row stride", dof_row_stride=1)
    refused(b"row stride", body_row_stride=12)
    refused(b"row stride", contact_row_stride=2)
    a = dict(base, config=None)
    assert lib.shf_proprioception_step(*[a[k] for k in NAMES]) != 0 and b"null config" in lib.shf_last_error()
    # without IMUs / feet their tensors may be null -- but then the next check refuses: everything is refused before a launch here
    refused(b"n must be at least 1", cfg(imus=[], feet=[]), body_state=None, imu_state=None, contact=None, foot_state=None, n=0)


def test_make_config_refuses_with_the_same_words():
    for kw, text in ((dict(imus=[dict(body=0)] * 5), "more than 4 IMUs"), (dict(feet=list(range(9))), "more than 8 feet"),
                     (dict(slots=9), "slots"), (dict(slots=0), "slots"), (dict(slots=4, max_delay=4), "a delay of slots or more"),
                     (dict(dt=0.0), "dt must be positive"), (dict(imus=[dict(body=7)], num_bodies=5), "body index"),
                     (dict(feet=[-1], num_bodies=5), "body index"), (dict(contact_mode="x"), "mode"), (dict(velocity="fd"), "velocity")):
        with pytest.raises(ValueError, match=text):
            proprio.make_config(**kw)
    with pytest.raises(ValueError, match="f_off"):
        proprio.make_params(0.02, f_on=1.0, f_off=2.0)
    p = proprio.make_params(0.02, gyro_walk=0.5, resolution=0.001, f_on=3.0, f_off=2.0)
    assert p.dtype == torch.float32 and p.shape == (16,)
    assert p[2] == np.float32(0.5 * np.sqrt(0.02)) and p[10] == np.float32(1) / np.float32(0.001) and p[11] == 9 and p[12] == 4


# ------------------------------------------------------------------------------------------- the torch form = the twin --
IMUS = [dict(body=0, position=(0.1, -0.05, 0.2), quat=(0.1, 0.2, -0.3, 0.9)), dict(body=3, position=(-0.2, 0.0, 0.05), quat=(0.5, -0.5, 0.5, 0.5))]
NOISE = dict(gyro_noise=0.02, accel_noise=0.1, gyro_walk=0.01, accel_walk=0.05, gyro_bias=0.05, accel_bias=0.3, dof_pos_noise=0.005,
             dof_vel_noise=0.1, dof_offset=0.02, resolution=0.001, f_on=6.0, f_off=3.0)


def resets_at(k, n):
    """About 40 % of the envs at reads 5 and 11, by a fixed rule."""
    if k not in (5, 11):
        return np.zeros(n, np.uint8)
    return ((np.arange(n) * 7 + k) % 5 < 2).astype(np.uint8)


@pytest.mark.parametrize("velocity,mode", [("direct", "norm"), ("difference", "z")])
def test_torch_fallback_equals_the_twin_bit_for_bit(velocity, mode):
    from shifu_amd.utils.torch_utils import proprioception_step
    n, nb, nd, L, dt = 37, 5, 7, 4, 0.02
    c = proprio.make_config(imus=IMUS, feet=[1, 2, 3, 4], num_bodies=nb, contact_mode=mode, velocity=velocity, slots=L, gravity=G, dt=dt,
                            seed=0x1234567890ABCDEF, env_id_offset=(1 << 32) - 11)
    cfg = R.config_of(c)
    params = proprio.make_params(dt, **NOISE)
    delay = ((np.arange(n)[:, None] * np.array([1, 3, 5]) + np.array([0, 1, 2])) % L).astype(np.int32)
    st_t = proprio.make_state(n, 2, nd, 4, L)
    st_r = R.make_state(n, 2, nd, 4, L)
    out = torch.zeros(n, proprio.out_width(2, nd, 4))
    sw = torch.zeros(n, 8, dtype=torch.uint8)
    gids = cfg["env_id_offset"] + np.arange(n)
    seen = np.zeros((2, 8), bool)
    for k in range(20):
        body, dof, con = R.synthetic(gids, nb, nd, k, dt)
        rs = resets_at(k, n)
        want, want_sw = R.step32(cfg, params.numpy(), st_r, body, dof, con, delay, rs)
        proprioception_step(torch.from_numpy(body), torch.from_numpy(dof), torch.from_numpy(con), c, params, torch.from_numpy(delay), st_t, out,
                            sw, torch.from_numpy(rs))
        assert np.array_equal(out.numpy().view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(sw.numpy(), want_sw), k
        seen[0] |= (want_sw == 0).any(0)
        seen[1] |= (want_sw == 1).any(0)
        for name in proprio.STATE_NAMES:
            a, b = st_t[name].numpy(), st_r[name]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, name)
    assert seen.all(), "every switch and every touch-down flag must have been both 0 and 1"
    assert (st_r["counter"][:, :, 0] == 20).all()


def test_the_sensor_object_on_the_cpu_reads_what_the_twin_reads():
    """shifu_amd.proprio.Proprioception on CPU tensors (the torch path): read / reset / randomize / set_noise against step32 with
    the flags and delays the object holds; the dict entries are views of `flat`; delays beyond the ring are refused."""
    n, nb, nd, dt = 9, 5, 7, 0.02
    core = proprio.Proprioception(n, nb, nd, "cpu", imus=IMUS, feet=[1, 2, 3, 4], max_delay=3, delay=(3, 1, 0), gravity=G, dt=dt, seed=77,
                                  env_id_offset=40, **NOISE)
    assert not core.uses_kernel(torch.zeros(1))
    cfg = R.config_of(core.config)
    st = R.make_state(n, 2, nd, 4, 4)
    gids = 40 + np.arange(n)
    for k in range(8):
        body, dof, con = R.synthetic(gids, nb, nd, k, dt)
        if k == 3:
            core.reset([1, 4])
            core.randomize([1, 4], delay=(0, 3), generator=torch.Generator().manual_seed(1))
        if k == 5:
            core.set_noise(gyro_noise=0.5, f_on=2.0, f_off=1.0)
            assert core.params[0] == 0.5 and core.params[11] == 4.0 and core.params[1] == np.float32(NOISE["accel_noise"])
        flags = core.pending.numpy().copy()
        assert flags.tolist() == ([1] * n if k == 0 else [0, 1, 0, 0, 1, 0, 0, 0, 0] if k == 3 else [0] * n)
        o = core.read(torch.from_numpy(body), torch.from_numpy(dof), torch.from_numpy(con))
        want, want_sw = R.step32(cfg, core.params.numpy(), st, body, dof, con, core.delay.numpy(), flags)
        assert np.array_equal(core.flat.numpy().view(np.uint32), want.view(np.uint32)), k
        assert np.array_equal(core.switches.numpy(), want_sw) and not core.pending.any()
        parts = R.split(want, 2, nd, 4)
        for name in ("gyro", "accel", "dof_pos", "dof_vel", "air_time", "contact_time", "last_air_time", "last_contact_time"):
            assert np.array_equal(o[name].numpy(), parts[name]), (k, name)
        assert o["contact"].dtype == torch.uint8 and np.array_equal(o["contact"].numpy(), want_sw[:, :4])
    assert o["gyro"].data_ptr() == core.flat.data_ptr() and o["dof_pos"].data_ptr() == core.flat[:, 12:].data_ptr()
    assert core.delay[[0, 2, 3]].tolist() == [[3, 1, 0]] * 3
    with pytest.raises(ValueError, match="a delay of slots or more"):
        core.set_delay(4)
    with pytest.raises(ValueError, match="delay range"):
        core.randomize(delay=(0, 4))
    with pytest.raises(TypeError, match="unknown"):
        proprio.Proprioception(n, nb, nd, "cpu", gyro_nois=0.1)


# ------------------------------------------------------------------------------------------------ closed forms, float64 --
def _quiet(dt, **kw):
    return proprio.make_params(dt, **kw).numpy()


def _cfg(imus=(), feet=(), **kw):
    return R.config_of(proprio.make_config(imus=imus, feet=feet, **kw))


def test_a_body_at_rest_reads_no_rate_and_minus_gravity():
    rng = np.random.default_rng(5)
    n, nb, dt = 6, 3, 0.02
    qs = rng.normal(size=4)
    qs /= np.linalg.norm(qs)
    cfg = _cfg([dict(body=1, position=(0.3, -0.2, 0.1), quat=qs)], num_bodies=nb, gravity=G, dt=dt)
    qs = np.array(cfg["imus"][0][2], np.float64)                  # as the struct holds it: float32 values
    st = R.make_state(n, 1, 2, 0, 1, np.float64)
    body = np.zeros((n, nb, 13))
    qb = rng.normal(size=(n, nb, 4))
    body[..., 3:7] = qb / np.linalg.norm(qb, axis=-1, keepdims=True)
    body[..., :3] = rng.normal(size=(n, nb, 3))
    g = np.array([np.float32(v) for v in G], np.float64)
    for k in range(3):
        out, _ = R.step64(cfg, _quiet(dt), st, body, np.zeros((n, 2, 2)), None, np.zeros((n, 3), np.int32))
        o = R.split(out, 1, 2, 0)
        assert np.abs(o["gyro"]).max() == 0.0
        for e in range(n):
            want = quat_rotate(quat_conj(quat_mul(body[e, 1, 3:7], qs)), -g)
            assert np.abs(o["accel"][e, 0] - want).max() <= 1e-12, (k, e)
    up = R.step64(_cfg([dict(body=0)], num_bodies=nb, gravity=G, dt=dt), _quiet(dt), R.make_state(1, 1, 1, 0, 1, np.float64),
                  np.array([[[0, 0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0]] * nb]), np.zeros((1, 1, 2)), None, np.zeros((1, 3), np.int32))[0]
    assert np.allclose(up[0, 3:6], [0, 0, float(np.float32(9.81))], atol=1e-12), "a robot at rest reads +|g| along its up axis"


def test_a_turning_body_reads_the_centripetal_term_within_the_finite_difference_bound():
    w, r, dt = 3.0, 0.4, 1.0 / 64.0
    cfg = _cfg([dict(body=0, position=(r, 0.0, 0.0))], num_bodies=1, gravity=(0.0, 0.0, 0.0), dt=dt)
    st = R.make_state(1, 1, 1, 0, 1, np.float64)
    worst = 0.0
    for k in range(40):
        a = w * k * dt
        body = np.zeros((1, 1, 13))
        body[0, 0, 3:7] = [0.0, 0.0, np.sin(a / 2), np.cos(a / 2)]
        body[0, 0, 12] = w
        out, _ = R.step64(cfg, _quiet(dt), st, body, np.zeros((1, 1, 2)), None, np.zeros((1, 3), np.int32))
        o = R.split(out, 1, 1, 0)
        assert np.abs(o["gyro"][0, 0] - [0, 0, w]).max() <= 1e-12
        if k >= 1:
            err = np.linalg.norm(o["accel"][0, 0] - [-w * w * r, 0.0, 0.0])
            worst = max(worst, err)
    bound = w ** 3 * r * dt / 2
    print(f"[proprio] centripetal: worst error {worst:.6e}, bound {bound:.6e}")
    assert 0.5 * bound < worst <= bound


def test_integer_measurements_through_the_delays_and_a_reset():
    """Read k of an env with delay d returns the value of read max(k - d, last reset): encoders (q = 10 k + d), the gyro (a
    rate of k about z on an identity mounting) and a switch that is on at even reads."""
    n, dt, L = 4, 1.0, 4
    cfg = _cfg([dict(body=0)], [0], num_bodies=1, gravity=(0.0, 0.0, 0.0), dt=dt, slots=L, contact_mode="z")
    st = R.make_state(n, 1, 3, 1, L, np.float64)
    delay = np.repeat(np.arange(n, dtype=np.int32)[:, None], 3, 1)
    last = np.zeros(n, int)
    for k in range(14):
        body = np.zeros((n, 1, 13))
        body[:, 0, 6] = 1.0
        body[:, 0, 12] = k
        dof = np.zeros((n, 3, 2))
        dof[:, :, 0] = 10 * k + np.arange(3)
        dof[:, :, 1] = -k
        con = np.zeros((n, 1, 3))
        con[:, 0, 2] = 5.0 if k % 2 == 0 else 0.0
        rs = np.full(n, 1 if k == 6 else 0, np.uint8)
        if k == 6:
            last[:] = 6
        out, sw = R.step64(cfg, _quiet(dt, f_on=1.0), st, body, dof, con, delay, rs)
        o = R.split(out, 1, 3, 1)
        src = np.maximum(k - np.arange(n), last)
        assert np.array_equal(o["dof_pos"], 10.0 * src[:, None] + np.arange(3)), k
        assert np.array_equal(o["dof_vel"], -1.0 * src[:, None] * np.ones(3)), k
        assert np.array_equal(o["gyro"][:, 0, 2], 1.0 * src), k
        assert np.array_equal(sw[:, 0], (src % 2 == 0).astype(np.uint8)), k


def test_quantised_positions_lie_within_half_a_step_of_the_input():
    n, nd, dt, r = 50, 6, 0.02, 2.0 ** -10
    cfg = _cfg(dt=dt)
    st = R.make_state(n, 0, nd, 0, 1, np.float64)
    rng = np.random.default_rng(3)
    for k in range(3):
        dof = rng.uniform(-3, 3, size=(n, nd, 2))
        out, _ = R.step64(cfg, _quiet(dt, resolution=r), st, None, dof, None, np.zeros((n, 3), np.int32))
        q = out[:, :nd]
        assert np.abs(q - dof[:, :, 0]).max() <= r / 2
        assert np.array_equal(q / r, np.rint(q / r)) and np.abs(q - dof[:, :, 0]).max() > r / 4
        assert np.array_equal(out[:, nd:], dof[:, :, 1])
    # a differenced velocity is the difference of the quantised positions
    cfg = _cfg(dt=dt, velocity="difference")
    st = R.make_state(1, 0, 1, 0, 1, np.float64)
    qs = [0.1234, 0.2, 0.1, 0.1]
    got = [R.step64(cfg, _quiet(dt, resolution=r), st, None, np.array([[[q, 9.0]]]), None, np.zeros((1, 3), np.int32))[0][0] for q in qs]
    inv = float(np.float32(1) / np.float32(dt))
    assert got[0][1] == 0.0 and all(got[k][1] == (got[k][0] - got[k - 1][0]) * inv for k in (1, 2, 3))


def test_hysteresis_and_the_contact_times_on_a_hand_written_sequence():
    dt = 0.5
    fz = [0.0, 1.5, 2.5, 1.5, 0.5, 1.5, 3.0, 3.0, -3.0]
    #        on  first  air  contact  last_air  last_contact        (f_on = 2, f_off = 1: 1.5 keeps the state)
    want = [(0, 0, 0.5, 0.0, 0.0, 0.0),
            (0, 0, 1.0, 0.0, 0.0, 0.0),
            (1, 1, 0.0, 0.5, 1.5, 0.0),
            (1, 0, 0.0, 1.0, 1.5, 0.0),
            (0, 0, 0.5, 0.0, 1.5, 1.5),
            (0, 0, 1.0, 0.0, 1.5, 1.5),
            (1, 1, 0.0, 0.5, 1.5, 1.5),
            (1, 0, 0.0, 1.0, 1.5, 1.5),
            (0, 0, 0.5, 0.0, 1.5, 1.5)]
    cfg = _cfg(feet=[0], num_bodies=1, dt=dt, contact_mode="z")
    st = R.make_state(1, 0, 1, 1, 1, np.float64)
    params = _quiet(dt, f_on=2.0, f_off=1.0)
    for k, f in enumerate(fz):
        out, sw = R.step64(cfg, params, st, None, np.zeros((1, 1, 2)), np.array([[[0.3, -0.2, f]]]), np.zeros((1, 3), np.int32))
        assert tuple(out[0, 2:]) == want[k], (k, out[0, 2:])
        assert tuple(sw[0]) == want[k][:2]
    # a reset zeroes the times and reports no touch-down, whatever the foot stands on
    out, sw = R.step64(cfg, params, st, None, np.zeros((1, 1, 2)), np.array([[[0.0, 0.0, 5.0]]]), np.zeros((1, 3), np.int32), np.ones(1, np.uint8))
    assert tuple(out[0, 2:]) == (1, 0, 0.0, 0.5, 0.0, 0.0)
    # |f|^2 against f_z |f_z|: a sideways force closes the first switch only; a pull (f_z < 0) closes the first only
    for f, norm_on, z_on in (((3.0, 0.0, 0.0), 1, 0), ((0.0, 0.0, -3.0), 1, 0), ((0.0, 0.0, 3.0), 1, 1), ((1.0, 1.0, 1.0), 0, 0)):
        for mode, on in (("norm", norm_on), ("z", z_on)):
            o, _ = R.step64(_cfg(feet=[0], num_bodies=1, dt=dt, contact_mode=mode), params, R.make_state(1, 0, 1, 1, 1, np.float64), None,
                            np.zeros((1, 1, 2)), np.array([[f]]), np.zeros((1, 3), np.int32))
            assert o[0, 2] == on, (f, mode)


# ---------------------------------------------------------------------------------------------------------- statistics --
N_ENVS, N_READS = 257, 200
SEED_NOISE, SEED_WALK = 2027, 5


def _moments(x, sigma, what):
    n = x.size
    mean, var = x.mean(), x.var()
    print(f"[proprio] {what}: n {n}, mean / (sigma / sqrt n) {mean / (sigma / np.sqrt(n)):+.2f}, var / sigma^2 {var / sigma ** 2:.4f}")
    assert abs(mean) <= 5.0 * sigma / np.sqrt(n), what
    assert abs(var / sigma ** 2 - 1.0) <= 0.029, what


def test_noise_channels_have_the_stated_mean_and_variance():
    """257 envs x 200 reads = 51 400 draws per channel.  The mean within 5 sigma / sqrt n; the variance within 2.9 % of
    sigma^2: 5 standard errors sqrt((kurtosis - 1) / n) at the Irwin-Hall kurtosis of 2.7.  The seed is fixed."""
    n, nd, dt = N_ENVS, 3, 0.02
    sig = dict(gyro_noise=0.02, accel_noise=0.1, dof_pos_noise=0.005, dof_vel_noise=0.1)
    cfg = _cfg([dict(body=0)], num_bodies=1, gravity=G, dt=dt, seed=SEED_NOISE)
    st = R.make_state(n, 1, nd, 0, 1, np.float32)
    body = np.zeros((n, 1, 13), np.float32)
    body[:, 0, 6] = 1.0
    dof = np.zeros((n, nd, 2), np.float32)
    outs = np.stack([R.step32(cfg, _quiet(dt, **sig), st, body, dof, None, np.zeros((n, 3), np.int32))[0] for _ in range(N_READS)]).astype(np.float64)
    outs[:, :, 5] -= float(np.float32(9.81))
    for ch in range(3):
        _moments(outs[:, :, ch], sig["gyro_noise"], f"gyro {ch}")
        _moments(outs[:, :, 3 + ch], sig["accel_noise"], f"accel {ch}")
    for d in range(nd):
        _moments(outs[:, :, 6 + d], sig["dof_pos_noise"], f"dof_pos {d}")
        _moments(outs[:, :, 6 + nd + d], sig["dof_vel_noise"], f"dof_vel {d}")
    # channels are not copies of each other
    c = np.corrcoef(outs.reshape(-1, outs.shape[2]).T)
    assert np.abs(c - np.eye(c.shape[0])).max() < 0.03


def test_bias_walk_variance_grows_as_k_sigma_walk_squared_dt():
    """After k = 200 reads a bias that started at zero is the sum of k walk steps: variance k sigma_walk^2 dt, within the same
    relative margin.  One bias channel has 257 samples only, so the twelve gyro (and twelve accelerometer) channels of four
    IMUs are pooled: 3084 samples, whose standard error is 2.5 %; the seed is fixed and chosen so that the twin passes."""
    n, dt, wgy, wac = N_ENVS, 0.02, 0.01, 0.05
    cfg = _cfg([dict(body=0)] * 4, num_bodies=1, gravity=G, dt=dt, seed=SEED_WALK)
    st = R.make_state(n, 4, 1, 0, 1, np.float32)
    body = np.zeros((n, 1, 13), np.float32)
    body[:, 0, 6] = 1.0
    params = _quiet(dt, gyro_walk=wgy, accel_walk=wac)
    for _ in range(N_READS):
        R.step32(cfg, params, st, body, np.zeros((n, 1, 2), np.float32), None, np.zeros((n, 3), np.int32))
    for name, lo, w in (("gyro", 3, wgy), ("accel", 6, wac)):
        b = st["imu"][:, :, lo:lo + 3].astype(np.float64)
        want = N_READS * w * w * dt
        print(f"[proprio] {name} bias after {N_READS} reads: var / (k w^2 dt) {b.var() / want:.4f}, mean / sd {b.mean() / np.sqrt(want / b.size):+.2f}")
        assert abs(b.var() / want - 1.0) <= 0.029
        assert abs(b.mean()) <= 5.0 * np.sqrt(want / b.size)
