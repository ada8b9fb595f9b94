"""Host-side checks of the gait planner and the effort merge (csrc/shf_gait.hip: shf_gait_plan, shf_leg_effort_mix), no GPU: the
entries are declared, bound and additive (SHF_ABI_VERSION stays 22) and refuse what they cannot compute; the algorithm (its
float64 NumPy twin, tests/gait_ref.py) has the properties its header claims; the torch fallback equals the twin."""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi
from tests import gait_ref as G

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.005
NOM = G.NOMINAL
TROT = (60, [0, 30, 30, 0], [30, 30, 30, 30])
STAND = (60, [0, 0, 0, 0], [60, 60, 60, 60])
PLAN_NAMES = ["root_pose", "root_env_stride", "foot_pos", "foot_env_stride", "foot_stride", "contact_z_or_null", "contact_env_stride",
              "contact_foot_stride", "command", "nominal", "reset_or_null", "period_ticks", "offset_ticks", "stance_ticks", "params",
              "tick", "sched", "anchor", "target", "yaw", "n", "num_feet", "stance_out", "swing_target_out", "phase_out", "stream"]
MIX_NAMES = ["stance_efforts", "swing_efforts", "stance", "chain_mask", "effort_limit_or_null", "n", "num_feet", "num_dof", "efforts_out",
             "stream"]


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


def _flat(n=1, yaw=0.0, v=(0.0, 0.0), pos=(0.0, 0.0, 0.30)):
    """n identical level bases at `pos`, heading `yaw`, moving at v, with the feet at their nominal places on the ground."""
    root = np.zeros((n, 13))
    root[:, :3] = pos
    root[:, 5], root[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    root[:, 7:9] = v
    R = G.rotation(root[:, 3:7])
    feet = root[:, None, :3] + np.einsum("nij,fj->nfi", R, NOM)
    return root, feet


def _start(n, root, feet, P, ticks=TROT):
    """A state after its reset tick with a zero command (the clock then stands at 1)."""
    st = G.new_state(n, 4)
    G.plan(st, root, feet, None, np.zeros((n, 3)), NOM, np.ones(n, np.uint8), *ticks, P)
    return st


# ---------------------------------------------------------------------------------------------------------- plumbing --
def test_header_declares_the_entries():
    for name, names in (("shf_gait_plan", PLAN_NAMES), ("shf_leg_effort_mix", MIX_NAMES)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(names)
        for a, nm in zip(args, names):
            assert re.search(r"\b" + nm + r"$", a), (a, nm)
    assert os.path.exists(os.path.join(ROOT, "shifu_amd", "csrc", "shf_gait.hip"))
    from shifu_amd import build
    assert "shf_gait.hip" in build.UNITY_SOURCES and "shf_gait.hip" in build.SOURCES
    guarded = {p: (v, s) for p, v, s in build.BUDGETS}
    assert guarded["_ZN12_GLOBAL__N_111k_gait_plan"][1] == 0 and guarded["_ZN12_GLOBAL__N_116k_leg_effort_mix"][1] == 0


def test_binding_table_and_struct_cover_the_entries(lib, tmp_path):
    import subprocess
    from shifu_amd import _lib, glue
    assert "shf_gait_plan" in _lib.EXPORTS and len(_lib._SIGS["shf_gait_plan"][0]) == len(PLAN_NAMES)
    assert "shf_leg_effort_mix" in _lib.EXPORTS and len(_lib._SIGS["shf_leg_effort_mix"][0]) == len(MIX_NAMES)
    assert _lib._SIGS["shf_gait_plan"][0][PLAN_NAMES.index("params")] is _abi.ShfGaitParams
    assert [f for f, _ in _abi.ShfGaitParams._fields_] == list(G.PARAM_NAMES)
    assert callable(glue.gait_plan) and callable(glue.leg_effort_mix) and callable(glue.locomotion_control)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "shifu_amd.h"\nint main(){printf("%zu\\n",sizeof(ShfGaitParams));}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert int(subprocess.check_output([str(exe)])) == ctypes.sizeof(_abi.ShfGaitParams) == 36
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header()) and lib.shf_abi_version() == 22


def test_library_refuses_what_it_cannot_compute(lib):
    """Every refusal is decided on the host, before any launch: the device pointers below are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    ia = ctypes.c_int32 * 4
    par = _abi.ShfGaitParams(DT, 0.3, 0.06, 0.01, 0.02, 0.18, 0.15, float("inf"), 1.0)
    good = dict(zip(PLAN_NAMES, [out, 13, out, 12, 3, None, 0, 0, out, out, None, 60, ia(0, 30, 30, 0), ia(30, 30, 30, 30), par,
                                 out, out, out, out, out, 1, 4, out, out, out, None]))

    def refused(text, **kw):
        a = dict(good, **kw)
        assert lib.shf_gait_plan(*[a[k] for k in PLAN_NAMES]) != 0, kw
        msg = lib.shf_last_error()
        assert b"shf_gait_plan" in msg and text in msg, (kw, msg)

    for name in ("root_pose", "foot_pos", "command", "nominal", "offset_ticks", "stance_ticks", "tick", "sched", "anchor", "target", "yaw",
                 "stance_out", "swing_target_out", "phase_out"):
        refused(b"null tensor", **{name: None})
    refused(b"1 to 4 feet", num_feet=0)
    refused(b"1 to 4 feet", num_feet=5)
    refused(b"period_ticks", period_ticks=0)
    refused(b"stance_ticks", stance_ticks=ia(30, 0, 30, 30))
    refused(b"stance_ticks", stance_ticks=ia(30, 30, 30, 61))
    refused(b"offset_ticks", offset_ticks=ia(0, -1, 30, 0))
    refused(b"offset_ticks", offset_ticks=ia(0, 30, 60, 0))
    for dt in (0.0, -DT, float("nan")):
        refused(b"dt", params=_abi.ShfGaitParams(dt, 0.3, 0.06, 0.01, 0.02, 0.18, 0.15, float("inf"), 1.0))
    refused(b"max_step", params=_abi.ShfGaitParams(DT, 0.3, 0.06, 0.01, 0.02, 0.18, -0.1, float("inf"), 1.0))
    assert lib.shf_gait_plan(*[dict(good, n=0)[k] for k in PLAN_NAMES]) == 0          # nothing to do: no launch
    goodm = dict(zip(MIX_NAMES, [out, out, out, out, None, 1, 4, 12, out, None]))
    for name in ("stance_efforts", "swing_efforts", "stance", "chain_mask", "efforts_out"):
        a = dict(goodm, **{name: None})
        assert lib.shf_leg_effort_mix(*[a[k] for k in MIX_NAMES]) != 0 and b"shf_leg_effort_mix: null tensor" in lib.shf_last_error()
    for kw, text in ((dict(num_feet=0), b"feet"), (dict(num_feet=33), b"feet"), (dict(num_dof=0), b"dof")):
        a = dict(goodm, **kw)
        assert lib.shf_leg_effort_mix(*[a[k] for k in MIX_NAMES]) != 0 and text in lib.shf_last_error()
    assert lib.shf_leg_effort_mix(*[dict(goodm, n=0)[k] for k in MIX_NAMES]) == 0


def test_gait_presets_and_tick_conversion():
    from shifu_amd.units.gait import PRESETS, Gait, GaitState
    assert Gait.trot().ticks(DT) == TROT and Gait.stand().ticks(DT) == STAND
    P, off, st = Gait.walk().ticks(DT)
    assert P == 120 and sorted(off) == [0, 30, 60, 90] and st == [90] * 4
    assert Gait.pace().ticks(DT)[1] == [0, 30, 0, 30] and Gait.bound().ticks(DT)[1] == [0, 0, 30, 30]
    assert set(PRESETS) == {"trot", "stand", "walk", "pace", "bound"}
    g = Gait.trot()
    assert (g.apex, g.late_depth, g.k_fb, g.max_step, g.leash, g.contact_threshold) == (0.06, 0.02, 0.18, 0.15, float("inf"), 1.0)
    with pytest.raises(ValueError, match="whole number"):
        Gait.trot(period_s=0.3).ticks(0.007)
    with pytest.raises(ValueError, match="whole number"):
        Gait.trot(period_s=0.001).ticks(DT)
    s = GaitState(5, 4, "cpu")
    assert s.tick.dtype == torch.int32 and s.sched.dtype == torch.uint8 and tuple(s.anchor.shape) == (5, 4, 3)
    assert tuple(s.target.shape) == (5, 13) and tuple(s.yaw.shape) == (5,)
    r = s.take_pending()
    assert r is not None and bool(r.all()) and s.take_pending() is None
    s.reset(torch.tensor([1, 3]))
    assert s.take_pending().tolist() == [0, 1, 0, 1, 0]


# ---------------------------------------------------------------------------------------------------------- schedule --
@pytest.mark.parametrize("ticks", [TROT, STAND, (120, [0, 60, 30, 90], [90] * 4), (7, [0, 3, 5, 6], [1, 7, 4, 6])])
def test_every_foot_stands_its_stance_ticks_per_period(ticks):
    P = G.params(DT)
    root, feet = _flat(3)
    st = G.new_state(3, 4)
    st["tick"][:] = [0, 17, -5]                                   # any start, a negative one included
    sched = []
    for _ in range(ticks[0]):
        sched.append(G.plan(st, root, feet, None, np.zeros((3, 3)), NOM, None, *ticks, P)["scheduled"])
    sched = np.array(sched)
    assert (sched.sum(0) == np.array(ticks[2])[None]).all()
    if ticks is TROT:
        assert (sched[..., 0] == sched[..., 3]).all() and (sched[..., 1] == sched[..., 2]).all()
        assert (sched[..., 0] != sched[..., 1]).all(), "the diagonal pairs alternate"
    if ticks is STAND:
        assert sched.all(), "Gait.stand() never lifts a foot"


def test_stance_is_the_schedule_gated_by_contact_and_phase_is_reported():
    P = G.params(DT)
    root, feet = _flat(2)
    st = _start(2, root, feet, P)
    cz = np.array([[5.0, 5.0, 0.5, 1.0], [0.0, 50.0, 50.0, 1.001]])
    o = G.plan(st, root, feet, cz, np.zeros((2, 3)), NOM, None, *TROT, P)
    assert o["scheduled"].tolist() == [[1, 0, 0, 1]] * 2
    assert o["stance"].tolist() == [[1, 0, 0, 0], [0, 0, 0, 1]], "contact z must exceed the threshold"
    assert np.allclose(o["phase"], [[1 / 60, 31 / 60, 31 / 60, 1 / 60]] * 2)
    st2 = _start(2, root, feet, P)
    assert (G.plan(st2, root, feet, None, np.zeros((2, 3)), NOM, None, *TROT, P)["stance"] == o["scheduled"]).all()


# ------------------------------------------------------------------------------------------------------------- swing --
def _one_swing(P, cmd=(0.3, 0.0, 0.0), v=(0.3, 0.0)):
    """Foot 1's whole swing of a trot on a base that does not move (so hip and foothold stay put): the per-tick outputs."""
    root, feet = _flat(1, v=v)
    feet[0, 1] += [0.02, -0.01, 0.0]                               # the foot lifts off from somewhere else than its nominal place
    st = _start(1, root, feet, P)
    st["tick"][:] = 0
    outs = [G.plan(st, root, feet, None, np.array([cmd]), NOM, None, *TROT, P) for _ in range(30)]
    return root, feet, st, outs


def test_swing_starts_at_lift_off_and_ends_exactly_on_the_foothold():
    P = G.params(DT, as_float32=False)
    root, feet, st, outs = _one_swing(P)
    assert all(o["scheduled"][0].tolist() == [1, 0, 0, 1] for o in outs)
    y = np.array([o["world_target"][0, 1] for o in outs])
    fh = outs[-1]["foothold"][0, 1]
    assert (y[-1, :2] == fh).all() and y[-1, 2] == P["touchdown_z"], "the last target is (foothold, touchdown_z) exactly"
    # one tick's motion: the swing covers |foothold - lift-off| in 30 ticks with a peak blend rate of 1.5, and climbs at most
    # 4 apex / 30 per tick
    span = np.linalg.norm(fh - feet[0, 1, :2]) + abs(P["touchdown_z"] - feet[0, 1, 2])
    assert np.linalg.norm(y[0] - feet[0, 1]) <= 1.5 * span / 30 + 4 * P["apex"] / 30
    assert np.linalg.norm(y[0] - feet[0, 1]) > 0
    # the base-frame output is R^T (y - p)
    assert np.allclose(outs[3]["swing_target"][0, 1], y[3] - root[0, :3], atol=1e-15)
    # the next tick is the scheduled touchdown: the anchor becomes the foothold, late_depth below touchdown_z
    o = G.plan(st, root, feet, np.zeros((1, 4)), np.array([[0.3, 0.0, 0.0]]), NOM, None, *TROT, P)
    assert o["scheduled"][0].tolist() == [0, 1, 1, 0]
    assert np.allclose(st["anchor"][0, 1], [*o["foothold"][0, 1], P["touchdown_z"] - P["late_depth"]], atol=0)
    assert (o["world_target"][0, 1] == st["anchor"][0, 1]).all(), "a late foot's target is its anchor"
    assert (st["anchor"][0, 0] == feet[0, 0]).all(), "lift-off anchors the foot where it is"


def test_swing_apex_above_the_chord():
    P = G.params(DT, as_float32=False)
    _, feet, _, outs = _one_swing(P)
    u = np.arange(1, 31) / 30.0
    b = u * u * (3 - 2 * u)
    chord = (1 - b) * feet[0, 1, 2] + b * P["touchdown_z"]
    above = np.array([o["world_target"][0, 1, 2] for o in outs]) - chord
    assert abs(above.max() - P["apex"]) <= 1e-15 and np.argmax(above) == 14 and (above >= -1e-15).all()


def test_foothold_is_half_a_stance_ahead_of_the_hip_and_feedback_shifts_it():
    P = G.params(DT, as_float32=False)
    for yaw in (0.0, 0.7, -2.0):
        c, s = np.cos(yaw), np.sin(yaw)
        vw = np.array([c * 0.3 - s * 0.1, s * 0.3 + c * 0.1])
        root, feet = _flat(1, yaw=yaw, v=vw)
        st = _start(1, root, feet, P)
        o = G.plan(st, root, feet, None, np.array([[0.3, 0.1, 0.0]]), NOM, None, *TROT, P)
        hip = feet[0, :, :2]
        assert np.allclose(o["foothold"][0] - hip, vw * (30 * DT) / 2, atol=1e-15)
        dv = np.array([0.2, -0.1])
        root2 = root.copy()
        root2[:, 7:9] += dv
        st = _start(1, root2, feet, P)
        o2 = G.plan(st, root2, feet, None, np.array([[0.3, 0.1, 0.0]]), NOM, None, *TROT, P)
        assert np.allclose(o2["foothold"] - o["foothold"], P["k_fb"] * dv, atol=1e-15)


def test_max_step_and_leash_bind_only_when_exceeded():
    root, feet = _flat(1, v=(0.0, 0.0))
    hip = feet[0, :, :2]
    for vx, binds in ((1.0, False), (3.0, True)):                 # |v T_st / 2 + k_fb (0 - v)| = |v| (0.075 - 0.18): 0.105, 0.315
        P = G.params(DT, as_float32=False)
        st = _start(1, root, feet, P)
        o = G.plan(st, root, feet, None, np.array([[vx, 0.0, 0.0]]), NOM, None, *TROT, P)
        step = o["foothold"][0] - hip
        free = vx * (0.075 - 0.18)
        if binds:
            assert np.allclose(np.linalg.norm(step, axis=1), P["max_step"], atol=1e-15) and (step[:, 0] < 0).all()
        else:
            assert np.allclose(step[:, 0], free, atol=1e-15) and abs(free) < P["max_step"]
    # the leash: the base stays put, the target runs away at 1 m/s
    for leash, n_free in ((np.inf, 10 ** 9), (0.05, 10)):
        P = G.params(DT, leash=leash, as_float32=False)
        st = _start(1, root, feet, P)
        for k in range(1, 40):
            G.plan(st, root, feet, None, np.array([[1.0, 0.0, 0.0]]), NOM, None, *TROT, P)
            d = st["target"][0, 0] - root[0, 0]
            assert np.isclose(d, k * DT if k <= n_free else leash, atol=1e-12), (leash, k, d)
            assert st["target"][0, 1] == 0.0


def test_yaw_rate_moves_the_footholds_tangentially():
    P = G.params(DT, as_float32=False)
    root, feet = _flat(1)
    st = _start(1, root, feet, P)
    o = G.plan(st, root, feet, None, np.array([[0.0, 0.0, 1.0]]), NOM, None, *TROT, P)
    step = o["foothold"][0] - feet[0, :, :2]
    want = np.stack([-NOM[:, 1], NOM[:, 0]], 1) * (30 * DT) / 2    # z x r, half a stance of it
    assert np.allclose(step, want, atol=1e-15)
    assert (np.sign(step[:, 0]) == -np.sign(NOM[:, 1])).all() and (np.sign(step[:, 1]) == np.sign(NOM[:, 0])).all()
    assert np.isclose(st["yaw"][0], DT) and np.allclose(st["target"][0, 3:7], [0, 0, np.sin(DT / 2), np.cos(DT / 2)])
    assert st["target"][0, 12] == 1.0


def test_reset_restores_the_documented_state():
    P = G.params(DT, as_float32=False)
    rng = np.random.default_rng(5)
    X = G.seeded_inputs(6, rng)
    st = G.new_state(6, 4)
    st["tick"][:], st["sched"][:] = 37, 0
    st["anchor"][:], st["target"][:], st["yaw"][:] = 9.0, 7.0, 2.0
    reset = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    before = {k: v.copy() for k, v in st.items()}
    o = G.plan(st, X["root"], X["feet"], X["contact"], np.zeros((6, 3)), NOM, reset, *TROT, P)
    r = reset.astype(bool)
    q = X["root"][:, 3:7]
    R = G.rotation(q)
    heading = np.arctan2(R[:, 1, 0], R[:, 0, 0])
    assert (st["tick"][r] == 1).all() and (st["tick"][~r] == 38).all()
    assert (o["scheduled"][r] == [1, 0, 0, 1]).all(), "the clock restarts at the top of the period"
    assert np.allclose(st["yaw"][r], heading[r], atol=1e-15) and (st["yaw"][~r] == before["yaw"][~r]).all()
    assert np.allclose(st["target"][r, :3], np.c_[X["root"][r, :2], np.full(r.sum(), P["height"])], atol=0)
    assert np.allclose(st["target"][r, 3:7], np.c_[np.zeros((r.sum(), 2)), np.sin(heading[r] / 2), np.cos(heading[r] / 2)], atol=1e-15)
    assert (st["target"][r, 7:] == 0).all()
    # feet 0 and 3 stand on, anchored under themselves; feet 1 and 2 lift off on this very tick, from where they are
    under = np.concatenate([X["feet"][..., :2], np.full((6, 4, 1), P["touchdown_z"] - P["late_depth"])], -1)
    assert (st["anchor"][r][:, [0, 3]] == under[r][:, [0, 3]]).all() and (st["anchor"][r][:, [1, 2]] == X["feet"][r][:, [1, 2]]).all()


# ----------------------------------------------------------------------------------------------------- torch fallback --
def test_torch_fallback_equals_the_twin_over_200_ticks():
    from shifu_amd.units.gait import Gait, GaitState
    from shifu_amd.utils import torch_utils as TU
    rng = np.random.default_rng(11)
    n = 33
    gait = Gait.trot(leash=0.3)
    ticks = gait.ticks(DT)
    P = G.params(DT, leash=0.3, as_float32=False)
    st, ts = G.new_state(n, 4), GaitState(n, 4, "cpu", torch.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    worst, lifted, late = 0.0, 0, 0
    for k in range(200):
        X = G.seeded_inputs(n, rng)
        if k == 0:
            X["reset"][:] = 1
        if k == 1:                                                # per-env different phases from here on
            st["tick"][:] = np.arange(n)
            ts.tick.copy_(torch.arange(n, dtype=torch.int32))
        cz = None if k % 7 == 3 else X["contact"]
        o = G.plan(st, X["root"], X["feet"], cz, X["command"], NOM, X["reset"], *ticks, P)
        s, sw, ph, ex = TU.gait_plan(ts, t(X["root"]), t(X["feet"]), None if cz is None else t(cz), t(X["command"]), t(NOM), t(X["reset"]),
                                     ticks, DT, 0.30, gait.apex, 0.01, gait.late_depth, gait.k_fb, gait.max_step, gait.leash,
                                     gait.contact_threshold)
        assert (s.numpy() == o["stance"]).all() and (ts.tick.numpy() == st["tick"]).all() and (ts.sched.numpy() == st["sched"]).all()
        for a, b in ((sw, o["swing_target"]), (ph, o["phase"]), (ts.target, st["target"]), (ts.anchor, st["anchor"]), (ts.yaw, st["yaw"]),
                     (ex["foothold"], o["foothold"]), (ex["world_target"], o["world_target"])):
            worst = max(worst, float(np.abs(a.numpy() - b).max()))
        lifted += int((o["scheduled"] == 0).sum())
        late += int(((o["scheduled"] == 1) & (o["stance"] == 0)).sum())
    assert worst <= 1e-9, worst
    assert lifted > 1000 and late > 100, "swinging and late feet both occur"


# --------------------------------------------------------------------------------------------------------------- mix --
def test_mix_equals_its_closed_form():
    from shifu_amd.utils import torch_utils as TU
    rng = np.random.default_rng(2)
    n, nd = 50, 12
    a, b = rng.normal(0, 20, (n, nd)).astype(np.float32), rng.normal(0, 20, (n, nd)).astype(np.float32)
    stance = (rng.uniform(size=(n, 4)) < 0.5).astype(np.uint8)
    chain = np.zeros((4, nd), np.uint8)
    for f in range(4):
        chain[f, 3 * f:3 * f + 3] = 1
    limit = np.full(nd, 15.0, np.float32)
    limit[2], limit[7] = 0.0, -1.0                                # no limit on these two
    want = a + np.repeat(1.0 - stance.astype(np.float32), 3, axis=1) * b
    capped = np.clip(want, -15.0, 15.0)
    capped[:, [2, 7]] = want[:, [2, 7]]
    assert (np.abs(want) > 15.0).any() and (np.abs(want[:, [2, 7]]) > 15.0).any()
    got = G.mix(a, b, stance, chain, limit)
    assert got.dtype == np.float32 and np.array_equal(got, capped)
    assert np.array_equal(G.mix(a, b, stance, chain, None), want)
    t = lambda x: torch.from_numpy(x)
    assert np.array_equal(TU.leg_effort_mix(t(a), t(b), t(stance), t(chain), t(limit)).numpy(), capped)
    assert np.array_equal(TU.leg_effort_mix(t(a), t(b), t(stance), t(chain)).numpy(), want)
    # a dof shared by two feet's chains moves with either of them
    chain2 = chain.copy()
    chain2[1, 0] = 1
    st = np.array([[1, 0, 1, 1]], np.uint8)
    assert G.mix(a[:1], b[:1], st, chain2)[0, 0] == a[0, 0] + b[0, 0] and G.mix(a[:1], b[:1], st, chain)[0, 0] == a[0, 0]


def test_nominal_foot_positions_and_chain_mask_of_the_a1():
    from shifu_amd.units import gait as UG
    from tests import balance_cpu as B
    from tests import helpers as H
    from tests import trot_cpu as T
    m = H.a1_model().blob
    assert np.allclose(UG.nominal_foot_positions(m, B.STAND_Q, list(B.FEET)), B.swing_targets(m), atol=1e-12)
    assert np.array_equal(UG.chain_mask(m, list(B.FEET)).numpy(), T.chain_mask(m)) and T.chain_mask(m).sum() == 12
    assert UG.foot_radius(m, list(B.FEET)) == T.foot_radius(m) > 0
