"""The contact tensor of the velocity-level solve (SHF_SOLVER_PGS / SHF_SOLVER_TGS; oracle/shf_oracle.c hard_solve) against
Newton's second law, at iteration counts away from the reference's 8 + 1.

The law: for a free body of mass m whose only loads are gravity and contacts, m ((v_after - v_before) / dt - g) is the body's
row of the contact tensor.  It is an identity of the time stepping, not a statement about convergence: whatever impulses the
sweeps end with, the velocities are advanced with one impulse set and the tensor reports impulses / dt -- of the same set, or
the law breaks.  With no velocity iterations under TGS the velocities take the MEAN of the position sub-iterations' impulses;
until this file existed the oracle (and csrc/shf_chain_hard.h) reported the final sweep's impulses there, which were never
applied: the block at rest showed 1.019 (pos_iters 8), 1.090 (3) and 1.137 (2) times its weight, and an impact step was off by
several times the weight (the figures per test below).  The rule now: the tensor reports the impulse set the velocities took.

Every test runs both solvers, the double and the float build of the oracle, and (pos_iters, vel_iters) in SETTINGS.  The bound on
the law's residual is 5e-6 of the body's weight in float64 and 1e-5 in float32: four times the largest residual of the settings
that never were in question (1.04e-6 / 2.45e-6: the contact tensor is float32 in both builds -- 3.4e-8 of the weight at rest,
more on an impact step that carries sixty times the weight), the factor for changes of summation order."""
import numpy as np
import pytest

from tests import kat_models as K
from tests.helpers import sim_params
from tests.test_hard_contact import PREC, SOLVERS, run_block

SETTINGS = [(8, 1), (8, 0), (3, 0), (2, 0), (1, 0), (1, 2), (4, 2), (12, 3)]
STEPS = 300
MASS = 2.0                                     # kat_models.block_model
# slope (tan theta), height of the block's centre over the plane, initial velocity
SCENARIOS = {"stick": (0.3, 0.05, (0.0, 0.0, 0.0)), "slide": (0.9, 0.05, (0.0, 0.0, 0.0)), "drop": (0.0, 0.35, (0.5, 0.0, 0.0))}


def _bound(f64):
    return 5e-6 if f64 else 1e-5


def _law_residual(v_before, v_after, force, mass, g, dt):
    """Largest component of m (dv / dt - g) - f over the steps, as a fraction of the body's weight (float64 arithmetic)."""
    v0, v1, f = np.asarray(v_before, np.float64), np.asarray(v_after, np.float64), np.asarray(force, np.float64)
    res = mass * ((v1 - v0) / dt - np.asarray(g, np.float64)) - f
    return float(np.abs(res).max() / (mass * K.G))


@pytest.mark.parametrize("scenario", list(SCENARIOS))
@pytest.mark.parametrize("pos_iters,vel_iters", SETTINGS)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("f64", PREC)
def test_block_contact_force_is_the_momentum_the_block_gained(oracle, f64, solver, pos_iters, vel_iters, scenario):
    """The 2 kg block sticking on a slope (tan 0.3), sliding on one (tan 0.9), and dropped from 0.3 m with 0.5 m/s sideways (the
    impact step carries about sixty times the weight): every one of 300 steps.

    Measured, largest residual over the three scenarios as a fraction of the weight -- before the rule, TGS with no velocity
    iterations: pos_iters 8: stick 3.6e-2, slide 1.9e-2, drop 1.5; 3: 1.0e-1, 6.2e-2, 5.4; 2: 1.4e-1, 8.6e-2, 7.2 (float64
    and float32 alike); every other setting as now.  Now, all sixteen solver / iteration settings: float64 <= 1.16e-6 (the drop's
    impact step; stick and slide <= 4.0e-8), float32 <= 2.45e-6."""
    tan, z0, lin = SCENARIOS[scenario]
    th = np.arctan(tan)
    tr, f = run_block(oracle, f64, th, 0.2, STEPS, lin=lin, z0=z0, solver=solver, pos_iters=pos_iters, vel_iters=vel_iters)
    v = np.vstack([np.asarray(lin, np.float64)[None], tr[:, 7:10].astype(np.float64)])
    # conditions on the inputs: the block is in contact (it carries load in most steps; the drop lands within 60)
    loaded = np.abs(f).max(1) > 0.0
    assert loaded.sum() >= (200 if scenario == "drop" else STEPS), loaded.sum()
    if scenario == "drop":
        assert not loaded[:40].any() and np.abs(f[:, 2]).max() > 20.0 * MASS * K.G, "free fall, then an impact"
    r = _law_residual(v[:-1], v[1:], f, MASS, (K.G * np.sin(th), 0.0, -K.G * np.cos(th)), K.DT)
    print(f"law residual / weight: {r:.3e}")
    assert r <= _bound(f64), r


def _push(oracle, f64, solver, pos_iters, vel_iters, yaw, steps=STEPS):
    """The pusher scene of tests/test_contact_kats.py under the velocity-level solve: the rail-mounted slider, driven at 0.5 m/s,
    shoves the free 0.5 kg cube over the ground with its capsule -- the cube is a solver body of its own (a box actor), the B side
    of the capsule's pair constraints and the A side of its corners' ground contacts."""
    from shifu_amd.abb_task import box_desc
    cm = K.pusher_model(yaw=yaw)
    m = cm.blob
    sp = sim_params(solver=solver, pos_iters=pos_iters, vel_iters=vel_iters)
    dt = np.float64 if f64 else np.float32
    cube = box_desc((0.1, 0.1, 0.1), 0.5, 0.6, False, (0.12, 0.0, 0.05))
    dof = np.zeros((1, 2), dt)
    root = np.zeros((2, 13), dt); root[:, 6] = 1.0
    root[1, :3] = (0.12, 0.0, 0.05)
    vt = np.full(1, 0.5, dt)
    fr = np.ones(1, np.float32)
    v0, v1, fc, fs = [], [], [], []
    for k in range(steps):
        v0.append(root[1, 7:10].copy())
        contact, _, _ = oracle.scene_step(m, sp, [cube], 1, dof, root, vel_target=vt, friction=fr, f64=f64)
        v1.append(root[1, 7:10].copy()); fc.append(contact[m.nb].copy()); fs.append(contact[m.nb - 1].copy())
    return np.array(v0), np.array(v1), np.array(fc), np.array(fs)


@pytest.mark.parametrize("yaw_deg", [0.0, 25.0])
@pytest.mark.parametrize("pos_iters,vel_iters", SETTINGS)
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("f64", PREC)
def test_pushed_cube_contact_force_is_the_momentum_the_cube_gained(oracle, f64, solver, pos_iters, vel_iters, yaw_deg):
    """A box actor as a solver body, taking impulses on the B side of a pair (the capsule along the cube's face: a line contact of
    two constraints; turned by 25 degrees: its end, off centre, which also turns the cube) and on the A side of its four ground
    corners: the cube's row of the contact tensor is the momentum it gained less gravity's, every step.

    Measured as a fraction of the cube's weight -- before the rule, TGS with no velocity iterations: pos_iters 8: 6.3 (0 degrees)
    and 2.7 (25 degrees); 3: 2.6, 2.7; 2: 1.8, 2.3.  Now, all settings: float64 <= 1.5e-7, float32 <= 2.6e-6."""
    v0, v1, fc, fs = _push(oracle, f64, solver, pos_iters, vel_iters, np.deg2rad(yaw_deg))
    # condition on the inputs: the two-sided pair is in play (the slider feels the cube) in at least 50 steps
    assert (np.abs(fs).max(1) > 0.0).sum() >= 50
    r = _law_residual(v0, v1, fc, 0.5, (0.0, 0.0, -K.G), K.DT)
    print(f"law residual / weight: {r:.3e}")
    assert r <= _bound(f64), r


# The settings under which the block on the slope of tan 0.3 comes to rest by the sticking tolerance of
# tests/test_hard_contact.py::test_block_sticks_below_the_friction_angle_without_creep (largest velocity component over the last
# 100 of 400 steps below 1e-6 / 2e-5 under PGS in float64 / float32, below 2.5e-3 under TGS).  The others creep faster than that:
# few sweeps leave the friction short of what holds the block -- PGS (3,0) 5e-4, (4,2) 4e-4, (2,0) 2e-3, (1,2) 3e-2, (1,0) 6e-2 m/s;
# TGS (8,0) 6e-3, (3,0) 2e-2, (2,0) 2e-2, (1,2) 3e-2, (1,0) 6e-2 m/s -- and the static force is not theirs to meet.
RESTING = {"pgs": [(8, 1), (8, 0), (12, 3)], "tgs": [(8, 1), (4, 2), (12, 3)]}


@pytest.mark.parametrize("solver,pos_iters,vel_iters", [(s, p, v) for s in SOLVERS for p, v in RESTING[s]])
@pytest.mark.parametrize("f64", PREC)
def test_resting_block_reports_its_weight(oracle, f64, solver, pos_iters, vel_iters):
    """At rest on the slope the contact force is gravity's opposite: f_z = m g cos(theta), f_x = -m g sin(theta), to 1e-3 of the
    weight (measured: 4e-6 at most), for the settings that hold the block still."""
    th = np.arctan(0.3)
    tr, f = run_block(oracle, f64, th, 0.2, 400, solver=solver, pos_iters=pos_iters, vel_iters=vel_iters)
    tol = 2.5e-3 if solver == "tgs" else (1e-6 if f64 else 2e-5)
    assert np.abs(tr[-100:, 7:13]).max() < tol, "condition on the inputs: the setting holds the block still"
    w = MASS * K.G
    assert abs(f[-1, 2] - w * np.cos(th)) < 1e-3 * w and abs(f[-1, 0] + w * np.sin(th)) < 1e-3 * w and abs(f[-1, 1]) < 1e-3 * w, f[-1]


@pytest.mark.parametrize("pos_iters,vel_iters", [(8, 0), (3, 0)])
@pytest.mark.parametrize("solver", SOLVERS)
def test_independent_solver_takes_the_same_impulse_set(oracle, solver, pos_iters, vel_iters):
    """oracle/hard_contact_ref.py (joint-space inertia matrix, dense Delassus matrix) one step at a time from the oracle's states,
    the A1 trotting open loop for 60 sub-steps: the same joint velocities and the same total normal force when
    there are no velocity iterations -- under TGS both advance the velocities with the mean of the sub-iterations' impulses and
    report that set.  (Which set the velocities take there is the oracle's convention, which the other solver was changed to: as
    first written it took the final sweep's.  So under TGS this case checks the arithmetic of the convention with different
    building blocks, not the choice; the tests above pin that the tensor reports what the velocities took.)  Bounds: the joint positions to 1e-9 rad per sub-step, as tests/test_hard_contact.py holds the two to at
    8 + 1; the joint velocities to that over dt, 2e-7 rad/s (measured: 7e-9); the force to 1e-6 of the weight (measured: 4e-9)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import model_gap as G
    from oracle.hard_contact_ref import HardContactStepper
    cm, sp = G.a1_setup(solver)
    sp.pos_iters, sp.vel_iters = pos_iters, vel_iters
    m = cm.blob
    ref = HardContactStepper(m, sp, mu=1.0, sweeps=(pos_iters, vel_iters), tgs=solver == "tgs")
    dof = np.zeros((m.nd, 2)); dof[:, 0] = G.A1_Q0
    root = np.zeros((1, 13)); root[0, 2] = 0.33; root[0, 6] = 1.0
    weight = sum(m.mass[b] for b in range(m.nb)) * K.G
    dq = dqd = df = fmax = 0.0
    for k in range(60):
        tgt = G.a1_targets("trot", k, sp.dt)
        tau = G.KP * (tgt - dof[:, 0]) - G.KD * dof[:, 1]
        ql, qdl, rl = dof[:, 0].copy(), dof[:, 1].copy(), root[0].copy()
        fz = ref.step(ql, qdl, rl, tau.copy())
        c, _ = oracle.step(m, sp, 1, dof, root, effort=np.ascontiguousarray(tau, np.float64), friction=np.ones(1, np.float32), f64=True,
                           want_contact=True)
        dq, dqd = max(dq, np.abs(ql - dof[:, 0]).max()), max(dqd, np.abs(qdl - dof[:, 1]).max())
        df, fmax = max(df, abs(fz - c[:, 2].sum()) / weight), max(fmax, c[:, 2].sum() / weight)
    assert fmax > 0.5, "condition on the inputs: the feet carry the robot"
    assert dq < 1e-9 and dqd < 2e-7 and df < 1e-6, (dq, dqd, df)
