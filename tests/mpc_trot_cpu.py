"""The locomotion controller's closed loop on the CPU with the horizon MPC in place of the QP: the scenario and the loop of
tests/trot_cpu.py (the same 8 robots, the settle phase, then a trot at 0.3 m/s through oracle.pyoracle.step), the float64 twins
as controller, tests/mpc_ref.horizon + twin where trot_cpu.control calls tests/qp_ref.twin.  As glue.locomotion_control does, the
MPC is solved every `every` ticks (and on the first), warm-started from its last solution shifted by every // S steps, and its
forces are held on the current Jacobian in between (a foot that has lifted since counts as zero).

`python -m tests.mpc_trot_cpu` prints the figures at the default interval (a solve every tick) and at 2, 3 and 6 ticks -- the
prototype runs that made a solve every tick the default: with forces held for even one more tick the robots fall (DESIGN.md
8h "Horizon MPC") -- and for Gait.walk() at 0.15 m/s under the QP and under the MPC, and rewrites tests/golden/mpc_trot_cpu.npz
(per step and env: x, z, tilt of the default run; float32).
"""
import os

import numpy as np

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import floating_ref as FR
from tests import gait_ref as G
from tests import helpers as H
from tests import mpc_ref as R
from tests import qp_ref as Q
from tests import trot_cpu as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpc_trot_cpu.npz")
WALK_TICKS = T.ticks(0.6, 0.75, (0.0, 0.5, 0.25, 0.75))            # Gait.walk()
WALK_VX, WALK_STEPS = 0.15, 600
# what the QP trot is held to in tests/test_gpu_gait.py (test_the_a1_trots_at_the_commanded_speed: literals there): the CPU run's
# peak tilt and speed error below these, the base above z_min at every step
BOUNDS = {"tilt": 0.3, "speed": 0.2, "z_min": 0.2}
# python -m tests.mpc_trot_cpu: (peak tilt rad, lowest base z m, speed error) of the trot, per `every`
CPU_FIGURES = {1: (0.01406, 0.29437, 0.010678)}


def steps_per_tick(tk, horizon=R.HORIZON):
    return -(-tk[0] // horizon)


def control(m, state, mpc, q, qd, root, feet_pos, contact_z, command, tk, P, every, reset=None, horizon=R.HORIZON, iters=R.ITERS,
            out=np.float32):
    """One control tick in float64 on float32 state, as trot_cpu.control: (efforts float32 or `out`, forces, stance, swing
    targets).  mpc: the dict {"u", "forces", "count"} kept between ticks (empty at the start).  As glue.locomotion_control, a
    reset makes everybody solve on this tick and the reset envs start cold (a zero warm start is a cold start)."""
    plan = G.plan(state, root, feet_pos, contact_z, command, B.swing_targets(m), reset, *tk, P)
    J, M, h = B.dynamics64(m, q, qd, root)
    limit = np.array([m.effort[d] for d in range(m.nd)])
    S = steps_per_tick(tk, horizon)
    if "u" not in mpc or mpc.get("tk") != tk:
        mpc.update(u=None, count=0, tk=tk)
    if reset is not None:
        mpc.update(u=None if mpc["u"] is None else mpc["u"] * (np.asarray(reset) == 0)[:, None, None, None], count=0)
    if mpc["count"] % every == 0:
        contact, xref, pos = R.horizon(state["tick"], state["target"], state["yaw"], *tk, plan["stance"], feet_pos, command,
                                       B.swing_targets(m), P, horizon, S)
        prob = R.problem(contact, xref, pos, root, M, h, float(np.float32(S) * np.float32(P["dt"])))
        mpc["u"] = R.twin(prob, B.MU, R.WEIGHTS12, R.ALPHA, B.FZ_MIN, np.inf, iters, u0=mpc["u"], warm_shift=every // S)
        mpc["forces"] = mpc["u"][:, 0]
    mpc["count"] += 1
    f = mpc["forces"] * (plan["stance"] != 0)[..., None]
    _, tau_st = Q.efforts(J, f, h, limit)
    _, tau_sw = FR.foot_impedance(J, qd, root[:, :3], root[:, 3:7], feet_pos, plan["swing_target"], np.full(3, T.SWING_KP),
                                  np.full(3, T.SWING_KD), None, limit)
    tau = G.mix(tau_st, tau_sw, plan["stance"], T.chain_mask(m), limit)
    return tau.astype(out), f, plan["stance"], plan["swing_target"]


def run(every=R.EVERY, controller="mpc", settle=T.SETTLE, trot=T.TROT, vx=T.VX, trot_ticks=T.TROT_TICKS, n=T.N_ENVS, verbose=False):
    """trot_cpu.run with the stance forces from `controller` ("mpc" or "qp"): {"x", "z", "tilt" (steps, n), "cone", "finite"}."""
    from oracle import pyoracle
    pyoracle.build()
    m = H.a1_model().blob
    p = B.params()
    q, qd, root, _ = B.initial_state(m)
    q, qd, root = q[:n], qd[:n], root[:n]
    dof = np.ascontiguousarray(np.stack([q, qd], -1).reshape(n * m.nd, 2))
    root = np.ascontiguousarray(root)
    terr = _abi.ShfTerrain()
    terr.rows = terr.cols = 0
    terr.hscale = terr.vscale = 1.0
    terr.friction, terr.nz_min = 1.0, 0.99
    fric = np.ones(n, np.float32)
    contact = np.zeros((n, m.nb, 3), np.float32)
    P = T.gait_params(m)
    state, mpc = G.new_state(n, 4), {}
    out = {k: [] for k in ("x", "z", "tilt")}
    cone, finite = True, True
    for s in range(settle + trot):
        d3 = dof.reshape(n, m.nd, 2)
        feet = B.feet_positions(m, d3[..., 0], root).astype(np.float32)
        if s == settle:
            state["tick"][:] = 0
        command = np.zeros((n, 3))
        command[:, 0] = vx if s >= settle else 0.0
        tk = trot_ticks if s >= settle else T.STAND_TICKS
        reset = np.ones(n, np.uint8) if s == 0 else None
        cz = contact[:, list(B.FEET), 2]
        if controller == "mpc":
            tau, f, stance, _ = control(m, state, mpc, d3[..., 0], d3[..., 1], root, feet, cz, command, tk, P, every, reset)
        else:
            tau, f, stance, _ = T.control(m, state, d3[..., 0], d3[..., 1], root, feet, cz, command, tk, P, reset=reset)
        on = stance.astype(bool)
        if controller == "mpc" and (mpc["count"] - 1) % every != 0:
            on = on & False                      # held forces stood on the solve's stance: the cones are checked on the ticks with a solve
            f = f * 0.0
        cone = cone and bool((f[..., 2][on] >= B.FZ_MIN).all() and (f[~on] == 0).all()
                             and (np.abs(f[..., :2]) <= B.MU * f[..., 2:3] + 1e-12)[on].all())
        c, _ = pyoracle.step(m, p, n, dof, root, terrain=terr, effort=np.ascontiguousarray(tau), friction=fric, want_contact=True)
        contact = c.reshape(n, m.nb, 3)
        finite = finite and bool(np.isfinite(dof).all() and np.isfinite(root).all())
        out["x"].append(root[:, 0].copy()); out["z"].append(root[:, 2].copy()); out["tilt"].append(B.tilt_of(root[:, 3:7]))
        if verbose and s % 100 == 99:
            print(s, "z", np.round(root[:, 2], 3), "tilt", np.round(out["tilt"][-1], 3), "x", np.round(root[:, 0] - np.arange(n), 3), flush=True)
    res = {k: np.array(v) for k, v in out.items()}
    res["cone"], res["finite"] = cone, finite
    return res


def report(name, r, vx=T.VX, period_ticks=T.TROT_TICKS[0]):
    pt, zmin, es = T.figures(r["x"], r["z"], r["tilt"], vx=vx, period_ticks=period_ticks)
    print(f"[cpu] {name}: peak tilt {pt.max():.4f} rad, lowest base z {zmin.min():.4f} m, speed error {es.max():.4f} of the command; "
          f"cones {r['cone']}, finite {r['finite']}", flush=True)
    return float(pt.max()), float(zmin.min()), float(es.max())


if __name__ == "__main__":
    for every in (R.EVERY, 2, 3, 6):
        r = run(every)
        report(f"MPC trot at {T.VX} m/s, a solve every {every} tick(s)", r)
        if every == R.EVERY:
            np.savez_compressed(GOLDEN, x=r["x"].astype(np.float32), z=r["z"].astype(np.float32), tilt=r["tilt"].astype(np.float32))
            print("wrote", GOLDEN)
    for controller in ("qp", "mpc"):
        r = run(R.EVERY, controller, trot=WALK_STEPS, vx=WALK_VX, trot_ticks=WALK_TICKS)
        report(f"walk at {WALK_VX} m/s under the {controller}", r, WALK_VX, WALK_TICKS[0])
