"""The locomotion controller's closed loop on the CPU: the oracle's float32 step (oracle.pyoracle.step, TGS solver, 5 ms, plane,
friction 1) with the float64 twins as controller -- tests/gait_ref.plan (gait clock, footholds, swing targets, base target),
tests/qp_ref.twin on the plan's target and stance, tests/floating_ref.foot_impedance towards the swing targets (explicit
kp / kd, no bias), tests/gait_ref.mix -- on float64 J, M and h.  The GPU test (tests/test_gpu_gait.py) runs the same loop with
the kernels on a bare sim and is measured against this run's figures.

The scenario: the 8 A1s of tests/balance_cpu.initial_state, SETTLE ticks of Gait.stand() with a zero command, then the gait
clock set to 0 and TROT ticks of Gait.trot() at VX m/s.

`python -m tests.trot_cpu` prints the figures and rewrites tests/golden/trot_cpu.npz (per step and env: x, z, tilt; float32).
"""
import os

import numpy as np

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import floating_ref as FR
from tests import gait_ref as G
from tests import helpers as H
from tests import qp_ref as Q

N_ENVS, DT = B.N_ENVS, B.DT
SETTLE, TROT, VX = 100, 500, 0.3
PERIOD_S, DUTY, OFFSETS = 0.3, 0.5, (0.0, 0.5, 0.5, 0.0)           # Gait.trot()
SWING_KP, SWING_KD = 400.0, 10.0
TOUCHDOWN_DEPTH = 0.01                                              # a swing ends this far below the foot's resting height
PERIODS = 5                                                         # the mean speed is taken over the last five whole periods
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trot_cpu.npz")


def ticks(period_s, duty, offsets, dt=DT):
    """units.gait.Gait.ticks without torch: (period_ticks, offset_ticks, stance_ticks)."""
    P = int(round(period_s / dt))
    return P, [int(round(o * P)) % P for o in offsets], [min(P, max(1, int(round(duty * P))))] * len(offsets)


STAND_TICKS = ticks(PERIOD_S, 1.0, (0.0,) * 4)
TROT_TICKS = ticks(PERIOD_S, DUTY, OFFSETS)


def foot_radius(m):
    return max(float(m.pt_radius[i]) for i in range(m.np) if m.pt_body[i] in B.FEET)


def gait_params(m, **over):
    """The planner's scalars for the A1 on the plane: the defaults of units.gait.Gait, base height 0.30 m, a swing ending 1 cm
    below the foot's resting height."""
    return G.params(DT, height=B.HEIGHT, touchdown_z=foot_radius(m) - TOUCHDOWN_DEPTH, **over)


def chain_mask(m):
    """(4, nd) uint8: the dofs on the chain from the root to each foot."""
    mask = np.zeros((len(B.FEET), m.nd), np.uint8)
    for f, b in enumerate(B.FEET):
        while b > 0:
            if m.dof[b] >= 0:
                mask[f, m.dof[b]] = 1
            b = m.parent[b]
    return mask


def control(m, state, q, qd, root, feet_pos, contact_z, command, tk, P, swing_kp=SWING_KP, swing_kd=SWING_KD, reset=None, out=np.float32):
    """One control tick in float64 on float32 state: (efforts (n, nd) float32 -- what the simulator takes; `out` float64 keeps
    them as computed --, forces, stance, swing targets)."""
    n = q.shape[0]
    plan = G.plan(state, root, feet_pos, contact_z, command, B.swing_targets(m), reset, *tk, P)
    J, M, h = B.dynamics64(m, q, qd, root)
    w = Q.wrench(M, h, root, state["target"], B.gains12())
    rr = feet_pos.astype(np.float64) - root[:, None, :3].astype(np.float64)
    f = Q.twin(rr, w, B.WEIGHTS, B.ALPHA, 0.0, None, plan["stance"], B.MU, B.FZ_MIN, np.inf, Q.ITERS)
    limit = np.array([m.effort[d] for d in range(m.nd)])
    _, tau_st = Q.efforts(J, f, h, limit)
    _, tau_sw = FR.foot_impedance(J, qd, root[:, :3], root[:, 3:7], feet_pos, plan["swing_target"], np.full(3, swing_kp),
                                  np.full(3, swing_kd), None, limit)
    tau = G.mix(tau_st, tau_sw, plan["stance"], chain_mask(m), limit)
    return tau.astype(out), f, plan["stance"], plan["swing_target"]


def run(settle=SETTLE, trot=TROT, vx=VX, trot_ticks=TROT_TICKS, swing_kp=SWING_KP, swing_kd=SWING_KD, n=N_ENVS, verbose=False, **over):
    """The loop.  Returns {"x", "z", "tilt" (steps, n), "cone" (every stance force inside its cone), "finite"}."""
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
    P = gait_params(m, **over)
    state = G.new_state(n, 4)
    out = {k: [] for k in ("x", "z", "tilt")}
    cone, finite = True, True
    for s in range(settle + trot):
        d3 = dof.reshape(n, m.nd, 2)
        feet = B.feet_positions(m, d3[..., 0], root).astype(np.float32)
        if s == settle:
            state["tick"][:] = 0                 # the trot starts at the top of its period
        command = np.zeros((n, 3))
        command[:, 0] = vx if s >= settle else 0.0
        tau, f, stance, _ = control(m, state, d3[..., 0], d3[..., 1], root, feet, contact[:, list(B.FEET), 2], command,
                                    trot_ticks if s >= settle else STAND_TICKS, P, swing_kp, swing_kd,
                                    np.ones(n, np.uint8) if s == 0 else None)
        on = stance.astype(bool)
        cone = cone and bool((f[..., 2][on] >= B.FZ_MIN).all() and (f[~on] == 0).all()
                             and (np.abs(f[..., :2]) <= B.MU * f[..., 2:3] + 1e-12)[on].all())
        c, _ = pyoracle.step(m, p, n, dof, root, terrain=terr, effort=np.ascontiguousarray(tau), friction=fric, want_contact=True)
        contact = c.reshape(n, m.nb, 3)
        finite = finite and bool(np.isfinite(dof).all() and np.isfinite(root).all())
        out["x"].append(root[:, 0].copy()); out["z"].append(root[:, 2].copy()); out["tilt"].append(B.tilt_of(root[:, 3:7]))
        if verbose and s % 50 == 49:
            print(s, "z", np.round(root[:, 2], 3), "tilt", np.round(out["tilt"][-1], 3), "x", np.round(root[:, 0] - np.arange(n), 3), flush=True)
    res = {k: np.array(v) for k, v in out.items()}
    res["cone"], res["finite"] = cone, finite
    return res


def figures(x, z, tilt, settle=SETTLE, vx=VX, period_ticks=TROT_TICKS[0], dt=DT):
    """(peak tilt over the trot per env, lowest base z over the whole run per env, relative error of the mean speed over the
    last PERIODS whole periods per env)."""
    k = PERIODS * period_ticks
    speed = (x[-1] - x[-1 - k]) / (k * dt)
    return tilt[settle:].max(0), z.min(0), np.abs(speed - vx) / abs(vx)


if __name__ == "__main__":
    r = run(verbose=True)
    pt, zmin, es = figures(r["x"], r["z"], r["tilt"])
    print(f"[cpu] trot at {VX} m/s: peak tilt {pt.max():.4f} rad (per env {np.round(pt, 3)}), lowest base z {zmin.min():.4f} m, "
          f"speed error {es.max():.4f} of the command (per env {np.round(es, 3)}); advanced {np.round(r['x'][-1] - r['x'][SETTLE - 1], 3)}; "
          f"cones {r['cone']}, finite {r['finite']}")
    np.savez_compressed(GOLDEN, x=r["x"].astype(np.float32), z=r["z"].astype(np.float32), tilt=r["tilt"].astype(np.float32))
    print("wrote", GOLDEN)
