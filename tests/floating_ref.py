"""Float64 references for the floating-base dynamics tensors (csrc/shf_dyn.h: shf_sim_floating_dynamics) and the foot
controller (shf_foot_impedance), built on tests/helpers.forward_kinematics / newton_euler / mechanical_state: classical
vectors, nothing shared with the kernels' spatial algebra.

Order of the generalised velocity: nu = (v, w, qd), v the world velocity of the root origin, w the root's world angular
velocity, qd the dof velocities."""
import copy

import numpy as np

from shifu_amd import _abi
from tests import helpers as H


def scaled(m, s):
    """A copy of model m whose masses and inertia tensors carry the per-body factors s."""
    m2 = copy.deepcopy(m)
    for b in range(m.nb):
        m2.mass[b] = float(m.mass[b]) * float(s[b])
        for k in range(6):
            m2.inertia[b][k] = float(m.inertia[b][k]) * float(s[b])
    return m2


def skew(r):
    return np.array([[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]])


def jacobian(m, q, root_pos, root_quat):
    """(nb, 6, nd + 6): rows [velocity of the body's origin; angular velocity] per unit nu, from forward_kinematics."""
    R, p, aw = H.forward_kinematics(m, q, root_pos, root_quat)
    D = m.nd + 6
    J = np.zeros((m.nb, 6, D))
    for b in range(m.nb):
        J[b, :3, :3] = np.eye(3)
        J[b, :3, 3:6] = -skew(p[b] - p[0])
        J[b, 3:, 3:6] = np.eye(3)
        a = b
        while a > 0:
            if m.jtype[a] == _abi.JOINT_REVOLUTE:
                d = m.dof[a]
                J[b, :3, 6 + d] = np.cross(aw[a], p[b] - p[a])
                J[b, 3:, 6 + d] = aw[a]
            elif m.jtype[a] == _abi.JOINT_PRISMATIC:
                J[b, :3, 6 + m.dof[a]] = aw[a]
            a = m.parent[a]
    return J


def chain_mask(m):
    """(nb, nd + 6) bool: the columns that may be non-zero in body b's block (base columns and the dofs of its chain)."""
    mask = np.zeros((m.nb, m.nd + 6), bool)
    mask[:, :6] = True
    for b in range(m.nb):
        a = b
        while a > 0:
            if m.dof[a] >= 0:
                mask[b, 6 + m.dof[a]] = True
            a = m.parent[a]
    return mask


def mass_and_bias(m, q, qd, root_pos, root_quat, root_lin, root_ang, gravity):
    """(M_ref (nd+6, nd+6), h_ref (nd+6)): M column by column from newton_euler with zero velocities, zero gravity and unit
    accelerations (root_lin_acc, root_ang_acc, qdd) plus the armature; h = (f0, n0, tau) with all accelerations zero."""
    nd = m.nd
    D = nd + 6
    z3, zd = np.zeros(3), np.zeros(nd)
    M = np.zeros((D, D))
    for j in range(D):
        e = np.zeros(D)
        e[j] = 1.0
        tau, f0, n0 = H.newton_euler(m, q, zd, e[6:], root_pos, root_quat, z3, z3, e[:3], e[3:6], (0.0, 0.0, 0.0))
        M[:, j] = np.concatenate([f0, n0, tau])
    M[6:, 6:] += np.diag([m.armature[d] for d in range(nd)])
    tau, f0, n0 = H.newton_euler(m, q, qd, zd, root_pos, root_quat, root_lin, root_ang, z3, z3, gravity)
    return M, np.concatenate([f0, n0, tau])


def momentum_and_energy(m, q, qd, root_pos, root_quat, root_lin, root_ang):
    """(linear momentum, angular momentum about the root origin, kinetic energy) from mechanical_state without gravity (the
    model's armature is not part of it: compare on models without armature, or subtract it)."""
    E, P, L, _ = H.mechanical_state(m, q, qd, root_pos, root_quat, root_lin, root_ang, (0.0, 0.0, 0.0))
    return P, L - np.cross(np.asarray(root_pos, float), P), E


def foot_impedance(J, qd, root_pos, root_quat, foot_pos, target, kp3, kd3, bias=None, limit=None):
    """The closed form of shf_foot_impedance in float64, per env.  J (n, F, 6, nd + 6), qd (n, nd), root_pos (n, 3), root_quat
    (n, 4) xyzw, foot_pos / target (n, F, 3); returns (tau before the clamp, tau)."""
    J, qd, root_pos, root_quat, foot_pos, target = (np.asarray(a, np.float64) for a in (J, qd, root_pos, root_quat, foot_pos, target))
    kp3, kd3 = np.asarray(kp3, np.float64), np.asarray(kd3, np.float64)
    n, F = J.shape[:2]
    tau = np.zeros((n, J.shape[3] - 6))
    for e in range(n):
        R = H.quat_to_mat(root_quat[e])
        for f in range(F):
            Jl = J[e, f, :3, 6:]
            p = R.T @ (foot_pos[e, f] - root_pos[e])
            pd = R.T @ (Jl @ qd[e])
            tau[e] += Jl.T @ (R @ (kp3 * (target[e, f] - p) - kd3 * pd))
        if bias is not None:
            tau[e] += np.asarray(bias[e], np.float64)[6:]
    free = tau.copy()
    if limit is not None:
        lim = np.asarray(limit, np.float64)
        tau = np.where(lim > 0, np.clip(tau, -np.abs(lim), np.abs(lim)), tau)
    return free, tau
