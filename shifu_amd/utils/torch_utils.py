"""Quaternion / IK helpers (reference shifu/utils/torch_utils.py:4-58), xyzw order."""
import torch

from shifu_amd.isaacgym.torch_utils import quat_conjugate, quat_mul  # same formulas (:12-40)


def free_tensor_attrs(obj):
    """Drop tensor attributes so device memory can be reclaimed (:4-9)."""
    for name in list(vars(obj).keys()):
        if isinstance(getattr(obj, name, None), torch.Tensor):
            delattr(obj, name)
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def orientation_error(desired, current):
    q_r = quat_mul(desired, quat_conjugate(current))
    return q_r[:, 0:3] * torch.sign(q_r[:, 3]).unsqueeze(-1)


def inverse_kinematics(dof_pos, ee_pos, ee_quat, tar_pos, tar_quat, j_ee, device, damping=0.05):
    """Damped least squares: dq = J^T (J J^T + lambda^2 I)^-1 dpose (:43-58)."""
    dpose = torch.cat([tar_pos - ee_pos, orientation_error(tar_quat, ee_quat)], -1).unsqueeze(-1)
    jt = torch.transpose(j_ee, 1, 2)
    lam = torch.eye(6, device=device) * (damping ** 2)
    u = (jt @ torch.inverse(j_ee @ jt + lam) @ dpose).view(dof_pos.shape[0], dof_pos.shape[1])
    return dof_pos + u


def _effort_clamp(tau, effort_limit):
    """tau clamped to +-effort_limit (entries <= 0: no limit; None: no clamp)."""
    if effort_limit is None:
        return tau
    lim = torch.where(effort_limit > 0, effort_limit, torch.full_like(effort_limit, float("inf")))
    return torch.maximum(torch.minimum(tau, lim), -lim)


def wrap_to_pi(x):
    return x - 2.0 * torch.pi * torch.round(x / (2.0 * torch.pi))


def operational_space_control(j_ee, mass_matrix, dof_pos, dof_vel, ee_pos, ee_quat, tar_pos, tar_quat, kp6, kd6, damping=0.0,
                              bias=None, q_rest=None, kp_null=0.0, kd_null=0.0, effort_limit=None):
    """Operational-space (torque) control, the controller of Isaac Gym's arm examples: tau = J^T A^-1 (kp e - kd J qd) with
    A = J M^-1 J^T + damping^2 I (symmetrised); with q_rest and more than 6 dofs the null-space posture term
    M u - J^T A^-1 J u, u = kp_null wrap_to_pi(q_rest - q) - kd_null qd; then + bias, then the clamp to +-effort_limit
    (entries <= 0: no limit).  The torch expressions of csrc/shf_glue.hip's shf_osc (which solves by LDL^T)."""
    n, nd = dof_pos.shape
    e = torch.cat([tar_pos - ee_pos, orientation_error(tar_quat, ee_quat)], -1)
    a = kp6 * e - kd6 * (j_ee @ dof_vel.unsqueeze(-1)).squeeze(-1)
    jt = torch.transpose(j_ee, 1, 2)
    x = torch.linalg.solve(mass_matrix, jt)
    A = j_ee @ x
    A = 0.5 * (A + torch.transpose(A, 1, 2)) + torch.eye(6, device=j_ee.device, dtype=j_ee.dtype) * (damping ** 2)
    tau = (jt @ torch.linalg.solve(A, a.unsqueeze(-1))).squeeze(-1)
    if q_rest is not None and nd > 6:
        u = (kp_null * wrap_to_pi(q_rest - dof_pos) - kd_null * dof_vel).unsqueeze(-1)
        tau = tau + (mass_matrix @ u - jt @ torch.linalg.solve(A, j_ee @ u)).squeeze(-1)
    if bias is not None:
        tau = tau + bias
    return _effort_clamp(tau, effort_limit)


def quat_to_matrix(q):
    """(n, 4) xyzw -> (n, 3, 3)."""
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).view(-1, 3, 3)


def foot_impedance_control(j_feet, dof_vel, root_pos, root_quat, foot_pos, target, kp3, kd3, bias=None, effort_limit=None):
    """Cartesian foot control in the base frame.  j_feet (n, F, 6, nd + 6): the foot rows of the floating-base Jacobian; with
    R the root's rotation and Jl = j_feet[:, f, :3, 6:] (the foot's velocity relative to the base per unit dof velocity):
    p = R^T (p_foot - p_root), pd = R^T (Jl qd), F = R (kp3 (p_target - p) - kd3 pd), tau = sum over feet of Jl^T F; then
    + bias[:, 6:], then the clamp to +-effort_limit (entries <= 0: no limit).  The torch expressions of csrc/shf_glue.hip's
    shf_foot_impedance."""
    R = quat_to_matrix(root_quat).unsqueeze(1)                      # (n, 1, 3, 3)
    Rt = torch.transpose(R, 2, 3)
    jl = j_feet[:, :, :3, 6:]                                       # (n, F, 3, nd)
    p = (Rt @ (foot_pos - root_pos.unsqueeze(1)).unsqueeze(-1)).squeeze(-1)
    pd = (Rt @ (jl @ dof_vel.unsqueeze(1).unsqueeze(-1))).squeeze(-1)
    f = (R @ (kp3 * (target - p) - kd3 * pd).unsqueeze(-1))         # (n, F, 3, 1)
    tau = (torch.transpose(jl, 2, 3) @ f).squeeze(-1).sum(1)
    if bias is not None:
        tau = tau + bias[:, 6:]
    return _effort_clamp(tau, effort_limit)


def balance_wrench(mass_matrix, bias, root_state, base_target, gains12):
    """The base wrench (n, 6) the balance controller asks the feet for: w = M[0:6, 0:6] (a_lin, a_ang) + h[0:6] with
    a_lin = kp_lin (p* - p) + kd_lin (v* - v), a_ang = kp_ang orientation_error(q*, q) + kd_ang (omega* - omega); root_state
    and base_target rows (pos, quat xyzw, v, omega), gains12 = (kp_lin, kd_lin, kp_ang, kd_ang).  The coupling of the dof
    accelerations, M[0:6, 6:] qdd, is neglected."""
    g = gains12.reshape(4, 3)
    a = torch.cat([g[0] * (base_target[:, :3] - root_state[:, :3]) + g[1] * (base_target[:, 7:10] - root_state[:, 7:10]),
                   g[2] * orientation_error(base_target[:, 3:7], root_state[:, 3:7])
                   + g[3] * (base_target[:, 10:13] - root_state[:, 10:13])], -1)
    return (mass_matrix[:, :6, :6] @ a.unsqueeze(-1)).squeeze(-1) + bias[:, :6]


def _ldlt_inverse(K):
    """K^-1 of a batch of symmetric positive definite matrices (n, N, N) by K = L D L^T, column by column as csrc/shf_qp.hip
    factors it, then the solves against the identity; elementwise and matmul expressions only.  (torch's batched Cholesky
    solver is not used: in float32 on the GPU it returned wrong solutions inside this loop at 4096 envs.)"""
    n, N, _ = K.shape
    L = torch.zeros_like(K)
    D = torch.zeros(n, N, dtype=K.dtype, device=K.device)
    for j in range(N):
        D[:, j] = K[:, j, j] - (L[:, j, :j] * L[:, j, :j] * D[:, :j]).sum(-1)
        if j + 1 < N:
            L[:, j + 1:, j] = (K[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j:j + 1, :j] * D[:, None, :j]).sum(-1)) / D[:, j:j + 1]
    X = torch.eye(N, dtype=K.dtype, device=K.device).repeat(n, 1, 1)
    for i in range(1, N):
        X[:, i] = X[:, i] - (L[:, i, :i].unsqueeze(1) @ X[:, :i]).squeeze(1)
    X = X / D.unsqueeze(-1)
    for i in range(N - 2, -1, -1):
        X[:, i] = X[:, i] - (L[:, i + 1:, i].unsqueeze(1) @ X[:, i + 1:]).squeeze(1)
    return X


def _cone_ata(mu, feet):
    """The diagonal of A^T A (n, 3 feet) of the friction-cone rows: (2, 2, 1 + 4 mu^2) per foot."""
    d = torch.stack([torch.full_like(mu, 2.0), torch.full_like(mu, 2.0), 1.0 + 4.0 * (mu * mu)], -1)
    return d.unsqueeze(1).expand(mu.shape[0], feet, 3).reshape(mu.shape[0], 3 * feet)


def _cone_admm(Kinv, q, sigma, rho, mu, contact, fz_min, fz_max, iters, x0=None):
    """The friction-cone ADMM sweeps and the exact clamp of csrc/shf_cone.h as batched torch expressions: forces (n, feet, 3).
    Kinv (n, N, N) = (P + sigma I + rho A^T A)^-1 and q (n, N) over N = 3 feet variables (a foot of a horizon step counts as a
    foot); sigma, rho (n, 1); mu (n) >= 0; contact (n, feet) bool: the feet that stand; x0 (n, feet, 3) or None: the warm start,
    read where the foot stands."""
    n, feet = contact.shape
    N, T, dev = 3 * feet, q.dtype, q.device
    mu_, rho3 = mu.view(n, 1), rho.unsqueeze(-1)

    def rows(v):                                   # A v of every foot: (n, feet, 5)
        v = v.reshape(n, feet, 3)
        mz = mu_ * v[..., 2]
        return torch.stack([v[..., 2], mz - v[..., 0], mz + v[..., 0], mz - v[..., 1], mz + v[..., 1]], -1)

    x = torch.zeros(n, N, dtype=T, device=dev)
    if x0 is not None:
        x = torch.where(contact.unsqueeze(-1), x0, x.view(n, feet, 3)).reshape(n, N)
    z, y = rows(x), torch.zeros(n, feet, 5, dtype=T, device=dev)
    zero = torch.zeros(n, feet, dtype=T, device=dev)
    lo, hi = torch.zeros(n, feet, 5, dtype=T, device=dev), torch.zeros(n, feet, 5, dtype=T, device=dev)
    lo[..., 0] = torch.where(contact, torch.full_like(zero, fz_min), zero)
    hi[..., 0] = torch.where(contact, torch.full_like(zero, fz_max), zero)
    hi[..., 1:] = torch.where(contact, torch.full_like(zero, float("inf")), zero).unsqueeze(-1)
    for _ in range(int(iters)):
        v = rho3 * z - y
        add = torch.stack([v[..., 2] - v[..., 1], v[..., 4] - v[..., 3],
                           v[..., 0] + mu_ * (((v[..., 1] + v[..., 2]) + v[..., 3]) + v[..., 4])], -1).reshape(n, N)
        xt = (Kinv @ ((sigma * x - q) + add).unsqueeze(-1)).squeeze(-1)
        zt = rows(xt)
        x = 1.6 * xt + (1.0 - 1.6) * x
        zr = 1.6 * zt + (1.0 - 1.6) * z
        zn = torch.minimum(torch.maximum(zr + y / rho3, lo), hi)
        y = y + rho3 * (zr - zn)
        z = zn
    xv = x.reshape(n, feet, 3)
    fz = xv[..., 2].clamp(fz_min, fz_max)
    bnd = mu_ * fz
    f = torch.stack([torch.minimum(torch.maximum(xv[..., 0], -bnd), bnd), torch.minimum(torch.maximum(xv[..., 1], -bnd), bnd), fz], -1)
    return torch.where(contact.unsqueeze(-1), f, torch.zeros_like(f))


def foot_force_qp(j_feet, root_pos, foot_pos, wrench, stance, mu, weights6, alpha=1e-2, beta=0.0, f_prev=None, fz_min=5.0,
                  fz_max=float("inf"), iters=100, bias=None, effort_limit=None):
    """Foot-force distribution of the balance controller: (forces (n, F, 3), efforts (n, nd)).  Per env, with r_f = p_foot_f -
    p_root and G = [[I .. I], [[r_1]x .. [r_F]x]], minimise 1/2 (G f - w)^T S (G f - w) + 1/2 alpha |f|^2 + 1/2 beta |f - f_prev|^2
    subject to fz_min <= f_z <= fz_max, |f_x|, |f_y| <= mu f_z on the stance feet and f = 0 on the others, by `iters` sweeps of
    _cone_admm (rho = sqrt((alpha + beta) m), sigma = 1e-6 m, m the mean diagonal of the stance feet's Hessian block) on K^-1
    from one LDL^T; the efforts are foot_force_efforts' of those forces.  The algorithm of csrc/shf_qp.hip's shf_foot_force_qp
    in torch (its CPU fallback); tests/qp_ref.py holds the NumPy twin."""
    n, F = stance.shape
    N, dt, dev = 3 * F, j_feet.dtype, j_feet.device
    s = stance.to(dt)
    st = stance.to(torch.bool)
    mu = torch.as_tensor(mu, dtype=dt, device=dev).expand(n).clamp(min=0.0)
    S = weights6.to(dt)
    be = float(beta) if f_prev is not None else 0.0
    ab = float(alpha) + be
    r = (foot_pos - root_pos.unsqueeze(1)) * s.unsqueeze(-1)
    G = torch.zeros(n, 6, F, 3, dtype=dt, device=dev)
    for k in range(3):
        G[:, k, :, k] = s
    G[:, 3, :, 1], G[:, 3, :, 2] = -r[..., 2], r[..., 1]
    G[:, 4, :, 0], G[:, 4, :, 2] = r[..., 2], -r[..., 0]
    G[:, 5, :, 0], G[:, 5, :, 1] = -r[..., 1], r[..., 0]
    G = G.reshape(n, 6, N)
    eye = torch.eye(N, dtype=dt, device=dev)
    P = torch.transpose(G, 1, 2) @ (S.view(1, 6, 1) * G) + ab * eye
    q = -(torch.transpose(G, 1, 2) @ (S * wrench).unsqueeze(-1)).squeeze(-1)
    if f_prev is not None:
        q = q - be * (f_prev * s.unsqueeze(-1)).reshape(n, N)
    sv = s.repeat_interleave(3, 1)
    ns = s.sum(1)
    mean = (torch.diagonal(P, dim1=1, dim2=2) * sv).sum(1) / (3.0 * ns.clamp(min=1.0))
    mean = torch.where(ns > 0, mean, torch.ones_like(mean))
    rho, sigma = torch.sqrt(ab * mean).view(n, 1), (1e-6 * mean).view(n, 1)
    K = P + torch.diag_embed(sigma + rho * _cone_ata(mu, F))
    forces = _cone_admm(_ldlt_inverse(K), q, sigma, rho, mu, st, fz_min, fz_max, iters)
    return forces, foot_force_efforts(forces, stance, j_feet, bias, effort_limit)


def gait_plan(state, root_state, foot_pos, contact_z, command, nominal, reset, ticks, dt, height, apex, touchdown_z, late_depth, k_fb,
              max_step, leash=float("inf"), contact_threshold=1.0):
    """One tick of the gait planner: (stance (n, F) uint8, swing_target (n, F, 3) base frame, phase (n, F)), plus the dict
    {"foothold" (n, F, 2), "world_target" (n, F, 3)}.  The algorithm of csrc/shf_gait.hip's shf_gait_plan (its header states
    it step by step) as batched torch expressions, in the dtype of root_state (its CPU fallback); tests/gait_ref.py holds the
    NumPy twin.  state: an object with tick (n) int32, sched (n, F) uint8, anchor (n, F, 3), target (n, 13), yaw (n)
    (units.gait.GaitState), updated in place.  ticks = (period_ticks, offset_ticks, stance_ticks)."""
    P, offsets, stance_ticks = ticks
    n, F = foot_pos.shape[:2]
    dt_, dev = root_state.dtype, root_state.device
    p, q, v = root_state[:, :3], root_state[:, 3:7], root_state[:, 7:10]
    off = torch.as_tensor(list(offsets), dtype=torch.int64, device=dev)
    S = torch.as_tensor(list(stance_ticks), dtype=torch.int64, device=dev)
    assert P >= 1 and bool(((S >= 1) & (S <= P)).all()) and bool(((off >= 0) & (off < P)).all()) and dt > 0 and max_step >= 0
    tick = state.tick.to(torch.int64)
    was = state.sched != 0
    anchor = state.anchor.clone()
    yaw = state.yaw.clone()
    txy = state.target[:, :2].clone()
    # 1. reset
    if reset is not None:
        r = reset.reshape(n) != 0
        tick = torch.where(r, torch.zeros_like(tick), tick)
        was = was | r.unsqueeze(1)
        under = torch.cat([foot_pos[..., :2].to(dt_), torch.full((n, F, 1), touchdown_z - late_depth, dtype=dt_, device=dev)], -1)
        anchor = torch.where(r.view(n, 1, 1), under, anchor)
        heading = torch.atan2(2.0 * (q[:, 0] * q[:, 1] + q[:, 3] * q[:, 2]), 1.0 - 2.0 * (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]))
        yaw = torch.where(r, heading, yaw)
        txy = torch.where(r.unsqueeze(1), p[:, :2], txy)
    # 2. the base target
    cvx, cvy, wz = command[:, 0], command[:, 1], command[:, 2]
    cy, sy = torch.cos(yaw), torch.sin(yaw)
    vw = torch.stack([cy * cvx - sy * cvy, sy * cvx + cy * cvy], 1)
    txy = txy + vw * dt
    d = txy - p[:, :2]
    rr = torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    txy = torch.where((rr > leash).unsqueeze(1), p[:, :2] + d * (leash / rr).unsqueeze(1), txy)
    yaw = yaw + wz * dt
    hy = yaw * 0.5
    tg = state.target
    tg[:, :2], tg[:, 2] = txy, height
    tg[:, 3], tg[:, 4], tg[:, 5], tg[:, 6] = 0.0, 0.0, torch.sin(hy), torch.cos(hy)
    tg[:, 7:9], tg[:, 9] = vw, 0.0
    tg[:, 10], tg[:, 11], tg[:, 12] = 0.0, 0.0, wz
    R = quat_to_matrix(q)
    # 3. the schedule
    phi = (torch.remainder(tick, P).unsqueeze(1) + off.unsqueeze(0)) % P
    s = phi < S.unsqueeze(0)
    # 4. the foothold
    nfx, nfy = nominal[:, 0].to(dt_).unsqueeze(0), nominal[:, 1].to(dt_).unsqueeze(0)
    nwx = R[:, 0, 0].unsqueeze(1) * nfx + R[:, 0, 1].unsqueeze(1) * nfy
    nwy = R[:, 1, 0].unsqueeze(1) * nfx + R[:, 1, 1].unsqueeze(1) * nfy
    hx, hyp = p[:, 0:1] + nwx, p[:, 1:2] + nwy
    vdx, vdy = vw[:, 0:1] - wz.unsqueeze(1) * nwy, vw[:, 1:2] + wz.unsqueeze(1) * nwx
    half = (S.to(dt_).unsqueeze(0) * dt) * 0.5
    gx = vdx * half + k_fb * (v[:, 0:1] - vw[:, 0:1])
    gy = vdy * half + k_fb * (v[:, 1:2] - vw[:, 1:2])
    m = torch.sqrt(gx * gx + gy * gy)
    big = m > max_step
    km = max_step / m
    gx, gy = torch.where(big, gx * km, gx), torch.where(big, gy * km, gy)
    fx, fy = hx + gx, hyp + gy
    # 5. events
    lift, down = was & ~s, ~was & s
    anchor = torch.where(lift.unsqueeze(-1), foot_pos.to(dt_), anchor)
    td = torch.stack([fx, fy, torch.full_like(fx, touchdown_z - late_depth)], -1)
    anchor = torch.where(down.unsqueeze(-1), td, anchor)
    # 6. the feet's targets
    touching = torch.ones(n, F, dtype=torch.bool, device=dev) if contact_z is None else contact_z > contact_threshold
    u = (phi - S.unsqueeze(0) + 1).to(dt_) / (P - S).clamp(min=1).to(dt_).unsqueeze(0)
    b = (u * u) * (3.0 - 2.0 * u)
    a1 = 1.0 - b
    ys = torch.stack([a1 * anchor[..., 0] + b * fx, a1 * anchor[..., 1] + b * fy,
                      (a1 * anchor[..., 2] + b * touchdown_z) + ((4.0 * apex) * u) * (1.0 - u)], -1)
    y = torch.where((~s).unsqueeze(-1), ys, torch.where((~touching).unsqueeze(-1), anchor, foot_pos.to(dt_)))
    dl = y - p.unsqueeze(1)
    swing = torch.stack([(R[:, 0, k].unsqueeze(1) * dl[..., 0] + R[:, 1, k].unsqueeze(1) * dl[..., 1]) + R[:, 2, k].unsqueeze(1) * dl[..., 2]
                         for k in range(3)], -1)
    # 7. outputs
    state.tick.copy_((tick + 1).to(torch.int32))
    state.sched.copy_(s.to(torch.uint8))
    state.anchor.copy_(anchor)
    state.yaw.copy_(yaw)
    return (s & touching).to(torch.uint8), swing, phi.to(dt_) / float(P), {"foothold": torch.stack([fx, fy], -1), "world_target": y}


def leg_effort_mix(stance_efforts, swing_efforts, stance, chain_mask, effort_limit=None):
    """clamp(stance_efforts + m swing_efforts, +-effort_limit): m (n, nd) = 1 where a foot with stance == 0 has the dof on its
    chain (chain_mask (F, nd)), else 0; limit entries <= 0 or None: no clamp.  The torch expression of csrc/shf_gait.hip's
    shf_leg_effort_mix."""
    m = ((stance == 0).unsqueeze(-1) & (chain_mask != 0).unsqueeze(0)).any(1).to(stance_efforts.dtype)
    tau = stance_efforts + m * swing_efforts
    return _effort_clamp(tau, effort_limit)


# -- actuator models (csrc/shf_actuator.hip, whose header states the algorithm step by step; tests/actuator_ref.py holds the NumPy twin)
def _actuator_shift(hist, reset, fill, value):
    """Steps 1 and 2 on a history (n, S, nd), in place: reset rows take `fill`, the slots move back by one, `value` enters."""
    if reset is not None:
        r = (reset.reshape(-1) != 0).view(-1, 1, 1)
        hist.copy_(torch.where(r, fill.unsqueeze(1) if torch.is_tensor(fill) else torch.full_like(hist, fill), hist))
    if hist.shape[1] > 1:
        hist[:, 1:] = hist[:, :-1].clone()
    hist[:, 0] = value


def actuator_activation(h, name):
    if name == "softsign":
        return h / (1.0 + h.abs())
    if name == "relu":
        return torch.where(h > 0, h, torch.zeros_like(h))
    if name == "tanh":
        return torch.tanh(h)
    if name == "elu":
        return torch.nn.functional.elu(h)
    raise ValueError(f"unknown activation {name!r}")


def actuator_step(target, dof_state, cmd_hist, kp=None, kd=None, delay=0, strength=None, saturation=None, velocity_limit=None,
                  effort_limit=None, reset=None, net=None, err_hist=None, vel_hist=None, applied_out=None, efforts_out=None):
    """One sub-step of the actuator model: efforts (n, nd).  The algorithm of csrc/shf_actuator.hip's shf_actuator_step as
    batched torch expressions in the same operation order (its CPU fallback, and the timing baseline on the GPU); a network's
    layers go through torch.nn.functional.linear, which sums in an order of its own.  target (n, nd); dof_state (n, nd, >= 2):
    position and velocity in the last axis; cmd_hist (n, L, nd) and, with a net, err_hist / vel_hist (n, H, nd): the caller's
    state, updated in place; kp / kd (nd) or (n, nd); delay an int or a (n) integer tensor; strength (n, nd); saturation /
    velocity_limit / effort_limit (nd); reset (n) uint8 / bool; net: a units.actuators.ActuatorNet on target's device.
    applied_out / efforts_out (n, nd): written when given."""
    n, nd = target.shape
    L = cmd_hist.shape[1]
    q, qd = dof_state[..., 0], dof_state[..., 1]
    _actuator_shift(cmd_hist, reset, target, target)
    if torch.is_tensor(delay):
        D = delay.reshape(n).to(torch.int64).clamp(0, L - 1)
        a = torch.gather(cmd_hist, 1, D.view(n, 1, 1).expand(n, 1, nd)).squeeze(1)
    else:
        assert 0 <= int(delay) < L, "delay outside 0..L-1"
        a = cmd_hist[:, int(delay)].clone()
    if applied_out is not None:
        applied_out.copy_(a)
    err = a - q
    if net is None:
        tau = (kp * err) - (kd * qd)
    else:
        _actuator_shift(err_hist, reset, 0.0, err)
        _actuator_shift(vel_hist, reset, 0.0, qd)
        taps = list(net.taps)
        x = torch.cat([net.err_scale * err_hist[:, taps], net.vel_scale * vel_hist[:, taps]], 1)       # (n, 2T, nd)
        h = x.transpose(1, 2).reshape(n * nd, 2 * len(taps))
        layers = net.layers
        for l, (W, b) in enumerate(layers):
            h = torch.nn.functional.linear(h, W, b)
            if l < len(layers) - 1:
                h = actuator_activation(h, net.activation)
        tau = (net.out_scale * h[:, 0]).reshape(n, nd)
    if strength is not None:
        tau = tau * strength
    if saturation is not None and velocity_limit is not None:
        cap = torch.full_like(saturation, float("inf")) if effort_limit is None else \
            torch.where(effort_limit > 0, effort_limit, torch.full_like(effort_limit, float("inf")))
        r = qd / velocity_limit
        hi = torch.minimum(torch.clamp_min(saturation * (1.0 - r), 0.0), cap)
        lo = torch.maximum(torch.clamp_max(saturation * (-1.0 - r), 0.0), -cap)
        tau = torch.maximum(torch.minimum(tau, hi), lo)
    else:
        tau = _effort_clamp(tau, effort_limit)
    if efforts_out is not None:
        efforts_out.copy_(tau)
        return efforts_out
    return tau


# -- proprioceptive sensors (csrc/shf_proprio.hip, whose header states the algorithm step by step; tests/proprio_ref.py holds the NumPy twin)
def _philox_mulhilo(a: int, b):
    """(high, low) 32-bit words of a * b for a 32-bit constant a and int64 tensors b of 32-bit words, without leaving int64:
    b = bh 2^16 + bl, so that both partial products stay below 2^48."""
    pl, ph = a * (b & 0xFFFF), a * (b >> 16)
    return ((ph + (pl >> 16)) >> 16) & 0xFFFFFFFF, (pl + ((ph & 0xFFFF) << 16)) & 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0: int, k1: int):
    """Philox4x32-10 (csrc/shf_task.h: philox4x32) on int64 tensors of 32-bit words."""
    c0, c1, c2, c3 = torch.broadcast_tensors(c0, c1, c2, c3)
    for _ in range(10):
        h0, l0 = _philox_mulhilo(0xD2511F53, c0)
        h1, l1 = _philox_mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _proprio_latency(ring, h, D, rs, m):
    """ring (n, L, C), a view of the state: the delayed (n, C) output, and the ring updated in place."""
    n, L, C = ring.shape
    slot = h - D
    slot = torch.where(slot < 0, slot + L, slot)
    old = torch.gather(ring, 1, slot.view(n, 1, 1).expand(n, 1, C)).squeeze(1)
    out = torch.where((rs | (D == 0)).view(n, 1), m, old)
    here = rs.view(n, 1) | (torch.arange(L, device=ring.device).view(1, L) == h.view(n, 1))       # (n, L): the slots that take m
    ring.copy_(torch.where(here.unsqueeze(2), m.unsqueeze(1), ring))
    return out


def proprioception_step(body_state, dof_state, contact, config, params, delay, state, out, switches=None, reset=None, global_ids=None):
    """One sensor read of every env: fills and returns out (n, D).  The algorithm of csrc/shf_proprio.hip's
    shf_proprioception_step as batched torch expressions in the same operation order (its CPU path, and the timing baseline on
    the GPU); the arguments are glue.proprioception_step's, on any device."""
    f32 = torch.float32
    n, nd = dof_state.shape[:2]
    dev = dof_state.device
    I, F, L = int(config.num_imus), int(config.num_feet), int(config.slots)
    P = params.to(f32)
    sg, sa, wg, wa, b0g, b0a, sq, sv, o_rng, res, inv_res, on2, off2 = (P[k] for k in range(13))
    dt, inv_dt = torch.tensor(config.dt, dtype=f32, device=dev), torch.tensor(config.inv_dt, dtype=f32, device=dev)
    cnt = state["counter"]
    c = cnt[:, 0, 0].to(torch.int64) & 0xFFFFFFFF
    h = cnt[:, 0, 1].to(torch.int64)
    rs = c == 0
    if reset is not None:
        rs = rs | (reset.reshape(n) != 0)
    Dl = delay.reshape(n, 3).to(torch.int64).clamp(0, int(config.max_delay))
    gid = int(config.env_id_offset) + torch.arange(n, device=dev, dtype=torch.int64) if global_ids is None else global_ids.reshape(n).to(torch.int64)
    lo, hi = gid & 0xFFFFFFFF, (gid >> 32) & 0xFFFFFFFF
    k0, k1 = int(config.seed_lo), int(config.seed_hi)

    def block(stream):
        s = torch.as_tensor(stream, dtype=torch.int64, device=dev)
        sh = (n,) + (1,) * s.dim()
        w = philox4x32(lo.view(sh), c.view(sh), s, hi.view(sh), k0, k1)
        return [(x >> 8).to(f32) * 5.9604644775390625e-08 for x in w]

    def gauss(stream):
        u = block(stream)
        return (((u[0] + u[1]) + (u[2] + u[3])) - 2.0) * 1.7320508

    usym = lambda u, b: ((b - (-b)) * u) + (-b)

    def matrix(q):
        x, y, z, w = q
        return [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
                [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]

    for i in range(I):
        S = 0x50000000 + 16 * i
        b = int(config.imu_body[i])
        ps = [torch.tensor(float(v), dtype=f32, device=dev) for v in config.imu_pos[i]]
        bx, by, bz, bw = [torch.tensor(float(v), dtype=f32, device=dev) for v in config.imu_quat[i]]
        bs = body_state[:, b]
        ax, ay, az, aw = (bs[:, 3 + k] for k in range(4))
        wb = [bs[:, 10 + k] for k in range(3)]
        q = (((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by - ax * bz) + ay * bw) + az * bx,
             ((aw * bz + ax * by) - ay * bx) + az * bw, ((aw * bw - ax * bx) - ay * by) - az * bz)
        R, Rb = matrix(q), matrix((ax, ay, az, aw))
        arm = [(Rb[a][0] * ps[0] + Rb[a][1] * ps[1]) + Rb[a][2] * ps[2] for a in range(3)]
        vs = [bs[:, 7] + (wb[1] * arm[2] - wb[2] * arm[1]), bs[:, 8] + (wb[2] * arm[0] - wb[0] * arm[2]),
              bs[:, 9] + (wb[0] * arm[1] - wb[1] * arm[0])]
        st = state["imu"][:, i]
        ug, ua = block(S + 12), block(S + 13)
        vp = [torch.where(rs, vs[a], st[:, a]) for a in range(3)]
        bg = [torch.where(rs, usym(ug[a], b0g), st[:, 3 + a]) for a in range(3)]
        ba = [torch.where(rs, usym(ua[a], b0a), st[:, 6 + a]) for a in range(3)]
        accw = [((vs[a] - vp[a]) * inv_dt) - float(config.gravity[a]) for a in range(3)]
        m = []
        for a in range(3):
            gw = (R[0][a] * wb[0] + R[1][a] * wb[1]) + R[2][a] * wb[2]
            m.append((gw + bg[a]) + (sg * gauss(S + a)))
        for a in range(3):
            aw_ = (R[0][a] * accw[0] + R[1][a] * accw[1]) + R[2][a] * accw[2]
            m.append((aw_ + ba[a]) + (sa * gauss(S + 3 + a)))
        o = _proprio_latency(st[:, 9:].view(n, L, 6), h, Dl[:, 0], rs, torch.stack(m, 1))
        for a in range(3):
            st[:, 3 + a] = bg[a] + (wg * gauss(S + 6 + a))
            st[:, 6 + a] = ba[a] + (wa * gauss(S + 9 + a))
            st[:, a] = vs[a]
        out[:, 3 * i:3 * i + 3] = o[:, :3]
        out[:, 3 * I + 3 * i:3 * I + 3 * i + 3] = o[:, 3:]

    S = 0x50001000 + 4 * torch.arange(nd, device=dev, dtype=torch.int64)
    st = state["enc"]
    q, qd = dof_state[:, :, 0], dof_state[:, :, 1]
    off = torch.where(rs.view(n, 1), usym(block(S + 2)[0], o_rng), st[:, :, 0])
    st[:, :, 0] = off
    x = (q + off) + (sq * gauss(S))
    x = torch.where(res > 0, res * torch.round(x * inv_res), x)
    if int(config.velocity_mode) == 1:
        v = (x - torch.where(rs.view(n, 1), x, st[:, :, 1])) * inv_dt
    else:
        v = qd + (sv * gauss(S + 1))
    rep = lambda a: a.repeat_interleave(nd)
    o = _proprio_latency(st[:, :, 2:].view(n * nd, L, 2), rep(h), rep(Dl[:, 1]), rep(rs), torch.stack([x, v], -1).view(n * nd, 2)).view(n, nd, 2)
    st[:, :, 1] = x
    out[:, 6 * I:6 * I + nd] = o[:, :, 0]
    out[:, 6 * I + nd:6 * I + 2 * nd] = o[:, :, 1]

    base = 6 * I + 2 * nd
    zero = torch.zeros((), dtype=f32, device=dev)
    for k in range(F):
        cf = contact[:, int(config.foot_body[k])]
        fx, fy, fz = cf[:, 0], cf[:, 1], cf[:, 2]
        s = fz * fz.abs() if int(config.contact_mode) == 1 else (fx * fx + fy * fy) + fz * fz
        st = state["foot"][:, k]
        p = (st[:, 0] != 0) & ~rs
        air, con, lair, lcon = (torch.where(rs, zero, st[:, j]) for j in (1, 2, 3, 4))
        on = torch.where(s > on2, torch.ones_like(p), torch.where(s < off2, torch.zeros_like(p), p))
        first, left = on & ~p & ~rs, p & ~on
        lair = torch.where(first, air + dt, lair)
        lcon = torch.where(left, con + dt, lcon)
        air = torch.where(on, zero, air + dt)
        con = torch.where(on, con + dt, zero)
        m = torch.stack([on.to(f32), first.to(f32), air, con, lair, lcon], -1)
        o = _proprio_latency(st[:, 5:].view(n, L, 6), h, Dl[:, 2], rs, m)
        st[:, :5] = torch.stack([m[:, 0], air, con, lair, lcon], -1)
        for j in range(6):
            out[:, base + j * F + k] = o[:, j]
        if switches is not None:
            switches[:, k] = o[:, 0] != 0
            switches[:, F + k] = o[:, 1] != 0
    c1 = (c + 1) & 0xFFFFFFFF
    cnt[:, :, 0] = torch.where(c1 >= 2 ** 31, c1 - 2 ** 32, c1).to(torch.int32).view(n, 1)
    cnt[:, :, 1] = torch.where(h + 1 == L, torch.zeros_like(h), h + 1).to(torch.int32).view(n, 1)
    return out


# -- the horizon MPC (csrc/shf_mpc.hip, whose header states the three algorithms step by step; tests/mpc_ref.py holds the NumPy twins)
def mpc_horizon(state, stance, foot_pos, command, nominal, ticks, dt, touchdown_z, max_step, horizon, steps_per_tick):
    """The MPC's tables: (contact (n, H, F) uint8, xref (n, H + 1, 12), pos (n, H, F, 3)).  The algorithm of shf_mpc_horizon as
    batched torch expressions, in the dtype of state.target (its CPU fallback).  state: tick / target / yaw as gait_plan left
    them this tick (the stored tick already advanced); stance (n, F): gait_plan's; ticks = (period_ticks, offset_ticks,
    stance_ticks)."""
    P, offsets, stance_ticks = ticks
    n, F = foot_pos.shape[:2]
    H, S = int(horizon), int(steps_per_tick)
    tg, yaw = state.target, state.yaw
    T, dev = tg.dtype, tg.device
    delta = float(S) * dt
    k = torch.arange(H + 1, device=dev, dtype=T)
    kd = (k * delta).unsqueeze(0)                                           # (1, H + 1)
    xref = torch.zeros(n, H + 1, 12, dtype=T, device=dev)
    xref[:, :, 2] = yaw.unsqueeze(1) + kd * tg[:, 12:13]
    xref[:, :, 3], xref[:, :, 4], xref[:, :, 5] = tg[:, 0:1] + kd * tg[:, 7:8], tg[:, 1:2] + kd * tg[:, 8:9], tg[:, 2:3].expand(n, H + 1)
    xref[:, :, 6:9], xref[:, :, 9:12] = tg[:, None, 10:13], tg[:, None, 7:10]
    tm = torch.remainder(state.tick.to(torch.int64) - 1, P)
    off = torch.as_tensor(list(offsets), dtype=torch.int64, device=dev)
    stt = torch.as_tensor(list(stance_ticks), dtype=torch.int64, device=dev)
    ks = torch.remainder(torch.arange(H, device=dev, dtype=torch.int64) * S, P)
    phi = torch.remainder(tm.view(n, 1, 1) + ks.view(1, H, 1) + off.view(1, 1, F), P)
    contact = phi < stt.view(1, 1, F)
    contact[:, 0] = stance != 0
    psi = xref[:, :H, 2].unsqueeze(-1)                                      # (n, H, 1)
    cs, sn = torch.cos(psi), torch.sin(psi)
    nfx, nfy = nominal[:, 0].to(T).view(1, 1, F), nominal[:, 1].to(T).view(1, 1, F)
    nwx, nwy = cs * nfx - sn * nfy, sn * nfx + cs * nfy
    hx, hy = xref[:, :H, 3:4] + nwx, xref[:, :H, 4:5] + nwy
    cvx, cvy, cwz = (command[:, i].to(T).view(n, 1, 1) for i in range(3))
    vdx, vdy = (cs * cvx - sn * cvy) - cwz * nwy, (sn * cvx + cs * cvy) + cwz * nwx
    half = ((stt.to(T) * dt) * 0.5).view(1, 1, F)
    gx, gy = vdx * half, vdy * half
    m = torch.sqrt(gx * gx + gy * gy)
    q = max_step / m
    big = m > max_step
    gx, gy = torch.where(big, gx * q, gx), torch.where(big, gy * q, gy)
    new = torch.stack([hx + gx, hy + gy, torch.full_like(gx, touchdown_z)], -1)          # (n, H, F, 3)
    pos = torch.zeros(n, H, F, 3, dtype=T, device=dev)
    hold = torch.where(contact[:, 0].unsqueeze(-1), foot_pos.to(T), torch.zeros(n, F, 3, dtype=T, device=dev))
    pos[:, 0] = hold
    for j in range(1, H):
        start = contact[:, j] & ~contact[:, j - 1]
        hold = torch.where(start.unsqueeze(-1), new[:, j], hold)
        pos[:, j] = torch.where(contact[:, j].unsqueeze(-1), hold, torch.zeros_like(hold))
    return contact.to(torch.uint8), xref, pos


def _gauss_jordan_inverse(A):
    """A^-1 of a batch (n, N, N) by the in-place Gauss-Jordan sweep without pivoting, as csrc/shf_mpc.hip inverts."""
    A = A.clone()
    for k in range(A.shape[-1]):
        p = 1.0 / A[:, k, k]
        row = A[:, k, :] * p.unsqueeze(1)
        f = A[:, :, k].clone()
        A = A - f.unsqueeze(2) * row.unsqueeze(1)
        A[:, :, k] = -(f * p.unsqueeze(1))
        A[:, k, :] = row
        A[:, k, k] = p
    return A


def _mpc_state(root_state, psi0):
    x, y, z, w = (root_state[:, 3 + k] for k in range(4))
    R20, R21, R22 = 2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)
    R10, R00 = 2.0 * (x * y + w * z), 1.0 - 2.0 * (y * y + z * z)
    yaw = torch.atan2(R10, R00)
    yaw = yaw + torch.round((psi0 - yaw) * 0.15915494309189535) * 6.283185307179586
    return torch.cat([torch.atan2(R21, R22).unsqueeze(1), torch.asin((-R20).clamp(-1.0, 1.0)).unsqueeze(1), yaw.unsqueeze(1),
                      root_state[:, 0:3], root_state[:, 10:13], root_state[:, 7:10]], 1)


def foot_force_mpc(contact, xref, pos, root_state, mass_matrix, dyn_bias, j_feet, mu, weights12, alpha=1e-5, fz_min=5.0,
                   fz_max=float("inf"), iters=100, step_dt=0.03, bias=None, effort_limit=None, u_io=None, warm_shift=0):
    """The horizon MPC's solve: (forces (n, F, 3), efforts (n, nd)); u_io (n, H, F, 3) or None is the warm start and receives
    the solution.  The algorithm of csrc/shf_mpc.hip's shf_foot_force_mpc as batched torch expressions in the dtype of xref
    (its CPU fallback): the condensed P and q in closed form, K^-1 formed once (Gauss-Jordan) and multiplied by in every sweep."""
    n, H, F = contact.shape
    F3, N = 3 * F, 3 * F * H
    T, dev = xref.dtype, xref.device
    L = weights12.to(T)
    d = float(step_dt)
    Mi = _gauss_jordan_inverse(mass_matrix[:, :6, :6].to(T))
    g = -(Mi @ dyn_bias[:, :6].to(T).unsqueeze(-1)).squeeze(-1)
    root = root_state.to(T)
    x = _mpc_state(root, xref[:, 0, 2])
    CA, CB = torch.zeros(n, H + 1, dtype=T, device=dev), torch.zeros(n, H + 1, dtype=T, device=dev)
    E = torch.zeros(n, H, 12, dtype=T, device=dev)
    for s in range(H):
        psi = xref[:, s, 2]
        cs, sn = torch.cos(psi), torch.sin(psi)
        th = torch.stack([cs * x[:, 6] + sn * x[:, 7], cs * x[:, 7] - sn * x[:, 6], x[:, 8]], 1)
        x = torch.cat([x[:, 0:3] + d * th, x[:, 3:6] + d * x[:, 9:12], x[:, 6:9] + d * g[:, 3:6], x[:, 9:12] + d * g[:, 0:3]], 1)
        CA[:, s + 1], CB[:, s + 1] = CA[:, s] + cs, CB[:, s] + sn
        E[:, s] = x - xref[:, s + 1]
    ar = torch.arange(N, device=dev)
    ki, fi, ci = ar // F3, (ar % F3) // 3, ar % 3
    cf = contact[:, ki, fi].to(T)
    r = pos[:, ki, fi].to(T) - (root[:, None, :3] + (xref[:, ki, 3:6] - xref[:, :1, 3:6]))
    zero = torch.zeros(n, N, dtype=T, device=dev)
    c0, c1 = (ci == 0).unsqueeze(0), (ci == 1).unsqueeze(0)
    a0 = torch.where(c0, zero, torch.where(c1, -r[..., 2], r[..., 1]))
    a1 = torch.where(c0, r[..., 2], torch.where(c1, zero, -r[..., 0]))
    a2 = torch.where(c0, -r[..., 1], torch.where(c1, r[..., 0], zero))
    W = torch.stack([(d * (Mi[:, q, :3][:, ci] + ((Mi[:, q, 3:4] * a0 + Mi[:, q, 4:5] * a1) + Mi[:, q, 5:6] * a2))) * cf for q in range(6)], 1)
    TX, TY = torch.zeros(n, H + 1, N, dtype=T, device=dev), torch.zeros(n, H + 1, N, dtype=T, device=dev)
    for s in range(1, H + 1):
        a, b = CA[:, s, None] - CA[:, ki + 1], CB[:, s, None] - CB[:, ki + 1]
        on = (s > ki + 1).unsqueeze(0)
        TX[:, s] = torch.where(on, a * W[:, 3] + b * W[:, 4], zero)
        TY[:, s] = torch.where(on, a * W[:, 4] - b * W[:, 3], zero)
    dd = d * d
    o = lambda u, v: u.unsqueeze(2) * v.unsqueeze(1)
    wLv = [W[:, k] * L[9 + k] for k in range(3)]
    wLw = [W[:, 3 + k] * L[6 + k] for k in range(3)]
    wLp = [W[:, k] * L[3 + k] for k in range(3)]
    wLz = W[:, 5] * L[2]
    m = torch.maximum(ki.unsqueeze(1), ki.unsqueeze(0))
    s2 = torch.zeros(N, N, dtype=torch.int64, device=dev)
    for s in range(1, H + 1):
        s2 += torch.where(s > m, (s - 1 - ki.unsqueeze(1)) * (s - 1 - ki.unsqueeze(0)), torch.zeros_like(m))
    dv = (o(wLv[0], W[:, 0]) + o(wLv[1], W[:, 1])) + o(wLv[2], W[:, 2])
    dw = (o(wLw[0], W[:, 3]) + o(wLw[1], W[:, 4])) + o(wLw[2], W[:, 5])
    dp = (o(wLp[0], W[:, 0]) + o(wLp[1], W[:, 1])) + o(wLp[2], W[:, 2])
    dz = o(wLz, W[:, 5])
    th = torch.zeros(n, N, N, dtype=T, device=dev)
    for s in range(1, H + 1):
        th = th + (o(L[0] * TX[:, s], TX[:, s]) + o(L[1] * TY[:, s], TY[:, s]))
    P = ((H - m).to(T).unsqueeze(0) * (dw + dv) + (dd * s2.to(T)).unsqueeze(0) * (dp + dz)) + dd * th
    eye = torch.eye(N, dtype=T, device=dev)
    P = P + float(alpha) * eye
    q = torch.zeros(n, N, dtype=T, device=dev)
    for s in range(1, H + 1):
        nn = (s - 1 - ki).to(T).unsqueeze(0)
        Es = E[:, s - 1]
        pa = d * (((L[0] * TX[:, s]) * Es[:, 0:1] + (L[1] * TY[:, s]) * Es[:, 1:2]) + nn * (wLz * Es[:, 2:3]))
        pb = (d * nn) * ((wLp[0] * Es[:, 3:4] + wLp[1] * Es[:, 4:5]) + wLp[2] * Es[:, 5:6])
        pc = ((wLw[0] * Es[:, 6:7] + wLw[1] * Es[:, 7:8]) + wLw[2] * Es[:, 8:9]) \
            + ((wLv[0] * Es[:, 9:10] + wLv[1] * Es[:, 10:11]) + wLv[2] * Es[:, 11:12])
        q = torch.where((s > ki).unsqueeze(0), q + ((pa + pb) + pc), q)
    mu = torch.as_tensor(mu, dtype=T, device=dev).expand(n).clamp(min=0.0)
    dgl = torch.diagonal(P, dim1=1, dim2=2)
    nc = cf.sum(1)
    mean = (dgl * cf).sum(1) / nc.clamp(min=1.0)
    mean = torch.where(nc > 0, mean, torch.ones_like(mean))
    rho, sigma = torch.sqrt(float(alpha) * mean).view(n, 1), (1e-6 * mean).view(n, 1)
    Kinv = _gauss_jordan_inverse(P + torch.diag_embed(sigma + rho * _cone_ata(mu, H * F)))
    x0 = None if u_io is None else u_io[:, (torch.arange(H, device=dev) + int(warm_shift)).clamp(max=H - 1)].reshape(n, H * F, 3).to(T)
    u = _cone_admm(Kinv, q, sigma, rho, mu, (cf != 0).reshape(n, H * F, 3)[..., 0], fz_min, fz_max, iters, x0).reshape(n, H, F, 3)
    if u_io is not None:
        u_io.copy_(u)
    forces = u[:, 0]
    return forces, foot_force_efforts(forces, contact[:, 0], j_feet, bias, effort_limit)


def foot_force_efforts(forces, stance, j_feet, bias=None, effort_limit=None):
    """efforts (n, nd) = -sum over the feet with stance != 0 of Jl_f^T f_f, + bias[:, 6:], clamped to +-effort_limit (entries <=
    0: no limit): the torch expression of csrc/shf_mpc.hip's shf_foot_force_efforts."""
    f = torch.where((stance != 0).unsqueeze(-1), forces, torch.zeros_like(forces)).to(j_feet.dtype)
    tau = -(torch.transpose(j_feet[:, :, :3, 6:], 2, 3) @ f.unsqueeze(-1)).squeeze(-1).sum(1)
    if bias is not None:
        tau = tau + bias[:, 6:]
    return _effort_clamp(tau, effort_limit)


class Primitives:
    """The functions above under the signatures of shifu_amd.glue's kernel wrappers: the set of primitives
    glue.balance_control / glue.locomotion_control run on when the tensors are not float32 CUDA tensors."""

    @staticmethod
    def gait_params(dt, height, touchdown_z, gait):
        from types import SimpleNamespace
        return SimpleNamespace(dt=float(dt), height=float(height), apex=gait.apex, touchdown_z=float(touchdown_z), late_depth=gait.late_depth,
                               k_fb=gait.k_fb, max_step=gait.max_step, leash=gait.leash, contact_threshold=gait.contact_threshold)

    @staticmethod
    def gait_plan(state, root_state, foot_pos, contact_z, command, nominal, reset, ticks, p):
        return gait_plan(state, root_state, foot_pos, contact_z, command, nominal, reset, ticks, p.dt, p.height, p.apex, p.touchdown_z,
                         p.late_depth, p.k_fb, p.max_step, p.leash, p.contact_threshold)[:3]

    @staticmethod
    def foot_force_qp(j_feet, root_pose, foot_pos, stance, mu, weights6, wrench=None, mass_matrix=None, dyn_bias=None, base_target=None,
                      gains12=None, alpha=1e-2, beta=0.0, f_prev=None, fz_min=5.0, fz_max=float("inf"), iters=100, bias=None,
                      effort_limit=None):
        if wrench is None:
            wrench = balance_wrench(mass_matrix, dyn_bias, root_pose, base_target, gains12)
        return foot_force_qp(j_feet, root_pose[:, :3], foot_pos, wrench, stance, mu, weights6, alpha, beta, f_prev, fz_min, fz_max, iters,
                             bias, effort_limit)

    @staticmethod
    def mpc_horizon(state, stance, foot_pos, command, nominal, ticks, p, horizon, steps_per_tick):
        return mpc_horizon(state, stance, foot_pos, command, nominal, ticks, p.dt, p.touchdown_z, p.max_step, horizon, steps_per_tick)

    @staticmethod
    def foot_force_mpc(*args, forces_out=None):
        forces, efforts = foot_force_mpc(*args)
        if forces_out is not None:
            forces = forces_out.copy_(forces)
        return forces, efforts

    foot_force_efforts = staticmethod(foot_force_efforts)
    leg_effort_mix = staticmethod(leg_effort_mix)

    @staticmethod
    def foot_impedance(j_feet, dof_state, root_pose, foot_pos, target, kp3, kd3, bias=None, effort_limit=None):
        return foot_impedance_control(j_feet, dof_state[..., 1], root_pose[:, :3], root_pose[:, 3:7], foot_pos, target, kp3, kd3, bias,
                                      effort_limit)
