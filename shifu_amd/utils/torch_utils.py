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
    if effort_limit is not None:
        lim = torch.where(effort_limit > 0, effort_limit, torch.full_like(effort_limit, float("inf")))
        tau = torch.maximum(torch.minimum(tau, lim), -lim)
    return tau


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
    if effort_limit is not None:
        lim = torch.where(effort_limit > 0, effort_limit, torch.full_like(effort_limit, float("inf")))
        tau = torch.maximum(torch.minimum(tau, lim), -lim)
    return tau
