"""Host side of csrc/shf_glue.hip: the LIBRARY glue of the hook-compatible path as single HIP launches.

ShifuVecEnv with torch hooks (the source-compatible path) spends most of its 2.4 ms per vec-step in small torch launches,
and a good part of those are not user hooks but library code: LeggedRobot.post_step (reference
shifu/units/robot.py:222-229), TerrainGymEnv.get_heights (shifu/gym/isaac_gym.py:393-433), HistoryRecorder
(shifu/utils/train.py:12-35), ShifuVecEnv.log_info / compute_reward (shifu/gym/env.py:149-185).  Each function below is
that piece as one kernel, used by the mirror classes whenever their tensors live on the GPU.  Results equal the oracle's
glue_* functions bit for bit (tests/test_gpu_glue.py); there is no CPU path here -- CPU tensors (golden-vector tests of
the Python mirror) keep the reference's torch expressions in the classes themselves.  The two control sequences of the legged
robots (balance_control, locomotion_control) are the exception: they exist here alone and take the primitives they run on."""
import ctypes as C

import torch

from ._lib import check, lib

_vp = C.c_void_p


def _stream(dev):
    return _vp(torch._C._cuda_getCurrentRawStream(dev.index if dev.index is not None else torch.cuda.current_device()))


def _f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda, "float32 contiguous CUDA tensor expected"
    return _vp(t.data_ptr())


def usable(*tensors) -> bool:
    return all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def base_frame_state(root_state, root_indices, up_axis, lin, ang, pg, gvec):
    """In place: lin / ang / pg / gvec (n, 3) from root_state rows root_indices (int64) -- LeggedRobot.post_step."""
    n = lin.shape[0]
    idx = None if root_indices is None else root_indices.contiguous()
    assert idx is None or (idx.dtype == torch.int64 and idx.is_cuda and idx.numel() == n)
    with torch.cuda.device(root_state.device):
        check(lib().shf_base_frame_state(_f32c(root_state), None if idx is None else _vp(idx.data_ptr()), root_state.shape[0], n,
                                         int(up_axis), _f32c(lin), _f32c(ang), _f32c(pg), _f32c(gvec), _stream(root_state.device)))


def get_heights(terrain_struct, height_samples, root_state, root_indices, points_xy, n):
    """(n, P) measured heights -- TerrainGymEnv.get_heights.  height_samples: int16 (rows, cols) device tensor."""
    P = points_xy.shape[0]
    out = torch.empty(n, P, device=root_state.device, dtype=torch.float32)
    idx = None if root_indices is None else root_indices.contiguous()
    assert height_samples is None or (height_samples.dtype == torch.int16 and height_samples.is_contiguous())
    with torch.cuda.device(root_state.device):
        check(lib().shf_get_heights(C.byref(terrain_struct), None if height_samples is None else _vp(height_samples.data_ptr()),
                                    _f32c(root_state), None if idx is None else _vp(idx.data_ptr()), root_state.shape[0],
                                    _f32c(points_xy), n, P, _f32c(out), _stream(root_state.device)))
    return out


def history_add(history_buf, x):
    """HistoryRecorder.add on a contiguous (..., H) buffer."""
    H = history_buf.shape[-1]
    rows = history_buf.numel() // H
    x = x.contiguous()
    assert x.numel() == rows
    with torch.cuda.device(history_buf.device):
        check(lib().shf_history_add(_f32c(history_buf), _f32c(x), rows, H, _stream(history_buf.device)))


def rows_fill_indexed(buf, idx, value=0.0):
    """buf[idx] = value along dim 0 (HistoryRecorder.reset_idx)."""
    idx = idx.contiguous()
    assert idx.dtype == torch.int64 and idx.is_cuda
    row_words = buf.numel() // buf.shape[0]
    with torch.cuda.device(buf.device):
        check(lib().shf_rows_fill_indexed(_f32c(buf), _vp(idx.data_ptr()), idx.numel(), buf.shape[0], row_words, float(value),
                                          _stream(buf.device)))


class EpisodeLog:
    """extras["episode"] means for one reset set in one launch (ShifuVecEnv.log_info): keeps the 17-word workspace and
    hands out a fresh (K,) result tensor per call (the caller stores 0-d views of it in `extras`)."""

    def __init__(self, device):
        self.ws = torch.zeros(17, dtype=torch.int64, device=device)

    def __call__(self, sums_list, env_ids, episode_length_s, episode_length=None, reset_buf=None, history=None):
        """episode_length / reset_buf / history given: the rest of ShifuVecEnv.reset_idx's buffer writes for the same ids in the
        same launch (shf_reset_bookkeeping): episode_length[ids] = 0, reset_buf[ids] = 1, history[ids] = 0."""
        K, dev = len(sums_list), self.ws.device
        if env_ids.numel() == 0:          # torch.mean over an empty selection (the kernel returns before writing)
            return torch.full((K,), float("nan"), dtype=torch.float32, device=dev)
        out = torch.empty(K, dtype=torch.float32, device=dev)
        ptrs = (_vp * K)(*[t.data_ptr() for t in sums_list])
        ids = env_ids.contiguous()
        assert ids.dtype == torch.int64
        with torch.cuda.device(dev):
            if episode_length is None and reset_buf is None and history is None:
                check(lib().shf_episode_log(ptrs, K, _vp(ids.data_ptr()), ids.numel(), sums_list[0].numel(), float(episode_length_s),
                                            _vp(self.ws.data_ptr()), _vp(out.data_ptr()), _stream(dev)))
            else:
                n = sums_list[0].numel()
                check(lib().shf_reset_bookkeeping(
                    ptrs, K, _vp(ids.data_ptr()), ids.numel(), n, float(episode_length_s), _vp(self.ws.data_ptr()), _vp(out.data_ptr()),
                    _vp(episode_length.data_ptr()) if episode_length is not None else None,
                    _vp(reset_buf.data_ptr()) if reset_buf is not None else None, reset_buf.element_size() if reset_buf is not None else 0,
                    _vp(history.data_ptr()) if history is not None else None, history.numel() // n if history is not None else 0,
                    _stream(dev)))
        return out


def reward_accumulate(terms, sums_list, rew_buf):
    """rew_buf = terms[0] + terms[1] + ...; sums_list[k] += terms[k] (ShifuVecEnv.compute_reward)."""
    K = len(terms)
    tp = (_vp * K)(*[t.data_ptr() for t in terms])
    sp = (_vp * K)(*[t.data_ptr() for t in sums_list])
    with torch.cuda.device(rew_buf.device):
        check(lib().shf_reward_accumulate(tp, sp, K, rew_buf.numel(), _f32c(rew_buf), _stream(rew_buf.device)))


def reset_dof_rows(dof_state, dof_targets, default_dof_pos, env_ids, root_indices):
    """Robot._reset_dof_state's tensor writes in one launch; returns the int32 actor ids for the indexed commits."""
    ids = env_ids.contiguous()
    assert ids.dtype == torch.int64 and ids.is_cuda
    n, nd = dof_targets.shape
    actor_ids = torch.empty(ids.numel(), dtype=torch.int32, device=ids.device)
    ri = root_indices.contiguous()
    with torch.cuda.device(ids.device):
        check(lib().shf_reset_dof_rows(_f32c(dof_state), _f32c(dof_targets), _f32c(default_dof_pos), _vp(ids.data_ptr()), ids.numel(),
                                       n, nd, _vp(ri.data_ptr()), _vp(actor_ids.data_ptr()), _stream(ids.device)))
    return actor_ids


def ik_dls(j_ee, dof_pos, ee_pose, goal_pose, damping):
    """ArmRobot.inverse_kinematics in one launch.  j_ee (n, 6, nd), ee_pose (n, 7) and dof_pos (n, nd) may be strided
    views into the Jacobian / rigid-body-state / dof-state tensors (unit stride inside a block, any stride between envs)."""
    n, six, nd = j_ee.shape
    assert six == 6 and j_ee.stride(2) == 1 and j_ee.stride(1) == nd and ee_pose.stride(1) == 1
    assert dof_pos.shape == (n, nd) and dof_pos.stride(0) == nd * dof_pos.stride(1)
    goal = goal_pose.contiguous()
    out = torch.empty(n, nd, device=j_ee.device, dtype=torch.float32)
    with torch.cuda.device(j_ee.device):
        check(lib().shf_ik_dls(_vp(j_ee.data_ptr()), j_ee.stride(0), _vp(dof_pos.data_ptr()), dof_pos.stride(1),
                               _vp(ee_pose.data_ptr()), ee_pose.stride(0), _f32c(goal), n, nd, float(damping), _f32c(out),
                               _stream(j_ee.device)))
    return out


def osc(j_ee, mass_matrix, bias, dof_state, ee_pose, goal_pose, kp6, kd6, damping=0.0, q_rest=None, kp_null=0.0, kd_null=0.0,
        effort_limit=None):
    """ArmRobot.operational_space_control in one launch (shf_osc): efforts (n, nd).  j_ee (n, 6, nd) and ee_pose (n, 7) may be
    strided views as for ik_dls; dof_state (n, nd, >= 2) holds position and velocity in its last axis (the dof-state tensor
    itself, or any view with unit stride there and rows packed per env).  mass_matrix (n, nd, nd), bias (n, nd) or None,
    kp6 / kd6 (6), q_rest / effort_limit (nd) or None."""
    n, six, nd = j_ee.shape
    assert six == 6 and j_ee.stride(2) == 1 and j_ee.stride(1) == nd and ee_pose.stride(1) == 1
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (j_ee, ee_pose, dof_state)), "float32 CUDA tensors expected"
    assert dof_state.shape[:2] == (n, nd) and dof_state.shape[2] >= 2 and dof_state.stride(2) == 1
    assert dof_state.stride(1) >= 2 and dof_state.stride(0) == nd * dof_state.stride(1)
    assert mass_matrix.shape == (n, nd, nd) and (bias is None or bias.shape == (n, nd))
    assert kp6.numel() == 6 and kd6.numel() == 6
    assert q_rest is None or q_rest.numel() == nd
    assert effort_limit is None or effort_limit.numel() == nd
    goal = goal_pose.contiguous()
    out = torch.empty(n, nd, device=j_ee.device, dtype=torch.float32)
    with torch.cuda.device(j_ee.device):
        check(lib().shf_osc(_vp(j_ee.data_ptr()), j_ee.stride(0), _f32c(mass_matrix), None if bias is None else _f32c(bias),
                            _vp(dof_state.data_ptr()), dof_state.stride(1), _vp(ee_pose.data_ptr()), ee_pose.stride(0), _f32c(goal),
                            _f32c(kp6), _f32c(kd6), float(damping), None if q_rest is None else _f32c(q_rest), float(kp_null),
                            float(kd_null), None if effort_limit is None else _f32c(effort_limit), n, nd, _f32c(out),
                            _stream(j_ee.device)))
    return out


def _foot_args(j_feet, bias, effort_limit, mu=None):
    """What the foot controllers' wrappers check and prepare alike: j_feet (n, F, 6, nd + 6) is a float32 CUDA view with a
    foot's rows packed (any stride between feet and envs), bias (n, nd + 6) or None, effort_limit (nd) or None, mu a float or a
    (n) tensor.  Returns (n, F, nd, o, mu_args): o(t) is the pointer of a contiguous float32 copy of an optional tensor (None
    for None), kept referenced by o until the launch is enqueued; mu_args the (per-env pointer or None, scalar) pair."""
    n, F, six, D = j_feet.shape
    assert six == 6 and j_feet.stride(3) == 1 and j_feet.stride(2) == D
    assert j_feet.is_cuda and j_feet.dtype == torch.float32, "float32 CUDA tensors expected"
    assert bias is None or tuple(bias.shape) == (n, D)
    assert effort_limit is None or effort_limit.numel() == D - 6
    keep = []

    def o(t):
        if t is None:
            return None
        keep.append(t.contiguous())
        return _f32c(keep[-1])

    per_env = torch.is_tensor(mu) and mu.numel() > 1
    assert not per_env or mu.numel() == n
    return n, F, D - 6, o, (o(mu.reshape(n)) if per_env else None, 0.0 if per_env or mu is None else float(mu))


def foot_impedance(j_feet, dof_state, root_pose, foot_pos, target, kp3, kd3, bias=None, effort_limit=None):
    """LeggedRobot.foot_impedance_control in one launch (shf_foot_impedance): efforts (n, nd).  j_feet (n, F, 6, nd + 6): the
    foot rows of the floating-base Jacobian tensor (a view: rows packed inside a foot's block, any stride between feet and
    envs); dof_state as for osc; root_pose (n, >= 7) rows (pos, quat xyzw) and foot_pos (n, F, 3) world origins, unit stride
    in the last axis; target (n, F, 3) in the base frame; kp3 / kd3 (3); bias (n, nd + 6) or None; effort_limit (nd) or None."""
    n, F, nd, o, _ = _foot_args(j_feet, bias, effort_limit)
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (dof_state, root_pose, foot_pos)), "float32 CUDA tensors expected"
    assert dof_state.shape[:2] == (n, nd) and dof_state.shape[2] >= 2 and dof_state.stride(2) == 1
    assert dof_state.stride(1) >= 2 and dof_state.stride(0) == nd * dof_state.stride(1)
    assert root_pose.shape[0] == n and root_pose.shape[1] >= 7 and root_pose.stride(1) == 1
    assert foot_pos.shape == (n, F, 3) and foot_pos.stride(2) == 1 and tuple(target.shape) == (n, F, 3)
    assert kp3.numel() == 3 and kd3.numel() == 3
    out = torch.empty(n, nd, device=j_feet.device, dtype=torch.float32)
    with torch.cuda.device(j_feet.device):
        check(lib().shf_foot_impedance(_vp(j_feet.data_ptr()), j_feet.stride(0), j_feet.stride(1), _vp(dof_state.data_ptr()),
                                       dof_state.stride(1), _vp(root_pose.data_ptr()), root_pose.stride(0), _vp(foot_pos.data_ptr()),
                                       foot_pos.stride(0), foot_pos.stride(1), o(target), _f32c(kp3), _f32c(kd3), o(bias), o(effort_limit),
                                       n, F, nd, _f32c(out), _stream(j_feet.device)))
    return out


QP_ITERS = 100       # default sweeps of foot_force_qp (DESIGN.md 8h "Balance controller": what they leave of the optimum)


def foot_force_qp(j_feet, root_pose, foot_pos, stance, mu, weights6, wrench=None, mass_matrix=None, dyn_bias=None, base_target=None,
                  gains12=None, alpha=1e-2, beta=0.0, f_prev=None, fz_min=5.0, fz_max=float("inf"), iters=QP_ITERS, bias=None,
                  effort_limit=None):
    """LeggedRobot.balance_control in one launch (shf_foot_force_qp): (forces (n, F, 3), efforts (n, nd)).  j_feet, root_pose,
    foot_pos: views as for foot_impedance (root_pose rows of >= 13 floats (pos, quat, v, omega) unless `wrench` is given).
    stance (n, F) uint8 / bool; mu a float or a (n) tensor; weights6 (6).  The wanted base wrench: `wrench` (n, 6), or
    mass_matrix (n, nd + 6, nd + 6), dyn_bias (n, nd + 6), base_target (n, 13) and gains12 (12) = (kp_lin, kd_lin, kp_ang,
    kd_ang).  f_prev (n, F, 3) or None; bias (n, nd + 6) or None: added to the efforts; effort_limit (nd) or None."""
    n, F, nd, o, mu_args = _foot_args(j_feet, bias, effort_limit, mu)
    D = nd + 6
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (root_pose, foot_pos)), "float32 CUDA tensors expected"
    assert root_pose.shape[0] == n and root_pose.shape[1] >= (7 if wrench is not None else 13) and root_pose.stride(1) == 1
    assert foot_pos.shape == (n, F, 3) and foot_pos.stride(2) == 1
    assert tuple(stance.shape) == (n, F) and stance.dtype in (torch.uint8, torch.bool) and stance.is_cuda
    assert weights6.numel() == 6
    if wrench is None:
        assert mass_matrix is not None and dyn_bias is not None and base_target is not None and gains12 is not None, \
            "without a wrench: mass_matrix, dyn_bias, base_target and gains12"
        assert tuple(mass_matrix.shape) == (n, D, D) and tuple(dyn_bias.shape) == (n, D)
        assert tuple(base_target.shape) == (n, 13) and gains12.numel() == 12
    else:
        assert tuple(wrench.shape) == (n, 6)
    assert f_prev is None or tuple(f_prev.shape) == (n, F, 3)
    st = stance.contiguous().view(torch.uint8)
    forces = torch.empty(n, F, 3, device=j_feet.device, dtype=torch.float32)
    out = torch.empty(n, nd, device=j_feet.device, dtype=torch.float32)
    with torch.cuda.device(j_feet.device):
        check(lib().shf_foot_force_qp(_vp(j_feet.data_ptr()), j_feet.stride(0), j_feet.stride(1), _vp(root_pose.data_ptr()),
                                      root_pose.stride(0), _vp(foot_pos.data_ptr()), foot_pos.stride(0), foot_pos.stride(1),
                                      o(wrench), o(mass_matrix), o(dyn_bias), o(base_target), o(gains12), _vp(st.data_ptr()),
                                      *mu_args, o(weights6),
                                      float(alpha), float(beta), o(f_prev), float(fz_min), float(fz_max), int(iters), o(bias),
                                      o(effort_limit), n, F, nd, _f32c(forces), _f32c(out), _stream(j_feet.device)))
    return forces, out


def gain3(g, device, dtype=torch.float32):
    g = torch.as_tensor(g, dtype=dtype, device=device)
    return (g.expand(3) if g.dim() == 0 else g.reshape(3)).contiguous()


def _kernels():
    """The default set of primitives of balance_control / locomotion_control: this module's kernel wrappers.  The other set,
    utils.torch_utils.Primitives, presents the torch expressions under the same names and signatures."""
    import sys
    return sys.modules[__name__]


def balance_control(j_feet, root_state, foot_pos, contact_z, shape_friction, ground_friction, mass_matrix, bias, target, effort_limit,
                    base_pos, base_quat, base_lin_vel=None, base_ang_vel=None, stance=None, kp_lin=100., kd_lin=None, kp_ang=400.,
                    kd_ang=None, mu=None, fz_min=5., fz_max=None, weights=(1, 1, 1, 10, 10, 10), alpha=1e-2, beta=0.,
                    gravity_compensation=True, f_prev=None, prims=None):
    """What LeggedRobot.balance_control and FusedA1Env.balance_control share: the gains (kd None = 2 sqrt(kp)), the base target
    written into the caller's (n, 13) buffer `target`, stance None = the feet whose contact force z (contact_z (n, F)) exceeds
    1 N, mu None = the friction the simulator applies, (shape_friction (n) + ground_friction) / 2 -- formed per call, so it
    follows the friction tensor --, then foot_force_qp.  prims: the primitives it runs on (None = this module's kernels;
    constants are made in j_feet's dtype, float32 for those).  Returns (efforts, forces)."""
    prims = prims or _kernels()
    dev, T = j_feet.device, j_feet.dtype
    kpl, kpa = gain3(kp_lin, dev, T), gain3(kp_ang, dev, T)
    gains = torch.cat([kpl, 2.0 * torch.sqrt(kpl) if kd_lin is None else gain3(kd_lin, dev, T),
                       kpa, 2.0 * torch.sqrt(kpa) if kd_ang is None else gain3(kd_ang, dev, T)])
    target[:, :3], target[:, 3:7] = base_pos, base_quat
    target[:, 7:10] = 0.0 if base_lin_vel is None else base_lin_vel
    target[:, 10:13] = 0.0 if base_ang_vel is None else base_ang_vel
    if stance is None:
        stance = (contact_z > 1.0).to(torch.uint8)
    if mu is None:
        mu = 0.5 * (shape_friction + float(ground_friction))
    S = torch.as_tensor(weights, dtype=T, device=dev).reshape(6).contiguous()
    forces, efforts = prims.foot_force_qp(j_feet, root_state, foot_pos, stance, mu, S, None, mass_matrix, bias, target, gains, alpha, beta,
                                          f_prev if beta > 0 else None, fz_min, float("inf") if fz_max is None else float(fz_max),
                                          QP_ITERS, bias if gravity_compensation else None, effort_limit)
    return efforts, forces


# -- locomotion: gait plan -> foot-force QP -> swing spring -> merge (csrc/shf_gait.hip) ---------------------------------------
def gait_params(dt, height, touchdown_z, gait):
    """The by-value scalars of shf_gait_plan from a units.gait.Gait."""
    from ._abi import ShfGaitParams
    return ShfGaitParams(float(dt), float(height), gait.apex, float(touchdown_z), gait.late_depth, gait.k_fb, gait.max_step, gait.leash,
                         gait.contact_threshold)


def gait_plan(state, root_state, foot_pos, contact_z, command, nominal, reset, ticks, params):
    """One tick of the gait planner in one launch (shf_gait_plan): (stance (n, F) uint8, swing_target (n, F, 3) base frame,
    phase (n, F)).  state: a units.gait.GaitState, updated in place.  root_state (n, >= 13) rows and foot_pos (n, F, 3): views
    as for foot_impedance; contact_z (n, F) any strides, or None: the schedule alone decides the stance; command (n, 3) = (vx,
    vy, yaw rate) in the target's heading frame; nominal (F, 3): the feet in the base frame at the default pose; reset (n)
    uint8 / bool or None; ticks = (period_ticks, offset_ticks, stance_ticks) of Gait.ticks(dt); params: gait_params(...)."""
    n, F = foot_pos.shape[:2]
    P, offsets, stance_ticks = ticks
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (root_state, foot_pos, command, nominal)), "float32 CUDA tensors expected"
    assert root_state.shape[0] == n and root_state.shape[1] >= 13 and root_state.stride(1) == 1
    assert foot_pos.shape == (n, F, 3) and foot_pos.stride(2) == 1
    assert contact_z is None or (tuple(contact_z.shape) == (n, F) and contact_z.is_cuda and contact_z.dtype == torch.float32)
    assert tuple(command.shape) == (n, 3) and tuple(nominal.shape) == (F, 3)
    assert len(offsets) == F and len(stance_ticks) == F
    assert reset is None or (reset.numel() == n and reset.dtype in (torch.uint8, torch.bool) and reset.is_cuda)
    tick, sched, anchor, target, yaw = state.tensors()
    assert tick.dtype == torch.int32 and sched.dtype == torch.uint8 and tuple(sched.shape) == (n, F) and tuple(anchor.shape) == (n, F, 3)
    assert tuple(target.shape) == (n, 13) and yaw.numel() == n and all(t.is_cuda and t.is_contiguous() for t in state.tensors())
    dev = foot_pos.device
    cmd, nom = command.contiguous(), nominal.contiguous()
    rs = None if reset is None else reset.contiguous().view(torch.uint8)
    stance = torch.empty(n, F, dtype=torch.uint8, device=dev)
    swing = torch.empty(n, F, 3, dtype=torch.float32, device=dev)
    phase = torch.empty(n, F, dtype=torch.float32, device=dev)
    ia = C.c_int32 * F
    with torch.cuda.device(dev):
        check(lib().shf_gait_plan(_vp(root_state.data_ptr()), root_state.stride(0), _vp(foot_pos.data_ptr()), foot_pos.stride(0),
                                  foot_pos.stride(1), None if contact_z is None else _vp(contact_z.data_ptr()),
                                  0 if contact_z is None else contact_z.stride(0), 0 if contact_z is None else contact_z.stride(1),
                                  _f32c(cmd), _f32c(nom), None if rs is None else _vp(rs.data_ptr()), int(P),
                                  ia(*[int(o) for o in offsets]), ia(*[int(s) for s in stance_ticks]), params, _vp(tick.data_ptr()),
                                  _vp(sched.data_ptr()), _f32c(anchor), _f32c(target), _f32c(yaw), n, F, _vp(stance.data_ptr()),
                                  _f32c(swing), _f32c(phase), _stream(dev)))
    return stance, swing, phase


def leg_effort_mix(stance_efforts, swing_efforts, stance, chain_mask, effort_limit=None):
    """clamp(stance_efforts + m swing_efforts, +-effort_limit) in one launch (shf_leg_effort_mix): m = 1 on the dofs of the feet
    that are not in stance (chain_mask (F, nd) uint8: the dofs on each foot's chain), 0 elsewhere; limit entries <= 0: none."""
    n, nd = stance_efforts.shape
    F = stance.shape[1]
    assert tuple(swing_efforts.shape) == (n, nd) and tuple(stance.shape) == (n, F) and tuple(chain_mask.shape) == (F, nd)
    assert stance.dtype in (torch.uint8, torch.bool) and chain_mask.dtype == torch.uint8 and stance.is_cuda and chain_mask.is_cuda
    assert effort_limit is None or effort_limit.numel() == nd
    a, b = stance_efforts.contiguous(), swing_efforts.contiguous()
    st, cm = stance.contiguous().view(torch.uint8), chain_mask.contiguous()
    lim = None if effort_limit is None else effort_limit.contiguous()
    out = torch.empty(n, nd, device=a.device, dtype=torch.float32)
    with torch.cuda.device(a.device):
        check(lib().shf_leg_effort_mix(_f32c(a), _f32c(b), _vp(st.data_ptr()), _vp(cm.data_ptr()), None if lim is None else _f32c(lim),
                                       n, F, nd, _f32c(out), _stream(a.device)))
    return out


# -- actuator models: delay, PD or actuator net, strength, DC-motor clip in one launch (csrc/shf_actuator.hip) --------------------
def actuator_step(target, dof_state, cmd_hist, kp=None, kd=None, delay=0, strength=None, saturation=None, velocity_limit=None,
                  effort_limit=None, reset=None, net=None, err_hist=None, vel_hist=None, applied_out=None, efforts_out=None):
    """One simulation sub-step of the actuator model in one launch (shf_actuator_step): efforts (n, nd).  target (n, nd)
    contiguous; dof_state (n, nd, >= 2) as for osc (the dof-state tensor itself, read in place); cmd_hist (n, L, nd) and, with a
    net, err_hist / vel_hist (n, H, nd): the caller's state, contiguous, updated in place (slot 0 = this call).  kp / kd (nd)
    or (n, nd) (PD mode: net None); delay an int in 0..L-1 or a (n) int32 tensor (clamped to 0..L-1); strength (n, nd);
    saturation / velocity_limit / effort_limit (nd); reset (n) uint8 / bool; net: a units.actuators.ActuatorNet on the device
    (its padded weight buffer and host-side description).  applied_out / efforts_out (n, nd) contiguous: written when given
    (efforts_out None: a new tensor).  utils.torch_utils.actuator_step is the same algorithm as torch expressions."""
    from . import _abi
    n, nd = target.shape
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (target, dof_state, cmd_hist)), "float32 CUDA tensors expected"
    assert target.is_contiguous() and cmd_hist.is_contiguous() and cmd_hist.dim() == 3 and cmd_hist.shape[0] == n and cmd_hist.shape[2] == nd
    assert dof_state.shape[:2] == (n, nd) and dof_state.shape[2] >= 2 and dof_state.stride(2) == 1
    assert dof_state.stride(1) >= 2 and dof_state.stride(0) == nd * dof_state.stride(1)
    L = cmd_hist.shape[1]

    def o(t, shape, dtype=torch.float32):
        if t is None:
            return None
        assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda and t.is_contiguous(), (tuple(t.shape), shape, t.dtype)
        return _vp(t.data_ptr())

    stride = 0
    if net is None:
        assert kp is not None and kd is not None and kp.shape == kd.shape and tuple(kp.shape) in ((nd,), (n, nd)), "kp / kd: (nd) or (n, nd)"
        stride = nd if kp.dim() == 2 else 0
    per_env = torch.is_tensor(delay)
    rs = None if reset is None else reset.contiguous().view(torch.uint8)
    H = 1 if err_hist is None else err_hist.shape[1]
    out = torch.empty(n, nd, device=target.device, dtype=torch.float32) if efforts_out is None else efforts_out
    with torch.cuda.device(target.device):
        check(lib().shf_actuator_step(
            _f32c(target), _vp(dof_state.data_ptr()), dof_state.stride(1), None if net is not None else o(kp, tuple(kp.shape)),
            None if net is not None else o(kd, tuple(kd.shape)), stride, o(delay, (n,), torch.int32) if per_env else None,
            0 if per_env else int(delay), o(strength, (n, nd)), o(saturation, (nd,)), o(velocity_limit, (nd,)), o(effort_limit, (nd,)),
            o(rs, (n,), torch.uint8), _abi.ACTUATOR_PD if net is None else _abi.ACTUATOR_NET,
            None if net is None else C.byref(net.struct), None if net is None else _f32c(net.packed),
            0 if net is None else net.packed.numel(), _f32c(cmd_hist), L, o(err_hist, (n, H, nd)), o(vel_hist, (n, H, nd)), H, n, nd,
            o(applied_out, (n, nd)), o(out, (n, nd)), _stream(target.device)))
    return out


# -- proprioceptive sensors: IMUs, encoders and foot contact switches in one launch (csrc/shf_proprio.hip) -------------------------
def proprioception_step(body_state, dof_state, contact, config, params, delay, state, out, switches=None, reset=None, global_ids=None):
    """One sensor read of every env in one launch (shf_proprioception_step): fills and returns out (n, D).  body_state
    (n, nb, 13), dof_state (n, nd, >= 2), contact (n, nb, 3): float32 CUDA tensors or strided views of them with a contiguous
    last axis, read in place (body_state / contact may be None without IMUs / feet); config: the _abi.ShfProprioConfig
    (proprio.make_config); params (PROPRIO_NUM_PARAMS) float32 on the device (proprio.make_params); delay (n, 3) int32;
    state: proprio.make_state's tensors on the device, updated in place; out (n, D) float32 and switches (n, 2 F) uint8 or None,
    contiguous; reset (n) uint8 / bool or None (read, not cleared); global_ids (n) int64 or None: the ids that key the noise
    (None: config.env_id_offset + e).  utils.torch_utils.proprioception_step is the same algorithm as torch expressions."""
    from . import _abi, proprio
    n, nd = dof_state.shape[:2]
    I, F, L = config.num_imus, config.num_feet, config.slots

    def strided(t, width, name):
        if t is None:
            return None, 0, 0, 0
        assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and t.shape[0] == n and t.shape[2] >= width, f"{name}: (n, rows, >= {width}) float32 CUDA"
        assert t.stride(2) == 1 or t.shape[2] == 1, f"{name}: the last axis must be contiguous"
        return _vp(t.data_ptr()), t.stride(0), t.stride(1), t.shape[1]

    def own(t, shape, dtype, name):
        if t is None:
            return None
        assert tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_cuda and t.is_contiguous(), (name, tuple(t.shape), tuple(shape), t.dtype)
        return _vp(t.data_ptr())

    bp, be, br, nb = strided(body_state, 13, "body_state")
    dp, de, dr, _ = strided(dof_state, 2, "dof_state")
    cp, ce, cr, nbc = strided(contact, 3, "contact")
    assert body_state is None or contact is None or nb == nbc, "body_state and contact disagree about the bodies"
    shapes = proprio.state_shapes(n, I, nd, F, L)
    rs = None if reset is None else reset.contiguous().view(torch.uint8)
    with torch.cuda.device(dof_state.device):
        check(lib().shf_proprioception_step(
            bp, be, br, dp, de, dr, cp, ce, cr, own(rs, (n,), torch.uint8, "reset"), C.byref(config),
            own(params, (_abi.PROPRIO_NUM_PARAMS,), torch.float32, "params"), own(delay, (n, 3), torch.int32, "delay"),
            own(global_ids, (n,), torch.int64, "global_ids"),
            own(state["counter"], shapes["counter"], torch.int32, "counter"),
            own(state["imu"], shapes["imu"], torch.float32, "imu") if I else None,
            own(state["enc"], shapes["enc"], torch.float32, "enc"),
            own(state["foot"], shapes["foot"], torch.float32, "foot") if F else None,
            n, max(nb, nbc, 1), nd, own(out, (n, proprio.out_width(I, nd, F)), torch.float32, "out"),
            own(switches, (n, 2 * F), torch.uint8, "switches") if F else None, _stream(dof_state.device)))
    return out


# -- the horizon MPC: tables over the gait schedule -> condensed QP -> efforts (csrc/shf_mpc.hip) ---------------------------------
# The defaults (DESIGN.md 8h "Horizon MPC" says where each comes from): horizon steps, sweeps, force weight, ticks between two
# solves, and the weights of (roll, pitch, yaw, x, y, z, omega, v)
MPC_HORIZON, MPC_ITERS, MPC_ALPHA, MPC_EVERY = 10, 100, 1e-5, 1
MPC_WEIGHTS = (25.0, 25.0, 10.0, 2.0, 2.0, 50.0, 0.0, 0.0, 0.3, 0.2, 0.2, 0.2)


def mpc_step_dt(steps_per_tick, dt):
    """delta, the length of a horizon step, as shf_mpc_horizon forms it: the float32 product of the two."""
    import numpy as np
    return float(np.float32(steps_per_tick) * np.float32(dt))


def mpc_horizon(state, stance, foot_pos, command, nominal, ticks, params, horizon=MPC_HORIZON, steps_per_tick=1):
    """The MPC's tables in one launch (shf_mpc_horizon): (contact (n, H, F) uint8, xref (n, H + 1, 12), pos (n, H, F, 3)), from
    the GaitState as gait_plan left it this tick, gait_plan's stance (n, F), foot_pos (n, F, 3) (a view as for foot_impedance),
    command (n, 3), nominal (F, 3), ticks = Gait.ticks(dt), params = gait_params(...)."""
    n, F = foot_pos.shape[:2]
    P, offsets, stance_ticks = ticks
    H = int(horizon)
    assert foot_pos.is_cuda and foot_pos.dtype == torch.float32 and foot_pos.shape == (n, F, 3) and foot_pos.stride(2) == 1
    assert tuple(stance.shape) == (n, F) and stance.dtype in (torch.uint8, torch.bool) and stance.is_cuda
    assert tuple(command.shape) == (n, 3) and tuple(nominal.shape) == (F, 3) and len(offsets) == F and len(stance_ticks) == F
    tick, _, _, target, yaw = state.tensors()
    assert tick.dtype == torch.int32 and tuple(target.shape) == (n, 13) and yaw.numel() == n
    dev = foot_pos.device
    st, cmd, nom = stance.contiguous().view(torch.uint8), command.contiguous(), nominal.contiguous()
    contact = torch.empty(n, max(H, 0), F, dtype=torch.uint8, device=dev)
    xref = torch.empty(n, max(H, 0) + 1, 12, dtype=torch.float32, device=dev)
    pos = torch.empty(n, max(H, 0), F, 3, dtype=torch.float32, device=dev)
    ia = C.c_int32 * F
    with torch.cuda.device(dev):
        check(lib().shf_mpc_horizon(_vp(tick.data_ptr()), _f32c(target), _f32c(yaw), int(P), ia(*[int(o) for o in offsets]),
                                    ia(*[int(s) for s in stance_ticks]), _vp(st.data_ptr()), _vp(foot_pos.data_ptr()),
                                    foot_pos.stride(0), foot_pos.stride(1), _f32c(cmd), _f32c(nom), params, H, int(steps_per_tick), n, F,
                                    _vp(contact.data_ptr()), _f32c(xref), _f32c(pos), _stream(dev)))
    return contact, xref, pos


def foot_force_mpc(contact, xref, pos, root_state, mass_matrix, dyn_bias, j_feet, mu, weights12, alpha=MPC_ALPHA, fz_min=5.0,
                   fz_max=float("inf"), iters=MPC_ITERS, step_dt=0.03, bias=None, effort_limit=None, u_io=None, warm_shift=0,
                   forces_out=None):
    """The horizon MPC's solve in one launch (shf_foot_force_mpc): (forces (n, F, 3) = step 0 of the solution, efforts (n, nd)).
    contact, xref, pos: mpc_horizon's tables; root_state (n, >= 13) rows and j_feet (n, F, 6, nd + 6): views as for
    foot_force_qp; mass_matrix (n, nd + 6, nd + 6), dyn_bias (n, nd + 6); mu a float or a (n) tensor; weights12 (12); step_dt:
    mpc_step_dt(S, dt); bias (n, nd + 6) or None: added to the efforts; effort_limit (nd) or None; u_io (n, H, F, 3)
    contiguous or None: the warm start, read shifted by warm_shift steps and overwritten with the solution."""
    n, F, nd, o, mu_args = _foot_args(j_feet, bias, effort_limit, mu)
    D, H = nd + 6, contact.shape[1]
    assert all(t.is_cuda and t.dtype == torch.float32 for t in (root_state, xref, pos)), "float32 CUDA tensors expected"
    assert root_state.shape[0] == n and root_state.shape[1] >= 13 and root_state.stride(1) == 1
    assert tuple(contact.shape) == (n, H, F) and contact.dtype == torch.uint8 and contact.is_cuda
    assert tuple(xref.shape) == (n, H + 1, 12) and tuple(pos.shape) == (n, H, F, 3)
    assert tuple(mass_matrix.shape) == (n, D, D) and tuple(dyn_bias.shape) == (n, D) and weights12.numel() == 12
    assert u_io is None or (tuple(u_io.shape) == (n, H, F, 3) and u_io.is_contiguous() and u_io.is_cuda and u_io.dtype == torch.float32)
    ct = contact.contiguous()
    forces = torch.empty(n, F, 3, device=j_feet.device, dtype=torch.float32) if forces_out is None else forces_out
    out = torch.empty(n, nd, device=j_feet.device, dtype=torch.float32)
    with torch.cuda.device(j_feet.device):
        check(lib().shf_foot_force_mpc(_vp(ct.data_ptr()), o(xref), o(pos), _vp(root_state.data_ptr()), root_state.stride(0),
                                       o(mass_matrix), o(dyn_bias), _vp(j_feet.data_ptr()), j_feet.stride(0), j_feet.stride(1),
                                       *mu_args, o(weights12),
                                       float(alpha), float(fz_min), float(fz_max), int(iters), float(step_dt), o(bias),
                                       o(effort_limit), None if u_io is None else _f32c(u_io), int(warm_shift), n, H, F, nd,
                                       _f32c(forces), _f32c(out), _stream(j_feet.device)))
    return forces, out


def foot_force_efforts(forces, stance, j_feet, bias=None, effort_limit=None):
    """efforts (n, nd) = -sum over the feet with stance != 0 of Jl_f^T f_f, + bias[:, 6:], clamped to +-effort_limit, in one launch
    (shf_foot_force_efforts): the effort step of foot_force_qp / foot_force_mpc on its own, bit-equal to theirs."""
    n, F, nd, o, _ = _foot_args(j_feet, bias, effort_limit)
    assert tuple(forces.shape) == (n, F, 3) and tuple(stance.shape) == (n, F) and stance.dtype in (torch.uint8, torch.bool)
    st = stance.contiguous().view(torch.uint8)
    out = torch.empty(n, nd, device=j_feet.device, dtype=torch.float32)
    with torch.cuda.device(j_feet.device):
        check(lib().shf_foot_force_efforts(o(forces), _vp(st.data_ptr()), _vp(j_feet.data_ptr()), j_feet.stride(0), j_feet.stride(1),
                                           o(bias), o(effort_limit), n, F, nd, _f32c(out), _stream(j_feet.device)))
    return out


_CONSTANTS = {}


def _constant(values, device, dtype=torch.float32):
    """A small device tensor of python numbers, made once per value, device and dtype."""
    key = (str(device), dtype, tuple(float(v) for v in values))
    if key not in _CONSTANTS:
        _CONSTANTS[key] = torch.tensor(key[2], dtype=dtype, device=device)
    return _CONSTANTS[key]


def _vec3(g):
    g = [float(x) for x in (g.reshape(-1).tolist() if torch.is_tensor(g) else (g if hasattr(g, "__len__") else [g]))]
    return g * 3 if len(g) == 1 else g


def locomotion_control(j_feet, dof_state, root_state, foot_pos, contact_z, shape_friction, ground_friction, mass_matrix, bias,
                       effort_limit, chain_mask, nominal, state, command, gait, dt, height=0.30, touchdown_z=0.01, swing_kp=400.,
                       swing_kd=10., reset=None, kp_lin=100., kd_lin=None, kp_ang=400., kd_ang=None, mu=None, fz_min=5., fz_max=None,
                       weights=(1, 1, 1, 10, 10, 10), alpha=1e-2, gravity_compensation=True, controller="qp", horizon=MPC_HORIZON,
                       mpc_steps_per_tick=None, mpc_every=MPC_EVERY, mpc_weights=MPC_WEIGHTS, mpc_alpha=MPC_ALPHA, mpc_iters=MPC_ITERS,
                       prims=None):
    """What LeggedRobot.locomotion_control and FusedA1Env.locomotion_control share, four launches: the gait plan (base target
    and stance from `gait`'s schedule gated by contact_z, swing targets), foot_force_qp on that target and stance (as
    balance_control: kd None = 2 sqrt(kp), mu None = (shape_friction + ground_friction) / 2), foot_impedance towards the swing
    targets with the explicit swing_kp / swing_kd and no bias, and leg_effort_mix.  state: the GaitState, advanced by one tick;
    reset None = the state's pending resets.  controller="mpc": the stance forces come from the horizon MPC instead
    (csrc/shf_mpc.hip) -- mpc_horizon and foot_force_mpc in place of foot_force_qp every `mpc_every` ticks (and on the tick
    after a reset), `horizon` steps of mpc_steps_per_tick gait ticks (None = ceil(period_ticks / horizon): the horizon covers
    one gait period), warm-started from the last solve; on the ticks in between foot_force_efforts holds the last solve's forces
    on the current Jacobian (a foot that has lifted since counts as zero; `forces` is then the held solve's).  The QP's gains
    and weights are not read by the MPC.  prims: the primitives it runs on, as balance_control's.  Returns (efforts (n, nd),
    forces (n, F, 3), stance (n, F), swing_targets (n, F, 3))."""
    import math
    prims = prims or _kernels()
    dev, T = j_feet.device, j_feet.dtype
    if reset is None:
        reset = state.take_pending()
    ticks, params = gait.ticks(dt), prims.gait_params(dt, height, touchdown_z, gait)
    stance, swing_t, _ = prims.gait_plan(state, root_state, foot_pos, contact_z, command, nominal, reset, ticks, params)
    if mu is None:
        mu = 0.5 * (shape_friction + float(ground_friction))
    fz_max = float("inf") if fz_max is None else float(fz_max)
    tau_bias = bias if gravity_compensation else None
    if controller == "mpc":
        S = int(mpc_steps_per_tick) if mpc_steps_per_tick else -(-ticks[0] // int(horizon))
        u_io, held = state.mpc_buffers(horizon)
        if reset is not None:                        # a reset env starts cold, and everybody solves on this tick
            keep = (1 - reset.view(torch.uint8).to(u_io.dtype))
            u_io.mul_(keep.view(-1, 1, 1, 1))
            state.mpc_count = 0
        if state.mpc_count % max(int(mpc_every), 1) == 0:
            contact, xref, pos = prims.mpc_horizon(state, stance, foot_pos, command, nominal, ticks, params, horizon, S)
            forces, tau_st = prims.foot_force_mpc(contact, xref, pos, root_state, mass_matrix, bias, j_feet, mu,
                                                  _constant(mpc_weights, dev, T), mpc_alpha, fz_min, fz_max, mpc_iters, mpc_step_dt(S, dt),
                                                  tau_bias, effort_limit, u_io, int(mpc_every) // S, forces_out=held)
        else:
            forces = held
            tau_st = prims.foot_force_efforts(held, stance, j_feet, tau_bias, effort_limit)
        state.mpc_count += 1
    elif controller == "qp":
        kpl, kpa = _vec3(kp_lin), _vec3(kp_ang)
        kdl = [2.0 * math.sqrt(k) for k in kpl] if kd_lin is None else _vec3(kd_lin)
        kda = [2.0 * math.sqrt(k) for k in kpa] if kd_ang is None else _vec3(kd_ang)
        forces, tau_st = prims.foot_force_qp(j_feet, root_state, foot_pos, stance, mu, _constant(weights, dev, T), None, mass_matrix, bias,
                                             state.target, _constant(kpl + kdl + kpa + kda, dev, T), alpha, 0.0, None, fz_min, fz_max,
                                             QP_ITERS, tau_bias, effort_limit)
    else:
        raise ValueError(f"locomotion_control: controller {controller!r} (\"qp\" or \"mpc\")")
    tau_sw = prims.foot_impedance(j_feet, dof_state, root_state, foot_pos, swing_t, _constant(_vec3(swing_kp), dev, T),
                                  _constant(_vec3(swing_kd), dev, T), None, effort_limit)
    return prims.leg_effort_mix(tau_st, tau_sw, stance, chain_mask, effort_limit), forces, stance, swing_t
