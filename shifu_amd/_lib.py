"""ctypes binding of include/shifu_amd.h.  There is no CPU fallback: if the HIP
library is missing this module raises, and so does everything built on it."""
import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# SHIFU_AMD_LIB overrides the in-tree library (kernel A/B experiments only)
_PATH = os.environ.get("SHIFU_AMD_LIB") or os.path.join(_HERE, "libshifu_amd.so")
_lib = None

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
_SIGS = {
    "shf_abi_version": ([], i32),
    "shf_sim_create": ([C.POINTER(_abi.ShfSimParams), C.POINTER(vp)], i32),
    "shf_sim_destroy": ([vp], i32),
    "shf_sim_set_terrain": ([vp, C.POINTER(_abi.ShfTerrain)], i32),
    "shf_sim_set_articulation": ([vp, C.POINTER(_abi.ShfModel)], i32),
    "shf_model_bounds": ([C.POINTER(_abi.ShfModel)], i32),
    "shf_model_pgs_supported": ([C.POINTER(_abi.ShfModel), i32], i32),
    "shf_abb_step_pgs_is_wide": ([vp], i32),
    "shf_sim_add_box": ([vp, C.POINTER(_abi.ShfBoxDesc)], i32),
    "shf_sim_set_hulls": ([vp, C.POINTER(_abi.ShfHullSet)], i32),
    "shf_sim_set_scene_flags": ([vp, i32], i32),
    "shf_convex_manifold": ([i32, vp, vp, C.c_float, i32, vp, vp], i32),
    "shf_cap_select_test": ([i32, vp, vp, vp, vp, vp], i32),
    "shf_sim_finalize": ([vp, i32, i64], i32),
    "shf_sim_set_group": ([vp, i32], i32),
    "shf_sim_set_mapping": ([vp, i32], i32),
    "shf_sim_layout": ([vp, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)], i32),
    "shf_sim_bind": ([vp, i32, vp], i32),
    "shf_sim_reset_all": ([vp, vp, vp, vp, vp], i32),
    "shf_sim_step": ([vp, vp], i32),
    "shf_sim_step_plan": ([vp, C.POINTER(_abi.ShfLaunchPlan)], i32),
    "shf_sim_refresh": ([vp, i32, vp], i32),
    "shf_sim_dynamics": ([vp, vp, vp, vp], i32),
    "shf_sim_floating_dynamics": ([vp, vp, vp, vp, vp], i32),
    "shf_sim_set_dof_command": ([vp, i32, vp, vp], i32),
    "shf_sim_set_pos_target_indexed": ([vp, vp, vp, i32, vp], i32),
    "shf_sim_apply_body_force": ([vp, vp, vp], i32),
    "shf_sim_apply_body_force_at_pos": ([vp, vp, vp, vp], i32),
    "shf_sim_commit_root_indexed": ([vp, vp, vp, i32, vp], i32),
    "shf_sim_commit_root_all": ([vp, vp, vp], i32),
    "shf_sim_commit_dof_indexed": ([vp, vp, vp, i32, vp], i32),
    "shf_sim_commit_reset": ([vp, vp, vp, i32, vp, vp, vp, i32, vp], i32),
    "shf_sim_step_split_supported": ([vp], i32),
    "shf_a1_create": ([vp, C.POINTER(_abi.ShfA1TaskParams), C.POINTER(vp)], i32),
    "shf_a1_destroy": ([vp], i32),
    "shf_a1_layout": ([vp, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)], i32),
    "shf_a1_bind": ([vp, i32, vp], i32),
    "shf_a1_step": ([vp, vp, vp], i32),
    "shf_a1_step_random": ([vp, vp], i32),
    "shf_a1_step_plan": ([vp, C.POINTER(_abi.ShfLaunchPlan)], i32),
    "shf_a1_reset_all": ([vp, vp], i32),
    "shf_abb_create": ([vp, C.POINTER(_abi.ShfAbbTaskParams), C.POINTER(vp)], i32),
    "shf_abb_destroy": ([vp], i32),
    "shf_abb_layout": ([vp, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)], i32),
    "shf_abb_bind": ([vp, i32, vp], i32),
    "shf_abb_step": ([vp, vp, vp], i32),
    "shf_abb_step_random": ([vp, vp], i32),
    "shf_abb_step_plan": ([vp, C.POINTER(_abi.ShfLaunchPlan)], i32),
    "shf_abb_reset_all": ([vp, vp], i32),
    "shf_mlp_linear_forward": ([vp, vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "shf_mlp_linear_forward_ld": ([vp, i32, vp, vp, vp, i32, i32, i32, i32, i32, vp], i32),
    "shf_mlp_linear_backward_input": ([vp, vp, vp, vp, i32, i32, i32, vp], i32),
    "shf_mlp_backward_weight_workspace": ([i32, i32, i32, C.POINTER(i64)], i32),
    "shf_mlp_pack_bytes": ([i32, i32, C.POINTER(i64)], i32),
    "shf_mlp_pack_weights": ([vp, vp, i32, i32, vp], i32),
    "shf_mlp_panel_forward": ([vp, vp, vp, vp, i32, i32, i32, i32, vp], i32),
    "shf_mlp_panel_backward_input": ([vp, vp, vp, vp, i32, i32, i32, vp], i32),
    "shf_mlp_chain_forward": ([vp, i32, vp, vp], i32),
    "shf_mlp_chain_fits": ([vp], i32),
    "shf_mlp_set_precision": ([i32], i32),
    "shf_mlp_get_precision": ([], i32),
    "shf_mlp_linear_backward_weight": ([vp, vp, vp, vp, vp, vp, i32, i32, i32, vp], i32),
    "shf_copy_many": ([C.POINTER(vp), C.POINTER(vp), C.POINTER(i64), i32, vp], i32),
    "shf_episode_bookkeeping": ([vp, vp, i32, i64, vp, vp, vp, vp], i32),
    "shf_gather_rows": ([C.POINTER(vp), C.POINTER(vp), C.POINTER(i32), i32, vp, i64, vp], i32),
    "shf_adapt_lr": ([vp, vp] + [C.c_float] * 6 + [vp], i32),
    # library glue of the hook-compatible path (csrc/shf_glue.hip)
    "shf_base_frame_state": ([vp, vp, i64, i32, i32, vp, vp, vp, vp, vp], i32),
    "shf_get_heights": ([C.POINTER(_abi.ShfTerrain), vp, vp, vp, i64, vp, i32, i32, vp, vp], i32),
    "shf_history_add": ([vp, vp, i64, i32, vp], i32),
    "shf_rows_fill_indexed": ([vp, vp, i32, i64, i32, C.c_float, vp], i32),
    "shf_episode_log": ([C.POINTER(vp), i32, vp, i32, i64, C.c_float, vp, vp, vp], i32),
    "shf_reset_bookkeeping": ([C.POINTER(vp), i32, vp, i32, i64, C.c_float, vp, vp, vp, vp, i32, vp, i32, vp], i32),
    "shf_reset_dof_rows": ([vp, vp, vp, vp, i32, i64, i32, vp, vp, vp], i32),
    "shf_ik_dls": ([vp, i64, vp, i32, vp, i64, vp, i32, i32, C.c_float, vp, vp], i32),
    # j_ee, j_env_stride, mass_matrix, bias, dof_state, dof_elem_stride, ee_pose, ee_env_stride, goal_pose, kp6, kd6, damping,
    # q_rest, kp_null, kd_null, effort_limit, n, num_dof, efforts_out, stream
    "shf_osc": ([vp, i64, vp, vp, vp, i32, vp, i64, vp, vp, vp, C.c_float, vp, C.c_float, C.c_float, vp, i32, i32, vp, vp], i32),
    # j_feet, j_env_stride, j_foot_stride, dof_state, dof_elem_stride, root_pose, root_env_stride, foot_pos, foot_env_stride,
    # foot_stride, target, kp3, kd3, bias, effort_limit, n, num_feet, num_dof, efforts_out, stream
    "shf_foot_impedance": ([vp, i64, i64, vp, i32, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, i32, i32, i32, vp, vp], i32),
    # j_feet, j_env_stride, j_foot_stride, root_pose, root_env_stride, foot_pos, foot_env_stride, foot_stride, wrench, mass_matrix,
    # dyn_bias, base_target, gains12, stance, mu, mu_scalar, weights6, alpha, beta, f_prev, fz_min, fz_max, iters, bias,
    # effort_limit, n, num_feet, num_dof, forces_out, efforts_out, stream (csrc/shf_qp.hip)
    "shf_foot_force_qp": ([vp, i64, i64, vp, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, C.c_float, C.c_float, vp,
                           C.c_float, C.c_float, i32, vp, vp, i32, i32, i32, vp, vp, vp], i32),
    # root_pose, root_env_stride, foot_pos, foot_env_stride, foot_stride, contact_z, contact_env_stride, contact_foot_stride,
    # command, nominal, reset, period_ticks, offset_ticks (host), stance_ticks (host), params (by value), tick, sched, anchor,
    # target, yaw, n, num_feet, stance_out, swing_target_out, phase_out, stream (csrc/shf_gait.hip)
    "shf_gait_plan": ([vp, i64, vp, i64, i64, vp, i64, i64, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32), _abi.ShfGaitParams,
                       vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp], i32),
    # stance_efforts, swing_efforts, stance, chain_mask, effort_limit, n, num_feet, num_dof, efforts_out, stream
    "shf_leg_effort_mix": ([vp, vp, vp, vp, vp, i32, i32, i32, vp, vp], i32),
    # the horizon MPC (csrc/shf_mpc.hip).  tick, target, yaw, period_ticks, offset_ticks (host), stance_ticks (host), stance,
    # foot_pos, foot_env_stride, foot_stride, command, nominal, params (by value), horizon, ticks_per_step, n, num_feet,
    # contact_out, xref_out, pos_out, stream
    "shf_mpc_horizon": ([vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32), vp, vp, i64, i64, vp, vp, _abi.ShfGaitParams, i32, i32, i32,
                         i32, vp, vp, vp, vp], i32),
    # contact, xref, pos, root_pose, root_env_stride, mass_matrix, dyn_bias, j_feet, j_env_stride, j_foot_stride, mu, mu_scalar,
    # weights12, alpha, fz_min, fz_max, iters, step_dt, bias, effort_limit, u_io, warm_shift, n, horizon, num_feet, num_dof,
    # forces_out, efforts_out, stream
    "shf_foot_force_mpc": ([vp, vp, vp, vp, i64, vp, vp, vp, i64, i64, vp, C.c_float, vp, C.c_float, C.c_float, C.c_float, i32,
                            C.c_float, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp], i32),
    # forces, stance, j_feet, j_env_stride, j_foot_stride, bias, effort_limit, n, num_feet, num_dof, efforts_out, stream
    "shf_foot_force_efforts": ([vp, vp, vp, i64, i64, vp, vp, i32, i32, i32, vp, vp], i32),
    # actuator models (csrc/shf_actuator.hip).  target, dof_state, dof_elem_stride, kp, kd, gain_env_stride, delay, delay_scalar,
    # strength, saturation, velocity_limit, effort_limit, reset, mode, net (host struct), weights, weights_count, cmd_hist,
    # cmd_slots, err_hist, vel_hist, hist_slots, n, num_dof, applied_target_out, efforts_out, stream
    "shf_actuator_step": ([vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(_abi.ShfActuatorNet), vp, i64, vp,
                           i32, vp, vp, i32, i32, i32, vp, vp, vp], i32),
    # proprioceptive sensors (csrc/shf_proprio.hip).  body_state, its env and row strides, dof_state, its strides, contact, its
    # strides, reset, config (host struct), params, delay, global_ids, counter, imu_state, enc_state, foot_state, n, num_bodies, num_dof, out,
    # switch_out, stream
    "shf_proprioception_step": ([vp, i64, i64, vp, i64, i64, vp, i64, i64, vp, C.POINTER(_abi.ShfProprioConfig), vp, vp, vp, vp, vp, vp, vp,
                                 i32, i32, i32, vp, vp, vp], i32),
    "shf_reward_accumulate": ([C.POINTER(vp), C.POINTER(vp), i32, i64, vp, vp], i32),
    "shf_gae": ([vp, vp, vp, vp, i32, i64, C.c_float, C.c_float, vp, vp], i32),
    "shf_ppo_loss_workspace": ([i64, i32, C.POINTER(i64)], i32),
    "shf_ppo_loss": ([vp] * 10 + [i64, i32, C.c_float, C.c_float, C.c_float, i32] + [vp] * 6, i32),
    # camera sensors (csrc/shf_render.hip)
    "shf_render_cameras": ([vp, C.POINTER(_abi.ShfTerrain), vp, C.POINTER(_abi.ShfCamera), i32] + [vp] * 7 + [vp], i32),
    # ... with optical flow: the same arguments, then prev_body_pose, prev_cam_pose, prev_valid, flow, flow_i16, stream
    "shf_render_cameras_flow": ([vp, C.POINTER(_abi.ShfTerrain), vp, C.POINTER(_abi.ShfCamera), i32] + [vp] * 7 + [vp] * 5 + [vp], i32),
    # world view: scene, terrain, heights, camera, num_views, view_pose, num_envs, num_drawn, env_ids, env_offset, env_radius,
    # body_state, seg_ids, colors, depth, seg, rgba, env, stream
    "shf_render_world": ([vp, C.POINTER(_abi.ShfTerrain), vp, C.POINTER(_abi.ShfCamera), i32, vp, i32, i32, vp, vp, C.c_float]
                         + [vp] * 3 + [vp] * 4 + [vp], i32),
    # ray caster: scene, terrain, heights, num_envs, num_rays, ray_origin, ray_dir, body_state, sensor_pose, align, min_range,
    # max_range, shape_mask, seg_ids, dist, points, normal, seg, body, stream
    "shf_raycast": ([vp, C.POINTER(_abi.ShfTerrain), vp, i32, i32, vp, vp, vp, vp, i32, C.c_float, C.c_float, C.c_uint64, vp]
                    + [vp] * 5 + [vp], i32),
    "shf_raycast_debug_cull": ([i32], i32),
    # camera, num_envs, depth, cam_pose, world_frame, points, stream
    "shf_camera_points": ([C.POINTER(_abi.ShfCamera), i32, vp, vp, i32, vp, vp], i32),
    # conv-encoder inference (csrc/shf_conv.hip)
    "shf_conv_pack_bytes": ([i32, i32, C.POINTER(i64)], i32),
    "shf_conv_pack_weights": ([vp, vp, i32, i32, vp], i32),
    "shf_conv3x3s2_forward": ([vp, i32, C.POINTER(i64), vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp], i32),
    # LSTM cell step of the recurrent policy (csrc/shf_lstm.hip)
    "shf_lstm_pack_bytes": ([i32, i32, C.POINTER(i64)], i32),
    "shf_lstm_pack_weights": ([vp, vp, vp, i32, i32, vp], i32),
    "shf_lstm_cell_forward": ([vp, i32] + [vp] * 9 + [i32, i32, i32, vp], i32),
    "shf_lstm_cell_backward_pointwise": ([vp] * 8 + [i32, i32, vp], i32),
    # GRU cell step of the recurrent policy (csrc/shf_gru.hip)
    "shf_gru_pack_bytes": ([i32, i32, C.POINTER(i64)], i32),
    "shf_gru_pack_weights": ([vp, vp, vp, i32, i32, vp], i32),
    "shf_gru_cell_forward": ([vp, i32] + [vp] * 7 + [i32, i32, i32, vp], i32),
    "shf_gru_cell_backward_pointwise": ([vp] * 7 + [i32, i32, vp], i32),
}
EXPORTS = sorted(list(_SIGS) + ["shf_last_error", "shf_mlp_last_error", "shf_conv_last_error"])


class BackendError(RuntimeError):
    pass


def lib():
    """The loaded HIP library.  torch is imported first so that the HIP runtime
    already in the process (torch's bundled libamdhip64.so.7) is the one used."""
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise BackendError(f"{_PATH} is missing: build it with `python -m shifu_amd.build` "
                               "(there is no CPU fallback for the MI355X backend)")
        import torch  # noqa: F401  (loads the process-wide HIP runtime)
        l = C.CDLL(_PATH)
        for name, (args, res) in _SIGS.items():
            f = getattr(l, name)
            f.argtypes, f.restype = args, res
        l.shf_last_error.restype = C.c_char_p
        l.shf_mlp_last_error.restype = C.c_char_p
        l.shf_conv_last_error.restype = C.c_char_p
        if l.shf_abi_version() != _abi.SHF_ABI_VERSION:
            raise BackendError("libshifu_amd.so ABI version mismatch: rebuild")
        _lib = l
    return _lib


def check(rc: int):
    if rc != 0:
        raise BackendError(lib().shf_last_error().decode())
