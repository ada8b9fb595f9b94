"""Robot / ArmRobot / LeggedRobot (reference shifu/units/robot.py:11-236).

The tensors here are views into the sim's state tensors taken once in init_buffers
(`dof_pos` / `dof_vel` are strided views of dof_state, robot.py:51-52) and stay valid
because the backend's buffers are pointer-stable.  Every `self.gym.*` call goes to the
MI355X backend through the gymapi facade."""
import torch

from shifu_amd.isaacgym import gymapi, gymtorch
from shifu_amd.isaacgym.torch_utils import get_axis_params, quat_conjugate, quat_mul, quat_rotate_inverse, to_torch

from .units import Actor


class Robot(Actor):
    def reset_idx(self, env_ids):
        self._reset_dof_state(env_ids)
        self._reset_root_state(env_ids)
        if getattr(self, "actuator", None) is not None:
            self.actuator.reset(env_ids)
        for sensor in getattr(self, "proprioception_sensors", ()):       # units.ProprioceptionSensor: a reset is a teleport
            sensor.reset(env_ids)

    def step(self, actions):
        self._internal_motor_step(actions)

    # -- actuator models (not in the reference; units/actuators.py, csrc/shf_actuator.hip) ------------------------------------
    def set_actuator(self, actuator):
        """Puts an Actuator (units.actuators: PD with delay, DC motor, actuator net) between apply_actuator_targets' joint angles
        and the joint efforts; None takes it away.  The asset must be in DOF_MODE_EFFORT.  Call it once the buffers exist
        (after create_envs); the actuator is bound to this robot's envs, dofs and device."""
        if actuator is None:
            self.actuator = None
            return
        if self.asset_options.default_dof_drive_mode != gymapi.DOF_MODE_EFFORT:
            raise RuntimeError("set_actuator: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT")
        actuator.bind(self.env.num_envs, self.num_dof, self.device)
        self.actuator = actuator

    def apply_actuator_targets(self, dof_targets):
        """decimation x {actuator.efforts (one launch), set the efforts, simulate, refresh the dof state}: apply_dof_targets
        through the robot's actuator model.  dof_targets (num_envs, num_dof): the desired joint angles."""
        act = getattr(self, "actuator", None)
        if act is None:
            raise RuntimeError("apply_actuator_targets: no actuator (set_actuator first)")
        n = self.env.num_envs
        ds = self.env.dof_state.view(n, self.num_dof, 2)
        for _ in range(int(self.env.decimation)):
            efforts = act.efforts(dof_targets, ds)
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(efforts))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)
        return efforts

    def _init_props(self):
        super()._init_props()
        # written even in EFFORT mode (Q11); the backend ignores drive gains for EFFORT dofs
        self.dof_props['driveMode'][:] = self.asset_options.default_dof_drive_mode
        self.dof_props['stiffness'] = self.cfg.dof_stiffness
        self.dof_props['damping'] = self.cfg.dof_damping
        self.dof_lower_limits = to_torch(self.dof_props['lower'], device=self.device)
        self.dof_upper_limits = to_torch(self.dof_props['upper'], device=self.device)
        self.dof_vel_limits = to_torch(self.dof_props['velocity'], device=self.device)
        self.torque_limits = to_torch(self.dof_props['effort'], device=self.device)

    def load_to(self, env_id, env_handle, seg_id):
        super().load_to(env_id, env_handle, seg_id)
        self.gym.set_actor_dof_properties(env_handle, self.actor_handle, self.dof_props)

    def init_buffers(self):
        super().init_buffers()
        n = self.env.num_envs
        self.default_dof_pos = to_torch(self.cfg.default_dof_pos, device=self.device)
        self.dof_pos = self.env.dof_state.view(n, self.num_dof, 2)[..., 0]
        self.dof_vel = self.env.dof_state.view(n, self.num_dof, 2)[..., 1]
        self.dof_targets = torch.zeros((n, self.num_dof), dtype=torch.float, device=self.device)

    def _internal_motor_step(self, action):
        mode = self.asset_options.default_dof_drive_mode
        if mode == gymapi.DOF_MODE_EFFORT:
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(action))
        elif mode == gymapi.DOF_MODE_POS:
            self.gym.set_dof_position_target_tensor(self.sim, gymtorch.unwrap_tensor(action))
        elif mode == gymapi.DOF_MODE_VEL:
            self.gym.set_dof_velocity_target_tensor(self.sim, gymtorch.unwrap_tensor(action))
        else:
            raise NotImplementedError

    def apply_dof_targets(self, dof_targets):
        """decimation x {set targets, simulate, refresh dof state} (robot.py:66-72)."""
        for _ in range(int(self.env.decimation)):
            self.gym.set_dof_position_target_tensor(self.sim, gymtorch.unwrap_tensor(dof_targets))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)

    def _reset_dof_state(self, env_ids):
        ds = self.env.dof_state
        if ds.is_cuda and torch.is_tensor(env_ids) and env_ids.is_cuda and env_ids.dtype == torch.int64 \
                and ds.shape[0] == self.env.num_envs * self.num_dof:
            # the four statements below as one launch (csrc/shf_glue.hip: shf_reset_dof_rows); only a robot owns dofs
            # (robot.py:51-52 views dof_state as (N, num_dof, 2)), so env e's block starts at e * num_dof
            from shifu_amd import glue
            actor_ids = glue.reset_dof_rows(ds, self.dof_targets, self.default_dof_pos, env_ids, self.root_indices)
        else:
            self.dof_targets[env_ids] = self.default_dof_pos.clone()
            self.dof_pos[env_ids] = self.default_dof_pos.clone()
            self.dof_vel[env_ids] = 0.
            actor_ids = self.root_indices[env_ids].to(torch.int32)
        self.gym.set_dof_position_target_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.dof_targets),
                                                        gymtorch.unwrap_tensor(actor_ids), len(actor_ids))
        self.gym.set_dof_state_tensor_indexed(self.sim, gymtorch.unwrap_tensor(self.env.dof_state),
                                              gymtorch.unwrap_tensor(actor_ids), len(env_ids))

    def get_root_state(self):
        return self.env.root_state[self.root_indices]

    def set_root_state(self, root_state):
        self.env.root_state[self.root_indices] = root_state
        self.gym.set_actor_root_state_tensor(self.sim, gymtorch.unwrap_tensor(self.env.root_state))


class ArmRobot(Robot):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.end_effector_names = cfg.end_effector_names
        self.end_effector_velocity = cfg.end_effector_velocity

    def init_buffers(self):
        super().init_buffers()
        ee = [self.rigid_body_dict[n] for n in self.cfg.end_effector_names]
        self.ee_indices = to_torch(ee, dtype=torch.long, device=self.device)
        self.num_ee = len(ee)
        self.contact_forces = self.env.contact_state.view(self.env.num_envs, -1, 3)
        self.ee_pose_targets = torch.zeros((self.env.num_envs, 7), dtype=torch.float, device=self.device)
        jac = gymtorch.wrap_tensor(self.gym.acquire_jacobian_tensor(self.sim, self.name))
        self.gym.refresh_jacobian_tensors(self.sim)
        self.j_ee = jac[:, ee[0] - 1]   # a fixed base has no Jacobian row (robot.py:128)
        self._ee0 = int(ee[0])

    def load_to(self, env_id, env_handle, seg_id):
        super().load_to(env_id, env_handle, seg_id)
        self.set_segmentation_id(env_handle, seg_id)

    def apply_target_end_positions(self, tar_pose):
        self.dof_targets[:] = self.inverse_kinematics(tar_pose)
        self.apply_dof_targets(self.dof_targets)

    @property
    def body_state(self):
        n = self.env.num_envs
        return self.env.body_state.view(n, -1, 13)[:, :self.num_bodies].view(n, self.num_bodies, -1)

    @property
    def ee_pose(self):
        return self.body_state[:, self.ee_indices, :7]

    @property
    def ee_vel(self):
        return self.body_state[:, self.ee_indices, 7:]

    @property
    def ee_forces(self):
        return self.contact_forces[:, self.ee_indices]

    @staticmethod
    def orientation_error(desired, current):
        q_r = quat_mul(desired, quat_conjugate(current))
        return q_r[:, 0:3] * torch.sign(q_r[:, 3]).unsqueeze(-1)

    def inverse_kinematics(self, goal_pose, damping=0.05):
        """Damped least squares on the EE Jacobian (robot.py:162-182)."""
        if self.j_ee.is_cuda and self.j_ee.dim() == 3 and self.j_ee.dtype == torch.float32 and goal_pose.is_cuda \
                and hasattr(self, "_ee0"):
            # the expressions below as one launch (csrc/shf_glue.hip: shf_ik_dls, LDL^T instead of torch.inverse)
            from shifu_amd import glue
            n = self.env.num_envs
            ee = self.env.body_state.view(n, -1, 13)[:, self._ee0, :7]
            return glue.ik_dls(self.j_ee, self.dof_pos, ee, goal_pose, damping)
        ee_pos, ee_quat = self.ee_pose[:, 0, :3], self.ee_pose[:, 0, 3:7]
        dpose = torch.cat([goal_pose[:, :3] - ee_pos, self.orientation_error(goal_pose[:, 3:7], ee_quat)],
                          -1).unsqueeze(-1)
        jt = torch.transpose(self.j_ee, 1, 2)
        lam = torch.eye(6, device=self.device) * (damping ** 2)
        u = (jt @ torch.inverse(self.j_ee @ jt + lam) @ dpose).view(self.env.num_envs, self.num_dof)
        return self.dof_pos + u

    # -- torque-level control (not in the reference: the controller of Isaac Gym's own arm examples) ---------------------
    @property
    def mass_matrix(self):
        """(num_envs, nd, nd) joint-space mass matrix; gym.refresh_mass_matrix_tensors fills it."""
        if getattr(self, "_mass_matrix", None) is None:
            self._mass_matrix = gymtorch.wrap_tensor(self.gym.acquire_mass_matrix_tensor(self.sim, self.name))
        return self._mass_matrix

    @property
    def bias_forces(self):
        """(num_envs, nd) gravity + Coriolis + centrifugal joint forces; gym.refresh_mass_matrix_tensors fills it."""
        if getattr(self, "_bias_forces", None) is None:
            self._bias_forces = gymtorch.wrap_tensor(self.gym.acquire_dof_bias_force_tensor(self.sim, self.name))
        return self._bias_forces

    def _gain6(self, g):
        g = torch.as_tensor(g, dtype=torch.float32, device=self.device)
        return (g.expand(6) if g.dim() == 0 else g.reshape(6)).contiguous()

    def operational_space_control(self, goal_pose, kp=150., kd=None, damping=0., gravity_compensation=True, q_rest=None,
                                  kp_null=10., kd_null=None):
        """Efforts (num_envs, nd) that drive the end effector to goal_pose (n, 7): u = J^T Lambda (kp e - kd xdot),
        Lambda = (J M^-1 J^T + damping^2 I)^-1, from the Jacobian, mass-matrix, dof and body tensors as last refreshed.
        kp / kd: scalars or 6-vectors; kd None = critical damping 2 sqrt(kp).  gravity_compensation adds bias_forces.
        q_rest (nd), for arms with more than 6 dofs: a posture task in the null space of the end effector (kd_null None =
        2 sqrt(kp_null)).  Clamped to the asset's effort limits."""
        kp6 = self._gain6(kp)
        kd6 = 2.0 * torch.sqrt(kp6) if kd is None else self._gain6(kd)
        if kd_null is None:
            kd_null = 2.0 * float(kp_null) ** 0.5
        bias = self.bias_forces if gravity_compensation else None
        M = self.mass_matrix
        if q_rest is not None:
            q_rest = torch.as_tensor(q_rest, dtype=torch.float32, device=self.device).reshape(self.num_dof).contiguous()
        n = self.env.num_envs
        if self.j_ee.is_cuda and self.j_ee.dim() == 3 and self.j_ee.dtype == torch.float32 and goal_pose.is_cuda \
                and hasattr(self, "_ee0"):
            # the expressions of utils.torch_utils.operational_space_control as one launch (csrc/shf_glue.hip: shf_osc)
            from shifu_amd import glue
            ee = self.env.body_state.view(n, -1, 13)[:, self._ee0, :7]
            return glue.osc(self.j_ee, M, bias, self.env.dof_state.view(n, self.num_dof, 2), ee, goal_pose, kp6, kd6, damping,
                            q_rest, kp_null, kd_null, self.torque_limits.contiguous())
        from shifu_amd.utils.torch_utils import operational_space_control
        ee_pos, ee_quat = self.ee_pose[:, 0, :3], self.ee_pose[:, 0, 3:7]
        return operational_space_control(self.j_ee, M, self.dof_pos, self.dof_vel, ee_pos, ee_quat, goal_pose[:, :3],
                                         goal_pose[:, 3:7], kp6, kd6, damping, bias, q_rest, kp_null, kd_null, self.torque_limits)

    def apply_target_end_positions_osc(self, tar_pose, **gains):
        """decimation x {refresh dof / body / Jacobian / mass matrix / bias, compute efforts, set them, simulate, refresh the
        dof state}: apply_target_end_positions at torque level.  The asset must be in DOF_MODE_EFFORT."""
        if self.asset_options.default_dof_drive_mode != gymapi.DOF_MODE_EFFORT:
            raise RuntimeError("apply_target_end_positions_osc: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT")
        self.mass_matrix, self.bias_forces      # acquired before the first refresh
        for _ in range(int(self.env.decimation)):
            self.gym.refresh_all_state_tensors(self.sim)      # dof, body and Jacobian tensors among them, one backend call
            self.gym.refresh_mass_matrix_tensors(self.sim)
            efforts = self.operational_space_control(tar_pose, **gains)
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(efforts))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)


class LeggedRobot(ArmRobot):
    def __init__(self, cfg):
        Robot.__init__(self, cfg)        # the reference skips ArmRobot.__init__ (robot.py:190)
        self.end_effector_names = cfg.end_effector_names
        self.ee_indices = []

    def init_buffers(self):
        Robot.init_buffers(self)
        n = self.env.num_envs
        ee = [self.rigid_body_dict[k] for k in self.cfg.end_effector_names]
        self.ee_indices = to_torch(ee, dtype=torch.long, device=self.device)
        self.num_ee = len(ee)
        self.contact_forces = self.env.contact_state.view(n, -1, 3)
        jac = gymtorch.wrap_tensor(self.gym.acquire_jacobian_tensor(self.sim, self.name))
        self.gym.refresh_jacobian_tensors(self.sim)
        self.j_ee = jac[:, ee]
        self._jac, self._ee_list = jac, [int(b) for b in ee]
        self.gravity_vec = to_torch(get_axis_params(-1., self.env.up_axis_idx), device=self.device).repeat((n, 1))
        quat = self.base_pose[:, 3:7]
        self.base_lin_vel = quat_rotate_inverse(quat, self.env.root_state[self.root_indices, 7:10])
        self.base_ang_vel = quat_rotate_inverse(quat, self.env.root_state[self.root_indices, 10:13])
        self.projected_gravity = quat_rotate_inverse(quat, self.gravity_vec)

    def step(self, actions):
        self.dof_targets[:] = self.dof_pos[:, :self.num_dof] + actions
        self.apply_dof_targets(self.dof_targets)
        self.post_step()

    def post_step(self):
        """Base-frame velocities from the root_state TENSOR -- which has not been refreshed
        since the previous env step (Q2)."""
        n = self.env.num_envs
        rs = self.env.root_state
        if rs.is_cuda:
            # the four expressions below as one launch (csrc/shf_glue.hip: shf_base_frame_state)
            from shifu_amd import glue
            if glue.usable(rs, self.base_lin_vel, self.base_ang_vel, self.projected_gravity, self.gravity_vec):
                glue.base_frame_state(rs, self.root_indices, self.env.up_axis_idx, self.base_lin_vel, self.base_ang_vel,
                                      self.projected_gravity, self.gravity_vec)
                return
        self.gravity_vec[:] = to_torch(get_axis_params(-1., self.env.up_axis_idx), device=self.device).repeat((n, 1))
        quat = self.base_pose[:, 3:7]
        self.base_lin_vel[:] = quat_rotate_inverse(quat, self.env.root_state[self.root_indices, 7:10])
        self.base_ang_vel[:] = quat_rotate_inverse(quat, self.env.root_state[self.root_indices, 10:13])
        self.projected_gravity[:] = quat_rotate_inverse(quat, self.gravity_vec)

    def apply_force_on_base(self, force_tensor, pos_tensor=None):
        self.gym.apply_rigid_body_force_at_pos_tensors(
            self.sim, gymtorch.unwrap_tensor(force_tensor),
            gymtorch.unwrap_tensor(pos_tensor) if pos_tensor is not None else None)

    # -- whole-body dynamics and Cartesian foot control (not in the reference; SHIFU_AMD_FLOATING_DYNAMICS=1) --------------
    # mass_matrix (num_envs, nd + 6, nd + 6) and bias_forces (num_envs, nd + 6) are ArmRobot's properties: for a floating base
    # the facade hands them out in the order nu = (root linear, root angular, dofs) of csrc/shf_dyn.h, and refuses them
    # ("fixed base") while the variable is unset.
    def _end_rows(self, t):
        """t[:, end bodies]: a view where the end bodies are evenly spaced (the A1's feet), else a copy."""
        ee = self._ee_list
        step = ee[1] - ee[0] if len(ee) > 1 else 1
        if step > 0 and all(b - a == step for a, b in zip(ee, ee[1:])):
            return t[:, ee[0]:ee[-1] + 1:step]
        return t[:, ee]

    @property
    def foot_jacobians(self):
        """(num_envs, num_ee, 6, nd + 6): the end bodies' rows of the Jacobian tensor as last refreshed."""
        return self._end_rows(self._jac)

    def _gain3(self, g):
        g = torch.as_tensor(g, dtype=torch.float32, device=self.device)
        return (g.expand(3) if g.dim() == 0 else g.reshape(3)).contiguous()

    def foot_impedance_control(self, targets, kp=200., kd=None, gravity_compensation=True):
        """Efforts (num_envs, nd) of a Cartesian spring-damper that pulls every end body to targets (n, num_ee, 3), positions
        in the base frame: per foot F = R (kp (target - p) - kd pd) with p, pd the foot's position and velocity relative to
        the base in base axes, tau = sum J^T F over the dof columns of the foot's linear Jacobian rows; from the Jacobian,
        dof, root and body tensors as last refreshed.  kp / kd: scalars or 3-vectors; kd None = 2 sqrt(kp).
        gravity_compensation adds bias_forces[:, 6:].  Clamped to the asset's effort limits."""
        bias = self.bias_forces                  # (refused with "fixed base" unless SHIFU_AMD_FLOATING_DYNAMICS=1)
        if not gravity_compensation:
            bias = None
        kp3 = self._gain3(kp)
        kd3 = 2.0 * torch.sqrt(kp3) if kd is None else self._gain3(kd)
        n = self.env.num_envs
        jf = self.foot_jacobians
        root = self.env.root_state.view(n, -1, 13)[:, 0]
        feet = self._end_rows(self.env.body_state.view(n, -1, 13))[..., :3]
        if jf.is_cuda and jf.dtype == torch.float32 and targets.is_cuda:
            # the expressions of utils.torch_utils.foot_impedance_control as one launch (csrc/shf_glue.hip: shf_foot_impedance)
            from shifu_amd import glue
            return glue.foot_impedance(jf, self.env.dof_state.view(n, self.num_dof, 2), root, feet, targets, kp3, kd3, bias,
                                       self.torque_limits.contiguous())
        from shifu_amd.utils.torch_utils import foot_impedance_control
        return foot_impedance_control(jf, self.dof_vel, root[:, :3], root[:, 3:7], feet, targets, kp3, kd3, bias, self.torque_limits)

    def apply_target_foot_positions(self, targets, **gains):
        """decimation x {refresh the state, Jacobian, mass-matrix and bias tensors, compute efforts, set them, simulate, refresh
        the dof state}.  The asset must be in DOF_MODE_EFFORT."""
        if self.asset_options.default_dof_drive_mode != gymapi.DOF_MODE_EFFORT:
            raise RuntimeError("apply_target_foot_positions: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT")
        self.mass_matrix, self.bias_forces      # acquired before the first refresh
        for _ in range(int(self.env.decimation)):
            self.gym.refresh_all_state_tensors(self.sim)
            self.gym.refresh_mass_matrix_tensors(self.sim)
            efforts = self.foot_impedance_control(targets, **gains)
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(efforts))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)

    # -- balance control: the stance feet's forces from a QP (not in the reference; SHIFU_AMD_FLOATING_DYNAMICS=1) ----------
    def _contact_friction(self):
        """(num_envs) the friction coefficient the simulator applies between this robot's shapes and the ground, as it stands."""
        from shifu_amd import _abi
        be = self.sim.backend
        return 0.5 * (be.tensors[_abi.T_FRICTION] + float(be.terrain.friction)).to(self.device)

    def _foot_dof_mask(self):
        """(num_ee, nd): 1 where a dof lies on the chain from the root to an end body."""
        if getattr(self, "_bal_chain", None) is None:
            m = self.sim.backend.model
            mask = torch.zeros(len(self._ee_list), self.num_dof)
            for f, b in enumerate(self._ee_list):
                while b > 0:
                    if m.dof[b] >= 0:
                        mask[f, m.dof[b]] = 1.0
                    b = m.parent[b]
            self._bal_chain = mask.to(self.device)
        return self._bal_chain

    @staticmethod
    def _control_prims(*tensors):
        """The primitives glue's control sequences run on: the kernels (None) for float32 CUDA tensors, else their torch expressions."""
        if all(t.is_cuda and t.dtype == torch.float32 for t in tensors):
            return None
        from shifu_amd.utils.torch_utils import Primitives
        return Primitives

    def stance_from_contacts(self, threshold=1.0):
        """(num_envs, num_ee) uint8: the end bodies whose net contact force along z, as last refreshed, exceeds `threshold`."""
        return (self._end_rows(self.contact_forces)[..., 2] > threshold).to(torch.uint8)

    def balance_control(self, base_pos, base_quat, base_lin_vel=None, base_ang_vel=None, stance=None, kp_lin=100., kd_lin=None,
                        kp_ang=400., kd_ang=None, mu=None, fz_min=5., fz_max=None, weights=(1, 1, 1, 10, 10, 10), alpha=1e-2,
                        beta=0., gravity_compensation=True):
        """(efforts (num_envs, nd), forces (num_envs, num_ee, 3)): the ground-reaction forces that give the base the wrench
        w = M[0:6, 0:6] (a_lin, a_ang) + h[0:6] of a spring-damper towards base_pos (n, 3) / base_quat (n, 4) (and the world
        velocities base_lin_vel / base_ang_vel, None = rest) without slipping, and the efforts -sum J^T f that produce them; from
        the mass-matrix, bias, Jacobian, root, body and contact tensors as last refreshed.  a_lin = kp_lin (p* - p) + kd_lin (v* - v),
        a_ang = kp_ang orientation_error(q*, q) + kd_ang (omega* - omega); the coupling of the dof accelerations is neglected.
        The forces minimise 1/2 |G f - w|^2 weighted by `weights` + 1/2 alpha |f|^2 + 1/2 beta |f - previous call's f|^2 subject to
        fz_min <= f_z <= fz_max (None: no upper bound) and |f_x|, |f_y| <= mu f_z on the stance feet, f = 0 on the others
        (csrc/shf_qp.hip).  stance (n, num_ee) None = stance_from_contacts(); mu None = the env's contact friction, else a
        float or (n); kp / kd: scalars or 3-vectors, kd None = 2 sqrt(kp).  gravity_compensation adds bias_forces[:, 6:].
        Clamped to the asset's effort limits."""
        h = self.bias_forces                     # (refused with "fixed base" unless SHIFU_AMD_FLOATING_DYNAMICS=1)
        M = self.mass_matrix
        n = self.env.num_envs
        if getattr(self, "_bal_target", None) is None:
            self._bal_target = torch.zeros(n, 13, device=self.device)
        tg = self._bal_target
        jf = self.foot_jacobians
        root = self.env.root_state.view(n, -1, 13)[:, 0]
        feet = self._end_rows(self.env.body_state.view(n, -1, 13))[..., :3]
        f_prev = getattr(self, "_bal_forces", None)
        # one sequence (glue.balance_control) on the kernels (csrc/shf_qp.hip: shf_foot_force_qp), or on their torch expressions
        from shifu_amd import _abi, glue
        be = self.sim.backend
        efforts, forces = glue.balance_control(
            jf, root, feet, self._end_rows(self.contact_forces)[..., 2], be.tensors[_abi.T_FRICTION].to(self.device), be.terrain.friction,
            M, h, tg, self.torque_limits.contiguous(), base_pos, base_quat, base_lin_vel, base_ang_vel, stance, kp_lin, kd_lin, kp_ang,
            kd_ang, mu, fz_min, fz_max, weights, alpha, beta, gravity_compensation, f_prev, prims=self._control_prims(jf, tg))
        self._bal_forces = forces
        return efforts, forces

    def apply_balance_control(self, base_pos, base_quat, swing_targets=None, swing_gains=None, **kw):
        """decimation x {refresh the state, Jacobian, mass-matrix and bias tensors, balance_control, set the efforts, simulate,
        refresh the dof state}.  swing_targets (n, num_ee, 3), positions in the base frame: the efforts of
        foot_impedance_control(swing_targets, **swing_gains) without its bias are added on the dofs of the feet that are not in
        stance (one more launch).  The asset must be in DOF_MODE_EFFORT.  Returns the last (efforts, forces)."""
        if self.asset_options.default_dof_drive_mode != gymapi.DOF_MODE_EFFORT:
            raise RuntimeError("apply_balance_control: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT")
        self.mass_matrix, self.bias_forces      # acquired before the first refresh
        efforts = forces = None
        for _ in range(int(self.env.decimation)):
            self.gym.refresh_all_state_tensors(self.sim)
            self.gym.refresh_mass_matrix_tensors(self.sim)
            stance = kw.get("stance")
            if stance is None:
                stance = self.stance_from_contacts()
            efforts, forces = self.balance_control(base_pos, base_quat, **dict(kw, stance=stance))
            if swing_targets is not None:
                swing = self.foot_impedance_control(swing_targets, gravity_compensation=False, **(swing_gains or {}))
                dofs = ((1.0 - stance.to(torch.float32)) @ self._foot_dof_mask()).clamp(max=1.0)
                efforts = torch.maximum(torch.minimum(efforts + dofs * swing, self._effort_cap()), -self._effort_cap())
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(efforts))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)
        return efforts, forces

    def _effort_cap(self):
        lim = self.torque_limits
        return torch.where(lim > 0, lim, torch.full_like(lim, float("inf")))

    # -- locomotion: gait schedule, footholds and swing trajectories on top of the balance controller (not in the reference;
    # SHIFU_AMD_FLOATING_DYNAMICS=1) ------------------------------------------------------------------------------------------
    @property
    def nominal_foot_positions(self):
        """(num_ee, 3): the end bodies' origins in the base frame at the default dof positions (forward kinematics)."""
        if getattr(self, "_gait_nominal", None) is None:
            from .gait import nominal_foot_positions
            q = self.default_dof_pos.reshape(-1)[:self.num_dof].detach().cpu().numpy()
            p = nominal_foot_positions(self.sim.backend.model, q, self._ee_list)
            self._gait_nominal = torch.tensor(p, dtype=torch.float32, device=self.device)
        return self._gait_nominal

    def _foot_radius(self):
        from .gait import foot_radius
        return foot_radius(self.sim.backend.model, self._ee_list)

    def _gait_state(self):
        if getattr(self, "_gait", None) is None:
            from .gait import GaitState
            self._gait = GaitState(self.env.num_envs, self.num_ee, self.device)
        return self._gait

    def reset_gait(self, env_ids=None):
        """The next locomotion_control restarts these envs' gait (None: every env's): clock at 0, every foot scheduled to stand,
        the base target over the base and heading as the base does."""
        self._gait_state().reset(env_ids)

    def locomotion_control(self, command, gait=None, swing_kp=400., swing_kd=10., height=0.30, touchdown_z=None, **balance_kw):
        """One tick of a model-based walking controller: (efforts (num_envs, nd), forces (num_envs, num_ee, 3), stance
        (num_envs, num_ee) uint8, swing_targets (num_envs, num_ee, 3) in the base frame).  command (n, 3) = (vx, vy, yaw
        rate) in the heading frame of the base target.  The gait plan (csrc/shf_gait.hip) advances the base target at the
        commanded velocity at `height`, schedules the feet by `gait` (units.gait.Gait; None = Gait.trot()) gated by the
        contact forces, and gives every foot a target; the stance feet get balance_control's forces towards the base target
        (**balance_kw: its gains and bounds), the legs of the others a Cartesian spring-damper swing_kp / swing_kd (an explicit,
        light damper: at 2 sqrt(kp) the feet lag their targets) without bias; one launch merges the two and clamps to the
        effort limits.  One call is one tick of dt = the simulation step.  touchdown_z None = 1 cm below the resting height of a
        foot's origin on the plane z = 0.  A change of `gait` restarts the clock; reset_gait() restarts everything.  From the
        tensors as last refreshed.  controller="mpc" (among **balance_kw, with horizon, mpc_steps_per_tick, mpc_every,
        mpc_weights, mpc_alpha, mpc_iters: glue.locomotion_control says what each is) takes the stance forces from the horizon
        MPC over the gait's schedule (csrc/shf_mpc.hip) instead of the QP of this instant."""
        from .gait import Gait
        h = self.bias_forces                     # (refused with "fixed base" unless SHIFU_AMD_FLOATING_DYNAMICS=1)
        M = self.mass_matrix
        n = self.env.num_envs
        if gait is None:
            gait = getattr(self, "_gait_default", None) or Gait.trot()
            self._gait_default = gait
        st = self._gait_state()
        if getattr(self, "_gait_last", None) is not gait:
            st.tick.zero_()
            st.mpc_count = 0                         # the horizon MPC starts cold on the new schedule
            if st.mpc_u is not None:
                st.mpc_u.zero_()
            self._gait_last = gait
        if touchdown_z is None:
            touchdown_z = self._foot_radius() - 0.01
        dt = float(self.env.sim_params.dt)
        jf = self.foot_jacobians
        root = self.env.root_state.view(n, -1, 13)[:, 0]
        feet = self._end_rows(self.env.body_state.view(n, -1, 13))[..., :3]
        cz = self._end_rows(self.contact_forces)[..., 2]
        if getattr(self, "_gait_chain", None) is None:
            self._gait_chain = self._foot_dof_mask().to(torch.uint8)
        command = torch.as_tensor(command, dtype=torch.float32, device=self.device).expand(n, 3)
        from shifu_amd import _abi, glue
        be = self.sim.backend
        return glue.locomotion_control(
            jf, self.env.dof_state.view(n, self.num_dof, 2), root, feet, cz, be.tensors[_abi.T_FRICTION].to(self.device), be.terrain.friction,
            M, h, self.torque_limits.contiguous(), self._gait_chain, self.nominal_foot_positions, st, command, gait, dt, height,
            touchdown_z, swing_kp, swing_kd, **balance_kw, prims=self._control_prims(jf))

    def apply_locomotion_control(self, command, **kw):
        """decimation x {refresh the state, Jacobian, mass-matrix and bias tensors, locomotion_control (one gait tick), set the
        efforts, simulate, refresh the dof state}.  The asset must be in DOF_MODE_EFFORT.  Returns the last (efforts, forces,
        stance, swing_targets)."""
        if self.asset_options.default_dof_drive_mode != gymapi.DOF_MODE_EFFORT:
            raise RuntimeError("apply_locomotion_control: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT")
        self.mass_matrix, self.bias_forces      # acquired before the first refresh
        out = None
        for _ in range(int(self.env.decimation)):
            self.gym.refresh_all_state_tensors(self.sim)
            self.gym.refresh_mass_matrix_tensors(self.sim)
            out = self.locomotion_control(command, **kw)
            self.gym.set_dof_actuation_force_tensor(self.sim, gymtorch.unwrap_tensor(out[0]))
            self.gym.simulate(self.sim)
            if self.device == 'cpu':
                self.gym.fetch_results(self.sim, True)
            self.gym.refresh_dof_state_tensor(self.sim)
        return out
