"""CameraSensor (reference shifu/units/sensors.py:46-188) on this backend's camera sensors (shifu_amd/render.py).

Same public surface: color_buf / depth_buf / segmentation_buf (N, H, W[, C]), proj_matrix / view_matrix of env 0,
init_buffers, refresh, set_camera_location, set_camera_transform, the local_lookat_positions / transform poses and
image_normalization.  refresh() fills every env at once from the camera group's image tensors (the reference loops over
envs, one get_camera_image_gpu_tensor per env and image type); IsaacGymEnv.refresh_sensors renders first.  The images
are drawn from the collision geometry by a ray caster, not by Isaac Gym's renderer (DESIGN.md "Camera sensors").
The cv2 viewer `render()` is not provided.

IMAGE_OPTICAL_FLOW is rendered under SHIFU_AMD_OPTICAL_FLOW=1 only (read when the sensor and the sim are built; without
it the type is refused as before, so the default config's image_types still raise): ground-truth flow from the same cast,
flow = where a pixel's surface point is now minus where it was at this sensor's previous render, in Isaac Gym's int16
encoding (DESIGN.md "Camera sensors"; no parity with Isaac Gym's own sign conventions is claimed).  optical_flow_buf is
(N, H, W, 2) int16, u first -- the reference allocates (N, H, W) and its own comment doubts that shape (sensors.py:88-94);
a flow image has two channels.  normalize_optical_flow(optical_flow, width, height) returns pixels.  reset_idx(env_ids)
marks those envs' previous frame unusable: their next flow image is zero.

CameraSensor.point_cloud() and RayCasterSensor have no counterpart in the reference (its to-do list, sensors.py:16-20, names
point clouds): the world-frame point behind every pixel of the last depth image, and a sensor of arbitrary rays -- a height
scanner, a lidar -- on the same ray caster (shifu_amd/raycast.py; DESIGN.md 8e "Ray caster")."""
import enum

import numpy as np
import torch

from shifu_amd.isaacgym import gymapi

from .units import Sensor

IMAGE_TYPE_COLOR = gymapi.IMAGE_COLOR
IMAGE_TYPE_DEPTH = gymapi.IMAGE_DEPTH
IMAGE_TYPE_SEGMENTATION = gymapi.IMAGE_SEGMENTATION
IMAGE_TYPE_OPTICAL_FLOW = gymapi.IMAGE_OPTICAL_FLOW


def optical_flow_enabled() -> bool:
    return gymapi.Gym._optical_flow_enabled()


def normalize_optical_flow(optical_flow, width, height):
    """Pixels (..., 2) float32 of an int16 flow image: u = q_u width / 32768, v = q_v height / 32768 -- a working form of the
    reference's helper (sensors.py:31-36)."""
    from shifu_amd.render import flow_from_i16
    return flow_from_i16(optical_flow, width, height)


class CameraPose(enum.Enum):
    LocalLookat = 0
    Transform = 1
    AttachLocalTransform = 2


class CameraSensor(Sensor):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.width = cfg.camera_props.width
        self.height = cfg.camera_props.height
        self.near_plane = cfg.camera_props.near_plane
        self.far_plane = cfg.camera_props.far_plane

    def _init_props(self):
        if self.cfg.local_lookat_positions is not None:
            assert self.cfg.transform is None and self.cfg.attach_local_transform is None
            self.local_lookat_position = (gymapi.Vec3(*self.cfg.local_lookat_positions[0]),
                                          gymapi.Vec3(*self.cfg.local_lookat_positions[1]))
            self._pose_type = CameraPose.LocalLookat
        elif self.cfg.transform is not None:
            assert self.cfg.local_lookat_positions is None and self.cfg.attach_local_transform is None
            self.transform = gymapi.Transform()
            self.transform.p = gymapi.Vec3(*self.cfg.transform[0])
            self.transform.r = gymapi.Quat(*self.cfg.transform[1])
            self._pose_type = CameraPose.Transform
        elif self.cfg.attach_local_transform is not None:
            raise NotImplementedError('Currently not support')      # as the reference (sensors.py:117-119)
        else:
            raise NotImplementedError('choose one of method from local_lookat_positions and transform')
        if IMAGE_TYPE_OPTICAL_FLOW in self.cfg.image_types and not optical_flow_enabled():
            raise NotImplementedError("CameraSensor: IMAGE_OPTICAL_FLOW is not rendered by this backend (depth, "
                                      "segmentation and color are)")

    def reset_idx(self, env_ids):
        # optical flow: the poses of the previous render say nothing about motion across a reset
        if IMAGE_TYPE_OPTICAL_FLOW in self.cfg.image_types and getattr(self, "camera_handle", None) is not None:
            self.gym.invalidate_camera_flow(self.sim, self.camera_handle, env_ids)

    def load_to(self, env_id, env_handle, seg_id):
        camera_handle = self.gym.create_camera_sensor(env_handle, self.cfg.camera_props)
        if self._pose_type == CameraPose.LocalLookat:
            self.gym.set_camera_location(camera_handle, env_handle, self.local_lookat_position[0], self.local_lookat_position[1])
        else:
            self.gym.set_camera_transform(camera_handle, env_handle, self.transform)
        if env_id == 0:
            self.camera_handle = camera_handle
            self._update_matrices(env_handle)

    def _update_matrices(self, env_handle):
        self.proj_matrix = np.matrix(self.gym.get_camera_proj_matrix(self.sim, env_handle, self.camera_handle))
        self.view_matrix = np.matrix(self.gym.get_camera_view_matrix(self.sim, env_handle, self.camera_handle))

    def init_buffers(self):
        n = self.env.num_envs
        for img_type in self.cfg.image_types:
            if img_type == IMAGE_TYPE_COLOR:
                # RGBA u8, or RGB float in [0, 1] with image_normalization
                self.color_buf = torch.zeros(n, self.height, self.width, 3 if self.cfg.image_normalization else 4,
                                             dtype=torch.float if self.cfg.image_normalization else torch.uint8, device=self.device)
            elif img_type == IMAGE_TYPE_DEPTH:
                # view-space distance (positive; the facade's IMAGE_DEPTH is its negative)
                self.depth_buf = torch.zeros(n, self.height, self.width, dtype=torch.float, device=self.device)
            elif img_type == IMAGE_TYPE_SEGMENTATION:
                self.segmentation_buf = torch.zeros(n, self.height, self.width, dtype=torch.int32, device=self.device)
            elif img_type == IMAGE_TYPE_OPTICAL_FLOW and optical_flow_enabled():
                # (u, v) x 32768 / (W, H), int16 (module docstring: the reference's (N, H, W) has no room for two channels)
                self.optical_flow_buf = torch.zeros(n, self.height, self.width, 2, dtype=torch.int16, device=self.device)
            else:
                raise NotImplementedError
        self._images = self.gym.camera_group_tensors(self.sim, self.camera_handle)

    def set_camera_transform(self, position, rotation):
        transform = gymapi.Transform(gymapi.Vec3(*position), gymapi.Quat(*rotation))
        for env_handle in self.env.env_handles:
            self.gym.set_camera_transform(self.camera_handle, env_handle, transform)
        self.transform = transform
        self._pose_type = CameraPose.Transform
        self._update_matrices(self.env.env_handles[0])

    def set_camera_location(self, local_pos, lookat_pos):
        for env_handle in self.env.env_handles:
            self.gym.set_camera_location(self.camera_handle, env_handle, gymapi.Vec3(*local_pos), gymapi.Vec3(*lookat_pos))
        self.local_lookat_position = (local_pos, lookat_pos)
        self._pose_type = CameraPose.LocalLookat
        self._update_matrices(self.env.env_handles[0])

    def render_images(self):
        """This sensor's camera group, rendered for every env (one launch)."""
        self.gym.render_camera_group(self.sim, self.camera_handle)

    def raw_images(self):
        """The camera group's own image tensors as rendered, before refresh() converts them: {"rgba": (N, H, W, 4) u8,
        "depth": (N, H, W) f32, negative view depth, "seg": (N, H, W) i32} and, under SHIFU_AMD_OPTICAL_FLOW=1, "flow": (N, H, W, 2)
        int16.  Views, not copies."""
        return self._images

    def refresh(self):
        self.refresh_image_tensors()

    def point_cloud(self, world_frame=True):
        """(N, H, W, 3) f32: the point behind every pixel of the camera group's last rendered depth image, in the frame of
        the state tensors (world_frame=False: in the camera's own axes, +x the view axis, +y left, +z up); a pixel that shows
        nothing gives the point at far_plane along its ray.  One launch (shf_camera_points) into a tensor allocated on first
        use; refresh() and the image buffers are as they were."""
        return self.gym.camera_group_points(self.sim, self.camera_handle, world_frame)

    def refresh_image_tensors(self):
        im = self._images
        types = self.cfg.image_types
        if IMAGE_TYPE_COLOR in types:
            if self.cfg.image_normalization:
                torch.div(im["rgba"][..., :3], 255.0, out=self.color_buf)       # normalize_color (shifu/utils/image.py)
            else:
                self.color_buf.copy_(im["rgba"])
        if IMAGE_TYPE_DEPTH in types:
            torch.neg(im["depth"], out=self.depth_buf)                       # Isaac gives negative depth (sensors.py:174-178)
        if IMAGE_TYPE_SEGMENTATION in types:
            self.segmentation_buf.copy_(im["seg"])
        if IMAGE_TYPE_OPTICAL_FLOW in types:
            self.optical_flow_buf.copy_(im["flow"])


class RayCasterSensor(Sensor):
    """A ray-caster sensor (configs.RayCasterSensorConfig): after refresh(), ray_distances (N, R) f32 holds every ray's range
    (+inf: nothing within max_range) and ray_hits_w (N, R, 3) f32 its hit point in the frame of the state tensors (a miss:
    the ray's end at max_range, finite).  The rays see the env's collision world -- the robot unless ignore_robot, the box
    actors, the terrain with everything standing on it -- where get_heights samples the height-field lattice.  Nothing is
    registered with the gym before prepare_sim: the sensor is built in init_buffers on the render scene the sim builds
    lazily, and IsaacGymEnv.refresh_sensors casts it (one launch, no host sync)."""

    def __init__(self, cfg):
        super().__init__(cfg)
        from shifu_amd.raycast import ALIGN, check_pattern
        if cfg.pattern is None:
            raise ValueError("RayCasterSensor: cfg.pattern must be (origins, dirs) -- see shifu_amd.raycast")
        self.origins, self.dirs = check_pattern(*cfg.pattern)
        self.num_rays = int(self.origins.shape[0])
        if cfg.align not in ALIGN:
            raise ValueError(f"RayCasterSensor: align must be one of {sorted(ALIGN)}, got {cfg.align!r}")
        if (cfg.transform is None) == (cfg.attach_local_transform is None):
            raise ValueError("RayCasterSensor: give exactly one of transform and attach_local_transform")
        if cfg.attach_local_transform is not None and cfg.attach_body_name is None:
            raise ValueError("RayCasterSensor: attach_local_transform needs attach_body_name")
        self._handle = None

    def _init_props(self):
        pass

    def load_to(self, env_id, env_handle, seg_id):
        pass                                                 # nothing to create per env: one group for all envs, after prepare_sim

    def reset_idx(self, env_ids):
        pass

    def init_buffers(self):
        cfg, robot = self.cfg, self.env.robot
        attach = None
        pos, quat = cfg.transform if cfg.transform is not None else cfg.attach_local_transform
        if cfg.attach_local_transform is not None:
            bodies = robot.rigid_body_dict
            if cfg.attach_body_name not in bodies:
                raise ValueError(f"RayCasterSensor: the robot has no rigid body {cfg.attach_body_name!r} (it has {sorted(bodies)})")
            attach = int(bodies[cfg.attach_body_name])
        ignore = range(int(robot.num_bodies)) if cfg.ignore_robot else ()
        self._handle = self.gym.create_ray_caster_group(self.sim, (self.origins, self.dirs), pos, quat, attach_body=attach,
                                                        align=cfg.align, min_range=cfg.min_range, max_range=cfg.max_range,
                                                        ignore_bodies=ignore)
        self._group = self.sim.ray_caster_groups[self._handle]
        self.ray_distances, self.ray_hits_w = self._group["dist"], self._group["points"]

    def refresh(self):
        self.gym.cast_ray_caster_group(self.sim, self._handle)


class ProprioceptionSensor(Sensor):
    """What the robot measures about itself (configs.ProprioceptionSensorConfig; shifu_amd/proprio.py; DESIGN.md 8e
    "Proprioception"): IMUs with bias, noise and a bias walk, joint encoders with offset, noise and quantisation, foot contact
    switches with hysteresis and the air / contact times, each behind a per-env latency.  read() is one launch on the GPU
    (csrc/shf_proprio.hip) and the same algorithm in torch on the CPU or with cfg.backend = "torch"; it returns a dict of
    views of `flat` (N, D) -- gyro / accel (N, I, 3), dof_pos / dof_vel (N, nd), contact / first_contact (N, F) uint8, air_time
    / contact_time / last_air_time / last_contact_time (N, F) -- on the state tensors as the last refresh left them.
    refresh() is read().  Robot.reset_idx raises the reset flags of the envs it resets; reset(env_ids) does it by hand."""

    def __init__(self, cfg):
        super().__init__(cfg)
        self.core = None

    def _init_props(self):
        pass

    def load_to(self, env_id, env_handle, seg_id):
        pass                                                 # nothing to create per env: the sensor reads the state tensors

    def reset_idx(self, env_ids):
        self.reset(env_ids)

    def _body(self, b, bodies):
        if isinstance(b, str):
            if b not in bodies:
                raise ValueError(f"ProprioceptionSensor: the robot has no rigid body {b!r} (it has {sorted(bodies)})")
            return int(bodies[b])
        return int(b)

    def init_buffers(self):
        from shifu_amd.proprio import NOISE_NAMES, Proprioception
        cfg, env, robot = self.cfg, self.env, self.env.robot
        bodies = robot.rigid_body_dict
        n = env.num_envs
        imus = [dict(m, body=self._body(m["body"], bodies)) for m in cfg.imu]
        feet = cfg.feet
        if isinstance(feet, str):
            if feet != "auto":
                raise ValueError(f"ProprioceptionSensor: feet must be 'auto' or a list of bodies, got {feet!r}")
            feet = list(getattr(robot.cfg, "end_effector_names", ()) or ())
        feet = [self._body(b, bodies) for b in feet]
        self._body_view = env.body_state.view(n, -1, 13)
        self._contact_view = env.contact_state.view(n, -1, 3)
        self._dof_view = env.dof_state.view(n, -1, 2)[:, :robot.num_dof]
        gravity = cfg.gravity if cfg.gravity is not None else _sim_gravity(self.sim)
        dt = float(cfg.dt) if cfg.dt is not None else float(env.dt)
        noise = {k: getattr(cfg, k) for k in NOISE_NAMES if getattr(cfg, k, None) is not None}
        self.core = Proprioception(n, self._body_view.shape[1], robot.num_dof, self.device, imus=imus, feet=feet,
                                   contact_mode=cfg.contact_mode, velocity=cfg.velocity, max_delay=cfg.max_delay, delay=cfg.delay,
                                   gravity=gravity, dt=dt, seed=cfg.seed, backend=cfg.backend, **noise)
        self.flat = self.core.flat
        if not hasattr(robot, "proprioception_sensors"):
            robot.proprioception_sensors = []
        robot.proprioception_sensors.append(self)

    def read(self):
        return self.core.read(self._body_view, self._dof_view, self._contact_view)

    def refresh(self):
        self.read()

    def reset(self, env_ids=None):
        if self.core is not None:
            self.core.reset(env_ids)

    def randomize(self, env_ids=None, delay=None, generator=None):
        self.core.randomize(env_ids, delay=delay, generator=generator)


def _sim_gravity(sim):
    """The simulation's gravity vector as three floats."""
    for holder in (getattr(sim, "params", None), getattr(sim, "sim_params", None), getattr(getattr(sim, "backend", None), "params", None)):
        g = getattr(holder, "gravity", None)
        if g is not None:
            return (float(g.x), float(g.y), float(g.z)) if hasattr(g, "x") else tuple(float(v) for v in g)
    raise RuntimeError("ProprioceptionSensor: the sim's gravity is not known here; set cfg.gravity")
