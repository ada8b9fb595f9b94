"""Camera sensors on the fused envs (FusedA1Env / FusedAbbEnv): the ray caster of shifu_amd/render.py on the body states
the fused step kernels write (SHF_T_BODY_STATE), one launch per render and camera.

The fused envs own their scene -- the articulation's render shapes (CompiledModel.render_shapes), the box actors after
them in the body-state rows, and the terrain the env was built on, the warped trimesh included -- so cameras can be added
at any time.  Nothing here is part of the simulation state: images are derived data (state_dict is unchanged).

Optical flow (add_camera(..., flow=True)): the camera keeps the body and camera poses of its previous render
(render.FlowHistory) and renders with shf_render_cameras_flow.  The fused step kernels reset envs inside the launch, so
whether an env's previous frame is usable is worked out on the device: an env is valid iff its reset counter
(A1_RESET_COUNT / ABB_RESET_COUNT) still equals the value snapshotted at the previous flow render; env.reset()
invalidates every env.

Proprioceptive sensors (add_proprioception; DESIGN.md 8e "Proprioception") stand beside them: IMUs, joint encoders and foot
contact switches on the body, dof and contact tensors the step writes, one launch per read, with the same reset-counter rule for
the envs the fused step teleported since the last read."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from .. import _abi


class FusedCamera:
    """One camera per env, the same properties in every env.  Fixed: pose (position, quat) in the frame of root_state.
    Attached: the pose is body pose o (position, quat) at every render (Isaac Gym's FOLLOW_TRANSFORM)."""

    def __init__(self, env, width: int, height: int, horizontal_fov: float, near_plane: float, far_plane: float,
                 position, quat, attach_body: Optional[int], flow: bool = False):
        from ..render import FlowHistory, camera_struct
        n, dev = env.num_envs, env.device
        self.env = env
        self.width, self.height = int(width), int(height)
        self.horizontal_fov, self.near_plane, self.far_plane = float(horizontal_fov), float(near_plane), float(far_plane)
        self.camera = camera_struct(width, height, horizontal_fov, near_plane, far_plane, depth_negative=True)
        self.attach_body = None if attach_body is None else int(attach_body)
        B = env.cam_seg.shape[1]
        if self.attach_body is not None and not 0 <= self.attach_body < B:
            raise ValueError(f"add_camera: attach_body {attach_body} outside the env's {B} body-state rows")
        pose = torch.tensor(np.concatenate([np.asarray(position, float), np.asarray(quat, float)]), dtype=torch.float32)
        # fixed: the (N, 7) world poses, writable; attached: the local transform and the body's rows
        self.pose = pose.repeat(n, 1).to(dev).contiguous()
        if self.attach_body is not None:
            self._rows = torch.arange(n, device=dev, dtype=torch.long) * B + self.attach_body
        self._images = dict(rgba=torch.zeros(n, self.height, self.width, 4, dtype=torch.uint8, device=dev),
                            depth=torch.full((n, self.height, self.width), -float("inf"), dtype=torch.float32, device=dev),
                            seg=torch.zeros(n, self.height, self.width, dtype=torch.int32, device=dev))
        self._clouds = {}                                        # point_cloud(): allocated on first use
        self.flow = bool(flow)
        if self.flow:
            self._images["flow"] = torch.zeros(n, self.height, self.width, 2, dtype=torch.float32, device=dev)
            self._images["flow_i16"] = torch.zeros(n, self.height, self.width, 2, dtype=torch.int16, device=dev)
            self.history = FlowHistory(n, B, dev)
            self._count = env._cam_reset_count                   # (N,) int32, bumped by the step kernel's resets
            self._count_seen = self._count.clone()
            self._same = torch.zeros(n, dtype=torch.bool, device=dev)
            self._valid = torch.zeros(n, dtype=torch.int32, device=dev)

    def world_pose(self) -> torch.Tensor:
        """(N, 7) camera poses (pos, quat xyzw) on the env's current body states."""
        if self.attach_body is None:
            return self.pose
        from ..isaacgym.torch_utils import quat_apply, quat_mul
        bs = self.env.body_state.index_select(0, self._rows)
        return torch.cat([bs[:, :3] + quat_apply(bs[:, 3:7], self.pose[:, :3]), quat_mul(bs[:, 3:7], self.pose[:, 3:7])],
                         dim=1).contiguous()

    def render(self):
        """One launch for all envs on the body states of the last step / reset; no host sync."""
        env, im = self.env, self._images
        if self.flow:
            return self._render_flow()
        env._renderer.render(env.body_state, self.world_pose(), env.cam_seg, env.cam_color, self.camera, depth=im["depth"],
                             seg_out=im["seg"], rgba=im["rgba"])
        return im

    def _render_flow(self):
        """The flow launch, then this render becomes the previous one: preallocated tensors only, no host sync."""
        env, im, h = self.env, self._images, self.history
        pose = self.world_pose()
        torch.eq(self._count, self._count_seen, out=self._same)       # no reset inside a step since the previous render
        self._valid.copy_(self._same)
        self._valid.mul_(h.prev_valid)
        env._renderer.render(env.body_state, pose, env.cam_seg, env.cam_color, self.camera, depth=im["depth"], seg_out=im["seg"],
                             rgba=im["rgba"], flow=im["flow"], flow_i16=im["flow_i16"], prev_body_pose=h.prev_body_pose,
                             prev_cam_pose=h.prev_cam_pose, prev_valid=self._valid)
        h.update(env.body_state, pose)
        self._count_seen.copy_(self._count)
        return im

    def invalidate_flow(self, env_ids=None):
        """The next render's flow is zero in env_ids (all by default); nothing to do on a camera without flow."""
        if self.flow:
            self.history.invalidate(env_ids)

    def point_cloud(self, world_frame: bool = True) -> torch.Tensor:
        """(N, H, W, 3) f32: the point behind every pixel of the LAST render's depth image (shf_camera_points), in world
        coordinates on the camera poses as they are now -- call it after render(), before the next step -- or, with
        world_frame=False, in the camera's own axes (+x view axis, +y left, +z up).  A pixel that shows nothing: the point at
        far_plane along its ray.  One launch into a tensor allocated on first use; no host sync."""
        key = "points_w" if world_frame else "points_c"
        if key not in self._clouds:
            self._clouds[key] = torch.zeros(self.env.num_envs, self.height, self.width, 3, dtype=torch.float32, device=self.env.device)
        self.env._renderer.camera_points(self._images["depth"], self.world_pose(), self.camera, self._clouds[key], world_frame)
        return self._clouds[key]

    def raw_images(self):
        """{"rgba": (N, H, W, 4) u8, "depth": (N, H, W) f32, negative view depth, -inf where nothing is hit, "seg":
        (N, H, W) i32} -- the tensors render() writes (CameraSensor.raw_images's conventions).  Views, not copies.  A camera
        added with flow=True also has "flow": (N, H, W, 2) f32, (u, v) in pixels, and "flow_i16": (N, H, W, 2) int16."""
        return self._images


class FusedRayCaster:
    """A ray-caster sensor in every env (shifu_amd/raycast.py; shf_raycast): one pattern, one launch per cast().  Fixed:
    pose (position, quat) in the frame of root_state.  Attached: the pose is body pose o (position, quat) at every cast.
    origins / dirs: the pattern on the device; align, min_range, max_range, shape_mask: as Renderer.raycast takes them."""

    def __init__(self, env, pattern, position, quat, attach_body: Optional[int], align: str, min_range: float, max_range: float,
                 shape_mask: int, outputs: Sequence[str]):
        from ..raycast import ALIGN, check_pattern
        n, dev = env.num_envs, env.device
        o, d = check_pattern(*pattern)
        if align not in ALIGN:
            raise ValueError(f"add_ray_caster: align must be one of {sorted(ALIGN)}, got {align!r}")
        if not (0.0 <= float(min_range) <= float(max_range) and np.isfinite(float(max_range))):
            raise ValueError("add_ray_caster: need 0 <= min_range <= max_range, max_range finite")
        names = ("dist", "points", "normal", "seg", "body")
        if not outputs or any(k not in names for k in outputs):
            raise ValueError(f"add_ray_caster: outputs must name some of {names}, got {tuple(outputs)}")
        self.env = env
        self.origins, self.dirs = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
        self.num_rays = int(o.shape[0])
        self.align, self.min_range, self.max_range = align, float(min_range), float(max_range)
        self.shape_mask = int(shape_mask)
        self.attach_body = None if attach_body is None else int(attach_body)
        B = env.cam_seg.shape[1]
        if self.attach_body is not None and not 0 <= self.attach_body < B:
            raise ValueError(f"add_ray_caster: attach_body {attach_body} outside the env's {B} body-state rows")
        pose = torch.tensor(np.concatenate([np.asarray(position, float), np.asarray(quat, float)]), dtype=torch.float32)
        self.pose = pose.repeat(n, 1).to(dev).contiguous()
        if self.attach_body is not None:
            self._rows = torch.arange(n, device=dev, dtype=torch.long) * B + self.attach_body
            self._world = torch.zeros(n, 7, dtype=torch.float32, device=dev)
        R = self.num_rays
        make = dict(dist=lambda: torch.full((n, R), float("inf"), dtype=torch.float32, device=dev),
                    points=lambda: torch.zeros(n, R, 3, dtype=torch.float32, device=dev),
                    normal=lambda: torch.zeros(n, R, 3, dtype=torch.float32, device=dev),
                    seg=lambda: torch.zeros(n, R, dtype=torch.int32, device=dev),
                    body=lambda: torch.full((n, R), -2, dtype=torch.int32, device=dev))
        self._out = {k: make[k]() for k in names if k in outputs}

    def world_pose(self) -> torch.Tensor:
        """(N, 7) sensor poses (pos, quat xyzw) on the env's current body states."""
        if self.attach_body is None:
            return self.pose
        from ..isaacgym.torch_utils import quat_apply, quat_mul
        bs = self.env.body_state.index_select(0, self._rows)
        return torch.cat([bs[:, :3] + quat_apply(bs[:, 3:7], self.pose[:, :3]), quat_mul(bs[:, 3:7], self.pose[:, 3:7])],
                         dim=1, out=self._world)

    def cast(self) -> dict:
        """One launch for all envs on the body states of the last step / reset, into this sensor's own tensors; no host
        sync.  {"dist": (N, R) f32 range, +inf a miss; "points": (N, R, 3) f32 world frame, a miss: the ray's end at
        max_range; "normal": (N, R, 3); "seg": (N, R) int32 from env.cam_seg; "body": (N, R) int32 body-state row within
        the env, -1 terrain, -2 a miss} -- those named in `outputs`.  Views, not copies."""
        env, o = self.env, self._out
        env._renderer.raycast(env.body_state, self.world_pose(), self.origins, self.dirs, self.align, self.min_range,
                              self.max_range, self.shape_mask, seg=env.cam_seg if "seg" in o else None, dist=o.get("dist"),
                              points=o.get("points"), normal=o.get("normal"), seg_out=o.get("seg"), body=o.get("body"))
        return o


class FusedProprioception:
    """Proprioceptive sensors in every env (shifu_amd/proprio.py; shf_proprioception_step): IMUs, joint encoders and foot
    contact switches on the tensors the fused step writes, one launch per read().  The fused step resets envs inside the
    launch, so which envs were teleported since the last read is worked out on the device, the way flow cameras do it: an
    env's reset counter no longer equals the value snapshotted at the previous read.  reset(env_ids) raises flags by hand;
    env.reset() raises them all."""

    def __init__(self, env, core, reset_count):
        n, nd = env.num_envs, core.num_dof
        self.env, self.core = env, core
        self.flat = core.flat
        self._body = env.body_state.view(n, -1, 13)
        self._dof = env.dof_state.view(n, -1, 2)[:, :nd]
        self._contact = env.contact_state.view(n, -1, 3)
        self._count = reset_count
        self._count_seen = None if reset_count is None else reset_count.clone()
        self._moved = torch.zeros(n, dtype=torch.bool, device=env.device)

    def read(self) -> dict:
        """One launch for all envs on the states of the last step / reset, into this sensor's own tensors; no host sync.
        {"gyro", "accel": (N, I, 3); "dof_pos", "dof_vel": (N, nd); "contact", "first_contact": (N, F) uint8; "air_time",
        "contact_time", "last_air_time", "last_contact_time": (N, F)}: views of `flat` (N, D) and of the switch bytes."""
        extra = None
        if self._count is not None:
            torch.ne(self._count, self._count_seen, out=self._moved)
            self._count_seen.copy_(self._count)
            extra = self._moved.view(torch.uint8)
        return self.core.read(self._body, self._dof, self._contact, extra_reset=extra)

    def reset(self, env_ids=None):
        self.core.reset(env_ids)

    def randomize(self, env_ids=None, delay=None, generator=None):
        self.core.randomize(env_ids, delay=delay, generator=generator)

    def set_noise(self, **noise):
        self.core.set_noise(**noise)

    @property
    def last_reset(self):
        """(N) uint8: the reset flags the last read used."""
        return self.core.last_reset


class FusedCameraHost:
    """What FusedA1Env and FusedAbbEnv share: the per-env segmentation / color tables, add_camera, add_ray_caster and
    add_proprioception."""

    def _init_cameras(self, box_dims: Sequence = (), reset_count=None):
        """box_dims: full extents of the env's box actors, in body-state row order after the articulation's bodies;
        reset_count: the task's (N,) int32 per-env reset counter (what flow cameras check their previous frame against)."""
        from ..render import DEFAULT_BODY_COLOR
        self._cam_box_dims = [tuple(float(v) for v in d) for d in box_dims]
        B = int(self.cm.blob.nb) + len(self._cam_box_dims)
        # per env and body-state row, writable: segmentation id (0, the facade's default) and color in [0, 1]
        self.cam_seg = torch.zeros(self.num_envs, B, dtype=torch.int32, device=self.device)
        self.cam_color = torch.tensor(DEFAULT_BODY_COLOR, dtype=torch.float32, device=self.device).repeat(self.num_envs, B, 1)
        self.cameras = []
        self.ray_casters = []
        self.proprioception = []
        self.viewers = []
        self._renderer = None
        self._cam_reset_count = reset_count

    def _invalidate_camera_flow(self, env_ids=None):
        for cam in self.cameras:
            cam.invalidate_flow(env_ids)
        for s in self.proprioception:             # the same moment for the proprioceptive sensors: a reset is a teleport
            s.reset(env_ids)

    def add_camera(self, width: int, height: int, horizontal_fov: float, near_plane: float, far_plane: float,
                   position=(0.0, 0.0, 0.0), target=None, quat=None, attach_body: Optional[int] = None,
                   flow: bool = False) -> FusedCamera:
        """A camera in every env: looking from `position` at `target`, or with orientation `quat` (xyzw; local +x forward,
        +z up), in the frame of root_state -- or, with attach_body (a row of the env's body states), in that body's frame.
        flow=True: render() also writes optical flow ("flow", "flow_i16"; module docstring); the default leaves the images and
        the launch as they are."""
        from ..render import lookat_quat
        if target is not None and quat is not None:
            raise ValueError("add_camera: give target or quat, not both")
        if target is not None:
            quat = lookat_quat(position, target)
        elif quat is None:
            quat = (0.0, 0.0, 0.0, 1.0)
        quat = np.asarray(quat, float) / np.linalg.norm(quat)
        self._ensure_renderer()
        if flow and self._cam_reset_count is None:
            raise ValueError("add_camera: flow=True needs the env's reset counter (_init_cameras(reset_count=...))")
        cam = FusedCamera(self, width, height, horizontal_fov, near_plane, far_plane, position, quat, attach_body, flow=flow)
        self.cameras.append(cam)
        return cam

    def add_ray_caster(self, pattern, position=(0.0, 0.0, 0.0), quat=None, attach_body: Optional[int] = None,
                       align: str = "base", min_range: float = 0.0, max_range: float = 10.0, ignore_bodies=(),
                       outputs: Sequence[str] = ("dist", "points")) -> FusedRayCaster:
        """A ray-caster sensor in every env -- a height scanner, a lidar, any (origins, dirs) pattern of shifu_amd/raycast.py
        -- at `position` with orientation `quat` (xyzw) in the frame of root_state or, with attach_body (a row of the env's
        body states), in that body's frame.  align: "base" (the rays turn with the sensor), "yaw" (with its yaw about world
        z only: a height scanner under a pitching trunk keeps looking straight down) or "world".  ignore_bodies: body-state
        rows whose shapes the rays pass through; "articulation": every row of the articulation (the box actors stay).
        outputs: which of "dist", "points", "normal", "seg", "body" cast() writes.  Derived data, like the cameras."""
        from ..render import shape_mask_for
        quat = (0.0, 0.0, 0.0, 1.0) if quat is None else quat
        quat = np.asarray(quat, float) / np.linalg.norm(quat)
        r = self._ensure_renderer()
        if isinstance(ignore_bodies, str):
            if ignore_bodies != "articulation":
                raise ValueError(f"add_ray_caster: ignore_bodies must be body rows or 'articulation', got {ignore_bodies!r}")
            ignore_bodies = range(int(self.cm.blob.nb))
        rc = FusedRayCaster(self, pattern, position, quat, attach_body, align, min_range, max_range,
                            shape_mask_for(r.scene, ignore_bodies), tuple(outputs))
        self.ray_casters.append(rc)
        return rc

    def add_proprioception(self, imu=(), feet="auto", contact_mode="norm", velocity="direct", max_delay=0, delay=0, dt=None,
                           seed=0, backend="auto", **noise) -> FusedProprioception:
        """Proprioceptive sensors in every env (DESIGN.md 8e "Proprioception"): s = env.add_proprioception(imu=[dict(body=0,
        position=..., quat=...)], feet="auto", gyro_noise=..., ...); s.read() after a step.  imu: up to 4 mountings on rows
        of the env's body states; feet: "auto" (the articulation's bodies named *_foot), or up to 8 body rows, or ();
        contact_mode "norm" | "z" with f_on / f_off newtons; velocity "direct" | "difference"; max_delay <= 7 reads of latency
        and `delay` (an int, three ints for IMUs / encoders / feet, or an (N, 3) tensor; randomize() draws them per env); dt:
        seconds between two reads (default: the env's dt, one read per step); seed: the noise key (the draws are keyed by global
        env ids, so a sharded run draws what the unsharded one draws); the noise terms are shifu_amd.proprio.NOISE_NAMES.
        Derived data, like the cameras: the simulation and state_dict are unchanged."""
        from ..proprio import Proprioception
        names = list(self.cm.body_names)
        if isinstance(feet, str):
            if feet != "auto":
                raise ValueError(f"add_proprioception: feet must be 'auto' or body rows, got {feet!r}")
            feet = [b for b, name in enumerate(names) if name.endswith("_foot")]
        B = self.cam_seg.shape[1]
        core = Proprioception(self.num_envs, B, int(self.cm.blob.nd), self.device, imus=list(imu), feet=list(feet), contact_mode=contact_mode,
                              velocity=velocity, max_delay=max_delay, delay=delay, gravity=tuple(float(v) for v in self.sim_params.gravity),
                              dt=float(self.dt) if dt is None else float(dt), seed=seed, env_id_offset=int(getattr(self, "env_id_offset", 0)),
                              backend=backend, **noise)
        s = FusedProprioception(self, core, self._cam_reset_count)
        self.proprioception.append(s)
        return s

    def _ensure_renderer(self):
        from ..render import Renderer, build_scene
        if self._renderer is None:
            t = self.sim.terrain
            hs = self.sim.height_samples if t.rows > 0 else None
            scene = build_scene(self.cm.render_shapes, int(self.cm.blob.nb), self._cam_box_dims, height_samples=hs,
                                vscale=t.vscale)
            # the sim's own terrain payload on the device (a warped terrain: samples followed by the vertex bytes)
            self._renderer = Renderer(scene, t, self.sim._heights if t.rows > 0 else None, self.device)
        return self._renderer

    # what add_viewer takes when the caller names none: FusedA1Env's envs really are apart on the terrain ("world", and a
    # radius about the trunk that holds the whole robot, for the env-level cull); FusedAbbEnv's all sit at the origin
    # ("grid"), and its box roams free of the arm's base, so no radius bounds the env (0: no env-level cull)
    _viewer_layout = "world"

    def _viewer_env_radius(self) -> float:
        return 0.0

    def add_viewer(self, width: int, height: int, horizontal_fov: float = 90.0, near_plane: float = 0.05,
                   far_plane: float = 100.0, env_ids=None, layout: Optional[str] = None, spacing=2.0,
                   per_row: Optional[int] = None):
        """A viewer.Viewer over env_ids (default: every env) on the body states the step kernels write: one camera that sees
        them all (shf_render_world), with the cameras' segmentation / color tables.  Derived data, like the cameras."""
        from ..viewer import Viewer
        layout = self._viewer_layout if layout is None else layout
        v = Viewer(self._ensure_renderer(), self.num_envs, self.body_state, self.cam_seg, self.cam_color, width, height,
                   horizontal_fov, near_plane, far_plane, env_ids=env_ids, layout=layout, spacing=spacing, per_row=per_row,
                   env_radius=self._viewer_env_radius())
        self.viewers.append(v)
        return v
