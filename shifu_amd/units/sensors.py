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
marks those envs' previous frame unusable: their next flow image is zero."""
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
