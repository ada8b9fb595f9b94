"""Headless viewer: one world camera over many envs (shf_render_world, csrc/shf_render.hip), and frames to disk.

A camera sensor (render.Renderer.render, gym/fused_camera.py) belongs to one env and sees that env alone.  A Viewer is one
camera that sees a list of envs at once -- the A1 robots spread over their shared terrain (layout "world": the envs are
where their states say), or the push-box envs, which all sit at the origin, laid out on the grid Isaac Gym would have
used (layout "grid": list position j is displaced by (spacing_x (j % per_row), spacing_y (j // per_row), 0)).  It draws
what the camera sensors draw -- the collision geometry, flat-shaded, the same rays and conventions (render.py's module
docstring) -- with one launch per draw(), into preallocated tensors, without a host sync: a draw can be captured in a
hipGraph with the step it follows.  There is no window: FrameRecorder keeps frames on the device and writes PNG files (and
one animated PNG) at the end, with zlib and struct alone.

The tie rule: a pixel shows the nearest surface among the terrain, which is cast once and never displaced, and every
shape of every drawn env.  Among shapes at exactly equal depth the earlier (list position, shape index) wins; the terrain
wins over a shape only where it is strictly nearer.  "env" is the env id behind each pixel, -1 for terrain or nothing.
"""
from __future__ import annotations

import os
import struct
import zlib
from typing import Callable, Optional, Sequence

import numpy as np

from . import _abi

LAYOUTS = ("world", "grid")


# -- PNG / APNG: zlib and struct only -------------------------------------------------------------------------------------
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def _image_array(array) -> np.ndarray:
    a = np.asarray(array)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"expected an (H, W, 3) or (H, W, 4) uint8 image, got {a.shape} {a.dtype}")
    return np.ascontiguousarray(a)


def _ihdr(a: np.ndarray) -> bytes:
    # 8 bits per sample; color type 2 = RGB, 6 = RGBA; deflate, adaptive filtering (every row: filter 0), no interlace
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8, 2 if a.shape[2] == 3 else 6, 0, 0, 0))


def _deflated_rows(a: np.ndarray, level: int) -> bytes:
    rows = np.zeros((a.shape[0], 1 + a.shape[1] * a.shape[2]), np.uint8)      # a filter-type byte (0: none) before each row
    rows[:, 1:] = a.reshape(a.shape[0], -1)
    return zlib.compress(rows.tobytes(), level)


def write_png(path, array, level: int = 6):
    """An (H, W, 3) RGB or (H, W, 4) RGBA uint8 image as an 8-bit PNG."""
    a = _image_array(array)
    with open(path, "wb") as f:
        f.write(_PNG_SIGNATURE + _ihdr(a) + _chunk(b"IDAT", _deflated_rows(a, level)) + _chunk(b"IEND", b""))


def write_apng(path, frames: Sequence, fps: float = 25.0, loops: int = 0, level: int = 6):
    """Frames of one shape and channel count as one animated PNG (IHDR, acTL, then fcTL + IDAT for the first frame and
    fcTL + fdAT for every later one, IEND; loops = 0: forever).  A viewer without APNG support shows the first frame."""
    imgs = [_image_array(f) for f in frames]
    if not imgs or any(i.shape != imgs[0].shape for i in imgs):
        raise ValueError("write_apng: need at least one frame, all of one shape")
    den = 1000
    num = max(1, min(65535, int(round(den / float(fps)))))
    H, W = imgs[0].shape[:2]
    out = [_PNG_SIGNATURE, _ihdr(imgs[0]), _chunk(b"acTL", struct.pack(">II", len(imgs), int(loops)))]
    seq = 0
    for k, a in enumerate(imgs):
        # sequence number, width, height, x / y offset, delay numerator / denominator, dispose op 0 (none), blend op 0 (source)
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, num, den, 0, 0)))
        seq += 1
        data = _deflated_rows(a, level)
        if k == 0:
            out.append(_chunk(b"IDAT", data))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + data))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as f:
        f.write(b"".join(out))


# -- layout ---------------------------------------------------------------------------------------------------------------
def grid_offsets(count: int, spacing=2.0, per_row: Optional[int] = None) -> np.ndarray:
    """(count, 3) float32: list position j at (spacing_x (j % per_row), spacing_y (j // per_row), 0).  spacing: one number
    or (x, y); per_row defaults to ceil(sqrt(count))."""
    count = int(count)
    if count < 1:
        raise ValueError("grid_offsets: count < 1")
    sx, sy = (float(spacing), float(spacing)) if np.isscalar(spacing) else (float(spacing[0]), float(spacing[1]))
    per_row = int(np.ceil(np.sqrt(count))) if per_row is None else int(per_row)
    if per_row < 1:
        raise ValueError("grid_offsets: per_row < 1")
    j = np.arange(count)
    return np.stack([sx * (j % per_row), sy * (j // per_row), np.zeros(count)], axis=1).astype(np.float32)


def model_env_radius(cm) -> float:
    """A radius about body 0's origin that holds every render shape of a compiled articulation in any joint configuration:
    the longest chain of joint offsets from the root, each followed by the farthest reach of a shape on that body."""
    blob = cm.blob
    nb = int(blob.nb)
    dist = np.zeros(nb)
    for b in range(1, nb):                              # (parents precede children in the compiled order)
        p = int(blob.parent[b])
        dist[b] = (dist[p] if 0 <= p < b else 0.0) + float(np.linalg.norm(blob.tpos[b][:]))
        if int(blob.jtype[b]) == _abi.JOINT_PRISMATIC and 0 <= int(blob.dof[b]) < int(blob.nd):          # a prismatic joint: its travel
            dist[b] += max(abs(float(blob.lower[blob.dof[b]])), abs(float(blob.upper[blob.dof[b]])))
    reach = 0.0
    for s in cm.render_shapes:
        size = np.asarray(s.size, float)
        if s.kind == "box":
            r = float(np.linalg.norm(0.5 * size))
        elif s.kind == "sphere":
            r = float(size[0])
        elif s.kind == "capsule":
            r = float(size[0]) + 0.5 * float(size[1])
        else:
            r = float(np.linalg.norm(np.asarray(s.poly["verts"], float), axis=1).max())
        reach = max(reach, dist[int(s.body)] + float(np.linalg.norm(s.pos)) + r)
    return float(reach)


# -- the viewer ------------------------------------------------------------------------------------------------------------
class Viewer:
    """One camera over env_ids (default: all num_envs envs) of a render scene.

    renderer: the render.Renderer that holds the scene and the terrain; body_state (num_envs * num_bodies, 13), seg
    (num_envs, num_bodies) int32 and color (num_envs, num_bodies, 3) f32: the tables the camera sensors read, used in place.
    All four may be None when `source` is given: a callable returning (renderer, body_state, seg, color), called once at the
    first draw -- the gym facade makes its viewer before the sim is on the device.  Everything the host can check is
    checked here; device tensors are allocated at the first draw, none after it."""

    def __init__(self, renderer, num_envs: int, body_state, seg, color, width: int, height: int, horizontal_fov: float = 90.0,
                 near: float = 0.05, far: float = 100.0, env_ids=None, layout: str = "world", spacing=2.0,
                 per_row: Optional[int] = None, env_radius: float = 0.0, source: Optional[Callable] = None):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("Viewer: num_envs < 1")
        self.width, self.height = int(width), int(height)
        if self.width < 1 or self.height < 1:
            raise ValueError("Viewer: width and height must be positive")
        if not (0.0 < float(horizontal_fov) < 180.0) or not (0.0 < float(near) < float(far)):
            raise ValueError("Viewer: need 0 < horizontal_fov < 180 and 0 < near < far")
        self.horizontal_fov, self.near, self.far = float(horizontal_fov), float(near), float(far)
        ids = np.arange(self.num_envs) if env_ids is None else np.asarray(env_ids)
        if ids.ndim != 1 or ids.size < 1:
            raise ValueError("Viewer: env_ids must be a non-empty list of env ids")
        if not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= self.num_envs:
            raise ValueError(f"Viewer: env_ids must be integers in [0, {self.num_envs})")
        self.env_ids = ids.astype(np.int32)
        if layout not in LAYOUTS:
            raise ValueError(f"Viewer: layout must be one of {LAYOUTS}, got {layout!r}")
        self.layout = layout
        self.offsets = (grid_offsets(len(ids), spacing, per_row) if layout == "grid"
                        else np.zeros((len(ids), 3), np.float32))
        self.env_radius = float(env_radius)
        if renderer is None and source is None:
            raise ValueError("Viewer: give renderer, body_state, seg and color, or a source that returns them")
        self._bound = None if renderer is None else (renderer, body_state, seg, color)
        self._source = source
        self._pose = np.array([0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
        self._follow = None
        self._dev = None                                   # device state, built by the first draw
        self.images = None

    # -- the camera ------------------------------------------------------------------------------------------------------
    def env_offset(self, env_id: int) -> np.ndarray:
        """Where the viewer displaces env_id to: the offset of its first position in env_ids."""
        pos = np.nonzero(self.env_ids == int(env_id))[0]
        if pos.size == 0:
            raise ValueError(f"Viewer: env {env_id} is not among the envs drawn")
        return self.offsets[pos[0]].astype(np.float64)

    def set_pose(self, position, quat):
        """A fixed camera at `position` with orientation `quat` (xyzw; local +x forward, +z up), in viewer coordinates (the
        frame of the states, plus the layout's offsets)."""
        q = np.asarray(quat, float)
        if q.shape != (4,) or np.linalg.norm(q) == 0.0:
            raise ValueError("Viewer.set_pose: quat must be four numbers, not all zero")
        self._pose = np.concatenate([np.asarray(position, float).reshape(3), q / np.linalg.norm(q)])
        self._follow = None
        self._push_pose()

    def look_at(self, position, target):
        from .render import lookat_quat
        self.set_pose(position, lookat_quat(position, target))

    def follow(self, env_id: int, body: int = 0, offset=(-2.0, -2.0, 1.5)):
        """The camera sits at that body's position + the env's layout offset + `offset` at every draw and looks back at the
        body (a fixed orientation).  The position is composed on the device from the body states: no host sync."""
        from .render import lookat_quat
        off = np.asarray(offset, float).reshape(3)
        self._follow = (int(env_id), int(body), self.env_offset(env_id) + off)
        if not 0 <= int(env_id) < self.num_envs or int(body) < 0:
            raise ValueError("Viewer.follow: env_id or body out of range")
        self._pose = np.concatenate([np.zeros(3), lookat_quat(off, np.zeros(3))])
        if self._dev is not None:
            self._bind_follow()
        self._push_pose()

    def _push_pose(self):
        if self._dev is not None:
            import torch
            self._dev["pose"].copy_(torch.from_numpy(self._pose.astype(np.float32)).view(1, 7))

    def _bind_follow(self):
        import torch
        env_id, body, add = self._follow
        B = self._dev["num_bodies"]
        if body >= B:
            raise ValueError(f"Viewer.follow: body {body} outside the env's {B} body-state rows")
        self._dev["follow_src"] = self._dev["body_state"][env_id * B + body, :3]
        self._dev["follow_add"] = torch.from_numpy(add.astype(np.float32)).to(self._dev["pose"].device)

    # -- drawing ---------------------------------------------------------------------------------------------------------
    def _build(self):
        import torch
        from .render import camera_struct
        renderer, body_state, seg, color = self._bound if self._bound is not None else self._source()
        dev = renderer.device
        B = int(renderer.scene.num_bodies)
        if tuple(seg.shape) != (self.num_envs, B):
            raise ValueError(f"Viewer: the scene has {tuple(seg.shape)} (envs, bodies), the viewer was made for {self.num_envs} envs")
        H, W = self.height, self.width
        self._dev = dict(renderer=renderer, body_state=body_state, seg=seg, color=color, num_bodies=B,
                         camera=camera_struct(W, H, self.horizontal_fov, self.near, self.far, depth_negative=False),
                         pose=torch.zeros(1, 7, dtype=torch.float32, device=dev),
                         env_ids=torch.from_numpy(self.env_ids).to(dev), offsets=torch.from_numpy(self.offsets).to(dev),
                         rgba=torch.zeros(1, H, W, 4, dtype=torch.uint8, device=dev),
                         depth=torch.full((1, H, W), float("inf"), dtype=torch.float32, device=dev),
                         seg_out=torch.zeros(1, H, W, dtype=torch.int32, device=dev),
                         env_out=torch.full((1, H, W), -1, dtype=torch.int32, device=dev))
        d = self._dev
        self.images = {"rgba": d["rgba"][0], "depth": d["depth"][0], "seg": d["seg_out"][0], "env": d["env_out"][0]}
        if self._follow is not None:
            self._bind_follow()
        self._push_pose()

    def draw(self) -> dict:
        """One launch on the current body states.  Returns {"rgba": (H, W, 4) u8, "depth": (H, W) f32, the view depth, +inf
        where nothing is hit, "seg": (H, W) i32, "env": (H, W) i32, -1 for terrain or nothing}: views of preallocated
        tensors, the same ones at every draw."""
        if self._dev is None:
            self._build()
        d = self._dev
        if self._follow is not None:
            import torch
            torch.add(d["follow_src"], d["follow_add"], out=d["pose"][0, :3])
        d["renderer"].render_world(d["body_state"], d["pose"], d["seg"], d["color"], d["camera"], env_ids=d["env_ids"],
                                   env_offset=d["offsets"] if self.layout == "grid" else None, env_radius=self.env_radius,
                                   depth=d["depth"], seg_out=d["seg_out"], rgba=d["rgba"], env_out=d["env_out"])
        return self.images

    def pose(self):
        """The (7,) device tensor of the camera pose the last draw used (pos, quat xyzw); None before the first draw."""
        return None if self._dev is None else self._dev["pose"][0]


class FrameRecorder:
    """Keeps up to max_frames of a viewer's color image on the device: record() is one copy into a preallocated (F, H, W, 4)
    buffer on the current stream (no host sync, capturable); which frame is next is a Python counter, so a record() inside
    a replayed graph always writes the frame it wrote when captured.  save() brings the frames to the host."""

    def __init__(self, viewer: Viewer, max_frames: int):
        self.viewer, self.max_frames = viewer, int(max_frames)
        if self.max_frames < 1:
            raise ValueError("FrameRecorder: max_frames < 1")
        self.count = 0
        self.frames = None

    def record(self):
        if self.count >= self.max_frames:
            raise RuntimeError(f"FrameRecorder: all {self.max_frames} frames are taken")
        v = self.viewer
        if v.images is None:
            raise RuntimeError("FrameRecorder.record: the viewer has not drawn yet")
        if self.frames is None:
            import torch
            self.frames = torch.zeros(self.max_frames, v.height, v.width, 4, dtype=torch.uint8, device=v.images["rgba"].device)
        self.frames[self.count].copy_(v.images["rgba"])
        self.count += 1

    def save(self, directory, apng: Optional[str] = None, fps: float = 25.0) -> list:
        """frame_%06d.png for every recorded frame, in `directory` (made if missing); apng="name.png": also one animated
        PNG of them all.  Returns the paths written."""
        os.makedirs(directory, exist_ok=True)
        frames = self.frames[:self.count].cpu().numpy() if self.count else np.zeros((0, 1, 1, 4), np.uint8)
        paths = []
        for k in range(self.count):
            paths.append(os.path.join(directory, "frame_%06d.png" % k))
            write_png(paths[-1], frames[k])
        if apng is not None and self.count:
            paths.append(os.path.join(directory, apng))
            write_apng(paths[-1], list(frames), fps=fps)
        return paths
