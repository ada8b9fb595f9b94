"""Camera sensors: the scene description behind include/shifu_amd.h shf_render_cameras (csrc/shf_render.hip).

A render scene holds every collision shape of the articulation (CompiledModel.render_shapes) and of the box actors in the
frame of the body that moves it, plus the terrain; the kernel casts one ray per pixel against them.  This module also
owns the conventions the kernel mirrors (DESIGN.md "Camera sensors"):

  * a camera pose (pos, quat xyzw) looks along its local +x with +z up (Isaac Gym's camera transform);
  * pixel (row r, col c), row 0 at the top, casts  dir = fwd + right x t + up y t H/W,  t = tan(hfov / 2),
    x = 2 (c + 1/2) / W - 1,  y = 1 - 2 (r + 1/2) / H  -- so the ray parameter is the view-space depth;
  * view / projection matrices are row-vector 4 x 4 (p_clip = [p, 1] @ view @ proj, the form of the reference's
    shifu/utils/camera.py), proj[0, 0] = 1 / t, proj[1, 1] = proj[0, 0] W / H;
  * color = body color x (AMBIENT + DIFFUSE max(0, n . LIGHT)) rounded to u8, alpha 255; background BACKGROUND;
  * optical flow (shf_render_cameras_flow): for the surface point X a pixel (r, c) shows on body b, X' = p_b' + R_b' R_b^T
    (X - p_b) is where it was at the previous flow render (primed: that render's body pose; the terrain does not move);
    projected into the previous camera pose with the pixel-ray convention it lands at (r', c'), and flow = (c - c', r - r')
    in pixels, u to the right, v downwards -- backward-looking.  Exactly +0.0 where nothing is hit, where the point was
    behind the previous camera, where the env's previous frame is marked invalid (FlowHistory) and where neither the
    body's pose nor the camera's changed bits.  flow_to_i16 / flow_from_i16: Isaac Gym's int16 encoding.
  * ray caster (shf_raycast; Renderer.raycast, shifu_amd/raycast.py): arbitrary rays per env from a sensor pose; the ray
    parameter is the Euclidean range, not the view depth; otherwise the cameras' hit and tie rules.  Renderer.camera_points
    (shf_camera_points): the point o + |depth| d behind every pixel of a rendered depth image.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _abi

AMBIENT, DIFFUSE = _abi.RENDER_AMBIENT, _abi.RENDER_DIFFUSE
LIGHT = np.array(_abi.RENDER_LIGHT, dtype=np.float64)
BACKGROUND = tuple(_abi.RENDER_BG)
DEFAULT_BODY_COLOR = (0.8, 0.8, 0.8)
DEFAULT_GROUND_COLOR = (0.5, 0.5, 0.5)
_KINDS = {"box": _abi.RENDER_BOX, "sphere": _abi.RENDER_SPHERE, "capsule": _abi.RENDER_CAPSULE, "hull": _abi.RENDER_POLY}


# -- conventions ------------------------------------------------------------------------------------------------------
def quat_to_mat(q) -> np.ndarray:
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def mat_to_quat(R) -> np.ndarray:
    """Unit quaternion (x, y, z, w) of a rotation matrix."""
    R = np.asarray(R, float)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    q = np.asarray(q)
    return q / np.linalg.norm(q)


def camera_basis(quat):
    """(fwd, right, up) of a camera pose: local +x, -(local +y), local +z."""
    R = quat_to_mat(quat)
    return R[:, 0], -R[:, 1], R[:, 2]


def lookat_quat(pos, target) -> np.ndarray:
    """The camera quaternion of set_camera_location(pos, target): looking from pos at target, world +z up."""
    f = np.asarray(target, float) - np.asarray(pos, float)
    n = np.linalg.norm(f)
    if n == 0.0:
        raise ValueError("camera position and target coincide")
    f = f / n
    r = np.cross(f, [0.0, 0.0, 1.0])
    if np.linalg.norm(r) < 1e-9:               # looking straight up or down: world +x / -x as the image's up
        r = np.cross(f, [1.0, 0.0, 0.0]) if f[2] < 0 else np.cross([1.0, 0.0, 0.0], f)
    r = r / np.linalg.norm(r)
    u = np.cross(r, f)
    return mat_to_quat(np.stack([f, -r, u], axis=1))


def pixel_rays(quat, width: int, height: int, horizontal_fov: float) -> np.ndarray:
    """(H, W, 3) ray directions (not unit: their component along fwd is 1) of a camera, row 0 at the top."""
    fwd, right, up = camera_basis(quat)
    t = np.tan(0.5 * np.deg2rad(horizontal_fov))
    x = 2.0 * (np.arange(width) + 0.5) / width - 1.0
    y = 1.0 - 2.0 * (np.arange(height) + 0.5) / height
    return (fwd[None, None, :] + right[None, None, :] * (x[None, :, None] * t)
            + up[None, None, :] * (y[:, None, None] * t * height / width))


def view_matrix(pos, quat) -> np.ndarray:
    """Row-vector world -> view matrix: [p, 1] @ V = (right . (p - o), up . (p - o), -fwd . (p - o), 1)."""
    fwd, right, up = camera_basis(quat)
    o = np.asarray(pos, float)
    V = np.eye(4)
    V[:3, 0], V[:3, 1], V[:3, 2] = right, up, -fwd
    V[3, :3] = [-right @ o, -up @ o, fwd @ o]
    return V


def proj_matrix(width: int, height: int, horizontal_fov: float, near: float, far: float) -> np.ndarray:
    """Row-vector perspective projection: ndc x = x_view / (t (-z_view)), ndc y = y_view W / (t H (-z_view)); the z row maps
    [near, far] to [-1, 1] (OpenGL)."""
    t = np.tan(0.5 * np.deg2rad(horizontal_fov))
    P = np.zeros((4, 4))
    P[0, 0] = 1.0 / t
    P[1, 1] = P[0, 0] * width / height
    P[2, 2] = -(far + near) / (far - near)
    P[2, 3] = -1.0
    P[3, 2] = -2.0 * far * near / (far - near)
    return P


def shade(color, normal) -> np.ndarray:
    """u8 RGB of a surface of `color` ([0, 1]) with unit outward normal `normal` (broadcasts over leading axes)."""
    lam = AMBIENT + DIFFUSE * np.maximum(np.sum(np.asarray(normal, float) * LIGHT, axis=-1), 0.0)
    return np.floor(np.clip(np.asarray(color, float) * lam[..., None], 0.0, 1.0) * 255.0 + 0.5).astype(np.uint8)


# -- scene --------------------------------------------------------------------------------------------------------------
def _fill_shape(rec, body: int, kind: str, pos, rot, param, radius: float, poly: int = -1):
    rec.body, rec.kind, rec.poly = int(body), _KINDS[kind], int(poly)
    rec.pos[:] = [float(v) for v in pos]
    rec.rot[:] = [float(v) for v in np.asarray(rot, float).reshape(-1)]
    p = list(param) + [0.0] * (3 - len(param))
    rec.param[:] = [float(v) for v in p[:3]]
    rec.radius = float(radius)


def build_scene(render_shapes: Sequence, nb: int, boxes: Sequence = (), ground: bool = True,
                ground_color=DEFAULT_GROUND_COLOR, height_samples: Optional[np.ndarray] = None,
                vscale: float = 1.0) -> "_abi.ShfRenderScene":
    """ShfRenderScene of an articulation's render shapes (model.RenderShape, bodies 0..nb-1) and box actors `boxes` (full
    extents (x, y, z) each; box k is body row nb + k, in its own frame): nb + len(boxes) body_state rows per env.
    height_samples / vscale: the height field's bounding box in z."""
    sc = _abi.ShfRenderScene()
    n_shapes = len(render_shapes) + len(boxes)
    if n_shapes > _abi.RENDER_MAX_SHAPES:
        raise ValueError(f"{n_shapes} shapes > SHF_RENDER_MAX_SHAPES = {_abi.RENDER_MAX_SHAPES}")
    if any(not 0 <= int(s.body) < nb for s in render_shapes):
        raise ValueError("render shape on a body outside 0..nb-1")
    k = npoly = 0
    for s in render_shapes:
        rec = sc.shape[k]
        size = np.asarray(s.size, float)
        if s.kind == "box":
            h = 0.5 * size
            _fill_shape(rec, s.body, "box", s.pos, s.rot, h, np.linalg.norm(h))
        elif s.kind == "sphere":
            _fill_shape(rec, s.body, "sphere", s.pos, s.rot, [size[0]], size[0])
        elif s.kind == "capsule":
            r, hl = float(size[0]), 0.5 * float(size[1])
            _fill_shape(rec, s.body, "capsule", s.pos, s.rot, [r, hl], r + hl)
        elif s.kind == "hull":
            if npoly >= _abi.RENDER_MAX_POLYS:
                raise ValueError(f"more than SHF_RENDER_MAX_POLYS = {_abi.RENDER_MAX_POLYS} convex polytopes")
            v, planes = np.asarray(s.poly["verts"], float), np.asarray(s.poly["planes"], float)
            if len(planes) > _abi.RENDER_POLY_MAX_FACES:
                raise ValueError(f"polytope with {len(planes)} faces > SHF_RENDER_POLY_MAX_FACES")
            c = v.mean(0)                        # re-centred: the bounding sphere is taken about the vertex centroid
            P = sc.poly[npoly]
            P.nf = len(planes)
            for f, pl in enumerate(planes):
                P.plane[f][:] = [float(pl[0]), float(pl[1]), float(pl[2]), float(pl[3] - pl[:3] @ c)]
            rot = np.asarray(s.rot, float)
            _fill_shape(rec, s.body, "hull", np.asarray(s.pos, float) + rot @ c, rot, [], np.linalg.norm(v - c, axis=1).max(), npoly)
            npoly += 1
        else:
            raise ValueError(f"render shape kind {s.kind!r}")
        k += 1
    for j, dim in enumerate(boxes):
        h = 0.5 * np.asarray(dim, float)
        _fill_shape(sc.shape[k], nb + j, "box", np.zeros(3), np.eye(3), h, np.linalg.norm(h))
        k += 1
    sc.nshapes, sc.npolys = k, npoly
    sc.num_bodies = int(nb) + len(boxes)
    sc.ground = int(bool(ground))
    sc.ground_color[:] = [float(v) for v in ground_color]
    if height_samples is not None and np.asarray(height_samples).size:
        z = np.asarray(height_samples, np.float64) * float(vscale)
        sc.hf_zmin, sc.hf_zmax = float(z.min()), float(z.max())
    return sc


def camera_struct(width: int, height: int, horizontal_fov: float, near: float, far: float,
                  depth_negative: bool = False) -> "_abi.ShfCamera":
    c = _abi.ShfCamera()
    c.width, c.height = int(width), int(height)
    c.horizontal_fov, c.near_plane, c.far_plane = float(horizontal_fov), float(near), float(far)
    c.depth_negative = int(bool(depth_negative))
    return c


class Renderer:
    """Device copies of one render scene (+ the terrain) and the launch of shf_render_cameras.

    heights: the (rows, cols) int16 samples, host or device.  A warped terrain (ShfTerrain.warped, the triangle mesh
    convert_heightfield_to_trimesh makes) takes the packed payload the sim holds -- samples followed by one byte per vertex
    (terrain_utils.pack_trimesh_samples) -- either as that flat int16 array / device tensor, or as the samples plus `warp`,
    the (rows, cols) uint8 bytes of terrain_utils.trimesh_warp_map, which are packed here."""

    def __init__(self, scene: "_abi.ShfRenderScene", terrain: Optional["_abi.ShfTerrain"] = None, heights=None,
                 device="cuda:0", warp=None):
        import torch
        from .backend import _struct_to_device
        self.device = torch.device(device)
        if terrain is None:
            terrain = _abi.ShfTerrain()
            terrain.hscale = terrain.vscale = 1.0
        if warp is not None and not terrain.warped:
            raise ValueError("Renderer: warp bytes given for a terrain that is not warped")
        self.scene, self.terrain = scene, terrain
        self._scene_dev = _struct_to_device(scene, self.device)
        self._heights = None
        if terrain.rows > 0:
            nv = int(terrain.rows) * int(terrain.cols)
            if warp is not None:
                from .isaacgym.terrain_utils import pack_trimesh_samples
                hs = heights.cpu().numpy() if isinstance(heights, torch.Tensor) else np.asarray(heights)
                if hs.size != nv or np.asarray(warp).size != nv:
                    raise ValueError(f"Renderer: samples and warp bytes must hold rows x cols = {nv} values each")
                heights = pack_trimesh_samples(hs, warp)
            h = heights if isinstance(heights, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(heights, np.int16))
            need = nv + (nv + 1) // 2 if terrain.warped else nv
            if h.dtype != torch.int16 or h.numel() < need:
                raise ValueError(f"Renderer: the terrain needs {need} int16 values (a warped terrain: samples followed by "
                                 f"one byte per vertex), got {h.numel()} {h.dtype}")
            self._heights = h.to(self.device).contiguous()

    def render(self, body_state, cam_pose, seg, color, camera: "_abi.ShfCamera", depth=None, seg_out=None, rgba=None,
               flow=None, flow_i16=None, prev_body_pose=None, prev_cam_pose=None, prev_valid=None):
        """One launch for all envs: body_state (N * num_bodies, 13), cam_pose (N, 7), seg (N, num_bodies) int32, color
        (N, num_bodies, 3) f32; writes depth (N, H, W) f32, seg_out (N, H, W) int32 and rgba (N, H, W, 4) u8, each optional.

        Optical flow (module docstring): with flow (N, H, W, 2) f32 pixels and / or flow_i16 (N, H, W, 2) int16 given, the
        launch is shf_render_cameras_flow and needs the previous flow render's prev_body_pose (N * num_bodies, 7),
        prev_cam_pose (N, 7) and prev_valid (N,) int32 (0: that env's flow is zero) -- a FlowHistory holds them."""
        import torch
        from ._lib import check, lib
        from .backend import _stream_ptr
        n = int(cam_pose.shape[0])
        B, H, W = self.scene.num_bodies, camera.height, camera.width
        with_flow = flow is not None or flow_i16 is not None
        if with_flow and (prev_body_pose is None or prev_cam_pose is None or prev_valid is None):
            raise ValueError("render: a flow output needs prev_body_pose, prev_cam_pose and prev_valid (render.FlowHistory)")
        for t, shape, dt in ((body_state, (n * B, 13), torch.float32), (cam_pose, (n, 7), torch.float32),
                             (seg, (n, B), torch.int32), (color, (n, B, 3), torch.float32),
                             (depth, (n, H, W), torch.float32), (seg_out, (n, H, W), torch.int32),
                             (rgba, (n, H, W, 4), torch.uint8), (flow, (n, H, W, 2), torch.float32),
                             (flow_i16, (n, H, W, 2), torch.int16), (prev_body_pose, (n * B, 7), torch.float32),
                             (prev_cam_pose, (n, 7), torch.float32), (prev_valid, (n,), torch.int32)):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"render: expected a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            if with_flow:
                check(lib().shf_render_cameras_flow(ptr(self._scene_dev), C.byref(self.terrain), ptr(self._heights),
                                                    C.byref(camera), n, ptr(body_state), ptr(cam_pose), ptr(seg), ptr(color),
                                                    ptr(depth), ptr(seg_out), ptr(rgba), ptr(prev_body_pose), ptr(prev_cam_pose),
                                                    ptr(prev_valid), ptr(flow), ptr(flow_i16), _stream_ptr(self.device)))
                return
            check(lib().shf_render_cameras(ptr(self._scene_dev), C.byref(self.terrain), ptr(self._heights), C.byref(camera), n,
                                           ptr(body_state), ptr(cam_pose), ptr(seg), ptr(color), ptr(depth), ptr(seg_out),
                                           ptr(rgba), _stream_ptr(self.device)))

    def render_world(self, body_state, view_pose, seg, color, camera: "_abi.ShfCamera", env_ids=None, env_offset=None,
                     env_radius: float = 0.0, depth=None, seg_out=None, rgba=None, env_out=None):
        """One launch of shf_render_world: view_pose (V, 7) cameras that each see many envs.  body_state (N * num_bodies,
        13), seg (N, num_bodies) int32 and color (N, num_bodies, 3) f32 are render()'s per-env tables, N their number of
        rows.  env_ids (E,) int32: the envs drawn (None: all N, in order); env_offset (E, 3) f32: the displacement of the
        env at each LIST POSITION (None: zeros); env_radius > 0: a sphere about body 0 that bounds every env, for the
        env-level cull (0: none).  Writes depth (V, H, W) f32, seg_out (V, H, W) int32, rgba (V, H, W, 4) u8 and env_out
        (V, H, W) int32 -- the env id a pixel shows, -1 for the terrain or nothing -- each optional.  The tie rule: module
        docstring of shifu_amd/viewer.py.  A warped terrain takes the kernel's trimesh form."""
        import torch
        from ._lib import check, lib
        from .backend import _stream_ptr
        B, H, W = self.scene.num_bodies, camera.height, camera.width
        for name, t in (("body_state", body_state), ("view_pose", view_pose), ("seg", seg)):
            if not isinstance(t, torch.Tensor) or t.dim() < 1:
                raise ValueError(f"render_world: {name} must be a tensor")
        n, v = int(seg.shape[0]), int(view_pose.shape[0])
        if n < 1 or v < 1:
            raise ValueError("render_world: no envs or no views")
        e = n if env_ids is None else int(env_ids.shape[0]) if env_ids.dim() == 1 else -1
        if e < 1:
            raise ValueError("render_world: env_ids must be a non-empty (E,) int32 tensor")
        for t, shape, dt in ((body_state, (n * B, 13), torch.float32), (view_pose, (v, 7), torch.float32),
                             (seg, (n, B), torch.int32), (color, (n, B, 3), torch.float32), (env_ids, (e,), torch.int32),
                             (env_offset, (e, 3), torch.float32), (depth, (v, H, W), torch.float32),
                             (seg_out, (v, H, W), torch.int32), (rgba, (v, H, W, 4), torch.uint8),
                             (env_out, (v, H, W), torch.int32)):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"render_world: expected a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        if not np.isfinite(float(env_radius)):
            raise ValueError("render_world: env_radius must be finite")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            check(lib().shf_render_world(ptr(self._scene_dev), C.byref(self.terrain), ptr(self._heights), C.byref(camera), v,
                                         ptr(view_pose), n, e, ptr(env_ids), ptr(env_offset), C.c_float(float(env_radius)),
                                         ptr(body_state), ptr(seg), ptr(color), ptr(depth), ptr(seg_out), ptr(rgba),
                                         ptr(env_out), _stream_ptr(self.device)))

    def raycast(self, body_state, sensor_pose, origins_dev, dirs_dev, align, min_range: float, max_range: float,
                shape_mask: int, seg=None, dist=None, points=None, normal=None, seg_out=None, body=None):
        """One launch of shf_raycast (shifu_amd/raycast.py): the pattern origins_dev / dirs_dev (R, 3) f32 on the device, the
        same in every env, from sensor_pose (N, 7); body_state (N * num_bodies, 13) as for render().  align: _abi.RAY_ALIGN_*
        or "base" | "yaw" | "world"; [min_range, max_range]: Euclidean ranges; shape_mask: bit k = shape k of the scene is
        cast (shape_mask_for).  Writes, each optional but not all None: dist (N, R) f32 (+inf: a miss), points (N, R, 3) f32
        world frame (a miss: the ray's end at max_range), normal (N, R, 3) f32, seg_out (N, R) int32 (needs seg, the (N,
        num_bodies) int32 table) and body (N, R) int32 -- the hit body's row within the env, -1 terrain, -2 a miss."""
        import torch
        from ._lib import check, lib
        from .backend import _stream_ptr
        from .raycast import ALIGN
        for name, t in (("body_state", body_state), ("sensor_pose", sensor_pose), ("origins_dev", origins_dev), ("dirs_dev", dirs_dev)):
            if not isinstance(t, torch.Tensor) or t.dim() < 1:
                raise ValueError(f"raycast: {name} must be a tensor")
        n, R, B = int(sensor_pose.shape[0]), int(origins_dev.shape[0]), self.scene.num_bodies
        if n < 1 or R < 1:
            raise ValueError("raycast: no envs or no rays")
        if isinstance(align, str):
            if align not in ALIGN:
                raise ValueError(f"raycast: align must be one of {sorted(ALIGN)}, got {align!r}")
            align = ALIGN[align]
        if int(align) not in ALIGN.values():
            raise ValueError(f"raycast: align {align} outside 0..2")
        lo, hi = float(min_range), float(max_range)
        if not (0.0 <= lo <= hi and np.isfinite(hi)):
            raise ValueError("raycast: need 0 <= min_range <= max_range, max_range finite")
        if dist is None and points is None and normal is None and seg_out is None and body is None:
            raise ValueError("raycast: no output tensor given")
        if seg_out is not None and seg is None:
            raise ValueError("raycast: seg_out needs the seg table")
        for t, shape, dt in ((body_state, (n * B, 13), torch.float32), (sensor_pose, (n, 7), torch.float32),
                             (origins_dev, (R, 3), torch.float32), (dirs_dev, (R, 3), torch.float32), (seg, (n, B), torch.int32),
                             (dist, (n, R), torch.float32), (points, (n, R, 3), torch.float32),
                             (normal, (n, R, 3), torch.float32), (seg_out, (n, R), torch.int32), (body, (n, R), torch.int32)):
            if t is None:
                continue
            if tuple(t.shape) != shape or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"raycast: expected a contiguous {dt} tensor of shape {shape} on {self.device}, got "
                                 f"{tuple(t.shape)} {t.dtype} on {t.device}")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(self.device):
            check(lib().shf_raycast(ptr(self._scene_dev), C.byref(self.terrain), ptr(self._heights), n, R, ptr(origins_dev),
                                    ptr(dirs_dev), ptr(body_state), ptr(sensor_pose), int(align), C.c_float(lo), C.c_float(hi),
                                    C.c_uint64(int(shape_mask) & 0xFFFFFFFFFFFFFFFF), ptr(seg), ptr(dist), ptr(points),
                                    ptr(normal), ptr(seg_out), ptr(body), _stream_ptr(self.device)))

    def camera_points(self, depth, cam_pose, camera: "_abi.ShfCamera", points, world_frame: bool = True):
        """One launch of shf_camera_points: the point behind every pixel of a rendered depth image (N, H, W) -- either sign
        convention; a pixel that shows nothing: the point at far_plane along its ray -- into points (N, H, W, 3) f32, in
        world coordinates from cam_pose (N, 7), or with world_frame=False in the camera's axes (+x view axis, +y left, +z up)."""
        import torch
        from ._lib import check, lib
        from .backend import _stream_ptr
        if not isinstance(depth, torch.Tensor) or depth.dim() != 3:
            raise ValueError("camera_points: depth must be an (N, H, W) tensor")
        n, H, W = int(depth.shape[0]), camera.height, camera.width
        if n < 1:
            raise ValueError("camera_points: no envs")
        for t, shape in ((depth, (n, H, W)), (cam_pose, (n, 7)), (points, (n, H, W, 3))):
            if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"camera_points: expected a contiguous float32 tensor of shape {shape} on {self.device}, got "
                                 + ("None" if t is None else f"{tuple(t.shape)} {t.dtype} on {t.device}"))
        with torch.cuda.device(self.device):
            check(lib().shf_camera_points(C.byref(camera), n, C.c_void_p(depth.data_ptr()), C.c_void_p(cam_pose.data_ptr()),
                                          int(bool(world_frame)), C.c_void_p(points.data_ptr()), _stream_ptr(self.device)))


def shape_mask_for(scene: "_abi.ShfRenderScene", ignore_bodies=()) -> int:
    """shf_raycast's 64-bit shape_mask of a scene: bit k set for every shape k whose body row is not in ignore_bodies (rows
    within the env, 0 .. num_bodies - 1)."""
    ignore = {int(b) for b in ignore_bodies}
    bad = [b for b in ignore if not 0 <= b < int(scene.num_bodies)]
    if bad:
        raise ValueError(f"shape_mask_for: body rows {sorted(bad)} outside the scene's 0..{int(scene.num_bodies) - 1}")
    mask = 0
    for k in range(int(scene.nshapes)):
        if int(scene.shape[k].body) not in ignore:
            mask |= 1 << k
    return mask


# -- optical flow -------------------------------------------------------------------------------------------------------
def flow_to_i16(flow, W: int, H: int):
    """Isaac Gym's integer encoding of a (..., 2) pixel flow (u, v): q_u = sat16(rint(u 32768 / W)), q_v = sat16(rint(v
    32768 / H)) as (..., 2) int16 -- float32 arithmetic as the kernel's (u x 32768 is exact, one correctly rounded division,
    round half to even, saturation to [-32768, 32767]).  torch tensor or numpy array in, the same kind out."""
    try:
        import torch
        is_torch = isinstance(flow, torch.Tensor)
    except ImportError:
        is_torch = False
    if is_torch:
        f = flow.to(torch.float32)
        scale = torch.tensor([float(W), float(H)], dtype=torch.float32, device=f.device)
        return torch.clamp(torch.round(f * 32768.0 / scale), -32768.0, 32767.0).to(torch.int16)
    f = np.asarray(flow, np.float32)
    q = np.rint((f * np.float32(32768.0)) / np.array([W, H], np.float32))
    return np.clip(q, -32768.0, 32767.0).astype(np.int16)


def flow_from_i16(q, W: int, H: int):
    """The pixel flow (..., 2) float32 of flow_to_i16's integers: u = q_u W / 32768, v = q_v H / 32768 (what the
    reference's normalize_optical_flow means to compute)."""
    try:
        import torch
        is_torch = isinstance(q, torch.Tensor)
    except ImportError:
        is_torch = False
    if is_torch:
        scale = torch.tensor([float(W), float(H)], dtype=torch.float32, device=q.device)
        return q.to(torch.float32) * scale / 32768.0
    return np.asarray(q).astype(np.float32) * np.array([W, H], np.float32) / np.float32(32768.0)


class FlowHistory:
    """What a camera (or camera group) keeps between two flow renders: the body poses and camera poses of the previous
    one and, per env, whether they are usable.  Everything is allocated here; update() is two strided copies and a fill on
    the current stream -- no allocation, no host sync, capturable.  Born invalid: the first render's flow is zero."""

    def __init__(self, num_envs: int, num_bodies: int, device):
        import torch
        self.num_envs, self.num_bodies = int(num_envs), int(num_bodies)
        self.prev_body_pose = torch.zeros(self.num_envs * self.num_bodies, 7, dtype=torch.float32, device=device)
        self.prev_cam_pose = torch.zeros(self.num_envs, 7, dtype=torch.float32, device=device)
        self.prev_valid = torch.zeros(self.num_envs, dtype=torch.int32, device=device)

    def update(self, body_state, cam_pose):
        """After a flow render on (body_state, cam_pose): they become the previous frame, valid in every env."""
        self.prev_body_pose.copy_(body_state[:, :7])
        self.prev_cam_pose.copy_(cam_pose)
        self.prev_valid.fill_(1)

    def invalidate(self, env_ids=None):
        """The next flow render is zero in env_ids (all envs by default): after a reset or a teleport."""
        if env_ids is None:
            self.prev_valid.zero_()
        else:
            import torch
            ids = torch.as_tensor(env_ids, device=self.prev_valid.device).long()
            self.prev_valid.index_fill_(0, ids, 0)

    def tensors(self) -> dict:
        return dict(prev_body_pose=self.prev_body_pose, prev_cam_pose=self.prev_cam_pose, prev_valid=self.prev_valid)
