"""Ray-caster sensors: the ray patterns behind include/shifu_amd.h shf_raycast (csrc/shf_render.hip, k_raycast).

A pattern is (origins (R, 3), dirs (R, 3)), float32 numpy arrays in the SENSOR frame (+x forward, +y left, +z up, the
camera's frame): ray r of env e starts at p_e + R o_r and runs along unit(R d_r), with R the sensor's rotation as the
caster's `align` takes it (ALIGN: "base" all of it, "yaw" its yaw about world z only, "world" none).  The ray parameter is
the Euclidean range.  Patterns come out in scan order -- neighbouring rays are neighbours in the array -- which is what
lets the kernel's per-wave ballot skip most shapes.  Renderer.raycast (shifu_amd/render.py) casts them; the fused envs'
add_ray_caster and units.RayCasterSensor are built on it.  Conventions: DESIGN.md 8e "Ray caster"."""
from typing import Tuple

import numpy as np

from . import _abi

ALIGN = {"base": _abi.RAY_ALIGN_BASE, "yaw": _abi.RAY_ALIGN_YAW, "world": _abi.RAY_ALIGN_WORLD}


def check_pattern(origins, dirs) -> Tuple[np.ndarray, np.ndarray]:
    """(origins, dirs) as contiguous float32 (R, 3) arrays, R >= 1; refuses values that are not finite and zero directions."""
    o, d = np.ascontiguousarray(origins, np.float32), np.ascontiguousarray(dirs, np.float32)
    if o.ndim != 2 or o.shape[1] != 3 or o.shape != d.shape or o.shape[0] < 1:
        raise ValueError(f"ray pattern: origins and dirs must both be (R, 3) with R >= 1, got {o.shape} and {d.shape}")
    if not (np.isfinite(o).all() and np.isfinite(d).all()):
        raise ValueError("ray pattern: origins and dirs must be finite")
    if not (np.einsum("ij,ij->i", d.astype(np.float64), d.astype(np.float64)) > 0.0).all():
        raise ValueError("ray pattern: a direction is zero")
    return o, d


def _axis(lo: float, hi: float, step: float) -> np.ndarray:
    return np.arange(lo, hi + 1e-9, step)


def grid_pattern(size=(1.6, 1.0), resolution: float = 0.1, direction=(0.0, 0.0, -1.0)):
    """A height scanner: parallel rays from a grid in the sensor's xy plane, x = arange(-size[0] / 2, size[0] / 2 + 1e-9,
    resolution) and likewise y, x-major, origins (x, y, 0), every ray along `direction`."""
    sx, sy, res = float(size[0]), float(size[1]), float(resolution)
    if not (np.isfinite([sx, sy, res]).all() and sx >= 0.0 and sy >= 0.0 and res > 0.0):
        raise ValueError("grid_pattern: size must be >= 0 and resolution > 0, all finite")
    x, y = _axis(-0.5 * sx, 0.5 * sx, res), _axis(-0.5 * sy, 0.5 * sy, res)
    o = np.zeros((len(x), len(y), 3))
    o[..., 0], o[..., 1] = x[:, None], y[None, :]
    o = o.reshape(-1, 3)
    return check_pattern(o, np.broadcast_to(np.asarray(direction, float), o.shape))


def lidar_pattern(channels: int, vertical_fov=(-15.0, 15.0), horizontal_fov=(-180.0, 180.0), horizontal_res: float = 1.0):
    """A spinning lidar: `channels` rings at elevations linspace(vertical_fov) (degrees, up positive), azimuths
    horizontal_fov[0] + horizontal_res k for k < round((horizontal_fov[1] - horizontal_fov[0]) / horizontal_res) (degrees,
    counter-clockwise from +x), channel-major, d = (cos e cos a, cos e sin a, sin e), every origin 0."""
    channels, res = int(channels), float(horizontal_res)
    (v0, v1), (h0, h1) = (float(v) for v in vertical_fov), (float(v) for v in horizontal_fov)
    if channels < 1 or not (np.isfinite([v0, v1, h0, h1, res]).all() and res > 0.0 and h1 > h0):
        raise ValueError("lidar_pattern: channels >= 1, horizontal_res > 0 and horizontal_fov[1] > horizontal_fov[0], all finite")
    n = int(round((h1 - h0) / res))
    if n < 1:
        raise ValueError("lidar_pattern: horizontal_fov and horizontal_res leave no azimuth")
    e = np.deg2rad(np.linspace(v0, v1, channels))[:, None]
    a = np.deg2rad(h0 + res * np.arange(n))[None, :]
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e) + 0.0 * a], axis=-1).reshape(-1, 3)
    return check_pattern(np.zeros_like(d), d)


def pinhole_pattern(width: int, height: int, horizontal_fov: float):
    """The camera convention's pixel rays in the sensor frame, row-major (row 0 at the top): render.pixel_rays of the
    identity quaternion, so their component along the view axis (+x) is 1 and range = view depth x |d|.  Every origin 0."""
    from .render import pixel_rays
    width, height, fov = int(width), int(height), float(horizontal_fov)
    if width < 1 or height < 1 or not 0.0 < fov < 180.0:
        raise ValueError("pinhole_pattern: width, height >= 1 and horizontal_fov in (0, 180) degrees")
    d = pixel_rays((0.0, 0.0, 0.0, 1.0), width, height, fov).reshape(-1, 3)
    return check_pattern(np.zeros_like(d), d)
