"""The ray caster's host side, without a GPU: the pattern generators (shifu_amd/raycast.py), the shape mask, the ABI
entries and their ctypes signatures, the budgets of the two kernels, and the config / unit / facade surface."""
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- patterns ---------------------------------------------------------------------------------------------------------
def test_grid_pattern_counts_order_and_direction():
    from shifu_amd.raycast import grid_pattern
    o, d = grid_pattern()
    assert o.shape == d.shape == (17 * 11, 3) and o.dtype == d.dtype == np.float32
    np.testing.assert_allclose(o[:11, 0], -0.8, atol=1e-6)                   # x-major: the first row of y values
    np.testing.assert_allclose(o[:11, 1], np.arange(-0.5, 0.5 + 1e-9, 0.1), atol=1e-6)
    np.testing.assert_allclose(o[::11, 0], np.arange(-0.8, 0.8 + 1e-9, 0.1), atol=1e-6)
    assert (o[:, 2] == 0).all() and (d == [0, 0, -1]).all()
    o, d = grid_pattern((1.56, 1.04), 0.13)
    assert len(o) == 13 * 9 == 117
    o, d = grid_pattern((0.2, 0.0), 0.1, direction=(1.0, 0.0, -1.0))
    assert len(o) == 3 and (d == [1, 0, -1]).all()                           # directions need not be unit
    for bad in (dict(resolution=0.0), dict(resolution=-0.1), dict(size=(np.inf, 1.0)), dict(direction=(0, 0, 0)),
                dict(direction=(0, np.nan, -1)), dict(size=(-1.0, 1.0))):
        with pytest.raises(ValueError):
            grid_pattern(**bad)


def test_lidar_pattern_counts_order_and_unit_directions():
    from shifu_amd.raycast import lidar_pattern
    o, d = lidar_pattern(16, (-25, 15), horizontal_res=4.0)
    assert o.shape == d.shape == (1440, 3) and d.dtype == np.float32 and (o == 0).all()
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)
    el = np.degrees(np.arcsin(d[:, 2].astype(np.float64))).reshape(16, 90)
    az = np.degrees(np.arctan2(d[:, 1].astype(np.float64), d[:, 0].astype(np.float64))).reshape(16, 90)
    np.testing.assert_allclose(el, np.linspace(-25, 15, 16)[:, None] + 0 * el, atol=1e-4)     # channel-major
    np.testing.assert_allclose(az[:, 1:], (-180 + 4.0 * np.arange(1, 90))[None, :] + 0 * az[:, 1:], atol=1e-4)
    assert abs(abs(az[0, 0]) - 180) < 1e-4                                  # the first azimuth is hfov[0]; the last is 176, not 180
    o, d = lidar_pattern(1, (0, 0), (-45, 45), 30.0)
    assert len(d) == 3 and np.allclose(np.degrees(np.arctan2(d[:, 1], d[:, 0])), [-45, -15, 15], atol=1e-4)
    assert len(lidar_pattern(4)[0]) == 4 * 360
    for bad in (dict(channels=0), dict(channels=2, horizontal_res=0.0), dict(channels=2, horizontal_fov=(10, 10)),
                dict(channels=2, vertical_fov=(np.nan, 1)), dict(channels=2, horizontal_fov=(0, 0.1), horizontal_res=1.0)):
        with pytest.raises(ValueError):
            lidar_pattern(**bad)


def test_pinhole_pattern_is_the_camera_convention():
    from shifu_amd.raycast import pinhole_pattern
    from shifu_amd.render import pixel_rays
    o, d = pinhole_pattern(64, 48, 87)
    assert d.shape == (64 * 48, 3) and (o == 0).all()
    np.testing.assert_array_equal(d, pixel_rays((0, 0, 0, 1.0), 64, 48, 87.0).reshape(-1, 3).astype(np.float32))   # row-major
    assert (d[:, 0] == 1).all()                                              # view-axis component 1
    assert d[0, 1] > 0 and d[0, 2] > 0 and d[-1, 1] < 0 and d[-1, 2] < 0      # top left is +y (left), +z (up)
    for bad in ((0, 4, 60), (4, 4, 0), (4, 4, 180)):
        with pytest.raises(ValueError):
            pinhole_pattern(*bad)


def test_check_pattern_refuses():
    from shifu_amd.raycast import check_pattern
    good = np.zeros((2, 3)), np.array([[0, 0, -1.0], [1, 0, 0]])
    o, d = check_pattern(*good)
    assert o.dtype == d.dtype == np.float32 and o.flags.c_contiguous
    for o, d in ((np.zeros((2, 3)), np.zeros((2, 3))), (np.zeros((2, 3)), np.array([[0, 0, -1.0], [np.inf, 0, 0]])),
                 (np.full((2, 3), np.nan), good[1]), (np.zeros((2, 2)), np.ones((2, 2))), (np.zeros((3, 3)), good[1]),
                 (np.zeros((0, 3)), np.zeros((0, 3)))):
        with pytest.raises(ValueError):
            check_pattern(o, d)


# ---- the shape mask -----------------------------------------------------------------------------------------------------
def test_shape_mask_for():
    from shifu_amd.model import RenderShape
    from shifu_amd.render import build_scene, shape_mask_for
    box = lambda b: RenderShape(b, "box", np.zeros(3), np.eye(3), np.array([0.1, 0.1, 0.1]))
    sc = build_scene([box(0), box(0), box(1), box(2)], 3, boxes=[(0.2, 0.2, 0.2), (0.1, 0.1, 0.1)])
    assert sc.nshapes == 6 and sc.num_bodies == 5
    assert shape_mask_for(sc) == 0b111111
    assert shape_mask_for(sc, [0]) == 0b111100                               # both shapes of body 0
    assert shape_mask_for(sc, range(3)) == 0b110000                          # the articulation: the box actors stay
    assert shape_mask_for(sc, [3, 1]) == 0b101011
    assert shape_mask_for(sc, range(5)) == 0
    with pytest.raises(ValueError):
        shape_mask_for(sc, [5])
    full = build_scene([box(k) for k in range(64)], 64)
    assert shape_mask_for(full) == 2 ** 64 - 1 and shape_mask_for(full, [63]) == 2 ** 63 - 1


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_abi_entries_and_constants():
    hdr = open(os.path.join(ROOT, "include", "shifu_amd.h")).read()
    for name, nargs in (("shf_raycast", 20), ("shf_camera_points", 7), ("shf_raycast_debug_cull", 1)):
        m = re.search(r"^int " + name + r"\(([^;]*)\);", hdr, re.M)
        assert m, name + " is not declared in include/shifu_amd.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib._SIGS[name][0]), name
        assert name in _lib.EXPORTS
    for k, v in (("BASE", 0), ("YAW", 1), ("WORLD", 2)):
        assert re.search(rf"#define SHF_RAY_ALIGN_{k}\s+{v}\b", hdr) and getattr(_abi, "RAY_ALIGN_" + k) == v
    from shifu_amd.raycast import ALIGN
    assert ALIGN == {"base": 0, "yaw": 1, "world": 2}
    assert re.search(r"#define SHF_ABI_VERSION\s+(\d+)", hdr).group(1) == str(_abi.SHF_ABI_VERSION)     # not bumped: additive


def test_built_library_exports_and_budgets():
    import ctypes as C
    from shifu_amd import build
    assert os.path.exists(build.LIB), "libshifu_amd.so is not built"
    lib = C.CDLL(build.LIB)
    for name in ("shf_raycast", "shf_camera_points", "shf_raycast_debug_cull"):
        assert hasattr(lib, name), name
    prefixes = {p: (v, s) for p, v, s in build.BUDGETS}
    assert prefixes["_Z9k_raycast"][1] == 0 and prefixes["_Z12k_raycast_tw"][1] == 0        # no scratch
    if os.path.exists(build.RESOURCES):
        import json
        res = json.load(open(build.RESOURCES))
        build.check_budgets(res)
        for p in ("_Z9k_raycast", "_Z12k_raycast_tw"):
            ks = [v for k, v in res.items() if k.startswith(p)]
            assert len(ks) == 1 and ks[0]["scratch"] == 0


# ---- config, unit, facade -------------------------------------------------------------------------------------------------
def test_config_and_unit_construction():
    from shifu_amd import compat
    from shifu_amd.configs import BaseSensorConfig, RayCasterSensorConfig
    from shifu_amd.raycast import grid_pattern, lidar_pattern
    from shifu_amd.units import RayCasterSensor, Sensor
    compat.install()
    import shifu.configs
    import shifu.units
    assert shifu.units.RayCasterSensor is RayCasterSensor and shifu.configs.RayCasterSensorConfig is RayCasterSensorConfig
    assert issubclass(RayCasterSensorConfig, BaseSensorConfig) and issubclass(RayCasterSensor, Sensor)
    base = RayCasterSensorConfig()
    assert (base.align, base.min_range, base.max_range, base.ignore_robot) == ("base", 0.0, 10.0, True)
    assert base.pattern is None and base.transform is None and base.attach_local_transform is None and base.attach_body_name is None

    class Scan(RayCasterSensorConfig):
        name = "scan"
        pattern = grid_pattern()
        attach_local_transform = [[0.0, 0.0, 0.5], [0.0, 0.0, 0.0, 1.0]]
        attach_body_name = "trunk"
        align = "yaw"
        max_range = 3.0

    s = RayCasterSensor(Scan())
    assert s.num_rays == 187 and s.name == "scan" and s.origins.dtype == np.float32
    with pytest.raises(ValueError):
        RayCasterSensor(RayCasterSensorConfig())                           # no pattern

    class Both(Scan):
        transform = [[0, 0, 1.0], [0, 0, 0, 1.0]]

    class Nowhere(Scan):
        attach_local_transform = None

    class Loose(Scan):
        attach_body_name = None

    class Sideways(Scan):
        align = "sideways"

    class Zero(Scan):
        pattern = (np.zeros((2, 3)), np.zeros((2, 3)))

    for cfg in (Both, Nowhere, Loose, Sideways, Zero):
        with pytest.raises(ValueError):
            RayCasterSensor(cfg())

    class Lidar(RayCasterSensorConfig):
        pattern = lidar_pattern(4)
        transform = [[0, 0, 1.0], [0, 0, 0, 1.0]]

    assert RayCasterSensor(Lidar()).num_rays == 1440


def test_facade_and_fused_surface():
    from shifu_amd.gym.fused_camera import FusedCamera, FusedCameraHost, FusedRayCaster
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.render import Renderer
    from shifu_amd.units import CameraSensor
    for name in ("create_ray_caster_group", "cast_ray_caster_group", "camera_group_points"):
        assert "Not an Isaac Gym call" in getattr(gymapi.Gym, name).__doc__
    assert callable(Renderer.raycast) and callable(Renderer.camera_points) and callable(CameraSensor.point_cloud)
    assert callable(FusedCameraHost.add_ray_caster) and callable(FusedCamera.point_cloud)
    assert callable(FusedRayCaster.cast) and callable(FusedRayCaster.world_pose)
    sim = gymapi.acquire_gym().create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    assert sim.ray_caster_groups == []
    with pytest.raises(NotImplementedError):                                  # before prepare_sim there is no scene to cast in
        gymapi.acquire_gym().create_ray_caster_group(sim, (np.zeros((1, 3)), np.array([[0, 0, -1.0]])))
