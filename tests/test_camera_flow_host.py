"""Optical-flow images of the camera sensors, host side (no GPU): the C entry shf_render_cameras_flow and its binding, the
int16 encoding helpers, the SHIFU_AMD_OPTICAL_FLOW opt-in of the facade and CameraSensor, FlowHistory, and
Renderer.render's argument checks for the new tensors."""
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch = pytest.importorskip("torch")


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


def test_header_declares_the_entry_and_the_binding_matches():
    from shifu_amd import _lib
    hdr = _header()
    plain = re.search(r"\bint shf_render_cameras\(([^;]*?)\);", hdr, re.S).group(1)
    flow = re.search(r"\bint shf_render_cameras_flow\(([^;]*?)\);", hdr, re.S).group(1)
    names = lambda args: [a.split()[-1].lstrip("*") for a in args.split(",")]
    p, f = names(plain), names(flow)
    # every argument of shf_render_cameras in its place, then the new ones, the stream last
    assert f[:len(p) - 1] == p[:-1] and f[-1] == p[-1] == "stream"
    assert f[len(p) - 1:-1] == ["prev_body_pose", "prev_cam_pose", "prev_valid", "flow_or_null", "flow_i16_or_null"]
    assert len(_lib._SIGS["shf_render_cameras_flow"][0]) == len(f) == 18
    assert len(_lib._SIGS["shf_render_cameras"][0]) == len(p) == 13
    assert "shf_render_cameras_flow" in _lib.EXPORTS
    assert hasattr(_lib.lib(), "shf_render_cameras_flow")


def test_abi_version_is_unchanged_by_the_additive_entry():
    version = int(re.search(r"#define SHF_ABI_VERSION (\d+)", _header()).group(1))
    assert version == _abi.SHF_ABI_VERSION
    from shifu_amd import _lib
    assert _lib.lib().shf_abi_version() == version


def test_entry_checks_its_arguments_on_the_host():
    """No launch: every call here fails (or returns) before the kernel."""
    import ctypes as C
    from shifu_amd import _lib
    from shifu_amd.render import camera_struct
    L = _lib.lib()
    t = _abi.ShfTerrain()
    cam = camera_struct(32, 24, 60.0, 0.1, 5.0)
    one = C.c_void_p(16)                     # never dereferenced on these paths
    call = lambda scene=one, camera=cam, n=1, bs=one, prev=(one, one, one), flow=one, q=one: L.shf_render_cameras_flow(
        scene, C.byref(t), None, C.byref(camera), n, bs, one, one, one, None, None, None, prev[0], prev[1], prev[2], flow, q, None)
    err = lambda: L.shf_last_error().decode()
    assert call(scene=None) != 0 and "null scene" in err()
    assert call(camera=camera_struct(0, 24, 60.0, 0.1, 5.0)) != 0 and "width and height" in err()
    assert call(camera=camera_struct(32, 24, 180.0, 0.1, 5.0)) != 0 and "horizontal_fov" in err()
    assert call(camera=camera_struct(32, 24, 60.0, 1.0, 0.5)) != 0 and "near_plane" in err()
    assert call(n=-1) != 0 and "num_envs" in err()
    assert call(n=0) == 0
    assert call(bs=None) != 0 and "null input tensor" in err()
    for k in range(3):
        prev = [one, one, one]
        prev[k] = None
        assert call(prev=prev) != 0 and "prev_" in err()
    assert call(flow=C.c_void_p(20)) != 0 and "aligned" in err()
    # both flow outputs null: shf_render_cameras itself -- which returns at once with no output image
    assert call(flow=None, q=None, prev=(None, None, None)) == 0
    assert call(flow=None, q=None, camera=camera_struct(0, 24, 60.0, 0.1, 5.0)) != 0 and err().startswith("shf_render_cameras:")


def test_budgets_guard_the_flow_kernels_and_the_plain_ones_are_as_they_were():
    import json
    from shifu_amd import build
    build.build_native()
    res = json.load(open(build.RESOURCES))
    build.check_budgets(res)
    guarded = [p for p, _, _ in build.BUDGETS]
    assert "_Z21k_render_cameras_flow" in guarded and "_Z24k_render_cameras_tw_flow" in guarded
    for sym in ("_Z21k_render_cameras_flow", "_Z24k_render_cameras_tw_flow"):
        k = [v for n, v in res.items() if n.startswith(sym)]
        assert len(k) == 1 and k[0]["scratch"] == 0 and k[0]["spill"] == 0
    plain = [v for n, v in res.items() if n.startswith("_Z16k_render_cameras")][0]
    assert plain["vgprs"] == 68 and plain["scratch"] == 0          # the height-field kernel keeps its registers


# ---- the int16 encoding ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_flow_i16_rounding_saturation_and_round_trip(kind):
    from shifu_amd.render import flow_from_i16, flow_to_i16
    W, H = 64, 48
    wrap = (lambda a: torch.from_numpy(np.asarray(a, np.float32))) if kind == "torch" else (lambda a: np.asarray(a, np.float32))
    back = lambda a: a.numpy() if kind == "torch" else a
    # halves round to even: q = u 32768 / W, so u = k W / 65536 sits exactly on k / 2
    halves = np.array([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5], np.float64)
    f = np.stack([halves * W / 32768, halves * H / 32768], axis=-1)
    q = back(flow_to_i16(wrap(f), W, H))
    assert q.dtype == np.int16 and q.shape == (7, 2)
    np.testing.assert_array_equal(q[:, 0], [0, 2, 2, 4, 0, -2, -2])
    np.testing.assert_array_equal(q[:, 1], [0, 2, 2, 4, 0, -2, -2])
    # saturation at +-32768 / 32767
    edge = np.array([[W, H], [-W, -H], [2.0 * W, -3.0 * H], [W * 32767 / 32768, -H * 32767 / 32768], [1e9, -1e9]])
    np.testing.assert_array_equal(back(flow_to_i16(wrap(edge), W, H)),
                                  [[32767, 32767], [-32768, -32768], [32767, -32768], [32767, -32767], [32767, -32768]])
    # every integer comes back: to_i16(from_i16(q)) == q over the whole range, and +0 stays 0
    allq = np.stack([np.arange(-32768, 32768), np.arange(-32768, 32768)[::-1]], axis=-1).astype(np.int16)
    src = torch.from_numpy(allq) if kind == "torch" else allq
    px = flow_from_i16(src, W, H)
    assert back(px).dtype == np.float32
    np.testing.assert_array_equal(back(flow_to_i16(px, W, H)), allq)
    np.testing.assert_allclose(back(px)[:, 0], allq[:, 0].astype(np.float64) * W / 32768, rtol=1e-7)
    # a width that is no power of two: the kernel's float32 sequence (u x 32768 exact, one correctly rounded division)
    rng = np.random.default_rng(0)
    u = rng.uniform(-3, 3, (1000, 2)).astype(np.float32)
    want = np.rint((u * np.float32(32768)) / np.array([40, 24], np.float32)).astype(np.int16)
    np.testing.assert_array_equal(back(flow_to_i16(wrap(u), 40, 24)), want)


def test_normalize_optical_flow_returns_pixels():
    from shifu_amd.units import normalize_optical_flow
    q = np.array([[[16384, -8192]]], np.int16)
    np.testing.assert_array_equal(normalize_optical_flow(q, 128, 64), [[[64.0, -16.0]]])
    np.testing.assert_array_equal(normalize_optical_flow(torch.from_numpy(q), 128, 64).numpy(), [[[64.0, -16.0]]])


# ---- the opt-in ---------------------------------------------------------------------------------------------------------
def _facade_scene():
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.model import asset_path
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    arm = gym.load_asset(sim, os.path.dirname(asset_path("abb_rod.urdf")), "abb_rod.urdf", opts)
    env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
    gym.create_actor(env, arm, gymapi.Transform(), "arm", 0, 0)
    props = gymapi.CameraProperties()
    props.width, props.height = 32, 24
    cam = gym.create_camera_sensor(env, props)
    return gym, sim, env, cam


class _FakeEnv:
    device = "cpu"
    gym = sim = None


def _default_sensor():
    from shifu_amd.configs.sensor_config import CameraSensorConfig
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.units.sensors import CameraSensor

    class Cfg(CameraSensorConfig):
        name = "cam"
        local_lookat_positions = [[0.7, 0.0, 0.7], [0.0, 0.0, 0.1]]

    assert gymapi.IMAGE_OPTICAL_FLOW in Cfg.image_types          # the reference's default lists all four types
    return CameraSensor(Cfg())


def test_without_the_variable_the_refusals_are_as_before(monkeypatch):
    monkeypatch.delenv("SHIFU_AMD_OPTICAL_FLOW", raising=False)
    from shifu_amd.isaacgym import gymapi
    gym, sim, env, cam = _facade_scene()
    with pytest.raises(NotImplementedError, match="OPTICAL_FLOW"):
        gym.get_camera_image_gpu_tensor(sim, env, cam, gymapi.IMAGE_OPTICAL_FLOW)
    gym.invalidate_camera_flow(sim, cam)                          # accepted, nothing to do
    with pytest.raises(NotImplementedError, match="IMAGE_OPTICAL_FLOW is not rendered"):
        _default_sensor().set_env(_FakeEnv())
    monkeypatch.setenv("SHIFU_AMD_OPTICAL_FLOW", "0")
    with pytest.raises(NotImplementedError, match="IMAGE_OPTICAL_FLOW is not rendered"):
        _default_sensor().set_env(_FakeEnv())


def test_with_the_variable_the_default_image_types_are_accepted(monkeypatch):
    monkeypatch.setenv("SHIFU_AMD_OPTICAL_FLOW", "1")
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.units import sensors
    assert gymapi.Gym._optical_flow_enabled() and sensors.optical_flow_enabled()
    s = _default_sensor()
    s.set_env(_FakeEnv())                                         # _init_props: no refusal
    assert s._pose_type == sensors.CameraPose.LocalLookat
    # before prepare_sim there is no camera group yet: the usual error, not the refusal
    gym, sim, env, cam = _facade_scene()
    with pytest.raises(RuntimeError, match="no camera sensors"):
        gym.get_camera_image_gpu_tensor(sim, env, cam, gymapi.IMAGE_OPTICAL_FLOW)


# ---- FlowHistory and Renderer.render's checks (CPU tensors: nothing is launched) ------------------------------------
def test_flow_history_is_born_invalid_and_updates_in_place():
    from shifu_amd.render import FlowHistory
    h = FlowHistory(3, 2, "cpu")
    assert h.prev_body_pose.shape == (6, 7) and h.prev_cam_pose.shape == (3, 7) and h.prev_valid.dtype == torch.int32
    assert int(h.prev_valid.sum()) == 0
    ptrs = [t.data_ptr() for t in h.tensors().values()]
    bs, cp = torch.rand(6, 13), torch.rand(3, 7)
    h.update(bs, cp)
    assert torch.equal(h.prev_body_pose, bs[:, :7]) and torch.equal(h.prev_cam_pose, cp) and h.prev_valid.tolist() == [1, 1, 1]
    h.invalidate([1])
    assert h.prev_valid.tolist() == [1, 0, 1]
    h.invalidate(torch.tensor([0, 2]))
    assert h.prev_valid.tolist() == [0, 0, 0]
    h.update(bs, cp)
    h.invalidate()
    assert h.prev_valid.tolist() == [0, 0, 0]
    assert ptrs == [t.data_ptr() for t in h.tensors().values()]          # preallocated: never rebound


def test_render_rejects_wrong_flow_tensors_before_any_launch(monkeypatch):
    from shifu_amd import _lib, render

    class _NoLaunch:
        def __getattr__(self, name):
            raise AssertionError("the library was called: " + name)

    monkeypatch.setattr(_lib, "lib", lambda: _NoLaunch())
    r = object.__new__(render.Renderer)          # the checks need the scene's body count and the device only
    r.device, r.scene = torch.device("cpu"), _abi.ShfRenderScene()
    r.scene.num_bodies = 2
    cam = render.camera_struct(8, 6, 60.0, 0.1, 5.0)
    n, B, H, W = 3, 2, 6, 8
    good = dict(flow=torch.zeros(n, H, W, 2), flow_i16=torch.zeros(n, H, W, 2, dtype=torch.int16),
                prev_body_pose=torch.zeros(n * B, 7), prev_cam_pose=torch.zeros(n, 7),
                prev_valid=torch.zeros(n, dtype=torch.int32))
    base = (torch.zeros(n * B, 13), torch.zeros(n, 7), torch.zeros(n, B, dtype=torch.int32), torch.zeros(n, B, 3), cam)
    bad = dict(flow=[torch.zeros(n, H, W), torch.zeros(n, H, W, 2, dtype=torch.float64), torch.zeros(n, W, H, 2)],
               flow_i16=[torch.zeros(n, H, W, 2, dtype=torch.int32), torch.zeros(n, H, W, dtype=torch.int16)],
               prev_body_pose=[torch.zeros(n * B, 13), torch.zeros(n, B, 7), torch.zeros(n * B, 7, dtype=torch.float64),
                               torch.zeros(n * B, 13)[:, :7]],
               prev_cam_pose=[torch.zeros(n, 6), torch.zeros(n + 1, 7)],
               prev_valid=[torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.bool), torch.zeros(n, 1, dtype=torch.int32)])
    for key, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError, match="render: expected a contiguous"):
                r.render(*base, **dict(good, **{key: t}))
    for key in ("prev_body_pose", "prev_cam_pose", "prev_valid"):      # a flow output without its history
        with pytest.raises(ValueError, match="prev_body_pose, prev_cam_pose and prev_valid"):
            r.render(*base, **dict(good, **{key: None}))
    with pytest.raises(ValueError, match="prev_body_pose"):
        r.render(*base, flow_i16=good["flow_i16"])
