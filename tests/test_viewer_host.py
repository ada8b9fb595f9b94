"""The headless viewer without a GPU (shifu_amd/viewer.py, Renderer.render_world, the facade's viewer calls): the PNG and
APNG writers against a decoder written here, the ABI of the added entry, the grid layout, host-side validation, the
facade's opt-in, and the register budgets of the two new kernels."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

from shifu_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a small PNG reader: chunks with their CRCs checked, zlib, filter type 0 only ---------------------------------------
def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(data):
        n, = struct.unpack(">I", data[p:p + 4])
        kind, body = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        crc, = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xFFFFFFFF), f"bad CRC in {kind}"
        out.append((kind, body))
        p += 12 + n
    assert p == len(data)
    return out


def _unfilter0(raw, H, W, ch):
    rows = np.frombuffer(raw, np.uint8).reshape(H, 1 + W * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, ch)


def _decode_png(path):
    ch = _chunks(open(path, "rb").read())
    assert ch[0][0] == b"IHDR" and ch[-1] == (b"IEND", b"")
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and ctype in (2, 6)
    raw = zlib.decompress(b"".join(b for k, b in ch if k == b"IDAT"))
    return _unfilter0(raw, H, W, 3 if ctype == 2 else 4)


@pytest.mark.parametrize("shape", [(5, 7, 4), (1, 1, 3), (32, 48, 4), (3, 2, 3)])
def test_png_round_trip(tmp_path, shape):
    from shifu_amd.viewer import write_png
    img = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    p = tmp_path / "a.png"
    write_png(p, img)
    np.testing.assert_array_equal(_decode_png(p), img)


def test_png_round_trip_through_pil(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from shifu_amd.viewer import write_apng, write_png
    rng = np.random.default_rng(1)
    for ch in (3, 4):
        img = rng.integers(0, 256, (9, 13, ch), dtype=np.uint8)
        write_png(tmp_path / "b.png", img)
        np.testing.assert_array_equal(np.asarray(Image.open(tmp_path / "b.png")), img)
    frames = [rng.integers(0, 256, (6, 5, 4), dtype=np.uint8) for _ in range(3)]
    write_apng(tmp_path / "c.png", frames)
    im = Image.open(tmp_path / "c.png")
    assert getattr(im, "n_frames", 1) == 3
    for k, f in enumerate(frames):
        im.seek(k)
        np.testing.assert_array_equal(np.asarray(im.convert("RGBA")), f)


def test_png_writer_refuses_what_it_cannot_write(tmp_path):
    from shifu_amd.viewer import write_apng, write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 2), np.uint8), np.zeros((4, 4, 4), np.float32), np.zeros((0, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            write_png(tmp_path / "x.png", bad)
    with pytest.raises(ValueError):
        write_apng(tmp_path / "x.png", [])
    with pytest.raises(ValueError):
        write_apng(tmp_path / "x.png", [np.zeros((2, 2, 4), np.uint8), np.zeros((2, 3, 4), np.uint8)])


def test_apng_structure(tmp_path):
    from shifu_amd.viewer import write_apng
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (6, 10, 4), dtype=np.uint8) for _ in range(4)]
    p = tmp_path / "anim.png"
    write_apng(p, frames, fps=20.0)
    ch = _chunks(open(p, "rb").read())                       # (every CRC is checked there)
    kinds = [k for k, _ in ch]
    assert kinds == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * 3 + [b"IEND"]
    assert struct.unpack(">II", ch[1][1]) == (4, 0)          # four frames, looping forever
    seq, got = 0, []
    for k, body in ch[2:-1]:
        if k == b"fcTL":
            s, W, H, x, y, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", body)
            assert (s, W, H, x, y, dispose, blend) == (seq, 10, 6, 0, 0, 0, 0) and abs(num / den - 0.05) < 1e-9
            seq += 1
        elif k == b"fdAT":
            assert struct.unpack(">I", body[:4])[0] == seq
            seq += 1
            got.append(_unfilter0(zlib.decompress(body[4:]), 6, 10, 4))
        else:
            got.append(_unfilter0(zlib.decompress(body), 6, 10, 4))
    assert seq == 7
    for a, b in zip(got, frames):
        np.testing.assert_array_equal(a, b)


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_the_entry_is_declared_and_bound_without_a_new_abi_version():
    from shifu_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "shifu_amd.h")).read()
    assert re.search(r"\bint shf_render_world\s*\(", hdr)
    assert "shf_render_world" in _lib._SIGS and "shf_render_world" in _lib.EXPORTS
    assert len(_lib._SIGS["shf_render_world"][0]) == 19
    assert int(re.search(r"#define SHF_ABI_VERSION (\d+)", hdr).group(1)) == 22 == _abi.SHF_ABI_VERSION
    val = lambda name: int(re.search(r"#define SHF_RENDER_WORLD_" + name + r"\s+(\d+)", hdr).group(1))
    assert (val("LIST"), val("CHUNK")) == (_abi.RENDER_WORLD_LIST, _abi.RENDER_WORLD_CHUNK)
    assert _abi.RENDER_WORLD_LIST >= _abi.RENDER_WORLD_CHUNK >= _abi.RENDER_MAX_SHAPES


def test_the_entry_refuses_bad_arguments_on_the_host():
    """Through the library's error path, before any launch (no GPU is touched: every case fails a host check)."""
    import ctypes as C
    from shifu_amd import _lib
    from shifu_amd.render import camera_struct
    l = _lib.lib()
    t = _abi.ShfTerrain()
    t.hscale = t.vscale = 1.0
    cam = camera_struct(48, 32, 60.0, 0.1, 4.0)
    one = C.c_void_p(16)                                    # a non-null pointer that no host check dereferences
    call = lambda cam=cam, views=1, envs=1, drawn=1, bs=one, scene=one: l.shf_render_world(
        scene, C.byref(t), None, C.byref(cam), views, one, envs, drawn, None, None, C.c_float(0.0), bs, one, one, one, None, None,
        None, None)
    for kw, word in ((dict(views=0), b"at least 1"), (dict(envs=0), b"at least 1"), (dict(drawn=0), b"at least 1"),
                     (dict(drawn=-3), b"at least 1"), (dict(bs=None), b"null input"), (dict(scene=None), b"null scene"),
                     (dict(cam=camera_struct(0, 32, 60.0, 0.1, 4.0)), b"width"),
                     (dict(cam=camera_struct(16384, 16384, 60.0, 0.1, 4.0), views=4096), b"too many")):
        assert call(**kw) != 0
        assert word in l.shf_last_error(), (kw, l.shf_last_error())


# ---- layout and host-side validation -------------------------------------------------------------------------------------
def _host_viewer(**kw):
    from shifu_amd.viewer import Viewer
    kw.setdefault("source", lambda: None)
    num_envs = kw.pop("num_envs", 12)
    return Viewer(None, num_envs, None, None, None, 48, 32, **kw)


def test_grid_layout_offsets():
    from shifu_amd.viewer import grid_offsets
    off = grid_offsets(7, spacing=(2.0, 3.0), per_row=3)
    assert off.dtype == np.float32 and off.shape == (7, 3)
    for j in range(7):
        np.testing.assert_array_equal(off[j], [2.0 * (j % 3), 3.0 * (j // 3), 0.0])
    np.testing.assert_array_equal(grid_offsets(5, 1.5)[4], [1.5 * (4 % 3), 1.5 * (4 // 3), 0.0])     # per_row: ceil(sqrt(5)) = 3
    v = _host_viewer(env_ids=[5, 2, 9], layout="grid", spacing=2.0, per_row=2)
    np.testing.assert_array_equal(v.offsets, [[0, 0, 0], [2, 0, 0], [0, 2, 0]])                         # by list position
    np.testing.assert_array_equal(v.env_offset(9), [0, 2, 0])
    assert (_host_viewer(layout="world").offsets == 0).all()
    with pytest.raises(ValueError, match="not among"):
        v.env_offset(3)


def test_viewer_refuses_bad_env_ids_and_layouts():
    for bad in ([], [12], [-1, 3], [[1, 2]], [0.5]):
        with pytest.raises(ValueError, match="env_ids"):
            _host_viewer(env_ids=bad)
    with pytest.raises(ValueError, match="layout"):
        _host_viewer(layout="ring")
    with pytest.raises(ValueError):
        _host_viewer(num_envs=0)
    from shifu_amd.viewer import Viewer
    with pytest.raises(ValueError, match="source"):
        Viewer(None, 4, None, None, None, 48, 32)
    v = _host_viewer(env_ids=[3, 4])
    with pytest.raises(ValueError, match="not among"):
        v.follow(7)
    v.look_at([1.0, -1.0, 1.0], [0.0, 0.0, 0.0])
    from shifu_amd.render import camera_basis
    np.testing.assert_allclose(camera_basis(v._pose[3:])[0], np.array([-1, 1, -1]) / np.sqrt(3), atol=1e-12)


def test_frame_recorder_counts_on_the_host():
    from shifu_amd.viewer import FrameRecorder
    v = _host_viewer()
    with pytest.raises(ValueError):
        FrameRecorder(v, 0)
    rec = FrameRecorder(v, 2)
    with pytest.raises(RuntimeError, match="not drawn"):
        rec.record()
    rec.count = 2
    with pytest.raises(RuntimeError, match="frames are taken"):
        rec.record()


def test_render_world_validates_before_any_device_call(monkeypatch):
    torch = pytest.importorskip("torch")
    from shifu_amd import _lib, render
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("render_world reached the library"))
    r = object.__new__(render.Renderer)
    r.scene, r.device = _abi.ShfRenderScene(), torch.device("cpu")
    r.scene.num_bodies, r.scene.nshapes = 2, 1
    r.terrain, r._scene_dev, r._heights = _abi.ShfTerrain(), torch.zeros(1), None
    cam = render.camera_struct(48, 32, 60.0, 0.1, 4.0)
    n = 3
    good = dict(body_state=torch.zeros(n * 2, 13), view_pose=torch.zeros(1, 7), seg=torch.zeros(n, 2, dtype=torch.int32),
                color=torch.zeros(n, 2, 3), camera=cam, env_ids=torch.zeros(2, dtype=torch.int32), env_offset=torch.zeros(2, 3),
                depth=torch.zeros(1, 32, 48), seg_out=torch.zeros(1, 32, 48, dtype=torch.int32),
                rgba=torch.zeros(1, 32, 48, 4, dtype=torch.uint8), env_out=torch.zeros(1, 32, 48, dtype=torch.int32))
    bad = dict(body_state=torch.zeros(n * 2, 7), view_pose=torch.zeros(7), seg=torch.zeros(n, 2, dtype=torch.int64),
               color=torch.zeros(n, 2, 3, dtype=torch.float64), env_ids=torch.zeros(2, dtype=torch.int64),
               env_offset=torch.zeros(3, 3), depth=torch.zeros(1, 48, 32), seg_out=torch.zeros(1, 32, 48),
               rgba=torch.zeros(1, 32, 48, 3, dtype=torch.uint8), env_out=torch.zeros(2, 32, 48, dtype=torch.int32))
    for k, v in bad.items():
        with pytest.raises(ValueError):
            r.render_world(**{**good, k: v})
    with pytest.raises(ValueError):
        r.render_world(**{**good, "env_ids": torch.zeros(0, dtype=torch.int32), "env_offset": None})
    with pytest.raises(ValueError):
        r.render_world(**{**good, "rgba": torch.zeros(1, 32, 48, 8, dtype=torch.uint8)[..., ::2]})     # not contiguous
    with pytest.raises(ValueError):
        r.render_world(**{**good, "env_radius": float("nan")})


# ---- the facade's opt-in -------------------------------------------------------------------------------------------------
def _facade_scene(n=4, spacing=1.5, per_row=2):
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.model import asset_path
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    arm = gym.load_asset(sim, os.path.dirname(asset_path("abb_rod.urdf")), "abb_rod.urdf", opts)
    envs = []
    for e in range(n):
        env = gym.create_env(sim, gymapi.Vec3(-spacing, -spacing, -spacing), gymapi.Vec3(spacing, spacing, spacing), per_row)
        gym.create_actor(env, arm, gymapi.Transform(), "arm", e, 0)
        envs.append(env)
    return gym, sim, envs


def test_facade_viewer_calls_are_no_ops_by_default(monkeypatch, tmp_path):
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.isaacgym import gymapi
    monkeypatch.delenv("SHIFU_AMD_VIEWER", raising=False)
    gym, sim, envs = _facade_scene()
    assert gym.create_viewer(sim, gymapi.CameraProperties()) is None
    assert gym.viewer_camera_look_at(None, None, gymapi.Vec3(1, 1, 1), gymapi.Vec3(0, 0, 0)) is None
    assert gym.draw_viewer(None, sim, True) is None
    assert gym.write_viewer_image_to_file(None, str(tmp_path / "never.png")) is None
    assert gym.query_viewer_has_closed(None) is False
    # IsaacGymEnv.render(): no viewer, nothing written -- also with the variable set on an env that made none (headless)
    env = object.__new__(IsaacGymEnv)
    env.viewer, env.gym, env.sim = None, gym, sim
    monkeypatch.chdir(tmp_path)
    assert env.render() is None
    monkeypatch.setenv("SHIFU_AMD_VIEWER", str(tmp_path / "frames"))
    assert env.render() is None
    assert os.listdir(tmp_path) == []


def test_facade_viewer_opt_in_needs_no_gpu_before_the_first_draw(monkeypatch, tmp_path):
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.viewer import Viewer
    monkeypatch.setenv("SHIFU_AMD_VIEWER", str(tmp_path))
    gym, sim, envs = _facade_scene(n=4, spacing=1.5, per_row=2)
    props = gymapi.CameraProperties()
    props.width, props.height = 64, 40
    v = gym.create_viewer(sim, props)                        # before prepare_sim
    assert isinstance(v, Viewer) and sim.backend is None and v.images is None
    assert (v.width, v.height, v.layout) == (64, 40, "grid")
    np.testing.assert_array_equal(v.offsets, [[0, 0, 0], [3, 0, 0], [0, 3, 0], [3, 3, 0]])      # create_env's grid: pitch 3, 2 per row
    assert gym.query_viewer_has_closed(v) is False
    # look_at relative to an env: its grid offset is added to both points
    gym.viewer_camera_look_at(v, envs[3], gymapi.Vec3(1.0, 0.0, 1.0), gymapi.Vec3(0.0, 0.0, 0.0))
    np.testing.assert_allclose(v._pose[:3], [4.0, 3.0, 1.0])
    gym.viewer_camera_look_at(v, None, gymapi.Vec3(1.0, 0.0, 1.0), gymapi.Vec3(0.0, 0.0, 0.0))
    np.testing.assert_allclose(v._pose[:3], [1.0, 0.0, 1.0])
    # a spacing of 0 (TerrainGymEnv): the envs are where their states say
    gym2, sim2, _ = _facade_scene(n=2, spacing=0.0)
    assert gym2.create_viewer(sim2, props).layout == "world"


def test_facade_viewer_refuses_a_warped_trimesh_as_the_cameras_do(monkeypatch, tmp_path):
    from shifu_amd.gym.a1_fused import default_terrain_cfg
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.utils.terrain import Terrain
    monkeypatch.setenv("SHIFU_AMD_VIEWER", str(tmp_path))
    monkeypatch.delenv("SHIFU_AMD_TRIMESH_CAMERAS", raising=False)
    cfg = default_terrain_cfg(mesh_type="trimesh", num_rows=1, num_cols=2, border_size=1)
    np.random.seed(3)
    ter = Terrain(cfg, 4)
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    p = gymapi.TriangleMeshParams()
    p.nb_vertices, p.nb_triangles = ter.vertices.shape[0], ter.triangles.shape[0]
    p.transform.p.x = p.transform.p.y = -cfg.border_size
    gym.add_triangle_mesh(sim, ter.vertices.flatten(order="C"), ter.triangles.flatten(order="C"), p)
    gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
    with pytest.raises(NotImplementedError, match="warped trimesh"):
        gym.create_viewer(sim, gymapi.CameraProperties())
    monkeypatch.setenv("SHIFU_AMD_TRIMESH_CAMERAS", "1")
    assert gym.create_viewer(sim, gymapi.CameraProperties()) is not None


# ---- the model's bounding radius and the budgets ----------------------------------------------------------------------------
def test_a1_env_radius_bounds_the_robot():
    from shifu_amd.model import asset_path, compile_urdf
    from shifu_amd.viewer import model_env_radius
    cm = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT)
    r = model_env_radius(cm)
    assert 0.45 < r < 1.2          # trunk half-diagonal 0.15 + hip, thigh and calf offsets (~0.5 m of leg) + a foot; not a blanket bound


def test_budgets_name_both_world_kernels_without_scratch():
    from shifu_amd import build
    got = {p: (v, s) for p, v, s in build.BUDGETS if "k_render_world" in p}
    assert set(got) == {"_Z14k_render_world", "_Z17k_render_world_tw"}
    assert all(s == 0 and 0 < v <= 256 for v, s in got.values())
    assert not any(p.startswith(q) for p in got for q in ("_Z16k_render_cameras", "_Z19k_render_cameras_tw"))
    import json
    build.build_native()
    res = json.load(open(build.RESOURCES))
    for prefix in got:
        k = [v for n, v in res.items() if n.startswith(prefix)]
        assert len(k) == 1 and k[0]["scratch"] == 0 and k[0]["spill"] == 0


# ---- recorded frames ---------------------------------------------------------------------------------------------------------
def test_recorded_frames_read_back():
    """tests/golden/world_view_frame_*.png: frames 0, 30 and 59 that tools/play_a1.py --video wrote on the GPU (FrameRecorder.save
    -> write_png, 640 x 360) -- files of real size from the writer, read by the decoder above.  What must hold of any such
    frame: opaque; mostly terrain, whose grey (0.5, 0.5, 0.5) shades to r = g = b; and the followed robot, colored (0.95,
    0.45, 0.1), whose shaded pixels keep r : g = 2.11 whatever the light (up to the rounding to u8)."""
    frames = [_decode_png(os.path.join(ROOT, "tests", "golden", "world_view_frame_%03d.png" % k)) for k in (0, 30, 59)]
    for f in frames:
        assert f.shape == (360, 640, 4) and (f[..., 3] == 255).all()
        r, g, b = (f[..., k].astype(float) for k in range(3))
        assert ((r == g) & (g == b)).mean() > 0.5
        orange = (r > 60) & (np.abs(r / np.maximum(g, 1) - 0.95 / 0.45) < 0.15) & (b < 0.5 * g)
        assert orange.sum() > 30
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
