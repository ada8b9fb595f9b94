"""Camera sensors without a GPU: the facade's bookkeeping, the render-shape export of the model compiler (which must
change nothing the step kernels read), the pixel-ray convention, the view / projection matrices against the reference's
own get_pixel_position, and the refusal of a warped trimesh terrain."""
import hashlib
import os
import sys

import numpy as np
import pytest

from shifu_amd import _abi

REF = "/root/reference"


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


# ---- the compiled model: render shapes exported, nothing else changed ------------------------------------------------
# digests of bytes(model.blob) / bytes(model.hulls) as compiled before camera sensors existed
A1_BLOB = "6920f8654695cdfa708293771feedcf14401e85fc04d631416632c9578c26e7f"
A1_FACADE_BLOB = "1d3032df323d1d7ba7d13da47ab9a565b92f78f10c365b9db5d7d7c76754824a"
ABB_HULL_BLOB = "2c91817bf2cf75c1734d6cbeb240c681be0a1bd05f30f3dc153dc94c1dacfe6e"
ABB_HULL_SET = "4ab03627cd6a43c7f819ba746615a0785cbf077c584fddddbf1252333efa3e30"
ABB_FACADE_BLOB = "0bfaef5e4146a9dbc4ade7a1585a4fa9c81c9ba9a8233bb65ab40971824937d0"


def test_render_export_leaves_the_compiled_models_unchanged():
    from shifu_amd.abb_task import ROD_CAPSULE, abb_link_boxes, abb_model
    from shifu_amd.model import asset_path, compile_urdf
    a1 = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT)
    assert _sha(a1.blob) == A1_BLOB
    assert _sha(compile_urdf(asset_path("a1.urdf"), link_contacts=True, meshes="auto").blob) == A1_FACADE_BLOB
    abb = abb_model(link_contacts=True, link_shapes="hull")
    assert _sha(abb.blob) == ABB_HULL_BLOB and _sha(abb.hulls) == ABB_HULL_SET
    facade = compile_urdf(asset_path("abb_rod.urdf"), extra_spheres=ROD_CAPSULE, extra_boxes=abb_link_boxes(), link_contacts=True,
                          fix_base_link=True, disable_gravity=True, meshes="auto")
    assert _sha(facade.blob) == ABB_FACADE_BLOB


def test_a1_render_shapes_are_its_collision_shapes():
    """Every <collision> primitive of a1.urdf, in its reported body's frame: the box corners / sphere centres the compiler
    turns into contact points are exactly the shapes' own."""
    from shifu_amd.model import asset_path, compile_urdf
    cm = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT)
    rs = cm.render_shapes
    assert len(rs) > 0 and {s.kind for s in rs} <= {"box", "sphere", "capsule"}
    pts = {(int(cm.blob.pt_body[i]), tuple(np.round(np.array(cm.blob.pt_pos[i][:]), 4))) for i in range(cm.blob.np)}
    for s in rs:
        assert 0 <= s.body < cm.blob.nb
        if s.kind == "sphere":
            assert (s.body, tuple(np.round(s.pos, 4))) in pts
        elif s.kind == "box":
            h = 0.5 * np.asarray(s.size)
            for sx in (-1, 1):
                for sy in (-1, 1):
                    for sz in (-1, 1):
                        corner = s.pos + s.rot @ (h * [sx, sy, sz])
                        assert (s.body, tuple(np.round(corner, 4))) in pts


def test_abb_render_shapes_are_the_narrow_phase_hulls():
    """abb_rod.urdf with its link hulls: each mesh collider is exported as the polytope the convex narrow phase collides
    (CompiledModel.hulls: same planes once placed in the body frame), plus the rod capsules."""
    from shifu_amd.abb_task import abb_model
    cm = abb_model(link_contacts=True, link_shapes="hull")
    polys = [s for s in cm.render_shapes if s.kind == "hull"]
    assert len(polys) == cm.hulls.nhull == 7
    caps = [s for s in cm.render_shapes if s.kind == "capsule"]
    assert any(abs(s.size[0] - 0.0194) < 1e-9 for s in caps)          # ROD_CAPSULE
    recs = sorted(((s.body, s) for s in polys), key=lambda t: t[0])
    for j, (b, s) in enumerate(recs):
        h = cm.hulls.hull[j]
        assert h.body == b and h.nf == len(s.poly["planes"])
        for f, pl in enumerate(s.poly["planes"]):
            nw = s.rot @ pl[:3]
            np.testing.assert_allclose(np.array(h.plane[f][:3]), nw, atol=1e-6)
            np.testing.assert_allclose(h.plane[f][3], pl[3] + nw @ s.pos, atol=1e-5)


def test_build_scene_layout():
    from shifu_amd.abb_task import abb_model
    from shifu_amd.render import build_scene
    cm = abb_model(link_contacts=True, link_shapes="hull")
    sc = build_scene(cm.render_shapes, cm.blob.nb, [(0.6, 0.6, 0.1), (0.05, 0.05, 0.05)])
    assert sc.nshapes == len(cm.render_shapes) + 2 and sc.npolys == 7 and sc.num_bodies == cm.blob.nb + 2
    assert sc.shape[sc.nshapes - 1].body == cm.blob.nb + 1 and sc.shape[sc.nshapes - 1].kind == _abi.RENDER_BOX
    for k in range(sc.nshapes):
        s = sc.shape[k]
        if s.kind == _abi.RENDER_POLY:
            P = sc.poly[s.poly]
            # re-centred: the shape origin lies inside the polytope, the bounding radius holds every face's support
            assert all(P.plane[f][3] > 0 for f in range(P.nf))
    with pytest.raises(ValueError, match="SHF_RENDER_MAX_SHAPES"):
        build_scene(cm.render_shapes, cm.blob.nb, [(0.1, 0.1, 0.1)] * 64)


# ---- conventions -------------------------------------------------------------------------------------------------------
def test_pixel_rays_closed_forms():
    from shifu_amd.render import camera_basis, lookat_quat, pixel_rays
    q = lookat_quat([0.7, 0.0, 0.7], [0.0, 0.0, 0.1])
    fwd, right, up = camera_basis(q)
    np.testing.assert_allclose(fwd, np.array([-0.7, 0, -0.6]) / np.hypot(0.7, 0.6), atol=1e-12)
    np.testing.assert_allclose(right, [0, 1, 0], atol=1e-12)        # looking towards -x with +z up: the image's right is world +y
    assert up[2] > 0 and abs(up @ fwd) < 1e-12
    W, H, fov = 8, 6, 60.0
    d = pixel_rays(q, W, H, fov)
    t = np.tan(np.radians(30))
    assert d.shape == (H, W, 3)
    np.testing.assert_allclose(d @ fwd, 1.0, atol=1e-12)             # the ray parameter is the view depth
    # pixel (r, c) centre: x = 2 (c + 1/2) / W - 1, y = 1 - 2 (r + 1/2) / H
    for r, c in ((0, 0), (H - 1, W - 1), (2, 5)):
        x, y = 2 * (c + 0.5) / W - 1, 1 - 2 * (r + 0.5) / H
        np.testing.assert_allclose(d[r, c] @ right, x * t, atol=1e-12)
        np.testing.assert_allclose(d[r, c] @ up, y * t * H / W, atol=1e-12)
    # the outermost columns' edges are at +-hfov / 2
    edge = fwd + right * t
    assert abs(np.degrees(np.arccos(edge @ fwd / np.linalg.norm(edge))) - 30.0) < 1e-9
    # an identity transform looks along +x with +z up
    f0, r0, u0 = camera_basis([0, 0, 0, 1])
    np.testing.assert_allclose(np.stack([f0, r0, u0]), [[1, 0, 0], [0, -1, 0], [0, 0, 1]])


def test_view_and_proj_matrices_project_onto_the_ray_pixel():
    """[p, 1] @ view @ proj / w gives NDC (x, y) = the pixel-ray coordinates of p; proj[0,0] = 1/t, proj[1,1] = W/(H t)."""
    from shifu_amd.render import lookat_quat, pixel_rays, proj_matrix, view_matrix
    pos, W, H, fov, near, far = np.array([0.7, 0.0, 0.7]), 128, 96, 42.0, 0.1, 3.0
    q = lookat_quat(pos, [0.0, 0.0, 0.1])
    V, P = view_matrix(pos, q), proj_matrix(W, H, fov, near, far)
    t = np.tan(np.radians(21))
    assert abs(P[0, 0] - 1 / t) < 1e-12 and abs(P[1, 1] - P[0, 0] * W / H) < 1e-12
    d = pixel_rays(q, W, H, fov)
    for r, c, s in ((0, 0, 0.5), (50, 77, 1.3), (H - 1, W - 1, 2.9)):
        p = pos + s * d[r, c]
        clip = np.append(p, 1.0) @ V @ P
        ndc = clip[:2] / clip[3]
        np.testing.assert_allclose(ndc, [2 * (c + 0.5) / W - 1, 1 - 2 * (r + 0.5) / H], atol=1e-9)
        assert abs(clip[3] - s) < 1e-9                               # w = view depth
        z = clip[2] / clip[3]
        assert -1 - 1e-9 <= z <= 1 + 1e-9


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "shifu", "utils")), reason="reference tree not present")
def test_reference_get_pixel_position_lands_on_the_ray_pixel():
    """The reference's own get_pixel_position (shifu/utils/camera.py) with the facade's matrices names the pixel whose
    ray the convention casts through each random point of the frustum."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_ref_camera", os.path.join(REF, "shifu", "utils", "camera.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from shifu_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
    props = gymapi.CameraProperties()
    props.width, props.height, props.horizontal_fov, props.near_plane, props.far_plane = 128, 96, 42.0, 0.1, 3.0
    cam = gym.create_camera_sensor(env, props)
    pos = np.array([0.7, 0.0, 0.7])
    gym.set_camera_location(cam, env, gymapi.Vec3(*pos), gymapi.Vec3(0.0, 0.0, 0.1))
    V = np.matrix(gym.get_camera_view_matrix(sim, env, cam)).astype(np.float64)
    P = np.matrix(gym.get_camera_proj_matrix(sim, env, cam)).astype(np.float64)
    from shifu_amd.render import pixel_rays
    q = env.cameras[cam].quat
    d = pixel_rays(q, 128, 96, 42.0)
    rng = np.random.default_rng(0)
    for _ in range(200):
        r, c = int(rng.integers(0, 96)), int(rng.integers(0, 128))
        # a point on pixel (r, c)'s footprint, away from its borders (float32 matrices), at a random depth
        u, v = rng.uniform(-0.3, 0.3, 2)
        x, y = 2 * (c + 0.5 + u) / 128 - 1, 1 - 2 * (r + 0.5 + v) / 96
        from shifu_amd.render import camera_basis
        f, rt, up = camera_basis(q)
        t = np.tan(np.radians(21))
        s = rng.uniform(0.1, 3.0)
        p = pos + s * (f + rt * x * t + up * y * t * 96 / 128)
        px = mod.get_pixel_position(p, V, P, 128, 96)
        assert (int(px[0]), int(px[1])) == (c, r)
        # and the pixel's own ray passes through the point's pixel centre
        pc = pos + s * d[r, c]
        assert tuple(int(k) for k in mod.get_pixel_position(pc, V, P, 128, 96)) == (c, r)


def test_lookat_pose_of_the_push_box_camera():
    from shifu_amd.render import camera_basis, lookat_quat
    q = lookat_quat([0.7, 0.0, 0.7], [0.0, 0.0, 0.1])
    assert abs(np.linalg.norm(q) - 1) < 1e-12
    f, r, u = camera_basis(q)
    np.testing.assert_allclose(np.cross(r, u), -f, atol=1e-12)       # right-handed view frame (x right, y up, z back)
    straight_down = lookat_quat([0, 0, 2], [0, 0, 0])
    f, r, u = camera_basis(straight_down)
    np.testing.assert_allclose(f, [0, 0, -1], atol=1e-12)
    assert abs(r @ u) < 1e-12 and abs(np.linalg.norm(r) - 1) < 1e-12


# ---- facade bookkeeping ------------------------------------------------------------------------------------------------
def _facade_scene(n=3):
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.model import asset_path
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    plane = gymapi.PlaneParams()
    gym.add_ground(sim, plane)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    arm = gym.load_asset(sim, os.path.dirname(asset_path("abb_rod.urdf")), "abb_rod.urdf", opts)
    box = gym.create_box(sim, 0.05, 0.05, 0.05)
    envs = []
    for e in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        a = gym.create_actor(env, arm, gymapi.Transform(), "arm", e, 0)
        b = gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.3, 0, 0.025)), "box", e, 0)
        envs.append((env, a, b))
    return gym, sim, envs, arm


def test_facade_camera_bookkeeping():
    from shifu_amd.isaacgym import gymapi
    gym, sim, envs, arm = _facade_scene()
    props = gymapi.CameraProperties()
    props.width, props.height = 32, 24
    with pytest.warns(UserWarning, match="collision geometry"):
        gymapi.Gym._warned_visual = False
        cams = [gym.create_camera_sensor(env, props) for env, _, _ in envs]
    assert cams == [0, 0, 0]
    env0, a0, b0 = envs[0]
    gym.set_camera_location(0, env0, gymapi.Vec3(1, 0, 1), gymapi.Vec3(0, 0, 0))
    c = env0.cameras[0]
    np.testing.assert_allclose(c.pos, [1, 0, 1])
    from shifu_amd.render import camera_basis
    np.testing.assert_allclose(camera_basis(c.quat)[0], np.array([-1, 0, -1]) / np.sqrt(2), atol=1e-12)
    tr = gymapi.Transform(gymapi.Vec3(0.1, 0.2, 0.3), gymapi.Quat(0, 0, 0.7071068, 0.7071068))
    gym.set_camera_transform(0, envs[1][0], tr)
    np.testing.assert_allclose(envs[1][0].cameras[0].pos, [0.1, 0.2, 0.3])
    np.testing.assert_allclose(np.linalg.norm(envs[1][0].cameras[0].quat), 1.0)
    gym.attach_camera_to_body(0, envs[2][0], 3, tr, gymapi.FOLLOW_TRANSFORM)
    assert envs[2][0].cameras[0].attach[0] == 3
    with pytest.raises(NotImplementedError, match="FOLLOW_TRANSFORM"):
        gym.attach_camera_to_body(0, envs[2][0], 3, tr, gymapi.FOLLOW_POSITION)
    # segmentation ids and colors, per env, actor and body
    gym.set_rigid_body_segmentation_id(env0, a0, 2, 7)
    gym.set_rigid_body_segmentation_id(envs[1][0], b0, 0, 9)
    gym.set_rigid_body_color(env0, b0, 0, gymapi.MESH_VISUAL, gymapi.Vec3(1.0, 0.0, 0.25))
    assert gym.get_rigid_body_segmentation_id(env0, a0, 2) == 7
    assert gym.get_rigid_body_segmentation_id(envs[1][0], a0, 2) == 0
    assert gym.get_rigid_body_segmentation_id(envs[1][0], b0, 0) == 9
    assert tuple(gym.get_rigid_body_color(env0, b0, 0)) == (1.0, 0.0, 0.25)
    # matrices: row-vector view of the pose, projection of the properties
    V = gym.get_camera_view_matrix(sim, env0, 0)
    P = gym.get_camera_proj_matrix(sim, env0, 0)
    assert V.shape == P.shape == (4, 4)
    np.testing.assert_allclose(np.append([1.0, 0.0, 1.0], 1.0) @ V, [0, 0, 0, 1], atol=1e-6)   # the camera sits at the origin
    np.testing.assert_allclose(P[0, 0], 1 / np.tan(np.radians(45)), rtol=1e-6)
    np.testing.assert_allclose(P[1, 1], P[0, 0] * 32 / 24, rtol=1e-6)
    with pytest.raises(NotImplementedError, match="OPTICAL_FLOW"):
        gym.get_camera_image_gpu_tensor(sim, env0, 0, gymapi.IMAGE_OPTICAL_FLOW)


def test_camera_on_a_warped_trimesh_raises():
    from shifu_amd.gym.a1_fused import default_terrain_cfg
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.utils.terrain import Terrain
    cfg = default_terrain_cfg(mesh_type="trimesh", num_rows=1, num_cols=2, border_size=1)
    np.random.seed(3)
    ter = Terrain(cfg, 4)
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    p = gymapi.TriangleMeshParams()
    p.nb_vertices, p.nb_triangles = ter.vertices.shape[0], ter.triangles.shape[0]
    p.transform.p.x = p.transform.p.y = -cfg.border_size
    gym.add_triangle_mesh(sim, ter.vertices.flatten(order="C"), ter.triangles.flatten(order="C"), p)
    assert sim.terrain[0] == "heightfield" and sim.terrain[6] is not None and sim.terrain[6].any()
    env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
    with pytest.raises(NotImplementedError, match="warped trimesh"):
        gym.create_camera_sensor(env, gymapi.CameraProperties())


def test_camera_sensor_is_exported_under_compat():
    from shifu_amd import compat
    compat.install()
    import importlib
    units = importlib.import_module("shifu.units")
    from shifu_amd.units.sensors import CameraSensor
    assert units.CameraSensor is CameraSensor


def test_camera_struct_layout_matches_the_header(tmp_path):
    import ctypes
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "shifu_amd.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n",'
                   'sizeof(ShfRenderShape),sizeof(ShfRenderPoly),sizeof(ShfRenderScene),sizeof(ShfCamera),'
                   'offsetof(ShfRenderScene, shape),offsetof(ShfRenderScene, poly));}')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [ctypes.sizeof(_abi.ShfRenderShape), ctypes.sizeof(_abi.ShfRenderPoly), ctypes.sizeof(_abi.ShfRenderScene),
            ctypes.sizeof(_abi.ShfCamera), _abi.ShfRenderScene.shape.offset, _abi.ShfRenderScene.poly.offset]
    assert got == want


def test_render_constants_mirror_the_header():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "shifu_amd.h")).read()
    val = lambda name: float(re.search(r"#define SHF_RENDER_" + name + r"\s+([0-9.]+)f?", hdr).group(1))
    assert (val("AMBIENT"), val("DIFFUSE")) == (_abi.RENDER_AMBIENT, _abi.RENDER_DIFFUSE)
    assert (val("LIGHT_X"), val("LIGHT_Y"), val("LIGHT_Z")) == _abi.RENDER_LIGHT
    assert (val("BG_R"), val("BG_G"), val("BG_B")) == _abi.RENDER_BG
    assert int(val("MAX_SHAPES")) == _abi.RENDER_MAX_SHAPES and int(val("MAX_POLYS")) == _abi.RENDER_MAX_POLYS
    np.testing.assert_allclose(np.linalg.norm(_abi.RENDER_LIGHT), 1.0, atol=1e-7)
    sys.modules.pop("tests.render_ref", None)
    from tests import render_ref
    assert render_ref.AMBIENT == _abi.RENDER_AMBIENT and tuple(render_ref.BACKGROUND) == _abi.RENDER_BG
    np.testing.assert_allclose(render_ref.LIGHT, _abi.RENDER_LIGHT, atol=1e-7)


def test_kernel_has_no_scratch():
    """-Rpass-analysis=kernel-resource-usage of the build: the ray caster keeps its state in registers."""
    import json
    from shifu_amd import build
    build.build_native()
    res = json.load(open(build.RESOURCES))
    k = [v for n, v in res.items() if n.startswith("_Z16k_render_cameras")]
    assert len(k) == 1 and k[0]["scratch"] == 0 and k[0]["spill"] == 0
