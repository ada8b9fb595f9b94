"""Cameras on the fused envs (shifu_amd/gym/fused_camera.py): the A1 on its trimesh terrain against the float64 brute
force, the ABB push-box camera against the gym facade's bit for bit, the fused regressor straight from a fused-env
camera, and the facade's opt-in for trimesh terrains (SHIFU_AMD_TRIMESH_CAMERAS=1)."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import trimesh_render_ref as tr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


def _compose(body_row, lp, lq):
    """body pose o (lp, lq) in float64: what an attached camera's pose has to be."""
    from tests import render_ref as rr
    from shifu_amd.render import mat_to_quat
    R = rr.qmat(body_row[3:7])
    return np.asarray(body_row[:3], float) + R @ lp, mat_to_quat(R @ rr.qmat(lq))


def test_a1_on_its_trimesh_terrain_against_the_brute_force():
    """A trunk-mounted camera looking 0.5 rad down on the terrain the A1 task runs on, after reset() and after 5 steps:
    legs, feet and the warped mesh (its risers included) as the brute force over the env's own body states sees them.
    Body row 0 against root_state, measured: position and velocity columns differ by 0; the quaternion columns by up to
    5.96e-8 (one float32 rounding of a component near 1), which is why those four take 2 ulp and not bitwise equality."""
    _need_gpu()
    from shifu_amd.gym.a1_fused import FusedA1Env, default_terrain_cfg
    from tests import render_ref as rr
    n, W, H, FOV, NEAR, FAR = 4, 32, 24, 87.0, 0.05, 3.0
    env = FusedA1Env(num_envs=n, terrain="trimesh",
                     terrain_cfg=default_terrain_cfg(mesh_type="trimesh", num_rows=1, num_cols=1, border_size=1, terrain_length=6.,
                                                     terrain_width=6.))
    assert env.sim.terrain.warped == 1
    nb = env.cm.blob.nb
    assert tuple(env.cam_seg.shape) == (n, nb) and env.cam_seg.dtype == torch.int32 and int(env.cam_seg.abs().sum()) == 0
    assert tuple(env.cam_color.shape) == (n, nb, 3) and bool((env.cam_color == 0.8).all())          # the facade's defaults
    rng = np.random.default_rng(2)
    env.cam_seg.copy_(torch.from_numpy(rng.permutation(n * nb).reshape(n, nb).astype(np.int32) + 1))
    env.cam_color.copy_(torch.from_numpy(rng.uniform(0.2, 1.0, (n, nb, 3)).astype(np.float32)))
    lp, lq = np.array([0.25, 0.0, 0.05]), np.array([0.0, np.sin(0.25), 0.0, np.cos(0.25)])      # pitched 0.5 rad down
    cam = env.add_camera(W, H, FOV, NEAR, FAR, position=lp, quat=lq, attach_body=0)
    ct = env.cfg_terrain
    tri = env.terrain.vertices.astype(np.float64)[env.terrain.triangles.astype(np.int64)]
    tri[..., :2] -= ct.border_size

    def check(tag):
        im = cam.render()
        torch.cuda.synchronize()
        assert im is cam.raw_images()
        bs = env.body_state.view(n, nb, 13).cpu().numpy().astype(np.float64)
        # body row 0 is the root of the same instant: position and velocities bit for bit; the quaternion is stored after one
        # more normalisation than root_state's, which may move each component by a float32 rounding (2 ulp of 1 allowed)
        root, row0 = env.root_state.view(n, 13).cpu().numpy(), env.body_state.view(n, nb, 13)[:, 0].cpu().numpy()
        print(f"{tag}: body row 0 - root_state, largest per column:", np.abs(row0.astype(np.float64) - root).max(0))
        np.testing.assert_array_equal(row0[:, :3], root[:, :3])
        np.testing.assert_array_equal(row0[:, 7:], root[:, 7:])
        np.testing.assert_allclose(row0[:, 3:7], root[:, 3:7], rtol=0, atol=2 * 2.0 ** -23)
        pose = cam.world_pose().cpu().numpy().astype(np.float64)
        depth, seg, rgba = (-im["depth"]).cpu().numpy(), im["seg"].cpu().numpy(), im["rgba"].cpu().numpy()
        segs, cols = env.cam_seg.cpu().numpy(), env.cam_color.cpu().numpy()
        bad = masked = body_px = terrain_px = riser_px = 0
        for e in range(n):
            p, q = _compose(bs[e, 0], lp, lq)
            assert np.abs(pose[e, :3] - p).max() < 1e-5 and min(np.abs(pose[e, 3:] - q).max(), np.abs(pose[e, 3:] + q).max()) < 1e-5
            near_tri = tr.visible_triangles(tri, pose[e, :3], pose[e, 3:], W, H, FOV, FAR)
            ref, amb = tr.render(tr.world_shapes(env.cm.render_shapes, bs[e], segs[e], cols[e]), near_tri, pose[e, :3], pose[e, 3:],
                                 W, H, FOV, NEAR, FAR)
            b, m = tr.compare(depth[e], seg[e], rgba[e], ref, amb, extra_mask=rr.silhouette_adjacent(ref[1]))
            bad, masked = bad + b, masked + m
            body_px, terrain_px = body_px + int((ref[1] > 0).sum()), terrain_px + int((ref[1] == 0).sum())
            riser_px += int(tr.triangle_classes(near_tri)[1][ref[3][ref[1] == 0]].sum())
        print(f"{tag}: {bad} mismatching, {masked} ambiguous of {n * W * H} pixels; {body_px} on the robot, {terrain_px} on the "
              f"terrain, {riser_px} of those on risers")
        assert terrain_px > 0.3 * n * W * H
        assert masked <= 0.005 * n * W * H and bad <= 0.005 * n * W * H
        return im["depth"].clone()

    env.reset()
    d0 = check("after reset")
    g = torch.Generator().manual_seed(7)
    for _ in range(5):
        env.step((2 * torch.rand(n, env.num_actions, generator=g) - 1).to(env.device))
    d1 = check("after 5 steps")
    assert not torch.equal(d0, d1)
    sd = env.state_dict()
    assert set(sd) == {"format", "kind", "num_envs", "env_id_offset", "step_index", "common_step_counter", "sim", "task",
                       "sim_params", "kernel_form"}                   # images are derived data: not part of the state
    env.destroy()


def test_abb_push_box_camera_equals_the_facade_bitwise():
    """FusedAbbEnv with the push-box camera (128 x 128, fov 42, from (0.7, 0, 0.7) at (0, 0, 0.1)) and the example's ids and
    colors, against the gym facade's CameraSensor on the same state tensors."""
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from tests import test_gpu_camera as tc
    n = 4
    hook = tc._vision_env(n)
    hook.reset()
    fused = FusedAbbEnv(num_envs=n, seed=5, link_contacts=True, solver="tgs")
    cam = fused.add_camera(128, 128, 42, 0.1, 3, position=(0.7, 0.0, 0.7), target=(0.0, 0.0, 0.1))
    fused.reset()
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        fused.step((2 * torch.rand(n, 3, generator=g) - 1).to(fused.device))
    sim = hook.isg_env.sim
    be = sim.backend
    B = fused.cm.blob.nb + len(fused.boxes)
    assert tuple(sim.cam_seg.shape) == tuple(fused.cam_seg.shape) == (n, B)
    # the example's ids and colors: robot, table, cube and goal as the units set them through the facade
    ids = {int(v) for v in sim.cam_seg.unique().cpu()}
    assert {hook.robot.segmentation_id, hook.cube.segmentation_id} <= ids and len(ids) >= 3
    fused.cam_seg.copy_(sim.cam_seg)
    fused.cam_color.copy_(sim.cam_color)
    for tid in (_abi.T_DOF_STATE, _abi.T_ROOT_STATE, _abi.T_BODY_STATE):
        be.tensors[tid].copy_(fused.sim.tensors[tid])
    sim.body_fresh = True                                         # the body states just copied in are the ones to draw
    assert torch.equal(sim.camera_groups[hook.camera.camera_handle]["pose"], cam.pose)
    hook.camera.render_images()
    cam.render()
    torch.cuda.synchronize()
    a, b = hook.camera.raw_images(), cam.raw_images()
    assert set(a) == set(b) == {"rgba", "depth", "seg"}
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype
        assert torch.equal(a[k], b[k]), k
    seg = b["seg"]
    assert int((seg == hook.cube.segmentation_id).sum()) > 0 and int((seg == hook.robot.segmentation_id).sum()) > 0
    hook.destroy()
    fused.destroy()


def test_fused_regressor_from_a_fused_env_camera():
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from tests import test_gpu_vision as tv
    env = FusedAbbEnv(num_envs=4, seed=3)
    cam = env.add_camera(128, 128, 42, 0.1, 3, position=(0.7, 0.0, 0.7), target=(0.0, 0.0, 0.1))
    env.reset()
    im = cam.render()
    assert bool(torch.isfinite(im["depth"]).all())                # the push-box view is closed: table and ground everywhere
    m = tv._to_device(tv._seeded_full_model()).enable_fused_inference()
    want = {k: v.clone() for k, v in m({'rgb': torch.div(im["rgba"][..., :3], 255.0).permute(0, 3, 1, 2),
                                        'depth': torch.neg(im["depth"]).unsqueeze(1)}).items()}
    got = m.fused.from_camera(cam)
    for k in tv.KEYS:
        assert torch.equal(want[k], got[k]), k
    assert float(want["obj_pos"].std()) > 0
    env.destroy()


def _trimesh_sim(gym):
    from shifu_amd.gym.a1_fused import default_terrain_cfg
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.utils.terrain import Terrain
    cfg = default_terrain_cfg(mesh_type="trimesh", num_rows=1, num_cols=1, border_size=1, terrain_length=6., terrain_width=6.)
    np.random.seed(3)
    ter = Terrain(cfg, 2)
    sp = gymapi.SimParams()
    sp.up_axis, sp.gravity = gymapi.UP_AXIS_Z, gymapi.Vec3(0, 0, -9.81)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    p = gymapi.TriangleMeshParams()
    p.nb_vertices, p.nb_triangles = ter.vertices.shape[0], ter.triangles.shape[0]
    p.transform.p.x = p.transform.p.y = -cfg.border_size
    gym.add_triangle_mesh(sim, ter.vertices.flatten(order="C"), ter.triangles.flatten(order="C"), p)
    assert sim.terrain[6] is not None and sim.terrain[6].any()
    return sim


def test_facade_renders_a_trimesh_terrain_when_asked(monkeypatch):
    _need_gpu()
    import os
    from shifu_amd.isaacgym import gymapi
    from shifu_amd.model import asset_path
    from shifu_amd.render import Renderer, build_scene
    gym = gymapi.acquire_gym()
    monkeypatch.delenv("SHIFU_AMD_TRIMESH_CAMERAS", raising=False)
    sim = _trimesh_sim(gym)
    env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
    with pytest.raises(NotImplementedError, match="warped trimesh.*SHIFU_AMD_TRIMESH_CAMERAS=1"):
        gym.create_camera_sensor(env, gymapi.CameraProperties())
    monkeypatch.setenv("SHIFU_AMD_TRIMESH_CAMERAS", "1")
    sim = _trimesh_sim(gym)
    a1 = gym.load_asset(sim, os.path.dirname(asset_path("a1.urdf")), "a1.urdf", gymapi.AssetOptions())
    props = gymapi.CameraProperties()
    props.width, props.height, props.horizontal_fov, props.near_plane, props.far_plane = 48, 32, 70.0, 0.05, 6.0
    envs = []
    for e in range(2):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        gym.create_actor(env, a1, gymapi.Transform(gymapi.Vec3(2.0 + e, 2.0, 0.6)), "a1", e, 0)
        c = gym.create_camera_sensor(env, props)
        gym.set_camera_location(c, env, gymapi.Vec3(0.8 + e, 0.9, 1.4), gymapi.Vec3(2.0 + e, 2.0, 0.3))
        envs.append(env)
    gym.prepare_sim(sim)
    gym.simulate(sim)
    gym.render_all_camera_sensors(sim)
    be, g = sim.backend, sim.camera_groups[0]
    assert be.terrain.warped == 1
    model = envs[0].actors[0].asset.model
    r = Renderer(build_scene(model.render_shapes, model.blob.nb, height_samples=be.height_samples, vscale=be.terrain.vscale),
                 be.terrain, be._heights, be.device)
    depth, seg, rgba = torch.empty_like(g["depth"]), torch.empty_like(g["seg"]), torch.empty_like(g["rgba"])
    r.render(be.tensors[_abi.T_BODY_STATE], g["pose"], sim.cam_seg, sim.cam_color, g["camera"], depth=depth, seg_out=seg, rgba=rgba)
    torch.cuda.synchronize()
    assert torch.equal(depth, g["depth"]) and torch.equal(seg, g["seg"]) and torch.equal(rgba, g["rgba"])
    assert float(torch.isfinite(depth).float().mean()) > 0.5      # the terrain fills most of the view
    gym.destroy_sim(sim)
