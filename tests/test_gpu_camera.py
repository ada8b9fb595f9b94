"""Camera sensors on the GPU (csrc/shf_render.hip via shifu_amd/render.py, the gym facade and CameraSensor): known
answers, every shape kind and a height field against the independent float64 caster tests/render_ref.py, batch
independence, and the vision stage's camera on the ABB push-box hook env -- eager and replayed from hipGraphs."""
import numpy as np
import pytest

from shifu_amd import _abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, FOV = 48, 32, 60.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _shape_defs(rng):
    """One shape of each kind, each on a body of its own (body k), in its body frame (identity: the body pose places it)."""
    from shifu_amd.model import RenderShape, reduce_hull
    pts = rng.normal(size=(40, 3)) * [0.12, 0.08, 0.1]
    poly = reduce_hull(pts)
    return [RenderShape(0, "box", np.zeros(3), np.eye(3), np.array([0.3, 0.2, 0.12])),
            RenderShape(1, "sphere", np.zeros(3), np.eye(3), np.array([0.13])),
            RenderShape(2, "capsule", np.zeros(3), np.eye(3), np.array([0.07, 0.3])),
            RenderShape(3, "hull", np.zeros(3), np.eye(3), np.zeros(3), poly)]


def _ref_shapes(defs, poses, seg, col):
    """render_ref shape dicts of one env: body k's pose (pos, quat) applied to shape k."""
    from tests import render_ref as rr
    out = []
    for s, (p, q), sid, c in zip(defs, poses, seg, col):
        Rb = rr.qmat(q)
        d = dict(kind={"hull": "poly"}.get(s.kind, s.kind), pos=np.asarray(p, float) + Rb @ s.pos, rot=Rb @ s.rot, seg=int(sid),
                 color=np.asarray(c, float))
        if s.kind == "box":
            d["half"] = 0.5 * s.size
        elif s.kind == "sphere":
            d["r"] = s.size[0]
        elif s.kind == "capsule":
            d["r"], d["hl"] = s.size[0], 0.5 * s.size[1]
        else:
            d["planes"] = s.poly["planes"]
        out.append(d)
    return out


def _heightfield():
    """A Terrain-generated height field (the A1 task's generator: a rough pyramid slope at difficulty 0.8), 26 x 26 samples
    of a sub-terrain's corner (its centre is a flat platform) placed around the origin."""
    from shifu_amd.gym.a1_fused import default_terrain_cfg
    from shifu_amd.utils.terrain import Terrain
    cfg = default_terrain_cfg(num_rows=1, num_cols=1, border_size=0, terrain_length=6., terrain_width=6.)
    np.random.seed(11)
    ter = Terrain(cfg, 1)
    hs = np.ascontiguousarray(ter.make_terrain(0.15, 0.8).height_field_raw[0:26, 0:26]).astype(np.int16)
    t = _abi.ShfTerrain()
    t.rows, t.cols = hs.shape
    t.hscale, t.vscale, t.border = 0.1, 0.005, 1.25
    return t, hs


def _render(defs, poses, cams, seg, col, terrain=None, heights=None, nb=None, ground=True, near=0.1, far=4.0,
            depth_negative=False, W_=W, H_=H, fov=FOV):
    from shifu_amd.render import Renderer, build_scene, camera_struct
    n = len(cams)
    nb = len(defs) if nb is None else nb
    sc = build_scene(defs, nb, ground=ground, height_samples=heights, vscale=terrain.vscale if terrain is not None else 1.0)
    r = Renderer(sc, terrain, heights, "cuda:0")
    bs = torch.zeros(n * nb, 13)
    for e in range(n):
        for k, (p, q) in enumerate(poses[e]):
            bs[e * nb + k, :3] = torch.tensor(p)
            bs[e * nb + k, 3:7] = torch.tensor(q)
    cam = torch.tensor(np.array([np.concatenate([p, q]) for p, q in cams]), dtype=torch.float32)
    dev = torch.device("cuda:0")
    depth = torch.empty(n, H_, W_, device=dev)
    segi = torch.empty(n, H_, W_, dtype=torch.int32, device=dev)
    rgba = torch.empty(n, H_, W_, 4, dtype=torch.uint8, device=dev)
    r.render(bs.to(dev), cam.to(dev), torch.as_tensor(np.asarray(seg), dtype=torch.int32).to(dev).contiguous(),
             torch.as_tensor(np.asarray(col), dtype=torch.float32).to(dev).contiguous(),
             camera_struct(W_, H_, fov, near, far, depth_negative), depth=depth, seg_out=segi, rgba=rgba)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), segi.cpu().numpy(), rgba.cpu().numpy()


def _compare(depth, seg, rgba, ref):
    """Kernel images against render_ref: ids (hit flag + segmentation) equal except next to a reference silhouette
    (<= 0.5 % of the pixels), depth within 1e-4 m where they agree, RGB within 1 LSB where they agree away from the
    reference's facet edges (a ray that grazes the edge between two flat faces or height-field triangles may take either
    face's normal: same depth, another shade).  At grazing incidence the float32 entry depth is ill-conditioned: there the
    depth bound widens by 1e-6 s / cos(incidence), the float32 rounding of s amplified by the incidence."""
    from tests import render_ref as rr
    rd, rid, rrgb, rfacet, rcos = ref
    got_id = np.where(np.isfinite(depth), seg, -1)
    bad = got_id != rid
    edge = rr.silhouette_adjacent(rid)
    assert not (bad & ~edge).any(), f"{int((bad & ~edge).sum())} id mismatches away from silhouettes"
    assert bad.mean() <= 0.005, f"{bad.mean():.4f} of the pixels differ"
    ok = ~bad & np.isfinite(rd)
    tol = 1e-4 + 1e-6 * rd[ok] / np.maximum(rcos[ok], 1e-6)
    assert (np.abs(depth[ok] - rd[ok]) <= tol).all(), f"depth off by {np.abs(depth[ok] - rd[ok]).max():.3g} m"
    assert (np.abs(depth[ok] - rd[ok]) > 1e-4).mean() <= 0.001
    diff = np.abs(rgba[..., :3].astype(int) - rrgb.astype(int)).max(-1)
    shade_ok = ~bad & ~rr.silhouette_adjacent(rfacet)
    assert diff[shade_ok].max(initial=0) <= 1, f"RGB off by {diff[shade_ok].max()} LSB"
    assert (diff[~bad] > 1).mean() <= 0.002
    assert (rgba[..., 3] == 255).all()
    return int(bad.sum())


# ---- known answers ----------------------------------------------------------------------------------------------------
def test_plane_seen_from_above_has_depth_h_everywhere():
    _need_gpu()
    from shifu_amd.render import lookat_quat
    hts = [0.5, 1.0, 2.5]
    cams = [(np.array([0.3, -0.2, h]), lookat_quat([0.3, -0.2, h], [0.3, -0.2, 0.0])) for h in hts]
    # one body row per env, no shapes: the plane alone
    depth, seg, rgba = _render([], [[(np.zeros(3), np.array([0, 0, 0, 1.0]))] for _ in cams], cams, np.zeros((3, 1)),
                               np.zeros((3, 1, 3)), nb=1, far=10.0)
    for e, h in enumerate(hts):
        np.testing.assert_allclose(depth[e], h, rtol=1e-6)
    assert (seg == 0).all()
    from shifu_amd.render import DEFAULT_GROUND_COLOR, shade
    np.testing.assert_array_equal(rgba[..., :3], np.broadcast_to(shade(DEFAULT_GROUND_COLOR, [0, 0, 1]), rgba[..., :3].shape))


def test_sphere_silhouette_radius_matches_the_closed_form():
    _need_gpu()
    from shifu_amd.model import RenderShape
    from shifu_amd.render import lookat_quat, pixel_rays
    r, D = 0.2, 1.5
    defs = [RenderShape(0, "sphere", np.zeros(3), np.eye(3), np.array([r]))]
    pos = np.array([-D, 0.0, 1.0])
    q = lookat_quat(pos, [0.0, 0.0, 1.0])
    depth, seg, _ = _render(defs, [[(np.array([0.0, 0.0, 1.0]), np.array([0, 0, 0, 1.0]))]], [(pos, q)], [[7]], [[[1, 0, 0]]],
                            ground=False, W_=96, H_=96)
    d = pixel_rays(q, 96, 96, FOV)
    ang = np.arccos((d @ (np.array([D, 0, 0]) / D)) / np.linalg.norm(d, axis=-1))
    alpha = np.arcsin(r / D)                                    # the silhouette's angular radius
    inside, outside = ang < alpha - 1e-4, ang > alpha + 1e-4
    assert (seg[0][inside] == 7).all() and (seg[0][outside] == 0).all() and inside.sum() > 100
    assert np.isinf(depth[0][outside]).all()
    # the centre pixel's depth: D - r along the axis (the four central rays are off-axis by half a pixel)
    c = depth[0][47:49, 47:49]
    assert np.all(np.abs(c - (D - r)) < 2e-3)


def test_near_and_far_clipping():
    """Shapes entered before `near` or beyond `far` are not drawn (also one that straddles the near plane)."""
    _need_gpu()
    from shifu_amd.model import RenderShape
    from shifu_amd.render import lookat_quat
    pos = np.array([0.0, 0.0, 1.0])
    q = lookat_quat(pos, [1.0, 0.0, 1.0])
    defs = [RenderShape(0, "sphere", np.zeros(3), np.eye(3), np.array([0.05]))]
    ident = np.array([0, 0, 0, 1.0])
    n, far = 4, 2.0
    near = 0.5
    centres = [0.3, 0.52, 1.0, 2.03]         # wholly before near / straddling near / inside / beyond far (entry 1.98 < far!)
    cams = [(pos, q)] * n
    poses = [[(np.array([x, 0.0, 1.0]), ident)] for x in centres]
    depth, seg, _ = _render(defs, poses, cams, [[5]] * n, [[[1, 1, 1]]] * n, ground=False, near=near, far=far)
    from tests import render_ref as rr
    mid = (H // 2, W // 2)                                # (its ray is half a pixel off the sphere's centre)
    want = lambda x: rr.render([dict(kind="sphere", pos=[x, 0, 1], rot=np.eye(3), r=0.05, seg=5, color=[1, 1, 1])],
                               pos, q, W, H, FOV, 1e-3, 10.0)[0][mid]
    assert seg[0][mid] == 0 and seg[1][mid] == 0          # entered before near: not drawn
    assert seg[2][mid] == 5 and abs(depth[2][mid] - want(1.0)) < 1e-5
    assert seg[3][mid] == 5 and abs(depth[3][mid] - want(2.03)) < 1e-5 and want(2.03) < far     # entered before far: drawn
    poses[3] = [(np.array([2.06, 0.0, 1.0]), ident)]
    depth, seg, _ = _render(defs, poses, cams, [[5]] * n, [[[1, 1, 1]]] * n, ground=False, near=near, far=far,
                            depth_negative=True)
    assert seg[3][mid] == 0 and depth[3][mid] == -np.inf                # entered at 2.01 > far; negated depth: -inf


# ---- against the float64 reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["box", "sphere", "capsule", "hull"])
def test_each_shape_kind_against_the_reference(kind):
    _need_gpu()
    from tests import render_ref as rr
    from shifu_amd.render import lookat_quat
    rng = np.random.default_rng({"box": 1, "sphere": 2, "capsule": 3, "hull": 4}[kind])
    defs = [s for s in _shape_defs(rng) if s.kind == kind]
    defs[0].body = 0
    n = 16
    poses, cams, seg, col = [], [], [], []
    for e in range(n):
        poses.append([(rng.uniform([-0.2, -0.2, 0.2], [0.2, 0.2, 0.5]), _rand_quat(rng))])
        p = np.array([-1.0, 0.0, 0.6]) + rng.uniform(-0.2, 0.2, 3)
        cams.append((p, lookat_quat(p, rng.uniform(-0.1, 0.1, 3) + [0, 0, 0.3])))
        seg.append([3 + e])
        col.append([rng.uniform(0, 1, 3)])
    depth, sg, rgba = _render(defs, poses, cams, seg, col)
    for e in range(n):
        ref = rr.render(_ref_shapes(defs, poses[e], seg[e], col[e]), cams[e][0], cams[e][1], W, H, FOV, 0.1, 4.0, ground="plane",
                        facets=True)
        assert (ref[1] == 3 + e).sum() > 20                   # the shape is in view
        _compare(depth[e], sg[e], rgba[e], ref)


def _mixed_scene(n, seed=7):
    from shifu_amd.render import lookat_quat
    rng = np.random.default_rng(seed)
    defs = _shape_defs(rng)
    poses, cams, seg, col = [], [], [], []
    for e in range(n):
        poses.append([(rng.uniform([-0.5, -0.5, 0.1], [0.5, 0.5, 0.6]), _rand_quat(rng)) for _ in defs])
        p = np.array([-1.4, 0.0, 1.0]) + rng.uniform(-0.3, 0.3, 3)
        cams.append((p, lookat_quat(p, rng.uniform(-0.2, 0.2, 3))))
        seg.append(list(rng.choice(np.arange(1, 100), len(defs), replace=False)))
        col.append(rng.uniform(0, 1, (len(defs), 3)))
    return defs, poses, cams, seg, col


def test_all_shapes_on_a_height_field_against_the_reference():
    _need_gpu()
    from tests import render_ref as rr
    n = 64
    defs, poses, cams, seg, col = _mixed_scene(n)
    t, hs = _heightfield()
    assert hs.max() > hs.min()                                # a non-flat field
    depth, sg, rgba = _render(defs, poses, cams, seg, col, terrain=t, heights=hs)
    bad = 0
    for e in range(n):
        ref = rr.render(_ref_shapes(defs, poses[e], seg[e], col[e]), cams[e][0], cams[e][1], W, H, FOV, 0.1, 4.0,
                        ground=(hs, t.hscale, t.vscale, t.border), facets=True)
        bad += _compare(depth[e], sg[e], rgba[e], ref)
    assert bad <= 0.005 * n * W * H


def test_batch_independence():
    """Envs permuted or rendered as a subset give bitwise the same per-env images."""
    _need_gpu()
    n = 24
    defs, poses, cams, seg, col = _mixed_scene(n, seed=9)
    t, hs = _heightfield()
    full = _render(defs, poses, cams, seg, col, terrain=t, heights=hs)
    perm = np.random.default_rng(0).permutation(n)
    pick = lambda xs, idx: [xs[i] for i in idx]
    permuted = _render(defs, pick(poses, perm), pick(cams, perm), pick(seg, perm), pick(col, perm), terrain=t, heights=hs)
    sub = [3, 17, 5]
    subset = _render(defs, pick(poses, sub), pick(cams, sub), pick(seg, sub), pick(col, sub), terrain=t, heights=hs)
    for a, b, c in zip(full, permuted, subset):
        np.testing.assert_array_equal(a[perm], b)
        np.testing.assert_array_equal(a[sub], c)


def test_facade_images_background_is_minus_inf():
    """Through the gym facade: zero-copy per-env image views; IMAGE_DEPTH is minus the view depth, -inf where nothing is hit;
    the box actor shows its segmentation id and color."""
    _need_gpu()
    from shifu_amd.isaacgym import gymapi, gymtorch
    from shifu_amd.model import asset_path
    import os
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.up_axis, sp.gravity = gymapi.UP_AXIS_Z, gymapi.Vec3(0, 0, -9.81)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    pl = gymapi.PlaneParams()
    pl.normal = gymapi.Vec3(0, 0, 1)
    gym.add_ground(sim, pl)
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    arm = gym.load_asset(sim, os.path.dirname(asset_path("abb_rod.urdf")), "abb_rod.urdf", opts)
    box = gym.create_box(sim, 0.2, 0.2, 0.2, gymapi.AssetOptions())
    props = gymapi.CameraProperties()
    props.width, props.height, props.horizontal_fov, props.near_plane, props.far_plane = 64, 48, 60.0, 0.05, 5.0
    envs = []
    for e in range(3):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        gym.create_actor(env, arm, gymapi.Transform(gymapi.Vec3(-0.5, 3.0, 0)), "arm", e, 0)     # out of the view
        b = gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.6, 0.0, 0.1)), "box", e, 0)
        gym.set_rigid_body_segmentation_id(env, b, 0, 40 + e)
        gym.set_rigid_body_color(env, b, 0, gymapi.MESH_VISUAL, gymapi.Vec3(1.0, 0.0, 0.0))
        c = gym.create_camera_sensor(env, props)
        gym.set_camera_location(c, env, gymapi.Vec3(1.5, 0.0, 0.1), gymapi.Vec3(0.0, 0.0, 0.1))   # horizontal: sky above
        envs.append(env)
    gym.prepare_sim(sim)
    gym.simulate(sim)
    gym.render_all_camera_sensors(sim)
    torch.cuda.synchronize()
    for e, env in enumerate(envs):
        d = gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, env, 0, gymapi.IMAGE_DEPTH)).cpu().numpy()
        s = gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, env, 0, gymapi.IMAGE_SEGMENTATION)).cpu().numpy()
        c = gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, env, 0, gymapi.IMAGE_COLOR)).cpu().numpy()
        assert d.shape == (48, 64) and s.dtype == np.int32 and c.shape == (48, 64, 4) and c.dtype == np.uint8
        assert (d[0] == -np.inf).all() and (s[0] == 0).all()                       # top row: sky
        assert tuple(c[0, 0, :3]) == _abi.RENDER_BG
        assert s[24, 32] == 40 + e and abs(-d[24, 32] - 0.8) < 1e-4              # the box's face at x = 0.7
        assert c[24, 32, 0] > 0 and c[24, 32, 1] == 0 and c[24, 32, 2] == 0
        assert (d[-1] < 0).all() and np.isfinite(d[-1]).all()                      # bottom row: the ground
    view = gym.get_camera_image_gpu_tensor(sim, envs[1], 0, gymapi.IMAGE_DEPTH).tensor
    assert view.data_ptr() == sim.camera_groups[0]["depth"][1].data_ptr()          # zero-copy row of the group tensor
    gym.destroy_sim(sim)


# ---- the vision stage's camera on the ABB push-box hook env -------------------------------------------------------------
def _vision_env(n):
    from shifu_amd import compat
    compat.install()
    from shifu.configs import CameraSensorConfig
    from shifu.units import CameraSensor
    from isaacgym import gymapi as ga
    from examples.abb_pushbox_vision.a_prior_stage import AbbPushBox, AbbRobot, GoalBox, RandPosBox
    from examples.abb_pushbox_vision.task_config import (AbbRobotConfig, GoalBoxConfig, PriorStageEnvConfig, PushBoxConfig,
                                                         TableConfig)
    from shifu_amd.gym import ShifuVecEnv
    from shifu_amd.units import Box

    class PushBoxCameraConfig(CameraSensorConfig):          # the reference's task_config.py:124-145
        name = 'rgbd_camera'
        local_lookat_positions = [[0.7, 0., 0.7], [0., 0., 0.1]]
        image_types = [ga.IMAGE_COLOR, ga.IMAGE_DEPTH, ga.IMAGE_SEGMENTATION]
        image_normalization = True

        class camera_props(CameraSensorConfig.camera_props):
            enable_tensors = True
            use_collision_geometry = False
            width = 128
            height = 128
            horizontal_fov = 42
            near_plane = 0.1
            far_plane = 3

    class AbbPushBoxVision(AbbPushBox):
        def __init__(self, cfg):
            ShifuVecEnv.__init__(self, cfg)
            self.robot = AbbRobot(AbbRobotConfig())
            self.table = Box(TableConfig())
            self.cube = RandPosBox(PushBoxConfig())
            self.goal = GoalBox(GoalBoxConfig())
            self.camera = CameraSensor(PushBoxCameraConfig())
            self.isg_env.create_envs(robot=self.robot, objects=[self.table, self.cube, self.goal], sensors=[self.camera])
            self.success_buf = torch.zeros(self.num_envs, device=self.device, dtype=torch.float)

    cfg = PriorStageEnvConfig()
    cfg.num_envs = n
    return AbbPushBoxVision(cfg)


def _box_pixel_checks(env):
    import importlib
    from tests import render_ref as rr
    cam = env.camera
    n = env.num_envs
    assert cam.color_buf.shape == (n, 128, 128, 3) and cam.color_buf.dtype == torch.float32
    assert cam.depth_buf.shape == (n, 128, 128) and cam.depth_buf.dtype == torch.float32
    assert cam.segmentation_buf.shape == (n, 128, 128) and cam.segmentation_buf.dtype == torch.int32
    assert float(cam.color_buf.min()) >= 0.0 and float(cam.color_buf.max()) <= 1.0
    V, P = np.asarray(cam.view_matrix, float), np.asarray(cam.proj_matrix, float)
    cube = env.cube.base_pose.cpu().numpy()
    seg = cam.segmentation_buf.cpu().numpy()
    depth = cam.depth_buf.cpu().numpy()
    sid = env.cube.segmentation_id
    pos = np.array([0.7, 0.0, 0.7])
    from shifu_amd.render import lookat_quat
    q = lookat_quat(pos, [0.0, 0.0, 0.1])
    shown = 0
    for e in range(n):
        clip = np.append(cube[e, :3], 1.0) @ V @ P
        ndc = np.clip(clip / clip[3], -1, 1)
        px, py = int((ndc[0] + 1) * 128 / 2), int((1 - ndc[1]) * 128 / 2)
        # the view-space depth of the surface the pixel's ray enters: one ray against the cube's box, in float64
        box = dict(kind="box", pos=cube[e, :3], rot=rr.qmat(cube[e, 3:7]), half=[0.025] * 3, seg=sid, color=[1, 1, 1])
        rd, _, _ = rr.render([box], pos, q, 128, 128, 42.0, 0.1, 3.0)
        if seg[e, py, px] != sid:
            # the arm hangs over the cube in this env: then it is the arm that is seen there, in front of the cube
            assert seg[e, py, px] == env.robot.segmentation_id and depth[e, py, px] < rd[py, px], (e, seg[e, py, px])
            continue
        shown += 1
        assert abs(depth[e, py, px] - rd[py, px]) < 0.01
        assert abs(depth[e, py, px] - clip[3]) < 0.05                   # and near the centre's own view depth
    assert shown >= 0.5 * n, f"the cube's centre pixel shows the cube in {shown} of {n} envs"


def test_camera_sensor_on_the_push_box_env():
    _need_gpu()
    torch.manual_seed(0)
    env = _vision_env(48)
    env.reset()
    g = torch.Generator().manual_seed(3)
    for _ in range(4):
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    torch.cuda.synchronize()
    _box_pixel_checks(env)
    env.destroy()


def test_refresh_issues_one_render_launch_per_sensor(monkeypatch):
    _need_gpu()
    from shifu_amd import render
    env = _vision_env(8)
    env.reset()
    calls = []
    orig = render.Renderer.render
    monkeypatch.setattr(render.Renderer, "render", lambda self, *a, **k: (calls.append(1), orig(self, *a, **k))[1])
    env.isg_env.refresh_sensors()
    assert len(calls) == 1
    env.step(torch.zeros(env.num_envs, env.num_actions, device=env.device))
    assert len(calls) == 2
    env.destroy()


def test_graph_hooks_render_the_same_images_as_eager():
    """With enable_graph_hooks the render launch is replayed from the second hipGraph; its images equal an eager render of
    the same state, bit for bit, and the sensor checks hold on them."""
    _need_gpu()
    torch.manual_seed(1)
    env = _vision_env(32)
    env.reset()
    env.enable_graph_hooks()
    assert env._hook_graphs is not None
    g = torch.Generator().manual_seed(4)
    for _ in range(5):
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    torch.cuda.synchronize()
    cam = env.camera
    replayed = [cam.color_buf.clone(), cam.depth_buf.clone(), cam.segmentation_buf.clone()]
    cam.color_buf.zero_(); cam.depth_buf.zero_(); cam.segmentation_buf.zero_()
    for im in env.isg_env.gym.camera_group_tensors(env.isg_env.sim, cam.camera_handle).values():
        im.zero_()
    env.isg_env.refresh_sensors()                 # eager: render + refresh on the same state
    torch.cuda.synchronize()
    for a, b in zip(replayed, [cam.color_buf, cam.depth_buf, cam.segmentation_buf]):
        assert torch.equal(a, b)
    _box_pixel_checks(env)
    env.destroy()
