"""Optical-flow images on the GPU (csrc/shf_render.hip, k_render_cameras_flow / k_render_cameras_tw_flow, through
shifu_amd/render.py, the fused envs, the gym facade and CameraSensor): the same cast as the plain kernels bit for bit, the
exact-zero rules, the float64 checker tests/flow_ref.py, the int16 encoding, batch independence, FusedAbbEnv's device-side
validity and the SHIFU_AMD_OPTICAL_FLOW opt-in."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import flow_ref as fr
from tests import test_gpu_camera as tc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, FOV, NEAR, FAR = 40, 24, 60.0, 0.1, 4.0          # 2.5 x 1.5 tiles: partial tiles in both directions

# |flow_gpu - flow_ref| over the pixels where both casters show the same thing, in pixels.  Measured on the MI355X on
# checked_scene() (N = 3, 40 x 24, box / sphere / capsule / hull on the height field, every body and the camera moved by
# <= 0.05 m and <= 0.1 rad): FLOW_ERR_MEASURED is the maximum; the bound asserted is 3 x that, the margin for seed-to-seed
# variation of the float32 rounding (the depth error of <= 1e-4 m feeds the parallax term).  At most 0.1 % of the agreeing
# pixels may exceed it, as for the depth comparison of tests/test_gpu_camera.py; at most 0.5 % of the pixels may disagree.
# Measured: max 1.25e-05 px (99.9th percentile 8.8e-06, mean 2.1e-06; 0 of 2880 pixels disagree) on flows of up to 5.7 px --
# a few float32 roundings of a pixel coordinate of ~20 (ulp 1.9e-06).  FusedAbbEnv's scene (test 6) under the same bound:
# max 2.9e-05 px, 0 of 5376 pixels disagree.  The sliding-camera wall of test 2: 9.5e-07 px.
FLOW_ERR_MEASURED = 1.25e-05
FLOW_TOL = 3.0 * FLOW_ERR_MEASURED


def _f32(a):
    """The float32 value the kernel gets, as float64 for the checker."""
    return np.asarray(a, np.float32).astype(np.float64)


def _round_poses(poses):
    return [[(_f32(p), _f32(q)) for p, q in env] for env in poses]


def _perturb(rng, p, q, dmax=0.05, amax=0.1):
    """(p, q) moved by a random rigid motion of <= dmax metres and <= amax radians."""
    from shifu_amd.render import mat_to_quat
    from tests import render_ref as rr
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.3, 1.0) * amax
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rd = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    step = rng.normal(size=3)
    step *= rng.uniform(0.3, 1.0) * dmax / np.linalg.norm(step)
    return np.asarray(p, float) + step, mat_to_quat(Rd @ rr.qmat(q))


class _Scene:
    """One Renderer and its inputs on the device; flow() / plain() launch on them and return numpy images."""

    def __init__(self, defs, poses, cams, seg, col, terrain=None, heights=None, warp=None, ground=True, nb=None,
                 W_=W, H_=H, fov=FOV, near=NEAR, far=FAR):
        from shifu_amd.render import Renderer, build_scene, camera_struct
        self.n, self.nb = len(cams), (len(defs) if nb is None else nb)
        self.W, self.H = W_, H_
        sc = build_scene(defs, self.nb, ground=ground, height_samples=heights, vscale=terrain.vscale if terrain is not None else 1.0)
        self.r = Renderer(sc, terrain, heights, "cuda:0", warp=warp)
        self.dev = torch.device("cuda:0")
        self.camera = camera_struct(W_, H_, fov, near, far, False)
        self.bs, self.cam = self._body_state(poses), self._cam(cams)
        self.seg = torch.as_tensor(np.asarray(seg), dtype=torch.int32).to(self.dev).contiguous()
        self.col = torch.as_tensor(np.asarray(col), dtype=torch.float32).to(self.dev).contiguous()

    def _body_state(self, poses, width=13):
        bs = torch.zeros(self.n * self.nb, width)
        bs[:, 6] = 1.0
        for e in range(self.n):
            for k, (p, q) in enumerate(poses[e]):
                bs[e * self.nb + k, :3] = torch.tensor(np.asarray(p, np.float32))
                bs[e * self.nb + k, 3:7] = torch.tensor(np.asarray(q, np.float32))
        return bs.to(self.dev)

    def _cam(self, cams):
        return torch.tensor(np.array([np.concatenate([p, q]) for p, q in cams]), dtype=torch.float32).to(self.dev)

    def _images(self):
        n, H_, W_, dev = self.n, self.H, self.W, self.dev
        return dict(depth=torch.full((n, H_, W_), 7.0, device=dev), seg_out=torch.full((n, H_, W_), 7, dtype=torch.int32, device=dev),
                    rgba=torch.full((n, H_, W_, 4), 7, dtype=torch.uint8, device=dev))

    def plain(self):
        im = self._images()
        self.r.render(self.bs, self.cam, self.seg, self.col, self.camera, **im)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in im.items()}

    def flow(self, prev_poses, prev_cams, valid):
        """prev_poses / prev_cams: None = bit-equal to the current ones."""
        im = self._images()
        n, H_, W_, dev = self.n, self.H, self.W, self.dev
        im["flow"] = torch.full((n, H_, W_, 2), 7.0, device=dev)                    # (prefilled: every pixel must be written)
        im["flow_i16"] = torch.full((n, H_, W_, 2), 7, dtype=torch.int16, device=dev)
        pb = self.bs[:, :7].contiguous() if prev_poses is None else self._body_state(prev_poses, 7)
        pc = self.cam.clone() if prev_cams is None else self._cam(prev_cams)
        pv = torch.as_tensor(np.asarray(valid), dtype=torch.int32).to(dev)
        self.r.render(self.bs, self.cam, self.seg, self.col, self.camera, prev_body_pose=pb, prev_cam_pose=pc, prev_valid=pv, **im)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in im.items()}


def _moving_scene(n, seed):
    """tests/test_gpu_camera.py's mixed scene (one box, sphere, capsule and hull per env, each with its own segmentation
    id) as the current frame, and a previous frame in which every body and the camera stood elsewhere by a small rigid
    motion; all poses rounded to float32, the values the kernel gets."""
    defs, poses, cams, seg, col = tc._mixed_scene(n, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    poses = _round_poses(poses)
    cams = [(_f32(p), _f32(q)) for p, q in cams]
    prev_poses = _round_poses([[_perturb(rng, p, q) for p, q in env] for env in poses])
    prev_cams = [tuple(_f32(v) for v in _perturb(rng, p, q)) for p, q in cams]
    return defs, poses, cams, seg, col, prev_poses, prev_cams


def _assert_same_cast(a, b):
    for k in ("depth", "seg_out", "rgba"):
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=k)       # bit for bit (inf included)


def _assert_zero_bits(flow, flow_i16):
    assert not flow.view(np.uint32).any(), "flow is not +0.0 everywhere"
    assert not flow_i16.any()


# ---- 1. the same cast ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ground", ["heightfield", "trimesh"])
def test_the_flow_launch_writes_the_same_depth_segmentation_and_color(ground):
    tc._need_gpu()
    n = 3
    defs, poses, cams, seg, col, prev_poses, prev_cams = _moving_scene(n, seed=7)
    if ground == "heightfield":
        t, hs = tc._heightfield()
        sc = _Scene(defs, poses, cams, seg, col, terrain=t, heights=hs)
    else:
        from tests import test_gpu_camera_trimesh as tt
        hs, warp, t = tt._fixture()
        lift = np.array([0.0, 0.0, 0.4])                      # the fixture's platform is 0.36 m high
        up = lambda ps: [[(_f32(p + lift), q) for p, q in env] for env in ps]
        poses, prev_poses = up(poses), up(prev_poses)
        cams, prev_cams = [(_f32(p + lift), q) for p, q in cams], [(_f32(p + lift), q) for p, q in prev_cams]
        sc = _Scene(defs, poses, cams, seg, col, terrain=t, heights=hs, warp=warp)
    plain = sc.plain()
    assert np.isfinite(plain["depth"]).mean() > 0.5 and len(np.unique(plain["seg_out"])) > 3
    invalid = sc.flow(prev_poses, prev_cams, [0] * n)
    _assert_same_cast(plain, invalid)
    _assert_zero_bits(invalid["flow"], invalid["flow_i16"])
    valid = sc.flow(prev_poses, prev_cams, [1, 0, 1])
    _assert_same_cast(plain, valid)
    _assert_zero_bits(valid["flow"][1], valid["flow_i16"][1])
    hit = np.isfinite(plain["depth"])
    for e in (0, 2):
        assert (valid["flow"][e][hit[e]] != 0).any(axis=-1).mean() > 0.99       # everything moved against the camera
        _assert_zero_bits(valid["flow"][e][~hit[e]], valid["flow_i16"][e][~hit[e]])


# ---- 2. exact zero, and the wall's closed form ----------------------------------------------------------------------------
def test_static_env_is_bitwise_zero_and_a_sliding_camera_shows_the_closed_form():
    """Two envs with a valid previous frame.  Env 1: every pose bit-equal -> +0.0 everywhere.  Env 0: the camera moved by
    0.1 along its right axis, a wall at depth 2, W = 32, fov 90: u = -W D / (2 z) = -0.8, v = 0 on the wall."""
    tc._need_gpu()
    from shifu_amd.model import RenderShape
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    defs = [RenderShape(0, "box", np.zeros(3), np.eye(3), np.array([1.0, 100.0, 100.0]))]
    poses = [[(np.array([2.5, 0.0, 0.0]), ident)]] * 2                # front face: the plane x = 2
    cams = [(np.array([0.0, -0.1, 0.0]), ident), (np.array([0.0, 0.1, 0.2]), ident)]      # right = -y
    prev_cams = [(np.zeros(3), ident), cams[1]]
    sc = _Scene(defs, poses, cams, [[5], [5]], np.ones((2, 1, 3)), ground=False, W_=32, H_=24, fov=90.0, near=0.1, far=10.0)
    out = sc.flow(None, prev_cams, [1, 1])
    assert (out["seg_out"] == 5).all()
    np.testing.assert_allclose(out["depth"][0], 2.0, rtol=1e-6)
    _assert_zero_bits(out["flow"][1], out["flow_i16"][1])
    err = np.abs(out["flow"][0] - np.array([-0.8, 0.0])).max()
    print(f"wall: largest |flow - (-0.8, 0)| = {err:.3g} px")
    assert err <= FLOW_TOL
    # a static body in front of a moved camera moves in the image; a moved body in front of a static camera too
    moved_wall = [[(np.array([2.5, 0.05, 0.0]), ident)]] * 2
    out = sc.flow(moved_wall, [cams[0], cams[1]], [1, 1])
    np.testing.assert_allclose(out["flow"][..., 0], 32 * 0.05 / (2 * 2.0), atol=FLOW_TOL)       # the wall slid to the right (-y)
    np.testing.assert_allclose(out["flow"][..., 1], 0.0, atol=FLOW_TOL)


# ---- 3. / 4. against the checker; the int16 image ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checked_scene():
    """The scene of tests 3 and 4, rendered once, and its float64 reference."""
    tc._need_gpu()
    n = 3
    defs, poses, cams, seg, col, prev_poses, prev_cams = _moving_scene(n, seed=7)
    t, hs = tc._heightfield()
    out = _Scene(defs, poses, cams, seg, col, terrain=t, heights=hs).flow(prev_poses, prev_cams, [1] * n)
    ground = (hs, t.hscale, t.vscale, t.border)
    ref = [fr.flow(tc._ref_shapes(defs, poses[e], seg[e], col[e]), tc._ref_shapes(defs, prev_poses[e], seg[e], col[e]), cams[e],
                   prev_cams[e], W, H, FOV, NEAR, FAR, ground=ground) for e in range(n)]
    return out, ref


def _flow_errors(flow, depth, seg, ref):
    """(|flow - ref| on the pixels where hit flag and segmentation id agree with the checker's, disagreeing pixels, pixels)."""
    rflow, rdepth, rid, _ = ref
    got = np.where(np.isfinite(depth), seg, -1)
    agree = got == rid
    return np.abs(flow - rflow).max(-1)[agree], int((~agree).sum()), agree.size


def _check_against_ref(errs, bad, npx, tag):
    errs = np.concatenate(errs)
    print(f"{tag}: {bad} of {npx} pixels disagree with the checker; on the others max |flow - ref| = {errs.max():.3g} px, "
          f"99.9th percentile {np.quantile(errs, 0.999):.3g} px, mean {errs.mean():.3g} px")
    assert bad <= 0.005 * npx
    assert (errs > FLOW_TOL).mean() <= 0.001, f"{(errs > FLOW_TOL).sum()} of {errs.size} pixels off by more than {FLOW_TOL:.3g} px"


def test_flow_against_the_float64_checker(checked_scene):
    out, ref = checked_scene
    errs, bad = [], 0
    for e in range(len(ref)):
        assert len(np.unique(ref[e][2])) >= 5                     # the terrain and the four bodies (and perhaps sky) in view
        assert np.abs(ref[e][0]).max() > 1.0                      # pixels of motion, not noise
        er, b, _ = _flow_errors(out["flow"][e], out["depth"][e], out["seg_out"][e], ref[e])
        errs.append(er)
        bad += b
    _check_against_ref(errs, bad, len(ref) * W * H, "mixed scene")


def test_flow_i16_is_the_quantised_flow(checked_scene):
    from shifu_amd.render import flow_from_i16, flow_to_i16
    out, _ = checked_scene
    assert out["flow_i16"].any()
    np.testing.assert_array_equal(out["flow_i16"], flow_to_i16(out["flow"], W, H))
    np.testing.assert_array_equal(out["flow_i16"], flow_to_i16(torch.from_numpy(out["flow"]), W, H).numpy())
    assert np.abs(flow_from_i16(out["flow_i16"], W, H) - out["flow"]).max() <= 0.5 * max(W, H) / 32768 * (1 + 1e-6)


# ---- 5. batch independence ---------------------------------------------------------------------------------------------------
def test_flow_batch_independence():
    """Envs permuted or rendered as a subset give bitwise the same per-env flow."""
    tc._need_gpu()
    n = 6
    defs, poses, cams, seg, col, prev_poses, prev_cams = _moving_scene(n, seed=9)
    t, hs = tc._heightfield()
    valid = [1, 1, 0, 1, 1, 1]
    full = _Scene(defs, poses, cams, seg, col, terrain=t, heights=hs).flow(prev_poses, prev_cams, valid)
    assert full["flow"].any()
    perm = np.random.default_rng(0).permutation(n)
    for idx in (list(perm), [4, 0, 3]):
        pick = lambda xs: [xs[i] for i in idx]
        part = _Scene(defs, pick(poses), pick(cams), pick(seg), pick(col), terrain=t, heights=hs).flow(
            pick(prev_poses), pick(prev_cams), pick(valid))
        for k in full:
            np.testing.assert_array_equal(full[k][idx].view(np.uint8), part[k].view(np.uint8), err_msg=k)


# ---- 6. the fused env -----------------------------------------------------------------------------------------------------------
def test_fused_abb_env_flow_camera():
    tc._need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from tests import trimesh_render_ref as tr
    n, CW, CH, CFOV, CNEAR, CFAR = 8, 32, 24, 42.0, 0.1, 3.0         # the vision stage's view of the push-box scene
    env = FusedAbbEnv(num_envs=n, seed=5)
    nb = int(env.cm.blob.nb)
    B = nb + len(env.boxes)
    env.cam_seg.copy_(torch.arange(1, B + 1, dtype=torch.int32).repeat(n, 1))         # a segmentation id per body-state row
    pos, target = np.array([0.7, 0.0, 0.7]), np.array([0.0, 0.0, 0.1])
    plain = env.add_camera(CW, CH, CFOV, CNEAR, CFAR, position=pos, target=target)
    cam = env.add_camera(CW, CH, CFOV, CNEAR, CFAR, position=pos, target=target, flow=True)
    assert set(plain.render()) == set(plain.raw_images()) == {"rgba", "depth", "seg"}      # flow=False: the dict as before
    env.reset()
    im = cam.render()
    assert set(im) == {"rgba", "depth", "seg", "flow", "flow_i16"} and im is cam.raw_images()
    assert im["flow"].shape == (n, CH, CW, 2) and im["flow_i16"].dtype == torch.int16
    torch.cuda.synchronize()
    _assert_zero_bits(im["flow"].cpu().numpy(), im["flow_i16"].cpu().numpy())          # the first render: no previous frame
    count = env.task.tensors[_abi.ABB_RESET_COUNT]
    bs0, c0 = env.body_state.clone(), count.clone()
    env.episode_length_buf[3] = env.max_episode_length + 1       # env 3 times out in this step: reset inside the step kernel
    g = torch.Generator().manual_seed(2)
    env.step((2 * torch.rand(n, 3, generator=g) - 1).sign().to(env.device))            # full-scale actions
    im = cam.render()
    plain.render()
    torch.cuda.synchronize()
    for k in ("rgba", "depth", "seg"):
        assert torch.equal(im[k], plain.raw_images()[k]), k                            # the same cast as the plain camera's
    reset = (count != c0).cpu().numpy()
    assert reset[3] and not reset.all()
    bs = [b.view(n, B, 13).cpu().numpy().astype(np.float64) for b in (bs0, env.body_state)]
    flow, q = im["flow"].cpu().numpy(), im["flow_i16"].cpu().numpy()
    depth, seg = (-im["depth"]).cpu().numpy(), im["seg"].cpu().numpy()
    segs, cols = env.cam_seg.cpu().numpy(), env.cam_color.cpu().numpy()
    pose = cam.world_pose().cpu().numpy().astype(np.float64)
    camera = (pose[0, :3], pose[0, 3:])

    def shapes(rows, e):
        out = tr.world_shapes(env.cm.render_shapes, rows, segs[e], cols[e])
        for k, b in enumerate(env.boxes):
            from tests import render_ref as rr
            out.append(dict(kind="box", pos=rows[nb + k][:3], rot=rr.qmat(rows[nb + k][3:7]), half=0.5 * np.asarray(b.dim, float),
                            seg=int(segs[e][nb + k]), color=cols[e][nb + k]))
        return out

    errs, bad, npx = [], 0, 0
    for e in range(n):
        if reset[e]:
            _assert_zero_bits(flow[e], q[e])                     # its reset counter changed between the two renders
            continue
        arm = (seg[e] >= 1) & (seg[e] <= nb)
        assert arm.sum() > 20 and (flow[e][arm] != 0).any(axis=-1).sum() > 10, "no flow on the arm"
        ref = fr.flow(shapes(bs[1][e], e), shapes(bs[0][e], e), camera, camera, CW, CH, CFOV, CNEAR, CFAR, ground="plane")
        er, b, m = _flow_errors(flow[e], depth[e], seg[e], ref)
        errs.append(er)
        bad, npx = bad + b, npx + m
    _check_against_ref(errs, bad, npx, "FusedAbbEnv")
    from shifu_amd.render import flow_to_i16
    np.testing.assert_array_equal(q, flow_to_i16(flow, CW, CH))
    # env.reset() voids every env's previous frame, whatever the counters say
    env.reset()
    im = cam.render()
    torch.cuda.synchronize()
    _assert_zero_bits(im["flow"].cpu().numpy(), im["flow_i16"].cpu().numpy())
    env.destroy()


# ---- 7. the facade and CameraSensor under SHIFU_AMD_OPTICAL_FLOW=1 --------------------------------------------------------------
def test_facade_optical_flow_image(monkeypatch):
    tc._need_gpu()
    import os
    monkeypatch.setenv("SHIFU_AMD_OPTICAL_FLOW", "1")
    from shifu_amd.isaacgym import gymapi, gymtorch
    from shifu_amd.model import asset_path
    from shifu_amd.render import flow_from_i16
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
    props.width, props.height, props.horizontal_fov, props.near_plane, props.far_plane = 32, 24, 60.0, 0.05, 5.0
    envs = []
    for e in range(3):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        gym.create_actor(env, arm, gymapi.Transform(gymapi.Vec3(-0.5, 3.0, 0)), "arm", e, 0)     # out of the view
        b = gym.create_actor(env, box, gymapi.Transform(gymapi.Vec3(0.6, 0.0, 0.6)), "box", e, 0)    # in the air: it falls
        bp = gym.get_actor_rigid_body_properties(env, b)
        bp[0].mass = 1.0                                              # (a box actor without a mass is static)
        gym.set_actor_rigid_body_properties(env, b, bp)
        gym.set_rigid_body_segmentation_id(env, b, 0, 40 + e)
        c = gym.create_camera_sensor(env, props)
        gym.set_camera_location(c, env, gymapi.Vec3(1.8, 0.0, 0.5), gymapi.Vec3(0.0, 0.0, 0.4))
        envs.append(env)
    gym.prepare_sim(sim)
    gym.simulate(sim)
    gym.render_all_camera_sensors(sim)
    torch.cuda.synchronize()
    g = sim.camera_groups[0]
    assert set(gym.camera_group_tensors(sim, 0)) == {"rgba", "depth", "seg", "flow"}
    assert gym.camera_group_tensors(sim, 0)["flow"] is g["flow_i16"]
    views = [gymtorch.wrap_tensor(gym.get_camera_image_gpu_tensor(sim, env, 0, gymapi.IMAGE_OPTICAL_FLOW)) for env in envs]
    for e, v in enumerate(views):
        assert tuple(v.shape) == (24, 32, 2) and v.dtype == torch.int16
        assert v.data_ptr() == g["flow_i16"][e].data_ptr()                              # zero-copy row of the group tensor
        assert not v.any()                                                              # the first render: no previous frame
    for _ in range(4):
        gym.simulate(sim)
    gym.render_all_camera_sensors(sim)
    torch.cuda.synchronize()
    seg = g["seg"].cpu().numpy()
    for e, v in enumerate(views):
        px = flow_from_i16(v, 32, 24).cpu().numpy()
        on = seg[e] == 40 + e
        assert on.sum() > 10 and (px[on][:, 1] > 0).all()             # the box fell: it moved down the image (v > 0)
        assert not px[~on].any()                                      # plane and sky: static under a static camera
    # invalidate_camera_flow: env 1's next frame is zero, the others' is not
    gym.invalidate_camera_flow(sim, 0, [1])
    gym.set_camera_location(0, envs[0], gymapi.Vec3(1.8, 0.05, 0.5), gymapi.Vec3(0.0, 0.0, 0.4))
    gym.set_camera_location(0, envs[1], gymapi.Vec3(1.8, 0.05, 0.5), gymapi.Vec3(0.0, 0.0, 0.4))
    gym.simulate(sim)
    gym.render_all_camera_sensors(sim)
    torch.cuda.synchronize()
    assert views[0].any() and not views[1].any()
    gym.destroy_sim(sim)


def _flow_vision_env(n):
    """tests/test_gpu_camera.py's push-box env with the vision stage's camera, at 32 x 24 and with all four image types."""
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

    class FlowCameraConfig(CameraSensorConfig):
        name = 'flow_camera'
        local_lookat_positions = [[0.7, 0., 0.7], [0., 0., 0.1]]
        image_types = [ga.IMAGE_COLOR, ga.IMAGE_DEPTH, ga.IMAGE_SEGMENTATION, ga.IMAGE_OPTICAL_FLOW]
        image_normalization = True

        class camera_props(CameraSensorConfig.camera_props):
            enable_tensors = True
            width, height, horizontal_fov, near_plane, far_plane = 32, 24, 60, 0.1, 3

    class AbbPushBoxFlow(AbbPushBox):
        def __init__(self, cfg):
            ShifuVecEnv.__init__(self, cfg)
            self.robot = AbbRobot(AbbRobotConfig())
            self.table = Box(TableConfig())
            self.cube = RandPosBox(PushBoxConfig())
            self.goal = GoalBox(GoalBoxConfig())
            self.camera = CameraSensor(FlowCameraConfig())
            self.isg_env.create_envs(robot=self.robot, objects=[self.table, self.cube, self.goal], sensors=[self.camera])
            self.success_buf = torch.zeros(self.num_envs, device=self.device, dtype=torch.float)

    cfg = PriorStageEnvConfig()
    cfg.num_envs = n
    return AbbPushBoxFlow(cfg)


@pytest.mark.parametrize("graphs", [False, True])
def test_camera_sensor_optical_flow_buf_and_reset_idx(monkeypatch, graphs):
    """CameraSensor with the reference's four image types: optical_flow_buf is the group's flow image; reset_idx([1]) zeroes
    env 1's next frame only (and that of any env the step itself resets).  graphs: the same under enable_graph_hooks, the
    flow launch and the history update replayed from the second hipGraph."""
    tc._need_gpu()
    monkeypatch.setenv("SHIFU_AMD_OPTICAL_FLOW", "1")
    torch.manual_seed(0)
    n = 6
    env = _flow_vision_env(n)
    cam = env.camera
    assert cam.optical_flow_buf.shape == (n, 24, 32, 2) and cam.optical_flow_buf.dtype == torch.int16
    env.reset()
    if graphs:
        env.enable_graph_hooks()
        assert env._hook_graphs is not None
    g = torch.Generator().manual_seed(3)
    act = lambda: (2 * torch.rand(n, env.num_actions, generator=g) - 1).sign().to(env.device)
    for _ in range(3):
        _, _, _, done, _ = env.step(act())
    torch.cuda.synchronize()
    group = env.isg_env.gym.camera_group_tensors(env.isg_env.sim, cam.camera_handle)["flow"]
    assert cam.raw_images()["flow"] is group and torch.equal(cam.optical_flow_buf, group)
    moving = ~done.bool().cpu().numpy()
    flow = cam.optical_flow_buf.cpu().numpy()
    assert moving.sum() >= n - 2 and all(flow[e].any() for e in range(n) if moving[e])       # the arm moves in every env
    env.reset_idx(torch.tensor([1], device=env.device))
    _, _, _, done, _ = env.step(act())
    torch.cuda.synchronize()
    flow = cam.optical_flow_buf.cpu().numpy()
    zero = done.bool().cpu().numpy().copy()
    zero[1] = True
    for e in range(n):
        assert flow[e].any() != zero[e], (e, zero)
    env.destroy()
