"""The ray caster on the GPU (shf_raycast: k_raycast / k_raycast_tw, csrc/shf_render.hip; Renderer.raycast, the fused envs'
add_ray_caster, units.RayCasterSensor) against the float64 brute force tests/raycast_ref.py, against the camera kernel on the
same rays, its bitwise invariances (ray order, env order, pattern length, the cull, the mask), the alignment rule on known
answers, the envs, and the refusals.  Fixtures and caps: tests/raycast_ref.py (SENSORS)."""
import ctypes as C

import numpy as np
import pytest

from shifu_amd import _abi
from tests import raycast_ref as rc
from tests import trimesh_render_ref as tr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KEYS = ("dist", "points", "normal", "seg", "body")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


def _renderer(defs, nb, terrain, ground=True):
    """A Renderer of `defs` over the plane, the fixture's height field or its warped trimesh."""
    from shifu_amd.isaacgym.terrain_utils import trimesh_warp_map
    from shifu_amd.render import Renderer, build_scene
    if terrain == "plane":
        return Renderer(build_scene(defs, nb, ground=ground), None, None, "cuda:0")
    hs = tr.fixture_samples()
    t = _abi.ShfTerrain()
    t.rows, t.cols = hs.shape
    t.hscale, t.vscale, t.border = tr.HSCALE, tr.VSCALE, tr.BORDER
    sc = build_scene(defs, nb, ground=ground, height_samples=hs, vscale=t.vscale)
    if terrain == "heightfield":
        return Renderer(sc, t, hs, "cuda:0")
    t.warped = 1
    return Renderer(sc, t, hs, "cuda:0", warp=trimesh_warp_map(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD))


def _body_state(poses):
    """(E * nb, 13) body states of poses[e][k] = (pos, quat)."""
    nb = max(len(poses[0]), 1)
    bs = torch.zeros(len(poses) * nb, 13)
    bs[:, 6] = 1.0
    for e, env in enumerate(poses):
        for k, (p, q) in enumerate(env):
            bs[e * nb + k, :3] = torch.tensor(p)
            bs[e * nb + k, 3:7] = torch.tensor(q)
    return bs.to("cuda:0")


def _cast(r, bs, pose, pattern, align, lo, hi, mask=None, seg=None, keys=KEYS):
    """One shf_raycast launch: numpy outputs by name.  pose: (7,) for every env or (n, 7); seg: (n, nb) int32 table."""
    from shifu_amd.render import shape_mask_for
    dev = torch.device("cuda:0")
    n = bs.shape[0] // r.scene.num_bodies
    pose = np.asarray(pose, np.float32)
    pose = torch.from_numpy(np.broadcast_to(pose, (n, 7)).copy()).to(dev)
    o, d = (torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) for a in pattern)
    R = o.shape[0]
    out = dict(dist=torch.full((n, R), -7.0, device=dev), points=torch.full((n, R, 3), -7.0, device=dev),
               normal=torch.full((n, R, 3), -7.0, device=dev), seg=torch.full((n, R), -7, dtype=torch.int32, device=dev),
               body=torch.full((n, R), -7, dtype=torch.int32, device=dev))
    out = {k: v for k, v in out.items() if k in keys and (k != "seg" or seg is not None)}      # (no table, no seg output)
    segt = None if seg is None else torch.as_tensor(np.asarray(seg), dtype=torch.int32).to(dev).contiguous()
    r.raycast(bs, pose, o, d, align, lo, hi, shape_mask_for(r.scene) if mask is None else mask, seg=segt, dist=out.get("dist"),
              points=out.get("points"), normal=out.get("normal"), seg_out=out.get("seg"), body=out.get("body"))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _sensor_pose(name):
    return np.concatenate([np.asarray(rc.SENSORS[name][1], float), rc.SENSOR_QUAT])


def _fixture_cast(name, terrain, seed, **kw):
    sc = rc.scene(seed)
    r = _renderer(sc.defs, sc.nb, terrain)
    _, _, align, lo, hi, _, _ = rc.SENSORS[name]
    return sc, r, _cast(r, _body_state(sc.poses), _sensor_pose(name), rc.pattern(name), align, lo, hi, seg=sc.seg, **kw)


def _equal(a, b, rows=None, what=""):
    for k in a:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        assert x.tobytes() == y.tobytes(), f"{what}: {k} differs in {int((x != y).sum())} values"


# ---- 1: against the float64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", rc.SEEDS)
@pytest.mark.parametrize("terrain", rc.TERRAINS)
@pytest.mark.parametrize("name", sorted(rc.SENSORS))
def test_against_the_reference(name, terrain, seed):
    _need_gpu()
    _, pos, _, _, hi, amb_cap, _ = rc.SENSORS[name]
    sc, _, out = _fixture_cast(name, terrain, seed)
    refs = rc.fixture(name, terrain, seed)
    for e, ref in enumerate(refs):
        body, seg, dist, pts, nrm = (out[k][e] for k in ("body", "seg", "dist", "points", "normal"))
        amb, facet, rid = ref["ambiguous"], ref["facet"], ref["id"]
        bad = body != rid
        print(f"{name} {terrain} seed {seed} env {e}: {int(bad.sum())} ids differ, {int(amb.sum())} ambiguous, "
              f"{int(facet.sum())} on facet edges of {len(rid)} rays")
        assert not (bad & ~amb).any(), f"{int((bad & ~amb).sum())} id mismatches outside the ambiguity mask"
        assert bad.mean() <= amb_cap, f"{bad.mean():.4f} of the rays differ"
        # seg: the hit body's entry of the table, 0 for the terrain and for a miss -- consistent with body on EVERY ray
        want_seg = np.where(body >= 0, sc.seg[e][np.maximum(body, 0)], 0)
        np.testing.assert_array_equal(seg, want_seg)
        ok = ~bad & (rid != rc.MISS)
        tol = 1e-4 + 1e-6 * ref["dist"][ok] / np.maximum(ref["cos"][ok], 1e-6)
        err = np.abs(dist[ok] - ref["dist"][ok])
        perr = np.abs(pts[ok] - ref["points"][ok]).max(1)
        print(f"  dist: max error {err.max(initial=0):.3g} m, error / bound {(err / tol).max(initial=0):.3g}; points: max "
              f"error {perr.max(initial=0):.3g} m, error / bound {(perr / (tol + 1e-5)).max(initial=0):.3g}")
        assert (err <= tol).all(), f"dist off by {err.max():.3g} m"
        assert (perr <= tol + 1e-5).all(), f"points off by {perr.max():.3g} m"
        shade_ok = ok & ~amb & ~facet
        ndot = np.einsum("ij,ij->i", nrm[shade_ok].astype(np.float64), ref["normal"][shade_ok])
        print(f"  normal: min n . n_ref {ndot.min(initial=1):.8f}")
        assert (ndot >= 1 - 1e-5).all()
        # the miss conventions, exactly: +inf, zero normal, seg 0, body -2; the point is the ray's end at max_range
        miss = body == rc.MISS
        assert np.array_equal(miss, np.isinf(dist)) and (dist[miss] > 0).all() and np.isfinite(pts).all()
        assert (nrm[miss] == 0).all() and (seg[miss] == 0).all()
        both = miss & (rid == rc.MISS)
        assert (np.abs(pts[both] - ref["points"][both]) <= 1e-5).all()
        if name == "lidar":                                                   # (its rays all start at the sensor)
            np.testing.assert_allclose(np.linalg.norm(pts[miss].astype(np.float64) - np.asarray(pos), axis=1), hi, rtol=1e-6)


def test_degenerate_directions():
    """A zero or non-finite direction is a miss whose point is the ray's origin; a long direction still gives the range."""
    _need_gpu()
    r = _renderer([], 1, "plane")
    bs = _body_state([[]])
    o = np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 0.0], [0.3, 0.0, 0.0]], np.float32)
    d = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, -1.0], [0.0, 0.0, -2.0], [np.inf, 0.0, -1.0]], np.float32)
    out = _cast(r, bs, [0, 0, 1.0, 0, 0, 0, 1.0], (o, d), "world", 0.0, 5.0)
    assert out["body"][0].tolist() == [-2, -2, -1, -2]
    np.testing.assert_array_equal(out["points"][0], np.array([[0.1, 0, 1.0], [0, 0.2, 1.0], [0, 0, 0], [0.3, 0, 1.0]], np.float32))
    assert out["dist"][0][2] == 1.0 and np.isinf(out["dist"][0][[0, 1, 3]]).all()
    assert (out["normal"][0][2] == [0, 0, 1]).all() and (out["normal"][0][[0, 1, 3]] == 0).all()


# ---- 2: against the camera kernel -------------------------------------------------------------------------------------------
def test_pinhole_pattern_against_the_camera():
    _need_gpu()
    from shifu_amd.raycast import pinhole_pattern
    from shifu_amd.render import camera_struct
    from tests import render_ref as rr
    W, H, FOV = 64, 48, 87.0
    sc = rc.scene(2)
    r = _renderer(sc.defs, sc.nb, "heightfield")
    bs = _body_state(sc.poses)
    pos, quat = tr.fixture_cameras()[0]
    pose = np.concatenate([pos, quat])
    o, d = pinhole_pattern(W, H, FOV)
    out = _cast(r, bs, pose, (o, d), "base", 0.0, 20.0, seg=sc.seg)
    dev = torch.device("cuda:0")
    n = sc.E
    cam = camera_struct(W, H, FOV, tr.CAM_NEAR, tr.CAM_FAR)
    depth = torch.empty(n, H, W, device=dev)
    segi = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    posed = torch.tensor(np.broadcast_to(pose, (n, 7)).copy(), dtype=torch.float32, device=dev)
    r.render(bs, posed, torch.from_numpy(sc.seg).to(dev).contiguous(), torch.from_numpy(sc.col).to(dev).contiguous(), cam,
             depth=depth, seg_out=segi)
    cpts, lpts = torch.empty(n, H, W, 3, device=dev), torch.empty(n, H, W, 3, device=dev)
    r.camera_points(depth, posed, cam, cpts)
    r.camera_points(-depth, posed, cam, lpts, world_frame=False)          # the other sign convention, the camera's own axes
    torch.cuda.synchronize()
    depth, segi, cpts, lpts = depth.cpu().numpy(), segi.cpu().numpy(), cpts.cpu().numpy(), lpts.cpu().numpy()
    norm = np.linalg.norm(d.astype(np.float64), axis=1).reshape(H, W)
    Rc = rr.qmat(quat)
    for e in range(n):
        cid = np.where(np.isfinite(depth[e]), segi[e], -1)
        gid = np.where(np.isfinite(out["dist"][e]), out["seg"][e], -1).reshape(H, W)
        bad = cid != gid
        edge = rr.silhouette_adjacent(cid)
        print(f"env {e}: {int(bad.sum())} of {bad.size} ids differ ({int((bad & ~edge).sum())} away from silhouettes)")
        assert not (bad & ~edge).any() and bad.mean() <= 0.005
        assert (cid > 0).sum() > 50 and (cid == 0).sum() > 500 and (cid == -1).sum() > 50
        ok = ~bad & np.isfinite(depth[e])
        dist, pts, nrm = out["dist"][e].reshape(H, W), out["points"][e].reshape(H, W, 3), out["normal"][e].reshape(H, W, 3)
        ray = (pts.astype(np.float64) - pos) / np.where(np.isfinite(dist), dist, 1.0)[..., None]
        cos = np.abs(np.einsum("hwk,hwk->hw", nrm.astype(np.float64), ray))
        tol = 2 * (1e-4 + 1e-6 * depth[e][ok] / np.maximum(cos[ok], 1e-6))
        err = np.abs(dist[ok] / norm[ok] - depth[e][ok])
        perr = np.abs(cpts[e][ok].astype(np.float64) - pts[ok]).max(1)
        print(f"  depth: max difference {err.max():.3g} m ({(err / tol).max():.3g} of the bound); points: {perr.max():.3g} m "
              f"({(perr / tol).max():.3g} of the bound)")
        assert (err <= tol).all() and (perr <= tol).all()
        # the camera-frame cloud is the world one seen from the camera: R^T (X - o), +x the view depth
        local = (cpts[e].astype(np.float64) - pos) @ Rc
        assert np.abs(local - lpts[e]).max() < 1e-5 * (1 + np.abs(local).max())
        np.testing.assert_array_equal(lpts[e][..., 0][ok], depth[e][ok])
        # nothing hit: the point at far_plane along the pixel's ray
        np.testing.assert_array_equal(lpts[e][..., 0][~np.isfinite(depth[e])], np.float32(tr.CAM_FAR))


# ---- 3: independence, bitwise -------------------------------------------------------------------------------------------------
def test_independence_of_ray_and_env_order_and_of_the_pattern_length():
    _need_gpu()
    name, terrain = "lidar", "heightfield"
    sc, r, full = _fixture_cast(name, terrain, 0)
    _, _, align, lo, hi, _, _ = rc.SENSORS[name]
    o, d = rc.pattern(name)
    pose = _sensor_pose(name)
    assert len(set(full["body"].ravel().tolist())) >= 5                       # misses, terrain and several bodies
    perm = np.random.default_rng(0).permutation(len(o))
    got = _cast(r, _body_state(sc.poses), pose, (o[perm], d[perm]), align, lo, hi, seg=sc.seg)
    _equal({k: v[:, perm] for k, v in full.items()}, got, what="rays permuted")
    for envs in ([1, 0], [1], [0, 1, 0]):                                      # permuted, a subset (1 env), 3 envs
        got = _cast(r, _body_state([sc.poses[e] for e in envs]), pose, (o, d), align, lo, hi, seg=sc.seg[envs])
        _equal({k: v[envs] for k, v in full.items()}, got, what=f"envs {envs}")
    for count in (1, 63, 64, 65, 257):
        got = _cast(r, _body_state(sc.poses), pose, (o[:count], d[:count]), align, lo, hi, seg=sc.seg)
        _equal({k: v[:, :count] for k, v in full.items()}, got, what=f"the first {count} rays")
    part = _cast(r, _body_state(sc.poses), pose, (o, d), align, lo, hi, seg=sc.seg, keys=("points", "body"))
    _equal({k: full[k] for k in part}, part, what="two outputs only")


# ---- 4: the cull ---------------------------------------------------------------------------------------------------------------
def _sixty_four_shapes(seed=5):
    """SHF_RENDER_MAX_SHAPES shapes, sixteen of each kind, each on a body of its own, around the lidar."""
    from tests import world_view_ref as wr
    rng = np.random.default_rng(seed)
    defs = []
    for _ in range(16):
        four = wr.shape_defs(rng)
        for s in four:
            s.body = len(defs)
            defs.append(s)
    poses = [[(rng.uniform([-1.5, -1.5, 0.1], [1.5, 1.5, 1.5]), wr.rand_quat(rng)) for _ in defs] for _ in range(2)]
    return defs, poses


def _without_cull(fn):
    from shifu_amd._lib import lib
    assert lib().shf_raycast_debug_cull(0) == 1
    try:
        return fn()
    finally:
        assert lib().shf_raycast_debug_cull(1) == 0


def test_the_cull_changes_no_bit():
    _need_gpu()
    for terrain in ("trimesh", "plane"):
        _, _, on = _fixture_cast("lidar", terrain, 0)
        _, _, off = _without_cull(lambda: _fixture_cast("lidar", terrain, 0))
        _equal(on, off, what=f"lidar fixture on the {terrain}")
    defs, poses = _sixty_four_shapes()
    assert len(defs) == _abi.RENDER_MAX_SHAPES
    r = _renderer(defs, len(defs), "plane")
    bs = _body_state(poses)
    seg = np.arange(1, 2 * len(defs) + 1, dtype=np.int32).reshape(2, -1)
    run = lambda pat, align: _cast(r, bs, _sensor_pose("lidar"), pat, align, 0.05, 6.0, seg=seg)
    for name in ("lidar", "grid"):
        on = run(rc.pattern(name), rc.SENSORS[name][2])
        off = _without_cull(lambda: run(rc.pattern(name), rc.SENSORS[name][2]))
        _equal(on, off, what=f"64 shapes, {name}")
        if name == "lidar":
            assert len(set(on["body"].ravel().tolist()) - {-1, -2}) >= 30     # most of the shapes are seen
    r0 = _renderer([], 1, "heightfield")                                      # no shapes: the terrain alone
    run0 = lambda: _cast(r0, _body_state([[], []]), _sensor_pose("grid"), rc.pattern("grid"), "yaw", 0.0, 3.0)
    on = run0()
    _equal(on, _without_cull(run0), what="terrain only")
    assert (on["body"] == -1).all()


# ---- 5: the mask --------------------------------------------------------------------------------------------------------------
def test_shape_mask():
    _need_gpu()
    from shifu_amd.render import shape_mask_for
    sc, r, full = _fixture_cast("lidar", "plane", 0)
    _, _, align, lo, hi, _, _ = rc.SENSORS["lidar"]
    bs, pose, pat = _body_state(sc.poses), _sensor_pose("lidar"), rc.pattern("lidar")
    hit = full["body"][full["body"] >= 0]
    b = int(np.bincount(hit).argmax())                                         # the body most rays report
    assert (full["body"] == b).sum() > 20
    mask = shape_mask_for(r.scene, [b])
    assert mask == 0b1111 & ~(1 << b)
    got = _cast(r, bs, pose, pat, align, lo, hi, mask=mask, seg=sc.seg)
    assert not (got["body"] == b).any() and not (got["seg"] == sc.seg[:, b][:, None]).any()
    other = full["body"] != b
    _equal(full, got, rows=other, what="rays that did not report the masked body")
    assert (got["dist"][~other] > full["dist"][~other]).all()                   # what lay behind it, or nothing
    # nothing to cast at all: every shape masked, no ground
    r2 = _renderer(sc.defs, sc.nb, "plane", ground=False)
    none = _cast(r2, bs, pose, pat, align, lo, hi, mask=0, seg=sc.seg)
    assert (none["body"] == -2).all() and np.isinf(none["dist"]).all() and (none["seg"] == 0).all() and (none["normal"] == 0).all()
    some = _cast(r2, bs, pose, pat, align, lo, hi, seg=sc.seg)
    assert (some["body"] >= 0).sum() > 100 and not (some["body"] == -1).any()


# ---- 6: alignment -----------------------------------------------------------------------------------------------------------
def test_alignment_on_the_plane():
    """From height h over the plane, a downward grid: yaw-aligned rays all return h whatever the roll and pitch; base-aligned
    ones o_z / R22 (the float64 closed form; float32 rotation entries through a handful of operations: 1e-5 relative leaves
    a margin of more than ten); world-aligned ones do not see the orientation at all."""
    _need_gpu()
    from shifu_amd.raycast import grid_pattern
    from tests import render_ref as rr
    r = _renderer([], 1, "plane")
    bs = _body_state([[]])
    pat = grid_pattern((1.56, 1.04), 0.13)
    h = 1.37
    for roll, pitch, yaw in ((0.1, -0.15, 0.7), (-0.4, 0.3, 2.9), (0.0, 0.0, -1.3)):
        q = rc.euler_quat(roll, pitch, yaw)
        pose = np.concatenate([[0.3, -0.2, h], q])
        out = _cast(r, bs, pose, pat, "yaw", 0.0, 5.0)
        assert (out["body"] == -1).all()
        np.testing.assert_allclose(out["dist"], h, rtol=1e-6)
        # the hit points: the grid turned by the yaw alone, on the ground
        a = np.arctan2(rr.qmat(q)[1, 0], rr.qmat(q)[0, 0])
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
        np.testing.assert_allclose(out["points"][0], np.asarray(pat[0], float) @ Rz.T + [0.3, -0.2, 0.0], atol=1e-5)
        R = rr.qmat(q)
        base = _cast(r, bs, pose, pat, "base", 0.0, 5.0)
        np.testing.assert_allclose(base["dist"][0], (h + (np.asarray(pat[0], float) @ R.T)[:, 2]) / R[2, 2], rtol=1e-5)
    w0 = _cast(r, bs, np.concatenate([[0.3, -0.2, h], rc.euler_quat(0.1, -0.15, 0.3)]), pat, "world", 0.0, 5.0)
    w1 = _cast(r, bs, np.concatenate([[0.3, -0.2, h], rc.euler_quat(-0.2, 0.4, 1.9)]), pat, "world", 0.0, 5.0)
    wi = _cast(r, bs, [0.3, -0.2, h, 0, 0, 0, 1.0], pat, "base", 0.0, 5.0)
    _equal(w0, w1, what="world-aligned, two orientations")
    _equal(w0, wi, what="world-aligned against the identity orientation")


# ---- 7: the envs --------------------------------------------------------------------------------------------------------------
def _by_hand(env, caster):
    """Renderer.raycast on the env's body states with the caster's own pattern and settings, into fresh tensors."""
    n, R, dev = env.num_envs, caster.num_rays, env.device
    out = dict(dist=torch.empty(n, R, device=dev), points=torch.empty(n, R, 3, device=dev),
               body=torch.empty(n, R, dtype=torch.int32, device=dev))
    env._renderer.raycast(env.body_state, caster.world_pose(), caster.origins, caster.dirs, caster.align, caster.min_range,
                          caster.max_range, caster.shape_mask, dist=out["dist"], points=out["points"], body=out["body"])
    return out


def test_height_scanner_on_the_fused_a1_env():
    _need_gpu()
    from shifu_amd.gym.a1_fused import FusedA1Env, default_terrain_cfg
    from shifu_amd.raycast import grid_pattern
    n = 8
    env = FusedA1Env(num_envs=n, terrain="trimesh",
                     terrain_cfg=default_terrain_cfg(mesh_type="trimesh", num_rows=1, num_cols=1, border_size=1, terrain_length=6.,
                                                     terrain_width=6.))
    assert env.sim.terrain.warped == 1
    keys = set(env.state_dict())
    scan = env.add_ray_caster(grid_pattern(), attach_body=0, align="yaw", position=(0, 0, 0.5), ignore_bodies="articulation",
                              max_range=3, outputs=("dist", "points", "body"))
    assert scan.num_rays == 17 * 11 and scan.shape_mask == 0
    env.reset()
    g = torch.Generator().manual_seed(7)
    for _ in range(3):
        env.step((2 * torch.rand(n, env.num_actions, generator=g) - 1).to(env.device))
    out = scan.cast()
    hand = _by_hand(env, scan)
    torch.cuda.synchronize()
    assert set(out) == {"dist", "points", "body"}
    for k in out:
        assert torch.equal(out[k], hand[k]), k
    assert bool((out["body"] == -1).all())                                     # the terrain under the robot, never the robot
    trunk_z = env.body_state.view(n, -1, 13)[:, 0, 2]
    assert bool(((out["dist"] > 0.2) & (out["dist"] < 3.0)).all())
    assert bool((out["points"][..., 2] < trunk_z[:, None] + 0.5).all())
    # with the robot in: some rays stop on it
    seen = env.add_ray_caster(grid_pattern(), attach_body=0, align="yaw", position=(0, 0, 0.5), max_range=3, outputs=("body",))
    assert int((seen.cast()["body"] >= 0).sum()) > 0
    assert set(env.state_dict()) == keys                                       # derived data: not part of the state
    # captured: the replay writes the same bits as the eager launch
    eager = {k: v.clone() for k, v in out.items()}
    for v in out.values():
        v.zero_()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        scan.cast()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scan.cast()
    for v in out.values():
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], eager[k]), k
    env.destroy()


def test_lidar_on_the_fused_abb_env_and_its_point_cloud():
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from shifu_amd.raycast import lidar_pattern
    n = 4
    env = FusedAbbEnv(num_envs=n, seed=5)
    nb = int(env.cm.blob.nb)
    ee = int(env.task_params.ee_body)
    lidar = env.add_ray_caster(lidar_pattern(8, (-60.0, 60.0), horizontal_res=4.0), attach_body=ee, align="base",
                               ignore_bodies="articulation", min_range=0.0, max_range=5.0, outputs=("dist", "points", "body", "seg", "normal"))
    cam = env.add_camera(32, 24, 60, 0.1, 3, position=(0.7, 0.0, 0.7), target=(0.0, 0.0, 0.1))
    env.cam_seg.copy_(torch.arange(1, env.cam_seg.numel() + 1, dtype=torch.int32, device=env.device).view_as(env.cam_seg))
    env.reset()
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        env.step((2 * torch.rand(n, 3, generator=g) - 1).to(env.device))
    out = lidar.cast()
    hand = _by_hand(env, lidar)
    torch.cuda.synchronize()
    for k in hand:
        assert torch.equal(out[k], hand[k]), k
    body = out["body"]
    assert not bool(((body >= 0) & (body < nb)).any())                         # never the arm
    assert int((body >= nb).sum()) > 0 and int(body.max()) < nb + len(env.boxes)     # the box rows: table, cube or goal
    hit = body >= 0
    assert torch.equal(out["seg"][hit], env.cam_seg.gather(1, body.clamp(min=0).long())[hit])
    # the camera's point cloud: the depth image's points, in the world and in the camera's axes
    cam.render()
    pts, local = cam.point_cloud().clone(), cam.point_cloud(world_frame=False).clone()
    torch.cuda.synchronize()
    depth = -cam.raw_images()["depth"]
    assert tuple(pts.shape) == (n, 24, 32, 3)
    shown = torch.isfinite(depth)
    assert torch.equal(local[..., 0][shown], depth[shown]) and bool((local[..., 0][~shown] == 3.0).all())
    eye = torch.tensor([0.7, 0.0, 0.7], device=env.device)
    rng_ = (pts - eye).norm(dim=-1)
    assert bool(((rng_ - local.norm(dim=-1)).abs() < 1e-5).all())
    assert float(pts[..., 2][shown].min()) > -1e-4                              # nothing below the ground
    env.destroy()


def test_ray_caster_sensor_on_a_hook_env():
    """RayCasterSensor in create_envs(sensors=[...]) on the push-box hook env: buffers, one launch per refresh, and the cast
    equals Renderer.raycast by hand on the sim's body states."""
    _need_gpu()
    from shifu_amd import compat
    compat.install()
    from shifu.configs import RayCasterSensorConfig
    from shifu.units import RayCasterSensor
    from examples.abb_pushbox_vision.a_prior_stage import AbbPushBox, AbbRobot, GoalBox, RandPosBox
    from examples.abb_pushbox_vision.task_config import (AbbRobotConfig, GoalBoxConfig, PriorStageEnvConfig, PushBoxConfig,
                                                         TableConfig)
    from shifu_amd.gym import ShifuVecEnv
    from shifu_amd.raycast import grid_pattern
    from shifu_amd.units import Box

    class ScanConfig(RayCasterSensorConfig):
        name = "height_scan"
        pattern = grid_pattern((0.6, 0.4), 0.1)
        transform = [[0.45, 0.0, 1.0], [0.0, 0.0, 0.0, 1.0]]
        align = "yaw"
        max_range = 3.0
        ignore_robot = True

    class AbbPushBoxScan(AbbPushBox):
        def __init__(self, cfg):
            ShifuVecEnv.__init__(self, cfg)
            self.robot = AbbRobot(AbbRobotConfig())
            self.table = Box(TableConfig())
            self.cube = RandPosBox(PushBoxConfig())
            self.goal = GoalBox(GoalBoxConfig())
            self.scan = RayCasterSensor(ScanConfig())
            self.isg_env.create_envs(robot=self.robot, objects=[self.table, self.cube, self.goal], sensors=[self.scan])
            self.success_buf = torch.zeros(self.num_envs, device=self.device, dtype=torch.float)

    cfg = PriorStageEnvConfig()
    cfg.num_envs = 6
    env = AbbPushBoxScan(cfg)
    env.reset()
    env.step(torch.zeros(env.num_envs, env.num_actions, device=env.device))
    scan, sim = env.scan, env.isg_env.sim
    R = 7 * 5
    assert scan.num_rays == R and tuple(scan.ray_distances.shape) == (6, R) and tuple(scan.ray_hits_w.shape) == (6, R, 3)
    torch.cuda.synchronize()
    got_d, got_p = scan.ray_distances.clone(), scan.ray_hits_w.clone()
    assert bool(torch.isfinite(got_d).all()) and float(got_d.max()) <= 1.0 + 1e-5     # the ground at most, the table or a box
    assert float(got_d.min()) < 0.99                                                   # ... and something above the ground
    nb = sim.robot_asset.num_bodies
    body = torch.empty(6, R, dtype=torch.int32, device=env.device)
    dist = torch.empty(6, R, device=env.device)
    g = scan._group
    sim.renderer.raycast(sim.backend.tensors[_abi.T_BODY_STATE], g["pose"], g["origins"], g["dirs"], g["align"], g["min_range"],
                         g["max_range"], g["shape_mask"], dist=dist, body=body)
    torch.cuda.synchronize()
    assert torch.equal(dist, got_d)
    assert not bool(((body >= 0) & (body < nb)).any()) and int((body >= nb).sum()) > 0
    env.destroy()


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    _need_gpu()
    from shifu_amd._lib import lib
    sc = rc.scene(0)
    r = _renderer(sc.defs, sc.nb, "plane")
    dev = torch.device("cuda:0")
    bs = _body_state(sc.poses)
    pose = torch.tensor(np.broadcast_to(_sensor_pose("grid"), (2, 7)).copy(), dtype=torch.float32, device=dev)
    o, d = (torch.from_numpy(a).to(dev) for a in rc.pattern("grid"))
    R = o.shape[0]
    segt = torch.from_numpy(sc.seg).to(dev).contiguous()
    dist, seg = torch.empty(2, R, device=dev), torch.empty(2, R, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    good = dict(scene=p(r._scene_dev), terrain=C.byref(r.terrain), heights=None, num_envs=2, num_rays=R, origin=p(o), dir=p(d),
                body_state=p(bs), pose=p(pose), align=0, lo=0.0, hi=3.0, mask=0xF, seg_ids=p(segt), dist=p(dist), points=None,
                normal=None, seg=p(seg), body=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib().shf_raycast(a["scene"], a["terrain"], a["heights"], a["num_envs"], a["num_rays"], a["origin"], a["dir"],
                                 a["body_state"], a["pose"], a["align"], C.c_float(a["lo"]), C.c_float(a["hi"]),
                                 C.c_uint64(a["mask"]), a["seg_ids"], a["dist"], a["points"], a["normal"], a["seg"], a["body"], None)

    assert call() == 0
    torch.cuda.synchronize()
    bad = [dict(num_envs=0), dict(num_rays=0), dict(num_envs=-1), dict(scene=None), dict(terrain=None), dict(origin=None),
           dict(dir=None), dict(body_state=None), dict(pose=None), dict(dist=None, seg=None), dict(align=-1), dict(align=3),
           dict(lo=-0.1), dict(lo=3.5), dict(hi=float("inf")), dict(hi=float("nan")), dict(lo=float("nan")), dict(seg_ids=None),
           dict(num_envs=2 ** 31 - 1, num_rays=257)]
    for kw in bad:
        rc_ = call(**kw)
        msg = lib().shf_last_error().decode()
        assert rc_ != 0 and msg.startswith("shf_raycast:"), (kw, rc_, msg)
    assert call(seg_ids=None, seg=None) == 0                                  # seg_ids may be null when seg is
    torch.cuda.synchronize()
    # the wrapper refuses what it can see before the launch
    with pytest.raises(ValueError):
        r.raycast(bs, pose, o, d, "sideways", 0.0, 3.0, 0xF, dist=dist)
    with pytest.raises(ValueError):
        r.raycast(bs, pose, o, d, "base", 0.0, 3.0, 0xF)
    with pytest.raises(ValueError):
        r.raycast(bs, pose, o, d, "base", 0.0, 3.0, 0xF, seg_out=seg)
    with pytest.raises(ValueError):
        r.raycast(bs, pose, o, d[:-1].contiguous(), "base", 0.0, 3.0, 0xF, dist=dist)
