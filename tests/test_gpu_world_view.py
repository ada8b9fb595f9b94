"""The world view on the GPU (shf_render_world: k_render_world / k_render_world_tw, csrc/shf_render.hip; Renderer.render_world,
viewer.Viewer, the fused envs' add_viewer): against the float64 caster tests/render_ref.py on the concatenated, displaced
shape list, against the depth-nearest composite of per-env shf_render_cameras images, the chunk and flush edges of the
candidate list, partial tiles, the bitwise invariances of the kernel with itself, the tie rule, the terrains, the envs, and
the frame recorder.  The acceptance criterion is tests/world_view_ref.py::compare (the project's own numbers)."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import world_view_ref as wr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, FOV = wr.W, wr.H, wr.FOV
NEAR, FAR = 0.1, 8.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


def _renderer(scene, terrain=None, heights=None, warp=None):
    from shifu_amd.render import Renderer, build_scene
    sc = build_scene(scene.defs, scene.nb, ground=True, height_samples=heights, vscale=terrain.vscale if terrain is not None else 1.0)
    return Renderer(sc, terrain, heights, "cuda:0", warp=warp)


def _tables(scene):
    dev = torch.device("cuda:0")
    bs = torch.zeros(scene.E * scene.nb, 13)
    bs[:, 6] = 1.0
    for e in range(scene.E):
        for k, (p, q) in enumerate(scene.poses[e]):
            bs[e * scene.nb + k, :3] = torch.tensor(p)
            bs[e * scene.nb + k, 3:7] = torch.tensor(q)
    return bs.to(dev), torch.from_numpy(scene.seg).to(dev).contiguous(), torch.from_numpy(scene.col).to(dev).contiguous()


def _world(scene, cams, env_ids=None, offsets=None, env_radius=0.0, r=None, near=NEAR, far=FAR, W_=W, H_=H, fov=FOV):
    """One shf_render_world launch for the views `cams`: (depth, seg, rgba, env) as numpy arrays, (V, H, W[, 4])."""
    from shifu_amd.render import camera_struct
    dev = torch.device("cuda:0")
    r = _renderer(scene) if r is None else r
    bs, seg, col = _tables(scene)
    V = len(cams)
    pose = torch.tensor(np.array([np.concatenate([p, q]) for p, q in cams]), dtype=torch.float32, device=dev)
    out = dict(depth=torch.empty(V, H_, W_, device=dev), seg_out=torch.empty(V, H_, W_, dtype=torch.int32, device=dev),
               rgba=torch.empty(V, H_, W_, 4, dtype=torch.uint8, device=dev), env_out=torch.empty(V, H_, W_, dtype=torch.int32, device=dev))
    ids = None if env_ids is None else torch.tensor(list(env_ids), dtype=torch.int32, device=dev)
    off = None if offsets is None else torch.tensor(np.asarray(offsets), dtype=torch.float32, device=dev).contiguous()
    r.render_world(bs, pose, seg, col, camera_struct(W_, H_, fov, near, far), env_ids=ids, env_offset=off, env_radius=env_radius, **out)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("depth", "seg_out", "rgba", "env_out"))


def _overview(rng=None, centre=(0.9, 0.0, 0.25), eye=(-1.6, -0.3, 1.5)):
    from shifu_amd.render import lookat_quat
    eye = np.asarray(eye, float) + (rng.uniform(-0.2, 0.2, 3) if rng is not None else 0.0)
    return eye, lookat_quat(eye, centre)


def _spread_scene(E, seed):
    """E envs, all posed about the origin, spread by offsets over the ground plane in front of _overview's camera, 1 to
    3.5 m from it: the range of tests/test_gpu_camera.py's scenes, for which the depth bound of the criterion was set.  (The
    float32 closed forms the kernels share lose accuracy with range: hit_sphere's discriminant b^2 - a c cancels at the
    size of |o|^2, so its entry depth errs by about ulp(s^2) / (r cos) -- quadratic in s where the bound's 1e-6 s / cos is
    linear.  That is the shared intersection code's, at any range, and not what these tests are about.)"""
    sc = wr.Scene(E, seed)
    off = np.zeros((E, 3))
    off[:, 0] = sc.rng.uniform(0.0, 1.8, E)
    off[:, 1] = sc.rng.uniform(-1.2, 1.2, E)
    return sc, off


# ---- 1, 2: against float64 and against the per-env composite ------------------------------------------------------------
_SIX = {}


def _six_envs():
    """The six-env scene of tests 1 and 2 with its float64 reference, computed once and left unchanged."""
    if not _SIX:
        sc, off = _spread_scene(6, seed=21)
        cam = _overview()
        ids = list(range(6))
        ref, ref_env = wr.reference(sc, ids, off, cam, NEAR, FAR)
        _SIX.update(sc=sc, off=off, cam=cam, ids=ids, ref=ref, ref_env=ref_env)
    return _SIX


def test_six_envs_against_float64():
    _need_gpu()
    s = _six_envs()
    depth, seg, rgba, env = _world(s["sc"], [s["cam"]], s["ids"], s["off"])
    assert len(set(s["ref_env"].ravel()) - {-1}) == 6                      # every env is in view
    assert (s["ref"][1] == 0).sum() > 100                                   # and so is the ground
    wr.compare(depth[0], seg[0], rgba[0], s["ref"], env[0], s["ref_env"])


def test_composite_of_per_env_cameras():
    """The same image from what existed before: one shf_render_cameras camera per env, shifted by minus the env's offset,
    composited by nearest depth (ties: the earlier env).  Different kernels, so the acceptance criterion, not equality;
    whether they are in fact bit-equal is printed."""
    _need_gpu()
    from shifu_amd.render import camera_struct
    s = _six_envs()
    sc, off, (cp, cq) = s["sc"], s["off"], s["cam"]
    dev = torch.device("cuda:0")
    r = _renderer(sc)
    bs, seg, col = _tables(sc)
    pose = torch.tensor(np.array([np.concatenate([cp - off[e], cq]) for e in range(sc.E)]), dtype=torch.float32, device=dev)
    d = torch.empty(sc.E, H, W, device=dev)
    g = torch.empty(sc.E, H, W, dtype=torch.int32, device=dev)
    c = torch.empty(sc.E, H, W, 4, dtype=torch.uint8, device=dev)
    r.render(bs, pose, seg, col, camera_struct(W, H, FOV, NEAR, FAR), depth=d, seg_out=g, rgba=c)
    torch.cuda.synchronize()
    d, g, c = d.cpu().numpy(), g.cpu().numpy(), c.cpu().numpy()
    first = d.argmin(0)                                                     # (argmin takes the first of equal depths)
    pick = lambda a: np.take_along_axis(a, first.reshape((1, H, W) + (1,) * (a.ndim - 3)), 0)[0]
    cd, cg, cc = pick(d), pick(g), pick(c)
    depth, segw, rgba, env = _world(sc, [s["cam"]], s["ids"], off, r=r)
    equal = {k: bool(np.array_equal(a, b)) for k, a, b in (("depth", depth[0], cd), ("seg", segw[0], cg), ("rgba", rgba[0], cc))}
    print("bit-equal to the composite:", equal, "-- depth differs in", int((depth[0] != cd).sum()), "pixels")
    # the criterion with the composite as the reference image (facet edges and incidence: the float64 reference's)
    comp = (cd, np.where(np.isfinite(cd), cg, -1), cc[..., :3], s["ref"][3], s["ref"][4])
    wr.compare(depth[0], segw[0], rgba[0], comp)


# ---- 3: chunk and flush edges ----------------------------------------------------------------------------------------------
_CHUNK_ENVS = _abi.RENDER_WORLD_CHUNK // 4       # envs per pass with the four shapes of these scenes


@pytest.mark.parametrize("E", [1, 3, 4, 5, _CHUNK_ENVS + 1])
def test_env_counts_around_a_pass(E):
    _need_gpu()
    sc, off = _spread_scene(E, seed=30 + E)
    cam = _overview()
    ref, ref_env = wr.reference(sc, range(E), off, cam, NEAR, FAR)
    depth, seg, rgba, env = _world(sc, [cam], None, off)
    wr.compare(depth[0], seg[0], rgba[0], ref, env[0], ref_env)


def test_more_candidates_in_one_tile_than_the_list_holds_twice_over():
    """A corridor of envs along the central ray of tile (1, 0): every shape's centre projects into that tile, so its
    workgroup lists them all -- more than twice SHF_RENDER_WORLD_LIST records, at least two flushes before the last."""
    _need_gpu()
    from shifu_amd.render import camera_basis, lookat_quat
    cap = _abi.RENDER_WORLD_LIST
    E = 2 * cap // 4 + 40
    sc = wr.Scene(E, seed=5, low=(-0.05, -0.05, -0.05), high=(0.05, 0.05, 0.05))
    eye = np.array([0.0, 0.0, 1.5])
    q = lookat_quat(eye, [4.0, 0.0, 1.0])
    fwd, right, up = camera_basis(q)
    t = np.tan(np.radians(FOV / 2))
    axis = fwd + up * (0.5 * t * H / W)                                       # through pixel corner (24, 8): the centre of tile (1, 0)
    dist = np.linspace(1.5, 3.5, E)
    lat = sc.rng.uniform(-0.08, 0.08, (E, 2)) * dist[:, None]
    off = eye + dist[:, None] * axis + lat[:, :1] * right + lat[:, 1:] * up
    # count the shape centres that project inside the tile's pixels: those are candidates whatever the cull's slack
    inside = 0
    for e in range(E):
        for p, _ in sc.poses[e]:
            v = p + off[e] - eye
            z = v @ fwd
            col, row = ((v @ right) / (z * t) + 1) * W / 2, (1 - (v @ up) / (z * t * H / W)) * H / 2
            inside += int(16 <= col < 32 and 0 <= row < 16)
    assert inside > 2 * cap
    ref, ref_env = wr.reference(sc, range(E), off, (eye, q), NEAR, FAR)
    assert len(set(ref_env.ravel()) - {-1}) > 20
    depth, seg, rgba, env = _world(sc, [(eye, q)], None, off)
    wr.compare(depth[0], seg[0], rgba[0], ref, env[0], ref_env)


# ---- 4: partial tiles ----------------------------------------------------------------------------------------------------------
def test_partial_tiles():
    _need_gpu()
    sc, off = _spread_scene(5, seed=44)
    cam = _overview()
    ref, ref_env = wr.reference(sc, range(5), off, cam, NEAR, FAR, W_=40, H_=24)
    depth, seg, rgba, env = _world(sc, [cam], None, off, W_=40, H_=24)
    assert depth.shape == (1, 24, 40)
    wr.compare(depth[0], seg[0], rgba[0], ref, env[0], ref_env)


# ---- 5: the kernel against itself, bit for bit ----------------------------------------------------------------------------------
def test_permuting_the_list_changes_nothing_but_follows_in_env_out():
    _need_gpu()
    E = 9
    sc, off = _spread_scene(E, seed=51)              # random poses: no two surfaces at exactly the same depth
    cam = _overview()
    base = _world(sc, [cam], list(range(E)), off)
    perm = np.random.default_rng(1).permutation(E)
    # the same envs at the same places, listed in another order ...
    listed = _world(sc, [cam], list(perm), off[perm])
    for a, b in zip(base, listed):
        np.testing.assert_array_equal(a, b)
    # ... and other envs at those places: env_out follows
    moved = _world(sc, [cam], list(perm), off)
    sc2 = wr.Scene(E, seed=51)
    sc2.poses, sc2.seg, sc2.col = [sc.poses[i] for i in perm], sc.seg[perm], sc.col[perm]
    want = _world(sc2, [cam], None, off)
    for k in range(3):
        np.testing.assert_array_equal(moved[k], want[k])
    np.testing.assert_array_equal(moved[3], np.where(want[3] >= 0, perm[np.maximum(want[3], 0)], -1))


def test_env_level_cull_with_a_true_bound_changes_nothing():
    _need_gpu()
    E = 40
    sc, off = _spread_scene(E, seed=52)
    off[:, 0] = sc.rng.uniform(-6.0, 8.0, E)         # some envs behind the camera and off to the sides: culled as a whole
    off[:, 1] = sc.rng.uniform(-8.0, 8.0, E)
    cam = _overview()
    plain = _world(sc, [cam], None, off)
    culled = _world(sc, [cam], None, off, env_radius=sc.true_env_radius())
    for a, b in zip(plain, culled):
        np.testing.assert_array_equal(a, b)
    assert len(set(plain[3].ravel()) - {-1}) >= 5


def test_two_views_equal_two_launches():
    _need_gpu()
    sc, off = _spread_scene(7, seed=53)
    cams = [_overview(), _overview(eye=(4.5, 2.5, 1.5))]
    both = _world(sc, cams, None, off)
    for v, cam in enumerate(cams):
        one = _world(sc, [cam], None, off)
        for a, b in zip(both, one):
            np.testing.assert_array_equal(a[v], b[0])
    assert not np.array_equal(both[0][0], both[0][1])


def test_a_sublist_equals_a_scene_of_those_envs_alone():
    _need_gpu()
    sc, off = _spread_scene(7, seed=54)
    cam = _overview()
    sub = [5, 2]
    got = _world(sc, [cam], sub, off[:2])
    small = wr.Scene(2, seed=54)
    small.poses, small.seg, small.col = [sc.poses[i] for i in sub], sc.seg[sub], sc.col[sub]
    want = _world(small, [cam], None, off[:2])
    for k in range(3):
        np.testing.assert_array_equal(got[k], want[k])
    np.testing.assert_array_equal(got[3], np.where(want[3] >= 0, np.array(sub)[np.maximum(want[3], 0)], -1))
    assert set(got[3].ravel()) == {-1, 2, 5}


# ---- 6: the tie rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [[0, 1], [1, 0]])
def test_equal_depth_shows_the_earlier_list_position(order):
    _need_gpu()
    sc = wr.Scene(2, seed=61)
    sc.poses[1] = sc.poses[0]                        # two envs, identical poses and offsets: every hit is a tie
    off = np.array([[0.8, 0.0, 0.0]] * 2)
    depth, seg, rgba, env = _world(sc, [_overview()], order, off)
    hit = seg[0] > 0
    assert hit.sum() > 50
    assert (env[0][hit] == order[0]).all() and (env[0][~hit] == -1).all()
    assert set(seg[0][hit]) <= set(sc.seg[order[0]])


# ---- 7: terrains -------------------------------------------------------------------------------------------------------------------------
def test_three_envs_on_a_height_field():
    """The small height field of tests/test_gpu_camera.py, cast once and not displaced; envs placed at different origins by
    their own states (the A1 layout) and, for one of them, by an offset as well."""
    _need_gpu()
    from tests import test_gpu_camera as tc
    t, hs = tc._heightfield()
    sc = wr.Scene(3, seed=71, low=(-0.3, -0.3, 0.35), high=(0.3, 0.3, 0.8))
    origins = np.array([[-0.6, -0.5, 0.0], [0.5, 0.4, 0.0], [0.0, 0.0, 0.0]])
    sc.poses = [[(p + origins[e], q) for p, q in env] for e, env in enumerate(sc.poses)]
    off = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, -0.7, 0.1]])
    from shifu_amd.render import lookat_quat
    eye = np.array([-1.6, -0.2, 1.6])
    cam = (eye, lookat_quat(eye, [0.1, 0.0, 0.2]))
    ref, ref_env = wr.reference(sc, range(3), off, cam, NEAR, 6.0, ground=(hs, t.hscale, t.vscale, t.border))
    assert len(set(ref_env.ravel()) - {-1}) == 3 and (ref[1] == 0).sum() > 300
    depth, seg, rgba, env = _world(sc, [cam], None, off, r=_renderer(sc, t, hs), far=6.0)
    wr.compare(depth[0], seg[0], rgba[0], ref, env[0], ref_env)


def test_two_envs_on_the_warped_trimesh():
    """k_render_world_tw on the riser fixture of tests/trimesh_render_ref.py with its own comparison."""
    _need_gpu()
    from shifu_amd.isaacgym.terrain_utils import trimesh_warp_map
    from tests import render_ref as rr
    from tests import trimesh_render_ref as tr
    hs = tr.fixture_samples()
    warp = trimesh_warp_map(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD)
    t = _abi.ShfTerrain()
    t.rows, t.cols = hs.shape
    t.hscale, t.vscale, t.border, t.warped = tr.HSCALE, tr.VSCALE, tr.BORDER, 1
    sc = wr.Scene(2, seed=72, low=(-0.5, -0.5, 0.6), high=(0.5, 0.5, 1.0))
    off = np.array([[0.0, 0.0, 0.0], [0.4, -0.3, 0.0]])
    cam = tr.fixture_cameras()[0]
    tri = tr.mesh_triangles(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD, tr.BORDER)
    ref, amb = tr.render(wr.ref_shapes(sc, range(2), off), tri, cam[0], cam[1], W, H, FOV, 0.1, 4.0)
    depth, seg, rgba, env = _world(sc, [cam], None, off, r=_renderer(sc, t, hs, warp), near=0.1, far=4.0)
    bad, masked = tr.compare(depth[0], seg[0], rgba[0], ref, amb, extra_mask=rr.silhouette_adjacent(ref[1]))
    print(f"{bad} mismatching, {masked} ambiguous of {W * H} pixels; {int((ref[1] > 0).sum())} on shapes")
    assert masked <= 0.005 * W * H and bad <= 0.005 * W * H
    assert ((env[0] >= 0) == (seg[0] > 0)).all()


# ---- 8: the fused envs ----------------------------------------------------------------------------------------------------------------
def test_a1_viewer_sees_every_env():
    _need_gpu()
    from shifu_amd.gym.a1_fused import FusedA1Env, default_terrain_cfg
    env = FusedA1Env(num_envs=8, terrain_cfg=default_terrain_cfg(num_rows=1, num_cols=2, border_size=1, terrain_length=6.,
                                                                 terrain_width=6.))
    v = env.add_viewer(128, 128, 90.0, 0.05, 100.0)
    assert v.layout == "world" and 0.45 < v.env_radius < 1.2
    env.reset()
    B = env.cam_seg.shape[1]
    trunks = env.body_state.view(8, B, 13)[:, 0, :3].cpu().numpy()
    centre = trunks.mean(0)
    extent = np.abs(trunks - centre)[:, :2].max()
    v.look_at(centre + [0.0, -0.01, extent + 2.0], centre)                   # from above: fov 90 shows +- its height
    im = v.draw()
    torch.cuda.synchronize()
    assert set(im) == {"rgba", "depth", "seg", "env"} and im["rgba"].shape == (128, 128, 4)
    seen = set(im["env"].unique().cpu().tolist())
    assert seen == {-1} | set(range(8)), seen
    assert v.draw()["env"].data_ptr() == im["env"].data_ptr()               # preallocated: the same tensors at every draw
    env.destroy()


def test_abb_viewer_lays_the_envs_out_on_a_grid():
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from shifu_amd.render import camera_basis
    env = FusedAbbEnv(num_envs=4, seed=3)
    v = env.add_viewer(160, 160, 60.0, 0.05, 20.0, spacing=2.0, per_row=2)
    assert v.layout == "grid" and v.env_radius == 0.0
    np.testing.assert_array_equal(v.offsets, [[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0]])
    env.reset()
    eye = np.array([1.0, 0.99, 4.0])
    v.look_at(eye, [1.0, 1.0, 0.0])
    im = v.draw()
    torch.cuda.synchronize()
    B, nb = env.cam_seg.shape[1], int(env.cm.blob.nb)
    cube = env.body_state.view(4, B, 13)[:, nb + int(env.task_params.cube_actor) - 1, :3].cpu().numpy()
    fwd, right, up = camera_basis(v._pose[3:])
    t = np.tan(np.radians(30.0))
    e_img = im["env"].cpu().numpy()
    for k in range(4):
        p = cube[k] + v.offsets[k] - eye
        z = p @ fwd
        col, row = int(((p @ right) / (z * t) + 1) * 80), int((1 - (p @ up) / (z * t)) * 80)
        assert e_img[row, col] == k, (k, row, col, e_img[row, col])
    assert set(np.unique(e_img)) == {-1, 0, 1, 2, 3}
    env.destroy()


def test_a_draw_replayed_from_a_graph_equals_the_eager_one():
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    env = FusedAbbEnv(num_envs=4, seed=3)
    v = env.add_viewer(W, H, 70.0, 0.05, 20.0)
    env.reset()
    v.follow(0, body=0, offset=(2.5, 2.0, 2.5))
    eager = {k: t.clone() for k, t in v.draw().items()}
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        v.draw()                                     # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        v.draw()
    for t in v.images.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k, t in v.images.items():
        assert torch.equal(t, eager[k]), k
    assert int((eager["env"] >= 0).sum()) > 20 and float(v.pose()[2]) > 2.0
    env.destroy()


# ---- 9: the recorder ----------------------------------------------------------------------------------------------------------------------
def test_recorded_frames_come_back_from_disk_byte_for_byte(tmp_path):
    _need_gpu()
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    from shifu_amd.viewer import FrameRecorder
    from tests import test_viewer_host as th
    env = FusedAbbEnv(num_envs=4, seed=3)
    v = env.add_viewer(W, H, 70.0, 0.05, 20.0)
    env.reset()
    v.look_at([3.5, -1.5, 2.5], [1.0, 1.0, 0.2])
    rec = FrameRecorder(v, 3)
    g = torch.Generator().manual_seed(2)
    kept = []
    for k in range(3):
        if k:
            env.step((2 * torch.rand(4, 3, generator=g) - 1).to(env.device))
        kept.append(v.draw()["rgba"].clone())
        rec.record()
    with pytest.raises(RuntimeError, match="frames are taken"):
        rec.record()
    paths = rec.save(tmp_path / "frames", apng="all.png")
    assert [p.split("/")[-1] for p in paths] == ["frame_000000.png", "frame_000001.png", "frame_000002.png", "all.png"]
    for p, want in zip(paths[:3], kept):
        np.testing.assert_array_equal(th._decode_png(p), want.cpu().numpy())
    assert not torch.equal(kept[0], kept[2])                                 # the arm moved between the frames
    assert [k for k, _ in th._chunks(open(paths[3], "rb").read())].count(b"fcTL") == 3
    env.destroy()


# ---- the facade, opted in ---------------------------------------------------------------------------------------------------------------
def test_facade_viewer_draws_the_grid_and_writes_frames(monkeypatch, tmp_path):
    """SHIFU_AMD_VIEWER set: a viewer made before prepare_sim builds its device state at the first draw, shows every env on
    create_env's grid, write_viewer_image_to_file writes what was drawn, and IsaacGymEnv.render() numbers its frames."""
    _need_gpu()
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.isaacgym import gymapi
    from tests import test_viewer_host as th
    monkeypatch.setenv("SHIFU_AMD_VIEWER", str(tmp_path / "frames"))
    gym, sim, envs = th._facade_scene(n=4, spacing=1.0, per_row=2)
    props = gymapi.CameraProperties()
    props.width, props.height, props.horizontal_fov = 96, 64, 70.0
    v = gym.create_viewer(sim, props)
    gym.prepare_sim(sim)
    gym.simulate(sim)
    gym.viewer_camera_look_at(v, None, gymapi.Vec3(1.0, -3.0, 4.0), gymapi.Vec3(1.0, 1.0, 0.3))
    gym.draw_viewer(v, sim, True)
    torch.cuda.synchronize()
    assert set(v.images["env"].unique().cpu().tolist()) == {-1, 0, 1, 2, 3}
    gym.write_viewer_image_to_file(v, str(tmp_path / "one.png"))
    np.testing.assert_array_equal(th._decode_png(tmp_path / "one.png"), v.images["rgba"].cpu().numpy())
    env = object.__new__(IsaacGymEnv)
    env.viewer, env.gym, env.sim, env._viewer_frame = v, gym, sim, 0
    env.render()
    gym.simulate(sim)
    env.render()
    import os
    assert sorted(os.listdir(tmp_path / "frames")) == ["frame_000000.png", "frame_000001.png"]
    np.testing.assert_array_equal(th._decode_png(tmp_path / "frames" / "frame_000001.png"), v.images["rgba"].cpu().numpy())
    gym.destroy_sim(sim)
