"""The camera ray caster on a warped trimesh terrain (csrc/shf_render.hip, k_render_cameras_tw) against the float64 brute
force of tests/trimesh_render_ref.py: the riser fixture alone, shapes above it, an unshifted mesh (all vertex bytes
zero shifts), batch independence -- and the height-field / plane path, which must render what it rendered before."""
import hashlib

import numpy as np
import pytest

from shifu_amd import _abi
from tests import test_gpu_camera as tc
from tests import trimesh_render_ref as tr

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _terrain(hs, hscale, vscale, border):
    t = _abi.ShfTerrain()
    t.rows, t.cols = hs.shape
    t.hscale, t.vscale, t.border = hscale, vscale, border
    t.warped = 1
    return t


def _render_warped(defs, poses, cams, seg, col, terrain, hs, warp, nb=None, W=tr.CAM_W, H=tr.CAM_H, fov=tr.CAM_FOV,
                   near=tr.CAM_NEAR, far=tr.CAM_FAR, packed=False):
    """tests/test_gpu_camera.py's _render with a warped terrain: samples + warp bytes, or (packed) the sim's payload."""
    from shifu_amd.isaacgym.terrain_utils import pack_trimesh_samples
    from shifu_amd.render import Renderer, build_scene, camera_struct
    n = len(cams)
    nb = max(len(defs), 1) if nb is None else nb
    sc = build_scene(defs, nb, ground=True, height_samples=hs, vscale=terrain.vscale)
    if packed:
        r = Renderer(sc, terrain, torch.from_numpy(pack_trimesh_samples(hs, warp)).to("cuda:0"), "cuda:0")
    else:
        r = Renderer(sc, terrain, hs, "cuda:0", warp=warp)
    bs = torch.zeros(n * nb, 13)
    bs[:, 6] = 1.0
    for e in range(n):
        for k, (p, q) in enumerate(poses[e]):
            bs[e * nb + k, :3] = torch.tensor(p)
            bs[e * nb + k, 3:7] = torch.tensor(q)
    cam = torch.tensor(np.array([np.concatenate([p, q]) for p, q in cams]), dtype=torch.float32)
    dev = torch.device("cuda:0")
    depth = torch.empty(n, H, W, device=dev)
    segi = torch.empty(n, H, W, dtype=torch.int32, device=dev)
    rgba = torch.empty(n, H, W, 4, dtype=torch.uint8, device=dev)
    seg = np.zeros((n, nb), np.int32) if seg is None else np.asarray(seg)
    col = np.full((n, nb, 3), 0.8, np.float32) if col is None else np.asarray(col)
    r.render(bs.to(dev), cam.to(dev), torch.as_tensor(seg, dtype=torch.int32).to(dev).contiguous(),
             torch.as_tensor(col, dtype=torch.float32).to(dev).contiguous(), camera_struct(W, H, fov, near, far),
             depth=depth, seg_out=segi, rgba=rgba)
    torch.cuda.synchronize()
    return depth.cpu().numpy(), segi.cpu().numpy(), rgba.cpu().numpy()


def _fixture():
    from shifu_amd.isaacgym.terrain_utils import trimesh_warp_map
    hs = tr.fixture_samples()
    return hs, trimesh_warp_map(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD), _terrain(hs, tr.HSCALE, tr.VSCALE, tr.BORDER)


def test_warped_terrain_alone_against_the_brute_force():
    """The four fixture cameras as four envs: stairs with vertical risers (183 / 1535 / 0 / 622 riser pixels), noise on the
    treads, 34 collapsed triangles."""
    tc._need_gpu()
    hs, warp, t = _fixture()
    assert t.warped == 1 and (warp & 0xF != 5).any()
    cams = tr.fixture_cameras()
    depth, seg, rgba = _render_warped([], [[] for _ in cams], cams, None, None, t, hs, warp)
    assert np.isfinite(depth).sum() > 5000 and not np.isnan(depth).any()
    _, refs = tr.fixture_reference()
    bad = masked = 0
    for e, (ref, amb) in enumerate(refs):
        b, m = tr.compare(depth[e], seg[e], rgba[e], ref, amb)
        print(f"camera {e}: {b} mismatching, {m} ambiguous pixels")
        bad, masked = bad + b, masked + m
    npx = len(cams) * tr.CAM_W * tr.CAM_H
    assert masked <= 0.005 * npx and bad <= 0.005 * npx


def test_shapes_above_the_warped_terrain_against_the_brute_force():
    """The mixed shapes of the height-field test (box, sphere, capsule, hull) over the riser fixture."""
    tc._need_gpu()
    from tests import render_ref as rr
    n, W, H, FOV = 8, tc.W, tc.H, tc.FOV
    defs, poses, cams, seg, col = tc._mixed_scene(n)
    lift = np.array([0.0, 0.0, 0.4])                          # the fixture's platform is 0.36 m high: shapes and cameras go up
    poses = [[(p + lift, q) for p, q in env] for env in poses]
    cams = [(p + lift, q) for p, q in cams]
    hs, warp, t = _fixture()
    depth, sg, rgba = _render_warped(defs, poses, cams, seg, col, t, hs, warp, W=W, H=H, fov=FOV, near=0.1, far=4.0)
    tri, _ = tr.fixture_reference()
    bad = masked = shape_px = 0
    for e in range(n):
        ref, amb = tr.render(tc._ref_shapes(defs, poses[e], seg[e], col[e]), tri, cams[e][0], cams[e][1], W, H, FOV, 0.1, 4.0)
        b, m = tr.compare(depth[e], sg[e], rgba[e], ref, amb, extra_mask=rr.silhouette_adjacent(ref[1]))
        bad, masked, shape_px = bad + b, masked + m, shape_px + int((ref[1] > 0).sum())
    print(f"{bad} mismatching, {masked} ambiguous of {n * W * H} pixels; {shape_px} on shapes")
    assert shape_px > 300
    assert masked <= 0.005 * n * W * H and bad <= 0.005 * n * W * H


def test_unshifted_mesh_against_its_triangles():
    """All shifts zero: the warped path draws the grid split along (i, j)-(i+1, j+1) -- not the height field's diagonal --
    so the reference is the triangles.  Also the packed-payload form of Renderer, and odd grid sizes."""
    tc._need_gpu()
    from shifu_amd.isaacgym.terrain_utils import SubTerrain, random_uniform_terrain, trimesh_warp_map
    np.random.seed(5)
    st = SubTerrain(width=21, length=17, vertical_scale=0.005, horizontal_scale=0.1)
    random_uniform_terrain(st, -0.1, 0.1, 0.005, downsampled_scale=0.2)
    hs = np.ascontiguousarray(st.height_field_raw, np.int16)
    warp = trimesh_warp_map(hs, 0.1, 0.005, None)
    assert (warp == 5).all()                                      # dx = dy = 0, no hint bits
    border = 0.8
    t = _terrain(hs, 0.1, 0.005, border)
    cams = tr.fixture_cameras()
    depth, seg, rgba = _render_warped([], [[] for _ in cams], cams, None, None, t, hs, warp, packed=True)
    tri = tr.mesh_triangles(hs, 0.1, 0.005, None, border)
    hits = 0
    for e, (p, q) in enumerate(cams):
        ref, amb = tr.render([], tri, p, q, tr.CAM_W, tr.CAM_H, tr.CAM_FOV, tr.CAM_NEAR, tr.CAM_FAR)
        tr.compare(depth[e], seg[e], rgba[e], ref, amb)
        hits += int(np.isfinite(ref[0]).sum())
    assert hits > 3000


def test_batch_independence_on_the_warped_terrain():
    tc._need_gpu()
    n = 12
    defs, poses, cams, seg, col = tc._mixed_scene(n, seed=9)
    hs, warp, t = _fixture()
    kw = dict(W=tc.W, H=tc.H, fov=tc.FOV, near=0.1, far=4.0)
    full = _render_warped(defs, poses, cams, seg, col, t, hs, warp, **kw)
    perm = np.random.default_rng(0).permutation(n)
    pick = lambda xs: [xs[i] for i in perm]
    permuted = _render_warped(defs, pick(poses), pick(cams), pick(seg), pick(col), t, hs, warp, **kw)
    for a, b in zip(full, permuted):
        np.testing.assert_array_equal(a[perm], b)


# sha256 over depth, segmentation and rgba of unchanged_digest()'s scenes, rendered by the height-field-only kernel before the
# trimesh kernel existed (recorded once on that commit)
UNCHANGED_DIGEST = "f5fd7afc847737fbeb4f42a2d140458639b47687700994bb972cb42a9ce10d81"


def unchanged_digest():
    """Eight envs of the mixed scene on the height field, and eight on the plane: warped = 0, the entry as it always was."""
    n = 8
    defs, poses, cams, seg, col = tc._mixed_scene(n, seed=21)
    t, hs = tc._heightfield()
    h = hashlib.sha256()
    for images in (tc._render(defs, poses, cams, seg, col, terrain=t, heights=hs), tc._render(defs, poses, cams, seg, col)):
        for a in images:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def test_height_field_and_plane_render_what_they_did():
    tc._need_gpu()
    assert unchanged_digest() == UNCHANGED_DIGEST
