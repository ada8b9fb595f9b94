"""Independent float64 checker for the camera ray caster on a warped trimesh terrain (csrc/shf_render.hip, k_render_cameras_tw):
brute force over every triangle `vertices[triangles]` of terrain_utils.convert_heightfield_to_trimesh -- no cell walk, no
vertex bytes.  A pixel shows the nearest FRONT face (the side of (v1 - v0) x (v2 - v0)) entered at a view depth in
[near, far]; triangles of zero area are skipped.  Shapes come from tests/render_ref.py and are merged by nearest depth.

Besides the images the caster returns an ambiguity mask: pixels whose ray meets some front-facing triangle, at a depth in
[near, far] no more than 1e-3 behind the nearest hit, within 1e-4 of one of its edges in barycentric coordinates (inside
or outside).  Those rays graze an edge or just miss an occluder, where float32 may fall either way."""
import numpy as np

from tests import render_ref as rr

ZERO_AREA = 1e-8          # |(v1 - v0) x (v2 - v0)| in m^2 below which a triangle has collapsed (the smallest real one: 5e-4)
AMBIGUOUS_BARY, AMBIGUOUS_DEPTH = 1e-4, 1e-3


def mesh_triangles(samples, hscale, vscale, slope_threshold, border):
    """(T, 3, 3) float64 corners of the mesh convert_heightfield_to_trimesh makes, moved by -border in x and y."""
    from shifu_amd.isaacgym.terrain_utils import convert_heightfield_to_trimesh
    v, t = convert_heightfield_to_trimesh(np.asarray(samples), hscale, vscale, slope_threshold)
    tri = v.astype(np.float64)[t.astype(np.int64)]
    tri[..., :2] -= border
    return tri


def triangle_classes(tri):
    """(zero_area, vertical) masks over (T, 3, 3) triangles: collapsed ones, and risers (no extent in the horizontal plane)."""
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    zero = np.linalg.norm(n, axis=1) < ZERO_AREA
    return zero, ~zero & (np.abs(n[:, 2]) < ZERO_AREA)


def entry_triangles(o, d, tri, near, far):
    """Rays o (3,), d (R, 3) against (T, 3, 3) triangles: nearest front-face entry s (R,) (inf: none) in [near, far], its
    unit normal (R, 3), triangle index (R,) and the ambiguity mask (R,)."""
    o, d, tri = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(tri, np.float64)
    zero, _ = triangle_classes(tri)
    tri = tri[~zero]
    index = np.nonzero(~zero)[0]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    c = np.cross(e1, e2)
    nrm = c / np.linalg.norm(c, axis=1, keepdims=True)
    dn = d @ c.T                                              # (R, T)
    front = dn < 0
    with np.errstate(divide="ignore", invalid="ignore"):
        s = ((v0 - o) * c).sum(1)[None, :] / dn
        q = o[None, None, :] + s[..., None] * d[:, None, :] - v0[None]          # hit point relative to v0
        cc = (c * c).sum(1)
        v = np.einsum("rtk,tk->rt", np.cross(q, e2[None]), c) / cc              # weight of v1
        w = np.einsum("rtk,tk->rt", np.cross(e1[None], q), c) / cc              # weight of v2
    m = np.minimum(np.minimum(v, w), 1.0 - v - w)
    in_range = front & (s >= near) & (s <= far)
    hit = np.where(in_range & (m >= 0), s, np.inf)
    j = hit.argmin(1)
    R = np.arange(len(d))
    best = hit[R, j]
    amb = (in_range & (np.abs(m) <= AMBIGUOUS_BARY) & (s <= best[:, None] + AMBIGUOUS_DEPTH)).any(1)
    return best, nrm[j], index[j], amb


def render(shapes, tri, cam_pos, cam_quat, W, H, hfov, near, far, ground_color=(0.5, 0.5, 0.5)):
    """The tuple of render_ref.render(..., facets=True) -- depth, id (-1 nothing, 0 terrain), rgb, facet, cos -- for shapes
    over the mesh `tri`, and the (H, W) ambiguity mask of the terrain."""
    depth, ids, rgb, facet, cos = (a.copy() for a in rr.render(shapes, cam_pos, cam_quat, W, H, hfov, near, far, ground=None,
                                                               facets=True))
    o, d = rr.rays(cam_pos, cam_quat, W, H, hfov)
    s, n, j, amb = entry_triangles(o, d, tri, near, far)
    s, n, j, amb = s.reshape(H, W), n.reshape(H, W, 3), j.reshape(H, W), amb.reshape(H, W)
    t = s < depth
    lam = rr.AMBIENT + rr.DIFFUSE * np.maximum(n @ rr.LIGHT, 0.0)
    shaded = np.floor(np.clip(np.asarray(ground_color, float)[None, None, :] * lam[..., None], 0, 1) * 255 + 0.5).astype(np.uint8)
    dl = d.reshape(H, W, 3)
    tcos = np.abs((n * dl).sum(-1)) / np.linalg.norm(dl, axis=-1)
    depth[t], ids[t], rgb[t], facet[t], cos[t] = s[t], 0, shaded[t], j[t], tcos[t]
    return (depth, ids, rgb, facet, cos), amb


def visible_triangles(tri, cam_pos, cam_quat, W, H, hfov, far, reach=0.3):
    """The triangles of `tri` a camera can see at all: those with a corner at a view depth below far + reach (depth is the
    distance along the view axis: towards the image corners a surface at depth `far` is up to 1.5 x as far away, so a
    sphere of radius far + reach around the camera would drop visible triangles), minus those whose three corners all lie
    outside one and the same side plane of the view frustum.  No ray of the image reaches a triangle left out, so the
    images are those of the whole mesh; it keeps the brute force small."""
    R = rr.qmat(cam_quat)
    rel = np.asarray(tri, np.float64) - np.asarray(cam_pos, float)
    x, y, z = -(rel @ R[:, 1]), rel @ R[:, 2], rel @ R[:, 0]                      # right, up, forward: (T, 3) each
    t = np.tan(np.radians(hfov) / 2)
    ty = t * H / W
    near_enough = (z <= far + reach).any(1)
    outside = (z <= 0).all(1) | (x > t * z).all(1) | (x < -t * z).all(1) | (y > ty * z).all(1) | (y < -ty * z).all(1)
    return tri[near_enough & ~outside]


def world_shapes(render_shapes, body_rows, seg, color):
    """render_ref shape dicts of one env: model.RenderShape records placed by the env's body states body_rows (B, >= 7:
    pos, quat xyzw), with the rows' segmentation ids seg (B,) and colors color (B, 3)."""
    out = []
    for s in render_shapes:
        p, q = np.asarray(body_rows[s.body][:3], float), np.asarray(body_rows[s.body][3:7], float)
        Rb = rr.qmat(q)
        d = dict(kind={"hull": "poly"}.get(s.kind, s.kind), pos=p + Rb @ s.pos, rot=Rb @ s.rot, seg=int(seg[s.body]),
                 color=np.asarray(color[s.body], float))
        if s.kind == "box":
            d["half"] = 0.5 * np.asarray(s.size, float)
        elif s.kind == "sphere":
            d["r"] = float(s.size[0])
        elif s.kind == "capsule":
            d["r"], d["hl"] = float(s.size[0]), 0.5 * float(s.size[1])
        else:
            d["planes"] = np.asarray(s.poly["planes"], float)
        out.append(d)
    return out


def compare(depth, seg, rgba, ref, amb, extra_mask=None):
    """The bounds of tests/test_gpu_camera.py's _compare with the ambiguity mask in the place of the silhouette mask: hit / miss
    and segmentation equal outside the mask; depth within 1e-4 + 1e-6 s / cos(incidence) where they agree; RGB within 1 LSB
    away from the reference's facet edges; alpha 255; the mask and the mismatches each cover at most 0.5 % of the pixels.
    Returns (mismatching pixels, masked pixels)."""
    rd, rid, rrgb, rfacet, rcos = ref
    mask = amb if extra_mask is None else amb | extra_mask
    got_id = np.where(np.isfinite(depth), seg, -1)
    bad = got_id != rid
    assert not (bad & ~mask).any(), f"{int((bad & ~mask).sum())} id mismatches outside the ambiguity mask"
    assert amb.mean() <= 0.005, f"the ambiguity mask covers {amb.mean():.4f} of the pixels"
    assert bad.mean() <= 0.005, f"{bad.mean():.4f} of the pixels differ"
    ok = ~bad & np.isfinite(rd)
    err = np.abs(depth[ok] - rd[ok])
    tol = 1e-4 + 1e-6 * rd[ok] / np.maximum(rcos[ok], 1e-6)
    assert (err <= tol).all(), f"depth off by {err.max():.3g} m"
    assert (err > 1e-4).mean() <= 0.001
    diff = np.abs(rgba[..., :3].astype(int) - rrgb.astype(int)).max(-1)
    shade_ok = ~bad & ~rr.silhouette_adjacent(rfacet)
    assert diff[shade_ok].max(initial=0) <= 1, f"RGB off by {diff[shade_ok].max()} LSB"
    assert (diff[~bad] > 1).mean() <= 0.002
    assert (rgba[..., 3] == 255).all()
    return int(bad.sum()), int(amb.sum())


# ---- the fixture: pyramid stairs with noise, as a warped mesh with risers ----------------------------------------------
HSCALE, VSCALE, SLOPE_THRESHOLD, BORDER = 0.1, 0.005, 0.75, 1.15
CAM_W, CAM_H, CAM_FOV, CAM_NEAR, CAM_FAR = 64, 48, 87.0, 0.05, 6.0
CAMERAS = [((-1.0, -0.9, 1.2), (0.0, 0.0, 0.2)), ((-0.95, 0.05, 0.33), (0.5, 0.0, 0.25)),
           ((0.03, 0.02, 1.5), (0.03, 0.021, 0.0)), ((0.9, -1.0, 0.45), (-0.2, 0.3, 0.3))]


def fixture_samples():
    from shifu_amd.isaacgym.terrain_utils import SubTerrain, pyramid_stairs_terrain, random_uniform_terrain
    np.random.seed(3)
    t = SubTerrain(width=24, length=24, vertical_scale=VSCALE, horizontal_scale=HSCALE)
    pyramid_stairs_terrain(t, step_width=0.3, step_height=0.12, platform_size=0.6)
    random_uniform_terrain(t, -0.02, 0.02, 0.005, downsampled_scale=0.2)
    return np.ascontiguousarray(t.height_field_raw, np.int16)


def fixture_cameras():
    from shifu_amd.render import lookat_quat
    return [(np.array(p, float), lookat_quat(p, a)) for p, a in CAMERAS]


_FIXTURE_REF = {}


def fixture_reference():
    """Per camera: (reference tuple, ambiguity mask) of the bare fixture -- computed once per process, not to be modified."""
    if not _FIXTURE_REF:
        tri = mesh_triangles(fixture_samples(), HSCALE, VSCALE, SLOPE_THRESHOLD, BORDER)
        _FIXTURE_REF["tri"] = tri
        _FIXTURE_REF["ref"] = [render([], tri, p, q, CAM_W, CAM_H, CAM_FOV, CAM_NEAR, CAM_FAR) for p, q in fixture_cameras()]
    return _FIXTURE_REF["tri"], _FIXTURE_REF["ref"]
