"""Independent float64 checker for the camera ray caster (csrc/shf_render.hip): brute force per pixel, numpy only.

Written from the conventions of DESIGN.md "Camera sensors", not from the kernel: every shape is tested against every
pixel ray; the height field against every one of its triangles (no cell walk).  A pixel shows the nearest surface
ENTERED (front face) at a view depth in [near, far]; depth = view-space depth, id = segmentation id, or -1 where nothing
is hit (the kernel writes 0 there; callers compare hit flags separately)."""
import numpy as np

AMBIENT, DIFFUSE = 0.35, 0.65
LIGHT = np.array([1.0, 1.0, 2.0]) / np.sqrt(6.0)
BACKGROUND = (140, 170, 200)


def qmat(q):
    x, y, z, w = (float(v) for v in q)
    n = np.sqrt(x * x + y * y + z * z + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def rays(cam_pos, cam_quat, W, H, hfov_deg):
    """origin (3,), directions (H*W, 3) scaled so that their component along the view axis is 1."""
    R = qmat(cam_quat)
    fwd, left, up = R[:, 0], R[:, 1], R[:, 2]
    t = np.tan(np.radians(hfov_deg) / 2)
    cc, rr = np.meshgrid(np.arange(W), np.arange(H))
    x = (2 * cc + 1) / W - 1
    y = 1 - (2 * rr + 1) / H
    d = fwd + (-left) * (x * t)[..., None] + up * (y * t * H / W)[..., None]
    return np.asarray(cam_pos, float), d.reshape(-1, 3)


def _entry_convex(o, d, planes):
    """Entry parameter (inf: missed) and outward normal of rays against {x : n . x <= w} (rows n, w)."""
    n, w = planes[:, :3], planes[:, 3]
    dn = d @ n.T                                      # (R, F)
    num = w[None, :] - (o @ n.T)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        s = num / dn
    enter = np.where(dn < 0, s, -np.inf)
    leave = np.where(dn > 0, s, np.inf)
    outside_parallel = np.any((dn == 0) & (num < 0), axis=1)
    sin, sout = enter.max(1), leave.min(1)
    face = enter.argmax(1)
    ok = (sin <= sout) & ~outside_parallel & np.isfinite(sin)
    return np.where(ok, sin, np.inf), n[face], face


def _entry_sphere(o, d, c, r):
    oc = o - c
    a = np.einsum("ij,ij->i", d, d)
    b = d @ oc
    cc = oc @ oc - r * r
    disc = b * b - a * cc
    s = np.where(disc >= 0, (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    nrm = (o + s[:, None] * d - c) / r
    return s, nrm


def _entry_capsule(o, d, c, axis, r, hl):
    """Capsule = segment c +- hl axis, radius r: the convex hull of two spheres; its first entry is the nearest of the
    lateral surface's entry (within the segment) and the two spheres' entries."""
    best = np.full(len(d), np.inf)
    nrm = np.zeros((len(d), 3))
    for e in (-1.0, 1.0):
        s, n = _entry_sphere(o, d, c + e * hl * axis, r)
        m = s < best
        best[m], nrm[m] = s[m], n[m]
    oc = o - c
    dp = d - np.outer(d @ axis, axis)
    op = oc - (oc @ axis) * axis
    a = np.einsum("ij,ij->i", dp, dp)
    b = dp @ op
    cc = op @ op - r * r
    disc = b * b - a * cc
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where((disc >= 0) & (a > 0), (-b - np.sqrt(np.maximum(disc, 0))) / a, np.inf)
    z = oc @ axis + s * (d @ axis)
    ok = np.isfinite(s) & (np.abs(z) <= hl) & (s < best)
    p = oc + s[:, None] * d
    radial = p - np.outer(p @ axis, axis)
    best[ok] = s[ok]
    nrm[ok] = radial[ok] / r
    return best, nrm


def _entry_triangles(o, d, tri):
    """Front faces (normal (v1 - v0) x (v2 - v0), facing the ray) of triangles (T, 3, 3): nearest entry per ray."""
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.cross(e1, e2)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dn = d @ n.T                                             # (R, T)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (np.einsum("tk,tk->t", v0 - o, n))[None, :] / dn
    p = o[None, None, :] + s[..., None] * d[:, None, :]      # (R, T, 3)
    # barycentric inside test
    q = p - v0[None]
    d00, d01, d11 = np.einsum("tk,tk->t", e1, e1), np.einsum("tk,tk->t", e1, e2), np.einsum("tk,tk->t", e2, e2)
    d20, d21 = np.einsum("rtk,tk->rt", q, e1), np.einsum("rtk,tk->rt", q, e2)
    den = d00 * d11 - d01 * d01
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    inside = (v >= -1e-9) & (w >= -1e-9) & (v + w <= 1 + 1e-9) & (dn < 0)
    return np.where(inside, s, np.inf), n


def heightfield_triangles(samples, hscale, vscale, border):
    """Every triangle of a height field, split along (i+1, j)-(i, j+1), normals up."""
    rows, cols = samples.shape
    X = np.arange(rows)[:, None] * hscale - border + 0 * np.arange(cols)[None, :]
    Y = np.arange(cols)[None, :] * hscale - border + 0 * np.arange(rows)[:, None]
    P = np.stack([X, Y, samples.astype(np.float64) * vscale], axis=-1)
    a, b, c, e = P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:]
    lower = np.stack([a, b, c], axis=2).reshape(-1, 3, 3)
    upper = np.stack([e, c, b], axis=2).reshape(-1, 3, 3)
    return np.concatenate([lower, upper])


def render(shapes, cam_pos, cam_quat, W, H, hfov, near, far, ground=None, ground_color=(0.5, 0.5, 0.5), facets=False):
    """shapes: dicts with kind ('box' | 'sphere' | 'capsule' | 'poly'), pos (3,), rot (3, 3) world, seg, color and
    half (box), r (sphere / capsule), hl (capsule, along local z), planes (poly: (F, 4) in the shape frame).
    ground: None, 'plane' (z = 0) or (samples, hscale, vscale, border).
    Returns depth (H, W) (inf: nothing), id (H, W) (-1: nothing), rgb (H, W, 3) u8 [, facet (H, W): which shape and which
    of its flat faces / triangles each pixel shows (-1: nothing), cos (H, W): |cos| of the ray's incidence there, with
    facets=True]."""
    o, d = rays(cam_pos, cam_quat, W, H, hfov)
    R = len(d)
    best = np.full(R, np.inf)
    ids = np.full(R, -1)
    col = np.zeros((R, 3))
    nrm = np.zeros((R, 3))
    facet = np.full(R, -1)

    def take(s, n, sid, c, fid):
        m = (s >= near) & (s <= far) & (s < best)
        best[m], ids[m], nrm[m] = s[m], sid, n[m]
        col[m] = c
        facet[m] = np.broadcast_to(fid, (R,))[m]

    for k_sh, sh in enumerate(shapes):
        Rw, c = np.asarray(sh["rot"], float), np.asarray(sh["pos"], float)
        ol, dl = Rw.T @ (o - c), d @ Rw                   # shape frame
        k = sh["kind"]
        if k == "box":
            h = np.asarray(sh["half"], float)
            planes = np.array([[1, 0, 0, h[0]], [-1, 0, 0, h[0]], [0, 1, 0, h[1]], [0, -1, 0, h[1]],
                               [0, 0, 1, h[2]], [0, 0, -1, h[2]]], float)
            s, n, f = _entry_convex(ol, dl, planes)
        elif k == "poly":
            s, n, f = _entry_convex(ol, dl, np.asarray(sh["planes"], float))
        elif k == "sphere":
            (s, n), f = _entry_sphere(ol, dl, np.zeros(3), float(sh["r"])), 0
        elif k == "capsule":
            (s, n), f = _entry_capsule(ol, dl, np.zeros(3), np.array([0.0, 0.0, 1.0]), float(sh["r"]), float(sh["hl"])), 0
        else:
            raise ValueError(k)
        take(s, n @ Rw.T, sh["seg"], np.asarray(sh["color"], float), 100000 * (k_sh + 1) + np.asarray(f))
    if ground is not None:
        if isinstance(ground, str):
            with np.errstate(divide="ignore", invalid="ignore"):
                s = np.where(d[:, 2] < 0, -o[2] / d[:, 2], np.inf)
            n = np.tile([0.0, 0.0, 1.0], (R, 1))
            j = 0
        else:
            tri = heightfield_triangles(*ground)
            s_all, n_t = _entry_triangles(o, d, tri)
            j = s_all.argmin(1)
            s = s_all[np.arange(R), j]
            n = n_t[j]
        take(s, n, 0, np.asarray(ground_color, float), j)
    lam = AMBIENT + DIFFUSE * np.maximum(np.einsum("ij,j->i", nrm, LIGHT), 0.0)
    rgb = np.floor(np.clip(col * lam[:, None], 0, 1) * 255 + 0.5).astype(np.uint8)
    rgb[~np.isfinite(best)] = BACKGROUND
    out = best.reshape(H, W), ids.reshape(H, W), rgb.reshape(H, W, 3)
    if not facets:
        return out
    cos = np.abs(np.einsum("ij,ij->i", nrm, d)) / np.linalg.norm(d, axis=1)     # incidence: 1 head-on, 0 grazing
    return out + (facet.reshape(H, W), cos.reshape(H, W))


def silhouette_adjacent(ids):
    """Pixels with a 4- or 8-neighbour of another id (or that are themselves on such an edge)."""
    H, W = ids.shape
    p = np.pad(ids, 1, mode="edge")
    m = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m |= p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] != ids
    return m
