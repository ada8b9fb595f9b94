"""Independent float64 checker for the optical-flow images of the camera ray caster (csrc/shf_render.hip, FLOW form).

Built on tests/render_ref.py (imported, not edited): render(..., facets=True) gives the view depth and the hit shape of
every pixel; from those the definition of DESIGN.md "Camera sensors" is evaluated directly, per pixel (row r, col c):

    X  = o + s d                                   the surface point now (s: view depth, d: the pixel's ray)
    X' = c_k' + R_k' R_k^T (X - c_k)               where it was: shape k's world pose at the previous render, primed
                                                   (a shape is rigid on its body, so this is the body's motion); terrain: X
    z' = fwd'.(X' - o'),  x' = right'.(X' - o') / (z' t),  y' = up'.(X' - o') / (z' t H/W)
    c' = (x' + 1) W/2 - 1/2,  r' = (1 - y') H/2 - 1/2
    flow = (c - c', r - r')                        pixels, u to the right, v downwards

Flow is exactly 0 where nothing is hit, where z' <= 0 or a term is not finite, and where neither the hit shape's pose nor
the camera's differs from the previous render's (compared as given: callers pass the float32 values the kernel gets)."""
import numpy as np

from tests import render_ref as rr


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


def flow(shapes, shapes_prev, cam, cam_prev, W, H, hfov, near, far, ground=None):
    """shapes / shapes_prev: render_ref shape dicts now / at the previous render (same order; only pos and rot may differ);
    cam / cam_prev: (pos (3,), quat xyzw).  Returns flow (H, W, 2), depth (H, W) (inf: nothing), ids (H, W) (-1: nothing),
    hit (H, W): the index of the shape each pixel shows, -1 for the terrain and -2 for nothing."""
    depth, ids, _, facet, _ = rr.render(shapes, cam[0], cam[1], W, H, hfov, near, far, ground=ground, facets=True)
    o, d = rr.rays(cam[0], cam[1], W, H, hfov)
    s = depth.reshape(-1)
    facet = facet.reshape(-1)
    hit = np.where(facet < 0, -2, np.where(facet >= 100000, facet // 100000 - 1, -1))
    some = hit > -2
    X = o[None, :] + np.where(some, s, 0.0)[:, None] * d
    Xp = X.copy()
    cam_moved = not (_same(cam[0], cam_prev[0]) and _same(cam[1], cam_prev[1]))
    moved = np.full(len(d), cam_moved)
    for k, (a, b) in enumerate(zip(shapes, shapes_prev)):
        m = hit == k
        c, R = np.asarray(a["pos"], float), np.asarray(a["rot"], float)
        cp, Rp = np.asarray(b["pos"], float), np.asarray(b["rot"], float)
        Xp[m] = cp + (X[m] - c) @ (Rp @ R.T).T
        if not (_same(c, cp) and _same(R, Rp)):
            moved |= m
    Rc = rr.qmat(cam_prev[1])
    fwd, right, up = Rc[:, 0], -Rc[:, 1], Rc[:, 2]
    t = np.tan(np.radians(hfov) / 2)
    rel = Xp - np.asarray(cam_prev[0], float)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = rel @ fwd
        x = (rel @ right) / (z * t)
        y = (rel @ up) / (z * t * H / W)
        cprev = (x + 1) * W / 2 - 0.5
        rprev = (1 - y) * H / 2 - 0.5
    cc, rrow = np.meshgrid(np.arange(W), np.arange(H))
    u, v = cc.reshape(-1) - cprev, rrow.reshape(-1) - rprev
    ok = some & moved & (z > 0) & np.isfinite(u) & np.isfinite(v)
    out = np.zeros((len(d), 2))
    out[ok, 0], out[ok, 1] = u[ok], v[ok]
    return out.reshape(H, W, 2), depth, ids, hit.reshape(H, W)
