"""What the world-view tests (tests/test_gpu_world_view.py) share: random multi-env scenes, the float64 reference of a world
view -- tests/render_ref.render on the concatenated, displaced shape list of the drawn envs -- and the project's acceptance
criterion against a reference image, restated from tests/test_gpu_camera.py::_compare (the same numbers: ids equal except
next to a reference silhouette and in at most 0.5 % of the pixels, depth within 1e-4 + 1e-6 s / cos, RGB within 1 LSB away
from facet edges)."""
import numpy as np

from tests import render_ref as rr

W, H, FOV = 48, 32, 60.0


def rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def shape_defs(rng):
    """One shape of each kind, each on a body of its own, in its body frame (tests/test_gpu_camera.py::_shape_defs)."""
    from shifu_amd.model import RenderShape, reduce_hull
    pts = rng.normal(size=(40, 3)) * [0.12, 0.08, 0.1]
    poly = reduce_hull(pts)
    return [RenderShape(0, "box", np.zeros(3), np.eye(3), np.array([0.3, 0.2, 0.12])),
            RenderShape(1, "sphere", np.zeros(3), np.eye(3), np.array([0.13])),
            RenderShape(2, "capsule", np.zeros(3), np.eye(3), np.array([0.07, 0.3])),
            RenderShape(3, "hull", np.zeros(3), np.eye(3), np.zeros(3), poly)]


def shape_radii(defs):
    """Bounding radius of each shape about its body's origin, as render.build_scene computes it (hulls: about the centroid,
    so the centroid's own distance is added)."""
    out = []
    for s in defs:
        if s.kind == "box":
            out.append(np.linalg.norm(0.5 * s.size))
        elif s.kind == "sphere":
            out.append(s.size[0])
        elif s.kind == "capsule":
            out.append(s.size[0] + 0.5 * s.size[1])
        else:
            out.append(np.linalg.norm(np.asarray(s.poly["verts"], float), axis=1).max())
    return np.array(out, float)


class Scene:
    """E envs of the four shapes: poses[e][k] = (pos, quat) of body k, seg ids unique over the whole scene (1 + 4 e + k),
    random colors.  low / high: the box the body positions are drawn from."""

    def __init__(self, E, seed, low=(-0.5, -0.5, 0.1), high=(0.5, 0.5, 0.6)):
        rng = np.random.default_rng(seed)
        self.defs = shape_defs(rng)
        nb = len(self.defs)
        self.E, self.nb = E, nb
        self.poses = [[(rng.uniform(low, high), rand_quat(rng)) for _ in range(nb)] for _ in range(E)]
        self.seg = np.array([[1 + nb * e + k for k in range(nb)] for e in range(E)], np.int32)
        self.col = rng.uniform(0, 1, (E, nb, 3)).astype(np.float32)
        self.rng = rng

    def true_env_radius(self):
        """A sphere about body 0 that really bounds every env's shapes."""
        r = shape_radii(self.defs)
        return max(np.linalg.norm(p - env[0][0]) + r[k] for env in self.poses for k, (p, _) in enumerate(env)) + 1e-3


def ref_shapes(scene, env_ids, offsets):
    """render_ref shape dicts of the drawn envs, in (list position, shape) order, displaced by the list position's offset."""
    out = []
    for j, e in enumerate(env_ids):
        for s, (p, q), sid, c in zip(scene.defs, scene.poses[e], scene.seg[e], scene.col[e]):
            Rb = rr.qmat(q)
            d = dict(kind={"hull": "poly"}.get(s.kind, s.kind), pos=np.asarray(p, float) + Rb @ s.pos + np.asarray(offsets[j], float),
                     rot=Rb @ s.rot, seg=int(sid), color=np.asarray(c, float))
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


def reference(scene, env_ids, offsets, cam, near, far, ground="plane", W_=W, H_=H, fov=FOV):
    """(depth, id, rgb, facet, cos) of render_ref and the env id behind every pixel (-1: terrain or nothing)."""
    ref = rr.render(ref_shapes(scene, env_ids, offsets), cam[0], cam[1], W_, H_, fov, near, far, ground=ground, facets=True)
    facet = ref[3]
    on_shape = facet >= 100000                              # render_ref numbers shape k's facets from 100000 (k + 1)
    pos = np.where(on_shape, facet // 100000 - 1, 0) // scene.nb
    env = np.where(on_shape, np.asarray(env_ids)[pos], -1)
    return ref, env


def compare(depth, seg, rgba, ref, env=None, ref_env=None):
    """tests/test_gpu_camera.py::_compare; with env / ref_env also: the env image equals the reference's wherever the ids
    agree.  Returns the number of pixels whose id differs."""
    rd, rid, rrgb, rfacet, rcos = ref
    got_id = np.where(np.isfinite(depth), seg, -1)
    bad = got_id != rid
    edge = rr.silhouette_adjacent(rid)
    print(f"ids: {int(bad.sum())} of {bad.size} differ ({int((bad & ~edge).sum())} away from silhouettes)")
    assert not (bad & ~edge).any(), f"{int((bad & ~edge).sum())} id mismatches away from silhouettes"
    assert bad.mean() <= 0.005, f"{bad.mean():.4f} of the pixels differ"
    ok = ~bad & np.isfinite(rd)
    tol = 1e-4 + 1e-6 * rd[ok] / np.maximum(rcos[ok], 1e-6)
    err = np.abs(depth[ok] - rd[ok])
    print(f"depth: max error {err.max(initial=0):.3g} m, max error / bound {(err / tol).max(initial=0):.3g}")
    assert (err <= tol).all(), f"depth off by {err.max():.3g} m"
    assert (err > 1e-4).mean() <= 0.001
    diff = np.abs(rgba[..., :3].astype(int) - rrgb.astype(int)).max(-1)
    shade_ok = ~bad & ~rr.silhouette_adjacent(rfacet)
    print(f"rgb: max difference {diff[shade_ok].max(initial=0)} LSB away from facet edges")
    assert diff[shade_ok].max(initial=0) <= 1, f"RGB off by {diff[shade_ok].max()} LSB"
    assert (diff[~bad] > 1).mean() <= 0.002
    assert (rgba[..., 3] == 255).all()
    if env is not None:
        assert (env[~bad] == ref_env[~bad]).all(), "env image differs from the reference where the ids agree"
        assert (env[~np.isfinite(depth)] == -1).all()
    return int(bad.sum())
