"""Independent float64 checker for the ray caster (csrc/shf_render.hip, k_raycast / k_raycast_tw): brute force per ray, numpy only.

Written from the conventions of include/shifu_amd.h (shf_raycast), not from the kernel, on the closed forms of
tests/render_ref.py: every shape against every ray, the height field and the warped trimesh against every one of their
triangles.  Ray r starts at p + R o_r and runs along unit(R d_r), R the sensor's rotation as `align` takes it ("base": all of
it, "yaw": Rz(atan2(R10, R00)), "world": none); the ray parameter is the Euclidean range; a ray reports the nearest surface
ENTERED at a range in [lo, hi]; among shapes at equal range the earlier one wins, the terrain only where it is strictly
nearer.  The id of a ray is the kernel's `body` output: the hit shape's body row, -1 for the terrain, -2 for a miss.

The closed forms take one origin for many rays, so rays are cast in groups of equal origin (a lidar is one group).

Two masks come with every cast, both from four copies of every ray tilted by TILT rad along two axes perpendicular to it:
ambiguous -- a tilted copy hits another id, or the same id at a range that differs by more than 0.02 + 0.05 dist (the ray
passes a silhouette or a step edge within a milliradian: float32 may fall either way); facet -- a tilted copy hits the same
id with a normal that differs (n . n' < 0.999: the ray passes an edge between two faces, where either normal is right)."""
import numpy as np

from tests import render_ref as rr
from tests import trimesh_render_ref as tr

TILT = 1e-3
MISS, TERRAIN = -2, -1


def align_matrix(quat, align):
    R = rr.qmat(quat)
    if align == "base":
        return R
    if align == "yaw":
        a = np.arctan2(R[1, 0], R[0, 0])
        return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    if align == "world":
        return np.eye(3)
    raise ValueError(align)


def world_rays(origins, dirs, pos, quat, align):
    """World origins (R, 3), unit directions (R, 3) and the mask of rays that have one (direction not zero, finite)."""
    R = align_matrix(quat, align)
    o = np.asarray(pos, np.float64)[None, :] + np.asarray(origins, np.float64) @ R.T
    d = np.asarray(dirs, np.float64) @ R.T
    with np.errstate(invalid="ignore", over="ignore"):
        l2 = np.einsum("ij,ij->i", d, d)
    valid = np.isfinite(l2) & (l2 > 0)
    d = np.where(valid[:, None], d / np.sqrt(np.where(valid, l2, 1.0))[:, None], [1.0, 0.0, 0.0])
    return o, d, valid


def tilted(d):
    """(4 R, 3): every unit direction tilted by +-TILT rad along two axes perpendicular to it and to each other."""
    k = np.argmin(np.abs(d), axis=1)
    e = np.zeros_like(d)
    e[np.arange(len(d)), k] = 1.0
    u = np.cross(d, e)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(d, u)
    out = [d * np.cos(TILT) + w * np.sin(TILT) for w in (u, -u, v, -v)]
    return np.concatenate(out)


def _groups(o):
    """Index arrays of the rays that share an origin."""
    _, inv = np.unique(o, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(inv, kind="stable")
    cuts = np.nonzero(np.diff(inv[order]))[0] + 1
    return np.split(order, cuts)


def cast_shapes(o, d, shapes, lo, hi):
    """Nearest shape entered at a range in [lo, hi] (the earlier shape on a tie): range (R,) (inf: none), id (R,), normal."""
    n_rays = len(d)
    best, ids, nrm = np.full(n_rays, np.inf), np.full(n_rays, MISS), np.zeros((n_rays, 3))
    if not shapes:
        return best, ids, nrm
    for g in _groups(o):
        og, dg = o[g[0]], d[g]
        b, i, n = np.full(len(g), np.inf), np.full(len(g), MISS), np.zeros((len(g), 3))
        for k, sh in enumerate(shapes):
            Rw, c = np.asarray(sh["rot"], float), np.asarray(sh["pos"], float)
            ol, dl = Rw.T @ (og - c), dg @ Rw
            kind = sh["kind"]
            if kind == "box":
                h = np.asarray(sh["half"], float)
                planes = np.array([[1, 0, 0, h[0]], [-1, 0, 0, h[0]], [0, 1, 0, h[1]], [0, -1, 0, h[1]],
                                   [0, 0, 1, h[2]], [0, 0, -1, h[2]]], float)
                s, nl, _ = rr._entry_convex(ol, dl, planes)
            elif kind == "poly":
                s, nl, _ = rr._entry_convex(ol, dl, np.asarray(sh["planes"], float))
            elif kind == "sphere":
                s, nl = rr._entry_sphere(ol, dl, np.zeros(3), float(sh["r"]))
            elif kind == "capsule":
                with np.errstate(invalid="ignore"):          # (rays that miss carry inf through its normal)
                    s, nl = rr._entry_capsule(ol, dl, np.zeros(3), np.array([0.0, 0.0, 1.0]), float(sh["r"]), float(sh["hl"]))
            else:
                raise ValueError(kind)
            m = (s >= lo) & (s <= hi) & (s < b)
            b[m], i[m], n[m] = s[m], sh.get("body", k), nl[m] @ Rw.T
        best[g], ids[g], nrm[g] = b, i, n
    return best, ids, nrm


def cast_ground(o, d, ground, lo, hi, chunk=256):
    """ground: None, 'plane' (z = 0), ('heightfield', samples, hscale, vscale, border) or ('trimesh', triangles (T, 3, 3)).
    Nearest front face entered at a range in [lo, hi]: range (R,) (inf: none) and unit normal (R, 3)."""
    n_rays = len(d)
    best, nrm = np.full(n_rays, np.inf), np.zeros((n_rays, 3))
    if ground is None:
        return best, nrm
    if isinstance(ground, str):
        assert ground == "plane"
        with np.errstate(divide="ignore", invalid="ignore"):
            s = np.where(d[:, 2] < 0, -o[:, 2] / d[:, 2], np.inf)
        m = (s >= lo) & (s <= hi)
        best[m], nrm[m] = s[m], [0.0, 0.0, 1.0]
        return best, nrm
    tri = rr.heightfield_triangles(*ground[1:]) if ground[0] == "heightfield" else np.asarray(ground[1], np.float64)
    for g in _groups(o):
        for a in range(0, len(g), chunk):
            gi = g[a:a + chunk]
            if ground[0] == "heightfield":
                s_all, n_t = rr._entry_triangles(o[gi[0]], d[gi], tri)
                s_all = np.where((s_all >= lo) & (s_all <= hi), s_all, np.inf)
                j = s_all.argmin(1)
                s, n = s_all[np.arange(len(gi)), j], n_t[j]
            else:
                s, n, _, _ = tr.entry_triangles(o[gi[0]], d[gi], tri, lo, hi)
            m = np.isfinite(s)
            best[gi[m]], nrm[gi[m]] = s[m], n[m]
    return best, nrm


def merge(shape_hit, ground_hit):
    """The nearest of both; the terrain wins only where it is strictly nearer."""
    (bs, ids, ns), (bg, ng) = shape_hit, ground_hit
    t = bg < bs
    return np.where(t, bg, bs), np.where(t, TERRAIN, ids), np.where(t[:, None], ng, ns)


class Rays:
    """The world rays of a pattern from one sensor pose, followed by their four tilted copies (5 R rays, the copies of ray r
    at r + k R); rays without a direction are cast as misses."""

    def __init__(self, origins, dirs, pos, quat, align):
        self.o, self.d, self.valid = world_rays(origins, dirs, pos, quat, align)
        self.R = len(self.d)
        self.o5 = np.concatenate([self.o] * 5)
        self.d5 = np.concatenate([self.d, tilted(self.d)])


def result(rays, shape_hit5, ground_hit5, hi):
    """dict(dist, id, normal, cos, points, ambiguous, facet) over the R rays from the casts of rays.o5 / rays.d5."""
    R = rays.R
    s5, id5, n5 = merge(shape_hit5, ground_hit5)
    inv5 = np.concatenate([~rays.valid] * 5)
    s5, id5, n5 = np.where(inv5, np.inf, s5), np.where(inv5, MISS, id5), np.where(inv5[:, None], 0.0, n5)
    s, ids, n = s5[:R], id5[:R], n5[:R]
    amb, facet = np.zeros(R, bool), np.zeros(R, bool)
    for k in range(1, 5):
        st, it, nt = s5[k * R:(k + 1) * R], id5[k * R:(k + 1) * R], n5[k * R:(k + 1) * R]
        same = it == ids
        with np.errstate(invalid="ignore"):
            far = np.abs(np.where(np.isfinite(st), st, 0.0) - np.where(np.isfinite(s), s, 0.0)) > 0.02 + 0.05 * np.where(np.isfinite(s), s, 0.0)
        amb |= ~same | (same & (ids != MISS) & far)
        facet |= same & (ids != MISS) & (np.einsum("ij,ij->i", n, nt) < 0.999)
    hit = ids != MISS
    reach = np.where(hit, np.where(hit, s, 0.0), np.where(rays.valid, hi, 0.0))
    return dict(dist=s, id=ids, normal=n, cos=np.abs(np.einsum("ij,ij->i", n, rays.d)), points=rays.o + reach[:, None] * rays.d,
                ambiguous=amb, facet=facet)


def cast(origins, dirs, pos, quat, align, lo, hi, shapes=(), ground=None):
    """The whole reference for one env: see result()."""
    rays = Rays(origins, dirs, pos, quat, align)
    return result(rays, cast_shapes(rays.o5, rays.d5, list(shapes), lo, hi), cast_ground(rays.o5, rays.d5, ground, lo, hi), hi)


# ---- the fixtures of tests/test_raycast_ref.py and tests/test_gpu_raycast.py ---------------------------------------------
def euler_quat(roll, pitch, yaw):
    """Quaternion (x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll)."""
    cr, sr, cp, sp, cy, sy = np.cos(roll / 2), np.sin(roll / 2), np.cos(pitch / 2), np.sin(pitch / 2), np.cos(yaw / 2), np.sin(yaw / 2)
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy,
                     cr * cp * cy + sr * sp * sy])


SENSOR_QUAT = euler_quat(0.1, -0.15, 0.7)
SEEDS = (0, 1, 2, 3)
TERRAINS = ("plane", "heightfield", "trimesh")
# name -> (pattern arguments, sensor position, align, min_range, max_range, ambiguity cap, facet cap)
SENSORS = {"lidar": ((16, (-25.0, 15.0), (-180.0, 180.0), 4.0), (0.05, -0.1, 0.75), "base", 0.05, 4.0, 0.01, 0.02),
           "grid": (((1.56, 1.04), 0.13), (0.1037, 0.0471, 1.6), "yaw", 0.0, 3.0, 0.02, 0.10)}


def pattern(name):
    from shifu_amd.raycast import grid_pattern, lidar_pattern
    return (lidar_pattern if name == "lidar" else grid_pattern)(*SENSORS[name][0])


def scene(seed):
    from tests import world_view_ref as wr
    return wr.Scene(2, seed, low=(-0.6, -0.6, 0.35), high=(0.6, 0.6, 0.9))


def scene_shapes(sc, env):
    """render_ref shape dicts of one env of a world_view_ref.Scene, each with its body row."""
    from tests import world_view_ref as wr
    out = wr.ref_shapes(sc, [env], [np.zeros(3)])
    for k, s in enumerate(out):
        s["body"] = int(sc.defs[k].body)
    return out


def ground_of(terrain):
    if terrain == "plane":
        return "plane"
    hs = tr.fixture_samples()
    if terrain == "heightfield":
        return ("heightfield", hs, tr.HSCALE, tr.VSCALE, tr.BORDER)
    return ("trimesh", tr.mesh_triangles(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD, tr.BORDER))


_CACHE = {}


def fixture(name, terrain, seed):
    """[result of env 0, result of env 1] of a fixture case -- computed once per process, not to be modified.  The terrain's
    cast does not depend on the shapes nor the shapes' on the terrain, so each is computed once and shared."""
    key = (name, terrain, seed)
    if key not in _CACHE:
        _, pos, align, lo, hi, _, _ = SENSORS[name]
        if ("rays", name) not in _CACHE:
            o, d = pattern(name)
            _CACHE[("rays", name)] = Rays(o, d, pos, SENSOR_QUAT, align)
        rays = _CACHE[("rays", name)]
        if ("ground", name, terrain) not in _CACHE:
            _CACHE[("ground", name, terrain)] = cast_ground(rays.o5, rays.d5, ground_of(terrain), lo, hi)
        if ("shapes", name, seed) not in _CACHE:
            sc = scene(seed)
            _CACHE[("shapes", name, seed)] = [cast_shapes(rays.o5, rays.d5, scene_shapes(sc, e), lo, hi) for e in range(sc.E)]
        _CACHE[key] = [result(rays, sh, _CACHE[("ground", name, terrain)], hi) for sh in _CACHE[("shapes", name, seed)]]
    return _CACHE[key]
