"""The warped-trimesh checker (tests/trimesh_render_ref.py) and the fixture the GPU tests render, on the CPU: the checker
against triangles built directly from the grid, the fixture's risers and collapsed triangles counted, and the search set
the kernel's walk takes from the cells' hint bits (csrc/shf_render.hip tw_cell) shown to hold every triangle that can be
hit inside a cell's square."""
import numpy as np

from tests import trimesh_render_ref as tr


def _unshifted_field():
    from shifu_amd.isaacgym.terrain_utils import SubTerrain, random_uniform_terrain
    np.random.seed(5)
    t = SubTerrain(width=20, length=17, vertical_scale=0.005, horizontal_scale=0.1)
    random_uniform_terrain(t, -0.1, 0.1, 0.005, downsampled_scale=0.2)
    return np.ascontiguousarray(t.height_field_raw, np.int16)


def test_unshifted_mesh_equals_the_grid_triangles_built_directly():
    """slope_threshold=None: the mesh is the grid's (v00, v11, v01) / (v00, v10, v11) triangles."""
    from tests import render_ref as rr
    hs, border = _unshifted_field(), 0.8
    rows, cols = hs.shape
    P = np.stack(np.broadcast_arrays(np.arange(rows)[:, None] * 0.1 - border, np.arange(cols)[None, :] * 0.1 - border,
                                     hs.astype(np.float64) * 0.005), axis=-1)
    v00, v10, v01, v11 = P[:-1, :-1], P[1:, :-1], P[:-1, 1:], P[1:, 1:]
    direct = np.concatenate([np.stack([v00, v11, v01], 2).reshape(-1, 3, 3), np.stack([v00, v10, v11], 2).reshape(-1, 3, 3)])
    tri = tr.mesh_triangles(hs, 0.1, 0.005, None, border)
    assert len(tri) == len(direct) == 2 * (rows - 1) * (cols - 1)
    seen = 0
    for pos, quat in tr.fixture_cameras():
        (depth, ids, _, _, _), _ = tr.render([], tri, pos, quat, 32, 24, 87.0, 0.05, 6.0)
        o, d = rr.rays(pos, quat, 32, 24, 87.0)
        s, n = rr._entry_triangles(o, d, direct)                  # render_ref's own triangle test, on the direct triangles
        s = np.where((s >= 0.05) & (s <= 6.0), s, np.inf).min(1).reshape(24, 32)
        both = np.isfinite(s) & np.isfinite(depth)
        # (vertices are float32 in the mesh and float64 here: 1e-6 m covers that; the hit flags may differ only on an edge ray)
        assert (np.isfinite(s) != np.isfinite(depth)).sum() <= 2
        np.testing.assert_allclose(depth[both], s[both], rtol=0, atol=1e-5)
        assert ((ids == 0) == np.isfinite(depth)).all()
        seen += int(both.sum())
    assert seen > 1000


def test_fixture_keeps_its_risers():
    from shifu_amd.isaacgym.terrain_utils import vertex_shifts
    hs = tr.fixture_samples()
    assert hs.shape == (24, 24)
    dx, dy = vertex_shifts(hs.astype(np.int64), tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD)
    assert int(((dx != 0) | (dy != 0)).sum()) == 250
    tri, refs = tr.fixture_reference()
    zero, vertical = tr.triangle_classes(tri)
    assert int(zero.sum()) == 34 and int(vertical.sum()) == 466
    riser_px, ambiguous = [], 0
    for (depth, ids, rgb, facet, cos), amb in refs:
        riser_px.append(int((vertical[np.maximum(facet, 0)] & (facet >= 0)).sum()))
        ambiguous += int(amb.sum())
        assert not zero[facet[facet >= 0]].any()
    assert riser_px == [183, 1535, 0, 622]
    assert ambiguous == 7                                         # 0.057 % of 4 x 64 x 48 pixels


def _clip(poly, i, j):
    """Sutherland-Hodgman: the polygon (or segment: two points) `poly` clipped to the closed square [i, i + 1] x [j, j + 1]."""
    for axis, bound, keep_less in ((0, i, False), (0, i + 1, True), (1, j, False), (1, j + 1, True)):
        inside = lambda p: p[axis] <= bound if keep_less else p[axis] >= bound
        out, n = [], len(poly)
        for k in range(n if n > 2 else n - 1):
            p, q = poly[k], poly[(k + 1) % n]
            if inside(p):
                out.append(p)
            if inside(p) != inside(q):
                t = (bound - p[axis]) / (q[axis] - p[axis])
                out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        if n == 2 and inside(poly[1]):
            out.append(poly[1])
        poly = out
        if len(poly) < 2:
            return []
    return poly


def _reaches_into(pts, i, j):
    """The horizontal projection of a triangle (3 integer points in cell units) shares more than isolated points or, for a
    triangle with extent, more than a boundary line with the closed square [i, i + 1] x [j, j + 1]: a projection with area
    overlaps the square in an area; a riser, which projects to a segment, in a length (a riser standing on the cell's
    boundary counts).  Rays that hit a surface exactly on such a point or line are of measure zero."""
    pts = [(float(x), float(y)) for x, y in pts]
    area2 = (pts[1][0] - pts[0][0]) * (pts[2][1] - pts[0][1]) - (pts[1][1] - pts[0][1]) * (pts[2][0] - pts[0][0])
    if area2 != 0:
        c = _clip(pts, i, j)
        return len(c) >= 3 and abs(sum(c[k][0] * c[(k + 1) % len(c)][1] - c[(k + 1) % len(c)][0] * c[k][1]
                                       for k in range(len(c)))) > 1e-9
    ends = [min(pts), max(pts)]
    if ends[0] == ends[1]:
        return False                                              # three corners over one point: a collapsed or edge-on sliver
    c = _clip(ends, i, j)
    return len(c) >= 2 and abs(c[-1][0] - c[0][0]) + abs(c[-1][1] - c[0][1]) > 1e-9


def test_hint_bits_cover_every_triangle_that_reaches_into_a_cell():
    """The kernel tests, in cell (i, j), the triangles of rows [i - bit4, i + bit5] x columns [j - bit6, j + bit7] and accepts
    hits inside the cell's closed square.  For the fixture: every triangle whose horizontal projection reaches into that
    square (_reaches_into: risers standing exactly on the cell's boundary included) is in the set.  The bits were derived
    for vertical queries; the criterion -- which projections reach into the square -- is the same for a ray, whose hits are
    filtered to the square too.  Not in the set are only contacts of measure zero: a neighbour's surface along the shared
    edge (the walk meets it in its own cell) and single corner points."""
    from shifu_amd.isaacgym.terrain_utils import trimesh_warp_map, vertex_shifts
    hs = tr.fixture_samples()
    rows, cols = hs.shape
    warp = trimesh_warp_map(hs, tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD).astype(np.int64)
    dx, dy = vertex_shifts(hs.astype(np.int64), tr.HSCALE, tr.VSCALE, tr.SLOPE_THRESHOLD)
    assert np.array_equal(warp & 3, dx.astype(np.int64) + 1) and np.array_equal((warp >> 2) & 3, dy.astype(np.int64) + 1)
    X = (np.arange(rows)[:, None] + dx).astype(np.int64)
    Y = (np.arange(cols)[None, :] + dy).astype(np.int64)

    def cell_triangles(a, b):
        v = lambda p, q: (int(X[p, q]), int(Y[p, q]))
        v00, v10, v01, v11 = v(a, b), v(a + 1, b), v(a, b + 1), v(a + 1, b + 1)
        return [(v00, v11, v01), (v00, v10, v11)]

    # the criterion itself: a cell's own triangles, a riser on its boundary, a neighbour along an edge, a corner point
    assert _reaches_into([(0, 0), (1, 1), (0, 1)], 0, 0) and _reaches_into([(1, 0), (1, 1), (1, 1)], 0, 0)
    assert _reaches_into([(0, 0), (2, 2), (0, 1)], 1, 1) and not _reaches_into([(1, 0), (2, 1), (1, 1)], 0, 0)
    assert not _reaches_into([(0, 0), (2, 2), (0, 1)], 1, 2) and not _reaches_into([(1, 1), (1, 2), (1, 2)], 0, 0)
    checked = reaching = single = 0
    for i in range(rows - 1):
        for j in range(cols - 1):
            w = warp[i, j]
            ilo, ihi = i - ((w >> 4) & 1 if i > 0 else 0), i + ((w >> 5) & 1 if i < rows - 2 else 0)
            jlo, jhi = j - ((w >> 6) & 1 if j > 0 else 0), j + ((w >> 7) & 1 if j < cols - 2 else 0)
            single += int(ilo == ihi and jlo == jhi)
            # a vertex moves by at most one cell: only the 5 x 5 block of cells around the cell can reach it
            for a in range(max(i - 2, 0), min(i + 3, rows - 1)):
                for b in range(max(j - 2, 0), min(j + 3, cols - 1)):
                    searched = ilo <= a <= ihi and jlo <= b <= jhi
                    for t in cell_triangles(a, b):
                        r = _reaches_into(t, i, j)
                        assert searched or not r, (i, j, a, b, t)
                        reaching += int(r and (a, b) != (i, j))
                    checked += 1
    assert checked > 5000 and reaching > 500                      # neighbours do reach in, and the set holds them
    assert 0 < single < (rows - 1) * (cols - 1)                   # and it is not the whole 3 x 3 block everywhere
