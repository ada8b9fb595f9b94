"""The float64 ray-caster reference (tests/raycast_ref.py) on its own: the conditions the GPU tests' fixtures rest on -- few
rays within a milliradian of a silhouette or of a facet edge --, its hit and miss conventions, the alignment rule, and that
the pinhole pattern through it reproduces tests/render_ref.py's camera depth."""
import numpy as np
import pytest

from tests import raycast_ref as rc
from tests import render_ref as rr


@pytest.mark.parametrize("terrain", rc.TERRAINS)
@pytest.mark.parametrize("name", sorted(rc.SENSORS))
def test_fixture_conditions(name, terrain):
    """Per case (both envs of every seed): the ambiguity and facet masks stay within the caps, and the fixture sees both
    shapes and terrain."""
    _, _, _, _, _, amb_cap, facet_cap = rc.SENSORS[name]
    o, _ = rc.pattern(name)
    assert len(o) == {"lidar": 1440, "grid": 117}[name]
    kinds = set()
    for seed in rc.SEEDS:
        for ref in rc.fixture(name, terrain, seed):
            amb, facet = ref["ambiguous"].mean(), ref["facet"].mean()
            print(f"{name} {terrain} seed {seed}: ambiguous {amb:.4f}, facet {facet:.4f}, "
                  f"hits {np.bincount(ref['id'] + 2, minlength=6).tolist()}")
            assert amb <= amb_cap, f"ambiguity mask {amb:.4f} > {amb_cap}"
            assert facet <= facet_cap, f"facet mask {facet:.4f} > {facet_cap}"
            assert (ref["id"] == rc.TERRAIN).sum() >= 10
            kinds |= set(ref["id"][ref["id"] >= 0].tolist())
            hit = ref["id"] != rc.MISS
            assert np.isinf(ref["dist"][~hit]).all() and (ref["normal"][~hit] == 0).all()
            assert np.allclose(np.linalg.norm(ref["normal"][hit], axis=1), 1.0, atol=1e-9)
            assert np.isfinite(ref["points"]).all()
    assert len(kinds) >= 3                                        # shapes of several kinds are hit somewhere


def test_lidar_sees_misses_and_the_grid_does_not():
    ref = rc.fixture("lidar", "plane", 0)[0]
    assert (ref["id"] == rc.MISS).sum() > 100                     # the upward channels
    _, pos, _, _, hi, _, _ = rc.SENSORS["lidar"]
    miss = ref["id"] == rc.MISS
    np.testing.assert_allclose(np.linalg.norm(ref["points"][miss] - np.asarray(pos), axis=1), hi, rtol=1e-12)
    assert (rc.fixture("grid", "plane", 0)[0]["id"] != rc.MISS).all()


def test_alignment_rule():
    q = rc.SENSOR_QUAT
    R = rr.qmat(q)
    np.testing.assert_allclose(rc.align_matrix(q, "base"), R)
    Y = rc.align_matrix(q, "yaw")
    np.testing.assert_allclose(Y, [[np.cos(0.7), -np.sin(0.7), 0], [np.sin(0.7), np.cos(0.7), 0], [0, 0, 1]], atol=1e-12)
    np.testing.assert_array_equal(rc.align_matrix(q, "world"), np.eye(3))
    # a downward grid from height h over the plane: yaw-aligned h everywhere, base-aligned h / cos
    from shifu_amd.raycast import grid_pattern
    o, d = grid_pattern((0.4, 0.2), 0.1)
    h = 1.3
    yaw = rc.cast(o, d, (0.2, -0.1, h), q, "yaw", 0.0, 5.0, ground="plane")
    np.testing.assert_allclose(yaw["dist"], h, rtol=1e-12)
    base = rc.cast(o, d, (0.2, -0.1, h), q, "base", 0.0, 5.0, ground="plane")
    oz = h + (np.asarray(o, float) @ R.T)[:, 2]
    np.testing.assert_allclose(base["dist"], oz / R[2, 2], rtol=1e-12)
    assert (base["id"] == rc.TERRAIN).all()


def test_degenerate_directions_miss_at_the_origin():
    o = np.array([[0.1, 0.0, 0.0], [0.0, 0.2, 0.0], [0.0, 0.0, 0.0]])
    d = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, -1.0], [0.0, 0.0, -2.0]])
    ref = rc.cast(o, d, (0.0, 0.0, 1.0), (0, 0, 0, 1.0), "world", 0.0, 5.0, ground="plane")
    assert ref["id"].tolist() == [rc.MISS, rc.MISS, rc.TERRAIN]
    np.testing.assert_allclose(ref["points"], [[0.1, 0.0, 1.0], [0.0, 0.2, 1.0], [0.0, 0.0, 0.0]], atol=1e-15)
    assert ref["dist"][2] == 1.0                                  # range, whatever the direction's length


def test_pinhole_pattern_reproduces_the_camera_reference():
    """dist / |d| of the pinhole pattern is render_ref.render's view depth, ids alike: same closed forms, other bookkeeping."""
    from shifu_amd.raycast import pinhole_pattern
    from shifu_amd.render import lookat_quat
    W, H, fov, near, far = 32, 24, 87.0, 0.05, 6.0
    o, d = pinhole_pattern(W, H, fov)
    norm = np.linalg.norm(d.astype(np.float64), axis=1)
    sc = rc.scene(1)
    shapes = rc.scene_shapes(sc, 0)
    pos = np.array([-1.3, 0.2, 1.1])
    q = lookat_quat(pos, [0.0, 0.0, 0.5])
    hs = rc.ground_of("heightfield")
    # the camera's [near, far] are view depths: cast to the far corner's range and compare where both are inside
    ref = rc.cast(o, d, pos, q, "base", 0.0, 1e3, shapes, hs)
    depth, ids, _ = rr.render(shapes, pos, q, W, H, fov, 1e-9, 1e3, ground=hs[1:])
    got = (ref["dist"] / norm).reshape(H, W)
    both = np.isfinite(depth) & np.isfinite(got) & ~rr.silhouette_adjacent(ids)
    assert both.sum() > 0.25 * W * H
    # (float32 pattern directions against render_ref's float64 pixel rays: compare along the pattern's own rays)
    depth32, ids32 = _render_along(shapes, pos, q, o, d, hs)
    np.testing.assert_allclose(ref["dist"] / norm, depth32, rtol=0, atol=1e-12)
    seg_of_body = {int(s["body"]): int(s["seg"]) for s in shapes}
    want = np.array([seg_of_body.get(int(b), 0 if b == rc.TERRAIN else -1) for b in ref["id"]])
    assert np.array_equal(want, ids32)
    assert np.abs(got[both] - depth[both]).max() < 1e-4        # float32 pattern against float64 pixel rays, off silhouettes


def _render_along(shapes, pos, q, o, d, hs):
    """render_ref.render's own loop along given sensor-frame directions (not unit: view-axis component 1): depth and id."""
    real = rr.rays
    dw = np.asarray(d, np.float64) @ rr.qmat(q).T
    try:
        rr.rays = lambda *a: (np.asarray(pos, float), dw)
        depth, ids, _ = rr.render(shapes, pos, q, len(d), 1, 87.0, 1e-9, 1e3, ground=hs[1:])
    finally:
        rr.rays = real
    return depth.reshape(-1), ids.reshape(-1)
