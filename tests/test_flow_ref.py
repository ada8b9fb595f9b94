"""Closed-form known answers of the optical-flow checker tests/flow_ref.py (numpy only)."""
import numpy as np

from tests import flow_ref as fr

IDENT = np.array([0.0, 0.0, 0.0, 1.0])          # camera looking along world +x, +z up: right = -y
W, H = 32, 24


def _wall(z, seg=3):
    """A box whose front face is the plane x = z, far wider than the view."""
    return dict(kind="box", pos=np.array([z + 0.5, 0.0, 0.0]), rot=np.eye(3), half=np.array([0.5, 50.0, 50.0]), seg=seg,
                color=np.ones(3))


def _yaw(theta):
    return np.array([0.0, 0.0, np.sin(theta / 2), np.cos(theta / 2)])


def test_camera_translating_along_its_right_axis_past_a_wall():
    """fov 90 (t = 1), wall at depth z, camera moved by D along right: every wall pixel shows u = -W D / (2 z), v = 0."""
    z, D = 2.0, 0.1
    wall = [_wall(z)]
    prev, now = (np.zeros(3), IDENT), (np.array([0.0, -D, 0.0]), IDENT)
    flow, depth, ids, hit = fr.flow(wall, wall, now, prev, W, H, 90.0, 0.1, 10.0)
    assert (ids == 3).all() and (hit == 0).all()
    np.testing.assert_allclose(depth, z, rtol=1e-12)
    np.testing.assert_allclose(flow[..., 0], -W * D / (2 * z), rtol=0, atol=1e-12)
    np.testing.assert_allclose(flow[..., 1], 0.0, atol=1e-12)
    assert abs(-W * D / (2 * z) + 0.8) < 1e-15       # the figure the GPU test asks for


def test_pure_camera_yaw_matches_the_tangent_difference():
    """The camera yawed to the left by theta since the previous render: a pixel whose ray makes tan(alpha) = a with the
    forward axis (to the right) was at tan(alpha - theta) before (the previous camera pointed theta further right), whatever
    its depth; rows scale with the change of z."""
    theta, fov = 0.02, 70.0
    t = np.tan(np.radians(fov) / 2)
    wall = [_wall(1.7)]
    flow, _, ids, _ = fr.flow(wall, wall, (np.zeros(3), _yaw(theta)), (np.zeros(3), IDENT), W, H, fov, 0.1, 10.0)
    assert (ids == 3).all()
    x = 2 * (np.arange(W) + 0.5) / W - 1
    y = 1 - 2 * (np.arange(H) + 0.5) / H
    a = x * t
    u = (W / 2) * (a - np.tan(np.arctan(a) - theta)) / t
    yprev = y[:, None] / (np.cos(theta) + a[None, :] * np.sin(theta))
    v = (H / 2) * (yprev - y[:, None])
    np.testing.assert_allclose(flow[..., 0], np.broadcast_to(u, (H, W)), atol=1e-11)
    np.testing.assert_allclose(flow[..., 1], v, atol=1e-11)
    assert (flow[..., 0] > 0).all()                  # yaw to the left: the image moves to the right


def test_box_approaching_a_static_camera_expands_about_the_principal_point():
    z, delta = 1.5, 0.05
    now = dict(kind="box", pos=np.array([z + 0.1, 0.0, 0.0]), rot=np.eye(3), half=np.array([0.1, 0.3, 0.2]), seg=5, color=np.ones(3))
    prev = dict(now, pos=now["pos"] + [delta, 0.0, 0.0])
    cam = (np.zeros(3), IDENT)
    flow, depth, ids, hit = fr.flow([now], [prev], cam, cam, W, H, 60.0, 0.1, 10.0)
    on = ids == 5
    assert 40 < on.sum() < W * H and (hit[on] == 0).all() and (hit[~on] == -2).all()
    np.testing.assert_allclose(depth[on], z, rtol=1e-12)
    cc, rr_ = np.meshgrid(np.arange(W), np.arange(H))
    k = delta / (z + delta)                            # c' - c_pp = (c - c_pp) z / (z + delta)
    np.testing.assert_allclose(flow[..., 0][on], (cc[on] - (W / 2 - 0.5)) * k, atol=1e-12)
    np.testing.assert_allclose(flow[..., 1][on], (rr_[on] - (H / 2 - 0.5)) * k, atol=1e-12)
    assert (flow[~on] == 0).all()                      # nothing hit: exactly zero


def test_a_static_scene_is_exactly_zero():
    shapes = [_wall(2.0), dict(kind="sphere", pos=np.array([1.0, 0.1, 0.0]), rot=np.eye(3), r=0.2, seg=4, color=np.ones(3))]
    cam = (np.array([0.013, -0.02, 0.3]), _yaw(0.1))
    flow, _, ids, _ = fr.flow(shapes, shapes, cam, cam, W, H, 60.0, 0.1, 10.0, ground="plane")
    assert set(np.unique(ids)) == {0, 3, 4}
    assert (flow == 0).all() and not np.signbit(flow).any()
    # only the sphere moves: every other pixel stays exactly zero
    moved = [shapes[0], dict(shapes[1], pos=shapes[1]["pos"] + [0.0, 0.01, 0.0])]
    flow, _, ids, _ = fr.flow(shapes, moved, cam, cam, W, H, 60.0, 0.1, 10.0, ground="plane")
    assert (flow[ids != 4] == 0).all() and (flow[ids == 4] != 0).any()


def test_a_point_behind_the_previous_camera_has_no_flow():
    wall = [_wall(1.0)]
    now, prev = (np.zeros(3), IDENT), (np.array([2.0, 0.0, 0.0]), IDENT)      # the previous camera stood beyond the face
    flow, _, ids, _ = fr.flow(wall, wall, now, prev, W, H, 60.0, 0.1, 10.0)
    assert (ids == 3).all() and (flow == 0).all()
