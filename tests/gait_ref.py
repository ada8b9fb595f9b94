"""The float64 NumPy twin of csrc/shf_gait.hip (shf_gait_plan, shf_leg_effort_mix): the kernel's header text, operation by
operation, batched over the envs.  No GPU, no torch."""
import numpy as np

PARAM_NAMES = ("dt", "height", "apex", "touchdown_z", "late_depth", "k_fb", "max_step", "leash", "contact_threshold")


def params(dt, height=0.30, apex=0.06, touchdown_z=0.01, late_depth=0.02, k_fb=0.18, max_step=0.15, leash=np.inf,
           contact_threshold=1.0, as_float32=True):
    """The kernel's by-value scalars as a dict; as_float32 rounds each to float32 first (what the kernel receives)."""
    v = dict(dt=dt, height=height, apex=apex, touchdown_z=touchdown_z, late_depth=late_depth, k_fb=k_fb, max_step=max_step,
             leash=leash, contact_threshold=contact_threshold)
    return {k: float(np.float32(x)) if as_float32 else float(x) for k, x in v.items()}


def new_state(n, F):
    """The five state tensors, zeroed (tick int32, sched uint8, the rest float64): call `plan` with reset set before use."""
    return {"tick": np.zeros(n, np.int32), "sched": np.ones((n, F), np.uint8), "anchor": np.zeros((n, F, 3)),
            "target": np.zeros((n, 13)), "yaw": np.zeros(n)}


def rotation(q):
    """(n, 4) xyzw -> (n, 3, 3), the expressions of k_foot_impedance."""
    x, y, z, w = (q[:, k] for k in range(4))
    return np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                     2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x),
                     2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], -1).reshape(-1, 3, 3)


def plan(state, root, feet, contact_z, command, nominal, reset, period, offsets, stance_ticks, P):
    """One tick.  state: the dict of new_state, updated in place.  root (n, 13), feet (n, F, 3), contact_z (n, F) or None,
    command (n, 3), nominal (F, 3), reset (n) or None, period int, offsets / stance_ticks (F) ints, P the dict of `params`.
    Returns {"stance" (n, F) uint8, "swing_target" (n, F, 3) base frame, "phase" (n, F), and for the tests "foothold" (n, F, 2),
    "world_target" (n, F, 3), "scheduled" (n, F) uint8}."""
    root, feet, command, nominal = (np.asarray(a, np.float64) for a in (root, feet, command, nominal))
    n, F = feet.shape[:2]
    offsets, stance_ticks = np.asarray(offsets, np.int64), np.asarray(stance_ticks, np.int64)
    p, q, v = root[:, :3], root[:, 3:7], root[:, 7:10]
    tick = state["tick"].astype(np.int64)
    was = state["sched"] != 0
    anchor, tg, yaw = state["anchor"], state["target"], state["yaw"]
    txy = tg[:, :2].copy()
    # 1. reset
    if reset is not None:
        r = np.asarray(reset) != 0
        tick = np.where(r, 0, tick)
        was = was | r[:, None]
        anchor[r] = np.concatenate([feet[r][..., :2], np.full(feet[r].shape[:2] + (1,), P["touchdown_z"] - P["late_depth"])], -1)
        heading = np.arctan2(2.0 * (q[:, 0] * q[:, 1] + q[:, 3] * q[:, 2]), 1.0 - 2.0 * (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]))
        yaw = np.where(r, heading, yaw)
        txy[r] = p[r, :2]
    # 2. the base target
    cvx, cvy, wz = command[:, 0], command[:, 1], command[:, 2]
    dt = P["dt"]
    cy, sy = np.cos(yaw), np.sin(yaw)
    vw = np.stack([cy * cvx - sy * cvy, sy * cvx + cy * cvy], 1)
    txy = txy + vw * dt
    d = txy - p[:, :2]
    r_ = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    far = r_ > P["leash"]
    with np.errstate(divide="ignore", invalid="ignore"):
        k = P["leash"] / r_
        txy = np.where(far[:, None], p[:, :2] + d * k[:, None], txy)
    yaw = yaw + wz * dt
    hy = yaw * 0.5
    tg[:, :2], tg[:, 2] = txy, P["height"]
    tg[:, 3], tg[:, 4], tg[:, 5], tg[:, 6] = 0.0, 0.0, np.sin(hy), np.cos(hy)
    tg[:, 7:9], tg[:, 9] = vw, 0.0
    tg[:, 10], tg[:, 11], tg[:, 12] = 0.0, 0.0, wz
    R = rotation(q)
    # 3. the schedule
    phi = ((tick % period)[:, None] + offsets[None]) % period                    # (n, F); numpy's % is non-negative
    s = phi < stance_ticks[None]
    # 4. the foothold
    nfx, nfy = nominal[None, :, 0], nominal[None, :, 1]
    nwx = R[:, None, 0, 0] * nfx + R[:, None, 0, 1] * nfy
    nwy = R[:, None, 1, 0] * nfx + R[:, None, 1, 1] * nfy
    hx, hyp = p[:, None, 0] + nwx, p[:, None, 1] + nwy
    vdx, vdy = vw[:, None, 0] - wz[:, None] * nwy, vw[:, None, 1] + wz[:, None] * nwx
    half = (stance_ticks[None].astype(np.float64) * dt) * 0.5
    gx = vdx * half + P["k_fb"] * (v[:, None, 0] - vw[:, None, 0])
    gy = vdy * half + P["k_fb"] * (v[:, None, 1] - vw[:, None, 1])
    m = np.sqrt(gx * gx + gy * gy)
    big = m > P["max_step"]
    with np.errstate(divide="ignore", invalid="ignore"):
        km = P["max_step"] / m
        gx, gy = np.where(big, gx * km, gx), np.where(big, gy * km, gy)
    fx, fy = hx + gx, hyp + gy
    # 5. events
    lift, down = was & ~s, ~was & s
    anchor[lift] = feet[lift]
    td = np.stack([fx, fy, np.full_like(fx, P["touchdown_z"] - P["late_depth"])], -1)
    anchor[down] = td[down]
    # 6. the feet's targets
    touching = np.ones((n, F), bool) if contact_z is None else np.asarray(contact_z, np.float64) > P["contact_threshold"]
    swing_len = np.maximum(period - stance_ticks, 1)[None].astype(np.float64)
    u = (phi - stance_ticks[None] + 1).astype(np.float64) / swing_len
    b = (u * u) * (3.0 - 2.0 * u)
    a1 = 1.0 - b
    ys = np.stack([a1 * anchor[..., 0] + b * fx, a1 * anchor[..., 1] + b * fy,
                   (a1 * anchor[..., 2] + b * P["touchdown_z"]) + ((4.0 * P["apex"]) * u) * (1.0 - u)], -1)
    y = np.where((~s)[..., None], ys, np.where((~touching)[..., None], anchor, feet))
    dlt = y - p[:, None]
    swing = np.stack([(R[:, None, 0, k] * dlt[..., 0] + R[:, None, 1, k] * dlt[..., 1]) + R[:, None, 2, k] * dlt[..., 2]
                      for k in range(3)], -1)
    # 7. outputs
    state["tick"] = (tick + 1).astype(np.int32)
    state["sched"] = s.astype(np.uint8)
    state["yaw"] = yaw
    return {"stance": (s & touching).astype(np.uint8), "swing_target": swing, "phase": phi.astype(np.float64) / float(period),
            "foothold": np.stack([fx, fy], -1), "world_target": y, "scheduled": s.astype(np.uint8)}


def mix(stance_efforts, swing_efforts, stance, chain, limit=None):
    """shf_leg_effort_mix: clamp(stance_efforts + m swing_efforts, +-limit), m (n, nd) = 1 where a foot that is not in stance
    has the dof on its chain (chain (F, nd)); limit entries <= 0 or None: no clamp.  In the inputs' dtype."""
    m = ((np.asarray(stance) == 0)[:, :, None] & (np.asarray(chain) != 0)[None]).any(1).astype(stance_efforts.dtype)
    out = stance_efforts + m * swing_efforts
    if limit is not None:
        lim = np.where(limit > 0, limit, np.inf).astype(stance_efforts.dtype)
        out = np.maximum(np.minimum(out, lim), -lim)
    return out


NOMINAL = np.array([[0.18, -0.13, -0.29], [0.18, 0.13, -0.29], [-0.18, -0.13, -0.29], [-0.18, 0.13, -0.29]])   # A1-like


def seeded_inputs(n, rng, nominal=NOMINAL):
    """One tick's inputs for n envs near a stance: root rows (any yaw, tilted by up to 0.3 rad, moving), feet within 5 cm of
    their nominal places, contact forces z of 0 .. 40 N of which a quarter lie below 1 N, commands in +-0.5 m/s and +-1 rad/s,
    one env in eight flagged for reset.  float32 values (what the kernel reads) as float64 arrays."""
    F = nominal.shape[0]
    yaw, ang, tilt = rng.uniform(-np.pi, np.pi, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 0.3, n)
    a = np.stack([np.cos(ang) * np.sin(tilt / 2), np.sin(ang) * np.sin(tilt / 2), np.zeros(n), np.cos(tilt / 2)], 1)
    b = np.stack([np.zeros(n), np.zeros(n), np.sin(yaw / 2), np.cos(yaw / 2)], 1)
    x1, y1, z1, w1 = b.T
    x2, y2, z2, w2 = a.T
    q = np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                  w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], 1)
    root = np.zeros((n, 13))
    root[:, :2], root[:, 2] = rng.uniform(-2, 2, (n, 2)), rng.uniform(0.25, 0.35, n)
    root[:, 3:7] = q
    root[:, 7:10], root[:, 10:13] = rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-1, 1, (n, 3))
    root = root.astype(np.float32).astype(np.float64)
    R = rotation(root[:, 3:7])
    feet = root[:, None, :3] + np.einsum("nij,fj->nfi", R, nominal) + rng.uniform(-0.05, 0.05, (n, F, 3))
    contact = np.where(rng.uniform(size=(n, F)) < 0.25, rng.uniform(0, 1, (n, F)), rng.uniform(1, 40, (n, F)))
    command = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-1, 1, n)], 1)
    reset = (rng.uniform(size=n) < 0.125).astype(np.uint8)
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    return {"root": root, "feet": f32(feet), "contact": f32(contact), "command": f32(command), "reset": reset}
