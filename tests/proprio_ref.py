"""The proprioceptive sensors' algorithm (the header of shifu_amd/csrc/shf_proprio.hip) in NumPy, step by step as that text
states it.  `step32` keeps the kernel's float32 operations in the kernel's order: NumPy rounds every elementwise float32
operation correctly and fuses nothing, so it is bit-equal to the kernel.  `step64` is the same text in float64: the reference
for what the float32 arithmetic costs.  (The uniforms are 24-bit integers times 2^-24, exact in both.)

cfg: dict(imus=[(body, (px, py, pz), (qx, qy, qz, qw))], feet=[body, ...], contact_mode="norm" | "z", velocity="direct" |
"difference", slots=L, max_delay=, gravity=(3), dt=, inv_dt=, seed=, env_id_offset=); `config_of` makes it from the library's
ShfProprioConfig.  params: the 16 floats of shifu_amd.proprio.make_params.  state: {"counter" (N, U, 2) int32, "imu" (N, I, 9 + 6 L),
"enc" (N, nd, 2 + 2 L), "foot" (N, F, 5 + 6 L)}, the kernel's layouts, updated in place."""
import numpy as np

M0, M1, W0, W1, MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
STREAM_IMU, STREAM_ENC = 0x50000000, 0x50001000
S32 = np.uint64(32)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of 32-bit words held in uint64 (csrc/shf_task.h: philox4x32)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def config_of(c):
    """The twin's cfg dict from an _abi.ShfProprioConfig."""
    return dict(imus=[(int(c.imu_body[i]), tuple(c.imu_pos[i]), tuple(c.imu_quat[i])) for i in range(c.num_imus)],
                feet=[int(c.foot_body[f]) for f in range(c.num_feet)], contact_mode=("norm", "z")[c.contact_mode],
                velocity=("direct", "difference")[c.velocity_mode], slots=int(c.slots), max_delay=int(c.max_delay),
                gravity=tuple(c.gravity), dt=float(c.dt), inv_dt=float(c.inv_dt), seed=int(c.seed_lo) | (int(c.seed_hi) << 32),
                env_id_offset=int(c.env_id_offset))


def make_state(n, num_imus, nd, num_feet, L, dtype=np.float32):
    return dict(counter=np.zeros((n, num_imus + nd + num_feet, 2), np.int32), imu=np.zeros((n, num_imus, 9 + 6 * L), dtype),
                enc=np.zeros((n, nd, 2 + 2 * L), dtype), foot=np.zeros((n, num_feet, 5 + 6 * L), dtype))


class _Draws:
    def __init__(self, cfg, c, T, gids=None):
        n = c.shape[0]
        gid = np.uint64(cfg["env_id_offset"]) + np.arange(n, dtype=np.uint64) if gids is None else np.asarray(gids).astype(np.uint64)
        self.lo, self.hi, self.c, self.T = gid & MASK, gid >> S32, c.astype(np.uint64), T
        self.k0, self.k1 = cfg["seed"] & 0xFFFFFFFF, (cfg["seed"] >> 32) & 0xFFFFFFFF

    def block(self, stream):
        """u_0 .. u_3 of one block per env; stream: an int, or an array (..., ) broadcast against the envs' leading axis."""
        stream = np.asarray(stream, np.uint64)
        sh = (-1,) + (1,) * stream.ndim
        w = philox4x32(self.lo.reshape(sh), self.c.reshape(sh), stream, self.hi.reshape(sh), self.k0, self.k1)
        return [((x >> np.uint64(8)).astype(np.float32) * np.float32(5.9604644775390625e-08)).astype(self.T) for x in w]

    def gauss(self, stream):
        u, T = self.block(stream), self.T
        return (((u[0] + u[1]) + (u[2] + u[3])) - T(2.0)) * T(np.float32(1.7320508))


def _usym(u, b):
    return ((b - (-b)) * u) + (-b)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return (((aw * bx + ax * bw) + ay * bz) - az * by, ((aw * by - ax * bz) + ay * bw) + az * bx,
            ((aw * bz + ax * by) - ay * bx) + az * bw, ((aw * bw - ax * bx) - ay * by) - az * bz)


def _matrix(q, T):
    x, y, z, w = q
    one, two = T(1.0), T(2.0)
    return [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
            [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
            [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]


def _ring(a, shape):
    r = a.reshape(shape)
    assert np.shares_memory(r, a), "the ring must be a view of the state"
    return r


def _latency(ring, h, D, rs, m):
    """ring (n, L, C) a view into the state, m (n, C): the delayed output; the ring updated in place."""
    n, L, _ = ring.shape
    rows = np.arange(n)
    slot = h - D
    slot = np.where(slot < 0, slot + L, slot)
    out = np.where((rs | (D == 0))[:, None], m, ring[rows, slot])
    ring[rs] = m[rs][:, None, :]
    keep = ~rs
    ring[rows[keep], h[keep]] = m[keep]
    return out


def _step(T, cfg, params, state, body_state, dof_state, contact, delay, reset, gids=None):
    f = lambda a: None if a is None else np.asarray(a).astype(T)
    body_state, dof_state, contact = f(body_state), f(dof_state), f(contact)
    P = [T(np.float32(v)) for v in np.asarray(params, np.float32)]
    sg, sa, wg, wa, b0g, b0a, sq, sv, o_rng, res, inv_res, on2, off2 = P[:13]
    n, nd = dof_state.shape[:2]
    imus, feet, L = cfg["imus"], cfg["feet"], cfg["slots"]
    I, F = len(imus), len(feet)
    dt, inv_dt = T(np.float32(cfg["dt"])), T(np.float32(cfg["inv_dt"]))
    g = [T(np.float32(v)) for v in cfg["gravity"]]
    cnt = state["counter"]
    assert cnt.shape == (n, I + nd + F, 2)
    c = cnt[:, 0, 0].view(np.uint32).copy()
    assert (cnt[:, :, 0] == cnt[:, :1, 0]).all(), "every unit of an env carries the same read counter"
    h = cnt[:, 0, 1].copy()
    rs = (c == 0)
    if reset is not None:
        rs = rs | (np.asarray(reset).reshape(n) != 0)
    Dl = np.minimum(np.maximum(np.asarray(delay, np.int32).reshape(n, 3), 0), cfg["max_delay"])
    draws = _Draws(cfg, c, T, gids)
    out = np.zeros((n, 6 * I + 2 * nd + 6 * F), T)
    sw = np.zeros((n, 2 * F), np.uint8)
    # 1. IMUs
    for i, (b, ps, qs) in enumerate(imus):
        S = STREAM_IMU + 16 * i
        ps, qs = [T(np.float32(v)) for v in ps], [T(np.float32(v)) for v in qs]
        bs = body_state[:, b]
        qb = [bs[:, 3 + k] for k in range(4)]
        vb, wb = [bs[:, 7 + k] for k in range(3)], [bs[:, 10 + k] for k in range(3)]
        R, Rb = _matrix(_qmul(qb, qs), T), _matrix(qb, T)
        arm = [(Rb[a][0] * ps[0] + Rb[a][1] * ps[1]) + Rb[a][2] * ps[2] for a in range(3)]
        vs = [vb[0] + (wb[1] * arm[2] - wb[2] * arm[1]), vb[1] + (wb[2] * arm[0] - wb[0] * arm[2]), vb[2] + (wb[0] * arm[1] - wb[1] * arm[0])]
        st = state["imu"][:, i]
        ug, ua = draws.block(S + 12), draws.block(S + 13)
        vp = [np.where(rs, vs[a], st[:, a]) for a in range(3)]
        bg = [np.where(rs, _usym(ug[a], b0g), st[:, 3 + a]) for a in range(3)]
        ba = [np.where(rs, _usym(ua[a], b0a), st[:, 6 + a]) for a in range(3)]
        accw = [((vs[a] - vp[a]) * inv_dt) - g[a] for a in range(3)]
        m = np.zeros((n, 6), T)
        for a in range(3):
            gw = (R[0][a] * wb[0] + R[1][a] * wb[1]) + R[2][a] * wb[2]
            aw = (R[0][a] * accw[0] + R[1][a] * accw[1]) + R[2][a] * accw[2]
            m[:, a] = (gw + bg[a]) + (sg * draws.gauss(S + a))
            m[:, 3 + a] = (aw + ba[a]) + (sa * draws.gauss(S + 3 + a))
        o = _latency(_ring(st[:, 9:], (n, L, 6)), h, Dl[:, 0], rs, m)
        for a in range(3):
            st[:, a] = vs[a]
            st[:, 3 + a] = bg[a] + (wg * draws.gauss(S + 6 + a))
            st[:, 6 + a] = ba[a] + (wa * draws.gauss(S + 9 + a))
        out[:, 3 * i:3 * i + 3] = o[:, :3]
        out[:, 3 * I + 3 * i:3 * I + 3 * i + 3] = o[:, 3:]
    # 2. encoders, all dofs at once: arrays (n, nd)
    S = STREAM_ENC + 4 * np.arange(nd)
    st = state["enc"]
    q, qd = dof_state[:, :, 0], dof_state[:, :, 1]
    off = np.where(rs[:, None], _usym(draws.block(S + 2)[0], o_rng), st[:, :, 0])
    st[:, :, 0] = off
    x = (q + off) + (sq * draws.gauss(S))
    if res > 0:
        x = res * np.rint(x * inv_res)
    if cfg["velocity"] == "difference":
        prev = np.where(rs[:, None], x, st[:, :, 1])
        v = (x - prev) * inv_dt
    else:
        v = qd + (sv * draws.gauss(S + 1))
    m = np.stack([x, v], -1).reshape(n * nd, 2)
    rep = lambda a: np.repeat(a, nd)
    o = _latency(_ring(st[:, :, 2:], (n * nd, L, 2)), rep(h), rep(Dl[:, 1]), rep(rs), m).reshape(n, nd, 2)
    st[:, :, 1] = x
    out[:, 6 * I:6 * I + nd] = o[:, :, 0]
    out[:, 6 * I + nd:6 * I + 2 * nd] = o[:, :, 1]
    # 3. feet
    base = 6 * I + 2 * nd
    for k, b in enumerate(feet):
        fx, fy, fz = contact[:, b, 0], contact[:, b, 1], contact[:, b, 2]
        s = fz * np.abs(fz) if cfg["contact_mode"] == "z" else (fx * fx + fy * fy) + fz * fz
        st = state["foot"][:, k]
        zero = T(0.0)
        p = np.where(rs, False, st[:, 0] != 0)
        air, con, lair, lcon = (np.where(rs, zero, st[:, j]) for j in (1, 2, 3, 4))
        on = np.where(s > on2, True, np.where(s < off2, False, p))
        first, left = on & ~p & ~rs, p & ~on
        lair = np.where(first, air + dt, lair)
        lcon = np.where(left, con + dt, lcon)
        air = np.where(on, zero, air + dt)
        con = np.where(on, con + dt, zero)
        m = np.stack([on.astype(T), first.astype(T), air, con, lair, lcon], -1)
        o = _latency(_ring(st[:, 5:], (n, L, 6)), h, Dl[:, 2], rs, m)
        st[:, :5] = np.stack([m[:, 0], air, con, lair, lcon], -1)
        for j in range(6):
            out[:, base + j * F + k] = o[:, j]
        sw[:, k], sw[:, F + k] = o[:, 0] != 0, o[:, 1] != 0
    cnt[:, :, 0] = (c + np.uint32(1)).view(np.int32)[:, None]
    cnt[:, :, 1] = np.where(h + 1 == L, 0, h + 1)[:, None]
    return out, sw


def step32(cfg, params, state, body_state, dof_state, contact, delay, reset=None, gids=None):
    """One read in float32, bit-equal to the kernel: (out (n, D) float32, switches (n, 2 F) uint8); state updated in place."""
    assert all(state[k].dtype == np.float32 for k in ("imu", "enc", "foot"))
    return _step(np.float32, cfg, params, state, body_state, dof_state, contact, delay, reset, gids)


def step64(cfg, params, state, body_state, dof_state, contact, delay, reset=None, gids=None):
    """The same text in float64 (state tensors float64)."""
    assert all(state[k].dtype == np.float64 for k in ("imu", "enc", "foot"))
    return _step(np.float64, cfg, params, state, body_state, dof_state, contact, delay, reset, gids)


def split(out, num_imus, nd, num_feet):
    """The named parts of a packed output row (views)."""
    n, I, F = out.shape[0], num_imus, num_feet
    o = dict(gyro=out[:, :3 * I].reshape(n, I, 3), accel=out[:, 3 * I:6 * I].reshape(n, I, 3), dof_pos=out[:, 6 * I:6 * I + nd],
             dof_vel=out[:, 6 * I + nd:6 * I + 2 * nd])
    for j, k in enumerate(("contact", "first_contact", "air_time", "contact_time", "last_air_time", "last_contact_time")):
        o[k] = out[:, 6 * I + 2 * nd + j * F:6 * I + 2 * nd + (j + 1) * F]
    return o


def synthetic(gids, nb, nd, k, dt=0.02):
    """Smooth test motions for read k, a function of the GLOBAL env id alone (so that shards, subsets and permutations of envs
    see the rows the full batch sees): (body_state (n, nb, 13), dof_state (n, nd, 2), contact (n, nb, 3)) float32.  Unit
    quaternions, velocities of a few m/s and rad/s, contact forces that cross a threshold of a few newtons both ways."""
    g = np.asarray(gids, np.float64).reshape(-1, 1, 1)
    t = k * dt
    b, ch = np.arange(nb).reshape(1, -1, 1), np.arange(13).reshape(1, 1, -1)
    body = np.sin(0.7 * g + 1.3 * b + 0.9 * ch + (1.0 + 0.1 * ch) * 3.0 * t)
    body[..., 6] += 1.5
    body[..., 3:7] /= np.linalg.norm(body[..., 3:7], axis=-1, keepdims=True)
    body[..., 7:10] *= 1.5
    body[..., 10:13] *= 3.0
    d, c2 = np.arange(nd).reshape(1, -1, 1), np.arange(2).reshape(1, 1, -1)
    dof = np.sin(0.3 * g + 0.5 * d + 1.1 * c2 + 2.0 * t) * np.array([1.0, 5.0])
    con = np.array([1.5, 1.5, 8.0]) * np.sin(0.45 * g + 0.8 * b + 1.7 * np.arange(3).reshape(1, 1, -1) + 9.0 * t)
    return body.astype(np.float32), dof.astype(np.float32), con.astype(np.float32)
