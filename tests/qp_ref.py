"""References of the foot-force QP (csrc/shf_qp.hip: shf_foot_force_qp), NumPy only.

Per env, F feet, x = (f_1, .., f_F) in world axes (z up), r_f = p_foot_f - p_root, G = [[I .. I], [[r_1]x .. [r_F]x]]:

    minimise  1/2 (G f - w)^T S (G f - w) + 1/2 alpha |f|^2 + 1/2 beta |f - f_prev|^2
    stance:   fz_min <= f_z <= fz_max,  |f_x| <= mu f_z,  |f_y| <= mu f_z          swing:  f = 0

* `twin`: the kernel's algorithm (ADMM in OSQP form, a fixed number of sweeps), the same operations in the same order, in
  the dtype asked for (float64 by default; float32 to see what the number format alone does).
* `exact`: the optimum by an active-set search whose every answer is verified against the KKT conditions (stationarity,
  feasibility, multiplier signs, each to 1e-9 relative).  It shares nothing with `twin` but the problem statement.
* `wrench`, `efforts`: the wanted base wrench and the joint efforts around the QP, closed forms.
"""
import itertools

import numpy as np

from tests import cone_ref as CR
from tests.cone_ref import RELAX, SIGMA_C              # the sweep's constants live with the sweep (re-exported)

RHO_C, ITERS = 1.0, 100                                # the kernel's constant (csrc/shf_qp.hip) and glue's default sweeps


# ------------------------------------------------------------------------------------------------------ the problem --
def grasp(r):
    """G (6, 3F) of one env from r (F, 3)."""
    F = r.shape[0]
    G = np.zeros((6, 3 * F), r.dtype)
    for f in range(F):
        x, y, z = r[f]
        G[:3, 3 * f:3 * f + 3] = np.eye(3)
        G[3:, 3 * f:3 * f + 3] = [[0, -z, y], [z, 0, -x], [-y, x, 0]]
    return G


def cost(r, w, S, alpha, beta, f_prev, f):
    """The objective of one env at f (F, 3), float64."""
    e = grasp(np.asarray(r, np.float64)) @ f.reshape(-1) - w
    c = 0.5 * e @ (np.asarray(S, np.float64) * e) + 0.5 * alpha * (f ** 2).sum()
    if f_prev is not None and beta > 0:
        c += 0.5 * beta * ((f - f_prev) ** 2).sum()
    return c


def quat_mul(a, b):
    x1, y1, z1, w1 = np.moveaxis(a, -1, 0)
    x2, y2, z2, w2 = np.moveaxis(b, -1, 0)
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], -1)


def orientation_error(desired, current):
    """shf_ik_dls's: the vector part of desired * conj(current), signed by its scalar part (xyzw)."""
    qr = quat_mul(desired, current * np.array([-1.0, -1.0, -1.0, 1.0]))
    return qr[..., :3] * np.sign(qr[..., 3:4])


def wrench(M, h, root, target, gains):
    """w (n, 6) = M[0:6, 0:6] (a_lin, a_ang) + h[0:6]; root / target rows (pos, quat xyzw, v, omega), gains (4, 3) =
    (kp_lin, kd_lin, kp_ang, kd_ang).  The dof accelerations' coupling M[0:6, 6:] qdd is neglected."""
    root, target, g = np.asarray(root, np.float64), np.asarray(target, np.float64), np.asarray(gains, np.float64).reshape(4, 3)
    a = np.concatenate([g[0] * (target[:, :3] - root[:, :3]) + g[1] * (target[:, 7:10] - root[:, 7:10]),
                        g[2] * orientation_error(target[:, 3:7], root[:, 3:7]) + g[3] * (target[:, 10:13] - root[:, 10:13])], 1)
    return np.einsum("nij,nj->ni", np.asarray(M, np.float64)[:, :6, :6], a) + np.asarray(h, np.float64)[:, :6]


def efforts(J, f, bias=None, limit=None):
    """(free, clamped): tau = -sum_f Jl_f^T f_f over the dof columns of the linear rows of J (n, F, 6, nd + 6), + bias[:, 6:],
    then the clamp to +-limit (entries <= 0: none)."""
    J = np.asarray(J, np.float64)
    tau = -np.einsum("nfkd,nfk->nd", J[:, :, :3, 6:], np.asarray(f, np.float64))
    if bias is not None:
        tau = tau + np.asarray(bias, np.float64)[:, 6:]
    out = tau
    if limit is not None:
        lim = np.where(np.asarray(limit, np.float64) > 0, np.asarray(limit, np.float64), np.inf)
        out = np.maximum(np.minimum(tau, lim), -lim)
    return tau, out


# --------------------------------------------------------------------------------------------------------- the twin --
def twin(r, w, S, alpha, beta, f_prev, stance, mu, fz_min, fz_max, iters=ITERS, dtype=np.float64, return_state=False):
    """The kernel's sweeps, batched over envs: r (n, F, 3), w (n, 6), S (6), stance (n, F), mu (n) or scalar -> f (n, F, 3).
    Every step below is one line of k_foot_force_qp, in its order; nothing is fused."""
    T = dtype
    r, w, S = np.asarray(r, T), np.asarray(w, T), np.asarray(S, T)
    n, F, _ = r.shape
    N = 3 * F
    st = np.asarray(stance).astype(bool)
    s = st.astype(T)
    mu = np.maximum(np.broadcast_to(np.asarray(mu, T), (n,)), T(0))
    be = T(beta) if f_prev is not None else T(0)
    ab = T(alpha) + be
    zero, one = np.zeros(n, T), np.ones(n, T)
    # G, column 3 f + k, rows 0..5; a swing foot's columns are zero
    G = [[zero] * N for _ in range(6)]
    for f in range(F):
        x, y, z = r[:, f, 0] * s[:, f], r[:, f, 1] * s[:, f], r[:, f, 2] * s[:, f]
        for k in range(3):
            G[k][3 * f + k] = s[:, f]
        G[3][3 * f + 1], G[3][3 * f + 2] = -z, y
        G[4][3 * f + 0], G[4][3 * f + 2] = z, -x
        G[5][3 * f + 0], G[5][3 * f + 1] = -y, x
    sw = [S[c] * w[:, c] for c in range(6)]
    P = [[None] * N for _ in range(N)]
    q = [None] * N
    for i in range(N):
        for j in range(i + 1):
            acc = G[0][i] * S[0] * G[0][j]
            for c in range(1, 6):
                acc = acc + G[c][i] * S[c] * G[c][j]
            P[i][j] = acc + ab if i == j else acc
        acc = G[0][i] * sw[0]
        for c in range(1, 6):
            acc = acc + G[c][i] * sw[c]
        q[i] = -acc
        if f_prev is not None:
            q[i] = q[i] - be * (np.asarray(f_prev, T)[:, i // 3, i % 3] * s[:, i // 3])
    # rho = RHO_C sqrt((alpha + beta) m), sigma = SIGMA_C m, m = the mean diagonal of P over the stance feet's variables
    tr, ns = zero, zero
    for i in range(N):
        tr = tr + P[i][i] * s[:, i // 3]
    for f in range(F):
        ns = ns + s[:, f]
    mean = tr / (T(3) * np.maximum(ns, one))
    mean = np.where(ns > 0, mean, one)
    rho, sigma = T(RHO_C) * np.sqrt(ab * mean), T(SIGMA_C) * mean
    # K = P + sigma I + rho A^T A (diagonal: 2, 2, 1 + 4 mu^2 per foot), K = L D L^T
    dz = one + T(4) * (mu * mu)
    L = [[None] * N for _ in range(N)]
    D, iD = [None] * N, [None] * N
    for j in range(N):
        d = P[j][j] + (sigma + rho * (dz if j % 3 == 2 else T(2)))
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        D[j], iD[j] = d, one / d
        for i in range(j + 1, N):
            v = P[i][j]
            for k in range(j):
                v = v - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = v * iD[j]
    inf = T(np.inf)
    lo = [[np.where(st[:, f], T(fz_min) if m == 0 else T(0), T(0)) for m in range(5)] for f in range(F)]
    hi = [[np.where(st[:, f], T(fz_max) if m == 0 else inf, T(0)) for m in range(5)] for f in range(F)]
    x = [zero] * N
    z = [[zero] * 5 for _ in range(F)]
    y = [[zero] * 5 for _ in range(F)]
    irho = one / rho
    for _ in range(int(iters)):
        b = [None] * N
        for f in range(F):
            add = CR.at(mu, [rho * z[f][m] - y[f][m] for m in range(5)])
            for k in range(3):
                b[3 * f + k] = (sigma * x[3 * f + k] - q[3 * f + k]) + add[k]
        for i in range(N):
            for k in range(i):
                b[i] = b[i] - L[i][k] * b[k]
        for i in range(N):
            b[i] = b[i] * iD[i]
        for i in range(N - 1, -1, -1):
            for k in range(i + 1, N):
                b[i] = b[i] - L[k][i] * b[k]
        for f in range(F):
            zt = CR.rows(mu, b[3 * f], b[3 * f + 1], b[3 * f + 2])
            for k in range(3):
                x[3 * f + k] = CR.relax(b[3 * f + k], x[3 * f + k], T)
            for m in range(5):
                z[f][m], y[f][m] = CR.project(zt[m], z[f][m], y[f][m], rho, irho, lo[f][m], hi[f][m], T)
    out = np.zeros((n, F, 3), T)
    for f in range(F):
        out[:, f, 0], out[:, f, 1], out[:, f, 2] = CR.feasible(st[:, f], mu, x[3 * f], x[3 * f + 1], x[3 * f + 2], fz_min, fz_max, T)
    if return_state:
        return out, {"x": np.stack(x, 1).reshape(n, F, 3), "y": np.stack([np.stack(v, 1) for v in y], 1), "rho": rho, "sigma": sigma}
    return out


def face_distance(f, stance, mu, fz_min, fz_max, x_raw=None):
    """Per env: the smallest distance of a stance foot's (unclamped, when given) force to a constraint face it is not meant to
    lie on, relative to the env's largest force: min over |f_z - fz_min|, |f_z - fz_max|, |mu f_z -+ f_x|, |mu f_z -+ f_y|."""
    g = np.asarray(f if x_raw is None else x_raw, np.float64)
    n, F, _ = g.shape
    mu = np.broadcast_to(np.asarray(mu, np.float64), (n,))[:, None]
    fz = g[..., 2]
    d = np.stack([np.abs(fz - fz_min), np.abs(fz - fz_max) if np.isfinite(fz_max) else np.full_like(fz, np.inf),
                  np.abs(mu * fz - g[..., 0]), np.abs(mu * fz + g[..., 0]), np.abs(mu * fz - g[..., 1]), np.abs(mu * fz + g[..., 1])], -1)
    d = np.where(np.asarray(stance).astype(bool)[..., None], d, np.inf)
    return d.reshape(n, -1), np.abs(g).reshape(n, -1).max(1)


# ------------------------------------------------------------------------------------------------- the exact optimum --
def _rows(mu, fz_min, fz_max):
    """One stance foot's constraints as (a (3), bound, sign): sign * (a . f - bound) <= 0; grouped in opposing pairs."""
    rows = [((0, 0, 1.0), fz_min, -1.0), ((0, 0, 1.0), fz_max, +1.0),
            ((1.0, 0, -mu), 0.0, +1.0), ((-1.0, 0, -mu), 0.0, +1.0),
            ((0, 1.0, -mu), 0.0, +1.0), ((0, -1.0, -mu), 0.0, +1.0)]
    return rows


def _kkt_solve(P, q, A, b, active):
    m = len(active)
    N = P.shape[0]
    if m == 0:
        return np.linalg.solve(P, -q), np.zeros(0)
    Aw = A[active]
    K = np.block([[P, Aw.T], [Aw, np.zeros((m, m))]])
    try:
        sol = np.linalg.solve(K, np.concatenate([-q, b[active]]))
    except np.linalg.LinAlgError:
        return None, None
    return sol[:N], sol[N:]


def _verify(P, q, A, b, sg, x, active, lam, tol=1e-9):
    """Stationarity, feasibility and multiplier signs, each relative to the problem's scale."""
    scale = max(np.abs(q).max(), np.abs(P @ x).max(), 1e-300)
    xs = max(np.abs(x).max(), 1e-300)
    g = P @ x + q + (A[active].T @ lam if len(active) else 0.0)
    viol = sg * (A @ x - b)
    viol = viol[np.isfinite(b)]
    ok = np.abs(g).max() <= tol * scale and (viol.max() if viol.size else 0.0) <= tol * xs
    if len(active):
        ok = ok and (sg[active] * lam).min() >= -tol * scale
    return bool(ok)


def exact(r, w, S, alpha, beta, f_prev, stance, mu, fz_min, fz_max, guess=None):
    """The optimum of ONE env, float64: f (F, 3).  The swing feet are eliminated; over the stance feet a primal active set is
    searched -- from `guess` (a force near the optimum, e.g. the twin's, read for which faces it touches) by adding the most
    violated and dropping the worst-signed constraint, then, if that does not verify, by enumerating every set with at most one
    of each opposing pair per foot (27 per foot).  Only a KKT-verified point is returned; otherwise RuntimeError."""
    r, w, S = np.asarray(r, np.float64), np.asarray(w, np.float64), np.asarray(S, np.float64)
    F = r.shape[0]
    feet = [f for f in range(F) if stance[f]]
    out = np.zeros((F, 3))
    if not feet:
        return out
    G = grasp(r[feet])
    N = 3 * len(feet)
    be = beta if f_prev is not None else 0.0
    P = G.T @ (S[:, None] * G) + (alpha + be) * np.eye(N)
    q = -G.T @ (S * w)
    if f_prev is not None:
        q = q - be * np.asarray(f_prev, np.float64)[feet].reshape(-1)
    A, b, sg = [], [], []
    for i in range(len(feet)):
        for a3, bound, sign in _rows(float(mu), float(fz_min), float(fz_max)):
            row = np.zeros(N)
            row[3 * i:3 * i + 3] = a3
            A.append(row); b.append(bound); sg.append(sign)
    A, b, sg = np.array(A), np.array(b), np.array(sg)
    fin = np.isfinite(b)
    bz = np.where(fin, b, 0.0)

    def attempt(active):
        x, lam = _kkt_solve(P, q, A, bz, active)
        if x is None:
            return None
        return x if _verify(P, q, A, b, sg, x, active, lam) else None

    active = []
    if guess is not None:
        gx = np.asarray(guess, np.float64)[feet].reshape(-1)
        slack = np.where(fin, np.abs(A @ gx - bz), np.inf)
        active = [int(i) for i in np.nonzero(slack <= 1e-3 * max(np.abs(gx).max(), 1.0))[0]]
        # one of each opposing pair at most
        active = [i for i in active if not (i % 2 == 1 and i - 1 in active)]
    for _ in range(60):
        x, lam = _kkt_solve(P, q, A, bz, active)
        if x is None:
            break
        if _verify(P, q, A, b, sg, x, active, lam):
            out[feet] = x.reshape(-1, 3)
            return out
        viol = np.where(fin, sg * (A @ x - bz), -np.inf)
        viol[active] = -np.inf
        worst = int(np.argmax(viol))
        if viol[worst] > 1e-12 * max(np.abs(x).max(), 1.0):
            partner = worst ^ 1
            active = [i for i in active if i != partner] + [worst]
            continue
        signs = sg[active] * lam
        active = [i for k, i in enumerate(active) if k != int(np.argmin(signs))]
    # enumeration: per foot, each opposing pair is free, at its first or at its second face
    per_foot = list(itertools.product((None, 0, 1), repeat=3))
    for combo in itertools.product(per_foot, repeat=len(feet)):
        act = [6 * i + 2 * p + side for i, c in enumerate(combo) for p, side in enumerate(c) if side is not None]
        if any(not fin[i] for i in act):
            continue
        x = attempt(act)
        if x is not None:
            out[feet] = x.reshape(-1, 3)
            return out
    raise RuntimeError("exact: no active set satisfies the KKT conditions")


# ------------------------------------------------------------------------------------------------- seeded problems --
A1_FEET = np.array([[0.183, 0.13, -0.30], [0.183, -0.13, -0.30], [-0.183, 0.13, -0.30], [-0.183, -0.13, -0.30]])
A1_WEIGHT = 12.45 * 9.81
STANCES = {"all": (1, 1, 1, 1), "diagonal": (1, 0, 0, 1), "three": (1, 1, 0, 1)}


def a1_problems(n, seed, stance):
    """n A1-like problems: foot offsets within 6 cm of the A1's stance, wanted wrench = the weight plus pushes (up to 40 N
    and 10 N m), friction 0.4 .. 1."""
    rng = np.random.default_rng(seed)
    r = A1_FEET[None] + rng.uniform(-0.06, 0.06, (n, 4, 3))
    w = np.concatenate([rng.uniform(-40, 40, (n, 2)), A1_WEIGHT + rng.uniform(-40, 40, (n, 1)), rng.uniform(-10, 10, (n, 3))], 1)
    mu = rng.uniform(0.4, 1.0, n)
    return r, w, mu, np.tile(np.array(stance, np.uint8), (n, 1))
