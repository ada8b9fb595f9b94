"""References of the horizon MPC (csrc/shf_mpc.hip: shf_mpc_horizon, shf_foot_force_mpc, shf_foot_force_efforts), NumPy only.

* `horizon`: k_mpc_horizon's text -- the contact, reference and foothold tables over the horizon.
* `rollout`: the recurrences of the problem statement, literally, for given forces u: the states x_0 .. x_H.
* `condense`: steps 1 to 4 of k_foot_force_mpc (P, q and what they are built from), in the dtype asked for.
* `twin`: the kernel's algorithm, the same operations in the same order, in the dtype asked for.
* `certified`: the float64 optimum by other means -- the condensed problem is formed from `rollout` alone (x is affine in u),
  a long ADMM run with another penalty finds which faces are touched, and an active-set polish whose every answer is
  verified against the KKT conditions (tests/qp_ref._verify: stationarity, feasibility, multiplier signs, each to 1e-9
  relative; complementarity holds by construction: a multiplier is non-zero only on a face solved as an equality).  It
  shares nothing with `twin` but the problem statement.
"""
import numpy as np

from tests import cone_ref as CR
from tests import qp_ref as Q
from tests.cone_ref import RELAX, SIGMA_C              # the sweep's constants live with the sweep (re-exported)

# glue's defaults (DESIGN.md 8h "Horizon MPC" says where each comes from)
HORIZON, ITERS, ALPHA, EVERY = 10, 100, 1e-5, 1
WEIGHTS12 = (25.0, 25.0, 10.0, 2.0, 2.0, 50.0, 0.0, 0.0, 0.3, 0.2, 0.2, 0.2)
MAX_HORIZON = 10
# the float32 twin's distance from the float64 twin at the default sweeps, the worst over the seeded problems of
# tests/test_mpc_host.py (which measures and asserts it): step 0's forces over the largest force, the efforts -J^T f over the
# largest effort.  Four times this is the GPU tests' bound.
F32_DIST = {"forces": 3.1e-3, "efforts": 1.4e-3}


# ------------------------------------------------------------------------------------------------------ the horizon --
def horizon(tick, target, yaw, period, offsets, stance_ticks, stance, feet, command, nominal, P, H, S, dtype=np.float64):
    """tick (n) as shf_gait_plan left it (already advanced), target (n, 13), yaw (n), stance (n, F) this tick's, feet (n, F, 3),
    command (n, 3), nominal (F, 3), P the dict of gait_ref.params -> contact (n, H, F) uint8, xref (n, H + 1, 12), pos (n, H, F, 3)."""
    T = dtype
    target, yaw, feet, command, nominal = (np.asarray(a, T) for a in (target, yaw, feet, command, nominal))
    n, F = feet.shape[:2]
    offsets, stance_ticks = np.asarray(offsets, np.int64), np.asarray(stance_ticks, np.int64)
    dt = T(P["dt"])
    delta = T(S) * dt
    xref = np.zeros((n, H + 1, 12), T)
    for k in range(H + 1):
        kd = T(k) * delta
        xref[:, k, 2] = yaw + kd * target[:, 12]
        xref[:, k, 3], xref[:, k, 4], xref[:, k, 5] = target[:, 0] + kd * target[:, 7], target[:, 1] + kd * target[:, 8], target[:, 2]
        xref[:, k, 6:9], xref[:, k, 9:12] = target[:, 10:13], target[:, 7:10]
    tm = (np.asarray(tick, np.int64) - 1) % period                     # this tick's clock; numpy's % is non-negative
    contact = np.zeros((n, H, F), np.uint8)
    pos = np.zeros((n, H, F, 3), T)
    cvx, cvy, cwz = command[:, 0], command[:, 1], command[:, 2]
    for f in range(F):
        prev = np.zeros(n, bool)
        hold = np.zeros((n, 3), T)
        for k in range(H):
            phi = (tm + (k * S) % period + offsets[f]) % period
            c = (np.asarray(stance)[:, f] != 0) if k == 0 else phi < stance_ticks[f]
            if k == 0:
                hold = np.where(c[:, None], feet[:, f], hold)
            else:
                kd = T(k) * delta
                psi = yaw + kd * target[:, 12]
                cs, sn = np.cos(psi), np.sin(psi)
                nwx, nwy = cs * nominal[f, 0] - sn * nominal[f, 1], sn * nominal[f, 0] + cs * nominal[f, 1]
                hx, hy = (target[:, 0] + kd * target[:, 7]) + nwx, (target[:, 1] + kd * target[:, 8]) + nwy
                vdx, vdy = (cs * cvx - sn * cvy) - cwz * nwy, (sn * cvx + cs * cvy) + cwz * nwx
                half = (T(stance_ticks[f]) * dt) * T(0.5)
                gx, gy = vdx * half, vdy * half
                m = np.sqrt(gx * gx + gy * gy)
                with np.errstate(divide="ignore", invalid="ignore"):
                    q = T(P["max_step"]) / m
                    big = m > T(P["max_step"])
                    gx, gy = np.where(big, gx * q, gx), np.where(big, gy * q, gy)
                new = np.stack([hx + gx, hy + gy, np.full(n, T(P["touchdown_z"]))], 1)
                hold = np.where((c & ~prev)[:, None], new, hold)
            contact[:, k, f] = c
            pos[:, k, f] = np.where(c[:, None], hold, T(0))
            prev = c
    return contact, xref, pos


def problem(contact, xref, pos, root, M, h, delta):
    """The inputs of the solve as one dict (root (n, 13) rows, M (n, D, D) and h (n, D) of shf_sim_floating_dynamics or their
    leading 6 x 6 / 6)."""
    return {"contact": np.asarray(contact), "xref": np.asarray(xref, np.float64), "pos": np.asarray(pos, np.float64),
            "root": np.asarray(root, np.float64), "M6": np.asarray(M, np.float64)[:, :6, :6], "h6": np.asarray(h, np.float64)[:, :6],
            "delta": float(delta)}


def initial_state(root, psi0, T=np.float64):
    """x_0 (n, 12) = (ZYX angles with the yaw unwrapped to within pi of psi0, p, omega, v) of root rows (pos, quat xyzw, v, omega)."""
    root = np.asarray(root, T)
    qx, qy, qz, qw = (root[:, 3 + k] for k in range(4))
    R20, R21 = T(2) * (qx * qz - qw * qy), T(2) * (qy * qz + qw * qx)
    R22 = T(1) - T(2) * (qx * qx + qy * qy)
    R10, R00 = T(2) * (qx * qy + qw * qz), T(1) - T(2) * (qy * qy + qz * qz)
    x = np.zeros((root.shape[0], 12), T)
    x[:, 0], x[:, 1] = np.arctan2(R21, R22), np.arcsin(np.minimum(np.maximum(-R20, T(-1)), T(1)))
    yaw = np.arctan2(R10, R00)
    x[:, 2] = yaw + np.rint((np.asarray(psi0, T) - yaw) * T(0.15915494309189535)) * T(6.283185307179586)
    x[:, 3:6], x[:, 6:9], x[:, 9:12] = root[:, 0:3], root[:, 10:13], root[:, 7:10]
    return x


def rollout(prob, u):
    """x (n, H + 1, 12), float64: the recurrences of the problem statement for forces u (n, H, F, 3) (contact applied here)."""
    c, xref, pos, root = prob["contact"], prob["xref"], prob["pos"], prob["root"]
    n, H, F = c.shape
    d = prob["delta"]
    x = np.zeros((n, H + 1, 12))
    x[:, 0] = initial_state(root, xref[:, 0, 2])
    for k in range(H):
        wr = -prob["h6"].copy()
        for f in range(F):
            r = pos[:, k, f] - (root[:, :3] + xref[:, k, 3:6] - xref[:, 0, 3:6])
            uf = u[:, k, f] * c[:, k, f, None]
            wr[:, :3] += uf
            wr[:, 3:] += np.cross(r, uf)
        acc = np.linalg.solve(prob["M6"], wr[..., None])[..., 0]
        psi = xref[:, k, 2]
        cs, sn = np.cos(psi), np.sin(psi)
        om, v = x[:, k, 6:9], x[:, k, 9:12]
        x[:, k + 1, 0] = x[:, k, 0] + d * (cs * om[:, 0] + sn * om[:, 1])
        x[:, k + 1, 1] = x[:, k, 1] + d * (-sn * om[:, 0] + cs * om[:, 1])
        x[:, k + 1, 2] = x[:, k, 2] + d * om[:, 2]
        x[:, k + 1, 3:6] = x[:, k, 3:6] + d * v
        x[:, k + 1, 6:9] = om + d * acc[:, 3:]
        x[:, k + 1, 9:12] = v + d * acc[:, :3]
    return x


def cost(prob, u, weights, alpha):
    """The objective (n) at u (n, H, F, 3), float64, by `rollout`."""
    x = rollout(prob, u)
    e = x[:, 1:] - prob["xref"][:, 1:]
    return 0.5 * (e * e * np.asarray(weights, np.float64)).sum((1, 2)) + 0.5 * alpha * ((u * prob["contact"][..., None]) ** 2).sum((1, 2, 3))


# --------------------------------------------------------------------------------------------------------- the twin --
def invert(A):
    """The kernel's in-place Gauss-Jordan sweep without pivoting, batched: (n, N, N) -> the inverses, in A's dtype."""
    A = A.copy()
    for k in range(A.shape[-1]):
        p = A.dtype.type(1) / A[:, k, k]
        row = A[:, k, :] * p[:, None]
        f = A[:, :, k].copy()
        A = A - f[:, :, None] * row[:, None, :]
        A[:, :, k] = -(f * p[:, None])
        A[:, k, :] = row
        A[:, k, k] = p
    return A


def condense(prob, weights, alpha, dtype=np.float64):
    """Steps 1 to 4 of k_foot_force_mpc: {"P" (n, N, N), "q" (n, N), "W" (n, 6, N), "E" (n, H, 12), "cf" (n, N)}."""
    T = dtype
    c = prob["contact"]
    n, H, F = c.shape
    F3, N = 3 * F, 3 * F * H
    xref, pos, root = (np.asarray(prob[k], T) for k in ("xref", "pos", "root"))
    L = np.asarray(weights, T)
    d = T(prob["delta"])
    Mi = invert(np.asarray(prob["M6"], T))
    h6 = np.asarray(prob["h6"], T)
    g = np.zeros((n, 6), T)
    for r in range(6):
        acc = Mi[:, r, 0] * h6[:, 0]
        for k in range(1, 6):
            acc = acc + Mi[:, r, k] * h6[:, k]
        g[:, r] = -acc
    # 2. the free response
    x = initial_state(root, xref[:, 0, 2], T)
    CA, CB = np.zeros((n, H + 1), T), np.zeros((n, H + 1), T)
    E = np.zeros((n, H, 12), T)
    for s in range(H):
        psi = xref[:, s, 2]
        cs, sn = np.cos(psi), np.sin(psi)
        t0, t1 = cs * x[:, 6] + sn * x[:, 7], cs * x[:, 7] - sn * x[:, 6]
        x[:, 0], x[:, 1], x[:, 2] = x[:, 0] + d * t0, x[:, 1] + d * t1, x[:, 2] + d * x[:, 8]
        x[:, 3:6] = x[:, 3:6] + d * x[:, 9:12]
        x[:, 6:9], x[:, 9:12] = x[:, 6:9] + d * g[:, 3:6], x[:, 9:12] + d * g[:, 0:3]
        CA[:, s + 1], CB[:, s + 1] = CA[:, s] + cs, CB[:, s] + sn
        E[:, s] = x - xref[:, s + 1]
    # 3. W, TX, TY
    ki = np.arange(N) // F3
    fi = (np.arange(N) % F3) // 3
    ci = np.arange(N) % 3
    cf = c[:, ki, fi].astype(T)                                            # (n, N)
    r = pos[:, ki, fi] - (root[:, None, :3] + (xref[:, ki, 3:6] - xref[:, :1, 3:6]))     # (n, N, 3)
    zero = np.zeros((n, N), T)
    a0 = np.where(ci == 0, zero, np.where(ci == 1, -r[..., 2], r[..., 1]))
    a1 = np.where(ci == 0, r[..., 2], np.where(ci == 1, zero, -r[..., 0]))
    a2 = np.where(ci == 0, -r[..., 1], np.where(ci == 1, r[..., 0], zero))
    W = np.zeros((n, 6, N), T)
    for q_ in range(6):
        mc = Mi[:, q_, :3][:, ci]                                          # (n, N)
        W[:, q_] = (d * (mc + ((Mi[:, q_, 3:4] * a0 + Mi[:, q_, 4:5] * a1) + Mi[:, q_, 5:6] * a2))) * cf
    TX, TY = np.zeros((n, H + 1, N), T), np.zeros((n, H + 1, N), T)        # index s = 1..H
    for s in range(1, H + 1):
        a, b = CA[:, s, None] - CA[:, ki + 1], CB[:, s, None] - CB[:, ki + 1]
        on = (s > ki + 1)[None]
        TX[:, s] = np.where(on, a * W[:, 3] + b * W[:, 4], zero)
        TY[:, s] = np.where(on, a * W[:, 4] - b * W[:, 3], zero)
    # 4. P, q
    dd = d * d
    wLv = [W[:, k] * L[9 + k] for k in range(3)]
    wLw = [W[:, 3 + k] * L[6 + k] for k in range(3)]
    wLp = [W[:, k] * L[3 + k] for k in range(3)]
    wLz = W[:, 5] * L[2]
    m = np.maximum(ki[:, None], ki[None, :])
    S0 = (H - m).astype(T)[None]
    s2 = np.zeros((N, N), np.int64)
    for s in range(1, H + 1):
        s2 += np.where(s > m, (s - 1 - ki[:, None]) * (s - 1 - ki[None, :]), 0)
    d2 = dd * s2.astype(T)[None]
    o = lambda a, b: a[:, :, None] * b[:, None, :]
    dv = (o(wLv[0], W[:, 0]) + o(wLv[1], W[:, 1])) + o(wLv[2], W[:, 2])
    dw = (o(wLw[0], W[:, 3]) + o(wLw[1], W[:, 4])) + o(wLw[2], W[:, 5])
    dp = (o(wLp[0], W[:, 0]) + o(wLp[1], W[:, 1])) + o(wLp[2], W[:, 2])
    dz = o(wLz, W[:, 5])
    th = np.zeros((n, N, N), T)
    for s in range(1, H + 1):                      # TX, TY are exact zeros for s <= max(k_i, k_j) + 1: adding them changes nothing
        th = th + (o(L[0] * TX[:, s], TX[:, s]) + o(L[1] * TY[:, s], TY[:, s]))
    P = (S0 * (dw + dv) + d2 * (dp + dz)) + dd * th
    P[:, np.arange(N), np.arange(N)] = P[:, np.arange(N), np.arange(N)] + T(alpha)
    q = np.zeros((n, N), T)
    for s in range(1, H + 1):
        nn = (s - 1 - ki).astype(T)[None]
        Es = E[:, s - 1]
        lx, ly = L[0] * TX[:, s], L[1] * TY[:, s]
        pa = d * ((lx * Es[:, 0:1] + ly * Es[:, 1:2]) + nn * (wLz * Es[:, 2:3]))
        pb = (d * nn) * ((wLp[0] * Es[:, 3:4] + wLp[1] * Es[:, 4:5]) + wLp[2] * Es[:, 5:6])
        pc = ((wLw[0] * Es[:, 6:7] + wLw[1] * Es[:, 7:8]) + wLw[2] * Es[:, 8:9]) \
            + ((wLv[0] * Es[:, 9:10] + wLv[1] * Es[:, 10:11]) + wLv[2] * Es[:, 11:12])
        q = np.where((s > ki)[None], q + ((pa + pb) + pc), q)
    return {"P": P, "q": q, "W": W, "E": E, "cf": cf}


def twin(prob, mu, weights, alpha, fz_min, fz_max, iters=ITERS, dtype=np.float64, u0=None, warm_shift=0, return_state=False):
    """k_foot_force_mpc's steps, batched over envs: the clamped solution u (n, H, F, 3); u[:, 0] is forces_out."""
    T = dtype
    c = prob["contact"]
    n, H, F = c.shape
    F3, N = 3 * F, 3 * F * H
    N4 = (N + 3) & ~3
    C = condense(prob, weights, alpha, T)
    P, q, cf = C["P"], C["q"], C["cf"]
    ci = np.arange(N) % 3
    con = cf != 0
    mu = np.maximum(np.broadcast_to(np.asarray(mu, T), (n,)), T(0)).astype(T)
    dgl = P[:, np.arange(N), np.arange(N)]
    tr, nc = np.zeros(n, T), np.zeros(n, T)
    for j in range(N):
        tr, nc = tr + dgl[:, j] * cf[:, j], nc + cf[:, j]
    mean = tr / np.maximum(nc, T(1))
    mean = np.where(nc > 0, mean, T(1)).astype(T)
    rho, sigma = np.sqrt(T(alpha) * mean), T(SIGMA_C) * mean
    K = P.copy()
    ata = np.where(ci[None] == 2, (T(1) + T(4) * (mu * mu))[:, None], T(2)).astype(T)
    K[:, np.arange(N), np.arange(N)] = dgl + (sigma[:, None] + rho[:, None] * ata)
    Kinv = np.zeros((n, N, N4), T)
    Kinv[:, :, :N] = invert(K)
    x = np.zeros((n, N), T)
    if u0 is not None:
        kk = np.minimum(np.arange(H) + int(warm_shift), H - 1)
        x = np.where(con, np.asarray(u0, T)[:, kk].reshape(n, N), T(0)).astype(T)
    mu_ = mu[:, None]

    def rows(v):                                   # A v of every (k, f): (n, H F, 5)
        v = v.reshape(n, H * F, 3)
        return np.stack(CR.rows(mu_, v[..., 0], v[..., 1], v[..., 2]), -1)

    z, y = rows(x), np.zeros((n, H * F, 5), T)
    cfoot = con.reshape(n, H * F, 3)[..., 0]
    inf = T(np.inf)
    lo = np.zeros((n, H * F, 5), T)
    hi = np.zeros((n, H * F, 5), T)
    lo[..., 0] = np.where(cfoot, T(fz_min), T(0))
    hi[..., 0] = np.where(cfoot, T(fz_max), T(0))
    hi[..., 1:] = np.where(cfoot, inf, T(0))[..., None]
    irho = (T(1) / rho)[:, None, None]
    rho3, rho2 = rho[:, None, None], rho[:, None]
    for _ in range(int(iters)):
        add = np.stack(CR.at(mu_, np.moveaxis(rho3 * z - y, -1, 0)), -1).reshape(n, N)
        b = np.zeros((n, N4), T)
        b[:, :N] = (sigma[:, None] * x - q) + add
        s = [np.zeros((n, N), T) for _ in range(4)]
        for j4 in range(N4 // 4):
            for l in range(4):
                s[l] = s[l] + Kinv[:, :, 4 * j4 + l] * b[:, 4 * j4 + l, None]
        xt = (s[0] + s[1]) + (s[2] + s[3])
        zt = rows(xt)
        x = CR.relax(xt, x, T)
        z, y = CR.project(zt, z, y, rho3, irho, lo, hi, T)
    xv = x.reshape(n, H * F, 3)
    u = np.stack(CR.feasible(cfoot, mu_, xv[..., 0], xv[..., 1], xv[..., 2], fz_min, fz_max, T), -1).astype(T).reshape(n, H, F, 3)
    if return_state:
        return u, {"x": x.reshape(n, H, F, 3), "rho": rho2, "sigma": sigma, "P": P, "q": q}
    return u


# ------------------------------------------------------------------------------------------------ the certified optimum --
def affine(prob):
    """x = a + B u from `rollout` alone: a (n, 12 H), B (n, 12 H, N) (steps 1..H)."""
    c = prob["contact"]
    n, H, F = c.shape
    N = 3 * F * H
    a = rollout(prob, np.zeros((n, H, F, 3)))[:, 1:].reshape(n, -1)
    B = np.zeros((n, 12 * H, N))
    for i in range(N):
        u = np.zeros((n, N))
        u[:, i] = 1.0
        B[:, :, i] = rollout(prob, u.reshape(n, H, F, 3))[:, 1:].reshape(n, -1) - a
    return a, B


def certified(prob, mu, weights, alpha, fz_min, fz_max, guess=None):
    """The optimum u (n, H, F, 3), float64, each env KKT-verified; RuntimeError when an env does not certify."""
    c = prob["contact"]
    n, H, F = c.shape
    N = 3 * F * H
    a, B = affine(prob)
    Lw = np.tile(np.asarray(weights, np.float64), H)
    mu = np.broadcast_to(np.asarray(mu, np.float64), (n,))
    out = np.zeros((n, N))
    for e in range(n):
        on = np.repeat(c[e].reshape(-1) != 0, 3)
        idx = np.nonzero(on)[0]
        if idx.size == 0:
            continue
        Be = B[e][:, idx]
        P = Be.T @ (Lw[:, None] * Be) + alpha * np.eye(idx.size)
        q = Be.T @ (Lw * (a[e] - prob["xref"][e, 1:].reshape(-1)))
        nfoot = idx.size // 3
        A, b, sg = [], [], []
        for i in range(nfoot):
            for a3, bound, sign in Q._rows(float(mu[e]), float(fz_min), float(fz_max)):
                row = np.zeros(idx.size)
                row[3 * i:3 * i + 3] = a3
                A.append(row); b.append(bound); sg.append(sign)
        A, b, sg = np.array(A), np.array(b), np.array(sg)
        fin = np.isfinite(b)
        bz = np.where(fin, b, 0.0)
        # a long ADMM run with another penalty (rho = 0.1 mean diag), on the inequality rows sg (A x - b) <= 0
        if guess is not None:
            gx = np.asarray(guess, np.float64)[e].reshape(-1)[idx]
        else:
            rho = 0.1 * np.trace(P) / idx.size
            Af = A[fin] * sg[fin, None]
            bf = bz[fin] * sg[fin]
            Ki = np.linalg.inv(P + 1e-9 * np.eye(idx.size) + rho * Af.T @ Af)
            gx, z, y = np.zeros(idx.size), np.minimum(0.0, bf), np.zeros(bf.size)
            for _ in range(3000):
                gx = Ki @ (1e-9 * gx - q + Af.T @ (rho * z - y))
                zt = Af @ gx
                z = np.minimum(zt + y / rho, bf)
                y = y + rho * (zt - z)
        slack = np.where(fin, np.abs(A @ gx - bz), np.inf)
        active = [int(i) for i in np.nonzero(slack <= 1e-6 * max(np.abs(gx).max(), 1.0))[0]]
        active = [i for i in active if not (i % 2 == 1 and i - 1 in active)]
        sol = None
        for _ in range(400):
            x, lam = Q._kkt_solve(P, q, A, bz, active)
            if x is None:
                break
            if Q._verify(P, q, A, b, sg, x, active, lam):
                sol = x
                break
            viol = np.where(fin, sg * (A @ x - bz), -np.inf)
            viol[active] = -np.inf
            worst = int(np.argmax(viol))
            if viol[worst] > 1e-12 * max(np.abs(x).max(), 1.0):
                active = [i for i in active if i != (worst ^ 1)] + [worst]
                continue
            signs = sg[active] * lam
            active = [i for k, i in enumerate(active) if k != int(np.argmin(signs))]
        if sol is None:
            raise RuntimeError(f"certified: env {e} did not satisfy the KKT conditions")
        out[e, idx] = sol
    return out.reshape(n, H, F, 3)


# ------------------------------------------------------------------------------------------------- seeded problems --
A1_INERTIA = np.diag([12.45, 12.45, 12.45, 0.11, 0.30, 0.33])        # an A1-like composite base inertia (linear, angular)
GAITS = {"stand": (60, (0, 0, 0, 0), (60,) * 4), "trot": (60, (0, 30, 30, 0), (30,) * 4), "walk": (120, (0, 60, 30, 90), (90,) * 4),
         "bound": (60, (0, 0, 30, 30), (24,) * 4)}          # (period, offsets, stance ticks) at 5 ms; bound with a flight phase
STANCE_OF = {"stand": "all", "trot": "diagonal", "walk": "three"}


def a1_problems(n, seed, gait, H=HORIZON, S=6, dt=0.005):
    """n A1-like problems in the ranges of qp_ref.a1_problems -- feet within 6 cm of the A1's stance, pushes of up to 40 N and
    10 N m on top of the weight in h6, friction 0.4 .. 1 -- under `gait`'s schedule from a random tick, every scheduled foot
    touching; the base within 3 cm, 0.1 rad, 0.3 m/s and 0.5 rad/s of its target, commands up to 0.5 m/s and 0.5 rad/s.
    Returns (prob, mu)."""
    from tests import gait_ref as G
    rng = np.random.default_rng(seed)
    period, offsets, st = GAITS[gait]
    r, w, mu, _ = Q.a1_problems(n, seed, (1, 1, 1, 1))
    yaw = rng.uniform(-np.pi, np.pi, n)
    eul = rng.uniform(-0.1, 0.1, (n, 3))
    eul[:, 2] += yaw
    cr, sr, cp, sp, cy, sy = np.cos(eul[:, 0] / 2), np.sin(eul[:, 0] / 2), np.cos(eul[:, 1] / 2), np.sin(eul[:, 1] / 2), np.cos(eul[:, 2] / 2), np.sin(eul[:, 2] / 2)
    quat = np.stack([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy], 1)
    root = np.zeros((n, 13))
    root[:, :2], root[:, 2] = rng.uniform(-2, 2, (n, 2)), 0.30 + rng.uniform(-0.03, 0.03, n)
    root[:, 3:7] = quat
    command = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.5, 0.5, n)], 1)
    cyw, syw = np.cos(yaw), np.sin(yaw)
    vw = np.stack([cyw * command[:, 0] - syw * command[:, 1], syw * command[:, 0] + cyw * command[:, 1]], 1)
    target = np.zeros((n, 13))
    target[:, :2], target[:, 2] = root[:, :2] + rng.uniform(-0.03, 0.03, (n, 2)), 0.30
    target[:, 5], target[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    target[:, 7:9], target[:, 12] = vw, command[:, 2]
    root[:, 7:9], root[:, 9] = vw + rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-0.3, 0.3, n)
    root[:, 10:13] = rng.uniform(-0.5, 0.5, (n, 3))
    root[:, 12] += command[:, 2]
    Rz = np.zeros((n, 3, 3))
    Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1], Rz[:, 2, 2] = cyw, -syw, syw, cyw, 1.0
    feet = root[:, None, :3] + np.einsum("nij,nfj->nfi", Rz, r)
    tick = rng.integers(1, 4 * period, n)
    sched = ((tick[:, None] - 1) % period + np.asarray(offsets)[None]) % period < np.asarray(st)[None]
    nominal = Q.A1_FEET.copy()
    P = G.params(dt, height=0.30, touchdown_z=0.01)
    contact, xref, pos = horizon(tick, target, yaw, period, offsets, st, sched.astype(np.uint8), feet, command, nominal, P, H, S)
    A = rng.uniform(-1, 1, (n, 6, 6)) * 0.02
    M6 = A1_INERTIA[None] + np.einsum("nij,nkj->nik", A, A)
    return problem(contact, xref, pos, root, M6, w, float(S * P["dt"])), mu
