"""The friction-cone sweep the foot-force QP and the horizon MPC share (csrc/shf_cone.h), NumPy only, for tests/qp_ref.twin and
tests/mpc_ref.twin.  Every function is elementwise on arrays of one shape (or scalars that broadcast), one line of the header
per operation, nothing fused: the operands may sit in lists per foot and row (qp_ref) or in stacked axes (mpc_ref), the bits
are the same."""
import numpy as np

SIGMA_C, RELAX = 1e-6, 1.6                             # the kernels' constants (cone::SIGMA, cone::RELAX)


def rows(mu, tx, ty, tz):
    """A_f t of a foot's force t: its five rows."""
    mz = mu * tz
    return [tz, mz - tx, mz + tx, mz - ty, mz + ty]


def at(mu, v):
    """A_f^T v, v[m] the five rows' values: the x, y and z components."""
    return [v[2] - v[1], v[4] - v[3], v[0] + mu * (((v[1] + v[2]) + v[3]) + v[4])]


def relax(xt, x, T):
    return T(RELAX) * xt + (T(1) - T(RELAX)) * x


def project(zt, z, y, rho, irho, lo, hi, T):
    """One sweep's (z', y') of rows with bounds [lo, hi] from zt = A xt."""
    zr = relax(zt, z, T)
    zn = np.minimum(np.maximum(zr + y * irho, lo), hi)
    return zn, y + rho * (zr - zn)


def feasible(on, mu, x0, x1, x2, fz_min, fz_max, T):
    """The exactly feasible force (x, y, z components) of a foot whose sweeps ended at (x0, x1, x2); zero where it does not stand."""
    fz = np.minimum(np.maximum(x2, T(fz_min)), T(fz_max))
    bnd = mu * fz
    return [np.where(on, np.minimum(np.maximum(x0, -bnd), bnd), T(0)), np.where(on, np.minimum(np.maximum(x1, -bnd), bnd), T(0)),
            np.where(on, fz, T(0))]
