"""Host-side checks of the balance controller's foot-force QP (csrc/shf_qp.hip: shf_foot_force_qp), no GPU: the entry is
declared, bound and additive (SHF_ABI_VERSION stays 22) and refuses what it cannot compute; the exact float64 solver of
tests/qp_ref.py is what it claims to be; the kernel's algorithm (its NumPy twin) converges to that optimum on A1-like problems;
the torch fallback equals the twin; closed-form cases.

Convergence of the twin at the default 100 sweeps, rho = sqrt((alpha + beta) m), sigma = 1e-6 m, relaxation 1.6, measured on
200 seeded problems per stance set (all four feet, a diagonal pair, three feet), the worst over the three sets (WORST below):
    alpha = 1e-2:  cost gap / (w^T S w / 2) 6.44e-5,  |G f - G f*| / max|w| 4.21e-4,  |f - f*| / max|f*| 1.63e-3
    alpha = 1e-3:  cost gap 3.06e-4,  wrench error 5.17e-3  (the forces themselves are not asserted: H is rank 6 plus alpha I,
                   and along its flat directions 100 sweeps leave 5.4e-2 of the largest force)
(at 200 sweeps and alpha = 1e-2: 4.2e-7, 3.8e-6, 6.8e-5).  Each is asserted at four times the measured value, the wrench error
never above 1e-2.  float32 against float64 of the same sweeps on the GPU test's own seeded launch: 1.19e-5 of the largest force.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import helpers as H
from tests import qp_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S6 = np.array([1.0, 1.0, 1.0, 10.0, 10.0, 10.0])
WORST = {("cost", 1e-2): 6.44e-5, ("wrench", 1e-2): 4.21e-4, ("force", 1e-2): 1.63e-3,
         ("cost", 1e-3): 3.06e-4, ("wrench", 1e-3): 5.17e-3, "f32": 1.190e-5}
TOL = {k: 4.0 * v for k, v in WORST.items()}
TOL[("wrench", 1e-2)], TOL[("wrench", 1e-3)] = min(TOL[("wrench", 1e-2)], 1e-2), min(TOL[("wrench", 1e-3)], 1e-2)
NAMES = ["j_feet", "j_env_stride", "j_foot_stride", "root_pose", "root_env_stride", "foot_pos", "foot_env_stride", "foot_stride",
         "wrench_or_null", "mass_matrix_or_null", "dyn_bias_or_null", "base_target_or_null", "gains12_or_null", "stance",
         "mu_or_null", "mu_scalar", "weights6", "alpha", "beta", "f_prev_or_null", "fz_min", "fz_max", "iters", "bias_or_null",
         "effort_limit_or_null", "n", "num_feet", "num_dof", "forces_out", "efforts_out", "stream"]


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


# ---------------------------------------------------------------------------------------------------------- plumbing --
def test_header_declares_the_entry():
    m = re.search(r"\bint\s+shf_foot_force_qp\s*\(([^;]*)\)\s*;", _header())
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == len(NAMES) == 31
    for a, name in zip(args, NAMES):
        assert re.search(r"\b" + name + r"$", a), (a, name)
    assert os.path.exists(os.path.join(ROOT, "shifu_amd", "csrc", "shf_qp.hip"))


def test_binding_table_covers_the_entry(lib):
    from shifu_amd import _lib, glue
    assert "shf_foot_force_qp" in _lib.EXPORTS and len(_lib._SIGS["shf_foot_force_qp"][0]) == 31
    assert lib.shf_foot_force_qp.restype is ctypes.c_int32
    floats = [i for i, t in enumerate(_lib._SIGS["shf_foot_force_qp"][0]) if t is ctypes.c_float]
    assert [NAMES[i] for i in floats] == ["mu_scalar", "alpha", "beta", "fz_min", "fz_max"]
    assert callable(glue.foot_force_qp) and glue.QP_ITERS == Q.ITERS


def test_abi_version_is_still_22(lib):
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header())
    assert _abi.SHF_ABI_VERSION == 22 and lib.shf_abi_version() == 22


def test_library_refuses_what_it_cannot_compute(lib):
    """Every refusal is decided on the host, before any launch: the pointers below are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(zip(NAMES, [out, 0, 0, out, 0, out, 0, 0, out, None, None, None, None, out, None, 0.5, out, 1e-2, 0.0, None, 5.0,
                            100.0, 10, None, None, 1, 4, 12, out, out, None]))

    def refused(text, **kw):
        a = dict(good, **kw)
        assert lib.shf_foot_force_qp(*[a[k] for k in NAMES]) != 0, kw
        msg = lib.shf_last_error()
        assert b"shf_foot_force_qp" in msg and text in msg, (kw, msg)

    for name in ("j_feet", "root_pose", "foot_pos", "stance", "weights6", "forces_out", "efforts_out"):
        refused(b"null tensor", **{name: None})
    refused(b"null tensor", wrench_or_null=None)                                   # no wrench and nothing to form it from
    for name in ("mass_matrix_or_null", "dyn_bias_or_null", "base_target_or_null", "gains12_or_null"):
        full = dict(wrench_or_null=None, mass_matrix_or_null=out, dyn_bias_or_null=out, base_target_or_null=out, gains12_or_null=out)
        refused(b"null tensor", **dict(full, **{name: None}))
    refused(b"1 to 4 feet", num_feet=5)
    refused(b"1 to 4 feet", num_feet=0)
    refused(b"too many dofs", num_dof=_abi.MAX_DOFS + 1)
    refused(b"at least one dof", num_dof=0)
    refused(b"alpha", alpha=0.0)
    refused(b"alpha", alpha=-1.0)
    refused(b"beta", beta=-0.1)
    refused(b"fz_min", fz_min=10.0, fz_max=5.0)
    refused(b"mu", mu_scalar=-0.1)
    refused(b"iters", iters=0)
    assert lib.shf_foot_force_qp(*[dict(good, n=0)[k] for k in NAMES]) == 0          # nothing to do: no launch


# ------------------------------------------------------------------------------------------------- the exact solver --
def test_exact_solver_is_verified_and_beats_every_feasible_point():
    """`exact` against what it shares nothing with: an unconstrained problem's closed form, the same answer from a useless
    starting guess, and random feasible points, none of which may cost less."""
    rng = np.random.default_rng(3)
    r, w, mu, st = Q.a1_problems(12, 7, (1, 0, 0, 1))
    for e in range(12):
        f = Q.exact(r[e], w[e], S6, 1e-2, 0.0, None, st[e], mu[e], 5.0, np.inf)
        g = Q.exact(r[e], w[e], S6, 1e-2, 0.0, None, st[e], mu[e], 5.0, np.inf, guess=np.full((4, 3), 1e9))   # a useless guess
        assert np.abs(f - g).max() <= 1e-9 * np.abs(f).max()
        assert (f[[1, 2]] == 0).all() and (f[[0, 3], 2] >= 5.0 - 1e-9).all()
        assert (np.abs(f[:, :2]) <= mu[e] * f[:, 2:3] + 1e-9).all()
        c0 = Q.cost(r[e], w[e], S6, 1e-2, 0.0, None, f)
        for _ in range(200):
            p = np.zeros((4, 3))
            p[[0, 3], 2] = rng.uniform(5.0, 150.0, 2)
            p[[0, 3], :2] = rng.uniform(-1, 1, (2, 2)) * mu[e] * p[[0, 3], 2:3]
            assert Q.cost(r[e], w[e], S6, 1e-2, 0.0, None, p) >= c0 * (1 - 1e-12)
    # far inside every constraint the optimum is the regularised least-squares solution
    rr, ww = Q.A1_FEET, np.array([1.0, -2.0, Q.A1_WEIGHT, 0.3, -0.2, 0.1])
    f = Q.exact(rr, ww, S6, 1e-2, 0.0, None, (1, 1, 1, 1), 1.0, 5.0, np.inf)
    G = Q.grasp(rr)
    x = np.linalg.solve(G.T @ (S6[:, None] * G) + 1e-2 * np.eye(12), G.T @ (S6 * ww))
    assert np.abs(f.reshape(-1) - x).max() <= 1e-9 * np.abs(x).max()
    # the beta term pulls towards f_prev
    fp = np.tile([3.0, -2.0, 40.0], (4, 1))
    f2 = Q.exact(rr, ww, S6, 1e-2, 10.0, fp, (1, 1, 1, 1), 1.0, 5.0, np.inf)
    assert np.abs(f2 - fp).max() < np.abs(f - fp).max()


# -------------------------------------------------------------------------------------------------------- convergence --
_OPT = {}


def _figures(alpha, name):
    key = (alpha, name)
    if key not in _OPT:
        r, w, mu, st = Q.a1_problems(200, 101, Q.STANCES[name])
        f = Q.twin(r, w, S6, alpha, 0.0, None, st, mu, 5.0, np.inf)
        cg = wr = fe = 0.0
        for e in range(200):
            fs = Q.exact(r[e], w[e], S6, alpha, 0.0, None, st[e], mu[e], 5.0, np.inf, guess=f[e])
            c, cs = Q.cost(r[e], w[e], S6, alpha, 0.0, None, f[e]), Q.cost(r[e], w[e], S6, alpha, 0.0, None, fs)
            assert c >= cs * (1 - 1e-9), "the twin's point is feasible, so it cannot cost less than the optimum"
            cg = max(cg, (c - cs) / (0.5 * w[e] @ (S6 * w[e])))
            wr = max(wr, np.abs(Q.grasp(r[e]) @ (f[e] - fs).reshape(-1)).max() / np.abs(w[e]).max())
            fe = max(fe, np.abs(f[e] - fs).max() / np.abs(fs).max())
        _OPT[key] = (cg, wr, fe)
    return _OPT[key]


@pytest.mark.parametrize("name", list(Q.STANCES))
def test_twin_converges_to_the_exact_optimum(name):
    cg, wr, fe = _figures(1e-2, name)
    print(f"[qp] alpha 1e-2 {name}: cost gap {cg:.3e}  wrench error {wr:.3e}  force error {fe:.3e}")
    assert cg <= TOL[("cost", 1e-2)] and wr <= TOL[("wrench", 1e-2)] and fe <= TOL[("force", 1e-2)]


@pytest.mark.parametrize("name", list(Q.STANCES))
def test_twin_at_the_smaller_alpha_matches_cost_and_wrench(name):
    cg, wr, fe = _figures(1e-3, name)
    print(f"[qp] alpha 1e-3 {name}: cost gap {cg:.3e}  wrench error {wr:.3e}  (force error {fe:.3e}, not asserted)")
    assert cg <= TOL[("cost", 1e-3)] and wr <= TOL[("wrench", 1e-3)]


def test_float32_twin_leaves_out_no_env_of_the_gpu_launch():
    """The seeded launch of the GPU test, its wrench from the float64 dynamics: the twin in float32 against float64 stays
    within the GPU test's cap of 1e-4 in every env, so that test's allowance for clips that flip is not needed for the number
    format alone."""
    m = H.a1_model().blob
    X = B.qp_states(m)
    J, M, h = B.dynamics64(m, X["q"], X["qd"], X["root"])
    w = Q.wrench(M, h, X["root"], X["target"], B.gains12())
    r = B.feet_positions(m, X["q"], X["root"]) - X["root"][:, None, :3].astype(np.float64)
    worst = 0.0
    for fp, beta in ((None, 0.0), (X["f_prev"], 0.05)):
        a = Q.twin(r, w, S6, 1e-2, beta, fp, X["stance"], X["mu"], 5.0, 80.0)
        b = Q.twin(r.astype(np.float32), w.astype(np.float32), S6, 1e-2, beta, fp, X["stance"], X["mu"], 5.0, 80.0, dtype=np.float32)
        assert b.dtype == np.float32
        err = np.abs(a - b).reshape(len(a), -1).max(1) / np.abs(a).max()
        worst = max(worst, float(err.max()))
        assert ((a == 0) == (b == 0)).all()
    print(f"[qp] float32 twin against float64, {len(r)} envs: worst |f32 - f64| / max|f64| = {worst:.3e}")
    assert worst <= min(TOL["f32"], 1e-4)


# ----------------------------------------------------------------------------------------------------------- fallback --
def test_torch_fallback_equals_the_twin_in_float64():
    torch = pytest.importorskip("torch")
    from shifu_amd.utils.torch_utils import balance_wrench, foot_force_qp
    rng = np.random.default_rng(5)
    n = 40
    r, w, mu, st = Q.a1_problems(n, 9, (1, 1, 1, 1))
    st = (rng.uniform(size=(n, 4)) < 0.7).astype(np.uint8)
    st[0] = 0
    J, bias = rng.normal(size=(n, 4, 6, 18)), rng.normal(size=(n, 18))
    rp = rng.normal(size=(n, 3))
    fprev = rng.normal(size=(n, 4, 3)) * 10
    T = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
    for fp, beta, fzmax, b in ((None, 0.0, np.inf, None), (fprev, 0.05, 60.0, bias)):
        f = Q.twin(r, w, S6, 1e-2, beta, fp, st, mu, 5.0, fzmax)
        free, _ = Q.efforts(J, f, b)
        lim = np.abs(free).mean(0)
        lim[1], lim[4] = 0.0, -1.0
        _, tau = Q.efforts(J, f, b, lim)
        g, t = foot_force_qp(T(J), T(rp), T(r + rp[:, None]), T(w), torch.from_numpy(st), T(mu), T(S6), 1e-2, beta, T(fp), 5.0, fzmax,
                             Q.ITERS, T(b), T(lim))
        assert np.abs(g.numpy() - f).max() <= 1e-9 * np.abs(f).max()
        assert np.abs(t.numpy() - tau).max() <= 1e-9 * np.abs(free).max()
        assert (g.numpy()[st == 0] == 0).all()
    # the wanted wrench
    M = rng.normal(size=(n, 18, 18))
    root, tg = rng.normal(size=(n, 13)), rng.normal(size=(n, 13))
    for a in (root, tg):
        a[:, 3:7] /= np.linalg.norm(a[:, 3:7], axis=1, keepdims=True)
    gains = rng.uniform(1, 100, 12)
    want = Q.wrench(M, bias, root, tg, gains)
    got = balance_wrench(T(M), T(bias), T(root), T(tg), T(gains)).numpy()
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# -------------------------------------------------------------------------------------------------------- closed form --
def test_symmetric_stance_carries_a_quarter_of_the_weight_per_foot():
    mg = Q.A1_WEIGHT
    w = np.array([[0.0, 0.0, mg, 0.0, 0.0, 0.0]])
    f = Q.twin(Q.A1_FEET[None], w, S6, 1e-2, 0.0, None, np.ones((1, 4), np.uint8), 0.6, 5.0, np.inf)[0]
    # the optimum itself: 1/2 (4 f - mg)^2 + 1/2 alpha 4 f^2 is least at f = mg / (4 + alpha)
    assert np.abs(f[:, 2] - mg / 4.01).max() <= TOL[("force", 1e-2)] * mg / 4
    assert np.abs(f[:, 2] - mg / 4).max() <= (TOL[("force", 1e-2)] + 1e-2 / 4) * mg / 4
    assert np.abs(f[:, :2]).max() <= TOL[("force", 1e-2)] * mg / 4


def test_a_swing_foot_gets_exact_zeros():
    r, w, mu, st = Q.a1_problems(30, 13, (1, 0, 1, 1))
    for dt in (np.float64, np.float32):
        f = Q.twin(r, w, S6, 1e-2, 0.0, None, st, mu, 5.0, np.inf, dtype=dt)
        assert (f[:, 1] == 0).all() and (f[:, [0, 2, 3], 2] >= 5.0).all()


def test_a_horizontal_demand_beyond_friction_saturates_the_cones_exactly():
    mg, mu = Q.A1_WEIGHT, 0.5
    w = np.array([[2.0 * mu * mg, 0.0, mg, 0.0, 0.0, 0.0]])
    for st in ((1, 1, 1, 1), (1, 0, 0, 1)):
        f = Q.twin(Q.A1_FEET[None], w, S6, 1e-2, 0.0, None, np.array([st], np.uint8), mu, 5.0, np.inf)[0]
        on = np.array(st, bool)
        assert (f[on, 2] >= 5.0).all() and (f[on, 0] == mu * f[on, 2]).all() and (f[~on] == 0).all()
        assert (np.abs(f[on, 1]) <= mu * f[on, 2]).all()
