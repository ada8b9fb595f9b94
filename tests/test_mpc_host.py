"""Host-side checks of the horizon MPC (csrc/shf_mpc.hip: shf_mpc_horizon, shf_foot_force_mpc, shf_foot_force_efforts), no GPU:
the entries are declared, bound and refuse what they cannot compute; tests/mpc_ref.py's pieces agree with each other (the
condensed P, q against the literal recurrences; the contact table against the planner's schedule tick by tick; a stand
against a scalar model of the vertical axis); and how far the default sweeps and the float32 format leave the twin from the
certified optimum, on seeded A1-like problems.

Measured here (python -m pytest -s tests/test_mpc_host.py prints them), the worst of N_PROB problems per gait, at the defaults
(horizon 10 x 0.03 s, alpha 1e-5, 100 sweeps from a cold start): WORST below.  The assertions are four times these.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi
from tests import gait_ref as G
from tests import mpc_ref as R
from tests import qp_ref as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROB, SEED = 24, 11
FZ_MIN = 5.0
# (gait, figure): step 0 of the float64 twin against `certified` -- the cost's gap over the cost, the force error over the
# largest force -- and the float32 twin against the float64 twin (forces; efforts through a seeded J)
WORST = {("stand", "cost"): 5.13e-4, ("stand", "force"): 1.19e-1, ("trot", "cost"): 5.01e-4, ("trot", "force"): 5.71e-2,
         ("walk", "cost"): 6.60e-4, ("walk", "force"): 1.14e-1}
HORIZON_NAMES = ["tick", "target", "yaw", "period_ticks", "offset_ticks", "stance_ticks", "stance", "foot_pos", "foot_env_stride",
                 "foot_stride", "command", "nominal", "params", "horizon", "ticks_per_step", "n", "num_feet", "contact_out", "xref_out",
                 "pos_out", "stream"]
MPC_NAMES = ["contact", "xref", "pos", "root_pose", "root_env_stride", "mass_matrix", "dyn_bias", "j_feet", "j_env_stride",
             "j_foot_stride", "mu_or_null", "mu_scalar", "weights12", "alpha", "fz_min", "fz_max", "iters", "step_dt", "bias_or_null",
             "effort_limit_or_null", "u_io_or_null", "warm_shift", "n", "horizon", "num_feet", "num_dof", "forces_out", "efforts_out",
             "stream"]
EFF_NAMES = ["forces", "stance", "j_feet", "j_env_stride", "j_foot_stride", "bias_or_null", "effort_limit_or_null", "n", "num_feet",
             "num_dof", "efforts_out", "stream"]


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


# ---------------------------------------------------------------------------------------------------------- plumbing --
def test_header_declares_the_entries():
    for name, names in (("shf_mpc_horizon", HORIZON_NAMES), ("shf_foot_force_mpc", MPC_NAMES), ("shf_foot_force_efforts", EFF_NAMES)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", _header())
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == len(names), name
        for a, nm in zip(args, names):
            assert re.search(r"\b" + nm + r"$", a), (a, nm)
    assert re.search(r"#define\s+SHF_MPC_MAX_HORIZON\s+10\b", _header()) and _abi.MPC_MAX_HORIZON == R.MAX_HORIZON == 10
    assert os.path.exists(os.path.join(ROOT, "shifu_amd", "csrc", "shf_mpc.hip"))


def test_binding_table_and_build_cover_the_entries(lib):
    from shifu_amd import _lib, build, glue
    for name, names in (("shf_mpc_horizon", HORIZON_NAMES), ("shf_foot_force_mpc", MPC_NAMES), ("shf_foot_force_efforts", EFF_NAMES)):
        assert name in _lib.EXPORTS and len(_lib._SIGS[name][0]) == len(names)
        assert getattr(lib, name).restype is ctypes.c_int32
    floats = [MPC_NAMES[i] for i, t in enumerate(_lib._SIGS["shf_foot_force_mpc"][0]) if t is ctypes.c_float]
    assert floats == ["mu_scalar", "alpha", "fz_min", "fz_max", "step_dt"]
    assert _lib._SIGS["shf_mpc_horizon"][0][HORIZON_NAMES.index("params")] is _abi.ShfGaitParams
    assert "shf_mpc.hip" in build.SOURCES and "shf_mpc.hip" in build.UNITY_SOURCES
    budgets = {b[0]: b for b in build.BUDGETS}
    for k in ("13k_mpc_horizon", "16k_foot_force_mpc", "20k_foot_force_efforts"):
        assert budgets["_ZN12_GLOBAL__N_1" + k][2] == 0, "no scratch"
    assert (glue.MPC_HORIZON, glue.MPC_ITERS, glue.MPC_ALPHA, glue.MPC_EVERY) == (R.HORIZON, R.ITERS, R.ALPHA, R.EVERY)
    assert tuple(glue.MPC_WEIGHTS) == tuple(R.WEIGHTS12)


def test_abi_version_is_still_22(lib):
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header())
    assert _abi.SHF_ABI_VERSION == 22 and lib.shf_abi_version() == 22


def test_library_refuses_what_it_cannot_compute(lib):
    """Every refusal is decided on the host, before any launch: the pointers below are never dereferenced."""
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    ia = (ctypes.c_int32 * 4)
    par = _abi.ShfGaitParams(*[G.params(0.005)[k] for k in G.PARAM_NAMES])

    def refuser(fn, names, good):
        def refused(text, **kw):
            a = dict(good, **kw)
            assert getattr(lib, fn)(*[a[k] for k in names]) != 0, kw
            msg = lib.shf_last_error()
            assert fn.encode() in msg and text in msg, (kw, msg)
        return refused

    good = dict(zip(HORIZON_NAMES, [out, out, out, 60, ia(0, 30, 30, 0), ia(30, 30, 30, 30), out, out, 0, 0, out, out, par, 10, 6, 1, 4,
                                    out, out, out, None]))
    refused = refuser("shf_mpc_horizon", HORIZON_NAMES, good)
    for name in ("tick", "target", "yaw", "stance", "foot_pos", "command", "nominal", "contact_out", "xref_out", "pos_out"):
        refused(b"null tensor", **{name: None})
    refused(b"horizon outside", horizon=0)
    refused(b"horizon outside", horizon=_abi.MPC_MAX_HORIZON + 1)
    refused(b"ticks_per_step", ticks_per_step=0)
    refused(b"1 to 4 feet", num_feet=5)
    refused(b"1 to 4 feet", num_feet=0)
    refused(b"period_ticks", period_ticks=0)
    refused(b"stance_ticks", stance_ticks=ia(30, 61, 30, 30))
    refused(b"offset_ticks", offset_ticks=ia(0, 60, 30, 0))
    assert lib.shf_mpc_horizon(*[dict(good, n=0)[k] for k in HORIZON_NAMES]) == 0

    good = dict(zip(MPC_NAMES, [out, out, out, out, 0, out, out, out, 0, 0, None, 0.5, out, 1e-5, 5.0, 100.0, 10, 0.03, None, None, None, 0,
                                1, 10, 4, 12, out, out, None]))
    refused = refuser("shf_foot_force_mpc", MPC_NAMES, good)
    for name in ("contact", "xref", "pos", "root_pose", "mass_matrix", "dyn_bias", "j_feet", "weights12", "forces_out", "efforts_out"):
        refused(b"null tensor", **{name: None})
    refused(b"horizon outside", horizon=0)
    refused(b"horizon outside", horizon=11)
    refused(b"1 to 4 feet", num_feet=5)
    refused(b"1 to 4 feet", num_feet=0)
    refused(b"too many dofs", num_dof=_abi.MAX_DOFS + 1)
    refused(b"at least one dof", num_dof=0)
    refused(b"alpha", alpha=0.0)
    refused(b"alpha", alpha=-1.0)
    refused(b"fz_min", fz_min=10.0, fz_max=5.0)
    refused(b"mu", mu_scalar=-0.1)
    refused(b"iters", iters=0)
    refused(b"step_dt", step_dt=0.0)
    refused(b"warm_shift", warm_shift=-1)
    assert lib.shf_foot_force_mpc(*[dict(good, n=0)[k] for k in MPC_NAMES]) == 0

    good = dict(zip(EFF_NAMES, [out, out, out, 0, 0, None, None, 1, 4, 12, out, None]))
    refused = refuser("shf_foot_force_efforts", EFF_NAMES, good)
    for name in ("forces", "stance", "j_feet", "efforts_out"):
        refused(b"null tensor", **{name: None})
    refused(b"1 to 4 feet", num_feet=5)
    refused(b"too many dofs", num_dof=_abi.MAX_DOFS + 1)
    refused(b"at least one dof", num_dof=0)
    assert lib.shf_foot_force_efforts(*[dict(good, n=0)[k] for k in EFF_NAMES]) == 0


# ------------------------------------------------------------------------------------------------ the references agree --
@pytest.mark.parametrize("gait", ["stand", "trot", "walk", "bound"])
def test_condense_against_rollout(gait):
    """1/2 u^T P u + q^T u of `condense` is the cost of the literal recurrences (up to its value at u = 0), on random u."""
    prob, _ = R.a1_problems(6, 3, gait)
    n, H, F = prob["contact"].shape
    C = R.condense(prob, R.WEIGHTS12, R.ALPHA)
    u = np.random.default_rng(0).uniform(-60, 60, (n, H, F, 3))
    uc = (u * prob["contact"][..., None]).reshape(n, -1)
    c1 = R.cost(prob, u, R.WEIGHTS12, R.ALPHA) - R.cost(prob, 0 * u, R.WEIGHTS12, R.ALPHA)
    c2 = 0.5 * np.einsum("ni,nij,nj->n", uc, C["P"], uc) + np.einsum("ni,ni->n", C["q"], uc)
    assert np.abs(c1 - c2).max() <= 1e-10 * np.abs(c1).max()
    a, B = R.affine(prob)
    Lw = np.tile(np.asarray(R.WEIGHTS12), H)
    Pb = np.einsum("nri,r,nrj->nij", B, Lw, B)
    on = C["cf"] != 0
    Pm = C["P"] - R.ALPHA * np.eye(3 * F * H)
    assert np.abs((Pm - Pb) * on[:, :, None] * on[:, None, :]).max() <= 1e-10 * np.abs(Pb).max()
    assert (Pm[~on] == 0).all(), "the columns of a foot in the air are zero: it decouples"


@pytest.mark.parametrize("S", [1, 6])
@pytest.mark.parametrize("gait", ["trot", "walk", "bound"])
def test_contact_table_is_the_schedule_tick_by_tick(gait, S):
    """From every starting tick of a period: row 0 is the stance given, row k >= 1 what gait_ref.plan schedules k S ticks later
    (the planner has already advanced the stored tick when `horizon` reads it)."""
    period, offsets, st = R.GAITS[gait]
    H = 10
    P = G.params(0.005)
    rng = np.random.default_rng(1)
    state = G.new_state(1, 4)
    inp = G.seeded_inputs(1, rng)
    scheduled, ticks = [], []
    for t in range(period + H * S + 1):
        out = G.plan(state, inp["root"], inp["feet"], None, inp["command"] * 0, G.NOMINAL, np.ones(1, np.uint8) if t == 0 else None,
                     period, offsets, st, P)
        scheduled.append(out["scheduled"][0].copy())
        ticks.append(int(state["tick"][0]))
    for t0 in range(period):
        given = (np.arange(4) % 2 == t0 % 2).astype(np.uint8)[None]          # row 0 is taken as given, whatever the schedule says
        c, _, pos = R.horizon(np.array([ticks[t0]]), state["target"], state["yaw"], period, offsets, st, given, inp["feet"],
                              inp["command"], G.NOMINAL, P, H, S)
        assert np.array_equal(c[0, 0], given[0])
        for k in range(1, H):
            assert np.array_equal(c[0, k], scheduled[t0 + k * S]), (t0, k)
        assert (pos[c == 0] == 0).all()
        held = (np.cumprod(c[0], 0) != 0)                                    # in contact without a break since step 0
        assert np.array_equal(pos[0][held], np.broadcast_to(inp["feet"][0], (H, 4, 3))[held])


def test_symmetric_stand_carries_the_weight_less_what_alpha_buys():
    """x_0 = xref, h6 the weight, feet at (+-a, +-b, -c): by symmetry the optimum is four equal vertical forces per step, mg / 4 -
    d_k, and d solves the vertical axis alone -- v_{k+1} = v_k - delta 4 d_k / m, p_{k+1} = p_k + delta v_k, minimise
    1/2 sum (L_z p_k^2 + L_vz v_k^2) + 1/2 alpha 4 sum (mg / 4 - d_k)^2 -- an H x H system formed here from those two lines.  The
    forces so sum to the weight less 4 d_0: that much the alpha term buys, no more (d_0 is negative at the defaults: the last
    steps of a horizon cost little to starve -- the last one loses half its force -- and the first ones push 1.2 % harder to make
    up for them; only step 0 is ever applied)."""
    m, g, H, d = 12.45, 9.81, R.HORIZON, 0.03
    root = np.zeros((1, 13))
    root[0, 2], root[0, 6] = 0.30, 1.0
    xref = np.zeros((1, H + 1, 12))
    xref[:, :, 5] = 0.30
    feet = np.array([[0.18, 0.13, 0.0], [0.18, -0.13, 0.0], [-0.18, 0.13, 0.0], [-0.18, -0.13, 0.0]])
    pos = np.broadcast_to(feet, (1, H, 4, 3)).copy()
    M6 = np.diag([m, m, m, 0.11, 0.30, 0.33])[None]
    h6 = np.array([[0.0, 0.0, m * g, 0.0, 0.0, 0.0]])
    prob = R.problem(np.ones((1, H, 4), np.uint8), xref, pos, root, M6, h6, d)
    u = R.certified(prob, 0.6, R.WEIGHTS12, R.ALPHA, FZ_MIN, np.inf)[0]
    # the scalar model: p, v after each step are linear in the deficits dk
    Tv, Tp = np.zeros((H + 1, H)), np.zeros((H + 1, H))
    for k in range(H):
        Tp[k + 1] = Tp[k] + d * Tv[k]
        Tv[k + 1] = Tv[k]
        Tv[k + 1, k] -= d * 4.0 / m
    Lz, Lvz = R.WEIGHTS12[5], R.WEIGHTS12[11]
    A = Lz * Tp[1:].T @ Tp[1:] + Lvz * Tv[1:].T @ Tv[1:] + 4.0 * R.ALPHA * np.eye(H)
    dk = np.linalg.solve(A, 4.0 * R.ALPHA * (m * g / 4.0) * np.ones(H))
    assert np.abs(u[..., :2]).max() <= 1e-7 * m * g
    assert np.abs(u[..., 2] - (m * g / 4.0 - dk)[:, None]).max() <= 1e-7 * m * g
    assert 4.0 * abs(dk[0]) < 0.02 * m * g and dk[0] < 0.0 < dk[-1]
    tw = R.twin(prob, 0.6, R.WEIGHTS12, R.ALPHA, FZ_MIN, np.inf, 2000)[0]
    assert np.abs(tw - u).max() <= 1e-6 * m * g


# ------------------------------------------------------------------------------------- convergence and number format --
_PROBLEMS = {}


def _problems(gait):
    if gait not in _PROBLEMS:
        prob, mu = R.a1_problems(N_PROB, SEED, gait)
        ex = R.certified(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, np.inf)          # raises unless every problem certifies
        u64 = R.twin(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, np.inf, R.ITERS)
        u32 = R.twin(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, np.inf, R.ITERS, np.float32)
        _PROBLEMS[gait] = (prob, mu, ex, u64, u32)
    return _PROBLEMS[gait]


@pytest.mark.parametrize("gait", ["stand", "trot", "walk"])
def test_default_sweeps_against_the_certified_optimum(gait):
    prob, mu, ex, u64, _ = _problems(gait)
    n = N_PROB
    assert len({tuple(r) for r in prob["contact"][:, 0]}) >= (1 if gait == "stand" else 2)
    c_ex, c_tw = R.cost(prob, ex, R.WEIGHTS12, R.ALPHA), R.cost(prob, u64, R.WEIGHTS12, R.ALPHA)
    gap = (c_tw - c_ex) / np.abs(c_ex)
    ef = np.abs(u64[:, 0] - ex[:, 0]).reshape(n, -1).max(1) / np.abs(ex[:, 0]).reshape(n, -1).max(1)
    print(f"[mpc host] {gait} ({R.STANCE_OF[gait]} feet down at step 0), {R.ITERS} sweeps against the certified optimum: cost gap "
          f"{gap.max():.3e} of the cost, step 0's forces {ef.max():.3e} of the largest force")
    assert gap.min() >= -1e-9, "nothing feasible costs less than the certified optimum"
    assert gap.max() <= 4.0 * WORST[(gait, "cost")] and ef.max() <= 4.0 * WORST[(gait, "force")]


def test_float32_twin_against_float64_twin():
    """What the number format alone does, at the default sweeps; mpc_ref.F32_DIST records the worst and sets the GPU bound."""
    rng = np.random.default_rng(5)
    worst = {"forces": 0.0, "efforts": 0.0}
    for gait in ("stand", "trot", "walk"):
        prob, mu, _, u64, u32 = _problems(gait)
        n = N_PROB
        J = np.zeros((n, 4, 6, 18))
        J[:, :, :3, 6:] = rng.uniform(-0.3, 0.3, (n, 4, 3, 12))               # lever arms of the A1's size
        t64, _ = Q.efforts(J, u64[:, 0])
        t32, _ = Q.efforts(J, u32[:, 0].astype(np.float64))
        ef = (np.abs(u32[:, 0] - u64[:, 0]).reshape(n, -1).max(1) / max(np.abs(u64[:, 0]).max(), 1.0)).max()
        et = (np.abs(t32 - t64).max(1) / np.abs(t64).max()).max()
        print(f"[mpc host] {gait}: float32 twin against float64 twin: forces {ef:.3e} of the largest force, efforts {et:.3e} of the largest")
        near, scale = Q.face_distance(u64[:, 0], prob["contact"][:, 0], mu, FZ_MIN, np.inf)
        worst["forces"], worst["efforts"] = max(worst["forces"], ef), max(worst["efforts"], et)
    for k in worst:
        assert worst[k] <= R.F32_DIST[k] <= 1.25 * worst[k], (k, worst[k], R.F32_DIST[k])


def test_horizon_in_float32():
    """float32 against float64 `horizon`: the contact table is the same (integers only); the figures are printed."""
    rng = np.random.default_rng(2)
    n = 64
    inp = G.seeded_inputs(n, rng)
    period, offsets, st = R.GAITS["trot"]
    yaw = rng.uniform(-np.pi, np.pi, n).astype(np.float32).astype(np.float64)
    target = np.zeros((n, 13))
    target[:, :2], target[:, 2] = inp["root"][:, :2], 0.30
    target[:, 7:9], target[:, 12] = rng.uniform(-0.5, 0.5, (n, 2)), inp["command"][:, 2]
    target = target.astype(np.float32).astype(np.float64)
    tick = rng.integers(1, 4 * period, n)
    stance = (inp["contact"] > 1.0).astype(np.uint8)
    a = R.horizon(tick, target, yaw, period, offsets, st, stance, inp["feet"], inp["command"], G.NOMINAL, G.params(0.005), 10, 6)
    b = R.horizon(tick, target, yaw, period, offsets, st, stance, inp["feet"], inp["command"], G.NOMINAL, G.params(0.005), 10, 6, np.float32)
    assert np.array_equal(a[0], b[0])
    dx, dp = np.abs(a[1] - b[1]).max(), np.abs(a[2] - b[2]).max()
    print(f"[mpc host] horizon float32 against float64: xref {dx:.3e}, pos {dp:.3e}")
    assert dx <= 1e-5 and dp <= 1e-5


# ------------------------------------------------------------------------------------------------- the torch fallbacks --
def test_torch_fallbacks_equal_the_twins():
    torch = pytest.importorskip("torch")
    from shifu_amd.utils import torch_utils as TU
    T = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    rng = np.random.default_rng(4)
    for gait in ("trot", "bound"):
        prob, mu = R.a1_problems(5, 3, gait)
        n, H, F = prob["contact"].shape
        u = R.twin(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, 150.0, 60)
        M, h = np.zeros((n, 18, 18)), np.zeros((n, 18))
        M[:, :6, :6], h[:, :6] = prob["M6"], prob["h6"]
        h[:, 6:] = rng.normal(size=(n, 12))
        J = rng.normal(size=(n, 4, 6, 18))
        lim = np.full(12, 33.5)
        args = (torch.from_numpy(prob["contact"]), T(prob["xref"]), T(prob["pos"]), T(prob["root"]), T(M), T(h), T(J), T(mu), T(R.WEIGHTS12),
                R.ALPHA, FZ_MIN, 150.0)
        f, tau = TU.foot_force_mpc(*args, 60, prob["delta"], T(h), T(lim))
        scale = np.abs(u).max()
        assert np.abs(f.numpy() - u[:, 0]).max() <= 1e-9 * scale
        assert np.abs(tau.numpy() - Q.efforts(J, u[:, 0], h, lim)[1]).max() <= 1e-9 * scale
        u0 = T(u.copy())
        f2, _ = TU.foot_force_mpc(*args, 20, prob["delta"], None, None, u0, 1)
        u2 = R.twin(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, 150.0, 20, u0=u, warm_shift=1)
        assert np.abs(f2.numpy() - u2[:, 0]).max() <= 1e-9 * scale and np.abs(u0.numpy() - u2).max() <= 1e-9 * scale
    # the tables
    n = 16
    inp = G.seeded_inputs(n, rng)
    period, offsets, st = R.GAITS["walk"]

    class State:
        pass
    s = State()
    target = np.zeros((n, 13))
    target[:, :2], target[:, 2], target[:, 7:9], target[:, 12] = inp["root"][:, :2], 0.3, rng.uniform(-0.5, 0.5, (n, 2)), inp["command"][:, 2]
    yaw = rng.uniform(-4, 4, n)
    tick = rng.integers(1, 300, n)
    s.target, s.yaw, s.tick = T(target), T(yaw), torch.from_numpy(tick.astype(np.int32))
    stance = (inp["contact"] > 1.0).astype(np.uint8)
    P = G.params(0.005, as_float32=False)
    a = R.horizon(tick, target, yaw, period, offsets, st, stance, inp["feet"], inp["command"], G.NOMINAL, P, 7, 6)
    b = TU.mpc_horizon(s, torch.from_numpy(stance), T(inp["feet"]), T(inp["command"]), T(G.NOMINAL), (period, offsets, st), P["dt"],
                       P["touchdown_z"], P["max_step"], 7, 6)
    assert np.array_equal(a[0], b[0].numpy())
    assert np.abs(a[1] - b[1].numpy()).max() <= 1e-12 and np.abs(a[2] - b[2].numpy()).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------- edges --
def test_flight_rows_and_a_one_step_horizon_stay_finite_and_feasible():
    for gait, H in (("bound", 10), ("bound", 1), ("trot", 1)):
        prob, mu = R.a1_problems(12, 7, gait, H=H)
        c = prob["contact"]
        if gait == "bound" and H == 10:
            assert (c.sum(2) == 0).any(), "rows with every foot in the air"
            prob["contact"][0] = 0                                              # and an env that never touches down
            prob["pos"][0] = 0.0
        for T in (np.float64, np.float32):
            u = R.twin(prob, mu, R.WEIGHTS12, R.ALPHA, FZ_MIN, 150.0, R.ITERS, T)
            assert np.isfinite(u).all() and u.dtype == T
            on = c != 0
            assert (u[~on] == 0).all()
            fz = u[..., 2]
            assert (fz[on] >= T(FZ_MIN)).all() and (fz[on] <= T(150.0)).all()
            bnd = np.asarray(mu, T)[:, None, None] * fz
            assert (np.abs(u[..., 0]) <= bnd)[on].all() and (np.abs(u[..., 1]) <= bnd)[on].all()
