"""The horizon MPC on the GPU (csrc/shf_mpc.hip: shf_mpc_horizon, shf_foot_force_mpc, shf_foot_force_efforts).

The references are tests/mpc_ref.py's float64 `horizon` and `twin` (the kernels' texts, operation by operation) on the GPU's own
J, M, h and tables.  The bounds come from the number format alone, measured on the CPU: for the tables, four times the distance
between the float32 and the float64 `horizon` on the same inputs (formed here, per case); for forces and efforts, four times the
float32 twin's distance from the float64 twin on the seeded problems of tests/test_mpc_host.py (mpc_ref.F32_DIST).  An env may
exceed the bound only if a clip flips between float32 and float64; the number of such envs is printed and must be 0.

A bare A1 sim with the 257 seeded states of tests/balance_cpu.qp_states (tilted, moving, a touching pattern and a friction per
env, some envs standing on nothing); gait phase, command and heading differ from env to env.
"""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import gait_ref as G
from tests import helpers as Hh
from tests import mpc_ref as R
from tests import qp_ref as Q

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FEET = B.FEET
TOL = {k: 4.0 * v for k, v in R.F32_DIST.items()}
DT = 0.005
# (n, H, S, gait): every n, H and S of the issue; bound's schedule has rows with nothing standing
CASES = [(1, 1, 1, "trot"), (2, 3, 6, "walk"), (65, 10, 1, "trot"), (257, 10, 6, "trot"), (257, 3, 1, "bound")]
FZ_MIN, FZ_MAX = 5.0, 150.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


_SET = {}


def _setup():
    """The seeded states on a bare A1 sim with its tensors refreshed, a GaitState as the planner leaves it (ticks spread over
    four periods, targets near the bases, headings off by whole turns on some envs), and everything read back for the twins:
    built once, shared, never modified."""
    if not _SET:
        import copy
        from shifu_amd.backend import Sim
        from shifu_amd.units.gait import GaitState
        m = Hh.a1_model().blob
        X = B.qp_states(m)
        n = B.QP_N
        sim = Sim(Hh.sim_params(dt=DT, gravity=B.GRAVITY), "cuda:0")
        sim.set_plane(1.0)
        sim.set_articulation(copy.deepcopy(m))
        sim.finalize(n, 0)
        dof = np.stack([X["q"], X["qd"]], -1).reshape(n * m.nd, 2).astype(np.float32)
        for tid, a in ((_abi.T_SIM_DOF, dof), (_abi.T_DOF_STATE, dof), (_abi.T_SIM_ROOT, X["root"]), (_abi.T_ROOT_STATE, X["root"])):
            sim.tensors[tid].copy_(torch.from_numpy(np.array(a, np.float32)))
        sim.refresh(_abi.REFRESH_ALL)
        D = m.nd + 6
        dev = sim.device
        M, h = torch.zeros(n, D, D, device=dev), torch.zeros(n, D, device=dev)
        jac = sim.tensors[_abi.T_JACOBIAN]
        sim.floating_dynamics(jac, M, h)
        torch.cuda.synchronize()
        body = sim.tensors[_abi.T_BODY_STATE].view(n, m.nb, 13)
        rng = np.random.default_rng(97)
        root = X["root"].astype(np.float64)
        heading = np.arctan2(2.0 * (root[:, 3] * root[:, 4] + root[:, 6] * root[:, 5]), 1.0 - 2.0 * (root[:, 4] ** 2 + root[:, 5] ** 2))
        yaw = heading + rng.uniform(-0.2, 0.2, n) + 2.0 * np.pi * rng.integers(-2, 3, n)
        command = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.3, 0.3, n), rng.uniform(-1.0, 1.0, n)], 1).astype(np.float32)
        cy, sy = np.cos(yaw), np.sin(yaw)
        target = np.zeros((n, 13), np.float32)
        target[:, :2] = root[:, :2] + rng.uniform(-0.05, 0.05, (n, 2))
        target[:, 2] = 0.30
        target[:, 5], target[:, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
        target[:, 7], target[:, 8] = cy * command[:, 0] - sy * command[:, 1], sy * command[:, 0] + cy * command[:, 1]
        target[:, 12] = command[:, 2]
        st = GaitState(n, 4, dev)
        st.tick.copy_(torch.from_numpy(rng.integers(1, 481, n).astype(np.int32)))
        st.target.copy_(torch.from_numpy(target))
        st.yaw.copy_(torch.from_numpy(yaw.astype(np.float32)))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        nominal = B.swing_targets(m).astype(np.float32)
        _SET.update(sim=sim, m=m, n=n, jf=jac[:, FEET[0]::4], fp=body[:, FEET[0]::4, :3], rs=sim.tensors[_abi.T_ROOT_STATE].view(n, 13),
                    M=M, h=h, state=st, touching=t(X["stance"]), mu=t(X["mu"]), command=t(command), nominal=t(nominal),
                    L=t(np.array(R.WEIGHTS12, np.float32)), limit=torch.tensor([m.effort[d] for d in range(m.nd)], device=dev))
        assert not _SET["jf"].is_contiguous() and not _SET["fp"].is_contiguous()
        c = lambda k: _SET[k].cpu().numpy().astype(np.float64)
        _SET["np"] = {k: c(k) for k in ("jf", "fp", "rs", "M", "h", "mu", "limit", "command", "nominal")}
        _SET["np"].update(touching=X["stance"], tick=st.tick.cpu().numpy(), target=st.target.cpu().numpy().astype(np.float64),
                          yaw=st.yaw.cpu().numpy().astype(np.float64))
    return _SET


class _StateView:
    """The first n envs of the GaitState (what glue.mpc_horizon reads of it)."""

    def __init__(self, st, sl):
        self.t = (st.tick[sl], st.sched[sl], st.anchor[sl], st.target[sl], st.yaw[sl])

    def tensors(self):
        return self.t


def _params():
    return G.params(DT, height=0.30, touchdown_z=0.01)


def _stance(S, gait, sl):
    """This tick's stance: scheduled by `gait` at the stored tick, and touching."""
    period, offsets, st = R.GAITS[gait]
    sched = ((S["np"]["tick"][sl, None] - 1) % period + np.asarray(offsets)[None]) % period < np.asarray(st)[None]
    return (sched & (S["np"]["touching"][sl] != 0)).astype(np.uint8)


def _tables_gpu(S, sl, H, Sx, gait):
    from shifu_amd import glue
    period, offsets, st = R.GAITS[gait]
    p = _params()
    par = _abi.ShfGaitParams(*[p[k] for k in G.PARAM_NAMES])
    stance = torch.from_numpy(_stance(S, gait, sl)).to(S["rs"].device)
    return glue.mpc_horizon(_StateView(S["state"], sl), stance, S["fp"][sl], S["command"][sl], S["nominal"], (period, offsets, st), par, H, Sx), stance


def _tables_ref(S, sl, H, Sx, gait, dtype=np.float64):
    N = S["np"]
    period, offsets, st = R.GAITS[gait]
    return R.horizon(N["tick"][sl], N["target"][sl], N["yaw"][sl], period, offsets, st, _stance(S, gait, sl), N["fp"][sl], N["command"][sl],
                     N["nominal"], _params(), H, Sx, dtype)


_RUNS = {}


def _run(case, u_io=None, warm_shift=0, iters=R.ITERS, cache=True):
    """One case on the GPU (tables, then the solve on them) and its float64 twin on the tables the GPU made."""
    from shifu_amd import glue
    key = (case, iters)
    if cache and u_io is None and key in _RUNS:
        return _RUNS[key]
    n, H, Sx, gait = case
    S = _setup()
    sl = slice(0, n)
    (contact, xref, pos), stance = _tables_gpu(S, sl, H, Sx, gait)
    delta = glue.mpc_step_dt(Sx, DT)
    forces, efforts = glue.foot_force_mpc(contact, xref, pos, S["rs"][sl], S["M"][sl], S["h"][sl], S["jf"][sl], S["mu"][sl], S["L"],
                                          R.ALPHA, FZ_MIN, FZ_MAX, iters, delta, S["h"][sl], S["limit"], u_io, warm_shift)
    torch.cuda.synchronize()
    N = S["np"]
    g = lambda a: a.cpu().numpy()
    prob = R.problem(g(contact), g(xref), g(pos), N["rs"][sl], N["M"][sl], N["h"][sl], delta)
    out = dict(contact=g(contact), xref=g(xref), pos=g(pos), forces=g(forces), efforts=g(efforts), prob=prob, stance=g(stance),
               tensors=(contact, xref, pos, stance))
    if u_io is None:
        u, state = R.twin(prob, N["mu"][sl], np.array(R.WEIGHTS12, np.float32).astype(np.float64), np.float64(np.float32(R.ALPHA)),
                          FZ_MIN, FZ_MAX, iters, return_state=True)
        free, tau = Q.efforts(N["jf"][sl], u[:, 0], N["h"][sl], N["limit"])
        out.update(u=u, x=state["x"], free=free, tau=tau)
        if cache:
            _RUNS[key] = out
    return out


# ------------------------------------------------------------------------------------------------------- kernel 1 --
@pytest.mark.parametrize("case", CASES, ids=str)
def test_horizon_matches_the_twin(case):
    """contact bit-equal; xref and pos within four times what float32 alone does to `horizon` on the same inputs."""
    _need_gpu()
    n, H, Sx, gait = case
    S = _setup()
    r = _run(case)
    c64, x64, p64 = _tables_ref(S, slice(0, n), H, Sx, gait)
    c32, x32, p32 = _tables_ref(S, slice(0, n), H, Sx, gait, np.float32)
    assert r["contact"].dtype == np.uint8 and np.array_equal(r["contact"], c64) and np.array_equal(c32, c64)
    dx, dp = np.abs(x32 - x64).max(), np.abs(p32 - p64).max()
    ex, ep = np.abs(r["xref"] - x64).max(), np.abs(r["pos"] - p64).max()
    print(f"[mpc gpu] horizon {case}: xref {ex:.3e} (float32 on the CPU {dx:.3e})  pos {ep:.3e} (float32 on the CPU {dp:.3e})")
    assert ex <= 4.0 * dx and ep <= 4.0 * dp
    off = r["contact"] == 0
    assert (r["pos"][off].view(np.uint32) == 0).all(), "entries without contact are +0.0"
    if n == 257:
        assert (r["contact"].reshape(n, -1)[1:] != r["contact"].reshape(n, -1)[:-1]).any(1).mean() > 0.5, "neighbouring envs differ"
        assert (r["contact"][:, 0].sum(1) == 0).any(), "some envs stand on nothing"
    if gait == "bound":
        assert (r["contact"].sum(2) == 0).any(), "rows with every foot in the air"


# ------------------------------------------------------------------------------------------------------- kernel 2 --
@pytest.mark.parametrize("case", CASES, ids=str)
def test_solve_matches_the_float64_twin(case):
    """Forces and efforts against the twin on the GPU's own tensors and tables; every inequality exact; bit-zero where nothing
    stands."""
    _need_gpu()
    n, H, Sx, gait = case
    r = _run(case)
    S = _setup()
    forces, efforts, u = r["forces"], r["efforts"], r["u"]
    assert forces.shape == (n, 4, 3) and efforts.shape == (n, 12) and np.isfinite(forces).all() and np.isfinite(efforts).all()
    ef = np.abs(forces - u[:, 0]).reshape(n, -1).max(1) / max(np.abs(u[:, 0]).max(), 1.0)
    et = np.abs(efforts - r["tau"]).max(1) / np.abs(r["free"]).max()
    mu = S["np"]["mu"][:n]
    near, scale = Q.face_distance(u[:, 0], r["contact"][:, 0], mu, FZ_MIN, FZ_MAX, x_raw=r["x"][:, 0])
    out = (ef > TOL["forces"]) | (et > TOL["efforts"])
    print(f"[mpc gpu] solve {case}: forces {ef.max():.3e}  efforts {et.max():.3e} (of the largest reference entry); "
          f"{int(out.sum())} envs beyond the bound (a clip that flips between the formats)")
    assert out.sum() == 0, f"{out.sum()} envs beyond the bound: forces {ef.max():.3e} efforts {et.max():.3e}"
    on = r["contact"][:, 0] != 0
    mu32 = S["mu"][:n].cpu().numpy()[:, None]
    fz = forces[..., 2]
    assert (fz[on] >= np.float32(FZ_MIN)).all() and (fz[on] <= np.float32(FZ_MAX)).all()
    bnd = mu32 * fz                                                         # the kernel's own float32 product
    assert (np.abs(forces[..., 0]) <= bnd)[on].all() and (np.abs(forces[..., 1]) <= bnd)[on].all()
    assert (forces[~on].view(np.uint32) == 0).all(), "forces of feet without contact are +0.0"
    none = ~on.any(1)
    if none.any():
        assert np.array_equal(efforts[none], np.clip(S["h"][:n].cpu().numpy()[none, 6:], -S["np"]["limit"].astype(np.float32),
                                                     S["np"]["limit"].astype(np.float32))), "nothing stands: the bias alone"


def test_nothing_standing_gives_the_bias_exactly():
    _need_gpu()
    from shifu_amd import glue
    S = _setup()
    n, H = 65, 3
    sl = slice(0, n)
    (contact, xref, pos), _ = _tables_gpu(S, sl, H, 6, "trot")
    contact = torch.zeros_like(contact)
    pos = torch.zeros_like(pos)
    f, tau = glue.foot_force_mpc(contact, xref, pos, S["rs"][sl], S["M"][sl], S["h"][sl], S["jf"][sl], 0.6, S["L"], R.ALPHA, FZ_MIN, FZ_MAX,
                                 20, glue.mpc_step_dt(6, DT), S["h"][sl], None)
    torch.cuda.synchronize()
    assert (f.cpu().numpy().view(np.uint32) == 0).all()
    assert torch.equal(tau, S["h"][sl][:, 6:])


def test_env_alone_among_others_and_permuted_and_strided_views():
    """An env's rows do not depend on its place in the launch or on its neighbours; views with strides equal contiguous copies."""
    _need_gpu()
    from shifu_amd import glue
    S = _setup()
    case = (65, 10, 6, "trot")
    n, H, Sx, gait = case
    r = _run(case)
    contact, xref, pos, stance = r["tensors"]
    delta = glue.mpc_step_dt(Sx, DT)
    e = 37

    def solve(idx):
        ix = torch.as_tensor(idx, device=contact.device)
        jf, rs = S["jf"][ix], S["rs"][ix]                       # gathered copies: contiguous
        assert jf.is_contiguous()
        f, tau = glue.foot_force_mpc(contact[ix], xref[ix], pos[ix], rs, S["M"][ix], S["h"][ix], jf, S["mu"][ix], S["L"], R.ALPHA, FZ_MIN,
                                     FZ_MAX, R.ITERS, delta, S["h"][ix], S["limit"])
        torch.cuda.synchronize()
        return f.cpu().numpy(), tau.cpu().numpy()

    f1, t1 = solve([e])
    assert np.array_equal(f1[0], r["forces"][e]) and np.array_equal(t1[0], r["efforts"][e]), "alone"
    idx = [3, 9, e] + list(range(40, 57))
    f2, t2 = solve(idx)
    assert np.array_equal(f2[2], r["forces"][e]) and np.array_equal(t2[2], r["efforts"][e]), "among 19 others"
    perm = np.random.default_rng(5).permutation(n)
    f3, t3 = solve(perm)
    assert np.array_equal(f3, r["forces"][perm]) and np.array_equal(t3, r["efforts"][perm]), "permuted"
    # the cached run read strided views of the Jacobian and of the root rows; a contiguous copy gives the same bits
    f4, t4 = solve(np.arange(n))
    assert np.array_equal(f4, r["forces"]) and np.array_equal(t4, r["efforts"]), "strided views against contiguous copies"
    # kernel 1: strided foot positions against a contiguous copy
    sl = slice(0, n)
    period, offsets, st = R.GAITS[gait]
    p = _params()
    par = _abi.ShfGaitParams(*[p[k] for k in G.PARAM_NAMES])
    c2, x2, p2 = glue.mpc_horizon(_StateView(S["state"], sl), stance, S["fp"][sl].contiguous(), S["command"][sl], S["nominal"],
                                  (period, offsets, st), par, H, Sx)
    assert torch.equal(c2, contact) and torch.equal(x2, xref) and torch.equal(p2, pos)


def test_warm_start_is_no_further_from_the_twin_than_the_cold_start():
    """u_io written by one call and read back with warm_shift = 0 starts the second call at the first one's solution: after
    fewer sweeps it is no further from the converged twin than the cold start after the same sweeps."""
    _need_gpu()
    case = (65, 10, 6, "trot")
    n, H = case[0], case[1]
    ref = _run(case, iters=400)["u"][:, 0]
    u_io = torch.zeros(n, H, 4, 3, device="cuda:0")
    first = _run(case, u_io=u_io, iters=R.ITERS)
    assert np.array_equal(first["forces"], _run(case)["forces"]), "a zero u_io is the cold start"
    assert np.array_equal(u_io[:, 0].cpu().numpy(), first["forces"]), "the solution's step 0 is forces_out"
    warm = _run(case, u_io=u_io, warm_shift=0, iters=40)
    cold = _run(case, iters=40, cache=False)
    scale = max(np.abs(ref).max(), 1.0)
    ew, ec = np.abs(warm["forces"] - ref).max() / scale, np.abs(cold["forces"] - ref).max() / scale
    print(f"[mpc gpu] 40 sweeps against the twin's 400: warm {ew:.3e}  cold {ec:.3e}")
    assert ew <= ec


# ------------------------------------------------------------------------------------------------------- kernel 3 --
def test_efforts_kernel_is_bit_equal_to_the_solve():
    _need_gpu()
    from shifu_amd import glue
    S = _setup()
    for case in (CASES[3], CASES[4]):
        n = case[0]
        r = _run(case)
        sl = slice(0, n)
        contact = r["tensors"][0]
        forces = torch.from_numpy(r["forces"]).to(contact.device)
        tau = glue.foot_force_efforts(forces, contact[:, 0].contiguous(), S["jf"][sl], S["h"][sl], S["limit"])
        torch.cuda.synchronize()
        assert np.array_equal(tau.cpu().numpy(), r["efforts"])
        # a foot that has lifted since counts as zero
        lifted = contact[:, 0].clone()
        lifted[:, 1] = 0
        f0 = forces.clone()
        f0[:, 1] = 0.0
        a = glue.foot_force_efforts(forces, lifted, S["jf"][sl], S["h"][sl], S["limit"])
        b = glue.foot_force_efforts(f0, contact[:, 0].contiguous(), S["jf"][sl], S["h"][sl], S["limit"])
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------- refusals --
def test_refusals():
    _need_gpu()
    from shifu_amd import glue
    from shifu_amd._lib import BackendError
    S = _setup()
    n = 2
    sl = slice(0, n)
    (contact, xref, pos), stance = _tables_gpu(S, sl, 3, 6, "trot")
    p = _params()
    par = _abi.ShfGaitParams(*[p[k] for k in G.PARAM_NAMES])
    tk = R.GAITS["trot"]
    sv = _StateView(S["state"], sl)

    def hz(H=3, Sx=6):
        return glue.mpc_horizon(sv, stance, S["fp"][sl], S["command"][sl], S["nominal"], tk, par, H, Sx)

    def mpc(**kw):
        a = dict(mu=0.6, alpha=R.ALPHA, fz_min=FZ_MIN, fz_max=FZ_MAX, iters=10, step_dt=0.03)
        a.update(kw)
        return glue.foot_force_mpc(contact, xref, pos, S["rs"][sl], S["M"][sl], S["h"][sl], S["jf"][sl], a["mu"], S["L"], a["alpha"], a["fz_min"],
                                   a["fz_max"], a["iters"], a["step_dt"], None, None)

    # (a horizon of 0 and the refusals glue cannot reach -- feet, dofs, null tensors -- are in tests/test_mpc_host.py)
    for call, text in ((lambda: hz(H=11), "horizon outside"), (lambda: hz(Sx=0), "ticks_per_step"),
                       (lambda: mpc(alpha=0.0), "alpha must be positive"), (lambda: mpc(fz_min=10.0, fz_max=5.0), "fz_min exceeds fz_max"),
                       (lambda: mpc(mu=-0.1), "mu must not be negative"), (lambda: mpc(iters=0), "iters must be at least 1"),
                       (lambda: mpc(step_dt=0.0), "step_dt must be positive")):
        with pytest.raises(BackendError, match=text):
            call()
    hz(); mpc()
    torch.cuda.synchronize()
