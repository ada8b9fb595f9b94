"""The balance controller's foot-force QP on the GPU (csrc/shf_qp.hip: shf_foot_force_qp) and what stands on it
(LeggedRobot.balance_control / apply_balance_control under SHIFU_AMD_FLOATING_DYNAMICS=1, FusedA1Env.balance_control).

The reference is the float64 twin of tests/qp_ref.py (the kernel's sweeps, operation by operation) on the GPU's own J, M and h.
Measured on an MI355X, the worst over every case of test_kernel_matches_the_float64_twin (WORST below): forces 1.75e-5 of the
largest reference force, efforts 1.47e-5 of the largest reference effort; asserted at four times that, never above 1e-4.  An env
may exceed the bound only if a clip flips between float32 and float64 -- its unclamped force within 1e-5 of a constraint face
in the twin -- and at most 1 % of a launch may; with this seed none does (tests/test_foot_force_qp_host.py shows the same for the
number format alone).

Stand and push run the loop of tests/balance_cpu.py (which holds the scenario and its CPU run: the oracle's float32 step with the
float64 twin as controller) on a bare sim under the TGS solver.  The CPU run's own worst error over the last 50 of 200 steps:
|z - 0.30| 3.91e-4 m, tilt 5.94e-3 rad.  GPU against CPU over the same steps (tests/golden/balance_stand_cpu.npz), measured on an
MI355X: z 2.98e-8 m, tilt 8.79e-8 rad (TRAJ below); the GPU run's own error 3.913e-4 m and 5.937e-3 rad.  The bound asserted is twice the CPU run's error plus that difference.
"""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import helpers as H
from tests import qp_ref as Q

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FEET = B.FEET
WORST = {"forces": 1.752e-5, "efforts": 1.474e-5}
TOL = {k: min(4.0 * v, 1e-4) for k, v in WORST.items()}
CPU_ERR = {"z": 3.914e-4, "tilt": 5.937e-3}           # python -m tests.balance_cpu
TRAJ = {"z": 2.980e-8, "tilt": 8.793e-8}                # GPU against the CPU run, the last 50 steps of the stand (MI355X)
BOUND = {k: 2.0 * CPU_ERR[k] + TRAJ[k] for k in CPU_ERR}
S6 = B.WEIGHTS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


def _sim(m, q, qd, root, params=None):
    import copy
    from shifu_amd.backend import Sim
    n, nd = q.shape
    sim = Sim(params if params is not None else H.sim_params(dt=0.005, gravity=B.GRAVITY), "cuda:0")
    sim.set_plane(1.0)
    sim.set_articulation(copy.deepcopy(m))
    sim.finalize(n, 0)
    dof = np.stack([q, qd], -1).reshape(n * nd, 2).astype(np.float32)
    for tid, a in ((_abi.T_SIM_DOF, dof), (_abi.T_DOF_STATE, dof), (_abi.T_SIM_ROOT, root), (_abi.T_ROOT_STATE, root)):
        sim.tensors[tid].copy_(torch.from_numpy(np.array(a, np.float32)))
    return sim


_SET = {}


def _setup():
    """The seeded launch (tests/balance_cpu.qp_states) on a bare A1 sim with its tensors refreshed, and the twin's inputs read
    back from the GPU: built once, shared, never modified."""
    if not _SET:
        m = H.a1_model().blob
        X = B.qp_states(m)
        n = B.QP_N
        sim = _sim(m, X["q"], X["qd"], X["root"])
        sim.refresh(_abi.REFRESH_ALL)
        D = m.nd + 6
        dev = sim.device
        M, h = torch.zeros(n, D, D, device=dev), torch.zeros(n, D, device=dev)
        jac = sim.tensors[_abi.T_JACOBIAN]
        sim.floating_dynamics(jac, M, h)
        torch.cuda.synchronize()
        body = sim.tensors[_abi.T_BODY_STATE].view(n, m.nb, 13)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        _SET.update(sim=sim, m=m, n=n, jf=jac[:, FEET[0]::4], fp=body[:, FEET[0]::4, :3], rs=sim.tensors[_abi.T_ROOT_STATE].view(n, 13),
                    M=M, h=h, target=t(X["target"]), stance=t(X["stance"]), mu=t(X["mu"]), f_prev=t(X["f_prev"]),
                    gains=t(B.gains12().astype(np.float32)), S=t(S6.astype(np.float32)),
                    limit=torch.tensor([m.effort[d] for d in range(m.nd)], device=dev))
        assert not _SET["jf"].is_contiguous() and not _SET["fp"].is_contiguous()
        c = lambda k: _SET[k].cpu().numpy().astype(np.float64)
        _SET["np"] = {k: c(k) for k in ("jf", "fp", "rs", "M", "h", "target", "mu", "f_prev", "limit")}
        _SET["np"]["stance"] = X["stance"]
        _SET["np"]["w"] = Q.wrench(c("M"), c("h"), c("rs"), c("target"), B.gains12().astype(np.float32).astype(np.float64))
        _SET["w32"] = t(_SET["np"]["w"].astype(np.float32))
    return _SET


CASES = {"dynamics": dict(wrench=False, beta=0.0, fz_max=float("inf"), per_env_mu=True, bias=True, limit=True),
         "wrench": dict(wrench=True, beta=0.05, fz_max=80.0, per_env_mu=False, bias=False, limit=False)}


def _launch(S, sl, case, **over):
    from shifu_amd import glue
    c = dict(CASES[case], **over)
    g = lambda k: S[k][sl]
    return glue.foot_force_qp(g("jf"), g("rs"), g("fp"), g("stance"), g("mu") if c["per_env_mu"] else 0.6, S["S"],
                              g("w32") if c["wrench"] else None, g("M"), g("h"), g("target"), S["gains"], 1e-2, c["beta"],
                              g("f_prev") if c["beta"] > 0 else None, 5.0, c["fz_max"], Q.ITERS, g("h") if c["bias"] else None,
                              S["limit"] if c["limit"] else None)


def _twin(S, sl, case):
    c, N = CASES[case], S["np"]
    g = lambda k: N[k][sl]
    w = g("w").astype(np.float32).astype(np.float64) if c["wrench"] else g("w")
    r = g("fp") - g("rs")[:, None, :3]
    mu = g("mu") if c["per_env_mu"] else np.float64(np.float32(0.6))
    f, state = Q.twin(r, w, S6, np.float64(np.float32(1e-2)), np.float64(np.float32(c["beta"])), g("f_prev") if c["beta"] > 0 else None,
                      g("stance"), mu, 5.0, c["fz_max"], return_state=True)
    free, tau = Q.efforts(g("jf"), f, g("h") if c["bias"] else None, N["limit"] if c["limit"] else None)
    near, scale = Q.face_distance(f, g("stance"), mu, 5.0, c["fz_max"], x_raw=state["x"])
    return f, free, tau, near.min(1) / np.maximum(scale, 1e-300)


# ---------------------------------------------------------------------------------------------------- against the twin --
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_matches_the_float64_twin(n, case):
    """Forces and efforts against the twin on the GPU's own tensors; stance patterns, friction and targets differ from env to
    env inside one launch.  'dynamics': the wrench formed in the kernel from M and h, per-env friction, bias and limits;
    'wrench': the wrench passed in, the beta term, an upper force bound, scalar friction."""
    _need_gpu()
    S = _setup()
    sl = slice(0, n)
    forces, efforts = _launch(S, sl, case)
    torch.cuda.synchronize()
    forces, efforts = forces.cpu().numpy(), efforts.cpu().numpy()
    f, free, tau, near = _twin(S, sl, case)
    assert forces.shape == (n, 4, 3) and efforts.shape == (n, 12) and np.isfinite(forces).all() and np.isfinite(efforts).all()
    ef = np.abs(forces - f).reshape(n, -1).max(1) / max(np.abs(f).max(), 1.0)
    et = np.abs(efforts - tau).max(1) / np.abs(free).max()
    print(f"[qp gpu] {case} n {n}: forces {ef.max():.3e}  efforts {et.max():.3e}  (of the largest reference entry)")
    out = (ef > TOL["forces"]) | (et > TOL["efforts"])
    assert out.sum() <= n // 100, f"{out.sum()} envs beyond the bound: forces {ef.max():.3e} efforts {et.max():.3e}"
    assert (near[out] <= 1e-5).all(), "an env beyond the bound must sit on a constraint face in the twin"
    if n == 257:
        st = S["np"]["stance"]
        assert len({tuple(r) for r in st}) >= 12 and (st.sum(1) == 0).any() and (st.sum(1) == 4).any(), "mixed stance patterns"
        assert (st[1:] != st[:-1]).any(1).mean() > 0.5, "neighbouring lanes take different branches"


def test_the_effort_step_alone_is_bit_equal_to_the_solver_s():
    """glue.foot_force_efforts on the forces foot_force_qp returned gives foot_force_qp's efforts bit for bit (one effort step in
    csrc/shf_cone.h behind both), and clearing a foot's stance is the same as zeroing its force.  The 'dynamics' case (bias and
    limits) at 65 envs: more than one block."""
    _need_gpu()
    from shifu_amd import glue
    S = _setup()
    sl = slice(0, 65)
    forces, efforts = _launch(S, sl, "dynamics")
    jf, stance, h = S["jf"][sl], S["stance"][sl], S["h"][sl]
    assert torch.equal(glue.foot_force_efforts(forces, stance, jf, h, S["limit"]), efforts)
    assert (forces[:, 1].abs().amax(1) > 0).sum() > 30, "the foot that is cleared below carries force in many envs"
    cleared, zeroed = stance.clone(), forces.clone()
    cleared[:, 1], zeroed[:, 1] = 0, 0.0
    a = glue.foot_force_efforts(forces, cleared, jf, h, S["limit"])
    b = glue.foot_force_efforts(zeroed, stance, jf, h, S["limit"])
    assert torch.equal(a, b) and not torch.equal(a, efforts)


def test_torch_fallback_on_the_gpu_matches_the_kernel_at_4096_envs():
    """utils.torch_utils.balance_wrench + foot_force_qp on CUDA float32 tensors (what LeggedRobot.balance_control runs when the
    kernel's input conditions are not met) against the kernel, on the seeded launch tiled to 4112 envs -- a batch size at which
    torch's batched Cholesky solver once returned wrong solutions inside this loop.  Both are float32 runs of the same sweeps
    and each lies within the twin's float32 figure of the float64 twin, so they agree within the cap of 1e-4."""
    _need_gpu()
    from shifu_amd.utils.torch_utils import balance_wrench, foot_force_qp
    S = _setup()
    B_ = {k: S[k].repeat((16,) + (1,) * (S[k].dim() - 1)) for k in ("jf", "rs", "fp", "stance", "mu", "w32", "M", "h", "target", "f_prev")}
    B_.update(S=S["S"], gains=S["gains"], limit=S["limit"])
    n = B_["rs"].shape[0]
    assert n == 4112
    fk, tk = _launch(B_, slice(None), "dynamics")
    w = balance_wrench(B_["M"], B_["h"], B_["rs"], B_["target"], S["gains"])
    ft, tt = foot_force_qp(B_["jf"], B_["rs"][:, :3], B_["fp"], w, B_["stance"], B_["mu"], S["S"], 1e-2, 0.0, None, 5.0, float("inf"),
                           Q.ITERS, B_["h"], S["limit"])
    torch.cuda.synchronize()
    ef = float((fk - ft).abs().max() / ft.abs().max())
    et = float((tk - tt).abs().max() / tt.abs().max())
    print(f"[qp gpu] torch fallback on the GPU against the kernel, {n} envs: forces {ef:.3e}  efforts {et:.3e}")
    assert ef <= 1e-4 and et <= 1e-4
    assert torch.equal(fk[:257], fk[257:514]), "tiled envs give bit-equal rows"


def test_forces_are_exactly_feasible_and_swing_feet_bit_zero():
    _need_gpu()
    S = _setup()
    for case in CASES:
        c = CASES[case]
        forces, _ = _launch(S, slice(None), case)
        torch.cuda.synchronize()
        on = S["stance"].bool()
        mu = (S["mu"] if c["per_env_mu"] else torch.full_like(S["mu"], 0.6)).view(-1, 1)
        fz = forces[..., 2]
        assert (forces.view(torch.int32)[~on] == 0).all(), "swing feet: +0.0 in every component"
        assert (fz[on] >= 5.0).all() and (fz[on] <= c["fz_max"]).all()
        bound = mu * fz                                   # the kernel's own float32 product
        assert (forces[..., 0].abs() <= bound)[on].all() and (forces[..., 1].abs() <= bound)[on].all()
        assert ((forces[..., 0].abs() == bound) & on).any(), "some cone is active in this launch"


def test_an_env_does_not_depend_on_its_neighbours():
    """Alone, among 19 and permuted: bit-equal rows."""
    _need_gpu()
    S = _setup()
    for case in CASES:
        f_all, t_all = _launch(S, slice(None), case)
        f19, t19 = _launch(S, slice(0, 19), case)
        f1, t1 = _launch(S, slice(7, 8), case)
        perm = torch.randperm(S["n"], generator=torch.Generator().manual_seed(3)).to(S["M"].device)
        P = dict(S)
        for k in ("jf", "rs", "fp", "stance", "mu", "w32", "M", "h", "target", "f_prev"):
            P[k] = S[k][perm].contiguous()
        fp_, tp_ = _launch(P, slice(None), case)
        torch.cuda.synchronize()
        assert torch.equal(f19, f_all[:19]) and torch.equal(t19, t_all[:19])
        assert torch.equal(f1, f_all[7:8]) and torch.equal(t1, t_all[7:8])
        assert torch.equal(fp_, f_all[perm]) and torch.equal(tp_, t_all[perm])


def test_strided_views_equal_contiguous_copies():
    """The feet as slices of the Jacobian and body-state tensors, the root row of the 13-wide root state: bit-equal to contiguous
    copies, and to a root view inside a wider tensor."""
    _need_gpu()
    S = _setup()
    for case in CASES:
        a = _launch(S, slice(None), case)
        C = dict(S)
        C["jf"], C["fp"] = S["jf"].contiguous(), S["fp"].contiguous()
        wide = torch.zeros(S["n"], 20, device=S["M"].device)
        wide[:, :13] = S["rs"]
        C["rs"] = wide[:, :13]
        b = _launch(C, slice(None), case)
        torch.cuda.synchronize()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_effort_path_follows_the_foot_controller():
    """Nothing standing: the efforts are bias[:, 6:] exactly (zeros without bias).  The clamp comes last and entries <= 0 of the
    limit mean no limit."""
    _need_gpu()
    S = _setup()
    Z = dict(S)
    Z["stance"] = torch.zeros_like(S["stance"])
    f, tau = _launch(Z, slice(None), "dynamics", limit=False)
    f0, tau0 = _launch(Z, slice(None), "dynamics", limit=False, bias=False)
    torch.cuda.synchronize()
    assert (f == 0).all() and (f0 == 0).all() and torch.equal(tau, S["h"][:, 6:]) and (tau0 == 0).all()
    sl = slice(0, 2)
    assert int(S["stance"][sl].sum()) >= 4
    _, free = _launch(S, sl, "dynamics", limit=False)
    _, nobias = _launch(S, sl, "dynamics", limit=False, bias=False)
    lim = 0.5 * free.abs().min(0).values
    assert float(lim.min()) > 0.0
    lim[1], lim[4] = 0.0, -1.0
    L = dict(S)
    L["limit"] = lim
    _, got = _launch(L, sl, "dynamics")
    torch.cuda.synchronize()
    assert torch.equal(free, nobias + S["h"][sl, 6:]), "bias[:, 6:] is added to the finished sum"
    assert torch.equal(got, torch.where(lim > 0, torch.maximum(torch.minimum(free, lim), -lim), free))


# ------------------------------------------------------------------------------------------------------ stand and push --
def _loop(steps, controlled=True, push=False):
    """tests/balance_cpu.run on the GPU: refresh, stance from the contact tensor, shf_foot_force_qp for the stance feet plus the
    Cartesian hold of shf_foot_impedance on the other legs, one simulate() per step."""
    from shifu_amd import glue
    m = H.a1_model().blob
    q, qd, root, target = B.initial_state(m)
    n = B.N_ENVS
    sim = _sim(m, q, qd, root, params=B.params())
    dev = sim.device
    D = m.nd + 6
    M, h = torch.zeros(n, D, D, device=dev), torch.zeros(n, D, device=dev)
    jac = sim.tensors[_abi.T_JACOBIAN]
    body = sim.tensors[_abi.T_BODY_STATE].view(n, m.nb, 13)
    rs = sim.tensors[_abi.T_ROOT_STATE].view(n, 13)
    contact = sim.tensors[_abi.T_CONTACT].view(n, m.nb, 3)
    dof = sim.tensors[_abi.T_DOF_STATE].view(n, m.nd, 2)
    jf, fp = jac[:, FEET[0]::4], body[:, FEET[0]::4, :3]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    tg, gains, S = t(target), t(B.gains12()), t(S6)
    hold = t(np.broadcast_to(B.swing_targets(m), (n, 4, 3)))
    kp3 = torch.full((3,), B.SWING_KP, device=dev)
    kd3 = 2.0 * torch.sqrt(kp3)
    limit = torch.tensor([m.effort[d] for d in range(m.nd)], device=dev)
    force = torch.zeros(n, m.nb, 3, device=dev)
    zs, tilts, ys, ok = [], [], [], True
    for s in range(steps):
        sim.refresh(_abi.REFRESH_ALL)
        if controlled:
            sim.floating_dynamics(jac, M, h)
            stance = (contact[:, FEET[0]::4, 2] > 1.0).to(torch.uint8)
            forces, tau = glue.foot_force_qp(jf, rs, fp, stance, B.MU, S, None, M, h, tg, gains, B.ALPHA, 0.0, None, B.FZ_MIN,
                                             float("inf"), Q.ITERS, h, limit)
            swing = glue.foot_impedance(jf, dof, rs, fp, hold, kp3, kd3, None, limit)
            tau = torch.maximum(torch.minimum(tau + (1.0 - stance.float()).repeat_interleave(3, 1) * swing, limit), -limit)
            on = stance.bool()
            ok = ok and bool((forces[..., 2][on] >= B.FZ_MIN).all()) and bool((forces[~on] == 0).all())
            ok = ok and bool((forces[..., :2].abs() <= (B.MU * forces[..., 2:3]))[on].all())
        else:
            tau = torch.zeros(n, m.nd, device=dev)
        sim.set_dof_command(_abi.T_EFFORT, tau)
        if push:
            force[:, 0, 1] = B.PUSH if B.PUSH_FROM <= s < B.PUSH_FROM + B.PUSH_STEPS else 0.0
            sim.apply_body_force(force.view(-1, 3))
        sim.step()
        sim.refresh(_abi.REFRESH_ROOT)
        r = rs.cpu().numpy()
        zs.append(r[:, 2].copy()); tilts.append(B.tilt_of(r[:, 3:7])); ys.append(r[:, 1].copy())
    sim.refresh(_abi.REFRESH_ALL)
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(sim.tensors[k]).all()) for k in (_abi.T_DOF_STATE, _abi.T_ROOT_STATE, _abi.T_BODY_STATE))
    return np.array(zs), np.array(tilts), np.array(ys), ok, finite


def test_the_robots_collapse_without_the_controller():
    _need_gpu()
    z, _, _, _, finite = _loop(B.STEPS, controlled=False)
    print(f"[stand] no controller: base z after {B.STEPS} steps {z[-1].min():.4f} .. {z[-1].max():.4f}")
    assert finite and (z[-1] < 0.15).all()


def test_balance_control_stands_the_robots_up():
    """8 A1s dropped from 2 cm above their standing height, tilted and with joint offsets: after 150 of 200 steps of 5 ms the
    base stays within BOUND of 0.30 m and of upright."""
    _need_gpu()
    z, tilt, _, ok, finite = _loop(B.STEPS)
    gold = np.load(B.GOLDEN)
    ez, et = B.stand_errors(z, tilt)
    dz, dt = float(np.abs(z[-50:] - gold["z"][-50:]).max()), float(np.abs(tilt[-50:] - gold["tilt"][-50:]).max())
    print(f"[stand] worst |z - 0.30| {ez:.3e} m, tilt {et:.3e} rad over the last 50 steps; against the CPU run: z {dz:.3e}, tilt {dt:.3e}")
    assert finite and ok, "finite state; every force inside its cone at every step"
    assert ez <= BOUND["z"] and et <= BOUND["tilt"]
    # the GPU run follows the CPU run: further from it than the CPU run is from its own target would be drift, not rounding
    assert dz <= CPU_ERR["z"] and dt <= CPU_ERR["tilt"]


def test_a_lateral_push_is_absorbed_without_leaving_the_cones():
    """30 N along +y on the base for 20 steps: no stance force ever leaves its cone, and 100 steps after the push ends the base
    is back within the stand bound."""
    _need_gpu()
    z, tilt, y, ok, finite = _loop(B.PUSH_FROM + B.PUSH_STEPS + 100, push=True)
    ez, et = B.stand_errors(z, tilt, last=1)
    print(f"[push] peak |y - y0| {np.abs(y).max():.3e} m; 100 steps after the push: |z - 0.30| {ez:.3e} m, tilt {et:.3e} rad")
    assert finite and ok
    assert np.abs(y).max() > 2e-3, "the push moved the base"
    assert ez <= BOUND["z"] and et <= BOUND["tilt"]


# ------------------------------------------------------------------------------------------------------------ plumbing --
def _legged_env(n):
    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.units import LeggedRobot

    class EnvCfg(BaseEnvConfig):
        num_envs = n

        class control(BaseEnvConfig.control):
            decimation = 1

        class debug(BaseEnvConfig.debug):
            headless = True

    env = IsaacGymEnv(EnvCfg())
    robot = LeggedRobot(A1ActorConfig())
    env.create_envs(robot=robot)
    return env, robot


def test_legged_robot_balance_control_plumbing(monkeypatch):
    """With the variable set: balance_control returns (efforts, forces) of the documented shapes, finite, inside the limits and
    the cones, equal to the backend call on the same tensors; its tensors are allocated once; apply_balance_control runs an env
    step with and without swing targets.  Unset, the calls raise the facade's 'fixed base' error."""
    _need_gpu()
    from shifu_amd import glue
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    n = 4
    env, robot = _legged_env(n)
    nd = robot.num_dof
    robot.mass_matrix, robot.bias_forces
    env.gym.refresh_all_state_tensors(env.sim)
    env.gym.refresh_mass_matrix_tensors(env.sim)
    root = env.root_state.view(n, -1, 13)[:, 0]
    pos, quat = root[:, :3].clone(), root[:, 3:7].clone()
    stance = torch.tensor([[1, 1, 1, 1], [1, 0, 0, 1], [0, 0, 0, 0], [1, 1, 0, 1]], dtype=torch.uint8, device=robot.device)
    tau, f = robot.balance_control(pos, quat, stance=stance)
    p0, m0 = robot._bal_target.data_ptr(), robot.mass_matrix.data_ptr()
    tau2, f2 = robot.balance_control(pos, quat, stance=stance)
    torch.cuda.synchronize()
    assert robot._bal_target.data_ptr() == p0 and robot.mass_matrix.data_ptr() == m0
    assert tuple(tau.shape) == (n, nd) and tuple(f.shape) == (n, 4, 3) and torch.equal(tau, tau2) and torch.equal(f, f2)
    assert torch.isfinite(tau).all() and (tau.abs() <= robot.torque_limits).all()
    mu = robot._contact_friction()
    assert tuple(mu.shape) == (n,) and (f[~stance.bool()] == 0).all() and (f[..., 2][stance.bool()] >= 5.0).all()
    assert (f[..., :2].abs() <= mu.view(n, 1, 1) * f[..., 2:3])[stance.bool()].all()
    assert torch.equal(tau[2], robot.bias_forces[2, 6:].clamp(-robot.torque_limits, robot.torque_limits)), "nothing stands: the bias alone"
    kp, ka = torch.full((3,), 100.0, device=robot.device), torch.full((3,), 400.0, device=robot.device)
    gains = torch.cat([kp, 2 * torch.sqrt(kp), ka, 2 * torch.sqrt(ka)])
    tg = torch.zeros(n, 13, device=robot.device)
    tg[:, :3], tg[:, 3:7] = pos, quat
    feet = env.body_state.view(n, -1, 13)[:, [int(b) for b in robot.ee_indices.cpu()], :3].contiguous()
    fb, tb = glue.foot_force_qp(robot.foot_jacobians, root, feet, stance, mu, torch.tensor([1., 1, 1, 10, 10, 10], device=robot.device),
                                None, robot.mass_matrix, robot.bias_forces, tg, gains, bias=robot.bias_forces,
                                effort_limit=robot.torque_limits.contiguous())
    assert torch.equal(fb, f) and torch.equal(tb, tau)
    assert tuple(robot.stance_from_contacts().shape) == (n, 4)
    for swing in (None, torch.zeros(n, 4, 3, device=robot.device) + torch.tensor([0.0, 0.0, -0.3], device=robot.device)):
        e, ff = robot.apply_balance_control(pos, quat, swing_targets=swing)
        env.gym.refresh_all_state_tensors(env.sim)
        torch.cuda.synchronize()
        assert tuple(e.shape) == (n, nd) and (e.abs() <= robot.torque_limits).all() and torch.isfinite(ff).all()
        assert torch.isfinite(env.dof_state).all() and torch.isfinite(env.root_state).all() and torch.isfinite(env.body_state).all()
    monkeypatch.delenv("SHIFU_AMD_FLOATING_DYNAMICS")
    robot._mass_matrix = robot._bias_forces = None
    with pytest.raises(Exception, match="fixed base"):
        robot.balance_control(pos, quat)
    with pytest.raises(Exception, match="fixed base"):
        robot.apply_balance_control(pos, quat)


def test_balance_control_needs_effort_mode(monkeypatch):
    _need_gpu()
    from shifu_amd.isaacgym import gymapi
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    env, robot = _legged_env(2)
    monkeypatch.setattr(robot.asset_options, "default_dof_drive_mode", gymapi.DOF_MODE_POS)
    z = torch.zeros(2, 3, device=robot.device)
    with pytest.raises(RuntimeError, match="apply_balance_control: the asset's default_dof_drive_mode must be DOF_MODE_EFFORT"):
        robot.apply_balance_control(z, torch.tensor([[0.0, 0.0, 0.0, 1.0]] * 2, device=robot.device))


def test_fused_env_balance_control_equals_the_backend_call():
    _need_gpu()
    from shifu_amd import glue
    from shifu_amd.gym.a1_fused import FusedA1Env
    n = 8
    env = FusedA1Env(num_envs=n, terrain="flat")
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        for _ in range(5):
            env.step(0.2 * (2 * torch.rand(n, 12, device=env.device, generator=g) - 1))
        pos, quat = env.root_state[:, :3].clone(), env.root_state[:, 3:7].clone()
        pos[:, 2] += 0.02
        tau, f = env.balance_control(pos, quat)
        w = env.whole_body_dynamics()
        nb = env.cm.blob.nb
        feet = env.body_state.view(n, nb, 13)[:, 4::4, :3]
        stance = (env.contact_state.view(n, nb, 3)[:, 4::4, 2] > 1.0).to(torch.uint8)
        mu = 0.5 * (env.sim.tensors[_abi.T_FRICTION] + float(env.sim.terrain.friction))
        kp, ka = torch.full((3,), 100.0, device=env.device), torch.full((3,), 400.0, device=env.device)
        tg = torch.zeros(n, 13, device=env.device)
        tg[:, :3], tg[:, 3:7] = pos, quat
        limit = torch.tensor([env.cm.blob.effort[d] for d in range(12)], device=env.device)
        fb, tb = glue.foot_force_qp(env.foot_jacobians, env.root_state.view(n, 13), feet, stance, mu,
                                    torch.tensor([1., 1, 1, 10, 10, 10], device=env.device), None, w["mass_matrix"], w["bias"], tg,
                                    torch.cat([kp, 2 * torch.sqrt(kp), ka, 2 * torch.sqrt(ka)]), bias=w["bias"], effort_limit=limit)
        torch.cuda.synchronize()
        assert tuple(tau.shape) == (n, 12) and tuple(f.shape) == (n, 4, 3)
        assert torch.equal(fb, f) and torch.equal(tb, tau) and torch.isfinite(tau).all()
        assert int(stance.sum()) > 0 and float(f[..., 2].max()) >= 5.0, "some foot stands and carries load"
        p0 = env._bal_target.data_ptr()
        tau2, _ = env.balance_control(pos, quat)
        torch.cuda.synchronize()
        assert env._bal_target.data_ptr() == p0 and torch.equal(tau2, tau), "the target buffer is allocated once"
    finally:
        env.destroy()
