"""The gait planner and the effort merge on the GPU (csrc/shf_gait.hip: shf_gait_plan, shf_leg_effort_mix) and what stands on
them (glue.locomotion_control, LeggedRobot.locomotion_control / apply_locomotion_control under SHIFU_AMD_FLOATING_DYNAMICS=1,
FusedA1Env.locomotion_control).

Kernel against twin.  The reference is the float64 twin of tests/gait_ref.py on the GPU's own root and foot tensors, 70
consecutive calls with the state carried on each side.  The integer outputs (stance, sched, tick) must be bit-equal at every
call.  The float outputs are measured as the largest difference over a launch divided by max(largest reference entry, 1);
WORST below holds the worst over every case and call measured on an MI355X (swing targets 5.9e-7, anchors 1.8e-7, base target
2.1e-6, heading 2.6e-6 -- 70 float32 additions of yaw rate x dt --, phase 2.8e-8), asserted at four times that and never above
1e-4.

Closed loop.  tests/trot_cpu.py holds the scenario (8 A1s, 100 ticks of Gait.stand(), 500 ticks of Gait.trot() at 0.3 m/s) and
its CPU run, whose figures are CPU below: peak tilt 0.2116 rad, worst speed error over the last five periods 8.63e-5 of the
command, lowest base height 0.2893 m.  The GPU run shares the physics but not the controller's number format, and a trot is
not contractive, so the two part at contact events; what is asserted is that every env and step is finite, the base stays above
0.2 m, no stance force leaves its cone, the peak tilt is at most twice the CPU run's and the speed error at most twice the CPU
run's worst.  The GPU run's own figures on an MI355X are GPU below: peak tilt 0.2116 rad, speed error 1.350e-4, lowest base height
0.2893 m.
"""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import gait_ref as G
from tests import helpers as H
from tests import trot_cpu as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FEET = B.FEET
CALLS = 70
WORST = {"swing_target": 5.945e-7, "anchor": 1.755e-7, "target": 2.106e-6, "yaw": 2.555e-6, "phase": 2.782e-8}     # MI355X, see the docstring
TOL = {k: min(4.0 * v, 1e-4) for k, v in WORST.items()}
CPU = {"tilt": 0.2116, "speed": 8.63e-5, "z_min": 0.2893}         # python -m tests.trot_cpu
GPU = {"tilt": 0.2116, "speed": 1.350e-4, "z_min": 0.2893}        # the same figures of the GPU run (MI355X)
STAND_BOUND = {"z": 2.0 * 3.914e-4 + 2.980e-8, "tilt": 2.0 * 5.937e-3 + 8.793e-8}      # BOUND of tests/test_gpu_foot_force_qp.py


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
    """The seeded launch of tests/balance_cpu.qp_states on a bare A1 sim with its tensors refreshed; per call a seeded contact
    tensor; per env a command in +-0.5 m/s / +-1 rad/s and a start tick; resets for every env at call 0 and for one env in eight
    at calls 25 and 26.  Built once, shared, never modified."""
    if not _SET:
        from shifu_amd.units.gait import Gait
        m = H.a1_model().blob
        X = B.qp_states(m)
        n = B.QP_N
        sim = _sim(m, X["q"], X["qd"], X["root"])
        sim.refresh(_abi.REFRESH_ALL)
        torch.cuda.synchronize()
        dev = sim.device
        body = sim.tensors[_abi.T_BODY_STATE].view(n, m.nb, 13)
        rng = np.random.default_rng(77)
        contact = np.where(rng.uniform(size=(CALLS, n, m.nb, 3)) < 0.25, rng.uniform(0, 1, (CALLS, n, m.nb, 3)),
                           rng.uniform(1, 40, (CALLS, n, m.nb, 3))).astype(np.float32)
        command = np.stack([rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-1, 1, n)], 1).astype(np.float32)
        start = rng.integers(0, 60, n).astype(np.int32)
        reset = np.zeros((CALLS, n), np.uint8)
        reset[0] = 1
        reset[25, 3::8], reset[26, 5::8] = 1, 1
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        gait = Gait.trot(leash=0.05)                                # a leash short enough to bind on some envs within 70 calls
        _SET.update(sim=sim, m=m, n=n, rs=sim.tensors[_abi.T_ROOT_STATE].view(n, 13), fp=body[:, FEET[0]::4, :3], contact=t(contact),
                    command=t(command), start=t(start), reset=t(reset), nominal=t(B.swing_targets(m).astype(np.float32)), gait=gait,
                    ticks=gait.ticks(0.005), P=G.params(0.005, height=B.HEIGHT, touchdown_z=T.foot_radius(m) - T.TOUCHDOWN_DEPTH, leash=0.05))
        assert not _SET["fp"].is_contiguous()
        c = lambda k: _SET[k].cpu().numpy()
        _SET["np"] = {"rs": c("rs").astype(np.float64), "fp": c("fp").astype(np.float64), "contact": contact[:, :, FEET[0]::4, 2].astype(np.float64),
                      "command": command.astype(np.float64), "start": start, "reset": reset, "nominal": c("nominal").astype(np.float64)}
    return _SET


def _params(S):
    return _abi.ShfGaitParams(*[S["P"][k] for k in G.PARAM_NAMES])


def _plan(S, state, sl, call, with_contact=True, fp=None, rs=None):
    from shifu_amd import glue
    cz = S["contact"][call][sl][:, FEET[0]::4, 2] if with_contact else None
    return glue.gait_plan(state, (S["rs"] if rs is None else rs)[sl], (S["fp"] if fp is None else fp)[sl], cz, S["command"][sl], S["nominal"],
                          S["reset"][call][sl], S["ticks"], _params(S))


def _fresh_state(S, sl, scramble=True):
    """A GaitState whose contents before the first (resetting) call are junk, so that the reset has something to overwrite."""
    from shifu_amd.units.gait import GaitState
    n = S["rs"][sl].shape[0]
    st = GaitState(n, 4, S["rs"].device)
    if scramble:
        st.tick.fill_(1234), st.sched.zero_(), st.anchor.fill_(3.0), st.target.fill_(-2.0), st.yaw.fill_(0.5)
    return st


def _clone(st):
    from shifu_amd.units.gait import GaitState
    c = GaitState(st.n, st.F, st.tick.device)
    for a, b in zip(c.tensors() + (c.pending,), st.tensors() + (st.pending,)):
        a.copy_(b)
    c.any_pending = st.any_pending
    return c


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors()))


# ---------------------------------------------------------------------------------------------------- against the twin --
@pytest.mark.parametrize("with_contact", [True, False], ids=["contact", "schedule-only"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_kernel_matches_the_float64_twin_over_70_calls(n, with_contact):
    """State carried on the GPU and in the twin side by side: integers bit-equal at every call, floats within TOL.  After the
    first call the clocks are set to per-env start ticks, so that neighbouring lanes are in different phases."""
    _need_gpu()
    S = _setup()
    N = S["np"]
    sl = slice(0, n)
    gs = _fresh_state(S, sl)
    ts = G.new_state(n, 4)
    ts["tick"][:], ts["sched"][:], ts["anchor"][:], ts["target"][:], ts["yaw"][:] = 1234, 0, 3.0, -2.0, 0.5
    worst = {k: 0.0 for k in WORST}
    seen = {"lift": 0, "down": 0, "late": 0, "swing": 0, "leash": 0, "branches": 0.0}
    prev = None
    for c in range(CALLS):
        if c == 1:
            gs.tick.copy_(S["start"][sl])
            ts["tick"][:] = N["start"][sl]
        stance, swing, phase = _plan(S, gs, sl, c, with_contact)
        o = G.plan(ts, N["rs"][sl], N["fp"][sl], N["contact"][c][sl] if with_contact else None, N["command"][sl], N["nominal"],
                   N["reset"][c][sl], *S["ticks"], S["P"])
        torch.cuda.synchronize()
        assert np.array_equal(stance.cpu().numpy(), o["stance"]), f"stance, call {c}"
        assert np.array_equal(gs.sched.cpu().numpy(), ts["sched"]) and np.array_equal(gs.tick.cpu().numpy(), ts["tick"]), f"schedule, call {c}"
        for k, got, ref in (("swing_target", swing, o["swing_target"]), ("phase", phase, o["phase"]), ("anchor", gs.anchor, ts["anchor"]),
                            ("target", gs.target, ts["target"]), ("yaw", gs.yaw, ts["yaw"])):
            g = got.cpu().numpy()
            assert np.isfinite(g).all()
            worst[k] = max(worst[k], float(np.abs(g - ref).max() / max(np.abs(ref).max(), 1.0)))
        sc = o["scheduled"]
        if prev is not None:
            seen["lift"] += int(((prev == 1) & (sc == 0)).sum())
            seen["down"] += int(((prev == 0) & (sc == 1)).sum())
        prev = sc
        seen["late"] += int(((sc == 1) & (o["stance"] == 0)).sum())
        seen["swing"] += int((sc == 0).sum())
        d = ts["target"][:, :2] - N["rs"][sl][:, :2]
        seen["leash"] += int((np.abs(np.hypot(d[:, 0], d[:, 1]) - S["P"]["leash"]) < 1e-9).sum())
        if n > 1:
            seen["branches"] = max(seen["branches"], float((sc[1:] != sc[:-1]).any(1).mean()))
    print(f"[gait gpu] n {n} {'contact' if with_contact else 'schedule only'}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for k in WORST:
        assert worst[k] <= TOL[k], (k, worst[k], TOL[k])
    # 69 ticks after the start ticks are set: every foot lifts off and touches down once at least; a reset in between can take
    # one event of a foot away
    assert seen["lift"] >= 3 * n and seen["down"] >= 3 * n and seen["swing"] > 0
    assert (seen["late"] > 0) == with_contact
    if n == 257:
        assert seen["leash"] > 0, "the leash binds somewhere"
        assert seen["branches"] > 0.3, "neighbouring lanes take different branches"


# ---------------------------------------------------------------------------------------------------- bit-level properties --
def _advance(S, sl, calls, **kw):
    st = _fresh_state(S, sl)
    out = None
    for c in range(calls):
        if c == 1:
            st.tick.copy_(S["start"][sl])
        out = _plan(S, st, sl, c, **kw)
    return st, out


def test_an_env_does_not_depend_on_its_neighbours():
    """Alone, among 19 and permuted: bit-equal rows, after 40 calls (events and resets behind them)."""
    _need_gpu()
    S = _setup()
    n = S["n"]
    st_all, out_all = _advance(S, slice(None), 40)
    st19, out19 = _advance(S, slice(0, 19), 40)
    st1, out1 = _advance(S, slice(7, 8), 40)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to(S["rs"].device)
    Pm = dict(S)
    for k in ("rs", "fp", "command", "start"):
        Pm[k] = S[k][perm].contiguous()
    Pm["contact"], Pm["reset"] = S["contact"][:, perm].contiguous(), S["reset"][:, perm].contiguous()
    stp, outp = _advance(Pm, slice(None), 40)
    torch.cuda.synchronize()
    for a, b in zip(out19 + st19.tensors(), out_all + st_all.tensors()):
        assert torch.equal(a, b[:19])
    for a, b in zip(out1 + st1.tensors(), out_all + st_all.tensors()):
        assert torch.equal(a, b[7:8])
    for a, b in zip(outp + stp.tensors(), out_all + st_all.tensors()):
        assert torch.equal(a, b[perm])


def test_strided_views_equal_contiguous_copies_and_a_launch_repeats_itself():
    _need_gpu()
    S = _setup()
    n = S["n"]
    base, _ = _advance(S, slice(None), 33)
    a_st, b_st, c_st = _clone(base), _clone(base), _clone(base)
    a = _plan(S, a_st, slice(None), 33)
    wide = torch.zeros(n, 20, device=S["rs"].device)
    wide[:, :13] = S["rs"]
    b = _plan(S, b_st, slice(None), 33, fp=S["fp"].contiguous(), rs=wide[:, :13])
    c = _plan(S, c_st, slice(None), 33)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and _same(a_st, b_st), "strided views against contiguous copies"
    assert all(torch.equal(x, y) for x, y in zip(a, c)) and _same(a_st, c_st), "the same launch twice from the same state"
    assert not _same(a_st, base)


def test_leg_effort_mix_equals_its_torch_expression_bit_for_bit():
    _need_gpu()
    from shifu_amd import glue
    from shifu_amd.utils import torch_utils as TU
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(5)
    chain = torch.from_numpy(T.chain_mask(H.a1_model().blob)).to(dev)
    limit = torch.full((12,), 15.0, device=dev)
    limit[2], limit[7] = 0.0, -1.0
    for n in (1, 63, 64, 65, 257):
        a, b = 20 * torch.randn(n, 12, device=dev, generator=g), 20 * torch.randn(n, 12, device=dev, generator=g)
        a[0, 0], b[0, 1] = -0.0, -0.0
        stance = (torch.rand(n, 4, device=dev, generator=g) < 0.5).to(torch.uint8)
        for lim in (limit, None):
            got, want = glue.leg_effort_mix(a, b, stance, chain, lim), TU.leg_effort_mix(a, b, stance, chain, lim)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (n, lim is None)


# ------------------------------------------------------------------------------------------------------- closed loop --
def _loop(settle, trot, vx=T.VX):
    """tests/trot_cpu.run on the GPU: per tick refresh, J / M / h, glue.locomotion_control (four launches), one simulate()."""
    from shifu_amd import glue
    from shifu_amd.units.gait import Gait, GaitState
    m = H.a1_model().blob
    q, qd, root, _ = B.initial_state(m)
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
    jf, fp, cz = jac[:, FEET[0]::4], body[:, FEET[0]::4, :3], contact[:, FEET[0]::4, 2]
    limit = torch.tensor([m.effort[d] for d in range(m.nd)], device=dev)
    chain = torch.from_numpy(T.chain_mask(m)).to(dev)
    nominal = torch.from_numpy(B.swing_targets(m).astype(np.float32)).to(dev)
    stand, trot_g = Gait.stand(), Gait.trot()
    assert stand.ticks(T.DT) == T.STAND_TICKS and trot_g.ticks(T.DT) == T.TROT_TICKS
    state = GaitState(n, 4, dev)
    command = torch.zeros(n, 3, device=dev)
    fric = sim.tensors[_abi.T_FRICTION]
    ok = torch.ones((), dtype=torch.bool, device=dev)
    rows = []
    for s in range(settle + trot):
        sim.refresh(_abi.REFRESH_ALL)
        sim.floating_dynamics(jac, M, h)
        if s == settle:
            state.tick.zero_()
            command[:, 0] = vx
        tau, forces, stance, _ = glue.locomotion_control(jf, dof, rs, fp, cz, fric, 1.0, M, h, limit, chain, nominal, state, command,
                                                         trot_g if s >= settle else stand, T.DT, B.HEIGHT, T.foot_radius(m) - T.TOUCHDOWN_DEPTH,
                                                         T.SWING_KP, T.SWING_KD, mu=B.MU)
        on = stance.bool()
        ok = ok & (forces[..., 2] >= B.FZ_MIN)[on].all() & (forces[~on] == 0).all() & (forces[..., :2].abs() <= B.MU * forces[..., 2:3])[on].all()
        sim.set_dof_command(_abi.T_EFFORT, tau)
        sim.step()
        sim.refresh(_abi.REFRESH_ROOT)
        rows.append(rs[:, :7].clone())
    sim.refresh(_abi.REFRESH_ALL)
    torch.cuda.synchronize()
    finite = all(bool(torch.isfinite(sim.tensors[k]).all()) for k in (_abi.T_DOF_STATE, _abi.T_ROOT_STATE, _abi.T_BODY_STATE))
    r = torch.stack(rows).cpu().numpy()
    tilt = np.stack([B.tilt_of(r[s, :, 3:7]) for s in range(r.shape[0])])
    return r[..., 0].astype(np.float64), r[..., 2].astype(np.float64), tilt, bool(ok), finite and bool(np.isfinite(r).all())


def test_the_a1_trots_at_the_commanded_speed():
    """The scenario of tests/trot_cpu.py with the kernels: conditions on every env and step, and the two figures measured against
    the CPU run's (the module docstring)."""
    _need_gpu()
    x, z, tilt, ok, finite = _loop(T.SETTLE, T.TROT)
    pt, zmin, es = T.figures(x, z, tilt)
    gold = np.load(T.GOLDEN)
    cpt, czmin, ces = T.figures(gold["x"].astype(np.float64), gold["z"].astype(np.float64), gold["tilt"].astype(np.float64))
    print(f"[trot] gpu: peak tilt {pt.max():.4f} rad, lowest base z {zmin.min():.4f} m, speed error {es.max():.3e} of the command, advanced "
          f"{(x[-1] - x[T.SETTLE - 1]).min():.3f} .. {(x[-1] - x[T.SETTLE - 1]).max():.3f} m;  cpu: {cpt.max():.4f} rad, {czmin.min():.4f} m, {ces.max():.3e}")
    assert abs(cpt.max() - CPU["tilt"]) < 1e-3 and abs(ces.max() - CPU["speed"]) < 1e-6, "the constants are the stored CPU run's figures"
    assert cpt.max() < 0.3 and ces.max() < 0.2, "the defaults are accepted on the CPU run"
    assert finite and ok, "finite state; every stance force inside its cone at every step"
    assert (z > 0.2).all(), f"base z {z.min():.4f}"
    assert pt.max() <= 2.0 * CPU["tilt"], (pt.max(), CPU["tilt"])
    assert es.max() <= 2.0 * CPU["speed"], (es.max(), CPU["speed"])


def test_standing_gait_with_zero_command_reproduces_the_stand_bound():
    """Gait.stand() and a zero command through the new path: over the last 50 of 200 steps the base is within the stand test's
    bound (BOUND of tests/test_gpu_foot_force_qp.py) of 0.30 m and of upright."""
    _need_gpu()
    x, z, tilt, ok, finite = _loop(B.STEPS, 0)
    ez, et = B.stand_errors(z, tilt)
    print(f"[stand via gait] worst |z - 0.30| {ez:.3e} m, tilt {et:.3e} rad over the last 50 steps; drift in x {np.abs(x[-1] - np.arange(B.N_ENVS)).max():.3e} m")
    assert finite and ok
    assert ez <= STAND_BOUND["z"] and et <= STAND_BOUND["tilt"]


# ------------------------------------------------------------------------------------------------------------ surface --
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


def test_legged_robot_walks_through_the_facade(monkeypatch):
    """apply_locomotion_control under SHIFU_AMD_FLOATING_DYNAMICS=1, 8 envs in effort mode: 100 ticks of Gait.stand() (the robots
    are created 0.42 m up and land), then 200 ticks of the default trot at 0.3 m/s -- they move forward, stay up and finite,
    efforts inside the limits, forces inside the cones, the tilt while trotting within the closed-loop test's allowance.  Unset,
    the calls are refused ("fixed base")."""
    _need_gpu()
    from shifu_amd.units.gait import Gait
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    n = 8
    env, robot = _legged_env(n)
    assert tuple(robot.nominal_foot_positions.shape) == (4, 3) and bool((robot.nominal_foot_positions[:, 2] < -0.2).all())
    env.reset()                              # the default dof positions: a freshly created actor stands on straight legs
    robot.reset_gait()
    env.gym.refresh_all_state_tensors(env.sim)
    root = env.root_state.view(n, -1, 13)[:, 0]
    mu = robot._contact_friction().view(n, 1, 1)
    zmin, tmax, ok = float("inf"), 0.0, True
    stand = Gait.stand()
    for s in range(300):
        if s == 100:
            x0 = root[:, 0].clone()
        command = torch.tensor([0.3 if s >= 100 else 0.0, 0.0, 0.0], device=robot.device)
        tau, f, stance, swing = robot.apply_locomotion_control(command, gait=stand if s < 100 else None)
        env.gym.refresh_actor_root_state_tensor(env.sim)
        on = stance.bool()
        ok = ok and bool((tau.abs() <= robot.torque_limits).all()) and bool((f[~on] == 0).all()) and bool((f[..., 2][on] >= 5.0).all())
        ok = ok and bool((f[..., :2].abs() <= mu * f[..., 2:3])[on].all())
        r = root.cpu().numpy()
        zmin = min(zmin, float(r[:, 2].min()))
        if s >= 100:
            tmax = max(tmax, float(B.tilt_of(r[:, 3:7]).max()))
    torch.cuda.synchronize()
    adv = (root[:, 0] - x0).cpu().numpy()
    print(f"[facade] advanced {adv.min():.3f} .. {adv.max():.3f} m in 200 ticks, lowest base z {zmin:.4f} m, peak tilt {tmax:.4f} rad")
    assert tuple(tau.shape) == (n, robot.num_dof) and tuple(f.shape) == (n, 4, 3) and tuple(stance.shape) == (n, 4) and tuple(swing.shape) == (n, 4, 3)
    assert stance.dtype == torch.uint8 and ok
    assert torch.isfinite(env.dof_state).all() and torch.isfinite(env.root_state).all()
    assert zmin > 0.2 and tmax <= 2.0 * CPU["tilt"]
    assert (adv > 0.5 * 0.3 * 200 * float(env.sim_params.dt)).all(), "every env moves forward"
    assert int(robot._gait_state().tick[0]) == 200
    robot.reset_gait(torch.tensor([2], device=robot.device))
    robot.locomotion_control(command)
    assert robot._gait_state().tick.tolist() == [201, 201, 1] + [201] * 5
    monkeypatch.delenv("SHIFU_AMD_FLOATING_DYNAMICS")
    robot._mass_matrix = robot._bias_forces = None
    with pytest.raises(Exception, match="fixed base"):
        robot.locomotion_control(command)
    with pytest.raises(Exception, match="fixed base"):
        robot.apply_locomotion_control(command)


def test_fused_env_locomotion_control_equals_the_backend_call():
    _need_gpu()
    from shifu_amd import glue
    from shifu_amd.gym.a1_fused import FusedA1Env
    from shifu_amd.units import gait as UG
    n = 8
    env = FusedA1Env(num_envs=n, terrain="flat")
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        for _ in range(5):
            env.step(0.2 * (2 * torch.rand(n, 12, device=env.device, generator=g) - 1))
        command = torch.tensor([[0.3, 0.1, -0.2]], device=env.device).repeat(n, 1)
        env.locomotion_control(command)                       # the resetting tick
        env.gait_state.tick.copy_(torch.arange(n, dtype=torch.int32, device=env.device) * 9)
        mine = _clone(env.gait_state)
        tau, f, stance, swing = env.locomotion_control(command)
        w = env.whole_body_dynamics()
        m, nb = env.cm.blob, env.cm.blob.nb
        fb = [b for b, name in enumerate(env.cm.body_names) if name.endswith("_foot")]
        limit = torch.tensor([m.effort[d] for d in range(12)], device=env.device)
        nominal = torch.tensor(UG.nominal_foot_positions(m, [float(env.task_params.default_dof_pos[d]) for d in range(12)], fb),
                               dtype=torch.float32, device=env.device)
        out = glue.locomotion_control(env.foot_jacobians, env.dof_state.view(n, 12, 2), env.root_state.view(n, 13),
                                      env.body_state.view(n, nb, 13)[:, 4::4, :3], env.contact_state.view(n, nb, 3)[:, 4::4, 2],
                                      env.sim.tensors[_abi.T_FRICTION], env.sim.terrain.friction, w["mass_matrix"], w["bias"], limit,
                                      UG.chain_mask(m, fb).to(env.device), nominal, mine, command, UG.Gait.trot(), float(env.sim_params.dt),
                                      0.30, UG.foot_radius(m, fb) - 0.01, 400., 10.)
        torch.cuda.synchronize()
        assert fb == [4, 8, 12, 16]
        assert tuple(tau.shape) == (n, 12) and tuple(f.shape) == (n, 4, 3) and tuple(stance.shape) == (n, 4) and tuple(swing.shape) == (n, 4, 3)
        for a, b in zip((tau, f, stance, swing), out):
            assert torch.equal(a, b)
        assert _same(mine, env.gait_state) and torch.isfinite(tau).all()
        assert len({tuple(r) for r in stance.tolist()}) > 1 or int(stance.sum()) > 0
        p0 = env.gait_state.anchor.data_ptr()
        env.locomotion_control(command)
        assert env.gait_state.anchor.data_ptr() == p0, "the gait state is allocated once"
    finally:
        env.destroy()
