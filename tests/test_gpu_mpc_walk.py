"""The horizon MPC in the closed loop on the GPU: the scenario of tests/trot_cpu.py (8 A1s dropped 2 cm, 100 ticks of Gait.stand(),
500 ticks of Gait.trot() at 0.3 m/s) through glue.locomotion_control(controller="mpc") on a bare sim under the TGS solver, a
solve every tick, which is also the default interval (the CPU prototype fell with forces held for 2, 3 or 6 ticks).
tests/mpc_trot_cpu.py holds the CPU run (the oracle's float32 step with the float64 twins as controller); its figures are
mpc_trot_cpu.CPU_FIGURES.

Asserted on every env and step: the state stays finite, every force of a solve lies inside its cone, the base stays above 0.2 m;
and the bounds the QP trot is held to in tests/test_gpu_gait.py: peak tilt below 0.3 rad and speed error below 0.2 of the command
on the CPU run, and on the GPU figures no worse than twice the CPU run's plus their measured difference (figures are compared, not
trajectories: contact makes trajectories diverge).  GPU figures measured on an MI355X: GPU below.
"""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import balance_cpu as B
from tests import helpers as H
from tests import mpc_ref as R
from tests import mpc_trot_cpu as C
from tests import trot_cpu as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FEET = B.FEET
# (peak tilt rad, lowest base z m, speed error) of the GPU run per solve interval (MI355X)
GPU = {1: (0.0141, 0.2944, 1.072e-2)}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


def _loop(every, settle=T.SETTLE, trot=T.TROT, vx=T.VX):
    """tests/mpc_trot_cpu.run on the GPU: per tick refresh, J / M / h, glue.locomotion_control(controller="mpc"), one simulate()."""
    import copy
    from shifu_amd import glue
    from shifu_amd.backend import Sim
    from shifu_amd.units.gait import Gait, GaitState
    m = H.a1_model().blob
    q, qd, root, _ = B.initial_state(m)
    n = B.N_ENVS
    sim = Sim(B.params(), "cuda:0")
    sim.set_plane(1.0)
    sim.set_articulation(copy.deepcopy(m))
    sim.finalize(n, 0)
    dof0 = np.stack([q, qd], -1).reshape(n * m.nd, 2).astype(np.float32)
    for tid, a in ((_abi.T_SIM_DOF, dof0), (_abi.T_DOF_STATE, dof0), (_abi.T_SIM_ROOT, root), (_abi.T_ROOT_STATE, root)):
        sim.tensors[tid].copy_(torch.from_numpy(np.array(a, np.float32)))
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
            state.mpc_count = 0                      # the trot starts with a solve, as the CPU run's does
            state.mpc_u.zero_()
            command[:, 0] = vx
        tau, forces, stance, _ = glue.locomotion_control(jf, dof, rs, fp, cz, fric, 1.0, M, h, limit, chain, nominal, state, command,
                                                         trot_g if s >= settle else stand, T.DT, B.HEIGHT, T.foot_radius(m) - T.TOUCHDOWN_DEPTH,
                                                         T.SWING_KP, T.SWING_KD, mu=B.MU, controller="mpc", mpc_every=every)
        if (state.mpc_count - 1) % every == 0:       # a tick with a solve: its forces stand on this tick's stance
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


@pytest.mark.parametrize("every", sorted({1, R.EVERY}))
def test_the_a1_trots_under_the_mpc(every):
    _need_gpu()
    x, z, tilt, ok, finite = _loop(every)
    pt, zmin, es = T.figures(x, z, tilt)
    cpt, czmin, ces = C.CPU_FIGURES[every]
    print(f"[mpc trot] a solve every {every}: gpu: peak tilt {pt.max():.4f} rad, lowest base z {zmin.min():.4f} m, speed error "
          f"{es.max():.3e} of the command, advanced {(x[-1] - x[T.SETTLE - 1]).min():.3f} .. {(x[-1] - x[T.SETTLE - 1]).max():.3f} m;  "
          f"cpu: {cpt:.4f} rad, {czmin:.4f} m, {ces:.3e}")
    if every == R.EVERY:
        gold = np.load(C.GOLDEN)
        g = T.figures(gold["x"].astype(np.float64), gold["z"].astype(np.float64), gold["tilt"].astype(np.float64))
        assert abs(g[0].max() - cpt) < 1e-3 and abs(g[2].max() - ces) < 1e-4, "the constants are the stored CPU run's figures"
    assert cpt < C.BOUNDS["tilt"] and ces < C.BOUNDS["speed"] and czmin > C.BOUNDS["z_min"], "the defaults are accepted on the CPU run"
    assert finite and ok, "finite state; every solved force inside its cone"
    assert (z > C.BOUNDS["z_min"]).all(), f"base z {z.min():.4f}"
    assert pt.max() < C.BOUNDS["tilt"] and es.max() < C.BOUNDS["speed"]
    diff = (0.0, 0.0, 0.0) if GPU[every] is None else (abs(GPU[every][0] - cpt), 0.0, abs(GPU[every][2] - ces))
    assert pt.max() <= 2.0 * cpt + diff[0], (pt.max(), cpt)
    assert es.max() <= 2.0 * ces + diff[2], (es.max(), ces)


# ------------------------------------------------------------------------------------------------------------ surface --
def test_legged_robot_walks_under_the_mpc_through_the_facade(monkeypatch):
    """apply_locomotion_control(controller="mpc") under SHIFU_AMD_FLOATING_DYNAMICS=1, 8 envs in effort mode: 100 ticks of
    Gait.stand() (the robots are created 0.42 m up and land), then 200 ticks of the default trot at 0.3 m/s -- they move forward,
    stay up and finite, efforts inside the limits, forces inside the cones, the tilt within the bound of the closed loop; the
    default controller is still the QP."""
    _need_gpu()
    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.units import LeggedRobot
    from shifu_amd.units.gait import Gait
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    n = 8

    class EnvCfg(BaseEnvConfig):
        num_envs = n

        class control(BaseEnvConfig.control):
            decimation = 1

        class debug(BaseEnvConfig.debug):
            headless = True

    env = IsaacGymEnv(EnvCfg())
    robot = LeggedRobot(A1ActorConfig())
    env.create_envs(robot=robot)
    env.reset()
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
        tau, f, stance, swing = robot.apply_locomotion_control(command, gait=stand if s < 100 else None, controller="mpc")
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
    print(f"[mpc facade] advanced {adv.min():.3f} .. {adv.max():.3f} m in 200 ticks, lowest base z {zmin:.4f} m, peak tilt {tmax:.4f} rad")
    assert tuple(tau.shape) == (n, robot.num_dof) and tuple(f.shape) == (n, 4, 3) and stance.dtype == torch.uint8 and ok
    assert torch.isfinite(env.dof_state).all() and torch.isfinite(env.root_state).all()
    assert zmin > C.BOUNDS["z_min"] and tmax < C.BOUNDS["tilt"]
    assert (adv > 0.5 * 0.3 * 200 * float(env.sim_params.dt)).all(), "every env moves forward"
    st = robot._gait_state()
    assert st.mpc_count == 200 and tuple(st.mpc_u.shape) == (n, R.HORIZON, 4, 3)
    robot.reset_gait(torch.tensor([2], device=robot.device))
    assert st.mpc_count == 0 and float(st.mpc_u[2].abs().max()) == 0.0 and float(st.mpc_u[3].abs().max()) > 0.0
    with pytest.raises(ValueError, match="controller"):
        robot.locomotion_control(command, controller="lqr")


def test_fused_env_passes_the_controller_through():
    _need_gpu()
    from shifu_amd.gym.a1_fused import FusedA1Env
    n = 8
    env = FusedA1Env(num_envs=n, terrain="flat")
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        for _ in range(5):
            env.step(0.2 * (2 * torch.rand(n, 12, device=env.device, generator=g) - 1))
        command = torch.tensor([[0.3, 0.1, -0.2]], device=env.device).repeat(n, 1)
        tau, f, stance, swing = env.locomotion_control(command, controller="mpc", horizon=5)
        torch.cuda.synchronize()
        assert tuple(tau.shape) == (n, 12) and tuple(f.shape) == (n, 4, 3) and torch.isfinite(tau).all() and torch.isfinite(f).all()
        assert tuple(env.gait_state.mpc_u.shape) == (n, 5, 4, 3) and env.gait_state.mpc_count == 1
        assert torch.equal(env.gait_state.mpc_u[:, 0], f) and (f[~stance.bool()] == 0).all()
    finally:
        env.destroy()
