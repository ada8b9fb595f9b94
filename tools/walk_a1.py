"""The A1 walks at a commanded velocity without a policy: LeggedRobot.apply_locomotion_control through the gym facade in effort
mode (gait plan, foot-force QP, swing spring-damper and the merge: csrc/shf_gait.hip, csrc/shf_qp.hip, csrc/shf_glue.hip).

    python tools/walk_a1.py --command 0.3 0 0 --gait trot --envs 8 --steps 600 [--settle 100] [--controller mpc] [--video DIR]

The robots are reset to their default pose, land during `--settle` ticks of Gait.stand() and then follow `--command vx vy wz`
(m/s, m/s, rad/s in the heading frame) under `--gait` for `--steps` ticks of the simulation step.  Prints one JSON line: the
mean velocity over the walk in the world frame, the yaw rate, the lowest base height and the largest tilt.  --controller mpc takes
the stance forces from the horizon MPC (csrc/shf_mpc.hip; --mpc-every ticks between two solves) instead of the QP.  --video DIR writes
the headless viewer's frames (frame_%06d.png, one per `--video-every` ticks) into DIR."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--command", type=float, nargs=3, default=[0.3, 0.0, 0.0], metavar=("VX", "VY", "WZ"))
    ap.add_argument("--gait", choices=["trot", "stand", "walk", "pace", "bound"], default="trot")
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--settle", type=int, default=100)
    ap.add_argument("--controller", choices=["qp", "mpc"], default="qp")
    ap.add_argument("--mpc-every", type=int, default=None)
    ap.add_argument("--video", default=None, metavar="DIR")
    ap.add_argument("--video-every", type=int, default=4)
    a = ap.parse_args()
    os.environ["SHIFU_AMD_FLOATING_DYNAMICS"] = "1"
    if a.video:
        os.environ["SHIFU_AMD_VIEWER"] = a.video
    import math

    import torch

    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.units import LeggedRobot
    from shifu_amd.units.gait import PRESETS, Gait

    class EnvCfg(BaseEnvConfig):
        num_envs = a.envs

        class control(BaseEnvConfig.control):
            decimation = 1

        class debug(BaseEnvConfig.debug):
            headless = a.video is None

    env = IsaacGymEnv(EnvCfg())
    robot = LeggedRobot(A1ActorConfig())
    env.create_envs(robot=robot)
    env.reset()
    robot.reset_gait()
    n = a.envs
    dt = float(env.sim_params.dt)
    root = env.root_state.view(n, -1, 13)[:, 0]
    stand, gait = Gait.stand(), PRESETS[a.gait]()
    zero = torch.zeros(3, device=robot.device)
    command = torch.tensor(a.command, dtype=torch.float32, device=robot.device)
    mpc_kw = {} if a.mpc_every is None else {"mpc_every": a.mpc_every}
    zmin, tilt = float("inf"), 0.0
    start = None
    for s in range(a.settle + a.steps):
        walking = s >= a.settle
        robot.apply_locomotion_control(command if walking else zero, gait=gait if walking else stand, controller=a.controller, **mpc_kw)
        env.gym.refresh_actor_root_state_tensor(env.sim)
        if s == a.settle - 1 or (a.settle == 0 and s == 0):
            start = root[:, :7].clone()
        if a.video and s % max(a.video_every, 1) == 0:
            env.render()
        q = root[:, 3:7]
        zmin = min(zmin, float(root[:, 2].min()))
        tilt = max(tilt, float(torch.acos((1.0 - 2.0 * (q[:, 0] ** 2 + q[:, 1] ** 2)).clamp(-1.0, 1.0)).max()))
    T = a.steps * dt
    yaw = lambda r: torch.atan2(2.0 * (r[:, 3] * r[:, 4] + r[:, 6] * r[:, 5]), 1.0 - 2.0 * (r[:, 4] ** 2 + r[:, 5] ** 2))
    dyaw = yaw(root) - yaw(start)
    dyaw = dyaw - 2.0 * math.pi * torch.round(dyaw / (2.0 * math.pi))
    vel = (root[:, :2] - start[:, :2]) / T
    print(json.dumps({"gait": a.gait, "controller": a.controller, "command": a.command, "envs": n, "steps": a.steps, "dt": dt,
                      "mean_world_velocity_m_s": [float(vel[:, 0].mean()), float(vel[:, 1].mean())],
                      "mean_yaw_rate_rad_s_mod_turns": float((dyaw / T).mean()), "lowest_base_z_m": zmin, "largest_tilt_rad": tilt,
                      "finite": bool(torch.isfinite(env.root_state).all() and torch.isfinite(env.dof_state).all())}))


if __name__ == "__main__":
    main()
