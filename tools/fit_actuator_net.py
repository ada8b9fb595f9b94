"""Fits an actuator net to a recorded actuator: the A1Conditional hook env steps under random actions through a DC-motor
actuator with a command delay of two sub-steps (units.actuators.Actuator.dc_motor); every sub-step gives, per joint, the
position error of the un-delayed command and the joint velocity at lags 0, 1, 2, and the torque the actuator produced.  A
6-32-32-32-1 softsign MLP (legged_gym's actuator-net shape) is fitted to (error taps, velocity taps) -> torque in torch and
saved in the .npz form Actuator.network reads; the held-out RMSE is printed in N m.

    python tools/fit_actuator_net.py --envs 64 --steps 200 --epochs 30 --out actuator_net.npz

The net has to learn the delay, the PD law and the torque-speed clip from three taps; what is left is the RMSE."""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd.units import Actuator, ActuatorNet  # noqa: E402
from tools.bench_actuator import LIM, SAT, VLIM, actuated_step, hook_env  # noqa: E402,F401

TAPS, VEL_SCALE, OUT_SCALE = (0, 1, 2), 0.1, 20.0


def record(envs, steps, seed):
    env = hook_env(envs, seed)
    robot = env.robot
    act = Actuator.dc_motor(robot.p_gains, robot.d_gains, SAT, VLIM, effort_limit=robot.torque_limits, delay=2)
    robot.set_actuator(act)
    robot.step = types.MethodType(actuated_step, robot)
    rows = []
    inner = act.efforts

    def efforts(targets, dof_state):
        fresh = act.pending.bool().clone() if act.any_pending else torch.zeros(envs, dtype=torch.bool, device=targets.device)
        tau = inner(targets, dof_state)
        ds = dof_state.view(envs, -1, 2)
        rows.append(((targets - ds[..., 0]).clone(), ds[..., 1].clone(), tau.clone(), fresh))
        return tau

    act.efforts = efforts
    g = torch.Generator(device=robot.device).manual_seed(seed)
    for _ in range(steps):
        env.step(2 * torch.rand(envs, 12, device=robot.device, generator=g) - 1)
    err, vel, tau, fresh = (torch.stack(x) for x in zip(*rows))           # (ticks, n, nd) and (ticks, n)
    K = max(TAPS)
    ok = torch.ones_like(fresh[K:])
    for k in range(K + 1):                                                 # no reset inside a sample's history window
        ok &= ~fresh[K - k:fresh.shape[0] - k]
    x = torch.cat([torch.stack([err[K - k:err.shape[0] - k] for k in TAPS], -1),
                   VEL_SCALE * torch.stack([vel[K - k:vel.shape[0] - k] for k in TAPS], -1)], -1)
    keep = ok.unsqueeze(-1).expand(tau[K:].shape)
    return x[keep], tau[K:][keep] / OUT_SCALE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="actuator_net.npz")
    a = ap.parse_args()
    x, y = record(a.envs, a.steps, a.seed)
    g = torch.Generator(device=x.device).manual_seed(a.seed)
    perm = torch.randperm(x.shape[0], device=x.device, generator=g)
    held = perm[:x.shape[0] // 10]
    train = perm[x.shape[0] // 10:]
    nn = torch.nn
    torch.manual_seed(a.seed)
    net = nn.Sequential(nn.Linear(6, 32), nn.Softsign(), nn.Linear(32, 32), nn.Softsign(), nn.Linear(32, 32), nn.Softsign(), nn.Linear(32, 1)).to(x.device)
    opt = torch.optim.Adam(net.parameters(), lr=2e-3)
    for _ in range(a.epochs):
        order = train[torch.randperm(train.numel(), device=x.device, generator=g)]
        for i in range(0, order.numel(), 4096):
            b = order[i:i + 4096]
            loss = torch.mean((net(x[b]).squeeze(-1) - y[b]) ** 2)
            opt.zero_grad()
            loss.backward()
            opt.step()
    with torch.no_grad():
        rmse = OUT_SCALE * float(torch.sqrt(torch.mean((net(x[held]).squeeze(-1) - y[held]) ** 2)))
        spread = OUT_SCALE * float(y[held].std())
    ActuatorNet.from_module(net.cpu()).save_npz(a.out)
    print(json.dumps({"samples": int(x.shape[0]), "held_out": int(held.numel()), "epochs": a.epochs, "held_out_rmse_nm": rmse,
                      "torque_std_nm": spread, "taps": TAPS, "vel_scale": VEL_SCALE, "out_scale": OUT_SCALE, "out": a.out}))
    print(f"held-out RMSE {rmse:.3f} N m (torque std {spread:.2f} N m); load with Actuator.network({a.out!r}, taps={TAPS}, "
          f"vel_scale={VEL_SCALE}, out_scale={OUT_SCALE})")


if __name__ == "__main__":
    main()
