"""Times the torque-level control path on the push-box scene (arm + table + cube + pad, effort mode):

* shf_sim_dynamics (mass matrix + bias forces) beside shf_sim_refresh(BODY | JACOBIAN), the refresh kernel it is modelled on;
* shf_osc beside the torch expressions of the same controller (utils.torch_utils.operational_space_control: torch.linalg on
  the same tensors);
* the whole control step: refresh_all_state_tensors, refresh_mass_matrix_tensors, shf_osc, set_dof_actuation_force_tensor,
  simulate, refresh_dof_state_tensor.

    python tools/bench_osc.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_osc.json

ms per launch by device events: `repeats` interleaved blocks of `launches` launches per form, median [min .. max] over the
blocks (the convention of profiles/r17_raycast.md)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import _abi, glue  # noqa: E402
from shifu_amd.isaacgym import gymapi, gymtorch  # noqa: E402
from shifu_amd.model import asset_path  # noqa: E402
from shifu_amd.utils.torch_utils import operational_space_control  # noqa: E402

Q0 = np.array([0.3, 0.4, 0.3, 0.5, 0.8, 0.2])


def pushbox_scene(n):
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.dt = 0.005
    sp.gravity = gymapi.Vec3(0.0, 0.0, -9.81)
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, sp)
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link = True
    opts.default_dof_drive_mode = gymapi.DOF_MODE_EFFORT
    arm = gym.load_asset(sim, os.path.dirname(asset_path("abb_rod.urdf")), "abb_rod.urdf", opts)
    fixed = gymapi.AssetOptions()
    fixed.fix_base_link = True
    boxes = [(gym.create_box(sim, 0.6, 0.6, 0.1, fixed), (0.0, 0.0, 0.05)), (gym.create_box(sim, 0.05, 0.05, 0.05), (0.0, 0.0, 0.125)),
             (gym.create_box(sim, 0.08, 0.08, 0.002, fixed), (0.1, 0.1, 0.1))]
    for e in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        gym.create_actor(env, arm, gymapi.Transform(gymapi.Vec3(-0.48, 0.0, 0.0)), "arm", e, 0)
        for k, (b, p) in enumerate(boxes):
            gym.create_actor(env, b, gymapi.Transform(gymapi.Vec3(*p)), f"box{k}", e, 0)
    gym.prepare_sim(sim)
    return gym, sim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.envs
    gym, sim = pushbox_scene(n)
    be = sim.backend
    m = be.model
    nd, nb, A = m.nd, m.nb, sim.actors_per_env
    dev = be.device
    rng = np.random.default_rng(1)
    q0 = (Q0 + rng.uniform(-0.3, 0.3, (n, nd))).astype(np.float32)
    dof0 = torch.from_numpy(np.stack([q0, np.zeros_like(q0)], -1).reshape(n * nd, 2)).to(dev)
    root0 = be.tensors[_abi.T_SIM_ROOT].clone()

    def reset_state():
        be.tensors[_abi.T_SIM_DOF].copy_(dof0)
        be.tensors[_abi.T_SIM_ROOT].copy_(root0)
        gym.refresh_all_state_tensors(sim)

    M = gymtorch.wrap_tensor(gym.acquire_mass_matrix_tensor(sim, "arm"))
    h = gymtorch.wrap_tensor(gym.acquire_dof_bias_force_tensor(sim, "arm"))
    reset_state()
    gym.refresh_mass_matrix_tensors(sim)
    jac = be.tensors[_abi.T_JACOBIAN].view(n, nb - 1, 6, nd)
    body = be.tensors[_abi.T_BODY_STATE].view(n, nb + A - 1, 13)
    dof = be.tensors[_abi.T_DOF_STATE].view(n, nd, 2)
    j_ee, ee = jac[:, nb - 2], body[:, nb - 1, :7]
    goal = ee.clone()
    goal[:, :3] += torch.tensor([0.05, -0.03, 0.04], device=dev)
    kp6 = torch.full((6,), 150.0, device=dev)
    kd6 = 2.0 * torch.sqrt(kp6)
    lim = torch.tensor([m.effort[d] for d in range(nd)], device=dev)

    def f_dynamics():
        be.dynamics(M, h)

    def f_refresh():
        be.refresh(_abi.REFRESH_BODY | _abi.REFRESH_JACOBIAN)

    def f_osc():
        return glue.osc(j_ee, M, h, dof, ee, goal, kp6, kd6, 0.05, None, 0.0, 0.0, lim)

    def f_torch():
        return operational_space_control(j_ee, M, dof[..., 0], dof[..., 1], ee[:, :3], ee[:, 3:7], goal[:, :3], goal[:, 3:7], kp6, kd6,
                                         0.05, h, None, 0.0, 0.0, lim)

    def f_step():
        gym.refresh_all_state_tensors(sim)
        gym.refresh_mass_matrix_tensors(sim)
        tau = glue.osc(j_ee, M, h, dof, ee, goal, kp6, kd6, 0.05, None, 0.0, 0.0, lim)
        gym.set_dof_actuation_force_tensor(sim, gymtorch.unwrap_tensor(tau))
        gym.simulate(sim)
        gym.refresh_dof_state_tensor(sim)

    def f_simulate():
        gym.simulate(sim)

    forms = [("shf_sim_dynamics (M + h)", f_dynamics), ("shf_sim_refresh(BODY | JACOBIAN)", f_refresh), ("shf_osc", f_osc),
             ("torch expressions (torch.linalg)", f_torch), ("whole control step", f_step), ("gym.simulate alone", f_simulate)]
    diff = float((f_osc() - f_torch()).abs().max() / f_torch().abs().max())
    for _, f in forms:
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.repeats):
        for name, f in forms:
            reset_state()
            gym.refresh_mass_matrix_tensors(sim)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    res = {"envs": n, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev),
           "osc_vs_torch_max_rel_diff": diff, "ms_per_launch": {}}
    print(f"| form | ms per launch, {n} envs |\n|---|---|")
    for name, _ in forms:
        t = sorted(times[name])
        res["ms_per_launch"][name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
        print(f"| {name} | {t[len(t) // 2]:.4f} [{t[0]:.4f} .. {t[-1]:.4f}] |")
    assert torch.isfinite(be.tensors[_abi.T_DOF_STATE]).all()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
