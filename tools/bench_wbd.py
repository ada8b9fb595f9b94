"""Times the floating-base dynamics launch and the foot controller on A1 envs (a bare sim, effort mode, seeded states with every
velocity non-zero):

* shf_sim_floating_dynamics with all three outputs, with the Jacobian only and with M + h only, beside
  shf_sim_refresh(BODY), the refresh kernel it shares its layout with;
* shf_foot_impedance beside the torch expressions of the same controller (utils.torch_utils.foot_impedance_control).

    python tools/bench_wbd.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_wbd

ms per launch by device events: `repeats` interleaved blocks of `launches` launches per form, median [min .. max] over the
blocks (the convention of tools/bench_osc.py).  Beside them the bytes the full launch must store (Jacobian + M + h per env) and
the time those take at the measured HBM copy rate of the MI355X, 6.29 TB/s: a floor for the stores alone, not a target --
nobody has measured this kernel before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import _abi, glue  # noqa: E402
from shifu_amd.backend import Sim  # noqa: E402
from shifu_amd.model import asset_path, compile_urdf  # noqa: E402
from shifu_amd.utils.torch_utils import foot_impedance_control  # noqa: E402

HBM_BYTES_PER_S = 6.29e12        # float4 copy, measured


def a1_sim(n, group, seed=1):
    m = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT).blob
    p = _abi.ShfSimParams()
    p.dt = 0.005
    p.gravity[:] = (0.0, 0.0, -9.81)
    p.contact_k, p.contact_d, p.friction_vel, p.limit_k, p.limit_d = 5e4, 300.0, 0.002, 2000.0, 20.0
    p.max_ang_vel, p.max_depen_vel, p.contact_offset = 64.0, 1.0, 0.01
    sim = Sim(p, "cuda:0")
    sim.set_plane(1.0)
    sim.set_articulation(m)
    sim.finalize(n, 0, group=group)
    rng = np.random.default_rng(seed)
    lo = np.array([m.lower[d] for d in range(m.nd)]); hi = np.array([m.upper[d] for d in range(m.nd)])
    q = rng.uniform(lo, hi, (n, m.nd)); qd = rng.uniform(-2, 2, (n, m.nd))
    root = np.zeros((n, 13))
    root[:, :3] = rng.uniform(-1, 1, (n, 3)) + (0, 0, 3)
    quat = rng.normal(size=(n, 4))
    root[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    root[:, 7:10], root[:, 10:13] = rng.uniform(-1, 1, (n, 3)), rng.uniform(-2, 2, (n, 3))
    dof = torch.from_numpy(np.stack([q, qd], -1).reshape(n * m.nd, 2).astype(np.float32))
    root = torch.from_numpy(root.astype(np.float32))
    for tid, a in ((_abi.T_SIM_DOF, dof), (_abi.T_DOF_STATE, dof), (_abi.T_SIM_ROOT, root), (_abi.T_ROOT_STATE, root)):
        sim.tensors[tid].copy_(a)
    return sim, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--group", type=int, default=32)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.envs
    sim, m = a1_sim(n, a.group)
    nd, nb, D = m.nd, m.nb, m.nd + 6
    dev = sim.device
    jac = sim.tensors[_abi.T_JACOBIAN]
    M = torch.zeros(n, D, D, device=dev)
    h = torch.zeros(n, D, device=dev)
    sim.refresh(_abi.REFRESH_ALL)
    sim.floating_dynamics(jac, M, h)
    body = sim.tensors[_abi.T_BODY_STATE].view(n, nb, 13)
    rs = sim.tensors[_abi.T_ROOT_STATE].view(n, 13)
    dof = sim.tensors[_abi.T_DOF_STATE].view(n, nd, 2)
    jf, fp = jac[:, 4::4], body[:, 4::4, :3]                      # the feet: bodies 4, 8, 12, 16
    target = torch.zeros(n, 4, 3, device=dev)
    target[..., 2] = -0.3
    kp3 = torch.full((3,), 200.0, device=dev)
    kd3 = 2.0 * torch.sqrt(kp3)
    lim = torch.tensor([m.effort[d] for d in range(nd)], device=dev)

    forms = [("shf_sim_floating_dynamics (J + M + h)", lambda: sim.floating_dynamics(jac, M, h)),
             ("shf_sim_floating_dynamics (J only)", lambda: sim.floating_dynamics(jac, None, None)),
             ("shf_sim_floating_dynamics (M + h)", lambda: sim.floating_dynamics(None, M, h)),
             ("shf_sim_refresh(BODY)", lambda: sim.refresh(_abi.REFRESH_BODY)),
             ("shf_foot_impedance", lambda: glue.foot_impedance(jf, dof, rs, fp, target, kp3, kd3, h, lim)),
             ("torch expressions of the foot controller",
              lambda: foot_impedance_control(jf, dof[..., 1], rs[:, :3], rs[:, 3:7], fp, target, kp3, kd3, h, lim))]
    t_k, t_t = forms[4][1](), forms[5][1]()
    diff = float((t_k - t_t).abs().max() / t_t.abs().max())
    for _, f in forms:
        for _ in range(a.warmup):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(a.repeats):
        for name, f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.launches)
    stored = {"jacobian": nb * 6 * D * 4, "mass_matrix": D * D * 4, "bias": D * 4}
    per_env = sum(stored.values())
    floor_ms = n * per_env / HBM_BYTES_PER_S * 1e3
    res = {"envs": n, "group": a.group, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev),
           "foot_kernel_vs_torch_max_rel_diff": diff, "stored_bytes_per_env": stored, "stored_bytes_total": n * per_env,
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "store_floor_ms": floor_ms, "ms_per_launch": {}}
    lines = [f"| form | ms per launch, {n} envs, {a.group} lanes per env |", "|---|---|"]
    for name, _ in forms:
        t = sorted(times[name])
        res["ms_per_launch"][name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
        lines.append(f"| {name} | {t[len(t) // 2]:.4f} [{t[0]:.4f} .. {t[-1]:.4f}] |")
    full = res["ms_per_launch"][forms[0][0]]["median"]
    lines += ["", f"Stored by the full launch: {per_env} B per env (Jacobian {stored['jacobian']}, M {stored['mass_matrix']}, h {stored['bias']}), "
              f"{n * per_env / 1e6:.1f} MB for {n} envs: {floor_ms * 1e3:.1f} us at 6.29 TB/s (the measured HBM copy rate), "
              f"{floor_ms / full * 100:.0f} % of the launch's {full * 1e3:.1f} us.",
              f"Foot controller, kernel against its torch expressions: max relative difference {diff:.2e}.",
              f"{a.repeats} interleaved blocks of {a.launches} launches between device events, median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    assert torch.isfinite(M).all() and torch.isfinite(h).all() and torch.isfinite(jac).all() and torch.isfinite(t_k).all()
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Floating-base dynamics launch and foot controller (tools/bench_wbd.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
