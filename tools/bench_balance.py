"""Times the balance controller's foot-force QP (csrc/shf_qp.hip: shf_foot_force_qp) on A1 envs near their stance (a bare sim,
seeded states, the wrench formed in the kernel from M and h), with every foot standing and with a trot's diagonal pair, beside
the torch fallback of the same algorithm (utils.torch_utils.balance_wrench + foot_force_qp) on the same tensors.

    python tools/bench_balance.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_balance

ms per launch by device events: `repeats` interleaved blocks of `launches` launches per form (`torch-launches` for the torch
forms, which take a few hundred launches of their own per call), median [min .. max] over the blocks (the convention of
tools/bench_wbd.py).  There is no target: nobody has measured this kernel before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
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
from shifu_amd.utils.torch_utils import balance_wrench, foot_force_qp  # noqa: E402


def a1_sim(n, seed=1):
    m = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT).blob
    p = _abi.ShfSimParams()
    p.dt = 0.005
    p.gravity[:] = (0.0, 0.0, -9.81)
    p.contact_k, p.contact_d, p.friction_vel, p.limit_k, p.limit_d = 5e4, 300.0, 0.002, 2000.0, 20.0
    p.max_ang_vel, p.max_depen_vel, p.contact_offset = 64.0, 1.0, 0.01
    sim = Sim(p, "cuda:0")
    sim.set_plane(1.0)
    sim.set_articulation(m)
    sim.finalize(n, 0)
    rng = np.random.default_rng(seed)
    q = np.array([0.0, 0.8, -1.5] * 4) + rng.uniform(-0.3, 0.3, (n, m.nd))
    qd = rng.uniform(-1, 1, (n, m.nd))
    root = np.zeros((n, 13))
    root[:, :2], root[:, 2] = rng.uniform(-2, 2, (n, 2)), rng.uniform(0.25, 0.35, n)
    ang, tilt = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 0.3, n)
    root[:, 3], root[:, 4], root[:, 6] = np.cos(ang) * np.sin(tilt / 2), np.sin(ang) * np.sin(tilt / 2), np.cos(tilt / 2)
    root[:, 7:10], root[:, 10:13] = rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-1, 1, (n, 3))
    dof = torch.from_numpy(np.stack([q, qd], -1).reshape(n * m.nd, 2).astype(np.float32))
    root = torch.from_numpy(root.astype(np.float32))
    for tid, a in ((_abi.T_SIM_DOF, dof), (_abi.T_DOF_STATE, dof), (_abi.T_SIM_ROOT, root), (_abi.T_ROOT_STATE, root)):
        sim.tensors[tid].copy_(a)
    return sim, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=glue.QP_ITERS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.envs
    sim, m = a1_sim(n)
    nd, nb, D = m.nd, m.nb, m.nd + 6
    dev = sim.device
    jac = sim.tensors[_abi.T_JACOBIAN]
    M = torch.zeros(n, D, D, device=dev)
    h = torch.zeros(n, D, device=dev)
    sim.refresh(_abi.REFRESH_ALL)
    sim.floating_dynamics(jac, M, h)
    body = sim.tensors[_abi.T_BODY_STATE].view(n, nb, 13)
    rs = sim.tensors[_abi.T_ROOT_STATE].view(n, 13)
    jf, fp = jac[:, 4::4], body[:, 4::4, :3]                      # the feet: bodies 4, 8, 12, 16
    target = rs.clone()
    target[:, 2] = 0.30
    target[:, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=dev)
    target[:, 7:] = 0.0
    kp, ka = torch.full((3,), 100.0, device=dev), torch.full((3,), 400.0, device=dev)
    gains = torch.cat([kp, 2.0 * torch.sqrt(kp), ka, 2.0 * torch.sqrt(ka)])
    S = torch.tensor([1.0, 1.0, 1.0, 10.0, 10.0, 10.0], device=dev)
    lim = torch.tensor([m.effort[d] for d in range(nd)], device=dev)
    mu = torch.full((n,), 0.8, device=dev)
    stances = {"all four feet": torch.ones(n, 4, dtype=torch.uint8, device=dev),
               "trot (a diagonal pair)": torch.tensor([1, 0, 0, 1], dtype=torch.uint8, device=dev).repeat(n, 1)}

    def kernel(st):
        return lambda: glue.foot_force_qp(jf, rs, fp, st, mu, S, None, M, h, target, gains, 1e-2, 0.0, None, 5.0, float("inf"), a.iters, h, lim)

    def fallback(st):
        return lambda: foot_force_qp(jf, rs[:, :3], fp, balance_wrench(M, h, rs, target, gains), st, mu, S, 1e-2, 0.0, None, 5.0,
                                     float("inf"), a.iters, h, lim)

    forms = [(f"shf_foot_force_qp, {k}", kernel(st), a.launches) for k, st in stances.items()] \
        + [(f"torch fallback, {k}", fallback(st), a.torch_launches) for k, st in stances.items()]
    diffs = {}
    for k, st in stances.items():
        (fk, tk), (ft, tt) = kernel(st)(), fallback(st)()
        ef = (fk - ft).abs().flatten(1).max(1).values / ft.abs().max()
        diffs[k] = {"forces": float(ef.max()), "forces_median": float(ef.median()), "envs_above_1e-4": int((ef > 1e-4).sum()),
                    "efforts": float((tk - tt).abs().max() / tt.abs().max())}
        assert torch.isfinite(fk).all() and torch.isfinite(tk).all()
        if diffs[k]["forces"] > 1e-3 or diffs[k]["efforts"] > 1e-3:
            raise SystemExit(f"{k}: kernel and torch fallback disagree ({diffs[k]}): a time ratio between them would mean nothing")
    for _, f, reps in forms:
        for _ in range(min(a.warmup, reps)):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in forms}
    for _ in range(a.repeats):
        for name, f, reps in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    res = {"envs": n, "iters": a.iters, "launches": a.launches, "torch_launches": a.torch_launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(dev), "kernel_vs_torch_max_rel_diff": diffs, "ms_per_launch": {}}
    lines = [f"| form | ms per call, {n} envs, {a.iters} sweeps |", "|---|---|"]
    for name, _, _ in forms:
        t = sorted(times[name])
        res["ms_per_launch"][name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
        lines.append(f"| {name} | {t[len(t) // 2]:.4f} [{t[0]:.4f} .. {t[-1]:.4f}] |")
    for k in stances:
        r = res["ms_per_launch"][f"torch fallback, {k}"]["median"] / res["ms_per_launch"][f"shf_foot_force_qp, {k}"]["median"]
        lines.append("")
        lines.append(f"{k}: the torch fallback takes {r:.0f} x the kernel's time; kernel against fallback, max relative difference: "
                     f"forces {diffs[k]['forces']:.2e} (median over envs {diffs[k]['forces_median']:.2e}, {diffs[k]['envs_above_1e-4']} envs above 1e-4), "
                     f"efforts {diffs[k]['efforts']:.2e}.")
    lines += ["", f"{a.repeats} interleaved blocks of {a.launches} launches ({a.torch_launches} for the torch forms) between device events, "
              f"median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Foot-force QP of the balance controller (tools/bench_balance.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
