"""Times the horizon MPC (csrc/shf_mpc.hip: shf_mpc_horizon, shf_foot_force_mpc, shf_foot_force_efforts) and one whole control
tick of LeggedRobot.locomotion_control(controller="mpc") with a solve every tick and every 6 ticks, beside the existing QP tick
and the torch fallbacks of the same algorithms (utils.torch_utils) on the same tensors: A1 envs near their stance (a bare sim,
seeded states, per-env gait phases, commands and contact forces, as tools/bench_gait.py).

    python tools/bench_mpc.py --envs 4096 --launches 100 --warmup 10 --repeats 5 --out profiles/rNN_mpc

ms per call by device events: `repeats` interleaved blocks of `launches` calls per form (`torch-launches` for the torch forms),
median [min .. max] over the blocks.  The script stops rather than report a ratio if a kernel and its fallback disagree.  There is
no target: nobody has measured these kernels before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import _abi, glue  # noqa: E402
from shifu_amd.units import gait as UG  # noqa: E402
from shifu_amd.utils import torch_utils as TU  # noqa: E402
from tools.bench_balance import a1_sim  # noqa: E402
from tools.bench_gait import clone_state  # noqa: E402

DT, HEIGHT = 0.005, 0.30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--horizon", type=int, default=glue.MPC_HORIZON)
    ap.add_argument("--iters", type=int, default=glue.MPC_ITERS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, H = a.envs, a.horizon
    sim, m = a1_sim(n)
    nd, nb, D = m.nd, m.nb, m.nd + 6
    dev = sim.device
    jac = sim.tensors[_abi.T_JACOBIAN]
    M, h = torch.zeros(n, D, D, device=dev), torch.zeros(n, D, device=dev)
    sim.refresh(_abi.REFRESH_ALL)
    sim.floating_dynamics(jac, M, h)
    body = sim.tensors[_abi.T_BODY_STATE].view(n, nb, 13)
    rs = sim.tensors[_abi.T_ROOT_STATE].view(n, 13)
    dof = sim.tensors[_abi.T_DOF_STATE].view(n, nd, 2)
    feet = [4, 8, 12, 16]
    jf, fp = jac[:, 4::4], body[:, 4::4, :3]
    g = torch.Generator(device=dev).manual_seed(7)
    rnd = lambda *s: torch.rand(*s, device=dev, generator=g)
    cz = torch.where(rnd(n, 4) < 0.25, rnd(n, 4), 1.0 + 39.0 * rnd(n, 4))
    command = torch.stack([rnd(n) - 0.5, rnd(n) - 0.5, 2.0 * rnd(n) - 1.0], 1)
    gait = UG.Gait.trot()
    ticks = gait.ticks(DT)
    S = -(-ticks[0] // H)
    q0 = [0.0, 0.8, -1.5] * 4
    nominal = torch.tensor(UG.nominal_foot_positions(m, q0, feet), dtype=torch.float32, device=dev)
    tz = UG.foot_radius(m, feet) - 0.01
    chain = UG.chain_mask(m, feet).to(dev)
    lim = torch.tensor([m.effort[d] for d in range(nd)], device=dev)
    fric = torch.full((n,), 0.8, device=dev)
    mu = 0.5 * (fric + 1.0)
    par = glue.gait_params(DT, HEIGHT, tz, gait)
    state = UG.GaitState(n, 4, dev)
    glue.gait_plan(state, rs, fp, cz, command, nominal, state.take_pending(), ticks, par)          # the resetting tick
    state.tick.copy_(torch.randint(0, ticks[0], (n,), device=dev, generator=g).to(torch.int32))    # per-env phases
    stance, _, _ = glue.gait_plan(state, rs, fp, cz, command, nominal, None, ticks, par)
    L = torch.tensor(glue.MPC_WEIGHTS, device=dev)
    delta = glue.mpc_step_dt(S, DT)
    fz_max = float("inf")

    # agreement first
    tab_k = glue.mpc_horizon(state, stance, fp, command, nominal, ticks, par, H, S)
    tab_t = TU.mpc_horizon(state, stance, fp, command, nominal, ticks, DT, tz, gait.max_step, H, S)
    fk, ek = glue.foot_force_mpc(*tab_k, rs, M, h, jf, mu, L, glue.MPC_ALPHA, 5.0, fz_max, a.iters, delta, h, lim)
    ft, et = TU.foot_force_mpc(*tab_k, rs, M, h, jf, mu, L, glue.MPC_ALPHA, 5.0, fz_max, a.iters, delta, h, lim)
    ee = glue.foot_force_efforts(fk, tab_k[0][:, 0].contiguous(), jf, h, lim)
    diffs = {"contact_mismatches": int((tab_k[0] != tab_t[0]).sum()),
             "xref": float((tab_k[1] - tab_t[1]).abs().max()), "pos": float((tab_k[2] - tab_t[2]).abs().max()),
             "forces": float((fk - ft).abs().max() / ft.abs().max()), "efforts": float((ek - et).abs().max() / et.abs().max()),
             "efforts_kernel_bits_differing": int((ee.view(torch.int32) != ek.view(torch.int32)).sum())}
    torch.cuda.synchronize()
    if diffs["contact_mismatches"] or diffs["efforts_kernel_bits_differing"] or max(diffs["xref"], diffs["pos"]) > 1e-4 \
            or max(diffs["forces"], diffs["efforts"]) > 4.0 * 3.1e-3:          # four times the float32 twin's distance (tests/mpc_ref.F32_DIST)
        raise SystemExit(f"kernel and torch fallback disagree ({diffs}): a time ratio between them would mean nothing")

    def tick(st, controller, every):
        sim.floating_dynamics(jac, M, h)
        return glue.locomotion_control(jf, dof, rs, fp, cz, fric, 1.0, M, h, lim, chain, nominal, st, command, gait, DT, HEIGHT, tz,
                                       controller=controller, horizon=H, mpc_every=every, mpc_iters=a.iters)

    s_qp, s_1, s_6 = clone_state(state), clone_state(state), clone_state(state)
    st8 = tab_k[0][:, 0].contiguous()
    forms = [("shf_mpc_horizon", lambda: glue.mpc_horizon(state, stance, fp, command, nominal, ticks, par, H, S), a.launches),
             ("torch fallback, horizon", lambda: TU.mpc_horizon(state, stance, fp, command, nominal, ticks, DT, tz, gait.max_step, H, S), a.launches),
             ("shf_foot_force_mpc", lambda: glue.foot_force_mpc(*tab_k, rs, M, h, jf, mu, L, glue.MPC_ALPHA, 5.0, fz_max, a.iters, delta, h, lim), a.launches),
             ("torch fallback, solve", lambda: TU.foot_force_mpc(*tab_k, rs, M, h, jf, mu, L, glue.MPC_ALPHA, 5.0, fz_max, a.iters, delta, h, lim), a.torch_launches),
             ("shf_foot_force_efforts", lambda: glue.foot_force_efforts(fk, st8, jf, h, lim), a.launches),
             ("torch fallback, efforts", lambda: TU.foot_force_efforts(fk, st8, jf, h, lim), a.launches),
             ("control tick, QP: dynamics + 4 launches", lambda: tick(s_qp, "qp", 1), a.launches),
             ("control tick, MPC every tick: dynamics + 5 launches", lambda: tick(s_1, "mpc", 1), a.launches),
             ("control tick, MPC every 6 ticks (mean over the 6)", lambda: tick(s_6, "mpc", 6), 6 * max(a.launches // 6, 1))]
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
    res = {"envs": n, "horizon": H, "ticks_per_step": S, "iters": a.iters, "launches": a.launches, "torch_launches": a.torch_launches,
           "repeats": a.repeats, "device": torch.cuda.get_device_name(dev), "kernel_vs_torch": diffs, "ms_per_call": {}}
    lines = [f"| form | ms per call, {n} envs |", "|---|---|"]
    for name, _, _ in forms:
        t = sorted(times[name])
        res["ms_per_call"][name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
        lines.append(f"| {name} | {t[len(t) // 2]:.4f} [{t[0]:.4f} .. {t[-1]:.4f}] |")
    med = lambda k: res["ms_per_call"][k]["median"]
    lines += ["", f"The torch fallbacks take {med('torch fallback, horizon') / med('shf_mpc_horizon'):.0f} x (horizon), "
              f"{med('torch fallback, solve') / med('shf_foot_force_mpc'):.0f} x (solve) and "
              f"{med('torch fallback, efforts') / med('shf_foot_force_efforts'):.1f} x (efforts) the kernels' time.",
              f"Horizon {H} steps of {S} ticks, {a.iters} sweeps, {3 * 4 * H} variables per env.  Kernel against fallback on the same inputs: {diffs}.",
              "", f"{a.repeats} interleaved blocks of {a.launches} calls ({a.torch_launches} for the torch solve) between device events, "
              f"median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Horizon MPC: tables, solve, efforts and one locomotion control tick (tools/bench_mpc.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
