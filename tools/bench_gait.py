"""Times the gait planner (csrc/shf_gait.hip: shf_gait_plan), the stance / swing effort merge (shf_leg_effort_mix) and one whole
control tick of LeggedRobot.locomotion_control (floating-base dynamics + the four launches of glue.locomotion_control) on A1
envs near their stance (a bare sim, seeded states, per-env gait phases, commands and contact forces), beside the torch fallbacks
of the same algorithms (utils.torch_utils) on the same tensors.

    python tools/bench_gait.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_gait

ms per call by device events: `repeats` interleaved blocks of `launches` calls per form (`torch-launches` for the whole tick's
torch form, whose QP takes a few hundred launches of its own), median [min .. max] over the blocks (the convention of
tools/bench_balance.py).  The script stops rather than report a ratio if a kernel and its fallback disagree.  There is no
target: nobody has measured these kernels before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import _abi, glue  # noqa: E402
from shifu_amd.units import gait as UG  # noqa: E402
from shifu_amd.utils import torch_utils as TU  # noqa: E402
from tools.bench_balance import a1_sim  # noqa: E402

DT, HEIGHT = 0.005, 0.30


def clone_state(st):
    c = UG.GaitState(st.n, st.F, st.tick.device)
    for a, b in zip(c.tensors(), st.tensors()):
        a.copy_(b)
    c.take_pending()
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--torch-launches", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = a.envs
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
    q0 = [0.0, 0.8, -1.5] * 4
    nominal = torch.tensor(UG.nominal_foot_positions(m, q0, feet), dtype=torch.float32, device=dev)
    tz = UG.foot_radius(m, feet) - 0.01
    chain = UG.chain_mask(m, feet).to(dev)
    lim = torch.tensor([m.effort[d] for d in range(nd)], device=dev)
    fric = torch.full((n,), 0.8, device=dev)
    par = glue.gait_params(DT, HEIGHT, tz, gait)
    state = UG.GaitState(n, 4, dev)
    glue.gait_plan(state, rs, fp, cz, command, nominal, state.take_pending(), ticks, par)          # the resetting tick
    state.tick.copy_(torch.randint(0, ticks[0], (n,), device=dev, generator=g).to(torch.int32))    # per-env phases
    plan_args = (DT, HEIGHT, gait.apex, tz, gait.late_depth, gait.k_fb, gait.max_step, gait.leash, gait.contact_threshold)

    def tick_fallback(st):
        sim.floating_dynamics(jac, M, h)
        stance, swing, _, _ = TU.gait_plan(st, rs, fp, cz, command, nominal, None, ticks, *plan_args)
        kp, ka = torch.full((3,), 100.0, device=dev), torch.full((3,), 400.0, device=dev)
        gains = torch.cat([kp, 2.0 * torch.sqrt(kp), ka, 2.0 * torch.sqrt(ka)])
        S = torch.tensor([1.0, 1.0, 1.0, 10.0, 10.0, 10.0], device=dev)
        forces, t_st = TU.foot_force_qp(jf, rs[:, :3], fp, TU.balance_wrench(M, h, rs, st.target, gains), stance, 0.5 * (fric + 1.0), S,
                                        1e-2, 0.0, None, 5.0, float("inf"), glue.QP_ITERS, h, lim)
        t_sw = TU.foot_impedance_control(jf, dof[..., 1], rs[:, :3], rs[:, 3:7], fp, swing, torch.full((3,), 400.0, device=dev),
                                         torch.full((3,), 10.0, device=dev), None, lim)
        return TU.leg_effort_mix(t_st, t_sw, stance, chain, lim), forces, stance, swing

    def tick_kernel(st):
        sim.floating_dynamics(jac, M, h)
        return glue.locomotion_control(jf, dof, rs, fp, cz, fric, 1.0, M, h, lim, chain, nominal, st, command, gait, DT, HEIGHT, tz)

    # agreement first: the same tick from the same state by both routes
    sa, sb = clone_state(state), clone_state(state)
    ka_, kb_ = glue.gait_plan(sa, rs, fp, cz, command, nominal, None, ticks, par), TU.gait_plan(sb, rs, fp, cz, command, nominal, None, ticks, *plan_args)
    diffs = {"plan_stance_mismatches": int((ka_[0] != kb_[0]).sum()) + int((sa.sched != sb.sched).sum()) + int((sa.tick != sb.tick).sum()),
             "plan_swing_target": float((ka_[1] - kb_[1]).abs().max() / kb_[1].abs().max()),
             "plan_base_target": float((sa.target - sb.target).abs().max() / sb.target.abs().max().clamp(min=1.0))}
    t_st, t_sw = torch.randn(n, nd, device=dev, generator=g) * 20, torch.randn(n, nd, device=dev, generator=g) * 20
    diffs["mix_bits_differing"] = int((glue.leg_effort_mix(t_st, t_sw, ka_[0], chain, lim).view(torch.int32)
                                       != TU.leg_effort_mix(t_st, t_sw, ka_[0], chain, lim).view(torch.int32)).sum())
    sa, sb = clone_state(state), clone_state(state)
    ek, ef = tick_kernel(sa), tick_fallback(sb)
    diffs["tick_efforts"] = float((ek[0] - ef[0]).abs().max() / ef[0].abs().max())
    diffs["tick_forces"] = float((ek[1] - ef[1]).abs().max() / ef[1].abs().max())
    torch.cuda.synchronize()
    if diffs["plan_stance_mismatches"] or diffs["mix_bits_differing"] or max(diffs["plan_swing_target"], diffs["plan_base_target"]) > 1e-4 \
            or max(diffs["tick_efforts"], diffs["tick_forces"]) > 1e-3:
        raise SystemExit(f"kernel and torch fallback disagree ({diffs}): a time ratio between them would mean nothing")
    sk, sf = clone_state(state), clone_state(state)
    forms = [("shf_gait_plan", lambda: glue.gait_plan(sk, rs, fp, cz, command, nominal, None, ticks, par), a.launches),
             ("torch fallback, gait plan", lambda: TU.gait_plan(sf, rs, fp, cz, command, nominal, None, ticks, *plan_args), a.launches),
             ("shf_leg_effort_mix", lambda: glue.leg_effort_mix(t_st, t_sw, ka_[0], chain, lim), a.launches),
             ("torch fallback, effort mix", lambda: TU.leg_effort_mix(t_st, t_sw, ka_[0], chain, lim), a.launches),
             ("control tick: dynamics + 4 launches", lambda: tick_kernel(sk), a.launches),
             ("control tick: dynamics + torch fallbacks", lambda: tick_fallback(sf), a.torch_launches)]
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
    res = {"envs": n, "launches": a.launches, "torch_launches": a.torch_launches, "repeats": a.repeats,
           "device": torch.cuda.get_device_name(dev), "kernel_vs_torch": diffs, "ms_per_call": {}}
    lines = [f"| form | ms per call, {n} envs |", "|---|---|"]
    for name, _, _ in forms:
        t = sorted(times[name])
        res["ms_per_call"][name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
        lines.append(f"| {name} | {t[len(t) // 2]:.4f} [{t[0]:.4f} .. {t[-1]:.4f}] |")
    med = lambda k: res["ms_per_call"][k]["median"]
    lines += ["", f"The torch fallbacks take {med('torch fallback, gait plan') / med('shf_gait_plan'):.0f} x (gait plan), "
              f"{med('torch fallback, effort mix') / med('shf_leg_effort_mix'):.1f} x (effort mix) and "
              f"{med('control tick: dynamics + torch fallbacks') / med('control tick: dynamics + 4 launches'):.0f} x (whole tick) the kernels' time.",
              f"Kernel against fallback on the same tick: {diffs}.",
              "", f"{a.repeats} interleaved blocks of {a.launches} calls ({a.torch_launches} for the whole tick's torch form) between device "
              f"events, median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Gait planner, effort merge and one locomotion control tick (tools/bench_gait.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
