"""Times the actuator models (csrc/shf_actuator.hip: shf_actuator_step) beside their torch fallback (utils.torch_utils.
actuator_step) on the same tensors -- PD, the DC motor behind a two-sub-step delay, and the 6-32-32-32-1 softsign network --
with shf_leg_effort_mix as the yardstick of a launch of this size; then one A1Conditional hook-env step three ways: the
example's own torch PD loop, Robot.apply_actuator_targets with a PD actuator (delay 0), and with the network actuator.

    python tools/bench_actuator.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_actuator

ms per call by device events: `repeats` interleaved blocks of `launches` calls per form, median [min .. max] over the blocks
(the protocol of tools/bench_gait.py).  The script stops rather than report a ratio if a kernel and its fallback disagree.
There is no target: nobody has measured these kernels before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import glue  # noqa: E402
from shifu_amd.units import Actuator, ActuatorNet  # noqa: E402
from shifu_amd.utils import torch_utils as TU  # noqa: E402

SAT, VLIM, LIM = 33.5, 21.0, 33.5


def seeded_net(widths=(6, 32, 32, 32, 1), seed=3):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for i, o in zip(widths[:-1], widths[1:]):
        k = 1.0 / i ** 0.5
        layers.append(((2 * torch.rand(o, i, generator=g) - 1) * k, (2 * torch.rand(o, generator=g) - 1) * k))
    return ActuatorNet(layers, "softsign")


def timed(forms, launches, warmup, repeats):
    for _, f in forms:
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in forms}
    for _ in range(repeats):
        for name, f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / launches)
    out = {}
    for name, _ in forms:
        t = sorted(times[name])
        out[name] = {"median": t[len(t) // 2], "min": t[0], "max": t[-1], "blocks": times[name]}
    return out


def hook_env(n, seed):
    from examples.a1_conditional.a1_conditional import A1Conditional
    from examples.a1_conditional.task_config import A1EnvConfig
    cfg = A1EnvConfig()
    cfg.num_envs = n
    np.random.seed(42)
    torch.manual_seed(seed)
    env = A1Conditional(cfg)
    env.reset()
    return env


def actuated_step(self, actions):
    """A1Robot.step through the robot's actuator."""
    self.torques = self.apply_actuator_targets(actions + self.default_dof_pos)
    self.post_step()
    self.apply_force_on_base(self.rand_force_buf.view(-1, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, nd, dev = a.envs, 12, "cuda:0"
    g = torch.Generator(device=dev).manual_seed(7)
    q0 = torch.tensor([0.0, 0.8, -1.5] * 4, device=dev)
    dof = torch.stack([q0 + 0.3 * torch.randn(n, nd, device=dev, generator=g), 8.0 * torch.randn(n, nd, device=dev, generator=g)], -1).contiguous()
    target = (q0 + 0.3 * torch.randn(n, nd, device=dev, generator=g)).contiguous()
    kp, kd = torch.full((nd,), 40.0, device=dev), torch.full((nd,), 1.0, device=dev)
    lim = torch.full((nd,), LIM, device=dev)
    sat, vlim = torch.full((nd,), SAT, device=dev), torch.full((nd,), VLIM, device=dev)
    net = seeded_net().bind(dev, (0, 1, 2), 1.0, 0.1, 20.0)
    z = lambda *s: torch.zeros(*s, device=dev)
    modes = {"PD": dict(kp=kp, kd=kd, effort_limit=lim, delay=0, L=1),
             "DC motor, delay 2": dict(kp=kp, kd=kd, effort_limit=lim, saturation=sat, velocity_limit=vlim, delay=2, L=3),
             "net 6-32-32-32-1 softsign": dict(net=net, effort_limit=lim, delay=0, L=1)}
    forms, diffs = [], {}
    for name, kw in modes.items():
        kw = dict(kw)
        L = kw.pop("L")
        states = []
        for f in (glue.actuator_step, TU.actuator_step):
            st = dict(cmd_hist=z(n, L, nd), efforts_out=z(n, nd), applied_out=z(n, nd))
            if "net" in kw:
                st.update(err_hist=z(n, 3, nd), vel_hist=z(n, 3, nd))
            f(target, dof, reset=torch.ones(n, dtype=torch.uint8, device=dev), **st, **kw)
            for _ in range(3):                                    # agreement first: the same calls from the same state by both routes
                f(target, dof, **st, **kw)
            states.append(st)
        torch.cuda.synchronize()
        ka, kb = states
        diffs[name] = {"state_bits_differing": int(sum((ka[k].view(torch.int32) != kb[k].view(torch.int32)).sum() for k in ka if k != "efforts_out")),
                       "efforts": float((ka["efforts_out"] - kb["efforts_out"]).abs().max())}
        if diffs[name]["state_bits_differing"] or diffs[name]["efforts"] > (1e-4 if "net" in kw else 0.0):
            raise SystemExit(f"kernel and torch fallback disagree ({name}: {diffs[name]}): a time ratio between them would mean nothing")
        forms.append((f"shf_actuator_step, {name}", lambda ka=ka, kw=kw: glue.actuator_step(target, dof, **ka, **kw)))
        forms.append((f"torch fallback, {name}", lambda kb=kb, kw=kw: TU.actuator_step(target, dof, **kb, **kw)))
    stance = (torch.rand(n, 4, device=dev, generator=g) < 0.5).to(torch.uint8)
    chain = torch.zeros(4, nd, dtype=torch.uint8, device=dev)
    for f in range(4):
        chain[f, 3 * f:3 * f + 3] = 1
    forms.append(("shf_leg_effort_mix (yardstick)", lambda: glue.leg_effort_mix(target, target, stance, chain, lim)))
    res = {"envs": n, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev), "kernel_vs_torch": diffs,
           "ms_per_call": timed(forms, a.launches, a.warmup, a.repeats)}

    # one hook-env step three ways
    envs = {"A1Conditional step, the example's torch PD loop": hook_env(n, 0)}
    for name, make in (("A1Conditional step, apply_actuator_targets (PD, delay 0)",
                        lambda r: Actuator.pd(r.p_gains, r.d_gains, effort_limit=r.torque_limits)),
                       ("A1Conditional step, apply_actuator_targets (net 6-32-32-32-1, DC clip, delay 2)",
                        lambda r: Actuator.network(seeded_net(), vel_scale=0.1, out_scale=20.0, saturation_effort=SAT, velocity_limit=VLIM,
                                                   effort_limit=r.torque_limits, delay=2))):
        env = hook_env(n, 0)
        env.robot.set_actuator(make(env.robot))
        env.robot.step = types.MethodType(actuated_step, env.robot)
        envs[name] = env
    ga = torch.Generator(device=dev).manual_seed(1)
    actions = [2 * torch.rand(n, 12, device=dev, generator=ga) - 1 for _ in range(16)]
    count = {k: 0 for k in envs}

    def stepper(name, env):
        def f():
            env.step(actions[count[name] % len(actions)])
            count[name] += 1
        return f

    res["ms_per_env_step"] = timed([(k, stepper(k, e)) for k, e in envs.items()], a.launches, a.warmup, a.repeats)
    for e in envs.values():
        assert torch.isfinite(e.rew_buf).all()

    med = lambda k: res["ms_per_call"][k]["median"]
    lines = [f"| form | ms per call, {n} envs |", "|---|---|"]
    for name, t in res["ms_per_call"].items():
        lines.append(f"| {name} | {t['median']:.4f} [{t['min']:.4f} .. {t['max']:.4f}] |")
    lines += ["", "Fallback / kernel: " + ", ".join(f"{med('torch fallback, ' + m) / med('shf_actuator_step, ' + m):.1f} x ({m})" for m in modes) + ".",
              f"Kernel against fallback after four calls from the same state: {diffs}.", "",
              f"| hook env, decimation {int(next(iter(envs.values())).isg_env.decimation)} | ms per env step, {n} envs |", "|---|---|"]
    for name, t in res["ms_per_env_step"].items():
        lines.append(f"| {name} | {t['median']:.4f} [{t['min']:.4f} .. {t['max']:.4f}] |")
    lines += ["", f"{a.repeats} interleaved blocks of {a.launches} calls between device events, median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Actuator models: kernel, torch fallback and the hook-env step (tools/bench_actuator.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
