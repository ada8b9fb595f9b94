"""Times the proprioceptive sensors (csrc/shf_proprio.hip: shf_proprioception_step) beside their torch fallback
(utils.torch_utils.proprioception_step) on the tensors of a FusedA1Env -- one IMU on the trunk, the 12 encoders, the 4 foot
switches, every noise term on, per-env latencies of 0..3 reads -- with shf_leg_effort_mix as the yardstick of a launch of this
size; then FusedA1Env.step_random() alone and followed by a read.

    python tools/bench_proprioception.py --envs 4096 --launches 200 --warmup 20 --repeats 5 --out profiles/rNN_proprioception

ms per call by device events: `repeats` interleaved blocks of `launches` calls per form, median [min .. max] over the blocks
(the protocol of tools/bench_gait.py).  The script stops rather than report a ratio if the kernel and its fallback disagree.
There is no target: nobody has measured this kernel before.  --out PREFIX writes PREFIX.json and PREFIX.md."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from shifu_amd import glue  # noqa: E402
from shifu_amd.utils import torch_utils as TU  # noqa: E402

NOISE = dict(gyro_noise=0.02, accel_noise=0.1, gyro_walk=0.01, accel_walk=0.05, gyro_bias=0.05, accel_bias=0.3, dof_pos_noise=0.005,
             dof_vel_noise=0.1, dof_offset=0.02, resolution=0.001, f_on=6.0, f_off=3.0)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from shifu_amd.gym.a1_fused import FusedA1Env
    n, dev = a.envs, "cuda:0"
    env = FusedA1Env(num_envs=n)
    for _ in range(10):
        env.step_random()
    delay = (torch.arange(n, device=dev).view(n, 1) * torch.tensor([1, 3, 5], device=dev) % 4).to(torch.int32)
    kw = dict(imu=[dict(body=0, position=(0.1, -0.05, 0.02), quat=(0.1, 0.2, -0.3, 0.9))], feet="auto", max_delay=3, delay=delay, seed=7, **NOISE)
    sk, st = env.add_proprioception(**kw), env.add_proprioception(backend="torch", **kw)
    nd, F = sk.core.num_dof, sk.core.num_feet
    for _ in range(4):                                                # agreement first: the same reads by both routes
        env.step_random()
        sk.read(), st.read()
    torch.cuda.synchronize()
    differing = int((sk.flat.view(torch.int32) != st.flat.view(torch.int32)).sum()) + \
        int(sum((sk.core.state[k].view(torch.int32) != st.core.state[k].view(torch.int32)).sum() for k in sk.core.state))
    if differing:
        raise SystemExit(f"kernel and torch fallback disagree in {differing} words: a time ratio between them would mean nothing")
    none = torch.zeros(n, dtype=torch.uint8, device=dev)

    def raw(impl, s):
        c = s.core
        return lambda: impl.proprioception_step(s._body, s._dof, s._contact, c.config, c.params, c.delay, c.state, c.flat, c.switches, none)

    target = env.dof_state.view(n, nd, 2)[:, :, 0].contiguous()
    lim = torch.full((nd,), 33.5, device=dev)
    stance = (torch.rand(n, 4, device=dev) < 0.5).to(torch.uint8)
    chain = torch.zeros(4, nd, dtype=torch.uint8, device=dev)
    for f in range(4):
        chain[f, 3 * f:3 * f + 3] = 1
    what = f"1 IMU, {nd} encoders, {F} feet, delays 0..3"
    forms = [(f"shf_proprioception_step ({what})", raw(glue, sk)), (f"torch fallback ({what})", raw(TU, st)),
             ("FusedProprioception.read(): reset flags + the launch", sk.read),
             ("shf_leg_effort_mix (yardstick)", lambda: glue.leg_effort_mix(target, target, stance, chain, lim))]
    res = {"envs": n, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(dev),
           "kernel_vs_torch_words_differing": differing, "ms_per_call": timed(forms, a.launches, a.warmup, a.repeats)}

    def step_and_read():
        env.step_random()
        sk.read()

    res["ms_per_env_step"] = timed([("FusedA1Env.step_random()", env.step_random), ("FusedA1Env.step_random() + read()", step_and_read)],
                                   a.launches, a.warmup, a.repeats)
    assert torch.isfinite(sk.flat).all()
    k, t = (res["ms_per_call"][name]["median"] for name, _ in forms[:2])
    lines = [f"| form | ms per call, {n} envs |", "|---|---|"]
    for name, v in res["ms_per_call"].items():
        lines.append(f"| {name} | {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}] |")
    lines += ["", f"Fallback / kernel: {t / k:.0f} x.  Kernel against fallback after four reads of the env's tensors: {differing} words differ.", "",
              f"| fused env | ms per env step, {n} envs |", "|---|---|"]
    for name, v in res["ms_per_env_step"].items():
        lines.append(f"| {name} | {v['median']:.4f} [{v['min']:.4f} .. {v['max']:.4f}] |")
    lines += ["", f"{a.repeats} interleaved blocks of {a.launches} calls between device events, median [min .. max]; {res['device']}."]
    print("\n".join(lines))
    print(json.dumps(res))
    if a.out:
        with open(a.out + ".json", "w") as f:
            json.dump(res, f, indent=1)
        with open(a.out + ".md", "w") as f:
            f.write("# Proprioceptive sensors: kernel, torch fallback and the fused env step (tools/bench_proprioception.py)\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
