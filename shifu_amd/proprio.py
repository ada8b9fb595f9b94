"""Host side of the proprioceptive sensors (csrc/shf_proprio.hip: shf_proprioception_step, whose header states the algorithm):
the config struct, the device parameter vector with the products and reciprocals the kernel does not form itself, and the state
tensors.  Shared by glue.proprioception_step (the kernel), utils.torch_utils.proprioception_step (the same algorithm in torch),
units.ProprioceptionSensor and the fused envs' add_proprioception.  Nothing here needs a GPU."""
import math

import numpy as np
import torch

from . import _abi

MAX_IMUS, MAX_FEET, MAX_SLOTS = _abi.PROPRIO_MAX_IMUS, _abi.PROPRIO_MAX_FEET, _abi.PROPRIO_MAX_SLOTS
STATE_NAMES = ("counter", "imu", "enc", "foot")
OUTPUT_NAMES = ("gyro", "accel", "dof_pos", "dof_vel", "contact", "first_contact", "air_time", "contact_time", "last_air_time",
                "last_contact_time")


def make_config(imus=(), feet=(), num_bodies=None, contact_mode="norm", velocity="direct", slots=1, max_delay=None, gravity=(0.0, 0.0, -9.81),
                dt=0.02, seed=0, env_id_offset=0):
    """The ShfProprioConfig of a sensor.  imus: [dict(body=int, position=(x, y, z), quat=(x, y, z, w))] (position and quat
    optional: the body frame itself; the quat is normalised); feet: body indices; slots: the latency ring's slots L (1..8);
    max_delay: the largest per-env delay the sensor will be given (default L - 1); dt: seconds between two reads.  Refuses, with
    the words the library uses, what the library refuses."""
    imus, feet = list(imus), [int(b) for b in feet]
    if len(imus) > MAX_IMUS:
        raise ValueError(f"proprioception: more than {MAX_IMUS} IMUs ({len(imus)})")
    if len(feet) > MAX_FEET:
        raise ValueError(f"proprioception: more than {MAX_FEET} feet ({len(feet)})")
    if not 1 <= int(slots) <= MAX_SLOTS:
        raise ValueError(f"proprioception: slots {slots} outside 1..{MAX_SLOTS}")
    max_delay = int(slots) - 1 if max_delay is None else int(max_delay)
    if not 0 <= max_delay < int(slots):
        raise ValueError(f"proprioception: a delay of slots or more (max_delay {max_delay} outside 0..{int(slots) - 1})")
    if not float(dt) > 0.0:
        raise ValueError(f"proprioception: dt must be positive, got {dt}")
    if contact_mode not in _abi.PROPRIO_CONTACT_MODES:
        raise ValueError(f"proprioception: mode must be one of {sorted(_abi.PROPRIO_CONTACT_MODES)}, got {contact_mode!r}")
    if velocity not in _abi.PROPRIO_VELOCITY_MODES:
        raise ValueError(f"proprioception: velocity must be one of {sorted(_abi.PROPRIO_VELOCITY_MODES)}, got {velocity!r}")
    c = _abi.ShfProprioConfig()
    c.env_id_offset = int(env_id_offset)
    c.seed_lo, c.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    c.num_imus, c.num_feet = len(imus), len(feet)
    for i in range(MAX_IMUS):
        c.imu_quat[i][3] = 1.0
    for i, m in enumerate(imus):
        b = int(m["body"])
        if num_bodies is not None and not 0 <= b < int(num_bodies):
            raise ValueError(f"proprioception: IMU {i}'s body index {b} outside 0..{int(num_bodies) - 1}")
        c.imu_body[i] = b
        p = np.asarray(m.get("position", (0.0, 0.0, 0.0)), np.float64).reshape(3)
        q = np.asarray(m.get("quat", (0.0, 0.0, 0.0, 1.0)), np.float64).reshape(4)
        q = q / np.linalg.norm(q)
        for a in range(3):
            c.imu_pos[i][a] = float(p[a])
        for a in range(4):
            c.imu_quat[i][a] = float(q[a])
    for f, b in enumerate(feet):
        if num_bodies is not None and not 0 <= b < int(num_bodies):
            raise ValueError(f"proprioception: foot {f}'s body index {b} outside 0..{int(num_bodies) - 1}")
        c.foot_body[f] = b
    c.contact_mode, c.velocity_mode = _abi.PROPRIO_CONTACT_MODES[contact_mode], _abi.PROPRIO_VELOCITY_MODES[velocity]
    c.slots, c.max_delay = int(slots), max_delay
    for a in range(3):
        c.gravity[a] = float(gravity[a])
    c.dt = float(dt)
    c.inv_dt = float(np.float32(1.0) / np.float32(dt))
    return c


def make_params(dt, gyro_noise=0.0, accel_noise=0.0, gyro_walk=0.0, accel_walk=0.0, gyro_bias=0.0, accel_bias=0.0, dof_pos_noise=0.0,
                dof_vel_noise=0.0, dof_offset=0.0, resolution=0.0, f_on=1.0, f_off=None):
    """The (PROPRIO_NUM_PARAMS) float32 parameter vector (a CPU tensor; the order is _abi.PROPRIO_PARAMS): the noise levels, the
    walks times sqrt(dt), the encoder resolution with its reciprocal, the thresholds squared -- every product and reciprocal the
    kernel reads instead of forming it."""
    f_off = f_on if f_off is None else f_off
    if not 0.0 <= float(f_off) <= float(f_on):
        raise ValueError(f"proprioception: need 0 <= f_off <= f_on, got f_off {f_off}, f_on {f_on}")
    vals = dict(gyro_noise=gyro_noise, accel_noise=accel_noise, gyro_walk_sqrt_dt=gyro_walk * math.sqrt(dt),
                accel_walk_sqrt_dt=accel_walk * math.sqrt(dt), gyro_bias=gyro_bias, accel_bias=accel_bias, dof_pos_noise=dof_pos_noise,
                dof_vel_noise=dof_vel_noise, dof_offset=dof_offset, resolution=resolution,
                inv_resolution=float(np.float32(1.0) / np.float32(resolution)) if resolution > 0 else 0.0,
                f_on_sq=float(f_on) * float(f_on), f_off_sq=float(f_off) * float(f_off))
    for k, v in vals.items():
        if not (float(v) >= 0.0 and math.isfinite(float(v))):
            raise ValueError(f"proprioception: {k} must be finite and not negative, got {v}")
    p = torch.zeros(_abi.PROPRIO_NUM_PARAMS, dtype=torch.float32)
    for i, k in enumerate(_abi.PROPRIO_PARAMS):
        p[i] = float(vals[k])
    return p


def state_shapes(n, num_imus, num_dof, num_feet, slots):
    U = num_imus + num_dof + num_feet
    return dict(counter=(n, U, 2), imu=(n, num_imus, 9 + 6 * slots), enc=(n, num_dof, 2 + 2 * slots), foot=(n, num_feet, 5 + 6 * slots))


def make_state(n, num_imus, num_dof, num_feet, slots, device="cpu"):
    """The zeroed state tensors {"counter" int32, "imu", "enc", "foot" float32} (the layouts are in csrc/shf_proprio.hip's header)."""
    return {k: torch.zeros(s, dtype=torch.int32 if k == "counter" else torch.float32, device=device)
            for k, s in state_shapes(n, num_imus, num_dof, num_feet, slots).items()}


def out_width(num_imus, num_dof, num_feet):
    return 6 * num_imus + 2 * num_dof + 6 * num_feet


def split_output(flat, switches, num_imus, num_dof, num_feet):
    """The named views of the packed (n, D) output: gyro / accel (n, I, 3), dof_pos / dof_vel (n, nd), the four times (n, F);
    contact / first_contact (n, F) are views of the uint8 `switches` (n, 2 F) when given, else of the packed floats."""
    n, I, nd, F = flat.shape[0], num_imus, num_dof, num_feet
    o, at = {}, 0
    for name, w, shape in (("gyro", 3 * I, (n, I, 3)), ("accel", 3 * I, (n, I, 3)), ("dof_pos", nd, (n, nd)), ("dof_vel", nd, (n, nd))) + \
            tuple((k, F, (n, F)) for k in OUTPUT_NAMES[4:]):
        o[name] = flat[:, at:at + w].view(*shape) if name in ("gyro", "accel") and I > 0 else flat[:, at:at + w]
        at += w
    if switches is not None:
        o["contact"], o["first_contact"] = switches[:, :F], switches[:, F:]
    return o


NOISE_NAMES = ("gyro_noise", "accel_noise", "gyro_walk", "accel_walk", "gyro_bias", "accel_bias", "dof_pos_noise", "dof_vel_noise",
               "dof_offset", "resolution", "f_on", "f_off")


class Proprioception:
    """One proprioceptive sensor set for num_envs envs: the config, the device parameter vector, the per-env delays, the state
    and the output tensors, and the read.  On float32 CUDA tensors a read is one launch (glue.proprioception_step); on CPU
    tensors, or with backend="torch", the same algorithm runs as torch expressions (utils.torch_utils.proprioception_step).

    read(body_state, dof_state, contact) -> dict of views of `flat` (n, D): gyro / accel (n, I, 3), dof_pos / dof_vel (n, nd),
    air_time / contact_time / last_air_time / last_contact_time (n, F); contact / first_contact (n, F) uint8 are views of
    `switches` (the packed tensor holds them as 0 / 1 floats too).  The same tensors at every read.
    reset(env_ids): the next read treats these envs as teleported (no acceleration across the jump, biases and offsets redrawn,
    times zeroed, every latency slot filled with that read).  randomize(env_ids, delay=(lo, hi)): per-env latencies."""

    def __init__(self, num_envs, num_bodies, num_dof, device, imus=(), feet=(), contact_mode="norm", velocity="direct", max_delay=0,
                 delay=0, gravity=(0.0, 0.0, -9.81), dt=0.02, seed=0, env_id_offset=0, backend="auto", **noise):
        if backend not in ("auto", "torch"):
            raise ValueError("backend: 'auto' (the kernel on CUDA tensors, torch expressions elsewhere) or 'torch'")
        unknown = sorted(set(noise) - set(NOISE_NAMES))
        if unknown:
            raise TypeError(f"proprioception: unknown arguments {unknown} (noise terms: {NOISE_NAMES})")
        self.backend = backend
        self.num_envs, self.num_bodies, self.num_dof, self.device = int(num_envs), int(num_bodies), int(num_dof), torch.device(device)
        self.config = make_config(imus, feet, num_bodies=num_bodies, contact_mode=contact_mode, velocity=velocity, slots=int(max_delay) + 1,
                                  max_delay=int(max_delay), gravity=gravity, dt=dt, seed=seed, env_id_offset=env_id_offset)
        self.num_imus, self.num_feet, self.max_delay, self.dt = self.config.num_imus, self.config.num_feet, int(max_delay), float(dt)
        self.noise = dict(noise)
        self.params = make_params(dt, **noise).to(self.device)
        n, dev = self.num_envs, self.device
        self.delay = torch.zeros(n, 3, dtype=torch.int32, device=dev)
        self.set_delay(delay)
        self.state = make_state(n, self.num_imus, self.num_dof, self.num_feet, self.config.slots, dev)
        self.flat = torch.zeros(n, out_width(self.num_imus, self.num_dof, self.num_feet), dtype=torch.float32, device=dev)
        self.switches = torch.zeros(n, 2 * self.num_feet, dtype=torch.uint8, device=dev)
        self.outputs = split_output(self.flat, self.switches, self.num_imus, self.num_dof, self.num_feet)
        self.pending = torch.ones(n, dtype=torch.uint8, device=dev)         # the first read is a reset read anyway (counter 0)
        self.last_reset = torch.zeros(n, dtype=torch.uint8, device=dev)      # the flags the last read used

    def set_noise(self, **noise):
        """New noise levels / thresholds (NOISE_NAMES), written into the device parameter vector in place: a captured read
        sees them at its next replay."""
        unknown = sorted(set(noise) - set(NOISE_NAMES))
        if unknown:
            raise TypeError(f"proprioception: unknown noise terms {unknown}")
        self.noise.update(noise)
        self.params.copy_(make_params(self.dt, **self.noise))

    def set_delay(self, delay):
        """An int for every env and class, three ints (IMUs, encoders, feet), or a (num_envs, 3) integer tensor; 0..max_delay reads."""
        d = torch.as_tensor(delay, dtype=torch.int32).to(self.device)
        d = d.expand(self.num_envs, 3) if d.dim() < 2 else d.reshape(self.num_envs, 3)
        if int(d.min()) < 0 or int(d.max()) > self.max_delay:
            raise ValueError(f"proprioception: delay {int(d.min())}..{int(d.max())} outside 0..max_delay = {self.max_delay} (a delay of slots or more)")
        self.delay.copy_(d)

    def randomize(self, env_ids=None, delay=None, generator=None):
        """Per-env draws for env_ids (None: every env): delay = (lo, hi) whole reads, drawn per env and class."""
        dev = self.device
        ids = torch.arange(self.num_envs, device=dev) if env_ids is None else torch.as_tensor(env_ids, device=dev).reshape(-1)
        if delay is not None:
            lo, hi = int(delay[0]), int(delay[1])
            if lo < 0 or hi > self.max_delay or lo > hi:
                raise ValueError(f"proprioception: delay range {lo}..{hi} outside 0..max_delay = {self.max_delay}")
            self.delay[ids] = torch.randint(lo, hi + 1, (ids.numel(), 3), device=dev, generator=generator).to(torch.int32)

    def reset(self, env_ids=None):
        if env_ids is None:
            self.pending.fill_(1)
        else:
            self.pending[env_ids] = 1

    def uses_kernel(self, dof_state):
        return self.backend == "auto" and dof_state.is_cuda and dof_state.dtype == torch.float32

    def read(self, body_state, dof_state, contact, extra_reset=None):
        """body_state (n, nb, 13), dof_state (n, nd, >= 2), contact (n, nb, 3): tensors or strided views with a contiguous last
        axis, read in place.  extra_reset (n) uint8 or None: flags OR-ed into the pending ones for this read.  No host sync."""
        if extra_reset is not None:
            torch.bitwise_or(self.pending, extra_reset, out=self.pending)
        self.last_reset.copy_(self.pending)
        if self.uses_kernel(dof_state):
            from . import glue as impl
        else:
            from .utils import torch_utils as impl
        impl.proprioception_step(body_state if self.num_imus else None, dof_state, contact if self.num_feet else None, self.config, self.params,
                                 self.delay, self.state, self.flat, self.switches, self.last_reset)
        self.pending.zero_()
        return self.outputs
