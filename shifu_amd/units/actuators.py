"""Actuator models for the facade / hook path: what sits between a commanded joint angle and a joint torque
(csrc/shf_actuator.hip: shf_actuator_step, whose header states the algorithm step by step).

    Actuator.pd(kp, kd, effort_limit, delay)                                  an ideal PD, the command `delay` sub-steps late
    Actuator.dc_motor(kp, kd, saturation_effort, velocity_limit, effort_limit)  ... clipped by the motor's torque-speed line
    Actuator.network(net, taps, ...)                                          a learned actuator net over short histories of
                                                                              position error and velocity (ActuatorNet)

One `efforts(targets, dof_state)` call is one simulation sub-step and one launch on the GPU; on CPU tensors (or with
backend="torch") the same algorithm runs as torch expressions (utils.torch_utils.actuator_step).  The actuator owns its state:
the command history and, for a network, the error and velocity histories.  Robot.set_actuator / apply_actuator_targets drive
it from a robot in DOF_MODE_EFFORT; the fused one-launch envs keep their built-in PD (DESIGN.md 8h "Actuator models")."""
import numpy as np
import torch

from .. import _abi

MAX_SLOTS, MAX_TAPS, MAX_LAYERS, MAX_WIDTH = _abi.ACTUATOR_MAX_SLOTS, _abi.ACTUATOR_MAX_TAPS, _abi.ACTUATOR_MAX_LAYERS, _abi.ACTUATOR_MAX_WIDTH
_ACTIVATION_MODULES = {"Softsign": "softsign", "ReLU": "relu", "Tanh": "tanh", "ELU": "elu"}


class ActuatorNet:
    """A small MLP (error taps, velocity taps) -> torque: `layers` [(W (out, in), b (out)), ...] float32 CPU tensors and the
    activation between them.  The kernel's limits, each refused with a message that names it: at most 4 linear layers, widths
    at most 64, one output.  bind(device, taps, scales) gives the copy the two backends read: .layers there, .packed (the zero-padded weight
    buffer in the layout include/shifu_amd.h states) and .struct (the host-side description), for the taps and scales of one
    Actuator."""

    def __init__(self, layers, activation):
        if activation not in _abi.ACTUATOR_ACTIVATIONS:
            raise ValueError(f"actuator net: unknown activation {activation!r} (one of {sorted(_abi.ACTUATOR_ACTIVATIONS)})")
        self.layers = [(torch.as_tensor(W, dtype=torch.float32).detach().cpu().contiguous(),
                        torch.as_tensor(b, dtype=torch.float32).detach().cpu().contiguous()) for W, b in layers]
        self.activation = activation
        if not 1 <= len(self.layers) <= MAX_LAYERS:
            raise ValueError(f"actuator net: {len(self.layers)} linear layers, the kernel takes 1 to {MAX_LAYERS}")
        for l, (W, b) in enumerate(self.layers):
            if W.dim() != 2 or b.dim() != 1 or b.shape[0] != W.shape[0]:
                raise ValueError(f"actuator net: layer {l} is not a (out, in) weight with a (out) bias")
            if l > 0 and W.shape[1] != self.layers[l - 1][0].shape[0]:
                raise ValueError(f"actuator net: layer {l} takes {W.shape[1]} inputs, layer {l - 1} gives {self.layers[l - 1][0].shape[0]}")
        self.widths = [self.layers[0][0].shape[1]] + [W.shape[0] for W, _ in self.layers]
        for w in self.widths:
            if not 1 <= w <= MAX_WIDTH:
                raise ValueError(f"actuator net: width {w}, the kernel takes widths of 1 to {MAX_WIDTH}")
        if self.widths[0] % 2 or self.widths[0] > 2 * MAX_TAPS:
            raise ValueError(f"actuator net: {self.widths[0]} inputs, the kernel takes 2 x (1 to {MAX_TAPS} taps)")
        if self.widths[-1] != 1:
            raise ValueError(f"actuator net: {self.widths[-1]} outputs, the kernel takes a last width of 1")

    # -- the three sources -----------------------------------------------------------------------------------------------
    @classmethod
    def from_module(cls, module):
        """An nn.Sequential of Linear and activation modules: Linear, act, Linear, act, ..., Linear, one kind of activation."""
        layers, acts, last = [], set(), None
        for m in module:
            kind = type(m).__name__
            if isinstance(m, torch.nn.Linear):
                if last == "linear":
                    raise ValueError("actuator net: two Linear modules without an activation between them")
                if m.bias is None:
                    raise ValueError("actuator net: a Linear without bias")
                layers.append((m.weight, m.bias))
                last = "linear"
            elif kind in _ACTIVATION_MODULES:
                if last != "linear":
                    raise ValueError("actuator net: an activation that does not follow a Linear")
                if kind == "ELU" and float(m.alpha) != 1.0:
                    raise ValueError("actuator net: ELU with alpha other than 1")
                acts.add(_ACTIVATION_MODULES[kind])
                last = "act"
            else:
                raise ValueError(f"actuator net: module {kind} is neither a Linear nor one of {sorted(_ACTIVATION_MODULES)}")
        if last != "linear":
            raise ValueError("actuator net: the last module must be a Linear")
        if len(acts) > 1:
            raise ValueError(f"actuator net: one kind of activation, not {sorted(acts)}")
        return cls(layers, acts.pop() if acts else "softsign")

    @classmethod
    def from_state_dict(cls, state_dict, activation):
        """The 2-d `*weight` tensors of a state dict in their order, each with its `*bias`."""
        names = [k for k, v in state_dict.items() if k.endswith("weight") and getattr(v, "dim", lambda: 0)() == 2]
        if not names:
            raise ValueError("actuator net: no 2-d weight in the state dict")
        return cls([(state_dict[k], state_dict[k[:-len("weight")] + "bias"]) for k in names], activation)

    @classmethod
    def from_npz(cls, path, activation=None):
        """Keys w0, b0, w1, b1, ...; the activation from the file's `activation` entry unless given."""
        z = np.load(path)
        layers = []
        while f"w{len(layers)}" in z:
            layers.append((z[f"w{len(layers)}"], z[f"b{len(layers)}"]))
        if activation is None:
            activation = str(z["activation"]) if "activation" in z else "softsign"
        return cls(layers, activation)

    @classmethod
    def of(cls, net, activation=None):
        """net: an ActuatorNet, an nn.Sequential, a state dict (with `activation`) or the path of an .npz file."""
        if isinstance(net, cls):
            return net
        if isinstance(net, torch.nn.Module):
            return cls.from_module(net)
        if isinstance(net, dict):
            if activation is None:
                raise ValueError("actuator net: a state dict needs activation=")
            return cls.from_state_dict(net, activation)
        return cls.from_npz(net, activation)

    def save_npz(self, path):
        arrays = {"activation": np.array(self.activation)}
        for l, (W, b) in enumerate(self.layers):
            arrays[f"w{l}"], arrays[f"b{l}"] = W.numpy(), b.numpy()
        np.savez(path, **arrays)

    def module(self):
        """The net as an nn.Sequential (float32, CPU)."""
        act = {v: getattr(torch.nn, k) for k, v in _ACTIVATION_MODULES.items()}[self.activation]
        mods = []
        for l, (W, b) in enumerate(self.layers):
            lin = torch.nn.Linear(W.shape[1], W.shape[0])
            with torch.no_grad():
                lin.weight.copy_(W), lin.bias.copy_(b)
            mods += [lin] + ([act()] if l < len(self.layers) - 1 else [])
        return torch.nn.Sequential(*mods)

    # -- what the kernel reads -------------------------------------------------------------------------------------------
    @property
    def padded_width(self):
        return 32 if max(self.widths[1:-1], default=1) <= 32 else 64

    def pack(self):
        """The zero-padded weight buffer (float32, CPU): inputs padded to 8, hidden widths to padded_width; per layer W
        row-major (out, in) then b; a multiple of 4 floats."""
        P, n = self.padded_width, len(self.layers)
        parts = []
        for l, (W, b) in enumerate(self.layers):
            o = 1 if l == n - 1 else P
            i = P if (l > 0 or n == 1) else 2 * MAX_TAPS
            Wp, bp = torch.zeros(o, i), torch.zeros(o)
            Wp[:W.shape[0], :W.shape[1]], bp[:b.shape[0]] = W, b
            parts += [Wp.reshape(-1), bp]
        flat = torch.cat(parts)
        return torch.cat([flat, torch.zeros(-flat.numel() % 4)])

    def bind(self, device, taps, err_scale, vel_scale, out_scale):
        """The copy an Actuator uses: layers and the packed buffer on `device`, the description with its taps and scales."""
        taps = tuple(int(t) for t in taps)
        if not 1 <= len(taps) <= MAX_TAPS:
            raise ValueError(f"actuator net: {len(taps)} taps, the kernel takes 1 to {MAX_TAPS}")
        if self.widths[0] != 2 * len(taps):
            raise ValueError(f"actuator net: a first width of {self.widths[0]} for {len(taps)} taps, it must be 2 x the taps")
        if min(taps) < 0 or max(taps) >= MAX_SLOTS:
            raise ValueError(f"actuator net: tap lags {taps}, the kernel takes lags of 0 to {MAX_SLOTS - 1}")
        b = ActuatorNet.__new__(ActuatorNet)
        b.activation, b.widths = self.activation, self.widths
        b.layers = [(W.to(device), c.to(device)) for W, c in self.layers]
        b.packed = self.pack().to(device)
        b.taps, b.err_scale, b.vel_scale, b.out_scale = taps, float(err_scale), float(vel_scale), float(out_scale)
        s = _abi.ShfActuatorNet()
        s.activation, s.num_layers, s.num_taps = _abi.ACTUATOR_ACTIVATIONS[self.activation], len(self.layers), len(taps)
        for i, w in enumerate(self.widths):
            s.widths[i] = w
        for i, t in enumerate(taps):
            s.taps[i] = t
        s.err_scale, s.vel_scale, s.out_scale = b.err_scale, b.vel_scale, b.out_scale
        b.struct = s
        return b


class Actuator:
    """Gains, options and the state tensors of one actuator model for num_envs x num_dof joints.  Made by pd / dc_motor /
    network; bound to its sizes and device by Robot.set_actuator or by the first efforts() call.

    State: cmd_hist (n, L, nd), L = max_delay + 1 <= 8, and for a network err_hist / vel_hist (n, H, nd), H = the largest tap
    + 1; slot 0 is the last call's value.  A new actuator, and every env named to reset(), starts its next call from a
    history filled with that call's target (and zero error / velocity histories)."""

    def __init__(self, kp=None, kd=None, net=None, taps=(0, 1, 2), err_scale=1.0, vel_scale=1.0, out_scale=1.0, activation=None,
                 saturation_effort=None, velocity_limit=None, effort_limit=None, delay=0, max_delay=None, backend="auto"):
        if backend not in ("auto", "torch"):
            raise ValueError("backend: 'auto' (the kernel on float32 CUDA tensors, torch expressions elsewhere) or 'torch'")
        if (saturation_effort is None) != (velocity_limit is None):
            raise ValueError("the DC-motor clip takes saturation_effort and velocity_limit together")
        self.backend = backend
        self._kp, self._kd = kp, kd
        self._net = None if net is None else ActuatorNet.of(net, activation)
        self._net_args = (tuple(taps), err_scale, vel_scale, out_scale)
        if self._net is None and (kp is None or kd is None):
            raise ValueError("a PD actuator takes kp and kd")
        self._sat, self._vlim, self._lim = saturation_effort, velocity_limit, effort_limit
        if max_delay is None:
            max_delay = int(delay) if not torch.is_tensor(delay) else int(delay.max())
        if not 0 <= int(max_delay) <= MAX_SLOTS - 1:
            raise ValueError(f"max_delay {max_delay}: the command history holds at most {MAX_SLOTS} slots (delays of 0 to {MAX_SLOTS - 1})")
        self.max_delay = int(max_delay)
        self._delay0 = delay
        self.num_envs = self.num_dof = self.device = None
        if self._net is not None:
            self._net.bind("cpu", *self._net_args)            # refuses taps the net or the kernel cannot take, now

    # -- the three kinds -------------------------------------------------------------------------------------------------
    @classmethod
    def pd(cls, kp, kd, effort_limit=None, delay=0, max_delay=None, **kw):
        return cls(kp=kp, kd=kd, effort_limit=effort_limit, delay=delay, max_delay=max_delay, **kw)

    @classmethod
    def dc_motor(cls, kp, kd, saturation_effort, velocity_limit, effort_limit=None, delay=0, max_delay=None, **kw):
        return cls(kp=kp, kd=kd, saturation_effort=saturation_effort, velocity_limit=velocity_limit, effort_limit=effort_limit,
                   delay=delay, max_delay=max_delay, **kw)

    @classmethod
    def network(cls, net, taps=(0, 1, 2), err_scale=1.0, vel_scale=1.0, out_scale=1.0, activation=None, saturation_effort=None,
                velocity_limit=None, effort_limit=None, delay=0, max_delay=None, **kw):
        return cls(net=net, taps=taps, err_scale=err_scale, vel_scale=vel_scale, out_scale=out_scale, activation=activation,
                   saturation_effort=saturation_effort, velocity_limit=velocity_limit, effort_limit=effort_limit, delay=delay,
                   max_delay=max_delay, **kw)

    # -- sizes and device ------------------------------------------------------------------------------------------------
    def _per_dof(self, v, name):
        if v is None:
            return None
        t = torch.as_tensor(v, dtype=torch.float32, device=self.device)
        if t.dim() == 0:
            t = t.expand(self.num_dof)
        if tuple(t.shape) != (self.num_dof,):
            raise ValueError(f"{name}: a number or one per dof ({self.num_dof}), not {tuple(t.shape)}")
        return t.contiguous().clone()

    def _gain(self, v, name):
        t = torch.as_tensor(v, dtype=torch.float32, device=self.device)
        if t.dim() == 2:
            if tuple(t.shape) != (self.num_envs, self.num_dof):
                raise ValueError(f"{name}: per-env gains are (num_envs, num_dof), not {tuple(t.shape)}")
            return t.contiguous().clone()
        return self._per_dof(t, name)

    def bind(self, num_envs, num_dof, device):
        n, nd = int(num_envs), int(num_dof)
        self.num_envs, self.num_dof, self.device = n, nd, torch.device(device)
        dev = self.device
        self.net = None if self._net is None else self._net.bind(dev, *self._net_args)
        self.kp = self.kd = None
        if self.net is None:
            self.kp, self.kd = self._gain(self._kp, "kp"), self._gain(self._kd, "kd")
            if self.kp.dim() != self.kd.dim():
                self.kp, self.kd = self._per_env(self.kp), self._per_env(self.kd)
            self._kp_base, self._kd_base = self.kp.clone(), self.kd.clone()
        self.saturation, self.velocity_limit = self._per_dof(self._sat, "saturation_effort"), self._per_dof(self._vlim, "velocity_limit")
        self.effort_limit = self._per_dof(self._lim, "effort_limit")
        L = self.max_delay + 1
        self.cmd_hist = torch.zeros(n, L, nd, device=dev)
        self.err_hist = self.vel_hist = None
        if self.net is not None:
            H = max(self.net.taps) + 1
            self.err_hist, self.vel_hist = torch.zeros(n, H, nd, device=dev), torch.zeros(n, H, nd, device=dev)
        self.applied_target = torch.zeros(n, nd, device=dev)
        self.efforts_buf = torch.zeros(n, nd, device=dev)
        self.strength = None
        self.delay = 0
        self.set_delay(self._delay0)
        self.pending = torch.ones(n, dtype=torch.uint8, device=dev)
        self.any_pending = True
        return self

    def _per_env(self, g):
        return g if g.dim() == 2 else g.unsqueeze(0).expand(self.num_envs, self.num_dof).contiguous().clone()

    def _bound(self):
        if self.num_envs is None:
            raise RuntimeError("the actuator is not bound yet: Robot.set_actuator, bind(num_envs, num_dof, device) or a first efforts() call")

    # -- the interface ---------------------------------------------------------------------------------------------------
    def reset(self, env_ids=None):
        """The next efforts() call starts these envs (None: every env) from a history filled with that call's target."""
        self._bound()
        if env_ids is None:
            self.pending.fill_(1)
        else:
            self.pending[env_ids] = 1
        self.any_pending = True

    def set_delay(self, delay):
        """An int for every env, or a (num_envs) integer tensor; 0 .. max_delay sub-steps."""
        self._bound()
        if torch.is_tensor(delay):
            d = delay.to(device=self.device, dtype=torch.int32).reshape(self.num_envs).contiguous().clone()
            lo, hi = int(d.min()), int(d.max())
        else:
            d = lo = hi = int(delay)
        if lo < 0 or hi > self.max_delay:
            raise ValueError(f"delay {lo}..{hi} outside 0..max_delay = {self.max_delay} (the command history's slots; max_delay <= {MAX_SLOTS - 1})")
        self.delay = d

    def set_strength(self, strength):
        """(num_envs, num_dof) (or anything that broadcasts to it) factors on the torque before the limits; None: none."""
        self._bound()
        if strength is None:
            self.strength = None
            return
        s = torch.as_tensor(strength, dtype=torch.float32, device=self.device)
        self.strength = s.expand(self.num_envs, self.num_dof).contiguous().clone()

    def randomize(self, env_ids=None, delay=None, strength=None, kp_scale=None, kd_scale=None, generator=None):
        """Per-env draws for env_ids (None: every env), each range (lo, hi): delay whole sub-steps in lo..hi, strength one
        factor per env on every dof, kp_scale / kd_scale one factor per env on the gains the actuator was made with."""
        self._bound()
        n, nd, dev = self.num_envs, self.num_dof, self.device
        ids = torch.arange(n, device=dev) if env_ids is None else torch.as_tensor(env_ids, device=dev).reshape(-1)
        k = ids.numel()
        rand = lambda lo, hi: lo + (hi - lo) * torch.rand(k, device=dev, generator=generator)
        if delay is not None:
            lo, hi = int(delay[0]), int(delay[1])
            if lo < 0 or hi > self.max_delay or lo > hi:
                raise ValueError(f"delay range {lo}..{hi} outside 0..max_delay = {self.max_delay}")
            d = self.delay if torch.is_tensor(self.delay) else torch.full((n,), int(self.delay), dtype=torch.int32, device=dev)
            d[ids] = torch.randint(lo, hi + 1, (k,), device=dev, generator=generator).to(torch.int32)
            self.delay = d
        if strength is not None:
            if self.strength is None:
                self.strength = torch.ones(n, nd, device=dev)
            self.strength[ids] = rand(*strength).unsqueeze(1).expand(k, nd)
        for name, scale in (("kp", kp_scale), ("kd", kd_scale)):
            if scale is None:
                continue
            if self.net is not None:
                raise ValueError(f"{name}_scale: a network actuator has no PD gains")
            self.kp, self.kd = self._per_env(self.kp), self._per_env(self.kd)
            base = self._per_env(getattr(self, f"_{name}_base"))
            getattr(self, name)[ids] = base[ids] * rand(*scale).unsqueeze(1)

    def uses_kernel(self, targets):
        return self.backend == "auto" and targets.is_cuda and targets.dtype == torch.float32

    def efforts(self, targets, dof_state):
        """One sub-step: (num_envs, num_dof) joint efforts for the desired joint angles `targets` (n, nd) and dof_state
        (n, nd, 2) (or the flat (n * nd, 2) dof-state tensor).  Returns efforts_buf, the same tensor at every call;
        applied_target holds the delayed command."""
        if self.num_envs is None:
            self.bind(targets.shape[0], targets.shape[1], targets.device)
        n, nd = self.num_envs, self.num_dof
        if tuple(targets.shape) != (n, nd):
            raise ValueError(f"targets {tuple(targets.shape)}, the actuator is bound to ({n}, {nd})")
        ds = dof_state.view(n, nd, -1) if dof_state.dim() == 2 else dof_state
        reset = self.pending if self.any_pending else None
        kw = dict(kp=self.kp, kd=self.kd, delay=self.delay, strength=self.strength, saturation=self.saturation,
                  velocity_limit=self.velocity_limit, effort_limit=self.effort_limit, reset=reset, net=self.net, err_hist=self.err_hist,
                  vel_hist=self.vel_hist, applied_out=self.applied_target, efforts_out=self.efforts_buf)
        if self.uses_kernel(targets):
            from .. import glue
            glue.actuator_step(targets.contiguous(), ds, self.cmd_hist, **kw)
        else:
            from ..utils.torch_utils import actuator_step
            actuator_step(targets, ds, self.cmd_hist, **kw)
        if reset is not None:
            self.pending.zero_()
            self.any_pending = False
        return self.efforts_buf
