"""Gaits for LeggedRobot.locomotion_control: which feet stand when (csrc/shf_gait.hip: shf_gait_plan).

A Gait is a period, a duty factor (the fraction of the period a foot stands; a number or one per foot) and per-foot offsets
(fractions of the period by which a foot's cycle is ahead), plus the planner's settings.  The kernel counts integer ticks, one
per simulation step; `ticks(dt)` converts and refuses what does not fall on whole ticks.  GaitState holds the five per-env
tensors the planner reads and writes in place."""
import torch


class Gait:
    def __init__(self, period_s, duty, offsets, apex=0.06, late_depth=0.02, k_fb=0.18, max_step=0.15, leash=float("inf"),
                 contact_threshold=1.0):
        self.period_s = float(period_s)
        self.offsets = tuple(float(o) for o in offsets)
        self.duty = tuple(float(d) for d in duty) if hasattr(duty, "__len__") else (float(duty),) * len(self.offsets)
        assert len(self.duty) == len(self.offsets) and 1 <= len(self.offsets) <= 4, "one to four feet"
        assert self.period_s > 0 and all(0.0 < d <= 1.0 for d in self.duty) and all(0.0 <= o < 1.0 for o in self.offsets)
        self.apex, self.late_depth, self.k_fb, self.max_step = float(apex), float(late_depth), float(k_fb), float(max_step)
        self.leash, self.contact_threshold = float(leash), float(contact_threshold)

    # feet in body order; on the A1 feet (0, 3) and (1, 2) are the diagonal pairs, (0, 1) the front pair, (0, 2) one side
    @classmethod
    def trot(cls, period_s=0.3, duty=0.5, **kw):
        """Diagonal pairs in turn."""
        return cls(period_s, duty, (0.0, 0.5, 0.5, 0.0), **kw)

    @classmethod
    def stand(cls, period_s=0.3, **kw):
        """Every foot always scheduled to stand."""
        return cls(period_s, 1.0, (0.0, 0.0, 0.0, 0.0), **kw)

    @classmethod
    def walk(cls, period_s=0.6, duty=0.75, **kw):
        """One foot at a time, a quarter period apart, diagonal feet half a period apart."""
        return cls(period_s, duty, (0.0, 0.5, 0.25, 0.75), **kw)

    @classmethod
    def pace(cls, period_s=0.3, duty=0.5, **kw):
        """Left and right pairs in turn."""
        return cls(period_s, duty, (0.0, 0.5, 0.0, 0.5), **kw)

    @classmethod
    def bound(cls, period_s=0.3, duty=0.5, **kw):
        """Front and rear pairs in turn."""
        return cls(period_s, duty, (0.0, 0.0, 0.5, 0.5), **kw)

    @property
    def num_feet(self):
        return len(self.offsets)

    def ticks(self, dt):
        """(period_ticks, offset_ticks, stance_ticks) at `dt` seconds per tick.  The period must be a whole number of ticks
        (within 1e-6 of one); offsets and stance durations are rounded to the nearest tick, a stance to at least one."""
        x = self.period_s / float(dt)
        P = int(round(x))
        if P < 1 or abs(x - P) > 1e-6 * max(x, 1.0):
            raise ValueError(f"gait period {self.period_s} s is not a whole number of {dt} s ticks")
        offsets = [int(round(o * P)) % P for o in self.offsets]
        stance = [min(P, max(1, int(round(d * P)))) for d in self.duty]
        return P, offsets, stance


class GaitState:
    """tick (n) int32, sched (n, F) uint8, anchor (n, F, 3), target (n, 13), yaw (n): shf_gait_plan's per-env state.  A new state
    has `pending` set for every env: the next plan resets those envs (clock at 0, anchors at the feet, target over the base).
    It also carries what the horizon MPC keeps between ticks (mpc_u, mpc_forces, mpc_count); reset() clears them too."""

    def __init__(self, n, F, device, dtype=torch.float32):
        self.n, self.F = int(n), int(F)
        self.tick = torch.zeros(n, dtype=torch.int32, device=device)
        self.sched = torch.ones(n, F, dtype=torch.uint8, device=device)
        self.anchor = torch.zeros(n, F, 3, dtype=dtype, device=device)
        self.target = torch.zeros(n, 13, dtype=dtype, device=device)
        self.target[:, 6] = 1.0
        self.yaw = torch.zeros(n, dtype=dtype, device=device)
        self.pending = torch.ones(n, dtype=torch.uint8, device=device)
        self.any_pending = True
        # the horizon MPC's (controller="mpc"): the last solution u (n, H, F, 3), the forces held between two solves, and the
        # ticks since the state was made or reset (a solve falls on every mpc_every-th)
        self.mpc_u = None
        self.mpc_forces = torch.zeros(n, F, 3, dtype=dtype, device=device)
        self.mpc_count = 0

    def reset(self, env_ids=None):
        if env_ids is None:
            self.pending.fill_(1)
        else:
            self.pending[env_ids] = 1
        self.any_pending = True
        ids = slice(None) if env_ids is None else env_ids
        if self.mpc_u is not None:
            self.mpc_u[ids] = 0.0
        self.mpc_forces[ids] = 0.0
        self.mpc_count = 0                          # the next tick solves

    def mpc_buffers(self, horizon):
        """(u (n, horizon, F, 3), held forces (n, F, 3)) of the horizon MPC; u is made (zero: a cold start) on first use and
        whenever the horizon changes."""
        if self.mpc_u is None or self.mpc_u.shape[1] != int(horizon):
            self.mpc_u = torch.zeros(self.n, int(horizon), self.F, 3, dtype=self.mpc_forces.dtype, device=self.mpc_forces.device)
            self.mpc_count = 0
        return self.mpc_u, self.mpc_forces

    def take_pending(self):
        """The reset flags for the next plan (None when nothing is pending); a copy, the flags themselves are cleared."""
        if not self.any_pending:
            return None
        r = self.pending.clone()
        self.pending.zero_()
        self.any_pending = False
        return r

    def tensors(self):
        return self.tick, self.sched, self.anchor, self.target, self.yaw


def nominal_foot_positions(model, q, feet):
    """(len(feet), 3) float64: the origins of bodies `feet` in the base frame at dof positions q, by forward kinematics on a
    compiled model (ShfModel: parent, jtype, dof, tpos, trot, axis)."""
    import numpy as np
    from .. import _abi
    m = model
    R, p = [None] * m.nb, [None] * m.nb
    for b in range(m.nb):
        if m.jtype[b] == _abi.JOINT_ROOT:
            R[b], p[b] = np.eye(3), np.zeros(3)
            continue
        par = m.parent[b]
        Rj = R[par] @ np.array(m.trot[b], np.float64).reshape(3, 3)
        p[b] = p[par] + R[par] @ np.array(m.tpos[b], np.float64)
        a = np.array(m.axis[b], np.float64)
        if m.jtype[b] == _abi.JOINT_REVOLUTE:
            K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            t = float(q[m.dof[b]])
            R[b] = Rj @ (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K))
        elif m.jtype[b] == _abi.JOINT_PRISMATIC:
            R[b], p[b] = Rj, p[b] + (Rj @ a) * float(q[m.dof[b]])
        else:
            R[b] = Rj
    return np.array([p[b] for b in feet])


def foot_radius(model, feet):
    """The largest collision-sphere radius on bodies `feet` (0 when they carry none)."""
    r = [float(model.pt_radius[i]) for i in range(model.np) if int(model.pt_body[i]) in feet]
    return max(r) if r else 0.0


def chain_mask(model, feet):
    """(len(feet), nd) uint8 tensor (CPU): 1 where a dof lies on the chain from the root to a foot."""
    mask = torch.zeros(len(feet), model.nd, dtype=torch.uint8)
    for f, b in enumerate(feet):
        while b > 0:
            if model.dof[b] >= 0:
                mask[f, model.dof[b]] = 1
            b = model.parent[b]
    return mask


PRESETS = {"trot": Gait.trot, "stand": Gait.stand, "walk": Gait.walk, "pace": Gait.pace, "bound": Gait.bound}
