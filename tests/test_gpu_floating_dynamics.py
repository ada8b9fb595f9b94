"""Floating-base Jacobian, mass matrix and bias forces on the GPU (csrc/shf_dyn_fb.hip: shf_sim_floating_dynamics), the foot
controller (csrc/shf_glue.hip: shf_foot_impedance) and what stands on them (gymapi under SHIFU_AMD_FLOATING_DYNAMICS=1,
LeggedRobot, FusedA1Env.whole_body_dynamics).

The references are tests/floating_ref.py in float64 (tests/helpers.newton_euler / forward_kinematics / mechanical_state:
classical vectors, nothing shared with the kernels' spatial algebra), on the float32 inputs the kernel sees:
    M_ref column j = newton_euler(zero velocities, zero gravity, unit acceleration j) [+ armature],
    h_ref = (f0, n0, tau) of newton_euler(all accelerations zero),     J_ref from forward_kinematics.

Measured on an MI355X, the worst over every case (WORST below):  J 1.64e-7, M 1.29e-7, h 1.79e-7 of the largest reference
entry;  |J nu - body velocity| 1.19e-7 of the largest velocity;  momentum 1.29e-7, angular momentum 1.05e-7, kinetic energy
1.75e-7;  foot controller 4.41e-7 of the largest effort.  Each test asserts four times the worst value measured for its
quantity (operation order may change with compiler versions), and never more than 1e-4.  Hover: the held robots move 8.0e-7
(m, rad) in 50 steps while the free ones fall 0.313 m: a ratio of 2.6e-6 against the 1e-3 asked for.
"""
import copy
import os
import tempfile

import numpy as np
import pytest

from shifu_amd import _abi
from shifu_amd.model import asset_path, compile_urdf
from tests import floating_ref as FR
from tests import helpers as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRAVITY = (0.0, 0.0, -9.81)
# The worst value of each measure on an MI355X, over every case of the tests that assert it (they print every figure):
#   J, M, h     |X - X_ref| / max|X_ref|                  test_tensors_match_float64, test_mass_scale_matches_edited_model
#   vel         |J_b nu - body velocity| / max|velocity|  test_jacobian_times_nu_equals_the_body_state
#   P, L, E     |M nu - momentum| / max|momentum|, |nu M nu / 2 - E| / E     test_momentum_and_kinetic_energy
#   foot        |tau - tau64| / max|tau64|                test_foot_impedance_matches_float64
WORST = {"J": 1.635e-7, "M": 1.292e-7, "h": 1.790e-7, "vel": 1.191e-7, "P": 1.292e-7, "L": 1.054e-7, "E": 1.745e-7, "foot": 4.414e-7}
TOL = {k: min(4.0 * v, 1e-4) for k, v in WORST.items()}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible (these tests never fall back to CPU)")


# ---------------------------------------------------------------------------------------------------------- fixtures --
def _link(name, mass, com, I):
    return (f'<link name="{name}"><inertial><origin xyz="{com[0]} {com[1]} {com[2]}" rpy="0 0 0"/><mass value="{mass}"/>'
            f'<inertia ixx="{I[0]}" ixy="{I[1]}" ixz="{I[2]}" iyy="{I[3]}" iyz="{I[4]}" izz="{I[5]}"/></inertial></link>\n')


def _joint(name, kind, parent, child, xyz, rpy, axis):
    lim = '<limit effort="200" lower="-2.0" upper="2.0" velocity="100"/>' if kind != "fixed" else ""
    return (f'<joint name="{name}" type="{kind}"><origin xyz="{xyz[0]} {xyz[1]} {xyz[2]}" rpy="{rpy[0]} {rpy[1]} {rpy[2]}"/>'
            f'<parent link="{parent}"/><child link="{child}"/><axis xyz="{axis[0]} {axis[1]} {axis[2]}"/>{lim}</joint>\n')


# a free root carrying two two-joint fingers, plus one link on a fixed joint: bodies (depth first, siblings by name)
# base, fa1, fa2, fa_pad (welded to fa2), fb1, fb2; dofs fa1 0, fa2 1, fb1 2, fb2 3
TREE_URDF = ('<?xml version="1.0"?>\n<robot name="floating_tree">\n'
             + _link("base", 3.0, (0.01, -0.02, 0.03), (0.04, 0.002, -0.001, 0.05, 0.003, 0.02))
             + _link("fa1", 0.8, (0.07, 0.0, 0.01), (0.002, 0.0001, 0.0, 0.004, 0.0, 0.004))
             + _link("fa2", 0.5, (0.05, 0.01, 0.0), (0.001, 0.0, 0.0002, 0.002, 0.0, 0.002))
             + _link("fa_pad", 0.2, (0.0, 0.0, 0.02), (0.0004, 0.0, 0.0, 0.0004, 0.0, 0.0003))
             + _link("fb1", 0.9, (0.06, -0.01, 0.0), (0.002, 0.0, 0.0001, 0.005, 0.0, 0.005))
             + _link("fb2", 0.4, (0.04, 0.0, 0.01), (0.0008, 0.0, 0.0, 0.0015, 0.0001, 0.0015))
             + _joint("j_fa1", "revolute", "base", "fa1", (0.05, 0.08, 0.25), (0.2, 0, 0.3), (0, 1, 0))
             + _joint("j_fa2", "revolute", "fa1", "fa2", (0.15, 0, 0), (0, 0.1, 0), (0, 0.6, 0.8))
             + _joint("j_fa_pad", "fixed", "fa2", "fa_pad", (0.1, 0, 0), (0, 0.3, 0), (0, 0, 1))
             + _joint("j_fb1", "revolute", "base", "fb1", (0.05, -0.08, 0.25), (-0.2, 0, -0.3), (1, 0, 0))
             + _joint("j_fb2", "revolute", "fb1", "fb2", (0.14, 0, 0), (0, -0.1, 0.2), (0, 1, 0))
             + '</robot>\n')
GROUPS = {"a1": (32, 64), "tree": (16, 32, 64)}
CASES = [(name, g) for name in ("a1", "tree") for g in GROUPS[name]]

_MODELS = {}


def _model(name):
    if name not in _MODELS:
        if name == "a1":
            m = H.a1_model().blob
            assert (m.nb, m.nd, m.fixed_base) == (17, 12, 0) and sum(m.dyn[b] != b for b in range(m.nb)) == 4, "welded feet"
        else:
            with tempfile.NamedTemporaryFile("w", suffix=".urdf", delete=False) as f:
                f.write(TREE_URDF)
                path = f.name
            try:
                m = compile_urdf(path, default_dof_drive_mode=_abi.DOF_MODE_EFFORT, collapse_fixed_joints=False).blob
            finally:
                os.unlink(path)
            assert (m.nb, m.nd, m.fixed_base) == (6, 4, 0) and sum(m.dyn[b] != b for b in range(m.nb)) == 1, "one welded body"
            m.armature[1], m.armature[3] = 0.02, 0.05          # armature on some dofs
        assert all(m.jtype[b] != _abi.JOINT_PRISMATIC for b in range(m.nb)), "newton_euler is revolute-only"
        _MODELS[name] = m
    return _MODELS[name]


def _states(m, n, seed, qd_scale=2.0):
    """q inside the limits, qd, root position, quaternion, v and w: all non-zero."""
    rng = np.random.default_rng(seed)
    lo = np.array([m.lower[d] for d in range(m.nd)]); hi = np.array([m.upper[d] for d in range(m.nd)])
    q = rng.uniform(lo, hi, (n, m.nd)).astype(np.float32)
    qd = rng.uniform(-qd_scale, qd_scale, (n, m.nd)).astype(np.float32)
    root = np.zeros((n, 13), np.float32)
    root[:, :3] = rng.uniform(-1.0, 1.0, (n, 3)) + (0.0, 0.0, 3.0)
    quat = rng.normal(size=(n, 4))
    root[:, 3:7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    root[:, 7:10] = rng.uniform(-1.0, 1.0, (n, 3))
    root[:, 10:13] = rng.uniform(-2.0, 2.0, (n, 3))
    return q, qd, root


def _reference(m, q, qd, root, mscale=None):
    """float64 (J_ref, M_ref, h_ref) per env on the float32 inputs the kernel sees."""
    n = q.shape[0]
    D = m.nd + 6
    J = np.zeros((n, m.nb, 6, D)); M = np.zeros((n, D, D)); h = np.zeros((n, D))
    for e in range(n):
        me = m if mscale is None else FR.scaled(m, mscale[e])
        r = root[e].astype(np.float64)
        qe, qde = q[e].astype(np.float64), qd[e].astype(np.float64)
        J[e] = FR.jacobian(me, qe, r[:3], r[3:7])
        M[e], h[e] = FR.mass_and_bias(me, qe, qde, r[:3], r[3:7], r[7:10], r[10:13], GRAVITY)
    return J, M, h


_CASES = {}


def _case(name, n=19, seed=5):
    """The seeded states of a fixture and their float64 reference: computed once, shared, never modified."""
    key = (name, n, seed)
    if key not in _CASES:
        m = _model(name)
        q, qd, root = _states(m, n, seed)
        J, M, h = _reference(m, q, qd, root)
        for a in (q, qd, root, J, M, h):
            a.setflags(write=False)
        _CASES[key] = (q, qd, root, J, M, h)
    return _CASES[key]


def _sim(blob, q, qd, root, group=64, mscale=None, params=None):
    from shifu_amd.backend import Sim
    n, nd = q.shape
    sim = Sim(params if params is not None else H.sim_params(dt=0.005, gravity=GRAVITY), "cuda:0")
    sim.set_plane(1.0)
    sim.set_articulation(copy.deepcopy(blob))
    sim.finalize(n, 0, group=group)
    dof = np.stack([q, qd], -1).reshape(n * nd, 2).astype(np.float32)
    for tid, a in ((_abi.T_SIM_DOF, dof), (_abi.T_DOF_STATE, dof), (_abi.T_SIM_ROOT, root), (_abi.T_ROOT_STATE, root)):
        sim.tensors[tid].copy_(torch.from_numpy(np.array(a, np.float32)))
    if mscale is not None:
        sim.set_body_mass_scale(mscale)
    return sim


def _wbd(sim, which="JMh"):
    """(J, M, h) as NumPy from one launch into NaN-filled tensors (None for what was not asked for)."""
    n, nb, D = sim.num_envs, sim.model.nb, sim.model.nd + 6
    nan = lambda *s: torch.full(s, float("nan"), device=sim.device)
    J = nan(n, nb, 6, D) if "J" in which else None
    M = nan(n, D, D) if "M" in which else None
    h = nan(n, D) if "h" in which else None
    sim.floating_dynamics(J, M, h)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (J, M, h))


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


def _nu(qd, root):
    return np.concatenate([root[:, 7:10], root[:, 10:13], qd], 1).astype(np.float64)


# ------------------------------------------------------------------------------------------------ against float64 --
@pytest.mark.parametrize("name,group", CASES)
def test_tensors_match_float64(name, group):
    """19 envs (a partial last block at 16, 8 and 4 envs per block) and one env alone, every velocity non-zero: all three
    tensors are written everywhere, M is bit-symmetric, body 0's Jacobian block is exactly [I | 0], entries off a body's chain
    are exactly zero, and J, M and h match the float64 references."""
    _need_gpu()
    m = _model(name)
    q, qd, root, Jr, Mr, hr = _case(name)
    J, M, h = _wbd(_sim(m, q, qd, root, group=group))
    assert np.isfinite(J).all() and np.isfinite(M).all() and np.isfinite(h).all(), "every entry must be written"
    assert np.abs(Jr).max() > 0.5 and np.abs(J).max() > 0.5, "a non-zero Jacobian"
    assert np.array_equal(M, M.transpose(0, 2, 1)), "M must be bit-symmetric"
    assert np.array_equal(J[:, 0], np.broadcast_to(np.hstack([np.eye(6), np.zeros((6, m.nd))]), J[:, 0].shape))
    off = ~np.broadcast_to(FR.chain_mask(m)[None, :, None, :], J.shape)
    assert off.any() and (J[off] == 0.0).all(), "exact zeros off a body's chain"
    ej, em, eh = _rel(J, Jr), _rel(M, Mr), _rel(h, hr)
    print(f"[floating] {name} group {group} n 19: J {ej:.3e}  M {em:.3e}  h {eh:.3e}")
    assert ej <= TOL["J"] and em <= TOL["M"] and eh <= TOL["h"]
    J1, M1, h1 = _wbd(_sim(m, q[:1], qd[:1], root[:1], group=group))
    assert np.array_equal(J1[0], J[0]) and np.array_equal(M1[0], M[0]) and np.array_equal(h1[0], h[0]), "N = 1 must equal env 0 of 19"


@pytest.mark.parametrize("name", ["a1", "tree"])
def test_mass_scale_matches_edited_model(name):
    """SHF_T_BODY_MASS_SCALE bound, factors in [0.5, 2]: M and h are those of a model whose masses and inertia tensors carry
    the factors; the Jacobian does not change."""
    _need_gpu()
    m = _model(name)
    q, qd, root, Jr, _, _ = _case(name)
    s = np.random.default_rng(17).uniform(0.5, 2.0, (19, m.nb)).astype(np.float32)
    _, Mr, hr = _reference(m, q, qd, root, mscale=s.astype(np.float64))
    J, M, h = _wbd(_sim(m, q, qd, root, group=32, mscale=s))
    ej, em, eh = _rel(J, Jr), _rel(M, Mr), _rel(h, hr)
    print(f"[floating] {name} mass scale: J {ej:.3e}  M {em:.3e}  h {eh:.3e}")
    assert ej <= TOL["J"] and em <= TOL["M"] and eh <= TOL["h"]


# --------------------------------------------------------------------------------------- against the existing kernels --
@pytest.mark.parametrize("name,group", [("a1", 32), ("a1", 64), ("tree", 16)])
def test_jacobian_times_nu_equals_the_body_state(name, group):
    """J_b nu = columns 7:13 of SHF_T_BODY_STATE after refresh(BODY), for every body (welded ones included)."""
    _need_gpu()
    m = _model(name)
    q, qd, root, _, _, _ = _case(name)
    sim = _sim(m, q, qd, root, group=group)
    J, _, _ = _wbd(sim, "J")
    sim.refresh(_abi.REFRESH_BODY)
    torch.cuda.synchronize()
    vel = sim.tensors[_abi.T_BODY_STATE].view(19, m.nb, 13)[..., 7:13].cpu().numpy().astype(np.float64)
    got = np.einsum("nbij,nj->nbi", J.astype(np.float64), _nu(qd, root))
    e = _rel(got, vel)
    print(f"[floating] {name} group {group}: |J nu - body velocity| / max|velocity| = {e:.3e}")
    assert np.abs(vel).max() > 1.0 and e <= TOL["vel"]


# ------------------------------------------------------------------------------------------------ physics identities --
@pytest.mark.parametrize("name", ["a1", "tree"])
def test_momentum_and_kinetic_energy(name):
    """In float64 on the GPU's M: M[0:3] nu = the linear momentum, M[3:6] nu = the angular momentum about the root origin,
    nu M nu / 2 = the kinetic energy (mechanical_state knows no armature: its diagonal share is taken off M first)."""
    _need_gpu()
    m = _model(name)
    q, qd, root, _, _, _ = _case(name)
    _, M, _ = _wbd(_sim(m, q, qd, root, group=32), "M")
    M = M.astype(np.float64)
    M[:, 6:, 6:] -= np.diag([np.float64(np.float32(m.armature[d])) for d in range(m.nd)])
    nu = _nu(qd, root)
    P = np.zeros((19, 3)); L = np.zeros((19, 3)); E = np.zeros(19)
    for e in range(19):
        r = root[e].astype(np.float64)
        P[e], L[e], E[e] = FR.momentum_and_energy(m, q[e].astype(np.float64), qd[e].astype(np.float64), r[:3], r[3:7], r[7:10], r[10:13])
    Mnu = np.einsum("nij,nj->ni", M, nu)
    ep, el = _rel(Mnu[:, :3], P), _rel(Mnu[:, 3:6], L)
    ee = float((np.abs(0.5 * np.einsum("ni,ni->n", nu, Mnu) - E) / E).max())
    print(f"[floating] {name}: momentum {ep:.3e}  angular momentum {el:.3e}  kinetic energy {ee:.3e}")
    assert ep <= TOL["P"] and el <= TOL["L"] and ee <= TOL["E"]


# --------------------------------------------------------------------------------------------------------- structure --
@pytest.mark.parametrize("name,group", [("a1", 32), ("tree", 16)])
def test_results_do_not_depend_on_neighbours(name, group):
    """Bit-equal results for an env whether it runs alone, among 19, or at another place of the batch."""
    _need_gpu()
    m = _model(name)
    q, qd, root, _, _, _ = _case(name)
    out = _wbd(_sim(m, q, qd, root, group=group))
    perm = np.random.default_rng(3).permutation(19)
    outp = _wbd(_sim(m, q[perm], qd[perm], root[perm], group=group))
    for a, b in zip(out, outp):
        assert np.array_equal(b, a[perm])
    for e in (7, 18):
        out1 = _wbd(_sim(m, q[e:e + 1], qd[e:e + 1], root[e:e + 1], group=group))
        for a, b in zip(out, out1):
            assert np.array_equal(b[0], a[e])


def test_uniform_mass_factor_two_doubles_mass_matrix_and_bias():
    """Every factor 2, zero armature (the A1): exactly 2 M and 2 h -- every operation on the masses is linear and a factor of
    two is exact in binary floating point; the Jacobian is untouched."""
    _need_gpu()
    m = _model("a1")
    assert all(m.armature[d] == 0.0 for d in range(m.nd))
    q, qd, root, _, _, _ = _case("a1")
    J1, M1, h1 = _wbd(_sim(m, q, qd, root, group=32))
    J2, M2, h2 = _wbd(_sim(m, q, qd, root, group=32, mscale=np.full((19, m.nb), 2.0, np.float32)))
    assert np.array_equal(M2, 2.0 * M1) and np.array_equal(h2, 2.0 * h1) and np.array_equal(J2, J1)


@pytest.mark.parametrize("name,group", [("a1", 64), ("tree", 16)])
def test_any_subset_of_the_outputs_gives_the_same_values(name, group):
    """One output, or two, requested: bit-equal to the launch that fills all three; all three null is refused."""
    _need_gpu()
    from shifu_amd._lib import BackendError
    m = _model(name)
    q, qd, root, _, _, _ = _case(name)
    sim = _sim(m, q, qd, root, group=group)
    full = dict(zip("JMh", _wbd(sim)))
    for which in ("J", "M", "h", "Mh", "Jh"):
        part = dict(zip("JMh", _wbd(sim, which)))
        for k in "JMh":
            assert (part[k] is None) == (k not in which)
            if k in which:
                assert np.array_equal(part[k], full[k]), f"{k} of the '{which}' launch"
    with pytest.raises(BackendError, match="all three outputs"):
        sim.floating_dynamics(None, None, None)
    with pytest.raises(BackendError, match="fixed base"):          # the fixed-base entry keeps refusing
        sim.dynamics(torch.zeros(19, m.nd, m.nd, device="cuda:0"), None)


# ------------------------------------------------------------------------------------------------------------- hover --
def test_bias_wrench_and_efforts_hold_the_robot_in_the_air():
    """8 A1s at z = 1 m over the plane, nu = 0, random q inside the limits and random root orientation, effort mode, 50 steps
    of 5 ms.  Each step: refresh h, efforts = h[6:], and the single force F = h[0:3] on body 0 at the world point
    p_root + (F x N) / |F|^2, N = h[3:6] (it exists because a gravity wrench has N perpendicular to F), through the path of
    apply_rigid_body_force_at_pos_tensors.  The largest change of any joint angle (rad) and of the root position (m) must be
    at most 1e-3 of what the same robots do without compensation (they fall ~0.3 m and stay clear of the ground)."""
    _need_gpu()
    m = _model("a1")
    n = 8
    q0, _, root0 = _states(m, n, 41)
    root0 = root0.copy()
    root0[:, :3] = (0.0, 0.0, 1.0)
    root0[:, 7:] = 0.0
    moved = []
    for hold in (True, False):
        sim = _sim(m, q0, np.zeros_like(q0), root0)
        D = m.nd + 6
        h = torch.zeros(n, D, device=sim.device)
        force = torch.zeros(n, m.nb, 3, device=sim.device)
        pos = torch.zeros(n, m.nb, 3, device=sim.device)
        for _ in range(50):
            if hold:
                sim.floating_dynamics(None, None, h)
                F, N = h[:, 0:3], h[:, 3:6]
                force[:, 0] = F
                pos[:, 0] = sim.tensors[_abi.T_SIM_ROOT][:, :3] + torch.cross(F, N, dim=1) / (F * F).sum(1, keepdim=True)
                sim.apply_body_force(force.view(-1, 3), pos.view(-1, 3))
            sim.set_dof_command(_abi.T_EFFORT, h[:, 6:].contiguous())
            sim.step()
        sim.refresh(_abi.REFRESH_DOF | _abi.REFRESH_ROOT)
        torch.cuda.synchronize()
        if hold:
            hn = h.cpu().numpy().astype(np.float64)
            cosine = np.abs((hn[:, :3] * hn[:, 3:6]).sum(1)) / (np.linalg.norm(hn[:, :3], axis=1) * np.linalg.norm(hn[:, 3:6], axis=1) + 1e-30)
            assert (cosine <= 1e-5).all(), "a gravity wrench: N perpendicular to F"
        st = sim.tensors[_abi.T_DOF_STATE].view(n, m.nd, 2).cpu().numpy()
        rt = sim.tensors[_abi.T_ROOT_STATE].cpu().numpy()
        assert np.isfinite(st).all() and np.isfinite(rt).all()
        assert (rt[:, 2] > 0.6).all(), "clear of the ground"
        moved.append(max(float(np.abs(st[..., 0] - q0).max()), float(np.abs(rt[:, :3] - root0[:, :3]).max())))
    held, free = moved
    print(f"[hover] held {held:.3e}, free {free:.3e}, ratio {held / free:.3e}")
    assert free > 0.25, "the free robots must fall"
    assert held <= 1e-3 * free


# --------------------------------------------------------------------------------------------------- foot controller --
FEET = (4, 8, 12, 16)
_FOOT = {}


def _foot_setup(n=257):
    """A bare A1 sim of n seeded states with its Jacobian, body-state, dof-state, root-state and bias tensors refreshed on the
    GPU, and seeded targets in the base frame (|target - p| ~ 0.05 m: forces of ~10 N at kp 200)."""
    if not _FOOT:
        m = _model("a1")
        q, qd, root = _states(m, n, 31, qd_scale=1.0)
        sim = _sim(m, q, qd, root)
        sim.refresh(_abi.REFRESH_ALL)
        D = m.nd + 6
        h = torch.zeros(n, D, device=sim.device)
        jac = sim.tensors[_abi.T_JACOBIAN]
        assert tuple(jac.shape) == (n, m.nb, 6, D)
        sim.floating_dynamics(jac, None, h)
        torch.cuda.synchronize()
        body = sim.tensors[_abi.T_BODY_STATE].view(n, m.nb, 13)
        rs = sim.tensors[_abi.T_ROOT_STATE].view(n, 13)
        jf = jac[:, FEET[0]::4]
        fp = body[:, FEET[0]::4, :3]
        assert tuple(jf.shape) == (n, 4, 6, D) and not jf.is_contiguous() and not fp.is_contiguous()
        rng = np.random.default_rng(37)
        R = np.stack([H.quat_to_mat(x) for x in rs[:, 3:7].cpu().numpy().astype(np.float64)])
        p = np.einsum("nji,nfj->nfi", R, (fp.cpu().numpy() - rs[:, None, :3].cpu().numpy()).astype(np.float64))
        target = (p + rng.uniform(-0.05, 0.05, p.shape)).astype(np.float32)
        _FOOT.update(sim=sim, m=m, jf=jf, fp=fp, rs=rs, h=h, dof=sim.tensors[_abi.T_DOF_STATE].view(n, m.nd, 2),
                     target=torch.from_numpy(target).to(sim.device),
                     limit=torch.tensor([m.effort[d] for d in range(m.nd)], device=sim.device))
    return _FOOT


def _gains(dev, kp=200.0):
    kp3 = torch.tensor([kp, 0.8 * kp, 1.3 * kp], device=dev)
    return kp3, 2.0 * torch.sqrt(kp3)


def _foot_ref(S, n, bias, limit):
    kp3, kd3 = _gains("cpu")
    c = lambda t: t[:n].cpu().numpy()
    return FR.foot_impedance(c(S["jf"]), c(S["dof"])[..., 1], c(S["rs"])[:, :3], c(S["rs"])[:, 3:7], c(S["fp"]), c(S["target"]),
                             kp3.numpy(), kd3.numpy(), None if bias is None else c(bias), None if limit is None else limit.cpu().numpy())


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_foot_impedance_matches_float64(n):
    """glue.foot_impedance against the float64 closed form on the GPU's own J, with and without bias and limits."""
    _need_gpu()
    from shifu_amd import glue
    S = _foot_setup()
    kp3, kd3 = _gains(S["h"].device)
    assert float(np.abs(S["h"][:, 6:].cpu().numpy()).max()) > 1.0, "gravity must load the legs"
    for bias, limit in ((None, None), (S["h"], None), (S["h"], S["limit"])):
        tau = glue.foot_impedance(S["jf"][:n], S["dof"][:n], S["rs"][:n], S["fp"][:n], S["target"][:n], kp3, kd3,
                                  None if bias is None else bias[:n], limit)
        torch.cuda.synchronize()
        tau = tau.cpu().numpy()
        free, ref = _foot_ref(S, n, bias, limit)
        e = float(np.abs(tau - ref).max() / np.abs(free).max())
        print(f"[foot] n {n} bias {bias is not None} limit {limit is not None}: |tau - tau64| / max|tau64| = {e:.3e}")
        assert np.isfinite(tau).all() and tau.shape == (n, 12) and e <= TOL["foot"]


def test_foot_impedance_strided_views_equal_contiguous_copies():
    """The feet as a slice of the Jacobian tensor and of the body state, the root row inside the 13-wide root state, dof state
    with element stride 2: bit-equal to contiguous copies (and to a dof buffer of another element stride)."""
    _need_gpu()
    from shifu_amd import glue
    S = _foot_setup()
    kp3, kd3 = _gains(S["h"].device)
    assert S["dof"].stride(1) == 2
    a = glue.foot_impedance(S["jf"], S["dof"], S["rs"], S["fp"], S["target"], kp3, kd3, S["h"], S["limit"])
    wide = torch.zeros(257, 12, 3, device=kp3.device)
    wide[..., :2] = S["dof"]
    b = glue.foot_impedance(S["jf"].contiguous(), wide[..., :2], S["rs"][:, :7].contiguous(), S["fp"].contiguous(), S["target"],
                            kp3, kd3, S["h"], S["limit"])
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_foot_impedance_zero_gains_and_clamp():
    """Zero gains with bias return bias[:, 6:] exactly; the clamp comes last and entries <= 0 of the limit mean no limit."""
    _need_gpu()
    from shifu_amd import glue
    S = _foot_setup()
    dev = S["h"].device
    z3 = torch.zeros(3, device=dev)
    got = glue.foot_impedance(S["jf"], S["dof"], S["rs"], S["fp"], S["target"], z3, z3, S["h"])
    torch.cuda.synchronize()
    assert torch.equal(got, S["h"][:, 6:])
    kp3, kd3 = _gains(dev)
    free = glue.foot_impedance(S["jf"][:2], S["dof"][:2], S["rs"][:2], S["fp"][:2], S["target"][:2], kp3, kd3, S["h"][:2])
    lim = 0.5 * free.abs().min(0).values
    assert float(lim.min()) > 0.0
    lim[1], lim[4] = 0.0, -1.0
    got = glue.foot_impedance(S["jf"][:2], S["dof"][:2], S["rs"][:2], S["fp"][:2], S["target"][:2], kp3, kd3, S["h"][:2], lim)
    torch.cuda.synchronize()
    want = torch.where(lim > 0, torch.maximum(torch.minimum(free, lim), -lim), free)
    keep = [0, 2, 3] + list(range(5, 12))
    assert torch.equal(got, want)
    assert (got[:, keep].abs() == lim[keep]).all() and torch.equal(got[:, [1, 4]], free[:, [1, 4]])


# ------------------------------------------------------------------------------------------------------------ facade --
def _a1_facade(n):
    from shifu_amd.isaacgym import gymapi
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, 0, gymapi.SIM_PHYSX, gymapi.SimParams())
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.default_dof_drive_mode = gymapi.DOF_MODE_EFFORT
    a1 = gym.load_asset(sim, os.path.dirname(asset_path("a1.urdf")), "a1.urdf", opts)
    for e in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 1)
        gym.create_actor(env, a1, gymapi.Transform(gymapi.Vec3(0.0, 0.0, 0.6)), "a1", e, 0)
    gym.prepare_sim(sim)
    return gym, sim


def _set_state(be, q, qd, root):
    n, nd = q.shape
    dof = torch.from_numpy(np.stack([q, qd], -1).reshape(n * nd, 2)).to(be.device)
    be.tensors[_abi.T_SIM_DOF].copy_(dof)
    be.tensors[_abi.T_SIM_ROOT].copy_(torch.from_numpy(root).to(be.device))


def test_facade_tensors_equal_the_backend_when_enabled(monkeypatch):
    """SHIFU_AMD_FLOATING_DYNAMICS=1: the documented shapes, pointer-stable tensors, and the values of Sim.floating_dynamics on
    a bare sim holding the same state, bit for bit; the Jacobian tensor is filled by refresh_jacobian_tensors and by
    refresh_all_state_tensors."""
    _need_gpu()
    from shifu_amd.isaacgym import gymtorch
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    n = 5
    gym, sim = _a1_facade(n)
    be = sim.backend
    m = be.model
    D = m.nd + 6
    q, qd, root = _states(m, n, 23)
    _set_state(be, q, qd, root)
    jac = gymtorch.wrap_tensor(gym.acquire_jacobian_tensor(sim, "a1"))
    assert tuple(jac.shape) == (n, m.nb, 6, D) and float(jac.abs().max()) == 0.0
    gym.refresh_mass_matrix_tensors(sim)          # nothing acquired yet: a no-op
    M = gymtorch.wrap_tensor(gym.acquire_mass_matrix_tensor(sim, "a1"))
    h = gymtorch.wrap_tensor(gym.acquire_dof_bias_force_tensor(sim, "a1"))
    assert tuple(M.shape) == (n, D, D) and tuple(h.shape) == (n, D) and float(M.abs().max()) == 0.0
    gym.refresh_mass_matrix_tensors(sim)
    gym.refresh_jacobian_tensors(sim)
    assert gymtorch.wrap_tensor(gym.acquire_mass_matrix_tensor(sim, "a1")).data_ptr() == M.data_ptr()
    assert gymtorch.wrap_tensor(gym.acquire_dof_bias_force_tensor(sim, "a1")).data_ptr() == h.data_ptr()
    assert gymtorch.wrap_tensor(gym.acquire_jacobian_tensor(sim, "a1")).data_ptr() == jac.data_ptr()
    torch.cuda.synchronize()
    Jb, Mb, hb = _wbd(_sim(m, q, qd, root, params=be.params))          # the facade's gravity
    assert np.array_equal(jac.cpu().numpy(), Jb) and np.array_equal(M.cpu().numpy(), Mb) and np.array_equal(h.cpu().numpy(), hb)
    assert float(np.abs(hb[:, :3]).max()) > 50.0, "the robot's weight"
    jac.zero_()
    gym.refresh_all_state_tensors(sim)
    torch.cuda.synchronize()
    assert np.array_equal(jac.cpu().numpy(), Jb)


def test_facade_is_unchanged_when_the_variable_is_unset(monkeypatch):
    """Unset: the Jacobian tensor of a floating sim is still all zeros after refresh_all_state_tensors and the dynamics
    tensors are refused with 'fixed base'."""
    _need_gpu()
    from shifu_amd.isaacgym import gymtorch
    monkeypatch.delenv("SHIFU_AMD_FLOATING_DYNAMICS", raising=False)
    gym, sim = _a1_facade(3)
    q, qd, root = _states(sim.backend.model, 3, 29)
    _set_state(sim.backend, q, qd, root)
    jac = gymtorch.wrap_tensor(gym.acquire_jacobian_tensor(sim, "a1"))
    gym.refresh_all_state_tensors(sim)
    gym.refresh_jacobian_tensors(sim)
    torch.cuda.synchronize()
    assert float(jac.abs().max()) == 0.0
    with pytest.raises(Exception, match="fixed base"):
        gym.acquire_mass_matrix_tensor(sim, "a1")


def _legged_env(n):
    from examples.a1_conditional.task_config import A1ActorConfig
    from shifu_amd.configs import BaseEnvConfig
    from shifu_amd.gym.isaac_gym import IsaacGymEnv
    from shifu_amd.units import LeggedRobot

    class EnvCfg(BaseEnvConfig):
        num_envs = n

        class control(BaseEnvConfig.control):
            decimation = 1

        class debug(BaseEnvConfig.debug):
            headless = True

    env = IsaacGymEnv(EnvCfg())
    robot = LeggedRobot(A1ActorConfig())
    env.create_envs(robot=robot)
    return env, robot


def test_legged_robot_foot_control_plumbing(monkeypatch):
    """With the variable set: LeggedRobot.j_ee is non-zero and equals the foot rows of the Jacobian tensor, mass_matrix and
    bias_forces have the floating shapes, and apply_target_foot_positions with the current foot positions as targets runs one
    env step on the plane with finite state and efforts inside the limits (a plumbing check, not a behaviour claim).  Unset,
    the same calls raise the facade's 'fixed base' error."""
    _need_gpu()
    from shifu_amd.isaacgym.torch_utils import quat_rotate_inverse
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    n = 4
    env, robot = _legged_env(n)
    nd = robot.num_dof
    ee = [int(b) for b in robot.ee_indices.cpu()]
    jac = env.sim.backend.tensors[_abi.T_JACOBIAN]
    torch.cuda.synchronize()
    assert float(robot.j_ee.abs().max()) > 0.1 and torch.equal(robot.j_ee, jac[:, ee])
    assert torch.equal(robot.foot_jacobians, jac[:, ee])
    assert tuple(robot.mass_matrix.shape) == (n, nd + 6, nd + 6) and tuple(robot.bias_forces.shape) == (n, nd + 6)
    env.gym.refresh_all_state_tensors(env.sim)
    env.gym.refresh_mass_matrix_tensors(env.sim)
    body = env.body_state.view(n, -1, 13)
    root = env.root_state.view(n, -1, 13)[:, 0]
    targets = torch.stack([quat_rotate_inverse(root[:, 3:7], body[:, b, :3] - root[:, :3]) for b in ee], 1)
    tau = robot.foot_impedance_control(targets)
    torch.cuda.synchronize()
    assert tuple(tau.shape) == (n, nd) and torch.isfinite(tau).all() and (tau.abs() <= robot.torque_limits).all()
    assert float((tau - robot.bias_forces[:, 6:].clamp(-robot.torque_limits, robot.torque_limits)).abs().max()) < 1.0, \
        "at the targets and at rest: gravity compensation alone (up to rounding of p)"
    robot.apply_target_foot_positions(targets)
    env.gym.refresh_all_state_tensors(env.sim)
    torch.cuda.synchronize()
    assert torch.isfinite(env.dof_state).all() and torch.isfinite(env.root_state).all() and torch.isfinite(env.body_state).all()
    monkeypatch.delenv("SHIFU_AMD_FLOATING_DYNAMICS")
    robot._mass_matrix = robot._bias_forces = None
    with pytest.raises(Exception, match="fixed base"):
        robot.foot_impedance_control(targets)
    with pytest.raises(Exception, match="fixed base"):
        robot.apply_target_foot_positions(targets)


def test_foot_control_needs_effort_mode(monkeypatch):
    """apply_target_foot_positions raises unless the asset's drive mode is DOF_MODE_EFFORT."""
    _need_gpu()
    from shifu_amd.isaacgym import gymapi
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    env, robot = _legged_env(2)
    monkeypatch.setattr(robot.asset_options, "default_dof_drive_mode", gymapi.DOF_MODE_POS)
    with pytest.raises(RuntimeError, match="DOF_MODE_EFFORT"):
        robot.apply_target_foot_positions(torch.zeros(2, 4, 3, device=robot.device))


def test_fused_env_whole_body_dynamics_equals_the_backend():
    """FusedA1Env.whole_body_dynamics() agrees bit for bit with Sim.floating_dynamics on its own sim; the tensors are allocated
    once and foot_jacobians is the view (n, 4, 6, nd + 6) of the feet's rows."""
    _need_gpu()
    from shifu_amd.gym.a1_fused import FusedA1Env
    env = FusedA1Env(num_envs=8, terrain="flat")
    try:
        env.reset()
        g = torch.Generator(device=env.device).manual_seed(0)
        for _ in range(5):
            env.step(2 * torch.rand(8, 12, device=env.device, generator=g) - 1)
        w = env.whole_body_dynamics()
        J, M, h = _wbd(env.sim)
        torch.cuda.synchronize()
        assert np.array_equal(w["jacobian"].cpu().numpy(), J) and np.array_equal(w["mass_matrix"].cpu().numpy(), M)
        assert np.array_equal(w["bias"].cpu().numpy(), h)
        assert np.abs(J).max() > 0.1 and np.abs(h[:, 6:]).max() > 0.1
        w2 = env.whole_body_dynamics()
        assert all(w2[k].data_ptr() == w[k].data_ptr() for k in ("jacobian", "mass_matrix", "bias"))
        fj = env.foot_jacobians
        assert tuple(fj.shape) == (8, 4, 6, 18) and fj.data_ptr() == w["jacobian"][:, 4].data_ptr()
        assert torch.equal(fj, w["jacobian"][:, list(FEET)])
    finally:
        env.destroy()
