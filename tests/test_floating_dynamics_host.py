"""Host-side checks of the floating-base dynamics feature (no GPU): the two C-ABI entries are declared, bound and additive
(SHF_ABI_VERSION stays 22), the library refuses what it cannot compute, the torch expressions of the foot controller equal a
float64 NumPy evaluation, the float64 references agree with each other, and with SHIFU_AMD_FLOATING_DYNAMICS unset the
facade's Jacobian refresh reaches no new backend call."""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi
from tests import floating_ref as FR
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from shifu_amd import _lib
    from shifu_amd.build import build_native
    build_native()
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "shifu_amd.h")).read()


def test_header_declares_both_entries():
    hdr = _header()
    assert re.search(r"\bint\s+shf_sim_floating_dynamics\s*\(\s*ShfSim\*\s*sim\s*,\s*float\*\s*jacobian_or_null\s*,\s*float\*\s*"
                     r"mass_matrix_or_null\s*,\s*float\*\s*bias_or_null\s*,\s*void\*\s*stream\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+shf_foot_impedance\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 20
    for name in ("j_feet", "j_env_stride", "j_foot_stride", "dof_state", "dof_elem_stride", "root_pose", "root_env_stride", "foot_pos",
                 "foot_env_stride", "foot_stride", "target", "kp3", "kd3", "bias_or_null", "effort_limit_or_null", "num_feet",
                 "num_dof", "efforts_out"):
        assert name in m.group(1)


def test_binding_table_covers_both_entries(lib):
    from shifu_amd import _lib
    assert "shf_sim_floating_dynamics" in _lib.EXPORTS and "shf_foot_impedance" in _lib.EXPORTS
    assert len(_lib._SIGS["shf_sim_floating_dynamics"][0]) == 5 and len(_lib._SIGS["shf_foot_impedance"][0]) == 20
    assert lib.shf_sim_floating_dynamics.restype is ctypes.c_int32 and lib.shf_foot_impedance.restype is ctypes.c_int32


def test_abi_version_is_still_22(lib):
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header())
    assert _abi.SHF_ABI_VERSION == 22
    assert lib.shf_abi_version() == 22


def test_library_refuses_what_it_cannot_compute(lib):
    """A null sim, an unfinalised one, all three outputs null, unbound state and a fixed base: each with a message, all decided
    on the host.  shf_sim_dynamics keeps refusing the floating base."""
    from shifu_amd.model import asset_path, compile_urdf
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    f = lib.shf_sim_floating_dynamics
    assert f(None, out, out, out, None) != 0 and b"null sim" in lib.shf_last_error()
    p = H.sim_params()

    def make(model, finalize=True):
        h = ctypes.c_void_p()
        assert lib.shf_sim_create(ctypes.byref(p), ctypes.byref(h)) == 0
        assert lib.shf_model_bounds(ctypes.byref(model)) == 0
        assert lib.shf_sim_set_articulation(h, ctypes.byref(model)) == 0
        if finalize:
            assert lib.shf_sim_finalize(h, 4, 0) == 0
        return h

    a1 = H.a1_model().blob
    h = make(a1, finalize=False)
    assert f(h, out, out, out, None) != 0 and b"not finalized" in lib.shf_last_error()
    lib.shf_sim_destroy(h)
    h = make(a1)
    assert f(h, None, None, None, None) != 0 and b"all three outputs" in lib.shf_last_error()
    for args in ((out, None, None), (None, out, None), (None, None, out)):
        assert f(h, *args, None) != 0 and b"not bound" in lib.shf_last_error()   # no state tensors here
    assert lib.shf_sim_dynamics(h, out, out, None) != 0 and b"fixed base" in lib.shf_last_error()
    lib.shf_sim_destroy(h)
    arm = compile_urdf(asset_path("abb_rod.urdf"), fix_base_link=True, default_dof_drive_mode=_abi.DOF_MODE_EFFORT).blob
    h = make(arm)
    assert f(h, out, out, out, None) != 0 and b"floating base only" in lib.shf_last_error()
    lib.shf_sim_destroy(h)
    # shf_foot_impedance: null tensors, too many dofs, a dof view without the velocity
    g = lib.shf_foot_impedance
    assert g(None, 0, 0, None, 2, None, 0, None, 0, 0, None, None, None, None, None, 1, 4, 12, None, None) != 0
    assert b"shf_foot_impedance" in lib.shf_last_error()
    assert g(out, 0, 0, out, 2, out, 0, out, 0, 0, out, out, out, None, None, 1, 4, _abi.MAX_DOFS + 1, out, None) != 0
    assert b"too many dofs" in lib.shf_last_error()
    assert g(out, 0, 0, out, 1, out, 0, out, 0, 0, out, out, out, None, None, 1, 4, 12, out, None) != 0
    assert b"element stride" in lib.shf_last_error()


def test_jacobian_refresh_reaches_no_new_backend_call_when_unset(monkeypatch):
    """SHIFU_AMD_FLOATING_DYNAMICS unset: refresh_jacobian_tensors / refresh_all_state_tensors on a floating sim make the one
    backend.refresh call they always made and nothing else; the dynamics tensors stay refused."""
    from shifu_amd.isaacgym import gymapi
    monkeypatch.delenv("SHIFU_AMD_FLOATING_DYNAMICS", raising=False)
    calls = []

    class Model:
        fixed_base = 0
        nd = 12

    class Backend:
        model = Model()
        num_envs = 2

        def refresh(self, mask):
            calls.append(("refresh", mask))

        def __getattr__(self, name):
            raise AssertionError(f"backend.{name} reached although SHIFU_AMD_FLOATING_DYNAMICS is unset")

    sim = gymapi.SimHandle(0, gymapi.SimParams())
    sim.backend = Backend()
    gym = gymapi.acquire_gym()
    gym.refresh_jacobian_tensors(sim)
    gym.refresh_all_state_tensors(sim)
    gym.refresh_mass_matrix_tensors(sim)
    assert calls == [("refresh", _abi.REFRESH_JACOBIAN), ("refresh", _abi.REFRESH_ALL)]
    with pytest.raises(NotImplementedError, match="fixed base"):
        gym.acquire_mass_matrix_tensor(sim, "a1")
    # set: the same calls go on to the floating-base launch, for a floating base only
    monkeypatch.setenv("SHIFU_AMD_FLOATING_DYNAMICS", "1")
    with pytest.raises(AssertionError, match="floating_dynamics"):
        gym.refresh_jacobian_tensors(sim)
    Model.fixed_base = 1
    try:
        del calls[:]
        gym.refresh_jacobian_tensors(sim)
        assert calls == [("refresh", _abi.REFRESH_JACOBIAN)]
    finally:
        Model.fixed_base = 0


def test_float64_references_agree_with_each_other():
    """M_ref nu gives mechanical_state's momenta and kinetic energy, and J_ref nu the body velocities: the references the GPU
    tests lean on are consistent among themselves (A1, one random state with a moving root)."""
    m = H.a1_model().blob
    rng = np.random.default_rng(11)
    q, qd = rng.uniform(-0.5, 0.5, m.nd), rng.uniform(-2, 2, m.nd)
    quat = rng.normal(size=4)
    quat /= np.linalg.norm(quat)
    pr, v, w = rng.normal(size=3), rng.normal(size=3), rng.normal(size=3)
    M, h = FR.mass_and_bias(m, q, qd, pr, quat, v, w, (0.0, 0.0, -9.81))
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    nu = np.concatenate([v, w, qd])
    P, L0, E = FR.momentum_and_energy(m, q, qd, pr, quat, v, w)
    assert np.abs(M[:3] @ nu - P).max() <= 1e-12 * np.abs(P).max()
    assert np.abs(M[3:6] @ nu - L0).max() <= 1e-12 * max(np.abs(L0).max(), 1.0)
    assert abs(0.5 * nu @ M @ nu - E) <= 1e-12 * E
    J = FR.jacobian(m, q, pr, quat)
    assert (J[~np.broadcast_to(FR.chain_mask(m)[:, None, :], J.shape)] == 0.0).all()
    assert np.array_equal(J[0], np.hstack([np.eye(6), np.zeros((6, m.nd))]))
    # finite difference of the foot position along nu
    R, p, _ = H.forward_kinematics(m, q, pr, quat)
    eps = 1e-7
    # the root's orientation advanced by the world rotation vector w eps: q' = (w eps / 2, 1) * q
    x, y, z, s = quat
    hx, hy, hz = 0.5 * w * eps
    qn = np.array([s * hx + hy * z - hz * y + x, s * hy + hz * x - hx * z + y, s * hz + hx * y - hy * x + z, s - hx * x - hy * y - hz * z])
    qn /= np.linalg.norm(qn)
    _, p2, _ = H.forward_kinematics(m, q + eps * qd, pr + eps * v, qn)
    for b in (4, 16):
        assert np.abs((p2[b] - p[b]) / eps - (J[b] @ nu)[:3]).max() <= 1e-5


def test_torch_expressions_of_the_foot_controller_equal_float64_numpy():
    """utils.torch_utils.foot_impedance_control (float64 CPU tensors) against the NumPy closed form: with and without bias,
    clamp last, limit <= 0 = none."""
    torch = pytest.importorskip("torch")
    from shifu_amd.utils.torch_utils import foot_impedance_control
    rng = np.random.default_rng(19)
    n, F, nd = 7, 4, 12
    J = rng.normal(size=(n, F, 6, nd + 6))
    qd = rng.uniform(-2, 2, (n, nd))
    rp, fp, tg = rng.normal(size=(n, 3)), rng.normal(size=(n, F, 3)), rng.normal(size=(n, F, 3))
    rq = rng.normal(size=(n, 4))
    rq /= np.linalg.norm(rq, axis=1, keepdims=True)
    kp3, kd3 = rng.uniform(50, 400, 3), rng.uniform(5, 40, 3)
    bias = rng.normal(size=(n, nd + 6))
    T = lambda x: None if x is None else torch.from_numpy(np.asarray(x, np.float64))
    for b in (None, bias):
        free, _ = FR.foot_impedance(J, qd, rp, rq, fp, tg, kp3, kd3, b)
        lim = np.abs(free).min(0) * 0.5
        lim[0], lim[2] = 0.0, -3.0
        _, want = FR.foot_impedance(J, qd, rp, rq, fp, tg, kp3, kd3, b, lim)
        got = foot_impedance_control(T(J), T(qd), T(rp), T(rq), T(fp), T(tg), T(kp3), T(kd3), T(b), T(lim)).numpy()
        assert np.abs(got - want).max() <= 1e-9 * np.abs(free).max()
        assert np.allclose(got[:, [0, 2]], free[:, [0, 2]], rtol=1e-9) and (np.abs(got[:, 1]) <= lim[1] * (1 + 1e-12)).all()
        got = foot_impedance_control(T(J), T(qd), T(rp), T(rq), T(fp), T(tg), T(kp3), T(kd3), T(b)).numpy()
        assert np.abs(got - free).max() <= 1e-9 * np.abs(free).max()
    z3 = np.zeros(3)
    got = foot_impedance_control(T(J), T(qd), T(rp), T(rq), T(fp), T(tg), T(z3), T(z3), T(bias)).numpy()
    assert np.array_equal(got, bias[:, 6:])
