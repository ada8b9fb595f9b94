"""Host-side checks of the mass-matrix / operational-space-control feature (no GPU): the two C-ABI entries are declared, bound
and additive (SHF_ABI_VERSION stays 22), the facade's refresh is a no-op until a tensor is acquired, the library refuses what it
cannot compute, and the torch expressions of the controller (the CPU-tensor path of ArmRobot.operational_space_control) equal
a float64 NumPy evaluation of the formulas."""
import ctypes
import os
import re

import numpy as np
import pytest

from shifu_amd import _abi
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
    assert re.search(r"\bint\s+shf_sim_dynamics\s*\(\s*ShfSim\*\s*sim\s*,\s*float\*\s*mass_matrix_or_null\s*,\s*float\*\s*bias_or_null\s*,"
                     r"\s*void\*\s*stream\s*\)\s*;", hdr)
    m = re.search(r"\bint\s+shf_osc\s*\(([^;]*)\)\s*;", hdr)
    assert m and len(m.group(1).split(",")) == 20
    for name in ("j_env_stride", "mass_matrix", "bias_or_null", "dof_elem_stride", "ee_env_stride", "goal_pose", "kp6", "kd6",
                 "damping", "q_rest_or_null", "kp_null", "kd_null", "effort_limit_or_null", "efforts_out"):
        assert name in m.group(1)


def test_binding_table_covers_both_entries(lib):
    from shifu_amd import _lib
    assert "shf_sim_dynamics" in _lib.EXPORTS and "shf_osc" in _lib.EXPORTS
    assert len(_lib._SIGS["shf_sim_dynamics"][0]) == 4 and len(_lib._SIGS["shf_osc"][0]) == 20
    assert lib.shf_sim_dynamics.restype is ctypes.c_int32 and lib.shf_osc.restype is ctypes.c_int32


def test_abi_version_stays_22(lib):
    assert re.search(r"#define\s+SHF_ABI_VERSION\s+22\b", _header())
    assert _abi.SHF_ABI_VERSION == 22
    assert lib.shf_abi_version() == 22


def test_refresh_is_a_no_op_until_a_tensor_is_acquired():
    from shifu_amd.isaacgym import gymapi

    class NoBackend:
        def __getattr__(self, name):
            raise AssertionError(f"backend.{name} reached although no mass-matrix tensor was acquired")

    sim = gymapi.SimHandle(0, gymapi.SimParams())
    sim.backend = NoBackend()
    assert sim.mass_matrix is None and sim.dof_bias is None
    gymapi.acquire_gym().refresh_mass_matrix_tensors(sim)


def test_library_refuses_what_it_cannot_compute(lib):
    """Null and unfinalised sims, a floating base and two null outputs: each with a message, all decided on the host."""
    from shifu_amd.model import asset_path, compile_urdf
    buf = (ctypes.c_float * 64)()
    out = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.shf_sim_dynamics(None, out, out, None) != 0 and b"null sim" in lib.shf_last_error()
    p = H.sim_params()

    def make(model, finalize=True):
        h = ctypes.c_void_p()
        assert lib.shf_sim_create(ctypes.byref(p), ctypes.byref(h)) == 0
        assert lib.shf_model_bounds(ctypes.byref(model)) == 0
        assert lib.shf_sim_set_articulation(h, ctypes.byref(model)) == 0
        if finalize:
            assert lib.shf_sim_finalize(h, 4, 0) == 0
        return h

    arm = compile_urdf(asset_path("abb_rod.urdf"), fix_base_link=True, default_dof_drive_mode=_abi.DOF_MODE_EFFORT).blob
    h = make(arm, finalize=False)
    assert lib.shf_sim_dynamics(h, out, out, None) != 0 and b"not finalized" in lib.shf_last_error()
    lib.shf_sim_destroy(h)
    h = make(arm)
    assert lib.shf_sim_dynamics(h, None, None, None) != 0 and b"both outputs" in lib.shf_last_error()
    assert lib.shf_sim_dynamics(h, out, None, None) != 0 and b"not bound" in lib.shf_last_error()   # no state tensors here
    lib.shf_sim_destroy(h)
    h = make(H.a1_model().blob)
    assert lib.shf_sim_dynamics(h, out, out, None) != 0 and b"fixed base" in lib.shf_last_error()
    lib.shf_sim_destroy(h)
    # shf_osc: null tensors and too many dofs
    assert lib.shf_osc(None, 0, None, None, None, 2, None, 0, None, None, None, 0.0, None, 0.0, 0.0, None, 1, 6, None, None) != 0
    assert b"shf_osc" in lib.shf_last_error()
    assert lib.shf_osc(out, 36, out, None, out, 2, out, 7, out, out, out, 0.0, None, 0.0, 0.0, None, 1, _abi.MAX_DOFS + 1, out, None) != 0
    assert b"too many dofs" in lib.shf_last_error()


def _quat_mul(a, b):
    x1, y1, z1, w1 = a.T
    x2, y2, z2, w2 = b.T
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], 1)


@pytest.mark.parametrize("nd,posture", [(6, False), (7, False), (7, True), (6, True)])
def test_torch_expressions_equal_float64_numpy(nd, posture):
    """utils.torch_utils.operational_space_control (float64 CPU tensors) against NumPy: e, a = kp e - kd J qd, X = M^-1 J^T,
    A = sym(J X) + damping^2 I, tau = J^T A^-1 a [+ M u - J^T A^-1 J u] + bias, clamp last, limit <= 0 = none.  With 6 dofs
    q_rest is ignored (no null space)."""
    torch = pytest.importorskip("torch")
    from shifu_amd.utils.torch_utils import operational_space_control
    rng = np.random.default_rng(7 + nd)
    n = 9
    J = rng.normal(size=(n, 6, nd))
    L = rng.normal(size=(n, nd, nd))
    M = L @ L.transpose(0, 2, 1) + 0.5 * np.eye(nd)
    q, qd = rng.uniform(-2, 2, (n, nd)), rng.uniform(-1, 1, (n, nd))
    ee, goal = rng.normal(size=(n, 7)), rng.normal(size=(n, 7))
    ee[:, 3:] /= np.linalg.norm(ee[:, 3:], axis=1, keepdims=True)
    goal[:, 3:] /= np.linalg.norm(goal[:, 3:], axis=1, keepdims=True)
    kp6, kd6 = rng.uniform(50, 200, 6), rng.uniform(5, 30, 6)
    bias = rng.normal(size=(n, nd))
    q_rest = rng.uniform(-4, 4, nd) if posture else None
    damping, kpn, kdn = 0.05, 10.0, 6.0
    # float64 NumPy
    qr = _quat_mul(goal[:, 3:], ee[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0]))
    e = np.concatenate([goal[:, :3] - ee[:, :3], qr[:, :3] * np.sign(qr[:, 3:4])], 1)
    want = np.zeros((n, nd))
    for k in range(n):
        a = kp6 * e[k] - kd6 * (J[k] @ qd[k])
        A = J[k] @ np.linalg.solve(M[k], J[k].T)
        A = 0.5 * (A + A.T) + damping ** 2 * np.eye(6)
        t = J[k].T @ np.linalg.solve(A, a)
        if posture and nd > 6:
            d = q_rest - q[k]
            u = kpn * (d - 2 * np.pi * np.round(d / (2 * np.pi))) - kdn * qd[k]
            t += M[k] @ u - J[k].T @ np.linalg.solve(A, J[k] @ u)
        want[k] = t + bias[k]
    free = want.copy()
    lim = np.abs(want).min(0) * 0.5
    lim[0], lim[2] = 0.0, -3.0
    want = np.where(lim > 0, np.clip(want, -np.abs(lim), np.abs(lim)), want)
    T = lambda x: None if x is None else torch.from_numpy(np.asarray(x, np.float64))
    got = operational_space_control(T(J), T(M), T(q), T(qd), T(ee[:, :3]), T(ee[:, 3:]), T(goal[:, :3]), T(goal[:, 3:]), T(kp6),
                                    T(kd6), damping, T(bias), T(q_rest), kpn, kdn, T(lim)).numpy()
    assert np.abs(got - want).max() <= 1e-9 * np.abs(free).max()
    assert np.array_equal(got[:, [0, 2]] != 0, np.ones((n, 2), bool)) and np.allclose(got[:, [0, 2]], free[:, [0, 2]], rtol=1e-9)
    if posture and nd > 6:
        plain = operational_space_control(T(J), T(M), T(q), T(qd), T(ee[:, :3]), T(ee[:, 3:]), T(goal[:, :3]), T(goal[:, 3:]),
                                          T(kp6), T(kd6), damping, T(bias)).numpy()
        assert np.abs(plain - free).max() > 1e-3, "the posture term must change the efforts"
