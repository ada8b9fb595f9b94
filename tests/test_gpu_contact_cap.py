"""The fused A1 step when BOTH envs of a wavefront overflow the contact cap, by different amounts (csrc/shf_chain_hard.h, phase P:
hard_cap_select and the drop counter) -- against the oracle bit for bit over six steps.

Envs 0 and 1 (wavefront 0) start folded on the ground at two different fold angles, so their candidate counts differ; n = 3 adds a
wavefront whose second half is empty.  The poses were picked on the CPU oracle (seed 5, trunk 0.10 m above the env's origin, hips at
the default, thigh / calf as in ENVS): each of envs 0 and 1 alone (the others lifted to 0.42 m, which changes nothing for the env
itself) drops contacts at caps of 3, 8 and 12 under both solvers, on both terrains and the trimesh, at n = 2 and at n = 3, and nobody
resets in the six steps.  The set-up is that of tests/test_gpu_sweep_gating.py, from the same pieces.

The self-collision case: hips splayed inwards by 0.8 rad (HIPS_SELF), where the calves of a side press against each other.  That a
self-contact is among the candidates of an overflowing sub-step is established on the CPU oracle inside the test: one sub-step
(oracle.step) from the initial state drops total - kmax contacts, and it drops more with the capsule pairs on than with
ShfModel.self_collide cleared (same state, same sample points: the difference is the number of self-contacts offered) while it
already overflows without them."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests.test_gpu_parity import H_DEFAULT_Q, _a1_buffers, _compare, _make_sim, _need_gpu, _terrain, _upload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, STEPS, Z_LOW = 5, 6, 0.10
ENVS = [(1.0, -2.2), (0.9, -2.0), (1.0, -2.2)]            # thigh, calf of env 0, 1, 2
HIPS_SELF = (-0.8, 0.8, -0.8, 0.8)


def _model(selfc):
    if not selfc:
        return H.a1_model()
    from shifu_amd.model import asset_path, compile_urdf
    cm = compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT, self_collision=True)
    for d in range(cm.blob.nd):
        cm.blob.damping[d] = 0.5
    return cm


def _scene(n, rough, solver, kmax, trimesh=False, selfc=False):
    """everything but the GPU objects: model, parameters, terrain (heights as the oracle takes them), buffers, action generator"""
    from shifu_amd.a1_task import a1_task_params
    rng = np.random.default_rng(SEED)
    cm = _model(selfc)
    nd = cm.blob.nd
    sp = H.sim_params(angular_damping=0.5, solver=solver, max_contacts=kmax)
    tp = a1_task_params(cm, num_rows=4, num_cols=5, env_length=0.8)
    terr, hs = _terrain(rng, 60, 70, rough=rough)
    warp, packed = None, hs
    if trimesh:
        from shifu_amd.isaacgym.terrain_utils import pack_trimesh_samples, trimesh_warp_map
        warp = trimesh_warp_map(hs, terr.hscale, terr.vscale, 0.75)
        terr.warped = 1
        packed = pack_trimesh_samples(hs, warp)
    bufs = _a1_buffers(cm, tp, n, rng, terr.rows, terr.cols)
    bufs["ep_len"][:] = 0                                    # no time-outs in six steps
    for e in range(n):
        q = np.array(H_DEFAULT_Q, np.float32)
        q[1::3], q[2::3] = ENVS[e]
        if selfc:
            q[0::3] = HIPS_SELF
        bufs["root_state"][e, 2] = bufs["origins"][e, 2] + Z_LOW
        bufs["dof_state"][e * nd:(e + 1) * nd, 0] = q
    return cm, sp, tp, terr, hs, warp, packed, bufs, rng


def _self_contacts_offered(oracle, cm, sp, bufs, terr, packed):
    """(drops with the capsule pairs, drops without) of ONE sub-step of env 0 from its initial state, on the oracle"""
    out = []
    nd = cm.blob.nd
    for on in (1, 0):
        cm.blob.self_collide = on
        dof, root = bufs["dof_state"][:nd].copy(), bufs["root_state"][:1].copy()
        oracle.dropped(reset=True)
        oracle.step(cm.blob, sp, 1, dof, root, nsteps=1, terrain=terr, heights=packed)
        out.append(oracle.dropped())
    cm.blob.self_collide = 1
    return out


def _run(oracle, n, rough, solver, kmax, trimesh=False, selfc=False):
    _need_gpu()
    from shifu_amd.backend import A1Task
    bins = _abi.CONTACT_HIST_BINS
    grown = []
    for hist in (True, False):                               # the drop counter's two homes: the histogram's last column, T_DROPPED
        cm, sp, tp, terr, hs, warp, packed, bufs, rng = _scene(n, rough, solver, kmax, trimesh, selfc)
        if selfc and hist:
            with_pairs, without = _self_contacts_offered(oracle, cm, sp, bufs, terr, packed)
            assert with_pairs > without > 0, (with_pairs, without)
        sim = _make_sim(cm, sp, n, terr, hs, group="chain32", warp=warp)
        task = A1Task(sim, tp)
        _upload(sim, task, bufs)
        want = "_Z16k_a1_chain_%s16ILb%dELb%dEE" if kmax > 8 else "_Z14k_a1_chain_%sILb%dELb%dEE"
        assert task.kernel_symbol() == want % (solver, int(trimesh), int(selfc))
        ht = sim.bind_contact_hist(True) if hist else None
        before = sim.tensors[_abi.T_DROPPED].cpu().numpy().astype(np.int64).sum()
        oracle.dropped(reset=True)
        resets = 0
        for it in range(STEPS):
            raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32)
            task.step(torch.from_numpy(raw).cuda())
            oracle.a1_step(cm.blob, sp, tp, n, 0, bufs, raw, terrain=terr, heights=packed)
            _compare(sim, task, bufs, f"step {it} (histogram {'bound' if hist else 'not bound'})")
            resets += int(bufs["reset"].sum())
        d = oracle.dropped()
        now = sim.tensors[_abi.T_DROPPED].cpu().numpy().astype(np.int64).sum()
        assert d > 0 and resets == 0 and np.isfinite(bufs["obs"]).all()
        if hist:
            h = ht.cpu().numpy().astype(np.int64)
            assert (h[:, :bins].sum(1) == STEPS * 5).all()
            for e in (0, 1):                                 # both envs of wavefront 0 exceed the cap in some sub-step
                assert h[e, kmax + 1:bins].sum() > 0, f"env {e} never offers more than {kmax} candidates: {h[e]}"
            assert h[0, bins] != h[1, bins]                  # ... by different amounts (the envs' own drop counts)
            assert int(h[:, bins].sum()) == d and now == before      # (while the histogram is bound its last column takes the drop counts)
            sim.bind_contact_hist(False)
        else:
            assert now - before == d
        grown.append(d)
        sim.destroy()
    assert grown[0] == grown[1]


@pytest.mark.parametrize("kmax", [8, 3, 12])
@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_both_envs_of_a_wavefront_overflow_the_cap(oracle, solver, n, rough, kmax):
    _run(oracle, n, rough, solver, kmax)


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_both_envs_overflow_the_cap_on_the_trimesh(oracle, solver):
    _run(oracle, 3, True, solver, 8, trimesh=True)


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_self_contacts_among_the_candidates_of_an_overflowing_sub_step(oracle, solver):
    _run(oracle, 2, False, solver, 8, selfc=True)
