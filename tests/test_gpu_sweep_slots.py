"""The KC = 8 contact sweep without its count test (csrc/shf_chain_hard.h, SLOT_COUNT; profiles/r24_sweep_slots.md).

The unrolled sweep used to stop at the first visit c >= Kw, the larger constraint count of the wavefront's two envs.  Now every
one of the eight visits reaches the skip rule, which has to turn it away by itself: no env owns a contact c >= K, so the visit's
commit mask is empty.  The cases are the ones the count test used to shield -- wavefronts whose envs hold four constraints or
fewer, so that visits 4 to 7 find W's columns uninitialised LDS and must do nothing -- each held to the oracle bit for bit after
each of six steps, under both solvers, on the flat and on the rough terrain of tests/test_gpu_sweep_gating.py:

  (a) every robot standing on its feet, n = 2 (one full wavefront) and n = 3 (one more with an empty second half);
  (b) n = 2 with max_contacts = 4 on the KC = 8 kernel, both robots folded on the ground: more candidates than the cap, K = 4;
  (c) n = 2, env 0 standing and env 1 folded with max_contacts = 8: Kw = 8 with K <= 4 beside it.

The initial states were picked on the CPU oracle (seed 5).  A standing robot has the default joint angles and starts with its
trunk 0.33 m above its env's origin on the flat terrain; on the rough one it stands on the ramp (its random cells put a dozen
sample points of a standing robot within the contact offset), at (2.2, -0.4), (2.3, 0.0), (2.1, 0.4) for envs 0, 1, 2, trunk 0.36 m
above the terrain under it.  A folded robot is test_gpu_sweep_gating's (trunk 0.10 m, thigh 1.0, calf -2.2).  What the oracle
gave, counting the contacts dropped at max_contacts (a count of 0 at a cap says that no env offered more in any sub-step):
  (a) no drop at a cap of 4 and some at a cap of 3, in all eight cases: the feet reach four candidates and nothing ever adds a
      fifth (flat: the fourth in step 6; ramp: in step 1).  Bodies in contact by the end: feet only (4, 8, 12, 16).
  (b) both envs drop in every case (alone beside a robot far up in the air: 82 and 84 in step 1 on the flat terrain, 300 and 152
      on the rough one); on the flat terrain the folded robots have pushed themselves off the ground by step 4 (PGS: 5).
  (c) env 1 drops at the cap of 8 in steps 1 to 3 at least (63 to 124 in step 1) and env 0 contributes none of the drops; env 0
      alone drops nothing at a cap of 4 and something at a cap of 3 (flat: 4 in step 6; ramp: 1 to 2 in step 1).
Nobody resets.  The tests check the same on the GPU's candidate histogram."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests.test_gpu_parity import H_DEFAULT_Q, _a1_buffers, _compare, _make_sim, _need_gpu, _terrain, _upload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, STEPS, Z_LOW, FOLD = 5, 6, 0.10, (1.0, -2.2)
Z_STAND_FLAT, Z_STAND_RAMP = 0.33, 0.36
RAMP_XY = [(2.2, -0.4), (2.3, 0.0), (2.1, 0.4)]


def _setup(oracle, n, rough, solver, kinds, max_contacts):
    """kinds[e]: 's' a standing robot, 'f' a folded one."""
    from shifu_amd.a1_task import a1_task_params
    from shifu_amd.backend import A1Task
    rng = np.random.default_rng(SEED)
    cm = H.a1_model()
    nd = cm.blob.nd
    sp = H.sim_params(angular_damping=0.5, solver=solver, max_contacts=max_contacts)
    tp = a1_task_params(cm, num_rows=4, num_cols=5, env_length=0.8)
    terr, hs = _terrain(rng, 60, 70, rough=rough)
    bufs = _a1_buffers(cm, tp, n, rng, terr.rows, terr.cols)
    bufs["ep_len"][:] = 0                                    # no time-outs in six steps
    folded = np.array(H_DEFAULT_Q, np.float32)
    folded[1::3], folded[2::3] = FOLD
    for e in range(n):
        if kinds[e] == "f":
            bufs["root_state"][e, 2] = bufs["origins"][e, 2] + Z_LOW
            bufs["dof_state"][e * nd:(e + 1) * nd, 0] = folded
        elif rough:
            x, y = RAMP_XY[e]
            h = float(np.ravel(oracle.terrain_query(terr, hs, np.array([[x, y]], np.float32))[0])[0])
            bufs["root_state"][e, :3] = [x, y, h + Z_STAND_RAMP]
        else:
            bufs["root_state"][e, 2] = bufs["origins"][e, 2] + Z_STAND_FLAT
    sim = _make_sim(cm, sp, n, terr, hs, group="chain32")
    task = A1Task(sim, tp)
    _upload(sim, task, bufs)
    return cm, sp, tp, terr, hs, bufs, sim, task, rng


def _run(oracle, n, rough, solver, kinds, max_contacts):
    """Six steps against the oracle; returns the candidate histogram (env x count, last column: drops) and the oracle's drops."""
    _need_gpu()
    cm, sp, tp, terr, hs, bufs, sim, task, rng = _setup(oracle, n, rough, solver, kinds, max_contacts)
    assert task.kernel_symbol().startswith("_Z14k_a1_chain_%sI" % solver)       # the KC = 8 kernel
    ht = sim.bind_contact_hist(True)
    oracle.dropped(reset=True)
    resets = 0
    for it in range(STEPS):
        raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32)
        task.step(torch.from_numpy(raw).cuda())
        oracle.a1_step(cm.blob, sp, tp, n, 0, bufs, raw, terrain=terr, heights=hs)
        _compare(sim, task, bufs, f"step {it}")
        resets += int(bufs["reset"].sum())
    h = ht.cpu().numpy().astype(np.int64)
    bins = _abi.CONTACT_HIST_BINS
    assert (h[:, :bins].sum(1) == STEPS * 5).all()
    d = oracle.dropped()
    assert int(h[:, bins].sum()) == d                        # (while the histogram is bound its last column takes the drop counts)
    assert resets == 0 and np.isfinite(bufs["obs"]).all()
    assert np.abs(bufs["contact"]).max() > 10.0 and np.abs(bufs["dof_state"][:, 1]).max() > 0.0
    sim.bind_contact_hist(False)
    return h, bins, d


@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_standing_robots_leave_visits_4_to_7_nothing_to_do(oracle, solver, n, rough):
    h, bins, d = _run(oracle, n, rough, solver, "s" * n, 8)
    assert d == 0 and h[:, 5:bins].sum() == 0, f"an env offered more than four candidates: {h}"
    assert h[:, 4].sum() > 0, f"no env ever stood on four candidates: {h}"
    assert (h[:, 1:5].sum(1) > 0).all(), f"an env never touched the ground: {h}"


@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_a_cap_of_four_on_the_kernel_for_eight(oracle, solver, rough):
    h, bins, d = _run(oracle, 2, rough, solver, "ff", 4)
    assert d > 0 and (h[:, bins] > 0).all(), f"an env never dropped a candidate at the cap of 4: {h}"
    assert (h[:, 5:bins].sum(1) > 0).all(), f"an env never offered more than four candidates: {h}"


@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_a_full_env_beside_one_with_four_constraints(oracle, solver, rough):
    h, bins, d = _run(oracle, 2, rough, solver, "sf", 8)
    assert d > 0 and h[1, bins] == d and h[1, 9:bins].sum() > 0, f"env 1 never offered more than eight candidates: {h}"
    assert h[0, 5:bins].sum() == 0 and h[0, 4] > 0, f"env 0 did not stand on four candidates at the most: {h}"
