"""The KC = 8 contact sweep when the two envs of a wavefront want different things (csrc/shf_chain_hard.h, visit8).

A visit runs when contact c of either env of the wavefront is active; the env whose contact is not takes nothing from it (its
velocities stay bit for bit), the mask of loaded contacts is taken once per sweep, and the sliding step is computed by every lane of
a wavefront in which one contact slides.  The cases below put a robot that starts folded on the ground (trunk low, more candidate
contacts than the solve holds) next to one that starts in the air (none, or a few when it lands) in ONE wavefront, and hold the fused
A1 step to the oracle bit for bit: n = 2 is a full wavefront, n = 3 adds one whose second half is empty.

The initial states were picked on the CPU oracle (seed 5, trunk 0.10 m / 0.42 m above the env's origin, thigh 1.0 / calf -2.2 for
the folded robot): there the folded robots drop contacts at the cap of 8 in the six steps on both terrains and under both solvers, the
high robot meets the rough terrain in steps 5 and 6 and never the flat one, and nobody resets.  _a1_setup of test_gpu_parity.py
fixes an 80 x 60 terrain, so the set-up is spelled out here from the same pieces, on _terrain(rng, 60, 70)."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests.test_gpu_parity import H_DEFAULT_Q, _a1_buffers, _compare, _make_sim, _need_gpu, _terrain, _upload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, STEPS, Z_LOW, Z_HIGH, FOLD = 5, 6, 0.10, 0.42, (1.0, -2.2)


def _setup(n, rough, solver, friction):
    from shifu_amd.a1_task import a1_task_params
    from shifu_amd.backend import A1Task
    rng = np.random.default_rng(SEED)
    cm = H.a1_model()
    nd = cm.blob.nd
    sp = H.sim_params(angular_damping=0.5, solver=solver, max_contacts=8)
    tp = a1_task_params(cm, num_rows=4, num_cols=5, env_length=0.8)
    terr, hs = _terrain(rng, 60, 70, rough=rough)
    bufs = _a1_buffers(cm, tp, n, rng, terr.rows, terr.cols)
    bufs["ep_len"][:] = 0                                    # no time-outs in six steps
    folded = np.array(H_DEFAULT_Q, np.float32)
    folded[1::3], folded[2::3] = FOLD
    for e in range(n):                                       # env 1 -- the second half of wavefront 0 -- starts in the air
        low = e != 1
        bufs["root_state"][e, 2] = bufs["origins"][e, 2] + (Z_LOW if low else Z_HIGH)
        if low:
            bufs["dof_state"][e * nd:(e + 1) * nd, 0] = folded
    if friction is not None:
        bufs["friction"][:] = [friction[e % 2] for e in range(n)]
    sim = _make_sim(cm, sp, n, terr, hs, group="chain32")
    task = A1Task(sim, tp)
    _upload(sim, task, bufs)
    return cm, sp, tp, terr, hs, bufs, sim, task, rng


def _run(oracle, n, rough, solver, friction):
    _need_gpu()
    cm, sp, tp, terr, hs, bufs, sim, task, rng = _setup(n, rough, solver, friction)
    assert task.kernel_symbol().startswith("_Z14k_a1_chain_%sI" % solver)
    ht = sim.bind_contact_hist(True)
    oracle.dropped(reset=True)
    resets = 0
    for it in range(STEPS):
        raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32)
        task.step(torch.from_numpy(raw).cuda())
        oracle.a1_step(cm.blob, sp, tp, n, 0, bufs, raw, terrain=terr, heights=hs)
        _compare(sim, task, bufs, f"step {it}")
        resets += int(bufs["reset"].sum())
    # what the case is about really happened: one env of wavefront 0 at the cap while its neighbour has next to nothing, no resets
    h = ht.cpu().numpy().astype(np.int64)
    bins = _abi.CONTACT_HIST_BINS
    assert (h[:, :bins].sum(1) == STEPS * 5).all()
    assert h[0, 8:bins].sum() > 0, f"env 0 never offers 8 candidates: {h[0]}"
    assert h[1, :3].sum() > 0, f"env 1 never has 2 candidates or fewer: {h[1]}"
    d = oracle.dropped()
    assert d > 0 and int(h[:, bins].sum()) == d              # (while the histogram is bound its last column takes the drop counts)
    assert resets == 0 and np.isfinite(bufs["obs"]).all()
    assert np.abs(bufs["contact"]).max() > 10.0 and np.abs(bufs["dof_state"][:, 1]).max() > 0.0
    sim.bind_contact_hist(False)


@pytest.mark.parametrize("rough", [False, True])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_one_env_of_a_wavefront_commits_while_the_other_does_not(oracle, solver, n, rough):
    _run(oracle, n, rough, solver, None)


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_one_env_of_a_wavefront_slides_while_the_other_sticks(oracle, solver):
    """Friction 0.05 for the even envs and 1.25 for the odd ones: the sliding step is taken for one env of a wavefront and not for
    the other (the high robot has landed on the rough terrain by step 5)."""
    _run(oracle, 3, True, solver, (0.05, 1.25))
