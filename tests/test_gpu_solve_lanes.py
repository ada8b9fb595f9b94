"""Who does what in the contact solve's impulse passes (csrc/shf_chain_hard.h, chain_hard_apply) when the constraint counts move.

The fused KC = 8 step runs the two impulse sets of a sub-step side by side -- the position impulses on lanes 0-15 of an env, the
velocity impulses on lanes 16-31 -- when there are velocity iterations, and the position impulses alone on lanes 0-15 when there
are none.  Which body lane gathers which constraint, and how many there are, depends on the env's constraint count K, and the two
envs of a wavefront need not agree on it.  The cases below hold the fused A1 step to the oracle bit for bit while K of the two envs
of wavefront 0 runs through 5, 6, 7 and 8 and differs between them; n = 3 adds a wavefront whose second half is empty.

The initial states were picked on the CPU oracle (seed 5, _terrain(rng, 60, 70), a copy of the oracle that logs K per hard_solve):
thighs 1.2 / calves -2.4 with the trunk 0.40 m (env 0) and 0.18 m (env 1) above the env's origin, thighs 1.0 / calves -2.2 at
0.22 m for env 2.  There, in the six steps and for n = 2 and n = 3, both solvers, with one velocity iteration and with none, the two
envs of wavefront 0 offer 5, 6, 7 and 8 or more candidates each in at least one sub-step between them, offer different numbers in
23 to 26 of the 30 sub-steps (their histograms, which is all the test sees, overlap in 10 to 20 sub-steps: at least 10 differ), and
nobody resets.  The asserts on the candidate histogram below check that the inputs still do this;
they are conditions on the inputs, not tolerances."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests.test_gpu_parity import H_DEFAULT_Q, _a1_buffers, _compare, _make_sim, _need_gpu, _terrain, _upload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEED, STEPS = 5, 6
ENVS = [(0.40, 1.2, -2.4), (0.18, 1.2, -2.4), (0.22, 1.0, -2.2)]      # trunk height over the env's origin, thigh, calf


def _inputs(n, solver, vel_iters, pos_iters=8, max_contacts=8, cm=None):
    """The case's inputs, nothing on the GPU yet: the near-ground states of ENVS (reused in turn beyond the third env) on the seeded
    terrain.  tests/test_gpu_solve_settings.py runs the same states at other solver settings."""
    from shifu_amd.a1_task import a1_task_params
    rng = np.random.default_rng(SEED)
    cm = cm or H.a1_model()
    nd = cm.blob.nd
    sp = H.sim_params(angular_damping=0.5, solver=solver, max_contacts=max_contacts, vel_iters=vel_iters, pos_iters=pos_iters)
    assert sp.vel_iters == vel_iters and sp.pos_iters == pos_iters
    tp = a1_task_params(cm, num_rows=4, num_cols=5, env_length=0.8)
    terr, hs = _terrain(rng, 60, 70)
    bufs = _a1_buffers(cm, tp, n, rng, terr.rows, terr.cols)
    bufs["ep_len"][:] = 0                                    # no time-outs in six steps
    for e in range(n):
        z, thigh, calf = ENVS[e % len(ENVS)]
        q = np.array(H_DEFAULT_Q, np.float32)
        q[1::3], q[2::3] = thigh, calf
        bufs["root_state"][e, 2] = bufs["origins"][e, 2] + z
        bufs["dof_state"][e * nd:(e + 1) * nd, 0] = q
    return cm, sp, tp, terr, hs, bufs, rng


def _setup(n, solver, vel_iters, **kw):
    from shifu_amd.backend import A1Task
    cm, sp, tp, terr, hs, bufs, rng = _inputs(n, solver, vel_iters, **kw)
    sim = _make_sim(cm, sp, n, terr, hs, group="chain32")
    task = A1Task(sim, tp)
    _upload(sim, task, bufs)
    return cm, sp, tp, terr, hs, bufs, sim, task, rng


@pytest.mark.parametrize("vel_iters", [1, 0])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_impulse_passes_while_the_constraint_counts_of_a_wavefront_differ(oracle, solver, n, vel_iters):
    _need_gpu()
    cm, sp, tp, terr, hs, bufs, sim, task, rng = _setup(n, solver, vel_iters)
    assert task.kernel_symbol().startswith("_Z14k_a1_chain_%sI" % solver)
    ht = sim.bind_contact_hist(True)
    resets = 0
    for it in range(STEPS):
        raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32)
        task.step(torch.from_numpy(raw).cuda())
        oracle.a1_step(cm.blob, sp, tp, n, 0, bufs, raw, terrain=terr, heights=hs)
        _compare(sim, task, bufs, f"step {it}")
        resets += int(bufs["reset"].sum())
    # what the case is about really happened in wavefront 0: every K from 5 to 8, and the two envs apart
    bins = _abi.CONTACT_HIST_BINS
    h = ht.cpu().numpy().astype(np.int64)[:, :bins]
    assert (h.sum(1) == STEPS * 5).all()
    k = np.concatenate([h[:, :8], h[:, 8:].sum(1, keepdims=True)], axis=1)      # sub-steps by K = min(candidates, 8)
    for kk in (5, 6, 7, 8):
        assert k[0, kk] + k[1, kk] > 0, f"K = {kk} never occurs in wavefront 0: {k[0]} {k[1]}"
    # (the overlap of the two envs' histograms bounds the sub-steps in which they can have been at the same K: 10 - 20 of the
    # 30 on the oracle, so K differs in at least 10 sub-steps)
    assert STEPS * 5 - np.minimum(k[0], k[1]).sum() >= 10, f"the envs of wavefront 0 differ in K too rarely: {k[0]} {k[1]}"
    assert resets == 0 and np.isfinite(bufs["obs"]).all()
    assert np.abs(bufs["contact"]).max() > 10.0 and np.abs(bufs["dof_state"][:, 1]).max() > 0.0
    sim.bind_contact_hist(False)
