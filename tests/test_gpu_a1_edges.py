"""The code around the sub-step loop of the chain-mapped fused A1 step (csrc/shf_chain.h: a1_chain_step_body, csrc/shf_task.h:
a1_post_step on compile-time dimensions) against the oracle, bit for bit: every tensor and the statistics row after each of 12
vec-steps, under TGS and PGS, at env counts and reset patterns that reach the edges' own branches --

- n = 3: a wavefront with one of its two envs missing; the block's env count in the statistics is not 8;
- n = 9: a second block with a single env; the last ticket is drawn across two blocks;
- n = 16 with resets forced in the first steps: envs 0 and 1 (one wavefront) and envs 5 and 15 (each alone in its wavefront)
  run out of episode length, so the wave-uniform reset path runs with one and with two resetting envs beside wavefronts
  without any -- the reset draws, origins, levels, command, push, history and reset_count;
- the same with another height-point table (35 points: one trip of the height scan's loop with part of the lanes idle, where
  the default's 187 take two).  num_history other than 3 is refused by shf_a1_create, so that dimension has one value;
- the random actions drawn inside the launch (the Philox rounds run between the prologue's two waits), n = 9, three steps."""
import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests import test_gpu_parity as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
STEPS = 12


def _run(oracle, cm, sp, tp, terr, hs, bufs, sim, task, rng, n, steps=STEPS, env_off=0):
    resets = np.zeros(n, np.int64)
    per_step = []
    for it in range(steps):
        raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32) * 1.5
        slot = task.step(torch.from_numpy(raw).cuda())
        oracle.a1_step(cm.blob, sp, tp, n, env_off, bufs, raw, terrain=terr, heights=hs)
        P._compare(sim, task, bufs, f"step {it}")
        np.testing.assert_array_equal(task.tensors[_abi.A1_STATS][slot].cpu().numpy(), oracle.a1_stats(tp, n, bufs["done_sums"]),
                                      err_msg=f"stats step {it}")
        resets += bufs["reset"].astype(np.int64)
        per_step.append(bufs["reset"].astype(bool).copy())
    assert np.isfinite(bufs["obs"]).all()
    return resets, per_step


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
@pytest.mark.parametrize("n", [3, 9])
def test_ragged_blocks_match_oracle_after_every_step(oracle, n, solver):
    P._need_gpu()
    cm, sp, tp, terr, hs, bufs, sim, task, rng = P._a1_setup(n, True, seed=40 + n, group="chain32", solver=solver)
    assert task.kernel_symbol().startswith("_Z14k_a1_chain_" + solver + "I")
    _run(oracle, cm, sp, tp, terr, hs, bufs, sim, task, rng, n)


def _setup_with_points(n, xs, ys, seed, solver):
    """_a1_setup of tests/test_gpu_parity.py with another height-point table."""
    from shifu_amd.a1_task import a1_task_params, height_points
    from shifu_amd.backend import A1Task
    rng = np.random.default_rng(seed)
    cm = H.a1_model()
    sp = H.sim_params(angular_damping=0.5, solver=solver)
    pts = height_points(xs, ys)
    tp = a1_task_params(cm, num_rows=4, num_cols=5, env_length=0.8, num_height_points=len(pts))
    terr, hs = P._terrain(rng, rows=80, cols=60, rough=True)
    bufs = P._a1_buffers(cm, tp, n, rng, terr.rows, terr.cols)
    bufs["hpoints"] = pts
    sim = P._make_sim(cm, sp, n, terr, hs, group="chain32")
    task = A1Task(sim, tp)
    return cm, sp, tp, terr, hs, bufs, sim, task, rng


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
@pytest.mark.parametrize("points", [187, 35])
def test_forced_resets_match_oracle_after_every_step(oracle, points, solver):
    P._need_gpu()
    n, forced = 16, [0, 1, 5, 15]
    if points == 187:
        cm, sp, tp, terr, hs, bufs, sim, task, rng = P._a1_setup(n, True, seed=61, group="chain32", solver=solver)
    else:
        xs, ys = [-0.6, -0.4, -0.2, 0.0, 0.2, 0.4, 0.6], [-0.4, -0.2, 0.0, 0.2, 0.4]
        cm, sp, tp, terr, hs, bufs, sim, task, rng = _setup_with_points(n, xs, ys, 61, solver)
    assert tp.num_height_points == points and bufs["hpoints"].shape == (points, 2) and bufs["obs"].shape[1] == 12 + 24 + 36 + points
    # the forced envs time out at the first step; the others a long way from it
    bufs["ep_len"][:] = 10 + np.arange(n)
    bufs["ep_len"][forced] = int(tp.max_episode_length)
    bufs["history"][:] = rng.uniform(-1, 1, bufs["history"].shape).astype(np.float32)      # a reset has something to clear
    P._upload(sim, task, bufs)
    before = {k: bufs[k].copy() for k in ("command", "push", "origins", "levels")}
    resets, per_step = _run(oracle, cm, sp, tp, terr, hs, bufs, sim, task, rng, n)
    assert (resets[forced] >= 1).all(), resets
    first = per_step[0].reshape(n // 2, 2).sum(1)        # resetting envs per wavefront (two envs each) at the first step
    assert (first == 1).any() and (first == 2).any(), first
    assert per_step[0][forced].all() and (bufs["reset_count"][forced] >= 1).all()
    for k in ("command", "push"):
        assert not np.array_equal(before[k][forced], bufs[k][forced]), k


@pytest.mark.parametrize("solver", ["tgs", "pgs"])
def test_random_actions_inside_the_launch_match_oracle(oracle, solver):
    P._need_gpu()
    n, off = 9, 4096
    cm, sp, tp, terr, hs, bufs, sim, task, rng = P._a1_setup(n, True, seed=77, group="chain32", env_off=off, solver=solver)
    for it in range(3):
        step = task.step_index
        slot = task.step_random()
        raw = oracle.random_actions(tp.seed, n, off, step, cm.blob.nd)
        assert (np.abs(raw) <= 1).all() and len(np.unique(raw)) > 0.9 * raw.size
        oracle.a1_step(cm.blob, sp, tp, n, off, bufs, raw, terrain=terr, heights=hs)
        P._compare(sim, task, bufs, f"random step {it}")
        np.testing.assert_array_equal(task.tensors[_abi.A1_STATS][slot].cpu().numpy(), oracle.a1_stats(tp, n, bufs["done_sums"]),
                                      err_msg=f"stats random step {it}")
