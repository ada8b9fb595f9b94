"""The velocity-level contact solve's run-time settings -- pos_iters, vel_iters, max_contacts -- away from the reference's 8 + 1 / 8,
on every kernel form the solve is compiled in, under both solvers, bit for bit against the oracle (every tensor, the contact tensor
included), each case on the kernel it names:

  fused A1 step, chain mapping at 32 lanes    k_a1_chain_{pgs,tgs} and, above eight constraints per env, k_a1_chain_{pgs,tgs}16
  gym.simulate on the A1 (the hook path)      k_sim_step_chain_{pgs,tgs} and ..16
  gym.simulate on the 13-body A1              k_sim_step<32, false, SELF, false, true>: the body-per-lane solve without box actors
  gym.simulate on the ABB scene               k_sim_step<32, true, false, false, true> (rod only), k_sim_step_ws_hard (split), and with
                                              link contacts what the plan picks: k_sim_step_pgs_wide<false> (sixteen envs of the
                                              shipped scene fit a CU's LDS and two workgroups of eight do not, at any env count, so
                                              k_sim_step<32, true, false, true, true> is never this scene's kernel)
  fused ABB step                              k_abb_step_ws_hard (split), k_abb_step_pgs_wide (body, link contacts), the
                                              run-time-shaped k_abb_step<32, DynDims, DynScene, false, 0, true> (body, rod only)

SETTINGS are (pos_iters, vel_iters, max_contacts): one position iteration; three, which under TGS makes the sub-iteration's
1 / pos_iters no power of two; no velocity iterations (one impulse set through the tree, and under TGS the MEAN of the
sub-iterations' impulses, which is then also the set the contact tensor reports -- tests/test_contact_force_law.py); more than one;
caps of 1, 3 and 5 constraints, below what some env offers (_offer_conditions); on the sixteen-constraint forms 12 and 16, with an
env that keeps more than eight.  The env counts are the
smallest with a tail: nine envs for the kernels with eight envs per workgroup (a full workgroup and a wavefront with an empty half),
seventeen for those with sixteen.

Each case first runs the oracle alone and checks the conditions on its inputs (constraints were active; with no velocity
iterations under TGS, one velocity iteration on the same states would have reported other forces: the setting was live), then holds
the kernel to it.

The solve has two families of code: the chain-mapped one (csrc/shf_chain_hard.h: the fused A1 step and the hook path's A1 sub-step)
and the body-per-lane one (csrc/shf_hard.h: the generic k_sim_step forms, and every ABB kernel -- k_sim_step_ws_hard and
k_abb_step_ws_hard regroup at 32 lanes per env and run substep_hard_finish of that file, as the run-time-shaped kernels do).  No
robot has a kernel in both, so no case can run the two families on the same states: each is compared with the oracle on its own
robot, at (8, 0, 8) under TGS among the rest -- the chain family on the 17-body A1, the body-per-lane family on the 13-body A1 and
the ABB scene -- and the oracle is what holds them to one rule."""
import copy

import numpy as np
import pytest

from shifu_amd import _abi
from tests import helpers as H
from tests.test_gpu_parity import (_ABB_SIM_T, _ABB_T, _compare, _make_sim, _need_gpu, _random_states, _scene_on_gpu, _terrain,
                                   _upload)
from tests.test_gpu_solve_lanes import STEPS, _inputs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SETTINGS = [(1, 0, 8), (3, 0, 5), (8, 0, 8), (2, 2, 3), (8, 1, 1)]
SETTINGS16 = SETTINGS + [(3, 0, 12), (8, 0, 16)]          # the forms that hold up to sixteen constraints per env
SOLVERS = ["pgs", "tgs"]
# (self-collision, setting) of the chain forms: every setting without, and compiled with the A1's self-collision pairs (constraints
# with a body of the tree on either side) the two settings without velocity iterations that differ in form
CHAIN_CASES = [(False, s) for s in SETTINGS16] + [(True, (8, 0, 8)), (True, (3, 0, 12))]


def _ids(settings):
    return ["%d-%d-k%d" % s for s in settings]


def _chain_ids():
    return [("self-" if c else "") + i for (c, _), i in zip(CHAIN_CASES, _ids([s for _, s in CHAIN_CASES]))]


def _kw(solver, setting):
    return dict(solver=solver, pos_iters=setting[0], vel_iters=setting[1], max_contacts=setting[2])


def _with_one_velocity_iteration(sp):
    sp1 = copy.deepcopy(sp)
    sp1.vel_iters = 1
    return sp1


def _live(solver, setting):
    """Whether the case also has to show that dropping the velocity iteration changed the forces reported."""
    return solver == "tgs" and setting[1] == 0


def _chain_symbol(stem, solver, kmax, selfc, trimesh=False):
    name = stem + solver + ("16" if kmax > 8 else "")
    return "_Z%d%sILb%dELb%dEE" % (len(name), name, int(trimesh), int(selfc))


def _excess(oracle, one_substep, sp, lo, hi):
    """Candidate constraints, summed over the envs, above a cap of `lo` and not above a cap of `hi`, at the state one_substep(params)
    steps a copy of: what the oracle drops at the one cap less what it drops at the other.  The candidates are found before the
    solve, so both caps see the same ones, and drops at the other per-env limits (self and link contacts) cancel."""
    drops = []
    for k in (lo, hi):
        spk = copy.deepcopy(sp)
        spk.max_contacts = k
        oracle.dropped(reset=True)
        one_substep(spk)
        drops.append(oracle.dropped(reset=True))
    return drops[0] - drops[1]


def _offered(oracle, one_substep, sp):
    """(candidates above the case's cap, constraints kept beyond the eighth) at that state."""
    k = int(sp.max_contacts)
    return np.array([_excess(oracle, one_substep, sp, k, 16) if k < 16 else 0, _excess(oracle, one_substep, sp, 8, k) if k > 8 else 0])


def _offer_conditions(setting, offered):
    """Conditions on the inputs: a cap below eight was below what some env offered, and a cap above eight was used beyond the
    eighth constraint (else the sixteen-constraint form runs as the eight-constraint one does)."""
    if setting[2] < 8:
        assert offered[0] > 0, f"no env offered more candidates than the cap of {setting[2]}"
    if setting[2] > 8:
        assert offered[1] > 0, "no env kept more than eight constraints"


# ----------------------------------------------------------------------------------------------------- the fused A1 step --
def _a1_oracle_run(oracle, n, solver, setting, cm=None):
    """The oracle's side of the fused A1 case: the inputs, and per vec-step the actions and every buffer after the step."""
    cm, sp, tp, terr, hs, bufs, rng = _inputs(n, solver, setting[1], pos_iters=setting[0], max_contacts=setting[2], cm=cm)
    start = copy.deepcopy(bufs)
    sp1, steps, differs, fmax = _with_one_velocity_iteration(sp), [], False, 0.0
    offered = np.zeros(2, np.int64)
    for it in range(STEPS):
        raw = (2 * rng.random((n, cm.blob.nd)) - 1).astype(np.float32)
        # (the cap against the candidates of the state the vec-step starts from: its first sub-step)
        offered += _offered(oracle, lambda s: oracle.step(cm.blob, s, n, bufs["dof_state"].copy(), bufs["root_state"].copy(), terrain=terr,
                                                          heights=hs, friction=bufs["friction"]), sp)
        if _live(solver, setting):
            alt = copy.deepcopy(bufs)
            oracle.a1_step(cm.blob, sp1, tp, n, 0, alt, raw, terrain=terr, heights=hs)
        oracle.a1_step(cm.blob, sp, tp, n, 0, bufs, raw, terrain=terr, heights=hs)
        if _live(solver, setting):
            differs |= not np.array_equal(alt["contact"], bufs["contact"])
        fmax = max(fmax, float(np.abs(bufs["contact"]).max()))
        steps.append((raw, copy.deepcopy(bufs)))
    return cm, sp, tp, terr, hs, start, steps, differs, fmax, offered


def _a1_conditions(solver, setting, steps, differs, fmax, offered):
    _offer_conditions(setting, offered)
    assert fmax > 10.0, f"no foot carried 10 N in any step: {fmax}"
    assert np.isfinite(steps[-1][1]["obs"]).all()
    if _live(solver, setting):
        assert differs, "one velocity iteration on the same states reports the same forces: vel_iters = 0 was not live"


@pytest.mark.parametrize("selfc,setting", CHAIN_CASES, ids=_chain_ids())
@pytest.mark.parametrize("solver", SOLVERS)
def test_fused_a1_step_at_other_solver_settings(oracle, solver, selfc, setting):
    """k_a1_chain_{pgs,tgs} and the ..16 forms: nine envs (a full workgroup of eight and a wavefront with an empty half), six
    vec-steps from the near-ground states of tests/test_gpu_solve_lanes.py on the seeded terrain.  At (8, 0, 8) and (3, 0, 12) also
    the forms compiled with self-collision: from these crouching states no pair of the A1 comes within the contact offset (the
    oracle's run is the one without the pairs), so those cases hold the SELF forms' candidate pass and layout at these settings and
    no pair constraint; pairs that close are in the hook path's cases below."""
    _need_gpu()
    from shifu_amd.backend import A1Task
    n = 9
    cm, sp, tp, terr, hs, start, steps, differs, fmax, offered = _a1_oracle_run(oracle, n, solver, setting,
                                                                                cm=H.a1_model(self_collision=True) if selfc else None)
    _a1_conditions(solver, setting, steps, differs, fmax, offered)
    sim = _make_sim(cm, sp, n, terr, hs, group="chain32")
    task = A1Task(sim, tp)
    _upload(sim, task, start)
    assert task.kernel_symbol() == _chain_symbol("k_a1_chain_", solver, setting[2], selfc)
    for it, (raw, want) in enumerate(steps):
        task.step(torch.from_numpy(raw).cuda())
        _compare(sim, task, want, f"step {it}")
    sim.destroy()


# --------------------------------------------------------------------------- gym.simulate on an articulation without boxes --
def _thrown_oracle_run(oracle, cm, n, solver, setting, seed, push, substeps=30):
    """Thrown, folded states on rough terrain with random efforts (and pushes on the trunk): the recipe of
    tests/test_gpu_parity.py::test_velocity_level_solve_simulate_and_self_collision_match_oracle_bitwise."""
    m = cm.blob
    for d in range(m.nd):
        m.damping[d] = 0.5
    rng = np.random.default_rng(seed)
    sp = H.sim_params(angular_damping=0.5, **_kw(solver, setting))
    terr, hs = _terrain(rng, rough=True)
    dof, root = _random_states(m, n, rng, z_lo=0.1, z_hi=0.5)
    lo, up = np.array(m.lower[:m.nd]), np.array(m.upper[:m.nd])
    dof[:, 0] = rng.uniform(lo, up, (n, m.nd)).astype(np.float32).reshape(-1)
    dof[:, 1] = rng.uniform(-6, 6, n * m.nd)
    fr = rng.uniform(0.5, 1.25, n).astype(np.float32)
    start = (dof.copy(), root.copy())
    sp1, steps, differs, fmax = _with_one_velocity_iteration(sp), [], False, 0.0
    offered = np.zeros(2, np.int64)
    for it in range(substeps):
        eff = rng.uniform(-25, 25, n * m.nd).astype(np.float32)
        force = None
        if push:
            force = np.zeros((n * m.nb, 3), np.float32)
            force[::m.nb] = rng.uniform(-20, 20, (n, 3))
        kw = dict(effort=eff, friction=fr, body_force=force, terrain=terr, heights=hs, want_contact=True, want_body_state=True)
        offered += _offered(oracle, lambda s: oracle.step(m, s, n, dof.copy(), root.copy(), **kw), sp)
        if _live(solver, setting):
            alt, _ = oracle.step(m, sp1, n, dof.copy(), root.copy(), **kw)
        contact, bstate = oracle.step(m, sp, n, dof, root, **kw)
        if _live(solver, setting):
            differs |= not np.array_equal(alt, contact)
        fmax = max(fmax, float(np.abs(contact).max()))
        steps.append((eff, force, dof.copy(), root.copy(), contact.copy(), bstate.copy()))
    return sp, terr, hs, fr, start, steps, differs, fmax, offered


def _thrown_conditions(solver, setting, steps, differs, fmax, offered):
    _offer_conditions(setting, offered)
    assert fmax > 10.0, f"no body carried 10 N in any sub-step: {fmax}"
    assert np.isfinite(steps[-1][3]).all() and np.isfinite(steps[-1][2]).all()
    if _live(solver, setting):
        assert differs, "one velocity iteration on the same states reports the same forces: vel_iters = 0 was not live"


def _thrown_on_gpu(cm, n, sp, terr, hs, fr, start, steps, symbol):
    sim = _make_sim(cm, sp, n, terr, hs, group=32)
    assert sim.kernel_symbol() == symbol, sim.kernel_symbol()
    T = sim.tensors
    T[_abi.T_SIM_DOF].copy_(torch.from_numpy(start[0]))
    T[_abi.T_SIM_ROOT].copy_(torch.from_numpy(start[1]))
    T[_abi.T_FRICTION].copy_(torch.from_numpy(fr))
    for it, (eff, force, dof, root, contact, bstate) in enumerate(steps):
        sim.set_dof_command(_abi.T_EFFORT, torch.from_numpy(eff).cuda())
        if force is not None:
            sim.apply_body_force(torch.from_numpy(force).cuda())
        sim.step()
        sim.refresh(_abi.REFRESH_ALL)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(T[_abi.T_DOF_STATE].cpu().numpy(), dof, err_msg=f"dof sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_ROOT_STATE].cpu().numpy(), root, err_msg=f"root sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_CONTACT].cpu().numpy(), contact, err_msg=f"contact sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_BODY_STATE].cpu().numpy(), bstate, err_msg=f"body sub-step {it}")
    sim.destroy()


def _pairs_closed(oracle, model, n, solver, setting, seed, push, steps):
    """Condition on the inputs of a self-collision case: without the pairs the oracle's run goes another way, so constraints between
    two bodies of the tree were among the kept ones."""
    other = _thrown_oracle_run(oracle, model(False), n, solver, setting, seed, push)[5]
    return any(not np.array_equal(a[2], b[2]) for a, b in zip(steps, other))


def _hook_a1_model(selfc):
    from shifu_amd.model import asset_path, compile_urdf
    return compile_urdf(asset_path("a1.urdf"), default_dof_drive_mode=_abi.DOF_MODE_EFFORT, self_collision=selfc)


def _a1_13_model(selfc):
    from shifu_amd.model import asset_path, compile_urdf
    cm = compile_urdf(asset_path("a1.urdf"), honour_dont_collapse=False, default_dof_drive_mode=_abi.DOF_MODE_EFFORT, self_collision=selfc)
    assert cm.blob.nb == 13
    return cm


@pytest.mark.parametrize("selfc,setting", CHAIN_CASES, ids=_chain_ids())
@pytest.mark.parametrize("solver", SOLVERS)
def test_hook_path_a1_at_other_solver_settings(oracle, solver, selfc, setting):
    """k_sim_step_chain_{pgs,tgs} and the ..16 forms (gym.simulate on the A1): nine envs, thirty sub-steps from thrown, folded
    states with random efforts and pushes; with self-collision at (8, 0, 8) and (3, 0, 12), where pairs of the folded legs close."""
    _need_gpu()
    n, cm = 9, _hook_a1_model(selfc)
    sp, terr, hs, fr, start, steps, differs, fmax, offered = _thrown_oracle_run(oracle, cm, n, solver, setting, 33, push=True)
    _thrown_conditions(solver, setting, steps, differs, fmax, offered)
    assert not selfc or _pairs_closed(oracle, _hook_a1_model, n, solver, setting, 33, True, steps), "no self-collision pair closed"
    _thrown_on_gpu(cm, n, sp, terr, hs, fr, start, steps, _chain_symbol("k_sim_step_chain_", solver, setting[2], selfc))


@pytest.mark.parametrize("setting", SETTINGS, ids=_ids(SETTINGS))
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("selfc", [False, True], ids=["", "self"])
def test_generic_articulation_at_other_solver_settings(oracle, selfc, solver, setting):
    """k_sim_step<32, false, SELF, false, true>, the body-per-lane solve without box actors (csrc/shf_hard.h), on the 13-body A1
    (feet merged into the shanks: not the chain kernels' shape) -- under PGS and, which no test did at any setting, under TGS."""
    _need_gpu()
    n, cm = 9, _a1_13_model(selfc)
    sp, terr, hs, fr, start, steps, differs, fmax, offered = _thrown_oracle_run(oracle, cm, n, solver, setting, 34, push=False)
    _thrown_conditions(solver, setting, steps, differs, fmax, offered)
    assert not selfc or _pairs_closed(oracle, _a1_13_model, n, solver, setting, 34, False, steps), "no self-collision pair closed"
    _thrown_on_gpu(cm, n, sp, terr, hs, fr, start, steps, "_Z10k_sim_stepILi32ELb0ELb%dELb0ELb1ELb0EE" % int(selfc))


# ------------------------------------------------------------------------------------------- gym.simulate on the ABB scene --
SUBSTEPS_ABB = 60
# step kernel -> (link contacts, split mapping, envs: a tail behind the workgroup's 8 or 16 envs, kernel)
ABB_SCENE_FORMS = {"body": (False, False, 9, "_Z10k_sim_stepILi32ELb1ELb0ELb0ELb1ELb0EE"),
                   "split": (False, True, 17, "_Z18k_sim_step_ws_hardILb0EE"),
                   "body-link": (True, False, 17, "_Z19k_sim_step_pgs_wideILb0EE"),
                   "split-link": (True, True, 17, "_Z18k_sim_step_ws_hardILb1EE")}


def _abb_scene_oracle_run(oracle, link, n, solver, setting, seed=19):
    """The blind joint ramp of tests/test_gpu_parity.py::test_abb_scene_under_the_velocity_level_solve_matches_oracle_bitwise, which
    presses rod and links onto cube and table.  (Seed 19, not that test's 17: at one constraint per env the table's hold on the cube
    is most often the one kept, and from seed 17's poses the rod-only scene under PGS keeps no constraint of the arm in sixty
    sub-steps -- `touched` below fails on the oracle alone.  Seeds 19, 21 and 22 meet every condition at every setting.)"""
    from shifu_amd.abb_task import ABB_BASE_POS, ABB_DEFAULT_DOF_POS, abb_boxes, abb_model
    rng = np.random.default_rng(seed)
    cm = abb_model(link_contacts=link)
    m = cm.blob
    sp = H.sim_params(dt=0.02, angular_damping=0.5, **_kw(solver, setting))
    boxes = abb_boxes()
    A, B = 4, m.nb + 3
    dof = np.zeros((n * m.nd, 2), np.float32)
    root = np.zeros((n * A, 13), np.float32)
    root[:, 6] = 1.0
    for k, b in enumerate(boxes):
        root[1 + k::A, :3] = b.pos
    dof[:, 0] = np.tile(np.array(ABB_DEFAULT_DOF_POS, np.float32), n) + rng.uniform(-0.05, 0.05, n * m.nd)
    root[0::A, :3] = ABB_BASE_POS
    root[2::A, :3] = np.stack([rng.uniform(0.03, 0.08, n), rng.uniform(-0.03, 0.03, n), rng.uniform(0.125, 0.14, n)], 1)
    yaw = rng.uniform(-np.pi, np.pi, n)
    root[2::A, 5], root[2::A, 6] = np.sin(yaw / 2), np.cos(yaw / 2)
    start = (dof.copy(), root.copy())
    fr = np.ones(n, np.float32)
    sp1, steps, differs, fmax = _with_one_velocity_iteration(sp), [], False, 0.0
    touched = cube_held = False
    dropped, offered = 0, np.zeros(2, np.int64)
    oracle.dropped(reset=True)
    for it in range(SUBSTEPS_ABB):
        if it % 6 == 0:
            tgt = dof[:, 0].copy()
            tgt[1::m.nd] += 0.02
            tgt[2::m.nd] -= 0.01
        offered += _offered(oracle, lambda s: oracle.scene_step(m, s, boxes, n, dof.copy(), root.copy(), pos_target=tgt, friction=fr), sp)
        if _live(solver, setting):
            alt = oracle.scene_step(m, sp1, boxes, n, dof.copy(), root.copy(), pos_target=tgt, friction=fr)[0]
            oracle.dropped(reset=True)      # (what the side run dropped is not the case's)
        contact, bstate, jac = oracle.scene_step(m, sp, boxes, n, dof, root, pos_target=tgt, friction=fr, want_jacobian=True)
        dropped += oracle.dropped(reset=True)
        if _live(solver, setting):
            differs |= not np.array_equal(alt, contact)
        c = contact.reshape(n, B, 3)
        assert np.isfinite(c).all() and np.isfinite(dof).all(), f"sub-step {it}"
        touched |= bool(np.abs(c[:, :m.nb]).sum() > 0)
        cube_held |= bool((np.abs(c[:, m.nb + 1, 2] - 0.981) < 0.05).mean() > 0.5)
        fmax = max(fmax, float(np.abs(contact).max()))
        steps.append((tgt.copy(), dof.copy(), root.copy(), contact.copy(), bstate.copy()))
    assert touched, "the arm met a cube / the table"
    assert cube_held, "the table carries the cubes' weight"
    assert fmax > 0.9, fmax              # (a cube weighs 0.981 N)
    _offer_conditions(setting, offered)
    if _live(solver, setting):
        assert differs, "one velocity iteration on the same states reports the same forces: vel_iters = 0 was not live"
    return cm, sp, boxes, start, steps, dropped


def _abb_scene_on_gpu(cm, sp, boxes, n, start, steps, dropped, split, symbol):
    from shifu_amd._lib import lib
    sim, _, _ = _scene_on_gpu(cm, sp, boxes, [b.pos for b in boxes], n, 32)
    assert lib().shf_sim_step_split_supported(sim._h) == 1
    assert sim.use_split_step() if split else sim.mapping == "body"
    assert sim.kernel_symbol() == symbol, sim.kernel_symbol()
    T = sim.tensors
    T[_abi.T_SIM_DOF].copy_(torch.from_numpy(start[0]))
    T[_abi.T_SIM_ROOT].copy_(torch.from_numpy(start[1]))
    for it, (tgt, dof, root, contact, bstate) in enumerate(steps):
        sim.set_dof_command(_abi.T_POS_TARGET, torch.from_numpy(tgt).cuda())
        sim.step()
        sim.refresh(_abi.REFRESH_ALL)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(T[_abi.T_DOF_STATE].cpu().numpy(), dof, err_msg=f"{symbol} dof sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_ROOT_STATE].cpu().numpy(), root, err_msg=f"{symbol} root sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_CONTACT].cpu().numpy(), contact, err_msg=f"{symbol} contact sub-step {it}")
        np.testing.assert_array_equal(T[_abi.T_BODY_STATE].cpu().numpy(), bstate, err_msg=f"{symbol} body sub-step {it}")
    assert int(T[_abi.T_DROPPED].sum()) == dropped
    sim.destroy()


@pytest.mark.parametrize("setting", SETTINGS, ids=_ids(SETTINGS))
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("form", list(ABB_SCENE_FORMS))
def test_abb_scene_at_other_solver_settings(oracle, form, solver, setting):
    """gym.simulate on the arm with table, cube and pad: the free cube as a solver body of its own, the rod's capsule against it
    with impulses on both sides, with link contacts the arm's volumes against table / cube / pad -- sixty sub-steps of the ramp."""
    _need_gpu()
    link, split, n, symbol = ABB_SCENE_FORMS[form]
    cm, sp, boxes, start, steps, dropped = _abb_scene_oracle_run(oracle, link, n, solver, setting)
    _abb_scene_on_gpu(cm, sp, boxes, n, start, steps, dropped, split, symbol)


# ------------------------------------------------------------------------------------------------------ the fused ABB step --
VEC_STEPS_ABB = 12


def _abb_symbol(mapping, link):
    if mapping == "split":
        return "_Z18k_abb_step_ws_hardILb%dEE" % int(link)
    return "_Z19k_abb_step_pgs_wideILb1EE" if link else "_Z10k_abb_stepILi32E7DynDims8DynSceneLb0ELi0ELb1ELb0EE"


def _fused_abb_env(n, link, mapping, solver, setting):
    from shifu_amd.gym.abb_fused import FusedAbbEnv
    env = FusedAbbEnv(num_envs=n, seed=12, link_contacts=link, solver=solver,
                      solver_kw=dict(pos_iters=setting[0], vel_iters=setting[1], max_contacts=setting[2]),
                      **({"mapping": "body"} if mapping == "body" else {}))
    sp = env.sim_params
    assert (sp.pos_iters, sp.vel_iters, sp.max_contacts) == setting and env.mapping == mapping
    assert sp.solver == (_abi.SOLVER_TGS if solver == "tgs" else _abi.SOLVER_PGS)
    assert env.task.kernel_symbol() == _abb_symbol(mapping, link), env.task.kernel_symbol()
    # envs 0, 5 and 16 (the tail) time out within the run and re-spawn
    ep = env.task.tensors[_abi.ABB_EP_LEN]
    ep[0], ep[5], ep[16] = env.max_episode_length - 3, env.max_episode_length - 6, env.max_episode_length - 9
    torch.cuda.synchronize()
    return env


def _abb_bufs(env):
    bufs = {k: env.sim.tensors[t].cpu().numpy().copy() for k, t in _ABB_SIM_T.items()}
    bufs.update({k: env.task.tensors[t].cpu().numpy().copy() for k, t in _ABB_T.items()})
    return bufs


def _abb_check(env, bufs, tag):
    torch.cuda.synchronize()
    for k, t in list(_ABB_SIM_T.items()) + list(_ABB_T.items()):
        got = (env.sim.tensors if k in _ABB_SIM_T else env.task.tensors)[t].cpu().numpy().reshape(bufs[k].shape)
        np.testing.assert_array_equal(got, bufs[k], err_msg=f"{k} {tag}")


@pytest.mark.parametrize("setting", SETTINGS, ids=_ids(SETTINGS))
@pytest.mark.parametrize("solver", SOLVERS)
@pytest.mark.parametrize("link", [False, True], ids=["rod", "link"])
@pytest.mark.parametrize("mapping", ["split", "body"])
def test_fused_abb_step_at_other_solver_settings(oracle, mapping, link, solver, setting):
    """FusedAbbEnv(solver_kw=...): k_abb_step_ws_hard, k_abb_step_pgs_wide and the run-time-shaped k_abb_step, seventeen envs
    (sixteen to a workgroup and a tail), twelve vec-steps of random actions in which three envs time out and re-spawn."""
    _need_gpu()
    n = 17
    env = _fused_abb_env(n, link, mapping, solver, setting)
    bufs = _abb_bufs(env)
    sp1 = _with_one_velocity_iteration(env.sim_params)
    rng = np.random.default_rng(6)
    resets, differs, fmax = 0, False, 0.0
    offered = np.zeros(2, np.int64)
    for it in range(VEC_STEPS_ABB):
        raw = (2 * rng.random((n, 3)) - 1).astype(np.float32)
        env.task.step(torch.from_numpy(raw).cuda())
        offered += _offered(oracle, lambda s: oracle.scene_step(env.cm.blob, s, env.boxes, n, bufs["dof_state"].copy(), bufs["root_state"].copy(),
                                                                friction=bufs["friction"]), env.sim_params)
        if _live(solver, setting):
            alt = copy.deepcopy(bufs)
            oracle.abb_step(env.cm.blob, sp1, env.boxes, env.task_params, n, 0, alt, raw)
        oracle.abb_step(env.cm.blob, env.sim_params, env.boxes, env.task_params, n, 0, bufs, raw)
        if _live(solver, setting):
            differs |= not np.array_equal(alt["contact"], bufs["contact"])
        _abb_check(env, bufs, f"step {it}")
        resets += int(bufs["reset"].sum())
        fmax = max(fmax, float(np.abs(bufs["contact"]).max()))
    assert resets >= 3, resets
    assert fmax > 0.9 and np.isfinite(bufs["obs"]).all(), fmax           # (a cube weighs 0.981 N)
    _offer_conditions(setting, offered)
    if _live(solver, setting):
        assert differs, "one velocity iteration on the same states reports the same forces: vel_iters = 0 was not live"
