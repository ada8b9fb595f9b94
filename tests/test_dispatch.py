"""Which kernel a step launches, asked of the library itself (shf_sim_step_plan / shf_a1_step_plan / shf_abb_step_plan,
include/shifu_amd.h) over the whole configuration space -- no GPU, no tensors: the plan entries report on the configuration
alone, and the step entries launch what they report (csrc/shf_api.hip: one selection function per entry).

For every combination of solver x mapping x lanes x terrain x self-collision x link contacts x max_contacts x hulls / face
manifold that the models allow, either
 (a) the combination is accepted: the kernel is an instantiation the build holds (a key of libshifu_amd.resources.json), the
     workgroup has 256 or 512 threads, its LDS fits a CU's 160 KiB and the grid is ceil(n / envs per workgroup), or
 (b) it is refused with a message (by the set-up call that refuses it, or by the plan with the step's own message);
 (c) and where it is accepted, the fused steps' kernel is the one backend.py's name mirror (deleted with this test's arrival; its
     code lives on below as the expectation) would have named.
"""
import copy
import ctypes as C
import itertools
import json
import re
import types

import pytest

from shifu_amd import _abi, build
from shifu_amd._lib import lib
from shifu_amd.abb_task import abb_boxes, abb_model, abb_task_params, box_desc
from shifu_amd.backend import _plan_symbol
from tests import kat_models
from tests.helpers import a1_model, sim_params

N = 1000          # envs: not a multiple of 16, so that the grid's rounding shows
SOLVERS = ("compliant", "pgs", "tgs")
MAPPINGS = ("body", "chain", "split")
LANES = (16, 32, 64)
TERRAINS = ("flat", "heightfield", "trimesh")
ARG_TAILS = ("v7SimArgs", "v6A1Args", "v7AbbArgs", "6A1Args")


@pytest.fixture(scope="module")
def resources():
    build.build_native()
    return json.load(open(build.RESOURCES))


@pytest.fixture(scope="module")
def models():
    a1 = {(s, lk): a1_model(self_collision=s, link_contacts=lk).blob for s in (False, True) for lk in (False, True)}
    dyn = {}
    for s in (False, True):        # articulations the compile-time A1 shapes do not fit (only their shape matters: nothing is launched)
        dyn[(s, 17)] = copy.deepcopy(a1[(s, False)])
        dyn[(s, 17)].np = 75              # the A1 less one sample point
        for lk in (False, True):
            dyn[(s, 16, lk)] = copy.deepcopy(a1[(s, lk)])
            dyn[(s, 16, lk)].nb, dyn[(s, 16, lk)].np = 12, 60      # ... and the A1 less five bodies and sixteen points: fits 16 lanes, with box actors too
        dyn[(s, 16)] = dyn[(s, 16, False)]
    return types.SimpleNamespace(a1=a1, dyn=dyn, arm={lk: abb_model(link_contacts=lk) for lk in (False, True)},
                                 arm_hull=abb_model(link_contacts=True, link_shapes="hull"), ram=kat_models.box_pusher_model(),
                                 ram_hull=kat_models.hull_pusher_model(kat_models.prism_verts()), rod=kat_models.pusher_model())


def _err():
    return lib().shf_last_error().decode()


def _terrain(kind):
    t = _abi.ShfTerrain()
    t.hscale, t.vscale, t.friction, t.nz_min = 0.1, 0.005, 1.0, 0.0
    if kind != "flat":
        t.rows = t.cols = 8
    t.warped = int(kind == "trimesh")
    return t


def make_sim(blob, *, solver, mapping, lanes, terrain="flat", max_contacts=8, boxes=(), hulls=None, flags=0):
    """The set-up calls in backend.Sim's order.  (handle, None), or (None, message) from the call that refused."""
    l = lib()
    sp = sim_params(solver=solver, max_contacts=max_contacts)
    h = C.c_void_p()
    assert l.shf_sim_create(C.byref(sp), C.byref(h)) == 0
    t, m = _terrain(terrain), copy.deepcopy(blob)
    calls = [lambda: l.shf_sim_set_terrain(h, C.byref(t)), lambda: l.shf_sim_set_articulation(h, C.byref(m))]
    if hulls is not None:
        calls.append(lambda: l.shf_sim_set_hulls(h, C.byref(hulls)))
    if flags:
        calls.append(lambda: l.shf_sim_set_scene_flags(h, flags))
    calls += [lambda b=b: l.shf_sim_add_box(h, C.byref(b)) for b in boxes]
    calls.append(lambda: l.shf_sim_finalize(h, N, 0))
    if mapping != "body":
        calls.append(lambda: l.shf_sim_set_mapping(h, _abi.MAP_CHAIN if mapping == "chain" else _abi.MAP_CHAIN_SPLIT))
    if mapping != "body" or lanes != 64:
        calls.append(lambda: l.shf_sim_set_group(h, lanes))
    for call in calls:
        if call() != 0:
            msg = _err()
            l.shf_sim_destroy(h)
            return None, msg
    return h, None


def plan_of(fn, handle):
    p = _abi.ShfLaunchPlan()
    if fn(handle, C.byref(p)) != 0:
        return None, _err()
    return p, None


def envs_per_block(symbol, block):
    """The documented envs per workgroup of a step kernel (csrc/shf_kernels.h, csrc/shf_a1_chain.hip)."""
    if block == 512:                      # k_*_step_ws_hard, k_*_step_pgs_wide, k_abb_step_ws<512, true>: sixteen envs per workgroup
        return 16
    if "k_abb_step_wsILi256" in symbol:   # 2 arm waves + 2 box waves for 8 envs
        return 8
    if re.match(r"_Z\d+k_(a1_chain|sim_step_chain)_(pgs|tgs)", symbol) or symbol.endswith("_a1_g32"):       # 32 lanes per env
        return 8
    return 256 // int(re.search(r"ILi(\d+)E", symbol).group(1))         # k_sim_step / k_a1_step / k_a1_step_self / k_abb_step / k_a1_chain <G, ...>


def check_accepted(p, resources):
    """(a); returns the symbol without its parameter encoding, as kernel_symbol() does."""
    full = p.kernel.decode()
    assert full in resources, f"{full} is not an instantiation in the build"
    tail = [t for t in ARG_TAILS if full.endswith(t)][0]
    sym = full[:-len(tail)]
    assert p.block in (256, 512) and 0 < p.lds_bytes <= 160 * 1024
    epb = envs_per_block(sym, p.block)
    assert p.grid == -(-N // epb), (sym, p.grid, epb)
    return sym


LDS_REFUSAL = re.compile(r"kernel needs \d+ B of LDS per block, the CU has 160 KiB$")       # (what the launch itself said before there was a plan)


def check_refused(msg, who="shf_"):
    """(b)"""
    assert msg and (msg.startswith(who) or LDS_REFUSAL.match(msg)), msg


# ------------------------------------------------------------------ the name mirror that lived in shifu_amd/backend.py --
# A1Task.kernel_symbol() / AbbTask.kernel_symbol() as they stood, on a stand-in for the backend's Sim (group, mapping, terrain,
# model, params, nboxes, scene_flags).  Where the mirror returned only a prefix of the symbol (the body-mapped A1 kernels, the
# run-time-shaped compliant ABB kernels), the remaining template arguments are filled in here, so that the comparison is exact.
# The mirror and the C++ agreed on every accepted combination below: no case had to be resolved in favour of the C++.
def mirror_a1(sim):
    g, warped = sim.group, bool(sim.terrain.warped)
    mdl = sim.model
    selfc = int(bool(mdl.self_collide and mdl.npair > 0))
    if sim.params.solver != _abi.SOLVER_COMPLIANT:
        k16 = int(sim.params.max_contacts) > 8      # up to 16 constraints per env: the packed-response-matrix kernel
        name = ("k_a1_chain_tgs" if sim.params.solver == _abi.SOLVER_TGS else "k_a1_chain_pgs") + ("16" if k16 else "")
        return f"_Z{len(name)}{name}ILb{int(warped)}ELb{selfc}EE"
    if sim.mapping == "chain":
        return f"_Z10k_a1_chainILi{g}ELb{int(warped)}ELb{selfc}EE"
    a1 = mdl.nb == 17 and mdl.nd == 12 and mdl.np == 76
    fixed = "9FixedDimsILi17ELi12ELi76ELi3ELi4EEE"      # (completed: the mirror stopped at "9FixedDims" / "7DynDims")
    if selfc:
        if a1:
            return "_Z21k_a1_step_self_a1_g32" if not warped else "_Z14k_a1_step_selfILi32E" + fixed
        return f"_Z14k_a1_step_selfILi{g}E7DynDimsE"
    if a1:
        return "_Z16k_a1_step_a1_g32" if (g == 32 and not warped) else f"_Z9k_a1_stepILi{g}E" + fixed
    return f"_Z9k_a1_stepILi{g}E7DynDimsE"


def mirror_abb(sim, wide):
    mdl = sim.model
    link = bool(mdl.link_collide and sim.nboxes > 0)
    fixed = mdl.nb == 7 and mdl.np == (59 if link else 3) and sim.nboxes == 3
    pre = f"_Z10k_abb_stepILi{sim.group}E"
    if mdl.nhull > 0 or sim.scene_flags:     # the convex narrow phase compiled in (csrc/shf_hull.h): run-time shapes
        hard = int(sim.params.solver != _abi.SOLVER_COMPLIANT)
        return f"_Z10k_abb_stepILi{32 if hard else sim.group}E7DynDims8DynSceneLb1ELi0ELb{hard}ELb1EE"
    if sim.params.solver != _abi.SOLVER_COMPLIANT and sim.mapping == "split":
        return f"_Z18k_abb_step_ws_hardILb{int(link)}EE"     # arm wave + box wave, the solve regrouped at 32 lanes per env
    if sim.params.solver != _abi.SOLVER_COMPLIANT:    # the generic velocity-level solve: run-time shapes, 32 lanes per env
        if wide:   # sixteen envs per workgroup of 512 threads (the mirror asked shf_abb_step_pgs_is_wide; `wide` is pinned below)
            return f"_Z19k_abb_step_pgs_wideILb{int(link)}EE"
        return f"_Z10k_abb_stepILi32E7DynDims8DynSceneLb{int(link)}ELi0ELb1ELb0EE"
    if not fixed:
        return pre + f"7DynDims8DynSceneLb{int(link)}ELi0ELb0ELb0EE"     # (completed: the mirror stopped at "7DynDims")
    if link:    # the shipped arm with its link volumes in the shipped scene (AbbLinkDims, AbbScene)
        if sim.mapping == "split":
            return "_Z13k_abb_step_wsILi512ELb1EE"
        return pre + "9FixedDimsILi7ELi6ELi59ELi6ELi6EE10FixedSceneILi3ELi1ELi2EELb1ELi0ELb0ELb0EE"
    if sim.mapping == "split":
        return "_Z13k_abb_step_wsILi256ELb0EE"
    arm = 6 if sim.mapping == "chain" else 0
    return pre + f"9FixedDimsILi7ELi6ELi3ELi6ELi6EE10FixedSceneILi3ELi1ELi2EELb0ELi{arm}ELb0ELb0EE"


def _stand_in(blob, solver, mapping, lanes, terrain, max_contacts, nboxes=0, flags=0):
    return types.SimpleNamespace(group=lanes, mapping=mapping, terrain=_terrain(terrain), model=blob, nboxes=nboxes, scene_flags=flags,
                                 params=sim_params(solver=solver, max_contacts=max_contacts))


def _a1_params():
    tp = _abi.ShfA1TaskParams()
    tp.num_history, tp.num_height_points, tp.decimation = 3, 187, 4
    return tp


def _solver_cases():
    return [(s, k) for s in SOLVERS for k in ((8,) if s == "compliant" else (8, 16))]     # (max_contacts is a field of the velocity-level solves)


# --------------------------------------------------------------------------------------------------- the fused A1 step --
def test_a1_step_dispatch(resources, models):
    l = lib()
    seen, refused = set(), 0
    for (solver, kmax), mapping, lanes, terrain, selfc, dyn in itertools.product(_solver_cases(), MAPPINGS, LANES, TERRAINS, (False, True), (0, 17, 16)):
        blob = models.dyn[(selfc, dyn)] if dyn else models.a1[(selfc, False)]
        cfg = dict(solver=solver, mapping=mapping, lanes=lanes, terrain=terrain, max_contacts=kmax)
        h, msg = make_sim(blob, **cfg)
        if h is None:
            check_refused(msg)
            refused += 1
            continue
        task, tp = C.c_void_p(), _a1_params()
        if l.shf_a1_create(h, C.byref(tp), C.byref(task)) != 0:
            check_refused(_err())
            refused += 1
            l.shf_sim_destroy(h)
            continue
        p, msg = plan_of(l.shf_a1_step_plan, task)
        if p is None:
            check_refused(msg, "shf_a1_step: ")
            refused += 1
        else:
            sym = check_accepted(p, resources)
            assert sym == mirror_a1(_stand_in(blob, **cfg)), cfg
            assert sym == _plan_symbol(l.shf_a1_step_plan, task)
            seen.add(sym)
        l.shf_a1_destroy(task)
        l.shf_sim_destroy(h)
    # every kernel of the fused A1 step in the build is some configuration's choice
    built = {k[:-len(t)] for k in resources for t in ARG_TAILS[1:] if k.endswith(t) and re.match(r"_Z\d+k_a1_(step|chain)", k)}
    built = {k for k in built if not k.endswith("v")}      # ("...Ev6A1Args" also ends in "6A1Args")
    assert seen == built, (sorted(built - seen), sorted(seen - built))
    assert refused > 0


def test_a1_chain_with_self_collision_at_16_lanes_is_refused(models):
    l = lib()
    h, msg = make_sim(models.a1[(True, False)], solver="compliant", mapping="chain", lanes=16, terrain="heightfield")
    assert h is not None, msg
    task, tp = C.c_void_p(), _a1_params()
    assert l.shf_a1_create(h, C.byref(tp), C.byref(task)) == 0
    p, msg = plan_of(l.shf_a1_step_plan, task)
    assert p is None and msg == "shf_a1_step: the chain mapping with self-collision runs at 32 lanes per env"
    l.shf_a1_destroy(task)
    l.shf_sim_destroy(h)


# -------------------------------------------------------------------------------------------------- the fused ABB step --
def _abb_scenes(models):
    """(name, compiled model, boxes, link contacts): the shipped arm in the shipped scene, rod only and with its link volumes (boxes
    or hulls); the same with a fourth box (run-time shapes); a one-joint ram (no compile-time shape fits it)."""
    extra = box_desc([0.05, 0.05, 0.05], 0.0, 0.5, True, [0.2, 0.2, 0.125])
    yield "arm", models.arm[False], abb_boxes(), False
    yield "arm+link", models.arm[True], abb_boxes(), True
    yield "arm+hulls", models.arm_hull, abb_boxes(), True
    yield "arm, 4 boxes", models.arm[False], abb_boxes() + [extra], False
    many = copy.copy(models.arm[False])          # the rod-only arm with as many sample points as make an env's LDS that of the link scene
    many.blob = copy.deepcopy(many.blob)
    many.blob.np = 80
    yield "arm, 80 points", many, abb_boxes(), False
    yield "arm+link, 4 boxes", models.arm[True], abb_boxes() + [extra], True
    yield "ram+link", models.ram, abb_boxes(), True
    yield "rod", models.rod, abb_boxes(), False


def _abb_task(l, h, cm):
    tp = abb_task_params(cm) if "tip0" in cm.rigid_body_dict else _abi.ShfAbbTaskParams()
    if "tip0" not in cm.rigid_body_dict:
        tp.ee_body, tp.cube_actor, tp.goal_actor = cm.blob.nb - 1, 2, 3
    task = C.c_void_p()
    return task if l.shf_abb_create(h, C.byref(tp), C.byref(task)) == 0 else None


def test_abb_step_dispatch(resources, models):
    l = lib()
    seen, refused = set(), 0
    for (name, cm, boxes, link), (solver, kmax), mapping, lanes, terrain, flag in itertools.product(
            _abb_scenes(models), _solver_cases(), MAPPINGS, LANES, TERRAINS, (0, _abi.SCENE_FACE_MANIFOLD)):
        cfg = dict(solver=solver, mapping=mapping, lanes=lanes, terrain=terrain, max_contacts=kmax)
        h, msg = make_sim(cm.blob, boxes=boxes, hulls=cm.hulls, flags=flag, **cfg)
        if h is None:
            check_refused(msg)
            refused += 1
            continue
        task = _abb_task(l, h, cm)
        assert task is not None, _err()
        p, msg = plan_of(l.shf_abb_step_plan, task)
        if p is None:
            check_refused(msg, "shf_abb_step: ")
            assert l.shf_abb_step_pgs_is_wide(task) == 0
            refused += 1
        else:
            sym = check_accepted(p, resources)
            # the 512-thread form of the generic velocity-level step: where sixteen envs' LDS fits a CU and two workgroups of eight
            # do not -- with link contacts (8.7 KB per env in the shipped scene), not in the rod-only scenes
            wide = name in ("arm+link", "arm, 80 points")      # (with a fourth box sixteen envs no longer fit; of the ram, two workgroups of eight do)
            assert sym == mirror_abb(_stand_in(cm.blob, nboxes=len(boxes), flags=flag, **cfg), wide), (name, cfg, flag)
            assert l.shf_abb_step_pgs_is_wide(task) == int("pgs_wide" in sym)
            seen.add(sym)
        l.shf_abb_destroy(task)
        l.shf_sim_destroy(h)
    built = {k[:-len("v7AbbArgs")] for k in resources if re.match(r"_Z\d+k_abb_step", k)}
    assert seen == built, (sorted(built - seen), sorted(seen - built))
    assert refused > 0


@pytest.mark.parametrize("case, message", [
    (dict(link=True, solver="compliant", mapping="chain", lanes=16),
     "shf_abb_step: the chain mapping (arm recursions on one lane) is compiled without link contacts -- with link contacts use "
     "the split mapping (shf_sim_set_mapping(SHF_MAP_CHAIN_SPLIT), 16 lanes) or the body mapping"),
    (dict(link=True, solver="pgs", mapping="split", lanes=32),
     "shf_abb_step: the split mapping under SHF_SOLVER_PGS / _TGS needs the shipped arm, the table / cube / pad scene and 16 lanes per env"),
    (dict(link=False, solver="tgs", mapping="split", lanes=32),
     "shf_abb_step: the split mapping under SHF_SOLVER_PGS / _TGS needs the shipped arm, the table / cube / pad scene and 16 lanes per env"),
])
def test_abb_refusals_keep_their_text(models, case, message):
    l = lib()
    cm = models.arm[case["link"]]
    h, msg = make_sim(cm.blob, boxes=abb_boxes(), solver=case["solver"], mapping=case["mapping"], lanes=case["lanes"])
    assert h is not None, msg
    task = _abb_task(l, h, cm)
    p, msg = plan_of(l.shf_abb_step_plan, task)
    assert p is None and msg == message
    l.shf_abb_destroy(task)
    l.shf_sim_destroy(h)


# ------------------------------------------------------------------------------------------- gym.simulate (shf_sim_step) --
def _sim_scenes(models):
    """(name, model blob, hulls, boxes): articulations on their own and with box actors, without and with link contacts / hulls"""
    cube = box_desc([0.05, 0.05, 0.05], 0.1, 0.5, False, [0.5, 0, 0.125])
    for selfc in (False, True):
        yield f"a1 self={selfc}", models.a1[(selfc, False)], None, []
        yield f"a1 self={selfc} + box", models.a1[(selfc, False)], None, [cube]
        yield f"a1 self={selfc} link + box", models.a1[(selfc, True)], None, [cube]
    yield "cut self=True", models.dyn[(True, 16, False)], None, []
    yield "cut self=True + box", models.dyn[(True, 16, False)], None, [cube]
    yield "cut self=True link + box", models.dyn[(True, 16, True)], None, [cube]
    yield "cut self=True link + 3 boxes", models.dyn[(True, 16, True)], None, abb_boxes()
    yield "rod", models.rod.blob, None, []
    yield "arm", models.arm[False].blob, None, abb_boxes()
    yield "arm+link", models.arm[True].blob, None, abb_boxes()
    yield "arm+hulls", models.arm_hull.blob, models.arm_hull.hulls, abb_boxes()
    yield "ram+link", models.ram.blob, None, [cube]
    yield "ram+hull", models.ram_hull.blob, models.ram_hull.hulls, [cube]
    yield "arm+link, 4 boxes", models.arm[True].blob, None, abb_boxes() + [cube]


def test_sim_step_dispatch(resources, models):
    l = lib()
    seen, refused = set(), 0
    for (name, blob, hulls, boxes), (solver, kmax), mapping, lanes, terrain, flag in itertools.product(
            _sim_scenes(models), _solver_cases(), MAPPINGS, LANES, TERRAINS, (0, _abi.SCENE_FACE_MANIFOLD)):
        h, msg = make_sim(blob, boxes=boxes, hulls=hulls, flags=flag, solver=solver, mapping=mapping, lanes=lanes, terrain=terrain, max_contacts=kmax)
        if h is None:
            check_refused(msg)
            refused += 1
            continue
        p, msg = plan_of(l.shf_sim_step_plan, h)
        if p is None:
            check_refused(msg, "shf_sim_step: ")
            refused += 1
        else:
            sym = check_accepted(p, resources)
            ext = bool(boxes) and (flag != 0 or hulls is not None)
            if name.startswith("a1") and not boxes and solver != "compliant":      # the hook path's A1 sub-step: the chain-mapped solve
                k = "k_sim_step_chain_" + solver + ("16" if kmax > 8 else "")
                assert sym == f"_Z{len(k)}{k}ILb{int(terrain == 'trimesh')}ELb{int('self=True' in name)}EE"
            elif "ws_hard" in sym:       # the kernel compiled for the shipped arm + scene: the split mapping under a velocity-level solve
                assert mapping == "split" and solver != "compliant" and name in ("arm", "arm+link") and not ext
                assert l.shf_sim_step_split_supported(h) == 1
            else:                        # the run-time-shaped family: lanes as set (32 under the velocity-level solves), EXT for hulls / flags
                g = 32 if solver != "compliant" else 64 if (name.startswith("a1") and mapping == "chain") else lanes     # (the A1's chain mapping takes the width for the fused step only)
                assert re.match(r"_Z19k_sim_step_pgs_wideILb[01]EE$", sym) or re.match(
                    r"_Z10k_sim_stepILi%dELb%dELb[01]ELb[01]ELb%dELb%dEE$" % (g, int(bool(boxes)), int(solver != "compliant"), int(ext)), sym), (name, sym)
            seen.add(sym)
        l.shf_sim_destroy(h)
    built = {k[:-len("v7SimArgs")] for k in resources if re.match(r"_Z\d+k_sim_step", k)}
    assert seen == built, (sorted(built - seen), sorted(seen - built))
    assert refused > 0


def test_plan_entries_need_nothing_bound_and_refuse_null():
    """Before finalize shf_sim_step_plan gives the step's own message; a null handle is an error, not a crash."""
    l = lib()
    sp, h, p = sim_params(), C.c_void_p(), _abi.ShfLaunchPlan()
    assert l.shf_sim_create(C.byref(sp), C.byref(h)) == 0
    assert l.shf_sim_step_plan(h, C.byref(p)) != 0 and _err() == "shf_sim_step: sim not finalized"
    assert l.shf_sim_step_plan(None, C.byref(p)) != 0 and l.shf_a1_step_plan(None, C.byref(p)) != 0 and l.shf_abb_step_plan(None, C.byref(p)) != 0
    l.shf_sim_destroy(h)


# ------------------------------------------------------------------------------------------------- the shipped defaults --
def test_shipped_defaults_resolve_to_the_budgeted_kernels(models):
    """What FusedA1Env(), FusedAbbEnv() and the hook path's A1 sim configure (gym/a1_fused.py, gym/abb_fused.py, isaacgym/gymapi.py)
    lands on the kernels whose registers shifu_amd/build.py's BUDGETS protect."""
    l = lib()
    guarded = [p for p, _, _ in build.BUDGETS]
    # FusedA1Env(): no self-collision, height field, tgs, chain mapping at 32 lanes
    h, msg = make_sim(models.a1[(False, False)], solver="tgs", mapping="chain", lanes=32, terrain="heightfield")
    assert h is not None, msg
    task, tp = C.c_void_p(), _a1_params()
    assert l.shf_a1_create(h, C.byref(tp), C.byref(task)) == 0
    assert _plan_symbol(l.shf_a1_step_plan, task) == "_Z14k_a1_chain_tgsILb0ELb0EE" and "_Z14k_a1_chain_tgsILb0ELb0EE" in guarded
    hook = _plan_symbol(l.shf_sim_step_plan, h)          # (gym.simulate of the same sim: the hook path's sub-step)
    assert hook.startswith("_Z20k_sim_step_chain_tgs") and "_Z20k_sim_step_chain_tgs" in guarded
    l.shf_a1_destroy(task)
    l.shf_sim_destroy(h)
    h, msg = make_sim(models.a1[(False, False)], solver="tgs", mapping="body", lanes=64, terrain="heightfield")       # ... and body-mapped at the library's width
    assert h is not None, msg
    assert _plan_symbol(l.shf_sim_step_plan, h) == hook
    l.shf_sim_destroy(h)
    # FusedAbbEnv(): link contacts (box volumes), tgs, split mapping at 16 lanes
    cm = models.arm[True]
    h, msg = make_sim(cm.blob, boxes=abb_boxes(), solver="tgs", mapping="split", lanes=16)
    assert h is not None, msg
    task = _abb_task(l, h, cm)
    assert _plan_symbol(l.shf_abb_step_plan, task) == "_Z18k_abb_step_ws_hardILb1EE" and "_Z18k_abb_step_ws_hardILb1EE" in guarded
    l.shf_abb_destroy(task)
    l.shf_sim_destroy(h)
