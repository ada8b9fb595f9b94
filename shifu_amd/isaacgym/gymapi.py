"""`gymapi` facade: the names shifu and its examples take from `isaacgym.gymapi`
[EXT], re-hosted on the MI355X backend.

This is a naming facade, not a CUDA shim: `acquire_gym()` returns a `Gym` whose 69
methods used by the reference (103 call sites; shifu/gym/isaac_gym.py,
shifu/units/*.py, examples/*) record the scene while envs are created and, from
`prepare_sim` on, forward to the C ABI of include/shifu_amd.h through
shifu_amd.backend.Sim.  Viewer calls are accepted and ignored; camera sensors are rendered by a HIP ray
caster against the collision shapes (shifu_amd/render.py, DESIGN.md "Camera sensors").

Semantics kept from Isaac Gym:
  * state tensors are sim-owned, pointer-stable, viewed once (`acquire_*`), updated
    in place by `refresh_*`; user writes reach the solver only through
    `set_*_tensor[_indexed]` (int32 actor indices in sim domain);
  * `simulate` advances one dt; `apply_rigid_body_force_at_pos_tensors` acts on the
    next `simulate` only; efforts/targets persist.
"""
from __future__ import annotations

import copy
import ctypes as C
import os
from typing import Dict, List, Optional

import numpy as np

from .. import _abi

# -- constants ---------------------------------------------------------------
SIM_PHYSX = 1
SIM_FLEX = 2
UP_AXIS_Y, UP_AXIS_Z = 0, 1
DOF_MODE_NONE, DOF_MODE_POS, DOF_MODE_VEL, DOF_MODE_EFFORT = (_abi.DOF_MODE_NONE, _abi.DOF_MODE_POS,
                                                              _abi.DOF_MODE_VEL, _abi.DOF_MODE_EFFORT)
FROM_ASSET, COMPUTE_PER_VERTEX, COMPUTE_PER_FACE = 0, 1, 2
DOMAIN_ENV, DOMAIN_SIM, DOMAIN_ACTOR = 0, 1, 2
MESH_NONE, MESH_COLLISION, MESH_VISUAL, MESH_VISUAL_AND_COLLISION = 0, 1, 2, 3
IMAGE_COLOR, IMAGE_DEPTH, IMAGE_SEGMENTATION, IMAGE_OPTICAL_FLOW = 0, 1, 2, 3
FOLLOW_POSITION, FOLLOW_TRANSFORM = 0, 1
KEY_ESCAPE, KEY_V = 256, 86
ENV_SPACE, LOCAL_SPACE, GLOBAL_SPACE = 0, 1, 2


# -- plain value types -------------------------------------------------------
class Vec3:
    def __init__(self, x=0.0, y=0.0, z=0.0):
        self.x, self.y, self.z = float(x), float(y), float(z)

    def __add__(self, o):
        return Vec3(self.x + o.x, self.y + o.y, self.z + o.z)

    def __sub__(self, o):
        return Vec3(self.x - o.x, self.y - o.y, self.z - o.z)

    def __iter__(self):
        return iter((self.x, self.y, self.z))

    def __repr__(self):
        return f"Vec3({self.x}, {self.y}, {self.z})"


class Quat:
    def __init__(self, x=0.0, y=0.0, z=0.0, w=1.0):
        self.x, self.y, self.z, self.w = float(x), float(y), float(z), float(w)

    def __iter__(self):
        return iter((self.x, self.y, self.z, self.w))


class Transform:
    def __init__(self, p: Optional[Vec3] = None, r: Optional[Quat] = None):
        self.p = p if p is not None else Vec3()
        self.r = r if r is not None else Quat()


class PhysXParams:
    def __init__(self):
        self.num_threads = 0
        self.use_gpu = True
        self.solver_type = 1
        self.num_position_iterations = 4
        self.num_velocity_iterations = 1
        self.contact_offset = 0.02
        self.rest_offset = 0.0
        self.bounce_threshold_velocity = 0.2
        self.max_depenetration_velocity = 100.0
        self.max_gpu_contact_pairs = 1024 * 1024
        self.default_buffer_size_multiplier = 2.0
        self.contact_collection = 2


class SimParams:
    def __init__(self):
        self.dt = 1.0 / 60.0
        self.substeps = 2
        self.up_axis = UP_AXIS_Y
        self.gravity = Vec3(0.0, -9.8, 0.0)
        self.use_gpu_pipeline = False
        self.physx = PhysXParams()


class AssetOptions:
    def __init__(self):
        self.fix_base_link = False
        self.default_dof_drive_mode = DOF_MODE_NONE
        self.disable_gravity = False
        self.collapse_fixed_joints = False
        self.flip_visual_attachments = False
        self.replace_cylinder_with_capsule = False
        self.mesh_normal_mode = FROM_ASSET
        self.use_physx_armature = True
        self.thickness = 0.02
        self.armature = 0.0
        self.angular_damping = 0.5
        self.linear_damping = 0.0
        self.max_angular_velocity = 64.0
        self.max_linear_velocity = 1000.0
        self.density = 1000.0


class PlaneParams:
    def __init__(self):
        self.normal = Vec3(0.0, 1.0, 0.0)
        self.distance = 0.0
        self.static_friction = 1.0
        self.dynamic_friction = 1.0
        self.restitution = 0.0


class HeightFieldParams:
    def __init__(self):
        self.column_scale = 1.0
        self.row_scale = 1.0
        self.vertical_scale = 1.0
        self.nbRows = 0
        self.nbColumns = 0
        self.transform = Transform()
        self.static_friction = 1.0
        self.dynamic_friction = 1.0
        self.restitution = 0.0


class TriangleMeshParams:
    def __init__(self):
        self.nb_vertices = 0
        self.nb_triangles = 0
        self.transform = Transform()
        self.static_friction = 1.0
        self.dynamic_friction = 1.0
        self.restitution = 0.0


class CameraProperties:
    def __init__(self):
        self.enable_tensors = False
        self.use_collision_geometry = False
        self.width, self.height = 1600, 900
        self.near_plane, self.far_plane = 0.0010000000474974513, 2000000.0
        self.horizontal_fov = 90.0


class RigidShapeProperties:
    def __init__(self, friction=1.0):
        self.friction = friction
        self.rolling_friction = 0.0
        self.torsion_friction = 0.0
        self.restitution = 0.0
        self.compliance = 0.0
        self.thickness = 0.0
        self.contact_offset = 0.0
        self.rest_offset = 0.0
        self.filter = 0


class RigidBodyProperties:
    def __init__(self, mass=0.0):
        self.mass = mass
        self.com = Vec3()
        self.invMass = 0.0 if mass == 0 else 1.0 / mass


# -- scene records -----------------------------------------------------------
class Asset:
    """Result of load_asset / create_box."""

    def __init__(self, kind, name, options, model=None, box_dim=None):
        self.kind, self.name, self.options = kind, name, options
        self.model = model  # CompiledModel for articulations
        self.box_dim = box_dim
        nshapes = model.blob.np if model is not None else 1
        self.shape_props = [RigidShapeProperties() for _ in range(max(nshapes, 1))]

    @property
    def num_bodies(self):
        return self.model.blob.nb if self.model is not None else 1

    @property
    def num_dofs(self):
        return self.model.blob.nd if self.model is not None else 0

    @property
    def body_dict(self) -> Dict[str, int]:
        return self.model.rigid_body_dict if self.model is not None else {"box": 0}


class _Actor:
    def __init__(self, asset, pose, name, sim_index):
        self.asset, self.pose, self.name, self.sim_index = asset, pose, name, sim_index
        self.friction = float(np.mean([p.friction for p in asset.shape_props]))
        self.mass_override: Optional[float] = None
        self.mass_scale = None      # articulations: factor per body on the asset's mass and inertia (set_actor_rigid_body_properties)
        self.dof_props = None


class Env:
    def __init__(self, sim, index):
        self.sim, self.index = sim, index
        self.actors: List[_Actor] = []
        self.cameras: List["_Camera"] = []
        self.seg_ids: Dict[tuple, int] = {}        # (actor handle, body index) -> segmentation id
        self.colors: Dict[tuple, tuple] = {}       # (actor handle, body index) -> RGB in [0, 1]


class _Camera:
    """One create_camera_sensor: its properties and pose (pos, quat xyzw) in the frame of the state tensors, or a body it
    follows (body row within the env, local pos, local quat)."""

    def __init__(self, props: "CameraProperties"):
        self.props = copy.deepcopy(props)
        self.pos = np.zeros(3)
        self.quat = np.array([0.0, 0.0, 0.0, 1.0])
        self.attach = None


class _TensorHandle:
    """What acquire_*_tensor returns; gymtorch.wrap_tensor unwraps it."""

    def __init__(self, tensor):
        self.tensor = tensor


class SimHandle:
    def __init__(self, device_id, params: SimParams):
        self.device_id = device_id
        self.params = params
        self.envs: List[Env] = []
        self.terrain = None          # ("plane", friction) | ("heightfield", samples, hs, vs, border, friction)
        self.backend = None          # shifu_amd.backend.Sim after prepare_sim
        self.robot_asset: Optional[Asset] = None
        self.actors_per_env = 0
        self.num_actors = 0
        self.jacobian = None
        self.mass_matrix = None               # acquire_mass_matrix_tensor / acquire_dof_bias_force_tensor: allocated on first
        self.dof_bias = None                  # acquire, filled by refresh_mass_matrix_tensors
        self.camera_groups: List[dict] = []   # after prepare_sim: one per camera handle (one camera per env each)
        self.ray_caster_groups: List[dict] = []   # create_ray_caster_group: one ray-caster sensor per env each
        self.renderer = None
        self.body_fresh = False               # body_state refreshed since the last simulate (render_all_camera_sensors)
        self.env_grid = (0.0, 0.0, 1)         # create_env's (pitch x, pitch y, envs per row): the viewer's layout


class Gym:
    """The object `gymapi.acquire_gym()` returns."""

    # ---- lifecycle ---------------------------------------------------------
    # PhysX solver settings shifu's config sets (shifu/configs/env_config.py:46-58) that have no counterpart in this
    # backend's compliant, linearly-implicit contact model.  contact_offset and
    # max_depenetration_velocity ARE used (ShfSimParams); the ones below are accepted and ignored -- said once, at
    # create_sim, instead of only in a document.
    IGNORED_PHYSX_FIELDS = {
        "max_gpu_contact_pairs": "contact candidates are fixed per articulation (SHF_MAX_POINTS), no pair buffer",
        "default_buffer_size_multiplier": "no PhysX buffers",
    }
    # honoured (the velocity-level contact solve, include/shifu_amd.h): solver_type (1 = TGS -> SHF_SOLVER_TGS, the sub-stepped
    # sweeps, round 6; 0 = PGS -> SHF_SOLVER_PGS), num_position_iterations, num_velocity_iterations, contact_offset, rest_offset,
    # bounce_threshold_velocity, max_depenetration_velocity (shifu/configs/env_config.py:50-58).  A scene beyond the solve's
    # limits (more than 32 bodies + box actors, trees deeper than 8 levels, several articulations) keeps rounds 1-4's compliant
    # law and says so once at prepare_sim, with the reason.
    SOLVER_PHYSX_FIELDS = ("solver_type", "num_position_iterations", "num_velocity_iterations", "rest_offset", "bounce_threshold_velocity")
    _warned_physx = False
    _warned_compliant = False

    def create_sim(self, compute_device=0, graphics_device=0, physics_engine=SIM_PHYSX, params: SimParams = None):
        params = params or SimParams()
        if not Gym._warned_physx:
            Gym._warned_physx = True
            import warnings
            ref = PhysXParams()
            for name, why in Gym.IGNORED_PHYSX_FIELDS.items():
                val = getattr(params.physx, name, None)
                if val is not None and val != getattr(ref, name, None):
                    warnings.warn(f"shifu_amd: sim_params.physx.{name} = {val!r} is ignored by this backend ({why})",
                                  stacklevel=2)
        return SimHandle(compute_device, params)

    def add_ground(self, sim: SimHandle, params: PlaneParams):
        sim.terrain = ("plane", 0.5 * (params.static_friction + params.dynamic_friction))

    def add_heightfield(self, sim: SimHandle, samples, params: HeightFieldParams):
        # shifu passes nbRows = tot_cols / nbColumns = tot_rows with samples laid out (tot_rows, tot_cols),
        # x <-> first index, shifted by -border (isaac_gym.py:356-367)
        hs = np.ascontiguousarray(np.asarray(samples, dtype=np.int16).reshape(params.nbColumns, params.nbRows))
        sim.terrain = ("heightfield", hs, float(params.row_scale), float(params.vertical_scale),
                       float(-params.transform.p.x), 0.5 * (params.static_friction + params.dynamic_friction))

    def add_triangle_mesh(self, sim: SimHandle, vertices, triangles, params: TriangleMeshParams):
        """Trimesh terrain (the reference's effective A1 terrain, Q5).  The mesh is expected to come from
        convert_heightfield_to_trimesh; it is collided as that warped grid (ShfTerrain.warped) when
        the caller passes the height map and slope threshold it was made from; without that hint the map, its scales
        and the vertex shifts are recovered exactly from the vertex / triangle arrays (and any other kind of mesh is
        refused)."""
        if getattr(params, "height_samples", None) is not None:
            # hint set by shifu_amd's TerrainGymEnv._create_trimesh: the map the mesh came from
            from . import terrain_utils
            hs = np.ascontiguousarray(np.asarray(params.height_samples, dtype=np.int16))
            warp = None
            if hasattr(params, "slope_threshold"):
                warp = terrain_utils.trimesh_warp_map(hs, float(params.horizontal_scale), float(params.vertical_scale),
                                                      params.slope_threshold)
            sim.terrain = ("heightfield", hs, float(params.horizontal_scale), float(params.vertical_scale),
                           float(-params.transform.p.x), 0.5 * (params.static_friction + params.dynamic_friction), warp)
            return
        # no hint (e.g. the reference's own TerrainGymEnv._create_trimesh, isaac_gym.py:369-385, on this facade): the
        # generator keeps the vertices in grid order, so samples, scales and vertex shifts are recovered exactly
        from . import terrain_utils
        if params.nb_vertices * 3 != np.asarray(vertices).size or params.nb_triangles * 3 != np.asarray(triangles).size:
            raise ValueError("add_triangle_mesh: nb_vertices / nb_triangles do not match the arrays")
        hs, hscale, vscale, warp = terrain_utils.heightfield_from_trimesh(vertices, triangles)
        sim.terrain = ("heightfield", hs, hscale, vscale, float(-params.transform.p.x),
                       0.5 * (params.static_friction + params.dynamic_friction), warp)

    def load_asset(self, sim, rootpath, filename, options: AssetOptions = None):
        import os
        from ..model import compile_urdf, asset_path
        options = options or AssetOptions()
        path = os.path.join(rootpath, filename)
        if not os.path.exists(path):
            # the reference's asset tree does not travel; the physics-only URDFs ship in shifu_amd/assets
            base = os.path.basename(filename)
            alt = {"a1.urdf": "a1.urdf", "abb_rod_isaac.urdf": "abb_rod.urdf"}.get(base, base)
            path = asset_path(alt)
        # <mesh> colliders become convex hulls where the files are present (they do not ship with this repo: the vendored
        # URDFs are the physics-only reductions); against box actors only rounded shapes are tested, so the ABB rod gets its
        # documented capsule either way
        extra, boxes = (), ()
        if os.path.basename(path) in ("abb_rod.urdf", "abb_rod_isaac.urdf"):
            from ..abb_task import ROD_CAPSULE, abb_link_boxes
            extra = ROD_CAPSULE
            # box stand-ins for the links' mesh colliders (their files do not ship): only when the URDF brought no hulls
            boxes = abb_link_boxes() if os.path.basename(path) == "abb_rod.urdf" else ()
        # every shape of an env collides with every other actor's (create_actor(..., group = env, filter = 0),
        # units.py:68): link contacts on (ShfModel.link_collide; a scene without box actors never looks at it)
        model = compile_urdf(path, extra_spheres=extra, extra_boxes=boxes, link_contacts=True,
                             fix_base_link=bool(options.fix_base_link),
                             disable_gravity=bool(options.disable_gravity),
                             collapse_fixed_joints=bool(options.collapse_fixed_joints),
                             default_dof_drive_mode=int(options.default_dof_drive_mode),
                             armature=float(getattr(options, "armature", 0.0)),
                             density=float(getattr(options, "density", 1000.0)), meshes="auto")
        return Asset("articulation", filename, options, model=model)

    def create_box(self, sim, x, y, z, options: AssetOptions = None):
        return Asset("box", "box", options or AssetOptions(), box_dim=(float(x), float(y), float(z)))

    def create_env(self, sim: SimHandle, lower, upper, num_per_row):
        env = Env(sim, len(sim.envs))
        if not sim.envs:
            # the grid Isaac Gym would place the envs on (pitch = the env box's extent, num_per_row per row).  The sim does
            # not use it -- every env sits at the origin of the state tensors -- but the viewer lays the envs out on it
            sim.env_grid = (float(upper.x) - float(lower.x), float(upper.y) - float(lower.y), max(int(num_per_row), 1))
        sim.envs.append(env)
        return env

    def create_actor(self, env: Env, asset: Asset, pose: Transform, name="", group=0, filter=0, seg_id=0):
        idx = env.sim.num_actors
        env.sim.num_actors += 1
        a = _Actor(asset, copy.deepcopy(pose), name, idx)
        # [EXT] collision filter: two shapes of one actor collide unless (filter_a & filter_b) != 0; shifu passes 0
        # (units.py:68), i.e. self-collision on
        a.self_collide = (int(filter) == 0)
        env.actors.append(a)
        return len(env.actors) - 1

    def get_actor_index(self, env: Env, actor_handle, domain=DOMAIN_SIM):
        return env.actors[actor_handle].sim_index if domain == DOMAIN_SIM else actor_handle

    # ---- asset / actor queries ---------------------------------------------
    def get_asset_rigid_body_count(self, asset): return asset.num_bodies
    def get_asset_dof_count(self, asset): return asset.num_dofs
    def get_asset_rigid_body_dict(self, asset): return dict(asset.body_dict)
    def get_asset_dof_properties(self, asset):
        return asset.model.dof_properties() if asset.model is not None else np.zeros(0)
    def get_asset_rigid_shape_properties(self, asset): return copy.deepcopy(asset.shape_props)
    def set_asset_rigid_shape_properties(self, asset, props): asset.shape_props = copy.deepcopy(list(props))
    def get_actor_rigid_body_dict(self, env, actor_handle): return dict(env.actors[actor_handle].asset.body_dict)
    def find_actor_rigid_body_handle(self, env, actor_handle, name):
        return env.actors[actor_handle].asset.body_dict.get(name, -1)
    def get_actor_rigid_shape_properties(self, env, actor_handle):
        a = env.actors[actor_handle]
        return [RigidShapeProperties(a.friction) for _ in a.asset.shape_props]
    def set_actor_rigid_shape_properties(self, env, actor_handle, props):
        env.actors[actor_handle].friction = float(np.mean([p.friction for p in props]))
    def get_actor_rigid_body_properties(self, env, actor_handle):
        a = env.actors[actor_handle]
        if a.asset.model is None:
            return [RigidBodyProperties(a.mass_override or 0.0)]
        sc = a.mass_scale
        return [RigidBodyProperties(a.asset.model.blob.mass[b] * (1.0 if sc is None else float(sc[b]))) for b in range(a.asset.num_bodies)]
    def set_actor_rigid_body_properties(self, env, actor_handle, props, recomputeInertia=True):
        a = env.actors[actor_handle]
        if a.asset.model is None:
            a.mass_override = float(props[0].mass)
            return True
        # per-env link masses of an articulation (shifu/units/units.py:104-110, recomputeInertia=True): kept on the actor as a
        # factor per body on the asset's mass and inertia tensor -- uniform density, so the tensor scales with the mass and the
        # centre of mass stays -- and uploaded by prepare_sim as SHF_T_BODY_MASS_SCALE.  A body welded to its parent carries no
        # mass of its own here (the compiled model folds it into the parent): an edit of such a body is refused, not dropped.
        blob = a.asset.model.blob
        scale = np.ones(a.asset.num_bodies, np.float32)
        for b, pr in enumerate(props):
            m0, m1 = float(blob.mass[b]), float(pr.mass)
            if abs(m1 - m0) <= 1e-9 * max(1.0, abs(m0)):
                continue
            if not recomputeInertia:
                raise NotImplementedError("set_actor_rigid_body_properties: recomputeInertia=False (mass without its inertia "
                                          "tensor) is not supported")
            if m0 <= 0.0 or m1 <= 0.0:
                raise NotImplementedError(f"set_actor_rigid_body_properties: body {b} is welded to its parent (its mass is part "
                                          "of the parent's here) or the new mass is not positive")
            scale[b] = m1 / m0
        a.mass_scale = scale if bool((scale != 1.0).any()) else None
        return True
    def set_actor_dof_properties(self, env, actor_handle, props):
        env.actors[actor_handle].dof_props = props
    def set_rigid_body_segmentation_id(self, env: Env, actor_handle, rigid_body_index, segmentation_id):
        env.seg_ids[(int(actor_handle), int(rigid_body_index))] = int(segmentation_id)
        self._camera_table_update(env, actor_handle, rigid_body_index)

    def set_rigid_body_color(self, env: Env, actor_handle, rigid_body_index, mesh_type, color):
        rgb = (color.x, color.y, color.z) if isinstance(color, Vec3) else tuple(color)
        env.colors[(int(actor_handle), int(rigid_body_index))] = tuple(float(c) for c in rgb)
        self._camera_table_update(env, actor_handle, rigid_body_index)

    def get_rigid_body_segmentation_id(self, env: Env, actor_handle, rigid_body_index):
        return env.seg_ids.get((int(actor_handle), int(rigid_body_index)), 0)

    def get_rigid_body_color(self, env: Env, actor_handle, rigid_body_index, mesh_type=MESH_VISUAL):
        from ..render import DEFAULT_BODY_COLOR
        return Vec3(*env.colors.get((int(actor_handle), int(rigid_body_index)), DEFAULT_BODY_COLOR))

    # ---- prepare ---------------------------------------------------------------
    def prepare_sim(self, sim: SimHandle):
        import torch
        from ..backend import Sim, default_sim_params
        from .._lib import lib
        p = sim.params
        # the contact solver: the physx settings as they are (SHF_SOLVER_PGS) where the velocity-level solve is built for the
        # scene, else the compliant law (SHIFU_AMD_SOLVER=compliant forces it: A/B runs)
        env0 = sim.envs[0]
        arts = [a for a in env0.actors if a.asset.kind == "articulation"]
        probe = copy.deepcopy(arts[0].asset.model.blob) if len(arts) == 1 else None
        if probe is not None:
            probe.self_collide = int(bool(getattr(arts[0], "self_collide", False)) and probe.npair > 0 and
                                     os.environ.get("SHIFU_AMD_SELF_COLLISION", "1") != "0")
        # physx.solver_type: 1 = temporal Gauss-Seidel, the reference's value (env_config.py:50) -> SHF_SOLVER_TGS; 0 -> SHF_SOLVER_PGS;
        # SHIFU_AMD_SOLVER = tgs | pgs | compliant overrides.  The compliant law is the fallback, with the actual reason said once.
        want = os.environ.get("SHIFU_AMD_SOLVER", "tgs" if int(getattr(p.physx, "solver_type", 1)) == 1 else "pgs")
        reason = None
        if want == "compliant":
            reason = "SHIFU_AMD_SOLVER=compliant"
        elif probe is None:
            reason = f"{len(arts)} articulations per env (the solve is built for one)"
        elif int(p.physx.num_position_iterations) < 1:
            reason = f"physx.num_position_iterations = {int(p.physx.num_position_iterations)} (the solve needs at least one)"
        elif lib().shf_model_pgs_supported(C.byref(probe), len(env0.actors) - 1) != 1:
            reason = (f"{probe.nb} bodies + {len(env0.actors) - 1} box actors, {probe.nlevels} tree levels: beyond the generic solve's limits "
                      "(32 bodies + box actors, 8 levels; csrc/shf_hard.h)")
        pgs = reason is None
        # max_contacts is not a PhysX field: the 8 deepest candidates per env everywhere by default (a walking A1 offers more in 1e-6 of
        # its sub-steps, profiles/r06_play_a1_*.json); SHIFU_AMD_MAX_CONTACTS raises it to up to 16 for an A1 on its own
        solver_kw = dict(solver=("tgs" if want == "tgs" else "pgs"), pos_iters=int(p.physx.num_position_iterations),
                         vel_iters=int(p.physx.num_velocity_iterations), rest_offset=float(p.physx.rest_offset),
                         bounce_threshold=float(p.physx.bounce_threshold_velocity),
                         max_contacts=int(os.environ.get("SHIFU_AMD_MAX_CONTACTS", "8"))) if pgs else {}
        if not pgs and not Gym._warned_compliant:
            Gym._warned_compliant = True
            import warnings
            warnings.warn("shifu_amd: this scene runs the compliant contact law of rounds 1-4 instead of the velocity-level solve that "
                          "honours sim_params.physx." + " / ".join(Gym.SOLVER_PHYSX_FIELDS) + ": " + reason, stacklevel=2)
        sim.solver = solver_kw["solver"] if pgs else "compliant"
        sp = default_sim_params(dt=p.dt, gravity=tuple(p.gravity),
                                max_depen_vel=min(float(p.physx.max_depenetration_velocity), 10.0),
                                contact_offset=float(p.physx.contact_offset), **solver_kw)
        dev = torch.device("cuda", sim.device_id if isinstance(sim.device_id, int) and sim.device_id >= 0 else 0)
        be = Sim(sp, dev)
        if sim.terrain is None or sim.terrain[0] == "plane":
            be.set_plane(sim.terrain[1] if sim.terrain else 1.0)
        else:
            _, hs, hscale, vscale, border, mu = sim.terrain[:6]
            warp = sim.terrain[6] if len(sim.terrain) > 6 else None
            if any(a.asset.kind != "articulation" for a in sim.envs[0].actors):
                warp = None          # box actors collide with the height-field form only
            be.set_heightfield(hs, hscale, vscale, border, mu, warp=warp)
        env0 = sim.envs[0]
        robots = [a for a in env0.actors if a.asset.kind == "articulation"]
        if len(robots) != 1 or env0.actors[0] is not robots[0]:
            raise NotImplementedError("each env needs exactly one articulated actor, created first "
                                      "(shifu assumes only the robot has DOFs: robot.py:51-52)")
        robot = robots[0]
        sim.robot_asset = robot.asset
        m = copy.deepcopy(robot.asset.model.blob)
        m.self_collide = int(bool(getattr(robot, "self_collide", False)) and m.npair > 0 and
                             os.environ.get("SHIFU_AMD_SELF_COLLISION", "1") != "0")
        if robot.dof_props is not None:
            for d in range(m.nd):
                m.drive_mode[d] = int(robot.dof_props["driveMode"][d])
                m.kp[d] = float(robot.dof_props["stiffness"][d])
                m.kd[d] = float(robot.dof_props["damping"][d])
                # [EXT] dof_props['damping'] is the joint's passive damping (it is what <dynamics damping> of the URDF
                # is imported into); PhysX keeps applying it when the drive is off (DOF_MODE_NONE / EFFORT), where only
                # the position spring ('stiffness') has no target to act on.  shifu writes dof_stiffness / dof_damping
                # into the props in every mode (robot.py:35-37), so the torque-controlled A1 carries 0.5 N m s/rad of
                # implicit joint damping next to its explicit PD -- without it PPO on the reference schedule never
                # leaves the standing optimum in this simulator (profiles/r02_walk_ablation.json).
                if m.drive_mode[d] in (DOF_MODE_NONE, DOF_MODE_EFFORT):
                    m.damping[d] = float(robot.dof_props["damping"][d])
                if "armature" in robot.dof_props.dtype.names:
                    m.armature[d] = float(robot.dof_props["armature"][d])
        be.set_articulation(m)
        for a in env0.actors[1:]:
            if a.asset.kind != "box":
                raise NotImplementedError("extra actors must be boxes (object.py:19-39)")
            b = _abi.ShfBoxDesc()
            b.dim[:] = a.asset.box_dim
            b.mass = a.mass_override if a.mass_override is not None else 0.0
            b.friction = a.friction
            b.fixed = int(bool(a.asset.options.fix_base_link) or b.mass == 0.0)
            b.pos[:] = tuple(a.pose.p)
            b.quat[:] = tuple(a.pose.r)
            be.add_box(b)
        sim.actors_per_env = len(env0.actors)
        n = len(sim.envs)
        be.finalize(n, 0)
        # the shipped arm + scene under TGS / PGS WITHOUT self-collision has a gym.simulate kernel of its own (k_sim_step_ws_hard); with
        # self-collision on -- what collision filter 0 means for the reference's AbbPushBox -- this is a no-op and the step stays on
        # the run-time-shaped kernel
        be.use_split_step()
        A = sim.actors_per_env
        root = torch.zeros(n * A, 13)
        fr = torch.ones(n)
        for e, env in enumerate(sim.envs):
            for k, a in enumerate(env.actors):
                root[e * A + k, :3] = torch.tensor(tuple(a.pose.p))
                root[e * A + k, 3:7] = torch.tensor(tuple(a.pose.r))
            fr[e] = env.actors[0].friction
        root = root.to(dev)
        for tid in (_abi.T_SIM_ROOT, _abi.T_ROOT_STATE):
            be.tensors[tid].copy_(root)
        be.tensors[_abi.T_FRICTION].copy_(fr.to(dev))
        if any(env.actors[0].mass_scale is not None for env in sim.envs):
            one = np.ones(env0.actors[0].asset.num_bodies, np.float32)
            be.set_body_mass_scale(np.stack([one if env.actors[0].mass_scale is None else env.actors[0].mass_scale for env in sim.envs]))
        sim.backend = be
        if any(env.cameras for env in sim.envs):
            self._prepare_cameras(sim)
        return True

    # ---- tensors ---------------------------------------------------------------
    def _t(self, sim, tid): return _TensorHandle(sim.backend.tensors[tid])
    def acquire_dof_state_tensor(self, sim): return self._t(sim, _abi.T_DOF_STATE)
    def acquire_actor_root_state_tensor(self, sim): return self._t(sim, _abi.T_ROOT_STATE)
    def acquire_rigid_body_state_tensor(self, sim): return self._t(sim, _abi.T_BODY_STATE)
    def acquire_net_contact_force_tensor(self, sim): return self._t(sim, _abi.T_CONTACT)
    def acquire_jacobian_tensor(self, sim, name): return self._t(sim, _abi.T_JACOBIAN)
    def acquire_force_sensor_tensor(self, sim): return None

    def refresh_dof_state_tensor(self, sim): sim.backend.refresh(_abi.REFRESH_DOF)
    def refresh_actor_root_state_tensor(self, sim): sim.backend.refresh(_abi.REFRESH_ROOT)
    def refresh_rigid_body_state_tensor(self, sim):
        sim.backend.refresh(_abi.REFRESH_BODY)
        sim.body_fresh = True
    def refresh_net_contact_force_tensor(self, sim): sim.backend.refresh(_abi.REFRESH_CONTACT)
    def refresh_jacobian_tensors(self, sim):
        sim.backend.refresh(_abi.REFRESH_JACOBIAN)
        self._refresh_floating_jacobian(sim)
    def refresh_force_sensor_tensor(self, sim): pass

    def refresh_all_state_tensors(self, sim):
        """Not an Isaac Gym call: root, rigid-body, dof, Jacobian and net-contact-force tensors refreshed by ONE backend
        call (shifu's refresh_state issues the six refresh_* calls back to back, shifu/gym/isaac_gym.py:145-154)."""
        sim.backend.refresh(_abi.REFRESH_ALL)
        sim.body_fresh = True
        self._refresh_floating_jacobian(sim)

    @staticmethod
    def _floating_dynamics_enabled(sim):
        """SHIFU_AMD_FLOATING_DYNAMICS=1 (read at call time) and a floating base: the Jacobian tensor (N, nb, 6, nd + 6), the
        mass matrix (N, nd + 6, nd + 6) and the bias forces (N, nd + 6) in the order nu = (root linear, root angular, dofs) of
        csrc/shf_dyn.h (shf_sim_floating_dynamics).  Unset, every call is what it was; fixed-base sims
        are not affected either way."""
        return os.environ.get("SHIFU_AMD_FLOATING_DYNAMICS", "0") == "1" and not sim.backend.model.fixed_base

    def _refresh_floating_jacobian(self, sim):
        if self._floating_dynamics_enabled(sim):          # one more launch, for those who asked
            sim.backend.floating_dynamics(jacobian=sim.backend.tensors[_abi.T_JACOBIAN])

    def _acquire_dynamics(self, sim, attr, shape):
        import torch
        be = sim.backend
        if self._floating_dynamics_enabled(sim):
            D = be.model.nd + 6
            shape = (be.num_envs, D, D) if attr == "mass_matrix" else (be.num_envs, D)
        elif not be.model.fixed_base:
            raise NotImplementedError("mass-matrix and bias-force tensors: fixed base only (as the Jacobian tensor's dof columns)")
        if getattr(sim, attr) is None:        # allocated once per sim
            setattr(sim, attr, torch.zeros(shape, dtype=torch.float32, device=be.device))
        return _TensorHandle(getattr(sim, attr))

    def acquire_mass_matrix_tensor(self, sim, name):
        """(num_envs, nd, nd): M(q) of the articulation, armature on the diagonal (csrc/shf_dyn.h); filled by
        refresh_mass_matrix_tensors.  A floating base under SHIFU_AMD_FLOATING_DYNAMICS=1: (num_envs, nd + 6, nd + 6), root
        columns first (and the bias forces (num_envs, nd + 6))."""
        nd = sim.backend.model.nd
        return self._acquire_dynamics(sim, "mass_matrix", (sim.backend.num_envs, nd, nd))

    def acquire_dof_bias_force_tensor(self, sim, name):
        """Not an Isaac Gym call: (num_envs, nd) gravity + Coriolis + centrifugal joint forces h(q, qd), so that
        M qdd + h = tau in effort mode (gravity compensation = applying h); filled by refresh_mass_matrix_tensors."""
        return self._acquire_dynamics(sim, "dof_bias", (sim.backend.num_envs, sim.backend.model.nd))

    def refresh_mass_matrix_tensors(self, sim):
        """Fills whichever of the mass-matrix / bias-force tensors was acquired, in one launch; nothing to do otherwise."""
        if sim.mass_matrix is None and sim.dof_bias is None:
            return
        if self._floating_dynamics_enabled(sim):
            sim.backend.floating_dynamics(None, sim.mass_matrix, sim.dof_bias)
            return
        sim.backend.dynamics(sim.mass_matrix, sim.dof_bias)

    # ---- stepping --------------------------------------------------------------
    def simulate(self, sim):
        sim.body_fresh = False
        sim.backend.step()
    def fetch_results(self, sim, wait=True): pass

    def set_dof_actuation_force_tensor(self, sim, t): sim.backend.set_dof_command(_abi.T_EFFORT, t); return True
    def set_dof_position_target_tensor(self, sim, t): sim.backend.set_dof_command(_abi.T_POS_TARGET, t); return True
    def set_dof_velocity_target_tensor(self, sim, t): sim.backend.set_dof_command(_abi.T_VEL_TARGET, t); return True

    def apply_rigid_body_force_at_pos_tensors(self, sim, force, pos=None, space=ENV_SPACE):
        """force (N*B, 3) on every rigid body, at its centre of mass (pos None) or at the points pos (N*B, 3) -- both in env
        space, which here is the frame of the state tensors: the facade places every env at the sim's origin (create_env
        ignores the grid spacing -- envs never interact -- and TerrainGymEnv sets it to 0 anyway, isaac_gym.py:301)."""
        if space != ENV_SPACE:
            raise NotImplementedError("forces are taken in env (= world-aligned) axes only, the default the reference uses")
        sim.backend.apply_body_force(force, pos)
        return True

    def set_actor_root_state_tensor_indexed(self, sim, root, idx, n):
        sim.backend.commit_root_indexed(root, idx[:n]); return True
    def set_actor_root_state_tensor(self, sim, root): sim.backend.commit_root_all(root); return True
    def set_dof_state_tensor_indexed(self, sim, dof, idx, n):
        sim.backend.commit_dof_indexed(dof, idx[:n]); return True
    def set_dof_position_target_tensor_indexed(self, sim, tgt, idx, n):
        sim.backend.set_pos_target_indexed(tgt, idx[:n]); return True

    # ---- teardown ----------------------------------------------------------------
    def destroy_env(self, env): pass
    def destroy_viewer(self, viewer): pass
    def destroy_camera_sensor(self, *a): pass
    def destroy_sim(self, sim):
        if sim is not None and sim.backend is not None:
            sim.backend.destroy()
            sim.backend = None

    # ---- camera sensors (shifu_amd/render.py: one ray per pixel against the collision shapes) ---------------
    _warned_visual = False

    def create_camera_sensor(self, env: Env, props: CameraProperties):
        """Registered before prepare_sim; the handle is the camera's index within its env.  Cameras with one handle form a
        group -- one per env, one set of properties -- rendered by one launch."""
        sim = env.sim
        if sim.backend is not None:
            raise NotImplementedError("create_camera_sensor: cameras must be created before prepare_sim (the render scene is "
                                      "built there)")
        self._check_renderable_terrain(sim)
        if not props.use_collision_geometry and not Gym._warned_visual:
            Gym._warned_visual = True
            import warnings
            warnings.warn("shifu_amd: camera sensors draw the collision geometry (visual meshes are not loaded); "
                          "CameraProperties.use_collision_geometry = False is treated as True", stacklevel=2)
        env.cameras.append(_Camera(props))
        return len(env.cameras) - 1

    @staticmethod
    def _trimesh_cameras_enabled() -> bool:
        """SHIFU_AMD_TRIMESH_CAMERAS=1: camera sensors on a warped trimesh terrain (the ray caster draws it, risers
        included); refused without it, which is what callers of this facade have seen so far."""
        return os.environ.get("SHIFU_AMD_TRIMESH_CAMERAS", "0") == "1"

    @staticmethod
    def _optical_flow_enabled() -> bool:
        """SHIFU_AMD_OPTICAL_FLOW=1: camera groups also render IMAGE_OPTICAL_FLOW (shf_render_cameras_flow; DESIGN.md
        8e).  Off by default: the facade then refuses the image type as before."""
        return os.environ.get("SHIFU_AMD_OPTICAL_FLOW", "0") == "1"

    @staticmethod
    def _check_renderable_terrain(sim):
        t = sim.terrain
        if t is not None and t[0] == "heightfield" and len(t) > 6 and t[6] is not None and not Gym._trimesh_cameras_enabled():
            raise NotImplementedError("camera sensors cannot render a warped trimesh terrain (the triangle mesh "
                                      "convert_heightfield_to_trimesh makes, ShfTerrain.warped) unless "
                                      "SHIFU_AMD_TRIMESH_CAMERAS=1 is set: height fields and planes only by default")

    def set_camera_location(self, camera_handle, env: Env, position, target):
        from ..render import lookat_quat
        cam = env.cameras[camera_handle]
        cam.pos = np.array(tuple(position), float)
        cam.quat = lookat_quat(cam.pos, tuple(target))
        cam.attach = None
        self._camera_pose_update(env, camera_handle)

    def set_camera_transform(self, camera_handle, env: Env, transform: Transform):
        cam = env.cameras[camera_handle]
        cam.pos = np.array(tuple(transform.p), float)
        q = np.array(tuple(transform.r), float)
        cam.quat = q / np.linalg.norm(q)
        cam.attach = None
        self._camera_pose_update(env, camera_handle)

    def attach_camera_to_body(self, camera_handle, env: Env, body_handle, transform: Transform, follow_mode=FOLLOW_TRANSFORM):
        """body_handle: the body's row within the env's rigid-body states (articulation bodies, then one per box actor);
        the camera pose is body pose o transform at every render."""
        if follow_mode != FOLLOW_TRANSFORM:
            raise NotImplementedError("attach_camera_to_body: FOLLOW_TRANSFORM only")
        if env.sim.backend is not None:
            raise NotImplementedError("attach_camera_to_body: before prepare_sim")
        q = np.array(tuple(transform.r), float)
        env.cameras[camera_handle].attach = (int(body_handle), np.array(tuple(transform.p), float), q / np.linalg.norm(q))

    def get_camera_view_matrix(self, sim, env: Env, camera_handle):
        from ..render import view_matrix
        cam = env.cameras[camera_handle]
        pos, quat = cam.pos, cam.quat
        if cam.attach is not None and sim.backend is not None:
            pose = self._attached_poses(sim, self._group_of(sim, camera_handle))[env.index].cpu().numpy()
            pos, quat = pose[:3], pose[3:]
        return view_matrix(pos, quat).astype(np.float32)

    def get_camera_proj_matrix(self, sim, env: Env, camera_handle):
        from ..render import proj_matrix
        p = env.cameras[camera_handle].props
        return proj_matrix(p.width, p.height, p.horizontal_fov, p.near_plane, p.far_plane).astype(np.float32)

    def _prepare_cameras(self, sim):
        import torch
        from ..render import camera_struct
        self._prepare_render_scene(sim)
        be = sim.backend
        n = len(sim.envs)
        env0 = sim.envs[0]
        B = sim.cam_seg.shape[1]
        ncam = len(env0.cameras)
        sim.camera_groups = []
        for k in range(ncam):
            cams = [env.cameras[k] if k < len(env.cameras) else None for env in sim.envs]
            key = lambda c: (c.props.width, c.props.height, float(c.props.horizontal_fov), float(c.props.near_plane),
                             float(c.props.far_plane), c.attach is None)
            if any(c is None or key(c) != key(cams[0]) for c in cams) or any(len(env.cameras) != ncam for env in sim.envs):
                raise NotImplementedError("camera sensors: every env needs the same cameras (camera handle k: one per env, "
                                          "same width, height, fov, near, far, and all attached or none)")
            p = cams[0].props
            pose = torch.tensor(np.array([np.concatenate([c.pos, c.quat]) for c in cams]), dtype=torch.float32)
            g = dict(camera=camera_struct(p.width, p.height, p.horizontal_fov, p.near_plane, p.far_plane, depth_negative=True),
                     pose=pose.to(be.device), width=p.width, height=p.height,
                     depth=torch.full((n, p.height, p.width), -float("inf"), dtype=torch.float32, device=be.device),
                     seg=torch.zeros(n, p.height, p.width, dtype=torch.int32, device=be.device),
                     rgba=torch.zeros(n, p.height, p.width, 4, dtype=torch.uint8, device=be.device), attach=None)
            if cams[0].attach is not None:
                g["attach"] = (torch.tensor([e * B + c.attach[0] for e, c in enumerate(cams)], dtype=torch.long, device=be.device),
                               torch.tensor(np.array([c.attach[1] for c in cams]), dtype=torch.float32, device=be.device),
                               torch.tensor(np.array([c.attach[2] for c in cams]), dtype=torch.float32, device=be.device))
            if self._optical_flow_enabled():
                from ..render import FlowHistory
                g["flow_i16"] = torch.zeros(n, p.height, p.width, 2, dtype=torch.int16, device=be.device)
                g["history"] = FlowHistory(n, B, be.device)
            sim.camera_groups.append(g)

    def _prepare_render_scene(self, sim):
        """The render scene of a prepared sim and the per-env segmentation / color tables (sim.renderer, sim.cam_seg,
        sim.cam_color): what camera groups and the viewer draw from.  Built once."""
        if sim.renderer is not None:
            return
        import torch
        from ..render import DEFAULT_BODY_COLOR, Renderer, build_scene
        be = sim.backend
        if be.terrain.warped and not self._trimesh_cameras_enabled():
            raise NotImplementedError("camera sensors cannot render a warped trimesh terrain (ShfTerrain.warped) unless "
                                      "SHIFU_AMD_TRIMESH_CAMERAS=1 is set: height fields and planes only by default")
        env0 = sim.envs[0]
        model = env0.actors[0].asset.model
        boxes = [a.asset.box_dim for a in env0.actors[1:]]
        nb = model.blob.nb
        B = nb + len(boxes)
        hs = getattr(be, "height_samples", None) if be.terrain.rows > 0 else None
        scene = build_scene(model.render_shapes, nb, boxes, height_samples=hs, vscale=be.terrain.vscale)
        sim.renderer = Renderer(scene, be.terrain, be._heights if be.terrain.rows > 0 else None, be.device)
        n = len(sim.envs)
        row = lambda a, b: b if a == 0 else nb + a - 1
        seg = torch.zeros(n, B, dtype=torch.int32)
        col = torch.tensor(DEFAULT_BODY_COLOR, dtype=torch.float32).repeat(n, B, 1)
        for e, env in enumerate(sim.envs):
            for (a, b), v in env.seg_ids.items():
                seg[e, row(a, b)] = v
            for (a, b), v in env.colors.items():
                col[e, row(a, b)] = torch.tensor(v)
        sim.cam_seg, sim.cam_color = seg.to(be.device), col.to(be.device)

    def _group_of(self, sim, camera_handle):
        return sim.camera_groups[camera_handle]

    def _attached_poses(self, sim, g):
        """(N, 7) poses of a group attached to bodies: body pose o local transform, from the body-state tensor."""
        import torch
        from .torch_utils import quat_apply, quat_mul
        rows, lp, lq = g["attach"]
        bs = sim.backend.tensors[_abi.T_BODY_STATE].index_select(0, rows)
        return torch.cat([bs[:, :3] + quat_apply(bs[:, 3:7], lp), quat_mul(bs[:, 3:7], lq)], dim=1)

    def _camera_pose_update(self, env: Env, camera_handle):
        sim = env.sim
        if sim.backend is None or not sim.camera_groups:
            return
        import torch
        cam = env.cameras[camera_handle]
        row = np.concatenate([cam.pos, cam.quat]).astype(np.float32)
        sim.camera_groups[camera_handle]["pose"][env.index].copy_(torch.from_numpy(row))

    def _camera_table_update(self, env: Env, actor_handle, body):
        sim = env.sim
        if sim.backend is None or sim.renderer is None:
            return
        import torch
        from ..render import DEFAULT_BODY_COLOR
        r = int(body) if int(actor_handle) == 0 else sim.robot_asset.num_bodies + int(actor_handle) - 1
        sim.cam_seg[env.index, r] = env.seg_ids.get((int(actor_handle), int(body)), 0)
        sim.cam_color[env.index, r] = torch.tensor(env.colors.get((int(actor_handle), int(body)), DEFAULT_BODY_COLOR))

    def render_camera_group(self, sim, camera_handle):
        """Not an Isaac Gym call: renders one camera group (camera handle k of every env) -- one launch."""
        if sim.renderer is None:
            return
        if not sim.body_fresh:
            self.refresh_rigid_body_state_tensor(sim)
        g = sim.camera_groups[camera_handle]
        pose = g["pose"] if g["attach"] is None else self._attached_poses(sim, g).contiguous()
        bs = sim.backend.tensors[_abi.T_BODY_STATE]
        h = g.get("history")
        if h is not None:
            # with optical flow (SHIFU_AMD_OPTICAL_FLOW=1): against the poses of this group's previous render, which this
            # one then replaces -- preallocated tensors, no host sync
            sim.renderer.render(bs, pose, sim.cam_seg, sim.cam_color, g["camera"], depth=g["depth"], seg_out=g["seg"],
                                rgba=g["rgba"], flow_i16=g["flow_i16"], **h.tensors())
            h.update(bs, pose)
            return
        sim.renderer.render(bs, pose, sim.cam_seg, sim.cam_color, g["camera"],
                            depth=g["depth"], seg_out=g["seg"], rgba=g["rgba"])

    def invalidate_camera_flow(self, sim, camera_handle, env_ids=None):
        """Not an Isaac Gym call: the group's next render shows zero optical flow in env_ids (all envs by default) -- after a
        reset or any teleport, when the previous render's poses say nothing about motion.  Nothing to do without
        SHIFU_AMD_OPTICAL_FLOW=1."""
        if not sim.camera_groups:
            return
        h = sim.camera_groups[camera_handle].get("history")
        if h is not None:
            h.invalidate(env_ids)

    def render_all_camera_sensors(self, sim):
        """One launch per camera group, on the state of the last simulate (the rigid-body states are refreshed first when
        they have not been since)."""
        for k in range(len(sim.camera_groups)):
            self.render_camera_group(sim, k)

    def get_camera_image_gpu_tensor(self, sim, env: Env, camera_handle, image_type):
        """Zero-copy view of row env of the group's image: IMAGE_COLOR (H, W, 4) u8 RGBA, IMAGE_DEPTH (H, W) f32 (minus the
        view-space depth, -inf where nothing is hit), IMAGE_SEGMENTATION (H, W) int32.  IMAGE_OPTICAL_FLOW, under
        SHIFU_AMD_OPTICAL_FLOW=1 only: (H, W, 2) int16, (u, v) x 32768 / (W, H) (render.flow_from_i16 gives pixels)."""
        if image_type == IMAGE_OPTICAL_FLOW and not (self._optical_flow_enabled() and (
                not sim.camera_groups or "flow_i16" in sim.camera_groups[camera_handle])):
            # (also a sim prepared without the variable: its groups hold no flow image)
            raise NotImplementedError("IMAGE_OPTICAL_FLOW is not rendered by this backend (depth, segmentation and color are) "
                                      "unless SHIFU_AMD_OPTICAL_FLOW=1 is set")
        if not sim.camera_groups:
            raise RuntimeError("get_camera_image_gpu_tensor: no camera sensors (create them before prepare_sim)")
        g = sim.camera_groups[camera_handle]
        key = {IMAGE_COLOR: "rgba", IMAGE_DEPTH: "depth", IMAGE_SEGMENTATION: "seg", IMAGE_OPTICAL_FLOW: "flow_i16"}.get(image_type)
        if key is None:
            raise ValueError(f"get_camera_image_gpu_tensor: unknown image type {image_type}")
        return _TensorHandle(g[key][env.index])

    def camera_group_tensors(self, sim, camera_handle):
        """Not an Isaac Gym call: the group's (N, H, W[, 4]) images -- dict(rgba=, depth=, seg=) -- for all envs at once; under
        SHIFU_AMD_OPTICAL_FLOW=1 also flow=, the (N, H, W, 2) int16 optical flow."""
        g = sim.camera_groups[camera_handle]
        out = dict(rgba=g["rgba"], depth=g["depth"], seg=g["seg"])
        if "flow_i16" in g:
            out["flow"] = g["flow_i16"]
        return out

    def camera_group_points(self, sim, camera_handle, world_frame=True):
        """Not an Isaac Gym call: the (N, H, W, 3) f32 point behind every pixel of the group's last rendered depth image
        (shf_camera_points), in the frame of the state tensors on the group's poses as they are now, or with
        world_frame=False in the camera's own axes.  One launch into a tensor the group keeps; no host sync."""
        import torch
        g = sim.camera_groups[camera_handle]
        key = "points_w" if world_frame else "points_c"
        if key not in g:
            g[key] = torch.zeros(len(sim.envs), g["height"], g["width"], 3, dtype=torch.float32, device=sim.backend.device)
        pose = g["pose"] if g["attach"] is None else self._attached_poses(sim, g).contiguous()
        sim.renderer.camera_points(g["depth"], pose, g["camera"], g[key], world_frame)
        return g[key]

    # ---- ray-caster sensors (shifu_amd/raycast.py: arbitrary rays against the collision shapes and the terrain) -----------
    def create_ray_caster_group(self, sim, pattern, position=(0.0, 0.0, 0.0), quat=(0.0, 0.0, 0.0, 1.0), attach_body=None,
                                align="base", min_range=0.0, max_range=10.0, ignore_bodies=()):
        """Not an Isaac Gym call: a ray-caster sensor in every env -- pattern = (origins (R, 3), dirs (R, 3)) in the sensor
        frame, the sensor at (position, quat xyzw) in the frame of the state tensors or, with attach_body (a row of the
        env's rigid-body states), in that body's frame.  AFTER prepare_sim, unlike cameras: it is built on the render
        scene, which the sim builds on first use (a warped trimesh terrain: behind SHIFU_AMD_TRIMESH_CAMERAS=1, as for
        cameras).  ignore_bodies: rigid-body rows the rays pass through.  Returns the group's handle; its tensors --
        dist (N, R) f32, points (N, R, 3) f32 -- are sim.ray_caster_groups[handle]["dist" / "points"]."""
        import torch
        from ..raycast import ALIGN, check_pattern
        from ..render import shape_mask_for
        if sim.backend is None:
            raise NotImplementedError("create_ray_caster_group: after prepare_sim (the render scene is built from the prepared sim)")
        self._prepare_render_scene(sim)
        o, d = check_pattern(*pattern)
        if align not in ALIGN:
            raise ValueError(f"create_ray_caster_group: align must be one of {sorted(ALIGN)}, got {align!r}")
        if not (0.0 <= float(min_range) <= float(max_range) and np.isfinite(float(max_range))):
            raise ValueError("create_ray_caster_group: need 0 <= min_range <= max_range, max_range finite")
        dev, n, B = sim.backend.device, len(sim.envs), sim.cam_seg.shape[1]
        q = np.asarray(tuple(quat), float)
        local = torch.tensor(np.concatenate([np.asarray(tuple(position), float), q / np.linalg.norm(q)]), dtype=torch.float32)
        g = dict(origins=torch.from_numpy(o).to(dev), dirs=torch.from_numpy(d).to(dev), num_rays=int(o.shape[0]), align=align,
                 min_range=float(min_range), max_range=float(max_range), shape_mask=shape_mask_for(sim.renderer.scene, ignore_bodies),
                 pose=local.repeat(n, 1).to(dev).contiguous(), attach=None,
                 dist=torch.full((n, o.shape[0]), float("inf"), dtype=torch.float32, device=dev),
                 points=torch.zeros(n, o.shape[0], 3, dtype=torch.float32, device=dev))
        if attach_body is not None:
            if not 0 <= int(attach_body) < B:
                raise ValueError(f"create_ray_caster_group: attach_body {attach_body} outside the env's {B} rigid-body rows")
            g["attach"] = (torch.arange(n, dtype=torch.long, device=dev) * B + int(attach_body), g["pose"][:, :3].contiguous(),
                           g["pose"][:, 3:].contiguous())
            g["pose"] = torch.zeros(n, 7, dtype=torch.float32, device=dev)
        sim.ray_caster_groups.append(g)
        return len(sim.ray_caster_groups) - 1

    def cast_ray_caster_group(self, sim, handle):
        """Not an Isaac Gym call: casts one ray-caster group (every env, one launch) on the state of the last simulate -- the
        rigid-body states are refreshed first when they have not been since, as render_camera_group does -- into the
        group's dist / points tensors, which it returns as a dict.  No host sync."""
        if not sim.body_fresh:
            self.refresh_rigid_body_state_tensor(sim)
        g = sim.ray_caster_groups[handle]
        if g["attach"] is not None:
            g["pose"].copy_(self._attached_poses(sim, g))
        sim.renderer.raycast(sim.backend.tensors[_abi.T_BODY_STATE], g["pose"], g["origins"], g["dirs"], g["align"],
                             g["min_range"], g["max_range"], g["shape_mask"], dist=g["dist"], points=g["points"])
        return dict(dist=g["dist"], points=g["points"])

    # ---- graphics: accepted and ignored by default (no window on this path).  SHIFU_AMD_VIEWER=<directory> opts into the
    # headless viewer (shifu_amd/viewer.py): create_viewer then returns a Viewer -- one camera over all envs, laid out on
    # create_env's grid --, draw_viewer renders it and write_viewer_image_to_file writes a PNG; IsaacGymEnv.render() numbers
    # its frames into that directory.  Unset, every call below is the no-op it has always been.
    @staticmethod
    def _viewer_directory() -> Optional[str]:
        return os.environ.get("SHIFU_AMD_VIEWER") or None

    def create_viewer(self, sim=None, props=None, *a, **k):
        if self._viewer_directory() is None or sim is None:
            return None
        from ..viewer import Viewer
        if not sim.envs:
            raise RuntimeError("create_viewer: create the envs first (the viewer is laid out on create_env's grid)")
        self._check_renderable_terrain(sim)
        p = props if props is not None else CameraProperties()
        sx, sy, per_row = sim.env_grid
        grid = sx != 0.0 or sy != 0.0

        def source():
            # the first draw: the sim is on the device by now, and so are its scene and tables (shared with the cameras)
            if sim.backend is None:
                raise RuntimeError("draw_viewer: prepare_sim first")
            self._prepare_render_scene(sim)
            return sim.renderer, sim.backend.tensors[_abi.T_BODY_STATE], sim.cam_seg, sim.cam_color

        v = Viewer(None, len(sim.envs), None, None, None, int(p.width), int(p.height), float(p.horizontal_fov),
                   max(float(p.near_plane), 1e-3), min(float(p.far_plane), 1e4), layout="grid" if grid else "world",
                   spacing=(sx, sy), per_row=per_row, source=source)
        v.sim = sim
        return v

    def subscribe_viewer_keyboard_event(self, *a, **k): pass

    def viewer_camera_look_at(self, viewer=None, env=None, pos=None, target=None, *a, **k):
        """pos / target: world coordinates with env None, else relative to where the viewer puts that env."""
        if viewer is None:
            return
        off = np.zeros(3) if env is None else viewer.env_offset(env.index)
        viewer.look_at(np.array(tuple(pos), float) + off, np.array(tuple(target), float) + off)

    def query_viewer_has_closed(self, viewer): return False
    def query_viewer_action_events(self, viewer): return []
    def step_graphics(self, sim): pass

    def draw_viewer(self, viewer=None, sim=None, *a, **k):
        if viewer is None:
            return
        s = viewer.sim
        if s.backend is not None and not s.body_fresh:
            self.refresh_rigid_body_state_tensor(s)
        viewer.draw()

    def write_viewer_image_to_file(self, viewer, path):
        """Isaac Gym's name: the viewer's last drawn color image as a PNG (a host copy: it waits for the draw)."""
        if viewer is None:
            return
        from ..viewer import write_png
        if viewer.images is None:
            self.draw_viewer(viewer)
        write_png(path, viewer.images["rgba"].cpu().numpy())

    def sync_frame_time(self, sim): pass
    def poll_viewer_events(self, viewer): pass
    def set_light_parameters(self, *a, **k): pass
    def start_access_image_tensors(self, sim): pass
    def end_access_image_tensors(self, sim): pass


_GYM = None


def acquire_gym() -> Gym:
    global _GYM
    if _GYM is None:
        _GYM = Gym()
    return _GYM


Sim = SimHandle  # `gymapi.Sim` is used as a type annotation by the reference (units.py:13)
