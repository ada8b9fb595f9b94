"""Camera-sensor benchmark: the vision stage's camera (reference examples/abb_pushbox_vision/task_config.py:124-145 --
128 x 128, horizontal FOV 42, near 0.1, far 3, looking from (0.7, 0, 0.7) at (0, 0, 0.1), color + depth + segmentation)
on the ABB push-box scene through the gym facade and CameraSensor.  Times the render launch alone with device events
over --renders renders after warm-up, and prints one JSON line.

    python tools/bench_camera.py --envs 1000

--scene a1-heightfield / a1-trimesh: FusedA1Env on that terrain with a trunk-mounted 64 x 48 camera (depth, segmentation
and color; fov 87, near 0.05, far 6, pitched 0.5 rad down) after a reset and a few random steps -- the walk over the height
field against the walk over the warped trimesh on the same samples.

    python tools/bench_camera.py --scene a1-trimesh --envs 4096

--flow: the same launch with and without optical flow (shf_render_cameras_flow writing the int16 flow image on top of the
three others, against a previous frame one env step older, valid in every env), alternating --repeats times in one session;
reports both medians and their ratio.

    python tools/bench_camera.py --envs 1000 --flow

--scene world: the headless viewer's world-view launch at 640 x 360 over --envs A1 robots on the height field, with and
without the env-level cull, against the batched per-env render followed by a torch min composite (bench_world).

    python tools/bench_camera.py --scene world --envs 4096

--rays grid / lidar / pinhole (with --scene a1-heightfield, a1-trimesh or abb): the ray caster (shf_raycast) on FusedA1Env or
FusedAbbEnv after a reset and a few random steps, timed in interleaved blocks (--repeats), median [min .. max] ms.  pinhole:
the 64 x 48, fov 87 pinhole pattern writing `dist` only against shf_render_cameras writing depth only from the same poses --
the same rays, so the ratio is what arbitrary rays cost.  grid: the A1 height scan (17 x 11 rays under the trunk, yaw-aligned,
the robot ignored, max_range 3), beside shf_get_heights on the same envs and points.  lidar: 16 x 360 rays from the trunk /
the end effector, the articulation ignored.

    python tools/bench_camera.py --scene a1-trimesh --envs 4096 --rays grid
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

TARGET_MS = 1.0     # per render at 1000 envs, all three images


def vision_env_class():
    """(env class, env config class): the push-box scene of stage a with the vision stage's camera added."""
    import torch
    from shifu_amd import compat
    compat.install()
    from isaacgym import gymapi as ga
    from shifu.configs import CameraSensorConfig
    from shifu.units import CameraSensor
    from examples.abb_pushbox_vision.a_prior_stage import AbbPushBox, AbbRobot, GoalBox, RandPosBox
    from examples.abb_pushbox_vision.task_config import AbbRobotConfig, GoalBoxConfig, PriorStageEnvConfig, PushBoxConfig, TableConfig
    from shifu_amd.gym import ShifuVecEnv
    from shifu_amd.units import Box

    class PushBoxCameraConfig(CameraSensorConfig):
        name = 'rgbd_camera'
        local_lookat_positions = [[0.7, 0., 0.7], [0., 0., 0.1]]
        image_types = [ga.IMAGE_COLOR, ga.IMAGE_DEPTH, ga.IMAGE_SEGMENTATION]
        image_normalization = True

        class camera_props(CameraSensorConfig.camera_props):
            width, height, horizontal_fov, near_plane, far_plane = 128, 128, 42, 0.1, 3

    class AbbPushBoxVision(AbbPushBox):
        def __init__(self, cfg):
            ShifuVecEnv.__init__(self, cfg)
            self.robot = AbbRobot(AbbRobotConfig())
            self.table, self.cube, self.goal = Box(TableConfig()), RandPosBox(PushBoxConfig()), GoalBox(GoalBoxConfig())
            self.camera = CameraSensor(PushBoxCameraConfig())
            self.isg_env.create_envs(robot=self.robot, objects=[self.table, self.cube, self.goal], sensors=[self.camera])
            self.success_buf = torch.zeros(self.num_envs, device=self.device, dtype=torch.float)

    return AbbPushBoxVision, PriorStageEnvConfig


def make_env(n):
    env_class, cfg_class = vision_env_class()
    cfg = cfg_class()
    cfg.num_envs = n
    return env_class(cfg)


def time_renders(render, warmup, renders):
    """ms per call of render(), by device events."""
    import torch
    for _ in range(warmup):
        render()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(renders):
        render()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / renders


def flow_on_off(render_off, render_on, a):
    """{"ms_flow_off": median, "ms_flow_on": median, ...}: the two launches timed alternately, a.repeats times each."""
    import statistics
    off, on = [], []
    for _ in range(a.repeats):
        off.append(time_renders(render_off, a.warmup, a.renders))
        on.append(time_renders(render_on, a.warmup, a.renders))
    m_off, m_on = statistics.median(off), statistics.median(on)
    return dict(flow=True, repeats=a.repeats, ms_flow_off=round(m_off, 4), ms_flow_on=round(m_on, 4),
                flow_on_over_off=round(m_on / m_off, 4), ms_flow_off_runs=[round(v, 4) for v in off],
                ms_flow_on_runs=[round(v, 4) for v in on], flow_bytes_written_extra_per_ray=4)


def bench_a1(a):
    import math
    import torch
    from shifu_amd.gym.a1_fused import FusedA1Env
    terrain = a.scene[len("a1-"):]
    env = FusedA1Env(num_envs=a.envs, terrain=terrain)
    W, H = 64, 48
    cam = env.add_camera(W, H, 87.0, 0.05, 6.0, position=(0.25, 0.0, 0.05), quat=(0.0, math.sin(0.25), 0.0, math.cos(0.25)),
                         attach_body=0)
    env.cam_seg.fill_(1)                        # the robot; the terrain is segmentation 0
    env.reset()
    g = torch.Generator().manual_seed(0)
    from shifu_amd.render import FlowHistory
    hist = FlowHistory(env.num_envs, env.cam_seg.shape[1], env.device)
    for k in range(3):
        if k == 2:
            hist.update(env.body_state, cam.world_pose())          # --flow: the previous frame, one step older
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    # the attached pose is composed once: the timed call is the render launch alone, as in the default scene
    pose, im = cam.world_pose(), cam.raw_images()
    render = lambda: env._renderer.render(env.body_state, pose, env.cam_seg, env.cam_color, cam.camera, depth=im["depth"],
                                          seg_out=im["seg"], rgba=im["rgba"])
    flow_out = {}
    if a.flow:
        q = torch.zeros(env.num_envs, H, W, 2, dtype=torch.int16, device=env.device)
        render_on = lambda: env._renderer.render(env.body_state, pose, env.cam_seg, env.cam_color, cam.camera, depth=im["depth"],
                                                 seg_out=im["seg"], rgba=im["rgba"], flow_i16=q, **hist.tensors())
        flow_out = flow_on_off(render, render_on, a)
        flow_out["pixels_with_flow"] = round(float(q.ne(0).any(-1).float().mean()), 4)
    ms = time_renders(render, a.warmup, a.renders)
    rays = a.envs * W * H
    hit = torch.isfinite(im["depth"])
    out = dict(bench="camera_render", scene=a.scene, envs=a.envs, width=W, height=H,
               image_types=["color", "depth", "segmentation"], renders=a.renders, ms_per_render=round(ms, 4),
               rays_per_s=round(rays / (ms * 1e-3), 1), bytes_written=rays * 12,
               write_gb_per_s=round(rays * 12 / (ms * 1e-3) / 1e9, 1),
               pixels_on_terrain=round(float((hit & (im["seg"] == 0)).float().mean()), 4),
               pixels_hit=round(float(hit.float().mean()), 4), warped=int(env.sim.terrain.warped),
               device=torch.cuda.get_device_name(0))
    out.update(flow_out)
    print(json.dumps(out))
    env.destroy()


def bench_rays(a):
    """--rays: see the module docstring.  One JSON line; every timed call is the launch alone (poses composed once)."""
    import math
    import statistics
    import torch
    from shifu_amd.raycast import grid_pattern, lidar_pattern, pinhole_pattern
    a1 = a.scene.startswith("a1-")
    if a1:
        from shifu_amd.gym.a1_fused import FusedA1Env
        env = FusedA1Env(num_envs=a.envs, terrain=a.scene[len("a1-"):])
        actions, body = env.num_actions, 0
        cam_kw = dict(position=(0.25, 0.0, 0.05), quat=(0.0, math.sin(0.25), 0.0, math.cos(0.25)), attach_body=0)
    else:
        from shifu_amd.gym.abb_fused import FusedAbbEnv
        env = FusedAbbEnv(num_envs=a.envs, seed=0)
        actions, body = 3, int(env.task_params.ee_body)
        cam_kw = dict(position=(0.7, 0.0, 0.7), target=(0.0, 0.0, 0.1))
    W, H, FOV, NEAR, FAR = 64, 48, 87.0, 0.05, 6.0
    cam = env.add_camera(W, H, FOV, NEAR, FAR, **cam_kw)
    if a.rays == "pinhole":
        o, d = pinhole_pattern(W, H, FOV)
        lim = float(FAR * (d.astype("float64") ** 2).sum(1).max() ** 0.5)          # every surface the camera shows is in range
        rc = env.add_ray_caster((o, d), align="base", min_range=NEAR, max_range=lim, outputs=("dist",),
                                **{k: v for k, v in cam_kw.items() if k != "target"},
                                **({} if a1 else {"quat": cam.pose[0, 3:].cpu().numpy()}))
    elif a.rays == "grid":
        rc = env.add_ray_caster(grid_pattern(), position=(0.0, 0.0, 0.5) if a1 else (0.45, 0.0, 1.0), attach_body=0 if a1 else None,
                                align="yaw", ignore_bodies="articulation", max_range=3.0, outputs=("dist", "points"))
    else:
        rc = env.add_ray_caster(lidar_pattern(16, (-15.0, 15.0), horizontal_res=1.0), position=(0.0, 0.0, 0.2 if a1 else 0.0),
                                attach_body=body, align="base", ignore_bodies="articulation", min_range=0.05, max_range=10.0,
                                outputs=("dist", "points"))
    env.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        env.step((2 * torch.rand(env.num_envs, actions, generator=g) - 1).to(env.device))
    r, o_ = env._renderer, rc._out
    pose = rc.world_pose().clone()
    cast = lambda: r.raycast(env.body_state, pose, rc.origins, rc.dirs, rc.align, rc.min_range, rc.max_range, rc.shape_mask,
                             dist=o_.get("dist"), points=o_.get("points"))
    runs = {"raycast": cast}
    if a.rays == "pinhole":
        cpose, im = cam.world_pose().clone(), cam.raw_images()
        runs["camera_depth_only"] = lambda: r.render(env.body_state, cpose, env.cam_seg, env.cam_color, cam.camera, depth=im["depth"])
    if a.rays == "grid" and a1 and env.sim.terrain.rows > 0:
        import copy
        from shifu_amd import glue
        t = copy.copy(env.sim.terrain)
        nv = int(t.rows) * int(t.cols)
        samples = env.sim._heights[:nv].view(int(t.rows), int(t.cols))
        pts = rc.origins[:, :2].contiguous()
        runs["get_heights"] = lambda: glue.get_heights(t, samples, env.root_state, None, pts, env.num_envs)
    ms = {k: [] for k in runs}
    for _ in range(a.repeats):
        for k, fn in runs.items():
            ms[k].append(time_renders(fn, a.warmup, a.renders))
    cast()
    torch.cuda.synchronize()
    dist = o_["dist"]
    n_rays = env.num_envs * rc.num_rays
    out = dict(bench="raycast", rays=a.rays, scene=a.scene if a1 else "abb_pushbox", envs=a.envs, rays_per_env=rc.num_rays,
               outputs=sorted(o_), renders=a.renders, repeats=a.repeats, warped=int(env.sim.terrain.warped),
               shapes=int(r.scene.nshapes), shapes_cast=bin(rc.shape_mask).count("1"),
               rays_hit=round(float(torch.isfinite(dist).float().mean()), 4), device=torch.cuda.get_device_name(0))
    for k, xs in ms.items():
        out["ms_" + k] = dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4),
                              runs=[round(x, 4) for x in xs])
    med = statistics.median(ms["raycast"])
    out["rays_per_s"] = round(n_rays / (med * 1e-3), 1)
    if "camera_depth_only" in ms:
        out["raycast_over_camera"] = round(med / statistics.median(ms["camera_depth_only"]), 4)
        both = torch.isfinite(im["depth"].view(env.num_envs, -1)) & torch.isfinite(dist)
        norm = rc.dirs.norm(dim=1)[None, :]
        # (the camera writes minus the view depth; a ray on a silhouette may fall on either side of it: a fraction, not a maximum)
        diff = ((dist / norm) + im["depth"].view(env.num_envs, -1))[both].abs()
        out["rays_differing_over_1mm"] = round(float((diff > 1e-3).float().mean()), 6)
    print(json.dumps(out))
    env.destroy()


def bench_world(a):
    """--scene world: the headless viewer's launch (shf_render_world) alone, 640 x 360, on FusedA1Env's height field with
    --envs robots, from a camera behind env 0 that looks over its neighbours -- with the env-level cull (env_radius from
    the model) and without.  Baseline: what could be done before -- shf_render_cameras batched over the envs, every env's
    camera at the viewer's pose minus its offset (here zero: the envs are apart on the terrain), then a torch min over the
    envs' depth images and a gather of the color.  All three are timed in interleaved blocks, --repeats times each;
    reported as median [min .. max] ms."""
    import statistics
    import torch
    from shifu_amd.gym.a1_fused import FusedA1Env
    from shifu_amd.render import camera_struct
    W, H = 640, 360
    env = FusedA1Env(num_envs=a.envs, terrain="heightfield")
    env.cam_seg.fill_(1)
    v = env.add_viewer(W, H, 90.0, 0.05, 100.0)
    env.reset()
    g = torch.Generator().manual_seed(0)
    for _ in range(3):
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    v.follow(0, body=0, offset=(-3.0, -3.0, 2.5))
    im = v.draw()
    d = v._dev
    r, N = env._renderer, env.num_envs
    world = lambda radius: r.render_world(d["body_state"], d["pose"], d["seg"], d["color"], d["camera"], env_ids=d["env_ids"],
                                          env_radius=radius, depth=d["depth"], rgba=d["rgba"])
    # the baseline's buffers: one image per env
    pose = d["pose"].repeat(N, 1).contiguous()
    cam = camera_struct(W, H, 90.0, 0.05, 100.0)
    bd = torch.empty(N, H, W, device=env.device)
    bc = torch.empty(N, H, W, 4, dtype=torch.uint8, device=env.device)

    def baseline():
        r.render(env.body_state, pose, env.cam_seg, env.cam_color, cam, depth=bd, rgba=bc)
        depth, first = bd.min(0)
        return depth, torch.gather(bc.view(torch.int32).view(N, H, W), 0, first.unsqueeze(0))[0]

    depth0, color0 = baseline()
    torch.cuda.synchronize()
    same_depth = bool(torch.equal(depth0, d["depth"][0]))
    same_color = bool(torch.equal(color0, d["rgba"][0].view(torch.int32).view(H, W)))
    runs = {"world_cull_off": [], "world_cull_on": [], "baseline_batched_min": []}
    slow = max(3, a.renders // 20)
    for _ in range(a.repeats):
        runs["world_cull_off"].append(time_renders(lambda: world(0.0), a.warmup, a.renders))
        runs["world_cull_on"].append(time_renders(lambda: world(v.env_radius), a.warmup, a.renders))
        runs["baseline_batched_min"].append(time_renders(baseline, 1, slow))
    world(v.env_radius)
    torch.cuda.synchronize()
    env_seen = int((torch.unique(v.draw()["env"]) >= 0).sum())
    out = dict(bench="world_view", scene="a1-heightfield", envs=N, width=W, height=H, renders=a.renders, repeats=a.repeats,
               baseline_renders=slow, env_radius=round(v.env_radius, 4), envs_in_view=env_seen,
               pixels_on_robots=round(float((im["env"] >= 0).float().mean()), 4),
               baseline_depth_bit_equal=same_depth, baseline_color_bit_equal=same_color, device=torch.cuda.get_device_name(0))
    for k, xs in runs.items():
        out["ms_" + k] = dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4),
                              runs=[round(x, 4) for x in xs])
    print(json.dumps(out))
    env.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1000)
    ap.add_argument("--renders", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--scene", choices=["abb", "a1-heightfield", "a1-trimesh", "world"], default="abb")
    ap.add_argument("--flow", action="store_true", help="also time the launch with optical flow, alternating with the one without")
    ap.add_argument("--repeats", type=int, default=3, help="--flow / --rays / --scene world: timed runs of each form")
    ap.add_argument("--rays", choices=["grid", "lidar", "pinhole"], default=None,
                    help="time the ray caster with this pattern (scenes a1-heightfield, a1-trimesh, abb)")
    a = ap.parse_args()
    if a.rays is not None:
        if a.scene == "world":
            ap.error("--rays needs --scene a1-heightfield, a1-trimesh or abb")
        return bench_rays(a)
    if a.scene == "world":
        return bench_world(a)
    if a.scene != "abb":
        return bench_a1(a)
    import torch
    env = make_env(a.envs)
    env.reset()
    g = torch.Generator().manual_seed(0)
    gym, sim, cam = env.isg_env.gym, env.isg_env.sim, env.camera
    from shifu_amd import _abi
    from shifu_amd.render import FlowHistory
    grp = sim.camera_groups[cam.camera_handle]
    bs = sim.backend.tensors[_abi.T_BODY_STATE]
    hist = FlowHistory(a.envs, sim.cam_seg.shape[1], bs.device)
    for k in range(3):
        if k == 2:
            hist.update(bs, grp["pose"])                            # --flow: the previous frame, one step older
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    flow_out = {}
    if a.flow:
        q = torch.zeros(a.envs, cam.height, cam.width, 2, dtype=torch.int16, device=bs.device)
        gym.refresh_rigid_body_state_tensor(sim)
        render_off = lambda: sim.renderer.render(bs, grp["pose"], sim.cam_seg, sim.cam_color, grp["camera"], depth=grp["depth"],
                                                 seg_out=grp["seg"], rgba=grp["rgba"])
        render_on = lambda: sim.renderer.render(bs, grp["pose"], sim.cam_seg, sim.cam_color, grp["camera"], depth=grp["depth"],
                                                seg_out=grp["seg"], rgba=grp["rgba"], flow_i16=q, **hist.tensors())
        flow_out = flow_on_off(render_off, render_on, a)
        flow_out["pixels_with_flow"] = round(float(q.ne(0).any(-1).float().mean()), 4)
    for _ in range(a.warmup):
        gym.render_camera_group(sim, cam.camera_handle)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.renders):
        gym.render_camera_group(sim, cam.camera_handle)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.renders
    W, H = cam.width, cam.height
    rays = a.envs * W * H
    seg = cam.segmentation_buf
    out = dict(bench="camera_render", scene="abb_pushbox_vision", envs=a.envs, width=W, height=H,
               image_types=["color", "depth", "segmentation"], renders=a.renders, ms_per_render=round(ms, 4),
               rays_per_s=round(rays / (ms * 1e-3), 1), bytes_written=rays * (4 + 4 + 4),
               write_gb_per_s=round(rays * 12 / (ms * 1e-3) / 1e9, 1), target_ms=TARGET_MS,
               pixels_on_cube=round(float((seg == env.cube.segmentation_id).float().mean()), 4),
               pixels_on_arm=round(float((seg == env.robot.segmentation_id).float().mean()), 4),
               device=torch.cuda.get_device_name(0))
    if a.envs == 1000:
        out["meets_target"] = bool(ms <= TARGET_MS)
    out.update(flow_out)
    print(json.dumps(out))
    env.destroy()


if __name__ == "__main__":
    main()
