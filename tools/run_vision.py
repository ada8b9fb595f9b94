"""The vision pipeline on the ABB push-box scene end to end, on env and dataset classes of this tool's own:

    stage b   trains the CNN regressor (camera images -> object, goal and end-effector xy) for --steps batches of --batch
              envs through run_module / ModuleRunner (torch autograd), then measures its per-key RMSE in metres on fresh data
    stage c   PPO for --iterations iterations on --envs envs whose observations are that regressor's predictions, computed
              by the fused HIP forward (--torch-obs: by the torch modules); also times the env step with either forward

The images come from tools/bench_camera.py's scene (stage a's push-box env plus the 128 x 128 camera) left running: every
env keeps a random heading for --hold items, so that the arm travels over its workspace instead of jittering around its
home pose, and a --respawn share of the envs is reset before every item, which places their cube and goal pad anew.

Prints one JSON line with the wall times, the RMSE and the step times.

    python tools/run_vision.py --steps 300 --batch 128 --iterations 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KEYS = ("obj_pos", "goal_pos", "ee_pos")
MODEL_NAME = "push_box_regressor"


def make_regressor(device="cuda:0"):
    from bench_vision import make_regressor as full_size
    return full_size(device).train()


def camera_views(camera):
    """The sensor's images as the (N, C, H, W) views the regressor takes; no copy."""
    return {"rgb": camera.color_buf.permute(0, 3, 1, 2), "depth": camera.depth_buf.unsqueeze(1)}


def stage_classes(hold, respawn):
    """(dataset class, stage-c env class, env config class, PPO config class)."""
    import torch
    from bench_camera import vision_env_class
    from examples.abb_pushbox_vision.task_config import PriorStagePPOConfig
    from shifu_amd.utils.data import ShifuDataset
    PushBoxVision, EnvCfg = vision_env_class()

    class LabelledImages(ShifuDataset):
        """Item = ({'rgb', 'depth'} views of the camera buffers, {key: (N, 2) xy in metres}) after one more env step."""

        def __init__(self, batch_size, num_data):
            super().__init__(PushBoxVision, EnvCfg(), batch_size, num_data)
            self.heading = None

        def __getitem__(self, index):
            self.end_if_past(index)
            env = self.env
            if index % hold == 0 or self.heading is None:
                self.heading = self.random_actions(-env.clip_actions, env.clip_actions)
            again = (torch.rand(env.num_envs, device=env.device) < respawn).nonzero().flatten()
            env.reset_idx(again)
            env.step(self.heading)
            where = {"obj_pos": env.cube.base_pose, "goal_pos": env.goal.base_pose, "ee_pos": env.robot.ee_pose[:, 0]}
            return camera_views(env.camera), {k: v[:, :2].detach().clone() for k, v in where.items()}

    class RegressedObsPushBox(PushBoxVision):
        """The same scene and task; the policy sees the regressor's six numbers instead of the simulator's."""
        regressor = None        # assigned before the first step; until then the privileged observations stand in

        def compute_observations(self):
            if self.regressor is None:
                return super().compute_observations()
            with torch.no_grad():
                pred = self.regressor(camera_views(self.camera))
            self.obs_buf = torch.cat([pred[k].detach() for k in KEYS], dim=1)

    class StageCPPOConfig(PriorStagePPOConfig):
        class runner(PriorStagePPOConfig.runner):
            run_name = "regressed_observations"

    return LabelledImages, RegressedObsPushBox, EnvCfg, StageCPPOConfig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300, help="stage b: training batches")
    ap.add_argument("--batch", type=int, default=128, help="stage b: envs per batch")
    ap.add_argument("--eval-batches", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5, help="stage c: PPO iterations")
    ap.add_argument("--envs", type=int, default=1000, help="stage c: envs")
    ap.add_argument("--timed-steps", type=int, default=50)
    ap.add_argument("--torch-obs", action="store_true", help="stage c observations through the torch modules")
    ap.add_argument("--hold", type=int, default=10, help="stage b: items an env keeps its random heading for")
    ap.add_argument("--respawn", type=float, default=0.1, help="stage b: share of the envs reset before every item")
    ap.add_argument("--log-root", default="./logs/run_vision")
    a = ap.parse_args()
    import numpy as np
    import torch
    from shifu_amd.runner import run_module
    from shifu_amd.runner.policy_runner import build_policy_runner
    from shifu_amd.runner.utils import latest_logdir
    np.random.seed(0)
    torch.manual_seed(0)
    Dataset, StageC, EnvCfg, PPOCfg = stage_classes(a.hold, a.respawn)
    report = dict(tool="run_vision", stage_b=dict(steps=a.steps, batch=a.batch, hold=a.hold, respawn=a.respawn), stage_c=dict(iterations=a.iterations, envs=a.envs))

    # ---- stage b ----
    t0 = time.perf_counter()
    run_module('train', model=make_regressor(), dataset=Dataset(batch_size=a.batch, num_data=a.steps), model_name=MODEL_NAME,
               log_root=f"{a.log_root}/Regression")
    torch.cuda.synchronize()
    report["stage_b"]["wall_s"] = round(time.perf_counter() - t0, 2)
    model = make_regressor()
    model.load(latest_logdir(f"{a.log_root}/Regression", MODEL_NAME))          # load() leaves it in eval mode
    sq = {k: 0.0 for k in KEYS}
    fused_diff = 0.0
    for data, label in Dataset(batch_size=a.batch, num_data=a.eval_batches):
        with torch.no_grad():
            pred = model.enable_fused_inference(False)(data)
        fpred = model.enable_fused_inference()(data)
        for k in KEYS:
            sq[k] += float(((pred[k] - label[k]) ** 2).mean()) / a.eval_batches
            fused_diff = max(fused_diff, float((fpred[k] - pred[k]).abs().max()))
    report["stage_b"]["rmse_m"] = {k: round(v ** 0.5, 4) for k, v in sq.items()}
    report["stage_b"]["fused_vs_torch_max_abs_m"] = float(f"{fused_diff:.3g}")

    # ---- stage c ----
    cfg, ppo = EnvCfg(), PPOCfg()
    cfg.num_envs = a.envs
    ppo.runner.max_iterations = a.iterations
    env = StageC(cfg)
    env.regressor = model
    env.reset()
    acts = [2 * torch.rand(env.num_envs, env.num_actions, device=env.device) - 1 for _ in range(8)]
    step_ms = {}
    for mode, on in (("torch", False), ("fused", True), ("torch_again", False), ("fused_again", True)):
        env.regressor.enable_fused_inference(on)
        for i in range(5):
            env.step(acts[i % 8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(a.timed_steps):
            env.step(acts[i % 8])
        torch.cuda.synchronize()
        step_ms[mode] = round((time.perf_counter() - t0) / a.timed_steps * 1e3, 3)
    report["stage_c"]["env_step_ms"] = step_ms
    env.regressor.enable_fused_inference(not a.torch_obs)
    report["stage_c"]["observations"] = "torch" if a.torch_obs else "fused"
    runner = build_policy_runner(env, ppo, f"{a.log_root}/Vision", device=str(env.device))
    t0 = time.perf_counter()
    runner.learn(num_learning_iterations=a.iterations, init_at_random_ep_len=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    report["stage_c"]["wall_s"] = round(wall, 2)
    report["stage_c"]["env_steps_per_s"] = round(a.iterations * ppo.runner.num_steps_per_env * a.envs / wall, 1)
    report["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(report))
    env.destroy()


if __name__ == "__main__":
    main()
