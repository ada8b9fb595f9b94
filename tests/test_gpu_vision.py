"""The conv-encoder inference path on the GPU (csrc/shf_conv.hip, shifu_amd/models/fused.py).

Error bounds.  One layer (conv + eval batch norm + ReLU) against the same torch layer in float64 on the CPU: the project's
bound for this operand scheme, TOL of tests/test_gpu_mlp.py -- max 2e-4 and mean 2e-5 of the output scale for bf16x3, the
`bf16` row for that mode.  The whole regressor: E = max |y - y64| / max |y64| over all outputs; the fused forward's E_f must
stay within 12 x the per-layer max bound (twelve GEMM-like layers on the longest path: six convolutions, fc.0, fc.2, fusion,
three decoder layers), which holds while no layer amplifies error -- so the tests scale the weights to keep activations
O(1) and assert that on the float64 forward.  E_t, torch's own fp32 GPU forward, is printed beside it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

from tests.test_gpu_mlp import TOL
from tests.test_models import KEYS, regressor, small_golden_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYERS_ON_PATH = 12


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU is visible")


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _precision:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from shifu_amd._lib import lib
        self.old = lib().shf_mlp_get_precision()
        assert lib().shf_mlp_set_precision({"bf16": 0, "bf16x3": 1}[self.mode]) == 0

    def __exit__(self, *a):
        from shifu_amd._lib import lib
        lib().shf_mlp_set_precision(self.old)


def _conv_gpu(x, kind, strides, weight, scale, shift, n, cin, h, w, cout, flatten=False):
    """One shf_conv3x3s2_forward call on device tensors; returns (n, h/2, w/2, cout) or, flattened, (n, cout, h/2, w/2)."""
    from shifu_amd._lib import lib
    nbytes = C.c_int64()
    assert lib().shf_conv_pack_bytes(cin, cout, C.byref(nbytes)) == 0
    pack = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    wd = weight.to(DEV).float().contiguous()
    assert lib().shf_conv_pack_weights(C.c_void_p(wd.data_ptr()), C.c_void_p(pack.data_ptr()), cin, cout, _stream()) == 0
    y = torch.full((n, cout, h // 2, w // 2) if flatten else (n, h // 2, w // 2, cout), float("nan"), device=DEV)
    s, t = scale.to(DEV).float().contiguous(), shift.to(DEV).float().contiguous()
    rc = lib().shf_conv3x3s2_forward(C.c_void_p(x.data_ptr()), kind, (C.c_int64 * 4)(*strides), C.c_void_p(pack.data_ptr()),
                                     C.c_void_p(s.data_ptr()), C.c_void_p(t.data_ptr()), C.c_void_p(y.data_ptr()), int(flatten), n, cin, h, w,
                                     cout, _stream())
    assert rc == 0, lib().shf_conv_last_error()
    torch.cuda.synchronize()
    return y


def _check(got, ref, mode, what):
    err = (got.double().cpu() - ref).abs()
    scale = float(ref.abs().max()) + 1e-12
    tmax, tmean = TOL[mode]
    print(f"{what} [{mode}]: max err {float(err.max()) / scale:.3g}, mean err {float(err.mean()) / scale:.3g} of scale {scale:.3g}")
    assert float(err.max()) <= tmax * scale, f"{what} [{mode}]: max err {float(err.max()):.3g} vs scale {scale:.3g}"
    assert float(err.mean()) <= tmean * scale, f"{what} [{mode}]: mean err {float(err.mean()):.3g} vs scale {scale:.3g}"


# ---- fragment layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout,tap,ci,co", [(3, 5, (0, 2), 1, 3), (8, 40, (2, 0), 5, 33), (1, 16, (1, 2), 0, 9)])
def test_a_single_tap_weight_reproduces_the_shifted_strided_input(cin, cout, tap, ci, co):
    """w[co, ci, ky, kx] = 1 and nothing else (exact in bf16), inputs exact in bf16: output channel co is the input channel
    ci shifted by the tap and strided by 2, element for element; every other channel is zero.  The tap, the channels and
    the image (H != W) are asymmetric, so a transposed fragment or pixel layout cannot pass."""
    _need_gpu()
    n, h, w = 3, 12, 20
    g = torch.Generator().manual_seed(1)
    x = torch.randint(-64, 64, (n, cin, h, w), generator=g).float() / 8.0
    wt = torch.zeros(cout, cin, 3, 3)
    wt[co, ci, tap[0], tap[1]] = 1.0
    xd = x.to(DEV)
    y = _conv_gpu(xd, 0, xd.stride(), wt, torch.ones(cout), torch.zeros(cout), n, cin, h, w, cout).cpu()
    pad = torch.zeros(n, h + 2, w + 2)
    pad[:, 1:-1, 1:-1] = x[:, ci]
    want = torch.relu(pad[:, tap[0]:tap[0] + h:2, tap[1]:tap[1] + w:2])
    assert torch.equal(y[..., co], want)
    rest = y.clone()
    rest[..., co] = 0
    assert float(rest.abs().max()) == 0.0
    yf = _conv_gpu(xd, 0, xd.stride(), wt, torch.ones(cout), torch.zeros(cout), n, cin, h, w, cout, flatten=True).cpu()
    assert torch.equal(yf, y.permute(0, 3, 1, 2))


# ---- one layer against float64 ----------------------------------------------------------------------------------------------------
STAGE_SHAPES = [(3, 16, 128), (1, 16, 128), (16, 32, 64), (32, 64, 32), (64, 128, 16), (128, 256, 8), (256, 512, 4)]
SMALL_SHAPES = [(3, 4, 128), (1, 4, 128), (4, 4, 64), (4, 8, 32), (8, 8, 16), (8, 8, 8), (8, 16, 4), (5, 7, 6), (2, 33, 10)]


def _layer_case(cin, cout, size, batch, mode, seed):
    """Batch `batch` built from at most 50 distinct images (the larger batches repeat them in a shuffled order), so the
    float64 CPU reference stays cheap while every output row of the large batch is compared."""
    g = torch.Generator().manual_seed(seed)
    distinct = min(batch, 50)
    imgs = torch.randn(distinct, cin, size, size, generator=g)
    order = torch.randperm(batch, generator=g) % distinct
    layer = nn.Sequential(nn.Conv2d(cin, cout, 3, 2, 1), nn.BatchNorm2d(cout), nn.ReLU())
    with torch.no_grad():
        layer[0].weight.copy_(torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        layer[0].bias.copy_(0.2 * torch.randn(cout, generator=g))
        layer[1].running_mean.copy_(0.3 * torch.randn(cout, generator=g))
        layer[1].running_var.copy_(0.5 + torch.rand(cout, generator=g))
        layer[1].weight.copy_(0.7 + 0.6 * torch.rand(cout, generator=g))
        layer[1].bias.copy_(0.2 * torch.randn(cout, generator=g))
    layer.eval()
    from shifu_amd.models.fused import bn_affine
    s, t = bn_affine(layer[0], layer[1])
    with torch.no_grad():
        ref = layer.double()(imgs.double())[order].permute(0, 2, 3, 1)
    x = imgs[order].to(DEV).contiguous()
    with _precision(mode):
        y = _conv_gpu(x, 0, x.stride(), layer[0].weight.float(), s, t, batch, cin, size, size, cout)
    _check(y, ref, mode, f"conv {cin}->{cout} @ {size} x {size}, batch {batch}")


@pytest.mark.parametrize("batch", [1, 50, 1000])
@pytest.mark.parametrize("cin,cout,size", STAGE_SHAPES)
def test_stage_layer_against_float64(cin, cout, size, batch):
    _need_gpu()
    _layer_case(cin, cout, size, batch, "bf16x3", seed=100 + cin + size)


@pytest.mark.parametrize("batch", [1, 50])
@pytest.mark.parametrize("cin,cout,size", SMALL_SHAPES)
def test_odd_channel_layer_against_float64(cin, cout, size, batch):
    _need_gpu()
    _layer_case(cin, cout, size, batch, "bf16x3", seed=200 + cin + cout)


@pytest.mark.parametrize("cin,cout,size", [(5, 7, 6), (2, 33, 10), (8, 16, 4)])
def test_odd_channel_layer_at_batch_1000_against_float64(cin, cout, size):
    """The four-wave block path with padded fragments in N and K and a tail in M (1000 x 9 and 1000 x 25 output pixels)."""
    _need_gpu()
    _layer_case(cin, cout, size, 1000, "bf16x3", seed=200 + cin + cout)


@pytest.mark.parametrize("cin,cout,size", [(3, 16, 128), (64, 128, 16), (8, 16, 4)])
def test_layer_in_bf16_mode_against_float64(cin, cout, size):
    _need_gpu()
    _layer_case(cin, cout, size, 50, "bf16", seed=300 + cin)


def test_channels_last_input_takes_the_vector_path_and_equals_the_strided_read():
    """An NHWC fp32 input with C_in % 4 == 0 is read with 16-byte loads, any other layout element by element: same values."""
    _need_gpu()
    g = torch.Generator().manual_seed(5)
    n, cin, cout, size = 7, 8, 24, 16
    x = torch.randn(n, cin, size, size, generator=g).to(DEV)
    xl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)           # same values, NHWC memory
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.2
    s, t = 0.5 + torch.rand(cout, generator=g), torch.randn(cout, generator=g)
    a = _conv_gpu(x, 0, x.stride(), wt, s, t, n, cin, size, size, cout)
    b = _conv_gpu(xl, 0, xl.stride(), wt, s, t, n, cin, size, size, cout)
    assert torch.equal(a, b)


# ---- the whole regressor ----------------------------------------------------------------------------------------------------------
def _seeded_full_model(seed=7):
    """Full-size regressor with seeded weights scaled to keep activations O(1) (the default initialisation shrinks the signal
    layer by layer) and random batch-norm statistics / affine terms."""
    torch.manual_seed(seed)
    m = regressor()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (2.0 / (9 * mod.in_channels)) ** 0.5)
            elif isinstance(mod, nn.Linear):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=g) * (1.5 / mod.in_features) ** 0.5)
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
            elif isinstance(mod, nn.BatchNorm2d):
                mod.running_mean.copy_(0.3 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(0.7 + 0.6 * torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.2 * torch.randn(mod.bias.shape, generator=g))
    return m.eval()


def _images(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (n, 128, 128, 3), generator=g).float() / 255.0
    depth = 0.3 + 2.5 * torch.rand(n, 128, 128, generator=g)
    return rgb, depth


def _stage_views(rgb, depth):
    """The views stage c passes: NHWC color permuted to NCHW, depth with a channel axis."""
    return {"rgb": rgb.permute(0, 3, 1, 2), "depth": depth.unsqueeze(1)}


def _float64_forward(model, x):
    """float64 CPU forward of a copy of `model`; also the mean |activation| behind every ReLU / final layer."""
    import copy
    m64 = copy.deepcopy(model).cpu()
    m64.device = "cpu"
    m64.enable_fused_inference(False)
    m64 = m64.double().eval()
    acts = []
    hooks = [mod.register_forward_hook(lambda _m, _i, o: acts.append(float(o.abs().mean())))
             for mod in m64.modules() if isinstance(mod, (nn.ReLU, nn.Linear))]
    torch.set_default_dtype(torch.float64)       # cross_modal_encode stacks the latents in a default-dtype tensor
    try:
        with torch.no_grad():
            out = m64({k: v.double().cpu().clone() for k, v in x.items()})
    finally:
        torch.set_default_dtype(torch.float32)
    for h in hooks:
        h.remove()
    return out, acts


def _to_device(model):
    model.to(DEV)
    model.device = DEV
    return model


def _rel_err(out, ref):
    a = torch.cat([out[k].double().cpu() for k in KEYS], 1)
    b = torch.cat([ref[k] for k in KEYS], 1)
    return float((a - b).abs().max()) / float(b.abs().max())


def _end_to_end(model, x, what):
    ref, acts = _float64_forward(model, x)
    assert all(1e-2 <= a <= 1e2 for a in acts), f"{what}: activations are not O(1): {acts}"
    _to_device(model).eval()
    xd = {k: v.to(DEV) for k, v in x.items()}
    with torch.no_grad():
        e_t = _rel_err(model({k: v.clone() for k, v in xd.items()}), ref)
    model.enable_fused_inference()
    out = model(xd)
    torch.cuda.synchronize()
    assert all(o.grad_fn is None and not o.requires_grad for o in out.values())
    e_f = _rel_err(out, ref)
    print(f"{what}: E_f = {e_f:.3g} (fused), E_t = {e_t:.3g} (torch fp32 on the GPU), bound {LAYERS_ON_PATH * TOL['bf16x3'][0]:.3g}")
    assert e_f <= LAYERS_ON_PATH * TOL["bf16x3"][0], f"{what}: E_f = {e_f:.3g}, E_t = {e_t:.3g}"
    return e_f, e_t


def test_end_to_end_golden_small_model():
    _need_gpu()
    m, g = small_golden_model()
    x = {"rgb": torch.from_numpy(g["rgb"]), "depth": torch.from_numpy(g["depth"])}
    _end_to_end(m, x, "small golden model")


def test_end_to_end_full_size_model():
    _need_gpu()
    rgb, depth = _images(64)
    _end_to_end(_seeded_full_model(), _stage_views(rgb, depth), "full-size model, 64 images")


def test_batch_permutation_and_subsets_are_bitwise():
    _need_gpu()
    m = _to_device(_seeded_full_model()).enable_fused_inference()
    n = 37
    rgb, depth = _images(n, seed=11)
    rgb, depth = rgb.to(DEV), depth.to(DEV)
    base = {k: v.clone() for k, v in m(_stage_views(rgb, depth)).items()}
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(DEV)
    out = m(_stage_views(rgb[perm].contiguous(), depth[perm].contiguous()))
    for k in KEYS:
        assert torch.equal(out[k], base[k][perm]), k
    for idx in ([0, 1, 2, 3, 4], [36], [20, 5]):
        sel = torch.tensor(idx, device=DEV)
        out = m(_stage_views(rgb[sel].contiguous(), depth[sel].contiguous()))
        for k in KEYS:
            assert torch.equal(out[k], base[k][sel]), (k, idx)


def test_an_infinite_depth_pixel_spoils_its_own_image_only():
    _need_gpu()
    m = _to_device(_seeded_full_model()).enable_fused_inference()
    rgb, depth = _images(6, seed=13)
    rgb, depth = rgb.to(DEV), depth.to(DEV)
    base = {k: v.clone() for k, v in m(_stage_views(rgb, depth)).items()}
    depth[3, 17, 40] = float("inf")
    out = m(_stage_views(rgb, depth))
    others = torch.tensor([0, 1, 2, 4, 5], device=DEV)
    for k in KEYS:
        assert not torch.isfinite(out[k][3]).any(), k
        assert torch.equal(out[k][others], base[k][others]), k


def test_a_changed_model_is_repacked():
    _need_gpu()
    a = _to_device(_seeded_full_model(seed=7)).enable_fused_inference()
    b = _to_device(_seeded_full_model(seed=8)).enable_fused_inference()
    rgb, depth = _images(5, seed=17)
    x = _stage_views(rgb.to(DEV), depth.to(DEV))
    out_a = {k: v.clone() for k, v in a(x).items()}
    out_b = {k: v.clone() for k, v in b(x).items()}
    assert not torch.equal(out_a["obj_pos"], out_b["obj_pos"])
    a.load_state_dict(b.state_dict())
    got = a(x)
    for k in KEYS:
        assert torch.equal(got[k], out_b[k]), k
    with torch.no_grad():      # an in-place edit of one batch-norm buffer and of one conv weight, as an optimizer step makes them
        a.rgb.feature_extractor[2][1].running_mean.add_(0.5)
        assert not torch.equal(a(x)["obj_pos"], out_b["obj_pos"])
        a.rgb.feature_extractor[2][1].running_mean.sub_(0.5)
        a.depth.feature_extractor[0][0].weight.mul_(1.5)
        assert not torch.equal(a(x)["obj_pos"], out_b["obj_pos"])


def test_a_captured_forward_follows_a_weight_change_after_one_eager_call():
    """A repack writes into the buffers an earlier capture recorded: after load_state_dict and one eager call, replaying
    the old graph gives the new model's outputs."""
    _need_gpu()
    a = _to_device(_seeded_full_model(seed=7)).enable_fused_inference()
    b = _to_device(_seeded_full_model(seed=8)).enable_fused_inference()
    rgb, depth = _images(6, seed=23)
    x = _stage_views(rgb.to(DEV), depth.to(DEV))
    want_a = {k: v.clone() for k, v in a(x).items()}          # also the warm-up: packs, sizes the workspaces
    want_b = {k: v.clone() for k, v in b(x).items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a(x)
    graph.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], want_a[k]), k
    a.load_state_dict(b.state_dict())
    a(x)                                                      # the eager call that repacks, in place
    graph.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(out[k], want_b[k]), k


def test_train_mode_runs_torch_with_gradients_and_eval_returns_to_the_kernels():
    _need_gpu()
    m = _to_device(_seeded_full_model()).enable_fused_inference()
    rgb, depth = _images(4, seed=19)
    x = _stage_views(rgb.to(DEV), depth.to(DEV))
    fused = {k: v.clone() for k, v in m(x).items()}
    assert m.fused.launches == 20
    m.train()
    out = m({k: v.clone() for k, v in x.items()})
    assert all(o.grad_fn is not None for o in out.values())
    loss, _ = m.loss_func(out, {k: torch.zeros(4, 2, device=DEV) for k in KEYS})
    loss.backward()
    assert m.rgb.feature_extractor[0][0].weight.grad is not None and float(m.depth.fc[2].weight.grad.abs().max()) > 0
    m.eval()
    m.fused.launches = 0
    again = m(x)
    assert m.fused.launches == 20 and all(o.grad_fn is None for o in again.values())
    # the train-mode pass moved the running statistics (in place): the pack followed them
    assert not torch.equal(again["obj_pos"], fused["obj_pos"])
    m.enable_fused_inference(False)
    with torch.no_grad():
        ref = m({k: v.clone() for k, v in x.items()})
    scale = float(torch.cat([ref[k] for k in KEYS], 1).abs().max())
    for k in KEYS:
        assert float((again[k] - ref[k]).abs().max()) <= LAYERS_ON_PATH * TOL["bf16x3"][0] * scale


# ---- on the push-box vision env ---------------------------------------------------------------------------------------------------
def _vision_env(n, model=None, from_camera=False):
    """The push-box scene with the vision stage's 128 x 128 camera; with `model`, observations are its predictions (the
    reference's c_vision_stage.py compute_observations)."""
    from shifu_amd import compat
    compat.install()
    from shifu.configs import CameraSensorConfig
    from shifu.units import CameraSensor
    from isaacgym import gymapi as ga
    from examples.abb_pushbox_vision.a_prior_stage import AbbPushBox, AbbRobot, GoalBox, RandPosBox
    from examples.abb_pushbox_vision.task_config import (AbbRobotConfig, GoalBoxConfig, PriorStageEnvConfig, PushBoxConfig,
                                                         TableConfig)
    from shifu_amd.gym import ShifuVecEnv
    from shifu_amd.units import Box

    class PushBoxCameraConfig(CameraSensorConfig):
        name = 'rgbd_camera'
        local_lookat_positions = [[0.7, 0., 0.7], [0., 0., 0.1]]
        image_types = [ga.IMAGE_COLOR, ga.IMAGE_DEPTH, ga.IMAGE_SEGMENTATION]
        image_normalization = True

        class camera_props(CameraSensorConfig.camera_props):
            enable_tensors = True
            use_collision_geometry = False
            width = 128
            height = 128
            horizontal_fov = 42
            near_plane = 0.1
            far_plane = 3

    class VisionPushBox(AbbPushBox):
        def __init__(self, cfg):
            ShifuVecEnv.__init__(self, cfg)
            self.robot = AbbRobot(AbbRobotConfig())
            self.table = Box(TableConfig())
            self.cube = RandPosBox(PushBoxConfig())
            self.goal = GoalBox(GoalBoxConfig())
            self.camera = CameraSensor(PushBoxCameraConfig())
            self.isg_env.create_envs(robot=self.robot, objects=[self.table, self.cube, self.goal], sensors=[self.camera])
            self.success_buf = torch.zeros(self.num_envs, device=self.device, dtype=torch.float)
            self.regressor = model

        def compute_observations(self):
            if self.regressor is None:
                return AbbPushBox.compute_observations(self)
            if from_camera:
                pred = self.regressor.forward_from_camera(self.camera)
            else:
                pred = self.regressor({'rgb': self.camera.color_buf.permute(0, 3, 1, 2),
                                       'depth': self.camera.depth_buf.unsqueeze(3).permute(0, 3, 1, 2)})
            self.obs_buf = torch.cat([pred['obj_pos'].detach(), pred['goal_pos'].detach(), pred['ee_pos'].detach()], dim=1)

    cfg = PriorStageEnvConfig()
    cfg.num_envs = n
    return VisionPushBox(cfg)


def _random_steps(env, k, seed):
    g = torch.Generator().manual_seed(seed)
    for _ in range(k):
        env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))
    torch.cuda.synchronize()


def test_from_camera_equals_the_forward_on_the_sensor_buffers_bitwise():
    _need_gpu()
    env = _vision_env(48)
    env.reset()
    _random_steps(env, 4, seed=3)
    cam = env.camera
    assert bool(torch.isfinite(cam.depth_buf).all()), "precondition: every depth pixel of the push-box view is finite"
    assert float(cam.depth_buf.max()) < 3.0
    m = _to_device(_seeded_full_model()).enable_fused_inference()
    a = {k: v.clone() for k, v in m({'rgb': cam.color_buf.permute(0, 3, 1, 2), 'depth': cam.depth_buf.unsqueeze(1)}).items()}
    b = m.forward_from_camera(cam)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert bool(torch.isfinite(a["obj_pos"]).all()) and float(a["obj_pos"].std()) > 0
    env.destroy()


def test_graph_replay_of_a_vision_hook_env_equals_eager():
    """compute_observations calls the fused regressor inside the second hipGraph of enable_graph_hooks; the replayed
    obs_buf equals an eager fused forward on the images the step observed (those of the step before: observations are
    computed before the sensors refresh), bit for bit."""
    _need_gpu()
    torch.manual_seed(1)
    m = _to_device(_seeded_full_model()).enable_fused_inference()
    env = _vision_env(32, model=m)
    env.reset()
    env.enable_graph_hooks()
    assert env._hook_graphs is not None
    g = torch.Generator().manual_seed(4)
    cam = env.camera
    for _ in range(4):
        seen = {'rgb': cam.color_buf.clone().permute(0, 3, 1, 2), 'depth': cam.depth_buf.clone().unsqueeze(1)}
        obs = env.step((2 * torch.rand(env.num_envs, env.num_actions, generator=g) - 1).to(env.device))[0].clone()
        pred = m(seen)
        want = torch.clip(torch.cat([pred[k] for k in KEYS], 1), -env.clip_obs, env.clip_obs)
        torch.cuda.synchronize()
        assert torch.equal(obs, want)
    assert float(obs.std()) > 0
    env.destroy()


def test_the_regressor_learns_a_fixed_batch_and_the_fused_forward_follows():
    """64 rendered images with their labels, 200 Adam steps (lr 1e-3) through ModuleRunner.update: the batch loss falls
    below the constant predictor's (the labels' variance, measured in the same run); the fused eval forward of the trained
    weights then agrees with torch's within the end-to-end bound."""
    _need_gpu()
    from shifu_amd.runner.module_runner import ModuleRunner
    env = _vision_env(64)
    env.reset()
    _random_steps(env, 3, seed=5)
    cam = env.camera
    data = {'rgb': cam.color_buf.clone().permute(0, 3, 1, 2), 'depth': cam.depth_buf.clone().unsqueeze(1)}
    label = {'obj_pos': env.cube.base_pose[:, :2].detach().clone(), 'goal_pos': env.goal.base_pose[:, :2].detach().clone(),
             'ee_pos': env.robot.ee_pose[:, 0, :2].detach().clone()}
    env.destroy()
    assert bool(torch.isfinite(data['depth']).all())
    torch.manual_seed(0)
    m = regressor(device=DEV)
    runner = ModuleRunner(m, lr=1e-3, weight_decay=1e-5, device=DEV)
    const, _ = m.loss_func({k: v.mean(0, keepdim=True).expand_as(v) for k, v in label.items()}, label)
    m.train()
    for _ in range(200):
        pred, logs = runner.update(data, label)
    final = float(sum(logs.values()))
    print(f"batch loss after 200 steps {final:.3g}; constant predictor {float(const):.3g}")
    assert final < float(const)
    m.eval()
    with torch.no_grad():
        ref = m({k: v.clone() for k, v in data.items()})
    m.enable_fused_inference()
    out = m(data)
    scale = float(torch.cat([ref[k] for k in KEYS], 1).abs().max())
    err = max(float((out[k] - ref[k]).abs().max()) for k in KEYS)
    print(f"trained weights: fused vs torch max err {err / scale:.3g} of scale {scale:.3g}")
    assert err <= LAYERS_ON_PATH * TOL["bf16x3"][0] * scale
