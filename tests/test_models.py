"""The vision pipeline's model classes, dataset and runner on the CPU (no GPU, no reference tree).

tests/golden/g12_models.npz was written by tools/make_golden.py from the reference's own shifu/models classes: the
state_dict layout of the full-size regressor, and a small instance with its weights, inputs, eval / train outputs and
losses.  Same torch ops on the same fp32 CPU, so summation order is the only freedom: rtol 1e-5, atol 1e-6."""
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "g12_models.npz")
KEYS = ("obj_pos", "goal_pos", "ee_pos")


def regressor(latent=32, hidden=None, dec=(16, 8), device="cpu"):
    """The structure of the vision stage's `get_multi_regressor`, at any size."""
    from shifu_amd.models.autoencoders import ConvEncoder, Decoder, MultimodalAE
    kw = {} if hidden is None else dict(hidden_dims=hidden)
    act = nn.ReLU(True)
    enc = {"rgb": ConvEncoder(in_channels=3, latent_dim=latent, activation=act, **kw),
           "depth": ConvEncoder(in_channels=1, latent_dim=latent, activation=act, **kw)}
    decs = {k: Decoder(input_dim=latent, output_dim=2, hidden_dims=list(dec)) for k in KEYS}
    return MultimodalAE(encoders=enc, decoders=decs, latent_dim=latent, device=device)


def small_golden_model(device="cpu"):
    g = np.load(GOLD)
    m = regressor(8, hidden=(4, 4, 8, 8, 8, 16), device=device)
    sd = {k: torch.from_numpy(g["sd/" + k]) for k in json.loads(str(g["small_keys"]))}
    m.load_state_dict(sd, strict=True)
    return m, g


def test_full_size_state_dict_layout_matches_the_reference():
    g = np.load(GOLD)
    m = regressor()
    got = [[k, list(v.shape)] for k, v in m.state_dict().items()]
    want = json.loads(str(g["full_layout"]))
    assert got == want
    assert len(got) == 112
    assert sum(p.numel() for p in m.parameters()) == int(g["full_num_params"]) == 5284414
    for k in ("fusion_module.weight", "rgb.feature_extractor.0.0.weight", "rgb.feature_extractor.0.1.running_mean", "rgb.fc.0.weight",
              "obj_pos.lin_decoder.0.0.weight", "obj_pos.fc.0.weight"):
        assert k in dict(got)


def test_small_golden_state_loads_strictly_and_reproduces_outputs_and_losses():
    m, g = small_golden_model()
    assert sum(p.numel() for p in m.parameters()) == int(g["small_num_params"])
    x = {"rgb": torch.from_numpy(g["rgb"]), "depth": torch.from_numpy(g["depth"])}
    labels = {k: torch.from_numpy(g["label/" + k]) for k in KEYS}
    m.eval()
    with torch.no_grad():
        out = m({k: v.clone() for k, v in x.items()})
        total, logs = m.loss_func(out, labels)
    for k in KEYS:
        np.testing.assert_allclose(out[k].numpy(), g["eval/" + k], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(float(logs[k]), float(g["eval_loss/" + k]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(total), float(g["eval_loss"]), rtol=1e-5, atol=1e-6)
    assert float(np.abs(g["eval/obj_pos"][0] - g["eval/obj_pos"][1]).max()) > 1e-4, "the fixture's outputs must depend on the input"
    m.train()
    with torch.no_grad():
        out = m({k: v.clone() for k, v in x.items()})
        total, logs = m.loss_func(out, labels)
    for k in KEYS:
        np.testing.assert_allclose(out[k].numpy(), g["train/" + k], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(float(logs[k]), float(g["train_loss/" + k]), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(total), float(g["train_loss"]), rtol=1e-5, atol=1e-6)


def test_loss_func_is_the_sum_of_per_key_mse_and_refuses_unknown_keys():
    m, _ = small_golden_model()
    pred = {k: torch.randn(3, 2) for k in KEYS}
    label = {k: torch.randn(3, 2) for k in KEYS[:2]}
    total, logs = m.loss_func(pred, label)
    assert set(logs) == set(KEYS[:2])
    want = sum(((pred[k] - label[k]) ** 2).mean() for k in label)
    assert abs(float(total) - float(want)) < 1e-6
    with pytest.raises(AssertionError):
        m.loss_func(pred, {"nope": torch.zeros(3, 2)})
    with pytest.raises(AssertionError):
        m({"lidar": torch.zeros(1, 1, 128, 128)})


def test_module_save_load_round_trip_leaves_eval_mode(tmp_path):
    from shifu_amd.models import Module
    a, _ = small_golden_model()
    b = regressor(8, hidden=(4, 4, 8, 8, 8, 16))
    a.train()
    a.save(str(tmp_path))
    assert os.path.exists(tmp_path / "MultimodalAE.pt")
    b.train()
    b.load(str(tmp_path))
    assert not b.training
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    with pytest.raises(NotImplementedError):
        Module(device="cpu").loss_func(None, None)


def test_other_model_classes_construct_and_run():
    from shifu_amd.models import autoencoders as ae
    enc = ae.Encoder(10, 4, hidden_dims=(8, 6))
    assert enc(torch.zeros(2, 10)).shape == (2, 4)
    var = ae.ConvEncoder(1, 4, hidden_dims=(2, 2, 2, 2, 2, 2), variational=True)
    mu, lv = var(torch.zeros(2, 1, 128, 128))
    assert mu.shape == lv.shape == (2, 4) and "fc_mu.weight" in var.state_dict()
    assert ae.re_param(mu, lv, False) is mu and ae.re_param(mu, lv, True).shape == mu.shape
    pm, plv = ae.product_of_experts(mu, lv)
    assert pm.shape == (2, 4) and plv.shape == (2, 4)
    dec = ae.ConvDecoder(out_channels=1, latent_dim=4, middle_dim=8 * 4, hidden_dims=(8, 4, 2))
    assert dec(torch.zeros(2, 4)).shape == (2, 1, 16, 16)
    assert isinstance(ae.reconstruction_loss_func("seg_mask"), nn.CrossEntropyLoss)
    vgg = ae.VGGEncoder(1, 4, hidden_dims=(2, 'M', 512, 'M'))
    assert vgg(torch.zeros(1, 1, 16, 16)).shape == (1, 4)


def test_enable_fused_inference_refuses_structures_the_kernels_do_not_cover():
    from shifu_amd.models import autoencoders as ae
    enc = {"rgb": ae.ConvEncoder(3, 8, hidden_dims=(4, 4), activation=nn.ELU()), "depth": ae.ConvEncoder(1, 8, hidden_dims=(4, 4))}
    dec = {"obj_pos": ae.Decoder(8, 2, hidden_dims=[4])}
    m = ae.MultimodalAE(enc, dec, latent_dim=8, device="cpu")
    with pytest.raises(ValueError, match="ReLU"):
        m.enable_fused_inference()
    enc = {"rgb": ae.VGGEncoder(3, 8, hidden_dims=(4, 'M')), "depth": ae.ConvEncoder(1, 8, hidden_dims=(4, 4))}
    with pytest.raises(ValueError, match="ConvEncoder"):
        ae.MultimodalAE(enc, dec, latent_dim=8, device="cpu").enable_fused_inference()
    ok, _ = small_golden_model()
    ok.enable_fused_inference()            # accepted; on the CPU the forward stays on the torch modules
    ok.eval()
    with torch.no_grad():
        out = ok({"rgb": torch.zeros(1, 3, 128, 128), "depth": torch.ones(1, 1, 128, 128)})
    assert out["ee_pos"].shape == (1, 2)
    assert "_fused" not in "".join(ok.state_dict().keys())


# ---- dataset and runner on a stub env -----------------------------------------------------------------------------------------
class _StubCfg:
    num_envs = 0
    num_actions = 3

    class debug:
        headless = False


class _StubEnv:
    """The part of ShifuVecEnv the dataset touches; observations = 2 x the actions."""
    destroyed = 0

    def __init__(self, cfg):
        self.cfg, self.num_envs, self.device = cfg, cfg.num_envs, "cpu"
        self.max_episode_length = 50
        self.steps = 0

    def reset(self):
        self.steps = 0

    def step(self, actions):
        assert actions.shape == (self.num_envs, self.cfg.num_actions) and float(actions.min()) >= 0 and float(actions.max()) <= 1
        self.steps += 1
        return actions, 2 * actions, None, None, {}

    def destroy(self):
        type(self).destroyed += 1


def _linear_model():
    from shifu_amd.models import Module

    class Doubler(Module):
        def __init__(self):
            super().__init__(device="cpu")
            self.lin = nn.Linear(3, 3)

        def forward(self, x):
            return {"y": self.lin(x)}

        def loss_func(self, pred, label):
            l = nn.functional.mse_loss(pred["y"], label)
            return l, {"y": l}
    return Doubler()


def test_shifu_dataset_steps_a_stub_env_and_ends_with_index_error():
    from shifu_amd.utils.data import ShifuDataset, to_np
    _StubEnv.destroyed = 0
    ds = ShifuDataset(_StubEnv, _StubCfg(), batch_size=5, num_data=3)
    assert len(ds) == 3 and ds.env.num_envs == 5 and ds.env.cfg.debug.headless is True
    assert ds.env.episode_length_buf.shape == (5,) and int(ds.env.episode_length_buf.max()) < 50
    items = [it for it in ds]                      # the sequence protocol: ends at the IndexError
    assert len(items) == 3 and ds.env.steps == 3 and _StubEnv.destroyed == 1
    obs, priv = items[0]
    assert to_np(priv).dtype == np.float32 and np.allclose(to_np(priv), 2 * to_np(obs))
    ds2 = ShifuDataset(_StubEnv, _StubCfg(), batch_size=2, num_data=1, render_mode=1)
    assert ds2.env.cfg.debug.headless is False
    with pytest.raises(IndexError):
        ds2[1]
    assert _StubEnv.destroyed == 2
    ds3 = ShifuDataset(_StubEnv, _StubCfg(), batch_size=2, num_data=4)
    ds3[0], ds3[1]
    a = ds3.random_actions(-2., 3.)
    assert a.shape == (2, 3) and float(a.min()) >= -2. and float(a.max()) < 3.
    ds3.reset()                                    # resets the env; the items start over
    assert ds3.env.steps == 0 and len([it for it in ds3]) == 4


def test_run_module_train_then_play_on_a_stub_env(tmp_path, capsys):
    from shifu_amd.runner import run_module
    from shifu_amd.runner.utils import latest_logdir
    from shifu_amd.utils.data import ShifuDataset
    root = str(tmp_path / "logs")
    torch.manual_seed(0)
    model = _linear_model()
    w0 = model.lin.weight.detach().clone()
    run_module("train", model, ShifuDataset(_StubEnv, _StubCfg(), 16, 40), "Doubler-test", train_log_interval=10, log_root=root,
               lr=1e-2, device="cpu")
    run = latest_logdir(root, "Doubler-test")
    assert os.path.exists(os.path.join(run, "Doubler.pt"))
    assert not torch.equal(w0, model.lin.weight)
    import importlib.util
    if importlib.util.find_spec("tensorboard") is None:          # the JSON-lines log stands in for tensorboard
        rows = [json.loads(l) for l in open(os.path.join(run, "scalars.jsonl"))]
        assert [r["step"] for r in rows] == [0, 10, 20, 30] and all("Train/y" in r for r in rows)
        assert rows[-1]["Train/y"] < rows[0]["Train/y"]
    fresh = _linear_model()
    run_module("play", fresh, ShifuDataset(_StubEnv, _StubCfg(), 16, 5), "Doubler-test", log_root=root, device="cpu")
    saved = torch.load(os.path.join(run, "Doubler.pt"))          # the checkpoint of the last logged step (30), not of step 39
    assert torch.equal(fresh.lin.weight, saved["lin.weight"]) and not fresh.training
    assert os.path.isdir(root + "_play/Doubler-test")
    assert "Eval/" in capsys.readouterr().out
    with pytest.raises(NotImplementedError):
        run_module("bogus", fresh, [], "x", log_root=root, device="cpu")


def test_jsonl_scalar_log_writes_one_line_per_step(tmp_path):
    from shifu_amd.runner.module_runner import _JsonlWriter
    w = _JsonlWriter(str(tmp_path))
    w.add_scalar("Train/a", 1.0, global_step=0)
    w.add_scalar("Train/b", 2.0, global_step=0)
    w.add_scalar("Train/a", 0.5, global_step=7)
    w.close()
    rows = [json.loads(l) for l in open(tmp_path / "scalars.jsonl")]
    assert len(rows) == 2 and rows[0]["Train/b"] == 2.0 and rows[1]["step"] == 7 and rows[1]["Train/a"] == 0.5


def test_camera_entry_refuses_what_it_cannot_honour():
    """forward_from_camera needs the fused path in eval mode on a GPU, and from_camera a sensor with image_normalization."""
    import types
    from shifu_amd.models.autoencoders import ConvEncoder, Decoder, MultimodalAE
    from shifu_amd.models.fused import FusedRegressor
    enc = {"rgb": ConvEncoder(3, 8, hidden_dims=(4, 4, 8, 8, 8, 16), activation=nn.ReLU()),
           "depth": ConvEncoder(1, 8, hidden_dims=(4, 4, 8, 8, 8, 16), activation=nn.ReLU())}
    m = MultimodalAE(enc, {"obj_pos": Decoder(8, 2, hidden_dims=[16, 8], activation=nn.ReLU())}, latent_dim=8, device="cpu").eval()
    assert m.fused is None
    with pytest.raises(RuntimeError, match="enable_fused_inference"):
        m.forward_from_camera(None)
    m.enable_fused_inference()
    assert isinstance(m.fused, FusedRegressor)
    with pytest.raises(RuntimeError, match="GPU"):
        m.forward_from_camera(None)
    raw = types.SimpleNamespace(cfg=types.SimpleNamespace(image_normalization=False))
    with pytest.raises(ValueError, match="image_normalization"):
        m.fused.from_camera(raw)
