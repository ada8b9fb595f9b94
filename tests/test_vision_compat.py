"""The reference's UNMODIFIED vision-stage examples (b_regression_stage.py, c_vision_stage.py) import on this backend after
`shifu_amd.compat.install(force=True)` and bind to this repo's model, dataset, runner and camera classes (build container
only: needs the reference tree, which is never shipped)."""
import os
import subprocess
import sys

import pytest

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is only present in the build container")

_CHILD = r'''
import sys
sys.dont_write_bytecode = True
sys.path.insert(0, %(root)r)
import shifu_amd.compat
shifu_amd.compat.install(force=True)
sys.path.insert(0, %(ref)r)                           # `examples` now resolves to the reference's package
import examples.abb_pushbox_vision.b_regression_stage as b
import examples.abb_pushbox_vision.c_vision_stage as c
for m in (b, c):
    assert m.__file__.startswith(%(ref)r), m.__file__
import shifu.models, shifu.models.module, shifu.models.autoencoders, shifu.utils.data, shifu.runner.module_runner
import shifu_amd.models.autoencoders as ae
import shifu_amd.models.module as mod
import shifu_amd.runner.module_runner as mr
import shifu_amd.utils.data as data
from shifu_amd.gym import ShifuVecEnv
from shifu_amd.units import CameraSensor
assert shifu.models.autoencoders is ae and shifu.models.module is mod and shifu.utils.data is data and shifu.runner.module_runner is mr
assert shifu.models.Module is mod.Module
assert b.ShifuDataset is data.ShifuDataset and b.run_module is mr.run_module and b.CameraSensor is CameraSensor
assert c.CameraSensor is CameraSensor and c.get_multi_regressor is b.get_multi_regressor
assert issubclass(b.MultimodalDataset, data.ShifuDataset)
assert issubclass(b.VisionAbbPushBox, ShifuVecEnv) and issubclass(c.FullVisionAbbPushBox, ShifuVecEnv)
import torch
torch.set_default_device("cpu")
orig = ae.MultimodalAE.__init__
def on_cpu(self, encoders, decoders, latent_dim, device="cpu"):      # the example hard-codes the default 'cuda:0'
    orig(self, encoders, decoders, latent_dim, device="cpu")
ae.MultimodalAE.__init__ = on_cpu
m = b.get_multi_regressor()
assert type(m) is ae.MultimodalAE and type(m.encoders["rgb"]) is ae.ConvEncoder and type(m.decoders["ee_pos"]) is ae.Decoder
assert len(m.state_dict()) == 112 and sum(p.numel() for p in m.parameters()) == 5284414
m.eval()
with torch.no_grad():
    out = m({"rgb": torch.zeros(1, 128, 128, 3).permute(0, 3, 1, 2), "depth": torch.ones(1, 128, 128).unsqueeze(1)})
assert sorted(out) == ["ee_pos", "goal_pos", "obj_pos"] and out["obj_pos"].shape == (1, 2)
import inspect
assert inspect.getsourcefile(c.FullVisionAbbPushBox.compute_observations).startswith(%(ref)r)
print("VISION-COMPAT-OK")
'''


def _bytecode_files():
    return sorted(os.path.join(d, f) for d, _, fs in os.walk(REF) for f in fs if f.endswith(".pyc"))


@needs_ref
def test_unmodified_vision_stage_examples_bind_to_this_backend():
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    before = _bytecode_files()
    out = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "ref": REF}], capture_output=True, text=True, env=env, cwd="/tmp")
    assert out.returncode == 0 and "VISION-COMPAT-OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert _bytecode_files() == before, "bytecode written into the reference tree"


def test_compat_aliases_cover_the_vision_pipeline():
    """Without the reference tree: the alias table names every module the vision examples import."""
    from shifu_amd import compat
    for alias in ("shifu.models", "shifu.models.module", "shifu.models.autoencoders", "shifu.utils.data", "shifu.runner.module_runner"):
        assert compat._ALIASES[alias] == alias.replace("shifu", "shifu_amd", 1)
    import shifu_amd.runner
    assert callable(shifu_amd.runner.run_module)
