"""Model classes of the vision pipeline (reference shifu/models): Module, the encoders / decoders and MultimodalAE, plus
this backend's fused inference path for the conv-encoder regressor (shifu_amd/models/fused.py, csrc/shf_conv.hip)."""
from .module import Module
