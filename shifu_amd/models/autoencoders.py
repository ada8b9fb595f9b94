"""Encoders, decoders and the multimodal autoencoder of the vision stage (public surface of the reference's
shifu/models/autoencoders.py: constructor signatures, defaults and submodule names, so that a state_dict from either side
loads on the other).  Everything here is stock torch; the eval-mode forward of a conv-encoder MultimodalAE can be routed
through this backend's HIP kernels with MultimodalAE.enable_fused_inference() (shifu_amd/models/fused.py)."""
from typing import List, Tuple

import torch
from torch import nn

from .module import Module


def _relu():
    return nn.ReLU(inplace=True)


def linear_multilayer(input_dim: int, hidden_dims: [List, Tuple], activation: nn.Module = None):
    """Sequential of Sequential(Linear, activation) blocks, one per hidden width."""
    activation = _relu() if activation is None else activation
    widths = [input_dim] + list(hidden_dims)
    return nn.Sequential(*[nn.Sequential(nn.Linear(a, b), activation) for a, b in zip(widths[:-1], widths[1:])])


def conv_encoder(in_channels: int, hidden_dims: [List, Tuple] = (16, 32, 64, 128, 256, 512), activation: nn.Module = None):
    """Sequential of Sequential(Conv2d 3x3 / stride 2 / padding 1, BatchNorm2d, activation) blocks: every block halves H and W."""
    activation = _relu() if activation is None else activation
    chans = [in_channels] + list(hidden_dims)
    return nn.Sequential(*[nn.Sequential(nn.Conv2d(a, b, kernel_size=3, stride=2, padding=1, bias=True), nn.BatchNorm2d(b), activation)
                           for a, b in zip(chans[:-1], chans[1:])])


def make_conv_layers(in_channels: int, hidden_dims: [List, Tuple] = (64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'),
                     activation: nn.Module = None, batch_norm: bool = True):
    """VGG-style flat Sequential: 'M' = 2x2 max pool, a number = Conv2d 3x3 / padding 1 (+ BatchNorm2d) + activation."""
    activation = _relu() if activation is None else activation
    layers = []
    for v in hidden_dims:
        if v == 'M':
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        layers.append(nn.Conv2d(in_channels, v, kernel_size=3, padding=1))
        if batch_norm:
            layers.append(nn.BatchNorm2d(v))
        layers.append(activation)
        in_channels = v
    return nn.Sequential(*layers)


def conv_decoder(out_channels: int, hidden_dims: [List, Tuple] = (512, 256, 128, 64, 32, 16), activation: nn.Module = None):
    """Mirror of conv_encoder with transposed convolutions (each block doubles H and W); the output block has no norm / activation."""
    activation = _relu() if activation is None else activation

    def up(a, b):
        return nn.ConvTranspose2d(a, b, kernel_size=3, stride=2, padding=1, output_padding=1, bias=True)
    blocks = [nn.Sequential(up(a, b), nn.BatchNorm2d(b), activation) for a, b in zip(hidden_dims[:-1], hidden_dims[1:])]
    blocks.append(nn.Sequential(up(hidden_dims[-1], out_channels)))
    return nn.Sequential(*blocks)


def re_param(mu, log_var, training):
    """Reparameterisation trick; the mean at inference."""
    if not training:
        return mu
    std = torch.exp(0.5 * log_var)
    return mu + torch.randn_like(std) * std


def product_of_experts(x_mu, x_log_var, eps=1e-8):
    """Product of a standard-normal prior expert and the given Gaussian expert: (mu, log var) of the product."""
    mu = torch.stack((torch.zeros_like(x_mu), x_mu))
    log_var = torch.stack((torch.zeros_like(x_log_var), x_log_var))
    var = torch.exp(log_var) + eps
    prec = 1.0 / (var + eps)
    pd_mu = (mu * prec).sum(0) / prec.sum(0)
    pd_var = 1.0 / prec.sum(0)
    return pd_mu, torch.log(pd_var + eps)


def reconstruction_loss_func(task):
    return nn.CrossEntropyLoss() if 'seg' in task else nn.MSELoss()


class Encoder(nn.Module):
    def __init__(self, input_dim: int, output_dim: int, hidden_dims: [List, Tuple] = (512, 256, 128, 64, 32),
                 variational: bool = False, activation=None):
        super().__init__()
        self.input_dim = input_dim
        self.hidden_dims = hidden_dims
        self.latent_dim = output_dim
        self.activation = _relu() if activation is None else activation
        self.variational = variational
        self.feature_extractor = self._build_feature_extractor()
        self.num_out_features = 2 * output_dim if variational else output_dim
        mid = self.get_middle_dim()
        if variational:
            self.fc_mu = nn.Linear(mid, output_dim)
            self.fc_var = nn.Linear(mid, output_dim)
        else:
            self.fc = nn.Sequential(nn.Linear(mid, 512), self.activation, nn.Linear(512, output_dim))

    def get_middle_dim(self):
        return self.hidden_dims[-1]

    def _build_feature_extractor(self):
        return linear_multilayer(self.input_dim, self.hidden_dims, self.activation)

    def forward(self, x):
        x = torch.flatten(self.feature_extractor(x), start_dim=1)
        if self.variational:
            return self.fc_mu(x), self.fc_var(x)
        return self.fc(x)


class ConvEncoder(Encoder):
    """Images (N, C, H, W) whose conv stack ends at 2 x 2 (128 x 128 with the default six layers) -> latent vector."""

    def __init__(self, in_channels: int, latent_dim: int, hidden_dims: [List, Tuple] = (16, 32, 64, 128, 256, 512),
                 variational: bool = False, activation=None):
        self.in_channels = in_channels
        super().__init__(-1, latent_dim, hidden_dims, variational, activation)

    def get_middle_dim(self):
        return self.hidden_dims[-1] * 4

    def _build_feature_extractor(self):
        return conv_encoder(self.in_channels, self.hidden_dims, self.activation)


class VGGEncoder(ConvEncoder):
    def __init__(self, in_channels: int, latent_dim: int,
                 hidden_dims: [List, Tuple] = (64, 'M', 128, 'M', 256, 256, 'M', 512, 512, 'M', 512, 512, 'M'),
                 variational: bool = False, activation=None):
        super().__init__(in_channels, latent_dim, hidden_dims, variational, activation)

    def get_middle_dim(self):
        return 512 * 4 * 4

    def _build_feature_extractor(self):
        return make_conv_layers(self.in_channels, self.hidden_dims, self.activation)


class Decoder(nn.Module):
    def __init__(self, input_dim: int, output_dim: int, hidden_dims: [List, Tuple] = (32, 64, 128, 256, 512), activation=None):
        super().__init__()
        self.lin_decoder = linear_multilayer(input_dim, hidden_dims, activation)
        self.num_out_features = output_dim
        self.fc = nn.Sequential(nn.Linear(hidden_dims[-1], output_dim))

    def forward(self, x):
        return self.fc(self.lin_decoder(x))


class ConvDecoder(nn.Module):
    def __init__(self, out_channels: int, latent_dim: int, middle_dim: int, hidden_dims: [List, Tuple] = (512, 256, 128, 64, 32, 16),
                 activation=None):
        super().__init__()
        activation = _relu() if activation is None else activation
        self.hidden_dims = hidden_dims
        self.lin_decoder = nn.Sequential(nn.Linear(latent_dim, middle_dim), activation)
        self.conv_decoder = conv_decoder(out_channels=out_channels, hidden_dims=hidden_dims, activation=activation)

    def forward(self, x):
        x = self.lin_decoder(x).view(-1, self.hidden_dims[0], 2, 2)
        return self.conv_decoder(x)


class MultimodalAE(Module):
    """Per-modality encoders -> concatenated latents -> linear fusion -> one decoder per output key."""

    def __init__(self, encoders: dict, decoders: dict, latent_dim: int, device='cuda:0'):
        super().__init__(device=device)
        self.latent_dim = latent_dim
        self.encoders = encoders
        self.decoders = decoders
        self.fusion_module = nn.Linear(len(encoders) * latent_dim, latent_dim)
        self.position_dict = {name: i for i, name in enumerate(encoders)}
        self._fused = None
        self.fusion_module.to(device)
        for name, net in list(encoders.items()) + list(decoders.items()):
            self.add_module(name, net)
            net.to(device)

    def loss_func(self, pred, label):
        total, log = 0, {}
        for name in label:
            assert name in self.decoders, f"{name} must be in decoders"
        for name, target in label.items():
            log[name] = reconstruction_loss_func(name)(pred[name], target)
            total = total + log[name]
        return total, log

    def cross_modal_encode(self, x_dict):
        n = next(iter(x_dict.values())).size(0)
        stack = torch.zeros(n, len(self.encoders) * self.latent_dim, device=self.device)
        for name, x in x_dict.items():
            p = self.position_dict[name]
            stack[:, p * self.latent_dim:(p + 1) * self.latent_dim] = self.encoders[name](x)
        return self.fusion_module(stack)

    def cross_modal_decode(self, z):
        return {name: dec(z) for name, dec in self.decoders.items()}

    def enable_fused_inference(self, on=True):
        """Route the eval-mode forward on a GPU through the HIP kernels (csrc/shf_conv.hip, csrc/shf_mlp.hip); the returned
        tensors then carry no autograd graph.  Train mode always runs the torch modules.  A structure the kernels do not
        cover raises here, with the reason -- there is no silent fall-back."""
        if not on:
            self._fused = None
            return self
        from .fused import FusedRegressor
        self._fused = FusedRegressor(self)
        return self

    @property
    def fused(self):
        """The FusedRegressor behind enable_fused_inference(), or None while it is off."""
        return self._fused

    def forward_from_camera(self, camera_sensor):
        """The fused eval forward straight from a CameraSensor's rendered rgba / depth images: bit for bit
        forward({'rgb': color_buf.permute(0, 3, 1, 2), 'depth': depth_buf.unsqueeze(1)}) of a sensor with image_normalization,
        without the normalise / negate copies.  Needs enable_fused_inference() and eval mode on a GPU."""
        if self._fused is None or self.training or not self._fused.on_gpu():
            raise RuntimeError("forward_from_camera needs enable_fused_inference() and a model in eval mode on a GPU")
        return self._fused.from_camera(camera_sensor)

    def forward(self, joint_dict):
        for name in joint_dict:
            assert name in self.encoders, f"{name} must be in encoders"
        if self._fused is not None and not self.training and self._fused.on_gpu():
            return self._fused(joint_dict)
        return self.cross_modal_decode(self.cross_modal_encode(joint_dict))
