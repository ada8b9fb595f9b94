"""Base class of the trainable models ModuleRunner drives (reference shifu/models/module.py)."""
import os

import torch
from torch import nn


class Module(nn.Module):
    def __init__(self, device='cuda:0'):
        super().__init__()
        self.device = device

    def loss_func(self, pred, label):
        raise NotImplementedError

    def _checkpoint(self, logdir):
        return os.path.join(logdir, type(self).__name__ + ".pt")

    def save(self, logdir):
        torch.save(self.state_dict(), self._checkpoint(logdir))

    def load(self, logdir):
        self.load_state_dict(torch.load(self._checkpoint(logdir), map_location=self.device))
        self.eval()
