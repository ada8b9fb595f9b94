"""A vectorised env served as a torch Dataset: item i is what one more env step of `batch_size` envs gives.

ModuleRunner iterates `for data, label in dataset`, which Python turns into dataset[0], dataset[1], ... until an
IndexError.  The dataset therefore ends itself: asking for an item at or past `num_data` tears the env down and raises.
Subclasses override __getitem__ to return (data dict, label dict); `end_if_past` and `random_actions` are the two pieces
they need from here."""
import numpy as np
import torch
from torch.utils.data import Dataset

from .torch_utils import free_tensor_attrs


def to_np(tensor, dtype=np.float32):
    """A host numpy copy of `tensor` (cut from autograd) in `dtype`."""
    return np.array(tensor.detach().to("cpu").numpy(), dtype=dtype)


class ShifuDataset(Dataset):
    def __init__(self, env_class, env_cfg, batch_size, num_data, render_mode=0):
        env_cfg.num_envs = batch_size
        env_cfg.debug.headless = render_mode == 0
        self.num_data = int(num_data)
        self.env = env_class(env_cfg)
        # Datasets written against the reference count their items with `self._ctr += 1` in __getitem__, so the attribute
        # has to exist; nothing here reads it.
        self._ctr = 0
        self.reset()
        self.scatter_episode_phases()

    def scatter_episode_phases(self):
        """Put every env at a random point of its episode, so that the time-outs do not arrive in one item."""
        env = self.env
        horizon = max(int(env.max_episode_length), 1)
        env.episode_length_buf = torch.randint(0, horizon, (env.num_envs,), device=env.device)

    def random_actions(self, low=0., high=1.):
        """(num_envs, num_actions) actions, uniform in [low, high)."""
        env = self.env
        u = torch.rand((env.num_envs, env.cfg.num_actions), device=env.device)
        return u if (low, high) == (0., 1.) else low + (high - low) * u

    def end_if_past(self, index):
        if index >= self.num_data:
            self.destroy()
            raise IndexError(f"item {index} of a dataset of {self.num_data}")

    def reset(self):
        self._ctr = 0
        self.env.reset()

    def destroy(self):
        self.env.destroy()
        free_tensor_attrs(self)

    def __len__(self):
        return self.num_data

    def __getitem__(self, index):
        self.end_if_past(index)
        obs, privileged_obs = self.env.step(self.random_actions())[:2]
        return obs, privileged_obs
