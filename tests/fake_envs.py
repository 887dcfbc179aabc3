"""CPU stand-ins for MultiSnakeVecEnv with the device-side surface selfplay.learn() uses; shared by the host tests of the
trainers."""
import torch

import msnake


class FakeEnv:
    """CPU stand-in with the device-side surface learn() uses (reset_device / step_device)."""

    def __init__(self, n=8, n_snakes=2, seed=0):
        self.num_envs, self.n_snakes, self.obs_shape, self.device = n, n_snakes, (12, 12, 9), torch.device("cpu")
        self.g = torch.Generator().manual_seed(seed)
        self.len = torch.zeros(n, dtype=torch.int32)

    def reset_device(self):
        return torch.randint(0, 256, (self.num_envs,) + self.obs_shape, dtype=torch.uint8, generator=self.g)

    def step_device(self, actions):
        assert actions.shape == (self.num_envs, self.n_snakes) and actions.dtype == torch.int32
        self.len += 1
        done = (torch.rand(self.num_envs, generator=self.g) < 0.3)
        rew = torch.randint(0, 2, (self.num_envs,), generator=self.g).float()
        info = torch.zeros((self.num_envs, 4), dtype=torch.int32)
        info[:, 0] = torch.full((self.num_envs,), 7.0).view(torch.int32)
        info[:, 1] = self.len
        self.len = torch.where(done, torch.zeros_like(self.len), self.len)
        return self.reset_device(), rew, done.to(torch.uint8), info


class FakeLocalEnv:
    """CPU stand-in with the device-side surface learn(local_radius=...) uses: frames nobody looks at, seeded windows and
    headings through render_local_device, and a record of every call."""

    def __init__(self, n=8, n_snakes=3, seed=0):
        self.num_envs, self.n_snakes, self.obs_shape, self.device = n, n_snakes, (12, 12, 9), torch.device("cpu")
        self.g = torch.Generator().manual_seed(seed)
        self.renders, self.actions = [], []

    def reset_device(self):
        return torch.zeros((self.num_envs,) + self.obs_shape, dtype=torch.uint8)

    def local_shape(self, radius, snakes=None):
        return msnake.MultiSnakeVecEnv.local_shape(self, radius, snakes)

    def render_local_device(self, radius, snakes=None, oriented=True, out=None, heading_out=None):
        assert tuple(out.shape) == (self.num_envs,) + self.local_shape(radius, snakes) and out.dtype == torch.uint8
        assert tuple(heading_out.shape) == tuple(out.shape[:2]) and heading_out.dtype == torch.uint8
        out.copy_(torch.randint(0, 7, out.shape, dtype=torch.uint8, generator=self.g))
        heading_out.copy_(torch.randint(0, 4, heading_out.shape, dtype=torch.uint8, generator=self.g))
        self.renders.append((radius, list(snakes), bool(oriented)))
        return out, heading_out

    def step_device(self, actions):
        assert actions.shape == (self.num_envs, self.n_snakes) and actions.dtype == torch.int32
        assert int(actions.min()) >= 0 and int(actions.max()) <= 4
        self.actions.append(actions.clone())
        done = torch.rand(self.num_envs, generator=self.g) < 0.3
        info = torch.zeros((self.num_envs, 4), dtype=torch.int32)
        info[:, 0] = torch.full((self.num_envs,), 7.0).view(torch.int32)
        return self.reset_device(), torch.ones(self.num_envs), done.to(torch.uint8), info
