"""Self-play PPO driver on PyTorch-ROCm over the HIP env (BASELINE.json configs[4]).

A caller of the hot path, kept deliberately thin: it reproduces the structure of the reference's
`src/ppo_multi_agent.py` so that the env API is exercised exactly as there, with observations,
actions, rewards and dones staying on the GPU end to end (the reference moves every frame through
n pipes and NumPy, and sleeps 0.1 s per rollout step, ppo_multi_agent.py:175).

  reference                                         here
  policies.py:12-30  nature_cnn / custom_cnn        CnnPolicy (same layers, orthogonal init, /255)
  policies.py:45-59  CategoricalPd sample / neglogp Gumbel-max sample, cross-entropy neglogp
  ppo_multi_agent.py:23-53  MultiModel.multi_step   Runner.multi_step (opponent None -> action 1)
  ppo_multi_agent.py:164-168 channel slicing        obs[..., 0:3] / [3:6] / [6:9]
  ppo_multi_agent.py:205-214 GAE                    gae()
  ppo_multi_agent.py:72-86, 98-99 clipped PPO loss  ppo_loss() (+ per-minibatch advantage norm)
  ppo_multi_agent.py:314-322, 349-364 opponent pool OpponentPool (save every 50 updates, <= 1000,
                                                    uniform sampling)
  ppo_multi_agent.py:366-390 log keys               same key names; CSVLogger writes them in
                                                    baselines' logger.CSVOutputFormat layout, so
                                                    src/plotting.py reads the file unchanged
  baselines/bench/monitor.py:29-32,66-75            MonitorCSV ('#{json}' line, then r,l,t rows)
Parity with the reference here is statistical (learning curves), not bit-exact.
"""
import json
import os
import random
import time
from collections import deque

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ._capi import SCRIPTED_POLICY_NAMES as SCRIPTED_POLICIES
from ._capi import SCRIPTED_OPPONENT_NAMES as SCRIPTED_OPPONENTS  # SCRIPTED_POLICIES and path_greedy
from ._capi import SCRIPTED_PLAYER_NAMES as SCRIPTED_PLAYERS  # SCRIPTED_OPPONENTS and timed_greedy
from ._capi import SCRIPTED_NAMES  # SCRIPTED_PLAYERS and wary_greedy: what a ScriptedOpponent may play
from ._capi import AGENT_ENDED, AGENT_WAS_ALIVE
from ._capi import CAUSE_BODY, CAUSE_HEAD_ON, CAUSE_SELF, CAUSE_WALL
from ._capi import RULES
from .vec_env import check_radius, relative_to_absolute


# ----------------------------------------------------------------------------- policy
def _ortho(module, scale):
    nn.init.orthogonal_(module.weight, gain=scale)
    nn.init.zeros_(module.bias)
    return module


class CnnPolicy(nn.Module):
    """policies.py CnnPolicy: custom_cnn (4 x conv3x3 SAME, 32-32-64-64, fc512) for native frames,
    nature_cnn (8/4, 4/2, 3/1, fc512) for 84x84 frames; pi head init 0.01, value head init 1."""

    # MIOpen (ROCm 7.2, no tuning db in this image) falls back to a ~60x slower solver for these
    # small-image convolutions (a) when the input is NHWC-strided -- which a permuted view of the
    # env's HWC frames is, hence the .contiguous() below: backward 237 ms -> 4 ms at B=1024 on
    # MI355X -- and (b) once the batch exceeds a few thousand frames (1.9 s at B=8192), so the
    # trunk runs on plain NCHW batch chunks.
    CONV_CHUNK = 1024

    def __init__(self, ob_shape, n_actions=5, atari_size=None, amp_dtype=None):
        super().__init__()
        # opt-in mixed precision (torch.bfloat16): the trunk runs under autocast on MFMA, parameters,
        # heads' outputs, loss and optimizer stay fp32.  The reference trains in fp32, so None is the default.
        self.amp_dtype = amp_dtype
        h, w, c = ob_shape
        atari_size = (h == 84) if atari_size is None else atari_size
        g = float(np.sqrt(2))
        if atari_size:
            convs = [_ortho(nn.Conv2d(c, 32, 8, 4), g), nn.ReLU(), _ortho(nn.Conv2d(32, 64, 4, 2), g), nn.ReLU(),
                     _ortho(nn.Conv2d(64, 64, 3, 1), g), nn.ReLU()]
        else:
            convs = [_ortho(nn.Conv2d(c, 32, 3, 1, 1), g), nn.ReLU(), _ortho(nn.Conv2d(32, 32, 3, 1, 1), g), nn.ReLU(),
                     _ortho(nn.Conv2d(32, 64, 3, 1, 1), g), nn.ReLU(), _ortho(nn.Conv2d(64, 64, 3, 1, 1), g), nn.ReLU()]
        self.convs = nn.Sequential(*convs)
        with torch.no_grad():
            nflat = self.convs(torch.zeros(1, c, h, w)).numel()
        self.fc1 = _ortho(nn.Linear(nflat, 512), g)
        self.pi = _ortho(nn.Linear(512, n_actions), 0.01)
        self.v = _ortho(nn.Linear(512, 1), 1.0)

    def forward(self, ob_u8):
        """ob_u8: uint8 [B, H, W, 3] (NHWC like the env emits) -> logits [B, A], value [B]."""
        feats = []
        with torch.autocast(ob_u8.device.type, dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
            for i in range(0, ob_u8.shape[0], self.CONV_CHUNK):
                x = ob_u8[i:i + self.CONV_CHUNK].permute(0, 3, 1, 2).contiguous().float() / 255.0  # plain NCHW
                feats.append(self.convs(x).flatten(1))
            x = F.relu(self.fc1(torch.cat(feats) if len(feats) > 1 else feats[0]))
            logits, v = self.pi(x), self.v(x)[:, 0]
        return logits.float(), v.float()

    @torch.no_grad()
    def step(self, ob_u8):
        logits, v = self(ob_u8)
        u = torch.rand_like(logits).clamp_(1e-20, 1.0)
        a = torch.argmax(logits - torch.log(-torch.log(u)), dim=-1)  # CategoricalPd.sample (Gumbel-max)
        return a, v, neglogp(logits, a)

    @torch.no_grad()
    def value(self, ob_u8):
        return self(ob_u8)[1]


class WindowPolicy(CnnPolicy):
    """CnnPolicy's four-conv trunk, fc512 and two heads (same initialisation) over a head-centred window of cell codes
    (MultiSnakeVecEnv.render_local_device): the input is uint8 [B, W, W], W = 2 * radius + 1, one-hot encoded over the seven
    codes (0 empty, 1 fruit, 2 / 3 own body / head, 4 / 5 another snake's, 6 outside the grid) into seven NCHW channels.
    The input has one shape on every board, and with oriented windows it looks the same from every snake in every
    direction, so one set of weights can play any column of the action buffer.  The radius and the orientation flag the
    weights were trained under travel with them as the buffer `local_window` (load_weights refuses the other kind)."""

    N_CODES = 7

    def __init__(self, radius, n_actions=5, amp_dtype=None, oriented=True):
        radius = check_radius(radius)
        w = 2 * radius + 1
        super().__init__((w, w, self.N_CODES), n_actions=n_actions, atari_size=False, amp_dtype=amp_dtype)
        self.radius, self.oriented = radius, bool(oriented)
        self.register_buffer("local_window", torch.tensor([radius, int(self.oriented)], dtype=torch.int64))
        self.register_buffer("codes", torch.arange(self.N_CODES, dtype=torch.uint8).view(1, self.N_CODES, 1, 1), persistent=False)

    def forward(self, win_u8):
        """win_u8: uint8 [B, W, W] cell codes -> logits [B, A], value [B]."""
        w = 2 * self.radius + 1
        if win_u8.dim() != 3 or tuple(win_u8.shape[1:]) != (w, w) or win_u8.dtype != torch.uint8:
            raise ValueError(f"expected uint8 windows of shape [B, {w}, {w}], got {win_u8.dtype} {tuple(win_u8.shape)}")
        feats = []
        with torch.autocast(win_u8.device.type, dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
            for i in range(0, win_u8.shape[0], self.CONV_CHUNK):
                x = (win_u8[i:i + self.CONV_CHUNK].unsqueeze(1) == self.codes).float()  # plain NCHW, one channel per code
                feats.append(self.convs(x).flatten(1))
            x = F.relu(self.fc1(torch.cat(feats) if len(feats) > 1 else feats[0]))
            logits, v = self.pi(x), self.v(x)[:, 0]
        return logits.float(), v.float()


class RayPolicy(nn.Module):
    """An MLP over one snake's eight-direction rays (MultiSnakeVecEnv.render_rays_device): the input is uint8 [B, 8, 4],
    steps to the wall, the first fruit, the first piece of the own body and the first piece of another snake per
    direction.  Features are 1 / d where d > 0, else 0 (near things are large, absent things vanish), flattened to 32;
    two hidden layers of 64, five logits and a value, initialised like CnnPolicy's layers and heads.  No convolution.
    It has CnnPolicy's step / value surface; under oriented rays its actions are relative to the heading
    (relative_to_absolute), and one set of weights can play any column of the action buffer.  The orientation flag the
    weights were trained under travels with them as the buffer `ray_input` (load_weights refuses another kind)."""

    N_IN = 8 * 4
    HIDDEN = 64

    def __init__(self, n_actions=5, amp_dtype=None, oriented=True):
        super().__init__()
        self.amp_dtype, self.oriented = amp_dtype, bool(oriented)
        g = float(np.sqrt(2))
        self.fc1 = _ortho(nn.Linear(self.N_IN, self.HIDDEN), g)
        self.fc2 = _ortho(nn.Linear(self.HIDDEN, self.HIDDEN), g)
        self.pi = _ortho(nn.Linear(self.HIDDEN, n_actions), 0.01)
        self.v = _ortho(nn.Linear(self.HIDDEN, 1), 1.0)
        self.register_buffer("ray_input", torch.tensor([int(self.oriented)], dtype=torch.int64))

    @staticmethod
    def features(rays_u8):
        """uint8 [B, 8, 4] -> float32 [B, 32]: 1 / d where d > 0, else 0."""
        d = rays_u8.flatten(1).float()
        return torch.where(d > 0, 1.0 / d.clamp(min=1.0), torch.zeros_like(d))

    def forward(self, rays_u8):
        """rays_u8: uint8 [B, 8, 4] -> logits [B, A], value [B]."""
        if rays_u8.dim() != 3 or tuple(rays_u8.shape[1:]) != (8, 4) or rays_u8.dtype != torch.uint8:
            raise ValueError(f"expected uint8 rays of shape [B, 8, 4], got {rays_u8.dtype} {tuple(rays_u8.shape)}")
        with torch.autocast(rays_u8.device.type, dtype=self.amp_dtype or torch.bfloat16, enabled=self.amp_dtype is not None):
            x = F.relu(self.fc2(F.relu(self.fc1(self.features(rays_u8)))))
            logits, v = self.pi(x), self.v(x)[:, 0]
        return logits.float(), v.float()

    step, value = CnnPolicy.step, CnnPolicy.value


def window_kind(state_dict):
    """What a weights file was trained on, as far as windows go: None for anything else, (radius, oriented) for windows."""
    t = state_dict.get("local_window")
    return None if t is None else (int(t[0]), bool(int(t[1])))


def ray_kind(state_dict):
    """Likewise for rays: None for anything else, (oriented,) for rays."""
    t = state_dict.get("ray_input")
    return None if t is None else (bool(int(t[0])),)


def _kind_text(kind):
    """kind: None for full frames, (radius, oriented) for windows, (oriented,) for rays."""
    if kind is None:
        return "full frames"
    what = f"windows of radius {kind[0]}" if len(kind) == 2 else "rays"
    return f"{what}, {'oriented' if kind[-1] else 'not oriented'}"


def check_kind(model, state_dict, path):
    want = ((model.radius, model.oriented) if isinstance(model, WindowPolicy) else
            (model.oriented,) if isinstance(model, RayPolicy) else None)
    got = window_kind(state_dict) or ray_kind(state_dict)
    if got != want:
        raise RuntimeError(f"{path} holds a policy trained on {_kind_text(got)}; this run trains on {_kind_text(want)} "
                           "(local_radius / rays / oriented): the weights cannot be loaded")


def neglogp(logits, actions):
    return F.cross_entropy(logits, actions, reduction="none")


def entropy(logits):
    a0 = logits - logits.max(dim=-1, keepdim=True).values
    ea0 = torch.exp(a0)
    z0 = ea0.sum(dim=-1, keepdim=True)
    return (ea0 / z0 * (torch.log(z0) - a0)).sum(dim=-1)


# ----------------------------------------------------------------------------- PPO math
def gae(rewards, values, dones, last_values, last_dones, gamma=0.99, lam=0.95):
    """ppo_multi_agent.py:205-214.  rewards/values/dones: [T, N] where dones[t] is the done flag
    that PRECEDED step t (mb_dones), last_dones the flags after the last step."""
    T = rewards.shape[0]
    advs = torch.zeros_like(rewards)
    lastgaelam = torch.zeros_like(last_values)
    for t in reversed(range(T)):
        if t == T - 1:
            nextnonterminal, nextvalues = 1.0 - last_dones, last_values
        else:
            nextnonterminal, nextvalues = 1.0 - dones[t + 1], values[t + 1]
        delta = rewards[t] + gamma * nextvalues * nextnonterminal - values[t]
        advs[t] = lastgaelam = delta + gamma * lam * nextnonterminal * lastgaelam
    return advs + values, advs


def agent_targets(rew, val, flags, last_val, gamma=0.99, lam=0.95):
    """GAE targets for every snake of every env from the outputs of MultiSnakeVecEnv.agent_outcomes_device.  rew, val:
    float [T, N, S]; flags: uint8 [T, N, S] (AGENT_* bits); last_val: float [N, S], the values behind the last step.
    Returns (returns float [T, N, S], valid bool [T, N, S]).  A sample is valid iff WAS_ALIVE (the snake acted in that
    step) and terminal iff ENDED (it died, or the env's episode ended).  An invalid sample contributes nothing -- its
    return is 0 -- and cuts the recursion, and a run of valid samples that stops in front of an invalid one without
    ENDED is closed like a terminal one: there is no value to bootstrap from.  So on each agent's maximal runs of valid
    samples the result equals gae() run on that run alone."""
    valid, ended = (flags & AGENT_WAS_ALIVE) != 0, (flags & AGENT_ENDED) != 0
    T = rew.shape[0]
    advs = torch.zeros_like(rew)
    lastgaelam = torch.zeros_like(last_val)
    zero = torch.zeros_like(last_val)
    for t in reversed(range(T)):
        goes_on = ~ended[t] if t == T - 1 else ~ended[t] & valid[t + 1]
        nextnonterminal = goes_on.to(rew.dtype)
        nextvalues = torch.where(goes_on, last_val if t == T - 1 else val[t + 1], zero)
        delta = rew[t] + gamma * nextvalues * nextnonterminal - val[t]
        lastgaelam = torch.where(valid[t], delta + gamma * lam * nextnonterminal * lastgaelam, zero)
        advs[t] = lastgaelam
    return torch.where(valid, advs + val, torch.zeros_like(val)), valid


def ppo_loss(logits, vpred, actions, returns, old_values, old_neglogp, cliprange, ent_coef=0.01, vf_coef=0.5):
    """ppo_multi_agent.py:72-86 with the advantage normalisation of :98-99."""
    advs = returns - old_values
    advs = (advs - advs.mean()) / (advs.std(unbiased=False) + 1e-8)
    nlp = neglogp(logits, actions)
    ent = entropy(logits).mean()
    vclipped = old_values + torch.clamp(vpred - old_values, -cliprange, cliprange)
    vf_loss = 0.5 * torch.max((vpred - returns) ** 2, (vclipped - returns) ** 2).mean()
    ratio = torch.exp(old_neglogp - nlp)
    pg_loss = torch.max(-advs * ratio, -advs * torch.clamp(ratio, 1.0 - cliprange, 1.0 + cliprange)).mean()
    approxkl = 0.5 * ((nlp - old_neglogp) ** 2).mean()
    clipfrac = ((ratio - 1.0).abs() > cliprange).float().mean()
    loss = pg_loss - ent * ent_coef + vf_loss * vf_coef
    return loss, {"policy_loss": pg_loss, "value_loss": vf_loss, "policy_entropy": ent, "approxkl": approxkl,
                  "clipfrac": clipfrac}


def explained_variance(ypred, y):
    vary = y.var(unbiased=False)
    return float("nan") if float(vary) == 0 else float(1 - (y - ypred).var(unbiased=False) / vary)


# ----------------------------------------------------------------------------- opponent pool, logs
def save_weights(model, path):
    """Model.save (ppo_multi_agent.py:112-114: joblib.dump of the parameter list): here a plain
    state_dict of tensors, written atomically, loadable with torch.load(weights_only=True)."""
    tmp = path + ".tmp"
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, tmp)
    os.replace(tmp, path)


def load_weights(model, path):
    """Model.load (ppo_multi_agent.py:124-132).  weights_only: nothing in the file is executed."""
    state_dict = torch.load(path, map_location=next(model.parameters()).device, weights_only=True)
    check_kind(model, state_dict, path)
    model.load_state_dict(state_dict)


class OpponentPool:
    """Ring of past policies (config.py:13-14: save every 50 updates, keep <= 1000).  Held in device
    memory; with `directory` every save is also written through to `opponent<which>_<idx>.pt`
    (utils.py:57-64 names opponent1_<x>.pkl / opponent2_<x>.pkl) so a later run can restore the pool."""

    def __init__(self, max_saved=1000, directory=None, which=1):
        self.max_saved, self.slots, self.idx, self.num = max_saved, {}, 0, 0
        self.directory, self.which = directory, which

    def file(self, idx):
        return os.path.join(self.directory, f"opponent{self.which}_{idx}.pt")

    def save(self, model):
        self.slots[self.idx] = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if self.directory:
            save_weights(model, self.file(self.idx))
        self.idx += 1
        self.num = max(self.idx, self.num)
        self.idx %= self.max_saved

    def restore(self, device, idx, num):
        """Reload slots 0..num-1 from `directory` and continue writing at `idx` (resume)."""
        for i in range(num):
            self.slots[i] = torch.load(self.file(i), map_location=device, weights_only=True)
        self.idx, self.num = idx, num

    def load_random(self, model, rng=random):
        sel = rng.randint(0, max(self.num - 1, 0))  # ppo_multi_agent.py:315
        model.load_state_dict(self.slots[sel])
        return sel


class CSVLogger:
    """Same file layout as baselines.logger.CSVOutputFormat (logger.py:101-135): a header of keys,
    one row per writekvs, the header rewritten when new keys appear."""

    def __init__(self, filename):
        self.file, self.keys = open(filename, "w+t"), []

    def writekvs(self, kvs):
        extra = [k for k in kvs if k not in self.keys]
        if extra:
            self.keys.extend(extra)
            self.file.seek(0)
            lines = self.file.readlines()
            self.file.seek(0)
            self.file.write(",".join(self.keys) + "\n")
            for line in lines[1:]:
                self.file.write(line[:-1] + "," * len(extra) + "\n")
        self.file.write(",".join("" if kvs.get(k) is None else str(kvs.get(k)) for k in self.keys) + "\n")
        self.file.flush()

    def close(self):
        self.file.close()


class JSONLogger:
    """baselines.logger.JSONOutputFormat (logger.py:86-99): one JSON object per writekvs, per line."""

    def __init__(self, filename):
        self.file = open(filename, "wt")

    def writekvs(self, kvs):
        self.file.write(json.dumps({k: (float(v) if hasattr(v, "dtype") else v) for k, v in kvs.items()}) + "\n")
        self.file.flush()

    def close(self):
        self.file.close()


def _crc32c_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ 0x82F63B78 if c & 1 else c >> 1
        t.append(c)
    return t


_CRC32C = _crc32c_table()


def crc32c(data):
    c = 0xFFFFFFFF
    for b in data:
        c = _CRC32C[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def _masked_crc(data):
    c = crc32c(data)
    return (((c >> 15) | (c << 17)) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(n):
    out = bytearray()
    while True:
        b = n & 0x7F
        n >>= 7
        out.append(b | (0x80 if n else 0))
        if not n:
            return bytes(out)


class TensorBoardLogger:
    """baselines.logger.TensorBoardOutputFormat (logger.py:136-170) without TensorFlow: an
    `events.out.tfevents.*` file of TFRecord-framed Event protos (wall_time, step, one
    Summary.Value{tag, simple_value} per key), step counting from 1 like the reference.  The few
    proto fields involved are encoded by hand; records carry the masked CRC32C TensorBoard checks."""

    def __init__(self, directory):
        import socket
        import struct
        self._struct = struct
        os.makedirs(directory, exist_ok=True)
        self.path = os.path.join(directory, "events.out.tfevents.%d.%s" % (int(time.time()), socket.gethostname()))
        self.file = open(self.path, "wb")
        self.step = 1
        ver = b"brain.Event:2"
        self._record(b"\x09" + struct.pack("<d", time.time()) + b"\x1a" + _varint(len(ver)) + ver)

    def _record(self, data):
        st = self._struct
        head = st.pack("<Q", len(data))
        self.file.write(head + st.pack("<I", _masked_crc(head)) + data + st.pack("<I", _masked_crc(data)))
        self.file.flush()

    def writekvs(self, kvs):
        st = self._struct
        summary = b""
        for k, v in kvs.items():
            tag = str(k).encode()
            value = b"\x0a" + _varint(len(tag)) + tag + b"\x15" + st.pack("<f", float(v))
            summary += b"\x0a" + _varint(len(value)) + value
        event = (b"\x09" + st.pack("<d", time.time()) + b"\x10" + _varint(self.step) +
                 b"\x2a" + _varint(len(summary)) + summary)
        self._record(event)
        self.step += 1

    def close(self):
        self.file.close()


class MonitorCSV:
    """baselines.bench.Monitor's file: '#{"t_start":..,"env_id":..}' then r,l,t rows."""

    def __init__(self, filename, env_id=None):
        self.f = open(filename, "wt")
        self.f.write("#%s\n" % json.dumps({"t_start": time.time(), "env_id": env_id}))
        self.f.write("r,l,t\n")

    def write(self, epinfos):
        for ep in epinfos:
            self.f.write(f"{ep['r']},{ep['l']},{ep['t']}\n")
        self.f.flush()

    def close(self):
        self.f.close()


# ----------------------------------------------------------------------------- scripted opponents
class ScriptedColumns:
    """The scripted action columns of a team of ScriptedOpponents of one env, in a buffer of its own: refresh() fills the
    columns of every member with ONE env call per policy, each member's step() then reads its own.  Whoever drives the
    env calls refresh() once per env step, before the members' step() (Runner.multi_step does)."""

    def __init__(self, env):
        self.env, self.members, self.filled = env, [], False
        self.buf = torch.zeros((env.num_envs, env.n_snakes), dtype=torch.int32, device=env.device)

    def add(self, member):
        if any(m.snake == member.snake for m in self.members):
            raise ValueError(f"snake {member.snake} already has a scripted opponent in this team")
        self.members.append(member)
        self.filled = False

    def refresh(self):
        by_policy = {}
        for m in self.members:
            by_policy.setdefault(m.policy, []).append(m.snake)
        for policy, snakes in by_policy.items():
            self.env.scripted_actions_device(policy, snakes=sorted(snakes), out=self.buf)
        self.filled = True

    def column(self, snake):
        if not self.filled:
            raise RuntimeError("ScriptedColumns.refresh() has not been called since the team was put together")
        return self.buf[:, snake].to(torch.int64)  # (a copy: the next refresh() overwrites the buffer)


class ScriptedOpponent:
    """A fixed, deterministic opponent in the place of a CnnPolicy: snake `snake` plays the env's on-device scripted
    `policy` (one of SCRIPTED_NAMES, MultiSnakeVecEnv.scripted_actions_device).  step(obs) has the shape
    Runner.multi_step calls; the observation is ignored, the env's state is asked.  eps > 0: with probability eps
    the action is replaced by randint(0, 5), drawn with torch on the env's device from `generator` (the env's own
    random numbers are never used).  On its own (columns=None) every step() is one env call.  Several opponents of one
    env given the same ScriptedColumns form a team: one env call per policy and env step for all of them, made by
    columns.refresh(), which the driver calls before the members' step()."""

    def __init__(self, env, policy, snake, eps=0.0, generator=None, columns=None):
        if policy not in SCRIPTED_NAMES:
            raise ValueError(f"policy must be one of {', '.join(map(repr, SCRIPTED_NAMES))}, got {policy!r}")
        if not 0 <= int(snake) < env.n_snakes:
            raise ValueError(f"snake must lie in [0, {env.n_snakes}), got {snake!r}")
        self.env, self.policy, self.snake, self.eps, self.generator = env, policy, int(snake), float(eps), generator
        self.own = columns is None
        self.columns = ScriptedColumns(env) if columns is None else columns
        if self.columns.env is not env:
            raise ValueError("columns belongs to another env")
        self.columns.add(self)

    def step(self, obs=None):
        if self.own:
            self.columns.refresh()
        a = self.columns.column(self.snake)
        if self.eps > 0.0:
            swap = torch.rand(a.shape, device=a.device, generator=self.generator) < self.eps
            rnd = torch.randint(0, 5, a.shape, device=a.device, generator=self.generator)
            a = torch.where(swap, rnd, a)
        return a, None, None


def refresh_scripted(opponents):
    """One refresh() per team among `opponents` (lone ScriptedOpponents ask the env in their own step())."""
    teams = {id(o.columns): o.columns for o in opponents if isinstance(o, ScriptedOpponent) and not o.own}
    for columns in teams.values():
        columns.refresh()


# ----------------------------------------------------------------------------- rollouts
# what a rollout with death causes adds to an update's log: snakes that died by each cause (a death may count under
# more than one) and deaths on another snake's body, credited to that snake
DEATH_KEYS = ("deaths_wall", "deaths_self", "deaths_head_on", "deaths_body", "kills")


def body_kills(victims):
    """How many snakes ran into this snake's body: the set bits among bits 0..3 of msnake_death_causes' victims bytes."""
    v = victims.to(torch.int32)
    return (v & 1) + ((v >> 1) & 1) + ((v >> 2) & 1) + ((v >> 3) & 1)


def check_random_starts(random_starts, start_lengths, env=None):
    """(p, (lo, hi)) of Runner / learn: a probability and a range of body lengths, lo <= hi, as the generator takes them.
    With p > 0 a new_world `env` is refused here, before the first rollout (scatter_device would refuse it in its first step)."""
    p = float(random_starts)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"random_starts must be a probability in [0, 1], got {random_starts!r}")
    try:
        lo, hi = (int(x) for x in start_lengths)
    except (TypeError, ValueError):
        raise ValueError(f"start_lengths must be two ints (lo, hi), got {start_lengths!r}") from None
    if not 0 <= lo <= hi < 2 ** 31 or (lo, hi) != tuple(start_lengths):
        raise ValueError(f"start_lengths must be two ints with 0 <= lo <= hi, got {start_lengths!r}")
    if p > 0.0 and getattr(getattr(env, "cfg", None), "rules", None) == RULES["new_world"]:
        raise ValueError("random_starts > 0 needs a snake_env or adversarial env: new_world positions cannot be generated")
    return p, (lo, hi)


class Runner:
    """ppo_multi_agent.py:145-216 with everything on the device."""

    def __init__(self, env, model, opponents, nsteps, gamma, lam, local_radius=None, oriented=True, rays=False, all_snakes=False,
                 kill_bonus=0.0, random_starts=0.0, start_lengths=(3, 3)):
        """all_snakes=True: every snake of every env is played by `model` on its own window or rays, and run() returns the
        samples of all of them (agent_targets over env.step_agents_device).  Needs rays=True or local_radius, no
        opponents, and an env created with auto_reset=False.
        kill_bonus != 0 (all_snakes only; snake_env and adversarial): every step also asks why each snake died
        (step_agents_device(causes=True)), and a snake's reward grows by kill_bonus for every snake that ran into its body
        in that step.  With 0 the rollout is what it is without the argument.
        random_starts = p > 0 (snake_env and adversarial): after each step, every env whose episode just ended starts its
        next one, with probability p, from a generated position (env.scatter_device) whose per-snake body lengths are
        uniform in start_lengths = (lo, hi) instead of from the reset; see scatter_done().  With 0 the rollout is what it
        is without the argument, and torch's generator is not asked."""
        self.random_starts, self.start_lengths = check_random_starts(random_starts, start_lengths, env)
        self.start_salt = 0  # the generator's salt: moves with every scatter_device() call
        if rays and local_radius is not None:
            raise ValueError("rays=True and local_radius are mutually exclusive: a run trains on rays or on windows")
        self.all_snakes, self.kill_bonus = bool(all_snakes), float(kill_bonus)
        if self.kill_bonus != 0.0 and not self.all_snakes:
            raise ValueError("kill_bonus needs all_snakes=True: only there does every snake's reward reach the learner")
        if self.all_snakes:
            if not rays and local_radius is None:
                raise ValueError("all_snakes=True needs rays=True or local_radius: one set of weights can play every column "
                                 "only on per-snake observations")
            if opponents:
                raise ValueError("all_snakes=True plays every snake with the learner's weights: there is no opponent to give")
            if getattr(env, "_ctor", {}).get("auto_reset", True):
                raise ValueError("all_snakes=True needs an env created with auto_reset=False (step_agents_device)")
            opponents = []
        self.env, self.model, self.opponents = env, model, opponents
        self.nsteps, self.gamma, self.lam = nsteps, gamma, lam
        self.local_radius, self.oriented, self.rays = local_radius, bool(oriented), bool(rays)
        self.per_snake = self.rays or local_radius is not None   # windows or rays instead of the frame
        self.obs = env.reset_device()
        if self.per_snake:
            # the learner and every network opponent see their own snake's window / rays: one env call for all of them
            self.win_snakes = [0] + [i + 1 for i, opp in enumerate(opponents) if isinstance(opp, nn.Module)]
            if self.all_snakes:
                self.win_snakes = list(range(env.n_snakes))
            self.slot = {s: q for q, s in enumerate(self.win_snakes)}
            shape = (env.num_envs,) + (env.rays_shape(self.win_snakes) if self.rays else env.local_shape(local_radius, self.win_snakes))
            self.win = torch.empty(shape, dtype=torch.uint8, device=self.obs.device)
            self.heading = torch.empty(shape[:2], dtype=torch.uint8, device=self.obs.device)
            self.observe_local()
        self.dones = torch.zeros(env.num_envs, dtype=torch.float32, device=self.obs.device)
        self.tstart = time.time()

    def scatter_done(self, done):
        """Exploring starts: the envs of `done` (the step's done tensor), each with probability random_starts, are put onto
        a generated position.  Probability and lengths come from torch's generator on the env's device; nothing is
        synchronised, so the call is made whether or not an env was picked.  The frame is rendered again behind it; a
        window / ray runner reads its observation behind this anyway.  (On an all_snakes env the installed states make
        the next step arm the outcome tracker again: rewards and flags are unaffected, the tracker's episode totals of
        every env start over.)"""
        if self.random_starts == 0.0:
            return
        env, (lo, hi) = self.env, self.start_lengths
        pick = done.bool() & (torch.rand(env.num_envs, device=done.device) < self.random_starts)
        lengths = torch.randint(lo, hi + 1, (env.num_envs, env.n_snakes), dtype=torch.int32, device=done.device)
        self.start_salt += 1
        # compact=False: Warnsdorff's rule coils the body round its first piece, the head, and at 40 pieces on 19x19x3 leaves
        # every snake a safe move in 9 % of the positions against 66 % without it (README); a body that ends short is no loss here
        env.scatter_device(lengths, mask=pick, salt=self.start_salt, compact=False)
        if not self.per_snake:
            self.obs = env.render_device()

    def observe_local(self):
        if self.rays:
            self.env.render_rays_device(snakes=self.win_snakes, oriented=self.oriented, out=self.win, heading_out=self.heading)
        else:
            self.env.render_local_device(self.local_radius, snakes=self.win_snakes, oriented=self.oriented, out=self.win,
                                         heading_out=self.heading)

    def learner_obs(self):
        return self.win[:, 0] if self.per_snake else self.obs[..., 0:3]

    def absolute(self, a, snake):
        """A window / ray policy's sampled action as the step takes it: relative to the heading under `oriented`."""
        return relative_to_absolute(a, self.heading[:, self.slot[snake]]) if self.oriented else a

    def multi_step_local(self):
        a, v, nlp = self.model.step(self.win[:, 0])
        acts = [self.absolute(a, 0)]
        refresh_scripted(self.opponents)
        for i, opp in enumerate(self.opponents):
            if opp is None:
                acts.append(torch.ones_like(a))
            elif isinstance(opp, nn.Module):
                acts.append(self.absolute(opp.step(self.win[:, self.slot[i + 1]])[0], i + 1))
            else:
                acts.append(opp.step(None)[0])
        return a, v, nlp, torch.stack(acts, dim=1).to(torch.int32)

    def multi_step(self):
        if self.per_snake:
            return self.multi_step_local()
        a, v, nlp = self.model.step(self.obs[..., 0:3])
        acts = [a]
        refresh_scripted(self.opponents)
        for i, opp in enumerate(self.opponents):
            if opp is None:
                acts.append(torch.ones_like(a))  # ppo_multi_agent.py:32,37
            else:
                acts.append(opp.step(self.obs[..., 3 * (i + 1):3 * (i + 2)])[0])
        return a, v, nlp, torch.stack(acts, dim=1).to(torch.int32)

    def run_all_snakes(self):
        """run() for all_snakes=True: the batch is the valid (t, env, snake) samples, those in which the snake acted."""
        T, N, S = self.nsteps, self.env.num_envs, self.env.n_snakes
        dev = self.obs.device
        mb_obs = torch.empty((T,) + tuple(self.win.shape), dtype=torch.uint8, device=dev)
        mb_rew = torch.empty((T, N, S), device=dev); mb_val = torch.empty((T, N, S), device=dev)
        mb_nlp = torch.empty((T, N, S), device=dev); mb_flags = torch.empty((T, N, S), dtype=torch.uint8, device=dev)
        mb_act = torch.empty((T, N, S), dtype=torch.long, device=dev)
        ep_r, ep_l = [], []
        causes = self.kill_bonus != 0.0
        if causes:
            mb_cause = torch.empty((T, N, S), dtype=torch.uint8, device=dev); mb_victims = torch.empty_like(mb_cause)
        for t in range(T):
            a, v, nlp = self.model.step(self.win.flatten(0, 1))
            mb_obs[t] = self.win
            mb_act[t], mb_val[t], mb_nlp[t] = a.view(N, S), v.view(N, S), nlp.view(N, S)
            full = relative_to_absolute(a.view(N, S), self.heading) if self.oriented else a.view(N, S)
            if causes:
                self.obs, rew, done, info, agents, why = self.env.step_agents_device(full.to(torch.int32), causes=True)
                mb_cause[t], mb_victims[t] = why.cause, why.victims
            else:
                self.obs, rew, done, info, agents = self.env.step_agents_device(full.to(torch.int32))
            self.scatter_done(done)
            self.observe_local()
            mb_rew[t], mb_flags[t] = agents.rew, agents.flags  # (copies: the next step overwrites the env's tensors)
            self.dones = done.float()
            ep_r.append(torch.where(done.bool(), info[:, 0].view(torch.float32), torch.full_like(rew, float("nan"))))
            ep_l.append(info[:, 1].clone())  # `info` is the env's buffer: the next step overwrites it
        if causes:  # the snakes that ran into this snake's body (head-on meetings, bits 4.., credit nobody)
            kills = body_kills(mb_victims)
            self.last_agent_rew, self.last_cause, self.last_victims = mb_rew.clone(), mb_cause, mb_victims  # (tests)
            mb_rew += torch.where((mb_flags & AGENT_WAS_ALIVE) != 0, self.kill_bonus * kills.float(), torch.zeros_like(mb_rew))
            counts = torch.stack([((mb_cause & bit) != 0).sum() for bit in (CAUSE_WALL, CAUSE_SELF, CAUSE_HEAD_ON, CAUSE_BODY)] +
                                 [kills.sum()]).tolist()
            self.last_deaths = dict(zip(DEATH_KEYS, counts))
        self.last_rew = mb_rew
        last_values = self.model.value(self.win.flatten(0, 1)).view(N, S)
        returns, valid = agent_targets(mb_rew, mb_val, mb_flags, last_values, self.gamma, self.lam)
        self.last_flags = mb_flags  # (tests: the batch is exactly the WAS_ALIVE samples)
        r = torch.stack(ep_r).flatten(); l = torch.stack(ep_l).flatten()
        keep = ~torch.isnan(r)
        t_el = round(time.time() - self.tstart, 6)
        epinfos = [{"r": round(float(x), 6), "l": int(y), "t": t_el} for x, y in zip(r[keep].tolist(), l[keep].tolist())]
        idx = valid.flatten().nonzero()[:, 0]
        pick = lambda x: x.flatten(0, 2)[idx]
        ended = ((mb_flags & AGENT_ENDED) != 0).float()
        return pick(mb_obs), pick(returns), pick(ended), pick(mb_act), pick(mb_val), pick(mb_nlp), epinfos

    def run(self):
        if self.all_snakes:
            return self.run_all_snakes()
        T, N = self.nsteps, self.env.num_envs
        dev = self.obs.device
        mb_obs = torch.empty((T, N) + tuple(self.learner_obs().shape[1:]), dtype=torch.uint8, device=dev)
        mb_rew = torch.empty((T, N), device=dev); mb_val = torch.empty((T, N), device=dev)
        mb_nlp = torch.empty((T, N), device=dev); mb_done = torch.empty((T, N), device=dev)
        mb_act = torch.empty((T, N), dtype=torch.long, device=dev)
        ep_r, ep_l = [], []
        for t in range(T):
            a, v, nlp, full = self.multi_step()
            mb_obs[t] = self.learner_obs()
            mb_act[t], mb_val[t], mb_nlp[t], mb_done[t] = a, v, nlp, self.dones
            self.obs, rew, done, info = self.env.step_device(full)
            self.scatter_done(done)
            if self.per_snake:
                self.observe_local()
            mb_rew[t] = rew
            self.dones = done.float()
            ep_r.append(torch.where(done.bool(), info[:, 0].view(torch.float32), torch.full_like(rew, float("nan"))))
            ep_l.append(info[:, 1].clone())  # `info` is the env's buffer: the next step overwrites it
        last_values = self.model.value(self.learner_obs())
        returns, _ = gae(mb_rew, mb_val, mb_done, last_values, self.dones, self.gamma, self.lam)
        # episode infos: one host sync per rollout instead of one per step
        r = torch.stack(ep_r).flatten(); l = torch.stack(ep_l).flatten()
        keep = ~torch.isnan(r)
        t_el = round(time.time() - self.tstart, 6)
        epinfos = [{"r": round(float(x), 6), "l": int(y), "t": t_el} for x, y in zip(r[keep].tolist(), l[keep].tolist())]
        flat = lambda x: x.transpose(0, 1).reshape((T * N,) + tuple(x.shape[2:]))  # sf01
        return flat(mb_obs), flat(returns), flat(mb_done), flat(mb_act), flat(mb_val), flat(mb_nlp), epinfos


def learn(env, nsteps=64, total_timesteps=int(1e6), ent_coef=0.01, lr=lambda f: f * 2.5e-4, vf_coef=0.5,
          max_grad_norm=0.5, gamma=0.99, lam=0.95, log_interval=1, nminibatches=8, noptepochs=4,
          cliprange=lambda f: f * 0.1, opponent_save_interval=50, max_saved_opponents=1000, csv_path=None,
          monitor_path=None, seed=0, log_fn=print, amp_dtype=None, json_path=None, tb_dir=None,
          save_dir=None, save_interval=0, load_path=None, resume=False, scripted_opponents=None, local_radius=None,
          oriented=True, rays=False, all_snakes=False, kill_bonus=0.0, random_starts=0.0, start_lengths=(3, 3)):
    """ppo_multi_agent.py:231-404 (hyper-parameters of test/ppo1_single_test.py:42-47 as defaults).

    Checkpoints (ppo_multi_agent.py:112-133, 296-306, 349-364, 392-404), weights only, under `save_dir`
    (the reference's saved_models/<expr>/): the opponent pool as opponent<i>_<idx>.pt every
    `opponent_save_interval` updates, snake_model_num<N>_<k>.pt at update 1 and every `save_interval`
    updates, highscore_model.pt whenever the 100-episode mean passes the next integer above 5 (single
    snake only, :398-401), snake_model_num<N>.pt at the end.  `load_path` initialises the learner and
    its opponents from a weights file (the reference's `baseline_file`, :264-275).  `resume=True`
    continues a run from save_dir/trainer_state.pt (weights, Adam moments, update counter, pool
    positions -- the reference cannot do this; schedules continue where they stopped).
    `scripted_opponents`, e.g. {1: "safe_greedy"}: those snakes are played by a ScriptedOpponent (a fixed yardstick
    from update 1 on) instead of a past self; no pool is kept, saved or loaded for them.
    `local_radius`: the learner and its network opponents are WindowPolicies over their own snake's head-centred window
    of that radius (render_local_device) instead of CnnPolicies over the frame; under `oriented` the windows are turned
    along the heading and the sampled actions are relative to it (relative_to_absolute).  Weights and trainer states
    carry the radius and the flag: loading the other kind is refused.
    `rays=True`: the learner and its network opponents are RayPolicies over their own snake's eight-direction rays
    (render_rays_device, one env call per step for all of them), an MLP on 32 bytes per snake; `oriented` means the same
    as for windows.  Mutually exclusive with `local_radius`; weights and trainer states carry the kind here too.
    `all_snakes=True` (with `rays` or `local_radius`, an env created with auto_reset=False, no scripted opponents): every
    snake is played by the learner's current weights and every snake's transitions are learned from
    (Runner.run_all_snakes): the batch of an update is the valid (t, env, snake) samples, split into `nminibatches`
    parts.  No opponent pool is kept.  The episode statistics stay the env's own (snake 0), so curves remain comparable;
    the log gains agent_samples (the batch size) and sample_fps.
    `kill_bonus` != 0 (all_snakes only): a snake's reward grows by that much for every snake that ran into its body in
    the step (Runner, msnake_death_causes), and every update's log gains deaths_wall, deaths_self, deaths_head_on,
    deaths_body and kills, counted over its rollout.
    `random_starts` = p > 0 (snake_env and adversarial): an env whose episode just ended starts the next one, with
    probability p, from a position generated on the device with per-snake body lengths uniform in `start_lengths` = (lo,
    hi) (Runner.scatter_done, env.scatter_device): the late game as a place to start from.  Works with the frame, window,
    ray and all_snakes runners; with 0 the rollout is what it is without the argument."""
    check_random_starts(random_starts, start_lengths, env)
    if rays and local_radius is not None:
        raise ValueError("rays=True and local_radius are mutually exclusive: a run trains on rays or on windows")
    if all_snakes and not rays and local_radius is None:
        raise ValueError("all_snakes=True needs rays=True or local_radius: one set of weights can play every column only "
                         "on per-snake observations")
    if all_snakes and scripted_opponents:
        raise ValueError("all_snakes=True plays every snake with the learner's weights: scripted_opponents must be empty")
    if kill_bonus != 0.0 and not all_snakes:
        raise ValueError("kill_bonus needs all_snakes=True: only there does every snake's reward reach the learner")
    torch.manual_seed(seed); random.seed(seed)
    dev = env.device
    n_snakes = env.n_snakes
    H, W, _ = env.obs_shape
    if rays:
        make_policy = lambda: RayPolicy(amp_dtype=amp_dtype, oriented=oriented).to(dev)
    elif local_radius is None:
        make_policy = lambda: CnnPolicy((H, W, 3), amp_dtype=amp_dtype).to(dev)
    else:
        make_policy = lambda: WindowPolicy(local_radius, amp_dtype=amp_dtype, oriented=oriented).to(dev)
    model = make_policy()
    scripted = dict(scripted_opponents or {})
    if any(not 1 <= int(k) < n_snakes for k in scripted):
        raise ValueError(f"scripted_opponents: snake indices must lie in [1, {n_snakes}), got {sorted(scripted)}")
    team = ScriptedColumns(env) if scripted else None   # this run's own: nothing is left behind on the env
    opponents = [ScriptedOpponent(env, scripted[i + 1], i + 1, columns=team) if i + 1 in scripted else
                 make_policy() for i in range(0 if all_snakes else n_snakes - 1)]
    learned = [i for i in range(len(opponents)) if i + 1 not in scripted]  # opponent slots played by past selves
    if save_dir:
        os.makedirs(save_dir, exist_ok=True)
    if load_path:
        for m in [model] + [opponents[i] for i in learned]:
            load_weights(m, load_path)
    pools = [OpponentPool(max_saved_opponents, save_dir, i + 1) for i in learned]
    opt = torch.optim.Adam(model.parameters(), lr=lr(1.0), eps=1e-5)
    first_update, model_idx, next_highscore = 1, 0, 5
    state_file = os.path.join(save_dir, "trainer_state.pt") if save_dir else None
    fresh = not (resume and state_file and os.path.exists(state_file))
    if resume and fresh and save_dir and any(f.startswith("opponent") and f.endswith(".pt") for f in os.listdir(save_dir)):
        # an interrupted run left its opponent pool but no trainer state: starting over would overwrite the pool
        # from slot 0 under a model that never saw it
        raise RuntimeError(f"resume=True: {save_dir} holds opponent files but no trainer_state.pt; "
                           "pass resume=False to start over (the pool is overwritten) or restore the state file")
    if not fresh:
        ts = torch.load(state_file, map_location=dev, weights_only=True)
        check_kind(model, ts["model"], state_file)
        model.load_state_dict(ts["model"])
        opt.load_state_dict(ts["optimizer"])
        first_update, model_idx, next_highscore = ts["update"] + 1, ts["model_idx"], ts["next_highscore"]
        # pools belong to the opponent slots that past selves play; a state file written with another set of scripted
        # opponents (files from before the argument existed: every slot) cannot be continued with this one
        saved_slots = list(ts.get("learned_slots", range(len(ts["pools"]))))
        if saved_slots != learned:
            raise RuntimeError(f"resume=True: {state_file} was written with opponent pools for slots {saved_slots}, this run "
                               f"keeps pools for slots {learned} (scripted_opponents differs)")
        for pool, (idx, num) in zip(pools, ts["pools"]):
            pool.restore(dev, idx, num)

    def save_trainer_state(update):
        tmp = state_file + ".tmp"
        torch.save({"model": model.state_dict(), "optimizer": opt.state_dict(), "update": update,
                    "model_idx": model_idx, "next_highscore": next_highscore,
                    "pools": [(p.idx, p.num) for p in pools], "learned_slots": learned}, tmp)
        os.replace(tmp, state_file)

    if fresh:
        for pool in pools:
            pool.save(model)
        if save_dir:  # from the first pool file on there is a state a resume can start from
            save_trainer_state(0)
    runner = Runner(env, model, opponents, nsteps, gamma, lam, local_radius=local_radius, oriented=oriented, rays=rays,
                    all_snakes=all_snakes, kill_bonus=kill_bonus, random_starts=random_starts, start_lengths=start_lengths)
    nbatch = env.num_envs * nsteps
    nbatch_train = nbatch // nminibatches
    assert nbatch % nminibatches == 0
    nupdates = max(1, total_timesteps // nbatch)
    epinfobuf = deque(maxlen=100)
    sinks = [CSVLogger(csv_path)] if csv_path else []  # the reference's LOG_FORMAT sinks (logger.py:172-186)
    if json_path:
        sinks.append(JSONLogger(json_path))
    if tb_dir:
        sinks.append(TensorBoardLogger(tb_dir))
    mon = MonitorCSV(monitor_path, "msnake") if monitor_path else None
    history, tfirst = [], time.time()
    for update in range(first_update, nupdates + 1):
        for i, pool in zip(learned, pools):
            pool.load_random(opponents[i])
        tstart = time.time()
        frac = 1.0 - (update - 1.0) / nupdates
        lrnow, clipnow = lr(frac), cliprange(frac)
        for g in opt.param_groups:
            g["lr"] = lrnow
        obs, returns, masks, actions, values, nlps, epinfos = runner.run()
        epinfobuf.extend(epinfos)
        if mon:
            mon.write(epinfos)
        stats = []
        nsamples = obs.shape[0]  # nbatch; with all_snakes the number of valid samples of this rollout
        for _ in range(noptepochs):
            inds = torch.randperm(nsamples, device=dev)
            batches = ([b for b in torch.tensor_split(inds, nminibatches) if b.numel()] if all_snakes else
                       [inds[start:start + nbatch_train] for start in range(0, nbatch, nbatch_train)])
            for mb in batches:
                logits, vpred = model(obs[mb])
                loss, parts = ppo_loss(logits, vpred, actions[mb], returns[mb], values[mb], nlps[mb], clipnow,
                                       ent_coef, vf_coef)
                opt.zero_grad(set_to_none=True)
                loss.backward()
                if max_grad_norm is not None:
                    nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)
                opt.step()
                stats.append(torch.stack([parts[k].detach() for k in
                                          ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac")]))
        if update % opponent_save_interval == 0:
            for pool in pools:
                pool.save(model)
            if save_dir:  # the pool files and the state file move together: a restore never finds opponents newer
                save_trainer_state(update)  # than the model / optimizer / update counter it loads
        if update % log_interval == 0 or update == 1:
            lossvals = torch.stack(stats).mean(0).tolist()
            tnow = time.time()
            safemean = lambda xs: float("nan") if len(xs) == 0 else float(np.mean(xs))
            eprew = safemean([e["r"] for e in epinfobuf])
            kvs = {"serial_timesteps": update * nsteps, "nupdates": update, "total_timesteps": update * nbatch,
                   "fps": int(nbatch / (tnow - tstart)), "explained_variance": explained_variance(values, returns),
                   "eprewmean 100": eprew, "eplenmean": safemean([e["l"] for e in epinfobuf]),
                   "time_elapsed": tnow - tfirst, "ep_rew_mean": eprew}
            if pools:
                kvs["num_opponents"] = pools[0].num
            if all_snakes:
                kvs["agent_samples"], kvs["sample_fps"] = nsamples, int(nsamples / (tnow - tstart))
            if kill_bonus != 0.0:
                kvs.update(runner.last_deaths)
            kvs.update(dict(zip(("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac"), lossvals)))
            history.append(kvs)
            for sink in sinks:
                sink.writekvs(kvs)
            if log_fn:
                log_fn(" ".join(f"{k}={v:.4g}" if isinstance(v, float) else f"{k}={v}" for k, v in kvs.items()))
        if save_dir:
            if save_interval and (update % save_interval == 0 or update == 1):  # ppo_multi_agent.py:392-394
                save_weights(model, os.path.join(save_dir, f"snake_model_num{n_snakes}_{model_idx}.pt"))
                model_idx += 1
                save_trainer_state(update)
            eprew_now = float(np.mean([e["r"] for e in epinfobuf])) if epinfobuf else float("nan")
            if n_snakes == 1 and eprew_now > next_highscore:                    # ppo_multi_agent.py:397-401
                next_highscore += 1
                save_weights(model, os.path.join(save_dir, "highscore_model.pt"))
    if save_dir:
        save_weights(model, os.path.join(save_dir, f"snake_model_num{n_snakes}.pt"))  # ppo_multi_agent.py:402
        save_trainer_state(nupdates)
    for sink in sinks:
        sink.close()
    if mon:
        mon.close()
    return model, history
