"""MultiSnakeVecEnv -- the reference's VecEnv surface over the HIP batched step.

Replaces, for the snake path, what `utils.make_basic_env` builds in the reference
(src/utils.py:34-49): SubprocVecEnv([gym.make(id) + seed(seed+rank) + Monitor + WarpFrame] * n).
Same attributes and methods as baselines' VecEnv ABC (src/baselines/common/vec_env/__init__.py:22-88):
num_envs, observation_space, action_space, reset(), step_async(), step_wait(), step(), close(),
render(), unwrapped -- so `ppo_multi_agent.Runner` (src/ppo_multi_agent.py:145-216) can drive it
unchanged: env.reset() -> uint8[nenv,H,W,C]; env.step(list of per-env action tuples) ->
(obs, rews float32[nenv], dones bool[nenv], infos).

All env state and all step outputs live in HBM; `step_device()` is the zero-copy entry point for a
PyTorch-ROCm policy (device tensors in, device tensors out, asynchronous on the current stream),
`step()` is the NumPy-returning reference-compatible wrapper around it.
"""
import collections
import contextlib
import ctypes
import time

import numpy as np

from . import _capi
from .spaces import Box, Discrete

# gym ids of the reference (src/gym-snake/gym_snake/__init__.py:11-26) -> rule presets
GYM_IDS = {
    "snake-multiple-test-v0": dict(rules="snake_env", dim=19),
    "snake-new-multiple-v0": dict(rules="new_world", dim=10),
    "snake-adversarial-v0": dict(rules="adversarial", dim=10),
}


def normalize_actions(actions, num_envs, n_snakes):
    """list(zip(a0, a1[, a2])) / ndarray / scalar-per-env -> contiguous int32 [num_envs, stride].

    ppo_multi_agent.py:41-44 always sends tuples of length 2 or 3, even with one snake; surplus
    entries are ignored by the env (snake_multiple_test.py:174). A bare scalar per env is wrapped
    like snake_multiple_test.py:167-168 does.
    """
    a = np.asarray(actions)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[0] != num_envs:
        raise ValueError(f"expected {num_envs} action rows, got array of shape {a.shape}")
    if a.shape[1] < n_snakes:
        raise ValueError(f"each action row needs >= {n_snakes} entries, got {a.shape[1]}")
    return np.ascontiguousarray(a, dtype=np.int32)


def normalize_mask(mask, num_envs):
    """Env selection for a masked reset -> uint8 [num_envs] (1 = reset).

    A NumPy bool array is the mask itself (gymnasium's reset_mask, e.g. the `done` array step() returns); anything
    else is a sequence of env indices (envpool's reset(env_ids)).  Device tensors are handled by the env itself.
    """
    if isinstance(mask, np.ndarray) and mask.dtype == np.bool_:
        if mask.shape != (num_envs,):
            raise ValueError(f"a bool mask must have shape ({num_envs},), got {mask.shape}")
        return mask.astype(np.uint8)
    idx = np.asarray(mask)
    if idx.size == 0:
        idx = idx.reshape(0).astype(np.int64)
    if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"mask must be a bool array of shape ({num_envs},) or a sequence of env indices, got {mask!r}")
    if ((idx < 0) | (idx >= num_envs)).any():
        raise ValueError(f"env indices must lie in [0, {num_envs})")
    m = np.zeros(num_envs, np.uint8)
    m[idx] = 1
    return m


def normalize_copy_index(index, num_envs):
    """Source index of a device-side env copy -> contiguous int32 [num_envs] (entry e: the source env whose state
    destination env e receives; negative = leave env e as it is).

    Takes a sequence or an integer ndarray of shape [num_envs].  Entries past the int32 range become -1 / 2**31 - 1,
    i.e. stay "untouched" / "out of range"; the range check against the source is the library's.  Device tensors are
    handled by the env itself."""
    idx = np.asarray(index)
    if idx.ndim != 1 or idx.shape[0] != num_envs:
        raise ValueError(f"index must have shape ({num_envs},), got {idx.shape}")
    if not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"index must be of an integer dtype, got {idx.dtype}")
    lo, hi = idx < 0, idx > 2**31 - 1
    out = np.empty(num_envs, np.int32)
    out[lo], out[hi] = -1, 2**31 - 1
    keep = ~(lo | hi)
    out[keep] = idx[keep]
    return out


def normalize_hash_what(what):
    """"full" / "board" (or MSNAKE_HASH_FULL / MSNAKE_HASH_BOARD) -> the `what` of msnake_hash_states."""
    if isinstance(what, str) and what in _capi.HASH_WHAT:
        return _capi.HASH_WHAT[what]
    if isinstance(what, (int, np.integer)) and not isinstance(what, (bool, np.bool_)) and int(what) in _capi.HASH_WHAT.values():
        return int(what)
    raise ValueError(f"what must be one of {', '.join(map(repr, _capi.HASH_WHAT))}, got {what!r}")


def check_state_stride(stride, need_words=False):
    """The row length of a canonical-words tensor -> int: >= 0 for an export without words, >= 1 with them, >= 8 for an
    import (no state has fewer words; checked there)."""
    if isinstance(stride, (bool, np.bool_)) or not isinstance(stride, (int, np.integer)):
        raise ValueError(f"stride must be an int, got {stride!r}")
    if stride < (1 if need_words else 0) or stride > 2**31 - 1:
        raise ValueError(f"stride must lie in [{1 if need_words else 0}, 2**31 - 1], got {stride}")
    return int(stride)


_MIX_C1, _MIX_C2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
HASH_BOARD_SKIPS = (0, 1, 2, 4, 5)  # t, ctr_lo, ctr_hi, ep_len, ep_return: the words MSNAKE_HASH_BOARD leaves out


def mix64(z):
    """The splitmix64 finaliser on a NumPy uint64 array (mod 2^64)."""
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * _MIX_C1
    z = (z ^ (z >> np.uint64(27))) * _MIX_C2
    return z ^ (z >> np.uint64(31))


def state_hash(words, what="full"):
    """msnake_hash_states on the host: the 64-bit hash (a Python int in [0, 2^64)) of one env's canonical words -- a
    row of export_states_device() cut to its count, get_state_words(), a slice of a get_state_all() blob, the oracle's
    state_to_flat().  H = sum_i mix64((i + 1) << 32 | uint32(w[i])) mod 2^64; "board" leaves out words 0, 1, 2, 4, 5 and
    clears bit 8 of word 7."""
    board = normalize_hash_what(what) == _capi.HASH_WHAT["board"]
    w = np.asarray(words)
    if w.ndim != 1 or w.shape[0] < 8 or not np.issubdtype(w.dtype, np.integer):
        raise ValueError(f"words must be a 1-d integer array of at least 8 canonical words, got {w.dtype} {w.shape}")
    w = (w.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    keep = np.ones(len(w), bool)
    if board:
        keep[list(HASH_BOARD_SKIPS)] = False
        w[7] &= np.uint64(0xFFFFFFFF & ~0x100)
    terms = mix64((np.arange(1, len(w) + 1, dtype=np.uint64) << np.uint64(32)) | w)
    return int(np.add.reduce(terms[keep], dtype=np.uint64))


def normalize_views(views, n_views):
    """Selection of observation views for render_cells_device -> (view_mask, list of the selected views).

    None = every view; an int = that view alone; otherwise a sequence of strictly ascending view indices (the planes
    come out in ascending view order, so any other order would mislabel them); the empty sequence selects no plane."""
    if views is None:
        sel = list(range(n_views))
    elif isinstance(views, (int, np.integer)) and not isinstance(views, (bool, np.bool_)):
        sel = [int(views)]
    else:
        sel = list(views)
        for v in sel:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"views must be None, an int or a sequence of ints, got {views!r}")
        sel = [int(v) for v in sel]
    for v in sel:
        if not 0 <= v < n_views:
            raise ValueError(f"view indices must lie in [0, {n_views}), got {v}")
    if any(b <= a for a, b in zip(sel, sel[1:])):
        raise ValueError(f"views must be strictly ascending (the planes are written in ascending view order), got {sel}")
    return sum(1 << v for v in sel), sel


LOCAL_MAX_RADIUS = 31  # MSNAKE_LOCAL_MAX_RADIUS
CELL_OUTSIDE = 6       # MSNAKE_CELL_OUTSIDE: a window entry of render_local_device() that lies outside the grid
RAY_DIRS, RAY_CHANNELS = 8, 4                          # MSNAKE_RAY_DIRS, MSNAKE_RAY_CHANNELS: render_rays_device()
RAY_WALL, RAY_FRUIT, RAY_OWN, RAY_OTHER = 0, 1, 2, 3   # MSNAKE_RAY_*: the channels
# head_fields_device(): a distance no front reaches (MSNAKE_HEAD_NONE), a cell two snakes reach at once and a cell nobody
# owns (MSNAKE_OWNER_TIE, MSNAKE_OWNER_NONE)
HEAD_NONE, OWNER_TIE, OWNER_NONE = _capi.HEAD_NONE, _capi.OWNER_TIE, _capi.OWNER_NONE


def normalize_snakes(snakes, n_snakes):
    """Selection of snakes for render_local_device -> (snake_mask, list of the selected snakes).

    None = every snake; an int = that snake alone; otherwise a non-empty sequence of strictly ascending snake indices (the
    windows come out in ascending snake order, so any other order would mislabel them)."""
    try:
        mask, sel = normalize_views(snakes, n_snakes)
    except TypeError:
        raise ValueError(f"snakes must be None, an int or a sequence of ints, got {snakes!r}") from None
    except ValueError as err:
        raise ValueError(str(err).replace("views", "snakes").replace("view indices", "snake indices")
                         .replace("the planes", "the windows").replace("view order", "snake order")) from None
    if not sel:
        raise ValueError("snakes selects no snake: there is no window to write")
    return mask, sel


def check_radius(radius):
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 1 <= radius <= LOCAL_MAX_RADIUS:
        raise ValueError(f"radius must be an int in [1, {LOCAL_MAX_RADIUS}], got {radius!r}")
    return int(radius)


def relative_to_absolute(rel, heading):
    """Relative actions of a heading-aligned window policy -> the absolute actions the step takes (include/msnake.h,
    msnake_render_local): relative action r in 1..4 = forward, the +j side of the window, backward, the -j side, is the
    absolute action ((r - 1 + k) mod 4) + 1 under heading k; 0 stays 0.  `rel` and `heading` are integer tensors of one
    shape, [num_envs] or [num_envs, S] (the heading as render_local_device returns it); the result has rel's dtype and
    stays on its device."""
    import torch
    if not isinstance(rel, torch.Tensor) or not isinstance(heading, torch.Tensor):
        raise ValueError("rel and heading must be torch tensors")
    if rel.is_floating_point() or heading.is_floating_point() or rel.dtype == torch.bool or heading.dtype == torch.bool:
        raise ValueError(f"rel and heading must be integer tensors, got {rel.dtype} and {heading.dtype}")
    if rel.shape != heading.shape or rel.dim() not in (1, 2):
        raise ValueError(f"rel and heading must have one shape, [num_envs] or [num_envs, S], got {tuple(rel.shape)} and "
                         f"{tuple(heading.shape)}")
    k = heading.to(device=rel.device, dtype=rel.dtype)
    return torch.where(rel > 0, (rel - 1 + k) % 4 + 1, torch.zeros_like(rel))


# the scripted policies that are an entry point of their own with uint16 outputs behind safe_dev:
# name -> (the env's bound C function, its name, the keywords of those outputs in the order of the C arguments)
COUNT_POLICIES = {_capi.SPACE_POLICY: ("_space_fn", "msnake_space_actions", ("space_out",)),
                  _capi.TERRITORY_POLICY: ("_territory_fn", "msnake_territory_actions", ("territory_out",)),
                  _capi.PATH_POLICY: ("_path_fn", "msnake_path_actions", ("path_out", "field_out")),
                  _capi.TIMED_POLICY: ("_timed_fn", "msnake_timed_actions", ("reach_out", "life_out"))}
# output keyword -> the policy that writes it; every one is [num_envs, n_snakes, 4] but the field and the lifetimes,
# [num_envs, dim, dim]
COUNT_OUTPUTS = {kw: name for name, (_, _, kws) in COUNT_POLICIES.items() for kw in kws}

# constructor arguments that may differ between the two handles of a device-side copy (include/msnake.h,
# msnake_copy_envs): what MultiSnakeVecEnv.clone() lets a caller override
CLONE_OVERRIDES = ("record_policy", "envs_per_block", "obs_scale", "auto_reset", "max_steps", "seed", "env_id_base")


# what agent_outcomes_device() / step_agents_device() return of msnake_agent_outcomes: device tensors, None = not written
AgentOutcomes = collections.namedtuple("AgentOutcomes", ("rew", "ate", "flags", "info"))
# what death_causes_device() / step_agents_device(causes=True) return of msnake_death_causes, likewise
DeathCauses = collections.namedtuple("DeathCauses", ("cause", "by", "victims", "where"))
# what move_fates_device() returns of msnake_fate_actions, likewise: fate, by and eat are uint8 [num_envs, n_snakes, 5],
# mask is uint8 [num_envs, n_snakes, 2]
MoveFates = collections.namedtuple("MoveFates", ("fate", "by", "eat", "mask"))
# what playout_device() returns: device tensors, None for what was not written
Playout = collections.namedtuple("Playout", ("steps", "end", "ret", "info", "words", "count"))


class LazyInfos:
    """Sequence of per-env info dicts, materialised on access.

    Same keys as the reference: {"ale.lives": 1, "num_snakes": k} (snake_multiple_test.py:197) plus
    Monitor's info['episode'] = {'r','l','t'} on the step an episode ends (monitor.py:61-78).
    Building 4096 dicts per step would dominate the step time, so they are built on demand;
    `episodes()` is the fast path for the `info.get('episode')` scan at ppo_multi_agent.py:187-190.
    With `terminal` = (final_obs rows of the done envs in env order, truncated flags of every env) -- a
    terminal_obs=True env -- done envs also get Stable-Baselines3's "terminal_observation" and
    "TimeLimit.truncated".
    """

    def __init__(self, done, num_snakes, ep_return, ep_len, t_elapsed, terminal=None):
        self._done, self._ns, self._r, self._l, self._t = done, num_snakes, ep_return, ep_len, t_elapsed
        self._terminal = terminal
        if terminal is not None:
            self._row = np.cumsum(done) - 1  # env i's row among the done envs' terminal observations

    def __len__(self):
        return len(self._done)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if not 0 <= i < len(self):
            raise IndexError(i)
        info = {"ale.lives": 1, "num_snakes": int(self._ns[i])}
        if self._done[i]:
            info["episode"] = {"r": round(float(self._r[i]), 6), "l": int(self._l[i]), "t": self._t}
            if self._terminal is not None:
                info["terminal_observation"] = self._terminal[0][self._row[i]]
                info["TimeLimit.truncated"] = bool(self._terminal[1][i])
        return info

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def episodes(self):
        idx = np.nonzero(self._done)[0]
        return [{"r": round(float(self._r[i]), 6), "l": int(self._l[i]), "t": self._t} for i in idx]


class MultiSnakeVecEnv:
    """num_envs independent multi-snake games stepped in lockstep by one HIP kernel launch."""

    metadata = {"render.modes": ["rgb_array", "cells"]}

    def __init__(self, num_envs, dim=19, n_snakes=3, n_fruits=None, rules="snake_env", seed=0,
                 env_id_base=0, device=None, max_steps=2000, auto_reset=True, obs_scale=1,
                 declared_channels=6, host_views=False, envs_per_block=0, record_policy="auto",
                 obs_store_policy="auto", tape_store_policy="auto", terminal_obs=False):
        """terminal_obs=True (needs auto_reset=True): the handle runs without the in-kernel auto reset and every
        step_device() follows the step with msnake_reset_envs(done) on the same stream -- the same results, plus the
        terminal observation of every episode (`final_obs`, valid where done) and whether the time cap ended it
        (`truncated`).  One or two more launches per step; rollout_device() is not available then."""
        import torch  # device memory and streams only

        if not torch.cuda.is_available():
            raise RuntimeError("MultiSnakeVecEnv needs an MI355X (torch.cuda.is_available() is False); "
                               "there is no CPU path")
        self._torch = torch
        self._L = _capi.load()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device must be a cuda (HIP) device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        rules_id = _capi.RULES[rules] if isinstance(rules, str) else int(rules)
        self.terminal_obs = bool(terminal_obs)
        if self.terminal_obs and not auto_reset:
            raise ValueError("terminal_obs=True needs auto_reset=True (it replaces the in-kernel auto reset)")
        if n_fruits is None:
            n_fruits = n_snakes
        # what clone() needs to build the same env again
        self._ctor = dict(dim=dim, n_snakes=n_snakes, n_fruits=n_fruits, rules=rules, seed=seed, env_id_base=env_id_base,
                          device=self.device, max_steps=max_steps, auto_reset=auto_reset, obs_scale=obs_scale,
                          declared_channels=declared_channels, host_views=host_views, envs_per_block=envs_per_block,
                          record_policy=record_policy, obs_store_policy=obs_store_policy,
                          tape_store_policy=tape_store_policy, terminal_obs=terminal_obs)
        self.cfg = _capi.MsnakeConfig(ctypes.sizeof(_capi.MsnakeConfig), self.device.index or 0, int(num_envs),
                                      int(dim), int(n_snakes), int(n_fruits), rules_id, int(max_steps),
                                      int(bool(auto_reset) and not self.terminal_obs), int(obs_scale), int(seed),
                                      int(env_id_base),
                                      # launch tuning (msnake_config, ABI 3): how the work is laid out, never a result
                                      int(envs_per_block), _capi.RECORD_POLICY[record_policy],
                                      _capi.STORE_POLICY[obs_store_policy], _capi.STORE_POLICY[tape_store_policy])
        self._h = ctypes.c_void_p()
        _capi.apply_kernel_switch()  # (MSNAKE_GENERIC_KERNELS, read when the handle is created)
        _capi.check(self._L.msnake_create(ctypes.byref(self.cfg), ctypes.byref(self._h)), "msnake_create")
        H, W, C = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _capi.check(self._L.msnake_obs_shape(self._h, ctypes.byref(H), ctypes.byref(W), ctypes.byref(C)))
        self.num_envs = int(num_envs)
        self.n_snakes = int(n_snakes)
        self.rules = _capi.RULE_NAMES[rules_id]
        self.obs_shape = (H.value, W.value, C.value)
        # WarpFrame declares 6 channels whatever the env emits (utils.py:25) and get_shape halves
        # that (utils.py:51-55): keep the declaration so ppo_multi_agent builds 3-channel policies.
        self.observation_space = Box(0, 255, (H.value, W.value, declared_channels or C.value), np.uint8)
        self.action_space = Discrete(5)
        with torch.cuda.device(self.device):
            self._obs = torch.empty((self.num_envs,) + self.obs_shape, dtype=torch.uint8, device=self.device)
            self._rew = torch.zeros(self.num_envs, dtype=torch.float32, device=self.device)
            self._done = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            self._info = torch.zeros((self.num_envs, 4), dtype=torch.int32, device=self.device)
            # terminal_obs=True: overwritten by every step (final_obs rows are valid where done)
            self.final_obs = self.truncated = None
            if self.terminal_obs:
                self.final_obs = torch.zeros((self.num_envs,) + self.obs_shape, dtype=torch.uint8, device=self.device)
                self.truncated = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        # NumPy-returning calls copy device -> host.  Default: fresh arrays every call, like the
        # reference's np.stack (pageable copy, ~10 GB/s).  host_views=True returns views of pinned
        # staging buffers instead (~5x faster, but OVERWRITTEN by the next call: copy what you keep,
        # as ppo_multi_agent.py:165-168 does anyway).
        self._host_views = bool(host_views)
        self._pinned = None
        if self._host_views:
            pin = lambda t: torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            self._pinned = (pin(self._obs), pin(self._rew), pin(self._done), pin(self._info))
        self._pending = None
        self._tstart = time.time()
        self.closed = False
        # hot-path constants of step_device(): the handle's own output buffers never move
        self._p_obs, self._p_rew = self._obs.data_ptr(), self._rew.data_ptr()
        self._p_done, self._p_info = self._done.data_ptr(), self._info.data_ptr()
        self._step_fn = self._L.msnake_step
        self._reset_envs_fn = self._L.msnake_reset_envs
        if self.terminal_obs:
            self._p_final, self._p_trunc = self.final_obs.data_ptr(), self.truncated.data_ptr()
        self._cur_stream = torch.cuda.current_stream
        self._scripted_fn = self._L.msnake_scripted_actions
        self._scripted_out = None  # scripted_actions_device(out=None): allocated on first use
        self._space_fn = self._L.msnake_space_actions
        self._territory_fn = self._L.msnake_territory_actions
        self._path_fn = self._L.msnake_path_actions
        self._timed_fn = self._L.msnake_timed_actions
        self._cells_fn = self._L.msnake_render_cells
        self._local_fn = self._L.msnake_render_local
        self._rays_fn = self._L.msnake_render_rays
        self._agents_fn = self._L.msnake_agent_outcomes
        self._heads_fn = self._L.msnake_head_fields
        # msnake_agent_outcomes: the tracker and the env's own outputs, allocated on first use; stale = the tracker no
        # longer describes the state (a full reset, an installed or copied state, a tape): the next call arms it first
        self._track = self._agents_own = None
        self._track_stale = True
        # msnake_death_causes: the env's own outputs and the snapshot env of step_agents_device(causes=True), on first use
        self._causes_fn = self._L.msnake_death_causes
        self._causes_own = self._snapshot = None
        self._fates_fn = self._L.msnake_fate_actions
        self._scatter_own = None  # scatter_device(): words, count, got and status, allocated on first use

    # ------------------------------------------------------------------ device-side API
    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _checked(self, t, name, dtype, want):
        """The kernels write through raw pointers: a caller-supplied tensor must be exactly `dtype` and shape `want`,
        contiguous, on this device.  Returns it."""
        if (not isinstance(t, self._torch.Tensor) or t.dtype != dtype or t.device != self.device or
                tuple(t.shape) != want or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {want} on {self.device}")
        return t

    def _out(self, out):
        return self._obs if out is None else self._checked(out, "out", self._torch.uint8, (self.num_envs,) + self.obs_shape)

    def _mask(self, mask):
        """mask -> contiguous uint8 [num_envs] tensor on this device (a tensor that already is one is used as it is)."""
        torch = self._torch
        if isinstance(mask, torch.Tensor):
            if mask.dtype not in (torch.bool, torch.uint8) or tuple(mask.shape) != (self.num_envs,):
                raise ValueError(f"a mask tensor must be bool or uint8 of shape ({self.num_envs},), got {mask.dtype} "
                                 f"{tuple(mask.shape)}")
            if mask.dtype == torch.uint8 and mask.device == self.device and mask.is_contiguous():
                return mask
            return mask.to(device=self.device, dtype=torch.uint8).contiguous()
        return torch.from_numpy(normalize_mask(mask, self.num_envs)).to(self.device)

    def reset_device(self, mask=None, out=None, final_out=None, truncated_out=None):
        """mask=None: reset every env.  Otherwise reset only the envs `mask` selects (a bool / uint8 tensor or NumPy
        bool array of shape [num_envs], or a sequence of env indices): their reset observations go to `out`, their
        pre-reset observations to `final_out` (if given), the truncation flag of every env to `truncated_out` (if
        given); rows of unselected envs are left untouched.  Returns `out`; nothing is synchronised."""
        obs = self._out(out)
        if mask is None:
            if final_out is not None or truncated_out is not None:
                raise ValueError("final_out / truncated_out need a mask (a full reset has no terminal observations)")
            _capi.check(self._L.msnake_reset(self._h, obs.data_ptr(), self._stream()), "msnake_reset")
            self._track_stale = True
            return obs
        m = self._mask(mask)
        p_final = self._out(final_out).data_ptr() if final_out is not None else None
        p_trunc = None
        if truncated_out is not None:
            p_trunc = self._checked(truncated_out, "truncated_out", self._torch.uint8, (self.num_envs,)).data_ptr()
        _capi.check(self._reset_envs_fn(self._h, m.data_ptr(), obs.data_ptr(), p_final, p_trunc, self._stream()),
                    "msnake_reset_envs")
        return obs

    def step_device(self, actions, out=None):
        """actions: int32 cuda tensor [num_envs, >= n_snakes]. Returns device tensors
        (obs uint8[nenv,H,W,C], rew f32[nenv], done u8[nenv], info i32[nenv,4] = (ep_return bits,
        ep_len, num_snakes, done)); nothing is synchronised."""
        torch = self._torch
        if actions.dtype != torch.int32 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int32).contiguous()
        shape = actions.shape
        if len(shape) != 2 or shape[0] != self.num_envs or shape[1] < self.n_snakes:
            raise ValueError(f"actions must be [{self.num_envs}, >={self.n_snakes}], got {tuple(actions.shape)}")
        if out is None:
            obs, p_obs = self._obs, self._p_obs
        else:
            obs = self._out(out)
            p_obs = obs.data_ptr()
        rc = self._step_fn(self._h, actions.data_ptr(), shape[1], p_obs, self._p_rew, self._p_done, self._p_info,
                           self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_step")
        if self.terminal_obs:  # the auto reset, as a masked reset that keeps the terminal observations
            rc = self._reset_envs_fn(self._h, self._p_done, p_obs, self._p_final, self._p_trunc,
                                     self._cur_stream(self.device).cuda_stream)
            if rc < 0:
                _capi.check(rc, "msnake_reset_envs")
        return obs, self._rew, self._done, self._info

    def _count_shape(self, kw):
        if kw in ("field_out", "life_out"):
            return (self.num_envs, int(self.cfg.dim), int(self.cfg.dim))
        return (self.num_envs, self.n_snakes, 4)

    def scripted_actions_device(self, policy, snakes=None, out=None, safe_out=None, space_out=None, territory_out=None,
                                path_out=None, field_out=None, reach_out=None, life_out=None, fates_out=None):
        """Actions of a scripted policy ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy", "path_greedy", "timed_greedy", or None for the mask alone) for the
        snakes in `snakes` (indices; default every snake), computed on the device from the env's current state.  They go to
        columns `snakes` of `out`, an int32 [num_envs, >= n_snakes] device tensor as step_device() takes it; its other
        columns are left as they are (out=None: a cached, zero-initialised [num_envs, n_snakes] tensor of the env).
        `safe_out`, a uint8 [num_envs, n_snakes] device tensor, gets every snake's safe-move mask (bit a = move a leads
        to an on-board cell that no body occupies).  Returns `out`, or (out, safe_out) when a mask was asked for;
        nothing is synchronised.  Draws no random numbers and changes no env state.
        "space_greedy" (msnake_space_actions) flood-fills from every open move's target and refuses moves into a region
        smaller than the body; only with it, `space_out`, a uint16 [num_envs, n_snakes, 4] device tensor, gets the
        reachable-space counts (see reachable_space_device) and is returned behind the others that were asked for.
        "territory_greedy" (msnake_territory_actions) is space_greedy with the Voronoi territory in place of the space:
        the cells the snake reaches strictly before any other snake can; only with it, `territory_out`, a uint16
        [num_envs, n_snakes, 4] device tensor, gets those counts (see territory_device), returned like space_out.
        "path_greedy" (msnake_path_actions) chooses among space_greedy's eligible moves by the shortest path to a fruit
        around the bodies instead of the L1 distance, and plays space_greedy's move when no fruit can be reached; only
        with it, `path_out`, a uint16 [num_envs, n_snakes, 4] device tensor, gets the path lengths (see path_device)
        and `field_out`, a uint16 [num_envs, dim, dim] device tensor, the whole distance field (see
        fruit_field_device).  The return order is actions, safe, path, field for those asked for.
        "timed_greedy" (msnake_timed_actions) is space_greedy with the timed reach in place of the space: a flood fill
        that may enter a body cell once the piece lying there has moved on; only with it, `reach_out`, a uint16
        [num_envs, n_snakes, 4] device tensor, gets those counts (see timed_reach_device) and `life_out`, a uint16
        [num_envs, dim, dim] device tensor, the lifetime of every cell (see cell_lifetimes_device).  The return order
        is actions, safe, reach, life for those asked for.
        "wary_greedy" (msnake_fate_actions; snake_env and adversarial) plays by the fate of its moves: among the moves
        that are survived whatever the others do -- if there is none, among those that can be survived -- the one closest
        to a fruit; a move onto a tail that goes is open to it, a cell another head can enter is not.  It writes no
        safe-move mask (safe_out is refused); only with it, `fates_out`, a MoveFates of tensors (or None) as
        move_fates_device() takes them, is written in the same call.  Returns `out`, or (out, fates_out)."""
        torch = self._torch
        given = {"space_out": space_out, "territory_out": territory_out, "path_out": path_out, "field_out": field_out,
                 "reach_out": reach_out, "life_out": life_out}
        for kw, t in given.items():
            if t is not None and policy != COUNT_OUTPUTS[kw]:
                raise ValueError(f"{kw} is written by policy {COUNT_OUTPUTS[kw]!r} only, got policy {policy!r}")
        if fates_out is not None and policy != _capi.WARY_POLICY:
            raise ValueError(f"fates_out is written by policy {_capi.WARY_POLICY!r} only, got policy {policy!r}")
        if policy == _capi.WARY_POLICY and safe_out is not None:
            raise ValueError(f"policy {_capi.WARY_POLICY!r} writes no safe-move mask: ask fate_masks_device() or pass fates_out")
        count = COUNT_POLICIES.get(policy)
        if count is None and policy != _capi.WARY_POLICY and policy not in _capi.SCRIPTED_POLICY:
            raise ValueError(f"policy must be 'safe_greedy', 'hamiltonian' or None, got {policy!r}")
        if snakes is None:
            bits = (1 << self.n_snakes) - 1
        else:
            bits = 0
            for s in snakes:
                if int(s) != s or not 0 <= int(s) < self.n_snakes:
                    raise ValueError(f"snake indices must lie in [0, {self.n_snakes}), got {s!r}")
                bits |= 1 << int(s)
        if out is None:
            if self._scripted_out is None:
                with torch.cuda.device(self.device):
                    self._scripted_out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32, device=self.device)
            out = self._scripted_out
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != self.device or out.dim() != 2 or
              out.shape[0] != self.num_envs or out.shape[1] < self.n_snakes or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int32 tensor of shape ({self.num_envs}, >= {self.n_snakes}) on {self.device}")
        p_safe = None
        if safe_out is not None:
            p_safe = self._checked(safe_out, "safe_out", torch.uint8, (self.num_envs, self.n_snakes)).data_ptr()
        if policy == _capi.WARY_POLICY:
            fates = None if fates_out is None else self._fates_checked(fates_out)
            rc = self._fates_fn(self._h, bits, out.data_ptr(), int(out.shape[1]),
                                *([None] * 4 if fates is None else [None if t is None else t.data_ptr() for t in fates]),
                                self._cur_stream(self.device).cuda_stream)
            if rc < 0:
                _capi.check(rc, "msnake_fate_actions")
            return out if fates is None else (out, fates)
        if count is not None:
            fn, c_name, kws = count
            p_counts = [None if given[kw] is None else
                        self._checked(given[kw], kw, torch.uint16, self._count_shape(kw)).data_ptr() for kw in kws]
            rc = getattr(self, fn)(self._h, bits, out.data_ptr(), int(out.shape[1]), p_safe, *p_counts,
                                   self._cur_stream(self.device).cuda_stream)
            if rc < 0:
                _capi.check(rc, c_name)
            res = (out,) + tuple(t for t in [safe_out] + [given[kw] for kw in kws] if t is not None)
            return res[0] if len(res) == 1 else res
        rc = self._scripted_fn(self._h, _capi.SCRIPTED_POLICY[policy], bits, out.data_ptr(), int(out.shape[1]), p_safe,
                               self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_scripted_actions")
        return out if safe_out is None else (out, safe_out)

    def safe_moves_device(self, out=None):
        """uint8 [num_envs, n_snakes]: bit a (1..4) is set iff move a of that snake leads to an on-board cell that no
        body occupies (the action mask of masked PPO); 0 for an empty body.  Nothing is synchronised."""
        if out is None:
            with self._torch.cuda.device(self.device):
                out = self._torch.empty((self.num_envs, self.n_snakes), dtype=self._torch.uint8, device=self.device)
        self._checked(out, "safe_out", self._torch.uint8, (self.num_envs, self.n_snakes))
        rc = self._scripted_fn(self._h, 0, 0, None, 0, out.data_ptr(), self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_scripted_actions")
        return out

    def _counts_device(self, kw, out):
        """One uint16 output of a COUNT_POLICIES entry point alone: no action, no mask and no other output is written."""
        fn, c_name, kws = COUNT_POLICIES[COUNT_OUTPUTS[kw]]
        if out is None:
            with self._torch.cuda.device(self.device):
                out = self._torch.empty(self._count_shape(kw), dtype=self._torch.uint16, device=self.device)
        self._checked(out, kw, self._torch.uint16, self._count_shape(kw))
        rc = getattr(self, fn)(self._h, 0, None, 0, None, *[out.data_ptr() if k == kw else None for k in kws],
                               self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, c_name)
        return out

    def reachable_space_device(self, out=None):
        """uint16 [num_envs, n_snakes, 4]: entry m of a snake is the number of free cells 4-connected to the target of
        its move m + 1 through free cells, the target included; 0 when that move is not open (off the board or into a
        body) or the body is empty.  One flood fill per distinct region, on the device; nothing is synchronised."""
        return self._counts_device("space_out", out)

    def territory_device(self, out=None):
        """uint16 [num_envs, n_snakes, 4]: entry m of a snake is its Voronoi territory behind move m + 1: the number of
        free cells it reaches from that move's target in strictly fewer steps than any other snake needs from the targets
        of its own open moves (bodies static, ties to the others); 0 when the move is not open, the body is empty, or
        another snake can enter the same target.  Equals reachable_space_device() when no other snake can move.  On the
        device; nothing is synchronised."""
        return self._counts_device("territory_out", out)

    def path_device(self, out=None):
        """uint16 [num_envs, n_snakes, 4]: entry m of a snake is the length of the shortest 4-connected path through free
        cells from the target of its move m + 1 to a fruit that no body covers (0: the move eats); 0xFFFF
        (msnake_path_actions: MSNAKE_PATH_NONE) when the move is not open, the body is empty or no such fruit can be
        reached.  1 + the minimum over m is the snake's distance to food, the potential of reward shaping.  One BFS per
        env on the device; nothing is synchronised."""
        return self._counts_device("path_out", out)

    def fruit_field_device(self, out=None):
        """uint16 [num_envs, dim, dim]: entry [c0, c1] is the length of the shortest 4-connected path through free cells
        from cell (c0, c1) to a fruit that no body covers, the indexing of render_cells_device(); 0xFFFF for a cell
        under a body and for a free cell from which no such fruit can be reached.  On the device; nothing is
        synchronised."""
        return self._counts_device("field_out", out)

    def timed_reach_device(self, out=None):
        """uint16 [num_envs, n_snakes, 4]: entry m of a snake is its timed reach behind move m + 1: the number of cells a
        level-by-level flood fill from that move's target takes when level t may also enter a body cell whose lifetime
        (cell_lifetimes_device) is below t; 0 when the move is not open or the body is empty.  Never below
        reachable_space_device(), and equal to it where no body ever recedes.  On the device; nothing is synchronised."""
        return self._counts_device("reach_out", out)

    def cell_lifetimes_device(self, out=None):
        """uint16 [num_envs, dim, dim]: entry [c0, c1] is the lifetime of cell (c0, c1), the indexing of
        render_cells_device(): after how many steps the last body piece lying there will have moved on if every snake
        keeps moving and nobody eats or dies: (len - i) + max(0, grow_to - len) for piece i, capped at 0xFFFE, the
        maximum over stacked pieces; 0 for a cell under no body; 0xFFFF (msnake_timed_actions: MSNAKE_LIFE_NEVER) for
        every body cell of a new_world handle without fruits.  On the device; nothing is synchronised."""
        return self._counts_device("life_out", out)

    def _fates_checked(self, out):
        """A MoveFates (or any four-entry sequence) of caller-supplied tensors, None for what is not written."""
        if len(out) != 4:
            raise ValueError(f"a MoveFates has four entries (fate, by, eat, mask), got {len(out)}")
        n, ns, u8 = self.num_envs, self.n_snakes, self._torch.uint8
        return MoveFates(*[None if t is None else self._checked(t, f"{name}_out", u8, (n, ns, 2 if name == "mask" else 5))
                           for name, t in zip(MoveFates._fields, out)])

    def move_fates_device(self, fate=True, by=False, eat=False, mask=True, out=None):
        """What each of a snake's five actions leads to in the next step (msnake_fate_actions; snake_env and
        adversarial), as a MoveFates of uint8 device tensors, None for what was not asked for:
        fate [num_envs, n_snakes, 5]: entry [s, a] holds the FATE_* bits (_capi) of snake s playing action a: FATE_WALL,
        FATE_SELF, FATE_BODY (together FATE_CERTAIN: the snake dies whatever the others do), FATE_HEAD_ON, FATE_TAIL
        (together FATE_RISK: another head can enter the cell / another snake's last piece lies there and goes only if
        that snake moves and does not eat) and FATE_EATS;
        by [num_envs, n_snakes, 5]: bit k: HEAD_ON holds against snake k, bit 4 + k: TAIL holds against snake k;
        eat [num_envs, n_snakes, 5]: how many fruits the move eats (at most 255);
        mask [num_envs, n_snakes, 2]: [.., 0] has bit a set iff action a can be survived (no CERTAIN bit), [.., 1] iff it is
        survived whatever the others do (no CERTAIN and no RISK bit): the action masks of masked PPO.
        An empty body gives 0 everywhere.  `out`: a MoveFates of tensors to write into (None entries are not written;
        the flags are ignored); without it the flags choose, and the tensors are fresh.  One launch; nothing is
        synchronised, no random numbers are drawn and no env state changes."""
        torch = self._torch
        if out is None:
            n, ns = self.num_envs, self.n_snakes
            with torch.cuda.device(self.device):
                out = MoveFates(*[torch.empty((n, ns, 2 if name == "mask" else 5), dtype=torch.uint8, device=self.device) if want else None
                                  for name, want in zip(MoveFates._fields, (fate, by, eat, mask))])
        res = self._fates_checked(out)
        if all(t is None for t in res):
            raise ValueError("move_fates_device: nothing to write (fate, by, eat and mask are all off)")
        rc = self._fates_fn(self._h, 0, None, 0, *[None if t is None else t.data_ptr() for t in res],
                            self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_fate_actions")
        return res

    def fate_masks_device(self, out=None):
        """uint8 [num_envs, n_snakes, 2]: the two action masks of move_fates_device() alone: bit a (0..4) of [.., 0] is set
        iff action a can be survived, of [.., 1] iff it is survived whatever the other snakes do.  Unlike
        safe_moves_device() a move onto a tail that goes is open and a cell another head can enter is not.  Nothing is
        synchronised."""
        if out is None:
            return self.move_fates_device(fate=False, mask=True).mask
        return self.move_fates_device(out=MoveFates(None, None, None, out)).mask

    def head_fields_shape(self, snakes=None):
        """(P, dim, dim): one env's distance planes of head_fields_device(snakes)."""
        return (len(normalize_snakes(snakes, self.n_snakes)[1]), int(self.cfg.dim), int(self.cfg.dim))

    def head_fields_device(self, snakes=None, dist_out=None, owner_out=None, counts_out=None, dist=True, owner=True, counts=True):
        """Where the snakes stand relative to every cell (msnake_head_fields), in three outputs:
        the distance planes, uint16 [num_envs, P, dim, dim], one per selected snake in ascending snake order: entry
        [c0, c1] of snake s is 1 + the shortest 4-connected path through free cells from the target of one of its open
        moves to cell (c0, c1), the indexing of render_cells_device(); 0 on the snake's own head; HEAD_NONE (0xFFFF) for a
        cell under a body, a cell the snake cannot reach, and everywhere for an empty body or a snake without an open move;
        the owner map, uint8 [num_envs, dim, dim]: the index of the one snake with the smallest distance to the cell,
        OWNER_TIE (0xFE) where two or more share it, OWNER_NONE (0xFF) where no snake reaches and on every body cell;
        always over all snakes;
        the counts, uint16 [num_envs, n_snakes]: how many cells each snake owns.
        `snakes` selects the planes: None = every snake, an int, or a strictly ascending sequence.  An output is written
        when its tensor is given (`dist_out`, `owner_out`, `counts_out`: contiguous, of the shape and dtype above, on this
        device) or, without one, when its flag `dist` / `owner` / `counts` is true: then into a fresh tensor.  Returns the
        tensors it wrote, in that order (one tensor alone when only one was written); nothing is synchronised.  Draws no
        random numbers and changes no env state."""
        torch = self._torch
        mask, sel = normalize_snakes(snakes, self.n_snakes)
        dim = int(self.cfg.dim)
        wants = (("dist_out", dist_out, dist, torch.uint16, (self.num_envs, len(sel), dim, dim)),
                 ("owner_out", owner_out, owner, torch.uint8, (self.num_envs, dim, dim)),
                 ("counts_out", counts_out, counts, torch.uint16, (self.num_envs, self.n_snakes)))
        outs = []
        for name, t, flag, dtype, want in wants:
            if t is not None:
                self._checked(t, name, dtype, want)
            elif flag:
                with torch.cuda.device(self.device):
                    t = torch.empty(want, dtype=dtype, device=self.device)
            outs.append(t)
        if all(t is None for t in outs):
            raise ValueError("nothing to write: dist, owner and counts are all false and no output tensor is given")
        rc = self._heads_fn(self._h, mask if outs[0] is not None else 0, *[None if t is None else t.data_ptr() for t in outs],
                            self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_head_fields")
        res = tuple(t for t in outs if t is not None)
        return res[0] if len(res) == 1 else res

    def head_distances_device(self, snakes=None, out=None):
        """uint16 [num_envs, P, dim, dim]: the distance planes of head_fields_device() alone."""
        return self.head_fields_device(snakes, dist_out=out, owner=False, counts=False)

    def owner_map_device(self, out=None):
        """uint8 [num_envs, dim, dim]: the owner map of head_fields_device() alone."""
        return self.head_fields_device(owner_out=out, dist=False, counts=False)

    def owned_counts_device(self, out=None):
        """uint16 [num_envs, n_snakes]: the counts of head_fields_device() alone."""
        return self.head_fields_device(counts_out=out, dist=False, owner=False)

    @property
    def cells_shape(self):
        """(views, dim, dim): one env's planes of render_cells_device() with every view selected."""
        return (self.obs_shape[2] // 3, int(self.cfg.dim), int(self.cfg.dim))

    def render_cells_device(self, views=None, out=None, snakes_out=None, snakes=False):
        """The observation as cell codes (msnake_render_cells): uint8 [num_envs, V, dim, dim], one plane per selected view
        in ascending view order, entry [c0, c1] = what frame pixel [c0 + 1, c1 + 1] of that view shows: 0 empty, 1 fruit,
        2 / 3 body / head of the view's own snake, 4 / 5 body / head of another snake.  `views`: None = every view of
        the frame (cells_shape[0]), an int, or a strictly ascending sequence; the empty sequence writes no plane.
        `snakes_out`, an int32 [num_envs, n_snakes, 8] device tensor (snakes=True: a fresh one), gets every snake's
        (len, head c0, head c1, v0, v1, grow_to, alive, in_dead).  `out` must be a contiguous uint8 tensor of the shape
        above on this device; it needs no alignment.  Returns the planes, (planes, table) when the table was asked for,
        or the table alone when no view is selected; nothing is synchronised.  Draws no random numbers and changes no
        env state."""
        torch = self._torch
        n_views, dim = self.cells_shape[0], self.cells_shape[1]
        mask, sel = normalize_views(views, n_views)
        if snakes_out is None and snakes:
            with torch.cuda.device(self.device):
                snakes_out = torch.empty((self.num_envs, self.n_snakes, 8), dtype=torch.int32, device=self.device)
        elif snakes_out is not None:
            self._checked(snakes_out, "snakes_out", torch.int32, (self.num_envs, self.n_snakes, 8))
        want = (self.num_envs, len(sel), dim, dim)
        if not sel:
            if out is not None:
                raise ValueError("out is given but no view is selected")
            if snakes_out is None:
                raise ValueError("nothing to write: no view is selected and no table is asked for (snakes=True / snakes_out)")
        elif out is None:
            with torch.cuda.device(self.device):
                out = torch.empty(want, dtype=torch.uint8, device=self.device)
        else:
            self._checked(out, "out", torch.uint8, want)
        rc = self._cells_fn(self._h, mask, out.data_ptr() if sel else None,
                            snakes_out.data_ptr() if snakes_out is not None else None, self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_render_cells")
        if not sel:
            return snakes_out
        return out if snakes_out is None else (out, snakes_out)

    def local_shape(self, radius, snakes=None):
        """(S, W, W): one env's windows of render_local_device(radius, snakes), W = 2 * radius + 1."""
        w = 2 * check_radius(radius) + 1
        return (len(normalize_snakes(snakes, self.n_snakes)[1]), w, w)

    def render_local_device(self, radius, snakes=None, oriented=True, out=None, heading_out=None, heading=False):
        """Head-centred windows of cell codes (msnake_render_local): uint8 [num_envs, S, W, W], W = 2 * radius + 1, one
        window per selected snake in ascending snake order.  Entry [i, j] of snake s shows the cell head + (i - radius) * f
        + (j - radius) * g in the codes of view s of render_cells_device() (0 empty, 1 fruit, 2 / 3 own body / head, 4 / 5
        another snake's), or 6 outside the grid; oriented: f is the snake's direction of travel and g the move after it in
        the move table, so the snake looks along +i whatever its heading; otherwise f = (1, 0), g = (0, 1).  `snakes`:
        None = every snake, an int, or a strictly ascending sequence.  `heading_out`, a uint8 [num_envs, S] device tensor
        (heading=True: a fresh one), gets every selected snake's heading 0..3 (relative_to_absolute() takes it).  `out`
        must be a contiguous uint8 tensor of the shape above on this device; it needs no alignment.  Returns the windows,
        or (windows, heading) when the heading was asked for; nothing is synchronised.  Draws no random numbers and
        changes no env state."""
        torch = self._torch
        radius = check_radius(radius)
        mask, sel = normalize_snakes(snakes, self.n_snakes)
        if isinstance(oriented, (int, np.integer)) and oriented in (0, 1):
            oriented = int(oriented)
        else:
            raise ValueError(f"oriented must be True or False, got {oriented!r}")
        w = 2 * radius + 1
        want = (self.num_envs, len(sel), w, w)
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty(want, dtype=torch.uint8, device=self.device)
        else:
            self._checked(out, "out", torch.uint8, want)
        want = (self.num_envs, len(sel))
        if heading_out is None and heading:
            with torch.cuda.device(self.device):
                heading_out = torch.empty(want, dtype=torch.uint8, device=self.device)
        elif heading_out is not None:
            self._checked(heading_out, "heading_out", torch.uint8, want)
        rc = self._local_fn(self._h, radius, mask, oriented, out.data_ptr(),
                            heading_out.data_ptr() if heading_out is not None else None, self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_render_local")
        return out if heading_out is None else (out, heading_out)

    def rays_shape(self, snakes=None):
        """(S, 8, 4): one env's rays of render_rays_device(snakes)."""
        return (len(normalize_snakes(snakes, self.n_snakes)[1]), RAY_DIRS, RAY_CHANNELS)

    def render_rays_device(self, snakes=None, oriented=True, out=None, heading_out=None, heading=False):
        """Eight-direction ray observations (msnake_render_rays): uint8 [num_envs, S, 8, 4], one set per selected snake in
        ascending snake order.  Entry [j, c] of snake s looks from the head along direction j -- f, f + g, g, g - f, -f,
        -f - g, -g, f - g with f and g as in render_local_device(), a diagonal step counting as one -- and gives in
        channel c = 0 the number of steps to the first cell outside the grid (1..63) and in c = 1, 2, 3 the steps to the
        first fruit, the first piece of the snake's own body and the first piece of another snake in front of that wall,
        0 when there is none; the cells are read in the codes of view s of render_cells_device().  oriented: direction 0
        is the snake's direction of travel, and relative action r looks along direction 2 (r - 1); otherwise f = (1, 0),
        g = (0, 1).  `snakes`: None = every snake, an int, or a strictly ascending sequence.  `heading_out`, a uint8
        [num_envs, S] device tensor (heading=True: a fresh one), gets every selected snake's heading 0..3
        (relative_to_absolute() takes it).  `out` must be a contiguous uint8 tensor of the shape above on this device
        whose storage starts at a multiple of 4 bytes.  Returns the rays, or (rays, heading) when the heading was asked
        for; nothing is synchronised.  Draws no random numbers and changes no env state."""
        torch = self._torch
        mask, sel = normalize_snakes(snakes, self.n_snakes)
        if isinstance(oriented, (int, np.integer)) and oriented in (0, 1):
            oriented = int(oriented)
        else:
            raise ValueError(f"oriented must be True or False, got {oriented!r}")
        want = (self.num_envs, len(sel), RAY_DIRS, RAY_CHANNELS)
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.empty(want, dtype=torch.uint8, device=self.device)
        elif self._checked(out, "out", torch.uint8, want).data_ptr() % 4:
            raise ValueError("out must start at a multiple of 4 bytes (one direction's four channels are stored as one dword)")
        want = (self.num_envs, len(sel))
        if heading_out is None and heading:
            with torch.cuda.device(self.device):
                heading_out = torch.empty(want, dtype=torch.uint8, device=self.device)
        elif heading_out is not None:
            self._checked(heading_out, "heading_out", torch.uint8, want)
        rc = self._rays_fn(self._h, mask, oriented, out.data_ptr(), heading_out.data_ptr() if heading_out is not None else None,
                           self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_render_rays")
        return out if heading_out is None else (out, heading_out)

    @property
    def agent_tracker(self):
        """The int32 [num_envs, n_snakes, 8] device tensor msnake_agent_outcomes keeps its "before" facts and episode
        totals in (rows: _capi.AGENT_TRACK_WORDS); allocated on first use, owned by the env."""
        if self._track is None:
            with self._torch.cuda.device(self.device):
                self._track = self._torch.zeros((self.num_envs, self.n_snakes, 8), dtype=self._torch.int32, device=self.device)
        return self._track

    def arm_agents_device(self):
        """Write the tracker of agent_outcomes_device() from the env's current state, with every episode total zero
        (msnake_agent_outcomes with MSNAKE_AGENT_ARM).  The env does this itself before the next outcomes call after
        reset_device() without a mask, set_state_words(), set_state_all(), copy_envs_device(), import_states_device() and
        rollout_device(); a
        caller arms after anything else that moves the state without an outcomes call behind it (a step_device() whose
        outcomes were skipped, a masked reset of an env that was not done).  Returns the tracker; nothing is synchronised."""
        track = self.agent_tracker
        rc = self._agents_fn(self._h, _capi.AGENT_ARM, track.data_ptr(), None, None, None, None, None,
                             self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_agent_outcomes")
        self._track_stale = False
        return track

    def agent_outcomes_device(self, done, rew_out=None, ate_out=None, flags_out=None, info_out=None):
        """Every snake's outcome of the step just taken (msnake_agent_outcomes), called behind step_device() on an env
        created with auto_reset=False; `done` is that step's done tensor.  rew_out float32 [num_envs, n_snakes]: the rule
        set's reward formula applied to each snake (column 0 is the step's own reward); ate_out uint8 [num_envs,
        n_snakes]: fruits eaten, at most 255; flags_out uint8 [num_envs, n_snakes]: _capi.AGENT_ALIVE | AGENT_WAS_ALIVE |
        AGENT_DIED | AGENT_ENDED; info_out int32 [num_envs, n_snakes, 4]: ep_fruit, ep_alive_steps, first_death and
        ep_return (f32 bits) of the env's current episode after this step.  Only the outputs given are written; with none
        given all four go to tensors of the env's own, overwritten by the next such call.  Rows of a done env in the
        tracker are set up for the reset the caller issues next (reset_device(mask=done)).  Returns an AgentOutcomes
        (rew, ate, flags, info), None for what was not written; nothing is synchronised."""
        torch = self._torch
        n = (self.num_envs, self.n_snakes)
        if rew_out is None and ate_out is None and flags_out is None and info_out is None:
            if self._agents_own is None:
                with torch.cuda.device(self.device):
                    self._agents_own = AgentOutcomes(torch.zeros(n, dtype=torch.float32, device=self.device),
                                                     torch.zeros(n, dtype=torch.uint8, device=self.device),
                                                     torch.zeros(n, dtype=torch.uint8, device=self.device),
                                                     torch.zeros(n + (4,), dtype=torch.int32, device=self.device))
            res = self._agents_own
        else:
            res = AgentOutcomes(None if rew_out is None else self._checked(rew_out, "rew_out", torch.float32, n),
                                None if ate_out is None else self._checked(ate_out, "ate_out", torch.uint8, n),
                                None if flags_out is None else self._checked(flags_out, "flags_out", torch.uint8, n),
                                None if info_out is None else self._checked(info_out, "info_out", torch.int32, n + (4,)))
        done = self._mask(done)
        if self._track_stale:
            self.arm_agents_device()
        rc = self._agents_fn(self._h, 0, self._track.data_ptr(), done.data_ptr(), *[None if t is None else t.data_ptr() for t in res],
                             self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_agent_outcomes")
        return res

    def death_causes_device(self, before, cause_out=None, by_out=None, victims_out=None, where_out=None):
        """Why each snake died in the step just taken, and on whose body (msnake_death_causes; snake_env and adversarial).
        `before` is another MultiSnakeVecEnv that holds this env's state in front of that step -- before.copy_envs_device(
        self) ahead of step_device() -- and this env, created with auto_reset=False, has not been reset since.
        cause_out uint8 [num_envs, n_snakes]: _capi.CAUSE_WALL | CAUSE_SELF | CAUSE_HEAD_ON | CAUSE_BODY, 0 for a snake
        that did not die; by_out uint8 [num_envs, n_snakes]: bit k = on snake k's body, bit 4 + k = head-on with snake k;
        victims_out uint8 [num_envs, n_snakes]: the same from the killer's side (bit s of row k = snake s died on k's
        body, bit 4 + s = head-on); where_out int8 [num_envs, n_snakes, 2]: the cell the head died on, (-2, -2) for a
        snake that did not die.  Only the outputs given are written; with none given all four go to tensors of the env's
        own, overwritten by the next such call.  Returns a DeathCauses (cause, by, victims, where), None for what was
        not written; nothing is synchronised."""
        torch = self._torch
        if not isinstance(before, MultiSnakeVecEnv):
            raise TypeError(f"before must be a MultiSnakeVecEnv, got {type(before).__name__}")
        n = (self.num_envs, self.n_snakes)
        if cause_out is None and by_out is None and victims_out is None and where_out is None:
            if self._causes_own is None:
                with torch.cuda.device(self.device):
                    self._causes_own = DeathCauses(*[torch.zeros(n, dtype=torch.uint8, device=self.device) for _ in range(3)],
                                                   torch.zeros(n + (2,), dtype=torch.int8, device=self.device))
            res = self._causes_own
        else:
            res = DeathCauses(None if cause_out is None else self._checked(cause_out, "cause_out", torch.uint8, n),
                              None if by_out is None else self._checked(by_out, "by_out", torch.uint8, n),
                              None if victims_out is None else self._checked(victims_out, "victims_out", torch.uint8, n),
                              None if where_out is None else self._checked(where_out, "where_out", torch.int8, n + (2,)))
        rc = self._causes_fn(self._h, before._h, *[None if t is None else t.data_ptr() for t in res],
                             self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_death_causes")
        return res

    def step_agents_device(self, actions, out=None, causes=False):
        """step_device(), every snake's outcome of that step, and the reset of the envs it finished, on one stream:
        msnake_step -> msnake_agent_outcomes -> msnake_reset_envs(done).  Only on an env created with auto_reset=False.
        Returns (obs, rew, done, info, agents): the first four are exactly what an auto_reset=True env returns from
        step_device() (done envs show their reset observation), `agents` is the AgentOutcomes of
        agent_outcomes_device() in tensors of the env's own.  Nothing is synchronised.
        causes=True (snake_env and adversarial): the chain becomes msnake_copy_envs (into a snapshot env of this env's
        own, a clone() made on first use and closed with it) -> msnake_step -> msnake_agent_outcomes ->
        msnake_death_causes -> msnake_reset_envs(done), and the DeathCauses of death_causes_device(), in tensors of the
        env's own, is returned as a sixth element."""
        if self._ctor["auto_reset"]:
            raise ValueError("step_agents_device() needs an env created with auto_reset=False: the in-kernel auto reset "
                             "overwrites the terminal state that the other snakes' outcomes are read from")
        if self._track_stale:  # (before the step: the tracker holds the state the step starts from)
            self.arm_agents_device()
        if causes:
            if self._snapshot is None:
                self._snapshot = self.clone()
            rc = self._L.msnake_copy_envs(self._snapshot._h, self._h, None, self._cur_stream(self.device).cuda_stream)
            if rc < 0:
                _capi.check(rc, "msnake_copy_envs")
        obs, rew, done, info = self.step_device(actions, out)
        agents = self.agent_outcomes_device(done)
        why = self.death_causes_device(self._snapshot) if causes else None
        rc = self._reset_envs_fn(self._h, self._p_done, obs.data_ptr(), None, None, self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_reset_envs")
        return (obs, rew, done, info, agents, why) if causes else (obs, rew, done, info, agents)

    def rollout_device(self, tape, persistent=True, keep_obs=True):
        """T lockstep steps from an action tape int32 cuda [T, num_envs, >= n_snakes] in ONE call.

        persistent=True: msnake_rollout_tape (one launch, env state kept in registers across the steps);
        False: msnake_step_tape (one launch per step, issued from C).  Same results either way, and the
        same as T step_device() calls.  Returns fresh device tensors (obs uint8 [T, n, H, W, C] -- or
        only the last step's [n, H, W, C] when keep_obs is False --, rew f32 [T, n], done u8 [T, n],
        info i32 [T, n, 4]); nothing is synchronised."""
        torch = self._torch
        if self.terminal_obs:
            raise ValueError("rollout_device() is not available with terminal_obs=True: the tape paths have no per-step "
                             "masked reset")
        if tape.dtype != torch.int32 or tape.device != self.device or not tape.is_contiguous():
            tape = tape.to(device=self.device, dtype=torch.int32).contiguous()
        if tape.dim() != 3 or tape.shape[1] != self.num_envs or tape.shape[2] < self.n_snakes or tape.shape[0] < 1:
            raise ValueError(f"tape must be [T >= 1, {self.num_envs}, >= {self.n_snakes}], got {tuple(tape.shape)}")
        T, n = int(tape.shape[0]), self.num_envs
        H, W, C = self.obs_shape
        with torch.cuda.device(self.device):
            obs = torch.empty(((T, n) if keep_obs else (n,)) + (H, W, C), dtype=torch.uint8, device=self.device)
            rew = torch.empty((T, n), dtype=torch.float32, device=self.device)
            done = torch.empty((T, n), dtype=torch.uint8, device=self.device)
            info = torch.empty((T, n, 4), dtype=torch.int32, device=self.device)
        fn = self._L.msnake_rollout_tape if persistent else self._L.msnake_step_tape
        _capi.check(fn(self._h, tape.data_ptr(), int(tape.shape[2]), T, obs.data_ptr(), n * H * W * C if keep_obs else 0,
                       rew.data_ptr(), done.data_ptr(), info.data_ptr(), n, self._stream()),
                    "msnake_rollout_tape" if persistent else "msnake_step_tape")
        self._track_stale = True
        return obs, rew, done, info

    def copy_envs_device(self, src, index=None):
        """Overwrite envs of this env with the state of envs of `src`, another MultiSnakeVecEnv with the same dim,
        n_snakes, n_fruits and rules on the same device (msnake_copy_envs: one launch, no host round trip).  `index`:
        entry e names the env of `src` that env e receives, negative = env e stays as it is; an int32 / int64 tensor
        on this device, or a sequence / ndarray, which is uploaded; None = the identity (equal num_envs).  The envs'
        logging totals stay.  An env copied into the same global slot (equal seed and env_id_base, index[e] == e)
        continues bit-identically to its source; any other draws from its own slot's random stream at the copied
        counter.  Nothing is synchronised: the caller orders the call against work on both envs."""
        torch = self._torch
        if not isinstance(src, MultiSnakeVecEnv):
            raise TypeError(f"src must be a MultiSnakeVecEnv, got {type(src).__name__}")
        if self._pending is not None or src._pending is not None:
            raise RuntimeError("copy_envs_device() between step_async() and step_wait(): the pending step's results would "
                               "no longer belong to the state")
        if index is None:
            p_idx = None
        elif isinstance(index, torch.Tensor):
            if index.dtype not in (torch.int32, torch.int64) or tuple(index.shape) != (self.num_envs,):
                raise ValueError(f"an index tensor must be int32 or int64 of shape ({self.num_envs},), got {index.dtype} "
                                 f"{tuple(index.shape)}")
            if index.dtype == torch.int64:
                index = index.clamp(-1, 2**31 - 1)
            index = index.to(device=self.device, dtype=torch.int32).contiguous()
            p_idx = index.data_ptr()
        else:
            index = torch.from_numpy(normalize_copy_index(index, self.num_envs)).to(self.device)
            p_idx = index.data_ptr()
        rc = self._L.msnake_copy_envs(self._h, src._h, p_idx, self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_copy_envs")
        self._track_stale = True

    @property
    def state_words_max(self):
        """The largest word count any state this env accepts can have (msnake_state_words_max): a row of that many int32
        words holds every env, whatever is played or installed."""
        return _capi.check(self._L.msnake_state_words_max(self._h), "msnake_state_words_max")

    def _state_words(self, words, name):
        """A canonical-words tensor: contiguous int32 [num_envs, stride] on this device.  Returns (tensor, stride)."""
        torch = self._torch
        if (not isinstance(words, torch.Tensor) or words.dtype != torch.int32 or words.device != self.device or words.dim() != 2 or
                words.shape[0] != self.num_envs or not words.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous int32 tensor of shape ({self.num_envs}, stride) on {self.device}")
        return words, int(words.shape[1])

    def export_states_device(self, out=None, count_out=None, stride=None, words=True, count=True):
        """Every env's canonical words (the words of get_state_words) as rows of a device tensor, and how many each env
        has (msnake_export_states: one launch, no host round trip).  out int32 [num_envs, stride]: row e holds env e's
        words [0, count[e]); the words behind them are not written, and a row whose env needs more than `stride` words
        is not written at all -- its count says so.  count_out int32 [num_envs].  Without `out` a tensor of `stride`
        columns is allocated, state_words_max by default, which holds every env; words=False / count=False (without
        out / count_out): that output is skipped.  Returns (words, count), None for what was not written; nothing is
        synchronised."""
        torch = self._torch
        if out is not None:
            out, have = self._state_words(out, "out")
            if stride is not None and check_state_stride(stride, True) != have:
                raise ValueError(f"stride {stride} differs from out's row length {have}")
            stride = have
        elif words:
            stride = self.state_words_max if stride is None else check_state_stride(stride, True)
            with torch.cuda.device(self.device):
                out = torch.zeros((self.num_envs, stride), dtype=torch.int32, device=self.device)
        else:
            stride = 0 if stride is None else check_state_stride(stride)
        if count_out is not None:
            count_out = self._checked(count_out, "count_out", torch.int32, (self.num_envs,))
        elif count:
            with torch.cuda.device(self.device):
                count_out = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
        if out is None and count_out is None:
            raise ValueError("export_states_device(): nothing to write (words=False and count=False)")
        if out is not None and stride < 1:
            raise ValueError("out must have at least one column")
        rc = self._L.msnake_export_states(self._h, None if out is None else out.data_ptr(), stride,
                                          None if count_out is None else count_out.data_ptr(),
                                          self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_export_states")
        return out, count_out

    def import_states_device(self, words, mask=None, count=None, status_out=None):
        """Install rows of canonical words into the envs `mask` selects (msnake_import_states: one launch, no host round
        trip).  words int32 [num_envs, stride >= 8]; mask as for reset_device(), None = every env; count int32
        [num_envs]: the words of each row, None = every row has `stride` words (words behind the last snake are
        ignored).  Returns status uint8 [num_envs] (status_out if given): _capi.STATE_SKIPPED where the mask is 0,
        _capi.STATE_OK where the row was installed exactly as set_state_words() installs it, otherwise the reason
        (_capi.STATE_TOO_SHORT ... STATE_SCALAR) -- a refused env is left untouched, and a refusal raises nothing.  An env
        that runs a step kernel compiled for its shape refuses a head outside the grid (STATE_CELL); one on the generic
        kernels accepts it, as set_state_words() does.  Nothing is synchronised."""
        torch = self._torch
        if self._pending is not None:
            raise RuntimeError("import_states_device() between step_async() and step_wait(): the pending step's results "
                               "would no longer belong to the state")
        words, stride = self._state_words(words, "words")
        if stride < 8:
            raise ValueError(f"words must have at least 8 columns (no state has fewer words), got {stride}")
        p_mask = None if mask is None else self._mask(mask)
        p_count = None if count is None else self._checked(count, "count", torch.int32, (self.num_envs,))
        if status_out is None:
            with torch.cuda.device(self.device):
                status_out = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        else:
            status_out = self._checked(status_out, "status_out", torch.uint8, (self.num_envs,))
        self._track_stale = True
        rc = self._L.msnake_import_states(self._h, None if p_mask is None else p_mask.data_ptr(), words.data_ptr(), stride,
                                          None if p_count is None else p_count.data_ptr(), status_out.data_ptr(),
                                          self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_import_states")
        return status_out

    def _gen_lengths(self, lengths):
        """lengths -> contiguous int32 [num_envs, >= n_snakes] tensor on this device: an int (every snake), a sequence of
        n_snakes ints (every env), or such a tensor, used as it is.  An int or a sequence is expanded on the host and copied
        to the device once; the tensor of the last such request is kept, so repeating it costs no transfer."""
        torch = self._torch
        ns = self.n_snakes
        if isinstance(lengths, torch.Tensor):
            if (lengths.dtype != torch.int32 or lengths.device != self.device or lengths.dim() != 2 or lengths.shape[0] != self.num_envs or
                    lengths.shape[1] < ns or not lengths.is_contiguous()):
                raise ValueError(f"a lengths tensor must be contiguous int32 of shape ({self.num_envs}, >= {ns}) on {self.device}")
            return lengths
        if isinstance(lengths, (bool, np.bool_)):
            raise ValueError("lengths must be an int, a sequence of ints or an int32 tensor, got a bool")
        if isinstance(lengths, (int, np.integer)):
            row = [int(lengths)] * ns
        else:
            try:
                row = [int(x) for x in lengths]
            except (TypeError, ValueError):
                raise ValueError(f"lengths must be an int, a sequence of {ns} ints or an int32 tensor, got {lengths!r}") from None
            if len(row) != ns or any(isinstance(x, (bool, np.bool_, float, np.floating)) for x in lengths):
                raise ValueError(f"lengths must be one int per snake ({ns}), got {lengths!r}")
        if any(not -2 ** 31 <= x < 2 ** 31 for x in row):
            raise ValueError(f"lengths must fit an int32, got {lengths!r}")
        kept = getattr(self, "_gen_len_own", None)
        if kept is None or kept[0] != row:
            with self._alloc_ctx():
                kept = self._gen_len_own = (row, torch.tensor(row, dtype=torch.int32).repeat(self.num_envs, 1).to(self.device))
        return kept[1]

    def _alloc_ctx(self):
        """The context the env allocates its own tensors in: its HIP device (nothing on a host stand-in)."""
        return self._torch.cuda.device(self.device) if self.device.type == "cuda" else contextlib.nullcontext()

    def _gen_args(self, lengths, mask, salt):
        """The checks generate_states_device() and scatter_device() share -> (lengths tensor, mask tensor or None)."""
        if self.cfg.rules == _capi.RULES["new_world"]:
            raise ValueError("generate_states_device(): new_world is not supported (its alive / in_dead bookkeeping and its "
                             "init draws are another contract)")
        if isinstance(salt, (bool, np.bool_)) or not isinstance(salt, (int, np.integer)) or not 0 <= int(salt) < 2 ** 64:
            raise ValueError(f"salt must be an int in [0, 2^64), got {salt!r}")
        return self._gen_lengths(lengths), None if mask is None else self._mask(mask)

    def generate_states_device(self, lengths, mask=None, salt=0, compact=True, out=None, count_out=None, got_out=None):
        """Random legal positions in canonical words, built on the device for the envs `mask` selects
        (msnake_generate_states: one launch, no host round trip; snake_env and adversarial): non-overlapping snakes of
        the requested body lengths and fruits off the bodies.  `lengths`: an int, one int per snake, or an int32
        [num_envs, >= n_snakes] device tensor; below 0 counts as 0, snake 0 gets at least 1, 0 gives a dead snake.  mask as
        for reset_device(), None = every env; rows, counts and lengths of unselected envs are not written.  salt (0 ..
        2^64 - 1) picks the generator's stream, which is keyed by the global env id and never touches the env's own;
        compact=True grows bodies by Warnsdorff's rule, which is what lets long bodies reach their length.  out int32
        [num_envs, stride] (state_words_max columns when allocated here; a row that does not fit its stride is not
        written, its count says so), count_out int32 [num_envs], got_out int32 [num_envs, n_snakes]: the lengths reached.
        Returns (words, count, got), ready for import_states_device(words, mask=mask, count=count).  The env is only
        read.  With `lengths` (and `mask`) as device tensors and the three outputs given, the call is one launch: nothing
        is allocated, copied or synchronised, and it can be captured into a graph.  An int or a sequence of lengths, or
        a mask that is not a uint8 device tensor, is first copied from the host (a pageable transfer, not capturable;
        the lengths tensor of the last such request is kept and reused)."""
        torch = self._torch
        p_len, p_mask = self._gen_args(lengths, mask, salt)
        with self._alloc_ctx():
            if out is None:
                out = torch.zeros((self.num_envs, self.state_words_max), dtype=torch.int32, device=self.device)
            if count_out is None:
                count_out = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device)
            if got_out is None:
                got_out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32, device=self.device)
        out, stride = self._state_words(out, "out")
        if stride < 1:
            raise ValueError("out must have at least one column")
        count_out = self._checked(count_out, "count_out", torch.int32, (self.num_envs,))
        got_out = self._checked(got_out, "got_out", torch.int32, (self.num_envs, self.n_snakes))
        rc = self._L.msnake_generate_states(self._h, None if p_mask is None else p_mask.data_ptr(), p_len.data_ptr(),
                                            int(p_len.shape[1]), _capi.GEN_COMPACT if compact else 0, int(salt), out.data_ptr(),
                                            stride, count_out.data_ptr(), got_out.data_ptr(),
                                            self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_generate_states")
        return out, count_out, got_out

    def scatter_device(self, lengths, mask=None, salt=0, compact=True):
        """Put the envs `mask` selects (None = every env) onto generated positions: generate_states_device() followed by
        import_states_device(words, mask=mask, count=count) on the same stream, with buffers the env keeps (overwritten
        by the next call).  Returns (status, got): the status bytes of the import -- _capi.STATE_OK for every selected
        env, _capi.STATE_SKIPPED elsewhere -- and the lengths reached.  Two launches and nothing else when `lengths` and
        `mask` are device tensors (see generate_states_device() for what an int, a sequence or a host mask adds)."""
        torch = self._torch
        if self._pending is not None:
            raise RuntimeError("scatter_device() between step_async() and step_wait(): the pending step's results would no "
                               "longer belong to the state")
        p_len, p_mask = self._gen_args(lengths, mask, salt)
        if self._scatter_own is None:
            with self._alloc_ctx():
                self._scatter_own = (torch.zeros((self.num_envs, self.state_words_max), dtype=torch.int32, device=self.device),
                                     torch.zeros(self.num_envs, dtype=torch.int32, device=self.device),
                                     torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32, device=self.device),
                                     torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device))
        words, count, got, status = self._scatter_own
        self.generate_states_device(p_len, mask=p_mask, salt=salt, compact=compact, out=words, count_out=count, got_out=got)
        return self.import_states_device(words, mask=p_mask, count=count, status_out=status), got

    def hash_states_device(self, what="full", out=None):
        """A 64-bit hash of every env's canonical words (msnake_hash_states): int64 [num_envs] holding the 64 bits, equal
        to msnake.state_hash(get_state_words(e), what) for every env.  what "full": every word; "board": the position
        only (t, the draw counter, ep_len, ep_return and the finished bit left out) -- equal board hashes render the
        same frame.  Nothing is synchronised."""
        torch = self._torch
        code = normalize_hash_what(what)
        if out is None:
            with torch.cuda.device(self.device):
                out = torch.zeros(self.num_envs, dtype=torch.int64, device=self.device)
        else:
            out = self._checked(out, "out", torch.int64, (self.num_envs,))
        rc = self._L.msnake_hash_states(self._h, code, out.data_ptr(), self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_hash_states")
        return out

    def _playout_policies(self, policies):
        """One policy name for every snake, or one per snake -> (ctypes int32 [MAX_SNAKES], the ids)."""
        if policies is None or isinstance(policies, str):
            policies = [policies] * self.n_snakes
        policies = list(policies)
        if len(policies) != self.n_snakes:
            raise ValueError(f"policies must be one name or one per snake ({self.n_snakes}), got {len(policies)}")
        ids = []
        for name in policies:
            if name not in _capi.PLAYOUT_POLICY:
                raise ValueError(f"policies must be 'safe_greedy', 'hamiltonian', 'wary_greedy' or None, got {name!r}")
            if name == "hamiltonian" and int(self.cfg.dim) % 2:
                raise ValueError(f"policies: 'hamiltonian' needs an even dim (the cycle), got dim {int(self.cfg.dim)}")
            ids.append(_capi.PLAYOUT_POLICY[name])
        return (ctypes.c_int32 * _capi.MAX_SNAKES)(*ids), ids

    def _explore_args(self, explore, salt):
        """`explore`, a probability in [0, 1] for every snake or one per snake, and `salt` -> (ctypes uint32 [MAX_SNAKES] of
        eps_q16 = round(p * 65536), the salt as an int)."""
        if isinstance(salt, (bool, np.bool_)) or not isinstance(salt, (int, np.integer)) or not 0 <= int(salt) < 2 ** 64:
            raise ValueError(f"salt must be an int in [0, 2^64), got {salt!r}")
        if isinstance(explore, (int, float, np.integer, np.floating)) and not isinstance(explore, (bool, np.bool_)):
            explore = [explore] * self.n_snakes
        try:
            explore = list(explore)
        except TypeError:
            raise ValueError(f"explore must be a probability in [0, 1] or one per snake, got {explore!r}") from None
        if len(explore) != self.n_snakes:
            raise ValueError(f"explore must be one probability or one per snake ({self.n_snakes}), got {len(explore)}")
        eps = []
        for x in explore:
            if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)) or not 0.0 <= float(x) <= 1.0:
                raise ValueError(f"explore: a probability must lie in [0, 1], got {x!r}")
            eps.append(int(round(float(x) * _capi.EXPLORE_ONE)))
        return (ctypes.c_uint32 * _capi.MAX_SNAKES)(*eps), int(salt)

    def explore_actions_device(self, policies, explore, salt=0, snakes=None, out=None, explored_out=None):
        """Exploring scripted players (msnake_explore_actions): for the snakes in `snakes` (indices; default every snake)
        the action of its policy -- `policies` as playout_device() takes them -- or, with probability `explore` (a float in
        [0, 1] for all snakes or one per snake, taken as round(p * 65536) / 65536), a uniformly random member of its
        candidate set: the open moves, under "wary_greedy" that policy's own candidates.  The draw comes from a stream
        keyed by the env's seed, `salt` (0 .. 2^64 - 1), the global env id and the state's step and draw counters; it never
        touches the env's own, needs no torch RNG and repeats exactly for the same state: the very word
        playout_device(explore=..., salt=...) plays for that state.  Actions go to columns `snakes` of `out`, an int32
        [num_envs, >= n_snakes] device tensor as step_device() takes it (None: the cached tensor of
        scripted_actions_device()); `explored_out`, a uint8 [num_envs, n_snakes] device tensor, gets 1 where the action was
        drawn, for every snake.  Returns `out`, or (out, explored_out) when that was given.  "wary_greedy" needs snake_env
        or adversarial rules.  One launch; nothing is synchronised and the env is only read."""
        torch = self._torch
        pol, ids = self._playout_policies(policies)
        if _capi.PLAYOUT_POLICY[_capi.WARY_POLICY] in ids and self.cfg.rules == _capi.RULES["new_world"]:
            raise ValueError(f"policies: {_capi.WARY_POLICY!r} needs snake_env or adversarial rules, got 'new_world'")
        eps, salt = self._explore_args(explore, salt)
        if snakes is None:
            bits = (1 << self.n_snakes) - 1
        else:
            bits = 0
            for s in snakes:
                if int(s) != s or not 0 <= int(s) < self.n_snakes:
                    raise ValueError(f"snake indices must lie in [0, {self.n_snakes}), got {s!r}")
                bits |= 1 << int(s)
        if not bits:
            raise ValueError("snakes: no snake selected (no action to write)")
        if out is None:
            if getattr(self, "_scripted_out", None) is None:
                with self._alloc_ctx():
                    self._scripted_out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32, device=self.device)
            out = self._scripted_out
        elif (not isinstance(out, torch.Tensor) or out.dtype != torch.int32 or out.device != self.device or out.dim() != 2 or
              out.shape[0] != self.num_envs or out.shape[1] < self.n_snakes or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int32 tensor of shape ({self.num_envs}, >= {self.n_snakes}) on {self.device}")
        p_explored = None
        if explored_out is not None:
            p_explored = self._checked(explored_out, "explored_out", torch.uint8, (self.num_envs, self.n_snakes)).data_ptr()
        rc = self._L.msnake_explore_actions(self._h, pol, eps, salt, bits, out.data_ptr(), int(out.shape[1]), p_explored,
                                            self._cur_stream(self.device).cuda_stream)
        if rc < 0:
            _capi.check(rc, "msnake_explore_actions")
        return out if explored_out is None else (out, explored_out)

    def playout_device(self, n_steps, policies="safe_greedy", first_actions=None, first_snakes=None, end_state=False, out=None,
                       explore=None, salt=0):
        """Play every env on for up to `n_steps` steps with a scripted policy per snake, in one launch, without touching
        the env (msnake_playout; snake_env): the value of a position.  `policies`: one of "safe_greedy", "hamiltonian",
        "wary_greedy" or None (the constant action 0) for all snakes, or one per snake.  `first_actions`, an int32
        [num_envs, >= n_snakes] device tensor as step_device() takes it, forces the first action of the snakes in
        `first_snakes` (indices; default every snake); the other snakes, and every later step, follow their policy.
        Returns a Playout of device tensors: steps int32 [num_envs] (steps played; an env stops behind its first done
        step), end uint8 [num_envs] (_capi.PLAYOUT_HORIZON / _DEAD / _CAP / _FINISHED), ret float32 [num_envs, n_snakes]
        (every snake's summed reward, -1 for its death and +1 per fruit), info int32 [num_envs, n_snakes, 4] (fruits
        eaten, steps survived, the 1-based step of its death or 0, the action word of step 1); with `end_state` also
        words int32 [num_envs, state_words_max] and count int32 [num_envs], the state each playout ended in, as
        export_states_device() writes them and import_states_device() takes them -- else None.  `out`: a Playout (or
        six-entry sequence) of tensors to write into, None for what is not wanted; `end_state` is then ignored and
        words may have any stride.  `explore` (None: nobody explores, msnake_playout): a probability in [0, 1] for all
        snakes or one per snake with which a snake plays, in any step, a uniformly random member of its candidate set in
        place of its policy's move (msnake_playout_explore; the rule and the stream, keyed by `salt`, are those of
        explore_actions_device()); a forced first action wins over it.  Nothing is synchronised; no random number of the
        env is consumed."""
        torch = self._torch
        n, ns, dev = self.num_envs, self.n_snakes, self.device
        if int(n_steps) != n_steps or not 1 <= int(n_steps) <= _capi.PLAYOUT_MAX_STEPS:
            raise ValueError(f"n_steps must lie in [1, {_capi.PLAYOUT_MAX_STEPS}], got {n_steps!r}")
        if self.cfg.rules != _capi.RULES["snake_env"]:
            raise ValueError(f"playout_device() needs a snake_env env, got rules {_capi.RULE_NAMES[int(self.cfg.rules)]!r}")
        pol, _ = self._playout_policies(policies)
        eps, salt = (None, 0) if explore is None else self._explore_args(explore, salt)
        bits, p_first, stride = 0, None, 0
        if first_actions is None:
            if first_snakes is not None:
                raise ValueError("first_snakes needs first_actions")
        else:
            if (not isinstance(first_actions, torch.Tensor) or first_actions.dtype != torch.int32 or first_actions.device != dev or
                    first_actions.dim() != 2 or first_actions.shape[0] != n or first_actions.shape[1] < ns or
                    not first_actions.is_contiguous()):
                raise ValueError(f"first_actions must be a contiguous int32 tensor of shape ({n}, >= {ns}) on {dev}")
            if first_snakes is None:
                bits = (1 << ns) - 1
            else:
                for s in first_snakes:
                    if int(s) != s or not 0 <= int(s) < ns:
                        raise ValueError(f"first_snakes: snake indices must lie in [0, {ns}), got {s!r}")
                    bits |= 1 << int(s)
            if bits:
                p_first, stride = first_actions.data_ptr(), int(first_actions.shape[1])
        if out is None:
            out = Playout(torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                          torch.zeros((n, ns), dtype=torch.float32, device=dev),
                          torch.zeros((n, ns, 4), dtype=torch.int32, device=dev),
                          torch.zeros((n, self.state_words_max), dtype=torch.int32, device=dev) if end_state else None,
                          torch.zeros(n, dtype=torch.int32, device=dev) if end_state else None)
        elif len(out) != 6:
            raise ValueError(f"out: a Playout has six entries (steps, end, ret, info, words, count), got {len(out)}")
        want = (("steps", torch.int32, (n,)), ("end", torch.uint8, (n,)), ("ret", torch.float32, (n, ns)),
                ("info", torch.int32, (n, ns, 4)))
        res = [None if t is None else self._checked(t, f"out.{name}", dt, shape) for t, (name, dt, shape) in zip(out[:4], want)]
        words, wstride = (None, 0) if out[4] is None else self._state_words(out[4], "out.words")
        if words is not None and wstride < 1:
            raise ValueError("out.words must have at least one column")
        count = None if out[5] is None else self._checked(out[5], "out.count", torch.int32, (n,))
        res = Playout(*res, words, count)
        if all(t is None for t in res):
            raise ValueError("out: nothing to write (all six entries are None)")
        rest = (int(n_steps), p_first, stride, bits, *[None if t is None else t.data_ptr() for t in res[:5]], wstride,
                None if count is None else count.data_ptr(), self._cur_stream(dev).cuda_stream)
        if eps is None:
            rc = self._L.msnake_playout(self._h, pol, *rest)
        else:
            rc = self._L.msnake_playout_explore(self._h, pol, eps, salt, *rest)
        if rc < 0:
            _capi.check(rc, "msnake_playout" if eps is None else "msnake_playout_explore")
        return res

    def playout_values_device(self, scratch, n_steps, snake=0, reps=1, policies="safe_greedy", explore=None, salt=0):
        """The value of each of `snake`'s four moves in every env, by playouts on forks: (value, survive), both float32
        [num_envs, 4].  `scratch`: an env of the same board with num_envs * 4 * reps envs; env e is copied into its slots
        (e * 4 + m) * reps + r (copy_envs_device), and one playout_device() of n_steps steps there forces `snake`'s first
        action to m + 1, everything else following `policies`.  value[e, m] is the mean over r of the snake's summed
        reward, survive[e, m] the share of the reps in which it did not die.  The slots draw from their own random
        streams at the copied counter, which is what makes the reps differ once somebody eats; with `explore` (and
        `salt`, both as playout_device() takes them) the snakes also explore inside the playouts, every slot from its own
        stream, so the reps differ from the first step on.  Two launches and a few torch reductions; nothing is
        synchronised and this env is only read."""
        torch = self._torch
        n, ns = self.num_envs, self.n_snakes
        if int(snake) != snake or not 0 <= int(snake) < ns:
            raise ValueError(f"snake must lie in [0, {ns}), got {snake!r}")
        if int(reps) != reps or int(reps) < 1:
            raise ValueError(f"reps must be >= 1, got {reps!r}")
        snake, reps = int(snake), int(reps)
        more = {} if explore is None else dict(explore=explore, salt=salt)
        if more:
            self._explore_args(explore, salt)  # (refused here, before the copy)
        if not isinstance(scratch, MultiSnakeVecEnv):
            raise TypeError(f"scratch must be a MultiSnakeVecEnv, got {type(scratch).__name__}")
        if scratch.num_envs != n * 4 * reps:
            raise ValueError(f"scratch must have num_envs * 4 * reps = {n * 4 * reps} envs, got {scratch.num_envs}")
        key = (scratch.num_envs, snake, reps)
        if getattr(self, "_playout_plan", (None,))[0] != key:
            slot = torch.arange(n * 4 * reps, device=self.device)
            first = torch.zeros((n * 4 * reps, ns), dtype=torch.int32, device=self.device)
            first[:, snake] = ((slot // reps) % 4 + 1).to(torch.int32)
            self._playout_plan = (key, (slot // (4 * reps)).to(torch.int32), first)
        _, index, first = self._playout_plan
        scratch.copy_envs_device(self, index)
        res = scratch.playout_device(n_steps, policies, first_actions=first, first_snakes=[snake], **more)
        value = res.ret[:, snake].reshape(n, 4, reps).mean(dim=2)
        survive = (res.info[:, snake, 2] == 0).to(torch.float32).reshape(n, 4, reps).mean(dim=2)
        return value, survive

    def clone(self, num_envs=None, **overrides):
        """A new MultiSnakeVecEnv with this env's configuration; `overrides` may change what a device-side copy lets
        differ (CLONE_OVERRIDES).  With the same number of envs (the default) it starts as a copy of this env's state
        (copy_envs_device with the identity) -- a snapshot to roll back to when seed and env_id_base are kept;
        with another num_envs its envs are unset until reset_device() or copy_envs_device(self, index)."""
        bad = sorted(set(overrides) - set(CLONE_OVERRIDES))
        if bad:
            raise ValueError(f"clone() can override {', '.join(CLONE_OVERRIDES)}; got {', '.join(bad)}")
        n = self.num_envs if num_envs is None else int(num_envs)
        new = MultiSnakeVecEnv(n, **dict(self._ctor, **overrides))
        if n == self.num_envs:
            new.copy_envs_device(self)
        return new

    def render_device(self, out=None):
        obs = self._out(out)
        _capi.check(self._L.msnake_render(self._h, obs.data_ptr(), self._stream()), "msnake_render")
        return obs

    # ------------------------------------------------------------------ VecEnv surface (NumPy out)
    def _obs_to_host(self, obs):
        if not self._host_views:
            return obs.cpu().numpy()
        self._pinned[0].copy_(obs, non_blocking=True)
        self._torch.cuda.current_stream(self.device).synchronize()
        return self._pinned[0].numpy()

    def reset(self, mask=None):
        """mask=None: reset every env.  Otherwise only the selected envs (see reset_device); the returned array is
        the full observation batch, in which unselected envs keep their last observation (gymnasium's reset_mask)."""
        if mask is None:
            self._tstart = time.time()
        return self._obs_to_host(self.reset_device(mask))

    def step_async(self, actions):
        torch = self._torch
        if isinstance(actions, torch.Tensor):
            a = actions
        else:
            a = torch.from_numpy(normalize_actions(actions, self.num_envs, self.n_snakes)).to(self.device)
        self._pending = self.step_device(a)

    def step_wait(self):
        if self._pending is None:
            raise RuntimeError("step_wait() called without step_async()")  # NotSteppingError in baselines
        obs, rew, done, info = self._pending
        self._pending = None
        if self._host_views:
            for dst, src in zip(self._pinned, (obs, rew, done, info)):
                dst.copy_(src, non_blocking=True)
            self._torch.cuda.current_stream(self.device).synchronize()
            obs_h, rew_h, done_u8, info_h = (t.numpy() for t in self._pinned)
        else:
            obs_h, rew_h, done_u8, info_h = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy()
        done_h = done_u8.astype(bool)
        terminal = None
        if self.terminal_obs:  # (the copies above have synchronised the stream)
            terminal = (self.final_obs[done.bool()].cpu().numpy(), self.truncated.cpu().numpy())
        infos = LazyInfos(done_h, info_h[:, 2].copy(), info_h[:, 0].copy().view(np.float32), info_h[:, 1].copy(),
                          round(time.time() - self._tstart, 6), terminal)
        return obs_h, rew_h, done_h, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def render(self, mode="rgb_array"):
        """mode "rgb_array": the frames of every env; mode "cells": env 0's cell-code planes, uint8 [views, dim, dim]
        (render_cells_device), as the host convenience.  Always a fresh array."""
        if mode == "cells":
            return self.render_cells_device()[0].cpu().numpy()
        return self.render_device().cpu().numpy()

    def close(self):
        snapshot, self._snapshot = getattr(self, "_snapshot", None), None
        if snapshot is not None:
            snapshot.close()
        if not self.closed and self._h:
            self._L.msnake_destroy(self._h)
            self._h = ctypes.c_void_p()
        self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    @property
    def unwrapped(self):
        return self

    # ------------------------------------------------------------------ state / stats (tests, logging)
    def get_state_words(self, env):
        n = _capi.check(self._L.msnake_get_state(self._h, env, None, 0), "msnake_get_state")
        buf = np.zeros(n, np.int32)
        _capi.check(self._L.msnake_get_state(self._h, env, buf.ctypes.data, n), "msnake_get_state")
        return buf

    def set_state_words(self, env, words):
        w = np.ascontiguousarray(words, dtype=np.int32)
        self._track_stale = True  # (also when the words are refused: arming once more is harmless)
        _capi.check(self._L.msnake_set_state(self._h, env, w.ctypes.data, len(w)), "msnake_set_state")

    def get_state_all(self):
        """Canonical state of every env as one bytes-like blob (numpy uint8; layout: include/msnake.h)."""
        n = _capi.check(self._L.msnake_get_state_all(self._h, None, 0), "msnake_get_state_all")
        buf = np.zeros(n, np.uint8)
        _capi.check(self._L.msnake_get_state_all(self._h, buf.ctypes.data, n), "msnake_get_state_all")
        return buf

    def set_state_all(self, blob):
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob, dtype=np.uint8)
        self._track_stale = True
        _capi.check(self._L.msnake_set_state_all(self._h, b.ctypes.data, b.nbytes), "msnake_set_state_all")

    @staticmethod
    def blob_info(blob):
        """What a get_state_all() blob holds (host-only check, no handle needed): dict with version, num_envs,
        dim, n_snakes, n_fruits, rules (name), total_words.  Raises RuntimeError for a malformed blob."""
        b = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob, dtype=np.uint8)
        bi = _capi.MsnakeBlobInfo()
        _capi.check(_capi.load().msnake_state_blob_info(b.ctypes.data, b.nbytes, ctypes.byref(bi)), "msnake_state_blob_info")
        return {"version": bi.version, "num_envs": bi.num_envs, "dim": bi.dim, "n_snakes": bi.n_snakes,
                "n_fruits": bi.n_fruits, "rules": _capi.RULE_NAMES.get(bi.rules, bi.rules), "total_words": bi.total_words}

    def stats(self, reset=False):
        st = _capi.MsnakeStats()
        _capi.check(self._L.msnake_get_stats(self._h, ctypes.byref(st), int(reset)), "msnake_get_stats")
        return {"episodes": st.episodes, "ep_len_sum": st.ep_len_sum, "ep_return_sum": st.ep_return_sum,
                "env_steps": st.env_steps, "errors": st.errors}

    def kernel_name(self):
        return self._L.msnake_kernel_name(self._h).decode()

    def algorithmic_bytes_per_env_step(self):
        return int(self._L.msnake_algorithmic_bytes_per_env_step(self._h))


def make(env_id, num_envs, n_snakes=None, **kw):
    """make('snake-multiple-test-v0', 4096, n_snakes=3) -- the reference's gym ids as presets."""
    preset = dict(GYM_IDS[env_id])
    if n_snakes is not None:
        preset["n_snakes"] = n_snakes
    preset.update(kw)
    return MultiSnakeVecEnv(num_envs, **preset)
