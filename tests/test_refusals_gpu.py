"""Every refusal of the host glue, pinned in full: the return code and the whole text of msnake_last_error() for the C entry
points, the whole text of the ValueError for the tensor checks of MultiSnakeVecEnv.

The expected strings are literals, written out from the sources with the format arguments filled in by hand.  Calls that
are wrong in two ways at once pin the order of the checks.  Every bad pointer is refused on the host before anything is
launched: a misaligned pointer points into a live, over-allocated tensor, a NULL one is never dereferenced.  After the
refusals every output buffer still holds its guard value, the canonical state is the one it was, and env_steps is 0.
"""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 9
ARG, HANDLE, ALIGN = -1, -3, -4          # MSNAKE_E_ARG, MSNAKE_E_HANDLE, MSNAKE_E_ALIGN


class Bufs:
    """Guard-filled device buffers, each with spare bytes behind what a call would write, so that a pointer moved off
    its alignment still points into live memory."""

    def __init__(self, env, obs_numel):
        import torch
        full = lambda n, dt: torch.full((n,), GUARD, dtype=dt, device=env.device)
        self.acts = full(2 * 7 + 4, torch.int32)        # any action_stride up to 7
        self.rew = full(2 + 4, torch.float32)
        self.done = full(2 + 4, torch.uint8)
        self.info = full(2 * 4 + 8, torch.int32)
        self.obs = full(obs_numel + 16, torch.uint8)
        self.final = full(obs_numel + 16, torch.uint8)
        self.trunc = full(2 + 4, torch.uint8)
        self.mask = torch.ones(2 + 4, dtype=torch.uint8, device=env.device)
        self.safe = full(2 * 2 + 4, torch.uint8)
        self.count = full(2 * 2 * 4 + 4, torch.int16)   # space_dev / territory_dev
        self.cells = full(2 * 3 * 4 * 4 + 4, torch.uint8)
        self.table = full(2 * 2 * 8 + 4, torch.int32)
        self.win = full(2 * 2 * 3 * 3 + 4, torch.uint8)
        self.head = full(2 * 2 + 4, torch.uint8)
        self.guarded = [getattr(self, k) for k in ("acts", "rew", "done", "info", "obs", "final", "trunc", "safe", "count",
                                                   "cells", "table", "win", "head")]

    def untouched(self):
        return all(bool((t == GUARD).all()) for t in self.guarded) and bool((self.mask == 1).all())


def _env(**kw):
    import msnake
    env = msnake.MultiSnakeVecEnv(2, n_snakes=2, rules="snake_env", seed=3, device="cuda:0", **kw)
    env.reset_device()
    return env


def _refused(env, cases):
    """cases: (entry point, arguments behind the handle, return code, message)"""
    L = env._L
    for name, args, want_rc, want_msg in cases:
        rc = getattr(L, name)(env._h, *args)
        msg = L.msnake_last_error().decode()
        assert (rc, msg) == (want_rc, want_msg), (name, args, rc, msg)


def test_c_entry_points_refuse_with_the_same_code_and_text():
    import torch
    env = _env(dim=4)
    b = Bufs(env, 2 * 6 * 6 * 9)
    before = env.get_state_all().copy()
    a, r, d, i, o = b.acts.data_ptr(), b.rew.data_ptr(), b.done.data_ptr(), b.info.data_ptr(), b.obs.data_ptr()
    s, c, m = b.safe.data_ptr(), b.count.data_ptr(), b.mask.data_ptr()
    ce, tb, w, hd = b.cells.data_ptr(), b.table.data_ptr(), b.win.data_ptr(), b.head.data_ptr()
    assert i % 16 == 0
    N = None
    null3 = "actions/rew/done must not be NULL"
    stride1, stride8 = "action_stride 1 must be in [n_snakes=2, 7]", "action_stride 8 must be in [n_snakes=2, 7]"
    align = "actions/rew must be 4-byte and info 16-byte aligned"
    _refused(env, [
        # ---- msnake_step(actions_dev, action_stride, obs_dev, rew_dev, done_dev, info_dev, stream)
        ("msnake_step", (N, 2, o, r, d, i, N), ARG, "msnake_step: " + null3),
        ("msnake_step", (a, 2, o, N, d, i, N), ARG, "msnake_step: " + null3),
        ("msnake_step", (a, 2, o, r, N, i, N), ARG, "msnake_step: " + null3),
        ("msnake_step", (a, 1, o, r, d, i, N), ARG, stride1),
        ("msnake_step", (a, 8, o, r, d, i, N), ARG, stride8),
        ("msnake_step", (a + 2, 2, o, r, d, i, N), ALIGN, align),
        ("msnake_step", (a, 2, o, r + 2, d, i, N), ALIGN, align),
        ("msnake_step", (a, 2, o, r, d, i + 4, N), ALIGN, align),
        ("msnake_step", (a, 2, o, r, d, i + 8, N), ALIGN, align),
        ("msnake_step", (N, 1, o, r, d, i, N), ARG, "msnake_step: " + null3),         # the pointers before the stride
        ("msnake_step", (a + 2, 1, o, r, d, i, N), ARG, stride1),                     # the stride before the alignment
        ("msnake_step", (N, 2, o, r + 2, d, i, N), ARG, "msnake_step: " + null3),
        # ---- msnake_rollout_tape(actions_dev, action_stride, n_steps, obs_dev, obs_step_stride, rew_dev, done_dev,
        #                          info_dev, scalar_step_stride, stream)
        ("msnake_rollout_tape", (a, 2, 0, o, 0, r, d, i, 0, N), ARG, "n_steps must be >= 1"),
        ("msnake_rollout_tape", (a, 2, -1, o, 0, r, d, i, 0, N), ARG, "n_steps must be >= 1"),
        ("msnake_rollout_tape", (N, 1, 0, o, 0, r, d, i, 0, N), ARG, "n_steps must be >= 1"),   # n_steps first
        ("msnake_rollout_tape", (N, 2, 1, o, 0, r, d, i, 0, N), ARG, "msnake_rollout_tape: " + null3),
        ("msnake_rollout_tape", (a, 2, 1, o, 0, N, d, i, 0, N), ARG, "msnake_rollout_tape: " + null3),
        ("msnake_rollout_tape", (a, 2, 1, o, 0, r, N, i, 0, N), ARG, "msnake_rollout_tape: " + null3),
        ("msnake_rollout_tape", (a, 1, 1, o, 0, r, d, i, 0, N), ARG, stride1),
        ("msnake_rollout_tape", (a, 8, 1, o, 0, r, d, i, 0, N), ARG, stride8),
        ("msnake_rollout_tape", (a + 2, 2, 1, o, 0, r, d, i, 0, N), ALIGN, align),
        ("msnake_rollout_tape", (a, 2, 1, o, 0, r + 2, d, i, 0, N), ALIGN, align),
        ("msnake_rollout_tape", (a, 2, 1, o, 0, r, d, i + 4, 0, N), ALIGN, align),
        ("msnake_rollout_tape", (N, 1, 1, o, 0, r, d, i, 0, N), ARG, "msnake_rollout_tape: " + null3),
        ("msnake_rollout_tape", (a + 2, 8, 1, o, 0, r, d, i, 0, N), ARG, stride8),
        # ---- msnake_scripted_actions(policy, snake_mask, actions_dev, action_stride, safe_dev, stream)
        ("msnake_scripted_actions", (3, 1, a, 2, s, N), ARG, "msnake_scripted_actions: policy 3 is not one of MSNAKE_POLICY_*"),
        ("msnake_scripted_actions", (-1, 1, a, 2, s, N), ARG, "msnake_scripted_actions: policy -1 is not one of MSNAKE_POLICY_*"),
        ("msnake_scripted_actions", (3, 0b100, N, 1, N, N), ARG, "msnake_scripted_actions: policy 3 is not one of MSNAKE_POLICY_*"),
        ("msnake_scripted_actions", (1, 0b100, a, 2, s, N), ARG, "msnake_scripted_actions: snake_mask 0x4 has a bit >= n_snakes=2"),
        ("msnake_scripted_actions", (0, 0b111, N, 0, s, N), ARG, "msnake_scripted_actions: snake_mask 0x7 has a bit >= n_snakes=2"),
        ("msnake_scripted_actions", (1, 0b110, N, 1, N, N), ARG, "msnake_scripted_actions: snake_mask 0x6 has a bit >= n_snakes=2"),
        ("msnake_scripted_actions", (0, 0b11, a, 2, N, N), ARG,
         "msnake_scripted_actions: nothing to write (policy NONE or snake_mask 0, and safe_dev is NULL)"),
        ("msnake_scripted_actions", (1, 0, a, 2, N, N), ARG,
         "msnake_scripted_actions: nothing to write (policy NONE or snake_mask 0, and safe_dev is NULL)"),
        ("msnake_scripted_actions", (2, 0, N, 0, N, N), ARG,
         "msnake_scripted_actions: nothing to write (policy NONE or snake_mask 0, and safe_dev is NULL)"),
        ("msnake_scripted_actions", (1, 1, N, 2, s, N), ARG, "msnake_scripted_actions: actions_dev is NULL"),
        ("msnake_scripted_actions", (2, 1, N, 1, s, N), ARG, "msnake_scripted_actions: actions_dev is NULL"),   # the pointer first
        ("msnake_scripted_actions", (1, 0b11, a, 1, s, N), ARG, "msnake_scripted_actions: action_stride 1 must be >= n_snakes=2"),
        ("msnake_scripted_actions", (1, 0b11, a + 2, 1, s, N), ARG, "msnake_scripted_actions: action_stride 1 must be >= n_snakes=2"),
        ("msnake_scripted_actions", (1, 0b11, a + 2, 2, s, N), ALIGN, "actions_dev must be 4-byte aligned"),
        ("msnake_scripted_actions", (2, 0b01, a + 1, 7, N, N), ALIGN, "actions_dev must be 4-byte aligned"),
        # ---- msnake_space_actions(snake_mask, actions_dev, action_stride, safe_dev, space_dev, stream)
        ("msnake_space_actions", (0b100, a, 2, s, c, N), ARG, "msnake_space_actions: snake_mask 0x4 has a bit >= n_snakes=2"),
        ("msnake_space_actions", (0b101, N, 1, N, c + 1, N), ARG, "msnake_space_actions: snake_mask 0x5 has a bit >= n_snakes=2"),
        ("msnake_space_actions", (0, a, 2, N, N, N), ARG,
         "msnake_space_actions: nothing to write (snake_mask 0, safe_dev and space_dev are NULL)"),
        ("msnake_space_actions", (0, N, 0, N, N, N), ARG,
         "msnake_space_actions: nothing to write (snake_mask 0, safe_dev and space_dev are NULL)"),
        ("msnake_space_actions", (1, N, 2, s, c, N), ARG, "msnake_space_actions: actions_dev is NULL"),
        ("msnake_space_actions", (1, N, 1, s, c, N), ARG, "msnake_space_actions: actions_dev is NULL"),         # the pointer first
        ("msnake_space_actions", (1, N, 2, s, c + 1, N), ARG, "msnake_space_actions: actions_dev is NULL"),
        ("msnake_space_actions", (0b11, a, 1, s, c, N), ARG, "msnake_space_actions: action_stride 1 must be >= n_snakes=2"),
        ("msnake_space_actions", (0b11, a + 2, 0, s, c, N), ARG, "msnake_space_actions: action_stride 0 must be >= n_snakes=2"),
        ("msnake_space_actions", (0b11, a + 2, 2, s, c, N), ALIGN, "actions_dev must be 4-byte aligned"),
        ("msnake_space_actions", (0b11, a + 2, 2, s, c + 1, N), ALIGN, "actions_dev must be 4-byte aligned"),  # actions before counts
        ("msnake_space_actions", (0b11, a, 2, s, c + 1, N), ALIGN, "space_dev must be 2-byte aligned"),
        ("msnake_space_actions", (0, N, 0, N, c + 1, N), ALIGN, "space_dev must be 2-byte aligned"),
        # ---- msnake_territory_actions(snake_mask, actions_dev, action_stride, safe_dev, territory_dev, stream)
        ("msnake_territory_actions", (0b100, a, 2, s, c, N), ARG, "msnake_territory_actions: snake_mask 0x4 has a bit >= n_snakes=2"),
        ("msnake_territory_actions", (0b101, N, 1, N, c + 1, N), ARG, "msnake_territory_actions: snake_mask 0x5 has a bit >= n_snakes=2"),
        ("msnake_territory_actions", (0, a, 2, N, N, N), ARG,
         "msnake_territory_actions: nothing to write (snake_mask 0, safe_dev and territory_dev are NULL)"),
        ("msnake_territory_actions", (0, N, 0, N, N, N), ARG,
         "msnake_territory_actions: nothing to write (snake_mask 0, safe_dev and territory_dev are NULL)"),
        ("msnake_territory_actions", (1, N, 2, s, c, N), ARG, "msnake_territory_actions: actions_dev is NULL"),
        ("msnake_territory_actions", (1, N, 1, s, c, N), ARG, "msnake_territory_actions: actions_dev is NULL"),  # the pointer first
        ("msnake_territory_actions", (1, N, 2, s, c + 1, N), ARG, "msnake_territory_actions: actions_dev is NULL"),
        ("msnake_territory_actions", (0b11, a, 1, s, c, N), ARG, "msnake_territory_actions: action_stride 1 must be >= n_snakes=2"),
        ("msnake_territory_actions", (0b11, a + 2, 0, s, c, N), ARG, "msnake_territory_actions: action_stride 0 must be >= n_snakes=2"),
        ("msnake_territory_actions", (0b11, a + 2, 2, s, c, N), ALIGN, "actions_dev must be 4-byte aligned"),
        ("msnake_territory_actions", (0b11, a + 2, 2, s, c + 1, N), ALIGN, "actions_dev must be 4-byte aligned"),
        ("msnake_territory_actions", (0b11, a, 2, s, c + 1, N), ALIGN, "territory_dev must be 2-byte aligned"),
        ("msnake_territory_actions", (0, N, 0, N, c + 1, N), ALIGN, "territory_dev must be 2-byte aligned"),
        # ---- msnake_render_cells(view_mask, cells_dev, snakes_dev, stream): snake_env has 3 views
        ("msnake_render_cells", (0b1000, ce, tb, N), ARG, "msnake_render_cells: view_mask 0x8 has a bit >= views=3"),
        ("msnake_render_cells", (0b1001, N, tb + 2, N), ARG, "msnake_render_cells: view_mask 0x9 has a bit >= views=3"),
        ("msnake_render_cells", (0b001, N, tb, N), ARG, "msnake_render_cells: cells_dev is NULL but view_mask is 0x1"),
        ("msnake_render_cells", (0b110, N, tb + 2, N), ARG, "msnake_render_cells: cells_dev is NULL but view_mask is 0x6"),
        ("msnake_render_cells", (0, ce, tb, N), ARG, "msnake_render_cells: cells_dev is given but view_mask is 0"),
        ("msnake_render_cells", (0, ce, N, N), ARG, "msnake_render_cells: cells_dev is given but view_mask is 0"),
        ("msnake_render_cells", (0, N, N, N), ARG, "msnake_render_cells: nothing to write (view_mask 0 and snakes_dev is NULL)"),
        ("msnake_render_cells", (0b111, ce, tb + 2, N), ALIGN, "snakes_dev must be 4-byte aligned"),
        ("msnake_render_cells", (0, N, tb + 1, N), ALIGN, "snakes_dev must be 4-byte aligned"),
        # ---- msnake_render_local(radius, snake_mask, oriented, windows_dev, heading_dev, stream)
        ("msnake_render_local", (0, 0b11, 1, w, hd, N), ARG, "msnake_render_local: radius 0 must lie in [1, 31]"),
        ("msnake_render_local", (32, 0b11, 1, w, hd, N), ARG, "msnake_render_local: radius 32 must lie in [1, 31]"),
        ("msnake_render_local", (-1, 0, 2, N, N, N), ARG, "msnake_render_local: radius -1 must lie in [1, 31]"),
        ("msnake_render_local", (1, 0, 1, w, hd, N), ARG, "msnake_render_local: snake_mask is 0 (no window to write)"),
        ("msnake_render_local", (1, 0, 2, N, N, N), ARG, "msnake_render_local: snake_mask is 0 (no window to write)"),
        ("msnake_render_local", (1, 0b100, 1, w, hd, N), ARG, "msnake_render_local: snake_mask 0x4 has a bit >= n_snakes=2"),
        ("msnake_render_local", (1, 0b111, 2, N, N, N), ARG, "msnake_render_local: snake_mask 0x7 has a bit >= n_snakes=2"),
        ("msnake_render_local", (1, 0b11, 2, w, hd, N), ARG, "msnake_render_local: oriented must be 0 or 1, got 2"),
        ("msnake_render_local", (1, 0b11, -1, N, N, N), ARG, "msnake_render_local: oriented must be 0 or 1, got -1"),
        ("msnake_render_local", (1, 0b11, 1, N, hd, N), ARG, "msnake_render_local: windows_dev is NULL"),
        # ---- msnake_reset_envs(mask_dev, obs_dev, final_obs_dev, truncated_dev, stream)
        ("msnake_reset_envs", (N, o, b.final.data_ptr(), b.trunc.data_ptr(), N), ARG,
         "msnake_reset_envs: mask_dev is NULL (msnake_reset resets every env)"),
        ("msnake_reset_envs", (N, N, N, N, N), ARG, "msnake_reset_envs: mask_dev is NULL (msnake_reset resets every env)"),
    ])
    # the NULL handle comes before everything else
    L = env._L
    for rc in (L.msnake_step(N, N, 0, N, N, N, N, N), L.msnake_rollout_tape(N, N, 0, 0, N, 0, N, N, N, 0, N),
               L.msnake_scripted_actions(N, 9, 0b100, N, 0, N, N), L.msnake_space_actions(N, 0b100, N, 0, N, N, N),
               L.msnake_territory_actions(N, 0b100, N, 0, N, N, N), L.msnake_render_cells(N, 0b1000, N, N, N),
               L.msnake_render_local(N, 0, 0, 2, N, N, N), L.msnake_reset_envs(N, N, N, N, N, N)):
        assert (rc, L.msnake_last_error().decode()) == (HANDLE, "invalid or destroyed msnake handle")
    # msnake_call_shape_for_config: the stride, and nothing but the stride (NULL and odd addresses are only looked at)
    for stride, want in ((1, stride1), (8, stride8), (0, "action_stride 0 must be in [n_snakes=2, 7]")):
        out = ctypes.c_int32(-7)
        rc = L.msnake_call_shape_for_config(ctypes.byref(env.cfg), stride, N, N, N, 4, ctypes.byref(out))
        assert (rc, L.msnake_last_error().decode(), out.value) == (ARG, want, -7)
    torch.cuda.synchronize()
    assert b.untouched()
    assert np.array_equal(env.get_state_all(), before)
    assert env.stats()["env_steps"] == 0
    env.close()


def test_hamiltonian_parity_refusal_and_its_place_among_the_checks():
    import torch
    env = _env(dim=5)
    b = Bufs(env, 2 * 7 * 7 * 9)
    before = env.get_state_all().copy()
    a, s, N = b.acts.data_ptr(), b.safe.data_ptr(), None
    parity = "msnake_scripted_actions: policy HAMILTONIAN needs an even dim (the cycle), got dim 5"
    _refused(env, [
        ("msnake_scripted_actions", (2, 0b11, a, 2, s, N), ARG, parity),
        ("msnake_scripted_actions", (2, 0, N, 0, s, N), ARG, parity),                 # even when only the mask would be written
        ("msnake_scripted_actions", (2, 0b01, N, 1, N, N), ARG, parity),              # before the pointer and the stride
        ("msnake_scripted_actions", (2, 0, N, 0, N, N), ARG, parity),                 # before "nothing to write"
        ("msnake_scripted_actions", (2, 0b01, a + 2, 2, N, N), ARG, parity),          # before the alignment
        ("msnake_scripted_actions", (2, 0b100, a, 2, s, N), ARG, "msnake_scripted_actions: snake_mask 0x4 has a bit >= n_snakes=2"),
        ("msnake_scripted_actions", (5, 0b100, a, 2, s, N), ARG, "msnake_scripted_actions: policy 5 is not one of MSNAKE_POLICY_*"),
    ])
    with pytest.raises(RuntimeError) as err:
        env.scripted_actions_device("hamiltonian")
    assert str(err.value) == "msnake_scripted_actions failed (-1): " + parity
    torch.cuda.synchronize()
    assert b.untouched()
    assert np.array_equal(env.get_state_all(), before)
    assert env.stats()["env_steps"] == 0
    env.close()


def test_observation_alignment_refusals_at_obs_scale_4():
    import torch
    env = _env(dim=4, obs_scale=4)
    assert env.obs_shape == (24, 24, 9)
    b = Bufs(env, 2 * 24 * 24 * 9)
    before = env.get_state_all().copy()
    a, r, d, i, o, f = (t.data_ptr() for t in (b.acts, b.rew, b.done, b.info, b.obs, b.final))
    m, tr, N = b.mask.data_ptr(), b.trunc.data_ptr(), None
    both = "obs_dev and final_obs_dev must be 4-byte aligned when obs_scale > 1"
    tape = "obs_dev and obs_step_stride must be multiples of 4 when obs_scale > 1"
    _refused(env, [
        ("msnake_step", (a, 2, o + 2, r, d, i, N), ALIGN, "obs_dev must be 4-byte aligned when obs_scale > 1"),
        ("msnake_step", (a, 2, o + 1, r, d, N, N), ALIGN, "obs_dev must be 4-byte aligned when obs_scale > 1"),
        ("msnake_step", (a + 2, 2, o + 2, r, d, i, N), ALIGN, "actions/rew must be 4-byte and info 16-byte aligned"),
        ("msnake_step", (a, 1, o + 2, r, d, i, N), ARG, "action_stride 1 must be in [n_snakes=2, 7]"),
        ("msnake_rollout_tape", (a, 2, 1, o + 2, 0, r, d, i, 0, N), ALIGN, tape),
        ("msnake_rollout_tape", (a, 2, 2, o, 10370, r, d, i, 2, N), ALIGN, tape),
        ("msnake_rollout_tape", (a, 2, 1, o + 2, 0, r + 2, d, i, 0, N), ALIGN, "actions/rew must be 4-byte and info 16-byte aligned"),
        ("msnake_rollout_tape", (N, 2, 1, o + 2, 0, r, d, i, 0, N), ARG, "msnake_rollout_tape: actions/rew/done must not be NULL"),
        ("msnake_reset_envs", (m, o + 2, f, tr, N), ALIGN, both),
        ("msnake_reset_envs", (m, o, f + 2, tr, N), ALIGN, both),      # both pointers are checked before the first launch
        ("msnake_reset_envs", (m, o + 1, N, N, N), ALIGN, both),
        ("msnake_reset_envs", (N, o + 2, f + 2, tr, N), ARG, "msnake_reset_envs: mask_dev is NULL (msnake_reset resets every env)"),
        ("msnake_reset", (o + 2, N), ALIGN, "obs_dev must be 4-byte aligned when obs_scale > 1"),
        ("msnake_render", (o + 2, N), ALIGN, "obs_dev must be 4-byte aligned when obs_scale > 1"),
        ("msnake_render", (N, N), ARG, "msnake_render: obs_dev is NULL"),
    ])
    torch.cuda.synchronize()
    assert b.untouched()
    assert np.array_equal(env.get_state_all(), before)
    assert env.stats()["env_steps"] == 0
    env.close()


def _bad_tensors(torch, device, shape, dtype):
    """What a caller's tensor of `shape` and `dtype` on `device` must not be: (what, tensor)."""
    other = {torch.uint8: torch.int8, torch.uint16: torch.int16, torch.int32: torch.int64}[dtype]
    mk = lambda shp, dt=dtype, dev=device: torch.zeros(shp, dtype=torch.int16 if dt == torch.uint16 else dt, device=dev).view(dt)
    wide = mk(shape[:-1] + (2 * shape[-1],))
    return [("dtype", mk(shape, other)), ("last extent", mk(shape[:-1] + (shape[-1] + 1,))), ("first extent", mk((shape[0] + 1,) + shape[1:])),
            ("rank", mk(shape + (1,))), ("not contiguous", wide[..., ::2]), ("device", mk(shape, dev="cpu")),
            ("no tensor", np.zeros(shape, np.uint8)), ("no tensor", 0)]


def test_python_tensor_checks_refuse_with_the_same_text():
    import torch
    env = _env(dim=4)
    dev = env.device
    before = env.get_state_all().copy()
    u8, u16, i32 = torch.uint8, torch.uint16, torch.int32
    good = lambda shape, dt: torch.zeros(shape, dtype=torch.int16 if dt == u16 else dt, device=dev).view(dt)
    acts, safe, cnt = good((2, 2), i32), good((2, 2), u8), good((2, 2, 4), u16)
    # site -> (the sentence, shape, dtype, the call with the bad tensor)
    obs_msg = "out must be a contiguous uint8 tensor of shape (2, 6, 6, 9) on cuda:0"
    sites = [
        (obs_msg, (2, 6, 6, 9), u8, lambda t: env.reset_device(out=t)),
        (obs_msg, (2, 6, 6, 9), u8, lambda t: env.reset_device(mask=[0], out=t)),
        (obs_msg, (2, 6, 6, 9), u8, lambda t: env.reset_device(mask=[0], final_out=t)),          # (final_out is named "out")
        (obs_msg, (2, 6, 6, 9), u8, lambda t: env.render_device(out=t)),
        (obs_msg, (2, 6, 6, 9), u8, lambda t: env.step_device(acts, out=t)),
        ("truncated_out must be a contiguous uint8 tensor of shape (2,) on cuda:0", (2,), u8,
         lambda t: env.reset_device(mask=[1], truncated_out=t)),
        ("safe_out must be a contiguous uint8 tensor of shape (2, 2) on cuda:0", (2, 2), u8,
         lambda t: env.scripted_actions_device("safe_greedy", safe_out=t)),
        ("safe_out must be a contiguous uint8 tensor of shape (2, 2) on cuda:0", (2, 2), u8,
         lambda t: env.scripted_actions_device("territory_greedy", safe_out=t)),
        ("safe_out must be a contiguous uint8 tensor of shape (2, 2) on cuda:0", (2, 2), u8, lambda t: env.safe_moves_device(out=t)),
        ("space_out must be a contiguous uint16 tensor of shape (2, 2, 4) on cuda:0", (2, 2, 4), u16,
         lambda t: env.scripted_actions_device("space_greedy", space_out=t)),
        ("space_out must be a contiguous uint16 tensor of shape (2, 2, 4) on cuda:0", (2, 2, 4), u16,
         lambda t: env.reachable_space_device(out=t)),
        ("territory_out must be a contiguous uint16 tensor of shape (2, 2, 4) on cuda:0", (2, 2, 4), u16,
         lambda t: env.scripted_actions_device("territory_greedy", territory_out=t)),
        ("territory_out must be a contiguous uint16 tensor of shape (2, 2, 4) on cuda:0", (2, 2, 4), u16,
         lambda t: env.territory_device(out=t)),
        ("snakes_out must be a contiguous int32 tensor of shape (2, 2, 8) on cuda:0", (2, 2, 8), i32,
         lambda t: env.render_cells_device(snakes_out=t)),
        ("snakes_out must be a contiguous int32 tensor of shape (2, 2, 8) on cuda:0", (2, 2, 8), i32,
         lambda t: env.render_cells_device(views=[], snakes_out=t)),
        ("out must be a contiguous uint8 tensor of shape (2, 3, 4, 4) on cuda:0", (2, 3, 4, 4), u8,
         lambda t: env.render_cells_device(out=t)),
        ("out must be a contiguous uint8 tensor of shape (2, 1, 4, 4) on cuda:0", (2, 1, 4, 4), u8,
         lambda t: env.render_cells_device(views=2, out=t, snakes=True)),
        ("out must be a contiguous uint8 tensor of shape (2, 2, 3, 3) on cuda:0", (2, 2, 3, 3), u8,
         lambda t: env.render_local_device(1, out=t)),
        ("out must be a contiguous uint8 tensor of shape (2, 1, 5, 5) on cuda:0", (2, 1, 5, 5), u8,
         lambda t: env.render_local_device(2, snakes=[1], oriented=False, out=t, heading=True)),
        ("heading_out must be a contiguous uint8 tensor of shape (2, 2) on cuda:0", (2, 2), u8,
         lambda t: env.render_local_device(1, heading_out=t)),
        ("heading_out must be a contiguous uint8 tensor of shape (2, 1) on cuda:0", (2, 1), u8,
         lambda t: env.render_local_device(3, snakes=0, heading_out=t)),
    ]
    for want, shape, dtype, call in sites:
        for what, bad in _bad_tensors(torch, dev, shape, dtype):
            with pytest.raises(ValueError) as err:
                call(bad)
            assert str(err.value) == want, (want, what, str(err.value))
    # the checks that sit next to them, and the order in which they fire
    bad_acts = good((2, 2), i32)[:, :1]
    for bad in (bad_acts, good((2, 1), i32), good((3, 2), i32), good((2, 2), u8), good((2, 2, 1), i32), good((2, 4), i32)[:, ::2],
                torch.zeros((2, 2), dtype=i32), np.zeros((2, 2), np.int32)):
        with pytest.raises(ValueError) as err:
            env.scripted_actions_device("safe_greedy", out=bad, safe_out=good((2, 3), u8))               # out before safe_out
        assert str(err.value) == "out must be a contiguous int32 tensor of shape (2, >= 2) on cuda:0"
    for pol, kw in (("space_greedy", "space_out"), ("territory_greedy", "territory_out")):
        with pytest.raises(ValueError) as err:
            env.scripted_actions_device(pol, out=acts, safe_out=good((2, 3), u8), **{kw: good((2, 2, 5), u16)})   # safe_out before the counts
        assert str(err.value) == "safe_out must be a contiguous uint8 tensor of shape (2, 2) on cuda:0"
        with pytest.raises(ValueError) as err:
            env.scripted_actions_device(pol, snakes=[2], out=bad_acts, **{kw: good((2, 2, 5), u16)})      # the snakes before any tensor
        assert str(err.value) == "snake indices must lie in [0, 2), got 2"
    with pytest.raises(ValueError) as err:
        env.scripted_actions_device("safe_greedy", space_out=cnt, territory_out=cnt)
    assert str(err.value) == "space_out is written by policy 'space_greedy' only, got policy 'safe_greedy'"
    with pytest.raises(ValueError) as err:
        env.scripted_actions_device("space_greedy", out=bad_acts, territory_out=cnt)
    assert str(err.value) == "territory_out is written by policy 'territory_greedy' only, got policy 'space_greedy'"
    with pytest.raises(ValueError) as err:
        env.scripted_actions_device("territory", out=bad_acts)
    assert str(err.value) == "policy must be 'safe_greedy', 'hamiltonian' or None, got 'territory'"
    with pytest.raises(ValueError) as err:
        env.render_cells_device(out=good((2, 3, 4, 5), u8), snakes_out=good((2, 2, 7), i32))             # the table before the planes
    assert str(err.value) == "snakes_out must be a contiguous int32 tensor of shape (2, 2, 8) on cuda:0"
    with pytest.raises(ValueError) as err:
        env.render_cells_device(views=[], out=good((2, 0, 4, 4), u8), snakes_out=good((2, 2, 8), i32))
    assert str(err.value) == "out is given but no view is selected"
    with pytest.raises(ValueError) as err:
        env.render_cells_device(views=[])
    assert str(err.value) == "nothing to write: no view is selected and no table is asked for (snakes=True / snakes_out)"
    with pytest.raises(ValueError) as err:
        env.render_local_device(1, out=good((2, 2, 3, 4), u8), heading_out=good((2, 3), u8))             # the windows before the heading
    assert str(err.value) == "out must be a contiguous uint8 tensor of shape (2, 2, 3, 3) on cuda:0"
    with pytest.raises(ValueError) as err:
        env.reset_device(mask=[0], final_out=good((2, 6, 6, 8), u8), truncated_out=good((3,), u8))       # final_out before the flags
    assert str(err.value) == obs_msg
    with pytest.raises(ValueError) as err:
        env.reset_device(out=good((2, 6, 6, 9), u8), truncated_out=good((2,), u8))
    assert str(err.value) == "final_out / truncated_out need a mask (a full reset has no terminal observations)"
    torch.cuda.synchronize()
    assert np.array_equal(env.get_state_all(), before)                  # no refused call reached the library
    assert env.stats()["env_steps"] == 0
    assert not acts.any() and not safe.any() and not cnt.view(torch.int16).any()
    env.close()
