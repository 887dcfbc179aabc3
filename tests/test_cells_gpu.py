"""The observation as cell codes on the device (msnake_render_cells) against the oracle's own picture.

Everything is bit-exact and nothing is left out of a comparison: every env, view and cell, every row of the table.  The
expected planes are cells_play.decode_frame of the ORACLE's frame (its `render`, or the frame its step returned) and the
expected rows the oracle's state, after Oracle.set_state with the same state dicts the handle got through
set_state_words; neither ever comes from the library under test.  Every output sits between 64 guard bytes of 0xA5 on
each side in a buffer pre-filled with 0xA5, which is not a code, and the guards are checked after every call.
"""
import ctypes

import numpy as np
import pytest

import cells_play as cp
import gpu_harness as gh
import scripted_play as sp

pytestmark = pytest.mark.gpu

_mk = gh.make_env


def Guarded(env, n_planes, offset=0):
    """A uint8 [n, V, dim, dim] plane buffer `cells` that starts `offset` bytes behind its 64 guard bytes (3 more bytes
    of slack behind the back guard) and an int32 [n, ns, 8] `table` between 64 guard words, all filled with 0xA5."""
    n, dim = env.num_envs, env.cells_shape[1]
    return gh.GuardedOutputs(env.device, {"cells": dict(dtype="uint8", shape=(n, n_planes, dim, dim), fill=0xA5, offset=offset, align=4, slack=3),
                                          "table": dict(dtype="int32", shape=(n, env.n_snakes, 8), fill=0xA5A5A5A5)})


def _n_views(env):
    return cp.n_views(env.cfg.rules, env.n_snakes)


def _want_rows(ora):
    read = sp._StateReader(ora)
    return np.stack([cp.np_snake_rows(read(e), ora.n_snakes) for e in range(ora.num_envs)])


def _check(env, ora, frames=None, views=None, buf=None, offset=0, table=True, what=""):
    """One call, compared for every env, selected view and cell and every row of the table against the oracle."""
    nv = _n_views(env)
    assert env.cells_shape == (nv, env.cfg.dim, env.cfg.dim)
    sel = list(range(nv)) if views is None else [views] if isinstance(views, int) else list(views)
    buf = buf or Guarded(env, len(sel), offset)
    want = cp.decode_frame(ora.render() if frames is None else frames, sel)
    res = env.render_cells_device(views=views, out=buf.cells, snakes_out=buf.table if table else None)
    assert (res[0] is buf.cells and res[1] is buf.table) if table else res is buf.cells
    got = buf.host("cells")
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "cells", bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    if table:
        got_r, want_r = buf.host("table"), _want_rows(ora)
        bad = np.argwhere(got_r != want_r)
        assert bad.size == 0, (what, "table", bad[:5].tolist(), got_r[bad[0][0]].tolist(), want_r[bad[0][0]].tolist())
    else:
        assert buf.untouched("table"), what
    assert buf.guards_intact(), what
    return buf


def _install(cfg, states, **kw):
    """The same state dicts into a fresh handle (set_state_words) and a fresh oracle (Oracle.set_state)."""
    return gh.install(cfg, states, with_oracle=True, **kw)


def _ragged(states):
    """No multiple of the kernel's four waves per workgroup: the waves of the batch tail return early."""
    return states[1:] if len(states) % 4 == 0 else states


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim", [2, 3, 6, 19, 33, 62])
def test_hand_built_snake_env_states(dim):
    """Border and corner heads, heads at -1 / dim, stacked duplicates, empty bodies, dense boards, bodies in the overflow
    ring (dim >= 19), a head under a later snake's body and fruits under bodies: the paint order decides the cell."""
    states = cp.snake_env_states(dim)
    states = _ragged(states)
    if dim >= 19:
        assert max(len(b) for st in states for b in st["snakes"]) > 64
    env, ora = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    buf = _check(env, ora, what=("snake_env", dim))
    first = len(states) - 8                                 # the first paint-order state, stated without the helper
    assert buf.host("cells")[first, :, 0, 0].tolist() == [4, 4, 2] and buf.host("table")[first, 0, :3].tolist() == [1, 0, 0]
    env.close()


@pytest.mark.parametrize("nf", [0, 9, 32])
@pytest.mark.parametrize("ns", [1, 2, 4])
@pytest.mark.parametrize("dim", [6, 13])
def test_hand_built_new_world_states(dim, ns, nf):
    """views = n_snakes; dead snakes whose bodies are kept (alive 0) vanish from every plane and stay in the table."""
    states = cp.new_world_states(dim, ns, nf)
    states = _ragged(states)
    assert sum(1 for st in states for s in range(ns) if not st["alive"][s] and st["snakes"][s]) >= 4
    env, ora = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    assert env.cells_shape[0] == ns
    buf = _check(env, ora, what=("new_world", dim, ns, nf))
    rows, planes = buf.host("table"), buf.host("cells")
    for e, st in enumerate(states):                         # the dead keep their rows; a board of the dead alone shows no snake
        assert rows[e, :, 6].tolist() == [int(a) for a in st["alive"]] and rows[e, :, 0].tolist() == [len(b) for b in st["snakes"]]
        if not any(st["alive"]):
            assert planes[e].max(initial=0) <= 1, e
    env.close()


def test_the_largest_block_new_world_62x62x4():
    """Four planes of 3 844 bytes per env: the largest block a wave composes (the kernel's LDS slice at its maximum)."""
    states = _ragged(cp.new_world_states(62, 4, 32)[::3])
    env, ora = _install(dict(rules=1, dim=62, n_snakes=4, n_fruits=32), states)
    assert env.cells_shape == (4, 62, 62) and max(len(b) for st in states for b in st["snakes"]) > 64
    for offset in (0, 3):
        _check(env, ora, offset=offset, what=("62x62x4", offset))
    env.close()


@pytest.mark.parametrize("dim,ns", [(10, 3), (6, 2)])
def test_hand_built_adversarial_states(dim, ns):
    """Fruit lists up to the list's capacity (past 64 entries: the strided part), entries outside the grid; with two
    snakes the frame still has three views, and in view 2 every snake is another's."""
    states = cp.adversarial_states(dim, ns)
    states = _ragged(states)
    assert max(len(st["fruits"]) for st in states) > 64
    env, ora = _install(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)
    assert env.cells_shape[0] == 3
    buf = _check(env, ora, what=("adversarial", dim, ns))
    if ns == 2:
        last = buf.host("cells")[:, 2]
        assert not ((last == 2) | (last == 3)).any() and (last == 5).any()
    env.close()


# ------------------------------------------------------------------------------------------ 2. view masks, outputs, offsets
@pytest.mark.parametrize("rules,dim,ns,nf", [(0, 19, 3, 3), (1, 13, 4, 9), (2, 10, 2, 2)])
def test_every_view_mask_table_only_and_cells_only(rules, dim, ns, nf):
    """Every non-empty view_mask (the planes are packed in ascending view order), an int, the table alone, the planes alone."""
    states = {0: cp.snake_env_states, 1: lambda d: cp.new_world_states(d, ns, nf), 2: lambda d: cp.adversarial_states(d, ns)}[rules](dim)
    states = states[-21:]
    env, ora = _install(dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=nf), states)
    nv = _n_views(env)
    for mask in range(1, 1 << nv):
        views = [v for v in range(nv) if (mask >> v) & 1]
        _check(env, ora, views=views, table=bool(mask & 1), what=(rules, "mask", mask))
    _check(env, ora, views=nv - 1, what=(rules, "int"))
    # the table alone: no plane byte is written
    buf = Guarded(env, 1)
    res = env.render_cells_device(views=[], snakes_out=buf.table)
    assert res is buf.table and np.array_equal(buf.host("table"), _want_rows(ora)) and buf.untouched("cells") and buf.guards_intact()
    # fresh tensors of the env's own
    cells, table = env.render_cells_device(snakes=True)
    assert tuple(cells.shape) == (len(states),) + env.cells_shape and tuple(table.shape) == (len(states), ns, 8)
    assert np.array_equal(cells.cpu().numpy(), cp.decode_frame(ora.render(), range(nv))) and np.array_equal(table.cpu().numpy(), _want_rows(ora))
    assert np.array_equal(env.render(mode="cells"), cells[0].cpu().numpy())
    assert env.render().shape == (len(states),) + env.obs_shape      # the default mode is still the RGB frames
    env.close()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("dim", [3, 19])
def test_odd_plane_sizes_at_every_byte_offset(dim, offset):
    """9- and 361-byte planes: the env blocks start at every alignment; the output base sits 0..3 bytes into an allocation."""
    states = cp.snake_env_states(dim)[-23:]
    env, ora = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    for views in (None, [1], [0, 2]):
        buf = _check(env, ora, views=views, offset=offset, table=False, what=(dim, offset, views))
        assert buf.cells.data_ptr() % 4 == offset
    env.close()


# ------------------------------------------------------------------------------------------ 3. play
def _play(cfg, steps, seed, **kw):
    """Oracle-matched random play; render_cells after every step against the frame the oracle's step returned (auto-reset
    frames included)."""
    import torch
    env, ora = _mk(cfg, **kw), sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    rng = np.random.default_rng(seed)
    buf = Guarded(env, _n_views(env), offset=1)
    _check(env, ora, frames=ora.obs, buf=buf, what="reset")
    episodes = 0
    for t in range(steps):
        act = rng.integers(0, 5, (cfg["num_envs"], cfg["n_snakes"])).astype(np.int32)
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        o_obs, o_rew, o_done, *_ = ora.step(act)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        buf.refill()
        _check(env, ora, frames=o_obs, buf=buf, what=t)
        episodes += int(o_done.sum())
    assert episodes > 0 and env.stats()["errors"] == 0
    env.close()


def test_play_of_1027_small_envs():
    _play(dict(rules=0, dim=6, n_snakes=3, n_fruits=3, num_envs=1027, seed=4, env_id_base=9, max_steps=2000), 60, 1)


@pytest.mark.parametrize("epb", [1, 8])
@pytest.mark.parametrize("record_policy", ["short", "full"])
def test_play_under_record_policies_and_envs_per_block(record_policy, epb):
    cfg = dict(rules=0, dim=19, n_snakes=3, n_fruits=3, num_envs=37, seed=6, env_id_base=0, max_steps=2000)
    _play(cfg, 60, epb, record_policy=record_policy, envs_per_block=epb)


# ------------------------------------------------------------------------------------------ 4. read-only
def test_the_call_changes_no_state():
    """State blob and statistics are identical around a call, and play continued afterwards matches the oracle (the Philox
    counter stays); interleaved with reset(mask), copy_envs_device and scripted_actions_device on one handle."""
    import torch
    n, ns, dim = 24, 3, 19
    cfg = dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=n, seed=8, env_id_base=2, max_steps=2000)
    env, ora = _mk(cfg, auto_reset=False), sp.make_oracle(cfg, auto_reset=False)
    assert np.array_equal(env.reset(), ora.reset())
    rng = np.random.default_rng(2)
    buf = Guarded(env, 3, offset=3)
    acts = torch.zeros((n, ns), dtype=torch.int32, device=env.device)
    snap = saved = None
    resets = 0
    for t in range(30):
        states = gh.oracle_states(ora)
        before, st_before = env.get_state_all().tobytes(), env.stats()
        buf.refill()
        _check(env, ora, buf=buf, what=("before", t))
        env.render_cells_device(views=[1]), env.render_cells_device(views=[], snakes=True)
        assert env.get_state_all().tobytes() == before and env.stats() == st_before, t
        # snakes 1 and 2 scripted on the device, snake 0 random; the oracle gets the helper's actions
        want = np.array([sp.safe_greedy(st, dim, ns, None) for st in states], np.int32)
        want[:, 0] = rng.integers(0, 5, n)
        acts[:, 0] = torch.from_numpy(want[:, 0]).to(env.device)
        env.scripted_actions_device("safe_greedy", snakes=[1, 2], out=acts)
        assert np.array_equal(acts.cpu().numpy(), want), t
        _, rew, done, _ = env.step_device(acts)
        _, o_rew, o_done, *_ = ora.step(want, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        if o_done.any():                                   # reset(mask): the finished envs, on both
            env.reset_device(mask=done)
            ora.reset_envs(o_done, obs=None, final_obs=None, truncated=None)
            resets += int(o_done.sum())
        if t == 9:                                          # snapshot (no env is finished: the ended ones were just reset)
            snap, saved = env.clone(), [ora.get_state(e) for e in range(n)]
        if t == 19:                                         # roll every env back to it
            env.copy_envs_device(snap)
            for e in range(n):
                ora.set_state(e, saved[e])
    buf.refill()
    _check(env, ora, buf=buf, what="end")
    assert resets > 0 and env.stats()["errors"] == 0 and env.stats()["env_steps"] == 30 * n   # the call adds nothing to env_steps
    snap.close(), env.close()


# ------------------------------------------------------------------------------------------ 5. HIP graph
def test_graph_of_step_then_render_cells():
    """[msnake_step -> msnake_render_cells] captured on one stream as a linear chain and replayed 5 times with fresh
    actions in the captured buffer: every replay's planes and table against the oracle."""
    import torch
    n, ns = 50, 3
    cfg = dict(rules=0, dim=19, n_snakes=ns, n_fruits=ns, num_envs=n, seed=3, env_id_base=0, max_steps=2000)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    buf = Guarded(env, 3, offset=1)
    acts = torch.ones((n, ns), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.step_device(acts)
        env.render_cells_device(out=buf.cells, snakes_out=buf.table)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step_device(acts)
        env.render_cells_device(out=buf.cells, snakes_out=buf.table)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    rng = np.random.default_rng(7)
    for k in range(5):
        act = rng.integers(0, 5, (n, ns)).astype(np.int32)
        acts.copy_(torch.from_numpy(act).to(env.device))
        buf.refill()
        g.replay()
        torch.cuda.synchronize()
        o_obs, o_rew, o_done, *_ = ora.step(act)
        assert np.array_equal(out[1].cpu().numpy(), o_rew) and np.array_equal(out[2].cpu().numpy(), o_done), k
        assert np.array_equal(buf.host("cells"), cp.decode_frame(o_obs, [0, 1, 2])), k
        assert np.array_equal(buf.host("table"), _want_rows(ora)), k
        assert buf.guards_intact(), k
    env.close()


# ------------------------------------------------------------------------------------------ 6. errors
def test_argument_errors_leave_the_outputs_untouched():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=2, rules="snake_env", seed=0)      # views 3, n_snakes 2
    nw = msnake.MultiSnakeVecEnv(5, dim=6, n_snakes=2, n_fruits=1, rules="new_world", seed=0)   # views 2
    env.reset(), nw.reset()
    L = env._L
    buf = Guarded(env, 3)
    pc, pt = buf.cells.data_ptr(), buf.table.data_ptr()

    def call(h, mask, c, t):
        rc = L.msnake_render_cells(h, mask, c, t, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 0b1000, pc, pt), "view_mask"), ((env._h, 0b1001, pc, None), "view_mask"),
                       ((nw._h, 0b100, pc, pt), "view_mask"),                     # new_world: views = n_snakes = 2
                       ((env._h, 0b101, None, pt), "cells_dev"), ((env._h, 1, None, None), "cells_dev"),
                       ((env._h, 0, pc, pt), "view_mask is 0"), ((env._h, 0, pc, None), "view_mask is 0"),
                       ((env._h, 0, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args[1:], rc, msg)
    for off in (1, 2, 3):
        rc, msg = call(env._h, 0b111, pc, pt + off)
        assert rc == -4 and "snakes_dev" in msg, (off, rc, msg)                  # MSNAKE_E_ALIGN
        rc, msg = call(env._h, 0, None, pt + off)
        assert rc == -4 and "snakes_dev" in msg, (off, rc, msg)
    rc, msg = call(None, 1, pc, pt)
    assert rc == -3 and "handle" in msg
    assert call(env._h, 0b1000, pc, pt)[0] == -1               # (another message in between)
    dead = ctypes.create_string_buffer(4)                      # what a destroyed handle looks like: the magic word is gone
    for args in ((dead, 0b111, pc, pt), (dead, 0, None, pt), (dead, 1, pc, None), (dead, 0b1000, None, None)):
        rc, msg = call(*args)
        assert rc == -3 and "handle" in msg, (args[1:], rc, msg)   # MSNAKE_E_HANDLE, before any argument check
    torch.cuda.synchronize()
    assert buf.untouched("cells") and buf.untouched("table")
    # the wrapper's own refusals, before the library is asked
    for kw in (dict(out=buf.cells[:, :2]), dict(out=buf.cells.to(torch.int8)), dict(views=[0], out=buf.cells),
               dict(snakes_out=buf.table[:, :1]), dict(snakes_out=buf.table.to(torch.int64)), dict(views=[]),
               dict(views=[], out=buf.cells), dict(views=[3]), dict(views=[1, 0]), dict(out=buf.cells.cpu())):
        with pytest.raises(ValueError):
            env.render_cells_device(**kw)
    torch.cuda.synchronize()
    assert buf.untouched("cells") and buf.untouched("table")
    # what is NOT an error: an unaligned cells_dev, and each output alone
    assert call(env._h, 0b010, pc + 1, None)[0] == 0 and call(env._h, 0, None, pt)[0] == 0 and call(env._h, 0b111, pc, None)[0] == 0
    torch.cuda.synchronize()
    assert buf.guards_intact() and env.stats()["env_steps"] == 0
    env.close(), nw.close()
