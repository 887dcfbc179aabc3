"""Eight-direction rays on the device (msnake_render_rays) against tests/rays_play.py and the oracle.

Everything is bit-exact and nothing is left out of a comparison: every env, selected snake, direction and channel, every
heading.  The expected rays are rays_play.np_rays on the state dicts the handle was given (or on the ORACLE's state after
play); they never come from the library under test.  One cross-check needs no CPU reference at all: the rays equal what
rays_play.rays_from_window reads off the library's own radius-31 windows.  Every output sits between 64 guard bytes of
0xA5 on each side in a buffer pre-filled with 0xA5, which is neither a distance (<= 63) nor a heading, and the guards
are checked after every call.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import gpu_harness as gh
import local_play as lp
import rays_play as rp
import scripted_play as sp

pytestmark = pytest.mark.gpu

FILL = 0xA5
_mk = gh.make_env


class _Sets:
    """rays_play's builder sets by name, each built on first use."""

    def __getitem__(self, name):
        return rp.builder_set(name)

    def __iter__(self):
        return iter(rp.SET_NAMES)


SETS = _Sets()


def Guarded(env, n_sel):
    """A uint8 [n, S, 8, 4] ray buffer `rays` (4-byte aligned) and a uint8 [n, S] heading buffer `head`, each between 64
    guard bytes, all filled with 0xA5."""
    n = env.num_envs
    buf = gh.GuardedOutputs(env.device, {"rays": dict(dtype="uint8", shape=(n, n_sel, 8, 4), fill=FILL, align=4),
                                         "head": dict(dtype="uint8", shape=(n, n_sel), fill=FILL)})
    assert buf.rays.data_ptr() % 4 == 0
    return buf


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(unoriented rays, oriented rays, headings) of every snake of a builder set: computed once, never changed."""
    _, rules, dim, ns, _, states = SETS[name]
    planes = lp.planes_all(states, dim, ns, rules)
    un, head = rp.np_rays_all(states, dim, ns, rules, range(ns), False, planes)
    orr, _ = rp.np_rays_all(states, dim, ns, rules, range(ns), True, planes)
    for a in (un, orr, head):
        a.setflags(write=False)
    return un, orr, head


def _compare(env, want_rays, want_head, snakes, oriented, heading=True, buf=None, what=""):
    """One call, compared for every env, selected snake, direction and channel and every heading."""
    sel = list(range(env.n_snakes)) if snakes is None else [snakes] if isinstance(snakes, int) else list(snakes)
    assert env.rays_shape(snakes) == (len(sel), 8, 4)
    buf = buf or Guarded(env, len(sel))
    res = env.render_rays_device(snakes=snakes, oriented=oriented, out=buf.rays, heading_out=buf.head if heading else None)
    assert (res[0] is buf.rays and res[1] is buf.head) if heading else res is buf.rays
    got = buf.host("rays")
    bad = np.argwhere(got != want_rays)
    assert bad.size == 0, (what, "rays", bad[:5].tolist(), got[tuple(bad[0][:2])].tolist(), want_rays[tuple(bad[0][:2])].tolist())
    if heading:
        got_h = buf.host("head")
        assert np.array_equal(got_h, want_head), (what, "heading", np.argwhere(got_h != want_head)[:5].tolist())
    else:
        assert buf.untouched("head"), what
    assert buf.guards_intact(), what
    return buf


def _install(name, **kw):
    """The builder set's states into a fresh handle, one env per state."""
    _, rules, dim, ns, nf, states = SETS[name]
    return gh.install(dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=nf), states, **kw)


def _masks(ns):
    return [[s for s in range(ns) if (m >> s) & 1] for m in range(1, 1 << ns)]


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("name", list(SETS))
def test_hand_built_states_every_mask_orientation_and_record_policy(name):
    """snake_env at dim 2, 5, 19, 33 (past the 32-column mark) and 62 (the last lane), new_world with dead snakes and 32
    fruits, adversarial with lists past 64 entries and entries off the grid: every non-empty snake_mask, both `oriented`
    values, heading_dev given and NULL, the full and the short record where the rule set has both."""
    _, rules, dim, ns, _, states = SETS[name]
    assert 48 <= len(states) <= 97
    un, orr, head = _reference(name)
    for record_policy in (("full", "short") if rules != 1 else ("auto",)):
        env = _install(name, record_policy=record_policy)
        for k, sel in enumerate(_masks(ns)):
            for oriented in (False, True):
                want = (orr if oriented else un)[:, sel]
                for heading in (True, False):
                    snakes = sel[0] if len(sel) == 1 and k % 2 else sel        # (an int selects like a one-element list)
                    _compare(env, want, head[:, sel], snakes, oriented, heading, what=(name, record_policy, sel, oriented, heading))
        _compare(env, orr, head, None, True, what=(name, record_policy, "default"))
        env.close()


# ------------------------------------------------------------------------------------------ 2. in play
@pytest.mark.parametrize("dim,ns,compiled", [(19, 3, True), (10, 1, True), (12, 2, False)])
def test_space_greedy_play_followed_on_the_oracle(dim, ns, compiled):
    """64 envs, 200 steps of the device's space_greedy (every fourth step random, so that episodes end) on the kernels
    compiled for the shape and on the generic ones; the oracle takes the same actions, and every 10 steps the rays of every
    snake are compared with np_rays on the oracle's state."""
    import torch
    n = 64
    cfg = dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=n, seed=5, env_id_base=3, max_steps=2000)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    if os.environ.get("MSNAKE_GENERIC_KERNELS", "") in ("", "0"):   # (the switch puts every handle on the generic kernels)
        assert (env.kernel_name().count(",") == 4) == compiled, env.kernel_name()
    assert np.array_equal(env.reset(), ora.reset())
    rng = np.random.default_rng(dim)
    buf = Guarded(env, ns)
    nonzero = np.zeros(4, np.int64)
    for t in range(200):
        if t % 4 == 3:
            act = rng.integers(0, 5, (n, ns)).astype(np.int32)
        else:
            act = env.scripted_actions_device("space_greedy").cpu().numpy().copy()
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        if t % 10 == 9:
            states = gh.oracle_states(ora)
            oriented = t % 20 == 9
            want, want_h = rp.np_rays_all(states, dim, ns, 0, range(ns), oriented)
            buf.refill()
            _compare(env, want, want_h, None, oriented, buf=buf, what=(dim, ns, t))
            nonzero += (want != 0).sum(axis=(0, 1, 2))
    assert nonzero[rp.WALL] > 0 and nonzero[rp.FRUIT] > 0 and nonzero[rp.OWN] > 0 and (ns == 1 or nonzero[rp.OTHER] > 0)
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 3. against the library's own windows
@pytest.mark.parametrize("name", ["S19x3", "N6x4f4", "A10x3"])
def test_rays_equal_the_rays_read_off_render_local_31(name):
    """On one handle, for dim <= 30: the header's second identity, with no CPU reference of the board in it."""
    env = _install(name)
    for oriented in (False, True):
        win = env.render_local_device(31, oriented=oriented).cpu().numpy()
        got = env.render_rays_device(oriented=oriented).cpu().numpy()
        want = rp.rays_from_windows(win)
        assert np.array_equal(got, want), (name, oriented, np.argwhere(got != want)[:5].tolist())
        assert (got[..., rp.WALL] >= 1).sum() > 0 and (got[..., 1:] != 0).sum() > 100
    env.close()


# ------------------------------------------------------------------------------------------ 4. read-only
def test_the_call_changes_no_state():
    """State blob and statistics are identical before and after the calls, and the next step's outputs equal those of a
    twin handle that never rendered rays."""
    import torch
    n, ns = 24, 3
    cfg = dict(rules=0, dim=19, n_snakes=ns, n_fruits=ns, num_envs=n, seed=8, env_id_base=2, max_steps=2000)
    env, twin = _mk(cfg), _mk(cfg)
    env.reset(), twin.reset()
    rng = np.random.default_rng(2)
    buf = Guarded(env, ns)
    for t in range(30):
        act = torch.from_numpy(rng.integers(0, 5, (n, ns)).astype(np.int32)).to(env.device)
        env.step_device(act), twin.step_device(act)
    blob, stats = env.get_state_all().tobytes(), env.stats()
    env.render_rays_device(out=buf.rays, heading_out=buf.head)
    env.render_rays_device(snakes=[1], oriented=False)
    assert env.get_state_all().tobytes() == blob == twin.get_state_all().tobytes()
    assert env.stats() == stats == twin.stats() and stats["env_steps"] == 30 * n and stats["errors"] == 0
    for t in range(20):
        act = torch.from_numpy(rng.integers(0, 5, (n, ns)).astype(np.int32)).to(env.device)
        env.render_rays_device(out=buf.rays, heading_out=buf.head)
        a, b = env.step_device(act), twin.step_device(act)
        for x, y in zip(a, b):
            assert torch.equal(x, y), t
    assert env.get_state_all().tobytes() == twin.get_state_all().tobytes() and env.stats() == twin.stats()
    assert buf.guards_intact()
    env.close(), twin.close()


# ------------------------------------------------------------------------------------------ 5. HIP graph
def test_graph_of_step_then_render_rays():
    """[msnake_step -> msnake_render_rays] captured on one stream and replayed three times with fresh actions in the
    captured buffer; after every replay the outputs equal those of an eager twin."""
    import torch
    n, ns = 64, 3
    cfg = dict(rules=0, dim=19, n_snakes=ns, n_fruits=ns, num_envs=n, seed=3, env_id_base=0, max_steps=2000)
    env, twin = _mk(cfg), _mk(cfg)
    env.reset(), twin.reset()
    blob = env.get_state_all()
    buf = Guarded(env, ns)
    acts = torch.ones((n, ns), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.step_device(acts)
        env.render_rays_device(out=buf.rays, heading_out=buf.head)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step_device(acts)
        env.render_rays_device(out=buf.rays, heading_out=buf.head)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    rng = np.random.default_rng(7)
    for k in range(3):
        act = torch.from_numpy(rng.integers(1, 5, (n, ns)).astype(np.int32)).to(env.device)
        acts.copy_(act)
        buf.refill()
        g.replay()
        e_out = twin.step_device(act)
        e_rays, e_head = twin.render_rays_device(heading=True)
        torch.cuda.synchronize()
        assert torch.equal(out[1], e_out[1]) and torch.equal(out[2], e_out[2]), k
        assert np.array_equal(buf.host("rays"), e_rays.cpu().numpy()) and np.array_equal(buf.host("head"), e_head.cpu().numpy()), k
        assert buf.guards_intact() and (buf.host("rays")[..., rp.WALL] >= 1).mean() > 0.5   # (a snake that died has no rays)
    assert env.get_state_all().tobytes() == twin.get_state_all().tobytes()
    env.close(), twin.close()


# ------------------------------------------------------------------------------------------ 6. errors
def test_argument_errors_leave_the_outputs_untouched():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=2, rules="snake_env", seed=0)
    env.reset()
    L = env._L
    buf = Guarded(env, 2)
    pr, ph = buf.rays.data_ptr(), buf.head.data_ptr()

    def call(h, mask, oriented, r, hd):
        rc = L.msnake_render_rays(h, mask, oriented, r, hd, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((0, 1, pr, ph), "snake_mask"), ((0b100, 1, pr, ph), "snake_mask"), ((0b111, 0, pr, None), "snake_mask"),
                       ((0b11, 2, pr, ph), "oriented"), ((0b11, -1, pr, ph), "oriented"),
                       ((0b11, 1, None, ph), "rays_dev"), ((0b01, 0, None, None), "rays_dev")):
        rc, msg = call(env._h, *args)
        assert rc == -1 and word in msg and "msnake_render_rays" in msg, (args, rc, msg)     # MSNAKE_E_ARG
    for off in (1, 2, 3):
        rc, msg = call(env._h, 0b11, 1, pr + off, ph)
        assert rc == -4 and "rays_dev" in msg and "aligned" in msg, (off, rc, msg)            # MSNAKE_E_ALIGN
    rc, msg = call(None, 0b11, 1, pr, ph)
    assert rc == -3 and "handle" in msg                                                        # MSNAKE_E_HANDLE
    dead = ctypes.create_string_buffer(4)                      # what a destroyed handle looks like: the magic word is gone
    for args in ((0b11, 1, pr, ph), (0, 2, None, None)):
        rc, msg = call(dead, *args)
        assert rc == -3 and "handle" in msg, (args, rc, msg)                                   # before any argument check
    torch.cuda.synchronize()
    assert buf.untouched("rays") and buf.untouched("head")
    # the wrapper's own refusals, before the library is asked
    odd = torch.full((5 * 2 * 32 + 4,), FILL, dtype=torch.uint8, device=env.device)[1:1 + 5 * 2 * 32].view(5, 2, 8, 4)
    for kw in (dict(snakes=[]), dict(snakes=[2]), dict(snakes=[1, 0]), dict(oriented=2), dict(oriented=None),
               dict(out=buf.rays[:, :1]), dict(out=buf.rays.to(torch.int8)), dict(out=buf.rays.cpu()), dict(out=buf.rays[:4]),
               dict(out=buf.rays, snakes=[0]), dict(out=buf.rays.transpose(2, 3)), dict(out=odd),
               dict(heading_out=buf.head[:, :1]), dict(heading_out=buf.head.to(torch.int32)), dict(heading_out=buf.head.cpu()),
               dict(heading_out=buf.head, snakes=1, out=None)):
        with pytest.raises(ValueError) as err:
            env.render_rays_device(**dict(dict(out=buf.rays), **kw))
        name = {"snakes": "snake"}.get(next(iter(kw)), next(iter(kw)))     # (the argument the message must name)
        assert name in str(err.value), (kw, str(err.value))
    torch.cuda.synchronize()
    assert buf.untouched("rays") and buf.untouched("head") and (odd.cpu().numpy() == FILL).all()
    # what is NOT an error: heading_dev NULL or unaligned, fresh tensors of the env's own
    assert call(env._h, 0b10, 0, pr, None)[0] == 0 and call(env._h, 0b01, 1, pr, ph + 1)[0] == 0
    rays, head = env.render_rays_device(heading=True)
    assert tuple(rays.shape) == (5, 2, 8, 4) and tuple(head.shape) == (5, 2) and rays.dtype == head.dtype == torch.uint8
    assert env.render_rays_device(snakes=1).shape == (5, 1, 8, 4)
    torch.cuda.synchronize()
    assert buf.guards_intact() and env.stats()["env_steps"] == 0
    env.close()
