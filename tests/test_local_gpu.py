"""Head-centred cell-code windows on the device (msnake_render_local) against tests/local_play.py and the oracle.

Everything is bit-exact and nothing is left out of a comparison: every env, selected snake and window entry, every
heading.  The expected windows are local_play.np_local on the state dicts the handle was given (or on the ORACLE's state
after play), and in the closed loop also windows cut from cells_play.decode_frame of the oracle's frame; neither ever
comes from the library under test.  Every output sits between 64 guard bytes of 0xA5 on each side in a buffer pre-filled
with 0xA5, which is neither a code nor a heading, and the guards are checked after every call.
"""
import ctypes

import numpy as np
import pytest

import board_states as bs
import cells_play as cp
import gpu_harness as gh
import local_play as lp
import scripted_play as sp

pytestmark = pytest.mark.gpu

RADII = (1, 2, 5, 31)
_mk, _install = gh.make_env, gh.install


def Guarded(env, n_sel, radius, offset=0):
    """A uint8 [n, S, W, W] window buffer `win` that starts `offset` bytes behind its 64 guard bytes (3 more bytes of
    slack behind the back guard) and a uint8 [n, S] heading buffer `head` between 64 guard bytes, all filled with 0xA5."""
    n, w = env.num_envs, 2 * radius + 1
    return gh.GuardedOutputs(env.device, {"win": dict(dtype="uint8", shape=(n, n_sel, w, w), fill=0xA5, offset=offset, align=4, slack=3),
                                          "head": dict(dtype="uint8", shape=(n, n_sel), fill=0xA5)})


def _check(env, states, radius, snakes=None, oriented=True, offset=0, heading=True, planes=None, buf=None, what=""):
    """One call, compared for every env, selected snake and window entry and every heading against the helper."""
    ns, dim, rules = env.n_snakes, int(env.cfg.dim), int(env.cfg.rules)
    sel = list(range(ns)) if snakes is None else [snakes] if isinstance(snakes, int) else list(snakes)
    assert env.local_shape(radius, snakes) == (len(sel), 2 * radius + 1, 2 * radius + 1)
    buf = buf or Guarded(env, len(sel), radius, offset)
    want_w, want_h = lp.np_local_all(states, dim, ns, rules, sel, radius, oriented, planes=planes)
    res = env.render_local_device(radius, snakes=snakes, oriented=oriented, out=buf.win, heading_out=buf.head if heading else None)
    assert (res[0] is buf.win and res[1] is buf.head) if heading else res is buf.win
    got = buf.host("win")
    bad = np.argwhere(got != want_w)
    assert bad.size == 0, (what, "windows", bad[:5].tolist(), got[tuple(bad[0][:2])].tolist(), want_w[tuple(bad[0][:2])].tolist())
    if heading:
        got_h = buf.host("head")
        assert np.array_equal(got_h, want_h), (what, "heading", np.argwhere(got_h != want_h)[:5].tolist())
    else:
        assert buf.untouched("head"), what
    assert buf.guards_intact(), what
    return buf


def _ragged(states):
    """No multiple of the kernel's four waves per workgroup: the waves of the batch tail return early."""
    return states[1:] if len(states) % 4 == 0 else states


def _all_radii(env, states, radii=RADII, what=""):
    planes = lp.planes_all(states, int(env.cfg.dim), env.n_snakes, int(env.cfg.rules))
    for radius in radii:
        for oriented in (False, True):
            _check(env, states, radius, oriented=oriented, planes=planes, what=(what, radius, oriented))


# ------------------------------------------------------------------------------------------ 1. hand-built snake_env states
@pytest.mark.parametrize("dim", [2, 3, 6, 19, 33, 62])
def test_hand_built_snake_env_states(dim):
    """Border and corner heads, heads at -1 / dim (the centre of the window is 6), stacked duplicates, dense boards, empty
    bodies, every velocity on every kind of body; windows smaller and larger than the board."""
    states = cp.snake_env_states(dim) + [bs.state([[], [], []], [(0, 0), (dim - 1, 0), (1, 1)])]
    states = lp.deal_velocities(_ragged(states), 3)
    shares = lp.heading_shares(states, 3)
    assert min(shares) >= 1 / 8, shares
    assert any(not any(st["snakes"]) for st in states)                     # an env of empty bodies alone
    assert any(b and b[0][0] in (-1, dim) for st in states for b in st["snakes"])
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    _all_radii(env, states, what=("snake_env", dim))
    env.close()


# ------------------------------------------------------------------------------------------ 2. the other rule sets
@pytest.mark.parametrize("dim", [6, 10])
def test_hand_built_new_world_states(dim):
    """Four snakes; dead snakes whose bodies are kept vanish from every window, their own included, which stays centred
    on their head."""
    states = lp.deal_velocities(_ragged(cp.new_world_states(dim, 4, 5)), 4)
    dead = [(e, s) for e, st in enumerate(states) for s in range(4) if not st["alive"][s] and st["snakes"][s]]
    assert len(dead) >= 4 and {st["in_dead"][s] for e, st in enumerate(states) for s in range(4) if (e, s) in dead} == {False, True}
    env = _install(dict(rules=1, dim=dim, n_snakes=4, n_fruits=5), states)
    _all_radii(env, states, what=("new_world", dim))
    win = env.render_local_device(2).cpu().numpy()
    for e, s in dead:                                                     # stated without the helper: no own code in a dead snake's window
        assert not ((win[e, s] == 2) | (win[e, s] == 3)).any(), (e, s)
    env.close()


@pytest.mark.parametrize("dim", [6, 19])
def test_hand_built_adversarial_states(dim):
    """Fruit lists past 64 entries (the strided part of the list), entries at -1 and dim."""
    states = lp.deal_velocities(_ragged(cp.adversarial_states(dim, 3)), 3)
    assert max(len(st["fruits"]) for st in states) > 64
    assert any(f[0] in (-1, dim) or f[1] in (-1, dim) for st in states for f in st["fruits"])
    env = _install(dict(rules=2, dim=dim, n_snakes=3, n_fruits=3), states)
    _all_radii(env, states, what=("adversarial", dim))
    env.close()


# ------------------------------------------------------------------------------------------ 3. overflow ring
@pytest.mark.parametrize("dim", [19, 20])
def test_pieces_in_the_overflow_ring_inside_the_window(dim):
    """Bodies over 64 cells whose pieces >= 64 lie next to the head: they show in the radius-5 window."""
    states, _ = bs.overflow_states(dim, 3)
    states = lp.deal_velocities(_ragged(states), 3, start=1)
    near = 0
    for st in states:
        for b in st["snakes"]:
            near += any(max(abs(c[0] - b[0][0]), abs(c[1] - b[0][1])) <= 5 for c in b[64:])
    assert near >= 6, near
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    _all_radii(env, states, radii=(1, 5, 31), what=("overflow", dim))
    # without the pieces >= 64 the windows would differ: the test sees them
    cut = [dict(st, snakes=[b[:64] for b in st["snakes"]]) for st in states]
    a = lp.np_local_all(states, dim, 3, 0, [0], 5, True)[0]
    b = lp.np_local_all(cut, dim, 3, 0, [0], 5, True)[0]
    assert (a != b).any(axis=(1, 2, 3)).sum() >= 6
    env.close()


# ------------------------------------------------------------------------------------------ 4. closed loop
@pytest.mark.parametrize("name,steps", [("S19x3", 150), ("A10x3", 150), ("N10x4", 100)])
def test_closed_loop_with_the_oracle_as_master(name, steps):
    """Scenario play of 8 envs; after every step the windows and headings of every snake against np_local on the oracle's
    state, every 10th step also against windows cut from the decoded frame the oracle's step returned."""
    import torch
    cfg = dict(sp.SCENARIOS[name], num_envs=8)
    ns, dim = cfg["n_snakes"], cfg["dim"]
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    rs = sp.policy_rng(cfg)
    buf = Guarded(env, ns, 5, offset=1)
    seen = set()
    for t in range(steps):
        act = sp.choose_actions(cfg, gh.oracle_states(ora), rs)
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        o_obs, o_rew, o_done, *_ = ora.step(act)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        states = gh.oracle_states(ora)
        buf.refill()
        _check(env, states, 5, buf=buf, what=(name, t))
        seen |= set(buf.host("head").ravel().tolist())
        if t % 10 == 0 or t == steps - 1:
            want = lp.windows_from_planes(cp.decode_frame(o_obs, list(range(ns))), states, list(range(ns)), 5, True)
            assert np.array_equal(buf.host("win"), want), (name, t, "frame")
    assert seen == {0, 1, 2, 3} and env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 5. selection and address phase
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_snake_masks_at_every_byte_offset(offset):
    """121-byte windows: the env blocks start at every alignment, and the output base sits 0..3 bytes into an allocation.
    The windows of a selection are compact and in ascending snake order; heading_dev NULL and non-NULL."""
    states = lp.deal_velocities(cp.snake_env_states(19)[-23:], 3)
    env = _install(dict(rules=0, dim=19, n_snakes=3, n_fruits=3), states)
    planes = lp.planes_all(states, 19, 3, 0)
    for snakes in ([0, 2], [1], None, 2):
        for heading in (True, False):
            for radius, oriented in ((5, True), (1, False), (2, True)):
                buf = _check(env, states, radius, snakes=snakes, oriented=oriented, offset=offset, heading=heading, planes=planes,
                             what=(offset, snakes, heading, radius))
                assert buf.win.data_ptr() % 4 == offset
    env.close()


def test_snake_masks_under_new_world_with_four_snakes():
    states = lp.deal_velocities(_ragged(cp.new_world_states(10, 4, 5)), 4, start=3)
    env = _install(dict(rules=1, dim=10, n_snakes=4, n_fruits=5), states)
    planes = lp.planes_all(states, 10, 4, 1)
    for snakes in ([3], [0, 3], 3):
        for offset in (0, 1, 2, 3):
            _check(env, states, 5, snakes=snakes, offset=offset, heading=offset % 2 == 0, planes=planes, what=(snakes, offset))
    env.close()


def test_the_largest_shape_62x62x4_radius_31():
    """Four 63 x 63 windows per env over a 62 x 62 board: the kernel's LDS slice and its block of output at their maximum."""
    states = lp.deal_velocities(_ragged(cp.new_world_states(62, 4, 32)[::3]), 4)
    env = _install(dict(rules=1, dim=62, n_snakes=4, n_fruits=32), states)
    assert env.local_shape(31) == (4, 63, 63) and max(len(b) for st in states for b in st["snakes"]) > 64
    planes = lp.planes_all(states, 62, 4, 1)
    for offset in (0, 3):
        _check(env, states, 31, offset=offset, planes=planes, what=("62x62x4", offset))
    env.close()


# ------------------------------------------------------------------------------------------ 6. layout
@pytest.mark.parametrize("record_policy", ["full", "short"])
@pytest.mark.parametrize("n", [1, 3, 37, 257])
def test_batch_sizes_record_policies_and_envs_per_block(n, record_policy):
    for epb in (1, 4, 8):
        cfg = dict(rules=0, dim=19, n_snakes=3, n_fruits=3, num_envs=n, seed=6 + epb, env_id_base=2, max_steps=2000)
        env, ora = _mk(cfg, record_policy=record_policy, envs_per_block=epb), sp.make_oracle(cfg)
        assert np.array_equal(env.reset(), ora.reset())
        gh.play_random(env, ora, 12, np.random.default_rng(epb))
        states = gh.oracle_states(ora)
        _check(env, states, 5, what=(n, record_policy, epb))
        _check(env, states, 2, snakes=[0, 2], oriented=False, offset=3, what=(n, record_policy, epb, "r2"))
        env.close()


# ------------------------------------------------------------------------------------------ 7. read-only
def test_the_call_changes_no_state():
    """Twin handles play the same 100 random steps; one also renders windows every step.  State blob and statistics are
    equal afterwards, and the calls added nothing to env_steps."""
    import torch
    n, ns = 24, 3
    cfg = dict(rules=0, dim=19, n_snakes=ns, n_fruits=ns, num_envs=n, seed=8, env_id_base=2, max_steps=2000)
    env, twin = _mk(cfg), _mk(cfg)
    env.reset(), twin.reset()
    rng = np.random.default_rng(2)
    buf = Guarded(env, ns, 5, offset=2)
    for t in range(100):
        act = torch.from_numpy(rng.integers(0, 5, (n, ns)).astype(np.int32)).to(env.device)
        env.step_device(act), twin.step_device(act)
        env.render_local_device(5, out=buf.win, heading_out=buf.head)
        env.render_local_device(31, snakes=[1], oriented=False)
    assert env.get_state_all().tobytes() == twin.get_state_all().tobytes()
    st = env.stats()
    assert st == twin.stats() and st["env_steps"] == 100 * n and st["errors"] == 0 and st["episodes"] > 0
    assert buf.guards_intact()
    env.close(), twin.close()


# ------------------------------------------------------------------------------------------ 8. HIP graph
def test_graph_of_step_then_render_local():
    """[msnake_step -> msnake_render_local] captured on one stream as a linear chain and replayed 100 times on 64 envs with
    fresh actions in the captured buffer; the final windows, headings and state against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    n, ns = 64, 3
    cfg = dict(rules=0, dim=19, n_snakes=ns, n_fruits=ns, num_envs=n, seed=3, env_id_base=0, max_steps=2000)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    buf = Guarded(env, ns, 5, offset=1)
    acts = torch.ones((n, ns), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.step_device(acts)
        env.render_local_device(5, out=buf.win, heading_out=buf.head)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step_device(acts)
        env.render_local_device(5, out=buf.win, heading_out=buf.head)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    rng = np.random.default_rng(7)
    for k in range(100):
        act = rng.integers(0, 5, (n, ns)).astype(np.int32)
        acts.copy_(torch.from_numpy(act).to(env.device))
        if k == 99:
            buf.refill()
        g.replay()
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        if k % 20 == 19:
            assert np.array_equal(out[1].cpu().numpy(), o_rew) and np.array_equal(out[2].cpu().numpy(), o_done), k
    torch.cuda.synchronize()
    states = gh.oracle_states(ora)
    want_w, want_h = lp.np_local_all(states, 19, ns, 0, range(ns), 5, True)
    assert np.array_equal(buf.host("win"), want_w) and np.array_equal(buf.host("head"), want_h) and buf.guards_intact()
    for e in range(n):
        got = flat_to_state(env.get_state_words(e))
        for key in ("snakes", "fruits", "vels", "t"):
            assert got[key] == states[e][key], (e, key)
    env.close()


# ------------------------------------------------------------------------------------------ 9. errors
def test_argument_errors_leave_the_outputs_untouched():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=2, rules="snake_env", seed=0)
    env.reset()
    L = env._L
    buf = Guarded(env, 2, 5)
    pw, ph = buf.win.data_ptr(), buf.head.data_ptr()

    def call(h, radius, mask, oriented, w, hd):
        rc = L.msnake_render_local(h, radius, mask, oriented, w, hd, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((0, 0b11, 1, pw, ph), "radius"), ((32, 0b11, 1, pw, ph), "radius"), ((-1, 0b11, 1, pw, None), "radius"),
                       ((5, 0, 1, pw, ph), "snake_mask"), ((5, 0b100, 1, pw, ph), "snake_mask"), ((5, 0b111, 0, pw, None), "snake_mask"),
                       ((5, 0b11, 2, pw, ph), "oriented"), ((5, 0b11, -1, pw, ph), "oriented"),
                       ((5, 0b11, 1, None, ph), "windows_dev"), ((5, 0b01, 0, None, None), "windows_dev")):
        rc, msg = call(env._h, *args)
        assert rc == -1 and word in msg and "msnake_render_local" in msg, (args, rc, msg)     # MSNAKE_E_ARG
    rc, msg = call(None, 5, 0b11, 1, pw, ph)
    assert rc == -3 and "handle" in msg                                            # MSNAKE_E_HANDLE
    dead = ctypes.create_string_buffer(4)                      # what a destroyed handle looks like: the magic word is gone
    for args in ((5, 0b11, 1, pw, ph), (0, 0, 2, None, None)):
        rc, msg = call(dead, *args)
        assert rc == -3 and "handle" in msg, (args, rc, msg)                       # before any argument check
    torch.cuda.synchronize()
    assert buf.untouched("win") and buf.untouched("head")
    # the wrapper's own refusals, before the library is asked
    for kw in (dict(radius=0), dict(radius=32), dict(radius=2.5), dict(snakes=[]), dict(snakes=[2]), dict(snakes=[1, 0]),
               dict(oriented=2), dict(oriented=None), dict(out=buf.win[:, :1]), dict(out=buf.win.to(torch.int8)),
               dict(out=buf.win.cpu()), dict(out=buf.win[:4]), dict(out=buf.win, snakes=[0]), dict(out=buf.win.transpose(2, 3)),
               dict(heading_out=buf.head[:, :1]), dict(heading_out=buf.head.to(torch.int32)), dict(heading_out=buf.head.cpu()),
               dict(heading_out=buf.head, snakes=1, out=None)):
        with pytest.raises(ValueError) as err:
            env.render_local_device(**dict(dict(radius=5, out=buf.win), **kw))
        name = {"snakes": "snake"}.get(next(iter(kw)), next(iter(kw)))     # (the argument the message must name)
        assert name in str(err.value), (kw, str(err.value))
    torch.cuda.synchronize()
    assert buf.untouched("win") and buf.untouched("head")
    # what is NOT an error: an unaligned windows_dev, heading_dev NULL, fresh tensors of the env's own
    assert call(env._h, 5, 0b10, 0, pw + 1, None)[0] == 0 and call(env._h, 1, 0b11, 1, pw, ph)[0] == 0
    win, head = env.render_local_device(1, heading=True)
    assert tuple(win.shape) == (5, 2, 3, 3) and tuple(head.shape) == (5, 2) and win.dtype == head.dtype == torch.uint8
    assert env.render_local_device(2, snakes=1).shape == (5, 1, 5, 5)
    torch.cuda.synchronize()
    assert buf.guards_intact() and env.stats()["env_steps"] == 0
    env.close()
