"""Reachable-space counts and the flood-fill opponent on the device (msnake_space_actions) against tests/space_play.py.

Everything is bit-exact and nothing is left out of a comparison: every env, snake and move.  The expected counts are
space_play.np_space, the expected actions space_play.space_greedy with eps = 0, the expected mask
scripted_play.np_safe_mask, all on the canonical state of the CPU oracle or on a hand-built state dict; none of them
ever comes from the library under test.  Every output sits between guard elements.
"""

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import scripted_play as sp
import space_play as spp

pytestmark = pytest.mark.gpu

FILL = -77  # the sentinel of the action buffer (gpu_harness.action_spec)
_st, _mk, _states, _install = bs.state, gh.make_env, gh.oracle_states, gh.install


# ------------------------------------------------------------------------------------------ expectations
def expected(states, dim, ns):
    """(actions int32 [E, ns], masks uint8 [E, ns], counts uint16 [E, ns, 4]) of the helpers on canonical state dicts."""
    act = np.array([spp.space_greedy(st, dim, ns) for st in states], np.int32).reshape(len(states), ns)
    mask = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(len(states), ns)
    space = np.array([spp.np_space(st, dim, ns) for st in states]).reshape(len(states), ns, 4)
    assert space.max(initial=0) <= 62 * 62 - 1
    # the three statements agree with each other: a move is open iff its count is not 0, and the action is an open move
    assert np.array_equal(space > 0, (mask[:, :, None] >> np.arange(1, 5)) & 1 == 1)
    return act, mask, space.astype(np.uint16)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, policy="space_greedy", **kw)


def Guarded(env, stride=None):
    """Actions, mask and a uint16 [n, ns, 4] count buffer `space`, each between guard elements."""
    return gh.GuardedOutputs(env.device, dict(gh.action_spec(env, stride), **gh.count_spec(env, "space")))


def _check_call(env, states, buf=None, what=""):
    """One call with all three outputs, compared for every env, snake and move; returns the expected actions."""
    dim, ns = env.cfg.dim, env.n_snakes
    buf = buf or Guarded(env)
    want_a, want_m, want_c = expected(states, dim, ns)
    out, safe, space = env.scripted_actions_device("space_greedy", out=buf.act, safe_out=buf.safe, space_out=buf.space)
    got_a, got_m, got_c = out.cpu().numpy()[:, :ns], safe.cpu().numpy(), buf.host("space")
    bad = np.argwhere(got_c != want_c)
    assert bad.size == 0, (what, "space", bad[:5].tolist(), got_c[bad[0][0]].tolist(), want_c[bad[0][0]].tolist(), states[bad[0][0]])
    bad = np.argwhere(got_m != want_m)
    assert bad.size == 0, (what, "mask", bad[:5].tolist(), got_m[bad[0][0]], want_m[bad[0][0]], states[bad[0][0]])
    bad = np.argwhere(got_a != want_a)
    assert bad.size == 0, (what, "action", bad[:5].tolist(), got_a[bad[0][0]], want_a[bad[0][0]], states[bad[0][0]])
    assert buf.guards_intact(), what
    return want_a


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim", [2, 3, 6, 19, 32, 33, 62])
def test_hand_built_snake_env_states(dim):
    """Border and corner heads, heads at -1 / dim, random bodies, stacked duplicates, empty bodies, dense boards."""
    ns = 3
    rng = np.random.default_rng([7, dim])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, ns, rng, 30 if dim < 62 else 12)
    states.append(_st([[], [], []], [(0, 0)] * ns))
    env = _install(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states)
    _check_call(env, states, what=("snake_env", dim))
    env.close()


@pytest.mark.parametrize("dim", [6, 10])
def test_hand_built_new_world_states_with_four_snakes(dim):
    """Four snakes, some dead with their bodies kept (alive False, in and out of dead_snakes), stacked duplicates."""
    ns, nf = 4, 5
    rng = np.random.default_rng([8, dim])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 30)
    for st in states[::2]:
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    # a kept, stacked, dead body walls in the corner like any other
    states.append(_st([[(0, 0)], [(1, 0), (1, 0), (1, 1), (0, 2), (1, 2)], [], [(3, 3)]], [(0, 1)] * nf,
                      alive=[True, False, True, True], in_dead=[False, True, False, False]))
    env = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    assert spp.np_space(states[-1], dim, ns)[0].tolist() == [0, 1, 0, 0]   # the pocket of 1 cell at (0, 1)
    _check_call(env, states, what=("new_world", dim))
    env.close()


@pytest.mark.parametrize("dim", [6, 19])
def test_hand_built_adversarial_states_with_long_fruit_lists(dim):
    """Fruit lists past 64 entries (up to the list's capacity), entries at -1 / dim included, on dense boards; and the
    nearest fruit at an index >= 64 deciding between two eligible moves."""
    ns = 3
    rng = np.random.default_rng([9, dim])
    fcap = (3 + 3 * (dim * dim + 2) + 63) // 64 * 64      # the handle's fruit-list capacity
    states = []
    for n_list in (0, 1, 63, 64, 65, min(130, fcap - 3), fcap):   # (dim 6: the capacity is 128 entries)
        for st in bs.dense_states(dim, ns, n_list, rng, 5, fruit_lo=-1, fruit_hi=dim + 1):
            states.append(st)
    h = (dim // 2, dim // 2)
    first = len(states)
    for a in (1, 2, 3, 4):                                # an open board: the fruit at list index 70 sits on the target of move a
        fl = [(-1, -1)] * 100
        fl[70] = (h[0] + sp.DIRS[a][0], h[1] + sp.DIRS[a][1])
        states.append(_st([[h], [], []], fl))
    env = _install(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want = _check_call(env, states, what=("adversarial", dim))
    assert want[first:first + 4, 0].tolist() == [1, 2, 3, 4]
    env.close()


# ------------------------------------------------------------------------------------------ 2. longest fills
def _maze_states(dim, transposed):
    """Snake 1 is the wall of a serpentine maze, snake 0 a stack of k duplicates on corridor cell i: the corridor falls
    into the i cells before the head and the L - 1 - i cells behind it.  Heads at both ends, in the middle, and inside
    wall gaps (where the two parts are entered by opposite moves); k below, between and above the two sizes."""
    walls, path = spp.serpentine(dim, transposed)
    L = len(path)
    gaps = [i for i, c in enumerate(path) if c[0 if transposed else 1] % 2 == 1]
    at = sorted({0, 1, L - 1, L - 2, L // 2, L // 3, gaps[0], gaps[len(gaps) // 2], gaps[-1]})
    states, sizes = [], []
    for n, i in enumerate(at):
        small, large = sorted((i, L - 1 - i))
        k = (1, small + 1, large + 5)[n % 3]
        lure = path[i - 1] if i >= 1 and i <= L - 1 - i else path[min(i + 1, L - 1)]   # a fruit in the smaller part
        states.append(_st([[path[i]] * max(k, 1), walls], [lure, lure]))
        sizes.append((i, L - 1 - i))
    return states, sizes, L


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes(dim, transposed):
    """The longest fills there are: one corridor through the whole board (1 953 cells at dim 62), along the rows (the
    fill runs inside the lanes' masks) and transposed (it runs from lane to lane).  Every count is known in closed form."""
    states, sizes, L = _maze_states(dim, transposed)
    assert L == {6: 21, 33: 577, 62: 1953}[dim]
    env = _install(dict(rules=0, dim=dim, n_snakes=2, n_fruits=2), states)
    buf = Guarded(env)
    want = _check_call(env, states, buf, what=("maze", dim, transposed))
    got = buf.host("space")
    for e, (a, b) in enumerate(sizes):      # the closed form, without the helper
        assert sorted(v for v in got[e, 0].tolist() if v) == sorted(v for v in (a, b) if v), (e, a, b, got[e].tolist())
    # the stack of duplicates is longer than the smaller part: the move into the larger part, away from the fruit
    for e, (a, b) in enumerate(sizes):
        k = len(states[e]["snakes"][0])
        if min(a, b) and k > min(a, b) and a != b:
            assert got[e, 0, want[e, 0] - 1] == max(a, b), (e, a, b, k)
    env.close()


# ------------------------------------------------------------------------------------------ 3. overflow ring
@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (0, 19, 3), (1, 12, 2), (2, 10, 3), (0, 20, 3)])
def test_separating_piece_in_the_overflow_ring(rules, dim, ns):
    """Pieces with an index >= 64 block a move or wall two regions off.  Installed in the library and the oracle alike,
    compared after the install and after each of a few steps under space_greedy."""
    import torch
    from oracle.snake_oracle import state_to_flat
    states, walled = bs.overflow_states(dim, ns)
    for st in states[len(states) - walled:]:     # the wall: two regions of different sizes; one region without the pieces >= 64
        full = spp.np_space(st, dim, ns)[1]
        cut = spp.np_space(dict(st, snakes=[b[:64] for b in st["snakes"]]), dim, ns)[1]
        assert full[1] > 0 and full[3] == dim and full[1] != full[3] and cut[1] == cut[3] > full[1] + full[3], (full, cut)
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="space_greedy")
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    old_piece_decides = 0
    for t in range(8):
        cur = _states(ora)
        for st in cur:     # the cases this test is there for, from the oracle's state: pieces >= 64 decide which moves are open
            cut = dict(st, snakes=[b[:64] for b in st["snakes"]])
            old_piece_decides += not np.array_equal(spp.np_space(st, dim, ns) > 0, spp.np_space(cut, dim, ns) > 0)
        act = _check_call(env, cur, what=("overflow", t))
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert old_piece_decides >= 6, old_piece_decides
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 4. closed loop
def _call(env, buf, snakes=None):
    out, safe, _ = env.scripted_actions_device("space_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe, space_out=buf.space)
    return out, safe, buf.host("space")


def _closed_loop(cfg, env, steps, **kw):
    """gpu_harness.closed_loop under space_greedy with all three outputs; returns the number of episodes that ended."""
    episodes = []
    gh.closed_loop(cfg, env, _call, lambda states: expected(states, cfg["dim"], cfg["n_snakes"]), steps, buffers=Guarded,
                   observe=lambda t, states, wants, o_done, o_el: episodes.append(int(o_done.sum())), **kw)
    return sum(episodes)


@pytest.mark.parametrize("name,steps", [("S19x3", 150), ("A10x3", 150), ("N10x4", 100)])
def test_closed_loop_with_the_oracle_as_master(name, steps):
    cfg = _cfg(name, num_envs=8) if name != "N10x4" else _cfg(name)
    assert cfg["num_envs"] == 8
    env = _mk(cfg)
    _closed_loop(cfg, env, steps)
    env.close()


# ------------------------------------------------------------------------------------------ 5. layout
@pytest.mark.parametrize("record_policy", ["full", "short"])
@pytest.mark.parametrize("epb", [1, 4, 8])
def test_record_policies_and_envs_per_block(record_policy, epb):
    cfg = _cfg("S19x3", num_envs=37)   # ragged: no multiple of any envs_per_block, nor of the kernel's four waves per block
    env = _mk(cfg, record_policy=record_policy, envs_per_block=epb)
    _closed_loop(cfg, env, 30, obs_every=29)
    env.close()


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batch_sizes(n):
    cfg = _cfg("N10x4", num_envs=n)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    gh.play_random(env, ora, 6, np.random.default_rng(n), threads=1)
    _check_call(env, _states(ora), what=n)
    env.close()


@pytest.mark.parametrize("name", ["S19x3", "A10x3"])
def test_after_a_persistent_tape_rollout(name):
    import torch
    cfg = _cfg(name, num_envs=48)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    rng = np.random.default_rng(3)
    for chunk in range(2):
        tape = rng.integers(0, 5, (25, 48, cfg["n_snakes"])).astype(np.int32)
        tape[:, :, :] = np.where(rng.random(tape.shape) < 0.5, tape, 2 - chunk % 2)   # long runs in one direction too
        env.rollout_device(torch.from_numpy(tape).to(env.device), persistent=True, keep_obs=False)
        for t in range(25):
            ora.step(tape[t], want_obs=False)
        _check_call(env, _states(ora), what=(name, chunk))
    env.close()


def test_after_a_masked_reset():
    import torch
    cfg = _cfg("N10x4", num_envs=32)
    env, ora = _mk(cfg, auto_reset=False), sp.make_oracle(cfg, auto_reset=False)
    env.reset(), ora.reset()
    rng = np.random.default_rng(5)
    resets = 0
    for t in range(40):
        act = rng.integers(0, 5, (32, 4)).astype(np.int32)
        _, _, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, _, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), o_done)
        if o_done.any() and t % 2 == 0:
            _check_call(env, _states(ora), what=("finished envs in place", t))
            env.reset_device(mask=done)
            ora.reset_envs(o_done, obs=None, final_obs=None, truncated=None)
            resets += int(o_done.sum())
            _check_call(env, _states(ora), what=("after reset_envs", t))
    assert resets >= 10
    env.close()


# ------------------------------------------------------------------------------------------ 6. mixed control, strides, outputs
@pytest.mark.parametrize("name,stride,snakes", [("S19x3", 5, (1, 2)), ("N10x4", 7, (0, 3)), ("S19x3", 7, (1,))])
def test_mixed_control_leaves_the_other_columns_untouched(name, stride, snakes):
    cfg = _cfg(name, num_envs=8) if name != "N10x4" else _cfg(name)
    env = _mk(cfg)
    _closed_loop(cfg, env, 40, control=(np.random.default_rng(11), snakes), stride=stride, obs_every=39)
    env.close()


@pytest.mark.parametrize("stride", [4, 5, 7])
def test_each_output_alone_and_all_together(stride):
    cfg = _cfg("N10x4", num_envs=13)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    gh.play_random(env, ora, 6, np.random.default_rng(stride), threads=1)
    states = _states(ora)
    want_a, want_m, want_c = expected(states, 10, 4)
    buf = Guarded(env, stride)
    untouched = lambda: buf.untouched("act")
    # space_dev alone
    assert env.reachable_space_device(out=buf.space) is buf.space
    assert np.array_equal(buf.host("space"), want_c) and untouched() and buf.untouched("safe") and buf.guards_intact()
    assert np.array_equal(env.reachable_space_device().cpu().numpy(), want_c)      # a fresh tensor of the env's
    # safe_dev alone (an empty selection): no action word and no count is written
    buf.refill()
    out, safe = env.scripted_actions_device("space_greedy", snakes=[], out=buf.act, safe_out=buf.safe)
    assert np.array_equal(safe.cpu().numpy(), want_m) and untouched() and buf.untouched("space") and buf.guards_intact()
    # actions alone, snakes 3 and 1 only
    buf.refill()
    out = env.scripted_actions_device("space_greedy", snakes=[3, 1], out=buf.act)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [1, 3]], want_a[:, [1, 3]]) and (got[:, [0, 2] + list(range(4, stride))] == FILL).all()
    assert buf.untouched("safe") and buf.untouched("space") and buf.guards_intact()
    # all three, snake 2 only: the mask and the counts are written for every snake whatever the selection
    buf.refill()
    out, safe, space = env.scripted_actions_device("space_greedy", snakes=[2], out=buf.act, safe_out=buf.safe, space_out=buf.space)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 2], want_a[:, 2]) and (got[:, [0, 1, 3] + list(range(4, stride))] == FILL).all()
    assert np.array_equal(safe.cpu().numpy(), want_m) and np.array_equal(buf.host("space"), want_c) and buf.guards_intact()
    # the results do not depend on which outputs are asked for
    for kw in (dict(safe_out=buf.safe), dict(space_out=buf.space), dict()):
        buf.refill()
        res = env.scripted_actions_device("space_greedy", out=buf.act, **kw)
        got = (res if not kw else res[0]).cpu().numpy()
        assert np.array_equal(got[:, :4], want_a) and (got[:, 4:] == FILL).all() and buf.guards_intact(), kw
    # the env's own cached action buffer, shared with the other policies
    a = env.scripted_actions_device("space_greedy", snakes=[2])
    assert a.data_ptr() == env.scripted_actions_device("safe_greedy", snakes=[1]).data_ptr()
    assert np.array_equal(a.cpu().numpy()[:, 2], want_a[:, 2])
    env.close()


# ------------------------------------------------------------------------------------------ 7. read-only
def test_the_call_changes_no_state():
    import torch
    cfg = _cfg("A10x3", num_envs=40)
    env, plain = _mk(cfg), _mk(cfg)
    assert np.array_equal(env.reset(), plain.reset())
    rng = np.random.default_rng(8)
    buf = Guarded(env)
    for t in range(100):
        act = torch.from_numpy(rng.integers(0, 5, (40, 3)).astype(np.int32)).to(env.device)
        if t % 25 == 0:
            before, st_before = env.get_state_all().tobytes(), env.stats()
        env.scripted_actions_device("space_greedy", out=buf.act, safe_out=buf.safe, space_out=buf.space)
        env.reachable_space_device(out=buf.space)
        env.scripted_actions_device("space_greedy", snakes=[1])
        if t % 25 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 100 * 40   # the call adds nothing to env_steps
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 8. HIP graph
def test_graph_of_space_actions_then_step():
    """[msnake_space_actions -> msnake_step] captured as one linear chain and replayed 100 times on 64 envs: final state,
    rewards and last actions against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = _cfg("S19x3", num_envs=64)
    K = 100
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((64, 3), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("space_greedy", out=acts)
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("space_greedy", out=acts)
        out = env.step_device(acts)
    torch.cuda.synchronize()
    env.set_state_all(blob)
    rews = []
    for _ in range(K):
        g.replay()
        rews.append(out[1].clone())
    torch.cuda.synchronize()
    want, o_rews = None, []
    for _ in range(K):
        want = expected(_states(ora), 19, 3)[0]
        o_rews.append(ora.step(want)[1].copy())
    assert np.array_equal(acts.cpu().numpy(), want)
    assert np.array_equal(torch.stack(rews).cpu().numpy(), np.stack(o_rews))
    assert np.array_equal(out[0].cpu().numpy(), ora.obs)
    for e in range(64):
        assert flat_to_state(env.get_state_words(e)) == ora.get_state(e), e
    env.close()


# ------------------------------------------------------------------------------------------ 9. errors
def test_argument_errors_name_the_argument():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=3, rules="snake_env", seed=0)
    env.reset()
    L = env._L
    acts = torch.full((5, 3), 9, dtype=torch.int32, device=env.device)
    safe = torch.full((5, 3), 9, dtype=torch.uint8, device=env.device)
    space = torch.full((5 * 3 * 4 + 1,), 9, dtype=torch.int16, device=env.device)
    pa, ps, pc = acts.data_ptr(), safe.data_ptr(), space.data_ptr()

    def call(h, mask, a, stride, s, c):
        rc = L.msnake_space_actions(h, mask, a, stride, s, c, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 0b1000, pa, 3, None, None), "snake_mask"), ((env._h, 0b1000, None, 3, ps, pc), "snake_mask"),
                       ((env._h, 0b111, pa, 2, None, pc), "action_stride"), ((env._h, 1, None, 3, ps, pc), "actions_dev"),
                       ((env._h, 0, pa, 3, None, None), "nothing to write"), ((env._h, 0, None, 0, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args[1:], rc, msg)
    rc, msg = call(env._h, 0, None, 0, None, pc + 1)
    assert rc < 0 and rc != -1 and "space_dev" in msg, (rc, msg)        # MSNAKE_E_ALIGN
    assert call(None, 1, pa, 3, None, None)[0] == -3
    torch.cuda.synchronize()
    assert (acts.cpu().numpy() == 9).all() and (safe.cpu().numpy() == 9).all() and (space.cpu().numpy() == 9).all()
    # what is NOT an error: action_stride / actions_dev are not looked at when no action is written
    assert call(env._h, 0, None, 0, ps, None)[0] == 0 and call(env._h, 0, None, 0, None, pc)[0] == 0
    assert call(env._h, 0b101, pa, 3, None, None)[0] == 0
    with pytest.raises(ValueError, match="space_out"):
        env.scripted_actions_device("safe_greedy", space_out=space[:60].view(torch.uint16).view(5, 3, 4))
    assert env.stats()["env_steps"] == 0
    env.close()
