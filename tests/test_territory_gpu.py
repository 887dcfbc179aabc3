"""Voronoi territory counts and the opponent territory_greedy on the device (msnake_territory_actions) against
tests/territory_play.py.

Everything is bit-exact and nothing is left out of a comparison: every env, snake and move.  The expected counts are
territory_play.territory_sets (pinned to the BFS form np_territory by tests/test_territory_host.py, and again here on a
sample of the states of every hand-built test), the expected actions territory_play.territory_greedy with eps = 0, the
expected mask scripted_play.np_safe_mask, all on the canonical state of the CPU oracle or on a hand-built state dict;
none of them ever comes from the library under test.  Every output sits between guard elements.
"""

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import scripted_play as sp
import space_play as spp
import territory_play as tp

pytestmark = pytest.mark.gpu

FILL = -77  # the sentinel of the action buffer (gpu_harness.action_spec)
_st, _mk, _states, _install = bs.state, gh.make_env, gh.oracle_states, gh.install


def Guarded(env, stride=None):
    """Actions, mask and a uint16 [n, ns, 4] count buffer `terr`, each between guard elements."""
    return gh.GuardedOutputs(env.device, dict(gh.action_spec(env, stride), **gh.count_spec(env, "terr")))


# ------------------------------------------------------------------------------------------ expectations
def expected(states, dim, ns, bfs_every=0):
    """(actions int32 [E, ns], masks uint8 [E, ns], counts uint16 [E, ns, 4]) of the helpers on canonical state dicts.
    bfs_every = k > 0: every k-th state's counts are also computed by the BFS form and must agree."""
    counts = [tp.territory_sets(st, dim, ns) for st in states]
    if bfs_every:
        for st, c in list(zip(states, counts))[::bfs_every]:
            assert np.array_equal(tp.np_territory(st, dim, ns), c), st
    act = np.array([tp.greedy_by_count(st, dim, ns, c) for st, c in zip(states, counts)], np.int32).reshape(len(states), ns)
    mask = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(len(states), ns)
    terr = np.array(counts).reshape(len(states), ns, 4)
    assert terr.max(initial=0) <= 62 * 62 - 1
    is_open = (mask[:, :, None] >> np.arange(1, 5)) & 1 == 1
    assert not terr[~is_open].any()                       # (an open move may count 0: a contested target)
    return act, mask, terr.astype(np.uint16)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, policy="territory_greedy", **kw)


def _call(env, buf, snakes=None):
    out, safe, _ = env.scripted_actions_device("territory_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe, territory_out=buf.terr)
    return out, safe, buf.host("terr")


def _check_call(env, states, buf=None, what="", bfs_every=0):
    """One call with all three outputs, compared for every env, snake and move; returns the expectations."""
    dim, ns = env.cfg.dim, env.n_snakes
    buf = buf or Guarded(env)
    want_a, want_m, want_c = expected(states, dim, ns, bfs_every)
    out, safe, _ = _call(env, buf)
    got_a, got_m, got_c = out.cpu().numpy()[:, :ns], safe.cpu().numpy(), buf.host("terr")
    bad = np.argwhere(got_c != want_c)
    assert bad.size == 0, (what, "territory", bad[:5].tolist(), got_c[bad[0][0]].tolist(), want_c[bad[0][0]].tolist(), states[bad[0][0]])
    bad = np.argwhere(got_m != want_m)
    assert bad.size == 0, (what, "mask", bad[:5].tolist(), got_m[bad[0][0]], want_m[bad[0][0]], states[bad[0][0]])
    bad = np.argwhere(got_a != want_a)
    assert bad.size == 0, (what, "action", bad[:5].tolist(), got_a[bad[0][0]], want_a[bad[0][0]], states[bad[0][0]])
    assert buf.guards_intact(), what
    return want_a, want_m, want_c


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim,ns", [(2, 2), (3, 3), (6, 1), (6, 3), (19, 3), (32, 2), (33, 3), (62, 3)])
def test_hand_built_snake_env_states(dim, ns):
    """Border and corner heads, heads at -1 / dim, random bodies, stacked duplicates, empty bodies, boards 25 - 65 % full."""
    rng = np.random.default_rng([17, dim, ns])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, ns, rng, 30 if dim < 62 else 12)
    states.append(_st([[] for _ in range(ns)], [(0, 0)] * ns))
    env = _install(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states)
    _, _, want_c = _check_call(env, states, what=("snake_env", dim, ns), bfs_every=1 if dim <= 6 else 9 if dim < 62 else 25)
    if ns > 1:      # the boards are there for the opponents: on some of them they take cells away
        space = np.array([spp.np_space(st, dim, ns) for st in states])
        assert (want_c != space).any(axis=(1, 2)).sum() >= 10
    env.close()


def test_hand_built_new_world_states_with_four_snakes():
    """Four snakes, some dead with their bodies kept (alive False, in and out of dead_snakes): a dead snake that kept its
    body is an opponent like any other."""
    dim, ns, nf = 10, 4, 5
    rng = np.random.default_rng([18, dim])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 30)
    for st in states[::2]:
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    # the dead snake 1 at (2, 0) contests (1, 0) with snake 0 at (0, 0), and walls the rest of row 0 off with its body
    states.append(_st([[(0, 0)], [(2, 0), (3, 0), (3, 1), (2, 1)], [], [(9, 9)]], [(0, 1)] * nf,
                      alive=[True, False, True, True], in_dead=[False, True, False, False]))
    assert tp.np_territory(states[-1], dim, ns)[0, 0] == 0 and sp.np_safe_mask(states[-1], dim, ns)[0] == 0b00110
    env = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    _check_call(env, states, what=("new_world", dim), bfs_every=3)
    env.close()


def test_hand_built_adversarial_states_with_long_fruit_lists():
    """Fruit lists past 64 entries (up to the list's capacity), entries at -1 / dim included, on dense boards; and the
    nearest fruit at an index >= 64 deciding between eligible moves."""
    dim, ns = 6, 3
    rng = np.random.default_rng([19, dim])
    fcap = (3 + 3 * (dim * dim + 2) + 63) // 64 * 64      # the handle's fruit-list capacity
    states = []
    for n_list in (0, 1, 63, 64, 65, fcap - 3, fcap):
        states += bs.dense_states(dim, ns, n_list, rng, 5, fruit_lo=-1, fruit_hi=dim + 1)
    h = (dim // 2, dim // 2)
    first = len(states)
    for a in (1, 2, 3, 4):                                # an open board: the fruit at list index 70 sits on the target of move a
        fl = [(-1, -1)] * 100
        fl[70] = (h[0] + sp.DIRS[a][0], h[1] + sp.DIRS[a][1])
        states.append(_st([[h], [], []], fl))
    env = _install(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want, _, _ = _check_call(env, states, what=("adversarial", dim), bfs_every=1)
    assert want[first:first + 4, 0].tolist() == [1, 2, 3, 4]
    env.close()


# ------------------------------------------------------------------------------------------ 2. contested targets, tie parity
@pytest.mark.parametrize("dim", [39, 40])
def test_contested_targets_and_corridor_parity_at_the_edges_and_across_bit_32(dim):
    """Two heads two cells apart (the cell between them is open for both and counts 0), along a row and along a column,
    in the corners, on the borders and with the contested cell in column 31, 32 and 33 (the two 32-bit halves of a row
    mask); and a corridor under a full-width wall, raced from both ends: dim - 2 free cells, the odd one in the middle
    belongs to nobody.  The corridor runs along a row (inside the lanes' masks, across bit 31 / 32) and along a column."""
    states, contested = [], []
    for y in (0, 17, dim - 1):
        for x in (0, 30, 31, 32, dim - 3):
            states.append(_st([[(x, y)], [(x + 2, y)], []], [(0, 0)] * 3)), contested.append((0, 2))   # moves 1 / 3 meet
            states.append(_st([[(y, x)], [(y, x + 2)], []], [(0, 0)] * 3)), contested.append((1, 3))   # moves 2 / 4 meet
    each = (dim - 2) // 2
    wall = [(x, 1) for x in range(dim)]
    far = [(x, dim - 2) for x in range(dim)]
    first = len(states)
    states.append(_st([[(0, 0)], [(dim - 1, 0)], wall], [(5, 0)] * 3))
    states.append(_st([[(0, 0)], [(0, dim - 1)], [(y, x) for x, y in wall]], [(0, 5)] * 3))
    states.append(_st([[(0, dim - 1)], [(dim - 1, dim - 1)], far], [(5, 5)] * 3))
    states.append(_st([[(dim - 1, 0)], [(dim - 1, dim - 1)], [(y, x) for x, y in far]], [(5, 5)] * 3))
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    _, want_m, want_c = _check_call(env, states, what=("parity", dim), bfs_every=5)
    for e, (m0, m1) in enumerate(contested):           # the closed form, without the helper
        assert want_c[e, 0, m0] == 0 and want_c[e, 1, m1] == 0
        assert (want_m[e, 0] >> (m0 + 1)) & 1 and (want_m[e, 1] >> (m1 + 1)) & 1
    assert want_c[first, 0].tolist() == [each, 0, 0, 0] and want_c[first, 1].tolist() == [0, 0, each, 0]
    assert want_c[first + 1, 0].tolist() == [0, each, 0, 0] and want_c[first + 1, 1].tolist() == [0, 0, 0, each]
    assert want_c[first + 2, 0].tolist() == [each, 0, 0, 0] and want_c[first + 2, 1].tolist() == [0, 0, each, 0]
    assert want_c[first + 3, 0].tolist() == [0, each, 0, 0] and want_c[first + 3, 1].tolist() == [0, 0, 0, each]
    env.close()


# ------------------------------------------------------------------------------------------ 3. longest races
def _maze_states(dim, transposed):
    """The serpentine corridor of L cells with its walls stacked under snake 0's head (two snakes in all).  Both snakes
    on the two ends: L - 2 free cells between them, (L - 2) // 2 each.  Snake 0 alone on one end: L - 1 cells, after
    L - 2 rounds -- the longest race a board of this size has.  Both in the middle: three pieces, one shared."""
    walls, path = spp.serpentine(dim, transposed)
    L = len(path)
    i, j = L // 3, 2 * L // 3 + 1
    states = [_st([[path[0]] + walls, [path[-1]]], [path[1], path[-2]]),
              _st([[path[0]] + walls, []], [path[-1]] * 2),
              _st([[path[i]] + walls, [path[j]]], [path[i - 1], path[j - 1]]),
              _st([[path[-1]] + walls, [path[L // 2]]], [path[0]] * 2)]
    return states, L, (i, j)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes_entered_from_both_ends(dim, transposed):
    states, L, (i, j) = _maze_states(dim, transposed)
    assert L == {6: 21, 33: 577, 62: 1953}[dim] and L - 2 < dim * dim       # the kernel's cut lies behind the longest race
    env = _install(dict(rules=0, dim=dim, n_snakes=2, n_fruits=2), states)
    buf = Guarded(env)
    _check_call(env, states, buf, what=("maze", dim, transposed), bfs_every=1)
    got = buf.host("terr")
    nz = lambda row: sorted(int(v) for v in row if v)                       # the closed forms, without the helper
    assert nz(got[0, 0]) == [(L - 2) // 2] and nz(got[0, 1]) == [(L - 2) // 2]
    assert nz(got[1, 0]) == [L - 1] and nz(got[1, 1]) == []
    between = j - i - 1
    assert nz(got[2, 0]) == sorted([i, between // 2]) and nz(got[2, 1]) == sorted([L - 1 - j, between // 2])
    env.close()


# ------------------------------------------------------------------------------------------ 4. overflow ring
@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (1, 12, 2), (0, 20, 3)])
def test_separating_piece_in_the_overflow_ring(rules, dim, ns):
    """Pieces with an index >= 64 block a move or wall two regions off (the bodies of test_space_gpu.py).  Installed in
    the library and the oracle alike, compared after the install and after each of a few steps under territory_greedy."""
    import torch
    from oracle.snake_oracle import state_to_flat
    states, walled = bs.overflow_states(dim, ns)
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="territory_greedy")
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    old_piece_decides = 0
    for t in range(6):
        cur = _states(ora)
        for st in cur:     # what this test is there for, from the oracle's state: pieces >= 64 decide the counts
            cut = dict(st, snakes=[b[:64] for b in st["snakes"]])
            old_piece_decides += not np.array_equal(tp.territory_sets(st, dim, ns), tp.territory_sets(cut, dim, ns))
        act, _, _ = _check_call(env, cur, what=("overflow", t), bfs_every=4)
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert old_piece_decides >= 6, old_piece_decides
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 5. closed loop
def _closed_loop(cfg, env, steps, **kw):
    """gpu_harness.closed_loop under territory_greedy with all three outputs; returns the number of contested targets
    (open moves that count 0) the play came across."""
    contested = []

    def observe(t, states, wants, o_done, o_el):
        _, want_m, want_c = wants
        contested.append(int(((((want_m[:, :, None] >> np.arange(1, 5)) & 1) == 1) & (want_c == 0)).sum()))

    gh.closed_loop(cfg, env, _call, lambda states: expected(states, cfg["dim"], cfg["n_snakes"]), steps, buffers=Guarded,
                   observe=observe, **kw)
    return sum(contested)


@pytest.mark.parametrize("name,steps", [("S19x3", 150), ("A10x3", 150), ("N10x4", 100)])
def test_closed_loop_with_the_oracle_as_master(name, steps):
    cfg = _cfg(name, num_envs=8) if name != "N10x4" else _cfg(name)
    assert cfg["num_envs"] == 8
    env = _mk(cfg)
    _closed_loop(cfg, env, steps)
    env.close()


# ------------------------------------------------------------------------------------------ 6. layout
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
    _check_call(env, _states(ora), what=n, bfs_every=16)
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
        _check_call(env, _states(ora), what=(name, chunk), bfs_every=8)
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


# ------------------------------------------------------------------------------------------ 7. one snake: the space
@pytest.mark.parametrize("rules,dim", [(0, 10), (2, 7)])
def test_with_one_snake_the_counts_are_the_reachable_space(rules, dim):
    import torch
    cfg = dict(rules=rules, dim=dim, n_snakes=1, n_fruits=1, num_envs=24, seed=4, env_id_base=0, max_steps=2000,
               policy="territory_greedy", eps=0.0)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for t in range(60):                        # space_greedy grows bodies that cut the board into regions
        states = _states(ora)
        if t % 6 == 0:
            _, _, want_c = _check_call(env, states, what=("one snake", t), bfs_every=4)
            assert np.array_equal(want_c, np.array([spp.np_space(st, dim, 1) for st in states]))
            terr, space = env.territory_device(), env.reachable_space_device()
            assert terr.dtype == torch.uint16 and tuple(terr.shape) == (24, 1, 4)
            assert torch.equal(terr.view(torch.int16), space.view(torch.int16))
            assert np.array_equal(terr.cpu().numpy(), want_c)
        act = np.array([spp.space_greedy(st, dim, 1) for st in states], np.int32)
        env.step_device(torch.from_numpy(act).to(env.device))
        ora.step(act, want_obs=False)
    env.close()


# ------------------------------------------------------------------------------------------ 8. mixed control, strides, outputs
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
    want_a, want_m, want_c = expected(states, 10, 4, bfs_every=1)
    buf = Guarded(env, stride)
    untouched = lambda: buf.untouched("act")
    pol = "territory_greedy"
    # territory_dev alone
    assert env.territory_device(out=buf.terr) is buf.terr
    assert np.array_equal(buf.host("terr"), want_c) and untouched() and buf.untouched("safe") and buf.guards_intact()
    assert np.array_equal(env.territory_device().cpu().numpy(), want_c)            # a fresh tensor of the env's
    # safe_dev alone (an empty selection): no action word and no count is written
    buf.refill()
    out, safe = env.scripted_actions_device(pol, snakes=[], out=buf.act, safe_out=buf.safe)
    assert np.array_equal(safe.cpu().numpy(), want_m) and untouched() and buf.untouched("terr") and buf.guards_intact()
    # actions alone, snakes 3 and 1 only
    buf.refill()
    out = env.scripted_actions_device(pol, snakes=[3, 1], out=buf.act)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [1, 3]], want_a[:, [1, 3]]) and (got[:, [0, 2] + list(range(4, stride))] == FILL).all()
    assert buf.untouched("safe") and buf.untouched("terr") and buf.guards_intact()
    # all three, snake 2 only: the mask and the counts are written for every snake whatever the selection
    buf.refill()
    out, safe, terr = env.scripted_actions_device(pol, snakes=[2], out=buf.act, safe_out=buf.safe, territory_out=buf.terr)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, 2], want_a[:, 2]) and (got[:, [0, 1, 3] + list(range(4, stride))] == FILL).all()
    assert np.array_equal(safe.cpu().numpy(), want_m) and np.array_equal(buf.host("terr"), want_c) and buf.guards_intact()
    # the mask and the counts without actions
    buf.refill()
    out, safe, terr = env.scripted_actions_device(pol, snakes=[], out=buf.act, safe_out=buf.safe, territory_out=buf.terr)
    assert np.array_equal(safe.cpu().numpy(), want_m) and np.array_equal(buf.host("terr"), want_c) and untouched() and buf.guards_intact()
    # the results do not depend on which outputs are asked for
    for kw in (dict(safe_out=buf.safe), dict(territory_out=buf.terr), dict()):
        buf.refill()
        res = env.scripted_actions_device(pol, out=buf.act, **kw)
        got = (res if not kw else res[0]).cpu().numpy()
        assert np.array_equal(got[:, :4], want_a) and (got[:, 4:] == FILL).all() and buf.guards_intact(), kw
    # the env's own cached action buffer, shared with the other policies
    a = env.scripted_actions_device(pol, snakes=[2])
    assert a.data_ptr() == env.scripted_actions_device("space_greedy", snakes=[1]).data_ptr()
    assert np.array_equal(a.cpu().numpy()[:, 2], want_a[:, 2])
    env.close()


# ------------------------------------------------------------------------------------------ 9. read-only
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
        _call(env, buf)
        env.territory_device(out=buf.terr)
        env.scripted_actions_device("territory_greedy", snakes=[1])
        if t % 25 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 100 * 40   # the call adds nothing to env_steps
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 10. HIP graph
def test_graph_of_territory_actions_then_step():
    """[msnake_territory_actions -> msnake_step] captured as one linear chain and replayed 50 times on 64 envs: final
    state, rewards and last actions against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = _cfg("S19x3", num_envs=64)
    K = 50
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((64, 3), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("territory_greedy", out=acts)
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("territory_greedy", out=acts)
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


# ------------------------------------------------------------------------------------------ 11. errors
def test_argument_errors_name_the_argument():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=3, rules="snake_env", seed=0)
    env.reset()
    L = env._L
    acts = torch.full((5, 3), 9, dtype=torch.int32, device=env.device)
    safe = torch.full((5, 3), 9, dtype=torch.uint8, device=env.device)
    terr = torch.full((5 * 3 * 4 + 1,), 9, dtype=torch.int16, device=env.device)
    pa, ps, pc = acts.data_ptr(), safe.data_ptr(), terr.data_ptr()

    def call(h, mask, a, stride, s, c):
        rc = L.msnake_territory_actions(h, mask, a, stride, s, c, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 0b1000, pa, 3, None, None), "snake_mask"), ((env._h, 0b1000, None, 3, ps, pc), "snake_mask"),
                       ((env._h, 0b111, pa, 2, None, pc), "action_stride"), ((env._h, 1, None, 3, ps, pc), "actions_dev"),
                       ((env._h, 1, None, 2, ps, pc), "actions_dev"),          # the order of the checks: the pointer first
                       ((env._h, 0, pa, 3, None, None), "nothing to write"), ((env._h, 0, None, 0, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg and "msnake_territory_actions" in msg, (args[1:], rc, msg)
    rc, msg = call(env._h, 0, None, 0, None, pc + 1)
    assert rc < 0 and rc != -1 and "territory_dev" in msg, (rc, msg)        # MSNAKE_E_ALIGN
    rc, msg = call(env._h, 1, pa + 2, 3, None, None)
    assert rc < 0 and rc != -1 and "actions_dev" in msg, (rc, msg)
    assert call(None, 1, pa, 3, None, None)[0] == -3
    torch.cuda.synchronize()
    assert (acts.cpu().numpy() == 9).all() and (safe.cpu().numpy() == 9).all() and (terr.cpu().numpy() == 9).all()
    # what is NOT an error: action_stride / actions_dev are not looked at when no action is written
    assert call(env._h, 0, None, 0, ps, None)[0] == 0 and call(env._h, 0, None, 0, None, pc)[0] == 0
    assert call(env._h, 0b101, pa, 3, None, None)[0] == 0
    view = terr[:60].view(torch.uint16).view(5, 3, 4)
    with pytest.raises(ValueError, match="territory_out"):
        env.scripted_actions_device("space_greedy", territory_out=view)
    with pytest.raises(ValueError, match="space_out"):
        env.scripted_actions_device("territory_greedy", space_out=view)
    assert env.stats()["env_steps"] == 0
    env.close()
