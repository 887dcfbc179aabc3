"""Cell lifetimes, the timed reach and the opponent timed_greedy on the device (msnake_timed_actions) against
tests/timed_play.py.

Everything is bit-exact and nothing is left out of a comparison: every env, snake, move and cell.  The expected lifetimes
are timed_play.np_life, the expected reaches timed_play.np_timed, the expected actions timed_play.timed_greedy with
eps = 0, the expected mask scripted_play.np_safe_mask, all on the canonical state of the CPU oracle or on a hand-built
state dict; none of them ever comes from the library under test.  Every output sits between guard elements, and every
check call runs once with life_dev and once without it: then the lifetime buffer must keep its sentinel.
"""

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import scripted_play as sp
import space_play as spp
import timed_play as tp

pytestmark = pytest.mark.gpu

NEVER, BIG = tp.NEVER, tp.BIG
_st, _mk, _states, _install = bs.state, gh.make_env, gh.oracle_states, gh.install
FILL, SENT = -77, 0xA5A5   # the sentinels of the action buffer (gpu_harness.action_spec) and of the uint16 buffers


# ------------------------------------------------------------------------------------------ expectations
def expected(states, dim, ns, never=False):
    """(actions int32 [E, ns], masks uint8 [E, ns], reaches uint16 [E, ns, 4], lifetimes uint16 [E, dim, dim]) of the
    helpers on canonical state dicts."""
    E = len(states)
    mask = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(E, ns)
    life = np.array([tp.np_life(st, dim, never) for st in states]).reshape(E, dim, dim)
    reach = np.array([tp.np_timed(st, dim, ns, L) for st, L in zip(states, life)]).reshape(E, ns, 4)
    act = np.array([tp.greedy_by_count(st, ns, r) for st, r in zip(states, reach)], np.int32).reshape(E, ns)
    assert reach.max(initial=0) <= dim * dim and life.max(initial=0) <= NEVER
    # the statements agree with each other: a move is open iff its reach is not 0, and the action is an open move or 0
    is_open = (mask[:, :, None] >> np.arange(1, 5)) & 1 == 1
    assert np.array_equal(reach > 0, is_open)
    chosen = np.take_along_axis(np.concatenate([np.ones((E, ns, 1), bool), is_open], 2), act[:, :, None], 2)
    assert chosen.all()
    return act, mask, reach.astype(np.uint16), life.astype(np.uint16)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, policy="timed_greedy", **kw)


def Guarded(env, stride=None, shift=0):
    """Actions, mask, a uint16 [n, ns, 4] buffer `reach` and a uint16 [n, dim, dim] buffer `life`, each between guard
    elements.  shift = 1 starts the two uint16 payloads one element later: 2-byte aligned and no more."""
    dim = int(env.cfg.dim)
    u16 = dict(dtype="uint16", fill=SENT, offset=2 * shift, align=4)
    buf = gh.GuardedOutputs(env.device, dict(gh.action_spec(env, stride), reach=dict(u16, shape=(env.num_envs, env.n_snakes, 4)),
                                             life=dict(u16, shape=(env.num_envs, dim, dim))))
    assert buf.reach.data_ptr() % 4 == 2 * shift and buf.life.data_ptr() % 4 == 2 * shift
    return buf


def _diff(what, name, got, want, states):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, name, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist(), states[bad[0][0]])


def _check_call(env, states, buf=None, what="", want=None, never=False):
    """One call with all four outputs and one with all but the lifetimes, each compared for every env, snake, move and
    cell; returns the expected actions."""
    dim, ns = env.cfg.dim, env.n_snakes
    buf = buf or Guarded(env)
    want_a, want_m, want_r, want_l = want or expected(states, dim, ns, never)
    buf.refill()
    out, safe, reach, life = env.scripted_actions_device("timed_greedy", out=buf.act, safe_out=buf.safe, reach_out=buf.reach,
                                                         life_out=buf.life)
    _diff(what, "life", buf.host("life"), want_l, states)
    _diff(what, "reach", buf.host("reach"), want_r, states)
    _diff(what, "mask", safe.cpu().numpy(), want_m, states)
    _diff(what, "action", out.cpu().numpy()[:, :ns], want_a, states)
    assert buf.guards_intact(), what
    buf.refill()
    out, safe, reach = env.scripted_actions_device("timed_greedy", out=buf.act, safe_out=buf.safe, reach_out=buf.reach)
    _diff(what, "reach without the lifetimes", buf.host("reach"), want_r, states)
    _diff(what, "mask without the lifetimes", safe.cpu().numpy(), want_m, states)
    _diff(what, "action without the lifetimes", out.cpu().numpy()[:, :ns], want_a, states)
    assert buf.untouched("life") and buf.guards_intact(), what
    return want_a


def vary(states, rng, dim):
    """Random grow_to around the length (above, at, below, 0, the largest there is), and stacked duplicates of different
    lifetimes: a later piece on the head, an earlier piece on the tail, one >= 64 pieces from its twin, one on the
    neighbouring snake's head."""
    for st in states:
        heads = [b[0] for b in st["snakes"] if b and 0 <= b[0][0] < dim and 0 <= b[0][1] < dim]   # (only a head may lie outside)
        for s, b in enumerate(st["snakes"]):
            n = len(b)
            if n > 3 and b[0] in heads and rng.random() < 0.5:
                b[int(rng.integers(1, n))] = list(b[0])
                b[n // 2] = list(b[-1])
            if n >= 70:
                b[66] = list(b[1])
            if n > 1 and heads and rng.random() < 0.3:
                b[-1] = list(heads[int(rng.integers(0, len(heads)))])
            pick = rng.random()
            st["grow_to"][s] = BIG if pick < 0.05 else 0 if pick < 0.1 else max(0, n + int(rng.integers(-4, 7)))
    return states


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim", [2, 3, 6, 19, 32, 33, 62])
def test_hand_built_snake_env_states(dim):
    """Border and corner heads, heads at -1 / dim, random bodies, dense boards, empty bodies, with grow_to above and below
    the length and stacked pieces of different lifetimes, within one 64-piece pass and >= 64 pieces apart."""
    ns = 3
    rng = np.random.default_rng([27, dim])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 24, dup=True)
    states += bs.dense_states(dim, ns, ns, rng, 24 if dim < 62 else 8)
    vary(states, rng, dim)
    states.append(_st([[], [], []], [(0, 0)] * ns))                        # empty bodies: every reach 0, every lifetime 0
    states.append(dict(_st([[(0, 0)], [], []], [(dim - 1, dim - 1)] * ns), grow_to=[1, 1, 1]))   # the lone one-cell snake
    far = sum(len(b) >= 70 for st in states for b in st["snakes"])
    stacked = sum(len({tuple(c) for c in b}) < len(b) for st in states for b in st["snakes"])
    below = sum(g < len(b) for st in states for g, b in zip(st["grow_to"], st["snakes"]))
    assert stacked >= 10 and below >= 10 and (far >= 3 or dim < 19), (stacked, below, far)
    env = _install(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want = expected(states, dim, ns)
    assert (want[2][-2] == 0).all() and (want[3][-2] == 0).all()
    assert sorted(want[2][-1][0].tolist()) == [0, 0, dim * dim, dim * dim] and want[3][-1][0, 0] == 1
    _check_call(env, states, Guarded(env, shift=dim % 2 == 0), what=("snake_env", dim), want=want)
    env.close()


def test_the_timing_cases():
    """The doors and the coil of tests/test_timed_host.py, whose answers are closed forms."""
    states = [tp.door_state(life, second) for second in (False, True) for life in (1, 2, 3, 4, 5, 11, 12, BIG)]
    states += [tp.coil_state(g, 3) for g in (9, 10, 8, 0, BIG)]
    states += [dict(_st([[(2, 2)], [], []], [(0, 0)] * 3), grow_to=[g, 1, 1]) for g in (3, BIG, 0, 0xFFFE, 0xFFFF, 0x10000)]
    env = _install(dict(rules=0, dim=7, n_snakes=3, n_fruits=3), states)
    want = expected(states, 7, 3)
    assert want[2][:8, 0, 0].tolist() == [43, 43, 21, 21, 21, 21, 21, 21]           # the door opens on time or never
    assert want[2][8:16, 0, 0].tolist() == [44] * 5 + [43] * 3                      # ... or is taken from behind, at level 11
    assert want[0][16:21, 0].tolist() == [3, 1, 3, 3, 1] and want[2][17, 0, 2] == 2   # the coil leaves by its tail, if in time
    assert want[3][21:, 2, 2].tolist() == [3, 0xFFFE, 1, 0xFFFE, 0xFFFE, 0xFFFE]     # pending growth, capped
    _check_call(env, states, what="timing", want=want)
    env.close()


@pytest.mark.parametrize("dim,nf", [(6, 5), (10, 5), (6, 0), (10, 0)])
def test_hand_built_new_world_states_with_four_snakes(dim, nf):
    """Four snakes, some dead with their bodies kept (alive False, in and out of dead_snakes), stacked duplicates.  Without
    fruits the rule set never pops: every lifetime is NEVER and the reach is the space of msnake_space_actions."""
    import torch
    ns = 4
    rng = np.random.default_rng([28, dim])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 30)
    vary(states, rng, dim)
    for st in states[::2]:
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    env = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    want = expected(states, dim, ns, never=nf == 0)
    _check_call(env, states, what=("new_world", dim, nf), want=want)
    if nf == 0:
        assert set(np.unique(want[3]).tolist()) == {0, NEVER}
        space = np.array([spp.np_space(st, dim, ns) for st in states])
        assert np.array_equal(want[2], space)
        assert torch.equal(env.timed_reach_device(), env.reachable_space_device())
        assert np.array_equal(env.reachable_space_device().cpu().numpy(), space)
    else:
        assert (want[3] != NEVER).all()
    env.close()


@pytest.mark.parametrize("dim", [6, 19])
def test_hand_built_adversarial_states_with_long_fruit_lists(dim):
    """Fruit lists of 0, 1, 63, 64, 65 entries and up to the list's capacity, entries at -1 / dim included, on dense
    boards; and the nearest fruit at a list index >= 64 deciding between eligible moves."""
    ns = 3
    rng = np.random.default_rng([29, dim])
    fcap = (3 + 3 * (dim * dim + 2) + 63) // 64 * 64      # the handle's fruit-list capacity
    states = []
    for n_list in (0, 1, 63, 64, 65, min(130, fcap - 3), fcap):   # (dim 6: the capacity is 128 entries)
        states += bs.dense_states(dim, ns, n_list, rng, 5, fruit_lo=-1, fruit_hi=dim + 1)
    vary(states, rng, dim)
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
def _maze_states(dim, transposed, wall_grow):
    """Snake 1 is the wall of a serpentine maze with grow_to `wall_grow` (None: its length), snake 0 one cell on corridor
    cell i, with a lifetime of 1 (the fill passes over it) or clamped high (the corridor falls into two parts)."""
    walls, path = spp.serpentine(dim, transposed)
    L = len(path)
    gaps = [i for i, c in enumerate(path) if c[0 if transposed else 1] % 2 == 1]
    at = [0, L - 1, L // 2, 1, L - 3, L // 3, gaps[0], gaps[-1], gaps[len(gaps) // 2]]
    states = [dict(_st([[path[i]], walls], [path[0], path[0]]), grow_to=[1 if n % 2 else BIG, wall_grow or len(walls)])
              for n, i in enumerate(at)]
    return states, at, path


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes_with_lasting_walls(dim, transposed):
    """Walls whose lifetimes are clamped high: the fill is the corridor (1 953 cells at dim 62, as many levels), along the
    rows and transposed.  Every reach is known in closed form and is checked without the helper."""
    states, at, corridor = _maze_states(dim, transposed, BIG)
    L = len(corridor)
    assert L == {6: 21, 33: 577, 62: 1953}[dim]
    env = _install(dict(rules=0, dim=dim, n_snakes=2, n_fruits=2), states)
    buf = Guarded(env)
    _check_call(env, states, buf, what=("maze", dim, transposed))
    env.timed_reach_device(out=buf.reach)
    got, longest = buf.host("reach"), 0
    for e, i in enumerate(at):
        head = corridor[i]
        for a, (d0, d1) in sp.DIRS.items():
            t = (head[0] + d0, head[1] + d1)
            ahead, back = i + 1 < L and t == corridor[i + 1], i > 0 and t == corridor[i - 1]
            # a head that lasts cuts the corridor in two; one that is gone after a step is passed over at level 2
            want = (L - 1 - i if ahead else i if back else 0) if e % 2 == 0 else (L if ahead or back else 0)
            assert got[e, 0, a - 1] == want, (e, i, a)
            longest = max(longest, want)
    assert longest == L
    env.close()


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes_whose_walls_dissolve(dim, transposed):
    """The wall snake with its natural lifetimes: its tail rows open while the fill still runs up the corridor."""
    states, at, corridor = _maze_states(dim, transposed, None)
    env = _install(dict(rules=0, dim=dim, n_snakes=2, n_fruits=2), states)
    want = expected(states, dim, 2)
    lasting = expected(_maze_states(dim, transposed, BIG)[0], dim, 2)
    assert (want[2] >= lasting[2]).all() and (want[2] > lasting[2]).sum() >= 4       # the walls do open in time
    _check_call(env, states, what=("dissolving maze", dim, transposed), want=want)
    env.close()


# ------------------------------------------------------------------------------------------ 3. overflow ring
@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (0, 19, 3), (1, 12, 2), (2, 10, 3), (0, 20, 3)])
def test_a_piece_in_the_overflow_ring_decides_a_reach(rules, dim, ns):
    """Pieces with an index >= 64 decide a reach: the helper gives another one on the bodies cut at 64.  Installed in the
    library and the oracle alike, compared after the install and after each of a few steps under timed_greedy."""
    import torch
    from oracle.snake_oracle import state_to_flat
    states, _ = bs.overflow_states(dim, ns)
    states = [dict(st) for st in states]
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="timed_greedy")
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    old_piece_decides = 0
    buf = Guarded(env)
    for t in range(6):
        cur = _states(ora)
        for st in cur:     # the cases this test is there for, from the oracle's state
            cut = dict(st, snakes=[b[:64] for b in st["snakes"]])
            old_piece_decides += not np.array_equal(tp.np_timed(st, dim, ns), tp.np_timed(cut, dim, ns))
        act = _check_call(env, cur, buf, what=("overflow", t))
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert old_piece_decides >= 6, old_piece_decides
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 4. closed loop
def _closed_loop(cfg, env, steps, **kw):
    """gpu_harness.closed_loop under timed_greedy with actions, mask and reaches.  Even steps ask for the lifetimes too,
    odd steps do not: then the lifetime buffer must keep its sentinel."""
    step = [-1]
    never = tp.never_pops(cfg)

    def want(states):
        step[0] += 1
        want_a, want_m, want_r, want_l = expected(states, cfg["dim"], cfg["n_snakes"], never)
        return want_a, want_m, want_r, want_l if step[0] % 2 == 0 else np.full_like(want_l, SENT)

    def call(env, buf, snakes):
        buf.refill(["life"])
        life = dict(life_out=buf.life) if step[0] % 2 == 0 else {}
        out, safe, *_ = env.scripted_actions_device("timed_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe,
                                                    reach_out=buf.reach, **life)
        return out, safe, buf.host("reach"), buf.host("life")

    gh.closed_loop(cfg, env, call, want, steps, buffers=Guarded, **kw)


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
    _closed_loop(cfg, env, 20, obs_every=19)
    env.close()


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batch_sizes(n):
    cfg = _cfg("N10x4", num_envs=n)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    gh.play_random(env, ora, 6, np.random.default_rng(n), threads=1)
    _check_call(env, _states(ora), Guarded(env, shift=1), what=n)
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
    buf = Guarded(env)
    for t in range(40):
        act = rng.integers(0, 5, (32, 4)).astype(np.int32)
        _, _, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, _, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), o_done)
        if o_done.any() and t % 2 == 0:
            _check_call(env, _states(ora), buf, what=("finished envs in place", t))
            env.reset_device(mask=done)
            ora.reset_envs(o_done, obs=None, final_obs=None, truncated=None)
            resets += int(o_done.sum())
            _check_call(env, _states(ora), buf, what=("after reset_envs", t))
    assert resets >= 10
    env.close()


# ------------------------------------------------------------------------------------------ 6. mixed control, strides, outputs
@pytest.mark.parametrize("name,stride,snakes", [("S19x3", 5, (1, 2)), ("N10x4", 7, (0, 3)), ("S19x3", 7, (1,))])
def test_mixed_control_leaves_the_other_columns_untouched(name, stride, snakes):
    cfg = _cfg(name, num_envs=8) if name != "N10x4" else _cfg(name)
    env = _mk(cfg)
    _closed_loop(cfg, env, 30, control=(np.random.default_rng(11), snakes), stride=stride, obs_every=29)
    env.close()


@pytest.mark.parametrize("stride,shift", [(4, 0), (5, 1), (7, 0)])
def test_each_output_alone_and_all_together(stride, shift):
    import itertools
    cfg = _cfg("N10x4", num_envs=13)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    gh.play_random(env, ora, 6, np.random.default_rng(stride), threads=1)
    states = _states(ora)
    want_a, want_m, want_r, want_l = expected(states, 10, 4)
    buf = Guarded(env, stride, shift=shift)
    acts_untouched, safe_untouched = lambda: buf.untouched("act"), lambda: buf.untouched("safe")
    reach_untouched, life_untouched = lambda: buf.untouched("reach"), lambda: buf.untouched("life")
    # reach_dev alone
    assert env.timed_reach_device(out=buf.reach) is buf.reach
    assert np.array_equal(buf.host("reach"), want_r) and acts_untouched() and safe_untouched() and life_untouched() and buf.guards_intact()
    got = env.timed_reach_device()                                             # a fresh tensor of the env's
    assert got.dtype == __import__("torch").uint16 and np.array_equal(got.cpu().numpy(), want_r)
    # life_dev alone
    buf.refill()
    assert env.cell_lifetimes_device(out=buf.life) is buf.life
    assert np.array_equal(buf.host("life"), want_l) and acts_untouched() and safe_untouched() and reach_untouched() and buf.guards_intact()
    got = env.cell_lifetimes_device()
    assert tuple(got.shape) == (13, 10, 10) and np.array_equal(got.cpu().numpy(), want_l)
    # safe_dev alone (an empty selection): no action word, no reach and no lifetime is written
    buf.refill()
    out, safe = env.scripted_actions_device("timed_greedy", snakes=[], out=buf.act, safe_out=buf.safe)
    assert np.array_equal(safe.cpu().numpy(), want_m) and acts_untouched() and reach_untouched() and life_untouched() and buf.guards_intact()
    # actions alone, snakes 3 and 1 only
    buf.refill()
    out = env.scripted_actions_device("timed_greedy", snakes=[3, 1], out=buf.act)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [1, 3]], want_a[:, [1, 3]]) and (got[:, [0, 2] + list(range(4, stride))] == FILL).all()
    assert safe_untouched() and reach_untouched() and life_untouched() and buf.guards_intact()
    # all four, snake 2 only: the mask, the reaches and the lifetimes are written for every snake whatever the selection
    buf.refill()
    res = env.scripted_actions_device("timed_greedy", snakes=[2], out=buf.act, safe_out=buf.safe, reach_out=buf.reach, life_out=buf.life)
    assert [t.data_ptr() for t in res] == [buf.act.data_ptr(), buf.safe.data_ptr(), buf.reach.data_ptr(), buf.life.data_ptr()]
    got = res[0].cpu().numpy()
    assert np.array_equal(got[:, 2], want_a[:, 2]) and (got[:, [0, 1, 3] + list(range(4, stride))] == FILL).all()
    assert np.array_equal(buf.safe.cpu().numpy(), want_m) and np.array_equal(buf.host("reach"), want_r)
    assert np.array_equal(buf.host("life"), want_l) and buf.guards_intact()
    # the results do not depend on which outputs are asked for: every combination, with and without the actions
    names = ("safe_out", "reach_out", "life_out")
    for with_actions in (True, False):
        for pick in itertools.product((False, True), repeat=3):
            if not with_actions and not any(pick):
                continue                                                       # nothing to write: an argument error (below)
            kw = {k: getattr(buf, k[:-4]) for k, on in zip(names, pick) if on}
            buf.refill()
            env.scripted_actions_device("timed_greedy", snakes=None if with_actions else [], out=buf.act, **kw)
            got = buf.act.cpu().numpy()
            if with_actions:
                assert np.array_equal(got[:, :4], want_a) and (got[:, 4:] == FILL).all(), kw.keys()
            else:
                assert acts_untouched(), kw.keys()
            assert np.array_equal(buf.safe.cpu().numpy(), want_m) if pick[0] else safe_untouched(), kw.keys()
            assert np.array_equal(buf.host("reach"), want_r) if pick[1] else reach_untouched(), kw.keys()
            assert np.array_equal(buf.host("life"), want_l) if pick[2] else life_untouched(), kw.keys()
            assert buf.guards_intact(), kw.keys()
    # the env's own cached action buffer, shared with the other policies
    a = env.scripted_actions_device("timed_greedy", snakes=[2])
    assert a.data_ptr() == env.scripted_actions_device("safe_greedy", snakes=[1]).data_ptr()
    assert np.array_equal(a.cpu().numpy()[:, 2], want_a[:, 2])
    env.close()


# ------------------------------------------------------------------------------------------ 7. read-only
def test_the_call_changes_no_state_and_no_neighbouring_handle():
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
            other, st_other = plain.get_state_all().tobytes(), plain.stats()
        env.scripted_actions_device("timed_greedy", out=buf.act, safe_out=buf.safe, reach_out=buf.reach, life_out=buf.life)
        env.timed_reach_device(out=buf.reach)
        env.cell_lifetimes_device(out=buf.life)
        env.scripted_actions_device("timed_greedy", snakes=[1])
        if t % 25 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before
            assert plain.get_state_all().tobytes() == other and plain.stats() == st_other
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 100 * 40   # the call adds nothing to env_steps
    assert buf.guards_intact()
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 8. HIP graph
def test_graph_of_timed_actions_then_step():
    """[msnake_timed_actions -> msnake_step] captured as one linear chain and replayed 100 times on 64 envs: final state,
    rewards, last actions and last reaches against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = _cfg("S19x3", num_envs=64)
    K = 100
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((64, 3), dtype=torch.int32, device=env.device)
    reach = torch.zeros((64, 3, 4), dtype=torch.uint16, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("timed_greedy", out=acts, reach_out=reach)
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("timed_greedy", out=acts, reach_out=reach)
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
        want = expected(_states(ora), 19, 3)
        o_rews.append(ora.step(want[0])[1].copy())
    assert np.array_equal(acts.cpu().numpy(), want[0])
    assert np.array_equal(reach.cpu().numpy(), want[2])
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
    reach = torch.full((5 * 3 * 4 + 1,), 9, dtype=torch.int16, device=env.device)
    life = torch.full((5 * 19 * 19 + 1,), 9, dtype=torch.int16, device=env.device)
    pa, ps, pr, pl = acts.data_ptr(), safe.data_ptr(), reach.data_ptr(), life.data_ptr()

    def call(h, mask, a, stride, s, r, l):
        rc = L.msnake_timed_actions(h, mask, a, stride, s, r, l, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 0b1000, pa, 3, None, None, None), "snake_mask"), ((env._h, 0b1000, None, 3, ps, pr, pl), "snake_mask"),
                       ((env._h, 0b111, pa, 2, None, pr, None), "action_stride"), ((env._h, 1, None, 3, ps, pr, pl), "actions_dev"),
                       ((env._h, 0, pa, 3, None, None, None), "nothing to write"),
                       ((env._h, 0, None, 0, None, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg and "msnake_timed_actions" in msg, (args[1:], rc, msg)
    rc, msg = call(env._h, 0, None, 0, None, pr + 1, None)
    assert rc < 0 and rc != -1 and "reach_dev" in msg, (rc, msg)        # MSNAKE_E_ALIGN
    rc2, msg = call(env._h, 0, None, 0, None, pr, pl + 1)
    assert rc2 == rc and "life_dev" in msg, (rc2, msg)
    assert call(None, 1, pa, 3, None, None, None)[0] == -3
    torch.cuda.synchronize()
    assert (acts.cpu().numpy() == 9).all() and (safe.cpu().numpy() == 9).all()
    assert (reach.cpu().numpy() == 9).all() and (life.cpu().numpy() == 9).all()
    # what is NOT an error: action_stride / actions_dev are not looked at when no action is written; any output may be NULL
    assert call(env._h, 0, None, 0, ps, None, None)[0] == 0 and call(env._h, 0, None, 0, None, pr, None)[0] == 0
    assert call(env._h, 0, None, 0, None, None, pl)[0] == 0 and call(env._h, 0, None, 0, None, pr + 2, pl + 2)[0] == 0
    assert call(env._h, 0b101, pa, 3, None, None, None)[0] == 0
    for kw in ("reach_out", "life_out"):
        with pytest.raises(ValueError, match=kw):
            env.scripted_actions_device("space_greedy", **{kw: reach[:60].view(torch.uint16).view(5, 3, 4)})
    torch.cuda.synchronize()
    assert env.stats()["env_steps"] == 0
    env.close()
