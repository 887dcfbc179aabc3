"""BFS fruit distances, the distance field and the opponent path_greedy on the device (msnake_path_actions) against
tests/path_play.py.

Everything is bit-exact and nothing is left out of a comparison: every env, snake, move and field cell.  The expected
field is path_play.np_field, the expected paths path_play.np_path, the expected actions path_play.path_greedy with
eps = 0, the expected mask scripted_play.np_safe_mask, all on the canonical state of the CPU oracle or on a hand-built
state dict; none of them ever comes from the library under test.  Every output sits between guard elements.  The kernel
reads the levels off in two ways, with the staged field (field_dev given) and without it: every check call runs both.
"""

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import path_play as pp
import scripted_play as sp
import space_play as spp

pytestmark = pytest.mark.gpu

NONE = pp.NONE
_st, _mk, _states, _install = bs.state, gh.make_env, gh.oracle_states, gh.install
FILL, SENT = -77, 0xA5A5   # the sentinels of the action buffer (gpu_harness.action_spec) and of the uint16 buffers


# ------------------------------------------------------------------------------------------ expectations
def expected(states, dim, ns):
    """(actions int32 [E, ns], masks uint8 [E, ns], paths uint16 [E, ns, 4], fields uint16 [E, dim, dim]) of the helpers
    on canonical state dicts."""
    E = len(states)
    act = np.array([pp.path_greedy(st, dim, ns) for st in states], np.int32).reshape(E, ns)
    mask = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(E, ns)
    field = np.array([pp.np_field(st, dim) for st in states]).reshape(E, dim, dim)
    path = np.array([pp.np_path(st, dim, ns, f) for st, f in zip(states, field)]).reshape(E, ns, 4)
    assert ((field == NONE) | (field <= dim * dim - 2)).all()
    # the statements agree with each other: a finite path belongs to an open move, and the action is an open move or 0
    is_open = (mask[:, :, None] >> np.arange(1, 5)) & 1 == 1
    assert not (~is_open & (path != NONE)).any()
    chosen = np.take_along_axis(np.concatenate([np.ones((E, ns, 1), bool), is_open], 2), act[:, :, None], 2)
    assert chosen.all()
    return act, mask, path.astype(np.uint16), field.astype(np.uint16)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, policy="path_greedy", **kw)


def Guarded(env, stride=None, shift=0):
    """Actions, mask, a uint16 [n, ns, 4] buffer `path` and a uint16 [n, dim, dim] buffer `field`, each between guard
    elements.  shift = 1 starts the two uint16 payloads one element later: 2-byte aligned and no more."""
    dim = int(env.cfg.dim)
    u16 = dict(dtype="uint16", fill=SENT, offset=2 * shift, align=4)
    buf = gh.GuardedOutputs(env.device, dict(gh.action_spec(env, stride), path=dict(u16, shape=(env.num_envs, env.n_snakes, 4)),
                                             field=dict(u16, shape=(env.num_envs, dim, dim))))
    assert buf.path.data_ptr() % 4 == 2 * shift and buf.field.data_ptr() % 4 == 2 * shift
    return buf


def _diff(what, name, got, want, states):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, name, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist(), states[bad[0][0]])


def _check_call(env, states, buf=None, what="", want=None):
    """One call with all four outputs (the staged field) and one with all but the field (the read-off without it), each
    compared for every env, snake, move and cell; returns the expected actions."""
    dim, ns = env.cfg.dim, env.n_snakes
    buf = buf or Guarded(env)
    want_a, want_m, want_p, want_f = want or expected(states, dim, ns)
    buf.refill()
    out, safe, path, field = env.scripted_actions_device("path_greedy", out=buf.act, safe_out=buf.safe, path_out=buf.path,
                                                         field_out=buf.field)
    _diff(what, "field", buf.host("field"), want_f, states)
    _diff(what, "path", buf.host("path"), want_p, states)
    _diff(what, "mask", safe.cpu().numpy(), want_m, states)
    _diff(what, "action", out.cpu().numpy()[:, :ns], want_a, states)
    assert buf.guards_intact(), what
    buf.refill()
    out, safe, path = env.scripted_actions_device("path_greedy", out=buf.act, safe_out=buf.safe, path_out=buf.path)
    _diff(what, "path without the field", buf.host("path"), want_p, states)
    _diff(what, "mask without the field", safe.cpu().numpy(), want_m, states)
    _diff(what, "action without the field", out.cpu().numpy()[:, :ns], want_a, states)
    assert buf.untouched("field") and buf.guards_intact(), what
    return want_a


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim", [2, 3, 6, 19, 32, 33, 62])
def test_hand_built_snake_env_states(dim):
    """Border and corner heads, heads at -1 / dim, random bodies, stacked duplicates, empty bodies, dense boards; fruits
    under bodies and duplicated fruits come with the random draws and are counted."""
    ns = 3
    rng = np.random.default_rng([17, dim])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 24, dup=True)
    states += bs.dense_states(dim, ns, ns, rng, 24 if dim < 62 else 10)
    states.append(_st([[], [], []], [(0, 0)] * ns))                        # empty bodies: every path NONE, the field is whole
    states.append(_st([[(0, 0)], [(dim - 1, dim - 1)], []], [(0, 0), (dim - 1, dim - 1), (0, 0)]))   # every fruit under a head
    states.append(_st([[(0, 0)], [], []], [(dim - 1, dim - 1)] * ns))      # one fruit three times, the far corner
    under = sum(any(list(f) in b for b in st["snakes"]) for st in states for f in st["fruits"])
    dupes = sum(len({tuple(f) for f in st["fruits"]}) < len(st["fruits"]) for st in states)
    assert under >= 10 and dupes >= 3, (under, dupes)
    env = _install(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want = expected(states, dim, ns)
    assert (want[3][-3] != NONE).all() and (want[2][-3] == NONE).all() and (want[3][-2] == NONE).all()
    if dim > 2:
        assert want[3][-1][0, 1] == 2 * (dim - 1) - 1
    _check_call(env, states, Guarded(env, shift=dim % 2 == 0), what=("snake_env", dim), want=want)
    env.close()


@pytest.mark.parametrize("dim", [6, 10])
def test_hand_built_new_world_states_with_four_snakes(dim):
    """Four snakes, some dead with their bodies kept (alive False, in and out of dead_snakes), stacked duplicates."""
    ns, nf = 4, 5
    rng = np.random.default_rng([18, dim])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 30)
    for st in states[::2]:
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    # a kept, stacked, dead body walls the fruit at (0, 1) in with snake 0 and keeps snake 3 from it
    states.append(_st([[(0, 0)], [(1, 0), (1, 0), (1, 1), (0, 2), (1, 2)], [], [(3, 3)]], [(0, 1)] * nf,
                      alive=[True, False, True, True], in_dead=[False, True, False, False]))
    env = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    P = pp.np_path(states[-1], dim, ns)
    assert P[0].tolist() == [NONE, 0, NONE, NONE] and (P[3] == NONE).all() and (P[2] == NONE).all()
    _check_call(env, states, what=("new_world", dim))
    env.close()


@pytest.mark.parametrize("dim", [6, 19])
def test_hand_built_adversarial_states_with_long_fruit_lists(dim):
    """Fruit lists of 0, 1, 63, 64, 65 entries and up to the list's capacity, entries at -1 / dim included, on dense
    boards; and the only reachable fruit at a list index >= 64."""
    ns = 3
    rng = np.random.default_rng([19, dim])
    fcap = (3 + 3 * (dim * dim + 2) + 63) // 64 * 64      # the handle's fruit-list capacity
    states = []
    for n_list in (0, 1, 63, 64, 65, min(130, fcap - 3), fcap):   # (dim 6: the capacity is 128 entries)
        for st in bs.dense_states(dim, ns, n_list, rng, 5, fruit_lo=-1, fruit_hi=dim + 1):
            states.append(st)
    h = (dim // 2, dim // 2)
    first = len(states)
    for a in (1, 2, 3, 4):             # the one fruit on the board sits at list index 70, two cells from the head along move a;
        fl = [(-1, -1), (dim, 0), (0, dim), h] * 25                     # the rest lies outside or under the head
        fl[70] = (h[0] + 2 * sp.DIRS[a][0], h[1] + 2 * sp.DIRS[a][1])
        states.append(_st([[h], [], []], fl))
    outside = sum(not (0 <= f[0] < dim and 0 <= f[1] < dim) for st in states[:first] for f in st["fruits"])
    assert outside >= 50, outside
    env = _install(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want = _check_call(env, states, what=("adversarial", dim))
    assert want[first:first + 4, 0].tolist() == [1, 2, 3, 4]
    for k, a in enumerate((1, 2, 3, 4)):
        P = pp.np_path(states[first + k], dim, ns)[0]
        assert P[a - 1] == 1 and sorted(P.tolist()) == [1, 3, 3, 5]
    env.close()


# ------------------------------------------------------------------------------------------ 2. longest paths
def _maze_states(dim, transposed):
    """Snake 1 is the wall of a serpentine maze, snake 0 one cell on corridor cell i, the one fruit on corridor cell j."""
    walls, path = spp.serpentine(dim, transposed)
    L = len(path)
    gaps = [i for i, c in enumerate(path) if c[0 if transposed else 1] % 2 == 1]
    pairs = [(0, L - 1), (L - 1, 0), (L // 2, 0), (L // 2, L - 1), (1, 3), (L - 3, L - 5), (L // 3, L // 3 + 1),
             (gaps[0], L - 1), (gaps[-1], 0), (gaps[len(gaps) // 2], gaps[len(gaps) // 2] + 7)]
    return [_st([[path[i]], walls], [path[j], path[j]]) for i, j in pairs], pairs, path


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes(dim, transposed):
    """The longest paths there are: one corridor through the whole board (1 953 cells at dim 62, 1 951 steps from one
    end to the other), along the rows (the front runs inside the lanes' masks) and transposed (from lane to lane).
    Every distance is known in closed form and is checked without the helper."""
    states, pairs, corridor = _maze_states(dim, transposed)
    L = len(corridor)
    assert L == {6: 21, 33: 577, 62: 1953}[dim]
    env = _install(dict(rules=0, dim=dim, n_snakes=2, n_fruits=2), states)
    buf = Guarded(env)
    _check_call(env, states, buf, what=("maze", dim, transposed))
    env.scripted_actions_device("path_greedy", out=buf.act, path_out=buf.path, field_out=buf.field)
    got_p, got_f, got_a = buf.host("path"), buf.host("field"), buf.act.cpu().numpy()
    longest = 0
    for e, (i, j) in enumerate(pairs):
        head = corridor[i]
        for a, (d0, d1) in sp.DIRS.items():
            t = (head[0] + d0, head[1] + d1)
            if i + 1 < L and t == corridor[i + 1]:
                want = j - i - 1 if j > i else NONE
            elif i > 0 and t == corridor[i - 1]:
                want = i - j - 1 if j < i else NONE
            else:
                want = NONE
            assert got_p[e, 0, a - 1] == want, (e, i, j, a)
            if want != NONE:
                assert got_a[e, 0] == a          # the one move that leads to the fruit
                longest = max(longest, want)
        lo, hi = (i + 1, L) if j > i else (0, i)
        for k, c in enumerate(corridor):          # the field along the whole corridor: the corridor index difference
            assert got_f[e][c] == (abs(k - j) if lo <= k < hi else NONE), (e, k)
        assert (got_f[e] != NONE).sum() == hi - lo
    assert longest == L - 2
    env.close()


# ------------------------------------------------------------------------------------------ 3. overflow ring
@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (0, 19, 3), (1, 12, 2), (2, 10, 3), (0, 20, 3)])
def test_separating_piece_in_the_overflow_ring(rules, dim, ns):
    """Pieces with an index >= 64 wall a region off: with them a distance is NONE, without them finite.  Installed in the
    library and the oracle alike, compared after the install and after each of a few steps under path_greedy."""
    import torch
    from oracle.snake_oracle import state_to_flat
    states, walled = bs.overflow_states(dim, ns)
    states = [dict(st) for st in states]
    for st in states[len(states) - walled:]:
        # the wall of pieces >= 64 lies between snake 1's move 2 and the fruits at (0, 0); move 4 eats
        full = pp.np_path(st, dim, ns)[1]
        cut = pp.np_path(dict(st, snakes=[b[:64] for b in st["snakes"]]), dim, ns)[1]
        assert full[3] == 0 and full[1] == NONE and cut[3] == 0 and cut[1] not in (0, NONE), (full, cut)
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="path_greedy")
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    old_piece_decides = 0
    buf = Guarded(env)
    for t in range(6):
        cur = _states(ora)
        for st in cur:     # the cases this test is there for, from the oracle's state: pieces >= 64 decide a distance
            cut = dict(st, snakes=[b[:64] for b in st["snakes"]])
            old_piece_decides += not np.array_equal(pp.np_path(st, dim, ns), pp.np_path(cut, dim, ns))
        act = _check_call(env, cur, buf, what=("overflow", t))
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert old_piece_decides >= 6, old_piece_decides
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 4. closed loop
def _closed_loop(cfg, env, steps, **kw):
    """gpu_harness.closed_loop under path_greedy with actions, mask and paths.  Even steps ask for the field too, odd
    steps do not (the two read-offs): then the field buffer must keep its sentinel."""
    step = [-1]

    def want(states):
        step[0] += 1
        want_a, want_m, want_p, want_f = expected(states, cfg["dim"], cfg["n_snakes"])
        return want_a, want_m, want_p, want_f if step[0] % 2 == 0 else np.full_like(want_f, SENT)

    def call(env, buf, snakes):
        buf.refill(["field"])
        field = dict(field_out=buf.field) if step[0] % 2 == 0 else {}
        out, safe, *_ = env.scripted_actions_device("path_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe, path_out=buf.path, **field)
        return out, safe, buf.host("path"), buf.host("field")

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
    want_a, want_m, want_p, want_f = expected(states, 10, 4)
    buf = Guarded(env, stride, shift=shift)
    acts_untouched, safe_untouched = lambda: buf.untouched("act"), lambda: buf.untouched("safe")
    path_untouched, field_untouched = lambda: buf.untouched("path"), lambda: buf.untouched("field")
    # path_dev alone
    assert env.path_device(out=buf.path) is buf.path
    assert np.array_equal(buf.host("path"), want_p) and acts_untouched() and safe_untouched() and field_untouched() and buf.guards_intact()
    got = env.path_device()                                                    # a fresh tensor of the env's
    assert got.dtype == __import__("torch").uint16 and np.array_equal(got.cpu().numpy(), want_p)
    # field_dev alone
    buf.refill()
    assert env.fruit_field_device(out=buf.field) is buf.field
    assert np.array_equal(buf.host("field"), want_f) and acts_untouched() and safe_untouched() and path_untouched() and buf.guards_intact()
    got = env.fruit_field_device()
    assert tuple(got.shape) == (13, 10, 10) and np.array_equal(got.cpu().numpy(), want_f)
    # safe_dev alone (an empty selection): no action word, no path and no field is written
    buf.refill()
    out, safe = env.scripted_actions_device("path_greedy", snakes=[], out=buf.act, safe_out=buf.safe)
    assert np.array_equal(safe.cpu().numpy(), want_m) and acts_untouched() and path_untouched() and field_untouched() and buf.guards_intact()
    # actions alone, snakes 3 and 1 only
    buf.refill()
    out = env.scripted_actions_device("path_greedy", snakes=[3, 1], out=buf.act)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [1, 3]], want_a[:, [1, 3]]) and (got[:, [0, 2] + list(range(4, stride))] == FILL).all()
    assert safe_untouched() and path_untouched() and field_untouched() and buf.guards_intact()
    # all four, snake 2 only: the mask, the paths and the field are written for every snake whatever the selection
    buf.refill()
    res = env.scripted_actions_device("path_greedy", snakes=[2], out=buf.act, safe_out=buf.safe, path_out=buf.path, field_out=buf.field)
    assert [t.data_ptr() for t in res] == [buf.act.data_ptr(), buf.safe.data_ptr(), buf.path.data_ptr(), buf.field.data_ptr()]
    got = res[0].cpu().numpy()
    assert np.array_equal(got[:, 2], want_a[:, 2]) and (got[:, [0, 1, 3] + list(range(4, stride))] == FILL).all()
    assert np.array_equal(buf.safe.cpu().numpy(), want_m) and np.array_equal(buf.host("path"), want_p)
    assert np.array_equal(buf.host("field"), want_f) and buf.guards_intact()
    # the results do not depend on which outputs are asked for: every combination, with and without the actions
    names = ("safe_out", "path_out", "field_out")
    for with_actions in (True, False):
        for pick in itertools.product((False, True), repeat=3):
            if not with_actions and not any(pick):
                continue                                                       # nothing to write: an argument error (below)
            kw = {k: getattr(buf, k[:-4]) for k, on in zip(names, pick) if on}
            buf.refill()
            env.scripted_actions_device("path_greedy", snakes=None if with_actions else [], out=buf.act, **kw)
            got = buf.act.cpu().numpy()
            if with_actions:
                assert np.array_equal(got[:, :4], want_a) and (got[:, 4:] == FILL).all(), kw.keys()
            else:
                assert acts_untouched(), kw.keys()
            assert np.array_equal(buf.safe.cpu().numpy(), want_m) if pick[0] else safe_untouched(), kw.keys()
            assert np.array_equal(buf.host("path"), want_p) if pick[1] else path_untouched(), kw.keys()
            assert np.array_equal(buf.host("field"), want_f) if pick[2] else field_untouched(), kw.keys()
            assert buf.guards_intact(), kw.keys()
    # the env's own cached action buffer, shared with the other policies
    a = env.scripted_actions_device("path_greedy", snakes=[2])
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
        env.scripted_actions_device("path_greedy", out=buf.act, safe_out=buf.safe, path_out=buf.path, field_out=buf.field)
        env.path_device(out=buf.path)
        env.fruit_field_device(out=buf.field)
        env.scripted_actions_device("path_greedy", snakes=[1])
        if t % 25 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 100 * 40   # the call adds nothing to env_steps
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 8. HIP graph
def test_graph_of_path_actions_then_step():
    """[msnake_path_actions -> msnake_step] captured as one linear chain and replayed 100 times on 64 envs: final state,
    rewards, last actions and last paths against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = _cfg("S19x3", num_envs=64)
    K = 100
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((64, 3), dtype=torch.int32, device=env.device)
    path = torch.zeros((64, 3, 4), dtype=torch.uint16, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("path_greedy", out=acts, path_out=path)
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("path_greedy", out=acts, path_out=path)
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
    assert np.array_equal(path.cpu().numpy(), want[2])
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
    path = torch.full((5 * 3 * 4 + 1,), 9, dtype=torch.int16, device=env.device)
    field = torch.full((5 * 19 * 19 + 1,), 9, dtype=torch.int16, device=env.device)
    pa, ps, pp_, pf = acts.data_ptr(), safe.data_ptr(), path.data_ptr(), field.data_ptr()

    def call(h, mask, a, stride, s, p, f):
        rc = L.msnake_path_actions(h, mask, a, stride, s, p, f, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 0b1000, pa, 3, None, None, None), "snake_mask"), ((env._h, 0b1000, None, 3, ps, pp_, pf), "snake_mask"),
                       ((env._h, 0b111, pa, 2, None, pp_, None), "action_stride"), ((env._h, 1, None, 3, ps, pp_, pf), "actions_dev"),
                       ((env._h, 0, pa, 3, None, None, None), "nothing to write"),
                       ((env._h, 0, None, 0, None, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg and "msnake_path_actions" in msg, (args[1:], rc, msg)
    rc, msg = call(env._h, 0, None, 0, None, pp_ + 1, None)
    assert rc < 0 and rc != -1 and "path_dev" in msg, (rc, msg)        # MSNAKE_E_ALIGN
    rc2, msg = call(env._h, 0, None, 0, None, pp_, pf + 1)
    assert rc2 == rc and "field_dev" in msg, (rc2, msg)
    assert call(None, 1, pa, 3, None, None, None)[0] == -3
    torch.cuda.synchronize()
    assert (acts.cpu().numpy() == 9).all() and (safe.cpu().numpy() == 9).all()
    assert (path.cpu().numpy() == 9).all() and (field.cpu().numpy() == 9).all()
    # what is NOT an error: action_stride / actions_dev are not looked at when no action is written; any output may be NULL
    assert call(env._h, 0, None, 0, ps, None, None)[0] == 0 and call(env._h, 0, None, 0, None, pp_, None)[0] == 0
    assert call(env._h, 0, None, 0, None, None, pf)[0] == 0 and call(env._h, 0, None, 0, None, pp_ + 2, pf + 2)[0] == 0
    assert call(env._h, 0b101, pa, 3, None, None, None)[0] == 0
    for kw in ("path_out", "field_out"):
        with pytest.raises(ValueError, match=kw):
            env.scripted_actions_device("space_greedy", **{kw: path[:60].view(torch.uint16).view(5, 3, 4)})
    torch.cuda.synchronize()
    assert env.stats()["env_steps"] == 0
    env.close()
