"""Head distances, the Voronoi owner map and the owned counts on the device (msnake_head_fields) against
tests/heads_play.py.

Everything is bit-exact and nothing is left out of a comparison: every env, plane, cell and count.  The expectation is
heads_play.np_heads on the canonical state of the CPU oracle or on a hand-built state dict, never the library under
test.  Every output sits between guard elements, and the two uint16 buffers start once on a multiple of 4 bytes and once
on an odd multiple of 2.
"""

import itertools

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import heads_play as hp
import path_play as pp
import scripted_play as sp
import space_play as spp

pytestmark = pytest.mark.gpu

N, T, O = hp.NONE, hp.OWNER_TIE, hp.OWNER_NONE
_st, _mk, _states, _install = bs.state, gh.make_env, gh.oracle_states, gh.install
SENT, SENT8 = 0xA5A5, 0xA5   # the sentinels of the uint16 buffers and of the owner bytes (neither is a value of the contract here)


# ------------------------------------------------------------------------------------------ expectations
def expected(states, dim, ns, sel=None):
    """(dist uint16 [E, P, dim, dim], owner uint8 [E, dim, dim], counts uint16 [E, ns]) of np_heads on canonical state
    dicts; sel: the selected snakes in ascending order (default all)."""
    sel = list(range(ns)) if sel is None else list(sel)
    res = [hp.np_heads(st, dim, ns) for st in states]
    D = np.array([r[0] for r in res]).reshape(len(states), ns, dim, dim)
    assert ((D == N) | (D <= dim * dim - 1)).all()
    owner = np.array([r[1] for r in res], np.uint8).reshape(len(states), dim, dim)
    counts = np.array([r[2] for r in res]).reshape(len(states), ns)
    return D[:, sel].astype(np.uint16), owner, counts.astype(np.uint16)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, policy="safe_greedy", **kw)


def Guarded(env, sel=None, shift=0, actions=False):
    """dist uint16 [n, P, dim, dim], owner uint8 [n, dim, dim], counts uint16 [n, ns], each between guard elements.
    shift = 1 starts the two uint16 payloads one element later (2-byte aligned and no more) and the owner bytes one byte
    later.  actions: with the action and mask buffers of gpu_harness.action_spec in front."""
    dim, ns = int(env.cfg.dim), env.n_snakes
    P = ns if sel is None else len(sel)
    u16 = dict(dtype="uint16", fill=SENT, offset=2 * shift, align=4)
    spec = dict(gh.action_spec(env)) if actions else {}
    spec.update(dist=dict(u16, shape=(env.num_envs, P, dim, dim)), counts=dict(u16, shape=(env.num_envs, ns)),
                owner=dict(dtype="uint8", fill=SENT8, offset=shift, align=4, shape=(env.num_envs, dim, dim)))
    buf = gh.GuardedOutputs(env.device, spec)
    assert buf.dist.data_ptr() % 4 == 2 * shift and buf.counts.data_ptr() % 4 == 2 * shift and buf.owner.data_ptr() % 4 == shift
    return buf


def _diff(what, name, got, want, states):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, name, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist(), states[bad[0][0]])


def _check_call(env, states, buf=None, what="", want=None):
    """One call with all three outputs and every plane, compared for every env, plane, cell and count; then the owner
    map and the counts without a plane (the race alone), which must come out the same."""
    dim, ns = int(env.cfg.dim), env.n_snakes
    buf = buf or Guarded(env)
    want = want or expected(states, dim, ns)
    buf.refill()
    got = env.head_fields_device(dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
    assert [t.data_ptr() for t in got] == [buf.dist.data_ptr(), buf.owner.data_ptr(), buf.counts.data_ptr()]
    for name, w in zip(("dist", "owner", "counts"), want):
        _diff(what, name, buf.host(name), w, states)
    assert buf.guards_intact(), what
    buf.refill()
    env.head_fields_device(owner_out=buf.owner, counts_out=buf.counts, dist=False)
    _diff(what, "owner without planes", buf.host("owner"), want[1], states)
    _diff(what, "counts without planes", buf.host("counts"), want[2], states)
    assert buf.untouched("dist") and buf.guards_intact(), what
    return want


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("dim,ns", [(2, 1), (2, 3), (3, 2), (3, 3), (6, 1), (6, 3), (19, 2), (19, 3), (32, 3), (33, 1), (33, 3),
                                    (62, 2), (62, 3)])
def test_hand_built_snake_env_states(dim, ns):
    """Border and corner heads, heads at -1 / dim, random bodies, stacked duplicates, empty bodies, dense boards, heads
    stacked on one cell, a snake that cannot move."""
    rng = np.random.default_rng([31, dim, ns])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 16, dup=True)
    if ns > 1:
        states += bs.dense_states(dim, ns, ns, rng, 16 if dim < 62 else 6)
    states.append(_st([[]] * ns, [(0, 0)] * ns))                                        # empty bodies: nothing is reached
    states.append(_st([[(dim - 1, dim - 1)]] * ns, [(0, 0)] * ns))                      # every head on one cell
    states.append(_st([[(0, 0), (1, 0), (0, 1)]] + [[(dim - 1, 0)]] * (ns - 1), [(0, 0)] * ns))   # snake 0 cannot move
    states.append(_st([[(-1, 0)]] + [[(dim, dim - 1)]] * (ns - 1), [(0, 0)] * ns))      # every head outside, one move in
    env = _install(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states)
    want = expected(states, dim, ns)
    assert (want[0][-4] == N).all() and (want[1][-4] == O).all() and (want[2][-4] == 0).all()
    assert (want[0][-3][:, dim - 1, dim - 1] == 0).all() and (want[2][-3] == 0).all() == (ns > 1)
    assert want[0][-2][0, 0, 0] == 0 and (want[0][-2][0] != N).sum() == 1 and want[2][-2][0] == 0
    assert want[0][-1][0, 0, 0] == 1 and (want[0][-1] != 0).all() and want[0][-1][0, dim - 1, dim - 1] == 2 * dim - 1
    _check_call(env, states, Guarded(env, shift=(dim + ns) % 2), what=("snake_env", dim, ns), want=want)
    env.close()


@pytest.mark.parametrize("dim", [6, 10])
def test_hand_built_new_world_states_with_four_snakes(dim):
    """Four snakes, some dead with their bodies kept (alive False, in and out of dead_snakes): the alive bit plays no
    part, a kept body races like any other."""
    ns, nf = 4, 5
    rng = np.random.default_rng([32, dim])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 30, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 30)
    for st in states[::2]:
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    states.append(_st([[(0, 0)], [(dim - 1, dim - 1), (dim - 2, dim - 1)], [], [(0, dim - 1)]], [(1, 1)] * nf,
                      alive=[True, False, True, True], in_dead=[False, True, False, False]))
    env = _install(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)
    want = _check_call(env, states, what=("new_world", dim))
    assert want[2][-1][1] > 0 and want[2][-1][2] == 0 and (want[0][-1][2] == N).all()   # the dead snake owns cells, the empty one none
    env.close()


@pytest.mark.parametrize("dim", [6, 19])
def test_hand_built_adversarial_states(dim):
    ns = 3
    rng = np.random.default_rng([33, dim])
    states = bs.border_states(dim, ns, ns, rng)[-14:] + bs.dense_states(dim, ns, 70, rng, 12, fruit_lo=-1, fruit_hi=dim + 1)
    states += bs.random_states(dim, ns, 5, rng, 12)
    env = _install(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)
    _check_call(env, states, Guarded(env, shift=1), what=("adversarial", dim))
    env.close()


def test_heads_outside_the_grid_in_closed_form():
    """Heads at -1 and dim on every side of a 7x7 board, alone: the plane is 1 + the L1 distance from the one target, no
    cell holds a 0, and the snake owns the whole board."""
    dim = 7
    heads = [(-1, y) for y in (0, 3, 6)] + [(dim, y) for y in (0, 3, 6)] + [(x, -1) for x in (0, 3, 6)] + [(x, dim) for x in (0, 3, 6)]
    states = [_st([[h]], [(3, 3)]) for h in heads]
    env = _install(dict(rules=0, dim=dim, n_snakes=1, n_fruits=1), states)
    buf = Guarded(env, shift=1)
    _check_call(env, states, buf, what="outside")
    env.head_fields_device(dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
    D, owner, counts = buf.host("dist"), buf.host("owner"), buf.host("counts")
    for e, (hx, hy) in enumerate(heads):
        tx, ty = min(max(hx, 0), dim - 1), min(max(hy, 0), dim - 1)
        for x in range(dim):
            for y in range(dim):
                assert D[e, 0, x, y] == 1 + abs(x - tx) + abs(y - ty), (e, x, y)
        assert (owner[e] == 0).all() and counts[e, 0] == dim * dim
    env.close()


# ------------------------------------------------------------------------------------------ 2. parity and ties at the word boundary
@pytest.mark.parametrize("dim", [39, 40])
def test_ties_and_parity_across_columns_31_32_33(dim):
    """Two heads on one row (the race runs inside a lane's 64-bit mask, across its two dwords) and on one column (from
    lane to lane), an even and an odd number of cells apart, on the borders, in the middle and in the corners; on an
    open board and with the row walled in.  With an even gap the whole line c0 = mid between them is a tie."""
    states, mids = [], []
    for mid in (31, 32, 33):
        for r in (0, dim // 2, dim - 1):
            for k in (1, min(mid, dim - 1 - mid)):
                for odd in (0, 1):
                    a, b = (mid - k, r), (mid + k + odd, r)
                    if b[0] >= dim:
                        continue
                    wall = [(x, r + d) for d in (-1, 1) if 0 <= r + d < dim for x in range(dim)]
                    for tail in ([], wall):       # the wall is snake 0's own far pieces: no third head looks into the row
                        states.append(_st([[a] + tail, [b], []], [(0, 0)] * 3))
                        states.append(_st([[a[::-1]] + [c[::-1] for c in tail], [b[::-1]], []], [(0, 0)] * 3))
                        mids += [(mid, r, odd, False, bool(tail)), (mid, r, odd, True, bool(tail))]
    for a, b in (((0, 0), (dim - 1, dim - 1)), ((0, dim - 1), (dim - 1, 0)), ((0, 0), (dim - 1, 0)), ((0, 0), (0, dim - 1))):
        states.append(_st([[a], [b], []], [(0, 0)] * 3))
        mids.append(None)
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    buf = Guarded(env, shift=dim % 2)
    _check_call(env, states, buf, what=("columns", dim))
    env.owner_map_device(out=buf.owner)
    owner = buf.host("owner")
    ties = 0
    for e, m in enumerate(mids):
        if m is None:
            continue
        mid, r, odd, transposed, walled = m
        o = owner[e].T if transposed else owner[e]
        if not odd:
            assert o[mid, r] == T and (walled or (o[mid] == T).all()), (e, m)   # the tie line, in the corridor or on the whole board
            ties += 1
        else:
            assert o[mid, r] == 0 and o[mid + 1, r] == 1 and not (o[:, r] == T).any(), (e, m)
    assert ties >= 30
    env.close()


# ------------------------------------------------------------------------------------------ 3. the longest races
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("dim", [6, 33, 62])
def test_serpentine_mazes(dim, transposed):
    """One corridor through the whole board (1 953 cells at dim 62), along the rows (the front runs inside the lanes'
    masks) and transposed (from lane to lane): the most levels a race can have.  Snake 1 is the wall.  Env 0: snake 0 on
    the corridor's first cell; env 1: snake 0 on the first and snake 2 on the last cell; env 2: snake 0 on the last cell.
    Every distance along the corridor is known in closed form and is checked without the helper."""
    walls, corridor = spp.serpentine(dim, transposed)
    L = len(corridor)
    assert L == {6: 21, 33: 577, 62: 1953}[dim]
    states = [_st([[corridor[0]], walls, []], [(0, 0)] * 3), _st([[corridor[0]], walls, [corridor[-1]]], [(0, 0)] * 3),
              _st([[corridor[-1]], walls, []], [(0, 0)] * 3)]
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    buf = Guarded(env, shift=1)
    _check_call(env, states, buf, what=("maze", dim, transposed))
    env.head_fields_device(dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
    D, owner, counts = buf.host("dist"), buf.host("owner"), buf.host("counts")
    gate = 2 * dim                                   # the wall's head enters the corridor at its cell 2 dim
    for k, c in enumerate(corridor):
        assert D[0, 0][c] == k and D[2, 0][c] == L - 1 - k and D[0, 2][c] == N and D[2, 2][c] == N, k
        assert D[1, 0][c] == (k if k < L - 1 else N) and D[1, 2][c] == (L - 1 - k if k > 0 else N), k
        # the wall's head also looks at the corridor's first cell, which only env 2 leaves free
        assert D[0, 1][c] == (1 + abs(k - gate) if k > 0 else N) and D[1, 1][c] == (1 + abs(k - gate) if 0 < k < L - 1 else N), k
        assert D[2, 1][c] == (1 + min(k, abs(k - gate)) if k < L - 1 else N), k
        if 0 < k < L - 1:                            # env 1: the nearest of the three
            d = [k, 1 + abs(k - gate), L - 1 - k]
            assert owner[1][c] == (d.index(min(d)) if d.count(min(d)) == 1 else T), k
    assert D[0, 0][corridor[-1]] == L - 1 and (D[0, 0] != N).sum() == L and (D[2, 0] != N).sum() == L
    for e, free in ((0, L - 1), (1, L - 2), (2, L - 1)):
        assert int(counts[e].sum()) + int((owner[e] == T).sum()) == free and (owner[e] != O).sum() == free, e
    env.close()


# ------------------------------------------------------------------------------------------ 4. overflow ring
@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (0, 19, 3), (1, 12, 2), (2, 10, 3), (0, 20, 3)])
def test_walls_in_the_overflow_ring(rules, dim, ns):
    """Pieces with an index >= 64 wall a region off: with them a distance is NONE, without them finite.  Installed in the
    library and the oracle alike, compared after the install and after each of a few steps under safe_greedy, which
    change the distances."""
    import torch
    from oracle.snake_oracle import state_to_flat
    states, walled = bs.overflow_states(dim, ns)
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="safe_greedy")
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    old_piece_decides, changed, prev = 0, 0, None
    buf = Guarded(env)
    for t in range(3):
        cur = _states(ora)
        for st in cur:     # the cases this test is there for, from the oracle's state: pieces >= 64 decide a distance
            cut = dict(st, snakes=[b[:64] for b in st["snakes"]])
            old_piece_decides += not np.array_equal(hp.np_heads(st, dim, ns)[0], hp.np_heads(cut, dim, ns)[0])
        want = _check_call(env, cur, buf, what=("overflow", t))
        changed += prev is not None and not np.array_equal(prev, want[0])
        prev = want[0]
        act = np.array([sp.safe_greedy(st, dim, ns, None) for st in cur], np.int32)
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert old_piece_decides >= (3 if walled else 1) and changed == 2, (old_piece_decides, changed)
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 5. closed loop
def _closed_loop(cfg, env, steps, **kw):
    """gpu_harness.closed_loop under safe_greedy with the three outputs compared behind the actions and the mask at every
    step.  Even steps write every plane, odd steps the race alone: then the plane buffer must keep its sentinel."""
    dim, ns = cfg["dim"], cfg["n_snakes"]
    step = [-1]

    def want(states):
        step[0] += 1
        act = np.array([sp.safe_greedy(st, dim, ns, None) for st in states], np.int32).reshape(len(states), ns)
        mask = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(len(states), ns)
        D, owner, counts = expected(states, dim, ns)
        return act, mask, D if step[0] % 2 == 0 else np.full_like(D, SENT), owner, counts

    def call(env, buf, snakes):
        buf.refill(["dist", "owner", "counts"])
        out, safe = env.scripted_actions_device("safe_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe)
        planes = dict(dist_out=buf.dist) if step[0] % 2 == 0 else dict(dist=False)
        env.head_fields_device(owner_out=buf.owner, counts_out=buf.counts, **planes)
        return out, safe, buf.host("dist"), buf.host("owner"), buf.host("counts")

    gh.closed_loop(cfg, env, call, want, steps, buffers=lambda env, stride: Guarded(env, actions=True, shift=1), **kw)


@pytest.mark.parametrize("name", ["S19x3", "A10x3", "N10x4"])
def test_closed_loop_with_the_oracle_as_master(name):
    cfg = _cfg(name, num_envs=4)
    env = _mk(cfg)
    _closed_loop(cfg, env, 200, obs_every=199)
    env.close()


# ------------------------------------------------------------------------------------------ 6. layout
@pytest.mark.parametrize("record_policy", ["full", "short"])
@pytest.mark.parametrize("epb", [1, 4, 8])
def test_record_policies_and_envs_per_block(record_policy, epb):
    cfg = _cfg("S19x3", num_envs=37)   # ragged: no multiple of any envs_per_block, nor of the kernel's waves per block
    env = _mk(cfg, record_policy=record_policy, envs_per_block=epb)
    _closed_loop(cfg, env, 8, obs_every=7)
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
    cfg = _cfg(name, num_envs=32)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    rng = np.random.default_rng(3)
    tape = rng.integers(0, 5, (25, 32, cfg["n_snakes"])).astype(np.int32)
    tape[:, :, :] = np.where(rng.random(tape.shape) < 0.5, tape, 2)   # long runs in one direction too
    env.rollout_device(torch.from_numpy(tape).to(env.device), persistent=True, keep_obs=False)
    for t in range(25):
        ora.step(tape[t], want_obs=False)
    _check_call(env, _states(ora), what=name)
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
        if o_done.any() and t % 4 == 0:
            _check_call(env, _states(ora), buf, what=("finished envs in place", t))
            env.reset_device(mask=done)
            ora.reset_envs(o_done, obs=None, final_obs=None, truncated=None)
            resets += int(o_done.sum())
            _check_call(env, _states(ora), buf, what=("after reset_envs", t))
    assert resets >= 10
    env.close()


# ------------------------------------------------------------------------------------------ 7. selections and outputs
def _played(n, ns_name="S19x3", steps=12):
    cfg = _cfg(ns_name, num_envs=n)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    gh.play_random(env, ora, steps, np.random.default_rng(n), threads=1)
    return cfg, env, _states(ora)


def test_every_snake_mask_subset_and_the_plane_order():
    """Each of the 7 selections of 3 snakes: the planes are the selected snakes' in ascending order, and the owner map
    and the counts are the same under every one of them."""
    cfg, env, states = _played(21)
    D, owner, counts = expected(states, 19, 3)
    assert len({D[:, s].tobytes() for s in range(3)}) == 3          # the planes differ: a wrong order shows
    for sel in [list(c) for k in (1, 2, 3) for c in itertools.combinations(range(3), k)]:
        for shift in (0, 1):
            buf = Guarded(env, sel, shift=shift)
            assert env.head_fields_shape(sel) == (len(sel), 19, 19)
            got = env.head_fields_device(sel, dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
            assert len(got) == 3
            _diff(sel, "dist", buf.host("dist"), D[:, sel], states)
            _diff(sel, "owner", buf.host("owner"), owner, states)
            _diff(sel, "counts", buf.host("counts"), counts, states)
            assert buf.guards_intact(), sel
            buf.refill()
            assert env.head_distances_device(sel if len(sel) > 1 else sel[0], out=buf.dist) is buf.dist   # planes alone: only these fronts run
            _diff(sel, "dist alone", buf.host("dist"), D[:, sel], states)
            assert buf.untouched("owner") and buf.untouched("counts") and buf.guards_intact(), sel
    env.close()


@pytest.mark.parametrize("dim", [36, 37, 62])
def test_plane_counts_on_both_sides_of_the_staging_size(dim):
    """The planes leave through an LDS image while one wave's planes fit 8 KiB and straight to HBM beyond: three planes fit
    at 36x36 and not at 37x37, one plane of 62x62 fits and two do not.  Every selection size on the same states, alone and
    with the race, at both alignments; the owner map and the counts do not depend on it."""
    rng = np.random.default_rng([34, dim])
    states = bs.random_states(dim, 3, 3, rng, 6, dup=True) + bs.dense_states(dim, 3, 3, rng, 6) + bs.border_states(dim, 3, 3, rng)[-12::2]
    env = _install(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    D, owner, counts = expected(states, dim, 3)
    sides = set()
    for sel in ([1], [0, 2], [0, 1, 2]):
        sides.add(len(sel) * ((dim * dim + 1) // 2) * 4 <= 8192)
        for shift in (0, 1):
            buf = Guarded(env, sel, shift=shift)
            env.head_distances_device(sel, out=buf.dist)
            _diff((dim, sel), "dist alone", buf.host("dist"), D[:, sel], states)
            assert buf.guards_intact() and buf.untouched("owner") and buf.untouched("counts"), (dim, sel)
            buf.refill()
            env.head_fields_device(sel, dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
            _diff((dim, sel), "dist", buf.host("dist"), D[:, sel], states)
            _diff((dim, sel), "owner", buf.host("owner"), owner, states)
            _diff((dim, sel), "counts", buf.host("counts"), counts, states)
            assert buf.guards_intact(), (dim, sel)
    assert sides == ({True} if dim == 36 else {True, False})
    env.close()


@pytest.mark.parametrize("name,shift", [("S19x3", 0), ("N10x4", 1)])
def test_every_output_combination_leaves_the_others_untouched(name, shift):
    import torch
    cfg, env, states = _played(13, name, 6)
    dim, ns = cfg["dim"], cfg["n_snakes"]
    want = dict(zip(("dist", "owner", "counts"), expected(states, dim, ns)))
    buf = Guarded(env, shift=shift)
    for pick in itertools.product((False, True), repeat=3):
        if not any(pick):
            continue                                                           # nothing to write: an argument error (below)
        names = [n for n, on in zip(("dist", "owner", "counts"), pick) if on]
        buf.refill()
        got = env.head_fields_device(**{n + "_out": getattr(buf, n) for n in names}, **{n: False for n in want if n not in names})
        got = got if isinstance(got, tuple) else (got,)
        assert [t.data_ptr() for t in got] == [getattr(buf, n).data_ptr() for n in names], names
        for n in want:
            if n in names:
                _diff(names, n, buf.host(n), want[n], states)
            else:
                assert buf.untouched(n), (names, n)
        assert buf.guards_intact(), names
    # fresh tensors of the env's own: dtypes, shapes, values
    d, o, c = env.head_fields_device()
    assert (d.dtype, o.dtype, c.dtype) == (torch.uint16, torch.uint8, torch.uint16)
    assert tuple(d.shape) == (13, ns, dim, dim) and tuple(o.shape) == (13, dim, dim) and tuple(c.shape) == (13, ns)
    assert np.array_equal(d.cpu().numpy(), want["dist"]) and np.array_equal(o.cpu().numpy(), want["owner"])
    assert np.array_equal(c.cpu().numpy(), want["counts"])
    assert np.array_equal(env.owner_map_device().cpu().numpy(), want["owner"])
    assert np.array_equal(env.owned_counts_device().cpu().numpy(), want["counts"])
    assert np.array_equal(env.head_distances_device(ns - 1).cpu().numpy(), want["dist"][:, ns - 1:])
    env.close()


# ------------------------------------------------------------------------------------------ 8. read-only
def test_the_call_changes_no_state():
    import torch
    cfg = _cfg("A10x3", num_envs=40)
    env, plain = _mk(cfg), _mk(cfg)
    assert np.array_equal(env.reset(), plain.reset())
    rng = np.random.default_rng(8)
    buf = Guarded(env)
    for t in range(60):
        act = torch.from_numpy(rng.integers(0, 5, (40, 3)).astype(np.int32)).to(env.device)
        if t % 20 == 0:
            before, st_before = env.get_state_all().tobytes(), env.stats()
        env.head_fields_device(dist_out=buf.dist, owner_out=buf.owner, counts_out=buf.counts)
        env.head_distances_device([1])
        env.owned_counts_device(out=buf.counts)
        if t % 20 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before   # state blob, Philox counters, totals
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 60 * 40   # the call adds nothing to env_steps
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 9. HIP graph
def test_graph_of_head_fields_then_step():
    """[safe_greedy -> msnake_head_fields -> msnake_step -> msnake_head_fields] captured as one linear chain and replayed
    50 times on 32 envs: the outputs in front of the last step and behind it, the rewards and the final state against
    the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = _cfg("S19x3", num_envs=32)
    K, n = 50, 32
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((n, 3), dtype=torch.int32, device=env.device)
    front, behind = Guarded(env, shift=1), Guarded(env)

    def chain():
        env.scripted_actions_device("safe_greedy", out=acts)
        env.head_fields_device(dist_out=front.dist, owner_out=front.owner, counts_out=front.counts)
        out = env.step_device(acts)
        env.head_fields_device(dist_out=behind.dist, owner_out=behind.owner, counts_out=behind.counts)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = chain()
    torch.cuda.synchronize()
    env.set_state_all(blob)
    rews = []
    for _ in range(K):
        g.replay()
        rews.append(out[1].clone())
    torch.cuda.synchronize()
    o_rews = []
    for _ in range(K):
        states = _states(ora)
        act = np.array([sp.safe_greedy(st, 19, 3, None) for st in states], np.int32)
        o_rews.append(ora.step(act)[1].copy())
    for buf, st in ((front, states), (behind, _states(ora))):
        for name, w in zip(("dist", "owner", "counts"), expected(st, 19, 3)):
            _diff("graph", name, buf.host(name), w, st)
        assert buf.guards_intact()
    assert np.array_equal(torch.stack(rews).cpu().numpy(), np.stack(o_rews))
    for e in range(n):
        assert flat_to_state(env.get_state_words(e)) == ora.get_state(e), e
    env.close()


# ------------------------------------------------------------------------------------------ 10. against the siblings, on the device
@pytest.mark.parametrize("name", ["S19x3", "N10x4"])
def test_counts_against_territory_and_planes_against_paths_on_one_handle(name):
    """Identity 2 and identity 3 of heads_play's host tests between the library's own outputs: the owned counts lie
    between the largest and the sum of territory_device()'s per-move counts, and the smallest plane entry over
    fruit_field_device()'s sources is 1 + the smallest entry of path_device()."""
    cfg, env, _ = _played(64, name, 6)    # (random play dies young: six steps in, most snakes still have a way to a fruit)
    dist, owner, counts = (t.cpu().numpy().astype(np.int64) for t in env.head_fields_device())
    terr = env.territory_device().cpu().numpy().astype(np.int64)
    path = env.path_device().cpu().numpy().astype(np.int64)
    field = env.fruit_field_device().cpu().numpy()
    assert (terr.max(2) <= counts).all() and (counts <= terr.sum(2)).all()
    finite = 0
    for e in range(64):
        src = field[e] == 0
        for s in range(cfg["n_snakes"]):
            best = int(path[e, s].min())
            want = N if best == pp.NONE or not src.any() else 1 + best
            assert (int(dist[e, s][src].min()) if src.any() else N) == want, (e, s)
            finite += want != N
    assert finite >= 64
    env.close()


# ------------------------------------------------------------------------------------------ 11. errors
def test_argument_errors_and_their_order():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=3, rules="snake_env", seed=0)
    env.reset()
    L = env._L
    dist = torch.full((5 * 3 * 361 + 1,), 9, dtype=torch.int16, device=env.device)
    owner = torch.full((5 * 361 + 1,), 9, dtype=torch.uint8, device=env.device)
    counts = torch.full((5 * 3 + 1,), 9, dtype=torch.int16, device=env.device)
    pd, po, pc = dist.data_ptr(), owner.data_ptr(), counts.data_ptr()

    def call(h, mask, d, o, c):
        rc = L.msnake_head_fields(h, mask, d, o, c, None)
        return rc, L.msnake_last_error().decode()

    # MSNAKE_E_ARG in the header's order: the mask's range, planes without a selection, nothing to write; each wins
    # over an alignment error in the same call
    for args, word in (((env._h, 0b1000, pd, po, pc), "snake_mask 0x8"), ((env._h, 0b1000, None, None, None), "snake_mask 0x8"),
                       ((env._h, 0b1001, pd + 1, None, pc + 1), "snake_mask 0x9"),
                       ((env._h, 0, pd, po, pc), "snake_mask is 0"), ((env._h, 0, pd + 1, None, None), "snake_mask is 0"),
                       ((env._h, 0, None, None, None), "nothing to write"), ((env._h, 0b101, None, None, None), "nothing to write")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg and "msnake_head_fields" in msg, (args[1:], rc, msg)
    rc, msg = call(env._h, 0b1, pd + 1, po, pc)
    assert rc < 0 and rc != -1 and "dist_dev" in msg, (rc, msg)        # MSNAKE_E_ALIGN
    rc2, msg = call(env._h, 0, None, po, pc + 1)
    assert rc2 == rc and "counts_dev" in msg, (rc2, msg)
    assert call(None, 1, pd, po, pc)[0] == -3                          # MSNAKE_E_HANDLE
    torch.cuda.synchronize()
    assert (dist.cpu().numpy() == 9).all() and (owner.cpu().numpy() == 9).all() and (counts.cpu().numpy() == 9).all()
    # what is NOT an error: any output alone, the owner bytes at any address, a selection without planes
    assert call(env._h, 0b111, pd, None, None)[0] == 0 and call(env._h, 0, None, po + 1, None)[0] == 0
    assert call(env._h, 0, None, None, pc)[0] == 0 and call(env._h, 0b10, pd + 2, po, pc + 2)[0] == 0
    assert call(env._h, 0b11, None, po, None)[0] == 0
    with pytest.raises(ValueError, match="snakes"):
        env.head_fields_device([2, 1])
    with pytest.raises(ValueError, match="owner_out"):
        env.head_fields_device(owner_out=owner[:1805].view(5, 19, 19).to(torch.int8))
    torch.cuda.synchronize()
    assert env.stats()["env_steps"] == 0
    env.close()
