"""On-device scripted opponents and safe-move masks (msnake_scripted_actions) against tests/scripted_play.py.

Everything is bit-exact and nothing is left out of a comparison: every step, env and snake.  The expected actions are
scripted_play.POLICIES[...] with eps = 0 on the canonical state of the CPU oracle (or on a hand-built state dict); the
expected mask is the NumPy statement scripted_play.np_safe_mask.  Neither ever comes from the library under test.
"""

import numpy as np
import pytest

import board_states as bs
import gpu_harness as gh
import scripted_play as sp

pytestmark = pytest.mark.gpu

FILL = -77  # the sentinel of the action buffer (gpu_harness.action_spec)
_st, _mk, _states, _play_random = bs.state, gh.make_env, gh.oracle_states, gh.play_random


# ------------------------------------------------------------------------------------------ expectations
np_safe_mask = sp.np_safe_mask   # the NumPy statement of the mask (shared with tests/op_fuzz.py)


def expected(policy, states, dim, ns):
    """(actions int32 [E, ns], masks uint8 [E, ns]) of the helper / the NumPy mask on canonical state dicts."""
    pol = sp.POLICIES[policy]
    act = np.array([pol(st, dim, ns, None, 0.0) for st in states], np.int32).reshape(len(states), ns)
    return act, np.array([np_safe_mask(st, dim, ns) for st in states], np.uint8).reshape(len(states), ns)


def _cfg(name, **kw):
    return dict(sp.SCENARIOS[name], eps=0.0, **kw)


def _check_call(env, policy, states, buf=None, what=""):
    """One call with actions and mask, compared for every env and snake; returns the expected actions."""
    dim, ns = env.cfg.dim, env.n_snakes
    buf = buf or gh.action_buffers(env)
    want_a, want_m = expected(policy, states, dim, ns)
    out, safe = env.scripted_actions_device(policy, out=buf.act, safe_out=buf.safe)
    got_a, got_m = out.cpu().numpy()[:, :ns], safe.cpu().numpy()
    bad = np.argwhere(got_a != want_a)
    assert bad.size == 0, (what, policy, bad[:5].tolist(), got_a[bad[0][0]], want_a[bad[0][0]], states[bad[0][0]])
    bad = np.argwhere(got_m != want_m)
    assert bad.size == 0, (what, "mask", bad[:5].tolist(), got_m[bad[0][0]], want_m[bad[0][0]], states[bad[0][0]])
    assert buf.guards_intact(), what
    return want_a


# ------------------------------------------------------------------------------------------ 1. closed loop
# the coverage each eps = 0 play is there for (scripted_play.check_coverage, on the ORACLE's numbers); A10x3 without the
# eps of SCENARIOS reaches a fruit list of 57 entries, not 65
LOOP = {"S19x3": ["over64"], "A10x3": ["over64", "fruits40"], "N10x4": ["capped", "over64"], "N10x2": ["capped", "over64"],
        "S10": ["full", "over64", "overflow"], "S6x2": ["full"], "A10": ["full", "capped", "over64"]}
# ... and what the oracle's own eps = 0 plays reach (deterministic; the figures of the CPU oracle alone), as lower bounds
REACH = {"S19x3": dict(longest_body=93, env_steps_over_64=913, episodes=358),
         "A10x3": dict(longest_body=98, env_steps_over_64=156, longest_fruit_list=57, episodes=1464),
         "N10x4": dict(longest_body=75, env_steps_over_64=52, capped_episodes=8, episodes=195),
         "N10x2": dict(longest_body=76, env_steps_over_64=130, capped_episodes=16, episodes=1528),
         "S10": dict(longest_body=100, env_steps_over_64=8758, longest_run_over_64=257, episodes=47),
         "S6x2": dict(longest_body=36, full_env_steps=274), "A10": dict(longest_body=100, capped_episodes=12, env_steps_over_64=2147)}


def _closed_loop(cfg, env, expect, control=None, stride=None, obs_every=50, steps=None):
    """gpu_harness.closed_loop under cfg["policy"], with the coverage of the play counted on the ORACLE's numbers.
    control=(rng, k): snakes 0..k-1 get seeded random actions pre-filled in the buffer, the others are scripted."""
    E, ns, dim, T = cfg["num_envs"], cfg["n_snakes"], cfg["dim"], steps or cfg["steps"]
    body_max, n_fr = np.zeros((T, E), np.int16), np.zeros((T, E), np.int16)
    done_all, ep_len = np.zeros((T, E), np.uint8), np.zeros((T, E), np.int32)

    def observe(t, states, wants, o_done, o_el):
        body_max[t] = [max(len(b) for b in st["snakes"]) for st in states]
        n_fr[t] = [len(st["fruits"]) for st in states]
        done_all[t], ep_len[t] = o_done, o_el

    gh.closed_loop(cfg, env, lambda env, buf, snakes: env.scripted_actions_device(cfg["policy"], snakes=snakes, out=buf.act, safe_out=buf.safe),
                   lambda states: expected(cfg["policy"], states, dim, ns), T, stride=stride, obs_every=obs_every, observe=observe,
                   control=control and (control[0], range(control[1], ns)))
    cov = sp.coverage(cfg, body_max, n_fr, done_all, ep_len)
    sp.check_coverage(dict(cfg, expect=list(expect)), cov)
    return cov


@pytest.mark.parametrize("name", list(LOOP))
def test_closed_loop_with_the_oracle_as_master(name):
    cfg = _cfg(name)   # (A10x3 runs at env_id_base 48: a handle whose first env is not global env 0)
    env = _mk(cfg)
    cov = _closed_loop(cfg, env, LOOP[name])
    assert cov["episodes"] > 0 and all(cov[k] >= v for k, v in REACH[name].items()), cov
    env.close()


# ------------------------------------------------------------------------------------------ 2. mixed control
@pytest.mark.parametrize("name,steps,stride", [("S19x3", 500, 5), ("N10x4", 400, 7), ("A10x3", 400, 3)])
def test_mixed_control_leaves_the_other_columns_untouched(name, steps, stride):
    cfg = _cfg(name)
    env = _mk(cfg)
    _closed_loop(cfg, env, [], control=(np.random.default_rng(11), 1), stride=stride, steps=steps)
    env.close()


# ------------------------------------------------------------------------------------------ 3. hand-built states
def _install_and_check(cfg, states, policies):
    env = gh.install(cfg, states)
    for pol in policies:
        _check_call(env, pol, states, what=(cfg["rules"], cfg["dim"]))
    return env


@pytest.mark.parametrize("dim", [2, 6, 19, 20, 62])
@pytest.mark.parametrize("ns", [1, 2, 3])
def test_hand_built_snake_env_states(dim, ns):
    rng = np.random.default_rng([dim, ns])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 60)
    if ns == 2 and dim >= 6:
        states += bs.tie_states(dim)
    pols = ["safe_greedy"] + (["hamiltonian"] if dim % 2 == 0 else [])
    _install_and_check(dict(rules=0, dim=dim, n_snakes=ns, n_fruits=ns), states, pols).close()


@pytest.mark.parametrize("dim", [6, 10, 19])
def test_hand_built_adversarial_states_with_long_fruit_lists(dim):
    """Fruit lists of more than 64 entries whose nearest fruit has an index >= 64, entries at -1 / dim included."""
    rng = np.random.default_rng(dim)
    fcap = (3 + 3 * (dim * dim + 2) + 63) // 64 * 64      # the handle's fruit-list capacity (msnake_capi.hip)
    h = (dim // 2, dim // 2)
    border = [(-1, 0), (dim, dim - 1), (0, -1), (dim - 1, dim), (-1, -1), (dim, dim), (0, 0), (dim - 1, 0)]
    states, nearest = [], []   # nearest: (index of the first of four states, one per move; list length; index of the near fruit)
    for n_list in (0, 1, 63, 64, 65, 70, 127, fcap - 1, fcap):
        for near_at in sorted({n_list - 1, 64, 66, 100, 0}):
            if not 0 <= near_at < n_list:
                continue
            nearest.append((len(states), n_list, near_at))
            for a in (1, 2, 3, 4):
                fl = [border[i % len(border)] for i in range(n_list)]
                fl[near_at] = (h[0] + sp.DIRS[a][0], h[1] + sp.DIRS[a][1])      # on the target of move a
                states.append(_st([[h], [(0, dim - 1)], []], fl))
        states.append(_st([[h], [], []], [tuple(int(v) for v in rng.integers(-1, dim + 1, 2)) for _ in range(n_list)]))
    assert sum(1 for _, n, at in nearest if n > 64 and at >= 64) >= 6
    states += bs.random_states(dim, 3, 90, rng, 40, fruit_lo=-1, fruit_hi=dim + 1)
    pols = ["safe_greedy"] + (["hamiltonian"] if dim % 2 == 0 else [])
    env = _install_and_check(dict(rules=2, dim=dim, n_snakes=3, n_fruits=3), states, pols)
    # the nearest-fruit cases once more, stated without the helper: the fruit ON the target of move a wins
    out = env.scripted_actions_device("safe_greedy").cpu().numpy()
    for k, n_list, near_at in nearest:
        assert out[k:k + 4, 0].tolist() == [1, 2, 3, 4], (n_list, near_at)
    env.close()


@pytest.mark.parametrize("nf", [0, 1, 32])
@pytest.mark.parametrize("ns", [1, 4])
def test_hand_built_new_world_states(nf, ns):
    """n_fruits 0 and 32, four snakes, stacked duplicate cells, bodies kept after a self-hit (alive False)."""
    dim = 10
    rng = np.random.default_rng([nf, ns])
    states = bs.border_states(dim, ns, nf, rng) + bs.random_states(dim, ns, nf, rng, 60, dup=True)
    for st in states[::3]:   # every third state: some snakes dead with their bodies kept
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        st["in_dead"] = [not a and bool(rng.integers(0, 2)) for a in st["alive"]]
    h = (4, 4)
    dead = _st([[h, (5, 4), (5, 4), (5, 5)]] + [[(4, 5), (4, 5)]] * (ns - 1), [(9, 9)] * nf, alive=[False] * ns)
    states.append(dead)   # a kept, stacked body blocks like any other
    _install_and_check(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states, ["safe_greedy", "hamiltonian"]).close()


@pytest.mark.parametrize("rules,dim,ns", [(0, 10, 2), (0, 19, 3), (1, 12, 2), (2, 10, 3)])
def test_blocking_piece_in_the_overflow_ring(rules, dim, ns):
    """Bodies of more than 64 cells laid along the Hamiltonian cycle with the head in the return lane (column 0): the
    cell beside the head, in column 1, was visited long ago, so the piece that blocks that move has an index >= 64 --
    and the same bodies cut to 64 pieces, where that move is open.  Installed in the library and the oracle alike, then
    both are stepped (the overflow ring's head moves) and compared after the install and after every step."""
    from oracle.snake_oracle import state_to_flat
    states = bs.return_lane_states(dim, ns)
    cfg = dict(rules=rules, dim=dim, n_snakes=ns, n_fruits=ns, num_envs=len(states), seed=2, env_id_base=0, max_steps=2000,
               policy="safe_greedy")
    env = _mk(cfg)
    ora = sp.make_oracle(cfg)
    env.reset(), ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, ns))
        ora.set_state(e, st)
    read = sp._StateReader(ora)
    blocked_by_old_piece = 0
    for t in range(2 * dim):
        cur = [read(e) for e in range(len(states))]
        for st in cur:                      # count the cases this test is there for, from the oracle's state
            b = st["snakes"][0]
            near = {(b[0][0] + d0, b[0][1] + d1) for d0, d1 in sp.DIRS.values()} if b else set()
            blocked_by_old_piece += bool(near & ({tuple(c) for c in b[64:]} - {tuple(c) for c in b[:64]}))
        for pol in ("safe_greedy",) + (("hamiltonian",) if dim % 2 == 0 else ()):
            _check_call(env, pol, cur, what=("overflow", t))
        greedy = expected("safe_greedy", cur, dim, ns)[0]
        import torch
        _, rew, done, _ = env.step_device(torch.from_numpy(greedy).to(env.device))
        _, o_rew, o_done, *_ = ora.step(greedy, want_obs=False)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
    assert blocked_by_old_piece >= 6, blocked_by_old_piece
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ 4. scale and layout
@pytest.mark.parametrize("n", [16384, 20000])
def test_large_batches_compare_every_env(n):
    cfg = dict(_cfg("S19x3"), num_envs=n, seed=21, env_id_base=7)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    rng = np.random.default_rng(n)
    # 32 steps of play that the library has no part in: the helper's safe_greedy on the ORACLE's state of the first
    # 1 024 envs steers them, and every other env e follows env e % 1024 (for it an arbitrary, seeded sequence of
    # turns); every 4th step is random
    import torch
    read = sp._StateReader(ora)
    for t in range(32):
        if t % 4 == 3:
            act = rng.integers(0, 5, (n, 3)).astype(np.int32)
        else:
            lead = expected("safe_greedy", [read(e) for e in range(1024)], 19, 3)[0]
            act = np.ascontiguousarray(np.tile(lead, (n // 1024 + 1, 1))[:n])
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, threads=16, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), o_done) and np.array_equal(rew.cpu().numpy(), o_rew), t
    states = _states(ora)
    assert max(len(b) for st in states for b in st["snakes"]) >= 5     # the snakes have grown
    _check_call(env, "safe_greedy", states, what=n)
    env.close()


@pytest.mark.parametrize("record_policy", ["full", "short"])
@pytest.mark.parametrize("epb", [1, 4, 8])
@pytest.mark.parametrize("name", ["S19x3", "A10x3"])
def test_record_policies_and_envs_per_block(name, record_policy, epb):
    cfg = dict(_cfg(name), num_envs=37)   # ragged: not a multiple of any envs_per_block
    env = _mk(cfg, record_policy=record_policy, envs_per_block=epb)
    _closed_loop(cfg, env, [], steps=120, obs_every=40)
    env.close()


@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("name", ["S19x3", "N10x2", "A10x3"])
def test_after_tape_rollouts(name, persistent):
    import torch
    cfg = dict(_cfg(name), num_envs=48)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    rng = np.random.default_rng(3)
    for chunk in range(3):
        tape = rng.integers(0, 5, (25, 48, cfg["n_snakes"])).astype(np.int32)
        tape[:, :, :] = np.where(rng.random(tape.shape) < 0.5, tape, 2 - chunk % 2)   # long runs in one direction too
        env.rollout_device(torch.from_numpy(tape).to(env.device), persistent=persistent, keep_obs=False)
        for t in range(25):
            ora.step(tape[t], want_obs=False)
        for pol in ("safe_greedy",) + (("hamiltonian",) if cfg["dim"] % 2 == 0 else ()):
            _check_call(env, pol, _states(ora), what=(name, persistent, chunk))
    env.close()


@pytest.mark.parametrize("name", ["S19x3", "N10x4"])
def test_after_a_masked_reset(name):
    import torch
    cfg = dict(_cfg(name), num_envs=64)
    env, ora = _mk(cfg, auto_reset=False), sp.make_oracle(cfg, auto_reset=False)
    env.reset(), ora.reset()
    rng = np.random.default_rng(5)
    resets = 0
    for t in range(60):
        act = rng.integers(0, 5, (64, cfg["n_snakes"])).astype(np.int32)
        _, _, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, _, o_done, *_ = ora.step(act, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), o_done)
        _check_call(env, "safe_greedy", _states(ora), what=("finished envs in place", t))
        if o_done.any() and t % 2 == 0:
            env.reset_device(mask=done)
            ora.reset_envs(o_done, obs=None, final_obs=None, truncated=None)
            resets += int(o_done.sum())
            _check_call(env, "safe_greedy", _states(ora), what=("after reset_envs", t))
    assert resets >= 10
    env.close()


def test_on_a_terminal_obs_env():
    cfg = dict(_cfg("S19x3"), num_envs=32)
    env = _mk(cfg, terminal_obs=True)
    _closed_loop(cfg, env, [], steps=300)
    env.close()


# ------------------------------------------------------------------------------------------ 5. read-only
def test_the_call_changes_no_state():
    import torch
    cfg = dict(_cfg("A10x3"), num_envs=40)
    env, plain = _mk(cfg), _mk(cfg)
    o1, o2 = env.reset(), plain.reset()
    assert np.array_equal(o1, o2)
    rng = np.random.default_rng(8)
    safe = torch.zeros((40, 3), dtype=torch.uint8, device=env.device)
    for t in range(150):
        act = torch.from_numpy(rng.integers(0, 5, (40, 3)).astype(np.int32)).to(env.device)
        if t % 25 == 0:
            before, st_before = env.get_state_all().tobytes(), env.stats()
        env.scripted_actions_device("safe_greedy", safe_out=safe)      # into the env's own buffer, not into `act`
        env.scripted_actions_device("hamiltonian")
        env.safe_moves_device()
        if t % 25 == 0:
            assert env.get_state_all().tobytes() == before and env.stats() == st_before
        a, b = env.step_device(act), plain.step_device(act)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    assert env.get_state_all().tobytes() == plain.get_state_all().tobytes()
    assert env.stats() == plain.stats() and env.stats()["env_steps"] == 150 * 40   # the call adds nothing to env_steps
    env.close(), plain.close()


# ------------------------------------------------------------------------------------------ 6. outputs
@pytest.mark.parametrize("n", [1, 3, 13, 101, 257])
def test_outputs_guards_and_policy_none(n):
    import torch
    cfg = dict(_cfg("N10x4"), num_envs=n)
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    _play_random(env, ora, 6, np.random.default_rng(n), threads=1)
    states = _states(ora)
    want_a, want_m = expected("safe_greedy", states, 10, 4)
    for stride in (4, 6):
        buf = gh.action_buffers(env, stride)
        # the mask alone (MSNAKE_POLICY_NONE): no action word is written
        out, safe = env.scripted_actions_device(None, out=buf.act, safe_out=buf.safe)
        assert (out.cpu().numpy() == FILL).all() and np.array_equal(safe.cpu().numpy(), want_m) and buf.guards_intact()
        assert np.array_equal(env.safe_moves_device().cpu().numpy(), want_m)
        # an empty selection with a mask: the same
        buf.refill(["safe"])
        out, safe = env.scripted_actions_device("safe_greedy", snakes=[], out=buf.act, safe_out=buf.safe)
        assert (out.cpu().numpy() == FILL).all() and np.array_equal(safe.cpu().numpy(), want_m)
        # snakes 1 and 3 only, no mask
        out = env.scripted_actions_device("safe_greedy", snakes=[3, 1], out=buf.act)
        got = out.cpu().numpy()
        assert np.array_equal(got[:, [1, 3]], want_a[:, [1, 3]]) and (got[:, [0, 2] + list(range(4, stride))] == FILL).all()
        assert buf.guards_intact()
    # the env's own cached buffer: zero-filled, the same tensor on every call
    a = env.scripted_actions_device("hamiltonian", snakes=[2])
    assert a.data_ptr() == env.scripted_actions_device("hamiltonian", snakes=[2]).data_ptr()
    got = a.cpu().numpy()
    assert np.array_equal(got[:, 2], expected("hamiltonian", states, 10, 4)[0][:, 2]) and not got[:, [0, 1, 3]].any()
    with pytest.raises(ValueError):
        env.scripted_actions_device("safe_greedy", out=torch.zeros((n, 3), dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError):
        env.scripted_actions_device("safe_greedy", out=torch.zeros((n, 4), dtype=torch.int64, device=env.device))
    with pytest.raises(ValueError):
        env.scripted_actions_device("safe_greedy", safe_out=torch.zeros((n, 5), dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.scripted_actions_device("safe_greedy", snakes=[4])
    with pytest.raises(ValueError):
        env.scripted_actions_device("greedy")
    env.close()


# ------------------------------------------------------------------------------------------ 7. HIP graph
def test_graph_of_scripted_actions_then_step():
    """[msnake_scripted_actions -> msnake_step] captured as one linear chain and replayed: the env plays against itself
    on the device with no call from the host; final state and last actions against the oracle loop."""
    import torch
    from oracle.snake_oracle import flat_to_state
    cfg = dict(_cfg("S19x3"), num_envs=64)
    K = 150
    env, ora = _mk(cfg), sp.make_oracle(cfg)
    env.reset(), ora.reset()
    blob = env.get_state_all()
    acts = torch.zeros((64, 3), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("safe_greedy", out=acts)
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # the warm-up step moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("safe_greedy", out=acts)
        out = env.step_device(acts)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # (capture itself runs nothing; this keeps the start state explicit)
    rews = []
    for _ in range(K):
        g.replay()
        rews.append(out[1].clone())
    torch.cuda.synchronize()
    want = None
    o_rews = []
    for _ in range(K):
        want = expected("safe_greedy", _states(ora), 19, 3)[0]
        o_rews.append(ora.step(want)[1].copy())
    assert np.array_equal(acts.cpu().numpy(), want)
    assert np.array_equal(torch.stack(rews).cpu().numpy(), np.stack(o_rews))
    assert np.array_equal(out[0].cpu().numpy(), ora.obs)
    for e in range(64):
        got, exp = flat_to_state(env.get_state_words(e)), ora.get_state(e)
        assert got == exp, e
    env.close()


# ------------------------------------------------------------------------------------------ 8. errors
def test_argument_errors_name_the_argument():
    import torch
    import msnake
    env = msnake.MultiSnakeVecEnv(5, dim=19, n_snakes=3, rules="snake_env", seed=0)   # odd dim
    even = msnake.MultiSnakeVecEnv(5, dim=10, n_snakes=2, rules="snake_env", seed=0)
    env.reset(), even.reset()
    L = env._L
    acts = torch.full((5, 3), 9, dtype=torch.int32, device=env.device)
    safe = torch.full((5, 3), 9, dtype=torch.uint8, device=env.device)
    pa, ps = acts.data_ptr(), safe.data_ptr()

    def call(h, policy, mask, a, stride, s):
        rc = L.msnake_scripted_actions(h, policy, mask, a, stride, s, None)
        return rc, L.msnake_last_error().decode()

    for args, word in (((env._h, 3, 1, pa, 3, None), "policy"), ((env._h, -1, 1, pa, 3, None), "policy"),
                       ((env._h, 1, 0b1000, pa, 3, None), "snake_mask"), ((env._h, 0, 0b1000, None, 3, ps), "snake_mask"),
                       ((even._h, 2, 0b100, pa, 3, None), "snake_mask"),
                       ((env._h, 1, 0b111, pa, 2, None), "action_stride"), ((env._h, 1, 1, None, 3, ps), "actions_dev"),
                       ((env._h, 1, 0, pa, 3, None), "nothing to write"), ((env._h, 0, 0b111, pa, 3, None), "nothing to write"),
                       ((env._h, 0, 0, None, 0, None), "nothing to write"),
                       ((env._h, 2, 1, pa, 3, None), "dim"), ((env._h, 2, 0, None, 0, ps), "dim")):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (args[1:], rc, msg)
    assert call(None, 1, 1, pa, 3, None)[0] == -3
    torch.cuda.synchronize()
    assert (acts.cpu().numpy() == 9).all() and (safe.cpu().numpy() == 9).all()   # refused before any device work
    # what is NOT an error: action_stride / actions_dev are not looked at when no action is written
    assert call(env._h, 0, 0, None, 0, ps)[0] == 0 and call(env._h, 1, 0, None, 0, ps)[0] == 0
    assert call(even._h, 2, 0b11, pa, 2, None)[0] == 0
    with pytest.raises(RuntimeError, match="dim"):
        env.scripted_actions_device("hamiltonian")
    assert env.stats()["env_steps"] == 0
    env.close(), even.close()
