"""msnake_reset_envs against the oracle's plain statement of it (orc_reset_envs, pinned to the reference's recordings by
tests/test_oracle_reset_envs.py), on every path a masked launch can take: the short record and 4 envs per workgroup at
scale, the same paths forced small through msnake_config, ragged batches and every buffer alignment, long bodies / long
fruit lists / the 2^32 draw wrap at the moment of the reset, the odd corners of the C surface, a checkpoint between step
and reset, and the tape paths afterwards.

Bit-exact throughout (np.array_equal / torch.equal, no tolerance).  The plain outputs of a terminal_obs=True env are
compared against Oracle(auto_reset=True), its terminal observations and truncation flags against
Oracle(auto_reset=False) + reset_envs: every env, every step.  Only the canonical state at the end is compared on a
seeded sample of envs.  Every run with terminal_obs=True must see at least one episode cut by the cap and one ended by
the rules, and every random mask selects between 5 % and 95 % of the envs."""
import ctypes

import numpy as np
import pytest

from board_states import serpentine_body

pytestmark = pytest.mark.gpu

RULES = ["snake_env", "new_world", "adversarial"]
SENTINEL = 0xA5


def _mk(**kw):
    import msnake
    return msnake.MultiSnakeVecEnv(**kw)


def _oracle(n, **kw):
    from oracle.snake_oracle import Oracle
    return Oracle(n, **kw)


def _state(env, e):
    from oracle.snake_oracle import flat_to_state
    return flat_to_state(env.get_state_words(e))


def _finished(env, e):
    from oracle.snake_oracle import flat_finished
    return flat_finished(env.get_state_words(e))


def _set_both(env, ora, e, st):
    from oracle.snake_oracle import state_to_flat
    env.set_state_words(e, state_to_flat(st, env.n_snakes))
    ora.set_state(e, st)


def _up(frames, k):
    """The fused WarpFrame: integer pixel replication of the oracle frames [n, H, W, C]."""
    return frames if k == 1 else np.repeat(np.repeat(frames, k, axis=1), k, axis=2)


def _random_mask(rs, n):
    """A random selection of between 5 % and 95 % of n envs (None where no such selection exists: n = 1)."""
    lo, hi = int(np.ceil(0.05 * n)), int(np.floor(0.95 * n))
    if lo > hi:
        return None
    k = int(np.clip(round(float(rs.uniform(0.15, 0.85)) * n), lo, hi))
    mask = np.zeros(n, bool)
    mask[rs.choice(n, k, replace=False)] = True
    assert 0.05 * n <= mask.sum() <= 0.95 * n
    return mask


def _sample(n, k, seed):
    return sorted(np.random.default_rng(seed).choice(n, min(n, k), replace=False).tolist())


def _terminal_obs_run(n, steps, act_seed, scale=1, threads=8, sample=48, **kw):
    """A terminal_obs=True env through `steps` steps of uniform random actions: obs / rew / done / info against the
    auto-reset oracle, final_obs[done] and truncated (all envs) against step + reset_envs on the oracle without auto
    reset, every step; stats() and a seeded sample of canonical states at the end.  kw: what both sides are built
    with; launch tuning goes to the env alone."""
    tuning = {k: kw.pop(k) for k in ("envs_per_block", "record_policy", "obs_store_policy") if k in kw}
    ns = kw["n_snakes"]
    env = _mk(num_envs=n, terminal_obs=True, obs_scale=scale, **kw, **tuning)
    auto = _oracle(n, auto_reset=True, **kw)
    raw = _oracle(n, auto_reset=False, **kw)
    first = auto.reset().copy()
    assert np.array_equal(env.reset(), _up(first, scale)) and np.array_equal(raw.reset(), first)
    rs = np.random.default_rng(act_seed)
    n_cut = n_ended = 0
    ep = np.zeros(3, np.int64)
    for t in range(steps):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        obs, rew, done, infos = env.step(act)
        a_obs, a_rew, a_done, a_ns, a_er, a_el = auto.step(act, threads=threads)
        raw.step(act, threads=threads)
        sel = a_done != 0
        assert np.array_equal(raw.done, a_done), t
        raw.reset_envs(raw.done)  # (raw.obs: terminal rows become reset rows; raw.final_obs, raw.truncated)
        assert np.array_equal(raw.obs, a_obs), f"step + reset_envs(done) is not the auto reset on the oracle at step {t}"
        assert np.array_equal(rew, a_rew) and np.array_equal(done, sel), f"rew/done differ at step {t}"
        assert np.array_equal(infos._ns, a_ns) and np.array_equal(infos._r, a_er) and np.array_equal(infos._l, a_el), t
        assert np.array_equal(obs, _up(a_obs, scale)), f"obs differs at step {t}"
        final, trunc = env.final_obs.cpu().numpy(), env.truncated.cpu().numpy()
        assert np.array_equal(trunc, raw.truncated), f"truncation flags differ at step {t}"
        assert np.array_equal(final[sel], _up(raw.final_obs[sel], scale)), f"terminal observations differ at step {t}"
        n_cut += int(raw.truncated.sum())
        n_ended += int(sel.sum()) - int(raw.truncated.sum())
        ep += (int(sel.sum()), int(a_el.sum()), int(a_er.sum()))
    assert n_cut > 0 and n_ended > 0, (n_cut, n_ended)
    st = env.stats()
    assert st == {"episodes": ep[0], "ep_len_sum": ep[1], "ep_return_sum": ep[2], "env_steps": steps * n, "errors": 0}
    for e in _sample(n, sample, act_seed):
        assert _state(env, e) == raw.get_state(e) == auto.get_state(e), e
        assert not _finished(env, e) and not raw.finished(e), e
    env.close()
    return n_cut, n_ended


# ---------------------------------------------------------------------------------- scale and the auto launch shape
@pytest.mark.parametrize("rules,n,ns,base", [("snake_env", 16384, 3, 0), ("adversarial", 20000, 3, 7 * 4096),
                                             ("new_world", 20000, 2, 0)])
def test_terminal_obs_at_scale(rules, n, ns, base):
    """Above 8 192 envs the library takes 4 envs per workgroup and, for [S]/[A], the short record (a reset there finds no
    parked Philox draws and evaluates Philox itself); the batch spans hundreds of 64-workgroup groups of the XCD-aware
    workgroup mapping, which the masked kernels index their mask and flags through."""
    _terminal_obs_run(n, 40, 5, dim=19, n_snakes=ns, rules=rules, seed=1234, max_steps=12, env_id_base=base)


# ---------------------------------------------------------------------------------- the same paths forced small
def _forced_small_cases():
    """record_policy x envs_per_block x obs_store_policy in full for every rule set (16 x 3), the three observation scales
    dealt round-robin over them: every value of every knob meets every rule set, and every scale every value."""
    out = []
    for rules in RULES:
        i = 0
        for rec in ("full", "short"):
            for epb in (1, 2, 4, 8):
                for store in ("plain", "stream"):
                    out.append((rules, rec, epb, store, (1, 4, 7)[i % 3]))
                    i += 1
    return out


def test_forced_small_cases_cover_every_knob():
    cases = _forced_small_cases()
    for rules in RULES:
        mine = [c for c in cases if c[0] == rules]
        for pos, values in ((1, ("full", "short")), (2, (1, 2, 4, 8)), (3, ("plain", "stream")), (4, (1, 4, 7))):
            assert {c[pos] for c in mine} == set(values)
    for scale in (1, 4, 7):
        mine = [c for c in cases if c[4] == scale]
        assert {c[1] for c in mine} == {"full", "short"} and {c[2] for c in mine} == {1, 2, 4, 8}
        assert {c[3] for c in mine} == {"plain", "stream"}


@pytest.mark.parametrize("rules,rec,epb,store,scale", _forced_small_cases())
def test_terminal_obs_on_forced_launch_shapes(rules, rec, epb, store, scale):
    """150 envs: up to 150 workgroups (three 64-workgroup groups at one env per workgroup) and a ragged last workgroup
    for every envs_per_block but 1 and 2.  Boards that up-scale to 84 x 84: 19 x 19 at x4, 10 x 10 at x7."""
    dim = 10 if scale == 7 else 19
    ns = 2 if rules == "new_world" else 3
    _terminal_obs_run(150, 30, 5, scale=scale, threads=2, sample=24, dim=dim, n_snakes=ns, rules=rules, seed=77,
                      max_steps=8, env_id_base=3, record_policy=rec, envs_per_block=epb, obs_store_policy=store)


# ---------------------------------------------------------------------------------- ragged sizes and the edges of a launch
def _edge_masks(n, rs):
    last, first, waves = np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool)
    last[n - 1] = True
    first[0] = True
    waves[::8] = True  # the first wave of every workgroup (8 envs per workgroup up to 8 192 envs)
    but_one = np.ones(n, bool)
    but_one[int(rs.integers(0, n))] = False
    masks = [("last", last), ("first", first), ("first_waves", waves), ("all_but_one", but_one)]
    rnd = _random_mask(rs, n)
    if rnd is not None:  # (a single env has no selection between 5 % and 95 %)
        masks.append(("random", rnd))
    return masks


@pytest.mark.parametrize("scale", [1, 4, 7])
@pytest.mark.parametrize("n", [1, 7, 9, 63, 65, 130, 513, 520, 1031])
def test_ragged_batches_masks_and_buffer_alignments(n, scale):
    """Batches that end inside a workgroup and inside / past the first 64-workgroup group (513, 520, 1031 envs = 65, 65,
    129 workgroups); masks at the edges of the launch; out / final_out / truncated_out inside larger sentinel-filled
    buffers at all 16 byte offsets (native size) or every 4-byte one (x4 / x7).  The whole buffers are compared: guard
    bytes and every row of an unselected env must still hold the sentinel."""
    import torch
    rules = RULES[([1, 7, 9, 63, 65, 130, 513, 520, 1031].index(n) + scale) % 3]
    dim = 10 if scale == 7 else 19
    ns = 2 if rules == "new_world" else 3
    kw = dict(dim=dim, n_snakes=ns, rules=rules, seed=19, max_steps=6, env_id_base=11)
    env = _mk(num_envs=n, auto_reset=False, obs_scale=scale, **kw)
    ora = _oracle(n, auto_reset=False, **kw)
    assert np.array_equal(env.reset(), _up(ora.reset(), scale))
    rs = np.random.default_rng(n * 10 + scale)
    shape = (n,) + env.obs_shape
    nbytes = int(np.prod(shape))
    offsets = list(range(16)) if scale == 1 else [0, 4, 8, 12, 8, 0, 12, 4]
    masks, kinds = [], set()
    while len(masks) < len(offsets):
        masks += _edge_masks(n, rs)
    n_sel_finished = 0
    for it, lead in enumerate(offsets):
        for _ in range(int(rs.integers(1, 4))):  # some episodes end and stay finished: auto reset is off
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            obs, rew, done, _ = env.step(act)
            o_obs, o_rew, o_done = ora.step(act)[:3]
            assert np.array_equal(obs, _up(o_obs, scale)) and np.array_equal(rew, o_rew), (it, lead)
            assert np.array_equal(done, o_done.astype(bool)), (it, lead)
        kind, mask = masks[it]
        kinds.add(kind)
        lead_f = (lead * 5 + 3) % 16 if scale == 1 else (lead + 8) % 16
        lead_t = (lead * 3 + 1) % 16
        bufs = [torch.full((sz + 48,), SENTINEL, dtype=torch.uint8, device=env.device) for sz in (nbytes, nbytes, n)]
        out = bufs[0][lead:lead + nbytes].view(shape)
        final_out = bufs[1][lead_f:lead_f + nbytes].view(shape)
        trunc_out = bufs[2][lead_t:lead_t + n]
        n_sel_finished += sum(ora.finished(e) for e in np.nonzero(mask)[0])
        want = [np.full(shape[:1] + ora.obs_shape, SENTINEL, np.uint8), np.full(shape[:1] + ora.obs_shape, SENTINEL, np.uint8),
                np.full(n, SENTINEL, np.uint8)]
        ora.reset_envs(mask, obs=want[0], final_obs=want[1], truncated=want[2])
        env.reset_device(torch.from_numpy(mask).to(env.device), out=out, final_out=final_out, truncated_out=trunc_out)
        for buf, ld, w in ((bufs[0], lead, _up(want[0], scale)), (bufs[1], lead_f, _up(want[1], scale)), (bufs[2], lead_t, want[2])):
            whole = np.full(buf.numel(), SENTINEL, np.uint8)
            whole[ld:ld + w.size] = w.reshape(-1)
            assert np.array_equal(buf.cpu().numpy(), whole), (it, kind, lead, ld)
        assert np.array_equal(env.render(), _up(ora.render(), scale)), (it, kind)
    assert kinds >= {"last", "first", "first_waves", "all_but_one"} and (n == 1 or "random" in kinds)
    assert n_sel_finished > 0
    for e in _sample(n, 32, n):
        assert _state(env, e) == ora.get_state(e) and _finished(env, e) == ora.finished(e), e
    assert env.stats()["errors"] == 0
    env.close()


# ---------------------------------------------------------------------------------- state at the moment of the reset
@pytest.mark.parametrize("rules,rec", [("snake_env", "full"), ("snake_env", "short"), ("new_world", "full"),
                                       ("adversarial", "full"), ("adversarial", "short")])
def test_masked_reset_of_long_bodies_long_fruit_lists_and_wrapping_counters(rules, rec):
    """Hand-built states: bodies of 50..250 cells (the overflow ring behind the 64-cell register ring), [A] fruit lists of
    65..200 entries (past chunk 0) with spare fruits, and draw counters at 2^32 - k for every k in 0 .. 4 * n_snakes, so
    that the reset's draws straddle the 32-bit wrap at every phase.  Half of the envs are reset by mask: their terminal
    observations must be exact, the other half must be unharmed, and 30 more steps (each followed by a masked reset of
    the done envs) must match the oracle."""
    import torch
    rs = np.random.default_rng(404)
    dim, n, ns, M = 19, 104, 2, 40
    nf = 3 if rules == "new_world" else 2
    kw = dict(dim=dim, n_snakes=ns, n_fruits=nf, rules=rules, seed=13, max_steps=M, env_id_base=1 << 33)
    env = _mk(num_envs=n, auto_reset=False, record_policy=rec, **kw)
    ora = _oracle(n, auto_reset=False, **kw)
    env.reset(); ora.reset()
    ks = list(range(4 * ns + 1))
    for e in range(n):
        la, lb = int(rs.integers(50, 250)), int(rs.integers(1, 60))
        a, b = serpentine_body(dim, la, 0), serpentine_body(dim, lb, 15)
        va = [1, 0] if a[0][1] % 2 == 0 else [-1, 0]
        # [N]: the alive bit (the body stays; the episode ends while it is ON); [S]/[A]: a dead snake has no body
        main_dead = e % 2 == 1 if rules == "new_world" else e % 5 == 4
        if rules == "adversarial":
            fruits = [[int(rs.integers(-1, dim + 1)), int(rs.integers(-1, dim + 1))] for _ in range(int(rs.integers(65, 200)))]
        else:
            fruits = [[int(rs.integers(0, dim)), int(rs.integers(0, dim))] for _ in range(nf)]
        st = {"snakes": [[] if main_dead and rules != "new_world" else a, b], "fruits": fruits, "vels": [va, [0, 0]],
              "grow_to": [la + int(rs.integers(0, 3)), lb + 2], "t": int(rs.choice([3, M - 1, M, M + 2])),
              "ctr": (1 << 32) - ks[e % len(ks)], "alive": [not (main_dead and rules == "new_world"), True],
              "in_dead": [main_dead and rules == "new_world", False],
              "spare_fruits": int(rs.integers(0, 4)), "ep_len": 5, "ep_return": 2.0, "finished": bool(e % 3)}
        _set_both(env, ora, e, st)
    assert np.array_equal(env.render(), ora.render())
    mask = np.zeros(n, bool)
    mask[rs.choice(n, n // 2, replace=False)] = True
    assert {ks[e % len(ks)] for e in np.nonzero(mask)[0]} == set(ks)  # every phase of the wrap is among the reset ones
    before = [env.get_state_words(e) for e in range(n)]
    shape = (n,) + env.obs_shape
    out, final_out = (torch.full(shape, SENTINEL, dtype=torch.uint8, device=env.device) for _ in range(2))
    trunc_out = torch.full((n,), SENTINEL, dtype=torch.uint8, device=env.device)
    want = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8), np.full(n, SENTINEL, np.uint8)]
    ora.reset_envs(mask, obs=want[0], final_obs=want[1], truncated=want[2])
    env.reset_device(mask, out=out, final_out=final_out, truncated_out=trunc_out)
    assert np.array_equal(final_out.cpu().numpy(), want[1]), "terminal observations of the long bodies"
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(trunc_out.cpu().numpy(), want[2])
    assert 0 < want[2].sum() < mask.sum()
    min_draws = 2 * ns + nf if rules == "new_world" else 4 * ns  # what one reset draws ([N]: at least)
    assert all(ora.get_state(e)["ctr"] >= (1 << 32) for e in np.nonzero(mask)[0] if ks[e % len(ks)] <= min_draws)
    for e in range(n):
        if not mask[e]:
            assert np.array_equal(env.get_state_words(e), before[e]), e  # the unselected long bodies are unharmed
        assert _state(env, e) == ora.get_state(e) and _finished(env, e) == ora.finished(e), e
    assert np.array_equal(env.render(), ora.render())
    for t in range(30):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        act[:, 0] = np.where(rs.random(n) < 0.8, 0, act[:, 0])  # mostly keep going so the long snakes survive a while
        obs, rew, done, infos = env.step(act)
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(act)
        assert np.array_equal(obs, o_obs) and np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), t
        assert np.array_equal(infos._ns, o_ns) and np.array_equal(infos._l, o_el) and np.array_equal(infos._r, o_er), t
        sel = done & (rs.random(n) < 0.7)  # (some finished envs stay finished for a while)
        w_obs, w_final, w_trunc = ora.reset_envs(sel)
        w_final = w_final.copy()
        got = env.reset_device(sel, final_out=final_out, truncated_out=trunc_out).cpu().numpy()
        assert np.array_equal(got[sel], w_obs[sel]) and np.array_equal(final_out.cpu().numpy()[sel], w_final[sel]), t
        assert np.array_equal(trunc_out.cpu().numpy(), w_trunc), t
    for e in range(n):
        assert _state(env, e) == ora.get_state(e) and _finished(env, e) == ora.finished(e), e
    assert env.stats()["errors"] == 0
    env.close()


# ---------------------------------------------------------------------------------- the surface
def _advance(env, ora, rs, k):
    n, ns = env.num_envs, env.n_snakes
    for _ in range(k):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        obs, rew, done, _ = env.step(act)
        o_obs, o_rew, o_done = ora.step(act)[:3]
        assert np.array_equal(obs, o_obs) and np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool))


@pytest.mark.parametrize("rules", RULES)
def test_surface_mask_bytes_null_pointers_and_the_done_buffer(rules):
    import torch
    n, ns = 200, 2
    kw = dict(dim=10, n_snakes=ns, rules=rules, seed=61, max_steps=7)
    env = _mk(num_envs=n, auto_reset=False, **kw)
    ora = _oracle(n, auto_reset=False, **kw)
    assert np.array_equal(env.reset(), ora.reset())
    rs = np.random.default_rng(8)
    shape = (n,) + env.obs_shape
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)  # noqa: E731
    n_cut = 0

    # any non-zero byte selects: 2, 0x80, 0xFF (and 1)
    _advance(env, ora, rs, 8)
    sel = _random_mask(rs, n)
    mask = np.where(sel, np.array([2, 0x80, 0xFF, 1], np.uint8)[np.arange(n) % 4], 0).astype(np.uint8)
    out, final_out = (torch.full(shape, SENTINEL, dtype=torch.uint8, device=env.device) for _ in range(2))
    trunc_out = torch.full((n,), SENTINEL, dtype=torch.uint8, device=env.device)
    want = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8), np.full(n, SENTINEL, np.uint8)]
    ora.reset_envs(mask, obs=want[0], final_obs=want[1], truncated=want[2])
    env.reset_device(torch.from_numpy(mask).to(env.device), out=out, final_out=final_out, truncated_out=trunc_out)
    for got, w in zip((out, final_out, trunc_out), want):
        assert np.array_equal(got.cpu().numpy(), w)
    n_cut += int(want[2].sum())

    # obs_dev = NULL (and final_obs_dev = NULL): the state alone is reset; a following render shows it
    _advance(env, ora, rs, 8)
    sel = _random_mask(rs, n)
    m_dev = torch.from_numpy(sel.astype(np.uint8)).to(env.device)
    trunc_out.fill_(SENTINEL)
    assert env._L.msnake_reset_envs(env._h, m_dev.data_ptr(), None, None, trunc_out.data_ptr(), stream()) == 0
    w_trunc = ora.reset_envs(sel, obs=None, final_obs=None)[2]
    assert np.array_equal(trunc_out.cpu().numpy(), w_trunc)
    assert np.array_equal(env.render(), ora.render())
    n_cut += int(w_trunc.sum())

    # truncated_dev = NULL, with and without the observation pointers
    _advance(env, ora, rs, 8)
    sel = _random_mask(rs, n)
    m_dev = torch.from_numpy(sel.astype(np.uint8)).to(env.device)
    out.fill_(SENTINEL); final_out.fill_(SENTINEL)
    assert env._L.msnake_reset_envs(env._h, m_dev.data_ptr(), out.data_ptr(), final_out.data_ptr(), None, stream()) == 0
    want = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8)]
    ora.reset_envs(sel, obs=want[0], final_obs=want[1], truncated=None)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(final_out.cpu().numpy(), want[1])
    _advance(env, ora, rs, 3)
    sel = _random_mask(rs, n)
    m_dev = torch.from_numpy(sel.astype(np.uint8)).to(env.device)
    assert env._L.msnake_reset_envs(env._h, m_dev.data_ptr(), None, None, None, stream()) == 0
    ora.reset_envs(sel, obs=None, final_obs=None, truncated=None)
    assert np.array_equal(env.render(), ora.render())

    # the mask is the handle's own done buffer, as the step left it
    for t in range(12):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        obs, rew, done, info = env.step_device(torch.from_numpy(act).to(env.device))
        assert done.data_ptr() == env._done.data_ptr()
        o_done = ora.step(act)[2].copy()
        assert np.array_equal(done.cpu().numpy(), o_done)
        trunc_out.fill_(SENTINEL)
        got = env.reset_device(done, final_out=final_out, truncated_out=trunc_out)
        assert got.data_ptr() == obs.data_ptr()
        assert np.array_equal(env._done.cpu().numpy(), o_done)  # the reset does not write it
        sel = o_done != 0
        terminal = ora.obs[sel].copy()
        w_obs, _, w_trunc = ora.reset_envs(o_done)
        assert np.array_equal(got.cpu().numpy(), w_obs) and np.array_equal(trunc_out.cpu().numpy(), w_trunc), t
        assert np.array_equal(final_out.cpu().numpy()[sel], terminal), t
        n_cut += int(w_trunc.sum())
    assert n_cut > 0
    for e in _sample(n, 40, 1):
        assert _state(env, e) == ora.get_state(e) and _finished(env, e) == ora.finished(e), e
    assert env.stats()["errors"] == 0
    env.close()


@pytest.mark.parametrize("rules", RULES)
def test_two_half_handles_with_split_masks_equal_one(rules):
    import torch
    n, ns, base = 272, 2, 5 * 4096
    kw = dict(dim=10, n_snakes=ns, rules=rules, seed=33, max_steps=7, auto_reset=False)
    whole = _mk(num_envs=n, env_id_base=base, **kw)
    halves = [_mk(num_envs=n // 2, env_id_base=base + i * (n // 2), **kw) for i in range(2)]
    ora = _oracle(n, env_id_base=base, **kw)
    want = ora.reset()
    assert np.array_equal(whole.reset(), want)
    assert np.array_equal(np.concatenate([h.reset() for h in halves]), want)
    rs = np.random.default_rng(6)
    n_cut = 0
    for it in range(6):
        for _ in range(5):
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            o = ora.step(act)[0]
            assert np.array_equal(whole.step(act)[0], o)
            assert np.array_equal(np.concatenate([h.step(a)[0] for h, a in zip(halves, np.split(act, 2))]), o)
        mask = _random_mask(rs, n)
        shape = (n,) + whole.obs_shape
        want = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8), np.full(n, SENTINEL, np.uint8)]
        ora.reset_envs(mask, obs=want[0], final_obs=want[1], truncated=want[2])
        got = []
        for env, m in [(whole, mask)] + list(zip(halves, np.split(mask, 2))):
            sh = (env.num_envs,) + env.obs_shape
            bufs = [torch.full(sh, SENTINEL, dtype=torch.uint8, device=env.device) for _ in range(2)]
            tr = torch.full((env.num_envs,), SENTINEL, dtype=torch.uint8, device=env.device)
            env.reset_device(m, out=bufs[0], final_out=bufs[1], truncated_out=tr)
            got.append([x.cpu().numpy() for x in bufs + [tr]])
        for k in range(3):
            assert np.array_equal(got[0][k], want[k]), (it, k)
            assert np.array_equal(np.concatenate([got[1][k], got[2][k]]), want[k]), (it, k)
        n_cut += int(want[2].sum())
    assert n_cut > 0
    sw, sh = whole.stats(), [h.stats() for h in halves]
    assert all(sw[k] == sh[0][k] + sh[1][k] for k in sw)
    for e in _sample(n, 40, 2):
        h, le = halves[e // (n // 2)], e % (n // 2)
        assert np.array_equal(whole.get_state_words(e), h.get_state_words(le)) and _state(whole, e) == ora.get_state(e), e
    whole.close()
    for h in halves:
        h.close()


# ---------------------------------------------------------------------------------- a checkpoint in the gap
@pytest.mark.parametrize("rules", RULES)
def test_checkpoint_between_step_and_masked_reset(rules):
    """get_state_all() taken after msnake_step and before msnake_reset_envs on a handle without auto reset, restored into
    a fresh handle: the masked reset there gives the same rows, flags and state, and from then on the same episode
    totals.  The flags need the finished bit: it must survive the checkpoint."""
    import torch
    n, ns = 300, 2
    kw = dict(num_envs=n, dim=10, n_snakes=ns, rules=rules, seed=29, max_steps=6, auto_reset=False, env_id_base=9)
    a = _mk(**kw)
    ora = _oracle(n, **{k: v for k, v in kw.items() if k != "num_envs"})
    assert np.array_equal(a.reset(), ora.reset())
    rs = np.random.default_rng(14)
    n_cut = n_ended = 0
    for it in range(4):
        for j in range(2 * int(rs.integers(1, 4)) + 1):  # (an odd count: the last step is not followed by a reset)
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            done = a.step(act)[2]
            o_done = ora.step(act)[2].copy()
            assert np.array_equal(done, o_done.astype(bool))
            if j % 2:  # half of the done envs are reset, the others stay finished
                part = done & (rs.random(n) < 0.5)
                a.reset_device(part); ora.reset_envs(part)
        mask = done | (rs.random(n) < 0.2)  # the step's done envs and some that are in mid-episode or finished earlier
        blob = a.get_state_all()  # ---- the checkpoint, in the gap
        b = _mk(**kw)
        b.reset()
        b.set_state_all(blob)
        fin = [_finished(a, e) for e in range(n)]
        assert fin == [_finished(b, e) for e in range(n)] == [ora.finished(e) for e in range(n)] and any(fin)
        base_a, base_b = a.stats(), b.stats()
        shape = (n,) + a.obs_shape
        want = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8), np.full(n, SENTINEL, np.uint8)]
        ora.reset_envs(mask, obs=want[0], final_obs=want[1], truncated=want[2])
        for env in (a, b):
            bufs = [torch.full(shape, SENTINEL, dtype=torch.uint8, device=env.device) for _ in range(2)]
            tr = torch.full((n,), SENTINEL, dtype=torch.uint8, device=env.device)
            env.reset_device(mask, out=bufs[0], final_out=bufs[1], truncated_out=tr)
            for got, w in zip(bufs + [tr], want):
                assert np.array_equal(got.cpu().numpy(), w), it
        n_cut += int(want[2].sum())
        n_ended += int((mask & np.array(fin)).sum()) - int(want[2].sum())
        assert np.array_equal(a.get_state_all(), b.get_state_all())
        assert a.stats() == base_a and b.stats() == base_b  # a masked reset counts nothing
        for t in range(8):  # both go on alike, and count the same episodes from here
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            ra, rb = a.step(act), b.step(act)
            o = ora.step(act)
            assert all(np.array_equal(x, y) for x, y in zip(ra[:3], rb[:3])), (it, t)
            assert np.array_equal(ra[0], o[0]) and np.array_equal(ra[2], o[2].astype(bool)), (it, t)
        da = {k: a.stats()[k] - base_a[k] for k in base_a}
        db = {k: b.stats()[k] - base_b[k] for k in base_b}
        assert da == db and da["episodes"] > 0 and da["errors"] == 0
        for e in _sample(n, 40, it):
            assert _state(a, e) == ora.get_state(e) and _finished(a, e) == ora.finished(e), e
        b.close()
    assert n_cut > 0 and n_ended > 0, (n_cut, n_ended)
    a.close()


# ---------------------------------------------------------------------------------- the tape paths afterwards
@pytest.mark.parametrize("rules", RULES)
def test_tape_paths_after_a_masked_reset(rules):
    """A handle WITH auto reset: a masked reset of envs in mid-episode and of envs whose installed state carries the
    finished bit, then 48 steps as single steps, as one persistent launch and as a step tape: all equal, and equal to the
    oracle."""
    import torch
    n, ns, T, M = 600, 2, 48, 9
    kw = dict(dim=10, n_snakes=ns, rules=rules, seed=83, max_steps=M, env_id_base=77)
    envs = [_mk(num_envs=n, **kw) for _ in range(3)]
    ora = _oracle(n, **kw)
    rs = np.random.default_rng(21)
    want = ora.reset()
    for env in envs:
        assert np.array_equal(env.reset(), want)
    for t in range(7):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        o = ora.step(act)[0]
        for env in envs:
            assert np.array_equal(env.step(act)[0], o), t
    for e in range(0, n, 9):  # finished episodes on a handle with auto reset exist only as installed states
        st = ora.get_state(e)
        st.update(finished=True, t=M + (e % 2))
        if rules == "new_world":  # (cut by the cap alone: the main snake's alive bit, [N]'s own end condition, is off)
            st["alive"][0], st["in_dead"][0] = False, True
        for env in envs:
            _set_both(env, ora, e, st)
    mask = _random_mask(rs, n)
    mask[::18] = True
    mask[9::18] = False
    shape = (n,) + envs[0].obs_shape
    w = [np.full(shape, SENTINEL, np.uint8), np.full(shape, SENTINEL, np.uint8), np.full(n, SENTINEL, np.uint8)]
    ora.reset_envs(mask, obs=w[0], final_obs=w[1], truncated=w[2])
    assert w[2].sum() > 0
    for env in envs:
        bufs = [torch.full(shape, SENTINEL, dtype=torch.uint8, device=env.device) for _ in range(2)]
        tr = torch.full((n,), SENTINEL, dtype=torch.uint8, device=env.device)
        env.reset_device(mask, out=bufs[0], final_out=bufs[1], truncated_out=tr)
        for got, x in zip(bufs + [tr], w):
            assert np.array_equal(got.cpu().numpy(), x)
    tape = rs.integers(0, 5, (T, n, ns)).astype(np.int32)
    tape_dev = torch.from_numpy(tape).to(envs[0].device)
    single = [tuple(x.clone() for x in envs[0].step_device(tape_dev[t])) for t in range(T)]
    runs = [envs[1].rollout_device(tape_dev, persistent=True), envs[2].rollout_device(tape_dev, persistent=False)]
    n_done = 0
    for t in range(T):
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(tape[t])
        s_obs, s_rew, s_done, s_info = (x.cpu().numpy() for x in single[t])
        assert np.array_equal(s_obs, o_obs) and np.array_equal(s_rew, o_rew) and np.array_equal(s_done, o_done), t
        assert np.array_equal(s_info[:, 2], o_ns) and np.array_equal(s_info[:, 1], o_el), t
        assert np.array_equal(s_info[:, 0].copy().view(np.float32), o_er), t
        for run in runs:
            assert all(torch.equal(x[t], y) for x, y in zip(run, single[t])), t
        n_done += int(o_done.sum())
    assert n_done > n
    for e in _sample(n, 40, 3):
        for env in envs:
            assert _state(env, e) == ora.get_state(e), e
    assert envs[0].stats() == envs[1].stats() == envs[2].stats() and envs[0].stats()["errors"] == 0
    for env in envs:
        env.close()
