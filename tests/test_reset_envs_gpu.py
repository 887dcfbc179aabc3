"""Masked per-env reset (msnake_reset_envs), terminal observations and truncation flags, on the MI355X.

* terminal_obs=True (msnake_step on a handle without auto reset, then msnake_reset_envs(done)) reproduces the in-kernel
  auto reset byte for byte, and adds the terminal observation and the truncation flag of every episode;
* both are checked against the CPU oracle run without auto reset and its own masked reset (Oracle.reset_envs, pinned to
  the reference's recordings by tests/test_oracle_reset_envs.py); one test also keeps the older emulation of it by state
  export / import (the unselected envs' words survive a full reset), which lives in that CPU test;
* a masked reset leaves the rows and the state of unselected envs alone, and an all-one mask is msnake_reset.
Bit-exact throughout: this is integer / byte work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONFIGS = [("snake_env", 10, 3), ("new_world", 10, 2), ("adversarial", 10, 3)]


def _mk(**kw):
    import msnake
    return msnake.MultiSnakeVecEnv(**kw)


def _oracle(**kw):
    from oracle.snake_oracle import Oracle
    return Oracle(**kw)


@pytest.mark.parametrize("scale", [1, 4])
@pytest.mark.parametrize("rules,dim,ns", CONFIGS)
def test_terminal_obs_equals_in_kernel_auto_reset(rules, dim, ns, scale):
    import torch
    n, steps, max_steps = 96, 100, 10
    kw = dict(num_envs=n, dim=dim, n_snakes=ns, rules=rules, seed=31, max_steps=max_steps, obs_scale=scale)
    a = _mk(**kw)
    b = _mk(terminal_obs=True, **kw)
    assert b.cfg.auto_reset == 0 and a.cfg.auto_reset == 1
    assert torch.equal(a.reset_device(), b.reset_device())
    g = torch.Generator().manual_seed(5)
    episodes = 0
    for t in range(steps):
        act = torch.randint(0, 5, (n, ns), generator=g, dtype=torch.int32).to(a.device)
        oa, ra, da, ia = a.step_device(act)
        ob, rb, db, ib = b.step_device(act)
        assert torch.equal(oa, ob), f"obs differs at step {t}"
        assert torch.equal(ra, rb) and torch.equal(da, db) and torch.equal(ia, ib), f"rew/done/info differ at step {t}"
        episodes += int(da.sum())
    assert episodes > n  # many episodes ended, and were reset, along the way
    assert np.array_equal(a.get_state_all(), b.get_state_all())
    assert a.stats() == b.stats()
    with pytest.raises(ValueError):
        b.rollout_device(torch.zeros((2, n, ns), dtype=torch.int32, device=b.device))
    a.close(); b.close()


@pytest.mark.parametrize("rules,dim,ns", CONFIGS)
def test_terminal_obs_and_truncation_against_the_oracle(rules, dim, ns):
    n, steps, max_steps = 128, 100, 10
    kw = dict(num_envs=n, dim=dim, n_snakes=ns, rules=rules, seed=47, max_steps=max_steps)
    env = _mk(terminal_obs=True, **kw)
    ora = _oracle(auto_reset=False, **kw)
    assert np.array_equal(env.reset(), ora.reset())
    rs = np.random.default_rng(3)
    n_trunc = n_term = 0
    for t in range(steps):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        obs, rew, done, infos = env.step(act)
        o_obs, o_rew, o_done = (x.copy() for x in ora.step(act)[:3])
        assert np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), f"rew/done differ at step {t}"
        want_obs, _, want_trunc = ora.reset_envs(o_done)  # (into ora.obs: the done envs' rows become their reset rows)
        want_trunc = want_trunc.copy()
        final, trunc = env.final_obs.cpu().numpy(), env.truncated.cpu().numpy()
        assert np.array_equal(final[done], o_obs[done]), f"terminal observations differ at step {t}"
        assert np.array_equal(trunc, want_trunc), f"truncation flags differ at step {t}"
        for e in np.nonzero(done)[0]:
            assert np.array_equal(infos[e]["terminal_observation"], o_obs[e])
            assert infos[e]["TimeLimit.truncated"] is bool(want_trunc[e])
        assert all("terminal_observation" not in infos[e] for e in np.nonzero(~done)[0][:8])
        n_trunc += int(want_trunc.sum())
        n_term += int(done.sum()) - int(want_trunc.sum())
        assert np.array_equal(obs, want_obs), f"reset observations differ at step {t}"
    assert n_trunc > 0 and n_term > 0, (n_trunc, n_term)
    env.close()


def test_masked_reset_without_auto_reset():
    import torch
    n, ns, dim, max_steps, sentinel = 40, 3, 10, 12, 0xA5
    kw = dict(num_envs=n, dim=dim, n_snakes=ns, rules="snake_env", seed=8, max_steps=max_steps)
    from reset_emulation import cut_by_time, emulated_masked_reset
    env = _mk(auto_reset=False, **kw)
    ora = _oracle(auto_reset=False, **kw)
    emu = _oracle(auto_reset=False, **kw)  # the same oracle, on which the masked reset is emulated by state export / import
    env.reset(); ora.reset(); emu.reset()
    rs = np.random.default_rng(11)

    def advance(k):
        for _ in range(k):
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            obs, rew, done, _ = env.step(act)
            o_obs, o_rew, o_done = ora.step(act)[:3]
            emu.step(act)
            assert np.array_equal(obs, o_obs) and np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool))

    one = np.zeros(n, bool)
    one[17] = True
    masks = [np.zeros(n, bool), np.ones(n, bool), one, rs.random(n) < 0.4]
    forms = [lambda m: m,                                                      # NumPy bool array
             lambda m: torch.from_numpy(m).to(env.device),                     # bool tensor
             lambda m: list(np.nonzero(m)[0]),                                 # env indices
             lambda m: torch.from_numpy(m.astype(np.uint8)).to(env.device)]    # uint8 tensor, used as it is
    shape = (n,) + env.obs_shape
    for i, (mask, form) in enumerate(zip(masks, forms)):
        advance(7)  # (some episodes end and stay finished: auto reset is off)
        before = [env.get_state_words(e) for e in range(n)]
        before_blob = env.get_state_all()
        final_want = ora.render().copy()
        assert [bool(before[e][7] & 0x100) for e in range(n)] == [ora.finished(e) for e in range(n)], i
        out = torch.full(shape, sentinel, dtype=torch.uint8, device=env.device)
        final_out = torch.full(shape, sentinel, dtype=torch.uint8, device=env.device)
        trunc_out = torch.full((n,), sentinel, dtype=torch.uint8, device=env.device)
        trunc_emu = np.array([mask[e] and bool(before[e][7] & 0x100) and cut_by_time(before[e], "snake_env", max_steps)
                              for e in range(n)], np.uint8)
        env.reset_device(form(mask), out=out, final_out=final_out, truncated_out=trunc_out)
        trunc_want = ora.reset_envs(mask)[2].copy()
        want = ora.render().copy()
        assert np.array_equal(ora.final_obs[mask], final_want[mask]), i
        assert np.array_equal(emulated_masked_reset(emu, mask), want) and np.array_equal(trunc_emu, trunc_want), i
        out, final_out, trunc = out.cpu().numpy(), final_out.cpu().numpy(), trunc_out.cpu().numpy()
        assert np.array_equal(out[mask], want[mask]), i
        assert np.array_equal(final_out[mask], final_want[mask]), i
        assert (out[~mask] == sentinel).all() and (final_out[~mask] == sentinel).all(), i
        assert np.array_equal(trunc, trunc_want), i
        for e in range(n):
            if not mask[e]:
                assert np.array_equal(env.get_state_words(e), before[e]), (i, e)
        assert np.array_equal(env.render(), want), i  # the handle's state is the emulated oracle's
        if mask.all():  # an all-one mask is msnake_reset
            blob = env.get_state_all()
            env.set_state_all(before_blob)
            assert np.array_equal(env.reset(), out) and np.array_equal(env.get_state_all(), blob)
    advance(30)
    env.close()


def test_masked_reset_mid_episode_is_not_counted():
    n, ns = 16, 3
    env = _mk(num_envs=n, dim=19, n_snakes=ns, rules="snake_env", seed=2, max_steps=2000)
    env.reset()
    rs = np.random.default_rng(1)
    for _ in range(4):
        env.step(rs.integers(0, 5, (n, ns)).astype(np.int32))
    running = [e for e in range(n) if env.get_state_words(e)[4] > 0][:3]  # envs with an episode in progress
    assert running
    before = env.stats()
    obs = env.reset(mask=running)
    after = env.stats()
    assert after == before  # the abandoned episodes are not counted
    for e in running:
        w = env.get_state_words(e)
        assert w[0] == 0 and w[4] == 0  # t and the episode length start over
    assert np.array_equal(obs, env.render())
    env.close()


def test_graph_capture_of_terminal_obs_step():
    import torch
    n, ns = 256, 3
    kw = dict(num_envs=n, dim=10, n_snakes=ns, rules="snake_env", seed=17, max_steps=9, terminal_obs=True)
    a, b = _mk(**kw), _mk(**kw)
    a.reset(); b.reset()
    acts = torch.zeros((n, ns), dtype=torch.int32, device=a.device)
    tape = torch.randint(0, 5, (30, n, ns), dtype=torch.int32, device=a.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        a.step_device(acts); b.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        a.step_device(acts)
    done_total = 0
    for t in range(30):
        acts.copy_(tape[t])
        g.replay()
        o, r, d, i = b.step_device(tape[t])
        assert torch.equal(a._obs, o) and torch.equal(a._rew, r) and torch.equal(a._done, d) and torch.equal(a._info, i), t
        assert torch.equal(a.final_obs, b.final_obs) and torch.equal(a.truncated, b.truncated), t
        done_total += int(d.sum())
    assert done_total > 0
    a.close(); b.close()


def test_reset_envs_errors():
    import torch
    import msnake
    n = 8
    env = _mk(num_envs=n, dim=19, n_snakes=3, rules="snake_env", seed=4, obs_scale=4)
    env.reset()
    L = msnake._capi.load()
    assert L.msnake_reset_envs(env._h, None, env._obs.data_ptr(), None, None, None) == -1  # MSNAKE_E_ARG
    shape = (n,) + env.obs_shape
    size = int(np.prod(shape))
    buf = torch.zeros(size + 4, dtype=torch.uint8, device=env.device)
    final_out = buf[1:1 + size].view(shape)  # one byte off a dword boundary
    out = torch.full(shape, 7, dtype=torch.uint8, device=env.device)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        env.reset_device([0, 1], out=out, final_out=final_out)
    torch.cuda.synchronize()
    assert (out == 7).all() and (buf == 0).all()  # nothing was launched
    with pytest.raises(ValueError):
        env.reset_device(np.ones(n - 1, bool))
    with pytest.raises(ValueError):
        env.reset_device(final_out=out)  # terminal observations need a mask
    with pytest.raises(ValueError):
        _mk(num_envs=n, dim=10, n_snakes=1, auto_reset=False, terminal_obs=True)
    env.close()
