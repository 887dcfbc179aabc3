"""The compile-time-shape step kernels (msnake_step_kernel<RULES, NS, MODE, K, DIM>) against the generic ones, bit for
bit, through every entry point that launches them, and against the golden tapes of the reference.  A handle created
under MSNAKE_GENERIC_KERNELS=1 keeps the generic kernels; everything else about the two handles is the same."""
import os

import numpy as np
import pytest

from golden_util import crc_rows, load_tape, state_view, unpack_state

pytestmark = pytest.mark.gpu

SHAPES = [(19, 3), (19, 2), (10, 1)]
N = 192  # not a multiple of the 64-workgroup grid group (8 envs each): workgroups beyond the batch are launched and leave


def _mk(generic=False, **kw):
    import msnake
    old = os.environ.get("MSNAKE_GENERIC_KERNELS")
    os.environ["MSNAKE_GENERIC_KERNELS"] = "1" if generic else "0"
    try:
        env = msnake.MultiSnakeVecEnv(**kw)
    finally:
        if old is None:
            del os.environ["MSNAKE_GENERIC_KERNELS"]
        else:
            os.environ["MSNAKE_GENERIC_KERNELS"] = old
    return env


def _pair(dim, ns, seed=5, **kw):
    spec = _mk(num_envs=N, dim=dim, n_snakes=ns, seed=seed, **kw)
    gen = _mk(generic=True, num_envs=N, dim=dim, n_snakes=ns, seed=seed, **kw)
    assert spec.kernel_name() == f"msnake_step_kernel<0, {ns}, 0, 1, {dim}>"
    assert gen.kernel_name() == f"msnake_step_kernel<0, {ns}, 0, 1>"
    return spec, gen


def _tape(T, ns, width=None, seed=11):
    import torch
    rs = np.random.default_rng(seed)
    a = rs.integers(0, 5, (T, N, width or ns)).astype(np.int32)
    return torch.from_numpy(a).cuda()


def _same_state(a, b):
    assert bytes(a.get_state_all()) == bytes(b.get_state_all())


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_per_step_launches_match_the_generic_kernel(dim, ns):
    import torch
    spec, gen = _pair(dim, ns)
    assert torch.equal(spec.reset_device(), gen.reset_device())
    tape = _tape(400, ns)
    eats = 0
    for t in range(400):
        a = spec.step_device(tape[t])
        b = gen.step_device(tape[t])
        for x, y, what in zip(a, b, ("obs", "reward", "done", "info")):
            assert torch.equal(x, y), (what, t)
        eats += int((a[1] > 0).sum())
    _same_state(spec, gen)
    # the slow paths ran too: fruits were eaten (a respawn each) and episodes ended (a reset each)
    st, sg = spec.stats(), gen.stats()
    assert st == sg and st["errors"] == 0 and st["env_steps"] == 400 * N
    assert st["episodes"] > 0 and eats > 0, (st, eats)
    if (dim, ns) == (19, 3):
        assert st["episodes"] >= 100 and eats >= 100, (st, eats)
    spec.close(); gen.close()


@pytest.mark.parametrize("keep_obs", [True, False], ids=["stride_one_batch", "stride_0"])
@pytest.mark.parametrize("dim,ns", SHAPES)
def test_rollout_tape_matches_the_generic_kernel(dim, ns, keep_obs):
    import torch
    spec, gen = _pair(dim, ns)
    spec.reset_device(); gen.reset_device()
    tape = _tape(64, ns)
    for r in range(2):  # (the second launch starts from grown snakes and used-up parked draws)
        a = spec.rollout_device(tape, persistent=True, keep_obs=keep_obs)
        b = gen.rollout_device(tape, persistent=True, keep_obs=keep_obs)
        for x, y, what in zip(a, b, ("obs", "reward", "done", "info")):
            assert torch.equal(x, y), (what, r)
    _same_state(spec, gen)
    st = spec.stats()
    assert st == gen.stats() and st["errors"] == 0 and st["episodes"] > 0
    spec.close(); gen.close()


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_rollout_tape_with_an_unaligned_step_stride_matches_the_generic_kernel(dim, ns):
    """A step stride that is no multiple of 16 bytes takes the persistent kernel's byte-aligned copy-out (one batch of
    192 envs is a multiple of 16 at every compiled shape, so the other rollout cases never do): a padded stride, five
    guard bytes behind every step's observations, which must survive."""
    import torch
    from msnake import _capi
    spec, gen = _pair(dim, ns)
    spec.reset_device(); gen.reset_device()
    T = 64
    tape = _tape(T, ns)
    H, W, C = spec.obs_shape
    batch = N * H * W * C
    stride = batch + 5
    assert batch % 16 == 0 and stride % 16 != 0
    out = []
    for env in (spec, gen):
        obs = torch.full((T * stride,), 0xA5, dtype=torch.uint8, device="cuda")
        rew = torch.empty((T, N), dtype=torch.float32, device="cuda")
        done = torch.empty((T, N), dtype=torch.uint8, device="cuda")
        info = torch.empty((T, N, 4), dtype=torch.int32, device="cuda")
        _capi.check(env._L.msnake_rollout_tape(env._h, tape.data_ptr(), ns, T, obs.data_ptr(), stride, rew.data_ptr(),
                                               done.data_ptr(), info.data_ptr(), N, env._stream()), "msnake_rollout_tape")
        out.append((obs.view(T, stride), rew, done, info))
    for x, y, what in zip(out[0], out[1], ("obs", "reward", "done", "info")):
        assert torch.equal(x, y), what
    assert bool((out[0][0][:, batch:] == 0xA5).all()), "guard bytes between the steps' observations were written"
    # ... and the padded layout holds what the aligned one does
    spec2, gen2 = _pair(dim, ns)
    gen2.close()
    spec2.reset_device()
    ref = spec2.rollout_device(tape, persistent=True, keep_obs=True)
    assert torch.equal(out[0][0][:, :batch], ref[0].view(T, batch))
    _same_state(spec, gen)
    _same_state(spec, spec2)
    assert spec.stats() == gen.stats() and spec.stats()["errors"] == 0
    spec.close(); gen.close(); spec2.close()


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_step_tape_matches_the_generic_kernel(dim, ns):
    import torch
    spec, gen = _pair(dim, ns)
    spec.reset_device(); gen.reset_device()
    tape = _tape(64, ns)
    a = spec.rollout_device(tape, persistent=False, keep_obs=True)  # msnake_step_tape, per-step observation slices
    b = gen.rollout_device(tape, persistent=False, keep_obs=True)
    for x, y, what in zip(a, b, ("obs", "reward", "done", "info")):
        assert torch.equal(x, y), what
    # ... and the persistent kernel from the same start gives the per-step launches' results
    spec2, _gen2 = _pair(dim, ns)
    _gen2.close()
    spec2.reset_device()
    c = spec2.rollout_device(tape, persistent=True, keep_obs=True)
    for x, y, what in zip(a, c, ("obs", "reward", "done", "info")):
        assert torch.equal(x, y), what
    _same_state(spec, gen)
    _same_state(spec, spec2)
    spec.close(); gen.close(); spec2.close()


@pytest.mark.parametrize("name", ["tape_S_19x19_3", "tape_S_19x19_2"])
def test_compiled_shape_replays_the_golden_tape(name):
    from oracle.snake_oracle import flat_to_state
    meta, z = load_tape(name)
    rules, E, T = meta["rules"], meta["num_envs"], meta["steps"]
    assert rules == 0 and meta["auto_reset"]
    env = _mk(num_envs=E, dim=meta["dim"], n_snakes=meta["n_snakes"], n_fruits=meta["n_fruits"], rules=rules,
              seed=meta["seed"], env_id_base=meta["env_id_base"], max_steps=meta["max_steps"], auto_reset=meta["auto_reset"])
    assert env.kernel_name() == f"msnake_step_kernel<0, {meta['n_snakes']}, 0, 1, 19>"
    state = lambda e: state_view(flat_to_state(env.get_state_words(e)), rules)
    assert np.array_equal(env.reset(), z["obs0"])
    for e in range(E):
        assert state(e) == unpack_state(z, "s0_", 0, e, rules)
    full_t = {int(t): i for i, t in enumerate(z["full_obs_t"])}
    actions = z["actions"].astype(np.int32)
    for t in range(T):
        obs, rew, done, infos = env.step(actions[t])
        assert np.array_equal(rew, z["reward"][t]), (name, t)
        assert np.array_equal(done, z["done"][t].astype(bool)), (name, t)
        assert np.array_equal(infos._ns, z["num_snakes"][t].astype(np.int32)), (name, t)
        assert np.array_equal(infos._r, z["ep_return"][t]), (name, t)
        assert np.array_equal(infos._l, z["ep_len"][t]), (name, t)
        assert np.array_equal(crc_rows(obs), z["obs_crc"][t]), (name, t)
        if t in full_t:
            assert np.array_equal(obs, z["full_obs"][full_t[t]]), (name, t)
        if t % 16 == 0 or t == T - 1:
            for e in range(0, E, 3):
                assert state(e) == unpack_state(z, "st_", t, e, rules), (name, t, e)
    assert env.stats()["errors"] == 0
    env.close()


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_a_padded_action_stride_falls_back_per_call(dim, ns):
    """action_stride is folded into the compiled shapes (== n_snakes): a call with another stride runs the generic
    kernel for that call, and the handle goes back to its compiled shape afterwards."""
    import torch
    spec, gen = _pair(dim, ns)
    spec.reset_device(); gen.reset_device()
    wide = _tape(50, ns, width=4)
    wide[:, :, ns:] = 7  # padding columns: never an action of a snake
    for t in range(50):
        a = spec.step_device(wide[t])
        b = gen.step_device(wide[t])
        for x, y, what in zip(a, b, ("obs", "reward", "done", "info")):
            assert torch.equal(x, y), (what, t)
    narrow = wide[:, :, :ns].contiguous()
    for t in range(50):  # the same handle, back on its compiled shape, interleaved with padded calls
        a = spec.step_device(narrow[t] if t % 2 else wide[t])
        b = gen.step_device(narrow[t])
        for x, y, what in zip(a, b, ("obs", "reward", "done", "info")):
            assert torch.equal(x, y), (what, t)
    _same_state(spec, gen)
    assert spec.stats() == gen.stats()
    spec.close(); gen.close()
