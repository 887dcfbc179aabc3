"""The two per-step kernels of a compiled shape -- the plain-call variant (every output given, the observation base on
a 128-byte line) and the first variant (any other call) -- against the generic kernel, bit for bit: observations, reward,
done, info and the exported state, with a handle created under MSNAKE_GENERIC_KERNELS=1 that has the same seed and gets
the same actions, over enough steps for respawns and resets.  160 envs at 19x19: every shift (16) and every lead (8) of
the aligned copy-out occurs, the last workgroup is partly filled and the grid is rounded up to 64 workgroups; 24 envs at
10x10x1, where the shift is always 0 and the lead varies.  Every observation buffer sits between 256 guard bytes that
must survive.  Each case asserts on the host's choice (msnake_call_shape_for_config) that it runs the kernel it is for."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(19, 3, 160), (19, 2, 160), (10, 1, 24)]
T = 48
GUARD = 256
FILL = 0xA5


def _mk(n, dim, ns, generic=False, **kw):
    import msnake
    old = os.environ.get("MSNAKE_GENERIC_KERNELS")
    os.environ["MSNAKE_GENERIC_KERNELS"] = "1" if generic else "0"
    try:
        env = msnake.MultiSnakeVecEnv(num_envs=n, dim=dim, n_snakes=ns, seed=9, **kw)
    finally:
        if old is None:
            del os.environ["MSNAKE_GENERIC_KERNELS"]
        else:
            os.environ["MSNAKE_GENERIC_KERNELS"] = old
    assert env.kernel_name() == (f"msnake_step_kernel<0, {ns}, 0, 1>" if generic else f"msnake_step_kernel<0, {ns}, 0, 1, {dim}>")
    return env


def _actions(n, ns, steps=T):
    import torch
    return torch.from_numpy(np.random.default_rng(21).integers(0, 5, (steps, n, ns)).astype(np.int32)).cuda()


@functools.lru_cache(maxsize=None)
def _reference(dim, ns, n):
    """The generic kernels' T steps from reset, computed once per shape: per step (obs, rew, done, info), and the state."""
    gen = _mk(n, dim, ns, generic=True)
    gen.reset_device()
    tape = _actions(n, ns)
    steps = []
    for t in range(T):
        steps.append(tuple(x.clone() for x in gen.step_device(tape[t])))
    state = bytes(gen.get_state_all())
    st = gen.stats()
    assert st["errors"] == 0 and st["episodes"] > 0, st                 # resets ran ...
    assert sum(int((s[1] > 0).sum()) for s in steps) > 0                # ... and respawns
    gen.close()
    return steps, state


class Guarded:
    """`nbytes` of observations `offset` bytes behind a 128-byte line, 256 guard bytes in front and behind."""

    def __init__(self, nbytes, offset=0):
        import torch
        self.whole = torch.full((GUARD + 128 + offset + nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        base = self.whole.data_ptr()
        self.start = (base + GUARD + 127) // 128 * 128 + offset - base
        self.nbytes = nbytes
        self.ptr = base + self.start
        assert (self.ptr - offset) % 128 == 0 and self.start >= GUARD

    def data(self):
        return self.whole[self.start:self.start + self.nbytes]

    def check(self):
        assert bool((self.whole[:self.start] == FILL).all()), "bytes in front of the observations were written"
        assert bool((self.whole[self.start + self.nbytes:] == FILL).all()), "bytes behind the observations were written"


def _want(env, obs_ptr, info=True):
    from msnake import _capi
    return _capi.call_shape_for_config(env.cfg, env.n_snakes, obs_ptr, env._p_rew, env._p_done, env._p_info if info else 0)


def _step(env, acts, obs_ptr, info=True):
    from msnake import _capi
    _capi.check(env._L.msnake_step(env._h, acts.data_ptr(), env.n_snakes, obs_ptr or None, env._p_rew, env._p_done,
                                   env._p_info if info else None, env._stream()), "msnake_step")


def _run(dim, ns, n, offsets, want, obs=True, info=True, **kw):
    """T steps from reset; step t writes its observations at offset offsets[t % len(offsets)] behind a 128-byte line."""
    import torch
    ref, ref_state = _reference(dim, ns, n)
    env = _mk(n, dim, ns, **kw)
    env.reset_device()
    tape = _actions(n, ns)
    S = int(np.prod(env.obs_shape))
    bufs = [Guarded(n * S, off) for off in offsets]
    env._info.fill_(-7)
    for t in range(T):
        b = bufs[t % len(bufs)]
        assert _want(env, b.ptr if obs else 0, info) == want[t % len(want)]
        _step(env, tape[t], b.ptr if obs else 0, info)
        if obs:
            assert torch.equal(b.data(), ref[t][0].reshape(-1)), ("obs", t)
        assert torch.equal(env._rew, ref[t][1]) and torch.equal(env._done, ref[t][2]), ("reward / done", t)
        if info:
            assert torch.equal(env._info, ref[t][3]), ("info", t)
    for b in bufs:
        b.check()
        if not obs:
            assert bool((b.whole == FILL).all())
    if not info:
        assert bool((env._info == -7).all())
    assert bytes(env.get_state_all()) == ref_state
    assert env.stats()["errors"] == 0
    env.close()


@pytest.mark.parametrize("policy", ["plain", "stream"])
@pytest.mark.parametrize("dim,ns,n", SHAPES)
def test_plain_calls_match_the_generic_kernel(dim, ns, n, policy):
    _run(dim, ns, n, [0], ["plain"], obs_store_policy=policy)


@pytest.mark.parametrize("offset", [16, 1])
def test_an_unaligned_base_runs_the_first_variant(offset):
    _run(19, 3, 160, [offset], ["shape"])


def test_a_call_without_info_runs_the_first_variant():
    _run(19, 3, 160, [0], ["shape"], info=False)


def test_a_call_without_observations_runs_the_first_variant():
    _run(19, 3, 160, [0], ["shape"], obs=False)


@pytest.mark.parametrize("dim,ns,n", SHAPES)
def test_both_variants_interleaved_on_one_handle(dim, ns, n):
    _run(dim, ns, n, [0, 16, 0, 1, 64], ["plain", "shape", "plain", "shape", "shape"])


def test_step_tape_whose_steps_alternate_between_the_variants():
    """One msnake_step_tape call, every step's observations in its own slice: 160 * 3969 bytes per step is a multiple of
    16 but not of 128, so the steps of ONE call run both variants."""
    import torch
    from msnake import _capi
    dim, ns, n, K = 19, 3, 160, 8
    ref, _ = _reference(dim, ns, n)
    env = _mk(n, dim, ns)
    env.reset_device()
    tape = _actions(n, ns)
    S = int(np.prod(env.obs_shape))
    stride = n * S
    assert stride % 16 == 0 and stride % 128 != 0
    buf = Guarded(K * stride)
    rew = torch.empty((K, n), dtype=torch.float32, device="cuda")
    done = torch.empty((K, n), dtype=torch.uint8, device="cuda")
    info = torch.empty((K, n, 4), dtype=torch.int32, device="cuda")
    got = [_capi.call_shape_for_config(env.cfg, ns, buf.ptr + k * stride, rew[k].data_ptr(), done[k].data_ptr(), info[k].data_ptr())
           for k in range(K)]
    assert got == ["plain" if (k * stride) % 128 == 0 else "shape" for k in range(K)]
    assert got.count("plain") >= 2 and got.count("shape") >= 2, got
    _capi.check(env._L.msnake_step_tape(env._h, tape.data_ptr(), ns, K, buf.ptr, stride, rew.data_ptr(), done.data_ptr(),
                                        info.data_ptr(), n, env._stream()), "msnake_step_tape")
    obs = buf.data().view(K, stride)
    for k in range(K):
        assert torch.equal(obs[k], ref[k][0].reshape(-1)), ("obs", k)
        assert torch.equal(rew[k], ref[k][1]) and torch.equal(done[k], ref[k][2]) and torch.equal(info[k], ref[k][3]), k
    buf.check()
    # ... and the handle goes on from there like the generic one
    for t in range(K, T):
        out = env.step_device(tape[t])
        for x, y, what in zip(out, ref[t], ("obs", "reward", "done", "info")):
            assert torch.equal(x, y), (what, t)
    assert bytes(env.get_state_all()) == _reference(dim, ns, n)[1]
    env.close()


def test_a_captured_plain_call_replays():
    import torch
    dim, ns, n = 19, 3, 160
    ref, _ = _reference(dim, ns, n)
    env = _mk(n, dim, ns)
    env.reset()
    blob = env.get_state_all()
    tape = _actions(n, ns)
    S = int(np.prod(env.obs_shape))
    buf = Guarded(n * S)
    assert _want(env, buf.ptr) == "plain"
    acts = torch.zeros((n, ns), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        _step(env, acts, buf.ptr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _step(env, acts, buf.ptr)
    torch.cuda.synchronize()
    env.set_state_all(blob)  # warm-up and capture aside: back to the state after reset()
    for t in range(20):
        acts.copy_(tape[t])
        g.replay()
        assert torch.equal(buf.data(), ref[t][0].reshape(-1)), ("obs", t)
        assert torch.equal(env._rew, ref[t][1]) and torch.equal(env._done, ref[t][2]) and torch.equal(env._info, ref[t][3]), t
    buf.check()
    env.close()
