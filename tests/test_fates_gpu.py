"""The fate of every move, the two masks and the opponent wary_greedy on the device (msnake_fate_actions) against
tests/fates_play.py.

Everything is byte-exact and nothing is left out of a comparison: every env, snake and action.  The expectations are
fates_play.np_fates and fates_play.wary_choice on the canonical state of the CPU oracle or on a hand-built state dict;
none of them ever comes from the library under test.  Every output sits between guard elements.
"""
import ctypes
import itertools

import numpy as np
import pytest

import fates_play as fp
import gpu_harness as gh
import scripted_play as sp

pytestmark = pytest.mark.gpu

E_ARG, E_HANDLE = -1, -3
FILL, BFILL = -77, 0xA5
OUTPUTS = ("fate", "by", "eat", "mask")


def _cfg(rules, dim, ns, num_envs, seed=3, **kw):
    return dict(sp.scenario(rules, dim, ns, "wary_greedy", 0, num_envs, seed, max_steps=60), **kw)


def Bufs(env, stride=None):
    n, S = env.num_envs, env.n_snakes
    byte = dict(dtype="uint8", fill=BFILL, offset=1, align=4)   # payloads at odd addresses: no output needs alignment
    spec = {"act": dict(dtype="int32", shape=(n, stride or S), fill=FILL)}
    spec.update({k: dict(byte, shape=(n, S, 2 if k == "mask" else 5)) for k in OUTPUTS})
    return gh.GuardedOutputs(env.device, spec)


def _stream(env):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)


def _raw(env, bits, act=None, stride=0, fate=None, by=None, eat=None, mask=None):
    """msnake_fate_actions itself, on the current stream; outputs are addresses (or None)."""
    return env._L.msnake_fate_actions(env._h if env is not None else None, bits, act, stride, fate, by, eat, mask, _stream(env))


def _call(env, buf, bits=None, which=OUTPUTS):
    bits = (1 << env.n_snakes) - 1 if bits is None else bits
    ptr = {k: (getattr(buf, k).data_ptr() if k in which else None) for k in OUTPUTS}
    rc = _raw(env, bits, buf.act.data_ptr() if bits else None, int(buf.act.shape[1]) if bits else 0, **ptr)
    assert rc == 0, env._L.msnake_last_error()


def _diff(what, name, got, want, states):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, name, bad[:5].tolist(), got[bad[0][0]].tolist(), want[bad[0][0]].tolist(), states[bad[0][0]])


def _check(env, cfg, states, what="", buf=None):
    """One call with everything; every output against the model.  Returns (buf, the expectations)."""
    buf = buf or Bufs(env)
    want = fp.expected(cfg, states)
    buf.refill()
    _call(env, buf)
    _diff(what, "action", buf.host("act")[:, :env.n_snakes], want[0], states)
    for k, w in zip(OUTPUTS, want[1:]):
        _diff(what, k, buf.host(k), w, states)
    assert buf.guards_intact(), what
    return buf, want


# ------------------------------------------------------------------------------------------ 1. hand-built states
@pytest.mark.parametrize("rules", ["snake_env", "adversarial"])
def test_hand_built_states(rules):
    names, states, wants = fp.hand_states(rules)
    cfg = fp.hand_cfg(rules, len(states))
    env = gh.install(cfg, states)
    buf, want = _check(env, dict(cfg, num_envs=len(states)), states, rules)
    fate = buf.host("fate")
    for e, (name, bits) in enumerate(zip(names, wants)):           # and the bits each state was built for, as literals
        for (s, a), (on, off) in bits.items():
            assert fate[e, s, a] & on == on and fate[e, s, a] & off == 0, (name, s, a, int(fate[e, s, a]))
    env.close()


@pytest.mark.parametrize("rules", ["snake_env", "adversarial"])
def test_a_tail_out_of_the_overflow_ring_decides(rules):
    """A body of 70 pieces on 10x10: its last piece, 6 entries into the overflow ring, is BODY while it grows and TAIL
    when it does not, and the pieces before it come out of both rings."""
    states = [fp.long_body_state(False), fp.long_body_state(True)]
    # a head at -1 that runs into piece 66 of the long body: a piece of the overflow ring that is not the last one
    st = fp.long_body_state(False)
    assert st["snakes"][0][66] == [0, 4]
    st["snakes"][2], st["vels"][2] = [[-1, 4]], [1, 0]
    states.append(st)
    cfg = _cfg(rules, 10, 3, len(states))
    env = gh.install(cfg, states)
    buf, _ = _check(env, cfg, states, rules)
    fate, by = buf.host("fate"), buf.host("by")
    assert fate[0, 1, 2] == fp.TAIL and by[0, 1, 2] == 0x10 and fate[1, 1, 2] == fp.BODY
    assert fate[2, 2, 0] == fp.BODY
    env.close()


def test_an_eaten_fruit_behind_entry_64_of_the_adversarial_list():
    filler = [(x, y) for x in (0, 1) for y in range(10)] * 4          # 80 entries on the rows 0 and 1
    fruits = filler[:66] + [(6, 5), (9, 9), (6, 5), (4, 5)]
    st = fp.state([[(5, 5), (4, 5), (3, 5)], [(8, 8), (8, 7)], [(3, 9), (3, 8)]], [(1, 0), (0, 1), (0, 1)], fruits)
    near = fp.state([[(5, 5), (4, 5), (3, 5)], [(8, 8), (8, 7)], [(3, 9), (3, 8)]], [(1, 0), (0, 1), (0, 1)], fruits[:64] + [(6, 5)])
    cfg = _cfg("adversarial", 10, 3, 2)
    env = gh.install(cfg, [st, near])
    buf, _ = _check(env, cfg, [st, near])
    eat, fate = buf.host("eat"), buf.host("fate")
    assert eat[0, 0].tolist() == [2, 2, 0, 2, 0] and eat[1, 0].tolist() == [1, 1, 0, 1, 0] and fate[0, 0, 1] == fp.EATS
    assert buf.host("act")[0, 0] == 1                                  # distance 0: the fruit behind entry 64 is seen
    env.close()


# ------------------------------------------------------------------------------------------ 2. closed loops
def _loop(cfg, steps, control=None, stride=None, states_every=20, **kw):
    """gpu_harness.closed_loop with all five outputs compared at every step, and the env's canonical states against the
    oracle's every `states_every` steps."""
    from oracle.snake_oracle import flat_to_state
    env = gh.make_env(cfg, **kw)

    def call(env, buf, snakes):
        bits = (1 << env.n_snakes) - 1 if snakes is None else sum(1 << s for s in snakes)
        _call(env, buf, bits)
        return buf.act, buf.host("mask"), buf.host("fate"), buf.host("by"), buf.host("eat")

    def expected(states):
        act, fate, by, eat, mask = fp.expected(cfg, states)
        return act, mask, fate, by, eat

    def observe(t, states, wants, o_done, o_el):
        if t % states_every == 0:
            for e in range(cfg["num_envs"]):
                got = flat_to_state(env.get_state_words(e))
                assert got == states[e], (t, e)

    gh.closed_loop(cfg, env, call, expected, steps, control=control, stride=stride, observe=observe, buffers=Bufs)
    return env


@pytest.mark.parametrize("rules,dim,epb", [("snake_env", 5, 1), ("snake_env", 5, 8), ("adversarial", 6, 1), ("adversarial", 6, 8)])
def test_play_of_67_envs(rules, dim, epb):
    """67 envs (no multiple of the 4 envs of a workgroup), 150 steps, snake 1 under seeded random actions so that bodies
    meet: every output at every step."""
    env = _loop(_cfg(rules, dim, 3, 67), 150, control=(np.random.default_rng([5, dim, epb]), (0, 2)), stride=5, envs_per_block=epb)
    env.close()


def test_closed_loop_of_200_steps_all_snakes_wary():
    env = _loop(_cfg("snake_env", 6, 3, 24, seed=9), 200, states_every=10)
    env.close()


def test_nobody_else_on_the_board():
    env = _loop(_cfg("snake_env", 10, 1, 16), 120)
    env.close()


def test_a_handle_on_its_compiled_shape_kernel():
    cfg = dict(_cfg("snake_env", 19, 3, 32, seed=4), max_steps=2000)
    env = _loop(cfg, 60)
    assert env.kernel_name().endswith(", 19>"), env.kernel_name()
    env.close()


# ------------------------------------------------------------------------------------------ 3. the outputs and the selection
def _played(rules, dim, num_envs, steps, seed=6):
    """A handle and an oracle `steps` steps into the same wary play with noise; returns (cfg, env, states)."""
    import torch
    cfg = _cfg(rules, dim, 3, num_envs, seed=seed, eps=0.2)
    env, ora = gh.make_env(cfg), sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    rs = sp.policy_rng(cfg)
    for _ in range(steps):
        act = fp.choose_actions(cfg, gh.oracle_states(ora), rs)
        ora.step(act, want_obs=False)
        env.step_device(torch.from_numpy(act).to(env.device))
    return cfg, env, gh.oracle_states(ora)


def test_each_output_alone_all_together_and_every_snake_mask():
    cfg, env, states = _played("adversarial", 6, 21, 40)
    buf = Bufs(env, stride=5)
    want = dict(zip(("act",) + OUTPUTS, fp.expected(cfg, states)))
    assert want["fate"].any() and want["by"].any() and want["eat"].any()
    for bits in range(8):
        for pick in itertools.product((False, True), repeat=4):
            which = tuple(k for k, on in zip(OUTPUTS, pick) if on)
            if not bits and not which:
                continue                                                  # nothing to write: an argument error (below)
            if bits not in (0, 7) and len(which) not in (0, 4):
                continue                                                  # every selection with nothing and with everything
            buf.refill()
            _call(env, buf, bits, which)
            got = buf.host("act")
            for s in range(5):
                if s < 3 and bits >> s & 1:
                    assert np.array_equal(got[:, s], want["act"][:, s]), (bits, which, s)
                else:
                    assert (got[:, s] == FILL).all(), (bits, which, s, "an unselected column was written")
            for k in OUTPUTS:
                assert np.array_equal(buf.host(k), want[k]) if k in which else buf.untouched(k), (bits, which, k)
            assert buf.guards_intact(), (bits, which)
    # the Python surface: fresh tensors, the caller's tensors, the masks alone, the policy by name
    res = env.move_fates_device()
    assert res.by is None and res.eat is None and np.array_equal(res.fate.cpu().numpy(), want["fate"])
    assert np.array_equal(res.mask.cpu().numpy(), want["mask"])
    res = env.move_fates_device(fate=False, by=True, eat=True, mask=False)
    assert res.fate is None and np.array_equal(res.by.cpu().numpy(), want["by"]) and np.array_equal(res.eat.cpu().numpy(), want["eat"])
    assert np.array_equal(env.fate_masks_device().cpu().numpy(), want["mask"])
    buf.refill()
    assert env.fate_masks_device(out=buf.mask) is buf.mask and np.array_equal(buf.host("mask"), want["mask"])
    assert all(buf.untouched(k) for k in ("act", "fate", "by", "eat"))
    out = env.scripted_actions_device("wary_greedy", snakes=[2, 0], out=buf.act)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, [0, 2]], want["act"][:, [0, 2]]) and (got[:, [1, 3, 4]] == FILL).all()
    assert np.array_equal(env.scripted_actions_device("wary_greedy").cpu().numpy(), want["act"])
    env.close()


def test_every_refusal_in_order():
    import torch
    cfg = _cfg("snake_env", 6, 3, 5)
    env = gh.make_env(cfg)
    env.reset()
    nw = gh.make_env(dict(sp.scenario("new_world", 6, 3, "safe_greedy", 0, 5, 1, n_fruits=4)))
    nw.reset()
    buf = Bufs(env, stride=4)
    A, F = buf.act.data_ptr(), buf.fate.data_ptr()
    last = lambda: env._L.msnake_last_error().decode()
    # 1. the handle
    assert env._L.msnake_fate_actions(None, 1, A, 4, F, None, None, None, _stream(env)) == E_HANDLE and "handle" in last()
    # 2. new_world, in front of everything about the arguments
    assert _raw(nw, 0x10, None, 0) == E_ARG and "new_world" in last()
    assert _raw(nw, 1, A, 4, F) == E_ARG and "new_world" in last()
    # 3. a snake_mask bit >= n_snakes, in front of the action buffer
    assert _raw(env, 0b1000, None, 0, F) == E_ARG and "snake_mask" in last()
    # 4. the action buffer, only when actions are written
    assert _raw(env, 1, None, 4, F) == E_ARG and "actions_dev is NULL" in last()
    assert _raw(env, 1, A, 2, F) == E_ARG and "action_stride" in last()
    assert _raw(env, 1, None, 2) == E_ARG and "actions_dev is NULL" in last()       # in front of `nothing to write`
    # 5. nothing to write
    assert _raw(env, 0, A, 4) == E_ARG and "nothing to write" in last()
    assert _raw(env, 0, None, 0) == E_ARG and "nothing to write" in last()
    torch.cuda.synchronize()
    assert all(buf.untouched(k) for k in ("act",) + OUTPUTS), "a refused call wrote"
    assert _raw(env, 0, None, 0, F) == 0                                              # mask 0 needs no action buffer
    torch.cuda.synchronize()
    assert buf.untouched("act") and not buf.untouched("fate")
    with pytest.raises(RuntimeError, match="new_world"):
        nw.move_fates_device()
    env.close(), nw.close()


# ------------------------------------------------------------------------------------------ 4. read-only, HIP graph
def test_graph_of_fate_actions_then_step_equals_the_eager_run():
    """[msnake_fate_actions -> msnake_step] captured and replayed 60 times against the same two calls made eagerly on a
    twin handle, step for step; the call alone changes neither the state (the Philox counter is part of it) nor
    env_steps."""
    import torch
    cfg = _cfg("adversarial", 6, 3, 37, seed=12)
    K = 60
    env, twin = gh.make_env(cfg), gh.make_env(cfg)
    assert np.array_equal(env.reset(), twin.reset())
    blob = env.get_state_all()
    before, steps_before = blob.tobytes(), env.stats()["env_steps"]
    acts = torch.zeros((37, 3), dtype=torch.int32, device=env.device)
    fates = env.move_fates_device(by=True, eat=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.scripted_actions_device("wary_greedy", out=acts, fates_out=fates)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert env.get_state_all().tobytes() == before and env.stats()["env_steps"] == steps_before   # the call alone: nothing moved
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("wary_greedy", out=acts, fates_out=fates)
        out = env.step_device(acts)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # (whether or not the capture ran anything)
    t_acts = torch.zeros_like(acts)
    for t in range(K):
        g.replay()
        twin.scripted_actions_device("wary_greedy", out=t_acts)
        want = twin.move_fates_device(by=True, eat=True)
        t_out = twin.step_device(t_acts)
        assert torch.equal(acts, t_acts), t
        assert all(torch.equal(a, b) for a, b in zip(fates, want)), t
        assert all(torch.equal(a, b) for a, b in zip(out, t_out)), t
    torch.cuda.synchronize()
    assert env.get_state_all().tobytes() == twin.get_state_all().tobytes()
    assert twin.stats()["env_steps"] == K * 37                     # the fate calls added nothing
    # and the eager twin is where the model on the oracle is
    ora = sp.make_oracle(cfg)
    ora.reset()
    for _ in range(K):
        ora.step(fp.expected(cfg, gh.oracle_states(ora))[0], want_obs=False)
    from oracle.snake_oracle import flat_to_state
    assert [flat_to_state(twin.get_state_words(e)) for e in range(37)] == gh.oracle_states(ora)
    env.close(), twin.close()
