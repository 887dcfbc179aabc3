"""Exploring play on the GPU: msnake_explore_actions against the restatement np_explore_actions (tests/explore_play.py) on
all three rule sets, every policy and eps mix, a wider stride and a partial mask; msnake_playout_explore against
np_playout_explore in all six outputs for every scenario; both against the entry points they extend at eps 0; the playout
against the library's own loop of [msnake_explore_actions -> msnake_step -> msnake_agent_outcomes]; the handle left as it
was, graph capture, every refusal in order, playout_values_device, and the reason for the feature: reps that differ."""
import ctypes

import numpy as np
import pytest
import torch

import msnake
import explore_play as xp
import gpu_harness as gh
import playout_play as pp
import scripted_play as sp
from oracle.snake_oracle import state_to_flat

pytestmark = pytest.mark.gpu
C = msnake._capi
NAMES = ("steps", "end", "ret", "info", "words", "count")
ONE = xp.ONE


def handle(cfg, states, **kw):
    """A handle holding `states` (dicts, `finished` included), one env each, at cfg's seed and env ids."""
    env = gh.make_env(dict(cfg, num_envs=len(states)), **kw)
    env.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, cfg["n_snakes"]))
    return env


def action_buffers(env, stride=None):
    n, ns = env.num_envs, env.n_snakes
    return gh.GuardedOutputs(env.device, {"act": dict(dtype="int32", shape=(n, stride or ns), fill=-77),
                                          "explored": dict(dtype="uint8", shape=(n, ns), fill=0xA5)})


def playout_buffers(env):
    n, ns = env.num_envs, env.n_snakes
    return gh.GuardedOutputs(env.device, {
        "steps": dict(dtype="int32", shape=(n,), fill=-77), "end": dict(dtype="uint8", shape=(n,), fill=0xA5),
        "ret": dict(dtype="float32", shape=(n, ns), fill=-77.5), "info": dict(dtype="int32", shape=(n, ns, 4), fill=-77),
        "words": dict(dtype="int32", shape=(n, env.state_words_max), fill=-77), "count": dict(dtype="int32", shape=(n,), fill=-77)})


def probs(eps_q16):
    return [q / ONE for q in eps_q16]                               # exact: round(p * 65536) gives the entry back


def check_actions(env, cfg, states, policies, eps_q16, salt=0, snakes=None, stride=None, label=""):
    """One msnake_explore_actions call on `env`, which holds `states`, against the restatement."""
    ns = cfg["n_snakes"]
    buf = action_buffers(env, stride)
    env.explore_actions_device(policies, probs(eps_q16), salt=salt, snakes=snakes, out=buf.act, explored_out=buf.explored)
    torch.cuda.synchronize()
    want_a, want_x, _ = xp.np_explore_actions(cfg, states, policies, eps_q16, salt)
    got, sel = buf.host("act"), list(range(ns)) if snakes is None else sorted(snakes)
    assert np.array_equal(got[:, sel], want_a[:, sel]), (label, "actions", np.argwhere(got[:, sel] != want_a[:, sel])[:4].tolist())
    rest = [c for c in range(got.shape[1]) if c not in sel]
    assert (got[:, rest] == -77).all(), (label, "unselected entries")
    assert np.array_equal(buf.host("explored"), want_x), (label, "explored", np.argwhere(buf.host("explored") != want_x)[:4].tolist())
    assert buf.guards_intact(), label
    return want_x


def played(rules, dim, ns, num_envs, steps, seed=6, **kw):
    """A handle and an oracle `steps` steps into the same safe_greedy play; returns (cfg, env, states)."""
    cfg = sp.scenario(rules, dim, ns, "safe_greedy", steps, num_envs, seed, env_id_base=11, **kw)
    env, ora = gh.make_env(cfg), sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    for _ in range(steps):
        act = np.array([sp.safe_greedy(st, dim, ns, None) for st in gh.oracle_states(ora)], np.int32)
        ora.step(act, want_obs=False)
        env.step_device(torch.from_numpy(act).to(env.device))
    return cfg, env, gh.oracle_states(ora)


# ------------------------------------------------------------------------------------------ msnake_explore_actions
def test_a_wider_stride_and_a_partial_mask_on_6x6():
    sc = pp.scenario("C")
    assert sc["cfg"]["dim"] == 6 and sc["cfg"]["env_id_base"] == 5
    env = handle(sc["cfg"], sc["states"])
    x = check_actions(env, sc["cfg"], sc["states"], ("safe_greedy", "wary_greedy", None), [ONE // 2] * 3, salt=1, snakes=[2, 0], stride=5)
    assert x.any() and not x.all()
    env.close()


MIXES = [(("safe_greedy", "hamiltonian", "wary_greedy"), (0, 16384, ONE)), ((None, "wary_greedy", "safe_greedy"), (ONE, 16384, 0)),
         (("hamiltonian", None, "safe_greedy"), (16384, ONE, ONE)), (("wary_greedy", "safe_greedy", "hamiltonian"), (ONE, 16384, 0)),
         (("wary_greedy", "wary_greedy", None), (16384, 0, 16384))]


def test_mixes_of_all_four_policies_25_steps_into_play():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    for i, (pol, eps) in enumerate(MIXES):
        check_actions(env, sc["cfg"], sc["states"], pol, list(eps), salt=i, label=(pol, eps))
    env.close()


def test_the_compiled_shape_handle():
    sc = pp.scenario("D")
    env = handle(sc["cfg"], sc["states"])
    assert env.kernel_name().endswith(", 19>") and env.num_envs == 33
    check_actions(env, sc["cfg"], sc["states"], ("wary_greedy", "safe_greedy", None), [6554, ONE, ONE // 2], salt=3)
    env.close()


def test_an_adversarial_handle():
    cfg, env, states = played("adversarial", 10, 3, 21, 40)
    assert max(len(st["fruits"]) for st in states) > 3                           # the list has grown past the record's words
    for pol in ("safe_greedy", "wary_greedy", ("wary_greedy", "safe_greedy", None)):
        check_actions(env, cfg, states, pol, [ONE // 2, ONE, 16384], salt=2, label=pol)
    env.close()


def test_a_new_world_handle_of_four_snakes():
    cfg, env, states = played("new_world", 10, 4, 19, 30)
    x = check_actions(env, cfg, states, "safe_greedy", [ONE // 2, ONE, 16384, ONE], salt=4)
    assert x[:, 3].any()
    check_actions(env, cfg, states, ("safe_greedy", "hamiltonian", None, "safe_greedy"), [0, ONE, ONE, 16384], salt=5)
    env.close()


def test_an_env_id_base_past_32_bits():
    sc = pp.scenario("A")
    cfg = dict(sc["cfg"], env_id_base=2 ** 33)
    env = handle(cfg, sc["states"][:9])
    check_actions(env, cfg, sc["states"][:9], "safe_greedy", [ONE // 2] * 3, salt=2 ** 63 + 1)
    low = xp.np_explore_actions(dict(cfg, env_id_base=0), sc["states"][:9], "safe_greedy", [ONE // 2] * 3, 2 ** 63 + 1)
    assert not np.array_equal(low[1], xp.np_explore_actions(cfg, sc["states"][:9], "safe_greedy", [ONE // 2] * 3, 2 ** 63 + 1)[1])
    env.close()


@pytest.mark.parametrize("n", [1, 3, 67, 257])
def test_envs_per_block(n):
    sc = pp.scenario("A")
    states = [sc["states"][e % 67] for e in range(n)]               # env e draws under its own global id
    env = handle(sc["cfg"], states)
    check_actions(env, sc["cfg"], states, ("safe_greedy", "wary_greedy", "hamiltonian"), [ONE // 2] * 3, salt=8, label=n)
    env.close()


def test_with_every_eps_zero_the_actions_are_the_policies_own():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    before, stats = env.hash_states_device("full").clone(), env.stats()
    for pol in ("safe_greedy", "hamiltonian", "wary_greedy"):
        buf = action_buffers(env)
        env.explore_actions_device(pol, 0.0, salt=123, out=buf.act, explored_out=buf.explored)
        own = env.scripted_actions_device(pol, out=torch.full((67, 3), -5, dtype=torch.int32, device=env.device))
        torch.cuda.synchronize()
        assert np.array_equal(buf.host("act"), own.cpu().numpy()), pol
        assert not buf.host("explored").any() and buf.guards_intact(), pol
    buf = action_buffers(env)
    env.explore_actions_device(None, 0.0, out=buf.act, explored_out=buf.explored)
    torch.cuda.synchronize()
    assert not buf.host("act").any() and not buf.host("explored").any()
    # the same call twice: the same bytes; and the handle is only read
    a, b = action_buffers(env), action_buffers(env)
    for buf in (a, b):
        env.explore_actions_device(("safe_greedy", "wary_greedy", None), 0.5, salt=6, out=buf.act, explored_out=buf.explored)
    torch.cuda.synchronize()
    assert np.array_equal(a.host("act"), b.host("act")) and np.array_equal(a.host("explored"), b.host("explored")) and a.host("explored").any()
    assert torch.equal(env.hash_states_device("full"), before) and env.stats() == stats
    env.close()


# ------------------------------------------------------------------------------------------ msnake_playout_explore
def play(env, buf, sc, **kw):
    f = None if sc["first"] is None else torch.from_numpy(np.ascontiguousarray(sc["first"], np.int32)).to(env.device)
    args = dict(first_actions=f, first_snakes=sc["first_snakes"], out=[getattr(buf, n) for n in NAMES], explore=sc["explore"], salt=sc["salt"])
    args.update(kw)
    return env.playout_device(sc["K"], sc["policies"], **args)


def assert_equals_reference(buf, ref, label=""):
    for n in ("steps", "end", "ret", "info", "count"):
        got = buf.host(n)
        assert np.array_equal(got, ref[n]), (label, n, np.argwhere(got != ref[n])[:4].tolist())
    words = buf.host("words")
    for e, want in enumerate(ref["words"]):
        assert np.array_equal(words[e, :len(want)], want), (label, "words", e, np.argwhere(words[e, :len(want)] != want)[:4].tolist())
        assert (words[e, len(want):] == -77).all(), (label, "behind the words", e)
    assert buf.guards_intact(), label


@pytest.mark.parametrize("name", xp.SCENARIOS + ("X_forced",))
def test_the_playout_against_the_reference(name):
    sc, (ref, _) = xp.scenario(name), xp.reference(name)
    env = handle(sc["cfg"], sc["states"])
    if name == "XD":
        assert env.kernel_name().endswith(", 19>")                  # the compiled-shape handle
    before, stats = env.hash_states_device("full").clone(), env.stats()
    buf = playout_buffers(env)
    play(env, buf, sc)
    torch.cuda.synchronize()
    assert_equals_reference(buf, ref, name)
    again = playout_buffers(env)                                    # the same call twice: the same bytes
    play(env, again, sc)
    torch.cuda.synchronize()
    assert all(np.array_equal(buf.host(n), again.host(n)) for n in NAMES), name
    assert torch.equal(env.hash_states_device("full"), before) and env.stats() == stats, (name, "the handle was only to be read")
    env.close()


@pytest.mark.parametrize("name", ["XA", "XB", "XD", "XF"])
def test_with_every_eps_zero_the_playout_is_msnake_playout(name):
    sc = xp.scenario(name)
    env = handle(sc["cfg"], sc["states"])
    plain, zero = playout_buffers(env), playout_buffers(env)
    play(env, plain, sc, explore=None, salt=0)                      # msnake_playout, with the same forced first actions
    play(env, zero, sc, explore=0.0, salt=0xFEEDFACE)
    torch.cuda.synchronize()
    for n in NAMES:
        assert np.array_equal(plain.host(n), zero.host(n)), (name, n)   # the whole buffers, the words not written included
    env.close()


def explore_loop(twin, K, policies, explore, salt):
    """K steps of [explore actions -> step -> outcomes] on `twin` (auto_reset off), every env snapshotted at the step it ends:
    the six outputs as host arrays, the words as a device tensor."""
    n, ns = twin.num_envs, twin.n_snakes
    steps, end = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    ret, info = np.zeros((n, ns), np.float32), np.zeros((n, ns, 4), np.int32)
    words = torch.zeros((n, twin.state_words_max), dtype=torch.int32, device=twin.device)
    count = torch.zeros(n, dtype=torch.int32, device=twin.device)
    acts = torch.zeros((n, ns), dtype=torch.int32, device=twin.device)
    active = np.ones(n, bool)
    twin.arm_agents_device()
    for k in range(1, K + 1):
        twin.explore_actions_device(policies, explore, salt=salt, out=acts)
        if k == 1:
            info[:, :, 3] = acts.cpu().numpy()
        _, _, done, _ = twin.step_device(acts)
        oc = twin.agent_outcomes_device(done)
        rew, ate, flags, d = oc.rew.cpu().numpy(), oc.ate.cpu().numpy(), oc.flags.cpu().numpy(), done.cpu().numpy() != 0
        ret[active] += rew[active]
        info[active, :, 0] += ate[active]
        info[active, :, 1] += (flags[active] & C.AGENT_ALIVE) != 0
        died = active[:, None] & ((flags & C.AGENT_DIED) != 0)
        info[:, :, 2][died] = k
        steps[active] = k
        ended = active & d
        w, c = twin.export_states_device()
        sel = torch.from_numpy(ended | (active & (k == K))).to(twin.device)
        words[sel], count[sel] = w[sel], c[sel]
        end[ended] = np.where((flags[ended, 0] & C.AGENT_ALIVE) != 0, pp.CAP, pp.DEAD)
        active &= ~d
    return dict(steps=steps, end=end, ret=ret, info=info, words=words, count=count)


@pytest.mark.parametrize("name", ["XA", "XB"])
def test_the_playout_plays_the_very_words_of_explore_actions(name):
    sc = xp.scenario(name)
    env = handle(sc["cfg"], sc["states"])
    buf = playout_buffers(env)
    play(env, buf, sc)
    twin = env.clone(auto_reset=False)
    loop = explore_loop(twin, sc["K"], sc["policies"], sc["explore"], sc["salt"])   # t and ctr move under the loop as inside the playout
    for n in ("steps", "end", "ret", "info"):
        assert np.array_equal(buf.host(n), loop[n]), n
    count, words, l_words = buf.host("count"), buf.host("words"), loop["words"].cpu().numpy()
    assert np.array_equal(count, loop["count"].cpu().numpy())
    for e in range(len(count)):
        assert np.array_equal(words[e, :count[e]], l_words[e, :count[e]]), e
    env.close(), twin.close()


def test_graph_of_explore_actions_then_step():
    """[msnake_explore_actions -> msnake_step] captured once and replayed 20 times, with nothing in the arguments changing: every
    replay's actions are the restatement's on the state of that moment (the oracle is stepped with them alongside)."""
    cfg = sp.scenario("snake_env", 10, 3, "safe_greedy", 20, 24, 3, env_id_base=5)
    env, ora = gh.make_env(cfg), sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    pol, eps, salt = ("safe_greedy", "wary_greedy", "hamiltonian"), [ONE // 2, 16384, ONE], 77
    blob = env.get_state_all()
    buf = action_buffers(env)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up on the side stream, as graph capture wants
        env.explore_actions_device(pol, probs(eps), salt=salt, out=buf.act, explored_out=buf.explored)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.explore_actions_device(pol, probs(eps), salt=salt, out=buf.act, explored_out=buf.explored)
        env.step_device(buf.act)
    torch.cuda.synchronize()
    env.set_state_all(blob)                                        # (whether or not the capture ran anything)
    drawn = 0
    for t in range(20):
        want_a, want_x, _ = xp.np_explore_actions(cfg, gh.oracle_states(ora), pol, eps, salt)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.host("act"), want_a) and np.array_equal(buf.host("explored"), want_x), t
        ora.step(want_a, want_obs=False)
        drawn += int(want_x.sum())
    assert drawn > 100 and buf.guards_intact() and env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_explore_actions_in_order_with_nothing_written():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    odd = gh.make_env(dict(sc["cfg"], dim=9, num_envs=4))
    nw = gh.make_env(dict(sc["cfg"], rules=1, num_envs=4))
    buf = action_buffers(env)
    fn, ARG, HANDLE, ALIGN = C.load().msnake_explore_actions, -1, -3, -4
    pol, eps = lambda *ids: (ctypes.c_int32 * 4)(*ids), lambda *q: (ctypes.c_uint32 * 4)(*q)
    good = dict(h=env._h, pol=pol(1, 3, 2, 99), eps=eps(ONE, 0, 16384, 99999), salt=1, mask=0b111, act=buf.act.data_ptr(), stride=3,
                flags=buf.explored.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], a["pol"], a["eps"], a["salt"], a["mask"], a["act"], a["stride"], a["flags"], None)

    bad = buf.act.data_ptr() + 2  # an unaligned address.  Each case also carries reasons that come later in the list: the earlier one must win
    cases = [
        (HANDLE, "handle", dict(h=None, pol=None)),
        (ARG, "policies is NULL", dict(pol=None, eps=None)), (ARG, "policies[1]", dict(pol=pol(1, 4, 1, 0), eps=None)),
        (ARG, "policies[2]", dict(pol=pol(1, 1, -1, 0), h=nw._h)),
        (ARG, "WARY_GREEDY", dict(h=nw._h, pol=pol(1, 3, 2, 0), eps=None)),
        (ARG, "even dim", dict(h=odd._h, pol=pol(1, 2, 1, 0), eps=None)),
        (ARG, "eps_q16 is NULL", dict(eps=None, mask=0)), (ARG, "eps_q16[2]", dict(eps=eps(0, ONE, ONE + 1, 0), mask=0)),
        (ARG, "snake_mask is 0", dict(mask=0, act=None)), (ARG, "snake_mask 0x8", dict(mask=8, act=None)),
        (ARG, "actions_dev is NULL", dict(act=None, stride=2)), (ARG, "action_stride", dict(stride=2, act=bad)),
        (ALIGN, "aligned", dict(act=bad)),
    ]
    for want, msg, kw in cases:
        assert call(**kw) == want and msg in C.load().msnake_last_error().decode(), (want, msg, kw, C.load().msnake_last_error())
    torch.cuda.synchronize()
    assert buf.untouched("act") and buf.untouched("explored")
    assert call() == 0 and call(flags=None) == 0 and call(mask=0b010) == 0   # entries >= S are not looked at
    assert call(h=nw._h, pol=pol(1, 2, 0, 0), act=torch.zeros((4, 3), dtype=torch.int32, device="cuda").data_ptr(), flags=None) == 0
    torch.cuda.synchronize()


def test_every_refusal_of_playout_explore_in_order_with_nothing_written():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    odd = gh.make_env(dict(sc["cfg"], dim=9, num_envs=4))
    adv = gh.make_env(dict(sc["cfg"], rules=2, num_envs=4))
    nw = gh.make_env(dict(sc["cfg"], rules=1, num_envs=4))
    buf = playout_buffers(env)
    first = torch.zeros((67, 3), dtype=torch.int32, device=env.device)
    fn, ARG, HANDLE, ALIGN = C.load().msnake_playout_explore, -1, -3, -4
    pol, eps = lambda *ids: (ctypes.c_int32 * 4)(*ids), lambda *q: (ctypes.c_uint32 * 4)(*q)
    p = {n: getattr(buf, n).data_ptr() for n in NAMES}
    good = dict(h=env._h, pol=pol(1, 1, 1, 99), eps=eps(16384, 0, ONE, 99999), salt=5, n=8, first=None, fstride=0, mask=0, steps=p["steps"],
                end=p["end"], ret=p["ret"], info=p["info"], words=p["words"], wstride=int(buf.words.shape[1]), count=p["count"])

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], a["pol"], a["eps"], a["salt"], a["n"], a["first"], a["fstride"], a["mask"], a["steps"], a["end"], a["ret"],
                  a["info"], a["words"], a["wstride"], a["count"], None)

    bad = 5  # an unaligned address
    cases = [
        (HANDLE, "handle", dict(h=None, n=0)),
        (ARG, "snake_env", dict(h=adv._h, n=0)), (ARG, "snake_env", dict(h=nw._h, n=0)),
        (ARG, "n_steps", dict(n=0, pol=None)), (ARG, "n_steps", dict(n=C.PLAYOUT_MAX_STEPS + 1, pol=None)),
        (ARG, "policies is NULL", dict(pol=None, eps=None)), (ARG, "policies[1]", dict(pol=pol(1, 4, 1, 0), eps=None)),
        (ARG, "eps_q16 is NULL", dict(eps=None, h=odd._h, pol=pol(1, 2, 1, 0))), (ARG, "eps_q16[0]", dict(eps=eps(ONE + 1, 0, 0, 0), h=odd._h, pol=pol(1, 2, 1, 0))),
        (ARG, "even dim", dict(h=odd._h, pol=pol(1, 2, 1, 0), mask=8)),
        (ARG, "first_mask 0x8", dict(mask=8, first=None)), (ARG, "first_dev is NULL", dict(mask=1, first=None, wstride=0)),
        (ARG, "first_stride", dict(mask=1, first=first.data_ptr(), fstride=2, wstride=0)),
        (ARG, "words_stride", dict(wstride=0, steps=None, end=None, ret=None, info=None, count=None)),
        (ARG, "nothing to write", dict(steps=None, end=None, ret=None, info=None, words=None, count=None, mask=1, first=bad, fstride=3)),
        (ALIGN, "aligned", dict(steps=p["steps"] + 2)), (ALIGN, "aligned", dict(ret=p["ret"] + 1)), (ALIGN, "aligned", dict(words=p["words"] + 2)),
        (ALIGN, "aligned", dict(mask=1, first=first.data_ptr() + 2, fstride=3)),
    ]
    for want, msg, kw in cases:
        assert call(**kw) == want and msg in C.load().msnake_last_error().decode(), (want, msg, kw, C.load().msnake_last_error())
        assert "msnake_playout_explore" in C.load().msnake_last_error().decode() or want != ARG
    torch.cuda.synchronize()
    assert all(buf.untouched(n) for n in NAMES)
    assert call() == 0 and call(end=p["end"] + 1) == 0             # entries >= S are not looked at; a byte pointer needs no alignment
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ values, and what the feature is for
def test_playout_values_device_with_explore_equals_its_composition():
    sc = xp.scenario("XA")
    env = handle(sc["cfg"], sc["states"])
    before = env.get_state_all().tobytes()
    reps, snake, K, explore, salt = 3, 0, 12, (0.0, 0.25, 0.25), 21
    scratch = env.clone(num_envs=67 * 4 * reps, auto_reset=False)
    value, survive = env.playout_values_device(scratch, K, snake=snake, reps=reps, explore=explore, salt=salt)
    other = env.clone(num_envs=67 * 4 * reps, auto_reset=False)     # by hand: the forks, one playout, the means
    index = np.repeat(np.arange(67), 4 * reps).astype(np.int32)
    other.copy_envs_device(env, index)
    first = np.zeros((67 * 4 * reps, 3), np.int32)
    first[:, snake] = np.tile(np.repeat(np.arange(1, 5), reps), 67)
    res = other.playout_device(K, "safe_greedy", first_actions=torch.from_numpy(first).to(env.device), first_snakes=[snake],
                               explore=explore, salt=salt)
    ret, death = res.ret.cpu().numpy()[:, snake].reshape(67, 4, reps), res.info.cpu().numpy()[:, snake, 2].reshape(67, 4, reps)
    assert np.array_equal(res.info.cpu().numpy()[:, snake, 3], first[:, snake])      # forced, whatever was drawn
    assert np.allclose(value.cpu().numpy(), ret.mean(axis=2), rtol=0, atol=1e-6)     # sums of small integers over 3: one rounding
    assert np.array_equal(survive.cpu().numpy(), (death == 0).astype(np.float32).reshape(67, 4, reps).mean(axis=2, dtype=np.float32))
    # one slot against the reference: env 2, move 3, rep 1 plays as global env (env_id_base + its slot)
    slot = (2 * 4 + 2) * reps + 1
    ref = xp.np_playout_explore(dict(sc["cfg"], env_id_base=sc["cfg"]["env_id_base"] + slot), [sc["states"][2]], "safe_greedy",
                                xp.q16(list(explore)), salt, K, first=[first[slot]], first_snakes=[snake])
    assert np.array_equal(res.ret.cpu().numpy()[slot], ref["ret"][0]) and np.array_equal(res.info.cpu().numpy()[slot], ref["info"][0])
    assert env.get_state_all().tobytes() == before
    env.close(), scratch.close(), other.close()


def test_on_quiet_states_only_exploring_makes_the_reps_differ():
    """The reason for the feature.  On states from which nobody eats within the horizon, the reps of a move at eps 0 are one
    playout played `reps` times; with explore = 0.5 they are different playouts."""
    sc, reps = xp.scenario("quiet"), 4
    states, first = xp.quiet_forks(reps)
    E, K = len(sc["states"]), sc["K"]
    env = handle(sc["cfg"], sc["states"])
    scratch = env.clone(num_envs=E * 4 * reps, auto_reset=False)
    scratch.copy_envs_device(env, np.repeat(np.arange(E), 4 * reps).astype(np.int32))
    f = torch.from_numpy(first).to(env.device)
    quiet = scratch.playout_device(K, sc["policies"], first_actions=f, first_snakes=[0], end_state=True)
    loud = scratch.playout_device(K, sc["policies"], first_actions=f, first_snakes=[0], end_state=True, explore=sc["explore"], salt=sc["salt"])
    torch.cuda.synchronize()
    want = pp.np_playout(sc["cfg"], states, sc["policies"], K, first, [0])
    want_loud = xp.np_playout_explore(sc["cfg"], states, sc["policies"], sc["eps"], sc["salt"], K, first, [0])
    for got, ref in ((quiet, want), (loud, want_loud)):
        assert np.array_equal(got.ret.cpu().numpy(), ref["ret"]) and np.array_equal(got.info.cpu().numpy(), ref["info"])
        assert np.array_equal(got.count.cpu().numpy(), ref["count"])

    def board(res):   # each slot's end position: the words behind t, ctr, ep_len and ep_return, per (env, move) a row of reps
        w = res.words.cpu().numpy().copy()
        w[:, [0, 1, 2, 4, 5]] = 0
        return w.reshape(E, 4, reps, -1)

    q, l = board(quiet), board(loud)
    assert (q == q[:, :, :1]).all()                                 # today's behaviour: identical in every env and move
    assert (quiet.ret.cpu().numpy().reshape(E, 4, reps, -1).std(axis=2) == 0).all()
    differs = (l != l[:, :, :1]).any(axis=(1, 2, 3))
    assert differs.any(), "with explore = 0.5 the reps of a move differ in at least one env"
    print("envs whose reps differ with explore = 0.5:", int(differs.sum()), "of", E)
    env.close(), scratch.close()
