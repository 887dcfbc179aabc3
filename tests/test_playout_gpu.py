"""msnake_playout on the GPU: all six outputs against the reference np_playout (tests/playout_play.py) for every scenario,
the handle left byte for byte as it was, the call against the library's own step loop, the capacity rule against
msnake_step, NULL and partial outputs, envs per block, graph capture, every refusal, and playout_values_device."""
import ctypes

import numpy as np
import pytest
import torch

import msnake
import gpu_harness as gh
import playout_play as pp
from oracle.snake_oracle import state_to_flat

pytestmark = pytest.mark.gpu
C = msnake._capi
NAMES = ("steps", "end", "ret", "info", "words", "count")


def outputs(env, stride=None):
    n, ns = env.num_envs, env.n_snakes
    return gh.GuardedOutputs(env.device, {
        "steps": dict(dtype="int32", shape=(n,), fill=-77), "end": dict(dtype="uint8", shape=(n,), fill=0xA5),
        "ret": dict(dtype="float32", shape=(n, ns), fill=-77.5), "info": dict(dtype="int32", shape=(n, ns, 4), fill=-77),
        "words": dict(dtype="int32", shape=(n, stride or env.state_words_max), fill=-77),
        "count": dict(dtype="int32", shape=(n,), fill=-77)})


def handle(cfg, states, **kw):
    """A handle holding `states` (dicts, `finished` included), one env each, at cfg's seed and env ids."""
    env = gh.make_env(dict(cfg, num_envs=len(states)), **kw)
    env.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, cfg["n_snakes"]))
    return env


def play(env, buf, K, policies, first=None, first_snakes=None, which=NAMES):
    f = None if first is None else torch.from_numpy(np.ascontiguousarray(first, np.int32)).to(env.device)
    return env.playout_device(K, policies, first_actions=f, first_snakes=first_snakes,
                              out=[getattr(buf, n) if n in which else None for n in NAMES])


def assert_equals_reference(buf, ref, label=""):
    for n in ("steps", "end", "ret", "info", "count"):
        got = buf.host(n)
        assert np.array_equal(got, ref[n]), (label, n, np.argwhere(got != ref[n])[:4].tolist())
    words = buf.host("words")
    for e, want in enumerate(ref["words"]):
        assert np.array_equal(words[e, :len(want)], want), (label, "words", e, np.argwhere(words[e, :len(want)] != want)[:4].tolist())
        assert (words[e, len(want):] == -77).all(), (label, "behind the words", e)
    assert buf.guards_intact(), label


def run_and_compare(cfg, states, policies, K, ref, first=None, first_snakes=None, label="", **kw):
    env = handle(cfg, states, **kw)
    before, stats = env.get_state_all().tobytes(), env.stats()
    buf = outputs(env)
    play(env, buf, K, policies, first, first_snakes)
    torch.cuda.synchronize()
    assert_equals_reference(buf, ref, label)
    assert env.get_state_all().tobytes() == before and env.stats() == stats, (label, "the handle was only to be read")
    env.close()


# ------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("name", pp.SCENARIOS)
def test_against_the_reference(name):
    sc, (ref, _) = pp.scenario(name), pp.reference(name)
    if name == "D":
        assert gh.make_env(dict(sc["cfg"], num_envs=1)).kernel_name().endswith(", 19>")   # the compiled-shape handle
    run_and_compare(sc["cfg"], sc["states"], sc["policies"], sc["K"], ref, sc["first"], sc["first_snakes"], name)


def test_the_edge_cases_through_forced_first_actions():
    for label, cfg, st, actions, _ in pp.edge_cases():
        ref = pp.np_playout(cfg, [st], None, 1, first=[actions])
        run_and_compare(cfg, [st], None, 1, ref, first=[actions], label=label)


def test_forced_first_actions_of_some_snakes_only():
    sc = pp.scenario("A")
    first = np.random.default_rng(5).integers(-1, 7, (67, 4)).astype(np.int32)   # invalid codes included, a wider stride
    ref = pp.np_playout(sc["cfg"], sc["states"], ("safe_greedy", "wary_greedy", None), 12, first, [2, 0])
    assert (ref["info"][:, 0, 3] == first[:, 0]).all() and (ref["info"][:, 2, 3] == first[:, 2]).all()
    run_and_compare(sc["cfg"], sc["states"], ("safe_greedy", "wary_greedy", None), 12, ref, first, [2, 0], auto_reset=False)


@pytest.mark.parametrize("n", [1, 3, 67, 257])
def test_envs_per_block(n):
    sc = pp.scenario("A")
    states = [sc["states"][e % 67] for e in range(n)]           # env e draws from its own stream: the reference plays all n
    ref = pp.np_playout(sc["cfg"], states, "safe_greedy", 20)
    run_and_compare(sc["cfg"], states, "safe_greedy", 20, ref, label=n)


# ------------------------------------------------------------------------------------------ against the library itself
def step_loop(twin, K, policy=None):
    """K steps of [scripted actions -> step -> outcomes] on `twin` (auto_reset off), every env snapshotted at the step it
    ends: the six outputs as host arrays, the words as a device tensor."""
    n, ns = twin.num_envs, twin.n_snakes
    steps, end = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    ret, info = np.zeros((n, ns), np.float32), np.zeros((n, ns, 4), np.int32)
    words = torch.zeros((n, twin.state_words_max), dtype=torch.int32, device=twin.device)
    count = torch.zeros(n, dtype=torch.int32, device=twin.device)
    acts = torch.zeros((n, ns), dtype=torch.int32, device=twin.device)
    active = np.ones(n, bool)
    twin.arm_agents_device()
    for k in range(1, K + 1):
        if policy is not None:
            twin.scripted_actions_device(policy, out=acts)
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


def assert_equals_loop(buf, loop):
    for n in ("steps", "end", "ret", "info"):
        assert np.array_equal(buf.host(n), loop[n]), n
    count, words, l_words = buf.host("count"), buf.host("words"), loop["words"].cpu().numpy()
    assert np.array_equal(count, loop["count"].cpu().numpy())
    for e in range(len(count)):
        assert np.array_equal(words[e, :count[e]], l_words[e, :count[e]]), e


def test_against_the_librarys_own_step_loop():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    buf = outputs(env)
    play(env, buf, sc["K"], "safe_greedy")
    twin = env.clone(auto_reset=False)
    loop = step_loop(twin, sc["K"], "safe_greedy")
    assert_equals_loop(buf, loop)
    # the end words continue the game: imported, they hash as the twin's snapshots do
    a, b = env.clone(auto_reset=False), env.clone(auto_reset=False)
    assert (a.import_states_device(buf.words, count=buf.count) == C.STATE_OK).all()
    assert (b.import_states_device(loop["words"], count=loop["count"]) == C.STATE_OK).all()
    assert torch.equal(a.hash_states_device("full"), b.hash_states_device("full"))
    still = torch.from_numpy(buf.host("end") == pp.HORIZON).to(env.device)
    assert torch.equal(a.hash_states_device("full")[still], twin.hash_states_device("full")[still]) and bool(still.any())


def test_the_capacity_rule_is_the_steps():
    """6x6x1, cap 64: a body of 62 pieces (cells repeat) that keeps growing, two free cells ahead, then its own body.  Step 2
    eats on a full board (no free cell, no draw) and would make 64 pieces: the oldest goes; step 3 runs into piece (5, 0)."""
    cfg = sc_cfg = dict(pp.scenario("C")["cfg"], n_snakes=1, n_fruits=1)
    ring = [(x, y) if y % 2 else (5 - x, y) for y in range(1, 6) for x in range(6)]            # rows 1..5, 30 cells
    body = [(2, 0), (1, 0), (0, 0), (5, 0)] + (ring + ring[::-1])[:57] + [(5, 0)]
    assert len(body) == 62 and (3, 0) not in body and (4, 0) not in body
    st = {"t": 5, "ctr": 9, "spare_fruits": 0, "ep_len": 5, "ep_return": 1.0, "fruits": [[4, 0]], "snakes": [[list(c) for c in body]],
          "vels": [[1, 0]], "grow_to": [1000], "alive": [True], "in_dead": [False]}
    env = handle(sc_cfg, [st] * 3)
    buf = outputs(env)
    play(env, buf, 4, None)
    twin = env.clone(auto_reset=False)
    loop = step_loop(twin, 4)
    assert_equals_loop(buf, loop)
    assert buf.host("steps").tolist() == [3] * 3 and buf.host("end").tolist() == [pp.DEAD] * 3
    assert twin.stats()["errors"] > 0 and env.stats()["errors"] == 0      # the step counts the dropped piece, the playout does not
    assert cfg["dim"] == 6


# ------------------------------------------------------------------------------------------ outputs
def test_null_and_partial_outputs():
    sc, (ref, _) = pp.scenario("A"), pp.reference("A")
    env = handle(sc["cfg"], sc["states"])
    buf = outputs(env)
    for bits in range(1, 64):                                     # every NULL pattern, each output alone among them
        which = [n for i, n in enumerate(NAMES) if bits >> i & 1]
        buf.refill()
        play(env, buf, sc["K"], sc["policies"], which=which)
        torch.cuda.synchronize()
        for n in NAMES:
            if n not in which:
                assert buf.untouched(n), (which, n)
            elif n != "words":
                assert np.array_equal(buf.host(n), ref[n]), (which, n)
        if "words" in which:
            assert all(np.array_equal(buf.host("words")[e, :len(w)], w) for e, w in enumerate(ref["words"])), which
        assert buf.guards_intact()
    # a stride below some envs' counts: their counts are written, none of their words
    stride = int(np.median(ref["count"]))
    short = outputs(env, stride)
    play(env, short, sc["K"], sc["policies"])
    assert np.array_equal(short.host("count"), ref["count"]) and (ref["count"] > stride).any() and (ref["count"] <= stride).any()
    for e, w in enumerate(ref["words"]):
        row = short.host("words")[e]
        assert (row == -77).all() if len(w) > stride else (np.array_equal(row[:len(w)], w) and (row[len(w):] == -77).all()), e
    assert short.guards_intact()


def test_graph_capture_behind_a_step():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"], auto_reset=False)
    buf, acts = outputs(env), torch.zeros((67, 3), dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                  # warm-up on the side stream, as graph capture wants
        play(env, buf, 16, "wary_greedy")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    blob = env.get_state_all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.scripted_actions_device("safe_greedy", out=acts)
        env.step_device(acts)
        play(env, buf, 16, "wary_greedy")
    torch.cuda.synchronize()
    env.set_state_all(blob)                                        # (whether or not the capture ran anything)
    for t in range(3):
        buf.refill()
        g.replay()
        eager = outputs(env)
        play(env.clone(), eager, 16, "wary_greedy")                # the same state, played out by a plain call
        torch.cuda.synchronize()
        for n in NAMES:
            assert np.array_equal(buf.host(n), eager.host(n)), (t, n)
        assert buf.guards_intact()


def test_every_refusal_in_order_with_nothing_written():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    odd = gh.make_env(dict(sc["cfg"], dim=9, num_envs=4))
    adv = gh.make_env(dict(sc["cfg"], rules=2, num_envs=4))
    nw = gh.make_env(dict(sc["cfg"], rules=1, num_envs=4))
    buf = outputs(env)
    first = torch.zeros((67, 3), dtype=torch.int32, device=env.device)
    fn, ARG, HANDLE, ALIGN = C.load().msnake_playout, -1, -3, -4    # MSNAKE_E_ARG, MSNAKE_E_HANDLE, MSNAKE_E_ALIGN
    pol = lambda *ids: (ctypes.c_int32 * 4)(*ids)
    p = {n: getattr(buf, n).data_ptr() for n in NAMES}
    good = dict(h=env._h, pol=pol(1, 1, 1, 99), n=8, first=None, fstride=0, mask=0, steps=p["steps"], end=p["end"], ret=p["ret"],
                info=p["info"], words=p["words"], wstride=int(buf.words.shape[1]), count=p["count"])

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["h"], a["pol"], a["n"], a["first"], a["fstride"], a["mask"], a["steps"], a["end"], a["ret"], a["info"], a["words"],
                  a["wstride"], a["count"], None)

    bad = 5  # an unaligned address.  Each case also carries the reasons that come later in the list: the earlier one must win
    cases = [
        (HANDLE, "handle", dict(h=None, n=0)),
        (ARG, "snake_env", dict(h=adv._h, n=0)), (ARG, "snake_env", dict(h=nw._h, n=0)),
        (ARG, "n_steps", dict(n=0, pol=None)), (ARG, "n_steps", dict(n=C.PLAYOUT_MAX_STEPS + 1, pol=None)),
        (ARG, "policies is NULL", dict(pol=None, mask=8)), (ARG, "policies[1]", dict(pol=pol(1, 4, 1, 0), mask=8)),
        (ARG, "policies[2]", dict(pol=pol(1, 1, -1, 0), mask=8)),
        (ARG, "even dim", dict(h=odd._h, pol=pol(1, 2, 1, 0), mask=8)),
        (ARG, "first_mask 0x8", dict(mask=8, first=None)), (ARG, "first_dev is NULL", dict(mask=1, first=None, wstride=0)),
        (ARG, "first_stride", dict(mask=1, first=first.data_ptr(), fstride=2, wstride=0)),
        (ARG, "words_stride", dict(wstride=0, steps=None, end=None, ret=None, info=None, count=None)),
        (ARG, "words_stride", dict(wstride=-3, steps=bad)),
        (ARG, "nothing to write", dict(steps=None, end=None, ret=None, info=None, words=None, count=None, mask=1, first=bad, fstride=3)),
        (ALIGN, "aligned", dict(steps=p["steps"] + 2)), (ALIGN, "aligned", dict(ret=p["ret"] + 1)), (ALIGN, "aligned", dict(info=p["info"] + 2)),
        (ALIGN, "aligned", dict(words=p["words"] + 2)), (ALIGN, "aligned", dict(count=p["count"] + 3)),
        (ALIGN, "aligned", dict(mask=1, first=first.data_ptr() + 2, fstride=3)),
    ]
    for want, msg, kw in cases:
        assert call(**kw) == want and msg in C.load().msnake_last_error().decode(), (want, msg, kw, C.load().msnake_last_error())
    torch.cuda.synchronize()
    assert all(buf.untouched(n) for n in NAMES)
    assert call(pol=pol(1, 1, 1, 99)) == 0 and call(end=p["end"] + 1) == 0       # entries >= S are not looked at; a byte pointer needs no alignment
    assert call(h=odd._h, pol=pol(1, 3, 0, 2), steps=None, end=None, ret=None, info=None, words=None, wstride=0,
                count=torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr()) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ values
def test_playout_values_device_equals_its_composition():
    sc = pp.scenario("A")
    env = handle(sc["cfg"], sc["states"])
    before = env.get_state_all().tobytes()
    reps, snake, K = 3, 1, 16
    scratch = env.clone(num_envs=67 * 4 * reps, auto_reset=False)
    value, survive = env.playout_values_device(scratch, K, snake=snake, reps=reps, policies="wary_greedy")
    # by hand: the forks, one playout, the means
    other = env.clone(num_envs=67 * 4 * reps, auto_reset=False)
    index = np.repeat(np.arange(67), 4 * reps).astype(np.int32)
    other.copy_envs_device(env, index)
    first = np.zeros((67 * 4 * reps, 3), np.int32)
    first[:, snake] = np.tile(np.repeat(np.arange(1, 5), reps), 67)
    res = other.playout_device(K, "wary_greedy", first_actions=torch.from_numpy(first).to(env.device), first_snakes=[snake])
    ret, death = res.ret.cpu().numpy()[:, snake].reshape(67, 4, reps), res.info.cpu().numpy()[:, snake, 2].reshape(67, 4, reps)
    assert np.array_equal(res.info.cpu().numpy()[:, snake, 3], first[:, snake])
    assert np.allclose(value.cpu().numpy(), ret.mean(axis=2), rtol=0, atol=1e-6)     # sums of small integers over 3: one rounding
    assert np.array_equal(survive.cpu().numpy(), (death == 0).astype(np.float32).reshape(67, 4, reps).mean(axis=2, dtype=np.float32))
    assert (ret.std(axis=2) > 0).any()                                               # the reps draw from their own streams
    # one slot against the reference: env 0, move 2, rep 1 plays as global env (env_id_base + its slot)
    slot = (0 * 4 + 1) * reps + 1
    ref = pp.np_playout(dict(sc["cfg"], env_id_base=sc["cfg"]["env_id_base"] + slot), [sc["states"][0]], "wary_greedy", K,
                        first=[first[slot]], first_snakes=[snake])
    assert np.array_equal(res.ret.cpu().numpy()[slot], ref["ret"][0]) and np.array_equal(res.info.cpu().numpy()[slot], ref["info"][0])
    assert env.get_state_all().tobytes() == before
