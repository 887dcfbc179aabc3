"""Per-snake outcomes on the device (msnake_agent_outcomes) against tests/agents_play.py on an oracle twin.

Every expectation comes from agents_play.Twin: an Oracle(auto_reset=False) that is given the same seed and the same
actions, whose states before and after each step go through agents_play.np_outcomes.  Nothing is ever read back from the
library's own get_state to form an expectation.  All comparisons are bit-exact: rew (as bits), ate, flags, info and
every word of the tracker after every call.  The tracker and every output sit between guard elements in buffers
pre-filled with values no outcome can be; the int32 / float32 buffers start 12 bytes behind a 16-byte boundary, the
alignment the header promises to accept.
"""
import ctypes

import numpy as np
import pytest

import agents_play as ap
import gpu_harness as gh
import scripted_play as sp

pytestmark = pytest.mark.gpu

GW = 3            # guard elements in front of and behind an int32 / float32 buffer: 12 bytes, so the data is 4-byte aligned only
GB = 64           # guard bytes around a uint8 buffer
IFILL, FFILL, BFILL = -7777, -77.5, 0xA5
OUTPUTS = ("rew", "ate", "flags", "info")
_mk = gh.make_env


def _env(cfg, **kw):
    return _mk(cfg, **dict(dict(auto_reset=False), **kw))


def Bufs(env):
    """The tracker and the four outputs of one handle, each between guards."""
    n, S = env.num_envs, env.n_snakes
    word = dict(guard=GW, align=16)
    b = gh.GuardedOutputs(env.device, dict(track=dict(word, dtype="int32", shape=(n, S, 8), fill=IFILL),
                                           rew=dict(word, dtype="float32", shape=(n, S), fill=FFILL),
                                           ate=dict(dtype="uint8", shape=(n, S), fill=BFILL, guard=GB, align=4),
                                           flags=dict(dtype="uint8", shape=(n, S), fill=BFILL, guard=GB, align=4),
                                           info=dict(word, dtype="int32", shape=(n, S, 4), fill=IFILL)))
    assert all(_ptr(b, k) % 16 == 12 for k in ("track", "rew", "info")) and _ptr(b, "ate") % 4 == 0 and _ptr(b, "flags") % 4 == 0
    return b


def _ptr(b, k):
    return getattr(b, k).data_ptr()


def _raw(env, flags, track, done=None, rew=None, ate=None, flg=None, info=None):
    """msnake_agent_outcomes itself, on the current stream; arguments are addresses (or None).  Returns the code."""
    import torch
    return env._L.msnake_agent_outcomes(env._h, flags, track, done, rew, ate, flg, info,
                                        ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream))


def _arm(env, b):
    assert _raw(env, 1, _ptr(b, "track")) == 0


def _outcomes(env, b, done, which=OUTPUTS):
    key = dict(rew="rew", ate="ate", flg="flags", info="info")
    assert _raw(env, 0, _ptr(b, "track"), done.data_ptr(), **{a: (_ptr(b, k) if k in which else None) for a, k in key.items()}) == 0


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), np.asarray(want, np.float32).view(np.int32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _check_outputs(b, tw, what, which=OUTPUTS):
    for k in OUTPUTS:
        if k in which:
            _same(b.host(k), getattr(tw, k), (what, k))
        else:
            assert b.untouched(k), (what, k, "was written")
    _same(b.host("track"), tw.track, (what, "track"))
    assert b.guards_intact(), what


def _loop(cfg, steps, env=None, which=OUTPUTS, obs_every=20, tw=None, b=None, close=True):
    """[step -> outcomes -> reset_envs(done)] on the device next to the twin; every output and the tracker after every
    call, the step's own outputs too, the observation every `obs_every` steps.  Returns the event counts."""
    import torch
    env = env or _env(cfg)
    fresh = tw is None
    tw = tw or ap.Twin(cfg)
    b = b or Bufs(env)
    if fresh:
        _same(env.reset(), tw.obs, "reset obs")
        _arm(env, b)
        _same(b.host("track"), tw.track, "armed track")
    ev = dict(done=0, died_other=0, ate_other=0, ended_alive=0)
    for t in range(steps):
        act = tw.step()
        obs, rew, done, info = env.step_device(torch.from_numpy(act).to(env.device))
        b.refill(OUTPUTS)
        _outcomes(env, b, done, which)
        env.reset_device(mask=done)
        _same(done.cpu().numpy(), tw.done, (t, "done"))
        _same(rew.cpu().numpy(), tw.step_rew, (t, "step rew"))
        _check_outputs(b, tw, t, which)
        if "rew" in which:
            _same(b.host("rew")[:, 0], rew.cpu().numpy(), (t, "column 0 is the step's reward"))
        if t % obs_every == 0 or t == steps - 1:
            _same(obs.cpu().numpy(), tw.obs, (t, "obs"))
        died = (tw.flags & ap.DIED) != 0
        ev["done"] += int(tw.done.sum())
        ev["died_other"] += int(died[:, 1:].sum())
        ev["ate_other"] += int((tw.ate_raw[:, 1:] > 0).sum())
        ev["ended_alive"] += int((((tw.flags & ap.ENDED) != 0) & ~died)[:, 1:].sum())
    assert env.stats()["errors"] == 0
    if close:
        env.close()
    return ev


# ------------------------------------------------------------------------------------------ 1. closed loops
@pytest.mark.parametrize("name", ["S6", "A6", "N6", "S6cap"])
def test_closed_loop_against_the_oracle_twin(name):
    """The host scenarios at 8 envs x 200 steps, all three rule sets, and the max_steps-12 play whose episodes end at the
    cap while other snakes live."""
    cfg = dict(ap.SCENARIOS[name], steps=200)
    ev = _loop(cfg, 200)
    assert ev["done"] >= 10 and ev["ate_other"] >= 20 and ev["ended_alive"] >= 10, ev
    if cfg["n_snakes"] > 1:
        assert ev["died_other"] >= 10, ev


# ------------------------------------------------------------------------------------------ 2. layout
@pytest.mark.parametrize("rules,ns,nf", [("snake_env", 1, None), ("snake_env", 2, None), ("adversarial", 3, None),
                                         ("new_world", 1, 2), ("new_world", 4, 9)])
def test_every_snake_count_fills_its_group_of_four_lanes(rules, ns, nf):
    cfg = ap.scenario(rules, ns, 3, n_fruits=nf, max_steps=15, num_envs=21, steps=40)
    _loop(cfg, 40)


@pytest.mark.parametrize("num_envs", [1, 3, 15, 16, 17, 37, 257])
def test_wave_and_batch_tails(num_envs):
    """16 envs fill a wave, 64 a workgroup: one short of, exactly, and one past a wave, odd counts, several workgroups."""
    cfg = ap.scenario("snake_env", 3, 4, max_steps=15, num_envs=num_envs, steps=25)
    _loop(cfg, 25)


@pytest.mark.parametrize("record_policy", ["full", "short"])
@pytest.mark.parametrize("envs_per_block", [1, 4, 8])
def test_record_policies_and_envs_per_block(record_policy, envs_per_block):
    cfg = ap.scenario("adversarial", 3, 5, max_steps=15, num_envs=37, steps=20)
    _loop(cfg, 20, env=_env(cfg, record_policy=record_policy, envs_per_block=envs_per_block))


def test_arm_after_a_persistent_rollout_tape():
    """msnake_rollout_tape keeps the envs in registers for the whole tape; ARM behind it reads what it left in memory.
    Then the finished envs are reset, the tracker armed again, and the loop goes on from there."""
    import torch
    cfg = ap.scenario("snake_env", 3, 6, max_steps=30, num_envs=19, steps=8)
    env, tw, T = _env(cfg), ap.Twin(cfg), 8
    env.reset()
    rs = np.random.default_rng(2)
    tape = rs.integers(0, 5, (T, 19, 3)).astype(np.int32)
    _, rew, done, _ = env.rollout_device(torch.from_numpy(tape).to(env.device), persistent=True, keep_obs=False)
    for t in range(T):   # the twin's oracle without its masked resets: a finished env is stepped on, as on the device
        _, o_rew, o_done, _, _, _ = tw.ora.step(tape[t])
        _same(rew[t].cpu().numpy(), o_rew, (t, "tape rew"))
        _same(done[t].cpu().numpy(), o_done, (t, "tape done"))
    tw.states = [tw.read(e) for e in range(tw.E)]
    b = Bufs(env)
    _arm(env, b)
    _same(b.host("track"), tw.track, "armed behind the tape")
    fin = np.array([tw.ora.finished(e) for e in range(tw.E)], np.uint8)
    assert fin.any() and not fin.all()
    tw.ora.reset_envs(fin, final_obs=None, truncated=None)
    env.reset_device(mask=torch.from_numpy(fin).to(env.device))
    tw.states = [tw.read(e) for e in range(tw.E)]
    _arm(env, b)
    _same(b.host("track"), tw.track, "armed behind the masked reset")
    assert b.guards_intact()
    _loop(cfg, 15, env=env, tw=tw, b=b)


# ------------------------------------------------------------------------------------------ 3. semantics
def test_arm_writes_the_facts_and_zero_totals_whatever_the_tracker_held():
    cfg = ap.scenario("new_world", 4, 7, n_fruits=9, max_steps=20, num_envs=12, steps=30)
    env, tw = _env(cfg), ap.Twin(cfg)
    b = Bufs(env)
    _same(env.reset(), tw.obs, "reset obs")
    _arm(env, b)
    _loop(cfg, 30, env=env, tw=tw, b=b, close=False)   # (totals are running now)
    assert (b.host("track")[:, :, 2:7] != 0).any()
    _arm(env, b)
    want = np.stack([ap.track_rows(st, cfg["rules"], ap.zero_totals(4)) for st in tw.states])
    _same(b.host("track"), want, "re-armed")
    assert (want[:, :, ap.TR_ALIVE] == 0).any(), "some new_world snake is not alive: the alive bit is what is read"
    assert b.guards_intact()
    env.close()


def test_done_rows_equal_an_armed_tracker_after_reset_envs():
    """A done env's rows are set up for the reset without looking at it: after reset_envs(done) they equal what ARM
    writes, word for word."""
    import torch
    cfg = ap.scenario("adversarial", 3, 8, max_steps=10, num_envs=16, steps=30)
    env, tw = _env(cfg), ap.Twin(cfg)
    b, b2 = Bufs(env), Bufs(env)
    env.reset()
    _arm(env, b)
    seen = 0
    for t in range(30):
        act = tw.step()
        _, _, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _outcomes(env, b, done)
        env.reset_device(mask=done)
        _arm(env, b2)
        d = tw.done != 0
        got, armed = b.host("track"), b2.host("track")
        _same(got[d], armed[d], (t, "done rows"))
        _same(got[d][:, :, :2], np.broadcast_to([3, 1], got[d][:, :, :2].shape), (t, "grow_to 3, alive"))
        _same(got[~d][:, :, :2], armed[~d][:, :, :2], (t, "facts of the others"))
        seen += int(d.sum())
    assert seen >= 8
    env.close()


def test_each_output_alone_gives_the_bytes_of_all_together():
    import torch
    cfg = ap.scenario("snake_env", 3, 9, max_steps=15, num_envs=23, steps=12)
    envs = [_env(cfg) for _ in range(5)]
    bufs = [Bufs(e) for e in envs]
    tw = ap.Twin(cfg)
    for e, b in zip(envs, bufs):
        e.reset()
        _arm(e, b)
    for t in range(12):
        act = tw.step()
        for e, b, which in zip(envs, bufs, [OUTPUTS] + [(k,) for k in OUTPUTS]):
            _, _, done, _ = e.step_device(torch.from_numpy(act).to(e.device))
            b.refill(OUTPUTS)
            _outcomes(e, b, done, which)
            e.reset_device(mask=done)
            _check_outputs(b, tw, (t, which), which)
    for e in envs:
        e.close()


def test_ate_clamps_at_255_and_rew_does_not():
    """Adversarial 10x10x3, the smallest board whose fruit list (fcap 320) holds more than 255 entries: 300 entries lie on
    the cell snake 1 moves onto, 2 on the cell snake 0 moves onto; spare_fruits keeps the step from respawning any."""
    import torch
    from oracle.snake_oracle import state_to_flat
    cfg = ap.scenario("adversarial", 3, 1, dim=10, max_steps=50, num_envs=2, steps=1, eps=0.0)
    st = {"t": 4, "ctr": 64, "spare_fruits": 1000, "ep_len": 4, "ep_return": 0.0,
          "fruits": [[3, 2]] * 2 + [[6, 7]] * 300 + [[9, 9]],
          "snakes": [[[2, 2]], [[5, 7], [4, 7]], [[0, 9]]], "vels": [[1, 0], [1, 0], [0, 0]], "grow_to": [3, 3, 3],
          "alive": [True] * 3, "in_dead": [False] * 3}
    env, tw = _env(cfg), ap.Twin(cfg)
    b = Bufs(env)
    env.reset()
    words = state_to_flat(st, 3)
    tw.ora.set_state(1, st)
    env._L.msnake_set_state(env._h, 1, words.ctypes.data, len(words))   # (the bare call: the arming below is the test's own)
    tw.states[1] = tw.read(1)
    _arm(env, b)
    _same(b.host("track"), tw.track, "armed")
    act = tw.step(np.array([[0, 0, 0], [1, 1, 0]], np.int32))
    _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
    _outcomes(env, b, done)
    _same(rew.cpu().numpy(), tw.step_rew, "step rew")
    assert tw.ate_raw[1].tolist() == [2, 300, 0] and tw.rew[1].tolist() == [2.0, 300.0, 0.0] and tw.ate[1].tolist() == [2, 255, 0]
    assert tw.info[1, 1, 0] == 300 and tw.track[1, 1, ap.GROW_TO] == 603
    _check_outputs(b, tw, "clamp")
    env.close()


def test_wrapper_rearms_a_stale_tracker():
    """copy_envs_device, set_state_words, set_state_all, reset_device() and rollout_device() leave the env's tracker stale;
    the next agent_outcomes_device() arms it first, so it reports a quiet step (nothing eaten, nobody died) from the
    state it finds, and the tracker holds that state's facts."""
    import torch
    from oracle.snake_oracle import state_to_flat
    cfg = ap.scenario("snake_env", 3, 11, max_steps=40, num_envs=9, steps=10)
    env, src, tw = _env(cfg), _env(dict(cfg, seed=12)), ap.Twin(dict(cfg, seed=12))
    env.reset(), src.reset()
    zero_done = torch.zeros(9, dtype=torch.uint8, device=env.device)
    for _ in range(6):   # src and the twin move on; env stays at its reset
        src.step_device(torch.from_numpy(tw.step()).to(env.device))
        src.reset_device(mask=src._done)
    assert env._track_stale
    env.agent_outcomes_device(zero_done)
    assert not env._track_stale

    def quiet(what):
        facts = np.stack([ap.track_rows(st, cfg["rules"], ap.zero_totals(3)) for st in tw.states])
        assert env._track_stale, what
        out = env.agent_outcomes_device(zero_done)
        assert not env._track_stale
        alive = facts[:, :, ap.TR_ALIVE]
        _same(out.flags.cpu().numpy(), (alive * (ap.ALIVE | ap.WAS_ALIVE)).astype(np.uint8), (what, "flags"))
        _same(out.ate.cpu().numpy(), np.zeros((9, 3), np.uint8), (what, "ate"))
        _same(out.rew.cpu().numpy(), np.zeros((9, 3), np.float32), (what, "rew"))
        want = facts.copy()
        want[:, :, ap.EP_ALIVE_STEPS], want[:, :, ap.EP_STEPS] = alive, 1
        _same(env.agent_tracker.cpu().numpy(), want, (what, "track"))

    env.copy_envs_device(src)
    quiet("copy_envs_device")
    st = tw.states[4]
    env.set_state_words(2, state_to_flat(st, 3))
    states = list(tw.states)
    tw.states = states[:2] + [st] + states[3:]
    quiet("set_state_words")
    env.set_state_all(src.get_state_all())
    tw.states = states
    quiet("set_state_all")
    env.arm_agents_device()
    assert not env._track_stale
    env.reset_device()
    assert env._track_stale
    env.close(), src.close()


# ------------------------------------------------------------------------------------------ 4. read-only
def test_the_call_only_reads_the_state():
    import torch
    cfg = ap.scenario("adversarial", 3, 13, max_steps=20, num_envs=33, steps=10)
    env, tw = _env(cfg), ap.Twin(cfg)
    b = Bufs(env)
    env.reset()
    for _ in range(10):
        env.step_device(torch.from_numpy(tw.step()).to(env.device))
        env.reset_device(mask=env._done)
    blob, stats = env.get_state_all().copy(), env.stats()
    _arm(env, b)
    assert np.array_equal(env.get_state_all(), blob), "ARM changed the state (the Philox counters are words 1 and 2 of every env)"
    act = torch.from_numpy(tw.step()).to(env.device)
    _, _, done, _ = env.step_device(act)
    blob, stats = env.get_state_all().copy(), env.stats()
    for _ in range(3):
        _outcomes(env, b, done)
    assert np.array_equal(env.get_state_all(), blob), "outcomes changed the state"
    assert env.stats() == stats, "env_steps or a total moved"
    env.close()


# ------------------------------------------------------------------------------------------ 5. HIP graph
def test_graph_of_step_outcomes_reset_envs_replayed_50_times():
    import torch
    K = 50
    cfg = ap.scenario("snake_env", 3, 14, max_steps=15, num_envs=40, steps=K)
    env, tw = _env(cfg), ap.Twin(cfg)
    b = Bufs(env)
    _same(env.reset(), tw.obs, "reset obs")
    blob = env.get_state_all()
    acts = torch.zeros((40, 3), dtype=torch.int32, device=env.device)

    def chain():
        _, _, done, _ = env.step_device(acts)
        _outcomes(env, b, done)
        env.reset_device(mask=done)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        _arm(env, b)
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    _arm(env, b)
    dones = 0
    for t in range(K):
        acts.copy_(torch.from_numpy(tw.step()))
        b.refill(OUTPUTS)
        g.replay()
        _same(env._done.cpu().numpy(), tw.done, (t, "done"))
        _same(env._rew.cpu().numpy(), tw.step_rew, (t, "step rew"))
        _check_outputs(b, tw, t)
        dones += int(tw.done.sum())
    _same(env._obs.cpu().numpy(), tw.obs, "obs behind the last replay")
    assert dones >= 20
    env.close()


# ------------------------------------------------------------------------------------------ 6. the wrapper's fused step
def test_step_agents_device_equals_an_auto_reset_env():
    """obs, rew, done and info of step_agents_device() are what Oracle(auto_reset=True) returns, bit for bit, over 100 steps
    at 6x6x3; the agents' tensors are the twin's."""
    import torch
    cfg = dict(ap.SCENARIOS["S6"], steps=100)
    env, tw, ora = _env(cfg), ap.Twin(cfg), sp.make_oracle(cfg, auto_reset=True)
    _same(env.reset(), ora.reset(), "reset obs")
    dones = 0
    for t in range(100):
        act = tw.step()
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(act)
        obs, rew, done, info, agents = env.step_agents_device(torch.from_numpy(act).to(env.device))
        _same(obs.cpu().numpy(), o_obs, (t, "obs"))
        _same(rew.cpu().numpy(), o_rew, (t, "rew"))
        _same(done.cpu().numpy(), o_done, (t, "done"))
        info = info.cpu().numpy()
        _same(info[:, 0].copy().view(np.float32), o_er, (t, "ep_return"))
        _same(info[:, 1], o_el, (t, "ep_len"))
        _same(info[:, 2], o_ns, (t, "num_snakes"))
        _same(info[:, 3] & 1, o_done, (t, "info done bit"))
        for k in OUTPUTS:
            _same(getattr(agents, k).cpu().numpy(), getattr(tw, k), (t, k))
        _same(env.agent_tracker.cpu().numpy(), tw.track, (t, "track"))
        dones += int(o_done.sum())
    assert dones >= 10
    env.close()
    auto = _mk(cfg)
    with pytest.raises(ValueError, match="auto_reset=False"):
        auto.step_agents_device(torch.zeros((8, 3), dtype=torch.int32, device=auto.device))
    auto.close()


# ------------------------------------------------------------------------------------------ 7. refusals
def test_every_refusal():
    import msnake
    import torch
    E = dict(ARG=-1, HANDLE=-3, ALIGN=-4)
    cfg = ap.scenario("snake_env", 3, 15, num_envs=5)
    env = _env(cfg)
    b = Bufs(env)
    env.reset()
    done = torch.zeros(5, dtype=torch.uint8, device=env.device)
    T, D, R, A, F, I = _ptr(b, "track"), done.data_ptr(), _ptr(b, "rew"), _ptr(b, "ate"), _ptr(b, "flags"), _ptr(b, "info")
    last = lambda: env._L.msnake_last_error().decode()
    for flags in (2, 3, 4, -1, 1 << 31 - 1):
        assert _raw(env, flags, T, D, R) == E["ARG"] and "flags" in last(), flags
    assert _raw(env, 0, None, D, R) == E["ARG"] and "track_dev" in last()
    assert _raw(env, 1, None) == E["ARG"]
    for extra in (dict(done=D), dict(rew=R), dict(ate=A), dict(flg=F), dict(info=I)):   # ARM with done_dev or any output
        assert _raw(env, 1, T, **extra) == E["ARG"] and "arming" in last(), extra
    assert _raw(env, 0, T, None, R, A, F, I) == E["ARG"] and "done_dev" in last()
    assert _raw(env, 0, T, D) == E["ARG"] and "nothing to write" in last()
    assert _raw(env, 0, T + 1, D, R) == E["ALIGN"] and _raw(env, 1, T + 2) == E["ALIGN"]
    assert _raw(env, 0, T, D, R + 2, A, F, I) == E["ALIGN"]
    assert _raw(env, 0, T, D, R, A, F, I + 1) == E["ALIGN"]
    L = env._L
    assert L.msnake_agent_outcomes(None, 0, T, D, R, None, None, None, None) == E["HANDLE"]
    assert L.msnake_agent_outcomes(None, 1, T, None, None, None, None, None, None) == E["HANDLE"]
    auto = _mk(cfg)   # auto_reset = 1: refused for outcomes and for arming, whatever else is right
    auto.reset()
    assert _raw(auto, 0, T, D, R, A, F, I) == E["ARG"] and "auto_reset" in last()
    assert _raw(auto, 1, T) == E["ARG"] and "auto_reset" in last()
    with pytest.raises(RuntimeError, match="auto_reset"):
        auto.arm_agents_device()
    torch.cuda.synchronize()
    # nothing was written by a refused call
    assert all(b.untouched(k) for k in ("track",) + OUTPUTS)
    _arm(env, b)
    assert _raw(env, 0, T, D, None, A + 1, F + 3) == 0, "the byte outputs need no alignment"
    torch.cuda.synchronize()
    assert b.untouched("rew") and b.untouched("info") and (torch.as_strided(b.ate, (15,), (1,), b.ate.storage_offset() + 1) == 0).all()
    # the wrapper's own checks
    with pytest.raises(ValueError, match="rew_out"):
        env.agent_outcomes_device(done, rew_out=torch.zeros((5, 3), dtype=torch.float64, device=env.device))
    with pytest.raises(ValueError, match="info_out"):
        env.agent_outcomes_device(done, info_out=torch.zeros((5, 3, 3), dtype=torch.int32, device=env.device))
    with pytest.raises(ValueError, match="mask"):
        env.agent_outcomes_device(torch.zeros(4, dtype=torch.uint8, device=env.device))
    assert msnake._capi.AGENT_ARM == 1 and (msnake._capi.AGENT_ALIVE, msnake._capi.AGENT_WAS_ALIVE, msnake._capi.AGENT_DIED,
                                            msnake._capi.AGENT_ENDED) == (ap.ALIVE, ap.WAS_ALIVE, ap.DIED, ap.ENDED)
    env.close(), auto.close()


# ------------------------------------------------------------------------------------------ 8. training on every snake
def test_runner_batch_is_the_valid_samples_and_learn_runs():
    import torch
    from msnake import selfplay
    cfg = ap.scenario("snake_env", 3, 16, max_steps=60, num_envs=16)
    env = _env(cfg)
    torch.manual_seed(0)
    model = selfplay.RayPolicy().to(env.device)
    runner = selfplay.Runner(env, model, [], 8, 0.99, 0.95, rays=True, all_snakes=True)
    obs, returns, ended, actions, values, nlps, epinfos = runner.run()
    flags = runner.last_flags.cpu().numpy()
    n_valid = int(((flags & ap.WAS_ALIVE) != 0).sum())
    assert flags.shape == (8, 16, 3) and 16 * 8 < n_valid <= 16 * 8 * 3
    assert obs.shape == (n_valid, 8, 4) and all(x.shape == (n_valid,) for x in (returns, ended, actions, values, nlps))
    assert torch.isfinite(returns).all()
    _same(ended.cpu().numpy() != 0, ((flags & ap.ENDED) != 0)[(flags & ap.WAS_ALIVE) != 0], "ENDED of the valid samples")
    env.close()
    env = _env(cfg)
    model, history = selfplay.learn(env, nsteps=8, total_timesteps=2 * 16 * 8, nminibatches=4, noptepochs=2, rays=True,
                                    all_snakes=True, log_fn=None)
    assert len(history) == 2
    for kvs in history:
        assert 16 * 8 < kvs["agent_samples"] <= 16 * 8 * 3
        assert all(np.isfinite(kvs[k]) for k in ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac"))
    assert all(torch.isfinite(p).all() for p in model.parameters())
    env.close()
