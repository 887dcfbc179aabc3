"""Why a snake died, on the device (msnake_death_causes) against tests/causes_play.py on an oracle twin.

Every expectation comes from causes_play.Twin: an Oracle(auto_reset=False) that is given the same seed and the same
actions, whose states before and after each step go through causes_play.np_causes.  Nothing is ever read back from the
library's own get_state to form an expectation.  All comparisons are byte for byte.  Every output sits between guard
bytes in a buffer pre-filled with a value no output can take (with three snakes bit 7 of cause / by / victims is never
set, and no coordinate is 90).
"""
import ctypes

import numpy as np
import pytest

import agents_play as ap
import causes_play as cp
import gpu_harness as gh
import scripted_play as sp

pytestmark = pytest.mark.gpu

BFILL, WFILL = 0xA5, 90
OUTPUTS = ("cause", "by", "victims", "where")
FLOORS = dict(wall=50, self=15, head_on=100, body=30, dead_owner=4, last_piece=5)   # of tests/test_causes_host.py
E_ARG, E_HANDLE = -1, -3


def _env(cfg, **kw):
    return gh.make_env(cfg, **dict(dict(auto_reset=False), **kw))


def Bufs(env, offset=0):
    n, S = env.num_envs, env.n_snakes
    byte = dict(dtype="uint8", shape=(n, S), fill=BFILL, offset=offset, align=4)
    return gh.GuardedOutputs(env.device, dict(cause=dict(byte), by=dict(byte), victims=dict(byte),
                                              where=dict(dtype="int8", shape=(n, S, 2), fill=WFILL, offset=offset, align=4)))


def _ptr(b, k):
    return getattr(b, k).data_ptr()


def _stream(env):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(env.device).cuda_stream)


def _raw(after, before, cause=None, by=None, victims=None, where=None):
    """msnake_death_causes itself, on the current stream; handles are envs (or None), outputs addresses (or None)."""
    L = (after or before)._L
    return L.msnake_death_causes(after._h if after else None, before._h if before else None, cause, by, victims, where,
                                 _stream(after or before))


def _causes(env, snap, b, which=OUTPUTS):
    assert _raw(env, snap, **{k: (_ptr(b, k) if k in which else None) for k in OUTPUTS}) == 0, env._L.msnake_last_error()


def _snapshot(snap, env):
    assert env._L.msnake_copy_envs(snap._h, env._h, None, _stream(env)) == 0, env._L.msnake_last_error()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want) if got.shape == want.shape else np.array([[-1]])
    assert bad.size == 0, (what, got.shape, want.shape, bad[:5].tolist())


def _check_outputs(b, tw, what, which=OUTPUTS):
    for k in OUTPUTS:
        if k in which:
            _same(b.host(k), getattr(tw, k), (what, k))
        else:
            assert b.untouched(k), (what, k, "was written")
    assert b.guards_intact(), what


def _chain(env, snap, b, act, which=OUTPUTS):
    """copy_envs -> step -> outcomes -> causes -> reset_envs(done) on the current stream.  Returns done and the
    outcomes' flags (tensors of the env's own)."""
    if env._track_stale:   # (before the step: the tracker holds the state the step starts from)
        env.arm_agents_device()
    _snapshot(snap, env)
    _, _, done, _ = env.step_device(act)
    agents = env.agent_outcomes_device(done)
    _causes(env, snap, b, which)
    env.reset_device(mask=done)
    return done, agents.flags


def _loop(cfg, steps, env=None, snap=None, which=OUTPUTS, tw=None, close=True):
    """The chain next to the twin; all outputs after every step, cause != 0 against the device's own DIED flags.
    Returns the event counts."""
    import torch
    env = env or _env(cfg)
    snap = snap or _env(cfg)
    fresh = tw is None
    tw = tw or cp.Twin(cfg)
    b = Bufs(env)
    if fresh:
        _same(env.reset(), tw.obs, "reset obs")
    ev = {}
    for t in range(steps):
        act = tw.step()
        b.refill()
        done, flags = _chain(env, snap, b, torch.from_numpy(act).to(env.device), which)
        _same(done.cpu().numpy(), tw.done, (t, "done"))
        _check_outputs(b, tw, t, which)
        flags = flags.cpu().numpy()
        _same(flags, tw.flags, (t, "flags"))
        if "cause" in which:
            _same(b.host("cause") != 0, (flags & ap.DIED) != 0, (t, "cause != 0 is the device's DIED"))
        cp.add_events(ev, tw.events())
    assert env.stats()["errors"] == 0 and snap.stats()["errors"] == 0
    if close:
        env.close(), snap.close()
    return ev


# ------------------------------------------------------------------------------------------ 1. closed loops
@pytest.mark.parametrize("name", ["S6", "A6", "S6cap"])
def test_closed_loop_against_the_oracle_twin(name):
    cfg = dict(ap.SCENARIOS[name], steps=200)
    ev = _loop(cfg, 200)
    assert all(ev[k] >= v for k, v in FLOORS.items()), ev


# ------------------------------------------------------------------------------------------ 2. / 3. layout
@pytest.mark.parametrize("num_envs", [1, 3, 4, 5, 37, 257])
def test_batch_and_workgroup_tails(num_envs):
    """Four envs fill a workgroup: one short of, exactly, and one past it, odd counts, many workgroups."""
    cfg = ap.scenario("snake_env", 3, 4, max_steps=15, num_envs=num_envs, steps=25)
    _loop(cfg, 25)


@pytest.mark.parametrize("after_kw,before_kw", [
    (dict(record_policy="full", envs_per_block=1), dict(record_policy="short", envs_per_block=8)),
    (dict(record_policy="short", envs_per_block=4), dict(record_policy="full", envs_per_block=1)),
    (dict(record_policy="short", envs_per_block=8), dict(record_policy="short", envs_per_block=4)),
    (dict(record_policy="full", envs_per_block=4), dict(record_policy="full", envs_per_block=8, auto_reset=True)),
])
def test_two_layouts(after_kw, before_kw):
    cfg = ap.scenario("adversarial", 3, 5, max_steps=15, num_envs=37, steps=20)
    _loop(cfg, 20, env=_env(cfg, **after_kw), snap=_env(cfg, **before_kw))


# ------------------------------------------------------------------------------------------ 4. the hand-built table
@pytest.mark.parametrize("rules,names", [("snake_env", None), ("adversarial", cp.TABLE_ADVERSARIAL)])
def test_hand_built_table(rules, names):
    import torch
    names = list(cp.TABLE) if names is None else list(names)
    cfg = cp.table_cfg(rules, len(names))
    env = gh.install(cfg, [cp.TABLE[n][0] for n in names], auto_reset=False)
    snap, b = env.clone(), Bufs(env)
    _, prev, now = cp.step_table(rules, names)
    act = torch.tensor([cp.TABLE[n][1] for n in names], dtype=torch.int32, device=env.device)
    _chain(env, snap, b, act)
    for e, n in enumerate(names):
        _, _, cause, by, victims, where = cp.TABLE[n]
        _same(b.host("cause")[e], cause, (n, "cause"))
        _same(b.host("by")[e], by, (n, "by"))
        _same(b.host("victims")[e], victims, (n, "victims"))
        _same(b.host("where")[e], where, (n, "where"))
        want = cp.np_causes(prev[e], now[e], 6)
        for k, w in zip(OUTPUTS, want):
            _same(b.host(k)[e], w, (n, k, "np_causes on the oracle's states"))
    assert b.guards_intact()
    env.close(), snap.close()


# ------------------------------------------------------------------------------------------ 5. long bodies
def long_cycle():
    """A closed walk over the 80 cells c1 <= 7 of a 10x10 board: row 0 left to right, rows 1..9 as a serpentine over
    c1 1..7, back up c1 == 0.  Columns 8 and 9 stay free."""
    cyc = [(0, y) for y in range(8)]
    for r in range(1, 10):
        cyc += [(r, y) for y in (range(7, 0, -1) if r % 2 else range(1, 8))]
    cyc += [(r, 0) for r in range(9, 0, -1)]
    assert len(cyc) == len(set(cyc)) == 80
    assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(cyc, cyc[1:] + cyc[:1]))
    return cyc


# env -> (length of the long body, where snake 1 waits, where snake 2 waits or None, what happens):
#   "piece i": snake 1 runs into post-move piece i of the long body, which lives; "last": into its last piece;
#   "dies popped": the long snake turns into itself in the same step, its tail pops, snake 1 runs into its last piece;
#   "dies freed": likewise, and snake 1 moves onto the cell the popped tail left (and lives);
#   "dies kept": the long snake runs head-on into snake 2, which waits on a fruit: it eats while dying, its tail stays,
#   and snake 1 runs into that tail
LONG_CASES = [(76, (5, 8), None, 63), (76, (4, 8), None, 64), (76, (6, 8), None, 70), (76, (3, 8), None, "last"),
              (76, (5, 8), None, "dies popped"), (76, (7, 8), None, "dies freed"), (67, (6, 8), (4, 8), "dies kept")]
LONG_WARMUP = 130   # steps before anything happens: the 64-slot ring and the 128-cell overflow ring have both turned


def long_states(cyc):
    states = []
    for length, w1, w2, what in LONG_CASES:
        body = [cyc[(length - 1 - i) % 80] for i in range(length)]   # head at cyc[length - 1], tail at cyc[0]
        d = (body[0][0] - body[1][0], body[0][1] - body[1][1])
        fruits = [(0, 9), (1, 9), (2, 9)]
        if what == "dies kept":
            fruits[0] = w2
        states.append(cp.state([body, [w1], [w2] if w2 else []], [d, (0, 0), (0, 0)], fruits=fruits, grow_to=[length, 3, 3]))
    return states


def long_actions(cyc, states, t, fired):
    """The actions of one step, chosen on the twin's states: the long snake follows the cycle, snake 1 waits until its
    moment has come.  Marks the envs whose moment it was in `fired`."""
    nxt = {c: cyc[(i + 1) % 80] for i, c in enumerate(cyc)}
    code = {v: k for k, v in sp.DIRS.items()}
    act = np.zeros((len(states), 3), np.int32)
    for e, st in enumerate(states):
        body = [tuple(c) for c in st["snakes"][0]]
        _, w1, w2, what = LONG_CASES[e]
        if fired[e] or len(body) < 60 or body[0] not in nxt:
            continue
        head, to = body[0], nxt[body[0]]
        act[e, 0] = code[(to[0] - head[0], to[1] - head[1])]
        if t < LONG_WARMUP or [tuple(c) for c in st["snakes"][1]] != [w1]:
            continue
        target, n = (w1[0], 7), len(body)   # the cell snake 1 moves onto with action 4; the long snake pops: len == grow_to
        vel = tuple(st["vels"][0])
        turn_in = vel[0] == 0 and (head[0] - 1, head[1]) in body[1:n - 1] and to != (head[0] - 1, head[1])
        if isinstance(what, int):
            go = body.index(target) + 1 == what if target in body else False
        elif what == "last":
            go = body[n - 2] == target
        elif what == "dies popped":
            go = body[n - 2] == target and turn_in
        elif what == "dies freed":
            go = body[n - 1] == target and turn_in
        else:   # "dies kept"
            go = head == (w2[0], 7) and vel == (0, 1) and body[n - 1] == target
        if go:
            fired[e] = True
            act[e, 1] = 4
            if what in ("dies popped", "dies freed"):
                act[e, 0] = 3   # (-1, 0): into the row it came along
            if what == "dies kept":
                act[e, 0] = 0   # straight on, off the cycle, onto snake 2 and its fruit
    return act


def long_expectations(e, tw):
    """What the twin has to show in the step in which env e's moment came."""
    length, w1, w2, what = LONG_CASES[e]
    cause, by, bodies, now = tw.cause[e].tolist(), tw.by[e].tolist(), tw.bodies[e], tw.now[e]
    hit = bodies[0].index(bodies[1][0]) if bodies[1][0] in bodies[0][1:] else None
    if isinstance(what, int) or what == "last":
        assert cause == [0, cp.BODY, 0] and by == [0, 1, 0] and len(now["snakes"][0]) == length, (what, cause, by)
        assert hit == (length - 1 if what == "last" else what), (what, hit)
    elif what == "dies popped":
        assert cause == [cp.SELF, cp.BODY, 0] and by == [0, 1, 0] and hit == length - 1 and len(bodies[0]) == length, (cause, by, hit)
    elif what == "dies freed":
        assert cause == [cp.SELF, 0, 0] and by == [0, 0, 0] and len(bodies[0]) == length and len(now["snakes"][1]) == 2, (cause, by)
    else:
        assert cause == [cp.HEAD_ON, cp.BODY, cp.HEAD_ON] and by == [0x40, 0x01, 0x10], (cause, by)
        assert hit == length and len(bodies[0]) == length + 1 and now["grow_to"][0] == length + 2, (hit, len(bodies[0]))


def long_play(step):
    """The long-body play on the twin; `step(tw, act)` is called behind every twin step.  Returns the number of steps."""
    cyc = long_cycle()
    cfg = sp.scenario("snake_env", 10, 3, "safe_greedy", 1, len(LONG_CASES), 1, max_steps=2000)
    states = long_states(cyc)
    tw = cp.Twin(cfg)
    for e, st in enumerate(states):
        tw.ora.set_state(e, st)
        tw.states[e] = tw.read(e)
    fired, seen = [False] * len(states), [False] * len(states)
    t = 0
    while not all(seen):
        assert t < LONG_WARMUP + 170, ("a moment never came", fired)
        act = long_actions(cyc, tw.states, t, fired)
        tw.step(act)
        if t < LONG_WARMUP:
            assert all(len(st["snakes"][0]) == LONG_CASES[e][0] for e, st in enumerate(tw.now)), "the long snakes walk on"
        for e in range(len(states)):
            if fired[e] and not seen[e]:
                long_expectations(e, tw)
                seen[e] = True
        step(tw, act)
        t += 1
    return cfg, states, t


def test_long_bodies_out_of_both_rings():
    """Bodies of 76 and 67 pieces walk a closed path for 130 steps, then a waiting snake runs into piece 63, 64, 70 and
    the last piece of one that lives, and into the last piece of one that dies in the same step, its tail popped or
    kept: pieces past 63 come out of the overflow ring, through either view."""
    import torch
    cyc = long_cycle()
    cfg = sp.scenario("snake_env", 10, 3, "safe_greedy", 1, len(LONG_CASES), 1, max_steps=2000)
    env = gh.install(cfg, long_states(cyc), auto_reset=False)
    snap, b = env.clone(record_policy="short"), Bufs(env)

    def device_step(tw, act):
        b.refill()
        done, flags = _chain(env, snap, b, torch.from_numpy(act).to(env.device))
        _same(done.cpu().numpy(), tw.done, "done")
        _check_outputs(b, tw, "long bodies")
        _same(flags.cpu().numpy(), tw.flags, "flags")

    _, _, steps = long_play(device_step)
    assert steps >= LONG_WARMUP + 1 and env.stats()["errors"] == 0
    env.close(), snap.close()


# ------------------------------------------------------------------------------------------ 6. each output alone
def test_each_output_alone_gives_the_bytes_of_all_together():
    import torch
    cfg = ap.scenario("snake_env", 3, 9, max_steps=15, num_envs=23, steps=12)
    env, snap, tw = _env(cfg), _env(cfg), cp.Twin(cfg)
    bufs = [Bufs(env) for _ in range(5)]
    env.reset()
    for t in range(12):
        act = torch.from_numpy(tw.step()).to(env.device)
        _snapshot(snap, env)
        _, _, done, _ = env.step_device(act)
        for b, which in zip(bufs, [OUTPUTS] + [(k,) for k in OUTPUTS]):
            b.refill()
            _causes(env, snap, b, which)
            _check_outputs(b, tw, (t, which), which)
        env.reset_device(mask=done)
    env.close(), snap.close()


# ------------------------------------------------------------------------------------------ 7. read-only
def test_the_call_only_reads_both_handles():
    import torch
    cfg = ap.scenario("adversarial", 3, 13, max_steps=20, num_envs=33, steps=10)
    env, snap, tw = _env(cfg), _env(cfg), cp.Twin(cfg)
    b = Bufs(env)
    env.reset()
    for _ in range(10):
        env.step_device(torch.from_numpy(tw.step()).to(env.device))
        env.reset_device(mask=env._done)
    _snapshot(snap, env)
    env.step_device(torch.from_numpy(tw.step()).to(env.device))
    blobs = [h.get_state_all().copy() for h in (env, snap)]
    stats = [h.stats() for h in (env, snap)]
    for _ in range(3):
        _causes(env, snap, b)
    _check_outputs(b, tw, "read-only")
    for h, blob, st, name in zip((env, snap), blobs, stats, ("after", "before")):
        assert np.array_equal(h.get_state_all(), blob), (name, "state changed")
        assert h.stats() == st, (name, "env_steps or a total moved")
    env.close(), snap.close()


# ------------------------------------------------------------------------------------------ 8. HIP graph
def test_graph_of_the_five_calls_replayed_50_times():
    import torch
    K = 50
    cfg = ap.scenario("snake_env", 3, 14, max_steps=15, num_envs=40, steps=K)
    env, snap, tw = _env(cfg), _env(cfg), cp.Twin(cfg)
    b = Bufs(env)
    _same(env.reset(), tw.obs, "reset obs")
    blob = env.get_state_all()
    acts = torch.zeros((40, 3), dtype=torch.int32, device=env.device)
    env.arm_agents_device()
    chain = lambda: _chain(env, snap, b, acts)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        chain()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chain()
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    env.arm_agents_device()
    deaths = 0
    for t in range(K):
        acts.copy_(torch.from_numpy(tw.step()))
        b.refill()
        g.replay()
        _same(env._done.cpu().numpy(), tw.done, (t, "done"))
        _check_outputs(b, tw, t)
        deaths += int((tw.cause != 0).sum())
    assert deaths >= 20
    env.close(), snap.close()


# ------------------------------------------------------------------------------------------ 9. refusals
def test_every_refusal_in_order():
    import torch
    cfg = ap.scenario("snake_env", 3, 15, num_envs=5)
    env, snap = _env(cfg), _env(cfg)
    b = Bufs(env)
    env.reset()
    C, B, V, W = (_ptr(b, k) for k in OUTPUTS)
    last = lambda: env._L.msnake_last_error().decode()
    others = []

    def other(base=cfg, **kw):
        others.append(_env(dict(base, **{k: v for k, v in kw.items() if k in base}), **{k: v for k, v in kw.items() if k not in base}))
        return others[-1]

    # 1. handles
    assert _raw(None, snap, C) == E_HANDLE and _raw(env, None, C) == E_HANDLE
    gone = other()
    gone.close()
    assert _raw(env, gone, C) == E_HANDLE and _raw(gone, env, C) == E_HANDLE
    # 2. one handle twice, whatever else is wrong
    assert _raw(env, env, C) == E_ARG and "same handle" in last()
    assert _raw(env, env) == E_ARG and "same handle" in last()
    # 3. the board, with msnake_copy_envs' wording; in front of the env count
    assert _raw(env, other(dim=8, num_envs=4), C) == E_ARG and "before has dim 8, after has dim 6" in last()
    assert _raw(env, other(n_snakes=2, n_fruits=2), C) == E_ARG and "n_snakes" in last()
    assert _raw(env, other(rules=sp.RULES["adversarial"]), C) == E_ARG and "has rules" in last()
    nw = dict(ap.scenario("new_world", 3, 15, n_fruits=4, num_envs=5))
    nw1, nw2, nw3 = other(nw), other(nw, n_fruits=5), other(nw, num_envs=6)
    assert _raw(nw1, nw2, C) == E_ARG and "n_fruits" in last()
    # 4. the env count, in front of the rule set
    assert _raw(env, other(num_envs=6), C) == E_ARG and "num_envs" in last()
    assert _raw(nw1, nw3, C) == E_ARG and "num_envs" in last()
    # 5. new_world, in front of auto_reset
    assert _raw(nw1, other(nw), C, B, V, W) == E_ARG and "new_world" in last()
    assert _raw(other(nw, auto_reset=True), nw1) == E_ARG and "new_world" in last()
    # 6. an `after` that resets itself, in front of the outputs; `before` may
    auto = other(auto_reset=True)
    assert _raw(auto, snap, C) == E_ARG and "auto_reset" in last()
    assert _raw(auto, snap) == E_ARG and "auto_reset" in last()
    # 7. nothing to write
    assert _raw(env, snap) == E_ARG and "nothing to write" in last()
    torch.cuda.synchronize()
    assert all(b.untouched(k) for k in OUTPUTS), "a refused call wrote"
    # accepted: `before` with auto_reset = 1, other seed / max_steps / layout, outputs at odd addresses
    odd = Bufs(env, offset=1)
    assert all(_ptr(odd, k) % 2 == 1 for k in OUTPUTS)
    tw = cp.Twin(cfg)
    before = other(auto_reset=True, seed=99, max_steps=500, record_policy="short", envs_per_block=1)
    for t in range(6):
        act = torch.from_numpy(tw.step()).to(env.device)
        _snapshot(before, env)
        _, _, done, _ = env.step_device(act)
        odd.refill()
        _causes(env, before, odd)
        env.reset_device(mask=done)
        _check_outputs(odd, tw, (t, "odd addresses"))
    # the wrapper's own checks
    with pytest.raises(ValueError, match="cause_out"):
        env.death_causes_device(snap, cause_out=torch.zeros((5, 3), dtype=torch.int8, device=env.device))
    with pytest.raises(ValueError, match="where_out"):
        env.death_causes_device(snap, where_out=torch.zeros((5, 3), dtype=torch.int8, device=env.device))
    with pytest.raises(TypeError, match="MultiSnakeVecEnv"):
        env.death_causes_device(None)
    others.append(nw1.clone())
    with pytest.raises(RuntimeError, match="new_world"):
        nw1.death_causes_device(others[-1])
    for h in [env, snap] + others:
        h.close()


# ------------------------------------------------------------------------------------------ 10. wrapper and learner
def test_step_agents_device_with_causes_equals_the_manual_chain():
    import msnake
    import torch
    cfg = dict(ap.SCENARIOS["S6"], steps=60)
    env, manual, snap, tw = _env(cfg), _env(cfg), _env(cfg), cp.Twin(cfg)
    plain = _env(cfg)
    b = Bufs(manual)
    for h in (env, manual, plain):
        _same(h.reset(), tw.obs, "reset obs")
    deaths = 0
    for t in range(60):
        act = torch.from_numpy(tw.step()).to(env.device)
        b.refill()
        _chain(manual, snap, b, act)
        obs, rew, done, info, agents, why = env.step_agents_device(act, causes=True)
        assert isinstance(why, msnake.DeathCauses) and why._fields == OUTPUTS
        for k in OUTPUTS:
            _same(getattr(why, k).cpu().numpy(), b.host(k), (t, k, "the manual chain"))
            _same(b.host(k), getattr(tw, k), (t, k, "the twin"))
        out = plain.step_agents_device(act)
        assert len(out) == 5, "causes=False returns today's tuple"
        for got, want, what in zip((obs, rew, done, info), out[:4], ("obs", "rew", "done", "info")):
            _same(got.cpu().numpy(), want.cpu().numpy(), (t, what))
        for k in ("rew", "ate", "flags", "info"):
            _same(getattr(agents, k).cpu().numpy().view(np.uint8), getattr(out[4], k).cpu().numpy().view(np.uint8), (t, k))
            _same(getattr(agents, k).cpu().numpy().view(np.uint8), np.ascontiguousarray(getattr(tw, k)).view(np.uint8), (t, k, "twin"))
        _same(obs.cpu().numpy(), manual._obs.cpu().numpy(), (t, "obs of the manual chain"))
        deaths += int((tw.cause != 0).sum())
    assert deaths >= 20
    assert plain._snapshot is None and env._snapshot is not None
    held = env._snapshot
    env.close()
    assert held.closed, "close() closes the snapshot"
    for h in (manual, snap, plain):
        h.close()


def test_kill_bonus_in_the_runner_and_learn():
    import torch
    from msnake import selfplay
    cfg = ap.scenario("snake_env", 3, 16, max_steps=60, num_envs=16)
    env = _env(cfg)
    torch.manual_seed(0)
    model = selfplay.RayPolicy().to(env.device)
    runner = selfplay.Runner(env, model, [], 64, 0.99, 0.95, rays=True, all_snakes=True, kill_bonus=0.5)
    runner.run()
    flags, victims = runner.last_flags.cpu().numpy(), runner.last_victims.cpu().numpy()
    cause = runner.last_cause.cpu().numpy()
    pop = np.array([bin(v & 15).count("1") for v in range(256)], np.float32)[victims]
    want = runner.last_agent_rew.cpu().numpy() + np.where((flags & ap.WAS_ALIVE) != 0, np.float32(0.5) * pop, np.float32(0))
    _same(runner.last_rew.cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32), "rew + 0.5 x kills")
    assert pop.sum() >= 1, "some snake died on another's body"
    assert ((pop > 0) <= ((flags & ap.WAS_ALIVE) != 0)).all(), "a killer took part in the step"
    _same(cause != 0, (flags & ap.DIED) != 0, "cause != 0 is DIED")
    assert runner.last_deaths == dict(deaths_wall=int(((cause & cp.WALL) != 0).sum()), deaths_self=int(((cause & cp.SELF) != 0).sum()),
                                      deaths_head_on=int(((cause & cp.HEAD_ON) != 0).sum()),
                                      deaths_body=int(((cause & cp.BODY) != 0).sum()), kills=int(pop.sum()))
    env.close()
    with pytest.raises(ValueError, match="all_snakes"):
        selfplay.learn(env, rays=True, kill_bonus=0.5)
    env = _env(cfg)
    model, history = selfplay.learn(env, nsteps=8, total_timesteps=2 * 16 * 8, nminibatches=4, noptepochs=2, rays=True,
                                    all_snakes=True, kill_bonus=0.5, log_fn=None)
    assert len(history) == 2
    for kvs in history:
        assert all(np.isfinite(kvs[k]) for k in ("policy_loss", "value_loss", "policy_entropy", "approxkl", "clipfrac"))
        assert all(isinstance(kvs[k], int) and kvs[k] >= 0 for k in selfplay.DEATH_KEYS), kvs
    assert selfplay.DEATH_KEYS == ("deaths_wall", "deaths_self", "deaths_head_on", "deaths_body", "kills")
    env.close()
    env = _env(cfg)   # without the bonus nothing asks for causes
    _, history = selfplay.learn(env, nsteps=8, total_timesteps=16 * 8, nminibatches=4, noptepochs=1, rays=True, all_snakes=True,
                                log_fn=None)
    assert not set(selfplay.DEATH_KEYS) & set(history[0]) and env._snapshot is None
    env.close()
