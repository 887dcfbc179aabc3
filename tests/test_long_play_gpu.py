"""Long-lived play on the HIP path: action tapes recorded from scripted play on the CPU oracle (tests/scripted_play.py)
replayed through every kernel path of the library and compared with the oracle on EVERY step -- reward, done,
num_snakes, episode return / length and every observation byte; the canonical state at sampled steps and on the step
before and after every episode end; msnake_get_stats at the end.  Integer work: there is no tolerance.

What the plays reach (asserted on the oracle's recording before the library is touched, scripted_play.check_coverage):
boards that fill completely (6x6, 10x10), bodies that grow by eating through the 64-cell register ring into the
overflow ring and stay there for two turns of it, episodes that run into the default cap of 2000 steps, an
adversarial fruit list of 67 entries (past the one-chunk 64-entry path), new_world envs that play on to the cap after
the main snake's death.  tests/test_oracle_long_play.py pins the oracle to the reference on the same kinds of play.
"""
import numpy as np
import pytest

import scripted_play as sp
from gpu_harness import make_env as _mk

pytestmark = pytest.mark.gpu


def _state(env, e):
    from oracle.snake_oracle import flat_to_state
    return flat_to_state(env.get_state_words(e))


def _recording(name, auto_reset=True, envs=None, expect=None):
    """The oracle's recording of a scenario, its coverage conditions asserted.  envs=(lo, hi): that slice of the
    batch as a recording of its own (an env plays the same game in any batch that holds its global id)."""
    rec = sp.recorded(name, auto_reset)
    sp.check_coverage(rec["cfg"], rec["coverage"])
    if envs is not None:
        lo, hi = envs
        cfg = dict(rec["cfg"], num_envs=hi - lo, env_id_base=rec["cfg"]["env_id_base"] + lo, expect=list(expect or ()))
        sub = dict(cfg=cfg, auto_reset=rec["auto_reset"], states={t: s[lo:hi] for t, s in rec["states"].items()})
        for k, v in rec.items():
            if isinstance(v, np.ndarray):
                sub[k] = np.ascontiguousarray(v[:, lo:hi] if v.ndim > 1 else v[lo:hi])
        sub["coverage"] = sp.coverage(cfg, sub["body_max"], sub["n_fruits"], sub["done"], sub["ep_len"], sub["ctr"])
        sp.check_coverage(cfg, sub["coverage"])
        rec = sub
    return rec


def _check_steps(rec, every=64):
    """Steps after which the canonical state is compared: every `every`-th, the last, and the step before and the step
    of every episode end -> {t: envs to compare (None = all)}."""
    T, E = rec["done"].shape
    need = {t: None for t in list(range(0, T, every)) + [T - 1]}
    for t, e in zip(*np.nonzero(rec["done"])):
        for tt in (t - 1, t):
            if tt >= 0 and need.get(tt, ()) is not None:
                need.setdefault(tt, set()).add(int(e))
    return need


def _stepper(env, tape):
    """run(a, b): steps a..b-1 through msnake_step (step_device), outputs gathered on the device."""
    import torch

    def run(a, b):
        out = [tuple(x.clone() for x in env.step_device(tape[t])) for t in range(a, b)]
        return tuple(torch.stack([o[k] for o in out]).cpu().numpy() for k in range(4))
    return run


def _roller(env, tape, chunk):
    """run(a, b): steps a..b-1 through msnake_rollout_tape (one persistent launch per chunk of `chunk` steps)."""
    import torch

    def run(a, b):
        parts = [env.rollout_device(tape[t:min(t + chunk, b)]) for t in range(a, b, chunk)]
        return tuple(torch.cat([p[k] for p in parts]).cpu().numpy() for k in range(4))
    return run


def _replay(rec, env, run, scale=1, every=64, reset=None, counted_steps=None):
    """The recorded tape through `run` on `env` against the recording and a live replay of the oracle (frames, states).
    reset: what brings the handle to the start of the play and returns its observation (default env.reset).
    counted_steps: the steps msnake_get_stats' env_steps has seen (default: all of them)."""
    cfg = rec["cfg"]
    T, E = rec["done"].shape
    ora = sp.make_oracle(cfg)
    up = (lambda o: o) if scale == 1 else (lambda o: np.repeat(np.repeat(o, scale, axis=-3), scale, axis=-2))
    o0 = ora.reset()
    assert np.array_equal(sp.crc_rows(o0), rec["obs0_crc"])
    assert np.array_equal((reset or env.reset)(), up(o0)), "reset observation"
    need = _check_steps(rec, every)
    t0 = 0
    for b in sorted(need):
        obs, rew, done, info = run(t0, b + 1)
        for j, t in enumerate(range(t0, b + 1)):
            o_obs = ora.step(rec["actions"][t])[0]
            assert np.array_equal(sp.crc_rows(o_obs), rec["obs_crc"][t]), t       # (the live oracle is the recorded one)
            assert np.array_equal(rew[j], rec["reward"][t]), ("reward", t)
            assert np.array_equal(done[j], rec["done"][t]), ("done", t)
            assert np.array_equal(info[j][:, 3], rec["done"][t]), ("info.done", t)
            assert np.array_equal(info[j][:, 2], rec["num_snakes"][t]), ("num_snakes", t)
            assert np.array_equal(info[j][:, 1], rec["ep_len"][t]), ("ep_len", t)
            assert np.array_equal(info[j][:, 0].copy().view(np.float32), rec["ep_return"][t]), ("ep_return", t)
            assert np.array_equal(obs[j], up(o_obs)), ("obs", t)
        for e in (range(E) if need[b] is None else sorted(need[b])):
            want = ora.get_state(e)
            assert _state(env, e) == want, ("state", b, e)
            if b in rec["states"]:
                assert rec["states"][b][e] == want
        t0 = b + 1
    _check_stats(env, rec, counted_steps)


def _check_stats(env, rec, counted_steps=None):
    d = rec["done"].astype(bool)
    st = env.stats()
    T, E = d.shape
    assert st["errors"] == 0
    assert st["episodes"] == int(d.sum()) and st["ep_len_sum"] == int(rec["ep_len"][d].sum()), st
    assert st["ep_return_sum"] == int(round(float(rec["ep_return"][d].astype(np.float64).sum()))), st
    assert st["env_steps"] == (T if counted_steps is None else counted_steps) * E, st


def _tape(env, rec):
    import torch
    return torch.from_numpy(rec["actions"]).to(env.device)


# ------------------------------------------------------------------------------------------ msnake_step
@pytest.mark.parametrize("name", list(sp.SCENARIOS))
def test_every_scenario_on_the_step_path(name):
    """Every scenario through msnake_step on the handle's default launch shape.  A10x3: the fruit list passes 64
    entries (67), found with safe greedy at eps 0.02 in global env 54 of seed 7, so the bound there is 65."""
    rec = _recording(name)
    env = _mk(rec["cfg"])
    _replay(rec, env, _stepper(env, _tape(env, rec)))
    env.close()


@pytest.mark.parametrize("name,record,epb", [(n, r, b) for n in ("S6", "S12") for r, b in
                                             (("full", 1), ("short", 4), ("full", 8), ("short", 8), ("short", 1))] +
                         [("A10", "short", 4), ("A10", "full", 8)])
def test_record_policy_and_envs_per_block(name, record, epb):
    """Full and short record, 1 / 4 / 8 envs per workgroup: on a board that fills (6x6), on capped episodes with bodies
    two turns round the overflow ring (12x12), and on an adversarial 10x10 that does both."""
    rec = _recording(name)
    env = _mk(rec["cfg"], record_policy=record, envs_per_block=epb)
    _replay(rec, env, _stepper(env, _tape(env, rec)))
    env.close()


# ------------------------------------------------------------------------------------------ msnake_rollout_tape
@pytest.mark.parametrize("chunk,record", [(7, "auto"), (48, "short"), (200, "auto"), (200, "short")])
@pytest.mark.parametrize("name", ["S10", "S12"])
def test_persistent_tape_in_chunks(name, chunk, record):
    """msnake_rollout_tape through rollout_device: the state leaves and re-enters registers every `chunk` steps -- 7 (no
    divisor of 64: every phase of the register ring), 48, 200 (longer than the overflow ring: 128 cells at 10x10, 192
    at 12x12).  A launch ends at every step whose state is compared, so the 10x10 play is cut to two of its envs, whose
    6 episodes leave most 200-step launches whole; the 12x12 play has all its episode ends at the cap."""
    if name == "S10":
        rec = _recording(name, envs=(0, 2), expect=["filled", "over64"])
        assert rec["coverage"]["longest_run_over_64"] >= 200
    else:
        rec = _recording(name)
    env = _mk(rec["cfg"], record_policy=record)
    _replay(rec, env, _roller(env, _tape(env, rec), chunk), every=1024)
    env.close()


# ------------------------------------------------------------------------------------------ fused up-scale
@pytest.mark.parametrize("name,scale,lo,hi", [("S19x3", 4, 0, 8), ("S10", 7, 2, 6)])
def test_fused_upscale_on_long_play(name, scale, lo, hi):
    """obs_scale 4 (19x19) and 7 (10x10): every byte is the oracle's frame replicated, for the whole play."""
    rec = _recording(name, envs=(lo, hi), expect=["over64"])
    env = _mk(rec["cfg"], obs_scale=scale)
    assert env.obs_shape[:2] == (84, 84)
    _replay(rec, env, _stepper(env, _tape(env, rec)), scale=scale)
    env.close()


# ------------------------------------------------------------------------------------------ masked reset
def _reset_paths(rec, max_steps=None):
    """terminal_obs=True, and auto_reset=False + reset_device(mask=done, final_out, truncated_out), against the
    recording made with the oracle's reset_envs(done): terminal rows, truncation flags, everything else as ever."""
    import torch
    cfg = rec["cfg"]
    T, E = rec["done"].shape
    kw = {} if max_steps is None else dict(max_steps=max_steps)
    a = _mk(cfg, terminal_obs=True, **kw)
    b = _mk(cfg, auto_reset=False, **kw)
    ora = sp.make_oracle(cfg, auto_reset=False, max_steps=max_steps)
    o0 = ora.reset()
    assert np.array_equal(a.reset(), o0) and np.array_equal(b.reset(), o0)
    tape = _tape(a, rec)
    final_b = torch.zeros_like(b._obs)
    trunc_b = torch.zeros(E, dtype=torch.uint8, device=b.device)
    need = _check_steps(rec)
    for t in range(T):
        oa, ra, da, ia = (x.cpu().numpy() for x in a.step_device(tape[t]))
        ob, rb, db, ib = (x.cpu().numpy() for x in b.step_device(tape[t]))
        term = ora.step(rec["actions"][t])[0].copy()
        d = rec["done"][t].astype(bool)
        for rew, done, info in ((ra, da, ia), (rb, db, ib)):
            assert np.array_equal(rew, rec["reward"][t]) and np.array_equal(done, rec["done"][t]), t
            assert np.array_equal(info[:, 2], rec["num_snakes"][t]) and np.array_equal(info[:, 1], rec["ep_len"][t]), t
            assert np.array_equal(info[:, 0].copy().view(np.float32), rec["ep_return"][t]), t
        assert np.array_equal(ob, term), ("terminal frame of the raw step", t)
        if t in need:
            for e in (range(E) if need[t] is None else sorted(need[t])):
                assert _state(b, e) == ora.get_state(e), ("state before the reset", t, e)
        if d.any():
            b.reset_device(mask=torch.from_numpy(d).to(b.device), out=b._obs, final_out=final_b, truncated_out=trunc_b)
            want_obs, want_final, want_trunc = ora.reset_envs(d)
            assert np.array_equal(want_trunc, rec["truncated"][t]), t
            assert np.array_equal(sp.crc_rows(want_final[d]), rec["final_crc"][t][d]), t
            for final, trunc in ((a.final_obs, a.truncated), (final_b, trunc_b)):
                assert np.array_equal(final.cpu().numpy()[d], term[d]), ("terminal observation", t)
                assert np.array_equal(trunc.cpu().numpy(), want_trunc), ("truncated", t)
            assert np.array_equal(b._obs.cpu().numpy(), want_obs), ("reset observation", t)
            for e in np.nonzero(d)[0]:
                assert _state(a, e) == _state(b, e) == ora.get_state(int(e)), ("state after the reset", t, e)
        assert np.array_equal(oa, ora.obs), ("observation", t)
        assert np.array_equal(sp.crc_rows(oa), rec["obs_crc"][t]), t
    _check_stats(a, rec)
    _check_stats(b, rec)
    a.close(); b.close()


def test_masked_reset_truncation_at_the_2000_step_cap():
    """14x14: every episode that reaches step 2000 is reported truncated (with a body of up to 69 cells behind it),
    the early deaths are not."""
    rec = _recording("S14", auto_reset=False)
    d = rec["done"].astype(bool)
    capped = d & (rec["ep_len"] == 2000)
    assert capped.sum() >= 4 and (rec["truncated"][capped] == 1).all() and not rec["truncated"][d & ~capped].any()
    _reset_paths(rec)


@pytest.mark.parametrize("name", ["S6", "A10"])
def test_masked_reset_on_full_boards(name):
    """Board-filling play: no episode that ended by death is truncated; the terminal observation of a full board."""
    rec = _recording(name, auto_reset=False)
    d = rec["done"].astype(bool)
    died = d & (rec["ep_len"] < 2000)
    assert died.sum() >= 4 and not rec["truncated"][died].any()
    assert (rec["truncated"][d & (rec["ep_len"] == 2000)] == 1).all()
    _reset_paths(rec)


def test_death_exactly_on_step_max_steps():
    """max_steps lowered to a recorded death step: of the first episodes that filled the 6x6 board, the shortest one
    ends by death ON step max_steps = its length, which is not a truncation, while the longer ones are cut there
    alive, which is.  The play is recorded again on the oracle with the lowered cap (the tape is the same up to that
    step) and runs on for three caps."""
    base = _recording("S6", envs=(0, 8), expect=["filled"])
    first = [(int(np.nonzero(base["done"][:, e])[0][0]), e) for e in range(8)]   # (step, env) of every first episode end
    first = [(t, e) for t, e in first if base["body_max"][t - 1, e] >= 35]        # ... with the board full
    assert len(first) >= 2
    m, e0 = min((t + 1, e) for t, e in first)
    assert 50 < m < 2000 and base["ep_len"][m - 1, e0] == m
    rec = sp.record(dict(base["cfg"], max_steps=m, steps=3 * m), auto_reset=False)
    assert np.array_equal(rec["actions"][:m], base["actions"][:m])
    dd = rec["done"].astype(bool)
    assert dd[m - 1, e0] and rec["ep_len"][m - 1, e0] == m and rec["truncated"][m - 1, e0] == 0
    assert rec["body_max"][m - 2, e0] >= 35 and rec["truncated"][m - 1].sum() >= 1 and rec["truncated"][dd].sum() >= 3
    _reset_paths(rec, max_steps=m)


# ------------------------------------------------------------------------------------------ HIP graph, checkpoint
def test_hip_graph_replay_of_a_whole_play():
    """One captured msnake_step (a single-node graph) replayed for a whole capped 12x12 play."""
    import torch
    rec = _recording("S12")
    env = _mk(rec["cfg"])
    env.reset()
    blob = env.get_state_all()
    acts = torch.zeros((rec["cfg"]["num_envs"], rec["cfg"]["n_snakes"]), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step_device(acts)
    torch.cuda.synchronize()
    tape = _tape(env, rec)

    def run(a, b):
        res = []
        for t in range(a, b):
            acts.copy_(tape[t])
            g.replay()
            res.append(tuple(x.clone() for x in out))
        return tuple(torch.stack([o[k] for o in res]).cpu().numpy() for k in range(4))

    def back_to_start():  # the warm-up step moved the envs: back to the state after reset(), totals cleared
        env.set_state_all(blob)
        env.stats(reset=True)
        return env.render()
    # episodes and their totals are accumulated on the device, so replays count; env_steps is counted on the host per API
    # call (include/msnake.h, msnake_get_stats), so the replays of a captured step add nothing to it
    _replay(rec, env, run, reset=back_to_start, counted_steps=0)
    env.close()


@pytest.mark.parametrize("name", ["S12", "A10x3"])
def test_checkpoint_in_the_middle_of_a_long_play(name):
    """get_state_all() at a step where a body holds over 64 cells and its overflow ring has turned (the head of the
    overflow ring is not at 0), set_state_all() into a fresh handle (which lays the ring out from 0 again): both go
    on identically, and like the oracle, to the end of the play."""
    rec = _recording(name)
    over = rec["body_max"] > 64
    run = np.zeros(over.shape[1], int)
    t_cp = None
    for t in range(over.shape[0]):
        run = np.where(over[t], run + 1, 0)
        if (run >= (100 if name == "S12" else 10)).any():
            t_cp = t
            break
    assert t_cp is not None and t_cp < over.shape[0] - 300
    a = _mk(rec["cfg"])
    tape = _tape(a, rec)
    head = {k: (v[:t_cp + 1] if isinstance(v, np.ndarray) and v.ndim > 1 else v) for k, v in rec.items()}
    head["states"] = {t: s for t, s in rec["states"].items() if t <= t_cp}
    _replay(head, a, _stepper(a, tape))
    blob = a.get_state_all()
    b = _mk(rec["cfg"])
    b.reset()
    b.set_state_all(blob)
    ora = sp.make_oracle(rec["cfg"])
    ora.reset()
    for t in range(t_cp + 1):
        ora.step(rec["actions"][t], want_obs=False)
    for t in range(t_cp + 1, over.shape[0]):
        ra = [x.cpu().numpy() for x in a.step_device(tape[t])]
        rb = [x.cpu().numpy() for x in b.step_device(tape[t])]
        o_obs = ora.step(rec["actions"][t])[0]
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y), t
        assert np.array_equal(ra[0], o_obs), t
        assert np.array_equal(ra[1], rec["reward"][t]) and np.array_equal(ra[2], rec["done"][t]), t
        assert np.array_equal(ra[3][:, 1], rec["ep_len"][t]) and np.array_equal(ra[3][:, 2], rec["num_snakes"][t]), t
        if t % 97 == 0 or rec["done"][t].any():
            for e in range(over.shape[1]):
                assert _state(a, e) == _state(b, e) == ora.get_state(e), (t, e)
    _check_stats(a, rec)
    a.close(); b.close()
