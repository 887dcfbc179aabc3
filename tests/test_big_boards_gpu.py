"""The library against the reference at the top of the ranges: tests/golden/big_boards.npz (tests/big_boards.py) on
every step path.  The fixture holds what the REFERENCE did on boards up to 62x62 -- random play on both sides of every
board size at which a step kernel changes its envs per workgroup, late-game bodies of up to 3842 pieces, adversarial
fruit lists of over 3000 entries -- so nothing here rests on the CPU oracle but the terminal observations of the masked
reset, which the reference's vec layer never shows.

  msnake_step                      every run: observation CRCs, scalars and the tag of the states at every step
  msnake_step_tape / rollout_tape  every run, one call per stretch between the resets by hand: observation CRCs and
                                   scalars of every step, the states at the end of every call.  The persistent tape
                                   kernel has LDS bands of its own, and above them (9 channels from dim 57, 12 from
                                   dim 49) msnake_rollout_tape runs per-step launches: both sides are in the table
  msnake_step + msnake_reset_envs  the auto_reset runs on a handle without auto reset
  launch tuning                    one run per per-step band with every envs_per_block and both record policies
Integer work: there is no tolerance.
"""
import json
import os

import numpy as np
import pytest

import big_boards as bb
import scripted_play as sp
from golden_util import GOLDEN, crc_rows
from gpu_harness import make_env

pytestmark = pytest.mark.gpu

with np.load(os.path.join(GOLDEN, "big_boards.npz")) as _z:
    RUNS, REC = json.loads(str(_z["meta"]))["runs"], {k: _z[k] for k in _z.files if k != "meta"}
AUTO = [n for n, c in RUNS.items() if c["auto_reset"]]


def _g(name):
    return lambda k: REC[f"{name}_{k}"]


def _mk(cfg, **kw):
    return make_env(cfg, **dict(dict(auto_reset=cfg["auto_reset"]), **kw))


def _states(env):
    from oracle.snake_oracle import flat_to_state
    return [flat_to_state(env.get_state_words(e)) for e in range(env.num_envs)]


def _start(cfg, env):
    """The handle at the start of a run: reset, and for a late-game run the installed states.  Returns the observation."""
    from oracle.snake_oracle import state_to_flat
    obs = env.reset()
    if cfg["kind"] == "late":
        for e, st in enumerate(bb.start_states(cfg)):
            env.set_state_words(e, state_to_flat(st, cfg["n_snakes"]))
        obs = env.render()
    return obs


def _at_reset(name, k, obs, env):
    g = _g(name)
    assert np.array_equal(crc_rows(obs), g("reset_crc")[k]), (name, "reset observation", k)
    assert bb.state_tag(_states(env), RUNS[name]["rules"]) == g("reset_state_tag")[k], (name, "reset state", k)


def _scalars(name, t, rew, done, info):
    g = _g(name)
    assert np.array_equal(rew, g("reward")[t]), (name, "reward", t)
    assert np.array_equal(done, g("done")[t]) and np.array_equal(info[:, 3], g("done")[t]), (name, "done", t)
    assert np.array_equal(info[:, 2], g("num_snakes")[t]), (name, "num_snakes", t)
    assert np.array_equal(info[:, 1], g("ep_len")[t]), (name, "ep_len", t)
    assert np.array_equal(info[:, 0].copy().view(np.float32), g("ep_return")[t]), (name, "ep_return", t)


def _tape(name, env):
    import torch
    return torch.from_numpy(_g(name)("actions").astype(np.int32)).to(env.device)


def _launch_shape(env):
    import msnake
    return msnake._capi.launch_shape_for_config(env.cfg)


def _bands(cfg, env):
    """The envs per workgroup the library's host glue chose for this handle, which are the formula's."""
    step, tape = _launch_shape(env)
    C = bb.channels(cfg)
    assert step == bb.envs_per_workgroup(cfg["dim"], C, False) and tape == bb.envs_per_workgroup(cfg["dim"], C, True)
    return step, tape


def _finish(name, env, steps=None):
    cfg = RUNS[name]
    st = env.stats()
    assert st["errors"] == 0, st
    assert st["env_steps"] == (cfg["steps"] if steps is None else steps) * cfg["num_envs"], st
    env.close()


def _play_steps(name, env, every_state=True):
    """The whole run through msnake_step, compared at every step."""
    cfg, g = RUNS[name], _g(name)
    resets = bb.hand_resets(cfg)
    _at_reset(name, 0, _start(cfg, env), env)
    tape = _tape(name, env)
    for t in range(cfg["steps"]):
        obs, rew, done, info = (x.cpu().numpy() for x in env.step_device(tape[t]))
        assert np.array_equal(crc_rows(obs), g("obs_crc")[t]), (name, "observation", t)
        _scalars(name, t, rew, done, info)
        if every_state or t == cfg["steps"] - 1:
            assert bb.state_tag(_states(env), cfg["rules"]) == g("state_tag")[t], (name, "state", t)
        if t in resets:
            _at_reset(name, 1 + resets.index(t), env.reset(), env)


# ------------------------------------------------------------------------------------------ msnake_step
@pytest.mark.parametrize("name", list(bb.RUNS))
def test_every_run_on_the_step_path(name):
    env = _mk(RUNS[name])
    _bands(RUNS[name], env)
    _play_steps(name, env)
    _finish(name, env)


# ------------------------------------------------------------------------------------------ the tape calls
@pytest.mark.parametrize("persistent", [False, True], ids=["step_tape", "rollout_tape"])
@pytest.mark.parametrize("name", list(bb.RUNS))
def test_every_run_on_the_tape_paths(name, persistent):
    """One call per stretch between the resets by hand.  With persistent=True the handles above the tape kernel's last
    band (bb.envs_per_workgroup(.., tape=True) == 0: 57x57 and 62x62 with 9 channels, 49x49 and 62x62 with 12) are served
    by per-step launches, with the same results and the same env_steps."""
    cfg, g = RUNS[name], _g(name)
    env = _mk(cfg)
    _bands(cfg, env)
    resets = bb.hand_resets(cfg)
    _at_reset(name, 0, _start(cfg, env), env)
    tape = _tape(name, env)
    for a, b in bb.segments(cfg):
        obs, rew, done, info = (x.cpu().numpy() for x in env.rollout_device(tape[a:b], persistent=persistent))
        for t in range(a, b):
            assert np.array_equal(crc_rows(obs[t - a]), g("obs_crc")[t]), (name, "observation", t)
            _scalars(name, t, rew[t - a], done[t - a], info[t - a])
        assert bb.state_tag(_states(env), cfg["rules"]) == g("state_tag")[b - 1], (name, "state", b - 1)
        if b - 1 in resets:
            _at_reset(name, 1 + resets.index(b - 1), env.reset(), env)
    _finish(name, env)


def test_the_table_holds_both_sides_of_the_tape_limit():
    """The last dim on which the persistent kernel's second image fits and the first on which it does not, for 9 and 12
    channels, and the two handles the contract names: 62x62 snake_env and a 4-snake new_world handle above its limit."""
    tape = {n: bb.envs_per_workgroup(c["dim"], bb.channels(c), True) for n, c in RUNS.items()}
    assert tape["S56x3"] == 1 and tape["A57x3"] == 0 and tape["N48x4f32"] == 1 and tape["N49x4f17"] == 0
    assert tape["S62x3"] == 0 and tape["L_S62"] == 0 and tape["N62x4f32"] == 0 and tape["L_A62x3"] == 0
    assert {tape[n] for n in RUNS} == {0, 1, 2, 4, 8}


def test_the_tape_call_above_its_limit_is_capturable():
    """msnake_rollout_tape on a 57x57 handle (per-step launches) allocates nothing and does not synchronise: captured
    into a HIP graph five steps at a time and replayed, it plays the whole run."""
    import torch
    name = "A57x3"
    cfg, g = RUNS[name], _g(name)
    env = _mk(cfg)
    assert _bands(cfg, env)[1] == 0 and cfg["auto_reset"] and cfg["steps"] % 5 == 0
    _start(cfg, env)
    blob = env.get_state_all()
    tape = _tape(name, env)
    buf = torch.zeros_like(tape[:5])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.rollout_device(buf)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = env.rollout_device(buf)
    torch.cuda.synchronize()
    env.set_state_all(blob)   # the warm-up moved the envs: back to the start, totals cleared
    env.stats(reset=True)
    for a in range(0, cfg["steps"], 5):
        buf.copy_(tape[a:a + 5])
        graph.replay()
        obs, rew, done, info = (x.cpu().numpy() for x in out)
        for t in range(a, a + 5):
            assert np.array_equal(crc_rows(obs[t - a]), g("obs_crc")[t]), (name, "observation", t)
            _scalars(name, t, rew[t - a], done[t - a], info[t - a])
    assert bb.state_tag(_states(env), cfg["rules"]) == g("state_tag")[-1]
    _finish(name, env, steps=0)   # env_steps is counted on the host per API call: replays add nothing


# ------------------------------------------------------------------------------------------ step + masked reset
@pytest.mark.parametrize("name", AUTO)
def test_auto_reset_runs_through_step_and_reset_envs(name):
    """auto_reset = 0 and msnake_reset_envs(done, obs, final_obs, truncated) after every step with an episode end: the
    reset observations, scalars and states are the fixture's; the terminal observations and truncation flags, which the
    reference's vec layer drops, are the oracle's."""
    import torch
    cfg, g = RUNS[name], _g(name)
    E = cfg["num_envs"]
    env = _mk(cfg, auto_reset=False)
    ora = sp.make_oracle(cfg, auto_reset=False)
    ora.reset()
    if cfg["kind"] == "late":
        for e, st in enumerate(bb.start_states(cfg)):
            ora.set_state(e, st)
    _at_reset(name, 0, _start(cfg, env), env)
    tape = _tape(name, env)
    final = torch.full_like(env._obs, 0xA5)
    trunc = torch.full((E,), 0xA5, dtype=torch.uint8, device=env.device)
    n_done = 0
    for t in range(cfg["steps"]):
        obs, rew, done, info = env.step_device(tape[t])
        d = done.cpu().numpy().astype(bool)
        term = ora.step(g("actions")[t].astype(np.int32))[0].copy()
        assert np.array_equal(obs.cpu().numpy(), term), (name, "observation of the raw step", t)
        _scalars(name, t, rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy())
        if d.any():
            final.fill_(0xA5)
            env.reset_device(mask=done, out=env._obs, final_out=final, truncated_out=trunc)
            _, _, want_trunc = ora.reset_envs(d, final_obs=None)
            got = final.cpu().numpy()
            assert np.array_equal(got[d], term[d]) and (got[~d] == 0xA5).all(), (name, "terminal observation", t)
            assert np.array_equal(trunc.cpu().numpy(), want_trunc), (name, "truncated", t)
            n_done += int(d.sum())
        assert np.array_equal(crc_rows(env._obs.cpu().numpy()), g("obs_crc")[t]), (name, "observation", t)
        assert bb.state_tag(_states(env), cfg["rules"]) == g("state_tag")[t], (name, "state", t)
    assert n_done == int(g("done").sum())
    _finish(name, env)


# ------------------------------------------------------------------------------------------ launch tuning
@pytest.mark.parametrize("epb", range(1, 9))
@pytest.mark.parametrize("band,name", sorted(bb.step_bands().items()))
def test_launch_tuning_is_invisible(band, name, epb):
    """One random run per per-step band (8, 4, 2, 1 envs per workgroup by default) with every envs_per_block from 1 to 8
    and both record policies: the fixture's results, so identical ones.  A value above what LDS allows is lowered to it."""
    cfg = RUNS[name]
    for record in ("full", "short"):
        env = _mk(cfg, envs_per_block=epb, record_policy=record)
        assert _launch_shape(env)[0] == min(epb, band)
        _play_steps(name, env, every_state=False)
        _finish(name, env)
