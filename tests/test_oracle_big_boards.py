"""The CPU oracle against the reference at the top of the ranges (tests/golden/big_boards.npz, tests/big_boards.py).

Every other fixture stops at 23x23 boards and 9 fruits; the header promises dim up to 62 and 32 new_world fruits, and
what the GPU tests check above 23x23 compares the kernels with the oracle alone.  Here the reference itself played 37
runs: random play on both sides of every board size at which a step kernel changes its envs per workgroup (up to 62x62,
all three rule sets, 0 to 32 fruits, 1 to 4 snakes), and late-game states installed into it -- bodies of 63 to 3842
pieces along the Hamiltonian cycle, a 62x62 board that fills, adversarial fruit lists of over 3000 entries, new_world
bodies past 128 pieces.  The oracle replays the recorded actions and must agree on every step: the scalars, and through
the running BLAKE2b of golden_util.feed_step every observation byte and every canonical state.

What each run is there for is asserted from the fixture's own arrays, and the LDS arithmetic that chose the board sizes
is asserted against the library's host glue (msnake_launch_shape_for_config), for every dim.  No GPU in this file.
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import big_boards as bb
import scripted_play as sp
from golden_util import GOLDEN, crc_rows, feed_step

PATH = os.path.join(GOLDEN, "big_boards.npz")

with np.load(PATH) as _z:
    RUNS, REC = json.loads(str(_z["meta"]))["runs"], {k: _z[k] for k in _z.files if k != "meta"}


def _g(name):
    return lambda k: REC[f"{name}_{k}"]


def _cov(name):
    g = _g(name)
    return bb.coverage(RUNS[name], g("reward"), g("done"), g("body_max"), g("n_fruits"))


# ------------------------------------------------------------------------------------------ the fixture itself
def test_fixture_is_the_table_and_small_enough():
    """The file is the one tools/gen_golden.py writes from big_boards.RUNS, no larger than the largest fixture there was."""
    assert RUNS == bb.RUNS
    assert os.path.getsize(PATH) <= os.path.getsize(os.path.join(GOLDEN, "tape_S_19x19_3.npz")) == 294495


def test_coverage_of_the_table():
    """All three rule sets, both sides of every envs-per-workgroup boundary of both kernels for 9 and 12 channels, the
    required dims, fruit and snake counts; 64, 128 and 192 pieces crossed; a 62x62 board filled."""
    bb.check_table_coverage({name: _cov(name) for name in RUNS})


@pytest.mark.parametrize("name", list(bb.RUNS))
def test_coverage_of_the_recorded_run(name):
    """Random snake_env / adversarial: >= 3 fruits eaten by snake 0 and >= 1 episode end; random new_world with fruits:
    >= 3 steps on which the longest body grew; late game: every installed length exceeded by >= 2; adversarial late
    game: the fruit list passes 1000 entries (the reference reached 3003 and 3402) and a body grows from it afterwards."""
    bb.check_coverage(RUNS[name], _cov(name))


def test_the_bands_are_where_the_table_says():
    """The board sizes of the table, from the plain formula: per-step and persistent tape kernel, 9 and 12 channels."""
    band = lambda C, tape: [(d, bb.envs_per_workgroup(d, C, tape)) for d in range(2, 63)  # noqa: E731
                            if d == 2 or bb.envs_per_workgroup(d, C, tape) != bb.envs_per_workgroup(d - 1, C, tape)]
    assert band(9, False) == [(2, 8), (27, 4), (38, 2), (56, 1)]
    assert band(9, True) == [(2, 8), (17, 4), (27, 2), (40, 1), (57, 0)]
    assert band(12, False) == [(2, 8), (23, 4), (33, 2), (48, 1)]
    assert band(12, True) == [(2, 8), (14, 4), (23, 2), (34, 1), (49, 0)]
    assert bb.step_bands() == {1: "S62x3", 2: "A47x3", 4: "S37x3", 8: "S16x3"}


@pytest.mark.parametrize("rules,ns", [("snake_env", 3), ("adversarial", 1), ("new_world", 3), ("new_world", 4), ("new_world", 2),
                                      ("new_world", 1)])
def test_the_library_decides_by_the_same_formula(rules, ns):
    """msnake_launch_shape_for_config (the host glue of msnake_create and msnake_rollout_tape, no GPU) against the plain
    formula for every dim 2..62: envs per workgroup of the per-step launches and of the persistent tape launch, 0 = the
    tape call runs per-step launches -- from dim 57 with 9 channels, from dim 49 with 12, never with 3 or 6."""
    import msnake
    C = msnake._capi
    ch = 3 * ns if rules == "new_world" else 9
    none = []
    for dim in range(2, 63):
        for n, asked in ((3, 0), (4096, 0), (8193, 0), (37, 2), (37, 1)):
            cfg = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, n, dim, ns, ns, C.RULES[rules], 2000, 1, 1, 0, 0, asked, 0, 0, 0)
            want = bb.envs_per_workgroup(dim, ch, False, start=8 if n <= 8192 else 4)
            want = min(want, asked) if asked else want
            want_tape = bb.envs_per_workgroup(dim, ch, True, start=want)
            assert C.launch_shape_for_config(cfg) == (want, want_tape), (dim, n, asked)
        if want_tape == 0:
            none.append(dim)
    assert none == {9: list(range(57, 63)), 12: list(range(49, 63))}.get(ch, [])
    # a fused frame keeps no second image: the tape launch is the per-step launch's
    for dim, scale in ((19, 4), (10, 7)):
        cfg = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, 64, dim, ns, ns, C.RULES[rules], 2000, 1, scale, 0, 0, 0, 0, 0, 0)
        step, tape = C.launch_shape_for_config(cfg)
        assert step == tape >= 1
    bad = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, 64, 63, ns, ns, C.RULES[rules], 2000, 1, 1, 0, 0, 0, 0, 0, 0)
    assert C.load().msnake_launch_shape_for_config(ctypes.byref(bad), None, None) == -1
    assert C.load().msnake_launch_shape_for_config(None, None, None) == -1


# ------------------------------------------------------------------------------------------ the oracle against it
def start(cfg, ora):
    """The oracle at the start of a run: reset, and for a late-game run the installed states.  Returns the observation."""
    obs = ora.reset()
    if cfg["kind"] == "late":
        for e, st in enumerate(bb.start_states(cfg)):
            ora.set_state(e, st)
        obs = ora.render()
    return obs


def _replay(name, masked_reset):
    cfg, g = RUNS[name], _g(name)
    rules, E, T = cfg["rules"], cfg["num_envs"], cfg["steps"]
    o = sp.make_oracle(cfg, auto_reset=cfg["auto_reset"] and not masked_reset)
    read = sp._StateReader(o)
    states = lambda: [read(e) for e in range(E)]  # noqa: E731
    h = hashlib.blake2b(digest_size=32)

    def at_reset(k, obs):
        st = states()
        assert np.array_equal(crc_rows(obs), g("reset_crc")[k]), (name, "reset", k)
        assert bb.state_tag(st, rules) == g("reset_state_tag")[k], (name, "reset", k)
        assert feed_step(h, obs, st, rules) == g("reset_tag")[k], (name, "reset", k)
        return st
    st = at_reset(0, start(cfg, o))
    actions, resets = g("actions").astype(np.int32), bb.hand_resets(cfg)
    for t in range(T):
        if cfg["kind"] == "late":   # the scripted policy on the oracle's state chooses what it chose on the reference's
            assert np.array_equal(bb.late_actions(cfg, st, t), actions[t]), (name, t)
        obs, rew, done, ns, epr, epl = o.step(actions[t])
        if masked_reset:
            o.reset_envs(done, final_obs=None, truncated=None)
        assert np.array_equal(rew, g("reward")[t]), (name, t)
        assert np.array_equal(done, g("done")[t]), (name, t)
        assert np.array_equal(ns, g("num_snakes")[t].astype(np.int32)), (name, t)
        assert np.array_equal(epr, g("ep_return")[t]), (name, t)
        assert np.array_equal(epl, g("ep_len")[t].astype(np.int32)), (name, t)
        st = states()
        assert [max(len(b) for b in s["snakes"]) for s in st] == g("body_max")[t].tolist(), (name, t)
        assert [len(s["fruits"]) for s in st] == g("n_fruits")[t].tolist(), (name, t)
        assert np.array_equal(crc_rows(obs), g("obs_crc")[t]), (name, t)
        assert bb.state_tag(st, rules) == g("state_tag")[t], (name, t)
        assert feed_step(h, obs, st, rules) == g("tag")[t], (name, t)
        if t in resets:
            st = at_reset(1 + resets.index(t), o.reset())
    assert np.array_equal(np.frombuffer(h.digest(), np.uint8), g("digest")), name


@pytest.mark.parametrize("name", list(bb.RUNS))
def test_oracle_replays_the_reference(name):
    _replay(name, masked_reset=False)


@pytest.mark.parametrize("name", [n for n, c in bb.RUNS.items() if c["auto_reset"]])
def test_oracle_through_step_and_reset_envs(name):
    """The auto_reset runs once more: step without auto reset, then reset_envs(done) -- the vec layer's contract."""
    _replay(name, masked_reset=True)
