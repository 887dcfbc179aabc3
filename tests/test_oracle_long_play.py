"""The CPU oracle against the reference on long scripted play (tests/golden/long_play.npz).

Every other fixture drives the envs with random or eps-greedy actions, under which an episode lasts a few dozen steps.
Here the reference itself played under the scripted policies of tests/scripted_play.py for thousands of steps: full
boards, bodies over 64 cells, episodes cut by the 2000-step cap, an adversarial fruit list of 67 entries, new_world
envs that play on to the cap after the main snake's death.  The oracle replays the recorded actions and must agree
bit for bit on every step: reward, done, num_snakes, episode return / length, and (through the running BLAKE2b of
golden_util.feed_step) every observation byte and every canonical state.

What each run is there for is asserted from the fixture's own recorded data (the reference's body lengths and fruit
counts), so a regenerated fixture that lost its point fails here.  The reference has no truncation flag: that stays
pinned by the truth table in tests/test_oracle_reset_envs.py.
"""
import hashlib
import json
import os

import numpy as np
import pytest

import scripted_play as sp
from golden_util import GOLDEN, feed_step

PATH = os.path.join(GOLDEN, "long_play.npz")


def _load():
    z = np.load(PATH)
    return json.loads(str(z["meta"]))["runs"], z


def _run_names():
    return list(_load()[0])


def test_fixture_holds_the_runs_the_suite_relies_on():
    """The file is the one tools/gen_golden.py writes from scripted_play.FIXTURE_RUNS, and together the runs cover:
    snake_env boards that fill (6x6, 10x10), a snake_env run into the cap with a body over 64, a 2-snake run, an
    adversarial board that fills, a 3-snake adversarial run under safe greedy, new_world episodes ended by the cap."""
    runs, z = _load()
    assert runs == sp.FIXTURE_RUNS
    assert os.path.getsize(PATH) < os.path.getsize(os.path.join(GOLDEN, "tape_S_19x19_3.npz"))
    has = lambda rules, ns, dim, flag: any(c["rules"] == rules and c["n_snakes"] == ns and (dim is None or c["dim"] == dim)
                                           and flag in c["expect"] for c in runs.values())
    assert has(0, 1, 6, "full") and has(0, 1, 10, "full")
    assert any(c["rules"] == 0 and {"capped", "over64"} <= set(c["expect"]) for c in runs.values())
    assert has(0, 2, None, "full")
    assert has(2, 1, None, "full")
    assert any(c["rules"] == 2 and c["n_snakes"] == 3 and c["policy"] == "safe_greedy" for c in runs.values())
    assert has(1, 2, None, "capped")
    assert max(c["steps"] for c in runs.values()) > 2000


@pytest.mark.parametrize("name", _run_names())
def test_coverage_of_the_recorded_run(name):
    """Board full, capped, body over 64, fruit list over 64: whichever this run is there for, read from what the
    reference recorded."""
    runs, z = _load()
    cfg = runs[name]
    assert cfg["expect"]
    cov = sp.coverage(cfg, z[name + "_body_max"], z[name + "_n_fruits"], z[name + "_done"], z[name + "_ep_len"])
    sp.check_coverage(cfg, cov)
    if "capped" in cfg["expect"] and cfg["rules"] == 1:  # new_world: the capped episodes are the ones after the main
        d = z[name + "_done"].astype(bool)               # snake's death (done stays 0 from then on)
        t, e = np.nonzero(d & (z[name + "_ep_len"] == cfg["max_steps"]))
        assert all(ti >= 1999 and not d[ti - 1999:ti, ei].any() for ti, ei in zip(t, e))


@pytest.mark.parametrize("name", _run_names())
def test_oracle_replays_the_reference(name):
    runs, z = _load()
    cfg = runs[name]
    rules, T = cfg["rules"], cfg["steps"]
    g = lambda k: z[f"{name}_{k}"]
    o = sp.make_oracle(cfg)
    read = sp._StateReader(o)
    states = lambda: [read(e) for e in range(cfg["num_envs"])]
    h = hashlib.blake2b(digest_size=32)
    obs = o.reset()
    assert feed_step(h, obs, states(), rules) == g("reset_tag")[0], name
    actions = g("actions").astype(np.int32)
    rs = sp.policy_rng(cfg)
    st = states()
    for t in range(T):
        # the scripted policy on the oracle's state chooses what it chose on the reference's
        assert np.array_equal(sp.choose_actions(cfg, st, rs), actions[t]), (name, t)
        obs, rew, done, ns, epr, epl = o.step(actions[t])
        assert np.array_equal(rew, g("reward")[t]), (name, t)
        assert np.array_equal(done, g("done")[t]), (name, t)
        assert np.array_equal(ns, g("num_snakes")[t].astype(np.int32)), (name, t)
        assert np.array_equal(epr, g("ep_return")[t]), (name, t)
        assert np.array_equal(epl, g("ep_len")[t].astype(np.int32)), (name, t)
        st = states()
        assert [max(len(b) for b in s["snakes"]) for s in st] == g("body_max")[t].tolist(), (name, t)
        assert [len(s["fruits"]) for s in st] == g("n_fruits")[t].tolist(), (name, t)
        assert feed_step(h, obs, st, rules) == g("tag")[t], (name, t)
    assert np.array_equal(np.frombuffer(h.digest(), np.uint8), g("digest")), name


def test_recorder_is_deterministic_and_matches_the_fixture():
    """scripted_play.record() (what the GPU tests replay) on a fixture run gives the fixture's actions and scalars."""
    runs, z = _load()
    cfg = runs["S6x2"]
    a, b = sp.record(cfg), sp.record(cfg)
    for k in ("actions", "reward", "done", "num_snakes", "ep_return", "ep_len", "obs_crc", "body_max", "n_fruits", "ctr"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("actions", "reward", "done", "num_snakes", "ep_return", "ep_len", "body_max", "n_fruits"):
        assert np.array_equal(a[k], z["S6x2_" + k].astype(a[k].dtype)), k
    assert a["coverage"] == b["coverage"] and sorted(a["states"]) == sorted(b["states"])
    # without auto reset and with reset_envs(done) after every step the play is the same, plus terminal rows and flags
    c = sp.record(cfg, auto_reset=False)
    for k in ("actions", "reward", "done", "num_snakes", "ep_return", "ep_len", "obs_crc"):
        assert np.array_equal(a[k], c[k]), k
    d = c["done"].astype(bool)
    assert (c["final_crc"][d] != 0).all() and (c["final_crc"][~d] == 0).all()
    assert not c["truncated"].any()  # every 6x6 episode ends by death, long before the cap
