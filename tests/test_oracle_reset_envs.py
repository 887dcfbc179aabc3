"""The oracle's masked reset (orc_reset_envs / Oracle.reset_envs), the CPU reference of msnake_reset_envs, pinned.

* Against what the reference recorded: on every auto-reset tape of tests/golden/ and every auto-reset configuration of
  random_configs.npz, `step` without auto reset followed by `reset_envs(done)` must reproduce the recording exactly
  as test_oracle_golden.test_tape / test_oracle_vs_reference_live check it.  That is the vec layer's contract
  (subproc_vec_env.py:13-16) and include/msnake.h's "step + reset_envs(done) == auto_reset", checked against data
  the reference produced.
* Against the emulation the GPU tests used before this function existed (export the unselected envs' words, reset every
  env, import them again), for random, all-zero, all-one and single-env masks and all three rule sets.
* The truncation flag against a hand-built truth table (see test_truncation_truth_table).
No GPU anywhere in this file."""
import hashlib
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, crc_rows, feed_step, load_tape, state_view, tape_names, unpack_state
from oracle import snake_oracle as so
from reset_emulation import cut_by_time, emulated_masked_reset, raw_words

with np.load(os.path.join(GOLDEN, "random_configs.npz")) as _z:
    META, REC = json.loads(str(_z["meta"])), {k: _z[k] for k in _z.files if k != "meta"}

AUTO_TAPES = [n for n in tape_names() if load_tape(n)[0]["auto_reset"]]
RULESETS = [("snake_env", 10, 3, 3), ("new_world", 10, 3, 5), ("adversarial", 10, 3, 3)]
SENTINEL = 0xA5


def test_every_auto_reset_tape_is_covered():
    assert len(AUTO_TAPES) == 16
    assert {load_tape(n)[0]["rules"] for n in AUTO_TAPES} == {0, 1, 2}


@pytest.mark.parametrize("name", AUTO_TAPES)
def test_tape_through_step_and_reset_envs(name):
    meta, z = load_tape(name)
    rules, E, T = meta["rules"], meta["num_envs"], meta["steps"]
    o = so.Oracle(E, dim=meta["dim"], n_snakes=meta["n_snakes"], n_fruits=meta["n_fruits"], rules=rules,
                  seed=meta["seed"], env_id_base=meta["env_id_base"], max_steps=meta["max_steps"], auto_reset=False)
    assert np.array_equal(o.reset(), z["obs0"])
    full_t = {int(t): i for i, t in enumerate(z["full_obs_t"])}
    actions = z["actions"].astype(np.int32)
    n_done = 0
    for t in range(T):
        obs, rew, done, ns, epr, epl = o.step(actions[t])
        assert all(o.finished(e) == bool(done[e]) for e in range(E)), (name, t)
        terminal = obs.copy()
        o.reset_envs(done)  # (into o.obs: the rows of the done envs become their reset observations)
        assert not any(o.finished(e) for e in range(E)), (name, t)
        assert np.array_equal(o.final_obs[done != 0], terminal[done != 0]), (name, t)
        assert not o.truncated.any(), (name, t)  # every tape has max_steps = 2000: nothing is ever cut by the cap
        assert np.array_equal(rew, z["reward"][t]), (name, t)
        assert np.array_equal(done, z["done"][t]), (name, t)
        assert np.array_equal(ns, z["num_snakes"][t].astype(np.int32)), (name, t)
        assert np.array_equal(epr, z["ep_return"][t]), (name, t)
        assert np.array_equal(epl, z["ep_len"][t]), (name, t)
        assert np.array_equal(crc_rows(obs), z["obs_crc"][t]), (name, t)
        if t in full_t:
            assert np.array_equal(obs, z["full_obs"][full_t[t]]), (name, t)
        if t % 8 == 0 or t == T - 1:
            for e in range(E):
                assert state_view(o.get_state(e), rules) == unpack_state(z, "st_", t, e, rules), (name, t, e)
        n_done += int(done.sum())
    assert n_done > 0, "a tape without a single reset pins nothing here"


AUTO_CONFIGS = [(i, c) for i, c in enumerate(META["configs"]) if c["auto_reset"]]


def test_auto_reset_configurations_exist_for_every_rule_set():
    assert len(AUTO_CONFIGS) >= 30 and {c["rules"] for _, c in AUTO_CONFIGS} == {0, 1, 2}


@pytest.mark.parametrize("case", AUTO_CONFIGS,
                         ids=lambda ic: f"{['S', 'N', 'A'][ic[1]['rules']]}-{ic[1]['dim']}x{ic[1]['n_snakes']}x"
                                        f"{ic[1]['n_fruits']}-eps{ic[1]['eps']}")
def test_random_configuration_through_step_and_reset_envs(case):
    i, cfg = case
    ref = {k: v[i] for k, v in REC.items()}
    rules, E, ns = cfg["rules"], cfg["num_envs"], cfg["n_snakes"]
    ora = so.Oracle(E, dim=cfg["dim"], n_snakes=ns, n_fruits=cfg["n_fruits"], rules=rules, seed=cfg["seed"],
                    env_id_base=cfg["env_id_base"], auto_reset=False)
    h = hashlib.blake2b(digest_size=32)
    states = lambda: [ora.get_state(e) for e in range(E)]  # noqa: E731
    assert feed_step(h, ora.reset(), states(), rules) == ref["reset_tag"][0], "reset observation or state"
    for t in range(META["steps"]):
        o_obs, o_rew, o_done, o_ns, o_er, o_el = ora.step(ref["actions"][t, :E, :ns].astype(np.int32))
        ora.reset_envs(o_done, final_obs=None, truncated=None)
        assert np.array_equal(o_rew, ref["reward"][t, :E]) and np.array_equal(o_done, ref["done"][t, :E]), t
        assert np.array_equal(o_ns, ref["num_snakes"][t, :E]) and np.array_equal(o_er, ref["ep_return"][t, :E]), t
        assert np.array_equal(o_el, ref["ep_len"][t, :E]), t
        assert feed_step(h, o_obs, states(), rules) == ref["tag"][t], f"observation or state differs at step {t}"
    assert not ref["reset_tag"][1:].any()
    assert h.digest() == ref["digest"].tobytes(), "observations or states differ from the reference's"


# ---------------------------------------------------------------------------------- against the export / import emulation
@pytest.mark.parametrize("rules,dim,ns,nf", RULESETS)
def test_reset_envs_equals_the_export_import_emulation(rules, dim, ns, nf):
    n, max_steps = 48, 9
    kw = dict(dim=dim, n_snakes=ns, n_fruits=nf, rules=rules, seed=23, env_id_base=5000, max_steps=max_steps, auto_reset=False)
    a, b = so.Oracle(n, **kw), so.Oracle(n, **kw)
    assert np.array_equal(a.reset(), b.reset())
    rs = np.random.default_rng(77)
    finished = np.zeros(n, bool)  # the emulation's side of the vec-layer bit
    one = np.zeros(n, bool)
    one[n - 1] = True
    masks = [np.zeros(n, bool), np.ones(n, bool), one] + [rs.random(n) < p for p in (0.1, 0.3, 0.5, 0.7, 0.9)] * 3
    n_cut = n_mid = n_ended = 0
    for i, mask in enumerate(masks):
        for _ in range(int(rs.integers(1, 6))):
            act = rs.integers(0, 5, (n, ns)).astype(np.int32)
            ra = [x.copy() for x in a.step(act)]
            rb = [x.copy() for x in b.step(act)]
            assert all(np.array_equal(x, y) for x, y in zip(ra, rb))
            finished |= ra[2] != 0
        assert [a.finished(e) for e in range(n)] == list(finished), i
        if 0 < i and not (mask.all() or mask.sum() <= 1):
            assert 0.05 * n <= mask.sum() <= 0.95 * n
        before = [raw_words(a, e) for e in range(n)]
        final_want = a.render().copy()
        want_trunc = np.array([mask[e] and finished[e] and cut_by_time(before[e], rules, max_steps) for e in range(n)], np.uint8)
        obs = np.full((n,) + a.obs_shape, SENTINEL, np.uint8)
        final = np.full((n,) + a.obs_shape, SENTINEL, np.uint8)
        trunc = np.full(n, SENTINEL, np.uint8)
        # (the selection as arbitrary non-zero bytes: 1, 2, 0x80, 0xFF)
        a.reset_envs(np.where(mask, np.array([1, 2, 0x80, 0xFF], np.uint8)[np.arange(n) % 4], 0).astype(np.uint8),
                     obs=obs, final_obs=final, truncated=trunc)
        want = emulated_masked_reset(b, mask)
        assert np.array_equal(obs[mask], want[mask]) and np.array_equal(final[mask], final_want[mask]), i
        assert (obs[~mask] == SENTINEL).all() and (final[~mask] == SENTINEL).all(), i
        assert np.array_equal(trunc, want_trunc), i
        for e in range(n):
            assert np.array_equal(raw_words(a, e), raw_words(b, e)), (i, e)
            if not mask[e]:
                assert np.array_equal(raw_words(a, e), before[e]), (i, e)
            assert a.finished(e) == bool(finished[e] and not mask[e]), (i, e)
        assert np.array_equal(a.render(), want), i
        n_cut += int(want_trunc.sum())
        n_ended += int((mask & finished).sum()) - int(want_trunc.sum())
        n_mid += int((mask & ~finished).sum())
        finished &= ~mask
    assert n_cut > 0 and n_ended > 0 and n_mid > 0, (n_cut, n_ended, n_mid)


def test_reset_envs_without_the_optional_pointers():
    n, ns = 24, 3
    kw = dict(dim=10, n_snakes=ns, rules="snake_env", seed=4, max_steps=7, auto_reset=False)
    a, b = so.Oracle(n, **kw), so.Oracle(n, **kw)
    a.reset(); b.reset()
    rs = np.random.default_rng(2)
    for t in range(40):
        act = rs.integers(0, 5, (n, ns)).astype(np.int32)
        done = a.step(act)[2].copy()
        b.step(act)
        assert a.reset_envs(done, obs=None, final_obs=None, truncated=None) == (None, None, None)
        b.reset_envs(done)
        assert np.array_equal(a.render(), b.render()), t
        for e in range(n):
            assert np.array_equal(raw_words(a, e), raw_words(b, e)), (t, e)


# ---------------------------------------------------------------------------------- the truncation flag
def _table_state(rules, ns, t, main_ended, finished):
    """A legal state with the given clock, the rule set's own end condition of the main snake and the vec-layer bit."""
    bodies = [[[2 + s, 1], [2 + s, 2]] for s in range(ns)]
    alive = [True] * ns
    if rules == "new_world":
        alive[0] = main_ended  # [N]: the episode ends while snakes[0].alive (the reference's inverted done)
        if not main_ended:
            bodies[0] = []  # (a dead [N] snake may keep its body or not; the flag looks at the alive bit alone)
    elif main_ended:
        bodies[0] = []  # [S]/[A]: a dead snake's body is cleared
    return {"snakes": bodies, "fruits": [[6, 6 + s % 2] for s in range(ns)], "vels": [[0, 1]] * ns, "grow_to": [3] * ns, "t": t,
            "ctr": 40, "alive": alive, "in_dead": [not x for x in alive], "spare_fruits": 0, "ep_len": t,
            "ep_return": -1.0 if main_ended else 0.0, "finished": finished}


@pytest.mark.parametrize("rules", ["snake_env", "new_world", "adversarial"])
def test_truncation_truth_table(rules):
    """No committed fixture holds a truncated episode: every tape was recorded with max_steps = 2000 and none runs that
    long, and the reference has no notion of truncation at all (its step folds the cap into `done`).  So this table,
    built by hand from the text of include/msnake.h -- selected AND ended-and-not-reset-since AND t >= max_steps AND
    NOT the rule set's own end condition -- is, with that text, the only truth there is for the flag."""
    ns, M = 2, 10
    #        t      main_ended finished selected -> truncated
    rows = [(M,     False,     True,    True,    1),   # ended by the cap only
            (M + 3, False,     True,    True,    1),   # ... and stepped on after it ended (auto reset is off)
            (M - 4, True,      True,    True,    0),   # ended by the rules before the cap
            (M,     True,      True,    True,    0),   # the rules ended it exactly at the cap: not truncated
            (M - 4, False,     False,   True,    0),   # not ended (abandoned mid-episode)
            (M,     False,     False,   True,    0),   # at the cap on the clock, but no episode end was seen since the last reset
            (M,     False,     True,    False,   0),   # ended by the cap, not selected
            (M - 4, True,      True,    False,   0)]   # ended by the rules, not selected
    o = so.Oracle(len(rows), dim=10, n_snakes=ns, rules=rules, seed=3, max_steps=M, auto_reset=False)
    o.reset()
    for e, (t, ended, finished, _, _) in enumerate(rows):
        o.set_state(e, _table_state(rules, ns, t, ended, finished))
        assert o.finished(e) == finished
    before = [raw_words(o, e) for e in range(len(rows))]
    mask = np.array([r[3] for r in rows])
    _, _, trunc = o.reset_envs(mask)
    assert list(trunc) == [r[4] for r in rows]
    for e, sel in enumerate(mask):
        if sel:
            st = o.get_state(e)
            assert st["t"] == 0 and st["ep_len"] == 0 and st["ep_return"] == 0.0 and not o.finished(e)
        else:
            assert np.array_equal(raw_words(o, e), before[e]) and o.finished(e) == rows[e][2]
    # a second masked reset, of every env: the selected ones hold no finished episode any more, the two left out do
    assert list(o.reset_envs(np.ones(len(rows), bool))[2]) == [0, 0, 0, 0, 0, 0, 1, 0]


@pytest.mark.parametrize("rules", ["snake_env", "new_world", "adversarial"])
def test_truncation_of_played_episodes(rules):
    """The same through play: action 0 on a fresh env moves nothing (velocity (0, 0)), so [S]/[A] episodes run into the
    cap and are truncated; an [N] env that is reset whenever it is done never gets near the cap and never is (its episodes
    end by its own, inverted, rule: while the main snake is alive)."""
    n, ns, M = 4, 2, 6
    o = so.Oracle(n, dim=10, n_snakes=ns, rules=rules, seed=12, max_steps=M, auto_reset=False)
    o.reset()
    stay = np.full((n, ns), 1 if rules == "new_world" else 0, np.int32)  # ([N] piles a standing head onto itself: move)
    n_done = 0
    for t in range(1, M + 1):
        done = o.step(stay)[2].copy()
        sel = np.array([1, 0, 1, 0], np.uint8)
        trunc = o.reset_envs(done * sel)[2]
        if rules == "new_world":
            assert not trunc.any(), t
            n_done += int((done * sel).sum())
        else:
            assert done.all() == (t == M) and list(trunc) == ([1, 0, 1, 0] if t == M else [0] * n), t
    if rules == "new_world":
        assert n_done >= M
    else:
        assert [o.finished(e) for e in range(n)] == [False, True, False, True]
        o.step(stay)  # the unselected ones stay finished, and are cut by the cap when they are reset at last
        assert list(o.reset_envs(np.ones(n, bool))[2]) == [0, 1, 0, 1]
