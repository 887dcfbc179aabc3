"""Why a snake died, host side: tests/causes_play.py against the reference's own recorded bodies
(tests/golden/death_causes.npz), against the oracle's verdict on long scripted play, and on a hand-built table with
literal expectations; the entry point is declared, exported and bound.  Nothing here needs a GPU.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import agents_play as ap
import causes_play as cp
import msnake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "death_causes.npz")
# per rule set of the fixture (tools/gen_causes_golden.py) and per scenario of the oracle play
FIXTURE_FLOORS = dict(deaths=100, wall=10, self=10, head_on=10, body=10, dead_owner=3)
PLAY_FLOORS = dict(wall=50, self=15, head_on=100, body=30, dead_owner=4, last_piece=5)


# ------------------------------------------------------------------------------------------ 1. the reference's bodies
def _fixture_steps(z, run):
    """(dim, rules, [(state before, state after, recorded bodies, cleared)]) of one run of the fixture."""
    rules, dim, S, E, T, _ = z[f"{run}_meta"].tolist()
    get = lambda k: z[f"{run}_{k}"]

    def bodies(kind, t, e):
        n, cells = get(f"{kind}_len")[t, e], get(f"{kind}_cells")[t, e]
        return [[tuple(c) for c in cells[s, :n[s]].tolist()] for s in range(S)]

    steps = []
    for t in range(T):
        for e in range(E):
            st = {k: {"snakes": bodies(k, t, e), "vels": get(f"{k}_vel")[t, e].tolist(), "grow_to": get(f"{k}_grow")[t, e].tolist()}
                  for k in ("before", "after")}
            steps.append((st["before"], st["after"], bodies("post", t, e), get("cleared")[t, e].astype(bool)))
    return dim, rules, steps


def test_post_bodies_equal_the_bodies_the_reference_judged_with():
    z = np.load(FIXTURE)
    runs = sorted(k[:-5] for k in z.files if k.endswith("_meta"))
    assert runs == ["A6", "S10", "S6"]
    per_rules, bodies_seen, died_seen = {}, 0, 0
    for run in runs:
        dim, rules, steps = _fixture_steps(z, run)
        assert (dim, rules) == dict(S6=(6, 0), A6=(6, 2), S10=(10, 0))[run]
        for n, (before, after, post, cleared) in enumerate(steps):
            got = cp.post_bodies(before, after)
            for s in range(3):
                assert (got[s] or []) == post[s], (run, n, s, before, after)
                bodies_seen += bool(post[s])
            cause, by, victims, where = cp.np_causes(before, after, dim)
            assert np.array_equal(cause != 0, cleared), (run, n, cause, cleared)
            died_seen += int(cleared.sum())
            cp.add_events(per_rules.setdefault(rules, {}), cp.events(before, after, dim))
    assert bodies_seen >= 3000 and died_seen >= 600
    for rules, ev in per_rules.items():
        assert all(ev[k] >= v for k, v in FIXTURE_FLOORS.items()), (rules, ev)


def test_fixture_is_small():
    assert os.path.getsize(FIXTURE) <= 100_000


# ------------------------------------------------------------------------------------------ 2. the oracle's verdict
@functools.lru_cache(maxsize=None)
def played(name, steps=200):
    """One play of agents_play.SCENARIOS[name] on the twin: (event counts, violations of cause != 0 <=> DIED)."""
    tw = cp.Twin(dict(ap.SCENARIOS[name], steps=steps))
    total, bad = {}, []
    for t in range(steps):
        tw.step()
        died = (tw.flags & ap.DIED) != 0
        was = (tw.flags & ap.WAS_ALIVE) != 0
        if not np.array_equal(tw.cause != 0, died) or (tw.cause[~was] != 0).any():
            bad.append((t, tw.cause.tolist(), died.tolist()))
        cp.add_events(total, tw.events())
    return total, bad


@pytest.mark.parametrize("name", ["S6", "A6", "S6cap"])
def test_cause_is_set_exactly_where_the_oracle_cleared_a_snake(name):
    ev, bad = played(name)
    assert not bad, bad[:3]
    assert all(ev[k] >= v for k, v in PLAY_FLOORS.items()), (name, ev)


# ------------------------------------------------------------------------------------------ 3. the hand-built table
def _check_table(rules, names):
    names, prev, now = cp.step_table(rules, names)
    for name, p, n in zip(names, prev, now):
        _, _, want_cause, want_by, want_victims, want_where = cp.TABLE[name]
        cause, by, victims, where = cp.np_causes(p, n, 6, rules)
        assert cause.tolist() == list(want_cause), (rules, name, cause)
        assert by.tolist() == list(want_by), (rules, name, by)
        assert victims.tolist() == list(want_victims), (rules, name, victims)
        assert where.tolist() == [list(w) for w in want_where], (rules, name, where)
        assert [len(b) == 0 for b in n["snakes"]] == [c != 0 for c in want_cause], (rules, name, "the oracle's verdict")


def test_table_with_its_literal_values():
    assert list(cp.TABLE) == ["T1", "T2", "T3", "T4", "M1", "M2", "R"]
    _check_table("snake_env", None)
    _check_table("adversarial", cp.TABLE_ADVERSARIAL)


def test_table_t3_eats_while_dying_and_keeps_its_tail():
    _, prev, now = cp.step_table("snake_env", ["T2", "T3"])
    assert now[0]["grow_to"][0] == 3 and now[1]["grow_to"][0] == 5, "the dead snake's grow_to word carries the fruit"
    assert cp.post_bodies(prev[0], now[0])[0] == [(5, 2), (4, 2), (3, 2)]
    assert cp.post_bodies(prev[1], now[1])[0] == [(5, 2), (4, 2), (3, 2), (2, 2)]


# ------------------------------------------------------------------------------------------ 4. new_world
def test_new_world_raises():
    cfg = ap.SCENARIOS["N6"]
    with pytest.raises(ValueError, match="new_world"):
        cp.Twin(cfg)
    st = cp.TABLE["T1"][0]
    with pytest.raises(ValueError, match="new_world"):
        cp.np_causes(st, st, 6, "new_world")


# ------------------------------------------------------------------------------------------ 5. the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_death_causes\(msnake_handle after, msnake_handle before, uint8_t\* cause_dev, uint8_t\* by_dev,\s*"
           r"uint8_t\* victims_dev,\s*int8_t\* where_dev, void\* stream\);")
    assert re.search(sig, text)
    for name, value in (("WALL", cp.WALL), ("SELF", cp.SELF), ("HEAD_ON", cp.HEAD_ON), ("BODY", cp.BODY)):
        m = re.search(rf"#define MSNAKE_CAUSE_{name}\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value == getattr(msnake._capi, f"CAUSE_{name}"), name
    assert (cp.WALL, cp.SELF, cp.HEAD_ON, cp.BODY) == (1, 2, 4, 8)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_death_causes" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_death_causes is not None and lib.msnake_abi_version() == 3
    restype, argtypes = msnake._capi.PROTOTYPES["msnake_death_causes"]
    assert restype is ctypes.c_int and argtypes == [ctypes.c_void_p] * 7
    assert lib.msnake_death_causes(None, None, None, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    assert callable(msnake.MultiSnakeVecEnv.death_causes_device) and msnake.DeathCauses._fields == ("cause", "by", "victims", "where")
