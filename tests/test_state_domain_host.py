"""The acceptance domain of msnake_set_state as tests/state_domain.py states it, checked against the oracle alone: every
state the model accepts imports into the oracle and comes back word for word, and every scenario that
tests/test_state_domain_gpu.py steps from does in the oracle what it is there for.  No GPU, no library under test.
"""
import numpy as np
import pytest

import scripted_play as sp
import state_domain as sd

KEYS = sorted(sd.TABLE_KEYS)
N, VICTIM = 10, 4


def test_capacities_follow_the_configuration():
    got = {k: (sd.cap(c), sd.fcap(c)) for k, c in sd.CFGS.items()}
    assert got == {"S5": (64, 128), "N6": (128, 192), "A5": (64, 128), "S10": (128, 320), "A10": (128, 320), "S19": (384, 1152)}
    for c in sd.CFGS.values():
        assert sd.cap(c) == sp.ring_cap(dict(c, rules=sd.RULES[c["rules"]]))
    # new_world's body capacity follows the episode cap once that passes the board
    assert sd.cap(dict(sd.CFGS["N6"], max_steps=36)) == 64 and sd.cap(dict(sd.CFGS["N6"], max_steps=63)) == 128


@pytest.mark.parametrize("key", KEYS)
def test_the_model_gives_every_row_its_reason(key):
    names = [name for name, _, _ in sd.rows(key)]
    assert len(set(names)) == len(names)
    for name, build, expect in sd.rows(key):
        assert sd.accepts(sd.CFGS[key], build()) == expect, name


def test_every_rule_set_has_every_reason_next_to_an_accepted_row():
    for rules in sd.RULES:
        table = [(name, expect) for k in KEYS if sd.CFGS[k]["rules"] == rules for name, _, expect in sd.rows(k)]
        for reason in sd.REASON_RE:
            assert any(e == reason for _, e in table), (rules, reason)
        assert sum(e is None for _, e in table) >= 20, rules
        names = {name for name, _ in table}
        # the boundary pairs: the refused value and the accepted one next to it are both in the table
        for bad, good in (("t = -1", "t = 0"), ("spare_fruits = -1", "spare_fruits = 0"), ("ep_len = -1", "ep_len = 0"),
                          ("grow_to = -1", "grow_to = 0"), ("len cap - 1", "len cap - 2"), ("len -1", "len 0"),
                          ("head at c0 = -2", "head at c0 = -1"), ("head at c1 = dim + 1", "head at c1 = dim"),
                          ("velocity (1, 1)", "velocity (1, 0)"), ("velocity (2, 0)", "velocity (1, 0)"),
                          ("stray bit 0x200", "finished bit"), ("piece 64 of 70 at c0 = -1", "body of 70")):
            assert bad in names and good in names, (rules, bad, good)
        if rules == "adversarial":
            assert {"list of fcap", "list of fcap + 1", "list of -1", "list empty", "list entry at c0 = -2",
                    "list entry at c0 = -1"} <= names


@pytest.mark.parametrize("key", KEYS)
def test_accepted_rows_import_into_the_oracle_and_come_back(key):
    cfg = sd.CFGS[key]
    ora = sd.make_oracle(cfg, 2)
    ora.reset()
    n_accepted = 0
    for name, build, expect in sd.rows(key):
        if expect is not None:
            continue
        w = build()
        assert sd.imports(ora, 1, w) == 0, name
        back = sd.export(ora, 1, finished_bit=False)
        want = w[:sd.canonical_len(cfg, w)].copy()
        assert bool(want[7] & 0x100) == ora.finished(1), name
        want[7] &= ~0x100
        assert np.array_equal(back, want), name
        n_accepted += 1
    assert n_accepted >= 20


# ------------------------------------------------------------------------------------------ the steps after
def play(key, words, action_rows):
    """The oracle alone: `words` installed in env VICTIM of N envs fresh from a reset, one step per action row (the
    other envs rest).  Returns the victim's words after every step."""
    cfg = sd.CFGS[key]
    assert sd.accepts(cfg, words) is None
    ora = sd.make_oracle(cfg, N)
    ora.reset()
    assert sd.imports(ora, VICTIM, words) == 0
    out = []
    for row in action_rows:
        act = np.zeros((N, cfg["n_snakes"]), np.int32)
        act[VICTIM] = row
        ora.step(act)
        out.append(sd.St(sd.export(ora, VICTIM)))
    return out


def test_adversarial_list_ends_exactly_full_and_over():
    F = sd.fcap(sd.CFGS["A5"])
    for over in (0, 3):
        words, act, dying, steps = sd.adv_wall(over)
        assert int(words[6]) + dying == F + over
        st0 = sd.St(words)
        assert sum(len(sn["cells"]) for sn in st0.snakes) <= F and VICTIM < N - 2
        after = play("A5", words, [act] * steps)[-1]
        assert len(after.fruits) == F + over
        assert [len(sn["cells"]) for sn in after.snakes] == [2, 0, 0]            # the main snake lives: no reset
        assert after.hdr[3] == 5 - 2 + 2 * 25                                   # spare_fruits: two eaten, += len^2 twice
        assert after.fruits[:2] == [[5, 2], [5, 4]]                             # the eaten entries stayed
        assert after.fruits[-5:] == [[5, 4], [4, 4], [3, 4], [2, 4], [1, 4]]    # the last body, head first


def test_adversarial_neighbour_keeps_a_full_list():
    words = sd.adv_full_neighbour()
    assert int(words[6]) == sd.fcap(sd.CFGS["A5"])
    before = sd.St(words)
    for after in play("A5", words, [[0, 0, 0]] * 2):
        assert after.fruits == before.fruits and [sn["cells"] for sn in after.snakes] == [sn["cells"] for sn in before.snakes]


def test_growth_after_the_install_overflows_the_list():
    F = sd.fcap(sd.CFGS["A5"])
    words, act, lengths = sd.adv_growth()
    st0 = sd.St(words)
    assert int(words[6]) + sum(len(sn["cells"]) for sn in st0.snakes) == F and st0.hdr[3] > 0
    steps = play("A5", words, [act] * len(lengths))
    assert [len(st.fruits) for st in steps] == lengths and lengths[-1] == F + 3 and max(lengths[:-1]) < F
    assert steps[0].fruits == st0.fruits and steps[0].hdr[3] == 0               # both eaten entries stayed where they were
    assert [len(sn["cells"]) for sn in steps[1].snakes] == [1, 5, 5]            # grown after the install
    assert [len(sn["cells"]) for sn in steps[-1].snakes] == [1, 0, 0]


@pytest.mark.parametrize("key", ["S5", "A5", "N6"])
@pytest.mark.parametrize("eat", [False, True])
def test_grow_to_limits_scenario(key, eat):
    words, act = sd.grow_limits(key, eat)
    cfg = sd.CFGS[key]
    st0 = sd.St(words)
    first = 1 if cfg["rules"] == "new_world" else 0
    assert st0.snakes[first]["grow"] == 0 and st0.snakes[first + 1]["grow"] == len(st0.snakes[first + 1]["cells"])
    steps = play(key, words, [act] * sd.grow_limits_steps(key))
    assert [st.hdr[0] for st in steps] == [st0.hdr[0] + 1 + i for i in range(len(steps))]      # no reset in between
    one = steps[0]
    eater = one.snakes[first + 2]
    assert eater["grow"] == (5 if eat else 3) and (one.fruits != st0.fruits) == eat
    # grow_to 0 and grow_to == len: the head moves, the length stays (new_world pops once per fruit, down to 3, then adds the head)
    assert len(one.snakes[first]["cells"]) == (4 if cfg["rules"] == "new_world" else 3)
    assert len(one.snakes[first + 1]["cells"]) == 3 and one.snakes[first + 1]["cells"][0] == [2, 2]


@pytest.mark.parametrize("key", ["N6", "S5", "A5"])
def test_a_body_crosses_the_capacity_on_the_second_step(key):
    words, acts, s = sd.body_guard(key)
    C = sd.cap(sd.CFGS[key])
    assert len(sd.St(words).snakes[s]["cells"]) == C - 2 and len(acts) == 7
    steps = play(key, words, acts)
    assert [len(st.snakes[s]["cells"]) for st in steps[:2]] == [C - 1, C]
    assert [st.hdr[0] for st in steps[:2]] == [1, 2]                           # no reset on the way
    if key == "N6":
        assert [len(st.snakes[s]["cells"]) for st in steps] == [C - 1 + i for i in range(7)]     # it goes on growing


@pytest.mark.parametrize("key", ["S19", "S5", "A5", "N6"])
def test_a_head_outside_the_grid_turns_back_in(key):
    words, rows = sd.turn_back(key)
    dim = sd.CFGS[key]["dim"]
    first = 1 if sd.CFGS[key]["rules"] == "new_world" else 0
    steps = play(key, words, rows)
    for t, st in enumerate(steps):
        assert st.hdr[0] == 5 + t + 1                                           # no reset: both snakes live on
        a, c = st.snakes[first]["cells"], st.snakes[first + 1]["cells"]
        assert len(a) == 4 + t and len(c) == 4 + t
        assert a[0] == [t, 3] and a[t + 1] == [-1, 3] and c[0] == [3, dim - 1 - t] and c[t + 1] == [3, dim]
