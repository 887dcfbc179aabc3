"""Why a snake died and on whose body, stated on canonical state dicts (Oracle.get_state): include/msnake.h,
msnake_death_causes, restated without the library.

snake_env and adversarial move every snake, judge every snake against the same post-move bodies and then clear the dead
ones; a cleared snake keeps its velocity and grow_to words.  post_bodies rebuilds those bodies from the states before and
after a step, np_causes compares every head with them.  Twin adds both to agents_play.Twin's prev / now.  new_world judges
its snakes one after the other and is refused.  Nothing here asks the library under test.

A plain helper module in the style of agents_play, which it imports and does not edit; imported by
tests/test_causes_host.py and tests/test_causes_gpu.py.  `python tests/causes_play.py` prints the share of deaths by
cause under three scripted policies, from the CPU oracle (the table of the README).
"""
import numpy as np

import agents_play as ap
import scripted_play as sp
import timed_play as tp

WALL, SELF, HEAD_ON, BODY = 1, 2, 4, 8   # MSNAKE_CAUSE_*
NOWHERE = -2
NEW_WORLD = sp.RULES["new_world"]


def _refuse_new_world(rules):
    if rules is not None and ap._rules(rules) == NEW_WORLD:
        raise ValueError("new_world judges its snakes one after the other and clears bodies as it goes: the bodies a snake "
                         "was judged against cannot be rebuilt from two states")


def post_bodies(prev, now):
    """The post-move, pre-removal body of every snake of one env, head first, as lists of (c0, c1); None for a snake
    that had no body before the step."""
    out = []
    for k, before in enumerate(prev["snakes"]):
        before = [tuple(c) for c in before]
        after = [tuple(c) for c in now["snakes"][k]]
        if not before:
            out.append(None)
        elif after:
            out.append(after)
        else:
            v = tuple(now["vels"][k])
            if v == (0, 0):
                out.append(before)
            else:
                popped = len(before) >= now["grow_to"][k]
                head = (before[0][0] + v[0], before[0][1] + v[1])
                out.append([head] + before[:len(before) - popped])
    return out


def np_causes(prev, now, dim, rules=None):
    """One env, one step.  Returns (cause uint8 [S], by uint8 [S], victims uint8 [S], where int8 [S, 2])."""
    _refuse_new_world(rules)
    bodies = post_bodies(prev, now)
    S = len(bodies)
    cause, by, victims = np.zeros(S, np.uint8), np.zeros(S, np.uint8), np.zeros(S, np.uint8)
    where = np.full((S, 2), NOWHERE, np.int8)
    for s, mine in enumerate(bodies):
        if mine is None:
            continue
        h = mine[0]
        c = 0
        if not (0 <= h[0] < dim and 0 <= h[1] < dim):
            c |= WALL
        if h in mine[1:]:
            c |= SELF
        for k, other in enumerate(bodies):
            if k == s or other is None:
                continue
            if h == other[0]:
                c |= HEAD_ON
                by[s] |= 16 << k
                victims[k] |= 16 << s
            if h in other[1:]:
                c |= BODY
                by[s] |= 1 << k
                victims[k] |= 1 << s
        cause[s] = c
        if c:
            where[s] = h
    return cause, by, victims, where


def events(prev, now, dim):
    """Counts over one env-step: snakes with each cause bit, deaths on the body of a snake that died in the same step,
    and deaths on the last piece of another snake's body."""
    bodies = post_bodies(prev, now)
    cause, by, _, _ = np_causes(prev, now, dim)
    ev = dict(deaths=int((cause != 0).sum()), wall=int(((cause & WALL) != 0).sum()), self=int(((cause & SELF) != 0).sum()),
              head_on=int(((cause & HEAD_ON) != 0).sum()), body=int(((cause & BODY) != 0).sum()), dead_owner=0, last_piece=0)
    for s in range(len(bodies)):
        owners = [k for k in range(len(bodies)) if by[s] >> k & 1]
        ev["dead_owner"] += any(not now["snakes"][k] for k in owners)
        ev["last_piece"] += any(len(bodies[k]) > 1 and bodies[k][-1] == bodies[s][0] for k in owners)
    return ev


def add_events(total, ev):
    for k, v in ev.items():
        total[k] = total.get(k, 0) + int(v)
    return total


class Twin(ap.Twin):
    """agents_play.Twin plus, after every step, cause / by / victims ([E, S] uint8) and where ([E, S, 2] int8) as
    msnake_death_causes has to write them, and `bodies`, the rebuilt post-move bodies of every env.  Plays every policy
    of timed_play.POLICIES."""

    def __init__(self, cfg):
        _refuse_new_world(cfg["rules"])
        super().__init__(cfg)

    def actions(self):
        return tp.choose_actions(self.cfg, self.states, self.rs)

    def step(self, act=None):
        act = super().step(act)
        out = [np_causes(p, n, self.cfg["dim"]) for p, n in zip(self.prev, self.now)]
        self.cause, self.by, self.victims, self.where = (np.stack([o[k] for o in out]) for k in range(4))
        self.bodies = [post_bodies(p, n) for p, n in zip(self.prev, self.now)]
        return act

    def events(self):
        """events() of the step just taken, summed over the envs."""
        total = {}
        for p, n in zip(self.prev, self.now):
            add_events(total, events(p, n, self.cfg["dim"]))
        return total


# ------------------------------------------------------------------------------------------ the hand-built table
FRUITS = [(0, 0), (0, 1), (0, 5)]


def state(snakes, vels, fruits=FRUITS, grow_to=None):
    """A canonical state of the table's 6x6 board: grow_to = max(3, len) unless given."""
    n = len(snakes)
    grow = [max(3, len(b)) for b in snakes] if grow_to is None else list(grow_to)
    return {"t": 3, "ctr": 40, "spare_fruits": 0, "ep_len": 3, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [list(v) for v in vels], "grow_to": grow,
            "alive": [True] * n, "in_dead": [False] * n}


_T2 = dict(snakes=[[(4, 2), (3, 2), (2, 2)], [(2, 3), (2, 4), (2, 5)], [(5, 0), (5, 1), (5, 2), (5, 3)]],
           vels=[(1, 0), (0, -1), (0, 0)])
_N = (NOWHERE, NOWHERE)
# name -> (state, actions, cause, by, victims, where): the expected values are literals, not computed
TABLE = {
    # the tail pops under a wall death: snake 1 moves onto the cell it left and lives
    "T1": (state([[(5, 2), (4, 2), (3, 2)], [(3, 3), (3, 4), (3, 5)], [(0, 3)]], [(1, 0), (0, -1), (0, 0)]),
           (1, 4, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0), ((6, 2), _N, _N)),
    # the owner dies on snake 2 without eating, its tail pops, snake 1 lives
    "T2": (state(**_T2), (1, 4, 0), (8, 0, 0), (0x04, 0, 0), (0, 0, 0x01), ((5, 2), _N, _N)),
    # fruit 0 under snake 2's body: snake 0 eats while dying, its tail stays, snake 1 dies on a dead snake's body
    "T3": (state(fruits=[(5, 2), (0, 1), (0, 5)], **_T2), (1, 4, 0), (8, 8, 0), (0x04, 0x01, 0), (0x02, 0, 0x01),
           ((5, 2), (2, 2), _N)),
    # snake 0 is growing (no pop) and lives: snake 1 dies on its last piece
    "T4": (state([_T2["snakes"][0], _T2["snakes"][1], [(5, 5)]], _T2["vels"], grow_to=[5, 3, 3]),
           (1, 4, 0), (0, 8, 0), (0, 0x01, 0), (0x02, 0, 0), (_N, (2, 2), _N)),
    # two heads meet on a third snake's body
    "M1": (state([[(2, 2), (1, 2), (0, 2)], [(4, 2), (5, 2), (5, 3)], [(3, 0), (3, 1), (3, 2), (3, 3)]], [(1, 0), (-1, 0), (0, 0)]),
           (1, 3, 0), (12, 12, 0), (0x24, 0x14, 0), (0x20, 0x10, 0x03), ((3, 2), (3, 2), _N)),
    # head-on with a snake that stands still
    "M2": (state([[(2, 2), (1, 2), (0, 2)], [(3, 2)], [(5, 5)]], [(1, 0), (0, 0), (0, 0)]),
           (1, 0, 0), (4, 4, 0), (0x20, 0x10, 0), (0x20, 0x10, 0), ((3, 2), (3, 2), _N)),
    # a refused reverse runs on into the wall
    "R": (state([[(5, 2), (4, 2), (3, 2)], [(0, 4)], [(0, 3)]], [(1, 0), (0, 0), (0, 0)]),
          (3, 0, 0), (1, 0, 0), (0, 0, 0), (0, 0, 0), ((6, 2), _N, _N)),
}
TABLE_ADVERSARIAL = ("T3",)   # the cases that are also run under adversarial


def table_cfg(rules, num_envs):
    return sp.scenario(rules, 6, 3, "safe_greedy", 1, num_envs, 1)


def step_table(rules, names=None):
    """The table's states installed into one oracle, one env per case, and stepped once with the table's actions.
    Returns (names, prev states, now states)."""
    names = list(TABLE) if names is None else list(names)
    ora = sp.make_oracle(table_cfg(rules, len(names)), auto_reset=False)
    ora.reset()
    for e, name in enumerate(names):
        ora.set_state(e, TABLE[name][0])
    read = sp._StateReader(ora)
    prev = [read(e) for e in range(len(names))]
    ora.step(np.array([TABLE[name][1] for name in names], np.int32))
    return names, prev, [read(e) for e in range(len(names))]


# ------------------------------------------------------------------------------------------ the behaviour table
def shares(dim, policy, num_envs=16, steps=1000, seed=1):
    """Deaths by cause when all three snakes play `policy` (eps 0) on a dim x dim snake_env board: the event counts."""
    cfg = sp.scenario("snake_env", dim, 3, policy, steps, num_envs, seed, eps=0.0, max_steps=2000)
    tw, total = Twin(cfg), {}
    for _ in range(steps):
        tw.step()
        add_events(total, tw.events())
    return total


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # the oracle package
    print("| board | policy | deaths | wall | self | head-on | body |")
    print("|---|---|---|---|---|---|---|")
    for dim in (10, 19):
        for policy in ("safe_greedy", "space_greedy", "timed_greedy"):
            ev = shares(dim, policy)
            pct = lambda k: f"{100.0 * ev[k] / max(1, ev['deaths']):.0f} %"
            print(f"| {dim}x{dim}x3 | {policy} | {ev['deaths']} | {pct('wall')} | {pct('self')} | {pct('head_on')} | {pct('body')} |")
