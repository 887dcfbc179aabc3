"""Cell lifetimes, the timed reach and the opponent timed_greedy, stated on canonical state dicts (Oracle.get_state).

np_life is the lifetime of every cell: after how many steps the body piece lying there will have moved on.  np_timed is
the level-by-level flood fill that may enter a body cell once its lifetime has run out, counted for every move, and
timed_greedy is space_greedy with that count in place of the space.  The terms are scripted_play's and space_play's:
`used` = the cells of every body in the env, moves 1..4 = DIRS, a cell is free iff it lies on the board and not in
`used`, a move is open iff its target is free.  Nothing here asks the library under test.

A plain helper module like path_play; it imports space_play and does not edit it; imported by tests/test_timed_host.py
and tests/test_timed_gpu.py.
"""
import numpy as np

import scripted_play as sp
import space_play as spp

DIRS = sp.DIRS
NEVER = 0xFFFF    # MSNAKE_LIFE_NEVER
LIFE_CAP = 0xFFFE


def never_pops(cfg):
    """new_world without fruits: that rule set never pops a tail, every piece has the lifetime NEVER."""
    return cfg["rules"] == sp.RULES["new_world"] and cfg["n_fruits"] == 0


def piece_life(length, grow_to, i, never=False):
    """l(s, i) = min(0xFFFE, (len - i) + max(0, grow_to - len)); NEVER under a rule set that never pops."""
    return NEVER if never else min(LIFE_CAP, (length - i) + max(0, grow_to - length))


def np_life(st, dim, never=False):
    """int [dim, dim], indexed [c0, c1]: the maximum of the piece lifetimes over all pieces of all snakes that lie on the
    cell, stacked duplicates included; 0 for a cell with no piece.  Pieces outside the grid are ignored."""
    life = np.zeros((dim, dim), np.int64)
    for s, body in enumerate(st["snakes"]):
        for i, (c0, c1) in enumerate(body):
            if 0 <= c0 < dim and 0 <= c1 < dim:
                life[c0, c1] = max(life[c0, c1], piece_life(len(body), st["grow_to"][s], i, never))
    return life


def timed_fill(life, dim, target):
    """V of the timed fill from `target`, as a dict cell -> the level that took it.  V_1 = F_1 = {target}; level t takes
    the cells in the grid that are not taken yet, have Life < t and are 4-adjacent to a cell of F_(t-1); only the last
    front expands."""
    taken = {target: 1}
    front, t = [target], 1
    while front:
        t += 1
        fresh = []
        for x, y in front:
            for d0, d1 in DIRS.values():
                c = (x + d0, y + d1)
                if 0 <= c[0] < dim and 0 <= c[1] < dim and c not in taken and life[c] < t:
                    taken[c] = t
                    fresh.append(c)
        front = fresh
    assert t <= dim * dim + 1
    return taken


def _bitboard(life, dim):
    """The lifetimes as masks of one Python integer per value: cell (c0, c1) is bit c0 * (dim + 1) + c1, so that column
    c1 == dim is a gap no mask ever holds and a shift by 1 or dim + 1 is a step to a 4-neighbour or off the board."""
    by_life = {}
    for c0, row in enumerate(life.tolist()):
        for c1, v in enumerate(row):
            by_life[v] = by_life.get(v, 0) | 1 << (c0 * (dim + 1) + c1)
    return by_life


def timed_fill_size(by_life, dim, target):
    """|V| of timed_fill, by the same levels on _bitboard masks (the expectations of whole batches need the speed;
    tests/test_timed_host.py holds the two against each other)."""
    W = dim + 1
    front = seen = 1 << (int(target[0]) * W + int(target[1]))
    admit, t = by_life.get(0, 0) | by_life.get(1, 0), 1       # the cells with Life < 2
    while front:
        t += 1
        front = (front << 1 | front >> 1 | front << W | front >> W) & ~seen & admit
        seen |= front
        admit |= by_life.get(t, 0)                            # ... with Life < t + 1
    return bin(seen).count("1")


def np_timed(st, dim, n_snakes, life=None, never=False):
    """int [n_snakes, 4]: entry [s, m] = |V| of the timed fill from the target of move m + 1 of snake s; 0 when the move
    is not open or the body is empty."""
    life = np_life(st, dim, never) if life is None else life
    by_life = _bitboard(life, dim)
    out = np.zeros((n_snakes, 4), np.int64)
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            continue
        for a, (d0, d1) in DIRS.items():
            x, y = body[0][0] + d0, body[0][1] + d1
            if 0 <= x < dim and 0 <= y < dim and life[x, y] == 0:
                out[s, a - 1] = timed_fill_size(by_life, dim, (x, y))
    return out


def greedy_by_count(st, n_snakes, count):
    """space_greedy's choice with `count` [n_snakes, 4] (0 <=> the move is not open) in place of the space."""
    fruits = st["fruits"]
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body or not count[s].any():
            out.append(0)
            continue
        need = min(len(body), int(count[s].max()))
        hx, hy = body[0]
        best, best_d = 0, None
        for a in (1, 2, 3, 4):
            if count[s, a - 1] == 0 or count[s, a - 1] < need:
                continue
            x, y = hx + DIRS[a][0], hy + DIRS[a][1]
            d = min((abs(f[0] - x) + abs(f[1] - y) for f in fruits), default=0)
            if best_d is None or d < best_d:
                best, best_d = a, d
        out.append(best)
    return out


def timed_greedy(st, dim, n_snakes, rs=None, eps=0.0, never=False):
    """need = min(body length, largest timed reach of an open move); among the open moves whose reach is at least `need`,
    the one whose target is closest (L1) to a fruit, the first in the order 1, 2, 3, 4 on a tie; 0 for an empty body or
    when no move is open.  With probability eps a random action 0..4 instead (the POLICIES signature; the draws are
    space_greedy's)."""
    choice = greedy_by_count(st, n_snakes, np_timed(st, dim, n_snakes, never=never))
    if eps:
        for s in range(n_snakes):
            if rs.random() < eps:
                choice[s] = int(rs.integers(0, 5))
    return choice


POLICIES = dict(spp.POLICIES, timed_greedy=timed_greedy)


# ------------------------------------------------------------------------------------------ timing cases with closed forms
BIG = 2 ** 31 - 1   # the largest grow_to of an installed state: every lifetime of that body is 0xFFFE


def _state(snakes, fruits, grow_to):
    n = len(snakes)
    return {"t": 3, "ctr": 40, "spare_fruits": 0, "ep_len": 3, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n, "grow_to": list(grow_to),
            "alive": [True] * n, "in_dead": [False] * n}


def door_state(life, second_route=False):
    """7x7, three snakes.  Snake 1 is the wall c0 == 3 with lifetimes clamped high, but for the door (3, 3), which is the
    one piece of snake 2 with lifetime `life`.  Snake 0 is one cell at (0, 3): its move 1 has the target (1, 3), from
    which the door is reached at BFS level 3.  second_route: the wall has a gap at (3, 6)."""
    wall = [(3, y) for y in range(7) if y != 3 and not (second_route and y == 6)]
    return _state([[(0, 3)], wall, [(3, 3)]], [(6, 6)] * 3, [1, BIG, life])


COIL = [(3, 3), (3, 4), (2, 4), (1, 4), (0, 4), (0, 3), (0, 2), (1, 2), (2, 2)]   # round the pocket (2, 3), (1, 3); the tail at (2, 2)


def coil_state(grow_to=len(COIL), n_snakes=1):
    """7x7: a snake of 9 coiled round a pocket of two cells whose exit is its own tail; the fruit lies in the pocket."""
    return _state([COIL] + [[]] * (n_snakes - 1), [(1, 3)] * n_snakes, [grow_to] + [1] * (n_snakes - 1))


def choose_actions(cfg, states, rs):
    """scripted_play.choose_actions with timed_greedy among the policies (which is told whether the rule set pops)."""
    pol = POLICIES[cfg["policy"]]
    kw = dict(never=True) if cfg["policy"] == "timed_greedy" and never_pops(cfg) else {}
    return np.array([pol(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"], **kw) for st, r in zip(states, rs)], np.int32)


def survival(cfg, policy, steps, compare=None):
    """The oracle alone under `policy` at eps 0 for `steps` steps, every snake under that policy, auto reset on: (episodes
    that ended, sum of their lengths, total reward, snake-steps at which `compare` would have played another action on
    the same state)."""
    cfg = dict(cfg, policy=policy, eps=0.0)
    ora = sp.make_oracle(cfg)
    read = sp._StateReader(ora)
    ora.reset()
    total, episodes, len_sum, differ = 0.0, 0, 0, 0
    for _ in range(steps):
        states = [read(e) for e in range(cfg["num_envs"])]
        act = choose_actions(cfg, states, [None] * len(states))
        if compare is not None:
            other = choose_actions(dict(cfg, policy=compare), states, [None] * len(states))
            differ += int((act != other).sum())
        _, rew, done, _, _, ep_len = ora.step(act)
        total += float(np.asarray(rew, np.float64).sum())
        ended = np.asarray(done) != 0
        episodes += int(ended.sum())
        len_sum += int(np.asarray(ep_len)[ended].sum())
    return episodes, len_sum, total, differ
