"""Shortest-path distances to the fruits and the opponent path_greedy, stated on canonical state dicts (Oracle.get_state).

np_field is the multi-source BFS distance of every free cell to the nearest free fruit cell, np_path reads it at the
target of every move, and path_greedy is space_greedy with that distance in place of the L1 distance.  The terms are
scripted_play's and space_play's: `used` = the cells of every body in the env, moves 1..4 = DIRS, a cell is free iff
it lies on the board and not in `used`, a move is open iff its target is free.  Nothing here asks the library under
test.

A plain helper module like space_play, which it imports and does not edit; imported by tests/test_path_host.py and
tests/test_path_gpu.py.
"""
from collections import deque

import numpy as np

import scripted_play as sp
import space_play as spp

DIRS = sp.DIRS
NONE = 0xFFFF   # MSNAKE_PATH_NONE


def np_field(st, dim):
    """int [dim, dim], indexed [c0, c1]: the length of the shortest 4-connected path through free cells to a source,
    NONE where there is none.  The sources are the fruits that lie on the board and are free; a cell in `used` holds
    NONE.  A plain queue BFS."""
    occ = spp.occupancy(st, dim)
    F = np.full((dim, dim), NONE, np.int64)
    queue = deque()
    for f in st["fruits"]:
        x, y = int(f[0]), int(f[1])
        if 0 <= x < dim and 0 <= y < dim and not occ[x, y] and F[x, y] == NONE:
            F[x, y] = 0
            queue.append((x, y))
    while queue:
        x, y = queue.popleft()
        for d0, d1 in DIRS.values():
            u, v = x + d0, y + d1
            if 0 <= u < dim and 0 <= v < dim and not occ[u, v] and F[u, v] == NONE:
                F[u, v] = F[x, y] + 1
                queue.append((u, v))
    return F


def np_path(st, dim, n_snakes, field=None):
    """int [n_snakes, 4]: entry [s, m] = the field at the target of move m + 1 of snake s when that move is open, NONE
    when it is not or the body is empty."""
    F = np_field(st, dim) if field is None else field
    occ = spp.occupancy(st, dim)
    out = np.full((n_snakes, 4), NONE, np.int64)
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            continue
        for a, (d0, d1) in DIRS.items():
            x, y = body[0][0] + d0, body[0][1] + d1
            if 0 <= x < dim and 0 <= y < dim and not occ[x, y]:
                out[s, a - 1] = F[x, y]
    return out


def path_greedy(st, dim, n_snakes, rs=None, eps=0.0):
    """space_greedy's eligible moves (open, and space >= need = min(body length, largest space of an open move)); among
    them the one with the smallest path entry, the first in the order 1, 2, 3, 4 on a tie; space_greedy's own action
    when no eligible move reaches a source; 0 for an empty body or when no move is open.  With probability eps a random
    action 0..4 instead (the POLICIES signature; the draws are space_greedy's)."""
    if eps:
        draws = [(rs.random() < eps) and int(rs.integers(0, 5)) + 1 for _ in range(n_snakes)]
    else:
        draws = [0] * n_snakes
    space = spp.np_space(st, dim, n_snakes)
    path = np_path(st, dim, n_snakes)
    fallback = spp.space_greedy(st, dim, n_snakes)
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if draws[s]:
            out.append(draws[s] - 1)
            continue
        if not body or not space[s].any():
            out.append(0)
            continue
        need = min(len(body), int(space[s].max()))
        best, best_d = 0, NONE
        for a in (1, 2, 3, 4):
            if space[s, a - 1] == 0 or space[s, a - 1] < need:
                continue
            if path[s, a - 1] < best_d:
                best, best_d = a, int(path[s, a - 1])
        out.append(best if best else fallback[s])
    return out


POLICIES = dict(spp.POLICIES, path_greedy=path_greedy)


def choose_actions(cfg, states, rs):
    """scripted_play.choose_actions with path_greedy among the policies."""
    pol = POLICIES[cfg["policy"]]
    return np.array([pol(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"]) for st, r in zip(states, rs)], np.int32)


def forage(cfg, policy, steps, compare=None):
    """The oracle alone under `policy` at eps 0 for `steps` steps: (total reward, episodes that ended, sum of their
    lengths, snake-steps at which `compare` would have played another action on the same state)."""
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
    return total, episodes, len_sum, differ
