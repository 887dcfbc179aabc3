"""Reachable space and the flood-fill opponent space_greedy, stated on canonical state dicts (Oracle.get_state).

np_space counts, for every snake and move, the free cells 4-connected to the move's target; space_greedy is
safe_greedy restricted to the moves that lead into a region at least as large as the snake's body (or, when no region
is, into the largest).  The terms are scripted_play's: `used` = the cells of every body in the env, moves 1..4 =
DIRS, a move is open iff its target lies on the board and not in `used`.  Nothing here asks the library under test.

A plain helper module like scripted_play, which it imports and does not edit; imported by tests/test_space_host.py and
tests/test_space_gpu.py.
"""
import numpy as np

import scripted_play as sp

DIRS = sp.DIRS


def occupancy(st, dim):
    """bool [dim, dim], indexed [c0, c1]: the cell holds a piece of some body.  Cells outside the grid never count."""
    occ = np.zeros((dim, dim), bool)
    for body in st["snakes"]:
        for c0, c1 in body:
            if 0 <= c0 < dim and 0 <= c1 < dim:
                occ[c0, c1] = True
    return occ


def np_space(st, dim, n_snakes):
    """int [n_snakes, 4]: entry [s, m] = number of free cells 4-connected, through free cells, to the target of move
    m + 1 of snake s, the target included; 0 when the move is not open or the body is empty.  An explicit stack fill
    over the occupancy grid (padded by one blocked cell all round); a region that a fill has already covered keeps
    its label, so a second target inside it reads the stored size."""
    W = dim + 2
    pad = np.ones((W, W), bool)
    pad[1:-1, 1:-1] = occupancy(st, dim)
    lab = [-1 if b else 0 for b in pad.ravel().tolist()]   # -1 blocked, 0 free and not yet filled, k > 0 region k
    sizes = [0]
    out = np.zeros((n_snakes, 4), np.int64)
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            continue
        for a, (d0, d1) in DIRS.items():
            x, y = body[0][0] + d0, body[0][1] + d1
            if not (0 <= x < dim and 0 <= y < dim):
                continue
            start = (x + 1) * W + (y + 1)
            if lab[start] == -1:
                continue
            if lab[start] == 0:
                k = len(sizes)
                lab[start] = k
                stack, n = [start], 0
                while stack:
                    c = stack.pop()
                    n += 1
                    for nb in (c + W, c + 1, c - W, c - 1):
                        if lab[nb] == 0:
                            lab[nb] = k
                            stack.append(nb)
                sizes.append(n)
            out[s, a - 1] = sizes[lab[start]]
    return out


def space_greedy(st, dim, n_snakes, rs=None, eps=0.0):
    """need = min(body length, largest space of an open move); among the open moves whose space reaches `need`, the one
    whose target is closest (L1) to a fruit, the first in the order 1, 2, 3, 4 on a tie; 0 for an empty body or when
    no move is open.  With probability eps a random action 0..4 instead (the POLICIES signature)."""
    space = np_space(st, dim, n_snakes)
    fruits = st["fruits"]
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if eps and rs.random() < eps:
            out.append(int(rs.integers(0, 5)))
            continue
        if not body or not space[s].any():      # (an open move has a space of at least 1: its own target)
            out.append(0)
            continue
        need = min(len(body), int(space[s].max()))
        hx, hy = body[0]
        best, best_d = 0, None
        for a in (1, 2, 3, 4):
            if space[s, a - 1] == 0 or space[s, a - 1] < need:
                continue
            x, y = hx + DIRS[a][0], hy + DIRS[a][1]
            d = min((abs(f[0] - x) + abs(f[1] - y) for f in fruits), default=0)
            if best_d is None or d < best_d:
                best, best_d = a, d
        out.append(best)
    return out


POLICIES = dict(sp.POLICIES, space_greedy=space_greedy)


def choose_actions(cfg, states, rs):
    """scripted_play.choose_actions with space_greedy among the policies."""
    pol = POLICIES[cfg["policy"]]
    return np.array([pol(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"]) for st, r in zip(states, rs)], np.int32)


def mean_episode_length(cfg, policy, steps):
    """Mean length of the episodes that END within `steps` steps of the oracle alone under `policy` at eps 0, and the
    longest body seen."""
    cfg = dict(cfg, policy=policy, eps=0.0)
    ora = sp.make_oracle(cfg)
    read = sp._StateReader(ora)
    ora.reset()
    lens, longest = [], 0
    for _ in range(steps):
        states = [read(e) for e in range(cfg["num_envs"])]
        longest = max(longest, max(len(b) for st in states for b in st["snakes"]))
        _, _, done, _, _, ep_len = ora.step(choose_actions(cfg, states, [None] * len(states)))
        lens += [int(v) for v in np.asarray(ep_len)[np.asarray(done) != 0]]
    return float(np.mean(lens)), len(lens), longest


# ------------------------------------------------------------------------------------------ mazes
def serpentine(dim, transposed=False):
    """A serpentine maze as (wall cells, corridor cells in walking order).  Walls are the odd rows (c1 odd), each with
    a one-cell gap at alternating ends, so the free cells form ONE corridor that runs along every even row and through
    every gap.  transposed: the same with c0 and c1 swapped (walls on columns)."""
    walls, path = [], []
    right = True                                 # the direction the current even row is walked in
    for y in range(dim):
        if y % 2 == 0:
            xs = range(dim) if right else range(dim - 1, -1, -1)
            path += [(x, y) for x in xs]
        else:
            gap = dim - 1 if right else 0        # the wall's gap is where the row above ended
            walls += [(x, y) for x in range(dim) if x != gap]
            path.append((gap, y))
            right = not right
    if transposed:
        walls, path = [(y, x) for x, y in walls], [(y, x) for x, y in path]
    assert len(walls) + len(path) == dim * dim and not set(walls) & set(path)
    return walls, path
