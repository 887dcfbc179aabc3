"""Voronoi territory and the opponent territory_greedy, stated on canonical state dicts (Oracle.get_state).

np_territory counts, for every snake and move, the free cells the snake reaches from the move's target in strictly
fewer steps than any OTHER snake needs from the targets of its own open moves; territory_greedy is space_greedy with
that count in place of the reachable space.  The terms are scripted_play's and space_play's: `used` = the cells of every
body in the env, moves 1..4 = DIRS, a cell is free iff it lies on the board and not in `used`, a move is open iff its
target is free.  Bodies are static; velocities and alive bits play no part.  Nothing here asks the library under test.

Two statements of the same count: np_territory, by two plain BFS distance fields, is the definition;
territory_sets, a race of growing sets on whole-board bit masks (Python integers), is what the players use because it is
many times faster.  tests/test_territory_host.py pins the second to the first on seeded random boards.

A plain helper module like space_play, which it imports and does not edit; imported by tests/test_territory_host.py
and tests/test_territory_gpu.py.
"""
from collections import deque

import numpy as np

import scripted_play as sp
import space_play as spp

DIRS = sp.DIRS
INF = 1 << 30


def _body(st, s):
    return st["snakes"][s] if s < len(st["snakes"]) else []


def open_targets(st, dim, n_snakes):
    """Per snake, {move: target} of its open moves (empty for an empty body), and the occupancy grid."""
    occ = spp.occupancy(st, dim)
    out = []
    for s in range(n_snakes):
        body, tg = _body(st, s), {}
        if body:
            for a, (d0, d1) in DIRS.items():
                x, y = int(body[0][0]) + d0, int(body[0][1]) + d1   # (plain ints: the set form shifts by them)
                if 0 <= x < dim and 0 <= y < dim and not occ[x, y]:
                    tg[a] = (x, y)
        out.append(tg)
    return out, occ


def bfs(occ, dim, sources):
    """BFS distance through free cells from the set `sources` (free cells) to every cell; INF where it does not reach."""
    dist = np.full((dim, dim), INF, np.int64)
    q = deque()
    for c in sources:
        if dist[c] == INF:
            dist[c] = 0
            q.append(c)
    while q:
        x, y = q.popleft()
        d = dist[x, y] + 1
        for d0, d1 in DIRS.values():
            u, v = x + d0, y + d1
            if 0 <= u < dim and 0 <= v < dim and not occ[u, v] and dist[u, v] == INF:
                dist[u, v] = d
                q.append((u, v))
    return dist


def np_territory(st, dim, n_snakes):
    """int [n_snakes, 4]: entry [s, m] = |{c free: dA(c) < dB(c)}| with dA the BFS distance from the target of move
    m + 1 of snake s and dB the BFS distance from O_s, the targets of the open moves of every other snake (infinite
    when there is none, or no way); 0 when the move is not open or the body is empty.  Ties go to the others, so an
    open move whose target another snake can enter as well counts 0."""
    targets, occ = open_targets(st, dim, n_snakes)
    out = np.zeros((n_snakes, 4), np.int64)
    for s in range(n_snakes):
        if not targets[s]:
            continue
        others = [t for j in range(n_snakes) if j != s for t in targets[j].values()]
        dB = bfs(occ, dim, others)
        for a, t in targets[s].items():
            dA = bfs(occ, dim, [t])
            out[s, a - 1] = int(((dA < dB) & (dA < INF)).sum())
    return out


def territory_sets(st, dim, n_snakes):
    """The same counts by the set form: B_0 = O_s, A_0 = {t} \\ B_0; per round B grows by its free neighbours first, then
    A by its free neighbours outside the B that has already grown; |A| once A has stopped.  Sets are Python integers,
    bit x * W + y <-> cell (x, y) with W = dim + 1: the spare column is never free, so a shift by one cannot wrap."""
    targets, occ = open_targets(st, dim, n_snakes)
    W = dim + 1
    vacant = 0
    for x, y in zip(*np.nonzero(~occ)):
        vacant |= 1 << (int(x) * W + int(y))
    out = np.zeros((n_snakes, 4), np.int64)
    for s in range(n_snakes):
        if not targets[s]:
            continue
        B = 0
        for j in range(n_snakes):
            if j != s:
                for x, y in targets[j].values():
                    B |= 1 << (x * W + y)
        moves = sorted(targets[s])
        A = [(1 << (targets[s][a][0] * W + targets[s][a][1])) & ~B for a in moves]
        changed = True
        while changed:
            changed = False
            B |= ((B << 1) | (B >> 1) | (B << W) | (B >> W)) & vacant
            may = vacant & ~B
            for i, f in enumerate(A):
                g = f | (((f << 1) | (f >> 1) | (f << W) | (f >> W)) & may)
                if g != f:
                    A[i], changed = g, True
        for a, f in zip(moves, A):
            out[s, a - 1] = bin(f).count("1")
    return out


def greedy_by_count(st, dim, n_snakes, count, rs=None, eps=0.0):
    """space_greedy's choice with `count` [n_snakes, 4] in place of the space: need = min(body length, largest count
    of an open move); among the open moves whose count reaches `need` (all of them when every count is 0), the one
    whose target is closest (L1) to a fruit, the first in the order 1, 2, 3, 4 on a tie; 0 for an empty body or when
    no move is open.  With probability eps a random action 0..4 instead (the POLICIES signature)."""
    targets, _ = open_targets(st, dim, n_snakes)
    fruits = st["fruits"]
    out = []
    for s in range(n_snakes):
        body = _body(st, s)
        if eps and rs.random() < eps:
            out.append(int(rs.integers(0, 5)))
            continue
        if not body or not targets[s]:
            out.append(0)
            continue
        need = min(len(body), max(int(count[s, a - 1]) for a in targets[s]))
        best, best_d = 0, None
        for a in (1, 2, 3, 4):
            if a not in targets[s] or count[s, a - 1] < need:
                continue
            x, y = targets[s][a]
            d = min((abs(f[0] - x) + abs(f[1] - y) for f in fruits), default=0)
            if best_d is None or d < best_d:
                best, best_d = a, d
        out.append(best)
    return out


def territory_greedy(st, dim, n_snakes, rs=None, eps=0.0):
    """greedy_by_count on the territory (the set form; np_territory gives the same counts)."""
    return greedy_by_count(st, dim, n_snakes, territory_sets(st, dim, n_snakes), rs, eps)


def territory_greedy_bfs(st, dim, n_snakes, rs=None, eps=0.0):
    """The same policy on the BFS form: what the definition says, for the tests that pin the fast one."""
    return greedy_by_count(st, dim, n_snakes, np_territory(st, dim, n_snakes), rs, eps)


POLICIES = dict(spp.POLICIES, territory_greedy=territory_greedy)


def choose_actions(cfg, states, rs):
    """space_play.choose_actions with territory_greedy among the policies."""
    pol = POLICIES[cfg["policy"]]
    return np.array([pol(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"]) for st, r in zip(states, rs)], np.int32)


def seat_actions(cfg, states, seat0, others):
    """One action row per env at eps 0: snake 0 plays policy `seat0`, every other snake policy `others`.  Each policy is
    asked once per state, whatever the number of seats it holds."""
    ns, dim = cfg["n_snakes"], cfg["dim"]
    rows = []
    for st in states:
        a = POLICIES[others](st, dim, ns)
        if seat0 != others:
            a = [POLICIES[seat0](st, dim, ns)[0]] + a[1:]
        rows.append(a)
    return np.array(rows, np.int32)


def play_seats(cfg, seat0, others, steps):
    """`steps` steps of the oracle alone with snake 0 under `seat0` and the rest under `others`, eps 0: the number of
    episodes that ended, their mean length and their mean return."""
    cfg = dict(cfg, eps=0.0)
    ora = sp.make_oracle(cfg)
    read = sp._StateReader(ora)
    ora.reset()
    lens, rets = [], []
    for _ in range(steps):
        states = [read(e) for e in range(cfg["num_envs"])]
        _, _, done, _, ep_ret, ep_len = ora.step(seat_actions(cfg, states, seat0, others))
        ended = np.asarray(done) != 0
        lens += [int(v) for v in np.asarray(ep_len)[ended]]
        rets += [float(v) for v in np.asarray(ep_ret)[ended]]
    return len(lens), float(np.mean(lens)) if lens else 0.0, float(np.mean(rets)) if rets else 0.0
