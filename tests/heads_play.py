"""Head distances, the Voronoi owner map and the owned-cell counts, stated on canonical state dicts (Oracle.get_state).

np_heads gives, for every snake, the BFS distance D_s from the targets of its open moves to every free cell, plus one
(so that the head itself is the cell at distance 0); the owner of a free cell is the one snake with the smallest D_s, a
tie when two or more share it; counts are the cells a snake owns.  The terms are scripted_play's and space_play's: `used`
= the cells of every body in the env, moves 1..4 = DIRS, a cell is free iff it lies on the board and not in `used`, a move
is open iff its target is free.  Bodies are static; velocities and alive bits play no part.  Nothing here asks the
library under test.

A plain helper module like territory_play, which it imports and does not edit; imported by tests/test_heads_host.py and
tests/test_heads_gpu.py.
"""
import numpy as np

import territory_play as tp

NONE = 0xFFFF        # MSNAKE_HEAD_NONE
OWNER_TIE = 0xFE     # MSNAKE_OWNER_TIE
OWNER_NONE = 0xFF    # MSNAKE_OWNER_NONE


def np_heads(st, dim, n_snakes):
    """(D int [n_snakes, dim, dim], owner uint8 [dim, dim], counts int [n_snakes]), indexed [c0, c1].  D: a plain queue
    BFS (territory_play.bfs) from the snake's open targets, + 1; NONE where it does not reach, on every cell of `used`, and
    everywhere for an empty body or a snake without an open move; then 0 on the snake's own head where that lies on the
    board.  owner: for a free cell, the snake with the smallest D, OWNER_TIE when two or more share it, OWNER_NONE when
    none reaches; OWNER_NONE on every cell of `used`."""
    targets, occ = tp.open_targets(st, dim, n_snakes)
    D = np.full((n_snakes, dim, dim), NONE, np.int64)
    for s in range(n_snakes):
        if targets[s]:
            d = tp.bfs(occ, dim, list(targets[s].values()))
            D[s] = np.where(d < tp.INF, d + 1, NONE)
            assert (D[s][occ] == NONE).all() and D[s][D[s] != NONE].max() <= dim * dim - 1
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if body and 0 <= body[0][0] < dim and 0 <= body[0][1] < dim:
            D[s, int(body[0][0]), int(body[0][1])] = 0
    best = D.min(0)                                   # (NONE is larger than every finite distance)
    owner = np.where((D == best).sum(0) == 1, D.argmin(0), OWNER_TIE)
    owner = np.where(occ | (best == NONE), OWNER_NONE, owner).astype(np.uint8)
    counts = np.array([(owner == s).sum() for s in range(n_snakes)], np.int64)
    return D, owner, counts
