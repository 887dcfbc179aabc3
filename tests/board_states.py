"""Hand-built canonical state dicts for the tests and the *_play helpers: plain Python over scripted_play's tables and a
NumPy generator, no torch and no library.  Every builder draws from the rng it is given in a fixed order, so a seed
names a set of boards.
"""

import scripted_play as sp


def state(snakes, fruits, alive=None, in_dead=None):
    n = len(snakes)
    return {"t": 3, "ctr": 40, "spare_fruits": 0, "ep_len": 3, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n, "grow_to": [max(len(b), 1) for b in snakes],
            "alive": alive or [True] * n, "in_dead": in_dead or [False] * n}


def line(cells, dim):
    """Boustrophedon path over the board as a list of cells (for long bodies)."""
    out = []
    for y in range(dim):
        xs = range(dim) if y % 2 == 0 else range(dim - 1, -1, -1)
        out += [(x, y) for x in xs]
    return out[:cells]


def serpentine_body(dim, length, start_row):
    """A self-avoiding boustrophedon body of `length` cells starting in row `start_row` (head last
    visited, i.e. head first in the list), so bodies far longer than one 64-cell chunk are legal."""
    path = []
    for r in range(start_row, dim):
        cols = range(dim) if (r - start_row) % 2 == 0 else range(dim - 1, -1, -1)
        path += [[c, r] for c in cols]
    path = path[:length]
    return path[::-1]


def cycle(dim):
    """The cells of scripted_play's Hamiltonian cycle of an even board, from (0, 0)."""
    tab, c, out = sp.hamiltonian_table(dim), (0, 0), []
    for _ in range(dim * dim):
        out.append(c)
        d = sp.DIRS[tab[c[0]][c[1]]]
        c = (c[0] + d[0], c[1] + d[1])
    assert c == (0, 0) and len(set(out)) == dim * dim
    return out


def border_states(dim, ns, nf, rng):
    """Heads on every corner and border (all of them for small boards), at -1 / dim, single cells and short bodies."""
    cells = [(x, y) for x in range(dim) for y in range(dim) if x in (0, dim - 1) or y in (0, dim - 1)]
    if len(cells) > 40:
        keep = {(0, 0), (0, dim - 1), (dim - 1, 0), (dim - 1, dim - 1)}
        cells = sorted(keep) + [cells[i] for i in rng.choice(len(cells), 36, replace=False)]
    outside = [(-1, y) for y in (0, dim // 2, dim - 1)] + [(dim, y) for y in (0, dim // 2, dim - 1)] + \
              [(x, -1) for x in (0, dim // 2, dim - 1)] + [(x, dim) for x in (0, dim // 2, dim - 1)]
    states = []
    for head in cells + outside:
        bodies = [[head]]
        for s in range(1, ns):   # the other snakes: random cells, sometimes next to the head, sometimes empty
            k = int(rng.integers(0, 4))
            near = [(head[0] + d0, head[1] + d1) for d0, d1 in sp.DIRS.values()]
            near = [c for c in near if 0 <= c[0] < dim and 0 <= c[1] < dim]
            body = [tuple(rng.integers(0, dim, 2)) for _ in range(k)]
            if near and rng.random() < 0.6:
                body.append(near[int(rng.integers(0, len(near)))])
            bodies.append(body)
        fruits = [tuple(rng.integers(0, dim, 2)) for _ in range(nf)]
        states.append(state(bodies, fruits))
    return states


def random_states(dim, ns, nf, rng, count, fruit_lo=0, fruit_hi=None, dup=False):
    fruit_hi = dim if fruit_hi is None else fruit_hi
    states = []
    for _ in range(count):
        bodies = []
        for s in range(ns):
            k = int(rng.integers(0, min(dim * dim, 40) + 1)) if rng.random() < 0.9 else 0
            body = [tuple(int(v) for v in rng.integers(0, dim, 2)) for _ in range(k)]
            if dup and k > 2:
                body[2] = body[1]
            bodies.append(body)
        fruits = [tuple(int(v) for v in rng.integers(fruit_lo, fruit_hi, 2)) for _ in range(nf)]
        states.append(state(bodies, fruits))
    return states


def tie_states(dim):
    """Two snakes on a board of dim >= 6: for every pair of directions, the two other moves blocked by snake 1 and the
    distances of the two open ones equal (one fruit on the head: every move is at distance 1; two fruits at equal
    distances behind the targets); every single direction open alone; all four blocked."""
    h = (dim // 2, dim // 2)
    tgt = {a: (h[0] + d[0], h[1] + d[1]) for a, d in sp.DIRS.items()}
    far = {a: (h[0] + 2 * d[0], h[1] + 2 * d[1]) for a, d in sp.DIRS.items()}
    states = []
    for a in range(1, 5):
        for b in range(a + 1, 5):
            blockers = [tgt[c] for c in range(1, 5) if c not in (a, b)]
            states.append(state([[h], blockers], [h, h]))
            states.append(state([[h], blockers], [far[a], far[b]]))
            states.append(state([[h], blockers], [far[b], far[a]]))
            states.append(state([[h], []], [far[a], far[b]]))          # nothing blocked: the tie decides alone
    for a in range(1, 5):
        states.append(state([[h], [tgt[c] for c in range(1, 5) if c != a]], [h, far[a]]))
    states.append(state([[h], [tgt[c] for c in range(1, 5)]], [h, h]))                    # every move blocked by the other snake
    states.append(state([[h, tgt[1], tgt[2]], [tgt[3], tgt[4]]], [h, h]))                 # ... by both bodies
    states.append(state([[(0, 0), (1, 0)], [(0, 1)]], [h, h]))                            # ... by the wall and both bodies
    states.append(state([[h], []], [(h[0] + 2, h[1] + 2), (0, 0)]))                       # a diagonal fruit: moves 1 and 2 tie
    states.append(state([[h], []], [(h[0] - 2, h[1] - 2), (0, 0)]))                       # moves 3 and 4 tie
    states.append(state([[], []], [h, h]))                                                # empty bodies
    return states


def dense_states(dim, ns, nf, rng, count, fruit_lo=0, fruit_hi=None):
    """Boards with 25 .. 65 % of their cells in bodies (many separate regions, pockets of every size), dealt to the
    snakes at random; heads anywhere, sometimes stacked on a body.  Bodies reach the overflow ring on boards >= 19."""
    fruit_hi = dim if fruit_hi is None else fruit_hi
    cells = [(x, y) for x in range(dim) for y in range(dim)]
    states = []
    for _ in range(count):
        k = int(rng.uniform(0.25, 0.65) * dim * dim)
        pick = [cells[i] for i in rng.permutation(len(cells))[:k]]
        cuts = sorted(int(v) for v in rng.integers(0, k + 1, ns - 1))
        bodies = [pick[a:b] for a, b in zip([0] + cuts, cuts + [k])]
        fruits = [tuple(int(v) for v in rng.integers(fruit_lo, fruit_hi, 2)) for _ in range(nf)]
        states.append(state(bodies, fruits))
    return states


def return_lane_states(dim, ns):
    """Bodies of 64 and more cells laid along the Hamiltonian cycle with the head in the return lane (column 0): the cell
    beside the head, in column 1, was visited long ago, so the piece that blocks that move has an index >= 64 -- and the
    same bodies cut to 64 pieces, where that move is open."""
    d = dim - dim % 2
    cyc = cycle(d)
    N = d * d
    states = []
    for y in (1, 2, 3):
        k = N - y                                   # cyc[k] = (0, y), on the way up the return lane
        assert cyc[k] == (0, y)
        far = (k - cyc.index((1, y))) % N           # piece index of (1, y) in a body whose head is cyc[k]
        for n in sorted({far + 1, far + 4, min(far + 20, N - 8)} | {64}):
            if n < 64 or n > N - 8:
                continue
            body = [cyc[(k - i) % N] for i in range(n)]
            free = [c for c in cyc if c not in set(body)]
            others = [[free[3 + s]] for s in range(ns - 1)]
            states.append(state([body] + others, [free[-1 - s] for s in range(ns)]))
    return states


def overflow_states(dim, ns):
    """return_lane_states; on even boards also a body whose pieces >= 64 are a wall: it covers row 1 over columns
    1..dim-1 first and then 64 + 2 more cells of the cycle, so that snake 1's head at (0, 1) sees the cells above the
    wall by move 4 and the cells below it by move 2.  Returns (states, the number of walled ones at the end)."""
    states = return_lane_states(dim, ns)
    walled = 0
    if dim % 2 == 0:
        cyc = cycle(dim)
        t0 = cyc.index((dim - 1, 1))
        for extra in (2, 5):
            n = 64 + (dim - 1) + extra
            body = [cyc[t0 + n - 1 - i] for i in range(n)]             # the tail (dim-1, 1), the head n - 1 cells further on
            assert body[-1] == (dim - 1, 1) and all(c[0] >= 1 for c in body) and body.index((1, 1)) >= 64
            states.append(state([body, [(0, 1)]] + [[]] * (ns - 2), [(0, 0)] * ns))
            walled += 1
    return states, walled
