"""Head-centred cell-code windows (msnake_render_local), stated twice on canonical state dicts (Oracle.get_state).

np_local is the contract of include/msnake.h word for word: entry [i][j] shows the cell head + (i - radius) f +
(j - radius) g in the codes of the view's plane (cells_play.np_cells), or 6 outside the grid.  np_local_rot says the same
thing without f and g: pad the plane with 6, crop around the head, turn the crop by the heading.  The two are compared
with each other on the CPU (tests/test_local_host.py) and the first with the library on the GPU (tests/test_local_gpu.py).
Nothing here asks the library under test.

A plain helper module like cells_play; imported by tests/test_local_host.py and tests/test_local_gpu.py.
"""
import numpy as np

import cells_play as cp

OUTSIDE = 6                                         # MSNAKE_CELL_OUTSIDE
MOVES = {1: (1, 0), 2: (0, 1), 3: (-1, 0), 4: (0, -1)}   # the header's move table
VELOCITIES = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1)]
HEADING = {(1, 0): 0, (0, 1): 1, (-1, 0): 2, (0, -1): 3, (0, 0): 0}


def heading_of(st, s):
    """The heading the library reports for snake s: from the velocity, 0 for an empty body."""
    return HEADING[tuple(st["vels"][s])] if st["snakes"][s] else 0


def relative_to_absolute(r, k):
    """The header's rule on plain ints."""
    return 0 if r == 0 else (r - 1 + k) % 4 + 1


def plane_of(st, dim, n_snakes, rules, s):
    return cp.np_cells(st, dim, n_snakes, rules, [s])[0]


def np_local(st, dim, n_snakes, rules, s, radius, oriented, plane=None):
    """(uint8 [W, W], heading): the formula of the header.  `plane`: plane_of(...) when the caller already has it."""
    w = 2 * radius + 1
    body = st["snakes"][s]
    if not body:
        return np.zeros((w, w), np.uint8), 0
    plane = plane_of(st, dim, n_snakes, rules, s) if plane is None else plane
    k = heading_of(st, s)
    kw = k if oriented else 0
    f, g = MOVES[kw + 1], MOVES[(kw + 1) % 4 + 1]
    i, j = np.meshgrid(np.arange(w) - radius, np.arange(w) - radius, indexing="ij")
    c0, c1 = body[0][0] + i * f[0] + j * g[0], body[0][1] + i * f[1] + j * g[1]
    inside = (c0 >= 0) & (c0 < dim) & (c1 >= 0) & (c1 < dim)
    win = np.where(inside, plane[np.clip(c0, 0, dim - 1), np.clip(c1, 0, dim - 1)], OUTSIDE).astype(np.uint8)
    return win, k


def np_local_rot(st, dim, n_snakes, rules, s, radius, oriented, plane=None):
    """The same window without f and g: pad the plane of view s with 6 by radius + 1, crop around the head, rot90."""
    w = 2 * radius + 1
    body = st["snakes"][s]
    if not body:
        return np.zeros((w, w), np.uint8), 0
    plane = plane_of(st, dim, n_snakes, rules, s) if plane is None else plane
    k = heading_of(st, s)
    padded = np.pad(plane, radius + 1, constant_values=OUTSIDE)
    h0, h1 = body[0]                                # in [-1, dim]: the pad of radius + 1 holds the whole crop
    crop = padded[h0 + 1:h0 + 1 + w, h1 + 1:h1 + 1 + w]
    assert crop.shape == (w, w)
    return np.ascontiguousarray(np.rot90(crop, -k if oriented else 0)), k


def np_local_all(states, dim, n_snakes, rules, snakes, radius, oriented, fn=np_local, planes=None):
    """(uint8 [E, S, W, W], uint8 [E, S]) over a list of states; `planes`: planes_all(...) to reuse over radii."""
    w = 2 * radius + 1
    win = np.zeros((len(states), len(snakes), w, w), np.uint8)
    head = np.zeros((len(states), len(snakes)), np.uint8)
    for e, st in enumerate(states):
        for q, s in enumerate(snakes):
            win[e, q], head[e, q] = fn(st, dim, n_snakes, rules, s, radius, oriented, None if planes is None else planes[e][s])
    return win, head


def planes_all(states, dim, n_snakes, rules):
    """planes[e][s]: the plane of view s of state e, for every snake (painted once, used for every radius)."""
    return [cp.np_cells(st, dim, n_snakes, rules, list(range(n_snakes))) for st in states]


def deal_velocities(states, n_snakes, start=0):
    """Deal the five velocities round-robin over the (state, snake) pairs, in place (the state builders leave nearly every
    velocity alone; msnake_set_state accepts any of the five for any body).  Returns the states."""
    k = start
    for st in states:
        st["vels"] = [list(VELOCITIES[(k + s) % 5]) for s in range(n_snakes)]
        k += n_snakes
    return states


def heading_shares(states, n_snakes):
    """Share of the (state, snake) pairs with a body that move in each of the four directions (1,0), (0,1), (-1,0), (0,-1)."""
    pairs = [(st, s) for st in states for s in range(n_snakes) if st["snakes"][s]]
    return [sum(tuple(st["vels"][s]) == v for st, s in pairs) / max(len(pairs), 1) for v in VELOCITIES[1:]]


def windows_from_planes(planes, states, snakes, radius, oriented):
    """Windows cut out of given planes [E, >= max(snakes) + 1, dim, dim] (e.g. cells_play.decode_frame of the oracle's frame)
    around the heads and headings of `states`: an expectation whose codes owe nothing to np_cells."""
    dim = planes.shape[-1]
    out = []
    for e, st in enumerate(states):
        out.append([np_local_rot(st, dim, None, None, s, radius, oriented, plane=planes[e][s])[0] for s in snakes])
    return np.array(out, np.uint8)
