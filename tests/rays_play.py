"""Eight-direction ray observations (msnake_render_rays), stated twice on canonical state dicts (Oracle.get_state).

np_rays is the contract of include/msnake.h word for word: from the head, walk head + t d for t = 1, 2, ... over the
plane of the snake's view (cells_play.np_cells); `wall` is the first t whose cell lies outside the grid, and `fruit`,
`own` and `other` are the first t < wall whose cell holds code 1, 2 / 3, 4 / 5, or 0 when there is none.
rays_from_window says the same thing on a window of local_play.np_local: walk from its centre, the first 6 is the wall.
The two are compared with each other on the CPU (tests/test_rays_host.py) and the first with the library on the GPU
(tests/test_rays_gpu.py).  Nothing here asks the library under test.

A plain helper module like cells_play / local_play; imported by tests/test_rays_host.py and tests/test_rays_gpu.py.
"""
import numpy as np

import cells_play as cp
import local_play as lp

DIRS, CHANNELS = 8, 4                  # MSNAKE_RAY_DIRS, MSNAKE_RAY_CHANNELS
WALL, FRUIT, OWN, OTHER = 0, 1, 2, 3   # MSNAKE_RAY_*
CHANNEL_OF = {1: FRUIT, 2: OWN, 3: OWN, 4: OTHER, 5: OTHER}   # cell code of the view's plane -> channel


def directions(k):
    """The eight directions under heading k, in f / g terms: j = 0, 2, 4, 6 is f, g, -f, -g; j = 1, 3, 5, 7 is f + g,
    g - f, -f - g, f - g."""
    f, g = lp.MOVES[k + 1], lp.MOVES[(k + 1) % 4 + 1]
    nf, ng = (-f[0], -f[1]), (-g[0], -g[1])
    add = lambda a, b: (a[0] + b[0], a[1] + b[1])
    return [f, add(f, g), g, add(g, nf), nf, add(nf, ng), ng, add(f, ng)]


def np_rays(st, dim, n_snakes, rules, s, oriented, plane=None):
    """(uint8 [8, 4], heading): the walk of the header.  `plane`: local_play.plane_of(...) when the caller has it."""
    out = np.zeros((DIRS, CHANNELS), np.uint8)
    body = st["snakes"][s]
    if not body:
        return out, 0
    plane = lp.plane_of(st, dim, n_snakes, rules, s) if plane is None else plane
    k = lp.heading_of(st, s)
    for j, d in enumerate(directions(k if oriented else 0)):
        t = 1
        while True:
            c0, c1 = body[0][0] + t * d[0], body[0][1] + t * d[1]
            if not (0 <= c0 < dim and 0 <= c1 < dim):
                break
            ch = CHANNEL_OF.get(int(plane[c0, c1]))
            if ch is not None and out[j, ch] == 0:
                out[j, ch] = t
            t += 1
        out[j, WALL] = t
    return out, k


# window offsets (di, dj) of the eight directions: the window's axes ARE f and g
_WINDOW_DIRS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def rays_from_window(win):
    """uint8 [8, 4] read off one window uint8 [W, W] of local_play.np_local (same `oriented`): walk from the centre, the
    first 6 is the wall.  The window must reach the wall in every direction (radius 31 does for dim <= 30); a window of
    zeros (an empty body) gives zeros."""
    win = np.asarray(win)
    r = win.shape[0] // 2
    out = np.zeros((DIRS, CHANNELS), np.uint8)
    if not win.any():
        return out
    for j, (di, dj) in enumerate(_WINDOW_DIRS):
        for t in range(1, r + 1):
            code = int(win[r + t * di, r + t * dj])
            if code == lp.OUTSIDE:
                out[j, WALL] = t
                break
            ch = CHANNEL_OF.get(code)
            if ch is not None and out[j, ch] == 0:
                out[j, ch] = t
        else:
            raise AssertionError(f"the window of radius {r} does not reach the wall in direction {j}")
    return out


def np_rays_all(states, dim, n_snakes, rules, snakes, oriented, planes=None):
    """(uint8 [E, S, 8, 4], uint8 [E, S]) over a list of states; `planes`: local_play.planes_all(...) to reuse."""
    rays = np.zeros((len(states), len(snakes), DIRS, CHANNELS), np.uint8)
    head = np.zeros((len(states), len(snakes)), np.uint8)
    for e, st in enumerate(states):
        for q, s in enumerate(snakes):
            rays[e, q], head[e, q] = np_rays(st, dim, n_snakes, rules, s, oriented, None if planes is None else planes[e][s])
    return rays, head


def rays_from_windows(windows):
    """uint8 [E, S, 8, 4] read off windows uint8 [E, S, W, W]."""
    windows = np.asarray(windows)
    return np.array([[rays_from_window(w) for w in env] for env in windows], np.uint8).reshape(windows.shape[:2] + (DIRS, CHANNELS))


def rotate(rays_un, k):
    """The header's identity: the oriented rays of heading k out of the unoriented ones, rays_or[j] = rays_un[(j + 2 k) mod 8]."""
    return np.roll(np.asarray(rays_un), -2 * int(k), axis=-2)


# ------------------------------------------------------------------------------------------ the builder sets
SNAKE_ENV_SETS = [(2, 1), (2, 3), (5, 2), (5, 3), (19, 1), (19, 2), (19, 3), (33, 3), (62, 3)]   # (dim, n_snakes)
NEW_WORLD_SETS = [(6, 4, 4), (19, 4, 32), (62, 2, 2)]                                            # (dim, n_snakes, n_fruits)
ADVERSARIAL_SETS = [(10, 3), (19, 2)]                                                            # (dim, n_snakes)


_SPECS = {}
for _dim, _ns in SNAKE_ENV_SETS:
    _SPECS[f"S{_dim}x{_ns}"] = (0, _dim, _ns, _ns)
for _dim, _ns, _nf in NEW_WORLD_SETS:
    _SPECS[f"N{_dim}x{_ns}f{_nf}"] = (1, _dim, _ns, _nf)
for _dim, _ns in ADVERSARIAL_SETS:
    _SPECS[f"A{_dim}x{_ns}"] = (2, _dim, _ns, _ns)
SET_NAMES = list(_SPECS)
_BUILT = {}


def builder_set(name):
    """(name, rules, dim, n_snakes, n_fruits, states): the hand-built states of cells_play for one entry of SET_NAMES, with
    the five velocities dealt over the (state, snake) pairs.  Built once; callers leave the states as they are."""
    if name not in _BUILT:
        rules, dim, ns, nf = _SPECS[name]
        states = (cp.snake_env_states(dim, ns) if rules == 0 else cp.new_world_states(dim, ns, nf) if rules == 1 else
                  cp.adversarial_states(dim, ns))
        _BUILT[name] = (name, rules, dim, ns, nf, lp.deal_velocities(states, ns, start=rules))
    return _BUILT[name]


def builder_sets():
    """Every builder set, under all three rule sets."""
    return [builder_set(name) for name in SET_NAMES]
