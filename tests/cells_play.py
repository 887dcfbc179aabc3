"""The observation as cell codes (msnake_render_cells), stated on canonical state dicts (Oracle.get_state), and the
decoder that takes the reference's RGB frame back to those codes.

np_cells / np_snake_rows restate the contract of include/msnake.h in a dozen lines; decode_frame maps the frame's six
colours to the codes and cuts off the wall border, so that decode_frame(oracle.render()) is the expectation that owes
nothing to the helper either.  Nothing here asks the library under test.

A plain helper module like scripted_play / space_play; imported by tests/test_cells_host.py and tests/test_cells_gpu.py.
"""
import numpy as np

import board_states as bs

# the frame's colours (snake_multiple_test.py:35-58) -> the codes of the plane of the view they are drawn in
COLOURS = {(0, 0, 0): 0, (255, 0, 0): 1, (0, 204, 0): 2, (191, 242, 191): 3, (0, 51, 204): 4, (128, 154, 230): 5}
WALL = (255, 255, 255)
ROW_FIELDS = ("len", "head_c0", "head_c1", "v0", "v1", "grow_to", "alive", "in_dead")


def n_views(rules, n_snakes):
    """Views of the RGB frame: 3 for snake_env (0) and adversarial (2) whatever n_snakes is, n_snakes for new_world (1)."""
    return n_snakes if rules == 1 else 3


def np_cells(st, dim, n_snakes, rules, views):
    """uint8 [len(views), dim, dim]: the planes of `views` (ascending) in the frame's paint order, a later paint wins."""
    out = np.zeros((len(views), dim, dim), np.uint8)

    def paint(plane, c, code):
        if 0 <= c[0] < dim and 0 <= c[1] < dim:
            plane[c[0], c[1]] = code

    for plane, v in zip(out, views):
        for f in st["fruits"]:
            paint(plane, f, 1)
        for i in range(n_snakes):
            body = st["snakes"][i]
            if not body or (rules == 1 and not st["alive"][i]):
                continue
            for c in body:
                paint(plane, c, 2 if i == v else 4)
            paint(plane, body[0], 3 if i == v else 5)
    return out


def np_snake_rows(st, n_snakes):
    """int32 [n_snakes, 8]: len, head c0, head c1, v0, v1, grow_to, alive, in_dead; the head is (-2, -2) for an empty body."""
    rows = []
    for s in range(n_snakes):
        body = st["snakes"][s]
        head = body[0] if body else (-2, -2)
        rows.append([len(body), head[0], head[1], st["vels"][s][0], st["vels"][s][1], st["grow_to"][s],
                     int(bool(st["alive"][s])), int(bool(st["in_dead"][s]))])
    return np.array(rows, np.int32).reshape(n_snakes, 8)


def decode_frame(frame, views):
    """uint8 [..., dim + 2, dim + 2, 3 * n_views] native-scale frame(s) -> uint8 [..., len(views), dim, dim] codes.
    Asserts that the border is wall in every view and that no colour outside the table occurs inside it."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.shape[-1] % 3 == 0 and frame.shape[-3] == frame.shape[-2]
    planes = []
    for v in views:
        rgb = frame[..., 3 * v:3 * v + 3].astype(np.uint32)
        for edge in (rgb[..., 0, :, :], rgb[..., -1, :, :], rgb[..., :, 0, :], rgb[..., :, -1, :]):
            assert (edge == np.array(WALL, np.uint32)).all(), "the border is not wall"
        key = (rgb[..., 1:-1, 1:-1, 0] << 16) | (rgb[..., 1:-1, 1:-1, 1] << 8) | rgb[..., 1:-1, 1:-1, 2]
        plane = np.full(key.shape, 255, np.uint8)
        for (r, g, b), code in COLOURS.items():
            plane[key == ((r << 16) | (g << 8) | b)] = code
        assert (plane != 255).all(), ("a colour outside the six-colour table inside the border", np.unique(key[plane == 255])[:4])
        planes.append(plane)
    return np.stack(planes, axis=-3) if planes else np.zeros(frame.shape[:-3] + (0,) + tuple(s - 2 for s in frame.shape[-3:-1]), np.uint8)


def oracle_rows(ora):
    """int32 [num_envs, n_snakes, 8] from the oracle's own state."""
    return np.stack([np_snake_rows(ora.get_state(e), ora.n_snakes) for e in range(ora.num_envs)])


# ------------------------------------------------------------------------------------------ hand-built states
def _paint_order_states(dim, ns, fruit_list):
    """States in which the paint order decides a cell: a head under a later snake's body, fruits under bodies and
    heads, every head on one cell, heads outside the grid, empty bodies, a body that covers the whole board."""
    a, b, c, d = (0, 0), (1, 0), (dim - 1, dim - 1), (0, dim - 1)
    fr = lambda *cells: [cells[i % len(cells)] for i in range(fruit_list)]
    take = lambda bodies: [list(x) for x in bodies[:ns]] + [[]] * (ns - len(bodies[:ns]))
    out = [
        bs.state(take([[a], [b], [c, b, a, a], [d, c, a]]), fr(d)),        # heads of snakes 0 and 1 under the body of snake 2
        bs.state(take([[c, b, a, a], [d, c, a], [a], [b]]), fr(d)),        # ... and the later heads on top of an earlier body
        bs.state(take([[a, b], [c], [d], [b, a]]), fr(b, c, a, d)),        # fruits under a body and under heads
        bs.state(take([[a, b, b, b], [a], [a], [a, c]]), fr(a)),           # every head on one cell: the last snake's wins
        bs.state(take([[(-1, 0)], [(dim, dim - 1), c], [(0, -1), a], [(dim - 1, dim)]]), fr(a, c)),   # heads outside the grid
        bs.state(take([[], [], [], []]), fr(a, b, c, d)),                  # empty bodies: the fruits alone
        bs.state(take([[], [b, b], [], [a]]), fr(b)),
        bs.state(take([bs.line(dim * dim, dim)[::-1], [c], [a, d], [b]]), fr(c, a)),   # a body on every cell of the board
    ]
    return out


def _table_states(dim, ns, fruit_list):
    """States that vary what only the table shows: each of the five velocities (none and the four directions) on every
    snake in turn, and grow_to below, at and above the body length."""
    vels = [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1]]
    cells = [(0, 0), (1, 0), (dim - 1, dim - 1), (0, dim - 1)]
    out = []
    for k in range(5):
        bodies = [[cells[(s + k) % 4]] * (1 + (s + k) % 3) for s in range(ns)]
        st = bs.state(bodies, [cells[(k + i) % 4] for i in range(fruit_list)])
        st["vels"] = [list(vels[(k + s) % 5]) for s in range(ns)]
        st["grow_to"] = [(1, len(bodies[s]), len(bodies[s]) + 3 + k, 1000)[(k + s) % 4] for s in range(ns)]
        out.append(st)
    return out


def snake_env_states(dim, ns=3):
    """Hand-built snake_env states: the border / random / dense builders of the scripted and space tests (border and
    corner heads, heads at -1 and dim, stacked duplicates, empty bodies; bodies over 64 cells at dim >= 19) plus the
    paint-order states."""
    rng = np.random.default_rng([11, dim])
    states = bs.border_states(dim, ns, ns, rng) + bs.random_states(dim, ns, ns, rng, 20, dup=True)
    states += bs.dense_states(dim, ns, ns, rng, 12 if dim < 62 else 5)
    return states + _table_states(dim, ns, ns) + _paint_order_states(dim, ns, ns)


def new_world_states(dim, ns, nf):
    """new_world: every other state has dead snakes whose bodies are kept (alive False, in and out of dead_snakes)."""
    rng = np.random.default_rng([12, dim, ns, nf])
    states = bs.border_states(dim, ns, nf, rng)[::3] + bs.random_states(dim, ns, nf, rng, 16, dup=True)
    states += bs.dense_states(dim, ns, nf, rng, 8) if ns > 1 else []
    states += _table_states(dim, ns, nf) + _paint_order_states(dim, ns, nf)
    for k, st in enumerate(states[::2]):
        st["alive"] = [bool(rng.integers(0, 2)) for _ in range(ns)]
        if k % 4 == 0:
            st["alive"][k // 4 % ns] = False                     # (at least one dead snake in every eighth state)
        st["in_dead"] = [not al and bool(rng.integers(0, 2)) for al in st["alive"]]
    return states


def adversarial_states(dim, ns):
    """adversarial: fruit lists of 0 .. the list's capacity entries (past 64: the strided part), entries at -1 / dim."""
    rng = np.random.default_rng([13, dim, ns])
    fcap = (ns + ns * (dim * dim + 2) + 63) // 64 * 64           # the handle's fruit-list capacity
    states = []
    for n_list in (0, 1, 63, 64, 65, min(130, fcap - 3), fcap):
        states += bs.dense_states(dim, ns, n_list, rng, 3, fruit_lo=-1, fruit_hi=dim + 1) if ns > 1 else []
        states += _paint_order_states(dim, ns, n_list)[:5]
    edge = [(-1, -1), (dim, dim), (-1, 3), (3, dim), (dim, 0), (0, -1)]
    states.append(bs.state([[(2, 2)]] + [[]] * (ns - 1), edge * 12))    # 72 entries, every one outside the grid
    states += _table_states(dim, ns, 3)
    return states
