"""The states msnake_set_state accepts, stated in plain Python from the text of include/msnake.h (the comment above
msnake_get_state), and the hand-built states the tests step from.  Nothing here asks the library under test.

- cap(cfg), fcap(cfg): the two capacities as formulas of the configuration.
- accepts(cfg, words): None, or the reason (R_*) the header's ordered list of checks gives.
- rows(key): the case table of CFGS[key]: (name, builder, expected reason or None).  A builder turns a well-formed state
  taken from oracle play (base_words) into the words of the case.
- the scenarios of the steps after an install: an adversarial fruit list that ends exactly full or over, growth after
  the install, grow_to at its limits, bodies at the capacity guard.

A plain helper module like space_play and cells_play; imported by tests/test_state_domain_host.py and
tests/test_state_domain_gpu.py.
"""
import numpy as np

RULES = {"snake_env": 0, "new_world": 1, "adversarial": 2}
R_SHORT, R_SNAKES, R_FRUITS, R_CELL, R_LEN, R_SCALAR = 1, 2, 3, 4, 5, 6
# what the message of a refusal says (msnake_set_state checks the length and the low byte of word 7 on the host)
REASON_RE = {R_SHORT: "too short", R_SNAKES: r"snake count differs|state has -?\d+ snakes", R_FRUITS: "fruit count differs",
             R_CELL: "a cell lies outside", R_LEN: "a body length is outside", R_SCALAR: "a scalar field out of range"}
VELS = [(0, 0), (1, 0), (0, 1), (-1, 0), (0, -1)]

CFGS = {"S5": dict(rules="snake_env", dim=5, n_snakes=3, n_fruits=3, max_steps=2000),
        "N6": dict(rules="new_world", dim=6, n_snakes=4, n_fruits=5, max_steps=100),
        "A5": dict(rules="adversarial", dim=5, n_snakes=3, n_fruits=3, max_steps=2000),
        "S10": dict(rules="snake_env", dim=10, n_snakes=3, n_fruits=3, max_steps=2000),     # bodies over 64 pieces
        "A10": dict(rules="adversarial", dim=10, n_snakes=3, n_fruits=3, max_steps=2000),
        "S19": dict(rules="snake_env", dim=19, n_snakes=3, n_fruits=3, max_steps=2000)}     # a shape with kernels of its own
TABLE_KEYS = ("A10", "A5", "N6", "S10", "S5")                                               # the configurations rows() is run for


def roundup64(x):
    return (x + 63) // 64 * 64


def cap(cfg):
    """Pieces a body's storage holds: dim^2 + 2, under new_world at least max_steps + 2, in whole 64s."""
    need = cfg["dim"] ** 2 + 2
    if cfg["rules"] == "new_world":
        need = max(need, cfg["max_steps"] + 2)
    return roundup64(need)


def fcap(cfg):
    """Entries the adversarial fruit list holds: the n fruits and every body of one episode, in whole 64s."""
    ns = cfg["n_snakes"]
    return roundup64(ns + ns * (cfg["dim"] ** 2 + 2))


# ------------------------------------------------------------------------------------------ the model
def accepts(cfg, words):
    """The header's list, check by check and in its order: None if msnake_set_state takes `words`, else the reason."""
    w = [int(x) for x in words]
    n, dim, ns = len(w), cfg["dim"], cfg["n_snakes"]
    adv, nw = cfg["rules"] == "adversarial", cfg["rules"] == "new_world"
    if n < 8:
        return R_SHORT
    if w[7] not in (ns, ns | 0x100):
        return R_SNAKES
    if w[0] < 0 or w[3] < 0 or w[4] < 0:
        return R_SCALAR
    nfr = w[6]
    if (nfr < 0 or nfr > fcap(cfg)) if adv else nfr != cfg["n_fruits"]:
        return R_FRUITS
    if n < 8 + 2 * nfr:
        return R_SHORT
    lo, hi = (-1, dim) if adv else (0, dim - 1)
    if any(not (lo <= c <= hi) for c in w[8:8 + 2 * nfr]):
        return R_CELL
    k = 8 + 2 * nfr
    for _ in range(ns):
        if n < k + 6:
            return R_SHORT
        ln, v0, v1, grow, alive, in_dead = w[k:k + 6]
        if ln < 0 or ln > cap(cfg) - 2:
            return R_LEN
        if n < k + 6 + 2 * ln:
            return R_SHORT
        if (v0, v1) not in VELS or grow < 0:
            return R_SCALAR
        if (alive not in (0, 1) or in_dead not in (0, 1)) if nw else (alive, in_dead) != (1, 0):
            return R_SCALAR
        cells = w[k + 6:k + 6 + 2 * ln]
        if any(not (-1 <= c <= dim) for c in cells[:2]) or any(not (0 <= c < dim) for c in cells[2:]):
            return R_CELL
        k += 6 + 2 * ln
    return None


def canonical_len(cfg, words):
    """Words of an accepted state up to the end of its last snake: what msnake_get_state returns of it."""
    k = 8 + 2 * int(words[6])
    for _ in range(cfg["n_snakes"]):
        k += 6 + 2 * int(words[k])
    return k


# ------------------------------------------------------------------------------------------ words <-> a structure
class St:
    """The canonical words taken apart.  `nfr` and a snake's `len` are the DECLARED counts and may be set apart from
    the cells that follow (None = as many as there are)."""

    def __init__(self, words):
        w = [int(x) for x in words]
        self.hdr, self.nfr = w[:8], None
        nf = w[6]
        self.fruits = [[w[8 + 2 * i], w[9 + 2 * i]] for i in range(nf)]
        k = 8 + 2 * nf
        self.snakes = []
        for _ in range(w[7] & 0xFF):
            ln = w[k]
            self.snakes.append(dict(len=None, v=[w[k + 1], w[k + 2]], grow=w[k + 3], alive=w[k + 4], in_dead=w[k + 5],
                                    cells=[[w[k + 6 + 2 * i], w[k + 7 + 2 * i]] for i in range(ln)]))
            k += 6 + 2 * ln

    def flat(self):
        w = list(self.hdr)
        w[6] = len(self.fruits) if self.nfr is None else self.nfr
        for f in self.fruits:
            w += f
        for sn in self.snakes:
            w += [len(sn["cells"]) if sn["len"] is None else sn["len"], sn["v"][0], sn["v"][1], sn["grow"], sn["alive"],
                  sn["in_dead"]]
            for c in sn["cells"]:
                w += c
        return np.array(w, np.int32)

    def snake_start(self, s):
        """Index of snake s's first word."""
        k = 8 + 2 * len(self.fruits)
        for sn in self.snakes[:s]:
            k += 6 + 2 * len(sn["cells"])
        return k


def make_oracle(cfg, n, seed=11, **kw):
    from oracle.snake_oracle import Oracle
    return Oracle(n, dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"], rules=cfg["rules"], seed=seed,
                  max_steps=cfg["max_steps"], **kw)


def export(ora, e, finished_bit=True):
    """orc_export_state; with the oracle's `finished` where the product's words carry it (bit 8 of word 7)."""
    n = ora.L.orc_export_state(ora.h, e, None, 0)
    buf = np.zeros(n, np.int32)
    ora.L.orc_export_state(ora.h, e, buf.ctypes.data, n)
    if finished_bit and ora.finished(e):
        buf[7] |= 0x100
    return buf


def imports(ora, e, words):
    w = np.ascontiguousarray(words, np.int32)
    return int(ora.L.orc_import_state(ora.h, e, w.ctypes.data, len(w)))


_BASE = {}


def base_words(key):
    """A well-formed state from oracle play: the first env of 512, after two steps of random moves, in which every snake has
    at least two pieces and every head is on the board (without the auto reset: new_world ends an episode at every
    step on which the main snake is alive, and a reset body has one piece)."""
    if key not in _BASE:
        cfg = CFGS[key]
        ora = make_oracle(cfg, 512, seed=5, auto_reset=False)
        ora.reset()
        rs = np.random.default_rng(17)
        for _ in range(3):
            ora.step(rs.integers(1, 5, (512, cfg["n_snakes"])).astype(np.int32))
        for e in range(64):
            st = St(export(ora, e, False))
            if all(len(sn["cells"]) >= 2 and 0 <= min(sn["cells"][0]) and max(sn["cells"][0]) < cfg["dim"] for sn in st.snakes):
                _BASE[key] = st.flat()
                break
    assert accepts(CFGS[key], _BASE[key]) is None
    return _BASE[key].copy()


def walk(dim, n, start=0):
    """n cells of a walk to and fro along the rows of the board (a boustrophedon path and back): neighbours are one step
    apart, every cell is on the board, cells repeat once n exceeds dim^2."""
    path = []
    for y in range(dim):
        path += [[x, y] for x in (range(dim) if y % 2 == 0 else range(dim - 1, -1, -1))]
    there_and_back = path + path[-2:0:-1]
    return [list(there_and_back[(start + i) % len(there_and_back)]) for i in range(n)]


# ------------------------------------------------------------------------------------------ the case table
def rows(key):
    """[(name, builder() -> int32 words, expected R_* or None)] for CFGS[key]."""
    cfg = CFGS[key]
    dim, ns, rules = cfg["dim"], cfg["n_snakes"], cfg["rules"]
    adv, nw = rules == "adversarial", rules == "new_world"
    CAP, FCAP, last = cap(cfg), fcap(cfg), ns - 1
    out = []

    def row(name, expect, edit=None, post=None):
        def build():
            st = St(base_words(key))
            if edit:
                edit(st)
            w = st.flat()
            return np.asarray(post(w, st), np.int32) if post else w
        out.append((name, build, expect))

    def field(s, **kv):
        def edit(st):
            st.snakes[s].update(kv)
        return edit

    def hdr(i, v):
        def edit(st):
            st.hdr[i] = v
        return edit

    def cell(s, i, c0=None, c1=None):
        def edit(st):
            c = st.snakes[s]["cells"][i]
            st.snakes[s]["cells"][i] = [c[0] if c0 is None else c0, c[1] if c1 is None else c1]
        return edit

    def body(s, cells, **kv):
        def edit(st):
            st.snakes[s]["cells"] = [list(c) for c in cells]
            st.snakes[s].update(kv)
        return edit

    def both(*edits):
        def edit(st):
            for e in edits:
                e(st)
        return edit

    def fruit_edit(f):
        def edit(st):
            f(st.fruits)
        return edit

    row("base", None)
    # ---- buffer and counts
    row("n = 7", R_SHORT, post=lambda w, st: w[:7])
    row("cut inside the fruit list", R_SHORT, post=lambda w, st: w[:8 + 2 * len(st.fruits) - 1])
    row("cut inside the last snake's header", R_SHORT, post=lambda w, st: w[:st.snake_start(last) + 3])
    row("cut inside the first snake's header", R_SHORT, post=lambda w, st: w[:st.snake_start(0) + 5])
    row("cut inside the last cell", R_SHORT, post=lambda w, st: w[:-1])
    row("finished bit", None, hdr(7, ns | 0x100))
    row("snake count + 1", R_SNAKES, hdr(7, ns + 1))
    row("snake count - 1", R_SNAKES, hdr(7, ns - 1))
    row("stray bit 0x200", R_SNAKES, hdr(7, ns | 0x200))
    row("stray bit 0x10000", R_SNAKES, hdr(7, ns | 0x10000))
    row("stray sign bit", R_SNAKES, hdr(7, ns - (1 << 31)))
    row("surplus words", None, post=lambda w, st: np.concatenate([w, [7, -3, 1 << 30]]))
    if not adv:
        row("one fruit more", R_FRUITS, fruit_edit(lambda fr: fr.append([0, 0])))
        row("one fruit fewer", R_FRUITS, fruit_edit(lambda fr: fr.pop()))
        row("fruit at c0 = -1", R_CELL, fruit_edit(lambda fr: fr[0].__setitem__(0, -1)))
        row("fruit at c1 = dim", R_CELL, fruit_edit(lambda fr: fr[-1].__setitem__(1, dim)))
    else:
        edge = [[-1, -1], [dim, dim], [-1, dim], [dim, 0], [2, -1]]

        def full(st):
            # a full list: nothing may die on the next step (its pieces would not fit), so every body is empty
            st.fruits[:] = [list(edge[i % 5]) if i % 3 == 0 else [i % dim, i // dim % dim] for i in range(FCAP)]
            for sn in st.snakes:
                sn["cells"] = []
        row("list empty", None, fruit_edit(lambda fr: fr.clear()))
        row("list of fcap", None, full)
        row("list of fcap + 1", R_FRUITS, both(full, fruit_edit(lambda fr: fr.append([0, 0]))))

        def declared(v):
            def edit(st):
                st.nfr = v
            return edit
        row("list of -1", R_FRUITS, declared(-1))
        row("list of 65 with off-grid entries", None,
            fruit_edit(lambda fr: fr.__setitem__(slice(None), [list(edge[i % 5]) if i % 2 else [i % dim, 1] for i in range(65)])))
        row("list entry at c0 = -1", None, fruit_edit(lambda fr: fr[0].__setitem__(0, -1)))
        row("list entry at c1 = dim", None, fruit_edit(lambda fr: fr[-1].__setitem__(1, dim)))
        row("list entry at c0 = -2", R_CELL, fruit_edit(lambda fr: fr[0].__setitem__(0, -2)))
        row("list entry at c1 = dim + 1", R_CELL, fruit_edit(lambda fr: fr[-1].__setitem__(1, dim + 1)))
    # ---- body cells and lengths
    row("head at c0 = -1", None, cell(0, 0, c0=-1))
    row("head at c0 = dim", None, cell(last, 0, c0=dim))
    row("head at c1 = -1", None, cell(1 % ns, 0, c1=-1))
    row("head at c1 = dim", None, cell(0, 0, c1=dim))
    row("head at c0 = -2", R_CELL, cell(0, 0, c0=-2))
    row("head at c1 = dim + 1", R_CELL, cell(last, 0, c1=dim + 1))
    row("piece 1 at c0 = -1", R_CELL, cell(0, 1, c0=-1))
    row("piece 1 at c1 = dim", R_CELL, cell(last, 1, c1=dim))
    row("len 0", None, body(last, []))
    row("every body empty", None, both(*[body(s, []) for s in range(ns)]))
    # (grow_to stays at or below the length: the body does not grow on the step that follows)
    row("len cap - 2", None, body(last, walk(dim, CAP - 2, 3), grow=3))
    row("len cap - 1", R_LEN, body(last, walk(dim, CAP - 1, 3), grow=3))
    row("len cap - 1 in the first snake", R_LEN, body(0, walk(dim, CAP - 1, 3), grow=3))
    row("len -1", R_LEN, field(0, len=-1))
    row("len 65536 + 2", R_LEN, field(last, len=65538))
    row("duplicate on the head", None, lambda st: st.snakes[0]["cells"].insert(1, list(st.snakes[0]["cells"][0])))
    if CAP - 2 >= 70:
        long = walk(dim, 70, 5)
        row("body of 70", None, body(1, long, grow=3))
        for i in (63, 64, 65, 69):
            row(f"piece {i} of 70 at c0 = -1", R_CELL, both(body(1, long, grow=3), cell(1, i, c0=-1)))
            row(f"piece {i} of 70 at c1 = dim", R_CELL, both(body(1, long, grow=3), cell(1, i, c1=dim)))
    # ---- scalars: the nearest illegal value, and the nearest legal one next to it
    for name, i in (("t", 0), ("spare_fruits", 3), ("ep_len", 4)):
        row(f"{name} = -1", R_SCALAR, hdr(i, -1))
        row(f"{name} = 0", None, hdr(i, 0))
        row(f"{name} = -2^31", R_SCALAR, hdr(i, -(1 << 31)))
    row("t = max_steps + 2", None, hdr(0, cfg["max_steps"] + 2))
    row("ctr just below 2^64, ep_return -7.5", None, both(hdr(1, -1), hdr(2, -2), hdr(5, int(np.array([-7.5], np.float32).view(np.int32)[0]))))
    row("grow_to = -1", R_SCALAR, field(0, grow=-1))
    row("grow_to = -1 in the last snake", R_SCALAR, field(last, grow=-1))
    # (new_world pops once per fruit while len >= grow_to: the reference itself needs len > n_fruits at grow_to 0)
    row("grow_to = 0", None, body(0, walk(dim, 8, 2), grow=0))
    row("grow_to = 2^31 - 64", None, field(last, grow=(1 << 31) - 64))      # (a fruit adds 2: no overflow on the step after)
    for v in VELS:
        row(f"velocity {v}", None, field(1 % ns, v=list(v)))
    for v in ((1, 1), (-1, 1), (2, 0), (0, 2), (-2, 0), (0, -2), (1, -1), (256, 0)):
        row(f"velocity {v}", R_SCALAR, field(1 % ns, v=list(v)))
    if nw:
        for a, d in ((0, 0), (0, 1), (1, 0), (1, 1)):
            row(f"alive {a}, in_dead {d}", None, field(last, alive=a, in_dead=d))
        for kv in (dict(alive=2), dict(alive=-1), dict(in_dead=2), dict(in_dead=-1), dict(alive=256)):
            row(f"{kv}", R_SCALAR, field(0, **kv))
    else:
        row("alive 1, in_dead 0", None, field(last, alive=1, in_dead=0))
        for kv in (dict(alive=0), dict(alive=2), dict(in_dead=1), dict(in_dead=-1), dict(alive=0, in_dead=1)):
            row(f"{kv}", R_SCALAR, field(last, **kv))
    # ---- which snake the fault sits in, and which of two faults is reported: the first in the header's order
    row("bad cell in the first snake only", R_CELL, cell(0, 1, c1=-1))
    row("bad cell in the last snake only", R_CELL, cell(last, 1, c0=dim))
    row("bad length first, bad cell later", R_LEN, both(field(0, len=-1), cell(last, 1, c0=dim)))
    row("bad cell first, bad length later", R_CELL, both(cell(0, 1, c0=dim), body(last, walk(dim, CAP - 1), grow=3)))
    row("bad scalar first, bad cell in the same snake", R_SCALAR, both(field(0, grow=-1), cell(0, 1, c0=dim)))
    row("bad t, bad fruit count", R_SCALAR, both(hdr(0, -1), (lambda st: setattr(st, "nfr", -1))))
    row("bad snake count, bad t", R_SNAKES, both(hdr(7, ns | 0x200), hdr(0, -1)))
    row("bad fruit count, bad snake", R_FRUITS, both((lambda st: setattr(st, "nfr", -1)), field(0, grow=-1)))
    return out


def make_blob(cfg, env_words):
    """A msnake_get_state_all blob (version 2) holding env_words[e] as env e's words; layout: include/msnake.h."""
    offs = np.zeros(len(env_words) + 1, np.uint64)
    offs[1:] = np.cumsum([len(w) for w in env_words])
    head = np.array([0x5453534D, 2, len(env_words), cfg["dim"], cfg["n_snakes"], cfg["n_fruits"], RULES[cfg["rules"]], 0],
                    np.uint32)
    words = np.concatenate([np.asarray(w, np.int32) for w in env_words])
    return np.frombuffer(head.tobytes() + np.uint64(len(words)).tobytes() + offs.tobytes() + words.tobytes(), np.uint8).copy()


# ------------------------------------------------------------------------------------------ the steps after
def state_words(ns, fruits, snakes, t=0, ctr=40, spare=0, finished=False):
    """snakes: [(cells, (v0, v1), grow_to)] or with (alive, in_dead) appended."""
    w = [t, ctr, 0, spare, t, 0, len(fruits), ns | (0x100 if finished else 0)]
    for f in fruits:
        w += list(f)
    assert len(snakes) == ns
    for sn in snakes:
        cells, v, grow = sn[:3]
        alive, in_dead = sn[3:] if len(sn) > 3 else (1, 0)
        w += [len(cells), v[0], v[1], grow, alive, in_dead]
        for c in cells:
            w += list(c)
    return np.array(w, np.int32)


def _filler(n, dim=5):
    """n list entries on rows 1 and 3 and on the wall ring at c0 = -1: no snake of the scenarios below ever heads there."""
    spots = [[x, y] for y in (1, 3) for x in range(dim)] + [[-1, y] for y in range(dim)]
    return [list(spots[i % len(spots)]) for i in range(n)]


def adv_wall(over):
    """A5 (fcap 128): snakes 1 and 2, four pieces each, run into the wall at c0 = dim; each eats the list entry that lies
    there and dies with five pieces, while the main snake rests.  The list holds 118 + over entries, so it ends at
    fcap + over.  spare_fruits > 0: the eaten entries stay.  -> (words, action row, pieces that die, steps)"""
    cfg = CFGS["A5"]
    assert fcap(cfg) == 128 and cap(cfg) == 64
    fruits = [[5, 2], [5, 4]] + _filler(fcap(cfg) - 10 + over - 2)
    snakes = [([[2, 0], [1, 0]], (0, 0), 3),
              ([[4, 2], [3, 2], [2, 2], [1, 2]], (1, 0), 4),
              ([[4, 4], [3, 4], [2, 4], [1, 4]], (1, 0), 4)]
    return state_words(3, fruits, snakes, t=7, spare=5), [0, 0, 0], 10, 1


def adv_full_neighbour():
    """A5: a list of exactly fcap entries that every step leaves alone -- three resting one-piece snakes -- and
    msnake_get_state shows entry by entry: where entries written past the end of the previous env's list would land."""
    cfg = CFGS["A5"]
    fruits = [[(3 * i) % 7 - 1, (5 * i) % 7 - 1] for i in range(fcap(cfg))]
    snakes = [([[0, 0]], (0, 0), 3), ([[2, 2]], (0, 0), 3), ([[4, 4]], (0, 0), 3)]
    return state_words(3, fruits, snakes, t=2, spare=0)


def adv_growth():
    """A5: at the install n_fruits_cur + the sum of the body lengths is exactly fcap (121 + 1 + 3 + 3).  Snakes 1 and 2
    each eat an entry on their first step -- spare_fruits is 2, so both entries stay --, grow from 3 to 5 pieces and run
    into the wall: snake 2 on step 3 (the list reaches 126), snake 1 on step 4 (131 = fcap + 3).
    -> (words, action row, list length after each step)"""
    cfg = CFGS["A5"]
    fruits = [[2, 2], [3, 4]] + _filler(fcap(cfg) - 7 - 2)
    snakes = [([[2, 0]], (0, 0), 3),
              ([[1, 2], [0, 2], [0, 3]], (1, 0), 3),
              ([[2, 4], [1, 4], [0, 4]], (1, 0), 3)]
    w = state_words(3, fruits, snakes, t=1, spare=2)
    assert int(w[6]) + 1 + 3 + 3 == fcap(cfg)
    return w, [0, 0, 0], [121, 121, 126, 131]


def grow_limits(key, eat):
    """One snake at grow_to = 0, one at grow_to = len, both moving; a third moves onto a fruit (eat) or not.  Under
    snake_env every step takes the vector update; under adversarial and new_world a step on which some snake eats
    takes the sequential one.  -> (words, action row)"""
    cfg = CFGS[key]
    dim, ns, nf = cfg["dim"], cfg["n_snakes"], cfg["n_fruits"]
    a = [[c0, 0] for c0 in range(dim - 3, -1, -1)] + [[c0, 1] for c0 in range(dim)]      # two free cells ahead of the head
    snakes = [(a[:8] if cfg["rules"] == "new_world" else a[:3], (1, 0), 0),     # (new_world pops once per fruit: len > n_fruits)
              ([[1, 2], [0, 2], [0, 3]], (1, 0), 3),
              ([[1, 4], [0, 4]], (1, 0), 3)]
    if ns == 4:   # new_world ends the episode while the main snake is alive: it is dead and empty here
        snakes.insert(0, ([], (0, 0), 3, 0, 1))
    fruits = [[2, 4] if eat else [dim - 1, 3]] + [[dim - 1, 3]] * (nf - 1)
    return state_words(ns, fruits, snakes, t=3), [0] * ns


def grow_limits_steps(key):
    """Steps the grow_limits state can be played for.  new_world pops once per fruit while len >= grow_to, so at grow_to
    0 the reference pops an empty list as soon as the body is no longer than n_fruits: one step from eight pieces."""
    return 1 if CFGS[key]["rules"] == "new_world" else 2


def body_guard(key):
    """A body two pieces below the capacity with grow_to 10^6: it reaches cap - 1 on the first step and would pass it on
    the second.  N6 (cap 128): snake 1 is a walk of 126 in-grid cells with duplicates that goes on along free cells;
    the main snake is dead and empty, or the episode would end at once (new_world ends while it is alive).  S5 / A5
    (cap 64): the main snake is 62 pieces stacked on one cell, and its head moves away along a free row.
    -> (words, action row, index of the long snake)"""
    cfg = CFGS[key]
    dim, ns, nf, CAP = cfg["dim"], cfg["n_snakes"], cfg["n_fruits"], cap(cfg)
    if cfg["rules"] == "new_world":
        assert CAP == 128
        path = walk(dim, dim * dim)                       # the 36 cells, each once
        back = path[20::-1]                               # from cell 20 back to cell 0 ...
        cells = (back + (path[1:21] + path[19::-1]) * 4)[:CAP - 2]     # ... and to and fro over cells 0..20
        assert all(abs(p[0] - q[0]) + abs(p[1] - q[1]) == 1 for p, q in zip(cells, cells[1:]))
        v = (path[20][0] - path[19][0], path[20][1] - path[19][1])
        acts = [{(1, 0): 1, (0, 1): 2, (-1, 0): 3, (0, -1): 4}[(q[0] - p[0], q[1] - p[1])] for p, q in zip(path[20:], path[21:])]
        snakes = [([], (0, 0), 3, 0, 1), (cells, v, 10 ** 6), ([], (0, 0), 3, 0, 1), ([], (0, 0), 3, 0, 1)]
        return state_words(ns, path[31:31 + nf], snakes, t=0), [[0, a, 0, 0] for a in acts[:7]], 1
    assert CAP == 64
    snakes = [([[0, 2]] * (CAP - 2), (1, 0), 10 ** 6), ([[4, 0]], (0, 0), 3), ([[4, 4]], (0, 0), 3)]
    return state_words(ns, [[0, 0], [2, 0], [2, 4]], snakes, t=0), [[0, 0, 0]] * 7, 0


def turn_back(key):
    """Heads installed one step outside the grid that turn back into it: snake 0 runs along the outside of the wall at
    c0 = -1 and turns in, snake 1 does the same at c1 = dim.  Both live on, and the cell outside the grid stays in the
    body, as piece 1 and further back, for as long as the body keeps it: the reference draws the wall over it.
    -> (words, action rows)"""
    cfg = CFGS[key]
    dim, ns, nf = cfg["dim"], cfg["n_snakes"], cfg["n_fruits"]
    nw = cfg["rules"] == "new_world"
    snakes = [([[-1, 3], [0, 2], [0, 1]], (0, 1), 6), ([[3, dim], [2, dim - 1], [1, dim - 1]], (1, 0), 6)]
    snakes += [([[dim - 1, 0]], (0, 0), 3)] * (ns - 2)
    if nw:   # (the episode ends while the main snake is alive: it is dead and empty, and snakes 1 and 2 turn back)
        snakes = [([], (0, 0), 3, 0, 1)] + snakes[:ns - 1]
    fruits = [[dim - 1, dim - 1]] * nf
    rows = [([1, 4] + [0] * (ns - 2)), [0] * ns, [0] * ns]
    if nw:
        rows = [[0] + r[:ns - 1] for r in rows]
    return state_words(ns, fruits, snakes, t=5), rows


# ------------------------------------------------------------------------------------------ canonical words, read and compared
def blob_words(blob):
    """Per-env canonical words of a get_state_all blob (layout: include/msnake.h)."""
    b = np.ascontiguousarray(blob, dtype=np.uint8)
    n = int(b[8:12].view(np.int32)[0])
    offs = b[40:40 + 8 * (n + 1)].view(np.uint64).astype(np.int64)
    w = b[40 + 8 * (n + 1):].view(np.int32)
    assert offs[-1] == len(w)
    return [w[offs[e]:offs[e + 1]].copy() for e in range(n)]


def assert_words(got, want, what=None):
    assert len(got) == len(want)
    bad = [e for e, (g, w) in enumerate(zip(got, want)) if not np.array_equal(g, w)]
    assert not bad, (what, bad[:8], got[bad[0]][:16], want[bad[0]][:16])


# ------------------------------------------------------------------------------------------ the header's hash, on plain ints
_M64 = (1 << 64) - 1
HASH_BOARD_SKIPS = (0, 1, 2, 4, 5)   # t, the draw counter, ep_len, ep_return


def _mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def header_hash(words, board=False, clear_finished=True):
    """include/msnake.h, msnake_hash_states, restated on Python integers: the sum over the selected i of
    mix64((i + 1) << 32 | uint32(w[i])) mod 2^64, as the int64 the device tensor holds.  board: words 0, 1, 2, 4, 5 are
    left out and bit 8 of word 7 is cleared (clear_finished=False: the defect of a BOARD hash that keeps it)."""
    h = 0
    for i, w in enumerate(words):
        w = int(w) & 0xFFFFFFFF
        if board and i in HASH_BOARD_SKIPS:
            continue
        if board and i == 7 and clear_finished:
            w &= ~0x100
        h = (h + _mix64((i + 1) << 32 | w)) & _M64
    return h - (1 << 64) if h >> 63 else h
