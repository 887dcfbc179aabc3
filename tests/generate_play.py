"""msnake_generate_states restated in NumPy from the text of include/msnake.h, the scenarios its tests run, and the table
of the README (python tests/generate_play.py).  Nothing here asks the library under test: the random numbers are the
oracle's philox_u32 under the generator's key, everything else is plain Python.

- np_generate(cfg, lengths, mask, salt, compact, ctr, word3) -> (rows, count, got)
- cfg: dict(rules=, dim=, n_snakes=, n_fruits=, max_steps=, seed=, env_id_base=, num_envs=), rules by name
- CASES: the configurations and requests of tests/test_generate_gpu.py
- reach_share / safe_share: the numbers of the table

A plain helper module like playout_play and state_domain; imported by tests/test_generate_host.py and
tests/test_generate_gpu.py.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

M64 = (1 << 64) - 1
GEN_TAG = 0x67656E6572617465  # "generate"
MOVES = ((1, 0), (0, 1), (-1, 0), (0, -1))  # actions 1..4


def mix64(z):
    """The splitmix64 finaliser (include/msnake.h, msnake_hash_states) on a Python int."""
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def gen_seed(seed, salt):
    return mix64((seed & M64) ^ mix64((salt & M64) ^ GEN_TAG))


class _Stream:
    """Draw j of global env G under the generator's key; counts what it hands out."""

    def __init__(self, gseed, env_id):
        from oracle.snake_oracle import philox_u32
        self._u32, self.gseed, self.env_id, self.draws = philox_u32, gseed, env_id, 0

    def randint(self, n):
        u = self._u32(self.gseed, self.env_id, self.draws)
        self.draws += 1
        return (u * n) >> 32


def make_cfg(rules, dim, n_snakes, num_envs, seed=1, env_id_base=0, n_fruits=None, max_steps=2000):
    return dict(rules=rules, dim=dim, n_snakes=n_snakes, n_fruits=n_snakes if n_fruits is None else n_fruits,
                max_steps=max_steps, seed=seed, env_id_base=env_id_base, num_envs=num_envs)


def lengths_array(cfg, lengths):
    """An int, S ints or an [E, >= S] array -> int64 [E, S]."""
    E, S = cfg["num_envs"], cfg["n_snakes"]
    a = np.asarray(lengths, np.int64)
    if a.ndim == 0:
        a = np.full((E, S), int(a), np.int64)
    elif a.ndim == 1:
        assert a.shape == (S,), a.shape
        a = np.tile(a, (E, 1))
    assert a.ndim == 2 and a.shape[0] == E and a.shape[1] >= S, a.shape
    return a[:, :S]


def _kth_free(occ, k):
    """The k-th unoccupied cell in the order x = c1 * dim + c0; occ is indexed [c0, c1]."""
    dim = occ.shape[0]
    x = int(np.flatnonzero(~occ.T.reshape(-1))[k])   # (occ.T[c1, c0] flattens to c1 * dim + c0)
    return x % dim, x // dim


def generate_one(dim, n_fruits, request, stream, compact):
    """One env's position: (fruits, bodies, draws taken).  `request`: the S requested lengths as they were passed."""
    occ = np.zeros((dim, dim), bool)
    free = lambda c: 0 <= c[0] < dim and 0 <= c[1] < dim and not occ[c[0], c[1]]  # noqa: E731
    around = lambda c: [(c[0] + d0, c[1] + d1) for d0, d1 in MOVES]  # noqa: E731
    bodies = []
    for s, L in enumerate(int(x) for x in request):
        L = max(L, 0)
        if s == 0:
            L = max(L, 1)
        body = []
        nfree = int((~occ).sum())
        if L > 0 and nfree > 0:
            end = _kth_free(occ, stream.randint(nfree))
            occ[end] = True
            body.append(end)
            while len(body) < L:
                cand = [c for c in around(end) if free(c)]
                if not cand:
                    break
                if compact:
                    onward = [sum(free(c2) for c2 in around(c)) for c in cand]
                    cand = [c for c, n in zip(cand, onward) if n == min(onward)]
                end = cand[0 if len(cand) == 1 else stream.randint(len(cand))]
                occ[end] = True
                body.append(end)
        bodies.append(body)
    fruits = []
    for _ in range(n_fruits):
        nfree = int((~occ).sum())
        if nfree == 0:
            fruits.append((0, 0))
            continue
        f = _kth_free(occ, stream.randint(nfree))
        occ[f] = True
        fruits.append(f)
    return fruits, bodies, stream.draws


def position_words(n_snakes, fruits, bodies, ctr=0, word3=0):
    w = [0, ctr & 0xFFFFFFFF, (ctr >> 32) & 0xFFFFFFFF, word3, 0, 0, len(fruits), n_snakes]
    for f in fruits:
        w += [f[0], f[1]]
    for body in bodies:
        v = (body[0][0] - body[1][0], body[0][1] - body[1][1]) if len(body) > 1 else (0, 0)
        w += [len(body), v[0], v[1], max(len(body), 3), 1, 0]
        for c in body:
            w += [c[0], c[1]]
    return np.array(w, np.int64).astype(np.uint32).view(np.int32)   # (a counter half of 2^31 or more wraps into the int32)


def np_generate(cfg, lengths, mask=None, salt=0, compact=True, ctr=0, word3=0, draws_out=None):
    """Section "The position of one selected env" of msnake_generate_states for every env `mask` selects (None: all).
    ctr / word3: the envs' current draw counters and words 3, an int or one per env.  Returns (rows, count, got): rows[e]
    the env's int32 words or None where the mask is 0, count int64 [E] (-1 where unselected), got int64 [E, S] (-1
    likewise).  draws_out, a list, receives the number of draws each selected env took."""
    assert cfg["rules"] in ("snake_env", "adversarial"), cfg["rules"]
    E, S = cfg["num_envs"], cfg["n_snakes"]
    req = lengths_array(cfg, lengths)
    sel = np.ones(E, bool) if mask is None else np.asarray(mask) != 0
    ctr = np.broadcast_to(np.asarray(ctr, np.uint64), (E,))
    word3 = np.broadcast_to(np.asarray(word3, np.int64), (E,))
    gseed = gen_seed(cfg["seed"], salt)
    rows, count, got = [None] * E, np.full(E, -1, np.int64), np.full((E, S), -1, np.int64)
    for e in range(E):
        if not sel[e]:
            continue
        fruits, bodies, draws = generate_one(cfg["dim"], cfg["n_fruits"], req[e], _Stream(gseed, cfg["env_id_base"] + e), compact)
        rows[e] = position_words(S, fruits, bodies, int(ctr[e]), int(word3[e]))
        count[e] = len(rows[e])
        got[e] = [len(b) for b in bodies]
        if draws_out is not None:
            draws_out.append(draws)
    return rows, count, got


def row_state(row):
    """A row as the canonical state dict the oracle and the scripted policies read."""
    from oracle.snake_oracle import flat_to_state
    return flat_to_state(row)


# ------------------------------------------------------------------------------------------ the GPU tests' cases
def mixed_requests(E, rng):
    """Per-env mixed requests for three snakes: 0 for snakes 1 and 2, 0 and -3 for snake 0, and 1 000 are all in."""
    req = rng.integers(1, 40, (E, 3)).astype(np.int32)
    req[0] = (0, 5, 5)
    req[1] = (-3, 0, 7)
    req[2] = (4, 0, 0)
    req[3] = (1000, 3, 3)
    req[4] = (6, 1000, 0)
    req[5] = (2, 2, 1000)
    return req


# name -> (cfg, requests); the 19x19x3 snake_env configuration is one with step kernels compiled for its shape
def cases():
    rng = np.random.default_rng(20)
    c = {}
    c["S6"] = (make_cfg("snake_env", 6, 3, 67, seed=3, env_id_base=5), (10, 10, 10))
    c["S10mixed"] = (make_cfg("snake_env", 10, 3, 40, seed=4), mixed_requests(40, rng))
    c["S19"] = (make_cfg("snake_env", 19, 3, 12, seed=5, env_id_base=100),
                np.array([[40, 40, 40], [100, 100, 100], [200, 200, 200], [200, 40, 100]] * 3, np.int32))
    c["full3x3"] = (make_cfg("snake_env", 3, 2, 16, seed=6), (9, 5))
    c["full2x2"] = (make_cfg("snake_env", 2, 1, 8, seed=7), 4)
    c["S62"] = (make_cfg("snake_env", 62, 1, 3, seed=8), 3844)
    for n in (1, 3, 257):
        c[f"n{n}"] = (make_cfg("snake_env", 8, 2, n, seed=9, env_id_base=2 ** 33), (12, 6))
    return c


# ------------------------------------------------------------------------------------------ the table
def reach_share(cfg, request, compact, salt=0):
    """The share of snakes with a request > 0 that reach it."""
    req = lengths_array(cfg, request)
    _, _, got = np_generate(cfg, request, salt=salt, compact=compact)
    want = np.maximum(req, 0)
    want[:, 0] = np.maximum(want[:, 0], 1)
    asked = want > 0
    return float((got[asked] == want[asked]).mean())


def has_safe_move(dim, bodies):
    """Every live snake has a move whose target lies in the grid and in no body."""
    used = {c for b in bodies for c in b}
    for b in bodies:
        if b and not any(0 <= x < dim and 0 <= y < dim and (x, y) not in used
                         for x, y in ((b[0][0] + d0, b[0][1] + d1) for d0, d1 in MOVES)):
            return False
    return True


def safe_share(cfg, request, compact, salt=0):
    rows, _, _ = np_generate(cfg, request, salt=salt, compact=compact)
    states = [row_state(r) for r in rows]
    return float(np.mean([has_safe_move(cfg["dim"], [[tuple(c) for c in b] for b in st["snakes"]]) for st in states]))


TABLE = [(10, 3, (3, 10, 20, 30)), (19, 3, (3, 40, 100, 150))]


def table(num_envs=256):
    out = ["| board | request | reached, compact | reached, plain | safe move, compact | safe move, plain |", "|---|---|---|---|---|---|"]
    for dim, ns, reqs in TABLE:
        cfg = make_cfg("snake_env", dim, ns, num_envs, seed=1)
        for L in reqs:
            r1, r0 = reach_share(cfg, L, True), reach_share(cfg, L, False)
            s1, s0 = safe_share(cfg, L, True), safe_share(cfg, L, False)
            out.append(f"| {dim}x{dim}x{ns} | {L} | {r1:.2f} | {r0:.2f} | {s1:.2f} | {s0:.2f} |")
    return "\n".join(out)


if __name__ == "__main__":
    print(table())
