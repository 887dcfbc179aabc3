"""Exploring play, stated on the CPU oracle: include/msnake.h, msnake_explore_actions and msnake_playout_explore, restated
without the library.

explore_draw is the documented stream (oracle.snake_oracle.philox_u32 under the key mix64(xseed ^ ctr)); np_explore_actions
forms every snake's base action and candidate set from the helpers that already state them (scripted_play's open moves
and policies, fates_play.np_fates / wary_choice) and applies the rule; np_playout_explore is playout_play.np_playout's loop
with the rule applied per step, on the state's own t and ctr.  scenario() holds the exploring plays the tests compare the
library with; reference() computes each once per process.  Nothing here asks the library under test.

A plain helper module in the style of playout_play, which it imports and does not edit; imported by
tests/test_explore_host.py and tests/test_explore_gpu.py.
"""
import functools

import numpy as np

import fates_play as fp
import playout_play as pp
import scripted_play as sp
from generate_play import M64, mix64

TAG = 0x6578706C6F726521   # "explore!"
ONE = 65536                # eps_q16 of probability 1
WARY = "wary_greedy"


def q16(x):
    """A probability, or one per snake -> eps_q16 as the Python layer forms it."""
    return [int(round(float(v) * ONE)) for v in x] if isinstance(x, (list, tuple)) else int(round(float(x) * ONE))


def explore_seed(seed, salt):
    return mix64((seed & M64) ^ mix64((salt & M64) ^ TAG))


def explore_draw(seed, salt, G, t, ctr, s):
    """(u0, u1) of snake s of the env with global id G in a state with step counter t and draw counter ctr."""
    from oracle.snake_oracle import philox_u32
    k64 = mix64(explore_seed(seed, salt) ^ (int(ctr) & M64))
    j = 8 * (int(t) & 0xFFFFFFFF) + 2 * s
    return philox_u32(k64, G & M64, j), philox_u32(k64, G & M64, j + 1)


def candidates(st, dim, n_snakes, policies):
    """C_s of every snake as a list of moves in the order 1, 2, 3, 4."""
    policies = pp.per_snake(policies, n_snakes)
    open_mask = sp.np_safe_mask(st, dim, n_snakes)
    wary_mask = fp.np_fates(st, dim, n_snakes)[3] if WARY in policies else None
    out = []
    for s in range(n_snakes):
        moves = (1, 2, 3, 4)
        if policies[s] == WARY:
            out.append([a for a in moves if wary_mask[s, 1] >> a & 1] or [a for a in moves if wary_mask[s, 0] >> a & 1])
        else:
            out.append([a for a in moves if open_mask[s] >> a & 1])
    return out


def explore_row(st, G, cfg, policies, eps_q16, salt):
    """One env: (actions [S], explored [S], n [S]) of the rule on state st."""
    S, dim = cfg["n_snakes"], cfg["dim"]
    policies = pp.per_snake(policies, S)
    eps = [eps_q16] * S if isinstance(eps_q16, (int, np.integer)) else list(eps_q16)
    act = pp.policy_actions(st, dim, S, policies)
    cand = candidates(st, dim, S, policies)
    explored = [0] * S
    for s in range(S):
        n = len(cand[s])
        if eps[s] > 0 and n > 0:
            u0, u1 = explore_draw(cfg["seed"], salt, G, st.get("t", 0), st.get("ctr", 0), s)
            if (u0 >> 16) < eps[s]:
                act[s], explored[s] = cand[s][(u1 * n) >> 32], 1
    return act, explored, [len(c) for c in cand]


def np_explore_actions(cfg, states, policies, eps_q16, salt=0):
    """states: canonical dicts, env e being global env env_id_base + e.  Returns (actions int32 [E, S], explored uint8 [E, S],
    n int32 [E, S]: the size of every candidate set)."""
    rows = [explore_row(st, cfg["env_id_base"] + e, cfg, policies, eps_q16, salt) for e, st in enumerate(states)]
    return (np.array([r[0] for r in rows], np.int32).reshape(len(states), -1), np.array([r[1] for r in rows], np.uint8).reshape(len(states), -1),
            np.array([r[2] for r in rows], np.int32).reshape(len(states), -1))


def np_playout_explore(cfg, states, policies, eps_q16, salt, n_steps, first=None, first_snakes=None, trace=None):
    """playout_play.np_playout with the exploration rule applied in every step; the same arguments and the same result.
    `trace`, a dict, receives draws [E] (respawn draws consumed), explored and n [K, E, S] (0 behind an env's end)."""
    from oracle.snake_oracle import state_to_flat
    E, S = len(states), cfg["n_snakes"]
    policies = pp.per_snake(policies, S)
    forced = set(range(S)) if first_snakes is None else {int(s) for s in first_snakes}
    ora = sp.make_oracle(dict(cfg, num_envs=E), auto_reset=False)
    ora.reset()
    for e, st in enumerate(states):
        ora.set_state(e, st)
    read = sp._StateReader(ora)
    out = dict(steps=np.zeros(E, np.int32), end=np.zeros(E, np.uint8), ret=np.zeros((E, S), np.float32),
               info=np.zeros((E, S, 4), np.int32), words=[None] * E, count=np.zeros(E, np.int32))
    if trace is not None:
        trace.update(draws=np.zeros(E, np.int64), explored=np.zeros((n_steps, E, S), np.uint8), n=np.zeros((n_steps, E, S), np.int32))
    cur = [read(e) for e in range(E)]
    active = []
    for e, st in enumerate(states):
        if st.get("finished"):
            out["end"][e] = pp.FINISHED
            out["words"][e] = state_to_flat(dict(cur[e], finished=True), S)
        else:
            active.append(e)
    for k in range(1, n_steps + 1):
        if not active:
            break
        act = np.zeros((E, S), np.int32)
        for e in active:
            act[e], explored, n = explore_row(cur[e], cfg["env_id_base"] + e, cfg, policies, eps_q16, salt)
            if trace is not None:
                trace["explored"][k - 1, e], trace["n"][k - 1, e] = explored, n
            if k == 1 and first is not None:
                for s in forced:
                    act[e, s] = int(first[e][s])
            if k == 1:
                out["info"][e, :, 3] = act[e]
        _, _, done, *_ = ora.step(act, want_obs=False)
        still = []
        for e in active:
            before, after = cur[e], read(e)
            cur[e] = after
            for s in range(S):
                was = len(before["snakes"][s]) > 0
                died = was and len(after["snakes"][s]) == 0
                ate = max(0, int(after["grow_to"][s]) - int(before["grow_to"][s])) >> 1
                out["ret"][e, s] += np.float32(-1.0 if died else ate)
                out["info"][e, s, 0] += ate
                out["info"][e, s, 1] += len(after["snakes"][s]) > 0
                if died:
                    out["info"][e, s, 2] = k
            out["steps"][e] = k
            if done[e]:
                out["end"][e] = pp.DEAD if not after["snakes"][0] else pp.CAP
                out["words"][e] = state_to_flat(dict(after, finished=True), S)
            else:
                still.append(e)
        active = still
    for e in active:
        out["end"][e] = pp.HORIZON
        out["words"][e] = state_to_flat(cur[e], S)
    for e in range(E):
        out["count"][e] = len(out["words"][e])
        if trace is not None:
            w = out["words"][e]
            trace["draws"][e] = ((int(w[1]) & 0xFFFFFFFF) | ((int(w[2]) & 0xFFFFFFFF) << 32)) - int(states[e].get("ctr", 0))
    return out


def same_result(a, b):
    """Two results of np_playout / np_playout_explore hold the same six outputs."""
    return (all(np.array_equal(a[k], b[k]) for k in ("steps", "end", "ret", "info", "count")) and
            all(np.array_equal(x, y) for x, y in zip(a["words"], b["words"])))


# ------------------------------------------------------------------------------------------ the scenarios
# name -> (scenario of playout_play whose cfg and states it takes, policies, explore per snake or for all, salt, K, max_steps)
TABLE = {
    "XA": ("A", "safe_greedy", 0.25, 7, 60, None),                                   # the main exploring scenario
    "XB": ("B", "wary_greedy", (0.0, 0.25, 1.0), 1, 60, 40),                         # mixed eps, reaches the CAP end
    "XC": ("C", ("safe_greedy", None, "wary_greedy"), 1.0, 2, 40, None),             # pure random movers, reach the DEAD end
    "XD": ("D", ("wary_greedy", "safe_greedy", None), (0.1, 1.0, 0.5), 3, 120, None),  # the compiled-shape handle
    "XF": ("F", ("hamiltonian", "safe_greedy"), (0.5, 0.25), 4, 200, None),          # hamiltonian with eps on 8x8x2
    "X1": ("A", "safe_greedy", 0.25, 7, 1, None),                                    # K = 1
    "XG_long": ("G_long", "safe_greedy", 0.5, 5, 30, None),                          # bodies in the overflow ring
    "XG_finished": ("G_finished", "safe_greedy", 0.5, 6, 5, None),                   # a `finished` env
}
SCENARIOS = tuple(TABLE)
# the quiet states: 19x19x3 a few steps into play; in K steps at eps 0 nobody eats, whichever first move snake 0 is forced to
QUIET = dict(dim=19, n_snakes=3, envs=4, warm=6, K=3, seed=3)


@functools.lru_cache(maxsize=None)
def scenario(name):
    """dict(cfg, states, policies, eps (eps_q16 per snake), explore (the probabilities), salt, K, first, first_snakes)."""
    if name == "X_forced":
        a = scenario("XA")
        first = np.random.default_rng(11).integers(0, 5, (len(a["states"]), 3)).astype(np.int32)
        return dict(a, explore=1.0, eps=[ONE] * 3, K=6, first=first, first_snakes=[0, 2])
    if name == "quiet":
        q = QUIET
        cfg = dict(pp._cfg(q["dim"], q["n_snakes"], q["envs"]), seed=q["seed"])
        return dict(cfg=cfg, states=pp.warm_states(cfg, q["warm"]), policies="safe_greedy", explore=0.5, eps=[ONE // 2] * 3, salt=9,
                    K=q["K"], first=None, first_snakes=None)
    base, pol, explore, salt, K, cap = TABLE[name]
    sc = pp.scenario(base)
    S = sc["cfg"]["n_snakes"]
    cfg = sc["cfg"] if cap is None else dict(sc["cfg"], max_steps=cap)
    per = list(explore) if isinstance(explore, tuple) else [explore] * S
    return dict(cfg=cfg, states=sc["states"], policies=pol, explore=explore, eps=q16(per), salt=salt, K=K, first=sc["first"],
                first_snakes=sc["first_snakes"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(np_playout_explore's result, its trace) of a scenario, computed once per process and shared: treat it as read-only."""
    sc, trace = scenario(name), {}
    return np_playout_explore(sc["cfg"], sc["states"], sc["policies"], sc["eps"], sc["salt"], sc["K"], sc["first"], sc["first_snakes"], trace), trace


@functools.lru_cache(maxsize=None)
def reference_eps0(name):
    """The same scenario with nobody exploring: playout_play.np_playout and its trace."""
    sc, trace = scenario(name), {}
    return pp.np_playout(sc["cfg"], sc["states"], sc["policies"], sc["K"], sc["first"], sc["first_snakes"], trace), trace


def quiet_forks(reps=1):
    """The forks playout_values_device(snake=0, reps=reps) plays on the quiet states: (states, first), slot (e * 4 + m) * reps + r
    holding env e with snake 0's first action forced to m + 1."""
    sc = scenario("quiet")
    E = len(sc["states"])
    states = [sc["states"][e] for e in range(E) for _ in range(4 * reps)]
    first = np.zeros((E * 4 * reps, sc["cfg"]["n_snakes"]), np.int32)
    first[:, 0] = np.tile(np.repeat(np.arange(1, 5), reps), E)
    return states, first
