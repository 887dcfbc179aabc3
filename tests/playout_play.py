"""Scripted playouts, stated on the CPU oracle: include/msnake.h, msnake_playout, restated without the library.

np_playout plays a batch of canonical states on for up to n_steps steps on an oracle without auto reset, the actions
coming from the Python policies the other helpers already hold (scripted_play.safe_greedy / hamiltonian,
fates_play.wary_greedy), snapshots every env at the step it ends while the oracle goes on stepping the others, and
keeps the per-snake sums the header defines.  The end words are state_to_flat of the snapshot plus the `finished` bit.
scenarios() holds the plays the tests compare the library with; coverage() says what they reach, from the reference's
own outputs.  Nothing here asks the library under test.

A plain helper module in the style of fates_play, which it imports and does not edit; imported by
tests/test_playout_host.py and tests/test_playout_gpu.py.
"""
import functools
import json
import os

import numpy as np

import fates_play as fp
import scripted_play as sp

HORIZON, DEAD, CAP, FINISHED = 0, 1, 2, 3   # MSNAKE_PLAYOUT_*
MAX_STEPS = 4096                            # MSNAKE_PLAYOUT_MAX_STEPS
POLICY_ID = {None: 0, "safe_greedy": 1, "hamiltonian": 2, "wary_greedy": 3}
POLICIES = {None: lambda st, dim, ns, rs=None, eps=0.0: [0] * ns, "safe_greedy": sp.safe_greedy,
            "hamiltonian": sp.hamiltonian, "wary_greedy": fp.wary_greedy}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def per_snake(policies, n_snakes):
    """One name for all snakes or one per snake -> a list of n_snakes names."""
    if policies is None or isinstance(policies, str):
        return [policies] * n_snakes
    assert len(policies) == n_snakes
    return list(policies)


def policy_actions(st, dim, n_snakes, policies):
    """The action row of one env: policies[s] applied to the state, for every snake."""
    rows = {name: POLICIES[name](st, dim, n_snakes, None, 0.0) for name in set(policies)}
    return [int(rows[policies[s]][s]) for s in range(n_snakes)]


def np_playout(cfg, states, policies, n_steps, first=None, first_snakes=None, trace=None):
    """cfg: a scripted_play.scenario (dim, n_snakes, seed, env_id_base, max_steps; num_envs is taken from `states`);
    states: canonical dicts, one per env, env e being global env env_id_base + e (a dict may carry "finished": True);
    first: int [E, >= n_snakes] action words forced in step 1 for the snakes in first_snakes (default: every snake).
    Returns dict(steps int32 [E], end uint8 [E], ret float32 [E, S], info int32 [E, S, 4], words: list of int32 arrays,
    count int32 [E]).  `trace`, a dict, receives rew [K, E] (the oracle's step rewards, 0 behind an env's end), ate and
    died [K, E, S], and draws [E] (Philox draws consumed)."""
    from oracle.snake_oracle import state_to_flat
    E, S, dim = len(states), cfg["n_snakes"], cfg["dim"]
    policies = per_snake(policies, S)
    forced = set(range(S)) if first_snakes is None else {int(s) for s in first_snakes}
    ora = sp.make_oracle(dict(cfg, num_envs=E), auto_reset=False)
    ora.reset()
    for e, st in enumerate(states):
        ora.set_state(e, st)
    read = sp._StateReader(ora)
    out = dict(steps=np.zeros(E, np.int32), end=np.zeros(E, np.uint8), ret=np.zeros((E, S), np.float32),
               info=np.zeros((E, S, 4), np.int32), words=[None] * E, count=np.zeros(E, np.int32))
    if trace is not None:
        trace.update(rew=np.zeros((n_steps, E), np.float32), ate=np.zeros((n_steps, E, S), np.int32),
                     died=np.zeros((n_steps, E, S), bool), draws=np.zeros(E, np.int64))
    cur = [read(e) for e in range(E)]
    active = []
    for e, st in enumerate(states):
        if st.get("finished"):
            out["end"][e] = FINISHED
            out["words"][e] = state_to_flat(dict(cur[e], finished=True), S)
        else:
            active.append(e)
    for k in range(1, n_steps + 1):
        if not active:
            break
        act = np.zeros((E, S), np.int32)
        for e in active:
            act[e] = policy_actions(cur[e], dim, S, policies)
            if k == 1 and first is not None:
                for s in forced:
                    act[e, s] = int(first[e][s])
            if k == 1:
                out["info"][e, :, 3] = act[e]
        _, rew, done, *_ = ora.step(act, want_obs=False)
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
                if trace is not None:
                    trace["ate"][k - 1, e, s], trace["died"][k - 1, e, s] = ate, died
            if trace is not None:
                trace["rew"][k - 1, e] = rew[e]
            out["steps"][e] = k
            if done[e]:
                out["end"][e] = DEAD if not after["snakes"][0] else CAP
                out["words"][e] = state_to_flat(dict(after, finished=True), S)
            else:
                still.append(e)
        active = still
    for e in active:
        out["end"][e] = HORIZON
        out["words"][e] = state_to_flat(cur[e], S)
    for e in range(E):
        out["count"][e] = len(out["words"][e])
        if trace is not None:
            w = out["words"][e]
            trace["draws"][e] = ((int(w[1]) & 0xFFFFFFFF) | ((int(w[2]) & 0xFFFFFFFF) << 32)) - int(states[e].get("ctr", 0))
    return out


def words_to_state(words):
    """The canonical dict of a row of end words, the `finished` bit included: what a continued playout starts from."""
    from oracle.snake_oracle import flat_finished, flat_to_state
    st = flat_to_state(words)
    if flat_finished(words):
        st["finished"] = True
    return st


# ------------------------------------------------------------------------------------------ the scenarios
def warm_states(cfg, warm):
    """The states `warm` steps into safe_greedy play from a reset, on an oracle with auto reset."""
    ora = sp.make_oracle(cfg, auto_reset=True)
    ora.reset()
    read = sp._StateReader(ora)
    states = [read(e) for e in range(cfg["num_envs"])]
    for _ in range(warm):
        act = np.array([sp.safe_greedy(st, cfg["dim"], cfg["n_snakes"], None) for st in states], np.int32)
        ora.step(act, want_obs=False)
        states = [read(e) for e in range(cfg["num_envs"])]
    return states


def _cfg(dim, n_snakes, num_envs, max_steps=2000):
    return sp.scenario("snake_env", dim, n_snakes, "safe_greedy", 0, num_envs, 3, max_steps=max_steps, env_id_base=5)


# name -> (dim, n_snakes, envs, warm, K, policies, max_steps)
TABLE = {
    "A": (10, 3, 67, 25, 60, "safe_greedy", 2000),
    "B": (10, 3, 67, 25, 60, "wary_greedy", 40),
    "C": (6, 3, 67, 10, 40, "safe_greedy", 2000),
    "D": (19, 3, 33, 40, 120, ("wary_greedy", "safe_greedy", None), 2000),
    "E": (10, 1, 33, 30, 300, "safe_greedy", 2000),
    "F": (8, 2, 16, 0, 200, ("hamiltonian", "safe_greedy"), 2000),
}


@functools.lru_cache(maxsize=None)
def scenario(name):
    """dict(cfg, states, policies, K, first, first_snakes) of one scenario; the states are computed once per process."""
    if name in TABLE:
        dim, ns, envs, warm, K, pol, cap = TABLE[name]
        cfg = _cfg(dim, ns, envs, cap)
        return dict(cfg=cfg, states=warm_states(cfg, warm), policies=pol, K=K, first=None, first_snakes=None)
    if name == "H1":
        a = scenario("A")
        return dict(a, K=1)
    if name == "Hmax":
        a = scenario("A")
        return dict(a, cfg=dict(a["cfg"], num_envs=8), states=a["states"][:8], K=MAX_STEPS)
    if name == "G_long":
        cfg = dict(_cfg(10, 3, 2), seed=1, env_id_base=0)
        return dict(cfg=cfg, states=[fp.long_body_state(False), fp.long_body_state(True)], policies="safe_greedy", K=30,
                    first=None, first_snakes=None)
    if name == "G_finished":
        a = scenario("A")
        states = [dict(a["states"][0], finished=True), a["states"][1], dict(a["states"][2], finished=True)]
        return dict(a, cfg=dict(a["cfg"], num_envs=3), states=states, K=5)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(np_playout's result, its trace) of a scenario, computed once per process and shared: treat it as read-only."""
    sc, trace = scenario(name), {}
    return np_playout(sc["cfg"], sc["states"], sc["policies"], sc["K"], sc["first"], sc["first_snakes"], trace), trace


SCENARIOS = tuple(TABLE) + ("H1", "Hmax", "G_long", "G_finished")


def edge_cases():
    """Every snake_env step of tests/golden/edge_cases.json as a one-env playout of K = 1 with all actions forced:
    [(label, cfg, start state, actions, expected state)]."""
    with open(os.path.join(GOLDEN, "edge_cases.json")) as f:
        entries = json.load(f)
    out = []
    for en in entries:
        if not en["name"].startswith("S_"):
            continue
        cfg = sp.scenario("snake_env", en["dim"], en["n_snakes"], "safe_greedy", 0, 1, en["seed"], n_fruits=en["n_fruits"],
                          env_id_base=en["env_id"])
        st = en["state0"]
        for i, step in enumerate(en["steps"]):
            if "done" not in step:   # (S_reset_draw_order records resets, not steps)
                break
            out.append((f"{en['name']}[{i}]", cfg, st, list(step["actions"]), step["state"]))
            if step["done"]:
                break
            st = step["state"]
    return out


def coverage(names=("A", "B", "C")):
    """What the scenarios reach, from the reference's outputs alone."""
    ends = {HORIZON: 0, DEAD: 0, CAP: 0}
    other_deaths = two_eaters = 0
    for n in names:
        res, tr = reference(n)
        for c in ends:
            ends[c] += int((res["end"] == c).sum())
        K = tr["rew"].shape[0]
        played = np.arange(1, K + 1)[:, None] <= res["steps"][None, :]           # [K, E]
        last = np.arange(1, K + 1)[:, None] == res["steps"][None, :]
        went_on = played & ~(last & (res["end"] != HORIZON)[None, :])
        other_deaths += int((tr["died"][:, :, 1:].any(axis=2) & went_on).sum())
        two_eaters += int((((tr["ate"] > 0).sum(axis=2) >= 2) & played).sum())
    return dict(ends=ends, other_deaths=other_deaths, two_eaters=two_eaters)
