"""Per-snake outcomes of a step, stated on canonical state dicts (Oracle.get_state): include/msnake.h,
msnake_agent_outcomes, restated without the library.

np_outcomes compares the state before a step with the state after it: a fruit eaten raises grow_to by 2, a snake died if
it was alive before and is not after, and each rule set's reward formula for its main snake is applied to every snake.
Twin drives an Oracle(auto_reset=False) under a scripted policy, follows every step with reset_envs(done), and keeps
what the library's tracker has to hold after every call.  Nothing here asks the library under test.

A plain helper module in the style of space_play, which it imports and does not edit; imported by
tests/test_agents_host.py and tests/test_agents_gpu.py.
"""
import numpy as np

import scripted_play as sp
import space_play as spp

ALIVE, WAS_ALIVE, DIED, ENDED = 1, 2, 4, 8   # MSNAKE_AGENT_*
NEW_WORLD = sp.RULES["new_world"]
# the words of a tracker row; words 2..6 are the episode totals
GROW_TO, TR_ALIVE, EP_FRUIT, EP_ALIVE_STEPS, FIRST_DEATH, EP_STEPS, EP_RETURN, TR_ZERO = range(8)
N_TOTALS = 5


def _rules(rules):
    return sp.RULES[rules] if isinstance(rules, str) else int(rules)


def facts(st, rules):
    """(grow_to int64 [S], alive bool [S]) of a canonical state: alive is len > 0 under snake_env and adversarial, the
    alive word under new_world."""
    nw = _rules(rules) == NEW_WORLD
    alive = [bool(a) if nw else len(b) > 0 for a, b in zip(st["alive"], st["snakes"])]
    return np.array(st["grow_to"], np.int64), np.array(alive, bool)


def f32_bits(x):
    return np.asarray(x, np.float32).view(np.int32)


def zero_totals(n_snakes):
    """int32 [S, 5]: ep_fruit, ep_alive_steps, first_death, ep_steps, ep_return (f32 bits), all zero."""
    return np.zeros((n_snakes, N_TOTALS), np.int32)


def track_rows(st, rules, totals):
    """int32 [S, 8]: the tracker rows that describe state `st` with episode totals `totals` (zero_totals: an armed row)."""
    g, alive = facts(st, rules)
    rows = np.zeros((len(g), 8), np.int32)
    rows[:, GROW_TO], rows[:, TR_ALIVE] = g, alive
    rows[:, EP_FRUIT:EP_RETURN + 1] = totals
    return rows


def np_outcomes(prev_state, now_state, done, rules, totals):
    """One env, one step.  prev_state / now_state: the canonical states before and after the step (after: before any
    reset); done: the step's done flag; totals: int32 [S, 5] of the episode so far (not modified).
    Returns (rew float32 [S], ate uint8 [S], flags uint8 [S], info int32 [S, 4], new totals int32 [S, 5], ate unclamped
    int64 [S])."""
    nw = _rules(rules) == NEW_WORLD
    g0, was = facts(prev_state, rules)
    g1, now = facts(now_state, rules)
    ate = np.maximum(0, g1 - g0) >> 1
    died = was & ~now
    ended = was & (died | bool(done))
    rew = np.where(now if nw else died, np.float32(-1.0), ate.astype(np.float32)).astype(np.float32)
    new = np.array(totals, np.int32)
    new[:, 0] += ate.astype(np.int32)
    new[:, 1] += now
    new[:, 3] += 1
    new[:, 2] = np.where(died & (new[:, 2] == 0), new[:, 3], new[:, 2])
    new[:, 4] = f32_bits(new[:, 4].view(np.float32) + rew)
    flags = (now * ALIVE + was * WAS_ALIVE + died * DIED + ended * ENDED).astype(np.uint8)
    info = np.stack([new[:, 0], new[:, 1], new[:, 2], new[:, 4]], axis=1).astype(np.int32)
    return rew, np.minimum(ate, 255).astype(np.uint8), flags, info, new, ate


def scenario(rules, n_snakes, seed, n_fruits=None, max_steps=60, dim=6, policy="safe_greedy", eps=0.1, num_envs=8, steps=400,
             env_id_base=0):
    return sp.scenario(rules, dim, n_snakes, policy, steps, num_envs, seed, n_fruits=n_fruits, eps=eps, max_steps=max_steps,
                       env_id_base=env_id_base)


# The plays of the host and GPU tests.  "S6cap": max_steps 12, so episodes end at the time cap while snakes >= 1 live
# (ENDED without DIED); seeds were chosen on the CPU oracle so that every event class the tests ask for occurs.
SCENARIOS = {
    "S6": scenario("snake_env", 3, 1),
    "A6": scenario("adversarial", 3, 1),
    "N6": scenario("new_world", 4, 1, n_fruits=9),
    "S6cap": scenario("snake_env", 3, 1, max_steps=12),
}


class Twin:
    """An Oracle(auto_reset=False) under cfg's scripted policy: step() steps it with the given (or the policy's) actions,
    forms every env's outcomes from the states before and after, and resets the done envs with reset_envs(done).  After a
    step: rew / ate / flags / info as msnake_agent_outcomes has to write them ([E, S] and [E, S, 4]), `track` ([E, S, 8])
    as the tracker has to read behind that call, and step_rew / done / obs as the oracle's step returned them (obs: after
    the masked reset, i.e. what an auto_reset=True env shows)."""

    def __init__(self, cfg):
        self.cfg, self.E, self.S = cfg, cfg["num_envs"], cfg["n_snakes"]
        self.ora = sp.make_oracle(cfg, auto_reset=False)
        self.read = sp._StateReader(self.ora)
        self.rs = sp.policy_rng(cfg)
        self.obs = self.ora.reset().copy()
        self.states = [self.read(e) for e in range(self.E)]
        self.totals = [zero_totals(self.S) for _ in range(self.E)]

    @property
    def track(self):
        return np.stack([track_rows(st, self.cfg["rules"], tot) for st, tot in zip(self.states, self.totals)])

    def actions(self):
        return spp.choose_actions(self.cfg, self.states, self.rs)

    def step(self, act=None):
        act = self.actions() if act is None else np.ascontiguousarray(act, np.int32)
        prev = self.states
        obs, rew, done, num_snakes, ep_return, ep_len = self.ora.step(act)
        self.step_rew, self.done = rew.copy(), done.copy()
        self.num_snakes, self.ep_return, self.ep_len = num_snakes.copy(), ep_return.copy(), ep_len.copy()
        self.prev, self.now = prev, [self.read(e) for e in range(self.E)]
        out = [np_outcomes(prev[e], self.now[e], done[e], self.cfg["rules"], self.totals[e]) for e in range(self.E)]
        self.rew, self.ate, self.flags, self.info = (np.stack([o[k] for o in out]) for k in range(4))
        self.ate_raw = np.stack([o[5] for o in out])
        self.states = list(self.now)
        self.totals = [o[4] for o in out]
        if done.any():
            obs, _, _ = self.ora.reset_envs(done, final_obs=None, truncated=None)
            for e in np.nonzero(done)[0]:
                self.states[e], self.totals[e] = self.read(e), zero_totals(self.S)
        self.obs = obs.copy()
        return act
