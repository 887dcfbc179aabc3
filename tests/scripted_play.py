"""Scripted long-lived play: deterministic policies that keep snakes alive for hundreds of steps, a recorder that
runs them on the CPU oracle alone, and the coverage numbers of such a recording.

Random play dies within a few dozen steps, so it never reaches what a trained agent does all day: full boards, bodies
that grow through the 64-cell register ring into the overflow ring, the 2000-step cap, fruit lists of dozens of
entries.  The policies here reach all of that (see SCENARIOS).  They read only canonical state dicts
(Oracle.get_state / tools/gen_golden.py canon_state), so the same functions steer the reference when
tools/gen_golden.py records tests/golden/long_play.npz and the oracle when the GPU tests record their action tapes.

A plain helper module (like golden_util), imported by tests/test_oracle_long_play.py, tests/test_long_play_gpu.py and
tools/gen_golden.py.
"""
import zlib

import numpy as np

DIRS = {1: (1, 0), 2: (0, 1), 3: (-1, 0), 4: (0, -1)}
RULES = {"snake_env": 0, "new_world": 1, "adversarial": 2}


# ----------------------------------------------------------------------------------------------- policies
_HAM = {}


def hamiltonian_table(dim):
    """act[x][y] = the action that leads from cell (x, y) to its successor on a Hamiltonian cycle of an even board:
    column 0 is the return lane, the rows snake back and forth over columns 1..dim-1."""
    if dim not in _HAM:
        assert dim % 2 == 0 and dim >= 2, "the cycle needs an even board"
        act = [[0] * dim for _ in range(dim)]
        for y in range(dim):
            for x in range(dim):
                if x == 0:
                    a = 4 if y > 0 else 1                       # up the return lane, then into row 0
                elif y % 2 == 0:
                    a = 1 if x < dim - 1 else 2                 # even rows run right, then one row down
                elif y == dim - 1:
                    a = 3                                       # the last row runs left into the return lane
                else:
                    a = 3 if x > 1 else 2                       # odd rows run left to column 1, then one row down
                act[x][y] = a
        _HAM[dim] = act
    return _HAM[dim]


def hamiltonian(st, dim, n_snakes, rs=None, eps=0.0):
    """Every snake follows the cycle from wherever its head is (a reversal is ignored by the env; some first episodes
    die early because of it, which is part of what is compared)."""
    act = hamiltonian_table(dim)
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            out.append(0)
            continue
        x, y = body[0]
        out.append(act[x][y] if 0 <= x < dim and 0 <= y < dim else 0)
    return out


def safe_greedy(st, dim, n_snakes, rs, eps=0.0):
    """Among the four moves whose target cell is on the board and free of every body, the one that brings the head
    closest (L1) to a fruit; 0 when there is none.  With probability eps a random action 0..4 instead."""
    used = set()
    for b in st["snakes"]:
        for c in b:
            used.add((c[0], c[1]))
    fruits = st["fruits"]
    out = []
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if eps and rs.random() < eps:
            out.append(int(rs.integers(0, 5)))
            continue
        if not body:
            out.append(0)
            continue
        hx, hy = body[0]
        best, best_d = 0, None
        for a in (1, 2, 3, 4):
            x, y = hx + DIRS[a][0], hy + DIRS[a][1]
            if not (0 <= x < dim and 0 <= y < dim) or (x, y) in used:
                continue
            d = min((abs(f[0] - x) + abs(f[1] - y) for f in fruits), default=0)
            if best_d is None or d < best_d:
                best, best_d = a, d
        out.append(best)
    return out


POLICIES = {"hamiltonian": hamiltonian, "safe_greedy": safe_greedy}


def np_safe_mask(st, dim, n_snakes):
    """Bit a (1..4) of entry s: the target of move a of snake s lies on the board and in no body; 0 for an empty body."""
    occ = np.zeros((dim, dim), bool)
    for body in st["snakes"]:
        for c0, c1 in body:
            if 0 <= c0 < dim and 0 <= c1 < dim:
                occ[c0, c1] = True
    out = np.zeros(n_snakes, np.uint8)
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            continue
        for a, (d0, d1) in DIRS.items():
            x, y = body[0][0] + d0, body[0][1] + d1
            if 0 <= x < dim and 0 <= y < dim and not occ[x, y]:
                out[s] |= 1 << a
    return out


# ----------------------------------------------------------------------------------------------- scenarios
def scenario(rules, dim, n_snakes, policy, steps, num_envs, seed, n_fruits=None, eps=0.0, max_steps=2000,
             env_id_base=0, expect=()):
    """`expect`: which coverage conditions the scenario is there for (check_coverage):
    "full" the board fills (and stays nearly full for 20 env-steps; "filled": fills once), "over64" a body passes
    64 cells, "capped" episodes end at the 2000-step cap, "overflow" a body stays over 64 cells for two
    turns of the overflow ring, "fruits40" / "fruits65" the adversarial fruit list reaches 40 / 65 entries."""
    return dict(rules=RULES[rules] if isinstance(rules, str) else int(rules), dim=dim, n_snakes=n_snakes,
                n_fruits=n_snakes if n_fruits is None else n_fruits, policy=policy, steps=steps, num_envs=num_envs,
                seed=seed, eps=eps, max_steps=max_steps, env_id_base=env_id_base, expect=list(expect))


def ring_cap(cfg):
    """Cells of the kernel's overflow ring (msnake_capi.hip: dim^2 + 2, new_world max_steps + 2, in whole 64s)."""
    need = cfg["dim"] ** 2 + 2
    if cfg["rules"] == 1:
        need = max(need, cfg["max_steps"] + 2)
    return (need + 63) // 64 * 64


def policy_rng(cfg):
    """One generator per env, keyed by its global env id: an env plays the same game whatever batch it is part of."""
    return [np.random.default_rng([cfg["seed"], cfg["dim"], cfg["n_snakes"], cfg["rules"], cfg["env_id_base"] + e])
            for e in range(cfg["num_envs"])]


def choose_actions(cfg, states, rs):
    """One action row per env from the canonical states (the only consumer of the generators `rs`)."""
    pol = POLICIES[cfg["policy"]]
    return np.array([pol(st, cfg["dim"], cfg["n_snakes"], r, cfg["eps"]) for st, r in zip(states, rs)], np.int32)


# ----------------------------------------------------------------------------------------------- coverage
def longest_run(flags):
    """Longest run of consecutive non-zero entries along axis 0, per column, of a [T, E] array."""
    run = np.zeros(flags.shape[1], np.int64)
    best = np.zeros(flags.shape[1], np.int64)
    for row in np.asarray(flags, bool):
        run = np.where(row, run + 1, 0)
        best = np.maximum(best, run)
    return best


def coverage(cfg, body_max, n_fruits, done, ep_len, ctr=None):
    """Coverage numbers of a play from per-step, per-env arrays [T, E]: the longest body and the fruit count after
    each step, done and the reported episode length (0 where not done), and optionally the draw counter."""
    n2 = cfg["dim"] ** 2
    body_max = np.asarray(body_max, np.int64)
    done = np.asarray(done) != 0
    lens = np.asarray(ep_len)[done]
    cov = dict(longest_body=int(body_max.max()),
               full_env_steps=int((body_max == n2).sum()),
               nearly_full_env_steps=int((body_max >= n2 - 1).sum()),
               episodes=int(done.sum()),
               longest_episode=int(lens.max()) if lens.size else 0,
               capped_episodes=int((lens == cfg["max_steps"]).sum()),
               longest_fruit_list=int(np.asarray(n_fruits).max()),
               env_steps_over_64=int((body_max > 64).sum()),
               longest_run_over_64=int(longest_run(body_max > 64).max()))
    if ctr is not None:
        cov["largest_draw_counter"] = int(np.asarray(ctr).max())
    return cov


def check_coverage(cfg, cov):
    """The conditions a scenario is there for, from numbers that the code under test had no part in."""
    n2, ex = cfg["dim"] ** 2, cfg["expect"]
    if "full" in ex:
        assert cov["longest_body"] == n2 and cov["full_env_steps"] >= 1 and cov["nearly_full_env_steps"] >= 20, cov
    if "filled" in ex:
        assert cov["longest_body"] == n2 and cov["full_env_steps"] >= 1, cov
    if "capped" in ex:
        assert cfg["max_steps"] == 2000 and cov["capped_episodes"] >= 4, cov
    if "over64" in ex:
        assert cov["longest_body"] > 64 and cov["env_steps_over_64"] > 0, cov
    if "overflow" in ex:
        assert cov["longest_run_over_64"] >= 2 * ring_cap(cfg), (cov, ring_cap(cfg))
    if "fruits40" in ex:
        assert cov["longest_fruit_list"] >= 40, cov
    if "fruits65" in ex:
        assert cov["longest_fruit_list"] >= 65, cov


# ----------------------------------------------------------------------------------------------- recorder
def crc_rows(obs):
    return np.array([zlib.crc32(np.ascontiguousarray(o).tobytes()) for o in obs], np.uint32)


def make_oracle(cfg, auto_reset=True, max_steps=None):
    from oracle.snake_oracle import Oracle
    return Oracle(cfg["num_envs"], dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"],
                  rules=cfg["rules"], seed=cfg["seed"], env_id_base=cfg["env_id_base"],
                  max_steps=cfg["max_steps"] if max_steps is None else max_steps, auto_reset=auto_reset)


class _StateReader:
    """Oracle.get_state without the per-call buffer allocation and per-word int() (the recorder's hot spot)."""

    def __init__(self, ora):
        self.ora = ora
        self.buf = np.zeros(64, np.int32)

    def __call__(self, e):
        from oracle.snake_oracle import flat_to_state
        L, h = self.ora.L, self.ora.h
        n = L.orc_export_state(h, e, self.buf.ctypes.data, len(self.buf))
        if n > len(self.buf):
            self.buf = np.zeros(2 * n, np.int32)
            n = L.orc_export_state(h, e, self.buf.ctypes.data, len(self.buf))
        return flat_to_state(self.buf[:n].tolist())


def record(cfg, policy=None, steps=None, seed=None, auto_reset=True, state_every=64, full_obs_at=()):
    """Run the oracle alone under cfg's scripted policy (policy / steps / seed override cfg's).  Returns a dict:
      actions int32 [T, E, n_snakes]; reward, done, num_snakes, ep_return, ep_len [T, E] as the oracle returned them;
      obs_crc uint32 [T, E] (CRC32 of each env's observation) and obs0_crc [E]; full_obs {t: frames} at full_obs_at;
      states {t: [canonical state per env]} for every t % state_every == 0, the last step and every step at which an
      env is done (state after the step; with auto_reset=False after the step and before the masked reset);
      body_max, n_fruits int16 and ctr int64 [T, E] (state after the step, before any masked reset);
      coverage: see coverage().
    auto_reset=False: the oracle runs without auto reset and every step with a done env is followed by
    reset_envs(done); then also final_crc uint32 [T, E] (CRC32 of the terminal observation row, 0 where not done)
    and truncated uint8 [T, E] (the flags of every env at the steps where some env was done, else 0)."""
    cfg = dict(cfg)
    if policy is not None:
        cfg["policy"] = policy
    if steps is not None:
        cfg["steps"] = steps
    if seed is not None:
        cfg["seed"] = seed
    T, E, ns = cfg["steps"], cfg["num_envs"], cfg["n_snakes"]
    ora = make_oracle(cfg, auto_reset)
    read = _StateReader(ora)
    rs = policy_rng(cfg)
    rec = dict(cfg=cfg, auto_reset=bool(auto_reset), actions=np.zeros((T, E, ns), np.int32),
               reward=np.zeros((T, E), np.float32), done=np.zeros((T, E), np.uint8),
               num_snakes=np.zeros((T, E), np.int32), ep_return=np.zeros((T, E), np.float32),
               ep_len=np.zeros((T, E), np.int32), obs_crc=np.zeros((T, E), np.uint32), full_obs={}, states={},
               body_max=np.zeros((T, E), np.int16), n_fruits=np.zeros((T, E), np.int16), ctr=np.zeros((T, E), np.int64))
    if not auto_reset:
        rec["final_crc"] = np.zeros((T, E), np.uint32)
        rec["truncated"] = np.zeros((T, E), np.uint8)
    rec["obs0_crc"] = crc_rows(ora.reset())
    states = [read(e) for e in range(E)]
    full_obs_at = set(full_obs_at)
    for t in range(T):
        act = choose_actions(cfg, states, rs)
        rec["actions"][t] = act
        obs, rew, done, nsn, epr, epl = ora.step(act)
        for k, v in (("reward", rew), ("done", done), ("num_snakes", nsn), ("ep_return", epr), ("ep_len", epl)):
            rec[k][t] = v
        states = [read(e) for e in range(E)]
        rec["body_max"][t] = [max(len(b) for b in st["snakes"]) for st in states]
        rec["n_fruits"][t] = [len(st["fruits"]) for st in states]
        rec["ctr"][t] = [st["ctr"] for st in states]
        if t % state_every == 0 or t == T - 1 or done.any():
            rec["states"][t] = states
        if not auto_reset and done.any():
            obs, final, trunc = ora.reset_envs(done)
            rec["truncated"][t] = trunc
            for e in np.nonzero(done)[0]:
                rec["final_crc"][t, e] = zlib.crc32(final[e].tobytes())
                states[e] = read(e)
        rec["obs_crc"][t] = crc_rows(obs)
        if t in full_obs_at:
            rec["full_obs"][t] = obs.copy()
    rec["coverage"] = coverage(cfg, rec["body_max"], rec["n_fruits"], rec["done"], rec["ep_len"], rec["ctr"])
    return rec


_CACHE = {}


def recorded(name, auto_reset=True):
    """record() of SCENARIOS[name], computed once per process."""
    key = (name, bool(auto_reset))
    if key not in _CACHE:
        _CACHE[key] = record(SCENARIOS[name], auto_reset=auto_reset)
    return _CACHE[key]


# The plays of the GPU tests (tests/test_long_play_gpu.py).  The fixture tests/golden/long_play.npz holds the same
# kinds of play from the reference at a handful of envs each (tools/gen_golden.py LONG_PLAY).
SCENARIOS = {}


def _add(table, name, *a, **k):
    table[name] = scenario(*a, **k)


# name -> scenario.  14x14: global env 59 of seed 3 is one of the few whose body passes 64 cells before the cap
# (3 of envs 0..127 do); adversarial x3: global env 54 of seed 7 takes the fruit list past 64 entries (67).  Both were
# found on the CPU oracle; an env plays the same game in any batch that holds its global id.
_add(SCENARIOS, "S6", "snake_env", 6, 1, "hamiltonian", 1300, 32, 1, expect=["full"])
_add(SCENARIOS, "S10", "snake_env", 10, 1, "hamiltonian", 4100, 16, 2, expect=["full", "over64", "overflow"])
_add(SCENARIOS, "S12", "snake_env", 12, 1, "hamiltonian", 2100, 8, 3, expect=["capped", "over64", "overflow"])
_add(SCENARIOS, "S14", "snake_env", 14, 1, "hamiltonian", 2100, 8, 3, env_id_base=56, expect=["capped", "over64"])
_add(SCENARIOS, "S20", "snake_env", 20, 1, "hamiltonian", 2100, 8, 10, expect=["capped"])
_add(SCENARIOS, "S6x2", "snake_env", 6, 2, "hamiltonian", 1300, 24, 4, expect=["full"])
_add(SCENARIOS, "A6", "adversarial", 6, 1, "hamiltonian", 1300, 24, 5, expect=["full"])
_add(SCENARIOS, "A10", "adversarial", 10, 1, "hamiltonian", 4100, 12, 6, expect=["full", "capped", "over64"])
_add(SCENARIOS, "A10x3", "adversarial", 10, 3, "safe_greedy", 2500, 16, 7, eps=0.02, env_id_base=48,
     expect=["fruits40", "fruits65", "over64"])
_add(SCENARIOS, "S19x3", "snake_env", 19, 3, "safe_greedy", 2500, 16, 9, eps=0.01, expect=["over64"])
_add(SCENARIOS, "N10x2", "new_world", 10, 2, "safe_greedy", 2600, 16, 8, n_fruits=4, expect=["capped", "over64"])
_add(SCENARIOS, "N10x4", "new_world", 10, 4, "safe_greedy", 2100, 8, 8, expect=["capped", "over64"])

# The runs of tests/golden/long_play.npz: the same kinds of play on the reference (slow pure Python: a few envs each).
FIXTURE_RUNS = {}
_add(FIXTURE_RUNS, "S6", "snake_env", 6, 1, "hamiltonian", 1500, 4, 1, expect=["full"])
_add(FIXTURE_RUNS, "S10", "snake_env", 10, 1, "hamiltonian", 4100, 4, 2, expect=["full", "over64"])
_add(FIXTURE_RUNS, "S14", "snake_env", 14, 1, "hamiltonian", 2100, 4, 3, env_id_base=58, expect=["capped", "over64"])
_add(FIXTURE_RUNS, "S6x2", "snake_env", 6, 2, "hamiltonian", 1500, 4, 4, expect=["full"])
_add(FIXTURE_RUNS, "A6", "adversarial", 6, 1, "hamiltonian", 1500, 4, 5, expect=["full"])
_add(FIXTURE_RUNS, "A10", "adversarial", 10, 1, "hamiltonian", 2100, 2, 6, expect=["filled", "over64"])
_add(FIXTURE_RUNS, "A10x3", "adversarial", 10, 3, "safe_greedy", 2500, 4, 7, eps=0.02, env_id_base=52,
     expect=["fruits40", "fruits65", "over64"])
_add(FIXTURE_RUNS, "N10x2", "new_world", 10, 2, "safe_greedy", 2600, 4, 8, n_fruits=4, expect=["capped", "over64"])
