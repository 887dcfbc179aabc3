"""Every kernel that reads bodies out of HBM, on a ROTATED overflow ring.

The kernels off the step path (state export, render_cells, safe moves, reachable space, copy_envs) all walk a body
the same way, most of them through msnake_envread.inc: piece i >= 64 sits at ovf[(ohp + i - 64) % cap].  A state
installed with set_state starts at ohp = 0, which is all that the cells and copy_envs suites see of bodies over 64
cells.  Here a long body is installed and then DRIVEN: every step of a body over 64 cells evicts one piece into the overflow ring and moves ohp down by
one (mod cap), so k steps after the install ohp = (cap - k) % cap, and the walk wraps around the end of the ring
whenever ohp + len - 64 > cap -- from the first step on, until ohp has come down far enough, and again once ohp has
passed 0.

The CPU oracle is the master: it chooses the Hamiltonian move (scripted_play.hamiltonian), it steps next to the
handle, and every expectation is computed from its state (its exported words, cells_play, scripted_play.np_safe_mask,
space_play.np_space).  Everything is compared bit for bit, for all 8 envs.

Both plays keep grow_to far below the body length: a fruit then raises grow_to and the body keeps its length, where
a body that grew by 2 per fruit would fill the 10 free cells, and end the episode, long before the ring has turned.

snake_env 10x10, 1 snake (cap 128): a 90-cell body along the Hamiltonian cycle, driven for cap + 8 = 136 steps: ohp
passes every value of the ring and the walk wraps a second time.
new_world 10x10, 2 snakes, 1 fruit, max_steps 126 (cap 128 as well): snake 0 is dead with an empty body -- the rule
set ends the episode at every step at which snake 0 is alive --, snake 1 has 70 + 3 e cells in env e.  new_world sizes
the ring from max_steps (cap >= max_steps + 2), so no episode can turn the ring once: the play stops one step short
of the episode's cap, at 125 steps, where ohp has passed 125 of the 128 values; the wrap of the walk is covered from
the first step on.  copy_envs goes into a handle with max_steps 300, whose ring holds 320 cells.
"""
import numpy as np
import pytest

import cells_play as cp
import scripted_play as sp
import space_play as spp
from state_domain import assert_words, blob_words, export as ora_words

pytestmark = pytest.mark.gpu

N, DIM, CAP = 8, 10, 128
CASES = {
    "snake_env": dict(cfg=dict(rules="snake_env", dim=DIM, n_snakes=1, n_fruits=1), max_steps=2000, dst_max_steps=500,
                      lens=lambda e: (90,), steps=CAP + 8),
    "new_world": dict(cfg=dict(rules="new_world", dim=DIM, n_snakes=2, n_fruits=1), max_steps=126, dst_max_steps=300,
                      lens=lambda e: (0, 70 + 3 * e), steps=125),
}


def cycle(dim):
    """The cells of scripted_play.hamiltonian_table(dim) in walking order, from (0, 0)."""
    act, out, c = sp.hamiltonian_table(dim), [], (0, 0)
    for _ in range(dim * dim):
        out.append(c)
        d = sp.DIRS[act[c[0]][c[1]]]
        c = (c[0] + d[0], c[1] + d[1])
    assert c == (0, 0) and len(set(out)) == dim * dim
    return out


def start_state(key, e):
    """Env e's installed state: the body lies along the cycle, its head at cycle cell 11 e + 95, the fruit on a free
    cell; grow_to is 3 whatever the length, and an empty body belongs to a dead snake."""
    case, cyc, n2 = CASES[key], cycle(DIM), DIM * DIM
    lens = case["lens"](e)
    snakes = [[list(cyc[(11 * e + 95 - i) % n2]) for i in range(ln)] for ln in lens]
    vels = [[b[0][0] - b[1][0], b[0][1] - b[1][1]] if b else [0, 0] for b in snakes]
    used = {tuple(c) for b in snakes for c in b}
    free = [c for c in cyc if c not in used]
    rng = np.random.default_rng([5, e, len(lens)])
    fruits = [list(free[i]) for i in rng.choice(len(free), case["cfg"]["n_fruits"], replace=False)]
    return {"t": 0, "ctr": 40 + e, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": fruits, "snakes": snakes,
            "vels": vels, "grow_to": [3] * len(lens), "alive": [bool(b) for b in snakes], "in_dead": [not b for b in snakes]}


def longest_body(st):
    return max(len(b) for b in st["snakes"])


def make_oracle(key):
    from oracle.snake_oracle import Oracle
    case = CASES[key]
    ora = Oracle(N, seed=3, max_steps=case["max_steps"], **case["cfg"])
    ora.reset()
    for e in range(N):
        ora.set_state(e, start_state(key, e))
    return ora


def walk_wraps(k, body_len):
    """k steps after the install: does the walk over pieces 64.. pass the end of the overflow ring?"""
    return (CAP - k) % CAP + body_len - 64 > CAP


def compare_at(key, steps):
    """The steps (0 = straight after the install) at which everything is compared: every 8th, the last, and the step
    at which the walk first wraps."""
    first_wrap = next(k for k in range(1, steps + 1) if all(walk_wraps(k, max(CASES[key]["lens"](e))) for e in range(N)))
    return sorted(set(range(0, steps + 1, 8)) | {steps, first_wrap}), first_wrap


@pytest.mark.parametrize("key", sorted(CASES))
def test_every_reader_on_a_rotated_overflow_ring(key):
    import msnake
    from oracle.snake_oracle import state_to_flat
    case = CASES[key]
    cfg, ns, steps = case["cfg"], case["cfg"]["n_snakes"], case["steps"]
    rules = sp.RULES[cfg["rules"]]
    views = list(range(cp.n_views(rules, ns)))
    assert sp.ring_cap(dict(rules=rules, dim=DIM, max_steps=case["max_steps"])) == CAP
    assert sp.ring_cap(dict(rules=rules, dim=DIM, max_steps=case["dst_max_steps"])) == (CAP if rules != 1 else 320)

    ora = make_oracle(key)
    env = msnake.MultiSnakeVecEnv(N, seed=3, max_steps=case["max_steps"], **cfg)
    dst = msnake.MultiSnakeVecEnv(N, seed=3, max_steps=case["dst_max_steps"], **cfg)
    env.reset()
    dst.reset()
    for e in range(N):
        env.set_state_words(e, state_to_flat(start_state(key, e), ns))
    read = sp._StateReader(ora)
    at, first_wrap = compare_at(key, steps)
    wrapped_at, straight_at, ohp_seen = [], [], set()

    def compare(k):
        states = [read(e) for e in range(N)]
        longest = [longest_body(st) for st in states]
        assert min(longest) > 64, (k, longest)           # a body over 64 cells in every env
        (wrapped_at if all(walk_wraps(k, n) for n in longest) else straight_at).append(k)
        want = [ora_words(ora, e) for e in range(N)]
        assert_words(blob_words(env.get_state_all()), want, (k, "get_state_all"))
        cells, table = env.render_cells_device(snakes=True)
        assert np.array_equal(cells.cpu().numpy(), np.stack([cp.np_cells(st, DIM, ns, rules, views) for st in states])), (k, "cells")
        assert np.array_equal(table.cpu().numpy(), np.stack([cp.np_snake_rows(st, ns) for st in states])), (k, "table")
        assert np.array_equal(env.safe_moves_device().cpu().numpy(), np.stack([sp.np_safe_mask(st, DIM, ns) for st in states])), (k, "safe")
        assert np.array_equal(env.reachable_space_device().cpu().numpy().astype(np.int64),
                              np.stack([spp.np_space(st, DIM, ns) for st in states])), (k, "space")
        dst.copy_envs_device(env)
        assert_words(blob_words(dst.get_state_all()), want, (k, "copy_envs"))
        return states

    states = compare(0)
    for k in range(1, steps + 1):
        act = np.array([sp.hamiltonian(st, DIM, ns) for st in states], np.int32)
        obs, rew, done, _ = env.step(act)
        o_obs, o_rew, o_done = ora.step(act)[:3]
        assert np.array_equal(obs, o_obs) and np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), k
        assert not o_done.any(), k
        if k in at:
            states = compare(k)
        else:
            states = [read(e) for e in range(N)]
            assert min(longest_body(st) for st in states) > 64, k    # every step evicts: ohp = (cap - k) % cap
        ohp_seen.add((CAP - k) % CAP)

    assert first_wrap in wrapped_at and straight_at, (first_wrap, wrapped_at, straight_at)
    if steps >= CAP + 8:   # the overflow position has passed every value, and the walk wraps a second time
        assert ohp_seen == set(range(CAP)) and max(wrapped_at) > max(straight_at) > first_wrap
    assert env.stats()["errors"] == 0 and dst.stats()["errors"] == 0
    env.close()
    dst.close()
