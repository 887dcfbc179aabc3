"""Per-snake outcomes, host side: tests/agents_play.py against the oracle's own step outputs, selfplay.agent_targets
against a NumPy loop over segments, and the refusals of Runner(all_snakes=True).  Nothing here needs a GPU.

The formulas of include/msnake.h (msnake_agent_outcomes) are checked on the CPU oracle alone first: column 0 of the
per-snake reward is the step's own reward on every env-step of all three rule sets, the grow_to difference is even and
non-negative, and a reset env reads grow_to 3, alive, length 1 -- what the library writes into a done env's tracker rows
without looking.  Every scenario has to reach each class of event the GPU tests rely on.
"""
import functools

import numpy as np
import pytest

import agents_play as ap

MIN_EVENTS = 20


@functools.lru_cache(maxsize=None)
def _played(name):
    """One play of SCENARIOS[name] on the oracle alone: the event counts and every violated invariant."""
    cfg = ap.SCENARIOS[name]
    tw = ap.Twin(cfg)
    ev = dict(fruit_other=0, die_not_done=0, eat_and_die=0, ate_gt1=0, cap_alive=0, env_steps=0)
    bad = []
    for st in tw.states:   # the reset that starts the play
        g, alive = ap.facts(st, cfg["rules"])
        if not ((g == 3).all() and alive.all() and all(len(b) == 1 for b in st["snakes"])):
            bad.append(("reset", st))
    for t in range(cfg["steps"]):
        assert not any(tw.ora.finished(e) for e in range(tw.E)), "every step is taken from an unfinished episode"
        tw.step()
        ev["env_steps"] += tw.E
        if not np.array_equal(tw.rew[:, 0].view(np.int32), tw.step_rew.view(np.int32)):
            bad.append(("column 0", t, tw.rew[:, 0].tolist(), tw.step_rew.tolist()))
        for e in range(tw.E):
            diff = np.array(tw.now[e]["grow_to"]) - np.array(tw.prev[e]["grow_to"])
            if (diff < 0).any() or (diff & 1).any():
                bad.append(("grow_to", t, e, diff.tolist()))
            if tw.done[e]:   # tw.states[e] is the state after reset_envs(done)
                g, alive = ap.facts(tw.states[e], cfg["rules"])
                if not ((g == 3).all() and alive.all() and all(len(b) == 1 for b in tw.states[e]["snakes"])):
                    bad.append(("reset", t, e))
        died, ended = (tw.flags & ap.DIED) != 0, (tw.flags & ap.ENDED) != 0
        not_done = tw.done[:, None] == 0
        capped = np.array([tw.done[e] != 0 and tw.now[e]["t"] >= cfg["max_steps"] for e in range(tw.E)])[:, None]
        ev["fruit_other"] += int((tw.ate_raw[:, 1:] > 0).sum())
        ev["die_not_done"] += int((died[:, 1:] & not_done).sum())
        ev["eat_and_die"] += int((died & (tw.ate_raw > 0)).sum())
        ev["ate_gt1"] += int((tw.ate_raw > 1).sum())
        ev["cap_alive"] += int((ended[:, 1:] & ~died[:, 1:] & capped).sum())
    return ev, bad


@pytest.mark.parametrize("name", ["S6", "A6", "N6"])
def test_formulas_hold_on_the_oracle_and_every_event_class_occurs(name):
    ev, bad = _played(name)
    assert not bad, bad[:3]
    assert ev["env_steps"] == 8 * 400
    for k in ("fruit_other", "die_not_done", "eat_and_die", "ate_gt1"):
        assert ev[k] >= MIN_EVENTS, (name, ev)


def test_time_cap_ends_snakes_that_did_not_die():
    """max_steps 12: episodes reach the cap while a snake >= 1 lives: ENDED without DIED."""
    ev, bad = _played("S6cap")
    assert not bad, bad[:3]
    assert ev["cap_alive"] >= MIN_EVENTS, ev


def test_np_outcomes_by_hand():
    """Snake 0 eats two fruits and dies, snake 1 was dead, snake 2 lives on; new_world turns the sign of `alive`."""
    st = lambda grow, bodies, alive: {"grow_to": grow, "snakes": bodies, "alive": alive}
    prev = st([3, 5, 3], [[[0, 0]], [], [[2, 2]]], [True, True, True])
    now = st([7, 5, 3], [[], [], [[2, 3]]], [True, False, False])
    tot = ap.zero_totals(3)
    tot[:, 3] = 4
    rew, ate, flags, info, new, raw = ap.np_outcomes(prev, now, 1, "snake_env", tot)
    assert rew.tolist() == [-1.0, 0.0, 0.0] and ate.tolist() == [2, 0, 0] and raw.tolist() == [2, 0, 0]
    assert flags.tolist() == [ap.WAS_ALIVE | ap.DIED | ap.ENDED, 0, ap.ALIVE | ap.WAS_ALIVE | ap.ENDED]
    assert info[:, :3].tolist() == [[2, 0, 5], [0, 0, 0], [0, 1, 0]]
    assert info[:, 3].view(np.float32).tolist() == [-1.0, 0.0, 0.0] and new[:, 3].tolist() == [5, 5, 5]
    rew, ate, flags, info, new, raw = ap.np_outcomes(prev, now, 0, "new_world", tot)
    assert rew.tolist() == [-1.0, 0.0, 0.0] and flags.tolist() == [ap.ALIVE | ap.WAS_ALIVE, ap.WAS_ALIVE | ap.DIED | ap.ENDED,
                                                                   ap.WAS_ALIVE | ap.DIED | ap.ENDED]
    big = st([3 + 2 * 300], [[[0, 0]]], [True])
    rew, ate, _, info, _, raw = ap.np_outcomes(st([3], [[[0, 1]]], [True]), big, 0, "adversarial", ap.zero_totals(1))
    assert rew.tolist() == [300.0] and ate.tolist() == [255] and raw.tolist() == [300] and info[0, 0] == 300


# ------------------------------------------------------------------------------------------ agent_targets
def _np_gae_run(rew, val, ended, last_val, last_ended, gamma, lam):
    """The gae loop of selfplay.gae on ONE run of valid samples of one agent (float32, NumPy)."""
    T = len(rew)
    adv = np.zeros(T, np.float32)
    last = np.float32(0.0)
    for t in reversed(range(T)):
        if t == T - 1:
            nnt, nv = np.float32(1.0 - last_ended), last_val
        else:
            nnt, nv = np.float32(1.0 - ended[t]), val[t + 1]
        delta = rew[t] + np.float32(gamma) * nv * nnt - val[t]
        adv[t] = last = delta + np.float32(gamma) * np.float32(lam) * nnt * last
    return adv + val


def _random_flags(rs, T, N, S):
    """AGENT_* flags of a plausible play: snakes die and stay dead (snake_env pattern) or come alive again (new_world
    pattern), envs finish and everyone is alive again after the reset."""
    flags = np.zeros((T, N, S), np.uint8)
    alive = np.ones((N, S), bool)
    for t in range(T):
        was = alive.copy()
        revive = rs.random((N, S)) < 0.3
        now = np.where(was, rs.random((N, S)) > 0.25, revive & (np.arange(N)[:, None] % 2 == 1))   # odd envs: new_world
        done = rs.random(N) < 0.2
        died = was & ~now
        ended = was & (died | done[:, None])
        flags[t] = now * ap.ALIVE + was * ap.WAS_ALIVE + died * ap.DIED + ended * ap.ENDED
        alive = np.where(done[:, None], True, now)
    return flags


def test_agent_targets_equal_gae_on_every_run_of_valid_samples():
    import torch
    from msnake import selfplay
    T, N, S, gamma, lam = 9, 5, 3, 0.99, 0.95
    rs = np.random.default_rng(5)
    flags = _random_flags(rs, T, N, S)
    flags[3, 0, 0] &= ~np.uint8(ap.WAS_ALIVE | ap.ENDED | ap.DIED)   # a hole in a run that no ENDED closes (a stale tracker)
    flags[2, 0, 0] = ap.ALIVE | ap.WAS_ALIVE
    flags[4, 0, 0] = ap.ALIVE | ap.WAS_ALIVE
    rew = rs.integers(-1, 3, (T, N, S)).astype(np.float32)
    val = rs.normal(size=(T, N, S)).astype(np.float32)
    last_val = rs.normal(size=(N, S)).astype(np.float32)
    valid, ended = (flags & ap.WAS_ALIVE) != 0, (flags & ap.ENDED) != 0
    assert valid.any(axis=0).all() and (~valid).any() and ended.any() and (valid[-1] & ~ended[-1]).any(), "the cases are there"
    got, got_valid = selfplay.agent_targets(torch.from_numpy(rew), torch.from_numpy(val), torch.from_numpy(flags),
                                            torch.from_numpy(last_val), gamma, lam)
    got, got_valid = got.numpy(), got_valid.numpy()
    assert got_valid.dtype == bool and np.array_equal(got_valid, valid)
    assert (got[~valid] == 0).all(), "an invalid sample contributes nothing"
    runs = revivals = 0
    for n in range(N):
        for s in range(S):
            t = 0
            while t < T:
                if not valid[t, n, s]:
                    t += 1
                    continue
                t0 = t
                while t < T and valid[t, n, s]:
                    t += 1
                t1 = t - 1   # the run is [t0, t1]
                runs += 1
                revivals += t0 > 0
                at_end = t1 == T - 1
                # behind the run: the bootstrap value at the end of the rollout, nothing in front of an invalid sample
                last_ended = float(ended[t1, n, s]) if at_end else 1.0
                lv = last_val[n, s] if at_end else np.float32(0.0)
                seg = slice(t0, t1 + 1)
                want = _np_gae_run(rew[seg, n, s], val[seg, n, s], ended[seg, n, s].astype(np.float32), lv, last_ended, gamma, lam)
                # float32 on both sides, the same operations in the same order; 4 ulp of the largest magnitude for the
                # two libraries' freedom to fuse a multiply-add
                tol = 4 * np.finfo(np.float32).eps * max(1.0, float(np.abs(want).max()))
                assert np.allclose(got[seg, n, s], want, rtol=0, atol=tol), (n, s, t0, t1, got[seg, n, s], want)
                # ... and selfplay.gae itself on the run alone, bit for bit
                dones = np.concatenate([[0.0], ended[t0:t1, n, s].astype(np.float32)]).astype(np.float32)
                ref, _ = selfplay.gae(torch.from_numpy(rew[seg, n, s].copy())[:, None], torch.from_numpy(val[seg, n, s].copy())[:, None],
                                      torch.from_numpy(dones)[:, None], torch.tensor([lv]), torch.tensor([last_ended]), gamma, lam)
                assert np.array_equal(got[seg, n, s], ref.numpy()[:, 0]), (n, s, t0, t1)
    assert runs > N * S and revivals >= 5, (runs, revivals)


# ------------------------------------------------------------------------------------------ Runner(all_snakes=True)
class _StubEnv:
    """What Runner looks at before it touches the device."""
    num_envs, n_snakes = 4, 3

    def __init__(self, auto_reset):
        self._ctor = {"auto_reset": auto_reset}

    def reset_device(self):
        raise AssertionError("a refused Runner must not touch the env")


@pytest.mark.parametrize("kw,auto_reset,opponents,match", [
    (dict(), False, [], "rays=True or local_radius"),
    (dict(rays=True), False, [None, None], "no opponent"),
    (dict(local_radius=3), False, [object()], "no opponent"),
    (dict(rays=True), True, [], "auto_reset=False"),
    (dict(rays=True, local_radius=3), False, [], "mutually exclusive"),
])
def test_runner_all_snakes_refusals(kw, auto_reset, opponents, match):
    from msnake import selfplay
    with pytest.raises(ValueError, match=match):
        selfplay.Runner(_StubEnv(auto_reset), None, opponents, 8, 0.99, 0.95, all_snakes=True, **kw)


def test_learn_all_snakes_refusals():
    from msnake import selfplay
    env = _StubEnv(False)
    with pytest.raises(ValueError, match="rays=True or local_radius"):
        selfplay.learn(env, all_snakes=True)
    with pytest.raises(ValueError, match="scripted_opponents must be empty"):
        selfplay.learn(env, all_snakes=True, rays=True, scripted_opponents={1: "safe_greedy"})
