"""msnake_set_state / msnake_set_state_all at the edge of what they accept, and the step after.

The case table and the scenarios are tests/state_domain.py's (written from include/msnake.h; test_state_domain_host.py
proves on the oracle alone that each scenario does what it is there for).  Expected values come from the model
(which reason), from the words that were handed in (what an accepted install returns) and from the CPU oracle, which
imports every accepted state and never sees a refused one.  Every comparison is byte-exact.
"""

import numpy as np
import pytest

import state_domain as sd

pytestmark = pytest.mark.gpu

N_ROWS, N, VICTIM, NEIGHBOUR = 8, 10, 4, 5
RECORDS = {"S5": ("full", "short"), "A5": ("full", "short"), "N6": ("full",), "S10": ("full", "short"), "A10": ("full", "short")}


class Both:
    """A MultiSnakeVecEnv and the oracle of the same configuration, kept in step."""

    def __init__(self, key, n, seed=11, **kw):
        import msnake
        cfg = sd.CFGS[key]
        self.cfg, self.n, self.ns = cfg, n, cfg["n_snakes"]
        self.env = msnake.MultiSnakeVecEnv(n, seed=seed, **cfg, **kw)
        self.ora = sd.make_oracle(cfg, n, seed=seed)
        assert np.array_equal(self.env.reset(), self.ora.reset())

    def install(self, e, words):
        self.env.set_state_words(e, words)
        assert sd.imports(self.ora, e, words) == 0

    def words(self):
        return sd.blob_words(self.env.get_state_all())

    def check_words(self, what, skip=()):
        for e, got in enumerate(self.words()):
            if e not in skip:
                want = sd.export(self.ora, e)
                assert np.array_equal(got, want), (what, e, got[:16], want[:16])

    def check_outputs(self, obs, rew, done, what, skip=()):
        keep = np.array([e not in skip for e in range(self.n)])
        o_obs, o_rew, o_done = self.ora.obs, self.ora.rew, self.ora.done
        assert np.array_equal(rew[keep], o_rew[keep]) and np.array_equal(done[keep].astype(bool), o_done[keep].astype(bool)), what
        assert np.array_equal(obs[keep], o_obs[keep]), what

    def step(self, act, what, skip=()):
        obs, rew, done, _ = self.env.step(act)
        self.ora.step(act)
        self.check_outputs(obs, rew, done, what, skip)

    def run(self, acts, path, what, skip=()):
        """acts [T, n, ns] on msnake_step, msnake_step_tape ("tape") or msnake_rollout_tape ("rollout")."""
        if path == "step":
            for t, act in enumerate(acts):
                self.step(act, (what, t), skip)
            return
        import torch
        obs, rew, done, _ = self.env.rollout_device(torch.from_numpy(np.ascontiguousarray(acts)).to(self.env.device),
                                                    persistent=path == "rollout")
        obs, rew, done = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy()
        for t, act in enumerate(acts):
            self.ora.step(act)
            self.check_outputs(obs[t], rew[t], done[t], (what, t), skip)

    def actions(self, rs, steps, rows=None):
        """Random moves for every env; `rows`: {env: one action row, or a list of them per step}."""
        acts = rs.integers(0, 5, (steps, self.n, self.ns)).astype(np.int32)
        for e, r in (rows or {}).items():
            acts[:, e] = np.asarray(r, np.int32)
        return acts

    def errors(self):
        return self.env.stats()["errors"]


# ------------------------------------------------------------------------------------------ B. refusals
@pytest.mark.parametrize("key,record", [(k, r) for k in sorted(sd.TABLE_KEYS) for r in RECORDS[k]])
def test_every_row_through_set_state(key, record):
    """Accepted rows install and come back word for word; refused rows raise MSNAKE_E_STATE with the reason's text and
    leave the env's words and the frame as they were.  One step after every row all envs equal an oracle that was
    given the accepted words and never saw the refused ones."""
    b = Both(key, N_ROWS, record_policy=record)
    cfg, env, ora = b.cfg, b.env, b.ora
    rs = np.random.default_rng(3)
    for t in range(3):
        b.step(b.actions(rs, 1)[0], ("warm-up", t))
    for i, (name, build, expect) in enumerate(sd.rows(key)):
        e = (3 * i + 1) % N_ROWS
        w = build()
        assert sd.accepts(cfg, w) == expect, name
        if expect is None:
            b.install(e, w)
            assert np.array_equal(env.get_state_words(e), w[:sd.canonical_len(cfg, w)]), name
        else:
            before, frame = env.get_state_words(e).copy(), env.render().copy()
            with pytest.raises(RuntimeError, match=sd.REASON_RE[expect]) as err:
                env.set_state_words(e, w)
            assert "(-5)" in str(err.value), name
            assert np.array_equal(env.get_state_words(e), before), name
            assert np.array_equal(env.render(), frame), name
        b.step(b.actions(rs, 1)[0], name)
        b.check_words(name)
        if expect is None:   # back to play from a reset: the table's states are not meant to be played on
            mask = np.arange(N_ROWS) == e
            obs = env.reset(mask)
            ora.reset_envs(mask, obs=None, final_obs=None, truncated=None)
            assert np.array_equal(obs[e], ora.render()[e]), name
    assert b.errors() == 0
    env.close()


@pytest.mark.parametrize("key", ["S5", "N6", "A5"])
def test_set_state_all_with_three_bad_envs(key):
    """One blob of good envs and three bad ones, each bad for another reason: the message has the count, the lowest
    bad index and its reason; the bad envs stay as they were and every good env of the blob is installed."""
    b = Both(key, N_ROWS)
    cfg, env, ora = b.cfg, b.env, b.ora
    rs = np.random.default_rng(5)
    for t in range(3):
        b.step(b.actions(rs, 1)[0], ("warm-up", t))
    other = sd.make_oracle(cfg, N_ROWS, seed=77)
    other.reset()
    for t in range(4):
        other.step(rs.integers(0, 5, (N_ROWS, b.ns)).astype(np.int32))
    table = {name: (build, expect) for name, build, expect in sd.rows(key)}
    bad = {2: "grow_to = -1", 5: "len cap - 1", 6: "head at c0 = -2"}
    assert [table[bad[e]][1] for e in (2, 5, 6)] == [sd.R_SCALAR, sd.R_LEN, sd.R_CELL]
    env_words = [table[bad[e]][0]() if e in bad else sd.export(other, e) for e in range(N_ROWS)]
    before, frame = b.words(), env.render().copy()
    assert all(not np.array_equal(before[e], env_words[e]) for e in range(N_ROWS))
    msg = rf"3 env state\(s\) rejected; first: env 2: {sd.REASON_RE[sd.R_SCALAR]}.*left untouched"
    with pytest.raises(RuntimeError, match=msg) as err:
        env.set_state_all(sd.make_blob(cfg, env_words))
    assert "(-5)" in str(err.value)
    after, frame_after = b.words(), env.render()
    for e in range(N_ROWS):
        if e in bad:
            assert np.array_equal(after[e], before[e]) and np.array_equal(frame_after[e], frame[e]), e
        else:
            assert np.array_equal(after[e], env_words[e]), e
            assert sd.imports(ora, e, env_words[e]) == 0
    b.step(b.actions(rs, 1)[0], "the step after")
    b.check_words("the step after")
    # a blob of accepted states only goes in whole
    good = [sd.export(other, e) for e in range(N_ROWS)]
    env.set_state_all(sd.make_blob(cfg, good))
    for e in range(N_ROWS):
        assert sd.imports(ora, e, good[e]) == 0
    b.check_words("all good")
    assert b.errors() == 0
    env.close()


@pytest.mark.parametrize("key", ["S5", "N6", "A5"])
def test_word_7_is_checked_alike_on_the_host_and_on_the_device(key):
    """msnake_set_state looks at the low byte of word 7 before any device work, the device at the whole word: a stray
    bit is MSNAKE_E_STATE whichever of the two sees it, through both entry points."""
    b = Both(key, N_ROWS)
    env, ns = b.env, b.ns
    before = b.words()
    for w7 in (ns | 0x80, ns | 0x40, ns ^ 1, ns | 0x200, ns | 0x10000, ns | 0x300, ns - (1 << 31), 0x100, ns | 0x100 | 0x1000):
        w = sd.base_words(key)
        w[7] = w7
        assert sd.accepts(b.cfg, w) == sd.R_SNAKES
        with pytest.raises(RuntimeError, match=sd.REASON_RE[sd.R_SNAKES]) as err:
            env.set_state_words(3, w)
        assert "(-5)" in str(err.value), hex(w7)
        words = [x.copy() for x in before]
        words[3] = w
        with pytest.raises(RuntimeError, match=r"1 env state\(s\) rejected; first: env 3: snake count differs") as err:
            env.set_state_all(sd.make_blob(b.cfg, words))
        assert "(-5)" in str(err.value), hex(w7)
    after = b.words()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    env.close()


# ------------------------------------------------------------------------------------------ C. the step after
def truncated_list(words, n):
    """`words` with the fruit list cut to its first n entries."""
    st = sd.St(words)
    st.fruits = st.fruits[:n]
    return st.flat()


@pytest.mark.parametrize("over", [0, 3])
@pytest.mark.parametrize("epb", [1, 8])
@pytest.mark.parametrize("record", ["full", "short"])
@pytest.mark.parametrize("path", ["step", "tape", "rollout"])
def test_adversarial_list_exactly_full_and_over(path, record, epb, over):
    """Two snakes die and their pieces take the fruit list to exactly fcap (over 0: everything equals the oracle, no
    error) or to fcap + 3 (the list ends at fcap, the first fcap entries are the oracle's, one error is counted).  The
    next env holds a full list of its own, which get_state shows: it and every other env equal the oracle."""
    b = Both("A5", N, record_policy=record, envs_per_block=epb)
    F = sd.fcap(b.cfg)
    words, act, _, _ = sd.adv_wall(over)
    b.install(VICTIM, words)
    b.install(NEIGHBOUR, sd.adv_full_neighbour())
    acts = b.actions(np.random.default_rng(7), 2, {VICTIM: act, NEIGHBOUR: [0, 0, 0]})
    skip = (VICTIM,) if over else ()
    b.run(acts, path, "wall", skip)
    b.check_words("wall", skip)
    got = b.words()
    assert int(got[NEIGHBOUR][6]) == F and int(got[VICTIM][6]) == F
    if over:
        want = sd.export(b.ora, VICTIM)
        assert int(want[6]) == F + over
        assert np.array_equal(got[VICTIM], truncated_list(want, F))
    assert b.errors() == (1 if over else 0)
    b.env.close()


@pytest.mark.parametrize("path", ["step", "rollout"])
def test_adversarial_list_overflows_by_growth_after_the_install(path):
    """At the install the list and every body together fill the list exactly; two snakes then eat, grow and die: the
    first death fits, the second is over by 3."""
    b = Both("A5", N)
    F = sd.fcap(b.cfg)
    words, act, lengths = sd.adv_growth()
    b.install(VICTIM, words)
    b.install(NEIGHBOUR, sd.adv_full_neighbour())
    acts = b.actions(np.random.default_rng(9), len(lengths), {VICTIM: act, NEIGHBOUR: [0, 0, 0]})
    b.run(acts[:-1], path, "growth")
    b.check_words("growth, before the second death")
    assert int(b.words()[VICTIM][6]) == lengths[-2] and b.errors() == 0
    b.run(acts[-1:], path, "growth, last", (VICTIM,))
    b.check_words("growth, last", (VICTIM,))
    got, want = b.words(), sd.export(b.ora, VICTIM)
    assert int(want[6]) == lengths[-1] == F + 3 and int(got[VICTIM][6]) == F
    assert np.array_equal(got[VICTIM], truncated_list(want, F))
    assert b.errors() == 1
    b.env.close()


@pytest.mark.parametrize("eat", [False, True])
@pytest.mark.parametrize("key", ["S5", "A5", "N6"])
def test_grow_to_zero_and_grow_to_len(key, eat):
    """grow_to = 0 and grow_to = len on a step without a meal (every rule set's vector update) and on a step on which
    another snake of the env eats (adversarial, new_world: the sequential update).  grow_to = -1, which the two
    updates would treat differently, is refused (the table's row, through both entry points above)."""
    b = Both(key, N)
    words, act = sd.grow_limits(key, eat)
    b.install(VICTIM, words)
    steps = sd.grow_limits_steps(key)
    acts = b.actions(np.random.default_rng(13), steps, {VICTIM: act})
    for t in range(steps):
        b.step(acts[t], ("grow_to", t))
        b.check_words(("grow_to", t))
    bad = sd.St(words)
    bad.snakes[b.ns - 1]["grow"] = -1
    with pytest.raises(RuntimeError, match=sd.REASON_RE[sd.R_SCALAR]):
        b.env.set_state_words(VICTIM, bad.flat())
    b.check_words("after the refusal")
    assert b.errors() == 0
    b.env.close()


@pytest.mark.parametrize("path", ["step", "rollout"])
@pytest.mark.parametrize("key", ["N6", "S5", "A5"])
def test_body_capacity_guard(key, path):
    """A body of cap - 2 pieces with grow_to 10^6: cap - 1 after the first step, like the oracle and without an error;
    on the second step the guard holds it at cap - 1 and counts.  The other envs follow the oracle throughout."""
    b = Both(key, N)
    C = sd.cap(b.cfg)
    words, rows, s = sd.body_guard(key)
    b.install(VICTIM, words)
    acts = b.actions(np.random.default_rng(21), len(rows), {VICTIM: rows})
    b.run(acts[:1], path, "first")
    b.check_words("first")
    assert len(sd.St(b.env.get_state_words(VICTIM)).snakes[s]["cells"]) == C - 1 and b.errors() == 0
    b.run(acts[1:2], path, "second", (VICTIM,))
    b.check_words("second", (VICTIM,))
    assert b.errors() >= 1
    got = sd.St(b.env.get_state_words(VICTIM))
    assert len(got.snakes[s]["cells"]) == C - 1 and len(sd.St(sd.export(b.ora, VICTIM)).snakes[s]["cells"]) == C
    if path == "step":
        for t in range(2, len(rows)):
            b.run(acts[t:t + 1], path, ("further", t), (VICTIM,))
            b.check_words(("further", t), (VICTIM,))
    else:
        b.run(acts[2:], path, "further", (VICTIM,))
        b.check_words("further", (VICTIM,))
    assert all(len(sn["cells"]) <= C - 1 for sn in sd.St(b.env.get_state_words(VICTIM)).snakes)
    b.env.close()


@pytest.mark.parametrize("path", ["step", "rollout"])
@pytest.mark.parametrize("key", ["S19", "S5", "A5", "N6"])
def test_a_head_outside_the_grid_that_turns_back_in(key, path):
    """An installed head outside the grid can turn back into it; the cell outside then stays in the body, and the frame
    shows the wall there, as the reference's does.  S19 is a shape with step kernels of its own, whose painter has no
    clip: the handle goes over to the generic kernels when such a head is installed, and so does a handle that receives
    its envs by msnake_copy_envs."""
    b = Both(key, N)
    spec = key == "S19"
    assert b.env.kernel_name().endswith(", 19>") == spec
    words, rows = sd.turn_back(key)
    b.install(VICTIM, words)
    assert ", 19>" not in b.env.kernel_name()
    acts = b.actions(np.random.default_rng(31), len(rows), {VICTIM: rows})
    twin = b.env.clone()
    assert ", 19>" not in twin.kernel_name()
    b.run(acts, path, "turn back")
    b.check_words("turn back")
    for t in range(len(rows)):
        obs = twin.step(acts[t])[0]
    assert np.array_equal(obs, b.ora.obs)
    assert b.errors() == 0 and twin.stats()["errors"] == 0
    twin.close()
    b.env.close()
