"""The scenarios of tests/limits_play.py on the oracle alone: each does what tests/test_limits_gpu.py needs it for.
No GPU; the library is asked only for what its host glue decides without one (msnake_kernel_name_for_config).
"""
import ctypes

import numpy as np
import pytest

import limits_play as lp
import scripted_play as sp
import state_domain as sd
import timed_play as tmp


# ------------------------------------------------------------------------------------------ the bounds of max_steps
def _name_for(rules, max_steps, dim=12, n_snakes=2, n_fruits=None):
    import msnake
    C = msnake._capi
    cfg = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, 8, dim, n_snakes, n_snakes if n_fruits is None else n_fruits,
                         C.RULES[rules], max_steps, 1, 1, 0, 0, 0, 0, 0, 0)
    return C.kernel_name_for_config(cfg)


@pytest.mark.parametrize("rules", sorted(sd.RULES))
def test_max_steps_is_accepted_up_to_60000_and_no_further(rules):
    assert _name_for(rules, 60000).startswith("msnake_step_kernel<")
    assert _name_for(rules, 1).startswith("msnake_step_kernel<")
    for bad in (60001, 0, -1, 65536, 1 << 16 | 2000):
        with pytest.raises(RuntimeError, match=r"max_steps must be in \[1, 60000\]"):
            _name_for(rules, bad)


def test_new_world_sizes_the_body_storage_from_max_steps():
    for max_steps, cap in ((60000, 60032), (32800, 32832), (32768, 32832), (32766, 32768), (2000, 2048)):
        cfg = lp.cfg_of(max_steps)
        assert sd.cap(cfg) == sp.ring_cap(dict(cfg, rules=sp.RULES["new_world"])) == cap
    # ... and the other two rule sets from the board alone
    for rules in ("snake_env", "adversarial"):
        cfg = dict(lp.cfg_of(60000), rules=rules)
        assert sd.cap(cfg) == sp.ring_cap(dict(cfg, rules=sp.RULES[rules])) == 192


# ------------------------------------------------------------------------------------------ A. long bodies
@pytest.mark.parametrize("case", sorted(lp.LONG))
def test_long_bodies_import_and_come_back(case):
    c = lp.LONG[case]
    cfg, words = lp.cfg_of(c["max_steps"]), lp.long_states(case)
    cap = sd.cap(cfg)
    assert 4 <= len(words) <= 8 and max(c["lens"]) == cap - 2
    if case == "a":
        assert {32767, 32768, 32769, 40000, 60030} <= set(c["lens"]) and cap == 60032
    else:
        assert cap == 32832 and 32830 in c["lens"]
    ora = lp.make_oracle(cfg, words)
    heads = set()
    for e, w in enumerate(words):
        assert np.array_equal(sd.export(ora, e), w), e
        st = sd.St(w)
        body = st.snakes[1]["cells"]
        assert len(body) == c["lens"][e] and st.snakes[0]["cells"] == [] and (st.snakes[0]["alive"], st.snakes[0]["in_dead"]) == (0, 1)
        assert len({tuple(p) for p in body}) == lp.FOLD + 1 and body.count(body[0]) == 1
        assert all(abs(p[0] - q[0]) + abs(p[1] - q[1]) == 1 for p, q in zip(body[:200], body[1:200]))
        assert tuple(st.fruits[0]) not in {tuple(p) for p in body}
        heads.add(tuple(body[0]))
    assert len(heads) == len(words)                                   # every env starts on another cell


@pytest.mark.parametrize("max_steps", [60000, 32800])
def test_the_lengths_refused_at_the_large_caps(max_steps):
    cfg = lp.cfg_of(max_steps)
    cap = sd.cap(cfg)
    assert sd.accepts(cfg, lp.long_words(20, cap - 2, 3)) is None
    assert sd.accepts(cfg, lp.too_long_words(cap - 1)) == sd.R_LEN
    w = lp.too_long_words(65536, cells=cap - 2)
    assert lp.body_len(w) == 65536 and lp.body_len(w) & 0xFFFF == 0 and sd.accepts(cfg, w) == sd.R_LEN


# ------------------------------------------------------------------------------------------ B. the rotated ring
@pytest.mark.parametrize("case", sorted(lp.LONG))
def test_long_play_is_clear_for_130_steps_and_ends_on_its_own_trail(case):
    c, rec = lp.LONG[case], lp.long_play(case)
    assert lp.PLAY >= 130 and lp.PLAY < lp.CLEAR + 1 <= lp.PLAY + lp.BEYOND and rec.steps == lp.PLAY + lp.BEYOND
    assert not rec.done.any()                                         # the main snake is dead: only the step cap ends this
    for k in range(rec.steps + 1):
        alive = [h[1][4] for h in rec.headers[k]]
        assert alive == [int(k <= lp.CLEAR)] * rec.n, k               # the head meets the trail on step CLEAR + 1 = 134
        lens = rec.lens(k)
        # a body at or above grow_to keeps its length (one pop per fruit, one push); below it, it grows by one per step
        assert lens == [ln + (k if g > ln else 0) for ln, g in zip(c["lens"], c["grow"])], k
        assert min(lens) > 64 and max(lens) <= sd.cap(rec.cfg) - 2, k  # every step evicts a piece into the ring
    assert all(int(w[0]) == rec.steps for w in rec.end)               # no reset on the way
    # the fruit is eaten on the way (grow_to rises, the draw counter moves)
    assert all(int(a[1]) < int(b[1]) for a, b in zip(rec.start, rec.words[lp.PLAY]))
    assert (rec.info[:lp.CLEAR, :, 2] == 1).all() and (rec.info[lp.CLEAR:, :, 2] == 0).all()      # num_snakes


def test_the_ring_position_lies_above_2_to_15_and_crosses_it():
    """From the capacity and the step count: k steps after the install the position is (cap - k) mod cap."""
    cap_a, cap_b = (sd.cap(lp.cfg_of(lp.LONG[c]["max_steps"])) for c in "ab")
    T = lp.PLAY + lp.BEYOND
    assert lp.ohp_after(cap_a, 1) == cap_a - 1 == 60031
    assert all(lp.ohp_after(cap_a, k) > 32767 for k in range(1, T + 1))
    seen = [lp.ohp_after(cap_b, k) for k in range(1, lp.PLAY + 1)]
    assert seen[0] == 32831 and 32768 in seen and 32767 in seen and min(seen) < 32767
    at = lp.check_steps("b")
    assert {lp.ohp_after(cap_b, k) for k in at} >= {0, 32831, 32768, 32767} and at[-1] == lp.PLAY
    assert lp.check_steps("a")[0] == 1 and lp.check_steps("a")[-1] == lp.PLAY and len(lp.check_steps("a")) >= 3
    # the walk over pieces 64.. wraps around the end of the ring in both cases
    assert lp.ohp_after(cap_a, 1) + 60030 - 64 > cap_a and lp.ohp_after(cap_b, 64) + 32830 - 64 > cap_b


def test_lifetimes_below_and_on_the_clamp():
    rec = lp.long_play("a")
    k = lp.check_steps("a")[0]
    want = lp.long_expectations("a", k)
    lens = [lp.body_len(w) for w in rec.words[k]]
    assert lens[4] == 60030 and int(want["life"][4].max()) == 60030 < tmp.LIFE_CAP     # the head's cell, below the clamp
    assert int(want["life"][5].max()) == tmp.LIFE_CAP and lens[5] + 6000 > tmp.LIFE_CAP  # on it
    assert int((want["life"][5] == tmp.LIFE_CAP).sum()) >= 2
    assert all(int(want["life"][e].max()) == lens[e] for e in range(4))


# ------------------------------------------------------------------------------------------ C. the guard at the largest cap
def test_the_guard_scenario_passes_the_capacity_on_the_second_step():
    cfg, words = lp.cfg_of(60000), lp.guard_states()
    cap = sd.cap(cfg)
    assert cap == 60032 and lp.body_len(words[lp.GUARD_VICTIM]) == cap - 2
    assert sd.St(words[lp.GUARD_VICTIM]).snakes[1]["grow"] == (1 << 31) - 1
    rec = lp.guard_play()
    assert not rec.done.any() and rec.steps == lp.GUARD_STEPS >= 3
    lens = [[lp.body_len(w) for w in rec.words[k]] for k in range(rec.steps + 1)]
    assert [row[lp.GUARD_VICTIM] for row in lens] == [cap - 2 + k for k in range(rec.steps + 1)]   # the oracle has no capacity
    assert lens[1][lp.GUARD_VICTIM] == cap - 1 and lens[2][lp.GUARD_VICTIM] == cap
    for e in range(len(words)):
        if e != lp.GUARD_VICTIM:
            assert [row[e] for row in lens] == [lens[0][e]] * (rec.steps + 1) and 64 < lens[0][e] < cap - 2
    # nobody eats: grow_to 2^31 - 1 stays where it is
    assert sd.St(rec.words[rec.steps][lp.GUARD_VICTIM]).snakes[1]["grow"] == (1 << 31) - 1


# ------------------------------------------------------------------------------------------ D. copies between capacities
def test_what_fits_the_smaller_handle():
    src, dst = lp.cfg_of(lp.COPY["src_max_steps"]), lp.cfg_of(lp.COPY["dst_max_steps"])
    words = lp.copy_states()
    cap = sd.cap(dst)
    assert sd.cap(src) == 60032 and cap == 32832
    assert [lp.body_len(w) for w in words] == [cap - 1, cap, 60030, 32767, 100]
    assert all(sd.accepts(src, w) is None for w in words)
    assert [lp.fits(dst, w) for w in words] == [True, False, False, True, True]
    # cap - 1 pieces fit the storage but are more than msnake_set_state takes: only a copy brings them in
    assert sd.accepts(dst, words[0]) == sd.R_LEN and sd.accepts(dst, words[3]) is None
    back = lp.copy_back_states()
    assert all(sd.accepts(dst, w) is None and sd.accepts(src, w) is None for w in back)
    assert max(lp.body_len(w) for w in back) == cap - 2
    # the large handle's ring has rotated by then, above 2^15
    assert 32767 < lp.ohp_after(sd.cap(src), lp.COPY_SRC_STEPS) < sd.cap(src) - 1
    rec = lp.copy_src_play()
    assert not rec.done.any() and all(lp.alive_bit(w) == 1 for w in rec.end)


# ------------------------------------------------------------------------------------------ E. the step cap
@pytest.mark.parametrize("max_steps", [60000, 32768])
@pytest.mark.parametrize("key", sorted(lp.CAP_CONFIGS))
def test_done_first_rises_on_the_step_that_reaches_the_cap(key, max_steps):
    cfg, words = lp.cap_states(key, max_steps)
    assert len(words) == lp.CAP_N and all(sd.accepts(cfg, w) is None for w in words)
    assert [int(w[0]) for w in words] == [int(w[4]) for w in words] == [max_steps - 4 + e % 4 for e in range(lp.CAP_N)]
    assert any(int(w[5]) != 0 for w in words) or cfg["rules"] == "new_world"          # returns of play, not of a reset
    assert max(lp.body_len(w, s) for w in words for s in range(cfg["n_snakes"])) >= 2
    rec = lp.cap_play(key, max_steps, resets=False)
    at_cap = 0
    for e in range(lp.CAP_N):
        first = int(np.argmax(rec.done[:, e])) if rec.done[:, e].any() else None
        cap_step = 4 - e % 4                                          # 1-based: the step that makes ep_len max_steps
        assert first is not None and first + 1 <= cap_step, (e, first)
        assert rec.done[first:, e].all()                              # without a reset a finished env stays done
        if first + 1 == cap_step:
            at_cap += 1
            assert rec.info[first, e, 1] == max_steps and rec.info[first, e, 3] == 1
        else:                                                         # the rule set's own end came first
            assert rec.info[first, e, 1] < max_steps
    assert at_cap >= lp.CAP_N // 2, at_cap
    # with the masked reset after every step: the flags say which episodes the cap alone ended
    rec = lp.cap_play(key, max_steps, resets=True)
    assert int(sum(int(t.sum()) for t in rec.truncated.values())) >= lp.CAP_N // 2
    assert rec.ep_len_sum >= at_cap * max_steps and rec.episodes >= lp.CAP_N


# ------------------------------------------------------------------------------------------ F. the longest body of play
def test_the_body_play_can_reach_by_the_cap_fits_the_storage():
    cfg = lp.reach_cfg()
    cap = sd.cap(cfg)
    grown = lp.growth(40)
    ln0, grow0 = grown[0]
    assert grown == [(ln0 + k, grow0) for k in range(41)]             # never pops: one piece per step, grow_to stays
    length, grow = lp.reach_body()
    assert (length, grow) == (ln0 + lp.REACH["t0"], grow0) and 32768 < length
    assert length + (cfg["max_steps"] - lp.REACH["t0"]) < cap - 1     # what max_steps + 2 is there for
    rec = lp.reach_play()
    to_cap = cfg["max_steps"] - lp.REACH["t0"]
    assert to_cap < lp.CLEAR and rec.steps == to_cap + 2
    assert not rec.done[:to_cap - 1].any() and rec.done[to_cap - 1].all()
    assert (rec.info[to_cap - 1, :, 1] == cfg["max_steps"]).all()
    assert [lp.body_len(w) for w in rec.words[to_cap - 1]] == [length + to_cap - 1] * rec.n
    assert max(lp.body_len(w) for k in rec.words for w in rec.words[k]) < cap - 1
