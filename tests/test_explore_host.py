"""CPU-side checks of exploring play (msnake_explore_actions, msnake_playout_explore, MultiSnakeVecEnv.explore_actions_device
and the explore / salt arguments of playout_device / playout_values_device): the entry points are declared, exported and
bound as declared; properties of the restatement tests/explore_play.py, from the reference alone; what its scenarios
reach; the Python methods against a recording fake library; the register budget of the two kernels.  No GPU."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import msnake
import explore_play as xp
import playout_play as pp
from kernel_resources import unit_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = msnake._capi


# ------------------------------------------------------------------------------------------ the C entry points
def test_header_declares_and_library_exports_both_entry_points():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    head = r"msnake_handle h, const int32_t policies\[MSNAKE_MAX_SNAKES\],\s*const uint32_t eps_q16\[MSNAKE_MAX_SNAKES\], uint64_t salt, "
    assert re.search(r"\bint msnake_explore_actions\(" + head + r"uint32_t snake_mask,\s*int32_t\* actions_dev, int32_t action_stride, "
                     r"uint8_t\* explored_dev, void\* stream\);", text)
    assert re.search(r"\bint msnake_playout_explore\(" + head + r"int32_t n_steps,\s*const int32_t\* first_dev, int32_t first_stride, "
                     r"uint32_t first_mask, int32_t\* steps_dev,\s*uint8_t\* end_dev, float\* ret_dev, int32_t\* info_dev, int32_t\* words_dev, "
                     r"int32_t words_stride,\s*int32_t\* count_dev, void\* stream\);", text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "0x6578706C6F726521" in text and bytes.fromhex("6578706C6F726521") == b"explore!" and xp.TAG == 0x6578706C6F726521
    assert "msnake_explore_actions" in C.SYMBOLS and "msnake_playout_explore" in C.SYMBOLS
    assert C.EXPLORE_ONE == xp.ONE == 65536
    lib = C.load()
    assert lib.msnake_explore_actions is not None and lib.msnake_playout_explore is not None and lib.msnake_abi_version() == 3


def test_the_bindings_have_the_declared_signatures():
    vp, i32, u32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64
    head = [vp, ctypes.POINTER(i32), ctypes.POINTER(u32), u64]
    want = {"msnake_explore_actions": head + [u32, vp, i32, vp, vp],
            "msnake_playout_explore": head + C.PROTOTYPES["msnake_playout"][1][2:]}   # msnake_playout's arguments from n_steps on
    for name, argtypes in want.items():
        restype, bound = C.PROTOTYPES[name]
        assert restype is ctypes.c_int and bound == argtypes, name
        fn = getattr(C.load(), name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes, name


def test_null_handle_is_refused_first():
    lib = C.load()
    assert lib.msnake_explore_actions(None, None, None, 0, 0, None, 0, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    assert lib.msnake_playout_explore(None, None, None, 0, 0, None, 0, 0xFF, None, None, None, None, None, 0, None, None) == -3
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ properties of the restatement
def test_the_draw_is_the_documented_stream():
    from oracle.snake_oracle import philox_block
    seed, salt, G, t, ctr = 3, 7, (1 << 33) + 5, 0xFFFFFFFF, (1 << 40) + 9
    k64 = xp.mix64(xp.mix64(seed ^ xp.mix64(salt ^ xp.TAG)) ^ ctr)
    for s in range(4):
        j = 8 * t + 2 * s                                           # past 2^32: the block index carries into the counter's high word
        blk = philox_block([(j >> 2) & 0xFFFFFFFF, j >> 34, G & 0xFFFFFFFF, G >> 32], [k64 & 0xFFFFFFFF, k64 >> 32])
        assert xp.explore_draw(seed, salt, G, t, ctr, s) == (blk[j & 3], blk[(j & 3) + 1]), s
    assert xp.explore_draw(seed, salt, G, 5, ctr, 1) != xp.explore_draw(seed, salt, G, 5, ctr + 1, 1)
    assert xp.explore_draw(seed, salt, G, 5, ctr, 1) != xp.explore_draw(seed, salt + 1, G, 5, ctr, 1)


@pytest.mark.parametrize("name", ["A", "B"])
def test_with_every_eps_zero_the_playout_is_np_playout(name):
    sc, (ref, _) = pp.scenario(name), pp.reference(name)
    for salt in (0, 0xDEADBEEFCAFEF00D):
        got = xp.np_playout_explore(sc["cfg"], sc["states"], sc["policies"], 0, salt, sc["K"])
        assert xp.same_result(got, ref), (name, salt)


def test_at_eps_one_every_action_is_drawn_from_its_candidate_set():
    for name in ("XB", "XD"):
        sc = xp.scenario(name)
        cfg, S = sc["cfg"], sc["cfg"]["n_snakes"]
        act, explored, n = xp.np_explore_actions(cfg, sc["states"], sc["policies"], xp.ONE, sc["salt"])
        assert np.array_equal(explored, (n > 0).astype(np.uint8)) and (n > 0).any() and (n == 0).any()   # (dead snakes: no candidates)
        seen = set()
        for e, st in enumerate(sc["states"]):
            cand = xp.candidates(st, cfg["dim"], S, sc["policies"])
            for s in range(S):
                assert (act[e, s] in cand[s]) if cand[s] else (act[e, s] == pp.policy_actions(st, cfg["dim"], S, pp.per_snake(sc["policies"], S))[s])
                if len(cand[s]) > 1:
                    seen.add(cand[s].index(act[e, s]))
        assert seen >= {0, 1, 2}, seen                              # every rank of a set is drawn somewhere


def test_the_explored_share_is_binomial():
    sc = xp.scenario("XA")
    trace = {}
    xp.np_playout_explore(sc["cfg"], sc["states"], sc["policies"], 16384, 5, 12, trace=trace)
    decisions = trace["n"] > 0
    N, k = int(decisions.sum()), int(trace["explored"][decisions].sum())
    print("decisions", N, "explored", k, "share", k / N, "bound", 5 * math.sqrt(0.25 * 0.75 / N))
    assert N > 1000 and not trace["explored"][~decisions].any()
    assert abs(k / N - 0.25) <= 5 * math.sqrt(0.25 * 0.75 / N)      # five standard deviations of the binomial share


def test_rows_depend_on_the_global_id_only():
    sc = xp.scenario("XA")
    cfg, states = sc["cfg"], sc["states"]
    whole = xp.np_explore_actions(cfg, states, ("safe_greedy", "wary_greedy", None), sc["eps"], 3)
    cut = 29
    lo = xp.np_explore_actions(dict(cfg, num_envs=cut), states[:cut], ("safe_greedy", "wary_greedy", None), sc["eps"], 3)
    hi = xp.np_explore_actions(dict(cfg, num_envs=len(states) - cut, env_id_base=cfg["env_id_base"] + cut), states[cut:],
                               ("safe_greedy", "wary_greedy", None), sc["eps"], 3)
    for k in range(3):
        assert np.array_equal(whole[k], np.concatenate([lo[k], hi[k]]))
    moved = xp.np_explore_actions(dict(cfg, env_id_base=cfg["env_id_base"] + 1), states, ("safe_greedy", "wary_greedy", None), sc["eps"], 3)
    assert not np.array_equal(whole[1], moved[1])                   # the same states under other ids draw differently
    other = xp.np_explore_actions(cfg, states, ("safe_greedy", "wary_greedy", None), sc["eps"], 4)
    assert not np.array_equal(whole[0], other[0]) and np.array_equal(whole[2], other[2])   # another salt changes some row, no candidate set


# ------------------------------------------------------------------------------------------ what the scenarios reach
def test_the_scenarios_cover_what_they_are_there_for():
    ref, tr = xp.reference("XA")
    ref0, _ = xp.reference_eps0("XA")
    differ = sum(not np.array_equal(a, b) for a, b in zip(ref["words"], ref0["words"]))
    assert 2 * differ >= len(ref["words"]), differ                  # at least half of the envs end in other words than at eps 0
    assert tr["explored"].any() and (tr["draws"] > 0).any()
    ref, tr = xp.reference("XB")
    assert (ref["end"] == pp.CAP).sum() >= 5 and not tr["explored"][:, :, 0].any() and tr["explored"][:, :, 1].any()
    ref, tr = xp.reference("XC")
    assert (ref["end"] == pp.DEAD).sum() >= 5 and np.array_equal(tr["explored"], (tr["n"] > 0).astype(np.uint8))
    ref, tr = xp.reference("XD")
    assert tr["explored"][:, :, 2].any() and ref["steps"].max() == 120        # an exploring `none` snake; some env plays all K steps
    ref, tr = xp.reference("XF")
    assert tr["explored"][:, :, 0].any() and ref["steps"].max() > 20          # an exploring hamiltonian snake
    ref, _ = xp.reference("XG_finished")
    assert ref["end"].tolist()[::2] == [pp.FINISHED] * 2 and ref["steps"][1] > 0
    ref, tr = xp.reference("XG_long")
    assert tr["explored"].any() and max(len(b) for st in xp.scenario("XG_long")["states"] for b in st["snakes"]) == 70
    sc, (ref, tr) = xp.scenario("X_forced"), xp.reference("X_forced")
    assert np.array_equal(ref["info"][:, [0, 2], 3], sc["first"][:, [0, 2]]) and np.array_equal(tr["explored"][0], tr["n"][0] > 0)   # drawn, and overruled
    drawn = xp.np_explore_actions(sc["cfg"], sc["states"], sc["policies"], sc["eps"], sc["salt"])[0]
    assert (drawn[:, [0, 2]] != sc["first"][:, [0, 2]]).any() and np.array_equal(ref["info"][:, 1, 3], drawn[:, 1])


def test_the_quiet_states_draw_nothing_at_eps_zero():
    sc = xp.scenario("quiet")
    tr = {}
    pp.np_playout(sc["cfg"], sc["states"], sc["policies"], sc["K"], trace=tr)
    assert not tr["draws"].any() and not tr["ate"].any()
    states, first = xp.quiet_forks()                               # ... and whichever first move snake 0 is forced to
    tr = {}
    res = pp.np_playout(sc["cfg"], states, sc["policies"], sc["K"], first, [0], trace=tr)
    assert not tr["draws"].any() and len(states) == 4 * len(sc["states"])
    assert (res["steps"] >= 1).all()


# ------------------------------------------------------------------------------------------ the Python methods
class _FakeLib:
    """Records the C calls of explore_actions_device / playout_device / playout_values_device."""

    def __init__(self):
        self.calls = []

    def msnake_playout(self, h, pol, *a):
        self.calls.append(("playout", h, list(pol)) + a)
        return 0

    def msnake_playout_explore(self, h, pol, eps, *a):
        self.calls.append(("playout_explore", h, list(pol), list(eps)) + a)
        return 0

    def msnake_explore_actions(self, h, pol, eps, *a):
        self.calls.append(("explore", h, list(pol), list(eps)) + a)
        return 0

    def msnake_copy_envs(self, *a):
        self.calls.append(("copy",) + a)
        return 0

    def msnake_state_words_max(self, h):
        return 99


def _bare_env(n=5, ns=3, dim=10, rules=0, h=1234):
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, h
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env.cfg = types.SimpleNamespace(dim=dim, rules=rules)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    env._pending, env._track_stale, env._scripted_out = None, False, None
    return env, lib


def test_explore_actions_device_passes_what_the_header_asks_for():
    env, lib = _bare_env()
    out = env.explore_actions_device("safe_greedy", 0.25)
    assert out.dtype == torch.int32 and tuple(out.shape) == (5, 3) and out is env._scripted_out
    assert lib.calls[-1] == ("explore", 1234, [1, 1, 1, 0], [16384, 16384, 16384, 0], 0, 0b111, out.data_ptr(), 3, None, 77)
    wide, flags = torch.zeros((5, 4), dtype=torch.int32), torch.zeros((5, 3), dtype=torch.uint8)
    got = env.explore_actions_device(("wary_greedy", None, "hamiltonian"), (0, 1, 0.5), salt=2 ** 64 - 1, snakes=[2, 0], out=wide, explored_out=flags)
    assert got[0] is wide and got[1] is flags
    assert lib.calls[-1] == ("explore", 1234, [3, 0, 2, 0], [0, 65536, 32768, 0], 2 ** 64 - 1, 0b101, wide.data_ptr(), 4, flags.data_ptr(), 77)
    env.explore_actions_device(None, np.float32(1.0) / 3)
    assert lib.calls[-1][3] == [round(float(np.float32(1.0) / 3) * 65536)] * 3 + [0]
    adv, alib = _bare_env(rules=2)
    adv.explore_actions_device("wary_greedy", 0.0)
    assert alib.calls[-1][2:5] == ([3, 3, 3, 0], [0, 0, 0, 0], 0)


def test_explore_actions_device_refuses_before_the_c_call():
    env, lib = _bare_env()
    for bad in (-0.01, 1.5, float("nan"), "0.5", None, True, (0.1, 0.2), (0.1, 0.2, 0.3, 0.4), (0.1, 2.0, 0.3), (0.1, "x", 0.3)):
        with pytest.raises(ValueError, match="explore"):
            env.explore_actions_device("safe_greedy", bad)
    for bad in (-1, 2 ** 64, 1.0, "7", True):
        with pytest.raises(ValueError, match="salt"):
            env.explore_actions_device("safe_greedy", 0.5, salt=bad)
    for bad in ("greedy", ("safe_greedy",) * 2, ("safe_greedy", "space_greedy", None)):
        with pytest.raises(ValueError, match="policies"):
            env.explore_actions_device(bad, 0.5)
    odd, _ = _bare_env(dim=9)
    with pytest.raises(ValueError, match="policies.*even"):
        odd.explore_actions_device("hamiltonian", 0.5)
    nw, _ = _bare_env(rules=1)
    with pytest.raises(ValueError, match="policies.*wary_greedy"):
        nw.explore_actions_device(("safe_greedy", "wary_greedy", None), 0.5)
    for bad in ([3], [-1], [0.5], []):
        with pytest.raises(ValueError, match="snake"):
            env.explore_actions_device("safe_greedy", 0.5, snakes=bad)
    for bad in (torch.zeros((5, 2), dtype=torch.int32), torch.zeros((5, 3), dtype=torch.int64), torch.zeros((4, 3), dtype=torch.int32),
                torch.zeros((5, 6), dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="out"):
            env.explore_actions_device("safe_greedy", 0.5, out=bad)
    with pytest.raises(ValueError, match="explored_out"):
        env.explore_actions_device("safe_greedy", 0.5, explored_out=torch.zeros((5, 4), dtype=torch.uint8))
    assert lib.calls == []


def test_playout_device_without_explore_calls_msnake_playout_unchanged():
    env, lib = _bare_env()
    res = env.playout_device(16)
    assert lib.calls[-1] == ("playout", 1234, [1, 1, 1, 0], 16, None, 0, 0, res.steps.data_ptr(), res.end.data_ptr(),
                             res.ret.data_ptr(), res.info.data_ptr(), None, 0, None, 77)
    res = env.playout_device(16, explore=None, salt=5)
    assert lib.calls[-1][0] == "playout" and len(lib.calls[-1]) == 15
    first = torch.zeros((5, 4), dtype=torch.int32)
    res = env.playout_device(8, ("wary_greedy", None, "safe_greedy"), first_actions=first, first_snakes=[1], end_state=True,
                             explore=(0.1, 1.0, 0.0), salt=9)
    assert lib.calls[-1] == ("playout_explore", 1234, [3, 0, 1, 0], [6554, 65536, 0, 0], 9, 8, first.data_ptr(), 4, 0b010,
                             res.steps.data_ptr(), res.end.data_ptr(), res.ret.data_ptr(), res.info.data_ptr(), res.words.data_ptr(), 99,
                             res.count.data_ptr(), 77)
    env.playout_device(8, explore=0.0)                              # eps 0 asked for by name still goes through the exploring entry
    assert lib.calls[-1][:5] == ("playout_explore", 1234, [1, 1, 1, 0], [0, 0, 0, 0], 0)
    n = len(lib.calls)
    for kw, match in ((dict(explore=1.01), "explore"), (dict(explore=(0.5, 0.5)), "explore"), (dict(explore=0.5, salt=-1), "salt"),
                      (dict(explore=0.5, salt=2 ** 64), "salt")):
        with pytest.raises(ValueError, match=match):
            env.playout_device(8, **kw)
    assert len(lib.calls) == n


def test_playout_values_device_passes_explore_and_salt_through():
    env, lib = _bare_env(n=3)
    scratch, slib = _bare_env(n=3 * 4 * 2, h=5678)
    env.playout_values_device(scratch, 16, snake=1, reps=2)
    assert [c[0] for c in slib.calls] == ["copy", "playout"]
    env.playout_values_device(scratch, 16, snake=1, reps=2, explore=(0, 0.25, 0.25), salt=3)
    _, index, first = env._playout_plan
    assert slib.calls[-2][:4] == ("copy", 5678, 1234, index.data_ptr())
    assert slib.calls[-1][:9] == ("playout_explore", 5678, [1, 1, 1, 0], [0, 16384, 16384, 0], 3, 16, first.data_ptr(), 3, 0b010)
    with pytest.raises(ValueError, match="explore"):
        env.playout_values_device(scratch, 16, snake=1, reps=2, explore=2)
    assert len(slib.calls) == 4 and lib.calls == []


# ------------------------------------------------------------------------------------------ the kernels' budget
def test_the_kernels_spill_nothing():
    table, _ = unit_resources("msnake_opponents")
    playout = {k: v for k, v in table.items() if "msnake_playout_kernel" in k}
    explore = {k: v for k, v in table.items() if "msnake_explore_kernel" in k}
    assert len(playout) == 1 and len(explore) == 1, (sorted(playout), sorted(explore))   # still ONE playout kernel, one explore kernel
    for name, r in sorted({**playout, **explore}.items()):
        print(name, "VGPRs", r["VGPRs"], "SGPRs", r["TotalSGPRs"])
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
