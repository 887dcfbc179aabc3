"""CPU-side checks of the scripted playouts (msnake_playout, MultiSnakeVecEnv.playout_device / playout_values_device):
the entry point is declared, exported and bound as declared; what the scenarios of tests/playout_play.py reach, from the
reference's own outputs; properties of the reference np_playout; the Python methods against a recording fake library
(argument order, strides, masks, every refusal before the C call); the register budget of the kernels.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import msnake
import playout_play as pp
from kernel_resources import unit_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = msnake._capi


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_playout\(msnake_handle h, const int32_t policies\[MSNAKE_MAX_SNAKES\], int32_t n_steps,\s*"
           r"const int32_t\* first_dev,\s*int32_t first_stride, uint32_t first_mask,\s*int32_t\* steps_dev, uint8_t\* end_dev,\s*"
           r"float\* ret_dev,\s*int32_t\* info_dev,\s*int32_t\* words_dev, int32_t words_stride, int32_t\* count_dev, void\* stream\);")
    assert re.search(sig, text)
    for name, val in (("MSNAKE_POLICY_WARY_GREEDY", 3), ("MSNAKE_PLAYOUT_MAX_STEPS", 4096), ("MSNAKE_PLAYOUT_HORIZON", 0),
                      ("MSNAKE_PLAYOUT_DEAD", 1), ("MSNAKE_PLAYOUT_CAP", 2), ("MSNAKE_PLAYOUT_FINISHED", 3)):
        assert re.search(rf"#define {name}\s+{val}\b", text), name
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "snake_multiple_test.py:97-197" in text
    assert "msnake_playout" in C.SYMBOLS
    assert C.PLAYOUT_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2, "wary_greedy": 3} == pp.POLICY_ID
    assert C.SCRIPTED_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2}   # msnake_scripted_actions keeps its ids
    assert (C.PLAYOUT_HORIZON, C.PLAYOUT_DEAD, C.PLAYOUT_CAP, C.PLAYOUT_FINISHED) == (pp.HORIZON, pp.DEAD, pp.CAP, pp.FINISHED)
    assert C.PLAYOUT_MAX_STEPS == pp.MAX_STEPS == 4096
    lib = C.load()
    assert lib.msnake_playout is not None and lib.msnake_abi_version() == 3


def test_the_binding_has_the_declared_signature():
    restype, argtypes = C.PROTOTYPES["msnake_playout"]
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert restype is ctypes.c_int
    assert argtypes == [vp, ctypes.POINTER(i32), i32, vp, i32, ctypes.c_uint32, vp, vp, vp, vp, vp, i32, vp, vp]
    fn = C.load().msnake_playout
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_null_handle_is_refused_first():
    lib = C.load()
    assert lib.msnake_playout(None, None, 0, None, 0, 0xFF, None, None, None, None, None, 0, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ what the scenarios reach
def test_the_scenarios_cover_what_they_are_there_for():
    cov = pp.coverage(("A", "B", "C"))
    assert all(n >= 5 for n in cov["ends"].values()), cov          # every end code, at least 5 envs each
    assert cov["other_deaths"] >= 10 and cov["two_eaters"] >= 10, cov
    res, tr = pp.reference("A")
    assert np.bincount(res["end"], minlength=4).tolist() == [17, 50, 0, 0]
    assert res["steps"].min() == 1 and res["steps"].max() == 60
    # 65 of A's 67 envs draw; the other two end within two steps, before anybody eats
    assert int((tr["draws"] > 0).sum()) == 65 and not tr["ate"][:, tr["draws"] == 0].any() and res["steps"][tr["draws"] == 0].max() <= 2
    res, _ = pp.reference("B")
    assert np.bincount(res["end"], minlength=4).tolist() == [0, 20, 47, 0]
    res, _ = pp.reference("C")
    assert (res["end"] == pp.DEAD).all() and res["steps"].max() < 40
    res, _ = pp.reference("E")
    assert (res["end"] == pp.DEAD).all() and res["steps"].max() == 196
    sc = pp.scenario("F")
    assert all(v == [0, 0] for st in sc["states"] for v in st["vels"])   # straight from reset: standing snakes
    res, _ = pp.reference("G_finished")
    assert res["end"].tolist()[::2] == [pp.FINISHED] * 2 and res["steps"].tolist()[::2] == [0, 0] and res["steps"][1] > 0
    assert not res["ret"][::2].any() and not res["info"][::2].any()
    res, _ = pp.reference("G_long")
    assert res["steps"].min() >= 2 and max(len(b) for st in pp.scenario("G_long")["states"] for b in st["snakes"]) == 70
    res, _ = pp.reference("Hmax")
    assert len(res["steps"]) == 8 and pp.scenario("Hmax")["K"] == 4096


def test_the_edge_cases_end_in_their_recorded_states():
    cases = pp.edge_cases()
    assert len(cases) >= 30 and {c[0].split("[")[0] for c in cases} >= {"S_oob_alias_respawn", "S_respawn_sees_later_unmoved",
                                                                         "S_invalid_action", "S_no_free_cell", "S_step_cap"}
    for label, cfg, st, actions, want in cases:
        res = pp.np_playout(cfg, [st], None, 1, first=[actions])
        got = pp.words_to_state(res["words"][0])
        for key in ("snakes", "fruits", "grow_to", "t", "ctr"):
            assert got[key] == want[key], (label, key)
        assert [list(v) for v in got["vels"]] == [list(v) for v in want["vels"]], label
        assert res["info"][0, :, 3].tolist() == actions, label


# ------------------------------------------------------------------------------------------ properties of np_playout
@pytest.mark.parametrize("name", ["A", "B", "D"])
def test_returns_follow_the_step_rewards_and_the_fruits(name):
    res, tr = pp.reference(name)
    assert np.array_equal(res["ret"][:, 0], tr["rew"].sum(axis=0))        # column 0: the oracle's own rewards, summed
    died = res["info"][:, :, 2] > 0
    want = res["info"][:, :, 0] - died
    ate_dying = (tr["ate"] * tr["died"]).sum(axis=0)                       # a death step that also ate counts the fruit, not the reward
    assert np.array_equal(res["ret"], (want - ate_dying).astype(np.float32))
    assert (res["info"][:, :, 1] <= res["steps"][:, None]).all()
    assert np.array_equal(died[:, 0], res["end"] == pp.DEAD)


def test_a_playout_continues_from_its_end_words():
    sc = pp.scenario("A")
    cfg, states, a, b = dict(sc["cfg"], num_envs=24), sc["states"][:24], 7, 13
    whole = pp.np_playout(cfg, states, sc["policies"], a + b)
    head = pp.np_playout(cfg, states, sc["policies"], a)
    tail = pp.np_playout(cfg, [pp.words_to_state(w) for w in head["words"]], sc["policies"], b)
    assert (tail["end"][head["end"] != pp.HORIZON] == pp.FINISHED).all()
    for e in range(24):
        assert np.array_equal(whole["words"][e], tail["words"][e]), e
    assert np.array_equal(whole["steps"], head["steps"] + tail["steps"])
    assert np.array_equal(whole["ret"], head["ret"] + tail["ret"])
    assert np.array_equal(whole["end"], np.where(head["end"] != pp.HORIZON, head["end"], tail["end"]))


# ------------------------------------------------------------------------------------------ the Python methods
class _FakeLib:
    """Records the C calls of playout_device / playout_values_device."""

    def __init__(self):
        self.calls = []

    def msnake_playout(self, h, pol, *a):
        self.calls.append(("playout", h, list(pol)) + a)
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
    env._pending, env._track_stale = None, False
    return env, lib


def test_playout_device_passes_what_the_header_asks_for():
    env, lib = _bare_env()
    res = env.playout_device(16)
    assert isinstance(res, msnake.Playout) and res.words is None and res.count is None
    assert (res.steps.dtype, res.end.dtype, res.ret.dtype, res.info.dtype) == (torch.int32, torch.uint8, torch.float32, torch.int32)
    assert tuple(res.ret.shape) == (5, 3) and tuple(res.info.shape) == (5, 3, 4)
    assert lib.calls[-1] == ("playout", 1234, [1, 1, 1, 0], 16, None, 0, 0, res.steps.data_ptr(), res.end.data_ptr(),
                             res.ret.data_ptr(), res.info.data_ptr(), None, 0, None, 77)
    res = env.playout_device(4096, ("wary_greedy", None, "hamiltonian"), end_state=True)
    assert tuple(res.words.shape) == (5, 99) and tuple(res.count.shape) == (5,)
    assert lib.calls[-1][2:4] == ([3, 0, 2, 0], 4096) and lib.calls[-1][11:14] == (res.words.data_ptr(), 99, res.count.data_ptr())
    first = torch.zeros((5, 4), dtype=torch.int32)
    env.playout_device(1, None, first_actions=first)
    assert lib.calls[-1][2:7] == ([0, 0, 0, 0], 1, first.data_ptr(), 4, 0b111)
    env.playout_device(1, "safe_greedy", first_actions=first, first_snakes=[2, 0])
    assert lib.calls[-1][4:7] == (first.data_ptr(), 4, 0b101)
    env.playout_device(1, "safe_greedy", first_actions=first, first_snakes=[])
    assert lib.calls[-1][4:7] == (None, 0, 0)
    # caller-supplied outputs: any subset, the words of any stride
    ret, words = torch.zeros((5, 3)), torch.zeros((5, 40), dtype=torch.int32)
    got = env.playout_device(3, out=(None, None, ret, None, words, None))
    assert got.ret is ret and got.words is words and got.steps is None
    assert lib.calls[-1][7:15] == (None, None, ret.data_ptr(), None, words.data_ptr(), 40, None, 77)


def test_playout_device_refuses_before_the_c_call():
    env, lib = _bare_env()
    first = torch.zeros((5, 3), dtype=torch.int32)
    for bad in (0, 4097, -1, 2.5):
        with pytest.raises(ValueError, match="n_steps"):
            env.playout_device(bad)
    for bad in ("greedy", ("safe_greedy",) * 2, ("safe_greedy", "space_greedy", None)):
        with pytest.raises(ValueError, match="policies"):
            env.playout_device(4, bad)
    odd, _ = _bare_env(dim=9)
    with pytest.raises(ValueError, match="policies.*even"):
        odd.playout_device(4, "hamiltonian")
    other, _ = _bare_env(rules=2)
    with pytest.raises(ValueError, match="snake_env"):
        other.playout_device(4)
    with pytest.raises(ValueError, match="first_snakes"):
        env.playout_device(4, first_snakes=[0])
    with pytest.raises(ValueError, match="first_snakes"):
        env.playout_device(4, first_actions=first, first_snakes=[3])
    for bad in (first[:, :2], first.to(torch.int64), first[:4], torch.zeros((5, 6), dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="first_actions"):
            env.playout_device(4, first_actions=bad)
    with pytest.raises(ValueError, match="six entries"):
        env.playout_device(4, out=(None,) * 4)
    with pytest.raises(ValueError, match="nothing to write"):
        env.playout_device(4, out=(None,) * 6)
    with pytest.raises(ValueError, match="out.ret"):
        env.playout_device(4, out=(None, None, torch.zeros((5, 4)), None, None, None))
    with pytest.raises(ValueError, match="out.words"):
        env.playout_device(4, out=(None, None, None, None, torch.zeros((4, 40), dtype=torch.int32), None))
    assert lib.calls == []


def test_playout_values_device_is_its_composition():
    env, lib = _bare_env(n=3)
    scratch, slib = _bare_env(n=3 * 4 * 2, h=5678)
    scratch.playout_device = types.MethodType(msnake.MultiSnakeVecEnv.playout_device, scratch)
    value, survive = env.playout_values_device(scratch, 16, snake=1, reps=2, policies="wary_greedy")
    assert tuple(value.shape) == tuple(survive.shape) == (3, 4) and value.dtype == survive.dtype == torch.float32
    copy, play = slib.calls
    assert copy[:3] == ("copy", 5678, 1234)
    _, index, first = env._playout_plan
    assert copy[3] == index.data_ptr() and index.tolist() == [e for e in range(3) for _ in range(8)]
    assert first[:, 1].tolist() == [m + 1 for _ in range(3) for m in range(4) for _ in range(2)] and not first[:, [0, 2]].any()
    assert play[:7] == ("playout", 5678, [3, 3, 3, 0], 16, first.data_ptr(), 3, 0b010)
    assert lib.calls == []                                        # the env itself is only a source
    for kw, match in ((dict(snake=3), "snake"), (dict(reps=0), "reps")):
        with pytest.raises(ValueError, match=match):
            env.playout_values_device(scratch, 16, **kw)
    with pytest.raises(ValueError, match="num_envs"):
        env.playout_values_device(scratch, 16, reps=3)
    with pytest.raises(TypeError):
        env.playout_values_device(object(), 16)
    assert len(slib.calls) == 2


# ------------------------------------------------------------------------------------------ the kernels' budget
def test_the_playout_kernels_spill_nothing():
    table, _ = unit_resources("msnake_opponents")
    mine = {k: v for k, v in table.items() if "msnake_playout_kernel" in k}
    assert len(mine) == 1, sorted(mine)          # one kernel for every set of policies
    for name, r in sorted(mine.items()):
        print(name, "VGPRs", r["VGPRs"], "SGPRs", r["TotalSGPRs"])
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
