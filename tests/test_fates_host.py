"""The fate of every move, host side: tests/fates_play.py against the CPU oracle, exhaustively over every joint action of
the other snakes, on closed-loop play and on the hand-built states; the entry point is declared, exported and bound, and
wary_greedy is accepted as a policy name.  Nothing here needs a GPU.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import fates_play as fp
import msnake
import scripted_play as sp
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ 1. the guarantees on the oracle
@functools.lru_cache(maxsize=None)
def played_states(rules, dim, num_envs=8, steps=150, every=5):
    """Closed-loop play of the oracle under wary_greedy with a little noise (so that every bit turns up): the states in
    front of every `every`-th step, and those of the steps between as a second list."""
    cfg = sp.scenario(rules, dim, 3, "wary_greedy", steps, num_envs, seed=11, eps=0.15, max_steps=60)
    ora = sp.make_oracle(cfg)
    ora.reset()
    read, rs = sp._StateReader(ora), sp.policy_rng(cfg)
    picked, rest = [], []
    for t in range(steps):
        states = [read(e) for e in range(num_envs)]
        (picked if t % every == 0 else rest).extend(states)
        ora.step(fp.choose_actions(cfg, states, rs))
    return cfg, picked, rest


SEEN = {}


@pytest.mark.parametrize("rules,dim", [("adversarial", 5), ("adversarial", 6)])
def test_guarantees_hold_under_every_joint_action_of_the_others(rules, dim):
    """8 envs x 150 steps of closed-loop play; every state is stepped under all 5 x 25 joint actions per snake."""
    cfg, picked, rest = played_states(rules, dim)
    seen = SEEN.setdefault((rules, dim), {})
    n = fp.check_guarantees(cfg, picked + rest, seen)
    assert n >= 100_000, n
    for name, (on, off) in seen.items():
        assert on > 0 and off > 0, (name, on, off)      # every bit was seen set and clear


@pytest.mark.parametrize("rules", ["snake_env", "adversarial"])
def test_guarantees_hold_on_the_hand_built_states(rules):
    names, states, _ = fp.hand_states(rules)
    assert fp.check_guarantees(fp.hand_cfg(rules), states) > 0
    for grows in (False, True):
        assert fp.check_guarantees(sp.scenario(rules, 10, 3, "wary_greedy", 1, 1, 1), [fp.long_body_state(grows)]) > 0


# ------------------------------------------------------------------------------------------ 2. the hand-built states
@pytest.mark.parametrize("rules", ["snake_env", "adversarial"])
def test_hand_built_states_show_the_bits_they_were_built_for(rules):
    names, states, wants = fp.hand_states(rules)
    assert len(names) == (13 if rules == "adversarial" else 12)
    shown = {name: [False, False] for name in fp.BITS}
    for name, st, want in zip(names, states, wants):
        fate, by, eat, mask = fp.np_fates(st, fp.HAND_DIM, 3)
        for (s, a), (on, off) in want.items():
            assert fate[s, a] & on == on and fate[s, a] & off == 0, (name, s, a, int(fate[s, a]), on, off)
            for bit_name, bit in fp.BITS.items():
                shown[bit_name][0] |= bool(on & bit)
                shown[bit_name][1] |= bool(off & bit)
    assert all(on and off for on, off in shown.values()), shown


def test_hand_built_literals():
    table = dict(fp.HAND, **fp.HAND_ADVERSARIAL)
    fate, by, eat, mask = fp.np_fates(table["fruit_twice"][0], 6, 3)
    assert eat[0].tolist() == [2, 2, 0, 2, 0] and fate[0, 1] == fp.EATS            # action 3 is a refused reverse: it eats too
    fate, by, eat, mask = fp.np_fates(table["other_tail_pops"][0], 6, 3)
    assert fate[0, 1] == fp.TAIL and by[0, 1] == 0x20 and mask[0, 0] >> 1 & 1 and not mask[0, 1] >> 1 & 1
    fate, by, eat, mask = fp.np_fates(table["stacked_on_tail"][0], 6, 3)
    assert fate[0, 1] == fp.BODY | fp.TAIL and by[0, 1] == 0x20
    fate, by, eat, mask = fp.np_fates(table["standing"][0], 6, 3)
    assert by[0, 1] == 0x02 and by[1, 4] == 0x01 and fate[1, 0] == 0
    assert fate[2].tolist() == [0, fp.WALL, fp.WALL, 0, 0]                         # the snake at rest in the corner (5, 5)
    fate, by, eat, mask = fp.np_fates(table["dead_among_live"][0], 6, 3)
    assert not fate[1].any() and not by[1].any() and mask[1].tolist() == [0, 0]
    assert fp.wary_greedy(table["dead_among_live"][0], 6, 3)[1] == 0
    fate, by, eat, mask = fp.np_fates(fp.long_body_state(False), 10, 3)
    assert fate[1, 2] == fp.TAIL and by[1, 2] == 0x10
    assert fp.np_fates(fp.long_body_state(True), 10, 3)[0][1, 2] == fp.BODY
    # the own tail: open to wary_greedy, closed to safe_greedy
    st = fp.state([fp._SQUARE, [], []], [(0, -1), (0, 0), (0, 0)], [(3, 2)] * 3, grow_to=[4, 3, 3])
    assert fp.np_fates(st, 6, 3)[0][0, 1] == fp.SELF | fp.EATS                     # the fruit under the tail keeps the tail
    st = fp.state([fp._SQUARE, [], []], [(0, -1), (0, 0), (0, 0)], [(4, 2)] * 3, grow_to=[4, 3, 3])
    assert fp.wary_greedy(st, 6, 3)[0] == 1 and sp.safe_greedy(st, 6, 3, None)[0] != 1


def test_new_world_raises():
    st = fp.HAND["standing"][0]
    with pytest.raises(ValueError, match="new_world"):
        fp.np_fates(st, 6, 3, "new_world")


# ------------------------------------------------------------------------------------------ 3. the C entry point and the names
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_fate_actions\(msnake_handle h, uint32_t snake_mask, int32_t\* actions_dev, int32_t action_stride,\s*"
           r"uint8_t\* fate_dev, uint8_t\* by_dev, uint8_t\* eat_dev, uint8_t\* mask_dev, void\* stream\);")
    assert re.search(sig, text)
    C = msnake._capi
    for name, value in fp.BITS.items():
        m = re.search(rf"#define MSNAKE_FATE_{name}\s+(\d+)\b", text)
        assert m and int(m.group(1)) == value == getattr(C, f"FATE_{name}"), name
    assert (fp.WALL, fp.SELF, fp.BODY, fp.HEAD_ON, fp.TAIL, fp.EATS) == (1, 2, 4, 8, 16, 32)
    assert re.search(r"#define MSNAKE_FATE_CERTAIN \(MSNAKE_FATE_WALL \| MSNAKE_FATE_SELF \| MSNAKE_FATE_BODY\)", text)
    assert re.search(r"#define MSNAKE_FATE_RISK \(MSNAKE_FATE_HEAD_ON \| MSNAKE_FATE_TAIL\)", text)
    assert (C.FATE_CERTAIN, C.FATE_RISK) == (fp.CERTAIN, fp.RISK) == (7, 24)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_fate_actions" in C.SYMBOLS
    lib = C.load()
    assert lib.msnake_fate_actions is not None and lib.msnake_abi_version() == 3
    restype, argtypes = C.PROTOTYPES["msnake_fate_actions"]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int and argtypes == [vp, ctypes.c_uint32, vp, ctypes.c_int32, vp, vp, vp, vp, vp]
    assert lib.msnake_fate_actions(None, 1, None, 3, None, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    assert callable(msnake.MultiSnakeVecEnv.move_fates_device) and callable(msnake.MultiSnakeVecEnv.fate_masks_device)
    assert msnake.MoveFates._fields == ("fate", "by", "eat", "mask")


def test_fates_kernels_do_not_spill():
    """Every instantiation of msnake_fates_kernel<ACT, FATE, BY, EAT, MASK> spills no register, uses no scratch and no
    LDS, and stays within 64 VGPRs (8 waves per SIMD)."""
    from kernel_resources import unit_resources
    res, _ = unit_resources("msnake_opponents")
    seen = set()
    for name, rr in res.items():
        m = re.match(r"_ZN6msnake19msnake_fates_kernelILb([01])ELb([01])ELb([01])ELb([01])ELb([01])EEE", name)
        if not m:
            continue
        seen.add(m.groups())
        assert rr["SGPRs Spill"] == 0 and rr["VGPRs Spill"] == 0 and rr["ScratchSize [bytes/lane]"] == 0, (m.groups(), rr)
        assert rr["LDS Size [bytes/block]"] == 0 and rr["VGPRs"] <= 64, (m.groups(), rr)
    assert len(seen) == 31 and ("0",) * 5 not in seen, sorted(seen)     # every combination but `nothing to write`


def test_the_names():
    C = msnake._capi
    assert C.WARY_POLICY == "wary_greedy"
    assert C.SCRIPTED_NAMES == C.SCRIPTED_PLAYER_NAMES + ("wary_greedy",)
    assert selfplay.SCRIPTED_NAMES is C.SCRIPTED_NAMES
    for tool in ("train_selfplay.py", "eval_vs_scripted.py"):
        assert "msnake._capi.WARY_POLICY" in open(os.path.join(ROOT, "tools", tool)).read()


class _FakeEnv:
    def __init__(self, n=8, n_snakes=3):
        self.num_envs, self.n_snakes, self.device = n, n_snakes, torch.device("cpu")
        self.scripted_calls = []

    def scripted_actions_device(self, policy, snakes=None, out=None):
        self.scripted_calls.append((policy, tuple(snakes)))
        for s in snakes:
            out[:, s] = {"safe_greedy": 2, "wary_greedy": 4}[policy]
        return out


def test_selfplay_accepts_wary_greedy():
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "wary_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "safe_greedy", 2, columns=team)
    selfplay.refresh_scripted([o1, o2])
    assert sorted(env.scripted_calls) == [("safe_greedy", (2,)), ("wary_greedy", (1,))]
    assert o1.step()[0].tolist() == [4] * 8 and o2.step()[0].tolist() == [2] * 8
    with pytest.raises(ValueError, match="'timed_greedy', 'wary_greedy'"):
        selfplay.ScriptedOpponent(env, "wary", 1)


class _FakeLib:
    def __init__(self):
        self.calls = []

    def msnake_fate_actions(self, *a):
        self.calls.append(a)
        return 0


def _bare_env(n=5, ns=3):
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env._fates_fn = lib.msnake_fate_actions
    env._scripted_out = torch.zeros((n, ns), dtype=torch.int32)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    return env, lib


def test_vec_env_dispatches_wary_greedy_and_checks_its_outputs():
    env, lib = _bare_env()
    out = torch.zeros((5, 4), dtype=torch.int32)
    assert env.scripted_actions_device("wary_greedy", snakes=[2, 0], out=out) is out
    assert lib.calls[-1] == (1234, 0b101, out.data_ptr(), 4, None, None, None, None, 77)
    fate, mask = torch.zeros((5, 3, 5), dtype=torch.uint8), torch.zeros((5, 3, 2), dtype=torch.uint8)
    got = env.scripted_actions_device("wary_greedy", out=out, fates_out=msnake.MoveFates(fate, None, None, mask))
    assert got[0] is out and got[1].fate is fate and got[1].by is None and got[1].mask is mask
    assert lib.calls[-1] == (1234, 0b111, out.data_ptr(), 4, fate.data_ptr(), None, None, mask.data_ptr(), 77)
    res = env.move_fates_device(out=msnake.MoveFates(None, fate, None, None))
    assert res.by is fate and lib.calls[-1] == (1234, 0, None, 0, None, fate.data_ptr(), None, None, 77)
    assert env.fate_masks_device(out=mask) is mask
    assert lib.calls[-1] == (1234, 0, None, 0, None, None, None, mask.data_ptr(), 77)
    n_calls = len(lib.calls)
    with pytest.raises(ValueError, match="writes no safe-move mask"):
        env.scripted_actions_device("wary_greedy", out=out, safe_out=torch.zeros((5, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="fates_out is written by policy 'wary_greedy' only"):
        env.scripted_actions_device("safe_greedy", out=out, fates_out=msnake.MoveFates(fate, None, None, None))
    with pytest.raises(ValueError, match="mask_out"):
        env.fate_masks_device(out=fate)
    with pytest.raises(ValueError, match="fate_out"):
        env.move_fates_device(out=msnake.MoveFates(mask, None, None, None))
    with pytest.raises(ValueError, match="nothing to write"):
        env.move_fates_device(out=msnake.MoveFates(None, None, None, None))
    with pytest.raises(ValueError, match="policy must be 'safe_greedy', 'hamiltonian' or None"):
        env.scripted_actions_device("wary")
    assert len(lib.calls) == n_calls
