"""CPU-side checks of the cell lifetimes, the timed reach and the opponent timed_greedy (msnake_timed_actions,
MultiSnakeVecEnv.scripted_actions_device("timed_greedy"), timed_reach_device, cell_lifetimes_device,
selfplay.ScriptedOpponent): the entry point is declared, exported and refuses a NULL handle before it touches the GPU;
the names; dispatch by name on fake envs; the helper tests/timed_play.py on the properties of the definitions and on
hand-built timing cases with closed-form answers; the lifetime formula against the oracle's play; survival against
space_greedy on the oracle alone.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import msnake
import scripted_play as sp
import space_play as spp
import timed_play as tp
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEVER = tp.NEVER
BIG = tp.BIG


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_timed_actions\(msnake_handle h, uint32_t snake_mask, int32_t\* actions_dev, int32_t action_stride,\s*"
           r"uint8_t\* safe_dev, uint16_t\* reach_dev, uint16_t\* life_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_LIFE_NEVER 0xFFFFu\b", text) and NEVER == 0xFFFF
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_timed_actions" in msnake._capi.SYMBOLS
    assert msnake._capi.SCRIPTED_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2}   # no new policy id
    lib = msnake._capi.load()
    assert lib.msnake_timed_actions is not None and lib.msnake_abi_version() == 3


def test_the_binding_has_the_declared_signature():
    import ctypes
    restype, argtypes = msnake._capi.PROTOTYPES["msnake_timed_actions"]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int
    assert argtypes == [vp, ctypes.c_uint32, vp, ctypes.c_int32, vp, vp, vp, vp]
    fn = msnake._capi.load().msnake_timed_actions
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_timed_actions(None, 1, None, 3, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


def test_the_names():
    C = msnake._capi
    assert C.TIMED_POLICY == "timed_greedy"
    assert C.SCRIPTED_PLAYER_NAMES == C.SCRIPTED_OPPONENT_NAMES + ("timed_greedy",)
    assert C.SCRIPTED_PLAYER_NAMES == ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy", "path_greedy", "timed_greedy")
    # the older tuples are as they were
    assert C.SCRIPTED_POLICY_NAMES == ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy")
    assert C.SCRIPTED_OPPONENT_NAMES == C.SCRIPTED_POLICY_NAMES + ("path_greedy",)
    assert selfplay.SCRIPTED_POLICIES is C.SCRIPTED_POLICY_NAMES and selfplay.SCRIPTED_OPPONENTS is C.SCRIPTED_OPPONENT_NAMES
    assert selfplay.SCRIPTED_PLAYERS is C.SCRIPTED_PLAYER_NAMES
    assert msnake.vec_env.COUNT_POLICIES["timed_greedy"] == ("_timed_fn", "msnake_timed_actions", ("reach_out", "life_out"))


def test_the_tools_offer_the_new_opponent():
    for tool in ("train_selfplay.py", "eval_vs_scripted.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "msnake._capi.SCRIPTED_OPPONENT_NAMES + (msnake._capi.TIMED_POLICY,)" in text
        assert "SCRIPTED_POLICY_NAMES" not in text


# ------------------------------------------------------------------------------------------ dispatch by name
class _FakeEnv:
    """CPU stand-in with the device-side surface ScriptedOpponent uses (as in test_path_host.py): its
    scripted_actions_device has NO reach_out / life_out keyword, like the fake envs of the older host tests."""

    def __init__(self, n=8, n_snakes=3):
        self.num_envs, self.n_snakes, self.device = n, n_snakes, torch.device("cpu")
        self.scripted_calls = []

    def scripted_actions_device(self, policy, snakes=None, out=None, safe_out=None, space_out=None):
        self.scripted_calls.append((policy, tuple(snakes)))
        if out is None:
            out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32)
        for s in snakes:
            out[:, s] = {"safe_greedy": 2, "space_greedy": 4, "timed_greedy": 3}[policy]
        return out


def test_selfplay_dispatches_timed_greedy_by_name():
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "timed_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "safe_greedy", 2, columns=team)
    selfplay.refresh_scripted([o1, o2])
    assert sorted(env.scripted_calls) == [("safe_greedy", (2,)), ("timed_greedy", (1,))]
    assert o1.step()[0].tolist() == [3] * 8 and o2.step()[0].tolist() == [2] * 8
    assert selfplay.ScriptedOpponent(env, "timed_greedy", 2).step()[0].tolist() == [3] * 8   # a lone opponent asks itself
    with pytest.raises(ValueError, match="'path_greedy', 'timed_greedy'"):                    # the refusal lists the new name
        selfplay.ScriptedOpponent(env, "timed", 1)


class _FakeLib:
    """Records the C calls of MultiSnakeVecEnv's scripted entry points."""

    def __init__(self):
        self.calls = []

    def _rec(name):
        def fn(self, *a):
            self.calls.append((name,) + a)
            return 0
        return fn

    msnake_timed_actions, msnake_path_actions = _rec("timed"), _rec("path")
    msnake_space_actions, msnake_scripted_actions = _rec("space"), _rec("scripted")


def _bare_env(n=5, ns=3, dim=7):
    """A MultiSnakeVecEnv with only what scripted_actions_device / timed_reach_device / cell_lifetimes_device touch."""
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env.cfg = type("Cfg", (), {"dim": dim})()
    env._scripted_fn, env._space_fn, env._path_fn = lib.msnake_scripted_actions, lib.msnake_space_actions, lib.msnake_path_actions
    env._timed_fn = lib.msnake_timed_actions
    env._scripted_out = torch.zeros((n, ns), dtype=torch.int32)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    return env, lib


def test_vec_env_dispatches_by_name_and_checks_reach_out_and_life_out():
    env, lib = _bare_env()
    out = torch.zeros((5, 4), dtype=torch.int32)
    safe = torch.zeros((5, 3), dtype=torch.uint8)
    reach = torch.zeros((5, 3, 4), dtype=torch.uint16)
    life = torch.zeros((5, 7, 7), dtype=torch.uint16)
    space = torch.zeros((5, 3, 4), dtype=torch.uint16)
    assert env.scripted_actions_device("timed_greedy", snakes=[2, 0], out=out) is out
    assert lib.calls[-1] == ("timed", 1234, 0b101, out.data_ptr(), 4, None, None, None, 77)
    got = env.scripted_actions_device("timed_greedy", out=out, safe_out=safe, reach_out=reach, life_out=life)
    assert len(got) == 4 and got[0] is out and got[1] is safe and got[2] is reach and got[3] is life   # the return order
    assert lib.calls[-1] == ("timed", 1234, 0b111, out.data_ptr(), 4, safe.data_ptr(), reach.data_ptr(), life.data_ptr(), 77)
    got = env.scripted_actions_device("timed_greedy", life_out=life)
    assert len(got) == 2 and got[0] is env._scripted_out and got[1] is life
    assert lib.calls[-1] == ("timed", 1234, 0b111, env._scripted_out.data_ptr(), 3, None, None, life.data_ptr(), 77)
    got = env.scripted_actions_device("timed_greedy", out=out, reach_out=reach)
    assert len(got) == 2 and got[1] is reach and lib.calls[-1][6:8] == (reach.data_ptr(), None)
    # each output alone: no action, no mask, not the other one
    assert env.timed_reach_device(out=reach) is reach
    assert lib.calls[-1] == ("timed", 1234, 0, None, 0, None, reach.data_ptr(), None, 77)
    assert env.cell_lifetimes_device(out=life) is life
    assert lib.calls[-1] == ("timed", 1234, 0, None, 0, None, None, life.data_ptr(), 77)
    # the siblings are called as before -- on an env that has no _timed_fn at all
    del env._timed_fn
    env.scripted_actions_device("space_greedy", out=out, space_out=space)
    assert lib.calls[-1] == ("space", 1234, 0b111, out.data_ptr(), 4, None, space.data_ptr(), 77)
    env.scripted_actions_device("path_greedy", out=out, path_out=space, field_out=life)
    assert lib.calls[-1] == ("path", 1234, 0b111, out.data_ptr(), 4, None, space.data_ptr(), life.data_ptr(), 77)
    env.scripted_actions_device("safe_greedy", out=out)
    assert lib.calls[-1][:4] == ("scripted", 1234, 1, 0b111)
    env._timed_fn = lib.msnake_timed_actions
    n_calls = len(lib.calls)
    # reach_out and life_out belong to timed_greedy alone; the refusal names the keyword
    for pol in ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy", "path_greedy", None):
        with pytest.raises(ValueError, match="reach_out is written by policy 'timed_greedy' only"):
            env.scripted_actions_device(pol, out=out, reach_out=reach)
        with pytest.raises(ValueError, match="life_out is written by policy 'timed_greedy' only"):
            env.scripted_actions_device(pol, out=out, life_out=life)
    with pytest.raises(ValueError, match="space_out is written by policy 'space_greedy' only"):
        env.scripted_actions_device("timed_greedy", out=out, space_out=space)
    with pytest.raises(ValueError, match="field_out is written by policy 'path_greedy' only"):
        env.scripted_actions_device("timed_greedy", out=out, field_out=life)
    # one shape and type each
    for bad in (torch.zeros((5, 3, 4), dtype=torch.int16), torch.zeros((5, 3), dtype=torch.uint16),
                torch.zeros((5, 7, 7), dtype=torch.uint16), torch.zeros((5, 3, 8), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="reach_out"):
            env.scripted_actions_device("timed_greedy", out=out, reach_out=bad)
        with pytest.raises(ValueError, match="reach_out"):
            env.timed_reach_device(out=bad)
    for bad in (torch.zeros((5, 7, 7), dtype=torch.int16), torch.zeros((5, 3, 4), dtype=torch.uint16),
                torch.zeros((5, 7, 6), dtype=torch.uint16), torch.zeros((5, 7, 14), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="life_out"):
            env.scripted_actions_device("timed_greedy", out=out, life_out=bad)
        with pytest.raises(ValueError, match="life_out"):
            env.cell_lifetimes_device(out=bad)
    with pytest.raises(ValueError, match="policy must be 'safe_greedy', 'hamiltonian' or None"):
        env.scripted_actions_device("timed")                       # the text for unknown names is the one it was
    with pytest.raises(ValueError):
        env.scripted_actions_device("timed_greedy", snakes=[3])
    assert len(lib.calls) == n_calls                                 # every refusal came before the C call


# ------------------------------------------------------------------------------------------ the definitions on random boards
def _st(snakes, fruits, grow_to=None):
    n = len(snakes)
    return {"t": 0, "ctr": 0, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n,
            "grow_to": list(grow_to) if grow_to is not None else [max(len(b), 1) for b in snakes],
            "alive": [True] * n, "in_dead": [False] * n}


def _random_state(rng, dim, ns, density):
    """Random bodies (not connected: the helper does not care) covering about `density` of the board, with stacked
    duplicates, grow_to above, at and below the length, random fruits."""
    cells = [(x, y) for x in range(dim) for y in range(dim)]
    rng.shuffle(cells)
    k = int(density * dim * dim)
    parts = np.array_split(np.arange(k), ns)
    snakes = [[cells[i] for i in p] for p in parts]
    for b in snakes:
        if len(b) > 3 and rng.random() < 0.7:
            b[int(rng.integers(1, len(b)))] = b[0]                  # a piece stacked on the head: the head's lifetime wins
            b[len(b) // 2] = b[-1]                                  # one stacked on the tail: the older piece's lifetime wins
    grow = [max(0, len(b) + int(rng.integers(-4, 5))) for b in snakes]
    fruits = [tuple(int(v) for v in rng.integers(-1, dim + 1, 2)) for _ in range(int(rng.integers(0, 6)))]
    return _st(snakes, fruits, grow)


BOARDS = ((6, 2, 0.3), (10, 3, 0.5), (19, 3, 0.4), (33, 4, 0.55))


def test_definition_properties_on_random_boards():
    rng = np.random.default_rng(2)
    above = below = stacked = strictly_more = 0
    for dim, ns, density in BOARDS:
        for _ in range(6):
            st = _random_state(rng, dim, ns, density)
            above += sum(g > len(b) for g, b in zip(st["grow_to"], st["snakes"]))
            below += sum(g < len(b) for g, b in zip(st["grow_to"], st["snakes"]))
            stacked += sum(len({tuple(c) for c in b}) < len(b) for b in st["snakes"])
            occ = spp.occupancy(st, dim)
            life = tp.np_life(st, dim)
            assert ((life > 0) == occ).all() and life.max() <= tp.LIFE_CAP          # Life > 0 <=> occupancy
            for s, b in enumerate(st["snakes"]):                                   # the head's lifetime is the snake's largest
                assert life[tuple(b[0])] >= max(len(b), st["grow_to"][s])
            reach = tp.np_timed(st, dim, ns, life)
            for s, b in enumerate(st["snakes"]):                                   # the fast fill counts what the literal one takes
                for a, (d0, d1) in tp.DIRS.items():
                    t = (b[0][0] + d0, b[0][1] + d1)
                    if 0 <= t[0] < dim and 0 <= t[1] < dim and not occ[t]:
                        assert len(tp.timed_fill(life, dim, t)) == reach[s, a - 1], (dim, s, a)
            space = spp.np_space(st, dim, ns)
            mask = sp.np_safe_mask(st, dim, ns)
            is_open = (mask[:, None] >> np.arange(1, 5)) & 1 == 1
            assert (reach >= space).all()                                          # reach >= space, entry for entry
            assert ((reach == 0) == ~is_open).all()                                # reach == 0 <=> the move is not open
            assert reach.max() <= dim * dim
            strictly_more += int((reach > space).sum())
    assert above >= 10 and below >= 10 and stacked >= 20 and strictly_more >= 50, (above, below, stacked, strictly_more)


def test_the_lone_one_cell_snake_reaches_the_whole_board():
    for dim in (2, 3, 6, 19):
        for head in ((0, 0), (dim - 1, 0), (dim // 2, dim // 2), (0, dim - 1)):
            st = _st([[head]], [(0, 0)])
            reach = tp.np_timed(st, dim, 1)[0]
            for a, (d0, d1) in tp.DIRS.items():
                t = (head[0] + d0, head[1] + d1)
                inside = 0 <= t[0] < dim and 0 <= t[1] < dim
                assert reach[a - 1] == (dim * dim if inside else 0), (dim, head, a)
                if inside:
                    assert tp.timed_fill(tp.np_life(st, dim), dim, t)[head] == 2     # its own head cell is entered at level 2


def test_under_never_the_reach_is_the_space_and_the_policy_space_greedy():
    rng = np.random.default_rng(3)
    n = 0
    for dim, ns, density in BOARDS[:3]:
        for _ in range(8):
            st = _random_state(rng, dim, ns, density)
            life = tp.np_life(st, dim, never=True)
            assert set(np.unique(life).tolist()) <= {0, NEVER}
            assert np.array_equal(tp.np_timed(st, dim, ns, never=True), spp.np_space(st, dim, ns))
            assert tp.timed_greedy(st, dim, ns, never=True) == spp.space_greedy(st, dim, ns)
            n += 1
    assert n == 24
    assert tp.never_pops(dict(rules=1, n_fruits=0)) and not tp.never_pops(dict(rules=1, n_fruits=1))
    assert not tp.never_pops(dict(rules=0, n_fruits=0)) and not tp.never_pops(dict(rules=2, n_fruits=0))


# ------------------------------------------------------------------------------------------ hand-built timing cases
door_state, coil_state, COIL = tp.door_state, tp.coil_state, tp.COIL


def test_a_door_opens_on_time_or_never():
    for life, entered in ((1, True), (2, True), (3, False), (4, False), (BIG, False)):
        st = door_state(life)
        L = tp.np_life(st, 7)
        assert L[3, 3] == min(life, 0xFFFE) and L[3, 0] == 0xFFFE and L[0, 3] == 1
        taken = tp.timed_fill(L, 7, (1, 3))
        assert taken[(1, 3)] == 1 and taken[(2, 3)] == 2 and taken[(0, 3)] == 2
        # lifetime t - 1 = 2 enters at level t = 3; lifetime 3 does not, and with no other route the far side is never reached
        assert taken.get((3, 3)) == (3 if entered else None), life
        assert taken.get((4, 3)) == (4 if entered else None) and ((6, 0) in taken) == entered
        assert tp.timed_fill_size(tp._bitboard(L, 7), 7, (1, 3)) == len(taken)
        # from the targets of moves 2 and 4 the door is one step further, at level 5: there a lifetime of 3 or 4 still enters
        side = 43 if life <= 4 else 21
        assert tp.np_timed(st, 7, 3)[0].tolist() == [43 if entered else 21, side, 0, side]
        assert spp.np_space(st, 7, 3)[0].tolist() == [20, 20, 0, 20]


def test_a_door_that_missed_its_time_is_taken_from_behind():
    st = door_state(3, second_route=True)
    taken = tp.timed_fill(tp.np_life(st, 7), 7, (1, 3))
    # the gap (3, 6) lies 5 steps from the target: level 6; then down the far side to (4, 3) at level 10, the door at 11
    assert taken[(3, 6)] == 6 and taken[(4, 6)] == 7 and taken[(4, 3)] == 10 and taken[(3, 3)] == 11
    assert len(taken) == 49 - 5 and tp.np_timed(st, 7, 3)[0, 0] == 44
    on_time = tp.timed_fill(tp.np_life(door_state(2, second_route=True), 7), 7, (1, 3))
    assert on_time[(3, 3)] == 3 and on_time[(4, 3)] == 4 and len(on_time) == 44


def test_the_coiled_snake_leaves_by_its_own_tail():
    st = coil_state()
    space, reach = spp.np_space(st, 7, 1)[0], tp.np_timed(st, 7, 1)[0]
    assert space.tolist() == [38, 0, 2, 38]                       # the pocket is smaller than the body: not eligible
    taken = tp.timed_fill(tp.np_life(st, 7), 7, (2, 3))
    assert taken[(1, 3)] == 2 and taken[(2, 2)] == 2 and taken[(1, 2)] == 3 and taken[(3, 2)] == 3   # out through the tail
    assert reach[2] >= len(COIL) and reach[1] == 0
    # by L1 the pocket's cell (2, 3) is 1 from the fruit, the targets of moves 1 and 4 are 3 away
    assert spp.space_greedy(st, 7, 1) == [1] and tp.timed_greedy(st, 7, 1) == [3]
    # a body that still grows by one keeps its tail one step longer: the front has passed the exit by then, and only the
    # last front expands, so the pocket stays closed
    assert tp.np_timed(dict(st, grow_to=[10]), 7, 1)[0, 2] == 2 and tp.timed_greedy(dict(st, grow_to=[10]), 7, 1) == [1]
    # a body that never recedes stays out of the pocket
    assert tp.timed_greedy(st, 7, 1, never=True) == [1]


def test_pending_growth_and_bodies_longer_than_grow_to():
    assert tp.np_life(_st([[(2, 2)]], [], grow_to=[3]), 5)[2, 2] == 3            # len 1, grow_to 3
    assert tp.np_life(_st([[(2, 2)]], [], grow_to=[BIG]), 5)[2, 2] == 0xFFFE     # no 32-bit overflow, capped
    assert tp.np_life(_st([[(2, 2)]], [], grow_to=[0]), 5)[2, 2] == 1
    body = [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0)]
    assert tp.np_life(_st([body], [], grow_to=[2]), 5)[:, 0].tolist() == [5, 4, 3, 2, 1]      # len > grow_to: len - i
    assert tp.np_life(_st([body], [], grow_to=[8]), 5)[:, 0].tolist() == [8, 7, 6, 5, 4]
    assert tp.np_life(_st([body], [], grow_to=[0x10000]), 5)[:, 0].tolist() == [0xFFFE] * 3 + [0xFFFD, 0xFFFC]   # the cap
    stacked = [(0, 0), (1, 0), (0, 0), (1, 0), (1, 0)]
    assert tp.np_life(_st([stacked, [(1, 0)] * 2], [], grow_to=[5, 9]), 5)[:2, 0].tolist() == [5, 9]   # the maximum, across snakes
    assert tp.np_life(_st([[(-1, 0), (5, 5), (0, 5), (4, 4)]], []), 5).sum() == 1                      # outside the grid: ignored
    assert (tp.np_life(_st([body], [], grow_to=[2]), 5, never=True)[:, 0] == NEVER).all()


# ------------------------------------------------------------------------------------------ lifetimes against the oracle's play
def _play_windows(rules, ns, n_fruits, steps, seed):
    """The oracle under space_greedy with 15 % random moves 1..4; snake_env and adversarial with auto reset (a window ends
    where its env's episode does), new_world without it, played on past done.  For every start step, snake and k = 1..8, as
    long as the snake's grow_to is unchanged, its body non-empty and its velocity non-zero: the body after k steps, from
    index k on, must be the start pieces with lifetime > k.  Returns (windows checked, mismatches)."""
    cfg = sp.scenario(rules, 10, ns, "space_greedy", steps, 8, seed=seed, n_fruits=n_fruits)
    never = tp.never_pops(cfg)
    auto_reset = rules != "new_world"
    ora = sp.make_oracle(cfg, auto_reset=auto_reset)
    read = sp._StateReader(ora)
    ora.reset()
    rng = np.random.default_rng(seed)
    history, ended = [], []
    for _ in range(steps + 1):
        states = [read(e) for e in range(8)]
        history.append(states)
        act = spp.choose_actions(cfg, states, [None] * 8)
        rand = rng.integers(1, 5, act.shape).astype(np.int32)
        done = ora.step(np.where(rng.random(act.shape) < 0.15, rand, act).astype(np.int32))[2]
        ended.append(np.asarray(done).astype(bool) & auto_reset)    # the state behind this step belongs to the next episode
    checked = bad = 0
    for t0 in range(steps):
        for e in range(8):
            st0 = history[t0][e]
            for s in range(ns):
                body0, g0 = st0["snakes"][s], st0["grow_to"][s]
                if not body0:
                    continue
                for k in range(1, 9):
                    if t0 + k > steps or ended[t0 + k - 1][e]:
                        break
                    st = history[t0 + k][e]
                    if st["grow_to"][s] != g0 or not st["snakes"][s] or tuple(st["vels"][s]) == (0, 0):
                        break
                    want = [p for i, p in enumerate(body0) if tp.piece_life(len(body0), g0, i, never) > k]
                    checked += 1
                    bad += st["snakes"][s][k:] != want
    return checked, bad


@pytest.mark.parametrize("rules,ns,n_fruits,steps,floor", [("snake_env", 3, 3, 250, 5000), ("adversarial", 3, 3, 250, 5000),
                                                           ("new_world", 4, 5, 300, 1000), ("new_world", 4, 1, 150, 1000),
                                                           ("new_world", 4, 0, 150, 1000)])
def test_lifetimes_against_the_oracles_play(rules, ns, n_fruits, steps, floor):
    checked, bad = _play_windows(rules, ns, n_fruits, steps, seed=11)
    print(f"{rules} 10x10x{ns}, {n_fruits} fruits, {steps} steps: {checked} windows, {bad} mismatches")
    assert bad == 0 and checked >= floor, (checked, bad)


# ------------------------------------------------------------------------------------------ survival, on the oracle alone
@pytest.mark.parametrize("ns,envs,steps,space,timed", [
    (3, 16, 1500, (441, 22960, 3212.0), (334, 22931, 3325.0, 915)),
    (1, 8, 2000, (60, 14479, 1271.0), (24, 9950, 917.0, 698))])
def test_timed_greedy_survives_longer_than_space_greedy_on_the_oracle(ns, envs, steps, space, timed):
    """snake_env 10x10, seed 5, eps 0, every snake under the same policy, auto reset on, the oracle alone: (episodes ended,
    sum of their lengths, total reward[, snake-steps at which space_greedy would have played another action on the same
    state]).  10x10x3, 16 x 1 500: space_greedy 441 / mean length 52.06 / 3 212, timed_greedy 334 / 68.66 / 3 325, 915 of
    72 000 snake-steps differ.  10x10x1, 8 x 2 000: 60 / 241.3 / 1 271 against 24 / 414.6 / 917, 698 differ.  Both plays
    are deterministic: no tolerance."""
    cfg = sp.scenario("snake_env", 10, ns, "timed_greedy", steps, envs, seed=5)
    got_s = tp.survival(cfg, "space_greedy", steps)
    got_t = tp.survival(cfg, "timed_greedy", steps, compare="space_greedy")
    print(f"10x10x{ns}: space_greedy {got_s[0]} / {got_s[1] / got_s[0]:.2f} / {got_s[2]:.0f}, timed_greedy {got_t[0]} / "
          f"{got_t[1] / got_t[0]:.2f} / {got_t[2]:.0f}, {got_t[3]} of {envs * steps * ns} snake-steps differ")
    assert got_t[0] < got_s[0]                                       # fewer ended episodes
    assert got_s[:3] == space and got_t == timed
