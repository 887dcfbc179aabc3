"""CPU-side checks of the BFS fruit distances and the opponent path_greedy (msnake_path_actions,
MultiSnakeVecEnv.scripted_actions_device("path_greedy"), path_device, fruit_field_device, selfplay.ScriptedOpponent): the
entry point is declared, exported and refuses a NULL handle before it touches the GPU; the helper tests/path_play.py on
closed forms; the policy's foraging gain over space_greedy on the oracle alone; dispatch by name on fake envs.
No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import msnake
import path_play as pp
import scripted_play as sp
import space_play as spp
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = pp.NONE


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_path_actions\(msnake_handle h, uint32_t snake_mask, int32_t\* actions_dev, int32_t action_stride,\s*"
           r"uint8_t\* safe_dev, uint16_t\* path_dev, uint16_t\* field_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_PATH_NONE 0xFFFFu\b", text) and NONE == 0xFFFF
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_path_actions" in msnake._capi.SYMBOLS
    assert msnake._capi.SCRIPTED_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2}   # no new policy id
    lib = msnake._capi.load()
    assert lib.msnake_path_actions is not None and lib.msnake_abi_version() == 3


def test_the_binding_has_the_declared_signature():
    import ctypes
    restype, argtypes = msnake._capi.PROTOTYPES["msnake_path_actions"]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int
    assert argtypes == [vp, ctypes.c_uint32, vp, ctypes.c_int32, vp, vp, vp, vp]
    fn = msnake._capi.load().msnake_path_actions
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_path_actions(None, 1, None, 3, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


def test_the_names():
    C = msnake._capi
    assert C.PATH_POLICY == "path_greedy"
    assert C.SCRIPTED_OPPONENT_NAMES == C.SCRIPTED_POLICY_NAMES + ("path_greedy",)
    assert selfplay.SCRIPTED_OPPONENTS is C.SCRIPTED_OPPONENT_NAMES
    assert "path_greedy" not in selfplay.SCRIPTED_POLICIES            # the older tuple is as it was


# ------------------------------------------------------------------------------------------ the helper on closed forms
def _st(snakes, fruits):
    n = len(snakes)
    return {"t": 0, "ctr": 0, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n, "grow_to": [max(len(b), 1) for b in snakes],
            "alive": [True] * n, "in_dead": [False] * n}


def _l1(cell, fruits):
    return min(abs(cell[0] - f[0]) + abs(cell[1] - f[1]) for f in fruits)


def _round_one_cell(t, f, head):
    """The distance from t to f on a board whose only obstacle is `head`: L1, but 2 more when the head lies on the
    straight line between the two (the one case in which every monotone route crosses it)."""
    d = abs(t[0] - f[0]) + abs(t[1] - f[1])
    for k in (0, 1):
        if t[k] == f[k] == head[k] and min(t[1 - k], f[1 - k]) < head[1 - k] < max(t[1 - k], f[1 - k]):
            return d + 2
    return d


def test_a_lone_one_cell_snake_on_an_empty_board_has_l1_paths():
    """path == L1 to the nearest fruit for every open move -- except for the move that points straight away from a fruit
    in line behind the head: that target has to walk round the head, which costs 2."""
    rng = np.random.default_rng(1)
    n_l1 = n_round = 0
    for dim in (2, 3, 7, 19):
        for _ in range(20):
            head = tuple(int(v) for v in rng.integers(0, dim, 2))
            fruits = [tuple(int(v) for v in rng.integers(0, dim, 2)) for _ in range(int(rng.integers(1, 4)))]
            fruits = [f for f in fruits if f != head] or [((head[0] + 1) % dim, head[1])]
            st = _st([[head]], fruits)
            got = pp.np_path(st, dim, 1)[0]
            for a, (d0, d1) in pp.DIRS.items():
                t = (head[0] + d0, head[1] + d1)
                if 0 <= t[0] < dim and 0 <= t[1] < dim:
                    want = min(_round_one_cell(t, f, head) for f in fruits)
                    assert got[a - 1] == want >= _l1(t, fruits), (dim, head, fruits, a)
                    n_l1 += want == _l1(t, fruits)
                    n_round += want != _l1(t, fruits)
                else:
                    assert got[a - 1] == NONE
    assert n_l1 > 150 and n_round > 0


def _random_state(rng, dim, ns, density):
    """Random bodies (not connected: the helper does not care) covering about `density` of the board, random fruits."""
    cells = [(x, y) for x in range(dim) for y in range(dim)]
    rng.shuffle(cells)
    k = int(density * dim * dim)
    parts = np.array_split(np.arange(k), ns)
    snakes = [[cells[i] for i in p] for p in parts]
    fruits = [tuple(int(v) for v in rng.integers(-1, dim + 1, 2)) for _ in range(int(rng.integers(0, 6)))]
    return _st(snakes, fruits)


def test_field_properties_on_random_boards():
    rng = np.random.default_rng(2)
    for dim, ns, density in ((6, 2, 0.3), (10, 3, 0.5), (19, 3, 0.4), (33, 4, 0.55)):
        for _ in range(6):
            st = _random_state(rng, dim, ns, density)
            occ = spp.occupancy(st, dim)
            F = pp.np_field(st, dim)
            sources = {(f[0], f[1]) for f in st["fruits"] if 0 <= f[0] < dim and 0 <= f[1] < dim and not occ[f[0], f[1]]}
            # 0 exactly on the free fruit cells
            assert {(int(x), int(y)) for x, y in zip(*np.nonzero(F == 0))} == sources
            # NONE on `used`, finite values at most dim^2 - 2
            assert (F[occ] == NONE).all()
            assert ((F == NONE) | (F <= dim * dim - 2)).all()
            # neighbouring free cells differ by at most 1 (so both are finite or both NONE)
            for a, b in ((F[1:, :], F[:-1, :]), (F[:, 1:], F[:, :-1])):
                both = (a != NONE) & (b != NONE)
                assert (np.abs(a - b)[both] <= 1).all()
            free = ~occ
            for fa, fb, a, b in ((free[1:, :], free[:-1, :], F[1:, :], F[:-1, :]), (free[:, 1:], free[:, :-1], F[:, 1:], F[:, :-1])):
                pair = fa & fb
                assert ((a == NONE) == (b == NONE))[pair].all()
            # NONE on a free cell exactly when its region holds no source: compare with a fill per source region
            reach = np.zeros((dim, dim), bool)
            stack = list(sources)
            for c in stack:
                reach[c] = True
            while stack:
                x, y = stack.pop()
                for d0, d1 in pp.DIRS.values():
                    u, v = x + d0, y + d1
                    if 0 <= u < dim and 0 <= v < dim and free[u, v] and not reach[u, v]:
                        reach[u, v] = True
                        stack.append((u, v))
            assert ((F != NONE) == reach).all()
            # path >= L1 to the nearest source, always
            if sources:
                for x, y in zip(*np.nonzero(F != NONE)):
                    assert F[x, y] >= _l1((x, y), sources)
            # np_path reads the field at the open targets
            P = pp.np_path(st, dim, ns)
            for s in range(ns):
                hx, hy = st["snakes"][s][0]
                for a, (d0, d1) in pp.DIRS.items():
                    x, y = hx + d0, hy + d1
                    is_open = 0 <= x < dim and 0 <= y < dim and not occ[x, y]
                    assert P[s, a - 1] == (F[x, y] if is_open else NONE)


@pytest.mark.parametrize("dim", [6, 33, 62])
def test_the_serpentine_corridor(dim):
    for tr in (False, True):
        walls, path = spp.serpentine(dim, tr)
        n = len(path)
        pairs = [(0, n - 1), (n - 1, 0), (n // 2, 0), (n // 2, n - 1), (1, 3), (n - 3, n - 5), (n // 3, n // 3 + 1)]
        for i, j in pairs:
            st = _st([[path[i]], walls], [path[j]])
            got = pp.np_path(st, dim, 2)[0]
            for a, (d0, d1) in pp.DIRS.items():
                t = (path[i][0] + d0, path[i][1] + d1)
                if i + 1 < n and t == path[i + 1]:
                    want = j - i - 1 if j > i else NONE
                elif i > 0 and t == path[i - 1]:
                    want = i - j - 1 if j < i else NONE
                else:
                    want = NONE                       # a wall or the border
                assert got[a - 1] == want, (dim, tr, i, j, a)
            F = pp.np_field(st, dim)
            lo, hi = (i + 1, n) if j > i else (0, i)    # the part of the corridor on the fruit's side of the head
            for k, c in enumerate(path):
                assert F[c] == (abs(k - j) if lo <= k < hi else NONE)
    if dim == 62:
        walls, path = spp.serpentine(62)
        assert max(pp.np_path(_st([[path[0]], walls], [path[-1]]), 62, 2)[0][:2]) == NONE
        assert min(pp.np_path(_st([[path[0]], walls], [path[-1]]), 62, 2)[0]) == 1951      # the longest distance there is


def test_path_greedy_is_space_greedy_where_no_source_is_reachable():
    rng = np.random.default_rng(3)
    n = 0
    for dim, ns, density in ((6, 2, 0.3), (10, 3, 0.5), (19, 3, 0.4)):
        for _ in range(8):
            st = _random_state(rng, dim, ns, density)
            flat = [c for b in st["snakes"] for c in b]
            for fruits in ([], flat[:3], [flat[0], flat[0], [-1, 2], [dim, dim]]):       # empty, under bodies, outside
                st2 = dict(st, fruits=[list(f) for f in fruits])
                assert (pp.np_field(st2, dim) == NONE).all()
                assert pp.path_greedy(st2, dim, ns) == spp.space_greedy(st2, dim, ns)
                n += 1
    # a fruit walled off: 7x7, the wall c1 == 3 across the board, the fruit below it, the snake above it
    wall = [(x, 3) for x in range(7)]
    st = _st([[(2, 1), (2, 0)], wall], [(5, 5)])
    assert (pp.np_path(st, 7, 2)[0] == NONE).all() and pp.np_field(st, 7)[5, 6] == 1
    assert pp.path_greedy(st, 7, 2) == spp.space_greedy(st, 7, 2)
    assert n == 72


def test_path_greedy_walks_round_a_body_where_space_greedy_heads_into_it():
    # 7x7: the fruit (3, 1) sits two cells from the head (3, 3) behind the bar c1 == 2, x = 1..5.  Move 4 (into the bar)
    # is closed; by L1 moves 1, 2 and 3 tie at distance 3 (then 1 wins); by foot both ways round the bar are 7 steps.
    bar = [(x, 2) for x in range(1, 6)]
    st = _st([[(3, 3)], bar], [(3, 1)])
    assert pp.np_path(st, 7, 2)[0].tolist() == [7, 9, 7, NONE]
    assert pp.path_greedy(st, 7, 2)[0] == 1 and spp.space_greedy(st, 7, 2)[0] == 1
    # a longer bar on one side: x = 1..6, so the way round leads left only; L1 still says right (the tie goes to move 1)
    bar = [(x, 2) for x in range(1, 7)]
    st = _st([[(3, 3)], bar], [(3, 1)])
    assert pp.np_path(st, 7, 2)[0].tolist() == [11, 9, 7, NONE]   # (move 1 has to pass below the head first)
    assert spp.space_greedy(st, 7, 2)[0] == 1 and pp.path_greedy(st, 7, 2)[0] == 3
    # a move onto the fruit has path 0; the move away from it walks round the head
    assert pp.np_path(_st([[(3, 3)]], [(3, 4)]), 7, 1)[0].tolist() == [2, 0, 2, 4]
    # eligibility is space_greedy's: the fruit inside a pocket smaller than the body is not walked into
    body = [(3, 3), (3, 4), (2, 4), (1, 4), (0, 4), (0, 3), (0, 2), (1, 2), (2, 2), (3, 2)]
    st = _st([body], [(2, 3)])
    assert pp.np_path(st, 7, 1)[0].tolist() == [NONE, NONE, 0, NONE]
    assert pp.path_greedy(st, 7, 1) == spp.space_greedy(st, 7, 1) == [1]
    # an empty body plays 0, and so does a snake without an open move
    assert pp.path_greedy(_st([[], [(1, 1)]], [(0, 0)]), 4, 2) == [0, 3]
    assert pp.path_greedy(_st([[(0, 0)], [(1, 0), (0, 1)]], [(3, 3)]), 4, 2)[0] == 0


# ------------------------------------------------------------------------------------------ strength, on the oracle alone
def test_path_greedy_forages_better_than_space_greedy_on_the_oracle():
    """A10x3, 16 envs, 600 steps, eps 0, the oracle alone: total reward, and the snake-steps at which space_greedy would
    have played another action on the same state.  The helper gives 0.1705 reward per env-step (169 episodes ended, mean
    length 51.1) against 0.1608 (188 episodes, mean length 45.7), and 2 253 of the 28 800 snake-steps differ.  Both
    plays are deterministic: no tolerance."""
    cfg = dict(sp.SCENARIOS["A10x3"], num_envs=16)
    path, ep_p, len_p, differ = pp.forage(cfg, "path_greedy", 600, compare="space_greedy")
    space, ep_s, len_s, _ = pp.forage(cfg, "space_greedy", 600)
    print(f"path_greedy {path / 9600:.4f} reward per env-step ({ep_p} episodes, mean length {len_p / max(ep_p, 1):.1f}); "
          f"space_greedy {space / 9600:.4f} ({ep_s} episodes, mean length {len_s / max(ep_s, 1):.1f}); "
          f"{differ} of 28800 snake-steps differ")
    assert path > space, (path, space)
    assert differ >= 500, differ


# ------------------------------------------------------------------------------------------ dispatch by name
class _FakeEnv:
    """CPU stand-in with the device-side surface learn() and ScriptedOpponent use (as in test_space_host.py): its
    scripted_actions_device has NO path_out / field_out keyword, like the fake envs of the older host tests."""

    def __init__(self, n=8, n_snakes=3, seed=0):
        self.num_envs, self.n_snakes, self.obs_shape, self.device = n, n_snakes, (12, 12, 9), torch.device("cpu")
        self.g = torch.Generator().manual_seed(seed)
        self.len = torch.zeros(n, dtype=torch.int32)
        self.scripted_calls, self.steps, self.last_actions = [], 0, None

    def reset_device(self):
        return torch.randint(0, 256, (self.num_envs,) + self.obs_shape, dtype=torch.uint8, generator=self.g)

    def scripted_actions_device(self, policy, snakes=None, out=None, safe_out=None, space_out=None):
        self.scripted_calls.append((policy, tuple(snakes), self.steps))
        if out is None:
            out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32)
        for s in snakes:
            out[:, s] = {"safe_greedy": 2, "space_greedy": 4, "path_greedy": 3}[policy]
        return out

    def step_device(self, actions):
        assert actions.shape == (self.num_envs, self.n_snakes) and actions.dtype == torch.int32
        self.steps += 1
        self.last_actions = actions.clone()
        self.len += 1
        done = (torch.rand(self.num_envs, generator=self.g) < 0.3)
        rew = torch.randint(0, 2, (self.num_envs,), generator=self.g).float()
        info = torch.zeros((self.num_envs, 4), dtype=torch.int32)
        info[:, 1] = self.len
        self.len = torch.where(done, torch.zeros_like(self.len), self.len)
        obs = torch.randint(0, 256, (self.num_envs,) + self.obs_shape, dtype=torch.uint8, generator=self.g)
        return obs, rew, done.to(torch.uint8), info


def test_selfplay_dispatches_path_greedy_by_name(tmp_path):
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "path_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "safe_greedy", 2, columns=team)
    env.reset_device()
    selfplay.refresh_scripted([o1, o2])
    assert sorted(env.scripted_calls) == [("path_greedy", (1,), 0), ("safe_greedy", (2,), 0)]
    assert o1.step()[0].tolist() == [3] * 8 and o2.step()[0].tolist() == [2] * 8
    assert selfplay.ScriptedOpponent(env, "path_greedy", 2).step()[0].tolist() == [3] * 8   # a lone opponent asks itself
    with pytest.raises(ValueError, match="'path_greedy'"):                                   # the refusal lists the new name
        selfplay.ScriptedOpponent(env, "path", 1)
    env2 = _FakeEnv()
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 2, nminibatches=2, noptepochs=1, opponent_save_interval=2, log_fn=None)
    selfplay.learn(env2, save_dir=str(tmp_path / "run"), scripted_opponents={1: "path_greedy"}, **kw)
    assert env2.scripted_calls == [("path_greedy", (1,), t) for t in range(8)]
    assert env2.last_actions[:, 1].tolist() == [3] * 8
    assert not any(f.startswith("opponent1_") for f in os.listdir(str(tmp_path / "run")))   # no pool for that slot


def test_the_tools_offer_the_new_opponent():
    for tool in ("train_selfplay.py", "eval_vs_scripted.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "SCRIPTED_OPPONENT_NAMES" in text and "SCRIPTED_POLICY_NAMES" not in text


class _FakeLib:
    """Records the C calls of MultiSnakeVecEnv's scripted entry points."""

    def __init__(self):
        self.calls = []

    def msnake_path_actions(self, *a):
        self.calls.append(("path",) + a)
        return 0

    def msnake_space_actions(self, *a):
        self.calls.append(("space",) + a)
        return 0

    def msnake_scripted_actions(self, *a):
        self.calls.append(("scripted",) + a)
        return 0


def _bare_env(n=5, ns=3, dim=7):
    """A MultiSnakeVecEnv with only what scripted_actions_device / path_device / fruit_field_device touch, on the CPU."""
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env.cfg = type("Cfg", (), {"dim": dim})()
    env._scripted_fn, env._space_fn, env._path_fn = lib.msnake_scripted_actions, lib.msnake_space_actions, lib.msnake_path_actions
    env._scripted_out = torch.zeros((n, ns), dtype=torch.int32)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    return env, lib


def test_vec_env_dispatches_by_name_and_checks_path_out_and_field_out():
    env, lib = _bare_env()
    out = torch.zeros((5, 4), dtype=torch.int32)
    safe = torch.zeros((5, 3), dtype=torch.uint8)
    path = torch.zeros((5, 3, 4), dtype=torch.uint16)
    field = torch.zeros((5, 7, 7), dtype=torch.uint16)
    space = torch.zeros((5, 3, 4), dtype=torch.uint16)
    assert env.scripted_actions_device("path_greedy", snakes=[2, 0], out=out) is out
    assert lib.calls[-1] == ("path", 1234, 0b101, out.data_ptr(), 4, None, None, None, 77)
    got = env.scripted_actions_device("path_greedy", out=out, safe_out=safe, path_out=path, field_out=field)
    assert len(got) == 4 and got[0] is out and got[1] is safe and got[2] is path and got[3] is field   # the return order
    assert lib.calls[-1] == ("path", 1234, 0b111, out.data_ptr(), 4, safe.data_ptr(), path.data_ptr(), field.data_ptr(), 77)
    got = env.scripted_actions_device("path_greedy", field_out=field)
    assert len(got) == 2 and got[0] is env._scripted_out and got[1] is field
    assert lib.calls[-1] == ("path", 1234, 0b111, env._scripted_out.data_ptr(), 3, None, None, field.data_ptr(), 77)
    got = env.scripted_actions_device("path_greedy", out=out, path_out=path)
    assert len(got) == 2 and got[1] is path and lib.calls[-1][6:8] == (path.data_ptr(), None)
    # each output alone: no action, no mask, not the other one
    assert env.path_device(out=path) is path
    assert lib.calls[-1] == ("path", 1234, 0, None, 0, None, path.data_ptr(), None, 77)
    assert env.fruit_field_device(out=field) is field
    assert lib.calls[-1] == ("path", 1234, 0, None, 0, None, None, field.data_ptr(), 77)
    # the siblings are called as before
    env.scripted_actions_device("space_greedy", out=out, space_out=space)
    assert lib.calls[-1] == ("space", 1234, 0b111, out.data_ptr(), 4, None, space.data_ptr(), 77)
    env.scripted_actions_device("safe_greedy", out=out)
    assert lib.calls[-1][:4] == ("scripted", 1234, 1, 0b111)
    n_calls = len(lib.calls)
    # path_out and field_out belong to path_greedy alone; the refusal names the keyword
    for pol in ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy", None):
        with pytest.raises(ValueError, match="path_out is written by policy 'path_greedy' only"):
            env.scripted_actions_device(pol, out=out, path_out=path)
        with pytest.raises(ValueError, match="field_out is written by policy 'path_greedy' only"):
            env.scripted_actions_device(pol, out=out, field_out=field)
    with pytest.raises(ValueError, match="space_out is written by policy 'space_greedy' only"):
        env.scripted_actions_device("path_greedy", out=out, space_out=space)
    # one shape and type each
    for bad in (torch.zeros((5, 3, 4), dtype=torch.int16), torch.zeros((5, 3), dtype=torch.uint16),
                torch.zeros((5, 7, 7), dtype=torch.uint16), torch.zeros((5, 3, 8), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="path_out"):
            env.scripted_actions_device("path_greedy", out=out, path_out=bad)
        with pytest.raises(ValueError, match="path_out"):
            env.path_device(out=bad)
    for bad in (torch.zeros((5, 7, 7), dtype=torch.int16), torch.zeros((5, 3, 4), dtype=torch.uint16),
                torch.zeros((5, 7, 6), dtype=torch.uint16), torch.zeros((5, 7, 14), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="field_out"):
            env.scripted_actions_device("path_greedy", out=out, field_out=bad)
        with pytest.raises(ValueError, match="field_out"):
            env.fruit_field_device(out=bad)
    with pytest.raises(ValueError, match="policy must be 'safe_greedy', 'hamiltonian' or None"):
        env.scripted_actions_device("path")                        # the text for unknown names is the one it was
    with pytest.raises(ValueError):
        env.scripted_actions_device("path_greedy", snakes=[3])
    assert len(lib.calls) == n_calls                                 # every refusal came before the C call
