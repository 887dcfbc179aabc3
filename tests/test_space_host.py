"""CPU-side checks of reachable-space counts and the flood-fill opponent (msnake_space_actions,
MultiSnakeVecEnv.scripted_actions_device("space_greedy"), reachable_space_device, selfplay.ScriptedOpponent): the entry
point is declared, exported and refuses a NULL handle before it touches the GPU; the helper tests/space_play.py on
hand-computed boards; the policy's strength over safe_greedy on the oracle alone; dispatch by name on fake envs.
No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import msnake
import scripted_play as sp
import space_play as spp
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_space_actions\(msnake_handle h, uint32_t snake_mask, int32_t\* actions_dev, int32_t action_stride,\s*"
           r"uint8_t\* safe_dev, uint16_t\* space_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_space_actions" in msnake._capi.SYMBOLS
    assert msnake._capi.SCRIPTED_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2}   # no new policy id
    lib = msnake._capi.load()
    assert lib.msnake_space_actions is not None and lib.msnake_abi_version() == 3


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_space_actions(None, 1, None, 3, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ np_space by hand
def _st(snakes, fruits):
    n = len(snakes)
    return {"t": 0, "ctr": 0, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n, "grow_to": [max(len(b), 1) for b in snakes],
            "alive": [True] * n, "in_dead": [False] * n}


def test_np_space_on_an_empty_3x3():
    # the head in the centre: the 8 other cells are one region, every move sees all of it
    assert spp.np_space(_st([[(1, 1)]], []), 3, 1).tolist() == [[8, 8, 8, 8]]
    # the head in a corner: two moves leave the board
    assert spp.np_space(_st([[(0, 0)]], []), 3, 1).tolist() == [[8, 8, 0, 0]]
    # heads outside the grid count for nothing: move 1 from (-1, 1) enters a completely free board
    assert spp.np_space(_st([[(-1, 1)]], []), 3, 1).tolist() == [[9, 0, 0, 0]]
    # an empty body, and a second snake column that the state does not have
    assert spp.np_space(_st([[]], []), 3, 2).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]


def test_np_space_with_a_full_width_wall_splitting_a_6x6():
    # snake 1 is the wall c1 == 2 across the whole board: above it 2 rows (12 cells), below it 3 rows (18 cells)
    wall = [(x, 2) for x in range(6)]
    # snake 0's head sits IN the wall row (stacked on a wall cell, which the rules allow): move 2 goes down, move 4 up
    got = spp.np_space(_st([[(3, 2)], wall], []), 6, 2)
    assert got[0].tolist() == [0, 18, 0, 12]
    # the wall's own head (0, 2): right is the wall, left is off the board
    assert got[1].tolist() == [0, 18, 0, 12]
    # a head in the upper part takes one cell away from that region
    got = spp.np_space(_st([[(0, 0)], wall], []), 6, 2)
    assert got[0].tolist() == [11, 11, 0, 0]
    # duplicates and cells outside the grid change nothing
    got = spp.np_space(_st([[(0, 0), (0, 0), (-1, 0), (6, 6)], wall + wall[:3]], []), 6, 2)
    assert got[0].tolist() == [11, 11, 0, 0]


def test_np_space_with_a_pocket_of_size_one():
    # the corner (0, 0) of a 5x5 is closed off by the head at (1, 0) and a body cell at (0, 1)
    st = _st([[(1, 0), (1, 1), (0, 1)]], [])
    assert spp.np_space(st, 5, 1).tolist() == [[21, 0, 1, 0]]   # 25 - 3 body cells - the pocket = 21


# ------------------------------------------------------------------------------------------ the policy by hand
def _pocket_state(fruits, tail=()):
    """7x7.  The head (3, 3) of a 9-cell body closes a pocket of 2 cells, (2, 3) and (1, 3), entered by move 3; move 1 leads
    into the open board, moves 2 and 4 into the body."""
    body = [(3, 3), (3, 4), (2, 4), (1, 4), (0, 4), (0, 3), (0, 2), (1, 2), (2, 2), (3, 2)] + list(tail)
    return _st([body], fruits), body


def test_a_pocket_smaller_than_the_body_is_refused_even_with_the_fruit_inside():
    st, body = _pocket_state([(2, 3)])
    assert spp.np_space(st, 7, 1).tolist() == [[49 - len(body) - 2, 0, 2, 0]]
    assert sp.safe_greedy(st, 7, 1, None) == [3]          # one cell ahead: into the pocket, onto the fruit
    assert spp.space_greedy(st, 7, 1) == [1]              # need = min(10, 37) = 10 > 2
    # a body short enough for the pocket goes for the fruit: the same walls, as a second snake's body
    st2 = _st([[(3, 3), (3, 4)], body[2:]], [(2, 3)])
    assert spp.np_space(st2, 7, 2)[0].tolist() == [37, 0, 2, 0]
    assert spp.space_greedy(st2, 7, 2)[0] == 3            # need = min(2, 37) = 2 <= 2


def test_when_every_region_is_smaller_than_the_body_the_largest_wins():
    # 6x6, snake 1 walls off the corner: snake 0's head (1, 1) has a pocket of 1 cell by move 3, of 2 cells by move 4,
    # of 3 cells by move 2; move 1 is blocked.  Its body is 9 cells long (stacked duplicates count for the length)
    wall = [(2, 0), (2, 1), (2, 2), (2, 3), (1, 4), (0, 4), (0, 2)] + [(x, y) for x in range(3, 6) for y in range(6)]
    st = _st([[(1, 1)] + [(0, 1)] * 8, wall + [(2, 4), (2, 5), (0, 5), (1, 5)]], [(0, 0), (0, 0)])
    # regions: (0, 0) + (1, 0) by move 4 (2 cells); (1, 2), (1, 3), (0, 3) by move 2 (3 cells); move 3 hits the body
    assert spp.np_space(st, 6, 2)[0].tolist() == [0, 3, 0, 2]
    assert sp.safe_greedy(st, 6, 2, None)[0] == 4         # towards the fruit at (0, 0)
    assert spp.space_greedy(st, 6, 2)[0] == 2             # need = min(9, 3) = 3: only move 2 is eligible


def test_a_tie_goes_to_the_lower_move_number():
    # an open 9x9, the fruit diagonally off the head: moves 1 and 2 are equally near, then 3 and 4
    assert spp.space_greedy(_st([[(4, 4)]], [(6, 6)]), 9, 1) == [1]
    assert spp.space_greedy(_st([[(4, 4)]], [(2, 2)]), 9, 1) == [3]
    # moves 1 and 2 tie on distance but move 1 leads into a pocket smaller than the body: 2 wins, not 1
    # 7x7, the head (3, 3) with a 6-cell body; cell (4, 3) is a pocket of size 1 closed by snake 1
    st = _st([[(3, 3), (3, 2), (2, 2), (2, 3), (2, 4), (1, 4)], [(5, 3), (4, 2), (4, 4)]], [(5, 5)])
    assert spp.np_space(st, 7, 2)[0].tolist() == [1, 39, 0, 0]
    assert sp.safe_greedy(st, 7, 2, None)[0] == 1 and spp.space_greedy(st, 7, 2)[0] == 2


def test_an_empty_fruit_list_and_an_empty_body():
    st, _ = _pocket_state([])
    assert spp.space_greedy(st, 7, 1) == [1]                                       # distance 0 everywhere: the first eligible move
    assert spp.space_greedy(_st([[(0, 0)]], []), 4, 1) == [1]
    assert spp.space_greedy(_st([[(3, 3)]], []), 4, 1) == [3]                      # only 3 and 4 stay on the board
    assert spp.space_greedy(_st([[], [(1, 1)]], [(0, 0)]), 4, 2) == [0, 3]         # an empty body plays 0
    assert spp.space_greedy(_st([[(0, 0)], [(1, 0), (0, 1)]], [(3, 3)]), 4, 2)[0] == 0   # no open move


def test_the_serpentine_mazes_are_one_corridor():
    for dim, cells in ((6, 21), (33, 33 * 17 + 16), (62, 1953)):
        for tr in (False, True):
            walls, path = spp.serpentine(dim, tr)
            assert len(path) == cells and len(set(path)) == cells
            assert all(abs(a[0] - b[0]) + abs(a[1] - b[1]) == 1 for a, b in zip(path, path[1:]))
            # a head in the middle of the corridor splits it into the part before and the part behind
            i = cells // 2
            st = _st([[path[i]], walls], [])
            got = sorted(v for v in spp.np_space(st, dim, 2)[0].tolist() if v)
            assert got == sorted([i, cells - 1 - i])


# ------------------------------------------------------------------------------------------ strength, on the oracle alone
def test_space_greedy_outlives_safe_greedy_on_the_oracle():
    """S19x3, 8 envs, 1 200 steps, eps 0, the oracle alone: mean length of the episodes that ended.  Measured 283.5
    (25 episodes, longest body 143) against 96.7 (93 episodes, longest body 85), a ratio of 2.9; the floor is 1.5."""
    cfg = dict(sp.SCENARIOS["S19x3"], num_envs=8)
    greedy, n_g, body_g = spp.mean_episode_length(cfg, "safe_greedy", 1200)
    space, n_s, body_s = spp.mean_episode_length(cfg, "space_greedy", 1200)
    print(f"safe_greedy {greedy:.1f} over {n_g} episodes (longest body {body_g}); space_greedy {space:.1f} over {n_s} "
          f"(longest body {body_s}); ratio {space / greedy:.2f}")
    assert n_g >= 20 and n_s >= 10
    assert space >= 1.5 * greedy, (space, greedy)
    assert body_s > body_g


# ------------------------------------------------------------------------------------------ dispatch by name
class _FakeEnv:
    """CPU stand-in with the device-side surface learn() and ScriptedOpponent use (as in test_scripted_host.py)."""

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
            out[:, s] = {"safe_greedy": 2, "hamiltonian": 3, "space_greedy": 4}[policy]
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


def test_selfplay_dispatches_space_greedy_by_name(tmp_path):
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "space_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "safe_greedy", 2, columns=team)
    env.reset_device()
    selfplay.refresh_scripted([o1, o2])
    assert sorted(env.scripted_calls) == [("safe_greedy", (2,), 0), ("space_greedy", (1,), 0)]
    assert o1.step()[0].tolist() == [4] * 8 and o2.step()[0].tolist() == [2] * 8
    assert selfplay.ScriptedOpponent(env, "space_greedy", 2).step()[0].tolist() == [4] * 8   # a lone opponent asks itself
    with pytest.raises(ValueError):
        selfplay.ScriptedOpponent(env, "space", 1)
    env2 = _FakeEnv()
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 2, nminibatches=2, noptepochs=1, opponent_save_interval=2, log_fn=None)
    selfplay.learn(env2, save_dir=str(tmp_path / "run"), scripted_opponents={1: "space_greedy"}, **kw)
    assert env2.scripted_calls == [("space_greedy", (1,), t) for t in range(8)]
    assert env2.last_actions[:, 1].tolist() == [4] * 8
    assert not any(f.startswith("opponent1_") for f in os.listdir(str(tmp_path / "run")))   # no pool for that slot


class _FakeLib:
    """Records the C calls of MultiSnakeVecEnv's scripted entry points."""

    def __init__(self):
        self.calls = []

    def msnake_space_actions(self, *a):
        self.calls.append(("space",) + a)
        return 0

    def msnake_scripted_actions(self, *a):
        self.calls.append(("scripted",) + a)
        return 0


def _bare_env(n=5, ns=3):
    """A MultiSnakeVecEnv with only what scripted_actions_device / reachable_space_device touch, on the CPU."""
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env._scripted_fn, env._space_fn = lib.msnake_scripted_actions, lib.msnake_space_actions
    env._scripted_out = torch.zeros((n, ns), dtype=torch.int32)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    return env, lib


def test_vec_env_dispatches_by_name_and_checks_space_out():
    env, lib = _bare_env()
    out = torch.zeros((5, 4), dtype=torch.int32)
    safe = torch.zeros((5, 3), dtype=torch.uint8)
    space = torch.zeros((5, 3, 4), dtype=torch.uint16)
    assert env.scripted_actions_device("space_greedy", snakes=[2, 0], out=out) is out
    assert lib.calls[-1] == ("space", 1234, 0b101, out.data_ptr(), 4, None, None, 77)
    got = env.scripted_actions_device("space_greedy", out=out, safe_out=safe, space_out=space)
    assert len(got) == 3 and got[0] is out and got[1] is safe and got[2] is space
    assert lib.calls[-1] == ("space", 1234, 0b111, out.data_ptr(), 4, safe.data_ptr(), space.data_ptr(), 77)
    got = env.scripted_actions_device("space_greedy", space_out=space)
    assert got[0] is env._scripted_out and got[1] is space and lib.calls[-1][4] == 3
    # the counts alone
    assert env.reachable_space_device(out=space) is space
    assert lib.calls[-1] == ("space", 1234, 0, None, 0, None, space.data_ptr(), 77)
    # the other policies still go to msnake_scripted_actions, with their ids
    env.scripted_actions_device("safe_greedy", out=out)
    assert lib.calls[-1][:4] == ("scripted", 1234, 1, 0b111)
    env.scripted_actions_device("hamiltonian", snakes=[1], out=out, safe_out=safe)
    assert lib.calls[-1][:4] == ("scripted", 1234, 2, 0b010)
    n_calls = len(lib.calls)
    # space_out belongs to space_greedy alone, and has one shape and type
    for pol in ("safe_greedy", "hamiltonian", None):
        with pytest.raises(ValueError, match="space_out"):
            env.scripted_actions_device(pol, out=out, safe_out=safe, space_out=space)
    for bad in (torch.zeros((5, 3, 4), dtype=torch.int16), torch.zeros((5, 3), dtype=torch.uint16),
                torch.zeros((5, 4, 4), dtype=torch.uint16), torch.zeros((5, 3, 8), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="space_out"):
            env.scripted_actions_device("space_greedy", out=out, space_out=bad)
        with pytest.raises(ValueError, match="space_out"):
            env.reachable_space_device(out=bad)
    with pytest.raises(ValueError, match="policy must be 'safe_greedy', 'hamiltonian' or None"):
        env.scripted_actions_device("greedy")                      # the text for unknown names is the one it was
    with pytest.raises(ValueError):
        env.scripted_actions_device("space_greedy", snakes=[3])
    assert len(lib.calls) == n_calls                                 # every refusal came before the C call
