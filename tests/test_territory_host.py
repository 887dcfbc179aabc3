"""CPU-side checks of the Voronoi territory counts and the opponent territory_greedy (msnake_territory_actions,
MultiSnakeVecEnv.scripted_actions_device("territory_greedy"), territory_device, selfplay.ScriptedOpponent): the entry
point is declared, exported and refuses a NULL handle before it touches the GPU; the helper tests/territory_play.py on
hand-computed boards, its fast set form pinned to its BFS form; the policy's strength over space_greedy on the oracle
alone; dispatch by name on fake envs; the tools' --opponent.  No GPU."""
import argparse
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import msnake
import scripted_play as sp
import space_play as spp
import territory_play as tp
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_territory_actions\(msnake_handle h, uint32_t snake_mask, int32_t\* actions_dev, int32_t action_stride,\s*"
           r"uint8_t\* safe_dev, uint16_t\* territory_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    contract = text.split("int msnake_territory_actions(")[0].rsplit("/*", 1)[1]
    for word in ("dA(c) < dB(c)", "ties go to the", "head-on", "space_dev", "62^2 - 1", "MSNAKE_E_ALIGN", "territory >= need"):
        assert word in contract, word
    assert "msnake_territory_actions" in msnake._capi.SYMBOLS
    assert msnake._capi.TERRITORY_POLICY == "territory_greedy"
    assert msnake._capi.SCRIPTED_POLICY == {None: 0, "safe_greedy": 1, "hamiltonian": 2}   # no new policy id
    lib = msnake._capi.load()
    assert lib.msnake_territory_actions is not None and lib.msnake_abi_version() == 3


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_territory_actions(None, 1, None, 3, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ np_territory by hand
def _st(snakes, fruits):
    n = len(snakes)
    return {"t": 0, "ctr": 0, "spare_fruits": 0, "ep_len": 0, "ep_return": 0.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [[1, 0]] * n, "grow_to": [max(len(b), 1) for b in snakes],
            "alive": [True] * n, "in_dead": [False] * n}


def _both(st, dim, ns):
    """The counts by the BFS form, after checking that the set form gives the same."""
    got = tp.np_territory(st, dim, ns)
    assert np.array_equal(got, tp.territory_sets(st, dim, ns)), (got, tp.territory_sets(st, dim, ns))
    return got.tolist()


def test_a_contested_target_counts_zero_while_the_move_is_open():
    # an empty 3x3, the heads (0, 1) and (2, 1) two cells apart: both can enter the centre, so that move is open (the
    # mask has its bit) and counts 0; the moves along the edge keep their own target and lose the tie one cell on
    st = _st([[(0, 1)], [(2, 1)]], [])
    assert _both(st, 3, 2) == [[0, 1, 0, 1], [0, 1, 0, 1]]
    assert sp.np_safe_mask(st, 3, 2).tolist() == [0b10110, 0b11100]
    assert spp.np_space(st, 3, 2).tolist() == [[7, 7, 0, 7], [0, 7, 7, 7]]
    # a 2x2 with the heads in opposite corners: every open move of either snake is contested
    st = _st([[(0, 0)], [(1, 1)]], [])
    assert _both(st, 2, 2) == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert sp.np_safe_mask(st, 2, 2).tolist() == [0b00110, 0b11000]


@pytest.mark.parametrize("dim,each", [(7, 2), (8, 3)])
def test_a_corridor_raced_from_both_ends(dim, each):
    """Row c1 == 0 is a corridor under a full-width wall (snake 2's body), the heads stand on its two ends: dim - 2
    free cells between them.  An odd number leaves the middle cell to nobody (a tie), an even number splits evenly."""
    wall = [(x, 1) for x in range(dim)]
    st = _st([[(0, 0)], [(dim - 1, 0)], wall], [])
    got = _both(st, dim, 3)
    assert got[0] == [each, 0, 0, 0] and got[1] == [0, 0, each, 0]
    assert 2 * each == dim - 2 - (dim % 2)
    assert got[2] == [0, dim * (dim - 2), 0, 0]            # the wall's head (0, 1) owns everything below the wall
    # the same race along c0: the board transposed
    st = _st([[(0, 0)], [(0, dim - 1)], [(y, x) for x, y in wall]], [])
    got = _both(st, dim, 3)
    assert got[0] == [0, each, 0, 0] and got[1] == [0, 0, 0, each] and got[2] == [dim * (dim - 2), 0, 0, 0]


def test_a_pocket_whose_mouth_the_opponent_reaches_first():
    # 5x5: snake 1's body walls off columns 3 and 4 except for the mouth (2, 4); its head (3, 3) stands inside, one step
    # from (3, 4) and two from the mouth.  Snake 0 at (0, 0) is five steps from the mouth: its reachable space is
    # everything (19 cells), its territory ends where the opponent, coming out of the mouth, meets it.
    st = _st([[(0, 0)], [(3, 3), (2, 0), (2, 1), (2, 2), (2, 3)]], [])
    assert spp.np_space(st, 5, 2)[0].tolist() == [19, 19, 0, 0]
    got = _both(st, 5, 2)
    # move 1 -> (1, 0): (1,0) (1,1) (1,2) (0,1) (0,2); (1,3) and (0,3) are ties.  move 2 -> (0, 1): also (0,3), not (0,4)
    assert got[0] == [5, 6, 0, 0]
    # the opponent owns the 9 free cells behind the wall whatever it does.  move 2 -> (3, 4) is one step from the mouth:
    # the mouth and (1, 4) on top, (1, 3) and (0, 4) are ties.  move 1 -> (4, 3) is three steps from the mouth: the mouth
    # alone, (1, 4) is a tie.  move 4 -> (3, 2) is five steps from it, as far as snake 0: nothing outside
    assert got[1] == [10, 11, 0, 9]
    # without an opponent the pocket counts
    assert _both(_st([[(0, 0)], []], []), 5, 2)[0] == [24, 24, 0, 0]


def test_an_opponent_without_an_open_move_leaves_the_space():
    # 4x4: snake 1's head (3, 3) is shut in by its own body and the border
    st = _st([[(0, 0)], [(3, 3), (2, 3), (3, 2)]], [])
    assert _both(st, 4, 2) == [[12, 12, 0, 0], [0, 0, 0, 0]]
    assert np.array_equal(tp.np_territory(st, 4, 2), spp.np_space(st, 4, 2))
    # an empty body and a snake column that the state does not have are no opponents either
    st = _st([[(1, 1)], []], [])
    assert _both(st, 3, 3) == [[8, 8, 8, 8], [0, 0, 0, 0], [0, 0, 0, 0]]
    # heads outside the grid: move 1 from (-1, 1) enters a free board, and is an opponent like any other
    assert _both(_st([[(-1, 1)]], []), 3, 1) == [[9, 0, 0, 0]]
    assert _both(_st([[(-1, 1)], [(3, 1)]], []), 3, 2) == [[3, 0, 0, 0], [0, 0, 3, 0]]


@pytest.mark.parametrize("dim", [6, 33, 62])
def test_one_snake_alone_has_its_space_on_the_serpentine_mazes(dim):
    for tr in (False, True):
        walls, path = spp.serpentine(dim, tr)
        for i in (0, len(path) // 3, len(path) - 1):
            st = _st([[path[i]] + walls], [])
            want = spp.np_space(st, dim, 1)
            assert sorted(v for v in want[0].tolist() if v) == sorted(v for v in (i, len(path) - 1 - i) if v)
            assert np.array_equal(tp.territory_sets(st, dim, 1), want)
            if dim < 62 or i == 0:
                assert np.array_equal(tp.np_territory(st, dim, 1), want)


def _random_board(rng):
    """dim 2..12, 1..4 snakes, 0..60 % of the cells in bodies; empty bodies, and heads anywhere in [-1, dim]."""
    dim, ns = int(rng.integers(2, 13)), int(rng.integers(1, 5))
    cells = [(x, y) for x in range(dim) for y in range(dim)]
    k = int(rng.uniform(0.0, 0.6) * dim * dim)
    pick = [cells[j] for j in rng.permutation(len(cells))[:k]]
    cuts = sorted(int(v) for v in rng.integers(0, k + 1, ns - 1))
    bodies = [pick[a:b] for a, b in zip([0] + cuts, cuts + [k])]
    for b in bodies:
        r = rng.random()
        if r < 0.15:
            b.clear()
        elif r < 0.45:
            b.insert(0, (int(rng.integers(-1, dim + 1)), int(rng.integers(-1, dim + 1))))
    fruits = [tuple(int(v) for v in rng.integers(0, dim, 2)) for _ in range(int(rng.integers(0, 4)))]
    return _st(bodies, fruits), dim, ns


def test_the_set_form_equals_the_distance_form_on_random_boards():
    rng = np.random.default_rng(20240)
    seen = dict(empty=0, off=0, contested=0, differs_from_space=0)
    for _ in range(400):
        st, dim, ns = _random_board(rng)
        want = tp.np_territory(st, dim, ns)
        assert np.array_equal(tp.territory_sets(st, dim, ns), want), (st, dim, ns)
        assert tp.territory_greedy(st, dim, ns) == tp.territory_greedy_bfs(st, dim, ns)
        space = spp.np_space(st, dim, ns)
        assert (want <= space).all()                      # a territory is a part of the region
        mask = sp.np_safe_mask(st, dim, ns)
        is_open = (mask[:, None] >> np.arange(1, 5)) & 1 == 1
        assert not want[~is_open].any()
        seen["empty"] += any(not b for b in st["snakes"])
        seen["off"] += any(b and not (0 <= b[0][0] < dim and 0 <= b[0][1] < dim) for b in st["snakes"])
        seen["contested"] += bool((is_open & (want == 0)).any())
        seen["differs_from_space"] += bool((want != space).any())
    assert min(seen.values()) >= 30, seen


# ------------------------------------------------------------------------------------------ the policy by hand
def test_a_tie_goes_to_the_lower_move_number():
    # an open 9x9, the fruit diagonally off the head: moves 1 and 2 are equally near, then 3 and 4
    assert tp.territory_greedy(_st([[(4, 4)]], [(6, 6)]), 9, 1) == [1]
    assert tp.territory_greedy(_st([[(4, 4)]], [(2, 2)]), 9, 1) == [3]
    # the same with an opponent far away in the corner: every move of snake 0 keeps more than its length
    st = _st([[(4, 4)], [(0, 0)]], [(6, 6)])
    assert min(v for v in tp.np_territory(st, 9, 2)[0]) > 1
    assert tp.territory_greedy(st, 9, 2)[0] == 1


def test_territory_decides_where_space_does_not():
    # the 5x5 pocket board with a 6-cell body for snake 0 (stacked duplicates count for the length): both moves lead into
    # the same 19 cells, so space_greedy takes the one nearer the fruit, move 1; territory 5 < need = min(6, 6) = 6
    # leaves only move 2
    st = _st([[(0, 0)] * 6, [(3, 3), (2, 0), (2, 1), (2, 2), (2, 3)]], [(1, 0)])
    assert tp.np_territory(st, 5, 2)[0].tolist() == [5, 6, 0, 0]
    assert spp.space_greedy(st, 5, 2)[0] == 1 and tp.territory_greedy(st, 5, 2)[0] == 2
    # a body of five cells fits behind either move: the fruit decides again
    st = _st([[(0, 0)] * 5, [(3, 3), (2, 0), (2, 1), (2, 2), (2, 3)]], [(1, 0)])
    assert tp.territory_greedy(st, 5, 2)[0] == 1


def test_all_zero_territories_make_every_open_move_eligible():
    # the 2x2 with opposite corners: every count is 0, need = 0, so the fruit decides among the open moves
    st = _st([[(0, 0)], [(1, 1)]], [(0, 1)])
    assert tp.np_territory(st, 2, 2).tolist() == [[0, 0, 0, 0], [0, 0, 0, 0]]
    assert tp.territory_greedy(st, 2, 2) == [2, 3]
    assert tp.territory_greedy(_st([[(0, 0)], [(1, 1)]], [(1, 0)]), 2, 2) == [1, 4]
    assert tp.territory_greedy(_st([[(0, 0)], [(1, 1)]], []), 2, 2) == [1, 3]       # no fruit: the first open move


def test_an_empty_fruit_list_and_an_empty_body():
    assert tp.territory_greedy(_st([[(0, 0)]], []), 4, 1) == [1]
    assert tp.territory_greedy(_st([[(3, 3)]], []), 4, 1) == [3]                      # only 3 and 4 stay on the board
    assert tp.territory_greedy(_st([[], [(1, 1)]], [(0, 0)]), 4, 2) == [0, 3]         # an empty body plays 0
    assert tp.territory_greedy(_st([[(0, 0)], [(1, 0), (0, 1)]], [(3, 3)]), 4, 2)[0] == 0   # no open move
    assert set(tp.POLICIES) == set(spp.POLICIES) | {"territory_greedy"}
    cfg = dict(dim=4, n_snakes=2, policy="territory_greedy", eps=0.0)
    assert tp.choose_actions(cfg, [_st([[], [(1, 1)]], [(0, 0)])], [None]).tolist() == [[0, 3]]


# ------------------------------------------------------------------------------------------ strength, on the oracle alone
def test_territory_greedy_ends_fewer_episodes_than_space_greedy_in_the_same_seat():
    """S19x3, 32 envs, 3 000 steps (96 000 env-steps), eps 0, the oracle alone; snakes 1 and 2 always play space_greedy.
    Episodes that ended with snake 0 under space_greedy: 302 (mean length 264.4, mean return 18.5); under
    territory_greedy: 129 (mean length 654.7, mean return 43.1): 2.34 times fewer.  (16 envs x 1 500 steps: 82 against
    28; 16 x 3 000: 153 against 63.)  The measured ratio is above 2, so the floor of 1.5 is asserted."""
    cfg = dict(sp.SCENARIOS["S19x3"], num_envs=32)
    n_s, len_s, ret_s = tp.play_seats(cfg, "space_greedy", "space_greedy", 3000)
    n_t, len_t, ret_t = tp.play_seats(cfg, "territory_greedy", "space_greedy", 3000)
    print(f"space_greedy: {n_s} episodes ended (mean length {len_s:.1f}, mean return {ret_s:.1f}); territory_greedy: {n_t} "
          f"(mean length {len_t:.1f}, mean return {ret_t:.1f}); ratio {n_s / max(n_t, 1):.2f}")
    assert n_s >= 100 and n_t >= 20
    assert n_s >= 1.5 * n_t, (n_s, n_t)
    assert len_t > len_s and ret_t > ret_s


# ------------------------------------------------------------------------------------------ dispatch by name
class _FakeEnv:
    """CPU stand-in with the device-side surface learn() and ScriptedOpponent use (as in test_space_host.py): it has no
    territory_out keyword, so selfplay must not pass one."""

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
            out[:, s] = {"safe_greedy": 2, "hamiltonian": 3, "space_greedy": 4, "territory_greedy": 1}[policy]
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


def test_selfplay_dispatches_territory_greedy_by_name(tmp_path):
    assert selfplay.SCRIPTED_POLICIES == ("safe_greedy", "hamiltonian", "space_greedy", "territory_greedy")
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "territory_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "space_greedy", 2, columns=team)
    env.reset_device()
    selfplay.refresh_scripted([o1, o2])
    assert sorted(env.scripted_calls) == [("space_greedy", (2,), 0), ("territory_greedy", (1,), 0)]
    assert o1.step()[0].tolist() == [1] * 8 and o2.step()[0].tolist() == [4] * 8
    assert selfplay.ScriptedOpponent(env, "territory_greedy", 2).step()[0].tolist() == [1] * 8   # a lone opponent asks itself
    with pytest.raises(ValueError):
        selfplay.ScriptedOpponent(env, "territory", 1)
    env2 = _FakeEnv()
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 2, nminibatches=2, noptepochs=1, opponent_save_interval=2, log_fn=None)
    selfplay.learn(env2, save_dir=str(tmp_path / "run"), scripted_opponents={1: "territory_greedy"}, **kw)
    assert env2.scripted_calls == [("territory_greedy", (1,), t) for t in range(8)]
    assert env2.last_actions[:, 1].tolist() == [1] * 8
    assert not any(f.startswith("opponent1_") for f in os.listdir(str(tmp_path / "run")))   # no pool for that slot


class _FakeLib:
    """Records the C calls of MultiSnakeVecEnv's scripted entry points."""

    def __init__(self):
        self.calls = []

    def msnake_territory_actions(self, *a):
        self.calls.append(("territory",) + a)
        return 0

    def msnake_space_actions(self, *a):
        self.calls.append(("space",) + a)
        return 0

    def msnake_scripted_actions(self, *a):
        self.calls.append(("scripted",) + a)
        return 0


def _bare_env(n=5, ns=3):
    """A MultiSnakeVecEnv with only what the scripted calls touch, on the CPU (as test_space_host.py builds it, plus the
    bound entry point of territory_greedy)."""
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env._scripted_fn, env._space_fn = lib.msnake_scripted_actions, lib.msnake_space_actions
    env._territory_fn = lib.msnake_territory_actions
    env._scripted_out = torch.zeros((n, ns), dtype=torch.int32)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    return env, lib


def test_vec_env_dispatches_by_name_and_checks_territory_out():
    env, lib = _bare_env()
    out = torch.zeros((5, 4), dtype=torch.int32)
    safe = torch.zeros((5, 3), dtype=torch.uint8)
    terr = torch.zeros((5, 3, 4), dtype=torch.uint16)
    assert env.scripted_actions_device("territory_greedy", snakes=[2, 0], out=out) is out
    assert lib.calls[-1] == ("territory", 1234, 0b101, out.data_ptr(), 4, None, None, 77)
    got = env.scripted_actions_device("territory_greedy", out=out, safe_out=safe, territory_out=terr)
    assert len(got) == 3 and got[0] is out and got[1] is safe and got[2] is terr
    assert lib.calls[-1] == ("territory", 1234, 0b111, out.data_ptr(), 4, safe.data_ptr(), terr.data_ptr(), 77)
    got = env.scripted_actions_device("territory_greedy", territory_out=terr)
    assert got[0] is env._scripted_out and got[1] is terr and lib.calls[-1][4] == 3
    got = env.scripted_actions_device("territory_greedy", out=out, safe_out=safe)
    assert len(got) == 2 and got[1] is safe
    # the counts alone
    assert env.territory_device(out=terr) is terr
    assert lib.calls[-1] == ("territory", 1234, 0, None, 0, None, terr.data_ptr(), 77)
    # the other policies go where they went
    env.scripted_actions_device("space_greedy", out=out, space_out=terr)
    assert lib.calls[-1][:3] == ("space", 1234, 0b111)
    env.scripted_actions_device("safe_greedy", out=out)
    assert lib.calls[-1][:4] == ("scripted", 1234, 1, 0b111)
    env.scripted_actions_device("hamiltonian", snakes=[1], out=out, safe_out=safe)
    assert lib.calls[-1][:4] == ("scripted", 1234, 2, 0b010)
    n_calls = len(lib.calls)
    # territory_out belongs to territory_greedy alone, space_out to space_greedy alone
    for pol in ("safe_greedy", "hamiltonian", "space_greedy", None):
        with pytest.raises(ValueError, match="territory_out"):
            env.scripted_actions_device(pol, out=out, safe_out=safe, territory_out=terr)
    with pytest.raises(ValueError, match="space_out"):
        env.scripted_actions_device("territory_greedy", out=out, space_out=terr)
    for bad in (torch.zeros((5, 3, 4), dtype=torch.int16), torch.zeros((5, 3), dtype=torch.uint16),
                torch.zeros((5, 4, 4), dtype=torch.uint16), torch.zeros((5, 3, 8), dtype=torch.uint16)[:, :, ::2]):
        with pytest.raises(ValueError, match="territory_out"):
            env.scripted_actions_device("territory_greedy", out=out, territory_out=bad)
        with pytest.raises(ValueError, match="territory_out"):
            env.territory_device(out=bad)
    with pytest.raises(ValueError, match="policy must be 'safe_greedy', 'hamiltonian' or None"):
        env.scripted_actions_device("territory")                   # the text for unknown names is the one it was
    with pytest.raises(ValueError):
        env.scripted_actions_device("territory_greedy", snakes=[3])
    assert len(lib.calls) == n_calls                                 # every refusal came before the C call


# ------------------------------------------------------------------------------------------ the tools
class _Parsed(Exception):
    pass


@pytest.mark.parametrize("tool,extra", [("train_selfplay", []), ("eval_vs_scripted", ["--random"])])
def test_the_tools_accept_the_new_opponent(tool, extra, monkeypatch):
    """Parse only: main() is stopped right behind parse_args, before it imports anything that wants a GPU."""
    spec = importlib.util.spec_from_file_location(f"_tool_{tool}", os.path.join(ROOT, "tools", f"{tool}.py"))
    mod = importlib.util.module_from_spec(spec)
    monkeypatch.setattr("sys.path", list(__import__("sys").path))   # (the tools put the repository root in front)
    spec.loader.exec_module(mod)
    real = argparse.ArgumentParser.parse_args
    seen = {}

    def parse_and_stop(self, args=None, namespace=None):
        seen["args"] = real(self, args, namespace)
        raise _Parsed()

    monkeypatch.setattr(argparse.ArgumentParser, "parse_args", parse_and_stop)
    monkeypatch.setattr("sys.argv", [tool, "--opponent", "territory_greedy"] + extra)
    with pytest.raises(_Parsed):
        mod.main()
    assert seen["args"].opponent == "territory_greedy"
    monkeypatch.setattr("sys.argv", [tool, "--opponent", "territory"] + extra)
    with pytest.raises(SystemExit):
        mod.main()
