"""CPU-side checks of the on-device scripted opponents (msnake_scripted_actions, MultiSnakeVecEnv.scripted_actions_device,
selfplay.ScriptedOpponent): the entry point is declared, exported and refuses a NULL handle before it touches the GPU;
the self-play plumbing on a fake env; the safe-move mask, stated here in NumPy, against tests/scripted_play.py's
safe_greedy over an oracle play; the register budget of the new kernel.  No GPU: hipcc cross-compiles, nothing runs."""
import os
import re

import numpy as np
import pytest
import torch

import msnake
import scripted_play as sp
from kernel_resources import unit_resources
from msnake import selfplay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    assert re.search(r"\bint msnake_scripted_actions\(msnake_handle h, int32_t policy, uint32_t snake_mask,", text)
    for name, val in (("NONE", 0), ("SAFE_GREEDY", 1), ("HAMILTONIAN", 2)):
        assert re.search(rf"#define MSNAKE_POLICY_{name} {val}\b", text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_scripted_actions" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_scripted_actions is not None and lib.msnake_abi_version() == 3


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_scripted_actions(None, 1, 1, None, 3, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ the mask, in NumPy
def np_safe_mask(st, dim, n_snakes):
    """Bit a (1..4) of entry s: the target of move a of snake s lies on the board and in no body; 0 for an empty body."""
    occ = np.zeros((dim, dim), bool)
    for body in st["snakes"]:
        for c0, c1 in body:
            if 0 <= c0 < dim and 0 <= c1 < dim:
                occ[c0, c1] = True
    out = np.zeros(n_snakes, np.uint8)
    for s in range(n_snakes):
        body = st["snakes"][s] if s < len(st["snakes"]) else []
        if not body:
            continue
        for a, (d0, d1) in sp.DIRS.items():
            x, y = body[0][0] + d0, body[0][1] + d1
            if 0 <= x < dim and 0 <= y < dim and not occ[x, y]:
                out[s] |= 1 << a
    return out


@pytest.mark.parametrize("name,steps", [("S19x3", 400), ("N10x4", 400), ("A10x3", 400)])
def test_numpy_mask_is_consistent_with_safe_greedy_over_an_oracle_play(name, steps):
    cfg = dict(sp.SCENARIOS[name], eps=0.0, num_envs=4, steps=steps)
    ora = sp.make_oracle(cfg)
    read = sp._StateReader(ora)
    ora.reset()
    seen_zero = seen_move = 0
    for _ in range(steps):
        states = [read(e) for e in range(cfg["num_envs"])]
        act = sp.choose_actions(cfg, states, [None] * len(states))
        for st, row in zip(states, act):
            m = np_safe_mask(st, cfg["dim"], cfg["n_snakes"])
            assert not (m & 0xE1).any()
            for s in range(cfg["n_snakes"]):
                if row[s] != 0:
                    assert m[s] >> row[s] & 1, (st, s, row)
                    seen_move += 1
                else:
                    assert m[s] == 0, (st, s, row)  # 0 <=> no open move (or an empty body, whose mask is 0 too)
                    seen_zero += 1
        ora.step(act)
    assert seen_move > steps and seen_zero > 0


def test_hamiltonian_closed_form_is_the_table():
    """The closed form the header states (and the kernel computes) against scripted_play.hamiltonian_table."""
    def closed(x, y, dim):
        if x == 0:
            return 4 if y > 0 else 1
        if y % 2 == 0:
            return 1 if x < dim - 1 else 2
        if y == dim - 1:
            return 3
        return 3 if x > 1 else 2
    for dim in (2, 4, 6, 10, 20, 62):
        tab = sp.hamiltonian_table(dim)
        assert all(tab[x][y] == closed(x, y, dim) for x in range(dim) for y in range(dim))


# ------------------------------------------------------------------------------------------ self-play plumbing
class _FakeEnv:
    """CPU stand-in with the device-side surface learn() and ScriptedOpponent use."""

    def __init__(self, n=8, n_snakes=3, seed=0):
        self.num_envs, self.n_snakes, self.obs_shape, self.device = n, n_snakes, (12, 12, 9), torch.device("cpu")
        self.g = torch.Generator().manual_seed(seed)
        self.len = torch.zeros(n, dtype=torch.int32)
        self.scripted_calls, self.steps, self.last_actions = [], 0, None

    def reset_device(self):
        return torch.randint(0, 256, (self.num_envs,) + self.obs_shape, dtype=torch.uint8, generator=self.g)

    def scripted_actions_device(self, policy, snakes=None, out=None, safe_out=None):
        self.scripted_calls.append((policy, tuple(snakes), self.steps))
        if out is None:
            out = torch.zeros((self.num_envs, self.n_snakes), dtype=torch.int32)
        for s in snakes:
            out[:, s] = {"safe_greedy": 2, "hamiltonian": 3}[policy] + (self.steps % 2)
        return out

    def step_device(self, actions):
        assert actions.shape == (self.num_envs, self.n_snakes) and actions.dtype == torch.int32
        self.steps += 1
        self.last_actions = actions.clone()
        self.len += 1
        done = (torch.rand(self.num_envs, generator=self.g) < 0.3)
        rew = torch.randint(0, 2, (self.num_envs,), generator=self.g).float()
        info = torch.zeros((self.num_envs, 4), dtype=torch.int32)
        info[:, 0] = torch.full((self.num_envs,), 7.0).view(torch.int32)
        info[:, 1] = self.len
        self.len = torch.where(done, torch.zeros_like(self.len), self.len)
        obs = torch.randint(0, 256, (self.num_envs,) + self.obs_shape, dtype=torch.uint8, generator=self.g)
        return obs, rew, done.to(torch.uint8), info


def test_a_team_of_scripted_opponents_costs_one_env_call_per_step():
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "safe_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "safe_greedy", 2, columns=team)
    with pytest.raises(RuntimeError):
        o1.step()                              # a team member reads; the driver has not asked the env yet
    model = selfplay.CnnPolicy((12, 12, 3))
    runner = selfplay.Runner(env, model, [o1, o2], nsteps=5, gamma=0.99, lam=0.95)
    runner.run()
    assert env.scripted_calls == [("safe_greedy", (1, 2), t) for t in range(5)]
    assert env.last_actions[:, 1].tolist() == [2] * 8 and env.last_actions[:, 2].tolist() == [2] * 8  # (step 4: 2 + 0)
    a = o1.step(None)[0]
    assert a.dtype == torch.int64 and a.shape == (8,) and len(env.scripted_calls) == 5   # read, not recomputed
    team.refresh()
    assert len(env.scripted_calls) == 6 and o2.step()[0].tolist() == [3] * 8             # (5 steps: 2 + 1)
    # the team's buffer is its own: a direct call of the user's on the env does not reach it
    env.scripted_actions_device("hamiltonian", snakes=[1, 2])
    assert o1.step()[0].tolist() == [3] * 8
    # nothing is left on the env, and a second team does not launch for the first one's members
    assert not any("script" in k and k != "scripted_calls" for k in vars(env))
    team2 = selfplay.ScriptedColumns(env)
    selfplay.ScriptedOpponent(env, "hamiltonian", 1, columns=team2)
    env.scripted_calls.clear()
    team2.refresh()
    assert env.scripted_calls == [("hamiltonian", (1,), 5)]
    with pytest.raises(ValueError):
        selfplay.ScriptedOpponent(env, "safe_greedy", 1, columns=team2)   # one opponent per snake and team


def test_different_policies_take_one_call_each_and_lone_opponents_ask_themselves():
    env = _FakeEnv()
    team = selfplay.ScriptedColumns(env)
    o1 = selfplay.ScriptedOpponent(env, "safe_greedy", 1, columns=team)
    o2 = selfplay.ScriptedOpponent(env, "hamiltonian", 2, columns=team)
    env.reset_device()
    selfplay.refresh_scripted([o1, None, o2])
    assert o1.step()[0].tolist() == [2] * 8 and o2.step()[0].tolist() == [3] * 8
    assert sorted(env.scripted_calls) == [("hamiltonian", (2,), 0), ("safe_greedy", (1,), 0)]
    lone = selfplay.ScriptedOpponent(env, "hamiltonian", 1)
    env.scripted_calls.clear()
    assert lone.step()[0].tolist() == [3] * 8 and lone.step()[0].tolist() == [3] * 8
    assert env.scripted_calls == [("hamiltonian", (1,), 0)] * 2


def test_eps_mix_uses_the_given_generator_only():
    env = _FakeEnv(n=4096)
    env.reset_device()
    opp = selfplay.ScriptedOpponent(env, "safe_greedy", 1, eps=0.25, generator=torch.Generator().manual_seed(5))
    torch.manual_seed(0)
    before = torch.random.get_rng_state()
    a = opp.step()[0]
    assert torch.equal(torch.random.get_rng_state(), before)   # the global generator is not drawn from
    g = torch.Generator().manual_seed(5)
    swap = torch.rand((4096,), generator=g) < 0.25
    rnd = torch.randint(0, 5, (4096,), generator=g)
    assert torch.equal(a, torch.where(swap, rnd, torch.full((4096,), 2)))
    assert 0.2 < float(swap.float().mean()) < 0.3 and set(a.tolist()) == {0, 1, 2, 3, 4}
    assert selfplay.ScriptedOpponent(env, "safe_greedy", 2).step()[0].tolist() == [2] * 4096  # eps = 0: untouched


def test_scripted_opponent_rejects_bad_arguments():
    env = _FakeEnv()
    with pytest.raises(ValueError):
        selfplay.ScriptedOpponent(env, "random", 1)
    with pytest.raises(ValueError):
        selfplay.ScriptedOpponent(env, "safe_greedy", 3)
    with pytest.raises(ValueError):
        selfplay.learn(env, scripted_opponents={0: "safe_greedy"}, log_fn=None)


def test_learn_with_scripted_opponents_keeps_no_pool_for_them(tmp_path):
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 4, nminibatches=2, noptepochs=1, opponent_save_interval=2, log_fn=None)
    d = str(tmp_path / "mixed")
    env = _FakeEnv()
    _, hist = selfplay.learn(env, save_dir=d, scripted_opponents={2: "hamiltonian"}, **kw)
    files = set(os.listdir(d))
    assert "opponent1_0.pt" in files and not any(f.startswith("opponent2_") for f in files)
    assert {c[:2] for c in env.scripted_calls} == {("hamiltonian", (2,))} and len(env.scripted_calls) == 16
    assert env.last_actions[:, 2].tolist() == [4] * 8    # (the last fill saw 15 steps: 3 + 1)
    ts = torch.load(os.path.join(d, "trainer_state.pt"), weights_only=True)
    assert ts["pools"] == [(3, 3)] and hist[-1]["num_opponents"] == 3
    # resume reads the same file back
    _, hist2 = selfplay.learn(_FakeEnv(seed=1), save_dir=d, resume=True, scripted_opponents={2: "hamiltonian"},
                              **dict(kw, total_timesteps=8 * 4 * 6))
    assert [h["nupdates"] for h in hist2] == [5, 6]
    # ... but not under another set of scripted opponents: the pools would land in the wrong slots
    for other in (None, {1: "safe_greedy"}, {1: "safe_greedy", 2: "hamiltonian"}):
        with pytest.raises(RuntimeError, match="scripted_opponents"):
            selfplay.learn(_FakeEnv(seed=1), save_dir=d, resume=True, scripted_opponents=other, **dict(kw, total_timesteps=8 * 4 * 7))

    d2 = str(tmp_path / "all_scripted")
    env2 = _FakeEnv()
    _, hist3 = selfplay.learn(env2, save_dir=d2, scripted_opponents={1: "safe_greedy", 2: "safe_greedy"}, **kw)
    assert not any(f.startswith("opponent") for f in os.listdir(d2)) and "num_opponents" not in hist3[-1]
    assert env2.scripted_calls == [("safe_greedy", (1, 2), t) for t in range(16)]
    assert torch.load(os.path.join(d2, "trainer_state.pt"), weights_only=True)["pools"] == []


def test_default_arguments_reproduce_the_pool_only_run(tmp_path):
    """scripted_opponents=None (and {}) is the run learn() gave before the argument existed: same opponents, same pool
    files, same random streams, hence the same weights; the env is never asked for scripted actions."""
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 3, nminibatches=2, noptepochs=1, opponent_save_interval=2, log_fn=None)
    runs = []
    for i, extra in enumerate(({}, {"scripted_opponents": None}, {"scripted_opponents": {}})):
        env = _FakeEnv()
        d = str(tmp_path / f"run{i}")
        model, hist = selfplay.learn(env, save_dir=d, **kw, **extra)
        assert env.scripted_calls == [] and env.steps == 12
        assert {f for f in os.listdir(d) if f.startswith("opponent")} == {"opponent1_0.pt", "opponent1_1.pt", "opponent2_0.pt",
                                                                           "opponent2_1.pt"}
        ts = torch.load(os.path.join(d, "trainer_state.pt"), weights_only=True)
        assert ts["pools"] == [(2, 2), (2, 2)] and hist[-1]["num_opponents"] == 2
        runs.append(([v.clone() for v in model.state_dict().values()], env.last_actions))
    for w, acts in runs[1:]:
        assert torch.equal(acts, runs[0][1]) and all(torch.equal(a, b) for a, b in zip(w, runs[0][0]))


# ------------------------------------------------------------------------------------------ register budget
def test_scripted_kernels_do_not_spill():
    """Every instantiation of msnake_scripted_kernel<POLICY, SAFE> spills no register and uses no scratch."""
    res, _ = unit_resources("msnake_opponents")
    seen = set()
    for name, rr in res.items():
        m = re.match(r"_ZN6msnake22msnake_scripted_kernelILi(\d)ELb([01])EEE", name)
        if not m:
            continue
        seen.add(m.groups())
        assert rr["SGPRs Spill"] == 0 and rr["VGPRs Spill"] == 0 and rr["ScratchSize [bytes/lane]"] == 0, (m.groups(), rr)
        # the figures DESIGN.md quotes (45 / 45 / 12 / 35 / 39 VGPRs): all within 64, i.e. 8 waves per SIMD
        assert rr["VGPRs"] <= {("1", "0"): 45, ("1", "1"): 45, ("2", "0"): 12, ("2", "1"): 35, ("0", "1"): 39}[m.groups()], rr
    # safe_greedy and hamiltonian with and without the mask, and the mask alone
    assert seen == {("1", "0"), ("1", "1"), ("2", "0"), ("2", "1"), ("0", "1")}, sorted(seen)
