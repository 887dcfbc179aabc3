"""msnake_generate_states on the CPU: the NumPy restatement of the header's text (tests/generate_play.py) against the
properties the header promises, the Python surface on stand-in envs, the learner's random starts, the header and the
bindings, and the kernel's register budget.  Nothing here needs a GPU."""
import ctypes
import functools
import os
import re
import types

import numpy as np
import pytest
import torch

import generate_play as gp
import msnake
import state_domain as sd
from fake_envs import FakeEnv, FakeLocalEnv
from kernel_resources import unit_resources
from msnake import _capi, selfplay
from oracle.snake_oracle import Oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CFGS = {"S6": (gp.make_cfg("snake_env", 6, 3, 48, seed=3, env_id_base=5), (10, 10, 10)),
        "A10": (gp.make_cfg("adversarial", 10, 3, 32, seed=4), gp.mixed_requests(32, np.random.default_rng(1))),
        "S19": (gp.make_cfg("snake_env", 19, 3, 8, seed=5), (40, 100, 200)),
        "S4": (gp.make_cfg("snake_env", 4, 3, 32, seed=6), (7, 7, 7))}      # a board the requests fill


@functools.lru_cache(maxsize=None)
def generated(key, compact):
    cfg, req = CFGS[key]
    return gp.np_generate(cfg, req, salt=11, compact=compact, ctr=(1 << 40) + 5, word3=2)


def cells_of(row, cfg):
    st = gp.row_state(row)
    return [tuple(f) for f in st["fruits"]], [[tuple(c) for c in b] for b in st["snakes"]], st


# ------------------------------------------------------------------------------------------ domain
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("key", list(CFGS))
def test_every_row_is_accepted_by_the_oracle_and_by_the_state_domain(key, compact):
    cfg, _ = CFGS[key]
    rows, count, _ = generated(key, compact)
    ora = Oracle(cfg["num_envs"], dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"], rules=cfg["rules"], seed=cfg["seed"])
    ora.reset()
    for e, row in enumerate(rows):
        assert sd.accepts(cfg, row) is None, (e, sd.accepts(cfg, row))
        assert sd.canonical_len(cfg, row) == len(row) == count[e]
        st = gp.row_state(row)
        ora.set_state(e, st)                                   # raises if the oracle refuses
        back = ora.get_state(e)
        assert back["snakes"] == st["snakes"] and back["fruits"] == st["fruits"] and back["ctr"] == st["ctr"] == (1 << 40) + 5


# ------------------------------------------------------------------------------------------ shape of a position
@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("key", list(CFGS))
def test_shape_of_a_position(key, compact):
    cfg, req = CFGS[key]
    dim, S = cfg["dim"], cfg["n_snakes"]
    rows, count, got = generated(key, compact)
    want = gp.lengths_array(cfg, req)
    for e, row in enumerate(rows):
        fruits, bodies, st = cells_of(row, cfg)
        assert [int(x) for x in row[:8]] == [0, 5, 1 << 8, 2, 0, 0, cfg["n_fruits"], S]
        assert [len(b) for b in bodies] == got[e].tolist()
        ask = np.maximum(want[e], 0)
        ask[0] = max(ask[0], 1)
        assert (got[e] <= ask).all() and got[e, 0] >= 1 and ((ask > 0) | (got[e] == 0)).all()
        used = [c for b in bodies for c in b]
        assert len(set(used)) == len(used) and all(0 <= x < dim and 0 <= y < dim for x, y in used)   # disjoint, in the grid
        for s, b in enumerate(bodies):
            assert all(abs(p[0] - q[0]) + abs(p[1] - q[1]) == 1 for p, q in zip(b, b[1:]))           # 4-adjacent
            v = (b[0][0] - b[1][0], b[0][1] - b[1][1]) if len(b) > 1 else (0, 0)
            assert tuple(st["vels"][s]) == v and st["grow_to"][s] == max(len(b), 3)
            assert st["alive"][s] is True and st["in_dead"][s] is False
        free = dim * dim - len(used)
        k = min(free, len(fruits))
        assert len(set(fruits[:k])) == k and not set(fruits[:k]) & set(used)                        # distinct, off the bodies
        assert all(f == (0, 0) for f in fruits[k:])                                                 # no cell left
        assert count[e] == 8 + 2 * len(fruits) + sum(6 + 2 * len(b) for b in bodies)


def test_requests_of_zero_below_zero_and_far_too_long():
    cfg, req = CFGS["A10"]
    rows, _, got = generated("A10", True)
    assert got[0].tolist()[0] == 1 and got[1].tolist()[:2] == [1, 0] and got[2].tolist() == [4, 0, 0]   # snake 0 is raised to 1
    assert got[3, 0] <= 100 and got[4, 2] == 0 and max(got[3, 0], got[4, 1], got[5, 2]) > 40            # 1 000 ends where the walk does


# ------------------------------------------------------------------------------------------ determinism
def test_rows_depend_on_salt_and_global_id_only():
    cfg = gp.make_cfg("snake_env", 8, 3, 64, seed=9, env_id_base=3)
    req = (9, 6, 3)
    a = gp.np_generate(cfg, req, salt=5)
    b = gp.np_generate(cfg, req, salt=5)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[2], b[2])
    c = gp.np_generate(cfg, req, salt=6)
    changed = sum(not np.array_equal(x, y) for x, y in zip(a[0], c[0]))
    assert changed >= 0.9 * 64, changed
    d = gp.np_generate(dict(cfg, seed=10), req, salt=5)
    assert sum(not np.array_equal(x, y) for x, y in zip(a[0], d[0])) >= 0.9 * 64
    k = 40
    shard = gp.np_generate(dict(cfg, env_id_base=3 + k, num_envs=64 - k), req, salt=5)
    assert all(np.array_equal(x, y) for x, y in zip(shard[0], a[0][k:])) and np.array_equal(shard[2], a[2][k:])
    # a mask selects rows and changes none of them
    mask = np.arange(64) % 3 == 0
    m = gp.np_generate(cfg, req, mask=mask, salt=5)
    assert all((r is None) if not sel else np.array_equal(r, x) for r, x, sel in zip(m[0], a[0], mask))
    assert (m[1][~mask] == -1).all() and (m[2][~mask] == -1).all()


def test_the_generator_key_and_the_draw_formula():
    from msnake.vec_env import mix64 as np_mix64                        # (the hashes' finaliser, pinned by their known answers)
    probe = [0, 1, 7, gp.GEN_TAG, gp.M64, 0x9E3779B97F4A7C15]
    assert [gp.mix64(z) for z in probe] == np_mix64(np.array(probe, np.uint64)).tolist() and gp.mix64(0) == 0
    assert gp.GEN_TAG == int.from_bytes(b"generate", "big")
    assert gp.gen_seed(7, 3) == gp.mix64(7 ^ gp.mix64(3 ^ gp.GEN_TAG))
    from oracle.snake_oracle import philox_u32
    cfg = gp.make_cfg("snake_env", 5, 1, 1, seed=7, env_id_base=12)
    rows, _, _ = gp.np_generate(cfg, 1, salt=3)
    head = int(philox_u32(gp.gen_seed(7, 3), 12, 0)) * 25 >> 32         # draw 0: the head among 25 free cells
    assert [int(x) for x in rows[0][-2:]] == [head % 5, head // 5]


# ------------------------------------------------------------------------------------------ reached lengths
def test_compact_reaches_the_requested_lengths():
    cfg = gp.make_cfg("snake_env", 19, 3, 256, seed=1)
    with_c, without = gp.reach_share(cfg, (40, 40, 40), True), gp.reach_share(cfg, (40, 40, 40), False)
    print("share of snakes that reach 40 on 19x19x3: compact", with_c, "plain", without)
    assert with_c >= 0.85 and with_c >= without + 0.3, (with_c, without)


# ------------------------------------------------------------------------------------------ full boards
def test_a_full_board_leaves_nothing_for_the_second_snake_and_the_fruits():
    cfg, req = gp.cases()["full3x3"]
    draws = []
    rows, count, got = gp.np_generate(cfg, req, salt=1, compact=True, draws_out=draws)
    full = [e for e in range(cfg["num_envs"]) if got[e, 0] == 9]
    # (a path over all nine cells starts on the colour with five of them, so at most 5 heads in 9 can fill the board)
    assert 1 <= len(full) < cfg["num_envs"], got[:, 0].tolist()
    for e in set(range(cfg["num_envs"])) - set(full):                     # one cell short: it is the second snake's, the fruits get none
        fruits, bodies, _ = cells_of(rows[e], cfg)
        assert got[e].tolist() == [8, 1] and fruits == [(0, 0), (0, 0)] and not set(bodies[1]) & set(bodies[0])
    for e in full:
        fruits, bodies, _ = cells_of(rows[e], cfg)
        assert got[e, 1] == 0 and bodies[1] == [] and fruits == [(0, 0), (0, 0)]
        assert count[e] == 8 + 4 + 6 + 18 + 6
        assert draws[e] <= 1 + 8                                          # the head and at most one per piece: none for snake 1, none for a fruit
    # the same env without the second snake's request and without fruits to place takes the same draws
    for e in full[:3]:
        alone = []
        one = dict(cfg, n_snakes=1, n_fruits=0, num_envs=1, env_id_base=cfg["env_id_base"] + e)
        gp.np_generate(one, 9, salt=1, compact=True, draws_out=alone)
        assert alone == [draws[e]]


def test_two_by_two_with_request_four():
    cfg, req = gp.cases()["full2x2"]
    rows, count, got = gp.np_generate(cfg, req, salt=2, compact=True)
    assert (got[:, 0] == 4).all()                                         # a 2x2 board is a cycle: the walk cannot get stuck
    for row in rows:
        fruits, bodies, _ = cells_of(row, cfg)
        assert sorted(bodies[0]) == [(0, 0), (0, 1), (1, 0), (1, 1)] and fruits == [(0, 0)]
    assert len({tuple(r.tolist()) for r in rows}) > 1


# ------------------------------------------------------------------------------------------ the Python surface
class _FakeLib:
    def __init__(self):
        self.calls = []

    def msnake_state_words_max(self, h):
        return 99

    def msnake_generate_states(self, *a):
        self.calls.append(("generate",) + a)
        return 0

    def msnake_import_states(self, *a):
        self.calls.append(("import",) + a)
        return 0


def _bare_env(n=5, ns=3, rules=0):
    env = object.__new__(msnake.MultiSnakeVecEnv)
    lib = _FakeLib()
    env._torch, env._L, env._h = torch, lib, 1234
    env.num_envs, env.n_snakes, env.device = n, ns, torch.device("cpu")
    env.cfg = types.SimpleNamespace(dim=10, rules=rules)
    env._cur_stream = lambda dev: type("S", (), {"cuda_stream": 77})()
    env._pending, env._track_stale, env._scatter_own = None, False, None
    return env, lib


def test_generate_states_device_passes_what_the_header_asks_for():
    env, lib = _bare_env()
    words, count, got = env.generate_states_device(7)
    assert tuple(words.shape) == (5, 99) and tuple(count.shape) == (5,) and tuple(got.shape) == (5, 3)
    assert words.dtype == count.dtype == got.dtype == torch.int32
    name, h, mask, plen, lstride, flags, salt, pw, stride, pc, pg, stream = lib.calls[-1]
    assert (name, h, mask, lstride, flags, salt, pw, stride, pc, pg, stream) == \
        ("generate", 1234, None, 3, _capi.GEN_COMPACT, 0, words.data_ptr(), 99, count.data_ptr(), got.data_ptr(), 77)
    assert _capi.GEN_COMPACT == 1
    lengths = torch.arange(20, dtype=torch.int32).view(5, 4)
    out = torch.zeros((5, 40), dtype=torch.int32)
    mask = torch.tensor([1, 0, 0, 1, 0], dtype=torch.uint8)
    w2, c2, g2 = env.generate_states_device(lengths, mask=mask, salt=2 ** 64 - 1, compact=False, out=out, count_out=count, got_out=got)
    assert w2 is out and c2 is count and g2 is got
    assert lib.calls[-1][2:9] == (mask.data_ptr(), lengths.data_ptr(), 4, 0, 2 ** 64 - 1, out.data_ptr(), 40)
    env.generate_states_device((3, 0, -2), mask=[0, 4])
    assert lib.calls[-1][4] == 3 and lib.calls[-1][2] is not None


def test_generate_states_device_builds_the_lengths_tensor():
    env, _ = _bare_env()
    assert env._gen_lengths(4).tolist() == [[4, 4, 4]] * 5
    assert env._gen_lengths((3, 0, -2)).tolist() == [[3, 0, -2]] * 5
    assert env._gen_lengths(np.array([1, 2, 3])).dtype == torch.int32


def test_argument_checks_raise_before_the_c_call():
    env, lib = _bare_env()
    i32 = torch.int32
    for bad in ((1, 2), (1, 2, 3, 4), "long", None, 2.5, True, (1.5, 2, 3), 2 ** 31, torch.zeros((5, 2), dtype=i32),
                torch.zeros((4, 3), dtype=i32), torch.zeros((5, 3), dtype=torch.int64), torch.zeros((3, 5), dtype=i32).t()):
        with pytest.raises(ValueError, match="lengths"):
            env.generate_states_device(bad)
    for bad in (-1, 2 ** 64, 1.0, True, "3"):
        with pytest.raises(ValueError, match="salt"):
            env.generate_states_device(3, salt=bad)
    with pytest.raises(ValueError, match="mask"):
        env.generate_states_device(3, mask=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="out must be a contiguous int32"):
        env.generate_states_device(3, out=torch.zeros((5, 40), dtype=torch.int64))
    with pytest.raises(ValueError, match="count_out must be"):
        env.generate_states_device(3, count_out=torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="got_out must be"):
        env.generate_states_device(3, got_out=torch.zeros((5, 4), dtype=i32))
    nw, nwlib = _bare_env(rules=_capi.RULES["new_world"])
    for call in (nw.generate_states_device, nw.scatter_device):
        with pytest.raises(ValueError, match="new_world"):
            call(3)
    env._pending = (None,) * 4
    with pytest.raises(RuntimeError, match="between step_async"):
        env.scatter_device(3)
    assert lib.calls == [] and nwlib.calls == [] and env._track_stale is False


def test_scatter_device_is_generate_then_import_with_the_same_mask_and_count():
    env, lib = _bare_env()
    mask = torch.tensor([0, 1, 1, 0, 1], dtype=torch.uint8)
    status, got = env.scatter_device((5, 4, 3), mask=mask, salt=9, compact=False)
    gen, imp = lib.calls
    words, count, got_own, status_own = env._scatter_own
    assert status is status_own and got is got_own and status.dtype == torch.uint8 and tuple(words.shape) == (5, 99)
    assert gen[:3] == ("generate", 1234, mask.data_ptr()) and gen[5:] == (0, 9, words.data_ptr(), 99, count.data_ptr(), got.data_ptr(), 77)
    assert imp == ("import", 1234, mask.data_ptr(), words.data_ptr(), 99, count.data_ptr(), status.data_ptr(), 77)
    assert env._track_stale is True                               # an install: the outcome tracker is armed again
    env.scatter_device(3)                                         # every env, the buffers kept
    gen, imp = lib.calls[2:]
    assert gen[2] is None and imp[2] is None and gen[7] == words.data_ptr() and gen[5] == _capi.GEN_COMPACT


# ------------------------------------------------------------------------------------------ the learner
class _Starts:
    """What the runner's random starts ask of an env, recorded."""

    def _init_starts(self):
        self.scatters, self.frames, self.last_done = [], 0, None

    def scatter_device(self, lengths, mask=None, salt=0, compact=True):
        assert lengths.dtype == torch.int32 and tuple(lengths.shape) == (self.num_envs, self.n_snakes)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (self.num_envs,)
        assert not (mask & ~self.last_done.bool()).any()          # a subset of the step's done
        assert compact is False                                   # the learner wants heads with room, not full lengths
        self.scatters.append((lengths.clone(), mask.clone(), salt, self.last_done.clone()))
        return torch.zeros(self.num_envs, dtype=torch.uint8), lengths


class _FrameEnv(_Starts, FakeEnv):
    def __init__(self, **kw):
        FakeEnv.__init__(self, **kw)
        self._init_starts()

    def step_device(self, actions):
        out = FakeEnv.step_device(self, actions)
        self.last_done = out[2]
        return out

    def render_device(self):
        self.frames += 1
        return torch.full((self.num_envs,) + self.obs_shape, 200 + self.frames % 50, dtype=torch.uint8)


class _WindowEnv(_Starts, FakeLocalEnv):
    def __init__(self, **kw):
        FakeLocalEnv.__init__(self, **kw)
        self._init_starts()
        self.log = []

    def step_device(self, actions):
        out = FakeLocalEnv.step_device(self, actions)
        self.last_done = out[2]
        self.log.append("step")
        return out

    def scatter_device(self, *a, **kw):
        self.log.append("scatter")
        return _Starts.scatter_device(self, *a, **kw)

    def render_local_device(self, *a, **kw):
        self.log.append("observe")
        return FakeLocalEnv.render_local_device(self, *a, **kw)


def test_frame_runner_scatters_a_subset_of_done_and_renders_again():
    torch.manual_seed(0)
    env = _FrameEnv(n=8, n_snakes=2, seed=1)
    model = selfplay.CnnPolicy((12, 12, 3))
    run = selfplay.Runner(env, model, [None], 6, 0.99, 0.95, random_starts=1.0, start_lengths=(4, 9))
    obs = run.run()[0]
    assert len(env.scatters) == 6 and env.frames == 6
    assert [s[2] for s in env.scatters] == [1, 2, 3, 4, 5, 6]                     # the salt moves with every call
    for lengths, mask, _, done in env.scatters:
        assert torch.equal(mask, done.bool()) and 4 <= int(lengths.min()) and int(lengths.max()) <= 9   # p = 1: every done env
    assert any(m.any() for _, m, _, _ in env.scatters)
    assert int(run.obs[0, 0, 0, 0]) == 200 + 6                                    # the next observation is the re-rendered frame
    assert int(obs.view(8, 6, 12, 12, 3)[0, 1, 0, 0, 0]) == 201                   # ... and step 1's sample saw the one before
    half = _FrameEnv(n=64, n_snakes=2, seed=1)
    selfplay.Runner(half, model, [None], 8, 0.99, 0.95, random_starts=0.5).run()
    picked, done = sum(int(m.sum()) for _, m, _, _ in half.scatters), sum(int(d.sum()) for _, _, _, d in half.scatters)
    assert 0.3 * done < picked < 0.7 * done and int(half.scatters[0][0].min()) == int(half.scatters[0][0].max()) == 3


def test_window_runner_scatters_before_it_reads_the_windows():
    torch.manual_seed(0)
    env = _WindowEnv(n=8, n_snakes=3, seed=2)
    model = selfplay.WindowPolicy(2)
    run = selfplay.Runner(env, model, [None, None], 4, 0.99, 0.95, local_radius=2, random_starts=1.0, start_lengths=(5, 5))
    run.run()
    assert env.log == ["observe"] + ["step", "scatter", "observe"] * 4 and env.frames == 0


def test_without_random_starts_the_rollout_is_what_it_was():
    outs = []
    for kw in ({}, dict(random_starts=0.0, start_lengths=(7, 30))):
        torch.manual_seed(3)
        env = _FrameEnv(n=8, n_snakes=2, seed=1)
        model = selfplay.CnnPolicy((12, 12, 3))
        outs.append(selfplay.Runner(env, model, [None], 5, 0.99, 0.95, **kw).run()[:6])
        assert env.scatters == [] and env.frames == 0
    assert all(torch.equal(a, b) for a, b in zip(*outs))


@pytest.mark.parametrize("kw", [dict(random_starts=1.5), dict(random_starts=-0.1), dict(random_starts=0.5, start_lengths=(5, 4)),
                                dict(random_starts=0.5, start_lengths=(-1, 4)), dict(random_starts=0.5, start_lengths=(3,)),
                                dict(random_starts=0.5, start_lengths=(2.5, 4))])
def test_random_start_arguments_are_checked(kw):
    with pytest.raises(ValueError, match="random_starts|start_lengths"):
        selfplay.Runner(_FrameEnv(), selfplay.CnnPolicy((12, 12, 3)), [None], 4, 0.99, 0.95, **kw)
    with pytest.raises(ValueError, match="random_starts|start_lengths"):
        selfplay.learn(_FrameEnv(), nsteps=4, total_timesteps=32, **kw)


def test_learn_forwards_random_starts():
    torch.manual_seed(0)
    env = _FrameEnv(n=8, n_snakes=2, seed=1)
    selfplay.learn(env, nsteps=4, total_timesteps=64, nminibatches=4, noptepochs=1, log_fn=lambda *a: None, random_starts=1.0,
                   start_lengths=(2, 6))
    assert len(env.scatters) == 8 and all(2 <= int(s[0].min()) and int(s[0].max()) <= 6 for s in env.scatters)


def test_the_trainer_tool_names_the_two_options():
    text = open(os.path.join(ROOT, "tools", "train_selfplay.py")).read()
    assert '"--random-starts"' in text and '"--start-lengths"' in text and "random_starts=args.random_starts" in text


# ------------------------------------------------------------------------------------------ header and bindings
PROTO = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p,
                        ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])


def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    assert re.search(r"int msnake_generate_states\(msnake_handle h, const uint8_t\* mask_dev, const int32_t\* len_dev, int32_t len_stride,\s+"
                     r"uint32_t flags, uint64_t salt, int32_t\* words_dev, int32_t stride, int32_t\* count_dev,\s+"
                     r"int32_t\* got_dev, void\* stream\);", text)
    assert re.search(r"#define MSNAKE_GEN_COMPACT 1u", text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text) and _capi.ABI_VERSION == 3      # additive: the ABI version stays
    assert re.search(r"^ \*   msnake_generate_states: no reference counterpart", text, re.M)
    assert "msnake_generate_states" in _capi.SYMBOLS
    lib = _capi.load()
    assert lib.msnake_abi_version() == 3
    fn = lib.msnake_generate_states
    assert fn.restype is PROTO[0] and list(fn.argtypes) == PROTO[1]


def test_null_handles_are_refused():
    lib = _capi.load()
    dead, buf = ctypes.create_string_buffer(4), ctypes.create_string_buffer(64)
    for h in (None, dead):
        assert lib.msnake_generate_states(h, None, buf, 3, 1, 0, buf, 16, buf, buf, None) == -3      # MSNAKE_E_HANDLE
        assert b"handle" in lib.msnake_last_error()


def test_methods_exist_on_the_env_class():
    cls = msnake.MultiSnakeVecEnv
    assert callable(cls.generate_states_device) and callable(cls.scatter_device)


# ------------------------------------------------------------------------------------------ the kernel's budget
def test_the_generate_kernel_spills_nothing():
    table, asm = unit_resources("msnake_views")
    mine = {k: v for k, v in table.items() if "msnake_generate_kernel" in k}
    assert len(mine) == 1, sorted(mine)
    for name, r in mine.items():
        print(name, "VGPRs", r["VGPRs"], "SGPRs", r["TotalSGPRs"])
        assert r["SGPRs Spill"] == 0 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["VGPRs"] <= 64, (name, r)


def test_an_int_or_sequence_of_lengths_is_copied_once_and_kept():
    env, lib = _bare_env()
    a = env._gen_lengths((4, 5, 6))
    assert env._gen_lengths([4, 5, 6]) is a and env._gen_lengths(np.array([4, 5, 6])) is a      # the same request: the kept tensor
    b = env._gen_lengths(4)
    assert b is not a and b.tolist() == [[4, 4, 4]] * 5 and env._gen_lengths((4, 4, 4)) is b
    env.generate_states_device(4)
    assert lib.calls[-1][3] == b.data_ptr()
    given = torch.zeros((5, 3), dtype=torch.int32)
    assert env._gen_lengths(given) is given and env._gen_lengths(4) is b                       # a tensor is used as it is, nothing kept of it


def test_new_world_random_starts_are_refused_when_the_runner_is_built():
    env = _FrameEnv()
    env.cfg = types.SimpleNamespace(rules=_capi.RULES["new_world"])
    model = selfplay.CnnPolicy((12, 12, 3))
    with pytest.raises(ValueError, match="new_world"):
        selfplay.Runner(env, model, [None], 4, 0.99, 0.95, random_starts=0.5)
    with pytest.raises(ValueError, match="new_world"):
        selfplay.learn(env, nsteps=4, total_timesteps=32, random_starts=0.5)
    assert env.scatters == []
    selfplay.Runner(env, model, [None], 4, 0.99, 0.95)                                          # without random starts new_world is fine
    env.cfg = types.SimpleNamespace(rules=_capi.RULES["adversarial"])
    selfplay.Runner(env, model, [None], 4, 0.99, 0.95, random_starts=0.5)
