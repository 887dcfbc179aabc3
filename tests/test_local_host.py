"""CPU-side checks of the head-centred windows (msnake_render_local, MultiSnakeVecEnv.render_local_device): the entry
point is declared, exported and refuses a NULL handle before it touches the GPU; the two statements of the window in
tests/local_play.py agree on states with every velocity dealt; relative actions mean what the header says, in the
window and on the oracle; the wrapper's normalisation of `snakes`; WindowPolicy and the refusal of weights of the other
kind.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import cells_play as cp
from fake_envs import FakeEnv, FakeLocalEnv as _FakeLocalEnv
import local_play as lp
import msnake
import scripted_play as sp
from msnake import selfplay, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RADII = (1, 2, 5, 31)


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_render_local\(msnake_handle h, int32_t radius, uint32_t snake_mask, int32_t oriented,\s*"
           r"uint8_t\* windows_dev,\s*uint8_t\* heading_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_LOCAL_MAX_RADIUS 31\b", text) and re.search(r"#define MSNAKE_CELL_OUTSIDE 6\b", text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    contract = text.split("int msnake_render_local(")[0].rsplit("/*", 2)[1]
    assert "((r - 1 + k) mod 4) + 1" in contract and "MSNAKE_E_ARG" in contract
    assert "msnake_render_local" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_render_local is not None and lib.msnake_abi_version() == 3
    assert vec_env.LOCAL_MAX_RADIUS == 31 and vec_env.CELL_OUTSIDE == lp.OUTSIDE == 6


def test_null_and_destroyed_handles_are_refused():
    lib = msnake._capi.load()
    assert lib.msnake_render_local(None, 5, 1, 1, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    dead = ctypes.create_string_buffer(4)       # what a destroyed handle looks like: the magic word is gone
    for radius, mask, oriented in ((5, 1, 1), (0, 1, 1), (5, 0, 1), (5, 1, 2)):   # the handle check comes first
        assert lib.msnake_render_local(dead, radius, mask, oriented, None, None, None) == -3
        assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ the helper by hand
def test_np_local_on_a_hand_computed_3x3():
    st = {"fruits": [[2, 2]], "snakes": [[[1, 0], [0, 0]], [[1, 1]], []], "alive": [True] * 3, "vels": [[0, 1], [-1, 0], [1, 0]]}
    # snake 0 at (1, 0) moves along +c1: f = (0, 1), g = (-1, 0); row i = cells (1 + r - j, i - r)
    win, k = lp.np_local(st, 3, 3, 0, 0, 1, True)
    assert k == 1 and win.tolist() == [[6, 6, 6], [0, 3, 2], [0, 5, 0]]
    win, k = lp.np_local(st, 3, 3, 0, 0, 1, False)         # the heading is reported, the window keeps the board's axes
    assert k == 1 and win.tolist() == [[6, 2, 0], [6, 3, 5], [6, 0, 0]]
    win, k = lp.np_local(st, 3, 3, 0, 1, 1, True)          # snake 1 at (1, 1) moves along -c0: the board turned by 180 degrees
    assert k == 2 and win.tolist() == [[1, 0, 0], [0, 3, 5], [0, 0, 4]]
    win, k = lp.np_local(st, 3, 3, 0, 2, 2, True)          # an empty body: zeros, heading 0, whatever its velocity
    assert k == 0 and win.shape == (5, 5) and not win.any()
    for s in range(3):
        for oriented in (False, True):
            a, b = lp.np_local(st, 3, 3, 0, s, 2, oriented), lp.np_local_rot(st, 3, 3, 0, s, 2, oriented)
            assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ------------------------------------------------------------------------------------------ the two statements agree
def _agree(states, dim, ns, rules):
    lp.deal_velocities(states, ns)
    shares = lp.heading_shares(states, ns)
    assert min(shares) >= 1 / 8, shares
    planes = lp.planes_all(states, dim, ns, rules)
    cases = 0
    for radius in RADII:
        for oriented in (False, True):
            a = lp.np_local_all(states, dim, ns, rules, range(ns), radius, oriented, lp.np_local, planes)
            b = lp.np_local_all(states, dim, ns, rules, range(ns), radius, oriented, lp.np_local_rot, planes)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (dim, rules, radius, oriented)
            assert a[0].max() <= 6 and a[1].max() <= 3
            cases += a[1].size
    # a window larger than the board shows the whole plane once, whatever the heading: the counts of each code agree
    win = lp.np_local_all(states, dim, ns, rules, range(ns), 31, True, lp.np_local, planes)[0]
    for e, st in enumerate(states):
        for s in range(ns):
            h = st["snakes"][s][0] if st["snakes"][s] else None
            if h and 0 <= h[0] < dim and 0 <= h[1] < dim:
                assert np.bincount(win[e, s].ravel(), minlength=7)[:6].tolist() == np.bincount(planes[e][s].ravel(), minlength=6).tolist()
    return cases


@pytest.mark.parametrize("dim", [2, 3, 6, 19])
def test_statements_agree_on_snake_env_states(dim):
    assert _agree(cp.snake_env_states(dim), dim, 3, 0) > 0


@pytest.mark.parametrize("dim", [6, 10])
def test_statements_agree_on_new_world_states(dim):
    states = cp.new_world_states(dim, 4, 5)
    assert sum(1 for st in states for s in range(4) if not st["alive"][s] and st["snakes"][s]) >= 4
    _agree(states, dim, 4, 1)


@pytest.mark.parametrize("dim", [6, 19])
def test_statements_agree_on_adversarial_states(dim):
    states = cp.adversarial_states(dim, 3)
    assert max(len(st["fruits"]) for st in states) > 64
    _agree(states, dim, 3, 2)


# ------------------------------------------------------------------------------------------ relative actions
def test_relative_to_absolute_is_the_headers_rule():
    rel, k = torch.meshgrid(torch.arange(5), torch.arange(4), indexing="ij")
    want = [[lp.relative_to_absolute(r, h) for h in range(4)] for r in range(5)]
    assert want[0] == [0] * 4 and want[1] == [1, 2, 3, 4] and want[2] == [2, 3, 4, 1] and want[4] == [4, 1, 2, 3]
    for dtype in (torch.int64, torch.int32):
        got = msnake.relative_to_absolute(rel.to(dtype), k.to(torch.uint8))           # [5, 4]: the [num_envs, S] form
        assert got.dtype == dtype and got.tolist() == want
        got = msnake.relative_to_absolute(rel.flatten().to(dtype), k.flatten())      # [20]: the [num_envs] form
        assert got.dtype == dtype and got.tolist() == sum(want, [])
    for bad in ((rel.float(), k), (rel, k.float()), (rel[:, :2], k), (rel[None], k[None]), (rel.numpy(), k), (rel[0, 0], k[0, 0])):
        with pytest.raises(ValueError):
            msnake.relative_to_absolute(*bad)


@pytest.mark.parametrize("rules,dim,ns", [(0, 6, 3), (1, 6, 4), (2, 6, 3)])
def test_relative_actions_point_at_the_window_entries_the_header_names(rules, dim, ns):
    """Relative action 1 enters the cell shown at [radius + 1][radius]; 2, 3, 4 the +j side, the back, the -j side."""
    states = {0: cp.snake_env_states, 1: lambda d: cp.new_world_states(d, ns, 3), 2: lambda d: cp.adversarial_states(d, ns)}[rules](dim)
    lp.deal_velocities(states, ns, start=2)
    entry = {1: (1, 0), 2: (0, 1), 3: (-1, 0), 4: (0, -1)}
    checked = 0
    for radius in (1, 3):
        for st in states:
            for s in range(ns):
                if not st["snakes"][s]:
                    continue
                win, k = lp.np_local(st, dim, ns, rules, s, radius, True)
                plane = lp.plane_of(st, dim, ns, rules, s)
                for r in (1, 2, 3, 4):
                    move = lp.MOVES[lp.relative_to_absolute(r, k)]
                    c0, c1 = st["snakes"][s][0][0] + move[0], st["snakes"][s][0][1] + move[1]
                    want = plane[c0, c1] if 0 <= c0 < dim and 0 <= c1 < dim else lp.OUTSIDE
                    assert win[radius + entry[r][0], radius + entry[r][1]] == want, (st, s, r)
                    checked += 1
    assert checked > 400


@pytest.mark.parametrize("rules,ns", [(0, 3), (2, 3), (1, 4)])
def test_forward_never_turns_a_moving_snake_on_the_oracle(rules, ns):
    """Relative action 1 mapped through the rule keeps every non-zero velocity, step after step, on the oracle."""
    cfg = dict(rules=rules, dim=10, n_snakes=ns, n_fruits=ns, num_envs=8, seed=3, env_id_base=0, max_steps=2000)
    ora = sp.make_oracle(cfg)
    ora.reset()
    rng = np.random.default_rng(rules)
    read = sp._StateReader(ora)
    kept = seen = 0
    for t in range(120):
        before = [read(e) for e in range(8)]
        forward = t % 4 != 0                                      # every fourth step is random: the headings vary
        if forward:
            act = np.array([[lp.relative_to_absolute(1, lp.heading_of(st, s)) for s in range(ns)] for st in before], np.int32)
        else:
            act = rng.integers(0, 5, (8, ns)).astype(np.int32)
        _, _, done, *_ = ora.step(act, want_obs=False)
        if not forward:
            continue
        for e in range(8):
            after = read(e)
            if done[e]:
                continue                                          # (reset: another game)
            for s in range(ns):
                v = tuple(before[e]["vels"][s])
                if v != (0, 0) and before[e]["snakes"][s] and after["snakes"][s]:
                    assert tuple(after["vels"][s]) == v, (t, e, s, before[e], after)
                    kept += 1
                    seen |= 1 << lp.HEADING[v]
    assert kept > 50 and seen == 0b1111, (kept, seen)   # every direction was kept, many times


# ------------------------------------------------------------------------------------------ the wrapper's `snakes`
def test_snakes_are_normalised_to_a_mask_and_an_ascending_list():
    nsn = vec_env.normalize_snakes
    assert nsn(None, 3) == (0b111, [0, 1, 2]) and nsn(None, 4) == (0b1111, [0, 1, 2, 3]) and nsn(None, 1) == (1, [0])
    assert nsn(2, 3) == (0b100, [2]) and nsn(np.int64(0), 3) == (1, [0])
    assert nsn([0, 2], 3) == (0b101, [0, 2]) and nsn((3,), 4) == (0b1000, [3]) and nsn(np.array([0, 3]), 4) == (0b1001, [0, 3])
    for bad in (3, -1, [0, 3], [2, 0], [1, 1], [0.5], "01", True, [True], []):
        with pytest.raises(ValueError) as err:
            nsn(bad, 3)
        assert "snake" in str(err.value) and "view" not in str(err.value), str(err.value)


def test_local_shape():
    env = types.SimpleNamespace(n_snakes=3)
    shape = msnake.MultiSnakeVecEnv.local_shape
    assert shape(env, 5) == (3, 11, 11) and shape(env, 1, 2) == (1, 3, 3) and shape(env, 31, [0, 2]) == (2, 63, 63)
    for radius in (0, 32, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="radius"):
            shape(env, radius)
    with pytest.raises(ValueError, match="snake"):
        shape(env, 5, [3])


# ------------------------------------------------------------------------------------------ the policy
def test_window_policy_shapes_sampling_and_trunk():
    torch.manual_seed(0)
    pol, cnn = selfplay.WindowPolicy(5), selfplay.CnnPolicy((21, 21, 3))
    win = torch.randint(0, 7, (9, 11, 11), dtype=torch.uint8)
    logits, v = pol(win)
    assert logits.shape == (9, 5) and v.shape == (9,) and logits.dtype == v.dtype == torch.float32
    a, v2, nlp = pol.step(win)
    assert a.shape == (9,) and a.dtype == torch.int64 and int(a.min()) >= 0 and int(a.max()) < 5
    assert torch.equal(v2, v) and torch.allclose(nlp, selfplay.neglogp(logits, a)) and torch.equal(pol.value(win), v)
    # seven input channels, one per code: a window of one code lights one channel
    x = (torch.full((1, 11, 11), 6, dtype=torch.uint8).unsqueeze(1) == pol.codes).float()
    assert x.shape == (1, 7, 11, 11) and x[0, 6].all() and not x[0, :6].any()
    # the trunk is CnnPolicy's: the same layers, apart from the first conv's input channels and fc1's input width
    count = lambda m: sum(p.numel() for p in m.parameters())
    assert [type(m) for m in pol.convs] == [type(m) for m in cnn.convs]
    for i in (2, 4, 6):
        assert count(pol.convs[i]) == count(cnn.convs[i])
    assert count(pol.pi) == count(cnn.pi) and count(pol.v) == count(cnn.v) and pol.fc1.out_features == cnn.fc1.out_features == 512
    assert pol.convs[0].in_channels == 7 and pol.convs[0].out_channels == cnn.convs[0].out_channels == 32
    assert pol.fc1.in_features == 64 * 11 * 11 and cnn.fc1.in_features == 64 * 21 * 21
    assert float(pol.pi.bias.detach().abs().max()) == 0 and float(pol.pi.weight.detach().abs().max()) < 0.05     # the heads' initialisation
    assert selfplay.WindowPolicy(1)(torch.zeros((2, 3, 3), dtype=torch.uint8))[0].shape == (2, 5)
    for bad in (win[:, :10], win.long(), win[0]):
        with pytest.raises(ValueError):
            pol(bad)
    with pytest.raises(ValueError, match="radius"):
        selfplay.WindowPolicy(0)


def test_weights_of_the_other_kind_are_refused(tmp_path):
    """A window run's weights carry the radius and the orientation flag; loading frames into windows, windows into frames,
    another radius or the other orientation is refused with a message that names both kinds."""
    f = lambda name: str(tmp_path / name)
    cnn, w5, w5n, w2 = (selfplay.CnnPolicy((21, 21, 3)), selfplay.WindowPolicy(5), selfplay.WindowPolicy(5, oriented=False),
                        selfplay.WindowPolicy(2))
    for model, name in ((cnn, "cnn.pt"), (w5, "w5.pt"), (w5n, "w5n.pt"), (w2, "w2.pt")):
        selfplay.save_weights(model, f(name))
    assert selfplay.window_kind(torch.load(f("cnn.pt"), weights_only=True)) is None
    assert selfplay.window_kind(torch.load(f("w5.pt"), weights_only=True)) == (5, True)
    assert selfplay.window_kind(torch.load(f("w5n.pt"), weights_only=True)) == (5, False)
    selfplay.load_weights(selfplay.WindowPolicy(5), f("w5.pt"))           # the same kind loads
    selfplay.load_weights(selfplay.CnnPolicy((21, 21, 3)), f("cnn.pt"))
    for model, name, words in ((w5, "cnn.pt", ("full frames", "radius 5")), (cnn, "w5.pt", ("radius 5, oriented", "full frames")),
                               (w5, "w2.pt", ("radius 2", "radius 5")), (w5, "w5n.pt", ("not oriented", "radius 5, oriented")),
                               (w5n, "w5.pt", ("radius 5, oriented", "not oriented"))):
        with pytest.raises(RuntimeError) as err:
            selfplay.load_weights(model, f(name))
        assert all(w in str(err.value) for w in words) and "cannot be loaded" in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------------ the driver
def test_runner_feeds_windows_and_maps_relative_actions():
    torch.manual_seed(1)
    for oriented in (True, False):
        env = _FakeLocalEnv()
        model = selfplay.WindowPolicy(2, oriented=oriented)
        opponents = [selfplay.WindowPolicy(2, oriented=oriented), None]      # snake 1 a network, snake 2 the constant action 1
        runner = selfplay.Runner(env, model, opponents, 4, 0.99, 0.95, local_radius=2, oriented=oriented)
        assert env.renders == [(2, [0, 1], oriented)] and runner.win.shape == (8, 2, 5, 5)
        heading = runner.heading.clone()
        a, v, nlp, full = runner.multi_step()
        assert full.dtype == torch.int32 and full.shape == (8, 3) and (full[:, 2] == 1).all()
        want = msnake.relative_to_absolute(a, heading[:, 0]) if oriented else a
        assert torch.equal(full[:, 0].long(), want)
        obs, returns, masks, actions, values, nlps, _ = runner.run()
        assert obs.shape == (32, 5, 5) and obs.dtype == torch.uint8 and actions.shape == (32,) and len(env.actions) == 4
        assert len(env.renders) == 1 + 4                                     # one call per env step, for every network at once
        # a model sampling 0 ("keep going") is never turned into a move
        assert all(int(x) == 0 for x in msnake.relative_to_absolute(torch.zeros(8, dtype=torch.int64), heading[:, 0]))


def test_learn_on_windows_and_the_refusal_of_the_other_kind(tmp_path):
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 2, nminibatches=2, noptepochs=1, opponent_save_interval=1, log_fn=None)
    d = str(tmp_path / "win")
    model, hist = selfplay.learn(_FakeLocalEnv(n_snakes=2), save_dir=d, local_radius=2, **kw)
    assert isinstance(model, selfplay.WindowPolicy) and (model.radius, model.oriented) == (2, True) and len(hist) == 2
    path = os.path.join(d, "snake_model_num2.pt")
    assert selfplay.window_kind(torch.load(path, weights_only=True)) == (2, True)
    selfplay.learn(_FakeLocalEnv(n_snakes=2), load_path=path, local_radius=2, **kw)          # the same kind loads
    for other in (dict(local_radius=None), dict(local_radius=3), dict(local_radius=2, oriented=False)):
        env = _FakeLocalEnv(n_snakes=2) if other["local_radius"] else FakeEnv()
        with pytest.raises(RuntimeError, match="cannot be loaded"):
            selfplay.learn(env, load_path=path, **dict(kw, **other))
        with pytest.raises(RuntimeError, match="cannot be loaded"):                          # nor resumed
            selfplay.learn(env, save_dir=d, resume=True, **dict(kw, **other))
    d2 = str(tmp_path / "frames")
    selfplay.learn(FakeEnv(), save_dir=d2, **kw)
    with pytest.raises(RuntimeError, match="full frames"):
        selfplay.learn(_FakeLocalEnv(n_snakes=2), load_path=os.path.join(d2, "snake_model_num2.pt"), local_radius=2, **kw)
