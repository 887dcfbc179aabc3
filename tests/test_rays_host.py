"""CPU-side checks of the eight-direction rays (msnake_render_rays, MultiSnakeVecEnv.render_rays_device): the entry
point is declared, exported and refuses a NULL handle before it touches the GPU; tests/rays_play.py on boards computed
by hand; its two statements (the walk on the plane, the read off the radius-31 window) agree and the rotation identity
of the header holds on the hand-built states of all three rule sets; those states cover what the GPU test needs;
RayPolicy, the refusal of weights of another kind, and the driver on a fake env.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from fake_envs import FakeEnv, FakeLocalEnv
import local_play as lp
import msnake
import rays_play as rp
from msnake import selfplay, vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_render_rays\(msnake_handle h, uint32_t snake_mask, int32_t oriented,\s*uint8_t\* rays_dev,\s*"
           r"uint8_t\* heading_dev,\s*void\* stream\);")
    assert re.search(sig, text)
    for name, value in (("DIRS", 8), ("CHANNELS", 4), ("WALL", 0), ("FRUIT", 1), ("OWN", 2), ("OTHER", 3)):
        assert re.search(rf"#define MSNAKE_RAY_{name} {value}\b", text), name
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    contract = text.split("int msnake_render_rays(")[0].rsplit("/*", 1)[1]
    assert "rays_or[j] = rays_un[(j + 2 k)" in contract and "MSNAKE_E_ARG" in contract and "MSNAKE_E_ALIGN" in contract
    assert "msnake_render_rays" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_render_rays is not None and lib.msnake_abi_version() == 3
    assert (vec_env.RAY_DIRS, vec_env.RAY_CHANNELS) == (rp.DIRS, rp.CHANNELS) == (8, 4)
    assert (vec_env.RAY_WALL, vec_env.RAY_FRUIT, vec_env.RAY_OWN, vec_env.RAY_OTHER) == (rp.WALL, rp.FRUIT, rp.OWN, rp.OTHER)


def test_null_and_destroyed_handles_are_refused():
    lib = msnake._capi.load()
    assert lib.msnake_render_rays(None, 1, 1, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    dead = ctypes.create_string_buffer(4)       # what a destroyed handle looks like: the magic word is gone
    for mask, oriented in ((1, 1), (0, 1), (1, 2)):   # the handle check comes first
        assert lib.msnake_render_rays(dead, mask, oriented, None, None, None) == -3
        assert b"handle" in lib.msnake_last_error()


def test_rays_shape():
    env = types.SimpleNamespace(n_snakes=3)
    shape = msnake.MultiSnakeVecEnv.rays_shape
    assert shape(env) == (3, 8, 4) and shape(env, 2) == (1, 8, 4) and shape(env, [0, 2]) == (2, 8, 4)
    for bad in ([3], [], [1, 0]):
        with pytest.raises(ValueError, match="snake"):
            shape(env, bad)


# ------------------------------------------------------------------------------------------ boards computed by hand
def _st(snakes, fruits, vels=None, alive=None):
    n = len(snakes)
    return {"fruits": [list(f) for f in fruits], "snakes": [[list(c) for c in b] for b in snakes],
            "alive": list(alive) if alive else [True] * n, "vels": [list(v) for v in (vels or [(0, 0)] * n)]}


def _rays(st, dim, s=0, oriented=False, rules=0):
    return rp.np_rays(st, dim, len(st["snakes"]), rules, s, oriented)[0].tolist()


def test_an_empty_5x5_board_with_a_centred_head():
    assert _rays(_st([[(2, 2)]], []), 5) == [[3, 0, 0, 0]] * 8      # three steps to the wall on the axes and on the diagonals


def test_a_head_in_a_corner():
    got = _rays(_st([[(0, 0)]], []), 5)
    # directions: (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1)
    assert [r[0] for r in got] == [5, 5, 5, 1, 1, 1, 1, 1] and all(r[1:] == [0, 0, 0] for r in got)


def test_heads_at_minus_one_and_at_dim():
    got = _rays(_st([[(-1, 2)]], [(0, 2), (1, 4)]), 5)
    assert [r[0] for r in got] == [6, 3, 1, 1, 1, 1, 1, 3]          # into the board 5 cells and the wall; along the wall: 1
    assert got[0][1] == 1 and got[1][1] == 2                          # the fruits at t = 1 ahead and t = 2 on the diagonal
    got = _rays(_st([[(5, 5)]], []), 5)                              # (dim, dim): only the diagonal back in crosses the board
    assert [r[0] for r in got] == [1, 1, 1, 1, 1, 6, 1, 1]
    got = _rays(_st([[(-1, -1)]], [(61, 61)]), 62)                   # the longest ray there is: 62 cells, the wall at 63
    assert got[1] == [63, 62, 0, 0] and [r[0] for r in got[:1] + got[2:]] == [1] * 7


def test_a_fruit_hidden_under_a_body_and_rays_that_see_through():
    st = _st([[(0, 0), (0, 1), (0, 2)], [(0, 3)]], [(0, 2), (0, 4)])
    got = _rays(st, 6)
    assert got[2] == [6, 4, 1, 3]    # along +c1: the fruit under the body is hidden, the one behind the other snake is seen
    assert got[0] == [6, 0, 0, 0]
    assert _rays(st, 6, s=1)[6] == [4, 0, 0, 1] and _rays(st, 6, s=1)[2] == [3, 1, 0, 0]   # snake 1 looks back at snake 0


def test_the_snakes_own_stacked_duplicate_on_its_head():
    st = _st([[(2, 2), (2, 2), (2, 3)]], [])
    got = _rays(st, 5)
    assert got[2] == [3, 0, 1, 0] and all(r[2] == 0 for j, r in enumerate(got) if j != 2)   # t = 0 is not looked at


def test_a_later_snake_painted_over_an_earlier_one():
    st = _st([[(0, 0), (0, 2)], [(4, 4), (0, 2), (0, 3)]], [])
    assert _rays(st, 5)[2] == [5, 0, 0, 2]                           # (0, 2) shows snake 1: nothing of its own on the ray
    assert _rays(st, 5, s=1)[5] == [5, 0, 0, 4]                      # and snake 1 sees the head of snake 0 at (0, 0) only
    st2 = _st([[(4, 4), (0, 2), (0, 3)], [(0, 0), (0, 2)]], [])      # the other order: snake 1's piece on top
    assert _rays(st2, 5, s=1)[2] == [5, 0, 2, 3]


def test_a_dead_new_world_snake():
    st = _st([[(0, 0)], [(0, 2), (0, 3)]], [(0, 4)], alive=[True, False])
    assert _rays(st, 5, rules=1)[2] == [5, 4, 0, 0]                  # painted nowhere
    assert _rays(st, 5, s=1, rules=1)[2] == [3, 2, 0, 0]             # its own rays start at its head and miss its body
    assert _rays(st, 5, rules=0)[2] == [5, 4, 0, 2]                  # (the other rule sets have no dead snakes)


def test_an_empty_body():
    st = _st([[], [(1, 1)]], [(0, 0)], vels=[(0, 1), (0, 1)])
    rays, k = rp.np_rays(st, 5, 2, 0, 0, True)
    assert not rays.any() and k == 0
    assert not rp.rays_from_window(lp.np_local(st, 5, 2, 0, 0, 31, True)[0]).any()


def test_oriented_rays_turn_with_the_heading():
    st = _st([[(1, 2)]], [(3, 2)], vels=[(0, 1)])                    # moving along +c1: f = (0, 1), g = (-1, 0)
    un, k = rp.np_rays(st, 5, 1, 0, 0, False)
    orr, _ = rp.np_rays(st, 5, 1, 0, 0, True)
    assert k == 1 and un[0].tolist() == [4, 2, 0, 0] and orr[6].tolist() == [4, 2, 0, 0]   # the fruit lies on the -g side
    assert orr[0].tolist() == [3, 0, 0, 0] and np.array_equal(orr, rp.rotate(un, 1))


# ------------------------------------------------------------------------------------------ the builder sets
@pytest.fixture(scope="module")
def sets():
    """Every builder set once: (name, rules, dim, ns, states, planes, unoriented rays, oriented rays, headings)."""
    out = []
    for name, rules, dim, ns, _, states in rp.builder_sets():
        planes = lp.planes_all(states, dim, ns, rules)
        un, head = rp.np_rays_all(states, dim, ns, rules, range(ns), False, planes)
        orr, head2 = rp.np_rays_all(states, dim, ns, rules, range(ns), True, planes)
        assert np.array_equal(head, head2)
        out.append((name, rules, dim, ns, states, planes, un, orr, head))
    return out


def test_the_walk_equals_the_read_off_the_radius_31_window(sets):
    cases = 0
    for name, rules, dim, ns, states, planes, un, orr, _ in sets:
        if dim > 30:
            continue
        for oriented, want in ((False, un), (True, orr)):
            win = lp.np_local_all(states, dim, ns, rules, range(ns), 31, oriented, planes=planes)[0]
            got = rp.rays_from_windows(win)
            assert np.array_equal(got, want), (name, oriented, np.argwhere(got != want)[:4].tolist())
            cases += want.shape[0] * want.shape[1]
    assert cases > 2000


def test_the_rotation_identity(sets):
    seen = set()
    for name, rules, dim, ns, states, planes, un, orr, head in sets:
        for e in range(len(states)):
            for s in range(ns):
                assert np.array_equal(orr[e, s], rp.rotate(un[e, s], head[e, s])), (name, e, s)
                seen.add(int(head[e, s]))
    assert seen == {0, 1, 2, 3}


def test_the_builder_sets_cover_what_the_gpu_test_needs(sets):
    """So that no comparison passes on zeros: an off-grid head, the value 63, and non-zero shares of the three object
    channels of at least 0.03 / 0.06 / 0.09 over the oriented rays of snakes with a body (the reference alone gives about
    twice each)."""
    offgrid = total = 0
    nonzero = np.zeros(4)
    top = 0
    for name, rules, dim, ns, states, planes, un, orr, head in sets:
        assert 48 <= len(states) <= 97, (name, len(states))
        for e, st in enumerate(states):
            for s in range(ns):
                body = st["snakes"][s]
                if not body:
                    continue
                offgrid += not (0 <= body[0][0] < dim and 0 <= body[0][1] < dim)
                total += 8
                nonzero += (orr[e, s] != 0).sum(axis=0)
        top = max(top, int(orr.max()), int(un.max()))
    share = nonzero / total
    assert offgrid > 0 and top == 63, (offgrid, top)
    assert share[rp.WALL] == 1.0 and share[rp.FRUIT] >= 0.03 and share[rp.OWN] >= 0.06 and share[rp.OTHER] >= 0.09, share.tolist()


# ------------------------------------------------------------------------------------------ the policy
def test_ray_policy_shapes_sampling_and_features():
    torch.manual_seed(0)
    pol = selfplay.RayPolicy()
    rays = torch.randint(0, 64, (9, 8, 4), dtype=torch.uint8)
    logits, v = pol(rays)
    assert logits.shape == (9, 5) and v.shape == (9,) and logits.dtype == v.dtype == torch.float32
    a, v2, nlp = pol.step(rays)
    assert a.shape == (9,) and a.dtype == torch.int64 and int(a.min()) >= 0 and int(a.max()) < 5
    assert torch.equal(v2, v) and torch.allclose(nlp, selfplay.neglogp(logits, a)) and torch.equal(pol.value(rays), v)
    x = torch.zeros((1, 8, 4), dtype=torch.uint8)
    x[0, 0, 0], x[0, 0, 1], x[0, 7, 3] = 1, 4, 63
    f = selfplay.RayPolicy.features(x)
    assert f.shape == (1, 32) and f.dtype == torch.float32
    assert f[0, 0] == 1.0 and f[0, 1] == 0.25 and f[0, 2] == 0.0 and abs(float(f[0, 31]) - 1 / 63) < 1e-7
    assert int((f != 0).sum()) == 3 and torch.isfinite(f).all()                            # 0 stays 0: nothing divides by it
    assert [type(m) for m in (pol.fc1, pol.fc2, pol.pi, pol.v)] == [torch.nn.Linear] * 4
    assert (pol.fc1.in_features, pol.fc1.out_features, pol.fc2.in_features, pol.fc2.out_features) == (32, 64, 64, 64)
    assert pol.pi.out_features == 5 and pol.v.out_features == 1
    assert not any(isinstance(m, torch.nn.Conv2d) for m in pol.modules())
    assert float(pol.pi.bias.detach().abs().max()) == 0 and float(pol.pi.weight.detach().abs().max()) < 0.05
    for bad in (rays[:, :7], rays.long(), rays[0], rays.flatten(1)):
        with pytest.raises(ValueError):
            pol(bad)


def test_weights_of_another_kind_are_refused(tmp_path):
    """Frame, window and ray weights each load only into their own kind; the message names both kinds."""
    f = lambda name: str(tmp_path / name)
    cnn, w5, ray, rayn = selfplay.CnnPolicy((21, 21, 3)), selfplay.WindowPolicy(5), selfplay.RayPolicy(), selfplay.RayPolicy(oriented=False)
    for model, name in ((cnn, "cnn.pt"), (w5, "w5.pt"), (ray, "ray.pt"), (rayn, "rayn.pt")):
        selfplay.save_weights(model, f(name))
    sd = lambda name: torch.load(f(name), weights_only=True)
    assert selfplay.ray_kind(sd("ray.pt")) == (True,) and selfplay.ray_kind(sd("rayn.pt")) == (False,)
    assert selfplay.ray_kind(sd("cnn.pt")) is None and selfplay.ray_kind(sd("w5.pt")) is None
    assert selfplay.window_kind(sd("ray.pt")) is None
    selfplay.load_weights(selfplay.RayPolicy(), f("ray.pt"))              # the same kind loads
    selfplay.load_weights(selfplay.RayPolicy(oriented=False), f("rayn.pt"))
    for model, name, words in ((ray, "cnn.pt", ("full frames", "rays, oriented")), (ray, "w5.pt", ("radius 5", "rays, oriented")),
                               (cnn, "ray.pt", ("rays, oriented", "full frames")), (w5, "ray.pt", ("rays, oriented", "radius 5")),
                               (ray, "rayn.pt", ("rays, not oriented", "rays, oriented")), (rayn, "ray.pt", ("rays, oriented", "rays, not oriented")),
                               (w5, "rayn.pt", ("rays, not oriented", "radius 5, oriented")), (cnn, "w5.pt", ("radius 5", "full frames"))):
        with pytest.raises(RuntimeError) as err:
            selfplay.load_weights(model, f(name))
        assert all(w in str(err.value) for w in words) and "cannot be loaded" in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------------ the driver
class _FakeRayEnv:
    """CPU stand-in with the device-side surface learn(rays=True) uses: frames nobody looks at, seeded rays and headings
    through render_rays_device, and a record of every call."""

    def __init__(self, n=8, n_snakes=3, seed=0):
        self.num_envs, self.n_snakes, self.obs_shape, self.device = n, n_snakes, (12, 12, 9), torch.device("cpu")
        self.g = torch.Generator().manual_seed(seed)
        self.renders, self.actions = [], []

    def reset_device(self):
        return torch.zeros((self.num_envs,) + self.obs_shape, dtype=torch.uint8)

    def rays_shape(self, snakes=None):
        return msnake.MultiSnakeVecEnv.rays_shape(self, snakes)

    def render_rays_device(self, snakes=None, oriented=True, out=None, heading_out=None):
        assert tuple(out.shape) == (self.num_envs,) + self.rays_shape(snakes) and out.dtype == torch.uint8
        assert tuple(heading_out.shape) == tuple(out.shape[:2]) and heading_out.dtype == torch.uint8
        out.copy_(torch.randint(0, 64, out.shape, dtype=torch.uint8, generator=self.g))
        heading_out.copy_(torch.randint(0, 4, heading_out.shape, dtype=torch.uint8, generator=self.g))
        self.renders.append((list(snakes), bool(oriented)))
        return out, heading_out

    def step_device(self, actions):
        assert actions.shape == (self.num_envs, self.n_snakes) and actions.dtype == torch.int32
        assert int(actions.min()) >= 0 and int(actions.max()) <= 4
        self.actions.append(actions.clone())
        done = torch.rand(self.num_envs, generator=self.g) < 0.3
        info = torch.zeros((self.num_envs, 4), dtype=torch.int32)
        info[:, 0] = torch.full((self.num_envs,), 7.0).view(torch.int32)
        return self.reset_device(), torch.ones(self.num_envs), done.to(torch.uint8), info


def test_runner_feeds_rays_and_maps_relative_actions():
    torch.manual_seed(1)
    for oriented in (True, False):
        env = _FakeRayEnv()
        model = selfplay.RayPolicy(oriented=oriented)
        opponents = [None, selfplay.RayPolicy(oriented=oriented)]            # snake 1 the constant action 1, snake 2 a network
        runner = selfplay.Runner(env, model, opponents, 4, 0.99, 0.95, oriented=oriented, rays=True)
        assert env.renders == [([0, 2], oriented)] and runner.win.shape == (8, 2, 8, 4)
        heading = runner.heading.clone()
        a, v, nlp, full = runner.multi_step()
        assert full.dtype == torch.int32 and full.shape == (8, 3) and (full[:, 1] == 1).all()
        want = msnake.relative_to_absolute(a, heading[:, 0]) if oriented else a
        assert torch.equal(full[:, 0].long(), want)
        obs, returns, masks, actions, values, nlps, _ = runner.run()
        assert obs.shape == (32, 8, 4) and obs.dtype == torch.uint8 and actions.shape == (32,) and len(env.actions) == 4
        assert env.renders == [([0, 2], oriented)] * (1 + 4)                 # one call per env step, for exactly the networks
    with pytest.raises(ValueError, match="mutually exclusive"):
        selfplay.Runner(_FakeRayEnv(), model, opponents, 4, 0.99, 0.95, local_radius=2, rays=True)


def test_learn_on_rays_and_the_refusals(tmp_path):
    kw = dict(nsteps=4, total_timesteps=8 * 4 * 2, nminibatches=2, noptepochs=1, opponent_save_interval=1, log_fn=None)
    d = str(tmp_path / "rays")
    env = _FakeRayEnv(n_snakes=3)
    model, hist = selfplay.learn(env, save_dir=d, rays=True, scripted_opponents=None, **kw)
    assert isinstance(model, selfplay.RayPolicy) and model.oriented and len(hist) == 2
    assert env.renders == [([0, 1, 2], True)] * (1 + 2 * 4) and len(env.actions) == 2 * 4     # once per step, every network
    path = os.path.join(d, "snake_model_num3.pt")
    assert selfplay.ray_kind(torch.load(path, weights_only=True)) == (True,)
    selfplay.learn(_FakeRayEnv(n_snakes=3), load_path=path, rays=True, **kw)                  # the same kind loads
    with pytest.raises(ValueError, match="mutually exclusive"):                               # before anything is built
        selfplay.learn(_FakeRayEnv(n_snakes=3), rays=True, local_radius=2, **kw)
    d2 = str(tmp_path / "rays2")
    selfplay.learn(_FakeRayEnv(n_snakes=2), save_dir=d2, rays=True, **kw)
    path2 = os.path.join(d2, "snake_model_num2.pt")
    for other, fake in ((dict(), FakeEnv()), (dict(local_radius=2), FakeLocalEnv(n_snakes=2)),
                        (dict(rays=True, oriented=False), _FakeRayEnv(n_snakes=2))):
        with pytest.raises(RuntimeError, match="cannot be loaded"):
            selfplay.learn(fake, load_path=path2, **dict(kw, **other))
        with pytest.raises(RuntimeError, match="cannot be loaded"):                           # nor resumed
            selfplay.learn(fake, save_dir=d2, resume=True, **dict(kw, **other))
    d3 = str(tmp_path / "win")
    selfplay.learn(FakeLocalEnv(n_snakes=2), save_dir=d3, local_radius=2, **kw)
    with pytest.raises(RuntimeError, match="windows of radius 2"):
        selfplay.learn(_FakeRayEnv(n_snakes=2), load_path=os.path.join(d3, "snake_model_num2.pt"), rays=True, **kw)
