"""CPU-side checks of the cell-code observation (msnake_render_cells, MultiSnakeVecEnv.render_cells_device): the entry
point is declared, exported and refuses a NULL handle before it touches the GPU; the helper tests/cells_play.py is
pinned to the reference's picture -- np_cells equals decode_frame(oracle.render()) and np_snake_rows equals the
oracle's exported words, on oracle play from reset and on the hand-built states the GPU tests install; the wrapper's
normalisation of `views`.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cells_play as cp
import msnake
import scripted_play as sp
from msnake import vec_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_render_cells\(msnake_handle h, uint32_t view_mask, uint8_t\* cells_dev,\s*int32_t\* snakes_dev, "
           r"void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "snake_multiple_test.py:35-58,93-95" in text.split("int msnake_render_cells(")[0].rsplit("/*", 1)[1]
    assert "msnake_render_cells" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_render_cells is not None and lib.msnake_abi_version() == 3


def test_null_and_destroyed_handles_are_refused():
    lib = msnake._capi.load()
    assert lib.msnake_render_cells(None, 1, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    dead = ctypes.create_string_buffer(4)       # what a destroyed handle looks like: the magic word is gone
    lib.msnake_render_cells(None, 0b1000, None, None, None)     # (the NULL case's message is replaced, not kept)
    for mask in (1, 0, 0b10000):                # the handle check comes before every argument check
        assert lib.msnake_render_cells(dead, mask, None, None, None) == -3
        assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ the helper by hand
def test_np_cells_on_a_hand_computed_3x3():
    st = {"fruits": [[2, 2], [0, 1]], "snakes": [[[0, 0], [0, 1]], [[1, 1], [0, 0]], []], "alive": [True] * 3}
    # view 0: the fruit at (0, 1) lies under snake 0's body; snake 1's body piece at (0, 0) covers snake 0's head
    assert cp.np_cells(st, 3, 3, 0, [0]).tolist() == [[[4, 2, 0], [0, 5, 0], [0, 0, 1]]]
    assert cp.np_cells(st, 3, 3, 0, [1, 2]).tolist() == [[[2, 4, 0], [0, 3, 0], [0, 0, 1]], [[4, 4, 0], [0, 5, 0], [0, 0, 1]]]
    # new_world: the dead snake 1 vanishes, and snake 0's head shows again
    assert cp.np_cells(dict(st, alive=[True, False, True]), 3, 3, 1, [0]).tolist() == [[[3, 2, 0], [0, 0, 0], [0, 0, 1]]]
    # the same alive bits mean nothing under snake_env
    assert np.array_equal(cp.np_cells(dict(st, alive=[True, False, True]), 3, 3, 0, [0]), cp.np_cells(st, 3, 3, 0, [0]))
    # a head outside the grid paints nothing, its body does
    st = {"fruits": [[-1, 0], [3, 3]], "snakes": [[[-1, 1], [0, 1]]], "alive": [True]}
    assert cp.np_cells(st, 3, 1, 2, [0, 2]).tolist() == [[[0, 2, 0], [0, 0, 0], [0, 0, 0]], [[0, 4, 0], [0, 0, 0], [0, 0, 0]]]


def test_decode_frame_refuses_other_colours_and_a_broken_border():
    ora = sp.make_oracle(dict(num_envs=1, dim=4, n_snakes=2, n_fruits=2, rules=0, seed=0, env_id_base=0, max_steps=100))
    frame = ora.reset()[0].copy()
    assert cp.decode_frame(frame, [0, 1, 2]).shape == (3, 4, 4) and cp.decode_frame(frame, []).shape == (0, 4, 4)
    bad = frame.copy()
    bad[2, 2, 3:6] = (1, 2, 3)
    cp.decode_frame(bad, [0, 2])
    with pytest.raises(AssertionError, match="six-colour"):
        cp.decode_frame(bad, [1])
    bad = frame.copy()
    bad[0, 3, 0] = 0
    with pytest.raises(AssertionError, match="border"):
        cp.decode_frame(bad, [0])


# ------------------------------------------------------------------------------------------ the helper against the oracle
def _raw_rows(ora, e):
    """The eight row fields straight from the oracle's exported words, without flat_to_state / np_snake_rows."""
    n = ora.L.orc_export_state(ora.h, e, None, 0)
    w = np.zeros(n, np.int32)
    ora.L.orc_export_state(ora.h, e, w.ctypes.data, n)
    k, rows = 8 + 2 * int(w[6]), []
    for _ in range(ora.n_snakes):
        ln = int(w[k])
        head = [int(w[k + 6]), int(w[k + 7])] if ln else [-2, -2]
        rows.append([ln] + head + [int(v) for v in w[k + 1:k + 6]])
        k += 6 + 2 * ln
    return np.array(rows, np.int32)


def _check_oracle(ora, cfg, frames, what):
    views = list(range(cp.n_views(cfg["rules"], cfg["n_snakes"])))
    want = cp.decode_frame(frames, views)
    for e in range(ora.num_envs):
        st = ora.get_state(e)
        got = cp.np_cells(st, cfg["dim"], cfg["n_snakes"], cfg["rules"], views)
        assert np.array_equal(got, want[e]), (what, e, st)
        assert np.array_equal(cp.np_snake_rows(st, cfg["n_snakes"]), _raw_rows(ora, e)), (what, e)
        # a subset of the views is the subset of the planes
        assert np.array_equal(cp.np_cells(st, cfg["dim"], cfg["n_snakes"], cfg["rules"], views[1:]), want[e][1:])


PLAY = [dict(rules=0, dim=19, n_snakes=3, n_fruits=3), dict(rules=0, dim=6, n_snakes=1, n_fruits=1),
        dict(rules=1, dim=10, n_snakes=4, n_fruits=5), dict(rules=1, dim=6, n_snakes=2, n_fruits=0),
        dict(rules=2, dim=10, n_snakes=3, n_fruits=3), dict(rules=2, dim=6, n_snakes=2, n_fruits=2)]


@pytest.mark.parametrize("cfg", PLAY, ids=lambda c: "r{rules}_{dim}x{n_snakes}".format(**c))
def test_helper_equals_the_decoded_frame_on_oracle_play(cfg):
    cfg = dict(cfg, num_envs=6, seed=5, env_id_base=3, max_steps=2000)
    ora = sp.make_oracle(cfg)
    _check_oracle(ora, cfg, ora.reset(), "reset")
    rng = np.random.default_rng(cfg["dim"])
    seen = set()
    for t in range(40):
        obs, *_ = ora.step(rng.integers(0, 5, (6, cfg["n_snakes"])).astype(np.int32))
        _check_oracle(ora, cfg, obs, t)
        seen |= set(np.unique(cp.decode_frame(obs, [0])).tolist())
    # (bodies of one cell show their head alone, and a new_world game may have no fruit: the codes every play must show)
    assert {0, 3} <= seen and (cfg["n_fruits"] == 0 or 1 in seen) and (cfg["n_snakes"] == 1 or 5 in seen), seen


def _check_hand_built(cfg, states):
    ora = sp.make_oracle(dict(cfg, num_envs=len(states), seed=1, env_id_base=0, max_steps=2000))
    ora.reset()
    for e, st in enumerate(states):
        ora.set_state(e, st)
    _check_oracle(ora, cfg, ora.render(), "hand-built")


@pytest.mark.parametrize("dim", [2, 3, 6, 19, 33, 62])
def test_helper_on_the_hand_built_snake_env_states(dim):
    states = cp.snake_env_states(dim)
    if dim >= 19:
        assert max(len(b) for st in states for b in st["snakes"]) > 64
    _check_hand_built(dict(rules=0, dim=dim, n_snakes=3, n_fruits=3), states)
    # paint order decides: snake 0's head at (0, 0) lies under snake 2's body in the first paint-order state
    first = states[-8]
    assert first["snakes"][0] == [[0, 0]] and cp.np_cells(first, dim, 3, 0, [0, 2])[:, 0, 0].tolist() == [4, 2]


@pytest.mark.parametrize("nf", [0, 9, 32])
@pytest.mark.parametrize("ns", [1, 2, 4])
@pytest.mark.parametrize("dim", [6, 13])
def test_helper_on_the_hand_built_new_world_states(dim, ns, nf):
    states = cp.new_world_states(dim, ns, nf)
    assert sum(1 for st in states for s in range(ns) if not st["alive"][s] and st["snakes"][s]) >= 4   # dead, body kept
    _check_hand_built(dict(rules=1, dim=dim, n_snakes=ns, n_fruits=nf), states)


@pytest.mark.parametrize("dim,ns", [(10, 3), (6, 2)])
def test_helper_on_the_hand_built_adversarial_states(dim, ns):
    states = cp.adversarial_states(dim, ns)
    assert max(len(st["fruits"]) for st in states) > 64
    assert any(not (0 <= f[0] < dim and 0 <= f[1] < dim) for st in states for f in st["fruits"])
    _check_hand_built(dict(rules=2, dim=dim, n_snakes=ns, n_fruits=ns), states)


# ------------------------------------------------------------------------------------------ the wrapper's `views`
def test_views_are_normalised_to_a_mask_and_an_ascending_list():
    nv = vec_env.normalize_views
    assert nv(None, 3) == (0b111, [0, 1, 2]) and nv(None, 4) == (0b1111, [0, 1, 2, 3]) and nv(None, 1) == (1, [0])
    assert nv(2, 3) == (0b100, [2]) and nv(np.int64(0), 3) == (1, [0])
    assert nv([0, 2], 3) == (0b101, [0, 2]) and nv((1,), 3) == (0b10, [1]) and nv(range(1, 4), 4) == (0b1110, [1, 2, 3])
    assert nv(np.array([1, 3]), 4) == (0b1010, [1, 3])
    assert nv([], 3) == (0, [])
    for bad in (3, -1, [0, 3], [2, 0], [1, 1], [0.5], "01", True, [True]):
        with pytest.raises((ValueError, TypeError)):
            nv(bad, 3)
