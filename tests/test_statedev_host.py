"""CPU-side checks of the device-side state export / import / hash (msnake_export_states, msnake_import_states,
msnake_hash_states, msnake_state_words_max): the host hash against known answers and against a scalar pure-int
implementation, what BOARD ignores and what it does not, the word-count bound as a formula, dist.fingerprint and its
gloo all-gather, the prototypes, and the Python argument checks, which raise before any native call.  No GPU."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import board_states as bs
import msnake
import state_domain as sd
from msnake import _capi
from oracle.snake_oracle import state_to_flat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------ a second implementation
def mix64_int(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & M64
    return z ^ (z >> 31)


def hash_int(words, board=False):
    """The header's formula word by word, in Python ints."""
    total = 0
    for i, w in enumerate(int(x) for x in words):
        if board and i in (0, 1, 2, 4, 5):
            continue
        if board and i == 7:
            w &= ~0x100
        total = (total + mix64_int(((i + 1) << 32) | (w & 0xFFFFFFFF))) & M64
    return total


A = [5, 9, 0, 0, 5, 0x3F800000, 1, 0x101, 4, 4, 3, 1, 0, 3, 1, 0, 2, 2, 1, 2, 0, 2]
B = [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 3, 1, 0]


def test_known_answers():
    for h in (lambda w, what: msnake.state_hash(np.array(w, np.int32), what), lambda w, what: hash_int(w, what == "board")):
        assert h(A, "full") == 0xfca7cf3b97cf07f0 and h(A, "board") == 0x5c3dcc5ab7b75d44
        assert h(A[:-2] + [-1, 2], "full") == 0x5e0a0c0f1f3c08c3
        assert h(B, "full") == 0xe1edeac8b51ad827 and h(B, "board") == 0x1ed8d10b7096a632
    # any integer dtype, lists, and the numeric `what` of the C-ABI
    assert msnake.state_hash(A) == msnake.state_hash(np.array(A, np.int64)) == msnake.state_hash(np.array(A, np.uint32), 0)
    assert msnake.state_hash(A, 1) == msnake.state_hash(A, "board")


STATES = None


def states_200():
    """200 word lists from the hand-built boards, under all three rule sets (the oracle's state_to_flat)."""
    global STATES
    if STATES is None:
        rng = np.random.default_rng(2024)
        out = []
        for rules, dim, ns, nf in (("snake_env", 10, 3, 3), ("new_world", 6, 4, 5), ("adversarial", 10, 3, 3)):
            sts = bs.random_states(dim, ns, nf, rng, 40) + bs.dense_states(dim, ns, nf, rng, 16)
            for i, st in enumerate(sts):
                st.update(t=int(rng.integers(0, 500)), ctr=int(rng.integers(0, 1 << 40)), ep_len=int(rng.integers(0, 500)),
                          ep_return=float(rng.integers(-9, 9)), spare_fruits=int(rng.integers(0, 3)), finished=bool(i % 5 == 0))
                if rules == "adversarial":   # a list of its own length, sometimes past 64 entries, with off-grid entries
                    st["fruits"] = [[int(v) for v in rng.integers(-1, dim + 1, 2)] for _ in range(int(rng.integers(0, 90)))]
                if rules == "new_world":
                    st["alive"] = [bool(v) for v in rng.integers(0, 2, ns)]
                    st["in_dead"] = [bool(v) for v in rng.integers(0, 2, ns)]
            out += [state_to_flat(st, ns) for st in sts]
        over, _ = bs.overflow_states(12, 3)                                   # bodies past 64 pieces
        out += [state_to_flat(st, 3) for st in over]
        out += [state_to_flat(st, 3) for st in bs.dense_states(19, 3, 3, rng, 200 - len(out))]
        assert len(out) == 200 and max(len(w) for w in out) > 8 + 6 + 6 * 3 + 2 * 64
        STATES = out
    return STATES


def test_state_hash_equals_the_scalar_implementation_on_200_states():
    for w in states_200():
        assert msnake.state_hash(w) == hash_int(w) and msnake.state_hash(w, "board") == hash_int(w, True)


def test_distinct_words_give_distinct_full_hashes():
    words = states_200()
    distinct = {tuple(int(x) for x in w) for w in words}
    assert len({msnake.state_hash(np.array(w, np.int32)) for w in distinct}) == len(distinct) > 190


def test_board_ignores_exactly_the_bookkeeping_words():
    rng = np.random.default_rng(3)
    for w in states_200()[::7]:
        base_b, base_f = msnake.state_hash(w, "board"), msnake.state_hash(w)
        v = w.copy()
        v[[0, 1, 2, 4, 5]] = rng.integers(-2**31, 2**31, 5)
        v[7] ^= 0x100
        assert msnake.state_hash(v, "board") == base_b and msnake.state_hash(v) != base_f
        for i in (0, 1, 2, 4, 5):        # each alone moves FULL
            v = w.copy()
            v[i] ^= 1
            assert msnake.state_hash(v) != base_f and msnake.state_hash(v, "board") == base_b


def test_board_changes_with_every_other_word():
    for w in (states_200()[0], states_200()[100], states_200()[-1], np.array(A, np.int32)):
        base = msnake.state_hash(w, "board")
        for i in range(len(w)):
            if i in (0, 1, 2, 4, 5):
                continue
            for flip in (1, 1 << 31) if i != 7 else (1, 0x200):
                v = w.copy()
                v[i] ^= np.int32(flip - (1 << 32) if flip >> 31 else flip)
                assert msnake.state_hash(v, "board") != base, (i, flip)
        # the same word at another index is another term: two words swapped change the hash
        v = w.copy()
        v[8], v[9] = w[9] + 1, w[8] + 1
        u = w.copy()
        u[8], u[9] = w[8] + 1, w[9] + 1
        assert msnake.state_hash(v, "board") != msnake.state_hash(u, "board") or w[8] == w[9]


@pytest.mark.parametrize("bad", [np.zeros(7, np.int32), np.zeros((2, 8), np.int32), np.zeros(9, np.float32)])
def test_state_hash_argument_errors(bad):
    with pytest.raises(ValueError, match="words must be"):
        msnake.state_hash(bad)


@pytest.mark.parametrize("what", ["FULL", "position", 2, -1, None, True])
def test_what_errors(what):
    with pytest.raises(ValueError, match="what must be"):
        msnake.state_hash(np.array(A), what)


# ------------------------------------------------------------------------------------------ the word-count bound
def words_max(cfg):
    """8 + 2 F + n_snakes (6 + 2 (cap - 2)), F = n_fruits or, under adversarial, fcap (include/msnake.h)."""
    F = sd.fcap(cfg) if cfg["rules"] == "adversarial" else cfg["n_fruits"]
    return 8 + 2 * F + cfg["n_snakes"] * (6 + 2 * (sd.cap(cfg) - 2))


def test_words_max_formula_covers_every_accepted_row():
    """(env.state_words_max itself needs a handle: tests/test_statedev_gpu.py compares it with this formula.)"""
    assert words_max(sd.CFGS["S5"]) == 8 + 6 + 3 * (6 + 2 * 62) and words_max(sd.CFGS["A5"]) == 8 + 2 * 128 + 3 * (6 + 2 * 62)
    for key in sd.TABLE_KEYS:
        cfg, longest = sd.CFGS[key], 0
        for name, build, expect in sd.rows(key):
            if expect is None:
                w = build()
                assert sd.accepts(cfg, w) is None
                longest = max(longest, sd.canonical_len(cfg, w))
                assert sd.canonical_len(cfg, w) <= words_max(cfg), (key, name)
        assert longest >= 8 + 2 * 3 + 6 * cfg["n_snakes"] + 2 * (sd.cap(cfg) - 2)   # (the table reaches a body of cap - 2)


# ------------------------------------------------------------------------------------------ dist.fingerprint
def fingerprint_int(hashes, base):
    return sum(mix64_int((int(h) & M64) + (base + e) * 0x9E3779B97F4A7C15) for e, h in enumerate(hashes)) & M64


def fake_hashes(n=96):
    return torch.from_numpy(np.random.default_rng(9).integers(-2**63, 2**63, n, dtype=np.int64))


def test_fingerprint_is_independent_of_the_sharding():
    h = fake_hashes()
    whole = msnake.fingerprint(h, 0)
    assert whole == fingerprint_int(h.tolist(), 0) and 0 <= whole <= M64
    assert msnake.fingerprint(h, 1000) == fingerprint_int(h.tolist(), 1000) != whole
    for world in (2, 3, 5, 96):
        parts = [msnake.shard_range(len(h), r, world) for r in range(world)]
        assert sum(msnake.fingerprint(h[s:s + c], s) for s, c in parts) & M64 == whole
    assert msnake.fingerprint(h[:0], 7) == 0


def test_fingerprint_depends_on_which_env_holds_which_hash():
    h = fake_hashes()
    whole = msnake.fingerprint(h, 0)
    swapped = h.clone()
    swapped[[3, 50]] = h[[50, 3]]
    assert msnake.fingerprint(swapped, 0) != whole
    assert msnake.fingerprint(h.flip(0), 0) != whole and msnake.fingerprint(torch.roll(h, 1), 0) != whole
    one = h.clone()
    one[17] ^= 1
    assert msnake.fingerprint(one, 0) != whole


@pytest.mark.parametrize("bad", [[1, 2, 3], torch.zeros(4, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64)])
def test_fingerprint_argument_errors(bad):
    with pytest.raises(ValueError, match="hashes must be"):
        msnake.fingerprint(bad, 0)
    with pytest.raises(ValueError, match="env_id_base"):
        msnake.fingerprint(torch.zeros(2, dtype=torch.int64), -1)


class FakeHashEnv:
    """What dist.all_fingerprint asks of an env: hash_states_device() and the configured env_id_base."""

    def __init__(self, start, count):
        self.cfg, self._h = _capi.MsnakeConfig(env_id_base=start), fake_hashes()[start:start + count]

    def hash_states_device(self, what="full"):
        assert what == "full"
        return self._h


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    start, count = msnake.shard_range(96, rank, world)
    q.put((rank, msnake.all_fingerprint(FakeHashEnv(start, count))))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_all_fingerprint_equals_the_single_process_value():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    single = msnake.all_fingerprint(FakeHashEnv(0, 96))      # no process group here: the single-rank identity
    assert single == msnake.fingerprint(fake_hashes(), 0)
    assert res == {0: single, 1: single}


# ------------------------------------------------------------------------------------------ the C entry points
PROTOS = {"msnake_state_words_max": (ctypes.c_int32, [ctypes.c_void_p]),
          "msnake_export_states": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]),
          "msnake_import_states": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32,
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
          "msnake_hash_states": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p])}


def test_header_declares_and_library_exports_the_entry_points():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    for decl in (r"int32_t msnake_state_words_max\(msnake_handle h\);",
                 r"int msnake_export_states\(msnake_handle h, int32_t\* words_dev, int32_t stride, int32_t\* count_dev, void\* stream\);",
                 r"int msnake_import_states\(msnake_handle h, const uint8_t\* mask_dev, const int32_t\* words_dev, int32_t stride,\s+"
                 r"const int32_t\* count_dev, uint8_t\* status_dev, void\* stream\);",
                 r"int msnake_hash_states\(msnake_handle h, uint32_t what, uint64_t\* hash_dev, void\* stream\);"):
        assert re.search(decl, text), decl
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert re.search(r"^ \*   msnake_export_states / msnake_import_states / msnake_hash_states", text, re.M)
    lib = _capi.load()
    for name, (restype, argtypes) in PROTOS.items():
        assert name in _capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_public_codes_match_the_header_and_the_internal_numbering():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    pub = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define MSNAKE_STATE_(\w+) (0x[0-9A-Fa-f]+|\d+)", text)}
    assert pub == {"OK": 0, "TOO_SHORT": 1, "SNAKE_COUNT": 2, "FRUIT_COUNT": 3, "CELL": 4, "LENGTH": 5, "SCALAR": 6, "SKIPPED": 0xFF}
    assert (pub["TOO_SHORT"], pub["SNAKE_COUNT"], pub["FRUIT_COUNT"], pub["CELL"], pub["LENGTH"], pub["SCALAR"]) == \
        (sd.R_SHORT, sd.R_SNAKES, sd.R_FRUITS, sd.R_CELL, sd.R_LEN, sd.R_SCALAR)
    assert [getattr(_capi, "STATE_" + k) for k in pub] == list(pub.values())
    internal = open(os.path.join(os.path.dirname(_capi.__file__), "csrc", "msnake_internal.h")).read()
    for k, name in (("SHORT", "TOO_SHORT"), ("SNAKES", "SNAKE_COUNT"), ("FRUITS", "FRUIT_COUNT"), ("CELL", "CELL"), ("LEN", "LENGTH"),
                    ("SCALAR", "SCALAR")):
        assert int(re.search(rf"MSNAKE_ST_{k} = (\d+)", internal).group(1)) == pub[name]
    assert re.search(r"#define MSNAKE_HASH_FULL 0u", text) and re.search(r"#define MSNAKE_HASH_BOARD 1u", text)
    assert _capi.HASH_WHAT == {"full": 0, "board": 1}


def test_null_handles_are_refused():
    lib = _capi.load()
    dead = ctypes.create_string_buffer(4)
    buf = ctypes.create_string_buffer(64)
    for h in (None, dead):
        assert lib.msnake_state_words_max(h) == -3  # MSNAKE_E_HANDLE
        assert lib.msnake_export_states(h, buf, 8, buf, None) == -3
        assert lib.msnake_import_states(h, None, buf, 8, None, buf, None) == -3
        assert lib.msnake_hash_states(h, 0, buf, None) == -3
        assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ the Python argument checks
class NoNativeCalls:
    def __getattr__(self, name):
        raise AssertionError(f"native call {name} behind a bad argument")


def stub_env(n=4):
    """A MultiSnakeVecEnv without a handle, on the CPU: every native call fails the test."""
    env = object.__new__(msnake.MultiSnakeVecEnv)
    env.__dict__.update(_torch=torch, device=torch.device("cpu"), num_envs=n, n_snakes=3, _pending=None, _L=NoNativeCalls(),
                        _h=None, closed=True, _track_stale=False)
    return env


def test_methods_exist_on_the_env_class():
    cls = msnake.MultiSnakeVecEnv
    assert isinstance(cls.state_words_max, property)
    assert callable(cls.export_states_device) and callable(cls.import_states_device) and callable(cls.hash_states_device)
    assert callable(msnake.state_hash) and callable(msnake.fingerprint) and callable(msnake.all_fingerprint)


def test_import_argument_checks_raise_before_any_native_call():
    env, i32 = stub_env(), torch.int32
    good = torch.zeros((4, 16), dtype=i32)
    for bad in (torch.zeros((4, 16), dtype=torch.int64), torch.zeros((3, 16), dtype=i32), torch.zeros(64, dtype=i32),
                torch.zeros((16, 4), dtype=i32).t(), np.zeros((4, 16), np.int32)):
        with pytest.raises(ValueError, match="words must be a contiguous int32"):
            env.import_states_device(bad)
    with pytest.raises(ValueError, match="at least 8 columns"):
        env.import_states_device(torch.zeros((4, 7), dtype=i32))
    with pytest.raises(ValueError, match="count must be"):
        env.import_states_device(good, count=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="count must be"):
        env.import_states_device(good, count=torch.zeros(5, dtype=i32))
    with pytest.raises(ValueError, match="status_out must be"):
        env.import_states_device(good, status_out=torch.zeros(4, dtype=torch.int8))
    with pytest.raises(ValueError, match="mask"):
        env.import_states_device(good, mask=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(ValueError, match="env indices"):
        env.import_states_device(good, mask=[4])
    assert env._track_stale is False            # nothing was installed
    env._pending = (None,) * 4
    with pytest.raises(RuntimeError, match="between step_async"):
        env.import_states_device(good)


def test_export_and_hash_argument_checks_raise_before_any_native_call():
    env, i32 = stub_env(), torch.int32
    with pytest.raises(ValueError, match="out must be a contiguous int32"):
        env.export_states_device(out=torch.zeros((4, 16), dtype=torch.int16))
    with pytest.raises(ValueError, match="differs from out's row length"):
        env.export_states_device(out=torch.zeros((4, 16), dtype=i32), stride=17)
    with pytest.raises(ValueError, match="count_out must be"):
        env.export_states_device(out=torch.zeros((4, 16), dtype=i32), count_out=torch.zeros((4, 1), dtype=i32))
    for stride in (0, -1, 2**31, 2.5, True):
        with pytest.raises(ValueError, match="stride must"):
            env.export_states_device(stride=stride)
    with pytest.raises(ValueError, match="nothing to write"):
        env.export_states_device(words=False, count=False)
    with pytest.raises(ValueError, match="what must be"):
        env.hash_states_device("position")
    with pytest.raises(ValueError, match="out must be a contiguous int64"):
        env.hash_states_device(out=torch.zeros(4, dtype=i32))
    with pytest.raises(ValueError, match="out must be a contiguous int64"):
        env.hash_states_device(out=torch.zeros(5, dtype=torch.int64))
