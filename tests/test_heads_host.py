"""CPU-side checks of the head distances, the Voronoi owner map and the owned counts (msnake_head_fields,
MultiSnakeVecEnv.head_fields_device and its three one-output forms): the entry point is declared, exported, bound and
refuses a NULL handle before it touches the GPU; the helper tests/heads_play.py on hand-computed boards and on the
identities that tie it to territory_play, path_play and space_play; the wrapper's calls and refusals on a fake env.
No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import board_states as bs
import heads_play as hp
import msnake
import path_play as pp
import space_play as spp
import territory_play as tp
from fake_envs import FakeLocalEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T, O = hp.NONE, hp.OWNER_TIE, hp.OWNER_NONE
_st = bs.state


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    sig = (r"\bint msnake_head_fields\(msnake_handle h, uint32_t snake_mask, uint16_t\* dist_dev, uint8_t\* owner_dev,\s*"
           r"uint16_t\* counts_dev, void\* stream\);")
    assert re.search(sig, text)
    assert re.search(r"#define MSNAKE_HEAD_NONE\s+0xFFFFu\b", text) and N == 0xFFFF
    assert re.search(r"#define MSNAKE_OWNER_TIE\s+0xFEu\b", text) and T == 0xFE
    assert re.search(r"#define MSNAKE_OWNER_NONE\s+0xFFu\b", text) and O == 0xFF
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert "msnake_head_fields" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_head_fields is not None and lib.msnake_abi_version() == 3


def test_the_binding_has_the_declared_signature_and_the_constants_are_exported():
    restype, argtypes = msnake._capi.PROTOTYPES["msnake_head_fields"]
    vp = ctypes.c_void_p
    assert restype is ctypes.c_int and argtypes == [vp, ctypes.c_uint32, vp, vp, vp, vp]
    fn = msnake._capi.load().msnake_head_fields
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes
    assert (msnake.HEAD_NONE, msnake.OWNER_TIE, msnake.OWNER_NONE) == (0xFFFF, 0xFE, 0xFF)
    assert {"HEAD_NONE", "OWNER_TIE", "OWNER_NONE"} <= set(msnake.__all__)
    for name in ("head_fields_device", "head_distances_device", "owner_map_device", "owned_counts_device", "head_fields_shape"):
        assert callable(getattr(msnake.MultiSnakeVecEnv, name))


def test_null_handle_is_refused():
    lib = msnake._capi.load()
    assert lib.msnake_head_fields(None, 1, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


# ------------------------------------------------------------------------------------------ hand-computed boards
def _heads(st, dim, ns):
    D, owner, counts = hp.np_heads(st, dim, ns)
    assert D.shape == (ns, dim, dim) and owner.shape == (dim, dim) and owner.dtype == np.uint8 and counts.shape == (ns,)
    return D.tolist(), owner.tolist(), counts.tolist()


def test_empty_3x3_with_two_heads_in_opposite_corners():
    D, owner, counts = _heads(_st([[(0, 0)], [(2, 2)]], [(1, 1)] * 2), 3, 2)
    assert D[0] == [[0, 1, 2], [1, 2, 3], [2, 3, N]]          # the L1 distance from (0, 0); the other head is in `used`
    assert D[1] == [[N, 3, 2], [3, 2, 1], [2, 1, 0]]
    assert owner == [[O, 0, T], [0, T, 1], [T, 1, O]]          # the tie diagonal c0 + c1 = 2
    assert counts == [2, 2]


@pytest.mark.parametrize("dim,want_owner,want_counts", [(5, [0, T, 1], [1, 1]), (6, [0, 0, 1, 1], [2, 2])])
def test_a_corridor_raced_from_both_ends(dim, want_owner, want_counts):
    """Row c1 = 0 is the corridor, snake 2 lies along row c1 = 1 and owns what is behind it: odd length, the middle cell
    is a tie; even length, none is."""
    wall = [(x, 1) for x in range(dim)]
    D, owner, counts = _heads(_st([[(0, 0)], [(dim - 1, 0)], wall], [(2, 2)] * 3), dim, 3)
    for x in range(1, dim - 1):
        assert D[0][x][0] == x and D[1][x][0] == dim - 1 - x and D[2][x][0] == N
    assert D[0][0][0] == 0 and D[0][dim - 1][0] == N and D[1][dim - 1][0] == 0 and D[1][0][0] == N
    assert [owner[x][0] for x in range(1, dim - 1)] == want_owner
    for x in range(dim):
        assert owner[x][1] == O and D[0][x][1] == N and D[1][x][1] == N and D[2][x][1] == (0 if x == 0 else N)
        for y in range(2, dim):       # behind the wall: the wall's head at (0, 1) enters by (0, 2)
            assert D[2][x][y] == 1 + x + (y - 2) and owner[x][y] == 2 and D[0][x][y] == N and D[1][x][y] == N
    assert counts == want_counts + [dim * (dim - 2)]


def test_a_pocket_whose_mouth_the_other_snake_reaches_first():
    """Row c1 = 0 up to c0 = 2 is a pocket under snake 0's far pieces; snake 1 stands at its mouth.  Snake 0's front
    still runs through it: its plane is finite there, and the pocket is snake 1's."""
    st = _st([[(4, 4), (0, 1), (1, 1), (2, 1)], [(4, 0)]], [(2, 2)] * 2)
    D, owner, counts = _heads(st, 5, 2)
    assert [D[1][x][0] for x in range(5)] == [4, 3, 2, 1, 0]
    assert [D[0][x][0] for x in range(5)] == [8, 7, 6, 5, N]
    assert [owner[x][0] for x in range(5)] == [1, 1, 1, 1, O]
    assert D[0][0][2] == 6 and D[1][0][2] == 6 and owner[0][2] == T
    assert [owner[x][1] for x in range(5)] == [O, O, O, 1, 1] and D[0][4][4] == 0 and D[1][4][4] == N
    assert sum(counts) + sum(r.count(T) for r in owner) == 25 - 5


def test_a_snake_with_no_open_move():
    D, owner, counts = _heads(_st([[(0, 0)], [(2, 2), (1, 0), (0, 1)]], [(1, 1)] * 2), 3, 2)
    assert D[0] == [[0, N, N], [N, N, N], [N, N, N]]
    assert D[1] == [[N, N, 2], [N, 2, 1], [2, 1, 0]]
    assert owner == [[O, O, 1], [O, 1, 1], [1, 1, O]] and counts == [0, 5]


def test_a_head_outside_the_grid_with_one_open_move():
    D, owner, counts = _heads(_st([[(-1, 1)]], [(1, 1)]), 3, 1)
    assert D[0] == [[2, 1, 2], [3, 2, 3], [4, 3, 4]]           # 1 + c0 + |c1 - 1|: no cell holds the head's 0
    assert owner == [[0] * 3] * 3 and counts == [9]


def test_two_heads_stacked_on_one_cell():
    D, owner, counts = _heads(_st([[(1, 1)], [(1, 1)]], [(0, 0)] * 2), 3, 2)
    assert D[0] == D[1] == [[2, 1, 2], [1, 0, 1], [2, 1, 2]]   # each plane holds its head's 0 under the other piece
    assert owner == [[T, T, T], [T, O, T], [T, T, T]] and counts == [0, 0]


def test_an_empty_body():
    D, owner, counts = _heads(_st([[(0, 0)], []], [(1, 1)] * 2), 2, 2)
    assert D[0] == [[0, 1], [1, 2]] and D[1] == [[N, N], [N, N]]
    assert owner == [[O, 0], [0, 0]] and counts == [3, 0]


@pytest.mark.parametrize("dim", [6, 33, 62])
def test_the_serpentine_in_closed_form(dim):
    """Snake 0 on the corridor's first cell: distance k at the k-th corridor cell.  (The corridor of the maze has
    (dim / 2) (dim + 1) cells, 1 953 at dim 62: its far end holds 1 952.  dim^2 - 1 = 3 843 bounds every board and is
    reached by none: a path through every cell of a grid is never a shortest one.)  The wall snake's head at (0, 1)
    enters the corridor at (0, 2), corridor cell 2 dim."""
    walls, corridor = spp.serpentine(dim)
    L = len(corridor)
    assert L == (dim // 2) * (dim + 1) + (dim % 2) * dim and walls[0] == (0, 1) and corridor[2 * dim] == (0, 2)
    D, owner, counts = hp.np_heads(_st([[corridor[0]], walls], [(0, 0)] * 2), dim, 2)
    for k, c in enumerate(corridor):
        assert D[0][c] == k and D[1][c] == (N if k == 0 else 1 + abs(k - 2 * dim))
        assert owner[c] == (O if k == 0 else 0 if k <= dim else 1)
    assert D[0][corridor[-1]] == L - 1 == {6: 20, 33: 576, 62: 1952}[dim]
    assert (D[0] != N).sum() == L and counts.tolist() == [dim, L - 1 - dim]
    for c in walls:
        assert D[0][c] == N and D[1][c] == (0 if c == walls[0] else N) and owner[c] == O


# ------------------------------------------------------------------------------------------ identities
def _boards():
    """(dim, ns, state) of at least 400 boards: random, border, dense and tie states at dims 2, 3, 6, 19 and 33 with
    1 to 4 snakes."""
    out = []
    for dim, n_rand, n_dense in ((2, 12, 0), (3, 12, 6), (6, 12, 8), (19, 6, 5), (33, 2, 2)):
        for ns in (1, 2, 3, 4):
            rng = np.random.default_rng([29, dim, ns])
            states = bs.random_states(dim, ns, ns, rng, n_rand, dup=True)
            border = bs.border_states(dim, ns, ns, rng)
            states += border if dim <= 6 else border[:6] + border[-12::3]
            if n_dense and dim >= 3:
                states += bs.dense_states(dim, ns, ns, rng, n_dense)
            if ns == 2 and dim in (6, 19):
                states += bs.tie_states(dim)
            out += [(dim, ns, st) for st in states]
    return out


def test_identities_with_territory_path_and_space():
    boards = _boards()
    assert len(boards) >= 400 and {b[0] for b in boards} == {2, 3, 6, 19, 33} and {b[1] for b in boards} == {1, 2, 3, 4}
    seen = {"tie": 0, "none": 0, "walled": 0, "outside": 0}
    for dim, ns, st in boards:
        D, owner, counts = hp.np_heads(st, dim, ns)
        targets, occ = tp.open_targets(st, dim, ns)
        free = ~occ
        terr, space = tp.np_territory(st, dim, ns), spp.np_space(st, dim, ns)
        field = pp.np_field(st, dim)
        path = pp.np_path(st, dim, ns, field)
        assert (owner[occ] == O).all() and counts.sum() == (owner < ns).sum()
        seen["tie"] += int((owner == T).any())
        seen["none"] += int((owner[free] == O).any())
        for s in range(ns):
            body = st["snakes"][s] if s < len(st["snakes"]) else []
            fin = D[s] != N
            # 1. owner == s exactly where some open move of s gets there strictly before every other snake
            mine = np.zeros((dim, dim), bool)
            if targets[s]:
                dB = tp.bfs(occ, dim, [t for j in range(ns) if j != s for t in targets[j].values()])
                for t in targets[s].values():
                    dA = tp.bfs(occ, dim, [t])
                    mine |= free & (dA < dB) & (dA < tp.INF)
            assert np.array_equal(owner == s, mine), (dim, ns, s, st)
            # 2. the counts between the largest and the sum of the per-move territories
            assert terr[s].max() <= counts[s] <= terr[s].sum(), (dim, ns, s, st)
            # 3. the distance to food, through the field's sources
            src = free & (field == 0)
            best = int(path[s].min())
            want = N if best == pp.NONE or not src.any() else 1 + best
            got = int(D[s][src].min()) if src.any() else N
            assert got == want, (dim, ns, s, st)
            # 4. the finite free cells between the largest and the sum of the per-move spaces
            reached = int((fin & free).sum())
            assert space[s].max() <= reached <= space[s].sum(), (dim, ns, s, st)
            seen["walled"] += int(0 < reached < free.sum())
            # 5. neighbouring free cells with finite distances differ by at most 1
            both = fin & free
            for ax in (0, 1):
                a, b = np.moveaxis(D[s], ax, 0), np.moveaxis(both, ax, 0)
                pair = b[1:] & b[:-1]
                assert (np.abs(a[1:] - a[:-1])[pair] <= 1).all(), (dim, ns, s, st)
            # 6. finite and >= 1 implies free; the only 0 is the head
            assert free[fin & (D[s] >= 1)].all() and (D[s][fin] <= dim * dim - 1).all()
            zeros = np.argwhere(D[s] == 0).tolist()
            on_board = bool(body) and 0 <= body[0][0] < dim and 0 <= body[0][1] < dim
            assert zeros == ([[int(body[0][0]), int(body[0][1])]] if on_board else []), (dim, ns, s, st)
            seen["outside"] += int(bool(body) and not on_board and fin.any())
        # 7. one snake: it owns exactly what it reaches
        if ns == 1:
            assert np.array_equal(owner == 0, (D[0] != N) & free), (dim, st)
    assert min(seen.values()) >= 5, seen


# ------------------------------------------------------------------------------------------ the wrapper on a fake env
class _FakeLib:
    def __init__(self):
        self.calls = []

    def msnake_head_fields(self, *a):
        self.calls.append(a)
        return 0


def _fake_env(n=5, ns=3, dim=7):
    """fake_envs.FakeLocalEnv with what head_fields_device touches; MultiSnakeVecEnv's methods are called on it."""
    env = FakeLocalEnv(n=n, n_snakes=ns)
    lib = _FakeLib()
    env._torch, env._L, env._h, env._heads_fn = torch, lib, 1234, lib.msnake_head_fields
    env.cfg = types.SimpleNamespace(dim=dim)
    env._cur_stream = lambda dev: types.SimpleNamespace(cuda_stream=77)
    for name in ("_checked", "head_fields_device", "head_distances_device", "owner_map_device", "owned_counts_device",
                 "head_fields_shape"):
        setattr(env, name, types.MethodType(getattr(msnake.MultiSnakeVecEnv, name), env))
    return env, lib


def test_the_wrapper_passes_mask_pointers_and_stream_and_returns_what_it_wrote():
    env, lib = _fake_env()
    dist3 = torch.zeros((5, 3, 7, 7), dtype=torch.uint16)
    dist2 = torch.zeros((5, 2, 7, 7), dtype=torch.uint16)
    owner = torch.zeros((5, 7, 7), dtype=torch.uint8)
    counts = torch.zeros((5, 3), dtype=torch.uint16)
    assert env.head_fields_shape() == (3, 7, 7) and env.head_fields_shape([0, 2]) == (2, 7, 7) and env.head_fields_shape(1) == (1, 7, 7)
    got = env.head_fields_device(dist_out=dist3, owner_out=owner, counts_out=counts)
    assert len(got) == 3 and got[0] is dist3 and got[1] is owner and got[2] is counts          # the return order
    assert lib.calls[-1] == (1234, 0b111, dist3.data_ptr(), owner.data_ptr(), counts.data_ptr(), 77)
    got = env.head_fields_device([0, 2], dist_out=dist2, counts_out=counts, owner=False)
    assert len(got) == 2 and got[0] is dist2 and got[1] is counts
    assert lib.calls[-1] == (1234, 0b101, dist2.data_ptr(), None, counts.data_ptr(), 77)
    assert env.head_distances_device([0, 2], out=dist2) is dist2
    assert lib.calls[-1] == (1234, 0b101, dist2.data_ptr(), None, None, 77)
    assert env.owner_map_device(out=owner) is owner
    assert lib.calls[-1] == (1234, 0, None, owner.data_ptr(), None, 77)                        # no plane: no mask
    assert env.owned_counts_device(out=counts) is counts
    assert lib.calls[-1] == (1234, 0, None, None, counts.data_ptr(), 77)
    got = env.head_fields_device(1, owner_out=owner, counts_out=counts, dist=False)            # the selection alone writes nothing
    assert got[0] is owner and got[1] is counts and lib.calls[-1][:3] == (1234, 0, None)


def test_the_wrapper_refuses_before_any_call():
    env, lib = _fake_env()
    owner = torch.zeros((5, 7, 7), dtype=torch.uint8)
    for snakes in ([], [2, 0], [0, 0], [3], -1, "01", 1.5):
        with pytest.raises(ValueError, match="snake"):
            env.head_fields_device(snakes, owner_out=owner, dist=False, counts=False)
        with pytest.raises(ValueError, match="snake"):
            env.head_fields_shape(snakes)
    with pytest.raises(ValueError, match="nothing to write"):
        env.head_fields_device(dist=False, owner=False, counts=False)
    bad = {"dist_out": [torch.zeros((5, 2, 7, 7), dtype=torch.uint16), torch.zeros((5, 3, 7, 7), dtype=torch.int16),
                        torch.zeros((5, 3, 7, 14), dtype=torch.uint16)[..., ::2], np.zeros((5, 3, 7, 7), np.uint16)],
           "owner_out": [torch.zeros((5, 7, 7), dtype=torch.uint16), torch.zeros((5, 1, 7, 7), dtype=torch.uint8),
                         torch.zeros((4, 7, 7), dtype=torch.uint8)],
           "counts_out": [torch.zeros((5, 3, 4), dtype=torch.uint16), torch.zeros((5, 3), dtype=torch.int32),
                          torch.zeros((5, 4), dtype=torch.uint16)]}
    for kw, tensors in bad.items():
        for t in tensors:
            with pytest.raises(ValueError, match=kw):
                env.head_fields_device(**{kw: t}, dist=False, owner=False, counts=False)
    with pytest.raises(ValueError, match="dist_out"):      # the plane count follows the selection
        env.head_fields_device([1], dist_out=torch.zeros((5, 3, 7, 7), dtype=torch.uint16), owner=False, counts=False)
    with pytest.raises(ValueError, match="owner_out"):
        env.owner_map_device(out=torch.zeros((5, 7, 7), dtype=torch.int8))
    assert lib.calls == []
