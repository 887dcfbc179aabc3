"""Device-side env copies between handles (msnake_copy_envs, MultiSnakeVecEnv.copy_envs_device / clone).

Expected values never come from the call under test.  They are (a) the canonical words that get_state_all exported
from the SOURCE before the copy, (b) the CPU oracle after orc_import_state(dst, e, orc_export_state(src, idx[e])) --
the same Philox contract, env_id_base + e --, or (c) the first pass of a play, for the rollback test.  Every
comparison is bit-exact, over every env and every output byte.
"""
import ctypes

import numpy as np
import pytest

import scripted_play as sp
from state_domain import assert_words, blob_words, export as ora_words

pytestmark = pytest.mark.gpu

CFGS = {"S": dict(rules="snake_env", dim=10, n_snakes=3, n_fruits=3),
        "A": dict(rules="adversarial", dim=10, n_snakes=3, n_fruits=3),
        "N4": dict(rules="new_world", dim=10, n_snakes=4, n_fruits=4),
        "N2": dict(rules="new_world", dim=10, n_snakes=2, n_fruits=4),
        "S19": dict(rules="snake_env", dim=19, n_snakes=3, n_fruits=3)}
ORACLE_KW = ("seed", "env_id_base", "max_steps", "auto_reset")


# ------------------------------------------------------------------------------------------ helpers
class Pair:
    """A MultiSnakeVecEnv and the oracle of the same configuration, stepped together and compared in everything."""

    def __init__(self, key, n, threads=1, **kw):
        import msnake
        from oracle.snake_oracle import Oracle
        cfg = CFGS[key]
        self.env = msnake.MultiSnakeVecEnv(n, **cfg, **kw)
        self.ora = Oracle(n, **cfg, **{k: kw[k] for k in ORACLE_KW if k in kw})
        self.key, self.n, self.ns, self.K, self.threads = key, n, cfg["n_snakes"], kw.get("obs_scale", 1), threads

    def up(self, obs):
        return obs if self.K == 1 else obs.repeat(self.K, axis=1).repeat(self.K, axis=2)   # pixel replication

    def reset(self):
        assert np.array_equal(self.env.reset(), self.up(self.ora.reset()))
        return self

    def step(self, act, what=None):
        obs, rew, done, infos = self.env.step(act)
        o_obs, o_rew, o_done, o_ns, o_er, o_el = self.ora.step(act, threads=self.threads)
        assert np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), what
        assert np.array_equal(infos._ns, o_ns) and np.array_equal(infos._r, o_er) and np.array_equal(infos._l, o_el), what
        want = self.up(o_obs)
        assert np.array_equal(obs, want), (what, "obs of envs", np.nonzero((obs != want).reshape(self.n, -1).any(1))[0][:16].tolist())
        return obs, rew, done, np.stack([infos._ns, infos._r.view(np.int32), infos._l], 1)

    def play(self, steps, rng, what=None):
        """Pseudo-random actions that include the invalid codes -1 and 5, as the parity tests use."""
        for t in range(steps):
            self.step(rng.integers(-1, 6, (self.n, self.ns)).astype(np.int32), (what, t))
        return self

    def install(self, e, st):
        from oracle.snake_oracle import state_to_flat
        self.env.set_state_words(e, state_to_flat(st, self.ns))
        self.ora.set_state(e, st)

    def words(self):
        return blob_words(self.env.get_state_all())

    def check_states(self, what=None):
        from oracle.snake_oracle import flat_to_state
        read = sp._StateReader(self.ora)
        for e, w in enumerate(self.words()):
            assert flat_to_state(w) == read(e), (what, e)
            assert bool(w[7] & 0x100) == self.ora.finished(e), (what, e, "finished")

    def close(self):
        assert self.env.stats()["errors"] == 0
        self.env.close()


def ora_copy(o_dst, o_src, idx):
    """orc_dst.set_state(e, orc_src.get_state(idx[e])) for every selected e; all sources are read first."""
    idx = range(o_dst.num_envs) if idx is None else [int(i) for i in idx]
    bufs = {i: ora_words(o_src, i) for i in set(idx) if 0 <= i < o_src.num_envs}
    for e, i in enumerate(idx):
        if i in bufs:
            assert o_dst.L.orc_import_state(o_dst.h, e, bufs[i].ctypes.data, len(bufs[i])) == 0, (e, i)


def expected_words(src_before, dst_before, idx):
    idx = range(len(dst_before)) if idx is None else idx
    return [src_before[i] if 0 <= i < len(src_before) else dst_before[e] for e, i in enumerate(idx)]


def copy_both(dst, src, idx, what=None, via="numpy"):
    """The copy on the library and on the oracles, with the three word checks: the selected destination envs hold the
    source's words from BEFORE the call, the others their own, and the source is unchanged."""
    import torch
    s0, d0 = src.words(), dst.words()
    if idx is None or via == "numpy":
        dst.env.copy_envs_device(src.env, idx)
    elif via == "list":
        dst.env.copy_envs_device(src.env, [int(i) for i in idx])
    else:  # a device tensor of the given dtype
        dst.env.copy_envs_device(src.env, torch.from_numpy(np.asarray(idx)).to(device=dst.env.device, dtype=via))
    assert_words(dst.words(), expected_words(s0, d0, idx), (what, "dst"))
    assert_words(src.words(), s0, (what, "src"))
    ora_copy(dst.ora, src.ora, idx)
    dst.check_states(what)


def fixed_index(rng, n_dst, n_src, forced=()):
    """A random map with -1 entries, duplicates and unused sources; `forced`: (destination, source) pairs."""
    idx = rng.integers(-1, n_src, n_dst).astype(np.int64)
    idx[rng.choice(n_dst, max(2, n_dst // 8), replace=False)] = -1
    for e, i in forced:
        idx[e] = i
    sel = idx[idx >= 0]
    assert (idx < 0).any() and len(set(sel.tolist())) < len(sel) and len(set(sel.tolist())) < n_src
    return idx


# ------------------------------------------------------------------------------------------ hand-built states
def _path(dim):
    out = []
    for y in range(dim):
        out += [(x, y) for x in (range(dim) if y % 2 == 0 else range(dim - 1, -1, -1))]
    return out


PATH = _path(10)
LONG, SETUP = 78, 10      # the long body's cells and the steps the source takes after the install
ACT_OF = {d: a for a, d in sp.DIRS.items()}


def _st(snakes, fruits, vels=None, alive=None, in_dead=None, ctr=40, spare=0, grow=None):
    n = len(snakes)
    return {"t": 3, "ctr": ctr, "spare_fruits": spare, "ep_len": 3, "ep_return": 1.0, "fruits": [list(f) for f in fruits],
            "snakes": [[list(c) for c in b] for b in snakes], "vels": [list(v) for v in (vels or [(1, 0)] * n)],
            "grow_to": grow or [max(len(b), 3) for b in snakes], "alive": alive or [True] * n, "in_dead": in_dead or [False] * n}


def _fruits(key):
    return PATH[100 - CFGS[key]["n_fruits"]:]      # the far end of the last row


def _short(ns):
    return [[(4, 4), (3, 4)], [(6, 6)], [(7, 2)], [(1, 8)]][:ns]


def phase1_states(key):
    """Installed before the source's SETUP steps: {env: state}."""
    ns = CFGS[key]["n_snakes"]
    body = [PATH[LONG - 1 - i] for i in range(LONG)]
    v_long = (body[0][0] - body[1][0], body[0][1] - body[1][1])
    out = {1: _st([body] + [[]] * (ns - 1), _fruits(key), vels=[v_long] + [(0, 0)] * (ns - 1)),    # long body, empty bodies
           7: _st(_short(ns), _fruits(key), ctr=(3 << 32) + 17),                                     # ctr_hi != 0
           8: _st(_short(ns), _fruits(key), ctr=(1 << 32) - 2),                                      # ... or about to be
           9: _st([[(9, 5), (8, 5)]] + _short(ns)[1:], _fruits(key))}                                # runs into the wall
    if key == "A":
        out[2] = _st(_short(ns), [((i * 7) % 12 - 1, (i * 5) % 12 - 1) for i in range(70)], spare=5)   # 70 list entries
    return out


def phase2_states(key):
    """Installed after them: what a step would change at once (a head outside the grid, the alive bits)."""
    ns = CFGS[key]["n_snakes"]
    snakes = _short(ns)
    snakes[1] = [(-1, 5)]                          # moves inwards next, and takes its only cell along (grow_to = 1)
    out = {11: _st(snakes, _fruits(key), grow=[3, 1, 3, 3][:ns])}
    if key.startswith("N"):
        alive, in_dead = [True] * ns, [False] * ns
        alive[1], in_dead[1] = False, True
        if ns > 2:
            in_dead[3] = True
        out[5] = _st(_short(ns), _fruits(key), alive=alive, in_dead=in_dead)
    return out


def setup_actions(t, n, ns, rng):
    act = rng.integers(0, 5, (n, ns)).astype(np.int32)
    a, b = PATH[LONG - 1 + t], PATH[LONG + t]
    act[1] = 0
    act[1, 0] = ACT_OF[(b[0] - a[0], b[1] - a[1])]      # the long body follows the path
    act[9] = 0                                           # ... and env 9's main snake keeps going, into the wall
    return act


def build_source(src, rng):
    """Phase 1, SETUP steps, phase 2 on a Pair (library and oracle alike)."""
    src.reset()
    for e, st in phase1_states(src.key).items():
        src.install(e, st)
    for t in range(SETUP):
        src.step(setup_actions(t, src.n, src.ns, rng), ("setup", t))
    for e, st in phase2_states(src.key).items():
        src.install(e, st)


def assert_conditions(key, ora, selected):
    """What the copy has to cope with, asserted on the ORACLE's state of the selected source envs."""
    dim = CFGS[key]["dim"]
    sts = {i: ora.get_state(i) for i in selected}
    long_body = sts[1]["snakes"][0]
    assert len(long_body) >= 70 and SETUP >= 8 and tuple(long_body[0]) == PATH[LONG - 1 + SETUP], long_body[:3]
    assert any(ora.finished(i) for i in selected)
    assert any(st["ctr"] >> 32 for st in sts.values())
    assert any(len(b) == 0 for st in sts.values() for b in st["snakes"])
    assert any(b and not (0 <= b[0][0] < dim and 0 <= b[0][1] < dim) for st in sts.values() for b in st["snakes"])
    if key == "A":
        assert any(len(st["fruits"]) > 64 for st in sts.values())
    if key.startswith("N"):
        assert any(not a for st in sts.values() for a in st["alive"]) and any(d for st in sts.values() for d in st["in_dead"])


# ------------------------------------------------------------------------------------------ 1. words and play
@pytest.mark.parametrize("key", ["S", "A", "N4", "N2"])
def test_words_and_play_on_all_rule_sets(key):
    rng = np.random.default_rng(len(key) * 100 + ord(key[0]))
    src = Pair(key, 96, seed=5, env_id_base=1000, auto_reset=False)
    dst = Pair(key, 64, seed=9, env_id_base=7, auto_reset=True)
    build_source(src, rng)
    dst.reset().play(5, rng, "dst before")
    forced = [(0, 1), (1, 1), (2, 2), (3, 5), (4, 7), (5, 9), (6, 11), (7, 8), (63, 1)]
    idx = fixed_index(rng, 64, 96, forced)
    assert_conditions(key, src.ora, sorted(set(idx[idx >= 0].tolist())))
    copy_both(dst, src, idx, key)
    dst.play(60, rng, "dst after")
    src.play(60, rng, "src after")
    dst.check_states("end"), src.check_states("end")
    dst.close(), src.close()


# ------------------------------------------------------------------------------------------ 2. rollback
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("key", ["S19", "A"])
def test_rollback_is_exact(key, auto_reset):
    n, T = 200, 40
    rng = np.random.default_rng(31)
    p = Pair(key, n, seed=12, env_id_base=300, auto_reset=auto_reset).reset().play(7, rng, "before")
    snap = p.env.clone()                                           # same seed, same env_id_base
    snap_words = blob_words(snap.get_state_all())
    assert_words(snap_words, p.words(), "clone")
    o_snap = [ora_words(p.ora, e) for e in range(n)]
    acts = rng.integers(-1, 6, (T, n, p.ns)).astype(np.int32)
    first = [p.step(acts[t], ("pass 1", t)) for t in range(T)]
    assert any(d.any() for _, _, d, _ in first)
    assert_words(blob_words(snap.get_state_all()), snap_words, "the snapshot does not move")
    p.env.copy_envs_device(snap)
    for e in range(n):
        assert p.ora.L.orc_import_state(p.ora.h, e, o_snap[e].ctypes.data, len(o_snap[e])) == 0
    assert_words(p.words(), snap_words, "restored")
    for t in range(T):
        second = p.step(acts[t], ("pass 2", t))                    # (against the oracle, inside)
        for a, b in zip(first[t], second):
            assert a.tobytes() == b.tobytes(), t
    snap.close(), p.close()


# ------------------------------------------------------------------------------------------ 3. handle differences
def _differ(key, src_kw, dst_kw, n_src=80, n_dst=72, steps=30, via="numpy"):
    rng = np.random.default_rng(77)
    src = Pair(key, n_src, **dict(dict(seed=3, env_id_base=50), **src_kw)).reset().play(12, rng, "src before")
    dst = Pair(key, n_dst, **dict(dict(seed=3, env_id_base=50), **dst_kw)).reset().play(3, rng, "dst before")
    copy_both(dst, src, fixed_index(rng, n_dst, n_src), (key, src_kw, dst_kw), via=via)
    dst.play(steps, rng, "dst after")
    src.play(steps // 3, rng, "src after")
    dst.close(), src.close()


@pytest.mark.parametrize("key", ["S", "A"])
@pytest.mark.parametrize("a,b", [("short", "full"), ("full", "short"), ("full", "full"), ("short", "short")])
def test_record_policies_differ(key, a, b):
    """full -> anything after the source has stepped: its parked draws are valid and must not be carried over (the
    destination draws from its own slot's stream, which the oracle does too)."""
    import torch
    _differ(key, dict(record_policy=a), dict(record_policy=b, seed=4, env_id_base=900), via=torch.int64)


@pytest.mark.parametrize("epb", [1, 4, 8])
def test_envs_per_block_differ(epb):
    import torch
    _differ("S", dict(envs_per_block=8 if epb == 1 else 1), dict(envs_per_block=epb), n_dst=37, via=torch.int32)


@pytest.mark.parametrize("key,src_kw,dst_kw", [
    ("S", dict(obs_scale=1), dict(obs_scale=4)),
    ("A", dict(seed=3, env_id_base=50), dict(seed=11, env_id_base=2**33 + 5)),
    ("S", dict(auto_reset=False), dict(auto_reset=True)), ("A", dict(auto_reset=True), dict(auto_reset=False)),
    ("S", dict(max_steps=2000), dict(max_steps=25)), ("N2", dict(max_steps=2000), dict(max_steps=25)),
    ("N4", dict(max_steps=30), dict(max_steps=2000)),
])
def test_other_configuration_differs(key, src_kw, dst_kw):
    _differ(key, src_kw, dst_kw, via="list")


def test_16384_envs_with_a_permutation():
    """The library picks the short record itself above 8 192 envs; a random permutation, every env compared through
    one get_state_all blob per handle, then 5 steps against the oracle."""
    n = 16384
    rng = np.random.default_rng(16384)
    src = Pair("S", n, threads=16, seed=2, env_id_base=10).reset().play(6, rng)
    dst = Pair("S", n, threads=16, seed=8, env_id_base=10**6).reset()
    perm = rng.permutation(n)
    copy_both(dst, src, perm, "perm")
    dst.play(5, rng, "after")
    dst.close(), src.close()


# ------------------------------------------------------------------------------------------ 4. untouched
def test_untouched_means_untouched():
    import torch
    rng = np.random.default_rng(4)
    src = Pair("S", 50, seed=1).reset().play(40, rng)
    dst = Pair("S", 40, seed=2).reset().play(40, rng)
    st_src, st_dst = src.env.stats(), dst.env.stats()
    assert st_dst["episodes"] > 10 and st_src["episodes"] > 10 and st_dst["errors"] == 0
    idx = fixed_index(rng, 40, 50)
    copy_both(dst, src, idx, "valid")
    assert dst.env.stats() == st_dst and src.env.stats() == st_src         # totals stay, env_steps too
    # nothing selected: not a byte moves
    before = dst.env.get_state_all().tobytes()
    dst.env.copy_envs_device(src.env, np.full(40, -1))
    dst.env.copy_envs_device(src.env, torch.full((40,), -5, dtype=torch.int64, device=dst.env.device))
    assert dst.env.get_state_all().tobytes() == before and dst.env.stats() == st_dst
    # entries >= src.num_envs: the env keeps its words, its error total grows by exactly one per entry and call
    bad = idx.copy()
    bad[[3, 17, 39]] = [50, 51, 2**31 - 1]
    copy_both(dst, src, bad, "out of range")                                # (out-of-range entries: expected = unchanged)
    assert dst.env.stats() == dict(st_dst, errors=3) and src.env.stats() == st_src
    dst.env.copy_envs_device(src.env, [50] * 40)
    assert dst.env.stats(reset=True) == dict(st_dst, errors=43)
    dst.play(20, rng, "after")                                              # the guard counts, it breaks nothing
    assert dst.env.stats()["errors"] == 0
    dst.env.close(), src.env.close()


# ------------------------------------------------------------------------------------------ 5. interplay
@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("key", ["S", "A", "N2"])
def test_after_tape_rollouts(key, persistent):
    import torch
    rng = np.random.default_rng(6)
    src, dst = Pair(key, 48, seed=5).reset(), Pair(key, 48, seed=5, env_id_base=48).reset()
    for chunk in range(2):
        tape = rng.integers(0, 5, (25, 48, src.ns)).astype(np.int32)
        src.env.rollout_device(torch.from_numpy(tape).to(src.env.device), persistent=persistent, keep_obs=False)
        for t in range(25):
            src.ora.step(tape[t], want_obs=False)
        src.check_states(("tape", chunk))
        copy_both(dst, src, None if chunk else fixed_index(rng, 48, 48), (key, persistent, chunk))
        dst.play(15, rng, "after")
    dst.close(), src.close()


def test_after_a_masked_reset_and_before_the_scripted_calls():
    import torch
    rng = np.random.default_rng(8)
    for key in ("S", "N4", "A"):
        src = Pair(key, 64, seed=6, auto_reset=False).reset().play(30, rng)
        mask = (rng.random(64) < 0.5)
        src.env.reset(mask=mask)
        src.ora.reset_envs(mask.astype(np.uint8), obs=None, final_obs=None, truncated=None)
        dst = Pair(key, 64, seed=7, auto_reset=False).reset()
        copy_both(dst, src, fixed_index(rng, 64, 64), key)
        # the scripted opponents and the safe-move mask read the copied state: NumPy statements on the oracle's
        read = sp._StateReader(dst.ora)
        states = [read(e) for e in range(64)]
        dim, ns = CFGS[key]["dim"], dst.ns
        safe = torch.zeros((64, ns), dtype=torch.uint8, device=dst.env.device)
        for pol in ("safe_greedy", "hamiltonian"):
            want = np.array([sp.POLICIES[pol](st, dim, ns, None, 0.0) for st in states], np.int32)
            got, _ = dst.env.scripted_actions_device(pol, safe_out=safe)
            assert np.array_equal(got.cpu().numpy(), want), (key, pol)
        want_m = np.array([sp.np_safe_mask(st, dim, ns) for st in states], np.uint8)
        assert np.array_equal(safe.cpu().numpy(), want_m) and np.array_equal(dst.env.safe_moves_device().cpu().numpy(), want_m)
        dst.play(20, rng, "after")
        dst.close(), src.close()


def test_into_and_out_of_a_terminal_obs_env():
    rng = np.random.default_rng(10)
    plain = Pair("S", 56, seed=3).reset().play(20, rng)
    term = Pair("S", 56, seed=4, terminal_obs=True).reset().play(5, rng)
    copy_both(term, plain, fixed_index(rng, 56, 56), "into")
    term.play(30, rng, "terminal_obs after")
    copy_both(plain, term, None, "out of")
    plain.play(15, rng, "plain after")
    term.close(), plain.close()


def test_clone_and_its_overrides():
    rng = np.random.default_rng(12)
    p = Pair("A", 48, seed=5, env_id_base=9, record_policy="full").reset().play(15, rng)
    w = p.words()
    same = p.env.clone()
    assert same.num_envs == 48 and same.rules == "adversarial" and (same.cfg.seed, same.cfg.env_id_base) == (5, 9)
    assert_words(blob_words(same.get_state_all()), w, "clone")
    other = p.env.clone(record_policy="short", seed=6, env_id_base=100, auto_reset=False, max_steps=500, obs_scale=4,
                        envs_per_block=2)
    assert (other.cfg.seed, other.cfg.env_id_base, other.cfg.auto_reset, other.cfg.max_steps) == (6, 100, 0, 500)
    assert other.obs_shape == (48, 48, 9)
    assert_words(blob_words(other.get_state_all()), w, "clone with overrides")
    wide = p.env.clone(num_envs=100)                                # another size: no copy, the caller says which envs
    assert wide.num_envs == 100
    wide.reset()
    wide.copy_envs_device(p.env, np.arange(100) % 48)
    assert_words(blob_words(wide.get_state_all()), [w[e % 48] for e in range(100)], "fork")
    for bad in (dict(dim=12), dict(rules="snake_env"), dict(n_snakes=2), dict(n_fruits=2), dict(device="cuda:0")):
        with pytest.raises(ValueError, match="clone"):
            p.env.clone(**bad)
    same.close(), other.close(), wide.close(), p.close()


# ------------------------------------------------------------------------------------------ 6. HIP graph
def test_graph_of_copy_then_step():
    """[msnake_copy_envs -> msnake_step] captured as one linear chain (no parallel branches) and replayed three times
    with the source stepped in between; every replay against the oracle."""
    import torch
    rng = np.random.default_rng(14)
    n = 64
    src = Pair("S19", n, seed=5).reset().play(4, rng)
    dst = Pair("S19", n, seed=5, env_id_base=n).reset()
    idx = fixed_index(rng, n, n)
    idx_dev = torch.from_numpy(idx.astype(np.int32)).to(dst.env.device)
    acts = torch.zeros((n, 3), dtype=torch.int32, device=dst.env.device)
    blob = dst.env.get_state_all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        dst.env.copy_envs_device(src.env, idx_dev)
        dst.env.step_device(acts)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    dst.env.set_state_all(blob)    # the warm-up moved the envs: back to the state after reset()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dst.env.copy_envs_device(src.env, idx_dev)
        out = dst.env.step_device(acts)
    torch.cuda.synchronize()
    dst.env.set_state_all(blob)    # (capture itself runs nothing; this keeps the start state explicit)
    for k in range(3):
        a = rng.integers(0, 5, (n, 3)).astype(np.int32)
        acts.copy_(torch.from_numpy(a).to(acts.device))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        ora_copy(dst.ora, src.ora, idx)
        o_obs, o_rew, o_done, o_ns, _, o_el = dst.ora.step(a)
        info = out[3].cpu().numpy()
        assert np.array_equal(out[0].cpu().numpy(), o_obs) and np.array_equal(out[1].cpu().numpy(), o_rew), k
        assert np.array_equal(out[2].cpu().numpy(), o_done) and np.array_equal(info[:, 2], o_ns), k
        assert np.array_equal(info[:, 1], o_el), k
        dst.check_states(("replay", k))
        src.play(3, rng, ("src between", k))
    dst.close(), src.close()


# ------------------------------------------------------------------------------------------ 7. errors
def test_argument_errors_name_the_argument():
    """Every MSNAKE_E_ARG / MSNAKE_E_HANDLE case of include/msnake.h.  (Two handles on different devices need two
    GPUs: that case runs where torch sees a second one.)"""
    import msnake
    import torch
    mk = msnake.MultiSnakeVecEnv
    dst = mk(6, dim=10, n_snakes=3, rules="snake_env", seed=1)
    dst.reset()
    dst.step(np.ones((6, 3), np.int32))
    others = {"dim": mk(6, dim=12, n_snakes=3, rules="snake_env"), "n_snakes": mk(6, dim=10, n_snakes=2, rules="snake_env"),
              "rules": mk(6, dim=10, n_snakes=3, rules="adversarial"), "num_envs": mk(5, dim=10, n_snakes=3, rules="snake_env")}
    nw = {"dst": mk(6, dim=10, n_snakes=3, n_fruits=4, rules="new_world"), "src": mk(6, dim=10, n_snakes=3, n_fruits=5, rules="new_world")}
    for e in list(others.values()) + list(nw.values()):
        e.reset()
    L = dst._L
    before = dst.get_state_all().tobytes()
    idx = torch.zeros(6, dtype=torch.int32, device=dst.device)
    none = torch.full((6,), -1, dtype=torch.int32, device=dst.device)

    def call(d, s, i):
        rc = L.msnake_copy_envs(d, s, i, None)
        return rc, L.msnake_last_error().decode()

    rc, msg = call(dst._h, dst._h, idx.data_ptr())
    assert rc == -1 and "src" in msg and "dst" in msg, msg
    rc, msg = call(dst._h, dst._h, None)
    assert rc == -1 and "src" in msg, msg
    for word in ("dim", "n_snakes", "rules"):
        for i in (idx.data_ptr(), None):
            rc, msg = call(dst._h, others[word]._h, i)
            assert rc == -1 and word in msg, (word, msg)
    rc, msg = call(nw["dst"]._h, nw["src"]._h, idx.data_ptr())
    assert rc == -1 and "n_fruits" in msg, msg
    rc, msg = call(dst._h, others["num_envs"]._h, None)
    assert rc == -1 and "src_index_dev" in msg and "num_envs" in msg, msg
    assert call(dst._h, others["num_envs"]._h, none.data_ptr())[0] == 0     # with an index the env counts may differ
    assert call(others["num_envs"]._h, dst._h, idx.data_ptr())[0] == 0
    dead = ctypes.create_string_buffer(4)                                    # a handle whose magic word is gone
    for d, s in ((None, dst._h), (dst._h, None), (dead, dst._h), (dst._h, dead)):
        rc, msg = call(d, s, None)
        assert rc == -3 and "handle" in msg, msg
    if torch.cuda.device_count() > 1:
        far = mk(6, dim=10, n_snakes=3, rules="snake_env", device="cuda:1")
        rc, msg = call(dst._h, far._h, None)
        assert rc == -1 and "device" in msg, msg
        far.close()
    torch.cuda.synchronize()
    assert dst.get_state_all().tobytes() == before and dst.stats()["errors"] == 0   # refused before any device work
    # the wrapper: exceptions, and the pending step of step_async / step_wait is protected
    with pytest.raises(RuntimeError, match="dim"):
        dst.copy_envs_device(others["dim"])
    with pytest.raises(TypeError):
        dst.copy_envs_device(dst._h)
    for bad in (torch.zeros(6, dtype=torch.float32, device=dst.device), torch.zeros((6, 1), dtype=torch.int32, device=dst.device),
                torch.zeros(5, dtype=torch.int64, device=dst.device), np.zeros(6, np.float64), [0, 1, 2]):
        with pytest.raises(ValueError):
            dst.copy_envs_device(others["num_envs"], bad)
    twin = dst.clone()
    dst.step_async(np.ones((6, 3), np.int32))
    with pytest.raises(RuntimeError, match="step_wait"):
        dst.copy_envs_device(twin)
    with pytest.raises(RuntimeError, match="step_wait"):
        twin.copy_envs_device(dst)
    dst.step_wait()
    twin.copy_envs_device(dst)                                               # fine again
    dst.copy_envs_device(twin)
    st = dst.stats()
    assert st["errors"] == 0 and st["env_steps"] == 12                       # a copy adds nothing to env_steps
    assert dst.get_state_all().tobytes() == twin.get_state_all().tobytes()
    for e in list(others.values()) + list(nw.values()) + [twin, dst]:
        e.close()


def test_refused_calls_leave_the_destination_alone():
    import msnake
    mk = msnake.MultiSnakeVecEnv
    rng = np.random.default_rng(2)
    dst = mk(9, dim=10, n_snakes=3, rules="adversarial", seed=1)
    dst.reset()
    for _ in range(10):
        dst.step(rng.integers(0, 5, (9, 3)).astype(np.int32))
    before, st = dst.get_state_all().tobytes(), dst.stats()
    others = [mk(9, dim=11, n_snakes=3, rules="adversarial"), mk(9, dim=10, n_snakes=2, rules="adversarial"),
              mk(9, dim=10, n_snakes=3, rules="snake_env"), mk(8, dim=10, n_snakes=3, rules="adversarial")]
    for other in others:
        other.reset()
    for other in others + [dst]:
        with pytest.raises(RuntimeError, match="msnake_copy_envs"):
            dst.copy_envs_device(other)
    for other in others:
        other.close()
    assert dst.get_state_all().tobytes() == before and dst.stats() == st
    dst.close()
