"""Device-side state export, import and hashes (msnake_export_states, msnake_import_states, msnake_hash_states;
MultiSnakeVecEnv.export_states_device / import_states_device / hash_states_device).

Expected values never come from the calls under test: words are those of the blocking get_state_all / get_state_words,
hashes are msnake.state_hash of those words on the host, verdicts on rows come from state_domain.accepts (plain Python
from the header's text), and play after an import is compared with the CPU oracle.  Every output lies between guards.
"""
import numpy as np
import pytest

import board_states as bs
import state_domain as sd
from gpu_harness import GuardedOutputs
from state_domain import assert_words, blob_words

pytestmark = pytest.mark.gpu

SENT32, SENT64, SENT8 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5, 0xA5
M64 = (1 << 64) - 1


def i64(x):
    return x - (1 << 64) if x >> 63 else x


def words_max(cfg):
    F = sd.fcap(cfg) if cfg["rules"] == "adversarial" else cfg["n_fruits"]
    return 8 + 2 * F + cfg["n_snakes"] * (6 + 2 * (sd.cap(cfg) - 2))


def make(cfg, n, **kw):
    import msnake
    return msnake.MultiSnakeVecEnv(n, **cfg, **kw)


def compiled(env):
    return env.kernel_name().count(",") == 4


def ref_words(env):
    """Every env's canonical words from the blocking path."""
    return blob_words(env.get_state_all())


def play(envs, steps, seed, lo=0):
    """The same seeded random actions for every env of `envs`."""
    rng = np.random.default_rng(seed)
    out = None
    for _ in range(steps):
        act = rng.integers(lo, 5, (envs[0].num_envs, envs[0].n_snakes)).astype(np.int32)
        out = [e.step(act) for e in envs]
    return out


def buffers(env, stride, what=("words", "count", "full", "board", "status")):
    n = env.num_envs
    spec = {"words": dict(dtype="int32", shape=(n, stride), fill=SENT32), "count": dict(dtype="int32", shape=(n,), fill=SENT32),
            "full": dict(dtype="int64", shape=(n,), fill=SENT64, align=8), "board": dict(dtype="int64", shape=(n,), fill=SENT64, align=8),
            "status": dict(dtype="uint8", shape=(n,), fill=SENT8)}
    return GuardedOutputs(env.device, {k: spec[k] for k in what})


def check_rows(rows, counts, ref, stride, what=None):
    """Row e holds ref[e] and the sentinel behind it -- or, if ref[e] does not fit `stride`, the sentinel alone."""
    sent = np.array([SENT32], np.uint32).view(np.int32)[0]
    assert counts.tolist() == [len(w) for w in ref], what
    for e, w in enumerate(ref):
        n = len(w) if len(w) <= stride else 0
        assert np.array_equal(rows[e, :n], w[:n]) and (rows[e, n:] == sent).all(), (what, e, len(w), stride)


# ------------------------------------------------------------------------------------------ the export configurations
CFG = {"S5": dict(rules="snake_env", dim=5, n_snakes=3, n_fruits=3, max_steps=2000),
       "S19": dict(rules="snake_env", dim=19, n_snakes=3, n_fruits=3, max_steps=2000),
       "N6": dict(rules="new_world", dim=6, n_snakes=4, n_fruits=5, max_steps=2000),
       "A10": dict(rules="adversarial", dim=10, n_snakes=3, n_fruits=3, max_steps=2000),
       "LONG": dict(rules="snake_env", dim=12, n_snakes=3, n_fruits=3, max_steps=2000),
       "S62": dict(rules="snake_env", dim=62, n_snakes=3, n_fruits=3, max_steps=2000)}
_PLAYED = {}


def adv_long_list():
    """A10: a list of 70 entries, some on the wall ring; snakes 1 and 2, twelve pieces each, run into the wall at
    c0 = dim on the next step and their pieces join the list, while the main snake rests."""
    edge = [[-1, -1], [10, 10], [-1, 10], [10, 0], [2, -1]]
    fruits = [list(edge[i % 5]) if i % 4 == 0 else [i % 10, 1 + 2 * (i // 10 % 2)] for i in range(70)]
    body = lambda y: [[9 - i, y] for i in range(10)] + [[0, y + 1], [1, y + 1]]
    snakes = [([[2, 0], [1, 0]], (0, 0), 3), (body(4), (1, 0), 12), (body(7), (1, 0), 12)]
    return sd.state_words(3, fruits, snakes, t=7, spare=5)


def played(key):
    """(env, its reference words): 40 steps of seeded random play, or the hand-built states of the key.  Built once; the
    tests only read these envs."""
    if key not in _PLAYED:
        from oracle.snake_oracle import state_to_flat
        cfg = CFG[key]
        if key == "LONG":
            states, walled = bs.overflow_states(12, 3)
            assert walled == 2 and len(states) <= 16
            env = make(cfg, 16, seed=5)
            env.reset()
            for e in range(16):
                env.set_state_words(e, state_to_flat(states[e % len(states)], 3))
            assert max(int(w[8 + 6]) for w in ref_words(env)) > 64          # snake 0's len
        else:
            env = make(cfg, 16 if key == "S62" else 64, seed=7, env_id_base=1000)
            env.reset()
            play([env], 40, 21)
            if key == "A10":
                for e in (0, 5, 63):
                    env.set_state_words(e, adv_long_list())
                env.step(np.zeros((64, 3), np.int32))
                ref = ref_words(env)
                assert min(int(ref[e][6]) for e in (0, 5, 63)) > 70     # the dead bodies joined the list
        _PLAYED[key] = (env, ref_words(env))
    return _PLAYED[key]


@pytest.mark.parametrize("key", list(CFG))
def test_export_equals_get_state(key):
    import torch
    env, ref = played(key)
    stride = env.state_words_max
    assert stride == words_max(CFG[key]) >= max(len(w) for w in ref)
    before = env.stats()
    for e in (0, env.num_envs // 2, env.num_envs - 1):
        assert np.array_equal(env.get_state_words(e), ref[e])
    buf = buffers(env, stride, ("words", "count"))
    words, count = env.export_states_device(out=buf.words, count_out=buf.count)
    assert words is buf.words and count is buf.count
    torch.cuda.synchronize()
    check_rows(buf.host("words"), buf.host("count"), ref, stride, key)
    assert buf.guards_intact()
    # words only, counts only
    buf.refill()
    assert env.export_states_device(out=buf.words, count=False)[1] is None
    torch.cuda.synchronize()
    assert buf.untouched("count")
    check_rows(buf.host("words"), np.array([len(w) for w in ref]), ref, stride, key)
    buf.refill()
    assert env.export_states_device(words=False, count_out=buf.count)[0] is None
    torch.cuda.synchronize()
    assert buf.untouched("words") and buf.host("count").tolist() == [len(w) for w in ref] and buf.guards_intact()
    # the default: tensors of the env's choosing, state_words_max wide
    words, count = env.export_states_device()
    assert tuple(words.shape) == (env.num_envs, stride) and words.dtype == torch.int32 and count.dtype == torch.int32
    rows, cnt = words.cpu().numpy(), count.cpu().numpy()
    assert all(np.array_equal(rows[e, :cnt[e]], ref[e]) for e in range(env.num_envs))
    assert_words(ref_words(env), ref, "export only reads")
    assert env.stats() == before and before["errors"] == 0      # nothing is added to env_steps


@pytest.mark.parametrize("key", ["S5", "A10", "LONG"])
def test_export_with_a_stride_one_word_short(key):
    import torch
    env, ref = played(key)
    stride = max(len(w) for w in ref) - 1
    assert any(len(w) <= stride for w in ref)
    buf = buffers(env, stride, ("words", "count"))
    env.export_states_device(out=buf.words, count_out=buf.count)
    torch.cuda.synchronize()
    check_rows(buf.host("words"), buf.host("count"), ref, stride, key)   # (the longest rows keep the sentinel; counts stay right)
    assert buf.guards_intact()


# ------------------------------------------------------------------------------------------ hash
@pytest.mark.parametrize("key", list(CFG))
def test_hashes_equal_the_host_hash_of_the_words(key):
    import msnake
    import torch
    env, ref = played(key)
    buf = buffers(env, 1, ("full", "board"))
    assert env.hash_states_device("full", out=buf.full) is buf.full
    env.hash_states_device("board", out=buf.board)
    torch.cuda.synchronize()
    assert buf.host("full").tolist() == [i64(msnake.state_hash(w)) for w in ref]
    assert buf.host("board").tolist() == [i64(msnake.state_hash(w, "board")) for w in ref]
    assert buf.guards_intact()
    assert env.hash_states_device().cpu().tolist() == buf.host("full").tolist()     # a tensor of the env's choosing, "full"
    assert_words(ref_words(env), ref, "hash only reads")


def test_hashes_follow_a_permuted_copy():
    import torch
    src, ref = played("S19")
    dst = src.clone()
    perm = np.random.default_rng(4).permutation(src.num_envs)
    dst.copy_envs_device(src, perm)
    for what in ("full", "board"):
        h_src, h_dst = src.hash_states_device(what).cpu().numpy(), dst.hash_states_device(what).cpu().numpy()
        assert np.array_equal(h_dst, h_src[perm]) and len(set(h_src.tolist())) == src.num_envs
    dst.close()


def test_same_position_at_another_time():
    import msnake
    import torch
    env, ref = played("S5")
    twin = make(CFG["S5"], env.num_envs, seed=7, env_id_base=1000)
    twin.reset()
    later = [w.copy() for w in ref]
    for e, w in enumerate(later):
        w[0] += 1 + e
        w[1] += 4
        w[4] += 1
    rows, counts = pad(later, twin.state_words_max)
    status = twin.import_states_device(torch.from_numpy(rows).to(twin.device), count=torch.from_numpy(counts).to(twin.device))
    assert status.cpu().tolist() == [0] * env.num_envs
    assert torch.equal(env.hash_states_device("board"), twin.hash_states_device("board"))
    assert not (env.hash_states_device("full") == twin.hash_states_device("full")).any()
    assert twin.hash_states_device("full").cpu().tolist() == [i64(msnake.state_hash(w)) for w in later]
    twin.close()


def test_misaligned_hash_output_raises():
    import torch
    from msnake import _capi
    env, ref = played("S5")
    buf = buffers(env, 1, ("full",))
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        _capi.check(env._L.msnake_hash_states(env._h, 0, buf.full.data_ptr() + 4, None), "msnake_hash_states")
    with pytest.raises(RuntimeError, match="neither"):
        _capi.check(env._L.msnake_hash_states(env._h, 2, buf.full.data_ptr(), None), "msnake_hash_states")
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        _capi.check(env._L.msnake_export_states(env._h, buf.full.data_ptr() + 2, 8, None, None), "msnake_export_states")
    for args in ((None, 8, None), (buf.full.data_ptr(), 0, None), (buf.full.data_ptr(), -1, None)):
        assert env._L.msnake_export_states(env._h, *args, None) == -1     # MSNAKE_E_ARG
    assert env._L.msnake_import_states(env._h, None, buf.full.data_ptr(), 7, None, buf.full.data_ptr(), None) == -1
    assert env._L.msnake_import_states(env._h, None, None, 8, None, buf.full.data_ptr(), None) == -1
    assert env._L.msnake_import_states(env._h, None, buf.full.data_ptr(), 8, None, None, None) == -1
    torch.cuda.synchronize()
    assert buf.untouched("full")


# ------------------------------------------------------------------------------------------ import
def pad(words, stride, fill=-7):
    """(rows int32 [n, stride] with `fill` behind each env's words, counts int32 [n])."""
    rows = np.full((len(words), stride), fill, np.int32)
    for e, w in enumerate(words):
        rows[e, :len(w)] = w
    return rows, np.array([len(w) for w in words], np.int32)


IMPORT_CASES = {"generic": (CFG["S19"], dict(), True),
                "S19": (CFG["S19"], dict(), False),
                "S10x1": (dict(rules="snake_env", dim=10, n_snakes=1, n_fruits=1, max_steps=2000), dict(), False),
                "short4": (CFG["S19"], dict(record_policy="short", envs_per_block=4), False),
                "N6": (CFG["N6"], dict(), False),
                "A10": (CFG["A10"], dict(), False)}


@pytest.mark.parametrize("case", list(IMPORT_CASES))
def test_export_import_round_trip_then_lockstep_with_the_oracle(case, monkeypatch):
    import torch
    from oracle.snake_oracle import Oracle, flat_to_state
    cfg, kw, generic = IMPORT_CASES[case]
    if generic:
        monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "1")
    n = 48
    a, b = make(cfg, n, seed=3, env_id_base=500, **kw), make(cfg, n, seed=3, env_id_base=500, **kw)
    assert compiled(a) == (case in ("S19", "S10x1")) and compiled(b) == compiled(a), a.kernel_name()
    a.reset(), b.reset()
    play([a], 40, 8)
    play([b], 3, 9)                                            # B is somewhere else
    ref = ref_words(a)
    buf = buffers(a, a.state_words_max, ("words", "count", "status"))
    a.export_states_device(out=buf.words, count_out=buf.count)
    status = b.import_states_device(buf.words, count=buf.count, status_out=buf.status)
    assert status is buf.status
    torch.cuda.synchronize()
    assert buf.host("status").tolist() == [0] * n and buf.guards_intact()
    assert a.get_state_all().tobytes() == b.get_state_all().tobytes()
    assert compiled(b) == compiled(a)                          # (an import never moves a handle to other kernels)
    ora = Oracle(n, dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"], rules=cfg["rules"], seed=3, env_id_base=500)
    ora.reset()
    for e, w in enumerate(ref):
        ora.set_state(e, flat_to_state(w))
    rng = np.random.default_rng(10)
    for t in range(30):
        act = rng.integers(0, 5, (n, cfg["n_snakes"])).astype(np.int32)
        o_obs, o_rew, o_done, o_ns, _, _ = ora.step(act)
        for env in (a, b):
            obs, rew, done, infos = env.step(act)
            assert np.array_equal(rew, o_rew) and np.array_equal(done, o_done.astype(bool)), (case, t)
            assert [i["num_snakes"] for i in infos] == list(o_ns), (case, t)
    assert np.array_equal(a.render(), o_obs) and np.array_equal(obs, o_obs)
    assert a.get_state_all().tobytes() == b.get_state_all().tobytes()
    assert a.stats()["errors"] == 0 and b.stats()["errors"] == 0
    a.close(), b.close()


def test_import_mask_and_counts():
    import torch
    from msnake import _capi
    src, ref = played("S19")
    n = src.num_envs
    dst = make(CFG["S19"], n, seed=7, env_id_base=1000)
    dst.reset()
    play([dst], 5, 77)
    own = ref_words(dst)
    rows, counts = pad(ref, src.state_words_max)
    mask = np.arange(n) % 3 != 1
    buf = buffers(dst, 1, ("status",))
    t_rows, t_counts = torch.from_numpy(rows).to(dst.device), torch.from_numpy(counts).to(dst.device)
    dst.import_states_device(t_rows, mask=mask, count=t_counts, status_out=buf.status)
    torch.cuda.synchronize()
    assert buf.host("status").tolist() == [_capi.STATE_OK if m else _capi.STATE_SKIPPED for m in mask] and buf.guards_intact()
    assert_words(ref_words(dst), [ref[e] if mask[e] else own[e] for e in range(n)], "masked import")
    # a device mask; a count below 0 and one above the stride are "too short", the others are installed; without counts
    # every row has `stride` words and those behind the last snake are ignored
    bad = counts.copy()
    bad[3], bad[4], bad[6] = -1, rows.shape[1] + 1, counts[6] - 1
    status = dst.import_states_device(t_rows, mask=torch.ones(n, dtype=torch.bool, device=dst.device),
                                      count=torch.from_numpy(bad).to(dst.device))
    want = [_capi.STATE_TOO_SHORT if e in (3, 4, 6) else _capi.STATE_OK for e in range(n)]
    assert status.cpu().tolist() == want
    assert_words(ref_words(dst), [own[e] if e == 4 else ref[e] for e in range(n)], "bad counts")   # (3 and 6 held ref already)
    dst.import_states_device(torch.from_numpy(pad(own, src.state_words_max)[0]).to(dst.device), mask=[4])
    assert dst.import_states_device(t_rows).cpu().tolist() == [0] * n
    assert_words(ref_words(dst), ref, "import without counts")
    assert_words(ref_words(src), ref, "the source")
    assert dst.stats()["errors"] == 0
    dst.close()


def offgrid_head(cfg, w):
    st = sd.St(w)
    return any(sn["cells"] and not (0 <= min(sn["cells"][0]) and max(sn["cells"][0]) < cfg["dim"]) for sn in st.snakes)


@pytest.mark.parametrize("key", sd.TABLE_KEYS)
def test_refusals_next_to_accepted_rows(key):
    """One row of the case table per env, refused and accepted rows side by side in ONE call: each refusal gives the
    status code of its reason and leaves the env untouched, each accepted row comes back word for word."""
    import torch
    from msnake import _capi
    cfg, table = sd.CFGS[key], sd.rows(key)
    rows = [build() for _, build, _ in table]
    n = len(rows)
    assert 16 <= n <= 256 and sum(r is not None for _, _, r in table) > 20
    env = make(cfg, n, seed=2)
    env.reset()
    play([env], 2, 5, lo=1)
    own = ref_words(env)
    stride = max(env.state_words_max, max(len(r) for r in rows))
    padded, counts = pad(rows, stride)
    want = []
    for (name, _, reason), w in zip(table, rows):
        assert sd.accepts(cfg, w) == reason, name
        want.append(_capi.STATE_CELL if reason is None and compiled(env) and offgrid_head(cfg, w) else reason or _capi.STATE_OK)
    buf = buffers(env, 1, ("status",))
    env.import_states_device(torch.from_numpy(padded).to(env.device), count=torch.from_numpy(counts).to(env.device), status_out=buf.status)
    torch.cuda.synchronize()
    got = buf.host("status").tolist()
    assert got == want, [(table[e][0], got[e], want[e]) for e in range(n) if got[e] != want[e]][:6]
    assert buf.guards_intact()
    after = ref_words(env)
    for e, w in enumerate(rows):
        expect = w[:sd.canonical_len(cfg, w)] if want[e] == _capi.STATE_OK else own[e]
        assert np.array_equal(after[e], expect), (table[e][0], want[e])
    assert env.stats()["errors"] == 0
    env.close()


def test_head_outside_the_grid_by_kernel_kind(monkeypatch):
    import torch
    from msnake import _capi
    cfg = CFG["S19"]
    spec = make(cfg, 16, seed=1)
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "1")
    gen = make(cfg, 16, seed=1)
    assert compiled(spec) and not compiled(gen)
    spec.reset(), gen.reset()
    own = ref_words(spec)
    rows = [w.copy() for w in own]
    k = 8 + 2 * 3 + 6
    rows[2][k], rows[9][k + 1] = -1, 19                 # snake 0's head at c0 = -1 / c1 = dim
    padded, counts = pad(rows, spec.state_words_max)
    t_rows, t_counts = torch.from_numpy(padded).to(spec.device), torch.from_numpy(counts).to(spec.device)
    want = [_capi.STATE_CELL if e in (2, 9) else _capi.STATE_OK for e in range(16)]
    assert spec.import_states_device(t_rows, count=t_counts).cpu().tolist() == want
    assert_words(ref_words(spec), own, "refused heads leave the envs as they were")
    assert compiled(spec)
    assert gen.import_states_device(t_rows, count=t_counts).cpu().tolist() == [0] * 16
    assert_words(ref_words(gen), rows, "the generic kernels take the head as msnake_set_state does")
    spec.close(), gen.close()


def test_agent_outcomes_behind_the_step_after_an_import():
    import torch
    src, ref = played("S19")
    n = 32
    x, y = make(CFG["S19"], n, seed=7, env_id_base=1000, auto_reset=False), make(CFG["S19"], n, seed=7, env_id_base=1000, auto_reset=False)
    x.reset(), y.reset()
    acts = torch.from_numpy(np.random.default_rng(1).integers(0, 5, (3, n, 3)).astype(np.int32)).to(x.device)
    for env in (x, y):                                   # both trackers are armed and one step old
        env.agent_outcomes_device(env.step_device(acts[0])[2])
    padded, counts = pad(ref[:n], x.state_words_max)
    assert x.import_states_device(torch.from_numpy(padded).to(x.device), count=torch.from_numpy(counts).to(x.device)).cpu().tolist() == [0] * n
    for e in range(n):
        y.set_state_words(e, ref[e])
    for k in (1, 2):
        outs = [env.agent_outcomes_device(env.step_device(acts[k])[2]) for env in (x, y)]
        for got, want in zip(*outs):
            assert torch.equal(got, want), k
    assert x.get_state_all().tobytes() == y.get_state_all().tobytes()
    assert x.stats()["errors"] == 0
    x.close(), y.close()


# ------------------------------------------------------------------------------------------ HIP graph
def test_graph_of_step_export_hash():
    """[msnake_step -> msnake_export_states -> msnake_hash_states] captured as a linear chain on a side stream and
    replayed three times with fresh actions in the captured buffer; after every replay the outputs equal those of an
    eager twin stepped with the same actions."""
    import msnake
    import torch
    n, ns, cfg = 64, 3, CFG["S19"]
    env, twin = make(cfg, n, seed=3), make(cfg, n, seed=3)
    env.reset(), twin.reset()
    blob = env.get_state_all()
    stride = env.state_words_max
    buf = buffers(env, stride, ("words", "count", "full"))
    acts = torch.ones((n, ns), dtype=torch.int32, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as graph capture wants
        env.step_device(acts)
        env.export_states_device(out=buf.words, count_out=buf.count)
        env.hash_states_device("full", out=buf.full)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = env.step_device(acts)
        env.export_states_device(out=buf.words, count_out=buf.count)
        env.hash_states_device("full", out=buf.full)
    torch.cuda.synchronize()
    env.set_state_all(blob)        # warm-up and capture aside: back to the state after reset()
    rng = np.random.default_rng(7)
    for k in range(3):
        act = torch.from_numpy(rng.integers(1, 5, (n, ns)).astype(np.int32)).to(env.device)
        acts.copy_(act)
        buf.refill()
        g.replay()
        e_out = twin.step_device(act)
        torch.cuda.synchronize()
        assert torch.equal(out[1], e_out[1]) and torch.equal(out[2], e_out[2]), k
        ref = ref_words(twin)
        check_rows(buf.host("words"), buf.host("count"), ref, stride, k)
        assert buf.host("full").tolist() == [i64(msnake.state_hash(w)) for w in ref] == twin.hash_states_device().cpu().tolist(), k
        assert buf.guards_intact()
    assert env.get_state_all().tobytes() == twin.get_state_all().tobytes()
    assert env.stats()["errors"] == 0
    env.close(), twin.close()
