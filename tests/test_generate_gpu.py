"""msnake_generate_states on the device (MultiSnakeVecEnv.generate_states_device / scatter_device).

Expected rows never come from the call under test: they are tests/generate_play.np_generate, the header's text in NumPy on
the oracle's Philox; the env's draw counter and word 3 that go into them are read through the blocking get_state_all, and
play from a generated position is compared with the CPU oracle started from the same states.  Every output lies between
guards."""
import ctypes
import functools

import numpy as np
import pytest

import generate_play as gp
import scripted_play as sp
from gpu_harness import GuardedOutputs, action_buffers, make_env, oracle_states
from state_domain import blob_words

pytestmark = pytest.mark.gpu

SENT32 = 0xA5A5A5A5
SENT = np.array([SENT32], np.uint32).view(np.int32)[0]
STATE_OK, STATE_SKIPPED = 0, 0xFF
E_ARG, E_HANDLE, E_ALIGN = -1, -3, -4


def buffers(env, stride, len_cols=None):
    n, ns = env.num_envs, env.n_snakes
    return GuardedOutputs(env.device, {"words": dict(dtype="int32", shape=(n, stride), fill=SENT32),
                                       "count": dict(dtype="int32", shape=(n,), fill=SENT32),
                                       "got": dict(dtype="int32", shape=(n, ns), fill=SENT32),
                                       "status": dict(dtype="uint8", shape=(n,), fill=0xA5)})


def counters(env):
    """Every env's draw counter and word 3, from the blocking path."""
    ref = blob_words(env.get_state_all())
    ctr = [(int(w[1]) & 0xFFFFFFFF) | ((int(w[2]) & 0xFFFFFFFF) << 32) for w in ref]
    return np.array(ctr, np.uint64), np.array([int(w[3]) for w in ref], np.int64)


def lengths_tensor(env, cfg, req, cols=None):
    import torch
    a = gp.lengths_array(cfg, req).astype(np.int32)
    if cols:
        a = np.concatenate([a, np.full((a.shape[0], cols - a.shape[1]), 77, np.int32)], axis=1)   # surplus columns: ignored
    return torch.from_numpy(np.ascontiguousarray(a)).to(env.device)


def check_rows(buf, want, stride, what=None):
    """Selected rows hold the expected words and the sentinel behind them (or the sentinel alone if they do not fit),
    their count and their got; unselected rows, counts and gots hold the sentinel."""
    rows, count, got = want
    words, cnt, g = buf.host("words"), buf.host("count"), buf.host("got")
    for e, row in enumerate(rows):
        if row is None:
            assert (words[e] == SENT).all() and cnt[e] == SENT and (g[e] == SENT).all(), (what, e, "unselected")
            continue
        n = len(row) if len(row) <= stride else 0
        assert cnt[e] == len(row) == count[e], (what, e, cnt[e], len(row))
        assert np.array_equal(g[e], got[e]), (what, e, g[e], got[e])
        assert np.array_equal(words[e, :n], row[:n]), (what, e, np.flatnonzero(words[e, :n] != row[:n])[:4])
        assert (words[e, n:] == SENT).all(), (what, e, "behind the row")
    assert buf.guards_intact(), what


# ------------------------------------------------------------------------------------------ equality with the restatement
CASES = gp.cases()


@pytest.mark.parametrize("key", list(CASES))
def test_rows_equal_the_restatement(key):
    import torch
    cfg, req = CASES[key]
    env = make_env(cfg)
    env.reset()
    if key == "S19":
        assert env.kernel_name().count(",") == 4          # a handle on a step kernel compiled for its shape
    ctr, word3 = counters(env)
    stride = env.state_words_max
    buf = buffers(env, stride)
    lengths = lengths_tensor(env, cfg, req, cols=cfg["n_snakes"] + 2 if key == "S6" else None)
    for compact in (True, False):
        buf.refill()
        out = env.generate_states_device(lengths, salt=17, compact=compact, out=buf.words, count_out=buf.count, got_out=buf.got)
        assert out[0] is buf.words and out[1] is buf.count and out[2] is buf.got
        torch.cuda.synchronize()
        want = gp.np_generate(cfg, req, salt=17, compact=compact, ctr=ctr, word3=word3)
        check_rows(buf, want, stride, (key, compact))
        if key == "S19" and compact:
            assert want[2].max() > 64                     # bodies pass 64 pieces
        if key == "S62" and compact:
            assert want[2].max() > 3000, want[2].tolist()
    env.close()


def test_rows_on_an_adversarial_handle_in_the_middle_of_play():
    import torch
    cfg = gp.make_cfg("adversarial", 10, 3, 24, seed=12, env_id_base=7)
    env = make_env(cfg)
    env.reset()
    for _ in range(200):
        env.step_device(env.scripted_actions_device("safe_greedy"))
    ctr, word3 = counters(env)
    assert (ctr > 0).all() and (word3 > 0).any()          # the counter and spare_fruits have moved
    before, stats = env.get_state_all().tobytes(), env.stats()
    stride = env.state_words_max
    buf = buffers(env, stride)
    req = gp.mixed_requests(24, np.random.default_rng(3))
    lengths = lengths_tensor(env, cfg, req)
    for compact in (True, False):
        buf.refill()
        env.generate_states_device(lengths, salt=2 ** 63 + 5, compact=compact, out=buf.words, count_out=buf.count, got_out=buf.got)
        torch.cuda.synchronize()
        check_rows(buf, gp.np_generate(cfg, req, salt=2 ** 63 + 5, compact=compact, ctr=ctr, word3=word3), stride, compact)
    assert env.get_state_all().tobytes() == before and env.stats() == stats        # the handle is only read, by both walks
    env.close()


# ------------------------------------------------------------------------------------------ buffers
def raw(env, mask, lengths, flags, salt, words, stride, count, got, len_stride=None):
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
    if len_stride is None:
        len_stride = env.n_snakes if lengths is None or isinstance(lengths, int) else lengths.shape[1]
    return env._L.msnake_generate_states(env._h, ptr(mask), ptr(lengths), len_stride, flags, salt, ptr(words), stride, ptr(count),
                                         ptr(got), None)


@functools.lru_cache(maxsize=None)
def small():
    cfg = gp.make_cfg("snake_env", 7, 3, 21, seed=31, env_id_base=4)
    env = make_env(cfg)
    env.reset()
    return cfg, env


def test_unselected_envs_are_not_written():
    import torch
    cfg, env = small()
    ctr, word3 = counters(env)
    stride = env.state_words_max
    buf = buffers(env, stride)
    mask = np.arange(21) % 4 != 1
    mask[[0, 20]] = [False, True]
    env.generate_states_device((6, 5, 4), mask=torch.from_numpy(mask).to(env.device), salt=3, out=buf.words, count_out=buf.count, got_out=buf.got)
    torch.cuda.synchronize()
    check_rows(buf, gp.np_generate(cfg, (6, 5, 4), mask=mask, salt=3, ctr=ctr, word3=word3), stride)
    # a byte mask with values other than 1, and one that selects nothing
    buf.refill()
    m8 = torch.from_numpy(np.where(mask, 0x80, 0).astype(np.uint8)).to(env.device)
    env.generate_states_device((6, 5, 4), mask=m8, salt=3, out=buf.words, count_out=buf.count, got_out=buf.got)
    torch.cuda.synchronize()
    check_rows(buf, gp.np_generate(cfg, (6, 5, 4), mask=mask, salt=3, ctr=ctr, word3=word3), stride)
    buf.refill()
    env.generate_states_device(3, mask=[], out=buf.words, count_out=buf.count, got_out=buf.got)
    torch.cuda.synchronize()
    assert buf.untouched("words") and buf.untouched("count") and buf.untouched("got")


def test_a_stride_below_the_count_and_absent_outputs():
    import torch
    cfg, env = small()
    ctr, word3 = counters(env)
    req = np.tile(np.array([[2, 2, 2], [9, 9, 9], [5, 0, 12]], np.int32), (7, 1))
    want = gp.np_generate(cfg, req, salt=8, ctr=ctr, word3=word3)
    stride = int(np.median(want[1]))
    assert (want[1] > stride).any() and (want[1] <= stride).any()
    buf = buffers(env, stride)
    lengths = lengths_tensor(env, cfg, req)
    assert raw(env, None, lengths, 1, 8, buf.words, stride, buf.count, buf.got) == 0
    torch.cuda.synchronize()
    check_rows(buf, want, stride)                         # the count is written, no word of a row that does not fit is
    buf.refill()                                          # the count alone
    assert raw(env, None, lengths, 1, 8, None, 0, buf.count, None) == 0
    torch.cuda.synchronize()
    assert buf.untouched("words") and buf.untouched("got") and buf.host("count").tolist() == want[1].tolist() and buf.guards_intact()
    buf.refill()                                          # got alone; then words alone
    assert raw(env, None, lengths, 1, 8, None, 0, None, buf.got) == 0
    torch.cuda.synchronize()
    assert buf.untouched("words") and buf.untouched("count") and np.array_equal(buf.host("got"), want[2]) and buf.guards_intact()
    wide = buffers(env, env.state_words_max)
    assert raw(env, None, lengths, 1, 8, wide.words, env.state_words_max, None, None) == 0
    torch.cuda.synchronize()
    assert wide.untouched("count") and wide.untouched("got") and wide.guards_intact()
    assert all(np.array_equal(wide.host("words")[e, :len(r)], r) for e, r in enumerate(want[0]))


def test_refusals_in_order_with_nothing_written():
    import torch
    cfg, env = small()
    stride = 64
    buf = buffers(env, stride)
    lengths = lengths_tensor(env, cfg, 3)
    odd = buf.words.data_ptr() + 2
    dead = ctypes.create_string_buffer(4)
    for h in (None, dead):
        assert env._L.msnake_generate_states(h, None, None, 0, 2, 0, None, 0, None, None, None) == E_HANDLE    # before any argument
    nw = make_env(gp.make_cfg("snake_env", 6, 2, 4, n_fruits=3), rules="new_world")
    nw.reset()
    l2 = torch.zeros((4, 2), dtype=torch.int32, device=nw.device)
    assert raw(nw, None, l2, 2, 0, odd, 0, None, None) == E_ARG and b"new_world" in nw._L.msnake_last_error()   # before the flags
    with pytest.raises(ValueError, match="new_world"):
        nw.generate_states_device(3)
    with pytest.raises(ValueError, match="new_world"):
        nw.scatter_device(3)
    nw.close()
    for args, text in (((None, lengths, 2, 0, odd, 0, None, None), b"flag"),                  # a flag, before len_dev
                       ((None, lengths, 0x80000001, 0, buf.words, stride, None, None), b"flag"),
                       ((None, None, 1, 0, odd, 0, None, None), b"len_dev"),                   # len_dev NULL, before the stride
                       ((None, lengths, 1, 0, buf.words, 0, buf.count, buf.got), b"stride"),   # words_dev with stride <= 0
                       ((None, lengths, 1, 0, buf.words, -5, buf.count, buf.got), b"stride"),
                       ((None, lengths, 1, 0, None, stride, None, None), b"nothing to write")):
        rc = raw(env, *args)
        assert rc == E_ARG and text in env._L.msnake_last_error(), (args, env._L.msnake_last_error())
    assert raw(env, None, lengths, 1, 0, odd, 0, None, None, len_stride=2) == E_ARG and b"len_stride" in env._L.msnake_last_error()
    for args in ((None, lengths, 1, 0, odd, stride, buf.count, buf.got), (None, lengths, 1, 0, buf.words, stride, buf.count.data_ptr() + 1, None),
                 (None, lengths, 1, 0, None, 0, None, buf.got.data_ptr() + 2)):
        assert raw(env, *args) == E_ALIGN, args
    assert raw(env, None, lengths.data_ptr() + 2, 1, 0, buf.words, stride, None, None) == E_ALIGN
    torch.cuda.synchronize()
    assert buf.untouched("words") and buf.untouched("count") and buf.untouched("got")


# ------------------------------------------------------------------------------------------ round trip and play
ROUND = {"S10": (gp.make_cfg("snake_env", 10, 3, 48, seed=41, env_id_base=9), (12, 8, 5)),
         "S19": (gp.make_cfg("snake_env", 19, 3, 32, seed=42), (70, 40, 20)),
         "A10": (gp.make_cfg("adversarial", 10, 3, 32, seed=43, env_id_base=2), (10, 10, 0))}


def play_from(cfg, env, rows, steps):
    """The oracle, started from the same states, is the master for `steps` steps of safe_greedy (the loop of
    gpu_harness.closed_loop, without its reset)."""
    ora = sp.make_oracle(cfg)
    ora.reset()
    for e, row in enumerate(rows):
        ora.set_state(e, gp.row_state(row))
    buf = action_buffers(env)
    E, ns, dim = cfg["num_envs"], cfg["n_snakes"], cfg["dim"]
    for t in range(steps):
        states = oracle_states(ora)
        want_a = np.array([sp.safe_greedy(st, dim, ns, None) for st in states], np.int32)
        want_m = np.stack([sp.np_safe_mask(st, dim, ns) for st in states])
        out, safe = env.scripted_actions_device("safe_greedy", out=buf.act, safe_out=buf.safe)[:2]
        assert np.array_equal(out.cpu().numpy(), want_a) and np.array_equal(safe.cpu().numpy(), want_m), t
        obs, rew, done, info = env.step_device(out)
        o_obs, o_rew, o_done, o_ns, _, _ = ora.step(want_a)
        assert np.array_equal(rew.cpu().numpy(), o_rew) and np.array_equal(done.cpu().numpy(), o_done), t
        assert np.array_equal(info.cpu().numpy()[:, 2], o_ns), t
        if t % 10 == 0 or t == steps - 1:
            assert np.array_equal(obs.cpu().numpy(), o_obs), t
    assert buf.guards_intact() and env.stats()["errors"] == 0


@pytest.mark.parametrize("key", list(ROUND))
def test_generate_import_export_and_fifty_steps_against_the_oracle(key):
    import torch
    cfg, req = ROUND[key]
    env = make_env(cfg)
    env.reset()
    compiled = env.kernel_name().count(",") == 4
    assert compiled == (key == "S19")
    ctr, word3 = counters(env)
    compact = key != "A10"                                                 # the plain walk on the adversarial handle
    want = gp.np_generate(cfg, req, salt=5, compact=compact, ctr=ctr, word3=word3)
    words, count, got = env.generate_states_device(req, salt=5, compact=compact)
    status = env.import_states_device(words, count=count)
    assert (status.cpu().numpy() == STATE_OK).all()                        # every generated row lies in the acceptance domain
    out, n = env.export_states_device()
    rows, cnt = out.cpu().numpy(), n.cpu().numpy()
    assert all(cnt[e] == len(w) and np.array_equal(rows[e, :cnt[e]], w) for e, w in enumerate(want[0]))
    assert np.array_equal(got.cpu().numpy(), want[2])
    assert env.kernel_name().count(",") == (4 if compiled else 3)          # heads inside the grid: the handle keeps its kernels
    play_from(cfg, env, want[0], 50)
    env.close()


def test_scatter_device_equals_generate_then_import():
    import torch
    cfg, req = ROUND["S10"]
    a, b = make_env(cfg), make_env(cfg)
    a.reset(), b.reset()
    mask = torch.from_numpy(np.arange(cfg["num_envs"]) % 3 != 0).to(a.device)
    lengths = lengths_tensor(a, cfg, gp.mixed_requests(cfg["num_envs"], np.random.default_rng(6)))
    for salt, m in ((1, mask), (2, None), (3, ~mask)):
        words, count, got = a.generate_states_device(lengths, mask=m, salt=salt, compact=salt != 2)
        status = a.import_states_device(words, mask=m, count=count)
        s2, g2 = b.scatter_device(lengths, mask=m, salt=salt, compact=salt != 2)
        sel = np.ones(cfg["num_envs"], bool) if m is None else m.cpu().numpy()
        assert np.array_equal(s2.cpu().numpy(), status.cpu().numpy())
        assert np.array_equal(s2.cpu().numpy(), np.where(sel, STATE_OK, STATE_SKIPPED))
        assert np.array_equal(g2.cpu().numpy()[sel], got.cpu().numpy()[sel])
        assert a.get_state_all().tobytes() == b.get_state_all().tobytes(), salt
    a.close(), b.close()


def test_a_captured_generate_writes_the_same_rows():
    import torch
    cfg, env = small()
    ctr, word3 = counters(env)
    stride = env.state_words_max
    buf = buffers(env, stride)
    req = np.random.default_rng(8).integers(0, 20, (21, 3)).astype(np.int32)
    lengths = lengths_tensor(env, cfg, np.zeros((21, 3), np.int32))
    mask = torch.ones(21, dtype=torch.uint8, device=env.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # warm-up on the side stream, as graph capture wants
        env.generate_states_device(lengths, mask=mask, salt=4, out=buf.words, count_out=buf.count, got_out=buf.got)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        env.generate_states_device(lengths, mask=mask, salt=4, out=buf.words, count_out=buf.count, got_out=buf.got)
    torch.cuda.synchronize()
    for k in range(2):                                     # the replay reads the lengths and the mask that are there now
        sel = np.arange(21) % 2 == k
        lengths.copy_(torch.from_numpy(req).to(env.device))
        mask.copy_(torch.from_numpy(sel.astype(np.uint8)).to(env.device))
        buf.refill()
        g.replay()
        torch.cuda.synchronize()
        check_rows(buf, gp.np_generate(cfg, req, mask=sel, salt=4, ctr=ctr, word3=word3), stride, k)


# ------------------------------------------------------------------------------------------ the learner's random starts
@pytest.mark.parametrize("kind", ["frame", "window", "all_snakes"])
def test_runner_starts_ended_episodes_from_generated_positions(kind):
    """Episodes capped at 3 steps end all the time; with random_starts = 1 every one of them restarts from a generated
    position, so bodies of 6 and more pieces -- which 3 steps from a reset cannot grow -- are all over the batch, the frame
    the learner sees next is the frame of that state, and no kernel reports an error."""
    import torch
    from msnake import selfplay
    cfg = gp.make_cfg("snake_env", 10, 3, 32, seed=51, max_steps=3)
    env = make_env(cfg, auto_reset=kind != "all_snakes")
    torch.manual_seed(0)
    if kind == "frame":
        model, kw, opp = selfplay.CnnPolicy(env.obs_shape[:2] + (3,)).to(env.device), {}, [None, None]
    elif kind == "window":
        model, kw, opp = selfplay.WindowPolicy(2).to(env.device), dict(local_radius=2), [None, None]
    else:
        model, kw, opp = selfplay.RayPolicy().to(env.device), dict(rays=True, all_snakes=True), []
    runner = selfplay.Runner(env, model, opp, 12, 0.99, 0.95, random_starts=1.0, start_lengths=(6, 9), **kw)
    out = runner.run()
    assert all(torch.isfinite(x.float()).all() for x in out[:6]) and runner.start_salt == 12
    states = [gp.row_state(w) for w in blob_words(env.get_state_all())]
    longest = np.array([max(len(b) for b in st["snakes"]) for st in states])
    assert (longest >= 6).sum() >= 8, longest.tolist()
    if kind == "frame":
        assert torch.equal(runner.obs, env.render_device(out=torch.empty_like(runner.obs)))
    else:
        win = runner.win.clone()
        runner.observe_local()
        assert torch.equal(win, runner.win)
    assert env.stats()["errors"] == 0
    env.close()
