"""The top of the documented ranges on the device: max_steps 60000, body rings of 60032 cells, bodies past 32767 pieces.

The scenarios are tests/limits_play.py's (tests/test_limits_host.py proves on the oracle alone that each does what it is
there for).  The CPU oracle is the master: it is recorded once per scenario and process, and every kernel path is held
against the same record.  Every comparison is byte-exact -- words, frames, rewards, dones, infos, stats --, every output
buffer comes from gpu_harness.GuardedOutputs, and every guard element must survive.

Lengths, ring capacities, ring positions and step counts of this range all travel through 16-bit fields (len << 16 in a
state word, max_steps << 16 and cap << 16 in the kernel arguments, ring indices) that are right only while they are read
as unsigned: a signed shift, an int16 or a signed compare anywhere on the way shows here and nowhere else in the suite.

The long states go in through set_state_words as words, not through gpu_harness.install: turning a 60000-piece state
dict into words takes longer than everything the device does with it.
"""
import numpy as np
import pytest

import gpu_harness as gh
import limits_play as lp
import state_domain as sd

pytestmark = pytest.mark.gpu

PATHS = ["step", "tape", "rollout"]
EPBS = [1, 8]
FILL = dict(obs=0xA5, rew=-77.5, done=0xA5, info=-0x5A5A5A5B)           # (the int32 whose bytes are all 0xA5)
GENERIC = "msnake_step_kernel<%d, %d, 0, 1>"
SPEC = "msnake_step_kernel<0, %d, 0, 1, %d>"


def make_env(cfg, n, **kw):
    import msnake
    return msnake.MultiSnakeVecEnv(n, seed=lp.SEED, **cfg, **kw)


def install_words(env, words):
    env.reset()
    for e, w in enumerate(words):
        env.set_state_words(e, w)
    return env


def words_of(env):
    return sd.blob_words(env.get_state_all())


def same(got, want, what):
    """Byte for byte, dtype and shape included (floats by their bits)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        g, w = (a.view(f"u{a.dtype.itemsize}") for a in (got, want))
        where = np.argwhere(g != w)
        raise AssertionError((what, len(where), where[:6].tolist(), got[tuple(where[0])].item(), want[tuple(where[0])].item()))


class Outputs:
    """The four step outputs for up to T steps between guard elements, and the three step paths writing into them.
    The frames start on a 128-byte line (`offset` bytes behind one)."""

    def __init__(self, env, T, offset=0):
        n, (H, W, C) = env.num_envs, env.obs_shape
        self.env, self.T, self.frame = env, T, n * H * W * C
        self.buf = gh.GuardedOutputs(env.device, dict(
            obs=dict(dtype="uint8", shape=(T, n, H, W, C), fill=FILL["obs"], guard=128, align=128, offset=offset),
            rew=dict(dtype="float32", shape=(T, n), fill=FILL["rew"]),
            done=dict(dtype="uint8", shape=(T, n), fill=FILL["done"]),
            info=dict(dtype="int32", shape=(T, n, 4), fill=FILL["info"])))
        assert self.buf.obs.data_ptr() % 128 == offset

    def pointers(self, k=0):
        b = self.buf
        return b.obs[k].data_ptr(), b.rew[k].data_ptr(), b.done[k].data_ptr(), b.info[k].data_ptr()

    def run(self, acts, path):
        """acts [T', n, ns] on msnake_step ("step": one call per step), msnake_step_tape ("tape") or msnake_rollout_tape
        ("rollout"), step k into row k.  Returns the T' rows (obs, rew, done, info) as host arrays; the rows behind them
        still hold the sentinel."""
        import torch
        from msnake import _capi
        env, b, T = self.env, self.buf, len(acts)
        assert 1 <= T <= self.T
        b.refill()
        tape = torch.from_numpy(np.ascontiguousarray(acts, np.int32)).to(env.device)
        ns, n, L = env.n_snakes, env.num_envs, env._L
        if path == "step":
            for k in range(T):
                _capi.check(L.msnake_step(env._h, tape[k].data_ptr(), ns, *self.pointers(k), env._stream()), "msnake_step")
        else:
            fn = L.msnake_step_tape if path == "tape" else L.msnake_rollout_tape
            _capi.check(fn(env._h, tape.data_ptr(), ns, T, *self.pointers()[:1], self.frame, *self.pointers()[1:], n, env._stream()),
                        "msnake_rollout_tape" if path == "rollout" else "msnake_step_tape")
        torch.cuda.synchronize(env.device)
        out = []
        for name in ("obs", "rew", "done", "info"):
            a = b.host(name)
            assert (a[T:] == np.array(FILL[name]).astype(a.dtype)).all(), (name, "rows behind the last step were written")
            out.append(a[:T])
        assert b.guards_intact()
        return out


def compare_steps(rec, lo, got, what, skip=()):
    """Rows of Outputs.run against steps lo + 1 .. lo + T' of the record, for every env outside `skip`."""
    keep = [e for e in range(rec.n) if e not in skip]
    obs, rew, done, info = got
    for j in range(len(rew)):
        k = lo + j
        same(rew[j][keep], rec.rew[k][keep], (what, "reward", k + 1))
        same(done[j][keep], rec.done[k][keep], (what, "done", k + 1))
        same(info[j][keep], rec.info[k][keep], (what, "info", k + 1))
        same(obs[j][keep], rec.obs[k][keep], (what, "frame", k + 1))


def play(env, out, rec, lo, hi, path, what, skip=()):
    compare_steps(rec, lo, out.run(rec.acts[lo:hi], path), what, skip)


# ------------------------------------------------------------------------------------------ the read-only entry points
def readonly_buffers(env):
    n, ns, dim = env.num_envs, env.n_snakes, int(env.cfg.dim)
    u16 = dict(dtype="uint16", fill=0xA5A5, align=4)
    u8 = dict(dtype="uint8", fill=0xA5, align=4)
    spec = dict(gh.action_spec(env))
    for name in ("space", "territory", "path", "reach"):
        spec.update(gh.count_spec(env, name))
    spec.update(field=dict(u16, shape=(n, dim, dim)), life=dict(u16, shape=(n, dim, dim)),
                dist=dict(u16, shape=(n, ns, dim, dim)), counts=dict(u16, shape=(n, ns)), owner=dict(u8, shape=(n, dim, dim)),
                cells=dict(u8, shape=(n,) + env.cells_shape), table=dict(dtype="int32", fill=-77, shape=(n, ns, 8)),
                local2=dict(u8, shape=(n,) + env.local_shape(2)), local31=dict(u8, shape=(n,) + env.local_shape(31)),
                heading=dict(u8, shape=(n, ns)), rays=dict(u8, shape=(n,) + env.rays_shape()))
    return gh.GuardedOutputs(env.device, spec)


def check_readonly(env, ro, want, words, what):
    """get_state_all, render_cells with the table, every scripted policy with its extra outputs, head_fields,
    render_local at radius 2 and 31 and render_rays against limits_play.expectations on the oracle's states."""
    sd.assert_words(words_of(env), words, (what, "get_state_all"))
    ro.refill()
    env.render_cells_device(out=ro.cells, snakes_out=ro.table)
    same(ro.host("cells"), want["cells"], (what, "cells"))
    same(ro.host("table"), want["table"], (what, "table"))
    for policy, outs in (("safe_greedy", ()), ("space_greedy", ("space",)), ("territory_greedy", ("territory",)),
                         ("path_greedy", ("path", "field")), ("timed_greedy", ("reach", "life"))):
        ro.refill(["act", "safe"])
        env.scripted_actions_device(policy, out=ro.act, safe_out=ro.safe, **{name + "_out": getattr(ro, name) for name in outs})
        same(ro.host("act"), want[policy], (what, policy))
        same(ro.host("safe"), want["safe"], (what, policy, "safe mask"))
        for name in outs:
            same(ro.host(name), want[name], (what, policy, name))
    env.head_fields_device(dist_out=ro.dist, owner_out=ro.owner, counts_out=ro.counts)
    for name in ("dist", "owner", "counts"):
        same(ro.host(name), want[name], (what, "head_fields", name))
    for radius in (2, 31):
        ro.refill(["heading"])
        env.render_local_device(radius, out=getattr(ro, f"local{radius}"), heading_out=ro.heading)
        same(ro.host(f"local{radius}"), want[f"local{radius}"], (what, "render_local", radius))
        same(ro.host("heading"), want["heading"], (what, "render_local heading", radius))
    ro.refill(["heading"])
    env.render_rays_device(out=ro.rays, heading_out=ro.heading)
    same(ro.host("rays"), want["rays"], (what, "render_rays"))
    same(ro.host("heading"), want["heading"], (what, "render_rays heading"))
    assert ro.guards_intact(), what


# ------------------------------------------------------------------------------------------ A. long bodies in and out
@pytest.mark.parametrize("case", sorted(lp.LONG))
def test_long_bodies_install_and_come_back(case):
    """Bodies of 32767 .. 60030 pieces: get_state and get_state_all return the words that went in, render shows the
    oracle's frame, the exported blob round-trips through set_state_all into a second handle.  One piece more than the
    cap takes, and a length whose low 16 bits are 0, are refused for their length and leave the env as it was."""
    import torch
    cfg, words = lp.cfg_of(lp.LONG[case]["max_steps"]), lp.long_states(case)
    n, cap = len(words), sd.cap(lp.cfg_of(lp.LONG[case]["max_steps"]))
    ora = lp.make_oracle(cfg, words)
    env, twin = install_words(make_env(cfg, n), words), make_env(cfg, n, envs_per_block=8)
    frames = gh.GuardedOutputs(env.device, {"obs": dict(dtype="uint8", shape=(n,) + env.obs_shape, fill=FILL["obs"])})

    def check(h, what):
        for e in range(n):
            same(h.get_state_words(e), words[e], (what, "get_state", e))
        sd.assert_words(words_of(h), words, (what, "get_state_all"))
        frames.refill()
        h.render_device(out=frames.obs)
        torch.cuda.synchronize()
        same(frames.host("obs"), ora.render(), (what, "render"))

    check(env, "installed")
    twin.reset()
    twin.set_state_all(env.get_state_all())
    check(twin, "set_state_all of the exported blob")
    for e, bad in ((1, lp.too_long_words(cap - 1)), (n - 1, lp.too_long_words(65536, cells=cap - 2)), (0, lp.too_long_words(65536, cells=2))):
        assert sd.accepts(cfg, bad) == sd.R_LEN
        with pytest.raises(RuntimeError, match=sd.REASON_RE[sd.R_LEN]) as err:
            env.set_state_words(e, bad)
        assert "(-5)" in str(err.value)
        blob = [w for w in words]
        blob[e] = bad
        with pytest.raises(RuntimeError, match=rf"1 env state\(s\) rejected; first: env {e}: {sd.REASON_RE[sd.R_LEN]}"):
            twin.set_state_all(sd.make_blob(cfg, blob))
    check(env, "after the refusals")
    check(twin, "after the refused blobs")
    assert frames.guards_intact()
    assert env.stats()["errors"] == 0 and twin.stats()["errors"] == 0
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------ B. the rotated ring above 2^15
@pytest.mark.parametrize("epb", EPBS)
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", sorted(lp.LONG))
def test_long_bodies_driven_along_the_cycle(case, path, epb):
    """130 clear steps and 10 more through the self-hit, every step's outputs against the oracle's; at the steps of
    limits_play.check_steps every read-only entry point against its model on the oracle's state.  After the first step
    the ring position is cap - 1: above 2^15 throughout in case a, coming down past 2^15 in case b."""
    rec = lp.long_play(case)
    env = install_words(make_env(rec.cfg, rec.n, envs_per_block=epb), rec.start)
    at = lp.check_steps(case)
    bounds = sorted(set(at) | {0, rec.steps})
    out, ro = Outputs(env, max(b - a for a, b in zip(bounds, bounds[1:]))), readonly_buffers(env)
    for lo, hi in zip([None] + bounds, bounds):
        if lo is not None:
            play(env, out, rec, lo, hi, path, (case, path, epb))
        if hi in at:
            check_readonly(env, ro, lp.long_expectations(case, hi), rec.words[hi], (case, path, epb, "step", hi))
    sd.assert_words(words_of(env), rec.end, "the words after the last step")
    assert env.stats()["errors"] == 0
    env.close()


# ------------------------------------------------------------------------------------------ C. the guard at the largest cap
@pytest.mark.parametrize("epb", EPBS)
@pytest.mark.parametrize("path", PATHS)
def test_the_capacity_guard_at_cap_60032(path, epb):
    """cap - 2 pieces with grow_to 2^31 - 1: cap - 1 after the first step, like the oracle and without an error; from the
    second step on the guard holds the body at cap - 1 and counts one error per step.  The other envs of the handle
    follow the oracle throughout."""
    rec, V = lp.guard_play(), lp.GUARD_VICTIM
    cap = sd.cap(rec.cfg)
    env = install_words(make_env(rec.cfg, rec.n, envs_per_block=epb), rec.start)
    out = Outputs(env, rec.steps)
    play(env, out, rec, 0, 1, path, "first")
    sd.assert_words(words_of(env), rec.words[1], "first")
    assert lp.body_len(env.get_state_words(V)) == cap - 1 and env.stats()["errors"] == 0

    def after(k):
        got = words_of(env)
        for e in range(rec.n):
            if e != V:
                same(got[e], rec.words[k][e], ("the other envs after step", k, e))
        assert lp.body_len(got[V]) == cap - 1 and lp.body_len(rec.words[k][V]) == cap - 2 + k
        assert env.stats()["errors"] == k - 1, k

    if path == "step":
        for k in range(2, rec.steps + 1):
            play(env, out, rec, k - 1, k, path, "guarded", (V,))
            after(k)
    else:
        play(env, out, rec, 1, rec.steps, path, "guarded", (V,))
        after(rec.steps)
    env.close()


# ------------------------------------------------------------------------------------------ D. copies between capacities
@pytest.mark.parametrize("epb", EPBS)
def test_copy_envs_between_cap_60032_and_cap_32832(epb):
    """Into the smaller handle: a body of its cap - 1 pieces arrives word for word (one more than set_state takes);
    bodies of cap and of 60030 pieces leave their envs untouched and count one error each.  The envs that arrived play
    on like the oracle.  Then the other way, into the large handle after 40 steps have rotated its rings."""
    C = lp.COPY
    src_cfg, dst_cfg = lp.cfg_of(C["src_max_steps"]), lp.cfg_of(C["dst_max_steps"])
    src_rec, dst_rec, back_rec = lp.copy_src_play(), lp.copy_dst_play(), lp.copy_back_play()
    words, n = src_rec.start, src_rec.n
    fit = [lp.fits(dst_cfg, w) for w in words]
    src = install_words(make_env(src_cfg, n, envs_per_block=epb), words)
    # the identity copy into a handle fresh from a reset
    dst = make_env(dst_cfg, n)
    frame = dst.reset().copy()
    before = words_of(dst)
    dst.copy_envs_device(src)
    got = words_of(dst)
    for e in range(n):
        same(got[e], words[e] if fit[e] else before[e], ("copy into the smaller handle", e))
    same(dst.render()[[e for e in range(n) if not fit[e]]], frame[[e for e in range(n) if not fit[e]]], "frames of the envs left alone")
    assert dst.stats()["errors"] == fit.count(False) == 2 and src.stats()["errors"] == 0
    assert lp.body_len(got[0]) == sd.cap(dst_cfg) - 1
    dst.close()
    # the envs that fit, gathered into slots 0.. of another handle, play on
    small = make_env(dst_cfg, dst_rec.n, envs_per_block=epb)
    small.reset()
    small.copy_envs_device(src, [e for e in range(n) if fit[e]])
    sd.assert_words(words_of(small), dst_rec.start, "gathered copy")
    out = Outputs(small, dst_rec.steps)
    play(small, out, dst_rec, 0, dst_rec.steps, "step", "the smaller handle plays on")
    sd.assert_words(words_of(small), dst_rec.end, "the smaller handle after the play")
    assert small.stats()["errors"] == 0
    # the other way: the large handle's rings have rotated
    out = Outputs(src, src_rec.steps)
    play(src, out, src_rec, 0, src_rec.steps, "rollout", "the large handle rotates its rings")
    sd.assert_words(words_of(src), src_rec.end, "the large handle after 40 steps")
    install_words(small, lp.copy_back_states())
    src.copy_envs_device(small, list(C["back"]))
    sd.assert_words(words_of(src), back_rec.start, "copy into the large handle")
    play(src, out, back_rec, 0, back_rec.steps, "step", "the large handle plays on")
    sd.assert_words(words_of(src), back_rec.end, "the large handle after the play")
    assert src.stats()["errors"] == 0 and small.stats()["errors"] == 0
    src.close()
    small.close()


# ------------------------------------------------------------------------------------------ E. the step cap
def _cap_env(key, max_steps, **kw):
    from oracle.snake_oracle import flat_to_state
    cfg, words = lp.cap_states(key, max_steps)
    shape = {k: v for k, v in cfg.items() if k != "max_steps"}
    env = gh.install(shape, [flat_to_state(w) for w in words], max_steps=max_steps, **kw)
    sd.assert_words(words_of(env), words, "installed")
    return cfg, env


def _totals(rec):
    """(episodes, ep_len_sum) of a record without masked resets: an episode counts on the step it ends, once."""
    first = rec.done.astype(bool) & ~np.concatenate([np.zeros((1, rec.n), bool), rec.done[:-1].astype(bool)])
    return int(first.sum()), int(rec.info[:, :, 1][first].sum())


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("max_steps", [60000, 32768])
@pytest.mark.parametrize("key", sorted(lp.CAP_CONFIGS))
def test_the_step_cap_ends_the_episode_where_the_oracle_does(key, max_steps, path):
    """t = ep_len = max_steps - 4 + (e mod 4) installed on states from play, auto_reset off, six random steps: done, the
    reported episode length (max_steps at the cap) and every other output follow the oracle.  On msnake_step every step
    with a done env is followed by the masked reset: truncated, the terminal frames and the reset frames are the oracle's;
    on the tape paths a finished env stays done.  The episode totals are the oracle's."""
    import torch
    cfg, env = _cap_env(key, max_steps, auto_reset=False)
    rules = sd.RULES[cfg["rules"]]
    assert env.kernel_name() == GENERIC % (rules, cfg["n_snakes"])       # (the compiled shapes need the auto reset: below)
    out = Outputs(env, lp.CAP_STEPS)
    if path != "step":
        rec = lp.cap_play(key, max_steps, resets=False)
        play(env, out, rec, 0, rec.steps, path, (key, max_steps, path))
        episodes, ep_len_sum = _totals(rec)
    else:
        rec = lp.cap_play(key, max_steps, resets=True)
        n = rec.n
        r = gh.GuardedOutputs(env.device, {"obs": dict(dtype="uint8", shape=(n,) + env.obs_shape, fill=FILL["obs"]),
                                           "final": dict(dtype="uint8", shape=(n,) + env.obs_shape, fill=FILL["obs"]),
                                           "trunc": dict(dtype="uint8", shape=(n,), fill=FILL["done"])})
        for k in range(rec.steps):
            obs, rew, done, info = out.run(rec.acts[k:k + 1], "step")
            same(rew[0], rec.rew[k], ("reward", k + 1))
            same(done[0], rec.done[k], ("done", k + 1))
            same(info[0], rec.info[k], ("info", k + 1))
            if not rec.done[k].any():
                same(obs[0], rec.obs[k], ("frame", k + 1))
                continue
            sel = rec.done[k] != 0
            r.refill()
            r.obs.copy_(torch.from_numpy(obs[0]).to(env.device))
            env.reset_device(torch.from_numpy(done[0]).to(env.device), out=r.obs, final_out=r.final, truncated_out=r.trunc)
            same(r.host("trunc"), rec.truncated[k + 1], ("truncated", k + 1))
            same(r.host("final")[sel], rec.final[k + 1][sel], ("terminal frames", k + 1))
            assert (r.host("final")[~sel] == FILL["obs"]).all()
            same(r.host("obs"), rec.obs[k], ("frames after the masked reset", k + 1))
            assert r.guards_intact()
        episodes, ep_len_sum = rec.episodes, rec.ep_len_sum
        assert sum(int(t.sum()) for t in rec.truncated.values()) >= lp.CAP_N // 2      # the cap alone ended those
    sd.assert_words(words_of(env), rec.end, "the words after the play")
    st = env.stats()
    assert (st["episodes"], st["ep_len_sum"], st["errors"]) == (episodes, ep_len_sum, 0), st
    env.close()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("key", ["S10x1", "S19x3"])
def test_the_auto_reset_at_60000_on_the_compiled_shapes(key, path):
    """The kernels compiled for 19x19x3 and 10x10x1 (they need the auto reset) at max_steps 60000: the step on which the
    cap ends an episode resets it like the oracle's.  On msnake_step the calls alternate between the plain-call variant
    (frames on a 128-byte line) and the other one (16 bytes behind a line)."""
    from msnake import _capi
    cfg, env = _cap_env(key, 60000, auto_reset=True)
    assert env.kernel_name() == SPEC % (cfg["n_snakes"], cfg["dim"])
    rec = lp.cap_play(key, 60000, resets=False, auto_reset=True)
    assert rec.done.any() and (rec.info[:, :, 1].max() == 60000)
    if path == "step":
        outs, kinds = [Outputs(env, 1), Outputs(env, 1, offset=16)], []
        for k in range(rec.steps):
            kinds.append(_capi.call_shape_for_config(env.cfg, env.n_snakes, *outs[k % 2].pointers()))
            play(env, outs[k % 2], rec, k, k + 1, "step", (key, "call", kinds[-1]))
        assert kinds == ["plain", "shape"] * (rec.steps // 2)
    else:
        play(env, Outputs(env, rec.steps), rec, 0, rec.steps, path, (key, path))
    assert env.kernel_name() == SPEC % (cfg["n_snakes"], cfg["dim"])
    sd.assert_words(words_of(env), rec.end, "the words after the play")
    st = env.stats()
    assert (st["episodes"], st["ep_len_sum"], st["errors"]) == (int(rec.done.sum()), int(rec.info[:, :, 1][rec.done != 0].sum()), 0), st
    env.close()


# ------------------------------------------------------------------------------------------ F. the longest body of play
@pytest.mark.parametrize("epb", EPBS)
@pytest.mark.parametrize("path", PATHS)
def test_the_body_that_play_has_grown_by_the_cap(path, epb):
    """new_world without fruits never pops: at t = 59900 a body has 59900 pieces more than at the reset.  Driven to the
    cap it stays below cap - 1 (what sizing the storage by max_steps + 2 is for), no guard trips, done rises at 60000 and
    the auto reset follows."""
    rec = lp.reach_play()
    env = install_words(make_env(rec.cfg, rec.n, envs_per_block=epb), rec.start)
    cut = rec.steps - 3                                                  # the last step before the cap
    out = Outputs(env, cut)
    play(env, out, rec, 0, cut, path, "to the cap")
    sd.assert_words(words_of(env), rec.words[cut], "one step before the cap")
    assert max(lp.body_len(w) for w in rec.words[cut]) == lp.reach_body()[0] + cut < sd.cap(rec.cfg) - 1
    play(env, out, rec, cut, rec.steps, path, "through the cap")
    assert rec.done[cut].all() and (rec.info[cut, :, 1] == 60000).all()
    sd.assert_words(words_of(env), rec.end, "after the auto reset")
    st = env.stats()
    assert st["errors"] == 0 and st["ep_len_sum"] == int(rec.info[:, :, 1][rec.done != 0].sum())
    env.close()
