"""What a GPU test of an entry point needs: a handle from a scenario, output buffers between guard elements, the install
of hand-built states, and the closed loop with the CPU oracle as master.  Nothing here is collected as a test; the
harness itself is tested on the CPU by tests/test_gpu_harness_host.py.
"""

import math
import types

import numpy as np

import scripted_play as sp

GUARD = 64  # guard elements on each side of an output buffer


def make_env(cfg, **kw):
    import msnake
    base = dict(num_envs=cfg["num_envs"], dim=cfg["dim"], n_snakes=cfg["n_snakes"], n_fruits=cfg["n_fruits"],
                rules=cfg["rules"], seed=cfg["seed"], env_id_base=cfg["env_id_base"], max_steps=cfg["max_steps"])
    base.update(kw)
    return msnake.MultiSnakeVecEnv(**base)


# ------------------------------------------------------------------------------------------ guarded outputs
class GuardedOutputs:
    """One flat tensor per output, filled with a sentinel; the payload lies between `guard` elements on each side.

    spec: name -> dict(dtype=, shape=, fill=, offset=0, align=None, guard=GUARD, slack=0).  dtype is "uint8", "uint16",
    "int32" or "float32"; a uint16 output is stored as int16 and handed out as a uint16 view.  The payload starts
    `offset` bytes behind the front guard, `slack` more elements follow the back guard, and with `align` the front guard
    starts on a multiple of that many bytes (so with the default guard and offset 0 the payload does too).
    `buf.<name>` is the view to hand to the library."""

    def __init__(self, device, spec):
        import torch
        self.device, self._e = device, {}
        for name, s in spec.items():
            self._e[name] = self._make(torch, **s)

    def _make(self, torch, dtype, shape, fill, offset=0, align=None, guard=GUARD, slack=0):
        e = types.SimpleNamespace()
        store = torch.int16 if dtype == "uint16" else getattr(torch, dtype)
        e.np_dtype = np.dtype(dtype)
        item = e.np_dtype.itemsize
        assert offset % item == 0 and (align or item) % item == 0
        e.shape, e.size = tuple(shape), math.prod(shape)
        # the sentinel as the stored dtype holds it (0xA5A5 in an int16, 0xA5A5A5A5 in an int32) and as the host reads it
        if e.np_dtype.kind == "f":
            e.stored = e.sentinel = float(fill)
        else:
            bits = np.array([fill % (1 << 8 * item)], np.dtype(f"u{item}"))
            e.stored, e.sentinel = bits.view(np.int16 if dtype == "uint16" else e.np_dtype)[0].item(), bits.view(e.np_dtype)[0]
        room = (align or item) // item - 1
        e.raw = torch.full((room + guard + offset // item + e.size + guard + slack,), e.stored, dtype=store, device=self.device)
        lead = -e.raw.data_ptr() % (align or item)
        assert lead % item == 0 and lead // item <= room
        e.lo = lead // item + guard + offset // item
        view = e.raw[e.lo:e.lo + e.size]
        e.view = (view.view(torch.uint16) if dtype == "uint16" else view).view(e.shape)
        assert align is None or (e.view.data_ptr() - guard * item - offset) % align == 0
        return e

    def __getattr__(self, name):
        try:
            return self.__dict__["_e"][name].view
        except KeyError:
            raise AttributeError(name) from None

    def _all(self, name):
        e = self._e[name]
        return e, e.raw.cpu().numpy().view(e.np_dtype)

    def host(self, name):
        """The payload as a NumPy array, read from the whole buffer."""
        e, a = self._all(name)
        return a[e.lo:e.lo + e.size].reshape(e.shape)

    def refill(self, names=None):
        for name in self._e if names is None else names:
            self._e[name].raw.fill_(self._e[name].stored)

    def guards_intact(self):
        """Everything outside the payloads still holds the sentinel: both guards, the offset bytes, the slack."""
        for name in self._e:
            e, a = self._all(name)
            if not ((a[:e.lo] == e.sentinel).all() and (a[e.lo + e.size:] == e.sentinel).all()):
                return False
        return True

    def untouched(self, name):
        """The whole buffer, payload included, still holds the sentinel."""
        e, a = self._all(name)
        return bool((a == e.sentinel).all())


def action_spec(env, stride=None):
    """An int32 [n, stride] action buffer filled with -77 and a uint8 [n, ns] mask buffer filled with 0xA5."""
    n, ns = env.num_envs, env.n_snakes
    return {"act": dict(dtype="int32", shape=(n, stride or ns), fill=-77), "safe": dict(dtype="uint8", shape=(n, ns), fill=0xA5)}


def count_spec(env, name):
    """A uint16 [n, ns, 4] buffer of per-move counts filled with 0xA5A5."""
    return {name: dict(dtype="uint16", shape=(env.num_envs, env.n_snakes, 4), fill=0xA5A5)}


def action_buffers(env, stride=None):
    return GuardedOutputs(env.device, action_spec(env, stride))


# ------------------------------------------------------------------------------------------ states in, states out
def install(cfg, states, with_oracle=False, max_steps=2000, **kw):
    """The state dicts into a fresh handle (set_state_words), one env per state, and into a fresh oracle when asked for
    (Oracle.set_state); read back from the handle, they are what was built.  Both get the episode cap `max_steps`
    (under new_world the body storage follows it).  Returns env, or (env, oracle)."""
    from oracle.snake_oracle import flat_to_state, state_to_flat
    cfg = dict(cfg, num_envs=len(states), seed=1, env_id_base=0, max_steps=max_steps)
    env, ora = make_env(cfg, **kw), sp.make_oracle(cfg) if with_oracle else None
    env.reset()
    if ora is not None:
        ora.reset()
    for e, st in enumerate(states):
        env.set_state_words(e, state_to_flat(st, cfg["n_snakes"]))
        if ora is not None:
            ora.set_state(e, st)
    for e in sorted({0, len(states) // 2, len(states) - 1}):   # the state went in as it was built
        got = flat_to_state(env.get_state_words(e))
        assert got["snakes"] == states[e]["snakes"] and got["fruits"] == states[e]["fruits"], e
        assert [list(v) for v in got["vels"]] == [list(v) for v in states[e]["vels"]], e
    return (env, ora) if with_oracle else env


def oracle_states(ora):
    read = sp._StateReader(ora)
    return [read(e) for e in range(ora.num_envs)]


def play_random(env, ora, steps, rng, threads=16):
    """Seeded random play of both (random play dies young, which keeps resets in the picture); outputs compared."""
    import torch
    for t in range(steps):
        act = rng.integers(0, 5, (env.num_envs, env.n_snakes)).astype(np.int32)
        _, rew, done, _ = env.step_device(torch.from_numpy(act).to(env.device))
        _, o_rew, o_done, *_ = ora.step(act, threads=threads, want_obs=False)
        assert np.array_equal(done.cpu().numpy(), o_done) and np.array_equal(rew.cpu().numpy(), o_rew), t


# ------------------------------------------------------------------------------------------ closed loop
def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _where(got, want):
    return np.argwhere(got != want)[:4].tolist() if got.shape == want.shape else (got.shape, want.shape)


def closed_loop(cfg, env, call, expected, steps, control=None, stride=None, obs_every=50, observe=None, buffers=action_buffers):
    """The oracle is the master: at every step the expectations on the oracle's state are compared with the library's
    outputs for every env, snake and entry, both are stepped with the expected actions, and the step outputs are
    compared.
      expected(states) -> (want_actions, want_mask, *want_extras), from the oracle's canonical state dicts;
      call(env, buf, snakes) -> (out, safe, *extras), tensors or host arrays, out being buf.act;
      buffers(env, stride) -> the GuardedOutputs the loop hands to `call`;
      control=(rng, scripted_snakes): only those snakes are scripted, the other columns carry seeded random actions
      pre-filled in the buffer, and the surplus columns of a wider stride a value that must stay;
      observe(t, states, wants, o_done, o_ep_len), after step t: the oracle's states behind the step, the expectations
      the step was compared with, and the oracle's done flags and episode lengths."""
    import torch
    E, ns = cfg["num_envs"], cfg["n_snakes"]
    ora = sp.make_oracle(cfg)
    assert np.array_equal(env.reset(), ora.reset())
    buf = buffers(env, stride)
    states = oracle_states(ora)
    for t in range(steps):
        wants = expected(states)
        want_a, want_m, *want_x = wants
        snakes = rand = None
        if control is not None:
            rng, snakes = control
            rand = rng.integers(0, 5, (E, buf.act.shape[1])).astype(np.int32)
            rand[:, ns:] = -5 - t % 3                              # surplus columns: never written
            buf.act.copy_(torch.from_numpy(rand).to(env.device))
            keep = [s for s in range(ns) if s not in snakes]
            want_a[:, keep] = rand[:, keep]
        out, safe, *extras = call(env, buf, snakes)
        got = _np(out)
        assert np.array_equal(got[:, :ns], want_a), (t, "action", _where(got[:, :ns], want_a))
        if rand is not None:
            assert np.array_equal(got[:, ns:], rand[:, ns:]), (t, "surplus columns")
        got = _np(safe)
        assert np.array_equal(got, want_m), (t, "mask", _where(got, want_m))
        assert len(extras) == len(want_x), (len(extras), len(want_x))
        for k, (got, want) in enumerate(zip(extras, want_x)):
            got = _np(got)
            assert np.array_equal(got, want), (t, "extra output", k, _where(got, want))
        obs, rew, done, info = env.step_device(out)
        o_obs, o_rew, o_done, o_ns, _, o_el = ora.step(want_a)
        assert np.array_equal(_np(rew), o_rew) and np.array_equal(_np(done), o_done), t
        assert np.array_equal(_np(info)[:, 2], o_ns), t
        if t % obs_every == 0 or t == steps - 1:
            assert np.array_equal(_np(obs), o_obs), t
        states = oracle_states(ora)
        if observe is not None:
            observe(t, states, wants, o_done, o_el)
    assert buf.guards_intact()
    assert env.stats()["errors"] == 0
