"""tests/gpu_harness.py on the CPU: the guarded buffers see a write outside the payload, the closed loop fails for every
kind of wrong output, and the install's round-trip check sees words that are not the ones it gave.

The closed loop runs against a stub env backed by a second CPU oracle; a fault is one wrong value in one of the stub's
host arrays at one step.  Nothing here touches a GPU.
"""
import types

import numpy as np
import pytest
import torch

import board_states as bs
import gpu_harness as gh
import scripted_play as sp

CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------ 1. GuardedOutputs
FILLS = {"uint8": 0xA5, "uint16": 0xA5A5, "int32": -77, "float32": -77.5}


def _buf(dtype, k, **kw):
    """A [5, 3] payload of `dtype` that starts k elements behind the front guard, and the payload's first raw index."""
    item = np.dtype(dtype).itemsize
    buf = gh.GuardedOutputs(CPU, {"x": dict(dtype=dtype, shape=(5, 3), fill=FILLS[dtype], offset=k * item, slack=3, **kw)})
    return buf, buf._e["x"]


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", list(FILLS))
def test_guarded_outputs_see_every_write_outside_the_payload(dtype, k):
    buf, e = _buf(dtype, k)
    assert tuple(buf.x.shape) == (5, 3) and buf.x.dtype == getattr(torch, dtype)
    assert len(e.raw) == 2 * gh.GUARD + k + 15 + 3 and e.lo == gh.GUARD + k
    assert buf.guards_intact() and buf.untouched("x")                       # a fresh buffer
    assert (buf.host("x") == np.array(FILLS[dtype]).astype(dtype)).all()
    for at in (e.lo - 1, e.lo + e.size, 0, len(e.raw) - 1):                  # just before, just behind, both far ends
        e.raw[at] = 0
        assert not buf.guards_intact() and not buf.untouched("x"), at
        buf.refill()
        assert buf.guards_intact() and buf.untouched("x"), at
    for at in (e.lo, e.lo + e.size - 1):                                     # the payload's first and last element
        e.raw[at] = 7
        assert buf.guards_intact() and not buf.untouched("x"), at
        assert buf.host("x").ravel()[at - e.lo] == 7 and (buf.x.reshape(-1).view(e.raw.dtype) == 7).sum() == 1
        buf.refill(["x"])
        assert buf.untouched("x"), at


def test_guarded_outputs_alignment_and_sentinels():
    for align in (4, 16, 64):
        buf, e = _buf("uint8", 0, align=align)
        assert buf.x.data_ptr() % min(align, gh.GUARD) == 0
        buf, e = _buf("uint8", 3, align=align)
        assert buf.x.data_ptr() % 4 == 3 and buf.guards_intact()
    buf, e = _buf("int32", 0, align=16, guard=3)                             # 12 bytes behind a 16-byte boundary
    assert buf.x.data_ptr() % 16 == 12 and len(e.raw) == 3 + 3 + 15 + 3 + 3
    buf, e = _buf("uint16", 1, align=4)                                      # 2-byte aligned and no more
    assert buf.x.data_ptr() % 4 == 2
    assert e.raw.dtype == torch.int16 and int(e.raw[0]) == 0xA5A5 - 0x10000 and buf.host("x").dtype == np.uint16
    table = gh.GuardedOutputs(CPU, {"t": dict(dtype="int32", shape=(2, 8), fill=0xA5A5A5A5)})
    assert table.host("t").view(np.uint32).min() == 0xA5A5A5A5 and table.untouched("t")
    two = gh.GuardedOutputs(CPU, dict(gh.count_spec(types.SimpleNamespace(num_envs=2, n_snakes=3), "space"),
                                      a=dict(dtype="int32", shape=(2, 3), fill=-77)))
    two._e["space"].raw[0] = 0
    assert not two.guards_intact() and two.untouched("a") and not two.untouched("space")
    two.refill(["a"])
    assert not two.guards_intact()
    with pytest.raises(AttributeError):
        two.nothing


# ------------------------------------------------------------------------------------------ 2. closed_loop
CFG = dict(sp.SCENARIOS["S6x2"], num_envs=4, eps=0.0, policy="safe_greedy")
STEPS, AT = 10, 5


def _lengths(states):
    """The stub's extra output: uint16 [E, ns, 4], every snake's body length four times."""
    return np.array([[[len(b)] * 4 for b in st["snakes"]] for st in states], np.uint16)


def _expected(states):
    pol = sp.POLICIES[CFG["policy"]]
    act = np.array([pol(st, CFG["dim"], CFG["n_snakes"], None, 0.0) for st in states], np.int32)
    mask = np.array([sp.np_safe_mask(st, CFG["dim"], CFG["n_snakes"]) for st in states], np.uint8)
    return act, mask, _lengths(states)


class StubEnv:
    """What closed_loop asks of a handle, answered on the CPU by a second oracle and the helpers; `fault` names the one
    value that is wrong at step AT."""

    def __init__(self, fault=None):
        self.cfg = types.SimpleNamespace(dim=CFG["dim"], rules=CFG["rules"])
        self.num_envs, self.n_snakes, self.device = CFG["num_envs"], CFG["n_snakes"], CPU
        self.ora, self.fault, self.t = sp.make_oracle(CFG), fault, 0

    def _is(self, fault):
        return self.fault == fault and self.t == AT

    def reset(self):
        return self.ora.reset()

    def scripted_actions_device(self, policy, snakes=None, out=None, safe_out=None, space_out=None):
        act, mask, lengths = _expected(gh.oracle_states(self.ora))
        act[0, 1] = (act[0, 1] + 1) % 5 if self._is("action") else act[0, 1]
        mask[1, 0] ^= 2 * self._is("mask")
        lengths[2, 1, 3] += self._is("extra")
        for s in range(self.n_snakes) if snakes is None else snakes:
            out[:, s] = torch.from_numpy(act[:, s])
        if self._is("surplus"):
            out[3, self.n_snakes] = 0
        if self._is("guard"):
            torch.as_strided(out, (1,), (1,), out.storage_offset() - 1).fill_(0)
        safe_out.copy_(torch.from_numpy(mask))
        space_out.view(torch.int16).copy_(torch.from_numpy(lengths.view(np.int16)))
        return out, safe_out, space_out

    def step_device(self, actions):
        act = np.ascontiguousarray(actions.numpy()[:, :self.n_snakes])
        obs, rew, done, ns, _, _ = (np.array(x) for x in self.ora.step(act))
        obs[0, 1, 1, 0] ^= self._is("obs")
        rew[1] += self._is("reward")
        done[2] ^= self._is("done")
        ns[3] += self._is("num_snakes")
        info = np.zeros((self.num_envs, 4), np.int32)
        info[:, 2] = ns
        self.t += 1
        return tuple(torch.from_numpy(x) for x in (obs, rew, done, info))

    def stats(self):
        return {"errors": int(self.fault == "errors")}


def _buffers(env, stride=None):
    return gh.GuardedOutputs(env.device, dict(gh.action_spec(env, stride), **gh.count_spec(env, "space")))


def _call(env, buf, snakes):
    out, safe, _ = env.scripted_actions_device("safe_greedy", snakes=snakes, out=buf.act, safe_out=buf.safe, space_out=buf.space)
    return out, safe, buf.host("space")


def _loop(fault=None, control=False):
    kw = dict(control=(np.random.default_rng(11), (1,)), stride=4) if control else {}
    seen = []
    gh.closed_loop(CFG, StubEnv(fault), _call, _expected, STEPS, obs_every=5, buffers=_buffers,
                   observe=lambda t, states, wants, o_done, o_el: seen.append((t, len(states), len(wants), o_done.shape, o_el.shape)), **kw)
    return seen


@pytest.mark.parametrize("control", [False, True])
def test_closed_loop_passes_on_an_honest_stub(control):
    seen = _loop(control=control)
    assert seen == [(t, 4, 3, (4,), (4,)) for t in range(STEPS)]


@pytest.mark.parametrize("fault", ["action", "mask", "extra", "surplus", "reward", "done", "num_snakes", "obs", "guard", "errors"])
def test_closed_loop_fails_on_one_wrong_value(fault):
    """Each fault is one value at step AT (a step whose observation is compared); the surplus column exists only under
    mixed control with a wider stride."""
    assert AT % 5 == 0 and AT < STEPS
    with pytest.raises(AssertionError):
        _loop(fault, control=fault == "surplus")


# ------------------------------------------------------------------------------------------ 3. install
class _WordStore:
    """set_state_words / get_state_words of a handle; `spoil` changes the words on their way out."""

    def __init__(self, spoil=None):
        self.words, self.spoil = {}, spoil

    def reset(self):
        pass

    def set_state_words(self, e, words):
        self.words[e] = np.array(words)

    def get_state_words(self, e):
        return self.spoil(self.words[e].copy()) if self.spoil else self.words[e]


def _spoil(word):
    def spoil(w):
        w[word] += 1
        return w
    return spoil


def test_install_round_trip_check(monkeypatch):
    cfg = dict(rules=0, dim=6, n_snakes=2, n_fruits=2)
    states = bs.tie_states(6)[:5]
    fruit0, snake0 = 8, 8 + 2 * 2      # canonical words: 8 scalars, the fruits, then per snake len, v0, v1, grow_to, alive, in_dead, cells
    store = _WordStore()
    monkeypatch.setattr(gh, "make_env", lambda cfg, **kw: store)
    assert gh.install(cfg, states) is store and sorted(store.words) == [0, 1, 2, 3, 4]
    for word in (fruit0, snake0 + 1, snake0 + 2, snake0 + 6):               # a fruit, both velocity words, the head's cell
        monkeypatch.setattr(gh, "make_env", lambda cfg, **kw: _WordStore(_spoil(word)))
        with pytest.raises(AssertionError):
            gh.install(cfg, states)
    # ... and only in the envs it reads back: the first, the middle and the last
    for e, caught in ((0, True), (1, False), (2, True), (3, False), (4, True)):
        only = _WordStore()
        only.get_state_words = lambda i, e=e, only=only: _spoil(fruit0)(only.words[i].copy()) if i == e else only.words[i]
        monkeypatch.setattr(gh, "make_env", lambda cfg, **kw: only)
        if caught:
            with pytest.raises(AssertionError):
                gh.install(cfg, states)
        else:
            gh.install(cfg, states)
