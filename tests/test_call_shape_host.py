"""CPU-side checks of the per-call choice among a compiled shape's two per-step kernels (msnake_step_kernel<RULES, NS,
0, 1, DIM, PLAIN>): the plain-call variant for a call that gives every output, an observation base on a 128-byte line
and fewer than 2^31 observation bytes, the shape's first variant for any other call, the generic kernel where the
handle or the call has no compiled shape.  The choice is made on the host, per launch; it is asked of the library's own
glue (msnake_call_shape_for_config) -- no GPU, the addresses are plain numbers."""
import ctypes

import pytest

import msnake

SHAPES = [(19, 3), (19, 2), (10, 1)]
BASE = 0x7F0000000000  # a 128-byte-aligned "device address"; nothing is dereferenced
REW, DONE, INFO = 0x7F1000000000, 0x7F2000000000, 0x7F3000000000


def _cfg(num_envs=4096, dim=19, n_snakes=3, rules="snake_env", auto_reset=True, obs_scale=1, record_policy="auto"):
    C = msnake._capi
    return C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, num_envs, dim, n_snakes, n_snakes, C.RULES[rules], 2000,
                          int(auto_reset), obs_scale, 0, 0, 0, C.RECORD_POLICY[record_policy], 0, 0)


def _shape(cfg=None, stride=None, obs=BASE, rew=REW, done=DONE, info=INFO, **kw):
    cfg = cfg or _cfg(**kw)
    return msnake._capi.call_shape_for_config(cfg, stride or cfg.n_snakes, obs, rew, done, info)


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("MSNAKE_GENERIC_KERNELS", raising=False)


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_an_aligned_complete_call_is_a_plain_call(dim, ns):
    assert _shape(dim=dim, n_snakes=ns) == "plain"
    assert _shape(dim=dim, n_snakes=ns, num_envs=160) == "plain"
    for k in (1, 2, 7, 4097):  # any 128-byte line
        assert _shape(dim=dim, n_snakes=ns, obs=BASE + 128 * k) == "plain"
    # the other outputs only have to be there (msnake_step checks their own alignment)
    assert _shape(dim=dim, n_snakes=ns, rew=REW + 4, done=DONE + 1, info=INFO + 16) == "plain"


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_an_absent_output_or_an_unaligned_base_keeps_the_first_variant(dim, ns):
    assert _shape(dim=dim, n_snakes=ns, obs=0) == "shape"
    assert _shape(dim=dim, n_snakes=ns, info=0) == "shape"
    assert _shape(dim=dim, n_snakes=ns, rew=0) == "shape"   # (msnake_step refuses these two; the choice does not rely on it)
    assert _shape(dim=dim, n_snakes=ns, done=0) == "shape"
    for off in (1, 16, 64, 15, 127):
        assert _shape(dim=dim, n_snakes=ns, obs=BASE + off) == "shape", off


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_observation_offsets_must_fit_31_bits(dim, ns):
    S = (dim + 2) * (dim + 2) * 9
    most = (2 ** 31 - 1) // S  # the largest batch with num_envs * S < 2^31
    # (batches above 8 192 envs take the short record by default, which has no compiled shape: ask for the full one)
    assert _shape(dim=dim, n_snakes=ns, num_envs=most, record_policy="full") == "plain"
    assert _shape(dim=dim, n_snakes=ns, num_envs=most + 1, record_policy="full") == "shape"
    assert (most + 1) * S >= 2 ** 31 > most * S


@pytest.mark.parametrize("dim,ns", SHAPES)
def test_no_compiled_shape_means_the_generic_kernel(monkeypatch, dim, ns):
    assert _shape(dim=dim, n_snakes=ns, stride=ns + 1) == "generic"  # a padded action_stride: per call
    assert _shape(dim=dim, n_snakes=ns, stride=7) == "generic"
    assert _shape(dim=dim, n_snakes=ns, stride=ns + 1, obs=BASE + 1) == "generic"
    lib = msnake._capi.load()
    assert lib.msnake_set_generic_kernels(1) == 0
    try:  # (the binding re-applies the environment switch per query: ask the library directly)
        out = ctypes.c_int32(-1)
        cfg = _cfg(dim=dim, n_snakes=ns)
        assert lib.msnake_call_shape_for_config(ctypes.byref(cfg), ns, BASE, REW, DONE, INFO, ctypes.byref(out)) == 0
        assert out.value == 0
    finally:
        lib.msnake_set_generic_kernels(0)
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "1")
    assert _shape(dim=dim, n_snakes=ns) == "generic"
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "0")
    assert _shape(dim=dim, n_snakes=ns) == "plain"


@pytest.mark.parametrize("kw", [dict(dim=18), dict(rules="new_world"), dict(rules="adversarial"), dict(auto_reset=False),
                                dict(record_policy="short"), dict(num_envs=16384), dict(obs_scale=4), dict(dim=10, n_snakes=2)],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()))
def test_configurations_without_a_compiled_shape_are_generic_whatever_the_call(kw):
    assert _shape(**kw) == "generic"


def test_kernel_names_are_what_they_were():
    C = msnake._capi
    for dim, ns in SHAPES:
        assert C.kernel_name_for_config(_cfg(dim=dim, n_snakes=ns)) == f"msnake_step_kernel<0, {ns}, 0, 1, {dim}>"
    assert C.kernel_name_for_config(_cfg(dim=18)) == "msnake_step_kernel<0, 3, 0, 1>"
    assert C.kernel_name_for_config(_cfg(rules="new_world")) == "msnake_step_kernel<1, 3, 0, 1>"
    assert C.kernel_name_for_config(_cfg(obs_scale=4)) == "msnake_step_kernel<0, 3, 0, 4>"


def test_refusals():
    C = msnake._capi
    lib = C.load()
    out = ctypes.c_int32(-1)
    cfg = _cfg()
    assert lib.msnake_call_shape_for_config(None, 3, BASE, REW, DONE, INFO, ctypes.byref(out)) == -1
    assert lib.msnake_call_shape_for_config(ctypes.byref(cfg), 3, BASE, REW, DONE, INFO, None) == -1
    assert lib.msnake_call_shape_for_config(ctypes.byref(cfg), 2, BASE, REW, DONE, INFO, ctypes.byref(out)) == -1
    assert b"action_stride" in lib.msnake_last_error()
    assert lib.msnake_call_shape_for_config(ctypes.byref(cfg), 8, BASE, REW, DONE, INFO, ctypes.byref(out)) == -1
    bad = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, 4, 19, 4, 4, 0, 2000, 1, 1, 0, 0)  # snake_env has at most 3 snakes
    assert lib.msnake_call_shape_for_config(ctypes.byref(bad), 4, BASE, REW, DONE, INFO, ctypes.byref(out)) == -1
    assert out.value == -1
    assert "msnake_call_shape_for_config" in C.SYMBOLS
