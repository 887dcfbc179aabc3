"""CPU-side checks of the compile-time-shape step kernels (msnake_step_kernel<RULES, NS, MODE, K, DIM>): which
configurations msnake_create puts on them.  The decision is made on the host, so it is asked of the library's own
glue (msnake_kernel_name_for_config: the argument checks, the derived shape and the selection of msnake_create,
without a handle) -- no GPU.  MSNAKE_GENERIC_KERNELS is read by the Python binding when a handle is created (the
library itself reads no environment) and handed to the library as msnake_set_generic_kernels."""
import ctypes

import pytest

import msnake

GENERIC = "msnake_step_kernel<%d, %d, 0, %d>"
SPEC = "msnake_step_kernel<0, %d, 0, 1, %d>"


def _name(num_envs=4096, dim=19, n_snakes=3, rules="snake_env", auto_reset=True, obs_scale=1, record_policy="auto",
          n_fruits=None, max_steps=2000, struct_size=None):
    C = msnake._capi
    cfg = C.MsnakeConfig(struct_size or ctypes.sizeof(C.MsnakeConfig), 0, num_envs, dim, n_snakes,
                         n_snakes if n_fruits is None else n_fruits, C.RULES[rules], max_steps, int(auto_reset), obs_scale, 0, 0,
                         0, C.RECORD_POLICY[record_policy], 0, 0)
    return C.kernel_name_for_config(cfg)


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("MSNAKE_GENERIC_KERNELS", raising=False)


@pytest.mark.parametrize("dim,ns", [(19, 3), (19, 2), (10, 1)])
def test_exact_matches_select_the_compiled_shape(dim, ns):
    assert _name(dim=dim, n_snakes=ns) == SPEC % (ns, dim)
    # fields the kernels do not fold leave the choice alone: batch size (below the short-record threshold), step cap,
    # an explicit full record, an ABI-2 caller's 56-byte configuration
    assert _name(dim=dim, n_snakes=ns, num_envs=192, max_steps=60000, record_policy="full") == SPEC % (ns, dim)
    assert _name(dim=dim, n_snakes=ns, struct_size=msnake._capi.CONFIG_SIZE_V2) == SPEC % (ns, dim)
    # ... and a large batch with the full record asked for
    assert _name(dim=dim, n_snakes=ns, num_envs=16384, record_policy="full") == SPEC % (ns, dim)


@pytest.mark.parametrize("kw,generic", [
    (dict(dim=18), (0, 3, 1)), (dict(dim=20), (0, 3, 1)),
    (dict(rules="new_world"), (1, 3, 1)), (dict(rules="adversarial"), (2, 3, 1)),
    (dict(auto_reset=False), (0, 3, 1)),
    (dict(record_policy="short"), (0, 3, 1)),
    (dict(num_envs=16384), (0, 3, 1)),            # auto record policy: short above 8 192 envs
    (dict(obs_scale=4), (0, 3, 4)),
    (dict(rules="new_world", n_snakes=4), (1, 4, 1)),
    (dict(dim=19, n_snakes=1), (0, 1, 1)), (dict(dim=10, n_snakes=2), (0, 2, 1)), (dict(dim=10, n_snakes=3), (0, 3, 1)),
    (dict(dim=9, n_snakes=1), (0, 1, 1)), (dict(dim=11, n_snakes=1), (0, 1, 1)),
    (dict(rules="new_world", n_fruits=5), (1, 3, 1)),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_near_misses_select_the_generic_kernel(kw, generic):
    assert _name(**kw) == GENERIC % generic


@pytest.mark.parametrize("dim,ns", [(19, 3), (19, 2), (10, 1)])
def test_the_environment_switch_forces_the_generic_kernels(monkeypatch, dim, ns):
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "1")
    assert _name(dim=dim, n_snakes=ns) == GENERIC % (0, ns, 1)
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "0")  # "0" and the empty string mean "not set"
    assert _name(dim=dim, n_snakes=ns) == SPEC % (ns, dim)
    monkeypatch.setenv("MSNAKE_GENERIC_KERNELS", "")
    assert _name(dim=dim, n_snakes=ns) == SPEC % (ns, dim)


def test_the_switch_is_a_library_call_and_returns_the_previous_setting():
    lib = msnake._capi.load()
    lib.msnake_set_generic_kernels(0)
    assert lib.msnake_set_generic_kernels(1) == 0 and lib.msnake_set_generic_kernels(5) == 1
    assert lib.msnake_set_generic_kernels(0) == 1
    assert _name() == SPEC % (3, 19)


def test_a_refused_configuration_is_refused_here_too():
    C = msnake._capi
    lib = C.load()
    buf = ctypes.create_string_buffer(64)
    cfg = C.MsnakeConfig(ctypes.sizeof(C.MsnakeConfig), 0, 4, 19, 4, 4, 0, 2000, 1, 1, 0, 0)  # snake_env has at most 3 snakes
    assert lib.msnake_kernel_name_for_config(ctypes.byref(cfg), buf, len(buf)) == -1
    assert b"n_snakes" in lib.msnake_last_error()
    assert lib.msnake_kernel_name_for_config(None, buf, len(buf)) == -1
    assert lib.msnake_kernel_name_for_config(ctypes.byref(cfg), None, 0) == -1
