"""CPU-side checks of the device-side env copy (msnake_copy_envs, MultiSnakeVecEnv.copy_envs_device / clone): the
index normalisation and its errors, the entry point is declared, exported, bound with the declared signature and
refuses a NULL handle before it touches the GPU, and the register budget of the new kernel.  No GPU: hipcc
cross-compiles, nothing runs."""
import ctypes
import os
import re

import numpy as np
import pytest

import msnake
from kernel_resources import unit_resources
from msnake.vec_env import CLONE_OVERRIDES, normalize_copy_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ the index
def test_index_is_normalised_to_contiguous_int32():
    for given in ([3, -1, 0, 3, 7], (3, -1, 0, 3, 7), np.array([3, -1, 0, 3, 7], np.int64), np.array([3, -1, 0, 3, 7], np.int16),
                  np.array([9, 3, 9, -1, 9, 0, 9, 3, 9, 7], np.int32)[1::2]):     # a strided view
        out = normalize_copy_index(given, 5)
        assert out.dtype == np.int32 and out.shape == (5,) and out.flags.c_contiguous
        assert out.tolist() == [3, -1, 0, 3, 7]
    # other negative values mean "untouched" too; values past int32 stay out of range instead of wrapping into it
    out = normalize_copy_index(np.array([-7, 2**40, -2**40, 2**31], np.int64), 4)
    assert out.tolist() == [-1, 2**31 - 1, -1, 2**31 - 1]
    assert normalize_copy_index(np.array([2**32 + 1], np.uint64), 1).tolist() == [2**31 - 1]
    assert msnake.normalize_copy_index is normalize_copy_index


@pytest.mark.parametrize("bad,word", [
    ([0, 1, 2], "shape"), ([0, 1, 2, 3, 4, 5], "shape"), ([], "shape"),                  # wrong length
    (np.zeros((5, 1), np.int32), "shape"), (np.zeros((1, 5), np.int32), "shape"), (3, "shape"),   # 2-D, 0-D
    (np.zeros(5, np.float32), "integer"), ([0.0, 1.0, 2.0, 3.0, 4.0], "integer"), (np.zeros(5, bool), "integer"),
])
def test_index_errors(bad, word):
    with pytest.raises(ValueError, match=word):
        normalize_copy_index(bad, 5)


def test_clone_overrides_are_what_the_header_lets_differ():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    doc = text[text.index("/* Copy env state from"):text.index("int msnake_copy_envs(")]
    m = re.search(r"\(num_envs, ([a-z_, \n*]+?) and ([a-z_]+) may all differ", doc)
    assert m, doc
    named = [w for w in re.split(r"[,\s*]+", m.group(1)) if w] + [m.group(2)]
    assert sorted(named) == sorted(CLONE_OVERRIDES)


# ------------------------------------------------------------------------------------------ the C entry point
def test_header_declares_and_library_exports_the_entry_point():
    text = open(os.path.join(ROOT, "include", "msnake.h")).read()
    assert re.search(r"\bint msnake_copy_envs\(msnake_handle dst, msnake_handle src, const int32_t\* src_index_dev, void\* stream\);",
                     text)
    assert re.search(r"#define MSNAKE_ABI_VERSION 3\b", text)  # additive: the ABI version stays
    assert re.search(r"^ \*   msnake_copy_envs <- no reference counterpart", text, re.M) and "cloneState" in text
    assert "msnake_copy_envs" in msnake._capi.SYMBOLS
    lib = msnake._capi.load()
    assert lib.msnake_abi_version() == 3
    fn = lib.msnake_copy_envs
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == [ctypes.c_void_p] * 4   # dst, src, src_index_dev, stream


def test_null_handles_are_refused():
    lib = msnake._capi.load()
    assert lib.msnake_copy_envs(None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()
    dead = ctypes.create_string_buffer(4)       # what a destroyed handle looks like: the magic word is gone
    assert lib.msnake_copy_envs(dead, None, None, None) == -3 and lib.msnake_copy_envs(None, dead, None, None) == -3
    assert lib.msnake_copy_envs(dead, dead, None, None) == -3  # (the handle check comes before dst == src)


def test_methods_exist_on_the_env_class():
    assert callable(msnake.MultiSnakeVecEnv.copy_envs_device) and callable(msnake.MultiSnakeVecEnv.clone)


# ------------------------------------------------------------------------------------------ register budget
def test_copy_kernel_does_not_spill():
    """msnake_copy_envs_kernel spills no register, uses no scratch and no LDS, and stays within 64 VGPRs (8 waves
    per SIMD)."""
    res, _ = unit_resources("msnake_views")
    mine = [rr for name, rr in res.items() if "msnake_copy_envs_kernel" in name]
    assert len(mine) == 1, sorted(res)
    rr = mine[0]
    assert rr["SGPRs Spill"] == 0 and rr["VGPRs Spill"] == 0 and rr["ScratchSize [bytes/lane]"] == 0, rr
    assert rr["LDS Size [bytes/block]"] == 0 and rr["VGPRs"] <= 64, rr
