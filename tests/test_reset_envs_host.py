"""CPU-side checks of the masked reset (msnake_reset_envs, MultiSnakeVecEnv.reset_device(mask=...)): the C entry point
refuses a NULL handle before it touches the GPU, the Python mask normalisation, and the register budget of the masked
reset / render kernels.  No GPU: hipcc cross-compiles to assembly, nothing runs."""
import re

import numpy as np
import pytest

import msnake
from kernel_resources import unit_resources


def test_reset_envs_null_handle_is_refused():
    lib = msnake._capi.load()
    assert "msnake_reset_envs" in msnake._capi.SYMBOLS
    assert lib.msnake_reset_envs(None, None, None, None, None, None) == -3  # MSNAKE_E_HANDLE
    assert b"handle" in lib.msnake_last_error()


def test_mask_from_indices():
    assert msnake.normalize_mask([0, 3], 5).tolist() == [1, 0, 0, 1, 0]
    assert msnake.normalize_mask(np.array([4, 4, 1]), 5).tolist() == [0, 1, 0, 0, 1]
    assert msnake.normalize_mask(range(2), 3).tolist() == [1, 1, 0]
    assert msnake.normalize_mask([], 3).tolist() == [0, 0, 0]
    assert msnake.normalize_mask([2], 3).dtype == np.uint8


def test_mask_from_bool_array():
    m = msnake.normalize_mask(np.array([True, False, True]), 3)
    assert m.dtype == np.uint8 and m.tolist() == [1, 0, 1]
    assert msnake.normalize_mask(np.zeros(4, bool), 4).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("bad", [np.ones(4, bool), np.ones(6, bool), np.ones((5, 1), bool), [5], [-1], [[0, 1]], [0.5]])
def test_mask_rejects_wrong_shapes_and_indices(bad):
    with pytest.raises(ValueError):
        msnake.normalize_mask(bad, 5)


def test_lazy_infos_carry_terminal_observation_and_truncation():
    done = np.array([False, True, False, True])
    final = np.arange(2 * 3, dtype=np.uint8).reshape(2, 3)  # rows of the done envs, in env order
    trunc = np.array([0, 1, 0, 0], np.uint8)
    infos = msnake.LazyInfos(done, np.array([3, 1, 2, 0]), np.zeros(4, np.float32), np.zeros(4, np.int32), 0.5, (final, trunc))
    assert "terminal_observation" not in infos[0] and "TimeLimit.truncated" not in infos[2]
    assert infos[1]["TimeLimit.truncated"] is True and infos[3]["TimeLimit.truncated"] is False
    assert infos[1]["terminal_observation"].tolist() == [0, 1, 2]
    assert infos[3]["terminal_observation"].tolist() == [3, 4, 5]


def test_masked_reset_and_render_kernels_do_not_spill():
    """Every MODE 1 (reset) and MODE 2 (render) instantiation of all three rule sets -- the kernels msnake_reset_envs
    launches with its mask -- spills no register and uses no scratch (msnake_step_kernel<RULES, NS, MODE, K>)."""
    res, _ = unit_resources("msnake_kernels")  # the step unit holds every msnake_step_kernel instantiation
    seen = set()
    for name, rr in res.items():
        m = re.match(r"_ZN6msnake18msnake_step_kernelILi(\d)ELi(\d)ELi([12])ELi(\d)E", name)
        if not m:
            continue
        seen.add(m.groups())
        assert rr["SGPRs Spill"] == 0 and rr["VGPRs Spill"] == 0 and rr["ScratchSize [bytes/lane]"] == 0, (m.groups(), rr)
    # snake_env / adversarial: 1-3 snakes, new_world: 1-4; x obs_scale 1 / 4 / 7; x MODE 1 / 2
    assert {g[0] for g in seen} == {"0", "1", "2"} and len(seen) == (3 + 3 + 4) * 3 * 2, sorted(seen)
