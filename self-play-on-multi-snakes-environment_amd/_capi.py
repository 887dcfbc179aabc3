"""ctypes binding of include/msnake.h (libmsnake.so: HIP kernels + C-ABI, gfx950).

There is deliberately no fallback: if the shared library has not been built, or no MI355X is
visible, the env cannot be created and says so.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSNAKE_LIB: another build of the same library (kernel A/B runs on one box); never a different backend
LIB_PATH = os.environ.get("MSNAKE_LIB") or os.path.join(_HERE, "libmsnake.so")

RULES = {"snake_env": 0, "new_world": 1, "adversarial": 2}
RULE_NAMES = {v: k for k, v in RULES.items()}

class MsnakeConfig(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("device", ctypes.c_int32), ("num_envs", ctypes.c_int32),
                ("dim", ctypes.c_int32), ("n_snakes", ctypes.c_int32), ("n_fruits", ctypes.c_int32),
                ("rules", ctypes.c_int32), ("max_steps", ctypes.c_int32), ("auto_reset", ctypes.c_int32),
                ("obs_scale", ctypes.c_int32), ("seed", ctypes.c_uint64), ("env_id_base", ctypes.c_uint64),
                # ABI 3: launch tuning, 0 = the library decides
                ("envs_per_block", ctypes.c_int32), ("record_policy", ctypes.c_int32),
                ("obs_store_policy", ctypes.c_int32), ("tape_store_policy", ctypes.c_int32)]


ABI_VERSION = 3
CONFIG_SIZE_V2 = 56
RECORD_POLICY = {"auto": 0, "full": 1, "short": 2}
STORE_POLICY = {"auto": 0, "plain": 1, "stream": 2}
SCRIPTED_POLICY = {None: 0, "safe_greedy": 1, "hamiltonian": 2}  # MSNAKE_POLICY_*
SPACE_POLICY = "space_greedy"  # no policy id: an entry point of its own (msnake_space_actions)
TERRITORY_POLICY = "territory_greedy"  # likewise (msnake_territory_actions)
PATH_POLICY = "path_greedy"  # likewise (msnake_path_actions)
SCRIPTED_POLICY_NAMES = ("safe_greedy", "hamiltonian", SPACE_POLICY, TERRITORY_POLICY)  # the opponents selfplay.SCRIPTED_POLICIES names
TIMED_POLICY = "timed_greedy"  # likewise (msnake_timed_actions)
SCRIPTED_OPPONENT_NAMES = SCRIPTED_POLICY_NAMES + (PATH_POLICY,)  # the scripted opponents with static bodies
SCRIPTED_PLAYER_NAMES = SCRIPTED_OPPONENT_NAMES + (TIMED_POLICY,)  # every scripted opponent there is
WARY_POLICY = "wary_greedy"  # likewise (msnake_fate_actions)
SCRIPTED_NAMES = SCRIPTED_PLAYER_NAMES + (WARY_POLICY,)  # ... and the one that plays by the fates of its moves
# MSNAKE_POLICY_* as msnake_playout takes them: the scripted ids and wary_greedy (msnake_scripted_actions keeps refusing 3)
PLAYOUT_POLICY = {None: 0, "safe_greedy": 1, "hamiltonian": 2, "wary_greedy": 3}
EXPLORE_ONE = 65536  # eps_q16 of probability 1: msnake_explore_actions and msnake_playout_explore take round(p * 65536)
PLAYOUT_MAX_STEPS = 4096  # MSNAKE_PLAYOUT_MAX_STEPS
PLAYOUT_HORIZON, PLAYOUT_DEAD, PLAYOUT_CAP, PLAYOUT_FINISHED = 0, 1, 2, 3  # MSNAKE_PLAYOUT_*: msnake_playout's end codes
MAX_SNAKES = 4  # MSNAKE_MAX_SNAKES
# MSNAKE_FATE_*: the bits of msnake_fate_actions' fate output, and the two groups its masks are made of
FATE_WALL, FATE_SELF, FATE_BODY, FATE_HEAD_ON, FATE_TAIL, FATE_EATS = 1, 2, 4, 8, 16, 32
FATE_CERTAIN, FATE_RISK = FATE_WALL | FATE_SELF | FATE_BODY, FATE_HEAD_ON | FATE_TAIL
HEAD_NONE, OWNER_TIE, OWNER_NONE = 0xFFFF, 0xFE, 0xFF  # MSNAKE_HEAD_NONE, MSNAKE_OWNER_TIE, MSNAKE_OWNER_NONE: msnake_head_fields
AGENT_ARM = 1  # MSNAKE_AGENT_ARM: msnake_agent_outcomes writes the tracker from the state
AGENT_ALIVE, AGENT_WAS_ALIVE, AGENT_DIED, AGENT_ENDED = 1, 2, 4, 8  # MSNAKE_AGENT_*: the bits of its flags output
CAUSE_WALL, CAUSE_SELF, CAUSE_HEAD_ON, CAUSE_BODY = 1, 2, 4, 8  # MSNAKE_CAUSE_*: the bits of msnake_death_causes' cause output
HASH_WHAT = {"full": 0, "board": 1}  # MSNAKE_HASH_FULL, MSNAKE_HASH_BOARD: msnake_hash_states
# MSNAKE_STATE_*: the status bytes of msnake_import_states
STATE_OK, STATE_TOO_SHORT, STATE_SNAKE_COUNT, STATE_FRUIT_COUNT, STATE_CELL, STATE_LENGTH, STATE_SCALAR, STATE_SKIPPED = 0, 1, 2, 3, 4, 5, 6, 0xFF
GEN_COMPACT = 1  # MSNAKE_GEN_COMPACT: msnake_generate_states grows bodies by Warnsdorff's rule
# the words of a tracker row: grow_to, alive, then the totals of the env's current episode
AGENT_TRACK_WORDS = ("grow_to", "alive", "ep_fruit", "ep_alive_steps", "first_death", "ep_steps", "ep_return", "zero")


class MsnakeBlobInfo(ctypes.Structure):
    _fields_ = [("version", ctypes.c_int32), ("num_envs", ctypes.c_int32), ("dim", ctypes.c_int32),
                ("n_snakes", ctypes.c_int32), ("n_fruits", ctypes.c_int32), ("rules", ctypes.c_int32),
                ("total_words", ctypes.c_int64)]


class MsnakeStats(ctypes.Structure):
    _fields_ = [("episodes", ctypes.c_int64), ("ep_len_sum", ctypes.c_int64), ("ep_return_sum", ctypes.c_int64),
                ("env_steps", ctypes.c_int64), ("errors", ctypes.c_int64), ("reserved", ctypes.c_int64 * 3)]


_vp, _i32, _u32, _size = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_size_t
_int, _cfg = ctypes.c_int, ctypes.POINTER(MsnakeConfig)
# h, actions_dev, action_stride, n_steps, obs_dev, obs_step_stride, rew_dev, done_dev, info_dev, scalar_step_stride, stream
_TAPE = [_vp, _vp, _i32, _i32, _vp, _size, _vp, _vp, _vp, _size, _vp]
# every extern "C" symbol include/msnake.h declares (tests check the .so exports all of them): name -> (restype, argtypes)
PROTOTYPES = {
    "msnake_abi_version": (_int, None),
    "msnake_last_error": (ctypes.c_char_p, None),
    "msnake_create": (_int, [_cfg, ctypes.POINTER(_vp)]),
    "msnake_destroy": (_int, [_vp]),
    "msnake_obs_shape": (_int, [_vp] + [ctypes.POINTER(_i32)] * 3),  # h, H, W, C
    "msnake_reset": (_int, [_vp, _vp, _vp]),  # h, obs_dev, stream
    "msnake_reset_envs": (_int, [_vp, _vp, _vp, _vp, _vp, _vp]),  # h, mask_dev, obs_dev, final_obs_dev, truncated_dev, stream
    # h, actions_dev, action_stride, obs_dev, rew_dev, done_dev, info_dev, stream
    "msnake_step": (_int, [_vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "msnake_step_tape": (_int, _TAPE),
    "msnake_rollout_tape": (_int, _TAPE),
    "msnake_get_state": (_int, [_vp, _i32, _vp, _i32]),  # h, env, words, cap_words
    "msnake_set_state": (_int, [_vp, _i32, _vp, _i32]),  # h, env, words, n
    "msnake_get_state_all": (ctypes.c_int64, [_vp, _vp, _size]),  # h, buf, cap_bytes
    "msnake_set_state_all": (_int, [_vp, _vp, _size]),  # h, buf, bytes
    "msnake_state_blob_info": (_int, [_vp, _size, ctypes.POINTER(MsnakeBlobInfo)]),  # buf, bytes, out
    "msnake_render": (_int, [_vp, _vp, _vp]),  # h, obs_dev, stream
    "msnake_get_stats": (_int, [_vp, ctypes.POINTER(MsnakeStats), _i32]),  # h, out, reset
    "msnake_kernel_name": (ctypes.c_char_p, [_vp]),
    "msnake_algorithmic_bytes_per_env_step": (ctypes.c_int64, [_vp]),
    # h, policy, snake_mask, actions_dev, action_stride, safe_dev, stream
    "msnake_scripted_actions": (_int, [_vp, _i32, _u32, _vp, _i32, _vp, _vp]),
    "msnake_copy_envs": (_int, [_vp, _vp, _vp, _vp]),  # dst, src, src_index_dev (int32 [dst.num_envs] or NULL), stream
    "msnake_kernel_name_for_config": (_int, [_cfg, ctypes.c_char_p, _size]),  # cfg, out, n
    "msnake_set_generic_kernels": (_int, [_i32]),
    # h, snake_mask, actions_dev, action_stride, safe_dev, space_dev (uint16 [num_envs][n_snakes][4]), stream
    "msnake_space_actions": (_int, [_vp, _u32, _vp, _i32, _vp, _vp, _vp]),
    # h, view_mask, cells_dev (uint8 [num_envs][V][dim][dim]), snakes_dev (int32 [num_envs][n_snakes][8] or NULL), stream
    "msnake_render_cells": (_int, [_vp, _u32, _vp, _vp, _vp]),
    # h, radius, snake_mask, oriented, windows_dev (uint8 [num_envs][S][W][W]), heading_dev (uint8 [num_envs][S] or NULL), stream
    "msnake_render_local": (_int, [_vp, _i32, _u32, _i32, _vp, _vp, _vp]),
    # cfg, action_stride, obs / rew / done / info (addresses, only looked at), out
    "msnake_call_shape_for_config": (_int, [_cfg, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(_i32)]),
    # h, snake_mask, actions_dev, action_stride, safe_dev, territory_dev (uint16 [num_envs][n_snakes][4]), stream
    "msnake_territory_actions": (_int, [_vp, _u32, _vp, _i32, _vp, _vp, _vp]),
    # h, snake_mask, oriented, rays_dev (uint8 [num_envs][S][8][4], 4-byte aligned), heading_dev (uint8 [num_envs][S] or NULL), stream
    "msnake_render_rays": (_int, [_vp, _u32, _i32, _vp, _vp, _vp]),
    # h, snake_mask, actions_dev, action_stride, safe_dev, path_dev (uint16 [num_envs][n_snakes][4]),
    # field_dev (uint16 [num_envs][dim][dim]), stream
    "msnake_path_actions": (_int, [_vp, _u32, _vp, _i32, _vp, _vp, _vp, _vp]),
    # h, snake_mask, actions_dev, action_stride, safe_dev, reach_dev (uint16 [num_envs][n_snakes][4]),
    # life_dev (uint16 [num_envs][dim][dim]), stream
    "msnake_timed_actions": (_int, [_vp, _u32, _vp, _i32, _vp, _vp, _vp, _vp]),
    # h, flags (AGENT_ARM or 0), track_dev (int32 [num_envs][n_snakes][8]), done_dev (uint8 [num_envs]), rew_dev (float32
    # [num_envs][n_snakes]), ate_dev, flags_dev (uint8 [num_envs][n_snakes]), info_dev (int32 [num_envs][n_snakes][4]), stream
    "msnake_agent_outcomes": (_int, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # h, snake_mask, dist_dev (uint16 [num_envs][P][dim][dim]), owner_dev (uint8 [num_envs][dim][dim]),
    # counts_dev (uint16 [num_envs][n_snakes]), stream
    "msnake_head_fields": (_int, [_vp, _u32, _vp, _vp, _vp, _vp]),
    # after, before, cause_dev, by_dev, victims_dev (uint8 [num_envs][n_snakes]), where_dev (int8 [num_envs][n_snakes][2]), stream
    "msnake_death_causes": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # h, snake_mask, actions_dev, action_stride, fate_dev, by_dev, eat_dev (uint8 [num_envs][n_snakes][5]),
    # mask_dev (uint8 [num_envs][n_snakes][2]), stream
    "msnake_fate_actions": (_int, [_vp, _u32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    # h, policies (int32 [MSNAKE_MAX_SNAKES], host), n_steps, first_dev (int32 [num_envs][first_stride] or NULL), first_stride,
    # first_mask, steps_dev (int32 [num_envs]), end_dev (uint8 [num_envs]), ret_dev (float32 [num_envs][n_snakes]),
    # info_dev (int32 [num_envs][n_snakes][4]), words_dev (int32 [num_envs][words_stride]), words_stride, count_dev, stream
    "msnake_playout": (_int, [_vp, ctypes.POINTER(_i32), _i32, _vp, _i32, _u32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp]),
    # h, policies (int32 [MSNAKE_MAX_SNAKES], host), eps_q16 (uint32 [MSNAKE_MAX_SNAKES], host), salt, snake_mask, actions_dev,
    # action_stride, explored_dev (uint8 [num_envs][n_snakes] or NULL), stream
    "msnake_explore_actions": (_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_u32), ctypes.c_uint64, _u32, _vp, _i32, _vp, _vp]),
    # h, policies, eps_q16, salt, then msnake_playout's arguments from n_steps on
    "msnake_playout_explore": (_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_u32), ctypes.c_uint64, _i32, _vp, _i32, _u32, _vp, _vp,
                                      _vp, _vp, _vp, _i32, _vp, _vp]),
    "msnake_state_words_max": (_i32, [_vp]),  # h
    # h, words_dev (int32 [num_envs][stride] or NULL), stride, count_dev (int32 [num_envs] or NULL), stream
    "msnake_export_states": (_int, [_vp, _vp, _i32, _vp, _vp]),
    # h, mask_dev (uint8 [num_envs] or NULL), words_dev, stride, count_dev (or NULL), status_dev (uint8 [num_envs]), stream
    "msnake_import_states": (_int, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "msnake_hash_states": (_int, [_vp, _u32, _vp, _vp]),  # h, what (HASH_WHAT), hash_dev (uint64 [num_envs]), stream
    # h, mask_dev (uint8 [num_envs] or NULL), len_dev (int32 [num_envs][len_stride]), len_stride, flags (GEN_COMPACT or 0), salt,
    # words_dev (int32 [num_envs][stride] or NULL), stride, count_dev (int32 [num_envs] or NULL), got_dev (int32 [num_envs][n_snakes] or NULL), stream
    "msnake_generate_states": (_int, [_vp, _vp, _vp, _i32, _u32, ctypes.c_uint64, _vp, _i32, _vp, _vp, _vp]),
    "msnake_launch_shape_for_config": (_int, [_cfg, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),  # cfg, step_epb, tape_epb
}
SYMBOLS = list(PROTOTYPES)

_lib = None


def load(optional=()):
    """Load libmsnake.so, declare prototypes. Raises RuntimeError if it was never built.  `optional`: entry points that the
    library named by MSNAKE_LIB may lack (an older build in a same-box A/B run, tools/playout_cost.py); they are left unbound,
    and calling one fails.  Every other symbol must be there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.basename(LIB_PATH).startswith("libmsnake"):
        raise RuntimeError(f"MSNAKE_LIB={LIB_PATH}: only another build of libmsnake*.so may be named (kernel A/B runs)")
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C <pkg>/csrc). "
            "There is no CPU fallback.")
    # torch first: its wheel bundles a HIP runtime with the SONAME libmsnake.so links against
    # (libamdhip64.so.7), and the device pointers / streams handed to the library come from it.
    # Loading libmsnake.so before torch would pull /opt/rocm's copy in as a SECOND runtime in the
    # process, and that one finds no device (msnake_create -> MSNAKE_E_NOGPU).
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if name in optional and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def apply_kernel_switch():
    """MSNAKE_GENERIC_KERNELS=1 in the environment (anything but empty or "0") at the time a handle is created keeps that
    handle on the generic step kernels instead of the ones compiled for its shape: same-box A/B runs and tests.  Called
    right before msnake_create / msnake_kernel_name_for_config; the library itself reads no environment variable."""
    load().msnake_set_generic_kernels(int(os.environ.get("MSNAKE_GENERIC_KERNELS", "") not in ("", "0")))


def kernel_name_for_config(cfg):
    """The step kernel a handle created from `cfg` (a MsnakeConfig) right now would report, decided by the library's
    host glue without a GPU."""
    apply_kernel_switch()
    buf = ctypes.create_string_buffer(64)
    check(load().msnake_kernel_name_for_config(ctypes.byref(cfg), buf, len(buf)), "msnake_kernel_name_for_config")
    return buf.value.decode()


CALL_SHAPE = {0: "generic", 1: "shape", 2: "plain"}  # MSNAKE_CALL_*


def call_shape_for_config(cfg, action_stride, obs, rew, done, info):
    """Which per-step kernel one msnake_step call with these device addresses (integers, 0 / None = absent) gets on a handle
    created from `cfg` right now: "generic", "shape" (the kernel compiled for the shape) or "plain" (its plain-call
    variant).  Decided by the library's host glue without a GPU."""
    apply_kernel_switch()
    out = ctypes.c_int32(-1)
    check(load().msnake_call_shape_for_config(ctypes.byref(cfg), action_stride, obs or None, rew or None, done or None,
                                              info or None, ctypes.byref(out)), "msnake_call_shape_for_config")
    return CALL_SHAPE[out.value]


def launch_shape_for_config(cfg):
    """(envs per workgroup of msnake_step's launches, envs per workgroup of msnake_rollout_tape's persistent launch) of a
    handle created from `cfg` (a MsnakeConfig); the second is 0 where the persistent kernel's two LDS images do not fit
    and the call runs per-step launches.  Decided by the library's host glue without a GPU."""
    step, tape = ctypes.c_int32(-1), ctypes.c_int32(-1)
    check(load().msnake_launch_shape_for_config(ctypes.byref(cfg), ctypes.byref(step), ctypes.byref(tape)),
          "msnake_launch_shape_for_config")
    return step.value, tape.value


def check(rc, what="msnake call"):
    """Mirror of the reference's error behaviour: failures surface as Python exceptions."""
    if rc < 0:
        msg = load().msnake_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")
    return rc
