/*
 * msnake.h -- C-ABI of the MI355X-native batched multi-snake environment step.
 *
 * One handle owns the state of `num_envs` independent dim x dim multi-snake games in HBM and
 * steps all of them with ONE HIP kernel launch.  No torch types, no C++ types: plain pointers and
 * sizes, so it can be bound from ctypes / cffi / cgo / JNI alike.  All `*_dev` pointers are
 * DEVICE pointers owned by the caller (e.g. torch tensors' data_ptr()); the library never copies
 * observations through the host.  Every function returns 0 on success or a negative MSNAKE_E_*
 * code; msnake_last_error() returns a thread-local description of the last failure.
 *
 * What each entry point replaces in the reference (paths under /root/reference/src/):
 *   msnake_create   <- gym.make + env.__init__ + env.seed(seed+rank) for every SubprocVecEnv worker
 *                      (utils.py:34-49 make_basic_env, baselines/common/vec_env/subproc_vec_env.py:32-50)
 *   msnake_reset    <- SubprocVecEnv.reset (subproc_vec_env.py:63-66) -> SnakeEnv.reset
 *                      (gym-snake/gym_snake/envs/snake_multiple_test.py:219-232) /
 *                      NewMultipleSnakes.reset (envs/snake_multiple_env_new.py:27-33)
 *   msnake_step     <- SubprocVecEnv.step_async/step_wait (subproc_vec_env.py:52-61), the worker's
 *                      auto-reset (:13-16), Monitor.step episode stats (baselines/bench/monitor.py:57-78)
 *                      and SnakeEnv.step (snake_multiple_test.py:166-197) /
 *                      World.move_snakes + NewMultipleSnakes.step (core/new_world.py:88-109,
 *                      envs/snake_multiple_env_new.py:35-50) / SnakeAdversarial.step
 *                      (envs/snake_adversarial_env.py:166-201), including the observation render
 *                      get_multi_snake_ob (snake_multiple_test.py:35-58,93-95)
 *   msnake_reset_envs <- the worker's `ob = env.reset()` on done (subproc_vec_env.py:13-16), for the envs a mask
 *                      selects, plus what that line drops: the terminal observation and whether the time cap
 *                      ended the episode (gymnasium's reset_mask, envpool's reset(env_ids))
 *   msnake_destroy  <- SubprocVecEnv.close (subproc_vec_env.py:73-83)
 *   msnake_get_state / msnake_set_state / msnake_get_state_all / msnake_set_state_all: no reference
 *                      counterpart (env state is never checkpointed there); used by
 *                      the parity tests to install hand-built states and by callers to checkpoint.
 *   msnake_state_blob_info: no reference counterpart either; validates such a checkpoint on the host.
 *   msnake_export_states / msnake_import_states / msnake_hash_states / msnake_state_words_max: no reference
 *                      counterpart either; the same words as a device tensor that torch code can read, edit and archive,
 *                      and a 64-bit key per env (transpositions in a search over forks, archives keyed by position,
 *                      lockstep checks between shards) -- asynchronous and graph-capturable, unlike the four above.
 *   msnake_scripted_actions: no reference counterpart (its opponents are always networks: evaluate_snake.py,
 *                      ppo_multi_agent.py:28-50 MultiModel.multi_step); a fixed, deterministic opponent and the
 *                      safe-move mask, computed on the device from the state the handle already owns.
 *   msnake_space_actions / msnake_territory_actions: no reference counterpart either; opponents that look ahead -- how
 *                      much room a move leads into, and how much of it the snake reaches before any other snake can
 *                      (Voronoi territory) -- with the counts as per-move features.
 *   msnake_path_actions: no reference counterpart either; the BFS distance to the nearest fruit around the bodies, per
 *                      move and as a whole field, and the opponent that forages by it.
 *   msnake_timed_actions: no reference counterpart either; when each body cell frees up (from len, grow_to and the piece
 *                      order of the state), the flood fill that may pass through a cell once it has, and the opponent
 *                      that counts its room that way.
 *   msnake_head_fields: no reference counterpart either; the same fronts seen from the cells' side, as whole-board planes:
 *                      how far every cell is from each head and which snake gets there first.
 *   msnake_copy_envs <- no reference counterpart (a reference env can only be re-created and replayed); the analogue is
 *                      ALE's cloneState / restoreState, batched and on the device: snapshot, fork and restore of envs
 *                      between two handles without the host round trip of msnake_get_state / msnake_set_state.
 *   msnake_render_cells <- get_ob_for_snake / get_multi_snake_ob (snake_multiple_test.py:35-58,93-95) without its last
 *                      step, the colour table: which of six things each cell shows, per view, plus the per-snake facts.
 *   msnake_render_local: no reference counterpart; the head-centred, heading-aligned window of those cell codes that
 *                      snake policies outside the reference are trained on, cut on the device.
 *   msnake_render_rays: no reference counterpart; the eight-direction distance vector of snake agents (wall, fruit, own
 *                      body, another snake), read off the same cell codes on the device.
 *   msnake_agent_outcomes <- the per-snake rewards that update_snake computes and SnakeEnv.step drops for every snake
 *                      but the main one (snake_multiple_test.py:97-145,166-197), plus which snake died and each snake's episode
 *                      totals, which the reference never forms: what self-play needs to learn from every column.
 *   msnake_death_causes <- is_snake_alive (snake_multiple_test.py:147-164), whose verdict the reference reduces to one bit: whether
 *                      the head left the grid, and whose body or head it lies on, for every snake that was judged.
 *   msnake_fate_actions <- update_snake and is_snake_alive (snake_multiple_test.py:97-164) asked BEFORE the step: what each
 *                      of a snake's five actions leads to for certain, which risks remain, the two action masks that
 *                      follow, and the opponent that plays by them.
 *   msnake_generate_states: no reference counterpart (a reference env starts from its reset and nowhere else); random legal
 *                      positions with the body lengths the caller asks for, built on the device -- exploring starts.
 *   msnake_explore_actions, msnake_playout_explore: no reference counterpart (its opponents are networks, which sample);
 *                      epsilon-random moves of scripted players from a documented stream, standalone and inside the playout.
 *   msnake_get_stats <- the epinfobuf aggregation in ppo_multi_agent.py:288,331,366-390
 *
 * RNG contract (shared with oracle/ and tests/golden): draw i of global env g is word (i & 3) of
 * Philox4x32-10(counter = {i>>2 lo, i>>2 hi, g lo, g hi}, key = {seed lo, seed hi}) -- rocRAND's
 * (seed, subsequence, offset) convention -- and randint(n) = (u32 * n) >> 32.  g = env_id_base +
 * local index, so trajectories do not depend on how envs are sharded over GPUs.
 */
#ifndef MSNAKE_H
#define MSNAKE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSNAKE_ABI_VERSION 3

/* rule sets = the reference's gym ids (gym-snake/gym_snake/__init__.py:11-26) */
#define MSNAKE_RULES_SNAKE_ENV 0   /* snake-multiple-test-v0  : SnakeEnv            */
#define MSNAKE_RULES_NEW_WORLD 1   /* snake-new-multiple-v0   : NewMultipleSnakes   */
#define MSNAKE_RULES_ADVERSARIAL 2 /* snake-adversarial-v0    : SnakeAdversarial    */

#define MSNAKE_MAX_SNAKES 4
#define MSNAKE_MAX_FRUITS 32 /* inline fruits (snake_env / new_world) */
#define MSNAKE_MAX_DIM 62

#define MSNAKE_OK 0
#define MSNAKE_E_ARG (-1)     /* bad argument / configuration                     */
#define MSNAKE_E_HIP (-2)     /* a HIP runtime call failed (message has the text) */
#define MSNAKE_E_HANDLE (-3)  /* NULL or destroyed handle                         */
#define MSNAKE_E_ALIGN (-4)   /* device pointer not aligned as required           */
#define MSNAKE_E_STATE (-5)   /* malformed state buffer in set_state              */
#define MSNAKE_E_NOGPU (-6)   /* no usable HIP device                             */

typedef struct msnake_config {
    uint32_t struct_size;  /* = sizeof(msnake_config), for ABI evolution                   */
    int32_t device;        /* HIP device ordinal                                            */
    int32_t num_envs;      /* envs owned by this handle (this GPU's shard)                  */
    int32_t dim;           /* grid is dim x dim; observation is (dim+2) x (dim+2) x 3*views */
    int32_t n_snakes;      /* 1..3 for snake_env/adversarial (views fixed at 3), 1..4 new_world */
    int32_t n_fruits;      /* must equal n_snakes for snake_env/adversarial; 0..32 new_world */
    int32_t rules;         /* MSNAKE_RULES_*                                                */
    int32_t max_steps;     /* episode cap, 1..60000 (2000 in the reference; anything else is MSNAKE_E_ARG).  Under
                            * new_world the body storage is sized from it: see cap at msnake_get_state */
    int32_t auto_reset;    /* 1 = vec-env semantics (reset on done, return reset obs)       */
    int32_t obs_scale;     /* integer pixel replication of the observation (1 = native)     */
    uint64_t seed;         /* Philox key                                                    */
    uint64_t env_id_base;  /* global id of local env 0 (Philox subsequence = base + index)  */
    /* ---- ABI 3: launch tuning, all optional (0 = the library decides from the batch size).
     *      They change how the work is laid out on the GPU, never a result: every value is parity-tested.
     *      A caller built against ABI 2 passes struct_size = MSNAKE_CONFIG_SIZE_V2 (the fields above);
     *      the tail is then taken as zeros. */
    int32_t envs_per_block;    /* envs (= wavefronts) per workgroup: 0 auto | 1..8                      */
    int32_t record_policy;     /* MSNAKE_AUTO | MSNAKE_RECORD_FULL | MSNAKE_RECORD_SHORT (snake_env / adversarial) */
    int32_t obs_store_policy;  /* MSNAKE_AUTO | MSNAKE_STORE_PLAIN | MSNAKE_STORE_STREAM: msnake_step / reset / render */
    int32_t tape_store_policy; /* the same for msnake_rollout_tape                                      */
} msnake_config;

#define MSNAKE_CONFIG_SIZE_V2 56u
#define MSNAKE_AUTO 0
#define MSNAKE_RECORD_FULL 1  /* 256-byte env record: the upper half parks Philox draws between launches */
#define MSNAKE_RECORD_SHORT 2 /* only the first 128 bytes of the record move (bandwidth-bound batches)   */
#define MSNAKE_STORE_PLAIN 1  /* observation stores stay in L2 / Infinity Cache                          */
#define MSNAKE_STORE_STREAM 2 /* observation stores carry the nt (streaming) hint                        */

/* per-env info written by msnake_step, 16 bytes, same meaning as the reference's info dict */
typedef struct msnake_info {
    float ep_return;    /* info['episode']['r'] when done, else 0 */
    int32_t ep_len;     /* info['episode']['l'] when done, else 0 */
    int32_t num_snakes; /* info['num_snakes']                     */
    int32_t flags;      /* bit 0: done                            */
} msnake_info;

/* aggregate episode statistics since create (or since the last msnake_get_stats(reset=1)).  An
 * episode is counted on the step it ends; with auto_reset = 0 a finished env keeps returning
 * done = 1 until msnake_reset, but is counted once.  Per env the totals are kept as 32-bit episode
 * count / 64-bit length sum / 32-bit signed return sum between two msnake_get_stats(reset=1) calls. */
typedef struct msnake_stats {
    int64_t episodes;      /* number of finished episodes                 */
    int64_t ep_len_sum;    /* sum of their lengths                        */
    int64_t ep_return_sum; /* sum of their returns (rewards are integral) */
    int64_t env_steps;     /* env-steps executed                          */
    int64_t errors;        /* capacity guards tripped (0 in play from a reset; see msnake_set_state) */
    int64_t reserved[3];
} msnake_stats;

typedef struct msnake_env* msnake_handle;

int msnake_abi_version(void);
const char* msnake_last_error(void);

int msnake_create(const msnake_config* cfg, msnake_handle* out);
int msnake_destroy(msnake_handle h);

/* observation layout: uint8 [num_envs][H][W][C], C fastest (HWC like the reference) */
int msnake_obs_shape(msnake_handle h, int32_t* H, int32_t* W, int32_t* C);

/* Reset every env; writes observations if obs_dev != NULL.  Asynchronous on `stream`
 * (a hipStream_t passed as void*, NULL = the default stream). */
int msnake_reset(msnake_handle h, uint8_t* obs_dev, void* stream);

/* Reset only the envs that mask_dev (uint8 [num_envs], non-zero = selected; a step's done_dev can be passed
 * as it is) selects.  Extends the auto-reset of subproc_vec_env.py:13-16, which drops the last observation of an
 * episode: with final_obs_dev != NULL every selected env's current, pre-reset observation is first rendered into
 * its row of final_obs_dev, then the selected envs are reset and their reset observations written to obs_dev
 * (if non-NULL).  Rows of unselected envs are left untouched in both.  truncated_dev (uint8 [num_envs], may be
 * NULL) is written for every env: 1 iff the env is selected, its episode has ended, t >= max_steps and the rule
 * set's own end condition does not hold (snake_env / adversarial: the main snake is dead; new_world: the main
 * snake's alive bit, the reference's done = snake.alive), i.e. the time cap alone ended it.  A selected env whose
 * episode had not ended is abandoned: it is not counted in msnake_get_stats, as with msnake_reset.
 * msnake_step on a handle with auto_reset = 0 followed by msnake_reset_envs(done_dev, obs_dev, ...) on the same
 * stream gives exactly what auto_reset = 1 gives, plus the terminal observations and the truncation flags.
 * mask_dev NULL is MSNAKE_E_ARG (msnake_reset resets every env).  Both observation pointers need 4-byte
 * alignment at obs_scale 4 / 7 (MSNAKE_E_ALIGN).  Asynchronous; adds nothing to env_steps. */
int msnake_reset_envs(msnake_handle h, const uint8_t* mask_dev, uint8_t* obs_dev, uint8_t* final_obs_dev,
                      uint8_t* truncated_dev, void* stream);

/* One lockstep step of every env.  actions_dev: int32 [num_envs][action_stride], entry s of a
 * row is snake s's action in {0..4}; action_stride >= n_snakes, surplus entries are ignored
 * (ppo_multi_agent.py:41-44 always sends tuples of 2 or 3).  rew_dev float32[num_envs],
 * done_dev uint8[num_envs], info_dev msnake_info[num_envs] (may be NULL).  obs_dev may be NULL (no
 * render); it needs no alignment at obs_scale 1 and 4-byte alignment at obs_scale 4 / 7
 * (MSNAKE_E_ALIGN otherwise).  Asynchronous. */
int msnake_step(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, uint8_t* obs_dev,
                float* rew_dev, uint8_t* done_dev, msnake_info* info_dev, void* stream);

/* Same, for `n_steps` consecutive steps from an action tape int32 [n_steps][num_envs][stride];
 * outputs of step k go to obs_dev + k*obs_step_bytes etc. when the *_step_stride arguments are
 * non-zero, or are overwritten in place when they are zero.  One launch per step, issued from C. */
int msnake_step_tape(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, int32_t n_steps,
                     uint8_t* obs_dev, size_t obs_step_stride, float* rew_dev, uint8_t* done_dev,
                     msnake_info* info_dev, size_t scalar_step_stride, void* stream);

/* Same contract and same results as msnake_step_tape, but ONE persistent launch: every wave keeps
 * its env in registers across the n_steps steps, so there is no per-step launch boundary and no
 * per-step state round trip.  For callers that have the actions of several steps up front
 * (scripted / random opponents, evaluation replays, benchmarks); a policy in the loop needs
 * msnake_step.  At obs_scale 1 the persistent kernel keeps a second copy of the observation image in
 * LDS; on a handle whose two images and occupancy bytes pass 64 KB (with 9 channels from dim 57, with
 * the 12 of a 4-snake new_world handle from dim 49: msnake_launch_shape_for_config reports it) the call
 * is served by the per-step launches of msnake_step_tape instead, decided on the host before anything
 * is launched: the same results and the same env_steps, nothing allocated, still capturable. */
int msnake_rollout_tape(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, int32_t n_steps,
                        uint8_t* obs_dev, size_t obs_step_stride, float* rew_dev, uint8_t* done_dev,
                        msnake_info* info_dev, size_t scalar_step_stride, void* stream);

/* Canonical per-env state as int32 words (blocking; test / checkpoint path):
 *  [0] t  [1] ctr_lo  [2] ctr_hi  [3] spare_fruits  [4] ep_len  [5] ep_return (f32 bits)
 *  [6] n_fruits_cur  [7] n_snakes | finished << 8, then n_fruits_cur x (c0,c1), then per snake:
 *  len, v0, v1, grow_to, alive, in_dead, len x (c0,c1) head first.
 * `finished` (bit 8 of word 7): the episode has ended and the env has not been reset since (only ever set
 * with auto_reset = 0); it keeps a restored env from counting that episode into msnake_get_stats again.
 * What msnake_set_state accepts, complete; every accepted state comes back from msnake_get_state word for word, and
 * anything else is MSNAKE_E_STATE with one of six reasons in the message, the env left untouched.  With
 *   cap  = the body capacity: dim^2 + 2, under new_world max(dim^2 + 2, max_steps + 2), rounded up to a multiple of 64,
 *   fcap = the adversarial fruit-list capacity: n_snakes + n_snakes * (dim^2 + 2), rounded up to a multiple of 64,
 * the checks run in this order and the first that fails names the reason:
 *   1. at least 8 words (else "too short");
 *   2. word 7 is n_snakes, or n_snakes | 0x100; any other bit set is "snake count";
 *   3. t, spare_fruits and ep_len are >= 0 ("scalar").  t has no upper bound (a handle with a lower max_steps may be
 *      given any t; its next step ends the episode); ctr and the bits of ep_return are free;
 *   4. n_fruits_cur equals the handle's n_fruits (snake_env, new_world), lies in [0, fcap] (adversarial) ("fruit count");
 *   5. the words reach to the end of the fruit list ("too short");
 *   6. every fruit lies inside the grid [0, dim)^2; an entry of the adversarial list lies in [-1, dim]^2, one step
 *      outside the grid being where the reference can put a dead snake's head ("cell");
 *   7. then for snake 0, 1, ... in turn: its six header words are there ("too short"); len lies in [0, cap - 2]
 *      ("length"); its len cells are there ("too short"); (v0, v1) is one of (0,0), (1,0), (0,1), (-1,0), (0,-1),
 *      grow_to >= 0, alive and in_dead are 0 or 1 under new_world and exactly alive = 1, in_dead = 0 under snake_env and
 *      adversarial, which is what msnake_get_state reports there ("scalar"); the head lies in [-1, dim]^2 and every
 *      piece behind it inside the grid ("cell").  Cells may repeat, within a body and between bodies.  (A head
 *      outside the grid moves the handle to the generic step kernels: see msnake_kernel_name.)
 * Words behind the last snake are ignored.
 * Two capacity conditions can only arise in play after such a state was installed, so they are not refused but counted:
 * a body that would grow beyond cap - 1 pieces stays at cap - 1 (its oldest piece is dropped), and pieces of dying
 * adversarial snakes that would take the fruit list beyond fcap entries are dropped, the list ending at fcap.  Each
 * adds 1 per env and step to `errors` of msnake_get_stats; neither is reachable from a reset.  From such a step on the
 * env no longer follows the reference; every other env does, and every call keeps working.
 * msnake_get_state returns the number of words needed/written (>0) or a negative error. */
int msnake_get_state(msnake_handle h, int32_t env, int32_t* words, int32_t cap);
int msnake_set_state(msnake_handle h, int32_t env, const int32_t* words, int32_t n);

/* The same canonical words for EVERY env of the handle in one host buffer (blocking; checkpoints):
 * one packing kernel on the device and one copy, instead of num_envs round trips.  Layout of `buf`:
 *   { uint32 magic "MSST", uint32 version (2; version-1 blobs, which lack the finished bit, are accepted),
 *     int32 num_envs, dim, n_snakes, n_fruits, rules, reserved,
 *     uint64 total_words }  (40 bytes)
 *   uint64 offsets[num_envs + 1]   word offset of env e's state inside `words`
 *   int32  words[total_words]      env e's words = words[offsets[e] .. offsets[e+1]), layout as above
 * msnake_get_state_all returns the number of bytes needed; it writes them only if buf != NULL and
 * cap_bytes suffices (call once with NULL to size the buffer).  msnake_set_state_all checks the
 * blob against the handle's configuration and every env's words like msnake_set_state does; envs
 * with malformed words are left untouched and the call fails with MSNAKE_E_STATE.  The per-env
 * logging totals (msnake_get_stats) are not part of the canonical state and are kept. */
int64_t msnake_get_state_all(msnake_handle h, void* buf, size_t cap_bytes);
int msnake_set_state_all(msnake_handle h, const void* buf, size_t bytes);

/* What a blob holds, checked on the host without a handle or a device: magic / version, the offset table
 * (starts at 0, never decreases, ends at total_words) and that `bytes` covers all of it.  MSNAKE_E_STATE
 * otherwise.  Lets a caller size the handle a checkpoint needs before creating it; msnake_set_state_all
 * runs the same check first.  `out` may be NULL. */
typedef struct msnake_blob_info {
    int32_t version, num_envs, dim, n_snakes, n_fruits, rules;
    int64_t total_words;
} msnake_blob_info;
int msnake_state_blob_info(const void* buf, size_t bytes, msnake_blob_info* out);

/* ---- The canonical words as a device tensor: export, import and 64-bit hashes of EVERY env, asynchronous on `stream`.
 * The words are exactly those documented at msnake_get_state.  The three calls below allocate nothing, never
 * synchronise, draw no random numbers, add nothing to env_steps, and can be captured into a HIP graph in front of or
 * behind a step; export and hash only read the handle.  MSNAKE_E_HANDLE for a NULL or destroyed handle. */

/* The largest word count any state the handle accepts can have: 8 + 2 * F + n_snakes * (6 + 2 * (cap - 2)), F being
 * n_fruits under snake_env and new_world and fcap under adversarial (cap, fcap: see msnake_get_state).  A row of that
 * many words holds every env of the handle, whatever is played or installed.  Host only, no device work; negative
 * MSNAKE_E_HANDLE for a NULL handle. */
int32_t msnake_state_words_max(msnake_handle h);

/* Every env's words into row e of words_dev, int32 [num_envs][stride], and their number into count_dev, int32
 * [num_envs]; either may be NULL, not both.  count_dev[e] is the number of words env e's state has, whatever stride
 * is.  If that number is <= stride, words [0, n) of row e are exactly what msnake_get_state returns and words
 * [n, stride) are not written; if it is larger, NO word of row e is written, and count_dev is how the caller learns of
 * it.  Both pointers 4-byte aligned (MSNAKE_E_ALIGN otherwise).  MSNAKE_E_ARG, before any device work: stride < 0;
 * words_dev given with stride 0; both outputs NULL (nothing to write). */
int msnake_export_states(msnake_handle h, int32_t* words_dev, int32_t stride, int32_t* count_dev, void* stream);

/* What msnake_import_states writes to status_dev[e]: SKIPPED where the mask is 0, OK where the row was installed, else
 * why it was refused -- the six reasons of msnake_set_state, in the order their checks are listed at msnake_get_state
 * ("too short", "snake count", "fruit count", "cell", "length", "scalar"). */
#define MSNAKE_STATE_OK 0
#define MSNAKE_STATE_TOO_SHORT 1
#define MSNAKE_STATE_SNAKE_COUNT 2
#define MSNAKE_STATE_FRUIT_COUNT 3
#define MSNAKE_STATE_CELL 4
#define MSNAKE_STATE_LENGTH 5
#define MSNAKE_STATE_SCALAR 6
#define MSNAKE_STATE_SKIPPED 0xFF

/* Row e of words_dev, int32 [num_envs][stride], into env e, for the envs mask_dev selects: uint8 [num_envs], non-zero =
 * selected, NULL = every env.  count_dev, int32 [num_envs], is the number of words of each row; NULL = every row has
 * `stride` words, and words behind the last snake are ignored as msnake_set_state ignores them.  A count_dev[e] below 0
 * or above stride is reason "too short".  status_dev, uint8 [num_envs], is required and written for EVERY env:
 * MSNAKE_STATE_SKIPPED where the mask is 0 -- such an env is untouched, byte for byte --, MSNAKE_STATE_OK where the row
 * was installed, otherwise one of the six reasons above -- such an env is left untouched as well.  The checks, their
 * order and the first-failing-reason rule are items 1-7 at msnake_get_state; a row is validated as a whole before any
 * word of the env is written, and no word past its count is read.  An accepted env ends up exactly as
 * msnake_set_state(h, e, row, n) leaves it: the logging totals are kept, parked random draws are cleared, the
 * `finished` bit is restored, an episode in progress is abandoned, not counted.
 * One deliberate difference: the host cannot learn of a head outside the grid without a synchronisation, so
 *   - a handle that currently runs a step kernel compiled for its shape (msnake_kernel_name) REFUSES such a head with
 *     MSNAKE_STATE_CELL (install it with msnake_set_state, which moves the handle to the generic kernels, if needed);
 *   - a handle on the generic kernels accepts it, as msnake_set_state does, and counts from then on as one that may hold
 *     such a head (msnake_copy_envs from it moves the destination to the generic kernels too).
 * Refusals are data, not errors: the call returns MSNAKE_OK when the launch was issued.  MSNAKE_E_ARG, before any device
 * work: words_dev or status_dev NULL; stride < 8.  MSNAKE_E_ALIGN: words_dev or count_dev not 4-byte aligned. */
int msnake_import_states(msnake_handle h, const uint8_t* mask_dev, const int32_t* words_dev, int32_t stride,
                         const int32_t* count_dev, uint8_t* status_dev, void* stream);

/* A 64-bit hash of every env's words into hash_dev, uint64 [num_envs], 8-byte aligned (MSNAKE_E_ALIGN otherwise).  With
 * w[0..n) env e's canonical words,
 *     H = sum over the selected i of mix64(((uint64)(i + 1) << 32) | (uint32)w[i])   mod 2^64,
 * mix64 the splitmix64 finaliser: z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 * z ^= z >> 31.  Any holder of the words computes the same key on the host.
 *   MSNAKE_HASH_FULL:  every word.
 *   MSNAKE_HASH_BOARD: the position only -- words 0, 1, 2, 4, 5 (t, the draw counter, ep_len, ep_return) are left out
 *     and bit 8 of word 7 (`finished`) is cleared; spare_fruits stays, because it changes adversarial play.  Two envs
 *     with equal BOARD hashes render the same frame.
 * Any other `what` is MSNAKE_E_ARG; so is a NULL hash_dev. */
#define MSNAKE_HASH_FULL 0u
#define MSNAKE_HASH_BOARD 1u
int msnake_hash_states(msnake_handle h, uint32_t what, uint64_t* hash_dev, void* stream);

/* Render the current state of every env without stepping (asynchronous). */
int msnake_render(msnake_handle h, uint8_t* obs_dev, void* stream);

/* Scripted opponents and safe-move masks, computed on the device from the current state of every env (the state
 * the canonical words above describe).  Serves the callers that today can only put a network or the constant
 * action 1 into an opponent's column (evaluate_snake.py, ppo_multi_agent.py:28-50).  Terms: `used` = the cells of
 * every body in the env, heads, tails, new_world bodies kept after a self-hit and stacked duplicates included;
 * move a in 1..4 goes from the head by (+1,0), (0,+1), (-1,0), (0,-1) on (c0,c1); a move is open iff its target
 * lies in [0,dim)^2 and not in `used`.
 *   MSNAKE_POLICY_SAFE_GREEDY: the first open move, in the order 1, 2, 3, 4, whose target has the strictly
 *     smallest L1 distance to any fruit of the state's fruit list (adversarial: the complete list; distance 0
 *     when the list is empty); 0 when no move is open or the body is empty.  The velocity plays no part.
 *   MSNAKE_POLICY_HAMILTONIAN: the head's successor on a fixed Hamiltonian cycle of an even board (column 0 is
 *     the return lane, the rows run back and forth over columns 1..dim-1): at (x,y), x == 0 -> (y > 0 ? 4 : 1);
 *     y even -> (x < dim-1 ? 1 : 2); y == dim-1 -> 3; else (x > 1 ? 3 : 2).  0 for an empty body or a head
 *     outside the grid.  Odd dim is MSNAKE_E_ARG.
 * actions_dev: int32 [num_envs][action_stride], the buffer the step takes; entry s of every row is written for
 * each s with bit s of snake_mask set, all other entries are left untouched.  safe_dev (may be NULL): uint8
 * [num_envs][n_snakes], written for every snake whatever snake_mask is: bit a (1..4) is set iff move a is open,
 * bits 0 and 5..7 are zero, an empty body gives 0.  MSNAKE_POLICY_NONE writes safe_dev only.
 * The call only reads the handle's state (no random numbers are drawn, the Philox counter stays), allocates
 * nothing and does not synchronise: it can be captured into a HIP graph in front of the step.  Asynchronous on
 * `stream`; adds nothing to env_steps.  MSNAKE_E_ARG, before any device work: unknown policy; a snake_mask bit
 * >= n_snakes; action_stride < n_snakes or actions_dev NULL when actions are to be written; nothing to write. */
#define MSNAKE_POLICY_NONE 0         /* write no actions (safe_dev only) */
#define MSNAKE_POLICY_SAFE_GREEDY 1
#define MSNAKE_POLICY_HAMILTONIAN 2
int msnake_scripted_actions(msnake_handle h, int32_t policy, uint32_t snake_mask, int32_t* actions_dev,
                            int32_t action_stride, uint8_t* safe_dev, void* stream);

/* Reachable-space counts and the flood-fill opponent space_greedy, in the terms of msnake_scripted_actions (`used`,
 * moves 1..4, open); a cell is free iff it lies in the grid and not in `used`.
 * space_dev (may be NULL): uint16 [num_envs][n_snakes][4], written for every snake whatever snake_mask is: entry m
 * is the number of free cells 4-connected to the target of move m + 1 through free cells, the target included; 0
 * when move m + 1 is not open, and all four are 0 for an empty body.  At most 62^2 - 1.  2-byte aligned
 * (MSNAKE_E_ALIGN otherwise).
 * safe_dev (may be NULL): exactly what msnake_scripted_actions writes there.
 * actions_dev: int32 [num_envs][action_stride]; entry s of every row is written for each s with bit s of
 * snake_mask set, all other entries are left untouched.  The policy space_greedy: with len = the snake's body
 * length as the canonical state gives it (duplicates counted), the action is 0 if the body is empty or no move is
 * open; otherwise need = min(len, max over the open moves of space), the eligible moves are the open moves with
 * space >= need, and the action is the first eligible move, in the order 1, 2, 3, 4, whose target has the strictly
 * smallest L1 distance to any fruit of the state's fruit list (adversarial: the complete list; distance 0 when the
 * list is empty).  The velocity plays no part; odd boards are fine.
 * Like its sibling the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in
 * front of the step.  MSNAKE_E_ARG, before any device work: a snake_mask bit >= n_snakes; actions_dev NULL or
 * action_stride < n_snakes when snake_mask != 0; nothing to write (snake_mask 0, safe_dev and space_dev NULL). */
int msnake_space_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                         uint8_t* safe_dev, uint16_t* space_dev, void* stream);

/* Voronoi territory counts and the opponent territory_greedy, in the terms of the two calls above (`used`, moves 1..4,
 * free, open).  Bodies are static: tails do not recede, and neither the velocity nor the alive bit plays a part (a
 * new_world snake that kept its body after a self-hit still moves, so it counts like any other).
 * territory_dev (may be NULL): uint16 [num_envs][n_snakes][4], written for every snake whatever snake_mask is.  For
 * snake s with a non-empty body and open move m + 1 with target t: O_s = the targets of the open moves of every OTHER
 * snake with a non-empty body (where they can stand after the same lockstep step); dA(c) = the BFS distance from t to
 * c through free cells, 4-connected; dB(c) = the BFS distance from the set O_s, infinite when O_s is empty or c cannot
 * be reached from it.  Entry m = |{ c free : dA(c) < dB(c) }|, the cells s reaches strictly first; ties go to the
 * others.  So the entry is 0 when the move is not open or the body is empty, and ALSO for an open move whose target
 * lies in O_s -- a head-on cell, where both snakes die in this env; safe_dev tells the two zero cases apart.  When no
 * other snake can move, the entry equals space_dev of the call above exactly.  At most 62^2 - 1.  2-byte aligned
 * (MSNAKE_E_ALIGN otherwise).
 * safe_dev (may be NULL): exactly what the two calls above write there.
 * actions_dev: int32 [num_envs][action_stride]; entry s of every row is written for each s with bit s of
 * snake_mask set, all other entries are left untouched.  The policy territory_greedy is space_greedy with territory
 * in place of space: the action is 0 if the body is empty or no move is open; otherwise need = min(len, max over the
 * open moves of territory), with len the canonical state's body length (duplicates counted); the eligible moves are
 * the open moves with territory >= need -- when every open move has territory 0, all open moves; and the action is
 * the first eligible move, in the order 1, 2, 3, 4, whose target has the strictly smallest L1 distance to any fruit
 * of the state's fruit list (adversarial: the complete list; distance 0 when the list is empty).
 * Like its siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in
 * front of the step.  MSNAKE_E_ARG, before any device work: a snake_mask bit >= n_snakes; actions_dev NULL or
 * action_stride < n_snakes when snake_mask != 0; nothing to write (snake_mask 0, safe_dev and territory_dev NULL). */
int msnake_territory_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                             uint8_t* safe_dev, uint16_t* territory_dev, void* stream);

/* Shortest-path distances to the fruits, the whole distance field, and the opponent path_greedy, in the terms of the
 * three calls above (`used`, moves 1..4, free, open).  Bodies are static: tails do not recede, and neither the velocity
 * nor the alive bit plays a part.
 * Sources: the entries of the state's fruit list (adversarial: the complete list) that lie in [0,dim)^2 and are free.  An
 * entry at -1 or dim is no source, neither is a fruit under a body (or under a head at reset); duplicates count once.
 * The field F(c): for a free cell c, the length of the shortest 4-connected path through free cells from c to a
 * source, 0 on a source; MSNAKE_PATH_NONE for a cell in `used`, for a free cell whose region holds no source, and
 * everywhere when there is no source.  A finite value is at most dim^2 - 2.
 * field_dev (may be NULL): uint16 [num_envs][dim][dim], entry [c0][c1] = F((c0, c1)), the indexing of the
 * msnake_render_cells planes.  2-byte aligned (MSNAKE_E_ALIGN otherwise).
 * path_dev (may be NULL): uint16 [num_envs][n_snakes][4], written for every snake whatever snake_mask is: entry m =
 * F(target of move m + 1) when that move is open, MSNAKE_PATH_NONE when it is not or the body is empty.  0 means the
 * move eats; 1 + the minimum over m is the snake's own distance (its head lies in `used`, so the field holds NONE
 * there).  2-byte aligned (MSNAKE_E_ALIGN otherwise).
 * safe_dev (may be NULL): exactly what the three calls above write there.
 * actions_dev: int32 [num_envs][action_stride]; entry s of every row is written for each s with bit s of
 * snake_mask set, all other entries are left untouched.  The policy path_greedy: the action is 0 if the body is empty
 * or no move is open; otherwise the eligible moves are exactly space_greedy's (with space as msnake_space_actions
 * defines it, need = min(len, max over the open moves of space), eligible = open and space >= need), and the action is
 * the eligible move with the smallest path entry, the first in the order 1, 2, 3, 4 on a tie.  If every eligible
 * move's entry is MSNAKE_PATH_NONE the action is space_greedy's own, so path_greedy equals space_greedy wherever no
 * source can be reached.
 * Like its siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in
 * front of the step.  MSNAKE_E_ARG, before any device work: a snake_mask bit >= n_snakes; actions_dev NULL or
 * action_stride < n_snakes when snake_mask != 0; nothing to write (snake_mask 0, safe_dev, path_dev and field_dev
 * NULL). */
#define MSNAKE_PATH_NONE 0xFFFFu
int msnake_path_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                        uint8_t* safe_dev, uint16_t* path_dev, uint16_t* field_dev, void* stream);

/* Cell lifetimes, the timed reach of every move, and the opponent timed_greedy, in the terms of the four calls above
 * (`used`, moves 1..4, free, open).  Here bodies are NOT static: a body cell can be entered once the piece lying there has
 * moved on.  Neither the velocity nor the alive bit plays a part (a new_world body kept after a self-hit counts like any
 * other).
 * Piece lifetime: for snake s with body length len and grow_to as the canonical state gives them, piece i (0 the head,
 * len - 1 the tail) has l(s, i) = min(0xFFFE, (len - i) + max(0, grow_to - len)), formed without 32-bit overflow
 * (grow_to of an installed state may be 2^31 - 1).  Under new_world with the handle's n_fruits == 0 every piece has
 * l = MSNAKE_LIFE_NEVER: there the rule set never pops.
 * Cell lifetime: Life(c) = the maximum of l over all pieces of all snakes that lie on c, stacked duplicates included; 0
 * for a cell with no piece, so Life(c) > 0 <=> c in `used`.  Pieces outside the grid are ignored.  If every snake moves
 * on every step and nobody eats or dies, cell c is free of today's pieces after exactly Life(c) steps.  The step pops
 * before it tests collisions, so entering a cell only when Life < t (below) is one step conservative, the convention
 * by which `open` counts tails as used.
 * Timed fill from the target T of an open move: V_1 = F_1 = {T}; for t = 2, 3, ...: F_t = { c in the grid : c not in
 * V_(t-1), Life(c) < t, c 4-adjacent to a cell of F_(t-1) }, V_t = V_(t-1) + F_t; stop when F_t is empty.  Only the
 * last front expands: a cell is taken once, at the first level that both reaches and admits it, and a cell skipped
 * because it was still occupied can be taken later only from another, later front cell.  At most dim^2 levels.
 * reach_dev (may be NULL): uint16 [num_envs][n_snakes][4], written for every snake whatever snake_mask is: entry m =
 * |V| of the fill from the target of move m + 1; 0 when that move is not open or the body is empty.  So reach >= space
 * of msnake_space_actions entry for entry, reach == 0 <=> the move is not open, and reach == space where every
 * lifetime is MSNAKE_LIFE_NEVER.  At most 62^2.  2-byte aligned (MSNAKE_E_ALIGN otherwise).
 * life_dev (may be NULL): uint16 [num_envs][dim][dim], entry [c0][c1] = Life((c0, c1)), the indexing of the
 * msnake_render_cells planes and of field_dev.  2-byte aligned (MSNAKE_E_ALIGN otherwise).
 * safe_dev (may be NULL): exactly what the four calls above write there.
 * actions_dev: int32 [num_envs][action_stride]; entry s of every row is written for each s with bit s of
 * snake_mask set, all other entries are left untouched.  The policy timed_greedy is space_greedy with the timed reach
 * in place of the space: the action is 0 if the body is empty or no move is open; otherwise need = min(len, max over
 * the open moves of reach), the eligible moves are the open moves with reach >= need, and the action is the first
 * eligible move, in the order 1, 2, 3, 4, whose target has the strictly smallest L1 distance to any fruit of the
 * state's fruit list (adversarial: the complete list; distance 0 when the list is empty).
 * Like its siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in
 * front of the step.  MSNAKE_E_ARG, before any device work: a snake_mask bit >= n_snakes; actions_dev NULL or
 * action_stride < n_snakes when snake_mask != 0; nothing to write (snake_mask 0, safe_dev, reach_dev and life_dev
 * NULL). */
#define MSNAKE_LIFE_NEVER 0xFFFFu
int msnake_timed_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                         uint8_t* safe_dev, uint16_t* reach_dev, uint16_t* life_dev, void* stream);

/* Where the snakes stand relative to every cell: each snake's BFS distance to every cell, the Voronoi owner map, and the
 * number of cells each snake owns, in the terms of the calls above (`used`, moves 1..4, free, open).  Bodies are static,
 * and neither the velocity nor the alive bit plays a part.
 * D_s(c), for snake s with a non-empty body: for a free cell c, 1 + the minimum over the open moves m of s of the
 * 4-connected BFS distance through free cells from the target of m to c; MSNAKE_HEAD_NONE when s has no open move or c
 * cannot be reached.  A head at -1 or dim with an open move into the grid is a source like any other.  D_s(head of s) = 0
 * when the head lies in [0,dim)^2, although the head is in `used`, and even when another piece is stacked on it; every
 * other cell of `used` holds MSNAKE_HEAD_NONE.  For an empty body the whole plane is MSNAKE_HEAD_NONE.  A finite value
 * is at most dim^2 - 1.
 * dist_dev (may be NULL): uint16 [num_envs][P][dim][dim], P = popcount(snake_mask), the planes of the selected snakes in
 * ascending order; entry [c0][c1] = D_s((c0, c1)), the indexing of the msnake_render_cells planes.  2-byte aligned
 * (MSNAKE_E_ALIGN otherwise).
 * owner_dev (may be NULL): uint8 [num_envs][dim][dim], over ALL snakes whatever snake_mask is.  For a free cell c let
 * d = min over s of D_s(c): MSNAKE_OWNER_NONE if d is MSNAKE_HEAD_NONE, the index of the snake that attains d if exactly
 * one does, MSNAKE_OWNER_TIE if two or more do.  Every cell of `used`, heads included, holds MSNAKE_OWNER_NONE.
 * counts_dev (may be NULL): uint16 [num_envs][n_snakes], entry s = the number of cells whose owner is s.  2-byte aligned
 * (MSNAKE_E_ALIGN otherwise).
 * Like its siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in
 * front of or behind the step.  MSNAKE_E_ARG, before any device work and in this order: a snake_mask bit >= n_snakes;
 * dist_dev non-NULL with snake_mask == 0; nothing to write (all three pointers NULL, whatever snake_mask is).  Alignment
 * errors come after these. */
#define MSNAKE_HEAD_NONE  0xFFFFu
#define MSNAKE_OWNER_TIE  0xFEu
#define MSNAKE_OWNER_NONE 0xFFu
int msnake_head_fields(msnake_handle h, uint32_t snake_mask, uint16_t* dist_dev, uint8_t* owner_dev,
                       uint16_t* counts_dev, void* stream);

/* Copy env state from `src` into `dst` on the device: destination env e receives the state of source env
 * src_index_dev[e] (int32 [dst.num_envs], a device pointer).  A negative entry leaves destination env e completely
 * untouched: no byte of its record, rings or lists is written.  NULL means the identity and needs equal env counts.
 * An entry >= src.num_envs leaves env e untouched and adds 1 to that env's `errors` total (msnake_get_stats); nothing
 * out of range is read.  The same holds for a body that does not fit the destination (possible only between new_world
 * handles of different max_steps, whose body capacity follows the episode cap).
 * What moves is exactly the canonical state the words above describe -- t, the 64-bit draw counter, spare_fruits,
 * ep_len, ep_return, the fruit list, every snake's fields and cells, the new_world alive / in_dead bits, `finished`:
 * afterwards msnake_get_state(dst, e) returns word for word what msnake_get_state(src, src_index[e]) returned before.
 * What stays, as with msnake_set_state: the destination env's logging totals and the destination's configuration
 * (num_envs, record_policy, envs_per_block, obs_scale, auto_reset, max_steps, seed and env_id_base may all differ
 * between the two handles).  A destination env whose episode was in progress is abandoned: it is not counted in
 * msnake_get_stats, as with msnake_reset.
 * Random numbers: the Philox subsequence of an env is its slot's global id (env_id_base + index, see the RNG contract
 * above) and is not part of the state.  A copy into the SAME global slot (equal seed and env_id_base, src_index[e] ==
 * e: snapshot / restore) therefore continues bit-identically to the source; a copy into another slot starts from the
 * same position and draws from its own slot's stream at the copied counter.  Draws that a full-record source has
 * parked for later steps belong to the source slot's stream: they are never copied.
 * `src` is only read.  The call allocates nothing, does not synchronise, draws no random numbers and adds nothing to
 * env_steps: it can be captured into a HIP graph in front of a step.  Asynchronous on `stream`; the caller orders it
 * against work on both handles.  MSNAKE_E_ARG, before any device work: dst == src (stage an in-place permutation
 * through a second handle); dim, n_snakes, n_fruits or rules differ; the devices differ; src_index_dev NULL with
 * different env counts. */
int msnake_copy_envs(msnake_handle dst, msnake_handle src, const int32_t* src_index_dev, void* stream);

/* Why each snake died in a step, and on whose body: snake_env and adversarial handles only.  `before` holds the state of
 * every env in front of ONE msnake_step of `after` -- typically filled by msnake_copy_envs(before, after, NULL, stream)
 * on the same stream just before the step -- and `after` is the stepped handle, read before any msnake_reset_envs.
 * Under these two rule sets every snake moves, then every snake is judged against the same post-move bodies, then the
 * dead bodies are cleared (snake_multiple_test.py:147-197); a cleared snake keeps its velocity and grow_to words.  So the
 * bodies the snakes were judged with follow from the two canonical states alone, without actions or random numbers.
 * With P = the snakes whose len before is > 0, for k in P:
 *   len after(k) > 0:  B'_k = k's body in the after state;
 *   otherwise, with v = k's velocity words in the after state:
 *     v == (0, 0):     B'_k = k's body before;
 *     else:            H = head before + v, popped = (len before >= grow_to after), and
 *                      B'_k = [H] followed by pieces 0 .. len before - 1 - popped of the body before.
 * H_s = piece 0 of B'_s.  Cells are compared as coordinate pairs, -1 and dim included.  S = n_snakes below.
 * cause_dev (may be NULL): uint8 [num_envs][S].  For s in P any combination of
 *   MSNAKE_CAUSE_WALL     H_s lies outside [0, dim)^2
 *   MSNAKE_CAUSE_SELF     H_s equals a piece i >= 1 of B'_s
 *   MSNAKE_CAUSE_HEAD_ON  H_s == H_k for some k in P, k != s
 *   MSNAKE_CAUSE_BODY     H_s equals a piece i >= 1 of B'_k for some k in P, k != s
 *   and 0 for s not in P.  There is no short-circuit: every bit that holds is set (two heads that meet on a third
 *   snake's body give HEAD_ON | BODY).
 * by_dev (may be NULL): uint8 [num_envs][S]: bit k (0..3) is set iff BODY holds against snake k, bit 4 + k iff HEAD_ON
 *   holds against snake k.
 * victims_dev (may be NULL): uint8 [num_envs][S]: the same relation from the other side, row-aligned with the killer's
 *   reward: bit s of victims[k] is set iff bit k of by[s] is, bit 4 + s iff bit 4 + k of by[s] is.
 * where_dev (may be NULL): int8 [num_envs][S][2]: H_s as (c0, c1) where cause[s] != 0 (values -1 .. dim), (-2, -2) where
 *   cause[s] == 0.
 * No output needs any alignment.  Guarantee: when `before` and `after` are one msnake_step apart, cause[s] != 0 <=>
 * len before(s) > 0 && len after(s) == 0, which is MSNAKE_AGENT_DIED of msnake_agent_outcomes.  For any other pair of
 * states the outputs are what the formulas give, and they mean nothing.
 * Like its siblings the call only reads both handles, draws no random numbers, allocates nothing, does not synchronise
 * and adds nothing to env_steps; asynchronous on `stream`, and [msnake_copy_envs, msnake_step, msnake_agent_outcomes,
 * msnake_death_causes, msnake_reset_envs] can be captured into one HIP graph.  Refusals, before any device work and in
 * this order: MSNAKE_E_HANDLE for a NULL or destroyed handle; MSNAKE_E_ARG for after == before; for dim, n_snakes,
 * n_fruits, rules or device that differ; for num_envs that differ; for new_world rules (they judge the snakes one after
 * the other, clear bodies as they go and pop inside the fruit loop, new_world.py:101-158: how often a cleared snake
 * popped depends on which fruit it ate, which two states do not tell); for `after` created with auto_reset = 1 (the
 * after-state of a done env is gone; `before` may have any auto_reset); for four NULL outputs.  record_policy,
 * envs_per_block, obs_scale, max_steps and seed may differ between the two handles, as for msnake_copy_envs. */
#define MSNAKE_CAUSE_WALL 1
#define MSNAKE_CAUSE_SELF 2
#define MSNAKE_CAUSE_HEAD_ON 4
#define MSNAKE_CAUSE_BODY 8
int msnake_death_causes(msnake_handle after, msnake_handle before, uint8_t* cause_dev, uint8_t* by_dev, uint8_t* victims_dev,
                        int8_t* where_dev, void* stream);

/* The one-step fate of every move, the two action masks that follow from it, and the opponent wary_greedy: snake_env and
 * adversarial handles only.  Under these two rule sets every snake moves (update_snake pops, then inserts the new head,
 * snake_multiple_test.py:97-145), then every snake is judged against the same post-move bodies (is_snake_alive,
 * :147-164), and whether a piece stays depends only on len, grow_to and the fruit list.  So what happens to snake s if it
 * plays action a now follows from the state, but for what the others play and for where a fruit eaten earlier in the same
 * step respawns; those two are named as risks.  S = n_snakes, P = the snakes with len > 0.
 *   Effective direction d(k, a) of action a in 0..4 for snake k with velocity v_k: what turn() leaves
 *     (snake_multiple_test.py:108-115): a = 0 keeps v_k; a in 1..4 gives the move vector (+1,0), (0,+1), (-1,0), (0,-1)
 *     unless that is the reverse of v_k, then v_k.
 *   Standing: d == (0, 0), the state after a reset.  The snake stands: no move, no pop, no eating.
 *   Target: T(k, a) = head_k + d(k, a); for a standing snake it is the head.
 *   Fruit count: fruits(c) = the number of entries of the state's fruit list equal to c (adversarial: the complete list).
 *   Pop: a moving snake s with target T pops iff len_s >= grow_to_s + 2 * fruits(T), formed without 32-bit overflow
 *     (grow_to of an installed state may be 2^31 - 1).
 *   Own post-move body: moving, B'_s = [T] followed by pieces 0 .. len_s - 1 - pop of the current body; standing, B'_s =
 *     the current body.
 *   Head-on set of another snake k in P: R_k = { head_k + d(k, b) : b in 0..4, d(k, b) != (0, 0) }, three cells for a
 *     snake in motion and four for a standing one.
 * fate_dev (may be NULL): uint8 [num_envs][S][5], entry [s][a], written for every snake whatever snake_mask is; a snake
 * not in P gets 0.  For s in P any combination of
 *   MSNAKE_FATE_WALL     T lies outside [0, dim)^2
 *   MSNAKE_FATE_SELF     T equals a piece i >= 1 of B'_s
 *   MSNAKE_FATE_BODY     T equals piece i of another k in P with i < len_k - 1, or with i == len_k - 1 and len_k < grow_to_k
 *   MSNAKE_FATE_HEAD_ON  T lies in R_k for some other k in P
 *   MSNAKE_FATE_TAIL     T equals the last piece of another k in P with len_k >= grow_to_k: a piece that goes only if k
 *                        moves and does not eat
 *   MSNAKE_FATE_EATS     the snake moves and fruits(T) > 0
 *   Cells are compared as coordinate pairs, -1 and dim included; duplicates count by piece index; there is no
 *   short-circuit: every bit that holds is set.  MSNAKE_FATE_CERTAIN = WALL | SELF | BODY, MSNAKE_FATE_RISK = HEAD_ON | TAIL.
 * by_dev (may be NULL): uint8 [num_envs][S][5]: bit k (0..3) is set iff HEAD_ON holds against snake k, bit 4 + k iff TAIL
 *   holds against snake k.
 * eat_dev (may be NULL): uint8 [num_envs][S][5]: min(255, fruits(T)) for a moving snake, else 0.
 * mask_dev (may be NULL): uint8 [num_envs][S][2]: [0] has bit a (0..4) set iff fate[s][a] & CERTAIN == 0 (the move can be
 *   survived), [1] iff fate[s][a] & (CERTAIN | RISK) == 0 (the move is survived whatever the others do); both are 0 for a
 *   snake not in P.
 * No output needs any alignment.
 * actions_dev: int32 [num_envs][action_stride]; entry s of every row is written for each s with bit s of snake_mask set,
 * all other entries are left untouched.  The policy wary_greedy: the action is 0 for a snake not in P; otherwise the
 * candidates are the a in 1..4 with bit a of mask[1] set, if there are none those with bit a of mask[0] set, and if there
 * are still none the action is 0; the action is the first candidate, in the order 1, 2, 3, 4, whose T(s, a) has the
 * strictly smallest L1 distance to any fruit of the state's fruit list (distance 0 when the list is empty): safe_greedy's
 * rule.
 * Guarantees, for one msnake_step from the state with snake s playing a, and for every choice of the other snakes' actions:
 *   1. fate & CERTAIN != 0  =>  s is dead after the step;
 *   2. fate & (CERTAIN | RISK) == 0  =>  s is alive after the step;
 *   3. HEAD_ON against k without a CERTAIN bit  =>  there is an action of k under which s dies;
 *   4. for snake 0, which moves first: whenever it survives, the step's reward equals fruits(T).
 * TAIL carries no such converse: a fruit that an earlier snake ate may respawn under k's head, so the bit is a named risk
 * and not a prediction.
 * Like its scripted siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in front of
 * the step.  Refusals, before any device work and in this order: MSNAKE_E_HANDLE for a NULL or destroyed handle;
 * MSNAKE_E_ARG for new_world rules (they judge one snake after the other and clear bodies as they go, see
 * msnake_death_causes); for a snake_mask bit >= n_snakes; for actions_dev NULL or action_stride < n_snakes when snake_mask
 * != 0; for nothing to write (snake_mask 0 and all four outputs NULL). */
#define MSNAKE_FATE_WALL 1
#define MSNAKE_FATE_SELF 2
#define MSNAKE_FATE_BODY 4
#define MSNAKE_FATE_HEAD_ON 8
#define MSNAKE_FATE_TAIL 16
#define MSNAKE_FATE_EATS 32
#define MSNAKE_FATE_CERTAIN (MSNAKE_FATE_WALL | MSNAKE_FATE_SELF | MSNAKE_FATE_BODY)
#define MSNAKE_FATE_RISK (MSNAKE_FATE_HEAD_ON | MSNAKE_FATE_TAIL)
int msnake_fate_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                        uint8_t* fate_dev, uint8_t* by_dev, uint8_t* eat_dev, uint8_t* mask_dev, void* stream);

/* The observation as cell codes, computed on the device from the current state of every env: what the reference's
 * frame (get_ob_for_snake / get_multi_snake_ob, snake_multiple_test.py:35-58,93-95) shows before its colour table is
 * applied.  The yardstick is the reference's frame, not msnake_render: the two frames agree on every state that play
 * reaches, but msnake_render paints a snake's body and head in one pass, so on a hand-installed state whose body has a
 * duplicate stacked on its own head cell it can show the body colour where the reference shows the head.
 * `views` is what the RGB frame has (C / 3 of msnake_obs_shape): 3 for snake_env and adversarial whatever n_snakes is,
 * n_snakes for new_world.
 * cells_dev: uint8 [num_envs][V][dim][dim], V = popcount(view_mask), the planes of the selected views in ascending view
 * order.  Plane entry [c0][c1] is cell (c0, c1), the cell that frame pixel [c0 + 1][c1 + 1] shows; there is no wall
 * border.  No alignment is required (a 19 x 19 plane is 361 bytes, so blocks start at odd addresses).  The codes in the
 * plane of view v:
 *   0 empty   1 fruit   2 body of snake v   3 head of snake v   4 body of another snake   5 head of another snake
 * Paint order, the frame's; a later paint wins: every entry of the state's fruit list first (adversarial: the complete
 * list); then, for snake i = 0, 1, ... in turn, all of its body cells (duplicates included), then its piece 0 as the
 * head.  A snake with an empty body paints nothing; under new_world a snake whose alive bit is 0 paints nothing; a
 * coordinate outside [0, dim)^2 (heads and adversarial fruits can sit at -1 or dim) paints nothing; in a view v >=
 * n_snakes every snake is "other".
 * Equivalence to the frame: decoding the obs_scale-1 RGB frame through the six-colour table (black 0; 255,0,0 fruit;
 * 0,204,0 / 191,242,191 own body / head; 0,51,204 / 128,154,230 another's body / head) and cutting off the wall border
 * gives these planes byte for byte.  The handle's obs_scale plays no part.
 * snakes_dev (may be NULL): int32 [num_envs][n_snakes][8], 4-byte aligned (MSNAKE_E_ALIGN otherwise); row s holds
 *   len, head c0, head c1, v0, v1, grow_to, alive, in_dead
 * of snake s, the values msnake_get_state returns in those words with piece 0 as the head; the head is (-2, -2) for an
 * empty body.  The rows are not rotated per view.
 * Like msnake_scripted_actions the call only reads the handle's state (no random numbers are drawn, the Philox counter
 * stays), allocates nothing, does not synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be
 * captured into a HIP graph behind a step.  MSNAKE_E_ARG, before any device work: a view_mask bit >= views; view_mask
 * != 0 with cells_dev NULL; view_mask == 0 with cells_dev non-NULL; nothing to write (view_mask 0 and snakes_dev NULL). */
int msnake_render_cells(msnake_handle h, uint32_t view_mask, uint8_t* cells_dev, int32_t* snakes_dev, void* stream);

/* Head-centred windows of cell codes, one per selected snake, computed on the device from the current state of every
 * env: a fixed-size cut of the planes of msnake_render_cells around a snake's head, optionally turned so that the snake
 * looks along the window's first axis.  The input is the same on every board size and, oriented, from every snake in
 * every direction.
 * Shapes: W = 2 * radius + 1, S = popcount(snake_mask).  windows_dev: uint8 [num_envs][S][W][W], the selected snakes in
 * ascending order.  heading_dev (may be NULL): uint8 [num_envs][S].  Neither needs any alignment (W * W is odd, so blocks
 * start at every address phase).
 * Heading k of snake s, from its velocity (v0, v1) in the canonical state: (1,0) -> 0, (0,1) -> 1, (-1,0) -> 2,
 * (0,-1) -> 3, (0,0) -> 0: the action that keeps the direction, minus 1.  heading_dev receives k whatever `oriented` is.
 * Let f be move k + 1 and g move ((k + 1) mod 4) + 1 of the move table (1..4 = (+1,0), (0,+1), (-1,0), (0,-1));
 * with oriented == 0, k is taken as 0 for the window, so f = (1,0) and g = (0,1).
 * Window entry [i][j] of snake s shows the cell head + (i - radius) * f + (j - radius) * g, where head is piece 0.  If
 * that cell lies in [0, dim)^2 the entry is the byte the plane of view s of msnake_render_cells holds there: 0..5 with
 * the same paint order (a later paint wins, a dead new_world snake paints nothing, duplicates are included); view s
 * exists here for every s < n_snakes under all three rule sets.  Otherwise the entry is MSNAKE_CELL_OUTSIDE.  The centre
 * [radius][radius] is the head's own cell: usually 3; on installed states it can be another code, or 6 for a head at -1
 * or dim.  A snake with an empty body gets W * W zeros and heading 0.
 * Relative actions: under oriented == 1, relative action r in 1..4 means forward (+f), the +g side, backward, the -g
 * side; it is the absolute action ((r - 1 + k) mod 4) + 1, and 0 stays 0.
 * Like msnake_render_cells the call only reads the handle's state (no random numbers are drawn, the Philox counter
 * stays), allocates nothing, does not synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be
 * captured into a HIP graph behind a step.  MSNAKE_E_ARG, before any device work: radius outside [1,
 * MSNAKE_LOCAL_MAX_RADIUS]; snake_mask 0 or with a bit >= n_snakes; oriented not 0 or 1; windows_dev NULL.
 * MSNAKE_E_HANDLE for a NULL handle. */
#define MSNAKE_LOCAL_MAX_RADIUS 31
#define MSNAKE_CELL_OUTSIDE 6 /* a window entry that lies outside the grid */
int msnake_render_local(msnake_handle h, int32_t radius, uint32_t snake_mask, int32_t oriented, uint8_t* windows_dev,
                        uint8_t* heading_dev, void* stream);

/* Eight-direction ray observations, one set per selected snake, computed on the device from the current state of every
 * env: from the head, look along eight directions and report per direction how far the wall is and how far the first
 * fruit, the first piece of the snake's own body and the first piece of another snake are.  32 bytes per snake: the
 * classic vector observation of snake agents, the input of a policy without convolutions.
 * Shapes: S = popcount(snake_mask).  rays_dev: uint8 [num_envs][S][MSNAKE_RAY_DIRS][MSNAKE_RAY_CHANNELS], the selected
 * snakes in ascending order; it must be 4-byte aligned (MSNAKE_E_ALIGN otherwise): one (snake, direction) entry is
 * exactly one dword.  heading_dev (may be NULL): uint8 [num_envs][S], no alignment; it receives exactly what
 * msnake_render_local writes there, whatever `oriented` is.
 * Directions: heading k of snake s and the unit steps f and g are those of msnake_render_local; with oriented == 0, k is
 * taken as 0 for the rays, so f = (1,0) and g = (0,1).  Direction j for j = 0, 2, 4, 6 is f, g, -f, -g; for j = 1, 3, 5,
 * 7 it is f + g, g - f, -f - g, f - g.  A diagonal step counts as one step.  Relative action r in 1..4 (see
 * msnake_render_local) looks along direction 2 (r - 1).
 * The walk: the ray of snake s in direction d visits head + t * d for t = 1, 2, ..., where head is piece 0.  Channel
 * MSNAKE_RAY_WALL is the smallest t >= 1 whose cell lies outside [0, dim)^2: at least 1 and at most 63 (a head at -1
 * looking across a board of 62).  The other three channels look only at the cells with t < wall, and there at the byte
 * the plane of view s of msnake_render_cells holds: the same paint order (a later paint wins, a dead new_world snake
 * paints nothing, duplicates are included, a fruit under a body is hidden).  MSNAKE_RAY_FRUIT is the smallest t with
 * code 1, MSNAKE_RAY_OWN the smallest t with code 2 or 3, MSNAKE_RAY_OTHER the smallest t with code 4 or 5; each is 0
 * when there is none.  Rays see through everything: the four channels are independent of each other.  The head's own
 * cell (t = 0) is not looked at.  A snake with an empty body gets 32 zeros and heading 0.
 * Identities: the oriented rays of a snake of heading k are its unoriented ones turned, rays_or[j] = rays_un[(j + 2 k)
 * mod 8].  For dim <= 30 every entry can be read off the radius-31 window of msnake_render_local with the same
 * `oriented`: walk from the centre [31][31] by (1,0), (1,1), (0,1), (-1,1), (-1,0), (-1,-1), (0,-1), (1,-1) for j = 0..7;
 * the first MSNAKE_CELL_OUTSIDE on the walk is the wall.
 * Like msnake_render_local the call only reads the handle's state (no random numbers are drawn, the Philox counter
 * stays), allocates nothing, does not synchronise and adds nothing to env_steps; asynchronous on `stream`, and it can be
 * captured into a HIP graph behind a step.  MSNAKE_E_ARG, before any device work: snake_mask 0 or with a bit >=
 * n_snakes; oriented not 0 or 1; rays_dev NULL.  MSNAKE_E_HANDLE for a NULL handle. */
#define MSNAKE_RAY_DIRS 8
#define MSNAKE_RAY_CHANNELS 4
#define MSNAKE_RAY_WALL 0
#define MSNAKE_RAY_FRUIT 1
#define MSNAKE_RAY_OWN 2
#define MSNAKE_RAY_OTHER 3
int msnake_render_rays(msnake_handle h, uint32_t snake_mask, int32_t oriented, uint8_t* rays_dev, uint8_t* heading_dev,
                       void* stream);

/* Per-snake outcomes of a step: which snake ate, which died, what every snake's reward was, and each snake's running
 * totals of the env's current episode.  msnake_step reports snake 0 only; this call, issued behind it, derives every
 * snake's outcome from two consecutive canonical states: the "before" facts are kept in a tracker that the caller owns,
 * the "after" facts are read from the handle's state.  S = n_snakes in every shape below.
 * Terms: grow_to(s) is snake s's grow_to word of the canonical state; alive(s) is len > 0 under snake_env and
 * adversarial and the alive word (the new_world alive bit) under new_world.  Under new_world a snake that hits itself
 * keeps its body and its alive bit is set again by the next step that finds it clear, so there a snake can "die" more
 * than once in one episode and come alive again.
 * The tracker: track_dev is int32 [num_envs][S][8], 4-byte aligned, owned by the caller; row [env][s] holds
 *   [0] grow_to  [1] alive  [2] ep_fruit  [3] ep_alive_steps  [4] first_death  [5] ep_steps  [6] ep_return (f32 bits)  [7] 0
 * words 0 and 1 being the facts of the state the row was last brought up to, words 2..6 the totals of the env's current
 * episode so far (see info_dev).
 * Arming, flags = MSNAKE_AGENT_ARM: every row is written from the current state, the five episode words and word 7
 * zero.  No outcome is produced: done_dev and the four outputs must be NULL.  A tracker needs arming before its first
 * use and after msnake_reset, msnake_set_state / msnake_set_state_all, msnake_copy_envs into the handle, a
 * msnake_reset_envs of an env that was not done, and any step that was not followed by an outcomes call.
 * Outcomes, flags = 0, issued behind each msnake_step on the same stream; done_dev is that step's done output (uint8
 * [num_envs], required).  For every env and snake s, with `before` = the tracker row and `after` = the state:
 *   ate   = max(0, grow_to after - grow_to before) >> 1     (every fruit eaten raises grow_to by 2)
 *   was   = row word 1 != 0,  now = alive(s) after,  died = was && !now,  ended = was && (died || done[env])
 * rew_dev (may be NULL): float32 [num_envs][S], 4-byte aligned: the rule set's own reward formula applied to snake s:
 *   snake_env and adversarial: died ? -1 : ate;  new_world: now ? -1 : ate (the reference's done = snake.alive, kept).
 *   On a step taken from an unfinished episode, column 0 equals that step's rew_dev bit for bit under all three rule sets.
 * ate_dev (may be NULL): uint8 [num_envs][S]: min(ate, 255); rew_dev and the totals are not clamped.
 * flags_dev (may be NULL): uint8 [num_envs][S]: MSNAKE_AGENT_ALIVE (now) | MSNAKE_AGENT_WAS_ALIVE (was) |
 *   MSNAKE_AGENT_DIED | MSNAKE_AGENT_ENDED.  WAS_ALIVE marks the (env, snake) samples a learner can use, ENDED the last
 *   one of a snake's life or episode.
 * info_dev (may be NULL): int32 [num_envs][S][4], 4-byte aligned: the totals of the env's current episode after this step,
 *   ep_fruit (sum of ate), ep_alive_steps (steps at whose end the snake was alive), first_death (1-based episode step
 *   of the snake's first death, 0 = none), ep_return (sum of rew, f32 bits).  On a done step: the episode's totals.
 * At least one of the four outputs must be given.  The tracker is then brought up to date: a row of an env with
 * done[env] == 0 receives the after-facts and the totals just reported; a row of an env with done[env] != 0 receives
 * what arming writes after a reset (grow_to 3, alive 1, totals 0), because the caller is expected to reset that env
 * before its next step -- msnake_reset_envs(h, done_dev, ...) on the same stream -- and the next call then needs no
 * arming.  The result is defined for any tracker contents and meaningful only for an armed one.
 * Like its siblings the call only reads the handle's state, draws no random numbers, allocates nothing, does not
 * synchronise and adds nothing to env_steps; asynchronous on `stream`, and [msnake_step, msnake_agent_outcomes,
 * msnake_reset_envs] can be captured into one HIP graph.  MSNAKE_E_ARG, before any device work: unknown flag bits;
 * track_dev NULL; arming with done_dev or an output non-NULL; outcomes with done_dev NULL or without any output; a
 * handle created with auto_reset = 1 (there the step has already replaced the after-state of a done env by a fresh
 * episode, so the terminal outcomes of snakes >= 1 cannot be known).  MSNAKE_E_ALIGN: track_dev, rew_dev or info_dev not
 * 4-byte aligned.  MSNAKE_E_HANDLE for a NULL handle. */
#define MSNAKE_AGENT_ARM 1        /* flags: write the tracker from the current state, produce no outcome */
#define MSNAKE_AGENT_ALIVE 1      /* flags_dev bits */
#define MSNAKE_AGENT_WAS_ALIVE 2
#define MSNAKE_AGENT_DIED 4
#define MSNAKE_AGENT_ENDED 8
int msnake_agent_outcomes(msnake_handle h, int32_t flags, int32_t* track_dev, const uint8_t* done_dev, float* rew_dev,
                          uint8_t* ate_dev, uint8_t* flags_dev, int32_t* info_dev, void* stream);

/* Scripted playouts: play every env on for up to n_steps steps with a fixed policy per snake, in ONE launch, and report
 * who ate, who died and where it ended -- the value of a position for a search over forks.  The call stands for
 * n_steps x [msnake_scripted_actions / msnake_fate_actions -> msnake_step -> msnake_agent_outcomes] on a scratch copy of
 * the handle, without the copy: the handle is only read.  It restates update_snake, is_snake_alive and step of the
 * reference (snake_multiple_test.py:97-197), iterated.  S = n_snakes in every shape below.
 * Rule set: snake_env handles only.  adversarial and new_world are MSNAKE_E_ARG (new_world judges its snakes one after
 * the other, as for msnake_death_causes; the adversarial fruit list can grow to fcap entries).
 * Per env, with s_0 its canonical state (the words of msnake_get_state):
 *   - if bit 8 of word 7 (`finished`) is set: steps = 0, end = MSNAKE_PLAYOUT_FINISHED, ret = 0, info = 0, and the end
 *     state is s_0;
 *   - otherwise, for k = 1, 2, ..., n_steps: the action of snake s in step 1 is first_dev[env][s] (row stride
 *     first_stride) if bit s of first_mask is set, taken exactly as msnake_step takes an action word, invalid codes
 *     included.  In any other step, or without that bit, it is policies[s] applied to s_(k-1), the very word the
 *     policy's own entry point would write: MSNAKE_POLICY_NONE the constant 0, MSNAKE_POLICY_SAFE_GREEDY and
 *     MSNAKE_POLICY_HAMILTONIAN what msnake_scripted_actions writes, MSNAKE_POLICY_WARY_GREEDY what msnake_fate_actions
 *     writes.  s_k is what one msnake_step makes of s_(k-1) on a handle with the same seed, the same global env id
 *     (env_id_base + index) and the same max_steps, with auto_reset = 0: the same Philox draws at the same counter, the
 *     same respawns, t, ep_len, ep_return, and `finished` once done.  The playout of an env stops behind the first step
 *     whose done is set.  The handle's own auto_reset plays no part: nothing is ever reset.
 * Per snake and played step, as msnake_agent_outcomes counts: was = len before > 0, died = was && len after == 0,
 * ate = max(0, grow_to after - grow_to before) >> 1, rew = died ? -1 : ate.
 * Outputs, each may be NULL but not all six:
 *   steps_dev int32 [num_envs]: the steps played.
 *   end_dev   uint8 [num_envs]: MSNAKE_PLAYOUT_HORIZON (n_steps played, the last one not done), _DEAD (the main snake
 *             died; it wins over _CAP when both hold), _CAP (t reached max_steps) or _FINISHED.
 *   ret_dev   float32 [num_envs][S]: the sum of rew; column 0 equals the sum of the steps' own rew_dev bit for bit.
 *   info_dev  int32 [num_envs][S][4]: the sum of ate (the death step's included, as ep_fruit), the number of steps at
 *             whose end the snake was alive, the 1-based playout step of its death (0 = none), and the action word it
 *             played in step 1 (0 when no step was played).
 *   words_dev int32 [num_envs][words_stride] and count_dev int32 [num_envs]: the end state, under exactly the contract
 *             of msnake_export_states: the count is always written, and no word of a row that does not fit is.  So
 *             msnake_import_states(scratch, ..., words_dev, ...) continues the game where the playout ended.
 * The handle is only read: record, rings, parked draws and draw counter stay byte for byte, env_steps and errors do not
 * move.  The call allocates nothing, never synchronises and can be captured into a HIP graph.  It works on any snake_env
 * handle, also one on a step kernel compiled for its shape, one holding a head outside the grid, and bodies in the
 * overflow ring.  The capacity rule of msnake_set_state holds inside the playout as in the step: a body that would pass
 * cap - 1 pieces drops its oldest piece; here it is not counted.
 * Refusals, before any device work, in this order: MSNAKE_E_HANDLE; MSNAKE_E_ARG for rules other than snake_env, n_steps
 * outside [1, MSNAKE_PLAYOUT_MAX_STEPS], policies NULL or policies[s] outside 0..3 for an s < S (entries s >= S are not
 * looked at), MSNAKE_POLICY_HAMILTONIAN on an odd board, a first_mask bit >= S, first_mask != 0 with first_dev NULL or
 * first_stride < S, words_dev with words_stride <= 0, all six outputs NULL; MSNAKE_E_ALIGN for an int32 or float pointer
 * that is not 4-byte aligned. */
#define MSNAKE_POLICY_WARY_GREEDY 3 /* msnake_playout only; msnake_scripted_actions keeps refusing it */
#define MSNAKE_PLAYOUT_MAX_STEPS 4096
#define MSNAKE_PLAYOUT_HORIZON 0  /* n_steps played, episode still running       */
#define MSNAKE_PLAYOUT_DEAD 1     /* the main snake died                         */
#define MSNAKE_PLAYOUT_CAP 2      /* t reached max_steps, main snake alive       */
#define MSNAKE_PLAYOUT_FINISHED 3 /* the start state had `finished` set: 0 steps */
int msnake_playout(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES], int32_t n_steps, const int32_t* first_dev,
                   int32_t first_stride, uint32_t first_mask, int32_t* steps_dev, uint8_t* end_dev, float* ret_dev,
                   int32_t* info_dev, int32_t* words_dev, int32_t words_stride, int32_t* count_dev, void* stream);

/* Exploring play: with a probability per snake, a uniformly random legal move in place of the policy's own, drawn from a
 * documented stream of its own -- inside the one-launch playout (msnake_playout_explore: Monte-Carlo rollouts without
 * leaving the device) and as the standalone call that writes the very word such a playout plays (msnake_explore_actions:
 * what a search assumes about an opponent can be played against it, captured in a graph, with no host RNG).
 * The exploration rule.  S = n_snakes.  policies[s] is in 0..3 as msnake_playout takes them; eps_q16[s] is in [0, 65536]
 * and is snake s's exploration probability in units of 1 / 65536; salt is any uint64.  For an env with global id
 * G = env_id_base + e whose canonical state has t = word 0 and ctr = words 1, 2 as one uint64:
 *   Base action: b_s is what policies[s] writes for that state: MSNAKE_POLICY_NONE the constant 0, MSNAKE_POLICY_SAFE_GREEDY
 *     and MSNAKE_POLICY_HAMILTONIAN what msnake_scripted_actions writes, MSNAKE_POLICY_WARY_GREEDY what msnake_fate_actions
 *     writes.
 *   Candidate set C_s, moves in 1..4: under MSNAKE_POLICY_WARY_GREEDY wary_greedy's own candidates -- the a in 1..4 with bit a
 *     of mask[1] set, and if there are none those with bit a of mask[0] set (msnake_fate_actions' mask_dev); under every
 *     other policy the open moves, bits 1..4 of msnake_scripted_actions' safe_dev byte.  An empty body gives an empty set.
 *     n = |C_s|.
 *   The stream never touches the env's own.  xseed = mix64(seed ^ mix64(salt ^ 0x6578706C6F726521)) ("explore!"), mix64 the
 *     splitmix64 finaliser (see msnake_hash_states), seed the handle's.  k64 = mix64(xseed ^ ctr).  Draw j is word (j & 3)
 *     of Philox4x32-10(counter = {lo(j >> 2), hi(j >> 2), lo(G), hi(G)}, key = {lo(k64), hi(k64)}) -- the RNG contract at the
 *     top of this file under another key.  For snake s: u0 = draw 8 t + 2 s and u1 = draw 8 t + 2 s + 1, with t zero-extended
 *     from uint32.
 *   The action: if eps_q16[s] > 0, (u0 >> 16) < eps_q16[s] and n > 0, the snake explores: its action is the
 *     ((u1 * n) >> 32)-th member of C_s in the order 1, 2, 3, 4.  Otherwise it is b_s.  eps_q16 = 65536 always explores when
 *     n > 0 (a uniform random legal mover); eps_q16 = 0 never draws.
 * The draw depends on (seed, salt, G, t, ctr, s) only: it is stateless, a shard draws what the unsharded handle draws for
 * the same global ids, and nothing in the arguments has to change between the replays of a graph.  It does not repeat over
 * an env's life: ctr only grows, and t grows between two changes of ctr.
 *
 * msnake_explore_actions: entry s of every row of actions_dev (int32 [num_envs][action_stride]) is written for each s with
 * bit s of snake_mask set, all other entries are left untouched.  explored_dev (may be NULL): uint8 [num_envs][S], written
 * for every snake whatever snake_mask is: 1 iff that snake's action was drawn.  All three rule sets for policies 0..2;
 * MSNAKE_POLICY_WARY_GREEDY needs snake_env or adversarial, as msnake_fate_actions does.  Like its siblings the call only
 * reads the handle's state, draws none of the env's random numbers (the Philox counter stays), allocates nothing, never
 * synchronises and adds nothing to env_steps; asynchronous on `stream`, and it can be captured into a HIP graph in front of
 * the step.  Refusals, before any device work, in this order: MSNAKE_E_HANDLE; MSNAKE_E_ARG for policies NULL or
 * policies[s] outside 0..3 for an s < S; for MSNAKE_POLICY_WARY_GREEDY on a new_world handle; for MSNAKE_POLICY_HAMILTONIAN
 * on an odd board; for eps_q16 NULL or an entry > 65536 for an s < S; for snake_mask 0 or with a bit >= S; for actions_dev
 * NULL or action_stride < S; MSNAKE_E_ALIGN for actions_dev not 4-byte aligned.
 *
 * msnake_playout_explore: the contract of msnake_playout word for word, with one change: the action of snake s in step k is
 * the rule above applied to s_(k-1), with that state's t and ctr -- the draw counter moves with the respawns inside the
 * playout, as it does there.  A forced first action wins over exploring; info[..][3] reports the word played, explored or
 * not.  Refusals: msnake_playout's list, with "eps_q16 NULL or an entry > 65536 for an s < S" directly behind "policies NULL
 * or policies[s] outside 0..3" and in front of the odd board.  msnake_playout(h, ...) is msnake_playout_explore with every
 * eps 0, for any salt. */
int msnake_explore_actions(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES],
                           const uint32_t eps_q16[MSNAKE_MAX_SNAKES], uint64_t salt, uint32_t snake_mask,
                           int32_t* actions_dev, int32_t action_stride, uint8_t* explored_dev, void* stream);
int msnake_playout_explore(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES],
                           const uint32_t eps_q16[MSNAKE_MAX_SNAKES], uint64_t salt, int32_t n_steps,
                           const int32_t* first_dev, int32_t first_stride, uint32_t first_mask, int32_t* steps_dev,
                           uint8_t* end_dev, float* ret_dev, int32_t* info_dev, int32_t* words_dev, int32_t words_stride,
                           int32_t* count_dev, void* stream);

/* Random legal positions, built on the device: for the envs a mask selects, non-overlapping snakes of the body lengths the
 * caller asks for and fruits off the bodies, as canonical words (see msnake_get_state) that msnake_import_states installs
 * or an archive tensor keeps.  Exploring starts in the sense of ALE, batched: the late game as a place to start from.
 * snake_env and adversarial handles; new_world is MSNAKE_E_ARG (its alive and in_dead bookkeeping and its init draws are
 * another contract).  S = n_snakes, F = the handle's n_fruits.
 * The handle is only read -- its configuration and, per env, the draw counter and word 3: record, rings, parked draws,
 * draw counter, env_steps and errors stay byte for byte.  The call allocates nothing, never synchronises and can be
 * captured into a HIP graph.
 * mask_dev: uint8 [num_envs], non-zero = selected, NULL = every env.  For an unselected env nothing is written: not a byte
 *   of its row, its count or its got.
 * len_dev: int32 [num_envs][len_stride], required, len_stride >= S: the requested body length of each snake.  A request
 *   below 0 counts as 0; snake 0's request is raised to 1; a request of 0 gives an empty (dead) snake.
 * words_dev int32 [num_envs][stride] and count_dev int32 [num_envs]: the contract of msnake_export_states.  The count of a
 *   selected env is always written; if it exceeds stride, no word of that row is.
 * got_dev (may be NULL): int32 [num_envs][S], the lengths actually reached.
 * The generator's random stream never touches the env's own.  gseed = mix64(seed ^ mix64(salt ^ 0x67656E6572617465)), mix64
 * the splitmix64 finaliser (see msnake_hash_states), seed the handle's.  Draw j = 0, 1, 2, ... of the env with global id
 * G = env_id_base + e is word (j & 3) of Philox4x32-10(counter = {j >> 2, G}, key = gseed) -- the RNG contract at the top
 * of this file under another key -- and randint(n) = (u32 * n) >> 32.  So a shard generates exactly the rows the unsharded
 * handle generates for the same global ids.
 * The position of one selected env: start with an empty occupancy; draws are consumed in this order.
 *   For snake s = 0 .. S-1 with request L > 0:
 *     Head: let nfree be the number of unoccupied cells.  nfree == 0: the snake gets length 0, no draw.  Otherwise k =
 *       randint(nfree), one draw, and the head is the k-th unoccupied cell in the order x = c1 * dim + c0 (the respawn's).
 *       Occupy it.
 *     Body: it grows behind the head; `end` is the last piece laid.  While len < L: the candidates are the unoccupied
 *       in-grid neighbours of `end`, in the order of actions 1..4: (+1,0), (0,+1), (-1,0), (0,-1).  None: stop, the snake
 *       stays shorter and got says so.  With MSNAKE_GEN_COMPACT, keep only the candidates with the fewest unoccupied
 *       in-grid neighbours of their own, in the same order (Warnsdorff's rule: what makes long bodies reachable).  With n
 *       candidates left, take candidate n == 1 ? 0 : randint(n) -- a draw only when n > 1 --, occupy it, append it.
 *   Then for fruit f = 0 .. F-1: count the cells occupied by no body and no earlier fruit.  None: the fruit is (0, 0), no
 *     draw.  Otherwise it is the k-th such cell by one draw.
 *   Words: [0] t = 0; [1], [2] the env's current draw counter; [3] the env's current word 3 (adversarial keeps
 *     spare_fruits across a reset; so does this); [4] 0; [5] 0; [6] F; [7] n_snakes, `finished` clear; the fruits; then per
 *     snake len, v0, v1, grow_to = max(len, 3), alive = 1, in_dead = 0 and the cells head first, (v0, v1) = head - piece 1,
 *     (0, 0) for len <= 1.
 * Every generated row lies in the acceptance domain of msnake_set_state; the heads are inside the grid, so handles on a
 * step kernel compiled for their shape take them.
 * Refusals, before any device work, in this order: MSNAKE_E_HANDLE; MSNAKE_E_ARG for new_world, a flag bit other than
 * MSNAKE_GEN_COMPACT, len_dev NULL or len_stride < S, words_dev with stride <= 0, words_dev, count_dev and got_dev all
 * NULL; MSNAKE_E_ALIGN for an int32 pointer that is not 4-byte aligned. */
#define MSNAKE_GEN_COMPACT 1u
int msnake_generate_states(msnake_handle h, const uint8_t* mask_dev, const int32_t* len_dev, int32_t len_stride,
                           uint32_t flags, uint64_t salt, int32_t* words_dev, int32_t stride, int32_t* count_dev,
                           int32_t* got_dev, void* stream);

/* Copy the aggregate statistics to the host.  Blocking: waits for the device (every step issued so
 * far, on any stream) before it sums the per-env totals.  episodes / ep_len_sum / ep_return_sum /
 * errors are accumulated on the device; env_steps is counted on the host per API call, so replays
 * of a captured HIP graph are not included in it. */
int msnake_get_stats(msnake_handle h, msnake_stats* out, int32_t reset);

/* Name of the step kernel that msnake_step launches of this handle run with action_stride == n_snakes (for
 * profilers; the string is owned by the handle and lives until msnake_destroy) and algorithmic HBM bytes per
 * env-step.  Handles of the shapes 19x19 with 2 or 3 snakes and 10x10 with one snake (snake_env rules,
 * obs_scale 1, auto reset, the full record) run kernels compiled for that shape, named with a fifth template
 * argument, the board size; a call whose action_stride differs runs the generic kernel for that call, with the same
 * results.  So does, from then on, a handle that msnake_set_state / msnake_set_state_all gave a head outside the grid, or
 * that msnake_copy_envs filled from such a handle: only the generic kernels draw the wall over a body piece that such a
 * snake leaves outside the grid when it turns back in (no state that play reaches has one). */
const char* msnake_kernel_name(msnake_handle h);
/* The same name for a configuration, decided on the host exactly as msnake_create decides it, without a handle and
 * without touching a GPU (tests, tools).  Writes at most n bytes, NUL-terminated; MSNAKE_E_ARG for a configuration
 * msnake_create would refuse. */
int msnake_kernel_name_for_config(const msnake_config* cfg, char* out, size_t n);
/* Process-wide switch for same-box A/B runs and tests: while it is on, msnake_create (and the call above) choose the
 * generic kernels for every configuration; handles that exist keep what they were created with.  Returns the previous
 * setting.  The library itself reads no environment variable: the Python binding turns the switch on for handles
 * created while MSNAKE_GENERIC_KERNELS=1 is in the environment.  Not for concurrent use: the switch is one
 * process-wide value, so a thread that flips it while another thread is inside msnake_create (or the call above)
 * decides which kernels that handle gets; callers that create handles from several threads set it once, before. */
int msnake_set_generic_kernels(int32_t on);
/* Which per-step kernel ONE msnake_step call of a handle with this configuration runs, decided on the host exactly as
 * the launch glue decides it per call, without a handle and without touching a GPU (tests, tools): the pointers are
 * only looked at, never dereferenced.
 *   MSNAKE_CALL_GENERIC  the generic kernel: the configuration has no compile-time shape, the generic kernels are
 *                        switched on, or action_stride differs from n_snakes
 *   MSNAKE_CALL_SHAPE    the kernel compiled for the shape
 *   MSNAKE_CALL_PLAIN    its "plain call" variant: obs, rew, done and info are all given, obs_dev sits on a 128-byte
 *                        line and num_envs * (observation bytes per env) < 2^31, so the kernel tests no pointer, forms
 *                        every output address from a 32-bit offset and derives the layout of its observation stores
 *                        from the env index alone.  Same results, bit for bit.
 * msnake_kernel_name reports the same name for the last two.  MSNAKE_E_ARG for a configuration msnake_create would
 * refuse or an action_stride msnake_step would refuse. */
#define MSNAKE_CALL_GENERIC 0
#define MSNAKE_CALL_SHAPE 1
#define MSNAKE_CALL_PLAIN 2
int msnake_call_shape_for_config(const msnake_config* cfg, int32_t action_stride, const void* obs_dev, const void* rew_dev,
                                 const void* done_dev, const void* info_dev, int32_t* out);
/* How the launches of a handle with this configuration are laid out, decided on the host exactly as msnake_create and
 * msnake_rollout_tape decide it, without a handle and without touching a GPU (tests, tools).  *step_epb: envs (=
 * wavefronts) per workgroup of msnake_step's launches -- 8 up to 8 192 envs and 4 above, halved until that many LDS
 * images (padded observation + occupancy bytes) fit 64 KB, and never above envs_per_block.  *tape_epb: the same for
 * msnake_rollout_tape's persistent launch, whose image is twice as large at obs_scale 1; 0 where not even one env fits,
 * and the call runs per-step launches.  Either pointer may be NULL.  MSNAKE_E_ARG for a configuration msnake_create
 * would refuse.  Never a result: every value gives the same outputs. */
int msnake_launch_shape_for_config(const msnake_config* cfg, int32_t* step_epb, int32_t* tape_epb);
int64_t msnake_algorithmic_bytes_per_env_step(msnake_handle h);

#ifdef __cplusplus
}
#endif
#endif /* MSNAKE_H */
