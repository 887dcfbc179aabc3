// msnake_internal.h -- shared between the kernels and the C-ABI glue (not installed).
#ifndef MSNAKE_INTERNAL_H
#define MSNAKE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/msnake.h"

// One wavefront per env; up to 8 envs (512 threads) per workgroup, no workgroup barrier anywhere.
#define MSNAKE_BLOCK_THREADS 512
#define MSNAKE_MAX_ENVS_PER_BLOCK 8

// Per-env record in HBM: a 256-byte slot of 64 dwords (lane l <-> word l), loaded/stored by ONE
// coalesced wave instruction; snake_env / adversarial keep everything a step needs in the FIRST 128
// bytes, so large batches move only that half (StepParams::short_rec).  Next to it, per snake, a
// 128-byte RING of its 64 most recent body cells (slot l <-> lane l; piece i < min(len, 64) sits in
// slot (hp0 + i) & 63), and, only for bodies longer than 64 cells, an overflow ring with the older
// pieces (piece i >= 64 at ovf[(ohp + i - 64) % cap]).  Record and body rings sit at addresses that
// depend only on the env index: one memory round trip per step.  A step dirties the record, ONE
// 32-byte sector per moving snake (the sector that holds the new head slot) and the outputs.
#define MSNAKE_HDR_WORDS 64
#define MSNAKE_HDR_SHORT_WORDS 32
// words 0..11: three 4-lane "columns" so that lane s of a DPP row shift holds snake s's field
#define SN_A(s) (0 + (s))   // overflow ring head pos ohp | len << 16
#define SN_B(s) (4 + (s))   // grow_to ([S] grow_to_lengths / [N] Snake.snake_length)
#define SN_C(s) (8 + (s))   // head cell | velocity code << 16 | hp0 (body ring slot of the head) << 24
#define SN_C_HP0_SHIFT 24
#define HDR_T 12         // steps since reset ([S] state[4] / [NE] current_step)
#define HDR_CTR_LO 13    // Philox draws consumed (64 bit)
#define HDR_CTR_HI 14
#define HDR_FLAGS 15     // [N] bit s: Snake.alive, bit 4+s: snake in World.dead_snakes; all rules bit 8:
                         // the episode has ended and the env has not been reset since (auto_reset off)
#define HDR_FLAG_FINISHED 0x100u
#define HDR_EP_RETURN 16 // Monitor: running episode return (f32 bits)
#define HDR_EP_LEN 17    // Monitor: running episode length
#define HDR_SPARE 18     // [A] spare_fruits
#define HDR_NLIST 19     // [A] length of the fruit list
#define HDR_FRUIT0_S 20  // snake_env: words 20..22 = fruit f's cell (one fruit per snake, at most 3)
#define HDR_ACC_EPISODES 24  // per-env totals since the last msnake_get_stats(reset=1): no hot-path atomics
#define HDR_ACC_LEN 25       // low word; the carry goes to HDR_ACC_LEN_HI
#define HDR_ACC_RETURN 26    // int32, rewards are integral
#define HDR_ACC_ERRORS 27
#define HDR_ACC_LEN_HI 28
#define HDR_FRUIT0_N 32  // new_world: words 32+f = fruit f's cell (up to 32 fruits; always the full record)
// snake_env / adversarial, full record only: the upper half carries the next Philox draws, so the
// waves that respawn a fruit or reset -- the last ones to finish in a launch -- rarely have to
// evaluate Philox themselves.  Worth its 256 bytes per env-step only while launches are latency
// bound (small batches); with short_rec the words are neither loaded nor stored.
#define HDR_PC_VALID 35  // 1: words 37..63 hold the u32 of draws [PC_BASE, PC_BASE + 27)
#define HDR_PC_BASE 36   // low 32 bits of the first cached draw's index
#define HDR_PC_FIRST 37
#define HDR_PC_N 27

// native-size handles keep 16 pre-shifted copies of the background image (copy s: the image starts s bytes into its
// buffer), for the aligned copy-out of the step kernel; fused x4 / x7 handles keep one
#define MSNAKE_TMPL_COPIES 16

#define MSNAKE_NO_CELL 0xFFFFu  // never equals a real cell (rows/cols <= 63)

// why msnake_state_unpack_kernel rejects an env (state_reason() in msnake_capi.hip has the texts)
enum {
    MSNAKE_ST_SHORT = 1,   // buffer too short / truncated
    MSNAKE_ST_SNAKES = 2,  // snake count differs from the handle
    MSNAKE_ST_FRUITS = 3,  // fruit count differs from the handle / exceeds the list capacity
    MSNAKE_ST_CELL = 4,    // a cell outside [-1, dim]
    MSNAKE_ST_LEN = 5,     // a body length outside [0, cap - 2]
    MSNAKE_ST_SCALAR = 6   // a scalar field out of range: t, spare_fruits, ep_len, grow_to, a velocity, alive / in_dead
};
// msnake_import_states publishes them as they are (its status bytes)
static_assert(MSNAKE_ST_SHORT == MSNAKE_STATE_TOO_SHORT && MSNAKE_ST_SNAKES == MSNAKE_STATE_SNAKE_COUNT &&
              MSNAKE_ST_FRUITS == MSNAKE_STATE_FRUIT_COUNT && MSNAKE_ST_CELL == MSNAKE_STATE_CELL &&
              MSNAKE_ST_LEN == MSNAKE_STATE_LENGTH && MSNAKE_ST_SCALAR == MSNAKE_STATE_SCALAR && MSNAKE_STATE_OK == 0, "public reason codes");

#define MSNAKE_HD __host__ __device__ __forceinline__ constexpr

namespace msnake {

// ------------------------------------------------------------------------------------------------
// The shape numbers and the sections of the state allocation: THE definition, for the host glue (derive_shape,
// msnake_create, spec_dim_of, launch_k) and for the kernels alike.
// ------------------------------------------------------------------------------------------------
namespace shape {
MSNAKE_HD int obs_bytes(int dim, int C) { return (dim + 2) * (dim + 2) * C; }  // S: the wall ring included
MSNAKE_HD int ring_cap(int need) { return (need + 63) & ~63; }  // overflow ring: `need` cells (dim^2 + 2, new_world max_steps + 2) in whole waves
// LDS image, K-fold wide, in whole 1 KiB wave-instructions (native size: + room for the image's shift of up to 15 bytes)
MSNAKE_HD int img_bytes(int S, int K) { return (S * K + (K == 1 ? 15 : 0) + 1023) & ~1023; }
MSNAKE_HD int occ_bytes(int n2) { return (n2 + 15) & ~15; }  // respawn occupancy behind the image
// LDS per env: the image being composed, the occupancy, and (the tape kernel at native size) the pristine background
MSNAKE_HD int lds_per_wave(int img, int n2, bool ldsbg) { return img + occ_bytes(n2) + (ldsbg ? img : 0); }
// LDS one workgroup may use, and the envs (= waves) per workgroup that fit it: `epb` halved until epb * per_wave fits,
// 0 when one env alone does not.  THE arithmetic of msnake_create (per-step launches: lds_per_wave(.., false)), of
// launch_k (the persistent tape kernel at native size: lds_per_wave(.., true)) and of msnake_rollout_tape, which
// decides with it before any launch whether the persistent kernel can serve the handle at all.
constexpr int kLdsBytes = 64 * 1024;
MSNAKE_HD int epb_that_fits(int epb, int per_wave) {
    while (epb > 1 && (long long)epb * per_wave > kLdsBytes) epb >>= 1;
    return per_wave > kLdsBytes ? 0 : epb;
}
// envs per workgroup of the persistent tape launch of a handle whose per-step launches run `epb`; 0 = no such launch.
// A fused frame (K > 1) keeps no background copy: the image alone, as in the per-step kernel.
MSNAKE_HD int tape_epb(int epb, int img, int n2, int K) { return epb_that_fits(epb, lds_per_wave(img, n2, K == 1)); }
MSNAKE_HD int fruit_cap(int ns, int n2) { return (ns + ns * (n2 + 2) + 63) & ~63; }  // [A] list: n fruits + every body of one episode
MSNAKE_HD int fixed_bytes(int ns) { return MSNAKE_HDR_WORDS * 4 + ns * 128; }  // per env: record + the 64-slot ring of every snake

// byte offsets into the ONE allocation [hdr | body0 | tmpl | ovf | fl0 | flist]; fl0 and flist are empty unless adversarial
struct Sections { size_t hdr, body0, tmpl, ovf, fl0, flist, total; };
MSNAKE_HD Sections sections(int nenv, int ns, size_t tmpl_bytes, int cap, int fcap, int rules) {
    const size_t n = (size_t)nenv, adv = rules == MSNAKE_RULES_ADVERSARIAL ? 1 : 0;
    const size_t tmpl = n * (size_t)fixed_bytes(ns), ovf = tmpl + tmpl_bytes, fl0 = ovf + n * ns * cap * 2, flist = fl0 + adv * n * 128;
    return Sections{0, n * (MSNAKE_HDR_WORDS * 4), tmpl, ovf, fl0, flist, flist + adv * n * fcap * 2};
}

// the compile-time shapes of the step kernel, and one layout by hand
static_assert(obs_bytes(19, 9) == 3969 && img_bytes(3969, 1) == 4096 && ring_cap(19 * 19 + 2) == 384 && occ_bytes(361) == 368, "19x19x9");
static_assert(lds_per_wave(4096, 361, false) == 4464 && lds_per_wave(4096, 361, true) == 8560 && fruit_cap(3, 361) == 1152 && fruit_cap(2, 361) == 768, "19x19x9");
static_assert(obs_bytes(10, 9) == 1296 && img_bytes(1296, 1) == 2048 && ring_cap(10 * 10 + 2) == 128 && occ_bytes(100) == 112, "10x10x9");
static_assert(lds_per_wave(2048, 100, false) == 2160 && fruit_cap(1, 100) == 128 && img_bytes(3969, 4) == 16384, "10x10x9, fused x4");
// the last boards whose persistent tape launch exists: 56x56 with 9 channels, 48x48 with 12 (new_world, 4 snakes)
static_assert(tape_epb(8, img_bytes(obs_bytes(56, 9), 1), 56 * 56, 1) == 1 && tape_epb(8, img_bytes(obs_bytes(57, 9), 1), 57 * 57, 1) == 0, "tape limit, 9 channels");
static_assert(tape_epb(8, img_bytes(obs_bytes(48, 12), 1), 48 * 48, 1) == 1 && tape_epb(8, img_bytes(obs_bytes(49, 12), 1), 49 * 49, 1) == 0, "tape limit, 12 channels");
static_assert(epb_that_fits(8, lds_per_wave(4096, 361, false)) == 8 && tape_epb(8, 4096, 361, 1) == 4 && tape_epb(2, img_bytes(3969, 4), 361, 4) == 2, "19x19x9");
static_assert(fixed_bytes(3) == 640 && fixed_bytes(MSNAKE_MAX_SNAKES) == 768, "record + rings");
constexpr Sections kPinned = sections(2, 3, 16 * 4096, 384, 1152, MSNAKE_RULES_ADVERSARIAL);
static_assert(kPinned.hdr == 0 && kPinned.body0 == 512 && kPinned.tmpl == 1280 && kPinned.ovf == 66816 && kPinned.fl0 == 71424 &&
              kPinned.flist == 71680 && kPinned.total == 76288, "2 adversarial envs, 3 snakes, 19x19");
static_assert(sections(2, 3, 16 * 4096, 384, 1152, MSNAKE_RULES_SNAKE_ENV).total == 71424, "no fruit list: the rings end the allocation");
}  // namespace shape

// ------------------------------------------------------------------------------------------------
// The codes the state is written in.  A cell: 16 bits, (row << 8) | col in PADDED observation coordinates, row = c0 + 1,
// col = c1 + 1, so the grid is 1..dim and one step outside lands on the wall ring 0 / dim + 1.  A velocity: 0 = at rest,
// 1..4 = (1, 0), (0, 1), (-1, 0), (0, -1) -- action m + 1 keeps moving by move m's delta.
// ------------------------------------------------------------------------------------------------
// (The same as macros, for three sites whose instructions change when the expression goes through a function: the
//  painters of msnake_space.inc and msnake_local.inc, and the one encoder of velocities, msnake_state_unpack_kernel.)
#define MSNAKE_CELL_C0(c) ((int)((c) >> 8) - 1)
#define MSNAKE_CELL_C1(c) ((int)((c) & 255u) - 1)
#define MSNAKE_VEL_CODE(v0, v1) \
    (((v0) == 1 && (v1) == 0) ? 1 : ((v0) == 0 && (v1) == 1) ? 2 : ((v0) == -1 && (v1) == 0) ? 3 : ((v0) == 0 && (v1) == -1) ? 4 : 0)
MSNAKE_HD uint32_t cell_pack(int c0, int c1) { return ((uint32_t)(c0 + 1) << 8) | (uint32_t)(c1 + 1); }
MSNAKE_HD int cell_c0(uint32_t c) { return MSNAKE_CELL_C0(c); }
MSNAKE_HD int cell_c1(uint32_t c) { return MSNAKE_CELL_C1(c); }
MSNAKE_HD int vel_v0(int vel) { return vel == 1 ? 1 : vel == 3 ? -1 : 0; }
MSNAKE_HD int vel_v1(int vel) { return vel == 2 ? 1 : vel == 4 ? -1 : 0; }
MSNAKE_HD int move_d0(int m) { return m == 0 ? 1 : m == 2 ? -1 : 0; }  // move m = action m + 1
MSNAKE_HD int move_d1(int m) { return m == 1 ? 1 : m == 3 ? -1 : 0; }
static_assert(cell_pack(-1, 18) == 19 && cell_c0(cell_pack(7, 0)) == 7 && cell_c1(cell_pack(7, 0)) == 0, "cell code");
static_assert(MSNAKE_VEL_CODE(vel_v0(3), vel_v1(3)) == 3 && MSNAKE_VEL_CODE(move_d0(1), move_d1(1)) == 2 && MSNAKE_VEL_CODE(0, 0) == 0, "velocity code");

// the alive / in_dead words of the canonical state and of msnake_render_cells' table, out of HDR_FLAGS (only new_world
// keeps the bits: elsewhere a snake is alive and not in dead_snakes)
MSNAKE_HD int32_t snake_alive(uint32_t flags, int s, bool nw) { return nw ? (int32_t)((flags >> s) & 1u) : 1; }
MSNAKE_HD int32_t snake_in_dead(uint32_t flags, int s, bool nw) { return nw ? (int32_t)((flags >> (4 + s)) & 1u) : 0; }

// msnake_set_state's status word: (local env index + 1) in bits 8.., the MSNAKE_ST_* reason below (ONE atomicMin on ~0u
// gives index and reason of the first rejected env)
MSNAKE_HD uint32_t status_pack(int local, int reason) { return (((uint32_t)local + 1u) << 8) | (uint32_t)reason; }
MSNAKE_HD int status_env(uint32_t st) { return (int)(st >> 8) - 1; }
MSNAKE_HD uint32_t status_reason(uint32_t st) { return st & 0xFFu; }

// kernel arguments that did not fit the 13 preloaded dwords, passed by value behind them
struct StepRest {
    msnake_info* info;           // per-call output (may be NULL)
    float* rew;                  // (host copy; the kernel gets these two preloaded)
    uint8_t* done;
    uint64_t env_id_base;
    uint32_t seed_lo, seed_hi;
    int32_t cap;                 // overflow ring capacity in cells (multiple of 64)
    int32_t max_steps;
    uint32_t dbg_stage;          // timing-only early exits (MSNAKE_DBG_STAGES builds)
    unsigned long long* dbg_buf; // MSNAKE_DBG_STAGES builds: [nenv][8] s_memrealtime stamps (MSNAKE_DBG_BUF)
    unsigned long long* dbg_span; // MSNAKE_DBG_STAGES builds: this launch's [nenv][8] wave stamps (see SPAN in the kernel;
                                  // MSNAKE_DBG_SPAN = base of [slots][nenv][8], one slot per launch)
    int32_t n_steps;             // MODE 3 (msnake_rollout_tape): steps per launch
    uint64_t obs_step_stride;    // MODE 3: bytes between consecutive steps' observations (0 = overwrite)
    uint64_t scalar_step_stride; // MODE 3: elements between consecutive steps' rew/done/info
    uint32_t stream_obs;         // (host copy; the kernel gets it in pk2)
    // appended behind the fields above, so their offsets (and the preloaded arguments) stay put
    const uint8_t* env_mask;     // MODE 1 / 2 (msnake_reset_envs): non-NULL -> only envs with env_mask[e] != 0 are reset / rendered
    uint8_t* truncated;          // MODE 1 (msnake_reset_envs): per env, 1 = the episode was cut by max_steps (may be NULL)
};

// pk2: flag bits preloaded with the other kernel arguments
#define PK2_SHORT_REC 1u   // move only the first 128 bytes of each record
#define PK2_STREAM_OBS 2u  // observation stores carry the nt (streaming) hint (fused frames: the flat 16-byte copy-out)
#define PK2_STREAM_TAPE 4u // same for the persistent tape kernel (msnake_rollout_tape)
#define PK2_TAPE_ALIGNED 8u // msnake_rollout_tape: the step stride is a multiple of 16 bytes -> aligned copy-out for every step
#define PK2_EPB_SHIFT 8    // bits 8..15: envs (waves) per workgroup
#define PK2_DIVM_SHIFT 16  // bits 16..31: the multiplier of the division-free x / dim (slow paths)

struct StepParams {
    // configuration
    int32_t nenv, dim, n_snakes, n_fruits, views, C, S, auto_reset;
    int32_t lds_per_wave;  // bytes of LDS per env: padded image + occupancy bytes
    int32_t img_bytes;     // S rounded up to 1 KiB
    int32_t action_stride;
    int32_t obs_scale;     // fused WarpFrame replication factor (1, 4 or 7)
    int32_t short_rec;     // 1: the step moves only the first 128 bytes of each record
    int32_t stream_tape;   // 1: msnake_rollout_tape stores observations with the nt hint (set per call)
    int32_t spec_dim;      // != 0: the handle's step / tape launches use the compile-time shape msnake_step_kernel<.., spec_dim>
                           // (decided once by msnake_create: spec_dim_of; 0 = the generic kernels)
    // state (HBM, owned by the handle): ONE allocation
    //   [hdr: nenv x 256 B][body0: nenv x n_snakes x 128 B][tmpl: img_bytes][ovf: nenv x n_snakes x cap x 2 B]
    //   adversarial only: [fl0: nenv x 128 B][flist: nenv x fcap x 2 B] (fruit list chunk 0 / complete)
    uint8_t* state;
    uint32_t* hdr;               // views into `state` for the host-side paths
    uint16_t* body0;             // per snake: ring of the 64 most recent cells
    const uint8_t* tmpl;
    uint16_t* ring;              // per snake: overflow ring, pieces >= 64
    uint16_t* fl0;               // adversarial: first 64 fruit-list entries per env
    uint16_t* flist;             // adversarial: complete fruit list per env, fcap entries
    int32_t fcap;
    unsigned long long* stats;   // [8], separate small allocation (msnake_get_stats)
    // per-call i/o (device pointers owned by the caller)
    const int32_t* actions;
    uint8_t* obs;
    StepRest rest;
};

hipError_t launch_stats(uint32_t* hdr, int nenv, unsigned long long* stats, int clear, hipStream_t stream);
hipError_t launch_step(const StepParams& p, int rules, int mode, int envs_per_block, hipStream_t stream);
// canonical state words (include/msnake.h) of envs [env0, env0 + count) <-> the device layout
hipError_t launch_state_sizes(const StepParams& p, int rules, int env0, int count, uint32_t* need_words, hipStream_t stream);
hipError_t launch_state_pack(const StepParams& p, int rules, int env0, int count, const uint64_t* offsets, int32_t* words,
                             hipStream_t stream);
hipError_t launch_state_unpack(const StepParams& p, int rules, int env0, int count, const uint64_t* offsets,
                               const int32_t* words, uint32_t* status, hipStream_t stream);
// the same words of EVERY env as rows of a device tensor (msnake_export_states / msnake_import_states): row e at e * stride;
// export: words or count may be NULL; import: mask NULL = every env, count NULL = every row has `stride` words, status
// gets one byte per env, and a head outside the grid is refused when refuse_offgrid_head
hipError_t launch_state_export(const StepParams& p, int rules, int32_t* words, int32_t stride, int32_t* count, hipStream_t stream);
hipError_t launch_state_import(const StepParams& p, int rules, const uint8_t* mask, const int32_t* words, int32_t stride,
                               const int32_t* count, uint8_t* status, bool refuse_offgrid_head, hipStream_t stream);
// random legal positions as such rows, for the envs `mask` selects (msnake_generate.inc): len holds the requested body
// lengths, gseed is the generator's Philox key; words, count and got may be NULL.  Reads the handle's state only
hipError_t launch_generate(const StepParams& p, const uint8_t* mask, const int32_t* len, int32_t len_stride, bool compact,
                           uint64_t gseed, int32_t* words, int32_t stride, int32_t* count, int32_t* got, hipStream_t stream);
// MSNAKE_HASH_FULL / MSNAKE_HASH_BOARD of every env's canonical words (msnake_hash.inc); reads the handle's state only
hipError_t launch_state_hash(const StepParams& p, int rules, bool board, uint64_t* hash, hipStream_t stream);
// scripted opponents / safe-move masks from the state in HBM (msnake_scripted.inc); reads the handle's state only
hipError_t launch_scripted(const StepParams& p, int rules, int policy, uint32_t snake_mask, int32_t* actions, int32_t action_stride,
                           uint8_t* safe, hipStream_t stream);
// reachable-space counts and the space_greedy opponent (msnake_space.inc); reads the handle's state only
hipError_t launch_space(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                        uint16_t* space, hipStream_t stream);
// Voronoi territory counts and the territory_greedy opponent (msnake_territory.inc); reads the handle's state only
hipError_t launch_territory(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride,
                            uint8_t* safe, uint16_t* territory, hipStream_t stream);
// BFS distances to the fruits, per move and as a field, and the path_greedy opponent (msnake_path.inc); reads the handle's state only
hipError_t launch_path(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                       uint16_t* path, uint16_t* field, hipStream_t stream);
// every snake's BFS distance to every cell, the Voronoi owner map and the owned-cell counts (msnake_heads.inc); any of the
// three may be NULL, snake_mask selects the distance planes.  Reads the handle's state only
hipError_t launch_heads(const StepParams& p, int rules, uint32_t snake_mask, uint16_t* dist, uint8_t* owner, uint16_t* counts,
                        hipStream_t stream);
// cell lifetimes, the timed reach of every move and the timed_greedy opponent (msnake_timed.inc); reads the handle's state only
hipError_t launch_timed(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                        uint16_t* reach, uint16_t* life, hipStream_t stream);
// the fate of every move, the two action masks and the wary_greedy opponent (msnake_fates.inc); any of the four outputs may be
// NULL.  Reads the handle's state only
hipError_t launch_fates(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* fate,
                        uint8_t* by, uint8_t* eat, uint8_t* mask, hipStream_t stream);
// n_steps of [policies -> step] per env in one launch, the env held in LDS (msnake_playout.inc); snake_env only, any of the
// six outputs may be NULL.  eps NULL: nobody explores (msnake_playout); else eps_q16 per snake and the exploration stream's
// seed xseed (msnake_playout_explore).  Reads the handle's state only
hipError_t launch_playout(const StepParams& p, int rules, const int32_t* policies, const uint32_t* eps, uint64_t xseed,
                          int32_t n_steps, const int32_t* first, int32_t first_stride, uint32_t first_mask, int32_t* steps,
                          uint8_t* end, float* ret, int32_t* info, int32_t* words, int32_t words_stride, int32_t* count,
                          hipStream_t stream);
// the action every snake's policy writes, or with probability eps_q16 / 65536 a uniform draw from its candidate set, under the
// exploration stream's seed xseed (msnake_explore.inc); explored may be NULL.  Reads the handle's state only
hipError_t launch_explore(const StepParams& p, int rules, const int32_t* policies, const uint32_t* eps, uint64_t xseed,
                          uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* explored, hipStream_t stream);
// env state of `src` into `dst`, one wave per destination env (msnake_copy.inc); src_index NULL = the identity.  Reads `src` only
hipError_t launch_copy_envs(const StepParams& dst, const StepParams& src, int rules, const int32_t* src_index, hipStream_t stream);
// why each snake died in the step between `before` and `after`, and on whose body (msnake_causes.inc); any of the four
// outputs may be NULL.  Reads both handles only
hipError_t launch_death_causes(const StepParams& after, const StepParams& before, int rules, uint8_t* cause, uint8_t* by,
                               uint8_t* victims, int8_t* where, hipStream_t stream);
// the observation as cell codes and the per-snake table (msnake_cells.inc); view_mask 0 / snakes NULL = that output is not
// written.  Reads the handle's state only
hipError_t launch_cells(const StepParams& p, int rules, uint32_t view_mask, uint8_t* cells, int32_t* snakes, hipStream_t stream);
// head-centred cell-code windows of the snakes in snake_mask (msnake_local.inc); heading NULL = not written
hipError_t launch_local(const StepParams& p, int rules, int radius, uint32_t snake_mask, int oriented, uint8_t* windows,
                        uint8_t* heading, hipStream_t stream);
// eight-direction ray observations of the snakes in snake_mask (msnake_rays.inc); rays 4-byte aligned, heading NULL = not written
hipError_t launch_rays(const StepParams& p, int rules, uint32_t snake_mask, int oriented, uint8_t* rays, uint8_t* heading,
                       hipStream_t stream);
// per-snake outcomes of the last step against the caller's tracker, or (arm) the tracker from the state (msnake_agents.inc);
// any of rew / ate / flags / info may be NULL.  Reads the handle's state only
hipError_t launch_agents(const StepParams& p, int rules, bool arm, int32_t* track, const uint8_t* done, float* rew, uint8_t* ate,
                         uint8_t* flags, int32_t* info, hipStream_t stream);
// the DIM of the compile-time-shape instantiation that fits the configuration in `p` in every folded field, or 0 (host only)
int spec_dim_of(const StepParams& p, int rules);
// which kernel one launch gets: MSNAKE_CALL_GENERIC / _SHAPE / _PLAIN of include/msnake.h (host only, no HIP call)
int call_shape_of(const StepParams& p, int mode);
// the instantiation that per-step launches run (spec_dim 0: the generic four-parameter one)
void step_kernel_name(int rules, int n_snakes, int obs_scale, int spec_dim, char* out, size_t n);

}  // namespace msnake

#endif
