// msnake_capi.hip -- the C-ABI of include/msnake.h over the HIP kernels.  Host-side glue only:
// argument checks, HBM allocation of the per-env state, the background image, launches, and the
// (blocking, test/checkpoint-path) canonical state import/export, whose packing itself runs on the
// device.  No CPU fallback: without a HIP device every entry point fails with MSNAKE_E_NOGPU /
// MSNAKE_E_HIP.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "msnake_internal.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return fail(MSNAKE_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                        __LINE__);                                                                      \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

constexpr uint32_t kMagic = 0x4D534E4Bu;  // "MSNK"

}  // namespace

struct msnake_env {
    uint32_t magic;
    msnake_config cfg;
    msnake::StepParams p;  // configuration + state pointers; i/o pointers filled per call
    int epb;               // envs per workgroup
    int64_t env_steps;
    void* d_state;
    void* d_stats;
    void* d_scratch;       // per-env state import/export staging (grown on demand)
    size_t scratch_bytes;
    char kname[64];
    // a state with a head outside the grid was installed (msnake_set_state*) or may have been copied in (msnake_copy_envs
    // from such a handle): see note_offgrid_head
    int offgrid_head;
    // MSNAKE_DBG_STAGES builds only (tools/span_gap.py): per-launch slots of wave stamps
    unsigned long long* dbg_span;
    uint32_t dbg_span_slots, dbg_launch;
};

namespace {

int check(msnake_handle h) {
    if (!h || h->magic != kMagic) return fail(MSNAKE_E_HANDLE, "invalid or destroyed msnake handle");
    return MSNAKE_OK;
}

// a launch's hipError_t -> the return code and the message
int launched(hipError_t e) {
    if (e != hipSuccess) return fail(MSNAKE_E_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    return MSNAKE_OK;
}

// every device allocation of a handle, complete or partly built, and the handle itself (on the handle's device)
struct ReleaseHandle {
    void operator()(msnake_env* h) const {
        (void)hipFree(h->d_state); (void)hipFree(h->d_stats);
        if (h->d_scratch) (void)hipFree(h->d_scratch);
        h->magic = 0; free(h);
    }
};

// msnake_step's action_stride (msnake_call_shape_for_config checks nothing else)
int check_action_stride(int32_t action_stride, int ns) {
    if (action_stride < ns || action_stride > 7)
        return fail(MSNAKE_E_ARG, "action_stride %d must be in [n_snakes=%d, 7]", action_stride, ns);
    return MSNAKE_OK;
}

// the arguments of a step (msnake_step, msnake_rollout_tape); `fn` names the entry point in the message
int check_step_args(const char* fn, int ns, const int32_t* actions, int32_t action_stride, const float* rew, const uint8_t* done, const msnake_info* info) {
    if (!actions || !rew || !done) return fail(MSNAKE_E_ARG, "%s: actions/rew/done must not be NULL", fn);
    if (int rc = check_action_stride(action_stride, ns)) return rc;
    if (((uintptr_t)actions & 3) || ((uintptr_t)rew & 3) || ((uintptr_t)info & 15))
        return fail(MSNAKE_E_ALIGN, "actions/rew must be 4-byte and info 16-byte aligned");
    return MSNAKE_OK;
}

// the per-call fields of a copy of the handle's StepParams
void fill_call(msnake::StepParams& p, const int32_t* actions, int32_t action_stride, uint8_t* obs, float* rew, uint8_t* done, msnake_info* info) {
    p.actions = actions; p.action_stride = action_stride;
    p.obs = obs; p.rest.rew = rew; p.rest.done = done; p.rest.info = info;
}

// the arguments of a call that may write actions (msnake_scripted_ / _space_ / _territory_ / _path_ / _timed_ / _fate_actions); the last two count only if it does
int check_action_writer(const char* fn, int ns, bool writes_actions, uint32_t snake_mask, const int32_t* actions_dev, int32_t action_stride) {
    if (snake_mask >> ns) return fail(MSNAKE_E_ARG, "%s: snake_mask 0x%x has a bit >= n_snakes=%d", fn, snake_mask, ns);
    if (!writes_actions) return MSNAKE_OK;
    if (!actions_dev) return fail(MSNAKE_E_ARG, "%s: actions_dev is NULL", fn);
    if (action_stride < ns) return fail(MSNAKE_E_ARG, "%s: action_stride %d must be >= n_snakes=%d", fn, action_stride, ns);
    if ((uintptr_t)actions_dev & 3) return fail(MSNAKE_E_ALIGN, "actions_dev must be 4-byte aligned");
    return MSNAKE_OK;
}

// the snake selection and the `oriented` flag of a per-snake observation (msnake_render_local, msnake_render_rays);
// `what` names one snake's share of the output in the message
int check_snake_view(const char* fn, const char* what, int ns, uint32_t snake_mask, int32_t oriented) {
    if (!snake_mask) return fail(MSNAKE_E_ARG, "%s: snake_mask is 0 (no %s to write)", fn, what);
    if (snake_mask >> ns) return fail(MSNAKE_E_ARG, "%s: snake_mask 0x%x has a bit >= n_snakes=%d", fn, snake_mask, ns);
    if (oriented != 0 && oriented != 1) return fail(MSNAKE_E_ARG, "%s: oriented must be 0 or 1, got %d", fn, oriented);
    return MSNAKE_OK;
}

// two handles whose env state has the same layout on the same device (msnake_copy_envs, msnake_death_causes); `an` and
// `bn` name the two arguments in the message
int check_same_board(const char* fn, const char* an, const msnake_config& a, const char* bn, const msnake_config& b) {
    if (a.dim != b.dim) return fail(MSNAKE_E_ARG, "%s: %s has dim %d, %s has dim %d", fn, an, a.dim, bn, b.dim);
    if (a.n_snakes != b.n_snakes) return fail(MSNAKE_E_ARG, "%s: %s has n_snakes %d, %s has n_snakes %d", fn, an, a.n_snakes, bn, b.n_snakes);
    if (a.n_fruits != b.n_fruits) return fail(MSNAKE_E_ARG, "%s: %s has n_fruits %d, %s has n_fruits %d", fn, an, a.n_fruits, bn, b.n_fruits);
    if (a.rules != b.rules) return fail(MSNAKE_E_ARG, "%s: %s has rules %d, %s has rules %d", fn, an, a.rules, bn, b.rules);
    if (a.device != b.device) return fail(MSNAKE_E_ARG, "%s: %s lives on device %d, %s on device %d", fn, an, a.device, bn, b.device);
    return MSNAKE_OK;
}

int ensure_scratch(msnake_env* h, size_t bytes) {
    if (bytes <= h->scratch_bytes) return MSNAKE_OK;
    if (h->d_scratch) (void)hipFree(h->d_scratch);
    h->d_scratch = nullptr; h->scratch_bytes = 0;
    hipError_t e = hipMalloc(&h->d_scratch, bytes);
    if (e != hipSuccess) return fail(MSNAKE_E_HIP, "allocating %zu bytes of state staging failed: %s", bytes, hipGetErrorString(e));
    h->scratch_bytes = bytes;
    return MSNAKE_OK;
}

// A head outside the grid exists in no state that play leaves behind (a snake whose head leaves the grid is cleared in
// the same step); msnake_set_state accepts it.  If that snake turns back into the grid, its next step leaves a BODY piece
// outside the grid, which the reference draws under the wall.  The generic step kernels clip such a piece; the kernels
// compiled for a shape keep the painter that assumes it cannot exist, so a handle that may hold such a state runs the
// generic kernels from then on (same results; msnake_kernel_name follows).
void note_offgrid_head(msnake_env* h) {
    h->offgrid_head = 1;
    if (h->p.spec_dim != 0) {
        h->p.spec_dim = 0;
        msnake::step_kernel_name(h->cfg.rules, h->cfg.n_snakes, h->cfg.obs_scale, 0, h->kname, sizeof(h->kname));
    }
}

const char* state_reason(uint32_t code) {
    switch (code) {
        case MSNAKE_ST_SHORT: return "state buffer too short / truncated";
        case MSNAKE_ST_SNAKES: return "snake count differs from the handle's";
        case MSNAKE_ST_FRUITS: return "fruit count differs from the handle's (or exceeds the fruit-list capacity)";
        case MSNAKE_ST_CELL: return "a cell lies outside [-1, dim], or a body piece behind the head outside the grid";
        case MSNAKE_ST_LEN: return "a body length is outside [0, capacity]";
        case MSNAKE_ST_SCALAR: return "a scalar field out of range (t, spare_fruits, ep_len or grow_to negative, a velocity that is no unit step, alive / in_dead)";
        default: return "malformed state";
    }
}

}  // namespace

extern "C" {

int msnake_abi_version(void) { return MSNAKE_ABI_VERSION; }
const char* msnake_last_error(void) { return g_err; }

namespace {

// argument checks of msnake_create (no GPU involved); *cfg_full <- the configuration widened to the current struct
int validate_config(const msnake_config* cfg_in, msnake_config* cfg_full) {
    // ABI 3 appended the launch-tuning fields; an ABI-2 caller passes the 56-byte prefix and gets "auto"
    if (cfg_in->struct_size != sizeof(msnake_config) && cfg_in->struct_size != MSNAKE_CONFIG_SIZE_V2)
        return fail(MSNAKE_E_ARG, "msnake_config.struct_size %u is neither %zu (ABI 3) nor %u (ABI 2)", cfg_in->struct_size,
                    sizeof(msnake_config), MSNAKE_CONFIG_SIZE_V2);
    memset(cfg_full, 0, sizeof(*cfg_full));
    memcpy(cfg_full, cfg_in, cfg_in->struct_size);
    cfg_full->struct_size = (uint32_t)sizeof(msnake_config);
    const msnake_config* cfg = cfg_full;
    if (cfg->num_envs < 1) return fail(MSNAKE_E_ARG, "num_envs must be >= 1 (got %d)", cfg->num_envs);
    if (cfg->dim < 2 || cfg->dim > MSNAKE_MAX_DIM)
        return fail(MSNAKE_E_ARG, "dim must be in [2, %d] (got %d)", MSNAKE_MAX_DIM, cfg->dim);
    if (cfg->rules != MSNAKE_RULES_SNAKE_ENV && cfg->rules != MSNAKE_RULES_NEW_WORLD &&
        cfg->rules != MSNAKE_RULES_ADVERSARIAL)
        return fail(MSNAKE_E_ARG, "rules %d is not one of MSNAKE_RULES_*", cfg->rules);
    if (cfg->rules == MSNAKE_RULES_NEW_WORLD) {
        if (cfg->n_snakes < 1 || cfg->n_snakes > MSNAKE_MAX_SNAKES)
            return fail(MSNAKE_E_ARG, "new_world: n_snakes must be in [1, %d]", MSNAKE_MAX_SNAKES);
        if (cfg->n_fruits < 0 || cfg->n_fruits > MSNAKE_MAX_FRUITS)
            return fail(MSNAKE_E_ARG, "new_world: n_fruits must be in [0, %d]", MSNAKE_MAX_FRUITS);
    } else {
        // SnakeEnv.reset hard-codes 3 velocity / grow_to slots and one fruit per snake
        // (snake_multiple_test.py:223-228)
        if (cfg->n_snakes < 1 || cfg->n_snakes > 3)
            return fail(MSNAKE_E_ARG, "snake_env: n_snakes must be in [1, 3] (got %d)", cfg->n_snakes);
        if (cfg->n_fruits != cfg->n_snakes)
            return fail(MSNAKE_E_ARG, "snake_env: n_fruits must equal n_snakes");
    }
    if (cfg->max_steps < 1 || cfg->max_steps > 60000)
        return fail(MSNAKE_E_ARG, "max_steps must be in [1, 60000]");
    if ((uint64_t)cfg->num_envs * (uint64_t)msnake::shape::fixed_bytes(MSNAKE_MAX_SNAKES) >= (1ull << 32))
        return fail(MSNAKE_E_ARG, "num_envs %d: records and body rings of one handle must stay below 4 GB (the kernel "
                                  "addresses them with 32-bit offsets); use several handles", cfg->num_envs);
    if (cfg->obs_scale != 1 && cfg->obs_scale != 4 && cfg->obs_scale != 7)
        return fail(MSNAKE_E_ARG, "obs_scale must be 1, 4 (21->84) or 7 (12->84), got %d", cfg->obs_scale);
    if (cfg->envs_per_block < 0 || cfg->envs_per_block > MSNAKE_MAX_ENVS_PER_BLOCK)
        return fail(MSNAKE_E_ARG, "envs_per_block must be 0 (auto) or in [1, %d], got %d", MSNAKE_MAX_ENVS_PER_BLOCK, cfg->envs_per_block);
    if (cfg->record_policy < 0 || cfg->record_policy > MSNAKE_RECORD_SHORT)
        return fail(MSNAKE_E_ARG, "record_policy must be MSNAKE_AUTO, MSNAKE_RECORD_FULL or MSNAKE_RECORD_SHORT, got %d", cfg->record_policy);
    if (cfg->obs_store_policy < 0 || cfg->obs_store_policy > MSNAKE_STORE_STREAM || cfg->tape_store_policy < 0 ||
        cfg->tape_store_policy > MSNAKE_STORE_STREAM)
        return fail(MSNAKE_E_ARG, "obs_store_policy / tape_store_policy must be MSNAKE_AUTO, MSNAKE_STORE_PLAIN or MSNAKE_STORE_STREAM");
    return MSNAKE_OK;
}

// Everything of StepParams that follows from the configuration alone: the shape of the observation, of the state and of
// the LDS image, and the record policy.  No GPU involved (msnake_kernel_name_for_config runs it without one).
int derive_shape(const msnake_config* cfg, msnake::StepParams& p) {
    namespace shape = msnake::shape;
    const int dim = cfg->dim, W = dim + 2, n2 = dim * dim;
    p.nenv = cfg->num_envs;
    p.dim = dim;
    p.n_snakes = cfg->n_snakes;
    p.n_fruits = cfg->n_fruits;
    p.views = cfg->rules == MSNAKE_RULES_NEW_WORLD ? cfg->n_snakes : 3;
    p.C = 3 * p.views;
    p.S = shape::obs_bytes(dim, p.C);
    p.obs_scale = cfg->obs_scale;
    p.rest.max_steps = cfg->max_steps;
    p.auto_reset = cfg->auto_reset ? 1 : 0;
    // ring capacity: snake_env bodies hold distinct in-grid cells plus one transient head;
    // new_world bodies can stack duplicates and are only bounded by the episode length
    int need = n2 + 2;
    if (cfg->rules == MSNAKE_RULES_NEW_WORLD && cfg->max_steps + 2 > need) need = cfg->max_steps + 2;
    p.rest.cap = shape::ring_cap(need);
    const int K = cfg->obs_scale;
    if (K > 1 && (W * K * p.C) % 4 != 0) return fail(MSNAKE_E_ARG, "obs_scale %d: output rows must be whole dwords", K);
    p.img_bytes = shape::img_bytes(p.S, K);
    p.lds_per_wave = shape::lds_per_wave(p.img_bytes, n2, false);
    if ((size_t)p.lds_per_wave > 64 * 1024 - 16 || p.S > 0xFFFF)
        return fail(MSNAKE_E_ARG, "observation image of %d bytes does not fit in LDS", p.S);
    // record_policy: snake_env / adversarial steps can run on the first 128 bytes of the 256-byte
    // record; the upper half only parks Philox draws for the waves that respawn or reset, which pays
    // while a launch is latency bound (<= 8 192 envs) and is pure traffic above
    p.short_rec = (cfg->rules != MSNAKE_RULES_NEW_WORLD && p.nenv > 8192) ? 1 : 0;
    if (cfg->record_policy != MSNAKE_AUTO)  // (new_world keeps its fruits in the upper half: always the full record)
        p.short_rec = (cfg->rules != MSNAKE_RULES_NEW_WORLD && cfg->record_policy == MSNAKE_RECORD_SHORT) ? 1 : 0;
    return MSNAKE_OK;
}

// msnake_set_generic_kernels: handles created while it is on stay on the generic kernels (A/B runs, tests)
std::atomic<int> g_generic_kernels{0};

// The compile-time shape the handle's step / tape launches use (0 = the generic kernels): decided once, from the
// derived configuration.
int pick_spec_dim(const msnake::StepParams& p, int rules) {
    if (g_generic_kernels.load(std::memory_order_relaxed)) return 0;
    return msnake::spec_dim_of(p, rules);
}

// envs (= waves) per workgroup of the handle's per-step launches: 8 up to 8 192 envs (512 workgroups at 4 096 envs start
// 3 % sooner than 1 024: 7.63 -> 7.40 us per launch), 4 above (an 8-wave workgroup needs 8 free wave slots on one CU at
// once: 29.5 vs 30.9 us at 32 768 envs), fewer where the LDS images need it, and never above cfg->envs_per_block
int pick_epb(const msnake_config* cfg, const msnake::StepParams& p) {
    int epb = msnake::shape::epb_that_fits(p.nenv <= 8192 ? MSNAKE_MAX_ENVS_PER_BLOCK : 4, p.lds_per_wave);
    if (cfg->envs_per_block > 0 && cfg->envs_per_block < epb) epb = cfg->envs_per_block;  // (never above what LDS allows)
    return epb;
}

// envs per workgroup of the handle's persistent tape launch (msnake_rollout_tape); 0: the kernel's second image does not
// fit in LDS beside the first, and the call is served by per-step launches
int pick_tape_epb(const msnake::StepParams& p, int epb) {
    return msnake::shape::tape_epb(epb, p.img_bytes, p.dim * p.dim, p.obs_scale);
}

// what a handle created from *cfg_in right now would step with, without a GPU: the *_for_config calls
int shape_for_config(const msnake_config* cfg_in, msnake_config* cfg, msnake::StepParams& p) {
    if (int rc = validate_config(cfg_in, cfg)) return rc;
    memset(&p, 0, sizeof(p));
    if (int rc = derive_shape(cfg, p)) return rc;
    p.spec_dim = pick_spec_dim(p, cfg->rules);
    return MSNAKE_OK;
}

}  // namespace

int msnake_create(const msnake_config* cfg_in, msnake_handle* out) {
    if (!cfg_in || !out) return fail(MSNAKE_E_ARG, "msnake_create: NULL argument");
    *out = nullptr;
    msnake_config cfg_full;
    if (int rc = validate_config(cfg_in, &cfg_full)) return rc;
    const msnake_config* cfg = &cfg_full;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(MSNAKE_E_NOGPU, "no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev)
        return fail(MSNAKE_E_ARG, "device %d out of range (have %d)", cfg->device, ndev);
    DeviceGuard guard(cfg->device);

    // (released on every return but the last one)
    std::unique_ptr<msnake_env, ReleaseHandle> owner(static_cast<msnake_env*>(calloc(1, sizeof(msnake_env))));
    msnake_env* h = owner.get();
    if (!h) return fail(MSNAKE_E_ARG, "out of host memory");
    h->cfg = *cfg;
    msnake::StepParams& p = h->p;
    if (int rc = derive_shape(cfg, p)) return rc;
    const int dim = cfg->dim, W = dim + 2, n2 = dim * dim;
    const int K = cfg->obs_scale;
    p.rest.seed_lo = (uint32_t)cfg->seed;
    p.rest.seed_hi = (uint32_t)(cfg->seed >> 32);
    p.rest.env_id_base = cfg->env_id_base;
    h->epb = pick_epb(cfg, p);

    const int tmpl_copies = K == 1 ? MSNAKE_TMPL_COPIES : 1;
    const size_t tmpl_bytes = (size_t)p.img_bytes * tmpl_copies;
    p.fcap = msnake::shape::fruit_cap(p.n_snakes, n2);
    const auto sec = msnake::shape::sections(p.nenv, p.n_snakes, tmpl_bytes, p.rest.cap, p.fcap, cfg->rules);
    const size_t state_bytes = sec.total;
    hipError_t e;
    if ((e = hipMalloc(&h->d_state, state_bytes)) != hipSuccess || (e = hipMalloc(&h->d_stats, 64)) != hipSuccess ||
        (e = hipMemset(h->d_state, 0, state_bytes)) != hipSuccess || (e = hipMemset(h->d_stats, 0, 64)) != hipSuccess)
        return fail(MSNAKE_E_HIP, "allocating %zu bytes of env state failed: %s", state_bytes, hipGetErrorString(e));
    p.state = static_cast<uint8_t*>(h->d_state);
    p.hdr = reinterpret_cast<uint32_t*>(p.state + sec.hdr);
    p.body0 = reinterpret_cast<uint16_t*>(p.state + sec.body0);
    p.tmpl = p.state + sec.tmpl;
    p.ring = reinterpret_cast<uint16_t*>(p.state + sec.ovf);
    p.fl0 = reinterpret_cast<uint16_t*>(p.state + sec.fl0);
    p.flist = reinterpret_cast<uint16_t*>(p.state + sec.flist);
    p.stats = static_cast<unsigned long long*>(h->d_stats);
    // background image: black interior, white 1-px wall ring (snake_multiple_test.py:38,52-56)
    std::vector<uint8_t> tmpl(tmpl_bytes, 0);
    for (int copy = 0; copy < tmpl_copies; ++copy)  // (copy s: the image starts s bytes into its buffer)
        for (int r = 0; r < W; ++r)
            for (int c = 0; c < W; ++c)
                if (r == 0 || r == W - 1 || c == 0 || c == W - 1)
                    memset(&tmpl[(size_t)copy * p.img_bytes + copy + ((size_t)r * W + c) * p.C * K], 255, (size_t)p.C * K);
    if ((e = hipMemcpy(const_cast<uint8_t*>(p.tmpl), tmpl.data(), tmpl_bytes, hipMemcpyHostToDevice)) != hipSuccess)
        return fail(MSNAKE_E_HIP, "uploading the background image failed: %s", hipGetErrorString(e));
    // obs_store_policy: should the observation stores carry the nt (streaming) hint?  Measured on
    // MI355X with the native 16-byte-per-lane copy-out (tools/kbench.py --store-policy plain/stream), per launch:
    //   <= 32 MiB of observations (<= 8 192 envs at 19x19x3; fits the 8 L2s): 2-3 % faster with nt
    //      (nothing is left to write back when the kernel ends);
    //   64-130 MiB (fits the 256 MB Infinity Cache): 0-4 % slower (a re-used buffer no longer hits);
    //   >= 260 MiB: 33-42 % faster (388 -> 243 us at 262 144 envs: plain stores thrash the cache).
    // The fused x4 / x7 copy-out stores dwords (256 B per wave instruction) and is 2.5x SLOWER with
    // nt, so it never streams; neither does the persistent tape kernel (187 -> 208 us).
    {
        const double obs_mib = (double)p.nenv * p.S * p.obs_scale * p.obs_scale / (1024.0 * 1024.0);
        p.rest.stream_obs = (p.obs_scale == 1 ? (obs_mib <= 32.0 || obs_mib >= 192.0) : obs_mib >= 400.0) ? 1u : 0u;
    }
    if (cfg->obs_store_policy != MSNAKE_AUTO) p.rest.stream_obs = cfg->obs_store_policy == MSNAKE_STORE_STREAM ? 1u : 0u;
#ifdef MSNAKE_DBG_STAGES  // diagnostic builds only (tools/stamp_profile.py): never in the shipped library
    if (const char* dbg = getenv("MSNAKE_DBG_STAGE")) p.rest.dbg_stage = (uint32_t)atoi(dbg);
    if (const char* dbg = getenv("MSNAKE_DBG_BUF")) p.rest.dbg_buf = reinterpret_cast<unsigned long long*>(strtoull(dbg, nullptr, 0));
#endif
#if defined(MSNAKE_DBG_STAGES) || defined(MSNAKE_SPAN_LIGHT)  // (measurement builds only, like the block above)
    if (const char* dbg = getenv("MSNAKE_DBG_SPAN")) {  // base of a caller-owned [MSNAKE_DBG_SPAN_SLOTS][num_envs][8] u64 device buffer
        h->dbg_span = reinterpret_cast<unsigned long long*>(strtoull(dbg, nullptr, 0));
        const char* sl = getenv("MSNAKE_DBG_SPAN_SLOTS");
        h->dbg_span_slots = sl ? (uint32_t)atoi(sl) : 1u;
        if (h->dbg_span_slots < 1) h->dbg_span_slots = 1;
    }
#endif
    p.spec_dim = pick_spec_dim(p, cfg->rules);
    msnake::step_kernel_name(cfg->rules, cfg->n_snakes, cfg->obs_scale, p.spec_dim, h->kname, sizeof(h->kname));
    h->magic = kMagic;
    *out = owner.release();
    return MSNAKE_OK;
}

int msnake_destroy(msnake_handle h) {
    if (int rc = check(h)) return rc;
    DeviceGuard guard(h->cfg.device);
    (void)hipDeviceSynchronize();
    ReleaseHandle()(h);
    return MSNAKE_OK;
}

int msnake_obs_shape(msnake_handle h, int32_t* H, int32_t* W, int32_t* C) {
    if (int rc = check(h)) return rc;
    if (H) *H = (h->p.dim + 2) * h->p.obs_scale;
    if (W) *W = (h->p.dim + 2) * h->p.obs_scale;
    if (C) *C = h->p.C;
    return MSNAKE_OK;
}

static int launch(msnake_handle h, int mode, const int32_t* actions, int32_t action_stride, uint8_t* obs, float* rew,
                  uint8_t* done, msnake_info* info, void* stream, const uint8_t* env_mask = nullptr,
                  uint8_t* truncated = nullptr) {
    msnake::StepParams p = h->p;
    fill_call(p, actions, action_stride, obs, rew, done, info);
    p.rest.env_mask = env_mask; p.rest.truncated = truncated;  // (MODE 1 / 2 only; msnake_reset_envs)
    DeviceGuard guard(h->cfg.device);
    if (obs && p.obs_scale > 1 && ((uintptr_t)obs & 3))  // the fused x4 / x7 copy-out stores dwords
        return fail(MSNAKE_E_ALIGN, "obs_dev must be 4-byte aligned when obs_scale > 1");
#if defined(MSNAKE_DBG_STAGES) || defined(MSNAKE_SPAN_LIGHT)
    if (h->dbg_span && mode == 0)  // every msnake_step launch stamps into its own slot (they wrap)
        p.rest.dbg_span = h->dbg_span + (size_t)(h->dbg_launch++ % h->dbg_span_slots) * (size_t)p.nenv * 8;
#endif
    return launched(msnake::launch_step(p, h->cfg.rules, mode, h->epb, static_cast<hipStream_t>(stream)));
}

int msnake_reset(msnake_handle h, uint8_t* obs_dev, void* stream) {
    if (int rc = check(h)) return rc;
    return launch(h, 1, nullptr, 0, obs_dev, nullptr, nullptr, nullptr, stream);
}

int msnake_reset_envs(msnake_handle h, const uint8_t* mask_dev, uint8_t* obs_dev, uint8_t* final_obs_dev,
                      uint8_t* truncated_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (!mask_dev) return fail(MSNAKE_E_ARG, "msnake_reset_envs: mask_dev is NULL (msnake_reset resets every env)");
    // both observation pointers are checked before anything is launched
    if (h->p.obs_scale > 1 && (((uintptr_t)obs_dev | (uintptr_t)final_obs_dev) & 3))
        return fail(MSNAKE_E_ALIGN, "obs_dev and final_obs_dev must be 4-byte aligned when obs_scale > 1");
    // the selected envs' terminal observations first (a masked render), then the masked reset on the same stream
    if (final_obs_dev)
        if (int rc = launch(h, 2, nullptr, 0, final_obs_dev, nullptr, nullptr, nullptr, stream, mask_dev)) return rc;
    return launch(h, 1, nullptr, 0, obs_dev, nullptr, nullptr, nullptr, stream, mask_dev, truncated_dev);
}

int msnake_render(msnake_handle h, uint8_t* obs_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (!obs_dev) return fail(MSNAKE_E_ARG, "msnake_render: obs_dev is NULL");
    return launch(h, 2, nullptr, 0, obs_dev, nullptr, nullptr, nullptr, stream);
}

int msnake_step(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, uint8_t* obs_dev, float* rew_dev,
                uint8_t* done_dev, msnake_info* info_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_step_args("msnake_step", h->p.n_snakes, actions_dev, action_stride, rew_dev, done_dev, info_dev)) return rc;
    int rc = launch(h, 0, actions_dev, action_stride, obs_dev, rew_dev, done_dev, info_dev, stream);
    if (rc == MSNAKE_OK) h->env_steps += h->p.nenv;
    return rc;
}

int msnake_step_tape(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, int32_t n_steps, uint8_t* obs_dev,
                     size_t obs_step_stride, float* rew_dev, uint8_t* done_dev, msnake_info* info_dev,
                     size_t scalar_step_stride, void* stream) {
    if (int rc = check(h)) return rc;
    if (n_steps < 0) return fail(MSNAKE_E_ARG, "n_steps < 0");
    const size_t astep = (size_t)h->p.nenv * (size_t)action_stride;
    for (int32_t k = 0; k < n_steps; ++k) {
        int rc = msnake_step(h, actions_dev + (size_t)k * astep, action_stride,
                             obs_dev ? obs_dev + (size_t)k * obs_step_stride : nullptr,
                             rew_dev + (size_t)k * scalar_step_stride, done_dev + (size_t)k * scalar_step_stride,
                             info_dev ? info_dev + (size_t)k * scalar_step_stride : nullptr, stream);
        if (rc != MSNAKE_OK) return rc;
    }
    return MSNAKE_OK;
}

int msnake_rollout_tape(msnake_handle h, const int32_t* actions_dev, int32_t action_stride, int32_t n_steps, uint8_t* obs_dev,
                        size_t obs_step_stride, float* rew_dev, uint8_t* done_dev, msnake_info* info_dev,
                        size_t scalar_step_stride, void* stream) {
    if (int rc = check(h)) return rc;
    if (n_steps < 1) return fail(MSNAKE_E_ARG, "n_steps must be >= 1");
    if (int rc = check_step_args("msnake_rollout_tape", h->p.n_snakes, actions_dev, action_stride, rew_dev, done_dev, info_dev)) return rc;
    // the persistent kernel keeps a second image in LDS; where that does not fit (decided here, before any launch, with
    // launch_k's arithmetic) the same steps go out as per-step launches: same results, same env_steps
    if (pick_tape_epb(h->p, h->epb) == 0)
        return msnake_step_tape(h, actions_dev, action_stride, n_steps, obs_dev, obs_step_stride, rew_dev, done_dev, info_dev,
                                scalar_step_stride, stream);
    msnake::StepParams p = h->p;
    fill_call(p, actions_dev, action_stride, obs_dev, rew_dev, done_dev, info_dev);
    p.rest.n_steps = n_steps;
    // tape_store_policy: a tape whose steps keep one alignment (step stride a multiple of 16 bytes: the aligned copy-out)
    // and whose observations go to per-step slices of >= 192 MiB in all streams (4 096 envs x 256 steps = 4.2 GB: 3.8 us per
    // step with nt, 4.05 plain); a re-used buffer (stride 0) merges in the L2s and stays plain, and so does the byte-aligned
    // shape of an odd stride (nt there: 4.45 us)
    {
        const double mib = (double)n_steps * p.nenv * p.S * p.obs_scale * p.obs_scale / (1024.0 * 1024.0);
        const bool aligned = p.obs_scale == 1 && obs_dev && obs_step_stride != 0 && obs_step_stride % 16 == 0;
        p.stream_tape = h->cfg.tape_store_policy == MSNAKE_STORE_STREAM || (h->cfg.tape_store_policy == MSNAKE_AUTO && aligned && mib >= 192.0) ? 1 : 0;
    }
    p.rest.obs_step_stride = obs_step_stride;
    p.rest.scalar_step_stride = scalar_step_stride;
    if (obs_dev && p.obs_scale > 1 && (((uintptr_t)obs_dev | obs_step_stride) & 3))
        return fail(MSNAKE_E_ALIGN, "obs_dev and obs_step_stride must be multiples of 4 when obs_scale > 1");
    DeviceGuard guard(h->cfg.device);
    int rc = launched(msnake::launch_step(p, h->cfg.rules, 3, h->epb, static_cast<hipStream_t>(stream)));
    if (rc == MSNAKE_OK) h->env_steps += (int64_t)h->p.nenv * n_steps;
    return rc;
}

int msnake_scripted_actions(msnake_handle h, int32_t policy, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride,
                            uint8_t* safe_dev, void* stream) {
    if (int rc = check(h)) return rc;
    const int ns = h->p.n_snakes;
    if (policy != MSNAKE_POLICY_NONE && policy != MSNAKE_POLICY_SAFE_GREEDY && policy != MSNAKE_POLICY_HAMILTONIAN)
        return fail(MSNAKE_E_ARG, "msnake_scripted_actions: policy %d is not one of MSNAKE_POLICY_*", policy);
    // (a snake_mask bit >= n_snakes is reported first: the parity check waits for a good mask)
    if (policy == MSNAKE_POLICY_HAMILTONIAN && (h->p.dim & 1) && !(snake_mask >> ns))
        return fail(MSNAKE_E_ARG, "msnake_scripted_actions: policy HAMILTONIAN needs an even dim (the cycle), got dim %d", h->p.dim);
    const bool writes_actions = policy != MSNAKE_POLICY_NONE && snake_mask != 0;
    if (int rc = check_action_writer("msnake_scripted_actions", ns, writes_actions, snake_mask, actions_dev, action_stride)) return rc;
    if (!writes_actions && !safe_dev)
        return fail(MSNAKE_E_ARG, "msnake_scripted_actions: nothing to write (policy NONE or snake_mask 0, and safe_dev is NULL)");
    DeviceGuard guard(h->cfg.device);
    // without actions to write the kernel only fills safe_dev: POLICY_NONE
    return launched(msnake::launch_scripted(h->p, h->cfg.rules, writes_actions ? policy : MSNAKE_POLICY_NONE, snake_mask, actions_dev,
                                            action_stride, safe_dev, static_cast<hipStream_t>(stream)));
}

int msnake_space_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* safe_dev,
                         uint16_t* space_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_action_writer("msnake_space_actions", h->p.n_snakes, snake_mask != 0, snake_mask, actions_dev, action_stride)) return rc;
    if (!snake_mask && !safe_dev && !space_dev)
        return fail(MSNAKE_E_ARG, "msnake_space_actions: nothing to write (snake_mask 0, safe_dev and space_dev are NULL)");
    if ((uintptr_t)space_dev & 1) return fail(MSNAKE_E_ALIGN, "space_dev must be 2-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_space(h->p, h->cfg.rules, snake_mask, actions_dev, action_stride, safe_dev, space_dev,
                                         static_cast<hipStream_t>(stream)));
}

int msnake_territory_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* safe_dev,
                             uint16_t* territory_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_action_writer("msnake_territory_actions", h->p.n_snakes, snake_mask != 0, snake_mask, actions_dev, action_stride)) return rc;
    if (!snake_mask && !safe_dev && !territory_dev)
        return fail(MSNAKE_E_ARG, "msnake_territory_actions: nothing to write (snake_mask 0, safe_dev and territory_dev are NULL)");
    if ((uintptr_t)territory_dev & 1) return fail(MSNAKE_E_ALIGN, "territory_dev must be 2-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_territory(h->p, h->cfg.rules, snake_mask, actions_dev, action_stride, safe_dev, territory_dev,
                                             static_cast<hipStream_t>(stream)));
}

int msnake_path_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* safe_dev,
                        uint16_t* path_dev, uint16_t* field_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_action_writer("msnake_path_actions", h->p.n_snakes, snake_mask != 0, snake_mask, actions_dev, action_stride)) return rc;
    if (!snake_mask && !safe_dev && !path_dev && !field_dev)
        return fail(MSNAKE_E_ARG, "msnake_path_actions: nothing to write (snake_mask 0, safe_dev, path_dev and field_dev are NULL)");
    if ((uintptr_t)path_dev & 1) return fail(MSNAKE_E_ALIGN, "path_dev must be 2-byte aligned");
    if ((uintptr_t)field_dev & 1) return fail(MSNAKE_E_ALIGN, "field_dev must be 2-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_path(h->p, h->cfg.rules, snake_mask, actions_dev, action_stride, safe_dev, path_dev, field_dev,
                                        static_cast<hipStream_t>(stream)));
}

int msnake_timed_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* safe_dev,
                         uint16_t* reach_dev, uint16_t* life_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_action_writer("msnake_timed_actions", h->p.n_snakes, snake_mask != 0, snake_mask, actions_dev, action_stride)) return rc;
    if (!snake_mask && !safe_dev && !reach_dev && !life_dev)
        return fail(MSNAKE_E_ARG, "msnake_timed_actions: nothing to write (snake_mask 0, safe_dev, reach_dev and life_dev are NULL)");
    if ((uintptr_t)reach_dev & 1) return fail(MSNAKE_E_ALIGN, "reach_dev must be 2-byte aligned");
    if ((uintptr_t)life_dev & 1) return fail(MSNAKE_E_ALIGN, "life_dev must be 2-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_timed(h->p, h->cfg.rules, snake_mask, actions_dev, action_stride, safe_dev, reach_dev, life_dev,
                                         static_cast<hipStream_t>(stream)));
}

int msnake_fate_actions(msnake_handle h, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* fate_dev,
                        uint8_t* by_dev, uint8_t* eat_dev, uint8_t* mask_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (h->cfg.rules == MSNAKE_RULES_NEW_WORLD)
        return fail(MSNAKE_E_ARG, "msnake_fate_actions: new_world judges its snakes one after the other and clears bodies as it "
                                  "goes, so the fate of a move does not follow from the state");
    if (int rc = check_action_writer("msnake_fate_actions", h->p.n_snakes, snake_mask != 0, snake_mask, actions_dev, action_stride)) return rc;
    if (!snake_mask && !fate_dev && !by_dev && !eat_dev && !mask_dev)
        return fail(MSNAKE_E_ARG, "msnake_fate_actions: nothing to write (snake_mask 0, fate_dev, by_dev, eat_dev and mask_dev are NULL)");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_fates(h->p, h->cfg.rules, snake_mask, actions_dev, action_stride, fate_dev, by_dev, eat_dev, mask_dev,
                                         static_cast<hipStream_t>(stream)));
}

namespace {

uint64_t mix64(uint64_t z) {  // the splitmix64 finaliser (msnake_hash_states)
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the seed of the exploration stream (msnake_explore_actions, msnake_playout_explore)
uint64_t explore_seed(uint64_t seed, uint64_t salt) { return mix64(seed ^ mix64(salt ^ 0x6578706C6F726521ull)); }  // "explore!"

// policies[s] for s < ns: one of MSNAKE_POLICY_* as msnake_playout takes them
int check_playout_policies(const char* fn, const int32_t* policies, int ns) {
    if (!policies) return fail(MSNAKE_E_ARG, "%s: policies is NULL", fn);
    for (int s = 0; s < ns; ++s)
        if (policies[s] < MSNAKE_POLICY_NONE || policies[s] > MSNAKE_POLICY_WARY_GREEDY)
            return fail(MSNAKE_E_ARG, "%s: policies[%d] = %d is not one of MSNAKE_POLICY_*", fn, s, policies[s]);
    return MSNAKE_OK;
}

int check_hamiltonian_board(const char* fn, const int32_t* policies, int ns, int dim) {
    for (int s = 0; s < ns; ++s)
        if (policies[s] == MSNAKE_POLICY_HAMILTONIAN && (dim & 1))
            return fail(MSNAKE_E_ARG, "%s: policy HAMILTONIAN needs an even dim (the cycle), got dim %d", fn, dim);
    return MSNAKE_OK;
}

// eps_q16[s] for s < ns: an exploration probability in units of 1 / 65536
int check_eps(const char* fn, const uint32_t* eps_q16, int ns) {
    if (!eps_q16) return fail(MSNAKE_E_ARG, "%s: eps_q16 is NULL", fn);
    for (int s = 0; s < ns; ++s)
        if (eps_q16[s] > 65536u) return fail(MSNAKE_E_ARG, "%s: eps_q16[%d] = %u is above 65536", fn, s, eps_q16[s]);
    return MSNAKE_OK;
}

// msnake_playout (eps_q16 NULL, not looked at) and msnake_playout_explore (explores = true)
int playout(const char* fn, msnake_handle h, const int32_t* policies, bool explores, const uint32_t* eps_q16, uint64_t salt, int32_t n_steps,
            const int32_t* first_dev, int32_t first_stride, uint32_t first_mask, int32_t* steps_dev, uint8_t* end_dev, float* ret_dev,
            int32_t* info_dev, int32_t* words_dev, int32_t words_stride, int32_t* count_dev, void* stream) {
    if (int rc = check(h)) return rc;
    const int ns = h->p.n_snakes;
    if (h->cfg.rules != MSNAKE_RULES_SNAKE_ENV)
        return fail(MSNAKE_E_ARG, "%s: snake_env handles only (rules %d): new_world judges its snakes one after the other, "
                                  "and the adversarial fruit list can grow to fcap entries", fn, h->cfg.rules);
    if (n_steps < 1 || n_steps > MSNAKE_PLAYOUT_MAX_STEPS)
        return fail(MSNAKE_E_ARG, "%s: n_steps %d must lie in [1, %d]", fn, n_steps, MSNAKE_PLAYOUT_MAX_STEPS);
    if (int rc = check_playout_policies(fn, policies, ns)) return rc;
    if (explores)
        if (int rc = check_eps(fn, eps_q16, ns)) return rc;
    if (int rc = check_hamiltonian_board(fn, policies, ns, h->p.dim)) return rc;
    if (first_mask >> ns) return fail(MSNAKE_E_ARG, "%s: first_mask 0x%x has a bit >= n_snakes=%d", fn, first_mask, ns);
    if (first_mask && !first_dev) return fail(MSNAKE_E_ARG, "%s: first_mask is 0x%x but first_dev is NULL", fn, first_mask);
    if (first_mask && first_stride < ns)
        return fail(MSNAKE_E_ARG, "%s: first_stride %d must be >= n_snakes=%d", fn, first_stride, ns);
    if (words_dev && words_stride <= 0) return fail(MSNAKE_E_ARG, "%s: words_dev is given but words_stride is %d", fn, words_stride);
    if (!steps_dev && !end_dev && !ret_dev && !info_dev && !words_dev && !count_dev)
        return fail(MSNAKE_E_ARG, "%s: nothing to write (steps_dev, end_dev, ret_dev, info_dev, words_dev and count_dev are NULL)", fn);
    if (((uintptr_t)first_dev & 3) || ((uintptr_t)steps_dev & 3) || ((uintptr_t)ret_dev & 3) || ((uintptr_t)info_dev & 3) ||
        ((uintptr_t)words_dev & 3) || ((uintptr_t)count_dev & 3))
        return fail(MSNAKE_E_ALIGN, "first_dev, steps_dev, ret_dev, info_dev, words_dev and count_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_playout(h->p, h->cfg.rules, policies, explores ? eps_q16 : nullptr, explore_seed(h->cfg.seed, salt), n_steps,
                                           first_mask ? first_dev : nullptr, first_stride, first_mask, steps_dev, end_dev, ret_dev, info_dev,
                                           words_dev, words_stride, count_dev, static_cast<hipStream_t>(stream)));
}

}  // namespace

int msnake_playout(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES], int32_t n_steps, const int32_t* first_dev,
                   int32_t first_stride, uint32_t first_mask, int32_t* steps_dev, uint8_t* end_dev, float* ret_dev, int32_t* info_dev,
                   int32_t* words_dev, int32_t words_stride, int32_t* count_dev, void* stream) {
    return playout("msnake_playout", h, policies, false, nullptr, 0, n_steps, first_dev, first_stride, first_mask, steps_dev, end_dev, ret_dev,
                   info_dev, words_dev, words_stride, count_dev, stream);
}

int msnake_playout_explore(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES], const uint32_t eps_q16[MSNAKE_MAX_SNAKES],
                           uint64_t salt, int32_t n_steps, const int32_t* first_dev, int32_t first_stride, uint32_t first_mask,
                           int32_t* steps_dev, uint8_t* end_dev, float* ret_dev, int32_t* info_dev, int32_t* words_dev,
                           int32_t words_stride, int32_t* count_dev, void* stream) {
    return playout("msnake_playout_explore", h, policies, true, eps_q16, salt, n_steps, first_dev, first_stride, first_mask, steps_dev, end_dev,
                   ret_dev, info_dev, words_dev, words_stride, count_dev, stream);
}

int msnake_explore_actions(msnake_handle h, const int32_t policies[MSNAKE_MAX_SNAKES], const uint32_t eps_q16[MSNAKE_MAX_SNAKES],
                           uint64_t salt, uint32_t snake_mask, int32_t* actions_dev, int32_t action_stride, uint8_t* explored_dev,
                           void* stream) {
    const char* fn = "msnake_explore_actions";
    if (int rc = check(h)) return rc;
    const int ns = h->p.n_snakes;
    if (int rc = check_playout_policies(fn, policies, ns)) return rc;
    for (int s = 0; s < ns; ++s)
        if (policies[s] == MSNAKE_POLICY_WARY_GREEDY && h->cfg.rules == MSNAKE_RULES_NEW_WORLD)
            return fail(MSNAKE_E_ARG, "%s: policy WARY_GREEDY needs snake_env or adversarial rules: new_world judges its snakes one after "
                                      "the other, so the fate of a move does not follow from the state", fn);
    if (int rc = check_hamiltonian_board(fn, policies, ns, h->p.dim)) return rc;
    if (int rc = check_eps(fn, eps_q16, ns)) return rc;
    if (!snake_mask) return fail(MSNAKE_E_ARG, "%s: snake_mask is 0 (no action to write)", fn);
    if (int rc = check_action_writer(fn, ns, true, snake_mask, actions_dev, action_stride)) return rc;
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_explore(h->p, h->cfg.rules, policies, eps_q16, explore_seed(h->cfg.seed, salt), snake_mask, actions_dev,
                                           action_stride, explored_dev, static_cast<hipStream_t>(stream)));
}

int msnake_head_fields(msnake_handle h, uint32_t snake_mask, uint16_t* dist_dev, uint8_t* owner_dev, uint16_t* counts_dev, void* stream) {
    if (int rc = check(h)) return rc;
    const int ns = h->p.n_snakes;
    if (snake_mask >> ns) return fail(MSNAKE_E_ARG, "msnake_head_fields: snake_mask 0x%x has a bit >= n_snakes=%d", snake_mask, ns);
    if (dist_dev && !snake_mask) return fail(MSNAKE_E_ARG, "msnake_head_fields: dist_dev is given but snake_mask is 0 (no plane to write)");
    if (!dist_dev && !owner_dev && !counts_dev)
        return fail(MSNAKE_E_ARG, "msnake_head_fields: nothing to write (dist_dev, owner_dev and counts_dev are NULL)");
    if ((uintptr_t)dist_dev & 1) return fail(MSNAKE_E_ALIGN, "dist_dev must be 2-byte aligned");
    if ((uintptr_t)counts_dev & 1) return fail(MSNAKE_E_ALIGN, "counts_dev must be 2-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_heads(h->p, h->cfg.rules, snake_mask, dist_dev, owner_dev, counts_dev, static_cast<hipStream_t>(stream)));
}

int msnake_copy_envs(msnake_handle dst, msnake_handle src, const int32_t* src_index_dev, void* stream) {
    if (int rc = check(dst)) return rc;
    if (int rc = check(src)) return rc;
    if (dst == src)
        return fail(MSNAKE_E_ARG, "msnake_copy_envs: src is the same handle as dst (copies within one handle are staged "
                                  "through a second handle)");
    const msnake_config &d = dst->cfg, &s = src->cfg;
    if (int rc = check_same_board("msnake_copy_envs", "src", s, "dst", d)) return rc;
    if (!src_index_dev && s.num_envs != d.num_envs)
        return fail(MSNAKE_E_ARG, "msnake_copy_envs: src_index_dev is NULL (the identity) but src has num_envs %d and dst has "
                                  "num_envs %d", s.num_envs, d.num_envs);
    if ((uintptr_t)src_index_dev & 3) return fail(MSNAKE_E_ALIGN, "src_index_dev must be 4-byte aligned");
    DeviceGuard guard(d.device);
    if (src->offgrid_head) note_offgrid_head(dst);
    return launched(msnake::launch_copy_envs(dst->p, src->p, d.rules, src_index_dev, static_cast<hipStream_t>(stream)));
}

int msnake_death_causes(msnake_handle after, msnake_handle before, uint8_t* cause_dev, uint8_t* by_dev, uint8_t* victims_dev,
                        int8_t* where_dev, void* stream) {
    if (int rc = check(after)) return rc;
    if (int rc = check(before)) return rc;
    if (after == before)
        return fail(MSNAKE_E_ARG, "msnake_death_causes: before is the same handle as after (the state in front of the step is "
                                  "kept in a second handle, msnake_copy_envs(before, after, NULL, stream))");
    const msnake_config &a = after->cfg, &b = before->cfg;
    if (int rc = check_same_board("msnake_death_causes", "before", b, "after", a)) return rc;
    if (b.num_envs != a.num_envs)
        return fail(MSNAKE_E_ARG, "msnake_death_causes: before has num_envs %d, after has num_envs %d", b.num_envs, a.num_envs);
    if (a.rules == MSNAKE_RULES_NEW_WORLD)
        return fail(MSNAKE_E_ARG, "msnake_death_causes: new_world judges its snakes one after the other and clears bodies as it "
                                  "goes, so the bodies a snake was judged against cannot be rebuilt from two states");
    if (after->p.auto_reset)
        return fail(MSNAKE_E_ARG, "msnake_death_causes: the handle `after` resets done envs inside the step (auto_reset = 1), so "
                                  "their after-state is gone; create it with auto_reset = 0 and follow the step with msnake_reset_envs");
    if (!cause_dev && !by_dev && !victims_dev && !where_dev)
        return fail(MSNAKE_E_ARG, "msnake_death_causes: nothing to write (cause_dev, by_dev, victims_dev and where_dev are NULL)");
    DeviceGuard guard(a.device);
    return launched(msnake::launch_death_causes(after->p, before->p, a.rules, cause_dev, by_dev, victims_dev, where_dev,
                                                static_cast<hipStream_t>(stream)));
}

int msnake_render_cells(msnake_handle h, uint32_t view_mask, uint8_t* cells_dev, int32_t* snakes_dev, void* stream) {
    if (int rc = check(h)) return rc;
    const int views = h->p.views;
    if (view_mask >> views) return fail(MSNAKE_E_ARG, "msnake_render_cells: view_mask 0x%x has a bit >= views=%d", view_mask, views);
    if (view_mask && !cells_dev) return fail(MSNAKE_E_ARG, "msnake_render_cells: cells_dev is NULL but view_mask is 0x%x", view_mask);
    if (!view_mask && cells_dev) return fail(MSNAKE_E_ARG, "msnake_render_cells: cells_dev is given but view_mask is 0");
    if (!view_mask && !snakes_dev)
        return fail(MSNAKE_E_ARG, "msnake_render_cells: nothing to write (view_mask 0 and snakes_dev is NULL)");
    if ((uintptr_t)snakes_dev & 3) return fail(MSNAKE_E_ALIGN, "snakes_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_cells(h->p, h->cfg.rules, view_mask, cells_dev, snakes_dev, static_cast<hipStream_t>(stream)));
}

int msnake_render_local(msnake_handle h, int32_t radius, uint32_t snake_mask, int32_t oriented, uint8_t* windows_dev,
                        uint8_t* heading_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (radius < 1 || radius > MSNAKE_LOCAL_MAX_RADIUS)
        return fail(MSNAKE_E_ARG, "msnake_render_local: radius %d must lie in [1, %d]", radius, MSNAKE_LOCAL_MAX_RADIUS);
    if (int rc = check_snake_view("msnake_render_local", "window", h->p.n_snakes, snake_mask, oriented)) return rc;
    if (!windows_dev) return fail(MSNAKE_E_ARG, "msnake_render_local: windows_dev is NULL");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_local(h->p, h->cfg.rules, radius, snake_mask, oriented, windows_dev, heading_dev,
                                         static_cast<hipStream_t>(stream)));
}

int msnake_render_rays(msnake_handle h, uint32_t snake_mask, int32_t oriented, uint8_t* rays_dev, uint8_t* heading_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (int rc = check_snake_view("msnake_render_rays", "rays", h->p.n_snakes, snake_mask, oriented)) return rc;
    if (!rays_dev) return fail(MSNAKE_E_ARG, "msnake_render_rays: rays_dev is NULL");
    if ((uintptr_t)rays_dev & 3) return fail(MSNAKE_E_ALIGN, "rays_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_rays(h->p, h->cfg.rules, snake_mask, oriented, rays_dev, heading_dev, static_cast<hipStream_t>(stream)));
}

int msnake_agent_outcomes(msnake_handle h, int32_t flags, int32_t* track_dev, const uint8_t* done_dev, float* rew_dev,
                          uint8_t* ate_dev, uint8_t* flags_dev, int32_t* info_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (flags & ~MSNAKE_AGENT_ARM) return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: flags 0x%x has bits other than MSNAKE_AGENT_ARM", flags);
    if (!track_dev) return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: track_dev is NULL");
    const bool arm = (flags & MSNAKE_AGENT_ARM) != 0, any_out = rew_dev || ate_dev || flags_dev || info_dev;
    if (arm && (done_dev || any_out))
        return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: arming produces no outcome (done_dev and the four outputs must be NULL)");
    if (!arm && !done_dev) return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: done_dev is NULL (the step's done output)");
    if (!arm && !any_out) return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: nothing to write (rew_dev, ate_dev, flags_dev and info_dev are NULL)");
    if (h->p.auto_reset)
        return fail(MSNAKE_E_ARG, "msnake_agent_outcomes: the handle resets done envs inside the step (auto_reset = 1), so their "
                                  "terminal state is gone; create it with auto_reset = 0 and follow the step with msnake_reset_envs");
    if (((uintptr_t)track_dev | (uintptr_t)rew_dev | (uintptr_t)info_dev) & 3)
        return fail(MSNAKE_E_ALIGN, "track_dev, rew_dev and info_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_agents(h->p, h->cfg.rules, arm, track_dev, done_dev, rew_dev, ate_dev, flags_dev, info_dev,
                                          static_cast<hipStream_t>(stream)));
}

// ---- canonical state import / export.  The device packs / unpacks (msnake_state_*_kernel); the host
//      only sizes buffers and copies.  Blocking: every call starts with a device synchronise. ----
namespace {

struct BlobHeader {  // msnake_get_state_all / msnake_set_state_all
    uint32_t magic, version;
    int32_t num_envs, dim, n_snakes, n_fruits, rules, reserved;
    uint64_t total_words;
};
constexpr uint32_t kBlobMagic = 0x5453534Du;  // "MSST"
constexpr uint32_t kBlobVersion = 2u;         // 2: word 7 of an env's words carries the "episode finished" bit

// need[i] (words) of envs [env0, env0 + count) -> host; offsets[count + 1] prefix sums
int state_offsets(msnake_env* h, int env0, int count, std::vector<uint64_t>& offsets) {
    if (int rc = ensure_scratch(h, (size_t)count * 4)) return rc;
    HIP_TRY(msnake::launch_state_sizes(h->p, h->cfg.rules, env0, count, static_cast<uint32_t*>(h->d_scratch), nullptr));
    std::vector<uint32_t> need((size_t)count);
    HIP_TRY(hipMemcpy(need.data(), h->d_scratch, (size_t)count * 4, hipMemcpyDeviceToHost));
    offsets.assign((size_t)count + 1, 0);
    for (int i = 0; i < count; ++i) offsets[(size_t)i + 1] = offsets[(size_t)i] + need[(size_t)i];
    return MSNAKE_OK;
}

// words of envs [env0, env0 + count) at `offsets` -> host buffer `out`
int state_export(msnake_env* h, int env0, int count, const std::vector<uint64_t>& offsets, int32_t* out) {
    const size_t off_bytes = ((size_t)count + 1) * 8, word_bytes = (size_t)offsets.back() * 4;
    if (int rc = ensure_scratch(h, off_bytes + word_bytes)) return rc;
    uint8_t* d = static_cast<uint8_t*>(h->d_scratch);
    HIP_TRY(hipMemcpy(d, offsets.data(), off_bytes, hipMemcpyHostToDevice));
    HIP_TRY(msnake::launch_state_pack(h->p, h->cfg.rules, env0, count, reinterpret_cast<const uint64_t*>(d),
                                      reinterpret_cast<int32_t*>(d + off_bytes), nullptr));
    HIP_TRY(hipMemcpy(out, d + off_bytes, word_bytes, hipMemcpyDeviceToHost));
    return MSNAKE_OK;
}

int state_import(msnake_env* h, int env0, int count, const uint64_t* offsets, const int32_t* words) {
    const size_t off_bytes = ((size_t)count + 1) * 8, word_bytes = (size_t)offsets[count] * 4;
    if (int rc = ensure_scratch(h, 16 + off_bytes + word_bytes)) return rc;
    uint8_t* d = static_cast<uint8_t*>(h->d_scratch);
    // [0] rejected envs, [1] min over them of status_pack(local index, reason), [2] != 0: an accepted env has a head outside the grid
    const uint32_t st0[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
    HIP_TRY(hipMemcpy(d, st0, 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + 16, offsets, off_bytes, hipMemcpyHostToDevice));
    if (word_bytes) HIP_TRY(hipMemcpy(d + 16 + off_bytes, words, word_bytes, hipMemcpyHostToDevice));
    HIP_TRY(msnake::launch_state_unpack(h->p, h->cfg.rules, env0, count, reinterpret_cast<const uint64_t*>(d + 16),
                                        reinterpret_cast<const int32_t*>(d + 16 + off_bytes),
                                        reinterpret_cast<uint32_t*>(d), nullptr));
    uint32_t st[4];
    HIP_TRY(hipMemcpy(st, d, 16, hipMemcpyDeviceToHost));
    if (st[2] != 0) note_offgrid_head(h);  // some accepted env has a head outside the grid
    if (st[0] != 0)
        return fail(MSNAKE_E_STATE, "%u env state(s) rejected; first: env %d: %s (the rejected envs were left untouched)", st[0],
                    env0 + msnake::status_env(st[1]), state_reason(msnake::status_reason(st[1])));
    return MSNAKE_OK;
}

}  // namespace

int msnake_get_state(msnake_handle h, int32_t env, int32_t* words, int32_t cap_words) {
    if (int rc = check(h)) return rc;
    if (env < 0 || env >= h->p.nenv) return fail(MSNAKE_E_ARG, "env %d out of range", env);
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint64_t> offsets;
    if (int rc = state_offsets(h, env, 1, offsets)) return rc;
    const int32_t need = (int32_t)offsets[1];
    if (!words || cap_words < need) return need;
    if (int rc = state_export(h, env, 1, offsets, words)) return rc;
    return need;
}

int msnake_set_state(msnake_handle h, int32_t env, const int32_t* words, int32_t n) {
    if (int rc = check(h)) return rc;
    if (env < 0 || env >= h->p.nenv) return fail(MSNAKE_E_ARG, "env %d out of range", env);
    if (!words || n < 8) return fail(MSNAKE_E_STATE, "state buffer too short");
    if ((words[7] & 0xFF) != h->p.n_snakes) return fail(MSNAKE_E_STATE, "state has %d snakes, handle has %d", words[7] & 0xFF, h->p.n_snakes);
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const uint64_t offsets[2] = {0, (uint64_t)n};
    return state_import(h, env, 1, offsets, words);
}

int64_t msnake_get_state_all(msnake_handle h, void* buf, size_t cap_bytes) {
    if (int rc = check(h)) return rc;
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    const int n = h->p.nenv;
    std::vector<uint64_t> offsets;
    if (int rc = state_offsets(h, 0, n, offsets)) return rc;
    const size_t head = sizeof(BlobHeader) + ((size_t)n + 1) * 8;
    const size_t need = head + (size_t)offsets.back() * 4;
    if (!buf || cap_bytes < need) return (int64_t)need;
    BlobHeader bh = {kBlobMagic, kBlobVersion, n, h->p.dim, h->p.n_snakes, h->p.n_fruits, h->cfg.rules, 0, offsets.back()};
    uint8_t* out = static_cast<uint8_t*>(buf);
    memcpy(out, &bh, sizeof(bh));
    memcpy(out + sizeof(bh), offsets.data(), ((size_t)n + 1) * 8);
    if (int rc = state_export(h, 0, n, offsets, reinterpret_cast<int32_t*>(out + head))) return rc;
    return (int64_t)need;
}

int msnake_state_blob_info(const void* buf, size_t bytes, msnake_blob_info* out) {
    // host-only: header, offset table and length of a msnake_get_state_all blob, before any handle exists
    if (!buf || bytes < sizeof(BlobHeader)) return fail(MSNAKE_E_STATE, "state blob too short");
    BlobHeader bh;
    memcpy(&bh, buf, sizeof(bh));
    if (bh.magic != kBlobMagic || (bh.version != 1u && bh.version != kBlobVersion))
        return fail(MSNAKE_E_STATE, "not an msnake state blob (magic/version)");
    if (bh.num_envs < 1) return fail(MSNAKE_E_STATE, "state blob: num_envs %d", bh.num_envs);
    const size_t n = (size_t)bh.num_envs;
    if ((bytes - sizeof(BlobHeader)) / 8 < n + 1) return fail(MSNAKE_E_STATE, "state blob truncated in its offset table");
    const size_t head = sizeof(BlobHeader) + (n + 1) * 8;
    const uint8_t* offp = static_cast<const uint8_t*>(buf) + sizeof(bh);
    uint64_t prev = 0, last = 0;
    memcpy(&prev, offp, 8);
    memcpy(&last, offp + n * 8, 8);
    // (the word count is bounded BEFORE it is multiplied: 2^62 words * 4 would wrap to 0 and pass a byte comparison)
    if (prev != 0 || last != bh.total_words || bh.total_words > (uint64_t)(bytes - head) / 4)
        return fail(MSNAKE_E_STATE, "state blob truncated or its offset table is inconsistent");
    for (size_t i = 1; i <= n; ++i) {
        uint64_t cur;
        memcpy(&cur, offp + i * 8, 8);
        if (cur < prev) return fail(MSNAKE_E_STATE, "state blob: offsets of env %zu decrease", i - 1);
        prev = cur;
    }
    if (out) {
        out->version = (int32_t)bh.version; out->num_envs = bh.num_envs; out->dim = bh.dim; out->n_snakes = bh.n_snakes;
        out->n_fruits = bh.n_fruits; out->rules = bh.rules; out->total_words = (int64_t)bh.total_words;
    }
    return MSNAKE_OK;
}

int msnake_set_state_all(msnake_handle h, const void* buf, size_t bytes) {
    if (int rc = check(h)) return rc;
    msnake_blob_info bi;
    if (int rc = msnake_state_blob_info(buf, bytes, &bi)) return rc;
    const msnake::StepParams& p = h->p;
    if (bi.num_envs != p.nenv || bi.dim != p.dim || bi.n_snakes != p.n_snakes || bi.rules != h->cfg.rules ||
        (h->cfg.rules != MSNAKE_RULES_ADVERSARIAL && bi.n_fruits != p.n_fruits))
        return fail(MSNAKE_E_STATE, "state blob is for %d envs, dim %d, %d snakes, %d fruits, rules %d; the handle differs",
                    bi.num_envs, bi.dim, bi.n_snakes, bi.n_fruits, bi.rules);
    const size_t n = (size_t)p.nenv, head = sizeof(BlobHeader) + (n + 1) * 8;
    std::vector<uint64_t> offsets(n + 1);
    memcpy(offsets.data(), static_cast<const uint8_t*>(buf) + sizeof(BlobHeader), (n + 1) * 8);
    DeviceGuard guard(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    return state_import(h, 0, p.nenv, offsets.data(),
                        reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(buf) + head));
}

// ---- the same words as a device tensor: one launch each, nothing allocated, nothing synchronised ----
int32_t msnake_state_words_max(msnake_handle h) {
    if (int rc = check(h)) return rc;
    const msnake::StepParams& p = h->p;
    const int F = h->cfg.rules == MSNAKE_RULES_ADVERSARIAL ? p.fcap : p.n_fruits;
    return 8 + 2 * F + p.n_snakes * (6 + 2 * (p.rest.cap - 2));
}

int msnake_export_states(msnake_handle h, int32_t* words_dev, int32_t stride, int32_t* count_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (stride < 0) return fail(MSNAKE_E_ARG, "msnake_export_states: stride %d < 0", stride);
    if (words_dev && stride == 0) return fail(MSNAKE_E_ARG, "msnake_export_states: words_dev is given but stride is 0");
    if (!words_dev && !count_dev) return fail(MSNAKE_E_ARG, "msnake_export_states: nothing to write (words_dev and count_dev are NULL)");
    if (((uintptr_t)words_dev | (uintptr_t)count_dev) & 3) return fail(MSNAKE_E_ALIGN, "words_dev and count_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_state_export(h->p, h->cfg.rules, words_dev, stride, count_dev, static_cast<hipStream_t>(stream)));
}

int msnake_import_states(msnake_handle h, const uint8_t* mask_dev, const int32_t* words_dev, int32_t stride,
                         const int32_t* count_dev, uint8_t* status_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (!words_dev || !status_dev) return fail(MSNAKE_E_ARG, "msnake_import_states: words_dev and status_dev must not be NULL");
    if (stride < 8) return fail(MSNAKE_E_ARG, "msnake_import_states: stride %d < 8 (no state has fewer words)", stride);
    if (((uintptr_t)words_dev | (uintptr_t)count_dev) & 3) return fail(MSNAKE_E_ALIGN, "words_dev and count_dev must be 4-byte aligned");
    DeviceGuard guard(h->cfg.device);
    // a head outside the grid: the kernels compiled for a shape cannot follow it (note_offgrid_head) and the host will not
    // hear of it, so such a handle refuses the row; a handle on the generic kernels takes it and counts as holding one
    const bool refuse = h->p.spec_dim != 0;
    int rc = launched(msnake::launch_state_import(h->p, h->cfg.rules, mask_dev, words_dev, stride, count_dev, status_dev, refuse,
                                                  static_cast<hipStream_t>(stream)));
    if (rc == MSNAKE_OK && !refuse) h->offgrid_head = 1;
    return rc;
}

int msnake_generate_states(msnake_handle h, const uint8_t* mask_dev, const int32_t* len_dev, int32_t len_stride, uint32_t flags,
                           uint64_t salt, int32_t* words_dev, int32_t stride, int32_t* count_dev, int32_t* got_dev, void* stream) {
    if (int rc = check(h)) return rc;
    const int ns = h->p.n_snakes;
    if (h->cfg.rules == MSNAKE_RULES_NEW_WORLD)
        return fail(MSNAKE_E_ARG, "msnake_generate_states: new_world keeps alive and in_dead bits per snake and draws its first "
                                  "positions by another contract; snake_env and adversarial handles only");
    if (flags & ~MSNAKE_GEN_COMPACT) return fail(MSNAKE_E_ARG, "msnake_generate_states: unknown flag bits 0x%x", flags & ~MSNAKE_GEN_COMPACT);
    if (!len_dev) return fail(MSNAKE_E_ARG, "msnake_generate_states: len_dev is NULL");
    if (len_stride < ns) return fail(MSNAKE_E_ARG, "msnake_generate_states: len_stride %d must be >= n_snakes=%d", len_stride, ns);
    if (words_dev && stride <= 0) return fail(MSNAKE_E_ARG, "msnake_generate_states: words_dev is given but stride is %d", stride);
    if (!words_dev && !count_dev && !got_dev)
        return fail(MSNAKE_E_ARG, "msnake_generate_states: nothing to write (words_dev, count_dev and got_dev are NULL)");
    if (((uintptr_t)len_dev | (uintptr_t)words_dev | (uintptr_t)count_dev | (uintptr_t)got_dev) & 3)
        return fail(MSNAKE_E_ALIGN, "len_dev, words_dev, count_dev and got_dev must be 4-byte aligned");
    const uint64_t gseed = mix64(h->cfg.seed ^ mix64(salt ^ 0x67656E6572617465ull));  // "generate"
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_generate(h->p, mask_dev, len_dev, len_stride, (flags & MSNAKE_GEN_COMPACT) != 0, gseed, words_dev,
                                            words_dev ? stride : 0, count_dev, got_dev, static_cast<hipStream_t>(stream)));
}

int msnake_hash_states(msnake_handle h, uint32_t what, uint64_t* hash_dev, void* stream) {
    if (int rc = check(h)) return rc;
    if (what != MSNAKE_HASH_FULL && what != MSNAKE_HASH_BOARD)
        return fail(MSNAKE_E_ARG, "msnake_hash_states: what %u is neither MSNAKE_HASH_FULL nor MSNAKE_HASH_BOARD", what);
    if (!hash_dev) return fail(MSNAKE_E_ARG, "msnake_hash_states: hash_dev is NULL");
    if ((uintptr_t)hash_dev & 7) return fail(MSNAKE_E_ALIGN, "hash_dev must be 8-byte aligned");
    DeviceGuard guard(h->cfg.device);
    return launched(msnake::launch_state_hash(h->p, h->cfg.rules, what == MSNAKE_HASH_BOARD, hash_dev, static_cast<hipStream_t>(stream)));
}

int msnake_get_stats(msnake_handle h, msnake_stats* out, int32_t reset) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(MSNAKE_E_ARG, "msnake_get_stats: out is NULL");
    DeviceGuard guard(h->cfg.device);
    // the totals live in the env records; sum (and optionally clear) them once every step issued so
    // far, on whatever stream, has finished (no stream handle is remembered between calls)
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemsetAsync(h->d_stats, 0, 64, nullptr));
    HIP_TRY(msnake::launch_stats(h->p.hdr, h->p.nenv, h->p.stats, reset ? 1 : 0, nullptr));
    unsigned long long raw[8];
    HIP_TRY(hipMemcpy(raw, h->d_stats, sizeof(raw), hipMemcpyDeviceToHost));
    memset(out, 0, sizeof(*out));
    out->episodes = (int64_t)raw[0];
    out->ep_len_sum = (int64_t)raw[1];
    out->ep_return_sum = (int64_t)raw[2];
    out->env_steps = h->env_steps;
    out->errors = (int64_t)raw[4];
    if (reset) h->env_steps = 0;
    return MSNAKE_OK;
}

const char* msnake_kernel_name(msnake_handle h) {
    if (check(h)) return "";
    return h->kname;  // owned by the handle: valid until msnake_destroy
}

int msnake_kernel_name_for_config(const msnake_config* cfg_in, char* out, size_t n) {
    if (!cfg_in || !out || n == 0) return fail(MSNAKE_E_ARG, "msnake_kernel_name_for_config: NULL argument");
    msnake_config cfg;
    msnake::StepParams p;
    if (int rc = shape_for_config(cfg_in, &cfg, p)) return rc;
    msnake::step_kernel_name(cfg.rules, cfg.n_snakes, cfg.obs_scale, p.spec_dim, out, n);
    return MSNAKE_OK;
}

int msnake_call_shape_for_config(const msnake_config* cfg_in, int32_t action_stride, const void* obs_dev, const void* rew_dev,
                                 const void* done_dev, const void* info_dev, int32_t* out) {
    if (!cfg_in || !out) return fail(MSNAKE_E_ARG, "msnake_call_shape_for_config: NULL argument");
    msnake_config cfg;
    msnake::StepParams p;
    if (int rc = shape_for_config(cfg_in, &cfg, p)) return rc;
    if (int rc = check_action_stride(action_stride, p.n_snakes)) return rc;
    fill_call(p, nullptr, action_stride, static_cast<uint8_t*>(const_cast<void*>(obs_dev)), static_cast<float*>(const_cast<void*>(rew_dev)),
              static_cast<uint8_t*>(const_cast<void*>(done_dev)), static_cast<msnake_info*>(const_cast<void*>(info_dev)));
    *out = msnake::call_shape_of(p, 0);
    return MSNAKE_OK;
}

int msnake_launch_shape_for_config(const msnake_config* cfg_in, int32_t* step_epb, int32_t* tape_epb) {
    if (!cfg_in) return fail(MSNAKE_E_ARG, "msnake_launch_shape_for_config: NULL argument");
    msnake_config cfg;
    msnake::StepParams p;
    if (int rc = shape_for_config(cfg_in, &cfg, p)) return rc;
    const int epb = pick_epb(&cfg, p);
    if (step_epb) *step_epb = epb;
    if (tape_epb) *tape_epb = pick_tape_epb(p, epb);
    return MSNAKE_OK;
}

int msnake_set_generic_kernels(int32_t on) { return g_generic_kernels.exchange(on ? 1 : 0, std::memory_order_relaxed); }

int64_t msnake_algorithmic_bytes_per_env_step(msnake_handle h) {
    if (check(h)) return -1;
    // obs write + one read of per-cell occupancy + actions + reward/done +
    // per-snake and per-env scalar read-modify-write
    const msnake::StepParams& p = h->p;
    return (int64_t)p.S * p.obs_scale * p.obs_scale + (int64_t)p.dim * p.dim + 4 * p.n_snakes + 5 + 16 * p.n_snakes + 16;
}

}  // extern "C"
