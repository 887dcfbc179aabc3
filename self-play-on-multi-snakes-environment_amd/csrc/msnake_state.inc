// msnake_state.inc -- the canonical state words (include/msnake.h) <-> the device layout (msnake_get_state[_all] /
// msnake_set_state[_all]; checkpoint and test path).  Included first by msnake_views.hip: it uses msnake_device.h's wave
// helpers and HV_SET macros.  Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per env (the sizes kernel: one thread).  Export reads through EnvReader (msnake_envread.inc); import
// validates everything before it writes anything, and a rejected env is left untouched.
// Each direction is ONE body with two kernels around it: the blocking entry points find a row through a host-built
// offset table and report through one global status triple; msnake_export_states / msnake_import_states (asynchronous,
// every env of the handle) find it at e * stride and report one count and one status byte per env.
namespace msnake {

__global__ __launch_bounds__(256) void msnake_state_sizes_kernel(StateView v, int env0, int count, uint32_t* __restrict__ need) {
    const int w = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (w >= count) return;
    const uint32_t* h = v.hdr + (size_t)(env0 + w) * MSNAKE_HDR_WORDS;
    uint32_t n = 8u + 2u * (uint32_t)fruit_count(v, h[HDR_NLIST]);
    for (int s = 0; s < v.ns; ++s) n += 6u + 2u * (h[SN_A(s)] >> 16);
    need[w] = n;
}

// Where a packed env's words go.  A row source answers row(rd): the first word of the env's row, or -- only a source
// with kMayDecline -- NULL for "write no word of this env".  The blocking entry points address rows through a host-built
// table of word offsets; msnake_export_states through e * stride, and says how many words the env has on the way.
struct RowsByOffset {
    static constexpr bool kMayDecline = false;
    const uint64_t* __restrict__ offsets; int32_t* __restrict__ words; int w;
    __device__ __forceinline__ int32_t* row(const EnvReader&) const { return words + offsets[w]; }
};
struct RowsByStride {
    static constexpr bool kMayDecline = true;
    int32_t* __restrict__ words; int32_t* __restrict__ count; int32_t stride;
    __device__ __forceinline__ int32_t* row(const EnvReader& rd) const {
        uint32_t n = 8u + 2u * (uint32_t)rd.n_fruits();  // (what msnake_state_sizes_kernel counts)
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            if (s < rd.v.ns) n += 6u + 2u * (rd.word(SN_A(s)) >> 16);
        if (count && rd.lane == 0) count[rd.e] = (int32_t)n;
        return words && n <= (uint32_t)stride ? words + (size_t)rd.e * (size_t)stride : nullptr;
    }
};

// env e's canonical words, by the wave that reads it
template <typename Rows>
__device__ __forceinline__ void state_pack_env(const StateView& v, int e, int lane, const Rows& rows) {
    const EnvReader rd(v, e, lane);
    int32_t* out = rows.row(rd);
    if (Rows::kMayDecline && !out) return;
    const bool nw = v.rules == MSNAKE_RULES_NEW_WORLD;
    const int nfr = rd.n_fruits();
    const uint32_t flags = rd.flags();
    if (lane == 0) {
        out[0] = (int32_t)rd.word(HDR_T); out[1] = (int32_t)rd.word(HDR_CTR_LO); out[2] = (int32_t)rd.word(HDR_CTR_HI);
        out[3] = (int32_t)rd.word(HDR_SPARE); out[4] = (int32_t)rd.word(HDR_EP_LEN); out[5] = (int32_t)rd.word(HDR_EP_RETURN);
        out[6] = nfr; out[7] = v.ns | ((flags & HDR_FLAG_FINISHED) ? 0x100 : 0);
    }
    size_t k = 8;
    rd.for_each_fruit([&](int f, uint32_t c, bool valid) {
        if (valid) {
            out[k + 2 * f] = cell_c0(c);
            out[k + 2 * f + 1] = cell_c1(c);
        }
    });
    k += 2 * (size_t)nfr;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= v.ns) continue;
        const SnakeRef sn = rd.snake(s);
        const int len = sn.len, vel = (int)((rd.word(SN_C(s)) >> 16) & 7u);
        if (lane == 0) {
            out[k] = len;
            out[k + 1] = vel_v0(vel);
            out[k + 2] = vel_v1(vel);
            out[k + 3] = (int32_t)rd.word(SN_B(s));
            out[k + 4] = snake_alive(flags, s, nw);
            out[k + 5] = snake_in_dead(flags, s, nw);
        }
        rd.for_each_piece(sn, [&](int i, uint32_t c, bool valid) {
            if (valid) {
                out[k + 6 + 2 * (size_t)i] = cell_c0(c);
                out[k + 6 + 2 * (size_t)i + 1] = cell_c1(c);
            }
        });
        k += 6 + 2 * (size_t)len;
    }
}

__global__ __launch_bounds__(256) void msnake_state_pack_kernel(StateView v, int env0, int count,
                                                                const uint64_t* __restrict__ offsets, int32_t* __restrict__ words) {
    const int lane = (int)(threadIdx.x & 63u);
    const int w = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (w >= count) return;
    state_pack_env(v, env0 + w, lane, RowsByOffset{offsets, words, w});
}

// msnake_export_states: row e of words[nenv][stride] and count[e]; either of the two may be NULL
__global__ __launch_bounds__(256) void msnake_state_export_kernel(StateView v, int32_t* __restrict__ words, int32_t stride,
                                                                  int32_t* __restrict__ count) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= v.nenv) return;
    state_pack_env(v, e, lane, RowsByStride{words, count, stride});
}

// status[0]: number of rejected envs, status[1]: min over them of status_pack(local index, MSNAKE_ST_* reason) (ONE
// atomicMin on ~0u: index and reason of the first rejected env cannot come from two different waves), status[2]: != 0 if
// an accepted env has a head outside the grid
struct StatusGlobal {
    // (the blocking entry points learn of a head outside the grid from status[2] and move the handle to the generic kernels)
    static constexpr bool kRefusesOffgridHead = false;
    uint32_t* __restrict__ status; int w;
    __device__ __forceinline__ bool refuses_offgrid_head() const { return false; }
    __device__ __forceinline__ void reject(int lane, int reason) const {
        if (lane == 0) {
            atomicAdd(&status[0], 1u);
            atomicMin(&status[1], status_pack(w, reason));
        }
    }
    __device__ __forceinline__ void accept(int, bool off_head) const {
        if (off_head) atomicOr(&status[2], 1u);
    }
};
// msnake_import_states: one status byte per env, MSNAKE_STATE_OK or the MSNAKE_ST_* reason.  `refuse` (wave-uniform): a
// head outside the grid is reason "cell" -- the host cannot learn of one without a sync, and the step kernels compiled
// for a shape cannot draw what such a head leaves behind (note_offgrid_head in msnake_capi.hip)
struct StatusPerEnv {
    static constexpr bool kRefusesOffgridHead = true;
    uint8_t* __restrict__ status; int e; bool refuse;
    __device__ __forceinline__ bool refuses_offgrid_head() const { return refuse; }
    __device__ __forceinline__ void reject(int lane, int reason) const {
        if (lane == 0) status[e] = (uint8_t)reason;
    }
    __device__ __forceinline__ void accept(int lane, bool) const {
        if (lane == 0) status[e] = (uint8_t)MSNAKE_STATE_OK;
    }
};

// the n words at `in` into env e, by one wave: validated as a whole, then written; the verdict goes to `sink`
template <typename Sink>
__device__ __forceinline__ void state_unpack_env(const StateView& v, int e, int lane, const int32_t* __restrict__ in, long long n,
                                                 const Sink& sink) {
    const bool adv = v.rules == MSNAKE_RULES_ADVERSARIAL, nw = v.rules == MSNAKE_RULES_NEW_WORLD;
    auto cell_ok = [&](int c0, int c1) { return c0 >= -1 && c0 <= v.dim && c1 >= -1 && c1 <= v.dim; };
    // ---- pass 1: validate everything before anything is written
    int bad = 0;
    int nfr = 0;
    bool off_head = false;  // (lane 0) some head lies outside the grid: reported in status[2] if the env is accepted
    if (n < 8) bad = MSNAKE_ST_SHORT;
    else if ((in[7] & ~0x100) != v.ns) bad = MSNAKE_ST_SNAKES;  // (bit 8: the episode-finished flag)
    // counters that play only ever raises from 0; a negative spare_fruits also stops the reference's respawns for good
    // ([A]:137-141 tests > 0 and == 0).  t has no upper bound: a handle with a lower episode cap may receive any t
    else if (in[0] < 0 || in[3] < 0 || in[4] < 0) bad = MSNAKE_ST_SCALAR;
    else {
        nfr = in[6];
        if (adv ? (nfr < 0 || nfr > v.fcap) : nfr != v.nf) bad = MSNAKE_ST_FRUITS;
        else if (n < 8 + 2LL * nfr) bad = MSNAKE_ST_SHORT;
    }
    long long k = 8;
    if (!bad) {
        bool okc = true;
        for (int f = lane; f < nfr; f += 64) {
            const int c0 = in[k + 2 * f], c1 = in[k + 2 * f + 1];
            // the adversarial fruit list may hold the off-grid head of a dead snake ([A]:183-185); the inline
            // fruits of the other rule sets are only ever placed inside the grid
            okc = okc && (adv ? cell_ok(c0, c1) : (c0 >= 0 && c0 < v.dim && c1 >= 0 && c1 < v.dim));
        }
        if (__builtin_amdgcn_ballot_w64(!okc) != 0) bad = MSNAKE_ST_CELL;
        k += 2LL * nfr;
    }
    for (int s = 0; s < v.ns && !bad; ++s) {
        if (n < k + 6) { bad = MSNAKE_ST_SHORT; break; }
        const int len = in[k];
        if (len < 0 || len > v.cap - 2) { bad = MSNAKE_ST_LEN; break; }
        if (n < k + 6 + 2LL * len) { bad = MSNAKE_ST_SHORT; break; }
        // what the record cannot hold, or holds as something else: a velocity that is not one of the five, a bit that is
        // not 0 / 1, a negative grow_to (the vector update compares it unsigned); without the new_world bits a snake
        // is alive and not in dead_snakes, which is what the export says there
        const int v0 = in[k + 1], v1 = in[k + 2], al = in[k + 4], ind = in[k + 5];
        const bool vel_ok = (v0 == 0 && (v1 >= -1 && v1 <= 1)) || (v1 == 0 && (v0 == -1 || v0 == 1));
        const bool bits_ok = nw ? ((al == 0 || al == 1) && (ind == 0 || ind == 1)) : (al == 1 && ind == 0);
        if (!vel_ok || in[k + 3] < 0 || !bits_ok) { bad = MSNAKE_ST_SCALAR; break; }
        bool okc = true;
        for (int i = lane; i < len; i += 64) {
            const int c0 = in[k + 6 + 2LL * i], c1 = in[k + 6 + 2LL * i + 1];
            okc = okc && cell_ok(c0, c1);
            if (i == 0) {
                const bool off = !(c0 >= 0 && c0 < v.dim && c1 >= 0 && c1 < v.dim);
                off_head = off_head || off;
                if (Sink::kRefusesOffgridHead && sink.refuses_offgrid_head()) okc = okc && !off;
            }
            // only a head may be one step outside the grid (where a reference snake can be, for one step)
            if (i > 0) okc = okc && c0 >= 0 && c0 < v.dim && c1 >= 0 && c1 < v.dim;
        }
        if (__builtin_amdgcn_ballot_w64(!okc) != 0) { bad = MSNAKE_ST_CELL; break; }
        k += 6 + 2LL * len;
    }
    if (bad) {
        sink.reject(lane, bad);
        return;
    }
    sink.accept(lane, off_head);
    // ---- pass 2: the record (lane l builds word l; logging totals are not part of the canonical
    //      state and stay; every other word, the parked Philox draws included, is cleared)
    uint32_t* h = v.hdr + (size_t)e * MSNAKE_HDR_WORDS;
    uint32_t hv = (lane >= HDR_ACC_EPISODES && lane <= HDR_ACC_LEN_HI) ? h[lane] : 0u;
    HV_SET_C(HDR_T, in[0]); HV_SET_C(HDR_CTR_LO, in[1]); HV_SET_C(HDR_CTR_HI, in[2]); HV_SET_C(HDR_SPARE, in[3]);
    HV_SET_C(HDR_EP_LEN, in[4]); HV_SET_C(HDR_EP_RETURN, in[5]);
    if (adv) HV_SET_C(HDR_NLIST, nfr);
    k = 8;
    const int fr0 = nw ? HDR_FRUIT0_N : HDR_FRUIT0_S;
    for (int f = lane; f < nfr; f += 64) {
        const uint32_t c = cell_pack(in[k + 2 * f], in[k + 2 * f + 1]);
        if (adv) {
            v.flist[(size_t)e * v.fcap + f] = (uint16_t)c;
            if (f < 64) v.fl0[(size_t)e * 64 + f] = (uint16_t)c;
        }
    }
    if (!adv)
        for (int f = 0; f < nfr; ++f)
            HV_SET(fr0 + f, cell_pack(in[k + 2 * f], in[k + 2 * f + 1]));
    k += 2LL * nfr;
    uint32_t flags = 0;
    for (int s = 0; s < v.ns; ++s) {
        const int len = in[k], v0 = in[k + 1], v1 = in[k + 2];
        const int vel = MSNAKE_VEL_CODE(v0, v1);
        if (in[k + 4]) flags |= 1u << s;
        if (in[k + 5]) flags |= 16u << s;
        uint32_t headc = 0;
        if (len > 0) headc = cell_pack(in[k + 6], in[k + 7]);
        for (int i = lane; i < len; i += 64) {
            const uint32_t c = cell_pack(in[k + 6 + 2LL * i], in[k + 6 + 2LL * i + 1]);
            if (i < 64) v.body0[((size_t)e * v.ns + s) * 64 + i] = (uint16_t)c;          // head in slot 0
            else v.ovf[((size_t)e * v.ns + s) * v.cap + (i - 64)] = (uint16_t)c;         // overflow from position 0
        }
        HV_SET(SN_A(s), (uint32_t)len << 16);
        HV_SET(SN_B(s), in[k + 3]);
        HV_SET(SN_C(s), headc | ((uint32_t)vel << 16));
        k += 6 + 2LL * len;
    }
    if (in[7] & 0x100) flags |= HDR_FLAG_FINISHED;  // restored as exported: the episode is not counted a second time
    HV_SET_C(HDR_FLAGS, flags);
    h[lane] = hv;
}

__global__ __launch_bounds__(256) void msnake_state_unpack_kernel(StateView v, int env0, int count,
                                                                  const uint64_t* __restrict__ offsets,
                                                                  const int32_t* __restrict__ words, uint32_t* __restrict__ status) {
    const int lane = (int)(threadIdx.x & 63u);
    const int w = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (w >= count) return;
    state_unpack_env(v, env0 + w, lane, words + offsets[w], (long long)(offsets[w + 1] - offsets[w]), StatusGlobal{status, w});
}

// msnake_import_states: row e of words[nenv][stride] into env e where mask[e] != 0 (mask NULL: every env); count NULL:
// every row has `stride` words.  A count outside [0, stride] reads as -1 words: "too short", before any word is read
__global__ __launch_bounds__(256) void msnake_state_import_kernel(StateView v, const uint8_t* __restrict__ mask,
                                                                  const int32_t* __restrict__ words, int32_t stride,
                                                                  const int32_t* __restrict__ count, uint8_t* __restrict__ status,
                                                                  int refuse_offgrid_head) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= v.nenv) return;
    if (mask && !mask[e]) {
        if (lane == 0) status[e] = (uint8_t)MSNAKE_STATE_SKIPPED;
        return;
    }
    long long n = stride;
    if (count) {
        const int32_t c = (int32_t)uni((uint32_t)count[e]);
        n = c < 0 || c > stride ? -1 : c;
    }
    state_unpack_env(v, e, lane, words + (size_t)e * (size_t)stride, n, StatusPerEnv{status, e, refuse_offgrid_head != 0});
}

hipError_t launch_state_sizes(const StepParams& p, int rules, int env0, int count, uint32_t* need_words, hipStream_t stream) {
    hipLaunchKernelGGL(msnake_state_sizes_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream,
                       state_view(p, rules), env0, count, need_words);
    return hipGetLastError();
}

hipError_t launch_state_pack(const StepParams& p, int rules, int env0, int count, const uint64_t* offsets, int32_t* words,
                             hipStream_t stream) {
    hipLaunchKernelGGL(msnake_state_pack_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream,
                       state_view(p, rules), env0, count, offsets, words);
    return hipGetLastError();
}

hipError_t launch_state_unpack(const StepParams& p, int rules, int env0, int count, const uint64_t* offsets,
                               const int32_t* words, uint32_t* status, hipStream_t stream) {
    hipLaunchKernelGGL(msnake_state_unpack_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, stream,
                       state_view(p, rules), env0, count, offsets, words, status);
    return hipGetLastError();
}

hipError_t launch_state_export(const StepParams& p, int rules, int32_t* words, int32_t stride, int32_t* count, hipStream_t stream) {
    hipLaunchKernelGGL(msnake_state_export_kernel, dim3((unsigned)((p.nenv + 3) / 4)), dim3(256), 0, stream,
                       state_view(p, rules), words, stride, count);
    return hipGetLastError();
}

hipError_t launch_state_import(const StepParams& p, int rules, const uint8_t* mask, const int32_t* words, int32_t stride,
                               const int32_t* count, uint8_t* status, bool refuse_offgrid_head, hipStream_t stream) {
    hipLaunchKernelGGL(msnake_state_import_kernel, dim3((unsigned)((p.nenv + 3) / 4)), dim3(256), 0, stream,
                       state_view(p, rules), mask, words, stride, count, status, refuse_offgrid_head ? 1 : 0);
    return hipGetLastError();
}

}  // namespace msnake
