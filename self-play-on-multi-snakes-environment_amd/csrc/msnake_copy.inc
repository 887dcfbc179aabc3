// msnake_copy.inc -- env state copied between two handles on the device (msnake_copy_envs: snapshot, fork, restore).
// Included at the end of msnake_kernels.hip: it uses that file's wave helpers and must stay in its translation unit.
// Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per DESTINATION env.  Its source index is wave-uniform; a negative one ends the wave before any load.
// Everything a step reads sits at addresses that depend only on the env index, so the copy is a handful of coalesced
// wave instructions, and its traffic follows the state that exists, not the capacity of the rings:
//   * the 256-byte record, lane l <-> word l: one load from the source, one store to the destination.  Merged by lane:
//     the destination keeps its logging totals (HDR_ACC_*), the overflow ring's head position is normalised to 0 (see
//     below), and for snake_env / adversarial the upper half -- the Philox draws parked there belong to the SOURCE
//     slot's stream -- is written as zeros, which is also what a short-record handle expects to find there;
//   * every snake's 128-byte body ring, lane l <-> slot l, as it is (the record carries hp0, the head's slot);
//   * bodies over 64 cells only: pieces 64.. of the overflow ring, len - 64 cells in whole waves, read at the source's
//     rotation (ohp, capacity of the source) and written from position 0 -- the capacities differ when the two
//     handles' max_steps do (new_world);
//   * adversarial only: chunk 0 of the fruit list (128 bytes) and the HDR_NLIST entries of the complete list.
// An env whose source index is >= the source's env count, or whose bodies do not fit the destination's overflow ring,
// is left as it is and its HDR_ACC_ERRORS grows by one.  No LDS, no barrier, no atomics, no random numbers.
namespace msnake {

struct CopyArgs {
    const uint32_t* s_hdr; const uint16_t* s_body0; const uint16_t* s_ovf; const uint16_t* s_fl0; const uint16_t* s_flist;
    uint32_t* d_hdr; uint16_t* d_body0; uint16_t* d_ovf; uint16_t* d_fl0; uint16_t* d_flist;
    const int32_t* index;  // [d_nenv] source env of every destination env; NULL = the identity
    int32_t s_nenv, d_nenv, ns, s_cap, d_cap, fcap, rules;
};

__global__ __launch_bounds__(256) void msnake_copy_envs_kernel(CopyArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.d_nenv) return;
    const int src = a.index ? (int)uni((uint32_t)a.index[e]) : e;
    if (src < 0) return;  // not selected: no load, no store
    uint32_t* dh = a.d_hdr + (size_t)e * MSNAKE_HDR_WORDS;
    const bool acc = lane >= HDR_ACC_EPISODES && lane <= HDR_ACC_LEN_HI;
    if (src >= a.s_nenv) {  // nothing of the source is read
        if (lane == HDR_ACC_ERRORS) dh[lane] += 1u;
        return;
    }
    const int ns = a.ns;
    const uint32_t sv = a.s_hdr[(size_t)src * MSNAKE_HDR_WORDS + lane];
    const uint32_t dv = acc ? dh[lane] : 0u;
    uint32_t ring[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        ring[s] = s < ns ? (uint32_t)a.s_body0[((size_t)src * ns + s) * 64 + lane] : 0u;
    const bool adv = a.rules == MSNAKE_RULES_ADVERSARIAL;
    uint32_t fr = 0u;
    if (adv) fr = a.s_fl0[(size_t)src * 64 + lane];

    int len[MSNAKE_MAX_SNAKES];
    bool fits = true;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        len[s] = s < ns ? (int)(rdlane(sv, SN_A(s)) >> 16) : 0;
        fits = fits && len[s] <= a.d_cap - 1;  // the step kernel's own bound on a body
    }
    if (!fits) {
        if (lane == HDR_ACC_ERRORS) dh[lane] = dv + 1u;
        return;
    }

    uint32_t hv = acc ? dv : sv;
    if (lane < ns) hv &= 0xFFFF0000u;  // SN_A: len stays, the overflow ring is written from position 0
    if (a.rules != MSNAKE_RULES_NEW_WORLD && lane >= MSNAKE_HDR_SHORT_WORDS) hv = 0u;  // no parked draws (new_world: fruits)
    dh[lane] = hv;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        if (s < ns) a.d_body0[((size_t)e * ns + s) * 64 + lane] = (uint16_t)ring[s];

#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= ns || len[s] <= 64) continue;
        const int ohp = (int)(rdlane(sv, SN_A(s)) & 0xFFFFu);
        const int n = len[s] - 64 < a.s_cap ? len[s] - 64 : a.s_cap;  // (<= d_cap - 65: checked above)
        const uint16_t* so = a.s_ovf + ((size_t)src * ns + s) * a.s_cap;
        uint16_t* dk = a.d_ovf + ((size_t)e * ns + s) * a.d_cap;
        for (int base = 0; base < n; base += 64) {
            const int j = base + lane;
            int idx = ohp + j;
            idx = idx >= a.s_cap ? idx - a.s_cap : idx;
            idx = idx >= a.s_cap ? a.s_cap - 1 : idx;  // (a well-formed record never gets here)
            if (j < n) dk[j] = so[idx];
        }
    }
    if (adv) {
        a.d_fl0[(size_t)e * 64 + lane] = (uint16_t)fr;
        int nl = (int)rdlane(sv, HDR_NLIST);
        nl = nl > a.fcap ? a.fcap : nl;
        const uint16_t* sl = a.s_flist + (size_t)src * a.fcap;
        uint16_t* dl = a.d_flist + (size_t)e * a.fcap;
        for (int base = 0; base < nl; base += 64) {
            const int f = base + lane;
            if (f < nl) dl[f] = sl[f];
        }
    }
}

hipError_t launch_copy_envs(const StepParams& dst, const StepParams& src, int rules, const int32_t* src_index, hipStream_t stream) {
    const CopyArgs a{src.hdr, src.body0, src.ring, src.fl0, src.flist, dst.hdr, dst.body0, dst.ring, dst.fl0, dst.flist, src_index,
                     src.nenv, dst.nenv, dst.n_snakes, src.rest.cap, dst.rest.cap, dst.fcap, rules};
    hipLaunchKernelGGL(msnake_copy_envs_kernel, dim3((unsigned)((dst.nenv + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
