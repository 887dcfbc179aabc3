// msnake_copy.inc -- env state copied between two handles on the device (msnake_copy_envs: snapshot, fork, restore).
// Included behind msnake_state.inc by msnake_views.hip: it uses msnake_device.h's wave helpers.
// Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per DESTINATION env.  Its source index is wave-uniform; a negative one ends the wave before any load.
// The source env is read through EnvReader (msnake_envread.inc).
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
    StateView src, dst;    // same rules, dim and snake count, hence fcap (msnake_copy_envs checks); only `dst` is written
    const int32_t* index;  // [dst.nenv] source env of every destination env; NULL = the identity
};

__global__ __launch_bounds__(256) void msnake_copy_envs_kernel(CopyArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.dst.nenv) return;
    const int src = a.index ? (int)uni((uint32_t)a.index[e]) : e;
    if (src < 0) return;  // not selected: no load, no store
    const StateView& d = a.dst;
    uint32_t* dh = d.hdr + (size_t)e * MSNAKE_HDR_WORDS;
    const bool acc = lane >= HDR_ACC_EPISODES && lane <= HDR_ACC_LEN_HI;
    if (src >= a.src.nenv) {  // nothing of the source is read
        if (lane == HDR_ACC_ERRORS) dh[lane] += 1u;
        return;
    }
    const int ns = d.ns;
    const EnvReader rd(a.src, src, lane);
    const uint32_t dv = acc ? dh[lane] : 0u;
    const bool adv = d.rules == MSNAKE_RULES_ADVERSARIAL;
    uint32_t fr = 0u;
    if (adv) fr = a.src.fl0[(size_t)src * 64 + lane];

    SnakeRef sn[MSNAKE_MAX_SNAKES];
    bool fits = true;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        sn[s] = rd.snake(s);
        fits = fits && sn[s].len <= d.cap - 1;  // the step kernel's own bound on a body
    }
    if (!fits) {
        if (lane == HDR_ACC_ERRORS) dh[lane] = dv + 1u;
        return;
    }

    uint32_t hv = acc ? dv : rd.hv;
    if (lane < ns) hv &= 0xFFFF0000u;  // SN_A: len stays, the overflow ring is written from position 0
    if (d.rules != MSNAKE_RULES_NEW_WORLD && lane >= MSNAKE_HDR_SHORT_WORDS) hv = 0u;  // no parked draws (new_world: fruits)
    dh[lane] = hv;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        if (s < ns) d.body0[((size_t)e * ns + s) * 64 + lane] = (uint16_t)rd.ring[s];

#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {  // (at most d.cap - 65 overflow pieces: checked above)
        uint16_t* dk = d.ovf + ((size_t)e * ns + s) * d.cap;
        rd.for_each_piece(sn[s], [&](int i, uint32_t c, bool valid) {
            if (valid && i >= 64) dk[i - 64] = (uint16_t)c;
        });
    }
    if (adv) {
        d.fl0[(size_t)e * 64 + lane] = (uint16_t)fr;
        uint16_t* dl = d.flist + (size_t)e * d.fcap;
        rd.for_each_fruit([&](int f, uint32_t c, bool valid) {
            if (valid) dl[f] = (uint16_t)c;
        });
    }
}

hipError_t launch_copy_envs(const StepParams& dst, const StepParams& src, int rules, const int32_t* src_index, hipStream_t stream) {
    const CopyArgs a{state_view(src, rules), state_view(dst, rules), src_index};
    hipLaunchKernelGGL(msnake_copy_envs_kernel, dim3((unsigned)((dst.nenv + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
