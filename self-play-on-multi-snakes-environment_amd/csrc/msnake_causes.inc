// msnake_causes.inc -- why each snake died in a step and on whose body, from the states before and after it
// (msnake_death_causes).  Included behind msnake_copy.inc by msnake_views.hip; it uses msnake_device.h's wave helpers
// and EnvReader.  Off the step path: nothing here is referenced by msnake_step_kernel, and both handles are only READ.
//
// snake_env and adversarial move every snake, judge every snake against the same post-move bodies and only then clear
// the dead ones; a cleared snake keeps its velocity and grow_to words.  So B'_k, the body snake k was judged with, is
//   * k's body in the after state, if k survived;
//   * otherwise, with v = k's velocity after: k's body before if v = (0, 0), else [head before + v] followed by pieces
//     0 .. len before - 1 - popped of the body before, popped = (len before >= grow_to after).
// One wavefront per env, two EnvReaders (before, after): both records and all rings are requested before either is
// used.  The query cells are the heads H_s = piece 0 of B'_s, at most four and wave-uniform, so no bitboard is built:
// every participant's non-head pieces are walked over the lanes with for_each_piece (a survivor: the after view from
// piece 1 on; a snake that died: the before view up to len - 1 - popped), each lane compares its piece with the four
// H_s, and a ballot turns the lane predicate into one wave-uniform bit per (s, k).  Bodies over 64 pieces come out of
// the overflow ring through the reader, under its bounds.  No LDS, no barrier, no atomics, no random numbers.
namespace msnake {

struct CausesArgs {
    StateView before, after;  // same dim, snake count, rules and env count (msnake_death_causes checks); both only read
    uint8_t* cause; uint8_t* by; uint8_t* victims; int8_t* where;  // [nenv][ns] and [nenv][ns][2]; any may be NULL
};

// a head as a cell code, or a value no piece of a ring can hold (pieces are 16 bits) where the code cannot express it
__device__ __forceinline__ uint32_t head_key(bool on, int x, int y) {
    return (on && x >= -1 && y >= -1) ? cell_pack(x, y) : ~0u;
}

// bit s: H_s (key hk[s]) equals one of the pieces lo .. hi - 1 of snake `sn` in view `rd`
__device__ __forceinline__ uint32_t heads_on_pieces(const EnvReader& rd, const SnakeRef& sn, int lo, int hi,
                                                    const uint32_t (&hk)[MSNAKE_MAX_SNAKES]) {
    uint32_t m = 0u;
    rd.for_each_piece(sn, [&](int i, uint32_t c, bool valid) {
        const bool in = valid && i >= lo && i < hi;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            if (__builtin_amdgcn_ballot_w64(in && c == hk[s]) != 0) m |= 1u << s;
    });
    return m;
}

// lane s < 4 <- v[s]
__device__ __forceinline__ uint32_t by_lane(int lane, const uint32_t (&v)[MSNAKE_MAX_SNAKES]) {
    return lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : v[3];
}

__global__ __launch_bounds__(256) void msnake_death_causes_kernel(CausesArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.after.nenv) return;
    const int ns = a.after.ns, dim = a.after.dim;
    const EnvReader rb(a.before, e, lane);
    const EnvReader ra(a.after, e, lane);

    // ---- the heads H_s and, per participant, which view holds its non-head pieces and which of them count
    SnakeRef sb[MSNAKE_MAX_SNAKES], sa[MSNAKE_MAX_SNAKES];
    bool part[MSNAKE_MAX_SNAKES], lives[MSNAKE_MAX_SNAKES];
    int hx[MSNAKE_MAX_SNAKES], hy[MSNAKE_MAX_SNAKES], lo[MSNAKE_MAX_SNAKES], hi[MSNAKE_MAX_SNAKES];
    uint32_t hk[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) {
        sb[k] = rb.snake(k);
        sa[k] = ra.snake(k);
        part[k] = sb[k].len > 0;
        lives[k] = sa[k].len > 0;
        const int vel = k < ns ? (int)((ra.word(SN_C(k)) >> 16) & 7u) : 0;
        const int grow = k < ns ? (int)ra.word(SN_B(k)) : 0;
        const int popped = sb[k].len >= grow ? 1 : 0;
        if (lives[k]) {
            hx[k] = sa[k].x; hy[k] = sa[k].y; lo[k] = 1; hi[k] = sa[k].len;
        } else if (vel == 0) {
            hx[k] = sb[k].x; hy[k] = sb[k].y; lo[k] = 1; hi[k] = sb[k].len;
        } else {
            hx[k] = sb[k].x + vel_v0(vel); hy[k] = sb[k].y + vel_v1(vel); lo[k] = 0; hi[k] = sb[k].len - popped;
        }
        hk[k] = head_key(part[k], hx[k], hy[k]);
    }

    // ---- on[k] bit s: H_s lies on a non-head piece of B'_k
    uint32_t on[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) {
        on[k] = 0u;
        if (!part[k]) continue;
        on[k] = lives[k] ? heads_on_pieces(ra, sa[k], lo[k], hi[k], hk) : heads_on_pieces(rb, sb[k], lo[k], hi[k], hk);
    }

    // ---- the four outputs, wave-uniform per snake, then one byte per lane
    uint32_t cause[MSNAKE_MAX_SNAKES], by[MSNAKE_MAX_SNAKES], victims[MSNAKE_MAX_SNAKES] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        uint32_t body = 0u, head = 0u, self = 0u;
#pragma unroll
        for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) {
            const uint32_t hit = (on[k] >> s) & 1u;
            if (k == s) self = hit;
            else {
                body |= hit << k;
                if (part[s] && part[k] && hx[k] == hx[s] && hy[k] == hy[s]) head |= 1u << k;
            }
        }
        const bool wall = hx[s] < 0 || hx[s] >= dim || hy[s] < 0 || hy[s] >= dim;
        cause[s] = !part[s] ? 0u : (wall ? MSNAKE_CAUSE_WALL : 0u) | (self ? MSNAKE_CAUSE_SELF : 0u) |
                                       (head ? MSNAKE_CAUSE_HEAD_ON : 0u) | (body ? MSNAKE_CAUSE_BODY : 0u);
        by[s] = body | (head << 4);
    }
#pragma unroll
    for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k)
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            victims[k] |= (((by[s] >> k) & 1u) << s) | (((by[s] >> (4 + k)) & 1u) << (4 + s));

    const size_t row = (size_t)e * (size_t)ns;
    if (lane < ns) {
        if (a.cause) a.cause[row + lane] = (uint8_t)by_lane(lane, cause);
        if (a.by) a.by[row + lane] = (uint8_t)by_lane(lane, by);
        if (a.victims) a.victims[row + lane] = (uint8_t)by_lane(lane, victims);
    }
    if (a.where && lane < 2 * ns) {  // lane 2 s: c0 of H_s, lane 2 s + 1: c1
        uint32_t xy[MSNAKE_MAX_SNAKES];
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) xy[s] = (uint32_t)(cause[s] == 0u ? -2 : (lane & 1) ? hy[s] : hx[s]);
        a.where[2 * row + lane] = (int8_t)(int32_t)by_lane(lane >> 1, xy);
    }
}

hipError_t launch_death_causes(const StepParams& after, const StepParams& before, int rules, uint8_t* cause, uint8_t* by,
                               uint8_t* victims, int8_t* where, hipStream_t stream) {
    const CausesArgs a{state_view(before, rules), state_view(after, rules), cause, by, victims, where};
    hipLaunchKernelGGL(msnake_death_causes_kernel, dim3((unsigned)((after.nenv + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
