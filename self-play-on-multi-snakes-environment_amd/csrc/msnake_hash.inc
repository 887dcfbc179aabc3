// msnake_hash.inc -- a 64-bit hash of every env's canonical state words (msnake_hash_states), formed on the device without
// forming the words.  Included behind msnake_state.inc by msnake_views.hip: it uses msnake_device.h's wave helpers.
// Off the step path: nothing here is referenced by msnake_step_kernel.
//
// With w[0..n) the words msnake_get_state returns for the env,
//     H = sum over the selected i of mix64(((uint64)(i + 1) << 32) | (uint32)w[i])   mod 2^64,
// mix64 being the splitmix64 finaliser.  A sum of per-index terms depends on which word sits where, yet may be formed in
// any order: one wavefront per env reads the state through EnvReader exactly as the pack kernel does, every lane adds
// the terms of its share of the words (the eight leading words, each snake's six and the first 16 inline fruits, one
// word per lane in one pass; ring pieces 32 to a pass, c0 on the lower and c1 on the upper half of the wave; list
// entries and overflow pieces two words per lane), and one wave reduction and one 8-byte store by lane 0 end it.  The word index
// of a snake's first word is a wave-uniform running offset, as in the pack kernel.  Bodies past 64 pieces come out of
// the overflow ring and adversarial lists past 64 entries out of `flist` (EnvReader's passes).
// MSNAKE_HASH_BOARD leaves out t, the draw counter, ep_len and ep_return (words 0, 1, 2, 4, 5) and the finished bit of
// word 7: what is left decides the frame and every future of the env but its random draws.
// No LDS, no barrier, no atomics, no random numbers; only `hash` is written.
namespace msnake {

__device__ __forceinline__ uint64_t hash_mix64(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the term of word `i` holding `w`
__device__ __forceinline__ uint64_t hash_term(size_t i, int32_t w) { return hash_mix64(((uint64_t)(i + 1) << 32) | (uint32_t)w); }
// the two terms of a cell whose first word is word `i`
__device__ __forceinline__ uint64_t hash_cell(size_t i, uint32_t c) { return hash_term(i, cell_c0(c)) + hash_term(i + 1, cell_c1(c)); }

// sum over the 64 lanes mod 2^64, in every lane: six butterfly steps (__shfl_xor moves the two halves through the
// cross-lane path, ds_bpermute: no LDS is allocated or touched)
__device__ __forceinline__ uint64_t hash_wave_sum(uint64_t x) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, d, 64);
    return x;
}

template <bool BOARD>
__global__ __launch_bounds__(256) void msnake_state_hash_kernel(StateView v, uint64_t* __restrict__ hash) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= v.nenv) return;
    const EnvReader rd(v, e, lane);
    const bool nw = v.rules == MSNAKE_RULES_NEW_WORLD;
    const int nfr = rd.n_fruits();
    const uint32_t flags = rd.flags();
    // The scalar words -- the eight leading ones and six per snake, 32 at most -- one per lane: lane l < 8 takes word l,
    // lane 8 + 6 s + j word j of snake s.  A term costs two 64-bit multiplies, which run at a quarter of the rate: summed
    // by lane 0 alone these words were 26 of the 34 terms a wave worked through one after the other.
    uint32_t sw = 0;   // this lane's scalar word,
    size_t si = 0;     // its index,
    bool sv = false;   // and whether the lane has one
    auto put = [&](int ln, size_t idx, int32_t w) {
        if (lane == ln) { sw = (uint32_t)w; si = idx; sv = true; }
    };
    if (!BOARD) {
        put(0, 0, (int32_t)rd.word(HDR_T)); put(1, 1, (int32_t)rd.word(HDR_CTR_LO)); put(2, 2, (int32_t)rd.word(HDR_CTR_HI));
        put(4, 4, (int32_t)rd.word(HDR_EP_LEN)); put(5, 5, (int32_t)rd.word(HDR_EP_RETURN));
    }
    put(3, 3, (int32_t)rd.word(HDR_SPARE)); put(6, 6, nfr);
    put(7, 7, v.ns | ((!BOARD && (flags & HDR_FLAG_FINISHED)) ? 0x100 : 0));
    // A cell is two words, and a pass over cells keeps a lane busy for two term-times while most lanes have no cell.  So
    // where the cells sit in registers -- the inline fruits (record words) and pieces 0..63 (the ring) -- a pass covers 32
    // cells, lanes 0..31 taking their c0 and lanes 32..63 their c1, each after one cross-lane read of the cell.
    const int half = lane & 31, comp = lane >> 5;
    const bool adv = v.rules == MSNAKE_RULES_ADVERSARIAL;
    uint64_t acc = 0;
    size_t k = 8;
    if (!adv) {  // inline fruits 0..15 ride in lanes 32..63 of the scalar pass: lane 32 + 2 f + c holds word c of fruit f
        const int f = (lane >> 1) & 15;
        const uint32_t c = (uint32_t)__shfl((int)rd.hv, (nw ? HDR_FRUIT0_N : HDR_FRUIT0_S) + f, 64) & 0xFFFFu;
        if (lane >= 32 && f < nfr) { sw = (uint32_t)((lane & 1) ? cell_c1(c) : cell_c0(c)); si = k + 2 * (size_t)f + (lane & 1); sv = true; }
    }
    if (adv || nfr > 16)  // the adversarial list, and inline fruits 16..31: through the reader's passes
        rd.for_each_fruit([&](int f, uint32_t c, bool valid) {
            if (valid && (adv || f >= 16)) acc += hash_cell(k + 2 * (size_t)f, c);
        });
    k += 2 * (size_t)nfr;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= v.ns) continue;
        const SnakeRef sn = rd.snake(s);
        const int len = sn.len, vel = (int)((rd.word(SN_C(s)) >> 16) & 7u);
        put(8 + 6 * s, k, len); put(9 + 6 * s, k + 1, vel_v0(vel)); put(10 + 6 * s, k + 2, vel_v1(vel));
        put(11 + 6 * s, k + 3, (int32_t)rd.word(SN_B(s))); put(12 + 6 * s, k + 4, snake_alive(flags, s, nw));
        put(13 + 6 * s, k + 5, snake_in_dead(flags, s, nw));
        const int in_ring = len < 64 ? len : 64;  // piece i < 64 sits in ring slot (hp0 + i) & 63 (msnake_envread.inc)
        for (int base = 0; base < in_ring; base += 32) {
            const int i = base + half;
            const uint32_t c = (uint32_t)__shfl((int)rd.ring[s], (sn.hp0 + i) & 63, 64);
            if (i < in_ring) acc += hash_term(k + 6 + 2 * (size_t)i + comp, comp ? cell_c1(c) : cell_c0(c));
        }
        if (len > 64)  // the overflow ring, through the reader and under its bounds
            rd.for_each_piece(sn, [&](int i, uint32_t c, bool valid) {
                if (valid && i >= 64) acc += hash_cell(k + 6 + 2 * (size_t)i, c);
            });
        k += 6 + 2 * (size_t)len;
    }
    if (sv) acc += hash_term(si, (int32_t)sw);
    acc = hash_wave_sum(acc);
    if (lane == 0) hash[e] = acc;
}

hipError_t launch_state_hash(const StepParams& p, int rules, bool board, uint64_t* hash, hipStream_t stream) {
    const dim3 grid((unsigned)((p.nenv + 3) / 4)), block(256);
    if (board) hipLaunchKernelGGL(msnake_state_hash_kernel<true>, grid, block, 0, stream, state_view(p, rules), hash);
    else hipLaunchKernelGGL(msnake_state_hash_kernel<false>, grid, block, 0, stream, state_view(p, rules), hash);
    return hipGetLastError();
}

}  // namespace msnake
