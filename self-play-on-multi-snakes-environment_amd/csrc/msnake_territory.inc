// msnake_territory.inc -- Voronoi territory counts and the opponent territory_greedy (msnake_territory_actions).
// Included behind msnake_space.inc by msnake_opponents.hip: it uses that file's Board / read_board, row_above,
// row_below, wave_sum and greedy_by_count.  Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader.  Occupancy and the 16 candidates
// (lane 4 s + m <-> move m + 1 of snake s) are read_board's, exactly as msnake_space_kernel has them.
//   * Per snake s with an open move, one race between five row-per-lane fronts: B, the BFS ball of the OTHER snakes'
//     open targets O_s, and A_m, what snake s reaches strictly first when it starts from the target of move m + 1.
//     B_0 = O_s, A_m,0 = {target} \ B_0.  One round: B |= N(B) & vacant first, then A_m |= N(A_m) & vacant & ~B with
//     the B that has already grown -- a tie goes to the others.  N is the space kernel's sweep: the row shifted both
//     ways, and the rows above and below by DPP.  No LDS traffic in the loop.
//   * B does not depend on any A_m, so the four moves of one snake share it.  Once no A_m gained a cell in a round none
//     ever does again (B only grows), so "no A_m changed" ends the race; B need not converge.  The test is one ballot
//     per four rounds.  A front gains at least one cell per round until it stops and has at most dim^2 cells, so the
//     loop is cut after dim^2 rounds, and there are at most MSNAKE_MAX_SNAKES races, whatever the record says.
//   * Count = popcount per lane + wave_sum, kept by lane 4 s + m.  A move that is not open starts from the empty set
//     and counts 0; so does an open move whose target lies in O_s.
//   * territory_greedy is space_greedy's choice (greedy_by_count) with this count: when every open move counts 0,
//     need = 0 and every open move is eligible.
//   * lane s stores snake s's action word and mask byte, lane 4 s + m the count of move m + 1.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct TerritoryArgs {
    StateView v;
    int32_t* actions; uint8_t* safe; uint16_t* territory;
    int32_t stride;
    uint32_t mask;
};

// the 4-neighbourhood of a row-per-lane set (cells outside the grid are cut by the caller's `& vacant`)
__device__ __forceinline__ uint64_t neighbours(uint64_t r) { return (r << 1) | (r >> 1) | row_above(r) | row_below(r); }

// ACT: the territory_greedy actions are written (snake_mask != 0); SAFE / TERR: safe_dev / territory_dev are written
template <bool ACT, bool SAFE, bool TERR>
__global__ __launch_bounds__(SPACE_WAVES * 64) void msnake_territory_kernel(TerritoryArgs a) {
    __shared__ uint32_t occ[SPACE_WAVES][128];  // per wave: row y = words 2 y (bits 0..31) and 2 y + 1 (bits 32..63)
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * SPACE_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int ns = a.v.ns, dim = a.v.dim;
    const EnvReader rd(a.v, e, lane);
    const Board b = read_board(a.v, rd, occ[wave], lane);
    const uint64_t vacant = b.vacant;
    const uint32_t open_all = b.open_all;

    // ---- one race per snake that has an open move
    uint32_t territory = 0u;
    if (ACT || TERR) {
        const int max_rounds = dim * dim;
#pragma nounroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            const uint32_t mine = (open_all >> (4 * s)) & 15u;
            if (mine == 0u) continue;
            uint64_t B = 0ull;  // O_s: where the others can stand after this step
            uint32_t others = open_all & ~(15u << (4 * s));
            for (int guard = 0; others != 0u && guard < 16; ++guard) {
                const int k = __builtin_ctz(others);
                others &= others - 1u;
                const int ox = (int)rdlane((uint32_t)b.gx, k), oy = (int)rdlane((uint32_t)b.gy, k);
                B |= lane == oy ? 1ull << ox : 0ull;
            }
            uint64_t A[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int sx = (int)rdlane((uint32_t)b.gx, 4 * s + m), sy = (int)rdlane((uint32_t)b.gy, 4 * s + m);
                A[m] = ((mine >> m) & 1u) && lane == sy ? (1ull << sx) & ~B : 0ull;
            }
            for (int rounds = 0; rounds < max_rounds; rounds += 4) {
                uint64_t gained = 0ull;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    B |= neighbours(B) & vacant;
                    const uint64_t mayA = vacant & ~B;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const uint64_t grown = A[m] | (neighbours(A[m]) & mayA);
                        gained |= grown ^ A[m];
                        A[m] = grown;
                    }
                }
                if (__ballot(gained != 0ull) == 0ull) break;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint32_t cells = wave_sum((uint32_t)__popcll(A[m]));
                if (lane == 4 * s + m) territory = cells;
            }
        }
    }

    // ---- territory_greedy: space_greedy's choice with the territory in place of the space
    uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) act[s] = 0u;
    if (ACT) greedy_by_count(rd, ns, lane, open_all, territory, b.my_len, b.hx, b.hy, act);

    // lane s owns snake s's action word and mask byte, lane 4 s + m the count of move m + 1
    if (lane < ns) {
        const uint32_t my_act = lane == 0 ? act[0] : lane == 1 ? act[1] : lane == 2 ? act[2] : act[3];
        if (ACT && ((a.mask >> lane) & 1u)) a.actions[(size_t)e * a.stride + lane] = (int32_t)my_act;
        if (SAFE) a.safe[(size_t)e * ns + lane] = (uint8_t)(((open_all >> (4 * lane)) & 15u) << 1);
    }
    if (TERR && lane < 4 * ns) a.territory[(size_t)e * ns * 4 + lane] = (uint16_t)territory;
}

hipError_t launch_territory(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride,
                            uint8_t* safe, uint16_t* territory, hipStream_t stream) {
    const TerritoryArgs a{state_view(p, rules), actions, safe, territory, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + SPACE_WAVES - 1) / SPACE_WAVES)), block(SPACE_WAVES * 64);
    return launch_by_flags<3>((snake_mask != 0u ? 4 : 0) | (safe ? 2 : 0) | (territory ? 1 : 0), [&](auto act, auto sf, auto terr) {
        hipLaunchKernelGGL((msnake_territory_kernel<act.value, sf.value, terr.value>), grid, block, 0, stream, a);
    });
}

}  // namespace msnake
