// msnake_space.inc -- reachable-space counts and the flood-fill opponent space_greedy (msnake_space_actions).
// Included behind msnake_scripted.inc by msnake_opponents.hip: it uses msnake_device.h's wave helpers, wave_scan_incl and
// launch_by_flags and msnake_scripted.inc's wave_reduce.  Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader (msnake_envread.inc).
//   * Occupancy: lane y owns row y of the board as ONE 64-bit mask, bit x <-> cell (x, y) = (c0, c1).  The body
//     cells arrive lane-distributed (lane <-> ring slot), so they are scattered through a wave-private 512-byte
//     slice of static LDS: one ds_or per cell, then every lane reads its own row once.  DS operations of one wave
//     execute in program order, so wave_sync() (a compiler fence) is all the ordering this needs: no workgroup
//     barrier -- the waves of the batch tail have returned by then.  `vacant` = ~used inside the grid; rows >= dim
//     and bits >= dim are 0, i.e. blocked.
//   * The 16 candidates (4 snakes x 4 moves) live in lanes 0..15, lane 4 s + m <-> move m + 1 of snake s: target
//     coordinates, open bit, and in the end the count.  Whether a target is free is one ds_bpermute gather of the
//     target row's mask.
//   * A fill is one seed bit, then sweeps r |= ((r << 1) | (r >> 1) | row_above | row_below) & vacant; the
//     neighbour rows come by DPP wave_shr:1 / wave_shl:1 with bound_ctrl (lane 0 / lane 63 receive 0; rows >= dim
//     hold 0 anyway).  No LDS traffic in the loop.  Four sweeps per convergence test (one ballot); growth is
//     monotone and a region has at most dim^2 cells, so the loop is cut after dim^2 sweeps whatever the record says.
//   * Count = popcount per lane + one DPP sum over the wave.  After a fill, every still-pending candidate whose
//     target bit lies in the finished region takes the same count (one more gather): a board with one big free
//     region costs ONE fill per env, however many snakes and moves.  The result does not depend on that reuse: the
//     regions of two targets are either equal or disjoint.
//   * space_greedy: need = min(len, max over the open moves of space) by two quad-permute DPP steps, eligible =
//     open && space >= need, then safe_greedy's choice among the eligible moves (min over (fruit, move) pairs of
//     distance << 3 | move, fruits lane-distributed).
//   * lane s stores snake s's action word and mask byte, lane 4 s + m the count of move m + 1.
// The occupancy build with the candidates (read_board), the fills (region_sizes) and the choice by count (greedy_by_count
// = eligible_moves, then greedy_among) are functions of their own: msnake_territory.inc, included behind this file, races
// on the same board and chooses in the same way, and msnake_path.inc takes the eligible moves from here and chooses among
// them by its own distance.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct SpaceArgs {
    StateView v;
    int32_t* actions; uint8_t* safe; uint16_t* space;
    int32_t stride;
    uint32_t mask;
};

constexpr int SPACE_WAVES = 4;  // waves (envs) per workgroup

// row y - 1 / row y + 1 of a row-per-lane mask; the lane without a neighbour receives 0
__device__ __forceinline__ uint64_t row_above(uint64_t r) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)r, 0x138, 0xF, 0xF, true);          // wave_shr:1
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(r >> 32), 0x138, 0xF, 0xF, true);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t row_below(uint64_t r) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)r, 0x130, 0xF, 0xF, true);          // wave_shl:1
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(r >> 32), 0x130, 0xF, 0xF, true);
    return ((uint64_t)hi << 32) | lo;
}

// sum over the wave: lane 63 of the inclusive prefix sum (msnake_device.h)
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) { return rdlane(wave_scan_incl(x), 63); }

// lane l receives v of lane src(l) & 63
__device__ __forceinline__ uint64_t gather_row(uint64_t v, int src) {
    const int addr = (src & 63) << 2;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(addr, (int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// What both count kernels (this file's and msnake_territory.inc's) know of the board before they fill anything: the
// free cells as row-per-lane masks and the 16 candidates.
struct Board {
    uint64_t vacant;   // lane y: bit x <-> cell (x, y) is free; 0 for lanes >= dim
    int len[MSNAKE_MAX_SNAKES], hx[MSNAKE_MAX_SNAKES], hy[MSNAKE_MAX_SNAKES];
    int my_len;        // lane 4 s + m: snake s's body length (0 for lanes >= 16)
    int gx, gy;        // lane 4 s + m: the target of move m + 1 where it lies in the grid, else (0, 0): safe to gather with
    uint32_t open_all; // bit 4 s + m: move m + 1 of snake s is open
};

// `my`: the wave's private 128 words of LDS (row y = words 2 y and 2 y + 1).  Every lane of the wave must call this.
__device__ __forceinline__ Board read_board(const StateView& v, const EnvReader& rd, uint32_t* my, int lane) {
    Board b;
    const int ns = v.ns, dim = v.dim;
    my[lane] = 0u;
    my[64 + lane] = 0u;
    wave_sync();

    // ---- occupancy: every body cell inside the grid sets its bit
    auto mark = [&](uint32_t c, bool valid) {
        const int x = MSNAKE_CELL_C0(c), y = MSNAKE_CELL_C1(c);
        if (valid && x >= 0 && x < dim && y >= 0 && y < dim)
            __hip_atomic_fetch_or(&my[2 * y + (x >> 5)], 1u << (x & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        const SnakeRef sn = rd.snake(s);
        b.len[s] = sn.len; b.hx[s] = sn.x; b.hy[s] = sn.y;
        rd.for_each_piece(sn, [&](int, uint32_t c, bool valid) { mark(c, valid); });
    }
    wave_sync();
    const uint64_t used = (uint64_t)my[2 * lane] | ((uint64_t)my[2 * lane + 1] << 32);
    b.vacant = lane < dim ? ~used & ((1ull << dim) - 1ull) : 0ull;

    // ---- the candidates: lane 4 s + m <-> move m + 1 of snake s
    const int cs = lane >> 2, cm = lane & 3;
    b.my_len = cs == 0 ? b.len[0] : cs == 1 ? b.len[1] : cs == 2 ? b.len[2] : cs == 3 ? b.len[3] : 0;
    const int my_hx = cs == 0 ? b.hx[0] : cs == 1 ? b.hx[1] : cs == 2 ? b.hx[2] : b.hx[3];
    const int my_hy = cs == 0 ? b.hy[0] : cs == 1 ? b.hy[1] : cs == 2 ? b.hy[2] : b.hy[3];
    const int tx = my_hx + move_d0(cm), ty = my_hy + move_d1(cm);
    const bool onb = lane < 4 * ns && b.my_len > 0 && tx >= 0 && tx < dim && ty >= 0 && ty < dim;
    b.gx = onb ? tx : 0, b.gy = onb ? ty : 0;  // what the gathers index with: always inside the wave
    const uint64_t target_row = gather_row(b.vacant, b.gy);  // (every lane takes part: the source lanes must be active)
    const bool is_open = onb && ((target_row >> b.gx) & 1ull);
    b.open_all = (uint32_t)__ballot(is_open);
    return b;
}

// The space of every candidate: one fill per distinct region that holds an open target.  Lane 4 s + m receives the
// number of free cells connected to the target of move m + 1 of snake s, 0 where the move is not open.  Every lane of
// the wave must call this.
__device__ __forceinline__ uint32_t region_sizes(const Board& b, int dim, int lane) {
    const uint64_t vacant = b.vacant;
    const int gx = b.gx, gy = b.gy;
    uint32_t space = 0u;
    uint32_t pending = b.open_all;
    const int max_sweeps = dim * dim;
    for (int guard = 0; pending != 0u && guard < 16; ++guard) {
        const int k = __builtin_ctz(pending);
        const int sx = (int)rdlane((uint32_t)gx, k), sy = (int)rdlane((uint32_t)gy, k);
        uint64_t r = lane == sy ? 1ull << sx : 0ull;
        for (int sweeps = 0; sweeps < max_sweeps; sweeps += 4) {
            const uint64_t before = r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r |= ((r << 1) | (r >> 1) | row_above(r) | row_below(r)) & vacant;
            if (__ballot(r != before) == 0ull) break;
        }
        const uint32_t cells = wave_sum((uint32_t)__popcll(r));
        const uint64_t filled_row = gather_row(r, gy);
        const bool inside = lane < 16 && ((pending >> lane) & 1u) && ((filled_row >> gx) & 1ull);
        const uint32_t got = (uint32_t)__ballot(inside) | (1u << k);
        if (lane < 16 && ((got >> lane) & 1u)) space = cells;
        pending &= ~got;
    }
    return space;
}

// The moves a count leaves to choose from.  `count`: lane 4 s + m holds the count of move m + 1 of snake s (0 where the
// move is not open).  need = min(len, max over the open moves of count) by two quad-permute DPP steps, eligible = open
// && count >= need; bit 4 s + m of the result.  Every lane of the wave must call this.
__device__ __forceinline__ uint32_t eligible_moves(int lane, uint32_t open_all, uint32_t count, int my_len) {
    uint32_t mx = count;
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
    mx = mx > o ? mx : o;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mx, 0x4E, 0xF, 0xF, true);           // quad_perm:[2,3,0,1]
    mx = mx > o ? mx : o;
    const uint32_t need = (uint32_t)my_len < mx ? (uint32_t)my_len : mx;
    return (uint32_t)__ballot(lane < 16 && ((open_all >> lane) & 1u) && count >= need);
}

// safe_greedy's choice among the moves in `elig_all` (bit 4 s + m): the first, in the order 1, 2, 3, 4, whose target has
// the strictly smallest L1 distance to any fruit.  act[s] is set for every snake with an eligible move and left alone
// otherwise.  Every lane of the wave must call this.
__device__ __forceinline__ void greedy_among(const EnvReader& rd, int ns, int lane, uint32_t elig_all,
                                             const int (&hx)[MSNAKE_MAX_SNAKES], const int (&hy)[MSNAKE_MAX_SNAKES],
                                             uint32_t (&act)[MSNAKE_MAX_SNAKES]) {
    uint32_t elig[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) elig[s] = (elig_all >> (4 * s)) & 15u;

    const int nfr = rd.n_fruits();
    uint32_t key[MSNAKE_MAX_SNAKES];  // min over this lane's fruits and the eligible moves of distance << 3 | move
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) key[s] = 0xFFFFFFFFu;
    rd.for_each_fruit([&](int, uint32_t c, bool valid) {
        const int fx = cell_c0(c), fy = cell_c1(c);
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int qx = hx[s] + move_d0(m), qy = hy[s] + move_d1(m);
                const int dx = fx - qx, dy = fy - qy;
                const uint32_t kk = ((uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) << 3) | (uint32_t)(m + 1);
                const uint32_t out = 0u - ((~elig[s] >> m) & 1u);  // all ones where the move is not eligible
                const uint32_t cand = valid ? kk | out : 0xFFFFFFFFu;
                key[s] = cand < key[s] ? cand : key[s];
            }
    });
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= ns || elig[s] == 0u) continue;
        if (nfr <= 0) {  // every distance is 0: the first eligible move
            act[s] = (uint32_t)__builtin_ctz(elig[s]) + 1u;
        } else {
            act[s] = wave_reduce(key[s], [](uint32_t x, uint32_t y) { return x < y ? x : y; }) & 7u;
        }
    }
}

// The choice space_greedy and territory_greedy share: safe_greedy's among the moves their count leaves eligible.
__device__ __forceinline__ void greedy_by_count(const EnvReader& rd, int ns, int lane, uint32_t open_all, uint32_t count, int my_len,
                                                const int (&hx)[MSNAKE_MAX_SNAKES], const int (&hy)[MSNAKE_MAX_SNAKES],
                                                uint32_t (&act)[MSNAKE_MAX_SNAKES]) {
    greedy_among(rd, ns, lane, eligible_moves(lane, open_all, count, my_len), hx, hy, act);
}

// ACT: the space_greedy actions are written (snake_mask != 0); SAFE / SPACE: safe_dev / space_dev are written
template <bool ACT, bool SAFE, bool SPACE>
__global__ __launch_bounds__(SPACE_WAVES * 64) void msnake_space_kernel(SpaceArgs a) {
    __shared__ uint32_t occ[SPACE_WAVES][128];  // per wave: row y = words 2 y (bits 0..31) and 2 y + 1 (bits 32..63)
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * SPACE_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int ns = a.v.ns, dim = a.v.dim;
    const EnvReader rd(a.v, e, lane);
    const Board b = read_board(a.v, rd, occ[wave], lane);
    const uint32_t open_all = b.open_all;

    // ---- fills: one per distinct region that holds an open target
    const uint32_t space = region_sizes(b, dim, lane);

    // ---- space_greedy: the eligible moves, then safe_greedy's choice among them
    uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) act[s] = 0u;
    if (ACT) greedy_by_count(rd, ns, lane, open_all, space, b.my_len, b.hx, b.hy, act);

    // lane s owns snake s's action word and mask byte, lane 4 s + m the count of move m + 1
    if (lane < ns) {
        const uint32_t my_act = lane == 0 ? act[0] : lane == 1 ? act[1] : lane == 2 ? act[2] : act[3];
        if (ACT && ((a.mask >> lane) & 1u)) a.actions[(size_t)e * a.stride + lane] = (int32_t)my_act;
        if (SAFE) a.safe[(size_t)e * ns + lane] = (uint8_t)(((open_all >> (4 * lane)) & 15u) << 1);
    }
    if (SPACE && lane < 4 * ns) a.space[(size_t)e * ns * 4 + lane] = (uint16_t)space;
}

hipError_t launch_space(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                        uint16_t* space, hipStream_t stream) {
    const SpaceArgs a{state_view(p, rules), actions, safe, space, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + SPACE_WAVES - 1) / SPACE_WAVES)), block(SPACE_WAVES * 64);
    return launch_by_flags<3>((snake_mask != 0u ? 4 : 0) | (safe ? 2 : 0) | (space ? 1 : 0), [&](auto act, auto sf, auto sp) {
        hipLaunchKernelGGL((msnake_space_kernel<act.value, sf.value, sp.value>), grid, block, 0, stream, a);
    });
}

}  // namespace msnake
