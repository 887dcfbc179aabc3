// msnake_timed.inc -- cell lifetimes, the timed reach of every move and the opponent timed_greedy (msnake_timed_actions).
// Included behind msnake_heads.inc, last, by msnake_opponents.hip: it uses msnake_space.inc's Board / read_board,
// gather_row, wave_sum and greedy_by_count, msnake_territory.inc's neighbours and msnake_scripted.inc's wave_reduce.
// Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader.  Occupancy and the 16 candidates
// (lane 4 s + m <-> move m + 1 of snake s) are read_board's, exactly as msnake_space_kernel has them.
//   * The lifetime image: a wave-private LDS image of dim^2 dwords (dynamic LDS: SPACE_WAVES * dim^2 * 4 bytes per
//     workgroup, so a small board does not pay for the largest), zeroed; every piece inside the grid puts its lifetime
//     there with ONE ds_max_u32.  The maximum over stacked pieces therefore does not depend on the order of the lanes,
//     of the 64-piece passes of the overflow ring or of the snakes.  life_dev leaves from this image in coalesced dword
//     stores of two entries (life_dev is only 2-byte aligned: an odd first and last entry go alone).
//   * admit(t), the cells with Life < t: the lifetimes are kept BIT-SLICED in registers, plane k of a lane that holds row y = bit k
//     of Life((x, y)) at bit x, stored inverted.  A level is at most dim^2 + 3, so PLANES = bits of (dim^2 + 4) <= 12 planes
//     suffice and a larger lifetime is clamped to all ones (never admitted).  The compare against the wave-uniform t
//     ripples from the low plane up, lt' = majority(~plane, lt, bit k of t): two VALU operations per plane and half, no
//     LDS or HBM access and no divergence inside the fill.  A free cell has lifetime 0 and is admitted from t = 1 on;
//     rows >= dim and bits >= dim are cut by the grid mask.
//     Two shortcuts, both wave-uniform: only the planes up to the highest bit of the longest lifetime below the clamp
//     are compared, and from the level behind that lifetime on admit is a constant (everything but the clamped cells).
//   * One fill per open candidate (two targets of one region can reach different sets, so nothing is shared):
//     seen = front = {target}; per level fresh = N(front) & ~seen & admit(t), seen |= fresh, front = fresh.  Four levels
//     per convergence ballot (an empty front stays empty); dim^2 levels cut the loop whatever the record says.  The reach
//     is popcount(seen) summed over the fill's lanes, kept by lane 4 s + m.
//   * Side by side: a board uses dim of the 64 lanes, so 64 / (dim + 1) fills run at once (3 at 19x19, 1 from 32x32 on),
//     fill g in lanes g (dim + 1) .. g (dim + 1) + dim - 1 with the rows of the board replicated there.  The lane between
//     two boards and the lanes behind the last one hold an empty grid mask: nothing is admitted there, so the DPP row moves
//     carry nothing from one board to the next.  Every fill of a group starts at level 1, so they share t and admit(t); the
//     group runs until its last front is empty; the counts are summed per segment.
//   * timed_greedy is space_greedy's choice (greedy_by_count) with this count.
//   * lane s stores snake s's action word and mask byte, lane 4 s + m the reach of move m + 1.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct TimedArgs {
    StateView v;
    int32_t* actions; uint8_t* safe; uint16_t* reach; uint16_t* life;
    int32_t stride;
    uint32_t mask;
};

constexpr int TIMED_PLANES = 12;  // 62^2 + 4 < 2^12

// ACT: the timed_greedy actions are written (snake_mask != 0); SAFE / REACH / LIFE: safe_dev / reach_dev / life_dev are written
template <bool ACT, bool SAFE, bool REACH, bool LIFE>
__global__ __launch_bounds__(SPACE_WAVES * 64) void msnake_timed_kernel(TimedArgs a) {
    __shared__ uint32_t occ[SPACE_WAVES][128];  // per wave: row y = words 2 y (bits 0..31) and 2 y + 1 (bits 32..63)
    extern __shared__ uint32_t timed_life[];    // per wave: dim^2 lifetimes, entry c0 * dim + c1
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * SPACE_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int ns = a.v.ns, dim = a.v.dim, n2 = dim * dim;
    const EnvReader rd(a.v, e, lane);
    uint32_t* const img = timed_life + (size_t)wave * n2;
    if (ACT || REACH || LIFE)
        for (int i = lane; i < n2; i += 64) img[i] = 0u;
    const Board b = read_board(a.v, rd, occ[wave], lane);  // (its wave_sync calls order the stores above as well)
    const uint32_t open_all = b.open_all;

    uint32_t reach = 0u;  // lane 4 s + m: |V| of the fill from the target of move m + 1 of snake s
    if (ACT || REACH || LIFE) {
        // ---- the lifetime image: the maximum over every piece that lies on a cell
        const bool never = a.v.rules == MSNAKE_RULES_NEW_WORLD && a.v.nf == 0;  // that rule set never pops
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            const SnakeRef sn = rd.snake(s);
            if (s >= ns) continue;
            const uint32_t len = (uint32_t)sn.len, grow = rd.word(SN_B(s));
            const uint32_t top = len + (grow > len ? grow - len : 0u);  // piece 0's lifetime before the cap: len < 2^16, no wrap
            rd.for_each_piece(sn, [&](int i, uint32_t c, bool valid) {
                const int x = cell_c0(c), y = cell_c1(c);
                uint32_t l = top - (uint32_t)i;   // (i < len for a valid piece)
                l = l > 0xFFFEu ? 0xFFFEu : l;
                l = never ? MSNAKE_LIFE_NEVER : l;
                if (valid && x >= 0 && x < dim && y >= 0 && y < dim)
                    __hip_atomic_fetch_max(&img[x * dim + y], l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            });
        }
        wave_sync();

        if (LIFE) {
            // the image leaves as it lies: [c0][c1], two entries per dword from the first 4-byte aligned entry on
            uint16_t* const dst = a.life + (size_t)e * n2;
            const int odd = (int)(((uintptr_t)dst >> 1) & 1u);
            const int pairs = (n2 - odd) >> 1, last = odd + 2 * pairs;
            uint32_t* const dst2 = reinterpret_cast<uint32_t*>(dst + odd);
            for (int p = lane; p < pairs; p += 64) dst2[p] = img[odd + 2 * p] | (img[odd + 2 * p + 1] << 16);
            if (lane == 0 && odd) dst[0] = (uint16_t)img[0];
            if (lane == 0 && last < n2) dst[last] = (uint16_t)img[last];
        }
    }

    if (ACT || REACH) {
        // ---- segments: lanes g * (dim + 1) + y, y < dim, hold row y of the board for the g-th fill of a group; lane
        // g * (dim + 1) + dim is a blocked row between two boards, and so are the lanes behind the last segment
        const int seg = dim + 1, nseg = 64 / seg;                        // wave-uniform; nseg >= 1 (dim <= 62)
        const int my_seg = lane / seg, y = lane - my_seg * seg;
        const bool in_row = my_seg < nseg && y < dim;
        const uint64_t grid = in_row ? (1ull << dim) - 1ull : 0ull;
        const uint64_t used = grid & ~gather_row(b.vacant, in_row ? y : 0);  // (every lane takes part in the gather)

        // ---- the lifetimes of this lane's row, bit-sliced and inverted; only the cells of `used` hold anything
        const uint32_t cap = (1u << (32 - __builtin_clz((uint32_t)n2 + 4u))) - 1u;   // >= every level: never admitted
        uint64_t nplane[TIMED_PLANES];
#pragma unroll
        for (int k = 0; k < TIMED_PLANES; ++k) nplane[k] = ~0ull;
        uint64_t lasting = 0ull;  // the cells whose lifetime no level reaches
        uint32_t longest = 0u;    // the largest lifetime below `cap` in this row
        for (uint64_t rest = used; rest != 0ull; rest &= rest - 1ull) {  // (rest != 0 only in rows of the grid)
            const uint64_t bit = rest & (0ull - rest);
            uint32_t l = img[__builtin_ctzll(rest) * dim + y];
            l = l > cap ? cap : l;
            lasting |= l == cap ? bit : 0ull;
            longest = l != cap && l > longest ? l : longest;
#pragma unroll
            for (int k = 0; k < TIMED_PLANES; ++k) nplane[k] &= ((l >> k) & 1u) ? ~bit : ~0ull;
        }
        // from level `longest` + 1 on every cell but the lasting ones is admitted: no compare; below it the planes above
        // the highest bit of `longest` decide nothing (a lasting cell is all ones in the lower planes: >= every such level)
        longest = wave_reduce(longest, [](uint32_t p, uint32_t q) { return p > q ? p : q; });
        const int planes = 32 - __builtin_clz(longest | 1u);             // wave-uniform, <= TIMED_PLANES
        const uint64_t settled = grid & ~lasting;
        // the row mask of the cells in the grid with Life < t (t wave-uniform, 1 <= t <= cap)
        auto admit = [&](uint32_t t) {
            if (t > longest) return settled;
            uint64_t lt = 0ull;
#pragma unroll
            for (int k = 0; k < TIMED_PLANES; ++k) {
                if (k >= planes) break;
                const uint64_t tk = 0ull - (uint64_t)((t >> k) & 1u);
                lt = (nplane[k] & lt) | (tk & (nplane[k] | lt));  // majority: t's bit 1 -> ~a | lt, 0 -> ~a & lt
            }
            return lt & settled;
        };

        // ---- one fill per open candidate, nseg of them side by side
        uint32_t pending = open_all;
        for (int guard = 0; pending != 0u && guard < 16; ++guard) {
            const uint32_t group = pending;
            uint64_t front = 0ull;
            for (int g = 0; g < nseg && pending != 0u; ++g) {
                const int k = __builtin_ctz(pending);
                pending &= pending - 1u;
                const int sx = (int)rdlane((uint32_t)b.gx, k), sy = (int)rdlane((uint32_t)b.gy, k);
                front |= lane == g * seg + sy ? 1ull << sx : 0ull;
            }
            uint64_t seen = front;
            uint32_t t = 1u;
            for (int levels = 1; levels < n2; levels += 4) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint64_t fresh = neighbours(front) & ~seen & admit(++t);
                    seen |= fresh;
                    front = fresh;
                }
                if (__ballot(front != 0ull) == 0ull) break;
            }
            const uint32_t mine = (uint32_t)__popcll(seen);
            uint32_t rest = group;
            for (int g = 0; g < nseg && rest != 0u; ++g) {
                const int k = __builtin_ctz(rest);
                rest &= rest - 1u;
                const uint32_t cells = wave_sum(my_seg == g ? mine : 0u);
                if (lane == k) reach = cells;
            }
        }
    }

    // ---- timed_greedy: space_greedy's choice with the timed reach in place of the space
    uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) act[s] = 0u;
    if (ACT) greedy_by_count(rd, ns, lane, open_all, reach, b.my_len, b.hx, b.hy, act);

    // lane s owns snake s's action word and mask byte, lane 4 s + m the reach of move m + 1
    if (lane < ns) {
        const uint32_t my_act = lane == 0 ? act[0] : lane == 1 ? act[1] : lane == 2 ? act[2] : act[3];
        if (ACT && ((a.mask >> lane) & 1u)) a.actions[(size_t)e * a.stride + lane] = (int32_t)my_act;
        if (SAFE) a.safe[(size_t)e * ns + lane] = (uint8_t)(((open_all >> (4 * lane)) & 15u) << 1);
    }
    if (REACH && lane < 4 * ns) a.reach[(size_t)e * ns * 4 + lane] = (uint16_t)reach;
}

hipError_t launch_timed(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                        uint16_t* reach, uint16_t* life, hipStream_t stream) {
    const TimedArgs a{state_view(p, rules), actions, safe, reach, life, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + SPACE_WAVES - 1) / SPACE_WAVES)), block(SPACE_WAVES * 64);
    const size_t image_bytes = (size_t)SPACE_WAVES * p.dim * p.dim * sizeof(uint32_t);  // at dim 62: 61 504, with occ under 64 KB
    return launch_by_flags<4>((snake_mask != 0u ? 8 : 0) | (safe ? 4 : 0) | (reach ? 2 : 0) | (life ? 1 : 0),
                              [&](auto act, auto sf, auto rc, auto lf) {
        hipLaunchKernelGGL((msnake_timed_kernel<act.value, sf.value, rc.value, lf.value>), grid, block, image_bytes, stream, a);
    });
}

}  // namespace msnake
