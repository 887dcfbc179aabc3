// msnake_path.inc -- BFS distances to the fruits, the whole distance field, and the opponent path_greedy
// (msnake_path_actions).  Included behind msnake_territory.inc by msnake_opponents.hip: it uses msnake_space.inc's
// Board / read_board, gather_row, region_sizes, eligible_moves and greedy_among and msnake_territory.inc's neighbours.
// Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader.  Occupancy and the 16 candidates
// (lane 4 s + m <-> move m + 1 of snake s) are read_board's, exactly as msnake_space_kernel has them.
//   * Sources: the fruits arrive lane-distributed (for_each_fruit) and are scattered into a second wave-private row
//     image in LDS, one ds_or per fruit inside the grid, like the body cells; every lane reads its row once and masks it
//     with `vacant`.  A fruit outside the grid or under a body is no source, duplicates fall together.
//   * The BFS is ONE multi-source fill per env: front' = front | (N(front) & vacant), one level per sweep, with the
//     space kernel's sweep (shifts and two DPP row moves, no LDS traffic).  The level is counted inside the unrolled
//     group of four sweeps; one ballot per group ends the loop when a group gained nothing, and dim^2 sweeps cut it
//     whatever the record says.
//   * Reading off the levels, FIELD (field_dev is written): the field is staged in a wave-private LDS image of dim^2
//     uint16, set to MSNAKE_PATH_NONE first; at each level a lane writes the level for the new bits of its row (c0 = bit,
//     c1 = lane -> entry c0 * dim + c1).  In the end lane 4 s + m reads its target's entry, and the image leaves in
//     coalesced 4-byte stores (field_dev is only 2-byte aligned: an odd first and last entry go alone).
//   * Reading off the levels, !FIELD: no image.  `cand` holds the open targets as a row-per-lane mask (scattered through
//     the occupancy image, which read_board is done with).  Only on a level whose new cells hit `cand` does one
//     gather_row hand the level to those candidates, and the fill ends as soon as every open target has its level.
//   * path_greedy: the eligible moves are space_greedy's (region_sizes, eligible_moves: computed only when actions are
//     written).  Lane 4 s + m holds path << 3 | move for an eligible move with a finite path, all ones otherwise; two
//     quad-permute DPP steps give every quad its minimum.  A snake that has eligible moves and no finite path among them
//     takes space_greedy's own choice (greedy_among), which is evaluated only if such a snake exists in the env.
//   * lane s stores snake s's action word and mask byte, lane 4 s + m the path of move m + 1.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct PathArgs {
    StateView v;
    int32_t* actions; uint8_t* safe; uint16_t* path; uint16_t* field;
    int32_t stride;
    uint32_t mask;
};

constexpr int PATH_FIELD_WORDS = (MSNAKE_MAX_DIM * MSNAKE_MAX_DIM + 1) / 2;  // the staged field of one wave, in dwords

// ACT: the path_greedy actions are written (snake_mask != 0); SAFE / PATH / FIELD: safe_dev / path_dev / field_dev are written
template <bool ACT, bool SAFE, bool PATH, bool FIELD>
__global__ __launch_bounds__(SPACE_WAVES * 64) void msnake_path_kernel(PathArgs a) {
    __shared__ uint32_t occ[SPACE_WAVES][128];  // per wave: row y = words 2 y (bits 0..31) and 2 y + 1 (bits 32..63)
    __shared__ uint32_t src[SPACE_WAVES][128];  // the same for the fruits
    __shared__ uint32_t staged[FIELD ? SPACE_WAVES : 1][FIELD ? PATH_FIELD_WORDS : 1];
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * SPACE_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int ns = a.v.ns, dim = a.v.dim, n2 = dim * dim;
    const EnvReader rd(a.v, e, lane);
    uint32_t* const my = occ[wave];
    uint32_t* const mysrc = src[wave];
    uint16_t* const img = reinterpret_cast<uint16_t*>(staged[FIELD ? wave : 0]);
    mysrc[lane] = 0u;
    mysrc[64 + lane] = 0u;
    const Board b = read_board(a.v, rd, my, lane);  // (its wave_sync calls order the two stores above as well)
    const uint64_t vacant = b.vacant;
    const int gx = b.gx, gy = b.gy;
    const uint32_t open_all = b.open_all;
    const bool my_open = lane < 16 && ((open_all >> lane) & 1u);

    // ---- space_greedy's eligible moves
    uint32_t elig_all = 0u;
    if (ACT) elig_all = eligible_moves(lane, open_all, region_sizes(b, dim, lane), b.my_len);

    uint32_t path = MSNAKE_PATH_NONE;  // lane 4 s + m: F(target of move m + 1 of snake s)
    if (ACT || PATH || FIELD) {
        // ---- sources: every fruit inside the grid sets its bit; a body on top of it takes it away again
        rd.for_each_fruit([&](int, uint32_t c, bool valid) {
            const int x = cell_c0(c), y = cell_c1(c);
            if (valid && x >= 0 && x < dim && y >= 0 && y < dim)
                __hip_atomic_fetch_or(&mysrc[2 * y + (x >> 5)], 1u << (x & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        });
        uint64_t cand = 0ull;  // !FIELD: the open targets that have no level yet
        if (FIELD) {
            for (int i = lane; i < (n2 + 1) >> 1; i += 64) staged[wave][i] = 0xFFFFFFFFu;  // MSNAKE_PATH_NONE twice
        } else {
            my[lane] = 0u;
            my[64 + lane] = 0u;
            wave_sync();
            if (my_open) __hip_atomic_fetch_or(&my[2 * gy + (gx >> 5)], 1u << (gx & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        wave_sync();
        uint64_t front = ((uint64_t)mysrc[2 * lane] | ((uint64_t)mysrc[2 * lane + 1] << 32)) & vacant;
        if (!FIELD) cand = (uint64_t)my[2 * lane] | ((uint64_t)my[2 * lane + 1] << 32);

        // what a level's new cells `fresh` leave behind
        auto record = [&](uint64_t fresh, uint32_t level) {
            if (FIELD) {
                for (uint64_t nb = fresh; nb != 0ull; nb &= nb - 1ull)  // (fresh != 0 only in lanes < dim)
                    img[__builtin_ctzll(nb) * dim + lane] = (uint16_t)level;
            } else if (__ballot((fresh & cand) != 0ull) != 0ull) {
                const uint64_t hit_row = gather_row(fresh, gy);
                if (my_open && ((hit_row >> gx) & 1ull)) path = level;
                cand &= ~fresh;
            }
        };

        // ---- the fill, level by level
        uint32_t level = 0u;
        record(front, level);
        for (int sweeps = 0; sweeps < n2; sweeps += 4) {
            const uint64_t before = front;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint64_t grown = front | (neighbours(front) & vacant);
                record(grown ^ front, ++level);
                front = grown;
            }
            if (__ballot(front != before) == 0ull) break;
            if (!FIELD && __ballot(cand != 0ull) == 0ull) break;
        }

        if (FIELD) {
            wave_sync();
            if (my_open) path = img[gx * dim + gy];
            // the image leaves as it lies: [c0][c1], in dwords from the first 4-byte aligned entry on
            uint16_t* const dst = a.field + (size_t)e * n2;
            const int odd = (int)(((uintptr_t)dst >> 1) & 1u);
            const int pairs = (n2 - odd) >> 1, last = odd + 2 * pairs;
            uint32_t* const dst2 = reinterpret_cast<uint32_t*>(dst + odd);
            for (int p = lane; p < pairs; p += 64)
                dst2[p] = (uint32_t)img[odd + 2 * p] | ((uint32_t)img[odd + 2 * p + 1] << 16);
            if (lane == 0 && odd) dst[0] = img[0];
            if (lane == 0 && last < n2) dst[last] = img[last];
        }
    }

    // ---- path_greedy: the smallest finite path among the eligible moves, else space_greedy's choice among them
    uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) act[s] = 0u;
    if (ACT) {
        const bool elig = lane < 16 && ((elig_all >> lane) & 1u);
        uint32_t key = elig && path != MSNAKE_PATH_NONE ? (path << 3) | (uint32_t)((lane & 3) + 1) : 0xFFFFFFFFu;
        uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0xB1, 0xF, 0xF, true);  // quad_perm:[1,0,3,2]
        key = key < o ? key : o;
        o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)key, 0x4E, 0xF, 0xF, true);           // quad_perm:[2,3,0,1]
        key = key < o ? key : o;
        const uint32_t lost = (uint32_t)__ballot(elig && key == 0xFFFFFFFFu);  // the eligible moves of snakes without a finite path
        if (lost != 0u) greedy_among(rd, ns, lane, lost, b.hx, b.hy, act);
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            const uint32_t k = rdlane(key, 4 * s);
            if (k != 0xFFFFFFFFu) act[s] = k & 7u;
        }
    }

    // lane s owns snake s's action word and mask byte, lane 4 s + m the path of move m + 1
    if (lane < ns) {
        const uint32_t my_act = lane == 0 ? act[0] : lane == 1 ? act[1] : lane == 2 ? act[2] : act[3];
        if (ACT && ((a.mask >> lane) & 1u)) a.actions[(size_t)e * a.stride + lane] = (int32_t)my_act;
        if (SAFE) a.safe[(size_t)e * ns + lane] = (uint8_t)(((open_all >> (4 * lane)) & 15u) << 1);
    }
    if (PATH && lane < 4 * ns) a.path[(size_t)e * ns * 4 + lane] = (uint16_t)path;
}

hipError_t launch_path(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* safe,
                       uint16_t* path, uint16_t* field, hipStream_t stream) {
    const PathArgs a{state_view(p, rules), actions, safe, path, field, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + SPACE_WAVES - 1) / SPACE_WAVES)), block(SPACE_WAVES * 64);
    return launch_by_flags<4>((snake_mask != 0u ? 8 : 0) | (safe ? 4 : 0) | (path ? 2 : 0) | (field ? 1 : 0),
                              [&](auto act, auto sf, auto pt, auto fd) {
        hipLaunchKernelGGL((msnake_path_kernel<act.value, sf.value, pt.value, fd.value>), grid, block, 0, stream, a);
    });
}

}  // namespace msnake
