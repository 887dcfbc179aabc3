// msnake_heads.inc -- every snake's BFS distance to every cell, the Voronoi owner map and the owned-cell counts
// (msnake_head_fields).  Included behind msnake_path.inc by msnake_opponents.hip: it uses msnake_space.inc's
// Board / read_board and wave_sum and msnake_territory.inc's neighbours.  Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader.  Occupancy and the 16 candidates
// (lane 4 s + m <-> move m + 1 of snake s) are read_board's, exactly as msnake_space_kernel has them.
//   * One front per snake, a row-per-lane mask like the fills of the siblings, seeded at level 1 with the targets of the
//     snake's open moves.  All fronts advance in ONE level-synchronous loop: grown = front | (N(front) & vacant),
//     new = grown & ~front.  Bodies are static, so a front runs through cells that another snake owns.  Four levels per
//     convergence ballot; a front gains a cell per level until it stops, so dim^2 levels cut the loop whatever the record
//     says.  With planes to write the loop runs until no front gains a cell.  Without, it ends as soon as a group of levels
//     claimed no cell: a claimed cell's free neighbours are claimed one level later at the latest, so a level without a
//     fresh cell is followed by none with one, and the fronts need not run each other's territory to its end.
//   * The race: a cell's owner is decided at the first level at which any front reaches it.  fresh = (OR of the new
//     sets) & ~claimed; snake s takes new_s & fresh & ~(OR of the other new sets), the rest of fresh is a tie and stays
//     in `claimed` alone.  Bit work on 64-bit rows: no LDS and no memory access in the race.  own_s stays in registers
//     to the end: the owner bytes leave once, one coalesced byte store per column, and a count is one popcount per lane
//     and a wave_sum.
//   * Only the fronts somebody needs run: every snake's when the owner map or the counts are written (RACE), else the
//     selected snakes' alone.
//   * The distance planes, STAGED: the selected planes are staged in wave-private dynamic LDS, P * ceil(dim^2 / 2) dwords
//     per wave sized by the call (a small board does not pay for the largest), set to MSNAKE_HEAD_NONE first; a level's
//     new cells receive the level there (c0 = bit, c1 = lane -> entry c0 * dim + c1), the head cell 0, and each plane
//     leaves in coalesced 4-byte stores (dist_dev is only 2-byte aligned: an odd first and last entry go alone).
//     !STAGED: no image.  A new cell's level goes straight to HBM, and the cells a front never reached receive NONE or
//     the head's 0 in one pass at the end.  Either way every entry of every selected plane is written exactly once per
//     call.  The launcher stages while one wave's planes fit HEADS_STAGE_BYTES (measured: DESIGN.md, section 21: the
//     image wins while it is small and loses once it costs the waves per CU).  The experiment builds MSNAKE_HEADS_DIRECT
//     and MSNAKE_HEADS_STAGED (tools/heads_cost.py --ab, never shipped) force one way for every shape; the second halves
//     the waves per workgroup until the planes fit 64 KiB.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct HeadsArgs {
    StateView v;
    uint16_t* dist; uint8_t* owner; uint16_t* counts;
    uint32_t mask;        // the snakes whose planes are written (0 when dist is NULL)
    int32_t waves;        // waves (envs) per workgroup
    int32_t plane_words;  // the staged image of one plane, in dwords
};

constexpr size_t HEADS_STAGE_BYTES = 8 * 1024;  // the planes of one wave that are still staged (msnake_path_kernel's field: 7 688)

// DIST / OWNER / COUNTS: dist_dev / owner_dev / counts_dev are written; STAGED: the planes leave through an LDS image
template <bool DIST, bool OWNER, bool COUNTS, bool STAGED>
__global__ __launch_bounds__(SPACE_WAVES * 64) void msnake_heads_kernel(HeadsArgs a) {
    __shared__ uint32_t occ[SPACE_WAVES][128];  // per wave: row y = words 2 y (bits 0..31) and 2 y + 1 (bits 32..63)
    extern __shared__ uint32_t heads_planes[];  // per wave: the selected planes, entry c0 * dim + c1 (uint16)
    constexpr bool RACE = OWNER || COUNTS;
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * (uint32_t)a.waves + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int ns = a.v.ns, dim = a.v.dim, n2 = dim * dim;
    const uint32_t sel = DIST ? a.mask & ((1u << ns) - 1u) : 0u;
    const uint32_t run = RACE ? (1u << ns) - 1u : sel;
    const int P = __builtin_popcount(sel);
    const EnvReader rd(a.v, e, lane);
    uint32_t* const img32 = heads_planes + (size_t)wave * P * a.plane_words;
    uint16_t* const img = reinterpret_cast<uint16_t*>(img32);
    const int plane_entries = 2 * a.plane_words;
    if (DIST && STAGED)
        for (int i = lane; i < P * a.plane_words; i += 64) img32[i] = 0xFFFFFFFFu;  // MSNAKE_HEAD_NONE twice
    const Board b = read_board(a.v, rd, occ[wave], lane);  // (its wave_sync calls order the stores above as well)
    const uint64_t vacant = b.vacant;
    const uint32_t open_all = b.open_all;

    // ---- level 1: the targets of every running snake's open moves
    uint64_t front[MSNAKE_MAX_SNAKES], news[MSNAKE_MAX_SNAKES], own[MSNAKE_MAX_SNAKES];
    int plane[MSNAKE_MAX_SNAKES];  // snake s's plane among the selected ones
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        uint64_t seed = 0ull;
        if ((run >> s) & 1u) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (!((open_all >> (4 * s + m)) & 1u)) continue;
                const int sx = (int)rdlane((uint32_t)b.gx, 4 * s + m), sy = (int)rdlane((uint32_t)b.gy, 4 * s + m);
                seed |= lane == sy ? 1ull << sx : 0ull;
            }
        }
        front[s] = news[s] = seed;
        own[s] = 0ull;
        plane[s] = __builtin_popcount(sel & ((1u << s) - 1u));
    }
    uint64_t claimed = 0ull;

    // what a level's new cells leave behind: the race's verdict, and the level in the selected planes.  Returns what keeps
    // the loop going: the cells the fronts gained (planes to write) or the cells the race claimed (none)
    auto settle = [&](uint32_t level) -> uint64_t {
        const uint64_t any = news[0] | news[1] | news[2] | news[3];
        uint64_t fresh = any;
        if (RACE) {
            fresh = any & ~claimed;
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                uint64_t others = 0ull;
#pragma unroll
                for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) others |= k != s ? news[k] : 0ull;
                own[s] |= news[s] & fresh & ~others;
            }
            claimed |= fresh;
        }
        if (DIST) {
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                if (!((sel >> s) & 1u)) continue;
                uint16_t* const plane_img = img + (size_t)plane[s] * plane_entries;
                uint16_t* const plane_dev = a.dist + ((size_t)e * P + plane[s]) * n2;
                for (uint64_t nb = news[s]; nb != 0ull; nb &= nb - 1ull) {  // (news != 0 only in lanes < dim)
                    const int at = __builtin_ctzll(nb) * dim + lane;
                    if (STAGED) plane_img[at] = (uint16_t)level;
                    else plane_dev[at] = (uint16_t)level;
                }
            }
        }
        return DIST ? any : fresh;
    };

    // ---- the fronts, level by level
    uint32_t level = 1u;
    (void)settle(level);
    for (int sweeps = 1; sweeps < n2; sweeps += 4) {
        uint64_t gained = 0ull;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                if ((run >> s) & 1u) {
                    const uint64_t grown = front[s] | (neighbours(front[s]) & vacant);
                    news[s] = grown ^ front[s];
                    front[s] = grown;
                } else {
                    news[s] = 0ull;
                }
            }
            gained |= settle(++level);
        }
        if (__ballot(gained != 0ull) == 0ull) break;
    }

    // ---- the planes leave
    if (DIST) {
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (!((sel >> s) & 1u)) continue;
            const int hx = b.hx[s], hy = b.hy[s];  // (-2, -2) for an empty body: no cell
            uint16_t* const dst = a.dist + ((size_t)e * P + plane[s]) * n2;
            if (STAGED) {
                uint16_t* const pl = img + (size_t)plane[s] * plane_entries;
                wave_sync();
                if (lane == 0 && hx >= 0 && hx < dim && hy >= 0 && hy < dim) pl[hx * dim + hy] = 0;
                wave_sync();
                // the image leaves as it lies: [c0][c1], in dwords from the first 4-byte aligned entry on
                const int odd = (int)(((uintptr_t)dst >> 1) & 1u);
                const int pairs = (n2 - odd) >> 1, last = odd + 2 * pairs;
                uint32_t* const dst2 = reinterpret_cast<uint32_t*>(dst + odd);
                for (int p = lane; p < pairs; p += 64)
                    dst2[p] = (uint32_t)pl[odd + 2 * p] | ((uint32_t)pl[odd + 2 * p + 1] << 16);
                if (lane == 0 && odd) dst[0] = pl[0];
                if (lane == 0 && last < n2) dst[last] = pl[last];
            } else {
                // the cells the front never took: the head's 0, NONE everywhere else (bodies, walled-off regions)
                for (int x = 0; x < dim; ++x)
                    if (lane < dim && !((front[s] >> x) & 1ull))
                        dst[x * dim + lane] = x == hx && lane == hy ? (uint16_t)0 : (uint16_t)MSNAKE_HEAD_NONE;
            }
        }
    }

    // ---- the owner map: column c0 = x is one coalesced byte store of the lanes c1 < dim
    if (OWNER) {
        const uint64_t tie = claimed & ~(own[0] | own[1] | own[2] | own[3]);
        uint8_t* const dst = a.owner + (size_t)e * n2;
        for (int x = 0; x < dim; ++x) {
            const uint32_t o = (own[0] >> x) & 1ull ? 0u : (own[1] >> x) & 1ull ? 1u : (own[2] >> x) & 1ull ? 2u : (own[3] >> x) & 1ull ? 3u :
                               (tie >> x) & 1ull ? MSNAKE_OWNER_TIE : MSNAKE_OWNER_NONE;
            if (lane < dim) dst[x * dim + lane] = (uint8_t)o;
        }
    }

    // ---- the counts: lane s keeps snake s's
    if (COUNTS) {
        uint32_t mine = 0u;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns) continue;
            const uint32_t cells = wave_sum((uint32_t)__popcll(own[s]));
            if (lane == s) mine = cells;
        }
        if (lane < ns) a.counts[(size_t)e * ns + lane] = (uint16_t)mine;
    }
}

hipError_t launch_heads(const StepParams& p, int rules, uint32_t snake_mask, uint16_t* dist, uint8_t* owner, uint16_t* counts,
                        hipStream_t stream) {
    HeadsArgs a{state_view(p, rules), dist, owner, counts, dist ? snake_mask : 0u, SPACE_WAVES, 0};
    const size_t plane_bytes = (size_t)((p.dim * p.dim + 1) / 2) * sizeof(uint32_t);
    const size_t per_wave = (size_t)__builtin_popcount(a.mask) * plane_bytes;
#if defined(MSNAKE_HEADS_DIRECT)
    const bool staged = false;
#elif defined(MSNAKE_HEADS_STAGED)
    const bool staged = dist != nullptr;
#else
    const bool staged = dist != nullptr && per_wave <= HEADS_STAGE_BYTES;
#endif
    size_t image_bytes = 0;
    if (staged) {
        a.plane_words = (int32_t)(plane_bytes / sizeof(uint32_t));
        const size_t room = 64 * 1024 - sizeof(uint32_t) * SPACE_WAVES * 128;  // a workgroup's LDS less the occupancy images
        while (a.waves > 1 && a.waves * per_wave > room) a.waves >>= 1;        // (MSNAKE_HEADS_STAGED only; one wave: <= 30 752 bytes)
        image_bytes = a.waves * per_wave;
    }
    const dim3 grid((unsigned)((p.nenv + a.waves - 1) / a.waves)), block((unsigned)a.waves * 64);
    const int flags = (dist ? 4 : 0) | (owner ? 2 : 0) | (counts ? 1 : 0);
    if (staged)
        return launch_by_flags<3>(flags, [&](auto ds, auto ow, auto ct) {
            if constexpr (ds.value)
                hipLaunchKernelGGL((msnake_heads_kernel<true, ow.value, ct.value, true>), grid, block, image_bytes, stream, a);
        });
    return launch_by_flags<3>(flags, [&](auto ds, auto ow, auto ct) {
        hipLaunchKernelGGL((msnake_heads_kernel<ds.value, ow.value, ct.value, false>), grid, block, 0, stream, a);
    });
}

}  // namespace msnake
