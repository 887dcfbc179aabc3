// msnake_rays.inc -- eight-direction ray observations per snake (msnake_render_rays).
// Included behind msnake_local.inc, last, by msnake_opponents.hip: it uses that file's board painter (paint_snake_board) and
// LOCAL_WAVES, and msnake_device.h's wave helpers.  Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader (msnake_envread.inc).
//   * Board: the snake-indexed plane of msnake_local_kernel, painted by the same function into the wave's own slice of
//     dynamic LDS (dim^2 bytes in whole dwords per wave).
//   * Rays: per selected snake, lane l owns direction j = l / 8 and the steps t = (l % 8) + 1 + 8 p of pass p = 0 ..
//     ceil(dim / 8) - 1: all eight rays of a snake advance together, eight steps per pass, and everything per ray is
//     vector work.  The wall needs no search: the grid is convex and a head sits in [-1, dim]^2, so the steps inside the
//     grid are exactly t < wall, and the wall is where the first axis leaves -- dim - h along +1, h + 1 along -1, and an
//     axis the ray does not move along is inside always or never (1 <= wall <= dim + 1 <= 63).  A lane whose step lies
//     below its wall reads its board byte (the others read byte 0 and count as empty) and classifies it for this snake --
//     fruit: 1; own: (b - 2) >> 1 == s; another's: any other body or head -- and keeps per channel the smallest t it has
//     seen, 255 for none.  After the last pass three DPP steps per channel (quad_perm xor 1, xor 2, row_half_mirror) take
//     the minimum over the eight lanes of a direction.  Lane 8 j packs the four bytes of direction j into one dword and
//     stores it: one store instruction of 8 consecutive dwords per snake.
//     (Two earlier versions gave lane t - 1 step t of ONE ray and took the distances from ballots: 24 rays per env one
//     after the other, each with about 95 instructions, most of them wave-uniform work on the CU's one scalar unit:
//     13-16 us per call for three snakes at 4 096 envs against 7.1 us for the radius-5 windows; see DESIGN.md, section 16.)
//   * Heading: lane q < S stores the heading of the q-th selected snake, as msnake_local_kernel does.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct RaysArgs {
    StateView v;
    uint32_t* rays; uint8_t* heading;  // rays: one dword per (env, slot, direction)
    int32_t nsel;                      // S = popcount(snake_mask)
    uint32_t sel4;                     // the snake of slot q in bits 4 q .. 4 q + 3
    int32_t oriented;
    int32_t slice_words;               // dwords of LDS per wave: dim^2 bytes in whole dwords
};

// Board direction jj = 0..7 is (1,0) (1,1) (0,1) (-1,1) (-1,0) (-1,-1) (0,-1) (1,-1): move jj / 2 of the move table, plus
// the move after it when jj is odd.  ray_table(axis): component `axis` of every direction, plus 1, in bits 2 jj .. 2 jj + 1.
MSNAKE_HD uint32_t ray_table(int axis) {
    uint32_t tab = 0u;
    for (int jj = 0; jj < MSNAKE_RAY_DIRS; ++jj) {
        const int m = jj >> 1, m1 = (m + 1) & 3;
        const int d = axis == 0 ? move_d0(m) + ((jj & 1) ? move_d0(m1) : 0) : move_d1(m) + ((jj & 1) ? move_d1(m1) : 0);
        tab |= (uint32_t)(d + 1) << (2 * jj);
    }
    return tab;
}
static_assert(ray_table(0) == 0x901Au && ray_table(1) == 0x01A9u, "the eight directions");

constexpr int RAY_NONE = 255;  // "no such cell on the ray so far": above every step there is
// min over the eight lanes of a direction (lanes 8 j .. 8 j + 7), in every one of them
__device__ __forceinline__ uint32_t ray_min8(uint32_t v) {
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(RAY_NONE, (int)v, 0xB1, 0xF, 0xF, false);  // quad_perm:[1,0,3,2]
    v = o < v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(RAY_NONE, (int)v, 0x4E, 0xF, 0xF, false);           // quad_perm:[2,3,0,1]
    v = o < v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(RAY_NONE, (int)v, 0x141, 0xF, 0xF, false);          // row_half_mirror: lane i <- 7 - i
    return o < v ? o : v;
}

__global__ __launch_bounds__(LOCAL_WAVES * 64) void msnake_rays_kernel(RaysArgs a) {
    extern __shared__ uint32_t rays_lds[];  // LOCAL_WAVES slices of a.slice_words dwords
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * LOCAL_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int dim = a.v.dim;
    const EnvReader rd(a.v, e, lane);
    uint32_t* board32 = rays_lds + wave * a.slice_words;
    const uint8_t* board = reinterpret_cast<const uint8_t*>(board32);
    uint32_t par[MSNAKE_MAX_SNAKES];
    paint_snake_board(a.v, rd, lane, board32, a.slice_words, par);

    // ---- heading: lane q <-> the q-th selected snake
    const auto slot_par = [&](int q, int& snake) {
        snake = (int)((a.sel4 >> (4 * q)) & 15u);
        return snake == 0 ? par[0] : snake == 1 ? par[1] : snake == 2 ? par[2] : par[3];
    };
    if (a.heading && lane < a.nsel) {
        int snake;
        a.heading[(size_t)e * a.nsel + lane] = (uint8_t)((slot_par(lane, snake) >> 20) & 3u);
    }

    // ---- rays: lane l <-> direction l / 8, steps (l % 8) + 1 + 8 p
    const int j = lane >> 3, t0 = (lane & 7) + 1;
    const int passes = (dim + 7) >> 3;  // the last step inside the grid is t = wall - 1 <= dim
    uint32_t* out = a.rays + (size_t)e * (size_t)(MSNAKE_RAY_DIRS * a.nsel);
    for (int q = 0; q < a.nsel; ++q) {
        int snake;
        const uint32_t p = slot_par(q, snake);
        uint32_t w = 0u;  // an empty body: 32 zeros
        if (p >> 22) {
            const int hx = (int)(p & 1023u) - 2, hy = (int)((p >> 10) & 1023u) - 2;
            const int turn = a.oriented ? 2 * (int)((p >> 20) & 3u) : 0;  // direction j of heading k is board direction j + 2 k
            const int jj = (j + turn) & 7;
            const int d0 = (int)((ray_table(0) >> (2 * jj)) & 3u) - 1, d1 = (int)((ray_table(1) >> (2 * jj)) & 3u) - 1;
            // an axis the ray does not move along is inside for every step or for none
            const int rest0 = (uint32_t)hx < (uint32_t)dim ? 64 : 1, rest1 = (uint32_t)hy < (uint32_t)dim ? 64 : 1;
            const int w0 = d0 > 0 ? dim - hx : d0 < 0 ? hx + 1 : rest0, w1 = d1 > 0 ? dim - hy : d1 < 0 ? hy + 1 : rest1;
            const int wmin = w0 < w1 ? w0 : w1;
            const int wall = wmin > 1 ? wmin : 1;
            const int head_idx = hx * dim + hy, stride = d0 * dim + d1;
            uint32_t fruit = RAY_NONE, own = RAY_NONE, other = RAY_NONE;
            for (int pass = 0; pass < passes; ++pass) {
                const int t = t0 + 8 * pass;
                const bool active = t < wall;  // the cell head + t d lies inside the grid
                const uint32_t b = active ? (uint32_t)board[active ? head_idx + t * stride : 0] : 0u;
                const bool mine = (int)((b - 2u) >> 1) == snake;  // (b < 2 wraps far away from every snake index)
                fruit = b == 1u && (uint32_t)t < fruit ? (uint32_t)t : fruit;
                own = mine && (uint32_t)t < own ? (uint32_t)t : own;
                other = b > 1u && !mine && (uint32_t)t < other ? (uint32_t)t : other;
            }
            fruit = ray_min8(fruit), own = ray_min8(own), other = ray_min8(other);
            w = ((uint32_t)wall << (8 * MSNAKE_RAY_WALL)) | ((fruit == RAY_NONE ? 0u : fruit) << (8 * MSNAKE_RAY_FRUIT)) |
                ((own == RAY_NONE ? 0u : own) << (8 * MSNAKE_RAY_OWN)) | ((other == RAY_NONE ? 0u : other) << (8 * MSNAKE_RAY_OTHER));
        }
        if ((lane & 7) == 0) out[MSNAKE_RAY_DIRS * q + j] = w;
    }
}

hipError_t launch_rays(const StepParams& p, int rules, uint32_t snake_mask, int oriented, uint8_t* rays, uint8_t* heading,
                       hipStream_t stream) {
    uint32_t sel4 = 0u;
    int nsel = 0;
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        if ((snake_mask >> s) & 1u) sel4 |= (uint32_t)s << (4 * nsel++);
    if (nsel == 0 || ((uintptr_t)rays & 3)) return hipErrorInvalidValue;
    const int slice_words = (p.dim * p.dim + 3) / 4;
    const RaysArgs a{state_view(p, rules), reinterpret_cast<uint32_t*>(rays), heading, nsel, sel4, oriented, slice_words};
    const size_t lds = (size_t)LOCAL_WAVES * slice_words * 4;  // <= 4 x 3 844 bytes
    const dim3 grid((unsigned)((p.nenv + LOCAL_WAVES - 1) / LOCAL_WAVES)), block(LOCAL_WAVES * 64);
    hipLaunchKernelGGL(msnake_rays_kernel, grid, block, lds, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
