// msnake_local.inc -- head-centred, heading-aligned cell-code windows per snake (msnake_render_local).
// Included behind msnake_timed.inc by msnake_opponents.hip (why there: see that file): it uses msnake_device.h's wave
// helpers and nothing of the opponents.  Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader (msnake_envread.inc).
//   * Board: ONE plane of dim^2 bytes in the wave's own slice of dynamic LDS (4 waves x dim^2 bytes in whole dwords: 1.4 KB
//     per workgroup at 19x19, 15.0 KB at 62x62, whatever the radius and the selection), with snake-indexed codes:
//     0 empty, 1 fruit, 2 + 2 i body of snake i, 3 + 2 i head of snake i.  Painted by paint_snake_board (which
//     msnake_rays_kernel of msnake_rays.inc calls too) in the phases of msnake_cells_kernel
//     -- the fruits, then per snake its body cells, then its head -- as byte stores; all stores of a phase that meet in
//     a byte carry the same value, DS operations of one wave execute in program order, so a later phase wins and
//     wave_sync() (a compiler fence) between the phases is all the ordering this needs.  No workgroup barrier.  The last
//     painter of a cell is the same in every view, so relabelling the code per view (own -> 2 / 3, another's -> 4 / 5)
//     reproduces the planes of msnake_render_cells.
//   * Gather: the env's S windows are ONE contiguous block of S * W^2 bytes in the output.  Lane l of pass p owns the
//     ALIGNED global dword l + 64 p of that block (the block starts `phase` = address & 3 bytes into dword 0) and
//     computes its four bytes: byte o -> (slot, i, j) by two multiply-high divisions (the reciprocals of W^2 and W come
//     from the host), -> the cell head + (i - r) f + (j - r) g, -> the board byte relabelled for the slot's snake, or 6
//     outside the grid, or 0 for an empty body.  A dword that lies inside the block goes out as one dword store; the
//     first and last dword, where they straddle the block's ends, go out as byte stores of the bytes inside.  Nothing
//     is written outside [0, S * W^2) of the env's own block.
//   * Heading: lane q < S stores the heading of the q-th selected snake.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct LocalArgs {
    StateView v;
    uint8_t* windows; uint8_t* heading;
    int32_t radius, W, W2;   // W = 2 radius + 1, W2 = W^2
    uint32_t inv_W, inv_W2;  // floor(2^32 / d) + 1: __umulhi(n, inv) == n / d for every n < 2^14
    int32_t nsel;            // S = popcount(snake_mask)
    uint32_t sel4;           // the snake of slot q in bits 4 q .. 4 q + 3
    int32_t oriented;
    int32_t slice_words;     // dwords of LDS per wave: dim^2 bytes in whole dwords
};

constexpr int LOCAL_WAVES = 4;  // waves (envs) per workgroup

// The snake-indexed board of the env `rd` reads, painted into the wave's slice board32[0 .. slice_words) of LDS; every
// lane of the wave calls it.  Shared by msnake_local_kernel and msnake_rays_kernel (msnake_rays.inc).  par[s] <- what the
// callers need of snake s: head c0 + 2 in bits 0..9, head c1 + 2 in bits 10..19, the heading in 20..21, bit 22 = the body
// is not empty (0 for an empty body and for s >= n_snakes).
__device__ __forceinline__ void paint_snake_board(const StateView& v, const EnvReader& rd, int lane, uint32_t* board32,
                                                  int slice_words, uint32_t (&par)[MSNAKE_MAX_SNAKES]) {
    const int dim = v.dim;
    const bool nw = v.rules == MSNAKE_RULES_NEW_WORLD;
    const uint32_t flags = rd.flags();
    uint8_t* board = reinterpret_cast<uint8_t*>(board32);
    for (int i = lane; i < slice_words; i += 64) board32[i] = 0u;
    wave_sync();

    // a cell inside the grid takes the phase's code; anything else is not stored
    auto paint = [&](uint32_t c, bool valid, uint32_t code) {
        const int c0 = MSNAKE_CELL_C0(c), c1 = MSNAKE_CELL_C1(c);
        if (valid && c0 >= 0 && c0 < dim && c1 >= 0 && c1 < dim) board[c0 * dim + c1] = (uint8_t)code;
    };

    // ---- phase 1: every entry of the fruit list
    rd.for_each_fruit([&](int, uint32_t c, bool valid) { paint(c, valid, 1u); });
    wave_sync();

    // ---- per snake: its body cells (duplicates and piece 0 included), then piece 0 as the head
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        par[s] = 0u;
        if (s >= v.ns) continue;
        const SnakeRef sn = rd.snake(s);
        if (sn.len == 0) continue;  // an empty body: nothing painted, a window of zeros, heading 0
        const uint32_t vel = (rd.word(SN_C(s)) >> 16) & 7u;  // 0 = at rest, 1..4 = the move that keeps the direction
        par[s] = (uint32_t)(sn.x + 2) | ((uint32_t)(sn.y + 2) << 10) | ((vel ? (vel - 1u) & 3u : 0u) << 20) | (1u << 22);
        if (nw && !((flags >> s) & 1u)) continue;  // a dead new_world snake paints nothing
        rd.for_each_piece(sn, [&](int, uint32_t c, bool valid) { paint(c, valid, 2u + 2u * s); });
        wave_sync();
        paint(sn.head, lane == 0, 3u + 2u * s);
        wave_sync();
    }
}

__global__ __launch_bounds__(LOCAL_WAVES * 64) void msnake_local_kernel(LocalArgs a) {
    extern __shared__ uint32_t local_lds[];  // LOCAL_WAVES slices of a.slice_words dwords
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * LOCAL_WAVES + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;  // (no workgroup barrier below)
    const int dim = a.v.dim;
    const EnvReader rd(a.v, e, lane);
    uint32_t* board32 = local_lds + wave * a.slice_words;
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

    // ---- gather: byte o of the env's block, o in [0, total)
    const int total = a.nsel * a.W2;
    const auto window_byte = [&](int o) -> uint32_t {
        const int q = (int)__umulhi((uint32_t)o, a.inv_W2);
        const int rem = o - q * a.W2;
        const int i = (int)__umulhi((uint32_t)rem, a.inv_W);
        const int di = i - a.radius, dj = rem - i * a.W - a.radius;
        int snake;
        const uint32_t p = slot_par(q, snake);
        const int k = a.oriented ? (int)((p >> 20) & 3u) : 0;
        const int f0 = move_d0(k), f1 = move_d1(k);  // g = (-f1, f0)
        const int c0 = (int)(p & 1023u) - 2 + di * f0 - dj * f1, c1 = (int)((p >> 10) & 1023u) - 2 + di * f1 + dj * f0;
        const bool inside = c0 >= 0 && c0 < dim && c1 >= 0 && c1 < dim;
        const uint32_t b = board[inside ? c0 * dim + c1 : 0];
        const uint32_t code = b < 2u ? b : ((int)((b - 2u) >> 1) == snake ? 2u : 4u) + (b & 1u);
        return !(p >> 22) ? 0u : inside ? code : (uint32_t)MSNAKE_CELL_OUTSIDE;
    };
    uint8_t* out = a.windows + (size_t)e * (size_t)total;
    const int phase = (int)((uintptr_t)out & 3u);  // byte o of the block sits in aligned dword (o + phase) >> 2
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out - phase);
    const int ndw = (phase + total + 3) >> 2;
    for (int d = lane; d < ndw; d += 64) {
        const int o0 = 4 * d - phase;
        uint32_t w = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int o = o0 + b;
            const int oc = o < 0 ? 0 : o >= total ? total - 1 : o;  // (a byte outside the block is computed, never stored)
            w |= window_byte(oc) << (8 * b);
        }
        if (o0 >= 0 && o0 + 4 <= total) {
            out32[d] = w;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (o0 + b >= 0 && o0 + b < total) out[o0 + b] = (uint8_t)(w >> (8 * b));
        }
    }
}

hipError_t launch_local(const StepParams& p, int rules, int radius, uint32_t snake_mask, int oriented, uint8_t* windows,
                        uint8_t* heading, hipStream_t stream) {
    uint32_t sel4 = 0u;
    int nsel = 0;
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        if ((snake_mask >> s) & 1u) sel4 |= (uint32_t)s << (4 * nsel++);
    if (nsel == 0 || radius < 1 || radius > MSNAKE_LOCAL_MAX_RADIUS) return hipErrorInvalidValue;
    const int W = 2 * radius + 1, W2 = W * W;  // S * W^2 <= 4 * 3969 < 2^14: the range the reciprocals are exact on
    const int slice_words = (p.dim * p.dim + 3) / 4;
    const LocalArgs a{state_view(p, rules), windows, heading, radius, W, W2, (uint32_t)(0x100000000ull / (uint32_t)W) + 1u,
                      (uint32_t)(0x100000000ull / (uint32_t)W2) + 1u, nsel, sel4, oriented, slice_words};
    const size_t lds = (size_t)LOCAL_WAVES * slice_words * 4;  // <= 4 x 3 844 bytes
    const dim3 grid((unsigned)((p.nenv + LOCAL_WAVES - 1) / LOCAL_WAVES)), block(LOCAL_WAVES * 64);
    hipLaunchKernelGGL(msnake_local_kernel, grid, block, lds, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
