// msnake_cells.inc -- the observation as cell codes and the per-snake table (msnake_render_cells).
// Included behind msnake_copy.inc by msnake_views.hip: it uses msnake_device.h's wave helpers and launch_by_flags.
// Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per env; the wave only READS the handle's state (record by lane, 64-slot rings by lane, overflow rings
// and the adversarial `flist` strided in whole waves), exactly as msnake_space_kernel does.
//   * Image: the env's V planes are ONE contiguous block of V * dim^2 bytes in the output, and every wave composes that
//     block, as it will be stored, in its own slice of dynamic LDS (4 waves x (V * dim^2 + 3 bytes, in whole dwords):
//     4.3 KB per workgroup at 19x19x3, 61.5 KB at the largest shape, 62x62x4).  The block starts `phase` = (global
//     address of the block) & 3 bytes into the slice, so that a byte's LDS address and its global address agree mod 4.
//   * Paint: the frame's order (snake_multiple_test.py:35-58) as phases of byte stores -- the fruits, then per snake its
//     body cells, then its head.  A phase stores one value per plane (fruit 1; body 2 in the plane of the snake's own
//     view and 4 in the others; head 3 / 5), so all stores of a phase that meet in a byte carry the same value, and DS
//     operations of one wave execute in program order: a later phase wins wherever two phases meet, and wave_sync() (a
//     compiler fence) between the phases is all the ordering this needs.  No workgroup barrier -- the waves of the batch
//     tail have returned by then.  A coordinate outside the grid is not stored.
//   * Copy-out: aligned dwords of the slice go to aligned dwords of global memory, lane l <-> dword l + 64 k; the at
//     most 3 bytes in front of the first aligned dword and behind the last go out as byte stores.  Nothing is written
//     outside [0, V * dim^2) of the env's own block.
//   * Table: lane 8 s + f holds field f of snake s (len, head c0, head c1, v0, v1, grow_to, alive, in_dead), read out
//     of the record by v_readlane as msnake_state_pack_kernel derives them: one coalesced store of 8 * n_snakes words.
// No random numbers, no global atomics, no workgroup barrier, no scratch.
namespace msnake {

struct CellsArgs {
    const uint32_t* hdr; const uint16_t* body0; const uint16_t* ovf; const uint16_t* flist;
    uint8_t* cells; int32_t* snakes;
    int32_t nenv, dim, ns, nf, cap, fcap, rules;
    int32_t nplanes;      // V = popcount(view_mask)
    uint32_t views4;      // the view of plane k in bits 4 k .. 4 k + 3
    int32_t slice_words;  // dwords of LDS per wave: (V * dim^2 + 3 bytes of phase) in whole dwords
};

constexpr int CELLS_WAVES = 4;  // waves (envs) per workgroup

// CELLS: cells_dev is written (view_mask != 0); TABLE: snakes_dev is written
template <bool CELLS, bool TABLE>
__global__ __launch_bounds__(CELLS_WAVES * 64) void msnake_cells_kernel(CellsArgs a) {
    extern __shared__ uint32_t cells_lds[];  // CELLS: CELLS_WAVES slices of a.slice_words dwords
    const int lane = (int)(threadIdx.x & 63u);
    const int wave = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * CELLS_WAVES + (threadIdx.x >> 6));
    if (e >= a.nenv) return;  // (no workgroup barrier below)
    const int ns = a.ns, dim = a.dim, n2 = dim * dim;
    const bool nw = a.rules == MSNAKE_RULES_NEW_WORLD;
    const uint32_t hv = a.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];
    uint32_t ring[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        ring[s] = s < ns ? (uint32_t)a.body0[((size_t)e * ns + s) * 64 + lane] : 0u;
    const uint32_t flags = rdlane(hv, HDR_FLAGS);

    if (TABLE) {
        int32_t field = 0;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns) continue;
            const uint32_t wA = rdlane(hv, SN_A(s)), wB = rdlane(hv, SN_B(s)), wC = rdlane(hv, SN_C(s));
            const int len = (int)(wA >> 16), vel = (int)((wC >> 16) & 7u);
            const uint32_t head = rdlane(ring[s], (int)((wC >> SN_C_HP0_SHIFT) & 63u));  // piece 0 sits in ring slot hp0
            const int32_t f[8] = {len, len > 0 ? cell_c0(head) : -2, len > 0 ? cell_c1(head) : -2, vel_v0(vel), vel_v1(vel),
                                  (int32_t)wB, snake_alive(flags, s, nw), snake_in_dead(flags, s, nw)};
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (lane == 8 * s + k) field = f[k];
        }
        if (lane < 8 * ns) a.snakes[(size_t)e * ns * 8 + lane] = field;
    }
    if (!CELLS) return;

    const int total = a.nplanes * n2;
    uint8_t* out = a.cells + (size_t)e * (size_t)total;
    const int phase = (int)((uintptr_t)out & 3u);  // LDS byte phase + o <-> byte o of the env's block: same address mod 4
    uint32_t* img32 = cells_lds + wave * a.slice_words;
    uint8_t* img = reinterpret_cast<uint8_t*>(img32) + phase;
    for (int i = lane; i < a.slice_words; i += 64) img32[i] = 0u;
    wave_sync();

    // a cell inside the grid takes, in every plane, the phase's code for that plane; anything else is not stored
    auto paint = [&](uint32_t c, bool valid, int snake, uint32_t own, uint32_t other) {
        const int c0 = cell_c0(c), c1 = cell_c1(c);
        if (valid && c0 >= 0 && c0 < dim && c1 >= 0 && c1 < dim) {
            uint8_t* p = img + c0 * dim + c1;
#pragma unroll
            for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k)
                if (k < a.nplanes) p[k * n2] = (uint8_t)((int)((a.views4 >> (4 * k)) & 15u) == snake ? own : other);
        }
    };

    // ---- phase 1: every entry of the fruit list
    if (a.rules == MSNAKE_RULES_ADVERSARIAL) {
        int nfr = (int)rdlane(hv, HDR_NLIST);
        nfr = nfr > a.fcap ? a.fcap : nfr;
        for (int base = 0; base < nfr; base += 64) {
            const int f = base + lane;
            paint((uint32_t)a.flist[(size_t)e * a.fcap + (f < nfr ? f : 0)], f < nfr, -1, 1u, 1u);
        }
    } else {
        const int fr0 = nw ? HDR_FRUIT0_N : HDR_FRUIT0_S;
        paint(hv & 0xFFFFu, lane >= fr0 && lane < fr0 + a.nf, -1, 1u, 1u);
    }
    wave_sync();

    // ---- per snake: its body cells (duplicates and piece 0 included), then piece 0 as the head
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= ns) continue;
        const uint32_t wA = rdlane(hv, SN_A(s));
        const int len = (int)(wA >> 16);
        if (len == 0 || (nw && !((flags >> s) & 1u))) continue;  // an empty body, a dead new_world snake: nothing
        const int hp0 = (int)((rdlane(hv, SN_C(s)) >> SN_C_HP0_SHIFT) & 63u);
        const int n0 = len < 64 ? len : 64;
        paint(ring[s], ((lane - hp0) & 63) < n0, s, 2u, 4u);
        if (len > 64) {  // pieces >= 64: the overflow ring, piece i at (ohp + i - 64) % cap
            const int ohp = (int)(wA & 0xFFFFu);
            const int n = len < 64 + a.cap ? len : 64 + a.cap;
            for (int base = 64; base < n; base += 64) {
                const int i = base + lane;
                int idx = ohp + i - 64;
                idx = idx >= a.cap ? idx - a.cap : idx;
                idx = idx >= a.cap ? a.cap - 1 : idx;  // (a well-formed record never gets here)
                idx = idx < 0 ? 0 : idx;
                paint((uint32_t)a.ovf[((size_t)e * ns + s) * a.cap + idx], i < n, s, 2u, 4u);
            }
        }
        wave_sync();
        paint(rdlane(ring[s], hp0), lane == 0, s, 3u, 5u);
        wave_sync();
    }

    // ---- copy-out: byte o of the env's block is img[o]; img + lead and out + lead are both 4-byte aligned
    // (msnake_create refuses dim < 2, so total >= 4 > lead; the clamp keeps the stores inside the block whatever total is)
    int lead = (4 - phase) & 3;              // bytes in front of the first aligned dword
    lead = lead < total ? lead : total;
    const int ndw = (total - lead) >> 2;
    const int tail0 = lead + 4 * ndw;        // [tail0, total): behind the last aligned dword
    if (lane < lead) out[lane] = img[lane];
    if (lane >= 32 && tail0 + (lane - 32) < total) out[tail0 + (lane - 32)] = img[tail0 + (lane - 32)];
    const uint32_t* src32 = img32 + ((phase + lead) >> 2);
    uint32_t* out32 = reinterpret_cast<uint32_t*>(out + lead);
    for (int j = lane; j < ndw; j += 64) out32[j] = src32[j];
}

hipError_t launch_cells(const StepParams& p, int rules, uint32_t view_mask, uint8_t* cells, int32_t* snakes, hipStream_t stream) {
    uint32_t views4 = 0u;
    int nplanes = 0;
    for (int v = 0; v < MSNAKE_MAX_SNAKES; ++v)
        if ((view_mask >> v) & 1u) views4 |= (uint32_t)v << (4 * nplanes++);
    const int slice_words = nplanes ? (nplanes * p.dim * p.dim + 3 + 3) / 4 : 0;
    const CellsArgs a{p.hdr, p.body0, p.ring, p.flist, cells, snakes, p.nenv, p.dim, p.n_snakes, p.n_fruits, p.rest.cap,
                      p.fcap, rules, nplanes, views4, slice_words};
    const size_t lds = (size_t)CELLS_WAVES * slice_words * 4;  // <= 4 x 15 384 bytes
    const dim3 grid((unsigned)((p.nenv + CELLS_WAVES - 1) / CELLS_WAVES)), block(CELLS_WAVES * 64);
    return launch_by_flags<2>((nplanes ? 2 : 0) | (snakes ? 1 : 0), [&](auto planes, auto table) {
        hipLaunchKernelGGL((msnake_cells_kernel<planes.value, table.value>), grid, block, lds, stream, a);
    });
}

}  // namespace msnake
