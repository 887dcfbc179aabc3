// msnake_scripted.inc -- scripted opponents and safe-move masks computed from the env state in HBM
// (msnake_scripted_actions).  Included first by msnake_opponents.hip: it uses msnake_device.h's wave helpers, and the
// files behind it use its wave_reduce.  Off the step path: nothing here is referenced by msnake_step_kernel.
//
// One wavefront per env, like everywhere else.  The wave only READS the handle's state:
//   * the 256-byte record, lane l <-> word l (one coalesced load); per-snake fields come out by v_readlane;
//   * every snake's 64-slot body ring, lane l <-> slot l (one 128-byte load per snake, issued with the record);
//   * the <= 16 candidate cells (4 snakes x 4 moves) are wave-uniform; every lane compares the body cell it
//     holds against all of them and keeps a 16-bit hit mask, bodies over 64 cells stride their overflow ring in
//     whole waves; one OR reduction over the wave (DPP) turns the hit masks into the "blocked" bits;
//   * fruits are lane-distributed too (record words for snake_env / new_world, the complete list `flist` for
//     adversarial, 64 entries per pass).  safe_greedy's choice -- the first move, in the order 1, 2, 3, 4, with
//     the strictly smallest distance to any fruit -- is the minimum over all (fruit, open move) pairs of the key
//     distance << 3 | move, so each snake needs ONE min reduction over the wave;
//   * lane s stores snake s's action word and mask byte.
// No LDS, no barrier, no atomics, no random numbers.
namespace msnake {

struct ScriptedArgs {
    const uint32_t* hdr; const uint16_t* body0; const uint16_t* ovf; const uint16_t* flist;
    int32_t* actions; uint8_t* safe;
    int32_t nenv, dim, ns, nf, cap, fcap, rules, stride;
    uint32_t mask;
};

// v_<op> dpp steps of a wave reduction: rows of 16 (row_shr 1, 2, 4, 8), then row_bcast:15 into rows 1, 3 and
// row_bcast:31 into rows 2, 3; a lane without a source combines with itself (the operations are idempotent).
// The result is in lane 63.
template <typename Op>
__device__ __forceinline__ uint32_t wave_reduce(uint32_t x, Op op) {
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x111, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x112, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x114, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x118, 0xF, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x142, 0xA, 0xF, false));
    x = op(x, (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x143, 0xC, 0xF, false));
    return rdlane(x, 63);
}

// hamiltonian_table(dim)[x][y] in closed form: column 0 is the return lane, the rows snake back and forth over
// columns 1..dim-1 (dim even)
__device__ __forceinline__ uint32_t hamiltonian_move(int x, int y, int dim) {
    if (x == 0) return y > 0 ? 4u : 1u;
    if ((y & 1) == 0) return x < dim - 1 ? 1u : 2u;
    if (y == dim - 1) return 3u;
    return x > 1 ? 3u : 2u;
}

constexpr uint32_t SCRIPTED_NO_CELL = 0xFFFFFFFFu;  // no 16-bit cell equals it

template <int POLICY, bool SAFE>
__global__ __launch_bounds__(256) void msnake_scripted_kernel(ScriptedArgs a) {
    constexpr bool GREEDY = POLICY == MSNAKE_POLICY_SAFE_GREEDY;
    constexpr bool BODIES = SAFE || GREEDY;  // the hamiltonian cycle alone looks at no body and no fruit
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.nenv) return;
    const int ns = a.ns, dim = a.dim;
    const uint32_t hv = a.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];
    uint32_t ring[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        ring[s] = s < ns ? (uint32_t)a.body0[((size_t)e * ns + s) * 64 + lane] : 0u;

    // per snake (wave-uniform): length, head coordinates, which moves stay on the board
    int len[MSNAKE_MAX_SNAKES], hx[MSNAKE_MAX_SNAKES], hy[MSNAKE_MAX_SNAKES];
    uint32_t onb[MSNAKE_MAX_SNAKES];                 // bit m: move m + 1 stays on the board
    uint32_t cand[MSNAKE_MAX_SNAKES][4];             // target cell of move m + 1, SCRIPTED_NO_CELL off the board
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        len[s] = 0; hx[s] = hy[s] = -2; onb[s] = 0u;
#pragma unroll
        for (int m = 0; m < 4; ++m) cand[s][m] = SCRIPTED_NO_CELL;
        if (s < ns) {
            len[s] = (int)(rdlane(hv, SN_A(s)) >> 16);
            const int hp0 = (int)((rdlane(hv, SN_C(s)) >> SN_C_HP0_SHIFT) & 63u);
            if (len[s] > 0) {
                const uint32_t head = rdlane(ring[s], hp0);  // piece 0 sits in ring slot hp0
                hx[s] = cell_c0(head); hy[s] = cell_c1(head);
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int tx = hx[s] + move_d0(m), ty = hy[s] + move_d1(m);
                    if (tx >= 0 && tx < dim && ty >= 0 && ty < dim) {
                        onb[s] |= 1u << m;
                        cand[s][m] = cell_pack(tx, ty);
                    }
                }
            }
        }
    }

    uint32_t open[MSNAKE_MAX_SNAKES];  // bit m: move m + 1 leads to an on-board cell that no body occupies
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) open[s] = 0u;
    if (BODIES) {
        uint32_t hit = 0u;  // bit 4 s + m: the cell this lane has seen equals cand[s][m]
        auto see = [&](uint32_t c) {
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
                for (int m = 0; m < 4; ++m) hit |= c == cand[s][m] ? 1u << (4 * s + m) : 0u;
        };
#pragma unroll
        for (int t = 0; t < MSNAKE_MAX_SNAKES; ++t) {
            if (t >= ns) continue;
            const int hp0 = (int)((rdlane(hv, SN_C(t)) >> SN_C_HP0_SHIFT) & 63u);
            const int n0 = len[t] < 64 ? len[t] : 64;
            see(((lane - hp0) & 63) < n0 ? ring[t] : 0xFFFFFFFEu);
            if (len[t] > 64) {  // pieces >= 64: the overflow ring, piece i at (ohp + i - 64) % cap
                const int ohp = (int)(rdlane(hv, SN_A(t)) & 0xFFFFu);
                const int n = len[t] < 64 + a.cap ? len[t] : 64 + a.cap;
                for (int base = 64; base < n; base += 64) {
                    const int i = base + lane;
                    int idx = ohp + i - 64;
                    idx = idx >= a.cap ? idx - a.cap : idx;
                    idx = idx >= a.cap ? a.cap - 1 : idx;  // (a well-formed record never gets here)
                    see(i < n ? (uint32_t)a.ovf[((size_t)e * ns + t) * a.cap + idx] : 0xFFFFFFFEu);
                }
            }
        }
        const uint32_t blocked = wave_reduce(hit, [](uint32_t x, uint32_t y) { return x | y; });
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) open[s] = onb[s] & ~(blocked >> (4 * s)) & 15u;
    }

    uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) act[s] = 0u;
    if (POLICY == MSNAKE_POLICY_HAMILTONIAN) {
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            if (len[s] > 0 && hx[s] >= 0 && hx[s] < dim && hy[s] >= 0 && hy[s] < dim) act[s] = hamiltonian_move(hx[s], hy[s], dim);
    }
    if (GREEDY) {
        const bool adv = a.rules == MSNAKE_RULES_ADVERSARIAL;
        const int fr0 = a.rules == MSNAKE_RULES_NEW_WORLD ? HDR_FRUIT0_N : HDR_FRUIT0_S;
        int nfr = adv ? (int)rdlane(hv, HDR_NLIST) : a.nf;
        if (adv && nfr > a.fcap) nfr = a.fcap;
        uint32_t key[MSNAKE_MAX_SNAKES];  // min over this lane's fruits and the open moves of distance << 3 | move
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) key[s] = 0xFFFFFFFFu;
        auto fruit = [&](uint32_t c, bool valid) {
            const int fx = cell_c0(c), fy = cell_c1(c);
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int tx = hx[s] + move_d0(m), ty = hy[s] + move_d1(m);
                    const int dx = fx - tx, dy = fy - ty;
                    const uint32_t k = ((uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) << 3) | (uint32_t)(m + 1);
                    if (valid && ((open[s] >> m) & 1u) && k < key[s]) key[s] = k;
                }
        };
        if (adv) {
            for (int base = 0; base < nfr; base += 64) {
                const int f = base + lane;
                const int fi = f < nfr ? f : 0;
                fruit((uint32_t)a.flist[(size_t)e * a.fcap + fi], f < nfr);
            }
        } else {
            fruit(hv & 0xFFFFu, lane >= fr0 && lane < fr0 + nfr);
        }
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns || open[s] == 0u) continue;
            if (nfr <= 0) {  // every distance is 0: the first open move
                act[s] = (uint32_t)__builtin_ctz(open[s]) + 1u;
            } else {
                act[s] = wave_reduce(key[s], [](uint32_t x, uint32_t y) { return x < y ? x : y; }) & 7u;
            }
        }
    }

    // lane s owns snake s's outputs
    if (lane < ns) {
        const uint32_t my_act = lane == 0 ? act[0] : lane == 1 ? act[1] : lane == 2 ? act[2] : act[3];
        const uint32_t my_open = lane == 0 ? open[0] : lane == 1 ? open[1] : lane == 2 ? open[2] : open[3];
        if (POLICY != MSNAKE_POLICY_NONE && ((a.mask >> lane) & 1u)) a.actions[(size_t)e * a.stride + lane] = (int32_t)my_act;
        if (SAFE) a.safe[(size_t)e * ns + lane] = (uint8_t)(my_open << 1);
    }
}

hipError_t launch_scripted(const StepParams& p, int rules, int policy, uint32_t snake_mask, int32_t* actions, int32_t action_stride,
                           uint8_t* safe, hipStream_t stream) {
    const ScriptedArgs a{p.hdr, p.body0, p.ring, p.flist, actions, safe, p.nenv, p.dim, p.n_snakes, p.n_fruits, p.rest.cap,
                         p.fcap, rules, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + 3) / 4)), block(256);
#define MSNAKE_SCRIPTED(P, S) hipLaunchKernelGGL((msnake_scripted_kernel<P, S>), grid, block, 0, stream, a)
    if (policy == MSNAKE_POLICY_SAFE_GREEDY) {
        if (safe) MSNAKE_SCRIPTED(MSNAKE_POLICY_SAFE_GREEDY, true); else MSNAKE_SCRIPTED(MSNAKE_POLICY_SAFE_GREEDY, false);
    } else if (policy == MSNAKE_POLICY_HAMILTONIAN) {
        if (safe) MSNAKE_SCRIPTED(MSNAKE_POLICY_HAMILTONIAN, true); else MSNAKE_SCRIPTED(MSNAKE_POLICY_HAMILTONIAN, false);
    } else if (policy == MSNAKE_POLICY_NONE && safe) {
        MSNAKE_SCRIPTED(MSNAKE_POLICY_NONE, true);
    } else {
        return hipErrorInvalidValue;
    }
#undef MSNAKE_SCRIPTED
    return hipGetLastError();
}

}  // namespace msnake
