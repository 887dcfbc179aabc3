// msnake_generate.inc -- random legal positions in canonical words, built on the device (msnake_generate_states).  Included
// by msnake_views.hip behind msnake_state.inc, whose row contract (count always, no word of a row that does not fit) it
// follows; it uses msnake_device.h's wave helpers and nothing else.  Off the step path, snake_env and adversarial handles.
//
// One wavefront per selected env.  The handle is only READ: one coalesced load of the env's record, for the draw counter
// and word 3.  It does not go through EnvReader -- one more caller of that reader's helpers changes the instructions of
// every sibling kernel in the unit (DESIGN.md, sections 22 and 26).
//   * Occupancy: lane r holds row r (c1 = r) of the board as 64 bits (bit = c0), in two VGPRs; a cell is occupied by ONE
//     lane's OR.  The k-th free cell in the order c1 * dim + c0 is the respawn's selection: a prefix sum of the rows'
//     population counts finds the row, a ballot over the ranks of its set bits the column.
//   * The walk is serial: per piece, lanes 0..3 hold the four neighbours of the last piece laid (the candidates, in the
//     order of actions 1..4) and lanes 4 + 4 m + j neighbour j of candidate m; each lane fetches the row its cell lies in
//     by ds_bpermute, and ONE ballot answers all twenty "in the grid and unoccupied?" questions.  The candidate set, the
//     Warnsdorff filter and the choice are scalar bit work on that mask.
//   * Philox4x32-10 under the generator's own key is evaluated once per block of four draws; lanes 0..3 of one VGPR keep
//     the block.
//   * The pieces are staged in LDS, snake after snake (bodies are disjoint: at most dim^2 uint16 cells), because the word
//     count must be known before any word of the row leaves; then the row is written in canonical order.
// No HBM traffic between the load and the results, no atomics, no barrier, no scratch; wave-uniform control flow.
namespace msnake {

struct GenerateArgs {
    const uint32_t* hdr; const uint8_t* mask; const int32_t* len;
    int32_t* words; int32_t* count; int32_t* got;
    uint64_t env_id_base;
    uint32_t key_lo, key_hi;  // gseed
    int32_t nenv, dim, ns, nf, len_stride, stride, compact, lds_per_wave;
};

MSNAKE_HD int generate_lds_per_wave(int dim) { return (dim * dim * 2 + 15) & ~15; }
static_assert(generate_lds_per_wave(19) == 736 && generate_lds_per_wave(62) == 7696, "19x19, 62x62");

__global__ __launch_bounds__(256) void msnake_generate_kernel(GenerateArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t generate_lds[];
    const int lane = (int)(threadIdx.x & 63u);
    const int wv = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.nenv) return;
    if (a.mask && uni((uint32_t)a.mask[e]) == 0u) return;  // an unselected env: not a byte is written
    const int dim = a.dim, ns = a.ns, nf = a.nf, n2 = dim * dim;
    uint16_t* const stage = reinterpret_cast<uint16_t*>(generate_lds + (size_t)wv * (size_t)a.lds_per_wave);
    const uint32_t hv = a.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];
    const uint64_t env_id = a.env_id_base + (uint64_t)e;

    // ---- the generator's stream: draw j is word j & 3 of block j >> 2 (fewer than 2^32 draws: S + dim^2 + F at most)
    uint32_t V_blk = 0u, ndraws = 0u;
    auto randint = [&](uint32_t n) -> uint32_t {
        if ((ndraws & 3u) == 0u) {
            uint32_t c0 = ndraws >> 2, c1 = 0u, c2 = (uint32_t)env_id, c3 = (uint32_t)(env_id >> 32);
            uint32_t k0 = a.key_lo, k1 = a.key_hi;
#pragma unroll
            for (int r = 0; r < 10; ++r) {
                const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
                const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2_ = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
                c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2_;
                k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
            }
            V_blk = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3;
        }
        const uint32_t u = rdlane(V_blk, (int)uni(ndraws & 3u));
        ++ndraws;
        return (uint32_t)(((uint64_t)u * (uint64_t)n) >> 32);
    };

    // ---- occupancy: row `lane`, bit c0
    uint64_t occ = 0ull;
    const uint64_t rowmask = dim >= 64 ? ~0ull : (1ull << dim) - 1ull;
    auto occupy = [&](int x, int y) { occ |= lane == y ? 1ull << x : 0ull; };
    // the number of unoccupied cells and, if there is one, the randint-th of them in the order c1 * dim + c0 (one draw)
    auto take_free_cell = [&](int& x, int& y) -> bool {
        const uint64_t freerow = lane < dim ? ~occ & rowmask : 0ull;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(freerow);
        const uint32_t incl = wave_scan_incl(cnt);
        const uint32_t nfree = rdlane(incl, 63);
        if (nfree == 0u) return false;
        const uint32_t kth = randint(nfree);
        const int row = __builtin_ctzll(ballot(incl > kth) | (1ull << 63));
        const uint32_t in_row = kth - (rdlane(incl, (int)uni((uint32_t)row)) - rdlane(cnt, (int)uni((uint32_t)row)));
        const uint64_t fr = ((uint64_t)rdlane((uint32_t)(freerow >> 32), (int)uni((uint32_t)row)) << 32) |
                            rdlane((uint32_t)freerow, (int)uni((uint32_t)row));
        const bool is_set = ((fr >> lane) & 1ull) != 0ull;
        const uint32_t rank = (uint32_t)__builtin_popcountll(fr & ((1ull << lane) - 1ull));
        x = __builtin_ctzll(ballot(is_set && rank == in_row) | (1ull << 63));
        y = row;
        occupy(x, y);
        return true;
    };

    // ---- the twenty cells around the last piece, as offsets from it: lanes 0..3 the candidates, 4 + 4 m + j their neighbours
    const int qm = lane < 4 ? lane : ((lane - 4) >> 2) & 3, qj = (lane - 4) & 3;
    const int offx = move_d0(qm) + (lane < 4 ? 0 : move_d0(qj)), offy = move_d1(qm) + (lane < 4 ? 0 : move_d1(qj));
    const bool asks = lane < 20;

    // ---- the snakes, one after the other: head, then the body behind it
    uint32_t V_len = 0u;  // lane s: the length snake s reached
    int total = 0;        // pieces staged so far
    int32_t req = 0;
    if (lane < ns) req = a.len[(size_t)e * (size_t)a.len_stride + lane];
    req = req < 0 ? 0 : req;
    req = lane == 0 && req < 1 ? 1 : req;
    const uint32_t V_req = (uint32_t)req;
#pragma nounroll
    for (int s = 0; s < ns; ++s) {
        const int L = (int)rdlane(V_req, (int)uni((uint32_t)s));
        int len = 0, ex = 0, ey = 0;
        if (L > 0 && take_free_cell(ex, ey)) {
            if (lane == 0 && total < n2) stage[total] = (uint16_t)cell_pack(ex, ey);
            len = 1;
#pragma nounroll
            while (len < L) {
                const int x = ex + offx, y = ey + offy;
                const uint32_t rlo = (uint32_t)__builtin_amdgcn_ds_bpermute((y & 63) << 2, (int)(uint32_t)occ);
                const uint32_t rhi = (uint32_t)__builtin_amdgcn_ds_bpermute((y & 63) << 2, (int)(uint32_t)(occ >> 32));
                const uint64_t row = ((uint64_t)rhi << 32) | rlo;
                const bool is_free = asks && x >= 0 && x < dim && y >= 0 && y < dim && ((row >> (x & 63)) & 1ull) == 0ull;
                const uint32_t fm = (uint32_t)ballot(is_free);
                uint32_t cand = fm & 15u;
                if (cand == 0u) break;
                if (a.compact) {  // Warnsdorff: only the candidates with the fewest unoccupied neighbours of their own
                    uint32_t best = 5u, keep = 0u;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const uint32_t c = (uint32_t)__builtin_popcount((fm >> (4 + 4 * m)) & 15u);
                        if ((cand >> m) & 1u) {
                            keep = c < best ? 0u : keep;
                            best = c < best ? c : best;
                            keep |= c == best ? 1u << m : 0u;
                        }
                    }
                    cand = keep;
                }
                const uint32_t n = (uint32_t)__builtin_popcount(cand);
                uint32_t idx = n == 1u ? 0u : randint(n);
#pragma nounroll
                for (; idx > 0u; --idx) cand &= cand - 1u;
                const int m = __builtin_ctz(cand);
                ex += move_d0(m); ey += move_d1(m);
                occupy(ex, ey);
                if (lane == 0 && total + len < n2) stage[total + len] = (uint16_t)cell_pack(ex, ey);
                ++len;
            }
        }
        V_len = hv_writelane(V_len, (uint32_t)len, (uint32_t)s);
        total += len;
    }

    // ---- the fruits: off the bodies and off each other; (0, 0) when no cell is left
    uint32_t V_fruit = cell_pack(0, 0);  // lane f: fruit f
#pragma nounroll
    for (int f = 0; f < nf; ++f) {
        int x = 0, y = 0;
        if (take_free_cell(x, y)) V_fruit = hv_writelane(V_fruit, cell_pack(x, y), (uint32_t)f);
    }
    wave_sync();

    // ---- results: got, the count, and -- if it fits -- the row, in the order of state_pack_env
    if (a.got && lane < ns) a.got[(size_t)e * ns + lane] = (int32_t)V_len;
    uint32_t n = 8u + 2u * (uint32_t)nf;
#pragma nounroll
    for (int s = 0; s < ns; ++s) n += 6u + 2u * rdlane(V_len, (int)uni((uint32_t)s));
    if (a.count && lane == 0) a.count[e] = (int32_t)n;
    if (!a.words || n > (uint32_t)a.stride) return;
    int32_t* const out = a.words + (size_t)e * (size_t)a.stride;
    {   // words 0..7: t = 0, the env's draw counter, its word 3, ep_len = 0, ep_return = 0, F, n_snakes (finished clear)
        const int src = lane == 1 ? HDR_CTR_LO : lane == 2 ? HDR_CTR_HI : HDR_SPARE;
        const uint32_t rec = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)hv);
        const uint32_t w = lane >= 1 && lane <= 3 ? rec : lane == 6 ? (uint32_t)nf : lane == 7 ? (uint32_t)ns : 0u;
        if (lane < 8) out[lane] = (int32_t)w;
    }
    if (lane < nf) {
        out[8 + 2 * lane] = cell_c0(V_fruit);
        out[8 + 2 * lane + 1] = cell_c1(V_fruit);
    }
    size_t k = 8 + 2 * (size_t)nf;
    int off = 0;
#pragma nounroll
    for (int s = 0; s < ns; ++s) {
        const int len = (int)rdlane(V_len, (int)uni((uint32_t)s));
        if (lane == 0) {
            int v0 = 0, v1 = 0;
            if (len > 1) {
                const uint32_t h0 = stage[off], h1 = stage[off + 1];
                v0 = cell_c0(h0) - cell_c0(h1); v1 = cell_c1(h0) - cell_c1(h1);
            }
            out[k] = len; out[k + 1] = v0; out[k + 2] = v1; out[k + 3] = len > 3 ? len : 3;
            out[k + 4] = 1; out[k + 5] = 0;
        }
#pragma nounroll
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            if (i < len) {
                const uint32_t c = stage[off + i];
                out[k + 6 + 2 * (size_t)i] = cell_c0(c);
                out[k + 6 + 2 * (size_t)i + 1] = cell_c1(c);
            }
        }
        k += 6 + 2 * (size_t)len;
        off += len;
    }
}

hipError_t launch_generate(const StepParams& p, const uint8_t* mask, const int32_t* len, int32_t len_stride, bool compact,
                           uint64_t gseed, int32_t* words, int32_t stride, int32_t* count, int32_t* got, hipStream_t stream) {
    const int per_wave = generate_lds_per_wave(p.dim), waves = 4;  // 62x62: 4 x 7696 bytes of LDS per block
    const GenerateArgs a{p.hdr, mask, len, words, count, got, p.rest.env_id_base, (uint32_t)gseed, (uint32_t)(gseed >> 32),
                         p.nenv, p.dim, p.n_snakes, p.n_fruits, len_stride, stride, compact ? 1 : 0, per_wave};
    hipLaunchKernelGGL(msnake_generate_kernel, dim3((unsigned)((p.nenv + waves - 1) / waves)), dim3((unsigned)(64 * waves)),
                       (size_t)waves * (size_t)per_wave, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
