// msnake_playout.inc -- scripted playouts of every env in ONE launch (msnake_playout): up to MSNAKE_PLAYOUT_MAX_STEPS steps
// of [policy of every snake -> step] per env, the env held in LDS from the first step to the last.  Included last by
// msnake_opponents.hip: it uses msnake_scripted.inc's wave_reduce and hamiltonian_move, msnake_fates.inc's fate_cell and
// msnake_explore.inc's lane_from, explore_draws and explore_pick (msnake_playout_explore: epsilon-random moves per step).
// Off the step path, snake_env rules only.
//
// One wavefront per env; the wave only READS the handle's state, once, in EnvReader's layout and bounds.
//   * Bodies: per snake a ring of `cap` uint16 cells in LDS, piece i at (hd + i) % cap.  An insert steps hd back by one and
//     ONE lane stores the new head; a pop lowers len.  len <= cap - 1 always (the capacity rule of msnake_set_state).
//   * Per-snake fields live in VGPRs, lane s <-> snake s (len, hd, grow_to, velocity code, head cell, and the sums the
//     call reports); the fruits likewise, lane f <-> fruit f.  The snakes move one after the other in a real loop: the
//     fields come out by v_readlane and go back by v_writelane with a run-time lane, so nothing is indexed in scratch.
//   * Policies read the LDS bodies the way msnake_scripted_kernel reads its rings: lanes stride the pieces against the
//     wave-uniform candidate cells (16 for safe_greedy, 20 for wary_greedy), one OR reduction per question.  The fruits
//     are at most four wave-uniform cells, so the choice among the candidates runs in the candidate lanes: safe_greedy's
//     min over (move, fruit) is one row reduction (lane 16 s + 4 m + f), wary_greedy's verdicts sit in lanes 5 s + a as in
//     msnake_fates_kernel.
//   * A respawn (safe_choose_cell) builds the occupancy bitboard from the bodies as they stand at that moment -- the
//     earlier snakes moved, the later ones not --: 64 rows of 64 bits in LDS, row = c1, bit = c0, set by ds_or; lane r
//     then holds row r, a prefix sum of the population counts finds the row of the k-th free cell and a ballot its bit.
//     One Philox4x32-10 draw (this file's own copy) unless no cell is free.
//   * The collision test walks every post-move body once against the heads; then the dead are cleared, the per-snake sums
//     are brought up to date in lanes 0..S-1, and t, ep_len, ep_return and `finished` follow msnake_step.
//   * The end words leave from LDS in the order of the canonical layout: a writer of its own, next to state_pack_env.
// No HBM traffic between the load and the results, no HBM atomics, no barrier, no scratch; wave-uniform control flow.
namespace msnake {

struct PlayoutArgs {
    StateView v;
    const int32_t* first; int32_t first_stride; uint32_t first_mask;
    uint32_t pol;        // policy of snake s in bits 4 s .. 4 s + 3
    int32_t n_steps, max_steps;
    uint32_t seed_lo, seed_hi; uint64_t env_id_base;
    int32_t* steps; uint8_t* end; float* ret; int32_t* info; int32_t* words; int32_t words_stride; int32_t* count;
    int32_t lds_per_wave;
    int32_t which;       // EXPLORE_* (msnake_explore.inc): which blocks a step runs
    uint32_t eps[MSNAKE_MAX_SNAKES];  // eps_q16 of snake s (msnake_playout_explore; all 0 for msnake_playout)
    uint32_t xseed_lo, xseed_hi;      // the exploration stream's seed, formed on the host
};

constexpr int PLAYOUT_OCC_BYTES = 512;  // 64 rows of 64 bits
MSNAKE_HD int playout_lds_per_wave(int ns, int cap) { return ns * cap * 2 + PLAYOUT_OCC_BYTES; }
static_assert(playout_lds_per_wave(3, 384) == 2816 && playout_lds_per_wave(3, 3904) == 23936, "19x19x3, 62x62x3");

// word (draw & 3) of Philox4x32-10(counter = {draw >> 2, global env id}, key = seed): tests/golden/philox_kat.json
__device__ __forceinline__ uint32_t playout_philox(uint32_t seed_lo, uint32_t seed_hi, uint64_t env_id, uint64_t draw) {
    const uint64_t blk = draw >> 2;
    uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = (uint32_t)env_id, c3 = (uint32_t)(env_id >> 32);
    uint32_t k0 = seed_lo, k1 = seed_hi;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint32_t w = (uint32_t)draw & 3u;
    return w == 0 ? c0 : w == 1 ? c1 : w == 2 ? c2 : c3;
}

__device__ __forceinline__ uint32_t rdl(uint32_t v, int l) { return rdlane(v, (int)uni((uint32_t)l)); }  // run-time lane

// ONE kernel, not one per set of policies: a.which (bit 0: the open moves and safe_greedy, bit 1: the verdicts and
// wary_greedy, bit 2: some snake explores) is tested per step, wave-uniformly.  As a template over the first two bits the
// kernel was the same code per instantiation, but with more than one instantiation in the unit every sibling kernel that
// reads through EnvReader came out with other instructions (tools/isa_diff.py: 87 of 93 differed); with one, every
// sibling is as it was (DESIGN.md, sections 26 and 28).
__global__ __launch_bounds__(256) void msnake_playout_kernel(PlayoutArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t playout_lds[];
    const int wave_lane = (int)(threadIdx.x & 63u), lane = wave_lane;
    const int wv = (int)uni(threadIdx.x >> 6);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;
    const int ns = a.v.ns, nf = a.v.nf < MSNAKE_MAX_SNAKES ? a.v.nf : MSNAKE_MAX_SNAKES, dim = a.v.dim, cap = a.v.cap;
    uint16_t* const body = reinterpret_cast<uint16_t*>(playout_lds + (size_t)wv * (size_t)a.lds_per_wave);
    uint32_t* const occ = reinterpret_cast<uint32_t*>(body + (size_t)ns * cap);
    // What only the end of the launch (the results) and the respawns (the Philox key) need waits in lanes of two VGPRs, not
    // in scalar registers held across the whole loop: lane OUT_* of V_out holds an output pointer, lanes REC_KEY.. of V_rec
    // the seed and the global env id.
    enum { OUT_STEPS = 0, OUT_END = 1, OUT_RET = 2, OUT_INFO = 3, OUT_WORDS = 4, OUT_COUNT = 5, OUT_STRIDE = 6 };
    uint64_t V_out;
    {
        const void* const p = lane == OUT_STEPS ? (const void*)a.steps : lane == OUT_END ? (const void*)a.end : lane == OUT_RET ? (const void*)a.ret :
                              lane == OUT_INFO ? (const void*)a.info : lane == OUT_WORDS ? (const void*)a.words : lane == OUT_COUNT ? (const void*)a.count : nullptr;
        V_out = lane == OUT_STRIDE ? (uint64_t)(uint32_t)a.words_stride : (uint64_t)(uintptr_t)p;
    }
    auto out_ptr = [&](int which) -> uint64_t {
        return ((uint64_t)rdlane((uint32_t)(V_out >> 32), which) << 32) | rdlane((uint32_t)V_out, which);
    };

    // ---- load: the record's fields into lanes 0..3, every body into its LDS ring (head at index 0)
    uint32_t V_len, V_hd = 0u, V_grow, V_vel, V_head = 0u, V_fruit;
    uint32_t V_rec;  // lane REC_*: the env's scalars (kept in one VGPR: as scalar registers they are what spills)
    enum { REC_T = 0, REC_CTR_LO = 1, REC_CTR_HI = 2, REC_FLAGS = 3, REC_EP_LEN = 4, REC_EP_RET = 5, REC_SPARE = 6,
           REC_SEED_LO = 8, REC_SEED_HI = 9, REC_ENV_LO = 10, REC_ENV_HI = 11, REC_N_STEPS = 12, REC_MAX_STEPS = 13,
           REC_XSEED_LO = 14, REC_XSEED_HI = 15, REC_EPS0 = 16 };  // REC_EPS0 + s: eps_q16 of snake s
    {
        // The layout and the bounds are EnvReader's (msnake_envread.inc), spelled out here: the compiler specialises that
        // reader's helpers by what all their callers in the unit pass, so one more caller changes the instructions of every
        // sibling kernel (DESIGN.md, sections 22 and 26), and those are to stay as they were measured.
        const uint32_t hv = a.v.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];
        V_len = lane < ns ? hv >> 16 : 0u;
        V_len = V_len > (uint32_t)(cap - 1) ? (uint32_t)(cap - 1) : V_len;  // (a well-formed record never gets here)
        V_grow = lane_from(hv, (lane & 3) + SN_B(0));
        V_vel = (lane_from(hv, (lane & 3) + SN_C(0)) >> 16) & 0xFFu;
        V_fruit = lane_from(hv, (lane & 3) + HDR_FRUIT0_S) & 0xFFFFu;
        V_fruit = lane < nf ? V_fruit : 0xFFFFFFFFu;
        {
            const int src = lane == REC_T ? HDR_T : lane == REC_CTR_LO ? HDR_CTR_LO : lane == REC_CTR_HI ? HDR_CTR_HI : lane == REC_FLAGS ? HDR_FLAGS :
                            lane == REC_EP_LEN ? HDR_EP_LEN : lane == REC_EP_RET ? HDR_EP_RETURN : HDR_SPARE;
            V_rec = lane_from(hv, src);
            const uint64_t env_id = a.env_id_base + (uint64_t)e;
            V_rec = lane == REC_SEED_LO ? a.seed_lo : lane == REC_SEED_HI ? a.seed_hi : lane == REC_ENV_LO ? (uint32_t)env_id :
                    lane == REC_ENV_HI ? (uint32_t)(env_id >> 32) : lane == REC_N_STEPS ? (uint32_t)a.n_steps :
                    lane == REC_MAX_STEPS ? (uint32_t)a.max_steps : V_rec;
            if (a.which & EXPLORE_DRAWS)
                V_rec = lane == REC_XSEED_LO ? a.xseed_lo : lane == REC_XSEED_HI ? a.xseed_hi : lane == REC_EPS0 ? a.eps[0] :
                        lane == REC_EPS0 + 1 ? a.eps[1] : lane == REC_EPS0 + 2 ? a.eps[2] : lane == REC_EPS0 + 3 ? a.eps[3] : V_rec;
        }
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns) continue;
            const uint32_t ring = (uint32_t)a.v.body0[((size_t)e * ns + s) * 64 + lane];  // ring slot `lane`
            const uint32_t wa = rdlane(hv, SN_A(s));
            const int hp0 = (int)((rdlane(hv, SN_C(s)) >> SN_C_HP0_SHIFT) & 63u), ohp = (int)(wa & 0xFFFFu);
            int len = (int)(wa >> 16);
            len = len > cap - 1 ? cap - 1 : len;
            V_head = hv_writelane_unrolled(V_head, len > 0 ? rdlane(ring, hp0) : 0u, (uint32_t)s);
            const int i0 = (lane - hp0) & 63;                      // piece i < 64 sits in ring slot (hp0 + i) & 63
            if (i0 < len) body[(size_t)s * cap + i0] = (uint16_t)ring;
#pragma nounroll
            for (int base = 64; base < len; base += 64) {          // piece i >= 64 at ovf[(ohp + i - 64) % cap]
                const int i = base + lane;
                int idx = ohp + i - 64;
                idx = idx >= cap ? idx - cap : idx;
                idx = idx >= cap || idx < 0 ? cap - 1 : idx;       // (a well-formed record never gets here)
                if (i < len) body[(size_t)s * cap + i] = a.v.ovf[((size_t)e * ns + s) * cap + idx];
            }
        }
    }
    wave_sync();

    // piece i of snake s (i < len <= cap - 1, hd < cap)
    auto piece_at = [&](int s, int hd, int i) -> uint32_t {
        int idx = hd + i;
        idx = idx >= cap ? idx - cap : idx;
        return (uint32_t)body[(size_t)s * cap + idx];
    };
    // fn(s, i, cell, valid) for every piece of every snake, the lanes striding each body
    auto for_each_body = [&](auto fn) {
#pragma nounroll
        for (int s = 0; s < ns; ++s) {
            const int len = (int)rdl(V_len, s), hd = (int)rdl(V_hd, s);
#pragma nounroll
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                const bool valid = i < len;
                fn(s, i, piece_at(s, hd, valid ? i : 0), valid);
            }
        }
    };

    // what the call reports, lane s <-> snake s
    float V_ret = 0.0f;
    uint32_t V_ate = 0u, V_alive = 0u, V_death = 0u, V_first = 0u;
    uint32_t steps = 0u, endc = MSNAKE_PLAYOUT_HORIZON;
    const uint32_t pol_of_lane = lane < ns ? (a.pol >> (4 * (lane & 7))) & 15u : 0u;
    // step 1's forced actions, read once: lane s holds first_dev[e][s] and whether it counts
    uint32_t V_force = 0u, V_forced = 0u;
    if (lane < ns && ((a.first_mask >> lane) & 1u)) {
        V_force = (uint32_t)a.first[(size_t)e * a.first_stride + lane];
        V_forced = 1u;
    }
    // a lane predicate as a number in a VGPR (as a lane mask it takes a pair of scalar registers for as long as it lives)
    auto as_vgpr = [](bool b) -> uint32_t { uint32_t x = b ? 1u : 0u; asm volatile("" : "+v"(x)); return x; };

    if (rdlane(V_rec, REC_FLAGS) & HDR_FLAG_FINISHED) {
        endc = MSNAKE_PLAYOUT_FINISHED;
    } else {
#pragma nounroll
        for (int k = 1; k <= (int)rdlane(V_rec, REC_N_STEPS); ++k) {
            // ================================================================ the policies, on the state as it stands
            // (the lane index is made opaque once per step: every lane mask the step needs is otherwise formed in front of
            //  the loop and held in a pair of scalar registers across it, which is what spills)
            int lane_of_step = wave_lane;
            asm volatile("" : "+v"(lane_of_step));
            const int lane = lane_of_step;
            uint32_t V_act = 0u, my_pol = pol_of_lane;
            asm volatile("" : "+v"(my_pol));
            uint32_t V_cand = 0u;  // lane s: the candidate set of snake s, bit m: move m + 1 (read only when some snake explores)
            if (my_pol == MSNAKE_POLICY_HAMILTONIAN) {
                const int hx = cell_c0(V_head), hy = cell_c1(V_head);
                if (V_len > 0u && hx >= 0 && hx < dim && hy >= 0 && hy < dim) V_act = hamiltonian_move(hx, hy, dim);
            }
            if (a.which & EXPLORE_NEEDS_OPEN) {
                // ---- safe_greedy (msnake_scripted_kernel): lane q = 4 s + m holds the target of move m + 1 of snake s
                const int qs = (lane >> 2) & 3, qm = lane & 3;
                const uint32_t qhead = lane_from(V_head, qs), qlen = lane_from(V_len, qs);
                const int tx = cell_c0(qhead) + move_d0(qm), ty = cell_c1(qhead) + move_d1(qm);
                const bool onb = lane < 16 && qs < ns && qlen > 0u && tx >= 0 && tx < dim && ty >= 0 && ty < dim;
                const uint32_t candv = onb ? cell_pack(tx, ty) : SCRIPTED_NO_CELL;
                // (the 16 candidates are read out of their lanes per pass, not kept: 16 scalar registers held across the walk
                //  are what spills; the empty asm keeps the reads inside the loop)
                uint32_t hit = 0u, cv = candv;
                for_each_body([&](int, int, uint32_t c, bool valid) {
                    const uint32_t cc = valid ? c : 0xFFFFFFFEu;
                    asm volatile("" : "+v"(cv));
#pragma unroll
                    for (int q = 0; q < 16; ++q) hit |= cc == rdlane(cv, q) ? 1u << q : 0u;
                });
                const uint32_t blocked = wave_reduce(hit, [](uint32_t x, uint32_t y) { return x | y; });
                const uint32_t open = (uint32_t)ballot(onb) & ~blocked & 0xFFFFu;  // bit 4 s + m
                // lane 16 s + 4 m + f: distance << 3 | move of (open move m + 1, fruit f); the row minimum is the choice
                const int gs = lane >> 4, gm = (lane >> 2) & 3, gf = lane & 3;
                const uint32_t ghead = lane_from(V_head, gs), gfruit = lane_from(V_fruit, gf);
                const int dx = cell_c0(gfruit) - (cell_c0(ghead) + move_d0(gm)), dy = cell_c1(gfruit) - (cell_c1(ghead) + move_d1(gm));
                uint32_t key = ((uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) << 3) | (uint32_t)(gm + 1);
                key = gf < nf && ((open >> (lane >> 2)) & 1u) ? key : 0xFFFFFFFFu;
                auto mn = [](uint32_t x, uint32_t y) { return x < y ? x : y; };
                key = mn(key, (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x111, 0xF, 0xF, false));
                key = mn(key, (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x112, 0xF, 0xF, false));
                key = mn(key, (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x114, 0xF, 0xF, false));
                key = mn(key, (uint32_t)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x118, 0xF, 0xF, false));
                const uint32_t mine = lane_from(key, 16 * (lane & 3) + 15);  // lane s <- the minimum of row s
                if (my_pol == MSNAKE_POLICY_SAFE_GREEDY) V_act = mine == 0xFFFFFFFFu ? 0u : mine & 7u;
                if (a.which & EXPLORE_DRAWS) V_cand = (open >> (4 * (lane & 3))) & 15u;
            }
            if (a.which & EXPLORE_NEEDS_WARY) {
                // ---- wary_greedy (msnake_fates_kernel): lane 5 s + a holds the target of action a of snake s
                const int my_s = (lane >= 5) + (lane >= 10) + (lane >= 15), my_a = lane - 5 * my_s;
                const int my_len = (int)lane_from(V_len, my_s), my_vel = (int)lane_from(V_vel, my_s);
                const uint32_t my_grow = lane_from(V_grow, my_s), my_head = lane_from(V_head, my_s);
                const bool live_p = lane < 5 * ns && my_len > 0;
                const uint32_t live = as_vgpr(live_p);
                const int reverse = my_vel == 0 ? 0 : ((my_vel - 1) ^ 2) + 1;
                const int dir = (my_a == 0 || my_a == reverse) ? my_vel : my_a;
                const uint32_t moving = as_vgpr(dir != 0);
                const int tx = cell_c0(my_head) + vel_v0(dir), ty = cell_c1(my_head) + vel_v1(dir);
                const uint32_t T = live_p ? fate_cell(tx, ty) : FATE_NO_CELL;
                uint32_t own = 0u, other = 0u, Tv = T;  // (the 20 targets: read per pass, as above)
                for_each_body([&](int s, int i, uint32_t c, bool valid) {
                    const uint32_t cc = c + 0x0101u;
                    uint32_t eq = 0u;
                    asm volatile("" : "+v"(Tv));
#pragma unroll
                    for (int q = 0; q < 20; ++q) eq |= cc == rdlane(Tv, q) ? 1u << q : 0u;
                    eq = valid && i < (int)rdl(V_len, s) - 1 ? eq : 0u;  // a piece before the last one
                    uint32_t o = eq & (31u << (5 * s));
                    if (i == 0 && rdl(V_vel, s) == 0u) o &= ~(1u << (5 * s));  // a standing snake's target is its own head
                    own |= o;
                    other |= eq & ~(31u << (5 * s));
                });
                own = wave_reduce(own, [](uint32_t x, uint32_t y) { return x | y; });
                other = wave_reduce(other, [](uint32_t x, uint32_t y) { return x | y; });
                uint32_t n_at = 0u, dist = FATE_FAR;
#pragma unroll
                for (int f = 0; f < MSNAKE_MAX_SNAKES; ++f) {
                    if (f >= nf) continue;
                    const uint32_t fc = rdlane(V_fruit, f);
                    n_at += T == fc + 0x0101u ? 1u : 0u;
                    const int dx = cell_c0(fc) - tx, dy = cell_c1(fc) - ty;
                    const uint32_t d = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
                    dist = d < dist ? d : dist;
                }
                const uint32_t pop = as_vgpr(moving != 0u && my_grow <= (uint32_t)my_len && 2u * n_at <= (uint32_t)my_len - my_grow);
                uint32_t self = (own >> (lane & 31)) & 1u, hitbody = (other >> (lane & 31)) & 1u;
                uint32_t by = 0u;
#pragma unroll
                for (int j = 0; j < MSNAKE_MAX_SNAKES; ++j) {
                    if (j >= ns) continue;
                    const uint32_t len_j = rdlane(V_len, j), vel_j = rdlane(V_vel, j);
                    if (len_j == 0u) continue;
                    const uint32_t tail = piece_at(j, (int)rdlane(V_hd, j), (int)len_j - 1) + 0x0101u;
                    const bool at_tail = T == tail, is_mine = my_s == j;
                    const bool grows = len_j < rdlane(V_grow, j);
                    self |= is_mine && at_tail && pop == 0u && !(moving == 0u && len_j == 1u) ? 1u : 0u;
                    hitbody |= !is_mine && at_tail && grows ? 1u : 0u;
                    by |= !is_mine && at_tail && !grows ? 16u << j : 0u;
#pragma unroll
                    for (int b = 0; b < 5; ++b) {
                        if (b == 0 && vel_j == 0u) continue;
                        by |= !is_mine && T == rdlane(T, 5 * j + b) ? 1u << j : 0u;
                    }
                }
                const uint32_t wall = tx < 0 || tx >= dim || ty < 0 || ty >= dim ? 1u : 0u;
                const uint32_t certain = wall | self | hitbody;
                const uint64_t ok0 = ballot(live != 0u && certain == 0u), ok1 = ballot(live != 0u && (certain | by) == 0u);
                uint32_t candbits = 0u;
#pragma unroll
                for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                    const uint32_t sure = (uint32_t)(ok1 >> (5 * s)) & 0x1Eu, maybe = (uint32_t)(ok0 >> (5 * s)) & 0x1Eu;
                    candbits |= (sure != 0u ? sure : maybe) << (5 * s);
                }
                const uint32_t wkey = lane < 20 && ((candbits >> (lane & 31)) & 1u) ? (dist << 3) | (uint32_t)my_a : 0xFFFFFFFFu;
                uint32_t wact = 0u;
#pragma unroll
                for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                    uint32_t m = 0xFFFFFFFFu;
#pragma unroll
                    for (int b = 1; b < 5; ++b) { const uint32_t x = rdlane(wkey, 5 * s + b); m = x < m ? x : m; }
                    wact = lane == s ? (m == 0xFFFFFFFFu ? 0u : m & 7u) : wact;
                }
                if (my_pol == MSNAKE_POLICY_WARY_GREEDY) V_act = wact;
                if ((a.which & EXPLORE_DRAWS) && my_pol == MSNAKE_POLICY_WARY_GREEDY) V_cand = (candbits >> (5 * (lane & 3) + 1)) & 15u;
            }
            if (a.which & EXPLORE_DRAWS) {
                // ---- the exploration rule (msnake_explore.inc), lane s <-> snake s: one Philox block per lane under the key
                // mix64(xseed ^ ctr), on the state's own t and ctr
                const uint64_t xseed = ((uint64_t)rdlane(V_rec, REC_XSEED_HI) << 32) | rdlane(V_rec, REC_XSEED_LO);
                const uint64_t ctr = ((uint64_t)rdlane(V_rec, REC_CTR_HI) << 32) | rdlane(V_rec, REC_CTR_LO);
                const uint64_t env_id = ((uint64_t)rdlane(V_rec, REC_ENV_HI) << 32) | rdlane(V_rec, REC_ENV_LO);
                const ExploreDraws d = explore_draws(xseed, ctr, env_id, rdlane(V_rec, REC_T), lane & 3);
                bool explored;
                const uint32_t drawn = explore_pick(V_act, V_cand, lane_from(V_rec, REC_EPS0 + (lane & 3)), d, &explored);
                V_act = lane < ns ? drawn : V_act;
            }
            if (k == 1) {
                V_act = V_forced != 0u ? V_force : V_act;
                V_first = lane < ns ? V_act : 0u;
            }

            // ================================================================ the step ([S]:97-197), one snake after the other
            const uint32_t len_before = V_len, grow_before = V_grow;
            float reward = 0.0f;
#pragma nounroll
            for (int s = 0; s < ns; ++s) {
                const uint32_t len = rdl(V_len, s);
                if (len == 0u) continue;
                const int vel = (int)rdl(V_vel, s), act = (int)rdl(V_act, s);
                const int nvel = (act >= 1 && act <= 4 && vel != ((act + 1) & 3) + 1) ? act : vel;
                if (nvel == 0) continue;
                const uint32_t head = rdl(V_head, s);
                const uint32_t nh = cell_pack(cell_c0(head) + vel_v0(nvel), cell_c1(head) + vel_v1(nvel)) & 0xFFFFu;
                uint32_t em = (uint32_t)ballot(V_fruit == nh) & 15u;  // (lanes >= nf hold no cell)
                const uint32_t neat = (uint32_t)__builtin_popcount(em);
                const uint32_t g = rdl(V_grow, s) + 2u * neat;
                uint32_t l = len;
                if (l >= g) l -= 1u;                                             // [S]:134-135
                int hd = (int)rdl(V_hd, s);
                hd = hd == 0 ? cap - 1 : hd - 1;
                if (lane == 0) body[(size_t)s * cap + hd] = (uint16_t)nh;        // insert(0, head)
                l += 1u;
                l = l > (uint32_t)(cap - 1) ? (uint32_t)(cap - 1) : l;           // the capacity rule: the oldest piece goes
                V_len = hv_writelane(V_len, l, (uint32_t)s);
                V_hd = hv_writelane(V_hd, (uint32_t)hd, (uint32_t)s);
                V_grow = hv_writelane(V_grow, g, (uint32_t)s);
                V_vel = hv_writelane(V_vel, (uint32_t)nvel, (uint32_t)s);
                V_head = hv_writelane(V_head, nh, (uint32_t)s);
                if (s == 0) reward = (float)neat;
                if (em == 0u) continue;
                // ---- safe_choose_cell ([S]:202-217) for each fruit eaten, in index order: the bodies as they stand now
                wave_sync();
                occ[2 * lane] = 0u; occ[2 * lane + 1] = 0u;
                wave_sync();
                for_each_body([&](int, int, uint32_t c, bool valid) {
                    int c0 = cell_c0(c), c1 = cell_c1(c);
                    bool in = valid;
                    if (c0 < 0 || c0 >= dim || c1 < 0 || c1 >= dim) {  // a head outside the grid: its alias c1 * dim + c0
                        const int used = c1 * dim + c0;
                        in = in && used >= 0 && used < dim * dim;
                        c1 = in ? used / dim : 0;
                        c0 = in ? used - c1 * dim : 0;
                    }
                    if (in) __hip_atomic_fetch_or(&occ[2 * c1 + (c0 >> 5)], 1u << (c0 & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                });
                wave_sync();
                const uint64_t rowmask = dim >= 64 ? ~0ull : (1ull << dim) - 1ull;
                const uint64_t freerow = lane < dim ? ~(((uint64_t)occ[2 * lane + 1] << 32) | occ[2 * lane]) & rowmask : 0ull;
                const uint32_t cnt = (uint32_t)__builtin_popcountll(freerow);
                const uint32_t incl = wave_scan_incl(cnt);
                const uint32_t nfree = rdlane(incl, 63);
#pragma nounroll
                while (em) {
                    const int f = __builtin_ctz(em);
                    em &= em - 1u;
                    uint32_t c0 = 0u, c1 = 0u;
                    if (nfree > 0u) {
                        const uint64_t ctr = ((uint64_t)rdlane(V_rec, REC_CTR_HI) << 32) | rdlane(V_rec, REC_CTR_LO);
                        const uint64_t env_id = ((uint64_t)rdlane(V_rec, REC_ENV_HI) << 32) | rdlane(V_rec, REC_ENV_LO);
                        const uint32_t u = playout_philox(rdlane(V_rec, REC_SEED_LO), rdlane(V_rec, REC_SEED_HI), env_id, ctr);
                        V_rec = hv_writelane_c<REC_CTR_LO>(V_rec, (uint32_t)(ctr + 1ull));
                        V_rec = hv_writelane_c<REC_CTR_HI>(V_rec, (uint32_t)((ctr + 1ull) >> 32));
                        const uint32_t kth = (uint32_t)(((uint64_t)u * (uint64_t)nfree) >> 32);
                        const int row = __builtin_ctzll(ballot(incl > kth));
                        const uint32_t in_row = kth - (rdl(incl, row) - rdl(cnt, row));
                        const uint64_t fr = ((uint64_t)rdl((uint32_t)(freerow >> 32), row) << 32) | rdl((uint32_t)freerow, row);
                        const bool is_set = ((fr >> lane) & 1ull) != 0ull;
                        const uint32_t rank = (uint32_t)__builtin_popcountll(fr & ((1ull << lane) - 1ull));
                        c0 = (uint32_t)__builtin_ctzll(ballot(is_set && rank == in_row) | (1ull << 63));
                        c1 = (uint32_t)row;
                    }
                    V_fruit = hv_writelane(V_fruit, cell_pack((int)c0, (int)c1), (uint32_t)f);
                }
            }
            wave_sync();

            // ================================================================ is_snake_alive, all against the same bodies
            uint32_t hit = 0u, hcv = V_len > 0u ? V_head : 0xFFFFFFFFu;  // lane s: the head of snake s, no cell for an empty body
            for_each_body([&](int j, int i, uint32_t c, bool valid) {
                const uint32_t cc = valid ? c : 0xFFFFFFFEu;
                asm volatile("" : "+v"(hcv));
#pragma unroll
                for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) hit |= cc == rdlane(hcv, s) && !(j == s && i == 0) ? 1u << s : 0u;
            });
            uint32_t hitmask = 0u;
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) hitmask |= ballot((hit >> s) & 1u) != 0ull ? 1u << s : 0u;
            {
                const int hx = cell_c0(V_head), hy = cell_c1(V_head);
                const bool dead = lane < ns && V_len > 0u && (hx < 0 || hx >= dim || hy < 0 || hy >= dim || ((hitmask >> (lane & 31)) & 1u));
                V_len = dead ? 0u : V_len;
            }
            // ---- the sums of msnake_agent_outcomes
            {
                const bool was = len_before > 0u, died = was && V_len == 0u;
                const int diff = (int)V_grow - (int)grow_before;
                const uint32_t ate = (uint32_t)(diff > 0 ? diff : 0) >> 1;
                V_ret += died ? -1.0f : (float)ate;
                V_ate += ate;
                V_alive += V_len > 0u ? 1u : 0u;
                V_death = died ? (uint32_t)k : V_death;
            }
            // ---- reward, t, done; the vec layer's episode totals (auto_reset = 0)
            const bool main_dead = rdlane(V_len, 0) == 0u;
            if (main_dead) reward = -1.0f;
            V_rec += lane == REC_T || lane == REC_EP_LEN ? 1u : 0u;
            V_rec = lane == REC_EP_RET ? __float_as_uint(__uint_as_float(V_rec) + reward) : V_rec;
            steps = (uint32_t)k;
            if (main_dead || (int32_t)rdlane(V_rec, REC_T) >= (int32_t)rdlane(V_rec, REC_MAX_STEPS)) {
                V_rec |= lane == REC_FLAGS ? HDR_FLAG_FINISHED : 0u;
                endc = main_dead ? MSNAKE_PLAYOUT_DEAD : MSNAKE_PLAYOUT_CAP;
                break;
            }
        }
    }

    // ---- results
    int32_t* const o_steps = reinterpret_cast<int32_t*>(out_ptr(OUT_STEPS));
    uint8_t* const o_end = reinterpret_cast<uint8_t*>(out_ptr(OUT_END));
    float* const o_ret = reinterpret_cast<float*>(out_ptr(OUT_RET));
    int32_t* const o_info = reinterpret_cast<int32_t*>(out_ptr(OUT_INFO));
    int32_t* const o_words = reinterpret_cast<int32_t*>(out_ptr(OUT_WORDS));
    int32_t* const o_count = reinterpret_cast<int32_t*>(out_ptr(OUT_COUNT));
    const uint32_t o_stride = rdlane((uint32_t)V_out, OUT_STRIDE);
    if (lane == 0) {
        if (o_steps) o_steps[e] = (int32_t)steps;
        if (o_end) o_end[e] = (uint8_t)endc;
    }
    if (lane < ns) {
        const size_t at = (size_t)e * ns + lane;
        if (o_ret) o_ret[at] = V_ret;
        if (o_info) {
            int32_t* row = o_info + at * 4;  // (4-byte aligned is all the caller owes)
            row[0] = (int32_t)V_ate; row[1] = (int32_t)V_alive; row[2] = (int32_t)V_death; row[3] = (int32_t)V_first;
        }
    }
    // ---- the end state in canonical words (the layout of state_pack_env), from LDS
    if (o_words || o_count) {
        uint32_t n = 8u + 2u * (uint32_t)nf;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            if (s < ns) n += 6u + 2u * rdlane(V_len, s);
        if (o_count && lane == 0) o_count[e] = (int32_t)n;
        if (o_words && n <= o_stride) {
            int32_t* out = o_words + (size_t)e * (size_t)o_stride;
            {   // words 0..7: t, ctr_lo, ctr_hi, spare_fruits, ep_len, ep_return, n_fruits, n_snakes | finished << 8
                const int src = lane == 0 ? REC_T : lane == 1 ? REC_CTR_LO : lane == 2 ? REC_CTR_HI : lane == 3 ? REC_SPARE : lane == 4 ? REC_EP_LEN : REC_EP_RET;
                const uint32_t fin = (rdlane(V_rec, REC_FLAGS) & HDR_FLAG_FINISHED) ? 0x100u : 0u;
                const uint32_t w = lane == 6 ? (uint32_t)nf : lane == 7 ? (uint32_t)ns | fin : lane_from(V_rec, src);
                if (lane < 8) out[lane] = (int32_t)w;
            }
            if (lane < nf) {
                out[8 + 2 * lane] = cell_c0(V_fruit);
                out[8 + 2 * lane + 1] = cell_c1(V_fruit);
            }
            size_t kk = 8 + 2 * (size_t)nf;
#pragma nounroll
            for (int s = 0; s < ns; ++s) {
                const int len = (int)rdl(V_len, s), hd = (int)rdl(V_hd, s), vel = (int)(rdl(V_vel, s) & 7u);
                if (lane == 0) {
                    out[kk] = len; out[kk + 1] = vel_v0(vel); out[kk + 2] = vel_v1(vel); out[kk + 3] = (int32_t)rdl(V_grow, s);
                    out[kk + 4] = 1; out[kk + 5] = 0;
                }
#pragma nounroll
                for (int base = 0; base < len; base += 64) {
                    const int i = base + lane;
                    if (i < len) {
                        const uint32_t c = piece_at(s, hd, i);
                        out[kk + 6 + 2 * (size_t)i] = cell_c0(c);
                        out[kk + 6 + 2 * (size_t)i + 1] = cell_c1(c);
                    }
                }
                kk += 6 + 2 * (size_t)len;
            }
        }
    }
}

hipError_t launch_playout(const StepParams& p, int rules, const int32_t* policies, const uint32_t* eps, uint64_t xseed,
                          int32_t n_steps, const int32_t* first,
                          int32_t first_stride, uint32_t first_mask, int32_t* steps, uint8_t* end, float* ret, int32_t* info,
                          int32_t* words, int32_t words_stride, int32_t* count, hipStream_t stream) {
    uint32_t pol = 0u;
    for (int s = 0; s < p.n_snakes; ++s) pol |= (uint32_t)policies[s] << (4 * s);
    const int which = explore_which(policies, eps, p.n_snakes);  // eps NULL: msnake_playout, nobody explores
    const int per_wave = playout_lds_per_wave(p.n_snakes, p.rest.cap);
    int waves = 65536 / per_wave;  // the block stays within 64 KiB of LDS
    waves = waves > 4 ? 4 : waves;
    if (waves < 1) return hipErrorInvalidValue;
    PlayoutArgs a{state_view(p, rules), first, first_stride, first_mask, pol, n_steps, p.rest.max_steps, p.rest.seed_lo,
                  p.rest.seed_hi, p.rest.env_id_base, steps, end, ret, info, words, words_stride, count, per_wave, which,
                  {0u, 0u, 0u, 0u}, (uint32_t)xseed, (uint32_t)(xseed >> 32)};
    for (int s = 0; s < p.n_snakes && eps != nullptr; ++s) a.eps[s] = eps[s];
    const dim3 grid((unsigned)((p.nenv + waves - 1) / waves)), block((unsigned)(64 * waves));
    const size_t lds = (size_t)waves * (size_t)per_wave;
    hipLaunchKernelGGL(msnake_playout_kernel, grid, block, lds, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
