// msnake_explore.inc -- epsilon-random moves drawn from a stream of their own: the draw and the choice that
// msnake_playout_kernel applies per step (msnake_playout_explore), and the standalone kernel that writes the very word such
// a playout plays (msnake_explore_actions).  Included behind msnake_fates.inc and in front of msnake_playout.inc by
// msnake_opponents.hip: it uses msnake_scripted.inc's wave_reduce and hamiltonian_move and msnake_fates.inc's fate_cell and
// pick4; msnake_playout.inc uses its lane_from, explore_draws and explore_pick.  Off the step path.
//
// The rule is the header's (include/msnake.h, msnake_explore_actions).  In the wave: lane s holds snake s.  Every lane
// forms the key k64 = mix64(xseed ^ ctr) from wave-uniform values, runs ONE Philox4x32-10 block -- counter {2 t + (s >> 1),
// global env id}: draws 8 t + 2 s and 8 t + 2 s + 1 are words 2 (s & 1) and 2 (s & 1) + 1 of it -- and decides and chooses
// in the lane, from its snake's candidate set as four bits (bit m: move m + 1).
//
// msnake_explore_kernel: one wavefront per env; the wave only READS the handle's state, in EnvReader's layout and bounds,
// spelled out here for the reason msnake_playout.inc gives (one more caller of that reader's helpers changes the
// instructions of every sibling kernel).  The open mask and safe_greedy's choice are computed as msnake_scripted_kernel
// computes them, the verdicts and wary_greedy's choice as msnake_fates_kernel does; a.which says which of the two the
// policies and the exploring snakes need, tested wave-uniformly: ONE kernel.  lane s stores snake s's action word and
// explored byte.  No LDS, no barrier, no atomics, no scratch.
namespace msnake {

struct ExploreArgs {
    StateView v;
    int32_t* actions; uint8_t* explored;
    int32_t stride;
    uint32_t snakes;                  // snake_mask
    uint32_t pol;                     // policy of snake s in bits 4 s .. 4 s + 3
    uint32_t eps[MSNAKE_MAX_SNAKES];  // eps_q16
    uint32_t xseed_lo, xseed_hi; uint64_t env_id_base;
    int32_t which;                    // EXPLORE_*
};

// a.which of both kernels: what a step has to compute
enum { EXPLORE_NEEDS_OPEN = 1,   // some snake plays safe_greedy, or explores under a policy other than wary_greedy
       EXPLORE_NEEDS_WARY = 2,   // some snake plays wary_greedy
       EXPLORE_DRAWS = 4 };      // some snake has eps > 0

MSNAKE_HD int explore_which(const int32_t* policies, const uint32_t* eps, int ns) {
    int which = 0;
    for (int s = 0; s < ns; ++s) {
        const bool wary = policies[s] == MSNAKE_POLICY_WARY_GREEDY, draws = eps != nullptr && eps[s] > 0u;
        which |= wary ? EXPLORE_NEEDS_WARY : (policies[s] == MSNAKE_POLICY_SAFE_GREEDY || draws) ? EXPLORE_NEEDS_OPEN : 0;
        which |= draws ? EXPLORE_DRAWS : 0;
    }
    return which;
}

__device__ __forceinline__ uint32_t lane_from(uint32_t v, int src_lane) {  // lane l <- lane src_lane(l): ds_bpermute
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}

__device__ __forceinline__ uint64_t explore_mix64(uint64_t z) {  // the splitmix64 finaliser (msnake_hash_states)
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct ExploreDraws { uint32_t u0, u1; };

// draws 8 t + 2 s and 8 t + 2 s + 1 of the env with global id env_id under the key mix64(xseed ^ ctr), s in 0..3
__device__ __forceinline__ ExploreDraws explore_draws(uint64_t xseed, uint64_t ctr, uint64_t env_id, uint32_t t, int s) {
    const uint64_t k64 = explore_mix64(xseed ^ ctr);
    const uint64_t blk = 2ull * (uint64_t)t + (uint64_t)((s >> 1) & 1);  // (8 t + 2 s) >> 2, t zero-extended
    uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32), c2 = (uint32_t)env_id, c3 = (uint32_t)(env_id >> 32);
    uint32_t k0 = (uint32_t)k64, k1 = (uint32_t)(k64 >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (s & 1) ? ExploreDraws{c2, c3} : ExploreDraws{c0, c1};
}

// the action of a snake with base action `base`, candidate set `cand` (bit m: move m + 1) and exploration probability eps
// (units of 1 / 65536) under the draws d; *explored: the action was drawn
__device__ __forceinline__ uint32_t explore_pick(uint32_t base, uint32_t cand, uint32_t eps, ExploreDraws d, bool* explored) {
    cand &= 15u;
    const uint32_t n = (uint32_t)__builtin_popcount(cand);
    const uint32_t idx = (uint32_t)(((uint64_t)d.u1 * (uint64_t)n) >> 32);
    uint32_t seen = 0u, act = 0u;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t bit = (cand >> m) & 1u;
        act = bit != 0u && seen == idx ? (uint32_t)(m + 1) : act;  // the idx-th member in the order 1, 2, 3, 4
        seen += bit;
    }
    *explored = eps > 0u && (d.u0 >> 16) < eps && n > 0u;
    return *explored ? act : base;
}

__global__ __launch_bounds__(256) void msnake_explore_kernel(ExploreArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;
    const int ns = a.v.ns, dim = a.v.dim, cap = a.v.cap;
    const uint32_t hv = a.v.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];  // record word `lane`
    uint32_t ring[MSNAKE_MAX_SNAKES];                                  // ring slot `lane` of every snake
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
        ring[s] = s < ns ? (uint32_t)a.v.body0[((size_t)e * ns + s) * 64 + lane] : 0u;

    // the per-snake fields, lane s <-> snake s (in lanes, not in scalar registers: four snakes' worth of them next to the 16
    // or 20 wave-uniform candidate cells is what spills; they are read out of their lanes where they are used)
    uint32_t V_len = lane < ns ? hv >> 16 : 0u, V_head = 0u;
    const uint32_t V_grow = lane_from(hv, (lane & 3) + SN_B(0));
    const uint32_t V_vel = (lane_from(hv, (lane & 3) + SN_C(0)) >> 16) & 0xFFu;
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        if (s >= ns) continue;
        const int hp0 = (int)((rdlane(hv, SN_C(s)) >> SN_C_HP0_SHIFT) & 63u);
        V_head = hv_writelane_unrolled(V_head, rdlane(ring[s], hp0), (uint32_t)s);  // piece 0 sits in ring slot hp0
    }
    // fn(i, cell, valid): this lane's piece i of snake t (a constant once the loop around the call is unrolled), once for
    // the ring and once per 64-piece pass of the overflow ring; a body is walked up to 64 + cap pieces, an overflow index
    // lies in [0, cap)
    auto for_each_piece = [&](int t, auto fn) {
        if (t >= ns) return;
        const uint32_t wa = rdlane(hv, SN_A(t));
        const int len = (int)(wa >> 16), hp0 = (int)((rdlane(hv, SN_C(t)) >> SN_C_HP0_SHIFT) & 63u);
        const int n = len < 64 + cap ? len : 64 + cap;
        fn((lane - hp0) & 63, ring[t], ((lane - hp0) & 63) < n);
        if (n <= 64) return;
        const int ohp = (int)(wa & 0xFFFFu);
        for (int base = 64; base < n; base += 64) {
            const int i = base + lane;
            int idx = ohp + i - 64;                // >= 0
            idx = idx >= cap ? idx - cap : idx;
            idx = idx >= cap ? cap - 1 : idx;      // (a well-formed record never gets here)
            fn(i, (uint32_t)a.v.ovf[((size_t)e * ns + t) * cap + idx], i < n);
        }
    };
    // fn(cell, valid): this lane's fruit, once (record words) or once per 64-entry pass of `flist`; a list index lies in [0, fcap)
    const bool adv = a.v.rules == MSNAKE_RULES_ADVERSARIAL;
    int nfr = a.v.nf;
    if (adv) {
        nfr = (int)rdlane(hv, HDR_NLIST);
        nfr = nfr < 0 ? 0 : nfr > a.v.fcap ? a.v.fcap : nfr;
    }
    auto for_each_fruit = [&](auto fn) {
        if (adv) {
            for (int base = 0; base < nfr; base += 64) {
                const int f = base + lane;
                fn((uint32_t)a.v.flist[(size_t)e * a.v.fcap + (f < nfr ? f : 0)], f < nfr);
            }
        } else {
            const int f = lane - (a.v.rules == MSNAKE_RULES_NEW_WORLD ? HDR_FRUIT0_N : HDR_FRUIT0_S);
            fn(hv & 0xFFFFu, f >= 0 && f < nfr);
        }
    };
    auto min_of = [](uint32_t x, uint32_t y) { return x < y ? x : y; };
    auto or_of = [](uint32_t x, uint32_t y) { return x | y; };

    const uint32_t my_pol = lane < ns ? (a.pol >> (4 * (lane & 7))) & 15u : 0u;
    uint32_t V_act = 0u;   // lane s: what snake s's policy writes
    uint32_t V_cand = 0u;  // lane s: snake s's candidate set, bit m: move m + 1

    if (my_pol == MSNAKE_POLICY_HAMILTONIAN) {
        const int x = cell_c0(V_head), y = cell_c1(V_head);
        if (V_len > 0u && x >= 0 && x < dim && y >= 0 && y < dim) V_act = hamiltonian_move(x, y, dim);
    }

    if (a.which & EXPLORE_NEEDS_OPEN) {
        // ---- the open moves and safe_greedy (msnake_scripted_kernel): lane q = 4 s + m holds the target of move m + 1 of snake s
        const int qs = (lane >> 2) & 3, qm = lane & 3;
        const uint32_t qhead = lane_from(V_head, qs), qlen = lane_from(V_len, qs);
        const int tx = cell_c0(qhead) + move_d0(qm), ty = cell_c1(qhead) + move_d1(qm);
        const bool onb = lane < 16 && qs < ns && qlen > 0u && tx >= 0 && tx < dim && ty >= 0 && ty < dim;
        uint32_t cv = onb ? cell_pack(tx, ty) : SCRIPTED_NO_CELL;
        uint32_t hit = 0u;  // bit q: a cell this lane has seen equals candidate q
#pragma unroll
        for (int t = 0; t < MSNAKE_MAX_SNAKES; ++t)
            for_each_piece(t, [&](int, uint32_t c, bool valid) {
                const uint32_t cc = valid ? c : 0xFFFFFFFEu;
                asm volatile("" : "+v"(cv));  // (the candidates are read out of their lanes per pass, not kept in 16 scalar registers)
#pragma unroll
                for (int q = 0; q < 16; ++q) hit |= cc == rdlane(cv, q) ? 1u << q : 0u;
            });
        const uint32_t blocked = wave_reduce(hit, or_of);
        const uint32_t open = (uint32_t)ballot(onb) & ~blocked & 0xFFFFu;  // bit 4 s + m
        V_cand = (open >> (4 * (lane & 3))) & 15u;

        if ((a.pol & 0x1111u) != 0u) {  // (bit 0 of a policy id: safe_greedy -- and wary_greedy, whose lanes do not read the result)
            uint32_t key[MSNAKE_MAX_SNAKES];  // min over this lane's fruits and the open moves of distance << 3 | move
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) key[s] = 0xFFFFFFFFu;
            for_each_fruit([&](uint32_t c, bool valid) {
                const int fx = cell_c0(c & 0xFFFFu), fy = cell_c1(c & 0xFFFFu);
#pragma unroll
                for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                    if (s >= ns) continue;
                    const uint32_t head = rdlane(V_head, s);
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const int dx = fx - (cell_c0(head) + move_d0(m)), dy = fy - (cell_c1(head) + move_d1(m));
                        const uint32_t k = ((uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy)) << 3) | (uint32_t)(m + 1);
                        if (valid && ((open >> (4 * s + m)) & 1u) && k < key[s]) key[s] = k;
                    }
                }
            });
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                const uint32_t op = (open >> (4 * s)) & 15u;
                if (s >= ns || op == 0u) continue;
                const uint32_t g = nfr <= 0 ? (uint32_t)__builtin_ctz(op) + 1u  // every distance is 0: the first open move
                                            : wave_reduce(key[s], min_of) & 7u;
                if (lane == s && my_pol == MSNAKE_POLICY_SAFE_GREEDY) V_act = g;
            }
        }
    }

    if (a.which & EXPLORE_NEEDS_WARY) {
        // ---- the verdicts and wary_greedy (msnake_fates_kernel): lane 5 s + a holds the target of action a of snake s
        const int my_s = (lane >= 5) + (lane >= 10) + (lane >= 15), my_a = lane - 5 * my_s;
        const int my_len = (int)lane_from(V_len, my_s), my_vel = (int)lane_from(V_vel, my_s);
        const uint32_t my_grow = lane_from(V_grow, my_s), my_head = lane_from(V_head, my_s);
        const bool live = lane < 5 * ns && my_len > 0;
        const int reverse = my_vel == 0 ? 0 : ((my_vel - 1) ^ 2) + 1;
        const int dir = (my_a == 0 || my_a == reverse) ? my_vel : my_a;  // what turn() leaves, as a velocity code
        const bool moving = dir != 0;
        const int tx = cell_c0(my_head) + vel_v0(dir), ty = cell_c1(my_head) + vel_v1(dir);
        const uint32_t T = live ? fate_cell(tx, ty) : FATE_NO_CELL;
        // bodies: bit 5 s + a of `own` / `other`: T(s, a) equals a piece before the last one of s's body / of another body
        uint32_t own = 0u, other = 0u, Tv = T;  // (the 20 targets: read out of their lanes per pass, as above)
        uint32_t V_tail = FATE_NO_CELL;         // lane t: the last piece of body t
#pragma unroll
        for (int t = 0; t < MSNAKE_MAX_SNAKES; ++t) {
            if (t >= ns) continue;
            const int last = (int)rdlane(V_len, t) - 1;
            const bool t_stands = rdlane(V_vel, t) == 0u;
            for_each_piece(t, [&](int i, uint32_t c, bool valid) {
                const uint32_t cc = c + 0x0101u;
                uint32_t eq = 0u;
                asm volatile("" : "+v"(Tv));
#pragma unroll
                for (int q = 0; q < 20; ++q) eq |= cc == rdlane(Tv, q) ? 1u << q : 0u;
                eq = valid && i < last ? eq : 0u;  // a piece before the last one
                uint32_t o = eq & (31u << (5 * t));
                if (i == 0 && t_stands) o &= ~(1u << (5 * t));  // a standing snake's target is its own head
                own |= o;
                other |= eq & ~(31u << (5 * t));
                const uint64_t at = ballot(valid && i == last);
                if (at != 0ull) V_tail = hv_writelane_unrolled(V_tail, rdlane(cc, (int)__builtin_ctzll(at)), (uint32_t)t);
            });
        }
        own = wave_reduce(own, or_of);
        other = wave_reduce(other, or_of);

        // fruits: lane 5 s + a gets fruits(T(s, a)); fd[s][m]: this lane's fruits' smallest distance to T(s, m + 1)
        uint32_t n_at = 0u;
        uint32_t fd[MSNAKE_MAX_SNAKES][4];
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
            for (int m = 0; m < 4; ++m) fd[s][m] = FATE_FAR;
        for_each_fruit([&](uint32_t c, bool valid) {
            const uint32_t cc = (c & 0xFFFFu) + 0x0101u;
            const int fx = (int)(cc >> 8), fy = (int)(cc & 255u);
            uint32_t pass = 0u;
            asm volatile("" : "+v"(Tv));
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                if (s >= ns) continue;
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const uint32_t tu = rdlane(Tv, 5 * s + k);
                    pass = hv_writelane_unrolled(pass, (uint32_t)__builtin_popcountll(ballot(valid && cc == tu)), (uint32_t)(5 * s + k));
                    if (k == 0) continue;
                    const int dx = fx - (int)((tu >> 8) & 255u), dy = fy - (int)(tu & 255u);
                    const uint32_t d = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
                    fd[s][k - 1] = valid && d < fd[s][k - 1] ? d : fd[s][k - 1];
                }
            }
            n_at += pass;
        });

        // the verdict of lane 5 s + a
        const bool pop = moving && my_grow <= (uint32_t)my_len && 2u * n_at <= (uint32_t)my_len - my_grow;  // len >= grow_to + 2 fruits(T)
        bool self = ((own >> (lane & 31)) & 1u) != 0u, body = ((other >> (lane & 31)) & 1u) != 0u, risk = false;
#pragma unroll
        for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) {
            if (k >= ns) continue;
            const uint32_t len_k = rdlane(V_len, k), vel_k = rdlane(V_vel, k);
            if (len_k == 0u) continue;
            const bool at_tail = T == rdlane(V_tail, k), mine = my_s == k;
            const bool grows = len_k < rdlane(V_grow, k);
            self = self || (mine && at_tail && !pop && !(!moving && len_k == 1u));
            body = body || (!mine && at_tail && grows);
            risk = risk || (!mine && at_tail && !grows);  // TAIL
#pragma unroll
            for (int b = 0; b < 5; ++b) {
                if (b == 0 && vel_k == 0u) continue;  // k stands: its head stays, as piece 0 of its body
                risk = risk || (!mine && T == rdlane(T, 5 * k + b));  // HEAD_ON
            }
        }
        const bool wall = tx < 0 || tx >= dim || ty < 0 || ty >= dim;
        const bool certain = wall || self || body;
        // the masks: bit 5 s + a of ok0 / ok1: the move can be survived / is survived whatever the others do
        const uint64_t ok0 = ballot(live && !certain), ok1 = ballot(live && !certain && !risk);
        const bool wary = my_pol == MSNAKE_POLICY_WARY_GREEDY;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns) continue;
            const uint32_t sure = (uint32_t)(ok1 >> (5 * s)) & 0x1Eu, maybe = (uint32_t)(ok0 >> (5 * s)) & 0x1Eu;
            const uint32_t cnd = sure != 0u ? sure : maybe;  // bit a: action a is a candidate
            uint32_t w = 0u;
            if (cnd != 0u) {
                if (nfr <= 0) {  // every distance is 0: the first candidate
                    w = (uint32_t)__builtin_ctz(cnd);
                } else {
                    uint32_t key = 0xFFFFFFFFu;
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        const uint32_t k = (fd[s][m] << 3) | (uint32_t)(m + 1);
                        key = ((cnd >> (m + 1)) & 1u) && k < key ? k : key;
                    }
                    w = wave_reduce(key, min_of) & 7u;
                }
            }
            if (lane == s && wary) { V_act = w; V_cand = cnd >> 1; }
        }
    }

    // ---- lane s owns snake s's outputs
    bool explored = false;
    if (a.which & EXPLORE_DRAWS) {
        const uint64_t xseed = ((uint64_t)a.xseed_hi << 32) | a.xseed_lo;
        const uint64_t ctr = ((uint64_t)rdlane(hv, HDR_CTR_HI) << 32) | rdlane(hv, HDR_CTR_LO);
        const uint32_t eps = pick4(lane & 3, a.eps[0], a.eps[1], a.eps[2], a.eps[3]);
        const ExploreDraws d = explore_draws(xseed, ctr, a.env_id_base + (uint64_t)e, rdlane(hv, HDR_T), lane & 3);
        V_act = explore_pick(V_act, V_cand, eps, d, &explored);
    }
    if (lane < ns) {
        if ((a.snakes >> lane) & 1u) a.actions[(size_t)e * a.stride + lane] = (int32_t)V_act;
        if (a.explored) a.explored[(size_t)e * ns + lane] = explored ? 1u : 0u;
    }
}

hipError_t launch_explore(const StepParams& p, int rules, const int32_t* policies, const uint32_t* eps, uint64_t xseed,
                          uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* explored, hipStream_t stream) {
    ExploreArgs a{state_view(p, rules), actions, explored, action_stride, snake_mask, 0u, {0u, 0u, 0u, 0u}, (uint32_t)xseed,
                  (uint32_t)(xseed >> 32), p.rest.env_id_base, explore_which(policies, eps, p.n_snakes)};
    for (int s = 0; s < p.n_snakes; ++s) {
        a.pol |= (uint32_t)policies[s] << (4 * s);
        a.eps[s] = eps[s];
    }
    const dim3 grid((unsigned)((p.nenv + 3) / 4)), block(256);
    hipLaunchKernelGGL(msnake_explore_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
