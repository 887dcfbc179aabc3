// msnake_fates.inc -- the one-step fate of every move, the two action masks that follow from it and the opponent
// wary_greedy (msnake_fate_actions).  Included last by msnake_opponents.hip: it uses msnake_scripted.inc's wave_reduce.
// Off the step path.
//
// One wavefront per env; the wave only READS the handle's state, through EnvReader.
//   * Targets: lane 5 s + a <-> action a of snake s (at most 20 lanes).  The lane forms the effective direction (a
//     velocity code: action 0 and a refused reverse keep the snake's own), the target T and whether the snake stands.  A
//     target is compared as ((c0 + 2) << 8) | (c1 + 2), exact for every coordinate from -2 to dim + 1: a head at -1 or
//     dim may step one cell further out.  The 20 targets are then read out once into scalars (v_readlane).
//   * Bodies, one pass: every lane compares the piece it holds (ring slot, or one entry per 64-piece pass of the overflow
//     ring) with the 20 targets and keeps two 20-bit hit masks, "a piece before the last one of the snake's own body" and
//     "... of another body"; two OR reductions over the wave (DPP).  The last piece of each body is one cell: the pass that
//     holds it reads it out (ballot + v_readlane), and the target lanes compare against the four of them afterwards,
//     because what a last piece means depends on the target: the own one counts unless the move pops it (len >= grow_to +
//     2 fruits(T), formed without overflow), another's is BODY while that snake grows and TAIL otherwise.
//   * Fruits, one pass: per target a ballot and a population count give fruits(T) exactly (an adversarial list may hold a
//     cell many times); v_writelane puts the 20 counts of a pass into the target lanes.  With actions asked for, the
//     same pass keeps every lane's smallest L1 distance to the 16 targets of the moves 1..4.
//   * Head-on: the target lanes compare their T with the scalar targets of the other snakes (the standing `action 0` of
//     a snake at rest left out: that head is piece 0 of its body).
//   * The masks are two ballots over the target lanes; wary_greedy is safe_greedy's choice among the candidates the
//     masks leave: the minimum over (fruit, candidate) of distance << 3 | move, ONE min reduction per snake.
//   * lane 5 s + a stores the fate, by and eat bytes, lane 2 s + j the mask bytes, lane s the action word.
// No LDS, no barrier, no atomics, no random numbers, no scratch.
namespace msnake {

struct FatesArgs {
    StateView v;
    int32_t* actions; uint8_t* fate; uint8_t* by; uint8_t* eat; uint8_t* mask;
    int32_t stride;
    uint32_t snakes;  // snake_mask
};

constexpr uint32_t FATE_NO_CELL = 0xFFFFFFFFu;  // equals no cell in the form below
constexpr uint32_t FATE_FAR = 0x0FFFFFFFu;      // no fruit seen: above every distance, and << 3 still fits

// a cell as this kernel compares it; a state cell (msnake_internal.h: coordinates + 1) gets there by + 0x0101
__device__ __forceinline__ uint32_t fate_cell(int c0, int c1) { return ((uint32_t)(c0 + 2) << 8) | (uint32_t)(c1 + 2); }

template <typename T>
__device__ __forceinline__ T pick4(int s, T a, T b, T c, T d) { return s == 0 ? a : s == 1 ? b : s == 2 ? c : d; }

// ACT: the wary_greedy actions are written (snake_mask != 0); FATE / BY / EAT / MASK: fate_dev / by_dev / eat_dev / mask_dev are
template <bool ACT, bool FATE, bool BY, bool EAT, bool MASK>
__global__ __launch_bounds__(256) void msnake_fates_kernel(FatesArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const int e = (int)uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (e >= a.v.nenv) return;
    const int ns = a.v.ns, dim = a.v.dim;
    const EnvReader rd(a.v, e, lane);

    // per snake (wave-uniform): the body, grow_to and the velocity code
    SnakeRef sn[MSNAKE_MAX_SNAKES];
    int len[MSNAKE_MAX_SNAKES], vel[MSNAKE_MAX_SNAKES];
    uint32_t grow[MSNAKE_MAX_SNAKES];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
        sn[s] = rd.snake(s);
        len[s] = sn[s].len;
        grow[s] = s < ns ? rd.word(SN_B(s)) : 0u;
        vel[s] = s < ns ? (int)((rd.word(SN_C(s)) >> 16) & 0xFFu) : 0;
    }

    // ---- lane 5 s + a: the target of action a of snake s
    const int my_s = (lane >= 5) + (lane >= 10) + (lane >= 15);
    const int my_a = lane - 5 * my_s;
    const int my_len = pick4(my_s, len[0], len[1], len[2], len[3]);
    const uint32_t my_grow = pick4(my_s, grow[0], grow[1], grow[2], grow[3]);
    const int my_vel = pick4(my_s, vel[0], vel[1], vel[2], vel[3]);
    const int my_hx = pick4(my_s, sn[0].x, sn[1].x, sn[2].x, sn[3].x), my_hy = pick4(my_s, sn[0].y, sn[1].y, sn[2].y, sn[3].y);
    const bool live = lane < 5 * ns && my_len > 0;
    const int reverse = my_vel == 0 ? 0 : ((my_vel - 1) ^ 2) + 1;
    const int dir = (my_a == 0 || my_a == reverse) ? my_vel : my_a;  // what turn() leaves, as a velocity code
    const bool moving = dir != 0;
    const int tx = my_hx + vel_v0(dir), ty = my_hy + vel_v1(dir);
    const uint32_t T = live ? fate_cell(tx, ty) : FATE_NO_CELL;
    uint32_t tu[MSNAKE_MAX_SNAKES][5];  // the same, wave-uniform
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
        for (int k = 0; k < 5; ++k) tu[s][k] = rdlane(T, 5 * s + k);

    // ---- bodies: bit 5 s + a of `own` / `other`: T(s, a) equals a piece before the last one of s's body / of another body
    uint32_t own = 0u, other = 0u;
    uint32_t tail[MSNAKE_MAX_SNAKES];  // every body's last piece
#pragma unroll
    for (int t = 0; t < MSNAKE_MAX_SNAKES; ++t) {
        tail[t] = FATE_NO_CELL;
        if (t >= ns) continue;
        const int last = len[t] - 1;
        const bool t_stands = vel[t] == 0;
        rd.for_each_piece(sn[t], [&](int i, uint32_t c, bool valid) {
            const uint32_t cc = c + 0x0101u;
            const bool inner = valid && i < last;
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    bool hit = inner && cc == tu[s][k];
                    if (s == t && k == 0) hit = hit && !(t_stands && i == 0);  // a standing snake's target is its own head
                    if (s == t) own |= hit ? 1u << (5 * s + k) : 0u; else other |= hit ? 1u << (5 * s + k) : 0u;
                }
            const uint64_t at = ballot(valid && i == last);
            if (at != 0ull) tail[t] = rdlane(cc, (int)__builtin_ctzll(at));
        });
    }
    own = wave_reduce(own, [](uint32_t x, uint32_t y) { return x | y; });
    other = wave_reduce(other, [](uint32_t x, uint32_t y) { return x | y; });

    // ---- fruits: lane 5 s + a gets fruits(T(s, a)); fd[s][m]: this lane's fruits' smallest distance to T(s, m + 1)
    uint32_t n_at = 0u;
    uint32_t fd[MSNAKE_MAX_SNAKES][4];
#pragma unroll
    for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
#pragma unroll
        for (int m = 0; m < 4; ++m) fd[s][m] = FATE_FAR;
    const int nfr = rd.n_fruits();
    rd.for_each_fruit([&](int, uint32_t c, bool valid) {
        const uint32_t cc = (c & 0xFFFFu) + 0x0101u;
        uint32_t pass = 0u;
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            if (s >= ns) continue;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                pass = hv_writelane_unrolled(pass, (uint32_t)__builtin_popcountll(ballot(valid && cc == tu[s][k])), (uint32_t)(5 * s + k));
        }
        n_at += pass;
        if (ACT) {
            const int fx = (int)(cc >> 8), fy = (int)(cc & 255u);
#pragma unroll
            for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
                if (s >= ns) continue;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int dx = fx - (int)((tu[s][m + 1] >> 8) & 255u), dy = fy - (int)(tu[s][m + 1] & 255u);
                    const uint32_t d = (uint32_t)((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy));
                    fd[s][m] = valid && d < fd[s][m] ? d : fd[s][m];
                }
            }
        }
    });

    // ---- the verdict of lane 5 s + a
    const bool pop = moving && my_grow <= (uint32_t)my_len && 2u * n_at <= (uint32_t)my_len - my_grow;  // len >= grow_to + 2 fruits(T)
    bool self = ((own >> (lane & 31)) & 1u) != 0u, body = ((other >> (lane & 31)) & 1u) != 0u;
    uint32_t by = 0u;
#pragma unroll
    for (int k = 0; k < MSNAKE_MAX_SNAKES; ++k) {
        if (k >= ns) continue;
        // (read again, not kept in scalar registers across the two passes: a v_readlane each)
        const uint32_t len_k = rd.word(SN_A(k)) >> 16, vel_k = (rd.word(SN_C(k)) >> 16) & 0xFFu;
        if (len_k == 0u) continue;
        const bool at_tail = T == tail[k], mine = my_s == k;
        const bool grows = len_k < rd.word(SN_B(k));
        self = self || (mine && at_tail && !pop && !(!moving && len_k == 1u));
        body = body || (!mine && at_tail && grows);
        by |= !mine && at_tail && !grows ? 16u << k : 0u;
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            if (b == 0 && vel_k == 0u) continue;  // k stands: its head stays, as piece 0 of its body
            by |= !mine && T == tu[k][b] ? 1u << k : 0u;
        }
    }
    const bool wall = tx < 0 || tx >= dim || ty < 0 || ty >= dim;
    uint32_t fate = (wall ? MSNAKE_FATE_WALL : 0u) | (self ? MSNAKE_FATE_SELF : 0u) | (body ? MSNAKE_FATE_BODY : 0u) |
                    ((by & 0x0Fu) ? MSNAKE_FATE_HEAD_ON : 0u) | ((by & 0xF0u) ? MSNAKE_FATE_TAIL : 0u) |
                    (moving && n_at != 0u ? MSNAKE_FATE_EATS : 0u);
    fate = live ? fate : 0u;
    by = live ? by : 0u;
    if (lane < 5 * ns) {
        const size_t at = (size_t)e * ns * 5 + lane;
        if (FATE) a.fate[at] = (uint8_t)fate;
        if (BY) a.by[at] = (uint8_t)by;
        if (EAT) a.eat[at] = (uint8_t)(live && moving ? (n_at < 255u ? n_at : 255u) : 0u);
    }

    // ---- the masks: bit 5 s + a of ok0 / ok1: the move can be survived / is survived whatever the others do
    const uint64_t ok0 = ballot(live && (fate & MSNAKE_FATE_CERTAIN) == 0u);
    const uint64_t ok1 = ballot(live && (fate & (MSNAKE_FATE_CERTAIN | MSNAKE_FATE_RISK)) == 0u);
    if (MASK && lane < 2 * ns)
        a.mask[(size_t)e * ns * 2 + lane] = (uint8_t)((((lane & 1) ? ok1 : ok0) >> (5 * (lane >> 1))) & 31ull);

    // ---- wary_greedy: safe_greedy's choice among the moves 1..4 of mask[1], or of mask[0] when that is empty
    if (ACT) {
        uint32_t act[MSNAKE_MAX_SNAKES];
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s) {
            act[s] = 0u;
            if (s >= ns) continue;
            const uint32_t sure = (uint32_t)(ok1 >> (5 * s)) & 0x1Eu, maybe = (uint32_t)(ok0 >> (5 * s)) & 0x1Eu;
            const uint32_t cand = sure != 0u ? sure : maybe;
            if (cand == 0u) continue;
            if (nfr <= 0) {  // every distance is 0: the first candidate
                act[s] = (uint32_t)__builtin_ctz(cand);
            } else {
                uint32_t key = 0xFFFFFFFFu;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t k = (fd[s][m] << 3) | (uint32_t)(m + 1);
                    key = ((cand >> (m + 1)) & 1u) && k < key ? k : key;
                }
                act[s] = wave_reduce(key, [](uint32_t x, uint32_t y) { return x < y ? x : y; }) & 7u;
            }
        }
        if (lane < ns && ((a.snakes >> lane) & 1u))
            a.actions[(size_t)e * a.stride + lane] = (int32_t)pick4(lane, act[0], act[1], act[2], act[3]);
    }
}

hipError_t launch_fates(const StepParams& p, int rules, uint32_t snake_mask, int32_t* actions, int32_t action_stride, uint8_t* fate,
                        uint8_t* by, uint8_t* eat, uint8_t* mask, hipStream_t stream) {
    const FatesArgs a{state_view(p, rules), actions, fate, by, eat, mask, action_stride, snake_mask};
    const dim3 grid((unsigned)((p.nenv + 3) / 4)), block(256);
    return launch_by_flags<5>((snake_mask != 0u ? 16 : 0) | (fate ? 8 : 0) | (by ? 4 : 0) | (eat ? 2 : 0) | (mask ? 1 : 0),
                              [&](auto act, auto ft, auto b, auto et, auto mk) {
        hipLaunchKernelGGL((msnake_fates_kernel<act.value, ft.value, b.value, et.value, mk.value>), grid, block, 0, stream, a);
    });
}

}  // namespace msnake
