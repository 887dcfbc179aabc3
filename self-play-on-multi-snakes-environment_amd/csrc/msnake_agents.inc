// msnake_agents.inc -- per-snake outcomes of a step from two consecutive states (msnake_agent_outcomes).
// Included behind msnake_cells.inc, last, by msnake_views.hip; it takes nothing from its siblings.  Off the step path:
// nothing here is referenced by msnake_step_kernel, and the kernel only READS the handle's state.
//
// One lane per (env, snake): a group of four lanes per env (lane s of the group = snake s; lanes s >= n_snakes idle),
// 16 envs per wave.  Everything the call needs of an env -- SN_A(s) for the length, SN_B(s) for grow_to, HDR_FLAGS for
// the new_world alive bits -- lies in the first 64 bytes of its record, so lane q of a group loads words 4 q .. 4 q + 3
// (ONE 16-byte load per lane, 64 contiguous bytes per env) and the group hands the words round by quad-permute DPP:
// lane s takes component s of lane 0 (SN_A) and of lane 1 (SN_B) and component 3 of lane 3 (HDR_FLAGS).  Lanes of the
// batch tail and lanes s >= n_snakes therefore stay in the kernel until the exchange is over (they read the last env's
// record) and are masked afterwards.  The "before" facts and the episode totals live in the caller's tracker, one
// 32-byte row per lane: two 16-byte loads and two 16-byte stores at 4-byte alignment.  The rows and every output are
// indexed by env * n_snakes + s, so consecutive live lanes touch consecutive memory.
// No random numbers, no LDS, no barrier, no atomics, no scratch.
namespace msnake {

struct AgentsArgs {
    const uint32_t* hdr; int32_t* track; const uint8_t* done;
    float* rew; uint8_t* ate; uint8_t* flags; int32_t* info;
    int32_t nenv, ns, rules;
};

constexpr int AGENTS_THREADS = 256;  // 64 envs per workgroup
static_assert(SN_A(0) == 0 && SN_B(0) == 4 && HDR_FLAGS == 15 && MSNAKE_MAX_SNAKES == 4, "the record words a group of four lanes exchanges");

// four dwords at 4-byte alignment (tracker rows and info rows need no more): one dwordx4 access
struct __attribute__((packed, aligned(4))) Words4 { uint32_t x, y, z, w; };

// every lane of a group of four <- lane Q of its group
template <int Q>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, Q * 0x55, 0xF, 0xF, true);
}
// component s of the four dwords that lane Q of the group holds
template <int Q>
__device__ __forceinline__ uint32_t quad_pick(const uint4& w, int s) {
    const uint32_t x = quad_bcast<Q>(w.x), y = quad_bcast<Q>(w.y), z = quad_bcast<Q>(w.z), t = quad_bcast<Q>(w.w);
    return s == 0 ? x : s == 1 ? y : s == 2 ? z : t;
}

// ARM: the tracker is written from the state; otherwise outcomes are produced and the tracker advanced
template <bool ARM>
__global__ __launch_bounds__(AGENTS_THREADS) void msnake_agents_kernel(AgentsArgs a) {
    const int tid = (int)(blockIdx.x * AGENTS_THREADS + threadIdx.x);
    const int e = tid >> 2, s = tid & 3;
    const bool live = e < a.nenv && s < a.ns;
    const int el = e < a.nenv ? e : a.nenv - 1;  // (the batch tail reads the last env's record and writes nothing)
    const uint4 w = reinterpret_cast<const uint4*>(a.hdr + (size_t)el * MSNAKE_HDR_WORDS)[s];
    const uint32_t wA = quad_pick<0>(w, s), wB = quad_pick<1>(w, s), hflags = quad_bcast<3>(w.w);
    if (!live) return;  // (behind the exchange: no cross-lane operation below)

    const bool nw = a.rules == MSNAKE_RULES_NEW_WORLD;
    const uint32_t now = nw ? (hflags >> s) & 1u : ((wA >> 16) != 0u ? 1u : 0u);
    const size_t k = (size_t)e * (size_t)a.ns + (size_t)s;
    Words4* row = reinterpret_cast<Words4*>(a.track) + 2 * k;
    if (ARM) {
        row[0] = Words4{wB, now, 0u, 0u};
        row[1] = Words4{0u, 0u, 0u, 0u};
        return;
    }
    const Words4 r0 = row[0], r1 = row[1];  // grow_to, alive, ep_fruit, ep_alive_steps | first_death, ep_steps, ep_return, 0
    const bool done = a.done[e] != 0;
    const bool was = r0.y != 0u;
    const int32_t diff = (int32_t)(wB - r0.x);
    const uint32_t ate = diff > 0 ? (uint32_t)diff >> 1 : 0u;
    const bool died = was && !now;
    const bool ended = was && (died || done);
    // the rule set's own formula for the main snake, applied to snake s ([S]:166-197, [A]:166-201; [NE]:39-40 with
    // [N]:107 done = snake.alive)
    const float rew = (nw ? now != 0u : died) ? -1.0f : (float)ate;
    const uint32_t ep_fruit = r0.z + ate, ep_alive = r0.w + now, ep_steps = r1.y + 1u;
    const uint32_t first_death = (died && r1.x == 0u) ? ep_steps : r1.x;
    const uint32_t ep_return = __float_as_uint(__uint_as_float(r1.z) + rew);

    if (a.rew) a.rew[k] = rew;
    if (a.ate) a.ate[k] = (uint8_t)(ate < 255u ? ate : 255u);
    if (a.flags)
        a.flags[k] = (uint8_t)((now ? MSNAKE_AGENT_ALIVE : 0) | (was ? MSNAKE_AGENT_WAS_ALIVE : 0) | (died ? MSNAKE_AGENT_DIED : 0) |
                               (ended ? MSNAKE_AGENT_ENDED : 0));
    if (a.info) reinterpret_cast<Words4*>(a.info)[k] = Words4{ep_fruit, ep_alive, first_death, ep_return};
    // a done env's rows become what ARM writes after the reset the caller issues next
    row[0] = done ? Words4{3u, 1u, 0u, 0u} : Words4{wB, now, ep_fruit, ep_alive};
    row[1] = done ? Words4{0u, 0u, 0u, 0u} : Words4{first_death, ep_steps, ep_return, 0u};
}

hipError_t launch_agents(const StepParams& p, int rules, bool arm, int32_t* track, const uint8_t* done, float* rew, uint8_t* ate,
                         uint8_t* flags, int32_t* info, hipStream_t stream) {
    const AgentsArgs a{p.hdr, track, done, rew, ate, flags, info, p.nenv, p.n_snakes, rules};
    const dim3 grid((unsigned)((4 * (size_t)p.nenv + AGENTS_THREADS - 1) / AGENTS_THREADS)), block(AGENTS_THREADS);
    if (arm) hipLaunchKernelGGL(msnake_agents_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(msnake_agents_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace msnake
