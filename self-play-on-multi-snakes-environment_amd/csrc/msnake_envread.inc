// msnake_envread.inc -- how a kernel off the step path reads one env's state out of HBM, written once.
// Included at the end of msnake_device.h, and through it by all three kernel units: it uses that header's rdlane and
// msnake_internal.h's cell codes.  Only inline functions and templates, so every unit may include it; nothing here is
// referenced by msnake_step_kernel.
//
// One wavefront per env.  The layout (msnake_internal.h) as the reader sees it:
//   * the 256-byte record, lane l <-> word l (one coalesced load); per-snake fields come out by v_readlane;
//   * every snake's 64-slot body ring, lane l <-> slot l (one 128-byte load per snake, issued with the record);
//     piece i < 64 sits in ring slot (hp0 + i) & 63;
//   * piece i >= 64 sits at ovf[(ohp + i - 64) % cap], strided in whole waves;
//   * fruits are record words by lane (snake_env / new_world) or the complete list `flist` in passes of 64
//     (adversarial).
// len, ohp and HDR_NLIST come straight out of HBM and turn into addresses here, under one set of bounds: a body is
// walked up to 64 + cap pieces, an overflow index lies in [0, cap), a fruit index in [0, fcap).  Used by the space,
// copy_envs, state export and local-window kernels; msnake_scripted.inc and msnake_cells.inc keep their own walk (DESIGN.md, section 12:
// on this reader they measured slower).
namespace msnake {

// a handle's state as the off-step kernels receive it
struct StateView {
    uint32_t* hdr; uint16_t* body0; uint16_t* ovf; uint16_t* fl0; uint16_t* flist;
    int32_t nenv, dim, ns, nf, cap, fcap, rules;
};

static StateView state_view(const StepParams& p, int rules) {
    return StateView{p.hdr, p.body0, p.ring, p.fl0, p.flist, p.nenv, p.dim, p.n_snakes, p.n_fruits, p.rest.cap, p.fcap, rules};
}

// fruits of an env whose record word HDR_NLIST is `nlist`
__device__ __forceinline__ int fruit_count(const StateView& v, uint32_t nlist) {
    if (v.rules != MSNAKE_RULES_ADVERSARIAL) return v.nf;
    const int n = (int)nlist;
    return n < 0 ? 0 : n > v.fcap ? v.fcap : n;
}

// One snake's wave-uniform fields, read out of the record and the ring once (EnvReader::snake)
struct SnakeRef {
    int s, len, hp0;  // index, body length (0 for s >= ns), ring slot of the head
    uint32_t head;    // piece 0's cell (0 for an empty body)
    int x, y;         // the head's coordinates; -2 for an empty body
};

// Env e of view v, as lane `lane` of the wave that reads it.  Every lane of the wave must build it.  s is a
// compile-time snake index (an unrolled loop).
struct EnvReader {
    const StateView& v;
    const int e, lane;
    uint32_t hv;                       // record word `lane`
    uint32_t ring[MSNAKE_MAX_SNAKES];  // ring slot `lane` of every snake

    __device__ __forceinline__ EnvReader(const StateView& view, int env, int ln) : v(view), e(env), lane(ln) {
        const int ns = v.ns;
        hv = v.hdr[(size_t)e * MSNAKE_HDR_WORDS + lane];
#pragma unroll
        for (int s = 0; s < MSNAKE_MAX_SNAKES; ++s)
            ring[s] = s < ns ? (uint32_t)v.body0[((size_t)e * ns + s) * 64 + lane] : 0u;
    }

    __device__ __forceinline__ uint32_t word(int i) const { return rdlane(hv, i); }
    __device__ __forceinline__ uint32_t flags() const { return word(HDR_FLAGS); }
    __device__ __forceinline__ int n_fruits() const { return fruit_count(v, word(HDR_NLIST)); }

    // the compiler does not merge v_readlane reads: ask once per snake and keep the answer
    __device__ __forceinline__ SnakeRef snake(int s) const {
        SnakeRef r{s, 0, 0, 0u, -2, -2};
        if (s < v.ns) {
            r.len = (int)(word(SN_A(s)) >> 16);
            r.hp0 = (int)((word(SN_C(s)) >> SN_C_HP0_SHIFT) & 63u);
            if (r.len > 0) {
                r.head = rdlane(ring[s], r.hp0);  // piece 0 sits in ring slot hp0
                r.x = cell_c0(r.head); r.y = cell_c1(r.head);
            }
        }
        return r;
    }

    // fn(i, cell, valid): this lane's piece i of the snake, once for the ring and once per 64-piece pass of the overflow
    // ring.  Wave-uniform control flow; `valid` is the lane predicate (an invalid lane's cell is some cell of the ring).
    template <typename F>
    __device__ __forceinline__ void for_each_piece(const SnakeRef& sn, F fn) const {
        const int s = sn.s, ns = v.ns, cap = v.cap;
        if (s >= ns) return;
        const int n = sn.len < 64 + cap ? sn.len : 64 + cap;
        fn((lane - sn.hp0) & 63, ring[s], ((lane - sn.hp0) & 63) < n);
        if (n <= 64) return;
        const int ohp = (int)(word(SN_A(s)) & 0xFFFFu);
        for (int base = 64; base < n; base += 64) {
            const int i = base + lane;
            int idx = ohp + i - 64;                // >= 0
            idx = idx >= cap ? idx - cap : idx;
            idx = idx >= cap ? cap - 1 : idx;      // (a well-formed record never gets here)
            fn(i, (uint32_t)v.ovf[((size_t)e * ns + s) * cap + idx], i < n);
        }
    }

    // fn(f, cell, valid): this lane's fruit f, once (record words) or once per 64-entry pass of `flist`
    template <typename F>
    __device__ __forceinline__ void for_each_fruit(F fn) const {
        const int nfr = n_fruits();
        if (v.rules == MSNAKE_RULES_ADVERSARIAL) {
            for (int base = 0; base < nfr; base += 64) {
                const int f = base + lane;
                fn(f, (uint32_t)v.flist[(size_t)e * v.fcap + (f < nfr ? f : 0)], f < nfr);
            }
        } else {
            const int f = lane - (v.rules == MSNAKE_RULES_NEW_WORLD ? HDR_FRUIT0_N : HDR_FRUIT0_S);
            fn(f, hv & 0xFFFFu, f >= 0 && f < nfr);
        }
    }
};

}  // namespace msnake
