// msnake_device.h -- what more than one of the three kernel units uses: the wave-level helpers, the record-word
// writers (HV_SET*), launch_by_flags, and -- through msnake_envread.inc, included at the end -- the reader of env
// state in HBM.  Included by msnake_kernels.hip (the step kernel), msnake_opponents.hip and msnake_views.hip (the
// kernels off the step path).  Everything here is an inline function, a template, a constant or a macro: including it
// emits no code, and no unit sees another's kernels.
#ifndef MSNAKE_DEVICE_H
#define MSNAKE_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "msnake_internal.h"

namespace msnake {

// ------------------------------------------------------------------------------------------------
// wave-level helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// lanes of one wave exchange data through LDS: DS operations of a wave execute in program order,
// this only stops the compiler from moving/forwarding accesses across the exchange point
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t mbcnt(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// within each row of 16 lanes: lane l <- lane l+N (row_shl) / lane l-N (row_shr); lanes without a
// source keep `old`
template <int N>
__device__ __forceinline__ uint32_t row_shl(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x100 + N, 0xF, 0xF, false);
}
template <int N>
__device__ __forceinline__ uint32_t row_shr(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x110 + N, 0xF, 0xF, false);
}
// v_mov_b32 dpp restricted to some rows (ROWS) and some groups of four lanes within each row (BANKS);
// every other lane keeps `old`: a column of the env record is replaced by ONE instruction
template <int CTRL, int ROWS, int BANKS>
__device__ __forceinline__ uint32_t dpp_into(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWS, BANKS, false);
}
constexpr int DPP_IDENTITY = 0xE4;  // quad_perm:[0,1,2,3]
// lane compares straight to a 64-bit lane mask (v_cmp into an SGPR pair), and a lane mask back to a
// per-lane predicate without an instruction: `ballot(b)` of a bool that also has other uses costs a
// v_cndmask + v_cmp pair, `(mask >> lane) & 1` a shift, an and and a compare
constexpr int CMP_EQ = 32, CMP_NE = 33, CMP_UGT = 34, CMP_UGE = 35, CMP_ULT = 36;
template <int PRED>
__device__ __forceinline__ uint64_t lanes_where(uint32_t a, uint32_t b) { return __builtin_amdgcn_uicmp(a, b, PRED); }
__device__ __forceinline__ bool in_mask(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }
// 1 << BIT if the (wave-uniform) lane mask is not empty, else 0: two scalar instructions.  (Written in C, a
// uniform `m != 0` that is used as a number takes a detour through a VGPR.)
template <int BIT>
__device__ __forceinline__ uint32_t bit_if_any(uint64_t m) {
    uint32_t b;
    asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, %2, 0" : "=s"(b) : "s"(m), "n"(1u << BIT) : "scc");
    return b;
}
// lane l <- lane l-1 (lane 0 keeps its value): v_mov_b32 dpp wave_shr:1
__device__ __forceinline__ uint32_t shift_up1(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false);
}

// inclusive prefix sum over the 64 lanes: Hillis-Steele inside each row of 16 (row_shr 1,2,4,8),
// then row_bcast:15 into rows 1,3 and row_bcast:31 into rows 2,3 (lanes without a source add 0)
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);
    return x;
}

// record word idx <- a wave-uniform value by v_writelane_b32, no lane mask (a `lane == idx` select
// costs a compare plus an SGPR pair per index, and the compiler keeps all those masks live for the
// whole kernel: 60+ SGPRs, the source of the SGPR spills of the persistent kernel).  clang has no
// builtin for it.  val must be wave-uniform (it goes through v_readfirstlane unless it is known to
// be).  gfx9 VALU instructions read ONE SGPR, so the lane select is an inline constant (HV_SET_C,
// literal index) or M0 (HV_SET, computed index; the s_nop covers an index that a VALU instruction
// produced: v_readlane -> SGPR -> lane select needs 4 wait states).
template <int IDX>
__device__ __forceinline__ uint32_t hv_writelane_c(uint32_t old, uint32_t val) {
    static_assert(IDX >= 0 && IDX < 64, "lane index");
    asm("v_writelane_b32 %0, %1, %2" : "+v"(old) : "s"(uni(val)), "n"(IDX));
    return old;
}
__device__ __forceinline__ uint32_t hv_writelane(uint32_t old, uint32_t val, uint32_t idx) {
    asm("s_nop 3\n\ts_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(old) : "s"(uni(val)), "s"(uni(idx)) : "m0");
    return old;
}
#define HV_SET_C(idx, val) hv = hv_writelane_c<(idx)>(hv, (uint32_t)(val))
#define HV_SET(idx, val) hv = hv_writelane(hv, (uint32_t)(val), (uint32_t)(idx))
// index that is a constant once the enclosing loop is unrolled (snake columns, inline fruits): the switch
// folds to the immediate form -- one instruction instead of M0 write + hazard nop + v_writelane.
// Never for an index that is only known at run time (that would be a 32-way jump table).
__device__ __forceinline__ uint32_t hv_writelane_unrolled(uint32_t old, uint32_t val, uint32_t idx) {
    switch (idx) {
        case 0: return hv_writelane_c<0>(old, val); case 1: return hv_writelane_c<1>(old, val); case 2: return hv_writelane_c<2>(old, val); case 3: return hv_writelane_c<3>(old, val); case 4: return hv_writelane_c<4>(old, val); case 5: return hv_writelane_c<5>(old, val); case 6: return hv_writelane_c<6>(old, val); case 7: return hv_writelane_c<7>(old, val); case 8: return hv_writelane_c<8>(old, val); case 9: return hv_writelane_c<9>(old, val); case 10: return hv_writelane_c<10>(old, val); case 11: return hv_writelane_c<11>(old, val); case 12: return hv_writelane_c<12>(old, val); case 13: return hv_writelane_c<13>(old, val); case 14: return hv_writelane_c<14>(old, val); case 15: return hv_writelane_c<15>(old, val); case 16: return hv_writelane_c<16>(old, val); case 17: return hv_writelane_c<17>(old, val); case 18: return hv_writelane_c<18>(old, val); case 19: return hv_writelane_c<19>(old, val); case 20: return hv_writelane_c<20>(old, val); case 21: return hv_writelane_c<21>(old, val); case 22: return hv_writelane_c<22>(old, val); case 23: return hv_writelane_c<23>(old, val); case 24: return hv_writelane_c<24>(old, val); case 25: return hv_writelane_c<25>(old, val); case 26: return hv_writelane_c<26>(old, val); case 27: return hv_writelane_c<27>(old, val); case 28: return hv_writelane_c<28>(old, val); case 29: return hv_writelane_c<29>(old, val); case 30: return hv_writelane_c<30>(old, val); case 31: return hv_writelane_c<31>(old, val);
        default: return hv_writelane(old, val, idx);
    }
}
#define HV_SET_U(idx, val) hv = hv_writelane_unrolled(hv, (uint32_t)(val), (uint32_t)(idx))

// Run-time flags -> bool template arguments, for the launchers of the off-step kernels: bit N - 1 - i of `flags` becomes
// argument i of f(std::bool_constant<..>...), which launches.  Host code only.  No flag set (nothing to write) is
// hipErrorInvalidValue, and f is never instantiated for it: no kernel exists for that combination.
template <int N, bool... B, typename F>
static hipError_t launch_by_flags(int flags, const F& f) {
    if constexpr (N > 0) {
        return !((flags >> (N - 1)) & 1) ? launch_by_flags<N - 1, B..., false>(flags, f) : launch_by_flags<N - 1, B..., true>(flags, f);
    } else if constexpr ((B || ...)) {
        f(std::bool_constant<B>{}...);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;
    }
}

}  // namespace msnake

#include "msnake_envread.inc"  // StateView and EnvReader: how the kernels off the step path read an env's state

#endif
