// ntm_base.h — what every layer of the device code shares: kInf, rsqrt_nr, the solver's
// constants, the build switches with their defaults, the chunk size of the LDS
// contractions (NTM_CH, NTM_CHUNK_PRAGMA) and the wave-level LDS fence NTM_WSYNC.
//
// Build switches.  A translation unit that wants its own NTM_CH, NTM_CHUNK_UNROLL,
// NTM_COLL3 or NTM_SUB_LANEIDX defines it before its first include of any ntm_*.h header
// (ntm_n20.hip, ntm_n20near*.hip, ntm_n50.hip and ntm_n50m3.hip do, as do
// tools/lift_lanes_check.hip and echelon_sub_check.hip); the command line may set any
// switch (-DNTM_CH=5).  This header only supplies the defaults, under #ifndef, and every
// header is #pragma once: a value defined after the first include is a redefinition error
// or has no effect.  All of the device code of one translation unit is compiled with one
// value of each.  NTM_FAR_N20 and NTM_QI_MAXN, which only a command line sets, have their
// defaults next to their users in ntm_ws.h.
#pragma once
#include <hip/hip_runtime.h>

namespace ntm {

constexpr double kInf = __builtin_huge_val();

// 1/sqrt(x) for x > 0: v_rsq_f64 plus two Newton steps (full fp64 accuracy;
// the pivots of the small Cholesky factorisations sit on their sequential
// critical path, where the IEEE sqrt + division expansions cost ~25 dependent ops)
__device__ __forceinline__ double rsqrt_nr(double x) {
    double y = __builtin_amdgcn_rsq(x);
    const double h = 0.5 * x;
    y = fma(y, fma(-h * y, y, 0.5), y);
    y = fma(y, fma(-h * y, y, 0.5), y);
    return y;
}

constexpr double kDepTol = 1e-8;   // GI linear-dependence threshold (oracle GI_DEP_TOL)
constexpr int kMaxNT = 32;         // explicit R^{-1} in GI up to this horizon (WS::useT)
// a failed candidate continues on Goldfarb-Idnani's dual path with certified
// re-solves (qp_phase); up to N + kCdpExtra re-solves before GI itself takes over
constexpr int kCdpExtra = 8;
#ifndef NTM_SUB_PRESCALE
#define NTM_SUB_PRESCALE 0 // 1: long horizons, echelon substitutions on accumulators scaled by 1/E[l][l] (slower)
#endif
#ifndef NTM_MU_AHEAD
#define NTM_MU_AHEAD 0     // long horizons: steps ahead the multipliers' back substitution loads E (0: none)
#endif
#ifndef NTM_SUB_LANEIDX
#define NTM_SUB_LANEIDX 0  // 1: the certificate's sparse pass takes rows and z by readlane (long horizons;
#endif                     // on in the mode-3 TU: 76.9 -> 76.3 ms, while mode 2 ran 64.9 -> 65.6 ms)
#ifndef NTM_COLL3
#define NTM_COLL3 1        // k = 2 sets with one collision (three holes) on the null-space path (round 6)
#endif
#ifndef NTM_N20_NO_RATE
#define NTM_N20_NO_RATE 0  // 1: the slim N = 20 far kernels of this unit are compiled without rate rows
#endif                     // (rate_rows in ntm_ws.h; on in ntm_n20.hip and the diag20 build)
constexpr int kBoxRepairs = 16;  // box-only QPs: single-row exchanges before GI (qp_phase)   // also at N = 50: 16 / 32 were no faster in mode 2, 6% / 10% slower in mode 3
// A constant row (Lin_i = 0: the x_0 rows of getWLc, state rows Gamma doesn't
// reach) is violated when b_i < -kConstTol (D22, oracle CONST_ROW_TOL): the same
// absolute 1e-9 the KKT certificate allows on a unit-scale row.  An exact test
// turned a state that the plant step leaves one ulp outside a bound the
// previous plan held it at (x_{k+1} = xmin - ulp) into an infeasible QP.
constexpr double kConstTol = 1e-9;
constexpr int kRowMulti = 256;     // WS::rinfo flag: the state row has two or more non-zeros
constexpr int kGiWarmRejected = 100;   // gi_solve: the warm-start set was not dual feasible (caller reruns cold)

// Terms per batch of the LDS contractions (loads issued ahead of their uses);
// a translation unit may set its own (ntm_n50.hip)
#ifndef NTM_CH
#define NTM_CH 4
#endif
// Unroll count of the CH-batched chunk loops: empty (the compiler's choice, full
// unrolling at the BASELINE horizons) unless a build sets NTM_CHUNK_UNROLL
#define NTM_STR_(x) #x
#define NTM_STR(x) NTM_STR_(x)
#ifdef NTM_CHUNK_UNROLL
#define NTM_CHUNK_PRAGMA _Pragma(NTM_STR(unroll NTM_CHUNK_UNROLL))
#else
#define NTM_CHUNK_PRAGMA
#endif

#define NTM_WSYNC()                                              \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
    } while (0)

}  // namespace ntm
