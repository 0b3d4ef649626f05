// ntm_diag.h — what the trace (NTM_DEBUG_SCEN) and diagnostic (NTM_STAMPS) builds add:
// the GI trace macros, the per-phase cycle stamps and the names of their slots.  The
// production library compiles all of it away.
#pragma once
#include <hip/hip_runtime.h>

namespace ntm {

// Trace build only (make trace NTM_DEBUG_SCEN=s): printf GI's iterations for
// one scenario.  The production library compiles every trace away.
#ifdef NTM_DEBUG_SCEN
__shared__ int ntm_trace_grp;   // group (of this one-wave block) that owns the traced scenario
#define NTM_TRACE_SET(s, g, l)                                                  \
    do {                                                                        \
        if (threadIdx.x == 0) ntm_trace_grp = -1;                               \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                 \
        __builtin_amdgcn_wave_barrier();                                        \
        if ((l) == 0 && (s) == NTM_DEBUG_SCEN) ntm_trace_grp = (g);             \
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");                 \
        __builtin_amdgcn_wave_barrier();                                        \
    } while (0)
#define NTM_TRACE(...) \
    do { if (ntm_trace_grp == (int)((threadIdx.x & 63) / P) && l == 0) printf(__VA_ARGS__); } while (0)
#else
#define NTM_TRACE_SET(s, g, l) (void)0
#define NTM_TRACE(...) (void)0
#endif

// Diagnostic build only (-DNTM_STAMPS): per-phase s_memtime cycle totals,
// summed over waves into ntm_stamps[] (read with ntm_debug_stamps).  The
// production library compiles every stamp away.
#define NTM_NSTAMPS 104
#ifdef NTM_STAMPS
extern __device__ unsigned long long ntm_stamps[NTM_NSTAMPS];
__shared__ unsigned long long ntm_lds_stamps[NTM_NSTAMPS];   // per block (= per wave), flushed once
#define NTM_T0(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define NTM_ACC(i, v)                                                                   \
    do {                                                                                \
        unsigned long long t1_ = __builtin_amdgcn_s_memtime();                         \
        if ((threadIdx.x & 63) == 0) ntm_lds_stamps[i] += t1_ - (v);                   \
        v = t1_;                                                                        \
    } while (0)
#define NTM_CNT(i) \
    do { if ((threadIdx.x & 63) == 0) ntm_lds_stamps[i] += 1ull; } while (0)
#define NTM_STAMPS_INIT() \
    do { for (int i_ = threadIdx.x; i_ < NTM_NSTAMPS; i_ += blockDim.x) ntm_lds_stamps[i_] = 0; __syncthreads(); } while (0)
#define NTM_STAMPS_FLUSH() \
    do { __syncthreads(); for (int i_ = threadIdx.x; i_ < NTM_NSTAMPS; i_ += blockDim.x) atomicAdd(&ntm_stamps[i_], ntm_lds_stamps[i_]); } while (0)
#else
#define NTM_T0(v) (void)0
#define NTM_ACC(i, v) (void)0
#define NTM_CNT(i) (void)0
#define NTM_STAMPS_INIT() (void)0
#define NTM_STAMPS_FLUSH() (void)0
#endif
enum { ST_LIFT, ST_COST, ST_SCALE, ST_CAND, ST_REGRAM, ST_GI, ST_POLISH, ST_ROLL, ST_GI_FACT, ST_GI_CHECK,
       ST_GI_DIR, ST_GI_ADD, ST_GI_DROP, CN_CHECK, CN_CAND, CN_HIT,
       ST_P_CLASS, ST_P_GRAM, ST_P_CHOL, ST_P_SCHUR, ST_P_BWD, ST_P_KKT, CN_REPAIR, CN_GIRUN,
       ST_S_E, ST_S_Y, ST_S_K, ST_S_CHOL, ST_S_SOLVE, CN_TRY_EARLY, CN_FAIL_EARLY, CN_FAIL_LATE,
       CN_FAIL_IT1, CN_FAIL_IT2, CN_GI_IT1, CN_GI_IT2, CN_GI_LATE, CN_TRY_IT1, CN_TRY_IT2, CN_WARM_TRY, CN_WARM_OK, CN_WARM_DEP, CN_WARM_NEG, CN_WARM_FULL, CN_ALT_TRY, CN_ALT_HIT,
       ST_K_Y, ST_K_CHK, ST_K_GRAD, ST_K_MU, ST_K_SUB, ST_C_A, ST_C_B, ST_C_Y, ST_C_SQ,
       ST_SC_COL, ST_SC_ROW, ST_SC_END, ST_L_COEF, ST_L_LOOP, CN_CYC_HIT, CN_CYC_SKIP,
       CN_FK_DUAL, CN_FK_PRIMAL, CN_FK_SING, CN_FK_BOTH, ST_GI_WARM,
       CN_CDP_DROP, CN_CDP_RES, CN_CDP_PART, CN_CDP_DIR, CN_CDP_GI,
       CN_CDPX_SING0, CN_CDPX_SING1, CN_CDPX_BUDGET, CN_CDPX_DIR, CN_CDPX_NOVIOL, CN_CDPX_FULLDUAL, CN_CDPX_TINF,
       CN_BORD_K0, CN_BORD_K1, CN_BORD_K2, CN_BORD_K3, CN_BORD_K4P, CN_SQ_K0, CN_SQ_K1, CN_SQ_K2, CN_SQ_COLL,
       CN_CDPX_NAN, CN_NAN_BORD, CN_NAN_K0, CN_NAN_K1, CN_NAN_K2, CN_NAN_COLL, CN_NAN_COLL2, CN_NAN_PRIMFAIL,
       CN_NAN_V, CN_BX_O1, CN_BX_O2, CN_BX_O3P, CN_BX_NEG, CN_BX_NOCLASS, CN_CDP_SKIP, CN_CDP_SKIPDIR,
       ST_COUNT };   // not a slot: the number of slots above
static_assert(ST_COUNT <= NTM_NSTAMPS, "a slot past ntm_lds_stamps[]: raise NTM_NSTAMPS (and tools/diag_phases.py's count)");

}  // namespace ntm
