// ntm_step.h — the hot-path kernels k_mpc_step / k_mpc_run (one fused launch
// per MPC time step, or per closed loop, for the whole scenario batch) and
// their per-scenario helpers.  Included by ntm_kernels.hip and, for the N = 50
// specialisation, by ntm_n50.hip: a translation unit of its own so that its
// chunk loops can be built without unrolling (NTM_CHUNK_UNROLL) while the
// other horizons keep the compiler's choice.  Each group of P lanes runs the
// complete NTM_MPC_Sim.m:94-130 body for one scenario out of LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "ntm_device.h"

namespace {

using namespace ntm;

template <int P, class W>
__device__ __forceinline__ void load_state(const W& w, int64_t B, int64_t s, const double* rho,
                                           const double* U_old, int l) {
    const int N = w.n();
    const double* rs = rho + s * (3 * N);
    for (int e = l; e < 3 * N; e += P) w.rho()[e] = rs[e];
    if (l < N) w.Uold()[l] = U_old[s * N + l];
    NTM_WSYNC();
}

__device__ __forceinline__ bool is16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One scenario's record of n doubles from LDS to HBM.  With a 16-byte aligned
// destination and an even n, lanes store two doubles each (16-B stores: every
// request carries whole 16-B granules); otherwise one double per lane.
template <int P>
__device__ __forceinline__ void store_record(double* dst, const double* src, int n, int l) {
    if (is16(dst) && (n & 1) == 0) {
        for (int e = 2 * l; e < n; e += 2 * P)
            *reinterpret_cast<double2*>(dst + e) = make_double2(src[e], src[e + 1]);
    } else {
        for (int e = l; e < n; e += P) dst[e] = src[e];
    }
}

// XCD-aware block order (bijective): blocks are dealt round-robin over the 8
// XCDs, so block b is given the k-th slot of XCD b%8's contiguous range of
// scenario blocks.  Neighbouring scenarios share the cache lines at the ends
// of their (scenario-major) records; this keeps each line's users on one L2.
__device__ __forceinline__ int64_t xcd_swizzle(int64_t b, int64_t nb) {
    const int64_t q = nb >> 3, r = nb & 7, x = b & 7, k = b >> 3;
    return x * q + (x < r ? x : r) + k;
}

// Warm-start workspace (ntm_mpc_step_ws): the active sets of the previous
// step's last two QPs, 2 slots x (N ids + count) per scenario, in/out.  It is
// only a hint (every candidate is re-solved exactly and KKT-certified), but it
// comes from the caller, so each slot is validated before use: count in
// [0, N], ids in [0, rows), no repeats; anything else disables the slot.
// RUN (k_mpc_run_from): an empty set in mode 0 is kept, as qp_phase leaves it from one
// step of k_mpc_run to the next, so a chunk boundary does not change the path taken.
template <int P, class W, bool RUN = false>
__device__ __forceinline__ void load_candidates(const Prob& pb, const W& w, int64_t B, int64_t s, const int32_t* ws, int l) {
    const int N = w.n();
    const int nrows = StructRows(pb).rows();
    const int32_t* wss = ws + s * (2 * (N + 1));
    for (int e = l; e < 2 * (N + 1); e += P) w.cand()[e] = wss[e];
    for (int i = l; i < nrows; i += P) w.aflag()[i] = 0;
    NTM_WSYNC();
    for (int slot = 0; slot < 2; ++slot) {
        int* c = w.cand() + slot * (N + 1);
        const int q = uni<P>(c[N]);
        if (q < 0) continue;
        bool bad = q > N || nrows == 0;
        if constexpr (RUN) bad = q > N || (nrows == 0 && q > 0);
        if (!bad) {
            int lb = 0;
            if (l < q) lb = (c[l] < 0 || c[l] >= nrows) ? 1 : 0;
            // the DPP reduction on purpose here and below, not a gany ballot: see
            // StructRows::feasible_const (ntm_device.h) and DESIGN.md §10; a change is
            // checked by the byte-equal A/B of profiles/r07_ab/bitwise.txt
            bad = gmaxi<P>(lb) != 0;
        }
        if (!bad) {
            int lb = 0;
            for (int i = 0; i < q; ++i) {         // lane l < q checks its id against the earlier ones
                const int ci = c[i];
                if (l < q && i < l && ci == c[l]) lb = 1;
            }
            bad = gmaxi<P>(lb) != 0;
        }
        if (bad && l == 0) c[N] = -1;
        NTM_WSYNC();
    }
}

// 1: the rollout of a certified plan is the lifted prediction e + Gamma U (rollout_phase)
#ifndef NTM_ROLL_LIFTED
#define NTM_ROLL_LIFTED 1
#endif
// one MPC step on LDS-resident state; returns exit flag, sets *iters.
// DUAL (k_mpc_step_dual): rho_qp (this scenario's 3N record in HBM) receives the
// scheduling rho each QP is built from, so it ends as the last QP's; *q_last is that
// QP's active-row count (w.act(), multipliers by position in w.uu(): qp_phase)
template <int P, class W, bool DUAL = false>
__device__ __forceinline__ int mpc_step_dev(const Prob& pb, const W& w, double x0, double x1, int l, int* iters,
                            int64_t B = 0, int64_t s = 0, double* rho_qp = nullptr, int* q_last = nullptr) {
    int flag = NTM_EXIT_OPTIMAL, it;
    int n_qp = 0, n_gi = 0, n_act = 0, n_gen = 0, n_try = 0, n_girun = 0;
#ifdef NTM_STAMPS
    // exact 2-cycle study (diagnostic build): is the state after iteration it
    // (rho and U) bit-identical to the state after iteration it-2?  A necessary
    // condition for the LPV loop to repeat exactly from there on
    double cr[2][3] = {{0, 0, 0}, {0, 0, 0}}, cu[2] = {0, 0};
    int cyc = 0;
#endif
    for (it = 1; it <= pb.i_sim; ++it) {
        int qi = 0, qa = 0, ns = 0;
        bool yv = false;
        if constexpr (DUAL) {
            for (int e = l; e < 3 * w.n(); e += P) rho_qp[e] = w.rho()[e];
        }
        flag = qp_phase<P, W, DUAL>(pb, w, x0, x1, l, &qi, &qa, &ns, (it - 1) & 1, &n_try, &n_girun, it, &yv);
        if constexpr (DUAL) *q_last = qa;
        ++n_qp;
        n_gi += qi;
        n_act += qa;
        n_gen += ns;
        NTM_T0(tr);
        bool conv = rollout_phase<P>(pb, w, x0, x1, l, NTM_ROLL_LIFTED && yv);
        NTM_ACC(ST_ROLL, tr);
#ifdef NTM_STAMPS
        {
            double r0 = 0.0, r1 = 0.0, r2 = 0.0, u = 0.0;
            if (l < w.n()) { r0 = w.rho()[3 * l]; r1 = w.rho()[3 * l + 1]; r2 = w.rho()[3 * l + 2]; u = w.U()[l]; }
            const int sl = it & 1;
            int ne = (it < 3) || (l < w.n() && (r0 != cr[sl][0] || r1 != cr[sl][1] || r2 != cr[sl][2] || u != cu[sl]));
            ne = gmaxi<P>(ne);
            if (!ne && !cyc) {
                cyc = it;
                NTM_CNT(CN_CYC_HIT);
                if ((threadIdx.x & 63) == 0) ntm_lds_stamps[CN_CYC_SKIP] += (unsigned long long)(pb.i_sim - it);
            }
            cr[sl][0] = r0; cr[sl][1] = r1; cr[sl][2] = r2; cu[sl] = u;
        }
#endif
        if (conv) break;
    }
    *iters = it > pb.i_sim ? pb.i_sim : it;
    if (pb.stats && l == 0) {
        pb.stats[s] += n_qp;
        pb.stats[B + s] += n_gi;
        pb.stats[2 * B + s] += n_act;
        pb.stats[3 * B + s] += n_gen;
        pb.stats[4 * B + s] += n_try;
        pb.stats[5 * B + s] += n_girun;
    }
    return flag;
}

#ifndef NTM_HOT_WAVES_PER_EU
#define NTM_HOT_WAVES_PER_EU 2
#endif
#ifndef NTM_N20_WAVES_PER_EU
#define NTM_N20_WAVES_PER_EU (NTM_FAR_N20 ? 4 : 2)
#endif
// Long horizons (NN > 32): the LDS workspace already limits a CU to fewer waves
// than SIMDs, so the register budget of one wave per SIMD costs no occupancy and
// removes the spills of the fully unrolled horizon loops.  N = 20: three waves per
// SIMD (the far workspace fits 12 scenarios per CU); 168 VGPRs spill ~60 of them,
// and the third wave still wins (11.92 -> 11.03 ms per step-batch, A/B on one box).
// FAR = false at N = 20: the all-LDS build (2 waves per SIMD, 256 VGPRs), which
// runs each wave faster and is launched for batches that fill no more than its
// 8 scenarios per CU (small_batch in ntm_kernels.hip)
#define NTM_WAVES_PER_EU(NN, FAR) \
    ((NN) > 32 ? 1 : ((NN) == 20 && (FAR) ? NTM_N20_WAVES_PER_EU : NTM_HOT_WAVES_PER_EU))
// two scenarios per wave at N = 20 (far layout, 24 KB of LDS per wave): at most 6
// waves per CU fit, so the register budget of 2 waves per SIMD costs nothing
#define NTM_WAVES_PER_EU_P(P, NN, FAR) ((P) < 64 && (NN) == 20 ? 2 : NTM_WAVES_PER_EU(NN, FAR))
// NTM_STATIC_LDS=1: compile-time horizons with one scenario per wave keep their
// workspace in a static __shared__ array (the launch passes no dynamic LDS), so
// every workspace address is a constant the backend folds into the ds_read /
// ds_write offset field (the dynamic-LDS base is an opaque value: the layout's
// loop-invariant addresses are held in VGPRs and spilled).  It cuts the N = 20
// kernel's scratch from 88 to 56 B per lane, yet measured 0.6% slower (9.96 vs
// 9.90 ms per step-batch, A/B on one box), so it stays off
#ifndef NTM_STATIC_LDS
#define NTM_STATIC_LDS 0
#endif
template <int P, int NN>
__host__ __device__ constexpr bool static_lds() { return NTM_STATIC_LDS && P == 64 && NN > 0; }

// ---------------------------------------------------------------- the kernels' shared pieces
// The ten kernels below are siblings, not flags of one another (their argument blocks
// differ: DESIGN.md §4a); what they have in common is written once here.  How much can be
// an inline function is decided by the register allocator, not by taste: a piece stays a
// function only where every production instantiation of every kernel that uses it keeps its
// spill counts, scratch and occupancy (tools/asm_digest.sh --per-kernel, profiles/fold/).
// That holds for the prologue (all ten kernels) and for start_from_state (the three
// sibling step kernels and the two _from kernels).  The closed loops and the Rho = rho(x0)
// start change the allocation of their kernels even as functions holding the same
// statements, so they are shared as text: macros on the kernel's own names, expanded to the
// tokens each kernel had.  The step epilogues differ from kernel to kernel and stay there.

// Block and lane to group g, lane l and scenario s of the launch (s >= B: none, the caller
// returns).  The diagnostic builds' hooks sit here, so every kernel has them: the stamps
// (make diag; each kernel ends with NTM_STAMPS_FLUSH) and the traced scenario (make trace).
struct Lanes { int g, l; int64_t s; };
template <int P>
__device__ __forceinline__ Lanes scn_lanes() {
    constexpr int G = 64 / P;
    const int g = threadIdx.x / P, l = threadIdx.x % P;
    const int64_t s = xcd_swizzle(blockIdx.x, gridDim.x) * G + g;
    NTM_STAMPS_INIT();
    NTM_TRACE_SET(s, g, l);
    return {g, l, s};
}
// debug build (make poison): the workspace starts as NTM_POISON-valued doubles, so
// a read of LDS this launch never wrote shows up as a run-to-run difference
// (tools/determinism.py + compare_runs.py; this found the x_0-row read of rinfo[-1])
template <int P>
__device__ __forceinline__ void ws_poison(char* sbase, int bytes, int l) {
#ifdef NTM_POISON
    for (int e = l; e < bytes / 8; e += P) reinterpret_cast<double*>(sbase)[e] = NTM_POISON;
    NTM_WSYNC();
#endif
}
// Group g's workspace bytes: its slice of the launch's dynamic LDS, or the kernel's static
// array (static_lds).  Carved by ws_carve<NN, GEN, FAR> or, for the observer kernels, ws_carve_obs.
template <int P, int NN, bool FAR>
__device__ __forceinline__ char* scn_lds(int N, int g, int l) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sbase = smem + g * ws_bytes(N, FAR);
    if constexpr (static_lds<P, NN>()) {
        __shared__ __attribute__((aligned(16))) char smem_s[ws_bytes(NN > 0 ? NN : 1, FAR)];
        sbase = smem_s;
    }
    ws_poison<P>(sbase, ws_bytes(N, FAR), l);
    return sbase;
}

// A step from the caller's state: the candidate sets (null for a step kernel: none), rho, U_old
template <int P, bool RUN, class W>
__device__ __forceinline__ void start_from_state(const Prob& pb, const W& w, int64_t B, int64_t s, const double* rho,
                                                 const double* U_old, const int32_t* active_ws, int l) {
    if (RUN || active_ws) {
        load_candidates<P, W, RUN>(pb, w, B, s, active_ws, l);
    } else if (l < 2) {
        w.cand()[l * (w.n() + 1) + w.n()] = -1;
    }
    load_state<P>(w, B, s, rho, U_old, l);
}


// Closed-loop start, k_mpc_run / _run_obs / _run_est: Rho = repmat(rho(A0, A1), 1, N) from the
// model's coefficients K (NTM_MPC_Sim.m:63-65), Uold = +inf (D14).  Uses the kernel's w, N, l.
#define NTM_START_FROM_X0(K, A0, A1)                                                                                  \
    {   /* Rho = repmat(rho(x0), 1, N) (NTM_MPC_Sim.m:63-65); Uold = +inf (D14) */                                    \
        double r1, r2, r3;                                                                                            \
        rho_eval(K, A0, A1, r1, r2, r3);                                                                              \
        if (l < N) {                                                                                                  \
            w.rho()[3 * l] = r1;                                                                                      \
            w.rho()[3 * l + 1] = r2;                                                                                  \
            w.rho()[3 * l + 2] = r3;                                                                                  \
            w.Uold()[l] = kInf;                                                                                       \
        }                                                                                                             \
        NTM_WSYNC();                                                                                                  \
    }

// k_mpc_run's loop and k_mpc_run_from's, on the kernel's pb, w, N, B, s, l, k_sim, the state
// x0, x1 and the history arrays xk, uk, Uk, wpred, exitflag, inner_iters (each may be null).
// It leaves the workspace as the next step reads it and x0, x1 as the plant's state.
// s is int64_t, so every offset is formed in 64 bits.
#define NTM_RUN_LOOP                                                                                                  \
    if (xk && l == 0) { xk[s * 2 * (k_sim + 1)] = x0; xk[s * 2 * (k_sim + 1) + 1] = x1; }                             \
    for (int kk = 0; kk < k_sim; ++kk) {                                                                              \
        int its;                                                                                                      \
        int flag = mpc_step_dev<P>(pb, w, x0, x1, l, &its, B, s);                                                     \
        if (Uk && l < N) Uk[(s * k_sim + kk) * N + l] = w.U()[l];                                                     \
        if (wpred) for (int i = l; i <= N; i += P) wpred[(s * k_sim + kk) * (N + 1) + i] = w.xp()[2 * i];             \
        double n0, n1;                                                                                                \
        plant_step<true>(pb, scn_coef(pb, w), x0, x1, w.U()[0], n0, n1, pb.g.first_id + s, pb.g.k0 + kk);             \
        if (l == 0) {                                                                                                 \
            if (uk) uk[s * k_sim + kk] = w.U()[0];                                                                    \
            if (exitflag) exitflag[s * k_sim + kk] = flag;                                                            \
            if (inner_iters) inner_iters[s * k_sim + kk] = its;                                                       \
            if (xk) { xk[s * 2 * (k_sim + 1) + 2 * kk + 2] = n0; xk[s * 2 * (k_sim + 1) + 2 * kk + 3] = n1; }         \
        }                                                                                                             \
        x0 = n0;                                                                                                      \
        x1 = n1;                                                                                                      \
        NTM_WSYNC();                                                                                                  \
    }

template <int P, int NN, bool GEN, bool FAR = ws_far(NN)>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, NN, FAR)) void k_mpc_step(Prob pb, int64_t B, const double* __restrict__ x_k,
                                                 double* __restrict__ rho, double* __restrict__ U_old,
                                                 double* __restrict__ U, double* __restrict__ x_pred,
                                                 double* __restrict__ x_next, int32_t* __restrict__ exitflag,
                                                 int32_t* __restrict__ inner_iters, int32_t* __restrict__ active_ws) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = NN > 0 ? NN : pb.N;
    if (s >= B) return;
    // scn_lds' and start_from_state's text, kept here: this is the kernel the benchmark
    // times; inlined from start_from_state the production units allocate its registers
    // differently, and scn_lds changes what the single-TU builds inline into it
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sbase = smem + g * ws_bytes(N, FAR);
    if constexpr (static_lds<P, NN>()) {
        __shared__ __attribute__((aligned(16))) char smem_s[ws_bytes(NN > 0 ? NN : 1, FAR)];
        sbase = smem_s;
    }
    ws_poison<P>(sbase, ws_bytes(N, FAR), l);
    auto w = ws_carve<NN, GEN, FAR>(sbase, N, &pb, s);
    const double x0 = x_k[2 * s], x1 = x_k[2 * s + 1];
    if (active_ws) {
        load_candidates<P>(pb, w, B, s, active_ws, l);
    } else if (l < 2) {
        w.cand()[l * (N + 1) + N] = -1;
    }
    load_state<P>(w, B, s, rho, U_old, l);
    scn_store(pb, w, pb.g.first_id + s, l);           // this scenario's plasma (generator)
    NTM_WSYNC();
    int its;
    int flag = mpc_step_dev<P>(pb, w, x0, x1, l, &its, B, s);
    store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
    store_record<P>(U_old + s * N, w.Uold(), N, l);
    store_record<P>(U + s * N, w.U(), N, l);
    store_record<P>(x_pred + s * (2 * (N + 1)), w.xp(), 2 * (N + 1), l);
    {
        double n0, n1;
        plant_step<GEN>(pb, scn_coef(pb, w), x0, x1, w.U()[0], n0, n1, pb.g.first_id + s, pb.g.k0);
        if (is16(x_next)) {
            if (l == 0) *reinterpret_cast<double2*>(x_next + 2 * s) = make_double2(n0, n1);
        } else if (l < 2) {
            x_next[2 * s + l] = l ? n1 : n0;
        }
    }
    if (l == 0) {
        exitflag[s] = flag;
        inner_iters[s] = its;
    }
    if (active_ws)
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
    NTM_STAMPS_FLUSH();
}

// k_mpc_step<P, 0, true> (the runtime-N kernel, generator build) with the last QP's
// multipliers and scheduling rho exported (ntm_mpc_step_dual).  A sibling kernel and
// not a flag of k_mpc_step: two more kernel arguments on the template would change
// every existing instantiation's argument block.  lambda[rows(mode)] per scenario,
// quadprog's lambda.ineqlin by row id (mu_i / rn_i; zero on inactive rows and for
// every exit flag but 1).  After the last rollout the workspace still holds that
// QP's Gamma, scaling and row norms: the rollout updates rho and does not re-lift.
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_step_dual(
    Prob pb, int64_t B, const double* __restrict__ x_k, double* __restrict__ rho, double* __restrict__ U_old,
    double* __restrict__ U, double* __restrict__ x_pred, double* __restrict__ x_next, int32_t* __restrict__ exitflag,
    int32_t* __restrict__ inner_iters, int32_t* __restrict__ active_ws, double* __restrict__ lambda,
    double* __restrict__ rho_qp) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    auto w = ws_carve<0, true, false>(scn_lds<P, 0, false>(N, g, l), N, &pb, s);
    const double x0 = x_k[2 * s], x1 = x_k[2 * s + 1];
    start_from_state<P, false>(pb, w, B, s, rho, U_old, active_ws, l);
    scn_store(pb, w, pb.g.first_id + s, l);
    NTM_WSYNC();
    int its, q = 0;
    int flag = mpc_step_dev<P, decltype(w), true>(pb, w, x0, x1, l, &its, B, s, rho_qp + s * (3 * N), &q);
    {
        const StructRows rows(pb);
        const int nrows = rows.rows();
        double* ls = lambda + s * nrows;
        for (int i = l; i < nrows; i += P) {
            double v = 0.0;
            if (flag == NTM_EXIT_OPTIMAL)
                for (int a = 0; a < q; ++a)
                    if (w.act()[a] == i) v = w.uu()[a] / rows.rnorm(w, i);
            ls[i] = v;
        }
    }
    store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
    store_record<P>(U_old + s * N, w.Uold(), N, l);
    store_record<P>(U + s * N, w.U(), N, l);
    store_record<P>(x_pred + s * (2 * (N + 1)), w.xp(), 2 * (N + 1), l);
    {
        double n0, n1;
        plant_step<true>(pb, scn_coef(pb, w), x0, x1, w.U()[0], n0, n1, pb.g.first_id + s, pb.g.k0);
        if (l < 2) x_next[2 * s + l] = l ? n1 : n0;
    }
    if (l == 0) {
        exitflag[s] = flag;
        inner_iters[s] = its;
    }
    if (active_ws)
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
    NTM_STAMPS_FLUSH();
}

template <int P, int NN, bool FAR = ws_far(NN)>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, NN, FAR)) void k_mpc_run(Prob pb, int64_t B, int k_sim, const double* __restrict__ x0v,
                                                double* xk, double* uk, double* Uk, double* wpred,
                                                int32_t* exitflag, int32_t* inner_iters) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = NN > 0 ? NN : pb.N;
    if (s >= B) return;
    auto w = ws_carve<NN, true, FAR>(scn_lds<P, NN, FAR>(N, g, l), N, &pb, s);
    double x0 = x0v[2 * s], x1 = x0v[2 * s + 1];
    if (l < 2) w.cand()[l * (N + 1) + N] = -1;
    scn_store(pb, w, pb.g.first_id + s, l);           // this scenario's plasma (generator)
    NTM_WSYNC();
    NTM_START_FROM_X0(scn_coef(pb, w), x0, x1)
    NTM_RUN_LOOP
    NTM_STAMPS_FLUSH();
}

// k_mpc_run from a carried state and back to it (ntm_mpc_run_from): x[2], rho[3N],
// U_old[N] and active_ws[2(N+1)] per scenario, in/out, in ntm_mpc_step_ws's layouts.
// A sibling kernel and not a flag of k_mpc_run, for k_mpc_step_dual's reason: more
// kernel arguments on the template would change every existing instantiation's
// argument block.  It is k_mpc_run with k_mpc_step's start (start_from_state) and a
// write-back: what the next step would read from the workspace (rho, U_old, the two
// candidate sets) and the plant state go back to HBM after the last step.  k_sim = 0
// stores nothing but xk's column 0.
template <int P, int NN, bool FAR = ws_far(NN)>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, NN, FAR)) void k_mpc_run_from(
    Prob pb, int64_t B, int k_sim, double* __restrict__ x, double* __restrict__ rho, double* __restrict__ U_old,
    int32_t* __restrict__ active_ws, double* xk, double* uk, double* Uk, double* wpred, int32_t* exitflag,
    int32_t* inner_iters) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = NN > 0 ? NN : pb.N;
    if (s >= B) return;
    auto w = ws_carve<NN, true, FAR>(scn_lds<P, NN, FAR>(N, g, l), N, &pb, s);
    double x0 = x[2 * s], x1 = x[2 * s + 1];
    start_from_state<P, true>(pb, w, B, s, rho, U_old, active_ws, l);
    scn_store(pb, w, pb.g.first_id + s, l);           // this scenario's plasma (generator)
    NTM_WSYNC();
    NTM_RUN_LOOP
    if (k_sim > 0) {
        store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
        store_record<P>(U_old + s * N, w.Uold(), N, l);
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
        if (is16(x)) {
            if (l == 0) *reinterpret_cast<double2*>(x + 2 * s) = make_double2(x0, x1);
        } else if (l < 2) {
            x[2 * s + l] = l ? x1 : x0;
        }
    }
    NTM_STAMPS_FLUSH();
}

// Plant-model mismatch and the offset-free disturbance estimate (ntm_mpc_step_obs /
// ntm_mpc_run_obs).  Siblings of the runtime-N kernels, as k_mpc_step_dual is, and for
// its reason: the estimate and the options are kernel arguments, and the model's
// per-scenario coefficients are four more live values, neither of which the existing
// instantiations should pay for.  Every horizon runs here (N = 10, 20 and 50 included,
// like step_dual, Ru != 0 and mode 3 at N = 20).
//   model  k_m = (nominal ? the launch's plasma : the scenario's), C + d_hat: the lift
//          and the rollout of every LPV iteration (WSObs, scn_coef's overload);
//   plant  k_p = the scenario's plasma (a generator with a spread), else the launch's;
//          it never sees d_hat;
//   e      = x_next - (k_m's one-step map from rho(x_k) without d_hat, no disturbance);
//   d_hat <- obs_update(gain, e, d_hat).
// The carved workspace and the model of scenario s of the launch, d = its estimate
template <class W>
__device__ __forceinline__ void obs_model(W& w, const Coef& km, double d0, double d1) {
    w.mC1 = km.C1 + d0;
    w.mC2 = km.C2 + d1;
    w.mbc = km.bc;
    w.mwdep = km.wdep;
}
// The model's one-step map from rho(x_k), without the estimate and without a disturbance:
// plant_step's own expressions on the model's coefficients.  Its inputs pass through an
// empty asm first, so the compiler sees values unrelated to the plant step's: sharing
// rho1, rho2, a11 x0, ... between the two would change how the plant step's sums are
// fused into multiply-adds, and x_next would no longer be k_mpc_step_dual's bit for bit
__device__ __forceinline__ void model_step(const Prob& pb, const Coef& km, double x0, double x1, double u, double& m0,
                                           double& m1) {
    asm volatile("" : "+v"(x0), "+v"(x1), "+v"(u));
    plant_step<false>(pb, km, x0, x1, u, m0, m1);
}
__device__ __forceinline__ WSObs ws_carve_obs(char* base, int N) {
    WSObs w;
    w.N_rt = N;
    w.base = reinterpret_cast<double*>(base);
    w.far = nullptr;
    w.mC1 = w.mC2 = w.mbc = w.mwdep = 0.0;
    return w;
}

// k_mpc_run_est's loop and k_mpc_run_est_from's, as NTM_RUN_LOOP: also on the kernel's gid, kp,
// km, eo, the carried h0, h1 (x_hat), d0, d1 (d_hat) and the histories dk, xhk, yk
#define NTM_RUN_EST_LOOP                                                                                              \
    const int64_t xs = s * 2 * (int64_t)(k_sim + 1);                                                                  \
    if (xk && l == 0) { xk[xs] = x0; xk[xs + 1] = x1; }                                                               \
    if (dk && l == 0) { dk[xs] = d0; dk[xs + 1] = d1; }                                                               \
    if (xhk && l == 0) { xhk[xs] = h0; xhk[xs + 1] = h1; }                                                            \
    for (int kk = 0; kk < k_sim; ++kk) {                                                                              \
        int its;                                                                                                      \
        int flag = mpc_step_dev<P>(pb, w, h0, h1, l, &its, B, s);                                                     \
        if (Uk && l < N) Uk[(s * k_sim + kk) * N + l] = w.U()[l];                                                     \
        if (wpred) for (int i = l; i <= N; i += P) wpred[(s * k_sim + kk) * (N + 1) + i] = w.xp()[2 * i];             \
        const double u0 = w.U()[0];                                                                                   \
        double n0, n1, m0, m1;                                                                                        \
        plant_step<true>(pb, kp, x0, x1, u0, n0, n1, gid, pb.g.k0 + kk);                                              \
        model_step(pb, km, h0, h1, u0, m0, m1);                                                                       \
        const double y0 = est_measure(pb, eo.sy[0], n0, gid, pb.g.k0 + kk, 2);                                        \
        const double y1 = est_measure(pb, eo.sy[1], n1, gid, pb.g.k0 + kk, 3);                                        \
        est_update(eo.gain[0], eo.kappa[0], y0, m0, d0, h0);                                                          \
        est_update(eo.gain[1], eo.kappa[1], y1, m1, d1, h1);                                                          \
        if (l == 0) {                                                                                                 \
            if (uk) uk[s * k_sim + kk] = u0;                                                                          \
            if (exitflag) exitflag[s * k_sim + kk] = flag;                                                            \
            if (inner_iters) inner_iters[s * k_sim + kk] = its;                                                       \
            if (xk) { xk[xs + 2 * kk + 2] = n0; xk[xs + 2 * kk + 3] = n1; }                                           \
            if (dk) { dk[xs + 2 * kk + 2] = d0; dk[xs + 2 * kk + 3] = d1; }                                           \
            if (xhk) { xhk[xs + 2 * kk + 2] = h0; xhk[xs + 2 * kk + 3] = h1; }                                        \
            if (yk) { yk[(s * k_sim + kk) * 2] = y0; yk[(s * k_sim + kk) * 2 + 1] = y1; }                             \
        }                                                                                                             \
        x0 = n0;                                                                                                      \
        x1 = n1;                                                                                                      \
        NTM_WSYNC();                                                                                                  \
        obs_model(w, km, d0, d1);                                                                                     \
    }

template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_step_obs(
    Prob pb, int64_t B, const double* __restrict__ x_k, double* __restrict__ rho, double* __restrict__ U_old,
    double* __restrict__ U, double* __restrict__ x_pred, double* __restrict__ x_next, int32_t* __restrict__ exitflag,
    int32_t* __restrict__ inner_iters, int32_t* __restrict__ active_ws, double* __restrict__ d_hat, int nominal,
    double gain) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    const double x0 = x_k[2 * s], x1 = x_k[2 * s + 1];
    const double d0 = d_hat[2 * s], d1 = d_hat[2 * s + 1];
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    start_from_state<P, false>(pb, w, B, s, rho, U_old, active_ws, l);
    int its;
    int flag = mpc_step_dev<P>(pb, w, x0, x1, l, &its, B, s);
    store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
    store_record<P>(U_old + s * N, w.Uold(), N, l);
    store_record<P>(U + s * N, w.U(), N, l);
    store_record<P>(x_pred + s * (2 * (N + 1)), w.xp(), 2 * (N + 1), l);
    const double u0 = w.U()[0];
    double n0, n1, m0, m1;
    plant_step<true>(pb, kp, x0, x1, u0, n0, n1, gid, pb.g.k0);
    model_step(pb, km, x0, x1, u0, m0, m1);
    const double e0 = obs_update(gain, n0 - m0, d0), e1 = obs_update(gain, n1 - m1, d1);
    if (l < 2) {
        x_next[2 * s + l] = l ? n1 : n0;
        d_hat[2 * s + l] = l ? e1 : e0;
    }
    if (l == 0) {
        exitflag[s] = flag;
        inner_iters[s] = its;
    }
    if (active_ws)
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
    NTM_STAMPS_FLUSH();
}

// k_mpc_run<P, 0> with the estimate carried on chip: d0v (2 per scenario, null: zeros),
// dk (2(k_sim+1) per scenario, may be null): column 0 the initial estimate, column k+1
// the estimate after step k.  Rho = repmat(rho(x0)) comes from the model.
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_run_obs(
    Prob pb, int64_t B, int k_sim, const double* __restrict__ x0v, const double* __restrict__ d0v, double* xk,
    double* uk, double* Uk, double* wpred, double* dk, int32_t* exitflag, int32_t* inner_iters, int nominal,
    double gain) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    double x0 = x0v[2 * s], x1 = x0v[2 * s + 1];
    double d0 = d0v ? d0v[2 * s] : 0.0, d1 = d0v ? d0v[2 * s + 1] : 0.0;
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    if (l < 2) w.cand()[l * (N + 1) + N] = -1;
    NTM_START_FROM_X0(km, x0, x1)
    const int64_t xs = s * 2 * (int64_t)(k_sim + 1);
    if (xk && l == 0) { xk[xs] = x0; xk[xs + 1] = x1; }
    if (dk && l == 0) { dk[xs] = d0; dk[xs + 1] = d1; }
    for (int kk = 0; kk < k_sim; ++kk) {
        int its;
        int flag = mpc_step_dev<P>(pb, w, x0, x1, l, &its, B, s);
        if (Uk && l < N) Uk[(s * k_sim + kk) * N + l] = w.U()[l];
        if (wpred) for (int i = l; i <= N; i += P) wpred[(s * k_sim + kk) * (N + 1) + i] = w.xp()[2 * i];
        const double u0 = w.U()[0];
        double n0, n1, m0, m1;
        plant_step<true>(pb, kp, x0, x1, u0, n0, n1, gid, pb.g.k0 + kk);
        model_step(pb, km, x0, x1, u0, m0, m1);
        d0 = obs_update(gain, n0 - m0, d0);
        d1 = obs_update(gain, n1 - m1, d1);
        if (l == 0) {
            if (uk) uk[s * k_sim + kk] = u0;
            if (exitflag) exitflag[s * k_sim + kk] = flag;
            if (inner_iters) inner_iters[s * k_sim + kk] = its;
            if (xk) { xk[xs + 2 * kk + 2] = n0; xk[xs + 2 * kk + 3] = n1; }
            if (dk) { dk[xs + 2 * kk + 2] = d0; dk[xs + 2 * kk + 3] = d1; }
        }
        x0 = n0;
        x1 = n1;
        NTM_WSYNC();
        obs_model(w, km, d0, d1);
    }
    NTM_STAMPS_FLUSH();
}

// Output feedback (ntm_mpc_step_est / ntm_mpc_run_est): the observer kernels with a
// noisy measurement and a fixed-gain state filter.  Three values are carried per
// scenario: the plant's state x, the estimate x_hat and d_hat.
//   controller: the observer step (model k_m, C + d_hat) planned FROM x_hat;
//   plant  x_next = k_p's step at (x, U[0]) + disturbance; it never sees x_hat, d_hat
//          or the measurement noise;
//   y      = x_next + sy n(gid, k, 2 + i)                            (est_measure);
//   m      = k_m's one-step map at (x_hat, U[0]) from rho(x_hat), without d_hat;
//   d_hat, x_hat <- est_update(gain, kappa, y, m, ...).
// With sy = 0, kappa = 0, gain[0] == gain[1] and x_hat == x this is k_mpc_step_obs's
// step bit for bit (x_hat = y = x_next): the plant step and the model's map are the same
// calls on the same values (feedback_step), and model_step keeps them apart for the compiler.
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_step_est(
    Prob pb, int64_t B, const double* __restrict__ x_k, double* __restrict__ rho, double* __restrict__ U_old,
    double* __restrict__ U, double* __restrict__ x_pred, double* __restrict__ x_next, int32_t* __restrict__ exitflag,
    int32_t* __restrict__ inner_iters, int32_t* __restrict__ active_ws, double* __restrict__ d_hat,
    double* __restrict__ x_hat, double* __restrict__ y, EstOpt eo) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    const double x0 = x_k[2 * s], x1 = x_k[2 * s + 1];
    const double h0 = x_hat[2 * s], h1 = x_hat[2 * s + 1];
    double d0 = d_hat[2 * s], d1 = d_hat[2 * s + 1];
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    start_from_state<P, false>(pb, w, B, s, rho, U_old, active_ws, l);
    int its;
    int flag = mpc_step_dev<P>(pb, w, h0, h1, l, &its, B, s);
    store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
    store_record<P>(U_old + s * N, w.Uold(), N, l);
    store_record<P>(U + s * N, w.U(), N, l);
    store_record<P>(x_pred + s * (2 * (N + 1)), w.xp(), 2 * (N + 1), l);
    const double u0 = w.U()[0];
    double n0, n1, m0, m1, e0, e1;
    plant_step<true>(pb, kp, x0, x1, u0, n0, n1, gid, pb.g.k0);
    model_step(pb, km, h0, h1, u0, m0, m1);
    const double y0 = est_measure(pb, eo.sy[0], n0, gid, pb.g.k0, 2);
    const double y1 = est_measure(pb, eo.sy[1], n1, gid, pb.g.k0, 3);
    est_update(eo.gain[0], eo.kappa[0], y0, m0, d0, e0);
    est_update(eo.gain[1], eo.kappa[1], y1, m1, d1, e1);
    if (l < 2) {
        x_next[2 * s + l] = l ? n1 : n0;
        d_hat[2 * s + l] = l ? d1 : d0;
        x_hat[2 * s + l] = l ? e1 : e0;
        if (y) y[2 * s + l] = l ? y1 : y0;
    }
    if (l == 0) {
        exitflag[s] = flag;
        inner_iters[s] = its;
    }
    if (active_ws)
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
    NTM_STAMPS_FLUSH();
}

// k_mpc_run_obs with the measurement and the filter, x, x_hat and d_hat carried on chip:
// h0v (2 per scenario, null: x0), xhk (2(k_sim+1) per scenario, may be null): column 0
// the initial estimate, column k+1 the estimate after step k; yk (2 k_sim per scenario,
// may be null): the measurement of step k.  Rho = repmat(rho(x_hat0)) comes from the model.
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_run_est(
    Prob pb, int64_t B, int k_sim, const double* __restrict__ x0v, const double* __restrict__ d0v,
    const double* __restrict__ h0v, double* xk, double* uk, double* Uk, double* wpred, double* dk, double* xhk,
    double* yk, int32_t* exitflag, int32_t* inner_iters, EstOpt eo) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    double x0 = x0v[2 * s], x1 = x0v[2 * s + 1];
    double h0 = h0v ? h0v[2 * s] : x0, h1 = h0v ? h0v[2 * s + 1] : x1;
    double d0 = d0v ? d0v[2 * s] : 0.0, d1 = d0v ? d0v[2 * s + 1] : 0.0;
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    if (l < 2) w.cand()[l * (N + 1) + N] = -1;
    NTM_START_FROM_X0(km, h0, h1)
    NTM_RUN_EST_LOOP
    NTM_STAMPS_FLUSH();
}

// k_mpc_run_est from a carried state and back to it (ntm_mpc_run_est_from), the sibling
// k_mpc_run_from is of k_mpc_run, with the same two differences: x, rho, U_old,
// active_ws, d_hat[2] and x_hat[2] per scenario, in/out.  The model is built from the
// loaded d_hat.  With sy = 0, kappa = 0, equal gains and x_hat == x it continues k_mpc_run_obs.
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_run_est_from(
    Prob pb, int64_t B, int k_sim, double* __restrict__ x, double* __restrict__ rho, double* __restrict__ U_old,
    int32_t* __restrict__ active_ws, double* __restrict__ d_hat, double* __restrict__ x_hat, double* xk, double* uk,
    double* Uk, double* wpred, double* dk, double* xhk, double* yk, int32_t* exitflag, int32_t* inner_iters,
    EstOpt eo) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    double x0 = x[2 * s], x1 = x[2 * s + 1];
    double h0 = x_hat[2 * s], h1 = x_hat[2 * s + 1];
    double d0 = d_hat[2 * s], d1 = d_hat[2 * s + 1];
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    start_from_state<P, true>(pb, w, B, s, rho, U_old, active_ws, l);
    NTM_RUN_EST_LOOP
    if (k_sim > 0) {
        store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
        store_record<P>(U_old + s * N, w.Uold(), N, l);
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
        if (l < 2) {
            x[2 * s + l] = l ? x1 : x0;
            d_hat[2 * s + l] = l ? d1 : d0;
            x_hat[2 * s + l] = l ? h1 : h0;
        }
    }
    NTM_STAMPS_FLUSH();
}

// Actuator dead time (ntm_mpc_step_dly / ntm_mpc_run_dly / ntm_mpc_run_dly_from): the
// estimator kernels with the input commanded d = dl.steps steps ago reaching the plant,
// d in [0, NTM_MAX_DELAY].  One more carried value per scenario, the queue of pending
// inputs u_queue[d], oldest first; lane j < d of the scenario's own group holds entry j
// (d <= 8 <= P, so it never leaves the group's first DPP row; lanes >= d hold 0).
//   plan state z = x_hat; with dl.predict, z <- k_m's one-step map WITH d_hat (scn_coef of
//          the workspace: C + d_hat) at (z, u_queue[j]) from rho(z), j = 0 .. d-1;
//   controller: k_mpc_step_est's, from z; u_cmd = U[0];
//   u_app  = d > 0 ? u_queue[0] : u_cmd; plant, measurement and estimator are
//          k_mpc_step_est's with u_app in the place of U[0];
//   queue  u_queue[j] <- u_queue[j+1], u_queue[d-1] <- u_cmd.
// With d = 0 no lane holds an entry, z is x_hat and u_app is U[0]: the estimator kernels'
// steps, bit for bit.
struct DlyOpt {
    int steps, predict;
};
// scenario s's queue into its lanes (qv null: zeros, power off until the first command arrives)
__device__ __forceinline__ double dly_load(const double* qv, int64_t s, int d, int l) {
    return (qv && l < d) ? qv[s * d + l] : 0.0;
}
// One prediction step.  Its inputs pass through model_step's empty asm, for model_step's
// reason: sub-expressions shared with the plant step or the model's map would change how
// those are fused, and d = 0 would no longer be the estimator kernels' step bit for bit
__device__ __forceinline__ void dly_predict(const Prob& pb, const Coef& kd, double& z0, double& z1, double u) {
    double a0 = z0, a1 = z1;
    asm volatile("" : "+v"(a0), "+v"(a1), "+v"(u));
    plant_step<false>(pb, kd, a0, a1, u, z0, z1);
}
// the plan state: x_hat carried over the d inputs already under way
template <int P>
__device__ __forceinline__ void dly_plan(const Prob& pb, const WSObs& w, const DlyOpt& dl, double q, double& z0,
                                         double& z1) {
    if (!dl.predict) return;
    const Coef kd = scn_coef(pb, w);
    for (int j = 0; j < dl.steps; ++j) dly_predict(pb, kd, z0, z1, gbcast<P>(q, j));
}
// the input that reaches the plant now
template <int P>
__device__ __forceinline__ double dly_applied(const DlyOpt& dl, double q, double u_cmd) {
    const double head = gbcast<P>(q, 0);
    return dl.steps > 0 ? head : u_cmd;
}
// Entry j takes entry j + 1's value, the last one the new command.  row_shl:1 moves every
// lane's value one lane down inside its row of 16; groups start at multiples of 16 and
// d <= 8, so what lanes 0 .. d-2 receive comes from their own group
__device__ __forceinline__ double dly_shift(const DlyOpt& dl, double q, double u_cmd, int l) {
    static_assert(NTM_MAX_DELAY < 16, "the queue must fit one DPP row");
    const double up = dpp_d<0x101>(q);
    return l + 1 < dl.steps ? up : (l + 1 == dl.steps ? u_cmd : 0.0);
}

// NTM_RUN_EST_LOOP with the dead time: also on the kernel's dl, the queue q and the
// histories uak (applied input) and xpk (plan state); uk stays the commanded U[0]
#define NTM_RUN_DLY_LOOP                                                                                              \
    const int64_t xs = s * 2 * (int64_t)(k_sim + 1);                                                                  \
    if (xk && l == 0) { xk[xs] = x0; xk[xs + 1] = x1; }                                                               \
    if (dk && l == 0) { dk[xs] = d0; dk[xs + 1] = d1; }                                                               \
    if (xhk && l == 0) { xhk[xs] = h0; xhk[xs + 1] = h1; }                                                            \
    for (int kk = 0; kk < k_sim; ++kk) {                                                                              \
        int its;                                                                                                      \
        double z0 = h0, z1 = h1;                                                                                      \
        dly_plan<P>(pb, w, dl, q, z0, z1);                                                                            \
        int flag = mpc_step_dev<P>(pb, w, z0, z1, l, &its, B, s);                                                     \
        if (Uk && l < N) Uk[(s * k_sim + kk) * N + l] = w.U()[l];                                                     \
        if (wpred) for (int i = l; i <= N; i += P) wpred[(s * k_sim + kk) * (N + 1) + i] = w.xp()[2 * i];             \
        const double u0 = w.U()[0];                                                                                   \
        const double ua = dly_applied<P>(dl, q, u0);                                                                  \
        double n0, n1, m0, m1;                                                                                        \
        plant_step<true>(pb, kp, x0, x1, ua, n0, n1, gid, pb.g.k0 + kk);                                              \
        model_step(pb, km, h0, h1, ua, m0, m1);                                                                       \
        const double y0 = est_measure(pb, eo.sy[0], n0, gid, pb.g.k0 + kk, 2);                                        \
        const double y1 = est_measure(pb, eo.sy[1], n1, gid, pb.g.k0 + kk, 3);                                        \
        est_update(eo.gain[0], eo.kappa[0], y0, m0, d0, h0);                                                          \
        est_update(eo.gain[1], eo.kappa[1], y1, m1, d1, h1);                                                          \
        q = dly_shift(dl, q, u0, l);                                                                                  \
        if (l == 0) {                                                                                                 \
            if (uk) uk[s * k_sim + kk] = u0;                                                                          \
            if (uak) uak[s * k_sim + kk] = ua;                                                                        \
            if (xpk) { xpk[(s * k_sim + kk) * 2] = z0; xpk[(s * k_sim + kk) * 2 + 1] = z1; }                          \
            if (exitflag) exitflag[s * k_sim + kk] = flag;                                                            \
            if (inner_iters) inner_iters[s * k_sim + kk] = its;                                                       \
            if (xk) { xk[xs + 2 * kk + 2] = n0; xk[xs + 2 * kk + 3] = n1; }                                           \
            if (dk) { dk[xs + 2 * kk + 2] = d0; dk[xs + 2 * kk + 3] = d1; }                                           \
            if (xhk) { xhk[xs + 2 * kk + 2] = h0; xhk[xs + 2 * kk + 3] = h1; }                                        \
            if (yk) { yk[(s * k_sim + kk) * 2] = y0; yk[(s * k_sim + kk) * 2 + 1] = y1; }                             \
        }                                                                                                             \
        x0 = n0;                                                                                                      \
        x1 = n1;                                                                                                      \
        NTM_WSYNC();                                                                                                  \
        obs_model(w, km, d0, d1);                                                                                     \
    }

// k_mpc_step_est with the dead time: u_queue (d per scenario, in/out; not read when
// d == 0), x_plan (2 per scenario, may be null): the z the plan was made from, u_applied
// (one per scenario, may be null)
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_step_dly(
    Prob pb, int64_t B, const double* __restrict__ x_k, double* __restrict__ rho, double* __restrict__ U_old,
    double* __restrict__ U, double* __restrict__ x_pred, double* __restrict__ x_next, int32_t* __restrict__ exitflag,
    int32_t* __restrict__ inner_iters, int32_t* __restrict__ active_ws, double* __restrict__ d_hat,
    double* __restrict__ x_hat, double* __restrict__ y, EstOpt eo, DlyOpt dl, double* __restrict__ u_queue,
    double* __restrict__ x_plan, double* __restrict__ u_applied) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    const double x0 = x_k[2 * s], x1 = x_k[2 * s + 1];
    const double h0 = x_hat[2 * s], h1 = x_hat[2 * s + 1];
    double d0 = d_hat[2 * s], d1 = d_hat[2 * s + 1];
    double q = dly_load(u_queue, s, dl.steps, l);
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    start_from_state<P, false>(pb, w, B, s, rho, U_old, active_ws, l);
    int its;
    double z0 = h0, z1 = h1;
    dly_plan<P>(pb, w, dl, q, z0, z1);
    int flag = mpc_step_dev<P>(pb, w, z0, z1, l, &its, B, s);
    store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
    store_record<P>(U_old + s * N, w.Uold(), N, l);
    store_record<P>(U + s * N, w.U(), N, l);
    store_record<P>(x_pred + s * (2 * (N + 1)), w.xp(), 2 * (N + 1), l);
    const double u0 = w.U()[0];
    const double ua = dly_applied<P>(dl, q, u0);
    double n0, n1, m0, m1, e0, e1;
    plant_step<true>(pb, kp, x0, x1, ua, n0, n1, gid, pb.g.k0);
    model_step(pb, km, h0, h1, ua, m0, m1);
    const double y0 = est_measure(pb, eo.sy[0], n0, gid, pb.g.k0, 2);
    const double y1 = est_measure(pb, eo.sy[1], n1, gid, pb.g.k0, 3);
    est_update(eo.gain[0], eo.kappa[0], y0, m0, d0, e0);
    est_update(eo.gain[1], eo.kappa[1], y1, m1, d1, e1);
    q = dly_shift(dl, q, u0, l);
    if (l < dl.steps) u_queue[s * dl.steps + l] = q;
    if (l < 2) {
        x_next[2 * s + l] = l ? n1 : n0;
        d_hat[2 * s + l] = l ? d1 : d0;
        x_hat[2 * s + l] = l ? e1 : e0;
        if (y) y[2 * s + l] = l ? y1 : y0;
        if (x_plan) x_plan[2 * s + l] = l ? z1 : z0;
    }
    if (l == 0) {
        exitflag[s] = flag;
        inner_iters[s] = its;
        if (u_applied) u_applied[s] = ua;
    }
    if (active_ws)
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
    NTM_STAMPS_FLUSH();
}

// k_mpc_run_est with the dead time, the queue carried in the lanes for the whole loop:
// uq0 (d per scenario, null: zeros), uak (k_sim per scenario, may be null): the applied
// input of step k, xpk (2 k_sim per scenario, may be null): the plan state of step k
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_run_dly(
    Prob pb, int64_t B, int k_sim, const double* __restrict__ x0v, const double* __restrict__ d0v,
    const double* __restrict__ h0v, const double* __restrict__ uq0, double* xk, double* uk, double* Uk, double* wpred,
    double* dk, double* xhk, double* yk, double* uak, double* xpk, int32_t* exitflag, int32_t* inner_iters, EstOpt eo,
    DlyOpt dl) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    double x0 = x0v[2 * s], x1 = x0v[2 * s + 1];
    double h0 = h0v ? h0v[2 * s] : x0, h1 = h0v ? h0v[2 * s + 1] : x1;
    double d0 = d0v ? d0v[2 * s] : 0.0, d1 = d0v ? d0v[2 * s + 1] : 0.0;
    double q = dly_load(uq0, s, dl.steps, l);
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    if (l < 2) w.cand()[l * (N + 1) + N] = -1;
    NTM_START_FROM_X0(km, h0, h1)
    NTM_RUN_DLY_LOOP
    NTM_STAMPS_FLUSH();
}

// k_mpc_run_est_from with the dead time: u_queue (d per scenario) in/out with the rest of
// the carried state, so a loop split into chunks carries the inputs still under way
template <int P>
__global__ __launch_bounds__(64, NTM_WAVES_PER_EU_P(P, 0, false)) void k_mpc_run_dly_from(
    Prob pb, int64_t B, int k_sim, double* __restrict__ x, double* __restrict__ rho, double* __restrict__ U_old,
    int32_t* __restrict__ active_ws, double* __restrict__ d_hat, double* __restrict__ x_hat,
    double* __restrict__ u_queue, double* xk, double* uk, double* Uk, double* wpred, double* dk, double* xhk,
    double* yk, double* uak, double* xpk, int32_t* exitflag, int32_t* inner_iters, EstOpt eo, DlyOpt dl) {
    const auto [g, l, s] = scn_lanes<P>();
    const int N = pb.N;
    if (s >= B) return;
    WSObs w = ws_carve_obs(scn_lds<P, 0, false>(N, g, l), N);
    double x0 = x[2 * s], x1 = x[2 * s + 1];
    double h0 = x_hat[2 * s], h1 = x_hat[2 * s + 1];
    double d0 = d_hat[2 * s], d1 = d_hat[2 * s + 1];
    double q = dly_load(u_queue, s, dl.steps, l);
    const int64_t gid = pb.g.first_id + s;
    const Coef kp = plant_coef(pb, gid);
    const Coef km = eo.nominal ? pb.k : kp;
    obs_model(w, km, d0, d1);
    start_from_state<P, true>(pb, w, B, s, rho, U_old, active_ws, l);
    NTM_RUN_DLY_LOOP
    if (k_sim > 0) {
        store_record<P>(rho + s * (3 * N), w.rho(), 3 * N, l);
        store_record<P>(U_old + s * N, w.Uold(), N, l);
        for (int e = l; e < 2 * (N + 1); e += P) active_ws[s * (2 * (N + 1)) + e] = w.cand()[e];
        if (l < 2) {
            x[2 * s + l] = l ? x1 : x0;
            d_hat[2 * s + l] = l ? d1 : d0;
            x_hat[2 * s + l] = l ? h1 : h0;
        }
        if (l < dl.steps) u_queue[s * dl.steps + l] = q;
    }
    NTM_STAMPS_FLUSH();
}

}  // namespace

// The launchers of the hot kernels of one (lanes, horizon, layout): k_mpc_step (the
// generator's build only when the generator is used), k_mpc_run and k_mpc_run_from.
// The generic horizons instantiate them in ntm_kernels.hip; a specialised horizon's are
// instantiated by the translation unit that owns it (ntm_n20.hip, ntm_n50.hip, ...: each
// sets its own LDS batch size) and reached through that unit's ntm_launch_<name>.
// Internal linkage: two translation units that build the same horizon with
// different settings (ntm_n50.hip and ntm_n50m3.hip) instantiate these templates
// with the same arguments, and external (COMDAT) instances would be folded into
// one of the two builds at link time
enum class Hot { step, run, run_from };
// the kernel arguments after (pb, B) of whichever of the three is launched
struct HotArgs {
    int k_sim;                                               // run, run_from
    const double* x_in;                                      // step: x_k; run: x0
    double *x, *rho, *U_old;                                 // step, run_from (x: run_from)
    double *U, *x_pred, *x_next;                             // step
    double *xk, *uk, *Uk, *wpred;                            // run, run_from
    int32_t *exitflag, *inner_iters, *active_ws;
};
namespace {
// a build without rate rows (rate_rows in ntm_ws.h) must never see mode 3: the host's
// dispatch sends it to the runtime-N kernels, and this keeps that explicit
template <int NN, bool FAR>
bool ntm_mode_built(const ntm::Prob& pb) {
    return ntm::rate_rows<ntm::WS<NN, false, FAR>>() || pb.mode != NTM_MODE_FULL_DU;
}
// the > 64 KiB opt-in, an empty batch, the launch: blocks of 64 / P scenarios
template <int P, int NN, typename K, typename... A>
hipError_t ntm_launch_k(K kern, int64_t B, size_t lds, hipStream_t st, A... args) {
    constexpr int G = 64 / P;
    if (static_lds<P, NN>()) lds = 0;                  // the workspace is the kernel's static LDS
    if (lds > 64 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int64_t blocks = (B + G - 1) / G;
    if (blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64), lds, st, args...);
    return hipGetLastError();
}
template <int P, int NN, bool FAR>
hipError_t ntm_launch_hot(Hot what, const ntm::Prob& pb, int64_t B, const HotArgs& a, size_t lds, hipStream_t st) {
    if (!ntm_mode_built<NN, FAR>(pb)) return hipErrorInvalidValue;
    switch (what) {
    case Hot::step:
        if (pb.g.phys_on || pb.g.dist_on)
            return ntm_launch_k<P, NN>(k_mpc_step<P, NN, true, FAR>, B, lds, st, pb, B, a.x_in, a.rho, a.U_old, a.U,
                                       a.x_pred, a.x_next, a.exitflag, a.inner_iters, a.active_ws);
        return ntm_launch_k<P, NN>(k_mpc_step<P, NN, false, FAR>, B, lds, st, pb, B, a.x_in, a.rho, a.U_old, a.U,
                                   a.x_pred, a.x_next, a.exitflag, a.inner_iters, a.active_ws);
    case Hot::run:
        return ntm_launch_k<P, NN>(k_mpc_run<P, NN, FAR>, B, lds, st, pb, B, a.k_sim, a.x_in, a.xk, a.uk, a.Uk,
                                   a.wpred, a.exitflag, a.inner_iters);
    case Hot::run_from:
        return ntm_launch_k<P, NN>(k_mpc_run_from<P, NN, FAR>, B, lds, st, pb, B, a.k_sim, a.x, a.rho, a.U_old,
                                   a.active_ws, a.xk, a.uk, a.Uk, a.wpred, a.exitflag, a.inner_iters);
    }
    return hipErrorInvalidValue;
}
}  // namespace
// One translation unit per (horizon, layout): ntm_n20.hip (far), ntm_n20near.hip (the
// all-LDS N = 20 build for small batches, its own batch settings), ntm_n20near1w.hip (the
// same with a one-wave register budget), ntm_n50.hip (far, modes 0-2) and ntm_n50m3.hip
// (far, input-rate rows: mode 3).  One wave per scenario: lds bytes per block
typedef hipError_t ntm_layout_launcher(Hot what, const ntm::Prob& pb, int64_t B, const HotArgs& a, size_t lds,
                                       hipStream_t st);
#define NTM_DEFINE_LAYOUT_LAUNCHER(NAME, NNV, FARV)                                                         \
    hipError_t ntm_launch_##NAME(Hot what, const ntm::Prob& pb, int64_t B, const HotArgs& a, size_t lds,    \
                                 hipStream_t st) {                                                          \
        return ntm_launch_hot<64, NNV, FARV>(what, pb, B, a, lds, st);                                      \
    }
ntm_layout_launcher ntm_launch_n20, ntm_launch_n20near, ntm_launch_n20near1w, ntm_launch_n50, ntm_launch_n50m3;
