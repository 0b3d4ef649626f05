// ntm_lift.h — the lifted prediction: Gamma, Phi and Lambda of one scenario from its
// scheduling trajectory (lift_literal, lift_phase) and the free response e = Phi x_k + Lambda.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ntm_mpc.h"

#include "ntm_base.h"
#include "ntm_collectives.h"
#include "ntm_diag.h"
#include "ntm_lanes.h"
#include "ntm_prob.h"
#include "ntm_ws.h"

namespace ntm {

// ---------------------------------------------------------------------------
// L2: lifted prediction  (Rho_to_PhiGammaLambda.m:17-52, CANON D4/D6)
// ---------------------------------------------------------------------------
// Literal-reference lift (D4 / D6; generic kernels only, the host dispatches any
// launch that sets these flags there): D6 takes A(rho_{i-j}) for Gamma_ij, i.e.
// the coefficient index i - j - 1 counted from 0 (Rho_to_PhiGammaLambda.m:32);
// D4 right-multiplies Phi_i = Phi_{i-1} A_i (:21).  Same arithmetic as
// oracle/ntm_oracle.c orc_lift.  Lane j < N runs Gamma's column j; lane 0 then
// runs Phi and Lambda.  Kept apart from lift_phase so that the specialised hot
// kernels compile exactly as before (folding the switches into lift_phase cost
// the N=20 kernel 72 B of scratch per lane although they are constant there).
template <int P, class W>
__device__ __forceinline__ void lift_literal(const Prob& pb, const W& w, const Coef& k, int l) {
    const int N = w.n();
    const bool d6 = (pb.flags & NTM_LITERAL_GAMMA_INDEX) != 0, d4 = (pb.flags & NTM_LITERAL_PHI_RIGHTMUL) != 0;
    for (int j = l; j < N; j += P) {
        double* col = w.Gt() + w.gidx(2 * j, j) - 2 * j;
        double g0 = w.bb()[j], g1 = 0.0;
        col[2 * j] = g0;
        col[2 * j + 1] = g1;
        for (int i = j + 1; i < N; ++i) {
            const int ai = d6 ? i - j - 1 : i;
            const double n0 = w.a11()[ai] * g0;
            const double n1 = w.a21()[ai] * g0 + k.a22 * g1;
            g0 = n0;
            g1 = n1;
            col[2 * i] = g0;
            col[2 * i + 1] = g1;
        }
    }
    if (l == 0) {
        double p00 = w.a11()[0], p10 = w.a21()[0], p01 = 0.0, p11 = k.a22;
        double l0 = k.C1, l1 = k.C2;
        w.Phi()[0] = p00; w.Phi()[1] = p10; w.Phi()[2] = p01; w.Phi()[3] = p11;
        w.Lam()[0] = l0; w.Lam()[1] = l1;
        for (int i = 1; i < N; ++i) {
            const double a11 = w.a11()[i], a21 = w.a21()[i];
            double q00, q01, q10, q11;
            if (d4) {                                  // Phi_{i-1} A_i
                q00 = p00 * a11 + p01 * a21;
                q01 = p01 * k.a22;
                q10 = p10 * a11 + p11 * a21;
                q11 = p11 * k.a22;
            } else {                                   // A_i Phi_{i-1}
                q00 = a11 * p00;
                q01 = a11 * p01;
                q10 = a21 * p00 + k.a22 * p10;
                q11 = a21 * p01 + k.a22 * p11;
            }
            p00 = q00; p01 = q01; p10 = q10; p11 = q11;
            const double m0 = a11 * l0 + k.C1;
            const double m1 = (a21 * l0 + k.a22 * l1) + k.C2;
            l0 = m0; l1 = m1;
            w.Phi()[4 * i] = p00; w.Phi()[4 * i + 1] = p10; w.Phi()[4 * i + 2] = p01; w.Phi()[4 * i + 3] = p11;
            w.Lam()[2 * i] = l0; w.Lam()[2 * i + 1] = l1;
        }
    }
    NTM_WSYNC();
}

// The scaling pass's column sums, accumulated by the slim lift at long horizons:
// lane l < N walks Gamma's column l stage by stage, so it can add G_ll's and F_l's
// terms as it produces them (the free response e_i is lane N's value at the same
// stage, read by readlane), instead of the scaling pass reading the column back
// from LDS.  Same terms in the same order as the pass (diag_scale_phase).  Round 6,
// A/B on one box: config 5 mode 2 73.9 -> 70.9 ms per step-batch; the far N = 20
// kernel 6.31 -> 6.50 ms (its register allocation again) and the all-LDS one (config
// 2 0.193 -> 0.210 ms: e_i takes six lane reads there), so N = 50 only.
struct ColSums {
    double s = 0.0, f = 0.0;   // sum_i Gamma_il' Om Gamma_il and sum_i Gamma_il' Om (e_i - r)
    int bad = 0;               // a non-finite Gamma entry
};
template <class W>
__device__ __forceinline__ constexpr bool fuse_colsum() {
    if constexpr (W::kSlim) return W::kNN > 32;   // N = 50: on; the far N = 20 kernel: off
    else return false;                            // the all-LDS N = 20 build and the generic kernels: off
}
// The slim far N = 20 lift runs its recursion lane-masked (lift_chunk_lanes): column l on
// lane l, a11 / a21 in LDS, chunks of five stages, no column sums riding on the loop
template <int P, int CH, class W>
__device__ __forceinline__ constexpr bool lift_lanes_ok() {
    if constexpr (W::kSlim) return lane_masked_ok<P, CH, W>() && W::kAB != 0 && !fuse_colsum<W>();
    else return false;
}
// chunk I0 of the lane-masked lift: the a11 / a21 loads batched at compile-time offsets, then the stages
template <int I0, int NS, class W>
__device__ __forceinline__ void lift_chunk_at(const W& w, double& g0, double& g1, double a22, double c0, double c1,
                                              unsigned rec) {
    double ca[5], cb[5];
    if constexpr (W::kPair && NS == 5) {                  // a11 / a21 are 16-byte aligned (ws_pair_aligned)
        ld5<I0, true>(w.a11(), ca);
        ld5<I0, true>(w.a21(), cb);
    } else if constexpr (W::kPair && I0 % 2 == 0) {       // the last chunk: stages 16..19, two aligned pairs
        const dpair a0 = ld_pair<true>(w.a11() + I0), a1 = ld_pair<true>(w.a11() + I0 + 2);
        const dpair b0 = ld_pair<true>(w.a21() + I0), b1 = ld_pair<true>(w.a21() + I0 + 2);
        ca[0] = a0.x; ca[1] = a0.y; ca[2] = a1.x; ca[3] = a1.y; ca[4] = 0.0;
        cb[0] = b0.x; cb[1] = b0.y; cb[2] = b1.x; cb[3] = b1.y; cb[4] = 0.0;
    } else {
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            ca[u] = u < NS ? w.a11()[I0 + u] : 0.0;
            cb[u] = u < NS ? w.a21()[I0 + u] : 0.0;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    lift_chunk_lanes<I0, NS>(g0, g1, ca, cb, a22, c0, c1, rec);
}

template <int P, class W>
__device__ __forceinline__ void lift_phase(const Prob& pb, const W& w, int l, double x0 = 0.0, double x1 = 0.0,
                                           ColSums* cs = nullptr) {
    const int N = w.n();
    const Coef k = scn_coef(pb, w);
    if constexpr (W::kSlim) {
        // lane l < N keeps stage l's A/B coefficients in registers; the loop takes
        // stage i's by readlane.  Lanes < N: Gamma columns (as below); lane N: the
        // free response e = Phi x_k + Lambda as its own recursion e_i = A_i e_{i-1} + C
        // with e_{-1} = x_k (CANON D4: Phi_i = A_i Phi_{i-1}; the same states as
        // Phi x_k + Lambda to rounding), written straight to w.e()
        double ra = 0.0, rc = 0.0, rbb = 0.0;
        if (l < N) {
            ra = coef_a11(k, w.rho()[3 * l]);
            rc = coef_a21(k, w.rho()[3 * l + 1]);
            rbb = coef_b(k, w.rho()[3 * l + 2]);
            // (WS::kBox: these 2N doubles held the last QP's vlo / vhi until here; they are the
            // lift's to the end of its recursion below, then the scaling pass's again)
            if constexpr (W::kAB) { w.a11()[l] = ra; w.a21()[l] = rc; }
        }
        if constexpr (W::kAB) NTM_WSYNC();
        const double a0 = gbcast<P>(ra, 0), c0v = gbcast<P>(rc, 0);
        NTM_T0(tlf);
        if (l <= N) {
            const bool gam = l < N;
            double g0 = gam ? rbb : (a0 * x0 + k.C1);
            double g1 = gam ? 0.0 : ((c0v * x0 + k.a22 * x1) + k.C2);
            const double c0 = gam ? 0.0 : k.C1, c1 = gam ? 0.0 : k.C2;
            double* const rec = gam ? w.Gt() + w.gidx(2 * l, l) - 2 * l : w.e();
            rec[2 * (gam ? l : 0)] = g0;
            rec[2 * (gam ? l : 0) + 1] = g1;
            // stage i's terms of the column sums (lane N holds e_i): the scaling pass's
            // and free_response's expressions
            double cs_s = 0.0, cs_f = 0.0;
            int cs_bad = 0;
            const OmQ<qi_on<W>()> cq(pb.Q);
            auto col_terms = [&](int i) {
                if constexpr (fuse_colsum<W>()) {
                    const double e0 = gbcast<P>(g0, N), e1 = gbcast<P>(g1, N);
                    const double d0 = e0 - pb.r[0], d1 = e1 - pb.r[1];
                    const double ea = cq.o0(d0, d1), eb = cq.o1(d0, d1);
                    const double o0 = cq.o0(g0, g1), o1 = cq.o1(g0, g1);
                    const double t = g0 * o0 + g1 * o1;
                    const double tf = g0 * ea + g1 * eb;
                    const bool on = gam && i >= l;
                    if (on) cs_bad |= !isfinite(g0) || !isfinite(g1);
                    cs_s += on ? t : 0.0;
                    cs_f += on ? tf : 0.0;
                }
            };
            col_terms(0);
            constexpr int CH = NTM_CH;
            if constexpr (lift_lanes_ok<P, CH, W>()) {
                // stages 1..19 under EXEC narrowed to the lanes that advance (lift_chunk_lanes)
                const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)rec;
                lift_chunk_at<1, 5>(w, g0, g1, k.a22, c0, c1, at);
                lift_chunk_at<6, 5>(w, g0, g1, k.a22, c0, c1, at);
                lift_chunk_at<11, 5>(w, g0, g1, k.a22, c0, c1, at);
                lift_chunk_at<16, 4>(w, g0, g1, k.a22, c0, c1, at);
            } else {
            NTM_CHUNK_PRAGMA
            for (int i0 = 1; i0 < N; i0 += CH) {
                double ca[CH], cb[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int i = i0 + u;
                    if constexpr (W::kAB) {
                        ca[u] = i < N ? w.a11()[i] : 0.0;
                        cb[u] = i < N ? w.a21()[i] : 0.0;
                    } else {
                        ca[u] = i < N ? gbcast<P>(ra, i) : 0.0;
                        cb[u] = i < N ? gbcast<P>(rc, i) : 0.0;
                    }
                }
                if constexpr (W::kAB) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int i = i0 + u;
                    if (i < N) {
                        const double n0 = ca[u] * g0 + c0;
                        const double n1 = (cb[u] * g0 + k.a22 * g1) + c1;
                        const bool live = !gam || i > l;
                        g0 = live ? n0 : g0;
                        g1 = live ? n1 : g1;
                        const int at = live ? i : l;
                        rec[2 * at] = g0;
                        rec[2 * at + 1] = g1;
                        col_terms(i);
                    }
                }
            }
            }
            if (cs) { cs->s = cs_s; cs->f = cs_f; cs->bad = cs_bad; }
        }
        NTM_ACC(ST_L_LOOP, tlf);
        NTM_WSYNC();
        return;
    } else {
    if (l < N) {
        w.a11()[l] = coef_a11(k, w.rho()[3 * l]);
        w.a21()[l] = coef_a21(k, w.rho()[3 * l + 1]);
        w.bb()[l] = coef_b(k, w.rho()[3 * l + 2]);
    }
    NTM_WSYNC();
    if constexpr (W::kNN == 0) {
        if (pb.flags & (NTM_LITERAL_PHI_RIGHTMUL | NTM_LITERAL_GAMMA_INDEX)) {
            lift_literal<P>(pb, w, k, l);
            return;
        }
    }
    NTM_T0(tlf);
    // Gamma: lane j owns column j: Gamma_jj = B_j, Gamma_ij = A_i Gamma_{i-1,j} (D6).
    // Lanes N and N+1 run the same 2-vector recursion for the two columns of
    // Phi_i = A_i Phi_{i-1} (D4), lane N+2 for Lambda_i = A_i Lambda_{i-1} + C,
    // all in the one loop (the group has the idle lanes for N + 3 <= P).
    const bool extra = N + 3 <= P;
    if (l < N || (extra && l < N + 3)) {
        const bool gam = l < N;
        const int ph = l - N;                          // 0, 1: Phi column; 2: Lambda
        double g0, g1;
        if (gam) { g0 = w.bb()[l]; g1 = 0.0; }
        else if (ph == 0) { g0 = w.a11()[0]; g1 = w.a21()[0]; }
        else if (ph == 1) { g0 = 0.0; g1 = k.a22; }
        else { g0 = k.C1; g1 = k.C2; }
        const double c0 = (ph == 2) ? k.C1 : 0.0, c1 = (ph == 2) ? k.C2 : 0.0;
        // this lane's record, stage i at rec[st i]: its Gamma column (col[r], r >= 2l),
        // its Phi column (stride 4) or Lambda; one address for the three kinds of
        // lanes, so every step is one pair of stores with no divergent branches
        double* const rec = gam ? w.Gt() + w.gidx(2 * l, l) - 2 * l : (ph < 2 ? w.Phi() + 2 * ph : w.Lam());
        const int st = (gam || ph == 2) ? 2 : 4;
        auto put = [&](int i) {
            rec[st * i] = g0;
            rec[st * i + 1] = g1;
        };
        put(gam ? l : 0);
        // fixed trip count (unrolls), branch-free: Gamma rows i <= l keep (B_l, 0) and
        // rewrite the diagonal.  The coefficients of CH steps are loaded ahead of the
        // chunk's stores (the stores cannot be proven not to alias them, so per-step
        // loads would wait for the previous step's stores: one LDS round trip a step)
        constexpr int CH = NTM_CH;
        NTM_CHUNK_PRAGMA
        for (int i0 = 1; i0 < N; i0 += CH) {
            double ca[CH], cb[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                ca[u] = i < N ? w.a11()[i] : 0.0;
                cb[u] = i < N ? w.a21()[i] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                if (i < N) {
                    const double n0 = ca[u] * g0 + c0;
                    const double n1 = (cb[u] * g0 + k.a22 * g1) + c1;
                    const bool live = !gam || i > l;
                    g0 = live ? n0 : g0;
                    g1 = live ? n1 : g1;
                    put(live ? i : l);
                }
            }
        }
    }
    NTM_ACC(ST_L_LOOP, tlf);
    // Phi and Lambda on lane 0 when the group has no idle lanes
    if (!extra && l == 0) {
        double p00 = w.a11()[0], p10 = w.a21()[0], p01 = 0.0, p11 = k.a22;
        double l0 = k.C1, l1 = k.C2;
        w.Phi()[0] = p00; w.Phi()[1] = p10; w.Phi()[2] = p01; w.Phi()[3] = p11;
        w.Lam()[0] = l0; w.Lam()[1] = l1;
        for (int i = 1; i < N; ++i) {
            double a11 = w.a11()[i], a21 = w.a21()[i];
            double q00 = a11 * p00, q01 = a11 * p01;
            double q10 = a21 * p00 + k.a22 * p10, q11 = a21 * p01 + k.a22 * p11;
            p00 = q00; p01 = q01; p10 = q10; p11 = q11;
            double m0 = a11 * l0 + k.C1;
            double m1 = (a21 * l0 + k.a22 * l1) + k.C2;
            l0 = m0; l1 = m1;
            w.Phi()[4 * i] = p00; w.Phi()[4 * i + 1] = p10; w.Phi()[4 * i + 2] = p01; w.Phi()[4 * i + 3] = p11;
            w.Lam()[2 * i] = l0; w.Lam()[2 * i + 1] = l1;
        }
    }
    NTM_WSYNC();
    }
}

// free response e = Phi x_k + Lambda (the x-dependent part of NTM_MPC_Sim.m:121
// and of c + W x_k at :97)
template <int P, class W>
__device__ __forceinline__ void free_response(const W& w, double x0, double x1, int l, const Prob* pw = nullptr) {
    for (int i = l; i < w.n(); i += P) {
        double e0, e1;
        if constexpr (W::kSlim) {                // the lift wrote e itself
            const dpair ev = ld_pair<pair_ld_ok<P, W>()>(w.e() + 2 * i);
            e0 = ev.x;
            e1 = ev.y;
        } else {
            const double* Ph = w.Phi() + 4 * i;
            e0 = (Ph[0] * x0 + Ph[2] * x1) + w.Lam()[2 * i];
            e1 = (Ph[1] * x0 + Ph[3] * x1) + w.Lam()[2 * i + 1];
            w.e()[2 * i] = e0;
            w.e()[2 * i + 1] = e1;
        }
        if (pw) {
            // Om (e_i - r) per stage for the scaling pass's F (scratch in w.xp(): the
            // rollout consumed it and rewrites it; the re-solve recomputes it)
            const double d0 = e0 - pw->r[0], d1 = e1 - pw->r[1];
            const OmQ<qi_on<W>()> om(pw->Q);
            w.xp()[2 * i] = om.o0(d0, d1);
            w.xp()[2 * i + 1] = om.o1(d0, d1);
        }
    }
    NTM_WSYNC();
}

}  // namespace ntm
