// ntm_gram.h — the cost: the Gram G = 2 Gamma' Om Gamma (+ 2 Ru I) on the matrix cores or
// row by row, the linear term F, and the diagonal scaling of both (scale_gram,
// diag_scale_phase, full_gram, scale_phase).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ntm_mpc.h"

#include "ntm_base.h"
#include "ntm_collectives.h"
#include "ntm_diag.h"
#include "ntm_lanes.h"
#include "ntm_lift.h"
#include "ntm_prob.h"
#include "ntm_ws.h"

namespace ntm {

// the launch has input-rate rows (never, in a kernel compiled without them: rate_rows)
template <class W>
__device__ __forceinline__ bool rate_mode(const Prob& pb) {
    if constexpr (rate_rows<W>()) return pb.mode == NTM_MODE_FULL_DU;
    else return false;
}

// ---------------------------------------------------------------------------
// Gram of Gamma columns on the matrix cores (long horizons): for the columns
// j_a = col_of(a), a < nc, S(a, c) = X_a' (I (x) Q) X_c with X_a = Gamma(:, j_a),
// i.e. S = X' Y with Y = (I (x) Q) X, the (nc x 2N) x (2N x nc) contraction of
// NTM_MPC_Sim.m:120 restricted to those columns.  V_MFMA_F64_16X16X4F64 on
// 16 x 16 tiles, K = 4 rows of Gamma per instruction (2N / 4 steps; NN even):
// lane l holds A = X(r, 16 t + (l & 15)) and B = Y(r, 16 t + (l & 15)) with
// r = 4 s + (l >> 4), both from the two Gamma rows of stage r / 2 (two LDS
// loads); the lower tile pairs accumulate in registers and put(a, c, S) takes
// every entry a >= c (D layout: column l & 15, row (l >> 4) + 4 i).  Same terms
// as qdot_rows / gram_rows, summed in the matrix core's order.  P = 64 only,
// called in wave-uniform control flow.
// ---------------------------------------------------------------------------
typedef double ntm_d4 __attribute__((ext_vector_type(4)));
template <int NN, class W, class ColOf, class Put>
__device__ __forceinline__ void gram_mfma(const Prob& pb, const W& w, int nc, ColOf col_of, Put put, int l) {
    static_assert(NN > 0 && NN % 2 == 0, "gram_mfma: compile-time even horizon");
    constexpr int TM = (NN + 15) / 16;                 // tiles of 16 columns
    constexpr int NP = TM * (TM + 1) / 2;              // lower tile pairs
    const OmQ<qi_on<W>()> om(pb.Q);
    const int li = l & 15, lk = l >> 4;
    const int T = (nc + 15) >> 4;
    int base[TM], r0[TM];
#pragma unroll
    for (int t = 0; t < TM; ++t) {
        const int a = 16 * t + li;
        const bool on = a < nc;
        const int j = on ? col_of(a) : 0;
        base[t] = w.gidx(2 * j, j) - 2 * j;             // Gamma(r, j) = Gt[base + r], r >= 2j
        r0[t] = on ? 2 * j : 2 * NN;                    // rows above the block diagonal are zero
    }
    ntm_d4 acc[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) acc[p] = ntm_d4{0.0, 0.0, 0.0, 0.0};
    const double* const G = w.Gt();
#pragma unroll 1
    for (int s = 0; s < NN / 2; ++s) {                  // not unrolled: the accumulators stay the only long-lived registers
        const int re = 4 * s + (lk & ~1);               // the even row of this lane's stage
        double xa[TM], yb[TM];
#pragma unroll
        for (int t = 0; t < TM; ++t) {
            const bool in = re >= r0[t];
            const double x0 = in ? G[base[t] + re] : 0.0, x1 = in ? G[base[t] + re + 1] : 0.0;
            xa[t] = (lk & 1) ? x1 : x0;
            yb[t] = (lk & 1) ? om.o1(x0, x1) : om.o0(x0, x1);
        }
        int p = 0;
#pragma unroll
        for (int ta = 0; ta < TM; ++ta)
#pragma unroll
            for (int tc = 0; tc <= ta; ++tc, ++p)
                if (ta < T) acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[ta], yb[tc], acc[p], 0, 0, 0);
    }
    int p = 0;
#pragma unroll
    for (int ta = 0; ta < TM; ++ta)
#pragma unroll
        for (int tc = 0; tc <= ta; ++tc, ++p) {
            if (ta >= T) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int a = 16 * ta + lk + 4 * i, c = 16 * tc + li;
                if (a < nc && c <= a) put(a, c, acc[p][i]);
            }
        }
}

// ---------------------------------------------------------------------------
// condensed cost G = 2 Gamma' Om Gamma (lower triangle into dst, col-major),
// F = 2 Gamma' Om (e - R)      NTM_MPC_Sim.m:120-121 (CANON D8, D12)
// ---------------------------------------------------------------------------
template <int P, class W, class Put>
__device__ __forceinline__ void gram_rows_put(const Prob& pb, const W& w, Put put, int l) {
    const int N = w.n();
    if constexpr (W::kNN > 32 && P == 64) {   // the matrix cores (gram_mfma)
        gram_mfma<W::kNN>(pb, w, N, [](int a) { return a; }, [&](int j, int kk, double sg) { put(j, kk, 2 * sg); },
                          l);
        return;
    }
    const OmQ<qi_on<W>()> om(pb.Q);
    // one (j, kk) entry per lane; fixed-trip masked dot (column reads below the
    // packed column start stay inside Gt, see StructRows::check)
    const int npair = N * (N + 1) / 2;
    for (int idx = l; idx < npair; idx += P) {
        int j = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
        if ((j + 1) * (j + 2) / 2 <= idx) ++j;
        if (j * (j + 1) / 2 > idx) --j;
        const int kk = idx - j * (j + 1) / 2;
        const double* cj = w.Gt() + w.gidx(2 * j, j) - 2 * j;
        const double* ck = w.Gt() + w.gidx(2 * kk, kk) - 2 * kk;
        double s = 0.0;
        for (int i = 0; i < N; ++i) {
            const double g0 = ck[2 * i], g1 = ck[2 * i + 1];
            const double o0 = om.o0(g0, g1);
            const double o1 = om.o1(g0, g1);
            const double t = cj[2 * i] * o0 + cj[2 * i + 1] * o1;
            s += (i >= j) ? t : 0.0;
        }
        double gv = 2 * s;
        if constexpr (ru_on<W>()) gv = (j == kk) ? gv + 2 * pb.Ru : gv;   // + 2 Ru I (ABI v5)
        put(j, kk, gv);             // G(j, kk), j >= kk
    }
}
template <int P, class W>
__device__ __forceinline__ void gram_rows(const Prob& pb, const W& w, double* dst, int l) {
    const int LD = w.ldj();
    gram_rows_put<P>(pb, w, [&](int j, int kk, double v) { dst[j + kk * LD] = v; }, l);
}

template <int P, class W>
__device__ __forceinline__ void cost_phase(const Prob& pb, const W& w, int l) {
    const int N = w.n();
    const double q00 = pb.Q[0], q01 = pb.Q[1], q10 = pb.Q[2], q11 = pb.Q[3];
    gram_rows<P>(pb, w, w.R(), l);
    if (l < N) {
        const double* cj = w.Gt() + w.gidx(2 * l, l) - 2 * l;
        double f = 0.0;
        for (int i = l; i < N; ++i) {
            double e0 = w.e()[2 * i] - pb.r[0], e1 = w.e()[2 * i + 1] - pb.r[1];
            double o0 = q00 * e0 + q01 * e1;
            double o1 = q10 * e0 + q11 * e1;
            f += cj[2 * i] * o0 + cj[2 * i + 1] * o1;
        }
        w.F()[l] = 2 * f;
    }
    NTM_WSYNC();
}

// G~ = D G D in place (lower triangle, col-major); the same expression order
// is used when the polish recomputes G~ (so both copies are bit-identical).
template <int P, class W>
__device__ __forceinline__ int scale_gram(const W& w, double* G, int l) {
    int bad = 0;
    if (l < w.n()) {
        double Dl = w.D()[l];
        for (int kk = 0; kk <= l; ++kk) {
            double v = G[l + kk * w.ldj()] * Dl * w.D()[kk];
            bad |= !isfinite(v);
            G[l + kk * w.ldj()] = v;
        }
    }
    return bad;
}

// ---------------------------------------------------------------------------
// Jacobi scaling U = D V with D = diag(G)^{-1/2}, computed from the Gram
// diagonal only (same summation order as gram_rows, so D is bit-identical to
// what the full G would give); F~ = D F; norms of the scaled state rows
// ||Gamma_r D||.  Gamma stays unscaled (D is applied on the fly).  The full
// G~ is only formed when the Goldfarb-Idnani fallback runs (full_gram).
// Returns (group-uniform) 2 if any datum is non-finite, else 1 if a constant
// row is violated (the x_0 rows and state rows Gamma does not reach: D15, D22,
// StructRows::feasible_const's test, folded into the row pass that finds them
// and into the one reduction, round 6), else 0.
// ---------------------------------------------------------------------------
// The far N = 20 build keeps the separate test (qp_phase calls feasible_const):
// folded in, it cost that kernel 1.3% through register allocation (6.30 -> 6.38 ms)
// while config 2 (0.201 -> 0.199 ms) and config 5 (74.2 -> 73.7 ms) gained.
template <class W>
__device__ __forceinline__ constexpr bool fold_const() { return !(W::kFar && W::kNN == 20); }
// Lane-masked chunk of the scaling pass's column pass (lane_masked_ok: column l on lane l),
// stages I0..I0+4 of column `lane`: the terms of G_ll and F_l formed on every lane, added
// on the lanes <= i, the non-finite Gamma entries of those lanes into nf
// (AL: cj and om are 16-byte aligned, ld_pair)
template <int I0, bool AL, class OM>
__device__ __forceinline__ void scale_col_chunk_lanes(const OM& qw, const double* cj, const double* om, double& s,
                                                      double& fs, unsigned long long& nf) {
    double ga[5], gb[5], ea[5], eb[5], t[5], tf[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const int i = I0 + u;
        const dpair gv = ld_pair<AL>(cj + 2 * i), ev = ld_pair<AL>(om + 2 * i);
        ga[u] = gv.x;
        gb[u] = gv.y;
        ea[u] = ev.x;
        eb[u] = ev.y;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const double g0 = ga[u], g1 = gb[u];
        const double o0 = qw.o0(g0, g1);
        const double o1 = qw.o1(g0, g1);
        t[u] = g0 * o0 + g1 * o1;
        tf[u] = g0 * ea[u] + g1 * eb[u];
    }
    fadd5x2_class_lanes_upto<I0>(s, fs, nf, t, tf, ga, gb);
}
// Lane-masked row pass of the scaling pass (esub_lanes_ok: state row r on lane r < 2N): s = the
// sum over j <= r / 2 of (Gamma_rj D_j)^2 in ascending j, last = the largest such j with
// Gamma_rj != 0 (-1: none), cnt = how many there are, added to what s / last / cnt hold on entry
template <class W>
__device__ __forceinline__ void row_norm_lanes(const W& w, int r, double& s, int& last, int& cnt) {
    static_assert(W::kNN == 20, "the packed offsets j (2N - 1 - j) of rownorm5_lanes_from are N = 20's");
    const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)(w.Gt() + r);
    const unsigned ad = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)w.D();
    rownorm5_lanes_from<0>(s, last, cnt, at, ad);
    rownorm5_lanes_from<5>(s, last, cnt, at, ad);
    rownorm5_lanes_from<10>(s, last, cnt, at, ad);
    rownorm5_lanes_from<15>(s, last, cnt, at, ad);
}
template <int P, class W>
__device__ __forceinline__ int diag_scale_phase(const Prob& pb, const W& w, int l, bool with_state_rows,
                                                double x0 = 0.0, double x1 = 0.0, const ColSums* cs = nullptr) {
    const int N = w.n();
    const OmQ<qi_on<W>()> qw(pb.Q);
    int bad = 0, infe = 0;
    auto const_row = [&](int r) {                         // 0 <= b on a constant state row, to kConstTol
        if constexpr (!fold_const<W>()) return;
        const int c = r & 1;
        const double er = w.e()[r];
        infe |= (er - pb.xmin[c]) < -kConstTol;
        infe |= (pb.xmax[c] - er) < -kConstTol;
    };
    if (fold_const<W>() && with_state_rows && l == 0) {   // the x_0 rows (D15)
        infe |= (x0 - pb.xmin[0]) < -kConstTol;
        infe |= (x1 - pb.xmin[1]) < -kConstTol;
        infe |= (pb.xmax[0] - x0) < -kConstTol;
        infe |= (pb.xmax[1] - x1) < -kConstTol;
    }
    NTM_T0(tsc);
    // Short horizons (2N <= 64, N = 20): the column pass and the row pass each split
    // their sums in two halves at H = ceil(N/2) on otherwise idle lanes, so the wave
    // runs H trips instead of N (lanes N..2N-1 take the columns' i >= H terms; lanes
    // 2N.. the j >= H terms of rows with r >= 2H).  The sums are then (first half) +
    // (second half) instead of one sequential pass.  The all-LDS build only (config 2,
    // B = 1024: 0.208 -> 0.199 ms; mode 2 at B = 1024: 0.545 -> 0.526 ms).  The far
    // build's register allocation does not absorb it: 6.36 -> 7.98 ms per step-batch
    // at B = 1e5 with the chunk unroll, 6.41 ms without; the column pass alone 7.11 ms,
    // the row pass alone 9.66 ms (A/B on one box)
    constexpr int NNs = W::kNN, Hs = (NNs + 1) / 2;
    constexpr bool kSplit = !W::kFar && P == 64 && NNs > 0 && 4 * NNs - 2 * Hs <= 64;
    if constexpr (kSplit) {
        double s = 0.0, fs = 0.0;
        const int col = l < N ? l : l - N;
        const int base = l < N ? 0 : Hs;
        if (l < 2 * N) {
            const double* cj = w.Gt() + w.gidx(2 * col, col) - 2 * col;
            const double* om = w.xp();
            constexpr int CH = NTM_CH;
            NTM_CHUNK_PRAGMA
            for (int u0 = 0; u0 < Hs; u0 += CH) {
                double ga[CH], gb[CH], ea[CH], eb[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int i = base + u0 + u;
                    const bool in = u0 + u < Hs && i < N;
                    ga[u] = in ? cj[2 * i] : 0.0;
                    gb[u] = in ? cj[2 * i + 1] : 0.0;
                    ea[u] = in ? om[2 * i] : 0.0;
                    eb[u] = in ? om[2 * i + 1] : 0.0;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int i = base + u0 + u;
                    const double g0 = ga[u], g1 = gb[u];
                    const double o0 = qw.o0(g0, g1);
                    const double o1 = qw.o1(g0, g1);
                    const double t = g0 * o0 + g1 * o1;
                    const double tf = g0 * ea[u] + g1 * eb[u];
                    const bool on = u0 + u < Hs && i >= col && i < N;
                    if (on) bad |= !isfinite(g0) || !isfinite(g1);
                    s += on ? t : 0.0;
                    fs += on ? tf : 0.0;
                }
            }
        }
        const double s2 = __shfl(s, (l + N) & 63, 64);
        const double f2 = __shfl(fs, (l + N) & 63, 64);
        if (l < N) {
            double g = 2 * (s + s2);
            if constexpr (ru_on<W>()) g = g + 2 * pb.Ru;   // G_ll + 2 Ru (ABI v5)
            const double Dl = (g > 0.0 && g < kInf) ? rsqrt_nr(g) : 1.0;
            w.D()[l] = Dl;
            const double f = (2 * (fs + f2)) * Dl;
            bad |= !isfinite(f) || !isfinite(Dl);
            w.F()[l] = f;
            if constexpr (!W::kSlim) {
                w.vlo()[l] = -((-pb.umin) / Dl);
                w.vhi()[l] = pb.umax / Dl;
            }
        }
        NTM_WSYNC();
        NTM_ACC(ST_SC_COL, tsc);
        if (rate_mode<W>(pb) && l >= 1 && l < N) {
            const double a = w.D()[l], b = w.D()[l - 1];
            w.idun()[l] = 1.0 / sqrt(a * a + b * b);
        }
        if (with_state_rows) {
            const bool lo = l < 2 * N, hi = !lo && l < 4 * N - 2 * Hs;
            const int r = lo ? l : (hi ? l - 2 * N + 2 * Hs : 0);
            const int jb = lo ? 0 : Hs;
            const int jmax = r >> 1;
            double rs = 0.0;
            int last = -1, cnt = 0;
            if (lo || hi) {
                constexpr int CH = NTM_CH;
                NTM_CHUNK_PRAGMA
                for (int u0 = 0; u0 < Hs; u0 += CH) {
                    double g[CH], dd[CH];
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        const int j = jb + u0 + u;
                        const bool in = u0 + u < Hs && j < N;
                        g[u] = in ? w.gt(r, j) : 0.0;
                        dd[u] = in ? w.D()[j] : 0.0;
                    }
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        const int j = jb + u0 + u;
                        const double v = g[u] * dd[u];
                        const bool in = u0 + u < Hs && j <= jmax;
                        rs += in ? v * v : 0.0;
                        if (in && g[u] != 0.0) { last = j; ++cnt; }
                    }
                }
            }
            // the row's second half sits on lane 2N + r - 2H (rows r >= 2H)
            const int src = (l >= 2 * Hs && l < 2 * N) ? l + 2 * N - 2 * Hs : l;
            const double rs2 = __shfl(rs, src & 63, 64);
            const int last2 = __shfl(last, src & 63, 64);
            const int cnt2 = __shfl(cnt, src & 63, 64);
            if (lo) {
                const bool two = src != l;
                const double sr = two ? rs + rs2 : rs;
                const int lr = (two && last2 >= 0) ? last2 : last;
                const int cr = two ? cnt + cnt2 : cnt;
                bad |= !isfinite(sr) || !isfinite(w.e()[r]);
                const double ir = (sr > 0.0 && sr < kInf) ? rsqrt_nr(sr) : 0.0;
                w.irn()[r] = ir;
                w.rinfo()[r] = (lr + 1) | (cr > 1 ? kRowMulti : 0);
                if (ir == 0.0) const_row(r);
            }
            NTM_WSYNC();
        }
        NTM_ACC(ST_SC_ROW, tsc);
        const int code = gany<P>(bad != 0) ? 2 : ((fold_const<W>() && gany<P>(infe != 0)) ? 1 : 0);
        NTM_ACC(ST_SC_END, tsc);
        return code;
    }
    if (l < N) {
        // one pass over Gamma's column l: the Gram diagonal G_ll and F_l = 2 Gamma_l' Om (e - r)
        const double* cj = w.Gt() + w.gidx(2 * l, l) - 2 * l;
        const double* om = w.xp();               // Om (e_i - r), from free_response
        double s = 0.0, fs = 0.0;
        constexpr int CH = NTM_CH;
        if (fuse_colsum<W>() && cs) {           // summed by the lift
            s = cs->s;
            fs = cs->f;
            bad |= cs->bad;
        } else if constexpr (lane_masked_ok<P, CH, W>()) {   // terms i < l masked by lane
            unsigned long long nf = 0ull;
            constexpr bool AL = pair_ld_ok<P, W>();     // a Gamma column from row 0, xp
            scale_col_chunk_lanes<0, AL>(qw, cj, om, s, fs, nf);
            scale_col_chunk_lanes<5, AL>(qw, cj, om, s, fs, nf);
            scale_col_chunk_lanes<10, AL>(qw, cj, om, s, fs, nf);
            scale_col_chunk_lanes<15, AL>(qw, cj, om, s, fs, nf);
            bad |= (int)((nf >> l) & 1ull);
        } else {
        NTM_CHUNK_PRAGMA
        for (int i0 = 0; i0 < N; i0 += CH) {     // fixed trip count, terms i < l masked; batched loads
            double ga[CH], gb[CH], ea[CH], eb[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                const bool in = i < N;
                ga[u] = in ? cj[2 * i] : 0.0;
                gb[u] = in ? cj[2 * i + 1] : 0.0;
                ea[u] = in ? om[2 * i] : 0.0;
                eb[u] = in ? om[2 * i + 1] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                const double g0 = ga[u], g1 = gb[u];
                const double o0 = qw.o0(g0, g1);
                const double o1 = qw.o1(g0, g1);
                const double t = g0 * o0 + g1 * o1;
                const double tf = g0 * ea[u] + g1 * eb[u];
                const bool on = i >= l && i < N;
                if (on) bad |= !isfinite(g0) || !isfinite(g1);
                s += on ? t : 0.0;
                fs += on ? tf : 0.0;
            }
        }
        }
        double g = 2 * s;
        if constexpr (ru_on<W>()) g = g + 2 * pb.Ru;   // G_ll + 2 Ru (ABI v5)
        double Dl = (g > 0.0 && g < kInf) ? rsqrt_nr(g) : 1.0;
        w.D()[l] = Dl;
        double f = (2 * fs) * Dl;
        bad |= !isfinite(f) || !isfinite(Dl);
        w.F()[l] = f;
        // V-space box of u_l (bc of the two u rows; same expressions as the oracle's b/rn).
        // kBox: into a11 / a21, which the lift has finished with (WS::kBox); once per QP, where
        // StructRows::check divided twice per call
        if constexpr (!W::kSlim || W::kBox) {
            w.vlo()[l] = -((-pb.umin) / Dl);
            w.vhi()[l] = pb.umax / Dl;
        }
    }
    NTM_WSYNC();
    NTM_ACC(ST_SC_COL, tsc);
    if (rate_mode<W>(pb) && l >= 1 && l < N) {                  // rate-row norms |D (e_l - e_{l-1})|
        const double a = w.D()[l], b = w.D()[l - 1];
        w.idun()[l] = 1.0 / sqrt(a * a + b * b);
    }
    if (with_state_rows) {
        for (int r = l; r < 2 * N; r += P) {
            double s = 0.0;
            const int jmax = r >> 1;
            int last = -1, cnt = 0;
            constexpr int CH = NTM_CH;
            if constexpr (esub_lanes_ok<P, CH, W>()) {   // terms j > jmax masked by lane (r = l: one trip)
                row_norm_lanes(w, r, s, last, cnt);
            } else {
            NTM_CHUNK_PRAGMA
            for (int j0 = 0; j0 < N; j0 += CH) { // fixed trip count, j > jmax masked; batched loads
                double g[CH], dd[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const int j = j0 + u;
                    g[u] = j < N ? w.gt(r, j) : 0.0;
                    dd[u] = j < N ? w.D()[j] : 0.0;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const double v = g[u] * dd[u];
                    const bool in = j0 + u <= jmax;
                    s += in ? v * v : 0.0;
                    if (in && g[u] != 0.0) { last = j0 + u; ++cnt; }
                }
            }
            }
            bad |= !isfinite(s) || !isfinite(w.e()[r]);
            const double ir = (s > 0.0 && s < kInf) ? rsqrt_nr(s) : 0.0;
            w.irn()[r] = ir;                     // 1/|Gamma_r D| (0: constant row)
            w.rinfo()[r] = (last + 1) | (cnt > 1 ? kRowMulti : 0);
            if (ir == 0.0) const_row(r);
        }
        NTM_WSYNC();
    }
    NTM_ACC(ST_SC_ROW, tsc);
    const int code = gany<P>(bad != 0) ? 2 : ((fold_const<W>() && gany<P>(infe != 0)) ? 1 : 0);
    NTM_ACC(ST_SC_END, tsc);
    return code;
}

// the full scaled Hessian G~ (lower triangle, WS::gr) for the GI fallback
template <int P, class W>
__device__ __forceinline__ bool full_gram(const Prob& pb, const W& w, int l) {
    int bad = 0;
    if constexpr (W::kGiLdsL) {
        gram_rows_put<P>(pb, w, [&](int j, int kk, double v) { w.grL(j, kk) = v; }, l);
        NTM_WSYNC();
        if (l < w.n()) {                      // scale_gram's expression order
            const double Dl = w.D()[l];
            for (int kk = 0; kk <= l; ++kk) {
                const double v = w.grL(l, kk) * Dl * w.D()[kk];
                bad |= !isfinite(v);
                w.grL(l, kk) = v;
            }
        }
    } else {
        gram_rows<P>(pb, w, w.R(), l);
        NTM_WSYNC();
        bad = scale_gram<P>(w, w.R(), l);
    }
    NTM_WSYNC();
    return !gany<P>(bad != 0);
}

// kept for the dense-row entry point (ntm_qp_device): G~ = D G D in place,
// F~ = D F (G given in w.R()); no state rows
template <int P, class W>
__device__ __forceinline__ bool scale_phase(const W& w, int l, bool /*with_state_rows*/) {
    const int N = w.n(), LD = w.ldj();
    if (l < N) {
        double g = w.R()[l + l * LD];
        w.D()[l] = (g > 0.0) ? 1.0 / sqrt(g) : 1.0;
    }
    NTM_WSYNC();
    int bad = scale_gram<P>(w, w.R(), l);
    if (l < N) {
        double f = w.F()[l] * w.D()[l];
        bad |= !isfinite(f);
        w.F()[l] = f;
    }
    NTM_WSYNC();
    return !gany<P>(bad != 0);
}

}  // namespace ntm
