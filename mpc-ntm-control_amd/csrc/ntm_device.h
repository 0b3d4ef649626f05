// ntm_device.h — device-side building blocks of the batched LPV-MPC hot path
// (gfx950 / CDNA4).  One scenario is owned by a GROUP of P lanes of a wave
// (P = 16, 32 or 64; 64/P scenarios per wave).  Lane l of a group owns index
// l of every length-N vector (decision variable u_l, prediction step l).
// All per-scenario matrices live in the group's slice of LDS; cross-lane
// traffic is LDS broadcast reads plus ds_bpermute shuffles inside the group.
// Every control decision is a group reduction, so control flow is
// group-uniform and the 64/P groups of a wave may diverge freely.
//
// Reference map (file:line of the MATLAB reference):
//   rho_eval          rho1.m:2, rho2.m:2, rho3.m:2-3
//   lift_phase        A.m:2, B.m:2, Rho_to_PhiGammaLambda.m:17-52 (CANON D4/D6)
//   cost_phase        NTM_MPC_Sim.m:67-73, 120-121 (CANON D8/D12)
//   StructRows        getWLc.m:9-59 rows, never materialised (implicit rows)
//   gi_solve          quadprog call NTM_MPC_Sim.m:97 (Goldfarb-Idnani)
//   rollout_phase     NTM_MPC_Sim.m:110-117, 123-127
//   plant_phase       NTM_MPC_Sim.m:130 (CANON D13)
//
// Every phase is __forceinline__: left to its heuristics the inliner outlines
// whichever phase crosses its size threshold, and an outlined phase is a real
// call on gfx950 (the Prob and WS references copied to scratch, the caller's
// live VGPRs saved around it): 15.9 -> 14.7 ms per step-batch at B=1e5, N=20
// once everything was inlined again.
//
// The layers below the solver have headers of their own, included here in this order (each
// is #pragma once, includes exactly what it uses and compiles on its own):
//   ntm_prob.h         Coef, Gen, Prob; the counter-based scenario generator (host and device)
//   ntm_diag.h         NTM_TRACE*, the stamp macros, NTM_NSTAMPS, the ST_* / CN_* slots, ST_COUNT
//   ntm_base.h         kInf, rsqrt_nr, the solver constants, the build switches and how a
//                      translation unit sets them, NTM_CH, NTM_CHUNK_PRAGMA, NTM_WSYNC
//   ntm_collectives.h  dpp_d .. gargmin: reductions, ballots and broadcasts over a group
//   ntm_ws.h           rho_eval / coef_*, ws_far, WS, ws_bytes, ws_carve, ru_on, qi_on, OmQ,
//                      scn_coef, scn_store
//   ntm_lanes.h        every inline-assembly helper that runs under a narrowed EXEC, with the
//                      rules they share: lane_masked_ok, fmac5*_lanes_from, fadd5*_lanes_upto,
//                      lift_chunk_lanes, esub_lanes_ok, fsub_lanes, bsub_lanes, rownorm5_lanes_from
//                      (lift_lanes_ok names fuse_colsum and stays with it in ntm_lift.h)
//   ntm_dots.h         qdot_rows, dot_batched, dot_range, sub_dot, axpy_sub, gamma_row_dot,
//                      gamma_row_dot2, dot_rows2
//   ntm_lift.h         lift_literal, ColSums, fuse_colsum, lift_lanes_ok, lift_chunk_at,
//                      lift_phase, free_response
//   ntm_gram.h         gram_mfma, gram_rows*, cost_phase, scale_gram, scale_col_chunk_lanes,
//                      diag_scale_phase, full_gram, scale_phase
// This file still holds the constraint-row providers (Pick, StructRows, DenseRows), the small
// dense kernels and Goldfarb-Idnani (chol_*, fwd_lanes, bwd_lanes, gi_solve), the two polishers
// (polish_phase, polish_compact) and the QP driver (rollout_phase, plant_step, shifted_into_act,
// gi_fallback, qp_phase).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ntm_mpc.h"

#include "ntm_prob.h"
#include "ntm_diag.h"
#include "ntm_base.h"
#include "ntm_collectives.h"
#include "ntm_ws.h"
#include "ntm_lanes.h"
#include "ntm_dots.h"
#include "ntm_lift.h"
#include "ntm_gram.h"

namespace ntm {

// ---------------------------------------------------------------------------
// Constraint-row providers (Lin U <= b form, getWLc.m row convention).  Row
// ids follow the oracle: box mode rows 0..N-1 are u_j >= umin, N..2N-1 are
// u_j <= umax; full mode rows follow getWLc.m:9-59 block by block (6 per
// step, 4 terminal).  In the solver each row is scaled and normalised:
//   GI normal n = -(Lin D)/rn,  GI rhs bc = -b/rn,  slack s = n'V - bc.
// ---------------------------------------------------------------------------
struct Pick {
    int p;        // row id (-1 none)
    double s;     // normalised slack (GI form n'V - bc)
    double bc;    // normalised GI right-hand side
};

// aflag bits per constraint row
constexpr unsigned char kActiveRow = 1;   // in GI's active set
constexpr unsigned char kCandRow = 2;     // row of a failed warm-start candidate (GI adds these first)
constexpr unsigned char kSkipRow = 4;     // dual path (long horizons): p left out until the active set changes

// Implicit getWLc rows: u-bounds are -+e_j, state rows are -+Gamma_r; the
// rows are never materialised.
struct StructRows {
    static constexpr bool kHasUnitRows = true;
    int N, mode;  // NTM_MODE_BOX, NTM_MODE_FULL or NTM_MODE_FULL_DU (NONE: no rows)
    double umin, umax, xmin0, xmin1, xmax0, xmax1, du;

    __device__ __forceinline__ StructRows(const Prob& p)
        : N(p.N), mode(p.mode), umin(p.umin), umax(p.umax), xmin0(p.xmin[0]), xmin1(p.xmin[1]),
          xmax0(p.xmax[0]), xmax1(p.xmax[1]), du(p.du) {}
    __device__ __forceinline__ bool has_state() const { return mode >= NTM_MODE_FULL; }
    __device__ __forceinline__ bool has_rate() const { return mode == NTM_MODE_FULL_DU; }
    __device__ __forceinline__ double xmin(int c) const { return c ? xmin1 : xmin0; }
    __device__ __forceinline__ double xmax(int c) const { return c ? xmax1 : xmax0; }

    __device__ __forceinline__ int rows() const {
        return mode == NTM_MODE_NONE ? 0 : (mode == NTM_MODE_BOX ? 2 * N : (mode == NTM_MODE_FULL_DU ? 8 * N + 2 : 6 * N + 4));
    }

    // decode a row id: kind 0 = u lower, 1 = u upper, 2 = state min, 3 = state max,
    // 4 = rate up (U_j - U_{j-1} <= du), 5 = rate down (U_{j-1} - U_j <= du);
    // j = variable (u and rate rows) or state row r (state rows); -1 for x_0 rows.
    // Rate rows follow the 6N+4 getWLc rows: id = 6N+4 + 2(j-1) + {0 up, 1 down}.
    // kRate = false (callers that know their kernel: rate_rows<W>() in ntm_ws.h): the
    // launch has no rate rows whatever `mode` says, so no kind >= 4 comes out, and the
    // callers' rate arms, written `rate_rows<W>() && ...`, fold away with every read of du
    template <bool kRate = true>
    __device__ __forceinline__ void decode(int id, int N, int& kind, int& j) const {
        if (kRate && mode == NTM_MODE_FULL_DU && id >= 6 * N + 4) {
            const int t = id - (6 * N + 4);
            kind = 4 + (t & 1);
            j = (t >> 1) + 1;
            return;
        }
        if (mode == NTM_MODE_BOX) {
            kind = id < N ? 0 : 1;
            j = id < N ? id : id - N;
            return;
        }
        int blk = id / 6, rr = id - 6 * blk;
        if (blk < N && rr < 2) { kind = rr; j = blk; return; }
        int i, c;
        bool upper;
        if (blk < N) { i = blk; c = (rr - 2) & 1; upper = rr >= 4; }
        else { i = N; c = rr & 1; upper = rr >= 2; }
        kind = upper ? 3 : 2;
        j = (i == 0) ? -1 : 2 * (i - 1) + c;
    }
    // u-bound row: its variable j and the sign of its GI normal (+1 lower, -1 upper); -1 otherwise
    __device__ __forceinline__ int unit_row(int id, int Nn, double& sg) const {
        int kind, j;
        decode(id, Nn, kind, j);
        sg = (kind == 0) ? 1.0 : -1.0;
        return kind < 2 ? j : -1;
    }
    template <class W>
    __device__ __forceinline__ double lin(const W& w, int id, int col) const {          // Lin[id][col]
        int kind, j;
        decode<rate_rows<W>()>(id, w.n(), kind, j);
        if (kind < 2) return (col == j) ? (kind == 0 ? -1.0 : 1.0) : 0.0;
        if (rate_rows<W>() && kind >= 4) {
            const double sg = kind == 4 ? 1.0 : -1.0;
            return col == j ? sg : (col == j - 1 ? -sg : 0.0);
        }
        if (j < 0 || col > (j >> 1)) return 0.0;
        double g = w.gt(j, col);
        return kind == 2 ? -g : g;
    }
    template <class W>
    __device__ __forceinline__ double bval(const W& w, int id) const {                  // b[id]
        int kind, j;
        decode<rate_rows<W>()>(id, w.n(), kind, j);
        if (kind == 0) return -umin;
        if (kind == 1) return umax;
        if (rate_rows<W>() && kind >= 4) return du;
        int c = j & 1;
        return kind == 2 ? (-xmin(c) + w.e()[j]) : (xmax(c) - w.e()[j]);
    }
    template <class W>
    __device__ __forceinline__ double rnorm(const W& w, int id) const {
        int kind, j;
        decode<rate_rows<W>()>(id, w.n(), kind, j);
        if (rate_rows<W>() && kind >= 4) return 1.0 / w.idun()[j];
        return kind < 2 ? w.D()[j] : 1.0 / w.irn()[j];
    }

    // constant rows (x_0 rows; state rows with Gamma_r == 0): 0 <= b, to kConstTol,
    // or infeasible (D15, D22)
    template <int P, class W>
    __device__ __forceinline__ bool feasible_const(const W& w, double x0, double x1, int l) const {
        int bad = 0;
        if (has_state()) {
            if (l == 0) {
                bad |= (x0 - xmin(0)) < -kConstTol;
                bad |= (x1 - xmin(1)) < -kConstTol;
                bad |= (xmax(0) - x0) < -kConstTol;
                bad |= (xmax(1) - x1) < -kConstTol;
            }
            for (int r = l; r < 2 * w.n(); r += P) {
                if (w.irn()[r] == 0.0) {
                    int c = r & 1;
                    bad |= (w.e()[r] - xmin(c)) < -kConstTol;
                    bad |= (xmax(c) - w.e()[r]) < -kConstTol;
                }
            }
        }
        // (kept as the DPP reduction, with load_candidates' two in ntm_step.h: with all
        // three as ballots the far N = 20 kernel returned wrong plans for 20 of 64
        // scenarios, and turning any one of them back gave the parent's results bit for
        // bit; so did the all-ballot source built without the N = 20 TU's scheduler
        // flag or with SGPR spills to memory: code generation, not the source, and not
        // located further.  Once per QP / per step: nothing to gain here.
        // Any change to these kernels is checked by the byte-equal A/B of the benchmark's
        // dumped outputs against the parent (profiles/r07_ab/bitwise.txt), not only by
        // the tolerance tests)
        return gmaxi<P>(bad) == 0;
    }

    // The certificate's primal tolerance on the input bounds.  A bound's slack V_l - lo
    // is exact (an active bound's is zero), so the runtime-N kernels hold it to
    // Goldfarb-Idnani's own stopping tolerance: with the 1e-9 of the general rows they
    // certified a set that left a variable free 2.8e-10 of the largest input outside
    // its bound, 1.2e-10 umax off the optimum (N = 49 mode 2,
    // tests/test_gpu_config_space.py).  The compiled horizons keep 1e-9: with 1e-12
    // the N = 20 far kernel measured 10% slower (6.34 -> 6.99 ms per step-batch, A/B on
    // one box) and the N = 50 mode-3 closed loops left the oracle's
    template <class W>
    __device__ static constexpr double bound_tol() { return W::kNN == 0 ? 1e-12 : 1e-9; }
    __device__ bool is_bound_row(int id, int N) const {
        return mode == NTM_MODE_BOX || (id < 6 * N && id % 6 < 2);
    }

    // Most violated inactive row (verify = false), or, with verify = true,
    // whether EVERY row has slack >= -tol * max(vmax, |bc|) (returned in .p).
    // Rows flagged kCandRow (the rows of a warm-start candidate that failed
    // its certificate) are taken first while any of them is violated beyond
    // GI's stopping tolerance: GI may add any violated row, so this only
    // steers it towards the nearby active set.
    template <int P, class W>
    __device__ __forceinline__ Pick check(const W& w, double Vl, int l, bool verify = false, double vmax = 1.0,
                                          const double* y_pre = nullptr) const {   // y_pre[r] = Gamma_r U if given
        const int N = w.n();
        if (mode == NTM_MODE_NONE) { Pick none; none.p = verify ? 0 : -1; none.s = 0.0; none.bc = 0.0; return none; }
        double bv = kInf, bs = 0.0, bbc = 0.0;
        int bid = 0x7fffffff, bad = 0;
        auto consider = [&](double s, int id, double bcv, double vtol = 1e-9) {
            if (verify) { bad |= s < -vtol * fmax(vmax, fabs(bcv)); return; }
            const unsigned char fl = w.aflag()[id];
            constexpr unsigned char kOut = (W::kNN > 32 || W::kNN == 0) ? (kActiveRow | kSkipRow) : kActiveRow;
            if (fl & kOut) return;
            const double key = ((fl & kCandRow) && s < -1e-12 * fmax(vmax, fabs(bcv))) ? s - 1e200 : s;
            if (key < bv || (key == bv && id < bid)) { bv = key; bid = id; bs = s; bbc = bcv; }
        };
        if (l < N) {
            double lo, hi;
            if constexpr (W::kSlim && !W::kBox) {             // (diag_scale_phase's expressions)
                const double Dl = w.D()[l];
                lo = -((-umin) / Dl);
                hi = umax / Dl;
            } else {
                lo = w.vlo()[l];
                hi = w.vhi()[l];
            }
            int idl = (mode == NTM_MODE_BOX) ? l : 6 * l;
            int idh = (mode == NTM_MODE_BOX) ? N + l : 6 * l + 1;
            consider(Vl - lo, idl, lo, bound_tol<W>());
            consider(hi - Vl, idh, -hi, bound_tol<W>());
        }
        if (rate_rows<W>() && has_rate() && l >= 1 && l < N) {   // rate rows on lane j
            const double ir = w.idun()[l];
            const double dU = w.U()[l] - w.U()[l - 1];
            const int id0 = 6 * N + 4 + 2 * (l - 1);
            consider((du - dU) * ir, id0, -(du * ir));
            consider((du + dU) * ir, id0 + 1, -(du * ir));
        }
        if (has_state()) {
            for (int r = l; r < 2 * N; r += P) {
                double ir = w.irn()[r];
                if (ir > 0.0) {
                    int jmax = r >> 1;
                    const double* gr = w.Gt() + r;           // gt(r, j) = gr[gidx(0, j)]
                    double xh = 0.0;
                    if (y_pre) {
                        xh = y_pre[r];
                    } else {
                        // fixed trip count, entries j > jmax masked.  The packed reads stay
                        // inside Gt: gidx(0, j) + r = j(2N-j-1) + r < N(N+1)
                        (void)gr;
                        xh = gamma_row_dot<NTM_CH, P>(w, r, w.U());
                    }
                    const double er = w.e()[r];
                    xh += er;
                    int c = r & 1, i = jmax + 1;
                    int idmin = (i < N) ? 6 * i + 2 + c : 6 * N + c;
                    consider((xh - xmin(c)) * ir, idmin, (xmin(c) - er) * ir);
                    consider((xmax(c) - xh) * ir, idmin + 2, -((xmax(c) - er) * ir));
                }
            }
        }
        Pick pk;
        if (verify) {
            pk.p = gany<P>(bad != 0) ? 1 : 0;
            pk.s = 0.0;
            pk.bc = 0.0;
            return pk;
        }
        gargmin<P>(bv, bid, bs, bbc);
        pk.p = (bv < kInf) ? bid : -1;
        pk.s = bs;
        pk.bc = bbc;
        return pk;
    }

    // GI normal n_p into w.np(); returns bc_p
    template <int P, class W>
    __device__ __forceinline__ double load_np(const W& w, int p, int l) const {
        double rn = rnorm(w, p);
        if (l < w.n()) w.np()[l] = -((lin(w, p, l) * w.D()[l]) / rn);
        NTM_WSYNC();
        return -(bval(w, p) / rn);
    }
};

// Explicit dense rows Lin U <= b (batched SoA in global memory) for the
// quadprog-level entry point ntm_qp_device.
struct DenseRows {
    static constexpr bool kHasUnitRows = false;
    __device__ int unit_row(int, int, double& sg) const { sg = 0.0; return -1; }
    const double* Lin;  // element (i, j) of scenario s at [s*m*N + i + j*m] (scenario-major)
    const double* b;    // [s*m + i]
    double* rnrm;       // LDS, m entries
    int64_t nv, s;      // variables per scenario (N), scenario index
    int m;

    __device__ int rows() const { return m; }
    template <class W>
    __device__ double lin(const W&, int i, int j) const { return Lin[s * ((int64_t)m * nv) + i + (int64_t)j * m]; }
    template <class W>
    __device__ double bval(const W&, int i) const { return b[s * m + i]; }
    template <class W>
    __device__ double rnorm(const W&, int i) const { return rnrm[i]; }

    template <int P, class W>
    __device__ int prepare_code(const W& w, int l) {
        int bad = 0;
        for (int i = l; i < m; i += P) {
            double ss = 0.0;
            for (int j = 0; j < w.n(); ++j) { double v = lin(w, i, j) * w.D()[j]; ss += v * v; }
            double bi = bval(w, i);
            if (!isfinite(ss) || !isfinite(bi)) bad |= 1;
            rnrm[i] = ss > 0.0 ? sqrt(ss) : 0.0;
            if (!(ss > 0.0) && bi < -kConstTol) bad |= 2;   // constant row violated (D15, D22)
        }
        NTM_WSYNC();
        return gmaxi<P>(bad);
    }
    template <int P, class W>
    __device__ Pick check(const W& w, double Vl, int l, bool verify = false, double vmax = 1.0) const {
        double bvv = kInf, bs = 0.0, bbc = 0.0;
        int bid = 0x7fffffff, bad = 0;
        for (int i = l; i < m; i += P) {
            double rn = rnrm[i];
            if (rn > 0.0 && (verify || !(w.aflag()[i] & kActiveRow))) {
                double sl = 0.0;
                for (int j = 0; j < w.n(); ++j) sl -= ((lin(w, i, j) * w.D()[j]) / rn) * w.V()[j];
                double bi = bval(w, i) / rn;
                sl += bi;
                if (verify) bad |= sl < -1e-9 * fmax(vmax, fabs(bi));
                else if (sl < bvv || (sl == bvv && i < bid)) { bvv = sl; bid = i; bs = sl; bbc = -bi; }
            }
        }
        Pick pk;
        if (verify) {
            pk.p = gany<P>(bad != 0) ? 1 : 0;
            pk.s = 0.0;
            pk.bc = 0.0;
            return pk;
        }
        gargmin<P>(bvv, bid, bs, bbc);
        pk.p = (bvv < kInf) ? bid : -1;
        pk.s = bs;
        pk.bc = bbc;
        return pk;
    }
    template <int P, class W>
    __device__ double load_np(const W& w, int p, int l) const {
        double rn = rnrm[p];
        if (l < w.n()) w.np()[l] = -((lin(w, p, l) * w.D()[l]) / rn);
        NTM_WSYNC();
        return -(bval(w, p) / rn);
    }
};

// ---------------------------------------------------------------------------
// small dense kernels on a group's LDS matrices (col-major, leading dim LD)
// ---------------------------------------------------------------------------
// Element (i, j) of a small matrix lives at A[i*RS + j*CS] (col-major: RS = 1,
// CS = LD; the polish's K is stored transposed: RS = LD, CS = 1).
// left-looking Cholesky of the n x n lower triangle of A, in place; the
// reciprocals of the diagonal go to rdiag[0..n) (the triangular solves then
// multiply instead of divide); false if not PD
template <int P>
__device__ __forceinline__ bool chol_inplace(double* A, int n, int RS, int CS, int l, double* rdiag) {
    for (int k = 0; k < n; ++k) {
        double s = 0.0;
        if (l >= k && l < n) {
            s = sub_dot<NTM_CH>(A[l * RS + k * CS], A + l * RS, CS, A + k * RS, CS, 0, k);
        }
        double dk = gbcast<P>(s, k);
        if (!(dk > 0.0) || !(dk < kInf)) return false;
        const double il = rsqrt_nr(dk);
        const double lk = dk * il;
        if (l > k && l < n) A[l * RS + k * CS] = s * il;
        if (l == k) { A[k * RS + k * CS] = lk; rdiag[k] = il; }
        NTM_WSYNC();
    }
    return true;
}
// chol_inplace on GI's factor storage (WS::gr / grow: rows of the lower triangle)
template <int P, class W>
__device__ __forceinline__ bool chol_gr(const W& w, int n, int l, double* rdiag) {
    if constexpr (!W::kGiLdsL) {
        return chol_inplace<P>(w.R(), n, 1, w.ldj(), l, rdiag);
    } else {
        for (int k = 0; k < n; ++k) {
            double s = 0.0;
            if (l >= k && l < n) s = sub_dot<NTM_CH>(w.grL(l, k), w.grow(l), 1, w.grow(k), 1, 0, k);
            const double dk = gbcast<P>(s, k);
            if (!(dk > 0.0) || !(dk < kInf)) return false;
            const double il = rsqrt_nr(dk);
            const double lk = dk * il;
            if (l > k && l < n) w.grL(l, k) = s * il;
            if (l == k) { w.grL(k, k) = lk; rdiag[k] = il; }
            NTM_WSYNC();
        }
        return true;
    }
}
// lane i holds b_i in `v`; returns x_i of L x = b (L lower, rdiag = 1/diag)
template <int P>
__device__ __forceinline__ double fwd_lanes(const double* L, const double* rdiag, int n, int RS, int CS, double v, int l) {
    double acc = (l < n) ? v : 0.0, x = 0.0;
    for (int k = 0; k < n; ++k) {
        double xk = gbcast<P>(acc, k) * rdiag[k];
        if (l == k) x = xk;
        if (l > k && l < n) acc -= L[l * RS + k * CS] * xk;
    }
    return x;
}
// lane i holds b_i in `v`; returns x_i of L' x = b (L lower, rdiag = 1/diag)
template <int P>
__device__ __forceinline__ double bwd_lanes(const double* L, const double* rdiag, int n, int RS, int CS, double v, int l) {
    double acc = (l < n) ? v : 0.0, x = 0.0;
    for (int k = n - 1; k >= 0; --k) {
        double xk = gbcast<P>(acc, k) * rdiag[k];
        if (l == k) x = xk;
        if (l < k) acc -= L[k * RS + l * CS] * xk;
    }
    return x;
}

// ---------------------------------------------------------------------------
// Goldfarb-Idnani dual active set on the Jacobi-scaled problem.
//   min 1/2 V'G~V + F~'V  s.t.  n_i'V >= bc_i (rows from the provider)
// Pre:  w.R() holds G~ (lower, col-major), w.F() holds F~, w.aflag() cleared.
// Post: w.V() holds V, w.act()[0..*q_out) the active rows; returns the quadprog
// exit flag.  Adds use a Householder reflector on J's trailing columns (one
// reduction instead of a Givens chain); drops restore R with a Givens sweep
// (Goldfarb & Idnani 1983, section 3).
// ---------------------------------------------------------------------------
template <int P, class Rows, class W>
__device__ __forceinline__ int gi_solve(const W& w, const Rows rows, bool has_rows, int nrows, int l, int* iters_out, int* q_out,
                        int nwarm = 0) {
    const int N = w.n();
    const int JR = w.jr(), JC = w.jc();     // J(r, c) at r JR + c JC (T alike)
    *iters_out = 0;
    *q_out = 0;
    NTM_T0(tg);
    // 1. Cholesky G~ = L L' (in place in w.R())
    if (!chol_gr<P>(w, N, l, w.ldi())) return NTM_EXIT_NONFINITE;
    // 2. J = L^{-T}: lane c computes row c of J (= column c of L^{-1})
    if (l < N) {
        for (int i = 0; i < N; ++i) {
            double x = 0.0;
            if (i >= l) {
                x = sub_dot<NTM_CH>((i == l) ? 1.0 : 0.0, w.grow(i), w.grs(), w.J() + l * JR, JC, l, i);
                x *= w.ldi()[i];
            }
            w.J()[l * JR + i * JC] = x;
        }
    }
    NTM_WSYNC();
    // 3. unconstrained minimiser V = -J J' F~
    double Vl = 0.0;
    {
        double t = 0.0;
        if (l < N) t = dot_batched<NTM_CH>(w.J() + l * JC, JR, w.F(), 1, N);
        if (l < N) w.d()[l] = t;
        NTM_WSYNC();
        if (l < N) {
            const double v = dot_batched<NTM_CH>(w.J() + l * JR, JC, w.d(), 1, N);
            Vl = -v;
            w.V()[l] = Vl;
            w.U()[l] = w.D()[l] * Vl;
        }
        NTM_WSYNC();
    }
    NTM_ACC(ST_GI_FACT, tg);
    if (!has_rows) return NTM_EXIT_OPTIMAL;
    const bool useT = w.useT();
    if (useT && l < N) for (int b = 0; b < N; ++b) w.T()[l * JR + b * JC] = 0.0;
    const int max_iter = 10 * (N + nrows) + 50;
    int q = 0, it = 0;
    // Warm start: the rows w.sidx()[0..nwarm) of a failed
    // candidate are added first without primal steps (Householder on J, R and T
    // gain their columns), then V is set to the equality-constrained optimum on
    // that set, V = -J2 J2' F~ + J1 R^{-T} bc, with multipliers
    // u = R^{-1} (R^{-T} bc + J1' F~) (matvecs with T = R^{-1} for N <= 32,
    // triangular solves on R above).
    // Rows dependent on those already added are skipped (a failed candidate often
    // holds a state row and a bound row that fix the same variable).  If every
    // u >= 0 the pair satisfies GI's invariant (optimal for the active set, dual
    // feasible) and the iteration continues from it; otherwise the caller
    // re-forms G~ and runs GI cold.
    if (nwarm > 0 && has_rows) {
        NTM_CNT(CN_WARM_TRY);
        bool okw = true;
        for (int a = 0; a < nwarm; ++a) {
            const int p = uni<P>(w.sidx()[a]);
            int ej = -1;
            double esg = 0.0, bcp, dl = 0.0;
            if constexpr (Rows::kHasUnitRows) {
                ej = uni<P>(rows.unit_row(p, N, esg));
                esg = uni<P>(esg);
            }
            if (ej >= 0) {                        // u-bound row: n_p = -+e_j, d = J' n_p a signed row of J
                bcp = uni<P>(-(rows.bval(w, p) / rows.rnorm(w, p)));
                if (l < N) dl = esg * w.J()[ej * JR + l * JC];
            } else {
                bcp = uni<P>(rows.template load_np<P>(w, p, l));
                if (l < N) dl = dot_batched<NTM_CH>(w.J() + l * JC, JR, w.np(), 1, N);
            }
            if (l < N) { w.d()[l] = (l >= q) ? dl : 0.0; w.dr()[l] = (l < q) ? dl : 0.0; }
            NTM_WSYNC();
            double rl = 0.0;
            if (useT && l < N) rl = dot_batched<NTM_CH>(w.T() + l * JR, JC, w.dr(), 1, N);
            const double zn = gsum<P>((l >= q && l < N) ? dl * dl : 0.0);
            const double dnrm = gsum<P>(dl * dl);
            if (q >= N) { NTM_CNT(CN_WARM_FULL); break; }
            if (zn <= 1e-300 || zn <= (kDepTol * kDepTol) * dnrm) {   // dependent on the rows added: skip it
                NTM_CNT(CN_WARM_DEP);
                NTM_WSYNC();
                continue;
            }
            const double nrm = sqrt(zn);
            const double dqv = gbcast<P>(dl, q);
            double h = dqv;
            if (q < N - 1) {
                h = (dqv >= 0.0) ? -nrm : nrm;
                double vl = (l == q) ? dl - h : ((l > q && l < N) ? dl : 0.0);
                if (l < N) w.hv()[l] = vl;
                double vtv = gsum<P>(vl * vl);
                NTM_WSYNC();
                if (l < N) {
                    const double dot = dot_batched<NTM_CH>(w.J() + l * JR, JC, w.hv(), 1, N);
                    const double f = 2.0 * dot / vtv;
                    axpy_sub<NTM_CH>(w.J() + l * JR, w.hv(), f, q, N, JC);
                }
            }
            const double ih = 1.0 / h;
            if (l < q) {
                w.gr(l, q) = dl;
                if (useT) w.T()[l * JR + q * JC] = -rl * ih;
            }
            if (l == q) {
                w.gr(q, q) = h;
                if (useT) w.T()[q * JR + q * JC] = ih;
                w.act()[q] = p;
                w.aflag()[p] = kActiveRow;
                w.Vb()[q] = bcp;                     // bc of active row q (scratch)
            }
            ++q;
            NTM_WSYNC();
        }
        if (okw) {
            // c = J' F~ (lane k), wv = (T' bc)_k for k < q
            double c = 0.0, wv = 0.0;
            if (l < N) c = dot_batched<NTM_CH>(w.J() + l * JC, JR, w.F(), 1, N);
            if (useT) {
                if (l < q) wv = dot_range<NTM_CH>(w.T() + l * JC, JR, w.Vb(), 1, 0, l + 1);
            } else {                                 // long horizons: R' wv = bc by forward substitution
                double acc = (l < q) ? w.Vb()[l] : 0.0;
                for (int k2 = 0; k2 < q; ++k2) {
                    const double xk = gbcast<P>(acc, k2) / w.gr(k2, k2);
                    if (l == k2) wv = xk;
                    if (l > k2 && l < q) acc -= w.gr(k2, l) * xk;
                }
            }
            if (l < N) {
                w.d()[l] = (l >= q) ? c : 0.0;
                w.dr()[l] = (l < q) ? wv : 0.0;
                w.np()[l] = (l < q) ? wv + c : 0.0;
            }
            NTM_WSYNC();
            double v = 0.0, u = 0.0;
            if (l < N) for (int k2 = 0; k2 < N; ++k2) v += w.J()[l * JR + k2 * JC] * (w.dr()[k2] - w.d()[k2]);
            if (useT) {
                if (l < q) u = dot_range<NTM_CH>(w.T() + l * JR, JC, w.np(), 1, l, q);
            } else {                                 // R u = wv + c1 by back substitution
                double acc = (l < q) ? w.np()[l] : 0.0;
                for (int b = q - 1; b >= 0; --b) {
                    const double ub = gbcast<P>(acc, b) / w.gr(b, b);
                    if (l == b) u = ub;
                    if (l < b) acc -= w.gr(l, b) * ub;
                }
            }
            const double uabs = gmax<P>(l < q ? fabs(u) : 0.0);
            const double umin = -gmax<P>(l < q ? -u : -kInf);
            okw = !(umin < -1e-9 * fmax(1.0, uabs)) && !gany<P>(l < N && !isfinite(v));
            if (!okw) {
                NTM_CNT(CN_WARM_NEG);
                // the added rows whose multipliers are >= 0: the caller's second warm pass
                const int lane = threadIdx.x & 63;
                const unsigned long long gm = (P == 64) ? ~0ull : (((1ull << P) - 1ull) << (lane & ~(P - 1)));
                const bool keep = l < q && u >= 0.0;
                const unsigned long long bk = __ballot(keep) & gm;
                const int id = (l < q) ? w.act()[l] : 0;
                NTM_WSYNC();
                if (keep) w.sidx()[__popcll(bk & ((1ull << lane) - 1ull))] = id;
                *q_out = uni<P>((int)__popcll(bk));
            }
            if (okw) {
                Vl = (l < N) ? v : 0.0;
                if (l < N) { w.V()[l] = Vl; w.U()[l] = w.D()[l] * Vl; }
                if (l < q) w.uu()[l] = fmax(0.0, u);
                NTM_CNT(CN_WARM_OK);
            }
            NTM_WSYNC();
        }
        if (!okw) {
            if (l < q) w.aflag()[w.act()[l]] = kCandRow;   // back to steering flags
            NTM_WSYNC();
            return kGiWarmRejected;                        // *q_out: rows kept in w.sidx() (0: none)
        }
    }
    NTM_ACC(ST_GI_WARM, tg);                               // the warm start's adds (not the first check)
    for (;;) {
        const double vmax = gmax<P>(l < N ? fabs(Vl) : 0.0);
        Pick pk = rows.template check<P>(w, Vl, l, false, fmax(1.0, vmax));
        NTM_ACC(ST_GI_CHECK, tg);
        NTM_CNT(CN_CHECK);
        NTM_TRACE("GI it %d q %d pick %d s %.6e bc %.6e\n", it, q, pk.p, pk.s, pk.bc);
        if (pk.p < 0 || pk.s >= -1e-12 * fmax(fmax(1.0, vmax), fabs(pk.bc))) {
            *iters_out = it;
            *q_out = q;
            return NTM_EXIT_OPTIMAL;
        }
        const int p = pk.p;
        const double bcp = uni<P>(rows.template load_np<P>(w, p, l));
        // u-bound rows have n_p = -+e_j: d = J' n_p is then a signed row of J
        int ej = -1;
        double esg = 0.0;
        if constexpr (Rows::kHasUnitRows) {
            ej = uni<P>(rows.unit_row(p, N, esg));
            esg = uni<P>(esg);
        }
        double upq = 0.0;   // multiplier of the constraint being added
        for (;;) {
            if (++it > max_iter) { *iters_out = it; *q_out = q; return NTM_EXIT_MAXITER; }
            // d = J' n_p
            double dl = 0.0;
            if (ej >= 0) {
                if (l < N) dl = esg * w.J()[ej * JR + l * JC];
            } else if (l < N) {
                dl = dot_batched<NTM_CH>(w.J() + l * JC, JR, w.np(), 1, N);
            }
            // d split at q: d2 = d[q:N] (w.d) and d1 = d[0:q] (w.dr), zero elsewhere, so
            // both matvecs run full fixed-length rows (unrolled, loads batched)
            if (l < N) { w.d()[l] = (l >= q) ? dl : 0.0; w.dr()[l] = (l < q) ? dl : 0.0; }
            NTM_WSYNC();
            // z = J2 d2 (primal direction) and r = T d1 = R^{-1} d1 (negative dual direction)
            double zl = 0.0, rl = 0.0;
            if (l < N) {
                zl = dot_batched<NTM_CH>(w.J() + l * JR, JC, w.d(), 1, N);
                if (useT) rl = dot_batched<NTM_CH>(w.T() + l * JR, JC, w.dr(), 1, N);
            }
            if (!useT) {                       // long horizons: back substitution on R
                double acc = (l < q) ? dl : 0.0;
                for (int b = q - 1; b >= 0; --b) {
                    const double rb = gbcast<P>(acc, b) / w.gr(b, b);
                    if (l == b) rl = rb;
                    if (l < b) acc -= w.gr(l, b) * rb;
                }
            }
            // partial (dual) step length t1
            double ratio = (l < q && rl > 0.0) ? w.uu()[l] / rl : kInf;
            int li = l;
            gargmin<P>(ratio, li);
            const double t1 = ratio;
            // full (primal) step length t2.  z'n_p = |d2|^2 exactly (z = J2 d2),
            // never negative; n_p counts as dependent on the active rows when
            // |d2| <= kDepTol |d|
            double npl = (l < N) ? w.np()[l] : 0.0;
            double zn = gsum<P>((l >= q && l < N) ? dl * dl : 0.0);
            double sp = gsum<P>(npl * Vl) - bcp;
            double dnrm = gsum<P>(dl * dl);
            double t2 = (zn <= 1e-300 || zn <= (kDepTol * kDepTol) * dnrm) ? kInf : -sp / zn;
            double t = fmin(t1, t2);
            NTM_TRACE("   dir: t1 %.6e (pos %d) t2 %.6e zn %.6e dn %.6e sp %.6e\n", t1, li, t2, zn, dnrm, sp);
            NTM_ACC(ST_GI_DIR, tg);
            if (!(t < kInf)) { *iters_out = it; *q_out = q; return NTM_EXIT_INFEASIBLE; }
            if (l < q) w.uu()[l] = fmax(0.0, w.uu()[l] - t * rl);
            upq += t;
            if (t2 < kInf) {
                Vl += t * zl;
                if (l < N) { w.V()[l] = Vl; w.U()[l] = w.D()[l] * Vl; }
                if (t == t2) {
                    // ---- add p: Householder on d[q:N] -> J(:, q:N) ----
                    double dq2 = (l >= q && l < N) ? dl * dl : 0.0;
                    double nrm = sqrt(gsum<P>(dq2));
                    double dqv = gbcast<P>(dl, q);
                    double h = dqv;
                    if (q < N - 1 && nrm > 0.0) {
                        h = (dqv >= 0.0) ? -nrm : nrm;
                        double vl = (l == q) ? dl - h : ((l > q && l < N) ? dl : 0.0);
                        if (l < N) w.hv()[l] = vl;          // zero for l < q
                        double vtv = gsum<P>(vl * vl);
                        NTM_WSYNC();
                        if (l < N) {
                            const double dot = dot_batched<NTM_CH>(w.J() + l * JR, JC, w.hv(), 1, N);
                            const double f = 2.0 * dot / vtv;
                            axpy_sub<NTM_CH>(w.J() + l * JR, w.hv(), f, q, N, JC);
                        }
                    }
                    // R gains column q = [d1; h]; T = R^{-1} gains column q = [-r/h; 1/h]
                    const double ih = 1.0 / h;
                    if (l < q) {
                        w.gr(l, q) = dl;
                        if (useT) w.T()[l * JR + q * JC] = -rl * ih;
                    }
                    if (l == q) {
                        w.gr(q, q) = h;
                        if (useT) w.T()[q * JR + q * JC] = ih;
                        w.act()[q] = p;
                        w.aflag()[p] = kActiveRow;
                        w.uu()[q] = upq;
                    }
                    ++q;
                    NTM_WSYNC();
                    NTM_ACC(ST_GI_ADD, tg);
                    break;
                }
            }
            // ---- drop active position li (partial or dual-only step) ----
            const int l0 = li;
            const int dropped = uni<P>(w.act()[l0]);
            NTM_WSYNC();
            if (l < q) {
                // column shift: rows l <= c + 1 (R upper, plus the subdiagonal the shift
                // creates); the rows below are zero and, in the packed LDS storage
                // (kGiLds), share their slots with the upper triangle
                for (int c = l0; c < q - 1; ++c)
                    if (!W::kGiLds || l <= c + 1) w.gr(l, c) = w.gr(l, c + 1);
                w.gr(l, q - 1) = 0.0;
            }
            {
                int an = 0;
                double un = 0.0;
                if (l >= l0 && l < q) { an = w.act()[l + 1]; un = w.uu()[l + 1]; }
                NTM_WSYNC();
                if (l >= l0 && l < q) { w.act()[l] = an; w.uu()[l] = un; }
                if (l == 0) w.aflag()[dropped] = 0;
            }
            NTM_WSYNC();
            for (int j = l0; j < q - 1; ++j) {
                double a = uni<P>(w.gr(j, j)), bq = uni<P>(w.gr(j + 1, j));
                double hh = hypot(a, bq);
                double cc = 1.0, ss = 0.0;
                if (hh != 0.0) { cc = a / hh; ss = bq / hh; }
                NTM_WSYNC();
                if (l >= j && l < q - 1) {
                    double r1 = w.gr(j, l), r2 = w.gr(j + 1, l);
                    double nr = cc * r1 + ss * r2;
                    w.gr(j, l) = nr;
                    w.gr(j + 1, l) = (l == j) ? 0.0 : (-ss * r1 + cc * r2);
                }
                if (l < N) {
                    double j1 = w.J()[l * JR + j * JC], j2 = w.J()[l * JR + (j + 1) * JC];
                    w.J()[l * JR + j * JC] = cc * j1 + ss * j2;
                    w.J()[l * JR + (j + 1) * JC] = -ss * j1 + cc * j2;
                }
                if (useT && l < q) {   // T <- T G_j' (the columns rotate like J's)
                    double t1v = w.T()[l * JR + j * JC], t2v = w.T()[l * JR + (j + 1) * JC];
                    w.T()[l * JR + j * JC] = cc * t1v + ss * t2v;
                    w.T()[l * JR + (j + 1) * JC] = -ss * t1v + cc * t2v;
                }
                NTM_WSYNC();
            }
            // R'^{-1} = (T Q) without row l0 and column q-1.  Lane c owns column c:
            // rows l0+1..q-1 move up one; the discarded column q-1 is cleared
            if (useT && l < q - 1) {
                for (int a = l0; a < q - 1; ++a) w.T()[a * JR + l * JC] = w.T()[(a + 1) * JR + l * JC];
                w.T()[(q - 1) * JR + l * JC] = 0.0;
            } else if (useT && l == q - 1) {
                for (int a = 0; a < q; ++a) w.T()[a * JR + l * JC] = 0.0;
            }
            NTM_WSYNC();
            --q;
            NTM_ACC(ST_GI_DROP, tg);
        }
    }
}

// ---------------------------------------------------------------------------
// Exact re-solve on GI's final active set (oracle: polish_active_set).
//   Rows with a single non-zero fix their variable exactly (U_j = b/Lin_j);
//   the other active rows S are equality constraints on the free variables:
//   masked Cholesky of G~ (fixed rows/cols -> identity), Schur complement
//   K = E G~_FF^{-1} E', then V_F.  Accepted only if the KKT certificate
//   holds; otherwise w.U() keeps GI's solution.  Pre: w.V() = GI solution.
//   Writes w.U() (unscaled U).  G~ comes from Gamma (gram, structured rows) or
//   from Gsave (a copy taken before the GI factorisation, dense rows).
//   lam_out (optional, one entry per row; may alias the rows' norm array): the
//   multipliers of a certified set, unscaled (mu_i / rn_i) and zero on the other
//   rows, written only on success.
// ---------------------------------------------------------------------------
template <int P, class Rows, class W>
__device__ __forceinline__ bool polish_phase(const Prob& pb, const W& w, const Rows* rows, int q, int l,
                             const double* Gsave, bool g_in_R, bool verify_only, int* ns_out,
                             double* lam_out = nullptr) {
    const int N = w.n(), LD = w.ldj(), LDJ = w.ldj();
    const double Vgi = (l < N) ? w.V()[l] : 0.0;
    // --- classify active rows ---
    if (l < N) w.fx()[l] = 0;
    NTM_WSYNC();
    int isgen = 0, fixj = -1;
    double ufix = 0.0;
    int id = -1;
    if (l < q) {
        id = w.act()[l];
        int nnz = 0;
        for (int j = 0; j < N; ++j) if (rows->lin(w, id, j) != 0.0) { ++nnz; fixj = j; }
        if (nnz == 1) ufix = rows->bval(w, id) / rows->lin(w, id, fixj);
        else isgen = 1;
    }
    double nfix = 0.0;   // GI normal entry of the single-entry row (for its multiplier)
    if (l < q && !isgen) nfix = -((rows->lin(w, id, fixj) * w.D()[fixj]) / rows->rnorm(w, id));
    const unsigned long long gmask = (P == 64) ? ~0ull : (((1ull << P) - 1ull) << ((threadIdx.x & 63) & ~(P - 1)));
    const unsigned long long bal = __ballot(isgen) & gmask;
    const int nS = __popcll(bal);
    const int spos = __popcll(bal & ((1ull << (threadIdx.x & 63)) - 1ull));
    if (l < q) {
        if (isgen) w.sidx()[spos] = id;
        else { w.fx()[fixj] = 1; w.Uf()[fixj] = ufix; w.hv()[fixj] = nfix; }
    }
    NTM_WSYNC();
    const bool fixed = (l < N) && w.fx()[l];
    const double vb = fixed ? w.Uf()[l] / w.D()[l] : 0.0;
    if (l < N) w.Vb()[l] = vb;
    if (ns_out) *ns_out = nS;
    // --- G~ again (bit-identical to the GI's copy), g = F~ + G~_{:,B} V_B ---
    if (g_in_R) {
        // candidate verification: G~ is still intact in w.R()
    } else if (Gsave) {
        if (l < N) for (int j = 0; j <= l; ++j) w.R()[l + j * LD] = Gsave[l + j * LD];
    } else {
        gram_rows<P>(pb, w, w.R(), l);
        NTM_WSYNC();
        (void)scale_gram<P>(w, w.R(), l);
    }
    NTM_WSYNC();
    double gl = 0.0;
    if (l < N) {
        gl = w.F()[l];
        for (int j = 0; j < N; ++j)
            if (w.fx()[j]) gl += ((j <= l) ? w.R()[l + j * LD] : w.R()[j + l * LD]) * w.Vb()[j];
        if (fixed) gl = 0.0;
    }
    NTM_WSYNC();
    if (l < N) {   // mask fixed rows/cols to identity (row l, columns <= l)
        for (int j = 0; j <= l; ++j)
            if (fixed || w.fx()[j]) w.R()[l + j * LD] = (j == l) ? 1.0 : 0.0;
    }
    NTM_WSYNC();
    bool ok = chol_inplace<P>(w.R(), N, 1, LD, l, w.ldi());
    double vfin = 0.0;
    if (ok) {
        double wl = fwd_lanes<P>(w.R(), w.ldi(), N, 1, LD, gl, l);      // w = L^{-1} g
        double tl = -wl;
        if (nS > 0) {
            // E' into Y (= w.J(), row-major N x nS), h_s
            if (l < N) {
                for (int s = 0; s < nS; ++s) {
                    int rid = w.sidx()[s];
                    double nj = -((rows->lin(w, rid, l) * w.D()[l]) / rows->rnorm(w, rid));
                    w.J()[l * LDJ + s] = fixed ? 0.0 : nj;
                }
            }
            double hs = 0.0;
            if (l < nS) {
                int rid = w.sidx()[l];
                double rn = rows->rnorm(w, rid);
                hs = -(rows->bval(w, rid) / rn);
                for (int j = 0; j < N; ++j)
                    if (w.fx()[j]) hs -= (-((rows->lin(w, rid, j) * w.D()[j]) / rn)) * w.Vb()[j];
            }
            if (l < N) w.d()[l] = wl;
            NTM_WSYNC();
            // Y = L^{-1} E' : lane s solves column s in place
            if (l < nS) {
                for (int i = 0; i < N; ++i) {
                    double y = w.J()[i * LDJ + l];
                    for (int k = 0; k < i; ++k) y -= w.R()[i + k * LD] * w.J()[k * LDJ + l];
                    w.J()[i * LDJ + l] = y * w.ldi()[i];
                }
            }
            NTM_WSYNC();
            // K = Y'Y (lower triangle stored transposed in R's strict upper part); rhs = h + Y'w
            double* K = w.R() + LD;
            double rhs = 0.0;
            if (l < nS) {
                for (int c = 0; c <= l; ++c) {
                    double sK = 0.0;
                    for (int i = 0; i < N; ++i) sK += w.J()[i * LDJ + l] * w.J()[i * LDJ + c];
                    K[l * LD + c] = sK;
                }
                rhs = hs;
                for (int i = 0; i < N; ++i) rhs += w.J()[i * LDJ + l] * w.d()[i];
            }
            NTM_WSYNC();
            ok = chol_inplace<P>(K, nS, LD, 1, l, w.kdi());
            if (ok) {
                double t1 = fwd_lanes<P>(K, w.kdi(), nS, LD, 1, rhs, l);
                double mu = bwd_lanes<P>(K, w.kdi(), nS, LD, 1, t1, l);
                if (l < nS) w.np()[l] = mu;
                NTM_WSYNC();
                if (l < N) {
                    double sY = 0.0;
                    for (int a = 0; a < nS; ++a) sY += w.J()[l * LDJ + a] * w.np()[a];
                    tl = sY - wl;
                }
            }
        }
        if (ok) {
            double vl = bwd_lanes<P>(w.R(), w.ldi(), N, 1, LD, tl, l);  // V_F = L^{-T} t
            vfin = fixed ? vb : vl;
        }
    }
    // ok is group-uniform already: chol_inplace decides on a broadcast pivot, and
    // the collectives of the solves above ran under it
    if (ok && Gsave) {
        // One step of fixed-precision iterative refinement on the KKT residual with
        // the same factors.  The range-space solve goes through L = chol(G~_FF),
        // which loses digits when G~_FF is nearly singular although the KKT system
        // is well conditioned (input-rate rows holding the last inputs: up to
        // ~1e-8 umax off the exact optimum); the residual of the well-conditioned
        // system, solved again, restores them.  Correction (dV, dmu):
        //   G~_FF dV - E' dmu = -r1,  r1 = G~V + F~ - E'mu (free variables)
        //   E dV = -r2,               r2 = n_s'V - bc_s   (general rows)
        if (l < N) w.V()[l] = vfin;
        NTM_WSYNC();
        double r1 = 0.0, r2 = 0.0;
        if (l < N && !fixed) {
            r1 = w.F()[l];
            for (int j = 0; j < N; ++j) r1 += ((j <= l) ? Gsave[l + j * LD] : Gsave[j + l * LD]) * w.V()[j];
            for (int s = 0; s < nS; ++s) {
                const int rid = w.sidx()[s];
                r1 -= w.np()[s] * (-((rows->lin(w, rid, l) * w.D()[l]) / rows->rnorm(w, rid)));
            }
        }
        if (l < nS) {
            const int rid = w.sidx()[l];
            const double rn = rows->rnorm(w, rid);
            double nv = 0.0;
            for (int j = 0; j < N; ++j) nv += (-((rows->lin(w, rid, j) * w.D()[j]) / rn)) * w.V()[j];
            r2 = nv + rows->bval(w, rid) / rn;
        }
        const double dwl = fwd_lanes<P>(w.R(), w.ldi(), N, 1, LD, r1, l);
        double dt = -dwl;
        if (nS > 0) {
            if (l < N) w.d()[l] = dwl;
            NTM_WSYNC();
            double rhs = 0.0;
            if (l < nS) {
                rhs = -r2;
                for (int i = 0; i < N; ++i) rhs += w.J()[i * LDJ + l] * w.d()[i];
            }
            const double* K = w.R() + LD;
            const double t1 = fwd_lanes<P>(K, w.kdi(), nS, LD, 1, rhs, l);
            const double dmu = bwd_lanes<P>(K, w.kdi(), nS, LD, 1, t1, l);
            NTM_WSYNC();
            if (l < nS) {
                w.d()[l] = dmu;
                w.np()[l] += dmu;
            }
            NTM_WSYNC();
            if (l < N) {
                double sY = 0.0;
                for (int a = 0; a < nS; ++a) sY += w.J()[l * LDJ + a] * w.d()[a];
                dt = sY - dwl;
            }
        }
        const double dv = bwd_lanes<P>(w.R(), w.ldi(), N, 1, LD, dt, l);
        const double vr = fixed ? vb : vfin + dv;
        ok = !gany<P>(l < N && !isfinite(vr));
        if (ok) vfin = vr;
    }
    if (ok) {
        // ---- KKT certificate ----
        if (l < N) w.V()[l] = vfin;
        NTM_WSYNC();
        double vmax = gmax<P>(l < N ? fabs(vfin) : 0.0);
        Pick vf = rows->template check<P>(w, vfin, l, true, fmax(1.0, vmax));
        ok = vf.p == 0;
        // gradient G~V + F~ (G~ itself is factored now)
        double res = 0.0;
        if (Gsave) {
            if (l < N) {
                res = w.F()[l];
                for (int j = 0; j < N; ++j)
                    res += ((j <= l) ? Gsave[l + j * LD] : Gsave[j + l * LD]) * w.V()[j];
            }
        } else {
            // through Gamma: y = Gamma (D V), grad_j = D_j 2 Gamma_j' Om y + F~_j
            for (int r = l; r < 2 * N; r += P) {
                double y = 0.0;
                for (int j = 0; j <= (r >> 1); ++j) y += w.gt(r, j) * (w.D()[j] * w.V()[j]);
                w.xp()[r] = y;              // scratch: xp is rewritten by the rollout
            }
            NTM_WSYNC();
            if (l < N) {
                double g2 = 0.0;
                for (int i = l; i < N; ++i) {
                    double y0 = w.xp()[2 * i], y1 = w.xp()[2 * i + 1];
                    double o0 = pb.Q[0] * y0 + pb.Q[1] * y1, o1 = pb.Q[2] * y0 + pb.Q[3] * y1;
                    g2 += w.gt(2 * i, l) * o0 + w.gt(2 * i + 1, l) * o1;
                }
                res = w.D()[l] * (2 * g2) + w.F()[l];
            }
        }
        if (l < N) {
            for (int s = 0; s < nS; ++s) {
                int rid = w.sidx()[s];
                res -= w.np()[s] * (-((rows->lin(w, rid, l) * w.D()[l]) / rows->rnorm(w, rid)));
            }
        }
        // multipliers: mu_s (general rows) and res_j / n_j (fixed variables)
        double mval = 0.0;
        bool has = false;
        if (l < nS) { mval = w.np()[l]; has = true; }
        if (fixed) {
            double lam = res / w.hv()[l];
            mval = has ? fmin(mval, lam) : lam;
            has = true;
        }
        double mabs = gmax<P>(has ? fabs(mval) : 0.0);
        // the smallest multiplier only feeds this comparison: a predicate per lane
        // (a NaN multiplier compares false here, as fmax dropped it from the minimum)
        ok = ok && !gany<P>(has && mval < -1e-9 * fmax(1.0, mabs));
        if (lam_out && ok) {
            // the certified set's multipliers in the caller's units (quadprog's
            // lambda.ineqlin: mu / rn), by row id.  Every lane forms its entries
            // before lam_out is written, so lam_out may be the row norms' own array
            if (fixed) w.d()[l] = res / w.hv()[l];
            NTM_WSYNC();
            int i1 = -1, i2 = -1;
            double v1 = 0.0, v2 = 0.0;
            if (l < nS) { i1 = w.sidx()[l]; v1 = w.np()[l] / rows->rnorm(w, i1); }
            if (l < q && !isgen) { i2 = id; v2 = w.d()[fixj] / rows->rnorm(w, id); }
            NTM_WSYNC();
            for (int i = l; i < rows->rows(); i += P) lam_out[i] = 0.0;
            NTM_WSYNC();
            if (i1 >= 0) lam_out[i1] = v1;
            if (i2 >= 0) lam_out[i2] = v2;
            NTM_WSYNC();
        }
    }
    if (verify_only && !ok) {
        if (l < N) w.V()[l] = Vgi;
        NTM_WSYNC();
        return false;
    }
    if (l < N) {
        double u;
        if (ok) u = fixed ? w.Uf()[l] : vfin * w.D()[l];
        else u = Vgi * w.D()[l];
        w.U()[l] = u;
        w.V()[l] = ok ? vfin : Vgi;
    }
    NTM_WSYNC();
    return ok;
}

// ---------------------------------------------------------------------------
// Exact re-solve on an active set, compact form for the implicit getWLc rows
// (oracle: polish_active_set).  Used both to VERIFY a warm-start candidate
// (the active set of LPV iteration it-2) and to POLISH the Goldfarb-Idnani
// result.  Single-entry rows fix their variable exactly (U_j = b/Lin_j); the
// nF free variables and the nS general (state) rows form a small KKT system
//   min 1/2 V_F' G~_FF V_F + g_F' V_F  s.t. E V_F = h
// solved in compact nF / nS coordinates: G~_FF from Gamma's free columns
// (bit-identical entries to the full Gram), g_F = D_F 2 Gamma_F' Om (Gamma U_B
// + e - r) by two O(N) passes, Cholesky of G~_FF, Schur complement
// K = E G~_FF^{-1} E'.  Accepted only if the KKT certificate holds (primal
// slack on every row, multiplier signs).  Writes w.U()/w.V() on success or
// when !verify_only (then GI's V is kept); returns success.
// ---------------------------------------------------------------------------
// fail_kind / fail_pos (optional): after a FAILED certificate, its kind (1 dual, 2
// primal, 3 singular, 4 both) and the active-list position of the most negative
// multiplier (kinds 1, 2, 4).  fail_pos is defined only then: a certified set runs
// no argmin and leaves 0 there, so a caller must not read it on success.
// mult_out (optional, LDS): every active row's multiplier (GI form, n'V >= bc rows),
// by active position, written when the certificate's multipliers are formed.
// dir_p >= 0 (the certified dual path of qp_phase): no solve at all.  The active
// set of q rows must be echelon (sq); the certificate's multiplier pass then runs
// with row dir_p's normal n_p in place of the gradient, i.e. it writes to mult_out
// the r with sum_i r_i n_i = n_p (n_p dependent on the set: Goldfarb-Idnani's
// dual-only step direction).  Returns false for any other set.  V and U are left
// untouched.
template <int P, class W>
__device__ __forceinline__ bool polish_compact(const Prob& pb, const W& w, const StructRows rows, int q, int l, bool verify_only,
                               int* ns_out, int* fail_kind = nullptr, int* fail_pos = nullptr,
                               double* v_out = nullptr, double* mult_out = nullptr, int dir_p = -1) {
    const int N = w.n(), LD = w.ldj(), LDJ = w.ldj();
    // false: no rate rows in this kernel, so no general-row code r >= 2N and no kind >= 4.
    // A constant in front of the plain tests, not a method of rows: a call from the
    // lambdas below changes their captures, and with them the code of every unit
    constexpr bool kRate = rate_rows<W>();
    const OmQ<qi_on<W>()> om(pb.Q);
    const bool dir = dir_p >= 0;
    const double Vprev = (l < N) ? w.V()[l] : 0.0;
    NTM_T0(tp);
    // --- classify active rows: single-entry rows fix a variable, the rest are general ---
    if (l < N) w.fx()[l] = 0;
    NTM_WSYNC();
    int isgen = 0, fixj = -1, id = -1, srow = 0, constrow = 0;
    double ufix = 0.0, nfix = 0.0, ssign = 0.0;
    if (l < q) {
        id = w.act()[l];
        int kind, j;
        rows.template decode<kRate>(id, N, kind, j);
        if (kind < 2) {                                   // u bound: Lin = -+e_j, b = -umin / umax
            fixj = j;
            // lv = -+1: b / lv is -+b exactly, and -((lv D_j) / D_j) is -lv exactly (D_j
            // is finite and non-zero: a non-finite scale left with NTM_EXIT_NONFINITE)
            const double bv = rows.bval(w, id);
            ufix = kind == 0 ? -bv : bv;
            nfix = kind == 0 ? 1.0 : -1.0;
        } else if (kRate && kind >= 4) {                  // rate row: Lin = sg (e_j - e_{j-1})
            isgen = 1;
            srow = 2 * N + j;                             // general-row code >= 2N: rate row j
            ssign = (kind == 4) ? 1.0 : -1.0;
        } else {                                          // state row r = j: Lin = -+Gamma_r
            const double sg = (kind == 2) ? -1.0 : 1.0;
            // an x_0 row (j < 0) or a state row Gamma doesn't reach has Lin = 0: a
            // constant row is never active (a caller's or a shifted candidate can
            // hold one); the set is rejected like a colliding one
            const int info = (j >= 0) ? w.rinfo()[j] : 0;  // scaling pass: last non-zero column
            const int jj = (info & (kRowMulti - 1)) - 1;
            const int nnz = (info & kRowMulti) ? 2 : (jj >= 0 ? 1 : 0);
            if (nnz == 0) {
                constrow = 1;
            } else if (nnz == 1) {
                double lv = sg * w.gt(j, jj);
                fixj = jj;
                ufix = rows.bval(w, id) / lv;
                nfix = -((lv * w.D()[jj]) * w.irn()[j]);
            } else {
                isgen = 1;
                srow = j;
                ssign = sg;
            }
        }
    }
    NTM_ACC(ST_C_A, tp);
    const int lane = threadIdx.x & 63;
    const unsigned long long gmask = (P == 64) ? ~0ull : (((1ull << P) - 1ull) << (lane & ~(P - 1)));
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long bal = __ballot(isgen) & gmask;
    const int nS = uni<P>((int)__popcll(bal));
    if (ns_out) *ns_out = nS;
    if (l < q) {
        if (isgen) {
            const int k = __popcll(bal & below);
            w.sidx()[k] = l;                              // its position in the active list
            w.srw()[k] = srow;
            w.ssg()[k] = ssign;
        } else if (!constrow) {
            w.fx()[fixj] = (unsigned char)(l + 1);       // tagged by the writing lane
            w.Uf()[fixj] = ufix;
            w.hv()[fixj] = nfix;
        }
    }
    NTM_WSYNC();
    // two active rows fixing one variable (only a caller-supplied candidate can
    // do that; GI never adds a dependent row) cannot be certified: reject; so is a
    // set holding a constant row
    const bool collide = gany<P>(l < q && !isgen && (constrow || w.fx()[fixj] != (unsigned char)(l + 1)));
    const bool fixed = (l < N) && w.fx()[l];
    const double uf = fixed ? w.Uf()[l] : 0.0;
    const double vb = fixed ? uf / w.D()[l] : 0.0;
    if (l < N) {
        w.Vb()[l] = vb;
        w.dr()[l] = uf;                                   // U_B: fixed values, 0 on free variables
    }
    // --- compact map of the free variables ---
    bal = __ballot((l < N) && !fixed) & gmask;
    const int nF = uni<P>((int)__popcll(bal));
    const int fpos = __popcll(bal & below);
    if (l < N && !fixed) w.fidx()[fpos] = l;
    // --- y_B = Gamma U_B (fixed variables only; scratch in w.Phi(), dead until the
    //     next lift) and z = y_B + e - r (scratch in w.xp(), rewritten by the rollout) ---
    NTM_WSYNC();
    NTM_ACC(ST_C_B, tp);
    // Every variable fixed by a bound (no free variable, no general row: the box-only
    // QPs of BASELINE config 2 hold 19.8 of 20 inputs at a bound): Gamma U_B is the
    // certificate's y = Gamma U already, so the pass below writes it where the
    // certificate reads it and the certificate skips its own Gamma U pass (the
    // all-LDS and generic builds; the far N = 20 / 50 kernels keep one code path)
    constexpr bool kFixedY = !W::kFar;
    const bool allfixed = kFixedY && nF == 0 && nS == 0;
    // Long horizons: the pass runs after the set's shape is known; an
    // echelon set needs Gamma_r U_B only at its active general rows (h), at most N < P
    // of them, so one trip over those rows replaces two over all 2N (z = y_B + e - r,
    // which only the bordered path's g_F reads, is not formed)
    constexpr bool kLateY = W::kNN > 32 && P == 64;
    if constexpr (!kLateY) {
        for (int r = l; r < 2 * N && !dir; r += P) {
            const double y = gamma_row_dot<NTM_CH, P>(w, r, w.dr());
            w.Phi()[r] = y;
            w.xp()[r] = allfixed ? y : y + w.e()[r] - ((r & 1) ? pb.r[1] : pb.r[0]);
        }
    }
    NTM_WSYNC();
    NTM_ACC(ST_C_Y, tp);
    // --- square, triangular E (nS == nF, the common "boundary arc": the state held
    //     at its bound by every free input).  The active general rows then pin the
    //     free variables down on their own: sorted by their last free variable they
    //     make E lower triangular with a non-zero diagonal, so V_F follows from
    //     E V_F = h by forward substitution and the multipliers from E' mu = grad_F
    //     by back substitution in the certificate; no Gram of the free columns and
    //     no bordered elimination.  perm[t] = the general row whose last free
    //     variable is the t-th (scratch ints in the R block; E goes to the J block).
    int* const perm = w.permi();                           // sorted row t -> general row
    int* const colrow = perm + (N + 1);                    // compact column -> row ending there
    bool sq = false;                                       // echelon path (k = nF - nS <= 1)
    int nc = -1;                                           // k = 1: the non-pivot compact column
    int nc2 = -1;                                          // k = 1 with one collision: the second hole
    int xb = -1;                                           // one collision: the row left out of the triangle
    int xb2 = -1;                                          // two collisions (k = 0): the second row left out
    int nc3 = -1;                                          // k = 2 with one collision: the third hole
    const int kdim = nF - nS;
#ifdef NTM_STAMPS
    int dg_orph = -1, dg_neg = 0;                          // diagnostic: the shape of a set left to the bordered path
#endif
    // a general row with no non-zero at a free column makes the KKT matrix singular
    // (its row of E is zero): rejected like a colliding set (fail kind 3) instead of
    // running the bordered elimination into a zero pivot (long horizons: N = 50 mode 2
    // met 0.11 such re-solves per MPC step, round 6)
    bool nofree = false;
    // Long horizons with rate rows (config 5) mostly give square sets with ONE
    // collision: two general rows (a rate row and a state row of the same stage)
    // end in the same free column, and one column has no row ending there (83% of
    // the N=50 mode-3 optima, none at N=20 mode 2).  Leaving one of the two rows out
    // makes the rest echelon with k = 1 (the hole as the non-pivot column); the row
    // left out then fixes the step along the null vector instead of the cost.
    constexpr bool kCollision = W::kNN == 0 || W::kNN > 32;
    // Echelon sets with two spare columns (k = 2, round 5; long horizons): the certified
    // dual path passes through them after a drop from a k = 1 set; V = V_0 + w1 Z1 + w2 Z2
    // is minimised over the plane (a 2 x 2 system) instead of the bordered elimination
    constexpr bool kPlane = kCollision;
    constexpr bool kColl2 = kCollision;   // square sets with two collisions on the null-space path
    // k = 2 with one collision (round 6): three holes and one row left out; the row
    // left out fixes one of the three spare directions, the cost is minimised over
    // the plane that remains (config 5 mode 3: 0.44 such sets per MPC step took the
    // bordered elimination)
    constexpr bool kColl3 = kPlane && NTM_COLL3;
    if ((kdim == 1 || (kdim == 0 && nS > 0) || (kPlane && kdim == 2 && nS > 0)) && !collide) {
        const unsigned long long fm = bal >> (lane & ~(P - 1));   // bit j: variable j is free
        int lastf = -1;
        if (l < nS) {
            const int r = w.srw()[l];
            int lj = -1;
            if (kRate && r >= 2 * N) {                         // rate row of input i: e_i - e_{i-1}
                const int i = r - 2 * N;
                lj = ((fm >> i) & 1ull) ? i : (((fm >> (i - 1)) & 1ull) ? i - 1 : -1);
            } else {                                           // state row r: from its last non-zero
                lj = (w.rinfo()[r] & (kRowMulti - 1)) - 1;     // column down to the first free one
                while (lj >= 0 && !(((fm >> lj) & 1ull) && w.gt(r, lj) != 0.0)) --lj;
            }
            if (lj >= 0) lastf = __popcll(fm & ((1ull << lj) - 1ull));
        }
        if (l < nF) colrow[l] = -1;
        NTM_WSYNC();
        if (lastf >= 0) colrow[lastf] = l;                     // a repeated last column leaves a hole
        NTM_WSYNC();
        const unsigned long long holes = __ballot(l < nF && colrow[l] < 0) & gmask;
        if constexpr (kCollision) nofree = (__ballot(l < nS && lastf < 0) & gmask) != 0;
#ifdef NTM_STAMPS
        dg_neg = (__ballot(l < nS && lastf < 0) & gmask) != 0;
        dg_orph = (int)__popcll(__ballot(l < nS && lastf >= 0 && colrow[lastf] != l) & gmask);
#endif
        if ((int)__popcll(holes) == kdim) {                    // every row ends in its own column
            sq = true;
            const unsigned long long hg = holes >> (lane & ~(P - 1));
            nc = kdim ? uni<P>((int)__ffsll((long long)hg) - 1) : -1;
            if (kPlane && kdim == 2) nc2 = uni<P>((int)__ffsll((long long)(hg & (hg - 1ull))) - 1);
            if (l < nS) {
                int c = l + ((nc >= 0 && l >= nc) ? 1 : 0);
                if (kPlane && nc2 >= 0 && c >= nc2) ++c;
                perm[l] = colrow[c];
            }
            NTM_WSYNC();
        } else if (kCollision && kdim <= (kColl3 ? 2 : 1) && (int)__popcll(holes) == kdim + 1 &&
                   (__ballot(l < nS && lastf < 0) & gmask) == 0) {
            // one row does not own its last column (the column's owner is the last writer):
            // k = 0 leaves one hole, k = 1 two (the triangle's spare column and the collision's),
            // k = 2 three
            const unsigned long long orph = __ballot(l < nS && colrow[lastf < 0 ? 0 : lastf] != l) & gmask;
            if ((int)__popcll(orph) == 1) {
                sq = true;
                const unsigned long long hg = holes >> (lane & ~(P - 1));
                const unsigned long long hg2 = hg & (hg - 1ull);
                nc = uni<P>((int)__ffsll((long long)hg) - 1);
                if (kdim >= 1) nc2 = uni<P>((int)__ffsll((long long)hg2) - 1);
                if (kColl3 && kdim == 2) nc3 = uni<P>((int)__ffsll((long long)(hg2 & (hg2 - 1ull))) - 1);
                xb = uni<P>((int)__ffsll((long long)(orph >> (lane & ~(P - 1)))) - 1);
                if (l < nS - 1) {
                    int c = l + (l >= nc ? 1 : 0);
                    if (nc2 >= 0 && c >= nc2) ++c;
                    if (kColl3 && nc3 >= 0 && c >= nc3) ++c;
                    perm[l] = colrow[c];
                }
                NTM_WSYNC();
            }
        } else if (kColl2 && kdim <= (kColl3 ? 1 : 0) && (int)__popcll(holes) == kdim + 2 &&
                   (__ballot(l < nS && lastf < 0) & gmask) == 0) {
            // two rows do not own their last columns (square set, two holes): leaving both
            // out leaves an echelon system with two spare columns, and the two rows left out
            // fix the step along the plane instead of the cost (round 5, rate rows at N = 50);
            // k = 1 leaves three holes, and the two rows fix a line (round 6, NTM_COLL3)
            const unsigned long long orph = __ballot(l < nS && colrow[lastf < 0 ? 0 : lastf] != l) & gmask;
            if ((int)__popcll(orph) == 2) {
                sq = true;
                const unsigned long long hg = holes >> (lane & ~(P - 1));
                const unsigned long long hg2 = hg & (hg - 1ull);
                nc = uni<P>((int)__ffsll((long long)hg) - 1);
                nc2 = uni<P>((int)__ffsll((long long)hg2) - 1);
                if (kColl3 && kdim == 1) nc3 = uni<P>((int)__ffsll((long long)(hg2 & (hg2 - 1ull))) - 1);
                const unsigned long long og = orph >> (lane & ~(P - 1));
                xb = uni<P>((int)__ffsll((long long)og) - 1);
                xb2 = uni<P>((int)__ffsll((long long)(og & (og - 1ull))) - 1);
                if (l < nS - 2) {
                    int c = l + (l >= nc ? 1 : 0);
                    if (c >= nc2) ++c;
                    if (kColl3 && nc3 >= 0 && c >= nc3) ++c;
                    perm[l] = colrow[c];
                }
                NTM_WSYNC();
            }
        }
    }
    if constexpr (kLateY) {
        if (!dir) {
            if (sq) {
                if (l < nS) {
                    const int r = w.srw()[l];
                    if (r < 2 * N) w.Phi()[r] = gamma_row_dot<NTM_CH>(w, r, w.dr());
                }
            } else {
                for (int r = l; r < 2 * N; r += P) {
                    const double y = gamma_row_dot<NTM_CH>(w, r, w.dr());
                    w.Phi()[r] = y;
                    w.xp()[r] = allfixed ? y : y + w.e()[r] - ((r & 1) ? pb.r[1] : pb.r[0]);
                }
            }
            NTM_WSYNC();
        }
    }
    NTM_ACC(ST_C_SQ, tp);
    if (dir && !sq) {                                      // the dual path's direction: echelon sets only
        if (fail_kind) *fail_kind = 3;
        return false;
    }
#ifdef NTM_STAMPS
    if (!collide) {                                        // which path the set takes, by spare columns
        if (sq) {
            if (xb >= 0) NTM_CNT(CN_SQ_COLL);
            else if (kdim == 0) NTM_CNT(CN_SQ_K0);
            else if (kdim == 1) NTM_CNT(CN_SQ_K1);
            else NTM_CNT(CN_SQ_K2);
        } else if (kdim <= 0) NTM_CNT(CN_BORD_K0);
        else if (kdim == 1) NTM_CNT(CN_BORD_K1);
        else if (kdim == 2) NTM_CNT(CN_BORD_K2);
        else if (kdim == 3) NTM_CNT(CN_BORD_K3);
        else NTM_CNT(CN_BORD_K4P);
        if (!sq) {
            if (dg_orph < 0) NTM_CNT(CN_BX_NOCLASS);
            else if (dg_neg) NTM_CNT(CN_BX_NEG);
            else if (dg_orph == 1) NTM_CNT(CN_BX_O1);
            else if (dg_orph == 2) NTM_CNT(CN_BX_O2);
            else if (dg_orph >= 3) NTM_CNT(CN_BX_O3P);
        }
    }
#endif
    // --- g_F (lane a = compact index) ---
    double gl = 0.0;
    if (!sq && l < nF) {
        const int ja = w.fidx()[l];
        const double* ca = w.Gt() + w.gidx(2 * ja, ja) - 2 * ja;   // ca[r] = gt(r, ja), r >= 2 ja
        const double g2 = qdot_rows<NTM_CH>(ca, w.xp(), N, ja, om);   // terms i < ja masked
        gl = w.D()[ja] * (2 * g2);
    }
    // Bordered KKT system (fused path): rows 0..nF-1 free variables, nF..nt-1 general
    // rows, nt the right-hand side; kept packed row-major (row r at r(r+1)/2) in the
    // contiguous J/R block.  Falls back to the two-stage Schur solve below when the
    // bordered rows do not fit the group's lanes or the block.
    const int nt = nF + nS;
    // nt <= 2N (nS <= nF); a compile-time horizon whose worst case fits compiles the fused path only
    // Lanes own RPL bordered rows each (row l + r P), enough for the nt + 1 <= 2N + 1 rows
    constexpr int NNc = W::kNN, LDc = NNc | 1;
    constexpr int RPL = NNc > 0 ? (2 * NNc + 1 + P - 1) / P : (2 * NTM_MAX_N + 1 + P - 1) / P;
    constexpr bool kAlwaysFused =
        NNc > 0 && (2 * NNc) * (2 * NNc + 1) / 2 + 2 * NNc <= NNc * LDc + (NNc + 1) * LDc;
    const bool fused = kAlwaysFused || ((nt + 1 <= RPL * P) && (nt * (nt + 1) / 2 + nt <= N * LDJ + (N + 1) * LD));
    double* const Lp = w.J();
    if (!sq && fused && l < nF) Lp[w.brow(nt) + w.bcol(l, nt)] = -gl;
    // --- compact G~_FF: one (a, c) entry per lane (packed rows, or lower col-major in R) ---
    const int npair = sq ? 0 : nF * (nF + 1) / 2;
    for (int idx = l; idx < npair; idx += P) {
        int a = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
        if ((a + 1) * (a + 2) / 2 <= idx) ++a;
        if (a * (a + 1) / 2 > idx) --a;
        const int c = idx - a * (a + 1) / 2;
        const int ja = w.fidx()[a], jc = w.fidx()[c];            // ja >= jc
        const double* ca = w.Gt() + w.gidx(2 * ja, ja) - 2 * ja;
        const double* cc = w.Gt() + w.gidx(2 * jc, jc) - 2 * jc;
        const double sg = qdot_rows<NTM_CH>(ca, cc, N, ja, om);   // terms i < ja masked
        double g2v = 2 * sg;
        if constexpr (ru_on<W>()) g2v = (a == c) ? g2v + 2 * pb.Ru : g2v;      // + 2 Ru I
        const double gv = g2v * w.D()[ja] * w.D()[jc];
        if (fused) Lp[w.brow(a) + w.bcol(c, nt)] = gv;            // row-major: idx == a(a+1)/2 + c
        else w.R()[a + c * LD] = gv;
    }
    NTM_WSYNC();
    // GI normal of general row s at variable j: n = -(Lin_j D_j)/rn, Lin = sg Gamma_r
    auto gen_n = [&](int s2, int j) -> double {
        const int r = w.srw()[s2];
        if (kRate && r >= 2 * N) {                        // rate row i = r - 2N
            const int i = r - 2 * N;
            const double sg = w.ssg()[s2];
            const double lv = (j == i) ? sg : (j == i - 1 ? -sg : 0.0);
            return -((lv * w.D()[j]) * w.idun()[i]);
        }
        return (j <= (r >> 1)) ? -(((w.ssg()[s2] * w.gt(r, j)) * w.D()[j]) * w.irn()[r]) : 0.0;
    };
    // h_s = n_s' V = bc_s - n_s,B' V_B with n_s,B' V_B = -sg irn_r (Gamma_r U_B)
    auto hs_of = [&](int s2) -> double {
        double hs = 0.0;
        if (s2 < nS) {
            const int r = w.srw()[s2];
            const double sg = w.ssg()[s2];
            if (kRate && r >= 2 * N) {                    // rate row i: b = du, fixed part sg (U_i - U_{i-1})
                const int i = r - 2 * N;
                const double ir = w.idun()[i];
                const double ui = w.fx()[i] ? w.Uf()[i] : 0.0;
                const double um = w.fx()[i - 1] ? w.Uf()[i - 1] : 0.0;
                hs = -(rows.du * ir) + (sg * (ui - um)) * ir;
            } else {
                const int c = r & 1;
                const double ir = w.irn()[r];
                const double bval = (sg > 0.0) ? (rows.xmax(c) - w.e()[r]) : (-rows.xmin(c) + w.e()[r]);
                hs = -(bval * ir) + (sg * w.Phi()[r]) * ir;
            }
        }
        return hs;
    };
    NTM_ACC(ST_P_GRAM, tp);
    bool ok = !collide && !nofree;
    int fk = ok ? 0 : 3, fpos_out = 0;
    double vfin = 0.0;
    double sq_id = 0.0;                                   // echelon path: 1 / E_p[t][t] on lane t
    bool y_ready = allfixed;                              // k = 1 / all fixed: y = Gamma U already in w.xp()
    if (sq) {
        // Sorted E over the pivot columns (row t = general row perm[t] ends in pivot
        // column pc(t) = t + (t >= nc); lower triangular, n x n row-major at Lp[t LD + u]),
        // the non-pivot column e_c (k = 1) and h
        const int n = nS - (xb >= 0 ? 1 : 0) - (xb2 >= 0 ? 1 : 0);
        auto pc = [&](int u) {                                // pivot column of sorted row u
            int c = u + ((nc >= 0 && u >= nc) ? 1 : 0);
            if (kCollision && nc2 >= 0 && c >= nc2) ++c;
            if (kColl3 && nc3 >= 0 && c >= nc3) ++c;
            return c;
        };
        double* const Ep = w.Ep();
        // long horizons: lane t builds sorted row t (n <= N <= 64 rows).  The row's
        // constants (its general row, sign, norm) are loaded once, and each batch of
        // CH columns costs one LDS round trip: the column index and D_j are the same
        // address on every lane (broadcast reads), only Gamma_rj differs.  The entry-
        // per-lane loop below issues ~5 dependent loads per entry, n^2 / 64 times per
        // lane (n ~ 43 at N = 50).  Entries as gen_n computes them, bit for bit.
        constexpr bool kRowE = W::kNN > 32 || W::kNN == 0;
        // (P = 64) lane u first loads pivot column u's variable and D_j, and
        // each row's loop takes them by readlane: one LDS round trip per batch (Gamma_rj)
        // instead of two (the column index, then Gamma_rj and D_j at it)
        constexpr bool kLaneIdx = P == 64;
        int jfl = 0;
        double dfl = 0.0;
        if constexpr (kRowE && kLaneIdx) {
            if (l < n) {
                jfl = w.fidx()[pc(l)];
                dfl = w.D()[jfl];
            }
        }
        auto col_of = [&](int u) -> int {                     // pivot column u's variable (u uniform)
            if constexpr (kLaneIdx) return __builtin_amdgcn_readlane(jfl, u);
            else return w.fidx()[pc(u)];
        };
        auto d_of = [&](int u, int j) -> double {             // D at it
            if constexpr (kLaneIdx) return gbcast<P>(dfl, u);
            else return w.D()[j];
        };
        if constexpr (kRowE) {
            if (l < n) {
                const int s2 = perm[l];
                const int r = w.srw()[s2];
                const double sg = w.ssg()[s2];
                double* const erow = Ep + w.eidx(l, 0);
                constexpr int CH = NTM_CH;
                if (r >= 2 * N) {                                  // rate row of input i
                    const int i = r - 2 * N;
                    const double ir = w.idun()[i];
                    for (int u = 0; u <= l; ++u) {
                        const int uu = kLaneIdx ? __builtin_amdgcn_readfirstlane(u) : u;
                        const int j = col_of(uu);
                        const double lv = (j == i) ? sg : (j == i - 1 ? -sg : 0.0);
                        erow[u] = -((lv * d_of(uu, j)) * ir);
                    }
                } else {
                    const double ir = w.irn()[r];
                    const int jm = r >> 1;
                    const double* gr = w.Gt() + r;                 // gt(r, j) = gr[gidx(0, j)]
                    for (int u0 = 0; u0 <= l; u0 += CH) {
                        int jj[CH];
                        double g[CH], d[CH];
                        const int ub = kLaneIdx ? __builtin_amdgcn_readfirstlane(u0) : u0;
#pragma unroll
                        for (int c = 0; c < CH; ++c) {
                            if constexpr (kLaneIdx) jj[c] = col_of((ub + c) & 63);     // lanes >= n hold 0
                            else jj[c] = (u0 + c <= l) ? w.fidx()[pc(u0 + c)] : 0;
                        }
#pragma unroll
                        for (int c = 0; c < CH; ++c) {
                            const bool in = u0 + c <= l && jj[c] <= jm;
                            g[c] = in ? gr[w.gidx(0, jj[c])] : 0.0;
                            if constexpr (kLaneIdx) d[c] = (u0 + c <= l) ? d_of((ub + c) & 63, 0) : 0.0;
                            else d[c] = (u0 + c <= l) ? w.D()[jj[c]] : 0.0;
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int c = 0; c < CH; ++c)
                            if (u0 + c <= l) erow[u0 + c] = (jj[c] <= jm) ? -(((sg * g[c]) * d[c]) * ir) : 0.0;
                    }
                }
                if constexpr (!W::kFar)
                    for (int u = l + 1; u < n; ++u) erow[u] = 0.0;
            }
        } else {
        for (int idx = l; idx < n * n; idx += P) {
            const int t = idx / n, u = idx - t * n;
            if constexpr (W::kFar) {                               // packed: the lower triangle only
                if (u <= t) Ep[w.eidx(t, u)] = gen_n(perm[t], w.fidx()[pc(u)]);
            } else {
                Ep[w.eidx(t, u)] = (u <= t) ? gen_n(perm[t], w.fidx()[pc(u)]) : 0.0;
            }
        }
        }
        double acc = 0.0, acz = 0.0, acz2 = 0.0, acz3 = 0.0;
        if (l < n && !dir) {
            acc = hs_of(perm[l]);
            if (nc >= 0 && nc < pc(l)) acz = -gen_n(perm[l], w.fidx()[nc]);
            if (kCollision && nc2 >= 0 && nc2 < pc(l)) acz2 = -gen_n(perm[l], w.fidx()[nc2]);
            if (kColl3 && nc3 >= 0 && nc3 < pc(l)) acz3 = -gen_n(perm[l], w.fidx()[nc3]);
        }
        const double hxb = (kCollision && xb >= 0 && !dir) ? hs_of(xb) : 0.0;   // before w.Phi() is reused
        const double hxb2 = (kColl2 && xb2 >= 0 && !dir) ? hs_of(xb2) : 0.0;
        NTM_WSYNC();
        if (l < n) sq_id = 1.0 / Ep[w.eidx(l, l)];
        NTM_ACC(ST_S_E, tp);
        if (!dir) {
        // E_p V_p = h and (k = 1) E_p Z_p = -e_c: lane t owns row t; step t broadcasts
        // x_t (z_t) and updates the rows below
        double x = 0.0, zz = 0.0, zz2 = 0.0, zz3 = 0.0;
        if constexpr (esub_lanes_ok<P, NTM_CH, W>()) {
            // the slim far N = 20 kernels: unrolled in batches of five under narrowed EXEC (fsub_lanes)
            const unsigned row = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)(Ep + w.eidx(l, 0));
            const int nu = __builtin_amdgcn_readfirstlane(n);
            if (nc >= 0) fsub_lanes<true>(nu, acc, x, acz, zz, sq_id, row);
            else fsub_lanes<false>(nu, acc, x, acz, zz, sq_id, row);
        } else {
        // E[l][t] loaded kAhead steps ahead (a register queue)
        constexpr int kAhead = 1;
        double eq[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) eq[a] = (a < n && l > a && l < n) ? Ep[w.eidx(l, a)] : 0.0;
        // NTM_SUB_PRESCALE (long horizons): the accumulators carry acc / E[l][l] and the
        // update uses E[l][t] / E[l][l], formed off the chain, so step t's broadcast waits
        // on one operation less (fma -> readlane -> fma)
        constexpr bool kPre = NTM_SUB_PRESCALE && W::kNN > 32;
        if constexpr (kPre) { acc *= sq_id; acz *= sq_id; acz2 *= sq_id; acz3 *= sq_id; }
        for (int t = 0; t < n; ++t) {
            const double et = kPre ? eq[0] * sq_id : eq[0];
#pragma unroll
            for (int a = 0; a + 1 < kAhead; ++a) eq[a] = eq[a + 1];
            {
                const int ta = t + kAhead;
                eq[kAhead - 1] = (ta < n && l > ta && l < n) ? Ep[w.eidx(l, ta)] : 0.0;
            }
            const double xt = gbcast<P>(kPre ? acc : acc * sq_id, t);
            if (l == t) x = xt;
            acc -= et * xt;
            if (nc >= 0) {
                const double zt = gbcast<P>(kPre ? acz : acz * sq_id, t);
                if (l == t) zz = zt;
                acz -= et * zt;
            }
            if (kCollision && nc2 >= 0) {
                const double zt2 = gbcast<P>(kPre ? acz2 : acz2 * sq_id, t);
                if (l == t) zz2 = zt2;
                acz2 -= et * zt2;
            }
            if (kColl3 && nc3 >= 0) {
                const double zt3 = gbcast<P>(kPre ? acz3 : acz3 * sq_id, t);
                if (l == t) zz3 = zt3;
                acz3 -= et * zt3;
            }
        }
        }
        ok = !gany<P>(l < n && !(isfinite(x) && isfinite(zz) && isfinite(zz2) && isfinite(zz3)));
        // V_0 (pivots from E_p V_p = h, fixed values, 0 on the non-pivot columns) and Z
        const bool hole = fpos == nc || (kCollision && nc2 >= 0 && fpos == nc2) || (kColl3 && nc3 >= 0 && fpos == nc3);
        const int rk = hole ? 0
                            : fpos - ((nc >= 0 && fpos > nc) ? 1 : 0) - ((kCollision && nc2 >= 0 && fpos > nc2) ? 1 : 0) -
                                  ((kColl3 && nc3 >= 0 && fpos > nc3) ? 1 : 0);
        const double xs = __shfl(x, (l < N && !fixed) ? rk : 0, P);
        const double zs = __shfl(zz, (l < N && !fixed) ? rk : 0, P);
        const double v0 = fixed ? vb : (hole ? 0.0 : xs);
        vfin = v0;
        // k = 1 with one collision: V = V_0 + w1 Z1 + w2 Z2 (Zi = e_{hole i} + Zi_p); the row
        // left out fixes a1 w1 + a2 w2 = h_B - n_B' V_0 (ai = n_B' Zi), which leaves the line
        // V_p + w Z_d (eliminating the w with the larger |ai|) for the cost to minimise below
        double vline = v0, zline = 0.0;
        bool line = false;
        // k = 2: V = V_0 + w1 Z1 + w2 Z2 (Zi = e_{hole i} + Zi_p); with yi = Gamma D Zi
        // and q = y_0 + e - r the cost is minimised at H w = -g, H_ij = yi' Om yj (+ Ru
        // dUi' dUj), g_i = yi' Om q (+ Ru dUi' U_0): three Gamma passes, five reductions
        auto plane_min = [&](const double v0, const double z1, const double z2) {
            double* const y2s = w.Vb();                       // 2N scratch (Vb, Uf: dead after hs_of)
            if (l < N) {
                w.U()[l] = w.D()[l] * v0;
                w.d()[l] = w.D()[l] * z1;
                w.dr()[l] = w.D()[l] * z2;
            }
            NTM_WSYNC();
            for (int r = l; r < 2 * N; r += P) {
                double ya, yb;
                gamma_row_dot2<NTM_CH, P>(w, r, w.U(), w.d(), ya, yb);
                w.xp()[r] = ya;
                w.Phi()[r] = yb;
                y2s[r] = gamma_row_dot<NTM_CH, P>(w, r, w.dr());
            }
            NTM_WSYNC();
            double g1 = 0.0, g2 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0;
            if (l < N) {
                constexpr bool AL = pair_ld_ok<P, W>();
                const dpair yv = ld_pair<AL>(w.xp() + 2 * l), ev = ld_pair<AL>(w.e() + 2 * l);
                const dpair av = ld_pair<AL>(w.Phi() + 2 * l), cv = ld_pair<AL>(y2s + 2 * l);
                const double qa = yv.x + ev.x - pb.r[0];
                const double qb = yv.y + ev.y - pb.r[1];
                const double aa = av.x, ab = av.y;
                const double ca = cv.x, cb = cv.y;
                const double oa = om.o0(aa, ab), ob = om.o1(aa, ab);      // Om y1
                const double oc = om.o0(ca, cb), od = om.o1(ca, cb);      // Om y2
                g1 = oa * qa + ob * qb;
                g2 = oc * qa + od * qb;
                h11 = oa * aa + ob * ab;
                h12 = oa * ca + ob * cb;
                h22 = oc * ca + od * cb;
                if constexpr (ru_on<W>()) {
                    const double u0 = w.U()[l], d1 = w.d()[l], d2 = w.dr()[l];
                    g1 += pb.Ru * (d1 * u0);
                    g2 += pb.Ru * (d2 * u0);
                    h11 += pb.Ru * (d1 * d1);
                    h12 += pb.Ru * (d1 * d2);
                    h22 += pb.Ru * (d2 * d2);
                }
            }
            g1 = gsum<P>(g1);
            g2 = gsum<P>(g2);
            h11 = gsum<P>(h11);
            h12 = gsum<P>(h12);
            h22 = gsum<P>(h22);
            const double det = h11 * h22 - h12 * h12;
            ok = det > 0.0 && h11 > 0.0 && det < kInf && isfinite(g1) && isfinite(g2);
            const double w1 = ok ? -((h22 * g1 - h12 * g2) / det) : 0.0;
            const double w2 = ok ? -((h11 * g2 - h12 * g1) / det) : 0.0;
            vfin = v0 + w1 * z1 + w2 * z2;
            for (int r = l; r < 2 * N; r += P) w.xp()[r] += w1 * w.Phi()[r] + w2 * y2s[r];   // y
            y_ready = true;
        };
        if (kColl3 && ok && xb2 >= 0 && nc3 >= 0) {
            // k = 1 with two collisions: V = V_0 + w1 Z1 + w2 Z2 + w3 Z3 and the two rows left
            // out fix A w = r (A 2 x 3, A_ij = n_Bi' Zj, r_i = h_Bi - n_Bi' V_0): a particular
            // solution from the best-conditioned 2 x 2 minor plus t times the null vector
            // (the rows' cross product) leaves the line V_p + t Z_n for the cost to minimise
            const double zs2 = __shfl(zz2, (l < N && !fixed) ? rk : 0, P);
            const double zs3 = __shfl(zz3, (l < N && !fixed) ? rk : 0, P);
            const double z1 = fixed ? 0.0 : ((fpos == nc) ? 1.0 : (hole ? 0.0 : zs));
            const double z2 = fixed ? 0.0 : ((fpos == nc2) ? 1.0 : (hole ? 0.0 : zs2));
            const double z3 = fixed ? 0.0 : ((fpos == nc3) ? 1.0 : (hole ? 0.0 : zs3));
            const double nb1 = (l < N && !fixed) ? gen_n(xb, l) : 0.0;
            const double nb2 = (l < N && !fixed) ? gen_n(xb2, l) : 0.0;
            const double b10 = gsum<P>(nb1 * v0), a11 = gsum<P>(nb1 * z1), a12 = gsum<P>(nb1 * z2), a13 = gsum<P>(nb1 * z3);
            const double b20 = gsum<P>(nb2 * v0), a21 = gsum<P>(nb2 * z1), a22 = gsum<P>(nb2 * z2), a23 = gsum<P>(nb2 * z3);
            const double r1 = hxb - b10, r2 = hxb2 - b20;
            const double d12 = a11 * a22 - a12 * a21, d13 = a11 * a23 - a13 * a21, d23 = a12 * a23 - a13 * a22;
            const double scl = fmax(fmax(fmax(fabs(a11), fabs(a12)), fabs(a13)), fmax(fmax(fabs(a21), fabs(a22)), fabs(a23)));
            const int im = (fabs(d12) >= fabs(d13) && fabs(d12) >= fabs(d23)) ? 0 : (fabs(d13) >= fabs(d23) ? 1 : 2);
            const double dm = im == 0 ? d12 : (im == 1 ? d13 : d23);
            ok = isfinite(dm) && fabs(dm) > 1e-14 * scl * scl && isfinite(b10) && isfinite(b20);
            double w1 = 0.0, w2 = 0.0, w3 = 0.0;
            if (ok) {
                if (im == 0) { w1 = (a22 * r1 - a12 * r2) / dm; w2 = (a11 * r2 - a21 * r1) / dm; }
                else if (im == 1) { w1 = (a23 * r1 - a13 * r2) / dm; w3 = (a11 * r2 - a21 * r1) / dm; }
                else { w2 = (a23 * r1 - a13 * r2) / dm; w3 = (a12 * r2 - a22 * r1) / dm; }
            }
            vline = ok ? v0 + w1 * z1 + w2 * z2 + w3 * z3 : v0;
            zline = ok ? (d23 / dm) * z1 - (d13 / dm) * z2 + (d12 / dm) * z3 : 0.0;
            line = ok;
        } else if (kColl3 && ok && xb >= 0 && nc3 >= 0) {
            // k = 2 with one collision: V = V_0 + w1 Z1 + w2 Z2 + w3 Z3; the row left out
            // fixes a1 w1 + a2 w2 + a3 w3 = h_B - n_B' V_0 (ai = n_B' Zi): eliminating the w
            // with the largest |ai| leaves the plane V_p + wa Za + wb Zb for the cost below
            const double zs2 = __shfl(zz2, (l < N && !fixed) ? rk : 0, P);
            const double zs3 = __shfl(zz3, (l < N && !fixed) ? rk : 0, P);
            const double z1 = fixed ? 0.0 : ((fpos == nc) ? 1.0 : (hole ? 0.0 : zs));
            const double z2 = fixed ? 0.0 : ((fpos == nc2) ? 1.0 : (hole ? 0.0 : zs2));
            const double z3 = fixed ? 0.0 : ((fpos == nc3) ? 1.0 : (hole ? 0.0 : zs3));
            const double nb = (l < N && !fixed) ? gen_n(xb, l) : 0.0;
            const double b0 = gsum<P>(nb * v0), a1 = gsum<P>(nb * z1), a2 = gsum<P>(nb * z2), a3 = gsum<P>(nb * z3);
            const int ip = (fabs(a3) > fabs(a2)) ? ((fabs(a3) > fabs(a1)) ? 3 : 1) : ((fabs(a2) >= fabs(a1)) ? 2 : 1);
            const double ap = ip == 1 ? a1 : (ip == 2 ? a2 : a3);
            const double aa = ip == 1 ? a2 : a1, ab = ip == 3 ? a2 : a3;
            const double zp = ip == 1 ? z1 : (ip == 2 ? z2 : z3);
            const double za = ip == 1 ? z2 : z1, zb = ip == 3 ? z2 : z3;
            ok = ap != 0.0 && isfinite(ap) && isfinite(aa) && isfinite(ab) && isfinite(b0);
            if (ok) plane_min(v0 + ((hxb - b0) / ap) * zp, za - (aa / ap) * zp, zb - (ab / ap) * zp);
        } else if (kColl2 && ok && xb2 >= 0) {
            // two collisions: V = V_0 + w1 Z1 + w2 Z2 with the rows left out fixing
            // [n_B1'Z1 n_B1'Z2; n_B2'Z1 n_B2'Z2] w = [h_B1 - n_B1'V_0; h_B2 - n_B2'V_0]
            const double zs2 = __shfl(zz2, (l < N && !fixed) ? rk : 0, P);
            const double z1 = fixed ? 0.0 : ((fpos == nc) ? 1.0 : (hole ? 0.0 : zs));
            const double z2 = fixed ? 0.0 : ((fpos == nc2) ? 1.0 : (hole ? 0.0 : zs2));
            const double nb1 = (l < N && !fixed) ? gen_n(xb, l) : 0.0;
            const double nb2 = (l < N && !fixed) ? gen_n(xb2, l) : 0.0;
            const double b10 = gsum<P>(nb1 * v0), a11 = gsum<P>(nb1 * z1), a12 = gsum<P>(nb1 * z2);
            const double b20 = gsum<P>(nb2 * v0), a21 = gsum<P>(nb2 * z1), a22 = gsum<P>(nb2 * z2);
            const double det = a11 * a22 - a12 * a21;
            const double scl = fmax(fmax(fabs(a11), fabs(a12)), fmax(fabs(a21), fabs(a22)));
            ok = isfinite(det) && fabs(det) > 1e-14 * scl * scl && isfinite(b10) && isfinite(b20);
            const double r1 = hxb - b10, r2 = hxb2 - b20;
            const double w1 = ok ? (a22 * r1 - a12 * r2) / det : 0.0;
            const double w2 = ok ? (a11 * r2 - a21 * r1) / det : 0.0;
            vfin = v0 + w1 * z1 + w2 * z2;
        } else if (kCollision && ok && xb >= 0 && nc2 >= 0) {
            const double zs2 = __shfl(zz2, (l < N && !fixed) ? rk : 0, P);
            const double z1 = fixed ? 0.0 : ((fpos == nc) ? 1.0 : (hole ? 0.0 : zs));
            const double z2 = fixed ? 0.0 : ((fpos == nc2) ? 1.0 : (hole ? 0.0 : zs2));
            const double nb = (l < N && !fixed) ? gen_n(xb, l) : 0.0;
            const double b0 = gsum<P>(nb * v0), a1 = gsum<P>(nb * z1), a2 = gsum<P>(nb * z2);
            const bool use2 = fabs(a2) >= fabs(a1);
            const double ap = use2 ? a2 : a1, ao = use2 ? a1 : a2;
            ok = ap != 0.0 && isfinite(ap) && isfinite(ao) && isfinite(b0);
            const double zp = use2 ? z2 : z1, zo = use2 ? z1 : z2;
            vline = ok ? v0 + ((hxb - b0) / ap) * zp : v0;
            zline = ok ? zo - (ao / ap) * zp : 0.0;
            line = ok;
        } else if (kCollision && ok && xb >= 0) {
            // the row left out fixes the step along Z: n_B' (V_0 + w Z) = h_B
            const double zv = fixed ? 0.0 : ((fpos == nc) ? 1.0 : zs);
            const double nb = (l < N && !fixed) ? gen_n(xb, l) : 0.0;
            const double b0 = gsum<P>(nb * v0), b1 = gsum<P>(nb * zv);
            ok = b1 != 0.0 && isfinite(b1) && isfinite(b0);
            const double wv = ok ? (hxb - b0) / b1 : 0.0;
            vfin = v0 + wv * zv;
        } else if (kPlane && ok && nc2 >= 0) {
            const double zs2 = __shfl(zz2, (l < N && !fixed) ? rk : 0, P);
            const double z1 = fixed ? 0.0 : ((fpos == nc) ? 1.0 : (hole ? 0.0 : zs));
            const double z2 = fixed ? 0.0 : ((fpos == nc2) ? 1.0 : (hole ? 0.0 : zs2));
            plane_min(v0, z1, z2);
        } else if (ok && nc >= 0) {
            zline = fixed ? 0.0 : ((fpos == nc) ? 1.0 : zs);
            line = true;
        }
        if (line) {
            // k = 1: the minimum along V_0 + w Z, Z = e_c + Z_p:
            //   w = -(2 yz' Om (y0 + e - r)) / (2 yz' Om yz), y0 = Gamma D V_0, yz = Gamma D Z
            const double v0 = vline, zv = zline;
            if (l < N) {
                w.U()[l] = w.D()[l] * v0;
                w.d()[l] = w.D()[l] * zv;
            }
            NTM_WSYNC();
            for (int r = l; r < 2 * N; r += P) {
                double ya, yb;
                gamma_row_dot2<NTM_CH, P>(w, r, w.U(), w.d(), ya, yb);
                w.xp()[r] = ya;
                w.Phi()[r] = yb;                             // scratch (hs_of is done with it)
            }
            NTM_WSYNC();
            double num = 0.0, den = 0.0;
            if (l < N) {
                constexpr bool AL = pair_ld_ok<P, W>();
                const dpair yv = ld_pair<AL>(w.xp() + 2 * l), ev = ld_pair<AL>(w.e() + 2 * l);
                const dpair zv2 = ld_pair<AL>(w.Phi() + 2 * l);
                const double y0a = yv.x + ev.x - pb.r[0];
                const double y0b = yv.y + ev.y - pb.r[1];
                const double za = zv2.x, zb = zv2.y;
                const double oa = om.o0(za, zb), ob = om.o1(za, zb);
                num = oa * y0a + ob * y0b;
                den = oa * za + ob * zb;
                if constexpr (ru_on<W>()) {               // Ru (dU' U_0, dU' dU): w.U() = D V_0, w.d() = D Z
                    const double ua = w.U()[l], da = w.d()[l];
                    num += pb.Ru * (da * ua);
                    den += pb.Ru * (da * da);
                }
            }
            num = gsum<P>(num);
            den = gsum<P>(den);
            ok = den > 0.0 && den < kInf && isfinite(num);
            const double wv = ok ? -(num / den) : 0.0;
            vfin = v0 + wv * zv;
            for (int r = l; r < 2 * N; r += P) w.xp()[r] += wv * w.Phi()[r];   // y = y0 + w yz
            y_ready = true;
        }
        }   // !dir
        if (!ok) fk = 3;
        NTM_ACC(ST_S_Y, tp);
    } else if (fused) {
        // E rows over the free variables (one entry per lane) and h; the trailing
        // block of A is zero and is never stored (the elimination starts it at 0)
        for (int idx = l; idx < nF * nS; idx += P) {
            const int s2 = idx / nF, a = idx - s2 * nF;
            Lp[w.brow(nF + s2) + w.bcol(a, nt)] = gen_n(s2, w.fidx()[a]);
        }
        if (l < nS) Lp[w.brow(nt) + w.bcol(nF + l, nt)] = hs_of(l);
        NTM_WSYNC();
        NTM_ACC(ST_S_E, tp);
        // Left-looking elimination of A = [[G~_FF, E'], [E, 0]] = L_A diag(I, -I) L_A'
        // over its nt columns: L_A = [[L, 0], [Y', L_K]] with L L' = G~_FF,
        // Y = L^{-1} E', L_K L_K' = K = Y'Y (the Schur complement), in one pass
        // whose right-hand-side row carries the forward substitution
        // z = L_A^{-1} [-g_F; h].  Lane r owns row r.
        // Lane l owns rows l + r P (r < RPL); a group-uniform row index k lives on
        // lane k % P in slot k / P.
        auto slot_of = [&](const double* v, int k) -> double {   // v[k / P] (k uniform)
            double o = v[0];
#pragma unroll
            for (int r = 1; r < RPL; ++r) o = (k / P == r) ? v[r] : o;
            return o;
        };
        double* myrow[RPL];
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
            const int lr = l + r * P;
            myrow[r] = Lp + w.brow(lr);
        }
        if (ok) {
            // blocks of KB columns: one pass of loads over the finished columns j < k
            // serves all KB pivot rows, then the block's own triangle is finished in
            // registers (L[k+b, k+c] broadcast from the lane of row k+b).  Each column
            // still accumulates its terms in column order, as the unblocked elimination.
            constexpr int KB = 4;
            for (int k = 0; k < nt; k += KB) {
                const int kb = (nt - k < KB) ? nt - k : KB;
                double sacc[RPL][KB];
                bool live[RPL];
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
                    live[r] = lr >= k && lr <= nt;
#pragma unroll
                    for (int b2 = 0; b2 < KB; ++b2) {
                        const int col = k + b2;
                        sacc[r][b2] = (b2 < kb && live[r] && lr >= col) ? ((col >= nF && lr < nt) ? 0.0 : myrow[r][w.bcol(col, nt)])
                                                                        : 0.0;
                    }
                }
                const int kf = k < nF ? k : nF;
                // unconditional loads (no branch per load): j + 1 <= k stays inside each
                // live row (>= k) and pivot row k+b2; pivot rows past the block clamp to row nt
                const double* prb[KB];
#pragma unroll
                for (int b2 = 0; b2 < KB; ++b2) {
                    const int rr = (k + b2 < nt) ? k + b2 : nt;
                    prb[b2] = Lp + w.brow(rr);
                }
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    if (!live[r]) continue;
                    for (int j = 0; j < k; j += 2) {
                        const bool in1 = j + 1 < k;
                        const int cj0 = w.bcol(j, nt), cj1 = w.bcol(j + 1, nt);
                        const double a0 = myrow[r][cj0], a1 = myrow[r][cj1];
                        double p0[KB], p1[KB];
#pragma unroll
                        for (int b2 = 0; b2 < KB; ++b2) {
                            p0[b2] = prb[b2][cj0];
                            p1[b2] = prb[b2][cj1];
                        }
                        const double s0 = (j < kf) ? -1.0 : 1.0, s1 = (j + 1 < kf) ? -1.0 : 1.0;
#pragma unroll
                        for (int b2 = 0; b2 < KB; ++b2) {
                            sacc[r][b2] += (s0 * a0) * p0[b2];
                            sacc[r][b2] += in1 ? (s1 * a1) * p1[b2] : 0.0;
                        }
                    }
                }
                double Lc[RPL][KB];
#pragma unroll
                for (int b2 = 0; b2 < KB; ++b2) {
#pragma unroll
                    for (int r = 0; r < RPL; ++r) Lc[r][b2] = 0.0;
                    if (b2 < kb) {
                        const int col = k + b2, cl = col % P;
#pragma unroll
                        for (int c = 0; c < b2; ++c) {           // block columns k..col-1, in order
                            double lcc[RPL];
#pragma unroll
                            for (int r = 0; r < RPL; ++r) lcc[r] = Lc[r][c];
                            const double lkc = gbcast<P>(slot_of(lcc, col), cl);   // L[col, k+c]
                            const double sc = (k + c < nF) ? -1.0 : 1.0;
#pragma unroll
                            for (int r = 0; r < RPL; ++r) sacc[r][b2] += (sc * Lc[r][c]) * lkc;
                        }
                        double skr[RPL];
#pragma unroll
                        for (int r = 0; r < RPL; ++r) skr[r] = (col < nF) ? sacc[r][b2] : -sacc[r][b2];
                        const double dk = gbcast<P>(slot_of(skr, col), cl);
                        if (!(dk > 0.0) || !(dk < kInf)) { ok = false; fk = 3; }
                        else {
                            const double il = rsqrt_nr(dk);
#pragma unroll
                            for (int r = 0; r < RPL; ++r) {
                                const int lr = l + r * P;
                                Lc[r][b2] = (lr == col) ? dk * il : skr[r] * il;
                                if (lr == col) w.ldi()[col] = il;   // ldi/kdi: 2N contiguous
                            }
                        }
                    }
                }
                if (!ok) break;
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
#pragma unroll
                    for (int b2 = 0; b2 < KB; ++b2)
                        if (b2 < kb && lr >= k + b2 && lr <= nt) myrow[r][w.bcol(k + b2, nt)] = Lc[r][b2];
                }
                NTM_WSYNC();
            }
        }
        NTM_ACC(ST_S_CHOL, tp);
        if (ok) {
            // L_A' x = diag(I, -I) z: x = [V_F; -mu], one backward sweep.  The
            // right-hand-side row holds sigma_k z_k (sigma = +1 free, -1 general
            // columns), which is exactly diag(I, -I) z
            double acc[RPL], x[RPL];
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
                const int lr = l + r * P;
                acc[r] = (lr < nt) ? Lp[w.brow(nt) + w.bcol(lr, nt)] : 0.0;
                x[r] = 0.0;
            }
            // the loads of column k-1 are issued before the broadcast of x_k (one-deep pipeline)
            double lkn[RPL], dkn = 0.0;
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
                const int lr = l + r * P;
                lkn[r] = (nt > 0 && lr < nt - 1) ? Lp[w.brow(nt - 1) + w.bcol(lr, nt)] : 0.0;
            }
            if (nt > 0) dkn = w.ldi()[nt - 1];
            for (int k = nt - 1; k >= 0; --k) {
                double lk[RPL];
#pragma unroll
                for (int r = 0; r < RPL; ++r) lk[r] = lkn[r];
                const double dk = dkn;
                if (k > 0) {
#pragma unroll
                    for (int r = 0; r < RPL; ++r) {
                        const int lr = l + r * P;
                        lkn[r] = (lr < k - 1) ? Lp[w.brow(k - 1) + w.bcol(lr, nt)] : 0.0;
                    }
                    dkn = w.ldi()[k - 1];
                }
                const double xk = gbcast<P>(slot_of(acc, k), k % P) * dk;
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
                    if (lr == k) x[r] = xk;
                    if (lr < k) acc[r] -= lk[r] * xk;
                }
            }
#pragma unroll
            for (int r = 0; r < RPL; ++r) {
                const int lr = l + r * P;
                if (lr >= nF && lr < nt) w.np()[lr - nF] = -x[r];
            }
            NTM_WSYNC();
            // V_F sits in rows < nF <= N <= P: slot 0
            const double vsc = __shfl(x[0], (l < N && !fixed) ? fpos : 0, P);
            vfin = fixed ? vb : vsc;
        }
        NTM_ACC(ST_S_SOLVE, tp);
    } else if constexpr (!kAlwaysFused) {
    ok = !collide && chol_inplace<P>(w.R(), nF, 1, LD, l, w.ldi());
    fk = ok ? 0 : 3;
    if (ok) {
        const double wl = fwd_lanes<P>(w.R(), w.ldi(), nF, 1, LD, gl, l);    // L^{-1} g_F
        double tl = -wl;
        NTM_ACC(ST_P_CHOL, tp);
        if (nS > 0) {
            // E' (compact rows) into Y = w.J() (row-major nF x nS), one entry per lane
            for (int idx = l; idx < nF * nS; idx += P) {
                const int a = idx / nS, s2 = idx - a * nS;
                w.J()[a * LDJ + s2] = gen_n(s2, w.fidx()[a]);
            }
            if (l < nF) w.d()[l] = wl;
            const double hs = hs_of(l);
            NTM_WSYNC();
            NTM_ACC(ST_S_E, tp);
            if (l < nS) {                          // Y = L^{-1} E': lane s solves column s
                for (int i = 0; i < nF; ++i) {
                    double y = w.J()[i * LDJ + l];
                    for (int k = 0; k < i; ++k) y -= w.R()[i + k * LD] * w.J()[k * LDJ + l];
                    w.J()[i * LDJ + l] = y * w.ldi()[i];
                }
            }
            NTM_WSYNC();
            NTM_ACC(ST_S_Y, tp);
            double* K = w.R() + LD;                // K(a, c), a >= c, at R[c + (a+1) LD]
            double rhs = 0.0;
            {
                const int npair = nS * (nS + 1) / 2;
                for (int idx = l; idx < npair; idx += P) {
                    int a = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
                    if ((a + 1) * (a + 2) / 2 <= idx) ++a;
                    if (a * (a + 1) / 2 > idx) --a;
                    const int c = idx - a * (a + 1) / 2;
                    double sK = 0.0;
                    for (int i = 0; i < nF; ++i) sK += w.J()[i * LDJ + a] * w.J()[i * LDJ + c];
                    K[a * LD + c] = sK;
                }
            }
            if (l < nS) {
                rhs = hs;
                for (int i = 0; i < nF; ++i) rhs += w.J()[i * LDJ + l] * w.d()[i];
            }
            NTM_WSYNC();
            NTM_ACC(ST_S_K, tp);
            ok = chol_inplace<P>(K, nS, LD, 1, l, w.kdi());
            NTM_ACC(ST_S_CHOL, tp);
            if (!ok) fk = 3;
            if (ok) {
                double t1 = fwd_lanes<P>(K, w.kdi(), nS, LD, 1, rhs, l);
                double mu = bwd_lanes<P>(K, w.kdi(), nS, LD, 1, t1, l);
                if (l < nS) w.np()[l] = mu;
                NTM_WSYNC();
                if (l < nF) {
                    double sY = 0.0;
                    for (int a = 0; a < nS; ++a) sY += w.J()[l * LDJ + a] * w.np()[a];
                    tl = sY - wl;
                }
                NTM_ACC(ST_S_SOLVE, tp);
            }
        }
        NTM_ACC(ST_P_SCHUR, tp);
        if (ok) {
            const double vF = bwd_lanes<P>(w.R(), w.ldi(), nF, 1, LD, tl, l);   // compact V_F
            const double vsc = __shfl(vF, (l < N && !fixed) ? fpos : 0, P);
            vfin = fixed ? vb : vsc;
        }
    }
    }
    NTM_ACC(ST_P_BWD, tp);
    // Generic kernels: one step of fixed-precision iterative refinement after the
    // bordered elimination.  Its range-space factor goes through L L' = G~_FF, which
    // loses digits when G~_FF is nearly singular although the KKT system is well
    // conditioned (input-rate rows holding the last inputs, N = 20 mode 3, which
    // runs here: ~1e-9 umax off the exact optimum).  Pass 0 of the certificate
    // loop computes the KKT residual [r1; r2] (r1 = G~V + F~ - E'mu on the free
    // variables, r2 = n_s'V - bc_s on the general rows), solves A [dV; -dmu] =
    // -[r1; r2] with the same factor (forward and backward sweeps), and pass 1
    // certifies the corrected point.  The specialised N = 20 / 50 kernels keep the
    // single pass (their register allocation decides their speed).
    constexpr bool kRefine = W::kNN == 0;
    bool refine = kRefine && ok && !sq && fused;
    double r2 = 0.0;
    for (int pass = 0; ok; ++pass) {
        // ---- KKT certificate ----
        const bool resid = refine && pass == 0;
        if (!dir) {
        if (l < N) { w.V()[l] = vfin; w.U()[l] = w.D()[l] * vfin; }
        NTM_WSYNC();
        // y = Gamma U once, for the primal check (state rows) and the gradient
        if (!y_ready) {
            for (int r = l; r < 2 * N; r += P) w.xp()[r] = gamma_row_dot<NTM_CH, P>(w, r, w.U());
            NTM_WSYNC();
        }
        }
        NTM_ACC(ST_K_Y, tp);
        Pick vf{};
        if (dir) {
        } else if (resid) {
            if (l < nS) {                                  // primal residual of general row l
                const int r = w.srw()[l];
                const double sg = w.ssg()[l];
                if (kRate && r >= 2 * N) {
                    const int i = r - 2 * N;
                    r2 = w.idun()[i] * (rows.du - sg * (w.U()[i] - w.U()[i - 1]));
                } else {
                    const int c = r & 1;
                    const double bval = (sg > 0.0) ? (rows.xmax(c) - w.e()[r]) : (-rows.xmin(c) + w.e()[r]);
                    r2 = w.irn()[r] * (bval - sg * w.xp()[r]);
                }
            }
        } else {
            double vmax = gmax<P>(l < N ? fabs(vfin) : 0.0);
            vf = rows.template check<P>(w, vfin, l, true, fmax(1.0, vmax), w.xp());
            ok = vf.p == 0;
        }
        NTM_ACC(ST_K_CHK, tp);
        // gradient G~V + F~ = D (2 Gamma' Om y) + F~, with Om y once per stage into
        // scratch (w.Phi() + 2N: Phi is dead until the next lift; the sparse pass
        // below uses its first nS entries, the refinement its first nt <= 2N): y
        // itself stays in w.xp(), where the rollout of a certified U reads it
        // (kSlim: Om = I, so Om y is y itself, read from w.xp())
        constexpr bool kOmyX = W::kSlim && qi_on<W>();     // Om y = y: read w.xp()
        double* const omy = kOmyX ? w.xp() : (W::kSlim ? w.Phi() : w.Phi() + 2 * N);
        double res = 0.0;
        if (dir) {                                         // n_p in place of the gradient
            if (l < N) res = -((rows.lin(w, dir_p, l) * w.D()[l]) / rows.rnorm(w, dir_p));
        } else {
        if (l < N && !kOmyX) {
            const double y0 = w.xp()[2 * l], y1 = w.xp()[2 * l + 1];
            omy[2 * l] = om.o0(y0, y1);
            omy[2 * l + 1] = om.o1(y0, y1);
        }
        NTM_WSYNC();
        if (l < N) {
            const double* cl = w.Gt() + w.gidx(2 * l, l) - 2 * l;
            const double g2 = dot_rows2<NTM_CH, P>(w, cl, omy, N, l);   // terms i < l masked
            double gu = 2 * g2;
            if constexpr (ru_on<W>()) gu = gu + 2 * pb.Ru * w.U()[l];  // + 2 Ru U_l
            res = w.D()[l] * gu + w.F()[l];
        }
        }
        NTM_ACC(ST_K_GRAD, tp);
        if (sq) {
            // square path: the multipliers from E' mu = grad_F (E upper triangular in
            // sorted order), back substitution; lane t owns row t and grad at f_t
            if (l < N && !fixed) w.d()[fpos] = res;
            NTM_WSYNC();
            const int n = nS - (xb >= 0 ? 1 : 0) - (xb2 >= 0 ? 1 : 0);
            int pl = l + ((nc >= 0 && l >= nc) ? 1 : 0);             // lane t's pivot column
            if (kCollision && nc2 >= 0 && pl >= nc2) ++pl;
            if (kColl3 && nc3 >= 0 && pl >= nc3) ++pl;
            double acc = (l < n) ? w.d()[pl] : 0.0, mu = 0.0;
            // one collision: a second right-hand side, the left-out row B at the pivot columns
            double acb = (kCollision && xb >= 0 && l < n) ? gen_n(xb, w.fidx()[pl]) : 0.0, mb = 0.0;
            double acb2 = (kColl2 && xb2 >= 0 && l < n) ? gen_n(xb2, w.fidx()[pl]) : 0.0, mb2 = 0.0;
            if constexpr (esub_lanes_ok<P, NTM_CH, W>()) {
                // the slim far N = 20 kernels: descending batches of five under narrowed EXEC (bsub_lanes)
                const unsigned col = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)(w.Ep() + l);
                bsub_lanes(__builtin_amdgcn_readfirstlane(n), acc, mu, sq_id, col);
            } else {
            // E[u][l] loaded kAheadB steps ahead (long horizons: NTM_MU_AHEAD; a register queue)
            constexpr int kAheadB = (W::kNN > 32) ? NTM_MU_AHEAD : 0;
            double bq[kAheadB > 0 ? kAheadB : 1];
#pragma unroll
            for (int a = 0; a < kAheadB; ++a) {
                const int ua = n - 1 - a;
                bq[a] = (ua >= 0 && l < ua) ? w.Ep()[w.eidx(ua, l)] : 0.0;
            }
            constexpr bool kPreB = NTM_SUB_PRESCALE && W::kNN > 32;   // as the forward substitution
            if constexpr (kPreB) { acc *= sq_id; acb *= sq_id; acb2 *= sq_id; }
            for (int u = n - 1; u >= 0; --u) {
                double eu;
                if constexpr (kAheadB > 0) {
                    eu = bq[0];
#pragma unroll
                    for (int a = 0; a + 1 < kAheadB; ++a) bq[a] = bq[a + 1];
                    const int ua = u - kAheadB;
                    bq[kAheadB - 1] = (ua >= 0 && l < ua) ? w.Ep()[w.eidx(ua, l)] : 0.0;
                } else {
                    eu = (l < u) ? w.Ep()[w.eidx(u, l)] : 0.0;
                }
                if constexpr (kPreB) eu *= sq_id;
                const double mu_u = gbcast<P>(kPreB ? acc : acc * sq_id, u);
                if (l == u) mu = mu_u;
                acc -= eu * mu_u;
                if (kCollision && xb >= 0) {
                    const double mb_u = gbcast<P>(kPreB ? acb : acb * sq_id, u);
                    if (l == u) mb = mb_u;
                    acb -= eu * mb_u;
                }
                if (kColl2 && xb2 >= 0) {
                    const double mb2_u = gbcast<P>(kPreB ? acb2 : acb2 * sq_id, u);
                    if (l == u) mb2 = mb2_u;
                    acb2 -= eu * mb2_u;
                }
            }
            }
            if (kColl2 && xb2 >= 0) {
                // mu = a - mu_1 b1 - mu_2 b2; the two hole columns' equations give mu_1, mu_2:
                // mu_1 (n_B1[h] - E_h' b1) + mu_2 (n_B2[h] - E_h' b2) = grad[h] - E_h' a
                const double e1 = (l < n && nc < pl) ? gen_n(perm[l], w.fidx()[nc]) : 0.0;
                const double e2 = (l < n && nc2 < pl) ? gen_n(perm[l], w.fidx()[nc2]) : 0.0;
                const double sa1 = gsum<P>(e1 * mu), s11 = gsum<P>(e1 * mb), s12 = gsum<P>(e1 * mb2);
                const double sa2 = gsum<P>(e2 * mu), s21 = gsum<P>(e2 * mb), s22 = gsum<P>(e2 * mb2);
                double m11 = gen_n(xb, w.fidx()[nc]) - s11, m12 = gen_n(xb2, w.fidx()[nc]) - s12;
                double m21 = gen_n(xb, w.fidx()[nc2]) - s21, m22 = gen_n(xb2, w.fidx()[nc2]) - s22;
                double q1 = w.d()[nc] - sa1, q2 = w.d()[nc2] - sa2;
                double det = m11 * m22 - m12 * m21;
                if (kColl3 && nc3 >= 0) {
                    // k = 1: three hole equations, two unknowns; the best-conditioned pair
                    const double e3 = (l < n && nc3 < pl) ? gen_n(perm[l], w.fidx()[nc3]) : 0.0;
                    const double sa3 = gsum<P>(e3 * mu), s31 = gsum<P>(e3 * mb), s32 = gsum<P>(e3 * mb2);
                    const double m31 = gen_n(xb, w.fidx()[nc3]) - s31, m32 = gen_n(xb2, w.fidx()[nc3]) - s32;
                    const double q3 = w.d()[nc3] - sa3;
                    const double det13 = m11 * m32 - m12 * m31, det23 = m21 * m32 - m22 * m31;
                    if (fabs(det13) > fabs(det) && fabs(det13) >= fabs(det23)) {
                        m21 = m31; m22 = m32; q2 = q3; det = det13;
                    } else if (fabs(det23) > fabs(det)) {
                        m11 = m31; m12 = m32; q1 = q3; det = -det23;   // rows (3, 2): det = m31 m22 - m32 m21
                    }
                }
                const double mu1 = (m22 * q1 - m12 * q2) / det, mu2 = (m11 * q2 - m21 * q1) / det;
                mu -= mu1 * mb + mu2 * mb2;
                if (l == 0) { w.np()[xb] = mu1; w.np()[xb2] = mu2; }
            } else if (kCollision && xb >= 0) {
                // mu = a - mu_B b; a hole column's equation gives mu_B (with two holes,
                // k = 1, the one with the larger pivot; the other holds at the optimum)
                const double eh = (l < n && nc < pl) ? gen_n(perm[l], w.fidx()[nc]) : 0.0;
                const double sa = gsum<P>(eh * mu), sb = gsum<P>(eh * mb);
                double den = gen_n(xb, w.fidx()[nc]) - sb;
                double muB = (w.d()[nc] - sa) / den;
                if (nc2 >= 0) {
                    const double eh2 = (l < n && nc2 < pl) ? gen_n(perm[l], w.fidx()[nc2]) : 0.0;
                    const double sa2 = gsum<P>(eh2 * mu), sb2 = gsum<P>(eh2 * mb);
                    const double den2 = gen_n(xb, w.fidx()[nc2]) - sb2;
                    if (fabs(den2) > fabs(den)) { den = den2; muB = (w.d()[nc2] - sa2) / den2; }
                }
                if (kColl3 && nc3 >= 0) {                  // k = 2: a third hole
                    const double eh3 = (l < n && nc3 < pl) ? gen_n(perm[l], w.fidx()[nc3]) : 0.0;
                    const double sa3 = gsum<P>(eh3 * mu), sb3 = gsum<P>(eh3 * mb);
                    const double den3 = gen_n(xb, w.fidx()[nc3]) - sb3;
                    if (fabs(den3) > fabs(den)) { den = den3; muB = (w.d()[nc3] - sa3) / den3; }
                }
                mu -= muB * mb;
                if (l == 0) w.np()[xb] = muB;
            }
            if (l < n) w.np()[perm[l]] = mu;
            NTM_WSYNC();
        }
        NTM_ACC(ST_K_MU, tp);
        // - sum_s mu_s n_s[l]: for state rows n_s[l] = -ssg_s Gamma_{r_s l} D_l irn_{r_s},
        // i.e. + D_l sum_s Gamma_{r_s l} z_s with z_s = mu_s ssg_s irn_{r_s}: a sparse
        // pass over the nS active general rows only (z_s scratch in w.Phi(), dead
        // until the next lift; rows r_s >= 2N are rate rows, handled directly)
        double* const z = w.Phi();
        // (NTM_SUB_LANEIDX, long horizons) row s's index and z_s stay on lane s and the
        // column loop takes them by readlane: one LDS round trip per batch instead of two
        constexpr bool kSubLane = NTM_SUB_LANEIDX && P == 64 && (W::kNN > 32 || W::kNN == 0);
        int rsl = 0;
        double zsl = 0.0;
        if (l < nS) {
            const int r = w.srw()[l];
            const double zl = (r < 2 * N) ? (w.np()[l] * w.ssg()[l]) * w.irn()[r] : 0.0;
            if constexpr (kSubLane) { rsl = r; zsl = zl; }
            else z[l] = zl;
        }
        if constexpr (!kSubLane) NTM_WSYNC();
        if (l < N) {
            const double* cl = w.Gt() + w.gidx(2 * l, l) - 2 * l;   // cl[r] = gt(r, l), r >= 2l
            double sub = 0.0;
            constexpr int CH = NTM_CH;
            NTM_CHUNK_PRAGMA
            for (int s0 = 0; s0 < nS; s0 += CH) {
                int rr[CH];
                double zv[CH], gv[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const bool in = s0 + u < nS;
                    if constexpr (kSubLane) {
                        const int src = __builtin_amdgcn_readfirstlane(s0 + u) & 63;
                        rr[u] = in ? __builtin_amdgcn_readlane(rsl, src) : 0;
                        zv[u] = in ? gbcast<P>(zsl, src) : 0.0;
                    } else {
                        rr[u] = in ? w.srw()[s0 + u] : 0;
                        zv[u] = in ? z[s0 + u] : 0.0;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    const bool on = s0 + u < nS && rr[u] < 2 * N && (rr[u] >> 1) >= l;
                    gv[u] = on ? cl[rr[u]] : 0.0;
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < CH; ++u) sub += gv[u] * zv[u];
            }
            res += w.D()[l] * sub;
        }
        if (W::kNN != 20 && rows.has_rate()) {            // (N = 20 with rate rows runs on the generic kernels)
            // active rate rows (mode 3): row s of input i has normal entries at i and i-1
            // only, so each scatters mu_s n_s into two per-input slots (scratch: w.Vb() and
            // w.d(), dead here) and lane l takes its two; one active rate row per input at
            // most (both directions of one input active is singular, rejected above).
            // Replaces an nS-long loop per lane (config 5 mode 3: k_sub 235K cycles per
            // wave-step)
            double* const rhi = w.Vb();
            double* const rlo = w.d();
            if (l < N) { rhi[l] = 0.0; rlo[l] = 0.0; }
            NTM_WSYNC();
            if (l < nS && w.srw()[l] >= 2 * N) {
                const int i = w.srw()[l] - 2 * N;
                const double m = w.np()[l];
                rhi[i] = m * gen_n(l, i);
                rlo[i - 1] = m * gen_n(l, i - 1);
            }
            NTM_WSYNC();
            if (l < N) res -= rhi[l] + rlo[l];
        }
        NTM_ACC(ST_K_SUB, tp);
        if constexpr (kRefine) {
            if (resid) {
                // right-hand side -[r1; r2] in bordered-row order (scratch: w.Phi(), dead
                // after the sparse pass above), then L_A z = b, L_A' x = diag(I, -I) z
                NTM_WSYNC();
                if (l < N && !fixed) z[fpos] = -res;
                if (l < nS) z[nF + l] = -r2;
                NTM_WSYNC();
                auto slot_of = [&](const double* v, int k) -> double {   // v[k / P] (k uniform)
                    double o = v[0];
#pragma unroll
                    for (int r = 1; r < RPL; ++r) o = (k / P == r) ? v[r] : o;
                    return o;
                };
                double acc[RPL], xr[RPL];
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
                    acc[r] = (lr < nt) ? z[lr] : 0.0;
                    xr[r] = 0.0;
                }
                for (int k = 0; k < nt; ++k) {             // forward: L_A z = b
                    const double zk = gbcast<P>(slot_of(acc, k), k % P) * w.ldi()[k];
#pragma unroll
                    for (int r = 0; r < RPL; ++r) {
                        const int lr = l + r * P;
                        if (lr == k) xr[r] = zk;
                        if (lr > k && lr < nt) acc[r] -= Lp[w.brow(lr) + w.bcol(k, nt)] * zk;
                    }
                }
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
                    acc[r] = (lr < nF) ? xr[r] : -xr[r];
                    xr[r] = 0.0;
                }
                for (int k = nt - 1; k >= 0; --k) {        // backward: L_A' x = diag(I, -I) z
                    const double xk = gbcast<P>(slot_of(acc, k), k % P) * w.ldi()[k];
#pragma unroll
                    for (int r = 0; r < RPL; ++r) {
                        const int lr = l + r * P;
                        if (lr == k) xr[r] = xk;
                        if (lr < k) acc[r] -= Lp[w.brow(k) + w.bcol(lr, nt)] * xk;
                    }
                }
                // x = [dV_F; -dmu]: V_F in rows < nF <= N <= P (slot 0)
                const double dvs = __shfl(xr[0], (l < N && !fixed) ? fpos : 0, P);
                const double vr = fixed ? vfin : vfin + dvs;
                bool good = !(l < N) || isfinite(vr);
                NTM_WSYNC();
#pragma unroll
                for (int r = 0; r < RPL; ++r) {
                    const int lr = l + r * P;
                    if (lr >= nF && lr < nt) good = good && isfinite(w.np()[lr - nF] - xr[r]);
                }
                good = !gany<P>(!good);
                if (good) {
                    vfin = vr;
#pragma unroll
                    for (int r = 0; r < RPL; ++r) {
                        const int lr = l + r * P;
                        if (lr >= nF && lr < nt) w.np()[lr - nF] -= xr[r];
                    }
                }
                NTM_WSYNC();
                refine = false;
                y_ready = false;                           // V moved: y again
                continue;
            }
        }
        // A fixed variable's multiplier res / hv, once.  hv is exactly -+1 for a
        // variable fixed by an input bound (classification above), so the quotient is
        // +-res bit for bit; only a single-entry state row (|hv| != 1) needs the IEEE
        // division: one ballot and a group-uniform branch
        const double hvl = fixed ? w.hv()[l] : 1.0;
        double lamf;
        if (gany<P>(fixed && fabs(hvl) != 1.0)) lamf = res / hvl;
        else lamf = hvl > 0.0 ? res : -res;
        if (mult_out) {                                    // by active position
            if (l < nS) mult_out[w.sidx()[l]] = w.np()[l];
            if (fixed) mult_out[w.fx()[l] - 1] = lamf;
        }
#ifdef NTM_STAMPS
        if (!dir) {                                        // non-finite multipliers, by re-solve path
            const bool nanm = gany<P>((l < nS && !isfinite(w.np()[l])) || (fixed && !isfinite(lamf)));
            const bool nanv = gany<P>(l < N && !isfinite(vfin));
            if (nanm) {
                if (!sq) NTM_CNT(CN_NAN_BORD);
                else if (xb2 >= 0) NTM_CNT(CN_NAN_COLL2);
                else if (xb >= 0) NTM_CNT(CN_NAN_COLL);
                else if (kdim == 0) NTM_CNT(CN_NAN_K0);
                else if (kdim == 1) NTM_CNT(CN_NAN_K1);
                else NTM_CNT(CN_NAN_K2);
                if (!ok) NTM_CNT(CN_NAN_PRIMFAIL);
                if (nanv) NTM_CNT(CN_NAN_V);
            }
        }
#endif
        if (dir) {
            ok = !gany<P>((l < nS && !isfinite(w.np()[l])) || (fixed && !isfinite(lamf)));
            fk = ok ? 0 : 3;
            break;
        }
        // multipliers: general row s on lane s, fixed variable j on lane j; each
        // lane keeps its most negative one and that row's active-list position
        double mval = 0.0;
        int mpos = 0x7fffffff;
        bool has = false;
        if (l < nS) { mval = w.np()[l]; mpos = w.sidx()[l]; has = true; }
        if (!(fabs(mval) < kInf)) mval = -1e300;         // a non-finite multiplier fails the dual check
        if (fixed) {
            double lam = lamf;
            if (!(fabs(lam) < kInf)) lam = -1e300;
            if (!has || lam < mval) { mval = lam; mpos = w.fx()[l] - 1; }
            has = true;
        }
        double mabs = gmax<P>(has ? fabs(mval) : 0.0);
        // The dual test is a predicate over the lanes' own multipliers: the smallest
        // one is below the threshold iff some lane's is (the key of a lane without a
        // multiplier was +inf, non-finite ones are -1e300 already).  The argmin's
        // position is read by the callers only after a failed certificate (the drop
        // position, or the slot an exchange overwrites), so it runs only then
        const bool dual_ok = !gany<P>(has && mval < -1e-9 * fmax(1.0, mabs));
        fk = !ok ? (dual_ok ? 2 : 4) : (!dual_ok ? 1 : 0);
        if (fail_pos && !(ok && dual_ok)) {
            double mkey = has ? mval : kInf;
            gargmin<P>(mkey, mpos);
            fpos_out = mpos;
        }
        ok = ok && dual_ok;
        break;
    }
    // ok needs no further reduction here, at any P: it is the certificate loop's own
    // condition, and that loop runs collectives (gmax, the check, the ballots), so it
    // was group-uniform on entry; inside the loop it is only assigned results of
    // collectives (the primal check's pick, the multipliers' finiteness, dual_ok).
    // Before the loop, the solves set it from scalars that are bit-identical across
    // the group: sums out of gsum (det, h11, num, den, the plane systems' terms) and
    // pivots out of gbcast (dk), besides collide and the substitution's ballot.  The
    // old reduction was also a safety net at P < 64 against a future per-lane term;
    // whoever adds one must reduce it where it is formed
    NTM_ACC(ST_P_KKT, tp);
    if (fail_kind) *fail_kind = uni<P>(fk);
    if (fail_pos) *fail_pos = uni<P>(fpos_out);
    if (v_out) *v_out = vfin;
    if (dir) {
        NTM_WSYNC();
        return ok;
    }
    if (verify_only && !ok) {
        if (l < N) w.V()[l] = Vprev;
        NTM_WSYNC();
        return false;
    }
    if (l < N) {
        w.U()[l] = ok ? (fixed ? uf : vfin * w.D()[l]) : Vprev * w.D()[l];
        w.V()[l] = ok ? vfin : Vprev;
    }
    NTM_WSYNC();
    return ok;
}

// ---------------------------------------------------------------------------
// rollout + scheduling update + convergence (NTM_MPC_Sim.m:110-117, 123-127)
// Returns (group-uniform) whether sum|Uold - U| < eps; updates Uold.
// ---------------------------------------------------------------------------
// With y_valid (the QP's U was certified by polish_compact, which leaves y = Gamma U
// in w.xp()) the rollout is the lifted prediction itself: x^_{i+1} = e_i + (Gamma U)_i
// with e = Phi x_k + Lambda, one row per lane.  That is the rollout identity the
// oracle tests pin (CANON D4/D6: Phi x_0 + Gamma U + Lambda == the recursion of
// NTM_MPC_Sim.m:113 with this iteration's rho), evaluated in another order: the
// same states to rounding, without the N-step serial recursion.  Otherwise (GI's
// uncertified result, a non-optimal flag, the literal D4/D6 lifts, for which the
// identity does not hold) the recursion runs on lane 0 as the reference writes it.
template <int P, class W>
__device__ __forceinline__ bool rollout_phase(const Prob& pb, const W& w, double x0, double x1, int l,
                                              bool y_valid = false) {
    const int N = w.n();
    const Coef k = scn_coef(pb, w);
    if constexpr (W::kNN == 0) {
        if (pb.flags & (NTM_LITERAL_PHI_RIGHTMUL | NTM_LITERAL_GAMMA_INDEX)) y_valid = false;
    }
    constexpr int RR = W::kNN > 0 ? (2 * W::kNN + P - 1) / P : 2;   // rows per lane (2N <= 2P)
    if (y_valid) {
        double v[RR];
#pragma unroll
        for (int t = 0; t < RR; ++t) {
            const int r = l + t * P;
            v[t] = (r < 2 * N) ? w.e()[r] + w.xp()[r] : 0.0;
        }
        NTM_WSYNC();
#pragma unroll
        for (int t = 0; t < RR; ++t) {
            const int r = l + t * P;
            if (r < 2 * N) w.xp()[r + 2] = v[t];
        }
        if (l == 0) {
            w.xp()[0] = x0;
            w.xp()[1] = x1;
        }
    } else if (l == 0) {
        double y0 = x0, y1 = x1;
        w.xp()[0] = y0;
        w.xp()[1] = y1;
        constexpr int CH = NTM_CH;                   // the loads of CH steps ahead of their stores
        NTM_CHUNK_PRAGMA
        for (int i0 = 0; i0 < N; i0 += CH) {
            double ca[CH], cb[CH], cc[CH], cu[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                if constexpr (W::kSlim) {           // the lift's coefficients, from this iteration's rho
                    ca[u] = i < N ? coef_a11(k, w.rho()[3 * i]) : 0.0;
                    cb[u] = i < N ? coef_b(k, w.rho()[3 * i + 2]) : 0.0;
                    cc[u] = i < N ? coef_a21(k, w.rho()[3 * i + 1]) : 0.0;
                } else {
                    ca[u] = i < N ? w.a11()[i] : 0.0;
                    cb[u] = i < N ? w.bb()[i] : 0.0;
                    cc[u] = i < N ? w.a21()[i] : 0.0;
                }
                cu[u] = i < N ? w.U()[i] : 0.0;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int i = i0 + u;
                if (i < N) {
                    const double n0 = (ca[u] * y0 + cb[u] * cu[u]) + k.C1;
                    const double n1 = (cc[u] * y0 + k.a22 * y1) + k.C2;
                    y0 = n0;
                    y1 = n1;
                    w.xp()[2 * i + 2] = y0;
                    w.xp()[2 * i + 3] = y1;
                }
            }
        }
    }
    NTM_WSYNC();
    double dsum = 0.0, u = 0.0;
    if (l < N) {
        double r1, r2, r3;
        const dpair xv = ld_pair<pair_ld_ok<P, W>()>(w.xp() + 2 * l);
        rho_eval(k, xv.x, xv.y, r1, r2, r3);
        w.rho()[3 * l] = r1;
        w.rho()[3 * l + 1] = r2;
        w.rho()[3 * l + 2] = r3;
        u = w.U()[l];
        dsum = fabs(w.Uold()[l] - u);
    }
    const bool conv = gsum<P>(dsum) < pb.eps;      // :123
    if (!conv && l < N) w.Uold()[l] = u;           // :127; the break at :125 skips it
    NTM_WSYNC();
    return conv;
}

// plant step NTM_MPC_Sim.m:130 (CANON D13: plant = prediction model, + C), plus
// the scenario's disturbance realisation at time index kt (ntm_ctx_set_scenarios;
// the model the controller predicts with does not know it)
template <bool GEN = false>
__device__ __forceinline__ void plant_step(const Prob& pb, const Coef& k, double x0, double x1, double u,
                                           double& n0, double& n1, int64_t gid = 0, int kt = 0) {
    double r1, r2, r3;
    rho_eval(k, x0, x1, r1, r2, r3);
    double a11 = coef_a11(k, r1), a21 = coef_a21(k, r2), b = coef_b(k, r3);
    n0 = a11 * x0 + b * u;
    n1 = a21 * x0 + k.a22 * x1;
    if (!(pb.flags & NTM_LITERAL_PLANT_NO_C)) { n0 += k.C1; n1 += k.C2; }
    if (GEN && gen_dist(pb)) {
        if (pb.g.sw != 0.0) n0 += pb.g.sw * gen_normal(pb.g.seed, gid, (uint32_t)kt, 0);
        if (pb.g.so != 0.0) n1 += pb.g.so * gen_normal(pb.g.seed, gid, (uint32_t)kt, 1);
    }
}

// ---------------------------------------------------------------------------
// Receding-horizon shift of a carried warm-start set, into w.act() (returns
// the shifted count).  The previous step planned stages k..k+N-1; this step
// plans k+1..k+N, so a row of stage i >= 1 moves to stage i-1, stage-0 rows
// are dropped, and the bound rows of the old last input and the terminal state
// rows are kept for the new last stage as well.  It is the SECOND candidate of inner iteration 2, after
// the unshifted set: in the closed loop's steady state the LPV iteration
// 2-cycles through the same pair of active sets every step (the odd and even
// iterations), so the previous step's set hits unshifted (70% at iteration 2
// over steps 5-20, against 7% shifted; 36% vs 31% over steps 1-4, where the
// plan still moves in time).  Only a hint: every candidate is re-solved
// exactly and KKT-certified.
// ---------------------------------------------------------------------------
template <int P, class W>
__device__ __forceinline__ int shifted_into_act(const Prob& pb, const W& w, const int* c, int l, bool hint_only = false) {
    const int N = w.n();
    const int lane = threadIdx.x & 63;
    const unsigned long long gmask = (P == 64) ? ~0ull : (((1ull << P) - 1ull) << (lane & ~(P - 1)));
    const unsigned long long below = (1ull << lane) - 1ull;
    const int q = uni<P>(c[N]);
    int nid = -1, dup = -1;
    if (l < q) {
        const int id = c[l];
        if (pb.mode == NTM_MODE_BOX) {
            const int j = id < N ? id : id - N;
            if (j >= 1) nid = id - 1;
            if (j == N - 1) dup = id;
        } else if (id >= 6 * N + 4) {                    // rate row of input j
            const int j = ((id - (6 * N + 4)) >> 1) + 1;
            if (j >= 2) nid = id - 2;
            if (j == N - 1) dup = id;
        } else if (id >= 6 * N) {                        // terminal state row -> stage N-1, and kept
            nid = 6 * (N - 1) + 2 + (id - 6 * N);
            dup = id;
        } else {
            const int blk = id / 6, rr = id - 6 * blk;
            if (blk >= 2 || (blk == 1 && rr < 2)) nid = id - 6;   // x_1's state rows would become
            if (blk == N - 1 && rr < 2) dup = id;                  // x_0 rows (constant): dropped
        }
    }
    if (hint_only) {                                     // flag the shifted rows (kCandRow) instead
        if (nid >= 0) w.aflag()[nid] = kCandRow;
        if (dup >= 0) w.aflag()[dup] = kCandRow;
        NTM_WSYNC();
        return 0;
    }
    const unsigned long long bk = __ballot(nid >= 0) & gmask;
    const unsigned long long bd = __ballot(dup >= 0) & gmask;
    const int nk = uni<P>((int)__popcll(bk)), nd = uni<P>((int)__popcll(bd));
    const bool with_dup = nk + nd <= N;
    if (nid >= 0) w.act()[__popcll(bk & below)] = nid;
    if (with_dup && dup >= 0) w.act()[nk + __popcll(bd & below)] = dup;
    NTM_WSYNC();
    return nk + (with_dup ? nd : 0);
}

// ---------------------------------------------------------------------------
// qp_phase's Goldfarb-Idnani fallback (the full G~, GI warm-started from the
// failed candidate, then its certified polish; ~2.5% of the QPs at N = 20).
// Inlined like every other phase.  DUAL (ntm_mpc_step_dual): the polish writes its
// certified multipliers to w.uu() by active position, as the dual path does; where
// it does not certify, GI's own stay there.
// ---------------------------------------------------------------------------
template <int P, class W, bool DUAL = false>
__device__ __forceinline__ int gi_fallback(const Prob& pb, const W w, const StructRows rows, int nrows, int l, int nwarm,
                                           int it, int* qp_iters, int* q_out, int* ns_out, bool* yv_out) {
    NTM_T0(tq);
    int flag, q = 0, ns = 0;
    bool yv = false;
    if (!full_gram<P>(pb, w, l)) {
        flag = NTM_EXIT_NONFINITE;
    } else {
        NTM_ACC(ST_REGRAM, tq);
        NTM_CNT(CN_GIRUN);
        if (it == 1) NTM_CNT(CN_GI_IT1); else if (it == 2) NTM_CNT(CN_GI_IT2); else NTM_CNT(CN_GI_LATE);
        // warm from the failed candidate; if its multipliers are not all >= 0, warm
        // again from the rows whose multipliers were; then cold
        for (int pass = 0;; ++pass) {
            flag = gi_solve<P, StructRows, W>(w, rows, pb.mode != NTM_MODE_NONE, nrows, l, qp_iters, &q,
                                              pass < 2 ? nwarm : 0);
            if (flag != kGiWarmRejected) break;
            nwarm = (pass == 0) ? q : 0;
            q = 0;
            if (!full_gram<P>(pb, w, l)) { flag = NTM_EXIT_NONFINITE; break; }
        }
        NTM_ACC(ST_GI, tq);
        if (flag == NTM_EXIT_OPTIMAL) {
            bool okp;
            if constexpr (DUAL) {
                const double ugi = (l < q) ? w.uu()[l] : 0.0;
                NTM_WSYNC();
                okp = polish_compact<P>(pb, w, rows, q, l, false, &ns, nullptr, nullptr, nullptr, w.uu());
                if (!okp && l < q) w.uu()[l] = ugi;
                NTM_WSYNC();
            } else {
                okp = polish_compact<P>(pb, w, rows, q, l, false, &ns);
            }
            NTM_TRACE("QP GI flag %d q %d polish %d\n", flag, q, (int)okp);
            yv = okp;
        }
        NTM_ACC(ST_POLISH, tq);
    }
    *q_out = q;
    *ns_out = ns;
    *yv_out = yv;
    return flag;
}

// ---------------------------------------------------------------------------
// one inner iteration's QP: build -> scale -> GI -> polish -> w.U()
// ---------------------------------------------------------------------------
template <int P, class W, bool DUAL = false>
__device__ __forceinline__ int qp_phase(const Prob& pb, const W& w, double x0, double x1, int l, int* qp_iters,
                        int* q_out, int* ns_out, int slot, int* n_try = nullptr, int* n_girun = nullptr,
                        int it = 0, bool* y_valid = nullptr) {
    const int N = w.n();
    bool yv = false;                                     // w.xp() holds Gamma U of the final U
    NTM_T0(tq);
    ColSums colsum;
    lift_phase<P>(pb, w, l, x0, x1, &colsum);
    NTM_ACC(ST_LIFT, tq);
    free_response<P>(w, x0, x1, l, &pb);     // F is formed with the Jacobi scaling below
    NTM_ACC(ST_COST, tq);
    const bool full = pb.mode >= NTM_MODE_FULL;        // state rows present
    int flag, q = 0, ns = 0;
    *qp_iters = 0;
    StructRows rows(pb);
    int* cand = w.cand() + slot * (N + 1);               // this QP's active set is stored here
    const int scode = diag_scale_phase<P>(pb, w, l, full, x0, x1, &colsum);
    if (scode >= 2) {
        flag = NTM_EXIT_NONFINITE;
    } else {
        const int nrows = (pb.mode == NTM_MODE_NONE) ? 0 : rows.rows();
        if (pb.mode != NTM_MODE_NONE) {
            for (int i = l; i < nrows; i += P) w.aflag()[i] = 0;
            NTM_WSYNC();
        }
        bool infeasible;                                   // a constant row violated (D15, D22)
        if constexpr (fold_const<W>()) infeasible = pb.mode != NTM_MODE_NONE && scode == 1;
        else infeasible = pb.mode != NTM_MODE_NONE && !rows.template feasible_const<P>(w, x0, x1, l);
        if (infeasible) {
            flag = NTM_EXIT_INFEASIBLE;
        } else {
            NTM_ACC(ST_SCALE, tq);
            bool done = false;
            int nwarm = 0;
            // warm start: the LPV loop alternates between two QPs (a 2-cycle),
            // so the active set of iteration it-2 is tried first; it is taken
            // only if the exact active-set solve passes the KKT certificate
            // (the optimum of this strictly convex QP is unique).
            const int cq0 = uni<P>(cand[N]);
            if (cq0 >= 0) {
                NTM_CNT(CN_CAND);
                int cq = cq0;
                // long horizons shift the carried set first at iteration 2: offline
                // (NumPy oracle, steps 5-12) the receding-horizon shift of the previous
                // step's last even set is iteration 2's optimum for 75% of the N = 50
                // scenario-steps (mode 2; 72% in mode 3) and the unshifted set for 19%;
                // at N = 20 the unshifted set wins (55% against 18%)
                const bool shift_first = (W::kNN > 32 || (W::kNN == 0 && N > 32)) && it == 2 &&
                                         pb.mode != NTM_MODE_NONE;
                if (shift_first) {
                    cq = shifted_into_act<P>(pb, w, cand, l);
                } else {
                    if (l < cq) w.act()[l] = cand[l];
                    NTM_WSYNC();
                }
#ifdef NTM_DEBUG_SCEN
                NTM_TRACE("SET it %d cand %d:", it, cq);
                for (int i = 0; i < cq; ++i) NTM_TRACE(" %d", w.act()[i]);
                NTM_TRACE("\n");
#endif
                // Certified dual path (round 5).  The candidate's re-solve either
                // certifies, or it gives the set's equality-constrained optimum and
                // multipliers.  A set whose multipliers are not all >= 0 first drops
                // its most negative one, re-solving each time, until it is dual
                // feasible.  From there Goldfarb & Idnani's dual method runs with
                // certified re-solves as its linear algebra: the most violated row p
                // is added; the re-solve on A + {p} is the end point of GI's (linear)
                // step, so a multiplier of A that is negative there is dropped at the
                // fraction of the step where it reaches zero (V and the multipliers
                // interpolated), and A - {i} + {p} is re-solved; a row p dependent on
                // A (a full set: q = N) takes GI's dual-only step, with r from the
                // certificate's multiplier pass on n_p (polish_compact, dir_p).  The
                // last re-solve of a full step that passes the KKT certificate is
                // the answer.  Offline (tools/repair_study.py, N = 20 mode 2, steps
                // 6-25): every iteration-2 QP certifies, 3.2 re-solves on average,
                // where the single-row repairs left 16% to Goldfarb-Idnani.  GI itself
                // (warm from the current set) is the fallback when the budget runs
                // out or the set degenerates.
                // Iteration 2: a singular carried set is replaced by the other form
                // (shifted or unshifted) of the previous step's last even set.
                bool alt = it == 2 && pb.mode != NTM_MODE_NONE;
                const int budget = N + kCdpExtra;
                // drop position `pos` of the active list (and of the lane-per-position u)
                auto drop_at = [&](int pos, double& u) {
                    int an = 0;
                    if (l >= pos && l + 1 < cq) an = w.act()[l + 1];
                    const double un = __shfl(u, (l + 1) & (P - 1), P);
                    NTM_WSYNC();
                    if (l >= pos && l + 1 < cq) w.act()[l] = an;
                    if (l >= pos) u = (l + 1 < cq) ? un : 0.0;
                    --cq;
                    NTM_WSYNC();
                };
                // One polish_compact call site (the kernel inlines it): each trip re-solves
                // qs rows (A, or A + {p} at position cq) or, with dirp >= 0, takes the
                // dual-only direction of row dirp on A.  stage 0: the carried set;
                // 1: dropping negative multipliers; 2: A + {p}; 3: the direction of p
                int stage = 0, qs = cq, dirp = -1, p = -1, nres = 0, fk = 0, fp = 0;
                // Long horizons: an A + {p} whose end point has a non-finite multiplier (p
                // (nearly) depends on A) leaves p out (kSkipRow) and adds another violated row
                // instead, as the dual method may add any violated row; p is eligible again
                // once A changes.  Before round 6 these QPs went to GI (N = 50 mode 2: 0.1 per
                // MPC step, 7% of the cycles)
                constexpr bool kSkipNan = W::kNN > 32 || W::kNN == 0;
                int nskip = 0;
                bool fresh_y = false;                      // the pick recomputes y = Gamma U at V0
                auto clear_skips = [&]() {
                    if (kSkipNan && nskip > 0) {
                        for (int i = l; i < nrows; i += P) w.aflag()[i] &= (unsigned char)~kSkipRow;
                        NTM_WSYNC();
                        nskip = 0;
                    }
                };
                // iteration 2 at N <= 32 starts from the unshifted carried set; the dual
                // path then adds violated rows of its receding-horizon shift first
                // (StructRows::check prefers kCandRow rows).  Offline (tools/repair_study.py,
                // N = 20 mode 2): 2.67 -> 2.50 re-solves per iteration-2 QP; on the device
                // 6.45 -> 6.36 ms per step-batch (A/B on one box).  Not for box-only QPs
                // (their single-row exchanges: config 2 0.206 -> 0.214 ms with it)
                if (alt && !shift_first && pb.mode != NTM_MODE_BOX)
                    (void)shifted_into_act<P>(pb, w, cand, l, true);
                double vf = 0.0, V0 = 0.0, u0 = 0.0;   // V0: lane = variable; u0: lane = active position
                bool okc = false;
                for (;;) {
                    if (n_try && dirp < 0) ++*n_try;
                    const bool oks = polish_compact<P>(pb, w, rows, qs, l, true, &ns, &fk, &fp, &vf, w.uu(), dirp);
                    NTM_TRACE("QP cdp stage %d qs %d dir %d ok %d fk %d fp %d\n", stage, qs, dirp, (int)oks, fk, fp);
                    ++nres;
                    bool pick = false;
                    if (stage == 0) {
                        if (it <= 2) NTM_CNT(CN_TRY_EARLY);
                        if (!oks) { if (it <= 2) NTM_CNT(CN_FAIL_EARLY); else NTM_CNT(CN_FAIL_LATE); }
                        if (it <= 2 && !oks) {
                            if (fk == 1) NTM_CNT(CN_FK_DUAL);
                            else if (fk == 2) NTM_CNT(CN_FK_PRIMAL);
                            else if (fk == 3) NTM_CNT(CN_FK_SING);
                            else NTM_CNT(CN_FK_BOTH);
                        }
                        if (it == 1) { NTM_CNT(CN_TRY_IT1); if (!oks) NTM_CNT(CN_FAIL_IT1); }
                        if (it == 2) { NTM_CNT(CN_TRY_IT2); if (!oks) NTM_CNT(CN_FAIL_IT2); }
                        if (oks) { okc = true; break; }
                        if (fk == 3) {                     // singular: the other form of the carried set
                            if (!alt) { NTM_CNT(CN_CDPX_SING0); break; }
                            alt = false;
                            NTM_CNT(CN_ALT_TRY);
                            if (shift_first) {
                                cq = cq0;
                                if (l < cq) w.act()[l] = cand[l];
                                NTM_WSYNC();
                            } else {
                                cq = shifted_into_act<P>(pb, w, cand, l);
                            }
                            qs = cq;
                            continue;
                        }
                        stage = pb.mode == NTM_MODE_BOX ? 4 : 1;
                    }
                    if (stage == 4) {
                        // Box-only QPs (BASELINE config 2): single-row exchanges, as before round
                        // 5.  A violated bound joins (with a negative multiplier too, that row
                        // leaves in the same exchange; in a full set it takes the place of the
                        // smallest multiplier); a negative multiplier alone leaves.  Measured on
                        // the all-LDS build at B = 1024 (one wave per SIMD: the longest scenario
                        // decides): 0.281 ms per step with the dual path, 0.262 with 8 exchanges,
                        // 0.224 with 16 (A/B on one box)
                        if (oks) { okc = true; break; }
                        if (fk == 3 || nres > kBoxRepairs) { NTM_CNT(CN_CDPX_BUDGET); break; }
                        if (fk == 1) {
                            double ud = 0.0;
                            drop_at(fp, ud);
                        } else {
                            if (l < cq) w.aflag()[w.act()[l]] = kActiveRow;
                            NTM_WSYNC();
                            const double vmx = fmax(1.0, gmax<P>(l < N ? fabs(vf) : 0.0));
                            const Pick pk = rows.template check<P>(w, vf, l, false, vmx, w.xp());
                            NTM_WSYNC();
                            if (l < cq) w.aflag()[w.act()[l]] = 0;
                            NTM_WSYNC();
                            if (pk.p < 0) break;
                            const int lane = threadIdx.x & 63;
                            const unsigned long long gm = (P == 64) ? ~0ull : (((1ull << P) - 1ull) << (lane & ~(P - 1)));
                            const bool keep = l < cq && !(fk == 4 && l == fp);
                            const unsigned long long km = __ballot(keep) & gm;
                            const int nkeep = uni<P>((int)__popcll(km));
                            const int my = (l < cq) ? w.act()[l] : 0;
                            NTM_WSYNC();
                            if (nkeep < N) {
                                if (keep) w.act()[__popcll(km & ((1ull << lane) - 1ull))] = my;
                                if (l == 0) w.act()[nkeep] = pk.p;
                                cq = nkeep + 1;
                            } else if (l == 0) {
                                w.act()[fp] = pk.p;
                            }
                            NTM_WSYNC();
                        }
                        qs = cq;
                        NTM_CNT(CN_CDP_DROP);
                        continue;
                    }
                    if (stage == 1) {                      // dual feasibility first
                        if (oks) { okc = true; break; }
                        if (fk == 1 || fk == 4) {
                            if (nres >= budget) { NTM_CNT(CN_CDPX_BUDGET); break; }
                            double ud = 0.0;
                            drop_at(fp, ud);
                            qs = cq;
                            NTM_CNT(CN_CDP_DROP);
                            continue;
                        }
                        if (fk != 2) { NTM_CNT(CN_CDPX_SING1); break; }
                        V0 = vf;
                        u0 = (l < cq) ? w.uu()[l] : 0.0;
                        pick = true;
                    } else if (stage == 2) {               // the end point of adding p
                        NTM_CNT(CN_CDP_RES);
                        if (oks) { ++cq; okc = true; break; }
                        if (fk == 3) {                     // A + {p} singular: p depends on A
                            dirp = p;
                            qs = cq;
                            stage = 3;
                            continue;
                        }
                        const double u1 = (l <= cq) ? w.uu()[l] : 0.0;
                        double th = (l < cq && u1 < 0.0) ? u0 / (u0 - u1) : kInf;
                        // a non-finite end-point multiplier (A's or p's own) makes the step
                        // meaningless: th = -1 (a real fraction is in [0, 1)) hands the QP to
                        // GI below instead of reading it as a negative multiplier
                        if (l <= cq && !isfinite(u1)) th = -1.0;
                        int li = l;
                        gargmin<P>(th, li);
                        if (th < 0.0) {
                            NTM_CNT(CN_CDPX_NAN);
                            if (!kSkipNan || nres >= budget) break;
                            if (l == 0) w.aflag()[p] |= kSkipRow;
                            if (l < N) w.U()[l] = w.D()[l] * V0;   // the pick's y at V0, not the end point's
                            NTM_WSYNC();
                            ++nskip;
                            NTM_CNT(CN_CDP_SKIP);
                            pick = true;
                            fresh_y = true;
                        } else if (!(th < kInf)) {         // full step: p joins A
                            if (fk != 2) {
                                // p's own multiplier < 0 at the end point (A's are all >= 0): p
                                // (nearly) depends on A, an ill-conditioned step at long horizons.
                                // GI would take its dual-only step there; so does the path (A, V0
                                // and u0 unchanged).  Dropping that multiplier and continuing
                                // instead measured slower (config 5 mode 2: 112 -> 156 ms)
                                NTM_CNT(CN_CDPX_FULLDUAL);
                                dirp = p;
                                qs = cq;
                                stage = 3;
                                continue;
                            }
                            ++cq;
                            u0 = (l < cq) ? u1 : 0.0;
                            V0 = vf;
                            pick = true;
                            clear_skips();
                        } else {                           // partial step: row li reaches u = 0 and leaves
                            V0 += th * (vf - V0);
                            u0 += th * (u1 - u0);
                            drop_at(li, u0);
                            NTM_CNT(CN_CDP_PART);
                            clear_skips();
                        }
                    } else {                               // dual-only step: n_p = sum_i r_i n_i over A
                        NTM_CNT(CN_CDP_DIR);
                        dirp = -1;
                        if (!oks) { NTM_CNT(CN_CDPX_DIR); break; }
                        const double r = (l < cq) ? w.uu()[l] : 0.0;
                        double tt = (l < cq && r > 0.0) ? u0 / r : kInf;
                        int li = l;
                        gargmin<P>(tt, li);
                        if (!(tt < kInf)) { NTM_CNT(CN_CDPX_TINF); break; }   // no row can leave: GI decides (infeasible)
                        u0 -= tt * r;
                        drop_at(li, u0);
                        clear_skips();
                    }
                    if (pick) {                            // the most violated row at V0 (y of the last re-solve in w.xp())
                        if (l < cq) w.aflag()[w.act()[l]] = kActiveRow;
                        NTM_WSYNC();
                        const double vmx = fmax(1.0, gmax<P>(l < N ? fabs(V0) : 0.0));
                        const Pick pk = rows.template check<P>(w, V0, l, false, vmx, fresh_y ? nullptr : w.xp());
                        fresh_y = false;
                        NTM_WSYNC();
                        if (l < cq) w.aflag()[w.act()[l]] = 0;
                        NTM_WSYNC();
                        // (an input bound counts as violated from the certificate's tolerance on)
                        const double ptol = (pk.p >= 0 && rows.is_bound_row(pk.p, N)) ? rows.template bound_tol<W>() : 1e-9;
                        if (pk.p < 0 || !(pk.s < -ptol * fmax(vmx, fabs(pk.bc)))) {
                            // the only violated rows left are skipped ones (A + {p} had a
                            // non-finite end point: p nearly depends on A): GI's step for a
                            // dependent row, the dual-only direction of the last skipped row p
                            // (round 6), instead of handing the QP to GI
                            if (kSkipNan && nskip > 0 && p >= 0 && nres < budget) {
                                NTM_CNT(CN_CDP_SKIPDIR);
                                dirp = p;
                                qs = cq;
                                stage = 3;
                                continue;
                            }
                            NTM_CNT(CN_CDPX_NOVIOL);
                            break;
                        }
                        p = pk.p;
                    }
                    if (nres >= budget) { NTM_CNT(CN_CDPX_BUDGET); break; }   // add p: A + {p}, or its direction when A is full
                    if (cq >= N) {
                        dirp = p;
                        qs = cq;
                        stage = 3;
                    } else {
                        if (l == 0) w.act()[cq] = p;
                        NTM_WSYNC();
                        qs = cq + 1;
                        stage = 2;
                    }
                }
                if (okc) {
                    flag = NTM_EXIT_OPTIMAL;
                    q = cq;
                    done = true;
                    yv = true;
                    NTM_CNT(CN_HIT);
                    if (nres > 1) NTM_CNT(CN_REPAIR);
                } else {
                    NTM_CNT(CN_CDP_GI);
                    clear_skips();
                    // GI warm from the current set (dual feasible on the primal phase)
                    if (l < cq) {
                        w.aflag()[w.act()[l]] = kCandRow;
                        w.sidx()[l] = w.act()[l];
                    }
                    nwarm = cq;
                    NTM_WSYNC();
                }
                NTM_ACC(ST_CAND, tq);
            }
            if (!done) {
                if (n_girun) ++*n_girun;
                flag = gi_fallback<P, W, DUAL>(pb, w, rows, nrows, l, nwarm, it, qp_iters, &q, &ns, &yv);
            }
        }
    }
    if (flag != NTM_EXIT_OPTIMAL) {
        if (l < N) w.U()[l] = (flag == NTM_EXIT_MAXITER) ? w.V()[l] * w.D()[l] : 0.0;
        if (l == 0) cand[N] = -1;
    } else {
        if (l < q) cand[l] = w.act()[l];
        if (l == 0) cand[N] = q;
    }
    NTM_WSYNC();
#ifdef NTM_DEBUG_SCEN
    NTM_TRACE("SET it %d final %d flag %d:", it, flag == NTM_EXIT_OPTIMAL ? q : -1, flag);
    for (int i = 0; flag == NTM_EXIT_OPTIMAL && i < q; ++i) NTM_TRACE(" %d", cand[i]);
    NTM_TRACE("\n");
#endif
    if (q_out) *q_out = q;
    if (ns_out) *ns_out = ns;
    if (y_valid) *y_valid = yv && flag == NTM_EXIT_OPTIMAL;
    return flag;
}

}  // namespace ntm
