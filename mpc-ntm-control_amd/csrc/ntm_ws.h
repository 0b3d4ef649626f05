// ntm_ws.h — the LPV coefficients (rho_eval, coef_*), the per-scenario LDS workspace (WS,
// its size and its carving), the traits a kernel reads off it (ru_on, qi_on, OmQ) and the
// per-scenario coefficients of the scenario generator (scn_coef, scn_store).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntm_base.h"
#include "ntm_prob.h"

namespace ntm {

// ---------------------------------------------------------------------------
// L0 / L1: scheduling parameters and LPV coefficients
// ---------------------------------------------------------------------------
// rho1.m:2, rho2.m:2, rho3.m:2-3 (same operation order as the oracle)
__device__ __forceinline__ void rho_eval(const Coef& k, double w, double om,
                                         double& r1, double& r2, double& r3) {
    r1 = 1.0 / ((k.rho1_sq ? w * w : w) + k.wmarg2);
    r2 = (w * w) / om;
    double ws = w / k.wdep;
    r3 = (0.25 + 0.24 * ws) / (1 + 1.5 * ws + 0.43 * (ws * ws) + 0.64 * (ws * ws * ws));
}
// A.m:2 entries a11, a21 (a12 = 0, a22 = k.a22); B.m:2 as the column [b; 0] (D5)
__device__ __forceinline__ double coef_a11(const Coef& k, double r1) { return k.a11c * r1 + 1; }
__device__ __forceinline__ double coef_a21(const Coef& k, double r2) { return (r2 * k.Ts) / k.za3; }
__device__ __forceinline__ double coef_b(const Coef& k, double r3) { return k.bc * r3; }

// ---------------------------------------------------------------------------
// per-scenario LDS workspace (all offsets in doubles; see ws_doubles())
// ---------------------------------------------------------------------------
// NN > 0: horizon fixed at compile time (strides become immediates, loops
// unroll); NN == 0: runtime horizon (generic kernels).
// GEN: the kernel is built with the scenario generator (per-scenario plasma in
// the workspace, plant disturbances); without it those paths are compiled out
// (they cost the N=20 step kernel 2% through register allocation even when off)
//
// FAR (ws_far: N = 20 and N > 32): the J/R(/T) block (GI's factors and the
// bordered KKT factor) lives in a per-scenario HBM block (Prob::far, L2-resident
// while the wave runs) instead of LDS, and the echelon re-solve's sorted E moves
// to an LDS block of its own, packed lower triangular (row t at t(t+1)/2).  The
// certified re-solve of an echelon set, the common path, stays LDS-only; GI and
// the bordered elimination read and write HBM.  More scenarios fit a CU:
//   N = 50: 78.5 -> 47.9 KB, 3 scenarios per CU instead of 2 (one wave on each
//           of 3 SIMDs instead of 2; the kernel has the 512-register budget of
//           one wave per SIMD either way);
//   N = 20: 20.4 -> 12.0 KB, 12 scenarios per CU instead of 8, i.e. 3 waves per
//           SIMD, which the kernel is built for (168 VGPRs, NTM_WAVES_PER_EU).
// Neither pays without the occupancy: at 2 waves per SIMD the N = 20 kernel is 6%
// slower with its GI in HBM.  NTM_FAR_N20=0 builds the all-LDS N = 20 kernel.
#ifndef NTM_FAR_N20
#define NTM_FAR_N20 1
#endif
__host__ __device__ constexpr bool ws_far(int NN) { return NN > 32 || (NTM_FAR_N20 && NN == 20); }
// the slim far N = 20 kernels keep the V-space box in LDS, in the lift's a11 / a21 (WS::kBox)
#ifndef NTM_N20_BOX_LDS
#define NTM_N20_BOX_LDS 1
#endif
// The slim far layout (N = 20 far, round 5): 16 scenarios per CU (4 waves per SIMD,
// <= 10,240 B of LDS each) instead of 12.  What leaves LDS: the A/B coefficient
// arrays (each lane keeps its stage's in registers, broadcast by readlane in the
// lift), Phi and Lambda (the lift runs the free response e = Phi x_k + Lambda as a
// recursion of its own, one more lane; 2N of the old Phi stay as the re-solve's
// scratch), the hoisted V-space box (vlo / vhi, recomputed from D), and the
// diagonal reciprocals of the bordered factor and GI's Cholesky (ldi / kdi), which
// move to the far block with the rate-row norms (idun, mode 3 never runs here).
// The Om products are the identity (qi_on), so the certificate's Om y is y itself.
// The slim N = 50 layout (round 5): 4 scenarios per CU (one wave on each SIMD) instead
// of 3, <= 40,960 B each.  Besides the N = 20 slim changes (its Om is general: the
// certificate's Om y goes to the 2N of scratch), rho, U_old and the two carried
// active sets move to the far block (touched once or twice per LPV iteration).
__host__ __device__ constexpr bool ws_slim(int N, bool far) {
    return far && (N == 20 || N == 50);
}
__host__ __device__ constexpr bool slim_far(int N, bool far) { return ws_slim(N, far) && N == 50; }
// the slim N = 20 layout keeps a11 / a21 in LDS after all (2N doubles, paid for by
// active-row flags for the 6N+4 getWLc rows only: mode 3 never runs on these kernels)
__host__ __device__ constexpr int slim_ab(int N, bool far) { return N == 20 && ws_slim(N, far) ? 2 : 0; }

template <int NN, bool GEN = false, bool FAR = ws_far(NN)>
struct WS {
    static constexpr int kNN = NN;
    static constexpr bool kGen = GEN;
    static constexpr bool kFar = FAR;
    static constexpr bool kSlim = ws_slim(NN, FAR);
    int N_rt;
    double* base;
    double* far;       // kFar: this scenario's J/R block in HBM
    __device__ __forceinline__ int n() const { return NN > 0 ? NN : N_rt; }
    __device__ __forceinline__ int ldj() const { return n() | 1; }
    __device__ __forceinline__ int ldg() const { return 2 * n(); }
    // double offsets of each array (n() is launch-uniform, so these fold to scalar math)
    static constexpr int kAB = slim_ab(NN, FAR);           // kSlim: a11 / a21 (N each) in LDS
    static constexpr bool kSF = slim_far(NN, FAR);          // rho, U_old, cand in the far block
    static constexpr int kRL = kSF ? 0 : 3;                 // kSlim: rho's N-vectors in LDS
    // kSlim: the 2N rinfo ints take N doubles, and vlo / vhi / ldi / kdi / idun leave LDS
    static constexpr int kRi = kSlim ? 1 : 2;                // doubles of rinfo per N
    static constexpr int kUo = kSF ? 0 : 1;                  // U_old's N-vector in LDS
    // (the constexpr forms in n are what the accessors below and the alignment asserts behind
    // the struct share)
    static constexpr int oJn(int n) { return (kSlim ? kRL + 4 + kAB : 14) * n + n * (n + 1); }
    __device__ __forceinline__ int oJ() const { return oJn(n()); }
    __device__ __forceinline__ int oR() const { return oJ() + n() * ldj(); }
    // T = R^{-1} is kept for N <= kMaxNT only: at long horizons its N^2 doubles would
    // halve the scenarios per CU, and the dual direction falls back to back substitution.
    // The far layouts keep no T either: maintaining it in HBM (a column per add, a
    // Givens sweep and a row shift per drop) cost more than the back substitution
    // on R saves (N = 20, 3 waves per SIMD: 10.09 -> 9.99 ms per step-batch without it)
    __device__ __forceinline__ bool useT() const { return !kFar && n() <= kMaxNT; }
    __device__ __forceinline__ int oT() const { return oR() + (n() + 1) * ldj(); }
    // kFar: the E block (packed lower-triangular E, then 2(N+1) ints) replaces J/R/T in LDS
    static constexpr int oVfar(int n) { return oJn(n) + (n * (n + 1)) / 2 + (n + 1); }
    __device__ __forceinline__ int oV() const {
        if constexpr (kFar) return oVfar(n());
        else return oT() + (useT() ? n() * ldj() : 0);   // vector block
    }
    // kPair (the slim far N = 20 layout, round 15): the 2N-vectors that a lane reads by the pair
    // [2i], [2i+1] (e, xp, Phi, irn, the re-solve's 2N of scratch at Vb / Uf, Gamma's columns)
    // start on 16-byte offsets, so such a pair is one aligned 128-bit LDS read (ld_pair,
    // ntm_lanes.h).  The vector block starts at an odd double (the E block's N + 1 doubles of
    // ints), and the one vector of odd length in it, uu (N + 1), came after Uf: F .. Uf sat on
    // odd offsets, xp and what follows on even ones.  uu moves to the head of the block, in
    // front of rinfo; nothing is padded and nothing else moves.
    static constexpr bool kPair = kSlim && NN == 20;
    static constexpr int kUu = kPair ? 1 : 0;               // uu's n() + 1 doubles lead the block
    // kBox (the slim far N = 20 layout, round 16): the V-space box vlo / vhi is back in LDS, in
    // the 2N doubles of a11 / a21, at no cost in bytes.  Who owns those 2N doubles, and when:
    // the lift, from its coefficient pass (lift_phase writes a11 / a21 first thing) to the end
    // of its recursion, the only reader (the slim rollout recomputes its coefficients from
    // rho); the box from the scaling pass (diag_scale_phase writes vlo / vhi where D_l is
    // final) through the candidates, the dual path and GI, until the next QP's lift.  Nothing
    // carries them over a step boundary or a state hand-over: every QP writes both before it
    // reads either.  NTM_N20_BOX_LDS=0 builds the parent's form (bounds divided out of D on
    // every call of StructRows::check), for the A/B.
    static constexpr bool kBox = kPair && NTM_N20_BOX_LDS != 0;
    static constexpr int oPhin(int n) { return (kSlim ? kRL + kAB : 6) * n; }
    static constexpr int oEn(int n) { return (kSlim ? kRL + 2 + kAB : 12) * n; }
    static constexpr int oGtn(int n) { return (kSlim ? kRL + 4 + kAB : 14) * n; }
    static constexpr int oVecn(int n, int k) { return oVfar(n) + kUu * (n + 1) + (kRi + k) * n; }   // kFar: F = 0, .. Uf = 7
    static constexpr int oXpn(int n) { return oVfar(n) + (kRi + 9) * n + 1; }
    static constexpr int oIrnn(int n) { return oVfar(n) + (kRi + 13 + kUo) * n + 3; }
    static constexpr int oUn(int n) { return oVfar(n) + (kRi + 11) * n + 3; }
    static constexpr int oDrn(int n) { return oVfar(n) + (kRi + 12 + kUo) * n + 3; }
    static constexpr int gcoln(int n, int l) { return l * (2 * n - l + 1) - 2 * l; }   // gidx(2l, l) - 2l
    __device__ __forceinline__ double* rho() const {                                  // 3N (3xN col-major)
        if constexpr (kSF) return far + n() * ldj() + (n() + 1) * ldj() + 3 * n();
        else return base;
    }
    // (kSlim: no a11 / a21 / bb / Lam, Phi is 2N of scratch; never called there.  kBox: a11 /
    // a21 are the lift's from its coefficient pass to the end of its recursion, vlo / vhi's after)
    __device__ __forceinline__ double* a11() const { return base + 3 * n(); }         // n()
    __device__ __forceinline__ double* a21() const { return base + 4 * n(); }         // n()
    __device__ __forceinline__ double* bb() const { return base + 5 * n(); }          // n()
    __device__ __forceinline__ double* Phi() const { return base + oPhin(n()); }   // 4N Phi_i (2x2 col-major)
    __device__ __forceinline__ double* Lam() const { return base + 10 * n(); }        // 2N
    __device__ __forceinline__ double* e() const { return base + oEn(n()); }    // 2N free response
    // Gamma, block-lower-triangular and packed by column: column j holds rows 2j..2N-1
    __device__ __forceinline__ double* Gt() const { return base + oGtn(n()); }   // n()(n()+1)
    __device__ __forceinline__ int gidx(int r, int j) const { return j * (2 * n() - j + 1) + r - 2 * j; }
    __device__ __forceinline__ double& gt(int r, int j) const { return Gt()[gidx(r, j)]; }   // r >= 2j
    __device__ __forceinline__ double* J() const {                                   // n() x ldj() row-major
        if constexpr (kFar) return far;
        else return base + oJ();
    }
    // R: n() rows x (n()+1) columns col-major; the polish keeps its Schur complement
    // K in the strict upper triangle: K(a, c), a >= c, at R[c + (a+1) ldj()]
    __device__ __forceinline__ double* R() const {
        if constexpr (kFar) return far + n() * ldj();
        else return base + oR();
    }
    // T = R^{-1} of the GI factorisation (upper triangular, row-major n() x ldj();
    // zero outside the leading q x q block), so the dual direction is a matvec
    __device__ __forceinline__ double* T() const {
        if constexpr (kFar) return far;   // never dereferenced: far layouts keep no T (useT)
        else return base + oT();
    }
    // element (r, c) of J (and of T) at J()[r jr() + c jc()]: row-major
    __device__ __forceinline__ int jr() const { return ldj(); }
    __device__ __forceinline__ int jc() const { return 1; }
    // packed bordered KKT factor (rows 0..nt, row nt the right-hand side), entry
    // (r, c), c <= r, at J()[brow(r) + bcol(c, nt)]: row-major (row r at r(r+1)/2)
    __device__ __forceinline__ int brow(int r) const { return (r * (r + 1)) / 2; }
    __device__ __forceinline__ int bcol(int c, int /*nt*/) const { return c; }
    // echelon re-solve: sorted E (entry (t, u), u <= t, at Ep()[eidx(t, u)]) and the
    // GI's triangular factor R (and, before it, the scaled Gram G~ and its Cholesky
    // factor L): element (i, j) at R()[i + j ldj()], or, in the far layouts
    // (kGiLds), in the LDS E block, which is dead while GI runs (the echelon
    // re-solve's sorted E is rebuilt by every re-solve): the lower triangle row-major
    // packed (row i at i(i+1)/2, so G~ / L rows are contiguous), the upper triangle
    // column-major packed in the same slots ((i, j) and (j, i) share one: the lower
    // triangle is dead once R is being built, the factor below R's subdiagonal is
    // never touched), and R's superdiagonal (i, i+1) apart after the triangle, so
    // that a drop's upper-Hessenberg subdiagonal (i+1, i) does not collide with it.
    // N(N+1)/2 + N-1 doubles <= the E block's N(N+1)/2 + N+1.  GI's back and forward
    // substitutions, adds and drops then run on LDS instead of the HBM far block
    // (J stays there).  kGiLdsL: G~ and L; kGiLds: R
    static constexpr bool kGiLdsL = FAR;
    static constexpr bool kGiLds = FAR;
    __device__ __forceinline__ int gio(int i, int j) const {
        if (i >= j) return (i * (i + 1)) / 2 + j;
        if (i == j - 1) return (n() * (n() + 1)) / 2 + i;
        return (j * (j + 1)) / 2 + i;
    }
    __device__ __forceinline__ double& gr(int i, int j) const {
        if constexpr (kGiLds) return Ep()[gio(i, j)];
        else return R()[i + j * ldj()];
    }
    __device__ __forceinline__ double& grL(int i, int j) const {   // lower triangle, i >= j
        if constexpr (kGiLdsL) return Ep()[(i * (i + 1)) / 2 + j];
        else return R()[i + j * ldj()];
    }
    // row i of the lower triangle (elements (i, 0..i) at stride grs())
    __device__ __forceinline__ double* grow(int i) const {
        if constexpr (kGiLdsL) return Ep() + (i * (i + 1)) / 2;
        else return R() + i;
    }
    __device__ __forceinline__ int grs() const { return kGiLdsL ? 1 : ldj(); }
    // row permutation / column owner ints (2(N+1)); in the J/R block unless kFar
    __device__ __forceinline__ double* Ep() const {
        if constexpr (kFar) return base + oJ();
        else return J();
    }
    __device__ __forceinline__ int eidx(int t, int u) const {
        if constexpr (kFar) return (t * (t + 1)) / 2 + u;
        else return t * ldj() + u;
    }
    __device__ __forceinline__ int* permi() const {
        if constexpr (kFar) return reinterpret_cast<int*>(base + oJ() + (n() * (n() + 1)) / 2);
        else return reinterpret_cast<int*>(R());
    }
    // 2N ints (in 2N doubles of space): per state row r, (last column j with
    // Gamma_rj != 0) + 1, plus kRowMulti if it has two or more non-zeros
    __device__ __forceinline__ int* rinfo() const { return reinterpret_cast<int*>(base + oV() + kUu * (n() + 1)); }
    // N-vector k of the block (F = 0 .. Uf = 7): kPair's come from the constexpr offsets the asserts check
    __device__ __forceinline__ int vec(int k) const {
        if constexpr (kPair) return oVecn(n(), k);
        else return oV() + (kRi + k) * n();
    }
    __device__ __forceinline__ double* F() const { return base + vec(0); }         // n()  F~
    __device__ __forceinline__ double* D() const { return base + vec(1); }   // n()  Jacobi scaling
    __device__ __forceinline__ double* V() const { return base + vec(2); }   // n()  scaled variables
    __device__ __forceinline__ double* d() const { return base + vec(3); }   // n()
    __device__ __forceinline__ double* np() const { return base + vec(4); }  // n()  GI normal
    __device__ __forceinline__ double* hv() const { return base + vec(5); }  // n()  Householder / polish
    __device__ __forceinline__ double* Vb() const { return base + vec(6); }  // n()  polish fixed (V)
    __device__ __forceinline__ double* Uf() const { return base + vec(7); }  // n()  polish fixed (U)
    __device__ __forceinline__ double* uu() const { return base + oV() + (kPair ? 0 : (kRi + 8) * n()); }  // n()+1 multipliers
    __device__ __forceinline__ double* xp() const { return base + (kPair ? oXpn(n()) : oV() + (kRi + 9) * n() + 1); }    // 2(n()+1) rollout
    __device__ __forceinline__ double* U() const { return base + (kPair ? oUn(n()) : oV() + (kRi + 11) * n() + 3); }    // n()
    __device__ __forceinline__ double* Uold() const {                                              // n()
        if constexpr (kSF) return rho() + 3 * n();
        else return base + oV() + (kRi + 12) * n() + 3;
    }
    __device__ __forceinline__ double* dr() const { return base + (kPair ? oDrn(n()) : oV() + (kRi + 12 + kUo) * n() + 3); }    // N: d masked to b < q (GI)
    __device__ __forceinline__ double* irn() const { return base + (kPair ? oIrnn(n()) : oV() + (kRi + 13 + kUo) * n() + 3); }   // 2N: 1/rn_r (0: const row)
    __device__ __forceinline__ double* ssg() const { return base + oV() + (kRi + 15 + kUo) * n() + 3; }   // N: sign of general row s
    // per-QP constants hoisted out of the solver loops (kSlim without kBox: recomputed from D;
    // kBox: in a11 / a21's 2N doubles, which are dead once the lift's recursion has run)
    __device__ __forceinline__ double* vlo() const {                                                 // N: umin/D_j
        if constexpr (kBox) return a11();
        else return base + oV() + (kRi + 17) * n() + 3;
    }
    __device__ __forceinline__ double* vhi() const {                                                 // N: umax/D_j
        if constexpr (kBox) return a21();
        else return base + oV() + (kRi + 18) * n() + 3;
    }
    // 1/L(k,k) (Cholesky), 1/K(k,k) (Schur), contiguous; 1/|D (e_i - e_{i-1})|: in the far block when kSlim
    __device__ __forceinline__ double* ldi() const {
        if constexpr (kSlim) return far + n() * ldj() + (n() + 1) * ldj();
        else return base + oV() + (kRi + 19) * n() + 3;
    }
    __device__ __forceinline__ double* kdi() const { return ldi() + n(); }
    __device__ __forceinline__ double* idun() const {
        if constexpr (kSlim) return ldi() + 2 * n();
        else return base + oV() + (kRi + 21) * n() + 3;
    }
    static constexpr int kVec = kSlim ? 17 + kUo : 24;        // N-vectors of the block (+ 3 + 3 scn)
    // this scenario's C1, B.m gain and w_dep (scenario generator; read only when pb.g.phys_on)
    __device__ __forceinline__ double* scn() const { return base + oV() + kVec * n() + 3; }
    __device__ __forceinline__ int* act() const { return reinterpret_cast<int*>(base + oV() + kVec * n() + 6); }
    __device__ __forceinline__ int* sidx() const { return act() + n() + 1; }
    static constexpr int kCL = kSF ? 0 : 2;                  // the carried sets' (N+1)-int tables in LDS
    __device__ __forceinline__ int* cand() const {                                   // 2(n()+1): last two active sets
        if constexpr (kSF) return reinterpret_cast<int*>(Uold() + n());
        else return act() + 2 * (n() + 1);
    }
    __device__ __forceinline__ int* fidx() const { return act() + (2 + kCL) * (n() + 1); }   // n()+1: free variables (polish)
    __device__ __forceinline__ int* srw() const { return act() + (3 + kCL) * (n() + 1); }    // n()+1: state row of general row s
    __device__ __forceinline__ unsigned char* fx() const {
        return reinterpret_cast<unsigned char*>(act() + (4 + kCL) * (n() + 1));
    }
    __device__ __forceinline__ unsigned char* aflag() const { return fx() + n(); }
};

// Input-rate rows (NTM_MODE_FULL_DU) in this kernel's code.  The host never launches
// mode 3 on the slim N = 20 far kernels (it takes the runtime-N kernels, and the layout
// has no active-row flags for rate rows: slim_ab), but `mode` is a launch value, so the
// compiler kept every rate arm and restored du wherever one stood.  A unit that sets
// NTM_N20_NO_RATE compiles those kernels without them (StructRows::decode<false>, the
// `rate_rows<W>() &&` tests of the row provider and polish_compact, rate_mode in ntm_gram.h);
// the launchers of ntm_step.h refuse mode 3 for such a build.
template <class W>
__host__ __device__ constexpr bool rate_rows() { return !(NTM_N20_NO_RATE && W::kAB != 0); }

__host__ __device__ constexpr int ldj_of(int N) { return N | 1; }
// the J/R block of a far layout, in HBM per scenario (no T: WS::useT)
__host__ __device__ constexpr int far_doubles(int N) {
    // + ldi, kdi, idun (slim); + rho, U_old and the carried sets' 2(N+1) ints (slim_far)
    return N * ldj_of(N) + (N + 1) * ldj_of(N) + (ws_slim(N, true) ? 3 * N : 0) +
           (slim_far(N, true) ? 4 * N + (N + 1) : 0);
}
__host__ __device__ constexpr int ws_doubles(int N, bool far = false) {
    // LDS: the E block (far), or J, R and (N <= kMaxNT) T
    const int jr = far ? (N * (N + 1)) / 2 + (N + 1) : (N <= kMaxNT ? 2 : 1) * N * ldj_of(N) + (N + 1) * ldj_of(N);
    const int rl = slim_far(N, far) ? 0 : 3, uo = slim_far(N, far) ? 0 : 1;
    return ws_slim(N, far) ? (rl + 4 + slim_ab(N, far)) * N + N * (N + 1) + jr + (17 + uo) * N + 6
                           : 14 * N + N * (N + 1) + jr + 24 * N + 6;
}
// workspace bytes with room for `rows` active-row flags: the structured rows of
// the MPC step are at most 8N+2 (getWLc 6N+4 plus 2(N-1) rate rows); a dense
// quadprog problem (k_qp) may carry more
__host__ __device__ constexpr int ws_bytes_rows(int N, int rows, bool far = false) {
    const int fmin = slim_ab(N, far) ? 6 * N + 4 : 8 * N + 4;      // (slim_ab: no rate rows)
    const int flags = rows > fmin ? rows : fmin;
    int b = ws_doubles(N, far) * 8 + (slim_far(N, far) ? 4 : 6) * (N + 1) * 4 + N + flags;   // ..., fx (N), aflag
    return (b + 15) & ~15;
}
__host__ __device__ constexpr int ws_bytes(int N, bool far = false) {
    return ws_bytes_rows(N, slim_ab(N, far) ? 6 * N + 4 : 8 * N + 4, far);
}
static_assert(16 * ws_bytes(20, true) <= 160 * 1024, "slim N = 20: 16 scenarios per CU");
// kPair: every vector that ld_pair reads starts on an even double (16 bytes; the workspace
// itself is a multiple of 16 bytes from a 16-byte aligned base), and so does every column of
// the packed Gamma: column l starts l (2N - 1 - l) doubles into Gt, and one of l, 2N - 1 - l is even
template <class W>
constexpr bool ws_pair_columns_even() {
    for (int l = 0; l < 20; ++l)
        if ((W::oGtn(20) + W::gcoln(20, l)) % 2 != 0) return false;
    return true;
}
template <class W>
constexpr bool ws_pair_aligned() {
    static_assert(W::kPair, "the slim far N = 20 layout");
    static_assert(ws_bytes(20, true) % 16 == 0, "a scenario's workspace keeps the next one 16-byte aligned");
    static_assert(W::oPhin(20) % 2 == 0, "Phi (the re-solve's 2N of scratch) on a 16-byte offset");
    static_assert(W::oEn(20) % 2 == 0, "e on a 16-byte offset");
    static_assert(W::oGtn(20) % 2 == 0, "Gt on a 16-byte offset");
    static_assert(ws_pair_columns_even<W>(), "every packed Gamma column on a 16-byte offset");
    static_assert(W::oVecn(20, 6) % 2 == 0, "Vb (with Uf the plane search's 2N of scratch) on a 16-byte offset");
    static_assert(W::oVecn(20, 7) == W::oVecn(20, 6) + 20, "Uf follows Vb");
    static_assert(W::oVecn(20, 7) + 20 == W::oXpn(20), "xp follows Uf: uu moved, nothing padded");
    static_assert(W::oXpn(20) % 2 == 0, "xp on a 16-byte offset");
    static_assert(W::oIrnn(20) % 2 == 0, "irn on a 16-byte offset");
    // the N-vectors read in chunks of five consecutive entries (ld5): the row dots' U, d, dr and
    // the lift's a11 / a21 (at 3N and 4N doubles, WS::a11 / a21)
    static_assert(W::oUn(20) % 2 == 0 && W::oDrn(20) % 2 == 0 && W::oVecn(20, 3) % 2 == 0, "U, dr, d on 16-byte offsets");
    static_assert(W::kAB == 2 && (3 * 20) % 2 == 0 && (4 * 20) % 2 == 0, "a11, a21 on 16-byte offsets");
    // kBox: vlo / vhi are N doubles each, as a11 / a21 are (a21 starts N doubles behind a11, Phi
    // N doubles behind a21), and they cost no LDS: one more 512-byte granule would cost the 16th wave
    static_assert(W::oPhin(20) == 5 * 20 && W::kAB * 20 == 2 * 20, "a11 / a21 hold vlo / vhi: N doubles each, in front of Phi");
    static_assert(ws_bytes(20, true) == 10224, "slim N = 20: the workspace's size is unchanged");
    return true;
}
static_assert(ws_pair_aligned<WS<20, false, true>>() && ws_pair_aligned<WS<20, true, true>>(), "slim N = 20: aligned pairs");
static_assert(4 * ws_bytes(50, true) <= 160 * 1024, "slim N = 50: 4 scenarios per CU");

// s: the scenario's index in the launch (its far block, when the WS has one)
template <int NN, bool GEN = false, bool FAR = ws_far(NN)>
__device__ inline WS<NN, GEN, FAR> ws_carve(char* base, int N, const Prob* pb = nullptr, int64_t s = 0) {
    WS<NN, GEN, FAR> w;
    w.N_rt = N;
    w.base = reinterpret_cast<double*>(base);
    w.far = nullptr;
    if constexpr (FAR) w.far = pb->far + s * (int64_t)far_doubles(N);
    return w;
}

// The scenario's LPV coefficients: the launch constants, with C1, the B.m gain and
// w_dep taken from the workspace when the scenario generator varies the plasma
// (written once per launch by scn_store).  Keeping the launch constants in the
// kernel arguments matters: a copy of the whole Prob per scenario cost the N=20
// step kernel 100 B of scratch per lane and 20 more spilled SGPRs.
// The input weight R_u: its term 2 Ru I of the Hessian enters the
// Gram diagonal (scaling, GI's full G~, the re-solve's G~_FF), the echelon k = 1 line
// search and the certificate's gradient.  Compiled into the generic kernels only
// (ru_on): the specialised N = 10 / 20 / 50 kernels keep their register allocation,
// and the host dispatches a launch with Ru != 0 to the generic ones (as D4 / D6)
template <class W>
__device__ __forceinline__ constexpr bool ru_on() { return W::kNN == 0; }
template <class W>
__device__ __forceinline__ double ru_of(const Prob& pb) {
    if constexpr (ru_on<W>()) return pb.Ru;
    else return 0.0;
}
// The reference's stage weight is Q = I (NTM_MPC_Sim.m:59, Omega = blkdiag(Q, ...)).
// The specialised kernels (compile-time horizons) assume it, so their Om products
// are the identity (bit for bit what 1 x + 0 y gives for finite data) and the
// weight's four launch constants leave their scalar registers; a launch with any
// other Q runs on the generic kernels (host dispatch, like Ru and D4 / D6).
#ifndef NTM_QI_MAXN
#define NTM_QI_MAXN 32     // compile-time horizons up to this one assume Q = I (qi_on): N = 10, 20 (at
                           // N = 50 it cost 11% through register allocation, A/B on one box)
#endif
template <class W>
__device__ __forceinline__ constexpr bool qi_on() { return W::kNN > 0 && NTM_QI_MAXN >= W::kNN; }
template <bool QI>
struct OmQ {                       // x -> Q x for one stage's 2-vector
    double q00, q01, q10, q11;
    __device__ __forceinline__ explicit OmQ(const double* Q) {
        if constexpr (QI) { q00 = 1.0; q01 = 0.0; q10 = 0.0; q11 = 1.0; }
        else { q00 = Q[0]; q01 = Q[1]; q10 = Q[2]; q11 = Q[3]; }
    }
    __device__ __forceinline__ double o0(double x0, double x1) const {
        if constexpr (QI) return x0;
        else return q00 * x0 + q01 * x1;
    }
    __device__ __forceinline__ double o1(double x0, double x1) const {
        if constexpr (QI) return x1;
        else return q10 * x0 + q11 * x1;
    }
};
__device__ __forceinline__ bool gen_phys(const Prob& pb) { return pb.g.phys_on != 0; }
__device__ __forceinline__ bool gen_dist(const Prob& pb) { return pb.g.dist_on != 0; }
template <class W>
__device__ __forceinline__ Coef scn_coef(const Prob& pb, const W& w) {
    Coef k = pb.k;
    if (W::kGen && gen_phys(pb)) {
        k.C1 = w.scn()[0];
        k.bc = w.scn()[1];
        k.wdep = w.scn()[2];
    }
    return k;
}
template <class W>
__device__ __forceinline__ void scn_store(const Prob& pb, const W& w, int64_t gid, int l) {
    if (W::kGen && gen_phys(pb) && l == 0) {
        Prob q = pb;
        gen_apply_physics(q, gid);
        w.scn()[0] = q.k.C1;
        w.scn()[1] = q.k.bc;
        w.scn()[2] = q.k.wdep;
    }
}

// The observer kernels' workspace (k_mpc_step_obs / k_mpc_run_obs, ntm_step.h): the
// runtime-N generator layout, plus the controller's model in lanes.  There the model is
// no longer the plant: it may be the nominal plasma while the plant is the scenario's
// (ntm_observer.nominal_model), and its offset C carries the disturbance estimate
// (C + d_hat), so it needs a per-scenario C2 besides scn()'s three values.  Every lane of
// a scenario's group holds the same four values (at P < 64 a wave runs several scenarios,
// so they are vector registers); the LDS layout is WS<0, true, false>'s, untouched.
// The lift and the rollout read their coefficients through scn_coef(pb, w) alone, so the
// overload below is all it takes to run them on this model; every other workspace type
// keeps the template above, and with it the code it had.
struct WSObs : WS<0, true, false> {
    double mC1, mC2, mbc, mwdep;
};
__device__ __forceinline__ Coef scn_coef(const Prob& pb, const WSObs& w) {
    Coef k = pb.k;
    k.C1 = w.mC1;
    k.C2 = w.mC2;
    k.bc = w.mbc;
    k.wdep = w.mwdep;
    return k;
}
// scenario gid's plant: the generator's plasma when a spread is attached (scn_store's
// values: the same function on the same inputs), else the launch's
__device__ __forceinline__ Coef plant_coef(const Prob& pb, int64_t gid) {
    Coef k = pb.k;
    if (gen_phys(pb)) {
        Prob q = pb;
        gen_apply_physics(q, gid);
        k.C1 = q.k.C1;
        k.bc = q.k.bc;
        k.wdep = q.k.wdep;
    }
    return k;
}
// d_hat <- d_hat + gain (e - d_hat), as one fused multiply-add of the rounded difference
// (include/ntm_mpc.h states it; fixed here so every implementation agrees bit for bit);
// a component whose innovation is not finite keeps its estimate
__device__ __forceinline__ double obs_update(double gain, double e, double d) {
    return isfinite(e) ? fma(gain, e - d, d) : d;
}

// Output feedback (k_mpc_step_est / k_mpc_run_est, ntm_step.h): ntm_estimator as the
// kernels take it, one by-value argument.  sy = the measurement noise's standard
// deviations; the samples are the generator's normal channels 2 and 3 at the plant
// step's (seed, global id, time index)
struct EstOpt {
    int nominal, pad;
    double gain[2], kappa[2], sy[2];
};
// y = x_next + sy n(gid, kt, 2 + i); a zero sy skips the draw, as plant_step skips a zero sigma
__device__ __forceinline__ double est_measure(const Prob& pb, double sy, double xn, int64_t gid, int kt, uint32_t ch) {
    return sy != 0.0 ? xn + sy * gen_normal(pb.g.seed, gid, (uint32_t)kt, ch) : xn;
}
// One component of the estimator's update from the measurement y and the model's one-step
// prediction m (without d_hat): r = y - m, iota = r - d_hat (the old one);
// d_hat <- obs_update(gain, r, d_hat); x_hat <- fma(-kappa, iota, y), one rounding
// (= (1 - kappa) y + kappa (m + d_hat)), and y itself where iota is not finite
__device__ __forceinline__ void est_update(double gain, double kappa, double y, double m, double& d, double& xh) {
    const double r = y - m, iota = r - d;
    d = obs_update(gain, r, d);
    xh = isfinite(iota) ? fma(-kappa, iota, y) : y;
}

}  // namespace ntm
