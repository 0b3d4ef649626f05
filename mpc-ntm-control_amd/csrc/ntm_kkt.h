// ntm_kkt.h — the KKT audit: the optimality conditions of min 1/2 U'GU + F'U s.t.
// Lin U <= b measured from (U, lambda) alone (ntm_qp_kkt_device).
//
// Deliberately plain arithmetic: straight loops over rows and variables striped
// over the group's lanes, and the group maxima of ntm_collectives.h.  None of the
// solver's helpers (the masked dots of ntm_lanes.h, the row providers' check, the
// polishers) appear here: the audit exists to be independent of them.
//
// Per scenario, with d_j = 1/sqrt(G_jj) (1 where G_jj <= 0), V = U/d,
// vmax = max(1, max|V|), rn_i = |Lin_i o d|_2 (1 for a constant row, rn_i = 0),
// mu_i = lambda_i rn_i and mumax = max(1, max|mu|):
//   kkt[0] stationarity     max_j |(GU + F + Lin'lambda)_j d_j| / max(1, max_j |F_j d_j|)
//   kkt[1] primal           max(0, max_i v_i), v_i = (Lin_i U - b_i)/(rn_i vmax), constant rows -b_i
//   kkt[2] dual             max(0, max_i -mu_i) / mumax
//   kkt[3] complementarity  max_i |mu_i (Lin_i U - b_i)/rn_i| / (mumax vmax), ordinary rows
// the units of the solver's own certificate.  m = 0: only kkt[0] is non-zero.  Any
// non-finite term makes all four NaN for that scenario.
//
// ntm_mpc_kkt_device audits an MPC step's own QP without materialising it: the
// kernel lifts rho_qp (lift_phase, the one piece shared with the step), and reads
// every row's Lin_i U, b_i and rn_i off Gamma, e = Phi x_k + Lambda and the bounds,
// G_jj, F and the gradient 2 Gamma' Om (e + Gamma U - R) + 2 Ru U off the same.
// Row order (the oracle's constraints(), the ids of active_ws):
//   mode 1: rows 0..N-1 are -U_j <= -umin, rows N..2N-1 are U_j <= umax;
//   modes 2, 3: getWLc's 6N+4 rows: per stage i = 0..N-1 the block
//     [-U_i <= -umin; U_i <= umax; -x_i <= -xmin (2 rows); x_i <= xmax (2 rows)]
//     (the x_0 rows are constant), then [-x_N <= -xmin; x_N <= xmax];
//   mode 3 then adds, for i = 1..N-1, row 6N+4 + 2(i-1): U_i - U_{i-1} <= du_max and
//     row 6N+4 + 2(i-1) + 1: U_{i-1} - U_i <= du_max.
#pragma once
#include <hip/hip_runtime.h>

#include "ntm_base.h"
#include "ntm_collectives.h"
#include "ntm_lift.h"
#include "ntm_ws.h"

namespace ntm {

constexpr int kKktMaxN = 64;   // NTM_MAX_N

// One group of P lanes per scenario (P = 16, 32, 64 as the solver's kernels).
// G (N x N), Lin (m x N) column-major per scenario, scenario-major batches.
template <int P>
__global__ __launch_bounds__(64) void k_qp_kkt(int64_t B, int N, int m, const double* G, const double* F,
                                               const double* Lin, const double* b, const double* U,
                                               const double* lambda, double* kkt) {
    __shared__ double sh[(64 / P) * 2 * kKktMaxN];
    const int g = threadIdx.x / P, l = threadIdx.x % P;
    const int64_t s = (int64_t)blockIdx.x * (64 / P) + g;
    if (s >= B) return;
    double* d = sh + g * (2 * kKktMaxN);
    double* Us = d + kKktMaxN;
    G += s * ((int64_t)N * N);
    F += s * N;
    U += s * N;
    Lin += s * ((int64_t)m * N);
    b += s * m;
    lambda += s * m;
    bool bad = false;
    double vm = 0.0, fm = 0.0;
    for (int j = l; j < N; j += P) {
        const double gjj = G[j + (int64_t)j * N];
        const double dj = (gjj > 0.0) ? 1.0 / sqrt(gjj) : 1.0;
        const double uj = U[j];
        const double v = uj / dj, f = F[j] * dj;
        bad = bad || !isfinite(v) || !isfinite(f);
        vm = fmax(vm, fabs(v));
        fm = fmax(fm, fabs(f));
        d[j] = dj;
        Us[j] = uj;
    }
    NTM_WSYNC();
    const double vmax = fmax(1.0, gmax<P>(vm));
    const double fmx = fmax(1.0, gmax<P>(fm));
    // rows: primal, dual and complementarity terms
    double prim = 0.0, mum = 0.0, dneg = 0.0, comp = 0.0;
    for (int i = l; i < m; i += P) {
        double lu = 0.0, ss = 0.0;
        for (int j = 0; j < N; ++j) {
            const double a = Lin[i + (int64_t)j * m];
            const double t = a * d[j];
            lu += a * Us[j];
            ss += t * t;
        }
        const double r = lu - b[i];
        const bool cst = !(ss > 0.0);
        const double rn = cst ? 1.0 : sqrt(ss);
        const double v = cst ? -b[i] : r / (rn * vmax);
        const double mu = lambda[i] * rn;
        const double c = cst ? 0.0 : fabs(mu * (r / rn));
        bad = bad || !isfinite(ss) || !isfinite(v) || !isfinite(mu) || !isfinite(c);
        prim = fmax(prim, v);
        mum = fmax(mum, fabs(mu));
        dneg = fmax(dneg, -mu);
        comp = fmax(comp, c);
    }
    const double mumax = fmax(1.0, gmax<P>(mum));
    prim = gmax<P>(prim);
    dneg = gmax<P>(dneg);
    comp = gmax<P>(comp);
    // variables: the gradient of the Lagrangian (rows with lambda_i = 0 add nothing)
    double stat = 0.0;
    for (int j = l; j < N; j += P) {
        double gj = F[j];
        for (int k = 0; k < N; ++k) gj += G[j + (int64_t)k * N] * Us[k];
        for (int i = 0; i < m; ++i) {
            const double li = lambda[i];
            if (li != 0.0) gj += Lin[i + (int64_t)j * m] * li;
        }
        const double t = gj * d[j];
        bad = bad || !isfinite(t);
        stat = fmax(stat, fabs(t));
    }
    stat = gmax<P>(stat);
    const bool nan = gany<P>(bad);
    if (l < 4) {
        double out = l == 0 ? stat / fmx : (l == 1 ? prim : (l == 2 ? dneg / mumax : comp / (mumax * vmax)));
        if (m == 0 && l > 0) out = 0.0;
        kkt[s * 4 + l] = nan ? __builtin_nan("") : out;
    }
}


// The step's own QP (ntm_mpc_kkt_device).  Workspace: a WS carved as the function-level
// kernels carve it (runtime horizon: NN = 0, the form their launch macro instantiates);
// the audit's own vectors live in arrays the lift leaves free.
template <int P, int NN = 0>
__global__ __launch_bounds__(64) void k_mpc_kkt(Prob pb, int64_t B, const double* x_k, const double* rho_qp,
                                                const double* U, const double* lambda, double* kkt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int g = threadIdx.x / P, l = threadIdx.x % P;
    const int64_t s = (int64_t)blockIdx.x * (64 / P) + g;
    const int N = pb.N;
    if (s >= B) return;
    auto w = ws_carve<0>(smem + g * ws_bytes(N), N);
    const int mode = pb.mode;
    const int m = mode == NTM_MODE_NONE ? 0 : (mode == NTM_MODE_BOX ? 2 * N : (mode == NTM_MODE_FULL_DU ? 8 * N + 2 : 6 * N + 4));
    const bool state = mode >= NTM_MODE_FULL, rate = mode == NTM_MODE_FULL_DU;
    const int nb = mode == NTM_MODE_BOX ? 1 : 6;       // bound rows of U_j: nb j (lower), + N or + 1 (upper)
    const int ub = mode == NTM_MODE_BOX ? N : 1;
    const int r0 = 6 * N + 4;                          // first rate row
    const double* lam = lambda + s * m;
    const double xk0 = x_k[2 * s], xk1 = x_k[2 * s + 1];
    for (int e = l; e < 3 * N; e += P) w.rho()[e] = rho_qp[s * (3 * N) + e];
    NTM_WSYNC();
    lift_phase<P>(pb, w, l);
    double* const e = w.e();        // 2N: free response Phi x_k + Lambda
    double* const y = w.xp();       // 2N: e + Gamma U
    double* const z = w.irn();      // 2N: state row r's upper minus lower multiplier
    double* const Us = w.U();       // N
    double* const d = w.D();        // N
    double* const gr = w.F();       // N: gradient of the cost
    for (int i = l; i < N; i += P) {
        const double* Ph = w.Phi() + 4 * i;
        e[2 * i] = (Ph[0] * xk0 + Ph[2] * xk1) + w.Lam()[2 * i];
        e[2 * i + 1] = (Ph[1] * xk0 + Ph[3] * xk1) + w.Lam()[2 * i + 1];
        Us[i] = U[s * N + i];
    }
    NTM_WSYNC();
    for (int r = l; r < 2 * N; r += P) {
        double gu = 0.0;
        for (int j = 0; j <= (r >> 1); ++j) gu += w.gt(r, j) * Us[j];
        y[r] = e[r] + gu;
        double zr = 0.0;
        if (state) {
            const int i = (r >> 1) + 1, c = r & 1;
            const int idmin = (i < N) ? 6 * i + 2 + c : 6 * N + c;
            zr = lam[idmin + 2] - lam[idmin];
        }
        z[r] = zr;
    }
    NTM_WSYNC();
    bool bad = false;
    double vm = 0.0, fm = 0.0;
    const double q00 = pb.Q[0], q01 = pb.Q[1], q10 = pb.Q[2], q11 = pb.Q[3];
    for (int j = l; j < N; j += P) {
        double gjj = 0.0, fj = 0.0, gj = 0.0;
        for (int i = j; i < N; ++i) {
            const double g0 = w.gt(2 * i, j), g1 = w.gt(2 * i + 1, j);
            gjj += g0 * (q00 * g0 + q01 * g1) + g1 * (q10 * g0 + q11 * g1);
            const double f0 = e[2 * i] - pb.r[0], f1 = e[2 * i + 1] - pb.r[1];
            fj += g0 * (q00 * f0 + q01 * f1) + g1 * (q10 * f0 + q11 * f1);
            const double y0 = y[2 * i] - pb.r[0], y1 = y[2 * i + 1] - pb.r[1];
            gj += g0 * (q00 * y0 + q01 * y1) + g1 * (q10 * y0 + q11 * y1);
        }
        gjj = 2.0 * gjj + 2.0 * pb.Ru;
        const double dj = (gjj > 0.0) ? 1.0 / sqrt(gjj) : 1.0;
        const double v = Us[j] / dj, f = (2.0 * fj) * dj;
        bad = bad || !isfinite(v) || !isfinite(f);
        vm = fmax(vm, fabs(v));
        fm = fmax(fm, fabs(f));
        d[j] = dj;
        gr[j] = 2.0 * gj + 2.0 * pb.Ru * Us[j];
    }
    NTM_WSYNC();
    const double vmax = fmax(1.0, gmax<P>(vm));
    const double fmx = fmax(1.0, gmax<P>(fm));
    double prim = 0.0, mum = 0.0, dneg = 0.0, comp = 0.0;
    for (int id = l; id < m; id += P) {
        double res, ss, bi = 0.0;      // res = Lin_i U - b_i, ss = rn_i^2, bi: b_i of a constant row
        if (rate && id >= r0) {
            const int t = id - r0, j = (t >> 1) + 1;
            const double sg = (t & 1) ? -1.0 : 1.0;
            res = sg * (Us[j] - Us[j - 1]) - pb.du;
            ss = d[j] * d[j] + d[j - 1] * d[j - 1];
        } else {
            const int blk = mode == NTM_MODE_BOX ? (id < N ? id : id - N) : id / 6;
            const int rr = mode == NTM_MODE_BOX ? (id < N ? 0 : 1) : id - 6 * blk;
            if (blk < N && rr < 2) {
                res = rr == 0 ? pb.umin - Us[blk] : Us[blk] - pb.umax;
                ss = d[blk] * d[blk];
            } else {
                int i, c;
                bool upper;
                if (blk < N) { i = blk; c = (rr - 2) & 1; upper = rr >= 4; }
                else { i = N; c = rr & 1; upper = rr >= 2; }
                const double xi = i == 0 ? (c ? xk1 : xk0) : y[2 * (i - 1) + c];
                res = upper ? xi - pb.xmax[c] : pb.xmin[c] - xi;
                ss = 0.0;
                if (i > 0) {
                    const int r = 2 * (i - 1) + c;
                    for (int j = 0; j < i; ++j) { const double t = w.gt(r, j) * d[j]; ss += t * t; }
                    // a constant row's b_i: Lin_i = 0, so Lin_i U - b_i is -b_i with U's part zero
                    const double ei = e[r];
                    bi = upper ? pb.xmax[c] - ei : ei - pb.xmin[c];
                } else {
                    bi = -res;
                }
            }
        }
        const bool cst = !(ss > 0.0);
        const double rn = cst ? 1.0 : sqrt(ss);
        const double v = cst ? -bi : res / (rn * vmax);
        const double mu = lam[id] * rn;
        const double c = cst ? 0.0 : fabs(mu * (res / rn));
        bad = bad || !isfinite(ss) || !isfinite(v) || !isfinite(mu) || !isfinite(c);
        prim = fmax(prim, v);
        mum = fmax(mum, fabs(mu));
        dneg = fmax(dneg, -mu);
        comp = fmax(comp, c);
    }
    const double mumax = fmax(1.0, gmax<P>(mum));
    prim = gmax<P>(prim);
    dneg = gmax<P>(dneg);
    comp = gmax<P>(comp);
    double stat = 0.0;
    for (int j = l; j < N; j += P) {
        double lt = 0.0;                                 // (Lin' lambda)_j
        if (m > 0) lt = lam[nb * j + ub] - lam[nb * j];
        if (state)
            for (int r = 2 * j; r < 2 * N; ++r) lt += w.gt(r, j) * z[r];
        if (rate) {
            if (j >= 1) lt += lam[r0 + 2 * (j - 1)] - lam[r0 + 2 * (j - 1) + 1];
            if (j + 1 < N) lt -= lam[r0 + 2 * j] - lam[r0 + 2 * j + 1];
        }
        const double t = (gr[j] + lt) * d[j];
        bad = bad || !isfinite(t);
        stat = fmax(stat, fabs(t));
    }
    stat = gmax<P>(stat);
    const bool nan = gany<P>(bad);
    if (l < 4) {
        double out = l == 0 ? stat / fmx : (l == 1 ? prim : (l == 2 ? dneg / mumax : comp / (mumax * vmax)));
        if (m == 0 && l > 0) out = 0.0;
        kkt[s * 4 + l] = nan ? __builtin_nan("") : out;
    }
}

}  // namespace ntm
