// Stand-alone check of the lane-masked triangular substitutions of csrc/ntm_lanes.h
// (fsub_lanes / bsub_lanes, the echelon re-solve of the slim far N = 20 kernels)
// against the loop form they replace, bit for bit.  One 64-lane block per case.
//
//   hipcc --offload-arch=gfx950 -O3 -o echelon_sub_check tools/echelon_sub_check.hip
//   ./echelon_sub_check       -> one PASS / FAIL line, exit status 1 on a mismatch
//
// The loop form lives here (ref_forward / ref_backward: polish_compact's loops as
// they stand for the other kernels, the contraction spelled out as the production
// build compiled it: the product sq_id acc, then fma(-E, x_t, acc)).  It runs
// with all 64 lanes on; the helpers run under the case's entry EXEC.
//   Cases: every n = 0..20; forward with nc = -1 (one right-hand side) and every
// nc = 0..n (two: -e_c is zero on the rows above the non-pivot column); a random
// finite lower-triangular E with exact zeros among its off-diagonal entries;
// accumulators and right-hand sides of -0.0; an infinity and a NaN in h, in an
// off-diagonal entry and in a diagonal reciprocal; the gradient of the backward
// solve the same.  Entry EXEC: all 64 lanes (the kernel's), the lanes <= 20, and an
// irregular subset.  The packed E sits in LDS between guard words, and the words
// past row n - 1 (past the triangle) and the guards hold a signalling NaN.
//   Compared: x, zz and mu bit for bit on every lane < n that entered and whose chain
// only takes values from lanes that entered (forward: the lanes below it; backward:
// the lanes above it, below n), which is every lane < n under the first two entry
// patterns; the `ok` flag (any non-finite x or zz on a lane < n) under those two; a
// lane that is off on entry or >= n keeps the sentinel it held; every lane that
// entered writes a sentinel behind the helpers (EXEC restored); LDS afterwards is
// the image that was put there, poison included, and no poison reached a result.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define NTM_CH 5                               // the far N = 20 unit's chunk (csrc/ntm_n20.hip)
#include "../mpc-ntm-control_amd/csrc/ntm_lanes.h"
#include "../mpc-ntm-control_amd/csrc/ntm_ws.h"
#include "check_common.h"

using W20 = ntm::WS<20, false, true>;
constexpr int kN = 20, kTri = kN * (kN + 1) / 2;
constexpr int kGuard = 32, kImg = kGuard + kTri + kGuard;   // guard, the packed triangle, guard
constexpr uint64_t kPoison = 0x7FF4000000000BADull;         // a signalling NaN
static_assert(ntm::esub_lanes_ok<64, 5, W20>(), "the slim far N = 20 workspace must take the masked substitutions");
static_assert(!ntm::esub_lanes_ok<64, 4, W20>() && !ntm::esub_lanes_ok<32, 5, W20>() &&
                  !ntm::esub_lanes_ok<64, 5, ntm::WS<20, false, false>>() &&
                  !ntm::esub_lanes_ok<64, 5, ntm::WS<50, false, true>>() && !ntm::esub_lanes_ok<64, 5, ntm::WS<0>>(),
              "no other kernel may reach the masked substitutions");

struct Case {
    int n, nc;
    unsigned long long entry;
    double img[kImg];                          // LDS image
    double sq[64], h[64], z[64], g[64];        // 1 / E[l][l]; the right-hand sides; the backward one
    // results: the loop form (r*) and the helpers (m*)
    double rx[64], rz[64], rmu[64], mx[64], mz[64], mmu[64];
    double after[kImg];
    unsigned sent[64];
    int rok, mok;
};

__device__ __forceinline__ int eidx(int t, int u) { return (t * (t + 1)) / 2 + u; }
__device__ __forceinline__ double sentinel(int lane, int which) { return 1.0e6 * (which + 1) + lane; }
static double h_sentinel(int lane, int which) { return 1.0e6 * (which + 1) + lane; }

// polish_compact's forward substitution, the loop form (one element loaded a step ahead)
__device__ __forceinline__ void ref_forward(const double* Ep, int n, int nc, int l, double acc, double acz, double sq_id,
                                            double& x, double& zz) {
#pragma clang fp contract(off)
    double eq = (0 < n && l > 0 && l < n) ? Ep[eidx(l, 0)] : 0.0;
    for (int t = 0; t < n; ++t) {
        const double et = eq;
        const int ta = t + 1;
        eq = (ta < n && l > ta && l < n) ? Ep[eidx(l, ta)] : 0.0;
        const double xt = ntm::gbcast<64>(sq_id * acc, t);
        if (l == t) x = xt;
        acc = __builtin_fma(-et, xt, acc);
        if (nc >= 0) {
            const double zt = ntm::gbcast<64>(sq_id * acz, t);
            if (l == t) zz = zt;
            acz = __builtin_fma(-et, zt, acz);
        }
    }
}
// the certificate's back substitution E' mu = grad, the loop form
__device__ __forceinline__ void ref_backward(const double* Ep, int n, int l, double acc, double sq_id, double& mu) {
#pragma clang fp contract(off)
    for (int u = n - 1; u >= 0; --u) {
        const double eu = (l < u) ? Ep[eidx(u, l)] : 0.0;
        const double mu_u = ntm::gbcast<64>(sq_id * acc, u);
        if (l == u) mu = mu_u;
        acc = __builtin_fma(-eu, mu_u, acc);
    }
}

__global__ void k_cases(Case* cases) {
    __shared__ double lds[kImg];
    Case& c = cases[blockIdx.x];
    const int lane = threadIdx.x;
    for (int i = lane; i < kImg; i += 64) lds[i] = c.img[i];
    __syncthreads();
    const int n = __builtin_amdgcn_readfirstlane(c.n), nc = __builtin_amdgcn_readfirstlane(c.nc);
    double* const Ep = lds + kGuard;
    const double sq = c.sq[lane], h = c.h[lane], z = c.z[lane], g = c.g[lane];
    // the loop form, every lane on
    double rx = 0.0, rz = 0.0, rmu = 0.0;
    ref_forward(Ep, n, nc, lane, h, z, sq, rx, rz);
    ref_backward(Ep, n, lane, g, sq, rmu);
    c.rok = !(__ballot(lane < n && !(isfinite(rx) && isfinite(rz))) != 0ull);
    // the helpers, under the entry EXEC
    double mx = sentinel(lane, 0), mz = sentinel(lane, 1), mmu = sentinel(lane, 2);
    if ((c.entry >> lane) & 1ull) {
        double acc = h, acz = z, acb = g;
        const unsigned row = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)(Ep + eidx(lane, 0));
        const unsigned col = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)(Ep + lane);
        if (nc >= 0) ntm::fsub_lanes<true>(n, acc, mx, acz, mz, sq, row);
        else ntm::fsub_lanes<false>(n, acc, mx, acz, mz, sq, row);
        c.sent[lane] = 0x5A000000u + lane;
        ntm::bsub_lanes(n, acb, mmu, sq, col);
        c.sent[lane] += 0x00010000u;
    }
    // one right-hand side: zz stays what it was (0.0 in the kernel) on every lane
    const double zv = (nc >= 0) ? mz : ((mz == sentinel(lane, 1)) ? 0.0 : mz);
    c.mok = !(__ballot(lane < n && !(isfinite(mx) && isfinite(zv))) != 0ull);
    c.rx[lane] = rx;
    c.rz[lane] = rz;
    c.rmu[lane] = rmu;
    c.mx[lane] = mx;
    c.mz[lane] = mz;
    c.mmu[lane] = mmu;
    __syncthreads();
    for (int i = lane; i < kImg; i += 64) c.after[i] = lds[i];
}

static double poison() { return from_bits(kPoison); }
static uint64_t rnd_u() { return rng_step() >> 11; }
static double rnd() {                                   // finite, both signs, 2^-2 .. 2^2
    const double u = (double)rnd_u() / 9007199254740992.0;
    const int e = (int)(rnd_u() % 5u) - 2;
    return (2.0 * u - 1.0) * std::ldexp(1.0, e);
}

static int bad = 0;
static void fail(const char* what, int c, const Case& k, int at, double a, double b) {
    if (bad < 16)
        std::printf("%s: case %d (n %d nc %d entry %016llx) at %d: loop form %.17g (%a) helpers %.17g (%a)\n", what, c,
                    k.n, k.nc, k.entry, at, a, a, b, b);
    ++bad;
}

enum Kind { kFinite, kInfH, kNanH, kInfE, kNanE, kInfD, kNanD, kKinds };
static void make_case(Case& c, int n, int nc, unsigned long long entry, int kind) {
    std::memset(&c, 0, sizeof c);
    c.n = n;
    c.nc = nc;
    c.entry = entry;
    for (int i = 0; i < kImg; ++i) c.img[i] = poison();
    double* const E = c.img + kGuard;
    for (int t = 0; t < n; ++t)
        for (int u = 0; u <= t; ++u) {
            double v = rnd();
            if (u < t && rnd_u() % 4u == 0) v = (rnd_u() & 1u) ? 0.0 : -0.0;   // exact zeros off the diagonal
            if (u == t && std::fabs(v) < 0x1p-6) v = 0.75;
            E[(t * (t + 1)) / 2 + u] = v;
        }
    for (int l = 0; l < 64; ++l) {
        const bool in = l < n;
        c.sq[l] = in ? 1.0 / E[(l * (l + 1)) / 2 + l] : 0.0;
        c.h[l] = in ? (rnd_u() % 6u == 0 ? -0.0 : rnd()) : 0.0;
        c.z[l] = (in && nc >= 0 && l >= nc) ? (rnd_u() % 6u == 0 ? -0.0 : rnd()) : 0.0;   // -e_c: rows from the hole on
        c.g[l] = in ? (rnd_u() % 6u == 0 ? -0.0 : rnd()) : 0.0;
        c.sent[l] = kPoison32;
    }
    if (n > 0 && kind != kFinite) {
        const double special = (kind == kInfH || kind == kInfE || kind == kInfD) ? __builtin_huge_val() : __builtin_nan("");
        const int at = (int)(rnd_u() % (unsigned)n);
        if (kind == kInfH || kind == kNanH) {
            c.h[at] = special;
            c.g[(at + 1) % n] = special;
            if (nc >= 0 && at >= nc) c.z[at] = -special;
        } else if (kind == kInfD || kind == kNanD) {
            c.sq[at] = special;
        } else if (n > 1) {
            const int t = 1 + (int)(rnd_u() % (unsigned)(n - 1)), u = (int)(rnd_u() % (unsigned)t);
            E[(t * (t + 1)) / 2 + u] = special;
        }
    }
}

static void check_case(int ci, const Case& c) {
    const int n = c.n;
    // forward: lane l is comparable when it and every lane below it entered; backward: it and every lane
    // above it that lies below n
    int fclean = 0;
    while (fclean < n && ((c.entry >> fclean) & 1ull)) ++fclean;
    int bclean = n;
    while (bclean > 0 && ((c.entry >> (bclean - 1)) & 1ull)) --bclean;
    for (int l = 0; l < 64; ++l) {
        const bool on = (c.entry >> l) & 1ull;
        if (on ? c.sent[l] != 0x5A010000u + l : c.sent[l] != kPoison32)
            fail(on ? "EXEC not restored (sentinel missing)" : "an off lane ran", ci, c, l, 0, 0);
        if (!on || l >= n) {
            if (!same_bits(c.mx[l], h_sentinel(l, 0))) fail("x of a lane that is off or >= n written", ci, c, l, 0, c.mx[l]);
            if (!same_bits(c.mz[l], h_sentinel(l, 1))) fail("zz of a lane that is off or >= n written", ci, c, l, 0, c.mz[l]);
            if (!same_bits(c.mmu[l], h_sentinel(l, 2))) fail("mu of a lane that is off or >= n written", ci, c, l, 0, c.mmu[l]);
            continue;
        }
        if (l < fclean) {
            if (!same_bits(c.rx[l], c.mx[l])) fail("x", ci, c, l, c.rx[l], c.mx[l]);
            if (c.nc >= 0 && !same_bits(c.rz[l], c.mz[l])) fail("zz", ci, c, l, c.rz[l], c.mz[l]);
        }
        if (c.nc < 0 && !same_bits(c.mz[l], h_sentinel(l, 1))) fail("zz written with one right-hand side", ci, c, l, 0, c.mz[l]);
        if (l >= bclean && !same_bits(c.rmu[l], c.mmu[l])) fail("mu", ci, c, l, c.rmu[l], c.mmu[l]);
    }
    if (fclean == n && c.rok != c.mok) fail("ok", ci, c, 0, c.rok, c.mok);
    for (int i = 0; i < kImg; ++i)
        if (!same_bits(c.img[i], c.after[i])) fail("an LDS word changed", ci, c, i, c.img[i], c.after[i]);
}

int main() {
    const unsigned long long all = ~0ull, upto_n = (1ull << (kN + 1)) - 1ull, irregular = 0xF0F00000002B56FFull;   // below n: 0..7, 9, 10, 12, 14, 16, 17, 19
    std::vector<Case> cases;
    for (int n = 0; n <= kN; ++n)
        for (int nc = -1; nc <= n; ++nc)
            for (unsigned long long entry : {all, upto_n, irregular})
                for (int kind = 0; kind < kKinds; ++kind) {
                    cases.emplace_back();
                    make_case(cases.back(), n, nc, entry, kind);
                }
    const int nb = (int)cases.size();
    Case* d = nullptr;
    if (hipMalloc(&d, sizeof(Case) * cases.size()) != hipSuccess ||
        hipMemcpy(d, cases.data(), sizeof(Case) * cases.size(), hipMemcpyHostToDevice) != hipSuccess) {
        std::printf("FAIL echelon_sub_check: no device memory\n");
        return 1;
    }
    hipLaunchKernelGGL(k_cases, dim3(nb), dim3(64), 0, 0, d);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(cases.data(), d, sizeof(Case) * cases.size(), hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("FAIL echelon_sub_check: the kernel failed\n");
        return 1;
    }
    (void)hipFree(d);
    int nonfinite = 0, notok = 0;
    for (int i = 0; i < nb; ++i) {
        check_case(i, cases[i]);
        notok += !cases[i].rok;
        for (int l = 0; l < cases[i].n; ++l) nonfinite += !std::isfinite(cases[i].rx[l]) || !std::isfinite(cases[i].rmu[l]);
    }
    if (notok == 0 || nonfinite == 0) {
        std::printf("the non-finite cases reached nothing\n");
        ++bad;
    }
    std::printf("%s echelon_sub_check: %d mismatches (%d cases: n = 0..20, nc = -1..n, three entry EXECs, %d data kinds; "
                "%d of them not ok)\n",
                bad ? "FAIL" : "PASS", bad, nb, (int)kKinds, notok);
    return bad ? 1 : 0;
}
