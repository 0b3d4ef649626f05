// Stand-alone check of the lane-masked accumulation helpers of csrc/ntm_lanes.h
// (fmac5_lanes_from, fmac5x2_lanes_from and the N = 20 far kernel's
// gamma_row_dot / gamma_row_dot2 of csrc/ntm_dots.h built on them; fadd5_lanes_upto and
// fadd5x2_class_lanes_upto of the column passes) against the select form they
// replace, bit for bit.  One 64-lane block.
//
//   hipcc --offload-arch=gfx950 -O3 -o masked_dot_check tools/masked_dot_check.hip
//   ./masked_dot_check        -> one PASS / FAIL line, exit status 1 on a mismatch
//
// Row level (the production functions on a far N = 20 workspace in LDS, the whole
// packed Gamma filled with random finite numbers, so the aliased entries a row
// reads past its last term hold ordinary data): the masked form (P = 64) against
// the select form (P = 0) and against a host fma chain, with the lanes >= 2N off
// on entry, and with an irregular subset of the rows off on entry.
// Term level (one chunk of five terms, every lane on, the accumulators seeded):
//   random    random finite data and seeds;
//   negzero   every lane with a term left after the chunk's first one passes
//             through -0.0 (a product that underflows to -0.0 onto +0.0) and moves
//             on: bit for bit;
//   endzero   a lane's accumulator is -0.0 when its terms end.  The select form's
//             later masked terms add +-0 (-0.0 + +0.0 = +0.0), the masked form
//             leaves -0.0: the check asserts that the two are equal as numbers and
//             prints how many signs differ.
//   nonfinite infinities and NaNs scattered over g and x2: the masked adds and the
//             non-finite flag of the scaling pass's column terms, bit for bit (the
//             select form adds +0.0 where a term is masked, whatever the term).
// Column level (the two column helpers under partial entry EXEC, as the kernel runs
// them under `l < N`): every lane on, the lanes >= 2N off, and the irregular pattern
// off, on random and on non-finite data of every lane.  The lanes that entered agree
// with the select form bit for bit, flag included; a lane that was off on entry wrote
// nothing (poisoned output, sentinel included), keeps its accumulators' seeds bit for
// bit, and has no bit in the non-finite lane mask, whatever its registers hold.
// EXEC after a helper: every lane that entered writes a sentinel right behind it.
// Non-finite v[j] (inf, NaN): every lane whose row uses entry j (lane >= 2j) must
// be non-finite in both forms.  The other lanes may differ and do: 0 * inf is NaN
// in the select form, the masked form never touches them; the check prints how
// many do.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mpc-ntm-control_amd/csrc/ntm_dots.h"
#include "../mpc-ntm-control_amd/csrc/ntm_ws.h"
#include "check_common.h"

using W20 = ntm::WS<20, false, true>;
constexpr int kN = 20, kGam = kN * (kN + 1), kLds = 1024;
static_assert(ntm::lane_masked_ok<64, 5, W20>(), "the N = 20 far workspace must take the masked form");
static_assert(!ntm::lane_masked_ok<0, 5, W20>() && !ntm::lane_masked_ok<32, 5, W20>() &&
                  !ntm::lane_masked_ok<64, 5, ntm::WS<50, false, true>>() && !ntm::lane_masked_ok<64, 5, ntm::WS<0>>(),
              "no other kernel may reach the masked form");

struct RowOut {
    double sel[64], msk[64], sel1[64], msk1[64], sel2[64], msk2[64];
    double fus[64], fum[64], css[64], csm[64], cfs[64], cfm[64];   // masked adds: select / masked
    unsigned cbs[64], cbm[64];                                     // non-finite flag
    unsigned sent[64], sent2[64], sent3[64];
};

// the production row dots, both forms, on the lanes of `entry`
__global__ void k_rows(const double* G, const double* v1, const double* v2, unsigned long long entry, RowOut* out) {
    __shared__ double lds[kLds];
    const int lane = threadIdx.x;
    W20 w;
    w.N_rt = kN;
    w.base = lds;
    w.far = nullptr;
    double* const sv1 = w.Gt() + kGam;
    double* const sv2 = sv1 + kN;
    for (int i = lane; i < kGam; i += 64) w.Gt()[i] = G[i];
    if (lane < kN) { sv1[lane] = v1[lane]; sv2[lane] = v2[lane]; }
    __syncthreads();
    if ((entry >> lane) & 1ull) {
        out->sel[lane] = ntm::gamma_row_dot<5>(w, lane, sv1);
        out->msk[lane] = ntm::gamma_row_dot<5, 64>(w, lane, sv1);
        out->sent[lane] = 0xA5000000u + lane;
        double a, b, c, d;
        ntm::gamma_row_dot2<5>(w, lane, sv1, sv2, a, b);
        ntm::gamma_row_dot2<5, 64>(w, lane, sv1, sv2, c, d);
        out->sent2[lane] = 0x5A000000u + lane;
        out->sel1[lane] = a;
        out->sel2[lane] = b;
        out->msk1[lane] = c;
        out->msk2[lane] = d;
    }
}

struct TermIn {
    double g[5][64], x1[5][64], x2[5][64], y1[64], y2[64];
};

// one chunk, every lane on: select form as the row dots write it, then the helpers
template <int J0>
__global__ void k_terms(const TermIn* in, RowOut* out) {
    const int lane = threadIdx.x, jm = lane >> 1;
    double g[5], x1[5], x2[5];
    for (int u = 0; u < 5; ++u) {
        g[u] = in->g[u][lane];
        x1[u] = in->x1[u][lane];
        x2[u] = in->x2[u][lane];
    }
    double ys = in->y1[lane], ys1 = in->y1[lane], ys2 = in->y2[lane];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const double gm = (J0 + u <= jm) ? g[u] : 0.0;
        ys += gm * x1[u];
        ys1 += gm * x1[u];
        ys2 += gm * x2[u];
    }
    double ym = in->y1[lane], ym1 = in->y1[lane], ym2 = in->y2[lane];
    ntm::fmac5_lanes_from<J0>(ym, g, x1);
    out->sent[lane] = 0xA5000000u + lane;
    ntm::fmac5x2_lanes_from<J0>(ym1, ym2, g, x1, x2);
    out->sent2[lane] = 0x5A000000u + lane;
    // the masked adds of the column passes: terms on lanes <= i, and the scaling pass's
    // pair with its non-finite flag
    const double s0 = in->y1[lane], f0 = in->y2[lane];
    double fus = s0, css = s0, cfs = f0;
    int bs = 0;
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const bool on = J0 + u >= lane;
        fus += on ? x1[u] : 0.0;
        if (on) bs |= !isfinite(g[u]) || !isfinite(x2[u]);
        css += on ? x1[u] : 0.0;
        cfs += on ? x2[u] : 0.0;
    }
    double fum = s0, csm = s0, cfm = f0;
    unsigned long long nf = 0ull;
    ntm::fadd5_lanes_upto<J0>(fum, x1);
    ntm::fadd5x2_class_lanes_upto<J0>(csm, cfm, nf, x1, x2, g, x2);
    out->sent3[lane] = 0xC3000000u + lane;
    out->fus[lane] = fus; out->fum[lane] = fum;
    out->css[lane] = css; out->csm[lane] = csm;
    out->cfs[lane] = cfs; out->cfm[lane] = cfm;
    out->cbs[lane] = (unsigned)bs;
    out->cbm[lane] = (unsigned)((nf >> lane) & 1ull);
    out->sel[lane] = ys;
    out->msk[lane] = ym;
    out->sel1[lane] = ys1;
    out->msk1[lane] = ym1;
    out->sel2[lane] = ys2;
    out->msk2[lane] = ym2;
}

struct ColOut {
    double fus[64], fum[64], css[64], csm[64], cfs[64], cfm[64];   // inside the region: select / masked
    unsigned long long nfw[64];                                    // the whole non-finite lane mask, as each lane saw it
    unsigned cbs[64], sent[64];
    double afum[64], acsm[64], acfm[64];                           // the accumulators behind the region, every lane
};

// the column helpers on the lanes of `entry`, stages I0..I0+4
template <int I0>
__global__ void k_cols(const TermIn* in, unsigned long long entry, ColOut* out) {
    const int lane = threadIdx.x;
    double g[5], x1[5], x2[5];
    for (int u = 0; u < 5; ++u) {
        g[u] = in->g[u][lane];
        x1[u] = in->x1[u][lane];
        x2[u] = in->x2[u][lane];
    }
    const double s0 = in->y1[lane], f0 = in->y2[lane];
    double fum = s0, csm = s0, cfm = f0;
    if ((entry >> lane) & 1ull) {
        double fus = s0, css = s0, cfs = f0;
        int bs = 0;
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const bool on = I0 + u >= lane;
            fus += on ? x1[u] : 0.0;
            if (on) bs |= !isfinite(g[u]) || !isfinite(x2[u]);
            css += on ? x1[u] : 0.0;
            cfs += on ? x2[u] : 0.0;
        }
        unsigned long long nf = 0ull;
        ntm::fadd5_lanes_upto<I0>(fum, x1);
        ntm::fadd5x2_class_lanes_upto<I0>(csm, cfm, nf, x1, x2, g, x2);
        out->sent[lane] = 0x3C000000u + lane;
        out->fus[lane] = fus; out->fum[lane] = fum;
        out->css[lane] = css; out->csm[lane] = csm;
        out->cfs[lane] = cfs; out->cfm[lane] = cfm;
        out->nfw[lane] = nf;
        out->cbs[lane] = (unsigned)bs;
    }
    out->afum[lane] = fum;
    out->acsm[lane] = csm;
    out->acfm[lane] = cfm;
}

static double rnd() {                                   // finite, both signs, a few decades
    const double u = (double)(rng_step() >> 11) / 9007199254740992.0;
    const int e = (int)((rng_step() >> 33) % 9u) - 4;
    return (2.0 * u - 1.0) * std::ldexp(1.0, 3 * e);
}

static int bad = 0;
static void fail(const char* what, int c, int lane, double a, double b) {
    if (bad < 12) std::printf("%s case %d lane %d: select %.17g (%a) masked %.17g (%a)\n", what, c, lane, a, a, b, b);
    ++bad;
}

static RowOut* d_out = nullptr;
static bool fetch(RowOut& h) {
    if (hipDeviceSynchronize() != hipSuccess) return false;
    return hipMemcpy(&h, d_out, sizeof h, hipMemcpyDeviceToHost) == hipSuccess;
}
static bool poison() { return hipMemset(d_out, kPoisonByte, sizeof(RowOut)) == hipSuccess; }

// row level; nonfinite_j < 0: finite data.  Returns the count of lanes outside the
// term's rows on which the two forms differ (non-finite data only)
static int rows_case(int c, unsigned long long entry, int nonfinite_j, double special) {
    std::vector<double> G(kGam), v1(kN), v2(kN);
    for (auto& e : G) e = rnd();
    for (auto& e : v1) e = rnd();
    for (auto& e : v2) e = rnd();
    if (nonfinite_j >= 0) v1[nonfinite_j] = special;
    double *dG, *dv1, *dv2;
    if (hipMalloc(&dG, kGam * 8) != hipSuccess || hipMalloc(&dv1, kN * 8) != hipSuccess ||
        hipMalloc(&dv2, kN * 8) != hipSuccess) { ++bad; return 0; }
    (void)hipMemcpy(dG, G.data(), kGam * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv1, v1.data(), kN * 8, hipMemcpyHostToDevice);
    (void)hipMemcpy(dv2, v2.data(), kN * 8, hipMemcpyHostToDevice);
    RowOut h;
    if (!poison()) { ++bad; return 0; }
    hipLaunchKernelGGL(k_rows, dim3(1), dim3(64), 0, 0, dG, dv1, dv2, entry, d_out);
    if (!fetch(h)) { std::printf("rows case %d: the kernel failed\n", c); ++bad; return 0; }
    (void)hipFree(dG); (void)hipFree(dv1); (void)hipFree(dv2);
    int differ = 0;
    for (int lane = 0; lane < 64; ++lane) {
        const bool on = (entry >> lane) & 1ull;
        if (!on) {                                      // nothing written, the sentinels included
            if (h.sent[lane] != kPoison32 || h.sent2[lane] != kPoison32) fail("rows: an off lane wrote", c, lane, 0, 0);
            continue;
        }
        if (h.sent[lane] != 0xA5000000u + lane || h.sent2[lane] != 0x5A000000u + lane)
            fail("rows: EXEC not restored (sentinel missing)", c, lane, 0, 0);
        if (nonfinite_j < 0) {
            double r1 = 0.0, r2 = 0.0;                  // host chain, the row's own terms in order
            for (int j = 0; j <= lane / 2; ++j) {
                const double g = G[j * (2 * kN - j - 1) + lane];
                r1 = std::fma(g, v1[j], r1);
                r2 = std::fma(g, v2[j], r2);
            }
            if (!same_bits(h.sel[lane], h.msk[lane])) fail("rows dot", c, lane, h.sel[lane], h.msk[lane]);
            if (!same_bits(h.sel1[lane], h.msk1[lane])) fail("rows dot2 first", c, lane, h.sel1[lane], h.msk1[lane]);
            if (!same_bits(h.sel2[lane], h.msk2[lane])) fail("rows dot2 second", c, lane, h.sel2[lane], h.msk2[lane]);
            if (!same_bits(h.msk[lane], r1) || !same_bits(h.msk1[lane], r1)) fail("rows dot against the host", c, lane, r1, h.msk[lane]);
            if (!same_bits(h.msk2[lane], r2)) fail("rows dot2 against the host", c, lane, r2, h.msk2[lane]);
        } else if (lane >= 2 * nonfinite_j) {           // the row uses v1[j]: non-finite in both forms
            if (std::isfinite(h.sel[lane]) || std::isfinite(h.msk[lane])) fail("rows non-finite dot", c, lane, h.sel[lane], h.msk[lane]);
            if (std::isfinite(h.sel1[lane]) || std::isfinite(h.msk1[lane])) fail("rows non-finite dot2", c, lane, h.sel1[lane], h.msk1[lane]);
            if (!same_bits(h.sel2[lane], h.msk2[lane])) fail("rows dot2 second (finite v2)", c, lane, h.sel2[lane], h.msk2[lane]);
        } else {
            differ += !same_bits(h.sel[lane], h.msk[lane]) || !same_bits(h.sel1[lane], h.msk1[lane]);
            if (!std::isfinite(h.msk[lane]) || !std::isfinite(h.msk1[lane])) fail("rows: masked form non-finite off the term's rows", c, lane, h.sel[lane], h.msk[lane]);
            if (!same_bits(h.sel2[lane], h.msk2[lane])) fail("rows dot2 second (finite v2)", c, lane, h.sel2[lane], h.msk2[lane]);
        }
    }
    return differ;
}

enum Kind { kRandom, kNegZero, kEndZero, kNonFinite };
template <int J0>
static int terms_case(int c, Kind kind, TermIn* d_in) {
    static TermIn in;
    for (int lane = 0; lane < 64; ++lane) {
        const int jm = lane >> 1;
        in.y1[lane] = (kind == kRandom || kind == kNonFinite) ? rnd() : 0.0;
        in.y2[lane] = (kind == kRandom || kind == kNonFinite) ? rnd() : 0.0;
        for (int u = 0; u < 5; ++u) {
            in.g[u][lane] = rnd();
            in.x1[u][lane] = rnd();
            in.x2[u][lane] = rnd();
        }
        if (kind == kNegZero && J0 + 1 <= jm) {         // first term underflows to -0.0, later ones are the lane's
            in.g[0][lane] = -1e-200;
            in.x1[0][lane] = 1e-200;
            in.x2[0][lane] = 1e-200;
        }
        if (kind == kNonFinite)                         // about one lane in three holds an infinity or a NaN
            for (int u = 0; u < 5; ++u) {
                const int h = (lane * 5 + u + c) % 17;
                if (h == 0) in.g[u][lane] = __builtin_huge_val();
                if (h == 5) in.g[u][lane] = __builtin_nan("");
                if (h == 9) in.x2[u][lane] = -__builtin_huge_val();
                if (h == 13) in.x2[u][lane] = __builtin_nan("");
            }
        if (kind == kEndZero) {                         // the lane's last term of the chunk leaves -0.0
            in.y1[lane] = -0.0;
            in.y2[lane] = -0.0;
            for (int u = 0; u < 5; ++u) {
                in.g[u][lane] = (J0 + u <= jm) ? -0.0 : rnd();
                in.x1[u][lane] = std::fabs(rnd()) + 1.0;
                in.x2[u][lane] = std::fabs(rnd()) + 1.0;
            }
        }
    }
    RowOut h;
    if (hipMemcpy(d_in, &in, sizeof in, hipMemcpyHostToDevice) != hipSuccess || !poison()) { ++bad; return 0; }
    hipLaunchKernelGGL(k_terms<J0>, dim3(1), dim3(64), 0, 0, d_in, d_out);
    if (!fetch(h)) { std::printf("terms case %d: the kernel failed\n", c); ++bad; return 0; }
    int signs = 0, flagged = 0;
    for (int lane = 0; lane < 64; ++lane) {
        if (h.sent[lane] != 0xA5000000u + lane || h.sent2[lane] != 0x5A000000u + lane || h.sent3[lane] != 0xC3000000u + lane)
            fail("terms: EXEC not restored (sentinel missing)", c, lane, 0, 0);
        const double as[3] = {h.fus[lane], h.css[lane], h.cfs[lane]};
        const double am[3] = {h.fum[lane], h.csm[lane], h.cfm[lane]};
        for (int k = 0; k < 3; ++k) {
            if (kind == kEndZero) {
                if (!(as[k] == am[k])) fail("terms endzero, masked add", c, lane, as[k], am[k]);
                signs += !same_bits(as[k], am[k]);
            } else if (!same_bits(as[k], am[k])) {
                static const char* const names[3] = {"terms add on lanes <= i", "terms scaling column s",
                                                     "terms scaling column fs"};
                fail(names[k], c, lane, as[k], am[k]);
            }
        }
        if (h.cbs[lane] != h.cbm[lane]) fail("terms non-finite flag", c, lane, h.cbs[lane], h.cbm[lane]);
        flagged += h.cbm[lane] != 0;
        if (kind == kNonFinite) continue;               // the row dots' forms differ off a non-finite term's rows
        const double s[3] = {h.sel[lane], h.sel1[lane], h.sel2[lane]}, m[3] = {h.msk[lane], h.msk1[lane], h.msk2[lane]};
        for (int k = 0; k < 3; ++k) {
            if (kind == kEndZero) {
                if (!(s[k] == m[k]) || m[k] != 0.0) fail("terms endzero", c, lane, s[k], m[k]);
                signs += !same_bits(s[k], m[k]);
            } else if (!same_bits(s[k], m[k])) {
                fail(kind == kNegZero ? "terms negzero" : "terms random", c, lane, s[k], m[k]);
            }
        }
        if (kind == kNegZero && J0 + 1 <= (lane >> 1) && h.msk[lane] == 0.0) fail("terms negzero: no later term", c, lane, h.sel[lane], h.msk[lane]);
    }
    if (kind == kNonFinite && flagged == 0) fail("terms nonfinite: no lane flagged", c, 0, 0, 0);
    if (kind != kNonFinite && flagged != 0) fail("terms: a lane flagged on finite data", c, 0, 0, 0);
    return signs;
}
template <int I0>
static void cols_case(int c, unsigned long long entry, bool nonfinite, TermIn* d_in, ColOut* d_col) {
    static TermIn in;
    static ColOut h;
    for (int lane = 0; lane < 64; ++lane) {
        in.y1[lane] = rnd();
        in.y2[lane] = rnd();
        for (int u = 0; u < 5; ++u) {
            in.g[u][lane] = rnd();
            in.x1[u][lane] = rnd();
            in.x2[u][lane] = rnd();
            const int k = (lane * 5 + u + c) % 11;          // every lane, the off ones too
            if (nonfinite && k == 0) in.g[u][lane] = __builtin_huge_val();
            if (nonfinite && k == 4) in.g[u][lane] = __builtin_nan("");
            if (nonfinite && k == 7) in.x2[u][lane] = -__builtin_huge_val();
        }
    }
    if (hipMemcpy(d_in, &in, sizeof in, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_col, kPoisonByte, sizeof(ColOut)) != hipSuccess) { ++bad; return; }
    hipLaunchKernelGGL(k_cols<I0>, dim3(1), dim3(64), 0, 0, d_in, entry, d_col);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, d_col, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("cols case %d: the kernel failed\n", c);
        ++bad;
        return;
    }
    int flagged = 0;
    for (int lane = 0; lane < 64; ++lane) {
        if (!((entry >> lane) & 1ull)) {                    // off on entry: nothing written, nothing touched
            const bool clean = poisoned(&h.fus[lane], 8) && poisoned(&h.fum[lane], 8) && poisoned(&h.css[lane], 8) &&
                               poisoned(&h.csm[lane], 8) && poisoned(&h.cfs[lane], 8) && poisoned(&h.cfm[lane], 8) &&
                               poisoned(&h.nfw[lane], 8) && poisoned(&h.cbs[lane], 4) && poisoned(&h.sent[lane], 4);
            if (!clean) fail("cols: an off lane wrote", c, lane, 0, 0);
            if (!same_bits(h.afum[lane], in.y1[lane])) fail("cols: an off lane's sum touched", c, lane, in.y1[lane], h.afum[lane]);
            if (!same_bits(h.acsm[lane], in.y1[lane])) fail("cols: an off lane's s touched", c, lane, in.y1[lane], h.acsm[lane]);
            if (!same_bits(h.acfm[lane], in.y2[lane])) fail("cols: an off lane's fs touched", c, lane, in.y2[lane], h.acfm[lane]);
            continue;
        }
        if (h.sent[lane] != 0x3C000000u + lane) fail("cols: EXEC not restored (sentinel missing)", c, lane, 0, 0);
        if (!same_bits(h.fus[lane], h.fum[lane])) fail("cols add on lanes <= i", c, lane, h.fus[lane], h.fum[lane]);
        if (!same_bits(h.css[lane], h.csm[lane])) fail("cols scaling column s", c, lane, h.css[lane], h.csm[lane]);
        if (!same_bits(h.cfs[lane], h.cfm[lane])) fail("cols scaling column fs", c, lane, h.cfs[lane], h.cfm[lane]);
        if (!same_bits(h.afum[lane], h.fum[lane]) || !same_bits(h.acsm[lane], h.csm[lane]) || !same_bits(h.acfm[lane], h.cfm[lane]))
            fail("cols: sums behind the region", c, lane, h.csm[lane], h.acsm[lane]);
        if (h.nfw[lane] & ~entry) fail("cols: non-finite bit of a lane off on entry", c, lane, 0, 0);
        if (h.cbs[lane] != (unsigned)((h.nfw[lane] >> lane) & 1ull)) fail("cols non-finite flag", c, lane, h.cbs[lane], (double)((h.nfw[lane] >> lane) & 1ull));
        flagged += h.cbs[lane] != 0;
    }
    if (!nonfinite && flagged) fail("cols: a lane flagged on finite data", c, 0, 0, 0);
}
template <int I0>
static void cols_all(int& c, TermIn* d_in, ColOut* d_col) {
    const unsigned long long rows40 = (1ull << 40) - 1ull, irregular = 0x000000B7D3A5C96Eull & rows40;
    for (unsigned long long entry : {~0ull, rows40, irregular, (1ull << 20) - 1ull, 0xAAAAAull})
        for (int nonfinite = 0; nonfinite < 2; ++nonfinite) cols_case<I0>(c++, entry, nonfinite != 0, d_in, d_col);
}
template <int J0>
static void terms_all(int& c, int& signs, TermIn* d_in) {
    for (int rep = 0; rep < 3; ++rep) terms_case<J0>(c++, kRandom, d_in);
    terms_case<J0>(c++, kNegZero, d_in);
    for (int rep = 0; rep < 2; ++rep) terms_case<J0>(c++, kNonFinite, d_in);
    signs += terms_case<J0>(c++, kEndZero, d_in);
}

int main() {
    TermIn* d_in = nullptr;
    if (hipMalloc(&d_out, sizeof(RowOut)) != hipSuccess || hipMalloc(&d_in, sizeof(TermIn)) != hipSuccess) {
        std::printf("FAIL masked_dot_check: no device memory\n");
        return 1;
    }
    const unsigned long long rows40 = (1ull << 40) - 1ull;                 // lanes >= 2N off
    const unsigned long long irregular = 0x000000B7D3A5C96Eull & rows40;   // some rows off, lane 0 among them
    int c = 0, differ = 0, signs = 0;
    for (int rep = 0; rep < 3; ++rep) rows_case(c++, rows40, -1, 0.0);
    for (int rep = 0; rep < 3; ++rep) rows_case(c++, irregular, -1, 0.0);
    rows_case(c++, 0x5555555555ull, -1, 0.0);
    rows_case(c++, 1ull << 39, -1, 0.0);
    const int nrows = c;
    for (int j : {0, 3, 7, 12, 19}) {
        differ += rows_case(c++, rows40, j, __builtin_huge_val());
        differ += rows_case(c++, irregular, j, __builtin_nan(""));
    }
    const int nnf = c - nrows;
    const int c0 = c;
    terms_all<0>(c, signs, d_in);
    terms_all<5>(c, signs, d_in);
    terms_all<10>(c, signs, d_in);
    terms_all<15>(c, signs, d_in);
    const int c1 = c;
    ColOut* d_col = nullptr;
    if (hipMalloc(&d_col, sizeof(ColOut)) != hipSuccess) { std::printf("FAIL masked_dot_check: no device memory\n"); return 1; }
    cols_all<0>(c, d_in, d_col);
    cols_all<5>(c, d_in, d_col);
    cols_all<10>(c, d_in, d_col);
    cols_all<15>(c, d_in, d_col);
    (void)hipFree(d_col);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    std::printf("%s masked_dot_check: %d mismatches (%d finite row cases, %d non-finite row cases, %d chunk cases, "
                "%d column cases under partial entry EXEC); "
                "allowed differences: %d lanes off a non-finite term's rows, %d signs of a zero left at -0.0\n",
                bad ? "FAIL" : "PASS", bad, nrows, nnf, c1 - c0, c - c1, differ, signs);
    return bad ? 1 : 0;
}
