// Stand-alone check of the lane-masked row pass of the scaling pass (csrc/ntm_lanes.h:
// rownorm5_lanes_from, under row_norm_lanes of csrc/ntm_gram.h) against the loop form it
// replaces in diag_scale_phase, bit for bit.  One 64-lane block per case.
//
//   hipcc --offload-arch=gfx950 -O3 -o cert_passes_check tools/cert_passes_check.hip
//   ./cert_passes_check       -> one PASS / FAIL line, exit status 1 on a mismatch
//
// A case fills the packed Gamma and D of a far N = 20 workspace in LDS, runs both forms on
// the lanes of an entry mask and compares, per lane, the sum of squares s (bits), the last
// non-zero column, the count of non-zeros and the rinfo word built from them; with them
// the values the kernel derives from s alone: 1 / sqrt(s) as it stores it in irn[r] (bits;
// 0 for a constant row) and the non-finite flag.  The loop form is the one of
// diag_scale_phase, copied: every term on every lane, the square and the tracking under
// `j <= r / 2`.
//   random     random finite Gamma and D;
//   sparse     rows with no, one and several non-zeros, the non-zeros first, last and in
//              the middle of the row's range, the rest exact zeros and -0.0 (a -0.0 is no
//              non-zero); the entries past a row's range (the aliased ones a lane >= 2j
//              never reads, and the ones a lane < 2j would) are random non-zeros;
//   nonfinite  an infinity or a NaN in Gamma, inside a row's range and outside it (on the
//              aliased entries past the row's range), and a non-finite D_j;
//   seeded     s, last and cnt not at their initial values on entry (the helper adds to
//              what it is given, as the loop form does).
// Every kind runs under four entry EXECs: full (the lanes >= 2N enter and must come out
// untouched: the kernel never does this, the helper allows it), the lanes >= 2N off, and
// two irregular patterns (rows below 2N off, lane 0 among them; every other pair of lanes
// off with the lanes >= 56 on).  s, last and cnt of the masked form live in registers that
// are set on every lane before the branch on the entry mask, a lane off on entry holding
// a sentinel of its own in each, and are stored by all 64 lanes after the branch has
// reconverged: a lane off on entry must still hold its three sentinels bit for bit (the
// helper's masks are ANDed with the entry EXEC), and it writes nothing inside the branch
// (poisoned output, sentinel word included).  A lane that entered writes its sentinel word
// right behind the helper (EXEC restored); a lane >= 2N that entered keeps s, last and cnt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../mpc-ntm-control_amd/csrc/ntm_gram.h"
#include "../mpc-ntm-control_amd/csrc/ntm_ws.h"
#include "check_common.h"

using W20 = ntm::WS<20, false, true>;
constexpr int kN = 20, kGam = kN * (kN + 1), kLds = ntm::ws_doubles(kN, true) + 8;
static_assert(W20::kSlim && ntm::esub_lanes_ok<64, 5, W20>(), "the slim far N = 20 workspace must take the masked form");
static_assert(!ntm::esub_lanes_ok<0, 5, W20>() && !ntm::esub_lanes_ok<32, 5, W20>() && !ntm::esub_lanes_ok<64, 4, W20>() &&
                  !ntm::esub_lanes_ok<64, 5, ntm::WS<50, false, true>>() && !ntm::esub_lanes_ok<64, 5, ntm::WS<20, false, false>>() &&
                  !ntm::esub_lanes_ok<64, 5, ntm::WS<0>>(),
              "no other kernel may reach the masked form");

struct RowIn {
    double G[kGam], D[kN], s0[64];
    int last0[64], cnt0[64];
};
struct RowOut {
    double s_loop[64], s_lane[64], ir_loop[64], ir_lane[64];
    int last_loop[64], last_lane[64], cnt_loop[64], cnt_lane[64], ri_loop[64], ri_lane[64], bad_loop[64], bad_lane[64];
    unsigned sent[64];
    double after_s[64];                                   // the masked form's registers behind the branch, every lane
    int after_last[64], after_cnt[64];
};

__device__ __forceinline__ void derive(double s, int last, int cnt, double& ir, int& ri, int& bad) {
    bad = !isfinite(s);
    ir = (s > 0.0 && s < ntm::kInf) ? ntm::rsqrt_nr(s) : 0.0;
    ri = (last + 1) | (cnt > 1 ? ntm::kRowMulti : 0);
}

__global__ void k_rows(const RowIn* in, unsigned long long entry, RowOut* out) {
    __shared__ double lds[kLds];
    const int lane = threadIdx.x;
    W20 w;
    w.N_rt = kN;
    w.base = lds;
    w.far = nullptr;
    for (int i = lane; i < kGam; i += 64) w.Gt()[i] = in->G[i];
    if (lane < kN) w.D()[lane] = in->D[lane];
    __syncthreads();
    // the masked form's sum and tracking: set on every lane (a lane off on entry: its sentinels)
    double sm = in->s0[lane];
    int lastm = in->last0[lane], cntm = in->cnt0[lane];
    if ((entry >> lane) & 1ull) {
        const int N = kN;
        // the loop form of diag_scale_phase; a lane >= 2N takes no trip of `r = l; r < 2N`
        double s = in->s0[lane];
        int last = in->last0[lane], cnt = in->cnt0[lane];
        if (lane < 2 * N) {
            const int r = lane, jmax = r >> 1;
            constexpr int CH = 5;
            for (int j0 = 0; j0 < N; j0 += CH) {
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
                    const bool inr = j0 + u <= jmax;
                    s += inr ? v * v : 0.0;
                    if (inr && g[u] != 0.0) { last = j0 + u; ++cnt; }
                }
            }
        }
        ntm::row_norm_lanes(w, lane, sm, lastm, cntm);
        out->sent[lane] = 0xA5000000u + lane;
        out->s_loop[lane] = s;
        out->s_lane[lane] = sm;
        out->last_loop[lane] = last;
        out->last_lane[lane] = lastm;
        out->cnt_loop[lane] = cnt;
        out->cnt_lane[lane] = cntm;
        derive(s, last, cnt, out->ir_loop[lane], out->ri_loop[lane], out->bad_loop[lane]);
        derive(sm, lastm, cntm, out->ir_lane[lane], out->ri_lane[lane], out->bad_lane[lane]);
    }
    // reconverged: what every lane's registers hold now, the lanes off on entry included
    out->after_s[lane] = sm;
    out->after_last[lane] = lastm;
    out->after_cnt[lane] = cntm;
}

static double rnd() {                                   // finite, both signs, a few decades, never zero
    const double u = (double)(rng_step() >> 11) / 9007199254740992.0;
    const int e = (int)((rng_step() >> 33) % 9u) - 4;
    const double v = (2.0 * u - 1.0) * std::ldexp(1.0, 3 * e);
    return v == 0.0 ? 1.0 : v;
}
static int gidx(int r, int j) { return j * (2 * kN - j - 1) + r; }   // W20::gidx

static int bad = 0;
static void fail(const char* what, int c, int lane, double a, double b) {
    if (bad < 12) std::printf("%s case %d lane %d: loop %.17g (%a) masked %.17g (%a)\n", what, c, lane, a, a, b, b);
    ++bad;
}

enum Kind { kRandom, kSparse, kNonFinite, kSeeded };
struct Tally { int rows_none = 0, rows_one = 0, rows_multi = 0, flagged = 0, constant = 0, off_checked = 0, off_rows = 0; };

static void rows_case(int c, Kind kind, unsigned long long entry, RowIn* d_in, RowOut* d_out, Tally& t) {
    static RowIn in;
    static RowOut h;
    for (auto& e : in.G) e = rnd();
    for (auto& e : in.D) e = std::fabs(rnd());
    for (int lane = 0; lane < 64; ++lane) {
        in.s0[lane] = 0.0;
        in.last0[lane] = -1;
        in.cnt0[lane] = 0;
    }
    if (kind == kSeeded)
        for (int lane = 0; lane < 64; ++lane) {
            in.s0[lane] = std::fabs(rnd());
            in.last0[lane] = (int)(rng_step() >> 40) % 20;
            in.cnt0[lane] = (int)(rng_step() >> 40) % 3;
        }
    for (int lane = 0; lane < 64; ++lane)                   // off on entry: a sentinel of its own in each register
        if (!((entry >> lane) & 1ull)) {
            in.s0[lane] = from_bits(0x40C0DE0000000000ull + (uint64_t)lane);
            in.last0[lane] = 1000 + lane;
            in.cnt0[lane] = 2000 + lane;
        }
    if (kind == kSparse)                                    // row r: a pattern of its own over j <= r / 2
        for (int r = 0; r < 2 * kN; ++r) {
            const int jm = r >> 1, pat = (r + c) % 8;
            for (int j = 0; j <= jm; ++j) {
                bool nz;
                switch (pat) {
                    case 0: nz = false; break;                          // no non-zero: a constant row
                    case 1: nz = j == 0; break;                         // one, first
                    case 2: nz = j == jm; break;                        // one, last
                    case 3: nz = j == jm / 2; break;                    // one, in the middle
                    case 4: nz = j == 0 || j == jm; break;              // first and last
                    case 5: nz = j > 0 && j < jm; break;                // all but the ends
                    case 6: nz = (j & 1) != 0; break;                   // every other one
                    default: nz = j + 1 >= jm; break;                   // the last two
                }
                if (!nz) in.G[gidx(r, j)] = ((r + j) & 1) ? -0.0 : 0.0;
            }
        }
    if (kind == kNonFinite) {
        const int r1 = 7 + c % 5, r2 = 25 + c % 9, r3 = 33;
        in.G[gidx(r1, r1 >> 1)] = __builtin_huge_val();                 // inside row r1's range, its last term
        in.G[gidx(r2, 1)] = __builtin_nan("");                          // inside row r2's range
        in.G[gidx(r3, 17)] = -__builtin_huge_val();                     // past row 33's range (j <= 16)
        in.G[gidx(4, 19)] = __builtin_nan("");                          // past row 4's range
        if (c & 1) in.D[12 + c % 8] = (c & 2) ? __builtin_huge_val() : __builtin_nan("");   // rows >= 2j see it
    }
    if (hipMemcpy(d_in, &in, sizeof in, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_out, kPoisonByte, sizeof(RowOut)) != hipSuccess) { ++bad; return; }
    hipLaunchKernelGGL(k_rows, dim3(1), dim3(64), 0, 0, d_in, entry, d_out);
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&h, d_out, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("rows case %d: the kernel failed\n", c);
        ++bad;
        return;
    }
    for (int lane = 0; lane < 64; ++lane) {
        if (!((entry >> lane) & 1ull)) {                    // off on entry: nothing written
            const bool clean = poisoned(&h.s_loop[lane], 8) && poisoned(&h.s_lane[lane], 8) && poisoned(&h.ir_lane[lane], 8) &&
                               poisoned(&h.last_lane[lane], 4) && poisoned(&h.cnt_lane[lane], 4) &&
                               poisoned(&h.ri_lane[lane], 4) && poisoned(&h.sent[lane], 4);
            if (!clean) fail("rows: an off lane wrote", c, lane, 0, 0);
            if (!same_bits(h.after_s[lane], in.s0[lane])) fail("rows: an off lane's sum touched", c, lane, in.s0[lane], h.after_s[lane]);
            if (h.after_last[lane] != in.last0[lane]) fail("rows: an off lane's last touched", c, lane, in.last0[lane], h.after_last[lane]);
            if (h.after_cnt[lane] != in.cnt0[lane]) fail("rows: an off lane's count touched", c, lane, in.cnt0[lane], h.after_cnt[lane]);
            ++t.off_checked;
            t.off_rows += lane < 2 * kN;
            continue;
        }
        if (!same_bits(h.after_s[lane], h.s_lane[lane]) || h.after_last[lane] != h.last_lane[lane] || h.after_cnt[lane] != h.cnt_lane[lane])
            fail("rows: registers behind the branch", c, lane, h.s_lane[lane], h.after_s[lane]);
        if (h.sent[lane] != 0xA5000000u + lane) fail("rows: EXEC not restored (sentinel missing)", c, lane, 0, 0);
        if (!same_bits(h.s_loop[lane], h.s_lane[lane])) fail("rows sum of squares", c, lane, h.s_loop[lane], h.s_lane[lane]);
        if (!same_bits(h.ir_loop[lane], h.ir_lane[lane])) fail("rows 1 / norm", c, lane, h.ir_loop[lane], h.ir_lane[lane]);
        if (h.last_loop[lane] != h.last_lane[lane]) fail("rows last non-zero", c, lane, h.last_loop[lane], h.last_lane[lane]);
        if (h.cnt_loop[lane] != h.cnt_lane[lane]) fail("rows non-zero count", c, lane, h.cnt_loop[lane], h.cnt_lane[lane]);
        if (h.ri_loop[lane] != h.ri_lane[lane]) fail("rows rinfo", c, lane, h.ri_loop[lane], h.ri_lane[lane]);
        if (h.bad_loop[lane] != h.bad_lane[lane]) fail("rows non-finite flag", c, lane, h.bad_loop[lane], h.bad_lane[lane]);
        if (lane >= 2 * kN) {                               // entered, but no row: untouched
            if (!same_bits(h.s_lane[lane], in.s0[lane]) || h.last_lane[lane] != in.last0[lane] || h.cnt_lane[lane] != in.cnt0[lane])
                fail("rows: a lane >= 2N touched", c, lane, in.s0[lane], h.s_lane[lane]);
            continue;
        }
        if (kind == kSeeded) continue;
        // against the host: the count and the last non-zero from the data itself
        int last = -1, cnt = 0;
        for (int j = 0; j <= lane >> 1; ++j)
            if (in.G[gidx(lane, j)] != 0.0) { last = j; ++cnt; }
        if (last != h.last_lane[lane] || cnt != h.cnt_lane[lane]) fail("rows tracking against the host", c, lane, last, h.last_lane[lane]);
        t.rows_none += cnt == 0;
        t.rows_one += cnt == 1;
        t.rows_multi += cnt > 1;
        t.flagged += h.bad_lane[lane] != 0;
        t.constant += h.ir_lane[lane] == 0.0;
    }
}

int main() {
    RowIn* d_in = nullptr;
    RowOut* d_out = nullptr;
    if (hipMalloc(&d_in, sizeof(RowIn)) != hipSuccess || hipMalloc(&d_out, sizeof(RowOut)) != hipSuccess) {
        std::printf("FAIL cert_passes_check: no device memory\n");
        return 1;
    }
    const unsigned long long rows40 = (1ull << 40) - 1ull;                 // lanes >= 2N off
    const unsigned long long irregular = 0x000000B7D3A5C96Eull & rows40;   // some rows off, lane 0 among them
    int c = 0;
    Tally t;
    for (unsigned long long entry : {~0ull, rows40, irregular, 0xFF5A5A5A5A5A5A5Aull}) {
        for (int rep = 0; rep < 2; ++rep) rows_case(c++, kRandom, entry, d_in, d_out, t);
        for (int rep = 0; rep < 8; ++rep) rows_case(c++, kSparse, entry, d_in, d_out, t);
        for (int rep = 0; rep < 4; ++rep) rows_case(c++, kNonFinite, entry, d_in, d_out, t);
        rows_case(c++, kSeeded, entry, d_in, d_out, t);
    }
    if (!t.off_rows) {
        std::printf("no lane below 2N was off on entry in any case\n");
        ++bad;
    }
    if (!t.rows_none || !t.rows_one || !t.rows_multi || !t.flagged || !t.constant) {
        std::printf("the cases miss a kind of row: none %d one %d several %d non-finite %d constant %d\n", t.rows_none,
                    t.rows_one, t.rows_multi, t.flagged, t.constant);
        ++bad;
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    std::printf("%s cert_passes_check: %d mismatches in %d row-pass cases (rows with no / one / several non-zeros: %d / %d / "
                "%d, non-finite sums %d, constant rows %d; lanes off on entry compared with their sentinels: %d, %d of them below 2N)\n",
                bad ? "FAIL" : "PASS", bad, c, t.rows_none, t.rows_one, t.rows_multi, t.flagged, t.constant, t.off_checked, t.off_rows);
    return bad ? 1 : 0;
}
