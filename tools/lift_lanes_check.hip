// Stand-alone check of the lane-masked lift recursion of csrc/ntm_lanes.h and ntm_lift.h
// (lift_chunk_lanes / lift_chunk_at under lift_phase's slim far N = 20 branch)
// against the select form it replaces, bit for bit.  One 64-lane block.
//
//   hipcc --offload-arch=gfx950 -O3 -o lift_lanes_check tools/lift_lanes_check.hip
//   ./lift_lanes_check        -> one PASS / FAIL line, exit status 1 on a mismatch
//
// The select form lives here (lift_select): every lane l <= N computes the next
// 2-vector at every stage, keeps the old one while the stage is above its
// diagonal, and stores at the stage or at its own diagonal again.  Its arithmetic
// is pinned to what the production build compiled the C++ loop to (contraction
// off, the fma spelled out): first and last stage of each chunk of five
// t = g0 a21, t = fma(a22, g1, t), g0 = fma(g0, a11, c0); the three between
// t = a22 g1, t = fma(a21, g0, t), g0 = fma(a11, g0, c0); g1 = c1 + t in both.
//
// Lift level: ntm::lift_phase<64> on a slim far N = 20 workspace in LDS, and the
// select form on a second workspace that got the same rho, the product's a11 / a21
// and the product's stage-0 pairs (Gamma's diagonal blocks and e_0), so that the
// recursion alone is compared.  Both workspaces start poisoned and are compared
// whole: rho, a11, a21, e (2N), the packed Gamma (N(N+1)) and the words between and
// behind them, which must still hold the poison.
//   random     finite coefficients, several seeds;
//   nonfinite  an infinity or a NaN in a11 / a21 / b of stage 9 and of stage 0, a NaN
//              x_k: the two forms agree bit for bit, and the parts the value cannot
//              reach equal the finite run of the same seed bit for bit: for a11 / a21
//              of stage j the columns whose diagonal is at or below stage j, for b of
//              stage j every column but j and the whole of e, for x_k all of Gamma.
// Chunk level: the four chunk helpers called directly, the select form under
// `l <= N` next to them, on random and on non-finite data of every lane, with the
// entry EXEC the kernel has (lanes <= N), with all 64 lanes on, and with an
// irregular subset of the lanes <= N.  Lanes above N get a record of their own in
// a poisoned area: they must write nothing and keep g0 / g1; so must a lane that
// was off on entry.  EXEC after the helpers: every lane that entered writes a
// sentinel behind them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define NTM_CH 5                               // the far N = 20 unit's chunk (csrc/ntm_n20.hip): lift_phase takes it from here
#include "../mpc-ntm-control_amd/csrc/ntm_lift.h"
#include "check_common.h"

using W20 = ntm::WS<20, false, true>;
constexpr int kN = 20, kGam = kN * (kN + 1);
constexpr int kWs = 640;                       // rho 60, a11 20, a21 20, scratch 40, e 40, Gamma 420, guard 40
constexpr int kJunk = 40 * (63 - kN);          // chunk level: a 20-stage record for each lane above N
constexpr int kWs2 = kWs + kJunk;
static_assert(ntm::lift_lanes_ok<64, 5, W20>(), "the slim far N = 20 workspace must take the masked lift");
static_assert(!ntm::lift_lanes_ok<64, 4, W20>() && !ntm::lift_lanes_ok<32, 5, W20>() &&
                  !ntm::lift_lanes_ok<64, 5, ntm::WS<20, false, false>>() &&
                  !ntm::lift_lanes_ok<64, 5, ntm::WS<50, false, true>>() && !ntm::lift_lanes_ok<64, 5, ntm::WS<0>>(),
              "no other kernel may reach the masked lift");

__device__ __forceinline__ double poison() { return __builtin_bit_cast(double, kPoison64); }
__device__ __forceinline__ W20 ws_at(double* base) {
    W20 w;
    w.N_rt = kN;
    w.base = base;
    w.far = nullptr;
    return w;
}
// the lane's record: Gamma's column l addressed by stage (lanes < N), e (lane N)
__device__ __forceinline__ double* rec_of(const W20& w, int l) {
    return l < kN ? w.Gt() + w.gidx(2 * l, l) - 2 * l : w.e();
}

// the select form: stage 0 put, then stages 1..N-1, on a lane l <= N
__device__ __forceinline__ void lift_select(double* rec, const double* a11, const double* a21, int l, double& g0,
                                            double& g1, double c0, double c1, double a22) {
#pragma clang fp contract(off)
    const bool gam = l < kN;
    rec[2 * (gam ? l : 0)] = g0;
    rec[2 * (gam ? l : 0) + 1] = g1;
    for (int i = 1; i < kN; ++i) {
        const int u = (i - 1) % 5;
        const double ca = a11[i], cb = a21[i];
        double t, n0;
        if (u == 0 || u == 4) {
            t = g0 * cb;
            t = __builtin_fma(a22, g1, t);
            n0 = __builtin_fma(g0, ca, c0);
        } else {
            t = a22 * g1;
            t = __builtin_fma(cb, g0, t);
            n0 = __builtin_fma(ca, g0, c0);
        }
        const double n1 = c1 + t;
        const bool live = !gam || i > l;
        g0 = live ? n0 : g0;
        g1 = live ? n1 : g1;
        const int at = live ? i : l;
        rec[2 * at] = g0;
        rec[2 * at + 1] = g1;
    }
}

// lift level: out = workspace A (the product), then workspace B (the select form)
__global__ void k_lift(ntm::Prob pb, const double* rho, double x0, double x1, double* out, unsigned* sent) {
    __shared__ double lds[2 * kWs];
    const int lane = threadIdx.x;
    for (int i = lane; i < 2 * kWs; i += 64) lds[i] = poison();
    __syncthreads();
    const W20 wa = ws_at(lds), wb = ws_at(lds + kWs);
    if (lane < 3 * kN) {
        wa.rho()[lane] = rho[lane];
        wb.rho()[lane] = rho[lane];
    }
    __syncthreads();
    ntm::lift_phase<64>(pb, wa, lane, x0, x1);
    sent[lane] = 0xA5000000u + lane;
    if (lane < kN) {
        wb.a11()[lane] = wa.a11()[lane];
        wb.a21()[lane] = wa.a21()[lane];
    }
    __syncthreads();
    if (lane <= kN) {
        const bool gam = lane < kN;
        const double* ra = rec_of(wa, lane);
        double g0 = ra[2 * (gam ? lane : 0)], g1 = ra[2 * (gam ? lane : 0) + 1];
        lift_select(rec_of(wb, lane), wb.a11(), wb.a21(), lane, g0, g1, gam ? 0.0 : pb.k.C1, gam ? 0.0 : pb.k.C2,
                    pb.k.a22);
    }
    __syncthreads();
    for (int i = lane; i < 2 * kWs; i += 64) out[i] = lds[i];
}

struct ChunkIo {
    double a11[kN], a21[kN], g0[64], g1[64], c0[64], c1[64];
    double m0[64], m1[64], s0[64], s1[64];     // g0 / g1 behind the masked and the select form
    unsigned sent[64];
};
// chunk level: the helpers on the lanes of `entry`, the select form under l <= N
__global__ void k_chunks(ChunkIo* io, double a22, unsigned long long entry, double* out) {
    __shared__ double lds[2 * kWs2];
    const int lane = threadIdx.x;
    for (int i = lane; i < 2 * kWs2; i += 64) lds[i] = poison();
    __syncthreads();
    const W20 wa = ws_at(lds), wb = ws_at(lds + kWs2);
    if (lane < kN) {
        wa.a11()[lane] = wb.a11()[lane] = io->a11[lane];
        wa.a21()[lane] = wb.a21()[lane] = io->a21[lane];
    }
    __syncthreads();
    double g0 = io->g0[lane], g1 = io->g1[lane], h0 = g0, h1 = g1;
    const double c0 = io->c0[lane], c1 = io->c1[lane];
    if ((entry >> lane) & 1ull) {
        double* const ra = lane <= kN ? rec_of(wa, lane) : wa.base + kWs + 40 * (lane - kN - 1);
        if (lane <= kN) {
            ra[2 * (lane < kN ? lane : 0)] = g0;
            ra[2 * (lane < kN ? lane : 0) + 1] = g1;
        }
        const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) double*)ra;
        ntm::lift_chunk_at<1, 5>(wa, g0, g1, a22, c0, c1, at);
        ntm::lift_chunk_at<6, 5>(wa, g0, g1, a22, c0, c1, at);
        ntm::lift_chunk_at<11, 5>(wa, g0, g1, a22, c0, c1, at);
        ntm::lift_chunk_at<16, 4>(wa, g0, g1, a22, c0, c1, at);
        io->sent[lane] = 0x5A000000u + lane;
        if (lane <= kN) lift_select(rec_of(wb, lane), wb.a11(), wb.a21(), lane, h0, h1, c0, c1, a22);
    }
    io->m0[lane] = g0;
    io->m1[lane] = g1;
    io->s0[lane] = h0;
    io->s1[lane] = h1;
    __syncthreads();
    for (int i = lane; i < 2 * kWs2; i += 64) out[i] = lds[i];
}

static bool is_poison(double a) { return bits_of(a) == kPoison64; }
static double rnd() {                                   // finite, both signs, 2^-2 .. 2^2
    const double u = (double)(rng_step() >> 11) / 9007199254740992.0;
    const int e = (int)((rng_step() >> 33) % 5u) - 2;
    return (2.0 * u - 1.0) * std::ldexp(1.0, e);
}

static int bad = 0;
static void fail(const char* what, int c, int at, double a, double b) {
    if (bad < 12) std::printf("%s case %d at %d: select %.17g (%a) masked %.17g (%a)\n", what, c, at, a, a, b, b);
    ++bad;
}
static int col_at(int j) { return 180 + j * (2 * kN - j + 1); }   // column j of the packed Gamma in the workspace
constexpr int kE = 140, kG = 180;

static double *d_rho, *d_out;
static unsigned* d_sent;
// runs the lift level on `rho`; ws = workspace A then B.  False if the kernel failed
static bool run_lift(const ntm::Prob& pb, const std::vector<double>& rho, double x0, double x1, std::vector<double>& ws,
                     int c) {
    unsigned sent[64];
    ws.assign(2 * kWs, 0.0);
    if (hipMemcpy(d_rho, rho.data(), 3 * kN * 8, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_sent, kPoisonByte, sizeof sent) != hipSuccess) return false;
    hipLaunchKernelGGL(k_lift, dim3(1), dim3(64), 0, 0, pb, d_rho, x0, x1, d_out, d_sent);
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(ws.data(), d_out, 2 * kWs * 8, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(sent, d_sent, sizeof sent, hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int l = 0; l < 64; ++l)
        if (sent[l] != 0xA5000000u + l) fail("lift: EXEC not restored (sentinel missing)", c, l, 0, 0);
    for (int i = 0; i < kWs; ++i) {
        if (!same_bits(ws[i], ws[kWs + i])) fail("lift: workspace word", c, i, ws[kWs + i], ws[i]);
        const bool guard = (i >= 100 && i < kE) || i >= kG + kGam;
        if (guard && !is_poison(ws[i])) fail("lift: guard word written", c, i, 0, ws[i]);
        if (!guard && is_poison(ws[i])) fail("lift: word not written", c, i, 0, ws[i]);
    }
    return true;
}
static ntm::Prob make_prob() {
    ntm::Prob pb;
    std::memset(&pb, 0, sizeof pb);
    pb.k.a11c = 0.25;
    pb.k.za3 = 2.0;
    pb.k.Ts = 0.5;
    pb.k.bc = 1.5;
    pb.k.a22 = 0.9375 + rnd() / 64;
    pb.k.C1 = rnd();
    pb.k.C2 = rnd();
    pb.N = kN;
    pb.mode = 2;
    pb.Q[0] = pb.Q[3] = 1.0;
    return pb;
}
enum Where { kA11, kA21, kB, kX };
// one injection against the finite run of the same data
static void lift_nonfinite(int& c, Where where, int stage, double special) {
    const ntm::Prob pb = make_prob();
    std::vector<double> rho(3 * kN), fin, nf;
    for (auto& e : rho) e = rnd();
    const double x0 = rnd(), x1 = rnd();
    if (!run_lift(pb, rho, x0, x1, fin, c++)) { std::printf("lift case %d: the kernel failed\n", c - 1); ++bad; return; }
    if (where != kX) rho[3 * stage + (int)where] = special;
    if (!run_lift(pb, rho, where == kX ? special : x0, x1, nf, c++)) { std::printf("lift case %d: the kernel failed\n", c - 1); ++bad; return; }
    int reached = 0;
    for (int j = 0; j < kN; ++j) {                       // Gamma's columns
        const bool touched = where == kX ? false : (where == kB ? j == stage : j < stage);
        for (int r = 0; r < 2 * (kN - j); ++r) {
            const double a = fin[col_at(j) + r], b = nf[col_at(j) + r];
            if (!touched && !same_bits(a, b)) fail("lift: a column the value cannot reach changed", c - 1, col_at(j) + r, a, b);
            reached += touched && !std::isfinite(b);
        }
    }
    const bool e_touched = where == kX || where == kA11 || where == kA21;
    for (int r = 0; r < 2 * kN; ++r) {
        if (!e_touched && !same_bits(fin[kE + r], nf[kE + r])) fail("lift: e changed", c - 1, kE + r, fin[kE + r], nf[kE + r]);
        reached += e_touched && !std::isfinite(nf[kE + r]);
    }
    if (reached == 0) fail("lift: the non-finite value reached nothing", c - 1, stage, 0, special);
}

static void chunks_case(int c, unsigned long long entry, bool nonfinite, ChunkIo* d_io, double* d_out2) {
    static ChunkIo io;
    static std::vector<double> ws(2 * kWs2);
    for (int i = 0; i < kN; ++i) {
        io.a11[i] = rnd();
        io.a21[i] = rnd();
    }
    for (int l = 0; l < 64; ++l) {
        io.g0[l] = rnd();
        io.g1[l] = rnd();
        io.c0[l] = l == kN ? rnd() : 0.0;
        io.c1[l] = l == kN ? rnd() : 0.0;
        if (nonfinite && (l + c) % 7 == 0) io.g0[l] = __builtin_huge_val();
        if (nonfinite && (l + c) % 7 == 3) io.g1[l] = __builtin_nan("");
    }
    if (nonfinite) {
        io.a11[3 + c % 5] = -__builtin_huge_val();
        io.a21[12 + c % 5] = __builtin_nan("");
    }
    std::memset(io.sent, kPoisonByte, sizeof io.sent);
    const double a22 = 0.9375 + rnd() / 64;
    if (hipMemcpy(d_io, &io, sizeof io, hipMemcpyHostToDevice) != hipSuccess) { ++bad; return; }
    hipLaunchKernelGGL(k_chunks, dim3(1), dim3(64), 0, 0, d_io, a22, entry, d_out2);
    static ChunkIo o;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(&o, d_io, sizeof o, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ws.data(), d_out2, 2 * kWs2 * 8, hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("chunks case %d: the kernel failed\n", c);
        ++bad;
        return;
    }
    for (int i = 0; i < kWs2; ++i) {
        if (!same_bits(ws[i], ws[kWs2 + i])) fail("chunks: workspace word", c, i, ws[kWs2 + i], ws[i]);
        const bool data = (i >= 60 && i < 100) || (i >= kE && i < kG + kGam);
        if (!data && !is_poison(ws[i])) fail("chunks: a word outside e and Gamma written", c, i, 0, ws[i]);
    }
    for (int l = 0; l < 64; ++l) {
        const bool on = (entry >> l) & 1ull;
        if (on ? o.sent[l] != 0x5A000000u + l : o.sent[l] != kPoison32)
            fail(on ? "chunks: EXEC not restored (sentinel missing)" : "chunks: an off lane ran", c, l, 0, 0);
        if (!same_bits(o.m0[l], o.s0[l]) || !same_bits(o.m1[l], o.s1[l])) fail("chunks: g behind the stages", c, l, o.s0[l], o.m0[l]);
        if ((!on || l > kN) && (!same_bits(o.m0[l], io.g0[l]) || !same_bits(o.m1[l], io.g1[l])))
            fail("chunks: g of a lane that is off or above N touched", c, l, io.g0[l], o.m0[l]);
        if (!on && l <= kN) {                           // its record stays poisoned in both workspaces
            const int at = l < kN ? col_at(l) : kE;
            if (!is_poison(ws[at]) || !is_poison(ws[at + 1])) fail("chunks: an off lane wrote", c, l, 0, ws[at]);
        }
    }
}

int main() {
    if (hipMalloc(&d_rho, 3 * kN * 8) != hipSuccess || hipMalloc(&d_out, 2 * kWs * 8) != hipSuccess ||
        hipMalloc(&d_sent, 64 * 4) != hipSuccess) {
        std::printf("FAIL lift_lanes_check: no device memory\n");
        return 1;
    }
    int c = 0;
    for (int rep = 0; rep < 6; ++rep) {                  // random finite data
        const ntm::Prob pb = make_prob();
        std::vector<double> rho(3 * kN), ws;
        for (auto& e : rho) e = rnd();
        if (!run_lift(pb, rho, rnd(), rnd(), ws, c++)) { std::printf("lift case %d: the kernel failed\n", c - 1); ++bad; }
    }
    const int nfin = c;
    for (int stage : {9, 0})
        for (Where where : {kA11, kA21, kB}) {
            lift_nonfinite(c, where, stage, __builtin_huge_val());
            lift_nonfinite(c, where, stage, __builtin_nan(""));
        }
    lift_nonfinite(c, kX, 0, __builtin_nan(""));
    const int nlift = c;
    ChunkIo* d_io = nullptr;
    double* d_out2 = nullptr;
    if (hipMalloc(&d_io, sizeof(ChunkIo)) != hipSuccess || hipMalloc(&d_out2, 2 * kWs2 * 8) != hipSuccess) {
        std::printf("FAIL lift_lanes_check: no device memory\n");
        return 1;
    }
    const unsigned long long kernel_entry = (1ull << (kN + 1)) - 1ull, irregular = 0x15A5A5ull;
    for (unsigned long long entry : {kernel_entry, ~0ull, irregular, kernel_entry | 0xF0F0000000000000ull})
        for (int rep = 0; rep < 4; ++rep) chunks_case(c++, entry, rep >= 2, d_io, d_out2);
    (void)hipFree(d_out2);
    (void)hipFree(d_io);
    (void)hipFree(d_sent);
    (void)hipFree(d_out);
    (void)hipFree(d_rho);
    std::printf("%s lift_lanes_check: %d mismatches (%d finite lifts, %d lifts of the non-finite cases, "
                "%d chunk cases under three entry EXECs and all lanes on)\n",
                bad ? "FAIL" : "PASS", bad, nfin, nlift - nfin, c - nlift);
    return bad ? 1 : 0;
}
