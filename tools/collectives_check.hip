// Stand-alone check of the predicate collectives (gany / gall) and the
// payload-free two-argument gargmin of csrc/ntm_collectives.h against the DPP forms
// they replace: gmaxi of a 0/1 flag, and the four-argument gargmin carrying two
// dummy payloads.  One wave, P = 16, 32 and 64; at P < 64 every group of the wave
// gets its own rotation of the pattern, and one round runs with the even groups
// inactive (the production kernels let groups diverge), so the group masks are
// exercised.
//
//   hipcc --offload-arch=gfx950 -O2 -o collectives_check tools/collectives_check.hip
//   ./collectives_check        -> one PASS / FAIL line, exit status 1 on a mismatch
//
// Patterns: all-false, all-true, a single set lane at every position, equal keys
// (the smaller id must win), -0.0 against +0.0, +-inf keys, all keys +inf, and NaN
// keys.  With NaN keys the argmin is not an order statistic (every comparison
// with a NaN is false), so there the new form is only compared with the old one,
// bit for bit; everywhere else both are also compared with a host reference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../mpc-ntm-control_amd/csrc/ntm_collectives.h"
#include "check_common.h"

struct Rec {
    int any_new, any_old, all_new, all_old;
    int id_new, id_old;
    double v_new, v_old;
};

// cases: 0 all-false, 1 all-true, 2 .. 2+P-1 a single lane, then kExtra key patterns
constexpr int kExtra = 8;
__host__ __device__ inline int n_cases(int P) { return 2 + P + kExtra; }
__host__ __device__ inline bool case_has_nan(int P, int c) { return c == 2 + P + 6 || c == 2 + P + 7; }

// lane li of group g in case c: the predicate, the key and the id
__host__ __device__ inline void pattern(int P, int c, int g, int li, bool& pred, double& key, int& id) {
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    id = (li * 7 + 3 + g) & (P - 1);                  // a permutation of 0..P-1 (7 is odd)
    if (c == 0) { pred = false; key = 1.0 + li; return; }
    if (c == 1) { pred = true; key = -1.0 - li; return; }
    if (c < 2 + P) {                                  // one set lane, rotated by the group
        const int pos = (c - 2 + 5 * g) & (P - 1);
        pred = li == pos;
        key = pred ? -2.5 : 1.0;
        return;
    }
    const int e = c - 2 - P;
    const unsigned h = (unsigned)(li * 2654435761u + g * 40503u + 12345u);
    pred = (h >> 7) & 1;
    switch (e) {
    case 0: key = 3.25; break;                                        // equal keys
    case 1: key = ((li + g) & 1) ? -0.0 : 0.0; break;                 // signed zeros
    case 2: key = (li == ((3 + g) & (P - 1))) ? -inf : ((li & 1) ? inf : 1e300); break;
    case 3: key = inf; break;                                         // nobody holds a key
    case 4: key = (double)(int)((h >> 9) % 11u) - 5.0; break;         // many ties
    case 5: key = (li == ((9 + g) & (P - 1))) ? -1e300 : ((li & 3) ? inf : (double)li); break;
    case 6: key = (li % 5 == 2) ? nan : (double)((int)((h >> 11) % 7u)) - 3.0; break;
    default: key = (li == ((1 + g) & (P - 1))) ? -4.0 : nan; break;   // one number among NaNs
    }
}

template <int P>
__device__ void one_case(int c, int lane, Rec* out) {
    const int g = lane / P, li = lane % P;
    bool pred;
    double key;
    int id;
    pattern(P, c, g, li, pred, key, id);
    Rec r;
    r.any_new = ntm::gany<P>(pred) ? 1 : 0;
    r.any_old = ntm::gmaxi<P>(pred ? 1 : 0) != 0 ? 1 : 0;
    r.all_new = ntm::gall<P>(pred) ? 1 : 0;
    r.all_old = ntm::gmaxi<P>(pred ? 0 : 1) == 0 ? 1 : 0;
    double v1 = key, v2 = key, a = 0.0, b = 0.0;
    int i1 = id, i2 = id;
    ntm::gargmin<P>(v1, i1);
    ntm::gargmin<P>(v2, i2, a, b);
    r.v_new = v1; r.id_new = i1;
    r.v_old = v2; r.id_old = i2;
    out[c * 64 + lane] = r;
}

// round 0: every group runs; round 1 (P < 64): the odd groups only
template <int P>
__global__ void k_check(Rec* out) {
    const int lane = threadIdx.x & 63;
    const int nc = n_cases(P);
    for (int c = 0; c < nc; ++c) one_case<P>(c, lane, out);
    if (P < 64) {
        Rec* out1 = out + nc * 64;
        if ((lane / P) & 1) {
            for (int c = 0; c < nc; ++c) one_case<P>(c, lane, out1);
        }
    }
}

template <int P>
static int run(Rec* d_out, std::vector<Rec>& h) {
    const int nc = n_cases(P), rounds = P < 64 ? 2 : 1;
    const size_t n = (size_t)rounds * nc * 64;
    Rec fill;
    std::memset(&fill, kPoisonByte, sizeof fill);
    h.assign(n, fill);
    if (hipMemcpy(d_out, h.data(), n * sizeof(Rec), hipMemcpyHostToDevice) != hipSuccess) return 1000000;
    hipLaunchKernelGGL(k_check<P>, dim3(1), dim3(64), 0, 0, d_out);
    if (hipDeviceSynchronize() != hipSuccess) return 1000000;
    if (hipMemcpy(h.data(), d_out, n * sizeof(Rec), hipMemcpyDeviceToHost) != hipSuccess) return 1000000;
    int bad = 0;
    for (int rd = 0; rd < rounds; ++rd)
        for (int c = 0; c < nc; ++c)
            for (int g = 0; g < 64 / P; ++g) {
                if (rd == 1 && !(g & 1)) continue;
                // host reference of the group
                bool any = false, all = true;
                double bv = 0.0;
                int bi = 0;
                for (int li = 0; li < P; ++li) {
                    bool p; double k; int id;
                    pattern(P, c, g, li, p, k, id);
                    any = any || p;
                    all = all && p;
                    if (li == 0 || k < bv || (k == bv && id < bi)) { bv = k; bi = id; }
                }
                for (int li = 0; li < P; ++li) {
                    const Rec& r = h[((size_t)rd * nc + c) * 64 + g * P + li];
                    bool ok = r.any_new == r.any_old && r.all_new == r.all_old && r.id_new == r.id_old &&
                              same_bits(r.v_new, r.v_old);
                    ok = ok && r.any_new == (any ? 1 : 0) && r.all_new == (all ? 1 : 0);
                    if (!case_has_nan(P, c)) ok = ok && r.id_new == bi && same_bits(r.v_new, bv);
                    if (!ok) {
                        if (bad < 8)
                            std::printf("P=%d round %d case %d group %d lane %d: any %d/%d (ref %d) all %d/%d (ref %d) "
                                        "argmin new (%g, %d) old (%g, %d) ref (%g, %d)\n",
                                        P, rd, c, g, li, r.any_new, r.any_old, (int)any, r.all_new, r.all_old, (int)all,
                                        r.v_new, r.id_new, r.v_old, r.id_old, bv, bi);
                        ++bad;
                    }
                }
            }
    return bad;
}

int main() {
    Rec* d_out = nullptr;
    const size_t cap = (size_t)2 * n_cases(64) * 64 * sizeof(Rec);   // the largest case count, two rounds
    if (hipMalloc(&d_out, cap) != hipSuccess) { std::printf("FAIL collectives_check: no device memory\n"); return 1; }
    std::vector<Rec> h;
    const int b16 = run<16>(d_out, h), b32 = run<32>(d_out, h), b64 = run<64>(d_out, h);
    (void)hipFree(d_out);
    const int bad = b16 + b32 + b64;
    std::printf("%s collectives_check: P=16 %d, P=32 %d, P=64 %d mismatching lanes (%d + %d + %d cases)\n",
                bad ? "FAIL" : "PASS", b16, b32, b64, 2 * n_cases(16), 2 * n_cases(32), n_cases(64));
    return bad ? 1 : 0;
}
