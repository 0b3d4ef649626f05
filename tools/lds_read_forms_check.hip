// The three ways to read a pair of adjacent doubles from LDS (16 contiguous bytes per lane):
//   one ds_read2_b64 offset1 = offset0 + 1   (what the compiler emits when it knows 8-byte alignment only)
//   two ds_read_b64
//   one ds_read_b128                          (needs 16-byte alignment)
// 1. Bits: the three forms return the same 16 bytes, with every lane on and under two partial
//    EXEC masks (lanes that are off write nothing).  The PASS line depends on this alone.
// 2. Time: in the far N = 20 kernels' shape (one wave per workgroup, 10 KB of LDS each, so 16
//    waves per CU, 4 per SIMD) every wave issues the same count of pair reads, eight per
//    s_waitcnt lgkmcnt(0), with s_memtime around the loop.  Printed: shader cycles per pair
//    per wave, and that over 16 = LDS cycles per pair as the CU's one LDS pipe sees them (the
//    16 waves run side by side), median over the workgroups.  Three address patterns: lane
//    stride 8 B (conflict-free for every form that can use it; ds_read_b128 cannot, its pairs
//    would be misaligned), lane stride 16 B (the pair of lane l at 16 l: how e / xp / Phi
//    are read by [2l], [2l+1]), and one address for all lanes (a broadcast: how a column pass
//    reads om[2i], om[2i+1]).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "check_common.h"

// a pair as the four dwords of its VGPR quad (x, y: the first double's low and high half)
typedef unsigned d2 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint64_t lo64(d2 v) { return (uint64_t)v.x | ((uint64_t)v.y << 32); }
__device__ __forceinline__ uint64_t hi64(d2 v) { return (uint64_t)v.z | ((uint64_t)v.w << 32); }
constexpr int kLdsBytes = 10240;            // per workgroup, as ws_bytes(20, far) rounds to
constexpr int kWavesPerCu = 16;
constexpr int kPairsPerWait = 8;

#define CHECK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            printf("FAIL %s: %s\n", #x, hipGetErrorString(e_));                         \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

enum Form { kRead2 = 0, kTwoB64 = 1, kB128 = 2 };

// one pair at LDS byte address `at` (a multiple of 16 for kB128, of 8 otherwise), waited for
template <int F>
__device__ __forceinline__ d2 read_pair(unsigned at) {
    d2 v;
    if constexpr (F == kRead2) {
        asm volatile("ds_read2_b64 %0, %1 offset1:1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(at) : "memory");
    } else if constexpr (F == kTwoB64) {
        uint64_t a, b;
        asm volatile("ds_read_b64 %0, %2\n\tds_read_b64 %1, %2 offset:8\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(a), "=&v"(b)
                     : "v"(at)
                     : "memory");
        v.x = (unsigned)a;
        v.y = (unsigned)(a >> 32);
        v.z = (unsigned)b;
        v.w = (unsigned)(b >> 32);
    } else {
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(at) : "memory");
    }
    return v;
}

__device__ __forceinline__ uint64_t lds_word(int i) { return 0x9E3779B97F4A7C15ull * (uint64_t)(i + 1); }

// every lane in `mask` reads the pair at doubles 2 lane + shift, 2 lane + shift + 1 by each form
// (kB128 only where the pair is 16-byte aligned: shift even); out[form][lane][2]
__global__ void __launch_bounds__(64) k_bits(uint64_t* out, unsigned long long mask, int shift) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* w = reinterpret_cast<uint64_t*>(smem);
    const int l = threadIdx.x;
    for (int i = l; i < kLdsBytes / 8; i += 64) w[i] = lds_word(i);
    __syncthreads();
    if ((mask >> l) & 1ull) {
        const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + 8u * (unsigned)(2 * l + shift);
        const d2 a = read_pair<kRead2>(at);
        const d2 b = read_pair<kTwoB64>(at);
        out[(0 * 64 + l) * 2] = lo64(a);
        out[(0 * 64 + l) * 2 + 1] = hi64(a);
        out[(1 * 64 + l) * 2] = lo64(b);
        out[(1 * 64 + l) * 2 + 1] = hi64(b);
        if ((shift & 1) == 0) {
            const d2 c = read_pair<kB128>(at);
            out[(2 * 64 + l) * 2] = lo64(c);
            out[(2 * 64 + l) * 2 + 1] = hi64(c);
        }
    }
}

#define RD2(k) "ds_read2_b64 %" #k ", %8 offset1:1\n\t"
#define RDB(k) "ds_read_b64 %" #k ", %8\n\t"
#define RDB8(k) "ds_read_b64 %" #k ", %8 offset:8\n\t"
#define RDQ(k) "ds_read_b128 %" #k ", %8\n\t"
#define OUT8 "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7)
// kPairsPerWait pair reads of one form, then one wait
template <int F>
__device__ __forceinline__ void eight_pairs(unsigned at) {
    if constexpr (F == kRead2) {
        d2 r0, r1, r2, r3, r4, r5, r6, r7;
        asm volatile(RD2(0) RD2(1) RD2(2) RD2(3) RD2(4) RD2(5) RD2(6) RD2(7) "s_waitcnt lgkmcnt(0)"
                     : OUT8 : "v"(at) : "memory");
    } else if constexpr (F == kTwoB64) {
        double r0, r1, r2, r3, r4, r5, r6, r7;
        asm volatile(RDB(0) RDB8(1) RDB(2) RDB8(3) RDB(4) RDB8(5) RDB(6) RDB8(7)
                     RDB(0) RDB8(1) RDB(2) RDB8(3) RDB(4) RDB8(5) RDB(6) RDB8(7) "s_waitcnt lgkmcnt(0)"
                     : OUT8 : "v"(at) : "memory");
    } else {
        d2 r0, r1, r2, r3, r4, r5, r6, r7;
        asm volatile(RDQ(0) RDQ(1) RDQ(2) RDQ(3) RDQ(4) RDQ(5) RDQ(6) RDQ(7) "s_waitcnt lgkmcnt(0)"
                     : OUT8 : "v"(at) : "memory");
    }
}

// stride: the lane stride of the pair addresses in bytes (8, 16, or 0 for one address)
template <int F>
__global__ void __launch_bounds__(64) k_time(unsigned long long* cyc, int stride, int reps) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t* w = reinterpret_cast<uint64_t*>(smem);
    const int l = threadIdx.x;
    for (int i = l; i < kLdsBytes / 8; i += 64) w[i] = lds_word(i);
    __syncthreads();
    const unsigned at = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem + (unsigned)(stride * l);
    unsigned long long t0, t1;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0) : : "memory");
    for (int r = 0; r < reps; ++r) eight_pairs<F>(at);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1) : : "memory");
    if (l == 0) cyc[blockIdx.x] = t1 - t0;
}

static int fails = 0;
static void bad(const char* what, int form, int lane, int shift, unsigned long long mask) {
    if (fails++ < 8) printf("  %s: form %d lane %d shift %d mask %016llx\n", what, form, lane, shift, mask);
}

template <int F>
static int time_form(unsigned long long* d_cyc, int grid, int stride, int reps, double* per_pair) {
    k_time<F><<<grid, 64, kLdsBytes>>>(d_cyc, stride, 16);          // warm-up: code load, clocks
    k_time<F><<<grid, 64, kLdsBytes>>>(d_cyc, stride, reps);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned long long> c(grid);
    CHECK(hipMemcpy(c.data(), d_cyc, grid * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::nth_element(c.begin(), c.begin() + grid / 2, c.end());
    *per_pair = (double)c[grid / 2] / ((double)reps * kPairsPerWait);
    return 0;
}

int main() {
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    // ---- 1. bits ----
    uint64_t* d_out;
    const size_t nout = 3 * 64 * 2;
    CHECK(hipMalloc(&d_out, nout * 8));
    const unsigned long long masks[3] = {~0ull, (1ull << 40) - 1ull, 0xA5A5F00F0F3C5A96ull};
    int cases = 0;
    for (int mi = 0; mi < 3; ++mi)
        for (int shift = 0; shift < 4; ++shift) {       // pairs at doubles 2 l + shift: 16-byte aligned for even shifts
            CHECK(hipMemset(d_out, kPoisonByte, nout * 8));
            k_bits<<<1, 64, kLdsBytes>>>(d_out, masks[mi], shift);
            CHECK(hipDeviceSynchronize());
            std::vector<uint64_t> o(nout);
            CHECK(hipMemcpy(o.data(), d_out, nout * 8, hipMemcpyDeviceToHost));
            for (int f = 0; f < 3; ++f)
                for (int l = 0; l < 64; ++l) {
                    const bool on = ((masks[mi] >> l) & 1ull) && (f != kB128 || (shift & 1) == 0);
                    for (int h = 0; h < 2; ++h) {
                        const uint64_t got = o[(f * 64 + l) * 2 + h];
                        const uint64_t want = 0x9E3779B97F4A7C15ull * (uint64_t)(2 * l + shift + h + 1);
                        if (on && got != want) bad("wrong bits", f, l, shift, masks[mi]);
                        if (!on && got != kPoison64) bad("a lane that is off wrote", f, l, shift, masks[mi]);
                    }
                    ++cases;
                }
        }
    // ---- 2. time ----
    const int grid = kWavesPerCu * prop.multiProcessorCount;
    unsigned long long* d_cyc;
    CHECK(hipMalloc(&d_cyc, grid * sizeof(unsigned long long)));
    const int reps = 4000;
    const int strides[3] = {8, 16, 0};
    const char* sname[3] = {"lane stride 8 B (conflict-free)", "lane stride 16 B (pair of lane l at 16 l)", "one address (broadcast)"};
    double t[3][3] = {};
    for (int s = 0; s < 3; ++s) {
        if (time_form<kRead2>(d_cyc, grid, strides[s], reps, &t[s][0])) return 1;
        if (time_form<kTwoB64>(d_cyc, grid, strides[s], reps, &t[s][1])) return 1;
        if (strides[s] != 8 && time_form<kB128>(d_cyc, grid, strides[s], reps, &t[s][2])) return 1;
    }
    if (fails) {
        printf("FAIL lds_read_forms_check: %d mismatches in %d lane cases\n", fails, cases);
        return 1;
    }
    printf("PASS lds_read_forms_check: ds_read2_b64 offset1:1, 2 x ds_read_b64 and ds_read_b128 return the same bits "
           "(%d lane cases, full and partial EXEC)\n", cases);
    printf("%d CUs, %d waves per CU (one per workgroup, %d B of LDS each), %d pairs per wave, %d per s_waitcnt\n",
           prop.multiProcessorCount, kWavesPerCu, kLdsBytes, reps * kPairsPerWait, kPairsPerWait);
    printf("cycles per pair: per wave | per CU (= per wave / %d)\n", kWavesPerCu);
    for (int s = 0; s < 3; ++s) {
        printf("  %-44s read2_b64 %7.2f | %5.2f   2 x read_b64 %7.2f | %5.2f", sname[s], t[s][0], t[s][0] / kWavesPerCu,
               t[s][1], t[s][1] / kWavesPerCu);
        if (strides[s] != 8) printf("   read_b128 %7.2f | %5.2f", t[s][2], t[s][2] / kWavesPerCu);
        printf("\n");
    }
    return 0;
}
