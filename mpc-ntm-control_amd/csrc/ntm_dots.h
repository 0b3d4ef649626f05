// ntm_dots.h — the chunked LDS contractions: plain and Q-weighted dots over strided
// vectors, the rows of the packed Gamma (gamma_row_dot*) and the column sums over
// 2-vectors (dot_rows2), the last two lane-masked on the far N = 20 kernel (ntm_lanes.h).
#pragma once
#include <hip/hip_runtime.h>

#include "ntm_base.h"
#include "ntm_lanes.h"

namespace ntm {

// ---------------------------------------------------------------------------
// Batched LDS contractions.  The long masked fixed-trip loops below are LDS
// latency chains when the scheduler interleaves each load with its use (the
// 256-VGPR kernels leave it no room to hoist); these helpers issue CH rows of
// loads, fence the scheduler, then consume them, so one LDS round trip serves
// CH terms.  Same terms in the same order as the plain loops.  Loads of the
// tail chunk past n are skipped (zero), never read out of the workspace.
// ---------------------------------------------------------------------------
// sum_{imin <= i < n} a_i' Q b_i over 2-vectors stored at stride 2
template <int CH, class OM>
__device__ __forceinline__ double qdot_rows(const double* a, const double* b, int n, int imin, const OM& om) {
    double s = 0.0;
    NTM_CHUNK_PRAGMA
    for (int i0 = 0; i0 < n; i0 += CH) {
        double a0[CH], a1[CH], b0[CH], b1[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = i0 + u;
            const bool in = i < n;
            a0[u] = in ? a[2 * i] : 0.0;
            a1[u] = in ? a[2 * i + 1] : 0.0;
            b0[u] = in ? b[2 * i] : 0.0;
            b1[u] = in ? b[2 * i + 1] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = i0 + u;
            const double o0 = om.o0(b0[u], b1[u]);
            const double o1 = om.o1(b0[u], b1[u]);
            const double t = a0[u] * o0 + a1[u] * o1;
            s += (i >= imin && i < n) ? t : 0.0;
        }
    }
    return s;
}
// sum_{j < n} a[j sa] b[j sb] (strided LDS vectors)
template <int CH>
__device__ __forceinline__ double dot_batched(const double* a, int sa, const double* b, int sb, int n) {
    double y = 0.0;
    NTM_CHUNK_PRAGMA
    for (int j0 = 0; j0 < n; j0 += CH) {
        double x[CH], z[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < n;
            x[u] = in ? a[j * sa] : 0.0;
            z[u] = in ? b[j * sb] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) y += x[u] * z[u];
    }
    return y;
}
// sum_{lo <= j < hi} a[j sa] b[j sb] (per-lane bounds; terms added in index order)
template <int CH>
__device__ __forceinline__ double dot_range(const double* a, int sa, const double* b, int sb, int lo, int hi) {
    double y = 0.0;
    NTM_CHUNK_PRAGMA
    for (int j0 = lo; j0 < hi; j0 += CH) {
        double x[CH], z[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < hi;
            x[u] = in ? a[j * sa] : 0.0;
            z[u] = in ? b[j * sb] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) y += x[u] * z[u];
    }
    return y;
}
// s - sum_{lo <= j < hi} a[j sa] b[j sb], the terms subtracted one by one in index order
template <int CH>
__device__ __forceinline__ double sub_dot(double s, const double* a, int sa, const double* b, int sb, int lo, int hi) {
    NTM_CHUNK_PRAGMA
    for (int j0 = lo; j0 < hi; j0 += CH) {
        double x[CH], z[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < hi;
            x[u] = in ? a[j * sa] : 0.0;
            z[u] = in ? b[j * sb] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) s -= x[u] * z[u];
    }
    return s;
}
// a[j] -= f b[j] for lo <= j < hi, the loads of CH entries issued ahead of their stores
template <int CH>
__device__ __forceinline__ void axpy_sub(double* a, const double* b, double f, int lo, int hi, int sa = 1) {
    NTM_CHUNK_PRAGMA
    for (int j0 = lo; j0 < hi; j0 += CH) {
        double x[CH], z[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < hi;
            x[u] = in ? a[j * sa] : 0.0;
            z[u] = in ? b[j] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (j0 + u < hi) a[(j0 + u) * sa] = x[u] - f * z[u];
    }
}
// chunk J0 / 5 of row `lane`'s dot(s): the batched loads at compile-time offsets, then the masked terms
template <int J0, class W>
__device__ __forceinline__ void gamma_row_chunk_lanes(const W& w, const double* gr, const double* v, double& y) {
    double g[5], x[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) g[u] = gr[w.gidx(0, J0 + u)];
    ld5<J0, W::kPair>(v, x);                              // (kPair: v is U, d or dr, 16-byte aligned)
    __builtin_amdgcn_sched_barrier(0);
    fmac5_lanes_from<J0>(y, g, x);
}
template <int J0, class W>
__device__ __forceinline__ void gamma_row_chunk2_lanes(const W& w, const double* gr, const double* v1,
                                                       const double* v2, double& y1, double& y2) {
    double g[5], x1[5], x2[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) g[u] = gr[w.gidx(0, J0 + u)];
    ld5<J0, W::kPair>(v1, x1);
    ld5<J0, W::kPair>(v2, x2);
    __builtin_amdgcn_sched_barrier(0);
    fmac5x2_lanes_from<J0>(y1, y2, g, x1, x2);
}

// Gamma_r v restricted to j <= r/2 (row r of the packed block-lower-triangular Gamma).
// P = 64 is passed where the caller's row is its lane (`for (r = l; r < 2N; r += P)`):
// the N = 20 far kernel then masks the terms by lane (lane_masked_ok)
template <int CH, int P = 0, class W>
__device__ __forceinline__ double gamma_row_dot(const W& w, int r, const double* v) {
    const double* gr = w.Gt() + r;                        // gt(r, j) = gr[gidx(0, j)]
    double y = 0.0;
    if constexpr (lane_masked_ok<P, CH, W>()) {
        gamma_row_chunk_lanes<0>(w, gr, v, y);
        gamma_row_chunk_lanes<5>(w, gr, v, y);
        gamma_row_chunk_lanes<10>(w, gr, v, y);
        gamma_row_chunk_lanes<15>(w, gr, v, y);
    } else {
    const int n = w.n(), jm = r >> 1;
    NTM_CHUNK_PRAGMA
    for (int j0 = 0; j0 < n; j0 += CH) {
        double g[CH], x[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < n;
            g[u] = in ? gr[w.gidx(0, j)] : 0.0;
            x[u] = in ? v[j] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            y += (j <= jm ? g[u] : 0.0) * x[u];
        }
    }
    }
    return y;
}

// Gamma_r v1 and Gamma_r v2 in one pass over row r (its loads shared)
template <int CH, int P = 0, class W>
__device__ __forceinline__ void gamma_row_dot2(const W& w, int r, const double* v1, const double* v2, double& y1,
                                               double& y2) {
    const double* gr = w.Gt() + r;
    y1 = 0.0;
    y2 = 0.0;
    if constexpr (lane_masked_ok<P, CH, W>()) {
        gamma_row_chunk2_lanes<0>(w, gr, v1, v2, y1, y2);
        gamma_row_chunk2_lanes<5>(w, gr, v1, v2, y1, y2);
        gamma_row_chunk2_lanes<10>(w, gr, v1, v2, y1, y2);
        gamma_row_chunk2_lanes<15>(w, gr, v1, v2, y1, y2);
    } else {
    const int n = w.n(), jm = r >> 1;
    NTM_CHUNK_PRAGMA
    for (int j0 = 0; j0 < n; j0 += CH) {
        double g[CH], x1[CH], x2[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = j0 + u;
            const bool in = j < n;
            g[u] = in ? gr[w.gidx(0, j)] : 0.0;
            x1[u] = in ? v1[j] : 0.0;
            x2[u] = in ? v2[j] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const double gm = (j0 + u <= jm) ? g[u] : 0.0;
            y1 += gm * x1[u];
            y2 += gm * x2[u];
        }
    }
    }
}

// sum_{imin <= i < n} a_i' c_i over 2-vectors stored at stride 2 (c = Om b precomputed)
template <int CH>
__device__ __forceinline__ double dot_rows2(const double* a, const double* c, int n, int imin) {
    double s = 0.0;
    NTM_CHUNK_PRAGMA
    for (int i0 = 0; i0 < n; i0 += CH) {
        double a0[CH], a1[CH], c0[CH], c1[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = i0 + u;
            const bool in = i < n;
            a0[u] = in ? a[2 * i] : 0.0;
            a1[u] = in ? a[2 * i + 1] : 0.0;
            c0[u] = in ? c[2 * i] : 0.0;
            c1[u] = in ? c[2 * i + 1] : 0.0;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int i = i0 + u;
            const double t = a0[u] * c0[u] + a1[u] * c1[u];
            s += (i >= imin && i < n) ? t : 0.0;
        }
    }
    return s;
}
// chunk I0 / 5 of column `lane`'s sum: the batched loads at compile-time offsets, the
// terms formed on every lane, then added on the lanes <= i
// (AL: a and c are 16-byte aligned, ld_pair)
template <int I0, bool AL>
__device__ __forceinline__ void dot_rows2_chunk_lanes(const double* a, const double* c, double& s) {
    double a0[5], a1[5], c0[5], c1[5], t[5];
#pragma unroll
    for (int u = 0; u < 5; ++u) {
        const int i = I0 + u;
        const dpair av = ld_pair<AL>(a + 2 * i), cv = ld_pair<AL>(c + 2 * i);
        a0[u] = av.x;
        a1[u] = av.y;
        c0[u] = cv.x;
        c1[u] = cv.y;
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 5; ++u) t[u] = a0[u] * c0[u] + a1[u] * c1[u];
    fadd5_lanes_upto<I0>(s, t);
}
// dot_rows2 with imin = the caller's lane (column l on lane l < N): the N = 20 far
// kernel masks the terms by lane (lane_masked_ok) and reads its pairs aligned (a: a
// column of the packed Gamma from its even row 0, c: one of the aligned 2N-vectors)
template <int CH, int P, class W>
__device__ __forceinline__ double dot_rows2(const W&, const double* a, const double* c, int n, int imin) {
    if constexpr (lane_masked_ok<P, CH, W>()) {
        double s = 0.0;
        constexpr bool AL = pair_ld_ok<P, W>();
        dot_rows2_chunk_lanes<0, AL>(a, c, s);
        dot_rows2_chunk_lanes<5, AL>(a, c, s);
        dot_rows2_chunk_lanes<10, AL>(a, c, s);
        dot_rows2_chunk_lanes<15, AL>(a, c, s);
        return s;
    } else {
        return dot_rows2<CH>(a, c, n, imin);
    }
}

}  // namespace ntm
