// ntm_collectives.h — reductions, predicates, broadcasts and argmin over a group of P
// lanes of the wave (P = 4 .. 64).
#pragma once
#include <hip/hip_runtime.h>

namespace ntm {

// ---------------------------------------------------------------------------
// group collectives (width-P segments of the 64-lane wave)
//
// Butterflies run on DPP / permlane VALU ops, not ds_bpermute: quad_perm
// (xor 1, xor 2), row_half_mirror (pairs the quads of an 8-lane group),
// row_mirror (pairs the 8-lane halves of a row), v_permlane16_swap (pairs
// the 16-lane rows of a 32-lane group) and v_permlane32_swap (pairs the wave
// halves).  Every pairing step combines the two operands symmetrically, so
// each lane of a group ends with the bit-identical result and every control
// decision taken on it stays group-uniform.  Callers must be in
// group-uniform control flow (all P lanes active).
// ---------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    int2 a = __builtin_bit_cast(int2, v);
    a.x = __builtin_amdgcn_update_dpp(0, a.x, CTRL, 0xF, 0xF, false);
    a.y = __builtin_amdgcn_update_dpp(0, a.y, CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, a);
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }

// (lower-row value, upper-row value) of a 16-lane (S=16) or 32-lane (S=32) pairing, same in both partners
template <int S>
__device__ __forceinline__ void pair_d(double v, double& lo, double& hi) {
    int2 a = __builtin_bit_cast(int2, v);
    int2 x, y;
    if constexpr (S == 16) {
        auto r0 = __builtin_amdgcn_permlane16_swap(a.x, a.x, false, false);
        auto r1 = __builtin_amdgcn_permlane16_swap(a.y, a.y, false, false);
        x.x = r0[0]; x.y = r1[0]; y.x = r0[1]; y.y = r1[1];
    } else {
        auto r0 = __builtin_amdgcn_permlane32_swap(a.x, a.x, false, false);
        auto r1 = __builtin_amdgcn_permlane32_swap(a.y, a.y, false, false);
        x.x = r0[0]; x.y = r1[0]; y.x = r0[1]; y.y = r1[1];
    }
    lo = __builtin_bit_cast(double, x);
    hi = __builtin_bit_cast(double, y);
}
template <int S>
__device__ __forceinline__ void pair_i(int v, int& lo, int& hi) {
    if constexpr (S == 16) {
        auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        lo = r[0]; hi = r[1];
    } else {
        auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        lo = r[0]; hi = r[1];
    }
}

// P = 64 (one scenario per wave): results of group reductions are identical
// in every lane; readfirstlane makes that visible to the compiler, so the
// branches they feed become scalar branches and loop counters live in SGPRs.
template <int P>
__device__ __forceinline__ int uni(int v) {
    if constexpr (P == 64) return __builtin_amdgcn_readfirstlane(v);
    else return v;
}
template <int P>
__device__ __forceinline__ double uni(double v) {
    if constexpr (P == 64) {
        int2 a = __builtin_bit_cast(int2, v);
        a.x = __builtin_amdgcn_readfirstlane(a.x);
        a.y = __builtin_amdgcn_readfirstlane(a.y);
        return __builtin_bit_cast(double, a);
    } else {
        return v;
    }
}
template <int P>
__device__ __forceinline__ double gsum(double v) {
    v = v + dpp_d<0xB1>(v);                       // quad_perm [1,0,3,2]
    v = v + dpp_d<0x4E>(v);                       // quad_perm [2,3,0,1]
    if constexpr (P >= 8) v = v + dpp_d<0x141>(v);   // row_half_mirror
    if constexpr (P >= 16) v = v + dpp_d<0x140>(v);  // row_mirror
    if constexpr (P >= 32) { double a, b; pair_d<16>(v, a, b); v = a + b; }
    if constexpr (P >= 64) { double a, b; pair_d<32>(v, a, b); v = a + b; }
    return uni<P>(v);
}
template <int P>
__device__ __forceinline__ double gmax(double v) {
    v = fmax(v, dpp_d<0xB1>(v));
    v = fmax(v, dpp_d<0x4E>(v));
    if constexpr (P >= 8) v = fmax(v, dpp_d<0x141>(v));
    if constexpr (P >= 16) v = fmax(v, dpp_d<0x140>(v));
    if constexpr (P >= 32) { double a, b; pair_d<16>(v, a, b); v = fmax(a, b); }
    if constexpr (P >= 64) { double a, b; pair_d<32>(v, a, b); v = fmax(a, b); }
    return uni<P>(v);
}
template <int P>
__device__ __forceinline__ int gmaxi(int v) {
    v = max(v, dpp_i<0xB1>(v));
    v = max(v, dpp_i<0x4E>(v));
    if constexpr (P >= 8) v = max(v, dpp_i<0x141>(v));
    if constexpr (P >= 16) v = max(v, dpp_i<0x140>(v));
    if constexpr (P >= 32) { int a, b; pair_i<16>(v, a, b); v = max(a, b); }
    if constexpr (P >= 64) { int a, b; pair_i<32>(v, a, b); v = max(a, b); }
    return uni<P>(v);
}
// Predicate collectives: does any / every lane of the group hold p?  One v_cmp
// into a lane mask instead of gmaxi's six dependent DPP steps.  P = 64: the
// wave's ballot, a scalar result (so the branch it feeds is a scalar branch);
// P < 64: the ballot masked to the lane's own group.  Same contract as the
// reductions above: group-uniform control flow, all P lanes of the group active
// (lanes of other groups may be inactive: their ballot bits are masked off).
template <int P>
__device__ __forceinline__ unsigned long long group_mask() {
    if constexpr (P == 64) return ~0ull;
    else return ((1ull << P) - 1ull) << ((threadIdx.x & 63) & ~(P - 1));
}
template <int P>
__device__ __forceinline__ bool gany(bool p) {
    if constexpr (P == 64) return __ballot(p) != 0ull;
    else return (__ballot(p) & group_mask<P>()) != 0ull;
}
template <int P>
__device__ __forceinline__ bool gall(bool p) { return !gany<P>(!p); }
// broadcast lane `src` of the group (src group-uniform)
template <int P>
__device__ __forceinline__ double gbcast(double v, int src) {
    if constexpr (P == 64) {
        int2 a = __builtin_bit_cast(int2, v);
        a.x = __builtin_amdgcn_readlane(a.x, src);
        a.y = __builtin_amdgcn_readlane(a.y, src);
        return __builtin_bit_cast(double, a);
    } else {
        return __shfl(v, src, P);
    }
}

// argmin over (v, id) with ties broken towards the smaller id; carries two
// payload doubles.  Identical result in every lane of the group.
__device__ __forceinline__ void amin_sel(double& v, int& id, double& a, double& b, double ov, int oid, double oa,
                                         double ob) {
    if (ov < v || (ov == v && oid < id)) { v = ov; id = oid; a = oa; b = ob; }
}
template <int CTRL>
__device__ __forceinline__ void amin_dpp(double& v, int& id, double& a, double& b) {
    amin_sel(v, id, a, b, dpp_d<CTRL>(v), dpp_i<CTRL>(id), dpp_d<CTRL>(a), dpp_d<CTRL>(b));
}
template <int S>
__device__ __forceinline__ void amin_pair(double& v, int& id, double& a, double& b) {
    double v0, v1, a0, a1, b0, b1;
    int i0, i1;
    pair_d<S>(v, v0, v1);
    pair_i<S>(id, i0, i1);
    pair_d<S>(a, a0, a1);
    pair_d<S>(b, b0, b1);
    v = v0; id = i0; a = a0; b = b0;
    amin_sel(v, id, a, b, v1, i1, a1, b1);
}
template <int P>
__device__ __forceinline__ void gargmin(double& v, int& id, double& a, double& b) {
    amin_dpp<0xB1>(v, id, a, b);
    amin_dpp<0x4E>(v, id, a, b);
    if constexpr (P >= 8) amin_dpp<0x141>(v, id, a, b);
    if constexpr (P >= 16) amin_dpp<0x140>(v, id, a, b);
    if constexpr (P >= 32) amin_pair<16>(v, id, a, b);
    if constexpr (P >= 64) amin_pair<32>(v, id, a, b);
    v = uni<P>(v);
    id = uni<P>(id);
    a = uni<P>(a);
    b = uni<P>(b);
}
// the same without payloads (same comparison, same tie rule: smaller id)
__device__ __forceinline__ void amin_sel(double& v, int& id, double ov, int oid) {
    if (ov < v || (ov == v && oid < id)) { v = ov; id = oid; }
}
template <int S>
__device__ __forceinline__ void amin_pair(double& v, int& id) {
    double v0, v1;
    int i0, i1;
    pair_d<S>(v, v0, v1);
    pair_i<S>(id, i0, i1);
    v = v0; id = i0;
    amin_sel(v, id, v1, i1);
}
template <int P>
__device__ __forceinline__ void gargmin(double& v, int& id) {
    amin_sel(v, id, dpp_d<0xB1>(v), dpp_i<0xB1>(id));
    amin_sel(v, id, dpp_d<0x4E>(v), dpp_i<0x4E>(id));
    if constexpr (P >= 8) amin_sel(v, id, dpp_d<0x141>(v), dpp_i<0x141>(id));
    if constexpr (P >= 16) amin_sel(v, id, dpp_d<0x140>(v), dpp_i<0x140>(id));
    if constexpr (P >= 32) amin_pair<16>(v, id);
    if constexpr (P >= 64) amin_pair<32>(v, id);
    v = uni<P>(v);
    id = uni<P>(id);
}

}  // namespace ntm
