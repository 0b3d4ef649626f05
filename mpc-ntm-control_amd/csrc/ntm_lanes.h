// ntm_lanes.h — the inline-assembly helpers that run under a narrowed EXEC.  Four
// families, all for the far N = 20 kernels (one scenario per wave, a row, a column
// or a substitution step's unknown on its own lane): the lane-masked accumulation
// of the triangular Gamma passes, the lane-masked lift recursion, the triangular
// substitutions of the echelon re-solve, and the row norms of the scaling pass
// with their non-zero tracking (and, in plain C++ ahead of them, the aligned pair
// loads ld_pair / ld5 of the same kernels).  In each the lanes an
// instruction belongs to are known at compile time, so the instruction runs with
// EXEC narrowed to them where the plain form computes on every lane and selects.
//
// Rules every block (one asm statement) below follows.  The families' comments
// add only what is their own: which lanes own what, why the result has the plain
// form's bits, and what was measured.
//
// 1. EXEC is saved, ANDed into every mask, restored.  The entry EXEC is copied to
//    an SGPR pair (s_mov_b64 at the head of a block; the echelon family saves it
//    once per chain, esub_enter, and hands it to every statement).  Every mask a
//    block installs is ANDed with the saved value, so lanes off on entry stay off
//    whatever the mask says, and EXEC is restored before the statement ends: the
//    compiler never sees it changed.  Only SALU builds the masks (compile-time
//    shifts of -1, literals, an AND with a gate).
// 2. A SALU write of EXEC needs no wait state before a VALU or an LDS instruction:
//    s_and_saveexec followed by a VALU is what the compiler emits for every
//    divergent branch, followed by a ds_write for every predicated store.  The
//    cases for which the ISA lists wait states behind an EXEC write or a
//    VALU-written SGPR (DPP, lane access, v_div_fmas, an EXECZ / VCCZ read) occur
//    in no block: the lane reads of the echelon family are the compiler's, between
//    two statements.  The one exception, a VALU that reads a VALU-written SGPR as
//    a source, is rule 4.
// 3. The end of a block: s_mov_b64 plus s_nop 0.  The compiler's hazard pass does
//    not look into a statement, so it does not see the block's last VALU write.  A
//    DPP read of that VGPR needs two wait states, a v_readlane_b32 one.  The
//    restoring s_mov_b64 is one and the s_nop 0 behind it the second, so whatever
//    the scheduler places next (a DPP or lane read of the result included) is
//    covered.  The echelon statements end with the s_mov_b64 alone; their comment
//    says why one wait state is enough there.
// 4. A VALU-written SGPR.  A VALU write of an SGPR pair needs no wait state before
//    the SALU that reads it (v_cmp then s_and / s_or), but a VALU that reads it as a
//    source needs two, and the compiler does not count them into a statement.  So
//    a block whose VALU takes an SGPR source that a VALU may have written directly
//    ahead of the statement (the v_readlane_b32 broadcast of the echelon steps)
//    opens with its s_and_b64 of EXEC and an s_nop 0 in front of that VALU.
// 5. Memory.  A block that holds an LDS instruction clobbers "memory", which keeps
//    the compiler's own accesses on their side of it; a block of VALU and SALU
//    only does not.  The compiler's wait counts do not include a block's LDS
//    operations.  Stores: LDS operations of one wave complete in order, so a
//    compiler wait for a load issued before or after such a store only waits
//    longer, never too little, and the last storing block of a phase ends with
//    s_waitcnt lgkmcnt(0), so nothing uncounted is in flight behind it.  A VALU
//    write of a VGPR needs no wait state before the LDS store that reads it as
//    data (the interlock the compiler's own v_add, ds_write2 pairs rely on), and a
//    store's data registers may be rewritten at once: the ISA asks for wait states
//    there only after a vector-memory store of more than 64 bits (one or two), LDS
//    stores are not in that list, and the compiler itself rewrites a ds_write2's
//    data one instruction later.  Loads: they and their s_waitcnt lgkmcnt(0) stand
//    in one statement, so no loaded register is visible to the compiler before it
//    has landed.
#pragma once
#include <hip/hip_runtime.h>

#include "ntm_collectives.h"

namespace ntm {

// ---------------------------------------------------------------------------
// Aligned pair loads (the slim far N = 20 kernels, W::kPair).  A lane that reads the
// doubles [2i], [2i+1] of a vector reads 16 contiguous bytes; knowing only that they
// are 8-byte aligned, the backend's load/store optimizer merges the two reads into one
// ds_read2_b64 offset1 = offset0 + 1, which the LDS serves as two accesses of four
// 16-lane groups each: 8 LDS-array cycles for the wave, against 4 for the same bytes
// as one ds_read_b128 (or as two ds_read_b64), and the 16 waves of a CU share one LDS
// pipe.  ld_pair<true> tells the compiler the pair is 16-byte aligned, so it reads it
// with one ds_read_b128; ld_pair<false> is the two plain loads every other kernel had.
//   Preconditions of ld_pair<true>(p): p is 16-byte aligned, i.e. an even number of
// doubles into one of the vectors ws_pair_aligned() (ntm_ws.h) asserts: e, xp, Phi,
// irn, Vb / Uf as one 2N-vector, or a column of the packed Gamma taken at an even row
// (Gt + gidx(2l, l) - 2l + 2i); and the workspace base is 16-byte aligned (the
// dynamic LDS base is, and a one-wave block has one workspace).  Loads only: the same
// bits reach the same arithmetic (tools/lds_read_forms_check.hip compares the three
// forms, full and partial EXEC).  Both doubles must be readable where the plain form
// was predicated per element; every caller reads both or neither.
// ---------------------------------------------------------------------------
typedef double dpair __attribute__((ext_vector_type(2)));
template <int P, class W>
__device__ __forceinline__ constexpr bool pair_ld_ok() {
    return P == 64 && W::kPair;                            // one scenario per wave, N = 20, far, slim
}
template <bool AL>
__device__ __forceinline__ dpair ld_pair(const double* p) {
    if constexpr (AL) {
        return *static_cast<const dpair*>(__builtin_assume_aligned(p, 16));
    } else {
        dpair v;
        v.x = p[0];
        v.y = p[1];
        return v;
    }
}
// x[u] = v[J0 + u], u = 0..4 (a chunk of five consecutive entries at a compile-time offset, the
// same address on every lane).  AL: v is 16-byte aligned, so the chunk holds two aligned
// pairs, from J0 if it is even and from J0 + 1 if not, and one single entry
template <int J0, bool AL>
__device__ __forceinline__ void ld5(const double* v, double (&x)[5]) {
    if constexpr (AL) {
        constexpr int o = J0 & 1;                          // the single entry: the first (odd J0) or the last
        const dpair p0 = ld_pair<true>(v + J0 + o), p1 = ld_pair<true>(v + J0 + o + 2);
        x[o] = p0.x;
        x[o + 1] = p0.y;
        x[o + 2] = p1.x;
        x[o + 3] = p1.y;
        x[o ? 0 : 4] = v[J0 + (o ? 0 : 4)];
    } else {
#pragma unroll
        for (int u = 0; u < 5; ++u) x[u] = v[J0 + u];
    }
}

// ---------------------------------------------------------------------------
// Lane-masked accumulation (N = 20, one scenario per wave, row or column =
// lane).  The triangular passes over the packed Gamma sum N fixed terms per
// lane and zero the ones outside the lane's row or column with a select (two
// v_cndmask and a v_cmp per fp64 term).  The lanes a term belongs to are
// contiguous and known at compile time (lanes >= 2j for the term j of a row
// pass, lanes <= i for the term i of a column pass), so the one accumulating
// instruction runs with EXEC narrowed to them instead: a lane that is off keeps
// its accumulator, which is what y + (+-0) leaves for any y other than -0.0.
//   Row dots (v_fmac_f64; a row's own terms come first, the masked ones after):
// the two forms differ on a lane the term does not belong to when x is not
// finite (NaN from 0 x against y untouched) and when y is -0.0 there (+0.0 from
// -0.0 + 0 against -0.0); never on a lane the term belongs to.
//   Column passes (v_add_f64 of a term formed on every lane; the select form adds
// +0.0, never a product with 0): a column's masked terms come first, onto the
// +0.0 the sum starts from, so no accumulator is -0.0 where a term is masked
// and the two forms are identical, whatever the data.
//   One block per chunk of five terms.  A term's mask costs one scalar instruction
// (round 16; it was s_lshl_b64 / s_lshr_b64 of -1 into an SGPR pair, then the AND):
// the saved EXEC ANDed with a 32-bit literal (lanes <= i, i <= 19) or and-not one (the
// lanes below 2j, 2j <= 32), straight into EXEC (rule 1); the row passes' terms 17..19
// keep the shift and the pair, their term 0 writes no EXEC at all.  The wait states
// are what they were: a SALU write of EXEC needs none before the VALU behind it
// (rule 2), whether it is an s_and_b64 of two SGPR pairs or of a pair and a literal,
// and nothing else of a block changed: the same VALU instructions in the same order,
// the restoring s_mov_b64 and the s_nop 0 at the end (rule 3).  The blocks hold no
// memory instruction (rule 5); the scaling pass's v_cmp_class writes an SGPR pair
// that only an s_or_b64 reads (rule 4).
//   Measured on the far N = 20 kernel at B = 1e5 (A/B on one box, three runs
// each): the row dots 6.057 -> 5.962 ms per step-batch, the certificate's
// gradient and the scaling pass's column pass on top 5.949 -> 5.772 ms; the
// scaling pass's row pass (masked adds of the squares, the last / cnt tracking
// left select-based) 5.762 -> 5.792 ms: not kept.  qdot_rows' callers take the
// column from fidx[], not from the lane, so it keeps its selects.
// ---------------------------------------------------------------------------
template <int P, int CH, class W>
__device__ __forceinline__ constexpr bool lane_masked_ok() {
    // row r / column l sits on lane r / l: one scenario per wave, 2N <= 64, one trip of `r += P`.
    // The far build only: its chunks hold five terms, which is what the asm blocks are written
    // for; the all-LDS builds batch four terms per round trip (ntm_n20near.hip) and run their
    // scaling pass split over idle lanes
    return P == 64 && CH == 5 && W::kNN == 20 && W::kFar;
}
// The masks.  Lanes >= 2j of a row pass: the entry EXEC and-not the lanes below 2j, one
// s_andn2_b64 with a 32-bit literal for 2j <= 32 (a literal of a 64-bit scalar operand is
// zero-extended, so its complement keeps the lanes 32..63); the terms j = 17..19 shift -1 and
// AND, two instructions; term j = 0 belongs to every lane and leaves EXEC as it is (it is
// the first term of its block: EXEC is still the entry EXEC).  Lanes <= i of a column pass,
// i <= 19: one s_and_b64 with the literal (2 << i) - 1.
constexpr unsigned long long lanes_below(int s) { return (1ull << s) - 1ull; }        // lanes 0..s-1
// the literal of a term equals the shift form's mask (s_lshl_b64 / s_lshr_b64 of -1), and fits 32 bits
constexpr bool from_lit_ok(int j) {
    return ~lanes_below(2 * j) == (~0ull << (2 * j)) && lanes_below(2 * j) <= 0xFFFFFFFFull;
}
constexpr bool upto_lit_ok(int i) {
    return lanes_below(i + 1) == (~0ull >> (63 - i)) && lanes_below(i + 1) <= 0xFFFFFFFFull;
}
template <int J0>
constexpr bool from_chunk_ok() {                          // terms J0..J0+4: 2j <= 32 by literal, shifts above
    static_assert(J0 == 0 || J0 == 5 || J0 == 10 || J0 == 15, "chunks of five terms of the N = 20 passes");
    for (int k = 0; k < 5; ++k)
        if (2 * (J0 + k) <= 32 && !from_lit_ok(J0 + k)) return false;
    return true;
}
template <int I0>
constexpr bool upto_chunk_ok() {
    static_assert(I0 >= 0 && I0 + 5 <= 20, "columns 0..19");
    for (int k = 0; k < 5; ++k)
        if (!upto_lit_ok(I0 + k)) return false;
    return true;
}
#define NTM_FROM_ALL(k)                                                                   // every lane: no EXEC write
#define NTM_FROM_LIT(k) "s_andn2_b64 exec, %[sv], %[s" #k "]\n\t"                         // s<k>: the lanes below 2j
#define NTM_FROM_SHL(k) "s_lshl_b64 %[m], -1, %[s" #k "]\n\ts_and_b64 exec, %[sv], %[m]\n\t"   // s<k>: the shift 2j
#define NTM_UPTO_LIT(k) "s_and_b64 exec, %[sv], %[s" #k "]\n\t"                           // s<k>: the lanes <= i
// a chunk's five "n" operands: literals (unsigned long long, so bit 31 prints unsigned); the last
// chunk of a row pass holds the two literals of j = 15, 16 and the three shifts of j = 17..19
#define NTM_LITS_FROM(J0)                                                                                  \
    [s0] "n"(lanes_below(2 * (J0))), [s1] "n"(lanes_below(2 * (J0) + 2)), [s2] "n"(lanes_below(2 * (J0) + 4)), \
        [s3] "n"(lanes_below(2 * (J0) + 6)), [s4] "n"(lanes_below(2 * (J0) + 8))
#define NTM_LITS_FROM_LAST \
    [s0] "n"(lanes_below(30)), [s1] "n"(lanes_below(32)), [s2] "n"(34), [s3] "n"(36), [s4] "n"(38)
#define NTM_LITS_UPTO(I0)                                                                                  \
    [s0] "n"(lanes_below((I0) + 1)), [s1] "n"(lanes_below((I0) + 2)), [s2] "n"(lanes_below((I0) + 3)),     \
        [s3] "n"(lanes_below((I0) + 4)), [s4] "n"(lanes_below((I0) + 5))
#define NTM_V5(n, a) [n##0] "v"(a[0]), [n##1] "v"(a[1]), [n##2] "v"(a[2]), [n##3] "v"(a[3]), [n##4] "v"(a[4])
#define NTM_M_NONE
#define NTM_M_PAIR , [m] "=&s"(m)
// y += g[u] x[u] on lanes >= 2 (J0 + u), u = 0..4 in order, one v_fmac_f64 each
template <int J0>
__device__ __forceinline__ void fmac5_lanes_from(double& y, const double (&g)[5], const double (&x)[5]) {
    static_assert(from_chunk_ok<J0>(), "a term's literal is not its shift form's mask");
    unsigned long long sv;
#define NTM_TERM(M, k) M(k) "v_fmac_f64_e32 %[y], %[g" #k "], %[x" #k "]\n\t"
#define NTM_BLOCK(M0, M1, M2, M3, M4, MOUT, LITS)                                                                    \
    asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_TERM(M0, 0) NTM_TERM(M1, 1) NTM_TERM(M2, 2) NTM_TERM(M3, 3)          \
                 NTM_TERM(M4, 4) "s_mov_b64 exec, %[sv]\n\ts_nop 0"                                                  \
                 : [y] "+v"(y), [sv] "=&s"(sv) MOUT                                                                  \
                 : NTM_V5(g, g), NTM_V5(x, x), LITS                                                                  \
                 : "scc")
    if constexpr (J0 == 0) {
        NTM_BLOCK(NTM_FROM_ALL, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_M_NONE, NTM_LITS_FROM(J0));
    } else if constexpr (J0 == 15) {
        unsigned long long m;
        NTM_BLOCK(NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_SHL, NTM_FROM_SHL, NTM_FROM_SHL, NTM_M_PAIR, NTM_LITS_FROM_LAST);
    } else {
        NTM_BLOCK(NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_M_NONE, NTM_LITS_FROM(J0));
    }
#undef NTM_BLOCK
#undef NTM_TERM
}
// the same for two accumulators that share g and the masks: y1 += g x1, then y2 += g x2, per term
template <int J0>
__device__ __forceinline__ void fmac5x2_lanes_from(double& y1, double& y2, const double (&g)[5],
                                                   const double (&x1)[5], const double (&x2)[5]) {
    static_assert(from_chunk_ok<J0>(), "a term's literal is not its shift form's mask");
    unsigned long long sv;
#define NTM_TERM(M, k) \
    M(k) "v_fmac_f64_e32 %[y1], %[g" #k "], %[a" #k "]\n\tv_fmac_f64_e32 %[y2], %[g" #k "], %[b" #k "]\n\t"
#define NTM_BLOCK(M0, M1, M2, M3, M4, MOUT, LITS)                                                                    \
    asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_TERM(M0, 0) NTM_TERM(M1, 1) NTM_TERM(M2, 2) NTM_TERM(M3, 3)          \
                 NTM_TERM(M4, 4) "s_mov_b64 exec, %[sv]\n\ts_nop 0"                                                  \
                 : [y1] "+v"(y1), [y2] "+v"(y2), [sv] "=&s"(sv) MOUT                                                 \
                 : NTM_V5(g, g), NTM_V5(a, x1), NTM_V5(b, x2), LITS                                                  \
                 : "scc")
    if constexpr (J0 == 0) {
        NTM_BLOCK(NTM_FROM_ALL, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_M_NONE, NTM_LITS_FROM(J0));
    } else if constexpr (J0 == 15) {
        unsigned long long m;
        NTM_BLOCK(NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_SHL, NTM_FROM_SHL, NTM_FROM_SHL, NTM_M_PAIR, NTM_LITS_FROM_LAST);
    } else {
        NTM_BLOCK(NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_FROM_LIT, NTM_M_NONE, NTM_LITS_FROM(J0));
    }
#undef NTM_BLOCK
#undef NTM_TERM
}
// s += t[u] on lanes <= I0 + u (column pass), one v_add_f64 each
template <int I0>
__device__ __forceinline__ void fadd5_lanes_upto(double& s, const double (&t)[5]) {
    static_assert(upto_chunk_ok<I0>(), "a term's literal is not its shift form's mask");
    unsigned long long sv;
#define NTM_TERM(k) NTM_UPTO_LIT(k) "v_add_f64 %[y], %[y], %[t" #k "]\n\t"
    asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_TERM(0) NTM_TERM(1) NTM_TERM(2) NTM_TERM(3) NTM_TERM(4)
                 "s_mov_b64 exec, %[sv]\n\ts_nop 0"
                 : [y] "+v"(s), [sv] "=&s"(sv)
                 : NTM_V5(t, t), NTM_LITS_UPTO(I0)
                 : "scc");
#undef NTM_TERM
}
// The scaling pass's column terms on lanes <= I0 + u: s += t[u], fs += tf[u], and the
// lanes on which g0[u] or g1[u] is an infinity or a NaN ORed into the lane mask nf
// (v_cmp_class under the narrowed EXEC writes zeros for the lanes that are off)
template <int I0>
__device__ __forceinline__ void fadd5x2_class_lanes_upto(double& s, double& fs, unsigned long long& nf,
                                                         const double (&t)[5], const double (&tf)[5],
                                                         const double (&g0)[5], const double (&g1)[5]) {
    static_assert(upto_chunk_ok<I0>(), "a term's literal is not its shift form's mask");
    unsigned long long sv, c;
    const int cls = 0x207;                                // signalling / quiet NaN, -inf, +inf
#define NTM_TERM(k)                                                                                      \
    NTM_UPTO_LIT(k) "v_cmp_class_f64_e64 %[c], %[p" #k "], %[cls]\n\ts_or_b64 %[nf], %[nf], %[c]\n\t"  \
                    "v_cmp_class_f64_e64 %[c], %[q" #k "], %[cls]\n\ts_or_b64 %[nf], %[nf], %[c]\n\t"  \
                    "v_add_f64 %[y], %[y], %[t" #k "]\n\tv_add_f64 %[z], %[z], %[u" #k "]\n\t"
    asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_TERM(0) NTM_TERM(1) NTM_TERM(2) NTM_TERM(3) NTM_TERM(4)
                 "s_mov_b64 exec, %[sv]\n\ts_nop 0"
                 : [y] "+v"(s), [z] "+v"(fs), [nf] "+s"(nf), [sv] "=&s"(sv), [c] "=&s"(c)
                 : NTM_V5(t, t), NTM_V5(u, tf), NTM_V5(p, g0), NTM_V5(q, g1), [cls] "s"(cls), NTM_LITS_UPTO(I0)
                 : "scc");
#undef NTM_TERM
}
#undef NTM_FROM_ALL
#undef NTM_FROM_LIT
#undef NTM_FROM_SHL
#undef NTM_UPTO_LIT
#undef NTM_LITS_FROM
#undef NTM_LITS_FROM_LAST
#undef NTM_LITS_UPTO
#undef NTM_M_NONE
#undef NTM_M_PAIR
#undef NTM_V5

// ---------------------------------------------------------------------------
// Lane-masked lift recursion (the slim far N = 20 lift: Gamma's column l on lane
// l < N, the free response on lane N).  At stage i the lanes that advance are
// known at compile time: columns 0..i-1 (their diagonal lies above row i) and
// lane N, the mask ((1 << i) - 1) | (1 << N).  The select form computes the next
// 2-vector on every lane, selects it or the old one, selects the store index
// (i, or the lane's own diagonal again) and builds the address: a v_cmp, five
// v_cndmask, a v_mov and a v_lshl_add per stage around four fp64 instructions,
// the selects on the chain to the next stage.  Here the four instructions and the
// pair store run with EXEC narrowed to that mask: a lane that is off keeps g0 /
// g1 and stores nothing, where the select form re-stored the same bits to the
// same place, so registers and LDS hold the same bits whatever the data.
//   The arithmetic is the select form's as the production build compiles it, which
// is not one form: the compiler contracts (a21 g0 + a22 g1) + c1 from either
// product, and it does so by the stage's place in its chunk of five.  First and
// last stage of a chunk (form A): t = g0 a21; t = fma(a22, g1, t); g0 = fma(g0,
// a11, c0).  The three between (form B): t = a22 g1; t = fma(a21, g0, t); g0 =
// fma(a11, g0, c0).  Both end g1 = c1 + t.  The two round differently, so each
// stage keeps the form, and the operand order, it had.
//   One block per chunk, the masks literals (rule 1).  a22 is wave-uniform in
// every kernel (an SGPR pair, src0 of the v_fmac / v_mul); c0 / c1 differ between
// the Gamma lanes and lane N: VGPRs.  The stores are in the block (ds_write2_b64
// at rec + 16 i: immediate offsets), so rule 5's store half applies: the last
// chunk is the one that ends with s_waitcnt lgkmcnt(0), and a store's data
// registers are next written by the following stage's v_fma / v_add, three or
// more instructions behind it (s_and, v_mul, v_fmac), or behind the restoring
// s_mov, the s_nop and the next block's s_mov / s_and.  After the block (rule 3):
// the last VALU write (g1) is followed by the store, the restoring s_mov and the
// s_nop 0, more than the two wait states a DPP or lane read of it needs.
//   Measured on the far N = 20 kernel at B = 1e5 (A/B on one box, three runs
// each): 5.804 -> 5.602 ms per step-batch, outputs byte-equal; VALU instructions
// per wave-step 25,977 -> 24,475, the fp64 ones unchanged.
// ---------------------------------------------------------------------------
#define NTM_V5(n, a) [n##0] "v"(a[0]), [n##1] "v"(a[1]), [n##2] "v"(a[2]), [n##3] "v"(a[3]), [n##4] "v"(a[4])
#define NTM_LIFT_MASK(k) "s_and_b64 exec, %[sv], %[m" #k "]\n\t"
#define NTM_LIFT_PUT(k) "ds_write2_b64 %[rec], %[g0], %[g1] offset0:%[o" #k "] offset1:%[p" #k "]\n\t"
#define NTM_LIFT_A(k)                                                                                    \
    NTM_LIFT_MASK(k) "v_mul_f64 %[t], %[g0], %[b" #k "]\n\tv_fmac_f64_e32 %[t], %[a22], %[g1]\n\t"       \
                     "v_fma_f64 %[g0], %[g0], %[a" #k "], %[c0]\n\tv_add_f64 %[g1], %[c1], %[t]\n\t" NTM_LIFT_PUT(k)
#define NTM_LIFT_B(k)                                                                                    \
    NTM_LIFT_MASK(k) "v_mul_f64 %[t], %[a22], %[g1]\n\tv_fmac_f64_e32 %[t], %[b" #k "], %[g0]\n\t"       \
                     "v_fma_f64 %[g0], %[a" #k "], %[g0], %[c0]\n\tv_add_f64 %[g1], %[c1], %[t]\n\t" NTM_LIFT_PUT(k)
#define NTM_LIFT_N(k, I0) \
    [m##k] "n"(((1 << ((I0) + k)) - 1) | (1 << 20)), [o##k] "n"(2 * ((I0) + k)), [p##k] "n"(2 * ((I0) + k) + 1)
// stages I0 .. I0 + NS - 1 (NS = 5, or 4 in the last chunk, which also drains the stores) of
// g <- A_i g + c on the lanes < i and lane 20, each stage's pair stored at rec + 16 i bytes
// (rec: the lane's LDS byte address).  ca / cb: a11 / a21 of the chunk's stages
template <int I0, int NS>
__device__ __forceinline__ void lift_chunk_lanes(double& g0, double& g1, const double (&ca)[5], const double (&cb)[5],
                                                 double a22, double c0, double c1, unsigned rec) {
    static_assert(I0 >= 1 && (NS == 4 || NS == 5) && I0 + NS <= 20, "stages 1..19 of the N = 20 lift");
    unsigned long long sv;
    double t;
    if constexpr (NS == 5) {
        asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_LIFT_A(0) NTM_LIFT_B(1) NTM_LIFT_B(2) NTM_LIFT_B(3) NTM_LIFT_A(4)
                     "s_mov_b64 exec, %[sv]\n\ts_nop 0"
                     : [g0] "+v"(g0), [g1] "+v"(g1), [t] "=&v"(t), [sv] "=&s"(sv)
                     : NTM_V5(a, ca), NTM_V5(b, cb), [a22] "s"(a22), [c0] "v"(c0), [c1] "v"(c1), [rec] "v"(rec),
                       NTM_LIFT_N(0, I0), NTM_LIFT_N(1, I0), NTM_LIFT_N(2, I0), NTM_LIFT_N(3, I0), NTM_LIFT_N(4, I0)
                     : "scc", "memory");
    } else {
        asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_LIFT_A(0) NTM_LIFT_B(1) NTM_LIFT_B(2) NTM_LIFT_B(3)
                     "s_mov_b64 exec, %[sv]\n\ts_waitcnt lgkmcnt(0)"
                     : [g0] "+v"(g0), [g1] "+v"(g1), [t] "=&v"(t), [sv] "=&s"(sv)
                     : [a0] "v"(ca[0]), [a1] "v"(ca[1]), [a2] "v"(ca[2]), [a3] "v"(ca[3]), [b0] "v"(cb[0]),
                       [b1] "v"(cb[1]), [b2] "v"(cb[2]), [b3] "v"(cb[3]), [a22] "s"(a22), [c0] "v"(c0), [c1] "v"(c1),
                       [rec] "v"(rec), NTM_LIFT_N(0, I0), NTM_LIFT_N(1, I0), NTM_LIFT_N(2, I0), NTM_LIFT_N(3, I0)
                     : "scc", "memory");
    }
}
#undef NTM_LIFT_MASK
#undef NTM_LIFT_PUT
#undef NTM_LIFT_A
#undef NTM_LIFT_B
#undef NTM_LIFT_N
#undef NTM_V5

// ---------------------------------------------------------------------------
// Lane-masked triangular substitutions of the echelon re-solve (the slim far
// N = 20 kernels: the sorted E packed in LDS, row t at Ep + t(t+1)/2, n <= 20
// rows, one scenario per wave).  Forward (E V = h, and E Z = -e_c with it when
// k = 1): lane l owns row l, step t forms x_t = acc_t / E_tt on lane t, takes it
// by two v_readlane_b32 and subtracts E_lt x_t on the rows below.  Backward (E'
// mu = grad): lane l owns column l, the steps descend from u = n - 1 and update
// the columns l < u.  The loop form does every step on every lane: a select
// captures x on the lane l == t (a v_cmp, two v_mov, two v_cndmask per right-hand
// side), the element load sits under a saved EXEC with a branch and its wait
// directly in front of the fma, the address is rebuilt per step.  Here the steps
// are unrolled over the compile-time t in batches of five: a batch's five
// elements are loaded first (ds_read_b64 at immediate offsets from one per-lane
// address, each under EXEC = the lanes that will use it: t < l < n forward, l < u
// backward, so nothing past a row's diagonal is read), waited for once, and
// the five chain steps follow without an LDS wait.  Per step and right-hand
// side: one v_mul_f64 (acc sq_id, written straight into x under EXEC = lanes t <=
// l < n: lane t's x is final after step t because the later steps exclude it, so
// there is no select), the two v_readlane_b32 (the compiler's, between two
// statements: v_readlane ignores EXEC, and a statement cannot name the halves of
// a 64-bit operand), one v_fma_f64 under EXEC = lanes t < l < n.
//   Bit-equality with the loop form, whatever the data: a lane l <= t there goes
// on computing acc -= 0 x_t after its x was captured, and a lane >= n does so from
// the start; neither acc is read again, by the loop or behind it.  x (zz, mu) of a
// lane < n is the same product acc sq_id of the same chain (v_mul_f64 with sq_id as
// src0; v_fma_f64 with the negated element as src0, the broadcast as src1: the
// operands, and so the NaN a non-finite step propagates, as the loop form was
// compiled); lanes >= n and lanes off on entry keep what they held (0.0 in the
// kernel).  A step t >= n inside a batch runs with an empty EXEC (the masks are ANDed
// with the lanes < n); backward a step u >= n would pass `lanes <= u`, so each
// step's masks are ANDed with a gate that is the entry EXEC if u < n and 0 if not
// (SALU, only in the batch the chain enters through).
//   The masks are 32-bit literals with bit 31 clear (n <= 20), ANDed with the
// entry EXEC that esub_enter saved, which every statement restores before it ends
// (rule 1).  v_mul_f64's result is read by v_readlane_b32 (one wait state): the
// restoring s_mov_b64 stands between them in every statement (rule 3).  The
// v_readlane's SGPR result feeds the v_fma_f64 as a source, and the v_readlane_b32
// may be the last thing ahead of the statement, so each step's s_and_b64 is
// followed by an s_nop 0 (rule 4).  A batch's loads and their wait are one
// statement (rule 5); the steps hold no memory instruction.
//   Measured on the far N = 20 kernel at B = 1e5 (A/B on one box, three runs
// each): the forward substitution 5.592 -> 5.495 ms per step-batch, the backward
// one on top 5.490 -> 5.405 ms, outputs byte-equal; VALU instructions per wave-
// step 24,475 -> 23,419.
// ---------------------------------------------------------------------------
template <int P, int CH, class W>
__device__ __forceinline__ constexpr bool esub_lanes_ok() {
    if constexpr (W::kSlim) return lane_masked_ok<P, CH, W>();
    else return false;
}
struct LaneExec {
    unsigned long long sv;                                // EXEC on entry
    unsigned long long mb;                                // its lanes below n
};
__device__ __forceinline__ LaneExec esub_enter(int n) {   // n wave-uniform, 0..20
    LaneExec x;
    const unsigned long long low = (1ull << n) - 1ull;
    asm volatile("s_mov_b64 %[sv], exec\n\ts_and_b64 %[mb], exec, %[lo]"
                 : [sv] "=&s"(x.sv), [mb] "=&s"(x.mb)
                 : [lo] "s"(low)
                 : "scc");
    return x;
}
constexpr unsigned esub_ge(int t) { return 0xFFFFFu & ~((1u << t) - 1u); }   // lanes t..19
constexpr unsigned esub_gt(int t) { return 0xFFFFFu & ~((2u << t) - 1u); }   // lanes t+1..19
constexpr unsigned esub_le(int u) { return (2u << u) - 1u; }                 // lanes 0..u
constexpr unsigned esub_lt(int u) { return (1u << u) - 1u; }                 // lanes 0..u-1
#define NTM_ESUB_LD(k) "s_and_b64 exec, %[mk], %[m" #k "]\n\tds_read_b64 %[e" #k "], %[at] offset:%[o" #k "]\n\t"
// forward batch T0..T0+4: the five loads E[l][T0 + k] (lanes > T0 + k below n), step T0's product(s), one wait
template <int T0, bool TWO>
__device__ __forceinline__ void fsub_open(double (&e)[5], double acc, double& x, double acz, double& zz, double sq,
                                          unsigned row, const LaneExec& c) {
    static_assert(T0 >= 0 && T0 + 5 <= 20, "steps 0..19");
    if constexpr (TWO) {
        asm volatile(NTM_ESUB_LD(0) NTM_ESUB_LD(1) NTM_ESUB_LD(2) NTM_ESUB_LD(3) NTM_ESUB_LD(4)
                     "s_and_b64 exec, %[mk], %[ge]\n\tv_mul_f64 %[x], %[sq], %[acc]\n\tv_mul_f64 %[z], %[sq], %[acz]\n\t"
                     "s_waitcnt lgkmcnt(0)\n\ts_mov_b64 exec, %[sv]"
                     : [e0] "=&v"(e[0]), [e1] "=&v"(e[1]), [e2] "=&v"(e[2]), [e3] "=&v"(e[3]), [e4] "=&v"(e[4]),
                       [x] "+v"(x), [z] "+v"(zz)
                     : [acc] "v"(acc), [acz] "v"(acz), [sq] "v"(sq), [at] "v"(row), [mk] "s"(c.mb), [sv] "s"(c.sv),
                       [ge] "n"(esub_ge(T0)), [m0] "n"(esub_gt(T0)), [m1] "n"(esub_gt(T0 + 1)), [m2] "n"(esub_gt(T0 + 2)),
                       [m3] "n"(esub_gt(T0 + 3)), [m4] "n"(esub_gt(T0 + 4)), [o0] "n"(8 * T0), [o1] "n"(8 * (T0 + 1)),
                       [o2] "n"(8 * (T0 + 2)), [o3] "n"(8 * (T0 + 3)), [o4] "n"(8 * (T0 + 4))
                     : "scc", "memory");
    } else {
        asm volatile(NTM_ESUB_LD(0) NTM_ESUB_LD(1) NTM_ESUB_LD(2) NTM_ESUB_LD(3) NTM_ESUB_LD(4)
                     "s_and_b64 exec, %[mk], %[ge]\n\tv_mul_f64 %[x], %[sq], %[acc]\n\t"
                     "s_waitcnt lgkmcnt(0)\n\ts_mov_b64 exec, %[sv]"
                     : [e0] "=&v"(e[0]), [e1] "=&v"(e[1]), [e2] "=&v"(e[2]), [e3] "=&v"(e[3]), [e4] "=&v"(e[4]),
                       [x] "+v"(x)
                     : [acc] "v"(acc), [sq] "v"(sq), [at] "v"(row), [mk] "s"(c.mb), [sv] "s"(c.sv),
                       [ge] "n"(esub_ge(T0)), [m0] "n"(esub_gt(T0)), [m1] "n"(esub_gt(T0 + 1)), [m2] "n"(esub_gt(T0 + 2)),
                       [m3] "n"(esub_gt(T0 + 3)), [m4] "n"(esub_gt(T0 + 4)), [o0] "n"(8 * T0), [o1] "n"(8 * (T0 + 1)),
                       [o2] "n"(8 * (T0 + 2)), [o3] "n"(8 * (T0 + 3)), [o4] "n"(8 * (T0 + 4))
                     : "scc", "memory");
    }
}
// forward step T: acc -= E[l][T] x_T on lanes > T, then (NEXT) step T + 1's product(s) on lanes >= T + 1,
// the same lanes: one mask
template <int T, bool TWO, bool NEXT>
__device__ __forceinline__ void fsub_step(double et, double& acc, double& x, double& acz, double& zz, double sq,
                                          const LaneExec& c) {
    const double xt = gbcast<64>(x, T);
    if constexpr (TWO) {
        const double zt = gbcast<64>(zz, T);
        if constexpr (NEXT)
            asm volatile("s_and_b64 exec, %[mk], %[gt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                         "v_fma_f64 %[acz], -%[e], %[zt], %[acz]\n\t"
                         "v_mul_f64 %[x], %[sq], %[acc]\n\tv_mul_f64 %[z], %[sq], %[acz]\n\ts_mov_b64 exec, %[sv]"
                         : [acc] "+v"(acc), [acz] "+v"(acz), [x] "+v"(x), [z] "+v"(zz)
                         : [e] "v"(et), [xt] "s"(xt), [zt] "s"(zt), [sq] "v"(sq), [mk] "s"(c.mb), [sv] "s"(c.sv),
                           [gt] "n"(esub_gt(T))
                         : "scc");
        else if constexpr (esub_gt(T) != 0)
            asm volatile("s_and_b64 exec, %[mk], %[gt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                         "v_fma_f64 %[acz], -%[e], %[zt], %[acz]\n\ts_mov_b64 exec, %[sv]"
                         : [acc] "+v"(acc), [acz] "+v"(acz)
                         : [e] "v"(et), [xt] "s"(xt), [zt] "s"(zt), [mk] "s"(c.mb), [sv] "s"(c.sv), [gt] "n"(esub_gt(T))
                         : "scc");
    } else {
        if constexpr (NEXT)
            asm volatile("s_and_b64 exec, %[mk], %[gt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                         "v_mul_f64 %[x], %[sq], %[acc]\n\ts_mov_b64 exec, %[sv]"
                         : [acc] "+v"(acc), [x] "+v"(x)
                         : [e] "v"(et), [xt] "s"(xt), [sq] "v"(sq), [mk] "s"(c.mb), [sv] "s"(c.sv),
                           [gt] "n"(esub_gt(T))
                         : "scc");
        else if constexpr (esub_gt(T) != 0)
            asm volatile("s_and_b64 exec, %[mk], %[gt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                         "s_mov_b64 exec, %[sv]"
                         : [acc] "+v"(acc)
                         : [e] "v"(et), [xt] "s"(xt), [mk] "s"(c.mb), [sv] "s"(c.sv), [gt] "n"(esub_gt(T))
                         : "scc");
    }
}
template <int T0, bool TWO>
__device__ __forceinline__ void fsub_batch(double& acc, double& x, double& acz, double& zz, double sq, unsigned row,
                                           const LaneExec& c) {
    double e[5];
    fsub_open<T0, TWO>(e, acc, x, acz, zz, sq, row, c);
    fsub_step<T0, TWO, true>(e[0], acc, x, acz, zz, sq, c);
    fsub_step<T0 + 1, TWO, true>(e[1], acc, x, acz, zz, sq, c);
    fsub_step<T0 + 2, TWO, true>(e[2], acc, x, acz, zz, sq, c);
    fsub_step<T0 + 3, TWO, true>(e[3], acc, x, acz, zz, sq, c);
    fsub_step<T0 + 4, TWO, false>(e[4], acc, x, acz, zz, sq, c);
}
// E x = acc (TWO: and E zz = acz) for the lanes < n of the entry EXEC; row: the LDS byte address of
// the lane's row of the packed E, sq: 1 / E[l][l].  n wave-uniform; the chain leaves at a batch boundary
template <bool TWO>
__device__ __forceinline__ void fsub_lanes(int n, double& acc, double& x, double& acz, double& zz, double sq,
                                           unsigned row) {
    const LaneExec c = esub_enter(n);
    if (n > 0) fsub_batch<0, TWO>(acc, x, acz, zz, sq, row, c);
    if (n > 5) fsub_batch<5, TWO>(acc, x, acz, zz, sq, row, c);
    if (n > 10) fsub_batch<10, TWO>(acc, x, acz, zz, sq, row, c);
    if (n > 15) fsub_batch<15, TWO>(acc, x, acz, zz, sq, row, c);
}
// backward batch U0+4 .. U0 (descending): the loads E[u][l] (lanes < u), step U0 + 4's product, one wait.
// g: the gate of step U0 + 4 (the entry EXEC, or 0 if the step lies at or above n)
template <int U0>
__device__ __forceinline__ void bsub_open(double (&e)[5], double acc, double& mu, double sq, unsigned col,
                                          unsigned long long g, const LaneExec& c) {
    static_assert(U0 >= 0 && U0 + 5 <= 20, "steps 19..0");
    constexpr int o0 = 4 * (U0 + 4) * (U0 + 5), o1 = 4 * (U0 + 3) * (U0 + 4), o2 = 4 * (U0 + 2) * (U0 + 3),
                  o3 = 4 * (U0 + 1) * (U0 + 2), o4 = 4 * U0 * (U0 + 1);           // 8 u (u + 1) / 2 bytes
    asm volatile(NTM_ESUB_LD(0) NTM_ESUB_LD(1) NTM_ESUB_LD(2) NTM_ESUB_LD(3) NTM_ESUB_LD(4)
                 "s_and_b64 exec, %[g], %[le]\n\tv_mul_f64 %[x], %[sq], %[acc]\n\t"
                 "s_waitcnt lgkmcnt(0)\n\ts_mov_b64 exec, %[sv]"
                 : [e0] "=&v"(e[0]), [e1] "=&v"(e[1]), [e2] "=&v"(e[2]), [e3] "=&v"(e[3]), [e4] "=&v"(e[4]), [x] "+v"(mu)
                 : [acc] "v"(acc), [sq] "v"(sq), [at] "v"(col), [mk] "s"(c.sv), [sv] "s"(c.sv), [g] "s"(g),
                   [le] "n"(esub_le(U0 + 4)), [m0] "n"(esub_lt(U0 + 4)), [m1] "n"(esub_lt(U0 + 3)),
                   [m2] "n"(esub_lt(U0 + 2)), [m3] "n"(esub_lt(U0 + 1)), [m4] "n"(esub_lt(U0)), [o0] "n"(o0),
                   [o1] "n"(o1), [o2] "n"(o2), [o3] "n"(o3), [o4] "n"(o4)
                 : "scc", "memory");
}
#undef NTM_ESUB_LD
// backward step U: acc -= E[U][l] mu_U on lanes < U under the step's gate g, then (NEXT) step U - 1's product
// on lanes <= U - 1 (the same lanes) under its gate gn
template <int U, bool NEXT, bool GATED>
__device__ __forceinline__ void bsub_step(double eu, double& acc, double& mu, double sq, unsigned long long g,
                                          unsigned long long gn, const LaneExec& c) {
    const double mu_u = gbcast<64>(mu, U);
    if constexpr (NEXT && U > 0 && !GATED)               // both gates are the entry EXEC: one mask
        asm volatile("s_and_b64 exec, %[g], %[lt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                     "v_mul_f64 %[x], %[sq], %[acc]\n\ts_mov_b64 exec, %[sv]"
                     : [acc] "+v"(acc), [x] "+v"(mu)
                     : [e] "v"(eu), [xt] "s"(mu_u), [sq] "v"(sq), [g] "s"(g), [sv] "s"(c.sv), [lt] "n"(esub_lt(U))
                     : "scc");
    else if constexpr (NEXT && U > 0)
        asm volatile("s_and_b64 exec, %[g], %[lt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                     "s_and_b64 exec, %[gn], %[le]\n\tv_mul_f64 %[x], %[sq], %[acc]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [acc] "+v"(acc), [x] "+v"(mu)
                     : [e] "v"(eu), [xt] "s"(mu_u), [sq] "v"(sq), [g] "s"(g), [gn] "s"(gn), [sv] "s"(c.sv),
                       [lt] "n"(esub_lt(U)), [le] "n"(esub_le(U > 0 ? U - 1 : 0))
                     : "scc");
    else if constexpr (U > 0)
        asm volatile("s_and_b64 exec, %[g], %[lt]\n\ts_nop 0\n\tv_fma_f64 %[acc], -%[e], %[xt], %[acc]\n\t"
                     "s_mov_b64 exec, %[sv]"
                     : [acc] "+v"(acc)
                     : [e] "v"(eu), [xt] "s"(mu_u), [g] "s"(g), [sv] "s"(c.sv), [lt] "n"(esub_lt(U))
                     : "scc");
}
template <int U0, bool GATED>
__device__ __forceinline__ void bsub_batch(int n, double& acc, double& mu, double sq, unsigned col, const LaneExec& c) {
    double e[5];
    auto gate = [&](int u) -> unsigned long long { return (!GATED || u < n) ? c.sv : 0ull; };
    bsub_open<U0>(e, acc, mu, sq, col, gate(U0 + 4), c);
    bsub_step<U0 + 4, true, GATED>(e[0], acc, mu, sq, gate(U0 + 4), gate(U0 + 3), c);
    bsub_step<U0 + 3, true, GATED>(e[1], acc, mu, sq, gate(U0 + 3), gate(U0 + 2), c);
    bsub_step<U0 + 2, true, GATED>(e[2], acc, mu, sq, gate(U0 + 2), gate(U0 + 1), c);
    bsub_step<U0 + 1, true, GATED>(e[3], acc, mu, sq, gate(U0 + 1), gate(U0), c);
    bsub_step<U0, false, GATED>(e[4], acc, mu, sq, gate(U0), 0ull, c);
}
// E' mu = acc for the lanes < n of the entry EXEC; col: the LDS byte address of E[0][l] (Ep + l), sq: 1 /
// E[l][l].  The batch that holds step n - 1 is gated per step, the ones below it are not
template <int U0>
__device__ __forceinline__ void bsub_from(int n, double& acc, double& mu, double sq, unsigned col, const LaneExec& c) {
    if (n > U0) {
        if (n >= U0 + 5) bsub_batch<U0, false>(n, acc, mu, sq, col, c);
        else bsub_batch<U0, true>(n, acc, mu, sq, col, c);
    }
}
__device__ __forceinline__ void bsub_lanes(int n, double& acc, double& mu, double sq, unsigned col) {
    const LaneExec c = esub_enter(n);
    bsub_from<15>(n, acc, mu, sq, col, c);
    bsub_from<10>(n, acc, mu, sq, col, c);
    bsub_from<5>(n, acc, mu, sq, col, c);
    bsub_from<0>(n, acc, mu, sq, col, c);
}

// ---------------------------------------------------------------------------
// Lane-masked row norms of the scaling pass (the slim far N = 20 kernels: state
// row r on lane r < 2N, |Gamma_r D|^2 = sum_j (Gamma_rj D_j)^2 over j <= r / 2, and
// with it the row's last non-zero column and the count of its non-zeros).  The
// loop form runs all N terms on every lane: it zeroes the square of a term outside
// the row with a select (a v_cmp and two v_cndmask), ANDs the row test into the
// non-zero test, tracks last / cnt by selects (a v_mov, two v_cndmask and half a
// v_add3 per term) and rebuilds the packed address per term (an s_mul, two s_add
// and a v_lshl_add).  Here the terms are unrolled over the compile-time j in
// chunks of five: gt(r, j) sits at Gt + r + j (2N - 1 - j), an immediate offset
// from the lane's address of Gt[r], D_j at an immediate offset from D, and term j
// runs with EXEC narrowed to the lanes 2j .. 2N - 1.  Per term: v_cmp_neq_f64 (the
// non-zero test, VCC), the two v_mul_f64 and the v_add_f64 of the loop form as it
// is compiled (g D_j with g as src0, the square, s + square; no contraction),
// v_cndmask_b32 last <- j under VCC and v_addc_co_u32 cnt += VCC.
//   Bit-equality with the loop form, whatever the data: the sum starts at +0.0 and
// adds squares (each +0.0 or above, or a NaN) in ascending j, so it is never -0.0,
// and a row's masked terms (j > r / 2) come after its own: s + (+0.0) leaves the
// bits of any such s, a quiet NaN included, which is what a lane that is off
// keeps.  last and cnt change only on a lane the term belongs to, under the same
// test (v_cmp_neq is true for a NaN, false for -0.0, as `g != 0.0`).  Lanes off on
// entry and lanes >= 2N are in no mask (rule 1) and keep s, last and cnt.
//   One block per chunk.  Its ten loads are issued first, under the chunk's widest
// mask (lanes >= 2 J0 below 2N: gt(r, j) of such a lane lies inside the packed
// Gamma for any j), and term k waits for its own pair (LDS loads return in order:
// lgkmcnt(8 - 2k)); loads and waits are one statement (rule 5).  A chunk's first
// mask is s_bfm_b64 (40 - 2j ones from bit 2j) ANDed with the saved EXEC.  The masks
// of a chunk are nested (term j + 1's lanes are term j's without the lanes 2j and
// 2j + 1), so a later term narrows the EXEC it finds by one s_andn2_b64 with the
// literal of the lanes below its 2j (2j <= 32: a 32-bit literal, zero-extended; round
// 16); the terms 17..19 build theirs by s_bfm_b64 as before.  VCC written by
// v_cmp is read as a mask by v_cndmask and as a carry by v_addc: two wait states
// (rule 4), which the two v_mul_f64 between them are, in the order the compiler
// itself schedules this pair (v_cmp, two VALU, v_cndmask).  v_addc's carry-out
// overwrites VCC, which the next term's v_cmp writes again; VCC is a clobber.  The
// block ends by rule 3.
//   Round 8 had masked only the add of this pass and kept the select-based tracking
// and the per-term address arithmetic (5.762 -> 5.792 ms, not kept; above).  This
// form, measured on the far N = 20 kernel at B = 1e5 (A/B on one box, three runs
// each): 5.261-5.269 -> 5.182-5.197 ms per step-batch, outputs byte-equal
// (DESIGN.md section 10, round 14).
// ---------------------------------------------------------------------------
#define NTM_RN_LD(k) \
    "ds_read_b64 %[g" #k "], %[at] offset:%[o" #k "]\n\tds_read_b64 %[d" #k "], %[ad] offset:%[q" #k "]\n\t"
#define NTM_RN_MASK(k) "s_bfm_b64 %[m], %[w" #k "], %[b" #k "]\n\ts_and_b64 exec, %[sv], %[m]\n\t"
#define NTM_RN_NARROW(k) "s_andn2_b64 exec, exec, %[n" #k "]\n\t"    // n<k>: the lanes below 2j, a 32-bit literal
#define NTM_RN_TERM(k, cntk)                                                                          \
    "s_waitcnt lgkmcnt(" #cntk ")\n\tv_cmp_neq_f64_e32 vcc, 0, %[g" #k "]\n\tv_mul_f64 %[v], %[g" #k "], %[d" #k "]\n\t"                \
    "v_mul_f64 %[v], %[v], %[v]\n\tv_cndmask_b32_e64 %[last], %[last], %[j" #k "], vcc\n\t"          \
    "v_addc_co_u32_e32 %[cnt], vcc, 0, %[cnt], vcc\n\tv_add_f64 %[s], %[s], %[v]\n\t"
#define NTM_RN_N(k, J0)                                                                               \
    [w##k] "n"(40 - 2 * ((J0) + k)), [b##k] "n"(2 * ((J0) + k)), [j##k] "n"((J0) + k),                \
        [n##k] "n"(lanes_below(2 * ((J0) + k) <= 32 ? 2 * ((J0) + k) : 0)),                           \
        [o##k] "n"(8 * ((J0) + k) * (39 - ((J0) + k))), [q##k] "n"(8 * ((J0) + k))
// terms J0 .. J0 + 4 of row `lane`: at / ad the LDS byte addresses of Gt[lane] and of D[0]
template <int J0>
__device__ __forceinline__ void rownorm5_lanes_from(double& s, int& last, int& cnt, unsigned at, unsigned ad) {
    static_assert(from_chunk_ok<J0>(), "a term's literal is not the mask of the lanes below 2j");
    unsigned long long sv, m;
    double g0, g1, g2, g3, g4, d0, d1, d2, d3, d4, v;
    // M1..M4: how terms 1..4 come by their lanes: NTM_RN_NARROW from the term before, or NTM_RN_MASK
#define NTM_RN_BLOCK(M1, M2, M3, M4)                                                                                \
    asm volatile("s_mov_b64 %[sv], exec\n\t" NTM_RN_MASK(0)                                                         \
                 NTM_RN_LD(0) NTM_RN_LD(1) NTM_RN_LD(2) NTM_RN_LD(3) NTM_RN_LD(4) NTM_RN_TERM(0, 8)                  \
                 M1(1) NTM_RN_TERM(1, 6) M2(2) NTM_RN_TERM(2, 4) M3(3) NTM_RN_TERM(3, 2) M4(4) NTM_RN_TERM(4, 0)     \
                 "s_mov_b64 exec, %[sv]\n\ts_nop 0"                                                                 \
                 : [s] "+v"(s), [last] "+v"(last), [cnt] "+v"(cnt), [v] "=&v"(v), [sv] "=&s"(sv), [m] "=&s"(m),     \
                   [g0] "=&v"(g0), [g1] "=&v"(g1), [g2] "=&v"(g2), [g3] "=&v"(g3), [g4] "=&v"(g4),                  \
                   [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2), [d3] "=&v"(d3), [d4] "=&v"(d4)                   \
                 : [at] "v"(at), [ad] "v"(ad), NTM_RN_N(0, J0), NTM_RN_N(1, J0), NTM_RN_N(2, J0), NTM_RN_N(3, J0),  \
                   NTM_RN_N(4, J0)                                                                                  \
                 : "scc", "vcc", "memory")
    if constexpr (J0 == 15) {                             // j = 16 by literal, j = 17..19 (bits 34..39) by s_bfm_b64
        NTM_RN_BLOCK(NTM_RN_NARROW, NTM_RN_MASK, NTM_RN_MASK, NTM_RN_MASK);
    } else {
        NTM_RN_BLOCK(NTM_RN_NARROW, NTM_RN_NARROW, NTM_RN_NARROW, NTM_RN_NARROW);
    }
#undef NTM_RN_BLOCK
}
#undef NTM_RN_LD
#undef NTM_RN_MASK
#undef NTM_RN_NARROW
#undef NTM_RN_TERM
#undef NTM_RN_N

}  // namespace ntm
