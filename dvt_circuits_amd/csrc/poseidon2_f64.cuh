// Poseidon2 (the permutation of poseidon2.cuh, bit for bit) for the gfx950 hashing kernels, computed on the
// FP64 pipe instead of the integer multiplier.
//
// Why: v_mul_lo/hi_u32 issue at quarter rate on gfx950 and a Montgomery product needs three of them, which
// bounds the integer permutation at about 4.5 Gperm/s per GPU (measured, tools/microbench).  v_fma_f64 issues at
// full rate, a modular product costs three to six FP64 operations and additions need no reduction at all.  (No
// MFMA: nothing here is a contraction.)
//
// How: a field element is an INTEGER carried in a double, congruent mod p to the value, of bounded magnitude
// ("lazy").  Integers below 2^53 are exact in a double, an FMA rounds once, so every step below is exact integer
// arithmetic as long as the stated bounds hold; they are stated at each function and the whole permutation is
// compared with the integer one over 2^24 states by tools/microbench/p2_f64_bench.hip and by the GPU parity
// tests (Merkle roots and proof bytes against the CPU oracle).
//   mm(a, b):  h = RN(a b), l = a b - h (exact, one FMA), q = round(h / p), r = (h - q p) + l.
//              Needs |a b| < 2^82 (q < 2^51 for the rounding trick).  |r| <= p/2 + |h| 2^-52 + |l| < 0.51 p
//              for |a b| < 2^76.
// HBM keeps Montgomery words (bb.cuh); from_mont / to_mont convert at the edges (one product each).
#pragma once
#include <math.h>
#include "bb.cuh"
#include "poseidon2_rc.inc"

namespace dvt {
namespace p2f {

// (host-callable as well: IEEE doubles and fma() behave the same there, which is how the CPU test suite checks
// this file against the integer permutation without a GPU)
#if defined(__HIP_DEVICE_COMPILE__)
#define DVT_F64_TABLE static __constant__ const
#else
#define DVT_F64_TABLE static const
#endif
#define DVT_DEV DVT_HD
DVT_F64_TABLE double RC_EXT[128] = DVT_P2_RC_EXT_F64_INIT;
DVT_F64_TABLE double RC_INT[13] = DVT_P2_RC_INT_F64_INIT;
DVT_F64_TABLE double DIAG[16] = DVT_P2_DIAG_F64_INIT;

constexpr double PD = 2013265921.0;
constexpr double PINV = 1.0 / 2013265921.0;
constexpr double MONT_R = 268435454.0;        // 2^32 mod p
constexpr double MONT_RINV = 943718400.0;     // 2^-32 mod p

// round(a * b) for |a b| < 2^51 in two full-rate operations: the fused multiply-add a * b + 1.5 * 2^52 is rounded once, at
// unit precision (its result lies in [2^52, 2^53)), i.e. to the nearest integer; subtracting the constant is exact.
// (v_mul_f64 + v_rndne_f64 is the same instruction count and measures the same within 1 %.)  Every quotient estimate
// below is such a rounded product; an estimate off by one only moves the representative by p, inside the stated bounds.
// Instruction budget of one permutation: 141 S-boxes of 19 operations (sbox below) + 141 round-constant additions
// + 1 294 operations of the linear layers and reductions = 4 114 FP64 operations in the source.  The gfx950 ISA of the
// bare kernel's loop (tools/microbench, which reduces the state once more per call) has 4 274 FP64 instructions among
// 4 989 vector ones (119 of them v_mov_b64); at four issue cycles per wave64 instruction that is 20.0 k cycles per wave,
// and 8.05 Gperm/s measured is 19.5 k at the nominal 2.4 GHz: the permutation is issue-bound.
// 210 of those vector instructions are v_readlane_b32: the loop keeps the 141 round constants live across iterations, they
// do not fit the SGPRs and are parked in VGPR lanes.  permute_in_loop (below) fetches them inside the iteration instead:
// 4 565 vector instructions, no SGPR spills, 8.77 Gperm/s (profiles/r13_p2_microbench.txt).
constexpr double MAGIC = 6755399441055744.0;  // 1.5 * 2^52
DVT_DEV double rnd_prod(double a, double b) { return fma(a, b, MAGIC) - MAGIC; }
DVT_DEV double mm(double a, double b) {
    double h = a * b;
    double l = fma(a, b, -h);
    double q = rnd_prod(h, PINV);
    return fma(-q, PD, h) + l;
}
// |a| < 2^51  ->  the representative in [-p/2, p/2] (+- a rounding slack far below 1 for |a| < 2^48)
DVT_DEV double red(double a) { return fma(-rnd_prod(a, PINV), PD, a); }

DVT_DEV double from_canonical(uint32_t c) { return (double)c; }
// r in (-p, p) -> canonical word
DVT_DEV uint32_t fix(double r) { return (uint32_t)(r < 0.0 ? r + PD : r); }
DVT_DEV uint32_t to_canonical(double x) { return fix(red(x)); }       // |x| < 2^48

// a * b mod p with bp = b / p (rounded) supplied: q = round(a * bp), then a b - q p = (a b - q (p - 1)) - q, where
// q (p - 1) = 15 q * 2^27 is exact in a double and the FMA result (the integer r + q, |r + q| < 2^50) is exact: 5 operations, no error
// term.  Needs 15 q < 2^53, which |a b| < 2^80 gives (2^80 / p < 2^53 / 15 because 15 * 2^27 < p).  With
// bp = RN(b * PINV) the estimate a * bp is a b / p (1 + e), |e| <= PINV_REL, so |r| <= (1/2 + |a b| / p * PINV_REL) p:
// 0.5004 p for |a b| <= 2^72.2, 0.573 p for |a b| <= 2^79.82.  Worth it where one bp serves several products.
constexpr double P_MINUS_1 = 2013265920.0;
// relative error of RN(b * PINV) against b / p: 2^-53 of the product's rounding + 2^-55.08 (the error of PINV itself, a
// property of this p) and their product: below 2^-52.69
constexpr double PINV_REL = 1.3718e-16;
DVT_DEV double mm_pre(double a, double b, double bp) {
    const double q = rnd_prod(a, bp);
    return fma(a, b, -(q * P_MINUS_1)) - q;
}
DVT_DEV double from_mont(uint32_t m) { return mm_pre((double)m, MONT_RINV, MONT_RINV / PD); }
DVT_DEV uint32_t to_mont(double x) { return fix(mm_pre(x, MONT_R, MONT_R / PD)); }      // |x| < 2^48
// a * b reduced only to a multiple of 2^K p, in 3 operations, for products whose result feeds one more product and
// nothing else.  bp = b / p as for mm_pre.  Adding MK = 1.5 * 2^(52+K) rounds the quotient estimate at unit 2^K:
// qm = MK + q with q a multiple of 2^K, |q - a bp| <= 2^(K-1) (needs |q| < 2^(51+K)).  qm p - MK p = q p is one FMA
// and exact when q p is representable, i.e. (q / 2^K) p < 2^53; MK p = 3 p 2^(51+K) is (3 p < 2^33).  The last FMA
// yields the integer a b - q p, below 2^53: exact.
//   Needs |a b| / p (1 + PINV_REL) + 2^(K-1) <= 2^(53+K) / p, which |a b| <= 2^(52.99+K) gives.
//   |r| <= (2^(K-1) + |a b| / p * PINV_REL) p  <=  (2^(K-1) + 2^-16) p  under that precondition.
// (mm_pre cannot take this route: at K = 0 the product q p has up to 80 bits, hence its detour over q (p - 1).)
template <int K>
DVT_DEV double mm_c(double a, double b, double bp) {
    constexpr double MK = 1.5 * (double)(1ull << 52) * (double)(1ull << K);
    constexpr double MKP = MK * PD;
    const double qm = fma(a, bp, MK);
    const double t = fma(qm, PD, -MKP);
    return fma(a, b, -t);
}

// x^7 in 19 operations (1 + 5 + 3 + 1 + 3 + 1 + 5): x^3 and x^4 feed only the last product and are reduced partially.
//   in : |x| <= SBOX_IN = 36 p (2^36.08)
//   x2 : |x x| <= 1296 p^2 = 2^72.16                          ->  |x2| <= 0.5004 p = 2^29.908        (mm_pre)
//   x3 : |x2 x| <= 0.5004 * 36 p^2 = 2^65.985 <= 2^65.99      ->  |x3| <= (2^12 + 2^-16) p = 2^42.907  (mm_c<13>)
//   x4 : |x2 x2| <= 0.2505 p^2 = 2^59.817 <= 2^59.99          ->  |x4| <= (2^6 + 2^-16) p = 2^36.907   (mm_c<7>)
//   out: |x3 x4| <= (2^18 + 2^-3) p^2 = 2^79.814 < 2^80       ->  |x7| <= SBOX_OUT = 0.573 p (2^30.10) (mm_pre)
// The granularities are not free: K = 14 for x3 or K = 8 for x4 puts the last product beyond 2^80, K = 12 / K = 6 makes
// q p of the partial product inexact at these magnitudes.  dvt_debug_p2_f64_sbox_check compares this function with x^7 mod p
// in integer arithmetic over the whole input range and reports the largest intermediates (tests/test_p2_f64_sbox_host.py).
constexpr double SBOX_IN = 36.0 * PD;
constexpr double SBOX_OUT = 0.573 * PD;
DVT_DEV double sbox_steps(double x, double &x2, double &x3, double &x4) {
    const double xp = x * PINV;
    x2 = mm_pre(x, x, xp);
    x3 = mm_c<13>(x2, x, xp);
    x4 = mm_c<7>(x2, x2, x2 * PINV);
    return mm_pre(x3, x4, x4 * PINV);
}
DVT_DEV double sbox(double x) {
    double x2, x3, x4;
    return sbox_steps(x, x2, x3, x4);
}

// max |s| = B  ->  <= 35 B
DVT_DEV void external_layer(double s[16]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        // circ(2,3,1,1) in 9 operations: y0 = 2x0+3x1+x2+x3, y1 = x0+2x1+3x2+x3, y2 = x0+x1+2x2+3x3, y3 = 3x0+x1+x2+2x3
        const double x0 = s[4 * c], x1 = s[4 * c + 1], x2 = s[4 * c + 2], x3 = s[4 * c + 3];
        const double t01 = x0 + x1, t23 = x2 + x3, t = t01 + t23;
        const double u = t + x1, v = t + x3;          // x0+2x1+x2+x3,  x0+x1+x2+2x3
        s[4 * c + 0] = u + t01;
        s[4 * c + 1] = fma(2.0, x2, u);
        s[4 * c + 2] = v + t23;
        s[4 * c + 3] = fma(2.0, x0, v);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        double sum = (s[k] + s[4 + k]) + (s[8 + k] + s[12 + k]);
#pragma unroll
        for (int c = 0; c < 4; c++) s[4 * c + k] += sum;
    }
}

// y_i = sum + d_i x_i, d = [-2, 1, 2, 3, 4, -3, -4, 5, -5, 6, -6, 7, 8, -8, 9, -1] (tools/gen_poseidon2_rc.py): one fused
// multiply-add per entry, exact.  max |s| = B (< 2^48) -> <= 25 B.
template <bool REDUCE>
DVT_DEV void internal_layer(double s[16]) {
    if (REDUCE) {
#pragma unroll
        for (int i = 1; i < 16; i++) s[i] = red(s[i]);
    }
    double sum = s[0];
#pragma unroll
    for (int i = 1; i < 16; i++) sum += s[i];
    s[0] = fma(-2.0, s[0], sum);
    s[1] = sum + s[1];
    s[2] = fma(2.0, s[2], sum);
    s[3] = fma(3.0, s[3], sum);
    s[4] = fma(4.0, s[4], sum);
    s[5] = fma(-3.0, s[5], sum);
    s[6] = fma(-4.0, s[6], sum);
    s[7] = fma(5.0, s[7], sum);
    s[8] = fma(-5.0, s[8], sum);
    s[9] = fma(6.0, s[9], sum);
    s[10] = fma(-6.0, s[10], sum);
    s[11] = fma(7.0, s[11], sum);
    s[12] = fma(8.0, s[12], sum);
    s[13] = fma(-8.0, s[13], sum);
    s[14] = fma(9.0, s[14], sum);
    s[15] = sum - s[15];
}

// in: |s_i| <= p (canonical words, from_mont results or a previous output; NOT any 32-bit word: the first S-box layer
// needs 35 |s_i| + p/2 <= SBOX_IN); out: |s_i| < 0.51 p (reduced).
// Magnitudes (round constants are centred, |rc| < p/2):
//   first layer           35 p + p/2 = 35.5 p                                        <= SBOX_IN
//   external rounds       an S-box layer leaves SBOX_OUT = 0.573 p, the external layer multiplies by 35: 20.06 p
//                         (2^35.24); with the round constant 20.6 p                  <= SBOX_IN
//   internal rounds       s[0] is reduced before each S-box (|red + rc| <= p), the other entries at r = 2, 5, 8, 11:
//                         20.06 p -> x25 -> 502 p (2^39.9) -> x25 -> 12 540 p (2^44.6) -> reduce; from a reduced
//                         state (s[0] <= 0.573 p, the others <= p/2) 14.4 p (2^34.8) -> 2^39.4 -> 2^44.1 -> reduce;
//                         all below 2^48 as red and the sums need.  After r = 12: 2^39.4, then every entry reduced.
//   last external rounds  |red + rc| <= p for the first, then as above; the final red leaves |s_i| <= p/2 + 2^-8.
DVT_DEV void permute_rc(double s[16], const double *rc_ext, const double *rc_int) {
    external_layer(s);
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox(s[i] + rc_ext[16 * r + i]);
        external_layer(s);
    }
#pragma unroll
    for (int r = 0; r < 13; r++) {
        s[0] = sbox(red(s[0]) + rc_int[r]);
        if (r == 2 || r == 5 || r == 8 || r == 11) internal_layer<true>(s); else internal_layer<false>(s);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = red(s[i]);
#pragma unroll
    for (int r = 4; r < 8; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox(s[i] + rc_ext[16 * r + i]);
        external_layer(s);
    }
#pragma unroll
    for (int i = 0; i < 16; i++) s[i] = red(s[i]);
}
DVT_DEV void permute(double s[16]) { permute_rc(s, RC_EXT, RC_INT); }

#if defined(__HIPCC__)
// ---- the same permutation for a kernel that runs it INSIDE a loop (the row sponge, the two passes of an injected level) ----
// With the tables named directly the compiler hoists all 141 round constants out of the loop, runs out of SGPRs, parks
// them in VGPR lanes and fetches each one back with a v_readlane_b32 in every iteration (222 SGPR spills, 222 readlanes
// among the 4 892 vector instructions of the leaf kernel's sponge loop).  Here the tables are addressed through a wave-uniform
// offset of zero that the compiler cannot see through and must assume changed by every iteration: the constants are
// fetched inside the iteration with scalar loads (17 s_load_dwordx16, which issue beside the vector instructions) and
// live in SGPRs only while their round runs.  (Hiding the POINTER instead loses its address space: flat loads.  An LDS
// table measures the same on the bare permutation, 8.79 against 8.77 Gperm/s, and takes 8 more VGPRs there, 76 against 68:
// the leaf kernel would pass the 80 of six waves per SIMD.)
// merkle_leaves_kernel: 76 VGPRs, -5.0 % time alone on the GPU; merkle_level_kernel<true>: 72 VGPRs.
__device__ __forceinline__ void permute_in_loop(double s[16]) {
    uint32_t off = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(off));
#endif
    permute_rc(s, RC_EXT + off, RC_INT + off);
}

// ---- the same permutation, one state per 16 LANES (lane e of a DPP row holds state element e) ---------------------
// A thread that owns a whole state runs ~5 600 FP64 operations back to back: ~9 us however few states there are, which
// is what the small Merkle levels and every tree top cost per level.  Spread over a DPP row the S-boxes of a round run
// in parallel and the linear layers become quad permutes / row rotations (v_mov_b32_dpp, no LDS): ~1 000 dependent
// operations per permutation.  Used where there are too few states to fill the machine anyway (merkle.hip).
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
constexpr int DPP_QUAD_NEXT = 0x39;   // quad_perm [1,2,3,0]: lane k reads lane k+1 of its quad
constexpr int DPP_QUAD_XOR1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;   // quad_perm [2,3,0,1]
constexpr int DPP_ROW_ROR = 0x120;    // + n: rotate the 16-lane row by n

struct CoopConsts {
    double rc[8];   // external round constants of this lane's element
    double diag;    // internal diagonal entry of this lane's element (centred residue)
    bool lane0;
};
__device__ __forceinline__ CoopConsts coop_consts(uint32_t e) {
    CoopConsts k;
#pragma unroll
    for (int r = 0; r < 8; r++) k.rc[r] = RC_EXT[16 * r + e];
    k.diag = DIAG[e];
    k.lane0 = e == 0;
    return k;
}
// max |s| = B -> <= 35 B (as external_layer)
__device__ __forceinline__ double coop_external_layer(double x) {
    const double x1 = dpp_mov<DPP_QUAD_NEXT>(x);
    double t = x + dpp_mov<DPP_QUAD_XOR1>(x);
    t = t + dpp_mov<DPP_QUAD_XOR2>(t);
    const double y = fma(2.0, x1, t + x);
    double a = y + dpp_mov<DPP_ROW_ROR + 8>(y);
    a = a + dpp_mov<DPP_ROW_ROR + 4>(a);
    return y + a;
}
// in: |s| <= p; out: |s| < 0.51 p (every lane of the row must be active).  The external rounds are those of permute;
// the internal rounds reduce every entry every round, so each S-box sees |s + rc| <= p.
__device__ __forceinline__ double coop_permute(double s, const CoopConsts &k) {
    s = coop_external_layer(s);
#pragma unroll
    for (int r = 0; r < 4; r++) s = coop_external_layer(sbox(s + k.rc[r]));
    s = red(s);
#pragma unroll
    for (int r = 0; r < 13; r++) {
        const double x = sbox(s + RC_INT[r]);
        s = k.lane0 ? x : s;
        double t = s + dpp_mov<DPP_ROW_ROR + 8>(s);
        t = t + dpp_mov<DPP_ROW_ROR + 4>(t);
        t = t + dpp_mov<DPP_ROW_ROR + 2>(t);
        t = t + dpp_mov<DPP_ROW_ROR + 1>(t);
        // every diagonal entry is a small integer and s is reduced: the fused multiply-add is exact
        s = red(fma(s, k.diag, t));                      // every entry stays reduced: |t| <= 15 p/2 + SBOX_OUT, |s diag| <= 9 p/2
    }
#pragma unroll
    for (int r = 4; r < 8; r++) s = coop_external_layer(sbox(s + k.rc[r]));
    return red(s);
}
#endif

}  // namespace p2f
}  // namespace dvt
