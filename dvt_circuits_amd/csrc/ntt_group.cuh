// The arithmetic of one radix-8 group of the K1 register passes (ntt.hip: dif_pass2 and dit_pass2 of lde_block2_kernel, C = 2
// trace columns per work item): three butterfly stages on eight values per column, in the FP64 formulation of
// poseidon2_f64.cuh.  Host-callable: IEEE doubles and fma() behave the same there, so dvt_debug_ntt_group_check
// (tests/test_ntt_group_host.py) runs THIS source against integer arithmetic mod p and asserts every bound stated below on
// the largest magnitudes it meets.
//
// A product whose result feeds only the next stage's butterfly need not be reduced to (-p, p): stages 0 and 1 use
// p2f::mm_c<K> (3 operations: reduced to a multiple of 2^K p), stage 2 keeps p2f::mm_pre (5 operations), and the sums
// are reduced once (p2f::red, 3 operations) on the way out.  Per group and column that is 12 butterflies of
//   DIF  2 (a + b, a - b) + product:  4 x 5 + 4 x 5 + 4 x 7 + 4 red x 3 =  80 operations  (all mm_pre: 96)
//   DIT  product + 2:                 4 x 5 + 4 x 5 + 4 x 7 + 8 red x 3 =  92 operations  (all mm_pre: 108)
// and with UNIT (the group's twiddle exponents are (j mod dist) << (stage bits): zero for j mod dist = 0, which is 1 + 2
// + 4 = 7 of the 12 butterflies when the pass has one row per group element) those seven products are not computed:
//   DIF, unit                         (8 + 3 x 3) + (8 + 2 x 3) + 4 x 5 + 12   =  63 operations.
//
// Magnitudes (p = 2^30.907; twiddles are centred residues, |w| <= (p - 1)/2 = 2^29.907; a granularity K that is one
// smaller makes q p of mm_c inexact at these magnitudes, one larger pushes a later product past its limit):
//   DIF  in      |v| <= DIF_IN = p                 (raw words of [0, p), or what a pass wrote: <= 0.52 p)
//        stage 0 |a - b| <= 2 p = 2^31.907, |(a - b) w| <= 2^61.814 <= 2^(52.99 + 9)
//                                                  -> mm_c<9>:  <= (2^8 + 2^-16) p  = DIF_S0 = 2^38.907; sums <= 2 p
//        stage 1 |a - b| <= 2 DIF_S0 = 2^39.907, |(a - b) w| <= 2^69.814 <= 2^(52.99 + 17)
//                                                  -> mm_c<17>: <= (2^16 + 2^-16) p = DIF_S1 = 2^46.907; sums <= 2^39.907
//        stage 2 |a - b| <= 2 DIF_S1 = 2^47.907, |(a - b) w| <= 2^77.814 < 2^80
//                                                  -> mm_pre:   <= 0.52 p = OUT_MAX (0.5 + 2^(77.814 - 30.907) PINV_REL)
//                sums <= 2 DIF_S1 < 2^48           -> red:      <= p/2 + 1
//        unit    a difference that skips its product is smaller than the product's bound (2 p, 2 DIF_S0); in stage 2
//                it is reduced: |a - b| < 2^48     -> red:      <= p/2 + 1
//   DIT  in      |v| <= DIT_IN = 0.52 p = OUT_MAX  (what the scaling step or a pass wrote)
//        stage 0 |v w| <= 0.26 p^2 = 2^59.871 <= 2^(52.99 + 7)
//                                                  -> mm_c<7>:  <= (2^6 + 2^-16) p;  a +- b <= DIT_S0 = 64.53 p = 2^36.919
//        stage 1 |v w| <= DIT_S0 p/2 = 2^66.826 <= 2^(52.99 + 14)
//                                                  -> mm_c<14>: <= (2^13 + 2^-16) p; a +- b <= DIT_S1 = 8256.6 p = 2^43.919
//        stage 2 |v w| <= DIT_S1 p/2 = 2^73.826 < 2^80
//                                                  -> mm_pre:   <= 0.502 p;          a +- b <= DIT_S2 = 8257.2 p < 2^44
//                                                  -> red:      <= p/2 + 1
// Everything a pass stores is at most OUT_MAX = 0.52 p < 2^31: it fits the int32 LDS tile.
#pragma once
#include "poseidon2_f64.cuh"

namespace dvt {
namespace ntg {

constexpr int DIF_K0 = 9, DIF_K1 = 17, DIT_K0 = 7, DIT_K1 = 14;
constexpr double TW_MAX = (p2f::PD - 1.0) / 2.0;
constexpr double OUT_MAX = 0.52 * p2f::PD;
constexpr double DIF_IN = p2f::PD;
constexpr double DIF_S0 = (256.0 + 1.0 / 65536.0) * p2f::PD;       // a stage-0 product
constexpr double DIF_S1 = (65536.0 + 1.0 / 65536.0) * p2f::PD;     // a stage-1 product
constexpr double DIT_IN = OUT_MAX;
constexpr double DIT_S0 = (64.0 + 1.0 / 65536.0) * p2f::PD + DIT_IN;      // a value after stage 0
constexpr double DIT_S1 = (8192.0 + 1.0 / 65536.0) * p2f::PD + DIT_S0;    // after stage 1
constexpr double DIT_S2 = 0.502 * p2f::PD + DIT_S1;                       // after stage 2 (before red)

// What the host check records (slot, |value|); the kernels pass nothing and the calls vanish.
//   DIF: 0/2/4 = |a - b| of stage 0/1/2, 1/3/5 = what that stage puts in its place (product, or the unit form),
//        6 = a sum before red, 7 = an output.
//   DIT: 0/2/4 = the factor v of stage 0/1/2, 1/3/5 = its product, 6 = a value before red, 7 = an output.
struct NoProbe {
    DVT_HD void operator()(int, double) const {}
};

// Twiddles of a DIF group: w[0..3] stage 0 (butterfly j, j + 4), w[4..5] stage 1 (j mod 2), w[6] stage 2; wp = w * PINV.
// UNIT: w[0], w[4] and w[6] are 1 and are not read.
template <int C, bool UNIT, class Probe = NoProbe>
DVT_HD void dif_group(double (&v)[8][C], const double (&w)[7], const double (&wp)[7], Probe probe = Probe()) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], d = a - v[j + 4][c];
            v[j][c] = a + v[j + 4][c];
            v[j + 4][c] = (UNIT && j == 0) ? d : p2f::mm_c<DIF_K0>(d, w[j], wp[j]);
            probe(0, d); probe(1, v[j + 4][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & 2) continue;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], d = a - v[j + 2][c];
            v[j][c] = a + v[j + 2][c];
            v[j + 2][c] = (UNIT && !(j & 1)) ? d : p2f::mm_c<DIF_K1>(d, w[4 + (j & 1)], wp[4 + (j & 1)]);
            probe(2, d); probe(3, v[j + 2][c]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], d = a - v[j + 1][c], s = a + v[j + 1][c];
            v[j][c] = p2f::red(s);
            v[j + 1][c] = UNIT ? p2f::red(d) : p2f::mm_pre(d, w[6], wp[6]);
            probe(4, d); probe(5, v[j + 1][c]); probe(6, s); probe(7, v[j][c]); probe(7, v[j + 1][c]);
        }
    }
}

// Twiddles of a DIT group: w[0] stage 0, w[1..2] stage 1 (j mod 2), w[3..6] stage 2 (j mod 4); wp = w * PINV.
template <int C, class Probe = NoProbe>
DVT_HD void dit_group(double (&v)[8][C], const double (&w)[7], const double (&wp)[7], Probe probe = Probe()) {
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], b = p2f::mm_c<DIT_K0>(v[j + 1][c], w[0], wp[0]);
            probe(0, v[j + 1][c]); probe(1, b);
            v[j][c] = a + b;
            v[j + 1][c] = a - b;
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
        if (j & 2) continue;
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], b = p2f::mm_c<DIT_K1>(v[j + 2][c], w[1 + (j & 1)], wp[1 + (j & 1)]);
            probe(2, v[j + 2][c]); probe(3, b);
            v[j][c] = a + b;
            v[j + 2][c] = a - b;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int c = 0; c < C; c++) {
            const double a = v[j][c], b = p2f::mm_pre(v[j + 4][c], w[3 + j], wp[3 + j]);
            probe(4, v[j + 4][c]); probe(5, b);
            const double s = a + b, d = a - b;
            probe(6, s); probe(6, d);
            v[j][c] = p2f::red(s);
            v[j + 4][c] = p2f::red(d);
            probe(7, v[j][c]); probe(7, v[j + 4][c]);
        }
    }
}

}  // namespace ntg
}  // namespace dvt
