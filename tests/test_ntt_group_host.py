"""The radix-8 group arithmetic of the K1 register passes (csrc/ntt_group.cuh: the products of stages 0 and 1 reduced only
to a multiple of 2^K p, the products by the twiddle 1 skipped in the last DIF pass) on the host: IEEE doubles and fma() are
the arithmetic the kernels run, and the header is the source they run.  Every bound that the header states is asserted here
on the largest magnitudes the check meets, and the stated bounds are checked against what each product form needs."""
import math

import pytest

from dvt_circuits_amd import capi

P = 2013265921
N = 300_000
# the header's bounds (ntt_group.cuh)
TW_MAX = (P - 1) / 2
OUT_MAX = 0.52 * P
DIF_IN = float(P)
DIF_K0, DIF_K1, DIT_K0, DIT_K1 = 9, 17, 7, 14
DIF_S0 = (2.0 ** 8 + 2.0 ** -16) * P
DIF_S1 = (2.0 ** 16 + 2.0 ** -16) * P
DIT_IN = OUT_MAX
DIT_S0 = (2.0 ** 6 + 2.0 ** -16) * P + DIT_IN
DIT_S1 = (2.0 ** 13 + 2.0 ** -16) * P + DIT_S0
DIT_S2 = 0.502 * P + DIT_S1
# groups of the edge grid: 3 kinds x (1 + 4 x 256 sign patterns) x (64 + 8) twiddle sets
N_GRID = 3 * (1 + 4 * 256) * 72


@pytest.fixture(scope="module")
def runs():
    return {seed: capi.ntt_group_check(N, seed) for seed in (1, 2)}


@pytest.mark.parametrize("seed", [1, 2])
def test_groups_match_integer_arithmetic(runs, seed):
    bad, _ = runs[seed]
    assert bad == 0, f"{bad} of {(3 * N + N_GRID) * 16} outputs are not congruent to the integer butterflies"


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("kind", ["dif", "dif_unit"])
def test_dif_magnitudes_within_stated_bounds(runs, seed, kind):
    d0, p0, d1, p1, d2, p2, pre, out = runs[seed][1][kind]
    print(f"seed {seed} {kind}: |a-b| 2^{math.log2(d0):.3f} 2^{math.log2(d1):.3f} 2^{math.log2(d2):.3f}; products "
          f"2^{math.log2(p0):.3f} 2^{math.log2(p1):.3f} {p2 / P:.4f} p; sum before red 2^{math.log2(pre):.3f}; output {out / P:.4f} p")
    assert 0 < d0 <= 2 * DIF_IN and 0 < p0 <= DIF_S0
    assert 0 < d1 <= 2 * DIF_S0 and 0 < p1 <= DIF_S1
    assert 0 < d2 <= 2 * DIF_S1 and 0 < p2 <= OUT_MAX
    assert 0 < pre <= 2 * DIF_S1
    assert 0 < out <= OUT_MAX
    # the magnitudes met satisfy what each product form needs (mm_c<K>: |a b| <= 2^(52.99 + K); mm_pre: < 2^80)
    assert d0 * TW_MAX <= 2.0 ** (52.99 + DIF_K0)
    assert d1 * TW_MAX <= 2.0 ** (52.99 + DIF_K1)
    assert d2 * TW_MAX < 2.0 ** 80
    assert pre < 2.0 ** 48 and d2 < 2.0 ** 48


@pytest.mark.parametrize("seed", [1, 2])
def test_dit_magnitudes_within_stated_bounds(runs, seed):
    f0, b0, f1, b1, f2, b2, pre, out = runs[seed][1]["dit"]
    print(f"seed {seed} dit: factors {f0 / P:.4f} p 2^{math.log2(f1):.3f} 2^{math.log2(f2):.3f}; products "
          f"2^{math.log2(b0):.3f} 2^{math.log2(b1):.3f} {b2 / P:.4f} p; before red 2^{math.log2(pre):.3f}; output {out / P:.4f} p")
    assert 0 < f0 <= DIT_IN and 0 < b0 <= DIT_S0 - DIT_IN
    assert 0 < f1 <= DIT_S0 and 0 < b1 <= DIT_S1 - DIT_S0
    assert 0 < f2 <= DIT_S1 and 0 < b2 <= DIT_S2 - DIT_S1
    assert 0 < pre <= DIT_S2
    assert 0 < out <= OUT_MAX
    assert f0 * TW_MAX <= 2.0 ** (52.99 + DIT_K0)
    assert f1 * TW_MAX <= 2.0 ** (52.99 + DIT_K1)
    assert f2 * TW_MAX < 2.0 ** 80
    assert pre < 2.0 ** 48


def test_stated_bounds_satisfy_the_product_forms():
    # DIF: |a - b| <= twice the larger operand of the stage, |w| <= TW_MAX
    assert 2 * DIF_IN * TW_MAX <= 2.0 ** (52.99 + DIF_K0)
    assert 2 * DIF_S0 * TW_MAX <= 2.0 ** (52.99 + DIF_K1)
    assert 2 * DIF_S1 * TW_MAX < 2.0 ** 80
    assert 2 * DIF_S1 < 2.0 ** 48                       # what red takes with a slack far below 1
    # mm_pre leaves (1/2 + |a b| / p * PINV_REL) p
    pinv_rel = 1.3718e-16
    assert (0.5 + 2 * DIF_S1 * TW_MAX / P * pinv_rel) * P <= OUT_MAX
    # DIT
    assert DIT_IN * TW_MAX <= 2.0 ** (52.99 + DIT_K0)
    assert DIT_S0 * TW_MAX <= 2.0 ** (52.99 + DIT_K1)
    assert DIT_S1 * TW_MAX < 2.0 ** 80
    assert (0.5 + DIT_S1 * TW_MAX / P * pinv_rel) * P <= 0.502 * P
    assert DIT_S2 < 2.0 ** 48
    # a granularity one smaller would not do: the product bound of the stage exceeds 2^(52.99 + K - 1)
    assert 2 * DIF_IN * TW_MAX > 2.0 ** (52.99 + DIF_K0 - 1) and 2 * DIF_S0 * TW_MAX > 2.0 ** (52.99 + DIF_K1 - 1)
    assert DIT_IN * TW_MAX > 2.0 ** (52.99 + DIT_K0 - 1) and DIT_S0 * TW_MAX > 2.0 ** (52.99 + DIT_K1 - 1)
    # whatever goes back to the int32 LDS tile (p/2 + 1 after red, OUT_MAX after mm_pre), and what the passes read from it
    assert P / 2 + 1 <= OUT_MAX < 2.0 ** 31 and DIF_IN < 2.0 ** 31 and DIT_IN < 2.0 ** 31
