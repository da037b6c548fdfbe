"""The S-box of the FP64 Poseidon2 (csrc/poseidon2_f64.cuh: x^7 in 19 operations, x^3 and x^4 reduced only to a multiple
of 2^12 p and 2^6 p) on the host: IEEE doubles and fma() are the arithmetic the kernels run.  Every bound that the
header states for the S-box is asserted here on the largest magnitudes the check meets over its whole input range."""
import pytest

from dvt_circuits_amd import capi

P = 2013265921
# the header's bounds (sbox in poseidon2_f64.cuh)
X2_MAX = 0.5004 * P
X3_MAX = (2.0 ** 12 + 2.0 ** -16) * P
X4_MAX = (2.0 ** 6 + 2.0 ** -16) * P
SBOX_OUT = 0.573 * P
N_EDGE = 4001 * (2 * 17 + 73 + 145)


@pytest.fixture(scope="module")
def runs():
    return {seed: capi.p2_f64_sbox_check(10_000_000, seed) for seed in (1, 2)}


@pytest.mark.parametrize("seed", [1, 2])
def test_sbox_is_x7_over_its_input_range(runs, seed):
    bad, _ = runs[seed]
    assert bad == 0, f"{bad} of {10_000_000 + N_EDGE} inputs differ from x^7 mod p"


@pytest.mark.parametrize("seed", [1, 2])
def test_sbox_intermediates_within_stated_bounds(runs, seed):
    _, (x2, x3, x4, x7) = runs[seed]
    print(f"seed {seed}: max |x2| = {x2 / P:.6f} p, |x3| = {x3 / P:.6f} p, |x4| = {x4 / P:.6f} p, |x7| = {x7 / P:.6f} p")
    assert 0 < x2 <= X2_MAX
    assert 0 < x3 <= X3_MAX
    assert 0 < x4 <= X4_MAX
    assert 0 < x7 <= SBOX_OUT
    # what the last product needs (mm_pre: 15 q < 2^53), from the stated bounds and from the maxima met
    assert X3_MAX * X4_MAX < 2.0 ** 80
    assert x3 * x4 < 2.0 ** 80
    # what the partial products need: (q / 2^K) p < 2^53 with |q| <= |a b| / p + 2^(K - 1)
    assert (X2_MAX * 36 * P / P / 2 ** 13 + 0.5) * P < 2.0 ** 53
    assert (X2_MAX * X2_MAX / P / 2 ** 7 + 0.5) * P < 2.0 ** 53


def test_permutation_matches_integer_one():
    assert capi.p2_f64_selfcheck(300000, 7) == 0
