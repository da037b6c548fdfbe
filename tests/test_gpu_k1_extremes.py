"""GPU parity tests (run with -m gpu on an MI355X) of the K1 register passes at the columns whose words are the largest
there are: the radix-8 groups of lde_block2_kernel keep the products of their first two stages only partially reduced and
skip the products by the twiddle 1 (csrc/ntt_group.cuh), and their exactness rests on magnitude bounds that constant and
square-wave columns of the largest word press hardest; ntt_strided_v4_kernel around it sees the same columns.  Integer work:
every comparison is exact.

Shapes, by launch_coset_lde's dispatch (test_gpu_commit_dispatch.py names the constants):
  log_n 12   lde_block2_kernel alone, log_n1 = 0: the raw words go into the tile
  log_n 13   the smallest size with strided passes: the four-step twiddles on load and store
  log_n 21   the one size of ntt_strided_v4_kernel (closed forms instead of the oracle, which is too slow there)
  width 2, 4 column pairs; width 3 the odd last column (lde_block_kernel) beside a pair
The tiles hold Montgomery words, so each pattern comes twice: with the canonical value P - 1 and with the value whose
Montgomery word is P - 1.  Random full columns against the oracle are test_gpu_stage_parity.py's and
test_gpu_commit_dispatch.py's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921
MONT_RINV = 943718400                      # 2^-32 mod P: the value c with Montgomery word w is w * MONT_RINV
INV2 = (P + 1) // 2


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


# (stage calls run on the prover's stream, torch on its own: see test_gpu_commit_dispatch.py)
def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def filled(words, value=0):
    import torch

    t = torch.full((words,), value, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint32)


def lde_shift(log_n, shift_mode):
    return {0: 31, 1: 1, 2: pow(pow(31, (P - 1) >> (log_n + 1), P), -1, P)}[shift_mode]


def gpu_lde(gpu, m, log_n, shift_mode):
    width = m.shape[0]
    t_in = dev(m)
    t_out = filled(width << (log_n + 1))
    gpu.to_internal(t_in)
    gpu.coset_lde(t_in, t_out, width, log_n, shift_mode)
    gpu.from_internal(t_out)
    gpu.sync()
    return host(t_out).reshape(width, -1)


def with_word(w):
    """the canonical value whose Montgomery word (what the LDS tile holds) is w"""
    return w * MONT_RINV % P


HIGH = [P - 1, with_word(P - 1)]


def pattern_columns(log_n):
    """(names, [columns][N]): all 0; all high; square waves high / 0 of half-period h, for the h that are the pair
    distances of the first stage of a register pass (4, 32, 256, N/2 for the DIF passes of a 2^12 block, 1, 8, 64, 512 for
    the DIT ones) - there the first butterflies see |a - b| = high; (p + 1)/2 and (p - 1)/2 alternating."""
    n = 1 << log_n
    i = np.arange(n)
    names, cols = ["zero"], [np.zeros(n, np.uint32)]
    for hi in HIGH:
        names.append(f"all {hi}")
        cols.append(np.full(n, hi, np.uint32))
        for h in (1, 4, 8, 32, 64, 256, 512, n // 2):
            names.append(f"{hi} / 0, half-period {h}")
            cols.append(np.where((i // h) & 1, 0, hi).astype(np.uint32))
    for a, b in (((P + 1) // 2, (P - 1) // 2), (with_word((P + 1) // 2), with_word((P - 1) // 2))):
        names.append(f"{a} / {b} alternating")
        cols.append(np.where(i & 1, b, a).astype(np.uint32))
    return names, np.stack(cols)


@pytest.fixture(scope="module")
def patterns(oracle):
    """the pattern columns and their oracle LDE per (log_n, shift_mode): computed once, shared by the widths, never changed"""
    cache = {}

    def get(log_n, shift_mode):
        key = (log_n, shift_mode)
        if key not in cache:
            names, m = pattern_columns(log_n)
            want = oracle.coset_lde(m, 1, lde_shift(log_n, shift_mode))
            m.setflags(write=False)
            want.setflags(write=False)
            cache[key] = (names, m, want)
        return cache[key]

    return get


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("shift_mode", [0, 1, 2])
@pytest.mark.parametrize("log_n", [12, 13])
def test_extreme_columns_against_oracle(gpu, patterns, log_n, shift_mode, width):
    names, m, want = patterns(log_n, shift_mode)
    ncols = m.shape[0]
    # every column, `width` at a time (the last call wraps round to the first columns)
    for c0 in range(0, ncols, width):
        sel = [(c0 + k) % ncols for k in range(width)]
        got = gpu_lde(gpu, m[sel], log_n, shift_mode)
        for k, c in enumerate(sel):
            bad = np.nonzero(got[k] != want[c])[0]
            assert bad.size == 0, (f"log_n {log_n}, shift_mode {shift_mode}, width {width}, column '{names[c]}' (slot {k}): {bad.size} of "
                                   f"{got.shape[1]} outputs differ, first at {int(bad[0])}: {int(got[k, bad[0]])} != {int(want[c, bad[0]])}")


LOG_BIG = 21


@pytest.fixture(scope="module")
def big_columns():
    """[constant, square wave high / 0 = A + B (-1)^i, random, random + square wave] at 2^21 rows"""
    n = 1 << LOG_BIG
    rng = np.random.default_rng(2113)
    hi = HIGH[1]
    a = b = hi * INV2 % P                                  # A + B = high, A - B = 0
    wave = np.where(np.arange(n) & 1, 0, hi).astype(np.uint32)
    rnd = rng.integers(0, P, n, dtype=np.uint32)
    both = ((rnd.astype(np.uint64) + wave) % P).astype(np.uint32)
    m = np.stack([np.full(n, P - 1, np.uint32), wave, rnd, both])
    m.setflags(write=False)
    return m, a, b


@pytest.mark.parametrize("width", [2, 3, 4])
@pytest.mark.parametrize("shift_mode", [0, 1, 2])
def test_closed_forms_and_linearity_at_2_21(gpu, big_columns, shift_mode, width):
    m, a, b = big_columns
    n = 1 << LOG_BIG
    sel = {2: [0, 1], 3: [1, 2, 3], 4: [0, 1, 2, 3]}[width]
    got = dict(zip(sel, gpu_lde(gpu, m[sel], LOG_BIG, shift_mode)))
    if 0 in got:    # the LDE of a constant is that constant
        bad = np.nonzero(got[0] != P - 1)[0]
        assert bad.size == 0, f"constant column: {bad.size} of {2 * n} outputs differ, first at {int(bad[0])}: {int(got[0][bad[0]])}"
    # A + B (-1)^i is the polynomial A + B x^(N/2); at x = s w_2N^j that is A + B s^(N/2) w_4^j
    w4 = pow(31, (P - 1) >> 2, P)
    s_half = pow(lde_shift(LOG_BIG, shift_mode), n // 2, P)
    per_j = np.array([(a + b * s_half % P * pow(w4, j, P)) % P for j in range(4)], np.uint32)
    want = np.tile(per_j, 2 * n // 4)
    bad = np.nonzero(got[1] != want)[0]
    assert bad.size == 0, f"square wave: {bad.size} of {2 * n} outputs differ, first at {int(bad[0])}: {int(got[1][bad[0]])} != {int(want[bad[0]])}"
    if 3 in got:    # linearity across the columns of one call
        want = ((got[1].astype(np.uint64) + got[2]) % P).astype(np.uint32)
        bad = np.nonzero(got[3] != want)[0]
        assert bad.size == 0, f"random + square wave: {bad.size} of {2 * n} outputs differ from the sum, first at {int(bad[0])}"
