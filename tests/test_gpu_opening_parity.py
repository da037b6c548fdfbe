"""GPU parity tests of the kernels behind the LogUp running sum (K4 tail), the out-of-domain openings (K6), the reduced
openings that form the FRI input (K7) and the proof-of-work grind (K9), each called through its stage entry point (which
runs the prover's own host code) and compared word for word with the CPU oracle or with Python integers mod p.

The shapes are the ones where the kernels change path: the prefix sum's one-block / multi-block split at 2^11 rows,
open_columns_kernel's row loop above 2^16 rows (and its periodic reduction from 2^21), reduced_opening_kernel's 8-wide
body and 0..7-column tail, n_two = 0 / n_all (no real proof opens such a height), and the grind's batch boundaries."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


@pytest.fixture(scope="module")
def lib(oracle):
    from tests import _oracle_prover

    return _oracle_prover._lib(oracle)


u32p = C.POINTER(C.c_uint32)


# The stage entry points run on the prover's stream, torch on its own: every buffer torch writes is complete before a
# stage reads or writes it (torch.cuda.synchronize), and the stage's results are read after gpu.sync().
def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def zeros(words):
    import torch

    t = torch.zeros(words, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint32)


def _p(a):
    return a.ctypes.data_as(u32p)


def internal(gpu, a):
    t = dev(a)
    gpu.to_internal(t)
    return t


def raw_internal(gpu, words):
    """device words written as they are (Montgomery form, no conversion) and their canonical values"""
    t, c = dev(words), dev(words)
    gpu.from_internal(c)
    gpu.sync()
    return t, host(c).reshape(np.shape(words))


def extreme_words(width, n):
    """[width][n] raw internal words P-1 and 0x77ffffff (the largest high and low 16-bit halves of a word below p)"""
    i = np.add.outer(np.arange(width), np.arange(n))
    return np.where(i % 3 == 1, np.uint32(0x77FFFFFF), np.uint32(P - 1)).astype(np.uint32)


def ext_mul(a, b):
    """F_p[x]/(x^4 - 11)"""
    r = [0] * 4
    for i in range(4):
        for j in range(4):
            if i + j < 4:
                r[i + j] += a[i] * b[j]
            else:
                r[i + j - 4] += 11 * a[i] * b[j]
    return [x % P for x in r]


def root(log_n):
    return pow(31, (P - 1) >> log_n, P)


# ------------------------------------------------------------------ K4 tail: running sum
@pytest.mark.parametrize("log_n", [0, 1, 10, 11, 12, 21, 22])
@pytest.mark.parametrize("kind", ["random", "max", "zero"])
def test_logup_running_sum_matches_field_arithmetic(gpu, log_n, kind):
    """phi[r] = S[r-1] - r S[n-1] / n with S the inclusive prefix sums; 2^11 rows are one scan block, 2^12 the first two"""
    n = 1 << log_n
    rng = np.random.default_rng(1000 + log_n)
    tot = {"random": rng.integers(0, P, (4, n), dtype=np.uint32), "max": np.full((4, n), P - 1, np.uint32),
           "zero": np.zeros((4, n), np.uint32)}[kind]
    t_tot = internal(gpu, tot)
    t_phi = zeros(4 * n)
    cum = gpu.logup_running_sum(t_tot, t_phi, log_n)
    gpu.from_internal(t_tot)
    gpu.from_internal(t_phi)
    gpu.sync()
    s = np.cumsum(tot.astype(np.uint64), axis=1) % P           # < 2^22 terms of < 2^31: exact in 64 bits
    assert (host(t_tot).reshape(4, n) == s).all()
    assert cum == [int(x) for x in s[:, -1]]
    r = np.arange(n, dtype=np.uint64)
    want = np.zeros((4, n), np.uint64)
    for k in range(4):
        c = int(s[k, -1]) * pow(n, -1, P) % P
        before = np.concatenate([np.zeros(1, np.uint64), s[k, :-1]])
        want[k] = (before + P - (r * np.uint64(c)) % P) % P
    got = host(t_phi).reshape(4, n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} phi words differ, first at (column, row) {bad[0].tolist()}"


# ------------------------------------------------------------------ K6: openings
# (log_n, widths of the matrices opened by one call): every width mod OPEN_CT = 4, the 1245 columns of the precompile chips;
# 2^16 rows: 256 row blocks of one row each; 2^17: the first size where a thread loops; 2^21 / 2^22: one / two periodic reductions
OPEN_CASES = [(0, [1, 2]), (1, [3, 4]), (2, [5, 7, 9]), (8, [33, 1245]), (9, [1, 2, 3, 4, 5, 7, 9]), (16, [5, 4]),
              (17, [3, 2]), (21, [2, 1]), (22, [1, 2])]


def open_points(log_n, rng):
    """a random extension element, a base-field element outside H, one with zero low coefficients"""
    z = [rng.integers(1, P, 4).tolist(), [int(rng.integers(2, P)), 0, 0, 0], [0, 0] + rng.integers(1, P, 2).tolist()]
    while pow(z[1][0], 1 << log_n, P) == 1:
        z[1][0] += 1
    return z


def oracle_open(lib, cols, log_n, z):
    """[width][2][4]: each column's interpolant at z and at z w_n (orc_eval_columns, shift 1)"""
    cols = np.ascontiguousarray(cols, np.uint32)
    zn = [x * root(log_n) % P for x in z]
    out = np.zeros((2, cols.shape[0], 4), np.uint32)
    for pt, zz in enumerate((z, zn)):
        lib.orc_eval_columns(_p(cols), cols.shape[0], log_n, 1, _p(np.array(zz, np.uint32)), _p(out[pt]))
    return out.transpose(1, 0, 2)


def _check_open(gpu, lib, t_mats, canon, log_n, z):
    got = gpu.open([(t, m.shape[0], log_n) for t, m in zip(t_mats, canon)], z)
    want = oracle_open(lib, np.concatenate(canon), log_n, z)
    bad = np.nonzero((got != want).any(axis=2))
    assert bad[0].size == 0, f"z {z}: {bad[0].size} values differ, first (column, point) {(int(bad[0][0]), int(bad[1][0]))}"


@pytest.mark.parametrize("log_n,widths", OPEN_CASES)
def test_open_matches_oracle(gpu, lib, log_n, widths):
    n = 1 << log_n
    rng = np.random.default_rng(2000 + log_n)
    mats = [rng.integers(0, P, (w, n), dtype=np.uint32) for w in widths]
    mats[0][0] = 0                  # a column that is non-zero in row 0 only: its value at z w_n comes from the weight of row n-1
    mats[0][0, 0] = P - 1
    t_mats = [internal(gpu, m) for m in mats]
    for z in open_points(log_n, rng):
        _check_open(gpu, lib, t_mats, mats, log_n, z)


@pytest.mark.parametrize("log_n,widths", [(9, [9]), (17, [5]), (21, [1])])
def test_open_extreme_words(gpu, lib, log_n, widths):
    """raw internal words P-1 and 0x77ffffff: every dot-product term at the top of the range f64dot.cuh assumes"""
    n = 1 << log_n
    rng = np.random.default_rng(3000 + log_n)
    words = extreme_words(widths[0], n)
    t, canon = raw_internal(gpu, words)
    for z in open_points(log_n, rng)[:2]:
        _check_open(gpu, lib, [t], [canon], log_n, z)


# ------------------------------------------------------------------ K7: reduced openings
# (n_all, log_m): the 8-wide body with tails of 0..7 columns and reductions every 16 terms; the widest only at small heights
K7_CASES = [(1, 1), (1, 2), (1, 9), (1, 23), (7, 1), (7, 8), (8, 2), (8, 9), (9, 8), (9, 17), (15, 9), (16, 8), (17, 9),
            (17, 22), (24, 8), (25, 2), (25, 9), (1245, 1), (1245, 8), (5003, 2)]


def oracle_reduced(lib, cols, n_two, log_m, alpha, ol, on, zeta):
    keep = [np.ascontiguousarray(c, np.uint32) for c in cols]
    ptrs = (u32p * len(keep))(*[_p(k) for k in keep])
    zn = ext_mul(zeta, [root(log_m - 1), 0, 0, 0])
    out = np.zeros((1 << log_m, 4), np.uint32)
    on_a = np.ascontiguousarray(on if n_two else np.zeros((1, 4)), np.uint32)
    lib.orc_reduced_opening(ptrs, n_two, len(cols), log_m, _p(np.array(alpha, np.uint32)), _p(np.ascontiguousarray(ol, np.uint32)),
                            _p(on_a), _p(np.array(zeta, np.uint32)), _p(np.array(zn, np.uint32)), _p(out))
    return out


def _check_reduced(gpu, lib, t_cols, canon_cols, log_m, rng):
    n_all = len(t_cols)
    alpha, zeta = rng.integers(0, P, 4).tolist(), rng.integers(0, P, 4).tolist()
    ol = rng.integers(0, P, (n_all, 4), dtype=np.uint32)
    on = rng.integers(0, P, (n_all, 4), dtype=np.uint32)
    t_out = zeros(4 << log_m)
    for n_two in sorted({0, 1, 8, n_all - 1, n_all} & set(range(n_all + 1))):
        gpu.reduced_opening(t_cols, n_two, log_m, alpha, ol, on[:n_two], zeta, t_out)
        gpu.from_internal(t_out)
        gpu.sync()
        got = host(t_out).reshape(-1, 4)
        want = oracle_reduced(lib, canon_cols, n_two, log_m, alpha, ol, on[:n_two], zeta)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, f"n_all {n_all}, n_two {n_two}: {bad.size} of {1 << log_m} outputs differ, first at {int(bad[0])}"


@pytest.mark.parametrize("n_all,log_m", K7_CASES)
def test_reduced_opening_matches_oracle(gpu, lib, n_all, log_m):
    m = 1 << log_m
    rng = np.random.default_rng(4000 + 31 * n_all + log_m)
    cols = rng.integers(0, P, (n_all, m), dtype=np.uint32)
    t_cols = internal(gpu, cols)
    _check_reduced(gpu, lib, list(t_cols.view(n_all, m)), list(cols), log_m, rng)


@pytest.mark.parametrize("n_all,log_m", [(25, 9), (1245, 2), (17, 17)])
def test_reduced_opening_extreme_words(gpu, lib, n_all, log_m):
    m = 1 << log_m
    words = extreme_words(n_all, m)
    t, canon = raw_internal(gpu, words)
    _check_reduced(gpu, lib, list(t.view(n_all, m)), list(canon), log_m, np.random.default_rng(5000 + n_all))


# ------------------------------------------------------------------ K9: grind
@pytest.mark.parametrize("bits", [0, 1, 4, 16, 20])
@pytest.mark.parametrize("pos", [0, 3, 7])
def test_pow_grind_smallest_witness(gpu, lib, bits, pos):
    """at 20 bits the 2^22-candidate batches apply"""
    state = np.random.default_rng(6000 + 8 * bits + pos).integers(0, P, 16, dtype=np.uint32)
    want = int(lib.orc_pow_grind(_p(state), pos, bits))
    assert gpu.pow_grind(state.tolist(), pos, bits) == want


def test_pow_grind_witness_beyond_first_batch(gpu, lib):
    """a state whose smallest 10-bit witness lies past the first 2^12-candidate batch (about 2 % of states): found by a
    deterministic search with the oracle"""
    for seed in range(2000):
        state = np.random.default_rng(7000 + seed).integers(0, P, 16, dtype=np.uint32)
        want = int(lib.orc_pow_grind(_p(state), 2, 10))
        if want >= 1 << 12:
            break
    else:
        pytest.fail("no state with a witness beyond the first batch among 2000 seeds")
    assert gpu.pow_grind(state.tolist(), 2, 10) == want


# ------------------------------------------------------------------ refusals
def test_stage_entries_reject_bad_arguments(gpu):
    from dvt_circuits_amd import capi

    L, h = gpu.lib, gpu.h
    E = capi.DVT_ERR_INPUT
    u4 = lambda *w: (C.c_uint32 * 4)(*w)
    ok4, bad4 = u4(1, 2, 3, 4), u4(1, 2, P, 4)
    # buffers sized for the largest size passed, so that a missing check could not write out of bounds
    big, other = zeros(4 << 24), zeros(4 << 24)
    cum = (C.c_uint32 * 4)()
    for args in ((None, other.data_ptr(), 4, cum), (big.data_ptr(), None, 4, cum), (big.data_ptr(), other.data_ptr(), 4, None),
                 (big.data_ptr(), other.data_ptr(), 23, cum), (big.data_ptr(), big.data_ptr() + 16, 4, cum)):
        assert L.dvt_stage_logup_running_sum(h, *args) == E, args
    out = np.zeros((8, 2, 4), np.uint32)
    mats = (capi.DevMatrix * 2)(capi.DevMatrix(big.data_ptr(), 1, 23), capi.DevMatrix(big.data_ptr(), 1, 23))
    assert L.dvt_stage_open(h, mats, 1, ok4, _p(out)) == E                       # log_n > 22
    mats[0].log_height = 4
    assert L.dvt_stage_open(h, mats, 2, ok4, _p(out)) == E                       # different heights
    mats[1].log_height = 4
    assert L.dvt_stage_open(h, mats, 2, bad4, _p(out)) == E                      # z not canonical
    assert L.dvt_stage_open(h, mats, 2, None, _p(out)) == E
    assert L.dvt_stage_open(h, mats, 2, ok4, None) == E
    assert L.dvt_stage_open(h, None, 2, ok4, _p(out)) == E
    mats[1].d_data = None
    assert L.dvt_stage_open(h, mats, 2, ok4, _p(out)) == E
    cols = (C.c_void_p * 3)(big.data_ptr(), other.data_ptr(), big.data_ptr())
    ov = np.zeros((3, 4), np.uint32)
    ob = ov.copy()
    ob[1, 3] = P
    d_out = other.data_ptr()
    for (cs, n_two, n_all, log_m, al, ol, on, ze) in (
            (None, 1, 3, 4, ok4, ov, ov, ok4), (cols, 1, 3, 0, ok4, ov, ov, ok4), (cols, 1, 3, 24, ok4, ov, ov, ok4),
            (cols, 4, 3, 4, ok4, ov, ov, ok4), (cols, 0, 0, 4, ok4, ov, ov, ok4), (cols, 1, 3, 4, bad4, ov, ov, ok4),
            (cols, 1, 3, 4, ok4, ov, ov, bad4), (cols, 1, 3, 4, None, ov, ov, ok4), (cols, 1, 3, 4, ok4, ob, ov, ok4),
            (cols, 2, 3, 4, ok4, ov, ob, ok4), (cols, 1, 3, 4, ok4, None, ov, ok4), (cols, 1, 3, 4, ok4, ov, None, ok4)):
        rc = L.dvt_stage_reduced_opening(h, cs, n_two, n_all, log_m, al, _p(ol) if ol is not None else None,
                                         _p(on) if on is not None else None, ze, d_out)
        assert rc == E, (n_two, n_all, log_m)
    assert L.dvt_stage_reduced_opening(h, cols, 1, 3, 4, ok4, _p(ov), _p(ov), ok4, None) == E
    cols[1] = None
    assert L.dvt_stage_reduced_opening(h, cols, 1, 3, 4, ok4, _p(ov), _p(ov), ok4, d_out) == E
    st, w = (C.c_uint32 * 16)(*range(16)), C.c_uint32()
    assert L.dvt_stage_pow_grind(h, st, 8, 4, C.byref(w)) == E
    assert L.dvt_stage_pow_grind(h, st, 0, 31, C.byref(w)) == E
    assert L.dvt_stage_pow_grind(h, None, 0, 4, C.byref(w)) == E
    assert L.dvt_stage_pow_grind(h, st, 0, 4, None) == E
    st[5] = P
    assert L.dvt_stage_pow_grind(h, st, 0, 4, C.byref(w)) == E
    gpu.sync()
