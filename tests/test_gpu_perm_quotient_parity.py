"""GPU parity tests of one chip's permutation trace (K4: perm_rows_kernel, perm_rows_parts_kernel + sum_parts_kernel, then
the running sum) and quotient (K5: quotient_kernel<Air, PART>, quotient_parts_kernel + sum_parts_kernel,
selector_table_kernel), called through dvt_stage_perm / dvt_stage_quotient (the prover's own host code) and compared word
for word with orc_perm_trace / orc_quotient, for every chip of the rv32 and toy machines.

Both stages are plain functions of their inputs, so random columns are valid test data.  Random columns switch on every
interaction; a proof only evaluates the tuples of interactions its guest switches on, so a wrong column, bus or sign in an
interaction that no guest uses would leave every proof byte unchanged.  Raw internal words P-1 and 0x77ffffff in every
column put every FP64 dot product (DotAcc4 with a reduce() every 32 terms, the Fd4 LogUp batch constraints) at the top of
its range.  Heights 2^0 .. 2^3 reach the next-row wrap and a partial 256-thread block; 2^15 is the largest part-parallel
height.  The in-kernel selectors only run when the selector table cannot be allocated, and the per-row / per-part
launches of the precompile chips only above 2^15 rows: both are selected explicitly here.

The heights were chosen by timing the oracle: 2^16 rows of the widest chip (bls_g1, 1245 columns) and 2^20 rows of the
cpu chip cost a few seconds each, and the whole file runs in well under a minute."""
import numpy as np
import pytest

from tests.test_gpu_opening_parity import extreme_words, host, internal, raw_internal

pytestmark = pytest.mark.gpu
P = 2013265921

CHIPS = [("toy", c) for c in range(3)] + [("rv32", c) for c in range(14)]
# chips with the part-parallel launches (dvt_circuits_amd/csrc/machine.h): K4 when N_LPARTS > 1, K5 when NP > 2 and MAIN_W >= 128
K4_PARTS = {"cpu", "muldiv", "fp_op", "fp2_op", "bls_g1", "secp_k1", "u256_mul"}
K5_PARTS = {"sha_extend", "sha_compress", "fp_op", "fp2_op", "bls_g1", "secp_k1", "u256_mul"}
# chips with first-row, last-row and transition constraints
SELECTOR_CHIPS = {"cpu", "sha_extend", "sha_compress", "fib"}


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


def airs():
    from tests import _orc

    return {m: _orc.air(m) for m in ("toy", "rv32")}


def chip_info(machine, cid):
    ch = airs()[machine].chip(cid)
    return dict(name=ch.name.decode(), main_w=ch.main_w, prep_w=ch.prep_w, n_pub=ch.n_pub, ni=ch.n_interactions,
                ext_w=(ch.n_interactions + 1) // 2 if ch.n_interactions else 0)


def chip_id(name):
    a = airs()
    for m in ("rv32", "toy"):
        for c in range(a[m].nchips):
            if a[m].chip(c).name.decode() == name:
                return m, c
    raise KeyError(name)


def sentinel(words):
    """an output buffer of 0xffffffff words: a word the kernels do not write fails the canonical check"""
    import torch

    t = torch.full((words,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def canonical_out(gpu, t, shape):
    """the words of t (Montgomery form) as canonical values, after checking that each is below p"""
    gpu.sync()
    raw = host(t)
    bad = np.nonzero(raw >= P)[0]
    assert bad.size == 0, f"{bad.size} output words not below p (first at {int(bad[0])}: {int(raw[bad[0]]):#x})"
    gpu.from_internal(t)
    gpu.sync()
    return host(t).reshape(shape)


def columns(gpu, kind, width, n, rng):
    """(device words in Montgomery form, canonical values) of a [width][n] matrix; no device words for width 0"""
    if width == 0:
        return None, np.zeros((0, n), np.uint32)
    if kind == "extreme":
        return raw_internal(gpu, extreme_words(width, n))
    c = rng.integers(0, P, (width, n), dtype=np.uint32)
    if kind == "zero":
        c[:] = 0
    elif kind == "alternate":   # random even rows, zero odd rows: both branches of PermRowCtx::interaction in one wave
        c[:, 1::2] = 0
    return internal(gpu, c), c


def first_bad(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} words differ, first at {bad[0].tolist()}" if len(bad) else ""


# ------------------------------------------------------------------ K4
def k4_paths(info, log_n):
    return ["default", "rows"] + (["parts"] if info["name"] in K4_PARTS and log_n <= 15 else [])


def check_perm(gpu, machine, cid, log_n, kind, rng, perm_alpha=None, beta=None):
    info, n = chip_info(machine, cid), 1 << log_n
    t_main, main = columns(gpu, kind, info["main_w"], n, rng)
    t_prep, prep = columns(gpu, "extreme" if kind == "extreme" else "random", info["prep_w"], n, rng)
    pubs = rng.integers(0, P, info["n_pub"]).tolist()
    perm_alpha = rng.integers(0, P, 4).tolist() if perm_alpha is None else perm_alpha
    beta = rng.integers(0, P, 4).tolist() if beta is None else beta
    want, want_cum = airs()[machine].perm_trace(cid, main, prep if info["prep_w"] else np.zeros((1, n), np.uint32), pubs, perm_alpha, beta)
    w = 4 * info["ext_w"]
    assert want.shape == (w, n)
    for path in k4_paths(info, log_n):
        t_perm = sentinel(w * n)
        cum = gpu.perm(machine, cid, t_main, t_prep, log_n, pubs, perm_alpha, beta, t_perm, path)
        got = canonical_out(gpu, t_perm, (w, n))
        where = f"{info['name']} 2^{log_n} {kind} path {path} beta {beta}"
        assert cum == [int(x) for x in want_cum], f"{where}: cumulative sum"
        assert (got == want).all(), f"{where}: {first_bad(got, want)}"


@pytest.mark.parametrize("machine,cid", CHIPS)
def test_perm_matches_oracle_small(gpu, machine, cid):
    """2^0 .. 2^3 (next-row wrap, partial block), 2^8 / 2^9 (one and two blocks): every input kind, every launch"""
    rng = np.random.default_rng(100 + 17 * cid + (machine == "toy"))
    for log_n in (0, 1, 2, 3, 8, 9):
        for kind in ("random", "zero", "alternate", "extreme"):
            check_perm(gpu, machine, cid, log_n, kind, rng)


@pytest.mark.parametrize("machine,cid", CHIPS)
def test_perm_edge_challenges(gpu, machine, cid):
    """beta in {0, 1, P-1}; all-zero columns with perm_alpha = P - bus, which makes the denominator of every tuple of
    only zero values on that bus vanish (the oracle's inverse of zero is the reference).  Of all chips only toy fib has an
    interaction that is switched on for an all-zero row with an all-zero tuple: there the denominator is exactly zero."""
    rng = np.random.default_rng(200 + 17 * cid + (machine == "toy"))
    for b in (0, 1, P - 1):
        for log_n in (3, 9):
            check_perm(gpu, machine, cid, log_n, "random", rng, beta=[b, 0, 0, 0])
    import ctypes as C
    from tests import _orc

    class Inter(C.Structure):
        _fields_ = [("bus", C.c_int32), ("sign", C.c_int32), ("scope", C.c_int32), ("arity", C.c_int32)]

    ch = airs()[machine].chip(cid)
    inter = C.cast(ch.inter, C.POINTER(Inter))
    assert _orc.P == P
    for bus in sorted({inter[j].bus for j in range(ch.n_interactions)}):
        check_perm(gpu, machine, cid, 3, "zero", rng, perm_alpha=[(P - bus) % P, 0, 0, 0])


TALL_K4 = [(m, c, lg) for m, c in CHIPS for lg in (15, 16)]


@pytest.mark.parametrize("machine,cid,log_n", TALL_K4)
def test_perm_matches_oracle_tall(gpu, machine, cid, log_n):
    """2^15: the largest part-parallel height; 2^16: the default turns to the per-row kernel"""
    check_perm(gpu, machine, cid, log_n, "random", np.random.default_rng(300 + 17 * cid + log_n + (machine == "toy")))


def test_perm_cpu_2_20(gpu):
    check_perm(gpu, "rv32", 2, 20, "random", np.random.default_rng(399))


# ------------------------------------------------------------------ K5
def k5_paths(info, log_n):
    return ["default", "rows"] + (["parts"] if info["name"] in K5_PARTS and log_n <= 15 else [])


def oracle_quotient(lib, machine, cid, log_n, main, prep, perm, pubs, perm_alpha, beta, alpha, cum):
    import ctypes as C

    from tests._oracle_prover import _a, _p

    n = 1 << log_n
    out = np.zeros((8, n), np.uint32)
    lib.orc_quotient(C.addressof(airs()[machine].chips[cid]), _p(_a(main)), _p(_a(prep)), _p(_a(perm)), log_n, _p(_a(pubs)),
                     _p(_a(perm_alpha)), _p(_a(beta)), _p(_a(alpha)), _p(_a(cum)), _p(out))
    return out


def check_quotient(gpu, lib, machine, cid, log_n, kind, rng, alphas=None, cum=None, selectors=("table", "kernel")):
    info, n = chip_info(machine, cid), 1 << log_n
    t_main, main = columns(gpu, kind, info["main_w"], 2 * n, rng)
    t_prep, prep = columns(gpu, kind, info["prep_w"], 2 * n, rng)
    t_perm, perm = columns(gpu, kind, 4 * info["ext_w"], 2 * n, rng)
    pubs = rng.integers(0, P, info["n_pub"]).tolist()
    perm_alpha, beta = rng.integers(0, P, 4).tolist(), rng.integers(0, P, 4).tolist()
    cum = rng.integers(0, P, 4).tolist() if cum is None else cum
    for alpha in alphas or [rng.integers(0, P, 4).tolist()]:
        want = oracle_quotient(lib, machine, cid, log_n, main, prep, perm, pubs, perm_alpha, beta, alpha, cum)
        for path in k5_paths(info, log_n):
            for sel in selectors:
                t_out = sentinel(8 * n)
                gpu.quotient(machine, cid, t_main, t_prep, t_perm, log_n, pubs, perm_alpha, beta, alpha, cum, t_out, path, sel)
                got = canonical_out(gpu, t_out, (8, n))
                assert (got == want).all(), f"{info['name']} 2^{log_n} {kind} path {path} selectors {sel} alpha {alpha}: {first_bad(got, want)}"


@pytest.mark.parametrize("machine,cid", CHIPS)
def test_quotient_matches_oracle_small(gpu, lib, machine, cid):
    """2^0 .. 2^3 and 2^8; alpha in {0, 1, P-1, random}, cum = 0; both selector sources and every launch"""
    rng = np.random.default_rng(500 + 17 * cid + (machine == "toy"))
    edge = [[0, 0, 0, 0], [1, 0, 0, 0], [P - 1, 0, 0, 0], rng.integers(0, P, 4).tolist()]
    for log_n in (0, 1, 2, 3, 8):
        check_quotient(gpu, lib, machine, cid, log_n, "random", rng, alphas=edge if log_n in (2, 8) else None)
        check_quotient(gpu, lib, machine, cid, log_n, "extreme", rng)
    check_quotient(gpu, lib, machine, cid, 3, "random", rng, cum=[0, 0, 0, 0])


# 2^15: the largest part-parallel height; 2^16: the default turns to one launch per part
TALL_K5 = [(m, c, lg) for m, c in CHIPS for lg in (15, 16)]


@pytest.mark.parametrize("machine,cid,log_n", TALL_K5)
def test_quotient_matches_oracle_tall(gpu, lib, machine, cid, log_n):
    info = chip_info(machine, cid)
    sel = ("table", "kernel") if info["name"] in SELECTOR_CHIPS else ("table",)
    check_quotient(gpu, lib, machine, cid, log_n, "random", np.random.default_rng(600 + 17 * cid + log_n + (machine == "toy")),
                   selectors=sel)


def test_quotient_cpu_2_20(gpu, lib):
    check_quotient(gpu, lib, "rv32", 2, 20, "random", np.random.default_rng(699))


def test_quotient_selector_table_reused_across_heights(lib):
    """one handle at heights A, B, A: the second call at A reads the table the first one built"""
    from dvt_circuits_amd import capi

    p = capi.Prover()
    try:
        rng = np.random.default_rng(700)
        for name in ("cpu", "fib"):
            m, c = chip_id(name)
            for log_n in (3, 9, 3):
                check_quotient(p, lib, m, c, log_n, "random", rng, selectors=("table",))
    finally:
        p.close()


# ------------------------------------------------------------------ refusals
def test_perm_quotient_entries_reject_bad_arguments(gpu):
    import ctypes as C

    import torch
    from dvt_circuits_amd import capi

    L, h, E = gpu.lib, gpu.h, capi.DVT_ERR_INPUT
    u4 = lambda *w: (C.c_uint32 * 4)(*w)
    ok4, bad4 = u4(1, 2, 3, 4), u4(1, 2, P, 4)
    # every buffer holds 2^26 words: as many as any matrix of the calls below (toy range8 at 2^23 rows: [8][2^23] words)
    bufs = [torch.zeros(1 << 26, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    a, b, c, o = [t.data_ptr() for t in bufs]
    pubs, pubs_bad = (C.c_uint32 * 8)(*range(1, 9)), (C.c_uint32 * 8)(1, P, 3, 4, 5, 6, 7, 8)   # (at most 5 public values per chip)
    cum = (C.c_uint32 * 4)()
    PATH, ROWS, PARTS = capi.PATHS["default"], capi.PATHS["rows"], capi.PATHS["parts"]
    # (machine, chip, main, prep, log_n, pub, perm_alpha, beta, path, perm, cum): toy 0 = range8 (prep 1), toy 1 = fib (3
    # public values), rv32 0 = program (no part-parallel launch), rv32 2 = cpu
    good = (b"toy", 0, a, b, 4, pubs, ok4, ok4, PATH, c, cum)
    assert L.dvt_stage_perm(h, *good) == capi.DVT_OK
    bad_perm = [
        (b"nope", 0, a, b, 4, pubs, ok4, ok4, PATH, c, cum), (None, 0, a, b, 4, pubs, ok4, ok4, PATH, c, cum),
        (b"toy", 3, a, b, 4, pubs, ok4, ok4, PATH, c, cum), (b"rv32", 14, a, b, 4, pubs, ok4, ok4, PATH, c, cum),
        (b"toy", 0, a, b, 23, pubs, ok4, ok4, PATH, c, cum),
        (b"toy", 0, a, b, 4, pubs, bad4, ok4, PATH, c, cum), (b"toy", 0, a, b, 4, pubs, ok4, bad4, PATH, c, cum),
        (b"toy", 1, a, None, 4, pubs_bad, ok4, ok4, PATH, c, cum), (b"toy", 1, a, None, 4, None, ok4, ok4, PATH, c, cum),
        (b"toy", 0, None, b, 4, pubs, ok4, ok4, PATH, c, cum), (b"toy", 0, a, None, 4, pubs, ok4, ok4, PATH, c, cum),
        (b"toy", 0, a, b, 4, pubs, ok4, ok4, PATH, None, cum), (b"toy", 0, a, b, 4, pubs, ok4, ok4, PATH, c, None),
        (b"toy", 0, a, b, 4, pubs, None, ok4, PATH, c, cum), (b"toy", 0, a, b, 4, pubs, ok4, None, PATH, c, cum),
        (b"toy", 0, a, b, 4, pubs, ok4, ok4, PATH, a + 32, cum), (b"toy", 0, a, b, 4, pubs, ok4, ok4, PATH, b - 64, cum),
        (b"toy", 0, a, b, 4, pubs, ok4, ok4, 3, c, cum), (b"rv32", 0, a, b, 4, pubs, ok4, ok4, PARTS, c, cum),
        (b"rv32", 2, a, None, 16, pubs, ok4, ok4, PARTS, c, cum),
    ]
    for args in bad_perm:
        assert L.dvt_stage_perm(h, *args) == E, args
    assert L.dvt_stage_perm(h, b"rv32", 2, a, None, 15, pubs, ok4, ok4, PARTS, c, cum) == capi.DVT_OK
    assert L.dvt_stage_perm(h, b"rv32", 2, a, None, 16, pubs, ok4, ok4, ROWS, c, cum) == capi.DVT_OK
    # (machine, chip, main_lde, prep_lde, perm_lde, log_n, pub, perm_alpha, beta, alpha, cum, path, selectors, out)
    good = (b"toy", 0, a, b, c, 4, pubs, ok4, ok4, ok4, ok4, PATH, 0, o)
    assert L.dvt_stage_quotient(h, *good) == capi.DVT_OK

    def q(i, v):
        args = list(good)
        args[i] = v
        return tuple(args)

    bad_quot = [q(0, b"nope"), q(0, None), q(1, 3), q(5, 23), q(7, bad4), q(8, bad4), q(9, bad4), q(10, bad4),
                q(7, None), q(8, None), q(9, None), q(10, None), q(2, None), q(3, None), q(4, None), q(13, None),
                q(13, a + 64), q(13, b - 64), q(13, c + 4), q(11, 3), q(12, 2), q(11, PARTS),
                (b"toy", 1, a, None, c, 4, pubs_bad, ok4, ok4, ok4, ok4, PATH, 0, o),
                (b"toy", 1, a, None, c, 4, None, ok4, ok4, ok4, ok4, PATH, 0, o),
                (b"rv32", 2, a, None, c, 4, pubs, ok4, ok4, ok4, ok4, PARTS, 0, o),         # cpu: no part-parallel K5
                (b"rv32", 9, a, None, c, 16, pubs, ok4, ok4, ok4, ok4, PARTS, 0, o)]        # fp_op above 2^15
    for args in bad_quot:
        assert L.dvt_stage_quotient(h, *args) == E, args
    assert L.dvt_stage_quotient(h, b"rv32", 9, a, None, c, 15, pubs, ok4, ok4, ok4, ok4, PARTS, 0, o) == capi.DVT_OK
    # the part-parallel launches exist for exactly the chips of K4_PARTS / K5_PARTS (the parity tests run those)
    for machine, cid in CHIPS:
        name, m = chip_info(machine, cid)["name"], machine.encode()
        rc = L.dvt_stage_perm(h, m, cid, a, b, 4, pubs, ok4, ok4, PARTS, c, cum)
        assert (rc == capi.DVT_OK) == (name in K4_PARTS), (name, rc)
        rc = L.dvt_stage_quotient(h, m, cid, a, b, c, 4, pubs, ok4, ok4, ok4, ok4, PARTS, 0, o)
        assert (rc == capi.DVT_OK) == (name in K5_PARTS), (name, rc)
    gpu.sync()
