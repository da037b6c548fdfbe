"""A deterministic corpus of precompile calls at the extremes of what the five big-integer chips accept (fp_op, fp2_op,
bls_g1, secp_k1, u256_mul), one guest per chip (tests/guests_bigops.py), and what the tests on it share: Knuth's
algorithm D restated with a record of the branches it takes, the reference rows (oracle/rv32_model.py) computed once per
(chip, shard size), and the carry cells of every identity read from those rows.  Needs no GPU.

Row counts sit just past the workgroups of the device's K0 kernels (csrc/rv32_bigops.hip): 65..130 rows per chip (cells
kernel: 64 threads), 257..300 for u256_mul (lookups kernel: 256 threads).

The operands that took a search (the long-division branches, the rows with high rel1 carries) were searched once and are
pinned here as literals; tests/test_bigop_corpus_cpu.py re-checks what they reach."""
import functools
import random

from tests import guests
from tests.guests import BLS_P, BLS_R, SECP_P, words_of
from tests.guests_bigops import ALIAS, precompile_calls

CHIPS = ("fp_op", "fp2_op", "bls_g1", "secp_k1", "u256_mul")
TOP256, TOP384 = (1 << 256) - 1, (1 << 384) - 1

# ------------------------------------------------------------------ Knuth's algorithm D, with the branches it takes
B32 = 1 << 32
DIV_BRANCHES = ("single_digit", "shift_zero", "shift_nonzero", "correction", "qhat_overflow", "rhat_exit", "add_back")


def digits32(v, n):
    return [(v >> (32 * i)) & (B32 - 1) for i in range(n)]


def knuth_d(u, v):
    """TAOCP vol. 2, 4.3.1, algorithm D on little-endian base-2^32 digits (u: m digits, v: n <= m digits, v[-1] != 0), from
    the book's steps D1..D8 -> (quotient digits, remainder digits, the set of DIV_BRANCHES taken):
      single_digit   n = 1 (the book sends this case to exercise 16: short division)
      shift_zero / shift_nonzero   D1: the normalisation factor is 1 / is a power of two above 1
      correction     D3: qhat was decreased at least once
      qhat_overflow  D3: the trial quotient came out as b or more
      rhat_exit      D3: the test was not repeated because rhat reached b
      add_back       D6"""
    m, n = len(u), len(v)
    taken = set()
    if n == 1:
        taken.add("single_digit")
        q, k = [0] * m, 0
        for j in reversed(range(m)):
            q[j], k = divmod(k * B32 + u[j], v[0])
        return q, [k], taken
    s = 32 - v[-1].bit_length()
    taken.add("shift_zero" if s == 0 else "shift_nonzero")
    vn = digits32(sum(d << (32 * i) for i, d in enumerate(v)) << s, n)
    un = digits32(sum(d << (32 * i) for i, d in enumerate(u)) << s, m + 1)
    q = [0] * (m - n + 1)
    for j in reversed(range(m - n + 1)):
        qhat, rhat = divmod(un[j + n] * B32 + un[j + n - 1], vn[n - 1])
        if qhat >= B32:
            taken.add("qhat_overflow")
        while qhat >= B32 or qhat * vn[n - 2] > B32 * rhat + un[j + n - 2]:
            taken.add("correction")
            qhat -= 1
            rhat += vn[n - 1]
            if rhat >= B32:
                taken.add("rhat_exit")
                break
        borrow = 0
        for i in range(n):
            t = un[i + j] - borrow - qhat * vn[i]
            un[i + j], borrow = t % B32, -(t // B32)
        t = un[j + n] - borrow
        un[j + n] = t % B32
        if t < 0:
            taken.add("add_back")
            qhat -= 1
            c = 0
            for i in range(n):
                c += un[i + j] + vn[i]
                un[i + j], c = c % B32, c // B32
            un[j + n] = (un[j + n] + c) % B32
        q[j] = qhat
    return q, digits32(sum(d << (32 * i) for i, d in enumerate(un[:n])) >> s, n), taken


def u256_division_branches(x, y, m):
    """the branches of the long division a u256_mul row needs: u = x*y - r in 17 digits by v = M in ceil(len(M) / 4)"""
    M = m or 1 << 256
    r = x * y % M
    nv = ((M.bit_length() + 7) // 8 + 3) // 4
    q, rem, taken = knuth_d(digits32(x * y - r, 17), digits32(M, nv))
    assert sum(d << (32 * i) for i, d in enumerate(q)) == x * y // M and not any(rem)
    return taken


# ------------------------------------------------------------------ u256_mul
# (x, y, m) found by a search over digits from {0, 1, 0x7fffffff, 0x80000000, 0xffffffff, random}, y = m in half the trials:
# the qhat correction, qhat >= 2^32, the rhat >= 2^32 exit and the add-back, each with and without a normalisation shift
U256_DIVISION_FINDS = [
    (0x180000000f9270f4e7fffffff7fffffff19999e3fffffffffed2f89d9, 0x80000000000000018d88348a80000000ffffffff8000000080000000, 0x80000000000000018d88348a80000000ffffffff8000000080000000),
    (0x18000000000000000f72f2bb88296f5ea7fffffff0000000180000000, 0x7fffffff7fffffff00000001000000017fffffffffffffff00000001, 0x7fffffff7fffffff00000001000000017fffffffffffffff00000001),
    (0x1000000008000000000000001e83b3ab1ffffffff00000000, 0x4d7598880000000000000002be893f480000000ffffffffffffffff80000000, 0x19a15a311ffffffff4e3d4d0fd2511c38000000010000000100000000),
    (0x7fffffffffffffffffffffff00000001ffffffff7fffffff00000000ffffffff, 0x1e830596800000007029381500000001e746ebeb61e1e80d0000000100000000, 0x1e830596800000007029381500000001e746ebeb61e1e80d0000000100000000),
    (0xffffffff7c0b03ee800000008b53c16b800000007fffffffffffffff00000001, 0x8000000000000001800000007fffffff3f64c50c, 0x8000000000000001800000007fffffff3f64c50c),
    (0xffffffff00000000ffffffff000000018c0354be00000000ffffffff, 0x80000000ffffffff, 0x80000000ffffffff),
    (0x8000000000000000f7fbc2217fffffff1a54fec67fffffffc9e901e1ffffffff, 0x80000000ffffffff7fffffff00000001800000008000000080000000, 0x80000000ffffffff7fffffff00000001800000008000000080000000),
    (0xffffffff723ac77500000000ffffffff000000007fffffff7fffffff00000000, 0xffffffffffffffff7fffffffffffffff7fffffff, 0xffffffffffffffff7fffffffffffffff7fffffff),
    (0xc8da380cffffffffffffffff00000000000000004c43fa7c00000000cefd0461, 0x7fffffffffffffffffffffffffffffff00000001, 0x7fffffffffffffffffffffffffffffff00000001),
    # an add-back example checked by hand (y = m, both operands of 32 bytes)
    (0x80000000ffffffff7fffffffffffffff216d27a2ffffffff7fffffff00000000, 0x8000000080000000ffffffffbd953dc2000000018000000014b9adb500000000, 0x8000000080000000ffffffffbd953dc2000000018000000014b9adb500000000),
]


@functools.lru_cache(maxsize=None)
def u256_triples():
    """(x, y, m) of every u256_mul row, all with floor(x * y / M) < 2^264 (the chip's 33-byte quotient)"""
    rng = random.Random(0x256)
    out = []
    # moduli of every byte length, top byte with and without its high bit; y < 256 m keeps the quotient inside 33 bytes
    for nbytes in range(1, 33):
        for high in (0, 1):
            topb = (0x80 if high else 0x01) | rng.getrandbits(7)
            m = (topb << (8 * (nbytes - 1))) | rng.getrandbits(8 * (nbytes - 1))
            ycap = min(1 << 256, m << 8)
            out.append((rng.getrandbits(256), rng.getrandbits(256) % ycap, m))       # random operands
            out.append((TOP256, ycap - 1, m))                                         # the largest quotient this modulus allows
    for nbytes in range(1, 33):          # exact multiples: y = m, r = 0, quotient x
        m = rng.getrandbits(8 * nbytes) | 1 << (8 * nbytes - 1) if nbytes % 2 else (rng.getrandbits(8 * nbytes) | 1 << (8 * nbytes - 8)) & ~1
        out.append((rng.getrandbits(256) | 1 << 255, m, m))
    for nbytes in range(1, 33):          # the modulus 0x01 00..00 / 0xff..ff of every length with extreme operands
        m = 1 << (8 * (nbytes - 1)) if nbytes % 2 else (1 << (8 * nbytes)) - 1
        out.append((TOP256, min(TOP256, (m << 8) - 1), m))
    out += [
        ((1 << 132) - 1, (1 << 132) + 1, 1),          # quotient 2^264 - 1: 33 bytes of 0xff
        (TOP256, 255, 1), (0, 0, 1), (1, 1, 1),
        (TOP256, TOP256, 0), (1 << 128, 1 << 128, 0), (0, TOP256, 0), (TOP256, 1, 0), (1 << 255, 2, 0),
        (TOP256, TOP256, 1 << 255), (1 << 255, 1 << 255, 1 << 255), ((1 << 255) - 1, 3, 1 << 255),
        (TOP256, TOP256, TOP256), (TOP256 - 1, TOP256 - 1, TOP256), (TOP256 - 1, 2, TOP256),
        # x = y = 2^256 - 1 with moduli of 32 bytes: quotients of exactly 33 significant bytes
        (TOP256, TOP256, 1 << 248), (TOP256, TOP256, (1 << 248) + 1), (TOP256, TOP256, (1 << 249) - 2), (TOP256, TOP256, BLS_R),
        (TOP256, TOP256, (1 << 256) - 189), (TOP256, TOP256, TOP256 - 1),
        # x * y < m: quotient 0
        (3, 5, BLS_R), (1 << 127, 1 << 127, 1 << 255), (0, TOP256, BLS_R), (1, BLS_R - 1, BLS_R), (0xffff, 0xffff, 0xfffe0002), (2, 3, 7),
        # even moduli
        (TOP256, TOP256, TOP256 - 1), (0x1234 << 200, 77, 1 << 255), (rng.getrandbits(256), rng.getrandbits(256), rng.getrandbits(256) & ~1 | 1 << 255),
        (rng.getrandbits(256), rng.getrandbits(64), 1 << 64), (rng.getrandbits(256), rng.getrandbits(10), 6),
    ]
    out += U256_DIVISION_FINDS
    pool = (0, 1, 0x7fffffff, 0x80000000, 0xffffffff)

    def num(n):
        return sum((pool[rng.getrandbits(8) % 5] if rng.getrandbits(2) else rng.getrandbits(32)) << (32 * i) for i in range(n))
    while len(out) < 264:                 # digits at the edges of the 32-bit words the division works on
        m = num(1 + rng.getrandbits(3))
        x, y = num(8), (m if rng.getrandbits(1) else num(8))
        if m and x * y // m < 1 << 264:
            out.append((x, y, m))
    assert all(x < 1 << 256 and y < 1 << 256 and m < 1 << 256 and x * y // (m or 1 << 256) < 1 << 264 for x, y, m in out)
    return tuple(out)


# ------------------------------------------------------------------ fp_op, fp2_op
FP_EDGES = (0, 1, BLS_P - 1, BLS_P, BLS_P + 1, TOP384, (BLS_P + 1) // 2)
FP2_SIGN_PATTERNS = ((1, 0, 1, 0), (0, 1, 0, 1), (0, 1, 1, 0), (1, 0, 0, 1))     # which of (x0, x1, y0, y1) is at the maximum


@functools.lru_cache(maxsize=None)
def fp_calls():
    """(op, x, y | "alias"): op 0 add, 1 sub, 2 mul"""
    out = []
    for op in (0, 1, 2):
        for i, x in enumerate(FP_EDGES):
            for j, y in enumerate(FP_EDGES):
                if op or i <= j:      # (add commutes)
                    out.append((op, x, y))
    out += [(0, TOP384, ALIAS), (1, BLS_P + 1, ALIAS), (2, BLS_P - 1, ALIAS)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fp2_calls():
    """(op, (x0, x1), (y0, y1) | "alias")"""
    rng = random.Random(0xF2)
    out = []
    for op in (0, 1, 2):
        for v in FP_EDGES:
            out.append((op, (v, v), (v, v)))
        for _ in range(26):
            x0, x1, y0, y1 = (FP_EDGES[rng.getrandbits(16) % 7] for _ in range(4))
            out.append((op, (x0, x1), (y0, y1)))
    for big in (BLS_P - 1, TOP384):      # x0 y0 - x1 y1 at both ends
        for pat in FP2_SIGN_PATTERNS:
            x0, x1, y0, y1 = (big * b for b in pat)
            out.append((2, (x0, x1), (y0, y1)))
    out += [(0, (TOP384, BLS_P), ALIAS), (1, (BLS_P + 1, 1), ALIAS), (2, (BLS_P - 1, TOP384), ALIAS)]
    return tuple(out)


# ------------------------------------------------------------------ bls_g1, secp_k1
# DOUBLE operands (x1, y1) with high rel1 carries: lam and y1 with 0xff bytes under the top byte, x1 = sqrt(2 lam y1 / 3)
# where that is a square, kept when x1's bytes make 3 x1^2 small at the middle coefficient (a search, done once)
HIGH_CARRY_DOUBLES = {
    "bls_g1": [
        (0x30f298c0ca1561348db5c0b117a2378093c3dfd15447019d6001cba5727bcfc260e2cffed319aaf6daa209ebacd2046, 0xcffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff),
        (0x47f3940312c1078842a3255046368b2a565d70f9584286f04cb0075760c60513e1427bae9741f381b8190c173312f30, 0x18ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffe0fffffffffffffffffffff7ffffffff),
        (0x2f8b61537072a27a993a95f34218e31e5cfa37ccc6107ff2f182748743f11150f00dc210c010f14348854c049264581, 0x18fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7ffffffffffff),
        (0x72ca23c30d57266b627808e1d45565c0dcd822c22ac2fd82c9c0a447d3b0e0a1a1ab7500d5ecf0d312a23dc141106d4, 0x8ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff),
    ],
    "secp_k1": [],
}


def curve_params(chip):
    """(p, words per coordinate, ADD code, DOUBLE code, generator)"""
    if chip == "bls_g1":
        return BLS_P, 12, guests.SYS_BLS12381_ADD, guests.SYS_BLS12381_DOUBLE, guests.BLS_G1
    return SECP_P, 8, guests.SYS_SECP256K1_ADD, guests.SYS_SECP256K1_DOUBLE, guests.SECP_G


def add_slope(pt, qt, p):
    return (qt[1] - pt[1]) * pow(qt[0] - pt[0], -1, p) % p


def double_slope(pt, p):
    return 3 * pt[0] * pt[0] * pow(2 * pt[1], -1, p) % p


@functools.lru_cache(maxsize=None)
def curve_calls(chip):
    """(P, Q) of every ADD row and P of every DOUBLE row of the chip: -> (adds, doubles).  The chips check no curve
    membership: any reduced coordinates with x1 != x2 (ADD) or y1 != 0 (DOUBLE) are a row."""
    p, _, _, _, G = curve_params(chip)
    rng = random.Random(0xEC if chip == "bls_g1" else 0x5EC)
    rnd = lambda: rng.getrandbits(p.bit_length() + 64) % p
    adds = [((p - 1, p - 1), (0, 0)), ((0, 0), (p - 1, p - 1)), ((p - 1, 0), (p - 2, p - 1)), ((0, p - 1), (1, 0)),
            # lam = 0 (equal ordinates), lam = 1, lam = p - 1
            ((0, p - 1), (p - 1, p - 1)), ((1, 1), (p - 1, 1)), ((0, 0), (1, 0)),
            ((0, 0), (1, 1)), ((p - 2, p - 2), (p - 1, p - 1)), ((p - 1, 0), (0, 1)),
            ((0, 1), (1, 0)), ((p - 1, 0), (p - 2, 1)), ((1, p - 1), (0, 0))]
    for lam in (0, 1, p - 1, 2, (p + 1) // 2):
        for _ in range(2):                # any x1, y1 with the slope given
            x1, y1 = rnd(), rnd()
            x2 = rnd()
            adds.append(((x1, y1), (x2, (y1 + lam * (x2 - x1)) % p)))
    for lam in (1, p - 1, 2, rnd(), rnd()):
        x1, y1 = rnd(), rnd()            # x3 = lam^2 - x1 - x2 = 0
        x2 = (lam * lam - x1) % p
        adds.append(((x1, y1), (x2, (y1 + lam * (x2 - x1)) % p)))
        x1, x2 = rnd(), rnd()            # y3 = lam (x1 - x3) - y1 = 0
        x3 = (lam * lam - x1 - x2) % p
        y1 = lam * (x1 - x3) % p
        adds.append(((x1, y1), (x2, (y1 + lam * (x2 - x1)) % p)))
        x1 = rnd()                       # x3 = y3 = 0: y1 = lam x1
        x2 = (lam * lam - x1) % p
        adds.append(((x1, lam * x1 % p), (x2, (lam * x1 + lam * (x2 - x1)) % p)))
    edge = (0, 1, p - 1, p - 2)
    while len(adds) < 52:                 # coordinates at the edges of the field
        x1, y1, x2, y2 = (edge[rng.getrandbits(8) % 4] for _ in range(4))
        if x1 != x2 and ((x1, y1), (x2, y2)) not in adds:
            adds.append(((x1, y1), (x2, y2)))
    g2 = guests.ec_double(G, p)
    adds += [(g2, G), (guests.ec_add(g2, G, p), g2)]                     # two rows on the curve
    adds += [((rnd(), rnd()), (rnd(), rnd())) for _ in range(16)]         # off-curve points
    adds = [a for a in adds if a[0][0] != a[1][0]]
    doubles = [(p - 1, p - 1), (0, 1), (p - 1, 1), (0, p - 1), (2, 6), (2, p - 6), (1, 1), (1, p - 1), (p - 2, 2), (p - 2, p - 2), (0, (p + 1) // 2),
               (p - 1, (p - 1) // 2), ((p + 1) // 2, (p + 1) // 2), G, g2]
    doubles += HIGH_CARRY_DOUBLES[chip]
    # the same recipe without the search: lam and y1 of 0xff bytes under p's top byte
    under = (1 << (8 * ((p.bit_length() + 7) // 8 - 1))) - 1
    tops = p >> under.bit_length()
    found = 0
    for k in range(2 * tops):             # (lam and y1 differ in the top byte: with lam = y1 the square depends on 2 / 3 alone)
        lam, y1 = under | (tops - 1 - k // 2) << under.bit_length(), under | (tops - 1 - (k + 1) // 2) << under.bit_length()
        c = 2 * lam * y1 * pow(3, -1, p) % p
        x1 = pow(c, (p + 1) // 4, p)          # (both fields have p = 3 mod 4)
        if x1 * x1 % p == c and found < 2:
            doubles += [(x1, y1), (p - x1, y1)]
            found += 1
    doubles.append((under, under))
    doubles += [(rnd(), rnd()) for _ in range(14)]
    doubles = [d for d in doubles if d[1] != 0]
    assert all(0 <= v < p for a in adds for pt in a for v in pt) and all(0 <= v < p for d in doubles for v in d)
    return tuple(adds), tuple(doubles)


# ------------------------------------------------------------------ the guests, and the reference rows
@functools.lru_cache(maxsize=None)
def cases(chip):
    """the chip's corpus as the case list of guests_bigops.precompile_calls"""
    if chip == "u256_mul":
        return tuple((guests.SYS_UINT256_MUL, tuple(words_of(x, 8)), tuple(words_of(y, 8) + words_of(m, 8))) for x, y, m in u256_triples())
    if chip == "fp_op":
        return tuple((guests.SYS_BLS12381_FP_ADD + op, tuple(words_of(x, 12)), y if y == ALIAS else tuple(words_of(y, 12))) for op, x, y in fp_calls())
    if chip == "fp2_op":
        w2 = lambda v: tuple(words_of(v[0], 12) + words_of(v[1], 12))
        return tuple((guests.SYS_BLS12381_FP2_ADD + op, w2(x), y if y == ALIAS else w2(y)) for op, x, y in fp2_calls())
    p, W, c_add, c_dbl, _ = curve_params(chip)
    adds, doubles = curve_calls(chip)
    pw = lambda pt: tuple(words_of(pt[0], W) + words_of(pt[1], W))
    out = [(c_add, pw(a), pw(b)) for a, b in adds] + [(c_dbl, pw(d), None) for d in doubles]
    # interleave the two operations (a row's selector changes from one row to the next)
    return tuple(out[i // 2] if i % 2 == 0 else out[len(out) - 1 - i // 2] for i in range(len(out)))


@functools.lru_cache(maxsize=None)
def guest(chip):
    """(elf, word offsets of the results in the guest's output)"""
    return precompile_calls(list(cases(chip)))


@functools.lru_cache(maxsize=None)
def model_run(chip, log_shard):
    from oracle import rv32_model

    return rv32_model.Run(guest(chip)[0], (), log_shard)


@functools.lru_cache(maxsize=8)       # (a shard's tables are megabytes: the five whole-run shards stay, the small shards pass through)
def model_traces(chip, log_shard, pos):
    """the reference rows of shard `pos`: computed once, shared by the tests, never written to"""
    from oracle import rv32_model

    chips, pubs = rv32_model.traces(model_run(chip, log_shard), pos)
    for c in chips:
        c["main"].setflags(write=False)
        c["prep"].setflags(write=False)
    pubs.setflags(write=False)
    return chips, pubs


@functools.lru_cache(maxsize=None)
def air_chip(chip):
    from tools.airgen import rv32 as airdef

    machine = airdef.build()
    return next(i for i, c in enumerate(machine.chips) if c.name == chip), next(c for c in machine.chips if c.name == chip)


def chip_rows(chip, traces_of_shard):
    """the real rows of the chip's own table in a shard's traces (columns x rows), or None when the shard has none"""
    cid, cdef = air_chip(chip)
    for c in traces_of_shard:
        if c["chip_id"] == cid:
            real = c["main"][cdef.main_names.index("is_real")] == 1
            return c["main"][:, real]
    return None


def carry_cells(chip, main):
    """{identity: (rows x (K - 1)) matrix of its carry cells W_k + off_k} of the rows `main` (columns x rows) of the chip's table"""
    _, cdef = air_chip(chip)
    col = {n: i for i, n in enumerate(cdef.main_names)}
    out = {}
    for rel in cdef.poly_rels:
        lo = main[[col[f"{rel.name}_w[{k}]"] for k in range(rel.K - 1)]].astype("int64")
        if rel.w_top is not None:
            lo = lo + (main[[col[f"{rel.name}_wb[{k}]"] for k in range(rel.K - 1)]].astype("int64") << 16)
        out[rel.name] = lo.T
    return out
