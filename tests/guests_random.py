"""Seeded random RV32IM guests (tools/rvasm.py): the operands nobody thought of.

random_guest(seed, n, profile) is a straight run of about n random instructions over ten working registers and a 64-word scratch
area, followed by the WRITE / COMMIT ending of tests/guests._finish.  Everything random comes from random.Random(seed), the
program text depends on nothing else, and the generator never executes anything: a "near copy" (a register with exactly one
byte of another changed, which is what makes a comparison be decided by a middle byte) is made by the guest itself with an XOR.

Control flow only moves forward: branches and JALs land 1..5 instructions ahead, on a label that is placed before the ending;
the functions of the `flow` profile lie behind the HALT and a function only calls functions of a higher index.  _assert_forward
checks both on the assembled items, so every program terminates by construction.

What the guests leave out: syscalls other than the ending's WRITE / COMMIT / HALT, precompiles, hints, backward branches, traps.
The only hint is the optional input prologue: with stdin_words = K > 0 the guest first reads one buffer of K words to
tests.guests.HEAP (HINT_LEN, HINT_READ) and copies word k into scratch slot slot_k (lw t3 / sw t3), so that what the random part
loads, compares and branches on depends on the input.  The K distinct slots come from a random.Random of their own, seeded from
the seed: the random part's text does not depend on K, and with K = 0 every byte of the ELF is what it is without the parameter.

CASES is the pinned list the tests run; coverage() computes, from the model's rows alone, what the list is there to contain.
INPUT_CASES is the pinned list of (case, kind, input seed) the divergence tests run on guests with the prologue; inputs_of()
gives an entry's two inputs."""
import collections
import functools
import random

from tests import _profile_ref
from tests.guests import HEAP, _finish
from tools.rvasm import ABI, SYS_HINT_LEN, SYS_HINT_READ, Asm

M32 = 0xFFFFFFFF
EDGES = (0, 1, 2, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x00FFFFFF, 0x01000000, 0x00FF00FF, 0xFF00FF00,
         0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF)
# the ten working registers.  s0 (scratch base), sp and the registers tests/guests._finish names (a0 a1 a2 a4 a5 t0 s1 s8 s9)
# are never destinations in the random part; ra is written by JAL and the calls only, and t3 is the generator's own temporary
# (the constant of a near copy, the address of a table call)
POOL = ("t1", "t2", "a3", "a6", "a7", "s2", "s3", "s4", "s5", "s6")
TMP = "t3"
SCRATCH_WORDS = 64
STACK_WORDS = 64
N_FUNCS = 6
IMMS = (0, 1, -1, 255, 256, 2047, -2048)
SHAMTS = (0, 1, 7, 8, 9, 15, 16, 17, 24, 31)
R_BASE = ("add", "sub", "and_", "or_", "xor", "slt", "sltu")
R_SHIFT = ("sll", "srl", "sra")
R_M = ("mul", "mulh", "mulhsu", "mulhu", "div", "divu", "rem", "remu")
I_ALU = ("addi", "slti", "sltiu", "xori", "ori", "andi")
I_SHIFT = ("slli", "srli", "srai")
LOADS = (("lw", 4), ("lh", 2), ("lhu", 2), ("lb", 1), ("lbu", 1))
STORES = (("sw", 4), ("sh", 2), ("sb", 1))
BRANCHES = ("beq", "bne", "blt", "bge", "bltu", "bgeu")
COMPARES = ("slt", "sltu", "blt", "bge", "bltu", "bgeu")

# every profile has every kind of step; a profile only changes the weights
KINDS = ("r_base", "r_shift", "r_m", "i_alu", "i_shift", "load", "store", "raw", "branch", "jal", "lui", "auipc", "li", "near", "call", "tcall")
WEIGHTS = {
    "mixed":  dict(r_base=14, r_shift=5, r_m=12, i_alu=10, i_shift=5, load=10, store=8, raw=3, branch=10, jal=2, lui=2, auipc=2, li=7, near=10, call=0, tcall=0),
    "alu":    dict(r_base=30, r_shift=0, r_m=0, i_alu=16, i_shift=0, load=0, store=0, raw=0, branch=16, jal=0, lui=3, auipc=2, li=8, near=25, call=0, tcall=0),
    "mem":    dict(r_base=6, r_shift=1, r_m=2, i_alu=4, i_shift=1, load=30, store=24, raw=14, branch=4, jal=1, lui=1, auipc=1, li=7, near=4, call=0, tcall=0),
    "muldiv": dict(r_base=4, r_shift=16, r_m=36, i_alu=3, i_shift=14, load=3, store=2, raw=1, branch=4, jal=1, lui=1, auipc=1, li=9, near=5, call=0, tcall=0),
    "flow":   dict(r_base=10, r_shift=3, r_m=5, i_alu=8, i_shift=3, load=7, store=6, raw=2, branch=16, jal=8, lui=1, auipc=2, li=5, near=8, call=4, tcall=3),
}
PROFILES = tuple(WEIGHTS)
# "alu": the cpu chip's own operations (MUL and MULHU have no other chip)
ALU_R = R_BASE + ("mul", "mulhu")

# (seed, profile, n): every profile, and one long case whose random part fills more than one K0 workgroup of 4096 rows
CASES = ((0, "mixed", 1500), (1, "mixed", 1500), (2, "mixed", 6000), (3, "alu", 1500), (4, "alu", 1500), (5, "mem", 1500), (6, "mem", 1500),
         (7, "muldiv", 1500), (8, "muldiv", 1500), (9, "flow", 1500), (10, "flow", 1500), (11, "flow", 900))
# the cases whose model traces are also put through the constraint checker and the bus balance (a third of the list)
AIR_CASES = CASES[0::3]
# one case of each profile is proven at 2^9; SHORT is the case whose proof bytes are compared with the oracle prover's
PROVE_CASES = ((0, "mixed", 1500), (3, "alu", 1500), (5, "mem", 1500), (7, "muldiv", 1500), (11, "flow", 900))
SHORT = (12, "mixed", 300)


INPUT_WORDS = 16
# (case, kind, seed of the inputs): the case's guest with the input prologue of INPUT_WORDS words, run on the two inputs of
# inputs_of().  "bit": one flipped bit of one word; "other": every word differs.  Every profile, and the long mixed case
# at least once.  The input seeds are chosen so that every split of a chain rejoins: a branch over a `jal ra` leaves the two
# sides at different call depths for good, which the rejoin rule does not match (most input seeds of the flow cases do that)
INPUT_CASES = (((0, "mixed", 1500), "other", 1), ((0, "mixed", 1500), "bit", 1), ((2, "mixed", 6000), "other", 5), ((2, "mixed", 6000), "bit", 4),
               ((3, "alu", 1500), "other", 0), ((5, "mem", 1500), "other", 4), ((5, "mem", 1500), "bit", 1), ((7, "muldiv", 1500), "other", 3),
               ((9, "flow", 1500), "other", 37), ((9, "flow", 1500), "bit", 2))


def case_id(case):
    return "%s-seed%d-n%d" % (case[1], case[0], case[2])


def input_case_id(entry):
    return "%s-%s%d" % (case_id(entry[0]), entry[1], entry[2])


class Guest:
    """elf; scratch = address of the scratch area; random_pcs = [(lo, hi)] pc ranges of the random part (the main run and, for
    flow, the functions behind the HALT); table = address of the jump table (0: none)"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def in_random_part(self, pc):
        return any(lo <= pc < hi for lo, hi in self.random_pcs)


def value(rng):
    """half from the edge list, a fifth an edge value +-1 or +-0x100, the rest 32 random bits"""
    x = rng.random()
    if x < 0.5:
        return rng.choice(EDGES)
    if x < 0.7:
        return (rng.choice(EDGES) + rng.choice((1, -1, 0x100, -0x100))) & M32
    return rng.getrandbits(32)


def _pack(words):
    return b"".join(w.to_bytes(4, "little") for w in words)


def input_of(seed, words=INPUT_WORDS):
    """an input buffer of `words` words: value() from random.Random(seed)"""
    rng = random.Random(seed)
    return _pack([value(rng) for _ in range(words)])


def inputs_of(entry):
    """the two input buffers (INPUT_WORDS little-endian words each) of an entry of INPUT_CASES: A is value() INPUT_WORDS times
    from random.Random(the entry's input seed); B is A with one bit of one word flipped ("bit"), or further value()s each of
    which differs from A's word ("other")"""
    _, kind, seed = entry
    rng = random.Random(seed)
    a = [value(rng) for _ in range(INPUT_WORDS)]
    assert _pack(a) == input_of(seed)
    if kind == "bit":
        b = list(a)
        b[rng.randrange(INPUT_WORDS)] ^= 1 << rng.randrange(32)
    else:
        assert kind == "other"
        b = []
        for w in a:
            x = value(rng)
            while x == w:
                x = value(rng)
            b.append(x)
    return _pack(a), _pack(b)


class _Gen:
    def __init__(self, seed, n, profile, stdin_words=0):
        self.rng = random.Random(seed)
        self.n, self.profile = n, profile
        assert 0 <= stdin_words <= SCRATCH_WORDS
        # a stream of its own: the generator's draws, and so the random part's text, do not depend on stdin_words
        self.slots = random.Random("input slots of seed %d" % seed).sample(range(SCRATCH_WORDS), stdin_words)
        w = WEIGHTS[profile]
        self.kinds, self.weights = list(KINDS), [w[k] for k in KINDS]
        self.a = Asm()
        self.pending = []            # [label, index of the item it must not come before]
        self.n_labels = 0
        self.calls = []              # (item index, function index of the call site or -1 for the main run, callee index)
        self.forward = []            # (item index of a branch / jal, its label)

    # ---- operands
    def dst(self):
        return "zero" if self.rng.random() < 0.06 else self.rng.choice(POOL)

    def src(self, zero=0.06):
        return "zero" if self.rng.random() < zero else self.rng.choice(POOL)

    def imm(self):
        return self.rng.choice(IMMS) if self.rng.random() < 0.875 else self.rng.randrange(-2048, 2048)

    def shamt(self):
        return self.rng.choice(SHAMTS) if self.rng.random() < 10 / 11 else self.rng.randrange(32)

    # ---- forward labels
    def label_ahead(self):
        """a new label that place_labels() puts 1..5 instructions behind the instruction emitted next"""
        name = "L%d" % self.n_labels
        self.n_labels += 1
        self.pending.append([name, len(self.a.items) + self.rng.randrange(1, 6)])
        return name

    def place_labels(self, everything=False):
        """between two steps (a step's instructions stay together): the labels that are due"""
        for p in list(self.pending):
            if everything or len(self.a.items) >= p[1]:
                self.a.label(p[0])
                self.pending.remove(p)

    # ---- steps
    def compare(self, x, y):
        """a comparison of two registers: SLT / SLTU or one of the four ordered branches"""
        op = self.rng.choice(COMPARES)
        if op in ("slt", "sltu"):
            getattr(self.a, op)(self.dst(), x, y)
        else:
            self.branch(op, x, y)

    def branch(self, op, x, y):
        lab = self.label_ahead()
        self.forward.append((len(self.a.items), lab))
        getattr(self.a, op)(x, y, lab)

    def mem_step(self, table, off=None, zero_base=False):
        name, width = self.rng.choice(table)
        if zero_base:                 # rs1 = x0: a word of the low, otherwise unused memory (32 .. 2047)
            return name, "zero", self.rng.randrange(32 // width, 2048 // width) * width
        if off is None:
            off = self.rng.randrange(4 * SCRATCH_WORDS // width) * width
        else:
            off += self.rng.randrange(4 // width) * width
        return name, "s0", off

    def step(self, fn):
        a, rng = self.a, self.rng
        kind = rng.choices(self.kinds, self.weights)[0]
        if kind in ("r_base", "r_shift", "r_m"):
            ops = {"r_base": ALU_R if self.profile == "alu" else R_BASE, "r_shift": R_SHIFT, "r_m": R_M}[kind]
            getattr(a, rng.choice(ops))(self.dst(), self.src(), self.src(0.03))
        elif kind == "i_alu":
            getattr(a, rng.choice(I_ALU))(self.dst(), self.src(), self.imm())
        elif kind == "i_shift":
            getattr(a, rng.choice(I_SHIFT))(self.dst(), self.src(), self.shamt())
        elif kind == "load":
            name, base, off = self.mem_step(LOADS, zero_base=rng.random() < 0.06)
            getattr(a, name)(self.dst(), base, off)
        elif kind == "store":
            name, base, off = self.mem_step(STORES)
            getattr(a, name)(self.src(), base, off)
        elif kind == "raw":           # read after write of the same word through different widths
            word = 4 * rng.randrange(SCRATCH_WORDS)
            name, base, off = self.mem_step(STORES, word)
            getattr(a, name)(self.src(), base, off)
            name, base, off = self.mem_step(LOADS, word)
            getattr(a, name)(self.dst(), base, off)
        elif kind == "branch":
            self.branch(rng.choice(BRANCHES), self.src(), self.src())
        elif kind == "jal":
            lab = self.label_ahead()
            self.forward.append((len(a.items), lab))
            a.jal(rng.choice(("zero", "ra")), lab)
        elif kind == "lui":
            a.lui(self.dst(), rng.getrandbits(20))
        elif kind == "auipc":
            a.auipc(self.dst(), rng.choice((0, 1, 0xFFFFF, 0x80000, rng.getrandbits(20))))
        elif kind == "li":
            a.li(rng.choice(POOL), value(rng))
        elif kind == "near":
            # rd = rs with exactly one byte changed, the byte uniform over 0..3; mostly followed by a comparison of the two
            rd, rs = rng.choice(POOL), rng.choice(POOL)
            byte, delta = rng.randrange(4), rng.randrange(1, 256)
            if byte == 0:
                a.xori(rd, rs, delta)
            else:
                a.li(TMP, delta << (8 * byte))
                a.xor(rd, rs, TMP)
            if rd != rs and rng.random() < 0.8:
                self.compare(*((rd, rs) if rng.random() < 0.5 else (rs, rd)))
        elif kind in ("call", "tcall"):
            callee = rng.randrange(fn + 1, N_FUNCS) if fn + 1 < N_FUNCS else None
            if callee is None:
                a.addi(self.dst(), self.src(), self.imm())
            elif kind == "call":
                self.calls.append((len(a.items), fn, callee))
                a.call("fn%d" % callee)
            else:                     # through the table of function addresses in the data segment
                a.li(TMP, self.table + 4 * callee)
                a.lw(TMP, TMP, 0)
                self.calls.append((len(a.items), fn, callee))
                a.jalr("ra", TMP, 0)
        else:
            raise AssertionError(kind)

    def run(self, count, fn=-1):
        for _ in range(count):
            self.place_labels()
            self.step(fn)
        self.place_labels(everything=True)

    # ---- the program
    def build(self):
        a, rng = self.a, self.rng
        has_funcs = WEIGHTS[self.profile]["call"] + WEIGHTS[self.profile]["tcall"] > 0
        scratch = a.dword("scratch", [value(rng) for _ in range(SCRATCH_WORDS)])
        out = a.dword("out", [0] * len(POOL))
        assert out == scratch + 4 * SCRATCH_WORDS
        stack = a.dword("stack", [0] * STACK_WORDS)
        self.table = a.dword("table", [0] * N_FUNCS) if has_funcs else 0
        a.li("s0", scratch)
        a.li("sp", stack + 4 * STACK_WORDS)
        if self.slots:
            # the input prologue (a0, a1, t0, t3 only): one buffer of len(slots) words to the heap, word k into scratch slot slots[k]
            a.li("t0", SYS_HINT_LEN)
            a.ecall()
            a.li("a0", HEAP)
            a.li("a1", 4 * len(self.slots))
            a.li("t0", SYS_HINT_READ)
            a.ecall()
            for k, slot in enumerate(self.slots):
                a.lw(TMP, "a0", 4 * k)
                a.sw(TMP, "s0", 4 * slot)
        for reg in POOL:
            a.li(reg, value(rng))
        ranges = []
        lo = a.pc()
        body = self.n if not has_funcs else self.n * 3 // 4
        self.run(body)
        ranges.append((lo, a.pc()))
        # the ending: the working registers behind the scratch area, both to fd 1 and their word sum to the public values
        for k, reg in enumerate(POOL):
            a.sw(reg, "s0", 4 * SCRATCH_WORDS + 4 * k)
        _finish(a, scratch, 4 * (SCRATCH_WORDS + len(POOL)))
        if has_funcs:
            # behind the HALT: fn0 .. fn5; each saves ra, runs random steps (calling only functions of a higher index) and returns
            per = (self.n - body) // N_FUNCS
            for f in range(N_FUNCS):
                a.label("fn%d" % f)
                lo = a.pc()
                a.addi("sp", "sp", -4)
                a.sw("ra", "sp", 0)
                self.run(max(per >> f, 4), f)
                a.lw("ra", "sp", 0)
                a.addi("sp", "sp", 4)
                a.ret()
                ranges.append((lo, a.pc()))
                a.data[(self.table - a.data_base) // 4 + f] = a.labels["fn%d" % f]
        self._assert_forward()
        return Guest(elf=a.elf(), scratch=scratch, out=out, table=self.table, random_pcs=ranges, seed=None, slots=tuple(self.slots))

    def _assert_forward(self):
        """termination by construction: every branch and JAL of the random part lands behind itself, at most five instructions
        (plus the step they fall into) ahead and before the ending; a function only calls functions of a higher index, and
        the deepest chain of calls fits the stack"""
        a = self.a
        assert not self.pending
        for idx, lab in self.forward:
            here, there = a.text_base + 4 * idx, a.labels[lab]
            assert here < there <= here + 4 * 8, (idx, lab)
        for idx, fn, callee in self.calls:
            assert fn < callee < N_FUNCS
        assert N_FUNCS + 1 <= STACK_WORDS


def build(seed, n=1500, profile="mixed", stdin_words=0):
    """the guest of that seed; stdin_words = K > 0: with the input prologue, to be run on one buffer of 4 K bytes"""
    g = _Gen(seed, n, profile, stdin_words).build()
    g.seed, g.profile, g.n, g.stdin_words = seed, profile, n, stdin_words
    return g


def random_guest(seed, n=1500, profile="mixed", stdin_words=0):
    """the ELF of the guest of that seed: the same bytes on every machine"""
    return build(seed, n, profile, stdin_words).elf


# ---------------------------------------------------------------------------------------------- reading a row
def disassemble(ins):
    """the instruction of a model row (oracle.rv32_model.Ins) as text: _profile_ref.mnemonic plus its registers and immediate"""
    m = _profile_ref.mnemonic(ins.word)
    rd, rs1, rs2 = ABI[(ins.word >> 7) & 31], ABI[(ins.word >> 15) & 31], ABI[(ins.word >> 20) & 31]
    sx = lambda v: v - (1 << 32) if v >> 31 else v
    op = ins.word & 0x7F
    if op == 0x33:
        return "%s %s, %s, %s" % (m, rd, rs1, rs2)
    if op == 0x13:
        return "%s %s, %s, %d" % (m, rd, rs1, (ins.word >> 20) & 31 if m in ("slli", "srli", "srai") else sx(ins.imm))
    if op == 0x03:
        return "%s %s, %d(%s)" % (m, rd, sx(ins.off), rs1)
    if op == 0x23:
        return "%s %s, %d(%s)" % (m, rs2, sx(ins.off), rs1)
    if op == 0x63:
        return "%s %s, %s, 0x%x" % (m, rs1, rs2, ins.tgt)
    if op == 0x6F:
        return "%s %s, 0x%x" % (m, rd, ins.tgt)
    if op == 0x67:
        return "%s %s, %d(%s)" % (m, rd, sx(ins.off), rs1)
    if op in (0x37, 0x17):
        return "%s %s, 0x%x" % (m, rd, ins.word >> 12)
    return m


def describe(run, shard, row):
    """the instruction of row `row` of the cpu table of the model's shard at position `shard` and its operand values; a padding
    row, or a row of a table with more rows than the shard has cycles, says so"""
    rows = run.shards[shard]["rows"]
    if row >= len(rows):
        return "(no instruction: the shard has %d cycles)" % len(rows)
    r = rows[row]
    text = "pc 0x%08x: %s  [rs1 = 0x%08x, rs2/imm = 0x%08x, rd <- 0x%08x, next pc 0x%08x" % (r.ins.pc, disassemble(r.ins), r.b, r.c, r.a, r.next_pc)
    if r.ins.kind in ("lb", "lbu", "lh", "lhu", "lw", "sb", "sh", "sw"):
        text += ", address 0x%08x, word 0x%08x -> 0x%08x" % (r.maddr, r.m_prev, r.m_val)
    return text + "]"


@functools.lru_cache(maxsize=None)
def chip_names():
    """chip id -> (name, main column names) of the rv32 machine, from the AIR's description"""
    from tools.airgen import rv32

    return {i: (c.name, list(c.main_names)) for i, c in enumerate(rv32.build().chips)}


def first_difference(case, log_shard, run, shard, got, want, part="main", who="device"):
    """None when the table `got` of one chip equals the model's `want`; else the message of the first differing cell: seed,
    profile, shard, chip, column name, row, both values and, for the cpu table, the instruction of that row.  The rows of the
    other tables follow their own order; the message then names the cpu row of the same index only as a place to start."""
    import numpy as np

    name, cols = chip_names()[want["chip_id"]]
    if got[part].shape != want[part].shape:
        return "seed %d profile %s n %d at 2^%d, shard %d chip %s %s: shape %s, the model's %s" % (
            case[0], case[1], case[2], log_shard, shard, name, part, got[part].shape, want[part].shape)
    diff = np.argwhere(got[part] != want[part])
    if diff.size == 0:
        return None
    # the first differing row, and the first differing column of it
    c, r = min(((int(c), int(r)) for c, r in diff), key=lambda cr: (cr[1], cr[0]))
    col = cols[c] if part == "main" and c < len(cols) else "%s[%d]" % (part, c)
    where = describe(run, shard, r) if name == "cpu" else "(row %d of the %s table)" % (r, name)
    return "seed %d profile %s n %d at 2^%d, shard %d chip %s column %s row %d: %s has %d, the model %d; %d cells of the table differ; %s" % (
        case[0], case[1], case[2], log_shard, shard, name, col, r, who, int(got[part][c, r]), int(want[part][c, r]), len(diff), where)


# ---------------------------------------------------------------------------------------------- what the list is there for
MNEMONICS = ("lui", "auipc", "jal", "jalr", "beq", "bne", "blt", "bge", "bltu", "bgeu", "lb", "lh", "lw", "lbu", "lhu", "sb", "sh", "sw",
             "addi", "slti", "sltiu", "xori", "ori", "andi", "slli", "srli", "srai", "add", "sub", "sll", "slt", "sltu", "xor", "srl", "sra",
             "or", "and", "mul", "mulh", "mulhsu", "mulhu", "div", "divu", "rem", "remu")


def _byts(w):
    return [(w >> (8 * i)) & 0xFF for i in range(4)]


def coverage(guest, run, into=None):
    """the counters of one guest, from the model's rows of its random part alone (added to `into` when given): a Counter
    whose keys are tuples such as ("op", "sltu"), ("decided", "blt", 2), ("taken", "beq", True), ("carry", "add", "byte0"),
    ("mul", "mulhu", "both_high"), ("offset", "sb", 3), ("sign", "lh", 1), ("rd_x0", "load")"""
    cov = collections.Counter() if into is None else into
    sx = lambda v: v - (1 << 32) if v >> 31 else v
    for sh in run.shards:
        for r in sh["rows"]:
            if not guest.in_random_part(r.ins.pc):
                continue
            w = r.ins.word
            m = _profile_ref.mnemonic(w)
            op = w & 0x7F
            cov[("op", m)] += 1
            base = {"slti": "slt", "sltiu": "sltu"}.get(m, m)
            if base in COMPARES:
                b, c = _byts(r.b), _byts(r.c)
                top = next((i for i in (3, 2, 1, 0) if b[i] != c[i]), "equal")
                cov[("decided", base, top)] += 1
            if op == 0x63:
                cov[("taken", m, r.next_pc == r.ins.tgt)] += 1
            if m in ("add", "sub", "addi"):
                # the byte carries of b + c (ADD) or of a + c (SUB: the borrows of b - c)
                x, cy, out = (r.a if m == "sub" else r.b), 0, []
                for i in range(4):
                    cy = (_byts(x)[i] + _byts(r.c)[i] + cy) >> 8
                    out.append(cy)
                which = {(1, 0, 0, 0): "byte0", (1, 1, 1, 1): "every", (0, 0, 0, 0): "none"}.get(tuple(out))
                if which and m != "addi":
                    cov[("carry", m, which)] += 1
            if m in ("mul", "mulhu"):
                if r.b >> 31 and r.c >> 31:
                    cov[("mul", m, "both_high")] += 1
                if (r.b == 0) != (r.c == 0):
                    cov[("mul", m, "one_zero")] += 1
            if m in ("sb", "sh", "lb", "lbu", "lh", "lhu"):
                cov[("offset", m, r.maddr & 3)] += 1
            if m in ("lb", "lh"):
                cov[("sign", m, r.a >> 31)] += 1
            form = {0x33: "rtype", 0x13: "itype", 0x03: "load"}.get(op)
            if form:
                if (w >> 7) & 31 == 0:
                    cov[("rd_x0", form)] += 1
                if (w >> 15) & 31 == 0:
                    cov[("rs1_x0", form)] += 1
    return cov


def required():
    """the keys every one of which the pinned list must reach (("op", m): at least 20 times; every other: at least once)"""
    keys = [("op", m) for m in MNEMONICS]
    keys += [("decided", op, top) for op in COMPARES for top in (3, 2, 1, 0, "equal")]
    keys += [("taken", op, t) for op in BRANCHES for t in (True, False)]
    keys += [("carry", op, which) for op in ("add", "sub") for which in ("byte0", "every", "none")]
    keys += [("mul", op, which) for op in ("mul", "mulhu") for which in ("both_high", "one_zero")]
    keys += [("offset", "sb", k) for k in range(4)] + [("offset", "lb", k) for k in range(4)] + [("offset", "lbu", k) for k in range(4)]
    keys += [("offset", op, k) for op in ("sh", "lh", "lhu") for k in (0, 2)]
    keys += [("sign", op, s) for op in ("lb", "lh") for s in (0, 1)]
    keys += [(what, form) for what in ("rd_x0", "rs1_x0") for form in ("rtype", "itype", "load")]
    return keys


def missing(cov):
    return [k for k in required() if cov[k] < (20 if k[0] == "op" else 1)]


def random_span(guest, run):
    """(first, one past the last) global record number of the main run's random part"""
    lo, hi = guest.random_pcs[0]
    rows = [r.ins.pc for sh in run.shards for r in sh["rows"]]
    first = next(g for g, pc in enumerate(rows) if lo <= pc < hi)
    return first, next(g for g in range(first, len(rows)) if rows[g] == hi)
