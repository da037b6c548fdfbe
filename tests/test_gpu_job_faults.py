"""GPU tests of the job-level code on jobs that are NOT honest: dvt_rv32_check_job (job_check of csrc/capi_inspect.hip),
dvt_rv32_job_bus_tuples on a whole job, and the rv32 proving path (K0 from the job's tables, phase 1, the common challenges,
phase 2) on a job with a planted wrong cell (dvt_rv32_debug_poke_cell, Prover.debug_poke_cell).

Every expectation is the oracle's.  After a poke the tables the job now yields are downloaded (debug_device_traces, which runs
K0 again from the poked tables) and must differ from the download before it in exactly the poked cell, by `add`; from those
canonical matrices and the preprocessed columns of the host traces the generated C constraints give the per-unit violation
counts, their sum and the first (row, unit) of every table (tests/_check_expect.py), and the exact LogUp multiset gives the
tuples that no longer cancel (ex.air("rv32").logup_unbalanced, asked once per tuple: each answer is handed back as a receive of
its net multiplicity until nothing is left).  The proofs are judged by the host verifier.

Shapes: the three-shard commit_only job at 2^11 cycles per shard (chips 0..3 and shift in every shard, mem_init in the last; on
"devices": [0, 0] shards 0 and 2 are on member 0 and shard 1 on member 1), and the six small single-shard guests that reach
all 14 chips between them (the `honest` fixture of tests/test_gpu_check_constraints.py).

The poked cells are constants (JOB3, GUEST_CELLS), found by a seeded search on the CPU over the honest host traces, like
_forger.DELTAS; every test asserts the pattern of its cell on the tables it downloaded ("stale constant" otherwise).
`python -m tests.test_gpu_job_faults --search` repeats the search without a GPU and prints both tables.  The patterns: "VU" the
cell violates at least one constraint and unbalances a bus; "V" it violates a constraint and unbalances nothing (mem_image's
one main column `pad` is such a cell, and the only kind mem_image has: no interaction reads it); "U" it violates nothing and
unbalances a bus (a multiplicity of byte or program: no constraint reads one).

The cpu chip's rows are rebuilt from the cycle records by every K0 and records are never altered, so a wrong cpu row reaches
the job check and the ledger only through a kept K0 output (test_kept_traces_are_really_reused) and never reaches a proof; wrong
cpu rows in proofs are covered at stage level (tests/test_gpu_check_constraints.py, test_gpu_bus_ledger.py, the verifier's
forgery tests)."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

from tests import _check_expect as ex
from tests import guests
from tests.test_gpu_bus_ledger import is_the_oracles_set, occurrences, ordered, where_it_occurs
from tests.test_rv32_exec_trace import pv_extra

pytestmark = pytest.mark.gpu
P = 2013265921
Q, POW = 8, 4
CFG = '"fri_queries": %d, "pow_bits": %d' % (Q, POW)
PV = b"check me"
PROGRAM, BYTE, CPU, MEM_IMAGE, MEM_INIT, SHIFT, MULDIV = 0, 1, 2, 3, 4, 5, 6
SEARCH_SEED, SEARCH_TRIES = 20261, 64

GUESTS = {
    "shifts": lambda: guests.shifts()[0],
    "muldiv": lambda: guests.muldiv()[0],
    "sha256": lambda: guests.sha256_precompiled(bytes(range(150)))[0],
    "field_ops": lambda: guests.field_ops()[0],
    "curve_ops": lambda: guests.curve_ops()[0],
    "u256_ops": lambda: guests.u256_ops()[0],
}

# ---- what the search found: (shard, chip, col, row, add, pattern)
JOB3 = {
    "image_s0": (0, 3, 0, 50, 1, "V"),
    "image_s1": (1, 3, 0, 228, 1, "V"),
    "image_s2": (2, 3, 0, 368, 1, "V"),
    "shift_s1": (1, 5, 16, 151, 1, "VU"),
    "init_s2": (2, 4, 3, 347, 1, "VU"),
    "byte_hot": (0, 1, 5, 0, 1, "U"),
    "cpu_s1": (1, 2, 40, 1846, 1, "VU"),
}
# guest -> chip -> (col, row, add, pattern): every table the job holds but cpu's
GUEST_CELLS = {
    "shifts": {0: (0, 605, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 202, 1, "V"), 4: (1, 1333, 1, "VU"), 5: (15, 1113, 1, "U")},
    "muldiv": {0: (0, 2423, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 809, 1, "V"), 4: (1, 5335, 1, "VU"), 5: (15, 1113, 1, "U"), 6: (7, 637, 1, "VU")},
    "sha256": {0: (0, 151, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 101, 1, "V"), 4: (1, 666, 1, "VU"), 5: (15, 1113, 1, "U"), 7: (86, 101, 1, "V"), 8: (85, 31, 1, "V")},
    "field_ops": {0: (0, 605, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 404, 1, "V"), 4: (1, 2667, 1, "VU"), 5: (15, 1113, 1, "U"), 9: (409, 11, 1, "VU"), 10: (736, 3, 1, "VU")},
    "curve_ops": {0: (0, 302, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 202, 1, "V"), 4: (18, 1143, 1, "VU"), 5: (15, 1113, 1, "U"), 11: (909, 6, 1, "V"), 12: (23, 3, 1, "VU")},
    "u256_ops": {0: (0, 302, 1, "U"), 1: (6, 26443, 1, "U"), 3: (0, 202, 1, "V"), 4: (18, 1143, 1, "VU"), 5: (15, 1113, 1, "U"), 13: (161, 2, 1, "VU")},
}


# ------------------------------------------------------------------ the CPU side: host traces, the oracle's verdict, the search
@functools.lru_cache(maxsize=None)
def host_job(name):
    """the honest tables of a job from the host alone: dict(elf, log_shard, pv, extra, shards = [(chips, pubs)])"""
    from dvt_circuits_amd import capi

    elf, log_shard = (guests.commit_only(PV), 11) if name == "commit3" else (GUESTS[name](), 21)
    rc, _, pv, err = capi.execute(elf)
    assert rc == 0, err
    shards, s, n = [], 0, 1
    while s < n:
        chips, pubs, n = capi.rv32_debug_traces(elf, [], log_shard, s)
        shards.append(([dict(chip_id=c["chip_id"], main=np.ascontiguousarray(c["main"]), prep=np.ascontiguousarray(c["prep"])) for c in chips],
                       [int(x) for x in pubs]))
        s += 1
    return dict(name=name, elf=elf, log_shard=log_shard, pv=pv, extra=pv_extra(pv), shards=shards)


def table(groups, shard, chip):
    return next(c for c in groups[shard][0] if c["chip_id"] == chip)


def with_cells(groups, pokes):
    """the groups with `add` added to every poked cell (mod p); pokes: (shard, chip, col, row, add)"""
    out = [([dict(c) for c in chips], pubs) for chips, pubs in groups]
    done = set()
    for shard, chip, col, row, add in pokes:
        t = table(out, shard, chip)
        if (shard, chip) not in done:
            t["main"] = t["main"].copy()
            done.add((shard, chip))
        t["main"][col, row] = (int(t["main"][col, row]) + add) % P
    return out


def oracle_findings(groups, pokes):
    """what check_job must report, sorted by (shard, chip): the rows that read a poked cell are its own and the one before
    it; every other row is honest (the honest job is clean under the oracle: honest_is_clean)"""
    rows = {}
    for shard, chip, col, row, add in pokes:
        rows.setdefault((shard, chip), set()).update((row - 1, row))
    found = []
    for (shard, chip), rr in sorted(rows.items()):
        t, pubs = table(groups, shard, chip), groups[shard][1]
        by_row = ex.violated_units("rv32", chip, t["main"], t["prep"], pubs, rows=rr)
        _, total, row, unit = ex.expectation("rv32", chip, by_row)
        if total:
            found.append(dict(shard=shard, chip=chip, log_n=t["main"].shape[1].bit_length() - 1, violations=total, first_row=row, first_constraint=unit))
    return found


def oracle_tuples(groups, extra, limit=64):
    """the oracle's unbalanced tuples [(bus, values, net)], one question per tuple"""
    air, back, out = ex.air("rv32"), list(extra), []
    while True:
        n, first = air.logup_unbalanced(groups, extra=back)
        if not n:
            return out
        assert len(out) < limit, f"more than {limit} unbalanced tuples"
        bus, arity, net, vals = first[0], first[1], first[2], first[3:]
        assert len(vals) == arity
        out.append((bus, vals, net))
        back.append((bus, vals, -1, net))


def pattern_of(groups, extra, poke):
    """"VU" / "V" / "U" / "" of one poke on otherwise honest groups"""
    forged = with_cells(groups, [poke])
    v = bool(oracle_findings(forged, [poke]))
    u = ex.air("rv32").logup_unbalanced(forged, extra=extra)[0] > 0
    return ("V" if v else "") + ("U" if u else "")


def honest_is_clean(groups, extra):
    air = ex.air("rv32")
    for chips, pubs in groups:
        for c in chips:
            n = c["main"].shape[1]
            assert air.check_constraints(c["chip_id"], c["main"], c["prep"] if c["prep"].shape[0] else np.zeros((1, n), np.uint32), pubs)[0] == 0
    assert air.logup_unbalanced(groups, extra=extra)[0] == 0


def search_cell(job, shard, chip, want):
    """the first seeded cell of that table whose + 1 shows a pattern in `want`: (col, row, 1, pattern) or None"""
    t = table(job["shards"], shard, chip)
    rng = np.random.default_rng([SEARCH_SEED, shard, chip])
    for _ in range(SEARCH_TRIES):
        col, row = int(rng.integers(t["main"].shape[0])), int(rng.integers(t["main"].shape[1]))
        pat = pattern_of(job["shards"], job["extra"], (shard, chip, col, row, 1))
        if pat in want:
            return col, row, 1, pat
    return None


def hot_byte_cell(job, shard):
    byte = table(job["shards"], shard, BYTE)["main"]
    col, row = np.unravel_index(int(np.argmax(byte)), byte.shape)
    return int(col), int(row), 1, pattern_of(job["shards"], job["extra"], (shard, BYTE, int(col), int(row), 1))


def search_job3():
    job = host_job("commit3")
    out = {}
    for s in range(3):
        out[f"image_s{s}"] = (s, MEM_IMAGE) + search_cell(job, s, MEM_IMAGE, ("V",))
    out["shift_s1"] = (1, SHIFT) + search_cell(job, 1, SHIFT, ("VU",))
    out["init_s2"] = (2, MEM_INIT) + search_cell(job, 2, MEM_INIT, ("VU",))
    out["byte_hot"] = (0, BYTE) + hot_byte_cell(job, 0)
    out["cpu_s1"] = (1, CPU) + search_cell(job, 1, CPU, ("VU",))
    return out


def search_guest(name):
    job = host_job(name)
    assert len(job["shards"]) == 1
    return {c["chip_id"]: search_cell(job, 0, c["chip_id"], ("VU", "V", "U")) for c in job["shards"][0][0] if c["chip_id"] != CPU}


# ------------------------------------------------------------------ the GPU side
class Job:
    """a prepared job on a handle of its own, with the host's honest tables"""

    def __init__(self, name, cfg_extra="", **prepare):
        from dvt_circuits_amd import capi

        self.host = host_job(name)
        self.p = capi.Prover('{%s, "log_shard_size": %d%s}' % (CFG, self.host["log_shard"], cfg_extra))
        self.pk, self.vk = self.p.setup(self.host["elf"])
        self.job, _ = self.p.prepare(self.pk, [], **prepare)
        assert self.p.job_shards(self.job) == len(self.host["shards"])

    def close(self):
        self.p.job_free(self.job)
        self.p.pk_free(self.pk)
        self.p.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def poke(self, shard, chip, col, row, add):
        self.p.debug_poke_cell(self.job, shard, chip, col, row, add)

    def download(self, shards=None):
        """the tables the job now yields (K0 again), with the host's preprocessed columns: {shard: (chips, pubs)}"""
        out = {}
        for s in range(len(self.host["shards"])) if shards is None else shards:
            dev, pubs = self.p.debug_device_traces(self.pk, self.job, s)
            hchips, hpubs = self.host["shards"][s]
            assert [c["chip_id"] for c in dev] == [c["chip_id"] for c in hchips] and [int(x) for x in pubs] == hpubs
            out[s] = ([dict(chip_id=d["chip_id"], main=np.ascontiguousarray(d["main"]), prep=h["prep"]) for d, h in zip(dev, hchips)], hpubs)
        return out

    def check(self, cap=256):
        return self.p.check_job(self.pk, self.job, cap)

    def tuples(self):
        return self.p.job_bus_tuples(self.pk, self.job)

    def prove(self):
        return self.p.prove_job(self.pk, self.job)


def only_these_cells_differ(before, after, pokes):
    """exactly the poked cells differ between two downloads, each by its add; returns the groups after, in shard order"""
    want = {}
    for shard, chip, col, row, add in pokes:
        want[shard, chip, col, row] = (want.get((shard, chip, col, row), 0) + add) % P
    seen = set()
    for s in after:
        for b, a in zip(before[s][0], after[s][0]):
            for col, row in zip(*np.nonzero(b["main"] != a["main"])):
                key = (s, a["chip_id"], int(col), int(row))
                assert key in want, f"cell {key} changed without a poke"
                assert (int(a["main"][col, row]) - int(b["main"][col, row])) % P == want[key], key
                seen.add(key)
    assert seen == {k for k, v in want.items() if v}, "a poked cell did not change"
    return [after[s] for s in sorted(after)]


def clean(summary, findings, bus_checked=1):
    assert summary["ok"] and summary["error"] == "" and summary["violations"] == 0 and summary["n_findings"] == 0 and findings == [], summary
    assert summary["bus_checked"] == bus_checked and summary["unbalanced_buses"] == 0, summary


def bus_mask(tuples):
    m = 0
    for bus, _, _ in tuples:
        m |= 1 << bus
    return m


def is_the_oracles_verdict(j, groups, pokes, summary, findings, where, whole=True):
    """summary and findings of check_job against the oracle on `groups`; returns (expected findings, oracle tuples)"""
    want = oracle_findings(groups, pokes)
    tuples = oracle_tuples(groups, j.host["extra"]) if whole else []
    print(f"{where}: GPU {summary} {findings}; oracle findings {want}, unbalanced tuples {tuples}")
    assert findings == want, where
    assert summary["n_findings"] == len(want) and summary["violations"] == sum(f["violations"] for f in want), where
    assert summary["bus_checked"] == int(whole) and summary["unbalanced_buses"] == bus_mask(tuples), where
    assert summary["ok"] == (not want and not tuples), where
    if want:
        f = want[0]
        text = "shard %d, chip %s: row %d violates constraint %d (%d violations in %d chip tables)" % (
            f["shard"], ex.chip("rv32", f["chip"])["name"], f["first_row"], f["first_constraint"], summary["violations"], len(want))
        assert summary["error"] == text, where
    elif tuples:
        assert summary["error"] == "the LogUp sums of the job do not balance (bus mask 0x%x)" % bus_mask(tuples), where
    return want, tuples


def are_the_oracles_tuples(j, groups, where):
    got, truncated = j.tuples()
    assert not truncated and ordered(got), where
    is_the_oracles_set(groups, j.host["extra"], got, where)
    return got


def stale(name, pat, want):
    assert pat == want, f"stale constant: {name} shows pattern {pat!r}, not {want!r}: run python -m tests.test_gpu_job_faults --search"


@functools.lru_cache(maxsize=None)
def honest_proof(name):
    """the bytes of a handle that never poked, accepted by the host verifier"""
    from dvt_circuits_amd import capi

    with Job(name) as j:
        proof = j.prove()
        ok, ec, pv, why = capi.verify(j.vk, proof, Q, POW)
        assert ok and ec == 0 and pv == j.host["pv"], why
    return proof


# ------------------------------------------------------------------ 1: one finding
@pytest.mark.parametrize("cfg_extra", ("", ', "devices": [0, 0]'), ids=("one_member", "two_members"))
@pytest.mark.parametrize("cell", ("image_s1", "shift_s1"))
def test_one_wrong_cell_is_one_finding(cell, cfg_extra):
    """the aux chips of shard 1 (not the first shard; on "devices": [0, 0] the one shard of member 1, so that finding and bus
    sums are member 1's alone): mem_image, whose cells are "V", and shift, which has the "VU" cell: finding, bus mask and the
    ledger's tuples at once"""
    shard, chip, col, row, add, pat = JOB3[cell]
    poke = (shard, chip, col, row, add)
    with Job("commit3", cfg_extra) as j:
        assert j.p.job_shard_member(j.job, shard) == (1 if cfg_extra else 0)
        honest_is_clean(j.host["shards"], j.host["extra"])
        clean(*j.check())
        before = j.download()
        j.poke(*poke)
        groups = only_these_cells_differ(before, j.download(), [poke])
        summary, findings = j.check()
        want, tuples = is_the_oracles_verdict(j, groups, [poke], summary, findings, cell)
        stale(cell, ("V" if want else "") + ("U" if tuples else ""), pat)
        assert len(want) == 1 and not summary["ok"]
        f = want[0]
        for part in ("shard %d," % shard, "chip %s:" % ex.chip("rv32", chip)["name"], "row %d " % f["first_row"], "constraint %d " % f["first_constraint"]):
            assert part in summary["error"], (part, summary["error"])
        got = are_the_oracles_tuples(j, groups, cell)
        assert len(got) == len(tuples) and {t["bus"] for t in got} == {b for b, _, _ in tuples}
        # every tuple occurs on the rows that read the poked cell, in the poked table or in the honest one (the partner that lost its match)
        t_poked, t_honest, pubs = table(groups, shard, chip), table(j.host["shards"], shard, chip), groups[shard][1]
        occ = [occurrences("rv32", chip, t["main"], t["prep"], pubs) for t in (t_poked, t_honest)]
        n = t_poked["main"].shape[1]
        for t in got:
            assert any(r in ((row - 1) % n, row) for o in occ for r, _, _ in where_it_occurs(o, t)), t


# ------------------------------------------------------------------ 2: balance only
def test_a_byte_multiplicity_unbalances_one_bus_and_violates_nothing():
    shard, chip, col, row, add, pat = JOB3["byte_hot"]
    poke = (shard, chip, col, row, add)
    byte_bus = ex.description("rv32").buses["byte"]
    with Job("commit3") as j:
        hot = table(j.host["shards"], shard, chip)["main"]
        assert (col, row) == np.unravel_index(int(np.argmax(hot)), hot.shape), "stale constant: byte_hot is not the hottest byte row"
        before = j.download()
        j.poke(*poke)
        groups = only_these_cells_differ(before, j.download(), [poke])
        summary, findings = j.check()
        want, tuples = is_the_oracles_verdict(j, groups, [poke], summary, findings, "byte_hot")
        stale("byte_hot", ("V" if want else "") + ("U" if tuples else ""), pat)
        assert findings == [] and summary["violations"] == 0 and summary["n_findings"] == 0 and not summary["ok"]
        assert len(tuples) == 1 and summary["unbalanced_buses"] == 1 << tuples[0][0]
        assert tuples[0][0] == byte_bus
        assert summary["error"] == "the LogUp sums of the job do not balance (bus mask 0x%x)" % (1 << tuples[0][0])
        got = are_the_oracles_tuples(j, groups, "byte_hot")
        assert len(got) == 1 and (got[0]["first_tag"], got[0]["first_chip"], got[0]["first_row"]) == (0, 1, row), got
        assert (got[0]["bus"], got[0]["values"], got[0]["net"]) == tuples[0]


# ------------------------------------------------------------------ 3, 4: several findings, their order, cap; two members
SEVERAL = ("init_s2", "image_s2", "image_s0", "image_s1")   # shard 2 (two chips, the higher id first), shard 0, shard 1


@functools.lru_cache(maxsize=None)
def several(cfg_extra):
    """the answers of a job poked in four tables, each compared with the oracle"""
    from dvt_circuits_amd import capi

    pokes = [JOB3[k][:5] for k in SEVERAL]
    with Job("commit3", cfg_extra) as j:
        members = [j.p.job_shard_member(j.job, s) for s in range(3)]
        before = j.download()
        for poke in pokes:
            j.poke(*poke)
        groups = only_these_cells_differ(before, j.download(), pokes)
        summary, findings = j.check()
        want, tuples = is_the_oracles_verdict(j, groups, pokes, summary, findings, f"four tables{cfg_extra}")
        assert [(f["shard"], f["chip"]) for f in want] == [(0, 3), (1, 3), (2, 3), (2, 4)] and tuples, "stale constants"
        # cap = 1, in an array with room for eight: one finding written, all counted, the rest of the array untouched
        arr, s1 = (capi.CheckFinding * 8)(), capi.CheckSummary()
        C.memset(arr, 0xA5, C.sizeof(arr))
        rc = j.p.lib.dvt_rv32_check_job(j.p.h, j.pk, j.job, arr, 1, C.byref(s1))
        text = j.p.lib.dvt_last_error(j.p.h).decode()
        assert rc == capi.DVT_ERR_REJECTED and s1.n_findings == 4 and s1.violations == summary["violations"]
        assert (arr[0].shard, arr[0].chip, arr[0].log_n, arr[0].r.violations, arr[0].r.first_row, arr[0].r.first_constraint) == tuple(want[0].values())
        assert bytes(arr)[C.sizeof(capi.CheckFinding):] == b"\xa5" * (7 * C.sizeof(capi.CheckFinding)), "findings written past cap"
        assert text == summary["error"]
        capped, one = j.check(cap=1)
        assert one == want[:1] and capped["n_findings"] == 4
        # cap = 0 and no array: the summary alone
        s0 = capi.CheckSummary()
        rc = j.p.lib.dvt_rv32_check_job(j.p.h, j.pk, j.job, None, 0, C.byref(s0))
        assert rc == capi.DVT_ERR_REJECTED and j.p.lib.dvt_last_error(j.p.h).decode() == summary["error"]
        assert (s0.violations, s0.n_findings, s0.bus_checked, s0.unbalanced_buses) == (s1.violations, 4, 1, summary["unbalanced_buses"])
        assert (s1.bus_checked, s1.unbalanced_buses) == (1, summary["unbalanced_buses"])
        got = are_the_oracles_tuples(j, groups, f"four tables{cfg_extra}")
    return dict(members=members, summary={k: v for k, v in summary.items() if k != "ms"}, findings=findings, tuples=got)


def test_several_findings_come_sorted_and_capped():
    a = several("")
    assert a["members"] == [0, 0, 0]
    f0 = a["findings"][0]
    assert a["summary"]["error"].startswith("shard 0, chip mem_image: row %d violates constraint %d " % (f0["first_row"], f0["first_constraint"]))


def test_two_members_give_the_same_answers():
    two = several(', "devices": [0, 0]')
    assert two["members"] == [0, 1, 0]
    one = several("")
    assert two["summary"] == one["summary"] and two["findings"] == one["findings"] and two["tuples"] == one["tuples"]


# ------------------------------------------------------------------ 5: a partial job
def test_a_partial_job_reports_the_finding_without_the_balance():
    """shards 0 and 2 of 3; the "VU" cell of mem_init in shard 2: the finding, and no word about buses"""
    poke = JOB3["init_s2"][:5]
    with Job("commit3", first=0, stride=2) as j:
        assert [j.p.job_shard_member(j.job, s) for s in range(3)] == [0, -1, 0]
        clean(*j.check(), bus_checked=0)
        before = j.download((0, 2))
        j.poke(*poke)
        after = j.download((0, 2))
        only_these_cells_differ(before, after, [poke])
        groups = [after[0], j.host["shards"][1], after[2]]   # (shard 1 is not held: nothing of it is read)
        summary, findings = j.check()
        want, _ = is_the_oracles_verdict(j, groups, [poke], summary, findings, "shards 0 and 2 of 3", whole=False)
        assert len(want) == 1 and (summary["bus_checked"], summary["unbalanced_buses"]) == (0, 0) and not summary["ok"]


# ------------------------------------------------------------------ 6: kept traces
def test_kept_traces_are_really_reused():
    """A cpu cell exists only in the K0 output phase 1 kept: the check and the ledger see the poke exactly while they reuse
    that buffer, and no longer after the shard's next K0.  The expected table is the honest one with the cell changed."""
    from dvt_circuits_amd import capi

    shard, chip, col, row, add, pat = JOB3["cpu_s1"]
    poke = (shard, chip, col, row, add)
    with Job("commit3") as j:
        assert j.p.job_shard_kept(j.job, shard) == capi.DVT_KEEP_FULL
        j.poke(*poke)
        groups = with_cells(j.host["shards"], [poke])
        for again in range(2):   # (the check leaves the kept buffer valid: the second reader sees the same)
            summary, findings = j.check()
            want, tuples = is_the_oracles_verdict(j, groups, [poke], summary, findings, f"cpu cell in the kept K0 output, check {again}")
        stale("cpu_s1", ("V" if want else "") + ("U" if tuples else ""), pat)
        assert [(f["shard"], f["chip"]) for f in want] == [(shard, CPU)]
        got = are_the_oracles_tuples(j, groups, "cpu cell in the kept K0 output")
        assert got
        # K0 again: the honest rows, cell for cell
        after = j.download((shard,))[shard][0]
        for a, h in zip(after, j.host["shards"][shard][0]):
            assert (a["main"] == h["main"]).all(), a["chip_id"]
        clean(*j.check())
        assert j.tuples() == ([], False)
        assert j.prove() == honest_proof("commit3")
    with Job("commit3", ', "keep_phase1": 0') as j:
        with pytest.raises(capi.DvtError) as e:
            j.poke(*poke)
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED
        clean(*j.check())
        assert j.prove() == honest_proof("commit3")


# ------------------------------------------------------------------ 7: no wrong table is provable
@pytest.mark.parametrize("name", list(GUESTS))
def test_no_wrong_table_is_provable(name):
    """Every table the job holds but cpu's (cpu is exempt: its poke does not survive the K0 of phase 1), one wrong cell at a
    time; between the six guests that is every chip but cpu (tests/test_job_faults_search.py asserts the union): the check rejects, prove_job raises or returns bytes both verifiers reject with one reason; after the undo the handle
    proves the honest bytes."""
    from dvt_circuits_amd import capi

    cells = GUEST_CELLS[name]
    with Job(name) as j:
        chips = [c["chip_id"] for c in j.host["shards"][0][0] if c["chip_id"] != CPU]
        assert sorted(cells) == chips, f"stale constants: {name} holds the chips {chips}"
        honest_is_clean(j.host["shards"], j.host["extra"])
        clean(*j.check())
        before = j.download()
        for chip in chips:
            col, row, add, pat = cells[chip]
            poke = (0, chip, col, row, add)
            where = f"{name}, {ex.chip('rv32', chip)['name']} ({col}, {row}) + {add}"
            j.poke(*poke)
            groups = only_these_cells_differ(before, j.download(), [poke])
            summary, findings = j.check()
            want, tuples = is_the_oracles_verdict(j, groups, [poke], summary, findings, where)
            stale(where, ("V" if want else "") + ("U" if tuples else ""), pat)
            assert (want or tuples) and not summary["ok"], f"{where}: the oracle finds nothing to reject"
            try:
                proof = j.prove()
            except capi.DvtError as e:
                print(f"{where}: prove_job raised {e.code}: {e}")
            else:
                ok, _, _, why = capi.verify(j.vk, proof, Q, POW)
                ok_gpu, _, _, why_gpu = j.p.verify(j.vk, proof, Q, POW)
                print(f"{where}: proof of {len(proof)} bytes rejected: {why}")
                assert not ok and not ok_gpu and why and why == why_gpu, (where, ok, ok_gpu, why, why_gpu)
            j.poke(0, chip, col, row, P - add)
            only_these_cells_differ(before, j.download(), [])
        clean(*j.check())
        proof = j.prove()
        assert proof == honest_proof(name)
        ok, ec, pv, why = capi.verify(j.vk, proof, Q, POW)
        assert ok and pv == j.host["pv"], why


# ------------------------------------------------------------------ 8: refusals
def test_the_hook_refuses_what_it_cannot_poke():
    from dvt_circuits_amd import capi

    with Job("commit3") as j:
        p, lib = j.p, j.p.lib
        assert lib.dvt_rv32_debug_poke_cell(None, j.job, 0, 3, 0, 0, 1) == capi.DVT_ERR_INPUT
        assert lib.dvt_rv32_debug_poke_cell(p.h, None, 0, 3, 0, 0, 1) == capi.DVT_ERR_INPUT
        assert p.job_shard_chips(j.job, 0) == 0b101111 and p.job_shard_chips(j.job, 2) == 0b111111
        w_cpu, h_cpu = p.job_shard_chip_shape(j.job, 0, CPU)
        w_byte, h_byte = p.job_shard_chip_shape(j.job, 0, BYTE)
        w_init, h_init = p.job_shard_chip_shape(j.job, 2, MEM_INIT)
        w_img, h_img = p.job_shard_chip_shape(j.job, 1, MEM_IMAGE)
        bad = [(3, 3, 0, 0, 1), (1 << 40, 3, 0, 0, 1),                       # a shard the job does not hold
               (0, 14, 0, 0, 1), (0, 0xffffffff, 0, 0, 1), (0, MULDIV, 0, 0, 1),   # no such chip; muldiv: not in this guest
               (0, MEM_INIT, 0, 0, 1), (1, MEM_INIT, 0, 0, 1),                # mem_init is in the last shard only
               (0, CPU, w_cpu, 0, 1), (0, CPU, 0, 1 << h_cpu, 1), (0, BYTE, w_byte, 0, 1), (0, BYTE, 0, 1 << h_byte, 1),
               (2, MEM_INIT, w_init, 0, 1), (2, MEM_INIT, 0, 1 << h_init, 1), (1, MEM_IMAGE, w_img, 0, 1), (1, MEM_IMAGE, 0, 1 << h_img, 1),
               (0, PROGRAM, 1, 0, 1), (0, PROGRAM, 0, 0xffffffff, 1), (0, BYTE, 0xffffffff, 0, 1),
               (0, MEM_IMAGE, 0, 0, 0), (0, MEM_IMAGE, 0, 0, P), (0, BYTE, 0, 0, 0xffffffff), (0, CPU, 0, 0, 0), (0, CPU, 0, 0, P)]
        for args in bad:
            with pytest.raises(capi.DvtError) as e:
                j.poke(*args)
            assert e.value.code == capi.DVT_ERR_INPUT, args
        clean(*j.check())
        assert j.prove() == honest_proof("commit3")
        # the proof consumed the kept K0 output: a cpu cell has nowhere to go
        with pytest.raises(capi.DvtError) as e:
            j.poke(*JOB3["cpu_s1"][:5])
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED
        clean(*j.check())
        assert j.tuples() == ([], False)
        assert j.prove() == honest_proof("commit3")
    with Job("commit3", first=0, stride=2) as j:
        with pytest.raises(capi.DvtError) as e:
            j.poke(*JOB3["image_s1"][:5])
        assert e.value.code == capi.DVT_ERR_INPUT
        clean(*j.check(), bus_checked=0)


# ------------------------------------------------------------------ the search
if __name__ == "__main__":
    if sys.argv[1:] != ["--search"]:
        sys.exit("usage: python -m tests.test_gpu_job_faults --search")
    found3 = search_job3()
    print("JOB3 = {")
    for k, v in found3.items():
        print(f"    {k!r}: {v!r},".replace("'", '"'))
    print("}")
    found = {name: search_guest(name) for name in GUESTS}
    print("GUEST_CELLS = {")
    for name, cells in found.items():
        print(f"    {name!r}: {cells!r},".replace("'", '"'))
    print("}")
    same = found3 == JOB3 and found == GUEST_CELLS
    print("these are the committed constants" if same else "the committed constants DIFFER")
    sys.exit(0 if same else 1)
