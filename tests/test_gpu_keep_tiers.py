"""The three tiers of what a committed shard keeps in HBM for phase 2 ("keep_phase1": 2, include/dvt_prover.h DVT_KEEP_*):
everything (FULL), the main Merkle tree alone (TREE), nothing (NONE).  A TREE shard runs K0 and the main LDEs again in
phase 2 and takes tree and root from phase 1; the launches are those of the other two paths on the same inputs, so headers,
shard proofs and containers are the bytes of the default mode on one lane, which every case compares against and which
must verify.  Jobs of this size never run out of HBM: "keep_full_max" (a diagnostic key) caps the shards kept in full, so
that the other tiers are reached."""
import functools

import pytest

from tests import guests
from tests.test_gpu_phase1_lanes import _lanes, _prover, _same_headers, _three_ways
from tests.test_gpu_phase2_lanes import _per_shard, _precompile_guest

pytestmark = pytest.mark.gpu

Q, POW = 8, 4
NONE, TREE, FULL = 0, 1, 2
N_CHIPS = 14
ALL_TREES = ', "keep_phase1": 2, "keep_full_max": 0'


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    yield


def _tiers(p, job):
    n = p.job_shards(job)
    return [p.job_shard_kept(job, i) for i in range(n)], [p.job_shard_kept_bytes(job, i) for i in range(n)]


def _shapes(p, job):
    """per shard: [(main_w, log_n)] of its chips"""
    out = []
    for i in range(p.job_shards(job)):
        mask = p.job_shard_chips(job, i)
        out.append([p.job_shard_chip_shape(job, i, c) for c in range(N_CHIPS) if mask >> c & 1])
    return out


@functools.lru_cache(maxsize=None)
def _run(extra, guest="bignum"):
    """the job under a config: headers, the container three ways, the vk, and tiers / kept bytes / chip shapes after prepare"""
    if guest == "bignum":
        elf, stdin, log_shard = guests.bignum(1, limbs=12)[0], (), 10
    else:
        elf, stdin, _ = _precompile_guest()
        log_shard = 12
    p = _prover(log_shard, extra)
    try:
        headers, loop, whole, core, vk = _three_ways(p, elf, stdin)
        pk, _ = p.setup(elf)
        job, _ = p.prepare(pk, stdin)
        tiers, kept = _tiers(p, job)
        shapes = _shapes(p, job)
        members = [p.job_shard_member(job, i) for i in range(len(tiers))]
        p.job_free(job)
        p.pk_free(pk)
    finally:
        p.close()
    return dict(headers=headers, loop=loop, whole=whole, core=core, vk=vk, tiers=tiers, kept=kept, shapes=shapes, members=members)


@pytest.fixture(scope="module")
def reference(gpu):
    """the 13-shard job on one lane in the default mode; its container verifies and gives the expected public values"""
    from dvt_circuits_amd import capi

    ref = _run(', "lanes": 1')
    assert len(ref["headers"]) == 13 and ref["loop"] == ref["whole"] == ref["core"]
    ok, ec, pv, why = capi.verify(ref["vk"], ref["loop"], Q, POW)
    assert ok and ec == 0 and pv == guests.bignum(1, limbs=12)[1], why
    return ref


def _same_bytes(got, ref):
    assert got["vk"] == ref["vk"]
    assert _same_headers(got["headers"], ref["headers"]), "headers differ from the reference's"
    for way in ("loop", "whole", "core"):
        assert got[way] == ref["loop"], "%s: bytes differ from the reference proof" % way


def _tree_bytes(shape):
    hmax = 1 + max(log_n for _, log_n in shape)
    return ((2 << hmax) - 1) * 32


@pytest.mark.parametrize("lanes", [', "lanes": 1', _lanes(3, 2)])
def test_all_trees(reference, lanes):
    got = _run(lanes + ALL_TREES)
    assert got["tiers"] == [TREE] * 13
    _same_bytes(got, reference)


def test_mixed_tiers_one_lane(reference):
    got = _run(', "lanes": 1, "keep_phase1": 2, "keep_full_max": 3')
    assert got["tiers"] == [FULL] * 3 + [TREE] * 10
    _same_bytes(got, reference)


def test_mixed_tiers_three_lanes(reference):
    got = _run(_lanes(3, 2) + ', "keep_phase1": 2, "keep_full_max": 3')
    assert sorted(got["tiers"]) == [TREE] * 10 + [FULL] * 3
    _same_bytes(got, reference)


def test_old_modes_through_the_getter(reference):
    assert reference["tiers"] == [FULL] * 13
    one = _run(', "lanes": 1, "keep_phase1": 1')
    assert one["tiers"] == [FULL] * 13 and one["kept"] == reference["kept"]
    zero = _run(', "lanes": 1, "keep_phase1": 0')
    assert zero["tiers"] == [NONE] * 13 and zero["kept"] == [0] * 13
    _same_bytes(zero, reference)
    two = _run(', "lanes": 1, "keep_phase1": 2')
    assert two["tiers"] == [FULL] * 13 and two["kept"] == reference["kept"]
    _same_bytes(two, reference)


def test_bytes_kept(reference):
    trees = _run(', "lanes": 1' + ALL_TREES)
    assert trees["shapes"] == reference["shapes"]
    for shape, tree_b, full_b in zip(reference["shapes"], trees["kept"], reference["kept"]):
        assert tree_b == _tree_bytes(shape)
        assert full_b >= tree_b + sum((8 * w) << log_n for w, log_n in shape)
    mixed = _run(', "lanes": 1, "keep_phase1": 2, "keep_full_max": 3')
    assert mixed["kept"] == reference["kept"][:3] + trees["kept"][3:]


def test_mixed_height_tree(gpu):
    """the precompile guest: several chips of different heights in one tree, and with compact openings the node gather
    reads the kept tree"""
    from dvt_circuits_amd import capi

    ref = _run(', "lanes": 1, "keep_phase1": 1', "precompile")
    assert ref["loop"] == ref["whole"] == ref["core"]
    ok, ec, pv, why = capi.verify(ref["vk"], ref["loop"], Q, POW)
    assert ok and ec == 0 and pv == _precompile_guest()[2], why
    assert any(len({log_n for _, log_n in shape}) > 1 for shape in ref["shapes"])
    got = _run(', "lanes": 1' + ALL_TREES, "precompile")
    assert got["tiers"] == [TREE] * len(ref["tiers"]) and got["kept"] == [_tree_bytes(s) for s in ref["shapes"]]
    _same_bytes(got, ref)
    compact_ref = _run(', "lanes": 1, "keep_phase1": 1, "compact_openings": 1', "precompile")
    assert compact_ref["loop"] != ref["loop"] and compact_ref["loop"] == capi.proof_compact(ref["vk"], ref["loop"], Q, POW)
    compact = _run(', "lanes": 1, "compact_openings": 1' + ALL_TREES, "precompile")
    assert compact["tiers"] == got["tiers"]
    _same_bytes(compact, compact_ref)


def test_recommit(reference):
    """phase 1 of a TREE shard again (its tree buffer is reused): the same header; a second prove_job: the same bytes"""
    elf = guests.bignum(1, limbs=12)[0]
    p = _prover(10, ', "lanes": 1' + ALL_TREES)
    try:
        pk, vk = p.setup(elf)
        job, headers, ch, proofs = _per_shard(p, pk, vk, ())   # (every header is consumed by its prove_shard)
        assert p.assemble(job, proofs) == reference["loop"]
        again = [p.commit_shard(pk, job, i) for i in range(13)]
        assert _same_headers(again, [headers[i] for i in range(13)]) and _same_headers(again, reference["headers"])
        assert _tiers(p, job)[0] == [TREE] * 13
        for _ in range(2):
            assert p.prove_job(pk, job) == reference["loop"]
            assert _tiers(p, job)[0] == [TREE] * 13
        p.job_free(job)
        p.pk_free(pk)
    finally:
        p.close()
    p = _prover(10, ', "lanes": 1, "keep_phase1": 2, "keep_full_max": 3')   # (mixed tiers stay too)
    try:
        pk, _ = p.setup(elf)
        job, _ = p.prepare(pk, ())
        want = _tiers(p, job)
        for _ in range(2):
            assert p.prove_job(pk, job) == reference["loop"]
            assert _tiers(p, job) == want
        p.job_free(job)
        p.pk_free(pk)
    finally:
        p.close()


def test_two_members_on_one_device_share_the_cap(reference):
    got = _run(', "lanes": 1, "devices": [0, 0], "keep_phase1": 2, "keep_full_max": 2')
    assert set(got["members"]) == {0, 1}
    assert sorted(got["tiers"]) == [TREE] * 11 + [FULL] * 2
    _same_bytes(got, reference)


def test_inspectors_on_a_tree_job(reference):
    elf = guests.bignum(1, limbs=12)[0]
    p = _prover(10, ', "lanes": 1' + ALL_TREES)
    try:
        pk, _ = p.setup(elf)
        job, _ = p.prepare(pk, ())
        for _ in range(2):
            summary, findings = p.check_job(pk, job)
            assert summary["ok"] and summary["violations"] == 0 and findings == [] and summary["unbalanced_buses"] == 0, summary
            assert _tiers(p, job)[0] == [TREE] * 13
            assert p.prove_job(pk, job) == reference["loop"]
        p.job_free(job)
        p.pk_free(pk)
    finally:
        p.close()


def test_one_shard(gpu):
    from dvt_circuits_amd import capi

    elf, want = guests.arith(commit=True)
    out = []
    for extra in ("", ALL_TREES):
        p = _prover(16, extra)
        try:
            pk, vk = p.setup(elf)
            job, _ = p.prepare(pk, ())
            assert p.job_shards(job) == 1 and p.job_shard_kept(job, 0) == (TREE if extra else FULL)
            assert p.job_shard_kept(job, 1) == -1 and p.job_shard_kept_bytes(job, 1) == 0
            p.job_free(job)
            out.append((p.prove_core(pk, ())[0], vk))
            p.pk_free(pk)
        finally:
            p.close()
    assert out[0] == out[1]
    ok, ec, pv, why = capi.verify(out[0][1], out[0][0], Q, POW)
    assert ok and ec == 0 and pv == guests.checksum(want), why


def test_profile_counters_count_what_ran(gpu):
    """a one-shard proof on a profiling handle: a TREE shard runs the main LDEs twice (phase 1, then phase 2 again) and hashes
    as much as a FULL shard, which runs each launch once; the proofs are the same bytes"""
    elf, _ = guests.arith(commit=True)
    stats, proofs = {}, {}
    for name, extra in (("full", ""), ("tree", ALL_TREES)):
        p = _prover(16, ', "profile": 1' + extra)
        try:
            pk, _ = p.setup(elf)
            job, _ = p.prepare(pk, ())
            shape = _shapes(p, job)[0]
            p.job_free(job)
            proofs[name] = p.prove_core(pk, ())[0]
            stats[name] = p.kernel_stats()
            p.pk_free(pk)
        finally:
            p.close()
    assert proofs["tree"] == proofs["full"]
    assert stats["tree"]["merkle_perms"] == stats["full"]["merkle_perms"] > 0
    assert stats["tree"]["lde_calls"] == stats["full"]["lde_calls"] + len(shape)
    assert stats["tree"]["lde_alg_bytes"] == stats["full"]["lde_alg_bytes"] + sum((12 * w) << log_n for w, log_n in shape)
    for key in ("cells_main", "cells_perm", "cells_quotient", "cells_prep"):
        assert stats["tree"][key] == stats["full"][key]
