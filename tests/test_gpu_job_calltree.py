"""GPU tests of the call-tree report of a prepared job (calltree_span_kernel through dvt_rv32_job_calltree /
Prover.job_calltree, and `dvt_prover_host check --show-calls`).

The yardstick is the rule written over the independent model's rows (tests/_calltree_ref.py); the host path
(capi.execute_calltree) must say the same.  Shapes: at 2^10 cycles per shard every shard is smaller than a workgroup's span of
4096 records; at 2^14 a full shard is four spans and the last shard is ragged; the guests of tests/guests_calltree.py put
whole spans inside one frame, spans of unmatched calls or returns only, spans with more than 1300 events, a CALL and a RET on
a shard's last record; the case at 2^21 is two shards and more than 512 spans, more workgroups than the device has CUs."""
import functools
import os
import subprocess

import pytest

from tests import _calltree_ref as ref
from tests import guests, guests_calltree
from tests.test_calltree_host import CLI, ROOT, block_of, entry_of

pytestmark = pytest.mark.gpu
Q, POW = 6, 5
GUESTS = dict(guests_calltree.GUESTS, bignum=lambda: guests.bignum(40)[0])


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


def _job_calltree(elf, log_shard, extra="", log_arc_slots=0):
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    job, _ = p.prepare(pk, [])
    tree = p.job_calltree(pk, job, log_arc_slots)
    n = p.job_shards(job)
    p.job_free(job)
    p.pk_free(pk)
    p.close()
    return tree, n


@functools.lru_cache(maxsize=None)
def _elf(name):
    return GUESTS[name]()


@functools.lru_cache(maxsize=None)
def _want(name):
    """the model's tree (the shard size does not enter the rule: one run at the default size)"""
    return ref.tree(ref.model_run(_elf(name)))


@functools.lru_cache(maxsize=None)
def _host(name):
    from dvt_circuits_amd import capi

    rc, rep, tree, err = capi.execute_calltree(_elf(name))
    assert rc == 0, err
    return tree


def _same(a, b, shards=True):
    """two reports say the same (everything but the time, and the shard count when the shard sizes differ)"""
    sa, sb = dict(a["summary"], ms=0), dict(b["summary"], ms=0)
    if not shards:
        sa["shards_total"] = sb["shards_total"] = 0
    assert sa == sb, (sa, sb)
    assert a["arcs"] == b["arcs"] and a["funcs"] == b["funcs"]


@pytest.mark.parametrize("log_shard", [10, 14])
@pytest.mark.parametrize("name", sorted(guests_calltree.GUESTS))
def test_job_calltree_is_the_models_and_the_hosts(name, log_shard):
    elf = _elf(name)
    tree, n = _job_calltree(elf, log_shard)
    s = tree["summary"]
    print(name, log_shard, s)
    cycles = _want(name)["cycles"]
    assert n == s["shards_total"] == -(-cycles // (1 << log_shard))
    ref.same_tree(tree, _want(name), "%s at 2^%d" % (name, log_shard))
    ref.sum_laws(tree, entry_of(elf))
    _same(tree, _host(name), shards=False)


def test_bignum_in_seven_shards():
    tree, n = _job_calltree(_elf("bignum"), 14)
    assert n == 7 and tree["summary"]["cycles"] == 102464
    ref.same_tree(tree, _want("bignum"), "bignum")
    _same(tree, _host("bignum"), shards=False)


def test_shard_size_does_not_change_the_tables():
    elf = _elf("recurse")
    small, n_small = _job_calltree(elf, 10)
    mid, n_mid = _job_calltree(elf, 14)
    one, n_one = _job_calltree(elf, 21)
    assert n_small > n_mid > n_one == 1
    _same(small, mid, shards=False)
    _same(mid, one, shards=False)
    _same(one, _host("recurse"))


@pytest.mark.parametrize("extra", [', "devices": [0, 0]', ', "keep_phase1": 0'])
def test_members_and_keep_tiers_give_the_same_report(extra):
    for name in ("recurse", "dense"):
        one, n = _job_calltree(_elf(name), 10)
        other, n_other = _job_calltree(_elf(name), 10, extra)
        assert n == n_other > 8
        _same(one, other)
        ref.same_tree(other, _want(name), name + extra)


def test_the_job_is_left_as_found():
    """the proof of a job that was inspected before and after proving equals that of a job that never was"""
    from dvt_circuits_amd import capi

    elf = guests.commit_only(b"check me")
    proofs = []
    for inspect in (True, False):
        p = _prover(11)
        pk, vk = p.setup(elf)
        job, _ = p.prepare(pk, [])
        assert p.job_shards(job) == 3
        before = p.job_calltree(pk, job) if inspect else None
        proofs.append(p.prove_job(pk, job))
        if inspect:
            _same(before, p.job_calltree(pk, job))
            ref.same_tree(before, ref.tree(ref.model_run(elf)), "commit_only")
            assert p.prove_job(pk, job) == proofs[0]
            assert all(v >= 0 for v in p.job_calltree_times().values())
        p.job_free(job)
        p.pk_free(pk)
        p.close()
    assert proofs[0] == proofs[1]
    ok, ec, pv, why = capi.verify(vk, proofs[0], Q, POW)
    assert ok and pv == b"check me", why


def test_a_partial_job_is_unsupported():
    from dvt_circuits_amd import capi

    p = _prover(10)
    pk, _ = p.setup(_elf("tail"))
    for first, stride in ((0, 2), (1, 2)):
        job, _ = p.prepare(pk, [], first=first, stride=stride)
        with pytest.raises(capi.DvtError) as e:
            p.job_calltree(pk, job)
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED and "gap" in str(e.value), e.value
        p.job_free(job)
    with pytest.raises(capi.DvtError) as e:
        job, _ = p.prepare(pk, [])
        try:
            p.job_calltree(pk, job, 2)
        finally:
            p.job_free(job)
    assert e.value.code == capi.DVT_ERR_INPUT
    p.pk_free(pk)
    p.close()


def test_a_small_arc_table_drops_and_says_so():
    elf, want = _elf("fanout"), _want("fanout")
    small, _ = _job_calltree(elf, 10, log_arc_slots=3)
    s = small["summary"]
    print("8 slots:", s)
    assert s["dropped_frames"] > 0 and s["dropped_cycles"] > 0 and s["n_funcs"] == 0 and small["funcs"] == []
    assert s["n_frames"] == want["n_frames"] and s["cycles"] == want["cycles"] and s["max_depth"] == want["max_depth"]
    ref.sum_laws(small, entry_of(elf))
    assert 0 < len(small["arcs"]) < len(want["arcs"])
    assert all(want["arcs"][(a, b)] == (n, c) for a, b, n, c in small["arcs"])
    assert sum(c for _, _, _, c in small["arcs"]) + s["dropped_cycles"] == sum(c for _, c in want["arcs"].values())
    full, _ = _job_calltree(elf, 10)
    assert full["summary"]["dropped_frames"] == 0 and full["summary"]["n_arcs"] == len(want["arcs"]) > guests_calltree.FANOUT_STUBS
    ref.same_tree(full, want, "default table")


@pytest.mark.parametrize("name", ["nest", "dense"])
def test_two_full_size_shards_against_the_host(name):
    """more than 2^21 cycles by more than a span: two shards, more than 512 spans, positions past 2^21; nest with frames that
    cover hundreds of spans, dense with a million frames.  Against the host path (the Python model is too slow here)."""
    from dvt_circuits_amd import capi

    elf = guests_calltree.nest(rounds=24, leaf_iters=29200) if name == "nest" else guests_calltree.dense(16200)
    rc, rep, host, err = capi.execute_calltree(elf)
    assert rc == 0 and (1 << 21) + 4096 < rep["cycles"] < (1 << 21) + (1 << 17), (rep, err)
    tree, n = _job_calltree(elf, 21)
    print(tree["summary"])
    assert n == 2 and tree["summary"]["cycles"] == rep["cycles"]
    _same(tree, host, shards=False)
    ref.sum_laws(tree, entry_of(elf))


def test_cli_check_show_calls(tmp_path):
    elf = guests.commit_only(b"check me")
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(ROOT, "tests", "golden", "finalization_example.json")
    want = ref.tree(ref.model_run(elf))
    base = [CLI, "check", "--type", "finalization", "-i", example, "--elf", str(path)]
    r = subprocess.run(base + ["--show-calls"], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("clean: ")
    frames, depth, rows = block_of(r.stdout)
    assert frames == want["n_frames"] and depth == want["max_depth"]
    assert rows == [(inc, own, n, "f_%x" % pc) for pc, n, inc, own in want["funcs"]]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.startswith("clean: ") and len(plain.stdout.splitlines()) == 1
