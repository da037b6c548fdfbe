"""GPU tests of the divergence report of two prepared jobs (diverge_classify_kernel, diverge_merge_kernel, diverge_emit_kernel and
origin_gather_kernel through dvt_rv32_job_diverge / Prover.job_diverge, and `dvt_prover_host diverge`).

Every case holds the device's answer against the rule written over the rows of two runs of the independent model
(tests/_diverge_ref.report) and against the host path (capi.execute_diverge at the same shard size), dict for dict.  Every
comparison is of exact integers, and every property of a shape is asserted on the reference's answer inside the test.
Shapes: finalization_like(6, 40 words) is 24436 cycles: at 2^10 cycles per shard 24 shards, each smaller than a span of 4096
pairs; at 2^12 a span is a shard, with a ragged last of 3956; at 2^14 four spans in the one full shard and a ragged shard of
8052 rows.  One prepared pair per shard size is shared by the tests that need it."""
import contextlib
import os
import subprocess

import pytest

from tests import _diverge_ref as ref
from tests import guests, guests_diverge
from tests.test_diverge_host import BRANCHY, DEPTHS, FLIPPED, INPUT, SHORTER, cli_agrees, fin_elf, small_elf, stream
from tests.test_memory_host import CLI

pytestmark = pytest.mark.gpu
Q, POW = 6, 5


def _prover(log_shard, extra=""):
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra))


@contextlib.contextmanager
def _jobs_of(elf, inputs, log_shard, extra=""):
    """diverge(x, y, **kw) over the prepared jobs of the guest on inputs[x] and inputs[y]; .p, .pk, .jobs"""
    p = _prover(log_shard, extra)
    pk, _ = p.setup(elf)
    jobs = [p.prepare(pk, [buf])[0] for buf in inputs]
    diverge = lambda x, y, **kw: p.job_diverge(pk, jobs[x], jobs[y], **kw)
    diverge.p, diverge.pk, diverge.jobs = p, pk, jobs
    try:
        yield diverge
    finally:
        for job in jobs:
            p.job_free(job)
        p.pk_free(pk)
        p.close()


FIN = (INPUT, FLIPPED, SHORTER)


@pytest.fixture(scope="module", params=[10, 12, 14])
def fin(request):
    with _jobs_of(fin_elf(), FIN, request.param) as diverge:
        diverge.log_shard = request.param
        yield diverge


@pytest.fixture(scope="module")
def fin10():
    with _jobs_of(fin_elf(), FIN, 10) as diverge:
        yield diverge


@pytest.fixture(scope="module")
def fin14():
    with _jobs_of(fin_elf(), FIN, 14) as diverge:
        yield diverge


def check(diverge, elf, inputs, x, y, log_shard, where, **kw):
    """one device answer against the rule and the host path; returns the rule's answer"""
    from dvt_circuits_amd import capi

    got = diverge(x, y, **kw)
    want = ref.report(stream(elf, inputs[x], log_shard), stream(elf, inputs[y], log_shard), **kw)
    ref.same(got, want, where)
    rc, reps, host, err = capi.execute_diverge(elf, inputs[x], inputs[y], log_shard=log_shard, **kw)
    assert rc == 0 and ref.without(host) == ref.without(got), (where, err)
    assert got["summary"]["launched_pairs"] >= want["summary"]["n_pairs"] + (want["summary"]["reason"] in (ref.SPLIT, ref.BAD)), where
    return want


def test_the_shapes_of_the_shard_sizes():
    sizes = {log: stream(fin_elf(), INPUT, log).sizes for log in (10, 12, 14)}
    assert sizes[10] == [1024] * 23 + [884] and sizes[12] == [4096] * 5 + [3956] and sizes[14] == [16384, 8052]


def test_one_flipped_bit_and_one_word_less(fin):
    log = fin.log_shard
    want = check(fin, fin_elf(), FIN, 0, 1, log, "one bit, 2^%d" % log, keep=16)
    s = want["summary"]
    assert s["reason"] == ref.END_BOTH and s["n_pairs"] == 24436 and s["n_data"] > 128 and want["first"][0]["dir"] == 1 and want["first"][0]["mask"] & ref.MEM
    assert len({e["shard_a"] for e in want["last"]} | {e["shard_a"] for e in want["first"]}) == 2
    want = check(fin, fin_elf(), FIN, 0, 2, log, "one word less, 2^%d" % log, rejoin=True)
    s = want["summary"]
    assert s["reason"] == ref.SPLIT and (s["rejoin_skip_a"], s["rejoin_skip_b"]) == (13, 0) and s["n_data"] == 44
    again = check(fin, fin_elf(), FIN, 0, 2, log, "from the rejoin, 2^%d" % log, rejoin=True, start_a=(s["rejoin_shard_a"], s["rejoin_row_a"]),
                  start_b=(s["rejoin_shard_b"], s["rejoin_row_b"]))
    assert again["summary"]["reason"] == ref.END_BOTH and again["summary"]["n_pairs"] == 24436 - s["n_pairs"] - 13
    # a job against itself, and against the job of the same input
    want = check(fin, fin_elf(), FIN, 0, 0, log, "itself, 2^%d" % log)
    assert want["summary"]["n_data"] == 0 and want["summary"]["reason"] == ref.END_BOTH and not any(r["n_diff"] for r in want["regs"])


@pytest.mark.parametrize("start", [(2, 4095), (2, 4096), (3, 0), (1, 4095), (1, 4096), (1, 16383), (2, 0), (2, 8051)])
def test_equal_starts_at_span_and_shard_edges(fin14, start):
    """span edges inside both shards, the shard edge, the last record, and (3, 0): past the end of an execution of two shards,
    which is its end (no pair is left)"""
    want = check(fin14, fin_elf(), FIN, 0, 1, 14, "both from %s" % (start,), start_a=start, start_b=start, keep=4)
    sa = stream(fin_elf(), INPUT, 14)
    assert want["summary"]["n_pairs"] == 24436 - sa.global_of(start) and want["summary"]["reason"] == ref.END_BOTH
    if start == (3, 0):
        assert want["summary"]["n_pairs"] == 0 and want["first"] == []
    elif start == (2, 8051):      # the last record alone: the HALT, the same in both runs
        assert want["summary"]["n_pairs"] == 1 and want["summary"]["n_data"] == 0
    else:
        assert want["summary"]["n_data"] > 0 and want["first"][0]["k"] == want["summary"]["first_data"]


def test_unequal_starts_straddle_shard_edges(fin10):
    """from the rejoin of `one word less` at 2^10 the two sides are 13 records apart: every segment ends at a shard edge of one
    side only, and there are about twice as many segments as shards"""
    first = ref.report(stream(fin_elf(), INPUT), stream(fin_elf(), SHORTER), rejoin=True)["summary"]
    a, b = (first["rejoin_shard_a"], first["rejoin_row_a"]), (first["rejoin_shard_b"], first["rejoin_row_b"])
    assert a[1] - b[1] == 13 and a[0] == b[0] == 1
    want = check(fin10, fin_elf(), FIN, 0, 2, 10, "unequal starts", start_a=a, start_b=b, keep=64)
    s = want["summary"]
    assert s["reason"] == ref.END_BOTH and s["n_pairs"] > 23 * 1024 and s["n_data"] > 128
    every = ref.report(stream(fin_elf(), INPUT), stream(fin_elf(), SHORTER), start_a=a, start_b=b, keep=1 << 30)["first"]      # all data pairs
    assert any(e["shard_a"] != e["shard_b"] for e in every) and any(e["shard_a"] == e["shard_b"] for e in every)
    assert all((e["shard_a"] - 1) * 1024 + e["row_a"] - ((e["shard_b"] - 1) * 1024 + e["row_b"]) == 13 for e in every)
    # and far apart: A from its third shard against B from its entry
    want = check(fin10, fin_elf(), FIN, 0, 1, 10, "two shards apart", start_a=(3, 100), start_b=(1, 0), rejoin=True)
    assert want["summary"]["reason"] == ref.SPLIT


@pytest.mark.parametrize("name,inputs", [("branchy", BRANCHY), ("depths", DEPTHS)])
def test_the_chain_of_segments(name, inputs):
    from dvt_circuits_amd import capi

    elf = small_elf(name)
    sa, sb = stream(elf, inputs[0]), stream(elf, inputs[1])
    want = ref.chain(sa, sb, 8)
    with _jobs_of(elf, inputs, 10) as diverge:
        got = ref.chain(sa, sb, 8, call=lambda **kw: diverge(0, 1, **kw))
    host = ref.chain(sa, sb, 8, call=lambda **kw: capi.execute_diverge(elf, inputs[0], inputs[1], log_shard=10, **kw)[2])
    assert len(got) == len(want) == len(host) >= 3
    for k, (g, w, h) in enumerate(zip(got, want, host)):
        ref.same(g, w, "%s segment %d" % (name, k))
        assert ref.without(g) == ref.without(h), k


@pytest.mark.parametrize("max_pairs", [1, 4096, 4097])
def test_the_pair_limit(fin14, max_pairs):
    want = check(fin14, fin_elf(), FIN, 0, 1, 14, "max_pairs %d" % max_pairs, max_pairs=max_pairs)
    assert want["summary"]["reason"] == ref.LIMIT and want["summary"]["n_pairs"] == max_pairs
    assert fin14(0, 1, max_pairs=max_pairs)["summary"]["launched_pairs"] == max_pairs


@pytest.mark.parametrize("keep", [0, 1, 4, 64])
def test_the_keep_sizes(fin14, keep):
    many = check(fin14, fin_elf(), FIN, 0, 1, 14, "keep %d, many" % keep, keep=keep)
    few = check(fin14, fin_elf(), FIN, 0, 2, 14, "keep %d, few" % keep, keep=keep)
    assert many["summary"]["n_data"] > 128 and few["summary"]["n_data"] == 44
    assert len(many["first"]) == keep and len(few["last"]) == min(keep, 44)


def test_an_early_split_launches_one_batch():
    """a job longer than two batches whose runs split in the first: no later batch is launched"""
    from dvt_circuits_amd import capi

    batch = capi.execute_diverge(fin_elf(), INPUT, INPUT)[2]["summary"]["batch_pairs"]      # the header constant as the library was built
    iters = 2 * batch // 2400 + 40
    elf = guests.finalization_like(iters, INPUT)[0]
    with _jobs_of(elf, (INPUT, SHORTER), 18) as diverge:
        got = diverge(0, 1, rejoin=True)
        s = got["summary"]
        print({k: s[k] for k in ("n_pairs", "launched_pairs", "cycles_a", "cycles_b")}, diverge.p.job_diverge_times())
        assert s["cycles_a"] > 2 * batch and s["cycles_b"] > 2 * batch
        assert s["reason"] == ref.SPLIT and s["n_pairs"] == 533 and (s["rejoin_skip_a"], s["rejoin_skip_b"]) == (13, 0)
        assert 0 < s["launched_pairs"] <= batch
        rc, reps, host, err = capi.execute_diverge(elf, INPUT, SHORTER, log_shard=18, rejoin=True)
        assert rc == 0 and ref.without(host) == ref.without(got), err
        # from the rejoin there is no split: every batch is launched, over segments that straddle the shard edges, and the answer
        # is the host path's
        at = dict(start_a=(s["rejoin_shard_a"], s["rejoin_row_a"]), start_b=(s["rejoin_shard_b"], s["rejoin_row_b"]))
        got = diverge(0, 1, keep=64, **at)
        print(diverge.p.job_diverge_times())
        assert got["summary"]["reason"] == ref.END_BOTH and got["summary"]["launched_pairs"] == got["summary"]["n_pairs"] == s["cycles_b"] - 533 > 2 * batch
        rc, reps, host, err = capi.execute_diverge(elf, INPUT, SHORTER, log_shard=18, keep=64, **at)
        assert rc == 0 and ref.without(host) == ref.without(got), err


def test_two_members(fin14):
    from dvt_circuits_amd import capi

    calls = [dict(keep=16), dict(start_a=(2, 0), start_b=(2, 0), keep=64), dict(max_pairs=20000, keep=4)]
    one = [fin14(0, 1, **kw) for kw in calls]
    split = fin14(0, 2, rejoin=True)
    with _jobs_of(fin_elf(), FIN, 14, ', "devices": [0, 0]') as diverge:
        assert [diverge.p.job_shards(j) for j in diverge.jobs] == [2, 2, 2]
        for kw, a in zip(calls, one):
            assert ref.without(diverge(0, 1, **kw)) == ref.without(a), kw
        assert ref.without(diverge(0, 2, rejoin=True)) == ref.without(split)
        # starts one shard apart: shard 1 of A is on member 0, shard 2 of B on member 1
        with pytest.raises(capi.DvtError) as e:
            diverge(0, 1, start_a=(1, 0), start_b=(2, 0))
        assert e.value.code == capi.DVT_ERR_UNSUPPORTED and "segment 0" in str(e.value)


def test_refusals(fin14):
    from dvt_circuits_amd import capi

    for kw in (dict(keep=65), dict(window=16385)):
        with pytest.raises(capi.DvtError) as e:
            fin14(0, 1, **kw)
        assert e.value.code == capi.DVT_ERR_INPUT, kw
    p, pk = fin14.p, fin14.pk
    part, _ = p.prepare(pk, [INPUT], first=0, stride=2)
    with pytest.raises(capi.DvtError) as e:
        p.job_diverge(pk, fin14.jobs[0], part)
    assert e.value.code == capi.DVT_ERR_UNSUPPORTED
    p.job_free(part)
    # the end of an execution is a start, however it is spelled: no pair
    for end in ((2, 8052), (2, 9000), (7, 1)):
        got = fin14(0, 1, start_a=end)
        assert got["summary"]["n_pairs"] == 0 and got["summary"]["reason"] == ref.END_A and got["summary"]["launched_pairs"] == 0
        assert (got["summary"]["stop_shard_a"], got["summary"]["stop_row_a"]) == (2, 8052)


def test_the_jobs_are_left_as_found_and_the_times(fin14):
    p, pk, jobs = fin14.p, fin14.pk, fin14.jobs
    before = fin14(0, 1, keep=8)
    proof = p.prove_job(pk, jobs[0])
    after = fin14(0, 1, keep=8)
    assert ref.without(before) == ref.without(after) and p.prove_job(pk, jobs[0]) == proof
    t = p.job_diverge_times()
    print(t, after["summary"]["ms"])
    assert sorted(t) == ["classify_ms", "emit_ms", "host_ms", "merge_ms"] and all(0 <= v < 5000 for v in t.values()) and t["classify_ms"] > 0
    assert abs(sum(t.values()) - after["summary"]["ms"]) < 0.01 * after["summary"]["ms"] + 0.01


def test_cli_diverge_on_the_gpu_is_the_host_output(tmp_path):
    elf = fin_elf()
    path = tmp_path / "guest.elf"
    path.write_bytes(elf)
    example = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finalization_example.json")
    other = tmp_path / "other.json"
    text = open(example).read()
    changed = text.replace('"gen_id": "8d17', '"gen_id": "9d17', 1)
    assert changed != text
    other.write_text(changed)
    base = [CLI, "diverge", "--type", "finalization", "-i", example, "--against", str(other), "--elf", str(path), "--log-shard", "12", "--rejoin", "2", "--keep", "3"]
    dev = subprocess.run(base, capture_output=True, text=True, timeout=300)
    host = subprocess.run(base + ["--host"], capture_output=True, text=True, timeout=300)
    print(dev.stdout[:3000], dev.stderr)
    assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
    assert dev.stdout == host.stdout and dev.stdout.startswith("diverge: pairs=")
    from dvt_circuits_amd import capi

    bufs = [capi.stdin_from_json("finalization", open(f, "rb").read()) for f in (example, str(other))]
    assert bufs[0] != bufs[1]
    sa, sb = [ref.stream_of(ref.model_run(elf, (b,), 12)) for b in bufs]
    want = ref.chain(sa, sb, 2, keep=3)
    cli_agrees(dev.stdout, want)
    assert want[0]["summary"]["n_data"] > 0
