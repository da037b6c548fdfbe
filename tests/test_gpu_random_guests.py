"""GPU tests on seeded random guests (tests/guests_random.py): what the device builds and reports on the pinned cases, at 2^21 and
2^9 cycles per shard, against the oracle's independent model (oracle/rv32_model.py) and the report rules written over it.

fill_cpu_row of csrc/rv32.h is one template compiled for the host and for the device; the host rows agreeing with the model
(tests/test_random_guests_cpu.py) says nothing about the device instantiation.  Here every word K0 writes on the device (the
cpu rows, the shift, muldiv and mem_init rows, the byte-table and program-table multiplicities) is compared with the model's;
the job check, the bus ledger and the five record reports run on the same jobs, the origin slice and the divergence report on
the positions, targets and pairs of inputs of tests/test_random_guests_slices_cpu.py; one case of each profile is proven and
verified, and the proof bytes of a short case equal the oracle prover's.  At 2^21 a job is one shard of two or three K0
workgroups with a ragged last one, at 2^9 thirteen or more shards of one partial workgroup each.

Every comparison is exact; a difference is reported with the seed, the chip, the column's name, the row and the instruction."""
import contextlib
import struct

import numpy as np
import pytest

from oracle import rv32_model
from tests import _calltree_ref, _diverge_ref, _memory_ref, _oracle_prover, _profile_ref, _snapshot_ref, _watch_ref
from tests import guests_random as gr
from tests.test_random_guests_cpu import FLOW, flow_positions, flow_queries, guest_of, run_of
from tests.test_random_guests_slices_cpu import INPUT_IDS, chains_agree, check_origin, host_diverge, host_origin, input_guest, streams_of

pytestmark = pytest.mark.gpu
Q, POW = 8, 4
LOGS = (21, 9)
CASE_IDS = [gr.case_id(c) for c in gr.CASES]


@pytest.fixture(scope="module")
def provers():
    """one handle per shard size for the whole module"""
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    made = {log: capi.Prover('{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d}' % (Q, POW, log)) for log in LOGS}
    yield made
    for p in made.values():
        p.close()


@contextlib.contextmanager
def job_of(p, case, log_shard, stdin=()):
    """(pk, vk, job) of a case prepared on a handle; the shard count and the cycles are the model's.  stdin: the input buffers
    of the case's guest with the input prologue (none: the guest without it)"""
    guest = input_guest(case) if stdin else guest_of(case)
    run = _profile_ref.model_run(guest.elf, stdin, log_shard)
    pk, vk = p.setup(guest.elf)
    job = None
    try:
        job, rep = p.prepare(pk, list(stdin))
        assert p.job_shards(job) == len(run.shards) and rep["cycles"] == run.cycles and rep["halted"] and rep["exit_code"] == 0, (case, log_shard, rep)
        yield pk, vk, job
    finally:
        if job is not None:
            p.job_free(job)
        p.pk_free(pk)


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_k0_device_traces_equal_the_model(provers, case, log_shard):
    p = provers[log_shard]
    run = run_of(case, log_shard)
    with job_of(p, case, log_shard) as (pk, vk, job):
        for shard in range(len(run.shards)):
            dev, dpubs = p.debug_device_traces(pk, job, shard)
            model, mpubs = rv32_model.traces(run, shard)
            where = "seed %d profile %s n %d at 2^%d, shard %d" % (case[0], case[1], case[2], log_shard, shard)
            assert [int(x) for x in dpubs] == [int(x) for x in mpubs], (where, "public values")
            assert [(c["chip_id"], c["log_n"]) for c in dev] == [(c["chip_id"], c["log_n"]) for c in model], (where, "chip set and heights")
            for d, m in zip(dev, model):
                why = gr.first_difference(case, log_shard, run, shard, d, m, "main", who="the device")
                assert why is None, why


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_job_check_and_ledger_are_clean(provers, case, log_shard):
    p = provers[log_shard]
    where = "%s at 2^%d" % (gr.case_id(case), log_shard)
    with job_of(p, case, log_shard) as (pk, vk, job):
        summary, findings = p.check_job(pk, job)
        assert summary["ok"] and summary["violations"] == 0 and summary["n_findings"] == 0 and findings == [], (where, summary, findings[:4])
        assert summary["bus_checked"] == 1 and summary["unbalanced_buses"] == 0, (where, summary)
        assert p.job_bus_tuples(pk, job) == ([], False), where


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_job_reports_are_the_models(provers, case, log_shard):
    p = provers[log_shard]
    guest, run = guest_of(case), run_of(case, log_shard)
    where = "%s at 2^%d" % (gr.case_id(case), log_shard)
    entry = struct.unpack_from("<I", guest.elf, 24)[0]
    with job_of(p, case, log_shard) as (pk, vk, job):
        prof = p.job_profile(pk, job)
        _profile_ref.same_tables(prof, _profile_ref.tally(run), where)
        _profile_ref.flow_law(prof, entry, run.shards[-1]["rows"][-1].ins.pc)
        assert prof["summary"]["shards_tallied"] == prof["summary"]["shards_total"] == len(run.shards), where
        mem = p.job_memory(pk, job)
        _memory_ref.same_report(mem, _memory_ref.report(run), where)
        tree = p.job_calltree(pk, job)
        _calltree_ref.same_tree(tree, _calltree_ref.tree(run), where)
        _calltree_ref.sum_laws(tree, entry)
        assert tree["summary"]["shards_total"] == len(run.shards), where
        if case in FLOW:
            queries = flow_queries(guest, run)
            want = _watch_ref.search(run, queries)
            assert all(w["total"] for w in want), where
            _watch_ref.same(p.job_watch(pk, job, queries, keep=16), want, 16, where)
            ranges = [(guest.scratch, guest.scratch + 4 * (gr.SCRATCH_WORDS + len(gr.POOL)))]
            for at in flow_positions(guest, run):
                snap = p.job_snapshot(pk, job, at, ranges, 64)
                want = _snapshot_ref.take(run, at, ranges, 64)
                _snapshot_ref.same(snap, want, "%s at %s" % (where, at))
                _snapshot_ref.agrees(snap, _snapshot_ref.state_at(guest.elf, (), log_shard, want["summary"]["position"]), run, where)


def _without_ms(got, passes=None):
    s = {k: v for k, v in got["summary"].items() if k != "ms"}
    return dict(got, summary=s if passes is None else dict(s, passes=passes))


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_job_origins_are_the_models(provers, case, log_shard):
    """origin_reduce_kernel and origin_gather_kernel on five of the pool registers, ra in the flow cases and four of the most
    stored scratch words (the subset is the seed's), from four positions of the random part and from the exit, follow_addr off
    and on: against the rule over the model's rows, passes = the sum of ceil(level questions / 256), both yardsticks, and the
    host path dict for dict"""
    p = provers[log_shard]
    host = host_origin(case, log_shard)
    with job_of(p, case, log_shard) as (pk, vk, job):
        def call(at, target, follow):
            got = p.job_origin(pk, job, at, target, follow_addr=follow)
            assert _without_ms(host(at, target, follow)) == _without_ms(got, passes=0), (gr.case_id(case), log_shard, at, target, follow)
            return got
        slices, edges, roots = check_origin(call, case, log_shard, subset=True, device=True)
    print(gr.case_id(case), "2^%d" % log_shard, "slices", slices, "edges checked", edges, "roots compared", roots)
    assert slices >= 2 * (4 * (5 if case[1] == "alu" else 9) + 5) and edges > 500 and roots == slices


@pytest.mark.parametrize("log_shard", LOGS)
@pytest.mark.parametrize("entry", gr.INPUT_CASES, ids=INPUT_IDS)
def test_job_divergence_is_the_models(provers, entry, log_shard):
    """diverge_classify_kernel, diverge_merge_kernel and diverge_emit_kernel on two jobs of one guest with the input prologue: the
    whole chain of segments against the rule over the model's two runs and against the host path, and one report with keep = 64"""
    p = provers[log_shard]
    a, b = gr.inputs_of(entry)
    sa, sb = streams_of(entry, log_shard)
    where = "%s at 2^%d" % (gr.input_case_id(entry), log_shard)
    host = host_diverge(entry, log_shard)
    with job_of(p, entry[0], log_shard, stdin=(a,)) as (pk, vk, job_a):
        job_b, rep = p.prepare(pk, [b])
        try:
            assert rep["cycles"] == len(sb) and rep["halted"] and rep["exit_code"] == 0 and p.job_shards(job_b) == len(sb.sizes), (where, rep)
            got = _diverge_ref.chain(sa, sb, 64, keep=16, call=lambda **kw: p.job_diverge(pk, job_a, job_b, **kw))
            wide = p.job_diverge(pk, job_a, job_b, keep=64)
        finally:
            p.job_free(job_b)
    want = _diverge_ref.chain(sa, sb, 64, keep=16)
    chains_agree(got, want, where)
    held = _diverge_ref.chain(sa, sb, 64, keep=16, call=host)
    assert len(held) == len(got), where
    for k, (g, w, h) in enumerate(zip(got, want, held)):
        assert _diverge_ref.without(g) == _diverge_ref.without(h), (where, k)
        s = w["summary"]
        assert g["summary"]["launched_pairs"] >= s["n_pairs"] + (s["reason"] in (_diverge_ref.SPLIT, _diverge_ref.BAD)), (where, k)
    _diverge_ref.same(wide, _diverge_ref.report(sa, sb, keep=64), where + ", keep 64 from the entry")
    assert _diverge_ref.without(wide) == _diverge_ref.without(host(keep=64)), where


def _prove_and_verify(p, case):
    """the proof container of a case at 2^9: both verifiers accept it and its public values are the model's"""
    from dvt_circuits_amd import capi

    run = run_of(case, 9)
    with job_of(p, case, 9) as (pk, vk, job):
        proof = p.prove_job(pk, job)
        for who, (ok, ec, pv, why) in (("capi.verify", capi.verify(vk, proof, Q, POW)), ("Prover.verify", p.verify(vk, proof, Q, POW))):
            assert ok and ec == 0 and pv == run.public_values, (gr.case_id(case), who, why)
    return proof


@pytest.mark.parametrize("case", gr.PROVE_CASES, ids=[gr.case_id(c) for c in gr.PROVE_CASES])
def test_prove_and_verify(provers, case):
    _prove_and_verify(provers[9], case)


def test_proof_bytes_equal_the_oracle_provers(provers):
    """the short case, shard by shard: the oracle side is the model's traces through the oracle CPU prover"""
    from dvt_circuits_amd import capi

    case = gr.SHORT
    run = run_of(case, 9)
    ec, pv, gpu_shards = capi.split_container(_prove_and_verify(provers[9], case))
    assert ec == 0 and pv == run.public_values and len(gpu_shards) == len(run.shards) > 1
    shards = [rv32_model.traces(run, i) for i in range(len(run.shards))]
    prep_root = _oracle_prover.prep_root_of(shards[0][0])
    headers = [_oracle_prover.main_root(chips) + [int(x) for x in pubs] for chips, pubs in shards]
    gc = _oracle_prover.global_challenges(prep_root, headers)
    for i, (chips, pubs) in enumerate(shards):
        cpu = _oracle_prover.prove_shard("rv32", chips, pubs, Q, POW, perm_challenges=gc)[0]
        wa, wb = np.frombuffer(gpu_shards[i], np.uint32), np.frombuffer(cpu, np.uint32)
        n = min(len(wa), len(wb))
        d = np.nonzero(wa[:n] != wb[:n])[0]
        assert gpu_shards[i] == cpu, "seed %d shard %d: first differing word %d, lengths %d and %d" % (case[0], i, int(d[0]) if len(d) else n, len(wa), len(wb))
