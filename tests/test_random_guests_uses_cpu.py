"""CPU tests of the uses slice on seeded random guests (tests/guests_random.py), no GPU: the host path (capi.execute_uses) on the
twelve pinned cases at 2^9 cycles per shard, from the three positions of tests/test_random_guests_slices_cpu.origin_places that
lie inside the random part, on the pool registers (ra in the flow cases) and the most stored scratch words, against the rule
written over the model's rows (tests/_uses_ref.uses_of) and the three yardsticks that do not depend on it (inverse_of_origin,
counts_agree, values_agree).  Every comparison is of exact integers.

uses_places() and check_uses() are shared with tests/test_gpu_random_guests_uses.py, which runs the same positions and targets
through the prepared jobs."""
import pytest

from dvt_circuits_amd import capi
from tests import _uses_ref as uref
from tests import guests_random as gr
from tests.test_random_guests_cpu import CASE_IDS, guest_of, run_of
from tests.test_random_guests_slices_cpu import origin_places, where_of

LOG = 9
INSIDE = ("middle", "shard row 0", "shard row 511")


def uses_places(case, subset=False):
    """the places of origin_places() that lie inside the random part, with their targets"""
    return [p for p in origin_places(case, LOG, subset) if p[0] in INSIDE]


def check_uses(call, case, subset=False, device=False):
    """every place, target and follow_addr of a case through call(at, target, follow_addr) -> slice, against the rule and the
    three yardsticks; returns (slices, edges checked, uses counted, values compared)"""
    run = run_of(case, LOG)
    slices = edges = uses = values = 0
    for name, at, g, targets in uses_places(case, subset):
        for target in targets:
            for follow in (False, True):
                where = where_of(case, LOG, name, at, target, follow)
                got = call(at, target, follow)
                want = uref.uses_of(run, at, target, follow)
                e, u, v = uref.check(got, run, want, follow, host=not device, where=where)
                assert got["summary"]["position"] == g, where
                if device:
                    assert got["summary"]["passes"] == sum(-(-q // 256) for q in want["level_defs"]), where
                edges, uses, values, slices = edges + e, uses + u, values + v, slices + 1
    return slices, edges, uses, values


def host_uses(case):
    elf = guest_of(case).elf

    def call(at, target, follow):
        rc, rep, got, err = capi.execute_uses(elf, [], at, target, log_shard=LOG, follow_addr=follow)
        assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, (case, at, target, err)
        return got
    return call


@pytest.mark.parametrize("case", gr.CASES, ids=CASE_IDS)
def test_host_uses_are_the_models(case):
    slices, edges, uses, values = check_uses(host_uses(case), case)
    print(gr.case_id(case), "slices", slices, "edges checked", edges, "uses counted", uses, "values compared", values)
    assert slices >= 2 * 3 * (10 if case[1] == "alu" else 18) and edges > 1000 and uses >= edges and values > 500


def test_the_places_lie_inside_the_random_part():
    assert len(gr.CASES) == 12
    for case in gr.CASES:
        first, end = gr.random_span(guest_of(case), run_of(case, LOG))
        places = uses_places(case)
        assert [p[0] for p in places] == list(INSIDE) and all(first <= g < end for _, _, g, _ in places), (case, first, end)
