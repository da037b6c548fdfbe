"""The call-tree report on the host (dvt_execute_calltree, no GPU) against the rule written over the independent model's rows
(tests/_calltree_ref.py): every guest of tests/guests_calltree.py and bignum(40), the three sum laws, what each guest is there
to show, a failing guest, and the CLI's block."""
import os
import re
import struct
import subprocess

import pytest

from dvt_circuits_amd import capi
from tests import _calltree_ref as ref
from tests import guests, guests_calltree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")
GOLD = os.path.join(ROOT, "tests", "golden")
SPAN = 4096

GUESTS = dict(guests_calltree.GUESTS, bignum=lambda: guests.bignum(40)[0])


def entry_of(elf):
    return struct.unpack_from("<I", elf, 24)[0]


def events_of(run):
    """per global position: "call", "ret" or None, as the rule classifies the model's rows"""
    out = []
    for r in ref.rows_of(run):
        ev = ref.event_of(r.ins.word)
        out.append(None if ev == "call" and r.next_pc not in run.text else ev)
    return out


@pytest.mark.parametrize("name", sorted(GUESTS))
def test_host_calltree_is_the_models(name):
    elf = GUESTS[name]()
    rc, rep, got, err = capi.execute_calltree(elf)
    assert rc == 0 and rep["halted"] and rep["exit_code"] == 0, err
    run = ref.model_run(elf)
    want = ref.tree(run)
    ref.same_tree(got, want, name)
    ref.sum_laws(got, entry_of(elf))
    s = got["summary"]
    assert s["cycles"] == rep["cycles"] == run.cycles == capi.execute(elf)[1]["cycles"]
    assert s["n_instr"] == run.n_instr and s["text_base"] == run.text_base and s["shards_total"] == 1
    print(name, s)


def test_what_the_guests_are_there_for():
    """from the model's rows: each shape stresses what its docstring says"""
    shapes = {}
    for name in guests_calltree.GUESTS:
        elf = guests_calltree.GUESTS[name]()
        shapes[name] = (elf, events_of(ref.model_run(elf)), ref.tree(ref.model_run(elf)))
    # nest: a frame covers two whole spans without an event, and a frame spans more than two shards of 2^10
    _, ev, tree = shapes["nest"]
    quiet = [k for k in range(len(ev) // SPAN) if not any(ev[k * SPAN:(k + 1) * SPAN])]
    assert len(quiet) >= 2 and tree["max_depth"] == 4
    # recurse: several spans of calls only, several of returns only, deeper than 300
    _, ev, tree = shapes["recurse"]
    kinds = [set(e for e in ev[k * SPAN:(k + 1) * SPAN] if e) for k in range(len(ev) // SPAN)]
    assert kinds.count({"call"}) >= 2 and kinds.count({"ret"}) >= 2 and tree["max_depth"] > 300
    assert min(len([e for e in ev[k * SPAN:(k + 1) * SPAN] if e]) for k in range(len(kinds)) if kinds[k] in ({"call"}, {"ret"})) > 50
    # dense: at least a third of the records are events, and a span carries more than 1300
    _, ev, _ = shapes["dense"]
    assert 3 * sum(1 for e in ev if e) >= len(ev) and max(sum(1 for e in ev[k:k + SPAN] if e) for k in range(0, len(ev), SPAN)) > 1300
    # tail: g is no function, f's frames include g's cycles; h is reached through jalr ra, t0
    elf, _, tree = shapes["tail"]
    root = entry_of(elf)
    g, f, h = root + 4, root + 12, root + 20      # behind the entry's `j main`: two instructions each
    assert tree["arcs"][(root, f)] == (2, 8) and tree["arcs"][(root, h)] == (1, 2) and all(g not in k for k in tree["arcs"]), tree["arcs"]
    # stray: one unmatched return, four frames open at the exit
    _, _, tree = shapes["stray"]
    assert tree["unmatched_returns"] == 1 and tree["open_at_exit"] == 4 and tree["max_depth"] >= 4
    # fanout: 129 distinct callees of the root
    elf, _, tree = shapes["fanout"]
    assert len([1 for (a, b) in tree["arcs"] if a == entry_of(elf)]) >= guests_calltree.FANOUT_STUBS
    # boundary: at 2^10 a CALL is the last record of a shard and a RET the last record of another
    elf = shapes["boundary"][0]
    run = ref.model_run(elf, (), 10)
    last = [ref.event_of(sh["rows"][-1].ins.word) for sh in run.shards]
    assert last[0] == "call" and last[1] == "ret" and len(run.shards[0]["rows"]) == len(run.shards[1]["rows"]) == 1024, last


def test_a_failing_guest_answers_as_execute_does():
    elf = guests.exit_with(1)
    rc, rep, got, err = capi.execute_calltree(elf)
    rc0, rep0, _, err0 = capi.execute(elf)
    assert rc == rc0 == capi.DVT_ERR_GUEST and rep == rep0 and err == err0
    assert got["summary"]["cycles"] == rep["cycles"]          # the tables of what retired come back all the same
    ref.sum_laws(got, entry_of(elf))


def test_max_cycles_cuts_the_tree_and_the_laws_hold():
    elf = guests_calltree.recurse()
    rc, rep, got, err = capi.execute_calltree(elf, max_cycles=5000)
    assert rc == capi.DVT_ERR_GUEST and rep["cycles"] == got["summary"]["cycles"] == 5000, (rc, rep, err)
    assert got["summary"]["open_at_exit"] > 100
    ref.sum_laws(got, entry_of(elf))


def block_of(stdout):
    """the --show-calls block: (frames, depth, [(inclusive, self, calls, name)])"""
    lines = stdout.splitlines()
    a = next(i for i, l in enumerate(lines) if l.startswith("call tree ("))
    frames, depth = map(int, re.fullmatch(r"call tree \((\d+) frames, depth (\d+)\):", lines[a]).groups())
    rows = []
    for l in lines[a + 1:]:
        f = l.split()
        if len(f) != 4 or not f[3].startswith("f_"):
            break
        rows.append((int(f[0]), int(f[1]), int(f[2]), f[3]))
    return frames, depth, rows


def test_cli_execute_show_calls(tmp_path):
    path = tmp_path / "hint_sum.elf"
    path.write_bytes(guests.hint_sum())
    inp = os.path.join(GOLD, "finalization_example.json")
    buf = capi.stdin_from_json("finalization", open(inp, "rb").read())
    rc, rep, got, err = capi.execute_calltree(guests.hint_sum(), [buf])
    assert rc == 0, err
    base = [CLI, "execute", "--type", "finalization", "-i", inp, "--elf", str(path)]
    r = subprocess.run(base + ["--show-calls"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    frames, depth, rows = block_of(r.stdout)
    assert frames == got["summary"]["n_frames"] and depth == got["summary"]["max_depth"]
    assert rows == [(inc, own, n, "f_%x" % pc) for pc, n, inc, own in got["funcs"]] and sum(row[1] for row in rows) == rep["cycles"]
    # without the flag every byte is as before, with and without --show-report
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0 and plain.stdout == f"input len: {len(buf) - 8}\n"
    report = subprocess.run(base + ["--show-report"], capture_output=True, text=True)
    both = subprocess.run(base + ["--show-report", "--show-calls"], capture_output=True, text=True)
    assert report.returncode == both.returncode == 0 and "call tree (" not in report.stdout
    assert both.stdout.startswith(report.stdout) and block_of(both.stdout) == (frames, depth, rows)
