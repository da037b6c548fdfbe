"""What the memory report must say, from the independent model (oracle/rv32_model.py): the rule of csrc/memreport.h written
over the rows of the model's shards (their maddr and the (shard, clk) pair `mem` the access found on its word) and over the
prev / wprev / hprev / aprev / bprev lists of its precompile events; the height of mem_init from the model's mem_rows()."""
import collections

import numpy as np

from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)

PAGE = 4096
LOADS, STORES = ("lb", "lh", "lw", "lbu", "lhu"), ("sb", "sh", "sw")
COUNTERS = ("loads", "stores", "pre_reads", "pre_writes", "first")
NEVER = (0, 0)


def report(run, positions=None):
    """the report of the model's shards at those positions (None: all, the whole execution): dict(summary = the figures of
    dvt_memory_summary the model can know, first_touch (numpy u64 over the text), pages = [dict as capi._memory gives them],
    pre_first = the precompile words whose previous access is (0, 0))"""
    whole = positions is None
    shards = run.shards if whole else [run.shards[k] for k in positions]
    first_touch = np.zeros(run.n_instr, np.uint64)
    pages = collections.defaultdict(lambda: dict({k: 0 for k in COUNTERS}, words=set()))
    sp, totals = [], collections.Counter()

    def page_of(addr):
        assert addr % 4 == 0 and 32 <= addr < 0x38000000, hex(addr)
        pg = pages[addr // PAGE * PAGE]
        pg["words"].add(addr)
        return pg

    def call_word(addr, read, write, prev):
        pg = page_of(addr)
        pg["pre_reads"] += read
        pg["pre_writes"] += write
        totals["pre_first"] += prev == NEVER
    for sh in shards:
        totals["cycles"] += len(sh["rows"])
        for r in sh["rows"]:
            if r.ins.rd == 2:
                sp.append(r.a)
            if r.ins.kind in LOADS + STORES:
                pg = page_of(r.maddr & ~3)
                pg["loads" if r.ins.kind in LOADS else "stores"] += 1
                if r.mem == NEVER:
                    pg["first"] += 1
                    first_touch[(r.ins.pc - run.text_base) // 4] += 1
        for ev in sh["sha_ext"]:
            for k in range(64):
                call_word(ev["ptr"] + 4 * k, k < 16, k >= 16, ev["prev"][k])
        for ev in sh["sha_cmp"]:
            for k in range(64):
                call_word(ev["w_ptr"] + 4 * k, 1, 0, ev["wprev"][k])
            for k in range(8):
                call_word(ev["h_ptr"] + 4 * k, 1, 1, ev["hprev"][k])
        for ev in sh["big"]:
            for k, prev in enumerate(ev["bprev"]):
                call_word(ev["b_ptr"] + 4 * k, 1, 0, prev)
            for k, prev in enumerate(ev["aprev"]):
                call_word(ev["a_ptr"] + 4 * k, 1, 1, prev)
        totals["pre_calls"] += len(sh["sha_ext"]) + len(sh["sha_cmp"]) + len(sh["big"])
    out_pages = [dict(page=addr, words=len(pg["words"]), **{k: pg[k] for k in COUNTERS}) for addr, pg in sorted(pages.items())]
    accessed = set().union(*(pg["words"] for pg in pages.values())) if pages else set()
    s = {k: sum(pg[k] for pg in out_pages) for k in ("loads", "stores", "pre_reads", "pre_writes", "words")}
    s.update(cycles=totals["cycles"], pre_calls=totals["pre_calls"], first_touches=int(first_touch.sum()), n_pages=len(out_pages),
             image_words=len(run.image_mem), image_words_accessed=len(accessed & set(run.image_mem)),
             mem_init_rows=len(run.mem_rows()) if whole else 0, sp_writes=len(sp), sp_min=min(sp, default=0), sp_max=max(sp, default=0),
             text_base=run.text_base, n_instr=run.n_instr, page_bytes=PAGE, shards_tallied=len(shards), shards_total=len(run.shards))
    return dict(summary=s, first_touch=first_touch, pages=out_pages, pre_first=totals["pre_first"])


def laws(got):
    """what holds between the report's own outputs"""
    s = got["summary"]
    assert int(got["first_touch"].sum()) == s["first_touches"] == sum(pg["first"] for pg in got["pages"]), s
    for k in ("words", "loads", "stores", "pre_reads", "pre_writes"):
        assert sum(pg[k] for pg in got["pages"]) == s[k], (k, s)
    assert len(got["pages"]) == s["n_pages"] and [pg["page"] for pg in got["pages"]] == sorted(set(pg["page"] for pg in got["pages"]))
    assert all(pg["page"] % PAGE == 0 and 0 < pg["words"] <= PAGE // 4 and pg["first"] <= pg["words"] for pg in got["pages"])
    assert s["image_words_accessed"] <= min(s["image_words"], s["words"]) and s["first_touches"] <= s["words"]
    if s["shards_tallied"] == s["shards_total"]:
        assert s["mem_init_rows"] == 32 + s["image_words"] + s["words"] - s["image_words_accessed"], s
    else:
        assert s["mem_init_rows"] == 0


def same_report(got, want, where="", shards=True):
    """a report (capi._memory's dict) against report()'s, everything but the time (and the shard counts when shards is False)"""
    gs = dict(got["summary"])
    gs.pop("ms")
    ws = dict(want["summary"])
    if not shards:
        for k in ("shards_tallied", "shards_total"):
            gs.pop(k), ws.pop(k)
    assert gs == ws, (where, sorted(set(gs.items()) ^ set(ws.items())))
    assert np.array_equal(got["first_touch"], want["first_touch"]), (where, np.nonzero(got["first_touch"] != want["first_touch"])[0][:8])
    assert got["pages"] == want["pages"], (where, [p for p in got["pages"] if p not in want["pages"]][:4], [p for p in want["pages"] if p not in got["pages"]][:4])
    laws(got)
    if "pre_first" in want and gs.get("mem_init_rows"):
        # the documented identity of a whole execution: the words no load or store touched first were touched first by a call
        assert gs["words"] - gs["first_touches"] == want["pre_first"], (where, gs["words"], gs["first_touches"], want["pre_first"])
