"""What a watchpoint search must find, from the independent model (oracle/rv32_model.py): the rule of csrc/watch.h written over
the rows of the model's shards (their a / b / c, maddr, m_prev, m_val and the (shard, clk) pair `mem` the access found on its
word) and over the pointers of its precompile events.  search() gives, per query, the total and the FULL ordered hit list; the
tests slice the first and the last K from it."""
from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)

PC, REG, MEM = 1, 2, 3
LOAD, STORE, PRE_READ, PRE_WRITE, VALUE, NO_VALUE = 1, 2, 4, 8, 16, 32
LOADS, STORES = ("lb", "lh", "lw", "lbu", "lhu"), ("sb", "sh", "sw")
SHA_EXTEND, SHA_COMPRESS = 0x00300105, 0x00010106
HIT_KEYS = ("query", "shard", "row", "pc", "idx", "kind", "flags", "addr", "n_words", "before", "after", "rd_value", "rs1", "rs2",
            "prev_shard", "prev_clk")


def _calls(sh):
    """the precompile calls of a shard by the row that made them: row index -> [(word address, is read, is write)] in the
    order of the call's arrays.  The events of a kind are in execution order, and so are the ECALL rows with that id."""
    ext, cmp_, big = iter(sh["sha_ext"]), iter(sh["sha_cmp"]), iter(sh["big"])
    out = {}
    for i, r in enumerate(sh["rows"]):
        if r.ins.kind != "ecall" or r.mem is None:    # (the calls with shapes read a1 through the port, and so does COMMIT)
            continue
        if r.b == SHA_EXTEND:
            ev = next(ext)
            assert ev["ptr"] == r.c
            out[i] = [(ev["ptr"] + 4 * k, k < 16, k >= 16) for k in range(64)]
        elif r.b == SHA_COMPRESS:
            ev = next(cmp_)
            assert (ev["w_ptr"], ev["h_ptr"]) == (r.c, r.m_prev)
            out[i] = [(ev["w_ptr"] + 4 * k, True, False) for k in range(64)] + [(ev["h_ptr"] + 4 * k, True, True) for k in range(8)]
        elif r.b != 0x10:
            ev = next(big)
            assert ev["a_ptr"] == r.c and (not ev["bprev"] or ev["b_ptr"] == r.m_prev)
            out[i] = [(ev["a_ptr"] + 4 * k, True, True) for k in range(len(ev["aprev"]))] + \
                     [(ev["b_ptr"] + 4 * k, True, False) for k in range(len(ev["bprev"]))]
    assert next(ext, None) is None and next(cmp_, None) is None and next(big, None) is None
    return out


def _access(r):
    """(direction, word, before, after, prev) of a load or store row, else None"""
    if r.ins.kind in LOADS:
        return LOAD, r.maddr & ~3, r.m_prev, r.m_prev, r.mem
    if r.ins.kind in STORES:
        return STORE, r.maddr & ~3, r.m_prev, r.m_val, r.mem
    return None


def search(run, queries, positions=None):
    """[dict(total, hits = [hit dicts in execution order])] per query, over the model's shards at those positions (None: all);
    queries are the dicts of capi.watch_pc / watch_reg / watch_mem"""
    shards = run.shards if positions is None else [run.shards[k] for k in positions]
    found = [[] for _ in queries]
    for sh in shards:
        calls = _calls(sh)
        for row, r in enumerate(sh["rows"]):
            acc = _access(r)
            for qi, q in enumerate(queries):
                if not (q["from_shard"], q["from_row"]) <= (sh["index"], row) < (q["to_shard"], q["to_row"]):
                    continue
                hit = dict.fromkeys(HIT_KEYS, 0)
                if q["kind"] == PC:
                    ok = q["lo"] <= r.ins.pc < q["hi"]
                elif q["kind"] == REG:
                    ok = r.ins.rd == q["lo"] and q["lo"] != 0 and (not q["flags"] & VALUE or (r.a ^ q["want"]) & q["mask"] == 0)
                elif acc:
                    ok = bool(acc[0] & q["flags"]) and q["lo"] <= acc[1] < q["hi"] and (not q["flags"] & VALUE or (acc[3] ^ q["want"]) & q["mask"] == 0)
                else:
                    words = [(addr, (PRE_READ if rd and q["flags"] & PRE_READ else 0) | (PRE_WRITE if wr and q["flags"] & PRE_WRITE else 0))
                             for addr, rd, wr in calls.get(row, ()) if q["lo"] <= addr < q["hi"]]
                    words = [(addr, d) for addr, d in words if d]
                    ok = bool(words) and not q["flags"] & VALUE
                    if ok:
                        dirs = 0
                        for _, d in words:
                            dirs |= d
                        hit.update(flags=dirs | NO_VALUE, addr=min(addr for addr, _ in words), n_words=len(words))
                if not ok:
                    continue
                hit.update(query=qi, shard=sh["index"], row=row, pc=r.ins.pc, idx=(r.ins.pc - run.text_base) // 4, kind=q["kind"], rd_value=r.a, rs1=r.b,
                           rs2=r.c)
                if acc:
                    hit.update(flags=acc[0], addr=acc[1], n_words=1, before=acc[2], after=acc[3], prev_shard=acc[4][0], prev_clk=acc[4][1])
                found[qi].append(hit)
    return [dict(total=len(h), hits=h) for h in found]


def sliced(want, keep):
    """what a call with that `keep` returns, from search()'s lists"""
    return [dict(total=w["total"], first=w["hits"][:keep], last=w["hits"][max(0, w["total"] - keep):] if keep else []) for w in want]


def same(got, want, keep, where=""):
    """a call's answer against search()'s"""
    exp = sliced(want, keep)
    assert len(got) == len(exp), where
    for qi, (g, e) in enumerate(zip(got, exp)):
        assert g["total"] == e["total"], (where, qi, g["total"], e["total"])
        for part in ("first", "last"):
            assert len(g[part]) == len(e[part]), (where, qi, part)
            for k, (a, b) in enumerate(zip(g[part], e[part])):
                assert a == b, (where, qi, part, k, sorted(set(a.items()) ^ set(b.items())))
