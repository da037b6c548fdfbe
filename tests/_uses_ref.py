"""What a uses slice must say, from the independent model (oracle/rv32_model.py).

uses_of() is the rule of csrc/uses.h written over the rows of the model's shards and the pointers of its precompile events, with
the row lists, the input edges and the node kinds of tests/_origin_ref (_flat, _inputs, _kind): every node, every definition,
every edge and the summary, to be compared with same().

Three yardsticks do not depend on that rule.  inverse_of_origin(): the uses relation is the exact inverse of the origin
relation, so for every edge the origin reference's writer (_origin_ref._writer) of the target before the consumer must be the
definition's record; for the root, no writer may lie between the position and the consumer.  counts_agree(): n_uses of every
definition against a count over ALL of the model's rows: a row counts once per input that names the target when its writer is
the definition's record.  values_agree(): the consumer's record holds the value it read, and that is the definition's value."""
import bisect
import functools

from tests._origin_ref import _flat, _inputs, _kind, _writer
from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)
from tests._snapshot_ref import EXIT, global_of, locate  # noqa: F401
from tests._watch_ref import STORES, _access

MAX_NODES, MAX_DEFS, MAX_EDGES, MAX_DEPTH, MAX_FAN, DEFAULT_FAN, PASS_DEFS, SPAN = 1024, 4096, 8192, 64, 16, 8, 256, 4096
NONE = 0xFFFFFFFF
REG, WORD = 1, 2
OP, LOAD, F_STORE, CALL, SYSCALL = 1, 2, 3, 4, 5
ADDR, RS1, RS2, MEM = 1, 2, 3, 4
LIVE_AT_EXIT, TRUNCATED, NO_VALUE, CUT, UNEXPANDED = 1, 2, 4, 8, 16
NODE_KEYS = ("shard", "row", "pc", "idx", "kind", "depth", "first_def", "n_defs", "flags", "rd_value", "rs1", "rs2", "addr", "before", "after")
DEF_KEYS = ("n_uses", "node", "what", "target", "value", "flags", "next_shard", "next_row", "first_edge", "n_edges")
EDGE_KEYS = ("def", "to", "role", "flags", "dst_shard", "dst_row")


def what_of(role):
    return WORD if role == MEM else REG


@functools.lru_cache(maxsize=None)
def _readers(run, follow_addr):
    """(what, target) -> [(global record number, role, value, flags)] in execution order, within a record in the rule's order"""
    out = {}
    for g, (_, _, r, call) in enumerate(_flat(run)[0]):
        for role, tgt, value, fl in _inputs(r, call, follow_addr):
            out.setdefault((what_of(role), tgt), []).append((g, role, value, fl))
    return out


@functools.lru_cache(maxsize=None)
def _global(run):
    """(shard, row) -> global record number"""
    return {(shard, row): g for g, (shard, row, _, _) in enumerate(_flat(run)[0])}


def _outputs(r, call):
    """[(what, target, value, flags)] a row defines, in the rule's order"""
    out = []
    if r.ins.rd:
        out.append((REG, r.ins.rd, r.a, 0))
    acc = _access(r)
    if acc and r.ins.kind in STORES:
        out.append((WORD, acc[1], acc[3], 0))
    if r.ins.kind == "ecall" and call is not None:
        out += [(WORD, addr, 0, NO_VALUE) for addr, _, wr in call if wr]
    return out


def uses_of(run, at, target, follow_addr=False, depth=MAX_DEPTH, fan=DEFAULT_FAN, nodes=MAX_NODES, defs=MAX_DEFS, edges=MAX_EDGES):
    """dict(summary, nodes, defs, edges) as capi._uses gives it (the summary without ms, passes as the device counts them), and
    level_defs: the definitions of every answered level"""
    flat, writers = _flat(run)
    readers = _readers(run, bool(follow_addr))
    g_at = global_of(run, tuple(at))
    out_nodes, out_defs, out_edges, node_of, node_g, def_from, levels = [], [], [], {}, [], [], []

    def new_def(node, what, tgt, value, flags, g_from):
        out_defs.append(dict(zip(DEF_KEYS, (0, node, what, tgt, value, flags, NONE, NONE, 0, 0))))
        def_from.append(g_from)

    def resolve(di, depth_new):
        d, g_from = out_defs[di], def_from[di]
        w = writers.get((d["what"], d["target"]), ())
        k = bisect.bisect_left(w, g_from)
        g_next = w[k] if k < len(w) else None
        if g_next is None:
            d["flags"] |= LIVE_AT_EXIT
        else:
            d["next_shard"], d["next_row"] = flat[g_next][0], flat[g_next][1]
        rd = readers.get((d["what"], d["target"]), ())
        lo = bisect.bisect_left(rd, (g_from,))
        hi = len(rd) if g_next is None else bisect.bisect_left(rd, (g_next + 1,))
        d["n_uses"] = hi - lo
        if hi - lo > fan:
            d["flags"] |= TRUNCATED
        kept = rd[lo:min(hi, lo + fan)]
        d["first_edge"], d["n_edges"] = (len(out_edges) if kept else 0), len(kept)
        if d["node"] == NONE:
            if not kept or kept[0][3] & NO_VALUE:
                d["flags"] |= NO_VALUE
            else:
                d["value"] = kept[0][2]
        for g, role, _, _ in kept:
            shard, row, r, call = flat[g]
            e = dict(zip(EDGE_KEYS, (di, NONE, role, 0, shard, row)))
            if g in node_of:
                e["to"] = node_of[g]
            elif len(out_nodes) >= nodes:
                e["flags"] |= CUT
            else:
                acc = _access(r)
                n = dict.fromkeys(NODE_KEYS, 0)
                n.update(shard=shard, row=row, pc=r.ins.pc, idx=(r.ins.pc - run.text_base) // 4, kind=_kind(r, call), depth=depth_new, rd_value=r.a,
                         rs1=r.b, rs2=r.c)
                if acc:
                    n.update(addr=acc[1], before=acc[2], after=acc[3])
                e["to"] = node_of[g] = len(out_nodes)
                out_nodes.append(n)
                node_g.append(g)
            out_edges.append(e)

    new_def(NONE, target[0], target[1], 0, 0, g_at)
    lo, d, full = 0, 0, False
    while lo < len(out_defs):
        hi, node_lo = len(out_defs), len(out_nodes)
        levels.append(hi - lo)
        for di in range(lo, hi):
            resolve(di, d + 1)
        if full:
            for n in out_nodes[node_lo:]:
                n["flags"] |= UNEXPANDED
            break
        lo = hi
        for i in range(node_lo, len(out_nodes)):
            n, outs = out_nodes[i], []
            if n["depth"] < depth and not full:
                _, _, r, call = flat[node_g[i]]
                outs = _outputs(r, call)
                full = len(out_defs) + len(outs) > defs or len(out_edges) + (len(out_defs) - lo + len(outs)) * fan > edges
            if n["depth"] >= depth or full:
                n["flags"] |= UNEXPANDED
                continue
            n["first_def"], n["n_defs"] = (len(out_defs) if outs else 0), len(outs)
            for what, tgt, value, fl in outs:
                new_def(i, what, tgt, value, fl, node_g[i] + 1)
        d += 1
    shard, row = locate(run, g_at)
    count = lambda items, flag: sum(1 for x in items if x["flags"] & flag)
    summary = dict(position=g_at, cycles=len(flat), uses_total=sum(x["n_uses"] for x in out_defs), n_nodes=len(out_nodes), n_defs=len(out_defs),
                   n_edges=len(out_edges), depth=max([n["depth"] for n in out_nodes] or [0]), cut=count(out_edges, CUT),
                   unexpanded=count(out_nodes, UNEXPANDED), truncated=count(out_defs, TRUNCATED), live_at_exit=count(out_defs, LIVE_AT_EXIT),
                   no_value=count(out_defs, NO_VALUE), dead=sum(1 for x in out_defs if not x["n_uses"]), levels=len(levels),
                   passes=sum(-(-q // PASS_DEFS) for q in levels), shard=shard, row=row, shards_total=len(run.shards), span=SPAN)
    return dict(summary=summary, nodes=out_nodes, defs=out_defs, edges=out_edges, level_defs=levels)


def same(got, want, host=False, where=""):
    """a slice (capi._uses's dict) against uses_of()'s: exact integers, dict for dict; host: the host path counts no passes"""
    gs = {k: v for k, v in got["summary"].items() if k != "ms"}
    ws = dict(want["summary"], passes=0 if host else want["summary"]["passes"])
    assert gs == ws, (where, sorted(set(gs.items()) ^ set(ws.items())))
    for part in ("nodes", "defs", "edges"):
        assert len(got[part]) == len(want[part]), (where, part, len(got[part]), len(want[part]))
        for k, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, (where, part, k, sorted(set(a.items()) ^ set(b.items())))


def _def_g(got, run, d):
    """the global record number of a definition's record (None: the root)"""
    if d["node"] == NONE:
        return None
    n = got["nodes"][d["node"]]
    return _global(run)[(n["shard"], n["row"])]


def inverse_of_origin(got, run, where=""):
    """yardstick 1; returns the number of edges checked"""
    g_p = got["summary"]["position"]
    for k, e in enumerate(got["edges"]):
        d = got["defs"][e["def"]]
        assert what_of(e["role"]) == d["what"], (where, k, e, d)
        g_c = _global(run)[(e["dst_shard"], e["dst_row"])]
        w = _writer(run, d["what"], d["target"], g_c)
        if d["node"] == NONE:
            assert g_c >= g_p and (w is None or w < g_p), (where, k, e, d, w)
        else:
            assert w == _def_g(got, run, d), (where, k, e, d, w)
    return len(got["edges"])


@functools.lru_cache(maxsize=None)
def _read_by(run, follow_addr, what, target):
    """every row of the run that reads the target, once per input that names it: [(global record number, the origin reference's
    writer of the target before it)], and how many of them each writer has"""
    pairs = [(g, _writer(run, what, target, g)) for g, _, _, _ in _readers(run, follow_addr).get((what, target), ())]
    per = {}
    for _, w in pairs:
        per[w] = per.get(w, 0) + 1
    return pairs, per


def counts_agree(got, run, follow_addr=False, where=""):
    """yardstick 2; returns the sum of the counts"""
    g_p, total = got["summary"]["position"], 0
    for k, d in enumerate(got["defs"]):
        pairs, per = _read_by(run, bool(follow_addr), d["what"], d["target"])
        g_d = _def_g(got, run, d)
        n = sum(1 for g, w in pairs if g >= g_p and (w is None or w < g_p)) if g_d is None else per.get(g_d, 0)
        assert n == d["n_uses"], (where, k, d, n)
        assert bool(d["flags"] & TRUNCATED) == (n > d["n_edges"]) and d["n_edges"] <= n, (where, k, d)
        total += n
    assert total == got["summary"]["uses_total"], (where, total)
    return total


def values_agree(got, where=""):
    """yardstick 3; returns the number of edges compared"""
    n = 0
    for k, e in enumerate(got["edges"]):
        d = got["defs"][e["def"]]
        if e["to"] == NONE or d["flags"] & NO_VALUE:
            continue
        node = got["nodes"][e["to"]]
        assert (node["shard"], node["row"]) == (e["dst_shard"], e["dst_row"]), (where, k, e, node)
        if e["role"] in (ADDR, RS1):
            assert node["rs1"] == d["value"], (where, k, e, d, node)
        elif e["role"] == RS2:
            assert node["rs2"] == d["value"], (where, k, e, d, node)
        elif node["kind"] in (LOAD, F_STORE):
            assert node["before"] == d["value"], (where, k, e, d, node)
        else:
            continue      # a call's read: the records do not hold the word
        n += 1
    return n


def check(got, run, want, follow_addr=False, host=False, where=""):
    """same() and the three yardsticks; returns (edges checked, uses counted, values compared)"""
    same(got, want, host, where)
    return inverse_of_origin(got, run, where), counts_agree(got, run, follow_addr, where), values_agree(got, where)


def shape_of(want, run):
    """what a slice exercises, as a set of names: the tests assert these on the reference's answer so that no case is vacuous.
    window_crosses_span / _shard: some [F, N] does; kept_in_two_spans / _shards: the kept uses of one definition lie in two;
    truncated, dead, live_at_exit, no_value_used (a NO_VALUE definition with uses), next_is_use (a next writer among its own
    definition's kept uses), wide_level (more than PASS_DEFS definitions in a level), cut, unexpanded"""
    flat, out = _flat(run)[0], set()
    for d in want["defs"]:
        if d["node"] == NONE:
            g = want["summary"]["position"]
        else:
            n = want["nodes"][d["node"]]
            g = _global(run)[(n["shard"], n["row"])] + 1
        es = want["edges"][d["first_edge"]:d["first_edge"] + d["n_edges"]]
        if d["next_shard"] != NONE and g < len(flat):
            if d["next_shard"] != flat[g][0]:
                out.add("window_crosses_shard")
            elif d["next_row"] // SPAN != flat[g][1] // SPAN:
                out.add("window_crosses_span")
            if any((e["dst_shard"], e["dst_row"]) == (d["next_shard"], d["next_row"]) for e in es):
                out.add("next_is_use")
        if len({(e["dst_shard"], e["dst_row"] // SPAN) for e in es}) > 1:
            out.add("kept_in_two_spans")
        if len({e["dst_shard"] for e in es}) > 1:
            out.add("kept_in_two_shards")
        for flag, name in ((TRUNCATED, "truncated"), (LIVE_AT_EXIT, "live_at_exit")):
            if d["flags"] & flag:
                out.add(name)
        if not d["n_uses"]:
            out.add("dead")
        if d["flags"] & NO_VALUE and d["n_uses"]:
            out.add("no_value_used")
    if max(want["level_defs"]) > PASS_DEFS:
        out.add("wide_level")
    if want["summary"]["cut"]:
        out.add("cut")
    if want["summary"]["unexpanded"]:
        out.add("unexpanded")
    return out


def store_load_op_store(want):
    """the nodes (store, load, op, store) of a chain in a slice: a store whose word a load reads, whose register an op reads,
    whose register a store writes out (RS2); None when the slice has none"""
    nodes, defs, edges = want["nodes"], want["defs"], want["edges"]

    def consumers(node, what):
        for d in defs:
            if d["node"] == node and d["what"] == what:
                for e in edges[d["first_edge"]:d["first_edge"] + d["n_edges"]]:
                    if e["to"] != NONE:
                        yield e["to"], e["role"]
    for a, n in enumerate(nodes):
        if n["kind"] != F_STORE:
            continue
        for b, role in consumers(a, WORD):
            if nodes[b]["kind"] != LOAD or role != MEM:
                continue
            for c, _ in consumers(b, REG):
                if nodes[c]["kind"] != OP:
                    continue
                for d, role in consumers(c, REG):
                    if nodes[d]["kind"] == F_STORE and role == RS2:
                        return a, b, c, d
    return None
