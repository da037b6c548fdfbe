"""What an origin slice must say, from the independent model (oracle/rv32_model.py).

slice_of() is the rule of csrc/origin.h written over the rows of the model's shards and the pointers of its precompile events
(tests/_watch_ref._calls, _access): every node, every edge and the summary, to be compared with same().

Two yardsticks do not depend on that rule.  edges_agree(): the value an edge carries is read from the CONSUMER's record, the
node behind it is the PRODUCER the search found, and the producer's record holds what it wrote: the two must be equal, on every
edge that has a node behind it and carries a value.  root_agrees(): the root's value against the model run again and stopped at
the position (tests/_snapshot_ref.state_at)."""
import bisect
import functools

from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)
from tests._snapshot_ref import EXIT, global_of, locate, state_at  # noqa: F401
from tests._watch_ref import LOADS, STORE, STORES, _access, _calls

MAX_NODES, MAX_EDGES, MAX_DEPTH, PASS_QUESTIONS, SPAN = 1024, 8192, 64, 256, 4096
NONE = 0xFFFFFFFF
REG, WORD = 1, 2
OP, LOAD, F_STORE, CALL, SYSCALL = 1, 2, 3, 4, 5
ROOT, ADDR, RS1, RS2, MEM = 0, 1, 2, 3, 4
INITIAL, IMAGE, NO_VALUE, CUT, UNEXPANDED = 1, 2, 4, 8, 16
NODE_KEYS = ("shard", "row", "pc", "idx", "kind", "depth", "first_edge", "n_edges", "flags", "rd_value", "rs1", "rs2", "addr", "before", "after")
EDGE_KEYS = ("from", "to", "role", "target", "value", "flags", "src_shard", "src_row")
READS_RS2 = ("beq", "bne", "blt", "bge", "bltu", "bgeu", "sb", "sh", "sw", "add", "sub", "and", "or", "xor", "slt", "sltu", "mul", "mulhu", "alu")


@functools.lru_cache(maxsize=None)
def _flat(run):
    """([(shard, row, model row, the words of the row's precompile call or None)] in execution order, the writers of every
    register and of every word as ascending lists of global record numbers)"""
    flat, writers = [], {}
    for sh in run.shards:
        calls = _calls(sh)
        for i, r in enumerate(sh["rows"]):
            g = len(flat)
            flat.append((sh["index"], i, r, calls.get(i)))
            if r.ins.rd:
                writers.setdefault((REG, r.ins.rd), []).append(g)
            acc = _access(r)
            if acc and acc[0] == STORE:
                writers.setdefault((WORD, acc[1]), []).append(g)
            for addr in sorted(set(a for a, _, wr in calls.get(i, ()) if wr)):
                writers.setdefault((WORD, addr), []).append(g)
    return flat, writers


def _writer(run, what, target, g):
    """the global number of the last record before record g that writes the target, or None"""
    w = _flat(run)[1].get((what, target), ())
    k = bisect.bisect_left(w, g)
    return w[k - 1] if k else None


def _kind(r, call):
    if r.ins.kind in LOADS:
        return LOAD
    if r.ins.kind in STORES:
        return F_STORE
    if r.ins.kind == "ecall":
        return CALL if call is not None else SYSCALL
    return OP


def _inputs(r, call, follow_addr):
    """[(role, target, value, flags)] of a row, in the rule's order"""
    k, out = r.ins.kind, []
    if k in LOADS or k in STORES:
        if follow_addr and r.ins.rs1:
            out.append((ADDR, r.ins.rs1, r.b, 0))
    elif k not in ("lui", "jal", "ecall") and r.ins.rs1:
        out.append((RS1, r.ins.rs1, r.b, 0))
    if k in READS_RS2 and not r.ins.imm_form and r.ins.rs2:
        out.append((RS2, r.ins.rs2, r.c, 0))
    if k in LOADS or k in ("sb", "sh"):
        out.append((MEM, r.maddr & ~3, r.m_prev, 0))
    if k == "ecall" and call is not None:
        out += [(MEM, addr, 0, NO_VALUE) for addr, rd, _ in call if rd]
    return out


def slice_of(run, at, target, follow_addr=False, depth=MAX_DEPTH, nodes=MAX_NODES, edges=MAX_EDGES):
    """dict(summary, nodes, edges) as capi._origin gives it (the summary without ms, passes as the device counts them), and
    level_questions: the questions of every answered level"""
    flat, _ = _flat(run)
    what, tgt = target
    g_at = global_of(run, tuple(at))
    out_nodes, out_edges, node_of, node_g, levels = [], [], {}, [], []

    def resolve(e, g_q, depth_new):
        q_what = what if e["from"] == NONE else (WORD if e["role"] == MEM else REG)
        g = _writer(run, q_what, e["target"], g_q)
        root = e["from"] == NONE
        if g is None:
            e["flags"] |= INITIAL
            image = q_what == WORD and e["target"] in run.image_mem
            if image:
                e["flags"] |= IMAGE
            if root and q_what == WORD:
                if image:
                    e["value"] = run.image_mem[e["target"]]
                else:
                    e["flags"] |= NO_VALUE
            return
        shard, row, r, call = flat[g]
        e["src_shard"], e["src_row"] = shard, row
        if root:
            if q_what == REG:
                e["value"] = r.a
            elif r.ins.kind in STORES:
                e["value"] = r.m_val
            else:
                e["flags"] |= NO_VALUE
        if g in node_of:
            e["to"] = node_of[g]
        elif len(out_nodes) >= nodes:
            e["flags"] |= CUT
        else:
            acc = _access(r)
            n = dict.fromkeys(NODE_KEYS, 0)
            n.update(shard=shard, row=row, pc=r.ins.pc, idx=(r.ins.pc - run.text_base) // 4, kind=_kind(r, call), depth=depth_new, rd_value=r.a, rs1=r.b,
                     rs2=r.c)
            if acc:
                n.update(addr=acc[1], before=acc[2], after=acc[3])
            e["to"] = node_of[g] = len(out_nodes)
            out_nodes.append(n)
            node_g.append(g)

    def answer(first, depth_new):
        levels.append(len(out_edges) - first)
        for e in out_edges[first:]:
            resolve(e, g_at if e["from"] == NONE else node_g[e["from"]], depth_new)

    out_edges.append(dict(zip(EDGE_KEYS, (NONE, NONE, ROOT, tgt, 0, 0, 0, 0))))
    answer(0, 0)
    lo, hi, d = 0, len(out_nodes), 0
    while lo < hi:
        first, full = len(out_edges), False
        for i in range(lo, hi):
            ins = []
            if d < depth and not full:
                _, _, r, call = flat[node_g[i]]
                ins = _inputs(r, call, follow_addr)
                full = len(out_edges) + len(ins) > edges
            if d >= depth or full:
                out_nodes[i]["flags"] |= UNEXPANDED
                continue
            out_nodes[i]["first_edge"] = len(out_edges) if ins else 0
            out_nodes[i]["n_edges"] = len(ins)
            out_edges += [dict(zip(EDGE_KEYS, (i, NONE, role, t, v, f, 0, 0))) for role, t, v, f in ins]
        if len(out_edges) == first:
            break
        answer(first, d + 1)
        lo, hi, d = hi, len(out_nodes), d + 1
        if full:
            for n in out_nodes[lo:hi]:
                n["flags"] |= UNEXPANDED
            break
    shard, row = locate(run, g_at)
    count = lambda items, flag: sum(1 for x in items if x["flags"] & flag)
    summary = dict(position=g_at, cycles=len(flat), n_nodes=len(out_nodes), n_edges=len(out_edges), depth=max([n["depth"] for n in out_nodes] or [0]),
                   cut=count(out_edges, CUT), unexpanded=count(out_nodes, UNEXPANDED), initial=count(out_edges, INITIAL), no_value=count(out_edges, NO_VALUE),
                   questions=sum(levels), levels=len(levels), passes=sum(-(-q // PASS_QUESTIONS) for q in levels), shard=shard, row=row,
                   shards_total=len(run.shards), span=SPAN)
    return dict(summary=summary, nodes=out_nodes, edges=out_edges, level_questions=levels)


def same(got, want, host=False, where=""):
    """a slice (capi._origin's dict) against slice_of()'s: exact integers, dict for dict; host: the host path counts no passes"""
    gs = {k: v for k, v in got["summary"].items() if k != "ms"}
    ws = dict(want["summary"], passes=0 if host else want["summary"]["passes"])
    assert gs == ws, (where, sorted(set(gs.items()) ^ set(ws.items())))
    for part in ("nodes", "edges"):
        assert len(got[part]) == len(want[part]), (where, part, len(got[part]), len(want[part]))
        for k, (a, b) in enumerate(zip(got[part], want[part])):
            assert a == b, (where, part, k, sorted(set(a.items()) ^ set(b.items())))


def edges_agree(got, where=""):
    """yardstick 1; returns the number of edges checked"""
    n = 0
    for k, e in enumerate(got["edges"]):
        if e["to"] == NONE or e["flags"] & NO_VALUE:
            continue
        node = got["nodes"][e["to"]]
        assert (node["shard"], node["row"]) == (e["src_shard"], e["src_row"]), (where, k, e, node)
        if e["role"] in (RS1, RS2, ADDR):
            assert node["rd_value"] == e["value"], (where, k, e, node)
            n += 1
        elif e["role"] == MEM and node["kind"] == F_STORE:
            assert node["after"] == e["value"], (where, k, e, node)
            n += 1
    return n


def root_agrees(got, target, state, where=""):
    """yardstick 2: the root's value against the model stopped at summary.position (state_at()); returns whether it was compared"""
    root = got["edges"][0]
    what, tgt = target
    if what == REG:
        assert root["value"] == state.reg[tgt], (where, root, state.reg[tgt])
        return True
    if root["flags"] & NO_VALUE:
        return False
    assert root["value"] == state.mem.get(tgt, 0), (where, root, state.mem.get(tgt, 0))
    return True


def spans_of(got):
    """the (shard, span) pairs the nodes of a slice lie in"""
    return set((n["shard"], n["row"] // SPAN) for n in got["nodes"])
