"""What the call-tree report must say, from the independent model (oracle/rv32_model.py): the rule of csrc/calltree.h written
sequentially over the rows of the model's shards (tests/_profile_ref.model_run), reading r.ins.word, r.ins.pc and r.next_pc
as _profile_ref.tally does.  Functions and arcs are named by pc; the root's caller is None."""
import collections

from tests._profile_ref import model_run  # noqa: F401  (the tests take the run from here)


def event_of(word):
    op, rd = word & 0x7F, (word >> 7) & 31
    if op in (0x6F, 0x67) and rd == 1:
        return "call"
    if op == 0x67 and rd == 0 and (word >> 15) & 31 == 1 and word >> 20 == 0:
        return "ret"
    return None


def rows_of(run):
    return [r for sh in run.shards for r in sh["rows"]]


def tree(run):
    """dict(cycles, arcs = {(caller_pc or None, callee_pc): (calls, cycles)}, funcs = [(pc, calls, inclusive, self)] by self
    descending then pc, n_frames, unmatched_returns, max_depth, open_at_exit)"""
    rows = rows_of(run)
    arcs = collections.defaultdict(lambda: [0, 0])
    stack, unmatched, max_depth = [], 0, 0   # frames (fn, open); the caller of stack[k] is stack[k - 1]

    def close(end):
        fn, opened = stack.pop()
        a = arcs[(stack[-1][0] if stack else None, fn)]
        a[0] += 1
        a[1] += end - opened
    for g, r in enumerate(rows):
        if g == 0:
            stack.append((r.ins.pc, 0))
        max_depth = max(max_depth, len(stack))
        ev = event_of(r.ins.word)
        if ev == "call" and r.next_pc in run.text:
            stack.append((r.next_pc, g + 1))
            max_depth = max(max_depth, len(stack))
        elif ev == "ret":
            if len(stack) > 1:
                close(g + 1)
            else:
                unmatched += 1
    open_at_exit = len(stack)
    while stack:
        close(len(rows))
    calls, incl, out = collections.Counter(), collections.Counter(), collections.Counter()
    for (caller, fn), (n, cyc) in arcs.items():
        calls[fn] += n
        incl[fn] += cyc
        if caller is not None:
            out[caller] += cyc
    funcs = sorted(((pc, calls[pc], incl[pc], incl[pc] - out[pc]) for pc in calls), key=lambda f: (-f[3], f[0]))
    return dict(cycles=len(rows), arcs={k: tuple(v) for k, v in arcs.items()}, funcs=funcs, n_frames=sum(v[0] for v in arcs.values()),
                unmatched_returns=unmatched, max_depth=max_depth, open_at_exit=open_at_exit)


def sum_laws(got, entry_pc=None):
    """the three sum laws from the report's own outputs: sum of self = cycles (when nothing was dropped), arc calls + dropped =
    frames, the root's arc = cycles"""
    s = got["summary"]
    assert sum(a[2] for a in got["arcs"]) + s["dropped_frames"] == s["n_frames"], s
    assert len(got["arcs"]) == s["n_arcs"] and len(got["funcs"]) == s["n_funcs"]
    roots = [a for a in got["arcs"] if a[0] is None]
    if s["cycles"]:
        assert len(roots) == 1 and roots[0][2] == 1 and roots[0][3] == s["cycles"], roots
        assert entry_pc is None or roots[0][1] == entry_pc
    if s["dropped_frames"]:
        assert s["n_funcs"] == 0 and s["dropped_cycles"] > 0
    else:
        assert s["dropped_cycles"] == 0 and sum(f[3] for f in got["funcs"]) == s["cycles"], s


def same_tree(got, want, where=""):
    """a report (capi._calltree's dict) against tree()'s, everything but the time"""
    s = got["summary"]
    assert s["cycles"] == want["cycles"], (where, s["cycles"], want["cycles"])
    key = lambda a: (0xffffffff if a[0] is None else a[0], a[1])
    assert got["arcs"] == sorted(got["arcs"], key=key), where
    got_arcs = {(a, b): (n, c) for a, b, n, c in got["arcs"]}
    assert len(got_arcs) == len(got["arcs"]) and got_arcs == want["arcs"], (where, sorted(set(got_arcs.items()) ^ set(want["arcs"].items()), key=str)[:8])
    assert got["funcs"] == want["funcs"], (where, got["funcs"][:4], want["funcs"][:4])
    for k in ("n_frames", "unmatched_returns", "max_depth", "open_at_exit"):
        assert s[k] == want[k], (where, k, s[k], want[k])
    assert s["dropped_frames"] == s["dropped_cycles"] == 0, (where, s)
    sum_laws(got)
