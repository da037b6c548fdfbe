#!/usr/bin/env python3
"""Busy, idle and cross-queue overlap of one timed call in a rocprofv3 --kernel-trace run:
    python tools/overlap.py DIR [--per-call K] [--call I] [--phase 1|2]
tools/gaps.py sums kernel durations on the assumption of one stream; with several prover lanes kernels of different queues
run at the same time.  A call is delimited by k0_cpu_rows launches (phase 1 runs K0 once per shard: K launches per call,
default 32, the bench's 32-shard execution); --call picks the call (default -2: the last complete one).  Prints the union
of busy intervals, the idle time, the time with kernels of at least two queues running, and the per-queue sums.  --phase
cuts the call at its last phase-1 kernel, the one before the first LogUp kernel (perm_*) of the call: 1 is the part up to
it (phase 1 of every shard), 2 the rest."""
import argparse
import csv
import glob


def load(d):
    rows = []
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            q = r.get("Queue_Id") or r.get("Stream_Id") or "0"
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), q, r["Kernel_Name"]))
    rows.sort()
    return rows


def window(rows, per_call, call):
    """the kernels from the first k0_cpu_rows launch of call `call` to the first of the next call"""
    k0 = [i for i, r in enumerate(rows) if "k0_cpu_rows" in r[3]]
    starts = k0[::per_call] if len(k0) % per_call == 0 else k0[len(k0) % per_call::per_call]
    starts = starts + [len(rows)]
    if len(starts) < 2:
        raise SystemExit("no complete call of %d k0_cpu_rows launches in the trace" % per_call)
    i = call % (len(starts) - 1)
    return rows[starts[i]:starts[i + 1]]


def phase(win, which):
    """the part of a call's kernels before (1) or from (2) its first perm_* kernel"""
    cut = next((i for i, r in enumerate(win) if "perm_" in r[3]), len(win))
    return win[:cut] if which == 1 else win[cut:]


def analyse(win):
    """(wall, busy union, time with >= 2 queues busy, {queue: summed kernel time}) in ns"""
    ev = []
    per_q = {}
    for s, e, q, _ in win:
        ev.append((s, 1, q))
        ev.append((e, -1, q))
        per_q[q] = per_q.get(q, 0) + (e - s)
    ev.sort(key=lambda x: (x[0], x[1]))
    active = {}
    busy = multi = 0
    last = ev[0][0] if ev else 0
    for t, d, q in ev:
        n_q = sum(1 for v in active.values() if v > 0)
        if n_q >= 1:
            busy += t - last
        if n_q >= 2:
            multi += t - last
        active[q] = active.get(q, 0) + d
        last = t
    wall = (max(e for _, e, _, _ in win) - win[0][0]) if win else 0
    return wall, busy, multi, per_q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--per-call", type=int, default=32)
    ap.add_argument("--call", type=int, default=-2)
    ap.add_argument("--phase", type=int, choices=(0, 1, 2), default=0, help="1 / 2: that phase of the call only")
    a = ap.parse_args()
    win = window(load(a.dir), a.per_call, a.call)
    if a.phase:
        win = phase(win, a.phase)
    wall, busy, multi, per_q = analyse(win)
    print("kernels %d  wall %.2f ms  busy (union) %.2f ms  idle %.2f ms  >=2 queues busy %.2f ms" %
          (len(win), wall / 1e6, busy / 1e6, (wall - busy) / 1e6, multi / 1e6))
    for q, t in sorted(per_q.items(), key=lambda kv: -kv[1]):
        print("  queue %-6s kernels %.2f ms" % (q, t / 1e6))


if __name__ == "__main__":
    main()
