#!/usr/bin/env python3
"""The forgery hunt of a guest's chip tables on the GPU (dvt_rv32_hunt_shard): which one- and two-cell changes of a trace does
nothing reject?

    python tools/hunt_cells.py --guest 'arith(commit=True)' [--chips cpu,shift] [--rows FIRST:COUNT] [--json OUT]
    python tools/hunt_cells.py --elf guest.elf [--stdin FILE ...]

The guest is an expression over the functions of tests/guests*.py (its ELF is the value, or the first element of it), or an
ELF file with its stdin buffers.  The job is prepared once; every named chip (default: all the shard has) is hunted over all
rows or the window: single cells, same-row pairs and adjacent pairs (--no-pairs: single cells only; --pair-modes same_row:
not the adjacent pairs).  Prints the free-cell
counts per column name and the reported pairs grouped by column-name pair; --json writes the same as JSON (one file per
chip when the path holds {chip}), with the wall time and the evaluations per second of every run.  A hunt whose candidates
x touched rows exceed --max-evals is recorded as skipped.

    python tools/hunt_cells.py --join --guest 'shifts()' --chips cpu,shift [--supply program,byte,mem_image]
                               [--rows-per-chip N] [--shards 0,1] [--json OUT]

--join runs the join hunt instead (dvt_rv32_hunt_join_job): the chips of --chips (required) are hunted on every shard of
--shards (default: --shard), over all rows or the first N rows of each table, and the tables of --supply in the first shard
supply; it finds pairs of cells of different tables or distant rows whose multiset differences cancel, and single cells that a
supply table absorbs.  Prints every group as its two sides, each by (chip, column, delta) with the count and the lowest row, and
the absorbed cells by column; writes the same as JSON, by default profiles/r10_hunt_join_<guest>.json."""
import argparse
import collections
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P = 2013265921
DELTAS = [1, P - 1, 256, P - 256, 2, 0x78]   # those of the CPU hunter (tests/test_soundness_pairs.py)


def guest_elf(expr):
    scope = {}
    for mod in ("guests", "guests_bls", "guests_finalization", "guests_share"):
        m = importlib.import_module("tests." + mod)
        scope.update({k: getattr(m, k) for k in dir(m) if not k.startswith("_") and k not in scope})
    v = eval(expr if "(" in expr else expr + "()", scope)   # noqa: S307 (the caller's own command line)
    return v if isinstance(v, (bytes, bytearray)) else v[0]


def groups_of(reported, names):
    """reported pairs by (column name, column name): count, deltas seen, lowest row, one record"""
    g = collections.OrderedDict()
    for e in reported:
        key = "%s , %s" % (names[e["col"][0]], names[e["col"][1]])
        d = g.setdefault(key, dict(count=0, deltas=[], first_row=e["row"], example=e))
        d["count"] += 1
        if e["delta"] not in d["deltas"]:
            d["deltas"].append(e["delta"])
    return g


def signed(delta):
    return "+%d" % delta if delta <= P // 2 else "-%d" % (P - delta)


def side_summary(side, desc):
    """the cells of one side of a group by (chip, column, delta): count and lowest row"""
    g = collections.OrderedDict()
    for c in side:
        key = "%s.%s %s" % (desc.chips[c["chip"]].name, desc.chips[c["chip"]].main_names[c["col"]], signed(c["delta"]))
        d = g.setdefault(key, dict(count=0, first_row=c["row"], first_shard=c["tag"]))
        d["count"] += 1
    return g


def run_join(a, p, capi, desc, pk, job, rep, deltas):
    names = [cd.name for cd in desc.chips]
    want = [s for s in a.chips.split(",") if s]
    if not want or any(w not in names for w in want):
        raise SystemExit("--join needs --chips with names out of " + ",".join(names))
    shards = [int(x) for x in a.shards.split(",")] if a.shards else [a.shard]
    supply = [names.index(x) for x in a.supply.split(",") if x]
    windows = []
    for sh in shards:
        present = p.job_shard_chips(job, sh)
        for w in want:
            if present >> names.index(w) & 1:
                windows.append((sh, names.index(w), 0, a.rows_per_chip))
    t0 = time.perf_counter()
    r = p.hunt_join_job(pk, job, windows, deltas, supply_chips=supply, seed=a.seed, max_evals=a.max_evals, cap_records=a.cap_records,
                        cap_absorbed=a.cap_records, cap_cells=a.cap_records)
    dt = time.perf_counter() - t0
    sm = r["summary"]
    print(f"== join over {len(windows)} windows ({','.join(want)} on shards {shards}), supply {a.supply or '-'}: {dt:.3f} s")
    print("   " + ", ".join(f"{k} {v}" for k, v in sm.items()))
    if sm["truncated"]:
        cut = [w for bit, w in ((1, "open records"), (2, "absorbed cells"), (4, "records without a slot of the join table"), (8, "returned cells")) if sm["truncated"] & bit]
        print("   WARNING: the answer is cut (%s): raise --cap-records; every group shown is a subset of a true group" % ", ".join(cut))
    groups = []
    for g in r["groups"]:
        sides = [side_summary(s, desc) for s in g]
        groups.append(dict(cells=[len(s) for s in g], sides=sides))
        print("   group: " + "   x   ".join("; ".join(f"{k} ({d['count']}, row {d['first_row']})" for k, d in s.items()) for s in sides))
    absorbed = collections.OrderedDict()
    for c in r["absorbed"]:
        key = "%s.%s %s" % (names[c["chip"]], desc.chips[c["chip"]].main_names[c["col"]], signed(c["delta"]))
        d = absorbed.setdefault(key, dict(count=0, first_row=c["row"], first_shard=c["tag"]))
        d["count"] += 1
    for k, d in absorbed.items():
        print(f"   absorbed {k}: {d['count']} (row {d['first_row']})")
    guest = "".join(ch if ch.isalnum() else "_" for ch in (a.guest or os.path.basename(a.elf))).strip("_")
    path = a.json or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r10_hunt_join_%s.json" % guest)
    with open(path, "w") as f:
        json.dump(dict(guest=a.guest or a.elf, cycles=int(rep["cycles"]), shards=shards, chips=want, supply=a.supply, deltas=deltas, seed=a.seed,
                       rows_per_chip=a.rows_per_chip, seconds=round(dt, 4), summary=sm, groups=groups, absorbed=absorbed), f, indent=1)
        f.write("\n")
    print("   wrote", path)


def write_json(path, out):
    """the results so far (one file per chip when the path holds {chip})"""
    if not path:
        return
    for name, rec in out["chips"].items() if "{chip}" in path else [(None, None)]:
        with open(path.replace("{chip}", name) if name else path, "w") as f:
            json.dump(dict(out, chips={name: rec}) if name else out, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--guest")
    ap.add_argument("--elf")
    ap.add_argument("--stdin", action="append", default=[])
    ap.add_argument("--chips", default="")
    ap.add_argument("--rows", default="", help="FIRST:COUNT (default: all rows)")
    ap.add_argument("--deltas", default=",".join(str(d) for d in DELTAS))
    ap.add_argument("--shard", type=int, default=0)
    ap.add_argument("--no-pairs", action="store_true")
    ap.add_argument("--pair-modes", default="same_row,adjacent", help="which pair hunts to run")
    ap.add_argument("--max-evals", type=int, default=0)
    ap.add_argument("--cap", type=int, default=1 << 16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json")
    ap.add_argument("--join", action="store_true", help="the join hunt over the chips of --chips")
    ap.add_argument("--supply", default="program,byte,mem_image", help="--join: the supply tables ('' for none)")
    ap.add_argument("--rows-per-chip", type=int, default=0, help="--join: the first N rows of every table (default: all rows)")
    ap.add_argument("--shards", default="", help="--join: the shards whose tables are hunted (default: --shard)")
    ap.add_argument("--log-shard", type=int, default=0, help="cycles per shard = 2^N (default: the prover's), e.g. to make a small guest two shards")
    ap.add_argument("--cap-records", type=int, default=1 << 21, help="--join: open records, absorbed cells and returned cells kept, each")
    a = ap.parse_args()
    from dvt_circuits_amd import capi
    from tools.airgen import rv32 as airdef

    if bool(a.guest) == bool(a.elf):
        ap.error("one of --guest and --elf")
    elf = guest_elf(a.guest) if a.guest else open(a.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in a.stdin]
    deltas = [int(x, 0) % P for x in a.deltas.split(",")]
    desc = airdef.build()
    p = capi.Prover('{"log_shard_size": %d}' % a.log_shard) if a.log_shard else capi.Prover()
    pk, _ = p.setup(elf)
    job, rep = p.prepare(pk, stdin)
    if a.join:
        run_join(a, p, capi, desc, pk, job, rep, deltas)
        p.job_free(job)
        p.pk_free(pk)
        p.close()
        return
    present = p.job_shard_chips(job, a.shard)
    want = [s for s in a.chips.split(",") if s]
    out = dict(guest=a.guest or a.elf, cycles=int(rep["cycles"]), shard=a.shard, deltas=deltas, seed=a.seed, chips={})
    for cid, cd in enumerate(desc.chips):
        if not present >> cid & 1 or (want and cd.name not in want):
            continue
        main_w, log_n = p.job_shard_chip_shape(job, a.shard, cid)
        n = 1 << log_n
        first, count = (int(x) for x in a.rows.split(":")) if a.rows else (0, n)
        names = cd.main_names
        rec = dict(main_w=main_w, log_n=log_n, row_first=first, row_count=count, runs={})
        out["chips"][cd.name] = rec
        print(f"== {cd.name}: {main_w} columns, 2^{log_n} rows, window {first}+{count}")

        def run(what, evals_of, **kw):
            t0 = time.perf_counter()
            try:
                r = p.hunt_shard(pk, job, a.shard, cid, deltas, row_first=first, row_count=count, seed=a.seed, max_evals=a.max_evals, **kw)
            except capi.DvtError as e:
                if e.code != capi.DVT_ERR_INPUT or "max_evals" not in e.msg:
                    raise
                rec["runs"][what] = dict(skipped=e.msg)
                print(f"   {what}: skipped ({e.msg})")
                return None
            dt = time.perf_counter() - t0
            evals = evals_of(r)
            rec["runs"][what] = dict(seconds=round(dt, 4), evaluations=evals, evaluations_per_second=round(evals / dt))
            print(f"   {what}: {dt:.3f} s, {evals} evaluations, {evals / dt:.3g} per second", flush=True)
            return r

        r = run("cells", lambda r: len(deltas) * main_w * count * min(2, n), want_map=False)
        counts = r[0]
        rec["free"] = {names[c]: [int(x) for x in counts[c]] for c in range(main_w) if counts[c].any()}
        for nm, v in rec["free"].items():
            print(f"   free {nm}: {v} of {count} rows per delta")
        for what, adjacent in () if a.no_pairs else [(w, w == "adjacent") for w in ("same_row", "adjacent") if w in a.pair_modes.split(",")]:
            r = run(what, lambda r: r["n_tried"] * min(3 if adjacent else 2, n), pairs=True, adjacent=adjacent, cap=a.cap)
            if r is None:
                continue
            g = groups_of(r["reported"], names)
            rec[what] = dict(n_tried=r["n_tried"], n_reported=r["n_reported"], returned=len(r["reported"]), groups=g)
            print(f"   {what}: tried {r['n_tried']}, reported {r['n_reported']}")
            for key, d in g.items():
                print(f"      {key}: {d['count']} (deltas {d['deltas'][:6]}, first row {d['first_row']})")
            write_json(a.json, out)   # (a long hunt that is interrupted keeps what is done)
    write_json(a.json, out)
    p.job_free(job)
    p.pk_free(pk)
    p.close()


if __name__ == "__main__":
    main()
