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
x touched rows exceed --max-evals is recorded as skipped."""
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
    a = ap.parse_args()
    from dvt_circuits_amd import capi
    from tools.airgen import rv32 as airdef

    if bool(a.guest) == bool(a.elf):
        ap.error("one of --guest and --elf")
    elf = guest_elf(a.guest) if a.guest else open(a.elf, "rb").read()
    stdin = [open(f, "rb").read() for f in a.stdin]
    deltas = [int(x, 0) % P for x in a.deltas.split(",")]
    desc = airdef.build()
    p = capi.Prover()
    pk, _ = p.setup(elf)
    job, rep = p.prepare(pk, stdin)
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
