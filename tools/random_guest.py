#!/usr/bin/env python3
"""A seeded random RV32IM guest (tests/guests_random.py) on the host: its ELF, the model's cycle count, and what it covers.

    python tools/random_guest.py SEED [PROFILE] [N] [-o guest.elf] [--log-shard L] [--first-diff] [--stdin-words K [--stdin-seed S]]

PROFILE is one of mixed, alu, mem, muldiv, flow (default mixed), N the number of random steps (default 1500).  The counters are
those of tests/guests_random.coverage over the rows of the oracle's model (oracle/rv32_model.py): mnemonics retired in the
random part, the byte that decided each comparison, carry shapes, sub-word offsets, x0 as rd and rs1.  --first-diff runs the
product's executor and host trace expansion against the model, as tests/test_random_guests_cpu.py does, and prints the first
differing cell with its instruction.  --stdin-words K builds the guest with the input prologue (K input words copied into K
scratch slots before the random part) and runs it on the K words of tests/guests_random.input_of(S, K).  A host tool: nothing
here touches a GPU."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import rv32_model  # noqa: E402
from tests import guests_random as gr  # noqa: E402


def first_diff(guest, run, log_shard, stdin=()):
    """None, or the first difference between the product on the host and the model, as text"""
    from dvt_circuits_amd import capi

    case = (guest.seed, guest.profile, guest.n)
    stdin = list(stdin)
    rc, rep, pv, out, err = capi.execute_io(guest.elf, stdin)
    if rc != 0 or run.error:
        return "execution: the product says rc %d %r, the model %r" % (rc, err, run.error)
    for what, got, want in (("cycles", rep["cycles"], run.cycles), ("exit code", rep["exit_code"], run.exit_code),
                            ("public values", pv, run.public_values), ("stdout", out, run.stdout)):
        if got != want:
            return "%s: the product has %r, the model %r" % (what, got, want)
    for pos in range(len(run.shards)):
        host, hpubs, n = capi.rv32_debug_traces(guest.elf, stdin, log_shard, pos)
        model, mpubs = rv32_model.traces(run, pos)
        if n != len(run.shards) or [int(x) for x in hpubs] != [int(x) for x in mpubs]:
            return "shard %d: %d shards and public values %s, the model's %d and %s" % (pos, n, list(hpubs), len(run.shards), list(mpubs))
        if [(c["chip_id"], c["log_n"]) for c in host] != [(c["chip_id"], c["log_n"]) for c in model]:
            return "shard %d: chips and heights %s, the model's %s" % (pos, [(c["chip_id"], c["log_n"]) for c in host], [(c["chip_id"], c["log_n"]) for c in model])
        for h, m in zip(host, model):
            for part in ("main", "prep"):
                why = gr.first_difference(case, log_shard, run, pos, h, m, part, who="the host expansion")
                if why:
                    return why
    return None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("seed", type=int)
    ap.add_argument("profile", nargs="?", default="mixed", choices=gr.PROFILES)
    ap.add_argument("n", nargs="?", type=int, default=1500)
    ap.add_argument("-o", "--out", help="where the ELF goes (default random_SEED_PROFILE_N.elf)")
    ap.add_argument("--log-shard", type=int, default=21)
    ap.add_argument("--first-diff", action="store_true", help="compare the product's host path with the model")
    ap.add_argument("--stdin-words", type=int, default=0, metavar="K", help="the input prologue: K input words copied into K scratch slots")
    ap.add_argument("--stdin-seed", type=int, default=0, metavar="S", help="the seed of the K input words (default 0)")
    args = ap.parse_args(argv)
    # without the flag the call is the plain one: the default guest is made exactly as it always was
    if args.stdin_words:
        guest = gr.build(args.seed, args.n, args.profile, stdin_words=args.stdin_words)
        stdin = [gr.input_of(args.stdin_seed, args.stdin_words)]
    else:
        guest, stdin = gr.build(args.seed, args.n, args.profile), []
    path = args.out or "random_%d_%s_%d.elf" % (args.seed, args.profile, args.n)
    with open(path, "wb") as f:
        f.write(guest.elf)
    run = rv32_model.Run(guest.elf, stdin, args.log_shard)
    if run.error or not run.halted:
        print("the model stops: %s" % run.error)
        return 1
    first, end = gr.random_span(guest, run)
    print("%s: %d bytes, %d cycles in %d shards of 2^%d (random part: records %d..%d of the main run%s)" % (
        path, len(guest.elf), run.cycles, len(run.shards), args.log_shard, first, end - 1,
        ", %d functions behind the HALT" % (len(guest.random_pcs) - 1) if len(guest.random_pcs) > 1 else ""))
    cov = gr.coverage(guest, run)
    ops = sorted(((v, k[1]) for k, v in cov.items() if k[0] == "op"), reverse=True)
    print("mnemonics (%d rows): %s" % (sum(v for v, _ in ops), " ".join("%s=%d" % (m, v) for v, m in ops)))
    for kind in ("decided", "taken", "carry", "mul", "offset", "sign", "rd_x0", "rs1_x0"):
        print("%s: %s" % (kind, " ".join("%s=%d" % ("/".join(str(x) for x in k[1:]), v) for k, v in sorted(cov.items(), key=str) if k[0] == kind)))
    lacking = gr.missing(cov)
    print("of the %d conditions of the pinned list this guest alone misses %d" % (len(gr.required()), len(lacking)))
    if args.first_diff:
        why = first_diff(guest, run, args.log_shard, stdin)
        print("host against model: %s" % (why or "equal, cell by cell"))
        return 1 if why else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
