#!/usr/bin/env python3
"""Writes the guest ELFs the host CLI looks up in $DVT_ELF_DIR (the reference embeds its guests at build time, reference
build.rs:56-73 / src/main.rs:115-118): `bad-share.elf` = the re-stated bad-share guest of tests/guests_share.py,
`finalization.elf` = the re-stated finalization guest of tests/guests_finalization.py.  NMAX / KMAX size both guests'
tables (base hashes or generations / base pubkeys).

    python tools/build_guests.py OUT_DIR [NMAX KMAX]"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    from tests import guests_finalization, guests_share

    out = sys.argv[1]
    nmax, kmax = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (8, 8)
    os.makedirs(out, exist_ok=True)
    for name, build in (("bad-share", guests_share.bad_share), ("finalization", guests_finalization.finalization)):
        with open(os.path.join(out, name + ".elf"), "wb") as f:
            f.write(build(nmax=nmax, kmax=kmax))
        print("wrote", os.path.join(out, name + ".elf"))


if __name__ == "__main__":
    main()
