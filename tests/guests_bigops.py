"""A guest that performs a given list of field / curve / UINT256_MUL precompile calls, each on data words of its own
(tests/_bigop_corpus.py supplies the lists: operands at the extremes of what the chips accept)."""
from tests.guests import _finish, _syscall
from tools.rvasm import Asm

ALIAS = "alias"


def precompile_calls(cases):
    """cases: list of (syscall code, a-words, b-words | None | "alias").  Call i runs with a0 = the address of its own copy
    of the a-words and a1 = the address of its own b-words, 0 (None: DOUBLE) or a0 again ("alias": x op x through one
    pointer).  The first operands lie back to back in one area, in call order, and the results stay where the precompile
    writes them; the epilogue WRITEs that area to fd 1 and commits the 32-bit sum of its words (guests.checksum).  A call
    costs five to seven cycles, so a hundred-odd calls span several shards at log_shard_size = 8.
    Returns (elf, offsets): offsets[i] is the word offset of call i's result in the bytes written to fd 1."""
    a = Asm()
    area, offsets = [], []
    for _, aw, _ in cases:
        offsets.append(len(area))
        area += list(aw)
    out = a.dword("res", area + [0] * 4)
    for n_, (code, aw, bw) in enumerate(cases):
        ap = out + 4 * offsets[n_]
        bp = 0 if bw is None else ap if isinstance(bw, str) and bw == ALIAS else a.dword(f"b{n_}", list(bw))
        _syscall(a, code, ap, bp)
    _finish(a, out, 4 * len(area))
    return a.elf(), offsets
