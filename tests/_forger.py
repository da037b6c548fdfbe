"""TEST INFRASTRUCTURE: a dishonest prover.  A Forgery is handed to tests/_oracle_prover.prove_shard as `cheat`; each of
its cheats deviates from the protocol at ONE place, and every later step of the prover runs honestly on the altered data.
The transcript and every Merkle tree of the forged proof are therefore consistent: the input-tree openings always pass,
and only the check a cheat aims at can fail.

The cheats (tuples made by the functions of the same name; `delta` is added to a base-field word, or to coefficient 0 of
an extension value):

  lde_point(tree, chip, col, k, delta)  word [col][k] of the chip's LDE in the "main", "perm" or "quot" tree, in the copy
                                        that is COMMITTED and opened by the queries.  Quotient and values at zeta come
                                        from the true matrices, so the zeta check passes; the reduced opening (FRI's
                                        input) comes from the committed one
  next_opening(chip, col, delta)        the claimed main_n[col] of a column no constraint reads at the next row
  opened_value(chip, col, delta)        the claimed main_l[col] of a constrained column
  cumsum(chip, delta)                   the chip's claimed cumulative sum
  layer_value(layer, k, delta)          value k of FRI layer `layer` (its position in fri_roots; negative counts from the
                                        end: -1 is the layer of 4 values, lm = 2) before that layer is committed
  final_poly(delta)                     the final value that is observed, ground and written
  witness(second=, bump=)               the second-smallest valid proof-of-work witness / the first invalid value above
                                        the smallest valid one

When the last fold leaves two different values (every low-degree-breaking cheat does), final_poly is last[final]; the
Forgery's `final` says which.  The honest-looking choice is the position the alteration did not reach.

predict() replays the order of the verifier (host part: cumulative sums, zeta, proof of work; then query by query, layer by
layer, then the final value) over what the forger itself computed and committed.  It needs no field arithmetic and never
calls the verifier: while the verifier's running value equals the forger's pre-alteration value of a layer, the pair it
hashes is the committed one unless that very value was altered before the commit, and its fold of a committed pair is the
forger's honest fold of it.

CASES holds the (cheat, delta, q) constants of the forged-proof tests (tests/test_verifier_forgeries.py on the host,
tests/test_gpu_verify_forgeries.py on the device).  Each delta was found once by search_delta (at most SEARCH_TRIES
values); the tests assert the pattern of every case, so a stale constant fails instead of testing nothing."""
import copy

import numpy as np

from tests import _oracle_prover, toy_traces

P = _oracle_prover.P
LAYER, FINAL = "Merkle opening rejected (FRI layer)", "FRI final value mismatch"
CUMSUM, POW_REASON, ZETA = "LogUp cumulative sums do not cancel", "proof-of-work witness rejected", "constraint check failed at zeta for chip "
SEARCH_TRIES = 32


def lde_point(tree, chip, col, k, delta):
    assert tree in ("main", "perm", "quot")
    return ("lde_point", tree, chip, col, k, delta)


def next_opening(chip, col, delta):
    return ("next_opening", chip, col, delta)


def opened_value(chip, col, delta):
    return ("opened_value", chip, col, delta)


def cumsum(chip, delta):
    return ("cumsum", chip, delta)


def layer_value(layer, k, delta):
    return ("layer_value", layer, k, delta)


def final_poly(delta):
    return ("final_poly", delta)


def witness(second=False, bump=False):
    assert second != bump
    return ("witness", "second" if second else "bump")


class Forgery:
    """the cheats of ONE proof (pass a fresh one to every prove_shard call), and afterwards the forger's record of it"""

    def __init__(self, *cheats, final=0):
        self.cheats, self.final_pick = list(cheats), final
        self.forged = {}                  # (tree, chip id) -> the committed LDE
        self.pre, self.committed_layers = [], []
        self.zeta_chip = self.last = self.final_poly = self.idx = self.cumsums_claimed = None
        self.witness_valid = True

    def _of(self, kind):
        return [c for c in self.cheats if c[0] == kind]

    # ---- the hooks of prove_shard, in the order it calls them
    def committed(self, tree, tree_cs, cs):
        out = []
        for c in tree_cs:
            m = c[tree + "_lde"]
            for _, t, chip, col, k, delta in self._of("lde_point"):
                if t == tree and chip == c["id"]:
                    if m is c[tree + "_lde"]:
                        m = m.copy()
                    m[col, k] = (int(m[col, k]) + delta) % P
            if m is not c[tree + "_lde"]:
                self.forged[(tree, c["id"])] = m
            out.append(m)
        return out

    def cumsums(self, cs):
        for _, chip, delta in self._of("cumsum"):
            c = next(c for c in cs if c["id"] == chip)
            c["cumsum"] = [(c["cumsum"][0] + delta) % P] + list(c["cumsum"][1:])

    def openings(self, cs):
        for kind, key in (("next_opening", "main_n"), ("opened_value", "main_l")):
            for _, chip, col, delta in self._of(kind):
                c = next(c for c in cs if c["id"] == chip)
                v = c["open"][key][col]
                c["open"][key][col] = [(v[0] + delta) % P] + list(v[1:])
        for c in cs:
            for tree in ("main", "perm", "quot"):
                if (tree, c["id"]) in self.forged:
                    c[tree + "_lde"] = self.forged[(tree, c["id"])]

    def layer(self, k, cur):
        self.pre.append(cur)
        n_layers = int(cur.shape[0]).bit_length() - 2 + k     # (layer k has 2^(hmax - k) values, the last one 4)
        for _, layer, at, delta in self._of("layer_value"):
            if layer % n_layers == k:
                if cur is self.pre[-1]:
                    cur = cur.copy()
                cur[at, 0] = (int(cur[at, 0]) + delta) % P
        self.committed_layers.append(cur)
        return cur

    def final(self, last):
        assert last.shape[0] == 2
        self.last = last
        fp = last[self.final_pick].tolist()
        for _, delta in self._of("final_poly"):
            fp[0] = (fp[0] + delta) % P
        self.final_poly = fp
        return fp

    def witness(self, ch, w, pow_bits):
        def valid(x):
            c = copy.copy(ch)
            c.state, c.inp, c.out = list(ch.state), list(ch.inp), list(ch.out)
            c.observe([x])
            return c.sample_bits(pow_bits) == 0

        assert valid(w)
        for _, how in self._of("witness"):
            w += 1
            while valid(w) != (how == "second"):
                w += 1
            self.witness_valid = how == "second"
        return w

    def done(self, air, cs, idx):
        self.idx = list(idx)
        self.cumsums_claimed = [list(c["cumsum"]) for c in cs]
        ids = [c["id"] for c in cs]
        hit = sorted(ids.index(chip) for _, chip, _, _ in self._of("opened_value"))
        self.zeta_chip = air.chip(ids[hit[0]]).name.decode() if hit else None

    # ---- the prediction
    def query(self, idx):
        """what the verifier's query part says of a query at idx: None, LAYER or FINAL"""
        for pre, com in zip(self.pre, self.committed_layers):
            j = idx & (pre.shape[0] - 1)
            # the verifier's running value is pre[j]: the first layer's from the rows it opened, a later one's as its fold
            # of the previous committed pair plus the reduced opening of that height
            if (pre[j] != com[j]).any():
                return LAYER
        return FINAL if self.last[idx & 1].tolist() != self.final_poly else None

    def outcomes(self):
        return [self.query(i) for i in self.idx]

    def predict(self, single_shard=True):
        """(accepted, reason).  single_shard: the proof stands alone, so its cumulative sums must cancel by themselves."""
        if single_shard and any(sum(c[k] for c in self.cumsums_claimed) % P for k in range(4)):
            return False, CUMSUM
        if self.zeta_chip is not None:
            return False, ZETA + self.zeta_chip
        if not self.witness_valid:
            return False, POW_REASON
        for why in self.outcomes():
            if why:
                return False, why
        return True, ""


# ---------------------------------------------------------------- the toy machine
def toy_chips(shape):
    prep, main, pubs = toy_traces.build(*shape)
    chips = [dict(chip_id=cid, main=m, prep=(prep[0][1] if cid == toy_traces.RANGE8 else np.zeros((0, m.shape[1]), np.uint32))) for cid, m in main]
    return chips, pubs


def toy_vk(prep_root):
    """the verifying key of the toy machine as csrc/capi.hip vk_words writes it: "DVK1", the machine name padded to 16
    bytes, the preprocessed root, the preprocessed chips [(range8 = 0, log_n = 8)], no extra words"""
    name = np.frombuffer(b"toy".ljust(16, b"\0"), np.uint32).tolist()
    return np.array([0x314B5644] + name + [int(x) for x in prep_root] + [1, toy_traces.RANGE8, 8, 0], np.uint32).tobytes()


def forge_toy(shape, cheats, q, pow_bits, final=0):
    """(proof bytes, prep root, the Forgery) of a toy-machine proof made with these cheats"""
    chips, pubs = toy_chips(shape)
    f = Forgery(*cheats, final=final)
    proof, prep_root = _oracle_prover.prove_shard("toy", chips, pubs, q, pow_bits, cheat=f)
    return proof, prep_root, f


def search_delta(c, tries=SEARCH_TRIES):
    """the first delta in 1..tries for which the forged proof of case c shows its pattern, or None.  Every delta changes
    the transcript, so every try draws fresh query indices.  (`python -m tests._forger` prints the table.)"""
    for delta in range(1, tries + 1):
        if PATTERNS[c["pattern"]](forge_case(c, delta)[2]):
            return delta
    return None


# ---- the patterns of the required coverage: predicates over the forger's per-query outcomes
def first_failure(f):
    o = f.outcomes()
    return next(((i, w) for i, w in enumerate(o) if w), (None, None))


PATTERNS = {
    # (a) "final value" where query 0 already fails
    "final_at_0": lambda f: first_failure(f) == (0, FINAL),
    # (b) "final value" where queries 0..j-1 pass and query j >= 2 fails
    "final_at_j": lambda f: first_failure(f)[1] == FINAL and first_failure(f)[0] >= 2,
    # (b) the same with j the last query
    "final_at_last": lambda f: first_failure(f) == (len(f.idx) - 1, FINAL) and len(f.idx) >= 3,
    # (c) a forged proof that no query catches
    "accepted": lambda f: not any(f.outcomes()),
    # (d) "FRI layer" is the reported reason
    "layer": lambda f: first_failure(f)[1] == LAYER,
    # (e) the lowest failing query fails on the final value, a later one on a layer
    "final_then_layer": lambda f: first_failure(f)[1] == FINAL and LAYER in f.outcomes(),
    # (f) the converse
    "layer_then_final": lambda f: first_failure(f)[1] == LAYER and FINAL in f.outcomes(),
    # (g), (h) reaches the final value
    "final": lambda f: first_failure(f)[1] == FINAL,
    # host-part reasons and plain acceptance are not patterns of the query outcomes
    None: lambda f: True,
}

Q, POW = 6, 5
BIG, SMALL = (6, 4, 11), (3, 0, 1)     # toy_traces.build shapes: range8 2^8 rows; fib 2^6, pairs 2^4 / fib 2^3, pairs one row
R8, FIB, PAIRS = toy_traces.RANGE8, toy_traces.FIB, toy_traces.PAIRS


def case(name, shape, q, cheats, final, pattern):
    """cheats: a function of delta -> list of cheats (the searched constant goes where the case wants it)"""
    return dict(name=name, shape=shape, q=q, cheats=cheats, final=final, pattern=pattern)


# Where a cheat's delta is searched, `d` is the searched value; DELTAS holds what the search found.  The alteration of an
# lde_point at k reaches last[k & 1], that of a layer_value at k' reaches last[k' & 1]: `final` names the other position
# unless stated.
CASES = [
    # (a) tallest chip, quot tree: k = 5 reaches last[1]; final_poly = last[0]
    case("a_quot_tall", BIG, Q, lambda d: [lde_point("quot", R8, 2, 5, d)], 0, "final_at_0"),
    # (b) the first failing query is query j >= 2 / is the last query
    case("b_quot_tall_late", BIG, Q, lambda d: [lde_point("quot", R8, 7, 300, d)], 1, "final_at_j"),
    case("b_perm_tall_last", BIG, 3, lambda d: [lde_point("perm", R8, 1, 77, d)], 0, "final_at_last"),
    # (c) q = 2: both queries miss the parity of k
    case("c_accepted", BIG, 2, lambda d: [lde_point("quot", R8, 0, 9, d)], 0, "accepted"),
    # (d) late layers: layer -2 has 8 values (lm = 3), one query in 8 opens value 6; layer -1 has 4 (lm = 2)
    case("d_layer_lm3", BIG, Q, lambda d: [layer_value(-2, 6, d)], 1, "layer"),
    # the first layer has 512 values: no query opens value 130, the queries of its parity fail on the final value
    case("layer_first_final", BIG, Q, lambda d: [layer_value(0, 130, d)], 1, "final"),
    case("d_layer_lm2", SMALL, Q, lambda d: [layer_value(-1, 3, d)], 0, "layer"),
    # (e) / (f) two cheats in one proof: an LDE point reaching last[1] and a layer value of even position
    case("e_final_then_layer", BIG, Q, lambda d: [lde_point("quot", R8, 3, 11, d), layer_value(-2, 2, 1)], 0, "final_then_layer"),
    case("f_layer_then_final", BIG, Q, lambda d: [lde_point("perm", R8, 0, 21, d), layer_value(-1, 2, 1)], 0, "layer_then_final"),
    # layer_value at two layers
    case("two_layers", BIG, Q, lambda d: [layer_value(2, 33, d), layer_value(-1, 1, 7)], 0, "layer"),
    # (g) pairs.x and range8.mult are read at the next row by no constraint
    case("g_next_pairs_x", BIG, Q, lambda d: [next_opening(PAIRS, 0, d)], 0, "final"),
    case("g_next_range_mult", SMALL, Q, lambda d: [next_opening(R8, 0, d)], 1, "final"),
    # (h) chips shorter than hmax - 1: their reduced opening joins the chain at a later layer
    case("h_quot_fib", BIG, Q, lambda d: [lde_point("quot", FIB, 4, 17, d)], 0, "final"),
    case("h_perm_pairs", BIG, Q, lambda d: [lde_point("perm", PAIRS, 2, 6, d)], 1, "final"),
    case("h_quot_one_row", SMALL, Q, lambda d: [lde_point("quot", PAIRS, 1, 1, d)], 0, "final"),
    case("h_main_fib", SMALL, Q, lambda d: [lde_point("main", FIB, 3, 4, d)], 1, "final"),
    # the final value alone, everything else honest
    case("final_poly", BIG, Q, lambda d: [final_poly(d)], 0, "final_at_0"),
    case("final_poly_small", SMALL, Q, lambda d: [final_poly(d)], 0, "final_at_0"),
    # host-part targets
    case("cumsum", BIG, Q, lambda d: [cumsum(FIB, d)], 0, None),
    case("opened_value", BIG, Q, lambda d: [opened_value(FIB, 0, d)], 0, None),
    case("witness_bump", BIG, Q, lambda d: [witness(bump=True)], 0, None),
    # ACCEPTED: a valid witness that is not the smallest
    case("witness_second", BIG, Q, lambda d: [witness(second=True)], 0, None),
]

# what search_delta found for each case
DELTAS = {
    "a_quot_tall": 1, "b_quot_tall_late": 1, "b_perm_tall_last": 8, "c_accepted": 3, "d_layer_lm3": 4, "layer_first_final": 1,
    "d_layer_lm2": 2, "e_final_then_layer": 2, "f_layer_then_final": 1, "two_layers": 2, "g_next_pairs_x": 1,
    "g_next_range_mult": 1, "h_quot_fib": 1, "h_perm_pairs": 1, "h_quot_one_row": 1, "h_main_fib": 1, "final_poly": 1,
    "final_poly_small": 1, "cumsum": 1, "opened_value": 1, "witness_bump": 1, "witness_second": 1,
}

# the host-part cases: the predicted reason ("" = accepted)
HOST_REASONS = {"cumsum": CUMSUM, "opened_value": ZETA + "fib", "witness_bump": POW_REASON, "witness_second": ""}


def forge_case(c, delta=None):
    d = DELTAS[c["name"]] if delta is None else delta
    return forge_toy(c["shape"], c["cheats"](d), c["q"], POW, final=c["final"])


if __name__ == "__main__":
    for _c in CASES:
        print('"%s": %s,' % (_c["name"], search_delta(_c)), flush=True)
