"""TEST TOOLING: the reference's finalization check restated in Python over tools/bls12_381.py — what the guest
`finalization_prove` runs inside the zkVM (reference crates/finalization_prove/src/main.rs:8-32 ->
crates/dkg/src/verification.rs:211-331, crates/dkg/src/dkg_math.rs:160-248).  Used to certify that
tools/gen_dkg_input.py emits inputs a DKG-verifying guest accepts, and pinned by the reference's own real vectors
(tests/golden/finalization_example.json = examples/finalization_test.json, finalization_no_auth_report1.json =
test_vectors/no_auth/finalization/report-1.json, which the reference's harness expects to exit 0).

verify_finalization(doc) returns None when the input is accepted, else the reason (the reference's error text class).
verify_share(doc) restates the bad-share guest (reference crates/bad_share_exchange_prove/src/main.rs) and returns
(exit_code, public_value_bytes), pinned by the reference's 10 no-auth share vectors (tests/golden/share_vectors/)."""
import hashlib
import struct

from tools import bls12_381 as B


def commitment_hash(gen_id: bytes, n: int, k: int, base_pubkeys) -> bytes:
    """reference crates/dkg/src/verification.rs:151-175: SHA-256(gen_id || n || k || len(base_pubkeys) as u8 || pubkeys...)"""
    return hashlib.sha256(gen_id + bytes([n, k, len(base_pubkeys) & 0xFF]) + b"".join(base_pubkeys)).digest()


def evaluate_polynomial(cfs, x: int):
    """Horner over G1 points (dkg_math.rs:160-174)"""
    if not cfs:
        return None
    y = cfs[-1]
    for c in reversed(cfs[:-1]):
        y = B.E1.add(B.E1.mul(y, x), c)
    return y


def lagrange_interpolation(ys, xs):
    """value at 0 of the interpolating polynomial (dkg_math.rs:178-227); raises ValueError as the reference returns Err"""
    k = len(xs)
    if k == 0 or k != len(ys):
        raise ValueError("invalid inputs")
    if k == 1:
        return ys[0]
    a = 1
    for x in xs:
        a = a * x % B.R
    if a == 0:
        raise ValueError("zero secret share id")
    r = None
    for i in range(k):
        b = xs[i]
        for j in range(k):
            if j != i:
                v = (xs[j] - xs[i]) % B.R
                if v == 0:
                    raise ValueError("duplicate secret share id")
                b = b * v % B.R
        li0 = a * pow(b, B.R - 2, B.R) % B.R
        r = B.E1.add(r, B.E1.mul(ys[i], li0))
    return r


def agg_coefficients(vectors, ids):
    """dkg_math.rs:230-248: sum the verification vectors coefficient-wise, evaluate the sum polynomial at every id"""
    final = []
    for i in range(len(vectors[0])):
        s = None
        for v in vectors:
            s = B.E1.add(s, v[i])
        final.append(s)
    return [evaluate_polynomial(final, x) for x in ids]


def verify_finalization(doc, check_signatures=True):
    B.ensure_ready()
    st = doc["settings"]
    n, k, gen_id = st["n"], st["k"], bytes.fromhex(st["gen_id"])
    gens = doc["generations"]
    if len(gens) != n:
        return "Invalid number of generations"
    if any(g["message_cleartext"] != gens[0]["message_cleartext"] for g in gens):
        return "Invalid message cleartext"
    hm = B.hash_to_g2(gens[0]["message_cleartext"].encode())          # one hash-to-G2 for all (verification.rs:233-235)
    for g in gens:
        try:
            sig = B.g2_decompress(bytes.fromhex(g["message_signature"]))
            key = B.g1_decompress(bytes.fromhex(g["partial_pubkey"]))
        except ValueError as e:
            return f"Invalid point: {e}"
        if check_signatures and not B.pairing_product_is_one([(key, hm), (B.E1.neg(B.G1), sig)]):
            return "Invalid signature " + g["message_signature"]
        pks = [bytes.fromhex(p) for p in g["base_pubkeys"]]
        if commitment_hash(gen_id, n, k, pks).hex() != g["base_hash"]:
            return "Invalid initial commitment hash " + g["base_hash"]
    ordered = sorted(gens, key=lambda g: bytes.fromhex(g["base_hash"]))
    try:
        vectors = [[B.g1_decompress(bytes.fromhex(p)) for p in g["base_pubkeys"]] for g in ordered]
        partial = [B.g1_decompress(bytes.fromhex(g["partial_pubkey"])) for g in ordered]
        agg = B.g1_decompress(bytes.fromhex(doc["aggregate_pubkey"]))
    except ValueError as e:
        return f"Invalid point: {e}"
    ids = list(range(1, n + 1))
    try:
        computed = lagrange_interpolation(agg_coefficients(vectors, ids), ids)
        if B.g1_compress(computed) != B.g1_compress(agg):
            return "Computed key does not match aggregate public key (verification vectors)"
        computed = lagrange_interpolation(partial, ids)
        if B.g1_compress(computed) != B.g1_compress(agg):
            return "Computed key does not match aggregate public key (partial keys)"
    except ValueError as e:
        return str(e)
    return None


def share_public_values(doc) -> bytes:
    """what the reference commits on a slashable share (main.rs:57-70): every base hash in input order, then the perpetrator's
    secp256k1 key, each the way `sp1_zkvm::io::commit` serialises a raw type: u64-LE length || lowercase hex"""
    out = b""
    for h in doc["base_hashes"]:
        out += struct.pack("<Q", 64) + h.lower().encode()
    pk = doc["seeds_exchange_commitment"]["commitment"]["pubkey"].lower()
    return out + struct.pack("<Q", len(pk)) + pk.encode()


def verify_share(doc):
    """-> (exit_code, public_value_bytes): 0 and the committed bytes when the share is provably bad (slashable), else 1 and b""
    (the reference panics: a failed sanity check, a bad base pubkey, or a valid share).  No auth_commitment checks."""
    ic = doc["initial_commitment"]
    st = ic["settings"]
    n, k = st["n"], st["k"]
    hashes = [bytes.fromhex(h) for h in doc["base_hashes"]]
    pks = [bytes.fromhex(p) for p in ic["base_pubkeys"]]
    # sanity panics (main.rs:24-43)
    if len(hashes) != n or n < k:
        return 1, b""
    if bytes.fromhex(ic["hash"]) not in hashes:
        return 1, b""
    if commitment_hash(bytes.fromhex(st["gen_id"]), n, k, pks) != bytes.fromhex(ic["hash"]):
        return 1, b""
    # verify_seed_exchange_commitment, no-auth branch (verification.rs:91-148)
    ss = doc["seeds_exchange_commitment"]["ssecret"]
    slashable = 0, share_public_values(doc)                              # main.rs:57-70: commit, return normally
    sk = int.from_bytes(bytes.fromhex(ss["shared_secret"]), "big")       # big-endian scalar (bls_keys.rs:98-114)
    if sk >= B.R:
        return slashable
    dst = bytes.fromhex(ss["dst_base_hash"])
    ordered = sorted(hashes)                                              # get_index_in_commitments (verification.rs:50-66)
    if dst not in ordered:
        return slashable
    dest_id = ordered.index(dst) + 1
    try:
        cfs = [B.g1_decompress(p) for p in pks]                           # `.expect("Invalid pubkey")`: a panic
    except ValueError:
        return 1, b""
    if B.g1_compress(B.E1.mul(B.G1, sk)) != B.g1_compress(evaluate_polynomial(cfs, dest_id)):
        return slashable
    return 1, b""                                                         # "The seed exchange commitment is valid" (main.rs:81)
