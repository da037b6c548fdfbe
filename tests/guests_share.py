"""The reference's bad-share guest (reference crates/bad_share_exchange_prove/src/main.rs) re-stated for the rv32 machine, on
the reference's REAL input format and with the reference's public-value bytes: the no-auth build of the guest.

What it does, step by step with the reference line it follows:
  * reads the one stdin buffer = u64-LE length || CBOR of `SharedData` (main.rs:20-22; crates/dkg/src/types.rs), walks the CBOR
    in the field order the host encoder emits: base_hashes[], initial_commitment {hash, settings {n, k, gen_id},
    base_pubkeys[]}, seeds_exchange_commitment {initial_commitment_hash, ssecret {dst_base_hash, shared_secret},
    commitment {pubkey}} (every byte array is a lowercase-hex text string, types.rs:322-330);
  * the sanity panics (main.rs:24-43): the number of base hashes is n; n >= k; initial_commitment.hash is one of the base
    hashes; it equals SHA-256(gen_id || n || k || len || base_pubkeys) (`verify_initial_commitment_hash`,
    crates/dkg/src/verification.rs:151-183);
  * `verify_seed_exchange_commitment`, the no-auth branch (verification.rs:91-148): the shared secret is a big-endian scalar
    (crates/dkg/src/crypto/bls_keys.rs:98-114) and a value >= r is slashable; the index of dst_base_hash among the byte-wise
    sorted base hashes (`get_index_in_commitments`, verification.rs:50-66: the number of hashes below it) gives the id =
    index + 1, and an absent hash is slashable; every base pubkey is decompressed with the subgroup check
    (G1Affine::from_compressed, a bad encoding panics: verification.rs:132-137, bls_common.rs:108-112); the Horner
    evaluation at id (`evaluate_polynomial`, crates/dkg/src/dkg_math.rs:160-174; no coefficients give the identity) must
    compress to the same bytes as [sk] G, else the share is slashable;
  * on a slashable error (main.rs:57-70) commits every base hash in INPUT order, then the perpetrator's 33-byte secp256k1
    key, the way `sp1_zkvm::io::commit` serialises a raw type: u64-LE length || lowercase hex; the proof binds the SHA-256
    of these bytes (eight COMMIT words) and the guest halts with 0.
NOT done: the `auth_commitment` build's checks (the ECDSA signature of the commitment, verification.rs:76-89, and
`compute_seed_exchange_hash`, :30-48, :106-119).
A valid share ends the guest with exit code 1 (main.rs:81: "The seed exchange commitment is valid"), as does every panic and
an input beyond the guest's nmax / kmax tables; `prove` reports that as DVT_ERR_GUEST.
The CBOR / hex routines are those of the finalization guest (tests/guests_finalization.py)."""
import struct

from tests.guests import SHA_H0, emit_sha256, _bswap
from tests.guests_bls import BLS_R, G1Lib, POINT_WORDS, words_of
from tools.rvasm import SYS_COMMIT, SYS_HINT_LEN, SYS_HINT_READ, SYS_WRITE, Asm

HEAP = 0x00400000
G1_X = 0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB
G1_Y = 0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1
SECP_PK = 33


def _be_words(v, nbytes):
    """the big-endian byte string of v as little-endian memory words (what hex_decode leaves in memory)"""
    return [w for (w,) in struct.iter_unpack("<I", v.to_bytes(nbytes, "big"))]


def emit_cbor_hex(a):
    """cbor_head, cbor_text, hex_decode, hex_encode, bytes_cmp: the finalization guest's routines"""
    # ---- cbor_head(a0 = ptr) -> a0 = ptr behind the head, a1 = major type, a2 = argument (lengths up to 32 bits)
    a.label("cbor_head")
    a.lbu("t1", "a0", 0)
    a.addi("a0", "a0", 1)
    a.srli("a1", "t1", 5)
    a.andi("a2", "t1", 31)
    a.sltiu("t2", "a2", 24)
    a.bne("t2", "zero", "cbor_head_r")
    a.addi("t2", "a2", -24)                 # 0 -> 1 byte, 1 -> 2, 2 -> 4 follow (big-endian)
    a.li("t3", 1)
    a.sll("t3", "t3", "t2")
    a.sltiu("t4", "t2", 3)
    a.bne("t4", "zero", "cbor_head_l")
    a.halt(1)                               # 64-bit arguments / indefinite lengths do not occur
    a.label("cbor_head_l")
    a.li("a2", 0)
    a.label("cbor_head_b")
    a.lbu("t1", "a0", 0)
    a.addi("a0", "a0", 1)
    a.slli("a2", "a2", 8)
    a.or_("a2", "a2", "t1")
    a.addi("t3", "t3", -1)
    a.bne("t3", "zero", "cbor_head_b")
    a.label("cbor_head_r")
    a.ret()
    # ---- text(a0 = ptr, a3 = expected length or 0 = any) -> a0 = ptr behind, a4 = start of the bytes, a2 = length
    a.label("cbor_text")
    a.addi("sp", "sp", -4)
    a.sw("ra", "sp", 0)
    a.call("cbor_head")
    a.addi("t1", "a1", -3)
    a.beq("t1", "zero", "cbor_text_t")
    a.halt(1)
    a.label("cbor_text_t")
    a.beq("a3", "zero", "cbor_text_l")
    a.beq("a3", "a2", "cbor_text_l")
    a.halt(1)
    a.label("cbor_text_l")
    a.mv("a4", "a0")
    a.add("a0", "a0", "a2")
    a.lw("ra", "sp", 0)
    a.addi("sp", "sp", 4)
    a.ret()
    # ---- hex_decode(a0 = ASCII source, a1 = destination, a2 = bytes to produce); anything but 0-9a-f ends the guest
    a.label("hex_decode")
    a.label("hex_dec_l")
    a.li("t4", 0)
    for half in range(2):
        a.lbu("t1", "a0", half)
        a.addi("t2", "t1", -48)
        a.sltiu("t3", "t2", 10)
        a.bne("t3", "zero", f"hex_dec_d{half}")
        a.addi("t2", "t1", -97)
        a.sltiu("t3", "t2", 6)
        a.bne("t3", "zero", f"hex_dec_a{half}")
        a.halt(1)
        a.label(f"hex_dec_a{half}")
        a.addi("t2", "t2", 10)
        a.label(f"hex_dec_d{half}")
        a.slli("t4", "t4", 4)
        a.or_("t4", "t4", "t2")
    a.sb("t4", "a1", 0)
    a.addi("a0", "a0", 2)
    a.addi("a1", "a1", 1)
    a.addi("a2", "a2", -1)
    a.bne("a2", "zero", "hex_dec_l")
    a.ret()
    # ---- hex_encode(a0 = bytes, a1 = ASCII destination, a2 = number of bytes): lowercase
    a.label("hex_encode")
    a.label("hex_enc_l")
    a.lbu("t1", "a0", 0)
    for half, sh in ((0, 4), (1, 0)):
        if sh:
            a.srli("t2", "t1", sh)
        else:
            a.andi("t2", "t1", 15)
        a.sltiu("t3", "t2", 10)
        a.addi("t4", "t2", 87)              # 'a' - 10
        a.beq("t3", "zero", f"hex_enc_s{half}")
        a.addi("t4", "t2", 48)
        a.label(f"hex_enc_s{half}")
        a.sb("t4", "a1", half)
    a.addi("a0", "a0", 1)
    a.addi("a1", "a1", 2)
    a.addi("a2", "a2", -1)
    a.bne("a2", "zero", "hex_enc_l")
    a.ret()
    # ---- bytes_cmp(a0, a1, a2 = n) -> a0 = 0 equal / 1 first greater / 2 first smaller (bytewise: RawBytes' Ord, types.rs:310-320)
    a.label("bytes_cmp")
    a.label("bytes_cmp_l")
    a.lbu("t1", "a0", 0)
    a.lbu("t2", "a1", 0)
    a.bltu("t2", "t1", "bytes_cmp_g")
    a.bltu("t1", "t2", "bytes_cmp_s")
    a.addi("a0", "a0", 1)
    a.addi("a1", "a1", 1)
    a.addi("a2", "a2", -1)
    a.bne("a2", "zero", "bytes_cmp_l")
    a.li("a0", 0)
    a.ret()
    a.label("bytes_cmp_g")
    a.li("a0", 1)
    a.ret()
    a.label("bytes_cmp_s")
    a.li("a0", 2)
    a.ret()


def bad_share(nmax=8, kmax=8, subgroup_check=True):
    """-> ELF.  nmax / kmax: capacity of the guest's tables of base hashes / base pubkeys (it exits with code 1 on larger inputs).
    subgroup_check=False skips the [r] P = 0 test of the decompressed pubkeys (shorter runs for the Python-side checks)."""
    a = Asm()
    lib = G1Lib(a)
    V = a.dword("svars", [0] * 16)
    V_N, V_K, V_NH, V_NPK, V_I, V_J, V_P, V_END, V_ID, V_FOUND = (V + 4 * i for i in range(10))
    gen_id = a.dword("gen_id", [0] * 4)
    hashes = a.dword("hashes", [0] * (8 * nmax))
    ic_hash = a.dword("ic_hash", [0] * 8)
    pks = a.dword("pks", [0] * (12 * kmax))
    ich = a.dword("ich", [0] * 8)
    dst = a.dword("dst", [0] * 8)
    sk_be = a.dword("sk_be", [0] * 8)
    sk_le = a.dword("sk_le", [0] * 8)
    secp = a.dword("secp", [0] * ((SECP_PK + 3) // 4))
    r_be = a.dword("r_be", _be_words(BLS_R, 32))
    g1 = a.dword("g1", words_of(G1_X, 12) + words_of(G1_Y, 12) + [0])
    cfs = a.dword("cfs", [0] * (POINT_WORDS * kmax))
    hy = a.dword("hy", [0] * POINT_WORDS)
    htmp = a.dword("htmp", [0] * POINT_WORDS)
    skpt = a.dword("skpt", [0] * POINT_WORDS)
    cmp_a = a.dword("cmp_a", [0] * 12)
    cmp_b = a.dword("cmp_b", [0] * 12)
    state = a.dword("hstate", [0] * 8)
    h0 = a.dword("h0", SHA_H0)
    a.dword("align", [0] * ((-len(a.data)) % 16))
    msgbuf = a.dword("msgbuf", [0] * (16 * ((19 + 48 * kmax + 9 + 63) // 64)))
    a.dword("align2", [0] * ((-len(a.data)) % 16))
    pvbuf = a.dword("pvbuf", [0] * (16 * ((72 * nmax + 8 + 2 * SECP_PK + 9 + 63) // 64)))
    assert (pvbuf - a.data_base) % 64 == 0 and (msgbuf - a.data_base) % 64 == 0

    def lv(reg, addr):
        a.li(reg, addr)
        a.lw(reg, reg, 0)

    def sv(reg, addr, tmp="t6"):
        a.li(tmp, addr)
        a.sw(reg, tmp, 0)

    def fail_if_ne(r1, r2, uid):
        a.beq(r1, r2, f"ok_{uid}")
        a.halt(1)
        a.label(f"ok_{uid}")

    def slash_if_ne(r1, r2, uid):
        a.beq(r1, r2, f"ns_{uid}")
        a.j("slash")                        # (a plain branch does not reach that far)
        a.label(f"ns_{uid}")

    def text_hex(key_len, dst_addr, nbytes):
        """key text, then a text of 2 nbytes hex digits decoded to dst_addr; a0 = CBOR cursor before and after"""
        a.li("a3", key_len)
        a.call("cbor_text")
        a.li("a3", 2 * nbytes)
        a.call("cbor_text")
        sv("a0", V_P)
        a.mv("a0", "a4")
        a.li("a1", dst_addr)
        a.li("a2", nbytes)
        a.call("hex_decode")
        lv("a0", V_P)

    def hex_array(key_len, count_var, cap, uid, dst_addr, nbytes):
        """key text, then array(count <= cap) of hex texts decoded to dst_addr + nbytes i"""
        a.li("a3", key_len)
        a.call("cbor_text")
        a.call("cbor_head")
        a.addi("t1", "a1", -4)
        fail_if_ne("t1", "zero", f"arr_{uid}")
        sv("a2", count_var)
        a.sltiu("t2", "a2", cap + 1)
        a.li("t3", 1)
        fail_if_ne("t2", "t3", f"cap_{uid}")   # beyond the guest's tables
        sv("a0", V_P)
        a.li("t1", 0)
        sv("t1", V_I)
        a.label(f"{uid}_l")
        lv("t1", V_I)
        lv("t2", count_var)
        a.beq("t1", "t2", f"{uid}_done")
        lv("a0", V_P)
        a.li("a3", 2 * nbytes)
        a.call("cbor_text")
        sv("a0", V_P)
        a.mv("a0", "a4")
        lv("t1", V_I)
        a.li("t2", nbytes)
        a.mul("t1", "t1", "t2")
        a.li("a1", dst_addr)
        a.add("a1", "a1", "t1")
        a.li("a2", nbytes)
        a.call("hex_decode")
        lv("t1", V_I)
        a.addi("t1", "t1", 1)
        sv("t1", V_I)
        a.j(f"{uid}_l")
        a.label(f"{uid}_done")
        lv("a0", V_P)

    a.j("main")
    emit_sha256(a)
    lib.emit()
    emit_cbor_hex(a)
    # ---- sha_msg(a0 = 64-byte aligned buffer, a1 = message length in bytes): pads in place, hstate := SHA-256 state of it
    a.label("sha_msg")
    lib.push_ra()
    a.add("t1", "a0", "a1")
    a.li("t2", 0x80)
    a.sb("t2", "t1", 0)
    a.addi("t1", "t1", 1)
    a.label("sha_msg_z")                    # zero bytes until the address is 56 mod 64, then the 64-bit big-endian bit length
    a.andi("t2", "t1", 63)
    a.addi("t2", "t2", -56)
    a.beq("t2", "zero", "sha_msg_l")
    a.sb("zero", "t1", 0)
    a.addi("t1", "t1", 1)
    a.j("sha_msg_z")
    a.label("sha_msg_l")
    a.sw("zero", "t1", 0)
    a.slli("t3", "a1", 3)
    _bswap(a, "t4", "t3", "t2", "t5")
    a.sw("t4", "t1", 4)
    a.addi("t1", "t1", 8)
    a.sub("a1", "t1", "a0")
    a.srli("a1", "a1", 6)
    a.li("t5", h0)
    a.li("t6", state)
    lib.copy_words("t6", "t5", 8)
    a.li("a2", state)
    a.call("sha256_blocks")
    lib.pop_ret()

    # =========================================================================================== main
    a.label("main")
    a.li("sp", lib.stack)
    a.li("t0", SYS_HINT_LEN)
    a.ecall()
    a.mv("a1", "t0")
    a.li("a0", HEAP)
    a.li("t0", SYS_HINT_READ)
    a.ecall()
    a.li("a0", HEAP + 8)                    # behind the u64 length of the bincode Vec<u8>
    # ---- SharedData = map(3): base_hashes, initial_commitment, seeds_exchange_commitment  (a malformed input panics, main.rs:21-22)
    a.call("cbor_head")
    a.addi("t1", "a1", -5)
    a.addi("t2", "a2", -3)
    a.or_("t1", "t1", "t2")
    fail_if_ne("t1", "zero", "top")
    hex_array(11, V_NH, nmax, "bh", hashes, 32)          # "base_hashes"
    a.li("a3", 18)
    a.call("cbor_text")                     # "initial_commitment"
    a.call("cbor_head")                     # map(3)
    text_hex(4, ic_hash, 32)                # "hash"
    a.li("a3", 8)
    a.call("cbor_text")                     # "settings"
    a.call("cbor_head")                     # map(3)
    for var in (V_N, V_K):
        a.li("a3", 1)
        a.call("cbor_text")                 # "n" / "k"
        a.call("cbor_head")                 # uint
        fail_if_ne("a1", "zero", f"uint{var}")
        sv("a2", var)
    text_hex(6, gen_id, 16)                 # "gen_id"
    hex_array(12, V_NPK, kmax, "pk", pks, 48)            # "base_pubkeys"
    a.li("a3", 25)
    a.call("cbor_text")                     # "seeds_exchange_commitment"
    a.call("cbor_head")                     # map(3)
    text_hex(23, ich, 32)                   # "initial_commitment_hash" (used by the auth build only)
    a.li("a3", 7)
    a.call("cbor_text")                     # "ssecret"
    a.call("cbor_head")                     # map(2)
    text_hex(13, dst, 32)                   # "dst_base_hash"
    text_hex(13, sk_be, 32)                 # "shared_secret"
    a.li("a3", 10)
    a.call("cbor_text")                     # "commitment"
    a.call("cbor_head")
    a.addi("t1", "a1", -5)
    a.addi("t2", "a2", -1)
    a.or_("t1", "t1", "t2")
    fail_if_ne("t1", "zero", "cmap")        # map(1): the no-auth Commitment has the pubkey alone (types.rs:71-78)
    text_hex(6, secp, SECP_PK)              # "pubkey"
    # ---- sanity panics (main.rs:24-43)
    lv("t1", V_NH)
    lv("t2", V_N)
    fail_if_ne("t1", "t2", "nh")            # "The number of verification hashes does not match the number of keys"
    lv("t3", V_K)
    a.bgeu("t2", "t3", "n_ge_k")
    a.halt(1)                               # "N should be greater than or equal to k"
    a.label("n_ge_k")
    a.li("t1", 0)
    sv("t1", V_I)
    a.label("in_l")                         # initial_commitment.hash must be one of the base hashes
    lv("t1", V_I)
    lv("t2", V_NH)
    a.bne("t1", "t2", "in_more")
    a.halt(1)                               # none equal: "The seed exchange commitment is not part of the verification hashes"
    a.label("in_more")
    a.slli("t1", "t1", 5)
    a.li("a0", hashes)
    a.add("a0", "a0", "t1")
    a.li("a1", ic_hash)
    a.li("a2", 32)
    a.call("bytes_cmp")
    a.beq("a0", "zero", "in_found")
    lv("t1", V_I)
    a.addi("t1", "t1", 1)
    sv("t1", V_I)
    a.j("in_l")
    a.label("in_found")
    # initial_commitment.hash = SHA-256(gen_id || n || k || len(base_pubkeys) as u8 || base_pubkeys)  (verification.rs:151-183)
    a.li("s2", msgbuf)
    a.li("t5", gen_id)
    lib.copy_words("s2", "t5", 4)
    lv("t1", V_N)
    a.sb("t1", "s2", 16)
    lv("t1", V_K)
    a.sb("t1", "s2", 17)
    lv("t1", V_NPK)
    a.sb("t1", "s2", 18)
    a.addi("s3", "s2", 19)
    a.li("s4", pks)
    a.li("t3", 48)
    a.mul("s5", "t1", "t3")                 # bytes of keys
    a.mv("a1", "s5")
    a.addi("a1", "a1", 19)                  # message length
    a.beq("s5", "zero", "ih_hash")
    a.label("ih_cp")
    a.lbu("t1", "s4", 0)
    a.sb("t1", "s3", 0)
    a.addi("s3", "s3", 1)
    a.addi("s4", "s4", 1)
    a.addi("s5", "s5", -1)
    a.bne("s5", "zero", "ih_cp")
    a.label("ih_hash")
    a.li("a0", msgbuf)
    a.call("sha_msg")
    a.li("s8", state)
    a.li("s1", ic_hash)
    for i in range(8):                      # digest word i (big-endian) against the hash bytes
        a.lw("t1", "s8", 4 * i)
        _bswap(a, "t3", "t1", "t2", "t6")
        a.lw("t4", "s1", 4 * i)
        fail_if_ne("t3", "t4", f"ih{i}")    # "Unsalshable error while verifying commitment hash"
    # ---- verify_seed_exchange_commitment (verification.rs:91-148); the shared secret must be a scalar below r
    a.li("a0", sk_be)
    a.li("a1", r_be)
    a.li("a2", 32)
    a.call("bytes_cmp")
    a.li("t1", 2)
    slash_if_ne("a0", "t1", "sk")           # "Invalid field seeds_exchange_commitment.shared_secret.secret"
    # id = 1 + the number of base hashes below dst_base_hash, if it is one of them (get_index_in_commitments, :50-66)
    a.li("t1", 1)
    sv("t1", V_ID)
    sv("zero", V_FOUND)
    sv("zero", V_I)
    a.label("id_l")
    lv("t1", V_I)
    lv("t2", V_NH)
    a.beq("t1", "t2", "id_done")
    a.slli("t1", "t1", 5)
    a.li("a0", hashes)
    a.add("a0", "a0", "t1")
    a.li("a1", dst)
    a.li("a2", 32)
    a.call("bytes_cmp")
    a.bne("a0", "zero", "id_ne")
    a.li("t1", 1)
    sv("t1", V_FOUND)
    a.label("id_ne")
    a.addi("a0", "a0", -2)
    a.bne("a0", "zero", "id_next")
    lv("t1", V_ID)
    a.addi("t1", "t1", 1)
    sv("t1", V_ID)
    a.label("id_next")
    lv("t1", V_I)
    a.addi("t1", "t1", 1)
    sv("t1", V_I)
    a.j("id_l")
    a.label("id_done")
    lv("t1", V_FOUND)
    a.li("t2", 1)
    slash_if_ne("t1", "t2", "dst")          # "Invalid field seeds_exchange_commitment.shared_secret.dst_base_hash"
    # every base pubkey through G1Affine::from_compressed; a bad one panics (`.expect("Invalid pubkey")`, :132-137)
    sv("zero", V_J)
    a.label("dec_l")
    lv("t1", V_J)
    lv("t2", V_NPK)
    a.beq("t1", "t2", "dec_done")
    a.li("t2", 48)
    a.mul("t1", "t1", "t2")
    a.li("a1", pks)
    a.add("a1", "a1", "t1")
    a.lbu("t1", "a1", 0)                    # the point at infinity must be canonical: 0xC0 and 47 zero bytes
    a.andi("t2", "t1", 0x40)
    a.beq("t2", "zero", "dec_fin")
    a.lw("t1", "a1", 0)
    a.addi("t1", "t1", -0xC0)
    for i in range(1, 12):
        a.lw("t2", "a1", 4 * i)
        a.or_("t1", "t1", "t2")
    fail_if_ne("t1", "zero", "inf")
    a.label("dec_fin")
    lv("t1", V_J)
    a.li("t2", 4 * POINT_WORDS)
    a.mul("t1", "t1", "t2")
    a.li("a0", cfs)
    a.add("a0", "a0", "t1")
    sv("a0", V_P)
    a.call("g1_decompress")
    if subgroup_check:
        lv("a0", V_P)
        a.call("g1_check_subgroup")
    lv("t1", V_J)
    a.addi("t1", "t1", 1)
    sv("t1", V_J)
    a.j("dec_l")
    a.label("dec_done")
    # Horner at id (dkg_math.rs:160-174): y = cfs[k-1]; for j = k-2 .. 0: y = [id] y + cfs[j]; no coefficients: the identity
    a.li("t4", hy)
    a.li("t1", 1)
    a.sw("t1", "t4", 96)
    lv("t1", V_NPK)
    a.beq("t1", "zero", "ev_done")
    a.addi("t1", "t1", -1)
    sv("t1", V_J)
    a.li("t2", 4 * POINT_WORDS)
    a.mul("t1", "t1", "t2")
    a.li("t5", cfs)
    a.add("t5", "t5", "t1")
    lib.copy_words("t4", "t5", POINT_WORDS)
    a.label("ev_j")
    lv("t1", V_J)
    a.beq("t1", "zero", "ev_done")
    a.li("a0", htmp)
    a.li("a1", hy)
    a.li("a2", V_ID)
    a.li("a3", 1)
    a.call("scalar_mul")
    lv("t1", V_J)
    a.addi("t1", "t1", -1)
    sv("t1", V_J)
    a.li("t2", 4 * POINT_WORDS)
    a.mul("t1", "t1", "t2")
    a.li("a1", cfs)
    a.add("a1", "a1", "t1")
    a.li("a0", htmp)
    a.call("g1_add")
    a.li("t4", hy)
    a.li("t5", htmp)
    lib.copy_words("t4", "t5", POINT_WORDS)
    a.j("ev_j")
    a.label("ev_done")
    # [sk] G against the evaluation, compressed
    a.li("t5", sk_be)
    a.li("t6", sk_le)
    for i in range(8):                      # big-endian bytes -> little-endian words
        a.lw("t1", "t5", 4 * (7 - i))
        _bswap(a, "t3", "t1", "t2", "t4")
        a.sw("t3", "t6", 4 * i)
    a.li("a0", skpt)
    a.li("a1", g1)
    a.li("a2", sk_le)
    a.li("a3", 8)
    a.call("scalar_mul")
    a.li("a0", cmp_a)
    a.li("a1", skpt)
    a.call("g1_compress")
    a.li("a0", cmp_b)
    a.li("a1", hy)
    a.call("g1_compress")
    a.li("a0", cmp_a)
    a.li("a1", cmp_b)
    a.li("a2", 48)
    a.call("bytes_cmp")
    slash_if_ne("a0", "zero", "pk")         # "Bad secret field : Expected secret with public key ..."
    a.halt(1)                               # "The seed exchange commitment is valid" (main.rs:81)

    # ---- slashable: public values = for every base hash IN INPUT ORDER u64(64) || hex(hash); then u64(66) || hex(pubkey)
    a.label("slash")
    a.li("t1", pvbuf)
    sv("t1", V_END)
    sv("zero", V_I)
    a.label("pv_l")
    lv("t1", V_I)
    lv("t2", V_NH)
    a.beq("t1", "t2", "pv_done")
    lv("s10", V_END)
    a.li("t1", 64)
    a.sw("t1", "s10", 0)
    a.sw("zero", "s10", 4)
    lv("t1", V_I)
    a.slli("t1", "t1", 5)
    a.li("a0", hashes)
    a.add("a0", "a0", "t1")
    a.addi("a1", "s10", 8)
    a.li("a2", 32)
    a.call("hex_encode")
    lv("s10", V_END)
    a.addi("s10", "s10", 72)
    sv("s10", V_END)
    lv("t1", V_I)
    a.addi("t1", "t1", 1)
    sv("t1", V_I)
    a.j("pv_l")
    a.label("pv_done")
    lv("s10", V_END)
    a.li("t1", 2 * SECP_PK)
    a.sw("t1", "s10", 0)
    a.sw("zero", "s10", 4)
    a.li("a0", secp)
    a.addi("a1", "s10", 8)
    a.li("a2", SECP_PK)
    a.call("hex_encode")
    lv("s10", V_END)
    a.addi("s10", "s10", 8 + 2 * SECP_PK)
    # ---- commit: WRITE to fd 3, SHA-256 of the bytes, COMMIT the eight digest words
    a.li("a1", pvbuf)
    a.sub("a2", "s10", "a1")
    sv("a2", V_END)                         # (now the byte count)
    a.li("a0", 3)
    a.li("t0", SYS_WRITE)
    a.ecall()
    a.li("a0", pvbuf)
    lv("a1", V_END)
    a.call("sha_msg")
    a.li("s8", state)
    for k_ in range(8):
        a.lw("t1", "s8", 4 * k_)
        _bswap(a, "a1", "t1", "t2", "t6")
        a.li("a0", k_)
        a.li("t0", SYS_COMMIT)
        a.ecall()
    a.halt(0)
    return a.elf()
