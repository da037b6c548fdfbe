// Mutation fuzz driver of the compact proof form ("DVP2", csrc/proof.h) on the UNTRUSTED-input side of the library:
// dvt_verify, dvt_proof_compact and dvt_proof_expand (csrc/capi_rv32.hip, csrc/verifier.hip).  Built host-only with
// AddressSanitizer + UBSan by `make -C dvt_circuits_amd/csrc asan-fuzz-compact` (no GPU involved: sanitizers run on the
// CPU build only) and run by tests/test_compact_fuzz.py on the fixtures fuzz_verify takes.
//
//   fuzz_compact <fixture> <iterations> <seed> <fri_queries> <pow_bits>
// fixture = u32 vk_len | vk | proof.  The proof is compacted first; the compact proof must verify and expand back to the
// fixture's bytes.  Every mutated compact proof then goes through all three entry points, each of which must come back
// with a clean DVT_OK / DVT_ERR_REJECTED / DVT_ERR_INPUT; the sanitizers abort on any out-of-bounds access, overflow or
// other undefined behaviour on the way.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvt_prover.h"

static uint64_t rng_state;
static uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
typedef std::vector<uint8_t> Bytes;
typedef int (*Transcode)(const uint8_t *, size_t, const uint8_t *, size_t, uint32_t, uint32_t, uint8_t **, size_t *, char **);

int main(int argc, char **argv) {
    if (argc < 6) { fprintf(stderr, "usage: fuzz_compact fixture iterations seed fri_queries pow_bits\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror("fixture"); return 2; }
    Bytes all;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) all.insert(all.end(), buf, buf + n);
    fclose(f);
    if (all.size() < 8) return 2;
    uint32_t vk_len;
    memcpy(&vk_len, all.data(), 4);
    if (4 + (size_t)vk_len >= all.size()) return 2;
    const Bytes vk(all.begin() + 4, all.begin() + 4 + vk_len), plain(all.begin() + 4 + vk_len, all.end());
    const long iters = atol(argv[2]);
    rng_state = strtoull(argv[3], nullptr, 10) * 2 + 1;
    const uint32_t q = (uint32_t)atoi(argv[4]), pw = (uint32_t)atoi(argv[5]);
    auto verify = [&](const Bytes &p) {
        int32_t ec = 0; uint8_t *pv = nullptr; size_t pvl = 0; char *why = nullptr;
        int rc = dvt_verify(vk.data(), vk.size(), p.data(), p.size(), q, pw, &ec, &pv, &pvl, &why);
        if (pv) dvt_free(pv);
        if (why) dvt_free(why);
        return rc;
    };
    auto transcode = [&](Transcode fn, const Bytes &p, Bytes *out) {
        uint8_t *o = nullptr; size_t ol = 0; char *why = nullptr;
        int rc = fn(vk.data(), vk.size(), p.data(), p.size(), q, pw, &o, &ol, &why);
        if (rc == DVT_OK && out) out->assign(o, o + ol);
        if (o) dvt_free(o);
        if (why) dvt_free(why);
        return rc;
    };
    if (verify(plain) != DVT_OK) { fprintf(stderr, "the pristine fixture does not verify\n"); return 3; }
    Bytes proof, back;
    if (transcode(dvt_proof_compact, plain, &proof) != DVT_OK || verify(proof) != DVT_OK || proof.size() >= plain.size() ||
        transcode(dvt_proof_expand, proof, &back) != DVT_OK || back != plain) {
        fprintf(stderr, "compact / expand of the pristine fixture failed\n");
        return 4;
    }
    long ok = 0, rejected = 0, input = 0, other = 0;
    auto tally = [&](int rc) {
        if (rc == DVT_OK) ok++;
        else if (rc == DVT_ERR_REJECTED) rejected++;
        else if (rc == DVT_ERR_INPUT) input++;
        else other++;
    };
    for (long it = 0; it < iters; it++) {
        Bytes p = proof;
        const int kind = (int)(rnd() % 8);
        if (kind == 0) {                                  // truncate
            p.resize(rnd() % p.size());
        } else if (kind == 1 || kind == 2) {              // a word becomes a hostile count: huge, tiny, or off by one
            size_t at = (rnd() % (p.size() / 4)) * 4;
            uint32_t w;
            memcpy(&w, &p[at], 4);
            const int how = (int)(rnd() % 4);
            w = how == 0 ? 0xFFFFFFFFu : how == 1 ? (uint32_t)(rnd() % 5) : how == 2 ? w + 1 : w - 1;
            memcpy(&p[at], &w, 4);
        } else if (kind == 3) {                           // splice: copy a random window over another place
            size_t len = 1 + rnd() % 64, a = rnd() % (p.size() - len), b = rnd() % (p.size() - len);
            memmove(&p[a], &p[b], len);
        } else if (kind == 4) {                           // append garbage
            for (int k = 0; k < 8; k++) p.push_back((uint8_t)rnd());
        } else if (kind == 5) {                           // a shard's magic flips between the two forms
            const uint32_t m1 = 0x31505644u, m2 = 0x32505644u;
            for (size_t at = 0, seen = rnd() % 4; at + 4 <= p.size(); at += 4) {
                uint32_t w;
                memcpy(&w, &p[at], 4);
                if (w == m2 && seen-- == 0) { memcpy(&p[at], &m1, 4); break; }
            }
        } else {                                          // 1..4 random byte changes, biased to the tail (the node lists)
            int m = 1 + (int)(rnd() % 4);
            for (int k = 0; k < m; k++) {
                size_t at = (rnd() & 1) ? rnd() % p.size() : p.size() - 1 - rnd() % (p.size() < 8192 ? p.size() : 8192);
                p[at] ^= (uint8_t)(1 + rnd() % 255);
            }
        }
        tally(verify(p));
        tally(transcode(dvt_proof_compact, p, nullptr));
        tally(transcode(dvt_proof_expand, p, nullptr));
    }
    printf("{\"iterations\": %ld, \"ok\": %ld, \"rejected\": %ld, \"input\": %ld, \"other\": %ld}\n", iters, ok, rejected, input, other);
    return other ? 5 : 0;
}
