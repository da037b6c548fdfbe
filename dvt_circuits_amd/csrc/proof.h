// Shard proof container and its wire format.
//
// The reference stores `SP1ProofWithPublicValues` with bincode (src/main.rs:472-474);
// that layout lives in the absent sp1-sdk crate, so this
// library defines its own: a flat little-endian stream of u32 words, every field
// element in canonical form, every vector preceded by its length.  DESIGN.md
// "Proof format" lists the fields in order.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "poseidon2.cuh"

namespace dvt {

struct ChipOpening {
    uint32_t chip_id = 0, log_n = 0;
    Fp4 cumsum;
    std::vector<Fp4> prep_l, prep_n, main_l, main_n, perm_l, perm_n, quot;  // quot: 2 chunks x 4 columns
};
struct TreeOpening {
    std::vector<std::vector<Fp>> rows;  // one opened row per matrix of the tree, in tree order
    std::vector<Digest> path;
};
struct FriLayerOpening {
    Fp4 sibling;
    std::vector<Digest> path;
};
struct QueryProof {
    TreeOpening trees[4];  // preprocessed, main, permutation, quotient
    std::vector<FriLayerOpening> layers;
};
struct ShardProof {
    Digest main_root, perm_root, quot_root;
    std::vector<Fp> public_values;
    std::vector<ChipOpening> chips;
    std::vector<Digest> fri_roots;
    Fp4 final_poly;
    Fp pow_witness;
    std::vector<QueryProof> queries;
    // the prover fills the query section directly in wire format (canonical words, exactly what write_shard_proof
    // emits for `queries`, including the leading count) instead of building `queries`: one pass over the downloaded
    // gather buffer, no per-query vectors.  Empty = serialise `queries`.
    std::vector<uint32_t> query_words;
    // The compact form ("DVP2"): no query carries a path; every tree of the shard (trees 0..3, then the FRI layers in
    // order) carries the nodes its queries cannot compute themselves, once, in the order of multipath_plan.
    bool compact = false;
    std::vector<std::vector<Digest>> node_lists;
};

// ---- shared Merkle paths.  Parents pair (i, i + half): node j of level s-1 has the children j and j + half of level s
// (level s has 2^s nodes, level `depth` holds the leaves).  K_s is the set of nodes of level s on a path from a queried
// leaf.  For s = depth .. 1 and n ascending over K_s, the sibling n ^ half is LISTED when it is not in K_s itself: a
// verifier that knows the leaves of K_depth and the listed nodes computes every node of every K_s, down to the root.
// Pure index logic: nothing here reads a digest.
constexpr uint32_t MP_LISTED = 0x80000000u;
struct MultipathJob {
    uint32_t l, r;   // the children: a slot of the level below (position in its sorted K_s), or MP_LISTED | k: the k-th listed node
    uint32_t j;      // the parent's index in level s-1; job i of a level writes slot i of the level above
};
struct MultipathPlan {
    uint32_t depth = 0;
    std::vector<std::vector<uint32_t>> keys;         // [s] = K_s, ascending, for s = 0 .. depth
    std::vector<std::vector<MultipathJob>> levels;   // [depth - s] for s = depth .. 1, each ascending in j
    std::vector<std::pair<uint32_t, uint32_t>> nodes;   // the listed nodes (level, index), in the order of the wire format
    std::vector<uint32_t> base;                      // [s] = how many listed nodes lie on levels above s (base[depth] = 0)
    // The plan of the same indices for a tree of only d <= depth levels is this plan from level d on: its leaves are
    // keys[d], its levels are levels[depth - s] for s = d .. 1, and its listed nodes are nodes[base[d] ..], so that a job's
    // k-th listed node is the tree's (k - base[d])-th.  All trees of a shard are walked with one plan.
    size_t listed(uint32_t d) const { return nodes.size() - base[d]; }
};
inline MultipathPlan multipath_plan(uint32_t depth, const uint32_t *indices, size_t n) {
    MultipathPlan pl;
    pl.depth = depth;
    std::vector<uint32_t> K(n);
    for (size_t i = 0; i < n; i++) K[i] = indices[i] & (uint32_t)(((uint64_t)1 << depth) - 1);
    std::sort(K.begin(), K.end());
    K.erase(std::unique(K.begin(), K.end()), K.end());
    pl.keys.resize(depth + 1);
    pl.base.assign(depth + 1, 0);
    pl.keys[depth] = K;
    pl.levels.resize(depth);
    for (uint32_t s = depth; s >= 1; s--) {
        const uint32_t half = 1u << (s - 1);
        const size_t m = std::lower_bound(K.begin(), K.end(), half) - K.begin();   // K[0, m) are left children, K[m, ..) right ones
        // (both halves ascending: a sibling is present when the other half holds the same offset)
        std::vector<uint32_t> listed(K.size(), 0);
        for (size_t i = 0, k = m; i < m || k < K.size();) {
            const uint32_t a = i < m ? K[i] : 0xffffffffu, b = k < K.size() ? K[k] - half : 0xffffffffu;
            if (a == b) { i++; k++; }
            else if (a < b) listed[i++] = MP_LISTED;
            else listed[k++] = MP_LISTED;
        }
        for (size_t i = 0; i < K.size(); i++)      // n ascending over K_s
            if (listed[i]) {
                listed[i] = MP_LISTED | (uint32_t)pl.nodes.size();
                pl.nodes.push_back({s, K[i] ^ half});
            }
        std::vector<MultipathJob> &jobs = pl.levels[depth - s];
        std::vector<uint32_t> &up = pl.keys[s - 1];
        for (size_t i = 0, k = m; i < m || k < K.size();) {
            const uint32_t a = i < m ? K[i] : 0xffffffffu, b = k < K.size() ? K[k] - half : 0xffffffffu, j = std::min(a, b);
            jobs.push_back({a == j ? (uint32_t)i : listed[k], b == j ? (uint32_t)k : listed[i], j});
            up.push_back(j);
            if (a == j) i++;
            if (b == j) k++;
        }
        pl.base[s - 1] = (uint32_t)pl.nodes.size();
        K = up;
    }
    return pl;
}

struct WordWriter {
    std::vector<uint32_t> w;
    void u32(uint32_t v) { w.push_back(v); }
    void fp(Fp x) { w.push_back(x.canonical()); }
    void ef(const Fp4 &x) { for (int i = 0; i < 4; i++) fp(x.c[i]); }
    void dg(const Digest &d) { for (int i = 0; i < 8; i++) fp(d.d[i]); }
    void fps(const std::vector<Fp> &v) { u32((uint32_t)v.size()); for (auto x : v) fp(x); }
    void efs(const std::vector<Fp4> &v) { u32((uint32_t)v.size()); for (auto &x : v) ef(x); }
    void dgs(const std::vector<Digest> &v) { u32((uint32_t)v.size()); for (auto &x : v) dg(x); }
};
struct WordReader {
    const uint32_t *p, *end;
    WordReader(const uint32_t *b, size_t n) : p(b), end(b + n) {}
    uint32_t u32() { if (p >= end) throw std::runtime_error("proof truncated"); return *p++; }
    uint32_t len(uint32_t max) { uint32_t n = u32(); if (n > max) throw std::runtime_error("proof: vector too long"); return n; }
    Fp fp() { uint32_t v = u32(); if (v >= P) throw std::runtime_error("proof: non-canonical field element"); return Fp::from_canonical(v); }
    Fp4 ef() { Fp4 r; for (int i = 0; i < 4; i++) r.c[i] = fp(); return r; }
    Digest dg() { Digest d; for (int i = 0; i < 8; i++) d.d[i] = fp(); return d; }
    std::vector<Fp> fps(uint32_t max = 1 << 20) { uint32_t n = len(max); std::vector<Fp> v(n); for (auto &x : v) x = fp(); return v; }
    std::vector<Fp4> efs(uint32_t max = 1 << 20) { uint32_t n = len(max); std::vector<Fp4> v(n); for (auto &x : v) x = ef(); return v; }
    std::vector<Digest> dgs(uint32_t max = 64) { uint32_t n = len(max); std::vector<Digest> v(n); for (auto &x : v) x = dg(); return v; }
};

constexpr uint32_t SHARD_PROOF_MAGIC = 0x31505644u;  // "DVP1"
constexpr uint32_t SHARD_PROOF_MAGIC_COMPACT = 0x32505644u;  // "DVP2"
constexpr uint32_t MAX_QUERIES = 1024, MAX_TREE_DEPTH = 22;

inline void write_shard_proof(WordWriter &w, const ShardProof &p) {
    w.u32(p.compact ? SHARD_PROOF_MAGIC_COMPACT : SHARD_PROOF_MAGIC);
    w.dg(p.main_root); w.dg(p.perm_root); w.dg(p.quot_root);
    w.fps(p.public_values);
    w.u32((uint32_t)p.chips.size());
    for (auto &c : p.chips) {
        w.u32(c.chip_id); w.u32(c.log_n); w.ef(c.cumsum);
        w.efs(c.prep_l); w.efs(c.prep_n); w.efs(c.main_l); w.efs(c.main_n);
        w.efs(c.perm_l); w.efs(c.perm_n); w.efs(c.quot);
    }
    w.dgs(p.fri_roots); w.ef(p.final_poly); w.fp(p.pow_witness);
    if (!p.query_words.empty()) {
        w.w.insert(w.w.end(), p.query_words.begin(), p.query_words.end());
        return;
    }
    w.u32((uint32_t)p.queries.size());
    for (auto &q : p.queries) {
        for (int t = 0; t < 4; t++) {
            w.u32((uint32_t)q.trees[t].rows.size());
            for (auto &r : q.trees[t].rows) w.fps(r);
            if (!p.compact) w.dgs(q.trees[t].path);
        }
        w.u32((uint32_t)q.layers.size());
        for (auto &l : q.layers) { w.ef(l.sibling); if (!p.compact) w.dgs(l.path); }
    }
    if (p.compact)
        for (auto &l : p.node_lists) w.dgs(l);
}

inline ShardProof read_shard_proof(WordReader &r) {
    ShardProof p;
    const uint32_t magic = r.u32();
    if (magic != SHARD_PROOF_MAGIC && magic != SHARD_PROOF_MAGIC_COMPACT) throw std::runtime_error("proof: bad magic");
    p.compact = magic == SHARD_PROOF_MAGIC_COMPACT;
    p.main_root = r.dg(); p.perm_root = r.dg(); p.quot_root = r.dg();
    p.public_values = r.fps(1 << 12);
    uint32_t nc = r.len(64);
    p.chips.resize(nc);
    for (auto &c : p.chips) {
        c.chip_id = r.u32(); c.log_n = r.u32(); c.cumsum = r.ef();
        // (untrusted input: bound both before anything indexes with them; the machine's own chip count is checked by the verifier)
        if (c.chip_id >= 64 || c.log_n > 22) throw std::runtime_error("proof: chip id or height out of range");
        c.prep_l = r.efs(1 << 12); c.prep_n = r.efs(1 << 12); c.main_l = r.efs(1 << 12); c.main_n = r.efs(1 << 12);
        c.perm_l = r.efs(1 << 12); c.perm_n = r.efs(1 << 12); c.quot = r.efs(8);
    }
    p.fri_roots = r.dgs(); p.final_poly = r.ef(); p.pow_witness = r.fp();
    uint32_t nq = r.len(MAX_QUERIES);
    p.queries.resize(nq);
    for (auto &q : p.queries) {
        for (int t = 0; t < 4; t++) {
            uint32_t nm = r.len(256);
            q.trees[t].rows.resize(nm);
            for (auto &row : q.trees[t].rows) row = r.fps(1 << 12);
            if (!p.compact) q.trees[t].path = r.dgs();
        }
        uint32_t nl = r.len(64);
        q.layers.resize(nl);
        for (auto &l : q.layers) { l.sibling = r.ef(); if (!p.compact) l.path = r.dgs(); }
    }
    if (p.compact) {
        // one list per tree: the four input trees, then one per FRI root (the verifier checks that number against the
        // chips' heights).  No tree lists more than one node per query and level.
        p.node_lists.resize(4 + p.fri_roots.size());
        for (auto &l : p.node_lists) l = r.dgs(MAX_QUERIES * MAX_TREE_DEPTH);
    }
    return p;
}

// The rv32 proof container ("DVC3"): the guest's exit code, its public-value bytes (little-endian, zero-padded to whole
// words) and the shard proofs in shard order, each preceded by its length in words.
constexpr uint32_t CORE_PROOF_MAGIC = 0x33435644u;  // "DVC3"

struct CoreProof {
    uint32_t exit_code = 0;
    std::vector<uint8_t> public_values;
    std::vector<std::vector<uint32_t>> shards;   // the words of each shard proof
};

inline std::vector<uint32_t> write_core_proof(const CoreProof &c) {
    WordWriter w;
    w.u32(CORE_PROOF_MAGIC);
    w.u32((uint32_t)c.shards.size());
    w.u32(c.exit_code);
    const auto &pv = c.public_values;
    w.u32((uint32_t)pv.size());
    for (size_t i = 0; i < pv.size(); i += 4) {
        uint32_t v = 0;
        for (size_t k = 0; k < 4 && i + k < pv.size(); k++) v |= (uint32_t)pv[i + k] << (8 * k);
        w.u32(v);
    }
    for (auto &s : c.shards) {
        w.u32((uint32_t)s.size());
        w.w.insert(w.w.end(), s.begin(), s.end());
    }
    return w.w;
}

// (untrusted input: throws on anything but the one encoding of a container; the shard proofs are not parsed here)
inline CoreProof read_core_proof(WordReader &r) {
    CoreProof c;
    if (r.u32() != CORE_PROOF_MAGIC) throw std::runtime_error("bad container magic");
    const uint32_t nshards = r.len(1 << 16);
    if (nshards == 0) throw std::runtime_error("no shards");
    c.exit_code = r.u32();
    const uint32_t pvl = r.len(1 << 24);
    // the AIR pins exit codes below 2^24 (the code itself, not a residue): a container word ec + p would pass the
    // comparison mod p of the verifier and be reported to the caller as is
    if (c.exit_code >> 24) throw std::runtime_error("exit code out of range");
    c.public_values.resize(pvl);
    for (uint32_t i = 0; i < pvl; i += 4) {
        uint32_t v = r.u32();
        for (uint32_t k = 0; k < 4; k++) {
            if (i + k < pvl) c.public_values[i + k] = (uint8_t)(v >> (8 * k));
            else if ((v >> (8 * k)) & 0xff) throw std::runtime_error("non-zero padding after the public values");   // (one encoding per proof)
        }
    }
    c.shards.resize(nshards);
    for (auto &s : c.shards) {
        uint32_t nw = r.len(1u << 30);
        if ((size_t)(r.end - r.p) < nw) throw std::runtime_error("container truncated");
        s.assign(r.p, r.p + nw);
        r.p += nw;
    }
    if (r.p != r.end) throw std::runtime_error("trailing bytes after proof");
    return c;
}

}  // namespace dvt
