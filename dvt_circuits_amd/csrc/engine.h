// Shard prover / verifier for a generic multi-chip machine.  The prover keeps
// every matrix in HBM (column-major, Montgomery form) for the whole shard and runs
// K1-K9 on one HIP stream; the host only drives the transcript.
//
// Stands behind reference src/main.rs:462-466 (`setup`, `prove(..).run()`); the
// protocol itself is an original restatement of the public multi-table STARK
// structure, see DESIGN.md "Protocol".
#pragma once
#include <array>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "challenger.h"
#include "keep_plan.h"
#include "machine.h"
#include "proof.h"

namespace dvt {

struct StarkConfig {
    uint32_t num_queries = 100;
    uint32_t pow_bits = 16;
    bool compact_openings = false;   // the prover writes the compact form of a shard proof (DVP2, proof.h); verifiers read both
};

struct ChipRef {
    int chip_id;
    uint32_t log_n;
};

struct VerifyingKey {
    const MachineDesc *machine = nullptr;
    Digest prep_root;                 // all-zero when the machine has no preprocessed chip
    std::vector<ChipRef> prep_chips;  // chips with preprocessed columns (always part of every shard)
    std::vector<uint32_t> extra;      // machine-specific words bound into the key (rv32: entry pc)
};

// FRI batching order of the LDE columns of log-height h: every column opened at two
// points (preprocessed, main, permutation; tree-major, then chip, then column) first,
// then the quotient columns (opened at zeta only).
struct ColRef {
    int tree, mat, col, chip_pos;
};
std::vector<ColRef> fri_columns(const MachineDesc *m, const std::vector<ChipRef> &chips, uint32_t h, uint32_t *n_two);
void transcript_begin(Challenger &ch, const VerifyingKey &vk, const std::vector<ChipRef> &chips);

// LogUp challenges shared by all shards of one execution (derived from every shard's main commitment);
// nullptr = the shard samples its own (single, self-contained proof).
struct PermChallenges {
    Fp4 alpha, beta;
};
// returns "" on success, otherwise the reason for rejection.  With cumsum_total != nullptr the sum of the
// chips' cumulative sums is returned instead of being required to vanish (the caller balances it across shards).
std::string verify_shard(const VerifyingKey &vk, const ShardProof &proof, const StarkConfig &cfg,
                         const PermChallenges *global = nullptr, Fp4 *cumsum_total = nullptr);

// The two parts of verify_shard.  The host part (shape checks, transcript, constraint check at zeta, FRI challenges, PoW,
// query indices) leaves what the query part needs in a ShardQueryCtx, which refers to the key and the proof it was made
// from; the query part is verify_query_host per query (dvt_verify) or the device path (verify_query.hip).
struct TreeShape {
    std::vector<std::pair<uint32_t, uint32_t>> mats;  // (width, log_h) in tree order
    uint32_t log_h = 0;
};
// Who provides what when the queries of a shard walk its trees together (proof.h, MultipathPlan: one plan of hmax levels
// serves every tree, a tree of d levels from level d on).  first[lh][slot]: the first query whose path passes the slot-th
// node (ascending index, plan.keys[lh]) of level lh; dups[lh]: (that query, a later query on the same node): where a tree
// has a digest per query at that level (leaves, rows of shorter matrices), both must carry the same.  listed_at[s]: the
// listed nodes of level s as (index, position in plan.nodes), ascending.
struct TreeSources {
    MultipathPlan plan;
    std::vector<std::vector<uint32_t>> first;
    std::vector<std::vector<std::array<uint32_t, 2>>> dups;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> listed_at;
};
TreeSources tree_sources(uint32_t depth, const std::vector<uint32_t> &idx);
struct ShardQueryCtx {
    const VerifyingKey *vk = nullptr;
    const ShardProof *pf = nullptr;
    uint32_t hmax = 0;
    Fp4 zeta;
    std::vector<Fp4> fold_betas, apow;               // per FRI layer; alpha_fri^0 .. alpha_fri^max_cols
    TreeShape shapes[4];
    const Digest *roots[4] = {};
    std::vector<std::vector<ColRef>> cols_by_h;      // [h] for h = 1 .. hmax
    std::vector<uint32_t> n_two_by_h;
    std::vector<uint32_t> idx;                       // the query indices (hmax bits each)
    TreeSources paths;                               // of a compact proof: tree_sources(hmax, idx)
};
std::string verify_shard_host(const VerifyingKey &vk, const ShardProof &proof, const StarkConfig &cfg, const PermChallenges *global,
                              Fp4 *cumsum_total, ShardQueryCtx *ctx);
// "" or the first failure of query qi in step order (tree 0..3, layer count, each layer's opening, final value)
std::string verify_query_host(const ShardQueryCtx &ctx, uint32_t qi);
// whether query qi's section passes every shape check (row counts and widths, path lengths, layer count, empty trees)
bool query_shape_ok(const ShardQueryCtx &ctx, uint32_t qi);

// ---- the compact form of a shard proof (DVP2, proof.h): its query part after verify_shard_host has left ctx.
// The checks run tree by tree, not query by query, because a tree's queries are verified together: the four input trees
// (equal digests where queries share a leaf or a row of a shorter matrix, then the walk with the listed nodes), the FRI
// layers in order, then each query's final value.
std::string verify_compact_queries(const ShardQueryCtx &ctx);
// every shape check of a compact shard's query section and node lists (what verify_compact_queries refuses before it hashes)
bool compact_shape_ok(const ShardQueryCtx &ctx, std::string *why = nullptr);
// The query part of a compact shard for tests: every word of every node list changed by +1 in turn (the host part, which
// reads no node list, stands), each time walking the list's tree; counts the words and the changes that were accepted.
void compact_list_sweep(const ShardQueryCtx &ctx, uint64_t *n_words, uint64_t *n_accepted);
// The two transcodings, after the host part: *out is ctx.pf's proof in the other form ("" or why not).  compact_shard drops
// what the rule of multipath_plan drops and hashes nothing; expand_shard recomputes the dropped siblings from the leaves
// upward.  A proof that is already in the wanted form is copied.
std::string compact_shard(const ShardQueryCtx &ctx, ShardProof *out);
std::string expand_shard(const ShardQueryCtx &ctx, ShardProof *out);

#if defined(__HIPCC__)
struct Arena {
    char *base = nullptr;
    size_t cap = 0, off = 0;
    hipError_t reserve(size_t bytes);
    void release();
    void reset() { off = 0; }
    template <class T> T *alloc(size_t n) {
        size_t bytes = (n * sizeof(T) + 255) & ~(size_t)255;
        if (off + bytes > cap) return nullptr;
        T *p = reinterpret_cast<T *>(base + off);
        off += bytes;
        return p;
    }
};

// Size-keyed cache of freed device buffers.  The per-shard buffers of a prove (cycle records, cpu trace, main-trace LDEs,
// Merkle tree: ~3 GB per 2^21-cycle shard) have the same sizes shard after shard and call after call; hipMalloc / hipFree
// of them cost ~80 ms per shard (measured: 3.85 s instead of 1.3 s per 32-shard prove), a cached buffer costs nothing.
// Not thread-safe: one thread at a time (the API thread under the prover's mutex; while phase 1 runs on several lanes, a lane's
// worker or the feeder under the device's admission lock).
struct DevPool {
    std::multimap<size_t, void *> cached;
    std::unordered_map<void *, size_t> live;
    size_t cached_bytes = 0, misses = 0;   // (misses: requests that went to hipMalloc)
    hipError_t alloc_bytes(void **out, size_t bytes) {
        bytes = (bytes + 4095) & ~(size_t)4095;
        auto it = cached.lower_bound(bytes);
        if (it != cached.end() && it->first <= bytes + bytes / 8) {
            *out = it->second;
            live[*out] = it->first;
            cached_bytes -= it->first;
            cached.erase(it);
            return hipSuccess;
        }
        misses++;
        hipError_t e = hipMalloc(out, bytes);
        if (e != hipSuccess) {   // give the cache back to the driver and try once more
            (void)hipGetLastError();
            trim();
            e = hipMalloc(out, bytes);
        }
        if (e == hipSuccess) live[*out] = bytes;
        return e;
    }
    template <class T> hipError_t alloc(T **out, size_t bytes) { return alloc_bytes(reinterpret_cast<void **>(out), bytes); }
    void free(void *p) {
        if (!p) return;
        auto it = live.find(p);
        if (it == live.end()) { (void)hipFree(p); return; }
        cached.emplace(it->second, p);
        cached_bytes += it->second;
        live.erase(it);
    }
    void trim() {
        for (auto &kv : cached) (void)hipFree(kv.second);
        cached.clear();
        cached_bytes = 0;
    }
};

struct ChipTrace {
    int chip_id;
    uint32_t log_n;
    const uint32_t *d_main;  // device [main_w][2^log_n], Montgomery form
};

struct ProvingKey {
    VerifyingKey vk;
    struct Prep { int chip_id; uint32_t log_n; uint32_t *d_trace, *d_lde; };
    std::vector<Prep> prep;
    uint32_t *d_prep_digests = nullptr;
    uint32_t prep_log_h = 0;  // log2 of the tallest preprocessed LDE
};

// Phase-1 results of one shard kept in HBM for phase 2, so that the common-challenge protocol does not pay K1-K3 of the
// main trace twice: the main-trace LDEs and their Merkle tree (KEEP_FULL), or the tree alone (KEEP_TREE, tree_only: phase 2
// pays K1 again and hashes nothing).  Owned by the caller.
struct MainCache {
    bool valid = false;
    bool tree_only = false;      // no LDEs are kept: lde and lde_words stay empty
    DevPool *pool = nullptr;     // where lde / tree came from
    std::vector<uint32_t *> lde;  // one per chip trace, in trace order
    std::vector<size_t> lde_words;
    uint32_t *tree = nullptr;
    uint32_t log_h = 0;
    Digest root;
    int tier() const { return !tree ? KEEP_NONE : tree_only ? KEEP_TREE : KEEP_FULL; }
    // buffers are reused by the next commit of a shard of the same shape (benchmarks prove the same job repeatedly)
    bool fits(const std::vector<size_t> &words, uint32_t h, bool only_tree) const {
        return tree && log_h == h && tree_only == only_tree && (only_tree || lde_words == words);
    }
    size_t tree_bytes() const { return tree ? (((size_t)2 << log_h) - 1) * 32 : 0; }
    size_t lde_bytes() const {
        size_t n = 0;
        for (auto w : lde_words) n += w * 4;
        return n;
    }
    void release() {
        for (auto p : lde) if (p) { if (pool) pool->free(p); else (void)hipFree(p); }
        lde.clear();
        lde_words.clear();
        if (tree) { if (pool) pool->free(tree); else (void)hipFree(tree); }
        tree = nullptr;
        tree_only = false;
        valid = false;
    }
};

struct StageTimes {  // milliseconds, HIP events on the prover stream (profile mode)
    float commit_main = 0, perm = 0, quotient = 0, open = 0, fri = 0, total = 0;
    // kernel families, summed over the launches of one prove_shard call
    float lde_ms = 0;          // K1: ntt_strided<inverse> + lde_block + ntt_strided<forward>
    double lde_alg_bytes = 0;  // sum over LDE calls of 12 * width * N  (read N words, write 2N words per column)
    int lde_calls = 0;
    float merkle_ms = 0;       // K2 + K3 of the three trace commitments (leaf hashing + levels)
    double merkle_perms = 0;   // Poseidon2 permutations executed by them
    // committed cells of the shard in BabyBear elements: main, permutation and quotient
    // (both flattened over F_p^4), preprocessed
    double cells_m = 0, cells_p = 0, cells_q = 0, cells_pre = 0;
};

class Engine {
  public:
    int device = 0;
    hipStream_t stream = nullptr;
    NttTables tabs;
    std::string err;
    StageTimes times;
    bool profile = false;
    // tables of at most 2^parts_parallel_log rows take the part-parallel K4 / K5 launches (stark.cuh); -1 = none.
    // At most PARTS_PARALLEL_LOG: the d_parts scratch is sized for that height.
    int parts_parallel_log = (int)PARTS_PARALLEL_LOG;

    hipError_t init(int dev);
    void shutdown();
    // small host->device tables (column pointer lists, powers, indices); stream-ordered
    const void *upload(const void *host, size_t bytes);
    template <class T> const T *upload_vec(const std::vector<T> &v) { return static_cast<const T *>(upload(v.data(), v.size() * sizeof(T))); }
    bool download(void *host, const void *dev, size_t bytes);  // synchronises the stream

    struct DevMat { const uint32_t *ptr; uint32_t width, log_h; };
    bool commit_tree(const std::vector<DevMat> &mats, uint32_t *d_digests);
    // upper levels of a tree whose 2^log_h leaf digests are already in place (no injection)
    bool commit_tree_levels(uint32_t *d_digests, uint32_t log_h);

    // host_prep[i]: canonical column-major trace of the i-th chip that has preprocessed columns
    bool setup(const MachineDesc *m, const std::vector<ChipRef> &prep_chips, const std::vector<std::vector<uint32_t>> &host_prep,
               ProvingKey *pk);
    void free_key(ProvingKey *pk);
    bool prove_shard(const ProvingKey &pk, const std::vector<ChipTrace> &traces, const std::vector<Fp> &pubs,
                     const StarkConfig &cfg, ShardProof *out, const PermChallenges *global = nullptr,
                     const MainCache *cached = nullptr);
    // phase 1 of a multi-shard proof: K1-K3 of the main traces only -> main_root; with keep != nullptr the
    // LDEs and the tree (tier KEEP_FULL) or the tree alone (KEEP_TREE: the LDEs are the arena's) stay in HBM (from this
    // engine's pool, into *keep) for prove_shard(..., cached = keep).  keep == nullptr is KEEP_NONE.  `admitted`: a
    // lock the caller holds over "how much is free?" and the allocations that follow; it is released once every buffer of
    // the commit is allocated, before the first kernel is launched.
    bool commit_main_root(const ProvingKey &pk, const std::vector<ChipTrace> &traces, Digest *root, MainCache *keep = nullptr,
                          std::unique_lock<std::mutex> *admitted = nullptr, int tier = KEEP_FULL);

    // ---- host side of the K4 running sum, K6, K7 and the K9 grind: prove_shard and the stage entry points (capi.hip) both
    // go through these.  Device words are in Montgomery form.
    // K4 tail: d_totals ([4][2^log_n] row totals) is overwritten by its inclusive prefix sums S; d_phi ([4][2^log_n])
    // receives phi[r] = S[r-1] - r S[n-1] / n and cum_out (device-writable, may be null) the four words of S[n-1].
    // d_scratch holds prefix_sum_scratch_words(4, 2^log_n) words.
    bool logup_running_sum(uint32_t *d_totals, uint32_t *d_scratch, uint32_t *d_phi, uint32_t log_n, uint32_t *cum_out);
    // K6: the weights of the point z over H (2^log_n rows) into d_w ([2^log_n]); *scale = (z^n - 1) / n, the factor that
    // turns the sums of launch_open_columns into p(z) and p(z w_n)
    bool open_point(Fp4 z, uint32_t log_n, Fp4 *d_w, Fp4 *scale);
    // K7: the FRI input d_out ([2^log_m]) of the n_all LDE columns d_cols of one height, the first n_two opened at zeta and
    // zeta w_{m/2}.  apow / d_apow: fri_alpha_powers of at least n_all columns; local [n_all] and next [n_two]: the opened values.
    bool reduced_opening(const uint32_t *const *d_cols, uint32_t n_two, uint32_t n_all, uint32_t log_m, const std::vector<Fp4> &apow,
                         const double *d_apow, const Fp4 *local, const Fp4 *next, Fp4 zeta, Fp4 *d_out);
    // K9: the smallest w such that the permutation of st16 (Montgomery words) with word pos = w has (word 7 mod 2^bits) == 0,
    // in batches of increasing candidates; d_found: one device word of scratch
    bool pow_grind(const uint32_t st16[16], uint32_t pos, uint32_t bits, uint32_t *d_found, uint32_t *witness);

    // ---- host side of one chip's K4 and K5 (prove_shard and dvt_stage_perm / dvt_stage_quotient)
    // the powers base^0 .. base^(n-1) (from_one) or base^1 .. base^n uploaded as Montgomery words and as centred canonical
    // doubles (the operands of the exact FP64 dot products of K4 / K5, f64dot.cuh)
    bool upload_powers(Fp4 base, size_t n, bool from_one, const Fp4 **d_pows, const double **d_pows_f64);
    struct ChipInputs {
        const uint32_t *main, *prep, *pub;   // device, Montgomery: trace (K4) or LDE (K5) columns, public values
        uint32_t log_n;                      // of the trace
        Fp4 perm_alpha;
        const Fp4 *beta_pows;                // upload_powers(beta, .., false)
        const double *beta_f64;
    };
    // K4: d_perm ([4 perm_ext_w][2^log_n]) receives the batch columns and phi, cum_out (device-writable) the four words of the
    // cumulative sum.  d_parts: the part-parallel scratch ([PARTS_MAX][4][2^log_n]) or nullptr for the per-row launch;
    // d_totals [4][2^log_n] and d_scan (prefix_sum_scratch_words(4, 2^log_n)) are scratch.
    bool perm_chip(const ChipDesc &d, const ChipInputs &in, uint32_t *d_parts, uint32_t *d_totals, uint32_t *d_scan, uint32_t *d_perm,
                   uint32_t *cum_out);
    // K5: the quotient chunks d_out ([2][4][2^log_n]) from the LDEs in `in` and perm_lde; cumsum is the chip's cumulative sum.
    // sel_table: read the selectors from this prover's per-height table (else selectors_of_row in the kernel); d_parts: the
    // part-parallel scratch ([PARTS_MAX][2][4][2^log_n]) or nullptr for one launch per part.
    bool quotient_chip(const ChipDesc &d, const ChipInputs &in, const uint32_t *perm_lde, Fp4 cumsum, const Fp4 *alpha_pows,
                       const double *alpha_f64, bool sel_table, uint32_t *d_parts, uint32_t *d_out);

    Arena arena;
    DevPool pool;
    // K5 selector tables, one per trace height this prover has seen ([3][2N] words each, stark.cuh QuotientArgs::sel)
    uint32_t *sel_tables[32] = {};
    // row digests of the shorter matrices of the tree being committed (commit_tree): reused tree after tree on the one stream
    uint32_t *inject_buf = nullptr;
    size_t inject_words = 0;
    const uint32_t *selector_table(const QuotientArgs &qa);

  private:
    char *d_ring = nullptr, *h_ring = nullptr;
    char *h_down = nullptr;  // pinned staging for downloads (roots, opened values, query data): no pageable-memory path
    static constexpr size_t DOWN_BYTES = 16u << 20;   // (every download of a proof goes through this pinned buffer: see the note on pageable memory in capi_internal.h)
    size_t ring_bytes = 0, ring_pos = 0;
    bool fail(const char *fmt, ...);
};

// K7 batching powers alpha^0 .. alpha^n_cols (alpha^n_cols weighs the second point), and the same as [n_cols + 1][4]
// centred canonical doubles: the operand of reduced_opening_kernel
void fri_alpha_powers(Fp4 alpha, size_t n_cols, std::vector<Fp4> *pows, std::vector<double> *pows_f64);
// how many beta and alpha powers a shard of machine m uploads for K4 / K5: the largest arity and folded count of its chips
void challenge_power_counts(const MachineDesc *m, int *n_beta, int *n_alpha);
#endif

}  // namespace dvt
