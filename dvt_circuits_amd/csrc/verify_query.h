// The device path of the verifier's query part (verify_query.hip): the flat description the kernels read, and the batch
// that flattens shard after shard into staging-size chunks.  Private to the library.
#pragma once
#include <array>
#include <string>
#include <utility>
#include <vector>

#include "capi_internal.h"

namespace dvt {
namespace vq {

constexpr uint32_t NONE = 0xffffffffu;
constexpr uint32_t LEAF_SEG = 0x80000000u;   // host-side mark of a segment in the fold kernel's leaf area (cleared at the flush)

// ---- the flat description (device tables; every offset indexes the chunk's word array)
struct Seg { uint32_t off, len; };
struct Sponge { uint32_t seg0, nseg, total, out; };   // `total` words over nseg segments -> 8 canonical words at `out`
struct Chain {
    uint32_t start, depth, leaf;   // start digest, number of levels, leaf index (below 2^depth)
    uint32_t sib;                  // `depth` sibling digests, contiguous
    uint32_t inj;                  // index into the injection table (`depth` entries: a digest offset or NONE), or NONE
    uint32_t root, status, kind;
};
// A tree of a compact shard (DVP2): all its queries walk up together, level by level.  Job i of a level compresses two
// children (each a slot of the level below, or with its flag in `dst` a digest at a word offset: a listed node), then where
// shorter matrices join the digest at `inj`, and writes slot `dst & MP_SLOT` of the level above.
constexpr uint32_t MP_L_WORD = 0x80000000u, MP_R_WORD = 0x40000000u, MP_SLOT = 0xffffu;
constexpr uint32_t MP_MAX_SLOTS = 1024;               // nodes of one level: at most one per query (the reader's cap)
struct MpJob { uint32_t l, r, inj, dst; };
struct MpLevel { uint32_t job0, njobs; };
struct MpCmp { uint32_t a, b, status; };               // two digests that queries on one node must agree on
struct Tree {
    uint32_t leaf0, nleaf;       // word offsets of the leaf digests: leaves[leaf0 ..], ascending leaf index
    uint32_t level0, nlevels;    // its levels, from the leaves' parents to the root
    uint32_t cmp0, ncmp;
    uint32_t root, status;
};
struct MpTables {
    std::vector<Tree> trees;
    std::vector<MpLevel> levels;
    std::vector<MpJob> jobs;
    std::vector<uint32_t> leaves;
    std::vector<MpCmp> cmps;
    uint32_t cap = 0;            // most slots of any level of any tree
    uint64_t perms = 0;
};
struct Col { uint32_t px, loc, nx; };   // the opened row word (relative to the query's section), p(zeta), p(zeta w) or NONE
struct Unit { uint32_t query, h; };
struct Query { uint32_t shard, idx, base, red0, sib0, leaf0, fin, pad; };
struct Shard {
    uint32_t zeta[4], final_poly[4];   // Montgomery words
    uint32_t hmax, apow, beta;         // indices into the F_p^4 table: alpha_f^0.., the fold challenges
    uint32_t slot[25], col0[25], ncol[25], ntwo[25];   // per LDE height: slot of its reduced opening (or NONE), its columns
};
struct Consts { uint32_t gen[25], shift, inv2; };      // two-adic generators, the coset shift, 1/2 (Montgomery)

struct Times {
    double flatten_ms = 0, upload_ms = 0, kernel_ms = 0, download_ms = 0, wait_ms = 0;
    uint64_t perms = 0, launches = 0, chunks = 0;
};

// pinned staging and events of the two chunks in flight: kept by the handle, reused call after call
struct Stage {
    struct Slot {
        char *pinned = nullptr;
        size_t cap = 0;
        hipEvent_t ev[4] = {};
    } slot[2];
    ~Stage();
};

constexpr size_t CHUNK_WORDS = (size_t)4 << 20;   // proof words per chunk (16 MiB of staging)

class Batch {
  public:
    Batch(const Lane &lane, Stage &stage, size_t chunk_words = CHUNK_WORDS);
    ~Batch();
    // Flattens the query sections of one shard (its host part has passed and left ctx; `words` are the shard proof's words
    // and stay valid until finish()).  A query that fails a shape check is answered by verify_query_host here and sends
    // nothing to the device.  A full chunk is uploaded and launched before the shard is added.
    int add(const ShardQueryCtx &ctx, const uint32_t *words, size_t nwords, size_t *shard_slot);
    int finish();                               // launches the last chunk and waits for all of them
    std::string why(size_t shard_slot) const;   // after finish(): "" or the first failure of the shard's queries, the host's text
    Times times;

  private:
    struct QueryResult {
        bool on_device = false;
        std::string host_why;
        uint32_t status0 = 0, n_tree_chains = 0, n_layer_chains = 0;
    };
    struct ShardResult {
        size_t chunk = 0;
        std::vector<QueryResult> queries;
        // a compact shard: answered on the host (a shape check failed), or the status ranges [first, last] of its trees in
        // the order of the wire format (the first n_input of them are input trees) and one final-value byte per query
        bool compact = false, on_device = false;
        std::string host_why;
        std::vector<std::pair<uint32_t, uint32_t>> tree_status;
        uint32_t n_input = 0;
        std::vector<uint32_t> fin;
    };
    struct Chunk {
        size_t words = 0, nshards = 0, leaf_words = 0, digest_words = 0, nred = 0, nstatus = 0;
        uint64_t perms = 0;
        std::vector<std::pair<const uint32_t *, size_t>> src;
        std::vector<Sponge> sponges;
        std::vector<Seg> segs;
        std::vector<Chain> chains;
        std::vector<uint32_t> inj, aux;
        std::vector<Unit> units0;       // (query, number of heights with columns)
        std::vector<Query> queries;
        std::vector<Shard> shards;
        std::vector<Col> cols;
        std::vector<Fp4> ext;
        MpTables mp;
    };
    struct Flight {
        bool active = false;
        void *dev = nullptr;
        size_t nstatus = 0;
        uint8_t *h_status = nullptr;
    };
    void reset_chunk();
    int flush();
    int collect(int slot);

    Lane lane;
    Stage &stage;
    size_t chunk_words;
    Chunk cur;
    Flight fl[2];
    size_t flushed = 0;
    Digest prep_root;
    std::vector<ShardResult> results;
    std::vector<std::vector<uint8_t>> status;   // per chunk, in order
};

// test hooks (dvt_stage_sponge_rows, dvt_stage_verify_paths, dvt_stage_verify_multipath)
int stage_sponge_rows(const Lane &lane, const uint32_t *words, const uint32_t *lens, size_t n, uint32_t *digests);
int stage_verify_paths(const Lane &lane, const dvt_path_chain *chains, size_t n, uint8_t *ok);
int stage_verify_multipath(const Lane &lane, uint32_t depth, const uint32_t *leaf_index, const uint32_t *leaf_digest, size_t n,
                           const uint8_t *inject_at, const uint32_t *inject, const uint32_t *nodes, size_t n_nodes, const uint32_t *root,
                           uint8_t *ok);

}  // namespace vq
}  // namespace dvt
