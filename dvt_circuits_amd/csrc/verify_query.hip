// The query part of verify_shard on the GPU (gfx950): reduced openings, the FRI fold chain, every row / leaf sponge and
// every Merkle path of all queries of a chunk of shards in four launches (the launch count does not depend on the number
// of queries).
//
// Word space.  A chunk's device buffer starts with the prep root of the key and the shards' proof words exactly as they
// arrived (canonical; WordReader::fp has refused everything else), followed by the index tables, the FRI leaf inputs the
// fold kernel writes and the digests the sponge kernel writes.  Every "word offset" below indexes this one array of
// 32-bit words, and every offset, length, depth and index in the tables is computed on the host from the SIZES of the
// parsed, shape-checked structures (vq::Batch::add walks the wire format the way write_shard_proof does): a kernel
// never takes one from a proof word.  Canonical words become doubles (Poseidon2, poseidon2_f64.cuh) or Montgomery
// words (F_p^4, bb.cuh) when they are loaded.
//
// Results.  One status byte per Merkle chain and one per query (the final value), written with plain stores; the host
// scans them in the host verifier's order (shard, query, tree 0..3, layers in order, final value) and reports the first.
// A compact shard (DVP2) has no chain: each of its trees is one job of vq_multipath_kernel, with one status byte per tree and
// one per pair of digests that queries on a common node must agree on, scanned in verify_compact_queries' order (the input
// trees, the FRI layers, then the final values).
#include <algorithm>
#include <chrono>

#include "capi_internal.h"
#include "poseidon2_f64.cuh"
#include "verify_query.h"

namespace dvt {
namespace vq {

// ------------------------------------------------------------------------------------------------ kernels

__device__ __forceinline__ Fp4 load_ext(const uint32_t *w) {   // four canonical words
    Fp4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.c[k] = Fp::from_canonical(w[k]);
    return r;
}
__device__ __forceinline__ Fp4 ext_of(const uint32_t m[4]) {   // four Montgomery words
    Fp4 r;
#pragma unroll
    for (int k = 0; k < 4; k++) r.c[k] = Fp::raw(m[k]);
    return r;
}

// (a) one wave per (query, height that has columns): the two batched sums of reduced(h), scaled and combined
__global__ void __launch_bounds__(256) vq_reduced_kernel(const Unit *units, uint32_t n, const Query *qs, const Shard *shards,
                                                         const Col *cols, const Fp4 *ext, const uint32_t *W, Consts k, Fp4 *red) {
    const uint32_t unit = (blockIdx.x * 256 + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (unit >= n) return;                       // (wave-uniform)
    const Unit u = units[unit];
    const Query q = qs[u.query];
    const Shard &S = shards[q.shard];
    const uint32_t h = u.h, ncol = S.ncol[h];
    const Col *cl = cols + S.col0[h];
    const Fp4 *apow = ext + S.apow;
    Fp4 s_all = Fp4::zero(), s_two = Fp4::zero();
    for (uint32_t c = lane; c < ncol; c += 64) {
        const Col cr = cl[c];
        const Fp4 px = Fp4::from_base(Fp::from_canonical(W[q.base + cr.px]));
        const Fp4 a = apow[c];
        s_all += a * (px - load_ext(W + cr.loc));
        if (cr.nx != NONE) s_two += a * (px - load_ext(W + cr.nx));
    }
    // field addition is exact: any reduction order gives the host's sums
#pragma unroll
    for (int k4 = 0; k4 < 4; k4++)
        for (int off = 32; off > 0; off >>= 1) {
            s_all.c[k4] += Fp::raw(__shfl_xor(s_all.c[k4].v, off));
            s_two.c[k4] += Fp::raw(__shfl_xor(s_two.c[k4].v, off));
        }
    if (lane) return;
    const Fp4 zeta = ext_of(S.zeta);
    const Fp x = Fp::raw(k.shift) * pow(Fp::raw(k.gen[h]), q.idx & ((1u << h) - 1));
    Fp4 r = s_all * inv(Fp4::from_base(x) - zeta);
    if (S.ntwo[h]) r += apow[ncol] * (s_two * inv(Fp4::from_base(x) - zeta * Fp::raw(k.gen[h - 1])));
    red[q.red0 + S.slot[h]] = r;
}

// (b) one thread per query: the fold chain; leaves the ordered pair of every layer as the 8-word leaf input
__global__ void __launch_bounds__(256) vq_fold_kernel(const Query *qs, uint32_t n, const Shard *shards, const uint32_t *aux,
                                                      const Fp4 *ext, const Fp4 *red, uint32_t *W, Consts k, uint8_t *status) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Query q = qs[i];
    const Shard &S = shards[q.shard];
    const uint32_t hmax = S.hmax;
    const Fp inv2 = Fp::raw(k.inv2);
    Fp4 e = S.slot[hmax] != NONE ? red[q.red0 + S.slot[hmax]] : Fp4::zero();
    for (uint32_t l = 0; l + 1 < hmax; l++) {
        const uint32_t lm = hmax - l, half = 1u << (lm - 1);
        const uint32_t j = q.idx & ((1u << lm) - 1), jl = j & (half - 1);
        const Fp4 sib = load_ext(W + aux[q.sib0 + l]);
        const Fp4 a = j < half ? e : sib, b = j < half ? sib : e;
        uint32_t *leaf = W + q.leaf0 + 8 * l;
#pragma unroll
        for (int c = 0; c < 4; c++) { leaf[c] = a.c[c].canonical(); leaf[4 + c] = b.c[c].canonical(); }
        const Fp xinv = inv(pow(Fp::raw(k.gen[lm]), jl));
        e = (a + b) * inv2 + ext[S.beta + l] * ((a - b) * (inv2 * xinv));
        if (S.slot[lm - 1] != NONE) e += red[q.red0 + S.slot[lm - 1]];
    }
    status[q.fin] = e == ext_of(S.final_poly) ? 1 : 0;
}

// (c) one sponge per 16 lanes (lane e holds state element e, lanes 0..7 are the rate): Sponge semantics over the
// concatenation of the job's segments, the ragged last block overwriting only what it has
__global__ void __launch_bounds__(256) vq_sponge_kernel(const Sponge *jobs, uint32_t n, const Seg *segs, uint32_t *W) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x, e = threadIdx.x & 15, job = t >> 4;
    const bool live = job < n;
    const p2f::CoopConsts k = p2f::coop_consts(e);
    Sponge jb = {0, 0, 0, 0};
    if (live) jb = jobs[job];
    double h = 0.0;
    // this lane's place in the segment list: segment s covers stream positions [cs, cs + slen)
    uint32_t s = jb.seg0, cs = 0, slen = 0, soff = 0;
    if (jb.total) { slen = segs[s].len; soff = segs[s].off; }
    for (uint32_t g = 0; g < jb.total; g += 8) {       // (the trip count is uniform over the 16 lanes of a row)
        const uint32_t pos = g + e;
        if (e < 8 && pos < jb.total) {
            while (pos - cs >= slen) { cs += slen; s++; slen = segs[s].len; soff = segs[s].off; }   // (total = sum of the lengths)
            h = p2f::from_canonical(W[soff + (pos - cs)]);
        }
        h = p2f::coop_permute(h, k);
    }
    if (live && e < 8) W[jb.out + e] = p2f::to_canonical(h);
}

// (d) one Merkle chain per 16 lanes: natural-order sides, one more compression where shorter matrices join, compare with
// the root.  Rows of one wave run different trip counts; a row stays together.
__global__ void __launch_bounds__(256) vq_path_kernel(const Chain *chains, uint32_t n, const uint32_t *inj, const uint32_t *W,
                                                      uint8_t *status) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x, e = threadIdx.x & 15, row = t >> 4;
    const bool live = row < n;
    const p2f::CoopConsts k = p2f::coop_consts(e);
    Chain c = {0, 0, 0, 0, NONE, 0, 0, 0};
    if (live) c = chains[row];
    double s = live ? p2f::from_canonical(W[c.start + (e & 7)]) : 0.0;
    uint32_t j = c.leaf;
    for (uint32_t l = 0; l < c.depth; l++) {
        const uint32_t half = 1u << (c.depth - l - 1);
        const double sib = p2f::from_canonical(W[c.sib + 8 * l + (e & 7)]);
        const double up = p2f::dpp_mov<p2f::DPP_ROW_ROR + 8>(s);     // lanes 8..15 see the node of lanes 0..7
        s = j < half ? (e < 8 ? s : sib) : (e < 8 ? sib : up);
        s = p2f::coop_permute(s, k);
        j &= half - 1;
        const uint32_t io = c.inj != NONE ? inj[c.inj + l] : NONE;   // (uniform over the row)
        if (io != NONE) {
            const double hs = p2f::from_canonical(W[io + (e & 7)]);
            s = e < 8 ? s : hs;
            s = p2f::coop_permute(s, k);
        }
    }
    const bool bad = live && e < 8 && p2f::to_canonical(s) != W[c.root + e];
    const unsigned long long m = __ballot(bad);
    if (live && e == 0) status[c.status] = ((m >> (threadIdx.x & 48)) & 0xffffu) ? 0 : 1;
}

// (e) one workgroup per tree of a compact shard: all queries of the tree walk up together.  The nodes of the current level
// and of the one above live in LDS as canonical words ([2][cap][8], cap <= MP_MAX_SLOTS: 64 KB at the reader's 1024
// queries); one compression per 16-lane row as in the path kernel, rows looping over the level's jobs; one barrier per
// level, whose trip counts come from the tree's tables and are uniform over the workgroup.  No workgroup waits for another.
__global__ void __launch_bounds__(256) vq_multipath_kernel(const Tree *trees, const MpLevel *levels, const MpJob *jobs, const uint32_t *leaves,
                                                           const MpCmp *cmps, uint32_t cap, const uint32_t *W, uint8_t *status) {
    extern __shared__ uint32_t mp_nodes[];   // [2][cap][8]: at most 64 KB, which a launch may ask for without any function attribute
    const Tree T = trees[blockIdx.x];
    const uint32_t tid = threadIdx.x, e = tid & 15, row = tid >> 4;
    const p2f::CoopConsts k = p2f::coop_consts(e);
    for (uint32_t i = tid; i < T.ncmp; i += 256) {
        const MpCmp c = cmps[T.cmp0 + i];
        bool same = true;
        for (int w = 0; w < 8; w++) same &= W[c.a + w] == W[c.b + w];
        status[c.status] = same ? 1 : 0;
    }
    uint32_t *cur = mp_nodes, *up = mp_nodes + 8 * (size_t)cap;
    for (uint32_t i = tid; i < 8 * T.nleaf; i += 256) cur[i] = W[leaves[T.leaf0 + (i >> 3)] + (i & 7)];
    __syncthreads();
    for (uint32_t lv = 0; lv < T.nlevels; lv++) {
        const MpLevel L = levels[T.level0 + lv];
        for (uint32_t base = 0; base < L.njobs; base += 16) {
            const bool live = base + row < L.njobs;        // (uniform over the row; a dead row permutes zeros)
            MpJob jb = {0, 0, NONE, 0};
            if (live) jb = jobs[L.job0 + base + row];
            const uint32_t src = e < 8 ? jb.l : jb.r;
            const bool word = jb.dst & (e < 8 ? MP_L_WORD : MP_R_WORD);
            double s = live ? p2f::from_canonical(word ? W[src + (e & 7)] : cur[8 * src + (e & 7)]) : 0.0;
            s = p2f::coop_permute(s, k);
            if (jb.inj != NONE) {
                const double hs = p2f::from_canonical(W[jb.inj + (e & 7)]);
                s = e < 8 ? s : hs;
                s = p2f::coop_permute(s, k);
            }
            if (live && e < 8) up[8 * (jb.dst & MP_SLOT) + e] = p2f::to_canonical(s);
        }
        __syncthreads();
        uint32_t *t = cur; cur = up; up = t;
    }
    if (tid == 0) {
        bool same = T.nleaf != 0;
        for (int w = 0; w < 8; w++) same &= cur[w] == W[T.root + w];
        status[T.status] = same ? 1 : 0;
    }
}

static_assert(2 * 32 * (size_t)MP_MAX_SLOTS <= 65536 && MP_MAX_SLOTS >= MAX_QUERIES && MP_MAX_SLOTS <= MP_SLOT + 1,
              "the two levels of a tree fit the dynamic LDS of a plain launch, and a level has at most one node per query");

// One tree of `depth` levels into the tables, from the shard's sources (one plan for all its trees).  digest_at(lh, q): the
// word offset of query q's digest of height lh, or NONE where the tree has no rows of that height; listed0: the word offset
// of the tree's first listed node; statuses are numbered from *nstatus on.  Returns the tree's status range [first, last]:
// its comparisons, then the walk.
template <class F>
static std::pair<uint32_t, uint32_t> emit_tree(MpTables &mp, const TreeSources &ts, uint32_t depth, F digest_at, uint32_t listed0, uint32_t root,
                                               size_t *nstatus) {
    const MultipathPlan &pl = ts.plan;
    const uint32_t base = pl.base[depth];
    Tree T = {};
    const uint32_t first = (uint32_t)*nstatus;
    T.cmp0 = (uint32_t)mp.cmps.size();
    for (uint32_t lh = 0; lh <= depth; lh++) {
        if (ts.dups[lh].empty() || digest_at(lh, 0) == NONE) continue;   // (a tree has rows of a height for every query or for none)
        for (auto &d : ts.dups[lh]) mp.cmps.push_back({digest_at(lh, d[0]), digest_at(lh, d[1]), (uint32_t)(*nstatus)++});
    }
    T.ncmp = (uint32_t)mp.cmps.size() - T.cmp0;
    T.leaf0 = (uint32_t)mp.leaves.size();
    T.nleaf = (uint32_t)pl.keys[depth].size();
    for (uint32_t i = 0; i < T.nleaf; i++) mp.leaves.push_back(digest_at(depth, ts.first[depth][i]));
    mp.cap = std::max(mp.cap, T.nleaf);
    T.level0 = (uint32_t)mp.levels.size();
    T.nlevels = depth;
    for (uint32_t s = depth; s >= 1; s--) {
        const auto &jobs = pl.levels[pl.depth - s];
        mp.levels.push_back({(uint32_t)mp.jobs.size(), (uint32_t)jobs.size()});
        const bool joins = digest_at(s - 1, 0) != NONE;
        for (size_t i = 0; i < jobs.size(); i++) {
            const MultipathJob &jb = jobs[i];
            MpJob out = {jb.l, jb.r, joins ? digest_at(s - 1, ts.first[s - 1][i]) : NONE, (uint32_t)i};
            if (jb.l & MP_LISTED) { out.l = listed0 + 8 * ((jb.l & ~MP_LISTED) - base); out.dst |= MP_L_WORD; }
            if (jb.r & MP_LISTED) { out.r = listed0 + 8 * ((jb.r & ~MP_LISTED) - base); out.dst |= MP_R_WORD; }
            mp.jobs.push_back(out);
        }
        mp.perms += jobs.size() * (1 + joins);
    }
    T.root = root;
    T.status = (uint32_t)(*nstatus)++;
    mp.trees.push_back(T);
    return {first, T.status};
}

static Consts make_consts() {
    Consts k;
    for (uint32_t h = 0; h < 25; h++) k.gen[h] = two_adic_generator(h).v;
    k.shift = Fp::from_canonical(COSET_SHIFT).v;
    k.inv2 = inv(Fp::two()).v;
    return k;
}
static const Consts &consts() {
    static const Consts k = make_consts();
    return k;
}

// ------------------------------------------------------------------------------------------------ the host side

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

Stage::~Stage() {
    for (auto &s : slot) {
        if (s.pinned) (void)hipHostFree(s.pinned);
        for (auto ev : s.ev)
            if (ev) (void)hipEventDestroy(ev);
    }
}

Batch::Batch(const Lane &lane, Stage &stage, size_t chunk_words) : lane(lane), stage(stage), chunk_words(chunk_words) { reset_chunk(); }
Batch::~Batch() {
    // (an error path: nothing of this call stays in flight or out of the pool)
    for (int s = 0; s < 2; s++)
        if (fl[s].active) {
            (void)hipStreamSynchronize(lane.eng.stream);
            lane.eng.pool.free(fl[s].dev);
            fl[s].active = false;
        }
}

void Batch::reset_chunk() {
    cur = Chunk{};
    cur.words = 8;   // the key's prep root
}

template <class T> static size_t put(std::vector<uint8_t> &blob, const std::vector<T> &v) {
    const size_t at = (blob.size() + 15) & ~(size_t)15;
    blob.resize(at + v.size() * sizeof(T));
    if (!v.empty()) memcpy(blob.data() + at, v.data(), v.size() * sizeof(T));
    return at;
}

int Batch::add(const ShardQueryCtx &ctx, const uint32_t *words, size_t nwords, size_t *shard_slot) {
    if (cur.nshards && cur.words + nwords > chunk_words)
        if (int rc = flush()) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    const ShardProof &pf = *ctx.pf;
    Chunk &c = cur;
    if (c.nshards == 0) prep_root = *ctx.roots[0];
    const uint32_t sbase = (uint32_t)c.words;     // word offset of this shard's first word
    c.src.push_back({words, nwords});
    c.words += nwords;
    c.nshards++;
    *shard_slot = results.size();
    results.push_back({});
    ShardResult &res = results.back();

    // ---- offsets of the head of the proof, from the sizes of the parsed vectors (write_shard_proof's order)
    size_t off = 1;
    const uint32_t root_off[4] = {0, sbase + 1, sbase + 9, sbase + 17};
    off += 24;
    off += 1 + pf.public_values.size();
    off += 1;
    std::vector<std::array<uint32_t, 7>> opened(pf.chips.size());   // prep_l, prep_n, main_l, main_n, perm_l, perm_n, quot
    for (size_t i = 0; i < pf.chips.size(); i++) {
        const ChipOpening &o = pf.chips[i];
        off += 6;
        int k = 0;
        for (auto *v : {&o.prep_l, &o.prep_n, &o.main_l, &o.main_n, &o.perm_l, &o.perm_n, &o.quot}) {
            opened[i][k++] = sbase + (uint32_t)(off + 1);
            off += 1 + 4 * v->size();
        }
    }
    const uint32_t fri_root0 = sbase + (uint32_t)(off + 1);
    off += 1 + 8 * pf.fri_roots.size();
    off += 4 + 1 + 1;   // final_poly, pow_witness, the query count

    // ---- the shard's constants and column maps
    const uint32_t hmax = ctx.hmax;
    Shard S = {};
    for (int k = 0; k < 4; k++) { S.zeta[k] = ctx.zeta.c[k].v; S.final_poly[k] = pf.final_poly.c[k].v; }
    S.hmax = hmax;
    S.apow = (uint32_t)c.ext.size();
    c.ext.insert(c.ext.end(), ctx.apow.begin(), ctx.apow.end());
    S.beta = (uint32_t)c.ext.size();
    c.ext.insert(c.ext.end(), ctx.fold_betas.begin(), ctx.fold_betas.end());
    // where row (tree, mat) starts inside a query's section, and the section's layout
    uint32_t row_rel[4] = {}, path_rel[4] = {};
    std::vector<uint32_t> mat_rel[4];
    size_t rel = 0;
    for (int t = 0; t < 4; t++) {
        rel += 1;
        row_rel[t] = (uint32_t)rel;
        for (auto &mt : ctx.shapes[t].mats) {
            mat_rel[t].push_back((uint32_t)(rel + 1));
            rel += 1 + mt.first;
        }
        if (pf.compact) continue;   // (no path, not even its length)
        path_rel[t] = (uint32_t)(rel + 1);
        rel += 1 + 8 * (size_t)(ctx.shapes[t].mats.empty() ? 0 : ctx.shapes[t].log_h);
    }
    rel += 1;   // the layer count
    std::vector<uint32_t> sib_rel(hmax - 1), lpath_rel(hmax - 1);
    for (uint32_t k = 0; k + 1 < hmax; k++) {
        sib_rel[k] = (uint32_t)rel;
        lpath_rel[k] = (uint32_t)(rel + 5);
        rel += pf.compact ? 4 : 4 + 1 + 8 * (size_t)(hmax - k - 1);
    }
    const size_t qwords = rel;   // words of a query section that passes the shape checks
    uint32_t nslot = 0;
    for (uint32_t h = 0; h < 25; h++) S.slot[h] = NONE;
    for (uint32_t h = 1; h <= hmax; h++) {
        const auto &cols = ctx.cols_by_h[h];
        S.col0[h] = (uint32_t)c.cols.size();
        S.ncol[h] = (uint32_t)cols.size();
        S.ntwo[h] = ctx.n_two_by_h[h];
        if (cols.empty()) continue;
        S.slot[h] = nslot++;
        for (auto &r : cols) {
            const auto &op = opened[r.chip_pos];
            const uint32_t loc = r.tree == 0 ? op[0] : r.tree == 1 ? op[2] : r.tree == 2 ? op[4] : op[6];
            const uint32_t nx = r.tree == 0 ? op[1] : r.tree == 1 ? op[3] : r.tree == 2 ? op[5] : NONE;
            c.cols.push_back({mat_rel[r.tree][r.mat] + (uint32_t)r.col, loc + 4 * (uint32_t)r.col, nx == NONE ? NONE : nx + 4 * (uint32_t)r.col});
        }
    }
    const uint32_t shard_index = (uint32_t)c.shards.size();
    c.shards.push_back(S);

    // ---- the queries
    res.chunk = flushed;
    res.queries.resize(pf.queries.size());
    res.compact = pf.compact;
    if (pf.compact && !compact_shape_ok(ctx)) {
        // nothing of this shard's queries goes to the device: the host names its first failure
        res.host_why = verify_compact_queries(ctx);
        times.flatten_ms += ms_since(t0);
        return DVT_OK;
    }
    res.on_device = pf.compact;
    // a compact shard: where each query's digests will be (relative to the digest area), for the trees below
    std::vector<std::vector<uint32_t>> row_dig[4];
    std::vector<std::vector<uint32_t>> leaf_dig(pf.compact ? pf.queries.size() : 0);
    for (uint32_t qi = 0; qi < pf.queries.size(); qi++) {
        QueryResult &qr = res.queries[qi];
        if (!pf.compact && !query_shape_ok(ctx, qi)) {
            // nothing of this query goes to the device: the host names its first failure (a shape, or a hash before it)
            qr.host_why = verify_query_host(ctx, qi);
            qr.on_device = false;
            const QueryProof &q = pf.queries[qi];
            for (int t = 0; t < 4; t++) {
                off += 1;
                for (auto &row : q.trees[t].rows) off += 1 + row.size();
                off += 1 + 8 * q.trees[t].path.size();
            }
            off += 1;
            for (auto &l : q.layers) off += 4 + 1 + 8 * l.path.size();
            continue;
        }
        const uint32_t qbase = sbase + (uint32_t)off;
        off += qwords;
        const uint32_t idx = ctx.idx[qi];
        Query Q = {};
        Q.shard = shard_index;
        Q.idx = idx;
        Q.base = qbase;
        Q.red0 = (uint32_t)c.nred;
        c.nred += nslot;
        Q.sib0 = (uint32_t)c.aux.size();
        for (uint32_t k = 0; k + 1 < hmax; k++) c.aux.push_back(qbase + sib_rel[k]);
        Q.leaf0 = (uint32_t)c.leaf_words;    // (relative to the scratch area: made absolute at the flush)
        c.leaf_words += 8 * (size_t)(hmax - 1);
        qr.on_device = true;
        qr.status0 = (uint32_t)c.nstatus;
        // input trees: a sponge per height of the tree, a chain from the tallest
        for (int t = 0; t < 4; t++) {
            const TreeShape &sh = ctx.shapes[t];
            if (sh.mats.empty()) continue;
            std::vector<uint32_t> dig(sh.log_h + 1, NONE);   // digest of the rows of height lh (relative to the digest area)
            for (uint32_t lh = 0; lh <= sh.log_h; lh++) {
                Sponge jb = {(uint32_t)c.segs.size(), 0, 0, 0};
                for (size_t i = 0; i < sh.mats.size(); i++)
                    if (sh.mats[i].second == lh) {
                        c.segs.push_back({qbase + mat_rel[t][i], sh.mats[i].first});
                        jb.nseg++;
                        jb.total += sh.mats[i].first;
                    }
                if (!jb.nseg) continue;
                dig[lh] = jb.out = (uint32_t)c.digest_words;
                c.digest_words += 8;
                c.sponges.push_back(jb);
                c.perms += (jb.total + 7) / 8;
            }
            if (pf.compact) { row_dig[t].push_back(dig); continue; }
            Chain ch = {dig[sh.log_h], sh.log_h, idx & ((1u << sh.log_h) - 1), qbase + path_rel[t], (uint32_t)c.inj.size(), root_off[t],
                        (uint32_t)c.nstatus++, 1};
            for (uint32_t s = sh.log_h; s >= 1; s--) {
                c.inj.push_back(dig[s - 1]);
                c.perms += 1 + (dig[s - 1] != NONE);
            }
            c.chains.push_back(ch);
            qr.n_tree_chains++;
        }
        // FRI layers: the leaf sponge of the fold kernel's pair, a chain to the layer's root
        for (uint32_t k = 0; k + 1 < hmax; k++) {
            const uint32_t lm = hmax - k, half = 1u << (lm - 1);
            Sponge jb = {(uint32_t)c.segs.size(), 1, 8, (uint32_t)c.digest_words};
            c.segs.push_back({Q.leaf0 + 8 * k, 8 | LEAF_SEG});
            c.digest_words += 8;
            c.sponges.push_back(jb);
            c.perms += 1;
            if (pf.compact) { leaf_dig[qi].push_back(jb.out); continue; }
            Chain ch = {jb.out, lm - 1, (idx & ((1u << lm) - 1)) & (half - 1), qbase + lpath_rel[k], NONE, fri_root0 + 8 * k,
                        (uint32_t)c.nstatus++, 0};
            c.chains.push_back(ch);
            c.perms += lm - 1;
        }
        qr.n_layer_chains = pf.compact ? 0 : hmax - 1;
        Q.fin = (uint32_t)c.nstatus++;
        if (pf.compact) res.fin.push_back(Q.fin);
        c.units0.push_back({(uint32_t)c.queries.size(), nslot});
        c.queries.push_back(Q);
    }
    if (pf.compact) {
        // the node lists follow the queries: a count and its digests per tree, in the order the trees are walked here
        for (int t = 0; t < 4; t++) {
            const TreeShape &sh = ctx.shapes[t];
            const uint32_t listed0 = sbase + (uint32_t)(off + 1);
            off += 1 + 8 * pf.node_lists[t].size();
            if (sh.mats.empty()) continue;
            res.tree_status.push_back(emit_tree(c.mp, ctx.paths, sh.log_h, [&](uint32_t lh, uint32_t q) { return row_dig[t][q][lh]; }, listed0, root_off[t], &c.nstatus));
            res.n_input++;
        }
        for (uint32_t k = 0; k + 1 < hmax; k++) {
            const uint32_t depth = hmax - k - 1, listed0 = sbase + (uint32_t)(off + 1);
            off += 1 + 8 * pf.node_lists[4 + k].size();
            res.tree_status.push_back(emit_tree(c.mp, ctx.paths, depth, [&](uint32_t lh, uint32_t q) { return lh == depth ? leaf_dig[q][k] : NONE; }, listed0,
                                                fri_root0 + 8 * k, &c.nstatus));
        }
    }
    times.flatten_ms += ms_since(t0);
    if (off != nwords) return fail(lane.err, DVT_ERR_DEVICE, "internal: the layout walk of a shard proof ended at word %zu of %zu", off, nwords);
    return DVT_OK;
}

int Batch::flush() {
    Chunk &c = cur;
    if (!c.nshards) return DVT_OK;
    const auto t0 = std::chrono::steady_clock::now();
    Engine &e = lane.eng;
    const int si = flushed & 1;
    if (int rc = collect(si)) return rc;     // the slot's previous chunk, two flushes ago
    Stage::Slot &slot = stage.slot[si];
    // ---- finish the tables: absolute scratch offsets, units per height, longest sponge first
    std::vector<Unit> units;
    for (auto &u : c.units0) {
        const Shard &S = c.shards[c.queries[u.query].shard];
        for (uint32_t h = 1; h <= S.hmax; h++)
            if (S.slot[h] != NONE) units.push_back({u.query, h});
    }
    {   // counting sort by permutation count, descending (workgroups are dispatched in order)
        uint32_t mx = 0;
        for (auto &j : c.sponges) mx = std::max(mx, (j.total + 7) / 8);
        std::vector<uint32_t> start(mx + 2, 0);
        for (auto &j : c.sponges) start[mx - (j.total + 7) / 8 + 1]++;
        for (uint32_t i = 1; i < start.size(); i++) start[i] += start[i - 1];
        std::vector<Sponge> sorted(c.sponges.size());
        for (auto &j : c.sponges) sorted[start[mx - (j.total + 7) / 8]++] = j;
        c.sponges.swap(sorted);
    }
    std::vector<uint8_t> blob;
    const size_t at_sp = put(blob, c.sponges), at_seg = put(blob, c.segs), at_ch = put(blob, c.chains), at_inj = put(blob, c.inj),
                 at_aux = put(blob, c.aux), at_un = put(blob, units), at_q = put(blob, c.queries), at_sh = put(blob, c.shards),
                 at_col = put(blob, c.cols), at_ext = put(blob, c.ext), at_tr = put(blob, c.mp.trees), at_lv = put(blob, c.mp.levels),
                 at_mj = put(blob, c.mp.jobs), at_lf = put(blob, c.mp.leaves), at_cm = put(blob, c.mp.cmps);
    const size_t up_words = (c.words + 3) & ~(size_t)3;
    const size_t tab_bytes = (blob.size() + 15) & ~(size_t)15;
    const size_t leaf0 = up_words + tab_bytes / 4;                 // word offsets of the scratch areas
    const size_t dig0 = leaf0 + ((c.leaf_words + 3) & ~(size_t)3);
    const size_t red0 = dig0 + c.digest_words;                     // (Fp4: 16-byte aligned, every area above is a multiple of 4 words)
    const size_t st0 = red0 + 4 * c.nred;
    const size_t total_bytes = st0 * 4 + ((c.nstatus + 15) & ~(size_t)15);
    if (st0 >= ((size_t)1 << 32)) return fail(lane.err, DVT_ERR_INPUT, "a verify chunk of %zu words exceeds the 32-bit word space", st0);
    // the offsets that were relative to a scratch area
    uint8_t *tb = blob.data();
    Sponge *sp = reinterpret_cast<Sponge *>(tb + at_sp);
    Seg *sg = reinterpret_cast<Seg *>(tb + at_seg);
    Chain *ch = reinterpret_cast<Chain *>(tb + at_ch);
    uint32_t *ij = reinterpret_cast<uint32_t *>(tb + at_inj);
    Query *qs = reinterpret_cast<Query *>(tb + at_q);
    for (size_t i = 0; i < c.sponges.size(); i++) sp[i].out += (uint32_t)dig0;
    for (size_t i = 0; i < c.segs.size(); i++)
        if (sg[i].len & LEAF_SEG) { sg[i].len &= ~LEAF_SEG; sg[i].off += (uint32_t)leaf0; }
    for (size_t i = 0; i < c.chains.size(); i++) ch[i].start += (uint32_t)dig0;
    for (size_t i = 0; i < c.inj.size(); i++)
        if (ij[i] != NONE) ij[i] += (uint32_t)dig0;
    for (size_t i = 0; i < c.queries.size(); i++) qs[i].leaf0 += (uint32_t)leaf0;
    {   // the trees of compact shards: leaves, joining digests and compared digests are in the digest area
        MpJob *mj = reinterpret_cast<MpJob *>(tb + at_mj);
        uint32_t *lf = reinterpret_cast<uint32_t *>(tb + at_lf);
        MpCmp *cm = reinterpret_cast<MpCmp *>(tb + at_cm);
        for (size_t i = 0; i < c.mp.jobs.size(); i++)
            if (mj[i].inj != NONE) mj[i].inj += (uint32_t)dig0;
        for (size_t i = 0; i < c.mp.leaves.size(); i++) lf[i] += (uint32_t)dig0;
        for (size_t i = 0; i < c.mp.cmps.size(); i++) { cm[i].a += (uint32_t)dig0; cm[i].b += (uint32_t)dig0; }
    }

    // ---- pinned staging: the words as they are, then the tables; the status bytes come back behind them
    const size_t up_bytes = up_words * 4 + tab_bytes;
    const size_t need = up_bytes + ((c.nstatus + 15) & ~(size_t)15);
    if (slot.cap < need) {
        if (slot.pinned) (void)hipHostFree(slot.pinned);
        slot.pinned = nullptr;
        slot.cap = 0;
        size_t cap = (size_t)1 << 20;
        while (cap < need) cap <<= 1;
        HIP_TRY(lane.err, hipHostMalloc(reinterpret_cast<void **>(&slot.pinned), cap, hipHostMallocDefault));
        slot.cap = cap;
    }
    for (auto &ev : slot.ev)
        if (!ev) HIP_TRY(lane.err, hipEventCreate(&ev));
    uint32_t *hw = reinterpret_cast<uint32_t *>(slot.pinned);
    for (int k = 0; k < 8; k++) hw[k] = prep_root.d[k].canonical();
    size_t w = 8;
    for (auto &s : c.src) { memcpy(hw + w, s.first, s.second * 4); w += s.second; }
    for (; w < up_words; w++) hw[w] = 0;
    memcpy(slot.pinned + up_words * 4, blob.data(), blob.size());

    Flight &f = fl[si];
    HIP_TRY(lane.err, e.pool.alloc_bytes(&f.dev, total_bytes));
    f.active = true;
    f.nstatus = c.nstatus;
    f.h_status = reinterpret_cast<uint8_t *>(slot.pinned + up_bytes);
    uint32_t *W = static_cast<uint32_t *>(f.dev);
    const uint8_t *T = reinterpret_cast<const uint8_t *>(W + up_words);
    uint8_t *d_status = reinterpret_cast<uint8_t *>(W + st0);
    Fp4 *d_red = reinterpret_cast<Fp4 *>(W + red0);
    const Fp4 *d_ext = reinterpret_cast<const Fp4 *>(T + at_ext);
    const Query *d_q = reinterpret_cast<const Query *>(T + at_q);
    const Shard *d_sh = reinterpret_cast<const Shard *>(T + at_sh);
    const hipStream_t st = e.stream;
    times.flatten_ms += ms_since(t0);
    HIP_TRY(lane.err, hipEventRecord(slot.ev[0], st));
    HIP_TRY(lane.err, hipMemcpyAsync(W, slot.pinned, up_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(lane.err, hipMemsetAsync(d_status, 0, c.nstatus, st));
    HIP_TRY(lane.err, hipEventRecord(slot.ev[1], st));
    const uint32_t nq = (uint32_t)c.queries.size(), nu = (uint32_t)units.size(), ns = (uint32_t)c.sponges.size(), nc = (uint32_t)c.chains.size();
    if (nu) vq_reduced_kernel<<<(nu + 3) / 4, 256, 0, st>>>(reinterpret_cast<const Unit *>(T + at_un), nu, d_q, d_sh, reinterpret_cast<const Col *>(T + at_col), d_ext, W, consts(), d_red);
    if (nq) vq_fold_kernel<<<(nq + 255) / 256, 256, 0, st>>>(d_q, nq, d_sh, reinterpret_cast<const uint32_t *>(T + at_aux), d_ext, d_red, W, consts(), d_status);
    if (ns) vq_sponge_kernel<<<(ns + 15) / 16, 256, 0, st>>>(reinterpret_cast<const Sponge *>(T + at_sp), ns, reinterpret_cast<const Seg *>(T + at_seg), W);
    if (nc) vq_path_kernel<<<(nc + 15) / 16, 256, 0, st>>>(reinterpret_cast<const Chain *>(T + at_ch), nc, reinterpret_cast<const uint32_t *>(T + at_inj), W, d_status);
    const uint32_t nt = (uint32_t)c.mp.trees.size();
    if (nt)
        vq_multipath_kernel<<<nt, 256, 2 * 32 * (size_t)c.mp.cap, st>>>(reinterpret_cast<const Tree *>(T + at_tr), reinterpret_cast<const MpLevel *>(T + at_lv),
                                                                       reinterpret_cast<const MpJob *>(T + at_mj), reinterpret_cast<const uint32_t *>(T + at_lf),
                                                                       reinterpret_cast<const MpCmp *>(T + at_cm), c.mp.cap, W, d_status);
    HIP_TRY(lane.err, hipGetLastError());
    HIP_TRY(lane.err, hipEventRecord(slot.ev[2], st));
    if (c.nstatus) HIP_TRY(lane.err, hipMemcpyAsync(f.h_status, d_status, c.nstatus, hipMemcpyDeviceToHost, st));
    HIP_TRY(lane.err, hipEventRecord(slot.ev[3], st));
    times.perms += c.perms + c.mp.perms;
    times.launches += (nu != 0) + (nq != 0) + (ns != 0) + (nc != 0) + (nt != 0);
    times.chunks++;
    flushed++;
    reset_chunk();
    return DVT_OK;
}

// waits for the chunk in flight on slot si, keeps its status bytes and gives its device buffer back
int Batch::collect(int si) {
    Flight &f = fl[si];
    if (!f.active) return DVT_OK;
    Stage::Slot &slot = stage.slot[si];
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t err = hipEventSynchronize(slot.ev[3]);
    times.wait_ms += ms_since(t0);
    lane.eng.pool.free(f.dev);
    f.active = false;
    HIP_TRY(lane.err, err);
    float a = 0, b = 0, d = 0;
    (void)hipEventElapsedTime(&a, slot.ev[0], slot.ev[1]);
    (void)hipEventElapsedTime(&b, slot.ev[1], slot.ev[2]);
    (void)hipEventElapsedTime(&d, slot.ev[2], slot.ev[3]);
    times.upload_ms += a; times.kernel_ms += b; times.download_ms += d;
    status.emplace_back(f.h_status, f.h_status + f.nstatus);
    return DVT_OK;
}

int Batch::finish() {
    if (int rc = flush()) return rc;
    // chunks complete in stream order: the older slot first
    if (int rc = collect(flushed & 1)) return rc;
    return collect((flushed & 1) ^ 1);
}

std::string Batch::why(size_t shard_slot) const {
    const ShardResult &r = results[shard_slot];
    if (r.compact) {
        if (!r.on_device) return r.host_why;
        const uint8_t *s = status[r.chunk].data();
        for (size_t t = 0; t < r.tree_status.size(); t++)
            for (uint32_t i = r.tree_status[t].first; i <= r.tree_status[t].second; i++)
                if (!s[i]) return t < r.n_input ? "Merkle opening rejected (input tree)" : "Merkle opening rejected (FRI layer)";
        for (uint32_t f : r.fin)
            if (!s[f]) return "FRI final value mismatch";
        return "";
    }
    for (auto &q : r.queries) {
        if (!q.on_device) {
            if (!q.host_why.empty()) return q.host_why;
            continue;
        }
        const uint8_t *s = status[r.chunk].data() + q.status0;
        for (uint32_t i = 0; i < q.n_tree_chains; i++)
            if (!s[i]) return "Merkle opening rejected (input tree)";
        for (uint32_t i = 0; i < q.n_layer_chains; i++)
            if (!s[q.n_tree_chains + i]) return "Merkle opening rejected (FRI layer)";
        if (!s[q.n_tree_chains + q.n_layer_chains]) return "FRI final value mismatch";
    }
    return "";
}

// ------------------------------------------------------------------------------------------------ the stage hooks

int stage_sponge_rows(const Lane &lane, const uint32_t *words, const uint32_t *lens, size_t n, uint32_t *digests) {
    Engine &e = lane.eng;
    std::vector<Sponge> jobs(n);
    std::vector<Seg> segs(n);
    size_t total = 0;
    for (size_t i = 0; i < n; i++) total += lens[i];
    const size_t w0 = (total + 3) & ~(size_t)3;
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        segs[i] = {(uint32_t)at, lens[i]};
        jobs[i] = {(uint32_t)i, 1, lens[i], (uint32_t)(w0 + 8 * i)};
        at += lens[i];
    }
    for (size_t i = 0; i < total; i++)
        if (words[i] >= P) return fail(lane.err, DVT_ERR_INPUT, "word %zu is not canonical", i);
    StageBuf buf{e.pool}, tab{e.pool};
    HIP_TRY(lane.err, e.pool.alloc_bytes(&buf.ptr, (w0 + 8 * n) * 4));
    HIP_TRY(lane.err, e.pool.alloc_bytes(&tab.ptr, n * (sizeof(Sponge) + sizeof(Seg))));
    uint32_t *W = static_cast<uint32_t *>(buf.ptr);
    Sponge *d_jobs = static_cast<Sponge *>(tab.ptr);
    Seg *d_segs = reinterpret_cast<Seg *>(d_jobs + n);
    // (a test hook: synchronous copies, which stage pageable memory inside the runtime)
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    if (total) HIP_TRY(lane.err, hipMemcpy(W, words, total * 4, hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemcpy(d_jobs, jobs.data(), n * sizeof(Sponge), hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemcpy(d_segs, segs.data(), n * sizeof(Seg), hipMemcpyHostToDevice));
    vq_sponge_kernel<<<(unsigned)((n + 15) / 16), 256, 0, e.stream>>>(d_jobs, (uint32_t)n, d_segs, W);
    HIP_TRY(lane.err, hipGetLastError());
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    HIP_TRY(lane.err, hipMemcpy(digests, W + w0, n * 32, hipMemcpyDeviceToHost));
    return DVT_OK;
}

int stage_verify_paths(const Lane &lane, const dvt_path_chain *chains, size_t n, uint8_t *ok) {
    Engine &e = lane.eng;
    std::vector<uint32_t> w, inj;
    std::vector<Chain> cs(n);
    auto digest = [&](const uint32_t *d) {
        const uint32_t at = (uint32_t)w.size();
        w.insert(w.end(), d, d + 8);
        return at;
    };
    for (size_t i = 0; i < n; i++) {
        const dvt_path_chain &c = chains[i];
        if (c.depth > 30 || (c.depth && !c.siblings)) return fail(lane.err, DVT_ERR_INPUT, "chain %zu: bad depth or null siblings", i);
        Chain ch = {digest(c.start), c.depth, c.leaf & ((1u << c.depth) - 1), (uint32_t)w.size(), NONE, 0, (uint32_t)i, 0};
        w.insert(w.end(), c.siblings, c.siblings + 8 * (size_t)c.depth);
        ch.root = digest(c.root);
        if (c.inject) {
            if (!c.inject_at) return fail(lane.err, DVT_ERR_INPUT, "chain %zu: inject without inject_at", i);
            ch.inj = (uint32_t)inj.size();
            for (uint32_t l = 0; l < c.depth; l++) inj.push_back(c.inject_at[l] ? digest(c.inject + 8 * (size_t)l) : NONE);
        }
        cs[i] = ch;
    }
    for (size_t i = 0; i < w.size(); i++)
        if (w[i] >= P) return fail(lane.err, DVT_ERR_INPUT, "a digest word is not canonical");
    if (inj.empty()) inj.push_back(NONE);
    StageBuf buf{e.pool};
    const size_t wb = (w.size() * 4 + 15) & ~(size_t)15, ib = (inj.size() * 4 + 15) & ~(size_t)15, cb = n * sizeof(Chain);
    HIP_TRY(lane.err, e.pool.alloc_bytes(&buf.ptr, wb + ib + cb + n));
    uint8_t *base = static_cast<uint8_t *>(buf.ptr);
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    HIP_TRY(lane.err, hipMemcpy(base, w.data(), w.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemcpy(base + wb, inj.data(), inj.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemcpy(base + wb + ib, cs.data(), cb, hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemset(base + wb + ib + cb, 0, n));
    vq_path_kernel<<<(unsigned)((n + 15) / 16), 256, 0, e.stream>>>(reinterpret_cast<const Chain *>(base + wb + ib), (uint32_t)n,
                                                                    reinterpret_cast<const uint32_t *>(base + wb),
                                                                    reinterpret_cast<const uint32_t *>(base), base + wb + ib + cb);
    HIP_TRY(lane.err, hipGetLastError());
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    HIP_TRY(lane.err, hipMemcpy(ok, base + wb + ib + cb, n, hipMemcpyDeviceToHost));
    return DVT_OK;
}

int stage_verify_multipath(const Lane &lane, uint32_t depth, const uint32_t *leaf_index, const uint32_t *leaf_digest, size_t n,
                           const uint8_t *inject_at, const uint32_t *inject, const uint32_t *nodes, size_t n_nodes, const uint32_t *root,
                           uint8_t *ok) {
    Engine &e = lane.eng;
    const TreeSources ts = tree_sources(depth, std::vector<uint32_t>(leaf_index, leaf_index + n));
    if (ts.plan.nodes.size() != n_nodes)
        return fail(lane.err, DVT_ERR_INPUT, "%zu listed nodes, the indices ask for %zu", n_nodes, ts.plan.nodes.size());
    // the word space: leaf digests [n][8], joining digests [depth][n][8], the listed nodes, the root
    std::vector<uint32_t> w(leaf_digest, leaf_digest + 8 * n);
    const uint32_t inj0 = (uint32_t)w.size();
    if (inject_at) w.insert(w.end(), inject, inject + 8 * n * (size_t)depth);
    const uint32_t listed0 = (uint32_t)w.size();
    w.insert(w.end(), nodes, nodes + 8 * n_nodes);
    const uint32_t root0 = (uint32_t)w.size();
    w.insert(w.end(), root, root + 8);
    for (size_t i = 0; i < w.size(); i++)
        if (w[i] >= P) return fail(lane.err, DVT_ERR_INPUT, "a digest word is not canonical");
    MpTables mp;
    size_t nstatus = 0;
    emit_tree(mp, ts, depth, [&](uint32_t lh, uint32_t q) {
        if (lh == depth) return (uint32_t)(8 * q);
        return inject_at && inject_at[lh] ? inj0 + 8 * (uint32_t)(lh * n + q) : NONE;
    }, listed0, root0, &nstatus);
    std::vector<uint8_t> blob;
    const size_t at_w = put(blob, w), at_tr = put(blob, mp.trees), at_lv = put(blob, mp.levels), at_mj = put(blob, mp.jobs),
                 at_lf = put(blob, mp.leaves), at_cm = put(blob, mp.cmps);
    const size_t at_st = (blob.size() + 15) & ~(size_t)15;
    StageBuf buf{e.pool};
    HIP_TRY(lane.err, e.pool.alloc_bytes(&buf.ptr, at_st + nstatus));
    uint8_t *base = static_cast<uint8_t *>(buf.ptr);
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    HIP_TRY(lane.err, hipMemcpy(base, blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(lane.err, hipMemset(base + at_st, 0, nstatus));
    vq_multipath_kernel<<<1, 256, 2 * 32 * (size_t)mp.cap, e.stream>>>(reinterpret_cast<const Tree *>(base + at_tr), reinterpret_cast<const MpLevel *>(base + at_lv),
                                                                     reinterpret_cast<const MpJob *>(base + at_mj), reinterpret_cast<const uint32_t *>(base + at_lf),
                                                                     reinterpret_cast<const MpCmp *>(base + at_cm), mp.cap, reinterpret_cast<const uint32_t *>(base + at_w),
                                                                     base + at_st);
    HIP_TRY(lane.err, hipGetLastError());
    HIP_TRY(lane.err, hipStreamSynchronize(e.stream));
    std::vector<uint8_t> st(nstatus);
    HIP_TRY(lane.err, hipMemcpy(st.data(), base + at_st, nstatus, hipMemcpyDeviceToHost));
    *ok = 1;
    for (uint8_t b : st) *ok &= b;
    return DVT_OK;
}

void stage_free(Stage *s) { delete s; }

}  // namespace vq

DeviceQueries::DeviceQueries(dvt_prover *p) : p(p), batch(nullptr) {
    if (!p->vq_stage) p->vq_stage = new vq::Stage();
    batch = new vq::Batch(lane0(p), *p->vq_stage, p->vq_chunk_words);
}
DeviceQueries::~DeviceQueries() { delete static_cast<vq::Batch *>(batch); }
void DeviceQueries::add(const ShardQueryCtx &ctx, const uint32_t *words, size_t nwords) {
    size_t slot = 0;
    if (!rc) rc = static_cast<vq::Batch *>(batch)->add(ctx, words, nwords, &slot);
}
void DeviceQueries::finish(double host_ms) {
    vq::Batch &b = *static_cast<vq::Batch *>(batch);
    if (!rc) rc = b.finish();
    const vq::Times &t = b.times;
    const double v[9] = {host_ms - t.flatten_ms - t.wait_ms, t.flatten_ms, t.upload_ms, t.kernel_ms, t.download_ms, t.wait_ms,
                         (double)t.perms, (double)t.launches, (double)t.chunks};
    for (int i = 0; i < 9; i++) p->vq_times[i] = v[i];
}
std::string DeviceQueries::why(size_t shard) const { return static_cast<const vq::Batch *>(batch)->why(shard); }

}  // namespace dvt
