// Host-side shard verifier (no device work).  Mirrors Engine::prove_shard's
// transcript step for step; see DESIGN.md "Protocol".  The reference's own
// `verify` sub-command is not a STARK verifier; this
// plays the role of stock `client.verify(&proof, &vk)`.
#include <cstring>

#include "engine.h"

namespace dvt {
namespace {

Digest hash_rows(const std::vector<const std::vector<Fp> *> &rows) {
    Sponge sp;
    for (auto *r : rows)
        for (Fp x : *r) sp.absorb(x);
    return sp.finish();
}

bool verify_tree_opening(const TreeShape &shape, const TreeOpening &op, uint32_t idx, const Digest &root) {
    if (op.rows.size() != shape.mats.size() || op.path.size() != shape.log_h) return false;
    for (size_t i = 0; i < shape.mats.size(); i++)
        if (op.rows[i].size() != shape.mats[i].first) return false;
    auto rows_at = [&](uint32_t lh) {
        std::vector<const std::vector<Fp> *> r;
        for (size_t i = 0; i < shape.mats.size(); i++)
            if (shape.mats[i].second == lh) r.push_back(&op.rows[i]);
        return r;
    };
    Digest cur = hash_rows(rows_at(shape.log_h));
    uint32_t j = idx & ((1u << shape.log_h) - 1);
    for (uint32_t s = shape.log_h; s >= 1; s--) {
        uint32_t half = 1u << (s - 1);
        const Digest &sib = op.path[shape.log_h - s];
        cur = j < half ? p2_compress(cur, sib) : p2_compress(sib, cur);
        j &= half - 1;
        auto inj = rows_at(s - 1);
        if (!inj.empty()) cur = p2_compress(cur, hash_rows(inj));
    }
    return cur == root;
}

bool verify_path(Digest cur, const std::vector<Digest> &path, uint32_t log_h, uint32_t leaf, const Digest &root) {
    if (path.size() != log_h) return false;
    uint32_t j = leaf & ((1u << log_h) - 1);
    for (uint32_t s = log_h; s >= 1; s--) {
        uint32_t half = 1u << (s - 1);
        cur = j < half ? p2_compress(cur, path[log_h - s]) : p2_compress(path[log_h - s], cur);
        j &= half - 1;
    }
    return cur == root;
}

Fp4 ext_from_flat(const Fp4 *p) {  // sum_k x^k * p[k]
    Fp4 acc = p[0];
    for (int k = 1; k < 4; k++) {
        Fp4 b = Fp4::zero();
        b.c[k] = Fp::one();
        acc += b * p[k];
    }
    return acc;
}

}  // namespace

// ---- the host part: everything up to the query indices
std::string verify_shard_host(const VerifyingKey &vk, const ShardProof &pf, const StarkConfig &cfg, const PermChallenges *global,
                              Fp4 *cumsum_total, ShardQueryCtx *ctx) {
    const MachineDesc *m = vk.machine;
    if (!m) return "no machine";
    if (pf.chips.empty()) return "no chips";
    std::vector<ChipRef> refs;
    uint32_t max_log_n = 0;
    int max_pub = 0;
    for (auto &o : pf.chips) {
        if (o.chip_id >= (uint32_t)m->n_chips) return "chip id out of range";
        if (!refs.empty() && (int)o.chip_id <= refs.back().chip_id) return "chips not sorted";
        if (o.log_n > 22) return "log_n too large";
        const ChipDesc &d = m->chips[o.chip_id];
        if (o.prep_l.size() != (size_t)d.prep_w || o.prep_n.size() != (size_t)d.prep_w || o.main_l.size() != (size_t)d.main_w ||
            o.main_n.size() != (size_t)d.main_w || o.perm_l.size() != (size_t)4 * d.perm_ext_w ||
            o.perm_n.size() != (size_t)4 * d.perm_ext_w || o.quot.size() != 8)
            return std::string("opened value shape mismatch for chip ") + d.name;
        refs.push_back({(int)o.chip_id, o.log_n});
        max_log_n = std::max(max_log_n, o.log_n);
        max_pub = std::max(max_pub, d.n_pub);
    }
    if ((int)pf.public_values.size() < max_pub) return "too few public values";
    for (auto &pc : vk.prep_chips) {
        bool ok = false;
        for (auto &r : refs) ok |= r.chip_id == pc.chip_id && r.log_n == pc.log_n;
        if (!ok) return "preprocessed chip missing or of wrong height";
    }
    for (auto &r : refs)
        if (m->chips[r.chip_id].prep_w) {
            bool ok = false;
            for (auto &pc : vk.prep_chips) ok |= pc.chip_id == r.chip_id;
            if (!ok) return "chip with preprocessed columns is not in the verifying key";
        }
    const uint32_t hmax = max_log_n + 1;
    if (pf.fri_roots.size() != hmax - 1) return "wrong number of FRI layers";
    if (pf.queries.size() != cfg.num_queries) return "wrong number of queries";

    // ---- transcript
    Challenger ch;
    transcript_begin(ch, vk, refs);
    ch.observe(pf.main_root);
    ch.observe_u32((uint32_t)pf.public_values.size());
    for (auto x : pf.public_values) ch.observe(x);
    Fp4 perm_alpha, beta;
    if (global) {
        perm_alpha = global->alpha;
        beta = global->beta;
        ch.observe(perm_alpha);
        ch.observe(beta);
    } else {
        perm_alpha = ch.sample_ext();
        beta = ch.sample_ext();
    }
    ch.observe(pf.perm_root);
    Fp4 total = Fp4::zero();
    for (auto &o : pf.chips) {
        const ChipDesc &d = m->chips[o.chip_id];
        if (!d.perm_ext_w && o.cumsum != Fp4::zero()) return "cumulative sum on a chip without interactions";
        ch.observe(o.cumsum);
        total += o.cumsum;
    }
    if (cumsum_total) *cumsum_total = total;
    else if (total != Fp4::zero()) return "LogUp cumulative sums do not cancel";
    Fp4 alpha = ch.sample_ext();
    ch.observe(pf.quot_root);
    Fp4 zeta = ch.sample_ext();
    for (auto &o : pf.chips)
        for (auto *v : {&o.prep_l, &o.prep_n, &o.main_l, &o.main_n, &o.perm_l, &o.perm_n, &o.quot}) ch.observe_values(*v);

    // ---- constraints at zeta
    int max_arity = 1, max_folded = 1;
    for (int i = 0; i < m->n_chips; i++) {
        max_arity = std::max(max_arity, m->chips[i].max_arity);
        max_folded = std::max(max_folded, m->chips[i].n_folded);
    }
    std::vector<Fp4> beta_pows(max_arity), alpha_pows(max_folded);
    { Fp4 x = beta; for (auto &b : beta_pows) { b = x; x = x * beta; } }
    { Fp4 x = Fp4::one(); for (auto &a : alpha_pows) { a = x; x = x * alpha; } }
    const Fp g = Fp::from_canonical(COSET_SHIFT);
    for (auto &o : pf.chips) {
        const ChipDesc &d = m->chips[o.chip_id];
        const size_t n = (size_t)1 << o.log_n;
        VerifierAccess ax{o.main_l.data(), o.main_n.data(), o.prep_l.data(), o.prep_n.data(), o.perm_l.data(), o.perm_n.data(),
                          pf.public_values.data()};
        VerifierPoint pt;
        pt.alpha_pows = alpha_pows.data();
        pt.beta_pows = beta_pows.data();
        pt.perm_alpha = perm_alpha;
        pt.cum_over_n = o.cumsum * inv(Fp::from_canonical((uint32_t)n));
        Fp w_inv = inv(two_adic_generator(o.log_n));
        Fp4 zh = pow(zeta, n) - Fp::one();
        Fp4 d1 = zeta - Fp::one(), d2 = zeta - w_inv;
        if (d1 == Fp4::zero() || d2 == Fp4::zero() || zh == Fp4::zero()) return "zeta lies in the trace domain";
        pt.sel_first = zh * inv(d1);
        pt.sel_last = zh * inv(d2);
        pt.sel_trans = d2;
        Fp4 folded = d.verify_eval(ax, pt);
        Fp4 r0 = ext_from_flat(o.quot.data()), r1 = ext_from_flat(o.quot.data() + 4);
        Fp4 u = pow(zeta * inv(g), n);
        Fp4 zd0 = u - Fp::one(), zd1 = -u - Fp::one();
        Fp4 q = (r0 * zd1 + r1 * zd0) * inv(-Fp::two());
        if (folded != zh * q) return std::string("constraint check failed at zeta for chip ") + d.name;
    }

    // ---- FRI
    Fp4 alpha_fri = ch.sample_ext();
    std::vector<Fp4> &fold_betas = ctx->fold_betas;
    fold_betas.clear();
    for (auto &r : pf.fri_roots) {
        ch.observe(r);
        fold_betas.push_back(ch.sample_ext());
    }
    ch.observe(pf.final_poly);
    if (!ch.check_witness(cfg.pow_bits, pf.pow_witness)) return "proof-of-work witness rejected";

    TreeShape *shapes = ctx->shapes;
    for (int t = 0; t < 4; t++) shapes[t] = TreeShape{};
    for (auto &r : refs) {
        const ChipDesc &d = m->chips[r.chip_id];
        if (d.prep_w) shapes[0].mats.push_back({(uint32_t)d.prep_w, r.log_n + 1});
        shapes[1].mats.push_back({(uint32_t)d.main_w, r.log_n + 1});
        if (d.perm_ext_w) shapes[2].mats.push_back({(uint32_t)(4 * d.perm_ext_w), r.log_n + 1});
        shapes[3].mats.push_back({8u, r.log_n + 1});
    }
    for (int t = 0; t < 4; t++)
        for (auto &mt : shapes[t].mats) shapes[t].log_h = std::max(shapes[t].log_h, mt.second);
    ctx->vk = &vk;
    ctx->pf = &pf;
    ctx->hmax = hmax;
    ctx->zeta = zeta;
    ctx->roots[0] = &vk.prep_root; ctx->roots[1] = &pf.main_root; ctx->roots[2] = &pf.perm_root; ctx->roots[3] = &pf.quot_root;

    std::vector<std::vector<ColRef>> &cols_by_h = ctx->cols_by_h;
    std::vector<uint32_t> &n_two_by_h = ctx->n_two_by_h;
    cols_by_h.assign(hmax + 1, {});
    n_two_by_h.assign(hmax + 1, 0);
    size_t max_cols = 1;
    for (uint32_t h = 1; h <= hmax; h++) {
        cols_by_h[h] = fri_columns(m, refs, h, &n_two_by_h[h]);
        max_cols = std::max(max_cols, cols_by_h[h].size());
    }
    ctx->apow.assign(max_cols + 1, Fp4::zero());
    { Fp4 x = Fp4::one(); for (auto &a : ctx->apow) { a = x; x = x * alpha_fri; } }
    // the query indices depend on nothing a query opens: all of them are drawn here
    ctx->idx.resize(cfg.num_queries);
    for (auto &i : ctx->idx) i = ch.sample_bits(hmax);
    if (pf.compact) ctx->paths = tree_sources(hmax, ctx->idx);   // one plan for every tree of the shard
    return "";
}

// the batched quotient of the columns of LDE height h at the point the query opens (the FRI input of that height)
static Fp4 reduced_opening_at(const ShardQueryCtx &ctx, const QueryProof &q, uint32_t idx, uint32_t h) {
    const ShardProof &pf = *ctx.pf;
    const std::vector<Fp4> &apow = ctx.apow;
    const auto &cols = ctx.cols_by_h[h];
    const Fp g = Fp::from_canonical(COSET_SHIFT);
    Fp x = g * pow(two_adic_generator(h), idx & ((1u << h) - 1));
    Fp4 s_all = Fp4::zero(), s_two = Fp4::zero();
    for (size_t c = 0; c < cols.size(); c++) {
        const ColRef &r = cols[c];
        const ChipOpening &o = pf.chips[r.chip_pos];
        Fp px = q.trees[r.tree].rows[r.mat][r.col];
        const std::vector<Fp4> &loc = r.tree == 0 ? o.prep_l : r.tree == 1 ? o.main_l : r.tree == 2 ? o.perm_l : o.quot;
        s_all += apow[c] * (Fp4::from_base(px) - loc[r.col]);
        if (r.tree < 3) {
            const std::vector<Fp4> &nx = r.tree == 0 ? o.prep_n : r.tree == 1 ? o.main_n : o.perm_n;
            s_two += apow[c] * (Fp4::from_base(px) - nx[r.col]);
        }
    }
    Fp4 zeta_next = ctx.zeta * two_adic_generator(h - 1);
    Fp4 r = s_all * inv(Fp4::from_base(x) - ctx.zeta);
    if (ctx.n_two_by_h[h]) r += apow[cols.size()] * (s_two * inv(Fp4::from_base(x) - zeta_next));
    return r;
}

// ---- the query part on the host: query qi of the shard whose host part left ctx
std::string verify_query_host(const ShardQueryCtx &ctx, uint32_t qi) {
    const ShardProof &pf = *ctx.pf;
    const TreeShape *shapes = ctx.shapes;
    const Digest *const *roots = ctx.roots;
    const std::vector<std::vector<ColRef>> &cols_by_h = ctx.cols_by_h;
    const std::vector<Fp4> &fold_betas = ctx.fold_betas;
    const uint32_t hmax = ctx.hmax;
    const Fp inv2 = inv(Fp::two());
    {
        const QueryProof &q = pf.queries[qi];
        const uint32_t idx = ctx.idx[qi];
        for (int t = 0; t < 4; t++) {
            if (shapes[t].mats.empty()) {
                if (!q.trees[t].rows.empty() || !q.trees[t].path.empty()) return "unexpected opening for an empty tree";
                continue;
            }
            if (!verify_tree_opening(shapes[t], q.trees[t], idx, *roots[t])) return "Merkle opening rejected (input tree)";
        }
        auto reduced = [&](uint32_t h) { return reduced_opening_at(ctx, q, idx, h); };
        if (q.layers.size() != hmax - 1) return "wrong number of FRI layer openings";
        Fp4 e = reduced(hmax);
        for (uint32_t k = 0; k + 1 < hmax; k++) {
            const uint32_t lm = hmax - k, half = 1u << (lm - 1);
            const uint32_t j = idx & ((1u << lm) - 1), jl = j & (half - 1);
            const FriLayerOpening &lo = q.layers[k];
            Fp4 a = j < half ? e : lo.sibling, b = j < half ? lo.sibling : e;
            Sponge sp;
            for (int c = 0; c < 4; c++) sp.absorb(a.c[c]);
            for (int c = 0; c < 4; c++) sp.absorb(b.c[c]);
            if (!verify_path(sp.finish(), lo.path, lm - 1, jl, pf.fri_roots[k])) return "Merkle opening rejected (FRI layer)";
            Fp xinv = inv(pow(two_adic_generator(lm), jl));
            e = (a + b) * inv2 + fold_betas[k] * ((a - b) * (inv2 * xinv));
            if (!cols_by_h[lm - 1].empty()) e += reduced(lm - 1);
        }
        if (e != pf.final_poly) return "FRI final value mismatch";
    }
    return "";
}

std::string verify_shard(const VerifyingKey &vk, const ShardProof &pf, const StarkConfig &cfg, const PermChallenges *global,
                         Fp4 *cumsum_total) {
    ShardQueryCtx ctx;
    std::string why = verify_shard_host(vk, pf, cfg, global, cumsum_total, &ctx);
    if (why.empty() && pf.compact) return verify_compact_queries(ctx);
    for (uint32_t qi = 0; why.empty() && qi < cfg.num_queries; qi++) why = verify_query_host(ctx, qi);
    return why;
}

// every shape check of query qi's section (what verify_query_host refuses before or while it hashes)
bool query_shape_ok(const ShardQueryCtx &ctx, uint32_t qi) {
    const QueryProof &q = ctx.pf->queries[qi];
    for (int t = 0; t < 4; t++) {
        const TreeShape &sh = ctx.shapes[t];
        const TreeOpening &op = q.trees[t];
        if (sh.mats.empty()) {
            if (!op.rows.empty() || !op.path.empty()) return false;
            continue;
        }
        if (op.rows.size() != sh.mats.size() || op.path.size() != sh.log_h) return false;
        for (size_t i = 0; i < sh.mats.size(); i++)
            if (op.rows[i].size() != sh.mats[i].first) return false;
    }
    if (q.layers.size() != ctx.hmax - 1) return false;
    for (uint32_t k = 0; k + 1 < ctx.hmax; k++)
        if (q.layers[k].path.size() != ctx.hmax - k - 1) return false;
    return true;
}

// ------------------------------------------------------------------------------------------------ the compact form (DVP2)

static uint32_t list_depth(const ShardQueryCtx &ctx, size_t li) { return li < 4 ? ctx.shapes[li].log_h : ctx.hmax - (uint32_t)(li - 4) - 1; }

bool compact_shape_ok(const ShardQueryCtx &ctx, std::string *why) {
    const ShardProof &pf = *ctx.pf;
    auto no = [&](const char *t) { if (why) *why = t; return false; };
    for (auto &q : pf.queries) {
        for (int t = 0; t < 4; t++) {
            const TreeShape &sh = ctx.shapes[t];
            const TreeOpening &op = q.trees[t];
            if (!op.path.empty()) return no("a compact shard proof carries a path");
            if (sh.mats.empty()) {
                if (!op.rows.empty()) return no("unexpected opening for an empty tree");
                continue;
            }
            if (op.rows.size() != sh.mats.size()) return no("Merkle opening rejected (input tree)");
            for (size_t i = 0; i < sh.mats.size(); i++)
                if (op.rows[i].size() != sh.mats[i].first) return no("Merkle opening rejected (input tree)");
        }
        if (q.layers.size() != ctx.hmax - 1) return no("wrong number of FRI layer openings");
        for (auto &l : q.layers)
            if (!l.path.empty()) return no("a compact shard proof carries a path");
    }
    if (pf.node_lists.size() != 4 + (size_t)ctx.hmax - 1) return no("wrong number of node lists");
    for (size_t i = 0; i < pf.node_lists.size(); i++) {
        const bool empty = i < 4 && ctx.shapes[i].mats.empty();
        const size_t want = empty ? 0 : ctx.paths.plan.listed(list_depth(ctx, i));
        if (pf.node_lists[i].size() != want) return no("node list length does not match the query indices");
    }
    return true;
}

TreeSources tree_sources(uint32_t depth, const std::vector<uint32_t> &idx) {
    TreeSources ts;
    ts.plan = multipath_plan(depth, idx.data(), idx.size());
    const uint32_t NOQ = 0xffffffffu;
    ts.first.resize(depth + 1);
    ts.dups.resize(depth + 1);
    ts.listed_at.resize(depth + 1);
    for (uint32_t lh = 0; lh <= depth; lh++) {
        const std::vector<uint32_t> &keys = ts.plan.keys[lh];
        ts.first[lh].assign(keys.size(), NOQ);
        for (uint32_t q = 0; q < idx.size(); q++) {
            const uint32_t j = idx[q] & (uint32_t)(((uint64_t)1 << lh) - 1);
            const size_t slot = std::lower_bound(keys.begin(), keys.end(), j) - keys.begin();
            uint32_t &f = ts.first[lh][slot];
            if (f == NOQ) f = q;
            else ts.dups[lh].push_back({f, q});
        }
    }
    for (size_t n = 0; n < ts.plan.nodes.size(); n++) ts.listed_at[ts.plan.nodes[n].first].push_back({ts.plan.nodes[n].second, (uint32_t)n});
    for (auto &l : ts.listed_at) std::sort(l.begin(), l.end());
    return ts;
}

namespace {

// what the opened values of one query come to before any path: the row digests of each height of each input tree, the
// leaf of every FRI layer and the value the fold chain ends in
struct QueryDigests {
    std::vector<Digest> rows[4];       // [lh] where the tree has matrices of that height
    std::vector<uint8_t> has[4];
    std::vector<Digest> layer_leaf;
    Fp4 final_value;
};
QueryDigests query_digests(const ShardQueryCtx &ctx, uint32_t qi) {
    const ShardProof &pf = *ctx.pf;
    const QueryProof &q = pf.queries[qi];
    const uint32_t idx = ctx.idx[qi], hmax = ctx.hmax;
    QueryDigests d;
    for (int t = 0; t < 4; t++) {
        const TreeShape &sh = ctx.shapes[t];
        if (sh.mats.empty()) continue;
        d.rows[t].resize(sh.log_h + 1);
        d.has[t].assign(sh.log_h + 1, 0);
        for (uint32_t lh = 0; lh <= sh.log_h; lh++) {
            std::vector<const std::vector<Fp> *> r;
            for (size_t i = 0; i < sh.mats.size(); i++)
                if (sh.mats[i].second == lh) r.push_back(&q.trees[t].rows[i]);
            if (r.empty()) continue;
            d.has[t][lh] = 1;
            d.rows[t][lh] = hash_rows(r);
        }
    }
    const Fp inv2 = inv(Fp::two());
    Fp4 e = reduced_opening_at(ctx, q, idx, hmax);
    for (uint32_t k = 0; k + 1 < hmax; k++) {
        const uint32_t lm = hmax - k, half = 1u << (lm - 1);
        const uint32_t j = idx & ((1u << lm) - 1), jl = j & (half - 1);
        const Fp4 sib = q.layers[k].sibling;
        Fp4 a = j < half ? e : sib, b = j < half ? sib : e;
        Sponge sp;
        for (int c = 0; c < 4; c++) sp.absorb(a.c[c]);
        for (int c = 0; c < 4; c++) sp.absorb(b.c[c]);
        d.layer_leaf.push_back(sp.finish());
        Fp xinv = inv(pow(two_adic_generator(lm), jl));
        e = (a + b) * inv2 + ctx.fold_betas[k] * ((a - b) * (inv2 * xinv));
        if (!ctx.cols_by_h[lm - 1].empty()) e += reduced_opening_at(ctx, q, idx, lm - 1);
    }
    d.final_value = e;
    return d;
}

// One tree of `depth` levels of a compact shard, walked with the shard's sources: `digest_of(lh, q)` is query q's digest of
// height lh (nullptr: the tree has none there), `listed` the tree's node list.  False when two queries disagree on a digest
// they share or the walk does not end in the root.  With levels != nullptr every node on a path is kept:
// (*levels)[lh][slot of ts.plan.keys[lh]].
template <class F>
bool walk_tree(const TreeSources &ts, uint32_t depth, const std::vector<Digest> &listed, const Digest &root, F digest_of,
               std::vector<std::vector<Digest>> *levels) {
    const MultipathPlan &pl = ts.plan;
    const uint32_t base = pl.base[depth];
    bool agree = true;
    for (uint32_t lh = 0; lh <= depth; lh++)
        for (auto &d : ts.dups[lh]) {
            const Digest *a = digest_of(lh, d[0]);
            if (a && !(*a == *digest_of(lh, d[1]))) agree = false;
        }
    if (!agree && !levels) return false;   // (a caller that wants the nodes gets those of the first query on each)
    std::vector<Digest> cur(pl.keys[depth].size());
    for (size_t i = 0; i < cur.size(); i++) cur[i] = *digest_of(depth, ts.first[depth][i]);
    if (levels) { levels->assign(depth + 1, {}); (*levels)[depth] = cur; }
    for (uint32_t s = depth; s >= 1; s--) {
        const auto &jobs = pl.levels[pl.depth - s];
        std::vector<Digest> up(jobs.size());
        for (size_t i = 0; i < jobs.size(); i++) {
            const MultipathJob &jb = jobs[i];
            const Digest &l = jb.l & MP_LISTED ? listed[(jb.l & ~MP_LISTED) - base] : cur[jb.l];
            const Digest &r = jb.r & MP_LISTED ? listed[(jb.r & ~MP_LISTED) - base] : cur[jb.r];
            up[i] = p2_compress(l, r);
            if (const Digest *inj = digest_of(s - 1, ts.first[s - 1][i])) up[i] = p2_compress(up[i], *inj);
        }
        cur.swap(up);
        if (levels) (*levels)[s - 1] = cur;
    }
    return agree && cur.size() == 1 && cur[0] == root;
}

// the trees of a compact shard in the order of the wire format, each walked by `visit(list index, depth, root, digest_of)`
template <class V>
void for_each_tree(const ShardQueryCtx &ctx, const std::vector<QueryDigests> &D, V visit) {
    for (int t = 0; t < 4; t++) {
        const TreeShape &sh = ctx.shapes[t];
        if (sh.mats.empty()) continue;
        if (!visit((size_t)t, sh.log_h, *ctx.roots[t], [&D, t](uint32_t lh, uint32_t q) { return D[q].has[t][lh] ? &D[q].rows[t][lh] : nullptr; })) return;
    }
    for (uint32_t k = 0; k + 1 < ctx.hmax; k++) {
        const uint32_t depth = ctx.hmax - k - 1;
        if (!visit((size_t)4 + k, depth, ctx.pf->fri_roots[k], [&D, k, depth](uint32_t lh, uint32_t q) { return lh == depth ? &D[q].layer_leaf[k] : nullptr; })) return;
    }
}

}  // namespace

std::string verify_compact_queries(const ShardQueryCtx &ctx) {
    std::string why;
    if (!compact_shape_ok(ctx, &why)) return why;
    const ShardProof &pf = *ctx.pf;
    std::vector<QueryDigests> D;
    for (uint32_t qi = 0; qi < pf.queries.size(); qi++) D.push_back(query_digests(ctx, qi));
    for_each_tree(ctx, D, [&](size_t li, uint32_t depth, const Digest &root, auto digest_of) {
        if (!walk_tree(ctx.paths, depth, pf.node_lists[li], root, digest_of, nullptr))
            why = li < 4 ? "Merkle opening rejected (input tree)" : "Merkle opening rejected (FRI layer)";
        return why.empty();
    });
    if (!why.empty()) return why;
    for (auto &d : D)
        if (d.final_value != pf.final_poly) return "FRI final value mismatch";
    return "";
}

void compact_list_sweep(const ShardQueryCtx &ctx, uint64_t *n_words, uint64_t *n_accepted) {
    const ShardProof &pf = *ctx.pf;
    std::vector<QueryDigests> D;
    for (uint32_t qi = 0; qi < pf.queries.size(); qi++) D.push_back(query_digests(ctx, qi));
    for_each_tree(ctx, D, [&](size_t li, uint32_t depth, const Digest &root, auto digest_of) {
        std::vector<Digest> listed = pf.node_lists[li];
        for (auto &dg : listed)
            for (int w = 0; w < 8; w++) {
                const Fp keep = dg.d[w];
                dg.d[w] = keep + Fp::one();
                ++*n_words;
                *n_accepted += walk_tree(ctx.paths, depth, listed, root, digest_of, nullptr);
                dg.d[w] = keep;
            }
        return true;
    });
}

std::string compact_shard(const ShardQueryCtx &ctx, ShardProof *out) {
    const ShardProof &pf = *ctx.pf;
    *out = pf;
    if (pf.compact) return "";
    for (uint32_t qi = 0; qi < pf.queries.size(); qi++)
        if (!query_shape_ok(ctx, qi)) return verify_query_host(ctx, qi);
    out->compact = true;
    out->query_words.clear();
    out->node_lists.assign(4 + (size_t)ctx.hmax - 1, {});
    const TreeSources ts = tree_sources(ctx.hmax, ctx.idx);
    const MultipathPlan &pl = ts.plan;
    // the listed node (level s, index i) is the sibling at level s of the queries whose path passes i ^ half
    auto fill = [&](size_t li, uint32_t depth, auto path_of) {
        for (size_t n = pl.base[depth]; n < pl.nodes.size(); n++) {
            const uint32_t s = pl.nodes[n].first, me = pl.nodes[n].second ^ (1u << (s - 1));
            const size_t slot = std::lower_bound(pl.keys[s].begin(), pl.keys[s].end(), me) - pl.keys[s].begin();
            out->node_lists[li].push_back(path_of(ts.first[s][slot])[depth - s]);
        }
    };
    for (int t = 0; t < 4; t++)
        if (!ctx.shapes[t].mats.empty()) fill((size_t)t, ctx.shapes[t].log_h, [&](uint32_t q) -> const std::vector<Digest> & { return pf.queries[q].trees[t].path; });
    for (uint32_t k = 0; k + 1 < ctx.hmax; k++)
        fill((size_t)4 + k, ctx.hmax - k - 1, [&](uint32_t q) -> const std::vector<Digest> & { return pf.queries[q].layers[k].path; });
    for (auto &q : out->queries) {
        for (auto &t : q.trees) t.path.clear();
        for (auto &l : q.layers) l.path.clear();
    }
    return "";
}

std::string expand_shard(const ShardQueryCtx &ctx, ShardProof *out) {
    const ShardProof &pf = *ctx.pf;
    *out = pf;
    if (!pf.compact) return "";
    std::string why;
    if (!compact_shape_ok(ctx, &why)) return why;
    out->compact = false;
    out->node_lists.clear();
    out->query_words.clear();
    std::vector<QueryDigests> D;
    for (uint32_t qi = 0; qi < pf.queries.size(); qi++) D.push_back(query_digests(ctx, qi));
    const TreeSources &ts = ctx.paths;
    const MultipathPlan &pl = ts.plan;
    for_each_tree(ctx, D, [&](size_t li, uint32_t depth, const Digest &root, auto digest_of) {
        std::vector<std::vector<Digest>> levels;
        (void)walk_tree(ts, depth, pf.node_lists[li], root, digest_of, &levels);
        // the sibling of a path's node at level s: a node another path computes, or the listed one (both by binary search)
        for (uint32_t q = 0; q < ctx.idx.size(); q++) {
            std::vector<Digest> &path = li < 4 ? out->queries[q].trees[li].path : out->queries[q].layers[li - 4].path;
            path.resize(depth);
            for (uint32_t s = depth; s >= 1; s--) {
                const uint32_t half = 1u << (s - 1), sib = (ctx.idx[q] & ((1u << s) - 1)) ^ half;
                const auto &keys = pl.keys[s];
                const auto it = std::lower_bound(keys.begin(), keys.end(), sib);
                if (it != keys.end() && *it == sib) { path[depth - s] = levels[s][it - keys.begin()]; continue; }
                const auto &at = ts.listed_at[s];
                const auto ln = std::lower_bound(at.begin(), at.end(), std::make_pair(sib, 0u));
                path[depth - s] = pf.node_lists[li][ln->second - pl.base[depth]];   // (present: the plan lists what no path computes)
            }
        }
        return true;
    });
    return "";
}

}  // namespace dvt
