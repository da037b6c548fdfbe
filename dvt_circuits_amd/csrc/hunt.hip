// The host's end of the forgery hunt (hunt.cuh) on one lane: the request's checks, the challenges from the seed, the
// honest table's precondition, the split of the candidates into bounded launches, and the results.  The kernels are
// instantiated per chip in hunt_toy.hip, hunt_rv32.hip and hunt_rv32_wide.hip.
#include <algorithm>

#include "capi_internal.h"
#include "challenger.h"
#include "hunt.cuh"

namespace dvt {
namespace {
static_assert(sizeof(dvt_escape) == sizeof(HuntEscape) && DVT_HUNT_MAX_DELTAS == HUNT_MAX_DELTAS, "hunt.cuh mirrors the header");

// xi of the closed-form identities and the key of the fingerprints: a transcript over a domain tag and the seed
void hunt_challenges(uint64_t seed, Fp4 *xi, uint64_t *key) {
    Challenger g;
    for (const char *t = "dvt-hunt-cells-1"; *t; t++) g.observe_u32((uint8_t)*t);
    g.observe_u32((uint32_t)(seed & 0x3fffffffu));
    g.observe_u32((uint32_t)((seed >> 30) & 0x3fffffffu));
    g.observe_u32((uint32_t)(seed >> 60));
    *xi = g.sample_ext();
    *key = 0;
    for (int k = 0; k < 3; k++) *key ^= (uint64_t)g.sample().canonical() << (k == 2 ? 33 : 31 * k);
}

HuntPlan plan_of(const ChipDesc &d, uint32_t log_n, const HuntRequest &rq) {
    HuntPlan pl;
    const uint64_t n = (uint64_t)1 << log_n;
    if (rq.pairs && rq.cols) {
        pl.cols.assign(rq.cols, rq.cols + rq.n_cols);
        std::sort(pl.cols.begin(), pl.cols.end());
        pl.cols.erase(std::unique(pl.cols.begin(), pl.cols.end()), pl.cols.end());
    } else {
        for (int c = 0; c < d.main_w; c++) pl.cols.push_back((uint32_t)c);
    }
    const uint32_t k = (uint32_t)pl.cols.size();
    pl.map_rows = (uint32_t)std::min<uint64_t>((uint64_t)rq.row_count + (rq.pairs ? rq.adjacent : 0), n);
    pl.cell_evals = (uint64_t)rq.n_deltas * k * pl.map_rows * std::min<uint64_t>(2, n);
    if (rq.pairs) {
        for (uint32_t a = 0; a < k; a++)
            for (uint32_t b = rq.adjacent ? 0 : a + 1; b < k; b++) pl.pairs.push_back(a | (b << 16));
        pl.pair_evals = (uint64_t)pl.pairs.size() * rq.n_deltas * rq.n_deltas * rq.row_count * std::min<uint64_t>(rq.adjacent ? 3 : 2, n);
    }
    return pl;
}
// free_counts[k * n_deltas + e] = set bits of map[e * n_cols + k][.] (the idle lanes' bits are 0); one workgroup per (e, k)
__global__ void __launch_bounds__(256) hunt_count_kernel(const unsigned long long *map, uint32_t map_words, uint32_t n_cols, uint32_t n_deltas,
                                                         uint32_t *free_counts) {
    __shared__ uint32_t lds[256];
    uint32_t s = 0;
    for (uint32_t w = threadIdx.x; w < map_words; w += 256) s += (uint32_t)__popcll(map[(size_t)blockIdx.x * map_words + w]);
    lds[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int k = 0; k < 256; k++) tot += lds[k];
        free_counts[(blockIdx.x % n_cols) * n_deltas + blockIdx.x / n_cols] = tot;
    }
}
}  // namespace

int hunt_plan(std::string &err, const ChipDesc &d, uint32_t log_n, const HuntRequest &rq, HuntPlan *out) {
    if (log_n > 22) return fail(err, DVT_ERR_INPUT, "log_n %u > 22", log_n);
    const uint64_t n = (uint64_t)1 << log_n;
    if (!rq.deltas || rq.n_deltas == 0 || rq.n_deltas > HUNT_MAX_DELTAS) return fail(err, DVT_ERR_INPUT, "n_deltas %u (1..%u)", rq.n_deltas, HUNT_MAX_DELTAS);
    for (uint32_t e = 0; e < rq.n_deltas; e++)
        if (rq.deltas[e] == 0 || rq.deltas[e] >= P) return fail(err, DVT_ERR_INPUT, "delta %u is 0 or not below p", e);
    if (rq.row_count == 0 || (uint64_t)rq.row_first + rq.row_count > n) return fail(err, DVT_ERR_INPUT, "rows %u + %u outside the table of %llu rows", rq.row_first, rq.row_count, (unsigned long long)n);
    if (rq.pairs) {
        if (rq.adjacent > 1) return fail(err, DVT_ERR_INPUT, "adjacent %u", rq.adjacent);
        if (!rq.n_reported || !rq.n_tried || (rq.cap && !rq.out)) return fail(err, DVT_ERR_INPUT, "null argument");
        if (rq.cols && rq.n_cols == 0) return fail(err, DVT_ERR_INPUT, "empty column list");
        for (uint32_t k = 0; rq.cols && k < rq.n_cols; k++)
            if (rq.cols[k] >= (uint32_t)d.main_w) return fail(err, DVT_ERR_INPUT, "column %u: chip %s has %d", rq.cols[k], d.name, d.main_w);
    } else if (!rq.free_counts) return fail(err, DVT_ERR_INPUT, "null argument");
    if (!d.launch_hunt || !d.launch_check) return fail(err, DVT_ERR_UNSUPPORTED, "chip %s has no forgery hunt", d.name);
    if (d.main_w > 0xffff) return fail(err, DVT_ERR_UNSUPPORTED, "chip %s is too wide", d.name);
    HuntPlan pl = plan_of(d, log_n, rq);
    const uint64_t limit = rq.max_evals ? rq.max_evals : HUNT_DEFAULT_MAX_EVALS;
    if (pl.cell_evals + pl.pair_evals > limit)
        return fail(err, DVT_ERR_INPUT, "%llu evaluations (candidates x touched rows) exceed max_evals %llu", (unsigned long long)(pl.cell_evals + pl.pair_evals), (unsigned long long)limit);
    if ((uint64_t)pl.pairs.size() * rq.n_deltas * rq.n_deltas > 0xffffffffull) return fail(err, DVT_ERR_INPUT, "too many candidates");
    *out = std::move(pl);
    return DVT_OK;
}

int hunt_table(const Lane &c, const MachineDesc *m, const CheckTable &t, const std::vector<uint32_t> &pub_mont, const HuntRequest &rq, const HuntPlan &pl) {
    Engine &e = c.eng;
    const ChipDesc &d = *t.d;
    const size_t n = (size_t)1 << t.log_n;
    Fp4 xi;
    uint64_t key;
    hunt_challenges(rq.seed, &xi, &key);
    // the precondition: the honest table violates nothing
    {
        std::vector<CheckTableOut> res;
        const CheckChallenges ch{xi, Fp4::zero(), Fp4::zero()};
        if (int rc = check_tables(c, m, {t}, pub_mont, ch, true, false, &res)) return rc;
        if (res[0].r.violations)
            return fail(c.err, DVT_ERR_REJECTED, "the table is not honest: row %u violates constraint %d of chip %s (%llu violations)", res[0].r.first_row,
                        res[0].r.first_constraint, d.name, (unsigned long long)res[0].r.violations);
    }
    const uint32_t k = (uint32_t)pl.cols.size(), nd = rq.n_deltas;
    const unsigned cell_blocks = (pl.map_rows + 255) / 256, pair_blocks = (rq.row_count + 255) / 256;
    const size_t cap = rq.pairs ? (size_t)std::min<uint64_t>({(uint64_t)rq.cap, (uint64_t)HUNT_MAX_RECORDS, pl.pair_evals}) : 0;

    StageBuf honest{e.pool}, map{e.pool}, cols{e.pool}, pairs{e.pool}, out{e.pool}, counters{e.pool}, counts{e.pool};
    const size_t map_words = (size_t)cell_blocks * 4, map_bytes = (size_t)nd * k * map_words * 8;
    HIP_TRY(c.err, e.pool.alloc_bytes(&honest.ptr, 12 * n));
    HIP_TRY(c.err, e.pool.alloc_bytes(&map.ptr, map_bytes));
    HIP_TRY(c.err, e.pool.alloc_bytes(&cols.ptr, (size_t)k * 4));
    HIP_TRY(c.err, e.pool.alloc_bytes(&counters.ptr, 16));
    HIP_TRY(c.err, e.pool.alloc_bytes(&counts.ptr, (size_t)nd * k * 4));
    HIP_TRY(c.err, hipMemcpyAsync(cols.ptr, pl.cols.data(), (size_t)k * 4, hipMemcpyHostToDevice, e.stream));
    HIP_TRY(c.err, hipMemsetAsync(counters.ptr, 0, 16, e.stream));
    if (rq.pairs) {
        HIP_TRY(c.err, e.pool.alloc_bytes(&pairs.ptr, std::max<size_t>(pl.pairs.size(), 1) * 4));
        HIP_TRY(c.err, e.pool.alloc_bytes(&out.ptr, std::max<size_t>(cap, 1) * sizeof(HuntEscape)));
        if (!pl.pairs.empty()) HIP_TRY(c.err, hipMemcpyAsync(pairs.ptr, pl.pairs.data(), pl.pairs.size() * 4, hipMemcpyHostToDevice, e.stream));
    }
    int n_beta, n_alpha;
    challenge_power_counts(m, &n_beta, &n_alpha);
    HuntArgs a{};
    a.main = t.main; a.prep = t.prep;
    a.pub = static_cast<const uint32_t *>(e.upload_vec(pub_mont));
    if (!a.pub || !e.upload_powers(xi, (size_t)n_alpha, true, &a.xi_pows, &a.xi_d)) return engine_fail(c.err, e);
    a.log_n = t.log_n;
    a.key = key;
    a.honest = static_cast<uint32_t *>(honest.ptr);
    a.row_first = rq.row_first;
    a.n_deltas = nd;
    for (uint32_t i = 0; i < nd; i++) { a.delta_c[i] = rq.deltas[i]; a.delta_m[i] = Fp::from_canonical(rq.deltas[i]).v; }
    a.cols = static_cast<const uint32_t *>(cols.ptr);
    a.n_cols = k;
    a.map = static_cast<unsigned long long *>(map.ptr);
    a.map_words = (uint32_t)map_words;
    a.map_rows = pl.map_rows;
    a.pairs = static_cast<const uint32_t *>(pairs.ptr);
    a.adjacent = rq.pairs ? rq.adjacent : 0;
    a.out = static_cast<HuntEscape *>(out.ptr);
    a.cap = (uint32_t)cap;
    a.counters = static_cast<unsigned long long *>(counters.ptr);

    // the launches of one pass: at most HUNT_LAUNCH_EVALS evaluations each, and the stream's status between them
    auto pass = [&](uint32_t mode, unsigned row_blocks, uint32_t rows, uint64_t n_candidates, uint32_t touched) -> int {
        a.mode = mode;
        a.rows = rows;
        const uint64_t per = (uint64_t)row_blocks * 256 * touched;
        const uint64_t step = std::max<uint64_t>(1, std::min<uint64_t>(HUNT_MAX_CANDIDATES, HUNT_LAUNCH_EVALS / per));
        for (uint64_t at = 0; at < n_candidates; at += step) {
            a.cand_first = (uint32_t)at;
            HIP_TRY(c.err, d.launch_hunt(e.stream, a, row_blocks, (unsigned)std::min<uint64_t>(step, n_candidates - at)));
            HIP_TRY(c.err, hipStreamSynchronize(e.stream));
        }
        return DVT_OK;
    };
    if (int rc = pass(HUNT_HONEST, (unsigned)((n + 255) / 256), (uint32_t)std::min<size_t>(n, 0xffffffffu), 1, 1)) return rc;
    if (int rc = pass(HUNT_CELLS, cell_blocks, pl.map_rows, (uint64_t)nd * k, 2)) return rc;
    if (!rq.pairs) {
        hunt_count_kernel<<<nd * k, 256, 0, e.stream>>>(a.map, a.map_words, k, nd, static_cast<uint32_t *>(counts.ptr));
        HIP_TRY(c.err, hipGetLastError());
        std::vector<uint32_t> h((size_t)nd * k);
        if (!e.download(h.data(), counts.ptr, h.size() * 4)) return engine_fail(c.err, e);
        if (rq.free_map) {
            std::vector<unsigned long long> w(map_bytes / 8);
            HIP_TRY(c.err, hipMemcpy(w.data(), map.ptr, map_bytes, hipMemcpyDeviceToHost));
            for (size_t ek = 0; ek < (size_t)nd * k; ek++)
                for (uint32_t i = 0; i < rq.row_count; i++) rq.free_map[ek * rq.row_count + i] = (w[ek * map_words + (i >> 6)] >> (i & 63)) & 1;
        }
        memcpy(rq.free_counts, h.data(), h.size() * 4);   // (outputs are written only when the whole call succeeded)
        return DVT_OK;
    }
    if (int rc = pass(HUNT_PAIRS, pair_blocks, rq.row_count, (uint64_t)pl.pairs.size() * nd * nd, rq.adjacent ? 3 : 2)) return rc;
    unsigned long long cnt[2];
    if (!e.download(cnt, counters.ptr, sizeof cnt)) return engine_fail(c.err, e);
    std::vector<dvt_escape> recs((size_t)std::min<uint64_t>(cnt[0], cap));
    if (!recs.empty()) HIP_TRY(c.err, hipMemcpy(recs.data(), out.ptr, recs.size() * sizeof(dvt_escape), hipMemcpyDeviceToHost));
    std::sort(recs.begin(), recs.end(), [](const dvt_escape &x, const dvt_escape &y) {
        if (x.row != y.row) return x.row < y.row;
        if (x.col[0] != y.col[0]) return x.col[0] < y.col[0];
        if (x.col[1] != y.col[1]) return x.col[1] < y.col[1];
        if (x.delta[0] != y.delta[0]) return x.delta[0] < y.delta[0];
        return x.delta[1] < y.delta[1];
    });
    for (size_t i = 0; i < recs.size(); i++) rq.out[i] = recs[i];
    *rq.n_reported = cnt[0];
    *rq.n_tried = cnt[1];
    return DVT_OK;
}
}  // namespace dvt
