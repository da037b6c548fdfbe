// Stand-alone driver of the divergence report's host rule (csrc/diverge.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-diverge && build/asan/diverge_host GUEST.elf STDIN_A.bin STDIN_B.bin
// Runs the guest in trace mode on both inputs (rv32::Vm, shards of 2^10 cycles; a run that traps or exits non-zero counts
// with what retired), keeps the records of both runs in diverge::Kept and runs diverge::compare from the entry, from span and
// shard edges, from unequal starts and from the end, with keep sizes 0, 1 and 64, pair limits 0, 1 and 4097 and rejoin windows 1,
// 4096 and 16384; follows the chain of rejoins up to 8 segments; compares run A with itself; then does the same over the records
// with their fields overwritten by a fixed pseudo-random stream (instruction indices outside the text, addresses outside guest
// memory), where the rule must stop at the first bad pair without reading or writing out of bounds.  Exit code 0 when every
// answer keeps the laws of the rule:
//   n_pairs is at most the pairs there are, the kept pairs are data pairs in ascending order below n_pairs, n_kept = min(K, n_data),
//   first_data / last_data are the ends of the kept lists when they are whole, every register's last_diff is a write at or before
//   its last_write, a rejoin lies inside its window, and a run against itself has no data pair and ends both streams.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "../../dvt_circuits_amd/csrc/diverge.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

using Shards = std::vector<std::vector<rv32::CycleRec>>;

struct Answer {
    std::vector<dvt_diverge_pair> first, last;
    dvt_diverge_reg regs[32];
    dvt_diverge_summary s;
    uint64_t pairs_there;
};

static void report(const rv32::Program &prog, const Shards &a, const Shards &b, dvt_diverge_pos at_a, dvt_diverge_pos at_b, uint64_t max_pairs, uint32_t flags,
                   uint32_t window, uint32_t K, Answer *out) {
    diverge::Kept ka, kb;
    for (auto &sh : a) ka.scan(sh.data(), sh.size(), at_a);
    for (auto &sh : b) kb.scan(sh.data(), sh.size(), at_b);
    const uint64_t ga = ka.st.global_of(at_a), gb = kb.st.global_of(at_b);
    out->first.assign(K + 1, dvt_diverge_pair{});
    out->last.assign(K + 1, dvt_diverge_pair{});
    diverge::compare(prog, ka, kb, ga, gb, max_pairs, flags, window, K, out->first.data(), out->last.data(), out->regs, &out->s);
    out->pairs_there = std::min(ka.st.len() - ga, kb.st.len() - gb);
    if (max_pairs) out->pairs_there = std::min<uint64_t>(out->pairs_there, max_pairs);
}

static bool lawful(const Answer &a, uint32_t K, uint32_t window) {
    const dvt_diverge_summary &s = a.s;
    bool good = s.n_pairs <= a.pairs_there && s.n_kept == std::min<uint64_t>(K, s.n_data) && s.n_data <= s.n_pairs && s.reason >= DVT_DIV_SPLIT && s.reason <= DVT_DIV_LIMIT;
    good = good && ((s.reason == DVT_DIV_SPLIT || s.reason == DVT_DIV_BAD) ? s.n_pairs < a.pairs_there : s.n_pairs == a.pairs_there);
    for (int half = 0; half < 2; half++) {
        const std::vector<dvt_diverge_pair> &l = half ? a.last : a.first;
        for (uint32_t i = 0; i < s.n_kept; i++)
            good = good && l[i].k < s.n_pairs && l[i].mask && l[i].mask <= 15 && (!i || l[i - 1].k < l[i].k) && !(l[i].mask & ~s.mask);
    }
    if (s.n_kept) good = good && a.first[0].k == s.first_data && a.last[s.n_kept - 1].k == s.last_data;
    if (!s.n_data) good = good && s.first_data == DVT_DIV_NONE && s.last_data == DVT_DIV_NONE && !s.mask;
    for (int r = 0; r < 32; r++) {
        const dvt_diverge_reg &g = a.regs[r];
        good = good && (g.n_diff ? g.first_diff <= g.last_diff && g.last_diff <= g.last_write && g.last_write < s.n_pairs : g.first_diff == DVT_DIV_NONE && !g.live);
        good = good && (r || g.last_write == DVT_DIV_NONE);
    }
    if (s.rejoin_skip_a != DVT_DIVERGE_NO_REJOIN) good = good && s.reason == DVT_DIV_SPLIT && s.rejoin_skip_a < window && s.rejoin_skip_b < window;
    return good;
}

// every call of the list over one pair of record sets; exact: the records are as executed
static bool sweep(const char *what, const rv32::Program &prog, const Shards &a, const Shards &b, bool exact) {
    const uint32_t S = (uint32_t)std::min(a.size(), b.size());
    const dvt_diverge_pos starts[][2] = {{{1, 0}, {1, 0}}, {{1, 1023}, {1, 1023}}, {{2, 0}, {2, 0}}, {{1, 5}, {1, 6}}, {{S, 3}, {1, 0}}, {{S + 1, 0}, {1, 0}}, {{0, 0}, {9, 9}}};
    bool ok = true;
    for (auto &at : starts) {
        uint64_t calls = 0, data = 0;
        bool good = true;
        for (uint32_t K : {0u, 1u, 64u})
            for (uint64_t max_pairs : {0ull, 1ull, 4097ull})
                for (uint32_t window : {1u, 4096u, 16384u}) {
                    Answer r{};
                    report(prog, a, b, at[0], at[1], max_pairs, DVT_DIVERGE_REJOIN, window, K, &r);
                    good = good && lawful(r, K, window) && (!exact || r.s.reason != DVT_DIV_BAD);
                    calls++; data += r.s.n_data;
                }
        printf("%s from %u:%u / %u:%u: %llu calls, %llu data pairs%s\n", what, at[0].shard, at[0].row, at[1].shard, at[1].row, (unsigned long long)calls,
               (unsigned long long)data, good ? "" : "  <- the laws fail");
        ok = ok && good;
    }
    // the chain of rejoins
    dvt_diverge_pos at[2] = {{1, 0}, {1, 0}};
    uint32_t segments = 0;
    for (; segments < 8; segments++) {
        Answer r{};
        report(prog, a, b, at[0], at[1], 0, DVT_DIVERGE_REJOIN, 0, 4, &r);
        ok = ok && lawful(r, 4, DVT_DIVERGE_DEFAULT_WINDOW);
        if (r.s.reason != DVT_DIV_SPLIT || r.s.rejoin_skip_a == DVT_DIVERGE_NO_REJOIN) break;
        at[0] = dvt_diverge_pos{r.s.rejoin_shard_a, r.s.rejoin_row_a};
        at[1] = dvt_diverge_pos{r.s.rejoin_shard_b, r.s.rejoin_row_b};
    }
    Answer self{};
    report(prog, a, a, {1, 0}, {1, 0}, 0, DVT_DIVERGE_REJOIN, 0, 64, &self);
    const bool same = lawful(self, 64, DVT_DIVERGE_DEFAULT_WINDOW) && self.s.n_data == 0 && (self.s.reason == DVT_DIV_END_BOTH || self.s.reason == DVT_DIV_BAD);
    printf("%s: a chain of %u rejoins; against itself %s\n", what, segments, same ? "nothing differs" : "  <- the laws fail");
    return ok && same;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: diverge_host GUEST.elf STDIN_A.bin STDIN_B.bin\n"); return 2; }
    std::vector<uint8_t> elf;
    if (!read_file(argv[1], &elf)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf.data(), elf.size(), &prog, &err)) { fprintf(stderr, "ELF: %s\n", err.c_str()); return 2; }
    Shards real[2], over[2];
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (int side = 0; side < 2; side++) {
        std::vector<std::vector<uint8_t>> stdin_bufs(1);
        if (!read_file(argv[2 + side], &stdin_bufs[0])) { fprintf(stderr, "cannot read %s\n", argv[2 + side]); return 2; }
        // (the shards as the host entry point takes them: what retired counts, also of a run that traps in the middle of a shard)
        constexpr uint32_t LOG_SHARD = 10;
        rv32::Vm vm(prog, &stdin_bufs, LOG_SHARD);
        vm.trace_unprovable = true;
        std::vector<rv32::CycleRec> buf((size_t)1 << LOG_SHARD);
        rv32::ShardOut so;
        so.recs = buf.data();
        Shards ran;
        for (;;) {
            vm.run_shard(true, &so, 1ull << 26);
            ran.emplace_back(so.recs, so.recs + so.n_recs);
            if (vm.halted || !vm.error.empty() || !vm.next_shard()) break;
        }
        printf("run %c: %llu cycles, %zu shards, %s\n", "AB"[side], (unsigned long long)vm.cycles, ran.size(), vm.halted ? "halted" : vm.error.c_str());
        for (auto &sh : ran) {
            real[side].push_back(sh);
            std::vector<rv32::CycleRec> recs = sh;   // the same records with one field of each overwritten
            for (auto &r : recs) {
                x ^= x << 13; x ^= x >> 7; x ^= x << 17;
                switch (x & 15) {
                case 0: r.idx = (uint32_t)(x >> 32); break;
                case 1: r.b = (uint32_t)(x >> 32); break;
                case 2: r.c = (uint32_t)(x >> 32); break;
                case 3: r.m_prev = (uint32_t)(x >> 32); break;
                case 4: r.b = rv32::ADDR_LIMIT - (uint32_t)((x >> 32) & 0xff); break;
                case 5: r.a = (uint32_t)(x >> 32); break;
                default: break;
                }
            }
            over[side].push_back(std::move(recs));
        }
        if (real[side].empty()) { fprintf(stderr, "run %c retired nothing\n", "AB"[side]); return 2; }
    }
    bool ok = sweep("as executed", prog, real[0], real[1], true);
    ok = sweep("overwritten", prog, over[0], over[1], false) && ok;
    ok = sweep("executed against overwritten", prog, real[0], over[1], false) && ok;
    return ok ? 0 : 1;
}
