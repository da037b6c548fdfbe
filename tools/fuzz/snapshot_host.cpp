// Stand-alone driver of the snapshot's host rule (csrc/snapshot.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-snapshot && build/asan/snapshot_host GUEST.elf [STDIN.bin ...]
// Runs the guest in trace mode (rv32::execute, shards of 2^12 cycles) and feeds every shard's cycle records to snap::Taker at
// ten positions (the first record, the second, span and shard edges, the middle, the end in three spellings), with ranges made
// of the words the execution accessed and of its image (at most 16 ranges and 4096 words); then feeds the same records with
// their fields overwritten by a fixed pseudo-random stream (instruction indices outside the text, addresses outside guest
// memory, unknown syscall ids, call arrays that leave guest memory), which the rule must count as bad or handle like any other
// record without reading or writing out of bounds.  Exit code 0 when, on the records as executed,
//   at the end position the registers equal the executor's final registers (the mem_init rows of the registers),
//   no cell except the NO_VALUE ones disagrees with the executor's final memory at the end, and at every position every
//   INITIAL cell shows the value the executor's memory argument starts the word with,
//   sources lie on their side of the position, (1, 0) has no frame and only INITIAL registers, and the three spellings of
//   the end give equal answers.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>

#include "../../dvt_circuits_amd/csrc/snapshot.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

struct Answer {
    dvt_snap_cell regs[32];
    std::vector<dvt_snap_cell> words;
    std::vector<dvt_snap_frame> frames;
    dvt_snap_summary s;
    uint64_t bad;
};

static bool take(const rv32::Program &prog, const std::vector<std::vector<rv32::CycleRec>> &shards, const std::vector<uint32_t> &next_pcs,
                 const std::vector<dvt_snap_range> &ranges, uint32_t shard, uint32_t row, size_t cap_frames, Answer *out) {
    snap::Ranges rg;
    std::string text;
    size_t n_words = 0;
    for (auto &r : ranges) n_words += (r.hi - r.lo) / 4;
    out->words.assign(n_words + 1, dvt_snap_cell{});
    out->frames.assign(cap_frames + 1, dvt_snap_frame{});
    if (snap::input_error(ranges.data(), ranges.size(), out->regs, out->words.data(), n_words, out->frames.data(), cap_frames, &rg, &text)) {
        fprintf(stderr, "the ranges are refused: %s\n", text.c_str());
        return false;
    }
    snap::Taker t(prog, rg, shard, row);
    for (size_t k = 0; k < shards.size(); k++) t.scan(prog, shards[k].data(), shards[k].size(), (uint32_t)k + 1, next_pcs[k]);
    t.emit(prog, 0.0, out->regs, out->words.data(), out->frames.data(), cap_frames, &out->s);
    out->words.resize(n_words);
    out->frames.resize(out->s.n_frames);
    out->bad = t.bad;
    return true;
}

static bool same_cells(const Answer &a, const Answer &b) {
    return !memcmp(a.regs, b.regs, sizeof a.regs) && a.words.size() == b.words.size() && a.frames.size() == b.frames.size() &&
           (a.words.empty() || !memcmp(a.words.data(), b.words.data(), a.words.size() * sizeof(dvt_snap_cell))) &&
           (a.frames.empty() || !memcmp(a.frames.data(), b.frames.data(), a.frames.size() * sizeof(dvt_snap_frame)));
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: snapshot_host GUEST.elf [STDIN.bin ...]\n"); return 2; }
    std::vector<uint8_t> elf;
    if (!read_file(argv[1], &elf)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<std::vector<uint8_t>> stdin_bufs(argc - 2);
    for (int i = 2; i < argc; i++)
        if (!read_file(argv[i], &stdin_bufs[i - 2])) { fprintf(stderr, "cannot read %s\n", argv[i]); return 2; }
    rv32::Program prog;
    std::string err;
    if (!rv32::load_elf(elf.data(), elf.size(), &prog, &err)) { fprintf(stderr, "ELF: %s\n", err.c_str()); return 2; }
    rv32::ExecResult res;
    rv32::execute(prog, stdin_bufs, true, 1ull << 26, 12, &res);
    if (!res.halted) { fprintf(stderr, "the guest did not halt: %s\n", res.error.c_str()); return 2; }
    std::vector<std::vector<rv32::CycleRec>> real, over;
    std::vector<uint32_t> next_pcs;
    for (auto &sh : res.shards) { real.push_back(sh.recs); next_pcs.push_back(sh.next_pc); }
    // the executor's own account of memory: per word the value it starts with and the value it ends with; the registers
    std::map<uint32_t, rv32::MemInitRow> rows;
    uint32_t final_reg[32] = {};
    for (const rv32::MemInitRow &m : res.mem_rows) {
        if (m.addr >= rv32::REG_BASE && m.addr < rv32::REG_BASE + 32) final_reg[m.addr - rv32::REG_BASE] = m.f;
        else if (m.addr < rv32::ADDR_LIMIT) rows[m.addr] = m;
    }
    // ranges: runs of up to 256 words from the words the executor lists (accessed words and the image), an unaligned-looking
    // but aligned range at the top of memory, a range nothing touches
    std::vector<dvt_snap_range> ranges;
    size_t total = 0;
    uint32_t covered = 0;
    for (auto &kv : rows) {
        if (ranges.size() >= DVT_SNAP_MAX_RANGES - 2 || total + 256 > DVT_SNAP_MAX_WORDS - 32) break;
        if (kv.first < covered || (kv.second.is_img && ranges.size() >= 4 && !kv.second.fsh)) continue;   // (most of the image is text nobody loads)
        const uint32_t hi = (uint32_t)std::min<uint64_t>((uint64_t)kv.first + 4 * 256, rv32::ADDR_LIMIT);
        ranges.push_back({kv.first, hi});
        total += (hi - kv.first) / 4;
        covered = hi;
    }
    ranges.push_back({rv32::ADDR_LIMIT - 64, rv32::ADDR_LIMIT});
    ranges.push_back({0x10, 0x50});
    const uint32_t S = (uint32_t)real.size(), last_n = S ? (uint32_t)real.back().size() : 0;
    const uint32_t places[][2] = {{1, 0}, {1, 1}, {1, 4095}, {2, 0}, {(S + 1) / 2, 2048}, {S, 0}, {S, last_n ? last_n - 1 : 0}, {S, last_n}, {S + 5, 0},
                                  {0xffffffffu, 0xffffffffu}};
    bool ok = true;
    Answer end{};
    for (auto &at : places) {
        Answer a{};
        if (!take(prog, real, next_pcs, ranges, at[0], at[1], 64, &a)) return 1;
        const unsigned long long P = watch::position(at[0], at[1]);
        bool good = !a.bad && a.s.cycles == res.cycles && a.s.position <= a.s.cycles && a.s.n_frames <= 64 && a.s.n_frames <= a.s.depth;
        const bool at_end = a.s.position == a.s.cycles;
        for (const dvt_snap_cell &c : a.words) {
            const auto it = rows.find(c.addr);
            if (c.flags & DVT_SNAP_NO_VALUE) { good = good && c.value == 0; continue; }
            good = good && it != rows.end();   // (a word with a value is a word the executor knows)
            if (it == rows.end()) continue;
            if (c.flags & DVT_SNAP_INITIAL) good = good && c.value == it->second.v;
            if (at_end) good = good && c.value == it->second.f;
            if (c.flags & DVT_SNAP_FROM_BEFORE) good = good && watch::position(c.shard, c.row) < P;
            if (c.flags & DVT_SNAP_FROM_AFTER) good = good && watch::position(c.shard, c.row) >= P;
        }
        for (uint32_t k = 1; k < 32; k++) {
            if (at_end) good = good && a.regs[k].value == final_reg[k];
            if (a.regs[k].flags & DVT_SNAP_FROM_BEFORE) good = good && watch::position(a.regs[k].shard, a.regs[k].row) < P;
            if (!a.s.position) good = good && a.regs[k].flags == DVT_SNAP_INITIAL;
        }
        if (!a.s.position) good = good && a.s.depth == 0;
        else good = good && a.s.depth >= 1 && (a.s.n_frames < a.s.depth || a.frames.back().call_pc == 0xffffffffu);
        if (at_end) {
            if (end.s.cycles) good = good && same_cells(a, end) && a.s.position == end.s.position;
            end = a;
        }
        printf("as executed at %u:%u: position=%llu of %llu depth=%u words=%u no_value=%u initial=%u untouched=%u%s\n", at[0], at[1],
               (unsigned long long)a.s.position, (unsigned long long)a.s.cycles, a.s.depth, a.s.n_words, a.s.no_value, a.s.initial, a.s.untouched,
               good ? "" : "  <- the laws fail");
        ok = ok && good;
    }
    if (!end.s.cycles) { fprintf(stderr, "no position was the end\n"); ok = false; }
    // the same records with one field of each overwritten
    uint64_t x = 0x9e3779b97f4a7c15ull;
    for (auto &sh : res.shards) {
        std::vector<rv32::CycleRec> recs = sh.recs;
        for (auto &r : recs) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            switch (x & 7) {
            case 0: r.idx = (uint32_t)(x >> 32); break;
            case 1: r.b = (uint32_t)(x >> 32); break;
            case 2: r.c = (uint32_t)(x >> 32); break;
            case 3: r.m_prev = (uint32_t)(x >> 32); break;
            case 4: r.b = rv32::ADDR_LIMIT - (uint32_t)((x >> 32) & 0xff); break;
            case 5: r.c = rv32::ADDR_LIMIT - (uint32_t)((x >> 32) & 0x1ff); break;
            default: break;
            }
        }
        over.push_back(std::move(recs));
    }
    for (auto &at : places)
        for (size_t cap_frames : {(size_t)0, (size_t)3, (size_t)512}) {
            Answer a{};
            if (!take(prog, over, next_pcs, ranges, at[0], at[1], cap_frames, &a)) return 1;
            const bool good = a.s.cycles == res.cycles && a.s.n_frames <= cap_frames && a.s.n_words == a.words.size();
            if (cap_frames == 3)
                printf("overwritten at %u:%u: bad=%llu depth=%u no_value=%u%s\n", at[0], at[1], (unsigned long long)a.bad, a.s.depth, a.s.no_value,
                       good ? "" : "  <- the laws fail");
            ok = ok && good;
        }
    return ok ? 0 : 1;
}
