// Stand-alone driver of the memory report's host rule (csrc/memreport.h) for AddressSanitizer / UBSan, on the CPU:
//   make -C dvt_circuits_amd/csrc asan-memreport && build/asan/memreport_host GUEST.elf [STDIN.bin ...]
// Runs the guest in trace mode (rv32::execute, shards of 2^12 cycles), feeds every shard's cycle records to
// memrep::tally_records and prints the summary; then feeds the same records with their fields overwritten by a fixed
// pseudo-random stream (instruction indices outside the text, addresses outside guest memory, unknown syscall ids), which
// the rule must count nothing for without reading or writing out of bounds.  Exit code 0 when the laws between the
// report's own outputs hold.
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../../dvt_circuits_amd/csrc/memreport.h"

using namespace dvt;

static bool read_file(const char *path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}

static bool laws(const rv32::Program &prog, const memrep::Tally &t, bool whole, const char *what) {
    std::vector<uint64_t> ft(t.first_touch.size());
    std::vector<dvt_memory_page> pages(t.pages.size());
    dvt_memory_summary s{};
    memrep::emit(prog, t, t.shards, whole, 0.0, memrep::Out{ft.data(), ft.size(), pages.data(), pages.size(), &s});
    uint64_t words = 0, first = 0, loads = 0;
    for (auto &p : pages) { words += p.words; first += p.first; loads += p.loads; }
    uint64_t ft_sum = 0;
    for (uint64_t x : ft) ft_sum += x;
    printf("%s: cycles=%llu loads=%llu stores=%llu pre_calls=%llu words=%llu first_touches=%llu pages=%u mem_init_rows=%llu sp_writes=%llu\n", what,
           (unsigned long long)s.cycles, (unsigned long long)s.loads, (unsigned long long)s.stores, (unsigned long long)s.pre_calls,
           (unsigned long long)s.words, (unsigned long long)s.first_touches, s.n_pages, (unsigned long long)s.mem_init_rows, (unsigned long long)s.sp_writes);
    const bool ok = words == s.words && first == s.first_touches && ft_sum == s.first_touches && loads == s.loads && s.n_pages == pages.size() &&
                    (!whole || s.mem_init_rows == 32 + s.image_words + s.words - s.image_words_accessed);
    if (!ok) fprintf(stderr, "%s: the report's outputs disagree\n", what);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: memreport_host GUEST.elf [STDIN.bin ...]\n"); return 2; }
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
    const std::vector<memrep::PreShape> shapes = memrep::pre_shapes();
    memrep::Tally t(prog);
    for (auto &sh : res.shards) memrep::tally_records(prog, shapes, sh.recs.data(), sh.recs.size(), &t);
    bool ok = laws(prog, t, true, "as executed");
    if (t.cycles != res.cycles) { fprintf(stderr, "cycles %llu, executed %llu\n", (unsigned long long)t.cycles, (unsigned long long)res.cycles); ok = false; }
    if (res.mem_rows.empty()) ok = false;
    {   // the height of mem_init against the executor's own table
        dvt_memory_summary s{};
        memrep::emit(prog, t, t.shards, true, 0.0, memrep::Out{nullptr, 0, nullptr, 0, &s});
        if (s.mem_init_rows != res.mem_rows.size()) { fprintf(stderr, "mem_init_rows %llu, the executor's table has %zu\n", (unsigned long long)s.mem_init_rows, res.mem_rows.size()); ok = false; }
    }
    // the same records with one field of each overwritten
    memrep::Tally bad(prog);
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
        memrep::tally_records(prog, shapes, recs.data(), recs.size(), &bad);
    }
    ok = laws(prog, bad, false, "overwritten") && ok;
    return ok ? 0 : 1;
}
