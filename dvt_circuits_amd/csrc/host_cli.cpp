// dvt_prover_host — the reference's CLI verbs (src/main.rs:58-106) over the C ABI.
//
//   dvt_prover_host prove   --type T -i INPUT.json [-o PROOF] [--elf GUEST.elf] [--devices D0,D1,...] [--compact]
//   dvt_prover_host execute --type T -i INPUT.json [--show-report] [--show-calls] [--show-memory] [--watch SPEC ...] [--snapshot S:R|exit [--dump ADDR+LEN ...] [--frames N]] [--origin SPEC [--depth N] [--nodes N] [--follow-addr]] [--uses SPEC [--depth N] [--fan N] [--nodes N] [--follow-addr]] [--elf GUEST.elf]
//   dvt_prover_host verify  --type T -i PROOF [--elf GUEST.elf]
//   dvt_prover_host compact --type T -i PROOF [-o PROOF] [--elf GUEST.elf]     (shared Merkle paths sent once: dvt_proof_compact)
//   dvt_prover_host expand  --type T -i PROOF [-o PROOF] [--elf GUEST.elf]     (the inverse; verify takes either form)
//   dvt_prover_host check   --type T -i INPUT.json [--show-report] [--show-calls] [--show-memory] [--watch SPEC ...] [--snapshot S:R|exit [--dump ADDR+LEN ...] [--frames N]] [--origin SPEC [--depth N] [--nodes N] [--follow-addr]] [--uses SPEC [--depth N] [--fan N] [--nodes N] [--follow-addr]] [--elf GUEST.elf] [--devices D0,D1,...]
//
// T = bad-share | finalization | bad-partial-key | bad-encrypted-share (clap names of CircuitType, :36-42).
// The reference embeds the four guest ELFs at build time (include_elf!, :115-118); they cannot be built in
// this image (no RISC-V toolchain), so the ELF comes from --elf or from $DVT_ELF_DIR/<type>.elf.
// Same contract as the reference: default proof path "<input>_proof.bin" (:468-470), "Proof saved to:" on
// success (:476), any error is printed and the process exits with code 1 (:421-427) — which is what the
// reference's 92 test vectors observe (script/run.sh:82-89).  `verify` has stock client.verify semantics
// (the reference's own verify sub-command re-executes the guest instead).
// --devices (prove only) spreads the shards of the execution over those GPUs (an index may repeat): the "devices" key of
// dvt_prover_create.
// check (no counterpart in the reference; SP1's debug_constraints) prepares the job as prove does and checks its trace rows
// against the AIR on the GPU (dvt_rv32_check_job) instead of proving: "clean: N shards, M chip tables, T ms" and exit code 0,
// or one line per finding and per unbalanced bus and exit code 1; after the bus lines, the tuples that do not cancel
// (dvt_rv32_job_bus_tuples): at most 32 lines, then "... and N more".
// --show-report: after execute's three report lines, and after check's verdict, the execution report (dvt_execute_profile on
// the host, dvt_rv32_job_profile on the GPU): "opcode counts (N total instructions):" and one "count name" line per RISC-V
// mnemonic, by count descending, then by name; then "syscall counts (N total syscall instructions):" with the ids of
// dvt_execute's syscall ABI named and any other in hex.  (The layout is this tool's: SP1's own text is not in the reference.)
// --show-calls: after that (or in its place), the call-tree report (dvt_execute_calltree on the host, dvt_rv32_job_calltree on the
// GPU): "call tree (N frames, depth D):" and one "inclusive self calls f_<pc>" line per function, by self cycles descending.
// --show-memory: after those (or in their place), the memory report (dvt_execute_memory on the host, dvt_rv32_job_memory on the
// GPU): one line "memory: cycles=N loads=N stores=N pre_reads=N pre_writes=N pre_calls=N words=N first_touches=N pages=N
// image_words=N image_words_accessed=N mem_init_rows=N sp_writes=N sp_min=0xX sp_max=0xX", then one line per run of
// consecutive accessed pages: "0xFIRST-0xLAST loads stores pre_reads pre_writes words" (byte addresses, LAST inclusive).
// --watch SPEC (repeatable, at most 16): after those, the watchpoint search (dvt_execute_watch on the host, dvt_rv32_job_watch on
// the GPU; csrc/watch.h).  SPEC is pc:ADDR[+BYTES], reg:NAME[=VALUE[/MASK]] (x1..x31 or an ABI name) or one of load: store: pread:
// pwrite: mem: followed by ADDR[+BYTES][=VALUE[/MASK]], as tools/watch_guest.py takes them.  Per spec one line
// "watch SPEC: total=N", then the last hits (at most 4), oldest first: "  SHARD:ROW pc=0xX rd=0xX rs1=0xX rs2=0xX" and, for a
// load or store, " load|store addr=0xX before=0xX after=0xX prev=SHARD:CLK", for a precompile call " call addr=0xX words=N".
// --snapshot S:R|exit: after those, the machine as it is before the record at shard S, row R executes, or after the last record
// (dvt_execute_snapshot on the host, dvt_rv32_job_snapshot on the GPU; csrc/snapshot.h).  --dump ADDR+LEN (repeatable, at most
// 16, 4096 words in all) names the memory to show, --frames N (default 16) how much of the call stack.  One line "snapshot:
// position=N cycles=N shard=S row=R pc=0xX depth=N frames=N unmatched_returns=N words=N no_value=N initial=N untouched=N", four
// lines "regs NAME=0xX ..." with x1..x31 by ABI name, one line per frame, innermost first: "#K 0xFN from 0xCALL ra=0xX opened
// S:R", and per dumped range lines "0xADDR: W W W W" of up to four words, ?? for a word the records do not hold (NO_VALUE).
// --origin S:R|exit, then :reg:NAME or :word:ADDR: after those, where the value that register or word holds before the position
// comes from (dvt_execute_origin on the host, dvt_rv32_job_origin on the GPU; csrc/origin.h).  --depth N (default 64) and --nodes N
// (default 1024) bound the slice, --follow-addr also follows the address registers of loads and stores.  One line "origin:
// position=N cycles=N shard=S row=R nodes=N edges=N depth=N cut=N unexpanded=N initial=N no_value=N questions=N levels=N
// passes=N", one line per node in discovery order: "node K depth=D at=S:R pc=0xX kind=op|load|store|call|syscall rd=0xX rs1=0xX
// rs2=0xX addr=0xX before=0xX after=0xX edges=FIRST+N flags=0xX", and one per edge, edge 0 the root: "edge K from=I to=J
// role=root|addr|rs1|rs2|mem target=0xX value=0xX flags=0xX src=S:R" (-1: no node).
// --uses S:R|exit, then :reg:NAME or :word:ADDR: who reads the value that register or word holds from the position on, and what
// those readers produce (dvt_execute_uses on the host, dvt_rv32_job_uses on the GPU; csrc/uses.h).  --depth, --nodes and
// --follow-addr as for --origin, --fan N (default 8, 1..16) the uses kept per definition.  One line "uses: position=N cycles=N
// shard=S row=R nodes=N defs=N edges=N depth=N cut=N unexpanded=N truncated=N live_at_exit=N no_value=N dead=N uses_total=N
// levels=N passes=N", one line per node in discovery order: "node K depth=D at=S:R pc=0xX kind=... rd=0xX rs1=0xX rs2=0xX
// addr=0xX before=0xX after=0xX defs=FIRST+N flags=0xX", one per definition, definition 0 the root: "def K node=I what=reg|word
// target=0xX value=0xX flags=0xX next=S:R uses=N edges=FIRST+N" (-1: no node, no next writer), and one per edge: "edge K def=I
// to=J role=addr|rs1|rs2|mem flags=0xX dst=S:R".
// diverge --type T -i A.json --against B.json --elf G [--host] [--from S:R --against-from S:R] [--rejoin N] [--keep K] [--log-shard L]
// [--devices D0,D1,...]: where the runs of one guest on two inputs part ways (dvt_rv32_job_diverge on two prepared jobs of one handle,
// with --host dvt_execute_diverge; csrc/diverge.h).  One block per lock-step segment: "diverge: pairs=N reason=split|bad|end_both|end_a|
// end_b|limit data=N first_data=K last_data=K mask=0xX load_diffs=N store_diffs=N stop_a=S:R stop_b=S:R cycles_a=N cycles_b=N
// rejoin_a=S:R rejoin_b=S:R skip_a=N skip_b=N" (-1: none), the deciding pair and the pair at the stop, one line per side ("deciding a:
// pc=0xX a=0xX b=0xX c=0xX m=0xX" or "none"), "live: NAME ..." with the registers that differ at the stop, and the first and last K
// (default 4) data pairs: "first|last k=K at=S:R/S:R pc=0xX mask=0xX a=0xX/0xX b=0xX/0xX c=0xX/0xX m=0xX/0xX" and, of a load or store,
// " load|store addr=0xX/0xX before=0xX/0xX after=0xX/0xX".  With --rejoin N the call is repeated from the rejoin positions up to N
// times.  The exit code is 0 whether or not the runs differ; only errors give 1.
// get-schema / validate-schema / node are product UI outside the accelerated path and are not provided.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/dvt_prover.h"

static bool read_file(const std::string &path, std::vector<uint8_t> *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    out->assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    return true;
}
static int die(const std::string &m) {
    fprintf(stderr, "Error: %s\n", m.c_str());
    return 1;
}
// bus and chip ids of the rv32 machine (tools/airgen/rv32.py)
static const char *const BUS_NAMES[] = {"?", "program", "byte", "mem", "image", "sys", "alu"};
static const char *const CHIP_NAMES[] = {"program", "byte", "cpu", "mem_image", "mem_init", "shift", "muldiv", "sha_extend", "sha_compress",
                                         "fp_op", "fp2_op", "bls_g1", "secp_k1", "u256_mul"};
static void print_bus_tuple(const dvt_bus_tuple &t) {
    printf("bus %s: (", t.bus < sizeof BUS_NAMES / sizeof *BUS_NAMES ? BUS_NAMES[t.bus] : "?");
    for (uint32_t k = 0; k < t.arity && k < DVT_LEDGER_MAX_ARITY; k++) printf(k ? " %u" : "%u", t.values[k]);
    printf(") net %u, sends %u, receives %u, first at ", t.net, t.n_send, t.n_recv);
    if (t.first_chip == 0xffffffffu) printf("the verifier's side\n");
    else printf("shard %u chip %s row %u interaction %u\n", t.first_tag, t.first_chip < sizeof CHIP_NAMES / sizeof *CHIP_NAMES ? CHIP_NAMES[t.first_chip] : "?",
                t.first_row, t.first_interaction);
}

// the syscall ids of the guest ABI (dvt_execute in include/dvt_prover.h; csrc/rv32.h)
static std::string syscall_name(uint32_t id) {
    static const struct { uint32_t id; const char *name; } NAMES[] = {
        {0x00, "halt"}, {0x02, "write"}, {0x10, "commit"}, {0x1A, "commit_deferred_proofs"}, {0xF0, "hint_len"}, {0xF1, "hint_read"},
        {0x00300105, "sha_extend"}, {0x00010106, "sha_compress"}, {0x0001010A, "secp256k1_add"}, {0x0000010B, "secp256k1_double"},
        {0x0001011D, "uint256_mul"}, {0x0001011E, "bls12381_add"}, {0x0000011F, "bls12381_double"}, {0x00010120, "bls12381_fp_add"},
        {0x00010121, "bls12381_fp_sub"}, {0x00010122, "bls12381_fp_mul"}, {0x00010123, "bls12381_fp2_add"}, {0x00010124, "bls12381_fp2_sub"},
        {0x00010125, "bls12381_fp2_mul"}};
    for (auto &n : NAMES)
        if (n.id == id) return n.name;
    char b[16];
    snprintf(b, sizeof b, "0x%08x", id);
    return b;
}
constexpr size_t REPORT_CAP = 64;   // opcodes (48 mnemonics and "unknown") and syscall ids (the library's bound) of a report
static void print_report(const dvt_profile_opcode *ops, const dvt_profile_syscall *sys, const dvt_profile_summary &s) {
    printf("opcode counts (%llu total instructions):\n", (unsigned long long)s.cycles);
    for (size_t i = 0; i < s.n_opcodes && i < REPORT_CAP; i++) printf("%12llu %s\n", (unsigned long long)ops[i].count, ops[i].name);   // (in the library's order)
    std::vector<std::pair<std::string, uint64_t>> calls;
    uint64_t total = 0;
    for (size_t i = 0; i < s.n_syscalls && i < REPORT_CAP; i++) {
        calls.emplace_back(syscall_name(sys[i].id), sys[i].count);
        total += sys[i].count;
    }
    std::sort(calls.begin(), calls.end(), [](const auto &a, const auto &b) { return a.second != b.second ? a.second > b.second : a.first < b.first; });
    printf("syscall counts (%llu total syscall instructions):\n", (unsigned long long)total);
    for (auto &c : calls) printf("%12llu %s\n", (unsigned long long)c.second, c.first.c_str());
}

// both sizes first, then the tables (call: dvt_execute_calltree or dvt_rv32_job_calltree with everything else bound)
template <class Call> static int print_calls(Call call) {
    dvt_calltree_summary s{};
    if (int rc = call(nullptr, 0, nullptr, 0, &s)) return rc;
    std::vector<dvt_calltree_func> funcs(s.n_funcs);
    if (int rc = call(nullptr, 0, funcs.data(), funcs.size(), &s)) return rc;
    printf("call tree (%llu frames, depth %u):\n", (unsigned long long)s.n_frames, s.max_depth);
    for (size_t i = 0; i < funcs.size() && i < s.n_funcs; i++)
        printf("%14llu %14llu %12llu f_%x\n", (unsigned long long)funcs[i].inclusive, (unsigned long long)funcs[i].self, (unsigned long long)funcs[i].calls, funcs[i].pc);
    if (s.dropped_frames) printf("(%llu frames dropped: no function table)\n", (unsigned long long)s.dropped_frames);
    return 0;
}

// the sizes first, then the pages (call: dvt_execute_memory or dvt_rv32_job_memory with everything else bound)
template <class Call> static int print_memory(Call call) {
    dvt_memory_summary s{};
    if (int rc = call(nullptr, 0, nullptr, 0, &s)) return rc;
    std::vector<dvt_memory_page> pages(s.n_pages);
    if (int rc = call(nullptr, 0, pages.data(), pages.size(), &s)) return rc;
    auto u = [](uint64_t v) { return (unsigned long long)v; };
    printf("memory: cycles=%llu loads=%llu stores=%llu pre_reads=%llu pre_writes=%llu pre_calls=%llu words=%llu first_touches=%llu pages=%u "
           "image_words=%llu image_words_accessed=%llu mem_init_rows=%llu sp_writes=%llu sp_min=0x%x sp_max=0x%x\n",
           u(s.cycles), u(s.loads), u(s.stores), u(s.pre_reads), u(s.pre_writes), u(s.pre_calls), u(s.words), u(s.first_touches), s.n_pages,
           u(s.image_words), u(s.image_words_accessed), u(s.mem_init_rows), u(s.sp_writes), s.sp_min, s.sp_max);
    const size_t n = std::min<size_t>(pages.size(), s.n_pages);
    for (size_t i = 0; i < n;) {   // a run of consecutive pages
        dvt_memory_page run = pages[i];
        size_t k = i + 1;
        for (; k < n && pages[k].page == pages[k - 1].page + s.page_bytes; k++) {
            run.loads += pages[k].loads; run.stores += pages[k].stores; run.pre_reads += pages[k].pre_reads; run.pre_writes += pages[k].pre_writes;
            run.words += pages[k].words;
        }
        printf("0x%08x-0x%08x %12llu %12llu %12llu %12llu %10u\n", run.page, pages[k - 1].page + s.page_bytes - 1, u(run.loads), u(run.stores),
               u(run.pre_reads), u(run.pre_writes), run.words);
        i = k;
    }
    return 0;
}

// a --watch spec as a query over every position; false: not a spec
static bool parse_watch(const std::string &spec, dvt_watch_query *q) {
    static const char *abi[32] = {"zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1", "a0", "a1", "a2", "a3", "a4", "a5",
                                  "a6", "a7", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9", "s10", "s11", "t3", "t4", "t5", "t6"};
    *q = dvt_watch_query{};
    q->to_shard = q->to_row = 0xffffffffu;
    const size_t colon = spec.find(':');
    if (colon == std::string::npos) return false;
    const std::string kind = spec.substr(0, colon);
    std::string rest = spec.substr(colon + 1);
    auto number = [](const std::string &t, uint32_t *out) {
        if (t.empty()) return false;
        char *end = nullptr;
        const unsigned long long v = strtoull(t.c_str(), &end, 0);
        *out = (uint32_t)v;
        return !*end && v <= 0xffffffffull;
    };
    const size_t eq = rest.find('=');
    if (eq != std::string::npos) {
        if (kind == "pc") return false;
        std::string v = rest.substr(eq + 1), m = "0xffffffff";
        rest = rest.substr(0, eq);
        const size_t slash = v.find('/');
        if (slash != std::string::npos) { m = v.substr(slash + 1); v = v.substr(0, slash); }
        if (!number(v, &q->want) || !number(m, &q->mask)) return false;
        q->flags |= DVT_WATCH_VALUE;
    }
    if (kind == "reg") {
        q->kind = DVT_WATCH_REG;
        for (uint32_t r = 1; r < 32; r++)
            if (rest == abi[r] || rest == "x" + std::to_string(r)) q->lo = r;
        q->hi = q->lo + 1;
        return q->lo != 0;
    }
    uint32_t bytes = 4;
    const size_t plus = rest.find('+');
    if (plus != std::string::npos && !number(rest.substr(plus + 1), &bytes)) return false;
    if (!number(rest.substr(0, plus), &q->lo)) return false;
    q->hi = q->lo + bytes;
    if (kind == "pc") { q->kind = DVT_WATCH_PC; return true; }
    q->kind = DVT_WATCH_MEM;
    q->lo &= ~3u;
    q->hi = (q->hi + 3) & ~3u;
    if (kind == "load") q->flags |= DVT_WATCH_LOAD;
    else if (kind == "store") q->flags |= DVT_WATCH_STORE;
    else if (kind == "pread") q->flags |= DVT_WATCH_PRE_READ;
    else if (kind == "pwrite") q->flags |= DVT_WATCH_PRE_WRITE;
    else if (kind == "mem") q->flags |= DVT_WATCH_LOAD | DVT_WATCH_STORE | DVT_WATCH_PRE_READ | DVT_WATCH_PRE_WRITE;
    else return false;
    return true;
}

// the totals and the last hits (call: dvt_execute_watch or dvt_rv32_job_watch with everything else bound)
template <class Call> static int print_watch(const std::vector<std::string> &specs, const std::vector<dvt_watch_query> &queries, Call call) {
    constexpr size_t KEEP = 4;
    std::vector<dvt_watch_hit> hits(2 * KEEP * queries.size());
    std::vector<uint64_t> totals(queries.size());
    dvt_watch_summary s{};
    if (int rc = call(queries.data(), queries.size(), KEEP, hits.data(), totals.data(), &s)) return rc;
    for (size_t q = 0; q < queries.size(); q++) {
        printf("watch %s: total=%llu\n", specs[q].c_str(), (unsigned long long)totals[q]);
        for (size_t i = 0; i < std::min<uint64_t>(KEEP, totals[q]); i++) {
            const dvt_watch_hit &h = hits[(2 * q + 1) * KEEP + i];
            printf("  %u:%u pc=0x%08x rd=0x%08x rs1=0x%08x rs2=0x%08x", h.shard, h.row, h.pc, h.rd_value, h.rs1, h.rs2);
            if (h.flags & (DVT_WATCH_LOAD | DVT_WATCH_STORE))
                printf(" %s addr=0x%08x before=0x%08x after=0x%08x prev=%u:%u", h.flags & DVT_WATCH_LOAD ? "load" : "store", h.addr, h.before, h.after,
                       h.prev_shard, h.prev_clk);
            else if (h.flags & DVT_WATCH_HIT_NO_VALUE) printf(" call addr=0x%08x words=%u", h.addr, h.n_words);
            printf("\n");
        }
    }
    return 0;
}

// a --snapshot position: S:R or exit
static bool parse_position(const std::string &t, uint32_t *shard, uint32_t *row) {
    if (t == "exit") { *shard = *row = 0xffffffffu; return true; }
    const size_t colon = t.find(':');
    if (colon == std::string::npos || colon == 0 || colon + 1 == t.size()) return false;
    char *e0 = nullptr, *e1 = nullptr;
    const unsigned long long s = strtoull(t.c_str(), &e0, 0), r = strtoull(t.c_str() + colon + 1, &e1, 0);
    *shard = (uint32_t)s; *row = (uint32_t)r;
    return e0 == t.c_str() + colon && !*e1 && s <= 0xffffffffull && r <= 0xffffffffull;
}
// a --dump ADDR+LEN as the range of the words that hold those bytes
static bool parse_dump(const std::string &t, dvt_snap_range *out) {
    const size_t plus = t.find('+');
    if (plus == std::string::npos || plus == 0 || plus + 1 == t.size()) return false;
    char *e0 = nullptr, *e1 = nullptr;
    const unsigned long long a = strtoull(t.c_str(), &e0, 0), n = strtoull(t.c_str() + plus + 1, &e1, 0);
    if (e0 != t.c_str() + plus || *e1 || !n || a + n > 0xffffffffull) return false;
    out->lo = (uint32_t)a & ~3u;
    out->hi = (uint32_t)((a + n + 3) & ~3ull);
    return true;
}

// the snapshot's block (call: dvt_execute_snapshot or dvt_rv32_job_snapshot with everything else bound)
template <class Call> static int print_snapshot(const std::vector<dvt_snap_range> &ranges, size_t n_frames, Call call) {
    static const char *abi[32] = {"zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1", "a0", "a1", "a2", "a3", "a4", "a5",
                                  "a6", "a7", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9", "s10", "s11", "t3", "t4", "t5", "t6"};
    size_t n_words = 0;
    for (auto &r : ranges) n_words += r.hi > r.lo ? (r.hi - r.lo) / 4 : 0;
    dvt_snap_cell regs[32];
    std::vector<dvt_snap_cell> words(std::max<size_t>(n_words, 1));
    std::vector<dvt_snap_frame> frames(std::max<size_t>(n_frames, 1));
    dvt_snap_summary s{};
    if (int rc = call(ranges.data(), ranges.size(), regs, words.data(), n_words, frames.data(), n_frames, &s)) return rc;
    printf("snapshot: position=%llu cycles=%llu shard=%u row=%u pc=0x%08x depth=%u frames=%u unmatched_returns=%u words=%u no_value=%u initial=%u untouched=%u\n",
           (unsigned long long)s.position, (unsigned long long)s.cycles, s.shard, s.row, s.pc, s.depth, s.n_frames, s.unmatched_returns, s.n_words,
           s.no_value, s.initial, s.untouched);
    for (uint32_t k = 1; k < 32; k++) printf("%s%s=0x%08x%s", k % 8 == 1 ? "regs " : "", abi[k], regs[k].value, k % 8 == 0 || k == 31 ? "\n" : " ");
    for (uint32_t f = 0; f < s.n_frames; f++)
        printf("#%u 0x%08x from 0x%08x ra=0x%08x opened %u:%u\n", f, frames[f].fn_pc, frames[f].call_pc, frames[f].ra, frames[f].open_shard, frames[f].open_row);
    size_t at = 0;
    for (auto &r : ranges)
        for (uint32_t k = 0; r.lo + 4 * k < r.hi; k++, at++) {
            if (k % 4 == 0) printf("0x%08x:", r.lo + 4 * k);
            if (words[at].flags & DVT_SNAP_NO_VALUE) printf(" ??");
            else printf(" %08x", words[at].value);
            if (k % 4 == 3 || r.lo + 4 * (k + 1) >= r.hi) printf("\n");
        }
    return 0;
}

// an --origin spec: POSITION:reg:NAME or POSITION:word:ADDR, POSITION = S:R or exit
struct OriginSpec { uint32_t shard, row, what, target; };
static bool parse_origin(const std::string &t, OriginSpec *out) {
    static const char *abi[32] = {"zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1", "a0", "a1", "a2", "a3", "a4", "a5",
                                  "a6", "a7", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9", "s10", "s11", "t3", "t4", "t5", "t6"};
    size_t at = t.find(":reg:");
    const bool reg = at != std::string::npos;
    if (!reg) at = t.find(":word:");
    if (at == std::string::npos || !parse_position(t.substr(0, at), &out->shard, &out->row)) return false;
    const std::string name = t.substr(at + (reg ? 5 : 6));
    if (reg) {
        out->what = DVT_ORIGIN_REG; out->target = 0;
        for (uint32_t r = 1; r < 32; r++)
            if (name == abi[r] || name == "x" + std::to_string(r)) out->target = r;
        return out->target != 0;
    }
    char *end = nullptr;
    const unsigned long long a = strtoull(name.c_str(), &end, 0);
    out->what = DVT_ORIGIN_WORD; out->target = (uint32_t)a & ~3u;
    return !name.empty() && !*end && a <= 0xffffffffull;
}

// the origin block (call: dvt_execute_origin or dvt_rv32_job_origin with everything else bound)
template <class Call> static int print_origin(size_t cap_nodes, Call call) {
    static const char *kinds[] = {"?", "op", "load", "store", "call", "syscall"}, *roles[] = {"root", "addr", "rs1", "rs2", "mem"};
    std::vector<dvt_origin_node> nodes(std::max<size_t>(cap_nodes, 1));
    std::vector<dvt_origin_edge> edges(DVT_ORIGIN_MAX_EDGES);
    dvt_origin_summary s{};
    if (int rc = call(nodes.data(), cap_nodes, edges.data(), edges.size(), &s)) return rc;
    printf("origin: position=%llu cycles=%llu shard=%u row=%u nodes=%u edges=%u depth=%u cut=%u unexpanded=%u initial=%u no_value=%u questions=%u levels=%u passes=%u\n",
           (unsigned long long)s.position, (unsigned long long)s.cycles, s.shard, s.row, s.n_nodes, s.n_edges, s.depth, s.cut, s.unexpanded, s.initial,
           s.no_value, s.questions, s.levels, s.passes);
    for (uint32_t i = 0; i < s.n_nodes; i++) {
        const dvt_origin_node &n = nodes[i];
        printf("node %u depth=%u at=%u:%u pc=0x%08x kind=%s rd=0x%08x rs1=0x%08x rs2=0x%08x addr=0x%08x before=0x%08x after=0x%08x edges=%u+%u flags=0x%x\n", i,
               n.depth, n.shard, n.row, n.pc, n.kind < 6 ? kinds[n.kind] : "?", n.rd_value, n.rs1, n.rs2, n.addr, n.before, n.after, n.first_edge, n.n_edges,
               n.flags);
    }
    for (uint32_t i = 0; i < s.n_edges; i++) {
        const dvt_origin_edge &e = edges[i];
        printf("edge %u from=%d to=%d role=%s target=0x%x value=0x%08x flags=0x%x src=%u:%u\n", i, (int)e.from, (int)e.to, e.role < 5 ? roles[e.role] : "?",
               e.target, e.value, e.flags, e.src_shard, e.src_row);
    }
    return 0;
}

// the uses block (call: dvt_execute_uses or dvt_rv32_job_uses with everything else bound)
template <class Call> static int print_uses(size_t cap_nodes, Call call) {
    static const char *kinds[] = {"?", "op", "load", "store", "call", "syscall"}, *roles[] = {"?", "addr", "rs1", "rs2", "mem"};
    std::vector<dvt_uses_node> nodes(std::max<size_t>(cap_nodes, 1));
    std::vector<dvt_uses_def> defs(DVT_USES_MAX_DEFS);
    std::vector<dvt_uses_edge> edges(DVT_USES_MAX_EDGES);
    dvt_uses_summary s{};
    if (int rc = call(nodes.data(), cap_nodes, defs.data(), defs.size(), edges.data(), edges.size(), &s)) return rc;
    printf("uses: position=%llu cycles=%llu shard=%u row=%u nodes=%u defs=%u edges=%u depth=%u cut=%u unexpanded=%u truncated=%u live_at_exit=%u no_value=%u dead=%u uses_total=%llu levels=%u passes=%u\n",
           (unsigned long long)s.position, (unsigned long long)s.cycles, s.shard, s.row, s.n_nodes, s.n_defs, s.n_edges, s.depth, s.cut, s.unexpanded, s.truncated,
           s.live_at_exit, s.no_value, s.dead, (unsigned long long)s.uses_total, s.levels, s.passes);
    for (uint32_t i = 0; i < s.n_nodes; i++) {
        const dvt_uses_node &n = nodes[i];
        printf("node %u depth=%u at=%u:%u pc=0x%08x kind=%s rd=0x%08x rs1=0x%08x rs2=0x%08x addr=0x%08x before=0x%08x after=0x%08x defs=%u+%u flags=0x%x\n", i,
               n.depth, n.shard, n.row, n.pc, n.kind < 6 ? kinds[n.kind] : "?", n.rd_value, n.rs1, n.rs2, n.addr, n.before, n.after, n.first_def, n.n_defs,
               n.flags);
    }
    for (uint32_t i = 0; i < s.n_defs; i++) {
        const dvt_uses_def &d = defs[i];
        printf("def %u node=%d what=%s target=0x%x value=0x%08x flags=0x%x next=%d:%d uses=%llu edges=%u+%u\n", i, (int)d.node, d.what == DVT_USES_REG ? "reg" : "word",
               d.target, d.value, d.flags, (int)d.next_shard, (int)d.next_row, (unsigned long long)d.n_uses, d.first_edge, d.n_edges);
    }
    for (uint32_t i = 0; i < s.n_edges; i++) {
        const dvt_uses_edge &e = edges[i];
        printf("edge %u def=%u to=%d role=%s flags=0x%x dst=%u:%u\n", i, e.def, (int)e.to, e.role < 5 ? roles[e.role] : "?", e.flags, e.dst_shard, e.dst_row);
    }
    return 0;
}

// one block of the diverge verb (call: dvt_execute_diverge or dvt_rv32_job_diverge with everything else bound); the summary in *out
template <class Call> static int print_diverge(size_t keep, Call call, dvt_diverge_summary *out) {
    static const char *REASONS[] = {"?", "split", "bad", "end_both", "end_a", "end_b", "limit"};
    static const char *REGS[32] = {"zero", "ra", "sp", "gp", "tp", "t0", "t1", "t2", "s0", "s1", "a0", "a1", "a2", "a3", "a4", "a5",
                                   "a6", "a7", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "s9", "s10", "s11", "t3", "t4", "t5", "t6"};
    std::vector<dvt_diverge_pair> first(std::max<size_t>(keep, 1)), last(std::max<size_t>(keep, 1));
    dvt_diverge_reg regs[32];
    dvt_diverge_summary s{};
    if (int rc = call(first.data(), last.data(), regs, &s)) return rc;
    auto num = [](uint64_t v) { return v == DVT_DIV_NONE ? -1ll : (long long)v; };
    auto pos = [](uint32_t v) { return v == DVT_DIVERGE_NO_REJOIN ? -1ll : (long long)v; };
    printf("diverge: pairs=%llu reason=%s data=%llu first_data=%lld last_data=%lld mask=0x%x load_diffs=%llu store_diffs=%llu stop_a=%u:%u stop_b=%u:%u "
           "cycles_a=%llu cycles_b=%llu rejoin_a=%lld:%lld rejoin_b=%lld:%lld skip_a=%lld skip_b=%lld\n",
           (unsigned long long)s.n_pairs, REASONS[s.reason <= 6 ? s.reason : 0], (unsigned long long)s.n_data, num(s.first_data), num(s.last_data), s.mask,
           (unsigned long long)s.n_load_diffs, (unsigned long long)s.n_store_diffs, s.stop_shard_a, s.stop_row_a, s.stop_shard_b, s.stop_row_b,
           (unsigned long long)s.cycles_a, (unsigned long long)s.cycles_b, pos(s.rejoin_shard_a), pos(s.rejoin_row_a), pos(s.rejoin_shard_b), pos(s.rejoin_row_b),
           pos(s.rejoin_skip_a), pos(s.rejoin_skip_b));
    auto rec = [](const char *what, const dvt_diverge_rec &r) {
        if (r.valid) printf("%s: pc=0x%x a=0x%x b=0x%x c=0x%x m=0x%x\n", what, r.pc, r.a, r.b, r.c, r.m_prev);
        else printf("%s: none\n", what);
    };
    rec("deciding a", s.prev_a); rec("deciding b", s.prev_b); rec("stop a", s.stop_a); rec("stop b", s.stop_b);
    printf("live:");
    for (int r = 1; r < 32; r++)
        if (regs[r].live) printf(" %s", REGS[r]);
    printf("\n");
    for (int half = 0; half < 2; half++)
        for (uint32_t i = 0; i < s.n_kept; i++) {
            const dvt_diverge_pair &e = (half ? last : first)[i];
            printf("%s k=%llu at=%u:%u/%u:%u pc=0x%x mask=0x%x a=0x%x/0x%x b=0x%x/0x%x c=0x%x/0x%x m=0x%x/0x%x", half ? "last" : "first", (unsigned long long)e.k,
                   e.shard_a, e.row_a, e.shard_b, e.row_b, e.pc, e.mask, e.a_a, e.a_b, e.b_a, e.b_b, e.c_a, e.c_b, e.m_a, e.m_b);
            if (e.dir) printf(" %s addr=0x%x/0x%x before=0x%x/0x%x after=0x%x/0x%x", e.dir == DVT_WATCH_LOAD ? "load" : "store", e.addr_a, e.addr_b, e.before_a,
                              e.before_b, e.after_a, e.after_b);
            printf("\n");
        }
    *out = s;
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return die("usage: dvt_prover_host prove|execute|verify|check|diverge|compact|expand --type T -i FILE [-o FILE] [--show-report] [--show-calls] [--show-memory] [--watch SPEC] [--snapshot S:R|exit] [--dump ADDR+LEN] [--frames N] [--origin SPEC] [--uses SPEC] [--depth N] [--fan N] [--nodes N] [--follow-addr] [--compact] [--keep-trees] [--elf FILE] [--devices D0,D1,...] [--device D] [--against FILE] [--host] [--from S:R] [--against-from S:R] [--rejoin N] [--keep K] [--log-shard L]");
    const std::string verb = argv[1];
    std::string type, input, output, elf_path, schema_path, devices, verify_device;
    bool show_report = false, show_calls = false, show_memory = false, auth = false, compact = false, keep_trees = false;
    std::vector<std::string> watch_specs;
    std::vector<dvt_watch_query> watch_queries;
    bool snapshot = false;
    uint32_t snap_shard = 0, snap_row = 0;
    size_t snap_frames = 16;
    std::vector<dvt_snap_range> snap_ranges;
    bool origin = false, uses = false;
    OriginSpec uses_spec{};
    uint32_t uses_fan = DVT_USES_DEFAULT_FAN;
    OriginSpec origin_spec{};
    uint32_t origin_depth = DVT_ORIGIN_MAX_DEPTH, origin_flags = 0;
    size_t origin_nodes = DVT_ORIGIN_MAX_NODES;
    std::string against;
    bool host_only = false;
    dvt_diverge_pos div_from[2] = {{1, 0}, {1, 0}};
    uint32_t div_rejoin = 0, div_log_shard = 0;
    size_t div_keep = 4;
    for (int i = 2; i < argc; i++) {
        std::string a = argv[i], inline_val;
        bool has_inline = false;
        if (a.rfind("--", 0) == 0) {   // --key=value, as the reference's test vectors write it (clap accepts both forms)
            size_t eq = a.find('=');
            if (eq != std::string::npos) { inline_val = a.substr(eq + 1); a = a.substr(0, eq); has_inline = true; }
        }
        auto next = [&]() -> std::string { return has_inline ? inline_val : (i + 1 < argc ? std::string(argv[++i]) : std::string()); };
        if (a == "--type") type = next();
        else if (a == "-i" || a == "--input-file") input = next();
        else if (a == "-o" || a == "--output-file-path") output = next();
        else if (a == "--elf") elf_path = next();
        else if (a == "--devices") devices = next();
        else if (a == "--device") verify_device = next();   // verify: the query part on that GPU (dvt_prover_verify)
        else if (a == "--show-report") show_report = true;
        else if (a == "--show-calls") show_calls = true;
        else if (a == "--show-memory") show_memory = true;
        else if (a == "--watch") {
            watch_specs.push_back(next());
            watch_queries.emplace_back();
            if (!parse_watch(watch_specs.back(), &watch_queries.back())) return die("no watch spec: " + watch_specs.back());
        }
        else if (a == "--snapshot") {
            const std::string t = next();
            if (!parse_position(t, &snap_shard, &snap_row)) return die("no position (S:R or exit): " + t);
            snapshot = true;
        }
        else if (a == "--dump") {
            const std::string t = next();
            snap_ranges.emplace_back();
            if (!parse_dump(t, &snap_ranges.back())) return die("no range (ADDR+LEN): " + t);
        }
        else if (a == "--frames") snap_frames = (size_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--origin") {
            const std::string t = next();
            if (!parse_origin(t, &origin_spec)) return die("no origin (S:R|exit, then :reg:NAME or :word:ADDR): " + t);
            origin = true;
        }
        else if (a == "--uses") {
            const std::string t = next();
            if (!parse_origin(t, &uses_spec)) return die("no uses (S:R|exit, then :reg:NAME or :word:ADDR): " + t);
            uses = true;
        }
        else if (a == "--fan") uses_fan = (uint32_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--depth") origin_depth = (uint32_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--nodes") origin_nodes = (size_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--follow-addr") origin_flags |= DVT_ORIGIN_FOLLOW_ADDR;
        else if (a == "--against") against = next();
        else if (a == "--host") host_only = true;
        else if (a == "--from" || a == "--against-from") {
            const std::string t = next();
            dvt_diverge_pos &at = div_from[a == "--from" ? 0 : 1];
            if (t == "exit" || !parse_position(t, &at.shard, &at.row)) return die("no position (S:R): " + t);
        }
        else if (a == "--rejoin") div_rejoin = (uint32_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--keep") div_keep = (size_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--log-shard") div_log_shard = (uint32_t)strtoull(next().c_str(), nullptr, 0);
        else if (a == "--compact") compact = true;       // prove: shard proofs in the compact form ("compact_openings")
        else if (a == "--keep-trees") keep_trees = true;  // prove / check: shards that do not fit in HBM in full keep their main Merkle tree ("keep_phase1": 2)
        else if (a == "--auth-commitment") auth = true;  // the reference selects this at build time (cargo feature)
        else if (a == "--json-schema-file") schema_path = next();
        else return die("unknown argument " + a);
    }
    const bool transcode = verb == "compact" || verb == "expand";   // -i: a proof; -o: the proof in the other form
    if (verb != "prove" && verb != "execute" && verb != "verify" && verb != "check" && verb != "diverge" && !transcode) return die("unknown sub-command " + verb);
    if (type.empty() || input.empty()) return die("--type and --input-file are required");
    if (elf_path.empty()) {
        const char *dir = getenv("DVT_ELF_DIR");
        if (!dir) return die("no guest ELF: pass --elf or set DVT_ELF_DIR (the reference embeds its guests at build time)");
        elf_path = std::string(dir) + "/" + type + ".elf";
    }
    std::vector<uint8_t> elf, in;
    if (!read_file(elf_path, &elf)) return die("cannot read ELF " + elf_path);
    if (!read_file(input, &in)) return die("cannot read " + input);

    if (!schema_path.empty() && verb != "verify" && !transcode) {  // validate_if_needed (src/main.rs:509-541)
        std::vector<uint8_t> sch;
        if (!read_file(schema_path, &sch)) return die("Could not read schema file '" + schema_path + "'");
        char *verr = nullptr;
        if (dvt_json_schema_validate((const char *)sch.data(), sch.size(), (const char *)in.data(), in.size(), &verr)) {
            std::string all = verr ? verr : "?";
            size_t at = 0;
            while (at <= all.size()) {
                size_t e = all.find('\n', at);
                fprintf(stderr, "Validation error in '%s': %s\n", input.c_str(), all.substr(at, e == std::string::npos ? std::string::npos : e - at).c_str());
                if (e == std::string::npos) break;
                at = e + 1;
            }
            return die("JSON validation failed for '" + input + "'");
        }
    }

    if (verb == "verify" || transcode) {
        dvt_prover *p = nullptr;
        const std::string vcfg = "{\"device\": " + std::to_string(atoi(verify_device.c_str())) + "}";
        if (dvt_prover_create(verify_device.empty() ? nullptr : vcfg.c_str(), &p)) return die(dvt_last_error(nullptr));
        dvt_pk *pk = nullptr;
        uint8_t *vk = nullptr;
        size_t vk_len = 0;
        if (dvt_setup(p, elf.data(), elf.size(), &pk, &vk, &vk_len)) return die(dvt_last_error(p));
        char *why = nullptr;
        if (transcode) {   // either form in, the named form out; verify takes both unchanged
            uint8_t *out = nullptr;
            size_t out_len = 0;
            const int rc = (verb == "compact" ? dvt_proof_compact : dvt_proof_expand)(vk, vk_len, in.data(), in.size(), 100, 16, &out, &out_len, &why);
            if (rc) return die(std::string("Proof rejected: ") + (why ? why : "?"));
            const std::string path = output.empty() ? input + (verb == "compact" ? "_compact.bin" : "_plain.bin") : output;
            std::ofstream f(path, std::ios::binary);
            if (!f || !f.write((const char *)out, (std::streamsize)out_len)) return die("Saving proof failed: " + path);
            printf("Proof saved to: %s (%zu -> %zu bytes)\n", path.c_str(), in.size(), out_len);
            return 0;
        }
        int32_t ec = 0;
        int rc = verify_device.empty() ? dvt_verify(vk, vk_len, in.data(), in.size(), 100, 16, &ec, nullptr, nullptr, &why)
                                       : dvt_prover_verify(p, vk, vk_len, in.data(), in.size(), 100, 16, &ec, nullptr, nullptr, &why);
        if (rc == DVT_ERR_DEVICE) return die(dvt_last_error(p));
        if (rc) return die(std::string("Verification failed: ") + (why ? why : "?"));
        printf("Proof verified (guest exit code %d)\n", ec);
        return 0;
    }

    uint8_t *stdin_buf = nullptr;
    size_t stdin_len = 0;
    char *err = nullptr;
    if (dvt_stdin_from_json(type.c_str(), (const char *)in.data(), in.size(), auth, &stdin_buf, &stdin_len, &err))
        return die(std::string("Failed to read input: ") + (err ? err : "?"));
    dvt_buf buf{stdin_buf, stdin_len};

    if (verb == "diverge") {
        std::vector<uint8_t> in_b;
        if (against.empty() || !read_file(against, &in_b)) return die("diverge needs --against FILE: cannot read '" + against + "'");
        uint8_t *stdin_b = nullptr;
        size_t len_b = 0;
        if (dvt_stdin_from_json(type.c_str(), (const char *)in_b.data(), in_b.size(), auth, &stdin_b, &len_b, &err))
            return die(std::string("Failed to read input: ") + (err ? err : "?"));
        if (div_keep > DVT_DIVERGE_MAX_KEEP) return die("--keep is at most " + std::to_string(DVT_DIVERGE_MAX_KEEP));
        dvt_buf buf_b{stdin_b, len_b};
        dvt_prover *p = nullptr;
        dvt_pk *pk = nullptr;
        dvt_job *jobs[2] = {nullptr, nullptr};
        if (!host_only) {
            std::string cfg;
            if (!devices.empty()) cfg += "\"devices\": [" + devices + "]";
            if (div_log_shard) cfg += std::string(cfg.empty() ? "" : ", ") + "\"log_shard_size\": " + std::to_string(div_log_shard);
            const bool plain = cfg.empty();
            cfg = "{" + cfg + "}";
            if (dvt_prover_create(plain ? nullptr : cfg.c_str(), &p)) return die(dvt_last_error(nullptr));
            if (dvt_setup(p, elf.data(), elf.size(), &pk, nullptr, nullptr)) return die(dvt_last_error(p));
            // (a run that traps or exits non-zero leaves no job to compare: --host is the way for those)
            dvt_report rep{};
            if (dvt_rv32_prepare(p, pk, &buf, 1, &jobs[0], &rep) || dvt_rv32_prepare(p, pk, &buf_b, 1, &jobs[1], &rep))
                return die(std::string("Preparing the job failed: ") + dvt_last_error(p));
        }
        dvt_diverge_pos at[2] = {div_from[0], div_from[1]};
        for (uint32_t round = 0; round <= div_rejoin; round++) {
            dvt_diverge_summary s{};
            char *derr = nullptr;
            if (print_diverge(div_keep, [&](dvt_diverge_pair *first, dvt_diverge_pair *last, dvt_diverge_reg *regs, dvt_diverge_summary *sum) {
                    return host_only ? dvt_execute_diverge(elf.data(), elf.size(), stdin_buf, stdin_len, stdin_b, len_b, 0, div_log_shard, at[0], at[1], 0,
                                                           DVT_DIVERGE_REJOIN, 0, div_keep, first, last, regs, sum, nullptr, nullptr, &derr)
                                     : dvt_rv32_job_diverge(p, pk, jobs[0], jobs[1], at[0], at[1], 0, DVT_DIVERGE_REJOIN, 0, div_keep, first, last, regs, sum);
                }, &s))
                return die(std::string("Divergence failed: ") + (host_only ? (derr ? derr : "?") : dvt_last_error(p)));
            if (s.reason != DVT_DIV_SPLIT || s.rejoin_skip_a == DVT_DIVERGE_NO_REJOIN) break;
            at[0] = dvt_diverge_pos{s.rejoin_shard_a, s.rejoin_row_a};
            at[1] = dvt_diverge_pos{s.rejoin_shard_b, s.rejoin_row_b};
        }
        if (p) {
            dvt_job_free(p, jobs[0]);
            dvt_job_free(p, jobs[1]);
            dvt_pk_free(p, pk);
            dvt_prover_destroy(p);
        }
        return 0;
    }

    if (verb == "execute") {
        printf("input len: %zu\n", stdin_len - 8);  // the reference prints the CBOR length (src/main.rs:436)
        dvt_report rep{};
        dvt_profile_opcode ops[REPORT_CAP];
        dvt_profile_syscall sys[REPORT_CAP];
        dvt_profile_summary sum{};
        int rc = show_report ? dvt_execute_profile(elf.data(), elf.size(), &buf, 1, 0, nullptr, 0, nullptr, 0, sys, REPORT_CAP, ops, REPORT_CAP, &sum, &rep, &err)
                             : dvt_execute(elf.data(), elf.size(), &buf, 1, 0, nullptr, nullptr, &rep, &err);
        if (rc) return die(std::string("Verification failed: ") + (err ? err : "?"));
        if (show_report) {
            printf("Verification report:\ntotal instructions: %llu\nexit code: %d\n", (unsigned long long)rep.cycles, rep.exit_code);
            print_report(ops, sys, sum);
        }
        if (show_calls) {
            char *cerr = nullptr;
            if (print_calls([&](dvt_calltree_arc *arcs, size_t cap_arcs, dvt_calltree_func *funcs, size_t cap_funcs, dvt_calltree_summary *s) {
                    return dvt_execute_calltree(elf.data(), elf.size(), &buf, 1, 0, arcs, cap_arcs, funcs, cap_funcs, s, nullptr, &cerr);
                }))
                return die(std::string("Verification failed: ") + (cerr ? cerr : "?"));
        }
        if (show_memory) {
            char *merr = nullptr;
            if (print_memory([&](uint64_t *ft, size_t cap_instr, dvt_memory_page *pages, size_t cap_pages, dvt_memory_summary *s) {
                    return dvt_execute_memory(elf.data(), elf.size(), &buf, 1, 0, ft, cap_instr, pages, cap_pages, s, nullptr, &merr);
                }))
                return die(std::string("Verification failed: ") + (merr ? merr : "?"));
        }
        if (!watch_queries.empty()) {
            char *werr = nullptr;
            if (print_watch(watch_specs, watch_queries, [&](const dvt_watch_query *q, size_t n, size_t keep, dvt_watch_hit *hits, uint64_t *totals, dvt_watch_summary *s) {
                    return dvt_execute_watch(elf.data(), elf.size(), &buf, 1, 0, 0, q, n, keep, hits, totals, s, nullptr, &werr);
                }))
                return die(std::string("Verification failed: ") + (werr ? werr : "?"));
        }
        if (snapshot) {
            char *serr = nullptr;
            if (print_snapshot(snap_ranges, snap_frames, [&](const dvt_snap_range *r, size_t n, dvt_snap_cell *regs, dvt_snap_cell *words, size_t cap_words,
                                                             dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *s) {
                    return dvt_execute_snapshot(elf.data(), elf.size(), &buf, 1, 0, 0, snap_shard, snap_row, r, n, regs, words, cap_words, frames, cap_frames, s,
                                                nullptr, &serr);
                }))
                return die(std::string("Verification failed: ") + (serr ? serr : "?"));
        }
        if (origin) {
            char *oerr = nullptr;
            if (print_origin(origin_nodes, [&](dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges, dvt_origin_summary *s) {
                    return dvt_execute_origin(elf.data(), elf.size(), &buf, 1, 0, 0, origin_spec.shard, origin_spec.row, origin_spec.what, origin_spec.target,
                                              origin_flags, origin_depth, nodes, cap_nodes, edges, cap_edges, s, nullptr, &oerr);
                }))
                return die(std::string("Verification failed: ") + (oerr ? oerr : "?"));
        }
        if (uses) {
            char *uerr = nullptr;
            if (print_uses(origin_nodes, [&](dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges, size_t cap_edges,
                                             dvt_uses_summary *s) {
                    return dvt_execute_uses(elf.data(), elf.size(), &buf, 1, 0, 0, uses_spec.shard, uses_spec.row, uses_spec.what, uses_spec.target, origin_flags,
                                            origin_depth, uses_fan, nodes, cap_nodes, defs, cap_defs, edges, cap_edges, s, nullptr, &uerr);
                }))
                return die(std::string("Verification failed: ") + (uerr ? uerr : "?"));
        }
        return 0;
    }

    dvt_prover *p = nullptr;
    // (the library checks the list; without either option the handle is made as before, from no config at all)
    std::string cfg;
    if (!devices.empty()) cfg += "\"devices\": [" + devices + "]";
    if (compact) cfg += std::string(cfg.empty() ? "" : ", ") + "\"compact_openings\": 1";
    if (keep_trees) cfg += std::string(cfg.empty() ? "" : ", ") + "\"keep_phase1\": 2";
    const bool plain = cfg.empty();
    cfg = "{" + cfg + "}";
    if (dvt_prover_create(plain ? nullptr : cfg.c_str(), &p)) return die(dvt_last_error(nullptr));
    dvt_pk *pk = nullptr;
    if (dvt_setup(p, elf.data(), elf.size(), &pk, nullptr, nullptr)) return die(dvt_last_error(p));
    if (verb == "check") {
        dvt_job *job = nullptr;
        dvt_report rep{};
        if (dvt_rv32_prepare(p, pk, &buf, 1, &job, &rep)) return die(std::string("Preparing the job failed: ") + dvt_last_error(p));
        std::vector<dvt_check_finding> found(256);
        dvt_check_summary sum{};
        const int rc = dvt_rv32_check_job(p, pk, job, found.data(), found.size(), &sum);
        if (rc && rc != DVT_ERR_REJECTED) return die(std::string("Check failed: ") + dvt_last_error(p));
        const size_t shards = dvt_rv32_job_shards(job);
        size_t tables = 0;
        for (size_t i = 0; i < shards; i++) tables += (size_t)__builtin_popcount(dvt_rv32_job_shard_chips(job, i));
        if (rc == DVT_OK) printf("clean: %zu shards, %zu chip tables, %.2f ms\n", shards, tables, sum.ms);
        for (size_t i = 0; i < sum.n_findings && i < found.size(); i++)
            printf("shard %u chip %u (2^%u rows): %llu violations, first at row %u, constraint %d\n", found[i].shard, found[i].chip, found[i].log_n,
                   (unsigned long long)found[i].r.violations, found[i].r.first_row, found[i].r.first_constraint);
        if (sum.n_findings > found.size()) printf("... and %zu more chip tables with violations\n", sum.n_findings - found.size());
        for (uint32_t b = 0; b < DVT_CHECK_BUSES; b++)
            if (sum.unbalanced_buses >> b & 1) printf("bus %u: the LogUp sums over all chips and shards do not balance\n", b);
        if (sum.unbalanced_buses) {   // the tuples behind the mask (the bus ledger)
            std::vector<dvt_bus_tuple> tuples(4096);
            size_t n = 0;
            uint32_t truncated = 0;
            if (dvt_rv32_job_bus_tuples(p, pk, job, tuples.data(), tuples.size(), &n, &truncated)) return die(std::string("Check failed: ") + dvt_last_error(p));
            for (size_t i = 0; i < n && i < 32; i++) print_bus_tuple(tuples[i]);
            if (n > 32) printf("... and %zu more%s\n", n - 32, truncated ? " (at least: the ledger was truncated)" : "");
        }
        if (show_report) {
            dvt_profile_opcode ops[REPORT_CAP];
            dvt_profile_syscall sys[REPORT_CAP];
            dvt_profile_summary psum{};
            if (dvt_rv32_job_profile(p, pk, job, 0, nullptr, 0, nullptr, 0, sys, REPORT_CAP, ops, REPORT_CAP, &psum)) return die(std::string("Report failed: ") + dvt_last_error(p));
            print_report(ops, sys, psum);
        }
        if (show_calls &&
            print_calls([&](dvt_calltree_arc *arcs, size_t cap_arcs, dvt_calltree_func *funcs, size_t cap_funcs, dvt_calltree_summary *s) {
                return dvt_rv32_job_calltree(p, pk, job, 0, arcs, cap_arcs, funcs, cap_funcs, s);
            }))
            return die(std::string("Call tree failed: ") + dvt_last_error(p));
        if (show_memory &&
            print_memory([&](uint64_t *ft, size_t cap_instr, dvt_memory_page *pages, size_t cap_pages, dvt_memory_summary *s) {
                return dvt_rv32_job_memory(p, pk, job, ft, cap_instr, pages, cap_pages, s);
            }))
            return die(std::string("Memory report failed: ") + dvt_last_error(p));
        if (!watch_queries.empty() &&
            print_watch(watch_specs, watch_queries, [&](const dvt_watch_query *q, size_t n, size_t keep, dvt_watch_hit *hits, uint64_t *totals, dvt_watch_summary *s) {
                return dvt_rv32_job_watch(p, pk, job, q, n, keep, hits, totals, s);
            }))
            return die(std::string("Watch failed: ") + dvt_last_error(p));
        if (snapshot &&
            print_snapshot(snap_ranges, snap_frames, [&](const dvt_snap_range *r, size_t n, dvt_snap_cell *regs, dvt_snap_cell *words, size_t cap_words,
                                                         dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *s) {
                return dvt_rv32_job_snapshot(p, pk, job, snap_shard, snap_row, r, n, regs, words, cap_words, frames, cap_frames, s);
            }))
            return die(std::string("Snapshot failed: ") + dvt_last_error(p));
        if (origin &&
            print_origin(origin_nodes, [&](dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges, dvt_origin_summary *s) {
                return dvt_rv32_job_origin(p, pk, job, origin_spec.shard, origin_spec.row, origin_spec.what, origin_spec.target, origin_flags, origin_depth,
                                           nodes, cap_nodes, edges, cap_edges, s);
            }))
            return die(std::string("Origin failed: ") + dvt_last_error(p));
        if (uses &&
            print_uses(origin_nodes, [&](dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges, size_t cap_edges,
                                         dvt_uses_summary *s) {
                return dvt_rv32_job_uses(p, pk, job, uses_spec.shard, uses_spec.row, uses_spec.what, uses_spec.target, origin_flags, origin_depth, uses_fan, nodes,
                                         cap_nodes, defs, cap_defs, edges, cap_edges, s);
            }))
            return die(std::string("Uses failed: ") + dvt_last_error(p));
        dvt_job_free(p, job);
        dvt_pk_free(p, pk);
        dvt_prover_destroy(p);
        return rc ? 1 : 0;
    }
    uint8_t *proof = nullptr;
    size_t proof_len = 0;
    dvt_report rep{};
    if (dvt_prove_core(p, pk, &buf, 1, &proof, &proof_len, &rep)) return die(std::string("Proof generation failed: ") + dvt_last_error(p));
    const std::string path = output.empty() ? input + "_proof.bin" : output;
    std::ofstream f(path, std::ios::binary);
    if (!f || !f.write((const char *)proof, (std::streamsize)proof_len)) return die("Saving proof failed: " + path);
    printf("Proof saved to: %s\n", path.c_str());
    dvt_free(proof);
    dvt_pk_free(p, pk);
    dvt_prover_destroy(p);
    return 0;
}
