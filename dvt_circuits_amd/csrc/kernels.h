// Internal launch interface between the C-ABI layer (capi.hip) and the gfx950
// kernels.  Not installed; the public surface is include/dvt_prover.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bb.cuh"
#include "poseidon2.cuh"

namespace dvt {

// Device-resident two-level power tables (built once per prover handle).
//   Omega = primitive 2^24-th root:  Omega^e = tw_hi[e >> 12] * tw_lo[e & 4095]
//   g = 31 (coset shift):            g^k     = sh_hi[k >> 12] * sh_lo[k & 4095], k < 2^23
//   lde_tw:    for every transform size 2^l, 1 <= l <= 13, the 2^(l-1) twiddles w_{2^l}^e at offset 2^(l-1) - 1
//   lde_scale: for every (shift_mode, log_n) the per-position coefficient scaling of lde_block (4096 words each,
//              at ((mode * LDE_MAX_LOG + log_n) << 12)): see ntt.hip
constexpr uint32_t LDE_MAX_LOG = 23;
struct NttTables {
    uint32_t *base = nullptr;
    const uint32_t *tw_hi = nullptr, *tw_lo = nullptr, *sh_hi = nullptr, *sh_lo = nullptr;
    const uint32_t *lde_tw = nullptr, *lde_scale = nullptr;      // Montgomery words
    const uint32_t *lde_tw_c = nullptr, *lde_scale_c = nullptr;  // the same as centred canonical residues (two's complement)
};
hipError_t ntt_tables_create(NttTables *t);
void ntt_tables_destroy(NttTables *t);

// ntt.hip
hipError_t launch_coset_lde(hipStream_t st, const NttTables &tabs, uint32_t *d_in, uint32_t *d_scratch, uint32_t *d_out,
                            uint32_t width, uint32_t log_n, uint32_t shift_mode);
hipError_t launch_to_internal(hipStream_t st, uint32_t *d, size_t n);
hipError_t launch_from_internal(hipStream_t st, uint32_t *d, size_t n);

// merkle.hip
// Row sponges of ONE tree in one launch: the leaves (the tallest matrices) and, for every lower level where shorter matrices
// join the tree, the digests of their rows ("injected" at that level by launch_merkle_level / launch_merkle_top).  A short
// and wide table (a precompile chip: 2^14 rows of 1245 columns = 156 sequential permutations per row on a few hundred
// waves) is latency-bound on its own; in the same launch as the tall leaves its chain hides behind them.  Segments run in
// the order given (the launch puts the longest chains first).
constexpr uint32_t MERKLE_TOP_LOG = 6;   // below this the levels share one single-workgroup launch (16 lanes per node)
constexpr uint32_t MERKLE_COOP_LOG = 13; // levels of at most 2^13 nodes run one node per 16 lanes (latency-, not throughput-bound)
constexpr uint32_t MERKLE_MAX_SEGMENTS = 24;
struct MerkleLeafSegments {
    uint32_t n = 0;
    const uint32_t *const *cols[MERKLE_MAX_SEGMENTS];   // device array of `ncols` column base pointers (2^log_h words each)
    uint32_t *out[MERKLE_MAX_SEGMENTS];                 // [2^log_h][8] digests
    uint32_t ncols[MERKLE_MAX_SEGMENTS], log_h[MERKLE_MAX_SEGMENTS];
    uint32_t coop[MERKLE_MAX_SEGMENTS];                 // set by the launch: 16 lanes per row
    uint32_t block0[MERKLE_MAX_SEGMENTS + 1];           // set by the launch: first workgroup of every segment
    void add(const uint32_t *const *c, uint32_t nc, uint32_t lh, uint32_t *o) { cols[n] = c; ncols[n] = nc; log_h[n] = lh; out[n] = o; n++; }
};
hipError_t launch_merkle_leaves(hipStream_t st, MerkleLeafSegments sg);
// d_out[i] = compress(prev[i], prev[i + len]); with d_inject additionally
// d_out[i] = compress(d_out[i], d_inject[i])   (d_inject: the row digests of the matrices that join at this level)
hipError_t launch_merkle_level(hipStream_t st, const uint32_t *d_prev, const uint32_t *d_inject, uint32_t log_len, uint32_t *d_out);
// every level below a layer of 2^log_start <= 2^MERKLE_TOP_LOG nodes, down to the root, in one launch
struct MerkleTopInject {  // per level lh (nodes = 2^lh): row digests injected at that level (or nullptr)
    const uint32_t *digests[MERKLE_TOP_LOG + 1] = {};
};
hipError_t launch_merkle_top(hipStream_t st, uint32_t *d_layer, uint32_t log_start, const MerkleTopInject &inj);
hipError_t launch_poseidon2_permute(hipStream_t st, uint32_t *d_states, size_t n);

// fri.hip
hipError_t launch_prefix_sum_columns(hipStream_t st, uint32_t *d_cols, uint32_t ncols, size_t n, uint32_t *d_scratch);
size_t prefix_sum_scratch_words(uint32_t ncols, size_t n);
// K4 tail: d_totals = inclusive prefix sums S of the row totals ([4][n], one F_p^4 per row); writes the running-sum
// column phi[r] = S[r-1] - r * S[n-1] / n  (phi[0] = 0) of the folded LogUp layout (stark.cuh) into d_phi ([4][n]) and,
// with cum_out != nullptr, the four words of S[n-1] to cum_out (device-accessible memory, e.g. pinned host memory)
hipError_t launch_phi_from_prefix_sums(hipStream_t st, const uint32_t *d_totals, uint32_t *d_phi, uint32_t log_n, uint32_t *cum_out);
hipError_t launch_open_weights(hipStream_t st, const NttTables &tabs, Fp4 z, uint32_t log_n, Fp4 *d_w);
constexpr uint32_t OPEN_MAX_ROW_BLOCKS = 256;
uint32_t open_row_blocks(uint32_t log_n);
hipError_t launch_open_columns(hipStream_t st, const uint32_t *const *d_cols, uint32_t ncols, uint32_t log_n, const Fp4 *d_w,
                               Fp4 *d_partial, Fp4 *d_out);
// d_alpha_pows_f64: [n_all][4] doubles, alpha^c as centred canonical residues (see centred_canonical in bb.cuh)
hipError_t launch_reduced_opening(hipStream_t st, const NttTables &tabs, const uint32_t *const *d_cols, uint32_t n_two,
                                  uint32_t n_all, uint32_t log_m, const double *d_alpha_pows_f64, Fp4 sz_all, Fp4 sz_two, Fp4 zeta,
                                  Fp4 zeta_next, Fp4 alpha_shift, Fp4 *d_out);
hipError_t launch_fri_fold(hipStream_t st, const NttTables &tabs, const Fp4 *d_v, Fp4 *d_out, const Fp4 *d_ro, Fp4 beta,
                           uint32_t log_m, const Fp4 *d_beta = nullptr);
// transcript step of one FRI round on the device: see fri.hip
hipError_t launch_fri_challenge(hipStream_t st, const uint32_t *d_root, uint32_t *d_state, Fp4 *d_beta_out, uint32_t *d_root_out);
hipError_t launch_fri_leaves(hipStream_t st, const Fp4 *d_v, uint32_t log_m, uint32_t *d_digests);
hipError_t launch_gather_rows(hipStream_t st, const uint32_t *const *d_cols, const uint32_t *d_log_h, uint32_t ncols,
                              const uint32_t *d_idx, uint32_t nq, uint32_t *d_out);
hipError_t launch_gather_paths(hipStream_t st, const uint32_t *d_digests, uint32_t log_h, const uint32_t *d_idx, uint32_t nq,
                               uint32_t *d_out);
// out[i][8] = digests[at[i]][8]: the listed nodes of a compact proof's tree, `at` being positions in the tree's digest array
hipError_t launch_gather_nodes(hipStream_t st, const uint32_t *d_digests, const uint32_t *d_at, uint32_t n, uint32_t *d_out);
hipError_t launch_gather_siblings(hipStream_t st, const Fp4 *d_v, uint32_t log_m, const uint32_t *d_idx, uint32_t nq, Fp4 *d_out);
hipError_t launch_pow_grind(hipStream_t st, const uint32_t state[16], uint32_t pos, uint32_t bits, uint32_t base, uint32_t count,
                            uint32_t *d_found);


// profile.hip
// The device tables of the execution report's tally (profile.h) and one pass over the cycle records of a shard into them.
// counts zeroed and keys all ones by the caller; classes: prof::instr_classes.  The records are only read.
namespace rv32 { struct CycleRec; }
enum ProfileCounter { PROFILE_TRANSFERS, PROFILE_DROPPED, PROFILE_SYS_OVERFLOW, PROFILE_BAD_RECORDS, PROFILE_COUNTERS };
struct ProfileTables {
    unsigned long long *pc_count, *taken;            // [n_instr]: retired; went to its static target (branches, JAL)
    unsigned long long *edge_keys, *edge_counts;     // [2^log_slots]: from << 32 | to of every other transfer
    unsigned long long *sys_keys, *sys_counts;       // [64]: syscall ids
    unsigned long long *counters;                    // [PROFILE_COUNTERS]
    const uint32_t *classes;                         // [n_instr]
    uint32_t n_instr, log_slots;
};
// last_succ: the instruction index of the shard's next_pc, or 0xffffffff when that is no instruction of the text
hipError_t launch_profile_records(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, const ProfileTables &t);

// calltree.hip
// The device pass of the call-tree report (calltree.h) over the cycle records of one shard: one workgroup per span of
// CALLTREE_SPAN consecutive records, spans numbered span0, span0 + 1, ... in the per-span arrays.  The records are only read.
constexpr uint32_t CALLTREE_SPAN = 4096;
enum CalltreeCounter { CALLTREE_DROPPED_FRAMES, CALLTREE_DROPPED_CYCLES, CALLTREE_UNMATCHED, CALLTREE_MAX_DEPTH, CALLTREE_BAD_RECORDS, CALLTREE_COUNTERS };
struct CalltreeSpanSummary { uint32_t u, c; };                        // the span reduced: u unmatched RETs, then c unmatched CALLs
struct CalltreeCall { uint32_t fn, pos; };                            // an unmatched CALL: the callee, its position in the span
struct CalltreeFrame { unsigned long long open; uint32_t fn, pad; };  // a frame of the stack on entry: global open position
struct CalltreeSpanIn { unsigned long long frames_at; uint32_t n_frames, depth; };   // emit mode: where the span's frames lie, top first; the depth on entry
struct CalltreeTables {
    const uint32_t *classes;                         // [n_instr]: calltree::instr_classes
    unsigned long long *counters;                    // [CALLTREE_COUNTERS], zeroed by the caller
    // summary mode: both written; calls_at == nullptr: the summaries alone, else span k's unmatched calls from calls[calls_at[k]]
    CalltreeSpanSummary *summaries;                  // [spans]
    const unsigned long long *calls_at;              // [spans]
    CalltreeCall *calls;
    // emit mode: read
    const CalltreeSpanIn *span_in;                   // [spans]
    const CalltreeFrame *frames;
    // emit mode: the arcs, caller << 32 | fn; keys all ones and sums zeroed by the caller
    unsigned long long *arc_keys, *arc_calls, *arc_cycles;   // [2^log_slots]
    uint32_t n_instr, log_slots;
};
// last_succ as launch_profile_records; base_position: the global position of the shard's first record
hipError_t launch_calltree_summary(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, size_t span0, const CalltreeTables &t);
hipError_t launch_calltree_emit(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t last_succ, size_t span0,
                                unsigned long long base_position, const CalltreeTables &t);

// memreport.hip
// The device tables of the memory report (memreport.h) and one pass over the cycle records of a shard into them.  Everything
// but sp[0] (all ones) is zeroed by the caller; classes / offs: memrep::instr_class and Instr::off per instruction; pre: the
// rows of memrep::pre_shapes(), six words each.  The records are only read.
enum MemoryCounter { MEMORY_CYCLES, MEMORY_PRE_CALLS, MEMORY_SP_WRITES, MEMORY_BAD_RECORDS, MEMORY_COUNTERS };
enum MemoryPageArray { MEMORY_LOADS, MEMORY_STORES, MEMORY_FIRST, MEMORY_PRE_READS, MEMORY_PRE_WRITES, MEMORY_PAGE_ARRAYS };
struct MemoryTables {
    unsigned long long *first_touch;                 // [n_instr]
    unsigned long long *page_ctr;                    // [MEMORY_PAGE_ARRAYS][memrep::N_PAGES], dense over the address space
    unsigned long long *counters;                    // [MEMORY_COUNTERS]
    uint32_t *sp;                                    // [2]: the minimum and the maximum of the values written to x2
    uint32_t *bitmap;                                // [memrep::BITMAP_WORDS]: one bit per word of guest memory
    const uint32_t *classes, *offs;                  // [n_instr]
    const uint32_t *pre;                             // [n_pre][6]
    uint32_t n_instr, n_pre;
};
hipError_t launch_memory_records(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const MemoryTables &t);
// after the shards: every page with a counted access as one dense entry (its counters and its 128-byte bitmap line), in no
// order, the first cap of them; *n_dense (zeroed by the caller) counts all
struct MemoryDensePage {
    uint32_t page, first;
    unsigned long long loads, stores, pre_reads, pre_writes;
    uint32_t bits[32];
};
hipError_t launch_memory_gather(hipStream_t st, const MemoryTables &t, MemoryDensePage *d_dense, uint32_t cap, uint32_t *d_n_dense);

// watch.hip
// The watchpoint search (watch.h) over the cycle records of one shard: count, scan, emit.  WatchArgs (watch.h) carries the
// queries, the precompile shapes, the static words per instruction and the shard's number; span_counts / span_offs are
// [spans of the shard][n_queries] u32, d_totals [n_queries] u32; d_bad_records is zeroed by the caller.  The emit pass writes
// the kept hits of the shard (WatchEmitArgs: per query the rank of the shard's first hit and the total over the job; cap_each)
// into d_out (dvt_watch_hit [n_queries][2][cap_each]).  The records are only read.
struct WatchArgs;
struct WatchEmitArgs;
hipError_t launch_watch_count(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const WatchArgs &a, uint32_t *d_span_counts,
                              unsigned long long *d_bad_records);
hipError_t launch_watch_scan(hipStream_t st, const uint32_t *d_span_counts, uint32_t *d_span_offs, uint32_t n_spans, uint32_t n_queries, uint32_t *d_totals);
hipError_t launch_watch_emit(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const WatchArgs &a, const WatchEmitArgs &e,
                             const uint32_t *d_span_counts, const uint32_t *d_span_offs, void *d_out);

// snapshot.hip
// The snapshot's passes (snapshot.h).  reduce: over the cycle records of one shard, into the member's winner tables
// (SnapTables: before and regs zeroed, after all ones, bad_records zeroed by the caller); SnapArgs carries the ranges, the
// precompile shapes, the static words per instruction, the shard's number and the position.  gather: one snap::Side per
// SnapFetch into d_out (snap::Side [n_items]).  The records are only read.
struct SnapArgs;
struct SnapTables;
struct SnapFetch;
hipError_t launch_snapshot_reduce(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, const SnapArgs &a, const SnapTables &t);
hipError_t launch_snapshot_gather(hipStream_t st, const SnapFetch *d_items, uint32_t n_items, const SnapArgs &a, void *d_out);

// origin.hip
// The passes of the origin search (origin.h).  reduce: over the first n_take records of one shard (the ones before the largest
// position any question of the pass asks at), the latest writer of every question's target before the question's position, as
// a position, into d_win [a.n] (zeroed by the caller: no position is 0); OriginArgs carries the sorted questions' device
// arrays, the offsets of the register questions, the precompile shapes, the static words per instruction and the shard's
// number; *d_bad_records (zeroed by the caller) counts the bad records among those taken.  gather: the record of every
// OriginFetch, 12 words each, into d_out (rv32::CycleRec [n_items]; all ones for an item outside its shard).  The records are
// only read.
struct OriginArgs;
struct OriginFetch;
hipError_t launch_origin_reduce(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_take, const OriginArgs &a, unsigned long long *d_win,
                                unsigned long long *d_bad_records);
hipError_t launch_origin_gather(hipStream_t st, const OriginFetch *d_items, uint32_t n_items, rv32::CycleRec *d_out);

// uses.hip
// The passes of the uses search (uses.h), each over the spans [first_span, first_span + n_spans) of one shard (UsesArgs carries the
// sorted definitions' device arrays, the offsets of the register definitions, the precompile shapes, the static words per
// instruction and the shard's number).  next: the first writer of every definition's target at or after its F, as a position, by
// atomicMin into d_win [a.n] (set to all ones by the caller); *d_bad_records (zeroed by the caller) counts the bad records at or
// after a.min_from.  count: with a.d_next known, the uses of every definition per span, one row of 256 u32 per span into d_table
// from row table_row on (every launched row is written in full).  scan: one workgroup over those rows in order, the running count
// per definition carried in d_carry [256] (zeroed by the caller before the first shard), one UsesItem per (span, definition) that
// holds a rank below fan appended to d_items, *d_n_items counts them (zeroed by the caller).  emit: one workgroup per item of a
// fixed grid of cap_items; position and role of the ranks below fan into d_out_pos / d_out_role [a.n * a.fan].  The records are
// only read.
struct UsesArgs;
struct UsesItem;
hipError_t launch_uses_next(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t first_span, uint32_t n_spans, const UsesArgs &a,
                            unsigned long long *d_win, unsigned long long *d_bad_records);
hipError_t launch_uses_count(hipStream_t st, const rv32::CycleRec *d_recs, size_t n_recs, uint32_t first_span, uint32_t n_spans, const UsesArgs &a,
                             uint32_t *d_table, size_t table_row, size_t table_rows);
hipError_t launch_uses_scan(hipStream_t st, const uint32_t *d_table, size_t table_row, uint32_t n_spans, size_t table_rows, const rv32::CycleRec *d_recs,
                            size_t n_recs, uint32_t shard, uint32_t first_span, uint32_t n_d, uint32_t fan, unsigned long long *d_carry, UsesItem *d_items,
                            uint32_t *d_n_items, uint32_t cap_items);
hipError_t launch_uses_emit(hipStream_t st, const UsesItem *d_items, const uint32_t *d_n_items, uint32_t cap_items, const UsesArgs &a,
                            unsigned long long *d_out_pos, uint32_t *d_out_role);

// diverge.hip
// The passes of the divergence report (diverge.h) over one segment of pairs (DivergeArgs: both record pointers at the segment's
// first pair, a.n_pairs pairs, the pair number a.k0 and the span number a.span0 of its first span).  classify: one DivergeSpan and
// one DivergeSpanRegs per span into d_spans / d_span_regs [cap_spans], and the pair number of a CONTROL or BAD pair by atomicMin
// into *d_stop_flag (set to all ones by the caller).  merge: over the spans [0, n_spans) of a call, up to the first with a stop,
// into *d_out and d_rank_base [n_spans].  emit: the first and the last K data pairs into d_first / d_last [K each].  The records
// are only read.
struct DivergeArgs;
struct DivergeSpan;
struct DivergeSpanRegs;
struct DivergeMerged;
hipError_t launch_diverge_classify(hipStream_t st, const DivergeArgs &a, DivergeSpan *d_spans, DivergeSpanRegs *d_span_regs, uint32_t cap_spans,
                                   unsigned long long *d_stop_flag);
hipError_t launch_diverge_merge(hipStream_t st, const DivergeSpan *d_spans, const DivergeSpanRegs *d_span_regs, uint32_t n_spans, unsigned long long *d_rank_base,
                                DivergeMerged *d_out);
hipError_t launch_diverge_emit(hipStream_t st, const DivergeArgs &a, const DivergeSpan *d_spans, const unsigned long long *d_rank_base, const DivergeMerged *d_merged,
                               uint32_t cap_spans, uint32_t K, void *d_first, void *d_last);

}  // namespace dvt
