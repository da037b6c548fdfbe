/*
 * dvt_prover.h — C ABI of the MI355X-native STARK prover that replaces the SP1
 * prover behind metacraft-labs/dvt-circuits' prove()/execute() boundary.
 *
 * The reference reaches its prover through six call sites in src/main.rs
 * (ProverClient::from_env :438,:461,:481; setup :462,:482; prove(..).run()
 * :463-466; execute(..).run() :439-442,:498-501; SP1Stdin::write :434-437,
 * :458-460; proof.save :472-474).  Each entry point below names the call site
 * it stands in for.  INTEGRATION.md shows the Rust `extern "C"` stub a
 * maintainer would add.
 *
 * Conventions
 *   - return 0 = ok; DVT_ERR_GUEST = guest halted non-zero / panicked (what the
 *     reference's 92 test vectors observe as process exit code 1, script/run.sh:82-89);
 *     DVT_ERR_INPUT = malformed argument / ELF / proof; DVT_ERR_DEVICE = HIP failure
 *     or no gfx950 device (there is NO CPU fallback); DVT_ERR_UNSUPPORTED = the
 *     program uses an instruction the prover has no chip for yet;
 *     DVT_ERR_REJECTED = a proof failed verification.
 *   - buffers returned through `uint8_t **` are library-allocated, release with dvt_free().
 *   - a dvt_prover is re-entrant per handle: one handle per caller thread (the
 *     reference's HTTP node calls prove() from concurrent tokio workers,
 *     src/service/node.rs:72-81); calls on one handle are serialised internally.
 *     (dvt_stream, dvt_last_error and the dvt_last_* metrics only read the handle:
 *     they are not serialised, and read what the last finished call left.)
 *   - "device field array": uint32_t words in HBM holding BabyBear elements in
 *     the library's internal (Montgomery) representation, COLUMN-MAJOR
 *     ([width][height], element (r,c) at c*height + r), natural row order.
 *   - all device work of a handle runs on the handle's own HIP streams (dvt_stream is the first of them).
 *   - a handle may own several devices ("devices"): the shards of one execution are then proven on all of them inside the
 *     same calls; see dvt_prover_create and the shard-level calls below.
 */
#ifndef DVT_PROVER_H
#define DVT_PROVER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DVT_OK 0
#define DVT_ERR_GUEST 1
#define DVT_ERR_INPUT 2
#define DVT_ERR_DEVICE 3
#define DVT_ERR_UNSUPPORTED 4
#define DVT_ERR_REJECTED 5

typedef struct dvt_prover dvt_prover;
typedef struct dvt_pk dvt_pk;

/* ---------------------------------------------------------------- lifecycle */
/* ProverClient::from_env() (src/main.rs:438,461,481).  cfg_json may be NULL or
 * a JSON object: {"device":0,"fri_queries":100,"pow_bits":16,"profile":0,"log_shard_size":21,
 * "keep_phase1":1,"exec_threads":0,"parts_parallel_log":15}.  exec_threads = trace-mode executor threads of the prove pipeline
 * (0 = from the host's core count).  "keep_phase1" is a mode: what a shard keeps in HBM between phase 1 and phase 2 (the
 * tiers DVT_KEEP_* below).  0: nothing; phase 2 of a shard recomputes K0 and the main-trace commitment.  1 (the default, and
 * what every value other than 0 and 2 reads as): K0 output, main LDEs and main Merkle tree (about 3 GB per 2^21-cycle
 * shard) while more than 24 GB plus the room of the lanes not yet created is free, else nothing.  2: the same in full
 * while that leaves every shard known to come room for its uploads and its tree; then the tree alone (268 MB per
 * 2^21-cycle shard: phase 2 runs K0 and the main LDEs again and hashes nothing); then nothing.  The rule is
 * dvt_debug_keep_plan.  Headers, shard proofs and containers are byte for byte the same in every mode and tier: the tier
 * only decides which launches of the same kernels on the same inputs run once and which twice.
 * "keep_full_max" (default -1 = no cap; a diagnostic key): at most that many shards per physical device and job are kept in
 * full, so that jobs far smaller than HBM reach the other tiers of mode 2.  Modes 0 and 1 do not read it.
 * parts_parallel_log: tables of
 * at most 2^parts_parallel_log rows compute their LogUp rows (K4) and quotient (K5) one constraint group per thread, taller
 * ones one row per thread; -1 = never, at most 15 (DVT_ERR_INPUT above).  The proof bytes do not depend on it.
 * "verify_chunk_words" (default 4194304; 0 or less is DVT_ERR_INPUT): proof words per chunk of dvt_prover_verify's device
 * part.  Shards are gathered into a chunk until the next one would not fit; a single shard larger than the chunk goes
 * alone.  Answers do not depend on it (a test knob, like parts_parallel_log: small proofs reach the multi-chunk path).
 * "compact_openings" (default 0): 1 makes every prove entry point write its shard proofs in the compact form (see
 * dvt_proof_compact): the bytes dvt_proof_compact makes of the default proof, without gathering the shared paths.
 * "lanes" (1..3, default 2; without the key the environment variable DVT_LANES sets the default; anything else is
 * DVT_ERR_INPUT): prover lanes that run phase 2 of different shards of one job at the same time, each with its own HIP
 * stream, device arena and buffer cache.  The further lanes are created on the first job that holds at least two shards;
 * "profile":1 forces one lane.  The proof bytes do not depend on it.
 * "phase1_lanes" (1..lanes, default lanes; without the key the environment variable DVT_PHASE1_LANES sets the
 * default, capped at "lanes"; a key outside 1..lanes is DVT_ERR_INPUT): how many of the lanes also run phase 1 (K0 and the
 * main commitment) of different shards at the same time inside prepare / prove_core.  1 is one compute stream that
 * uploads and commits shard after shard.  With more, a feeder uploads the shards in execution order on the copy stream and
 * each committing lane takes the next uploaded shard; lane k is created when a k-th shard waits and no lane is free, so
 * a job of one shard creates none.  Headers, shard order and proof bytes do not depend on it.  "profile":1 forces 1.
 * "devices": [d0, d1, ...] (1..8 HIP device indices, each a gfx950 device) instead of "device": the handle owns one device
 * MEMBER per entry, and shard i of an execution is proven on member i mod G (exactly: the k-th shard a job holds on member
 * k mod G).  An index may repeat: [0, 0] is two members on one GPU, each with its own streams, arenas and copy of the
 * proving key.  "devices": [d] is "device": d.  Both keys together, an empty list, more than 8 entries, an index that is
 * negative or not below the device count, or an entry that is not an integer: DVT_ERR_INPUT.  Without the key "devices"
 * the environment variable DVT_DEVICES (comma-separated indices, the same checks) is the list when it is set, and "device"
 * is then ignored.  "lanes" counts per member; its default is 2 for every G (measured on [0, 0], profiles/README.md
 * "Round 5": two members of two lanes each take 889 ms per 32-shard call, of one lane each 980 ms; one device with two
 * lanes 915 ms).
 * Proof bytes, verifying key and container do not depend on the device list.  With G > 1:
 *   dvt_setup            builds the proving key on every member (the setup runs once per member from the one decoded
 *                        program: no peer access between devices is needed) and fails with DVT_ERR_DEVICE if a member's
 *                        verifying key differs from member 0's; dvt_pk_free frees every copy
 *   prepare / prove_core / prove_job
 *                        ONE executor (one fast pass, one pool of trace threads) per call feeds all members; every member
 *                        uploads and runs phase 1 of its shards on a host thread of its own; the headers meet in host memory,
 *                        the challenges are computed once, phase 2 runs on every member's lanes at the same time
 *   commit_shard / prove_shard
 *                        go to the member that holds the shard; the first prove_shard of a job starts the run-ahead
 *                        pipeline on EVERY member (its own part from the shard asked for, the others from their first shard
 *                        after it), under the contract described at prove_shard below.  An abandoned job wastes at most
 *                        (sum of the members' lanes - 1) shard proofs.
 *   stage- and machine-level calls, dvt_dev_*, dvt_stream, dvt_last_*
 *                        run on member 0; dvt_sync also waits for the other members' streams
 * Two members on one physical device (and the phase-1 lanes of one member) take turns in the admission of a shard's first
 * phase 1: asking how much HBM is free and allocating what the commit keeps, so that no two count the same free bytes.
 * The turn ends before the commit's kernels are launched, which therefore overlap.  A second dvt_rv32_prove_job of the same job runs
 * phase 1 of all its shards again one after the other on the calling thread, member by member: only prepare runs the
 * members' phase 1 at the same time.  A proving key and a job are freed on the handle that made them: dvt_pk_free /
 * dvt_job_free on a handle with fewer members cannot reach the other members' device buffers and leave them allocated.
 * On return from a call the calling thread's current device is member 0's. */
int dvt_prover_create(const char *cfg_json, dvt_prover **out);
/* device members of the handle (1 unless "devices" / DVT_DEVICES named more), and the HIP device index of a member
 * (-1 when member >= the count) */
uint32_t dvt_prover_device_count(const dvt_prover *p);
int dvt_prover_device(const dvt_prover *p, uint32_t member);
void dvt_prover_destroy(dvt_prover *p);
/* last error text of this handle (or of the failed create when p == NULL) */
const char *dvt_last_error(const dvt_prover *p);
void dvt_free(void *ptr);
/* ABI version of this header (4: "devices", dvt_prover_device_count, dvt_prover_device, dvt_rv32_job_shard_member;
 * 5: dvt_rv32_job_shard_device_rows; 6: dvt_stage_check_constraints, dvt_stage_bus_sums, dvt_rv32_check_job,
 * dvt_rv32_job_shard_chips; 7: dvt_prover_verify, dvt_prover_machine_verify, dvt_stage_sponge_rows,
 * dvt_stage_verify_paths, dvt_prover_verify_times; 8: dvt_stage_bus_ledger_*, dvt_rv32_job_bus_tuples;
 * 9: dvt_stage_hunt_cells, dvt_stage_hunt_pairs, dvt_rv32_hunt_shard, dvt_rv32_job_shard_chip_shape;
 * 10: dvt_stage_hunt_join_*, dvt_rv32_hunt_join_job; 11: "compact_openings", dvt_proof_compact, dvt_proof_expand,
 * dvt_stage_multipath_nodes, dvt_stage_verify_multipath, dvt_debug_compact_list_sweep; 12: dvt_rv32_job_profile,
 * dvt_execute_profile; 13: "keep_phase1": 2, "keep_full_max", DVT_KEEP_*, dvt_rv32_job_shard_kept,
 * dvt_rv32_job_shard_kept_bytes, dvt_debug_keep_plan; 14: dvt_rv32_job_calltree,
 * dvt_rv32_job_calltree_times, dvt_execute_calltree; 15: dvt_rv32_job_memory, dvt_execute_memory;
 * 16: dvt_rv32_job_watch, dvt_execute_watch, dvt_rv32_job_watch_times; 17: dvt_rv32_job_snapshot,
 * dvt_rv32_job_snapshot_times, dvt_execute_snapshot; 18: dvt_rv32_debug_poke_cell; 19: dvt_rv32_job_origin, dvt_rv32_job_origin_times,
 * dvt_execute_origin; 20: dvt_rv32_job_diverge, dvt_rv32_job_diverge_times, dvt_execute_diverge; 21: dvt_rv32_job_uses,
 * dvt_rv32_job_uses_times, dvt_execute_uses) */
uint32_t dvt_abi_version(void);
/* the handle's hipStream_t (for event timing by the caller) */
void *dvt_stream(dvt_prover *p);
int dvt_sync(dvt_prover *p);

/* ------------------------------------------------- stage-level entry points
 * One call = one kernel family of SURVEY.md section 8(a) on caller-owned device
 * memory; used by the parity tests and by bench.py's roofline measurement.
 * Asynchronous on dvt_stream(p): call dvt_sync() before reading results. */
/* canonical <-> internal representation, in place, n words */
int dvt_dev_to_internal(dvt_prover *p, uint32_t *d_words, size_t n);
int dvt_dev_from_internal(dvt_prover *p, uint32_t *d_words, size_t n);

/* K1: coset low-degree extension, blow-up 2.  d_in [width][2^log_n] holds
 * evaluations over the subgroup H; d_out [width][2^(log_n+1)] receives the
 * evaluations on shift*H', |H'| = 2|H|.  shift_mode: 0 = the generator 31 (trace
 * commitments), 1 = 1, 2 = w_{2N}^-1 (the two quotient chunks).  d_scratch
 * ([width][2^log_n]) holds the intermediate of the first pass when log_n > 12;
 * pass NULL to run that pass in place, which clobbers d_in.  With d_scratch given,
 * d_in is left as it was; what d_scratch holds afterwards is unspecified at every
 * log_n (at log_n <= 12 it is not needed and may be NULL).  log_n <= 22. */
int dvt_stage_coset_lde(dvt_prover *p, uint32_t *d_in, uint32_t *d_scratch, uint32_t *d_out,
                        uint32_t width, uint32_t log_n, uint32_t shift_mode);

/* K2+K3: mixed-height Poseidon2 Merkle commitment (natural-order pairing). */
typedef struct {
    const uint32_t *d_data; /* device field array [width][2^log_height] */
    uint32_t width;
    uint32_t log_height;
} dvt_dev_matrix;
/* words the digest buffer must hold: (2*H - 1) * 8, H = tallest height */
size_t dvt_merkle_digest_words(const dvt_dev_matrix *mats, size_t n);
/* d_digests: layer 0 (H digests of 8 words) first, then H/2, ..., the root last.
 * DVT_ERR_INPUT (text in dvt_last_error, nothing launched, the handle stays usable)
 * for a matrix of width 0 - the prover builds none, and the tree's definition would
 * hash an empty row there - and for a log_height above 23 ("tree too tall"). */
int dvt_stage_merkle_commit(dvt_prover *p, const dvt_dev_matrix *mats, size_t n, uint32_t *d_digests);
/* raw permutation on n states of 16 words each (device array [n][16]); test hook */
int dvt_stage_poseidon2_permute(dvt_prover *p, uint32_t *d_states, size_t n);

/* K8: one FRI fold of d_v (2^log_m extension elements, 4 words each, natural
 * order) into d_out (2^(log_m-1)); d_ro (may be NULL) is added element-wise;
 * beta = 4 canonical words. */
int dvt_stage_fri_fold(dvt_prover *p, const uint32_t *d_v, uint32_t *d_out, const uint32_t *d_ro,
                       const uint32_t beta[4], uint32_t log_m);

/* The stages below run the prover's own host code (the same calls as a shard proof).  Field values
 * passed through host arrays are canonical words; extension elements are 4 words.  log_n <= 22. */
/* K4 tail: the LogUp running-sum column.  d_totals [4][2^log_n] holds one F_p^4 row total per row
 * and is overwritten by its inclusive prefix sums S; d_phi [4][2^log_n] (not overlapping d_totals)
 * receives phi[r] = S[r-1] - r S[n-1] / n (phi[0] = 0) and cum the cumulative sum S[n-1].
 * Synchronises the stream. */
int dvt_stage_logup_running_sum(dvt_prover *p, uint32_t *d_totals, uint32_t *d_phi, uint32_t log_n, uint32_t cum[4]);
/* K6: the values at z and at z*w_n of the polynomials that interpolate the columns of n matrices
 * of one height 2^log_height over the subgroup H (at most 65536 columns in all), opened by one launch
 * as a shard proof opens a chip's matrices.  out [columns][2][4], column order of mats.  Synchronises
 * the stream. */
int dvt_stage_open(dvt_prover *p, const dvt_dev_matrix *mats, size_t n, const uint32_t z[4], uint32_t *out);
/* K7: the FRI input of one height.  cols: host array of n_all (1..65536) device columns of
 * 2^log_m words (1 <= log_m <= 23), the LDE on 31*<w_m>; the first n_two were opened at zeta and
 * zeta * w_{m/2}.  open_local [n_all][4], open_next [n_two][4]; d_out [2^log_m][4] receives
 *   sum_c alpha^c (p_c(x) - p_c(zeta)) / (x - zeta)
 *   + alpha^n_all sum_{c < n_two} alpha^c (p_c(x) - p_c(zeta w_{m/2})) / (x - zeta w_{m/2}). */
int dvt_stage_reduced_opening(dvt_prover *p, const uint32_t *const *cols, uint32_t n_two, uint32_t n_all, uint32_t log_m,
                              const uint32_t alpha[4], const uint32_t *open_local, const uint32_t *open_next,
                              const uint32_t zeta[4], uint32_t *d_out);
/* K9: the smallest proof-of-work witness w: the Poseidon2 permutation of state with state[pos] = w
 * (pos < 8) has word 7 divisible by 2^bits (bits <= 30).  Synchronises the stream. */
int dvt_stage_pow_grind(dvt_prover *p, const uint32_t state[16], uint32_t pos, uint32_t bits, uint32_t *witness);
/* K4 and K5 of one chip of a machine ("rv32" or "toy", chip = its index), as a shard proof runs them.  Device matrices
 * hold Montgomery words (dvt_dev_to_internal), column-major; pub holds the chip's public values.  path selects the
 * launches: DVT_PATH_DEFAULT what a proof on this handle launches at this height, DVT_PATH_ROWS the per-row K4 kernel /
 * one K5 launch per part, DVT_PATH_PARTS the part-parallel launches (refused for a chip without them, and above 2^15
 * rows: their scratch is sized for that height at most). */
#define DVT_PATH_DEFAULT 0u
#define DVT_PATH_ROWS 1u
#define DVT_PATH_PARTS 2u
/* K4: d_main [main_w][2^log_n], d_prep [prep_w][2^log_n] (may be NULL when prep_w = 0) -> d_perm
 * [4 perm_ext_w][2^log_n] (the batch columns, then phi; may be NULL when the chip has no interactions) and cum, the
 * chip's cumulative sum.  Synchronises the stream. */
int dvt_stage_perm(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                   const uint32_t *pub, const uint32_t perm_alpha[4], const uint32_t beta[4], uint32_t path, uint32_t *d_perm,
                   uint32_t cum[4]);
/* K5 selectors: the handle's cached table of this height, or computed in the kernel */
#define DVT_SELECTORS_TABLE 0u
#define DVT_SELECTORS_IN_KERNEL 1u
/* K5: the LDEs d_main_lde [main_w][2^(log_n+1)], d_prep_lde [prep_w][..], d_perm_lde [4 perm_ext_w][..] (on 31*<w_2N>;
 * the last two may be NULL when their width is 0) -> d_out [2][4][2^log_n], the quotient's two chunks (even and odd LDE
 * rows) as a shard proof lays them out.  cum: the chip's cumulative sum. */
int dvt_stage_quotient(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main_lde, const uint32_t *d_prep_lde,
                       const uint32_t *d_perm_lde, uint32_t log_n, const uint32_t *pub, const uint32_t perm_alpha[4],
                       const uint32_t beta[4], const uint32_t alpha[4], const uint32_t cum[4], uint32_t path, uint32_t selectors,
                       uint32_t *d_out);

/* Trace-row checks of one chip (SP1 users know the first as debug_constraints): do the rows of a trace satisfy the chip's
 * AIR, and what do its LogUp terms add up to on each bus?  Both read the matrices dvt_stage_perm reads (d_main
 * [main_w][2^log_n], d_prep [prep_w][2^log_n] or NULL when prep_w = 0; Montgomery words, column-major; the row after the
 * last is row 0), evaluate the same generated AIR source as K4 / K5, and synchronise the stream.  log_n <= 22; a chip index
 * out of range or a NULL d_main is DVT_ERR_INPUT.
 * A constraint is checked on the rows where it is active (all rows, row 0, row n-1, every row but the last).  What is
 * counted is a UNIT: a plain constraint under its index, or a whole big-integer identity (its K coefficient constraints)
 * under the index of the FIRST of them: the library holds such an identity only in closed form, C(x) + (x - 256) W(x),
 * and evaluates it at the point xi of F_p^4 the caller supplies (4 canonical words).  A row with a wrong coefficient is
 * missed with probability at most K / p^4 over xi; the indices first + 1 .. first + K - 1 never fire.
 * counts (host array of the chip's n_constraints words, or NULL): rows that violate each unit.  out->violations: their
 * sum; out->first_row / first_constraint: the lowest violating row and the lowest violated unit of that row
 * (first_constraint = -1, first_row = 0 without a violation).  A chip without constraints returns zeros. */
#define DVT_CHECK_BUSES 8u
typedef struct {
    uint64_t violations;
    uint32_t first_row;
    int32_t first_constraint; /* -1: none */
} dvt_check_result;
int dvt_stage_check_constraints(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                                uint32_t log_n, const uint32_t *pub, const uint32_t xi[4], uint32_t *counts, dvt_check_result *out);
/* out[bus][4], canonical: the sum over the rows of the chip's signed LogUp terms +-mult / (perm_alpha + bus + sum_k
 * beta^(k+1) v_k) on each bus (bus ids of the machine; rv32 has 6).  The sum over the buses is the cumulative sum
 * dvt_stage_perm returns.  Field addition is exact: the result does not depend on the launch shape.  A chip without
 * interactions returns zeros. */
int dvt_stage_bus_sums(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                       uint32_t log_n, const uint32_t *pub, const uint32_t perm_alpha[4], const uint32_t beta[4],
                       uint32_t out[DVT_CHECK_BUSES][4]);

/* The bus ledger: WHICH tuples of the LogUp buses do not cancel (dvt_stage_bus_sums only says which bus).  A tuple is
 * (bus, arity, canonical values); an occurrence is one interaction of one row with a non-zero multiplicity, or a tuple the
 * caller adds.  Two passes over the same chip tables:
 *   new -> add / add_tuple (TALLY: every occurrence adds its signed multiplicity, weighted three ways, to the bucket its
 *   64-bit key selects; a balanced tuple adds up to 0 mod p) -> close (n_dirty: buckets with a non-zero sum; 0 means every
 *   bus balances, and nothing more is needed) -> collect / add_tuple over the SAME tables and tuples (COLLECT: the
 *   occurrences of the dirty buckets go into a table of cap_slots records, one per tuple) -> result -> free.
 * The matrices are those of dvt_stage_bus_sums (device, internal representation, column-major); pub: the chip's public
 * values, canonical.  tag (< 2^16) is the caller's label of a table, e.g. a shard position; it comes back in first_tag.
 * Every call runs on device 0 of the handle and synchronises.  Wrong order (collect before close, add after it), a NULL, a
 * chip out of range, log_n > 22, an arity above DVT_LEDGER_MAX_ARITY or a tag >= 2^16 is DVT_ERR_INPUT; a HIP failure is
 * DVT_ERR_DEVICE.  log_buckets: 10..24; seed: any (it keys the tuples: a retry after truncation takes another).
 * result: the tuples whose net multiplicity is not 0, sorted by (bus, values); at most cap are written.  *truncated is set
 * when the record table overflowed (64 probes found no free record: that occurrence was dropped) or cap is too small; the
 * tuples that are returned are exact all the same: a tuple that owns a record saw all of its occurrences.
 * A diagnostic, not a soundness boundary: an unmatched tuple goes unseen only when the three sums of its bucket cancel
 * against other unmatched tuples (about 2^-60); the seed does not depend on the rows. */
#define DVT_LEDGER_MAX_ARITY 40u /* rv32's widest tuple has 38 values */
typedef struct {
    uint32_t bus, arity, net; /* net: sum of the signed multiplicities mod p, canonical, never 0 */
    uint32_t n_send, n_recv;  /* occurrences with a non-zero multiplicity, saturating */
    uint32_t first_tag, first_chip, first_row, first_interaction; /* lowest occurrence; chip 0xffffffff: added by the caller */
    uint32_t values[DVT_LEDGER_MAX_ARITY]; /* canonical */
} dvt_bus_tuple;
typedef struct dvt_bus_ledger dvt_bus_ledger;
int dvt_stage_bus_ledger_new(dvt_prover *p, const char *machine, uint32_t log_buckets, uint32_t cap_slots, uint64_t seed,
                             dvt_bus_ledger **ledger);
int dvt_stage_bus_ledger_add(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                             uint32_t log_n, const uint32_t *pub, uint32_t tag);
/* a term of the caller's (sign > 0: a send of multiplicity mult, else a receive); before close it tallies, after it collects */
int dvt_stage_bus_ledger_add_tuple(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t bus, const uint32_t *values, uint32_t arity,
                                   int32_t sign, uint32_t mult, uint32_t tag);
int dvt_stage_bus_ledger_close(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t *n_dirty);
/* a no-op when close found no dirty bucket */
int dvt_stage_bus_ledger_collect(dvt_prover *p, dvt_bus_ledger *ledger, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                                 uint32_t log_n, const uint32_t *pub, uint32_t tag);
int dvt_stage_bus_ledger_result(dvt_prover *p, dvt_bus_ledger *ledger, dvt_bus_tuple *out, size_t cap, size_t *n_tuples,
                                uint32_t *truncated);
int dvt_stage_bus_ledger_free(dvt_prover *p, dvt_bus_ledger *ledger);

/* The forgery hunt: which one- and two-cell changes of a chip's main trace does NOTHING reject?  The matrices are those of
 * dvt_stage_check_constraints (device, Montgomery words, column-major); only main cells are changed, and the trace itself
 * is only read (the kernels evaluate the generated AIR through a view that overrides the changed cells).
 *   change     (col, row, delta), 1 <= delta < p canonical: the cell becomes value + delta mod p.
 *   forgery    one change, or two changes at different cells: a same-row pair has both cells in base row r, col[0] < col[1];
 *              an adjacent pair has the first cell in row r and the second in row (r + 1) mod n, any two columns.  A candidate
 *              whose two changes fall on one cell (n = 1 only) is skipped.
 *   touched    the set of rows {row - 1, row} mod n over the changed cells (the AIR reads rotations 0 and 1 only).
 *   caught     (a) a unit of the chip (dvt_stage_check_constraints: units, `when`, identities at xi) is violated on a touched
 *              row where it is active, or (b) the touched rows' signed multiset of (bus, values) over their interactions with
 *              non-zero multiplicity differs from the honest table's.  (b) is decided through a keyed fingerprint per row:
 *              a changed multiset is taken for unchanged with probability about 2^-60 over the key (one changed tuple: never),
 *              multiplicities compared mod p.  An escape of the exact multiset is never called caught.
 *   escape     not caught.  A single change that escapes makes its cell FREE for that delta on that row (cells the row's
 *              instruction family does not read are free, and that is expected).
 *   reported   a pair that escapes although at least one of its changes is caught on its own.  Pairs of two free cells are
 *              dropped without being evaluated.
 * seed: xi and the fingerprint key come from a transcript over a domain tag and seed; the answers for honest tables do not
 * depend on it apart from the stated miss probability.  Precondition: the honest table violates nothing; the call runs the
 * constraint check first and returns DVT_ERR_REJECTED, reporting nothing, when it does.
 * max_evals (0: the default, 2^33): an evaluation is one row evaluated for one candidate; a call whose candidates x touched
 * rows (for pairs: before the free x free rule, plus the single-cell pass of the listed columns) exceed it is DVT_ERR_INPUT
 * before anything is launched.  The work is split into launches of at most 2^24 lane slots (256 per candidate and touched row).
 * Every call runs on lane 0 of device 0 of the handle (dvt_rv32_hunt_shard: of the device that holds the shard) and
 * synchronises.  DVT_ERR_INPUT: a NULL handle, d_main or output, a chip out of range, log_n > 22, n_deltas 0 or above
 * DVT_HUNT_MAX_DELTAS, a delta of 0 or >= p, a column >= main_w, a window that is empty or not inside the table, adjacent
 * > 1, a shard the job does not hold.  DVT_ERR_UNSUPPORTED: a chip without the hunt.  DVT_ERR_DEVICE: a HIP failure (text in
 * dvt_last_error).  Outputs are written only by a call that returns DVT_OK. */
#define DVT_HUNT_MAX_DELTAS 8u
typedef struct {
    uint32_t row, n_cells;                 /* base row; 2 for a pair */
    uint32_t col[2], row_off[2], delta[2]; /* row_off 0 | 1; delta canonical */
    uint32_t alone;                        /* bit i: change i is caught on its own */
} dvt_escape;                              /* 36 bytes */
/* single cells of rows [row_first, row_first + row_count) (inside the table, no wrap of the window):
 * free_counts [main_w][n_deltas] = rows of the window where the change escapes;
 * free_map (host, may be NULL) [n_deltas][main_w][row_count] bytes 0 / 1 */
int dvt_stage_hunt_cells(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                         uint32_t log_n, const uint32_t *pub, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                         uint32_t row_first, uint32_t row_count, uint64_t max_evals, uint32_t *free_counts, uint8_t *free_map);
/* pairs with base row in the window; adjacent = 0: both cells in the base row, 1: the second in the next row;
 * cols (host, n_cols entries in any order, repeats count once; or NULL = every main column): the columns both cells are
 * taken from.  out: at most min(cap, 2^22) records, sorted by (row, col[0], col[1], delta[0], delta[1]); when fewer come
 * back than were reported, which ones is unspecified, and each is a true report.  *n_reported counts all; *n_tried =
 * pairs evaluated */
int dvt_stage_hunt_pairs(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                         uint32_t log_n, const uint32_t *pub, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                         const uint32_t *cols, uint32_t n_cols, uint32_t adjacent, uint32_t row_first, uint32_t row_count,
                         uint64_t max_evals, dvt_escape *out, size_t cap, uint64_t *n_reported, uint64_t *n_tried);

/* The join hunt: two-cell forgeries ACROSS tables and distant rows, and single cells that a lookup table absorbs.  The hunts
 * above stop at the edge of one table and at a distance of one row, and call a change caught as soon as the multiset of its
 * touched rows differs from the honest one.  The join keeps that difference and looks for the other half.
 *   window     (tag, chip, matrices, log_n, pub, row_first, row_count, optional columns): rows of one table instance.  tag
 *              (< 2^16) names the instance, e.g. a shard position.  The same (tag, chip) may be added more than once only with
 *              disjoint windows and the same log_n.
 *   candidate  (window, col, row, delta), delta from the call's list; touched rows {row - 1, row} mod n as above.
 *   supply     a table whose receive interactions carry preprocessed values under a bare multiplicity column (rv32 program,
 *              byte, mem_image; toy range8).  Its tuples are the values of its interactions on EVERY row, whatever the
 *              multiplicity holds: a forger re-counts that column.  Supply tables are not hunted (every change of their
 *              multiplicity cells is absorbed by definition).  WHETHER A CHIP MAY SERVE AS ONE IS THE CALLER'S STATEMENT: the
 *              call only refuses the chips that have no supply launch (DVT_ERR_UNSUPPORTED).
 *   difference D = (multiset of the touched rows under the change) - (honest multiset of those rows), after removing from
 *              both every tuple a supply table holds; D_all is the same over all tuples.  The device works with the
 *              fingerprint of the hunts above (three sums mod p), one key for the whole call, computed over all tuples and
 *              over the unsupplied ones; a tuple counts as supplied when its 64-bit key is in the supply set.
 *   outcome    caught by a constraint: nothing is kept.  free (D_all = 0): the business of dvt_stage_hunt_cells, nothing is
 *              kept.  ABSORBED (D_all != 0, D = 0): a one-cell finding.  OPEN (D != 0): a record is kept.
 *   group      a value D with the open records whose difference is D on one side and those whose difference is -D on the
 *              other; both sides non-empty.  Its pairs are the combinations of one cell of each side, EXCEPT those whose two
 *              cells lie in the same (tag, chip) at circular row distance <= 1: there the touched rows overlap, the
 *              differences do not add, and the pair belongs to dvt_stage_hunt_pairs.  A group that keeps no pair is dropped.
 *              For every pair that remains the touched rows are disjoint or lie in different tables, so constraints and
 *              multisets add: the pair escapes the whole machine, up to the fingerprint's miss probability stated above.
 * NOT LOOKED AT, and no soundness claim follows from an empty answer: three or more cells; a pair in which one half is caught
 * by a constraint and repaired by the other; permutation and quotient columns.
 * Order: new -> supply* -> add+ -> match -> result -> free.  A supply after the first add, overlapping windows of one (tag,
 * chip) and a tag >= 2^16 are DVT_ERR_INPUT, with everything the hunts above refuse.  The supply tables' matrices must stay
 * valid until the first add returns (the set is built then: its capacity is a power of two of at least four times the number
 * of keys; a key that finds no slot in 64 probes fails the call with DVT_ERR_INPUT "supply set too small").  add runs the
 * precondition on the window's table (DVT_ERR_REJECTED) and refuses more than max_evals evaluations (0: 2^33) before
 * anything is launched.  cap_records / cap_absorbed: records kept on the device (0: 2^22); the totals keep counting past
 * them.  log_slots (0: twice the stored records, rounded up to a power of two; else 6..26): the slots of the join's table;
 * a record that finds none in 64 probes is left out and sets DVT_JOIN_TRUNC_PROBES.  Whatever is truncated, every group
 * that comes back is a subset of a true group.  After an add that fails with DVT_ERR_DEVICE the join takes no further add or
 * match: free it.  Every call runs on lane 0 of device 0 of the handle and synchronises. */
#define DVT_JOIN_TRUNC_RECORDS 1u  /* more open records than cap_records */
#define DVT_JOIN_TRUNC_ABSORBED 2u /* more absorbed cells than cap_absorbed */
#define DVT_JOIN_TRUNC_PROBES 4u   /* a record found no slot of the join's table */
#define DVT_JOIN_TRUNC_OUTPUT 8u   /* more matched records than the device's output array holds */
#define DVT_JOIN_NO_GROUP 0xffffffffu
typedef struct {
    uint32_t group, side;                 /* group index, side 0 | 1; an absorbed cell: DVT_JOIN_NO_GROUP, 0 */
    uint32_t tag, chip, col, row, delta;  /* delta canonical */
} dvt_join_cell;                          /* 28 bytes */
typedef struct {
    uint64_t candidates;                      /* (window, col, row, delta) evaluated */
    uint64_t open_emitted, open_stored;       /* open records: all, and those below cap_records */
    uint64_t absorbed_emitted, absorbed_stored;
    uint64_t matched;                         /* records whose slot has both sides */
    uint64_t groups, pairs;                   /* after the exclusion rule */
    uint32_t truncated, reserved;             /* DVT_JOIN_TRUNC_* */
} dvt_join_summary;                           /* 72 bytes */
typedef struct dvt_hunt_join dvt_hunt_join;
int dvt_stage_hunt_join_new(dvt_prover *p, const char *machine, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                            size_t cap_records, size_t cap_absorbed, uint32_t log_slots, dvt_hunt_join **join);
int dvt_stage_hunt_join_supply(dvt_prover *p, dvt_hunt_join *join, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep,
                               uint32_t log_n, const uint32_t *pub);
/* cols (host, n_cols entries in any order, repeats count once; or NULL = every main column) */
int dvt_stage_hunt_join_add(dvt_prover *p, dvt_hunt_join *join, uint32_t tag, uint32_t chip, const uint32_t *d_main,
                            const uint32_t *d_prep, uint32_t log_n, const uint32_t *pub, uint32_t row_first, uint32_t row_count,
                            const uint32_t *cols, uint32_t n_cols, uint64_t max_evals);
/* once, after the last add */
int dvt_stage_hunt_join_match(dvt_prover *p, dvt_hunt_join *join, dvt_join_summary *summary);
/* cells: the groups' cells, groups sorted by the lowest (tag, chip, row, col, delta) of their side 0, which is the side that
 * holds the group's lowest cell; inside a group side 0 first, each side in that order.  absorbed: sorted likewise.
 * *n_cells / *n_absorbed: ALL there are; min(cap, all) are written, so a count above its cap says the list is cut. */
int dvt_stage_hunt_join_result(dvt_prover *p, dvt_hunt_join *join, dvt_join_cell *cells, size_t cap_cells, size_t *n_cells,
                               dvt_join_cell *absorbed, size_t cap_absorbed, size_t *n_absorbed);
int dvt_stage_hunt_join_free(dvt_prover *p, dvt_hunt_join *join);

/* The two hashing kernels of the device verifier (dvt_prover_verify), driven at chosen shapes without a proof.  Both
 * take and return HOST arrays of canonical words (a word >= p is DVT_ERR_INPUT) and are synchronous.
 * dvt_stage_sponge_rows: n word vectors, concatenated in `words`, of lens[i] words each -> digests [n][8]: the sponge of
 * every vector (rate 8, overwrite mode, the ragged last block keeps the state words it does not overwrite). */
int dvt_stage_sponge_rows(dvt_prover *p, const uint32_t *words, const uint32_t *lens, size_t n, uint32_t *digests);
/* dvt_stage_verify_paths: n Merkle chains -> ok[n] (1: the chain ends in its root).  A chain starts from `start` at leaf
 * `leaf` (taken modulo 2^depth) of a tree of 2^depth leaves, natural-order pairing (the node on the left while the index
 * is below half the level's width); siblings [depth][8] from the leaf level upwards; with inject != NULL, after the level
 * l at which inject_at[l] != 0 the node is compressed once more with inject[l] ([depth][8]: the row digest of the shorter
 * matrices that join there).  depth = 0 compares `start` with `root`. */
typedef struct {
    const uint32_t *start;    /* [8] */
    uint32_t depth, leaf;
    const uint32_t *siblings; /* [depth][8] */
    const uint32_t *inject;   /* [depth][8] or NULL */
    const uint8_t *inject_at; /* [depth], with inject */
    const uint32_t *root;     /* [8] */
} dvt_path_chain;
int dvt_stage_verify_paths(dvt_prover *p, const dvt_path_chain *chains, size_t n, uint8_t *ok);
/* The node rule of the compact proof form (see dvt_proof_compact), host only, pure index logic: the nodes that n queries
 * at leaves indices[i] mod 2^depth of a tree of 2^depth leaves cannot compute themselves, as (level, index) pairs in
 * out_level_index [2 * count] in the order of the wire format.  Level s has 2^s nodes, parents pair (i, i + 2^(s-1)).
 * *n_out = count; at most `cap` pairs are written (out_level_index may be NULL with cap = 0).  depth <= 30. */
int dvt_stage_multipath_nodes(uint32_t depth, const uint32_t *indices, size_t n, uint32_t *out_level_index, size_t cap, size_t *n_out);
/* dvt_stage_verify_multipath: the tree kernel of the device verifier on one tree of 2^depth leaves whose n queries
 * (n <= 1024, depth <= 30) walk up together.  Query i opens leaf leaf_index[i] mod 2^depth with the digest leaf_digest[i];
 * with inject_at != NULL and inject_at[lh] != 0 (lh < depth) it also carries inject[lh][i], the row digest of the shorter
 * matrices that join at level lh.  nodes [n_nodes][8]: the listed nodes in dvt_stage_multipath_nodes' order (another count
 * than that function's is DVT_ERR_INPUT).  *ok = 1 when queries on a common node carry equal digests and the walk ends in
 * root.  HOST arrays of canonical words, synchronous, as dvt_stage_verify_paths. */
int dvt_stage_verify_multipath(dvt_prover *p, uint32_t depth, const uint32_t *leaf_index, const uint32_t *leaf_digest, size_t n,
                               const uint8_t *inject_at, const uint32_t *inject, const uint32_t *nodes, size_t n_nodes,
                               const uint32_t *root, uint8_t *ok);

/* ------------------------------------------------- machine-level entry points
 * A "machine" is a fixed list of chips (AIRs) compiled into the library:
 * "toy" (engine unit tests) and "rv32" (the RISC-V core machine).  Traces are
 * host arrays, canonical form, column-major. */
typedef struct {
    uint32_t chip_id;
    uint32_t log_n;
    const uint32_t *data; /* [width][2^log_n] */
} dvt_host_trace;
/* preprocessed commitment = the prover half of client.setup(elf) (src/main.rs:462) */
int dvt_machine_setup(dvt_prover *p, const char *machine, const dvt_host_trace *prep, size_t nprep,
                      dvt_pk **pk, uint8_t **vk, size_t *vk_len);
void dvt_pk_free(dvt_prover *p, dvt_pk *pk);
/* prove one shard from explicit main traces (sorted by chip id) */
int dvt_machine_prove(dvt_prover *p, const dvt_pk *pk, const dvt_host_trace *main, size_t nmain,
                      const uint32_t *public_values, size_t npub, uint8_t **proof, size_t *proof_len);
/* host-only; DVT_ERR_REJECTED + reason in *reason (release with dvt_free) when the proof is bad */
int dvt_machine_verify(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len,
                       uint32_t fri_queries, uint32_t pow_bits, char **reason);
/* dvt_machine_verify with the query part (every sponge, Merkle path, reduced opening and fold of every query) on the
 * handle's GPU (member 0, lane 0): same arguments, same return codes, same *reason text for EVERY input.  p == NULL is
 * DVT_ERR_INPUT; a HIP failure is DVT_ERR_DEVICE with the text in dvt_last_error (there is no fallback to the host path). */
int dvt_prover_machine_verify(dvt_prover *p, const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len,
                              uint32_t fri_queries, uint32_t pow_bits, char **reason);
/* per-stage milliseconds of the last dvt_machine_prove on this handle (needs "profile":1):
 * out[0..5] = commit_main, permutation, quotient, openings, fri, total */
int dvt_last_stage_ms(dvt_prover *p, float out[6]);
/* kernel-family totals of the last prove on this handle (needs "profile":1), measured with HIP
 * events on the prover stream: out[0] = K1 LDE milliseconds, out[1] = K1 algorithmic bytes
 * (12 B per input element: read N, write 2N words per column), out[2] = K1 calls,
 * out[3] = K2+K3 (trace commitments) milliseconds, out[4] = Poseidon2 permutations they ran,
 * out[5..8] = committed cells of the shard in field elements: main, permutation, quotient (both
 * flattened over F_p^4), preprocessed -- the M, P, Q, Pre of SURVEY.md section 8d */
int dvt_last_kernel_stats(dvt_prover *p, double out[9]);

/* ------------------------------------------------- the reference's boundary
 * These five calls are what the reference's FFI for this path binds
 * (INTEGRATION.md).  ELF = RV32IM guest; stdin = list of byte buffers exactly
 * as SP1Stdin::write / write_vec push them (src/main.rs:434-437,458-460). */
typedef struct {
    const uint8_t *data;
    size_t len;
} dvt_buf;
typedef struct {
    uint64_t cycles;
    int32_t exit_code;    /* a0 at HALT; -1 if the guest never halted */
    uint32_t halted;
    uint32_t unprovable;  /* retired an instruction without a chip (prove would return DVT_ERR_UNSUPPORTED) */
} dvt_report;
/* The rest of SP1's ExecutionReport (counts per opcode and per syscall, and where the cycles go: counts per instruction and
 * per control transfer) is the execution report below: dvt_execute_profile on the host, dvt_rv32_job_profile on the GPU. */
/* client.setup(elf) (src/main.rs:462,482): decode the ELF, commit the preprocessed
 * tables (program, byte, memory image) on the GPU. */
int dvt_setup(dvt_prover *p, const uint8_t *elf, size_t elf_len, dvt_pk **pk, uint8_t **vk, size_t *vk_len);
/* client.execute(elf,&stdin).run() (src/main.rs:439-442,498-501): host-only emulation.
 * Returns DVT_ERR_GUEST when the guest halts with a non-zero exit code or traps
 * (the reference maps both to process exit code 1).  *public_values = the bytes the
 * guest wrote to fd 3 with the WRITE syscall (sp1_zkvm::io::commit, reference
 * crates/finalization_prove/src/main.rs:26-32), i.e. what SP1PublicValues holds;
 * *err_text (optional) = trap reason; both via dvt_free.
 * Guest syscall ABI (SP1's): t0 = id, a0..a2 = arguments: 0x00 HALT(code),
 * 0x02 WRITE(fd, ptr, len), 0x10 COMMIT(index, word) - the eight words of SHA-256(public-value bytes),
 * which the proof binds -, 0x1A COMMIT_DEFERRED_PROOFS (no-op), 0xF0 HINT_LEN, 0xF1 HINT_READ(ptr, len).
 * Precompiles (SP1 syscall codes with byte 1 = 1, proven by their own chips): 0x00_30_01_05 SHA_EXTEND(w) and
 * 0x00_01_01_06 SHA_COMPRESS(w, state), the two calls of SP1's patched `sha2` crate; the BLS12-381 accelerators (Fp and
 * Fp2 add / sub / mul, affine G1 add and double), secp256k1 affine add and double, and the 256-bit multiply UINT256_MUL,
 * each proven by a chip of its own.  Any other precompile code traps ("unknown syscall"): no proof is produced. */
int dvt_execute(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                uint8_t **public_values, size_t *pv_len, dvt_report *report, char **err_text);
/* the same, also handing back what the guest wrote to the other file descriptors (SP1 forwards fd 1 / 2 to the
 * host's stdout / stderr while executing) */
int dvt_execute_io(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                   uint8_t **public_values, size_t *pv_len, uint8_t **stdout_bytes, size_t *stdout_len,
                   dvt_report *report, char **err_text);
/* client.prove(&pk,&stdin).run() (src/main.rs:463-466), SP1 "core" mode: execute,
 * generate traces, prove on the GPU.  The returned bytes are what proof.save(path)
 * (src/main.rs:472-474) would write. */
int dvt_prove_core(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, uint8_t **proof,
                   size_t *proof_len, dvt_report *report);
/* dvt_prove_core in pieces, so that callers (and bench.py) can spread the shards of one execution over
 * several GPUs.  An execution is cut into shards of 2^log_shard_size cycles (cfg "log_shard_size",
 * default 21).  All shards are proven with COMMON LogUp challenges derived from every shard's header
 * (dvt_rv32_header_words() = 13 words: main-trace Merkle root + 5 public values), which is the one
 * exchange step of the path (an all-gather of 52 bytes per shard):
 *   prepare        the executor pipeline: one sequential fast pass of the guest cuts the execution into
 *                  shards; the shards this job owns (prepare: all; prepare_part: first, first + stride, ...)
 *                  are re-executed in trace mode on host threads, uploaded (compact 48-byte per-cycle
 *                  records; the events of the shift, muldiv, SHA and field / curve precompile chips and the rows of
 *                  the mem_init table, from which the GPU builds those chips' trace rows: the host builds no trace
 *                  row) and taken through phase 1 on the GPU as they arrive
 *   commit_shard   header of shard i (global position in the execution); phase 1 = K0 + K1..K3 of the
 *                  main traces runs here only if the pipeline's result has been consumed by an earlier proof
 *   challenges     host-only: the common challenges from ALL headers (in shard order)
 *   prove_shard    phase 2 of shard i: K0..K9 with those challenges -> shard proof bytes.  With more than one lane
 *                  the first call of a job starts a pipeline that proves the job's held shards with a valid header, in
 *                  job order from i, on the lanes, at most `lanes` shards past the last one asked for; the call returns
 *                  when shard i is done, and later calls with the SAME challenges collect their shard from the pipeline.
 *                  A call with other challenges, or for a shard the pipeline does not hold, stops it first (unclaimed
 *                  results are discarded) and then counts as a first call (a shard whose phase-1 result was consumed is
 *                  proven on lane 0 alone).  dvt_job_free, commit_shard, prepare, the stage entry points, dvt_sync and every
 *                  other call on the handle stop it too.  An error is that of the lowest failed shard.
 *   assemble       container (what proof.save would write) from the shard proofs, in order
 * dvt_rv32_prove_job runs everything on the handle's GPU; proof may be NULL to discard the bytes. */
typedef struct dvt_job dvt_job;
int dvt_rv32_prepare(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, dvt_job **job,
                     dvt_report *report);
int dvt_rv32_prepare_part(dvt_prover *p, const dvt_pk *pk, const dvt_buf *stdin_bufs, size_t nbuf, size_t first,
                          size_t stride, dvt_job **job, dvt_report *report);
/* words per shard header (13) */
uint32_t dvt_rv32_header_words(void);
/* seconds the GPU-side thread of the last prepare spent waiting for the host executor (0 = fully hidden); on a handle
 * with several members, of the member thread that waited longest */
double dvt_rv32_job_exec_wait_seconds(const dvt_job *job);
int dvt_rv32_prove_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint8_t **proof, size_t *proof_len);
void dvt_job_free(dvt_prover *p, dvt_job *job);
/* shards of the whole execution (a prepare_part job holds only its share of them) */
size_t dvt_rv32_job_shards(const dvt_job *job);
/* the device member that holds shard `shard` (global position in the execution): 0 on a one-device handle; -1 when this
 * job does not hold the shard */
int dvt_rv32_job_shard_member(const dvt_job *job, size_t shard);
/* bit mask over the chip ids of the rv32 machine (2 cpu, 4 mem_init, 5 shift, 6 muldiv, 7 sha_extend, 8 sha_compress,
 * 9..13 the field / curve precompile chips): bit c is set when the trace rows of chip c of shard `shard` (global position)
 * were built on the GPU from uploaded events, not uploaded as a table.  0 for a shard this job does not hold. */
uint32_t dvt_rv32_job_shard_device_rows(const dvt_job *job, size_t shard);
/* bit mask over the chip ids: the chip tables shard `shard` (global position) consists of.  0 for a shard this job does
 * not hold. */
uint32_t dvt_rv32_job_shard_chips(const dvt_job *job, size_t shard);
/* width and height (log2 of the rows) of the main trace of chip `chip` of that shard; DVT_ERR_INPUT when the job does not hold
 * the shard, the shard has no table of that chip, or a pointer is NULL.  Host-only. */
int dvt_rv32_job_shard_chip_shape(const dvt_job *job, size_t shard, uint32_t chip, uint32_t *main_w, uint32_t *log_n);
/* What a committed shard keeps in HBM for phase 2 ("keep_phase1" at dvt_prover_create).  The proof bytes are identical in
 * every tier. */
#define DVT_KEEP_NONE 0 /* nothing: phase 2 runs K0, the main LDEs and the main commitment again */
#define DVT_KEEP_TREE 1 /* the main Merkle tree and its root: phase 2 runs K0 and the main LDEs again, hashes nothing */
#define DVT_KEEP_FULL 2 /* K0 output, main LDEs and tree: phase 2 starts at the permutation trace */
/* the tier of shard `shard` (global position) from its last phase 1 (inside prepare, commit_shard or prove_job); a shard
 * keeps its buffers, and with them its tier, until the job is freed.  -1 when the job does not hold the shard or no
 * phase 1 of it has run.  Like the getters above it takes no lock: call it between calls on the job. */
int dvt_rv32_job_shard_kept(const dvt_job *job, size_t shard);
/* the bytes that tier holds in HBM: the tree, ((2 << hmax) - 1) * 32 with hmax = 1 + the largest log_n of the shard's
 * chips, for DVT_KEEP_TREE; tree + main LDEs (8 * main_w << log_n per chip) + the K0 buffers for DVT_KEEP_FULL; else 0.
 * (Sizes asked for: the buffer cache may hand out slightly larger buffers.) */
uint64_t dvt_rv32_job_shard_kept_bytes(const dvt_job *job, size_t shard);
int dvt_rv32_commit_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, uint32_t *header);
int dvt_rv32_challenges(const uint8_t *vk, size_t vk_len, const uint32_t *headers, size_t n_shards, uint32_t out[8]);
int dvt_rv32_prove_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, const uint32_t challenges[8],
                         uint8_t **proof, size_t *proof_len);
int dvt_rv32_assemble(const dvt_job *job, const uint8_t *const *shard_proofs, const size_t *lens, size_t n_shards,
                      uint8_t **proof, size_t *proof_len);
/* Check the trace rows of a prepared job against the AIR on the GPU, before (or instead of) proving: a wrong row otherwise
 * shows up only as a proof that dvt_verify rejects.  For every shard the job holds, on the device member that holds it:
 * the traces phase 1 kept in HBM are reused when they are valid, else K0 runs into the working buffers; every chip table
 * is checked (dvt_stage_check_constraints) against its preprocessed trace from the proving key; the per-bus LogUp sums
 * (dvt_stage_bus_sums) are accumulated.  The job is left as it was found (headers, phase-1 results and kept traces stay
 * valid or invalid as they were): a dvt_rv32_prove_job after the check returns the bytes it would have returned without.
 * Like every call on the handle it stops a running prove_shard pipeline first.
 * The point xi and the LogUp challenges are drawn from a transcript over a domain tag, the verifying key, the job's
 * public-value bytes and its shard count - NOT from the shard headers: the check works at any point of a job's life and
 * needs no phase 1.  They do not depend on the rows, so this is a diagnostic for honest-but-buggy rows (a K0 or guest-
 * restatement bug), not a soundness boundary: rows chosen after the challenges could pass it.
 * Bus balance is evaluated only when the job holds every shard of the execution (otherwise bus_checked = 0): the sums over
 * all chips and shards must vanish on every bus except the sys bus, which must equal the verifier's term for the
 * COMMITted public-value digest.
 * findings: one entry per (shard, chip) with violations, ordered by shard (global position), then chip; at most cap are
 * written, summary->n_findings counts all.  summary->ms: wall-clock milliseconds of the call after the entry guard.
 * Returns DVT_OK for a clean job; DVT_ERR_REJECTED when anything is violated or unbalanced, and dvt_last_error then names
 * the first finding (shard, chip name, row, constraint index) or the unbalanced buses. */
typedef struct {
    uint32_t shard, chip, log_n;
    dvt_check_result r;
} dvt_check_finding;
typedef struct {
    uint64_t violations;
    uint32_t n_findings, bus_checked, unbalanced_buses; /* bit b = bus b */
    float ms;
} dvt_check_summary;
int dvt_rv32_check_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, dvt_check_finding *findings, size_t cap,
                       dvt_check_summary *summary);
/* The same two hunts (dvt_stage_hunt_cells with pairs = 0: free_counts, free_map; dvt_stage_hunt_pairs with pairs = 1: cols,
 * n_cols, adjacent, out, cap, n_reported, n_tried; the other group is ignored) on chip `chip` of shard `shard` of a prepared
 * job.  The traces are taken as dvt_rv32_check_job takes them, the preprocessed trace comes from the proving key, and the job
 * is left as found: dvt_rv32_prove_job afterwards returns the bytes it would have returned without the hunt.  A shard the
 * job does not hold, or one without a table of that chip, is DVT_ERR_INPUT. */
int dvt_rv32_hunt_shard(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, uint32_t chip, uint64_t seed,
                        const uint32_t *deltas, uint32_t n_deltas, uint32_t pairs, const uint32_t *cols, uint32_t n_cols,
                        uint32_t adjacent, uint32_t row_first, uint32_t row_count, uint64_t max_evals, uint32_t *free_counts,
                        uint8_t *free_map, dvt_escape *out, size_t cap, uint64_t *n_reported, uint64_t *n_tried);
/* The join hunt (dvt_stage_hunt_join_*) over windows of a prepared job's tables.  A window is (shard, chip, row_first,
 * row_count), row_count 0 = from row_first to the end of the table; its tag is the shard index.  Traces are taken as
 * dvt_rv32_hunt_shard takes them, one shard after the other in the order of their first window; the supply tables are the
 * tables of supply_chips (n_supply may be 0) in the FIRST window's shard.  cols_count (or NULL = every main column of every
 * window) gives each window's number of listed columns, 0 = every column, and cols holds the lists one after the other.
 * Outputs as dvt_stage_hunt_join_match and dvt_stage_hunt_join_result give them, written only by a call that returns DVT_OK.
 * The job is left as found: dvt_rv32_prove_job afterwards returns the bytes it would have returned without the hunt.
 * All windows must lie on shards held by ONE member of the handle, else DVT_ERR_UNSUPPORTED: the join's supply set, record
 * arrays and table live on one lane of one device, and joining across devices is out of scope.  DVT_ERR_INPUT: what the
 * stage calls refuse, no window, a shard the job does not hold, a chip the shard has no table of. */
typedef struct {
    uint32_t shard, chip, row_first, row_count;
} dvt_join_window;
int dvt_rv32_hunt_join_job(dvt_prover *p, const dvt_pk *pk, dvt_job *job, const dvt_join_window *windows, size_t n_windows,
                           const uint32_t *supply_chips, uint32_t n_supply, uint64_t seed, const uint32_t *deltas, uint32_t n_deltas,
                           const uint32_t *cols, const uint32_t *cols_count, uint64_t max_evals, size_t cap_records,
                           size_t cap_absorbed, uint32_t log_slots, dvt_join_summary *summary, dvt_join_cell *cells, size_t cap_cells,
                           size_t *n_cells, dvt_join_cell *absorbed, size_t cap_absorbed_out, size_t *n_absorbed);
/* The unmatched LogUp tuples of a job (the bus ledger, dvt_stage_bus_ledger_*): what dvt_rv32_check_job's bus mask stands
 * for.  The traces of every shard the job holds are taken as dvt_rv32_check_job takes them, on the device that holds the
 * shard, and the job is left as found; first_tag is the shard's position, first_chip 0xffffffff one of the eight verifier-
 * side COMMIT tuples, which are always added.  With several devices each tallies into a ledger of its own; the host adds
 * the tallies, hands the dirty buckets back and merges the records by exact tuple.  On a job that holds only part of the
 * execution the result is what does not cancel among the held shards.  An honest whole job returns no tuple after the
 * TALLY pass alone.  2^20 buckets, 2^16 records, the seed from the check's transcript; when the records overflow the call
 * runs once more with another seed, and *truncated is set if that overflows too (or cap is too small). */
int dvt_rv32_job_bus_tuples(dvt_prover *p, const dvt_pk *pk, dvt_job *job, dvt_bus_tuple *out, size_t cap, size_t *n_tuples,
                            uint32_t *truncated);
/* The execution report of a prepared job: what retired how often, tallied on the GPU from the cycle records of the shards the
 * job holds (one launch per shard on the device that holds it; the records are only read and the job is left as found, so a
 * dvt_rv32_prove_job afterwards returns the bytes it would have returned without).  On a prepare_part job the report covers
 * the held shards only (summary->shards_tallied of summary->shards_total).
 *   pc_count[i]   how often instruction i = (pc - text_base) / 4 of the text retired (instructions without a chip included);
 *                 n_instr entries, always exact
 *   edges         a record whose successor (the next record; for the last record of a shard the instruction at the shard's
 *                 next_pc; none after HALT) is not instruction i + 1 is a transfer; every distinct (from_pc, to_pc) is an edge
 *                 with its count, sorted by (from_pc, to_pc).  The table of the edges of indirect jumps (JALR) is bounded and
 *                 insert-only: 2^log_edge_slots slots per device, 3..24, 0 = the smallest power of two of at least
 *                 4 n_instr and at least 2^10; a transfer whose edge finds no slot in 64 probes adds to dropped_transfers.
 *                 Always: the counts of all edges + dropped_transfers = n_transfers, and an edge that is returned carries
 *                 its exact count.  (The taken edges of branches and JAL are static and never dropped.)
 *   sys           ECALL records by syscall id (t0), sorted by id, always exact; a 65th distinct id is DVT_ERR_UNSUPPORTED
 *   ops           pc_count summed by the lowercase RISC-V mnemonic of the raw instruction word (lui auipc jal jalr beq bne
 *                 blt bge bltu bgeu lb lh lw lbu lhu sb sh sw addi slti sltiu xori ori andi slli srli srai add sub sll slt
 *                 sltu xor srl sra or and mul mulh mulhsu mulhu div divu rem remu ecall fence, else "unknown"), the names
 *                 with a non-zero count, sorted by count descending, then by name
 *   summary       cycles = the sum of pc_count (for a whole execution dvt_report.cycles); ms = wall clock of the call after
 *                 the entry guard
 * Every array takes at most its cap entries (the first ones of the order above; pc_count its first cap_pc); the summary
 * counts all, so NULL arrays with caps of 0 ask for the sizes.  DVT_ERR_INPUT: a NULL handle, key, job or summary, a NULL
 * array with a cap, log_edge_slots outside 0, 3..24, a key or job of a handle with other devices.  DVT_ERR_DEVICE: a HIP
 * failure.  Like every call on the handle it stops a running prove_shard pipeline first. */
typedef struct {
    uint32_t from_pc, to_pc;
    uint64_t count;
} dvt_profile_edge;
typedef struct {
    uint32_t id, pad;
    uint64_t count;
} dvt_profile_syscall;
typedef struct {
    char name[8];
    uint64_t count;
} dvt_profile_opcode;
typedef struct {
    uint64_t cycles, n_transfers, dropped_transfers;
    uint32_t text_base, n_instr, n_edges, n_syscalls, n_opcodes, shards_tallied, shards_total;
    float ms;
} dvt_profile_summary;
int dvt_rv32_job_profile(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t log_edge_slots, uint64_t *pc_count, size_t cap_pc,
                         dvt_profile_edge *edges, size_t cap_edges, dvt_profile_syscall *sys, size_t cap_sys,
                         dvt_profile_opcode *ops, size_t cap_ops, dvt_profile_summary *summary);
/* The same report on the host alone (no GPU is touched): the guest runs in trace mode shard by shard (2^21 cycles, at most
 * one shard's records in memory) and the records go through the same rule in plain C++; nothing is bounded, so
 * dropped_transfers is 0.  Return codes, *report and *err_text as dvt_execute gives them; the report is filled for whatever
 * retired, also when the guest fails.  An instruction without a chip (FENCE) is counted under its mnemonic. */
int dvt_execute_profile(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                        uint64_t *pc_count, size_t cap_pc, dvt_profile_edge *edges, size_t cap_edges, dvt_profile_syscall *sys,
                        size_t cap_sys, dvt_profile_opcode *ops, size_t cap_ops, dvt_profile_summary *summary, dvt_report *report,
                        char **err_text);
/* The call-tree report of a prepared job: inclusive and self cycles per function and per caller -> callee arc, from the cycle
 * records of the shards the job holds (read only; the job is left as found).  Positions g = 0 .. C - 1 number the records in
 * execution order across shards; the successor of a record is the execution report's.  From the raw instruction word alone,
 * a `jal` / `jalr` with rd == x1 is a CALL (none when it has no successor in the text) and `jalr x0, 0(x1)` is a RET; nothing
 * else is an event, so a tail jump stays in the frame of the function that was called.  A function is named by the pc of
 * its entry.  The stack starts with the root frame (the instruction the first record names, open at 0).  A CALL at g with
 * successor s pushes {s, open = g + 1}: the call instruction belongs to the caller.  A RET at g pops the top frame F,
 * WHATEVER ADDRESS IT RETURNS TO, and the arc (caller of F, F) gets calls += 1, cycles += g + 1 - F.open; a RET that finds
 * only the root adds to unmatched_returns and the root stays.  After the last record every open frame is closed at C, the
 * root last: its arc (0xffffffff, entry) has cycles = C, and open_at_exit counts the frames closed this way.
 *   arcs      every distinct (caller_pc, callee_pc) with its calls and cycles, sorted by (caller_pc, callee_pc).  On the
 *             device the arcs are added up in an insert-only table of 2^log_arc_slots slots per device (3..24; 0 = sized
 *             from the text as dvt_rv32_job_profile sizes its edge table); a closed frame whose arc finds no slot in 64
 *             probes adds to dropped_frames and dropped_cycles.  Always: the calls of all arcs + dropped_frames = n_frames,
 *             and an arc that is returned carries its exact sums.
 *   funcs     per callee: calls and inclusive = the sums over the arcs into it, self = inclusive - the cycles of the arcs
 *             out of it; sorted by self descending, then by pc.  Recursion counts nested frames of one function more than
 *             once in inclusive, never in self: the self cycles of all functions sum to summary->cycles.  When
 *             dropped_frames > 0 the table cannot be made: n_funcs is 0 and funcs is not filled.
 *   summary   cycles = C; n_frames = the frames closed; max_depth = the deepest stack, the root included; ms = wall clock of
 *             the call after the entry guard
 * Arrays, caps, the size query and DVT_ERR_INPUT as dvt_rv32_job_profile (log_arc_slots outside 0, 3..24; a cycle record that
 * names an instruction outside the text).  DVT_ERR_UNSUPPORTED: a job that does not hold every shard of its execution
 * (dvt_rv32_prepare_part with an offset or a stride): the stack across a gap is unknown.  Handles with several members work:
 * the spans are merged on the host.  Like every call on the handle it stops a running prove_shard pipeline first. */
typedef struct {
    uint32_t caller_pc, callee_pc;   /* caller_pc 0xffffffff: the root */
    uint64_t calls, cycles;
} dvt_calltree_arc;
typedef struct {
    uint32_t pc, pad;
    uint64_t calls, inclusive, self;
} dvt_calltree_func;
typedef struct {
    uint64_t cycles, n_frames, dropped_frames, dropped_cycles, unmatched_returns;
    uint32_t text_base, n_instr, n_arcs, n_funcs, max_depth, open_at_exit, shards_total;
    float ms;
} dvt_calltree_summary;
int dvt_rv32_job_calltree(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t log_arc_slots, dvt_calltree_arc *arcs,
                          size_t cap_arcs, dvt_calltree_func *funcs, size_t cap_funcs, dvt_calltree_summary *summary);
/* wall-clock milliseconds of the last dvt_rv32_job_calltree on this handle: summary mode (both runs, with their downloads),
 * the host's merge of the span summaries, emit mode (with its download) */
int dvt_rv32_job_calltree_times(dvt_prover *p, double out[3]);
/* The same report on the host alone (no GPU is touched), as dvt_execute_profile runs the guest: nothing is bounded, so nothing
 * is dropped.  Return codes, *report and *err_text as dvt_execute gives them; the tables are filled for whatever retired, also
 * when the guest fails. */
int dvt_execute_calltree(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                         dvt_calltree_arc *arcs, size_t cap_arcs, dvt_calltree_func *funcs, size_t cap_funcs,
                         dvt_calltree_summary *summary, dvt_report *report, char **err_text);
/* The memory report of a prepared job: which pages the execution loads from and stores to, how many distinct words it
 * accesses, which instructions access words first, and how far the stack pointer moves; from the cycle records of the shards
 * the job holds (one launch per shard on the device that holds it; the records are only read and the job is left as found,
 * so a dvt_rv32_prove_job afterwards returns the bytes it would have returned without).  Every distinct word an execution
 * accesses is a row of the mem_init table of the last shard: the report names what makes that table tall.
 * Words are the 4-byte aligned guest addresses below 0x38000000, pages are 4096 bytes; the registers are never part of the
 * report (nor is the a1 read that ECALLs make through the memory port).
 *   loads, stores   a record whose instruction is lb lh lw lbu lhu is one load, sb sh sw one store, of the word at
 *                   (rs1 value + offset) & ~3
 *   first touches   a load or store whose word no shard accessed before (the previous shard of the access is 0; shards are
 *                   numbered from 1) is the first access of that word in the whole execution, whether the word is part of
 *                   the image, was hinted (HINT_READ sets initial values without an access: the load that reads a hinted
 *                   word touches it first) or neither: first_touch[i] counts them per instruction i = (pc - text_base) / 4,
 *                   n_instr entries; `first` of a page per page
 *   precompiles     from the ECALL record (t0, a0, a1): SHA_EXTEND is 16 reads and 48 writes of the 64 words at a0;
 *                   SHA_COMPRESS 64 reads at a0, 8 reads and 8 writes at a1; a field, curve or u256 call reads its second
 *                   operand at a1 and reads and writes its first at a0.  They count into pre_reads / pre_writes of the page
 *                   of each word (an array may straddle a page) and into pre_calls.  HALT, WRITE, COMMIT, HINT_LEN and
 *                   HINT_READ access nothing in this sense.
 *   words           of a page: the distinct words any counted access hit.  The records do not say whether a precompile word
 *                   was touched first by the call, but on a whole execution words - first_touches (of the summary) is the
 *                   number of words first touched by a precompile call.
 *   pages           every page with at least one counted access, sorted by address (`page` is its byte address)
 *   stack           over the records whose instruction has rd == x2: sp_writes, and sp_min / sp_max of the value written
 *                   (all three 0 without such a record)
 *   summary         the totals of the above, n_pages; image_words = the words of the program image, image_words_accessed =
 *                   those of them that were accessed; mem_init_rows = 32 + image_words + words - image_words_accessed, the
 *                   rows of the mem_init table before padding, when the job holds every shard of its execution, else 0;
 *                   ms = wall clock of the call after the entry guard
 * On a prepare_part job the report covers the held shards (shards_tallied of shards_total): counters are sums, words is
 * distinct over the held shards, mem_init_rows is 0.  Handles with several members work: the host merges the members'
 * tables.  Nothing is bounded or probabilistic: every figure is exact and nothing can be dropped.
 * Arrays, caps, the size query, DVT_ERR_INPUT and DVT_ERR_DEVICE as dvt_rv32_job_profile (also DVT_ERR_INPUT: a cycle record
 * that names an instruction outside the text or an address outside guest memory).  Like every call on the handle it stops a
 * running prove_shard pipeline first. */
typedef struct {
    uint32_t page, words, first, pad;   /* page: byte address */
    uint64_t loads, stores, pre_reads, pre_writes;
} dvt_memory_page;
typedef struct {
    uint64_t cycles, loads, stores, pre_reads, pre_writes, pre_calls, words, first_touches, image_words, image_words_accessed, mem_init_rows, sp_writes;
    uint32_t sp_min, sp_max, text_base, n_instr, n_pages, page_bytes, shards_tallied, shards_total;
    float ms;
} dvt_memory_summary;
int dvt_rv32_job_memory(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint64_t *first_touch, size_t cap_instr, dvt_memory_page *pages,
                        size_t cap_pages, dvt_memory_summary *summary);
/* The same report on the host alone (no GPU is touched), as dvt_execute_profile runs the guest: shard by shard through the
 * same rule in plain C++.  Return codes, *report and *err_text as dvt_execute gives them; the tables are filled for whatever
 * retired, also when the guest fails (mem_init_rows then counts the words accessed so far). */
int dvt_execute_memory(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles,
                       uint64_t *first_touch, size_t cap_instr, dvt_memory_page *pages, size_t cap_pages, dvt_memory_summary *summary,
                       dvt_report *report, char **err_text);
/* Watchpoints on a prepared job: the cycle records of the shards the job holds are searched, every record against up to
 * DVT_WATCH_MAX_QUERIES queries (one launch per shard on the device that holds it; the records are only read and the job is
 * left as found).  A record is a hit of a query at most once.  The rule is stated in csrc/watch.h:
 *   DVT_WATCH_PC    the record's pc (text_base + 4 idx) lies in [lo, hi)
 *   DVT_WATCH_REG   the instruction has rd == lo (1..31; x0 never hits); the value is the one written.  With DVT_WATCH_VALUE
 *                   in flags the hit also requires (value & mask) == (want & mask).
 *   DVT_WATCH_MEM   a memory access in the sense of the memory report whose word address lies in [lo, hi); flags selects
 *                   among DVT_WATCH_LOAD, _STORE, _PRE_READ and _PRE_WRITE (at least one).  A load or store accesses the word
 *                   (rs1 value + offset) & ~3: `before` is the word before the access, `after` the word after it (a load
 *                   leaves it; sw writes rs2, sh / sb merge the half or byte of rs2 at the byte offset of the address).
 *                   DVT_WATCH_VALUE tests `after`, of loads and stores only.  A precompile ECALL (the shapes of the memory
 *                   report) hits when any word of its arrays lies in the range with a selected direction: one hit per call,
 *                   addr = the lowest such word, n_words = how many entries of the call's arrays matched (a word that both
 *                   arrays hold counts twice), flags = the selected directions that matched | DVT_WATCH_HIT_NO_VALUE; the
 *                   values of those words are not in the records: before = after = 0 and a VALUE filter never matches.
 *   window          only records at positions from <= (shard, row) < to, compared lexicographically, are searched: shard is
 *                   the shard's number in the execution (from 1, also on a prepare_part job), row the index of the record in
 *                   its shard (the row of the shard's cpu table; the memory timestamps of the row are 4 row + 4 .. 4 row + 7).
 *                   from = (0, 0) and to = (0xffffffff, 0xffffffff) search everything.
 * A hit carries the position, pc and idx, the values written and read (rd_value = a, rs1 = b, rs2 = c of the record), the
 * query's kind, and for a load or store under whichever kind of query: its direction in flags, addr, n_words = 1, before, after
 * and the previous access of the word as (prev_shard, prev_clk), (0, 0) when the access is the first of the word.  Searching
 * again with to = the position of that access walks the history of a word backwards.
 * Per query q the call returns totals[q], the exact number of hits in the window, the first min(cap_each, total) hits in
 * execution order in hits[2 q cap_each ...] and the last min(cap_each, total) in hits[(2 q + 1) cap_each ...] (the lists overlap
 * when total < 2 cap_each); the rest of `hits` is left as found.  cap_each may be 0 (totals only; hits may then be NULL).
 * Nothing is sampled: totals and order are exact whatever cap_each is.
 * DVT_ERR_INPUT: n_queries 0 or above DVT_WATCH_MAX_QUERIES, cap_each above DVT_WATCH_MAX_KEEP, an unknown kind, a flag the
 * kind does not take (or a MEM query without a direction), lo >= hi, a register outside 1..31, from >= to, null arrays, a
 * cycle record that names an instruction outside the text or an address outside guest memory.  Handles with several members
 * and prepare_part jobs work: positions stay those of the execution. */
#define DVT_WATCH_MAX_QUERIES 16
#define DVT_WATCH_MAX_KEEP 256
#define DVT_WATCH_SPAN 4096   /* records one workgroup of the device pass searches */
enum { DVT_WATCH_PC = 1, DVT_WATCH_REG = 2, DVT_WATCH_MEM = 3 };
enum { DVT_WATCH_LOAD = 1, DVT_WATCH_STORE = 2, DVT_WATCH_PRE_READ = 4, DVT_WATCH_PRE_WRITE = 8, DVT_WATCH_VALUE = 16, DVT_WATCH_HIT_NO_VALUE = 32 };
typedef struct {
    uint32_t kind, flags, lo, hi, mask, want;
    uint32_t from_shard, from_row, to_shard, to_row;
} dvt_watch_query;
typedef struct {
    uint32_t query, shard, row, pc, idx, kind, flags, addr, n_words, before, after, rd_value, rs1, rs2, prev_shard, prev_clk;
} dvt_watch_hit;
typedef struct {
    uint64_t cycles;   /* records of the held shards (all of them are tested, the window is part of the test) */
    uint32_t n_queries, cap_each, shards_searched, shards_total, text_base, n_instr, span;
    float ms;          /* wall clock of the call after the entry guard */
} dvt_watch_summary;
int dvt_rv32_job_watch(dvt_prover *p, const dvt_pk *pk, dvt_job *job, const dvt_watch_query *queries, size_t n_queries, size_t cap_each,
                       dvt_watch_hit *hits, uint64_t *totals, dvt_watch_summary *summary);
/* milliseconds of the last dvt_rv32_job_watch, by events on the members' streams and summed over the members: the count
 * launches, the scan launches, the emit launches; out[3]: the shards the emit pass ran over */
int dvt_rv32_job_watch_times(dvt_prover *p, double out[4]);
/* The same search on the host alone (no GPU is touched), as dvt_execute_profile runs the guest, in shards of
 * 2^log_shard_size cycles (0: 21; 4..22) so that positions are those of a job prepared with that shard size; one shard's
 * records are held at a time and the last cap_each hits of a query are kept in a ring.  Return codes, *report and *err_text as
 * dvt_execute gives them (an input error of the queries: DVT_ERR_INPUT and its text); the lists are filled for whatever
 * retired, also when the guest fails. */
int dvt_execute_watch(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                      const dvt_watch_query *queries, size_t n_queries, size_t cap_each, dvt_watch_hit *hits, uint64_t *totals,
                      dvt_watch_summary *summary, dvt_report *report, char **err_text);
/* Snapshots of a prepared job: registers, memory words and the call stack as they are BEFORE the record at position
 * (shard, row) executes, from the cycle records the job holds (the records are only read and the job is left as found).
 * Positions compare lexicographically as the windows of the watchpoints do; a position past the last record means the state
 * after the last record, so (0xffffffff, 0xffffffff) is the state at exit (on the host path: at the trap).  The rule is stated
 * in csrc/snapshot.h:
 *   registers   regs[k], k = 1..31: value = the value written by the last record before the position whose instruction has
 *               rd == k, flags = DVT_SNAP_FROM_BEFORE and (shard, row, pc) of that record; without one value 0 and
 *               DVT_SNAP_INITIAL.  regs[0] is all zero.  addr = k.  Register values are always exact.
 *   memory      up to DVT_SNAP_MAX_RANGES ranges [lo, hi) of word addresses (4-aligned, below the guest's address limit),
 *               DVT_SNAP_MAX_WORDS words in all; `words` holds one cell per word, the ranges concatenated in their order.
 *               Loads, stores and the words a precompile call WRITES decide a word (the words a call only reads do not).
 *               B = the last deciding access of the word before the position, A = the first at or after it.  The first case
 *               that applies:
 *                 B is a store                  the word after B         FROM_BEFORE | STORE     source B
 *                 B is a load                   the word B read          FROM_BEFORE | LOAD      source B
 *                 A is a load or a store        the word before A        FROM_AFTER (| INITIAL when there is no B)   source A
 *                 no B, a word of the image     the image's word         IMAGE | INITIAL         no source (0, 0, 0)
 *                 otherwise                     0                        NO_VALUE                source B, else A
 *               DVT_SNAP_UNTOUCHED is added when neither B nor A exists.  A NO_VALUE cell says that the records do not hold
 *               the word: a precompile call wrote it and nothing loads it before the next such write (the limit of
 *               DVT_WATCH_HIT_NO_VALUE); it still names the call in (shard, row, pc).  INITIAL: nothing accessed the word before
 *               the position, and the value is the one the memory argument starts the word with: image, hint or 0.  A hinted
 *               word holds that value in the machine only from its HINT_READ on; a snapshot before it shows it early.
 *   call stack  the rule of the call-tree report over the records before the position; the frames still open are the
 *               backtrace, innermost first: fn_pc, the position of the frame's first record (open_shard, open_row), call_pc
 *               and ra = the pc of the call instruction (the record before) and the value it wrote (the root: 0xffffffff
 *               and 0).  summary.depth counts all frames, n_frames = min(cap_frames, depth) are returned.
 *   summary     position = the number of records before the position, (shard, row) = the position of record `position`
 *               (of the end: the last shard and its record count), pc = that record's pc, at the end the last shard's
 *               next_pc; cycles = all records; n_words and how many of them carry NO_VALUE, INITIAL and UNTOUCHED.
 * DVT_ERR_INPUT: more than DVT_SNAP_MAX_RANGES ranges or DVT_SNAP_MAX_WORDS words, a misaligned or empty range, a range that
 * reaches past the address limit, cap_words below the words asked for, null arrays, a cycle record that names an instruction
 * outside the text or an address outside guest memory.  DVT_ERR_UNSUPPORTED: a prepare_part job that does not hold every
 * shard of its execution.  Handles with several members work. */
#define DVT_SNAP_MAX_RANGES 16
#define DVT_SNAP_MAX_WORDS 4096
#define DVT_SNAP_SPAN 4096   /* records one workgroup of the device pass reduces */
enum { DVT_SNAP_INITIAL = 1, DVT_SNAP_FROM_BEFORE = 2, DVT_SNAP_FROM_AFTER = 4, DVT_SNAP_LOAD = 8, DVT_SNAP_STORE = 16, DVT_SNAP_IMAGE = 32,
       DVT_SNAP_NO_VALUE = 64, DVT_SNAP_UNTOUCHED = 128 };
typedef struct { uint32_t lo, hi; } dvt_snap_range;
typedef struct { uint32_t addr, value, flags, shard, row, pc; } dvt_snap_cell;   /* addr: the register number of a register */
typedef struct { uint32_t fn_pc, call_pc, open_shard, open_row, ra, pad; } dvt_snap_frame;
typedef struct {
    uint64_t position, cycles;
    uint32_t shard, row, pc, depth, n_frames, unmatched_returns, n_words, no_value, initial, untouched, shards_total, text_base, n_instr, span;
    float ms;          /* wall clock of the call after the entry guard */
} dvt_snap_summary;
int dvt_rv32_job_snapshot(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, const dvt_snap_range *ranges,
                          size_t n_ranges, dvt_snap_cell regs[32], dvt_snap_cell *words, size_t cap_words, dvt_snap_frame *frames,
                          size_t cap_frames, dvt_snap_summary *summary);
/* milliseconds of the last dvt_rv32_job_snapshot, by events on the members' streams and summed over the members: the reduce
 * launches, the gather launches, the backtrace's call-tree launches */
int dvt_rv32_job_snapshot_times(dvt_prover *p, double out[3]);
/* The same snapshot on the host alone (no GPU is touched), the guest run in shards of 2^log_shard_size cycles (0: 21; 4..22)
 * as dvt_execute_watch runs it, one shard's records held at a time.  Return codes, *report and *err_text as dvt_execute gives
 * them; the outputs are filled for whatever retired, also when the guest fails: at (0xffffffff, 0xffffffff) they are the
 * post-mortem of a guest that traps. */
int dvt_execute_snapshot(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                         uint32_t shard, uint32_t row, const dvt_snap_range *ranges, size_t n_ranges, dvt_snap_cell regs[32],
                         dvt_snap_cell *words, size_t cap_words, dvt_snap_frame *frames, size_t cap_frames, dvt_snap_summary *summary,
                         dvt_report *report, char **err_text);
/* Origins of a prepared job: the backward data-flow slice of one value, from the cycle records the job holds (the records are
 * only read, nothing is executed again, the job is left as found).  The call names a position (shard, row) as the snapshot does
 * ((0xffffffff, 0xffffffff): the exit) and a target: what = DVT_ORIGIN_REG with target = k in 1..31 for the value x_k holds
 * before the position, or DVT_ORIGIN_WORD with target = a 4-aligned address below the guest's address limit for the word before
 * the position.  The rule is stated in csrc/origin.h:
 *   question    (what, target, Q): the last record before position Q that WRITES the target.  A register: the last record whose
 *               instruction has rd == k (the snapshot's rule: ECALL writes t0).  A word: the last store (sw / sh / sb) to it or
 *               precompile call that writes it; loads are no writers.  Without such a record the target is INITIAL.
 *   nodes       one per record of the slice, in discovery order (level by level): the fields of a watchpoint hit (shard, row, pc,
 *               idx, rd_value, rs1, rs2 and, of a load or store, addr, before, after), kind = DVT_ORIGIN_OP / _LOAD / _STORE /
 *               _CALL (an ECALL with a precompile shape) / _SYSCALL (any other ECALL), depth = its level, its input edges
 *               edges[first_edge .. first_edge + n_edges), flags = DVT_ORIGIN_UNEXPANDED when its inputs were not followed
 *               (depth == max_depth, or cap_edges was reached).
 *   edges       edge 0 is the root: from = DVT_ORIGIN_NONE, role ROOT, the question (what, target, position).  The input edges
 *               of a node depend on its record alone and ask at the node's own position, in this order: ADDR (loads and
 *               stores: register rs1; only with DVT_ORIGIN_FOLLOW_ADDR), RS1 (every other instruction that reads rs1, ECALL
 *               excepted), RS2 (every instruction that reads rs2, ECALL excepted; of a store the data), MEM (a load: the word
 *               it reads; sb / sh: the word whose other bytes they keep; a _CALL: one edge per word the call reads, array 0
 *               first).  No edge names x0.  role REG-like edges carry target = the register and value = the operand the record
 *               holds; MEM edges target = the word and value = the word before the access (of a _CALL: 0 and NO_VALUE).  The
 *               root's value is the writer's rd_value (REG), the store's `after` (WORD), NO_VALUE when a call wrote the word,
 *               the image's word with INITIAL | IMAGE or INITIAL | NO_VALUE without a writer.  to = the node of the writer,
 *               or DVT_ORIGIN_NONE with INITIAL (no writer; IMAGE: a word of the program image) or CUT (cap_nodes was
 *               reached); (src_shard, src_row) = the writer's position whenever there is one.
 *   summary     n_nodes, n_edges, depth = the deepest node's, the edges with CUT, INITIAL and NO_VALUE, the UNEXPANDED nodes,
 *               questions asked, levels answered, device passes (ceil(questions of the level / DVT_ORIGIN_PASS_QUESTIONS) per
 *               level; 0 on the host path), position / cycles / shard / row as the snapshot's summary.
 * Limits: the values of words a call read or wrote are not in the records; a hinted word nothing wrote is INITIAL; data
 * dependence only.  DVT_ERR_INPUT: what / target out of range, a flag other than FOLLOW_ADDR, cap_nodes, cap_edges or max_depth
 * above the limits, cap_edges 0, null arrays, a bad cycle record before the position.  DVT_ERR_UNSUPPORTED: a prepare_part job
 * that does not hold every shard of its execution.  Handles with several members work. */
#define DVT_ORIGIN_MAX_NODES 1024
#define DVT_ORIGIN_MAX_EDGES 8192
#define DVT_ORIGIN_MAX_DEPTH 64
#define DVT_ORIGIN_PASS_QUESTIONS 256   /* questions one device pass answers */
#define DVT_ORIGIN_SPAN 4096            /* records one workgroup of the device pass reduces */
#define DVT_ORIGIN_NONE 0xffffffffu
enum { DVT_ORIGIN_REG = 1, DVT_ORIGIN_WORD = 2 };                                                       /* what */
enum { DVT_ORIGIN_FOLLOW_ADDR = 1 };                                                                    /* flags of a call */
enum { DVT_ORIGIN_OP = 1, DVT_ORIGIN_LOAD = 2, DVT_ORIGIN_STORE = 3, DVT_ORIGIN_CALL = 4, DVT_ORIGIN_SYSCALL = 5 };   /* node kinds */
enum { DVT_ORIGIN_ROOT = 0, DVT_ORIGIN_ADDR = 1, DVT_ORIGIN_RS1 = 2, DVT_ORIGIN_RS2 = 3, DVT_ORIGIN_MEM = 4 };         /* edge roles */
enum { DVT_ORIGIN_INITIAL = 1, DVT_ORIGIN_IMAGE = 2, DVT_ORIGIN_NO_VALUE = 4, DVT_ORIGIN_CUT = 8, DVT_ORIGIN_UNEXPANDED = 16 };   /* flags of edges and nodes */
typedef struct { uint32_t shard, row, pc, idx, kind, depth, first_edge, n_edges, flags, rd_value, rs1, rs2, addr, before, after, pad; } dvt_origin_node;
typedef struct { uint32_t from, to, role, target, value, flags, src_shard, src_row; } dvt_origin_edge;
typedef struct {
    uint64_t position, cycles;
    uint32_t n_nodes, n_edges, depth, cut, unexpanded, initial, no_value, questions, levels, passes, shard, row, shards_total, span;
    float ms;          /* wall clock of the call after the entry guard */
} dvt_origin_summary;
int dvt_rv32_job_origin(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                        uint32_t max_depth, dvt_origin_node *nodes, size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges,
                        dvt_origin_summary *summary);
/* milliseconds of the last dvt_rv32_job_origin: the reduce launches and the gather launches by events on the members' streams,
 * summed over members, levels and passes; the host's share (the wall clock of the call less those two) */
int dvt_rv32_job_origin_times(dvt_prover *p, double out[3]);
/* The same slice on the host alone (no GPU is touched), the guest run in shards of 2^log_shard_size cycles (0: 21; 4..22) as
 * dvt_execute_snapshot runs it.  The records of the shards up to the position are kept, 48 bytes per cycle: past 2^24 of them the
 * call fails with DVT_ERR_UNSUPPORTED (dvt_rv32_job_origin is the way for such executions).  The questions of a level are answered
 * by one backward scan.  Return codes, *report and *err_text as dvt_execute gives them; the outputs are filled for whatever
 * retired, also when the guest fails: at (0xffffffff, 0xffffffff) a guest that traps is asked at its trap. */
int dvt_execute_origin(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                       uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, dvt_origin_node *nodes,
                       size_t cap_nodes, dvt_origin_edge *edges, size_t cap_edges, dvt_origin_summary *summary, dvt_report *report, char **err_text);
/* Uses of a prepared job: the forward data-flow slice of one value, from the cycle records the job holds (the records are only
 * read, nothing is executed again, the job is left as found).  The exact inverse of the origin relation above; the rule is stated
 * in csrc/uses.h:
 *   definition  (what, target, F): the value the register (DVT_USES_REG, 1..31) or the 4-aligned word below the address limit
 *               (DVT_USES_WORD) holds from position F on.  Its next writer N is the first record at a position >= F that writes the
 *               target as the origin search counts writers (rd == k, so ECALL writes t0; sw / sh / sb to the word; a call whose
 *               written words contain it); without one next_shard = next_row = DVT_USES_NONE and the flag LIVE_AT_EXIT.
 *   uses        every input edge (in the origin search's sense: roles ADDR, only with DVT_USES_FOLLOW_ADDR, RS1, RS2, MEM) of every
 *               record at a position in [F, N] that names the target.  N itself is included; a record that reads a register as rs1
 *               and as rs2 is two uses.  n_uses is exact; the first min(fan, n_uses) uses in execution order (within a record
 *               ADDR, RS1, RS2, MEM) are edges[first_edge .. first_edge + n_edges), TRUNCATED when n_uses > fan.
 *   defs        defs[0] is the root: node = DVT_USES_NONE, (what, target) as asked, F = the position ((0xffffffff, 0xffffffff):
 *               the exit, which has no uses); its value is what its first kept use read, else NO_VALUE.  The definitions of a
 *               node, F = its position + 1, in this order: rd when non-zero (value rd_value), the word of a store (value
 *               `after`), every word a call writes, array 0 first (value 0, NO_VALUE).
 *   edges       {def, to, role, flags, dst_shard, dst_row}: to = the consumer's node, or DVT_USES_NONE with CUT when cap_nodes was
 *               reached; (dst_shard, dst_row) = the consumer's position.
 *   nodes       one per consuming record in discovery order (breadth first: the definitions of level d give the nodes of depth
 *               d + 1), the fields of an origin node, with defs[first_def .. first_def + n_defs) in place of its edges.  UNEXPANDED:
 *               depth >= max_depth, or the node's definitions would take n_defs past cap_defs, or n_edges so far plus fan times
 *               the definitions of the level past cap_edges.  The edges of a level are known only after its answers, so room for
 *               fan edges is reserved per definition beforehand: the search may stop with fewer than cap_edges edges (never with
 *               more), the sooner the larger fan is.  That node and every later one stay unexpanded, and the search ends after
 *               the level's answers.  For the same reason cap_edges below fan is refused.
 *   summary     n_nodes, n_defs, n_edges, depth; the edges with CUT, the nodes UNEXPANDED, the definitions TRUNCATED, LIVE_AT_EXIT,
 *               NO_VALUE and dead (n_uses == 0); uses_total = the sum of n_uses; levels answered, device passes (ceil(definitions
 *               of the level / DVT_USES_PASS_DEFS) per level; 0 on the host path); position / cycles / shard / row as the
 *               snapshot's summary.
 * Limits: data dependence only (a branch is a consumer and a leaf); the values of words a call wrote are not in the records.
 * DVT_ERR_INPUT: what / target out of range, a flag other than FOLLOW_ADDR, fan outside 1..DVT_USES_MAX_FAN, a cap above its limit,
 * cap_defs 0, cap_edges below fan, null arrays, a bad cycle record at or after the position.  DVT_ERR_UNSUPPORTED: a prepare_part job
 * that does not hold every shard of its execution.  Handles with several members work. */
#define DVT_USES_MAX_NODES 1024
#define DVT_USES_MAX_DEFS 4096
#define DVT_USES_MAX_EDGES 8192
#define DVT_USES_MAX_DEPTH 64
#define DVT_USES_MAX_FAN 16
#define DVT_USES_DEFAULT_FAN 8
#define DVT_USES_PASS_DEFS 256   /* definitions one device pass answers */
#define DVT_USES_SPAN 4096       /* records one workgroup of a device pass reads */
#define DVT_USES_NONE 0xffffffffu
enum { DVT_USES_REG = 1, DVT_USES_WORD = 2 };                                                       /* what (= DVT_ORIGIN_*) */
enum { DVT_USES_FOLLOW_ADDR = 1 };                                                                  /* flags of a call */
enum { DVT_USES_OP = 1, DVT_USES_LOAD = 2, DVT_USES_STORE = 3, DVT_USES_CALL = 4, DVT_USES_SYSCALL = 5 };   /* node kinds (= DVT_ORIGIN_*) */
enum { DVT_USES_ADDR = 1, DVT_USES_RS1 = 2, DVT_USES_RS2 = 3, DVT_USES_MEM = 4 };                   /* edge roles (= DVT_ORIGIN_*) */
enum { DVT_USES_LIVE_AT_EXIT = 1, DVT_USES_TRUNCATED = 2, DVT_USES_NO_VALUE = 4, DVT_USES_CUT = 8, DVT_USES_UNEXPANDED = 16 };   /* flags of defs, edges and nodes */
typedef struct { uint32_t shard, row, pc, idx, kind, depth, first_def, n_defs, flags, rd_value, rs1, rs2, addr, before, after, pad; } dvt_uses_node;
typedef struct {
    uint64_t n_uses;
    uint32_t node, what, target, value, flags, next_shard, next_row, first_edge, n_edges, pad;
} dvt_uses_def;
typedef struct { uint32_t def, to, role, flags, dst_shard, dst_row; } dvt_uses_edge;
typedef struct {
    uint64_t position, cycles, uses_total;
    uint32_t n_nodes, n_defs, n_edges, depth, cut, unexpanded, truncated, live_at_exit, no_value, dead, levels, passes, shard, row, shards_total, span;
    float ms;          /* wall clock of the call after the entry guard */
    uint32_t pad;
} dvt_uses_summary;
int dvt_rv32_job_uses(dvt_prover *p, const dvt_pk *pk, dvt_job *job, uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags,
                      uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes, size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs,
                      dvt_uses_edge *edges, size_t cap_edges, dvt_uses_summary *summary);
/* milliseconds of the last dvt_rv32_job_uses: the next, the count and scan, the emit and the gather launches by events on the
 * members' streams, summed over members, levels and passes; the host's share (the wall clock of the call less those four) */
int dvt_rv32_job_uses_times(dvt_prover *p, double out[5]);
/* The same slice on the host alone (no GPU is touched), the guest run in shards of 2^log_shard_size cycles (0: 21; 4..22).  The
 * records at and after the position are kept, 48 bytes per cycle: past 2^24 of them the call fails with DVT_ERR_UNSUPPORTED
 * (dvt_rv32_job_uses is the way for such executions).  The definitions of a level are answered by one forward scan.  Return codes,
 * *report and *err_text as dvt_execute gives them; the outputs are filled for whatever retired, also when the guest fails. */
int dvt_execute_uses(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint64_t max_cycles, uint32_t log_shard_size,
                     uint32_t shard, uint32_t row, uint32_t what, uint32_t target, uint32_t flags, uint32_t max_depth, uint32_t fan, dvt_uses_node *nodes,
                     size_t cap_nodes, dvt_uses_def *defs, size_t cap_defs, dvt_uses_edge *edges, size_t cap_edges, dvt_uses_summary *summary,
                     dvt_report *report, char **err_text);
/* Divergence of two executions of one guest: where two prepared jobs of one handle (job_a == job_b is allowed) stop doing the
 * same thing, and which values differed before, from the cycle records both jobs hold (the records are only read, the jobs are
 * left as found).  The rule is stated in csrc/diverge.h:
 *   streams     execution X is its records in execution order.  A call names a start in each, (shard, row), at global record
 *               numbers gA and gB; pair k is (A[gA + k], B[gB + k]) for k < N = min(lenA - gA, lenB - gB, max_pairs; 0: no limit).
 *   class       BAD: either record is one the executor never writes.  CONTROL: the two idx differ.  DATA: same idx and at least
 *               one of the words a, b, c, m_prev differs; mask = DVT_DIV_RD | _RS1 | _RS2 | _MEM, one bit per differing word.
 *               The timestamp words of a record (pa_prev, *_ts, sh_*) are NOT compared.  SAME: everything else.
 *   stop        the smallest k whose class is CONTROL (reason DVT_DIV_SPLIT) or BAD (DVT_DIV_BAD); without one stop = N and the
 *               reason is END_BOTH (both streams end at pair N), END_A / END_B (only that stream does) or LIMIT.  Only pairs
 *               k < stop count below.
 *   summary     n_pairs = stop, reason, n_data / first_data / last_data (pair numbers or DVT_DIV_NONE), mask = the OR of the
 *               masks, n_load_diffs (loads whose word before differs), n_store_diffs (stores whose word AFTER differs), the
 *               positions of pair `stop` in A and B (past the end: the last shard and its record count), both records of pair
 *               `stop` and of pair stop - 1 with their pc (valid = 0: there is none), the deciding instruction being pair
 *               stop - 1; launched_pairs (pairs the device classified; 0 on the host path), cycles_a, cycles_b.
 *   regs[r]     r >= 1: n_diff = pairs that write r with a differing a; first_diff, last_diff, last_write (pair numbers);
 *               live = last_write != NONE && last_write == last_diff.  With both starts at the entry the live registers are
 *               exactly the ones that hold different values at the stop; with later starts, relative to the starts.
 *   first/last  the first and the last min(cap_each, n_data) DATA pairs (first: slot r = rank r; last: slot r = rank
 *               n_data - min(cap_each, n_data) + r), cap_each <= DVT_DIVERGE_MAX_KEEP: k, both positions, idx, pc, mask, dir
 *               (DVT_WATCH_LOAD / _STORE or 0), a b c m_prev of both sides and, of a load or store, addr, before, after of both.
 *   rejoin      with flags & DVT_DIVERGE_REJOIN and reason SPLIT: each side is walked from its record of pair `stop` for at most
 *               `window` records (0: DVT_DIVERGE_DEFAULT_WINDOW; at most DVT_DIVERGE_MAX_WINDOW) keeping a relative call depth;
 *               the first pair of records (i of A, j of B) at the same level (the split's frame, or the one record after the
 *               return out of it) with the same idx, smallest i + j, then smallest i: rejoin_* = their positions, rejoin_skip_* =
 *               i, j; DVT_DIVERGE_NO_REJOIN in all six without one.  A heuristic: the call from the rejoin positions confirms it.
 * DVT_ERR_INPUT: null arguments, cap_each or window above the limits, an unknown flag.  A start names the first record at or after
 * it, positions comparing as (shard, row) pairs as the snapshot's do: a start past the end of its execution is its end.
 * DVT_ERR_UNSUPPORTED: a job that does not hold every shard of its execution; a segment of pairs whose two shards are held by
 * different members of the handle (with one member, or with equal starts, there is none). */
#define DVT_DIVERGE_SPAN 4096              /* pairs one workgroup of the device pass classifies */
#define DVT_DIVERGE_MAX_KEEP 64
#define DVT_DIVERGE_MAX_WINDOW 16384
#define DVT_DIVERGE_DEFAULT_WINDOW 4096
#ifndef DVT_DIVERGE_BATCH_PAIRS           /* (a build may set another to measure it: tools/bench_diverge.py) */
#define DVT_DIVERGE_BATCH_PAIRS (1u << 20) /* pairs launched between two reads of the stop flag; a batch holds at least one segment.
                                            * Measured at 2^18, 2^20, 2^22 on 2^21-cycle shards (profiles/README.md, Divergence): the first two are
                                            * the same there, 2^22 costs an early split 0.09 ms more and the whole prefix 0.25 ms less */
#endif
#define DVT_DIV_NONE 0xffffffffffffffffull
#define DVT_DIVERGE_NO_REJOIN 0xffffffffu
enum { DVT_DIV_RD = 1, DVT_DIV_RS1 = 2, DVT_DIV_RS2 = 4, DVT_DIV_MEM = 8 };                                           /* mask */
enum { DVT_DIVERGE_REJOIN = 1 };                                                                                        /* flags of a call */
enum { DVT_DIV_SPLIT = 1, DVT_DIV_BAD = 2, DVT_DIV_END_BOTH = 3, DVT_DIV_END_A = 4, DVT_DIV_END_B = 5, DVT_DIV_LIMIT = 6 };   /* reason */
typedef struct { uint32_t shard, row; } dvt_diverge_pos;
typedef struct { uint32_t valid, pc, idx, a, b, c, m_prev, pad; } dvt_diverge_rec;
typedef struct {
    uint64_t k;
    uint32_t shard_a, row_a, shard_b, row_b, idx, pc, mask, dir;
    uint32_t a_a, b_a, c_a, m_a, a_b, b_b, c_b, m_b;
    uint32_t addr_a, before_a, after_a, addr_b, before_b, after_b;
} dvt_diverge_pair;
typedef struct { uint64_t n_diff, first_diff, last_diff, last_write; uint32_t live, pad; } dvt_diverge_reg;
typedef struct {
    uint64_t n_pairs, n_data, first_data, last_data, n_load_diffs, n_store_diffs, launched_pairs, cycles_a, cycles_b;
    uint32_t reason, mask, stop_shard_a, stop_row_a, stop_shard_b, stop_row_b;
    uint32_t rejoin_shard_a, rejoin_row_a, rejoin_shard_b, rejoin_row_b, rejoin_skip_a, rejoin_skip_b;
    uint32_t n_kept, span, window, batch_pairs;   /* n_kept = min(cap_each, n_data): the filled slots of first[] and of last[]; batch_pairs: DVT_DIVERGE_BATCH_PAIRS as built */
    dvt_diverge_rec stop_a, stop_b, prev_a, prev_b;
    float ms;          /* wall clock of the call after the entry guard */
    uint32_t pad2;
} dvt_diverge_summary;
int dvt_rv32_job_diverge(dvt_prover *p, const dvt_pk *pk, dvt_job *job_a, dvt_job *job_b, dvt_diverge_pos start_a, dvt_diverge_pos start_b,
                         uint64_t max_pairs, uint32_t flags, uint32_t window, size_t cap_each, dvt_diverge_pair *first, dvt_diverge_pair *last,
                         dvt_diverge_reg regs[32], dvt_diverge_summary *summary);
/* milliseconds of the last dvt_rv32_job_diverge: the classify launches, the merge launch, the emit and gather launches (by events
 * on the members' streams, summed over members and batches); the host's share (the wall clock of the call less those three) */
int dvt_rv32_job_diverge_times(dvt_prover *p, double out[4]);
/* The same comparison on the host alone (no GPU is touched): the guest is run twice, on stdin_a and on stdin_b (one buffer each, len 0:
 * none), in shards of 2^log_shard_size cycles (0: 21; 4..22), and the records of both runs from their starts on are kept, 48 bytes
 * per cycle: past 2^24 of them per run the call fails with DVT_ERR_UNSUPPORTED.  A guest that traps or exits non-zero is no
 * error here: its stream ends where it stopped, report_a / report_b (either may be null) say how each run ended, and the call
 * returns DVT_OK. */
int dvt_execute_diverge(const uint8_t *elf, size_t elf_len, const uint8_t *stdin_a, size_t n_a, const uint8_t *stdin_b, size_t n_b, uint64_t max_cycles,
                        uint32_t log_shard_size, dvt_diverge_pos start_a, dvt_diverge_pos start_b, uint64_t max_pairs, uint32_t flags, uint32_t window,
                        size_t cap_each, dvt_diverge_pair *first, dvt_diverge_pair *last, dvt_diverge_reg regs[32], dvt_diverge_summary *summary,
                        dvt_report *report_a, dvt_report *report_b, char **err_text);
/* test hook: run K0 on one shard of a prepared job and return the device-generated main traces
 * (canonical); blob layout as dvt_rv32_debug_traces with prep_width = 0. */
int dvt_rv32_debug_device_traces(dvt_prover *p, const dvt_pk *pk, dvt_job *job, size_t shard, uint32_t **blob,
                                 size_t *blob_words);
/* test hook: make a prepared job dishonest.  Adds the canonical field element `add` (1 .. p-1) to main-trace cell (col, row)
 * of the table of chip `chip` of shard `shard` (global position), on the device member that holds the shard, so that the job
 * check, the job's bus ledger and the prover can be tried on a wrong table.  Like every call on the handle it stops a running
 * prove_shard pipeline first; it returns after the write is complete on the member's stream.  What is written depends on
 * where the job holds the table:
 *  - the chips whose table the job holds as uploaded or as built at upload (mem_image, mem_init, shift, muldiv, the SHA and
 *    the field / curve chips): the cell of that table, in place, in the representation the table has there.  It lasts for
 *    the life of the job.
 *  - byte (1) and program (0): the word of the base multiplicities the job holds, which every K0 copies and adds the cpu
 *    rows' lookups to (plain integers below p there, so the sum is taken mod p).  It lasts for the life of the job; a K0
 *    output kept from phase 1 no longer matches it and is marked invalid, so the next reader of the shard runs K0 again.
 *  - cpu (2): its rows are rebuilt from the cycle records by every K0, and the records are not touched.  The cell of the K0
 *    output kept from phase 1 is written, which is allowed only while the shard holds a valid one (DVT_KEEP_FULL and not yet
 *    consumed by a phase 2); it lasts until the shard's next K0.  Otherwise DVT_ERR_UNSUPPORTED.
 * In every case the shard's header and phase-1 results are marked invalid: the next dvt_rv32_prove_job (or commit_shard) runs
 * phase 1 of that shard again, as a second prove_job of a job does, so no proof combines an honest commitment with the
 * poked table.  Adding p - add to the same cell restores the job.
 * DVT_ERR_INPUT: a null argument, a shard the job does not hold, a chip the shard has no table of, col >= main_w,
 * row >= 2^log_n, add == 0 or add >= p.  One word is written, inside a buffer whose bounds were just checked; no cycle
 * record is read or written. */
int dvt_rv32_debug_poke_cell(dvt_prover *p, dvt_job *job, size_t shard, uint32_t chip, uint32_t col, uint32_t row,
                             uint32_t add);
/* stock `client.verify(&proof,&vk)` semantics (NOT the reference's re-execution
 * `verify` sub-command).  Host-only.  *public_values = the guest's fd-3 byte
 * stream; the proof binds it through the eight COMMITted words of its SHA-256 digest, which the
 * verifier recomputes.  fri_queries / pow_bits are the parameters the CALLER accepts
 * (1..1024 queries, at most 30 bits; anything else is DVT_ERR_INPUT). */
int dvt_verify(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
               uint32_t pow_bits, int32_t *exit_code, uint8_t **public_values, size_t *pv_len, char **reason);
/* dvt_verify on the handle's GPU (member 0, lane 0): same arguments, same return codes, same *reason text, same
 * exit_code / public_values as dvt_verify for EVERY input.  The host runs, per shard, the shape checks, the transcript,
 * the constraint check at zeta, the FRI challenges and the proof-of-work check; the query part of all shards that pass
 * runs on the device, a staging-size chunk of shards at a time, and the first failure in dvt_verify's order (shard,
 * host part before queries, query, step) is reported.  p == NULL is DVT_ERR_INPUT; a HIP failure is DVT_ERR_DEVICE
 * with the text in dvt_last_error (there is no fallback to the host path). */
int dvt_prover_verify(dvt_prover *p, const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len,
                      uint32_t fri_queries, uint32_t pow_bits, int32_t *exit_code, uint8_t **public_values,
                      size_t *pv_len, char **reason);
/* The compact form of a proof.  A shard proof ("DVP1") carries one complete Merkle path per query and tree, and the
 * queries of a shard share most of them; the compact form ("DVP2") carries every query's opened rows and FRI siblings as
 * before, no path, and per tree (the four input trees, then the FRI layers) ONE list `u32 count, count digests` of the
 * nodes the queries cannot compute from each other, in the order of dvt_stage_multipath_nodes ("Proof format").
 * Every verify entry point reads both forms, and a container may mix them; a prover handle writes the compact form with
 * "compact_openings": 1 in its config (default 0: the bytes of every proof as before).
 * dvt_proof_compact / dvt_proof_expand turn a container (rv32 key) or a single machine-level shard proof into the other
 * form.  Host only.  They run the verifier's host part per shard to obtain the query indices (a shard that fails it, or a
 * malformed proof: DVT_ERR_REJECTED with the verifier's text in *reason) and do not check the openings: compact hashes
 * nothing, expand recomputes the dropped siblings from the leaves upward.  For a proof P that verifies,
 * expand(compact(P)) == P byte for byte, and compact(P) equals what the prover writes with "compact_openings": 1.  A
 * proof that is already in the wanted form comes back unchanged.  *out via dvt_free. */
int dvt_proof_compact(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                      uint32_t pow_bits, uint8_t **out, size_t *out_len, char **reason);
int dvt_proof_expand(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                     uint32_t pow_bits, uint8_t **out, size_t *out_len, char **reason);
/* test hook, host only: every word of every node list of every compact shard of a container changed by +1 mod p, one at a
 * time, and the query part of that shard's tree verified again.  The host part of a shard reads no node list (the query
 * indices come from the transcript), so it runs once per shard instead of once per changed word; the container itself
 * must verify (else DVT_ERR_REJECTED with the text).  *n_words: the words changed; *n_accepted: the changes after which the
 * tree was still accepted (0 for a sound verifier).  Plain shards are skipped. */
int dvt_debug_compact_list_sweep(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                                 uint32_t pow_bits, uint64_t *n_words, uint64_t *n_accepted, char **reason);
/* measurement hook: the last dvt_prover_verify / dvt_prover_machine_verify of this handle in milliseconds.  out[0] = the
 * host part (parse, transcript, zeta check), out[1] = flattening into pinned staging, out[2] = uploads, out[3] = kernels,
 * out[4] = downloads (2..4: HIP events, summed over the chunks), out[5] = host time spent waiting for the device,
 * out[6] = Poseidon2 permutations, out[7] = kernel launches, out[8] = chunks. */
int dvt_prover_verify_times(dvt_prover *p, double out[9]);
/* test hook, host only, no device: the admission rule of "keep_phase1" on the caller's figures; returns DVT_KEEP_*.
 *   mode 0: NONE.   mode 1 (and every value other than 0 and 2): FULL if free > reserve, else NONE.
 *   mode 2: FULL if free > reserve + (full - tree) + remaining * later, and (count_known or free > floor(3 total / 4)),
 *           and (full_cap < 0 or full_kept < full_cap); otherwise TREE if free > reserve; otherwise NONE.
 * free: bytes free on the device, the committing lane's cached buffers included; total: the device's bytes; reserve: 24 GB
 * plus the room of the lanes not yet created; full, tree: what this shard keeps in each tier; later: what every later
 * shard takes at least (its tree and what its upload allocates, estimated by this shard's); remaining: the shards the
 * members on this physical device are known to have still to commit in this prepare, after this one; count_known: the
 * executor's fast pass has finished, so `remaining` is exact (outside a prepare: remaining 0, known); full_cap
 * ("keep_full_max") and full_kept: the cap and the count of shards kept in full on the device in this job.  A sum that
 * leaves 64 bits counts as "does not fit". */
int dvt_debug_keep_plan(int mode, uint64_t free_bytes, uint64_t total_bytes, uint64_t reserve_bytes, uint64_t full_bytes,
                        uint64_t tree_bytes, uint64_t later_bytes, uint64_t remaining, int count_known, int64_t full_cap,
                        uint64_t full_kept);
/* measurement hook, host only: guest cycles per second of the executor alone; trace = 0: fast mode (the sequential
 * pass of the prove pipeline), 1: trace mode (48-byte record per cycle).  0.0 when the guest does not halt. */
double dvt_debug_exec_rate(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint32_t log_shard,
                           int trace);
/* test hook, host only: FP64 formulation of Poseidon2 (csrc/poseidon2_f64.cuh, what the hashing kernels run)
 * against the integer permutation on n states; returns the number of differing words (0 = identical) */
uint64_t dvt_debug_p2_f64_selfcheck(uint32_t n, uint32_t seed);
/* test hook, host only: the S-box of that formulation (x^7 with partially reduced x^3 and x^4) against integer arithmetic
 * on n pseudo-random inputs over its whole stated input range and on edge values; returns the number of wrong results.
 * max_abs[4] = the largest |x^2|, |x^3|, |x^4|, |x^7| representatives met, which its exactness conditions bound. */
uint64_t dvt_debug_p2_f64_sbox_check(uint32_t n, uint32_t seed, double *max_abs);
/* test hook, host only: the radix-8 group arithmetic of the K1 register passes (csrc/ntt_group.cuh: stages 0 and 1 reduced
 * only to a multiple of 2^K p) against integer arithmetic mod p, on n pseudo-random groups and on an edge grid of inputs
 * and twiddles; returns the number of outputs that are not integers congruent to the reference.  max_dif[8], max_dif_unit[8]
 * (the variant that skips the products by the twiddle 1) and max_dit[8] = the largest magnitudes met, in the slots that
 * ntg::NoProbe documents: stage 0/1/2 factor and product, value before the last reduction, output. */
uint64_t dvt_debug_ntt_group_check(uint32_t n, uint32_t seed, double *max_dif, double *max_dif_unit, double *max_dit);
/* test hook, host only: the bus ledger's key of a tuple (csrc/ledger_key.h: the function the kernels key the rows with) */
uint64_t dvt_debug_ledger_key(uint64_t seed, uint32_t bus, uint32_t arity, const uint32_t *values);

/* Host side of the reference's prove()/execute() above the prover call: the typed JSON input of
 * `--type` (bad-share | finalization | bad-partial-key | bad-encrypted-share; crates/dkg/src/types.rs:26-203)
 * -> serde_cbor::to_vec(data) (src/main.rs:435,459) -> the one SP1Stdin buffer (`stdin.write(&bin)`,
 * :437,:460: u64-LE length + CBOR bytes).  auth_commitment != 0 adds the fields of the reference's
 * cargo feature of that name.  Host-only; *out via dvt_free. */
int dvt_stdin_from_json(const char *type, const char *json, size_t json_len, int auth_commitment, uint8_t **out,
                        size_t *out_len, char **err_text);
/* `--json-schema-file` of the reference's CLI (src/main.rs:509-541: JSONSchema::compile + validate): checks
 * `json` against the draft-07 `schema` (the keyword subset of the schema files under the reference's spec/json/: type, $ref
 * into #/definitions, required, properties, items, minLength, maxLength, pattern, minimum, maximum).
 * DVT_OK, or DVT_ERR_INPUT with one violation per line in *err_text (dvt_free).  Host-only. */
int dvt_json_schema_validate(const char *schema, size_t schema_len, const char *json, size_t json_len, char **err_text);

/* test hook, host-only: the traces (canonical, column-major) the prover would commit for shard
 * `shard` (0-based position) of this run cut at 2^log_shard cycles (0 = default 21).  Layout of *blob
 * (u32 words): n_chips present, then per chip {chip_id, log_n, main_width, prep_width}, then n_pub,
 * pubs..., then per chip the main words followed by the preprocessed words. */
int dvt_rv32_debug_traces(const uint8_t *elf, size_t elf_len, const dvt_buf *stdin_bufs, size_t nbuf, uint32_t log_shard,
                          uint32_t shard, uint32_t *n_shards, uint32_t **blob, size_t *blob_words, char **err_text);

#ifdef __cplusplus
}
#endif
#endif
