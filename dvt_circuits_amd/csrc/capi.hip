// C-ABI layer (include/dvt_prover.h) over the gfx950 engine: the handle and its config, the entry guard and the error path,
// the stage entry points of the prover's kernels and the machine-level ones (the rv32 boundary is capi_rv32.hip, the
// inspectors of trace rows capi_inspect.hip, the reports over cycle records capi_report.hip).  There is no CPU fallback anywhere in this layer: without a HIP device every
// entry point that computes returns DVT_ERR_DEVICE.  (dvt_machine_verify is host-only by nature.)
#include <algorithm>
#include <cstdarg>
#include <cstdio>

#include <chrono>

#include "capi_internal.h"
#include "verify_query.h"

using namespace dvt;

namespace dvt {
static thread_local std::string g_create_err;

// the ABI layer's one formatter
static int vfail(std::string &err, int code, const char *fmt, va_list ap) {
    char buf[600];
    vsnprintf(buf, sizeof buf, fmt, ap);
    err = buf;
    return code;
}
int fail(std::string &err, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(err, code, fmt, ap);
    va_end(ap);
    return code;
}
int fail(dvt_prover *p, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfail(p ? p->err : g_create_err, code, fmt, ap);
    va_end(ap);
    return code;
}

hipError_t sync_lanes(Member &mem) {
    hipError_t first = hipStreamSynchronize(mem.eng.stream);
    for (auto &e : mem.more)
        if (e) { const hipError_t r = hipStreamSynchronize(e->stream); if (first == hipSuccess) first = r; }
    return first;
}

int pipe_drain(Member &mem, std::string *first_err) {
    if (!mem.pipe) return DVT_OK;
    Phase2Pipe &pp = *mem.pipe;
    {
        std::lock_guard<std::mutex> lk(pp.mu);
        pp.stop = true;
        pp.cv.notify_all();
    }
    for (auto &t : pp.workers) t.join();
    int rc = DVT_OK;
    for (auto &s : pp.slots)
        if (s.state == 2 && s.rc && !s.claimed) {
            rc = s.rc;
            if (first_err) *first_err = s.err;
            break;
        }
    (void)sync_lanes(mem);
    mem.pipe.reset();
    return rc;
}

void pipe_drain_all(dvt_prover *p) {
    for (size_t m = n_members(p); m-- > 0;) {
        Member &mem = member(p, m);
        if (!mem.pipe) continue;
        if (m) (void)hipSetDevice(mem.eng.device);   // (the streams a drain waits for are that device's)
        (void)pipe_drain(mem);
        if (m) (void)hipSetDevice(eng0(p).device);
    }
}

int select_member(dvt_prover *p, size_t m) {
    const hipError_t e = hipSetDevice(member(p, m).eng.device);
    return e == hipSuccess ? DVT_OK : fail(p, DVT_ERR_DEVICE, "hipSetDevice(%d): %s", member(p, m).eng.device, hipGetErrorString(e));
}

Guard::Guard(dvt_prover *p, const PipeClaim *claim, size_t claim_member) : p(p), lk(p->mu) {
    if (claim && member(p, claim_member).pipe) slot = member(p, claim_member).pipe->slot_of(*claim);
    if (slot < 0) pipe_drain_all(p);
    rc = select_member(p, 0);
}

// ---- the handle's config: a flat JSON object of integers, and one list of integers ("devices")

static int cfg_int(const char *json, const char *key, int dflt) {
    if (!json) return dflt;
    std::string pat = std::string("\"") + key + "\"";
    const char *s = strstr(json, pat.c_str());
    if (!s) return dflt;
    s = strchr(s + pat.size(), ':');
    if (!s) return dflt;
    return atoi(s + 1);
}

// the position after `"key" :` in json, or nullptr.  Like cfg_int it looks for the quoted text anywhere in the string and
// takes what follows the next ':' without checking that the match is a key: enough for the flat cfg object, no JSON parser.
static const char *cfg_value(const char *json, const char *key) {
    if (!json) return nullptr;
    const std::string pat = std::string("\"") + key + "\"";
    const char *s = strstr(json, pat.c_str());
    if (!s) return nullptr;
    s = strchr(s + pat.size(), ':');
    return s ? s + 1 : nullptr;
}
// A list of decimal integers: `[a, b, ...]` (json = true) or `a,b,...` up to the end of the string.  False on anything else
// (an entry that is not an integer, a missing bracket or comma).
static bool parse_int_list(const char *s, bool json, std::vector<long> *out) {
    auto blank = [&] { while (*s == ' ' || *s == '\t' || *s == '\n' || *s == '\r') s++; };
    blank();
    if (json && *s++ != '[') return false;
    blank();
    if (json ? *s == ']' : !*s) return true;   // empty
    for (;;) {
        blank();
        char *end = nullptr;
        const long v = strtol(s, &end, 10);
        if (end == s) return false;
        s = end;
        out->push_back(v);
        blank();
        if (json ? *s == ']' : !*s) return true;
        if (*s++ != ',') return false;
    }
}
// The device list of a handle: the cfg key "devices", else the environment variable DVT_DEVICES, else the key "device".
static int cfg_devices(const char *json, int ndev, std::vector<int> *out) {
    std::vector<long> list;
    const char *from = nullptr;
    const char *env = getenv("DVT_DEVICES");
    if (const char *v = cfg_value(json, "devices")) {
        from = "\"devices\"";
        if (cfg_value(json, "device")) return fail(nullptr, DVT_ERR_INPUT, "give \"device\" or \"devices\", not both");
        if (!parse_int_list(v, true, &list)) return fail(nullptr, DVT_ERR_INPUT, "\"devices\" must be a list of integers");
    } else if (env && *env) {
        from = "DVT_DEVICES";
        if (!parse_int_list(env, false, &list)) return fail(nullptr, DVT_ERR_INPUT, "DVT_DEVICES must be a comma-separated list of integers");
    } else {
        from = "\"device\"";
        list.push_back(cfg_int(json, "device", 0));
    }
    if (list.empty() || list.size() > (size_t)MAX_MEMBERS) return fail(nullptr, DVT_ERR_INPUT, "%s must name 1..%d devices (got %zu)", from, MAX_MEMBERS, list.size());
    for (long d : list) {
        if (d < 0 || d >= ndev) return fail(nullptr, DVT_ERR_INPUT, "%s: device %ld out of range (%d present)", from, d, ndev);
        out->push_back((int)d);
    }
    return DVT_OK;
}

const MachineDesc *machine_by_name(const char *name) {
    if (!name) return nullptr;
    if (!strcmp(name, "toy")) return machine_toy();
    if (!strcmp(name, "rv32")) return machine_rv32();
    return nullptr;
}

void pk_release(dvt_prover *p, dvt_pk *pk) {
    // (a key is freed on the handle that made it, include/dvt_prover.h; on another one the copies it cannot reach are skipped)
    for (size_t m = std::min(pk->dev.size(), n_members(p)); m-- > 0;) {   // in reverse: member 0's device stays current
        DeviceKey &k = pk->dev[m];
        (void)hipSetDevice(member(p, m).eng.device);
        member(p, m).eng.free_key(&k.key);
        if (k.d_instrs) (void)hipFree(k.d_instrs);
        if (k.d_prog_row) (void)hipFree(k.d_prog_row);
    }
    delete pk;
}
int setup_finish(dvt_prover *p, dvt_pk *pk, int rc, dvt_pk **pk_out, uint8_t **vk, size_t *vk_len) {
    if (!rc && vk && vk_len && !(*vk = copy_out(vk_words(pk->dev[0].key.vk), vk_len))) rc = fail(p, DVT_ERR_DEVICE, "out of host memory");
    if (rc) pk_release(p, pk);
    else *pk_out = pk;
    return rc;
}

std::vector<uint32_t> vk_words(const VerifyingKey &vk) {
    WordWriter w;
    w.u32(0x314b5644u);  // "DVK1"
    char name[16] = {0};
    strncpy(name, vk.machine->name, 15);
    for (int i = 0; i < 4; i++) { uint32_t v; memcpy(&v, name + 4 * i, 4); w.u32(v); }
    w.dg(vk.prep_root);
    w.u32((uint32_t)vk.prep_chips.size());
    for (auto &c : vk.prep_chips) { w.u32((uint32_t)c.chip_id); w.u32(c.log_n); }
    w.u32((uint32_t)vk.extra.size());
    for (auto x : vk.extra) w.u32(x);
    return w.w;
}
bool vk_parse(const uint8_t *b, size_t len, VerifyingKey *vk) {
    if (len % 4 || len < 4 * 15) return false;
    std::vector<uint32_t> wv(len / 4);
    memcpy(wv.data(), b, len);
    try {
        WordReader r(wv.data(), wv.size());
        if (r.u32() != 0x314b5644u) return false;
        char name[17] = {0};
        for (int i = 0; i < 4; i++) { uint32_t v = r.u32(); memcpy(name + 4 * i, &v, 4); }
        vk->machine = machine_by_name(name);
        if (!vk->machine) return false;
        for (size_t i = strlen(name); i < 16; i++)
            if (name[i]) return false;   // one encoding per key: the padding after the machine name is zero
        vk->prep_root = r.dg();
        uint32_t n = r.len(64);
        for (uint32_t i = 0; i < n; i++) {
            ChipRef c;
            c.chip_id = (int)r.u32();
            c.log_n = r.u32();
            if (c.chip_id < 0 || c.chip_id >= vk->machine->n_chips || c.log_n > 22) return false;
            vk->prep_chips.push_back(c);
        }
        uint32_t ne = r.len(16);
        for (uint32_t i = 0; i < ne; i++) vk->extra.push_back(r.u32());
        if (r.p != r.end) return false;
    } catch (const std::exception &) { return false; }
    return true;
}

int verify_words(const uint8_t *proof, size_t len, int len_code, char **reason,
                 const std::function<int(WordReader &, std::string &)> &check) {
    if (len % 4) return reject(reason, len_code, "proof length is not a multiple of 4");
    std::vector<uint32_t> words(len / 4);
    memcpy(words.data(), proof, len);
    std::string why;
    int rc = DVT_ERR_REJECTED;   // (what a malformed proof that throws gets)
    try {
        WordReader r(words.data(), words.size());
        rc = check(r, why);
    } catch (const std::exception &e) { why = e.what(); }
    return rc ? reject(reason, rc, why) : DVT_OK;
}


// ---- K4 / K5 of one chip: the argument checks both entries share (ChipStageArgs, capi_internal.h)
int chip_stage_args(dvt_prover *p, const char *machine, uint32_t chip, uint32_t log_n, const uint32_t *pub, const uint32_t perm_alpha[4],
                    const uint32_t beta[4], uint32_t path, ChipStageArgs *out) {
    const MachineDesc *m = machine_by_name(machine);
    if (!m) return fail(p, DVT_ERR_INPUT, "unknown machine '%s'", machine ? machine : "(null)");
    if (chip >= (uint32_t)m->n_chips) return fail(p, DVT_ERR_INPUT, "chip %u out of range (%d chips)", chip, m->n_chips);
    out->m = m;
    out->d = &m->chips[chip];
    challenge_power_counts(m, &out->n_beta, &out->n_alpha);
    if (log_n > 22) return fail(p, DVT_ERR_INPUT, "log_n %u > 22", log_n);
    if (path > DVT_PATH_PARTS) return fail(p, DVT_ERR_INPUT, "path %u", path);
    if (path == DVT_PATH_PARTS && log_n > PARTS_PARALLEL_LOG)
        return fail(p, DVT_ERR_INPUT, "the part-parallel launches take at most 2^%u rows", PARTS_PARALLEL_LOG);
    if (!perm_alpha || !beta || (out->d->n_pub && !pub)) return fail(p, DVT_ERR_INPUT, "null argument");
    if (!ext_from_canonical(perm_alpha, &out->perm_alpha) || !ext_from_canonical(beta, &out->beta))
        return fail(p, DVT_ERR_INPUT, "perm_alpha or beta not canonical");
    out->pub.assign(std::max(out->d->n_pub, 1), 0);
    for (int k = 0; k < out->d->n_pub; k++) {
        if (pub[k] >= P) return fail(p, DVT_ERR_INPUT, "public value %d not canonical", k);
        out->pub[k] = Fp::from_canonical(pub[k]).v;
    }
    return DVT_OK;
}
int stage_table(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                const uint32_t *pub, ChipStageArgs *out, const uint32_t *perm_alpha, const uint32_t *beta) {
    if (int rc = chip_stage_args(p, machine, chip, log_n, pub, perm_alpha, beta, DVT_PATH_DEFAULT, out)) return rc;
    if (!d_main || (out->d->prep_w && !d_prep)) return fail(p, DVT_ERR_INPUT, "null matrix");
    out->t = {out->d, d_main, out->d->prep_w ? d_prep : nullptr, log_n};
    return DVT_OK;
}
}  // namespace dvt

extern "C" {

uint32_t dvt_abi_version(void) { return 21; }

int dvt_prover_create(const char *cfg_json, dvt_prover **out) {
    if (!out) return fail(nullptr, DVT_ERR_INPUT, "out == NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, DVT_ERR_DEVICE, "no HIP device (%s); this library has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    std::vector<int> devs;
    if (int rc = cfg_devices(cfg_json, ndev, &devs)) return rc;
    for (int d : devs) {
        hipDeviceProp_t prop;
        HIP_TRY(nullptr, hipGetDeviceProperties(&prop, d));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
            return fail(nullptr, DVT_ERR_DEVICE, "device %d is %s; this library is built for gfx950 only", d, prop.gcnArchName);
    }
    std::unique_ptr<dvt_prover> p(new dvt_prover());   // (freed on the early returns)
    p->cfg.num_queries = (uint32_t)cfg_int(cfg_json, "fri_queries", 100);
    p->cfg.pow_bits = (uint32_t)cfg_int(cfg_json, "pow_bits", 16);
    p->cfg.compact_openings = cfg_int(cfg_json, "compact_openings", 0) != 0;
    const bool profile = cfg_int(cfg_json, "profile", 0) != 0;
    p->log_shard = (uint32_t)cfg_int(cfg_json, "log_shard_size", 21);
    {   // (0 and 2 are modes of their own; every other value reads as 1, as it did when the key was a flag)
        const int keep = cfg_int(cfg_json, "keep_phase1", 1);
        p->keep_phase1 = keep == 0 || keep == 2 ? keep : 1;
    }
    p->keep_full_max = cfg_int(cfg_json, "keep_full_max", -1);
    p->exec_threads = (uint32_t)std::max(0, cfg_int(cfg_json, "exec_threads", 0));
    const int parts_parallel_log = cfg_int(cfg_json, "parts_parallel_log", (int)PARTS_PARALLEL_LOG);
    if (parts_parallel_log < -1 || parts_parallel_log > (int)PARTS_PARALLEL_LOG)
        return fail(nullptr, DVT_ERR_INPUT, "parts_parallel_log must be -1..%u", PARTS_PARALLEL_LOG);
    const int verify_chunk_words = cfg_int(cfg_json, "verify_chunk_words", (int)vq::CHUNK_WORDS);
    if (verify_chunk_words <= 0) return fail(nullptr, DVT_ERR_INPUT, "verify_chunk_words must be positive");
    p->vq_chunk_words = (size_t)verify_chunk_words;
    {
        // phase-2 lanes (of every member): the config key, else DVT_LANES (same-process A/B measurements), else 2, which
        // measured best with one member and with two members on one device (profiles/README.md, round 5); profile mode
        // times stages with events on one stream and keeps one lane
        const char *env = getenv("DVT_LANES");
        const int dflt = env && *env ? atoi(env) : 2;
        const int lanes = cfg_int(cfg_json, "lanes", dflt);
        if (lanes < 1 || lanes > MAX_LANES) return fail(nullptr, DVT_ERR_INPUT, "lanes must be 1..%d (got %d)", MAX_LANES, lanes);
        p->lanes = profile ? 1 : lanes;
        // phase-1 lanes: the config key, else DVT_PHASE1_LANES (capped at the handle's lanes, so that one setting serves
        // handles of any lane count in an A/B run), else PHASE1_LANES_DEFAULT
        const char *env1 = getenv("DVT_PHASE1_LANES");
        const int dflt1 = std::min(p->lanes, env1 && *env1 ? atoi(env1) : PHASE1_LANES_DEFAULT);
        p->phase1_lanes = profile ? 1 : cfg_int(cfg_json, "phase1_lanes", dflt1);
        if (p->phase1_lanes < 1 || p->phase1_lanes > p->lanes)
            return fail(nullptr, DVT_ERR_INPUT, "phase1_lanes must be 1..lanes = 1..%d (got %d)", p->lanes, p->phase1_lanes);
    }
    if (p->log_shard < 4 || p->log_shard > 22) return fail(nullptr, DVT_ERR_INPUT, "log_shard_size must be 4..22");
    if (p->cfg.num_queries == 0 || p->cfg.num_queries > 1024 || p->cfg.pow_bits > 30)
        return fail(nullptr, DVT_ERR_INPUT, "fri_queries must be 1..1024 and pow_bits <= 30");
    HIP_TRY(nullptr, hipSetDevice(devs[0]));
    for (size_t m = 0; m < devs.size() && e == hipSuccess; m++) {
        p->members.emplace_back(new Member());   // (the destroy below takes care of a half-made member)
        Member &mem = *p->members.back();
        mem.index = m;
        mem.eng.device = devs[m];
        mem.eng.profile = profile;
        mem.eng.parts_parallel_log = parts_parallel_log;
        mem.shares_device = std::count(devs.begin(), devs.end(), devs[m]) > 1;
        e = mem.eng.init(devs[m]);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&mem.copy_stream, hipStreamNonBlocking);
    }
    if (e != hipSuccess) {
        fail(nullptr, DVT_ERR_DEVICE, "handle setup: %s", hipGetErrorString(e));
        dvt_prover_destroy(p.release());
        return DVT_ERR_DEVICE;
    }
    (void)hipSetDevice(devs[0]);
    *out = p.release();
    return DVT_OK;
}

void dvt_prover_destroy(dvt_prover *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        pipe_drain_all(p);
    }
    for (size_t m = n_members(p); m-- > 0;) {   // in reverse, each with its device current
        Member &mem = member(p, m);
        (void)hipSetDevice(mem.eng.device);
        if (mem.copy_stream) { (void)hipStreamSynchronize(mem.copy_stream); (void)hipStreamDestroy(mem.copy_stream); }
        if (mem.aux_pinned) (void)hipHostFree(mem.aux_pinned);
        if (m == 0) {   // (what the handle keeps, before the engine of the device it was made on goes)
            for (auto b : p->pinned) (void)hipHostFree(b);
            vq::stage_free(p->vq_stage);
        }
        for (auto &e : mem.more)
            if (e) e->shutdown();
        mem.eng.shutdown();
    }
    delete p;
}

const char *dvt_last_error(const dvt_prover *p) { return p ? p->err.c_str() : g_create_err.c_str(); }
void dvt_free(void *ptr) { free(ptr); }
void *dvt_stream(dvt_prover *p) { return p ? (void *)eng0(p).stream : nullptr; }

int dvt_sync(dvt_prover *p) {
    if (!p) return DVT_ERR_INPUT;
    Guard g(p); if (g.rc) return g.rc;
    for (size_t m = n_members(p); m-- > 0;) {   // (the guard has drained the lanes; member 0 last, its device stays current)
        if (int rc = select_member(p, m)) return rc;
        HIP_TRY(p, hipStreamSynchronize(member(p, m).eng.stream));
    }
    return DVT_OK;
}

uint32_t dvt_prover_device_count(const dvt_prover *p) { return p ? (uint32_t)n_members(p) : 0; }
int dvt_prover_device(const dvt_prover *p, uint32_t m) {
    return p && m < n_members(p) ? p->members[m]->eng.device : -1;
}

int dvt_dev_to_internal(dvt_prover *p, uint32_t *d, size_t n) {
    if (!p || (!d && n)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    HIP_TRY(p, launch_to_internal(eng0(p).stream, d, n));
    return DVT_OK;
}
int dvt_dev_from_internal(dvt_prover *p, uint32_t *d, size_t n) {
    if (!p || (!d && n)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    HIP_TRY(p, launch_from_internal(eng0(p).stream, d, n));
    return DVT_OK;
}

int dvt_stage_coset_lde(dvt_prover *p, uint32_t *d_in, uint32_t *d_scratch, uint32_t *d_out, uint32_t width, uint32_t log_n,
                        uint32_t shift_mode) {
    if (!p) return DVT_ERR_INPUT;
    if (width && (!d_in || !d_out)) return fail(p, DVT_ERR_INPUT, "null matrix");
    if (log_n > 22) return fail(p, DVT_ERR_INPUT, "log_n %u > 22", log_n);
    if (shift_mode > 2) return fail(p, DVT_ERR_INPUT, "shift_mode %u", shift_mode);
    Guard g(p); if (g.rc) return g.rc;
    HIP_TRY(p, launch_coset_lde(eng0(p).stream, eng0(p).tabs, d_in, d_scratch, d_out, width, log_n, shift_mode));
    return DVT_OK;
}

size_t dvt_merkle_digest_words(const dvt_dev_matrix *mats, size_t n) {
    uint32_t mx = 0;
    for (size_t i = 0; i < n; i++) mx = std::max(mx, mats[i].log_height);
    return (((size_t)2 << mx) - 1) * 8;
}

int dvt_stage_merkle_commit(dvt_prover *p, const dvt_dev_matrix *mats, size_t n, uint32_t *d_digests) {
    if (!p) return DVT_ERR_INPUT;
    if (!mats || !n || !d_digests) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    std::vector<Engine::DevMat> dm;
    for (size_t i = 0; i < n; i++) {
        if (mats[i].log_height >= MERKLE_MAX_SEGMENTS)
            return fail(p, DVT_ERR_INPUT, "tree too tall: matrix %zu has log_height %u, at most %u", i, mats[i].log_height, MERKLE_MAX_SEGMENTS - 1);
        // (commit_tree skips a matrix without columns, where the tree's definition hashes the empty row)
        if (!mats[i].width) return fail(p, DVT_ERR_INPUT, "matrix %zu has width 0", i);
        if (!mats[i].d_data) return fail(p, DVT_ERR_INPUT, "null matrix data");
        dm.push_back({mats[i].d_data, mats[i].width, mats[i].log_height});
    }
    if (!eng0(p).commit_tree(dm, d_digests)) return engine_fail(p->err, eng0(p));
    return DVT_OK;
}

int dvt_stage_poseidon2_permute(dvt_prover *p, uint32_t *d_states, size_t n) {
    if (!p || (!d_states && n)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    HIP_TRY(p, launch_poseidon2_permute(eng0(p).stream, d_states, n));
    return DVT_OK;
}

int dvt_stage_fri_fold(dvt_prover *p, const uint32_t *d_v, uint32_t *d_out, const uint32_t *d_ro, const uint32_t beta[4],
                       uint32_t log_m) {
    if (!p || !d_v || !d_out || !beta) return fail(p, DVT_ERR_INPUT, "null argument");
    if (log_m < 1 || log_m > 23) return fail(p, DVT_ERR_INPUT, "log_m out of range");
    Fp4 b;
    if (!ext_from_canonical(beta, &b)) return fail(p, DVT_ERR_INPUT, "beta not canonical");
    Guard g(p); if (g.rc) return g.rc;
    HIP_TRY(p, launch_fri_fold(eng0(p).stream, eng0(p).tabs, reinterpret_cast<const Fp4 *>(d_v), reinterpret_cast<Fp4 *>(d_out),
                               reinterpret_cast<const Fp4 *>(d_ro), b, log_m));
    return DVT_OK;
}

static bool overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}
static bool overlap(const void *a, const void *b, size_t bytes) { return overlap(a, bytes, b, bytes); }
constexpr size_t STAGE_MAX_COLS = 1u << 16;   // column pointers and alpha powers of one call go through the 16 MB upload ring

int dvt_stage_logup_running_sum(dvt_prover *p, uint32_t *d_totals, uint32_t *d_phi, uint32_t log_n, uint32_t cum[4]) {
    if (!p || !d_totals || !d_phi || !cum) return fail(p, DVT_ERR_INPUT, "null argument");
    if (log_n > 22) return fail(p, DVT_ERR_INPUT, "log_n %u > 22", log_n);
    const size_t n = (size_t)1 << log_n;
    if (overlap(d_totals, d_phi, 16 * n)) return fail(p, DVT_ERR_INPUT, "totals and phi overlap");
    Guard g(p); if (g.rc) return g.rc;
    StageBuf scratch{eng0(p).pool}, d_cum{eng0(p).pool};
    HIP_TRY(p, eng0(p).pool.alloc_bytes(&scratch.ptr, prefix_sum_scratch_words(4, n) * 4));
    HIP_TRY(p, eng0(p).pool.alloc_bytes(&d_cum.ptr, 16));
    uint32_t w[4];
    if (!eng0(p).logup_running_sum(d_totals, static_cast<uint32_t *>(scratch.ptr), d_phi, log_n, static_cast<uint32_t *>(d_cum.ptr)) ||
        !eng0(p).download(w, d_cum.ptr, sizeof w))
        return engine_fail(p->err, eng0(p));
    for (int k = 0; k < 4; k++) cum[k] = Fp::raw(w[k]).canonical();
    return DVT_OK;
}

int dvt_stage_open(dvt_prover *p, const dvt_dev_matrix *mats, size_t n, const uint32_t z[4], uint32_t *out) {
    if (!p || !mats || !n || !z || !out) return fail(p, DVT_ERR_INPUT, "null argument");
    const uint32_t log_n = mats[0].log_height;
    if (log_n > 22) return fail(p, DVT_ERR_INPUT, "log_height %u > 22", log_n);
    std::vector<uint64_t> ptrs;
    for (size_t i = 0; i < n; i++) {
        if (mats[i].log_height != log_n) return fail(p, DVT_ERR_INPUT, "matrices of different heights");
        if (mats[i].width && !mats[i].d_data) return fail(p, DVT_ERR_INPUT, "null matrix data");
        if (ptrs.size() + mats[i].width > STAGE_MAX_COLS) return fail(p, DVT_ERR_INPUT, "more than %zu columns", STAGE_MAX_COLS);
        for (uint32_t c = 0; c < mats[i].width; c++) ptrs.push_back((uint64_t)(uintptr_t)(mats[i].d_data + ((size_t)c << log_n)));
    }
    Fp4 zz;
    if (!ext_from_canonical(z, &zz)) return fail(p, DVT_ERR_INPUT, "z not canonical");
    const uint32_t width = (uint32_t)ptrs.size();
    if (!width) return DVT_OK;
    Guard g(p); if (g.rc) return g.rc;
    Engine &e = eng0(p);
    StageBuf w{e.pool}, partial{e.pool}, res{e.pool};
    HIP_TRY(p, e.pool.alloc_bytes(&w.ptr, sizeof(Fp4) << log_n));
    HIP_TRY(p, e.pool.alloc_bytes(&partial.ptr, sizeof(Fp4) * open_row_blocks(log_n) * width * 2));
    HIP_TRY(p, e.pool.alloc_bytes(&res.ptr, sizeof(Fp4) * width * 2));
    auto d_cols = reinterpret_cast<const uint32_t *const *>(e.upload(ptrs.data(), ptrs.size() * 8));
    Fp4 scale;
    if (!d_cols || !e.open_point(zz, log_n, static_cast<Fp4 *>(w.ptr), &scale)) return engine_fail(p->err, e);
    HIP_TRY(p, launch_open_columns(e.stream, d_cols, width, log_n, static_cast<Fp4 *>(w.ptr), static_cast<Fp4 *>(partial.ptr),
                                   static_cast<Fp4 *>(res.ptr)));
    std::vector<Fp4> h(2 * (size_t)width);
    if (!e.download(h.data(), res.ptr, h.size() * sizeof(Fp4))) return engine_fail(p->err, e);
    for (size_t i = 0; i < h.size(); i++) {
        const Fp4 v = h[i] * scale;
        for (int k = 0; k < 4; k++) out[4 * i + k] = v.c[k].canonical();
    }
    return DVT_OK;
}

int dvt_stage_reduced_opening(dvt_prover *p, const uint32_t *const *cols, uint32_t n_two, uint32_t n_all, uint32_t log_m,
                              const uint32_t alpha[4], const uint32_t *open_local, const uint32_t *open_next, const uint32_t zeta[4],
                              uint32_t *d_out) {
    if (!p || !cols || !alpha || !open_local || (n_two && !open_next) || !zeta || !d_out) return fail(p, DVT_ERR_INPUT, "null argument");
    if (log_m < 1 || log_m > 23) return fail(p, DVT_ERR_INPUT, "log_m out of range");
    if (n_all < 1 || n_all > STAGE_MAX_COLS || n_two > n_all) return fail(p, DVT_ERR_INPUT, "n_two %u / n_all %u out of range", n_two, n_all);
    Fp4 al, ze;
    if (!ext_from_canonical(alpha, &al) || !ext_from_canonical(zeta, &ze)) return fail(p, DVT_ERR_INPUT, "alpha or zeta not canonical");
    std::vector<uint64_t> ptrs(n_all);
    std::vector<Fp4> local(n_all), next(n_two);
    for (uint32_t c = 0; c < n_all; c++) {
        if (!cols[c]) return fail(p, DVT_ERR_INPUT, "null column %u", c);
        ptrs[c] = (uint64_t)(uintptr_t)cols[c];
        if (!ext_from_canonical(open_local + 4 * (size_t)c, &local[c]) || (c < n_two && !ext_from_canonical(open_next + 4 * (size_t)c, &next[c])))
            return fail(p, DVT_ERR_INPUT, "opened value of column %u not canonical", c);
    }
    Guard g(p); if (g.rc) return g.rc;
    Engine &e = eng0(p);
    std::vector<Fp4> apow;
    std::vector<double> apow_d;
    fri_alpha_powers(al, n_all, &apow, &apow_d);
    auto d_apow = reinterpret_cast<const double *>(e.upload(apow_d.data(), apow_d.size() * sizeof(double)));
    auto d_cols = reinterpret_cast<const uint32_t *const *>(d_apow ? e.upload(ptrs.data(), ptrs.size() * 8) : nullptr);
    if (!d_cols || !e.reduced_opening(d_cols, n_two, n_all, log_m, apow, d_apow, local.data(), next.data(), ze, reinterpret_cast<Fp4 *>(d_out)))
        return engine_fail(p->err, e);
    return DVT_OK;
}

int dvt_stage_pow_grind(dvt_prover *p, const uint32_t state[16], uint32_t pos, uint32_t bits, uint32_t *witness) {
    if (!p || !state || !witness) return fail(p, DVT_ERR_INPUT, "null argument");
    if (pos >= 8) return fail(p, DVT_ERR_INPUT, "pos %u >= 8", pos);
    if (bits > 30) return fail(p, DVT_ERR_INPUT, "bits %u > 30", bits);
    uint32_t st16[16];
    for (int k = 0; k < 16; k++) {
        if (state[k] >= P) return fail(p, DVT_ERR_INPUT, "state not canonical");
        st16[k] = Fp::from_canonical(state[k]).v;
    }
    Guard g(p); if (g.rc) return g.rc;
    StageBuf found{eng0(p).pool};
    HIP_TRY(p, eng0(p).pool.alloc_bytes(&found.ptr, 4));
    if (!eng0(p).pow_grind(st16, pos, bits, static_cast<uint32_t *>(found.ptr), witness)) return engine_fail(p->err, eng0(p));
    return DVT_OK;
}

// the part-parallel scratch of a K4 / K5 call, or nullptr (the per-row / per-part launches); words per row of the scratch
static int chip_stage_parts(dvt_prover *p, uint32_t path, bool has_parts, uint32_t log_n, size_t words_per_row, StageBuf *buf,
                            uint32_t **d_parts) {
    *d_parts = nullptr;
    if (path == DVT_PATH_PARTS && !has_parts) return fail(p, DVT_ERR_INPUT, "this chip has no part-parallel launch");
    const bool parts = path == DVT_PATH_PARTS || (path == DVT_PATH_DEFAULT && (int)log_n <= eng0(p).parts_parallel_log);
    if (!parts || !has_parts) return DVT_OK;
    HIP_TRY(p, eng0(p).pool.alloc_bytes(&buf->ptr, (size_t)PARTS_MAX * words_per_row * 4 << log_n));
    *d_parts = static_cast<uint32_t *>(buf->ptr);
    return DVT_OK;
}

int dvt_stage_perm(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main, const uint32_t *d_prep, uint32_t log_n,
                   const uint32_t *pub, const uint32_t perm_alpha[4], const uint32_t beta[4], uint32_t path, uint32_t *d_perm,
                   uint32_t cum[4]) {
    if (!p) return DVT_ERR_INPUT;
    ChipStageArgs a;
    if (int rc = chip_stage_args(p, machine, chip, log_n, pub, perm_alpha, beta, path, &a)) return rc;
    const ChipDesc &d = *a.d;
    const size_t n = (size_t)1 << log_n, perm_bytes = 16 * (size_t)d.perm_ext_w * n;
    if (!d_main || (d.prep_w && !d_prep) || (d.perm_ext_w && !d_perm) || !cum) return fail(p, DVT_ERR_INPUT, "null argument");
    if (d.perm_ext_w && (overlap(d_perm, perm_bytes, d_main, 4 * d.main_w * n) || (d.prep_w && overlap(d_perm, perm_bytes, d_prep, 4 * d.prep_w * n))))
        return fail(p, DVT_ERR_INPUT, "perm overlaps main or prep");
    Guard g(p); if (g.rc) return g.rc;
    Engine &e = eng0(p);
    StageBuf parts{e.pool}, totals{e.pool}, scan{e.pool}, d_cum{e.pool};
    uint32_t *d_parts;
    if (int rc = chip_stage_parts(p, path, d.perm_parts, log_n, 4, &parts, &d_parts)) return rc;
    if (!d.perm_ext_w) {   // no interactions: no permutation trace, cumulative sum 0
        for (int k = 0; k < 4; k++) cum[k] = 0;
        return DVT_OK;
    }
    HIP_TRY(p, e.pool.alloc_bytes(&totals.ptr, 16 * n));
    HIP_TRY(p, e.pool.alloc_bytes(&scan.ptr, prefix_sum_scratch_words(4, n) * 4));
    HIP_TRY(p, e.pool.alloc_bytes(&d_cum.ptr, 16));
    Engine::ChipInputs in{d_main, d.prep_w ? d_prep : nullptr, nullptr, log_n, a.perm_alpha, nullptr, nullptr};
    in.pub = static_cast<const uint32_t *>(e.upload_vec(a.pub));
    uint32_t w[4];
    if (!in.pub || !e.upload_powers(a.beta, a.n_beta, false, &in.beta_pows, &in.beta_f64) ||
        !e.perm_chip(d, in, d_parts, static_cast<uint32_t *>(totals.ptr), static_cast<uint32_t *>(scan.ptr), d_perm,
                     static_cast<uint32_t *>(d_cum.ptr)) ||
        !e.download(w, d_cum.ptr, sizeof w))
        return engine_fail(p->err, e);
    for (int k = 0; k < 4; k++) cum[k] = Fp::raw(w[k]).canonical();
    return DVT_OK;
}

int dvt_stage_quotient(dvt_prover *p, const char *machine, uint32_t chip, const uint32_t *d_main_lde, const uint32_t *d_prep_lde,
                       const uint32_t *d_perm_lde, uint32_t log_n, const uint32_t *pub, const uint32_t perm_alpha[4],
                       const uint32_t beta[4], const uint32_t alpha[4], const uint32_t cum[4], uint32_t path, uint32_t selectors,
                       uint32_t *d_out) {
    if (!p) return DVT_ERR_INPUT;
    ChipStageArgs a;
    if (int rc = chip_stage_args(p, machine, chip, log_n, pub, perm_alpha, beta, path, &a)) return rc;
    const ChipDesc &d = *a.d;
    Fp4 al, cs;
    if (!alpha || !cum) return fail(p, DVT_ERR_INPUT, "null argument");
    if (!ext_from_canonical(alpha, &al) || !ext_from_canonical(cum, &cs)) return fail(p, DVT_ERR_INPUT, "alpha or cum not canonical");
    if (selectors > DVT_SELECTORS_IN_KERNEL) return fail(p, DVT_ERR_INPUT, "selectors %u", selectors);
    if (!d_main_lde || (d.prep_w && !d_prep_lde) || (d.perm_ext_w && !d_perm_lde) || !d_out) return fail(p, DVT_ERR_INPUT, "null argument");
    const size_t m = (size_t)2 << log_n, out_bytes = 16 * m;
    if (overlap(d_out, out_bytes, d_main_lde, 4 * d.main_w * m) || (d.prep_w && overlap(d_out, out_bytes, d_prep_lde, 4 * d.prep_w * m)) ||
        (d.perm_ext_w && overlap(d_out, out_bytes, d_perm_lde, 16 * d.perm_ext_w * m)))
        return fail(p, DVT_ERR_INPUT, "out overlaps an input");
    Guard g(p); if (g.rc) return g.rc;
    Engine &e = eng0(p);
    StageBuf parts{e.pool};
    uint32_t *d_parts;
    if (int rc = chip_stage_parts(p, path, d.quot_parts, log_n, 8, &parts, &d_parts)) return rc;
    Engine::ChipInputs in{d_main_lde, d.prep_w ? d_prep_lde : nullptr, nullptr, log_n, a.perm_alpha, nullptr, nullptr};
    in.pub = static_cast<const uint32_t *>(e.upload_vec(a.pub));
    const Fp4 *d_alpha;
    const double *d_alpha_f64;
    if (!in.pub || !e.upload_powers(a.beta, a.n_beta, false, &in.beta_pows, &in.beta_f64) ||
        !e.upload_powers(al, a.n_alpha, true, &d_alpha, &d_alpha_f64) ||
        !e.quotient_chip(d, in, d.perm_ext_w ? d_perm_lde : nullptr, cs, d_alpha, d_alpha_f64, selectors == DVT_SELECTORS_TABLE, d_parts,
                         d_out))
        return engine_fail(p->err, e);
    return DVT_OK;
}

// ------------------------------------------------------------------ machine level
int dvt_machine_setup(dvt_prover *p, const char *machine, const dvt_host_trace *prep, size_t nprep, dvt_pk **pk_out,
                      uint8_t **vk, size_t *vk_len) {
    if (!p || !pk_out) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    const MachineDesc *m = machine_by_name(machine);
    if (!m) return fail(p, DVT_ERR_INPUT, "unknown machine '%s'", machine ? machine : "(null)");
    std::vector<ChipRef> refs;
    std::vector<std::vector<uint32_t>> host;
    for (size_t i = 0; i < nprep; i++) {
        if ((int)prep[i].chip_id >= m->n_chips || prep[i].log_n > 22 || !prep[i].data) return fail(p, DVT_ERR_INPUT, "bad preprocessed trace %zu", i);
        if (i && prep[i].chip_id <= prep[i - 1].chip_id) return fail(p, DVT_ERR_INPUT, "preprocessed traces must be sorted by chip id");
        size_t words = (size_t)m->chips[prep[i].chip_id].prep_w << prep[i].log_n;
        for (size_t k = 0; k < words; k++)
            if (prep[i].data[k] >= P) return fail(p, DVT_ERR_INPUT, "preprocessed trace %zu holds a non-canonical value", i);
        refs.push_back({(int)prep[i].chip_id, prep[i].log_n});
        host.emplace_back(prep[i].data, prep[i].data + words);
    }
    for (int c = 0; c < m->n_chips; c++)
        if (m->chips[c].prep_w) {
            bool have = false;
            for (auto &r : refs) have |= r.chip_id == c;
            if (!have) return fail(p, DVT_ERR_INPUT, "chip %s needs a preprocessed trace", m->chips[c].name);
        }
    dvt_pk *pk = new dvt_pk();
    pk->dev.emplace_back();
    const int rc = eng0(p).setup(m, refs, host, &pk->dev[0].key) ? DVT_OK : engine_fail(p->err, eng0(p));
    return setup_finish(p, pk, rc, pk_out, vk, vk_len);
}

void dvt_pk_free(dvt_prover *p, dvt_pk *pk) {
    if (!p || !pk) return;
    Guard g(p);
    pk_release(p, pk);
}

int dvt_machine_prove(dvt_prover *p, const dvt_pk *pk, const dvt_host_trace *main, size_t nmain, const uint32_t *pubs, size_t npub,
                      uint8_t **proof, size_t *proof_len) {
    if (!p || !pk || !main || !nmain || !proof || !proof_len || (npub && !pubs)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    const MachineDesc *m = pk->dev[0].key.vk.machine;
    std::vector<uint32_t *> dev(nmain, nullptr);
    std::vector<ChipTrace> traces;
    int rc = DVT_OK;
    auto cleanup = [&] { for (auto d : dev) if (d) (void)hipFree(d); };
    for (size_t i = 0; i < nmain && rc == DVT_OK; i++) {
        if ((int)main[i].chip_id >= m->n_chips || main[i].log_n > 22 || !main[i].data) { rc = fail(p, DVT_ERR_INPUT, "bad main trace %zu", i); break; }
        size_t words = (size_t)m->chips[main[i].chip_id].main_w << main[i].log_n;
        for (size_t k = 0; k < words; k++)
            if (main[i].data[k] >= P) { rc = fail(p, DVT_ERR_INPUT, "main trace %zu holds a non-canonical value", i); break; }
        if (rc) break;
        if (hipMalloc(&dev[i], words * 4) != hipSuccess || hipMemcpy(dev[i], main[i].data, words * 4, hipMemcpyHostToDevice) != hipSuccess ||
            launch_to_internal(eng0(p).stream, dev[i], words) != hipSuccess) {
            rc = fail(p, DVT_ERR_DEVICE, "uploading main trace %zu failed", i);
            break;
        }
        traces.push_back({(int)main[i].chip_id, main[i].log_n, dev[i]});
    }
    if (rc) { cleanup(); return rc; }
    std::vector<Fp> pv(npub);
    for (size_t i = 0; i < npub; i++) {
        if (pubs[i] >= P) { cleanup(); return fail(p, DVT_ERR_INPUT, "public value %zu not canonical", i); }
        pv[i] = Fp::from_canonical(pubs[i]);
    }
    ShardProof sp;
    bool ok = eng0(p).prove_shard(pk->dev[0].key, traces, pv, p->cfg, &sp);
    (void)hipStreamSynchronize(eng0(p).stream);
    cleanup();
    if (!ok) return engine_fail(p->err, eng0(p));
    WordWriter w;
    write_shard_proof(w, sp);
    *proof = copy_out(w.w, proof_len);
    if (!*proof) return fail(p, DVT_ERR_DEVICE, "out of host memory");
    return DVT_OK;
}

int dvt_machine_verify(const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len, uint32_t fri_queries,
                       uint32_t pow_bits, char **reason) {
    if (reason) *reason = nullptr;
    if (!vk || !proof) return reject(reason, DVT_ERR_INPUT, "null argument");
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key)) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    return verify_words(proof, proof_len, DVT_ERR_INPUT, reason, [&](WordReader &r, std::string &why) {
        const ShardProof sp = read_shard_proof(r);
        if (r.p != r.end) why = "trailing bytes after proof";
        else why = verify_shard(key, sp, StarkConfig{fri_queries, pow_bits});
        return why.empty() ? DVT_OK : DVT_ERR_REJECTED;
    });
}

int dvt_prover_machine_verify(dvt_prover *p, const uint8_t *vk, size_t vk_len, const uint8_t *proof, size_t proof_len,
                              uint32_t fri_queries, uint32_t pow_bits, char **reason) {
    if (reason) *reason = nullptr;
    if (!p) return DVT_ERR_INPUT;
    if (!vk || !proof) return reject(reason, DVT_ERR_INPUT, "null argument");
    VerifyingKey key;
    if (!vk_parse(vk, vk_len, &key)) return reject(reason, DVT_ERR_INPUT, "malformed verifying key");
    Guard g(p); if (g.rc) return g.rc;
    int dev_rc = DVT_OK;
    const int rc = verify_words(proof, proof_len, DVT_ERR_INPUT, reason, [&](WordReader &r, std::string &why) {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t *w0 = r.p;
        const ShardProof sp = read_shard_proof(r);
        if (r.p != r.end) why = "trailing bytes after proof";
        else {
            ShardQueryCtx ctx;
            why = verify_shard_host(key, sp, StarkConfig{fri_queries, pow_bits}, nullptr, nullptr, &ctx);
            if (why.empty()) {
                DeviceQueries dq(p);
                dq.add(ctx, w0, (size_t)(r.end - w0));
                dq.finish(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
                if ((dev_rc = dq.rc)) return DVT_OK;
                why = dq.why(0);
            }
        }
        return why.empty() ? DVT_OK : DVT_ERR_REJECTED;
    });
    return dev_rc ? dev_rc : rc;
}

int dvt_prover_verify_times(dvt_prover *p, double out[9]) {
    if (!p || !out) return DVT_ERR_INPUT;
    std::lock_guard<std::mutex> lk(p->mu);
    for (int i = 0; i < 9; i++) out[i] = p->vq_times[i];
    return DVT_OK;
}

int dvt_stage_sponge_rows(dvt_prover *p, const uint32_t *words, const uint32_t *lens, size_t n, uint32_t *digests) {
    if (!p) return DVT_ERR_INPUT;
    if (!n) return DVT_OK;
    if (!lens || !digests) return fail(p, DVT_ERR_INPUT, "null argument");
    size_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (lens[i] > (1u << 24)) return fail(p, DVT_ERR_INPUT, "vector %zu is longer than 2^24 words", i);
        total += lens[i];
    }
    if ((total && !words) || total + 8 * n >= ((size_t)1 << 31)) return fail(p, DVT_ERR_INPUT, "null or too many words");
    Guard g(p); if (g.rc) return g.rc;
    return vq::stage_sponge_rows(lane0(p), words, lens, n, digests);
}

int dvt_stage_verify_paths(dvt_prover *p, const dvt_path_chain *chains, size_t n, uint8_t *ok) {
    if (!p) return DVT_ERR_INPUT;
    if (!n) return DVT_OK;
    if (!chains || !ok || n > (1u << 24)) return fail(p, DVT_ERR_INPUT, "null argument or too many chains");
    for (size_t i = 0; i < n; i++)
        if (!chains[i].start || !chains[i].root) return fail(p, DVT_ERR_INPUT, "chain %zu: null digest", i);
    Guard g(p); if (g.rc) return g.rc;
    return vq::stage_verify_paths(lane0(p), chains, n, ok);
}

int dvt_stage_multipath_nodes(uint32_t depth, const uint32_t *indices, size_t n, uint32_t *out_level_index, size_t cap, size_t *n_out) {
    if (depth > 30 || (n && !indices) || (cap && !out_level_index) || !n_out) return DVT_ERR_INPUT;
    const MultipathPlan pl = multipath_plan(depth, indices, n);
    *n_out = pl.nodes.size();
    for (size_t i = 0; i < pl.nodes.size() && i < cap; i++) {
        out_level_index[2 * i] = pl.nodes[i].first;
        out_level_index[2 * i + 1] = pl.nodes[i].second;
    }
    return DVT_OK;
}

int dvt_stage_verify_multipath(dvt_prover *p, uint32_t depth, const uint32_t *leaf_index, const uint32_t *leaf_digest, size_t n,
                               const uint8_t *inject_at, const uint32_t *inject, const uint32_t *nodes, size_t n_nodes,
                               const uint32_t *root, uint8_t *ok) {
    if (!p) return DVT_ERR_INPUT;
    if (!n || n > vq::MP_MAX_SLOTS || depth > 30) return fail(p, DVT_ERR_INPUT, "1..%u queries and a depth of at most 30", vq::MP_MAX_SLOTS);
    if (!leaf_index || !leaf_digest || !root || !ok || (n_nodes && !nodes) || (inject_at && depth && !inject)) return fail(p, DVT_ERR_INPUT, "null argument");
    Guard g(p); if (g.rc) return g.rc;
    return vq::stage_verify_multipath(lane0(p), depth, leaf_index, leaf_digest, n, inject_at, inject, nodes, n_nodes, root, ok);
}

int dvt_last_kernel_stats(dvt_prover *p, double out[9]) {
    if (!p || !out) return DVT_ERR_INPUT;
    const StageTimes &t = eng0(p).times;
    out[0] = t.lde_ms; out[1] = t.lde_alg_bytes; out[2] = t.lde_calls; out[3] = t.merkle_ms; out[4] = t.merkle_perms;
    out[5] = t.cells_m; out[6] = t.cells_p; out[7] = t.cells_q; out[8] = t.cells_pre;
    return DVT_OK;
}

int dvt_last_stage_ms(dvt_prover *p, float out[6]) {
    if (!p || !out) return DVT_ERR_INPUT;
    const StageTimes &t = eng0(p).times;
    out[0] = t.commit_main; out[1] = t.perm; out[2] = t.quotient; out[3] = t.open; out[4] = t.fri; out[5] = t.total;
    return DVT_OK;
}

}  // extern "C"
