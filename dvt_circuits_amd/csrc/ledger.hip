// The bus ledger on one lane (ledger.cuh): its device buffers, the kernels that do not depend on a chip, and the host's
// end of it (the result records, their merge across ledgers).  The passes over the chips' interactions are instantiated in
// ledger_toy.hip, ledger_rv32.hip and ledger_rv32_wide.hip.
#include <map>

#include "capi_internal.h"
#include "ledger.cuh"

namespace dvt {
namespace {
// w[i * stride + at] mod p for i < n: the tallies (stride 1) and the records' sums after every launch that added to them
__global__ void __launch_bounds__(256) ledger_reduce_kernel(unsigned long long *w, size_t n, uint32_t stride, uint32_t at) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) w[i * stride + at] %= P;
}
// free records
__global__ void __launch_bounds__(256) ledger_clear_slots_kernel(LedgerSlot *s, uint32_t n) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    s[i].key = 0;
    s[i].sum = 0;
    s[i].first = LEDGER_NO_OCCURRENCE;
    s[i].n_send = s[i].n_recv = 0;
    s[i].bus = s[i].arity = 0;
}
// one bucket per thread, whole waves (2^log_buckets >= 1024): a wave's ballot is two words of the bitmap
__global__ void __launch_bounds__(256) ledger_close_kernel(const unsigned long long *tally, uint32_t *dirty, uint32_t *flags) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long *t = tally + b * 3;
    const unsigned long long m = __ballot((t[0] | t[1] | t[2]) != 0);
    if ((threadIdx.x & 63) == 0) {
        dirty[b >> 5] = (uint32_t)m;
        dirty[(b >> 5) + 1] = (uint32_t)(m >> 32);
        if (m) atomicAdd(flags, (uint32_t)__popcll(m));
    }
}
// a tuple the host adds: one thread
__global__ void ledger_tuple_kernel(LedgerArgs a, LedgerTuple t) {
    if (threadIdx.x || blockIdx.x || t.arity > LEDGER_MAX_ARITY) return;
    ledger_apply(a, t.key, t.bus, t.arity, t.m, t.send != 0, t.occurrence, [&](uint32_t *dst) {
        for (uint32_t k = 0; k < t.arity; k++) dst[k] = t.values[k];
    });
}

unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }
LedgerArgs args_of(const LedgerDev &l, uint32_t mode) {
    LedgerArgs a{};
    a.mode = mode;
    a.seed = l.seed;
    a.log_buckets = l.log_buckets;
    a.tally = l.d_tally;
    a.dirty = l.d_dirty;
    a.slots = static_cast<LedgerSlot *>(l.d_slots);
    a.cap_slots = l.cap_slots;
    a.flags = l.d_flags;
    return a;
}
// after a launch of `mode`: the words it added to, mod p again
hipError_t reduce_after(hipStream_t st, const LedgerDev &l, uint32_t mode) {
    if (mode == LEDGER_TALLY) {
        const size_t n = (size_t)3 << l.log_buckets;
        ledger_reduce_kernel<<<blocks_of(n), 256, 0, st>>>(l.d_tally, n, 1, 0);
    } else {
        ledger_reduce_kernel<<<blocks_of(l.cap_slots), 256, 0, st>>>(static_cast<unsigned long long *>(l.d_slots), l.cap_slots,
                                                                      (uint32_t)(sizeof(LedgerSlot) / 8), 1);
    }
    return hipGetLastError();
}
// the record table, made by the first COLLECT launch: an honest job never allocates it
int want_slots(const Lane &c, LedgerDev &l) {
    if (l.d_slots) return DVT_OK;
    HIP_TRY(c.err, c.eng.pool.alloc_bytes(&l.d_slots, (size_t)l.cap_slots * sizeof(LedgerSlot)));
    ledger_clear_slots_kernel<<<blocks_of(l.cap_slots), 256, 0, c.eng.stream>>>(static_cast<LedgerSlot *>(l.d_slots), l.cap_slots);
    HIP_TRY(c.err, hipGetLastError());
    return DVT_OK;
}
}  // namespace

int ledger_init(const Lane &c, LedgerDev *l, uint32_t log_buckets, uint32_t cap_slots, uint64_t seed) {
    if (log_buckets < 10 || log_buckets > 24) return fail(c.err, DVT_ERR_INPUT, "log_buckets %u (10..24)", log_buckets);
    if (cap_slots == 0 || cap_slots > (1u << 24)) return fail(c.err, DVT_ERR_INPUT, "cap_slots %u (1..2^24)", cap_slots);
    l->log_buckets = log_buckets;
    l->cap_slots = cap_slots;
    l->seed = seed;
    l->pool = &c.eng.pool;
    const size_t tally_bytes = (size_t)24 << log_buckets, dirty_bytes = (size_t)4 << (log_buckets - 5);
    void *t = nullptr, *d = nullptr, *f = nullptr;
    if (c.eng.pool.alloc_bytes(&t, tally_bytes) != hipSuccess || c.eng.pool.alloc_bytes(&d, dirty_bytes) != hipSuccess ||
        c.eng.pool.alloc_bytes(&f, 8) != hipSuccess) {
        for (void *q : {t, d, f}) c.eng.pool.free(q);
        return fail(c.err, DVT_ERR_DEVICE, "no device memory for a ledger of 2^%u buckets", log_buckets);
    }
    l->d_tally = static_cast<unsigned long long *>(t);
    l->d_dirty = static_cast<uint32_t *>(d);
    l->d_flags = static_cast<uint32_t *>(f);
    HIP_TRY(c.err, hipMemsetAsync(t, 0, tally_bytes, c.eng.stream));
    HIP_TRY(c.err, hipMemsetAsync(d, 0, dirty_bytes, c.eng.stream));
    HIP_TRY(c.err, hipMemsetAsync(f, 0, 8, c.eng.stream));
    return DVT_OK;
}

void ledger_release(LedgerDev *l) {
    if (!l->pool) return;
    for (void *q : {(void *)l->d_tally, (void *)l->d_dirty, (void *)l->d_flags, l->d_slots}) l->pool->free(q);
    *l = LedgerDev{};
}

int ledger_rows(const Lane &c, LedgerDev &l, const CheckTable &t, uint32_t chip, const std::vector<uint32_t> &pub_mont, uint32_t tag, uint32_t mode) {
    const ChipDesc &d = *t.d;
    if (!d.launch_ledger) return fail(c.err, DVT_ERR_UNSUPPORTED, "chip %s has no ledger pass", d.name);
    if (t.log_n > 22 || tag >= (1u << 16) || chip >= LEDGER_HOST_CHIP) return fail(c.err, DVT_ERR_INPUT, "log_n %u, tag %u or chip %u out of range", t.log_n, tag, chip);
    if (!d.n_interactions) return DVT_OK;
    const uint32_t *d_pub = c.eng.upload_vec(pub_mont);
    if (!d_pub) return engine_fail(c.err, c.eng);
    if (mode == LEDGER_COLLECT)
        if (int rc = want_slots(c, l)) return rc;
    LedgerArgs a = args_of(l, mode);
    a.main = t.main;
    a.prep = t.prep;
    a.pub = d_pub;
    a.log_n = t.log_n;
    a.tag = tag;
    a.chip = chip;
    HIP_TRY(c.err, d.launch_ledger(c.eng.stream, a));
    HIP_TRY(c.err, reduce_after(c.eng.stream, l, mode));
    return DVT_OK;
}

int ledger_tuple(const Lane &c, LedgerDev &l, uint32_t bus, const uint32_t *values, uint32_t arity, int sign, uint32_t mult, uint32_t tag, uint32_t mode) {
    if (arity > LEDGER_MAX_ARITY || tag >= (1u << 16) || mult >= P) return fail(c.err, DVT_ERR_INPUT, "arity %u, tag %u or multiplicity %u out of range", arity, tag, mult);
    if (mult == 0) return DVT_OK;
    LedgerTuple t{};
    t.bus = bus;
    t.arity = arity;
    for (uint32_t k = 0; k < arity; k++) {
        if (values[k] >= P) return fail(c.err, DVT_ERR_INPUT, "tuple value %u not canonical", k);
        t.values[k] = values[k];
    }
    t.m = sign > 0 ? mult : P - mult;
    t.send = sign > 0;
    t.key = ledger_key(l.seed, bus, arity, t.values);
    t.occurrence = ledger_occurrence(tag, LEDGER_HOST_CHIP, 0, 0);
    if (mode == LEDGER_COLLECT)
        if (int rc = want_slots(c, l)) return rc;
    ledger_tuple_kernel<<<1, 64, 0, c.eng.stream>>>(args_of(l, mode), t);
    HIP_TRY(c.err, hipGetLastError());
    HIP_TRY(c.err, reduce_after(c.eng.stream, l, mode));
    return DVT_OK;
}

int ledger_close(const Lane &c, LedgerDev &l, uint32_t *n_dirty) {
    HIP_TRY(c.err, hipMemsetAsync(l.d_flags, 0, 4, c.eng.stream));
    ledger_close_kernel<<<(1u << l.log_buckets) / 256, 256, 0, c.eng.stream>>>(l.d_tally, l.d_dirty, l.d_flags);
    HIP_TRY(c.err, hipGetLastError());
    if (!c.eng.download(n_dirty, l.d_flags, 4)) return engine_fail(c.err, c.eng);
    return DVT_OK;
}

int ledger_tallies(const Lane &c, LedgerDev &l, std::vector<uint64_t> *out) {
    out->resize((size_t)3 << l.log_buckets);
    if (!c.eng.download(out->data(), l.d_tally, out->size() * 8)) return engine_fail(c.err, c.eng);
    return DVT_OK;
}

uint32_t ledger_dirty_of(const std::vector<uint64_t> &tallies, std::vector<uint32_t> *bitmap) {
    const size_t nb = tallies.size() / 3;
    bitmap->assign(nb / 32, 0);
    uint32_t count = 0;
    for (size_t b = 0; b < nb; b++)
        if (tallies[3 * b] % P || tallies[3 * b + 1] % P || tallies[3 * b + 2] % P) {
            (*bitmap)[b >> 5] |= 1u << (b & 31);
            count++;
        }
    return count;
}

int ledger_set_dirty(const Lane &c, LedgerDev &l, const std::vector<uint32_t> &bitmap) {
    if (bitmap.size() != ((size_t)1 << (l.log_buckets - 5))) return fail(c.err, DVT_ERR_INPUT, "dirty bitmap of another ledger");
    HIP_TRY(c.err, hipMemcpyAsync(l.d_dirty, bitmap.data(), bitmap.size() * 4, hipMemcpyHostToDevice, c.eng.stream));
    HIP_TRY(c.err, hipStreamSynchronize(c.eng.stream));   // (the bitmap is the caller's)
    return DVT_OK;
}

int ledger_records(const Lane &c, LedgerDev &l, std::vector<dvt_bus_tuple> *out, bool *overflow) {
    uint32_t flags[2];
    if (!c.eng.download(flags, l.d_flags, 8)) return engine_fail(c.err, c.eng);
    if (flags[1]) *overflow = true;
    if (!l.d_slots) return DVT_OK;
    std::vector<LedgerSlot> h(l.cap_slots);
    if (!c.eng.download(h.data(), l.d_slots, h.size() * sizeof(LedgerSlot))) return engine_fail(c.err, c.eng);
    auto sat = [](unsigned long long x) { return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x; };
    for (const LedgerSlot &s : h) {
        if (!s.key || s.arity > LEDGER_MAX_ARITY) continue;
        dvt_bus_tuple t{};
        t.bus = s.bus;
        t.arity = s.arity;
        t.net = (uint32_t)(s.sum % P);
        t.n_send = sat(s.n_send);
        t.n_recv = sat(s.n_recv);
        const uint32_t chip = (uint32_t)(s.first >> 32) & 63u;
        t.first_tag = (uint32_t)(s.first >> 38) & 0xffffu;
        t.first_chip = chip == LEDGER_HOST_CHIP ? 0xffffffffu : chip;
        t.first_row = (uint32_t)(s.first >> 10) & 0x3fffffu;
        t.first_interaction = (uint32_t)s.first & 0x3ffu;
        memcpy(t.values, s.values, 4 * s.arity);
        out->push_back(t);
    }
    return DVT_OK;
}

// One list out of the records of one or several ledgers: records of one tuple (bus, arity, values) are added up, the
// balanced ones dropped, the rest sorted by (bus, values).
void ledger_finish(std::vector<dvt_bus_tuple> *tuples) {
    auto key_of = [](const dvt_bus_tuple &t) { return std::make_pair(t.bus, std::vector<uint32_t>(t.values, t.values + t.arity)); };
    auto occ = [](const dvt_bus_tuple &t) { return ledger_occurrence(t.first_tag, t.first_chip == 0xffffffffu ? LEDGER_HOST_CHIP : t.first_chip, t.first_row, t.first_interaction); };
    auto sat_add = [](uint32_t a, uint32_t b) { return a + b < a ? 0xffffffffu : a + b; };
    std::map<std::pair<uint32_t, std::vector<uint32_t>>, dvt_bus_tuple> by;   // (ordered as the result is)
    for (const dvt_bus_tuple &t : *tuples) {
        auto it = by.find(key_of(t));
        if (it == by.end()) { by.emplace(key_of(t), t); continue; }
        dvt_bus_tuple &d = it->second;
        d.net = (uint32_t)(((uint64_t)d.net + t.net) % P);
        d.n_send = sat_add(d.n_send, t.n_send);
        d.n_recv = sat_add(d.n_recv, t.n_recv);
        if (occ(t) < occ(d)) { d.first_tag = t.first_tag; d.first_chip = t.first_chip; d.first_row = t.first_row; d.first_interaction = t.first_interaction; }
    }
    tuples->clear();
    for (auto &kv : by)
        if (kv.second.net) tuples->push_back(kv.second);
}
}  // namespace dvt
