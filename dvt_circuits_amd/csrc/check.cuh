// Trace-row checks of a chip on the GPU, over the same generated AIR source (gen/air_*.inc) as K4 and K5:
//   - check_rows_kernel<Air>: one trace-domain row per thread; does every constraint of the chip vanish on the rows where
//     it is active?  (CheckRowCtx: the third context of the generated code next to ConstraintFolder and PermRowCtx.)
//   - bus_rows_kernel<Air> + bus_fold_kernel: the sum over the rows of the chip's signed LogUp terms, bus by bus.
// Inputs are the column-major Montgomery matrices K4 reads (main[c * n + row]; rotation 1 of the last row is row 0).
//
// UNITS.  What is counted and reported is a unit: a plain constraint (its index), or a whole big-integer identity
// (assert_poly_zero) under the index of its FIRST coefficient constraint.  The generated C++ holds an identity only in
// closed form, alpha^first (C(alpha) + (alpha - 256) W(alpha)); the checker evaluates C(xi) + (xi - 256) W(xi) at a point
// xi of F_p^4 that the caller supplies, and a non-zero value is ONE violation of unit `first`: the indices first + 1 ..
// first + K - 1 never fire.  The value is a polynomial of degree < K in xi whose coefficients are the K coefficient
// constraints, so a row with a wrong coefficient is missed with probability at most K / p^4 over xi (K <= 95, p^4 ~ 2^124).
// This is a diagnostic for rows that are wrong by accident, not a soundness boundary: xi does not depend on the rows.
#pragma once
#include <algorithm>

#include "stark.cuh"

#define DVT_CHECK_BUSES_N 8   // = DVT_CHECK_BUSES (include/dvt_prover.h): accumulators per row, indexed by bus id

namespace dvt {

#if defined(__HIPCC__)
constexpr unsigned long long CHECK_NO_KEY = ~0ull;

struct CheckArgs {
    const uint32_t *main;   // [MAIN_W][N]
    const uint32_t *prep;   // [PREP_W][N]
    const uint32_t *pub;    // device public values (Montgomery)
    const Fp4 *xi_pows;     // xi^0, xi^1, ... (upload_powers(xi, .., true)), at least as many as the longest limb vector
    const double *xi_d;     // the same as centred doubles [..][4]
    uint32_t log_n;
    uint32_t *counts;            // [N_CONSTRAINTS] out (zeroed by the caller): rows that violate each unit
    unsigned long long *first;   // out (CHECK_NO_KEY from the caller): min over the violations of row << 32 | unit
};

template <class Air>
struct CheckRowCtx {
    using T = Fp;
    const CheckArgs &a;
    size_t n, row;
    bool live;              // row < n: the threads past the table run along (the ballots want whole waves) and report nothing
    uint32_t first_unit;    // lowest violated unit of this row so far
    __device__ CheckRowCtx(const CheckArgs &args, size_t r)
        : a(args), n((size_t)1 << args.log_n), row(r & (((size_t)1 << args.log_n) - 1)), live(r < ((size_t)1 << args.log_n)), first_unit(~0u) {}
    __device__ static T K(uint32_t m) { return Fp::raw(m); }
    __device__ static T KI(uint32_t canonical) { return Fp::from_canonical(canonical); }
    __device__ T main(int c, int r) const { return Fp::raw(a.main[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T prep(int c, int r) const { return Fp::raw(a.prep[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T pub(int k) const { return Fp::raw(a.pub[k]); }

    // one ballot per unit; the first violating lane of a wave adds the wave's count: a clean trace issues no atomic
    __device__ __forceinline__ void report(int unit, bool bad) {
        const unsigned long long m = __ballot(bad);
        if (m) {
            if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(&a.counts[unit], (uint32_t)__popcll(m));
            if (bad && (uint32_t)unit < first_unit) first_unit = (uint32_t)unit;
        }
    }
    // `when` as a predicate on the trace row (oracle/air_oracle.c orc_check_constraints)
    __device__ __forceinline__ void constraint(int idx, int when, const T &v) {
        const bool active = when == WHEN_ALL || (when == WHEN_FIRST && row == 0) || (when == WHEN_LAST && row == n - 1) ||
                            (when == WHEN_TRANS && row != n - 1);
        report(idx, live && active && !v.is_zero());
    }
    // V(xi) = sum_k xi^k v_k
    __device__ __forceinline__ Fp4 poly(const T *v, int nv) const {
        DotAcc4 s;
        for (int k = 0; k < nv; k++) {
            s.add(a.xi_d + 4 * k, v[k]);
            if ((k & 31) == 31) s.reduce();
        }
        return s.value();
    }
    __device__ __forceinline__ Fp4 alpha_minus(uint32_t k) const { return a.xi_pows[1] - Fp::from_canonical(k); }
    __device__ __forceinline__ void fold_poly(int first, const Fp4 &tot) { report(first, live && tot != Fp4::zero()); }
    __device__ void interaction(int, int, int, int, const T &, const T *, int) {}
};

template <class Air, int PART, class Ctx>
__device__ __forceinline__ void constraints_of_part(Ctx &ctx, int part) {
    if (part == PART) Air::template constraints_part<PART>(ctx);
    else if constexpr (PART + 1 < Air::N_PARTS) constraints_of_part<Air, PART + 1>(ctx, part);
}
// grid (row blocks, Air::N_PARTS): the constraint group blockIdx.y of the generated code on one row per thread
template <class Air>
__global__ void __launch_bounds__(256) check_rows_kernel(CheckArgs a) {
    CheckRowCtx<Air> ctx(a, (size_t)blockIdx.x * blockDim.x + threadIdx.x);
    constraints_of_part<Air, 0>(ctx, (int)blockIdx.y);
    if (ctx.first_unit != ~0u) atomicMin(a.first, ((unsigned long long)ctx.row << 32) | ctx.first_unit);
}
template <class Air>
hipError_t launch_check_t(hipStream_t st, const CheckArgs &a) {
    if (Air::N_CONSTRAINTS == 0) return hipSuccess;
    const size_t n = (size_t)1 << a.log_n;
    check_rows_kernel<Air><<<dim3((unsigned)((n + 255) / 256), Air::N_PARTS), 256, 0, st>>>(a);
    return hipGetLastError();
}

// ------------------------------------------------------------------ per-bus LogUp sums
constexpr unsigned BUS_ROW_BLOCKS_MAX = 1024;   // row blocks of a launch: a block walks the rows with that stride
struct BusArgs {
    const uint32_t *main, *prep, *pub;
    const double *beta_d;   // beta^1 .. as centred doubles [..][4] (upload_powers(beta, .., false))
    Fp4 perm_alpha;
    uint32_t log_n;
    uint32_t *partial;      // [gridDim.y * gridDim.x][DVT_CHECK_BUSES_N][4] scratch
    uint32_t *out;          // [DVT_CHECK_BUSES_N][4] Montgomery words
};
inline unsigned bus_row_blocks(uint32_t log_n) { return (unsigned)std::min<size_t>(BUS_ROW_BLOCKS_MAX, (((size_t)1 << log_n) + 255) / 256); }

template <class Air>
struct BusRowCtx {
    using T = Fp;
    const BusArgs &a;
    size_t n, row;
    bool live;
    Fp4 (&acc)[DVT_CHECK_BUSES_N];
    __device__ BusRowCtx(const BusArgs &args, size_t r, Fp4 (&sums)[DVT_CHECK_BUSES_N])
        : a(args), n((size_t)1 << args.log_n), row(r & (((size_t)1 << args.log_n) - 1)), live(r < ((size_t)1 << args.log_n)), acc(sums) {}
    __device__ static T K(uint32_t m) { return Fp::raw(m); }
    __device__ static T KI(uint32_t canonical) { return Fp::from_canonical(canonical); }
    __device__ T main(int c, int r) const { return Fp::raw(a.main[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T prep(int c, int r) const { return Fp::raw(a.prep[(size_t)c * n + ((row + r) & (n - 1))]); }
    __device__ T pub(int k) const { return Fp::raw(a.pub[k]); }
    // +- mult / (alpha_p + bus + sum_k beta^(k+1) v_k) into the accumulator of the bus (a literal in the generated code)
    __device__ __forceinline__ void interaction(int /*j*/, int bus, int sign, int /*scope*/, const T &mult, const T *vals, int nv) {
        if (!live || mult.is_zero() || bus < 0 || bus >= DVT_CHECK_BUSES_N) return;
        DotAcc4 s;
        for (int k = 0; k < nv; k++) {
            s.add(a.beta_d + 4 * k, vals[k]);
            if ((k & 31) == 31) s.reduce();
        }
        const Fp4 d = a.perm_alpha + Fp::from_canonical((uint32_t)bus) + s.value();
        acc[bus] += inv(d) * (sign > 0 ? mult : -mult);
    }
};

// grid (row blocks <= BUS_ROW_BLOCKS_MAX, Air::N_LPARTS): the LogUp group blockIdx.y on the rows blockIdx.x * 256 + t,
// + gridDim.x * 256, ...  Sums within the wave by shuffles, across the block's waves through LDS.  Field addition is exact
// and commutative: the result does not depend on the launch shape, and no atomic is needed.
template <class Air>
__global__ void __launch_bounds__(256) bus_rows_kernel(BusArgs a) {
    constexpr int W = 4 * DVT_CHECK_BUSES_N;
    __shared__ uint32_t lds[4][W];
    Fp4 acc[DVT_CHECK_BUSES_N];
#pragma unroll
    for (int b = 0; b < DVT_CHECK_BUSES_N; b++) acc[b] = Fp4::zero();
    const size_t n = (size_t)1 << a.log_n;
    for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {
        BusRowCtx<Air> ctx(a, base + threadIdx.x, acc);
        interactions_of_part<Air, 0>(ctx, (int)blockIdx.y);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int b = 0; b < DVT_CHECK_BUSES_N; b++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            Fp v = acc[b].c[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v = v + Fp::raw((uint32_t)__shfl_down((int)v.v, off, 64));
            if (lane == 0) lds[wave][4 * b + k] = v.v;
        }
    __syncthreads();
    if (threadIdx.x < W) {
        const Fp v = Fp::raw(lds[0][threadIdx.x]) + Fp::raw(lds[1][threadIdx.x]) + Fp::raw(lds[2][threadIdx.x]) + Fp::raw(lds[3][threadIdx.x]);
        a.partial[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * W + threadIdx.x] = v.v;
    }
}
// one block: out[w] = sum over the n_partial blocks of partial[.][w]
template <int UNUSED>
__global__ void __launch_bounds__(256) bus_fold_kernel(const uint32_t *partial, uint32_t n_partial, uint32_t *out) {
    constexpr int W = 4 * DVT_CHECK_BUSES_N;
    __shared__ uint32_t lds[256 / W][W];
    const uint32_t w = threadIdx.x % W, g = threadIdx.x / W;
    Fp v = Fp::zero();
    for (uint32_t i = g; i < n_partial; i += 256 / W) v = v + Fp::raw(partial[(size_t)i * W + w]);
    lds[g][w] = v.v;
    __syncthreads();
    if (threadIdx.x < W) {
        Fp s = Fp::zero();
        for (int k = 0; k < 256 / W; k++) s = s + Fp::raw(lds[k][threadIdx.x]);
        out[threadIdx.x] = s.v;
    }
}
template <class Air>
hipError_t launch_bus_t(hipStream_t st, const BusArgs &a) {
    if (Air::N_INTERACTIONS == 0) return hipMemsetAsync(a.out, 0, 16 * DVT_CHECK_BUSES_N, st);
    const unsigned bx = bus_row_blocks(a.log_n);
    bus_rows_kernel<Air><<<dim3(bx, Air::N_LPARTS), 256, 0, st>>>(a);
    bus_fold_kernel<0><<<1, 256, 0, st>>>(a.partial, bx * Air::N_LPARTS, a.out);
    return hipGetLastError();
}
// words of BusArgs::partial that serve every chip at every height
constexpr size_t BUS_PARTIAL_WORDS = (size_t)BUS_ROW_BLOCKS_MAX * PARTS_MAX * 4 * DVT_CHECK_BUSES_N;
#endif  // __HIPCC__

}  // namespace dvt
