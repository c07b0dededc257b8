// ebm_ensemble_sums, ebm_ensemble_range and ebm_ensemble_histogram (include/ebm_hip.h): reductions ACROSS the columns of a
// handle, per entry of the call (a variable; a histogram may name one twice) and latitude — the column-wise partners of the
// hemispheric mean.  The order of the operations is part of the definitions (blocks of columns reduced in ascending column
// order, the block partials then in ascending block order), so every reduction is two kernels and no atomics, and the three
// share one skeleton:
//   partials   grid (latitude tiles) x (column blocks) x (entries).  A lane owns one 16-byte unit of the row — the pair of
//              cells that is the unit of the pair-split permutation (split_index, ebm_internal.h) — and walks the columns of
//              its block at that unit: its accesses never depend on the layout, only the natural unit it stands for does
//              (stored unit p of a split row is natural unit 2p for p < T, 2(p - T) + 1 otherwise), which indexes the
//              per-latitude input (open_walk).  A wave reads whole 128-byte lines of a column per access; the loads of
//              kWalkBatch columns are issued before the first dependent operation; w is read once per column through the
//              scalar cache, the index being wave-uniform (walk_columns).  The nslots rows of a block's result go to
//              partial[block][entry][slot][pitch] at the lane's own stored index, whole lines again (partial_rows).
//   finish     grid (cell tiles) x (slots) x (entries).  A lane owns one stored cell of one row of partials and combines the
//              blocks in ascending order, the loads of kFinishBatch blocks ahead of the dependent combine; the result goes to
//              the natural index (ensemble_finish_kernel).
// What each adds is its state and its term:
//   sums       three registers per cell, S0, S1, S2 (add_term); the optional center is the per-latitude input.  A tile is one
//              wave: 64 units = 1 KiB = eight whole lines of a column per access.
//   range      three registers per cell: n, min, max (range_term); strict < and > in ascending order, in both kernels, keep
//              the bits of the first of several equal extremes.
//   histogram  a dynamically indexed register array would become scratch, so the slots live in LDS as
//              hist[slot][cell of the pair][lane]: a lane touches only its own two columns of it (no atomics, no barrier),
//              and the 8-byte accesses of a wave to any mix of slots fall on distinct banks — the slot stride, 2 kHistLanes
//              doubles, is a multiple of the 64 banks, so the bank is 2 * lane mod 64 within a group of 32 lanes (reads) and
//              mod 32 within 16 (writes).  (nbins + 2) * kHistLanes * 16 bytes: 66 KiB at 64 bins and 64 lanes.  The
//              per-latitude input is the edges lo, hi and s.
// Nothing is contracted (the library is built with -ffp-contract=off, as the noise recurrence of ebm_noise.h relies on):
// t1 = w*d, t2 = t1*d and t = (x - lo) * s are rounded products of rounded differences, every add is a rounded sum.  Units
// whose first natural cell is at or beyond nlat are never loaded.  Plain vector loads and stores; no scratch.
#include "ebm_internal.h"

namespace ebm {

#ifndef EBM_HIST_LANES
#define EBM_HIST_LANES 64            // units per latitude tile of the histogram: 64 (one full wave) or 32
#endif
constexpr int kHistLanes = EBM_HIST_LANES;
constexpr int kSumsLanes = 64;       // one wave per workgroup: a tile is 64 units = 128 cells; pitch is a multiple of that
constexpr int kRangeLanes = 64;
constexpr int kFinishLanes = 64;     // cells per workgroup of the finish
constexpr int kWalkBatch = 16;       // columns whose loads are in flight together (16 KiB per wave of 64)
constexpr int kFinishBatch = 32;     // block partials in flight together (8-byte loads)
static_assert(kHistLanes == 64 || kHistLanes == 32, "a tile divides the 64 units that the pitch is a multiple of");
static_assert(kSumsBlock % kWalkBatch == 0 && kRangeBlock % kWalkBatch == 0 && kHistBlock % kWalkBatch == 0,
              "a block is a whole number of batches");

typedef const __attribute__((address_space(4))) double ConstDouble;      // never written by a kernel: scalar loads

// ---- the partials' skeleton -----------------------------------------------------------------------------------------------

// What a lane of a partials kernel stands for and reads
struct Walk {
    int v;                           // the entry of the call
    long long b;                     // the block of columns
    int p, u;                        // the stored unit, < pitch / 2, and the natural unit it stands for
    long long stride;                // units per row
    const double2 *col;              // the lane's unit of the block's first column
    ConstDouble *w;                  // the block's first weight
    int ncols;                       // columns of this block (wave-uniform)
};

// The lane of a tile of LANES units walking blocks of BLOCK columns; false: padding, never read — the kernel returns
template <int LANES, int BLOCK>
__device__ __forceinline__ bool open_walk(const EnsembleArgs &a, Walk &k) {
    k.v = blockIdx.z;
    k.b = blockIdx.y;
    k.p = blockIdx.x * LANES + threadIdx.x;
    k.u = natural_unit(k.p, a.threads, (a.split_mask >> k.v) & 1u);
    if (2 * k.u >= a.nlat) return false;
    k.stride = a.pitch / 2;
    k.col = reinterpret_cast<const double2 *>(a.row[k.v]) + k.b * BLOCK * k.stride + k.p;
    k.w = reinterpret_cast<ConstDouble *>(reinterpret_cast<uintptr_t>(a.w + k.b * BLOCK));
    k.ncols = min(BLOCK, a.ncol - (int)k.b * BLOCK);
    return true;
}

// term(x, w_c) for the columns of the block in ascending order
template <class Term>
__device__ __forceinline__ void walk_columns(const Walk &k, Term term) {
    int j0 = 0;
    for (; j0 + kWalkBatch <= k.ncols; j0 += kWalkBatch) {
        double2 x[kWalkBatch];
#pragma unroll
        for (int j = 0; j < kWalkBatch; ++j) x[j] = k.col[(j0 + j) * k.stride];
#pragma unroll
        for (int j = 0; j < kWalkBatch; ++j) term(x[j], k.w[j0 + j]);
    }
    for (; j0 < k.ncols; ++j0) term(k.col[j0 * k.stride], k.w[j0]);    // the last block's odd tail
}

// the lane's unit of row 0 of the nslots rows of its block's and entry's partials; row i is i * stride further
__device__ __forceinline__ double2 *partial_rows(const EnsembleArgs &a, const Walk &k, int nslots) {
    return reinterpret_cast<double2 *>(a.partial + (k.b * a.nvars + k.v) * nslots * (long long)a.pitch) + k.p;
}
__device__ __forceinline__ void store_three_rows(const EnsembleArgs &a, const Walk &k, double2 r0, double2 r1, double2 r2) {
    double2 *const out = partial_rows(a, k, 3);
    out[0] = r0;
    out[k.stride] = r1;
    out[2 * k.stride] = r2;
}

// ---- sums -----------------------------------------------------------------------------------------------------------------

// one column's term of one cell: contributes iff w != 0.0 and x is not NaN
__device__ __forceinline__ void add_term(double x, double c, bool centered, double w, double &s0, double &s1, double &s2) {
    const double d = centered ? x - c : x;
    const double t1 = w * d;
    const double t2 = t1 * d;
    const bool in = w != 0.0 && x == x;
    s0 = in ? s0 + w : s0;
    s1 = in ? s1 + t1 : s1;
    s2 = in ? s2 + t2 : s2;
}

__global__ void __launch_bounds__(kSumsLanes) ensemble_partials_kernel(const EnsembleArgs a) {
    Walk k;
    if (!open_walk<kSumsLanes, kSumsBlock>(a, k)) return;
    const bool centered = a.aux != nullptr;                          // aux: center [entry][pitch], natural layout
    const double2 c = centered ? reinterpret_cast<const double2 *>(a.aux + (long long)k.v * a.pitch)[k.u] : make_double2(0.0, 0.0);
    double2 s0 = make_double2(0.0, 0.0), s1 = s0, s2 = s0;
    walk_columns(k, [&](const double2 x, const double wc) {
        add_term(x.x, c.x, centered, wc, s0.x, s1.x, s2.x);
        add_term(x.y, c.y, centered, wc, s0.y, s1.y, s2.y);
    });
    store_three_rows(a, k, s0, s1, s2);
}

// ---- range ----------------------------------------------------------------------------------------------------------------

// one column's value of one cell: contributes iff w != 0.0 and x is not NaN
__device__ __forceinline__ void range_term(double x, double w, double &n, double &mn, double &mx) {
    const bool counts = w != 0.0 && x == x;
    n = counts ? n + 1.0 : n;
    mn = (counts && x < mn) ? x : mn;
    mx = (counts && x > mx) ? x : mx;
}

__global__ void __launch_bounds__(kRangeLanes) range_partials_kernel(const EnsembleArgs a) {
    Walk k;
    if (!open_walk<kRangeLanes, kRangeBlock>(a, k)) return;
    const double inf = __builtin_huge_val();
    double2 n = make_double2(0.0, 0.0), mn = make_double2(inf, inf), mx = make_double2(-inf, -inf);
    walk_columns(k, [&](const double2 x, const double wc) {
        range_term(x.x, wc, n.x, mn.x, mx.x);
        range_term(x.y, wc, n.y, mn.y, mx.y);
    });
    store_three_rows(a, k, n, mn, mx);
}

// ---- histogram ------------------------------------------------------------------------------------------------------------

// the slot of a value that is not NaN: 0 below lo, nbins + 1 at or above hi, else 1 + min((int)((x - lo) * s), nbins - 1)
__device__ __forceinline__ int slot_of(double x, double lo, double hi, double s, int nbins) {
    const bool below = x < lo, above = x >= hi;
    const double d = x - lo;
    const double t = d * s;
    const int i = (int)((below || above || x != x) ? 0.0 : t);       // converted only where 0 <= t <= nbins
    return below ? 0 : above ? nbins + 1 : 1 + min(i, nbins - 1);
}

__global__ void __launch_bounds__(kHistLanes) histogram_partials_kernel(const EnsembleArgs a) {
    extern __shared__ double hist[];                                 // [nslots][2][kHistLanes]
    Walk k;
    if (!open_walk<kHistLanes, kHistBlock>(a, k)) return;            // (no barrier below)
    const int nslots = a.nslots, nbins = nslots - 2;
    double *const mine0 = hist + threadIdx.x, *const mine1 = mine0 + kHistLanes;     // slot i of cell e: mine_e[i * 2 kHistLanes]
    for (int i = 0; i < nslots; ++i) {
        mine0[i * 2 * kHistLanes] = 0.0;
        mine1[i * 2 * kHistLanes] = 0.0;
    }
    // aux: edges [entry][lo, hi, s][pitch], natural layout
    const double2 *const edges = reinterpret_cast<const double2 *>(a.aux + 3LL * k.v * a.pitch) + k.u;
    const double2 lo = edges[0], hi = edges[k.stride], sc = edges[2 * k.stride];
    walk_columns(k, [&](const double2 x, const double wc) {
        double *const s0 = mine0 + slot_of(x.x, lo.x, hi.x, sc.x, nbins) * 2 * kHistLanes;
        double *const s1 = mine1 + slot_of(x.y, lo.y, hi.y, sc.y, nbins) * 2 * kHistLanes;
        const double h0 = *s0, h1 = *s1;                             // the two cells never share a word: both loads first
        const bool in0 = wc != 0.0 && x.x == x.x, in1 = wc != 0.0 && x.y == x.y;
        *s0 = in0 ? h0 + wc : h0;
        *s1 = in1 ? h1 + wc : h1;
    });
    double2 *const out = partial_rows(a, k, nslots);
    for (int i = 0; i < nslots; ++i) out[i * k.stride] = make_double2(mine0[i * 2 * kHistLanes], mine1[i * 2 * kHistLanes]);
}

// ---- finish ---------------------------------------------------------------------------------------------------------------

// The combine of the block partials of slot q, in ascending block order: the sum (sums, histogram) ...
struct SumOfBlocks {
    static __device__ __forceinline__ double none(int) { return 0.0; }
    static __device__ __forceinline__ double of(double r, double x, int) { return r + x; }
};
// ... or by quantity n, min, max (range): the first of equal extremes stays
struct RangeOfBlocks {
    static __device__ __forceinline__ double none(int q) { return q == 0 ? 0.0 : q == 1 ? __builtin_huge_val() : -__builtin_huge_val(); }
    static __device__ __forceinline__ double of(double r, double x, int q) { return q == 0 ? r + x : q == 1 ? (x < r ? x : r) : (x > r ? x : r); }
};

// blockIdx.y = slot, blockIdx.z = entry.  Lane = one stored cell s = 2p + e of that row of partials.  NSLOTS: the slots of an
// entry where the reduction fixes them, 0: a.nslots.
template <class Combine, int NSLOTS>
__global__ void __launch_bounds__(kFinishLanes) ensemble_finish_kernel(const EnsembleArgs a) {
    const int nslots = NSLOTS ? NSLOTS : a.nslots;
    const int row = blockIdx.y, v = row / nslots, q = row - nslots * v;
    const int s = blockIdx.x * kFinishLanes + threadIdx.x;           // stored cell, < pitch
    const int k = 2 * natural_unit(s >> 1, a.threads, (a.split_mask >> v) & 1u) + (s & 1);
    if (k >= a.nlat) return;
    const double *const part = a.partial + (long long)row * a.pitch + s;
    const long long stride = (long long)nslots * a.nvars * a.pitch;        // from block to block
    double r = Combine::none(q);
    int b = 0;
    for (; b + kFinishBatch <= a.nblocks; b += kFinishBatch) {
        double x[kFinishBatch];
#pragma unroll
        for (int j = 0; j < kFinishBatch; ++j) x[j] = part[(b + j) * stride];
#pragma unroll
        for (int j = 0; j < kFinishBatch; ++j) r = Combine::of(r, x[j], q);
    }
    for (; b < a.nblocks; ++b) r = Combine::of(r, part[b * stride], q);
    a.out[(long long)row * a.nlat + k] = r;
}

// ---- launches -------------------------------------------------------------------------------------------------------------

using EnsembleKernel = void (*)(const EnsembleArgs);
static hipError_t launch_two(EnsembleKernel partials, int lanes, size_t lds, EnsembleKernel finish, const EnsembleArgs &a, hipStream_t s) {
    const unsigned unit_tiles = (unsigned)(a.pitch / (2 * lanes)), cell_tiles = (unsigned)(a.pitch / kFinishLanes);
    partials<<<dim3(unit_tiles, (unsigned)a.nblocks, (unsigned)a.nvars), lanes, lds, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    finish<<<dim3(cell_tiles, (unsigned)(a.nslots * a.nvars)), kFinishLanes, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_ensemble_sums(const EnsembleArgs &a, hipStream_t s) {
    return launch_two(ensemble_partials_kernel, kSumsLanes, 0, ensemble_finish_kernel<SumOfBlocks, 3>, a, s);
}

hipError_t launch_ensemble_range(const EnsembleArgs &a, hipStream_t s) {
    return launch_two(range_partials_kernel, kRangeLanes, 0, ensemble_finish_kernel<RangeOfBlocks, 3>, a, s);
}

hipError_t launch_ensemble_histogram(const EnsembleArgs &a, hipStream_t s) {
    const size_t lds = sizeof(double) * 2 * kHistLanes * (size_t)a.nslots;
    if (lds > 48 * 1024) {                                           // beyond what a launch may ask for unannounced
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(histogram_partials_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 2 * kHistLanes * (kHistMaxBins + 2)));
        if (e != hipSuccess) return e;
    }
    return launch_two(histogram_partials_kernel, kHistLanes, lds, ensemble_finish_kernel<SumOfBlocks, 0>, a, s);
}

}  // namespace ebm
