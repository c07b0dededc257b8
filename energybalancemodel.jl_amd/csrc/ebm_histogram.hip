// ebm_ensemble_range and ebm_ensemble_histogram (include/ebm_hip.h): order statistics ACROSS the columns of a handle, per entry
// of the call and latitude — the partners of ebm_ensemble_sums (ebm_ensemble.hip), whose shape both follow: one kernel forms
// block partials in the order of the definition, a second combines the blocks in ascending order; no atomics.
//   walking    grid (latitude tiles) x (column blocks) x (entries).  A lane owns one 16-byte unit of the row — the pair of
//              cells that is the unit of the pair-split permutation — and walks the columns of its block at that unit, so its
//              accesses never depend on the layout; only the natural unit it stands for does, which indexes the edges.  A
//              wave reads whole 128-byte lines; the loads of kOrderBatch columns are issued before the first dependent
//              operation; w is read once per column through the scalar cache (walk_columns, shared by the two).
//   range      three registers per cell: n, min, max; strict < and > in ascending column order keep the bits of the first
//              of several equal extremes.
//   histogram  a dynamically indexed register array would become scratch, so the slots live in LDS as
//              hist[slot][cell of the pair][lane]: a lane touches only its own two columns of it (no atomics, no barrier),
//              and the 8-byte accesses of a wave to any mix of slots fall on distinct banks — the slot stride, 2 kHistLanes
//              doubles, is a multiple of the 64 banks, so the bank is 2 * lane mod 64 within a group of 32 lanes (reads) and
//              mod 32 within 16 (writes).  (nbins + 2) * kHistLanes * 16 bytes: 66 KiB at 64 bins and 64 lanes.
// Nothing is contracted (-ffp-contract=off): t = (x - lo) * s is a rounded difference times a rounded product.  Units whose
// first natural cell is at or beyond nlat are never loaded.  Plain vector loads and stores; no scratch.
#include "ebm_internal.h"

namespace ebm {

#ifndef EBM_HIST_LANES
#define EBM_HIST_LANES 64            // units per latitude tile of the histogram: 64 (one full wave) or 32
#endif
constexpr int kHistLanes = EBM_HIST_LANES;
constexpr int kRangeLanes = 64;      // one wave per workgroup: a tile is 64 units = 128 cells; pitch is a multiple of that
constexpr int kOrderBatch = 16;      // columns whose loads are in flight together
constexpr int kOrderFinishBatch = 32;    // block partials in flight together (8-byte loads)
static_assert(kHistLanes == 64 || kHistLanes == 32, "a tile divides the 64 units that the pitch is a multiple of");
static_assert(kRangeBlock % kOrderBatch == 0 && kHistBlock % kOrderBatch == 0, "a block is a whole number of batches");

typedef const __attribute__((address_space(4))) double ConstDouble;      // never written by a kernel: scalar loads

// natural index of stored index p (units of a row of 2T units) in a pair-split row
__device__ __forceinline__ int natural_unit_of(int p, int T, bool split) { return !split ? p : (p < T ? 2 * p : 2 * (p - T) + 1); }

// term(x, w_c) for the columns 0 ... ncols - 1 of a block in ascending order: col points at the lane's unit of the block's
// first column, w at the block's first weight
template <class Term>
__device__ __forceinline__ void walk_columns(const double2 *col, long long stride, ConstDouble *w, int ncols, Term term) {
    int j0 = 0;
    for (; j0 + kOrderBatch <= ncols; j0 += kOrderBatch) {
        double2 x[kOrderBatch];
#pragma unroll
        for (int j = 0; j < kOrderBatch; ++j) x[j] = col[(j0 + j) * stride];
#pragma unroll
        for (int j = 0; j < kOrderBatch; ++j) term(x[j], w[j0 + j]);
    }
    for (; j0 < ncols; ++j0) term(col[j0 * stride], w[j0]);           // the last block's odd tail
}

// ---- range --------------------------------------------------------------------------------------------------------------

// one column's value of one cell: contributes iff w != 0.0 and x is not NaN
__device__ __forceinline__ void range_term(double x, double w, double &n, double &mn, double &mx) {
    const bool in = w != 0.0 && x == x;
    n = in ? n + 1.0 : n;
    mn = (in && x < mn) ? x : mn;
    mx = (in && x > mx) ? x : mx;
}

__global__ void __launch_bounds__(kRangeLanes) range_partials_kernel(const EnsembleOrderArgs a) {
    const int v = blockIdx.z;
    const long long b = blockIdx.y;
    const int p = blockIdx.x * kRangeLanes + threadIdx.x;            // stored unit, < pitch / 2
    const int u = natural_unit_of(p, a.threads, (a.split_mask >> v) & 1u);
    if (2 * u >= a.nlat) return;                                     // padding: never read
    const long long stride = a.pitch / 2;                            // units per row
    const double2 *const col = reinterpret_cast<const double2 *>(a.row[v]) + b * kRangeBlock * stride + p;
    ConstDouble *const w = reinterpret_cast<ConstDouble *>(reinterpret_cast<uintptr_t>(a.w + b * kRangeBlock));
    const int ncols = min(kRangeBlock, a.ncol - (int)b * kRangeBlock);       // wave-uniform
    const double inf = __builtin_huge_val();
    double2 n = make_double2(0.0, 0.0), mn = make_double2(inf, inf), mx = make_double2(-inf, -inf);
    walk_columns(col, stride, w, ncols, [&](const double2 x, const double wc) {
        range_term(x.x, wc, n.x, mn.x, mx.x);
        range_term(x.y, wc, n.y, mn.y, mx.y);
    });
    double2 *const out = reinterpret_cast<double2 *>(a.partial + (b * a.nvars + v) * 3 * (long long)a.pitch) + p;
    out[0] = n;
    out[stride] = mn;
    out[2 * stride] = mx;
}

// blockIdx.y = entry * 3 + quantity (n, min, max).  Lane = one stored cell s = 2p + e of that row of partials: the shape of
// ensemble_finish_kernel, the loads of kOrderFinishBatch blocks ahead of the dependent combine.
__global__ void __launch_bounds__(kRangeLanes) range_finish_kernel(const EnsembleOrderArgs a) {
    const int vq = blockIdx.y, v = vq / 3, q = vq - 3 * v;
    const int s = blockIdx.x * kRangeLanes + threadIdx.x;            // stored cell, < pitch
    const int k = 2 * natural_unit_of(s >> 1, a.threads, (a.split_mask >> v) & 1u) + (s & 1);
    if (k >= a.nlat) return;
    const double *const part = a.partial + (long long)vq * a.pitch + s;
    const long long stride = 3LL * a.nvars * a.pitch;                // from block to block
    const double inf = __builtin_huge_val();
    double r = q == 0 ? 0.0 : q == 1 ? inf : -inf;
    const auto combine = [&](double x) {                             // ascending: the first of equal extremes stays
        r = q == 0 ? r + x : q == 1 ? (x < r ? x : r) : (x > r ? x : r);
    };
    int b = 0;
    for (; b + kOrderFinishBatch <= a.nblocks; b += kOrderFinishBatch) {
        double x[kOrderFinishBatch];
#pragma unroll
        for (int j = 0; j < kOrderFinishBatch; ++j) x[j] = part[(b + j) * stride];
#pragma unroll
        for (int j = 0; j < kOrderFinishBatch; ++j) combine(x[j]);
    }
    for (; b < a.nblocks; ++b) combine(part[b * stride]);
    a.out[(long long)vq * a.nlat + k] = r;
}

hipError_t launch_ensemble_range(const EnsembleOrderArgs &a, hipStream_t s) {
    const unsigned unit_tiles = (unsigned)(a.pitch / (2 * kRangeLanes)), cell_tiles = (unsigned)(a.pitch / kRangeLanes);
    range_partials_kernel<<<dim3(unit_tiles, (unsigned)a.nblocks, (unsigned)a.nvars), kRangeLanes, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    range_finish_kernel<<<dim3(cell_tiles, 3u * (unsigned)a.nvars), kRangeLanes, 0, s>>>(a);
    return hipGetLastError();
}

// ---- histogram ----------------------------------------------------------------------------------------------------------

// the slot of a value that is not NaN: 0 below lo, nbins + 1 at or above hi, else 1 + min((int)((x - lo) * s), nbins - 1)
__device__ __forceinline__ int slot_of(double x, double lo, double hi, double s, int nbins) {
    const bool below = x < lo, above = x >= hi;
    const double d = x - lo;
    const double t = d * s;
    const int i = (int)((below || above || x != x) ? 0.0 : t);       // converted only where 0 <= t <= nbins
    return below ? 0 : above ? nbins + 1 : 1 + min(i, nbins - 1);
}

__global__ void __launch_bounds__(kHistLanes) histogram_partials_kernel(const EnsembleOrderArgs a) {
    extern __shared__ double hist[];                                 // [nbins + 2][2][kHistLanes]
    const int v = blockIdx.z;
    const long long b = blockIdx.y;
    const int p = blockIdx.x * kHistLanes + threadIdx.x;             // stored unit, < pitch / 2
    const int u = natural_unit_of(p, a.threads, (a.split_mask >> v) & 1u);
    if (2 * u >= a.nlat) return;                                     // padding: never read (no barrier below)
    const long long stride = a.pitch / 2;                            // units per row
    const int nbins = a.nbins, nslots = nbins + 2;
    double *const mine0 = hist + threadIdx.x, *const mine1 = mine0 + kHistLanes;     // slot i of cell e: mine_e[i * 2 kHistLanes]
    for (int i = 0; i < nslots; ++i) {
        mine0[i * 2 * kHistLanes] = 0.0;
        mine1[i * 2 * kHistLanes] = 0.0;
    }
    const double2 *const edges = reinterpret_cast<const double2 *>(a.edges + 3LL * v * a.pitch) + u;
    const double2 lo = edges[0], hi = edges[stride], sc = edges[2 * stride];
    const double2 *const col = reinterpret_cast<const double2 *>(a.row[v]) + b * kHistBlock * stride + p;
    ConstDouble *const w = reinterpret_cast<ConstDouble *>(reinterpret_cast<uintptr_t>(a.w + b * kHistBlock));
    const int ncols = min(kHistBlock, a.ncol - (int)b * kHistBlock);         // wave-uniform
    walk_columns(col, stride, w, ncols, [&](const double2 x, const double wc) {
        double *const s0 = mine0 + slot_of(x.x, lo.x, hi.x, sc.x, nbins) * 2 * kHistLanes;
        double *const s1 = mine1 + slot_of(x.y, lo.y, hi.y, sc.y, nbins) * 2 * kHistLanes;
        const double h0 = *s0, h1 = *s1;                             // the two cells never share a word: both loads first
        const bool in0 = wc != 0.0 && x.x == x.x, in1 = wc != 0.0 && x.y == x.y;
        *s0 = in0 ? h0 + wc : h0;
        *s1 = in1 ? h1 + wc : h1;
    });
    double2 *const out = reinterpret_cast<double2 *>(a.partial + (b * a.nvars + v) * nslots * (long long)a.pitch) + p;
    for (int i = 0; i < nslots; ++i) out[i * stride] = make_double2(mine0[i * 2 * kHistLanes], mine1[i * 2 * kHistLanes]);
}

// blockIdx.y = slot, blockIdx.z = entry.  Lane = one stored cell s = 2p + e of the row of partials.
__global__ void __launch_bounds__(64) histogram_finish_kernel(const EnsembleOrderArgs a) {
    const int slot = blockIdx.y, v = blockIdx.z, nslots = a.nbins + 2;
    const int s = blockIdx.x * 64 + threadIdx.x;                     // stored cell, < pitch
    const int k = 2 * natural_unit_of(s >> 1, a.threads, (a.split_mask >> v) & 1u) + (s & 1);
    if (k >= a.nlat) return;
    const double *const part = a.partial + ((long long)v * nslots + slot) * a.pitch + s;
    const long long stride = (long long)nslots * a.nvars * a.pitch;  // from block to block
    double sum = 0.0;
    int b = 0;
    for (; b + kOrderFinishBatch <= a.nblocks; b += kOrderFinishBatch) {
        double x[kOrderFinishBatch];
#pragma unroll
        for (int j = 0; j < kOrderFinishBatch; ++j) x[j] = part[(b + j) * stride];
#pragma unroll
        for (int j = 0; j < kOrderFinishBatch; ++j) sum = sum + x[j];
    }
    for (; b < a.nblocks; ++b) sum = sum + part[b * stride];
    a.out[((long long)v * nslots + slot) * a.nlat + k] = sum;
}

hipError_t launch_ensemble_histogram(const EnsembleOrderArgs &a, hipStream_t s) {
    const unsigned unit_tiles = (unsigned)(a.pitch / (2 * kHistLanes)), cell_tiles = (unsigned)(a.pitch / 64);
    const unsigned nslots = (unsigned)a.nbins + 2u;
    const size_t lds = sizeof(double) * 2 * kHistLanes * nslots;
    if (lds > 48 * 1024) {                                           // beyond what a launch may ask for unannounced
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(histogram_partials_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 2 * kHistLanes * (kHistMaxBins + 2)));
        if (e != hipSuccess) return e;
    }
    histogram_partials_kernel<<<dim3(unit_tiles, (unsigned)a.nblocks, (unsigned)a.nvars), kHistLanes, lds, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    histogram_finish_kernel<<<dim3(cell_tiles, nslots, (unsigned)a.nvars), 64, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
