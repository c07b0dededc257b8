// ebm_ensemble_sums (include/ebm_hip.h): the weighted sums S0, S1, S2 ACROSS the columns of a handle, per variable and
// latitude — the column-wise partner of the hemispheric mean.  The summation order is part of the definition (blocks of
// kSumsBlock columns summed in ascending column order, the block partials then in ascending block order), so the work is
// two kernels and no atomics:
//   partials   grid (latitude tiles) x (column blocks) x (variables).  A lane owns one 16-byte unit of the row — the pair of
//              cells that is the unit of the pair-split permutation (split_index, ebm_internal.h) — and walks the columns of
//              its block at that unit: its accesses never depend on the layout, only the natural unit it stands for does
//              (stored unit p of a split row is natural unit 2p for p < T, 2(p - T) + 1 otherwise), which indexes `center`.
//              A wave reads 64 units = 1 KiB = eight whole 128-byte lines of a column per access; the loads of kSumsBatch
//              columns are issued before the first dependent add.  w is read once per column through the scalar cache (the
//              index is wave-uniform).  The three partials go to partial[block][variable][quantity][pitch] at the lane's
//              own stored index, whole lines again.
//   finish     a lane owns one stored cell of one (variable, quantity) and adds the block partials in ascending order, the
//              loads of kFinishBatch blocks ahead of the adds; the result goes to the natural index.
// Nothing is contracted (the library is built with -ffp-contract=off, as the noise recurrence of ebm_noise.h relies on):
// t1 = w*d and t2 = t1*d are rounded products, every add is a rounded sum.  Units whose first natural cell is at or beyond
// nlat are never loaded.  Plain vector loads and stores; no LDS, no scratch, no atomics.
#include "ebm_internal.h"

namespace ebm {

constexpr int kSumsLanes = 64;       // one wave per workgroup: a tile is 64 units = 128 cells; pitch is a multiple of that
constexpr int kSumsBatch = 16;       // columns whose loads are in flight together (16 KiB per wave)
constexpr int kFinishBatch = 32;     // block partials in flight together (8-byte loads)
static_assert(kSumsBlock % kSumsBatch == 0, "a block is a whole number of batches");

// natural index of stored index p (units of a row of 2T units, or cells of pairs: see finish) in a pair-split row
__device__ __forceinline__ int natural_unit(int p, int T, bool split) { return !split ? p : (p < T ? 2 * p : 2 * (p - T) + 1); }

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

__global__ void __launch_bounds__(kSumsLanes) ensemble_partials_kernel(const EnsembleSumsArgs a) {
    const int v = blockIdx.z;
    const long long b = blockIdx.y;
    const int p = blockIdx.x * kSumsLanes + threadIdx.x;             // stored unit, < pitch / 2
    const int u = natural_unit(p, a.threads, (a.split_mask >> v) & 1u);
    if (2 * u >= a.nlat) return;                                     // padding: never read
    const long long stride = a.pitch / 2;                            // units per row
    const double2 *const col = reinterpret_cast<const double2 *>(a.row[v]) + b * kSumsBlock * stride + p;
    typedef const __attribute__((address_space(4))) double ConstDouble;      // never written by a kernel: scalar loads
    ConstDouble *const w = reinterpret_cast<ConstDouble *>(reinterpret_cast<uintptr_t>(a.w + b * kSumsBlock));
    const bool centered = a.center != nullptr;
    const double2 c = centered ? reinterpret_cast<const double2 *>(a.center + (long long)v * a.pitch)[u] : make_double2(0.0, 0.0);
    const int ncols = min(kSumsBlock, a.ncol - (int)b * kSumsBlock);  // wave-uniform
    double2 s0 = make_double2(0.0, 0.0), s1 = s0, s2 = s0;
    int j0 = 0;
    for (; j0 + kSumsBatch <= ncols; j0 += kSumsBatch) {
        double2 x[kSumsBatch];
#pragma unroll
        for (int j = 0; j < kSumsBatch; ++j) x[j] = col[(j0 + j) * stride];
#pragma unroll
        for (int j = 0; j < kSumsBatch; ++j) {
            const double wc = w[j0 + j];
            add_term(x[j].x, c.x, centered, wc, s0.x, s1.x, s2.x);
            add_term(x[j].y, c.y, centered, wc, s0.y, s1.y, s2.y);
        }
    }
    for (; j0 < ncols; ++j0) {                                       // the last block's odd tail
        const double2 x = col[j0 * stride];
        const double wc = w[j0];
        add_term(x.x, c.x, centered, wc, s0.x, s1.x, s2.x);
        add_term(x.y, c.y, centered, wc, s0.y, s1.y, s2.y);
    }
    double2 *const out = reinterpret_cast<double2 *>(a.partial + (b * a.nvars + v) * 3 * (long long)a.pitch) + p;
    out[0] = s0;
    out[stride] = s1;
    out[2 * stride] = s2;
}

// blockIdx.y = variable * 3 + quantity.  Lane = one stored cell s = 2p + e of the row of partials.
__global__ void __launch_bounds__(kSumsLanes) ensemble_finish_kernel(const EnsembleSumsArgs a) {
    const int vq = blockIdx.y, v = vq / 3;
    const int s = blockIdx.x * kSumsLanes + threadIdx.x;             // stored cell, < pitch
    const int k = 2 * natural_unit(s >> 1, a.threads, (a.split_mask >> v) & 1u) + (s & 1);
    if (k >= a.nlat) return;
    const double *const part = a.partial + (long long)vq * a.pitch + s;
    const long long stride = 3LL * a.nvars * a.pitch;                // from block to block
    double sum = 0.0;
    int b = 0;
    for (; b + kFinishBatch <= a.nblocks; b += kFinishBatch) {
        double x[kFinishBatch];
#pragma unroll
        for (int j = 0; j < kFinishBatch; ++j) x[j] = part[(b + j) * stride];
#pragma unroll
        for (int j = 0; j < kFinishBatch; ++j) sum = sum + x[j];
    }
    for (; b < a.nblocks; ++b) sum = sum + part[b * stride];
    a.out[(long long)vq * a.nlat + k] = sum;
}

hipError_t launch_ensemble_sums(const EnsembleSumsArgs &a, hipStream_t s) {
    const unsigned unit_tiles = (unsigned)(a.pitch / (2 * kSumsLanes)), cell_tiles = (unsigned)(a.pitch / kSumsLanes);
    ensemble_partials_kernel<<<dim3(unit_tiles, (unsigned)a.nblocks, (unsigned)a.nvars), kSumsLanes, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ensemble_finish_kernel<<<dim3(cell_tiles, 3u * (unsigned)a.nvars), kSumsLanes, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
