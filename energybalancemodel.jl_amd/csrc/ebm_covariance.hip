// ebm_ensemble_covariance (include/ebm_hip.h): the covariance ACROSS the columns of a handle for every PAIR of latitudes,
// out[i][j] = sum_c a_c(i) * b_c(j) — the one dense contraction of the library, on v_mfma_f64_16x16x4_f64.  The order of the
// operations is part of the definition (blocks of kCovBlock columns; inside a block one MFMA per four columns, ascending;
// the block partials then in ascending block order), so the reduction is two kernels and no atomics, as in ebm_ensemble.hip:
//   partials   grid (tiles of row_b) x (tiles of row_a) x (column blocks), 256 lanes.  A workgroup owns 64 STORED cells of
//              row_a times 64 STORED cells of row_b: its accesses never depend on the layout, only the natural cells its tile
//              stands for do (stored unit p of a split row is natural unit 2p for p < T, 2(p - T) + 1 otherwise), which index
//              the centers, bound the padding and decide what rule 6 skips.  The columns of the block pass through LDS
//              sixteen at a time: lane (unit u = lane & 31, column lane >> 5) loads 16 bytes of each row, a wave two whole
//              512-byte runs of four lines; the A side is centred, weighted and NaN-cleaned on its way into LDS, the B side
//              centred and NaN-cleaned; the next sixteen are loaded into registers before the MFMAs of these start.  Both
//              sides are staged k-major (ebm_mfma_tile.h, which owns the tile, the operands and the accumulators): 20 KiB of
//              LDS.  The accumulators go to partial[block][stored i][stored j], each 16-lane group a whole line.
//   finish     grid (columns of out / 256) x (rows of out).  A lane owns one out[i][j], finds the stored cells of i and j,
//              adds the blocks in ascending order and writes the natural index — under rule 6 only for j >= i, and then
//              out[j][i] as well (that store has a stride of nlat doubles across a wave: uncoalesced).
// Rule 6 skips whole tiles and, inside a tile, a wave's whole 32 x 32 block, where the natural cells they stand for hold no
// pair with j >= i; a block that holds one is computed whole and its elements with j < i are never read.
// Every output element sees the same chain (ebm_mfma_tile.h) whichever tile, wave and register it falls in, over the groups
// of four columns of its block.  A tail group is padded with +0.0 terms; a group wholly past the block's last column
// is not issued.  Nothing else is contracted (-ffp-contract=off): d = x - center, a = w * d are rounded once each.
// Plain vector loads and stores; no scratch.
#include "ebm_internal.h"
#include "ebm_mfma_tile.h"

namespace ebm {

constexpr int kCovFinishLanes = 256;
static_assert(kCovBlock % kTileChunk == 0, "a block is whole chunks");
static_assert(kTileLanes == 32 * (kTileChunk / 2) && kTileSide == 64, "the staging map: 32 units x 8 columns, twice");

// the natural cells [lo, hi] that the stored units first ... first + n - 1 of a row stand for (n <= 32 divides T: a run never
// straddles the two halves of a split row, and natural_unit ascends along it)
__device__ __forceinline__ void natural_span(int first, int n, int T, bool split, int &lo, int &hi) {
    lo = 2 * natural_unit(first, T, split);
    hi = 2 * natural_unit(first + n - 1, T, split) + 1;
}

// what a lane stages of one side: its 16 bytes of two columns of the chunk
struct CovStage {
    const double2 *col;              // the lane's unit of the block's first column
    double2 c;                       // the centers of its two cells (0.0: none)
    bool centered, in0, in1;         // in*: the cell is below nlat (else padding: staged as +0.0)
};
__device__ __forceinline__ CovStage open_stage(const double *row, const double *center, bool split, int tile, long long c0,
                                               const CovarianceArgs &a) {
    CovStage s;
    const int p = tile * (kTileSide / 2) + (threadIdx.x & 31), u = natural_unit(p, a.threads, split);
    s.col = reinterpret_cast<const double2 *>(row) + c0 * (a.pitch / 2) + p;
    s.centered = center != nullptr;
    s.c = s.centered ? reinterpret_cast<const double2 *>(center)[u] : make_double2(0.0, 0.0);
    s.in0 = 2 * u < a.nlat;
    s.in1 = 2 * u + 1 < a.nlat;
    return s;
}
// one cell of a side as the MFMA takes it: (w *) (x - center), +0.0 for w == 0.0, a NaN cell or padding
template <bool WEIGHTED>
__device__ __forceinline__ double cov_term(double x, double c, bool centered, double w, bool in) {
    const double d = centered ? x - c : x;
    const double t = WEIGHTED ? w * d : d;
    return (in && w != 0.0 && x == x) ? t : 0.0;
}

__global__ void __launch_bounds__(kTileLanes) covariance_partials_kernel(const CovarianceArgs a) {
    __shared__ tile_k_major sa[kTileChunk], sb[kTileChunk];
    const int tj = blockIdx.x, ti = blockIdx.y;
    const long long blk = blockIdx.z;
    int ilo, ihi, jlo, jhi;
    natural_span(ti * 32, 32, a.threads, a.split_a, ilo, ihi);
    natural_span(tj * 32, 32, a.threads, a.split_b, jlo, jhi);
    if (ilo >= a.nlat || jlo >= a.nlat) return;            // padding only
    if (a.symmetric && ilo > jhi) return;                  // rule 6: no element with j >= i

    const long long c0 = blk * kCovBlock, stride = a.pitch / 2;
    const int ncols = min(kCovBlock, a.ncol - (int)c0);
    const CovStage A = open_stage(a.row_a, a.center_a, a.split_a, ti, c0, a), B = open_stage(a.row_b, a.center_b, a.split_b, tj, c0, a);
    const int su = threadIdx.x & 31, sm = threadIdx.x >> 5;      // staging: the unit of the tile, the column of a half chunk

    const int r0 = tile_lane(threadIdx.x).r0, q0 = tile_lane(threadIdx.x).q0;    // the wave's 32 x 32 of the tile
    natural_span(ti * 32 + r0 / 2, 16, a.threads, a.split_a, ilo, ihi);
    natural_span(tj * 32 + q0 / 2, 16, a.threads, a.split_b, jlo, jhi);
    const bool mine = ilo < a.nlat && jlo < a.nlat && !(a.symmetric && ilo > jhi);     // wave-uniform

    tile_acc acc[2][2];
    tile_clear(acc);

    double2 xa[2], xb[2];
    double wc[2];
    auto load = [&](int m0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int m = m0 + sm + 8 * h;
            const bool in = m < ncols;                     // a column past the block's last: a zero term
            wc[h] = in ? a.w[c0 + m] : 0.0;
            xa[h] = in ? A.col[m * stride] : make_double2(0.0, 0.0);
            xb[h] = in ? B.col[m * stride] : make_double2(0.0, 0.0);
        }
    };
    load(0);
    for (int m0 = 0; m0 < ncols; m0 += kTileChunk) {
        __syncthreads();                                   // the MFMAs of the chunk before have read LDS
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<double2 *>(&sa[sm + 8 * h][2 * su]) =
                make_double2(cov_term<true>(xa[h].x, A.c.x, A.centered, wc[h], A.in0), cov_term<true>(xa[h].y, A.c.y, A.centered, wc[h], A.in1));
            *reinterpret_cast<double2 *>(&sb[sm + 8 * h][2 * su]) =
                make_double2(cov_term<false>(xb[h].x, B.c.x, B.centered, wc[h], B.in0), cov_term<false>(xb[h].y, B.c.y, B.centered, wc[h], B.in1));
        }
        __syncthreads();
        if (m0 + kTileChunk < ncols) load(m0 + kTileChunk);  // in flight under the MFMAs
        if (mine) tile_mfma(acc, sa, sb, (ncols - m0 + 3) / 4);      // a group wholly past the last column is not issued
    }
    if (!mine) return;
    double *const part = a.partial + (blk * a.pitch + ti * kTileSide) * a.pitch + tj * kTileSide;
    for_each_element(acc, [&](int r, int c, double v) { part[(long long)r * a.pitch + c] = v; });
}

// the stored cell of natural cell k of a row
__device__ __forceinline__ int stored_cell(int k, int T, bool split) {
    const int u = k >> 1;
    return 2 * (split ? (u & 1) * T + (u >> 1) : u) + (k & 1);
}

__global__ void __launch_bounds__(kCovFinishLanes) covariance_finish_kernel(const CovarianceArgs a) {
    const int j = blockIdx.x * kCovFinishLanes + threadIdx.x, i = blockIdx.y;
    if (j >= a.nlat || (a.symmetric && j < i)) return;
    const long long stride = (long long)a.pitch * a.pitch;                 // from block to block
    const double *const part = a.partial + (long long)stored_cell(i, a.threads, a.split_a) * a.pitch + stored_cell(j, a.threads, a.split_b);
    double r = part[0];                                                    // one block: a copy
#pragma unroll 8
    for (int b = 1; b < a.nblocks; ++b) r = r + part[b * stride];
    a.out[(long long)i * a.nlat + j] = r;
    if (a.symmetric && j != i) a.out[(long long)j * a.nlat + i] = r;
}

hipError_t launch_ensemble_covariance(const CovarianceArgs &a, hipStream_t s) {
    const unsigned tiles = (unsigned)(a.pitch / kTileSide);
    covariance_partials_kernel<<<dim3(tiles, tiles, (unsigned)a.nblocks), kTileLanes, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    covariance_finish_kernel<<<dim3((unsigned)((a.nlat + kCovFinishLanes - 1) / kCovFinishLanes), (unsigned)a.nlat), kCovFinishLanes, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
