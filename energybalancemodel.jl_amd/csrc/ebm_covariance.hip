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
//              centred and NaN-cleaned; the next sixteen are loaded into registers before the MFMAs of these start.  Each of
//              the four waves owns 32 x 32 of the tile as 2 x 2 accumulators; per group of four columns it reads two A and
//              two B operands (lane & 15 the cell, lane >> 4 the column of the group) and issues four MFMAs.  LDS rows are
//              80 doubles: 160 words = 32 mod 64 banks, so the two rows that a half-wave reads fall on disjoint banks.
//              20 KiB of LDS.  The accumulators go to partial[block][stored i][stored j], each 16-lane group a whole line.
//   finish     grid (columns of out / 256) x (rows of out).  A lane owns one out[i][j], finds the stored cells of i and j,
//              adds the blocks in ascending order and writes the natural index — under rule 6 only for j >= i, and then
//              out[j][i] as well (that store has a stride of nlat doubles across a wave: uncoalesced).
// Rule 6 skips whole tiles and, inside a tile, a wave's whole 32 x 32 block, where the natural cells they stand for hold no
// pair with j >= i; a block that holds one is computed whole and its elements with j < i are never read.
// Every output element sees the same chain whichever tile, wave and register it falls in: acc = mfma(a[4], b[4], acc) over
// the groups of its block, ascending.  A tail group is padded with +0.0 terms; a group wholly past the block's last column
// is not issued.  Nothing else is contracted (-ffp-contract=off): d = x - center, a = w * d are rounded once each.
// Plain vector loads and stores; no scratch.
#include "ebm_internal.h"

namespace ebm {

constexpr int kCovTile = 64;                   // stored cells per side of a workgroup's tile; the pitch is a multiple of 128
constexpr int kCovLanes = 256;                 // four waves, 2 x 2 over the tile
constexpr int kCovChunk = 16;                  // columns in LDS together: two per lane and side
constexpr int kCovRow = kCovTile + 16;         // doubles per LDS row (see above)
constexpr int kCovFinishLanes = 256;
static_assert(kCovBlock % kCovChunk == 0 && kCovChunk % 4 == 0, "a block is whole chunks, a chunk whole MFMA groups");
static_assert(kCovLanes == 32 * (kCovChunk / 2) && kCovTile == 64, "the staging map: 32 units x 8 columns, twice");

typedef double cov_acc __attribute__((ext_vector_type(4)));

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
    const int p = tile * (kCovTile / 2) + (threadIdx.x & 31), u = natural_unit(p, a.threads, split);
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

__global__ void __launch_bounds__(kCovLanes) covariance_partials_kernel(const CovarianceArgs a) {
    __shared__ double sa[kCovChunk][kCovRow], sb[kCovChunk][kCovRow];
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

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;  // MFMA: the wave's 32 x 32 is at (r0, q0) of the tile
    const int r0 = (wave >> 1) * 32, q0 = (wave & 1) * 32, lk = lane >> 4, lc = lane & 15;
    natural_span(ti * 32 + r0 / 2, 16, a.threads, a.split_a, ilo, ihi);
    natural_span(tj * 32 + q0 / 2, 16, a.threads, a.split_b, jlo, jhi);
    const bool mine = ilo < a.nlat && jlo < a.nlat && !(a.symmetric && ilo > jhi);     // wave-uniform

    cov_acc acc[2][2];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = cov_acc{0.0, 0.0, 0.0, 0.0};

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
    for (int m0 = 0; m0 < ncols; m0 += kCovChunk) {
        __syncthreads();                                   // the MFMAs of the chunk before have read LDS
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<double2 *>(&sa[sm + 8 * h][2 * su]) =
                make_double2(cov_term<true>(xa[h].x, A.c.x, A.centered, wc[h], A.in0), cov_term<true>(xa[h].y, A.c.y, A.centered, wc[h], A.in1));
            *reinterpret_cast<double2 *>(&sb[sm + 8 * h][2 * su]) =
                make_double2(cov_term<false>(xb[h].x, B.c.x, B.centered, wc[h], B.in0), cov_term<false>(xb[h].y, B.c.y, B.centered, wc[h], B.in1));
        }
        __syncthreads();
        if (m0 + kCovChunk < ncols) load(m0 + kCovChunk);  // in flight under the MFMAs
        if (!mine) continue;
#pragma unroll
        for (int k0 = 0; k0 < kCovChunk; k0 += 4) {
            if (m0 + k0 >= ncols) break;                   // a group wholly past the last column is not part of the chain
            double av[2], bv[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                av[s] = sa[k0 + lk][r0 + 16 * s + lc];
                bv[s] = sb[k0 + lk][q0 + 16 * s + lc];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[t], acc[s][t], 0, 0, 0);
        }
    }
    if (!mine) return;
    // D of v_mfma_f64_16x16x4_f64: register g of a lane is row (lane >> 4) + 4 g, column lane & 15
    double *const part = a.partial + (blk * a.pitch + (ti * kCovTile + r0 + lk)) * a.pitch + tj * kCovTile + q0 + lc;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) part[(long long)(16 * s + 4 * g) * a.pitch + 16 * t] = acc[s][t][g];
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
    const unsigned tiles = (unsigned)(a.pitch / kCovTile);
    covariance_partials_kernel<<<dim3(tiles, tiles, (unsigned)a.nblocks), kCovLanes, 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    covariance_finish_kernel<<<dim3((unsigned)((a.nlat + kCovFinishLanes - 1) / kCovFinishLanes), (unsigned)a.nlat), kCovFinishLanes, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
