// ebm_spd_solve_device and ebm_kalman_gain_device (include/ebm_hip.h): X . S = B for a symmetric positive definite S — the
// middle of an ensemble Kalman filter, between ebm_covariance.hip and ebm_update.hip, on v_mfma_f64_16x16x4_f64.  Everything
// works on mp = m rounded up to kGainBlock = 64 with the identity in the padding of S and +0.0 in the padding of B, so no
// kernel of the factorisation or of the solve has a tail, and the padding never reaches a result.  T = mp / 64 block columns.
//   assemble   one lane per element.  S[a][b] = (rho * Poo[J[a]][J[b]]) * factor + (a == b ? R[J[a]] : 0.0);
//              B[v * nlat + k][a] = (factor * rho) * Pfo_v[k][J[a]], a non-finite Pfo as +0.0; rho = the Gaspari-Cohn taper
//              of |x_k - x_j| / localize in the expression order of ensemble.py's gaspari_cohn, exactly 1.0 without one.
//   factor     right-looking blocked Cholesky, per block column k three launches:
//              diagonal  one workgroup, the 64 x 64 block in LDS ([64][65]: a lane per row, no bank conflicts).  Column j:
//                        s = sqrt(a[j][j]); a[i][j] = a[i][j] / s for i > j; a[i][c] = a[i][c] - a[i][j] * a[c][j] for
//                        j < c <= i; two barriers per column, reached by every lane whatever the pivot is.  The first pivot
//                        that is not > 0 (a NaN is not) writes its 1-based index to the flag.  Then the inverse W of L_kk,
//                        lane c its column c by forward substitution: W[i][c] = ((i == c) - sum_{c <= j < i} L[i][j] * W[j][c])
//                        / L[i][i], j ascending, every term subtracted as it comes; to inv[k].
//              panel     a workgroup per tile i > k: A_ik = A_ik . W^T.
//              trailing  a workgroup per tile i >= j > k: A_ij = A_ij - L_ik . L_jk^T, one subtraction after the chain.  Only
//                        tiles of the lower triangle are read or written (a diagonal tile whole).
//   solve      two launches, a workgroup per 64 rows of B (rows at or beyond nrhs are staged as +0.0 and never written).
//              forward   block columns k ascending:  W = B_k - sum_{t < 64 k} Y[.][t] * L[64 k + c][t];  Y_k = W . inv[k]^T
//              backward  block columns k descending: W = Y_k - sum_{t >= 64 (k + 1)} X[.][t] * L[t][64 k + c];  X_k = W . inv[k]
//              W and then the result are written to B in place; a workgroup re-reads only what it wrote itself, behind a
//              block-level fence and a barrier.
//   scatter    one lane per element of the gain: gain[v][k][j] = X[v * nlat + k][pos[j]], +0.0 where cell j is unobserved.
// Every product above is ONE chain per element (ebm_mfma_tile.h, which owns the tile, the operands and the accumulators)
// whichever tile, wave and register it falls in, over the groups t = 0, 4, 8, ... of the contraction.  Both factors are
// staged line-major, sixteen t at a time, the next sixteen loaded before the MFMAs of these start.  Nothing else is contracted
// (-ffp-contract=off).  A launch that finds the flag set does nothing.  Plain vector loads and stores, no atomics, no scratch.
#include "ebm_internal.h"
#include "ebm_mfma_tile.h"

namespace ebm {

constexpr int kGainLanes = kTileLanes;         // of every kernel here: a block of the factorisation is a tile
constexpr int kGainTileWords = kGainBlock * kGainBlock;
static_assert(kGainBlock == kTileSide && kTileLanes == 4 * kTileSide && kTileChunk == 16, "the staging map: 64 lines x 4 quads of four t");

// acc[r][c] += sum_{t < nk} X[r][t] * (TB ? Y[t][c] : Y[c][t]), r, c < 64, nk a multiple of 16; rows r >= xrows of X are +0.0
// and not loaded.  Every global load of the call has landed in LDS before its last barrier.
template <bool TB>
__device__ __forceinline__ void tile_product(tile_acc (&acc)[2][2], tile_line_major *sx, tile_line_major *sy, const double *X, long long ldx,
                                             int xrows, const double *Y, long long ldy, int nk) {
    const int sl = threadIdx.x >> 2, sq = threadIdx.x & 3;           // staging: line sl, four t from 4 sq
    const int tl = threadIdx.x >> 4, c4 = 4 * (threadIdx.x & 15);    // ... of a transposed Y: row tl of the chunk, four c from c4
    const bool xin = sl < xrows;
    const double *const xp = X + (long long)(xin ? sl : 0) * ldx + 4 * sq;
    const double *const yp = TB ? Y + (long long)tl * ldy + c4 : Y + (long long)sl * ldy + 4 * sq;
    double xv[4], yv[4];
    auto load = [&](int t0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            xv[i] = xin ? xp[t0 + i] : 0.0;
            yv[i] = TB ? yp[(long long)t0 * ldy + i] : yp[t0 + i];
        }
    };
    if (nk > 0) load(0);                                   // nk == 0: nothing behind X or Y may be touched
    for (int t0 = 0; t0 < nk; t0 += kTileChunk) {
        __syncthreads();                                   // the MFMAs of the chunk before have read LDS
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sx[sl][4 * sq + i] = xv[i];
            if (TB) sy[c4 + i][tl] = yv[i];
            else sy[sl][4 * sq + i] = yv[i];
        }
        __syncthreads();
        if (t0 + kTileChunk < nk) load(t0 + kTileChunk);   // in flight under the MFMAs
        tile_mfma(acc, sx, sy, kTileChunk / 4);
    }
}

// ---- factor -----------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(kGainLanes) spd_diagonal_kernel(const SolveArgs a, const int k) {
    __shared__ double l[kGainBlock][kGainBlock + 1];
    __shared__ double w[kGainBlock * (kGainBlock + 1) / 2];          // W[i][c], c <= i, at i (i + 1) / 2 + c
    const int stop = *a.flag;                                        // read before the first barrier, written after it
    if (stop) return;
    const int tid = threadIdx.x, k0 = k * kGainBlock;
    double *const tile = a.S + (long long)k0 * a.lds + k0;
    for (int e = tid; e < kGainTileWords; e += kGainLanes) {
        const int i = e >> 6, j = e & 63;
        if (j <= i) l[i][j] = tile[(long long)i * a.lds + j];
    }
    __syncthreads();
    const int row = tid & 63, quarter = tid >> 6;
    bool failed = false;
    for (int j = 0; j < kGainBlock; ++j) {
        const double d = l[j][j];
        if (!(d > 0.0) && !failed) {                                 // uniform: every lane reads the same pivot
            failed = true;
            if (tid == 0) *a.flag = k0 + j + 1;
        }
        const double s = sqrt(d);
        if (quarter == 0 && row > j) l[row][j] = l[row][j] / s;
        __syncthreads();
        const double lij = l[row][j];
        for (int c = j + 1 + quarter; c <= row; c += 4) l[row][c] = l[row][c] - lij * l[c][j];
        if (tid == j) l[j][j] = s;
        __syncthreads();
    }
    for (int e = tid; e < kGainTileWords; e += kGainLanes) {
        const int i = e >> 6, j = e & 63;
        if (j <= i) tile[(long long)i * a.lds + j] = l[i][j];
    }
    if (tid < kGainBlock) {                                          // one wave: lane c owns column c of W, rows c ... 63
        const int c = tid;
        for (int i = c; i < kGainBlock; ++i) {
            double sum = i == c ? 1.0 : 0.0;
#pragma unroll 8
            for (int j = c; j < i; ++j) sum = sum - l[i][j] * w[j * (j + 1) / 2 + c];
            w[i * (i + 1) / 2 + c] = sum / l[i][i];
        }
    }
    __syncthreads();
    double *const inv = a.inv + (long long)k * kGainTileWords;
    for (int e = tid; e < kGainTileWords; e += kGainLanes) {
        const int i = e >> 6, c = e & 63;
        inv[e] = c <= i ? w[i * (i + 1) / 2 + c] : 0.0;
    }
}

__global__ void __launch_bounds__(kGainLanes) spd_panel_kernel(const SolveArgs a, const int k) {
    __shared__ tile_line_major sx[kTileSide], sy[kTileSide];
    if (*a.flag) return;
    const int i = k + 1 + blockIdx.x;
    double *const tile = a.S + (long long)i * kGainBlock * a.lds + k * kGainBlock;
    tile_acc acc[2][2];
    tile_clear(acc);
    tile_product<false>(acc, sx, sy, tile, a.lds, kGainBlock, a.inv + (long long)k * kGainTileWords, kGainBlock, kGainBlock);
    for_each_element(acc, [&](int r, int c, double v) { tile[(long long)r * a.lds + c] = v; });
}

__global__ void __launch_bounds__(kGainLanes) spd_trailing_kernel(const SolveArgs a, const int k) {
    __shared__ tile_line_major sx[kTileSide], sy[kTileSide];
    const int j = k + 1 + blockIdx.x, i = k + 1 + blockIdx.y;
    if (j > i || *a.flag) return;                                    // the lower triangle only
    const double *const li = a.S + (long long)i * kGainBlock * a.lds + k * kGainBlock;
    const double *const lj = a.S + (long long)j * kGainBlock * a.lds + k * kGainBlock;
    double *const tile = a.S + (long long)i * kGainBlock * a.lds + j * kGainBlock;
    tile_acc acc[2][2];
    tile_clear(acc);
    tile_product<false>(acc, sx, sy, li, a.lds, kGainBlock, lj, a.lds, kGainBlock);
    for_each_element(acc, [&](int r, int c, double v) {
        double *const p = tile + (long long)r * a.lds + c;
        *p = *p - v;
    });
}

// ---- solve ------------------------------------------------------------------------------------------------------------------

template <bool BACKWARD>
__global__ void __launch_bounds__(kGainLanes) spd_solve_kernel(const SolveArgs a) {
    __shared__ tile_line_major sx[kTileSide], sy[kTileSide];
    if (*a.flag) return;
    const long long row0 = (long long)blockIdx.x * kGainBlock;
    const int xrows = (int)(a.nrhs - row0 < kGainBlock ? a.nrhs - row0 : kGainBlock), T = a.mp / kGainBlock;
    double *const rows = a.B + row0 * a.ldb;
    for (int step = 0; step < T; ++step) {
        const int k = BACKWARD ? T - 1 - step : step, k0 = k * kGainBlock;
        tile_acc acc[2][2];
        tile_clear(acc);
        if (BACKWARD)       // the block columns behind k, already X, times the tiles of L below the diagonal one: L[t][k0 + c]
            tile_product<true>(acc, sx, sy, rows + k0 + kGainBlock, a.ldb, xrows, a.S + (long long)(k0 + kGainBlock) * a.lds + k0, a.lds,
                               a.mp - k0 - kGainBlock);
        else                // the block columns before k, already Y, times the tiles of L left of the diagonal one: L[k0 + c][t]
            tile_product<false>(acc, sx, sy, rows, a.ldb, xrows, a.S + (long long)k0 * a.lds, a.lds, k0);
        for_each_element(acc, [&](int r, int c, double v) {
            if (r >= xrows) return;
            double *const p = rows + (long long)r * a.ldb + k0 + c;
            *p = *p - v;
        });
        __threadfence_block();                             // W is read back by other lanes of this workgroup
        __syncthreads();
        tile_clear(acc);
        tile_product<BACKWARD>(acc, sx, sy, rows + k0, a.ldb, xrows, a.inv + (long long)k * kGainTileWords, kGainBlock, kGainBlock);
        for_each_element(acc, [&](int r, int c, double v) {
            if (r < xrows) rows[(long long)r * a.ldb + k0 + c] = v;
        });
        __threadfence_block();                             // ... and so is the solved block column, by the next step
        __syncthreads();
    }
}

// ---- assemble and scatter ---------------------------------------------------------------------------------------------------

// gaspari_cohn of ensemble.py, one operation per rounding in its order; 1.0 without localisation
__device__ __forceinline__ double taper(double xk, double xj, double localize) {
    if (!(localize > 0.0)) return 1.0;
    const double r = fabs(fabs(xk - xj) / localize);
    double out = 0.0;
    if (r <= 1.0) out = (((-0.25 * r + 0.5) * r + 0.625) * r - 5.0 / 3.0) * (r * r) + 1.0;
    else if (r < 2.0) out = (((r / 12.0 - 0.5) * r + 0.625) * r + 5.0 / 3.0) * (r * r) - 5.0 * r + 4.0 - 2.0 / (3.0 * r);
    out = out < 0.0 ? 0.0 : out;
    return out > 1.0 ? 1.0 : out;
}

__global__ void __launch_bounds__(kGainLanes) gain_assemble_system_kernel(const GainArgs g) {
    const int b = blockIdx.x * kGainLanes + threadIdx.x, a = blockIdx.y;
    if (b >= g.mp) return;
    double v = a == b ? 1.0 : 0.0;                                   // the padding: the identity
    if (a < g.m && b < g.m) {
        const int ja = g.index[a], jb = g.index[b];
        const double rho = taper(g.x[ja], g.x[jb], g.localize);
        v = (rho * g.Poo[(long long)ja * g.nlat + jb]) * g.factor + (a == b ? g.obs_var[ja] : 0.0);
    }
    g.S[(long long)a * g.mp + b] = v;
}

__global__ void __launch_bounds__(kGainLanes) gain_assemble_rhs_kernel(const GainArgs g) {
    const int a = blockIdx.x * kGainLanes + threadIdx.x, k = blockIdx.y, f = blockIdx.z;
    if (a >= g.mp) return;
    double v = 0.0;
    if (a < g.m) {
        const int ja = g.index[a];
        const double p = g.Pfo[f][(long long)k * g.nlat + ja];
        v = (g.factor * taper(g.x[k], g.x[ja], g.localize)) * (isfinite(p) ? p : 0.0);
    }
    g.B[((long long)f * g.nlat + k) * g.mp + a] = v;
}

__global__ void __launch_bounds__(kGainLanes) gain_scatter_kernel(const GainArgs g) {
    const int j = blockIdx.x * kGainLanes + threadIdx.x, k = blockIdx.y, f = blockIdx.z;
    if (j >= g.nlat || *g.flag) return;
    const int a = g.pos[j];
    const long long row = (long long)f * g.nlat + k;
    g.gain[row * g.nlat + j] = a >= 0 ? g.B[row * g.mp + a] : 0.0;
}

// ---- launchers --------------------------------------------------------------------------------------------------------------

hipError_t launch_spd_factor(const SolveArgs &a, hipStream_t s) {
    const int T = a.mp / kGainBlock;
    for (int k = 0; k < T; ++k) {
        spd_diagonal_kernel<<<1, kGainLanes, 0, s>>>(a, k);
        const unsigned below = (unsigned)(T - k - 1);
        if (below) {
            spd_panel_kernel<<<below, kGainLanes, 0, s>>>(a, k);
            spd_trailing_kernel<<<dim3(below, below), kGainLanes, 0, s>>>(a, k);
        }
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_spd_solve(const SolveArgs &a, hipStream_t s) {
    if (a.nrhs < 1) return hipSuccess;
    const unsigned groups = (unsigned)((a.nrhs + kGainBlock - 1) / kGainBlock);
    spd_solve_kernel<false><<<groups, kGainLanes, 0, s>>>(a);
    spd_solve_kernel<true><<<groups, kGainLanes, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_gain_assemble(const GainArgs &g, hipStream_t s) {
    const unsigned across = (unsigned)((g.mp + kGainLanes - 1) / kGainLanes);
    gain_assemble_system_kernel<<<dim3(across, (unsigned)g.mp), kGainLanes, 0, s>>>(g);
    gain_assemble_rhs_kernel<<<dim3(across, (unsigned)g.nlat, (unsigned)g.nvars), kGainLanes, 0, s>>>(g);
    return hipGetLastError();
}

hipError_t launch_gain_scatter(const GainArgs &g, hipStream_t s) {
    gain_scatter_kernel<<<dim3((unsigned)((g.nlat + kGainLanes - 1) / kGainLanes), (unsigned)g.nlat, (unsigned)g.nvars), kGainLanes, 0, s>>>(g);
    return hipGetLastError();
}

}  // namespace ebm
