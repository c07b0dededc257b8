// ebm_update_columns (include/ebm_hip.h): every member moved by a linear map of its own innovation,
// x_f[c][k] += sum_j G_f[k][j] * d[c][j] — the second dense contraction of the library, an (ncol x nlat) . (nlat x nlat)
// product per state field on v_mfma_f64_16x16x4_f64, next to ebm_covariance.hip.  There is no split of the j axis, so there
// are no partials and no atomics: two kernels, the second one writing the state.
//   innovations  grid (columns x unit tiles), 64 lanes.  A lane owns one 16-byte unit of the row of obs_field, read where
//                it lies; the natural unit it stands for (natural_unit, ebm_internal.h) indexes target, dev_perturb and the
//                staged d[c][pitch], which is in NATURAL order with +0.0 in every cell at or beyond nlat.  All innovations are
//                staged before the product kernel writes a field, so obs_field may be one of the fields.
//   product      grid (tiles of stored cells) x (member tiles) x (fields), 256 lanes.  A workgroup owns 64 members times 64
//                STORED cells of one field: its accesses to the field never depend on the layout, only the natural cells its
//                tile stands for do, which pick the rows of the gain and bound the padding.  The observation cells pass
//                through LDS sixteen at a time: lane (quad q = lane & 3, line lane >> 2) loads 32 bytes of d of one member
//                and four gain entries of one state cell, four lanes a whole 128-byte line; the next sixteen are loaded into
//                registers before the MFMAs of these start.  Both sides are staged line-major (ebm_mfma_tile.h, which owns
//                the tile, the operands and the accumulators), d as the left factor: 9 KiB of LDS.  Then the add, the clamp
//                and the store: the sixteen lanes that share a row of the tile write one whole line of a row of the field.
// Every (c, k) sees the same chain (ebm_mfma_tile.h) whichever tile, wave and register it falls in, over the groups
// j = 0, 4, 8, ... < nlat.  A tail group is padded with +0.0 terms on both sides; a group wholly past nlat is not issued.
// Nothing else is contracted (-ffp-contract=off): s = scale * xo, t = target + e, d = t - s and x + acc are rounded once
// each.  Cells at or beyond nlat of a row, and rows at or beyond ncol, are never written.  Plain vector loads and stores; no
// scratch.
#include "ebm_internal.h"
#include "ebm_mfma_tile.h"

namespace ebm {

constexpr int kInnovLanes = 64;                // units per workgroup of the innovations: 128 cells, which the pitch is a multiple of
static_assert(kTileLanes == 4 * kTileSide && kTileChunk == 16, "the staging map: 64 lines x 4 quads of four cells");

// one innovation: +0.0 for no observation (a NaN target), a NaN cell of obs_field or padding
__device__ __forceinline__ double innovation(double xo, double y, double e, bool perturbed, double scale, bool in) {
    const double s = scale * xo;
    const double t = perturbed ? y + e : y;
    const double d = t - s;
    return (in && y == y && xo == xo) ? d : 0.0;
}

__global__ void __launch_bounds__(kInnovLanes) update_innovations_kernel(const UpdateArgs a) {
    const int tiles = a.pitch / (2 * kInnovLanes), c = blockIdx.x / tiles;         // column
    const int p = (blockIdx.x - c * tiles) * kInnovLanes + threadIdx.x;            // stored unit < pitch / 2
    const int u = natural_unit(p, a.threads, a.obs_split), k = 2 * u;
    const bool in0 = k < a.nlat, in1 = k + 1 < a.nlat;
    double2 *const out = reinterpret_cast<double2 *>(a.d + (long long)c * a.pitch) + u;
    if (!in0) {                                                                     // padding: never loaded
        *out = make_double2(0.0, 0.0);
        return;
    }
    const double2 xo = (reinterpret_cast<const double2 *>(a.obs) + (long long)c * (a.pitch / 2))[p];
    const double y0 = a.target[k], y1 = in1 ? a.target[k + 1] : 0.0;
    const bool perturbed = a.perturb != nullptr;
    const double *const e = a.perturb + (long long)c * a.nlat + k;                  // packed rows: 8-byte loads
    const double e0 = perturbed ? e[0] : 0.0, e1 = (perturbed && in1) ? e[1] : 0.0;
    *out = make_double2(innovation(xo.x, y0, e0, perturbed, a.scale, true), innovation(xo.y, y1, e1, perturbed, a.scale, in1));
}

// the first natural cell that a run of stored units beginning at `first` stands for (a run of <= 32 units never straddles the
// two halves of a split row, and natural_unit ascends along it: the run is padding iff this cell is)
__device__ __forceinline__ int first_natural_cell(int first, int T, bool split) { return 2 * natural_unit(first, T, split); }

__global__ void __launch_bounds__(kTileLanes) update_product_kernel(const UpdateArgs a) {
    __shared__ tile_line_major sd[kTileSide], sg[kTileSide];
    const int tk = blockIdx.x, tc = blockIdx.y, v = blockIdx.z;
    const bool split = (a.split_mask >> v) & 1u;
    if (first_natural_cell(tk * (kTileSide / 2), a.threads, split) >= a.nlat) return;       // padding only (natural cells ascend)

    // staging: line sl of the tile — member c0 + sl of d, stored cell s0 + sl of the field — and four cells 4 sq ... of the chunk
    const int sl = threadIdx.x >> 2, sq = threadIdx.x & 3;
    const int c0 = tc * kTileSide, s0 = tk * kTileSide;
    const bool member_in = c0 + sl < a.ncol;
    const double2 *const drow = reinterpret_cast<const double2 *>(a.d + (long long)(member_in ? c0 + sl : 0) * a.pitch) + 2 * sq;
    const int ks = 2 * natural_unit((s0 + sl) >> 1, a.threads, split) + (sl & 1);          // the natural cell of the staged gain row
    const bool cell_in = ks < a.nlat;
    const double *const grow = a.gain + (long long)v * a.gain_field + (long long)(cell_in ? ks : 0) * a.gain_row + 4 * sq;

    const int r0 = tile_lane(threadIdx.x).r0, q0 = tile_lane(threadIdx.x).q0;      // the wave's 32 x 32 of the tile
    const bool mine = c0 + r0 < a.ncol && first_natural_cell((s0 + q0) / 2, a.threads, split) < a.nlat;      // wave-uniform

    tile_acc acc[2][2];
    tile_clear(acc);

    double2 xd[2];
    double xg[4];
    auto load = [&](int j0) {
        // d: the staged rows are pitch long with +0.0 beyond nlat, and j0 + 16 <= pitch
        xd[0] = member_in ? drow[j0 / 2] : make_double2(0.0, 0.0);
        xd[1] = member_in ? drow[j0 / 2 + 1] : make_double2(0.0, 0.0);
#pragma unroll
        for (int i = 0; i < 4; ++i) xg[i] = (cell_in && j0 + 4 * sq + i < a.nlat) ? grow[j0 + i] : 0.0;    // the j-tail: +0.0 terms
    };
    load(0);
    for (int j0 = 0; j0 < a.nlat; j0 += kTileChunk) {
        __syncthreads();                                   // the MFMAs of the chunk before have read LDS
        *reinterpret_cast<double2 *>(&sd[sl][4 * sq]) = xd[0];
        *reinterpret_cast<double2 *>(&sd[sl][4 * sq + 2]) = xd[1];
        *reinterpret_cast<double2 *>(&sg[sl][4 * sq]) = make_double2(xg[0], xg[1]);
        *reinterpret_cast<double2 *>(&sg[sl][4 * sq + 2]) = make_double2(xg[2], xg[3]);
        __syncthreads();
        if (j0 + kTileChunk < a.nlat) load(j0 + kTileChunk);  // in flight under the MFMAs
        if (mine) tile_mfma(acc, sd, sg, (a.nlat - j0 + 3) / 4);     // a group wholly past nlat is not issued
    }
    if (!mine) return;
    const double lo = a.lo[v], hi = a.hi[v];
    // for_each_element in another order: the natural cell of a column of the tile is found once, not once per element
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int s = s0 + tile_cell(threadIdx.x, 0, t, 0).col;                             // the stored cell
        const int k = 2 * natural_unit(s >> 1, a.threads, split) + (s & 1);
        if (k >= a.nlat) continue;                                                         // padding is never written
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c0 + tile_cell(threadIdx.x, r, t, g).row;
                if (c >= a.ncol) continue;
                double *const cell = a.row[v] + (long long)c * a.pitch + s;
                double x = *cell + acc[r][t][g];
                x = x < lo ? lo : x;
                x = x > hi ? hi : x;
                *cell = x;
            }
    }
}

hipError_t launch_update_innovations(const UpdateArgs &a, hipStream_t s) {
    update_innovations_kernel<<<dim3((unsigned)(a.pitch / (2 * kInnovLanes)) * (unsigned)a.ncol), kInnovLanes, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_update_product(const UpdateArgs &a, hipStream_t s) {
    update_product_kernel<<<dim3((unsigned)(a.pitch / kTileSide), (unsigned)((a.ncol + kTileSide - 1) / kTileSide), (unsigned)a.nvars),
                            kTileLanes, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
