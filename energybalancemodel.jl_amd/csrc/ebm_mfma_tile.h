// The one dense tile of the library: 64 x 64 results per workgroup of 256 lanes on v_mfma_f64_16x16x4_f64, shared by
// ebm_covariance.hip, ebm_update.hip and ebm_gain.hip.  Those files stage their operands into LDS, each in its own way;
// everything that knows the instruction's layout is here, and nowhere else.
//
// THE INSTRUCTION.  One wave computes D[i][j] += sum_{k < 4} A[i][k] * B[j][k], i, j < 16 (both factors are given by their
// "line": the left one by its row, the right one by the column of the product it makes).  Lane l supplies ONE double of each
// factor, A[l & 15][l >> 4] and B[l & 15][l >> 4], and holds four of D: register g of lane l is D[(l >> 4) + 4 g][l & 15].
//
// THE TILE.  The four waves lie 2 x 2 over the tile, wave w owning the 32 x 32 at (r0, q0) = ((w >> 1) * 32, (w & 1) * 32), as
// 2 x 2 accumulators: acc[s][t] is the 16 x 16 at (r0 + 16 s, q0 + 16 t).  The contraction passes through LDS kTileChunk = 16
// indices at a time, as four groups of four; per group a lane reads a[0], a[1], b[0], b[1] and the wave issues
// acc[s][t] = mfma(a[s], b[t], acc[s][t]).  A chain is that statement over ascending groups from +0.0 with the left factor
// as the A operand: the numerical definition of the three calls in include/ebm_hip.h.
//
// LDS holds a side either line-major, [64][kTileLinePitch = 18] doubles (36 words per line: the sixteen lines x two k that a
// half-wave reads for an operand fall on 32 distinct even banks), or k-major, [16][kTileKPitch = 80] (160 words = 32 mod 64
// banks: the two k that a half-wave reads fall on disjoint banks).
//
// The first part is plain constexpr C++ and is played on the host by tests/host_mfma_tile_main.cpp.
#pragma once

namespace ebm {

constexpr int kTileSide = 64;                  // results per side of a workgroup's tile
constexpr int kTileLanes = 256;                // four waves, 2 x 2 over the tile
constexpr int kTileChunk = 16;                 // contraction indices in LDS together: four groups of four
constexpr int kTileLinePitch = kTileChunk + 2; // doubles per line of a line-major side
constexpr int kTileKPitch = kTileSide + 16;    // doubles per k of a k-major side

struct TileLane { int r0, q0, lk, lc; };       // the wave's corner; the lane's k of a group and its line or column of a 16
constexpr TileLane tile_lane(int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    return {(wave >> 1) * 32, (wave & 1) * 32, lane >> 4, lane & 15};
}
// what lane tid supplies of a group as a[s] and as b[t]: line `line` of the tile's side, index k of the group's four
struct TileOperand { int line, k; };
constexpr TileOperand tile_operand_a(int tid, int s) { const TileLane l = tile_lane(tid); return {l.r0 + 16 * s + l.lc, l.lk}; }
constexpr TileOperand tile_operand_b(int tid, int t) { const TileLane l = tile_lane(tid); return {l.q0 + 16 * t + l.lc, l.lk}; }
// where register g of acc[s][t] of lane tid lies in the tile
struct TileCell { int row, col; };
constexpr TileCell tile_cell(int tid, int s, int t, int g) {
    const TileLane l = tile_lane(tid);
    return {l.r0 + 16 * s + 4 * g + l.lk, l.q0 + 16 * t + l.lc};
}
// a side staged in LDS, tile_line_major[kTileSide] or tile_k_major[kTileChunk], and its element (line, k)
typedef double tile_line_major[kTileLinePitch];
typedef double tile_k_major[kTileKPitch];
constexpr double tile_lds(const tile_line_major *side, int line, int k) { return side[line][k]; }
constexpr double tile_lds(const tile_k_major *side, int line, int k) { return side[k][line]; }

#ifdef __HIPCC__
typedef double tile_acc __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void tile_clear(tile_acc (&acc)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[s][t] = tile_acc{0.0, 0.0, 0.0, 0.0};
}

// the first `groups` (<= 4) groups of the chunk staged in sa (the left factor) and sb; which groups are part of a chain is
// its caller's rule
template <class SIDE>
__device__ __forceinline__ void tile_mfma(tile_acc (&acc)[2][2], const SIDE *sa, const SIDE *sb, int groups) {
#pragma unroll
    for (int n = 0; n < kTileChunk / 4; ++n) {
        if (n >= groups) break;
        double av[2], bv[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const TileOperand a = tile_operand_a(threadIdx.x, s), b = tile_operand_b(threadIdx.x, s);
            av[s] = tile_lds(sa, a.line, 4 * n + a.k);
            bv[s] = tile_lds(sb, b.line, 4 * n + b.k);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[s][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s], bv[t], acc[s][t], 0, 0, 0);
    }
}

// f(row, column, value) for the lane's sixteen results
template <class F>
__device__ __forceinline__ void for_each_element(const tile_acc (&acc)[2][2], F f) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const TileCell c = tile_cell(threadIdx.x, s, t, g);
                f(c.row, c.col, acc[s][t][g]);
            }
}
#endif

}  // namespace ebm
