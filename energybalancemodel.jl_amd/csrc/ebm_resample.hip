// ebm_resample_columns (include/ebm_hip.h): the gather of whole columns, new state of column c = old state of column
// parent[c], in two passes per array so that no map — swap, cycle, chain, fan-out — reads a row that has been overwritten:
//   stage    row parent of the array -> row m of the staging buffer, for every entry m = (destination, parent) of the list
//   scatter  row m of the staging buffer -> row destination of the array
// The list holds the moved columns only (parent != destination); a column that keeps its state gets no workgroup and
// moves no byte.  A row is a whole row of the array as it lies in memory — a field row of `pitch` doubles, padding
// included, or a row of the warm-start active set — so the pair-split layout, a permutation WITHIN a row, is carried
// along unseen.  Every row starts on a 128-byte line (pitch and the workgroup size are multiples of 64) and is a whole
// number of lines long: a lane moves 16 bytes per access, a wave 1 KiB of consecutive lines.  Plain loads and stores; no
// LDS, no scratch, no atomics.
#include "ebm_internal.h"

namespace ebm {

constexpr int kResampleThreads = 256;

// One workgroup per list entry.  The noise state N_c (r.nstate, null: none) travels with the pass as one double behind
// the row's units in the staging row (8-byte aligned: a unit is 16 bytes), moved by lane 0.
template <bool STAGE>
__global__ void __launch_bounds__(kResampleThreads) resample_rows_kernel(const ResampleArgs r) {
    const long long m = blockIdx.x;
    const int2 e = r.list[m];                            // (destination, parent)
    uint4 *const stage = r.stage + m * r.stage_stride;
    const uint4 *__restrict__ src = STAGE ? r.rows + (long long)e.y * r.row_stride : stage;
    uint4 *__restrict__ dst = STAGE ? stage : r.rows + (long long)e.x * r.row_stride;
    for (int i = threadIdx.x; i < r.units; i += kResampleThreads) dst[i] = src[i];
    if (r.nstate && threadIdx.x == 0) {
        double *const n = reinterpret_cast<double *>(stage + r.units);
        if (STAGE) *n = r.nstate[e.y];
        else r.nstate[e.x] = *n;
    }
}

hipError_t launch_resample_stage(const ResampleArgs &r, int moved, hipStream_t s) {
    resample_rows_kernel<true><<<dim3((unsigned)moved), kResampleThreads, 0, s>>>(r);
    return hipGetLastError();
}

hipError_t launch_resample_scatter(const ResampleArgs &r, int moved, hipStream_t s) {
    resample_rows_kernel<false><<<dim3((unsigned)moved), kResampleThreads, 0, s>>>(r);
    return hipGetLastError();
}

}  // namespace ebm
