// ebm_export_columns / ebm_import_columns (include/ebm_hip.h): whole columns between the handle's arrays and a packed
// device buffer of records, ONE launch per call over (records x slots) — the fusion over the arrays that the per-array
// passes of ebm_resample.hip leave open.  A record is
//   nfields slots of rowlen doubles | the active-set row (amask_units units of 16 bytes) | N_c, 0.0
// and every field slot is in the NATURAL layout: a row that the handle holds pair-split (bit s of split_mask) is
// un-permuted on the way out and permuted on the way in.  The unit of the permutation is the pair of cells, 16 bytes:
// natural unit u lies at split unit (u & 1) * T + (u >> 1) (split_index of ebm_internal.h in units), so a lane moves 16
// bytes per access in both layouts — lane i of a wave reads unit 64w + i of the natural side, and on the split side the
// even and the odd lanes each cover 512 consecutive bytes, whole 128-byte lines.  One workgroup of 256 lanes moves one
// row.  Plain loads and stores; no LDS, no scratch, no atomics.
#include "ebm_internal.h"

namespace ebm {

constexpr int kExchangeThreads = 256;

// blockIdx.x = entry i of the list, blockIdx.y = slot.  Export: record i <- column cols[i].  Import: column cols[i] <-
// record records[i] (null: i).  A slot whose row pointer is null does not move.
template <bool EXPORT>
__global__ void __launch_bounds__(kExchangeThreads) exchange_rows_kernel(const ExchangeArgs a) {
    const long long i = blockIdx.x;
    const int s = blockIdx.y;
    const long long col = a.cols[i];
    const long long rec = EXPORT ? i : (a.records ? (long long)a.records[i] : i);
    uint4 *const slot = reinterpret_cast<uint4 *>(a.buf + rec * a.record) + (long long)s * (a.rowlen / 2);
    if (s < a.nfields) {
        if (!a.row[s]) return;
        uint4 *const row = reinterpret_cast<uint4 *>(a.row[s] + col * a.pitch);
        const bool split = (a.split_mask >> s) & 1u;
        const int T = a.threads;
        for (int u = threadIdx.x; u < a.rowlen / 2; u += kExchangeThreads) {
            const int p = split ? (u & 1) * T + (u >> 1) : u;
            if (EXPORT) slot[u] = row[p];
            else row[p] = slot[u];
        }
        return;
    }
    // the last slot: the active-set row as it lies in memory, then the 16-byte tail (N_c, reserved)
    uint4 *const act = reinterpret_cast<uint4 *>(a.amask) + col * a.amask_units;
    for (int u = threadIdx.x; u < a.amask_units; u += kExchangeThreads) {
        if (EXPORT) slot[u] = act[u];
        else act[u] = slot[u];
    }
    if (threadIdx.x == 0) {
        double2 *const tail = reinterpret_cast<double2 *>(slot + a.amask_units);
        if (EXPORT) *tail = make_double2(a.nstate ? a.nstate[col] : 0.0, 0.0);
        else if (a.nstate) a.nstate[col] = tail->x;
    }
}

hipError_t launch_export_columns(const ExchangeArgs &a, int n, hipStream_t s) {
    exchange_rows_kernel<true><<<dim3((unsigned)n, (unsigned)a.nfields + 1u), kExchangeThreads, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_import_columns(const ExchangeArgs &a, int n, hipStream_t s) {
    exchange_rows_kernel<false><<<dim3((unsigned)n, (unsigned)a.nfields + 1u), kExchangeThreads, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
