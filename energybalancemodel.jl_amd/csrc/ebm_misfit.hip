// ebm_column_misfits (include/ebm_hip.h): per column, the weighted squared distance J of its profiles to each of ntargets
// target profiles and the number N of cells that entered it — the reduction ALONG a column that a particle filter's likelihood,
// a splitting coordinate and a nearest-branch sort all start from.  The order of the adds is part of the definition, and it is
// the order of one wave64:
//   work unit  one wave per column (blockIdx.x: ncol goes beyond 65 535).  Lane l owns the chains (l, 0) and (l, 1) of every
//              target: the cells 2 (l + 64 i) + e of natural unit u = l + 64 i, for the variables in the order of the call
//              and i ascending within each, one accumulator across the variables — double2 J[NT] and int2 N[NT] in registers,
//              NT a template parameter so that neither array is indexed dynamically (no scratch).
//   loads      16 bytes per lane.  A natural row: stored unit u, a wave reads 1 KiB, eight whole lines.  A pair-split row
//              (stored unit p is natural unit 2p for p < T, 2 (p - T) + 1 otherwise): an even lane reads l / 2 + 32 i of the
//              first half, an odd lane T + (l - 1) / 2 + 32 i of the second — two contiguous 512-byte runs of whole lines, and
//              every chain still sees its units in ascending order.  Nothing is converted.  Targets and rw are in the natural
//              layout at unit u; all columns share them (L2).  The loads of a batch of units — x, rw and the NT targets — are
//              issued before the first dependent add; the batch shrinks as NT grows (8, 4, 2 units), which keeps every
//              instantiation at three or four waves per SIMD.  Units with 2u >= nlat are not loaded, by any of the three.
//   finish     q_l = chain(l, 0) + chain(l, 1), then q_l += q_{l + s} for s = 32, 16, 8, 4, 2, 1 (__shfl_down: lanes >= s hold
//              values that no later step reads); lane 0 stores J and N.
// Nothing is contracted (-ffp-contract=off): d = x - y, t = (r * d) * d, every add a rounded sum.  No LDS, no atomics, plain
// vector loads and stores.
#include "ebm_internal.h"

namespace ebm {

constexpr int kMisfitLanes = 64;
template <int NT> constexpr int misfit_batch() { return NT <= 2 ? 8 : NT <= 4 ? 4 : 2; }      // units in flight per lane

// one cell's term to one target: contributes iff the cell exists, r != 0.0 and neither y nor x is NaN
__device__ __forceinline__ void misfit_term(double x, double y, double r, bool live, double &J, int &N) {
    const double d = x - y;
    const double t1 = r * d;
    const double t2 = t1 * d;
    const bool in = live && r != 0.0 && y == y && x == x;
    J = in ? J + t2 : J;
    N = in ? N + 1 : N;
}

template <int NT>
__global__ void __launch_bounds__(kMisfitLanes) column_misfits_kernel(const MisfitArgs a) {
    constexpr int B = misfit_batch<NT>();
    const long long c = blockIdx.x;
    const int l = threadIdx.x;
    const long long stride = a.pitch / 2;                            // units per row
    const int rounds = ((a.nlat + 1) / 2 + kMisfitLanes - 1) / kMisfitLanes;
    const double nan = __builtin_nan("");
    double2 J[NT];
    int2 N[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        J[t] = make_double2(0.0, 0.0);
        N[t] = make_int2(0, 0);
    }
    for (int v = 0; v < a.nvars; ++v) {
        const bool split = (a.split_mask >> v) & 1u;
        const int first = !split ? l : (l & 1) ? a.threads + (l >> 1) : (l >> 1), step = split ? 32 : 64;     // stored units
        const double2 *const x = reinterpret_cast<const double2 *>(a.row[v]) + c * stride + first;
        const double2 *const y = reinterpret_cast<const double2 *>(a.target) + v * stride + l;         // target t: t nvars rows on
        const double2 *const r = a.rw ? reinterpret_cast<const double2 *>(a.rw) + v * stride + l : nullptr;
        for (int i0 = 0; i0 < rounds; i0 += B) {
            double2 xs[B], rs[B], ys[B][NT];
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int i = i0 + j;
                const bool there = 2 * (l + 64 * i) < a.nlat;
                xs[j] = there ? x[i * step] : make_double2(nan, nan);
                rs[j] = (there && r) ? r[i * 64] : make_double2(1.0, 1.0);
#pragma unroll
                for (int t = 0; t < NT; ++t) ys[j][t] = there ? y[t * a.nvars * stride + i * 64] : make_double2(nan, nan);
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                const int k = 2 * (l + 64 * (i0 + j));
                const bool live0 = k < a.nlat, live1 = k + 1 < a.nlat;      // the odd tail's second cell is padding
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    misfit_term(xs[j].x, ys[j][t].x, rs[j].x, live0, J[t].x, N[t].x);
                    misfit_term(xs[j].y, ys[j][t].y, rs[j].y, live1, J[t].y, N[t].y);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        double q = J[t].x + J[t].y;
        int n = N[t].x + N[t].y;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            q = q + __shfl_down(q, s, 64);
            n = n + __shfl_down(n, s, 64);
        }
        if (l == 0) {
            a.out[(2LL * t) * a.ncol + c] = q;
            a.out[(2LL * t + 1) * a.ncol + c] = (double)n;
        }
    }
}

hipError_t launch_column_misfits(const MisfitArgs &a, hipStream_t s) {
    void (*kernel)(const MisfitArgs) = nullptr;
    switch (a.ntargets) {
        case 1: kernel = column_misfits_kernel<1>; break;
        case 2: kernel = column_misfits_kernel<2>; break;
        case 3: kernel = column_misfits_kernel<3>; break;
        case 4: kernel = column_misfits_kernel<4>; break;
        case 5: kernel = column_misfits_kernel<5>; break;
        case 6: kernel = column_misfits_kernel<6>; break;
        case 7: kernel = column_misfits_kernel<7>; break;
        case 8: kernel = column_misfits_kernel<8>; break;
        default: return hipErrorInvalidValue;
    }
    kernel<<<dim3((unsigned)a.ncol), kMisfitLanes, 0, s>>>(a);
    return hipGetLastError();
}

}  // namespace ebm
