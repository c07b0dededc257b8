// The fused-K kernels with savesol!'s sums: miz_resident_kernel<SAVE> and the two-cell miz_fused_kernel<SAVE>.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_resident_save_kernels(int grid_kind, int threads, bool imex) {
    if (imex) return grid_kind == 0 ? miz_resident_for<0, true, true>(threads) : miz_resident_for<1, true, true>(threads);
    return grid_kind == 0 ? miz_resident_for<0, false, true>(threads) : miz_resident_for<1, false, true>(threads);
}
KernelFn miz_fused2_save_kernels(int grid_kind, int threads) {     // two cells per thread: the register kernel with the sums
    return grid_kind == 0 ? miz_fused_for<2, 0, true>(threads) : miz_fused_for<2, 1, true>(threads);
}

}  // namespace ebm
