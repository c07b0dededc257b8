// miz_resident_kernel without savesol!'s sums: both grids, both models, every workgroup size.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_resident_kernels(int grid_kind, int threads, bool imex) {
    if (imex) return grid_kind == 0 ? miz_resident_for<0, true, false>(threads) : miz_resident_for<1, true, false>(threads);
    return grid_kind == 0 ? miz_resident_for<0, false, false>(threads) : miz_resident_for<1, false, false>(threads);
}

}  // namespace ebm
