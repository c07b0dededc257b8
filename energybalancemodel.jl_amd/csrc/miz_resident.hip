// miz_resident_kernel without savesol!'s sums: both grids, both models, every workgroup size.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_resident_kernels(const StepPlan &p) {
    if (p.imex) return p.grid == 0 ? miz_resident_for<0, true, false>(p.threads) : miz_resident_for<1, true, false>(p.threads);
    return p.grid == 0 ? miz_resident_for<0, false, false>(p.threads) : miz_resident_for<1, false, false>(p.threads);
}

}  // namespace ebm
