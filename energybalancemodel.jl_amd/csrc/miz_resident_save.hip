// The fused-K kernels with savesol!'s sums: miz_resident_kernel<SAVE> and the two-cell miz_fused_kernel<SAVE>.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_save_kernels(const StepPlan &p) {
    if (p.family == K_MIZ_FUSED)                          // two cells per thread: the register kernel with the sums
        return p.grid == 0 ? miz_fused_for<2, 0, true>(p.threads) : miz_fused_for<2, 1, true>(p.threads);
    if (p.imex) return p.grid == 0 ? miz_resident_for<0, true, true>(p.threads) : miz_resident_for<1, true, true>(p.threads);
    return p.grid == 0 ? miz_resident_for<0, false, true>(p.threads) : miz_resident_for<1, false, true>(p.threads);
}

}  // namespace ebm
