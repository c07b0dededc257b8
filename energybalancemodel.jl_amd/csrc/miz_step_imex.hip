// miz_step_kernel with the implicit-diffusion extension: both grids, every mode and workgroup size.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_step_kernels_imex(const StepPlan &p) {        // the extension: 4 cells per thread
    return p.grid == 0 ? miz_step_by_mode<4, 0, true>(p.mode, p.threads) : miz_step_by_mode<4, 1, true>(p.mode, p.threads);
}

}  // namespace ebm
