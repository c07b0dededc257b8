// miz_step_kernel with the implicit-diffusion extension: both grids, every mode and workgroup size.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_step_kernels_imex(int grid_kind, int mode, int threads) {        // the extension: 4 cells per thread
    return grid_kind == 0 ? miz_step_by_mode<4, 0, true>(mode, threads) : miz_step_by_mode<4, 1, true>(mode, threads);
}

}  // namespace ebm
