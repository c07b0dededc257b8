// miz_step_kernel on every other grid: every mode and workgroup size, two and four cells per thread, and the
// state-only step that derives phi (four cells per thread).
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_step_kernels_nonuniform(int cells, int mode, int threads) {
    return cells == 2 ? miz_step_by_mode<2, 1, false>(mode, threads) : miz_step_by_mode<4, 1, false>(mode, threads);
}
KernelFn miz_step_phi_derived_nonuniform(int threads) { return miz_step_phi_derived_for<1>(threads); }
KernelFn miz_step_zero_lines_nonuniform(int threads) { return miz_step_phi_derived_for<1, true>(threads); }

}  // namespace ebm
