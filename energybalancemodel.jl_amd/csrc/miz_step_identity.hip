// miz_step_kernel on the identity grid: every mode and workgroup size, two and four cells per thread, and the
// state-only step that derives phi (four cells per thread), without and with zero-line elision.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_step_kernels_identity(int cells, int mode, int threads) {
    return cells == 2 ? miz_step_by_mode<2, 0, false>(mode, threads) : miz_step_by_mode<4, 0, false>(mode, threads);
}
KernelFn miz_step_phi_derived_identity(int threads) { return miz_step_phi_derived_for<0>(threads); }
KernelFn miz_step_zero_lines_identity(int threads) { return miz_step_phi_derived_for<0, true>(threads); }

}  // namespace ebm
