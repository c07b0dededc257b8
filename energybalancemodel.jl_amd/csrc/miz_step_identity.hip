// miz_step_kernel on the identity grid: every mode and workgroup size, two and four cells per thread, and the
// state-only step that derives phi (four cells per thread), without and with zero-line elision.
#include "ebm_kernel_table.h"

namespace ebm {

KernelFn miz_step_kernels_identity(const StepPlan &p) { return miz_step_for<0>(p); }

}  // namespace ebm
