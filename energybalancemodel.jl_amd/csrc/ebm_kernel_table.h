// The compile-time lists of workgroup sizes and the lookup from a run-time size to a kernel instantiation.  Included by
// every translation unit that instantiates MIZ kernels; each instantiates only what its own accessor names.
#pragma once
#include "ebm_miz_step.h"
#include "ebm_miz_fused.h"
#include "ebm_miz_resident.h"

namespace ebm {

namespace {

// Every workgroup size is compiled as a constant: T = 64 ... 1024 in steps of one wave (two cells per thread: 64 ... 512,
// and 768 for every meridian of 1025 ... 1536 cells).  A list of sizes is a type; kernel_for(sizes, threads, pick) returns
// pick's instantiation for `threads`, nullptr if the list lacks it.
template <int... TT> struct Sizes {};
template <int... A, int... B> constexpr Sizes<A..., B...> operator+(Sizes<A...>, Sizes<B...>) { return {}; }
#ifdef EBM_QUICK   // development builds (tests/tools/resource_usage.py -DEBM_QUICK): four sizes only
constexpr Sizes<64, 256, 512> kUpTo512;
constexpr Sizes<1024> kAbove512;
#else
constexpr Sizes<64, 128, 192, 256, 320, 384, 448, 512> kUpTo512;
constexpr Sizes<576, 640, 704, 768, 832, 896, 960, 1024> kAbove512;
#endif
constexpr Sizes<768> kTwoCellsAbove512;   // two cells per thread, 1024 < nlat <= kMaxLat2: always 768 threads (choose_launch)
template <int TT> struct Threads { static constexpr int value = TT; };
template <typename Pick, int... TT>
KernelFn kernel_for(Sizes<TT...>, int threads, Pick pick) {
    KernelFn fn = nullptr;
    ((fn = threads == TT ? pick(Threads<TT>()) : fn), ...);
    return fn;
}

template <int C, int GRID, int OUT, bool IMEX>
KernelFn miz_kernel_for(int threads) {
    auto pick = [](auto tt) -> KernelFn { return miz_step_kernel<C, GRID, OUT, decltype(tt)::value, IMEX>; };
    if constexpr (C == 4) return kernel_for(kUpTo512 + kAbove512, threads, pick);
    else return kernel_for(kUpTo512 + kTwoCellsAbove512, threads, pick);
}
// the state-only step that derives phi from Ei and h instead of loading and storing it: four cells per thread, every size
// (ZERO_LINES: ... and neither loads nor stores state lines that are all zero)
template <int GRID, bool ZERO_LINES = false>
[[maybe_unused]] KernelFn miz_step_phi_derived_for(int threads) {
    return kernel_for(kUpTo512 + kAbove512, threads, [](auto tt) -> KernelFn {
        return miz_step_kernel<4, GRID, OUT_STATE, decltype(tt)::value, false, true, ZERO_LINES>;
    });
}
template <int C, int GRID, bool IMEX>
[[maybe_unused]] KernelFn miz_step_by_mode(int mode, int threads) {
    switch (mode) {
        case OUT_STATE: return miz_kernel_for<C, GRID, OUT_STATE, IMEX>(threads);
        case OUT_DIAG: return miz_kernel_for<C, GRID, OUT_DIAG, IMEX>(threads);
        case OUT_SAVE: return miz_kernel_for<C, GRID, OUT_SAVE, IMEX>(threads);
        default: return nullptr;
    }
}
// the one-step kernels of the reference's step on one grid, by the plan: eliding, deriving, or the mode's at two or four cells
template <int GRID>
[[maybe_unused]] KernelFn miz_step_for(const StepPlan &p) {
    if (p.phi_derived) return p.zero_lines ? miz_step_phi_derived_for<GRID, true>(p.threads) : miz_step_phi_derived_for<GRID>(p.threads);
    return p.cells == 2 ? miz_step_by_mode<2, GRID, false>(p.mode, p.threads) : miz_step_by_mode<4, GRID, false>(p.mode, p.threads);
}
// every size for both models: the extension has no other fused kernel; the reference's step where the register kernel ends
// (more than kFusedRegThreads threads) and, below that, where the handle prefers occupancy over latency; integrate (SAVE)
// has no other fused kernel at four cells per thread
template <int GRID, bool IMEX, bool SAVE>
KernelFn miz_resident_for(int threads) {
    return kernel_for(kUpTo512 + kAbove512, threads,
                      [](auto tt) -> KernelFn { return miz_resident_kernel<GRID, decltype(tt)::value, IMEX, SAVE>; });
}
// the register kernel: 768 threads at two cells per thread (166 VGPRs: three waves per SIMD = kFusedRegThreads2 threads),
// but not with the sums (SAVE: 144 B of scratch at its three waves per SIMD; ebm_integrate keeps one launch per step there)
template <int C, int GRID, bool SAVE = false>
KernelFn miz_fused_for(int threads) {
    auto pick = [](auto tt) -> KernelFn { return miz_fused_kernel<C, GRID, decltype(tt)::value, SAVE>; };
    if constexpr (C == 2 && !SAVE) return kernel_for(kUpTo512 + kTwoCellsAbove512, threads, pick);
    else return kernel_for(kUpTo512, threads, pick);
}

}  // namespace

}  // namespace ebm
