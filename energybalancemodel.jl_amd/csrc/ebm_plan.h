// The step launch plan: THE rule for which kernel family steps a handle's columns, with how much dynamic LDS, and whether its
// forcing-noise sequence has to be produced in memory by a launch of its own before it.  Plain C++17, no HIP include: the
// rule is walked exhaustively by a stand-alone host program (tests/host_plan_main.cpp).  The kernel table (kernel_of,
// ebm_launch.hip) maps a plan's coordinates to an instantiation and holds no rule; a new kernel family is added in plan_step
// and in kernel_of and nowhere else.
#pragma once
#include <cstddef>

#include "ebm_types.h"

namespace ebm {

struct LaunchCfg {
    int threads;        // workgroup size (multiple of 64)
    int cells;          // cells per thread (C)
    // fused-K launches of the reference's step where both kernels exist (four cells per thread, <= kFusedRegThreads threads):
    // state resident in LDS (128 VGPRs: up to four workgroups per CU fill each other's barrier stalls — launches of many
    // columns) instead of in registers (fewer LDS round trips: a few columns).  Same bits; set by the runtime, not by
    // choose_launch — the GEOMETRY stays a function of (nlat, cells) only.
    bool fused_in_lds;
};

// Cells per thread: 4 unless the caller asks for 2 (ebm_options::cells_per_thread; nlat <= kMaxLat2 = 1536: the
// fused kernel then still fits three waves per SIMD).  4 is the throughput geometry (32 contiguous bytes per lane and
// field); a run of a FEW short meridians is latency-bound on a handful of waves, and 2 cells per thread put twice as
// many SIMDs to work on every meridian.  The geometry — and with it the tridiagonal partition, i.e. the rounding of the
// solves — is a function of (nlat, cells) ONLY, never of the number of columns: a member gives the same bits alone, in
// a large ensemble and under any sharding.  threads = 0: nlat > kMaxLat, no geometry.
inline LaunchCfg choose_launch(int nlat, int cells_requested) {
    LaunchCfg cfg{};
    if (nlat > kMaxLat) return cfg;
    const int cells = (cells_requested == 2 && nlat <= kMaxLat2) ? 2 : 4;
    const int chunks = (nlat + cells - 1) / cells;
    cfg.threads = ((chunks + 63) / 64) * 64;
    if (cells == 2 && cfg.threads > 512) cfg.threads = 768;     // the one size compiled beyond 512 (padding cells stay zero)
    cfg.cells = cells;
    return cfg;
}

// What a caller asks for.  mode: OutMode; phi_derived, zero_lines: the field book's two answers for the launch
// (step_derives_phi, step_elides_zero_lines).  imex: the MIZ model with the implicit-diffusion extension.
enum StepModel { STEP_CLASSIC = 0, STEP_MIZ };
struct StepVariant {
    int model, grid;
    bool imex;
    int mode;
    bool phi_derived, zero_lines;
};
// The answer.  K_NONE: no such kernel.  The coordinates of the instantiation are the geometry's and the variant's own.
enum KernelFamily { K_NONE = 0, K_CLASSIC, K_MIZ_STEP, K_MIZ_FUSED, K_MIZ_RESIDENT };
struct StepPlan {
    KernelFamily family;
    int cells, threads, grid, mode;
    bool imex, phi_derived, zero_lines;
    size_t lds_bytes;          // dynamic LDS per workgroup
    bool noise_from_memory;    // with noise installed, launch_noise_sequence goes first: the kernel reads N_c from StepArgs::nseq
    bool stores_split;         // a one-step MIZ launch at four cells per thread: it leaves the diagnostic fields pair-split
    bool save() const { return mode == OUT_LOOP_SAVE; }
};
constexpr size_t kDefaultMaxLds = 64 * 1024;   // dynamic LDS above this must be requested per kernel (prepare_kernels)
inline bool needs_raised_lds(const StepPlan &p) { return p.family != K_NONE && p.lds_bytes > kDefaultMaxLds; }
constexpr bool is_fused_mode(int mode) { return mode == OUT_LOOP || mode == OUT_LOOP_SAVE; }

// LDS in doubles per thread: 2 x 3 for the cyclic reduction of every solve; the one-step MIZ kernel stashes Ew, h, Tw (3 C);
// the resident kernel has 4 for the solve and 4 fields x 4 cells for the state.
inline StepPlan plan_step(const LaunchCfg &cfg, const StepVariant &v) {
    const int C = cfg.cells, T = cfg.threads;
    auto plan = [&](KernelFamily family, int lds_doubles, bool noise_from_memory) {
        return StepPlan{family, C, T, v.grid, v.mode, v.imex, v.phi_derived, v.zero_lines, sizeof(double) * lds_doubles * (size_t)T,
                        noise_from_memory, family == K_MIZ_STEP && C == 4};
    };
    const StepPlan none = plan(K_NONE, 0, false);
    if (v.mode < OUT_STATE || v.mode > OUT_LOOP_SAVE || (v.zero_lines && !v.phi_derived)) return none;
    if (v.model == STEP_CLASSIC) {       // one kernel; E and Tg in registers between the steps of a fused launch, N_c in memory
        if (v.imex || v.phi_derived || v.mode == OUT_LOOP_SAVE) return none;
        return plan(K_CLASSIC, 6, v.mode == OUT_LOOP);
    }
    if (v.phi_derived && (v.mode != OUT_STATE || v.imex || C != 4)) return none;   // the deriving step: the reference's, four cells
    if (v.imex && C != 4) return none;                                             // the extension: four cells
    if (!is_fused_mode(v.mode)) return plan(K_MIZ_STEP, 6 + 3 * C, false);
    // fused-K: the state in registers where that kernel exists — and the handle does not prefer occupancy (fused_in_lds) —
    // resident in LDS otherwise.  The two compute the same bits.  With savesol!'s sums: resident at four cells, registers at two.
    const bool save = v.mode == OUT_LOOP_SAVE;
    const bool resident = save ? C == 4 : v.imex || (C == 4 && (T > kFusedRegThreads || cfg.fused_in_lds));
    if (resident) return C == 4 ? plan(K_MIZ_RESIDENT, 20, true) : none;
    // the register kernel: up to kFusedRegThreads threads, and kFusedRegThreads2 at two cells without the sums; up to
    // kFusedRegThreads it evaluates the noise sequence itself (kNoiseMem, ebm_miz_fused.h)
    if (T > ((C == 2 && !save) ? kFusedRegThreads2 : kFusedRegThreads)) return none;
    return plan(K_MIZ_FUSED, 6, T > kFusedRegThreads);
}

// Every variant of a geometry, fn(cfg with fused_in_lds set, variant) — the runtime's choice of fused_in_lds among them, so
// that what prepare_kernels readies at ebm_create covers whatever the handle launches later.
template <class Fn>
void for_each_variant(LaunchCfg cfg, Fn fn) {
    for (int in_lds = 0; in_lds < 2; ++in_lds)
        for (int model = 0; model < 3; ++model)          // classic, MIZ, MIZ with the extension
            for (int grid = 0; grid < 2; ++grid)
                for (int mode = OUT_STATE; mode <= OUT_LOOP_SAVE; ++mode)
                    for (int flags = 0; flags < 4; ++flags) {
                        cfg.fused_in_lds = in_lds != 0;
                        fn(cfg, StepVariant{model == 0 ? STEP_CLASSIC : STEP_MIZ, grid, model == 2, mode, (flags & 1) != 0, (flags & 2) != 0});
                    }
}

}  // namespace ebm
