// Stand-alone walk of the step launch plan of csrc/ebm_plan.h for tests/test_host_plan.py: no HIP, no GPU.
//   walk      prints
//     launch NLAT REQUESTED C T                       choose_launch, for nlat = 2 .. 4097 and cells_requested = 0, 2, 4 (T = 0: none)
//     plan C T IN_LDS MODEL GRID MODE PHI ZERO -> FAMILY LDS NOISE_MEM SPLIT RAISED
//                                                     one line per variant (for_each_variant, which prepare_kernels walks too) of
//                                                     every geometry that choose_launch returned; MODEL: classic, miz, imex
//     raise BYTES RAISED                              needs_raised_lds just below, at and just above the 64 KiB default
// The program states no rule of its own: the test holds the restatement and compares line by line.  It does check that the
// plan's coordinates are those asked for; exit status 1 and a line "VIOLATION ..." if not.
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>

#include "../energybalancemodel.jl_amd/csrc/ebm_plan.h"

namespace {

const char *const kFamilyName[] = {"none", "classic", "miz_step", "miz_fused", "miz_resident"};

int walk() {
    std::set<std::pair<int, int>> geometries;
    const int requested[] = {0, 2, 4};
    for (int nlat = 2; nlat <= ebm::kMaxLat + 1; ++nlat)
        for (int req : requested) {
            const ebm::LaunchCfg cfg = ebm::choose_launch(nlat, req);
            std::printf("launch %d %d %d %d\n", nlat, req, cfg.cells, cfg.threads);
            if (cfg.threads) geometries.insert({cfg.cells, cfg.threads});
        }
    int bad = 0;
    for (const auto &g : geometries) {
        ebm::LaunchCfg geometry{};
        geometry.cells = g.first;
        geometry.threads = g.second;
        ebm::for_each_variant(geometry, [&](const ebm::LaunchCfg &cfg, const ebm::StepVariant &v) {
            const ebm::StepPlan p = ebm::plan_step(cfg, v);
            if (p.cells != cfg.cells || p.threads != cfg.threads || p.grid != v.grid || p.mode != v.mode || p.imex != v.imex ||
                p.phi_derived != v.phi_derived || p.zero_lines != v.zero_lines || p.save() != (v.mode == ebm::OUT_LOOP_SAVE)) {
                std::printf("VIOLATION the plan's coordinates are not the variant's\n");
                bad = 1;
            }
            std::printf("plan %d %d %d %s %d %d %d %d -> %s %zu %d %d %d\n", cfg.cells, cfg.threads, (int)cfg.fused_in_lds,
                        v.model == ebm::STEP_CLASSIC ? "classic" : v.imex ? "imex" : "miz", v.grid, v.mode, (int)v.phi_derived,
                        (int)v.zero_lines, kFamilyName[p.family], p.lds_bytes, (int)p.noise_from_memory, (int)p.stores_split,
                        (int)ebm::needs_raised_lds(p));
        });
    }
    for (size_t bytes = ebm::kDefaultMaxLds - 1; bytes <= ebm::kDefaultMaxLds + 1; ++bytes) {
        ebm::StepPlan p{};
        p.family = ebm::K_MIZ_STEP;
        p.lds_bytes = bytes;
        std::printf("raise %zu %d\n", bytes, (int)ebm::needs_raised_lds(p));
    }
    return bad;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "walk")) return walk();
    std::fprintf(stderr, "usage: host_plan walk\n");
    return 2;
}
