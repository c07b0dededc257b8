// Stand-alone walk of the savesol! schedule of csrc/ebm_savesol.h for tests/test_host_savesol.py: no HIP, no GPU.
//   walk NT DUR LASTONLY WINTER SUMMER RAW WANT_WINTER WANT_SUMMER SUMS FUSE      one configuration
//   sweep                                                                         nt 1 .. 8, dur 1 .. 3, both indices 0 .. nt + 1,
//                                                                                 lastonly, every subset of the four outputs, fuse
//   each configuration prints
//     cfg NT DUR LASTONLY WINTER SUMMER RAW WANT_WINTER WANT_SUMMER SUMS FUSE
//     s FIRST SUMS TAB TAB_NEXT YEAR RAW_INDEX SEASON SNAPSHOT DIAG LAST MEAN RESTART      a single step (FIRST 0-based)
//     f FIRST N SUMS                                                                       a fused stretch
//   staging BUDGET NPITCH NVARS NRAW    or    staging  (nraw 1 .. 20; budgets for chunk 1 (also from too small a budget), 2, 3,
//                                                       nraw and more than nraw)
//   each prints
//     stage BUDGET NPITCH NVARS NRAW CHUNK TOTAL_ELEMS HALF1_BASE_ELEMS VAR_STRIDE_ELEMS
//     k HALF OFFSET SLOT_ELEMS                            a kept step's slot, nraw of them
//     x HALF COUNT RAW_BASE DST_SNAPSHOT_OF_LAST_VAR      a flush
// The program states no rule of its own: the test holds the restatement and compares line by line.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../energybalancemodel.jl_amd/csrc/ebm_savesol.h"

namespace {

void walk(const ebm::SaveConfig &c) {
    std::printf("cfg %d %d %d %d %d %d %d %d %d %d\n", c.nt, c.dur, (int)c.lastonly, c.winter_inx, c.summer_inx, (int)c.keep_raw,
                (int)c.want_winter, (int)c.want_summer, (int)c.want_sums, (int)c.may_fuse);
    ebm::SaveWalk w(c);
    for (ebm::SaveItem it; w.next(it);) {
        const ebm::SaveStep &s = it.step;
        if (it.n > 1)
            std::printf("f %lld %lld %d\n", it.first, it.n, (int)it.sums);
        else
            std::printf("s %lld %d %d %d %lld %lld %d %d %d %d %d %d\n", it.first, (int)it.sums, s.tab, s.tab_next, s.year, s.raw_index,
                        (int)s.season, (int)s.snapshot, (int)s.diag(), (int)s.last, (int)s.mean, (int)s.restart);
    }
}

void sweep() {
    for (int nt = 1; nt <= 8; ++nt)
        for (int dur = 1; dur <= 3; ++dur)
            for (int winter = 0; winter <= nt + 1; ++winter)
                for (int summer = 0; summer <= nt + 1; ++summer)
                    for (int flags = 0; flags < 64; ++flags)
                        walk(ebm::SaveConfig{nt, dur, (flags & 1) != 0, winter, summer, (flags & 2) != 0, (flags & 4) != 0,
                                             (flags & 8) != 0, (flags & 16) != 0, (flags & 32) != 0});
}

void staging(size_t budget, size_t npitch, int nvars, long long nraw) {
    ebm::RawStaging st(budget, npitch, nvars, nraw);
    std::printf("stage %zu %zu %d %lld %lld %zu %zu %zu\n", budget, npitch, nvars, nraw, st.chunk(), st.total_elems(),
                st.half_base_elems(1), st.var_stride_elems());
    ebm::RawFlush f;
    for (long long i = 0; i < nraw; ++i) {
        const ebm::RawSlot slot = st.slot();
        std::printf("k %d %lld %zu\n", slot.half, slot.offset, st.slot_elems(slot));
        if (st.kept(f)) std::printf("x %d %lld %lld %zu\n", f.half, f.count, f.raw_base, st.dst_snapshot(f, nvars - 1));
    }
    if (st.flush(f)) std::printf("x %d %lld %lld %zu\n", f.half, f.count, f.raw_base, st.dst_snapshot(f, nvars - 1));
}

void staging_sweep() {
    const size_t npitch = 7;
    const int nvars = 3;
    const size_t snapshot = sizeof(double) * npitch * nvars;
    for (long long nraw = 1; nraw <= 20; ++nraw) {
        const size_t budgets[] = {1, snapshot, 2 * snapshot, 3 * snapshot + 5, (size_t)nraw * snapshot, (size_t)(nraw + 5) * snapshot};
        for (size_t budget : budgets) staging(budget, npitch, nvars, nraw);
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep(), 0;
    if (argc == 12 && !std::strcmp(argv[1], "walk")) {
        int a[10];
        for (int i = 0; i < 10; ++i) a[i] = std::atoi(argv[2 + i]);
        return walk(ebm::SaveConfig{a[0], a[1], a[2] != 0, a[3], a[4], a[5] != 0, a[6] != 0, a[7] != 0, a[8] != 0, a[9] != 0}), 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "staging")) return staging_sweep(), 0;
    if (argc == 6 && !std::strcmp(argv[1], "staging"))
        return staging(std::strtoull(argv[2], nullptr, 10), std::strtoull(argv[3], nullptr, 10), std::atoi(argv[4]), std::atoll(argv[5])), 0;
    std::fprintf(stderr, "usage: host_savesol walk NT DUR LASTONLY WINTER SUMMER RAW WANT_WINTER WANT_SUMMER SUMS FUSE | sweep | "
                         "staging [BUDGET NPITCH NVARS NRAW]\n");
    return 2;
}
