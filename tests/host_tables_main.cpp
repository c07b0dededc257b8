// Stand-alone caller of csrc/ebm_tables.h for tests/test_host_tables.py: no HIP, no GPU.  Arrays travel as raw doubles
// in files, so that every bit arrives.
//   tables MODEL GRID NLAT GSTRIDE IN OUT   IN: dt, x[NLAT], params[EBM_P_COUNT]
//                                           OUT: cg_tau, dt_tau, dc, M, kLf, slab[G_COUNT][GSTRIDE]
//   periodic N IN OUT                       IN: a, B        OUT: M[N-1], E[N-1], W
//   zonal NLON NLAT THREADS CELLS IN OUT    IN: dt, x[NLAT], params[EBM_P_COUNT]
//                                           OUT: seg, chain_rows, red_rows, tab   (exit status 3 and the reason on stderr
//                                           if the tables are refused)
//   segments NLON...                        prints zonal_segments of every argument
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../energybalancemodel.jl_amd/csrc/ebm_tables.h"

static std::vector<double> read_doubles(const char *path, size_t n) {
    std::vector<double> v(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), sizeof(double), n, f) != n) {
        std::fprintf(stderr, "%s: cannot read %zu doubles\n", path, n);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static void write_doubles(const char *path, const std::vector<double> &v) {
    FILE *f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(double), v.size(), f) != v.size()) {
        std::fprintf(stderr, "%s: cannot write\n", path);
        std::exit(2);
    }
    std::fclose(f);
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "tables") && argc == 8) {
        const int model = std::atoi(argv[2]), grid = std::atoi(argv[3]), nlat = std::atoi(argv[4]);
        const long long gstride = std::atoll(argv[5]);
        const std::vector<double> in = read_doubles(argv[6], 1 + (size_t)nlat + EBM_P_COUNT);
        const double dt = in[0];
        ebm::Params p{};
        ebm_tables::fill_params(p, in.data() + 1 + nlat, dt);
        std::vector<double> out(5 + (size_t)ebm::G_COUNT * gstride, 0.0);
        out[0] = p.cg_tau; out[1] = p.dt_tau; out[2] = p.dc; out[3] = p.M; out[4] = p.kLf;
        ebm_tables::build_tables(model, grid, nlat, gstride, dt, p, in.data() + 1, out.data() + 5);
        write_doubles(argv[7], out);
        return 0;
    }
    if (!std::strcmp(mode, "periodic") && argc == 5) {
        const int n = std::atoi(argv[2]);
        const std::vector<double> in = read_doubles(argv[3], 2);
        std::vector<double> out(2 * (size_t)(n - 1) + 1);
        ebm_tables::periodic_tables(in[0], in[1], n, out.data(), out.data() + (n - 1), 1, &out[2 * (size_t)(n - 1)]);
        write_doubles(argv[4], out);
        return 0;
    }
    if (!std::strcmp(mode, "zonal") && argc == 8) {
        const int nlon = std::atoi(argv[2]), nlat = std::atoi(argv[3]), T = std::atoi(argv[4]), cells = std::atoi(argv[5]);
        const std::vector<double> in = read_doubles(argv[6], 1 + (size_t)nlat + EBM_P_COUNT);
        ebm::Params p{};
        ebm_tables::fill_params(p, in.data() + 1 + nlat, in[0]);
        ebm_tables::ZonalHostTables z;
        const char *why = ebm_tables::build_zonal_tables(nlon, nlat, T * cells, T, cells, in[0], in.data() + 1, p, z);
        if (why) {
            std::fprintf(stderr, "%s\n", why);
            return 3;
        }
        std::vector<double> out = {(double)z.seg, (double)z.chain_rows, (double)z.red_rows};
        out.insert(out.end(), z.tab.begin(), z.tab.end());
        write_doubles(argv[7], out);
        return 0;
    }
    if (!std::strcmp(mode, "segments") && argc > 2) {
        for (int i = 2; i < argc; ++i) std::printf("%d\n", ebm_tables::zonal_segments(std::atoi(argv[i])));
        return 0;
    }
    std::fprintf(stderr, "usage: see the head of tests/host_tables_main.cpp\n");
    return 2;
}
