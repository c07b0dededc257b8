// The host runtime's table math: plain fp64 arithmetic, the bit-exact restatement of the reference for every table the
// kernels read.  No HIP and no handle: every function takes what it uses, so a plain C++ compiler builds it
// (tests/test_host_tables.py compares it with the oracle without a GPU).  Header-only; not part of the public interface.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>
#include <vector>

#include "../../include/ebm_hip.h"
#include "ebm_types.h"

namespace ebm_tables {

// Per-latitude constants of parameter block p into the zero-filled host slab `slab` (G_COUNT x gstride).  Same
// expressions, in the same order, as the reference: get_diffop (src/infrastructure.jl:480-492), the non-uniform cache
// (:509-518) and get_statics (src/classic.jl:18-29).  ebm_create runs it for the handle's vector, ebm_set_column_params
// for every distinct row.
inline void build_tables(int model, int grid, int nlat, long long gstride, double dt, const ebm::Params &p, const double *x,
                         double *slab) {
    const int nx = nlat;
    std::vector<double> xv(x, x + nx), g0(nx), g1(nx), g2(nx), g3(nx, 0.0), g4(nx, 0.0), lo(nx), di(nx), up(nx);
    const bool uniform = (grid == EBM_GRID_IDENTITY) || (model == EBM_MODEL_CLASSIC);
    // classic: get_statics always uses get_diffop, whatever the grid type (src/classic.jl:21)
    const double Dscale = (model == EBM_MODEL_CLASSIC) ? 1.0 : p.D;
    if (uniform) {
        const double dx = 1.0 / nx;
        std::vector<double> lam(nx > 1 ? nx - 1 : 0);
        for (int i = 1; i < nx; ++i) {
            double xb = (double)i / nx;
            lam[i - 1] = (1.0 - xb * xb) / (dx * dx);
        }
        for (int k = 0; k < nx; ++k) {
            double sub = k > 0 ? lam[k - 1] : 0.0;
            double sup = k < nx - 1 ? lam[k] : 0.0;
            double l1 = k > 0 ? -lam[k - 1] : 0.0;
            double l2 = k < nx - 1 ? -lam[k] : 0.0;
            double l3 = (-l1) - l2;
            g0[k] = Dscale * sub;
            g1[k] = Dscale * (-l3);
            g2[k] = Dscale * sup;
            lo[k] = g0[k];
            di[k] = g1[k];
            up[k] = g2[k];
        }
    } else {
        for (int k = 0; k < nx; ++k) {
            double xk = x[k];
            double xm = k > 0 ? x[k - 1] : -x[0];
            double xp = k < nx - 1 ? x[k + 1] : 2.0 - x[nx - 1];
            double xxph = (xp + xk) / 2.0, xxmh = (xk + xm) / 2.0;
            g0[k] = 1.0 - xxph * xxph;
            g1[k] = 1.0 - xxmh * xxmh;
            g2[k] = xp - xk;
            g3[k] = xk - xm;
            g4[k] = xxph - xxmh;
            double u = p.D * g0[k] / (g2[k] * g4[k]);
            double l = p.D * g1[k] / (g3[k] * g4[k]);
            if (k == nx - 1) u = 0.0;
            if (k == 0) l = 0.0;
            lo[k] = l;
            up[k] = u;
            di[k] = -(l + u);
        }
    }
    // one zero-padded slab: table i at geom + i*gstride
    auto put = [&](int table, const std::vector<double> &v) {
        std::memcpy(slab + (size_t)table * gstride, v.data(), sizeof(double) * v.size());
    };
    put(ebm::G_X, xv); put(ebm::G_0, g0); put(ebm::G_1, g1); put(ebm::G_2, g2); put(ebm::G_3, g3);
    put(ebm::G_4, g4); put(ebm::G_LO, lo); put(ebm::G_DI, di); put(ebm::G_UP, up);
    if (model == EBM_MODEL_CLASSIC) {
        std::vector<double> ksub(nx), kdiag(nx), ksup(nx), aw(nx), Sb(nx);
        const double dtD = dt * p.D;
        const double one = 1.0 + p.dt_tau;
        for (int k = 0; k < nx; ++k) {
            ksub[k] = 0.0 - (dtD * g0[k]) / p.cg;
            ksup[k] = 0.0 - (dtD * g2[k]) / p.cg;
            kdiag[k] = one - (dtD * g1[k]) / p.cg;
            aw[k] = p.a0 - p.a2 * (x[k] * x[k]);
            Sb[k] = p.S0 - p.S2 * (x[k] * x[k]);
        }
        put(ebm::G_KSUB, ksub); put(ebm::G_KDIAG, kdiag); put(ebm::G_KSUP, ksup);
        put(ebm::G_AW, aw); put(ebm::G_SB, Sb);
    }
}

inline void fill_params(ebm::Params &p, const double *v, double dt) {
    p.D = v[EBM_P_D]; p.A = v[EBM_P_A]; p.B = v[EBM_P_B]; p.cw = v[EBM_P_cw];
    p.S0 = v[EBM_P_S0]; p.S1 = v[EBM_P_S1]; p.S2 = v[EBM_P_S2]; p.a0 = v[EBM_P_a0];
    p.a2 = v[EBM_P_a2]; p.ai = v[EBM_P_ai]; p.Fb = v[EBM_P_Fb]; p.k = v[EBM_P_k];
    p.Lf = v[EBM_P_Lf]; p.F = v[EBM_P_F]; p.cg = v[EBM_P_cg]; p.tau = v[EBM_P_tau];
    p.Tm = v[EBM_P_Tm]; p.m1 = v[EBM_P_m1]; p.m2 = v[EBM_P_m2]; p.alpha = v[EBM_P_alpha];
    p.rl = v[EBM_P_rl]; p.Dmin = v[EBM_P_Dmin]; p.Dmax = v[EBM_P_Dmax]; p.hmin = v[EBM_P_hmin];
    p.kappa = v[EBM_P_kappa];
    p.dt = dt;
    p.Tm_pow_m2 = std::pow(p.Tm, p.m2);
    p.c_latmelt = -M_PI / 2.0 * p.alpha;
    p.c_dn = p.Lf * p.alpha * (p.Dmin * p.Dmin) * p.hmin;
    p.c_weld = p.kappa * p.alpha / 4.0;
    p.c_ht = -1.0 / p.Lf;
    p.two_rl = 2.0 * p.rl;
    p.cg_tau = p.cg / p.tau;
    p.dt_tau = dt / p.tau;
    p.dc = p.dt_tau * p.cg_tau;
    p.M = p.B + p.cg_tau;
    p.kLf = p.k * p.Lf;
    p.theta_imex = dt / p.cw;            // EBM_MODEL_MIZ_IMEX: the solve's matrix is I - theta*Dif
}

// Segments a latitude circle of nlon unknowns is cut into (zonal_seg_* kernels): a power of two between 4 and 32 that
// leaves segments of at least 64 unknowns, else 1 (zonal_sweep_kernel walks the whole circle).  A function of nlon ONLY —
// like the column geometry, never of how many members share the handle.
inline int zonal_segments(int nlon) {
    int S = 1;
    for (int c = 4; c <= 32; c *= 2)
        if (nlon % c == 0 && nlon / c >= 64) S = c;
    return S;
}

// Data-independent part of the periodic Thomas elimination of the system (-a, B, -a) of n unknowns (see zonal_sweep_kernel):
// m_l and ep_l for l = 0 .. n-2 into M / E (stride P), the reciprocal of the reduced last diagonal into *W.
inline void periodic_tables(double a, double B, int n, double *M, double *E, size_t P, double *W) {
    double cp_prev = 0.0, ep_prev = 0.0, gW = 0.0, f = -a, cp = 0.0, ep = 0.0;
    for (int l = 0; l <= n - 2; ++l) {
        const double m = 1.0 / (l == 0 ? B : B - a * cp_prev);
        cp = a * m;
        ep = l == 0 ? cp : a * ep_prev * m;
        M[(size_t)l * P] = m;
        E[(size_t)l * P] = ep;
        if (l <= n - 3) {
            gW += f * ep;
            f = -a * ep;                // f_{l+1} = f_l cp_l = -a ep_l
        }
        cp_prev = cp;
        ep_prev = ep;
    }
    *W = 1.0 / (B + gW + (f - a) * (cp + ep));       // f = f_{n-2}, cp / ep = those of row n-2
}

// Tables of the zonal substep (ebm_zonal_diffusion, include/ebm_hip.h; kernels: zonal_sweep_kernel, zonal_seg_*): per
// latitude the coefficient a_k = (dt/cw) D / ((1 - x_k)(1 + x_k) dlambda^2) and the data-independent part of the
// elimination, stored in the handle's store index space: with 4 cells per thread entry p = j*2T + 2t + q belongs to
// latitude k = 4t + 2j + q (pair-split), with 2 cells p = k; padding latitudes get a = 0 (U = temp, Z = 0).  One segment
// (S = 1): the whole circle's chain with its wrap closure.  S > 1: the chain of ONE segment of m = nlon/S unknowns (open
// ends), and the reduced periodic system of the S segment ends, (-a'', B'', -a'') with a'' = a ep_{m-2},
// B'' = B - a cp_{m-2} - a alpha, alpha = sum_i P_i ep_i.
// tab: chain tables M | E (chain_rows x P each), reduced-system tables rM | rE (red_rows x P each), a | a2 | W (P each).
struct ZonalHostTables {
    int seg = 1;
    size_t chain_rows = 0, red_rows = 0;
    std::vector<double> tab;
};
// null, or why there are no tables (an argument error of the caller's)
inline const char *build_zonal_tables(int nlon, int nlat, int P, int T, int cells, double dt, const double *x,
                                      const ebm::Params &par, ZonalHostTables &out) {
    const int S = zonal_segments(nlon), m = nlon / S;
    const double D = par.D;
    const double dl = 2.0 * M_PI / nlon, theta = dt / par.cw;
    const size_t chain_rows = (size_t)(S == 1 ? nlon : m), red_rows = (size_t)(S == 1 ? 0 : S);
    std::vector<double> tab(2 * chain_rows * P + 2 * red_rows * P + 3 * (size_t)P, 0.0);
    double *zM = tab.data(), *zE = zM + chain_rows * P, *rM = zE + chain_rows * P, *rE = rM + red_rows * P,
           *za = rE + red_rows * P, *za2 = za + P, *zW = za2 + P;
    for (int p = 0; p < P; ++p) {
        int k = p;
        if (cells == 4) {
            const int j = p / (2 * T), rem = p % (2 * T), t = rem / 2, q = rem % 2;
            k = 4 * t + 2 * j + q;
        }
        double a = 0.0;
        if (k < nlat) {
            const double mm = (1.0 - x[k]) * (1.0 + x[k]);       // 1 - x^2 without the cancellation near the pole
            if (!(mm > 0.0)) return "ebm_zonal_diffusion: needs |x| < 1 at every cell centre (the zonal coefficient is D/(1-x^2))";
            a = theta * D / (mm * (dl * dl));
        }
        const double B = 1.0 + 2.0 * a;
        za[p] = a;
        if (S == 1) {
            periodic_tables(a, B, nlon, zM + p, zE + p, (size_t)P, &zW[p]);
            continue;
        }
        double unused;
        periodic_tables(a, B, m, zM + p, zE + p, (size_t)P, &unused);      // the open chain's m_l, ep_l are the same recurrences
        double alpha = 0.0;
        for (int i = 0; i <= m - 2; ++i) alpha += (i == 0 ? 1.0 : zE[(size_t)(i - 1) * P + p]) * zE[(size_t)i * P + p];
        const double cp_last = a * zM[(size_t)(m - 2) * P + p], ep_last = zE[(size_t)(m - 2) * P + p];
        const double a2 = a * ep_last, B2 = B - a * cp_last - a * alpha;
        za2[p] = a2;
        periodic_tables(a2, B2, S, rM + p, rE + p, (size_t)P, &zW[p]);
    }
    out.seg = S;
    out.chain_rows = chain_rows;
    out.red_rows = red_rows;
    out.tab = std::move(tab);
    return nullptr;
}

}  // namespace ebm_tables
