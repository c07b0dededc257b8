// Pieces of the MIZ step: the pointwise physics, the two diffusion stencils (also used by diffusion_kernel), the Newton
// iteration and savesol! from registers (also used by the classic kernel).  One definition each, shared by
// miz_step_kernel, miz_fused_kernel and miz_resident_kernel: bit-identical steps.
#pragma once
#include "ebm_device.h"
#include "ebm_noise.h"
#include "ebm_solve.h"

namespace ebm {

// Cell i of a thread's chunk has its neighbours in the chunk, or at the chunk's ends in the neighbouring chunks: `halo`
template <int C>
__device__ __forceinline__ double left_of(const double (&v)[C], int i, double halo) {
    return i > 0 ? v[i > 0 ? i - 1 : 0] : halo;
}
template <int C>
__device__ __forceinline__ double right_of(const double (&v)[C], int i, double halo) {
    return i < C - 1 ? v[i < C - 1 ? i + 1 : i] : halo;
}

// ---- MIZ pointwise physics (one cell), bit-exact restatement of src/miz.jl:160-194 ----------
struct MizCellOut {
    double q[Q_MIZ_COUNT];     // indexed by MizQuantity
};

// vert_flux, src/miz.jl:96-101: the vertical fluxes into ice and water (called twice in the reference with the same
// Tbar / diffusion term)
struct VertFlux {
    double Fvi, Fvw;
};
__device__ __forceinline__ VertFlux vert_flux(ConstParams &p, double S, double xk, double tb, double dif, double f) {
    const double Tm = p.Tm;
    const double L = p.A + p.B * (tb - Tm);
    const double sol_i = 0.0 + p.ai * S;
    const double sol_w = 0.0 + (p.a0 - p.a2 * (xk * xk)) * S;
    const double Fvi = sol_i - L + dif + p.Fb + f;
    const double Fvw = sol_w - L + dif + p.Fb + f;
    return {Fvi, Fvw};
}

// concentration, src/miz.jl:74-80: the ice cover of a cell from its ice enthalpy and thickness.  miz_cell_update ends with it
// and stores Ei (zeroed where h == 0, which phi does not see: h == 0 gives 0 first) and h, so after any step phi is this
// function of the stored Ei and h, bit for bit — what the one-step kernel that does not store phi forms in its phase A
// (miz_step_kernel, PHI_DERIVED) and restore_phi_kernel writes back.  Padding cells: Ei = h = 0 gives 0.
__device__ __forceinline__ double concentration(ConstParams &p, double Ei, double h) {
    double phi_n = ieee_div(-Ei, p.Lf * h);
    if (h == 0.0) phi_n = 0.0;
    if (phi_n > 1.0) phi_n = 1.0;
    return phi_n;
}

__device__ __forceinline__ MizCellOut miz_cell_update(ConstParams &p, double f, double S, double xk,
                                                     double dif, double tb, double Ei, double Ew,
                                                     double hk, double Dk, double ph, double Tw,
                                                     double Ti) {
    const double Lf = p.Lf, alpha = p.alpha, dt = p.dt;
    // num, src/miz.jl:83-87
    double n = ieee_div(ph, alpha * (Dk * Dk));
    if (Dk == 0.0) n = 0.0;
    const VertFlux fv = vert_flux(p, S, xk, tb, dif, f);
    const double Fvi = fv.Fvi, Fvw = fv.Fvw;
    // wlat :71, lat_flux :103-107
    const double wl = p.m1 * (Tw - p.Tm_pow_m2);
    double Flat = ieee_div(ph * hk * Lf * wl * M_PI, alpha * Dk);
    if (Dk == 0.0) Flat = 0.0;
    // forward Euler (:137-138,148,166-167) and redistributeE (:109-117)
    const double rEi = Ei + (ph * Fvi + Flat) * dt;
    const double rEw = Ew + ((1.0 - ph) * Fvw - Flat) * dt;
    const double cEi = jl_clamp(rEi, -INFINITY, 0.0);
    const double cEw = jl_clamp(rEw, 0.0, INFINITY);
    const double psiEidt = rEi - cEi, psiEwdt = rEw - cEw;
    double Ei_n = cEi + psiEwdt;
    const double Ew_n = cEw + psiEidt;
    // area_lead :90-93
    const double Dr = Dk + p.two_rl;
    const double ring = alpha * n * (Dr * Dr - Dk * Dk);
    const double Al = jl_min(ring, 1.0 - ph);
    // split_psiEw :120-125 applied to psiEwdt/dt (:173); the divisor is a constant of the run: its
    // refined reciprocal comes from the parameter block (same routine, same bits as ieee_div)
    const double psi = div_with_rcp(psiEwdt, dt, p.rcp_dt);
    double Ql = ieee_div(Al, 1.0 - ph) * psi;
    if (ph == 1.0) Ql = 0.0;
    const double Qp = psi - Ql;
    // psinplus :127, :174
    const double dn = dt * div_with_rcp(-Qp, p.c_dn, p.rcp_cdn);
    // D_t :140-146
    const double lat_melt = p.c_latmelt * wl;
    double lat_grow = ieee_div(-Dk, 2.0 * Lf * hk * ph) * Ql;
    const double weld = p.c_weld * ph * (Dk * Dk * Dk);
    if (hk == 0.0) lat_grow = 0.0;
    const double rD = Dk + (lat_melt + lat_grow + weld) * dt;
    // average :129-134, clamp!, zeroref! (:175-178)
    const double total = n + dn;
    const double rtotal = div_rcp(total);                 // D_n and h_n divide by the same total
    double D_n = div_with_rcp(n * rD + dn * p.Dmin, total, rtotal);
    if (total == 0.0) D_n = 0.0;
    D_n = jl_clamp(D_n, p.Dmin, p.Dmax);
    if (Ei_n == 0.0) D_n = 0.0;
    // thickness :179-181
    double rh = hk + (p.c_ht * Fvi) * dt;
    rh = jl_clamp(rh, 0.0, INFINITY);
    double h_n = div_with_rcp(n * rh + dn * p.hmin, total, rtotal);
    if (total == 0.0) h_n = 0.0;
    const double phi_n = concentration(p, Ei_n, h_n);
    if (h_n == 0.0) Ei_n = 0.0;   // :185
    MizCellOut o;
    o.q[Q_Ei] = Ei_n;
    o.q[Q_Ew] = Ew_n;
    o.q[Q_h] = h_n;
    o.q[Q_D] = D_n;
    o.q[Q_phi] = phi_n;
    o.q[Q_n] = n;
    o.q[Q_E] = phi_n * Ei_n + (1.0 - phi_n) * Ew_n;          // :186
    o.q[Q_T] = Ti * phi_n + (1.0 - phi_n) * Tw;              // :187 (old Ti, Tw; new phi)
    o.q[Q_Ti] = (Ei_n == 0.0) ? __builtin_nan("") : Ti;      // :193
    o.q[Q_Tw] = (phi_n > 0.99) ? __builtin_nan("") : Tw;     // :194
    return o;
}

// Uniform-x operator par.D*get_diffop(nx) applied at cell k in the CSC SpMV order of
// src/infrastructure.jl:495-497 (row k accumulates columns k-1, k, k+1 in that order); tbm/tbp = T
// at k-1 / k+1, g0/g1/g2 the sub-, main and super-diagonal.
__device__ __forceinline__ double diffusion_uniform(int k, int nlat, double g0, double g1, double g2,
                                                    double tbm, double tbk, double tbp) {
    double y = 0.0;
    y = (k > 0) ? y + g0 * tbm : y;
    y = y + g1 * tbk;
    y = (k < nlat - 1) ? y + g2 * tbp : y;
    return 0.0 + y;
}

// Flux through the interface between cells kI-1 (x = xa, T = tba) and kI (x = xb, T = tbb) of the
// non-uniform stencil, src/infrastructure.jl:510-524: (1 - xx^2) dT / dx with the ghost cells
// [-x[1]; x; 2-x[end]] and dT = 0 at the two ends.  Cell k-1 computes it as (mxxph*diffT[i])/diffx[i]
// and cell k as (mxxmh*diffT[i-1])/diffx[i-1]: the same operands in the same order, hence the same
// bits — so it is evaluated once per interface instead of twice.  Also returns xx, the interface
// position (xxph of the left cell, xxmh of the right one).
__device__ __forceinline__ double interface_flux(int kI, int nlat, double xa, double xb, double tba,
                                                 double tbb, double &xx) {
    double lo_x = xa, hi_x = xb, dT = tbb - tba;
    if (kI <= 0) {             // equator: xm = -x[1], diffT[1] = 0
        lo_x = -xb;
        dT = 0.0;
    }
    if (kI >= nlat) {          // pole: xp = 2 - x[end], diffT[end] = 0
        hi_x = 2.0 - xa;
        dT = 0.0;
    }
    xx = (hi_x + lo_x) / 2.0;
    return ieee_div((1.0 - xx * xx) * dT, hi_x - lo_x);
}

// ---- pieces of the MIZ step shared by miz_step_kernel, miz_fused_kernel and miz_resident_kernel --------------
// (one definition each, so that every kernel performs the same operations on the same operands: bit-identical steps)

// The Tbar diffusion term D d/dx[(1-x^2) dTbar/dx] of a thread's cells, visited in increasing order: the uniform operator
// on the identity grid (GRID 0), the non-uniform stencil on any other, which carries the flux and position of the interface
// left of the current cell from one cell to the next.  The caller passes the diagonals g0/g1/g2 of the identity grid's
// operator (unused on other grids): each kernel loads them in its own way.
template <int C, int GRID>
struct TbarStencil {
    double Fl = 0.0, xxl = 0.0;                           // flux / position of the interface left of the current cell
    // the interface left of the chunk: xl, tbl are x and Tbar of the previous chunk's last cell
    __device__ __forceinline__ void start(unsigned k0, int nlat, double xl, const double (&xk)[C], double tbl,
                                          const double (&tb)[C]) {
        if (GRID == 1) Fl = interface_flux((int)k0, nlat, xl, xk[0], tbl, tb[0], xxl);
    }
    // cell i of the chunk; xr, tbr: the next chunk's first cell
    __device__ __forceinline__ double dif(ConstParams &p, int i, unsigned k0, int nlat, const double (&xk)[C], double xr,
                                          const double (&tb)[C], double tbl, double tbr, double g0, double g1,
                                          double g2) {
        const int k = (int)k0 + i;
        const double tbm = left_of(tb, i, tbl), tbp = right_of(tb, i, tbr);
        if (GRID == 0) return diffusion_uniform(k, nlat, g0, g1, g2, tbm, tb[i], tbp);
        double xxr;
        const double Fr = interface_flux(k + 1, nlat, xk[i], right_of(xk, i, xr), tb[i], tbp, xxr);
        const double d = 0.0 + ieee_div(p.D * (Fr - Fl), xxr - xxl);             // :524
        Fl = Fr;
        xxl = xxr;
        return d;
    }
};

// water_temp (src/miz.jl:30) with the NaN -> 0 of :157
__device__ __forceinline__ double water_temperature(ConstParams &p, double Ew, double ph) {
    const double tw = p.Tm + ieee_div(Ew, (1.0 - ph) * p.cw);
    return __builtin_isnan(tw) ? 0.0 : tw;
}
// k/hp + B with hp = (h == 0 ? hmin : h), src/miz.jl:39,41,51
__device__ __forceinline__ double t0_diag_excess(ConstParams &p, double hk) {
    return __builtin_fma(p.k, fast_rcp((hk == 0.0) ? p.hmin : hk), p.B);
}
// right-hand side -(ai S - A + Dif((1-phi)(Tw-Tm)) + f), src/miz.jl:39-43: independent of the active set
__device__ __forceinline__ double t0_rhs(ConstParams &p, double S, double lo, double up, double rm,
                                         double rk, double rp, double f) {
    const double dif = __builtin_fma(up, rp - rk, lo * (rm - rk));
    return -((p.ai * S - p.A) + dif + f);
}
__device__ __forceinline__ double insolation(ConstParams &p, double xk, double ct) {
    return p.S0 - p.S1 * xk * ct - p.S2 * (xk * xk);                         // src/miz.jl:11
}
// The implicit-diffusion extension (IMEX; see miz_step_kernel).  The explicit increment of cell k's total enthalpy,
// dE = dt*(phi*Fvi + (1-phi)*Fvw).  Padding cells (k >= nlat; on a non-uniform grid their stencil is 0/0) must not reach
// the solve: their rows are decoupled but a NaN right-hand side would still spread through the elimination.
__device__ __forceinline__ double enthalpy_increment(ConstParams &p, int k, int nlat, double xk, double ct, double tb,
                                                     double dif, double f, double ph) {
    const VertFlux fv = vert_flux(p, insolation(p, xk, ct), xk, tb, dif, f);
    return k < nlat ? (ph * fv.Fvi + (1.0 - ph) * fv.Fvw) * p.dt : 0.0;
}
// the explicit diffusion term and enthalpy increment of every cell of the chunk (xl, tbl / xr, tbr: the neighbouring
// chunks' cells); on the identity grid the three diagonals are fetched here, not kept across the solve
template <int C, int GRID>
__device__ __forceinline__ void imex_increments(const StepArgs &a, ConstParams &p, const double *geom, unsigned k0, int nlat,
                                                double ct, double f, const double (&xk)[C], double xl, double xr,
                                                const double (&tb)[C], double tbl, double tbr, const double (&ph)[C],
                                                double (&dif)[C], double (&dE)[C]) {
    double g0[GRID == 0 ? C : 1], g1[GRID == 0 ? C : 1], g2[GRID == 0 ? C : 1];
    if constexpr (GRID == 0) {
        unsigned kg = k0;
        asm volatile("" : "+v"(kg));
        load_chunk<C>(geom + G_LO * a.gstride, kg, g0);
        load_chunk<C>(geom + G_DI * a.gstride, kg, g1);
        load_chunk<C>(geom + G_UP * a.gstride, kg, g2);
    }
    TbarStencil<C, GRID> stencil;
    stencil.start(k0, nlat, xl, xk, tbl, tb);
#pragma unroll
    for (int i = 0; i < C; ++i) {
        dif[i] = stencil.dif(p, i, k0, nlat, xk, xr, tb, tbl, tbr, g0[GRID == 0 ? i : 0], g1[GRID == 0 ? i : 0],
                             g2[GRID == 0 ? i : 0]);
        dE[i] = enthalpy_increment(p, (int)k0 + i, nlat, xk[i], ct, tb[i], dif[i], f, ph[i]);
    }
}
// row of I - theta*Dif, theta = dt/cw, from the solver's coefficients lo, up of the cell (padding rows: lo = up = 0,
// decoupled)
__device__ __forceinline__ void imex_row(ConstParams &p, double lo, double up, double &ra, double &rb, double &rc) {
    ra = -(p.theta_imex * lo);
    rc = -(p.theta_imex * up);
    rb = 1.0 + p.theta_imex * (lo + up);
}

// Newton statistics (ebm_newton_stats): thread 0 adds the column's iterations and unconverged steps
__device__ __forceinline__ void count_newton(const StepArgs &a, int col, int t, int nit, int nfail) {
    if (t == 0 && a.counters) {
        unsigned long long *cnt = a.counters + 2 * (col % kCounterShards);
        atomicAdd(cnt, (unsigned long long)nit);
        if (nfail) atomicAdd(cnt + 1, (unsigned long long)nfail);
    }
}

// One active-set Newton iteration (src/miz.jl:33-68): rows for the active set `smask` (bit i <=>
// T0 < Tm in cell i of this thread), tridiagonal solve, new active set; returns whether any thread's
// set changed.  P0/P1 must be free on entry; on exit every thread has passed a barrier after its last
// LDS access.
// COMPACT: P0 = 3T, P1 = T doubles (partition_solve_r); the halo goes through the lane crossbar and P1, the "any set
// changed" vote through words of P0 that nothing writes before the next barrier — no static LDS.
template <int C, int TT, bool COMPACT = false>
__device__ __forceinline__ bool newton_iteration(const double (&lo)[C], const double (&up)[C],
                                                 const double (&dd)[C], const double (&ph)[C],
                                                 const double (&rd)[C], double (&xs)[C], unsigned &smask,
                                                 int t, int T, unsigned k0, int nlat, double *P0, double *P1) {
    double g[C];
#pragma unroll
    for (int i = 0; i < C; ++i) g[i] = ((smask >> i) & 1u) ? ph[i] : 0.0;
    double gl, gr;
    if constexpr (COMPACT) halo_exchange_waves(P1, t, T, g[0], g[C - 1], gl, gr);
    else halo_exchange(P0, P0 + T, t, T, g[0], g[C - 1], gl, gr);
    double ra[C], rb[C], rc[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        ra[i] = lo[i] * left_of(g, i, gl);
        rc[i] = up[i] * right_of(g, i, gr);
        rb[i] = -__builtin_fma(lo[i] + up[i], g[i], dd[i]);
    }
    partition_solve<C, TT, COMPACT>(ra, rb, rc, rd, xs, t, T, P0, P1);
    unsigned snew = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) snew |= (xs[i] < 0.0) ? (1u << i) : 0u;
    const int nvalid = nlat - (int)k0;                // padding rows never count as a change
    snew &= nvalid >= C ? ~0u : (nvalid > 0 ? (1u << nvalid) - 1u : 0u);
    const int changed = snew != smask;
    smask = snew;
    if constexpr (COMPACT) {
        // one word per wave in the last third of P0: free here (the reduction's buffers were read before the solve's
        // last barrier) and next written — by a solve's chunk summaries — only after a halo exchange's barrier
        static_assert(TT > 0 && TT % 64 == 0, "whole waves");
        int *const F = reinterpret_cast<int *>(P0 + 2 * T);
        const bool wave_changed = __builtin_amdgcn_ballot_w64(changed != 0) != 0;
        if ((t & 63) == 0) F[t >> 6] = wave_changed ? 1 : 0;
        __syncthreads();
        int any = 0;
#pragma unroll
        for (int w = 0; w < TT / 64; ++w) any |= F[w];
        return any != 0;
    } else {
        return __syncthreads_or(changed) != 0;
    }
}

// The same iteration for a caller that exchanges g's halo itself and takes the vote itself (the one-step kernels of the
// batched head: g goes round with r on the first pass, and the vote's barrier carries the Tbar halo — ebm_miz_step.h):
// masked_concentration is newton_iteration's g; newton_solve_given_halo forms the rows from it and its halo gl, gr, solves,
// and sets the new active set.  The same expressions in the same order as newton_iteration: the same bits.  Returns whether
// THIS thread's set changed.  P1 must be free on entry and P0 after the solve's first barrier; on exit P0 may still be read
// (partition_solve_r).
template <int C>
__device__ __forceinline__ void masked_concentration(const double (&ph)[C], unsigned smask, double (&g)[C]) {
#pragma unroll
    for (int i = 0; i < C; ++i) g[i] = ((smask >> i) & 1u) ? ph[i] : 0.0;
}
template <int C, int TT>
__device__ __forceinline__ int newton_solve_given_halo(const double (&lo)[C], const double (&up)[C], const double (&dd)[C],
                                                       const double (&g)[C], double gl, double gr, const double (&rd)[C],
                                                       double (&xs)[C], unsigned &smask, int t, int T, unsigned k0, int nlat,
                                                       double *P0, double *P1) {
    double ra[C], rb[C], rc[C];
#pragma unroll
    for (int i = 0; i < C; ++i) {
        ra[i] = lo[i] * left_of(g, i, gl);
        rc[i] = up[i] * right_of(g, i, gr);
        rb[i] = -__builtin_fma(lo[i] + up[i], g[i], dd[i]);
    }
    partition_solve<C, TT>(ra, rb, rc, rd, xs, t, T, P0, P1);
    unsigned snew = 0;
#pragma unroll
    for (int i = 0; i < C; ++i) snew |= (xs[i] < 0.0) ? (1u << i) : 0u;
    const int nvalid = nlat - (int)k0;                // padding rows never count as a change
    snew &= nvalid >= C ? ~0u : (nvalid > 0 ? (1u << nvalid) - 1u : 0u);
    const int changed = snew != smask;
    smask = snew;
    return changed;
}

// ---- savesol! from registers (src/infrastructure.jl:549-591) -----------------------------------
// One pair of cells (2j, 2j+1 of this thread) of every saved quantity: running sum for the annual
// mean (crossmean, src/utilities.jl:390-395: per-cell sum over the year's steps in step order) and/or
// the raw snapshot.  The sums live in a layout private to the library ("pair-split": pair j of
// thread t at col*pitch + j*2T + 2t), so that a wave's read-modify-write covers whole 128-B lines;
// finish_mean_kernel undoes it.  Snapshots use the natural layout (kp = cell index of the pair).
template <int NQ, typename Q>
__device__ __forceinline__ void save_pair(const StepArgs &a, size_t col_off, unsigned split, unsigned kp,
                                          const Q &c0, const Q &c1, bool v0, bool v1) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int v = a.var_of[q];                        // wave-uniform (kernel argument)
        if (v < 0) continue;
        const double x0 = v0 ? c0.q[q] : 0.0, x1 = v1 ? c1.q[q] : 0.0;     // padding cells stay zero
        if (a.sums) {
            double2 *sp = reinterpret_cast<double2 *>(a.sums + (size_t)v * a.sum_stride + col_off + split);
            double2 s = *sp;
            s.x = s.x + x0;
            s.y = s.y + x1;
            *sp = s;
        }
        if (a.stage) {
            double2 d;
            d.x = x0;
            d.y = x1;
            EBM_STORE2(a.stage + (size_t)v * a.stage_var_stride + a.stage_offset + col_off + kp, d);
        }
    }
}

}  // namespace ebm
