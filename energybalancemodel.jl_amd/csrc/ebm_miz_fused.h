// miz_fused_kernel: K MIZ steps per launch, the state in registers.
#pragma once
#include "ebm_miz_pieces.h"

namespace ebm {

// Fused-K MIZ stepping for meridians of up to 4*kFusedRegThreads cells: a.nfused steps in one launch
// with the whole state (5 prognostics, the active set, the per-latitude tables) in registers between
// steps — 256 VGPRs per lane at <= 512 threads with four cells per thread, 166 at 768 threads with two
// (1025 ... 1536-cell meridians) — and LDS used only by the solve and the halo
// exchanges.  Global memory is touched at the start (state in), at the end (state out, diagnostics of
// the last step if write_diag) and by the scalar loads of the per-step table.  Every step performs the
// operations of miz_step_kernel in the same order on the same values: bit-identical results
// (tests: test_fused_run_equals_single_steps).
// SAVE (two cells per thread only — what a caller asks for to run ONE short meridian): savesol!'s running sums from every
// step of the launch, as in miz_resident_kernel<SAVE>; with two cells per thread the thread's chunk IS the pair.
template <int C, int GRID, int TT, bool SAVE = false>
__global__ void __launch_bounds__(TT) miz_fused_kernel(const StepArgs a) {
    static_assert(!SAVE || C == 2, "the savesol! variant of the register kernel exists for two cells per thread");
    static_assert(C == 2 || C == 4, "cells per thread");
    constexpr int T = TT;
    constexpr bool kNoiseMem = TT > kFusedRegThreads;                 // 168 VGPRs at three waves per SIMD: N_c in memory
    extern __shared__ double smem[];
    const int t = threadIdx.x, col = step_column(a);
    const int nlat = a.nlat;
    const unsigned k0 = (unsigned)t * C;
    double *P0 = smem, *P1 = smem + 3 * T;
    const int pset = param_set(a, col);                  // ebm_set_column_params (set 0 without a table)
    ConstParams &p = *reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p + pset));
    const double *const geom = a.geom + pset * a.set_stride;
    const double *const gX = geom + G_X * a.gstride;
    double *const st = a.state + (size_t)col * (size_t)a.pitch;
    const double Tm = p.Tm;
    ColumnNoise nz;
    if (!kNoiseMem && a.noise) {                                       // before the state is loaded, and any barrier
        nz.load(a, col);
        nz.prepare_launch(a, a.nfused);
    }
    unsigned short *const wmask = a.amask + (size_t)col * T + t;
    unsigned smask = *wmask;
    double Ei[C], Ew[C], hk[C], Dk[C], ph[C], xk[C], tlo[C], tup[C];
    double g1[GRID == 0 ? C : 1];
    load_chunk<C>(st + S_Ei * a.fstride, k0, Ei);
    load_chunk<C>(st + S_Ew * a.fstride, k0, Ew);
    load_chunk<C>(st + S_h * a.fstride, k0, hk);
    load_chunk<C>(st + S_D * a.fstride, k0, Dk);
    load_chunk<C>(st + S_phi * a.fstride, k0, ph);
    load_chunk<C>(gX, k0, xk);
    load_chunk<C>(geom + G_LO * a.gstride, k0, tlo);   // == G_0 / G_2 on the identity grid (build_tables)
    load_chunk<C>(geom + G_UP * a.gstride, k0, tup);
    if constexpr (GRID == 0) load_chunk<C>(geom + G_DI * a.gstride, k0, g1);
    const double xl = gX[k0 > 0 ? k0 - 1 : 0], xr = gX[k0 + C];
    int nit = 0, nfail = 0;
    const int nloop = a.nfused;
    for (int step = 0; step < nloop; ++step) {
        const StepSched sc = a.sched[a.slot + step];                   // scalar loads
        if constexpr (TT > 256) {
            // 256 VGPRs per lane: not enough to also keep the step-invariant stencil geometry (interface
            // positions, their reciprocals) that the compiler would hoist out of the step loop — make x
            // opaque once per step so that it is recomputed like in the per-step kernel
#pragma unroll
            for (int i = 0; i < C; ++i) asm volatile("" : "+v"(xk[i]));
        }
        const double ct = sc.ct;
        double f = column_forcing(a, col, sc.ft, sc.tyear);
        if (a.noise) f = f + nz.at_step<kNoiseMem>(a, col, step, sc.n);
        const bool diag = a.write_diag && step == nloop - 1;
        // phase A
        double tw[C], dd[C], r[C], rd[C], xs[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            tw[i] = water_temperature(p, Ew[i], ph[i]);
            dd[i] = t0_diag_excess(p, hk[i]);
            r[i] = (1.0 - ph[i]) * (tw[i] - Tm);
        }
        double rl, rr;
        halo_exchange(P0, P0 + T, t, T, r[0], r[C - 1], rl, rr);
#pragma unroll
        for (int i = 0; i < C; ++i)
            rd[i] = t0_rhs(p, insolation(p, xk[i], ct), tlo[i], tup[i], left_of(r, i, rl), r[i], right_of(r, i, rr), f);
        __syncthreads();
        // phase B
        int it = 0;
        bool again = true;
        while (again && it < kMaxNewton) {
            ++it;
            again = newton_iteration<C, TT>(tlo, tup, dd, ph, rd, xs, smask, t, T, k0, nlat, P0, P1);
        }
        nit += it;
        nfail += again ? 1 : 0;
        // phase D
        double tb[C];
        {
            double T0[C];
#pragma unroll
            for (int i = 0; i < C; ++i) {
                T0[i] = xs[i] + Tm;
                const double ti = jl_min(T0[i], Tm);
                xs[i] = (hk[i] == 0.0) ? 0.0 : ti;
                tb[i] = xs[i] * ph[i] + (1.0 - ph[i]) * tw[i];
            }
            if (diag) store_chunk<C>(st + S_T0 * a.fstride, T0, k0, nlat);
        }
        double tbl, tbr;
        halo_exchange(P0, P0 + T, t, T, tb[0], tb[C - 1], tbl, tbr);
        TbarStencil<C, GRID> stencil;
        stencil.start(k0, nlat, xl, xk, tbl, tb);
        [[maybe_unused]] MizCellOut o_even;                            // SAVE: the pair's first cell waits for its second
        [[maybe_unused]] bool v_even = false;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            __builtin_amdgcn_sched_barrier(0);                         // one cell at a time: bounded live ranges
            const int k = (int)k0 + i;
            const double S = insolation(p, xk[i], ct);
            const double dif = stencil.dif(p, i, k0, nlat, xk, xr, tb, tbl, tbr, tlo[i], g1[GRID == 0 ? i : 0], tup[i]);
            const MizCellOut o = miz_cell_update(p, f, S, xk[i], dif, tb[i], Ei[i], Ew[i], hk[i], Dk[i], ph[i],
                                                 tw[i], xs[i]);
            const bool valid = k < nlat;                               // padding cells stay zero
            if constexpr (SAVE) {
                if (i == 0) {
                    o_even = o;
                    v_even = valid;
                } else {
                    save_pair<Q_MIZ_COUNT>(a, (size_t)col * (size_t)a.pitch, 2u * (unsigned)t, k0, o_even, o, v_even, valid);
                }
            }
            Ei[i] = valid ? o.q[Q_Ei] : 0.0;
            Ew[i] = valid ? o.q[Q_Ew] : 0.0;
            hk[i] = valid ? o.q[Q_h] : 0.0;
            Dk[i] = valid ? o.q[Q_D] : 0.0;
            ph[i] = valid ? o.q[Q_phi] : 0.0;
            if (diag) {                                                // last step of the run only
                st[S_n * a.fstride + k] = valid ? o.q[Q_n] : 0.0;
                st[S_E * a.fstride + k] = valid ? o.q[Q_E] : 0.0;
                st[S_T * a.fstride + k] = valid ? o.q[Q_T] : 0.0;
                st[S_Ti * a.fstride + k] = valid ? o.q[Q_Ti] : 0.0;
                st[S_Tw * a.fstride + k] = valid ? o.q[Q_Tw] : 0.0;
            }
        }
        __syncthreads();                                               // halo words are rewritten by the next step
    }
    store_chunk<C>(st + S_Ei * a.fstride, Ei, k0, nlat);
    store_chunk<C>(st + S_Ew * a.fstride, Ew, k0, nlat);
    store_chunk<C>(st + S_h * a.fstride, hk, k0, nlat);
    store_chunk<C>(st + S_D * a.fstride, Dk, k0, nlat);
    store_chunk<C>(st + S_phi * a.fstride, ph, k0, nlat);
    *wmask = (unsigned short)smask;
    if (!kNoiseMem && a.noise) nz.store(a, col);                        // after the launch's last barrier
    count_newton(a, col, t, nit, nfail);
}

}  // namespace ebm
