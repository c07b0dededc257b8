// miz_resident_kernel: K MIZ steps per launch, the state resident in LDS.
#pragma once
#include "ebm_miz_pieces.h"

namespace ebm {

// Fused-K MIZ stepping for the meridians the register kernel (miz_fused_kernel) cannot hold (more than kFusedRegThreads threads
// at four cells per thread: 2049 ... 4096 cells), for the implicit-diffusion extension at every size, and for launches of
// many shorter meridians (LaunchCfg::fused_in_lds: at 128 VGPRs several workgroups share a CU): a.nfused steps
// in one launch with the state RESIDENT IN LDS — Ei, Ew, h, D of every cell (cell i of thread t at i*T + t, 16 T doubles),
// phi in registers.  What the per-step kernel spends its LDS on is cut to fit beside that: the solve runs in 4 T doubles
// instead of 6 T (partition_solve_r<COMPACT>: one more barrier), the halo exchanges go through the lane crossbar and 32
// words, the "any set changed" vote through words of the solve's buffer instead of the compiler's static LDS, and Tw is
// formed again for the cell updates (one division) instead of being stashed: 20 T doubles = exactly the CU's 160 KiB at
// T = 1024.  Global memory is touched at the start (state in), at the end (state out, diagnostics of the last step if
// write_diag) and by the per-step table loads (L2 hits).  Every step performs the operations of miz_step_kernel in the
// same order on the same values: bit-identical results (tests: test_fused_run_equals_single_steps, test_every_workgroup_size).
//
// SAVE: savesol!'s annual-mean running sums taken from every step of the launch (save_pair, as in miz_step_kernel<OUT_SAVE>:
// the same per-cell sum in step order, the same bits) — what ebm_integrate launches for the stretches of a year that need
// nothing else (no raw snapshot, no seasonal snapshot).  At four waves per SIMD for every workgroup size: this variant is
// bound by the sums' read-modify-write traffic (16 B per saved variable and cell-step) and wants the occupancy.
// Up to 512 threads every variant is held to four waves per SIMD (128 VGPRs): there the kernel exists FOR its occupancy —
// several workgroups per CU fill each other's barrier stalls (0.1278 -> 0.1121 ms per step on 2048 x 4096 against the
// register kernel, 0.304 -> 0.209 on 1024 x 16384) — and is chosen for launches of many columns (LaunchCfg::fused_in_lds).
template <int GRID, int TT, bool IMEX, bool SAVE = false>
__global__ void __launch_bounds__(TT, (SAVE || TT <= 512) ? 4 : 1) miz_resident_kernel(const StepArgs a) {
    constexpr int C = 4, T = TT;
    extern __shared__ double smem[];
    const int t = threadIdx.x, col = step_column(a);
    const int nlat = a.nlat;
    const unsigned k0 = (unsigned)t * C;
    double *const PA = smem, *const PB = smem + 3 * T;    // the solve's 3T + T
    // The state words: field F (Ei, Ew, h, D) of cell i of this thread at double (4 + 4F + i)*T + t.  A ds instruction
    // reaches 64 KiB from its address register: one opaque base per 64 KiB window (three at T = 1024) and compile-time
    // offsets, instead of one address register per word kept across the step loop.
    typedef __attribute__((address_space(3))) double lds_double;
    lds_double *win[3];
    // (formed again at every phase that touches the state, from that phase's own copy of the thread index: three
    // integer additions instead of three registers held across the solves)
    auto windows = [&](int tx) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            win[j] = (lds_double *)smem + (j * 8192 + tx);
            asm volatile("" : "+v"(win[j]));
        }
    };
    windows(t);
#define EBM_RES(F, i) win[((4 + 4 * (F) + (i)) * T) >> 13][((4 + 4 * (F) + (i)) * T) & 8191]
#define sEi(i) EBM_RES(0, i)
#define sEw(i) EBM_RES(1, i)
#define sh(i) EBM_RES(2, i)
#define sD(i) EBM_RES(3, i)
    const int pset = param_set(a, col);                  // ebm_set_column_params (set 0 without a table)
    ConstParams &p = *reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p + pset));
    const double *const geom = a.geom + pset * a.set_stride;
    const double *const gX = geom + G_X * a.gstride;
    double *const st = a.state + (size_t)col * (size_t)a.pitch;
    const double Tm = p.Tm;
    ColumnNoise nz;                                                    // N_c in memory (noise_sequence_kernel)
    unsigned short *const cmask = a.amask + (size_t)col * T;           // wave-uniform
    unsigned smask = cmask[t];
    double ph[C];
    {
        double v[C];
        load_chunk<C>(st + S_Ei * a.fstride, k0, v);
#pragma unroll
        for (int i = 0; i < C; ++i) sEi(i) = v[i];
        load_chunk<C>(st + S_Ew * a.fstride, k0, v);
#pragma unroll
        for (int i = 0; i < C; ++i) sEw(i) = v[i];
        load_chunk<C>(st + S_h * a.fstride, k0, v);
#pragma unroll
        for (int i = 0; i < C; ++i) sh(i) = v[i];
        load_chunk<C>(st + S_D * a.fstride, k0, v);
#pragma unroll
        for (int i = 0; i < C; ++i) sD(i) = v[i];
        load_chunk<C>(st + S_phi * a.fstride, k0, ph);
    }
    int nit = 0, nfail = 0;
    const int nloop = a.nfused;
    int ts = t;
    for (int step = 0; step < nloop; ++step) {
        // the step's scalars, read through the constant address space (the table is written by the host before the launch,
        // never by a kernel): scalar loads into SGPRs — through the plain pointer they would be per-lane vector loads once
        // the kernel has stored anything, and ct and f would occupy four VGPRs for the whole step
        typedef const __attribute__((address_space(4))) StepSched ConstSched;
        ConstSched &sc = *reinterpret_cast<ConstSched *>(reinterpret_cast<uintptr_t>(a.sched + (a.slot + step)));
        const double ct = sc.ct;
        // (the column's forcing is the same in every lane: moved to SGPRs — the column offset and schedule are read
        // through plain pointers, i.e. by vector loads)
        double fv = column_forcing(a, col, sc.ft, sc.tyear);
        if (a.noise) fv = fv + nz.at_step<true>(a, col, step, sc.n);
        const double f = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(fv)),
                                          __builtin_amdgcn_readfirstlane(__double2loint(fv)));
        const bool diag = a.write_diag != 0 && step + 1 == nloop;
        // The thread index is made opaque once per step: everything derived from it — the solve's neighbour rows at every
        // level of the reduction, the transposed interface slots — is formed again in the step (a handful of integer
        // operations) instead of being hoisted out of the step loop and kept in some thirty registers.
        asm volatile("" : "+v"(ts));
        const unsigned ks = (unsigned)ts * C;
        // ---------------- phases A and B, as in miz_step_kernel ----------------
        double rd[C], xs[C];
        int it = 0;
        bool again;
        do {
            double tlo[C], tup[C], dd[C];
            // (the lane's cell index is made opaque at every group of table loads: the per-latitude tables are fetched
            // again — L2 hits — through the wave-uniform base + 32-bit offset form, instead of living in registers, or
            // their per-lane 64-bit addresses, across the solve and the steps)
            unsigned kl = ks;
            asm volatile("" : "+v"(kl));
            windows(ts);
            load_chunk<C>(geom + G_LO * a.gstride, kl, tlo);
            load_chunk<C>(geom + G_UP * a.gstride, kl, tup);
            if (it == 0) {
                double xk[C], r[C];
                load_chunk<C>(gX, kl, xk);
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const double tw = water_temperature(p, sEw(i), ph[i]);
                    dd[i] = t0_diag_excess(p, sh(i));
                    r[i] = (1.0 - ph[i]) * (tw - Tm);
                }
                double rl, rr;
                halo_exchange_waves(PB, ts, T, r[0], r[C - 1], rl, rr);
#pragma unroll
                for (int i = 0; i < C; ++i)
                    rd[i] = t0_rhs(p, insolation(p, xk[i], ct), tlo[i], tup[i], left_of(r, i, rl), r[i], right_of(r, i, rr), f);
                __syncthreads();                                 // the halo words are rewritten by the iteration
            } else {
#pragma unroll
                for (int i = 0; i < C; ++i) dd[i] = t0_diag_excess(p, sh(i));
            }
            ++it;
            again = newton_iteration<C, TT, true>(tlo, tup, dd, ph, rd, xs, smask, ts, T, ks, nlat, PA, PB);
        } while (it < kMaxNewton && again);
        nit += it;
        nfail += again ? 1 : 0;
        // ---------------- phase D ----------------
        int td = ts;                                      // phase D's own copy: nothing index-derived crosses the solve
        asm volatile("" : "+v"(td));
        unsigned kl = (unsigned)td * C;
        windows(td);
        double xk[C];
        load_chunk<C>(gX, kl, xk);
        double xl = gX[kl > 0 ? kl - 1 : 0], xr = gX[kl + C];
        double g0[GRID == 0 ? C : 1], g1[GRID == 0 ? C : 1], g2[GRID == 0 ? C : 1];
        double tb[C];
        {
            double T0[C];
#pragma unroll
            for (int i = 0; i < C; ++i) {
                T0[i] = xs[i] + Tm;                                       // new warm start, :64
                const double ti = jl_min(T0[i], Tm);                      // ice_temp, :31,65
                xs[i] = (sh(i) == 0.0) ? 0.0 : ti;                    // Ti: zeroref!, :66
                const double tw = water_temperature(p, sEw(i), ph[i]);  // the value phase A formed
                tb[i] = xs[i] * ph[i] + (1.0 - ph[i]) * tw;               // Tbar, :21-26
            }
            if (diag) store_chunk<C>(st + S_T0 * a.fstride, T0, kl, nlat);
        }
        double tbl, tbr;
        halo_exchange_waves(PB, td, T, tb[0], tb[C - 1], tbl, tbr);
        double difx[IMEX ? C : 1];
        if constexpr (IMEX) {
            // the extension's second solve, as in miz_step_kernel; nothing is parked here (no LDS is left): the explicit
            // increment is evaluated a second time after the solve — same operands, same operations, same bits
            double sol[C];
            {
                double ra[C], rb[C], rc[C], dE[C], dif[C], qlo[C], qup[C];
                load_chunk<C>(geom + G_LO * a.gstride, kl, qlo);
                load_chunk<C>(geom + G_UP * a.gstride, kl, qup);
                imex_increments<C, GRID>(a, p, geom, kl, nlat, ct, f, xk, xl, xr, tb, tbl, tbr, ph, dif, dE);
#pragma unroll
                for (int i = 0; i < C; ++i) imex_row(p, qlo[i], qup[i], ra[i], rb[i], rc[i]);
                partition_solve<C, TT, true>(ra, rb, rc, dE, sol, ts, T, PA, PB);
            }
            __syncthreads();                                  // the solve's last LDS reads are done
            {
                // Only Ti (xs), phi, the two halo values of Tbar and the solution crossed the solve in registers: x is
                // fetched again (the lane's cell index made opaque, so that the reloads are real), Tw and Tbar are formed
                // again from the state words
                int tq = ts;
                asm volatile("" : "+v"(tq));
                const unsigned kq = (unsigned)tq * C;
                windows(tq);
                load_chunk<C>(gX, kq, xk);
                xl = gX[kq > 0 ? kq - 1 : 0];
                xr = gX[kq + C];
                kl = kq;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const double tw = water_temperature(p, sEw(i), ph[i]);
                    tb[i] = xs[i] * ph[i] + (1.0 - ph[i]) * tw;
                }
                double dif[C], dE[C];
                imex_increments<C, GRID>(a, p, geom, kl, nlat, ct, f, xk, xl, xr, tb, tbl, tbr, ph, dif, dE);
#pragma unroll
                for (int i = 0; i < C; ++i) difx[IMEX ? i : 0] = dif[i] + div_with_rcp(sol[i] - dE[i], p.dt, p.rcp_dt);
            }
        }
        TbarStencil<C, GRID> stencil;
        stencil.start(kl, nlat, xl, xk, tbl, tb);
        [[maybe_unused]] MizCellOut o_even;                           // SAVE: the pair's first cell waits for its second
        [[maybe_unused]] bool v_even = false;
#pragma unroll
        for (int i = 0; i < C; ++i) {
            __builtin_amdgcn_sched_barrier(0);                         // one cell at a time: bounded live ranges
            const int k = (int)kl + i;
            const double S = insolation(p, xk[i], ct);
            double dif;
            if constexpr (IMEX) {
                dif = difx[IMEX ? i : 0];
            } else {
                // the three diagonals of the cell's pair arrive with its first cell (16-byte loads, L2 hits), not all
                // twelve words before the loop
                if (GRID == 0 && (i & 1) == 0) {
                    const double2 q0 = *reinterpret_cast<const double2 *>(geom + G_LO * a.gstride + (kl + i));
                    const double2 q1 = *reinterpret_cast<const double2 *>(geom + G_DI * a.gstride + (kl + i));
                    const double2 q2 = *reinterpret_cast<const double2 *>(geom + G_UP * a.gstride + (kl + i));
                    g0[GRID == 0 ? i : 0] = q0.x;  g0[GRID == 0 ? i + 1 : 0] = q0.y;
                    g1[GRID == 0 ? i : 0] = q1.x;  g1[GRID == 0 ? i + 1 : 0] = q1.y;
                    g2[GRID == 0 ? i : 0] = q2.x;  g2[GRID == 0 ? i + 1 : 0] = q2.y;
                }
                dif = stencil.dif(p, i, kl, nlat, xk, xr, tb, tbl, tbr, g0[GRID == 0 ? i : 0], g1[GRID == 0 ? i : 0],
                                  g2[GRID == 0 ? i : 0]);
            }
            const double tw = water_temperature(p, sEw(i), ph[i]);      // and a third time: one division, no register
            const MizCellOut o = miz_cell_update(p, f, S, xk[i], dif, tb[i], sEi(i), sEw(i), sh(i),
                                                 sD(i), ph[i], tw, xs[i]);
            const bool valid = k < nlat;                               // padding cells stay zero
            sEi(i) = valid ? o.q[Q_Ei] : 0.0;
            sEw(i) = valid ? o.q[Q_Ew] : 0.0;
            sh(i) = valid ? o.q[Q_h] : 0.0;
            sD(i) = valid ? o.q[Q_D] : 0.0;
            ph[i] = valid ? o.q[Q_phi] : 0.0;
            if (diag) {
                // last step of the run only (wave-uniform base + the per-step opaque 32-bit cell index: no per-lane
                // 64-bit addresses for the compiler to hoist out of the step loop and keep in registers; kept out of a
                // helper shared with miz_fused_kernel: in one, it changes how hipcc peels this kernel's first Newton
                // iteration)
                (st + S_n * a.fstride)[kl + i] = valid ? o.q[Q_n] : 0.0;
                (st + S_E * a.fstride)[kl + i] = valid ? o.q[Q_E] : 0.0;
                (st + S_T * a.fstride)[kl + i] = valid ? o.q[Q_T] : 0.0;
                (st + S_Ti * a.fstride)[kl + i] = valid ? o.q[Q_Ti] : 0.0;
                (st + S_Tw * a.fstride)[kl + i] = valid ? o.q[Q_Tw] : 0.0;
            }
            if constexpr (SAVE) {
                if ((i & 1) == 0) {
                    o_even = o;
                    v_even = valid;
                } else {
                    save_pair<Q_MIZ_COUNT>(a, (size_t)col * (size_t)a.pitch, (unsigned)((i / 2) * 2 * T) + 2u * (unsigned)td,
                                           kl + (unsigned)(i - 1), o_even, o, v_even, valid);
                }
            }
        }
        __syncthreads();                                               // the halo words are rewritten by the next step
    }
    {
        // (indices made opaque: the addresses are formed here, not kept — and spilled — across the step loop)
        unsigned tl = (unsigned)ts;
        asm volatile("" : "+v"(tl));
        const unsigned ke = tl * C;
        windows((int)tl);
        double v[C];
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = sEi(i);
        store_chunk<C>(st + S_Ei * a.fstride, v, ke, nlat);
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = sEw(i);
        store_chunk<C>(st + S_Ew * a.fstride, v, ke, nlat);
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = sh(i);
        store_chunk<C>(st + S_h * a.fstride, v, ke, nlat);
#pragma unroll
        for (int i = 0; i < C; ++i) v[i] = sD(i);
        store_chunk<C>(st + S_D * a.fstride, v, ke, nlat);
        store_chunk<C>(st + S_phi * a.fstride, ph, ke, nlat);
        cmask[tl] = (unsigned short)smask;
    }
    count_newton(a, col, ts, nit, nfail);
}
#undef sEi
#undef sEw
#undef sh
#undef sD
#undef EBM_RES

}  // namespace ebm
