// miz_step_kernel: one MIZ step per launch.
#pragma once
#include "ebm_miz_pieces.h"

// A/B builds of the first Newton pass's two exchanges (MERGE_RG, TBAR_VOTE in miz_step_kernel): =0 gives the order before them
#ifndef EBM_MERGE_RG
#define EBM_MERGE_RG 1
#endif
#ifndef EBM_TBAR_VOTE
#define EBM_TBAR_VOTE 1
#endif

namespace ebm {

// MIZ step: one workgroup per meridian.
//
// Geometry (choose_launch): C = 4 cells per thread, T = ceil(nlat/4 / 64)*64 <= 1024 threads (<= 128
// VGPRs).  A 4096-cell fp64 meridian fills a CU (512 KiB of VGPRs + 160 KiB of LDS): one workgroup per
// CU; shorter meridians run several workgroups per CU, which overlap each other.  Longer meridians
// do not fit one workgroup and are refused (EBM_ERR_UNSUPPORTED).
//
// LDS map (doubles; per-cell arrays hold cell i of thread t at i*T + t: lane-consecutive,
// conflict-free):
//   P0 = [0,3T), P1 = [3T,6T)    cyclic-reduction ping-pong; idle otherwise, then borrowed for
//                                the r / g / Tbar halo exchanges.  BATCH_HEAD, first Newton pass: r's two words and g's
//                                first in P0[0, 3T), g's last in P1[0, T), one barrier for both (halo_exchange_two);
//                                above 256 threads Tbar's two words in P1[0, 2T), published after the solve's last
//                                barrier and before the active-set vote, whose barrier is the exchange's
//                                (publish_then_vote): 16 barriers on the one-solve path at T = 1024 where 18 stood
//                                (the barrier plan)
//   sEw, sh, sTw = [6T, 6T+3CT)  Ew, h, Tw of every cell, parked across the T0 solve so that the
//                                solve has the register file to itself
//
// OUT (OutMode): what is written besides the prognostics (OUT_STATE, OUT_DIAG, OUT_SAVE).
// TT: workgroup size, a compile-time constant (LDS offsets become immediates).
//
// IMEX: the implicit-diffusion EXTENSION (model EBM_MODEL_MIZ_IMEX; not in the reference — defined in
// include/ebm_hip.h): before the cell updates the explicit increment of
// every cell's total enthalpy, dE = dt*(phi*Fvi + (1-phi)*Fvw), goes through one more tridiagonal solve per
// meridian, (I - (dt/cw)*Dif) dE_new = dE — the same partition + cyclic reduction as the T0 system — and the
// diffusion term of both vertical fluxes is corrected by (dE_new - dE)/dt.  Lifts the explicit limit
// dt <= cw*dx^2/(2D) of the reference's step.
// __launch_bounds__(TT, 4): the workgroup size is the compile-time TT, never more; four waves per SIMD keep the
// 128-VGPR budget that lets a 1024-thread workgroup (and four 256-thread ones) share a CU.
//
// PHI_DERIVED (four cells per thread, the reference's step, OUT_STATE): phi is neither loaded nor stored.  After any step
// phi is concentration(Ei, h) of the stored Ei and h (ebm_miz_pieces.h), so phase A loads Ei instead and forms it, and
// phase D stores four fields instead of five: a fifth of the store traffic of a launch.  The phi field in HBM goes stale;
// the runtime launches this variant only on a state that step kernels wrote last and restores the field before anybody
// else reads it (ebm_ctx::phi_stored).
//
// ZERO_LINES (the PHI_DERIVED kernel only): state lines that hold nothing but zero bits are neither loaded nor stored.  A
// wave's access to pair j of one field covers 1 KiB of the column in the pair-split layout (128 cells); one flag per (column,
// wave, pair, field of Ei, Ew, h, D) — eight bits of the wave's flag word, zero_flag_bit — says that this KiB holds only
// zero bits in HBM.  The word is read once with a scalar load; a flagged pair is not loaded (+0.0 is what the load would
// have returned), and is not stored if its new values are all zero bits again (padding cells store +0.0 and count as
// zero).  The new word — the ballots of what the wave holds now, stored or not — is written by one lane after the last
// store.  The branches around loads and stores are wave-uniform (only the prefetch below is predicated per lane: the two
// halves of a wave fetch for two different lines); HBM stays complete and current, so no reader of the fields changes.  The flags
// know nothing about the physics: ice-free cells store Ei = h = D = +0.0, water at the freezing point under ice Ew = +0.0.
// Whoever else writes a prognostic field, or moves it to another layout, leaves the flags untrusted, and the runtime clears
// them before the next launch of this variant (FieldBook::zero_flags_trusted).  The L2 prefetch for the
// successor column skips, lane by lane, the sectors of lines that the successor's flags say it will not load.
//
// Order of requests in phase A (BATCH_HEAD: four cells per thread, the reference's step; IMEX and the two-cell kernels keep
// the head they had): a phase requests its inputs before anything that waits or writes.  The scalar words of the
// head in one batch behind one wait (StepHead), then the state, the mask word, the tables; the forcing, the noise record and
// Tm under the loads' latency.  Phase D keeps the order below: x, Ei and D requested ahead of the mask store and the
// counters' atomic, and ahead of the halo, measured 2.2 % slower on the headline (profiles/EXPERIMENTS.md, r30).
//
// Order of loads and stores in phase D (four cells per thread): after the Tbar halo a lane requests Ei and D of BOTH its
// pairs (flagged pairs excepted), then updates pair 0, stores it, updates pair 1 (the L2 prefetch for the successor leaves
// within it), stores it.  No load of the state follows a store.  IMEX, OUT_SAVE and the two-cell kernels
// request a pair's Ei and D at the top of that pair (see EARLY below).
template <int C, int GRID, int OUT, int TT, bool IMEX, bool PHI_DERIVED = false, bool ZERO_LINES = false>
__global__ void __launch_bounds__(TT, 4) miz_step_kernel(const StepArgs a) {
    static_assert(C == 2 || C == 4, "cells per thread");
    static_assert(!PHI_DERIVED || (C == 4 && !IMEX && OUT == OUT_STATE), "phi is derived by the state-only kernel of the reference's step");
    static_assert(!ZERO_LINES || PHI_DERIVED, "zero lines are elided by the kernel that derives phi");
    static_assert(OUT == OUT_STATE || OUT == OUT_DIAG || OUT == OUT_SAVE, "per-step kernel");
    constexpr bool MAYDIAG = OUT != OUT_STATE;            // diagnostic stores compiled in
    extern __shared__ double smem[];
    constexpr int T = TT;
    const int t = threadIdx.x, col = a.col0 + (int)blockIdx.x;
    const int nlat = a.nlat;
    const unsigned k0 = (unsigned)t * C;
    double *P0 = smem, *P1 = smem + 3 * T;
    double *sEw = smem + 6 * T + t, *sh = sEw + C * T, *sTw = sh + C * T;
    EBM_STAMP(0);
    EBM_STAMPW(0);                                        // per wave: first instruction
    // The head: every scalar word that depends only on the launch arguments and the column — this wave's zero-line flag word
    // and the successor column's two (ZERO_LINES: scalar loads, like the parameter block: nothing of them waits in a VGPR), the
    // step's scalars, the column's forcing offset and parameter set — in one batch behind one wait (StepHead, ebm_device.h).
    // What needs more than that (the forcing schedule, the noise, Tm) follows phase A's vector requests.
    // BATCH_HEAD: the four-cell kernels of the reference's step.  IMEX and the two-cell kernels keep the head they had — every
    // word asked for where it is first used, the forcing before the loads, the loads inside the Newton loop
    // (step_head_in_place): with the batch the IMEX headline shape measured 0.85 % slower, twice, and the two-cell kernels
    // need up to 28 more VGPRs, five waves per SIMD becoming four (profiles/EXPERIMENTS.md, r30).
    constexpr bool BATCH_HEAD = C == 4 && !IMEX;
    static_assert(BATCH_HEAD || !ZERO_LINES, "the eliding kernel has the batched head");
    static_assert(BATCH_HEAD || !PHI_DERIVED, "the in-place head loads phi, never Ei");
    // MERGE_RG, TBAR_VOTE: the two barriers the batched-head kernels leave out of the first Newton pass (see the loop below).
    // -DEBM_MERGE_RG=0 / -DEBM_TBAR_VOTE=0 give the order before them, for A/B builds.
    // TBAR_VOTE only above 256 threads: at 256, where four workgroups share a CU and fill each other's barrier intervals, the
    // 1024 x 16384 shape measured 0.6 % SLOWER with it, twice, and neither faster nor slower with MERGE_RG alone
    // (profiles/EXPERIMENTS.md, r34); at 512 (two per CU) and 1024 (one) the two together are faster.
    constexpr bool MERGE_RG = BATCH_HEAD && EBM_MERGE_RG, TBAR_VOTE = BATCH_HEAD && TT > 256 && EBM_TBAR_VOTE;
    StepHead hd;
    if constexpr (BATCH_HEAD) hd = step_head<ZERO_LINES, TT>(a, col, (unsigned)__builtin_amdgcn_readfirstlane(t >> 6));
    else hd = step_head_in_place(a, col);
    const int pset = hd.pset;                            // ebm_set_column_params (set 0 without a table)
    ConstParams &p = *reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p + pset));
    const double *const geom = a.geom + pset * a.set_stride;
    const double *const gX = geom + G_X * a.gstride;
    double *const st = a.state + (size_t)col * (size_t)a.pitch;         // wave-uniform
    // Warm start (src/miz.jl:47,52-54,64).  The reference carries T0 itself between steps; the
    // active-set iteration only uses its sign pattern, so between steps the library carries that
    // pattern (one bit per cell) and writes the fp64 T0 field on diagnostic launches only.
    unsigned short *const cmask = a.amask + (size_t)col * T;            // wave-uniform
    const unsigned zold = hd.zold, znext0 = hd.znext0, znext1 = hd.znext1;
    unsigned znew = 0;
    const double ct = hd.ct;                              // per-step scalars
    const bool diag = OUT == OUT_DIAG || (MAYDIAG && a.write_diag);

    // ---------------- phase A: loads, water temperature, T0-system coefficients ----------
    // Only phi and the right-hand side stay in registers across the solve; Ew, h, Tw wait in the
    // LDS stash.  The second and later Newton iterations (a changed active set: < 0.1 % of column-steps at the
    // reference's time steps, every second one with the extension's long ones) form the rows again from the stashed h
    // and the two coefficient tables and call the same solve — one copy of the solve in the kernel.
    // Order of the requests (first iteration): the state (Ew, Ei or phi, h: their first consumers, concentration and
    // water_temperature, come long before the tables' — after the r halo), the mask word, then the geometry (tlo, tup, x);
    // the forcing, the noise record and Tm are formed under the loads' latency, before their first use.  The
    // sched_barriers pin that order; tests/test_host_step_head_order.py reads it in the assembly.
    // (they stand before the Newton loop, not in its first iteration: with the forcing inside it the loop's body is too
    // large for hipcc to peel that iteration, and the whole kernel spills)
    double ph[C], rd[C], xs[C];
    double Ew[C], hk[C], xk0[C], tlo0[C], tup0[C];
    [[maybe_unused]] double Ei[C];                        // PHI_DERIVED (Ei is not kept: phase D loads its pairs again, as it always has)
    unsigned smask;                                       // active set: bit i <=> T0_i < Tm
    double Tm, f;
    ColumnNoise nz;
    if constexpr (!BATCH_HEAD) {
        Tm = p.Tm;
        if (a.noise) nz.load(a, col);
        f = step_forcing(a, nz, col, hd.ft, hd.fcol, hd.tyear, hd.n);
        smask = cmask[t];
    } else {
        // (the lane's cell index is made opaque per load group: the addresses are formed here, in the wave-uniform base +
        // 32-bit offset form, and none is kept.  Not `volatile`, like StepHead's pin: after a volatile asm hipcc reads the
        // forcing schedule and N_c below with per-lane vector loads, which wait behind the state's)
        unsigned kl = k0;
        asm("" : "+v"(kl));
        // (ZERO_LINES: a flagged pair is not loaded, it holds +0.0 — the same concentration and water_temperature of the
        // same bits)
        if constexpr (ZERO_LINES) load_state_unless_zero<C, TT>(st + S_Ew * a.fstride, kl, Ew, zold >> S_Ew);
        else load_state<C, TT>(st + S_Ew * a.fstride, kl, Ew);
        if constexpr (PHI_DERIVED) {
            if constexpr (ZERO_LINES) {
                load_state_unless_zero<C, TT>(st + S_Ei * a.fstride, kl, Ei, zold >> S_Ei);
                load_state_unless_zero<C, TT>(st + S_h * a.fstride, kl, hk, zold >> S_h);
            } else {
                load_state<C, TT>(st + S_Ei * a.fstride, kl, Ei);
                load_state<C, TT>(st + S_h * a.fstride, kl, hk);
            }
        } else {
            load_state<C, TT>(st + S_phi * a.fstride, kl, ph);
            load_state<C, TT>(st + S_h * a.fstride, kl, hk);
        }
        smask = cmask[t];
        __builtin_amdgcn_sched_barrier(0);
        asm("" : "+v"(kl));
        load_chunk<C>(geom + G_LO * a.gstride, kl, tlo0);
        load_chunk<C>(geom + G_UP * a.gstride, kl, tup0);
        load_chunk<C>(gX, kl, xk0);
        __builtin_amdgcn_sched_barrier(0);
        // under the loads: the parameter block's Tm, the noise record (before the workgroup's first barrier) and the forcing
        Tm = p.Tm;
        if (a.noise) nz.load(a, col);
        f = step_forcing(a, nz, col, hd.ft, hd.fcol, hd.tyear, hd.n);
        __builtin_amdgcn_sched_barrier(0);
    }
    int it = 0;
    bool again;
    // TBAR_VOTE: Ti, Tbar and Tbar's halo are formed inside the loop, under the vote (below); phase D finds them here
    [[maybe_unused]] double Ti[C];
    double tb[C], tbl, tbr;
    do {
        double tlo[C], tup[C], dd[C];
        [[maybe_unused]] double g[C], gl, gr;             // MERGE_RG / TBAR_VOTE: the masked concentration and its halo
        // (!BATCH_HEAD: the lane's cell index is made opaque inside the loop: hoisted out of it, the six addresses
        // would live as per-lane 64-bit pointers instead of the wave-uniform base + 32-bit offset form)
        unsigned kl = k0;
        if constexpr (!BATCH_HEAD) {
            asm volatile("" : "+v"(kl));
            load_chunk<C>(geom + G_LO * a.gstride, kl, tlo);
            load_chunk<C>(geom + G_UP * a.gstride, kl, tup);
        }
        if (it == 0) {
            double r[C];
            if constexpr (BATCH_HEAD) {
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    tlo[i] = tlo0[i];
                    tup[i] = tup0[i];
                }
            } else {
                load_state<C, TT>(st + S_Ew * a.fstride, kl, Ew);
                load_state<C, TT>(st + S_phi * a.fstride, kl, ph);
                load_state<C, TT>(st + S_h * a.fstride, kl, hk);
                load_chunk<C>(gX, kl, xk0);
            }
            if constexpr (PHI_DERIVED) {
#pragma unroll
                for (int i = 0; i < C; ++i) ph[i] = concentration(p, Ei[i], hk[i]);
            }
            // Padding cells (k >= nlat) need no special case in phases A and B: their state and table
            // entries are zero, so their rows are decoupled (lo = up = 0, g = phi = 0) and finite.
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const double tw = water_temperature(p, Ew[i], ph[i]);
                sEw[i * T] = Ew[i];
                sh[i * T] = hk[i];
                sTw[i * T] = tw;
                dd[i] = t0_diag_excess(p, hk[i]);
                r[i] = (1.0 - ph[i]) * (tw - Tm);
            }
            EBM_STAMP(1);
            EBM_STAMPW(1);                                    // per wave: inputs arrived
            double rl, rr;
            if constexpr (MERGE_RG) {
                // r and g are both functions of the loaded state and the mask word alone: one exchange, one barrier, carries
                // the four words (r's two and g's first in P0, g's last in P1[0, T): P1 is free until the solve)
                masked_concentration(ph, smask, g);
                halo_exchange_two(P0, P1, t, T, r[0], r[C - 1], g[0], g[C - 1], rl, rr, gl, gr);
            } else {
                halo_exchange(P0, P0 + T, t, T, r[0], r[C - 1], rl, rr);
            }
            EBM_STAMP(2);
            // (this loop stays in the kernels — the same two lines in all three: moved into a helper, it changes how hipcc
            // peels the first Newton iteration of this kernel and of miz_resident_kernel, and with it their whole code)
#pragma unroll
            for (int i = 0; i < C; ++i)
                rd[i] = t0_rhs(p, insolation(p, xk0[i], ct), tlo[i], tup[i], left_of(r, i, rl), r[i], right_of(r, i, rr), f);
            // r halo reads done before P0 is reused (!MERGE_RG: by newton_iteration's g exchange).  MERGE_RG: the barrier now
            // stands between the neighbour's read of g's last value in P1[t] and THIS thread's chunk summary W1[t] = P1[t],
            // the solve's very first write.  (P0's three words would do without it: the solve writes P0 only after its own
            // first barrier.)  It may stand anywhere between halo_exchange_two's reads and the solve; removed, the host play
            // reports the race (tests/test_host_step_lds.py).
            __syncthreads();
        } else {
            // second and later iterations (a changed active set): the right-hand side does not depend on the set and
            // is still in registers, like phi; only the rows' ingredients are fetched / formed again — the same values
            if constexpr (BATCH_HEAD) {
                asm volatile("" : "+v"(kl));
                load_chunk<C>(geom + G_LO * a.gstride, kl, tlo);
                load_chunk<C>(geom + G_UP * a.gstride, kl, tup);
            }
#pragma unroll
            for (int i = 0; i < C; ++i) dd[i] = t0_diag_excess(p, sh[i * T]);
        }
        EBM_STAMP(3);
        // ---------------- phase B: active-set Newton, src/miz.jl:33-68 --------------------
        ++it;
        if constexpr (MERGE_RG || TBAR_VOTE) {
            // Barrier by barrier, first pass: (1) halo_exchange_two's: r's and g's words are written.  (2) the one above: the
            // neighbours have read them; W1 may take P1.  (3 ..) the solve's.  (last) the vote, which is also the Tbar
            // exchange's barrier.  A second or later pass — the set changed — starts with today's g exchange through
            // P0[0, 2T): free, the interface solution Y was last read before the vote's barrier.
            if (!MERGE_RG || it > 1) {
                masked_concentration(ph, smask, g);
                halo_exchange(P0, P0 + T, t, T, g[0], g[C - 1], gl, gr);
            }
            const int changed = newton_solve_given_halo<C, TT>(tlo, tup, dd, g, gl, gr, rd, xs, smask, t, T, k0, nlat, P0, P1);
            if constexpr (TBAR_VOTE) {
                // The Tbar halo does not depend on the vote's outcome: after back-substitution the lane has all that Tbar
                // needs, so it publishes its first and last Tbar in P1[0, 2T) — free once the solve's last barrier is passed;
                // P0 is not, Y may still be read there — BEFORE the vote, whose barrier then serves the exchange.  The
                // expressions are phase D's, in its order.  If the vote says "again", the words are dropped: the next pass
                // forms them anew from its own solution.  Its g exchange writes P0 only, and its W1 write to P1 comes after
                // that exchange's barrier, hence after every thread's read of the dropped words (which stands before the
                // thread's write to P0, in program order).
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const double T0i = xs[i] + Tm;                            // new warm start, :64
                    const double ti = jl_min(T0i, Tm);                        // ice_temp, :31,65
                    Ti[i] = (sh[i * T] == 0.0) ? 0.0 : ti;                    // Ti: zeroref!, :66
                    tb[i] = Ti[i] * ph[i] + (1.0 - ph[i]) * sTw[i * T];       // Tbar, :21-26
                }
                again = publish_then_vote(P1, t, T, tb[0], tb[C - 1], changed, tbl, tbr);
            } else {
                again = __syncthreads_or(changed) != 0;
            }
        } else {
            again = newton_iteration<C, TT>(tlo, tup, dd, ph, rd, xs, smask, t, T, k0, nlat, P0, P1);
        }
    } while (again && it < kMaxNewton);
    count_newton(a, col, t, it, again ? 1 : 0);
    {
        // (the lane index is made opaque so that the mask word's per-lane 64-bit address is formed here
        // again instead of being kept — and spilled — across the solve)
        unsigned tl = (unsigned)t;
        asm volatile("" : "+v"(tl));
        cmask[tl] = (unsigned short)smask;                // new warm start, src/miz.jl:64
    }
    EBM_STAMP(6);
    EBM_STAMPW(2);                                        // per wave: phase D starts

    // ---------------- phase D: fluxes and state update ---------------------------------------
    double xk[C];
    load_chunk<C>(gX, k0, xk);
    const double xl = gX[k0 > 0 ? k0 - 1 : 0], xr = gX[k0 + C];     // zero-padded table; unused at the ends
    double g0[GRID == 0 ? C : 1], g1[GRID == 0 ? C : 1], g2[GRID == 0 ? C : 1];
    // (GRID == 0: sub-, main and super-diagonal of par.D*get_diffop — on the identity grid the physics stencil and the
    // solver's plain coefficients are the same three tables (build_tables) — are loaded pair by pair with Ei and D below:
    // all four cells' worth at once do not fit the cell updates' register budget at every workgroup size)
    {
        double T0[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            T0[i] = xs[i] + Tm;                                       // new warm start, :64
            if constexpr (TBAR_VOTE) {
                xs[i] = Ti[i];                                        // formed under the last pass's vote, like tb
            } else {
                const double ti = jl_min(T0[i], Tm);                  // ice_temp, :31,65
                xs[i] = (sh[i * T] == 0.0) ? 0.0 : ti;                // Ti: zeroref!, :66
                tb[i] = xs[i] * ph[i] + (1.0 - ph[i]) * sTw[i * T];   // Tbar, :21-26
            }
        }
        if (MAYDIAG && diag) store_chunk<C>(st + S_T0 * a.fstride, T0, k0, nlat);
    }
    // (TBAR_VOTE: the halo came with the vote)
    if constexpr (!TBAR_VOTE) halo_exchange(P0, P0 + T, t, T, tb[0], tb[C - 1], tbl, tbr);
    EBM_STAMP(7);
    EBM_STAMPW(3);                                        // per wave: Tbar halo done
    // Whole-line stores.  A lane owns 8*C contiguous bytes of every field in the natural layout; written pair by
    // pair, each 128-B line would reach L2 in two halves ~10^4 cycles apart and be written back to HBM twice.  The
    // prognostic fields of this kernel are therefore in the pair-split layout (state_index), in which every store
    // instruction of a wave covers whole lines: each pair's new prognostics leave as soon as the pair is computed.
    TbarStencil<C, GRID> stencil;
    stencil.start(k0, nlat, xl, xk, tbl, tb);
    double difx[IMEX ? C : 1];                            // IMEX: the corrected diffusion term of every cell
    if constexpr (IMEX) {
        double sol[C];
        {
            // rows of I - (dt/cw)*Dif and the right-hand side, the explicit increments
            double ra[C], rb[C], rc[C], dE[C], dif[C], tlo[C], tup[C];
            load_chunk<C>(geom + G_LO * a.gstride, k0, tlo);
            load_chunk<C>(geom + G_UP * a.gstride, k0, tup);
            imex_increments<C, GRID>(a, p, geom, k0, nlat, ct, f, xk, xl, xr, tb, tbl, tbr, ph, dif, dE);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                // the explicit diffusion term waits in the Tw words of the stash (Tw is formed again below from the stashed
                // Ew and phi — one division — instead of the whole stencil a second time)
                sTw[i * T] = dif[i];
                imex_row(p, tlo[i], tup[i], ra[i], rb[i], rc[i]);
            }
            partition_solve<C, TT>(ra, rb, rc, dE, sol, t, T, P0, P1);
        }
        __syncthreads();                                  // the solve's LDS reads are done before P0 is reused
        {
            // Only Ti (xs) and the solution crossed the solve in registers: phi and x are fetched again (the lane's cell
            // index made opaque, so that the reloads are real), Tw and Tbar are formed again, the parked diffusion term comes
            // back from the stash, and the explicit increment is evaluated a second time from it — same operands, same
            // operations, same bits — for the correction (dE_new - dE)/dt.
            unsigned kl = k0;
            asm volatile("" : "+v"(kl));
            load_state<C, TT>(st + S_phi * a.fstride, kl, ph);
            load_chunk<C>(gX, kl, xk);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const double dif0 = sTw[i * T];
                const double tw = water_temperature(p, sEw[i * T], ph[i]);
                sTw[i * T] = tw;                                      // the stash holds Tw again for the cell updates
                tb[i] = xs[i] * ph[i] + (1.0 - ph[i]) * tw;
                const double dE = enthalpy_increment(p, (int)k0 + i, nlat, xk[i], ct, tb[i], dif0, f, ph[i]);
                difx[IMEX ? i : 0] = dif0 + div_with_rcp(sol[i] - dE, p.dt, p.rcp_dt);
            }
        }
    }
    // after the step's last barrier (every wave has used the old N_c), and before the cell updates: their register budget
    // has no room for a value that only waits for the kernel's last line
    if (a.noise) nz.store(a, col);
    // Ei and D of pair j, where pair j of the lane whose first cell is kq lies (ZERO_LINES: a flagged pair is not loaded)
    auto load_pair_inputs = [&](int j, unsigned kq, double2 &Ei2, double2 &Dk2) {
        const unsigned ks = state_index<C, TT>(kq, j);
        if constexpr (ZERO_LINES) {
            Ei2 = load_pair_unless_zero(st + S_Ei * a.fstride + ks, zold & zero_flag_bit(j, S_Ei));
            Dk2 = load_pair_unless_zero(st + S_D * a.fstride + ks, zold & zero_flag_bit(j, S_D));
        } else {
            Ei2 = *reinterpret_cast<const double2 *>(st + S_Ei * a.fstride + ks);
            Dk2 = *reinterpret_cast<const double2 *>(st + S_D * a.fstride + ks);
        }
    };
    // EARLY: both pairs' Ei and D are requested here, before the first pair's arithmetic and so before any store of this wave.
    // gfx950 counts loads and stores in one vmcnt, retired in issue order: requested after the first pair's stores, as the
    // other kernels do, the second pair's inputs come back only once those stores are acknowledged.  Four more VGPRs per
    // field wait through the first pair's cell updates; the state-only and diagnostic four-cell kernels of the reference's
    // step have room for them (no scratch, <= 128 VGPRs).  OUT_SAVE keeps the pair-by-pair order (its sums need the
    // registers: with both pairs requested here it spills at 960 threads), like IMEX (whose second solve stands
    // between) and the two-cell kernels (one pair).  The identity grid's tables stay pair by pair.
    constexpr bool EARLY = C == 4 && !IMEX && OUT != OUT_SAVE;
    double2 Ei2a[C / 2], Dk2a[C / 2];
    if constexpr (EARLY) {
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < C / 2; ++j) load_pair_inputs(j, k0, Ei2a[j], Dk2a[j]);
    }
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        MizCellOut o[2];
        __builtin_amdgcn_sched_barrier(0);
        const unsigned ks = state_index<C, TT>(k0, j);    // the pair's place in every field this kernel stores
        if constexpr (!EARLY) load_pair_inputs(j, k0, Ei2a[j], Dk2a[j]);
        const double2 Ei2 = Ei2a[j], Dk2 = Dk2a[j];
        if (C == 4 && j == 1) {
            EBM_ARRIVED2(Ei2, Dk2);
            EBM_STAMPW(7);                                // per wave: the second pair's Ei and D have arrived
        }
        if constexpr (GRID == 0 && !IMEX) {
            const double2 lo = *reinterpret_cast<const double2 *>(geom + G_LO * a.gstride + (k0 + 2 * j));
            const double2 di = *reinterpret_cast<const double2 *>(geom + G_DI * a.gstride + (k0 + 2 * j));
            const double2 up = *reinterpret_cast<const double2 *>(geom + G_UP * a.gstride + (k0 + 2 * j));
            g0[GRID == 0 ? 2 * j : 0] = lo.x;  g0[GRID == 0 ? 2 * j + 1 : 0] = lo.y;
            g1[GRID == 0 ? 2 * j : 0] = di.x;  g1[GRID == 0 ? 2 * j + 1 : 0] = di.y;
            g2[GRID == 0 ? 2 * j : 0] = up.x;  g2[GRID == 0 ? 2 * j + 1 : 0] = up.y;
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            __builtin_amdgcn_sched_barrier(0);
            const int i = 2 * j + q;
            const double S = insolation(p, xk[i], ct);
            double dif;
            if constexpr (IMEX) {
                dif = difx[IMEX ? i : 0];
            } else {
                dif = stencil.dif(p, i, k0, nlat, xk, xr, tb, tbl, tbr, g0[GRID == 0 ? i : 0], g1[GRID == 0 ? i : 0],
                                  g2[GRID == 0 ? i : 0]);
            }
            o[q] = miz_cell_update(p, f, S, xk[i], dif, tb[i], q ? Ei2.y : Ei2.x, sEw[i * T], sh[i * T],
                                   q ? Dk2.y : Dk2.x, ph[i], sTw[i * T], xs[i]);
            if (C == 4 && i == C - 2) {
                // L2 prefetch for the workgroup that follows this one on the XCD (column + a.prefetch):
                // one 4-byte LDS-DMA load per 32-B sector of its phase-A inputs, issued once this
                // thread's own loads have all been consumed and hidden under the last cell's
                // arithmetic.  The data lands in stash words of cell C-2 that this wave has just
                // finished with and is never read.
                // (hipcc waits vmcnt(0) at the first use of any earlier load's result while an LDS-DMA is
                // in flight: retire the one load not consumed yet before issuing it)
                if constexpr (PHI_DERIVED)      // (the new phi is not formed at all)
                    asm volatile("" ::"v"(xr), "v"(o[q].q[Q_Ei]), "v"(o[q].q[Q_Ew]), "v"(o[q].q[Q_h]), "v"(o[q].q[Q_D]));
                else
                    asm volatile("" ::"v"(xr), "v"(o[q].q[Q_Ei]), "v"(o[q].q[Q_Ew]), "v"(o[q].q[Q_h]), "v"(o[q].q[Q_D]),
                                 "v"(o[q].q[Q_phi]));
                __builtin_amdgcn_sched_barrier(0);
                if (a.prefetch > 0 && col + a.prefetch < a.ncol) {
                    const double *nxt = a.state + (size_t)(col + a.prefetch) * (size_t)a.pitch +
                                        ((unsigned)(t >> 6) * 256u + (unsigned)(t & 63) * 4u);
                    auto *sink = (__attribute__((address_space(3))) void *)(smem + 6 * T + (C - 2) * T + (t & ~63));
                    // ZERO_LINES: lanes 0 .. 31 fetch the sectors of one KiB of the successor's field, lanes 32 .. 63 those of
                    // the next; a lane skips a field whose KiB the successor will not load
                    // (measured against prefetching them all the same: 1.45 % of the step, profiles/EXPERIMENTS.md)
                    unsigned skip = 0;
                    if constexpr (ZERO_LINES) skip = (t & 32) ? znext1 : znext0;
                    if (!(skip & (1u << S_Ew)))
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(nxt + S_Ew * a.fstride), sink, 4, 0, 0);
                    if (!(skip & (1u << (PHI_DERIVED ? S_Ei : S_phi))))
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(nxt + (PHI_DERIVED ? S_Ei : S_phi) * a.fstride), sink, 4, 0, 0);
                    if (!(skip & (1u << S_h)))
                        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(nxt + S_h * a.fstride), sink, 4, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned kp = k0 + 2 * j;
        const bool v0 = (int)kp < nlat, v1 = (int)kp + 1 < nlat;
        // (PHI_DERIVED: the phi field is not stored.  ZERO_LINES: neither is a pair of which all 64 lanes hold zero bits —
        // the integer pattern, not == 0.0: -0.0 is not what a skipped load returns — where the flag says memory holds
        // them already; the new flag is the ballot's result either way)
#define EBM_PUT(slot_, qi)                                                                         \
        if constexpr (!PHI_DERIVED || (slot_) != S_phi) {                                          \
            double2 d_;                                                                            \
            d_.x = v0 ? o[0].q[qi] : 0.0;                                                          \
            d_.y = v1 ? o[1].q[qi] : 0.0;                                                          \
            if constexpr (ZERO_LINES && (slot_) <= S_D) {                                          \
                const bool zero_ = wave_holds_zero_bits(d_);                                       \
                if (zero_) znew |= zero_flag_bit(j, (slot_));                                      \
                if (!(zero_ && (zold & zero_flag_bit(j, (slot_)))))                                \
                    EBM_STORE2(st + (slot_) * a.fstride + ks, d_);                                 \
            } else {                                                                               \
                EBM_STORE2(st + (slot_) * a.fstride + ks, d_);                                     \
            }                                                                                      \
        }
        if (j == C / 2 - 1) EBM_STAMPW(5);                // per wave: arithmetic done, before the last stores
        EBM_PUT(S_Ei, Q_Ei) EBM_PUT(S_Ew, Q_Ew) EBM_PUT(S_h, Q_h) EBM_PUT(S_D, Q_D) EBM_PUT(S_phi, Q_phi)
        if (MAYDIAG && diag) {
            // The diagnostic fields are outputs only and share the layout of the prognostic ones (stored in the natural
            // layout they cost 0.36 ms for a diagnostic step of the 4096 x 2048 shape against 0.164 state-only).  The runtime
            // un-permutes in place before the first read (permute_fields_kernel; ebm_ctx::diag_split).
            EBM_PUT(S_n, Q_n) EBM_PUT(S_E, Q_E) EBM_PUT(S_T, Q_T) EBM_PUT(S_Ti, Q_Ti) EBM_PUT(S_Tw, Q_Tw)
        }
#undef EBM_PUT
        if constexpr (OUT == OUT_SAVE)
            save_pair<Q_MIZ_COUNT>(a, (size_t)col * (size_t)a.pitch, ks, kp, o[0], o[1], v0, v1);
        if (j < 2) EBM_STAMP(8 + j);
        if (j == 0) EBM_STAMPW(4);                        // per wave: first pair done
    }
    // the LDS-DMA prefetch must have landed before this wave can end (its LDS is released with the workgroup); it was
    // issued a whole cell update ago
    if constexpr (C == 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (ZERO_LINES) store_zero_flag_word<TT>(a, col, t, znew);
    EBM_STAMP(15);
    EBM_STAMPW(6);                                        // per wave: stores issued
}

}  // namespace ebm
