// Plain types and constants shared by the kernels and the host runtime: the parameter block, the slot / quantity / output-mode /
// table enums and the k... limits.  No HIP include: ebm_tables.h (host table math) builds with a plain C++ compiler.
// Included through ebm_internal.h by everything else.
#pragma once

namespace ebm {

// Parameter block, resident in device memory and read through scalar loads.  The first 25
// entries mirror default_parval (reference src/infrastructure.jl:407-433); the derived
// constants are evaluated once on the host in the reference's operation order so that every
// cell sees the same rounded value.
struct Params {
    double D, A, B, cw, S0, S1, S2, a0, a2, ai, Fb, k, Lf, F, cg, tau, Tm, m1, m2, alpha, rl,
        Dmin, Dmax, hmin, kappa;
    double dt;          // st.dt
    // MIZ
    double Tm_pow_m2;   // Tm^m2                                   src/miz.jl:71
    double c_latmelt;   // -pi/2.0*alpha                           src/miz.jl:141
    double c_dn;        // Lf*alpha*Dmin^2*hmin                    src/miz.jl:127
    double c_weld;      // kappa*alpha/4                           src/miz.jl:143
    double c_ht;        // -1/Lf                                   src/miz.jl:139
    double two_rl;      // 2.0*rl                                  src/miz.jl:91
    // classic (get_statics, src/classic.jl:18-29)
    double cg_tau, dt_tau, dc, M, kLf;
    // Refined reciprocals of two constant divisors, produced ON THE DEVICE by the same routine the
    // physics' IEEE division uses (derive_params_kernel), so that dividing through them gives the
    // bits an in-kernel division gives: 1/dt (src/miz.jl:173) and 1/c_dn (src/miz.jl:127).
    double rcp_dt, rcp_cdn;
    double theta_imex;  // dt/cw: the implicit-diffusion extension's matrix is I - theta*Dif (EBM_MODEL_MIZ_IMEX)
};

// Device state: one slab, field slot s at state + s*fstride, each [ncol][pitch] with
// pitch = threads*cells >= nlat (latitude contiguous, padding cells kept at zero).
enum MizSlot { S_Ei = 0, S_Ew, S_h, S_D, S_phi, S_T0, S_Tw, S_Ti, S_n, S_E, S_T, S_MIZ_COUNT };
enum ClassicSlot { C_E = 0, C_Tg, C_T, C_h, C_COUNT };

// The quantities a step produces per cell, in the order the kernels hold them in registers
// (savesol! fusion: StepArgs::var_of maps each one to a saved-variable index or -1).
enum MizQuantity { Q_Ei = 0, Q_Ew, Q_h, Q_D, Q_phi, Q_n, Q_E, Q_T, Q_Ti, Q_Tw, Q_MIZ_COUNT };
enum ClassicQuantity { QC_E = 0, QC_Tg, QC_T, QC_h, QC_COUNT };
constexpr int kMaxQuantities = 12;

// What a step launch writes besides the prognostic state.
enum OutMode {
    OUT_STATE = 0,   // prognostics (+ warm-start mask) only
    OUT_DIAG = 1,    // + T0 and the diagnostic fields
    OUT_SAVE = 2,    // savesol! fused into the step: annual-mean running sums and/or a raw snapshot
                     // from registers; the diagnostic fields only if write_diag
    OUT_LOOP = 3,    // nfused steps in one launch, the whole state on the chip between them (miz_fused_kernel: in registers,
                     // meridians of up to 2048 cells; miz_resident_kernel: in LDS, longer ones and the extension; classic:
                     // registers, any); the diagnostic fields after the last step if write_diag
    OUT_LOOP_SAVE = 4,   // OUT_LOOP with savesol!'s running sums taken from every step (miz_resident_kernel<SAVE>; four cells
                         // per thread; ebm_integrate's stretches without snapshots)
};

// Per-latitude constant tables: one slab, table i at geom + i*gstride (gstride = pitch); one slab per parameter set,
// set_stride apart (G_X is the same in every set).
//   G_X              st.x
//   G_0..G_4         physics stencil, bit-exact restatement of the reference:
//                      identity grid: sub, diag, sup of par.D*get_diffop  (infrastructure.jl:480-497)
//                      other grids:   mxxph, mxxmh, diffx[i], diffx[i-1], phmmh  (:509-518)
//   G_LO, G_DI, G_UP the same operator as plain tridiagonal coefficients (T0 / Tg solves only)
//   G_KSUB..G_SB     classic: kappa's three diagonals, aw, S base (src/classic.jl:21-28)
enum GeomTable { G_X = 0, G_0, G_1, G_2, G_3, G_4, G_LO, G_DI, G_UP, G_KSUB, G_KDIAG, G_KSUP, G_AW, G_SB, G_COUNT };

constexpr int kCounterShards = 64;
constexpr int kNoiseMaxFused = 64; // with forcing noise, fused launches take at most one wave's lanes of steps (ColumnNoise)
constexpr int kSchedWords = 9;     // base, peak, cool, rate up, rate down, domain[1..4]
constexpr int kMaxNewton = 1000;   // the cap of the T0 iteration: NonlinearSolve's default maxiters (src/miz.jl:55-60 passes none)

constexpr int kMaxLat = 4096;      // one workgroup of <= 1024 threads x 4 cells owns a whole meridian
constexpr int kFusedRegThreads = 512;   // up to here the fused-K kernel keeps the whole state in registers (4 cells per thread)
constexpr int kFusedRegThreads2 = 768;  // ... with 2 cells per thread (168 VGPRs: three waves per SIMD)
constexpr int kMaxLat2 = 1536;          // longest meridian stepped with 2 cells per thread

}  // namespace ebm
