// HIP kernels (gfx950 / CDNA4, wave64) for the energy-balance time-stepping hot path.
//
// One workgroup of T threads integrates one meridian (column) for one step; thread t owns the
// C contiguous cells t*C .. t*C+C-1 ("chunk ownership") for the whole step.  A lane reads its
// 8*C contiguous bytes with 16-byte loads, so a wave covers 64*8*C contiguous bytes of the
// latitude axis per field.  Everything the reference does in ~60 temporary vectors per step
// (src/miz.jl:150-196) is fused into one kernel:
//
//   phase A  loads; water temperature; right-hand side of the T0 system (3-point stencil: the
//            chunk interior comes from registers, the two halo cells from the neighbouring
//            lanes through LDS, zero-flux at equator and pole)
//   phase B  T0 solve: active-set Newton on the piecewise-linear system of src/miz.jl:33-45.
//            Each linear system is tridiagonal and is solved per meridian by a chunk
//            partition (each thread Thomas-eliminates its C rows in registers) followed by
//            parallel cyclic reduction of the T-row interface system in LDS
//   phase D  Tbar stencil, radiative + lateral fluxes, enthalpy Euler step, redistribution,
//            floe size / thickness / concentration update, 16-byte stores
//
// Kernels of the library, and where each is defined and instantiated:
//   miz_step_kernel<C, GRID, OUT, T, IMEX, PHI_DERIVED, ZERO_LINES>   one step per launch; OUT: state only / + diagnostics / savesol! from
//                                       registers (annual-mean sums, raw snapshots); IMEX: the implicit-diffusion
//                                       extension (one more tridiagonal solve per step, see include/ebm_hip.h)
//                                       [ebm_miz_step.h; miz_step_identity.hip, miz_step_nonuniform.hip, miz_step_imex.hip]
//   miz_fused_kernel<C, GRID, T, SAVE>  K steps per launch, the whole state in registers (<= 512 threads; 768 with C = 2); SAVE (C = 2):
//                                       with savesol!'s sums                     [ebm_miz_fused.h; this file, SAVE: miz_resident_save.hip]
//   miz_resident_kernel<GRID, T, IMEX, SAVE>  K steps per launch, the state resident in LDS (more than 512 threads; the extension;
//                                       launches of many columns at any size; SAVE: with savesol!'s sums, for ebm_integrate)
//                                       [ebm_miz_resident.h; miz_resident.hip, SAVE: miz_resident_save.hip]
//   classic_step_kernel<C, MODE>        WE15 model: single step / savesol! / K steps per launch            [this file]
//   diffusion_kernel<GRID>              the diffusion operator on its own (ebm_diffusion)                  [this file]
//   finish_mean, hemispheric_means, mask_from_t0, derive_params, divide, permute_fields (split / unsplit), restore_phi,
//   noise_innovations, noise_sequence, equilibrium_check, passage_check, compact_active: small helpers     [this file]
//   column_scalars, passage_scalar: band integrals / means and edge positions per column (column_scalar)   [this file]
//   zonal_sweep, zonal_seg_forward / _backward, zonal_reduced_solve: the zonal diffusion substep           [ebm_zonal.hip]
// and every host-side launcher of the MIZ, classic and helper kernels [this file].  Which step kernel a launch takes, with
// how much LDS and which noise source, is decided in ebm_plan.h (plan_step: plain C++, no HIP); this file only executes a
// plan: kernel_of looks its instantiation up, launch_step_columns launches it, prepare_kernels readies every plan of a geometry.
// The layers below the kernels: ebm_device.h (stores, parameter block, IEEE division, chunk loads), ebm_noise.h, ebm_solve.h
// (halo exchanges, the tridiagonal solve), ebm_miz_pieces.h (the pieces of the MIZ step), ebm_kernel_table.h (sizes and lookup).
// C = cells per thread (4; 2 for a few short meridians), GRID = 0 identity / 1 any other grid, T =
// workgroup size as a compile-time constant (the lists of sizes and the lookup are in ebm_kernel_table.h).  Every one of
// the 523 kernels uses 0 bytes of scratch (tests/tools/resource_usage.py).
// The three MIZ step kernels are bit-identical by contract: every piece of the step that they do not do differently
// (pointwise physics, Tbar stencil, implicit-diffusion increments and rows, neighbour selection) has one definition, in
// ebm_miz_pieces.h; what stays in each kernel is how it holds its state and loads its tables.
//
// Arithmetic policy.  Everything outside the tridiagonal solves is a bit-exact restatement of
// the reference's expressions (IEEE division, no FMA contraction: build with
// -ffp-contract=off; the order of operations is the reference's).  The solves are free to use
// any arithmetic (explicit FMAs, v_rcp_f64 + Newton): their result is defined by the linear
// system, not by an operation order.
//
// No MFMA: there is no dense contraction on this path; it is HBM-/fp64-VALU-bound.
#include <set>

#include "ebm_kernel_table.h"

namespace ebm {

// ---- classic (WE15) step, src/classic.jl:37-71 ------------------------------------------------
// MODE: OUT_STATE (T, h written if write_diag), OUT_SAVE (savesol! from registers) or OUT_LOOP
// (a.nfused steps per launch, E and Tg in registers between steps).
struct ClassicCellOut {
    double q[QC_COUNT];
};
template <int C, int MODE>
__global__ void __launch_bounds__(1024) classic_step_kernel(const StepArgs a) {
    static_assert(C == 2 || C == 4, "cells per thread");
    constexpr bool LOOP = MODE == OUT_LOOP;
    extern __shared__ double smem[];
    const int T = blockDim.x, t = threadIdx.x, col = step_column(a);
    const int nlat = a.nlat;
    const unsigned k0 = (unsigned)t * C;
    double *P0 = smem, *P1 = smem + 3 * T;
    const int pset = param_set(a, col);                  // ebm_set_column_params (set 0 without a table)
    ConstParams &p = *reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p + pset));
    const double *const geom = a.geom + pset * a.set_stride;
    double *const st = a.state + (size_t)col * (size_t)a.pitch;          // wave-uniform
    ColumnNoise nz;                                                    // LOOP: N_c in memory (noise_sequence_kernel)
    if (!LOOP && a.noise) nz.load(a, col);                             // before the state is loaded, and any barrier
    double E[C], Tg[C];
    load_chunk<C>(st + C_E * a.fstride, k0, E);
    load_chunk<C>(st + C_Tg * a.fstride, k0, Tg);
    const int nloop = LOOP ? a.nfused : 1;
    for (int step = 0; step < nloop; ++step) {
        // per-latitude statics (get_statics, src/classic.jl:18-29): re-read every step (L2 hits) rather
        // than kept in 48 registers across the fused loop
        const double *ge = geom;
        if constexpr (LOOP) asm volatile("" : "+s"(ge));
        double xk[C], aw[C], Sb[C], kd[C], ca[C], cc[C];
        load_chunk<C>(ge + G_X * a.gstride, k0, xk);
        load_chunk<C>(ge + G_AW * a.gstride, k0, aw);
        load_chunk<C>(ge + G_SB * a.gstride, k0, Sb);
        load_chunk<C>(ge + G_KDIAG * a.gstride, k0, kd);
        load_chunk<C>(ge + G_KSUB * a.gstride, k0, ca);   // off-diagonals of kappa
        load_chunk<C>(ge + G_KSUP * a.gstride, k0, cc);
        const int slot = a.slot + step;
        const double ct = a.sched ? a.sched[slot].ct : a.ct;
        const double ct_next = a.sched ? a.sched[slot].ct_next : a.ct_next;
        const double ft = a.sched ? a.sched[slot].ft : a.ft;
        double f = column_forcing(a, col, ft, a.sched ? a.sched[slot].tyear : a.tyear);
        if (a.noise) {
            if constexpr (LOOP) f = f + nz.at_step<true>(a, col, step, a.sched[slot].n);
            else f = f + nz.advance(noise_innovation(a.seed, nz.stream, a.sched ? a.sched[slot].n : a.step));
        }
        double b[C], d[C], oT[C], oh[C], xs[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const bool valid = (int)k0 + i < nlat;
            double Ek = E[i];
            const double S_i = Sb[i] - (p.S1 * ct) * xk[i];                            // :23-24
            const double S_ip1 = Sb[i] - (p.S1 * ct_next) * xk[i];
            const double alpha = bool_mul(aw[i], Ek > 0.0) + bool_mul(p.ai, Ek < 0.0); // :47
            const double Cc = alpha * S_i + p.cg_tau * Tg[i] - p.A + f;                // :48
            const double T0 = ieee_div(Cc, p.M - ieee_div(p.kLf, Ek));                 // :50
            const double Tk = bool_mul(ieee_div(Ek, p.cw), Ek >= 0.0) + bool_mul(bool_mul(T0, Ek < 0.0), T0 < 0.0);
            Ek = Ek + p.dt * (Cc - p.M * Tk + p.Fb);                                   // :53
            const double den = p.M - ieee_div(p.kLf, Ek);
            const double q = bool_mul(bool_mul(ieee_div(p.dc, den), T0 < 0.0), Ek < 0.0);       // :56
            const double rhs = Tg[i] + p.dt_tau * (bool_mul(ieee_div(Ek, p.cw), Ek >= 0.0) +
                               bool_mul(bool_mul(ieee_div(p.ai * S_ip1 - p.A + f, den), T0 < 0.0), Ek < 0.0));
            b[i] = valid ? kd[i] - q : 1.0;
            d[i] = valid ? rhs : 0.0;
            E[i] = valid ? Ek : 0.0;                                                   // padding cells stay zero
            oT[i] = Tk;
            oh[i] = bool_mul(ieee_div(-Ek, p.Lf), Ek < 0.0);                           // :65
        }
        const bool last = step == nloop - 1;
        if (last) store_chunk<C>(st + C_E * a.fstride, E, k0, nlat);
        if (a.write_diag && last) {
            store_chunk<C>(st + C_T * a.fstride, oT, k0, nlat);
            store_chunk<C>(st + C_h * a.fstride, oh, k0, nlat);
        }
        partition_solve<C>(ca, b, cc, d, xs, t, T, P0, P1);   // Implicit Euler for Tg, :55-63
#pragma unroll
        for (int i = 0; i < C; ++i) Tg[i] = ((int)k0 + i < nlat) ? xs[i] : 0.0;
        if (last) store_chunk<C>(st + C_Tg * a.fstride, Tg, k0, nlat);
        if constexpr (MODE == OUT_SAVE) {
#pragma unroll
            for (int j = 0; j < C / 2; ++j) {
                ClassicCellOut c0, c1;
                c0.q[QC_E] = E[2 * j];  c0.q[QC_Tg] = Tg[2 * j];  c0.q[QC_T] = oT[2 * j];  c0.q[QC_h] = oh[2 * j];
                c1.q[QC_E] = E[2 * j + 1];  c1.q[QC_Tg] = Tg[2 * j + 1];  c1.q[QC_T] = oT[2 * j + 1];  c1.q[QC_h] = oh[2 * j + 1];
                const unsigned kp = k0 + 2 * j;
                save_pair<QC_COUNT>(a, (size_t)col * (size_t)a.pitch, (unsigned)(j * 2 * T + 2 * t), kp, c0, c1,
                                    (int)kp < nlat, (int)kp + 1 < nlat);
            }
        }
        // (no barrier between the solves of consecutive steps: after a solve's last barrier the threads only READ P0; the
        // next solve first writes each thread's own words of P1 — which nobody reads after that last barrier — and passes
        // a barrier of its own before anything is written to P0)
    }
    if (!LOOP && a.noise) nz.store(a, col);                            // after the solve's last barrier
}

// Active set of a T0 field (after ebm_set_field(T0)): bit i of amask[col][t] <=> T0 < Tm in cell t*C+i.
__global__ void mask_from_t0_kernel(const StepArgs a, int C) {
    const int T = blockDim.x, t = threadIdx.x, col = blockIdx.x;
    const double Tm = a.p[param_set(a, col)].Tm;
    const double *T0 = a.state + S_T0 * a.fstride + (size_t)col * (size_t)a.pitch + (size_t)t * C;
    unsigned m = 0;
    for (int i = 0; i < C; ++i)
        if (t * C + i < a.nlat && T0[i] < Tm) m |= 1u << i;
    a.amask[(size_t)col * T + t] = (unsigned short)m;
}

// ebm_noise_innovations: one thread per (column, step), through the step kernels' noise_innovation
__global__ void __launch_bounds__(256) noise_innovations_kernel(const NoiseRec *__restrict__ noise, unsigned long long seed,
                                                                long long first, int nsteps, long long total,
                                                                double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long c = i / nsteps, k = i - c * nsteps;
    out[i] = noise_innovation(seed, noise[c].stream, first + k);
}
// The N_c sequence of a fused launch for the kernels that read it from memory (ColumnNoise, MEM): one wave per column, lane l
// -> a.nseq[col][l] = N_c after step l of the launch; N_c advanced by the launch's a.nfused steps
__global__ void __launch_bounds__(64) noise_sequence_kernel(const StepArgs a) {
    const int col = step_column(a);
    ColumnNoise nz;
    nz.load(a, col);
    const double nl = nz.sequence(a, a.nfused);
    if ((int)threadIdx.x < a.nfused) a.nseq[(size_t)col * kNoiseMaxFused + threadIdx.x] = nl;
    nz.store(a, col);
}
hipError_t launch_noise_sequence(const StepArgs &a, int first, int count, hipStream_t s) {
    if (first < 0 || count < 1 || a.nfused < 1 || a.nfused > kNoiseMaxFused) return hipErrorInvalidValue;
    StepArgs b = a;
    b.col0 = first;
    noise_sequence_kernel<<<dim3(count), 64, 0, s>>>(b);
    return hipGetLastError();
}
hipError_t launch_noise_innovations(const NoiseRec *noise, unsigned long long seed, long long first, int nsteps, int ncol,
                                    double *out, hipStream_t s) {
    const long long total = (long long)nsteps * ncol;
    if (total <= 0) return hipSuccess;
    noise_innovations_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, s>>>(noise, seed, first, nsteps, total, out);
    return hipGetLastError();
}

// rcp_dt / rcp_cdn of the parameter block, with the device's own refinement sequence (see Params)
__global__ void derive_params_kernel(Params *p) {
    p->rcp_dt = div_rcp(p->dt);
    p->rcp_cdn = div_rcp(p->c_dn);
}
hipError_t launch_derive_params(Params *p_dev, hipStream_t s) {
    derive_params_kernel<<<1, 1, 0, s>>>(p_dev);
    return hipGetLastError();
}

// Self-test hook (ebm_selftest_divide): q[i] = ieee_div(a[i], b[i]) with the device routine the
// physics uses, so that tests can compare it bit for bit with host IEEE division.
__global__ void divide_kernel(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ q, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) q[i] = ieee_div(a[i], b[i]);
}
hipError_t launch_divide(const double *a, const double *b, double *q, int n, hipStream_t s) {
    divide_kernel<<<(n + 255) / 256, 256, 0, s>>>(a, b, q, n);
    return hipGetLastError();
}

// hemispheric_mean (src/utilities.jl:397-403) of nvars fields of one column, by a workgroup of LANES lanes:
//   int = 0; for i in 1:nx-1: int += (vec[i]+vec[i+1]) * (x[i+1]-x[i]) / 2.0
// THE definition of the mean in this library: every kernel that needs one calls this function, so they agree to the bit.
// The latitudes are walked in tiles of kMeanTile terms: the lanes form the terms of all fields (elementwise, exact order
// of operations; coalesced row reads, x[i+1]-x[i] once per latitude) into the LDS tile terms[nvars][row]; then lane v adds row
// v onto its running sum — the reference's strictly sequential left-to-right sum from 0.0, nvars chains side by side — so
// the result is bit-identical to the reference's loop.  field_of(v): field v of the column, natural layout.  Returns, in lane
// v < nvars, the mean of field v.  With several fields an odd `row` starts the lanes' rows on different banks.
template <int LANES, class FieldOf>
__device__ __forceinline__ double hemispheric_means_of_column(FieldOf field_of, const double *__restrict__ x, int nlat, int nvars,
                                                              double *terms, int row) {
    const int lane = threadIdx.x, nterms = nlat - 1;
    double acc = 0.0;
    for (int k0 = 0; k0 < nterms; k0 += kMeanTile) {
        const int n = min(kMeanTile, nterms - k0);
        for (int i = lane; i < n; i += LANES) {
            const double dx = x[k0 + i + 1] - x[k0 + i];
            for (int v = 0; v < nvars; ++v) {
                const double *f = field_of(v);
                terms[v * row + i] = ieee_div((f[k0 + i] + f[k0 + i + 1]) * dx, 2.0);
            }
        }
        __syncthreads();
        if (lane < nvars) {
            const double *t = terms + lane * row;
#pragma unroll 8
            for (int i = 0; i < n; ++i) acc = acc + t[i];
        }
        __syncthreads();                                  // (the tile is refilled by the next round)
    }
    return acc;
}
// The mean kernel of the library (MeansArgs): one workgroup per column, every column and every field in one launch; lane v
// writes the mean of field v to out[v][col] — ebm_hemispheric_mean (one field), ebm_integrate_hemispheric, and
// ebm_run_series, whose `out` is the sample's slot of the device series.  LANES: 64 (one wave, its barriers free), or 256
// for one field of a long meridian, where the one chain waits for the term loads of a tile and four waves issue them at
// once (the launcher's rule; measured, profiles/r16_means_ab.txt).  Same bits.
template <int LANES>
__global__ void __launch_bounds__(LANES) hemispheric_means_kernel(const MeansArgs s) {
    extern __shared__ double terms[];
    const int lane = threadIdx.x, col = blockIdx.x;
    const double *const column = s.state + (size_t)col * (size_t)s.pitch;
    const double acc = hemispheric_means_of_column<LANES>([&](int v) { return column + (size_t)s.slot[v] * (size_t)s.fstride; }, s.x,
                                                   s.nlat, s.nvars, terms, s.row);
    if (lane < s.nvars) s.out[(size_t)lane * (size_t)s.var_stride + col] = acc;
}
hipError_t launch_hemispheric_means(const MeansArgs &s, int ncol, hipStream_t st) {
    if (ncol < 1 || s.nlat < 2 || s.nvars < 1 || s.nvars > kMaxQuantities) return hipErrorInvalidValue;
    MeansArgs b = s;
    b.row = (s.nlat - 1 < kMeanTile ? s.nlat - 1 : kMeanTile) | 1;
    const size_t lds = sizeof(double) * (size_t)b.nvars * (size_t)b.row;
    if (b.nvars == 1 && s.nlat - 1 > 256) hemispheric_means_kernel<256><<<ncol, 256, lds, st>>>(b);
    else hemispheric_means_kernel<64><<<ncol, 64, lds, st>>>(b);
    return hipGetLastError();
}
// ebm_equilibrate's year-end test, one workgroup per active column (EquilArgs): rows k < nlat of this year's fields
// against last year's snapshot, which takes this year's values in the same pass.  The distance is a max of exact
// |differences|, NaN-propagating, so its value does not depend on the order of the reduction (lanes, then the waves
// through LDS); d <= tol is false for NaN.
__device__ __forceinline__ double max_nan(double x, double y) { return (x != x || x > y) ? x : y; }
__global__ void __launch_bounds__(256) equilibrium_check_kernel(const EquilArgs e) {
    __shared__ double part[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int col = e.cols[blockIdx.x];
    const size_t row = (size_t)col * (size_t)e.pitch;
    bool ok = true;
    for (int v = 0; v < e.nvars; ++v) {
        const double *cur = e.state + (size_t)e.slot[v] * (size_t)e.fstride + row;
        double *prev = e.snap + (size_t)v * (size_t)e.ncol * (size_t)e.pitch + row;
        double d = 0.0;
        for (int k = t; k < e.nlat; k += 256) {
            const double c = cur[k];
            d = max_nan(d, fabs(c - prev[k]));
            prev[k] = c;
        }
        for (int off = 32; off > 0; off >>= 1) d = max_nan(d, __shfl_xor(d, off, 64));
        if (lane == 0) part[wave] = d;
        __syncthreads();
        d = max_nan(max_nan(part[0], part[1]), max_nan(part[2], part[3]));
        __syncthreads();                                  // (part is refilled by the next variable)
        if (e.compare && t == 0) e.resid[(size_t)v * (size_t)e.ncol + col] = d;
        ok = ok && d <= e.tol[v];
    }
    if (t == 0) {
        e.years[col] = e.year;
        e.frozen[col] = (e.may_freeze && ok) ? 1 : 0;
    }
}
hipError_t launch_equilibrium_check(const EquilArgs &e, int nactive, hipStream_t s) {
    if (nactive < 1 || nactive > e.ncol || e.nvars < 1 || e.nvars > kMaxQuantities) return hipErrorInvalidValue;
    equilibrium_check_kernel<<<nactive, 256, 0, s>>>(e);
    return hipGetLastError();
}

// ebm_run_until's test after a round, one wave per active column c = cols[b] (PassageArgs): the hemispheric mean of the one
// field (hemispheric_means_of_column: lane 0 holds it), then the comparison with the column's level.  A NaN mean fails both
// comparisons: it never crosses.
// (one lane: the round's verdict on column col, whose sample is acc — the mean here, a column scalar below)
__device__ __forceinline__ void passage_verdict(const PassageArgs &p, int col, double acc) {
    const double level = p.level[col];
    const bool crossed = p.direction[col] > 0 ? acc >= level : acc <= level;
    p.value[col] = acc;
    p.samples[col] = p.round;
    p.frozen[col] = crossed ? 1 : 0;
}
__global__ void __launch_bounds__(64) passage_check_kernel(const PassageArgs p) {
    __shared__ double terms[kMeanTile];
    const int lane = threadIdx.x, col = p.cols[blockIdx.x];
    const double *const f = p.field + (size_t)col * (size_t)p.pitch;
    const double acc = hemispheric_means_of_column<64>([&](int) { return f; }, p.x, p.nlat, 1, terms, kMeanTile);
    if (lane == 0) passage_verdict(p, col, acc);
}

// A COLUMN SCALAR (include/ebm_hip.h, ebm_column_scalars: the definition) of the row f of one column, by one wave; lane 0
// returns it.  kind, k0, k1 and level are the same in every lane.
//   integral kinds  hemispheric_means_of_column over the cells k0 .. k1 (shifted pointers: the one sum of the library, so the
//                   full range IS ebm_hemispheric_mean); S_MEAN divides once by x[k1] - x[k0]
//   edge kinds      the smallest K in k0 .. k1 with a hit: tiles of 256 cells, lane l loads the cells l, l + 64, l + 128, l + 192
//                   of the tile (four coalesced 512-byte requests in flight), keeps the first of its hits, and a cross-lane min
//                   gives the tile's; the walk ends at the first tile with a hit, so a row is read at most once.  Then lane 0
//                   loads f[K-1], f[K], x[K-1], x[K] and interpolates: the value depends on K and these four only
// terms: the mean's LDS tile (kMeanTile doubles); the edge kinds use no LDS.
constexpr int kNoHit = 0x7fffffff;                       // later than any cell
__device__ __forceinline__ bool scalar_hit(int kind, double v, double level) { return kind == S_EDGE_GE ? v >= level : v <= level; }
__device__ __forceinline__ int earlier_hit(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ double column_scalar(int kind, const double *__restrict__ f, const double *__restrict__ x, int k0, int k1,
                                                double level, double *terms) {
    const int lane = threadIdx.x;
    if (kind == S_INTEGRAL || kind == S_MEAN) {
        const double *const band = f + k0;
        const double acc = hemispheric_means_of_column<64>([&](int) { return band; }, x + k0, k1 - k0 + 1, 1, terms, kMeanTile);
        return kind == S_MEAN ? ieee_div(acc, x[k1] - x[k0]) : acc;
    }
    int K = kNoHit;
    for (int base = k0; base <= k1 && K == kNoHit; base += 256) {
        double v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = base + 64 * u + lane;
            v[u] = k <= k1 ? f[k] : __builtin_nan("");        // (NaN hits nothing)
        }
        int first = kNoHit;
#pragma unroll
        for (int u = 3; u >= 0; --u)
            if (scalar_hit(kind, v[u], level)) first = base + 64 * u + lane;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) first = earlier_hit(first, __shfl_xor(first, off, 64));
        K = first;
    }
    if (lane != 0) return 0.0;
    if (K == kNoHit) return __builtin_inf();             // no edge in the band
    if (K == k0) return x[k0];
    const double a = f[K - 1], b = f[K];
    if (!__builtin_isfinite(a) || !__builtin_isfinite(b)) return x[K];
    const double t = ieee_div(level - a, b - a);
    return x[K - 1] + t * (x[K] - x[K - 1]);
}
// ebm_column_scalars, ebm_run_series_scalars (ScalarArgs): one wave per (column, scalar), blockIdx = (col, s)
__global__ void __launch_bounds__(64) column_scalars_kernel(const ScalarArgs a) {
    __shared__ double terms[kMeanTile];
    const int col = blockIdx.x, s = blockIdx.y;
    const double *const f = a.row[s] + (size_t)col * (size_t)a.pitch;
    const double v = column_scalar(a.kind[s], f, a.x, a.k0[s], a.k1[s], a.level[s], terms);
    if (threadIdx.x == 0) a.out[(size_t)s * (size_t)a.out_stride + col] = v;
}
hipError_t launch_column_scalars(const ScalarArgs &a, int ncol, hipStream_t s) {
    if (ncol < 1 || a.nscal < 1 || a.nscal > kMaxQuantities) return hipErrorInvalidValue;
    for (int i = 0; i < a.nscal; ++i)
        if (a.kind[i] < 0 || a.kind[i] >= S_KINDS || a.k0[i] < 0 || a.k0[i] > a.k1[i] || a.k1[i] >= a.pitch) return hipErrorInvalidValue;
    column_scalars_kernel<<<dim3((unsigned)ncol, (unsigned)a.nscal), 64, 0, s>>>(a);
    return hipGetLastError();
}
// ebm_run_until_scalar's test after a round: passage_check_kernel with the column scalar for a sample
__global__ void __launch_bounds__(64) passage_scalar_kernel(const PassageArgs p) {
    __shared__ double terms[kMeanTile];
    const int col = p.cols[blockIdx.x];
    const double *const f = p.field + (size_t)col * (size_t)p.pitch;
    const double m = column_scalar(p.kind, f, p.x, p.k0, p.k1, p.edge_level, terms);
    if (threadIdx.x == 0) passage_verdict(p, col, m);
}
hipError_t launch_passage_check(const PassageArgs &p, int nactive, hipStream_t s) {
    if (nactive < 1 || p.nlat < 1 || p.nlat > p.pitch) return hipErrorInvalidValue;
    if (!p.scalar) {
        passage_check_kernel<<<nactive, 64, 0, s>>>(p);
        return hipGetLastError();
    }
    if (p.kind < 0 || p.kind >= S_KINDS || p.k0 < 0 || p.k0 > p.k1 || p.k1 >= p.nlat) return hipErrorInvalidValue;
    passage_scalar_kernel<<<nactive, 64, 0, s>>>(p);
    return hipGetLastError();
}

// The next active list, in one workgroup: a stable stream compaction of in[0 .. n) by !frozen[in[i]], 1024 entries per
// round — per wave a ballot and a popcount below the lane, across the 16 waves a scan of their counts in LDS.
__global__ void __launch_bounds__(1024) compact_active_kernel(const int *__restrict__ in, int n, const int *__restrict__ frozen,
                                                              int *__restrict__ out, int *__restrict__ count) {
    __shared__ int wave_base[17];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int total = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + t;
        const int c = i < n ? in[i] : 0;
        const bool keep = i < n && frozen[c] == 0;
        const unsigned long long ballot = __ballot(keep);
        const int below = __popcll(ballot & ((1ull << lane) - 1ull));
        if (lane == 0) wave_base[wave + 1] = __popcll(ballot);
        __syncthreads();
        if (t == 0) {
            wave_base[0] = 0;
            for (int w = 1; w <= 16; ++w) wave_base[w] += wave_base[w - 1];
        }
        __syncthreads();
        if (keep) out[total + wave_base[wave] + below] = c;
        total += wave_base[16];
        __syncthreads();                                  // (wave_base is refilled by the next round)
    }
    if (t == 0) *count = total;
}
hipError_t launch_compact_active(const int *in, int n, const int *frozen, int *out, int *count, hipStream_t s) {
    if (n < 1) return hipErrorInvalidValue;
    compact_active_kernel<<<1, 1024, 0, s>>>(in, n, frozen, out, count);
    return hipGetLastError();
}

// The diffusion operator on its own: out = base + D d/dx[(1-x^2) d temp/dx], one thread per cell —
// diffusion!(base, temp, st, par) / diffusion(T, st, par), src/infrastructure.jl:495-533, with the
// same device functions (and hence the same bits) the step kernels use inside their fused physics.
template <int GRID>
__global__ void diffusion_kernel(const double *__restrict__ temp, const double *__restrict__ base,
                                 double *__restrict__ out, const double *__restrict__ geom_sets, long long gstride,
                                 const Params *__restrict__ p_sets, const int *__restrict__ pset, long long set_stride,
                                 int pitch, int nlat) {
    const int col = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nlat) return;
    const int set = pset ? pset[col] : 0;
    const double *const geom = geom_sets + set * set_stride;
    const Params *const pp = p_sets + set;
    const double *T = temp + (size_t)col * pitch;
    const double tk = T[k], tm = k > 0 ? T[k - 1] : 0.0, tp = k < nlat - 1 ? T[k + 1] : 0.0;
    double term;
    if (GRID == 0) {
        term = diffusion_uniform(k, nlat, geom[G_LO * gstride + k], geom[G_DI * gstride + k], geom[G_UP * gstride + k],
                                 tm, tk, tp);
    } else {
        const double *x = geom + G_X * gstride;
        const double xk = x[k], xm = k > 0 ? x[k - 1] : 0.0, xp = k < nlat - 1 ? x[k + 1] : 0.0;
        double xxl, xxr;
        const double Fl = interface_flux(k, nlat, xm, xk, tm, tk, xxl);
        const double Fr = interface_flux(k + 1, nlat, xk, xp, tk, tp, xxr);
        term = ieee_div(pp->D * (Fr - Fl), xxr - xxl);                  // :524
    }
    out[(size_t)col * pitch + k] = (base ? base[(size_t)col * pitch + k] : 0.0) + term;
}
hipError_t launch_diffusion(const double *temp, const double *base, double *out, const double *geom, long long gstride,
                            const Params *p, const int *pset, long long set_stride, int grid_kind, int pitch, int nlat,
                            int ncol, hipStream_t s) {
    dim3 grid((nlat + 255) / 256, ncol), block(256);
    if (grid_kind == 0)
        diffusion_kernel<0><<<grid, block, 0, s>>>(temp, base, out, geom, gstride, p, pset, set_stride, pitch, nlat);
    else diffusion_kernel<1><<<grid, block, 0, s>>>(temp, base, out, geom, gstride, p, pset, set_stride, pitch, nlat);
    return hipGetLastError();
}

// annual_mean (src/infrastructure.jl:536-544, crossmean src/utilities.jl:390-395): sum / nt, from
// the pair-split layout of save_pair to the natural [col][pitch] one; the sum restarts at zero.  blockIdx.y = saved
// variable (one launch for all of them): dst / sum advance by var_stride per variable.
__global__ void finish_mean_kernel(double *__restrict__ dst, double *__restrict__ sum, double nt, int threads,
                                   int cells, long long var_stride) {
    const int t = threadIdx.x, col = blockIdx.x;
    const size_t base = (size_t)blockIdx.y * (size_t)var_stride + (size_t)col * (size_t)threads * cells;
    for (int j = 0; j < cells / 2; ++j) {
        double2 *sp = reinterpret_cast<double2 *>(sum + base + (size_t)(j * 2 * threads + 2 * t));
        const double2 s = *sp;
        double2 m;
        m.x = s.x / nt;
        m.y = s.y / nt;
        *reinterpret_cast<double2 *>(dst + base + (size_t)(t * cells + 2 * j)) = m;
        double2 z;
        z.x = 0.0;
        z.y = 0.0;
        *sp = z;
    }
}

// Natural <-> pair-split layout (split_index), in place: SPLIT = false turns fields that a 4-cells-per-thread one-step
// launch left pair-split into [col][pitch] with cell k at k; SPLIT = true is the inverse (the prognostic fields before
// such a launch; a field the caller set, about to be read by a kernel that expects the split layout).  One workgroup per
// column holds the whole column in registers across a barrier, so the permutation needs no second buffer.  blockIdx.y =
// field: `fields` advances by field_stride per field.
template <bool SPLIT>
__global__ void permute_fields_kernel(double *__restrict__ fields, long long field_stride, int threads) {
    const unsigned t = threadIdx.x, T = (unsigned)threads;
    double *f = fields + (size_t)blockIdx.y * (size_t)field_stride + (size_t)blockIdx.x * (size_t)threads * 4;
    double2 *const nat0 = reinterpret_cast<double2 *>(f + 4 * t), *const nat1 = reinterpret_cast<double2 *>(f + 4 * t + 2);
    double2 *const spl0 = reinterpret_cast<double2 *>(f + split_index(t, 0, T));
    double2 *const spl1 = reinterpret_cast<double2 *>(f + split_index(t, 1, T));
    const double2 p0 = SPLIT ? *nat0 : *spl0, p1 = SPLIT ? *nat1 : *spl1;
    __syncthreads();
    *(SPLIT ? spl0 : nat0) = p0;
    *(SPLIT ? spl1 : nat1) = p1;
}
hipError_t launch_split_fields(double *fields, long long field_stride, int nfields, int ncol, const LaunchCfg &cfg,
                               hipStream_t s) {
    if (cfg.cells != 4) return hipSuccess;               // two cells per thread: the layouts coincide
    permute_fields_kernel<true><<<dim3(ncol, nfields), cfg.threads, 0, s>>>(fields, field_stride, cfg.threads);
    return hipGetLastError();
}
hipError_t launch_unsplit_fields(double *fields, long long field_stride, int nfields, int ncol, const LaunchCfg &cfg,
                                 hipStream_t s) {
    if (cfg.cells != 4) return hipSuccess;
    permute_fields_kernel<false><<<dim3(ncol, nfields), cfg.threads, 0, s>>>(fields, field_stride, cfg.threads);
    return hipGetLastError();
}

// phi from Ei and h, for the readers of the field after one-step launches that did not store it (miz_step_kernel,
// PHI_DERIVED): one workgroup of the step's size per column, thread t owns the two pairs of its chunk in the pair-split
// layout.  UNSPLIT: the un-split pass of permute_fields_kernel over the five prognostic fields (the whole column in
// registers across a barrier, then the natural layout) with phi formed instead of read; else in place: phi's two pairs
// are written where they lie.  The column's own parameter set gives Lf, as in the step.
template <bool UNSPLIT>
__global__ void restore_phi_kernel(const StepArgs a, int threads) {
    const unsigned t = threadIdx.x, T = (unsigned)threads;
    const int col = blockIdx.x;
    ConstParams &p = *reinterpret_cast<ConstParams *>(reinterpret_cast<uintptr_t>(a.p + param_set(a, col)));
    double *const st = a.state + (size_t)col * (size_t)threads * 4;
    const unsigned s0 = split_index(t, 0, T), s1 = split_index(t, 1, T);
    double2 v[S_phi + 1][2];
#pragma unroll
    for (int f = 0; f < S_phi; ++f) {
        if (!UNSPLIT && f != S_Ei && f != S_h) continue;
        v[f][0] = *reinterpret_cast<const double2 *>(st + f * a.fstride + s0);
        v[f][1] = *reinterpret_cast<const double2 *>(st + f * a.fstride + s1);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        v[S_phi][j].x = concentration(p, v[S_Ei][j].x, v[S_h][j].x);
        v[S_phi][j].y = concentration(p, v[S_Ei][j].y, v[S_h][j].y);
    }
    if constexpr (UNSPLIT) {
        __syncthreads();                                  // every pair of the column has been read
#pragma unroll
        for (int f = 0; f <= S_phi; ++f) {
            *reinterpret_cast<double2 *>(st + f * a.fstride + 4 * t) = v[f][0];
            *reinterpret_cast<double2 *>(st + f * a.fstride + 4 * t + 2) = v[f][1];
        }
    } else {
        *reinterpret_cast<double2 *>(st + S_phi * a.fstride + s0) = v[S_phi][0];
        *reinterpret_cast<double2 *>(st + S_phi * a.fstride + s1) = v[S_phi][1];
    }
}
hipError_t launch_restore_phi(const StepArgs &a, int ncol, const LaunchCfg &cfg, bool unsplit, hipStream_t s) {
    if (cfg.cells != 4 || a.pitch != 4 * cfg.threads) return hipErrorInvalidValue;     // the variant's only geometry
    if (unsplit) restore_phi_kernel<true><<<dim3(ncol), cfg.threads, 0, s>>>(a, cfg.threads);
    else restore_phi_kernel<false><<<dim3(ncol), cfg.threads, 0, s>>>(a, cfg.threads);
    return hipGetLastError();
}

// ---- host-side launchers ----------------------------------------------------------------------
// The kernel of a plan: a table lookup that holds no rule (ebm_plan.h has them all).  nullptr: no plan, or a size that this
// build lacks (EBM_QUICK).
static KernelFn kernel_of(const StepPlan &p) {
    switch (p.family) {
        case K_CLASSIC:
            if (p.mode == OUT_SAVE) return p.cells == 2 ? classic_step_kernel<2, OUT_SAVE> : classic_step_kernel<4, OUT_SAVE>;
            if (p.mode == OUT_LOOP) return p.cells == 2 ? classic_step_kernel<2, OUT_LOOP> : classic_step_kernel<4, OUT_LOOP>;
            return p.cells == 2 ? classic_step_kernel<2, OUT_STATE> : classic_step_kernel<4, OUT_STATE>;
        case K_MIZ_STEP:
            return p.imex ? miz_step_kernels_imex(p) : p.grid == 0 ? miz_step_kernels_identity(p) : miz_step_kernels_nonuniform(p);
        case K_MIZ_FUSED:
            if (p.save()) return miz_save_kernels(p);
            if (p.cells == 2) return p.grid == 0 ? miz_fused_for<2, 0>(p.threads) : miz_fused_for<2, 1>(p.threads);
            return p.grid == 0 ? miz_fused_for<4, 0>(p.threads) : miz_fused_for<4, 1>(p.threads);
        case K_MIZ_RESIDENT: return p.save() ? miz_save_kernels(p) : miz_resident_kernels(p);
        default: return nullptr;
    }
}

bool has_step_kernel(const LaunchCfg &cfg, const StepVariant &v) { return kernel_of(plan_step(cfg, v)) != nullptr; }

// Dynamic LDS above the 64 KiB default must be requested per kernel: every plan of the geometry that needs it, each kernel once.
hipError_t prepare_kernels(const LaunchCfg &cfg) {
    std::set<KernelFn> raised;
    hipError_t e = hipSuccess;
    for_each_variant(cfg, [&](const LaunchCfg &c, const StepVariant &v) {
        const StepPlan plan = plan_step(c, v);
        if (e != hipSuccess || !needs_raised_lds(plan)) return;
        KernelFn fn = kernel_of(plan);
        if (!fn) e = hipErrorInvalidValue;
        else if (raised.insert(fn).second)
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
    });
    return e;
}

hipError_t launch_step_columns(const StepArgs &a, const StepPlan &plan, int first, int count, hipStream_t s) {
    KernelFn fn = kernel_of(plan);
    if (!fn || first < 0 || count < 1 || first + count > a.ncol) return hipErrorInvalidValue;
    if (a.noise && plan.noise_from_memory) {
        hipError_t e = launch_noise_sequence(a, first, count, s);
        if (e != hipSuccess) return e;
    }
    StepArgs b = a;
    b.col0 = first;
    fn<<<dim3(count), dim3(plan.threads), plan.lds_bytes, s>>>(b);
    return hipGetLastError();
}

hipError_t launch_mask_from_t0(const StepArgs &a, int ncol, const LaunchCfg &cfg, hipStream_t s) {
    mask_from_t0_kernel<<<ncol, cfg.threads, 0, s>>>(a, cfg.cells);
    return hipGetLastError();
}

hipError_t launch_finish_mean(double *dst, double *sum, double nt, int ncol, int nvars, long long var_stride,
                              const LaunchCfg &cfg, hipStream_t s) {
    finish_mean_kernel<<<dim3(ncol, nvars), cfg.threads, 0, s>>>(dst, sum, nt, cfg.threads, cfg.cells, var_stride);
    return hipGetLastError();
}

}  // namespace ebm
