// Internal declarations shared by the HIP kernels (the other .hip files of this directory) and the host runtime
// behind the C ABI (ebm_runtime.hip, ebm_fields.hip, ebm_columns.hip, ebm_drive.hip).  Not part of the public interface
// (include/ebm_hip.h).  The plain types and constants are in ebm_types.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ebm_plan.h"
#include "ebm_types.h"

namespace ebm {

// Per-step scalars of a graph-replayed step: kernel node `slot` of the replayed graph reads entry
// `slot` of a small device table that the host refills before every replay.
struct StepSched {
    double ct, ct_next, ft, tyear;
    long long n;                     // 0-based global index of the step (the noise's counter; tyear is year_time(n))
};

// Per-column AR(1) forcing noise (ebm_set_column_noise, include/ebm_hip.h): s = sigma*sqrt(1 - rho^2), the lag-one
// autocorrelation rho and the column's stream id.  One record per column, read with scalar loads.
struct NoiseRec {
    double s, rho;
    unsigned long long stream;
};

struct StepArgs {
    double *state;
    long long fstride;
    const double *geom;
    long long gstride;
    const double *fcol;              // per-column forcing offset or nullptr
    const double *fsched;            // per-column Forcing schedules [ncol][kSchedWords] or nullptr
    const Params *p;                 // device memory: the parameter sets, set i at p[i]
    const int *pset;                 // column -> parameter set [ncol] (ebm_set_column_params), or nullptr: every column set 0
    long long set_stride;            // geometry slab of set i at geom + i*set_stride (G_COUNT*gstride)
    unsigned long long *counters;    // 64 shards x {solves, cap hits} (MIZ)
    unsigned short *amask;           // MIZ warm start as an active set: [ncol][threads], bit i <=> T0 < Tm in cell i of the thread
    int pitch, nlat, ncol;
    int col0;                        // first column of this launch (workgroup b steps column col0 + b): launch chains
    double ct, ct_next, ft;          // cos(2 pi t) [MIZ / classic column i], classic column i+1, forcing
    double tyear;                    // model time of the step in years (st.T[tinx]), for the schedules
    const StepSched *sched;          // if non-null, ct/ct_next/ft come from sched[slot] instead (graph replay)
    int slot;
    int write_diag;
    int prefetch;                    // MIZ: L2 prefetch distance in columns (0 = off)
    int nfused;                      // fused launches: steps in this launch, scalars from sched[slot .. slot+nfused)
    // savesol! fused into the step (OUT_SAVE), src/infrastructure.jl:549-591:
    double *sums;                    // annual-mean running sums [nvars][ncol*pitch] in the pair-split layout, or nullptr
    long long sum_stride;            // ncol*pitch
    double *stage;                   // raw snapshots [nvars][chunk][ncol][pitch], or nullptr
    long long stage_var_stride;      // chunk*ncol*pitch
    long long stage_offset;          // snapshot index * ncol*pitch
    signed char var_of[kMaxQuantities];   // quantity -> saved-variable index, -1 = not saved
    unsigned long long *stamps;      // diagnostic builds only (EBM_STAMPS), else nullptr
    const int *cols;                 // active columns (ebm_equilibrate, ebm_run_until): workgroup b steps column cols[col0 + b]; nullptr =
                                     // identity.  Read by the fused-K kernels and the classic kernel only.
    // forcing noise (ebm_set_column_noise): nullptr = none, and every kernel takes the noise-free path
    const NoiseRec *noise;           // [ncol]
    double *nstate;                  // N_c [ncol]: read once per workgroup before its first barrier, written back by one
                                     // thread after its last
    double *nseq;                    // [ncol][kNoiseMaxFused]: N_c after each step of a fused launch (ColumnNoise, MEM)
    unsigned long long seed;
    long long step;                  // global index of the step of a one-step launch without sched (with sched: sched[slot].n)
};

// THE pair-split permutation of a column at four cells per thread (T threads, pitch 4T): pair j of thread t — the natural
// cells 4t + 2j and 4t + 2j + 1 — lies at split_index(t, j, T), so that the 16-byte accesses of a wave to one pair cover
// whole 128-byte lines.  The layout of the annual-mean sums, of the zonal operator's index space, of the diagnostic
// fields as a one-step launch leaves them and of the prognostic fields between one-step launches.  With two
// cells per thread the pair is the chunk and the layout is the natural one.
__host__ __device__ constexpr unsigned split_index(unsigned t, unsigned j, unsigned T) { return j * 2u * T + 2u * t; }
// ... read backwards, in units of one pair (16 bytes; a row has 2T of them): the natural unit that stored unit p of a row
// stands for — p itself unless the row is held pair-split (ebm_ensemble.hip, ebm_covariance.hip)
__host__ __device__ constexpr int natural_unit(int p, int T, bool split) { return !split ? p : (p < T ? 2 * p : 2 * (p - T) + 1); }

// The zero-line flags of a MIZ handle (miz_step_kernel, ZERO_LINES; ebm_device.h): zero_flag_count 32-bit words, one per
// (column, wave), which lie behind the ncol rows of `threads` mask words in the allocation of StepArgs::amask — so the
// launch arguments, and with them every kernel that knows nothing of the flags, are what they were.  Nothing that moves mask
// rows between columns touches them.
__host__ __device__ inline unsigned *zero_flag_words(unsigned short *amask, int ncol, int threads) {
    return reinterpret_cast<unsigned *>(amask + (size_t)ncol * (size_t)threads);
}
__host__ __device__ constexpr size_t zero_flag_count(int ncol, int threads) { return (size_t)ncol * (size_t)(threads / 64); }

// The step kernels (ebm_plan.h decides which).  One workgroup per column; the fused modes run a.nfused steps per launch.
using KernelFn = void (*)(const StepArgs);
// The MIZ kernels, one accessor per translation unit (miz_step_*.hip, miz_resident*.hip), each for the plans that kernel_of
// sends it; nullptr = size not compiled
KernelFn miz_step_kernels_identity(const StepPlan &p);      // K_MIZ_STEP of the reference's step, deriving and eliding included
KernelFn miz_step_kernels_nonuniform(const StepPlan &p);
KernelFn miz_step_kernels_imex(const StepPlan &p);          // K_MIZ_STEP of the extension, both grids
KernelFn miz_resident_kernels(const StepPlan &p);           // K_MIZ_RESIDENT without savesol!'s sums
KernelFn miz_save_kernels(const StepPlan &p);               // K_MIZ_RESIDENT and the two-cell K_MIZ_FUSED with the sums

hipError_t prepare_kernels(const LaunchCfg &cfg);   // raises the dynamic-LDS limit of every plan of the geometry that needs it
bool has_step_kernel(const LaunchCfg &cfg, const StepVariant &v);   // is there a plan, and is its kernel compiled?
// `count` workgroups of the plan's kernel, stepping columns first ... first + count - 1; with noise installed, after the
// launch's noise sequence where the plan says the kernel reads it from memory.  Whoever asked for a deriving or eliding
// plan answers for the state and the zero-line flags (zero_flag_words).
hipError_t launch_step_columns(const StepArgs &a, const StepPlan &plan, int first, int count, hipStream_t s);
// rcp_dt / rcp_cdn of the device-resident parameter block (see Params)
hipError_t launch_derive_params(Params *p_dev, hipStream_t s);
// active set from the T0 field (after ebm_set_field(T0))
hipError_t launch_mask_from_t0(const StepArgs &a, int ncol, const LaunchCfg &cfg, hipStream_t s);
hipError_t launch_divide(const double *a, const double *b, double *q, int n, hipStream_t s);
// out[v * var_stride + col] = hemispheric_mean(field in slot slot[v] of column col, x), src/utilities.jl:397-403, for
// v < nvars, col < ncol: the sequential sum, bit-exact, by hemispheric_means_of_column (ebm_launch.hip) — the one definition
// of the mean in the library.  One wave per column, one launch.  Field v of column col starts at
// state + slot[v] * fstride + col * pitch, natural layout: a handle's slab with its slots, or any [nvars][ncol][pitch]
// buffer with slot[v] = v; one field is nvars = 1, slot[0] = 0.
constexpr int kMeanTile = 512;       // terms per LDS tile and variable: at most 12 x 513 doubles = 48 KiB of LDS
struct MeansArgs {
    const double *state;
    long long fstride;
    const double *x;
    double *out;                     // ebm_run_series: the sample's first word in the device series [nvars][nsamples][ncol]
    long long var_stride;            // ... and nsamples * ncol
    int pitch, nlat, nvars;
    int row;                         // doubles per variable of the LDS tile (odd; set by the launcher)
    int slot[kMaxQuantities];
};
hipError_t launch_hemispheric_means(const MeansArgs &s, int ncol, hipStream_t st);
// out = base + D d/dx[(1-x^2) d temp/dx] per column ([ncol][pitch] device arrays; base may be null)
// (parameter set of column c: pset[c], or 0 if pset is null — see StepArgs)
hipError_t launch_diffusion(const double *temp, const double *base, double *out, const double *geom, long long gstride,
                            const Params *p, const int *pset, long long set_stride, int grid_kind, int pitch, int nlat,
                            int ncol, hipStream_t s);
// annual_mean (src/infrastructure.jl:536-544): dst[v][col][k] = sum[v]/nt with `sum` in the pair-split
// layout of the step kernels, then sum = 0; all nvars variables (var_stride apart) in one launch
hipError_t launch_finish_mean(double *dst, double *sum, double nt, int ncol, int nvars, long long var_stride,
                              const LaunchCfg &cfg, hipStream_t s);
// Zonal diffusion substep (ebm_zonal_diffusion): per member and latitude the periodic tridiagonal solve along the circle.
// Everything lives in the handle's store index space p (4 cells per thread: pair-split, p = j*2T + 2t + q <-> latitude
// k = 4t + 2j + q; 2 cells per thread: p = k), so that all accesses are contiguous: T, out_Z, out_U [ncol][pitch];
// zM, zE [nlon][pitch]; za, zW [pitch].  out_Z is also the scratch of the forward sweep; out_U may be null.
hipError_t launch_zonal_sweep(const double *T, double *out_Z, double *out_U, const double *zM, const double *zE,
                              const double *za, const double *zW, int nlon, int nmember, int pitch, double rtheta,
                              hipStream_t s);
// The same systems partitioned along the circle into S segments (circles of >= 256 longitudes): chain tables cM, cE
// [nlon/S - 1][pitch] of one segment, reduced-system tables rM, rE [S - 1][pitch], za, za2, rW [pitch]; su, sg, sy are
// scratch [nmember][S][pitch].  Three launches.
hipError_t launch_zonal_sweep_segmented(const double *T, double *out_Z, double *out_U, const double *cM, const double *cE,
                                        const double *rM, const double *rE, const double *za, const double *za2,
                                        const double *rW, double *su, double *sg, double *sy, int nlon, int S, int nmember,
                                        int pitch, double rtheta, hipStream_t s);
// ebm_equilibrate, one workgroup per active column c = cols[b], b < nactive: for every criterion field v (state slot
// slot[v]) d = max over k < nlat of |field - snap| (NaN-propagating), snap = field; if `compare`, resid[v][c] = d; then
// years[c] = year and frozen[c] = (may_freeze && d <= tol[v] for every v)
struct EquilArgs {
    const double *state;
    long long fstride;
    double *snap;                    // [nvars][ncol][pitch], last year's snapshot
    double *resid;                   // [nvars][ncol]
    int *years, *frozen;             // [ncol]
    const int *cols;                 // [nactive], ascending
    int pitch, nlat, ncol, nvars;
    int year, compare, may_freeze;
    int slot[kMaxQuantities];
    double tol[kMaxQuantities];
};
hipError_t launch_equilibrium_check(const EquilArgs &e, int nactive, hipStream_t s);
// ebm_run_until, one wave per active column c = cols[b], b < nactive: m = hemispheric_mean(field of column c, x), the bits of
// hemispheric_means_of_column; value[c] = m, samples[c] = round and frozen[c] = (direction[c] > 0 ? m >= level[c] : m <= level[c])
struct PassageArgs {
    const double *field;             // the one field, [ncol][pitch], natural layout
    const double *x;
    const double *level;             // [ncol]
    const int *direction;            // [ncol], never 0
    const int *cols;                 // [nactive], ascending
    double *value;                   // [ncol]
    int *samples, *frozen;           // [ncol]
    int pitch, nlat, round;
    // ebm_run_until_scalar: m = the column scalar (kind, k0, k1, edge_level) of the field in place of its mean
    int scalar;                      // 0: the hemispheric mean (ebm_run_until)
    int kind, k0, k1;
    double edge_level;
};
hipError_t launch_passage_check(const PassageArgs &p, int nactive, hipStream_t s);
// Column scalars (ebm_column_scalars, include/ebm_hip.h: the definition): out[s * out_stride + col] = scalar s of column col <
// ncol, by column_scalar (ebm_launch.hip) — the integral kinds through hemispheric_means_of_column on the band, the edge kinds
// by a search for the first hit and one interpolation.  One wave per (column, scalar), one launch.  row[s]: the field of
// scalar s, [ncol][pitch], natural layout (several scalars may name one row); 0 <= k0[s] <= k1[s] < nlat, checked by the caller.
// ebm_run_series_scalars: `out` is the sample's first word in the device series [nscal][nsamples][ncol].
enum ScalarKind { S_INTEGRAL = 0, S_MEAN = 1, S_EDGE_GE = 2, S_EDGE_LE = 3, S_KINDS = 4 };     // enum ebm_scalar_kind
struct ScalarArgs {
    const double *row[kMaxQuantities];
    const double *x;
    double *out;
    long long out_stride;
    double level[kMaxQuantities];
    int kind[kMaxQuantities], k0[kMaxQuantities], k1[kMaxQuantities];
    int pitch, nscal;
};
hipError_t launch_column_scalars(const ScalarArgs &a, int ncol, hipStream_t s);
// the next active list: out = the entries of in[0 .. n) whose column is not frozen, in order; *count = their number
// (one workgroup)
hipError_t launch_compact_active(const int *in, int n, const int *frozen, int *out, int *count, hipStream_t s);
// ebm_noise_innovations: out[c][i] = xi(seed, noise[c].stream, first + i), c < ncol, i < nsteps, by the function the step
// kernels call
hipError_t launch_noise_innovations(const NoiseRec *noise, unsigned long long seed, long long first, int nsteps, int ncol,
                                    double *out, hipStream_t s);
// natural <-> pair-split layout (split_index) of whole fields ([ncol][pitch], 4 cells per thread; a no-op with 2), in
// place: nfields fields, field_stride apart
hipError_t launch_split_fields(double *fields, long long field_stride, int nfields, int ncol, const LaunchCfg &cfg,
                               hipStream_t s);
hipError_t launch_unsplit_fields(double *fields, long long field_stride, int nfields, int ncol, const LaunchCfg &cfg,
                                 hipStream_t s);
// The phi field of every column written again from the column's Ei and h and its own parameter set (concentration, the
// step kernels' piece: the bits a step that stores phi would have left), after one-step launches that did not store it;
// the five prognostic fields pair-split (four cells per thread).  unsplit: in the same pass the five fields go to the
// natural layout (what launch_unsplit_fields does to them); else in place, only phi is written.
hipError_t launch_restore_phi(const StepArgs &a, int ncol, const LaunchCfg &cfg, bool unsplit, hipStream_t s);
// ebm_resample_columns (ebm_resample.hip), one workgroup per entry m < moved of the list: `stage` copies row list[m].y (the
// parent) of `rows` to row m of `stage`, `scatter` row m of `stage` to row list[m].x (the destination) of `rows`.  Rows in
// units of 16 bytes: `units` of them are copied, row_stride / stage_stride apart.  nstate (null: none): N_c goes the same
// way, through the double behind the units of staging row m — so stage_stride >= units + 1.
struct ResampleArgs {
    uint4 *rows;
    long long row_stride;
    uint4 *stage;
    long long stage_stride;
    const int2 *list;                // [moved] (destination, parent), both < ncol
    int units;
    double *nstate;
};
hipError_t launch_resample_stage(const ResampleArgs &r, int moved, hipStream_t s);
hipError_t launch_resample_scatter(const ResampleArgs &r, int moved, hipStream_t s);
// ebm_export_columns / ebm_import_columns (ebm_exchange.hip), one workgroup per (list entry i < n, slot): export copies the
// rows of column cols[i] to record i of `buf`, import the rows of record records[i] (null: i) to column cols[i].  A record is
// `record` doubles: nfields field slots of rowlen doubles in the natural layout, the active-set row, N_c and one reserved
// double.  row[s] null: slot s does not move; bit s of split_mask: the handle holds the rows of slot s pair-split.
constexpr int kExchangeSlots = 11;   // fields of the largest model (MIZ: Ei .. T)
struct ExchangeArgs {
    double *row[kExchangeSlots];     // the field of slot s, [ncol][pitch], or null
    unsigned split_mask;
    const int *cols;                 // [n], all < ncol
    const int *records;              // [n] or null (import only)
    double *buf;                     // 16-byte aligned
    long long record;                // doubles per record (even)
    unsigned short *amask;           // [ncol][threads] or null (then amask_units = 0)
    double *nstate;                  // N_c [ncol] or null: export writes 0.0, import leaves the tail unread
    int nfields, rowlen, pitch, threads, amask_units;
};
hipError_t launch_export_columns(const ExchangeArgs &a, int n, hipStream_t s);
hipError_t launch_import_columns(const ExchangeArgs &a, int n, hipStream_t s);
// ebm_ensemble_sums, ebm_ensemble_range and ebm_ensemble_histogram (ebm_ensemble.hip): out[v][slot][k], slot < nslots, of
// entry v of the call at latitude k < nlat, reduced over the columns in the order of the definition (include/ebm_hip.h) —
// blocks of columns in ascending column order into partial[block][v][slot][pitch], then the blocks in ascending order.  Two
// launches each.  row[v]: the field of entry v, [ncol][pitch], read where it lies (an entry of a histogram may name the row of
// an earlier one); bit v of split_mask: the handle holds it pair-split (then partial is in that layout too; aux and out never
// are).
//   sums       slots S0, S1, S2; blocks of kSumsBlock columns.  aux: center[v][pitch], or null: nothing is subtracted.
//   range      slots n, min, max; blocks of kRangeBlock columns (the result does not depend on the blocking).  aux: unused.
//   histogram  nslots = nbins + 2; blocks of kHistBlock columns.  aux: edges[v][0..2][pitch] = lo, hi and s = nbins / (hi - lo),
//              padding zero.
constexpr int kSumsBlock = 32;       // columns per block of the sums: part of the definition (include/ebm_hip.h)
constexpr int kRangeBlock = 32;      // columns per block of the range: performance only
constexpr int kHistBlock = 256;      // columns per block of the histogram: part of the definition (include/ebm_hip.h)
constexpr int kHistMaxBins = 64;
struct EnsembleArgs {
    const double *row[kMaxQuantities];
    unsigned split_mask;
    int nslots;
    const double *w;                 // [ncol], finite; never written by a kernel
    const double *aux;               // the per-latitude input in natural latitude order, or null
    double *partial;                 // [nblocks][nvars][nslots][pitch]
    double *out;                     // [nvars][nslots][nlat], natural
    int pitch, nlat, ncol, nvars, nblocks, threads;
};
hipError_t launch_ensemble_sums(const EnsembleArgs &a, hipStream_t s);
hipError_t launch_ensemble_range(const EnsembleArgs &a, hipStream_t s);
hipError_t launch_ensemble_histogram(const EnsembleArgs &a, hipStream_t s);
// ebm_ensemble_covariance (ebm_covariance.hip): out[i][j] = sum over the columns of a * b, a the weighted, centred and
// NaN-cleaned cell of row_a at latitude i and b the centred and NaN-cleaned cell of row_b at latitude j, in the order of the
// definition (include/ebm_hip.h) — blocks of kCovBlock columns, inside a block one fp64 MFMA per four columns in ascending
// order (the chain of ebm_mfma_tile.h), into partial[block][stored i][stored j], then the blocks in ascending order.  Two
// launches.  The rows are read where they lie (split_a, split_b: the handle holds that row pair-split; partial is indexed by
// the stored cells of both); the centers and out are in natural latitude order.  symmetric: rule 6 of the definition — only
// j >= i is computed, out[j][i] is a copy.
constexpr int kCovBlock = 512;       // columns per block of the covariance: part of the definition (include/ebm_hip.h)
struct CovarianceArgs {
    const double *row_a, *row_b;     // [ncol][pitch]
    bool split_a, split_b, symmetric;
    const double *w;                 // [ncol], finite; never written by a kernel
    const double *center_a, *center_b;      // [pitch] each, padding zero, or null: nothing is subtracted
    double *partial;                 // [nblocks][pitch][pitch]
    double *out;                     // [nlat][nlat], natural
    int pitch, nlat, ncol, nblocks, threads;
};
hipError_t launch_ensemble_covariance(const CovarianceArgs &a, hipStream_t s);
// ebm_update_columns (ebm_update.hip): row[v][c][k] <- clamp(row[v][c][k] + sum_j gain[v][k][j] * d[c][j]) in the order of the
// definition (include/ebm_hip.h) — d staged first for all columns by launch_update_innovations from obs as it lies, then one
// fp64 MFMA per four observation cells in ascending order, d the A operand (the chain of ebm_mfma_tile.h).  row[v], obs:
// [ncol][pitch], read and written where they lie (bit v of split_mask, obs_split: the handle holds that row pair-split).
// gain, target, perturb and d are in natural latitude order: gain[v] at gain + v * gain_field, its row k at k * gain_row (only
// k, j < nlat are read); target[pitch]; perturb [ncol][nlat] packed or null; d [ncol][pitch], every cell at or beyond nlat
// written +0.0.
constexpr int kUpdateMaxFields = 5;
struct UpdateArgs {
    double *row[kUpdateMaxFields];
    unsigned split_mask;
    bool obs_split;
    const double *obs;
    const double *gain;
    long long gain_field, gain_row;
    const double *target;
    const double *perturb;
    double *d;
    double scale;
    double lo[kUpdateMaxFields], hi[kUpdateMaxFields];    // -Inf / +Inf: no bound
    int pitch, nlat, ncol, nvars, threads;
};
hipError_t launch_update_innovations(const UpdateArgs &a, hipStream_t s);
hipError_t launch_update_product(const UpdateArgs &a, hipStream_t s);
// ebm_column_misfits (ebm_misfit.hip): out[t][0][c] = J and out[t][1][c] = N of column c against target t, summed along the
// column in the order of the definition (include/ebm_hip.h).  One launch, one wave per column.  row[v], split_mask: as above.
// target[t][v][pitch] and rw[v][pitch] (null: every entry 1.0) in natural latitude order; their padding cells are never read
// into a result.
constexpr int kMisfitMaxTargets = 8;
struct MisfitArgs {
    const double *row[kMaxQuantities];
    unsigned split_mask;
    int ntargets;
    const double *target;
    const double *rw;
    double *out;                     // [ntargets][2][ncol]
    int pitch, nlat, ncol, nvars, threads;
};
hipError_t launch_column_misfits(const MisfitArgs &a, hipStream_t s);
// ebm_spd_solve_device and ebm_kalman_gain_device (ebm_gain.hip): X . S = B for a symmetric positive definite S by a blocked
// Cholesky factorisation, in the order of the definition (include/ebm_hip.h), every product a chain of ebm_mfma_tile.h on
// tiles of kGainBlock x kGainBlock.  Everything works on mp = m rounded up to kGainBlock:
// S is [mp][lds >= mp] with the identity in its padding, B is [nrhs][ldb >= mp] with +0.0 in its padding columns.
// inv: [mp / kGainBlock][kGainBlock][kGainBlock], the inverses of the diagonal blocks of L.  flag: one int, 0 before the first
// launch; the 1-based index of the first pivot that is not > 0 afterwards, and then every later launch does nothing.
constexpr int kGainBlock = 64;       // nb of the blocked factorisation: part of the definition (include/ebm_hip.h)
struct SolveArgs {
    double *S;
    long long lds;
    double *B;
    long long ldb, nrhs;
    double *inv;
    int *flag;
    int mp;
};
hipError_t launch_spd_factor(const SolveArgs &a, hipStream_t s);     // 3 launches per block column (the last one: 1)
hipError_t launch_spd_solve(const SolveArgs &a, hipStream_t s);      // 2 launches
// The compacted system of the observed cells J (index[a], a < m, ascending; pos[j] = a where index[a] == j, else -1):
// assemble writes S and, per field v < nvars, the rows (v * nlat + k) of B; scatter writes gain[v][k][j] = X or +0.0.
struct GainArgs {
    const double *Poo;               // [nlat][nlat]
    const double *Pfo[kUpdateMaxFields];
    const double *x;                 // st.x [nlat]
    const double *obs_var;           // [nlat]
    const int *index, *pos;          // [m], [nlat]
    const int *flag;                 // the solve's: scatter does nothing where it is set
    double localize, factor;         // localize <= 0: rho == 1.0
    double *S, *B, *gain;            // [mp][mp], [nvars * nlat][mp], [nvars][nlat][nlat]
    int nlat, nvars, m, mp;
};
hipError_t launch_gain_assemble(const GainArgs &a, hipStream_t s);   // 2 launches
hipError_t launch_gain_scatter(const GainArgs &a, hipStream_t s);

}  // namespace ebm
