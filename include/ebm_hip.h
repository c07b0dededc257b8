/* ebm_hip.h — C ABI of the MI355X-native energy-balance time-stepping path.
 *
 * This is the drop-in boundary for the hot path of waylonwh/EnergyBalanceModel.jl:
 *
 *   Infrastructure.step!(::Val{:MIZ}|::Val{:Classic}, t, f, vars, st, par; debug, verbose)
 *       stub   src/infrastructure.jl:594
 *       MIZ    src/miz.jl:150-196        classic  src/classic.jl:37-71
 *   Infrastructure.integrate(model, st, forcing, par, init; lastonly, debug, verbose)
 *       src/infrastructure.jl:615-636 (+ savesol! :549-591, annual_mean :536-544)
 *
 * The reference is pure Julia and has no FFI of its own; the entry points below are what a
 * Julia `ccall` shim binds (julia/EBMHip.jl).  The shim's two supported calls keep
 * the reference's signatures and model symbols, as functions of the shim module:
 *     EBMHip.integrate(:MIZ | :Classic, st, forcing, par, init; lastonly, verbose)   -> ebm_integrate
 *     EBMHip.step!(Val(:MIZ | :Classic), t, f, vars, st, par; verbose)               -> ebm_step
 * (no new model tag: the reference decides on the symbol's value what a run stores and which
 * parameters it gets, src/infrastructure.jl:621-624, :473-474).  Plain C: opaque handle,
 * `double*`/`int` only, no C++/torch types.  All arrays are fp64, latitude contiguous:
 * a field is `[ncol][nlat]` in C order == Julia `Array{Float64,2}(nlat, ncol)`; a column is
 * one independent meridian (a longitude of a 2-D grid and/or an ensemble member).
 *
 * Threading: all state — including the T0 warm start the reference hides in a module-level
 * closure (src/miz.jl:47,64) — is owned by the handle.  Different handles may be used from
 * different host threads; one handle must not be used concurrently.
 *
 * Errors: every function returns 0 on success, a negative ebm_status otherwise; the message
 * is available (per host thread) from ebm_last_error().  Numerical events are not errors:
 * NaN sentinels are data (src/miz.jl:193-194) and a T0 iteration that hits its cap is only
 * counted (the reference merely warns, src/miz.jl:61-63) — see ebm_get_counters.
 */
#ifndef EBM_HIP_H
#define EBM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ebm_ctx *ebm_handle_t;

enum ebm_status {
    EBM_OK = 0,
    EBM_ERR_ARG = -1,      /* bad argument */
    EBM_ERR_HIP = -2,      /* HIP runtime error */
    EBM_ERR_UNSUPPORTED = -3,
    EBM_ERR_NO_DEVICE = -4, /* no usable GPU: the library never falls back to the CPU */
    EBM_ERR_STALE = -5      /* the requested field is older than the state (see "Validity" below) */
};

/* model tag == the Val{...} the reference dispatches step! on (src/infrastructure.jl:594).
 *
 * EBM_MODEL_MIZ_IMEX is an EXTENSION with no counterpart in the reference (and therefore no parity to
 * claim): the MIZ model with its meridional diffusion treated linearly implicitly.  Each step the explicit
 * increment of every cell's total enthalpy, dE = dt*(phi*Fvi + (1-phi)*Fvw), goes through one tridiagonal
 * solve per meridian, (I - (dt/cw)*Dif) dE_new = dE, and the diffusion term of both vertical fluxes
 * (src/miz.jl:96-101) is corrected by (dE_new - dE)/dt; everything else is the reference's step.  This lifts
 * the explicit limit dt <= cw*dx^2/(2D) (more than 800,000 steps per year at 4096 latitudes) and converges
 * to the reference's scheme as dt -> 0.  Dif is the operator D d/dx[(1-x^2) d/dx] as a plain tridiagonal
 * matrix (zero-flux ends); assuming that the surface temperature follows the increment with the water's
 * heat capacity cw is an upper bound of the true response (heat that melts or grows ice changes no
 * temperature), which is what makes the scheme stable.  THIS TEXT IS THE DEFINITION.
 * Same fields, parameters and entry points as EBM_MODEL_MIZ, ebm_run_fused included. */
enum ebm_model { EBM_MODEL_MIZ = 0, EBM_MODEL_CLASSIC = 1, EBM_MODEL_MIZ_IMEX = 2 };

/* SpaceTime{identity} uses the sparse uniform-x operator (src/infrastructure.jl:495-497);
 * every other SpaceTime{F} (e.g. sin) the flux-form stencil (:505-526). */
enum ebm_grid { EBM_GRID_IDENTITY = 0, EBM_GRID_NONUNIFORM = 1 };

/* order of the 25 entries of default_parval (src/infrastructure.jl:407-433) */
enum ebm_param {
    EBM_P_D = 0, EBM_P_A, EBM_P_B, EBM_P_cw, EBM_P_S0, EBM_P_S1, EBM_P_S2, EBM_P_a0, EBM_P_a2,
    EBM_P_ai, EBM_P_Fb, EBM_P_k, EBM_P_Lf, EBM_P_F, EBM_P_cg, EBM_P_tau, EBM_P_Tm, EBM_P_m1,
    EBM_P_m2, EBM_P_alpha, EBM_P_rl, EBM_P_Dmin, EBM_P_Dmax, EBM_P_hmin, EBM_P_kappa,
    EBM_P_COUNT
};

/* fields of `vars` (src/infrastructure.jl:604-605, 621-624) plus the hidden warm start */
enum ebm_field {
    EBM_F_Ei = 0, EBM_F_Ew, EBM_F_h, EBM_F_D, EBM_F_phi, /* MIZ prognostics (init)          */
    EBM_F_T0,                                             /* MIZ warm start (src/miz.jl:47), see below */
    EBM_F_Tw, EBM_F_Ti, EBM_F_n, EBM_F_E, EBM_F_T,        /* MIZ diagnostics; E,T also classic */
    EBM_F_Tg,                                             /* classic ghost layer             */
    EBM_F_COUNT
};
/* classic uses EBM_F_E, EBM_F_Tg (prognostic) and EBM_F_T, EBM_F_h (diagnostic).
 *
 * EBM_F_T0: the reference keeps the previous T0 solution as the starting iterate of its nonlinear
 * solve.  The active-set iteration used here depends on that vector only through its sign pattern
 * [T0 < Tm], so between steps the library carries that pattern (one bit per cell) and writes the
 * fp64 EBM_F_T0 field together with the diagnostics (write_diag / diag_last != 0).
 * ebm_set_field(EBM_F_T0, ...) rebuilds the pattern from the given values. */

/* ---- lifetime ------------------------------------------------------------------------ */

/* Create a stepping context on HIP device `device` for `ncol` independent meridians of
 * `nlat` cells (2 <= nlat <= 4096: one workgroup owns a whole meridian; longer ones are refused with
 * EBM_ERR_UNSUPPORTED).  x[nlat] is st.x, params[EBM_P_COUNT] the parameter values (entries a model
 * does not use are ignored), dt = st.dt.  All state starts at zero (as the reference's T0
 * warm start does).  Fails with EBM_ERR_NO_DEVICE when no GPU is present. */
int ebm_create(ebm_handle_t *out, int model, int grid, int nlat, int ncol, const double *x,
               const double *params, double dt, int device);

/* Launch options.  The library reads NO environment variable: whatever changes how a handle runs is passed
 * here.  Zero-initialise (or call ebm_options_default) and set struct_bytes = sizeof(ebm_options); fields the
 * caller's struct does not have keep their defaults, so the struct can grow.
 *
 * cells_per_thread: latitudes per thread of the one workgroup that owns a meridian — 4 (default: 32
 *   contiguous bytes per lane and field, the throughput geometry) or 2 (nlat <= 1536: twice as many waves
 *   per meridian, for latency-bound runs of a FEW short meridians, e.g. one 180-band column).  The
 *   tridiagonal partition, hence the ROUNDING of the T0 / Tg solves, depends on this number and on nothing
 *   else a caller controls: the geometry is a function of (nlat, cells_per_thread) only — never of ncol — so
 *   a member gives the same bits alone, inside a large ensemble, and under any sharding over GPUs, as long as
 *   every rank passes the same options.
 * use_graph: replay hipGraphs of 64 captured step launches in ebm_run (-1 = by size: on for steps of at most
 *   262,144 cells, which are launch-bound; 0 = off; 1 = on).  Bit-identical either way.
 * prefetch_cols: L2-prefetch distance of the MIZ step kernel in columns (-1 = the successor workgroup on the
 *   same XCD when at most two workgroups fit a CU, else off; 0 = off).  Performance only.
 * launch_chains: 1 (and -1, the default) = every step is one launch over all columns; 2 = the two halves of the columns
 *   are stepped by two independent chains of launches on two streams, which fill each other's launch boundaries and store
 *   tails: worth it where a CU holds a single workgroup (meridians of more than 2048 cells) and every chain still fills
 *   the chip several times over (4096 x 2048: 0.1656 -> 0.1594 ms per step).  Columns are independent: bit-identical either
 *   way.  ebm_get_counters counts one launch per chain and step; ignored with graph replay.
 * fused_state_in_lds: where the fused-K launches (ebm_run_fused) of the reference's step keep the state when both of its
 *   kernels exist (four cells per thread, meridians of up to 2048 cells): 0 = in registers (fewest LDS round trips: the
 *   fastest for a few columns), 1 = in LDS (128 registers per lane, so that up to four workgroups share a CU and fill each
 *   other's barrier stalls: 1.15 ... 1.45 x the throughput on launches of many columns), -1 (default) = in LDS when the
 *   handle has more columns than the register kernel runs in one round (one 256-thread workgroup per compute unit, four of
 *   64 threads).  Performance only: the two kernels compute the same bits.
 * integrate_steps_per_launch: how ebm_integrate / ebm_integrate_hemispheric step through the stretches of a year that need
 *   nothing but the annual-mean sums (no raw snapshot, no seasonal snapshot, not a year's last step): -1 (default) and
 *   values > 1 = that many steps fused into one launch with the state resident on the chip and the sums taken from
 *   every step (default 64); 1 = one launch per step everywhere.  Bit-identical either way.  MIZ and MIZ_IMEX (not two
 *   cells per thread on meridians of more than 1024 cells); other handles always step one launch at a time.
 * elide_zero_lines: the state-only one-launch-per-step MIZ kernel that derives phi (four cells per thread, the reference's
 *   step) neither loads nor stores a KiB of Ei, Ew, h or D that holds only zero bits — what ice-free cells hold in Ei, h
 *   and D, and water at the freezing point under ice in Ew.  It keeps one flag per KiB on the device (ebm_zero_line_flags) and
 *   trusts it only while nothing but that kernel has written the prognostic fields; memory stays complete and current at all
 *   times, so nothing a caller can see changes, bit for bit.  -1 (default) and 1 = on where the handle has that kernel,
 *   0 = off. */
typedef struct ebm_options {
    int struct_bytes;
    int cells_per_thread;
    int use_graph;
    int prefetch_cols;
    int launch_chains;
    int integrate_steps_per_launch;
    int fused_state_in_lds;
    int elide_zero_lines;
} ebm_options;
int ebm_options_default(ebm_options *opt);
/* ebm_create with explicit options (opt == NULL: the defaults, i.e. exactly ebm_create). */
int ebm_create_ex(ebm_handle_t *out, int model, int grid, int nlat, int ncol, const double *x,
                  const double *params, double dt, int device, const ebm_options *opt);
int ebm_destroy(ebm_handle_t h);
const char *ebm_last_error(void);
const char *ebm_version(void);

/* ---- state --------------------------------------------------------------------------- */

/* Copy a whole field host<->device ([ncol][nlat] doubles, synchronous).  The copies run through a pinned
 * staging ring owned by the handle (device -> pinned by DMA while the previous piece is copied on to the
 * caller's pageable buffer by a few host threads).
 *
 * Validity.  The prognostic fields are always current.  The diagnostic fields (MIZ: Tw, Ti, n, E, T; classic:
 * T, h) and the fp64 warm start EBM_F_T0 are written only by steps that were asked to (ebm_step with
 * write_diag, the last step of ebm_run / ebm_run_fused with diag_last, the seasonal and last steps of
 * ebm_integrate).  A read of one of them — ebm_get_field, ebm_get_field_device, ebm_hemispheric_mean*,
 * ebm_ensemble_sums*, ebm_ensemble_range*, ebm_ensemble_histogram*, ebm_ensemble_covariance*, ebm_column_misfits*, ebm_column_scalars*, ebm_field_device_ptr — while the state is NEWER than the field (steps taken since without diagnostics, or
 * a prognostic field overwritten with ebm_set_field or ebm_update_columns*, the other writer of prognostic fields) fails with EBM_ERR_STALE; the message names the step
 * that last wrote the field and the state's step.  Nothing stale is ever returned silently — in particular
 * not the T0 a caller would checkpoint as the warm start (src/miz.jl:47,64).  ebm_field_step reports both
 * steps; ebm_get_field_as_of returns the field as of an EXPLICITLY named step (the 0-based global index of
 * the step that wrote it) however far the state has moved on since, and fails with EBM_ERR_STALE if that is
 * not the step that wrote it.  ebm_set_field(EBM_F_T0) makes T0 current; setting a diagnostic field directly
 * makes that field current as well (it is the caller's statement of what it holds). */
int ebm_set_field(ebm_handle_t h, int field, const double *host);
int ebm_get_field(ebm_handle_t h, int field, double *host);
/* *written_step: 0-based global index of the step that last wrote the field (-1: never written; for a field
 * set by the caller: the index of the last step taken before that, -1 if none); *state_step: the same for
 * the prognostic state.  The field is current iff the two are equal and no prognostic field has been
 * overwritten since (*current != 0).  Any output pointer may be NULL. */
int ebm_field_step(ebm_handle_t h, int field, long long *written_step, long long *state_step, int *current);
int ebm_get_field_as_of(ebm_handle_t h, int field, long long step, double *host);
/* hemispheric_mean (src/utilities.jl:397-403) of a field, per column, reduced on the device in the
 * reference's summation order (bit-identical): out[ncol] on the host.  Ensemble diagnostics are
 * O(columns) instead of O(state).  Synchronous. */
int ebm_hemispheric_mean(ebm_handle_t h, int field, double *out);
/* Device-to-device variants for callers that keep their own device buffers (e.g. the payload of an
 * RCCL gather): dev_out[ncol] / dev_out[ncol][nlat] packed, on the handle's device.  Synchronous. */
int ebm_hemispheric_mean_device(ebm_handle_t h, int field, double *dev_out);
int ebm_get_field_device(ebm_handle_t h, int field, double *dev_out);
/* The meridional diffusion operator on its own — diffusion!(base, temp, st, par) / diffusion(T, st, par)
 * = D∇², src/infrastructure.jl:495-533: out = base + D d/dx[(1-x^2) d temp/dx] per column, with the
 * handle's grid kind (identity: the CSC product of par.D*get_diffop, :495-497; any other grid: the flux
 * form, :505-526) and the very device functions the step kernels fuse — bit for bit the reference's
 * operation order.  temp, base (NULL = zeros), out: [ncol][nlat] host arrays.  MIZ handles only.
 * Synchronous. */
int ebm_diffusion(ebm_handle_t h, const double *temp, const double *base, double *out);
/* The ZONAL partner of the meridional operator above, as an implicit substep — an EXTENSION with no counterpart in the
 * reference (the reference has no longitude axis; the nearest text is the meridional operator,
 * src/infrastructure.jl:505-526), hence no parity to claim.  The columns of the handle are read as nmember = ncol / nlon
 * latitude-longitude grids of nlon equally spaced longitudes (column = member*nlon + longitude, periodic).  The zonal part
 * of the spherical diffusion operator, D/(1-x^2) d^2/dlambda^2, cannot be taken explicitly near the pole (1-x^2 = 6e-7 at
 * the last of 1024 latitudes); this is its backward-Euler step over the handle's dt on a field with the water's heat
 * capacity cw: for every member and latitude k solve the periodic tridiagonal system along the latitude circle
 *     (1 + 2 a_k) U_l - a_k (U_{l-1} + U_{l+1}) = temp_l,    a_k = (dt/cw) D / ((1 - x_k)(1 + x_k) dlambda^2),  dlambda = 2 pi/nlon
 * (1 - x^2 is evaluated as (1 - x)(1 + x), which does not cancel near the pole) and form the zonal heat-flux convergence
 *     Z_l = (U_l - temp_l) cw/dt      ( = D/((1-x_k^2) dlambda^2) (U_{l-1} - 2 U_l + U_{l+1}) ).
 * THIS TEXT IS THE DEFINITION.  The solve is free arithmetic (its result is defined by the linear system, like T0's): one
 * lane per (member, latitude) walks the longitudes, so every access is along the contiguous latitude axis; circles of 256
 * longitudes and more are cut into 4 ... 32 segments (a function of nlon only) with a reduced periodic system of their ends.
 * temp, out_U, out_Z: [ncol][nlat] host arrays (either output may be NULL); nlon >= 3 must divide ncol.  MIZ-family
 * handles.  Synchronous.
 * Why this is an operator and not a model: coupling it to the column step by operator splitting (Z of the previous step's
 * output temperature added to the diffusion term of both vertical fluxes) is stable on open water — there it converges
 * to the decay of the spherical harmonics P_l^m(x) cos(m lambda) at second order — but not over thin new ice, whose surface
 * temperature answers an enthalpy change ~60 times more strongly than water's does and without delay: zonal differences
 * then grow ~50-fold per step until the ice has thickened (measured with the checker's restatement,
 * tests/test_oracle_zonal.py).  A stable coupling has to put the zonal term inside the T0 balance of src/miz.jl:33-45 — a
 * two-dimensional elliptic solve per step — which this library does not contain. */
int ebm_zonal_diffusion(ebm_handle_t h, int nlon, const double *temp, double *out_U, double *out_Z);
/* Device pointer of a field and its row pitch in elements (>= nlat), for zero-copy users
 * (e.g. a torch tensor view).  The pointer stays valid until ebm_destroy.  For the MIZ fields (prognostic and
 * diagnostic, four cells per thread) the view shows the field as of this call: one-launch-per-step steps taken
 * afterwards keep the fields they read and write in a layout private to the library until the next access through
 * this interface (call again after such a step; do not write through the pointer while stepping).  Fails with
 * EBM_ERR_STALE like ebm_get_field.
 * The view of a prognostic MIZ field is writable, so the library takes the call as a possible write of the state: the
 * next step loads the phi field as it then is, instead of deriving it from Ei and h as the state-only one-launch-per-step
 * kernel otherwise does (the reference's step at four cells per thread), and a graph-replaying
 * ebm_run takes its first step directly.  Same results; a caller that takes views between steps only to read pays the
 * slower kernel for one step after each — ebm_get_field_device and ebm_hemispheric_mean_device read without that cost. */
int ebm_field_device_ptr(ebm_handle_t h, int field, double **dptr, long long *pitch);
/* Per-column forcing offset added to the per-step scalar forcing (forcing = f + fcol[col];
 * NULL clears it).  This is how ensemble members / longitudes get perturbed forcings — the
 * reference has a single scalar `f` per step (src/infrastructure.jl:631). */
int ebm_set_column_forcing(ebm_handle_t h, const double *fcol);
/* Per-column forcing SCHEDULES: column c is additionally forced by its own Forcing{false}
 * (src/infrastructure.jl:208-241), evaluated on the device at the model time T of every step as
 * the reference's call operator does (:294-307):
 *     T < d1: base;  T < d2: base + up*(T - d1);  T < d3: peak;  T < d4: peak + down*(T - d3);  else cool
 * sched[ncol][9] = {base, peak, cool, up, down, d1, d2, d3, d4} (d = Forcing.domain[2..5]); NULL
 * clears.  T of 0-based global step n is st.T[n+1] = (2n+1)/(2 nt): ebm_run takes n from
 * first_step, ebm_step and ebm_integrate use and advance the handle's step clock (0 after ebm_create, set by
 * ebm_set_step_clock, left at the step after the last one by every stepping call — so a run chunked into several
 * ebm_integrate calls of whole years sees the same model time as one call).  Needs the time table (its length is nt).  The three contributions add:
 * forcing = f + fcol[c] + schedule_c(T). */
int ebm_set_column_schedule(ebm_handle_t h, const double *sched);
int ebm_set_step_clock(ebm_handle_t h, long long step);
/* Per-column PARAMETER rows: params[ncol][EBM_P_COUNT] in enum ebm_param order; NULL returns every column to the
 * vector given to ebm_create.  Column c then steps exactly as a one-column handle created with row c and the same
 * model, grid, x, dt and options would: the same BITS, in every entry point — ebm_step, ebm_run, ebm_run_fused,
 * ebm_integrate, ebm_integrate_hemispheric, ebm_diffusion, the hemispheric means and the counters.  This is how a
 * parameter-sensitivity sweep (D, the albedo contrast, kappa, ...) runs as the members of ONE ensemble, together with
 * the per-column forcings above.  THIS TEXT IS THE DEFINITION.
 * Synchronous, like the forcing setters: the handle's stream is synchronised first.  The state, the warm-start pattern
 * and the validity of the fields (EBM_ERR_STALE) are left as they are; the new rows apply from the next step on.  A
 * change of Tm reaches the warm-start pattern [T0 < Tm] at the next T0 solve, as in the reference, whose T0 survives a
 * change of `par`.
 * A row is refused with EBM_ERR_ARG wherever ebm_create would refuse it as its vector (Tm < 0 with a non-integer m2
 * for the MIZ models); the message names the column, and the handle keeps the rows it had.  Entries a model does not
 * use are ignored, as in ebm_create.
 * Rows are deduplicated by bit pattern into parameter SETS: device memory is one parameter block and one set of
 * per-latitude tables per DISTINCT row (320 + 112 * pitch bytes per set, pitch = threads * cells_per_thread >= nlat;
 * at most ncol sets) plus 4 bytes per column for the column -> set index.
 * ebm_zonal_diffusion returns EBM_ERR_UNSUPPORTED while more than one distinct set is installed (its a_k tables come
 * from one D and one cw); with one set it uses that set's D and cw. */
int ebm_set_column_params(ebm_handle_t h, const double *params);
/* Per-column STOCHASTIC FORCING: AR(1) ("red") noise N_c added to every column's forcing, one independent realisation per
 * column, drawn on the device.  THIS TEXT IS THE DEFINITION.  For column c with stream id stream_c, the handle's seed and
 * the 0-based global index n of the step being taken:
 *   1. (w0,w1,w2,w3) = Philox4x32-10(counter = (lo32(n), hi32(n), lo32(stream_c), hi32(stream_c)),
 *                                   key = (lo32(seed), hi32(seed)))
 *      (Random123's Philox: multipliers 0xD2511F53, 0xCD9E8D57; key bumps 0x9E3779B9, 0xBB67AE85; ten rounds).
 *   2. a = (w0 << 21) | (w1 >> 11), b = (w2 << 21) | (w3 >> 11) (53-bit integers);
 *      u1 = (a + 1) * 2^-53 in (0, 1], u2 = b * 2^-53 in [0, 1).
 *   3. xi = sqrt(-2 log(u1)) * cospi(2 u2) (Box-Muller, first output; the device's own log and cospi).
 *   4. N_c <- rho_c * N_c + s_c * xi with s_c = sigma_c * sqrt(1 - rho_c^2), computed once on the host at set time; two
 *      rounded products and one sum (no contraction).  The step uses the updated N_c.
 *   5. The column's forcing is ((f + fcol[c]) + schedule_c(T)) + N_c (absent terms left out, in this order).
 * sigma_c is the stationary standard deviation of N_c in the units of f (W m^-2); rho_c in [0, 1) the lag-one-step
 * autocorrelation (0: white noise).  Because xi is keyed by (seed, stream_c, n), a column's noise does not depend on the
 * launch geometry, fused K, graph replay or launch chains, on how many columns share the handle or how an ensemble is
 * sharded (give every member its global index as stream id), nor on how a run is chunked into calls.  N_c is state: it
 * advances once per step taken, by every stepping entry point (ebm_step, ebm_run, ebm_run_fused, ebm_integrate,
 * ebm_integrate_hemispheric), for all models; ebm_get_noise_state / ebm_set_noise_state checkpoint it.
 * sigma, rho, stream: [ncol] each; sigma == NULL clears the noise (every kernel is then exactly the noise-free step);
 * stream == NULL means stream_c = c.  Every N_c is reset to 0.  EBM_ERR_ARG for a non-finite value, sigma < 0, rho outside
 * [0, 1) or a NULL rho with a non-NULL sigma; the handle then keeps what it had.  Synchronous, like the other column
 * setters.  ebm_equilibrate refuses with EBM_ERR_UNSUPPORTED while noise is installed (no repeating cycle).  Device memory:
 * 544 bytes per column (with 512 for the N_c sequence of a fused launch). */
int ebm_set_column_noise(ebm_handle_t h, const double *sigma, const double *rho, const unsigned long long *stream,
                         unsigned long long seed);
/* N[ncol]: the noise state N_c (all 0 without noise) / restore it (EBM_ERR_ARG without noise or for a non-finite value).
 * With the fields and the step clock this is a complete checkpoint: restored into a fresh handle with the same noise
 * settings, a run continues bit for bit.  Synchronous. */
int ebm_get_noise_state(ebm_handle_t h, double *N);
int ebm_set_noise_state(ebm_handle_t h, const double *N);
/* out[ncol][nsteps] = xi(seed, stream_c, first_step + i) of the installed noise, computed on the device by the function
 * the step kernels call (a test hook: the innovations bit for bit).  EBM_ERR_ARG without noise.  Synchronous. */
int ebm_noise_innovations(ebm_handle_t h, long long first_step, int nsteps, double *out);
/* Table of cos(2.0*pi*st.t[i]), i = 1..nt (src/miz.jl:11, src/classic.jl:24), needed by
 * ebm_run/ebm_integrate.  Computed by the caller so that host and device agree bit for bit. */
int ebm_set_time_table(ebm_handle_t h, int nt, const double *cos2pit);

/* ---- stepping ------------------------------------------------------------------------ */

/* One step!: cos2pit = cos(2.0*pi*t) for this step; cos2pit_next is column i+1 of the
 * classic model's S table (src/classic.jl:25,61; ignored for MIZ); f the scalar forcing.
 * write_diag != 0 also writes the diagnostic fields (Tw,Ti,n,E,T / T,h).  Asynchronous on
 * the handle's stream. */
int ebm_step(ebm_handle_t h, double cos2pit, double cos2pit_next, double f, int write_diag);

/* nsteps consecutive steps, one kernel launch per step (K = 1), starting at 0-based global
 * step index `first_step` (time-of-year index = first_step mod nt into the time table).
 * f_steps[nsteps] are the per-step scalar forcings (NULL = 0.0).  Diagnostics are written
 * on the last step only when diag_last != 0.  Asynchronous. */
int ebm_run(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps,
            int diag_last);

/* The same nsteps steps with `steps_per_launch` (K) consecutive steps fused into one kernel launch:
 * the time loop of integrate (src/infrastructure.jl:630-634) for callers that need no per-step
 * output.  Between the steps of a launch the whole state stays on the chip — in registers for
 * meridians of up to 2048 cells, in LDS for longer ones and for EBM_MODEL_MIZ_IMEX; the per-step
 * scalars come from a device table.  Results are bit-identical to ebm_run for every model and size
 * (ebm_get_counters reports the launches actually made: ceil(nsteps / K), twice that with two launch
 * chains).  Asynchronous. */
int ebm_run_fused(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps,
                  int diag_last, int steps_per_launch);

/* The same nsteps steps with a TIME SERIES of per-column hemispheric means sampled on the device every `every` steps: a
 * member's <T>(t) or ice area <phi>(t) at weather resolution — crossing times, residence times, the autocorrelation before
 * a transition — where ebm_integrate_hemispheric gives three numbers per year.  THIS TEXT IS THE DEFINITION.
 *   Stepping.  The call takes nsteps steps exactly as ebm_run_fused(h, first_step, nsteps, f_steps, diag, steps_per_launch)
 *     does, with diag = 1 iff one of fields[] is a diagnostic field of the model (see "Validity"): time table, per-column
 *     forcings, schedules, parameter rows, noise and launch options as there.
 *   Samples.  nsamples = nsteps / every; sample j (0-based) is taken after 0-based global step first_step + (j+1)*every - 1.
 *   Output.  series[nvars][nsamples][ncol] on the host: series[v][j][c] is bit for bit what ebm_hemispheric_mean(h,
 *     fields[v], out) puts into out[c] after ebm_run_fused(h, first_step, (j+1)*every, f_steps, diag, steps_per_launch) from
 *     the same start — hemispheric_mean (src/utilities.jl:397-403) in the reference's summation order; a NaN sentinel in
 *     Ti or Tw gives a NaN mean, as it does there.
 *   State after the call.  Bit for bit that of the one ebm_run_fused of nsteps steps: prognostic fields and warm start, the
 *     diagnostic fields if diag, the noise state, counters[0] and the validity bookkeeping (ebm_field_step).
 *   Launches.  A launch never spans a sample: counters[3] grows by nsamples * ceil(every / K') step launches, K' =
 *     min(steps_per_launch, 64 if noise is installed), twice that with two launch chains.  The reduction launches (one
 *     small kernel per sample: one wave per column sums all nvars fields side by side) are not counted.
 * fields[nvars]: solution variables of the model, prognostic or diagnostic, each at most once; EBM_F_T0 is not one (as in
 * ebm_integrate).  Refusals leave the handle as it was: EBM_ERR_ARG for every < 1, nsteps not a multiple of every, nvars < 1
 * or more than 12, a bad or repeated field, a missing time table, a NULL series or fields.  Device memory for the call:
 * nvars * nsamples * ncol doubles, allocated before the first step (a failure is EBM_ERR_HIP with no step taken) and freed
 * before it returns.  Nothing is synchronised between samples; the whole series comes down once at the end, through the
 * handle's pinned ring.  Synchronous.  Thresholds and first-passage times are host arithmetic on the returned series. */
int ebm_run_series(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int every, int steps_per_launch,
                   int nvars, const int *fields, double *series);

/* integrate + savesol! (src/infrastructure.jl:549-591, 615-636) with state resident on the
 * device: runs nt*dur steps from the current state.  `fields[nvars]` selects the saved
 * variables; outputs are host buffers (any may be NULL to skip):
 *   raw    [nvars][nraw][ncol][nlat]   nraw = lastonly ? nt : nt*dur
 *   winter, summer, avg  [nvars][dur][ncol][nlat]
 * winter_inx/summer_inx are the 1-based in-year indices st.winter.inx / st.summer.inx.
 * f_steps[nt*dur] as in ebm_run.  `fields` must be solution variables (not the hidden EBM_F_T0),
 * each at most once.  savesol! runs inside the step kernel: the annual-mean sums and the raw snapshot are taken
 * from the step's registers — one launch per step on the steps whose snapshot leaves the device (raw, winter,
 * summer, a year's last step), ebm_options.integrate_steps_per_launch steps per launch in between, with the
 * same bits.  The annual mean is sum / nt with the sum
 * taken per cell sequentially in step order; the reference's crossmean (src/utilities.jl:390-395) is
 * Statistics.mean over the year's snapshots, i.e. Julia's pairwise, SIMD-reassociated sum — the two agree up to
 * summation-order rounding (the parity tests hold avg to 1e-8 of the oracle's), not bit for bit.
 * The time-of-year index starts at 1 (the call begins a year); model time (per-column schedules) continues from
 * the handle's step clock.  Host output overlaps the stepping (device-to-device snapshot, then DMA through the
 * handle's pinned ring on a stream of its own).  Synchronous: returns when all outputs are in the caller's arrays. */
int ebm_integrate(ebm_handle_t h, int nt, int dur, const double *f_steps, int lastonly,
                  int winter_inx, int summer_inx, int nvars, const int *fields, double *raw,
                  double *winter, double *summer, double *avg);

/* The same integration when only the HEMISPHERIC MEANS of the seasonal outputs are wanted — the numbers
 * behind the reference's hysteresis plot (plot_seasonal, src/plot.jl:173-225: hemispheric_mean of
 * seasonal.avg.T[year] and of seasonal.{avg,winter,summer}.phi[year]): per saved variable, year and column,
 * hemispheric_mean (src/utilities.jl:397-403, the reference's summation order) of the winter snapshot, the
 * summer snapshot and the annual mean, reduced on the device.  Outputs are [nvars][dur][ncol] host arrays
 * (any may be NULL): O(columns x years) bytes cross the bus instead of O(state x years) — ensembles.
 * Bit-identical to applying hemispheric_mean to ebm_integrate's winter / summer / avg outputs. */
int ebm_integrate_hemispheric(ebm_handle_t h, int nt, int dur, const double *f_steps, int winter_inx,
                              int summer_inx, int nvars, const int *fields, double *hm_winter,
                              double *hm_summer, double *hm_avg);

/* Run whole years until each column's seasonal cycle repeats — the spin-up behind every steady state of the reference
 * (integrate(...; lastonly=true) run for "enough" years, src/infrastructure.jl:615-636), with a stated criterion and a
 * stopping year of its own for every column.  THIS TEXT IS THE DEFINITION.
 *   Year-end snapshot.  S_c,v(y) is field fields[v] of column c after y whole years of this call.  Every year is nt steps
 *     with time-of-year index 1 .. nt (as ebm_integrate) and the forcing f_year[i] + fcol[c], the same every year
 *     (f_year[nt]; NULL = 0).
 *   Distance.  d_c,v(y) = max over k < nlat of |S_c,v(y)[k] - S_c,v(y-1)[k]|, taken for y >= 2 only.
 *   Equilibrium year.  Y_c is the smallest y with max(2, min_years) <= y <= max_years such that d_c,v(y) <= tol[v] for
 *     every v.  A NaN anywhere (in a distance, hence in either snapshot) means "not converged" — so Ti and Tw, which hold
 *     NaN sentinels where there is no ice / no open water (src/miz.jl:193-194), never converge in a column that has one.
 *   Freezing.  Column c steps exactly Y_c years and then no further step.  Its whole state is bit for bit what
 *     ebm_run_fused (equivalently ebm_run, ebm_integrate) gives after Y_c * nt steps from the same start: the prognostic
 *     fields, the warm start T0 and the diagnostic fields, written at the column's own last year end.
 *   Outputs.  years[c] = Y_c and converged[c] = 1; a column that never meets the criterion steps max_years years and gets
 *     years[c] = max_years, converged[c] = 0.  resid[v][c] (may be NULL) is d_c,v of the last year compared for the
 *     column, NaN if none was (max_years = 1).  Host arrays: years, converged [ncol]; resid [nvars][ncol].
 *   The call returns as soon as every column is frozen.  Afterwards the step clock is at clock0 + nt * max_c years[c]
 *   (clock0: the clock at entry), counters[0] has counted nt * max_c years[c] steps, and every field is current: each
 *   column holds the values of its own last step, and the validity bookkeeping (ebm_field_step) records them as written
 *   by the handle's last step.
 * fields[nvars] may name any solution variable of the model, prognostic or diagnostic, each at most once; EBM_F_T0 is not
 * one (as in ebm_integrate).  All models (MIZ, MIZ_IMEX, classic), grids and options; per-column forcings and parameter
 * rows are honoured.  Columns are independent: a column's result does not depend on the others or on sharding.
 * Refusals leave the handle as it was: EBM_ERR_UNSUPPORTED while per-column schedules or forcing noise are installed (a
 * ramped or noisy forcing has no equilibrium); EBM_ERR_ARG for a time table whose length is not nt, max_years < 1, a tolerance that is negative or
 * NaN, a bad or repeated field.
 * How it runs: each year is the fused stepping of ebm_run_fused (ebm_options.integrate_steps_per_launch steps to a launch,
 * 1 = one launch per step) over the ACTIVE columns only — a frozen column gets no workgroup and moves no byte — then one
 * small kernel compares and snapshots the active columns' fields, a second one builds the next active list, and the host
 * reads its length (one stream synchronisation per year).  Device memory for the call: nvars * ncol * pitch doubles (last
 * year's snapshot), nvars * ncol doubles (resid) and 4 ints per column, freed before it returns.  Synchronous. */
int ebm_equilibrate(ebm_handle_t h, int nt, int max_years, int min_years, const double *f_year, int nvars, const int *fields,
                    const double *tol, int *years, int *converged, double *resid);

/* FIRST PASSAGE: step every column until the hemispheric mean of one field crosses the column's level — the tipping step of
 * a noisy member, the runaway under a forcing ramp, the loss of the summer ice — and keep the column's state at its
 * crossing.  Where ebm_run_series steps every member over the whole horizon and leaves the thresholding to the host, a member
 * that has crossed takes no further step here.  THIS TEXT IS THE DEFINITION.
 *   Rounds.  Round j = 1, 2, ... takes `every` steps, the 0-based global steps first_step + (j-1)*every .. first_step +
 *     j*every - 1, of the columns still active (all of them in round 1).  A column's stepping over its rounds 1 .. j is
 *     exactly that of ebm_run_fused(h, first_step, j*every, f_steps, diag, steps_per_launch), with diag = 1 iff `field` is a
 *     diagnostic field of the model: time table, per-column forcings, schedules, parameter rows, noise and launch options
 *     as there.  f_steps[max_samples * every] (NULL = 0.0).
 *   Sample.  After round j, m_c is bit for bit what ebm_hemispheric_mean(h, field, out) would put into out[c] at that point
 *     (hemispheric_mean, src/utilities.jl:397-403, in the reference's summation order), for every column c active in round j.
 *   Crossing.  Column c has crossed when direction[c] > 0 ? m_c >= level[c] : m_c <= level[c].  Equality crosses.  A NaN m_c
 *     never crosses (the NaN sentinels of Ti and Tw, src/miz.jl:193-194).  level[c] = +-inf is legal: "never", or "at the
 *     first sample", depending on the direction.
 *   Freezing.  A column that crosses at round j takes no further step: its whole state is bit for bit that of a run of
 *     j*every steps from the same start — the prognostic fields, the warm start, the noise state N_c and, if diag, the
 *     diagnostic fields and the fp64 T0, written at the column's own last step.  A column that never crosses takes
 *     max_samples*every steps.
 *   Outputs ([ncol] host arrays).  samples[c]: the rounds column c took; crossed[c]: 1 if it crossed (at round samples[c]),
 *     else 0 (samples[c] = max_samples); value[c] (may be NULL): its last m_c.  The first-passage step of a column that
 *     crossed is the 0-based global step first_step + samples[c]*every - 1.
 *   Afterwards.  The call returns as soon as no column is active.  With R = max_c samples[c], the step clock is at
 *     first_step + R*every and counters[0] has grown by R*every; counters[3] by ceil(every / K') launches per round and
 *     non-empty launch chain, K' = min(steps_per_launch, 64 if noise is installed) (the two small kernels per round are not
 *     counted).  Field validity is recorded as for ebm_equilibrate: each column holds the values of its own last step, and
 *     the bookkeeping (ebm_field_step) records them as written by the handle's last step.  Further stepping of such a handle
 *     — by any entry point, this one included — continues every member, the frozen ones too, from its own state, under the
 *     handle's one step clock: a second call tests every column anew, so a column whose mean still satisfies its comparison
 *     stops again after one round.
 * Columns are independent: a column's result does not depend on the others or on sharding.  All models, grids and options.
 * Refusals leave the handle as it was: EBM_ERR_ARG for every < 1, max_samples < 1, steps_per_launch < 1, first_step < 0, a
 * field that is not a solution variable of the model (EBM_F_T0 is not one), a NaN level, direction[c] == 0, a missing time
 * table, a NULL level, direction, samples or crossed; EBM_ERR_UNSUPPORTED where the shape has no fused-K kernel in this
 * build (as ebm_equilibrate).
 * How it runs: every round is the fused stepping of ebm_run_fused over the ACTIVE columns only — a frozen column gets no
 * workgroup and moves no byte; also with steps_per_launch = 1, which here is the fused kernel at one step per launch (same
 * bits), never ebm_run's one-step kernels or its graph replay, which know nothing of the list — then one small kernel takes
 * the mean of each active column (one wave per column) and compares, a second one builds the next active list, and the
 * host reads its length: ONE STREAM SYNCHRONISATION PER ROUND (none after the last possible one).  `every` is the caller's
 * knob for that cost: a crossing is only seen at a multiple of `every` steps.  Device memory for the call: 5 ints and 2
 * doubles per column (two lists, samples, crossed and direction; value and level), freed before it returns.  Synchronous. */
int ebm_run_until(ebm_handle_t h, long long first_step, int max_samples, int every, const double *f_steps, int steps_per_launch,
                  int field, const double *level, const int *direction, int *samples, int *crossed, double *value);

/* RESAMPLE the members on the device: column c continues from a copy of column parent[c]'s state and draws its own noise
 * from then on — the selection step of genealogical cloning (Giardina-Kurchan-Lecomte-Tailleur), of adaptive multilevel
 * splitting, of any particle filter — without the state leaving the device.  THIS TEXT IS THE DEFINITION.
 *   Gather, all at once.  parent[ncol] is a host array.  For every column c simultaneously, the new state of c is the old
 *     state of parent[c]: reads happen before writes.  A swap (parent = {1, 0}) exchanges two columns, a shift (parent[c] =
 *     c - 1) moves every column by one, a fan-out gives many columns one parent.  parent[c] == c leaves c untouched and
 *     moves no byte of it; the all-identity map launches nothing.
 *   What moves: the state — everything a checkpoint of the column consists of.  The prognostic fields (MIZ and MIZ_IMEX:
 *     Ei, Ew, h, D, phi; classic: E, Tg), the warm-start active set, the noise state N_c if noise is installed, and every
 *     diagnostic field, and the fp64 T0, that is current at the call.  Stale diagnostic fields are not copied and stay stale.
 *   What stays: the member's identity — everything installed per column stays with the slot: fcol[c], the schedule row,
 *     the parameter set, the noise record (sigma, rho, stream id).  From the next step on, column c steps exactly as a
 *     one-column handle created with c's settings and loaded with parent[c]'s state, T0, noise state and the same step
 *     clock would, bit for bit, in every stepping entry point.  Two clones of one parent keep their own streams, so they
 *     part at the next step; without noise they stay identical.
 *   Validity.  The call changes the prognostic state without a step, yet keeps the fields consistent: a field that was
 *     current before is current after and holds the parent's values; a field that was stale fails with EBM_ERR_STALE
 *     exactly as before, with the same steps in the message.  written_step and state_step (ebm_field_step) are unchanged,
 *     and ebm_get_field_as_of keeps answering for the step it answered for.  The step clock and counters[0..3] are
 *     unchanged: the copy kernels are not counted as launches.
 *   Layout.  Rows are copied whole — pitch doubles, padding included — in whatever layout the handle holds them (the
 *     layout private to the one-step MIZ kernel permutes WITHIN a row), so nothing is converted: ebm_state_conversions
 *     does not grow, and a steady ebm_run loop with a resample between its calls still converts once.
 *   Ordering.  The work is enqueued on the handle's stream, after every step launched so far (two launch chains are
 *     joined first).  parent has been consumed when the call returns.  Asynchronous, like ebm_run; a call waits only for
 *     the list upload of the call before it.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL parent or an entry outside [0, ncol); the message names the
 * first offending column.
 * How it runs: the host builds the list of moved columns (destination, parent) and uploads it; every array that moves is
 * then taken through two passes — the parents' rows into a staging buffer, the staging buffer into the destinations — so
 * that no swap, cycle or chain reads a row already overwritten; one workgroup per moved column, 16 bytes per lane and
 * access on whole 128-byte lines.  Device memory for the call, with moved = the number of columns with parent[c] != c:
 * moved * pitch doubles of staging (one field's worth at most — never a second copy of the state; the scratch of
 * ebm_diffusion is used instead where the handle has it) and the list, 2 ints per moved column; kept by the handle. */
int ebm_resample_columns(ebm_handle_t h, const int *parent);

/* EXPORT and IMPORT whole columns on the device: the state of a list of columns into one contiguous device buffer of
 * records and back — between two handles without the host, and as the payload of an all-to-all (RCCL) between the shards
 * of an ensemble, which makes the selection above possible across ranks.  THIS TEXT IS THE DEFINITION.
 *   The record.  One exported column is R doubles (ebm_column_record), a function of the model, nlat and cells_per_thread
 *     only — not of which fields are current, of the layout the handle holds, or of whether noise is installed.  With
 *     rowlen = nlat rounded up to a multiple of 16 doubles (whole 128-byte lines; rowlen <= pitch always), in this order:
 *       one slot of rowlen doubles per field the model has, in enum ebm_field order (MIZ and MIZ_IMEX: 11 slots, Ei ... T
 *         with T0 among them; classic: h, E, T, Tg);
 *       the warm-start active-set row as it lies in memory: `threads` unsigned shorts = threads/4 doubles (classic: none,
 *         zero length);
 *       a 16-byte tail: N_c (0.0 when no noise is installed), then one reserved double written as 0.0.
 *     Field slots are in the NATURAL layout: cell k of the column is double k of its slot, whatever layout the handle
 *     holds the row in (the layout private to the one-step MIZ kernel is un-permuted on the way out and permuted on the
 *     way in).  Cells between nlat and rowlen travel as the row holds them; no stepping entry point reads them.  The record
 *     is a transport format between handles of the same model, nlat and cells_per_thread.  It is not a file format.
 *   mask.  Bit f (enum ebm_field) is set when the slot of field f holds field f.  Export always sets the prognostic bits,
 *     and the bit of a diagnostic field, and of the fp64 T0, exactly when that field is current at the call — the rule by
 *     which ebm_resample_columns decides what moves.  Slots of fields that are not current are not written.  The mask
 *     travels on the host: an out-parameter of export, an argument of import.  Nothing in the device buffer is validated,
 *     so neither call synchronises to check it.  ebm_column_record returns R and the mask an export would return now.
 *   Export.  Record i of dev_buf (n * R doubles) is the state of column cols[i]; cols may repeat.  phi is made current
 *     first, as resampling does.  Nothing in the handle changes: no conversion, no validity change, no counter.
 *   Import.  Column cols[i] takes record records[i] of dev_buf; records == NULL means records[i] = i.  One record may seed
 *     many columns (the clones of one parent: the payload holds the distinct parents only).  cols must be distinct.  Written,
 *     all in the layout the handle holds at the call, ebm_state_conversions unchanged: the prognostic fields; the active-set
 *     row; N_c if noise is installed on the destination; every diagnostic field, and T0, that is current in the destination
 *     and present in mask.  A slot whose field is stale in the destination is ignored: the field stays stale, with the same
 *     steps in its message.  A field that is current in the destination but absent from mask refuses the call with
 *     EBM_ERR_STALE and nothing is written (the column would hold another member's prognostics under its own old
 *     diagnostics, flagged current).  Like resampling, import writes Ei, h and phi without a step: the next launch loads
 *     phi, which is not derived under the destination's parameters.  What stays with the slot: fcol, the schedule row, the
 *     parameter set, the noise record.  The step clock, counters[0..3] and ebm_field_step are unchanged.  From the next step
 *     on the column steps as a one-column handle with its settings, loaded with the source's state, T0, noise state and
 *     clock, would: bit for bit, in every stepping entry point.
 *   Ordering.  Both calls are asynchronous on the handle's stream, the two launch chains joined first.  An export followed
 *     by an import on the same handle through one buffer is ordered by the stream: for cols = the moved columns c and the
 *     records of parent[c] the pair IS ebm_resample_columns(parent), all reads before all writes.  Across handles or streams
 *     the caller orders the work: ebm_sync of the exporter before anyone else reads the buffer; the buffer complete before
 *     import is called; the buffer untouched until the importer's ebm_sync.  cols and records have been consumed when the
 *     call returns.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle, n < 0, NULL cols or dev_buf with n > 0, a dev_buf
 * that is not 16-byte aligned, a column outside [0, ncol), a repeated destination, a record index < 0, a mask without every
 * prognostic bit or with a bit of a field the model lacks — the message names the first offending entry; EBM_ERR_STALE as
 * above.  n == 0 launches nothing.
 * How it runs: ONE launch per call over (entries x slots), one workgroup of 256 lanes per row, the row pointers of all slots
 * in one argument struct; 16 bytes per lane and access in both layouts (the unit of the permutation is the pair of cells:
 * natural unit u lies at split unit (u & 1) * threads + (u >> 1)); plain loads and stores.  Device memory: the list, kept by
 * the handle.  The buffer is the caller's. */
int ebm_column_record(ebm_handle_t h, long long *record_doubles, unsigned *current_mask);
int ebm_export_columns(ebm_handle_t h, int n, const int *cols, double *dev_buf, unsigned *mask);
int ebm_import_columns(ebm_handle_t h, int n, const int *cols, const int *records, const double *dev_buf, unsigned mask);

/* WEIGHTED SUMS ACROSS THE MEMBERS, per latitude: the column-wise partner of ebm_hemispheric_mean — the ensemble mean T(x)
 * and its spread, the mean ice profile of the members that tipped, a mean under importance weights — reduced on the device,
 * so that O(nlat) doubles cross the bus, or enter an all-reduce between shards, instead of O(state).  THIS TEXT IS THE
 * DEFINITION.
 *   Arguments.  fields[nvars]: solution variables of the model, prognostic or diagnostic, each at most once; EBM_F_T0 is not
 *     one; 1 <= nvars <= 12 (the rules of ebm_run_series).  w[ncol]: host array of member weights, NULL = every w_c = 1.0.
 *     center[nvars][nlat]: host array in natural latitude order, NULL = nothing is subtracted.  out[nvars][3][nlat]: S0, S1
 *     and S2 in natural latitude order, on the host; the _device variant writes the same packed array into the caller's
 *     device buffer dev_out (the payload of an all-reduce).
 *   Terms.  For variable v, latitude k < nlat and column c, with x the value of field fields[v] of column c at k: the column
 *     CONTRIBUTES at k iff w_c != 0.0 and x is not NaN.  The NaN sentinels of Ti and Tw (src/miz.jl:193-194) mean "no ice / no
 *     water here"; a zero weight removes the member altogether, which is how a conditional mean over a sub-ensemble is taken
 *     (its cells may hold anything, Inf included); +-Inf in a contributing cell is data and propagates.  d = x - center[v][k],
 *     or d = x when center is NULL.  The three terms are t0 = w_c, t1 = w_c * d and t2 = (w_c * d) * d: every product and every
 *     sum is rounded once, nothing is contracted into a fused multiply-add.
 *   Order.  Block b holds the columns 32 b ... min(32 b + 31, ncol - 1).  The block partial of each of S0, S1, S2 starts at
 *     0.0 and adds the terms of the contributing columns of the block in ascending column order.  The result starts at 0.0
 *     and adds the block partials in ascending b; a block without a contributor adds its 0.0.  The order is part of the
 *     definition: the same call gives the same bits on every run, under either launch geometry (cells_per_thread) and in
 *     either stored layout, and no floating-point atomic is involved.  A latitude without a contributor gives S0 = S1 = S2 =
 *     0.0.  Mean and variance are the caller's arithmetic: with center NULL, mean = S1 / S0; with center = that mean,
 *     var = S2 / S0 - (S1 / S0)^2, whose second term is then of rounding size.
 *   Across shards.  Each shard's sums are defined to the bit.  Adding the sums of n shards adds the same terms in another
 *     order than the unsharded call does, so the two are not equal bit for bit.  A term of a call over m columns passes
 *     through at most D(m) = min(m, 32) + ceil(m / 32) - 2 rounded adds (inside its block, then over the blocks; an add to
 *     0.0 is exact), and the combination of n shards adds n - 1 more: per latitude the two agree to within
 *     (D(ncol) + max_r D(ncol_r) + n - 1) * 2^-53 * (sum of |terms|), to first order in 2^-53, ncol_r the columns of shard r.
 *   Validity.  A diagnostic field that is older than the state fails with EBM_ERR_STALE exactly as ebm_hemispheric_mean does
 *     (the same message).  If phi is among the fields and state-only one-step launches have left it underived, it is made
 *     current first, as ebm_export_columns does.
 *   Layout.  The reduction is elementwise along latitude, so rows are read in whatever layout the handle holds them (the
 *     layout private to the one-step MIZ kernel at four cells per thread, the natural one otherwise); only the indexing of
 *     center and of the output is un-permuted.  No field is converted: ebm_state_conversions does not grow, and a steady ebm_run
 *     loop with this call between its calls still converts once.  Cells between nlat and the row pitch are never read into
 *     a result (for odd nlat the last 16-byte pair is loaded with its padding cell, whose sums are never used).
 *   Bookkeeping.  The step clock, counters[0..3] and ebm_field_step are unchanged; the two reduction launches are not
 *     counted.  Both calls are synchronous on the handle's stream, the two launch chains joined first.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle, fields or out, nvars outside 1 ... 12, a field that is
 * not a solution variable of the model or is listed twice, a non-finite w[c] (the message names the column), a non-finite
 * center entry; EBM_ERR_STALE as above.  Negative weights are legal (differences of estimators).
 * How it runs: one kernel forms the block partials — grid (latitude tiles) x (column blocks) x (variables); a lane owns one
 * 16-byte pair of cells, the unit of the layout permutation, and walks the 32 columns of its block with the loads issued
 * ahead of the dependent adds, a wave reading whole 128-byte lines; w_c is read once per column through the scalar cache —
 * and a second one adds the block partials per latitude in ascending order and writes the natural index.  Plain loads and
 * stores, no LDS, no scratch.  Device memory, kept by the handle and reused: ceil(ncol / 32) * 3 * nvars * pitch doubles of
 * block partials, the uploaded weights (ncol doubles) and centers (12 * pitch doubles), and 36 * nlat doubles for the host
 * variant's result. */
int ebm_ensemble_sums(ebm_handle_t h, int nvars, const int *fields, const double *w, const double *center, double *out);
int ebm_ensemble_sums_device(ebm_handle_t h, int nvars, const int *fields, const double *w, const double *center,
                             double *dev_out);

/* Order statistics ACROSS the columns of a handle, per latitude: the number, minimum and maximum of the members' values
 * (ebm_ensemble_range) and a weighted histogram of them between per-latitude edges (ebm_ensemble_histogram), reduced on the
 * device.  Where the members of an ensemble sit on two branches (noise-induced transitions, hysteresis, cloning) the mean
 * describes no member; median, bands and the distribution itself come from these two calls (EnsembleRun.quantiles brackets
 * with them), and O((nbins + 2) * nlat) doubles cross the bus, or enter an all-reduce between shards, instead of O(state).
 * THIS TEXT IS THE DEFINITION.
 *   Arguments.  fields[nvars], w[ncol], the contribution rule, validity, layout, bookkeeping and ordering are those of
 *     ebm_ensemble_sums (one piece of code checks them for all three): solution variables only, EBM_F_T0 is not one,
 *     1 <= nvars <= 12; w NULL = every w_c = 1.0, finite, negative weights legal; column c CONTRIBUTES at (v, k) iff
 *     w_c != 0.0 and the cell is not NaN; a stale diagnostic field is EBM_ERR_STALE with the message of ebm_hemispheric_mean;
 *     phi is made current first; no field is converted and ebm_state_conversions does not grow; rows are read in whatever
 *     layout the handle holds and only the indexing of lo, hi and the output is un-permuted; padding cells never reach a
 *     result; the step clock, counters[0..3] and ebm_field_step are unchanged; the calls are synchronous on the handle's
 *     stream, the two launch chains joined first.  In ebm_ensemble_range each field may appear at most once.  In
 *     ebm_ensemble_histogram a field MAY be listed several times: every entry v has its own rows lo[v], hi[v], so several
 *     quantiles of one field refine in one call.
 *   Range.  out[nvars][3][nlat]: out[v][0][k] = the number of contributing columns (a double), out[v][1][k] their minimum,
 *     out[v][2][k] their maximum.  A weight acts only through being zero or not.  +-Inf is data.  No contributor: n = 0,
 *     min = +Inf, max = -Inf.  The minimum starts at +Inf and the columns are walked in ascending order, a contributing x
 *     replacing it iff x < min (strictly), within a block of columns and then over the blocks in ascending order; the
 *     maximum likewise from -Inf with x > max.  Where several contributors compare equal to the extreme (+0.0 and -0.0) the
 *     result therefore carries the bits of the first of them in ascending column order, and does not depend on how the
 *     columns are blocked.
 *   Histogram.  1 <= nbins <= 64.  lo[nvars][nlat], hi[nvars][nlat]: host arrays in natural latitude order, every entry finite
 *     with lo < hi, and hi - lo and s = (double)nbins / (hi - lo) finite; s is that one IEEE division, taken on the host.
 *     out[nvars][nbins + 2][nlat].  A contributing value x at (v, k) goes to ONE slot: slot 0 ("below") if x < lo; slot
 *     nbins + 1 ("above") if x >= hi; otherwise slot 1 + min((int)t, nbins - 1) with t = (x - lo) * s, a rounded difference
 *     times a rounded product, nothing contracted.  The clamp is needed: with lo = -1, hi = 2 and x = nextafter(2, -Inf),
 *     t == nbins exactly for nbins = 1, 2, 3, 5, 7, 32, 63, 64.  -Inf goes below and +Inf above; -0.0 with lo = 0.0 goes to
 *     bin 0 (slot 1).  A slot's value is the sum of w_c over its contributors in a fixed order: block b holds the columns
 *     256 b ... min(256 b + 255, ncol - 1); a block partial starts at 0.0 and adds in ascending column order; the result
 *     starts at 0.0 and adds the block partials in ascending b.  (256, not the sums' 32: the partials are nbins + 2 times
 *     larger than the sums'.)  With w = NULL every slot is an exact integer whatever the order, so unit-weight histograms of
 *     shards add to the unsharded one bit for bit, and the ranges of shards combine exactly with SUM, MIN and MAX.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle, fields, out, lo or hi, nvars outside 1 ... 12, a field
 * that is not a solution variable of the model (or, in the range, is listed twice), a non-finite w[c] (the message names the
 * column), nbins outside 1 ... 64, an edge pair that breaks the rule above (the message names the first offending entry and
 * latitude); EBM_ERR_STALE as above.
 * How it runs (csrc/ebm_ensemble.hip): the walk of ebm_ensemble_sums — grid (latitude tiles) x (column blocks) x (entries), a
 * lane owning one 16-byte pair of cells, whole 128-byte lines, the loads of 16 columns issued ahead of the dependent work,
 * w_c through the scalar cache — with n, min, max in registers for the range, and for the histogram the slots in LDS as
 * [slot][cell of the pair][lane], (nbins + 2) KiB per one-wave workgroup, each lane touching only its own two columns of it:
 * no atomics, no bank conflicts, no scratch.  A second kernel combines the block partials per latitude in ascending order
 * and writes the natural index.  Device memory, kept by the handle and reused: ceil(ncol / 256) * (nbins + 2) * nvars * pitch
 * doubles of block partials (range: ceil(ncol / 32) * 3 * nvars * pitch), 36 * pitch doubles of edges, and 12 * 66 * nlat
 * doubles for the host variants' result. */
int ebm_ensemble_range(ebm_handle_t h, int nvars, const int *fields, const double *w, double *out);
int ebm_ensemble_range_device(ebm_handle_t h, int nvars, const int *fields, const double *w, double *dev_out);
int ebm_ensemble_histogram(ebm_handle_t h, int nvars, const int *fields, const double *w, int nbins, const double *lo,
                           const double *hi, double *out);
int ebm_ensemble_histogram_device(ebm_handle_t h, int nvars, const int *fields, const double *w, int nbins, const double *lo,
                                  const double *hi, double *dev_out);

/* COVARIANCE ACROSS THE MEMBERS, per PAIR of latitudes: how field_a at latitude i co-varies with field_b at latitude j over
 * the columns of the handle — the matrix whose eigenvectors are the EOFs of an ensemble that sits on two branches, whose rows
 * are the correlation of the ice edge with the tropics, and which an ensemble Kalman update takes for its background
 * covariance — reduced on the device, so that nlat^2 doubles cross the bus, or enter an all-reduce between shards, instead of
 * O(state).  The one dense contraction of the library: it runs on the fp64 matrix instruction of gfx950.  (The covariance of
 * every latitude with a few SCALARS is ebm_ensemble_sums with the scalars' deviations for member weights.)  THIS TEXT IS THE
 * DEFINITION.
 *   Arguments.  field_a, field_b: solution variables of the model under the rules of ebm_ensemble_sums (one piece of code
 *     checks them for both), prognostic or diagnostic; EBM_F_T0 is not one; the two may be equal.  w[ncol]: host array of
 *     member weights, NULL = every w_c = 1.0; finite; negative weights are legal.  center_a[nlat], center_b[nlat]: host
 *     arrays in natural latitude order, finite, NULL = nothing is subtracted.  out[nlat][nlat], on the host: row i belongs to
 *     field_a at latitude i, column j to field_b at latitude j, both in natural latitude order; the _device variant writes
 *     the same packed array into the caller's device buffer dev_out.
 *   Terms.  For column c, with x the cell of field_a at latitude i and y the cell of field_b at latitude j:
 *     da = x - center_a[i] (da = x when center_a is NULL), a = w_c * da and b = y - center_b[j] (b = y when center_b is
 *     NULL) — two rounded differences and one rounded product.  a is replaced by +0.0 when w_c == 0.0 or x is NaN; b is
 *     replaced by +0.0 when w_c == 0.0 or y is NaN.  So a zero weight removes the member (its cells may hold anything, Inf
 *     included), and a NaN sentinel of Ti or Tw (src/miz.jl:193-194) contributes nothing to any pair it is in.
 *     out[i][j] = the sum over c of a * b.  +-Inf in a contributing cell is data and follows IEEE — in particular Inf * 0 is
 *     NaN: an infinite cell of a member at i makes out[i][j] NaN wherever that member's b is zero, a cleaned NaN sentinel
 *     included.  The number of contributors per latitude is S0 of ebm_ensemble_sums; this call returns none.
 *   Order.  The products and adds of a group of four members are ONE v_mfma_f64_16x16x4_f64 and their bits are the
 *     hardware's, so this text does not restate them operation by operation; it fixes everything around them:
 *     1. Block B holds the columns 512 B ... min(512 B + 511, ncol - 1) (kCovBlock = 512).
 *     2. The partial of a block starts at +0.0 and takes the block's members in ascending groups of four, one matrix
 *        instruction per group: partial <- mfma(a[0..3], b[0..3], partial).  A tail group of fewer than four is padded
 *        with terms a = b = +0.0.
 *     3. out[i][j] = partial_0 + partial_1 + ..., the block partials in ascending B with plain rounded adds.  With one block
 *        the result is that block's partial.  No atomic is involved.
 *     4. The same call on the same data gives the same bits on every run.
 *     5. The bits depend neither on the launch geometry (cells_per_thread) nor on the layout the handle holds the rows in:
 *        every out[i][j] sees the same chain over the members, whichever tile of the kernel it falls in.
 *     6. When field_a == field_b and the two centers are both NULL or equal bit for bit, out[i][j] is defined for j >= i
 *        only, and out[j][i] is a copy of out[i][j] — inside the tiles on the diagonal too.  The result is symmetric to
 *        the bit.  (Otherwise out[i][j] and out[j][i] differ in which factor carries w_c.)  The work that is skipped is
 *        decided per 32 x 32 block of stored cells, see "How it runs": towards half of it as nlat grows.
 *   Accuracy.  With n the number of members with w_c != 0, nblocks = ceil(ncol / 512) and T_ij = the sum over c of |a * b|:
 *     |out[i][j] - the exact sum of the stated terms| <= (n + nblocks) * 2^-53 * T_ij * (1 + 2^-4), for any order of correctly
 *     rounded multiplies, adds or fused multiply-adds inside the instruction; the last factor covers the second-order terms
 *     (and the 64-bit-mantissa reference of the tests).
 *   Across shards.  Each shard's matrix is defined as above.  Adding the matrices of several shards adds the same terms in
 *     another order than the unsharded call does: the two agree within the sum of their bounds, not bit for bit.
 *   Validity, layout, bookkeeping, ordering: those of ebm_ensemble_sums, through the same code.  A diagnostic field that is
 *     older than the state fails with EBM_ERR_STALE exactly as ebm_hemispheric_mean does (the same message); phi, left
 *     underived by state-only one-step launches, is made current first; rows are read in whatever layout the handle holds
 *     them and no field is converted (ebm_state_conversions does not grow) — only the indexing of the centers and of the
 *     output is un-permuted; cells between nlat and the row pitch never reach a result; the step clock, counters[0..3] and
 *     ebm_field_step are unchanged and the two launches are not counted; both calls are synchronous on the handle's stream,
 *     the two launch chains joined first.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle or out, a field that is not a solution variable of the
 * model, a non-finite w[c] (the message names the column), a non-finite center entry (the message names the center, a or b,
 * and the latitude); EBM_ERR_STALE as above.
 * How it runs (csrc/ebm_covariance.hip): one kernel forms the block partials — grid (tiles of field_b) x (tiles of field_a) x
 * (member blocks), 256 lanes owning 64 x 64 STORED cells, so that its accesses are whole 128-byte lines in either layout;
 * sixteen members at a time pass through 20 KiB of LDS, the A side centred, weighted and NaN-cleaned on the way in, the B
 * side centred and NaN-cleaned, the next sixteen in flight under the matrix instructions; the tile, its operands and its
 * accumulators are those of csrc/ebm_mfma_tile.h, both sides staged k-major — and a second one adds the block partials per
 * element in ascending order and writes the natural index, under rule 6 both out[i][j] and out[j][i].  Under rule 6 a 64 x 64
 * tile, and inside a tile each wave's 32 x 32 block, does nothing if the natural cells it stands for hold no pair with j >=
 * i; a block that holds one is computed whole, its elements with j < i are never read.  In natural rows that skips (t - 1) /
 * 2t of the blocks, t = ceil(nlat / 32) per side; in pair-split rows a block stands for every other pair of a 64-cell span
 * and two blocks of overlapping spans are both kept, so fewer are skipped.  Tiles and waves that hold only padding do nothing
 * either.  Plain vector loads and stores, no atomics, no scratch.  Device memory, kept by the handle and reused: ceil(ncol /
 * 512) * pitch^2 doubles of block partials (pitch: nlat rounded up to the launch geometry's row, a multiple of 128), 2 *
 * pitch doubles of centers, the weights of ebm_ensemble_sums (ncol doubles), and nlat^2 doubles for the host variant's
 * result.  For nlat x ncol = 180 x 4096 (pitch 256): 4 MiB + 4 KiB + 32 KiB + 253 KiB; 1024 x 16384: 256 MiB + 16 KiB + 128
 * KiB + 8 MiB; 4096 x 2048: 512 MiB + 64 KiB + 16 KiB + 128 MiB. */
int ebm_ensemble_covariance(ebm_handle_t h, int field_a, int field_b, const double *w, const double *center_a,
                            const double *center_b, double *out);
int ebm_ensemble_covariance_device(ebm_handle_t h, int field_a, int field_b, const double *w, const double *center_a,
                                   const double *center_b, double *dev_out);

/* PER-MEMBER MISFITS TO TARGET PROFILES, reduced ALONG each column on the device: for every column c and every one of
 * ntargets target profiles, J = the weighted squared distance of the column's profiles to the target and N = the number of
 * cells that entered it — one number per member, which is what every user of the selection step (ebm_resample_columns)
 * needs first: the likelihood weight exp(-J / 2) of a particle filter against an observed T(x) or ice profile (rw = quadrature
 * weight / sigma^2), the reaction coordinate d_A / (d_A + d_B) of a splitting method between the two equilibria that
 * ebm_equilibrate found, the nearest of several reference profiles where the ensemble mean describes no member.  O(ncol)
 * doubles cross the bus, or enter an all-gather between shards, instead of O(state).  THIS TEXT IS THE DEFINITION.
 *   Arguments.  fields[nvars]: solution variables of the model, prognostic or diagnostic, each at most once; EBM_F_T0 is not
 *     one; 1 <= nvars <= 12 (the rules of ebm_ensemble_sums: one piece of code checks them for both).  1 <= ntargets <= 8.
 *     target[ntargets][nvars][nlat]: host array in natural latitude order, every entry finite or NaN; NaN means "no
 *     observation here".  rw[nvars][nlat]: host array, every entry finite and >= 0 (quadrature weight / sigma^2, or a 0 / 1 band
 *     mask); NULL = every entry 1.0.  out[ntargets][2][ncol]: out[t][0][c] = J, out[t][1][c] = N (a count, stored as a
 *     double), on the host; the _device variant writes the same packed array into the caller's device buffer dev_out.
 *   Terms.  Cell k < nlat of variable v of column c, with value x, CONTRIBUTES to target t iff rw[v][k] != 0.0,
 *     y = target[t][v][k] is not NaN and x is not NaN (the NaN sentinels of Ti and Tw, src/miz.jl:193-194: "no ice / no
 *     water here").  Its term is d = x - y, then (rw[v][k] * d) * d: a rounded difference and two rounded products, nothing
 *     contracted into a fused multiply-add.  +-Inf in a contributing x is data and propagates (J = +Inf).
 *   Order.  The bits depend neither on the launch geometry (cells_per_thread) nor on the layout the handle holds the rows in.
 *     Unit u is the pair of cells (2u, 2u + 1); units with 2u >= nlat do not exist.  Chain (l, e), l = 0 ... 63 and e = 0, 1,
 *     starts at 0.0 and adds the contributing terms of the cells k = 2 (l + 64 i) + e: for v ascending in the order of the
 *     call, and within each v for i = 0, 1, ... ascending — ONE accumulator runs across the variables.  Then
 *     q_l = chain(l, 0) + chain(l, 1); then, for s = 32, 16, 8, 4, 2, 1 in this order, q_l <- q_l + q_{l + s} for every
 *     l < s; J = q_0.  A chain without a contributor keeps its 0.0 and is added as such.  N counts the contributors the
 *     same way and is exact in any order.  No contributor at all: J = 0.0 and N = 0.0.  A term passes through at most
 *     nvars * ceil(U / 64) + 7 rounded adds, U = ceil(nlat / 2).
 *   Validity, layout, bookkeeping: those of ebm_ensemble_sums.  A diagnostic field that is older than the state fails with
 *     EBM_ERR_STALE exactly as ebm_hemispheric_mean does (the same message); phi, left underived by state-only one-step
 *     launches, is made current first; rows are read in whatever layout the handle holds them and no field is converted
 *     (ebm_state_conversions does not grow); cells between nlat and the row pitch never reach a result; the step clock,
 *     counters[0..3] and ebm_field_step are unchanged and the launch is not counted; both calls are synchronous on the
 *     handle's stream, the two launch chains joined first.  Every model: the classic one has E, Tg, T, h.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle, fields, target or out, nvars outside 1 ... 12,
 * ntargets outside 1 ... 8, a field that is not a solution variable of the model or is listed twice, an infinite target entry,
 * a negative or non-finite rw entry (the message names the first offending target, variable and latitude); EBM_ERR_STALE as
 * above.
 * How it runs (csrc/ebm_misfit.hip): ONE launch, one wave64 workgroup per column; lane l holds the chains (l, 0) and (l, 1) of
 * all targets in registers (the kernel is instantiated per ntargets).  16 bytes per lane and load: of a natural row lane l
 * reads stored unit l + 64 i, a wave 1 KiB in eight whole lines; of a pair-split row (stored unit p is natural unit 2p for
 * p < threads, 2 (p - threads) + 1 otherwise) an even lane reads l / 2 + 32 i and an odd one threads + (l - 1) / 2 + 32 i, two
 * contiguous 512-byte runs of whole lines.  Targets and rw are read in the natural layout, shared by all columns.  The loads
 * of several units are issued ahead of the dependent adds; the finish is the six-step cross-lane tree.  No LDS, no atomics,
 * no scratch, plain loads and stores.  Device memory, kept by the handle and reused: 8 * 12 * pitch doubles of targets,
 * 12 * pitch of rw, and 2 * 8 * ncol doubles for the host variant's result. */
int ebm_column_misfits(ebm_handle_t h, int nvars, const int *fields, int ntargets, const double *target, const double *rw,
                       double *out);
int ebm_column_misfits_device(ebm_handle_t h, int nvars, const int *fields, int ntargets, const double *target,
                              const double *rw, double *dev_out);

/* ENSEMBLE KALMAN UPDATE: every member moved by a linear map of its own innovation,
 *     x_f[c][k] += sum_j G_f[k][j] * d[c][j],      d[c][j] = (target[j] + e[c][j]) - scale * xo[c][j],
 * for every listed prognostic field f, on the device — the write that the reductions above lacked.  With G the Kalman gain
 * formed on the host from ebm_ensemble_covariance (nlat^2 numbers, which a Schur product can localise there) this is the
 * analysis step of an EnKF: target = y, scale = 1 and e = observation noise is the perturbed-observation filter;
 * target = y - mean/2, scale = 1/2, e = NULL is the deterministic one (EnsembleRun.enkf).  An (ncol x nlat) . (nlat x nlat)
 * product per field, the second dense contraction of the library: it runs on the fp64 matrix instruction of gfx950.  No field
 * leaves the device.  THIS TEXT IS THE DEFINITION.
 *   Arguments.  fields[nvars]: PROGNOSTIC fields of the model (MIZ and MIZ_IMEX: Ei, Ew, h, D, phi; classic: E, Tg), each at
 *     most once, 1 <= nvars <= 5.  obs_field: any solution variable under the rules of ebm_ensemble_sums, prognostic or
 *     diagnostic; it may be one of `fields`.  gain[nvars][nlat][nlat]: host array, gain[v][k][j] maps observation cell j to
 *     cell k of fields[v], natural latitude order, every entry finite; the _device variant takes the same packed array at a
 *     16-byte aligned device address and does not look at its entries.  target[nlat]: host array, finite or NaN; NaN means
 *     "no observation here", as in ebm_column_misfits.  scale: finite.  dev_perturb[ncol][nlat]: packed DEVICE array of
 *     e[c][j], or NULL.  lo[nvars], hi[nvars]: host arrays of per-field bounds, either may be NULL = none.
 *   Innovation.  For column c and observation cell j < nlat, with xo the cell of obs_field: s = scale * xo, t = target[j] +
 *     e[c][j] (t = target[j] when dev_perturb is NULL), d = t - s — one rounded product, one rounded add, one rounded
 *     subtract, nothing contracted into a fused multiply-add.  d is replaced by +0.0 where target[j] is NaN or xo is NaN (the
 *     sentinels of Ti and Tw, src/miz.jl:193-194).  ALL innovations are formed from the state as it is at entry, before any
 *     field is written — also when obs_field is one of the fields.
 *   Increment.  For field v and state cell k the accumulator starts at +0.0 and takes the observation cells in ascending
 *     groups of four, ONE v_mfma_f64_16x16x4_f64 per group: acc <- mfma(d[c][j .. j+3], gain[v][k][j .. j+3], acc), d always
 *     the A operand.  The products and adds inside the instruction are the hardware's; this text fixes everything around
 *     them.  A tail group is padded with terms d = g = +0.0; a group wholly past nlat is not issued.  The j axis is never
 *     split: no partials, no atomics.  Every (c, k) sees the same chain whichever tile, wave and register of the kernel it
 *     falls in, so the bits depend neither on the launch geometry (cells_per_thread) nor on the layout the handle holds the
 *     rows in, and the same call on the same data gives the same bits on every run.
 *   Write.  x_new = x + acc, ONE rounded add — so a cell holding -0.0 with acc = +0.0 becomes +0.0, also under a gain of
 *     zeros.  Then, with bounds: x_new = lo[v] if x_new < lo[v]; then x_new = hi[v] if x_new > hi[v].  The comparisons are
 *     strict; a NaN x_new passes through; -Inf / +Inf bounds mean none and give the bits of the unbounded call.
 *   Accuracy.  The stated terms of (c, k) are p_j = d[c][j] * gain[v][k][j], j < nlat, n_obs of them nonzero.  Inside a
 *     group the hardware forms four products and adds them to acc in some order, each operation — multiply, add or fused
 *     multiply-add — correctly rounded: a term passes through at most one product rounding and then one add per term that
 *     joins the same sum after it, and only nonzero terms round (x + 0 is exact).  So a term sees at most n_obs roundings,
 *     each of relative size 2^-53 on a partial sum bounded by sum_j |p_j| (1 + O(2^-53)), and
 *       |acc - the exact sum of the stated terms| <= n_obs * 2^-53 * sum_j |d * g| * (1 + 2^-4);
 *     the last factor covers the second-order terms (and the 64-bit-mantissa reference of the tests), as in
 *     ebm_ensemble_covariance.  x_new adds the one rounding of x + acc: 2^-53 |x + acc|.
 *   Validity and bookkeeping: exactly those of one ebm_set_field per listed field with the new values, through the same
 *     code of the field book — the diagnostic fields and the fp64 T0 become stale (EBM_ERR_STALE names the step that wrote
 *     them and the state's step, "with prognostic fields overwritten since"), the next step loads phi as it then is, the
 *     zero-line flags lose their trust, a graph-replaying ebm_run takes its first step directly.  A stale obs_field fails
 *     with EBM_ERR_STALE exactly as ebm_hemispheric_mean does (the same message); phi, left underived by state-only one-step
 *     launches, is made current first.  Unchanged: the step clock, counters[0..3], the warm-start active set, the noise
 *     state, every per-column setting.
 *   Layout.  Rows are read AND written in whatever layout the handle holds them; only gain, target, dev_perturb and the
 *     staged innovations are indexed by natural latitude.  No field is converted: ebm_state_conversions does not grow.  Cells
 *     between nlat and the row pitch are never written.
 *   Ordering.  Synchronous on the handle's stream, the two launch chains joined first.
 * Refusals leave the handle bit for bit as it was: EBM_ERR_ARG for a NULL handle, fields, gain or target, nvars outside
 * 1 ... 5, a field that is not prognostic or is listed twice, an obs_field that is not a solution variable, a non-finite
 * scale, a non-finite gain entry (host variant; the message names field, k and j), an infinite target entry, a NaN bound or
 * lo[v] > hi[v], a device gain that is not 16-byte aligned or a dev_perturb that is not 8-byte aligned; EBM_ERR_STALE as above.
 * How it runs (csrc/ebm_update.hip): kernel 1 stages d for all columns, one lane per 16-byte unit of the row of obs_field
 * where it lies, into [ncol][pitch] doubles in natural order with +0.0 beyond nlat — the scratch of ebm_diffusion where the
 * handle has it, else the staging rows of ebm_resample_columns.  Kernel 2 is the tiled product: grid (tiles of 64 STORED
 * cells) x (tiles of 64 members) x (fields), 256 lanes; sixteen observation cells at a time pass through 9 KiB of LDS — 32
 * bytes of d of one member and four gain entries of one state cell per lane — the next sixteen in flight under the matrix
 * instructions; the tile, its operands and its accumulators are those of csrc/ebm_mfma_tile.h, both sides staged line-major;
 * then the add, the clamp and the store, sixteen lanes a whole 128-byte line of a row.  Tiles and waves that hold only padding
 * do nothing.  The host variant uploads gain one field at a time into one pitch^2 buffer and launches the product per field;
 * the _device variant is one launch over a grid z of fields.  Plain vector loads and stores, no atomics, no scratch
 * memory.  Device memory, kept by the handle and reused: pitch^2 doubles of gain (host variant), pitch doubles of target, and
 * the borrowed ncol * pitch of innovations. */
int ebm_update_columns(ebm_handle_t h, int nvars, const int *fields, int obs_field, const double *gain, const double *target,
                       double scale, const double *dev_perturb, const double *lo, const double *hi);
int ebm_update_columns_device(ebm_handle_t h, int nvars, const int *fields, int obs_field, const double *dev_gain,
                              const double *target, double scale, const double *dev_perturb, const double *lo, const double *hi);

/* KALMAN GAIN ON THE DEVICE: the middle of the filter, between ebm_ensemble_covariance_device and
 * ebm_update_columns_device — a symmetric positive definite solve in fp64 by a blocked Cholesky factorisation on the matrix
 * instruction of gfx950, so that an analysis step moves O(nlat) numbers over the bus.  THIS TEXT IS THE DEFINITION.
 *   The system.  S is m x m, symmetric positive definite, row-major, full storage; the right-hand sides are the ROWS of B
 *     ([nrhs][m]); the result X has X . S = B (S is symmetric: numpy.linalg.solve(S, B.T).T).  Everything works on mp = m
 *     rounded up to nb = 64 with the identity in the padding of S and +0.0 in the padding columns of B, so that no step below
 *     has a tail and the padding never reaches a result.  T = mp / 64 block columns; A_ij is the 64 x 64 tile (i, j) of S.
 *   Products.  Every matrix product below is, per element, ONE chain acc <- mfma(x[t .. t+3], y[t .. t+3], acc) of
 *     v_mfma_f64_16x16x4_f64 over the contraction index t = 0, 4, 8, ... ascending, from +0.0, the left factor the A operand,
 *     whichever tile, wave and register the element falls in.  Nothing else is contracted into a fused multiply-add.
 *   Factor, right-looking, for k = 0 ... T - 1:
 *     (a) the diagonal tile A_kk, for its columns j = 0 ... 63 in turn: s = sqrt(a[j][j]); a[i][j] <- a[i][j] / s for i > j;
 *         a[i][c] <- a[i][c] - a[i][j] * a[c][j] for j < c <= i; a[j][j] <- s.  The first pivot a[j][j] that is not > 0 (a
 *         NaN is not) records its 1-based index 64 k + j + 1; the sweep goes on regardless, and every later step of the call
 *         does nothing.  Then W = inverse of L_kk by forward substitution per column c: W[i][c] = ((i == c ? 1 : 0) -
 *         sum_{c <= j < i} L[i][j] * W[j][c]) / L[i][i], the terms subtracted one by one in ascending j.
 *     (b) the panel: A_ik <- A_ik . W^T for i > k (contraction over the 64 columns of the tile).
 *     (c) the trailing tiles: A_ij <- A_ij - L_ik . L_jk^T for i >= j > k, one rounded subtraction after the chain.  Only
 *         tiles of the lower triangle are read or written (the diagonal tiles whole; their strict upper parts are scratch).
 *   Solve.  Forward, k ascending:   W = B_k - sum_{t < 64 k} Y[.][t] * L[64 k + c][t];        Y_k = W . inv(L_kk)^T.
 *           Backward, k descending: W = Y_k - sum_{t >= 64 (k + 1)} X[.][t] * L[t][64 k + c];  X_k = W . inv(L_kk).
 *     The sums run over ALL earlier (later) columns in one chain; W = B_k - acc is one rounded subtraction.  Rows are
 *     independent: a workgroup owns 64 of them for the whole walk and writes W and then the result to B in place.
 *   ebm_spd_solve_device: the solver on caller-owned device buffers.  dev_S [mp][lds], dev_B [nrhs][ldb], lds, ldb >= mp, both
 *     16-byte aligned; the caller has padded them as above (or m is a multiple of 64).  On return the lower triangle of S
 *     holds L, B holds X and *info = 0.  If S is not positive definite, *info is the 1-based index of the first bad pivot,
 *     the call returns EBM_ERR_ARG with a message naming that index, and B is unspecified.
 *   ebm_kalman_gain_device: obs[nlat] (host; NaN = unobserved, J = the observed cells ascending, m of them), obs_var[nlat]
 *     (host; read at the observed cells), localize (half-width in x of the taper; <= 0: none), factor (inflation * n / (n - 1)
 *     for covariance sums divided by n), dev_Poo and Pfo_addr[v], v < nvars (a HOST array of device addresses): packed
 *     [nlat][nlat] device matrices, read only (Pfo_addr[v] may be dev_Poo) — typed double ** although nothing is written
 *     through it: const double *const * is what it means —, dev_gain [nvars][nlat][nlat], what ebm_update_columns_device
 *     takes.  Covariances, not field ids, so
 *     that a sharded run can all-reduce them first.  Assembly, one rounding per operation in this order:
 *       S[a][b]          = (rho(J[a], J[b]) * Poo[J[a]][J[b]]) * factor + (a == b ? obs_var[J[a]] : 0.0)
 *       B[v nlat + k][a] = (factor * rho(k, J[a])) * Pfo_v[k][J[a]],  a non-finite Pfo entry taken as +0.0
 *     rho(i, j) = the Gaspari-Cohn taper of r = |x_i - x_j| / localize: for r <= 1 (((-r/4 + 1/2) r + 5/8) r - 5/3) r^2 + 1, for
 *     1 < r < 2 (((r/12 - 1/2) r + 5/8) r + 5/3) r^2 - 5 r + 4 - 2/(3 r), else 0, clipped to [0, 1], evaluated left to right as
 *     written (gaspari_cohn of the Python package, bit for bit); exactly 1.0 without localisation.  Then the solve with
 *     nrhs = nvars * nlat, and gain[v][k][J[a]] = X[v nlat + k][a], +0.0 in every column of an unobserved cell.  No observed
 *     cell at all: a gain of +0.0 and no solve.  A bad pivot — a NaN covariance at an observed cell is one — returns
 *     EBM_ERR_ARG with *info set and a message naming the pivot and its observed latitude J[info - 1]; dev_gain is unspecified.
 *   Determinism.  The order of every operation is fixed above and depends on nothing but m and nrhs: the same call on the same
 *     data gives the same bits on every run, for every cells_per_thread and whatever layout the handle holds its rows in (the
 *     covariances are natural-order matrices).
 *   Ordering and bookkeeping.  Synchronous on the handle's stream, the two launch chains joined first.  Neither call reads or
 *     writes a field: no field's validity, the step clock, the counters and ebm_state_conversions do not change, and the
 *     launches are not counted.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL handle or pointer, a device pointer that is not 16-byte
 * aligned, m < 1, nrhs < 0, lds or ldb < mp; nvars outside 1 ... 5, an infinite obs entry, an obs_var entry at an observed
 * cell that is not finite and > 0, a factor that is not finite and > 0, a NaN localize; and the bad pivot above.
 * How it runs (csrc/ebm_gain.hip): every product is the 256-lane, 64 x 64 tile of csrc/ebm_mfma_tile.h, operands staged
 * line-major sixteen t at a time through 9 KiB of LDS, the next sixteen in flight under the matrix instructions.  (a) is
 * one workgroup with the tile in 32.5 KiB + 16.25 KiB of LDS, two barriers per column; (b) is T - k - 1 workgroups and (c)
 * (T - k - 1)^2, of which the upper half return at once: three launches per block column.  Each solve
 * direction is ONE launch of ceil(nrhs / 64) workgroups; a workgroup re-reads only what it wrote itself, behind a block-level
 * fence and a barrier.  Assembly and scatter are one lane per element.  Plain vector loads and stores, no atomics, no scratch
 * memory.  Device memory, kept by the handle, reused and freed by ebm_destroy: 64 mp doubles of block inverses and one int
 * of flag; for the gain also mp^2 doubles of S, nvars * nlat * mp of B, nlat of obs_var and mp + nlat ints of index lists. */
int ebm_spd_solve_device(ebm_handle_t h, int m, long long nrhs, double *dev_S, long long lds, double *dev_B, long long ldb, int *info);
int ebm_kalman_gain_device(ebm_handle_t h, int nvars, const double *obs, const double *obs_var, double localize, double factor,
                           const double *dev_Poo, double **Pfo_addr, double *dev_gain, int *info);
/* elapsed_ms[4]: the time between HIP events on the handle's stream around the assembly, the factorisation, the two solves and
 * the scatter of the LAST ebm_kalman_gain_device call of this handle that ran a solve (EBM_ERR_ARG: there was none, or a
 * NULL argument).  Measurement only; the events are always recorded (five per call). */
int ebm_kalman_gain_phases(ebm_handle_t h, float *elapsed_ms);

/* COLUMN SCALARS: numbers that reduce ALONG a column — the integral or mean of a field over a band of latitudes, and the
 * position of an edge: where, walking poleward, a field first reaches a level (the ice edge: the first cell with phi >= 0.15).
 * The number this model is known for, per member, without a field leaving the device.  THIS TEXT IS THE DEFINITION.
 *   A column scalar is described by four ints and one double: spec[s] = {kind, field, k0, k1}, where 0 <= k0 <= k1 <= nlat-1
 *     are 0-based cell indices, both inclusive, and level[s], which the edge kinds use and the others ignore.  `field` is a
 *     solution variable of the model under the rules of ebm_run_series: EBM_F_T0 is not one; a diagnostic field that is older
 *     than the state gives EBM_ERR_STALE with ebm_hemispheric_mean's message; phi, left underived by state-only one-step
 *     launches, is made current first.  f: the field's row of the column, x: the grid.
 *   EBM_S_INTEGRAL requires k0 < k1.  Start at 0.0 and add ((f[i]+f[i+1]) * (x[i+1]-x[i])) / 2.0 for i = k0 .. k1-1, strictly
 *     left to right: the very operations of ebm_hemispheric_mean, whose result the full range k0 = 0, k1 = nlat-1 therefore
 *     gives bit for bit.  A NaN in the band gives NaN.
 *   EBM_S_MEAN is that integral divided once, with the library's IEEE division, by x[k1] - x[k0].
 *   EBM_S_EDGE_GE / EBM_S_EDGE_LE require a level that is not NaN.  hit(k) is f[k] >= level for GE and f[k] <= level for LE; it
 *     is false for NaN.  K is the smallest k in k0 .. k1 with a hit.  No hit: the value is +Inf ("no edge in the band"), so
 *     that edge >= x* is true of an ice-free column, which is what a first-passage test on ice loss needs.  K == k0: the value
 *     is x[k0].  Otherwise let a = f[K-1] and b = f[K]; if either is not finite, the value is x[K]; otherwise
 *     t = (level - a) / (b - a) and the value is x[K-1] + t * (x[K] - x[K-1]), every operation rounded once, nothing contracted
 *     into a fused multiply-add.  The value depends only on K and four loads, so the bits do not depend on the order of the
 *     search.  Walking poleward (ascending k) is the only direction: the model has one hemisphere.
 *   1 <= nscal <= 12; the same field may appear in several scalars.
 * ebm_column_scalars: out[nscal][ncol] on the host; the _device variant writes the same packed array into the caller's device
 * buffer.  Both make every field readable exactly as ebm_hemispheric_mean makes its one (the same layout conversions, counted
 * by ebm_state_conversions the same way), leave the step clock, the counters and ebm_field_step unchanged, and are synchronous.
 * Refusals leave the handle as it was: EBM_ERR_ARG for a NULL argument, nscal outside 1 ... 12, an unknown kind, a field that
 * is not a solution variable of the model, k0 or k1 out of range or k0 > k1, k0 == k1 of an integral kind, a NaN level of an
 * edge kind — the message names the first offending scalar; EBM_ERR_STALE as above.
 * How it runs (csrc/ebm_launch.hip): ONE launch, one wave64 workgroup per (column, scalar).  The integral kinds are the
 * library's one mean walk (hemispheric_means_of_column) over the band: they cost what ebm_hemispheric_mean costs on as many
 * terms.  The edge kinds walk the band in tiles of 256 cells — each lane four coalesced loads, a cross-lane min of the first
 * hit — and stop at the first tile with a hit, so a row is read at most once; lane 0 then loads the four cells and interpolates.
 * No LDS beyond the mean's tile, no atomics, no scratch, plain loads and stores; rows are read in the natural layout. */
enum ebm_scalar_kind { EBM_S_INTEGRAL = 0, EBM_S_MEAN = 1, EBM_S_EDGE_GE = 2, EBM_S_EDGE_LE = 3, EBM_S_COUNT };
int ebm_column_scalars(ebm_handle_t h, int nscal, const int *spec, const double *level, double *out);
int ebm_column_scalars_device(ebm_handle_t h, int nscal, const int *spec, const double *level, double *dev_out);
/* ebm_run_series with the nscal column scalars for a sample, and nothing else different: stepping, the diag rule (diag = 1 iff
 * one of the scalars' fields is diagnostic), sample steps, launch counts, the state afterwards, the refusals and the one
 * download at the end are those of ebm_run_series.  series[nscal][nsamples][ncol]: series[s][j][c] is bit for bit what
 * ebm_column_scalars puts into out[s][c] after ebm_run_fused(h, first_step, (j+1)*every, f_steps, diag, steps_per_launch) from
 * the same start.  One loop in the library drives both calls. */
int ebm_run_series_scalars(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int every, int steps_per_launch,
                           int nscal, const int *spec, const double *level, double *series);
/* ebm_run_until with m_c = the column scalar spec[4] = {kind, field, k0, k1}, scalar_level of column c in place of the mean, and
 * nothing else different: rounds, crossing rule, freezing, outputs, clock, counters, validity bookkeeping and the one stream
 * synchronisation per round are those of ebm_run_until (diag = 1 iff the field is diagnostic).  A NaN m_c never crosses; the
 * +Inf of a band without an edge crosses an upward test: "stop when the ice edge has passed x*, or the ice is gone".
 * level[ncol], direction[ncol]: the per-column thresholds of ebm_run_until.  Refusals: those of ebm_run_until and, for the
 * scalar, of ebm_column_scalars.  One loop in the library drives both calls. */
int ebm_run_until_scalar(ebm_handle_t h, long long first_step, int max_samples, int every, const double *f_steps, int steps_per_launch,
                         const int *spec, double scalar_level, const double *level, const int *direction, int *samples,
                         int *crossed, double *value);

int ebm_sync(ebm_handle_t h);

/* ---- measurement / diagnostics ------------------------------------------------------- */

/* counters[0] steps, [1] tridiagonal solves summed over columns, [2] column-steps whose T0
 * active-set iteration hit its cap, [3] kernel launches.  Synchronises the stream. */
int ebm_get_counters(ebm_handle_t h, long long *counters);
int ebm_reset_counters(ebm_handle_t h);
/* *count: how often the handle has converted its prognostic fields between the natural layout and the layout private to
 * the one-launch-per-step MIZ kernel at four cells per thread (one in-place pass over the five fields each; see
 * ebm_field_device_ptr).  A steady loop of ebm_step / ebm_run converts once, at its start; reading or setting a prognostic
 * field, a fused launch, a series sample or a seasonal snapshot between two such steps costs two.  Since ebm_create (not
 * reset by ebm_reset_counters).  Does not synchronise. */
int ebm_state_conversions(ebm_handle_t h, long long *count);
/* The zero-line flags of a handle that elides zero lines (ebm_options::elide_zero_lines; EBM_ERR_UNSUPPORTED on any other),
 * read-only, for tests and cost tools: words[col * (threads / 64) + wave] with threads = info[0] of ebm_launch_info.  Bit
 * 4*j + f of a word, j = 0, 1 and f = 0 (Ei), 1 (Ew), 2 (h), 3 (D): the KiB of field f that holds cells 4t + 2j and
 * 4t + 2j + 1 of the wave's threads t = 64 wave .. 64 wave + 63 — in the layout private to the one-step kernel, where it is
 * contiguous — held only zero bits when the column was last stepped by the eliding kernel.  *trusted = 1: every set bit is
 * true now; 0: somebody else has written or moved the prognostic fields since, and the library will clear all flags before
 * it uses them again.  Synchronises the handle's stream. */
int ebm_zero_line_flags(ebm_handle_t h, unsigned *words, int *trusted);
/* HIP-event timing on the handle's stream (the stream the kernels are launched on). */
int ebm_timer_start(ebm_handle_t h);
int ebm_timer_stop(ebm_handle_t h, float *elapsed_ms);
/* Launch geometry chosen for this handle: info[0] threads per workgroup, [1] cells per
 * thread, [2] dynamic LDS bytes per workgroup, [3] workgroups per launch. */
int ebm_launch_info(ebm_handle_t h, int *info);
/* Self-test: q[i] = a[i] / b[i] computed on the device with the division routine the physics
 * kernels use (bit-exact IEEE fp64 division is part of the parity contract). */
int ebm_selftest_divide(int device, int n, const double *a, const double *b, double *q);
/* Self-test: the in-place layout conversions of the MIZ fields at four cells per thread, on ncol columns of 4*threads
 * cells (threads: a multiple of 64, <= 1024): split[ncol][4*threads] = `in` taken from the natural layout to the private
 * one (pair j of thread t, cells 4t+2j and 4t+2j+1, at j*2*threads + 2t), back[...] = that taken back again. */
int ebm_selftest_permute(int device, int threads, int ncol, const double *in, double *split, double *back);

#ifdef __cplusplus
}
#endif
#endif /* EBM_HIP_H */
