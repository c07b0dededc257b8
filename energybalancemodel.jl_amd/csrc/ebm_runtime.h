// Shared by the four translation units of the host runtime behind the C ABI of include/ebm_hip.h: the handle, the error
// idioms, the handle's stream and the field predicates.
//   ebm_runtime.hip   errors, options, create / destroy, sync, counters, timers, stamps, self-test, launch info
//   ebm_fields.hip    field I/O with the validity bookkeeping, device views, hemispheric means, the two diffusion operators
//   ebm_columns.hip   per-column forcing, schedules, noise and parameter sets; the step clock and the time table; resampling
//   ebm_drive.hip     step launches, graph replay, fused ranges, series, integrate, equilibrate, run-until
// Not part of the public interface.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/ebm_hip.h"
#include "ebm_hostcopy.h"
#include "ebm_internal.h"

using ebm_host::CopyJob;
using ebm_host::DevBuf;
using ebm_host::DevVec;
using ebm_host::Event;
using ebm_host::GraphExec;
using ebm_host::HostCopier;
using ebm_host::PinnedBuf;
using ebm_host::Stream;
using ebm_host::dev_alloc;

namespace ebm_rt {

extern thread_local std::string g_err;            // ebm_last_error (defined in ebm_runtime.hip)

inline int fail(int code, const std::string &msg) {
    g_err = msg;
    // a failed runtime call leaves its code as the thread's "last error", which the next kernel launch's
    // hipGetLastError() check would report as its own: the failure has been reported here, so clear it
    if (code == EBM_ERR_HIP) (void)hipGetLastError();
    return code;
}
// EBM_ERR_HIP with the message "<what>: <HIP's text for e>"
inline int hip_fail(const std::string &what, hipError_t e) { return fail(EBM_ERR_HIP, what + ": " + hipGetErrorString(e)); }
#define HIPCHK(expr)                                                   \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return ebm_rt::hip_fail(#expr, e_);      \
    } while (0)

// runs `f` when it goes out of scope, on every path
template <class F>
struct Finally {
    F f;
    ~Finally() { f(); }
};
template <class F>
Finally<F> finally(F f) { return {std::move(f)}; }

}  // namespace ebm_rt

// Every resource of the handle is held by an owner (ebm_host::Owned, DevVec, unique_ptr) and freed by it; the state of a
// feature is one member, which a call that installs it replaces with one move after everything new has been built (an
// install either succeeds or leaves the handle as it was).  Raw pointers here are views.
struct ebm_ctx {
    // declared first, destroyed last: the buffers below are freed before the streams and events of their work
    Stream stream;                                 // THE stream of the handle: everything is ordered on it (see main_stream)
    // Two chains of step launches.  Long meridians leave room for ONE workgroup per CU, so within a launch nothing runs under
    // a workgroup's load, solve and store phases, and a launch cannot start before the slowest workgroup of the previous one
    // has ended.  Columns are independent: the first half of them is stepped on `stream`, the second on `stream2`, each half
    // its own chain of launches; the chains drift apart and fill each other's gaps (measured on 4096 x 2048: 0.1656 ->
    // 0.1594 ms per step, tests/tools/ab_two_handles.py).  `forked` = the chains are running apart; any other use of the
    // handle's stream joins them first (main_stream).
    Stream stream2;
    Event ev0, ev1, ev_fork, ev_join;
    int split_col = 0;                             // 0: one chain; else the first column of the second chain
    bool forked = false;
    int model = 0, grid = 0, nlat = 0, ncol = 0, device = 0;
    bool imex = false;                             // EBM_MODEL_MIZ_IMEX: model == EBM_MODEL_MIZ plus the implicit-diffusion extension
    long long pitch = 0;
    double dt = 0.0;
    ebm::Params p{};
    ebm::LaunchCfg cfg{};
    DevBuf<ebm::Params> p_dev;                     // parameter block in device memory
    DevBuf<double> geom;                           // per-latitude tables, G_COUNT x gstride
    long long gstride = 0;
    // ebm_set_column_params: one parameter block and one geometry slab per distinct row (n of them, 0 = no table: every
    // column steps with p_dev / geom), and the column -> set index (null when every column has set 0)
    struct ParamSets {
        int n = 0;
        DevBuf<ebm::Params> p;
        DevBuf<double> geom;                       // n x G_COUNT x gstride
        DevBuf<int> col;
        std::vector<ebm::Params> host;             // host copies (the zonal operator's D and cw)
    } sets;
    DevBuf<double> state;                          // field slab, nslots x fstride
    long long fstride = 0;
    int nslots = 0;
    double *field[EBM_F_COUNT] = {nullptr};        // views into the slab (null: not in this model)
    DevBuf<double> fcol;
    DevBuf<double> fsched;                         // per-column Forcing schedules
    // ebm_set_column_noise: the per-column records, the AR(1) state N_c (null: no noise) and the seed
    struct Noise {
        DevBuf<ebm::NoiseRec> rec;
        DevBuf<double> state;
        DevBuf<double> seq;                        // [ncol][kNoiseMaxFused], the fused kernels' per-launch N_c sequence
        unsigned long long seed = 0;
    } noise;
    long long clock = 0;                           // global index of the next step (model time of ebm_step)
    DevBuf<unsigned long long> stamps;             // diagnostic builds only
    int num_cus = 0;
    int prefetch = 0;                 // L2 prefetch distance of the MIZ kernel, columns (0 = off)
    DevBuf<double> hm_dev;            // ebm_hemispheric_mean: per-column results on the device
    // per-step scalars of the fused-K launches: two device tables of kFusedTable entries used in turn, each with the event
    // that marks the end of the launches that read it — a table is refilled only after that event, so consecutive fused
    // calls neither wait for each other nor synchronise the stream
    struct SchedTable { DevBuf<ebm::StepSched> dev; Event done; bool in_use = false; } sched_tab[2];
    int sched_next = 0;
    int integrate_spl = 64;                  // ebm_options::integrate_steps_per_launch (1 = one launch per step)
    // hipGraph replay for launch-bound shapes (small grids): kGraphSteps step kernels per replay, node i reads sched[i]
    struct Graph { DevBuf<ebm::StepSched> sched; GraphExec exec; } graph;
    bool use_graph = false;
    std::vector<double> ttab;                      // cos(2*pi*t_i), host copy
    DevBuf<unsigned long long> counters;           // device, kCounterShards x 2
    DevBuf<unsigned short> amask;                  // MIZ warm-start active set, ncol x threads
    long long n_steps = 0, n_launches = 0;
    // ebm_equilibrate and ebm_run_until, for the duration of the call only: the launches step the columns active[0 .. nactive) (device list,
    // ascending) instead of all of them
    const int *active = nullptr;
    int nactive = 0;
    // Validity of the fields that only some steps write (diagnostics, the fp64 T0): `epoch` counts every change
    // of the prognostic state (steps taken, prognostic fields overwritten), `state_step` is the global index of
    // the last step taken (-1: none); a field is current iff written_epoch[f] == epoch.
    long long epoch = 0, state_step = -1;
    long long written_epoch[EBM_F_COUNT], written_step[EBM_F_COUNT];
    // The MIZ step kernels (4 cells per thread) store the five diagnostic fields in the pair-split layout (whole
    // 128-B lines per store instruction, csrc/ebm_miz_step.h); whoever reads one of them gets the natural layout:
    // the first reader after such a step runs the in-place un-permutation once.
    bool diag_split = false;
    // The same layout holds the five prognostic fields BETWEEN one-step launches at 4 cells per thread (miz_step_kernel
    // reads and writes them pair-split).  One rule (set_state_layout): the one-step launch path splits them first if they
    // are natural; every other reader or writer of a prognostic field — field I/O and views, the fused and resident
    // kernels, series, hemispheric means, snapshots — un-splits them first.  A steady ebm_run / ebm_step loop converts
    // nothing; n_conversions counts the conversions of a handle (ebm_state_conversions).
    bool state_split = false;
    long long n_conversions = 0;
    // One more bit of the same rule.  A state-only one-step launch of the reference's step at four cells per thread does not
    // store phi: after any step phi is concentration(Ei, h) of the stored fields, and the kernel forms it from them
    // (miz_step_kernel, PHI_DERIVED).
    //   phi_stored       the phi field in HBM is current.  Cleared by such a launch; false only while state_split.
    //                    Whoever reads phi otherwise restores it first (restore_phi; convert_state folds it into the
    //                    un-split pass): a restore with the bit set does nothing, a steady run of launches restores nothing.
    //   phi_consistent   Ei, h and phi were last written by step kernels of this library, so phi IS that function of Ei and
    //                    h under the column's parameters.  Cleared by every other writer of one of them and by a change of
    //                    the parameters (state_written_outside); set again by the next step launch over all columns.  Only
    //                    then may a launch take the deriving kernel; else it steps with the phi the caller left.
    bool phi_stored = true, phi_consistent = true;
    bool derive_phi = false;                       // this handle has the deriving kernel (ebm_create: has_phi_derived_kernel)
    // ebm_zonal_diffusion: the tables of the last nlon used, kept between calls
    struct ZonalTables {
        int nlon = 0, seg = 1;                     // seg: segments a circle is cut into (a function of nlon only)
        DevBuf<double> tab;                        // chain tables | reduced-system tables | per-latitude scalars | scratch
        double *M = nullptr, *E = nullptr, *rM = nullptr, *rE = nullptr, *a = nullptr, *a2 = nullptr, *W = nullptr,
               *su = nullptr, *sg = nullptr, *sy = nullptr;       // views into tab
    } zonal;
    std::vector<double> xhost;                     // st.x (the zonal tables are built on demand)
    std::unique_ptr<HostCopier> copier;            // pinned staging ring, lazily created by the first host transfer
    DevBuf<double> scratch;                        // ebm_diffusion / ebm_zonal_diffusion: three fields, kept between calls
    // ebm_resample_columns, kept between calls: the list of moved columns — (destination, parent) pairs — in pinned host
    // memory and on the device, the event after which the pinned list may be refilled (the upload has read it), and the
    // staging rows of a handle that has no `scratch`
    struct Resample {
        PinnedBuf<int> host;
        size_t host_cap = 0;                       // pairs
        DevVec<int> dev;
        DevVec<double> stage;
        Event uploaded;
        bool in_flight = false;
    } resample;
    // ebm_ensemble_sums, kept between calls: the block partials, the uploaded weights and centers ([nvars][pitch], padding
    // zero) and the result of the host variant
    struct EnsembleSums {
        DevVec<double> partial, w, center, out;
    } sums;
    // ebm_integrate's device buffers, kept between calls while the shape stays the same
    DevVec<double> ig_sums, ig_mean, ig_snap, ig_stage, ig_hm;
    ~ebm_ctx();
};

namespace ebm_rt {

// The handle's stream for everything that is not a step launch.  If the two chains of step launches are running apart
// (ebm_ctx::forked), the second one is joined first: whatever is enqueued next is ordered after all steps of all columns.
inline hipStream_t main_stream(ebm_ctx *h) {
    if (h->forked) {
        (void)hipEventRecord(h->ev_join.get(), h->stream2.get());
        (void)hipStreamWaitEvent(h->stream.get(), h->ev_join.get(), 0);
        h->forked = false;
    }
    return h->stream.get();
}

// st.x on the device (the same in every parameter set)
inline const double *x_table(const ebm_ctx *h) { return h->geom.get() + (size_t)ebm::G_X * h->gstride; }

// slab slot of a public field id for this model, -1 if the model does not have it
inline int slot_of(int model, int f) {
    if (model == EBM_MODEL_MIZ) return (f >= EBM_F_Ei && f <= EBM_F_T) ? f : -1;   // same order
    switch (f) {
        case EBM_F_E: return ebm::C_E;
        case EBM_F_Tg: return ebm::C_Tg;
        case EBM_F_T: return ebm::C_T;
        case EBM_F_h: return ebm::C_h;
        default: return -1;
    }
}
inline bool has_field(const ebm_ctx *h, int f) { return f >= 0 && f < EBM_F_COUNT && slot_of(h->model, f) >= 0; }

// fields that only diagnostic steps write (everything else is prognostic and always current)
inline bool is_diagnostic(const ebm_ctx *h, int f) {
    if (h->model == EBM_MODEL_MIZ)
        return f == EBM_F_T0 || f == EBM_F_Tw || f == EBM_F_Ti || f == EBM_F_n || f == EBM_F_E || f == EBM_F_T;
    return f == EBM_F_T || f == EBM_F_h;
}
// the diagnostic fields that a 4-cells-per-thread MIZ step stores pair-split (ensure_natural)
inline bool is_split_field(const ebm_ctx *h, int f) {
    return h->model == EBM_MODEL_MIZ && (f == EBM_F_Tw || f == EBM_F_Ti || f == EBM_F_n || f == EBM_F_E || f == EBM_F_T);
}
// the prognostic fields that a 4-cells-per-thread MIZ one-step launch keeps pair-split (set_state_layout)
inline bool is_split_state_field(const ebm_ctx *h, int f) {
    return h->model == EBM_MODEL_MIZ && f >= EBM_F_Ei && f <= EBM_F_phi;
}
inline const char *field_name(int f) {
    static const char *names[EBM_F_COUNT] = {"Ei", "Ew", "h", "D", "phi", "T0", "Tw", "Ti", "n", "E", "T", "Tg"};
    return (f >= 0 && f < EBM_F_COUNT) ? names[f] : "?";
}
// EBM_OK if `f` may be read now, else EBM_ERR_STALE with the two steps in the message
inline int check_current(const ebm_ctx *h, int f, const char *who) {
    if (!is_diagnostic(h, f) || h->written_epoch[f] == h->epoch) return EBM_OK;
    std::string msg = std::string(who) + ": field " + field_name(f) + " is stale — ";
    if (h->written_epoch[f] < 0) msg += "it has never been written";
    else if (h->written_step[f] < 0) msg += "it holds what it held before the first step";
    else msg += "last written by step " + std::to_string(h->written_step[f]);
    msg += "; the state is at step " + std::to_string(h->state_step) +
           (h->written_step[f] == h->state_step && h->written_epoch[f] >= 0 ? " with prognostic fields overwritten since" : "") +
           " (take a step with write_diag / diag_last, or name the step: ebm_get_field_as_of)";
    return fail(EBM_ERR_STALE, msg);
}

// quantity index (ebm::MizQuantity / ClassicQuantity) of a public field id, -1 if the step kernels
// do not produce it (the hidden warm start T0 is not a solution variable)
inline int quantity_of(int model, int f) {
    if (model == EBM_MODEL_MIZ) {
        switch (f) {
            case EBM_F_Ei: return ebm::Q_Ei;
            case EBM_F_Ew: return ebm::Q_Ew;
            case EBM_F_h: return ebm::Q_h;
            case EBM_F_D: return ebm::Q_D;
            case EBM_F_phi: return ebm::Q_phi;
            case EBM_F_n: return ebm::Q_n;
            case EBM_F_E: return ebm::Q_E;
            case EBM_F_T: return ebm::Q_T;
            case EBM_F_Ti: return ebm::Q_Ti;
            case EBM_F_Tw: return ebm::Q_Tw;
            default: return -1;
        }
    }
    switch (f) {
        case EBM_F_E: return ebm::QC_E;
        case EBM_F_Tg: return ebm::QC_Tg;
        case EBM_F_T: return ebm::QC_T;
        case EBM_F_h: return ebm::QC_h;
        default: return -1;
    }
}

// what crosses the units
ebm::StepArgs base_args(const ebm_ctx *h);        // ebm_drive.hip: the launch arguments every step launch starts from
void invalidate_graph(ebm_ctx *h);                // ebm_drive.hip: drop the captured graph (it holds old argument values)
int ensure_natural(ebm_ctx *h);                   // ebm_fields.hip: un-permute the diagnostic fields if a step left them split
// ebm_fields.hip: THE rule of ebm_ctx::state_split — the prognostic fields into the layout their next user expects
hipError_t convert_state(ebm_ctx *h, bool split);
int set_state_layout(ebm_ctx *h, bool split);     // the same, with the error reported (EBM_ERR_HIP)
// ebm_fields.hip: the prognostic fields natural (set_state_layout(h, false)), after the diagnostic ones if asked (ensure_natural)
int natural_layout(ebm_ctx *h, bool diagnostics_too);
// ebm_fields.hip: the phi field current again in whatever layout the state has (ebm_ctx::phi_stored), for readers that take
// the fields as they lie — a one-step launch that loads phi, resampling, a change of the parameters
hipError_t restore_phi(ebm_ctx *h);
// Ei, h or phi are about to be written by somebody who is not a step kernel, or the parameters they are tied by change:
// phi is restored under the present ones, then the state no longer counts as consistent (ebm_ctx::phi_consistent)
int state_written_outside(ebm_ctx *h);
int get_copier(ebm_ctx *h);                       // ebm_fields.hip: the handle's pinned staging ring, created on first use

}  // namespace ebm_rt
