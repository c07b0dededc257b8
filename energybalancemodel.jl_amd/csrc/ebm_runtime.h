// Shared by the four translation units of the host runtime behind the C ABI of include/ebm_hip.h: the handle, the error
// idioms and the handle's stream.
//   ebm_fieldbook.h   (HIP-free) the field predicates and THE rule of field validity, layout and phi: ebm_ctx::book
//   ebm_plan.h        (HIP-free) the launch geometry and THE rule of a step launch's kernel, LDS and noise source: plan_step
//   ebm_savesol.h     (HIP-free) THE rule of savesol!: what every step of an integrate owes its outputs, which stretches are
//                     fused, and where a raw snapshot lies in the staging buffer: SaveWalk, RawStaging
//   ebm_runtime.hip   errors, options, create / destroy, sync, counters, timers, stamps, self-test, launch info
//   ebm_fields.hip    field I/O with the validity bookkeeping, device views, hemispheric means, the one host path of the three
//                     ensemble reductions (ebm_ensemble.hip) and of the column misfits (ebm_misfit.hip), the ensemble
//                     Kalman update (ebm_update.hip), the two diffusion operators
//   ebm_columns.hip   per-column forcing, schedules, noise and parameter sets; the step clock and the time table; resampling
//   ebm_drive.hip     step launches, graph replay, fused ranges, series, integrate, equilibrate, run-until
// Not part of the public interface.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "../../include/ebm_hip.h"
#include "ebm_fieldbook.h"
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
    // Which fields are current, which layout device memory holds, whether phi lies in it: every reader and writer of a field
    // asks the book first and reports to it afterwards (ebm_fieldbook.h; nothing else of the handle holds any of that)
    ebm_rt::FieldBook book;
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
    // staging rows of a handle that has no `scratch` (ebm_update_columns stages its innovations in the same rows: calls on one
    // stream, one after the other)
    struct Resample {
        PinnedBuf<int> host;
        size_t host_cap = 0;                       // pairs
        DevVec<int> dev;
        DevVec<double> stage;
        Event uploaded;
        bool in_flight = false;
    } resample;
    // ebm_ensemble_sums, ebm_ensemble_range and ebm_ensemble_histogram, kept between calls (a call is synchronous, so the
    // three share them): the block partials, the uploaded weights, centers ([12][pitch], padding zero) and edges
    // ([12][lo, hi, s][pitch], natural order), and the result of the host variants, sized for the largest
    struct Ensemble {
        DevVec<double> partial, w, center, edges, out;
    } ensemble;
    // ebm_ensemble_covariance, kept between calls: the block partials ([nblocks][pitch][pitch]), the two uploaded centers
    // ([2][pitch], natural order, padding zero) and the result of the host variant ([nlat][nlat]); the weights are ensemble.w
    struct Covariance {
        DevVec<double> partial, center, out;
    } covariance;
    // ebm_column_misfits, kept between calls: the uploaded targets ([8][12][pitch]) and rw ([12][pitch]), natural order,
    // padding zero, and the result of the host variant ([8][2][ncol])
    struct Misfit {
        DevVec<double> target, rw, out;
    } misfit;
    // ebm_update_columns, kept between calls: one field's gain ([pitch][pitch], host variant) and the uploaded target ([pitch]).
    // The staged innovations are not its own: they lie in `scratch` or, where the handle has none, in resample.stage
    struct Update {
        DevVec<double> gain, target;
    } update;
    // ebm_spd_solve_device and ebm_kalman_gain_device, kept between calls: the inverses of the diagonal blocks of L
    // ([mp / 64][64][64]) and words[0], the bad-pivot flag; for the gain also the compacted system S ([mp][mp]) and B
    // ([nvars * nlat][mp]), the uploaded obs_var ([nlat]) and, behind the flag, the observed cells ([mp]) and their inverse
    // map ([nlat]), and five events around the four phases of the last gain.  mp = the observed cells rounded up to 64
    struct Gain {
        DevVec<double> inv, S, B, obs_var;
        DevVec<int> words;
        Event mark[5];                             // around assembly, factor, solve, scatter of the last gain (ebm_kalman_gain_phases)
        bool timed = false;
    } gain;
    DevVec<double> scalars_out;                  // ebm_column_scalars: the result of the host variant ([12][ncol]), kept between calls
    // ebm_integrate's device buffers, kept between calls while the shape stays the same: the annual-mean sums
    // [var][ncol*pitch] (pair-split layout), the means and the seasonal snapshots [var][ncol*pitch] in the natural layout, the
    // raw snapshots staged as two halves of [var][chunk][ncol][pitch] (ebm::RawStaging), the hemispheric means [var][ncol]
    struct Integrate {
        DevVec<double> sums, mean, snap, stage, hm;
    } integrate;
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

// EBM_OK if `f` may be read now, else EBM_ERR_STALE with the two steps in the message
inline int check_current(const ebm_ctx *h, int f, const char *who) {
    const FieldBook &b = h->book;
    if (b.is_current(f)) return EBM_OK;
    std::string msg = std::string(who) + ": field " + field_name(f) + " is stale — ";
    if (b.never_written(f)) msg += "it has never been written";
    else if (b.written_step(f) < 0) msg += "it holds what it held before the first step";
    else msg += "last written by step " + std::to_string(b.written_step(f));
    msg += "; the state is at step " + std::to_string(b.state_step()) +
           (!b.never_written(f) && b.written_step(f) == b.state_step() ? " with prognostic fields overwritten since" : "") +
           " (take a step with write_diag / diag_last, or name the step: ebm_get_field_as_of)";
    return fail(EBM_ERR_STALE, msg);
}

// what crosses the units
ebm::StepArgs base_args(const ebm_ctx *h);        // ebm_drive.hip: the launch arguments every step launch starts from
void invalidate_graph(ebm_ctx *h);                // ebm_drive.hip: drop the captured graph (it holds old argument values)
// ebm_fields.hip, the executors of the book's passes (FieldBook, ebm_fieldbook.h): each asks the book, launches the pass it
// names on the handle's stream and reports it done
int ensure_natural(ebm_ctx *h);                   // the diagnostic fields natural
hipError_t convert_state(ebm_ctx *h, bool split); // the prognostic fields in the layout their next user expects
int set_state_layout(ebm_ctx *h, bool split);     // the same, with the error reported (EBM_ERR_HIP)
int natural_layout(ebm_ctx *h, bool diagnostics_too);   // the prognostic fields natural, after the diagnostic ones if asked
// phi current where it lies, for readers that take the fields as they lie: a one-step launch that loads phi, resampling, export
hipError_t restore_phi(ebm_ctx *h);
int state_written_outside(ebm_ctx *h);            // restore_phi, then FieldBook::state_written_outside
int get_copier(ebm_ctx *h);                       // ebm_fields.hip: the handle's pinned staging ring, created on first use
// A caller's column scalars (ebm_column_scalars, ebm_run_series_scalars, ebm_run_until_scalar; ebm_fields.hip): spec[nscal][4]
// and level[nscal] checked by the rules of include/ebm_hip.h — the message names the first offending scalar — into out[s]
struct ScalarRef {
    int field, kind, k0, k1;
    double level;
    bool diagnostic;
};
int resolve_scalars(const ebm_ctx *h, const char *who, int nscal, const int *spec, const double *level, ScalarRef *out);
// ... and as launch arguments: the rows where they lie (natural layout: the caller's duty), the bands, x
ebm::ScalarArgs scalar_args(const ebm_ctx *h, int nscal, const ScalarRef *sc);

}  // namespace ebm_rt
