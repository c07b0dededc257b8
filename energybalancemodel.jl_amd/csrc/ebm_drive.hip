// Host runtime, the drivers (ebm_runtime.h lists the units): the launches of one step and their two chains, graph replay,
// fused ranges, and what is built on them: ebm_step, ebm_run, ebm_run_fused, ebm_run_series, ebm_integrate, ebm_equilibrate,
// ebm_run_until.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>

#include "ebm_runtime.h"
#include "ebm_savesol.h"

using namespace ebm_rt;

namespace ebm_rt {

ebm::StepArgs base_args(const ebm_ctx *h) {
    ebm::StepArgs a{};
    a.state = h->state.get(); a.fstride = h->fstride; a.geom = h->geom.get(); a.gstride = h->gstride;
    a.fcol = h->fcol.get(); a.fsched = h->fsched.get(); a.p = h->p_dev.get();
    a.noise = h->noise.rec.get(); a.nstate = h->noise.state.get(); a.nseq = h->noise.seq.get(); a.seed = h->noise.seed;
    a.counters = h->counters.get(); a.amask = h->amask.get();
    if (h->sets.n) {                 // per-column parameter sets (ebm_set_column_params)
        a.p = h->sets.p.get(); a.geom = h->sets.geom.get(); a.pset = h->sets.col.get();
        a.set_stride = (long long)ebm::G_COUNT * h->gstride;
    }
    a.pitch = (int)h->pitch; a.nlat = h->nlat; a.ncol = h->ncol;
    a.stamps = h->stamps.get();
    a.cols = h->active;
    a.prefetch = h->prefetch;
    a.nfused = 1;
    std::memset(a.var_of, -1, sizeof(a.var_of));
    return a;
}

// drop the captured graph: its kernel nodes hold the argument values of the time of capture
void invalidate_graph(ebm_ctx *h) { h->graph = ebm_ctx::Graph(); }

}  // namespace ebm_rt

namespace {

constexpr int kGraphSteps = 64;
constexpr int kFusedTable = 16384;     // per-step scalars resident on the device at a time (512 KiB)

// What a step launch of OutMode `mode` asks of the plan (ebm_plan.h): the handle's model and grid, and the book's two answers
// for this launch (step_derives_phi, step_elides_zero_lines).  capturing: into a graph (build_graph) — ebm_run asks with it
// again for a replay's bookkeeping, so the two cannot differ.  (The classic kernel decides about T, h at run time: write_diag.)
ebm::StepVariant step_variant(const ebm_ctx *h, int mode, bool capturing = false) {
    return {h->model == EBM_MODEL_MIZ ? ebm::STEP_MIZ : ebm::STEP_CLASSIC, h->grid, h->imex, mode,
            h->book.step_derives_phi(mode, capturing), h->book.step_elides_zero_lines(mode, capturing)};
}
// ... and whether this build has a kernel for it (the fused modes: "no fused-K kernel for this shape")
bool has_step_kernel(const ebm_ctx *h, int mode) { return ebm::has_step_kernel(h->cfg, step_variant(h, mode)); }
// The launches of one step: columns 0 .. ncol-1, or the entries 0 .. nactive-1 of the active list (ebm_equilibrate,
// ebm_run_until), as one chain or split in two halves; a chain with no columns is skipped.
int chain_count(const ebm_ctx *h, int *first_half) {
    const int n = h->active ? h->nactive : h->ncol;
    *first_half = h->split_col ? (h->active ? n / 2 : h->split_col) : n;
    return (*first_half > 0) + (n - *first_half > 0);
}
// ... as one chain of launches or as two (ebm_ctx::stream2)
hipError_t launch_chains(ebm_ctx *h, const ebm::StepArgs &a, const ebm::StepPlan &plan) {
    const int n = h->active ? h->nactive : h->ncol;
    if (!h->split_col) return ebm::launch_step_columns(a, plan, 0, n, main_stream(h));
    if (!h->forked) {            // the second chain starts after everything the handle's stream has been given so far
        hipError_t e = hipEventRecord(h->ev_fork.get(), h->stream.get());
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream2.get(), h->ev_fork.get(), 0);
        if (e != hipSuccess) return e;
        h->forked = true;
    }
    int half = 0;
    (void)chain_count(h, &half);
    hipError_t e = half > 0 ? ebm::launch_step_columns(a, plan, 0, half, h->stream.get()) : hipSuccess;
    if (e == hipSuccess && n > half) e = ebm::launch_step_columns(a, plan, half, n - half, h->stream2.get());
    return e;
}
// `nlaunch` launches of `plan` (one per launch chain each, chain_count) have been enqueued that take `nsteps` steps, the last of
// them global step `last_step`; wrote_diag: the last one stored the diagnostic fields.
void record_launches(ebm_ctx *h, const ebm::StepPlan &plan, long long nlaunch, long long nsteps, long long last_step, bool wrote_diag) {
    int half = 0;
    h->n_launches += nlaunch * chain_count(h, &half);
    h->n_steps += nsteps;
    h->clock = last_step + 1;
    h->book.steps(nsteps, last_step, wrote_diag, plan.stores_split, plan.phi_derived, !h->active, plan.zero_lines);
}
// What the runtime owes before an eliding launch, or a replay of captured ones, on flags that somebody may have made untrue
// (FieldBook::zero_flags_need_clear): all flags clear, on the handle's stream — after whatever disturbed them, before the launch.
hipError_t clear_untrusted_zero_flags(ebm_ctx *h) {
    if (!h->book.zero_flags_need_clear()) return hipSuccess;
    hipError_t e = hipMemsetAsync(ebm::zero_flag_words(h->amask.get(), h->ncol, h->cfg.threads), 0,
                                  sizeof(unsigned) * ebm::zero_flag_count(h->ncol, h->cfg.threads), main_stream(h));
    if (e == hipSuccess) h->book.zero_flags_cleared();
    return e;
}
// Every step launch of the library goes through here — a.nfused steps, the last of them global step `last_step` — so here the
// book is asked (ebm_fieldbook.h): a one-step MIZ launch reads and writes the prognostic fields pair-split, the fused-K and
// classic kernels the natural layout; a one-step launch that does not derive phi loads the field.  `capturing` (build_graph):
// nothing but the step launches is enqueued and the book hears nothing; ebm_run makes the state fit the captured kernels
// before a replay.
hipError_t launch_step(ebm_ctx *h, const ebm::StepArgs &a, int mode, long long last_step, bool capturing = false) {
    const ebm::StepPlan plan = ebm::plan_step(h->cfg, step_variant(h, mode, capturing));
    const bool one_step = !ebm::is_fused_mode(mode);
    if (!capturing) {
        if (one_step && !plan.phi_derived)
            if (hipError_t e = restore_phi(h); e != hipSuccess) return e;
        if (hipError_t e = convert_state(h, one_step); e != hipSuccess) return e;
        if (plan.zero_lines)                             // (after the conversion: it moves the lines)
            if (hipError_t e = clear_untrusted_zero_flags(h); e != hipSuccess) return e;
    }
    hipError_t e = launch_chains(h, a, plan);
    if (e == hipSuccess && !capturing) record_launches(h, plan, 1, a.nfused, last_step, a.write_diag != 0);
    return e;
}

// Capture kGraphSteps step kernels (node i reads graph.sched[i]) into a graph, once per handle.
int build_graph(ebm_ctx *h) {
    ebm_ctx::Graph g;
    HIPCHK(dev_alloc(g.sched, kGraphSteps));
    hipGraph_t graph = nullptr;
    int rc = set_state_layout(h, true);                  // never captured: the graph holds one-step launches only
    if (rc) return rc;
    HIPCHK(hipStreamBeginCapture(main_stream(h), hipStreamCaptureModeThreadLocal));
    hipError_t e = hipSuccess;
    for (int i = 0; i < kGraphSteps && e == hipSuccess; ++i) {
        ebm::StepArgs a = base_args(h);
        a.sched = g.sched.get();
        a.slot = i;
        a.write_diag = 0;
        e = launch_step(h, a, ebm::OUT_STATE, 0, true);  // the deriving kernel where the handle has it
    }
    hipError_t e2 = hipStreamEndCapture(main_stream(h), &graph);
    if (e != hipSuccess || e2 != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        return hip_fail("graph capture", e != hipSuccess ? e : e2);
    }
    e = hipGraphInstantiate(g.exec.out(), graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return hip_fail("hipGraphInstantiate", e);
    h->graph = std::move(g);
    return EBM_OK;
}

// model time of 0-based global step `step`: st.T[step+1] = (2 step + 1)/(2 nt), correctly rounded
double year_time(const ebm_ctx *h, long long step) {
    const double nt = (double)h->ttab.size();
    return nt > 0.0 ? (double)(2 * step + 1) / (2.0 * nt) : 0.0;
}

// per-step scalars of steps i = 0 .. n-1 into out[i]: time-table entry tab_first + i, model-time step clock_first + i and
// forcing f[i] (f null: 0)
void fill_sched(const ebm_ctx *h, long long tab_first, long long clock_first, int n, const double *f, ebm::StepSched *out) {
    const long long nt = (long long)h->ttab.size();
    for (int i = 0; i < n; ++i) {
        const long long ti = (tab_first + i) % nt;
        out[i].ct = h->ttab[ti];
        out[i].ct_next = h->ttab[(ti + 1) % nt];
        out[i].ft = f ? f[i] : 0.0;
        out[i].tyear = year_time(h, clock_first + i);
        out[i].n = clock_first + i;
    }
}

// savesol! fused into a step launch (ebm::OUT_SAVE): where the running sums and the raw snapshot go
struct SaveTarget {
    double *sums = nullptr;
    long long sum_stride = 0;
    double *stage = nullptr;
    long long stage_var_stride = 0, stage_offset = 0;
    signed char var_of[ebm::kMaxQuantities];
    // into a launch's arguments; a fused launch (OUT_LOOP_SAVE) takes the running sums only
    void put(ebm::StepArgs &a, bool sums_only) const {
        a.sums = sums; a.sum_stride = sum_stride;
        std::memcpy(a.var_of, var_of, sizeof(a.var_of));
        if (sums_only) return;
        a.stage = stage; a.stage_var_stride = stage_var_stride; a.stage_offset = stage_offset;
    }
};

int do_step(ebm_ctx *h, double ct, double ct_next, double f, int write_diag, long long step,
            const SaveTarget *save = nullptr) {
    ebm::StepArgs a = base_args(h);
    a.ct = ct; a.ct_next = ct_next; a.ft = f; a.write_diag = write_diag;
    a.tyear = year_time(h, step);
    a.step = step;
    if (save) save->put(a, false);
    hipError_t e = launch_step(h, a, save ? ebm::OUT_SAVE : write_diag ? ebm::OUT_DIAG : ebm::OUT_STATE, step);
    return e == hipSuccess ? EBM_OK : hip_fail("kernel launch", e);
}

// A caller's list of solution variables (ebm_run_series, ebm_integrate, ebm_equilibrate): each a field of this model, a
// quantity the step produces, not listed twice.  out[v] for v < nvars.
struct FieldRef {
    int field, slot, quantity;       // public id, state slot (slot_of), quantity index (quantity_of)
    bool diagnostic;
};
int resolve_fields(const ebm_ctx *h, const char *who, int nvars, const int *fields, FieldRef *out) {
    bool listed[EBM_F_COUNT] = {};
    for (int v = 0; v < nvars; ++v) {
        const int f = fields[v];
        if (!h->book.has(f) || quantity_of(h->model, f) < 0)
            return fail(EBM_ERR_ARG, std::string(who) + ": fields[" + std::to_string(v) + "] is not a solution variable of this model");
        if (listed[f]) return fail(EBM_ERR_ARG, std::string(who) + ": field " + field_name(f) + " is listed twice");
        listed[f] = true;
        out[v] = {f, slot_of(h->model, f), quantity_of(h->model, f), h->book.is_diagnostic(f)};
    }
    return EBM_OK;
}

// The active list of ebm_equilibrate and ebm_run_until: the columns that are still stepped, and the rounds that shorten it.
// A round is: activate, a fused_range over the list, the caller's check kernel — which writes round_of[c] and frozen[c] of
// every active column c — and, where the caller's rule says the list may have changed, advance.  The list is known to the
// launches only until the owner goes out of scope, on every path; they end before its buffers are freed (and before those
// that the caller declared before it).
struct ActiveRounds {
    int *cur = nullptr, *nxt = nullptr;      // [ncol] each: this round's list, ascending, and the one advance writes
    int *round_of = nullptr, *frozen = nullptr;   // [ncol]: the round that last tested the column (0: none); it froze it
    int *extra = nullptr;                    // [extra_ints_per_column][ncol], the caller's
    int nactive = 0;
    ~ActiveRounds() {
        if (!h) return;
        (void)hipStreamSynchronize(main_stream(h));
        h->active = nullptr;
        h->nactive = 0;
    }
    // every column active, none tested or frozen
    int begin(ebm_ctx *handle, int extra_ints_per_column) {
        h = handle;
        const size_t n = (size_t)(nactive = h->ncol);
        HIPCHK(dev_alloc(ints, (4 + (size_t)extra_ints_per_column) * n + 1));
        HIPCHK(hipHostMalloc(pinned.out(), sizeof(int), hipHostMallocDefault));
        cur = ints.get(); nxt = cur + n; round_of = nxt + n; frozen = round_of + n; extra = frozen + n;
        count = extra + (size_t)extra_ints_per_column * n;
        std::vector<int> ident(n);
        for (size_t c = 0; c < n; ++c) ident[c] = (int)c;
        HIPCHK(hipMemcpy(cur, ident.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(round_of, 0, sizeof(int) * n));
        HIPCHK(hipMemset(frozen, 0, sizeof(int) * n));
        return EBM_OK;
    }
    // the coming fused_range steps this round's list
    void activate() const { h->active = cur; h->nactive = nactive; }
    // The next list: compact_active_kernel drops the frozen columns, the host reads the new length (the round's one stream
    // synchronisation), and the list just written steps the next round.  Returns the new nactive, or an error (< 0).
    int advance(const char *who) {
        hipError_t e = ebm::launch_compact_active(cur, nactive, frozen, nxt, count, main_stream(h));
        if (e == hipSuccess) e = hipMemcpyAsync(pinned.get(), count, sizeof(int), hipMemcpyDeviceToHost, main_stream(h));
        if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
        if (e != hipSuccess) return hip_fail(std::string(who) + ": active list", e);
        std::swap(cur, nxt);
        return nactive = *pinned.get();
    }
    // after the last round: round_of and frozen of every column
    int download(int *round_out, int *frozen_out) const {
        HIPCHK(hipStreamSynchronize(main_stream(h)));
        HIPCHK(hipMemcpy(round_out, round_of, sizeof(int) * (size_t)h->ncol, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(frozen_out, frozen, sizeof(int) * (size_t)h->ncol, hipMemcpyDeviceToHost));
        return EBM_OK;
    }

private:
    ebm_ctx *h = nullptr;
    DevBuf<int> ints;
    PinnedBuf<int> pinned;
    int *count = nullptr;
};

}  // namespace

extern "C" {

int ebm_step(ebm_handle_t h, double cos2pit, double cos2pit_next, double f, int write_diag) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_step: null handle");
    HIPCHK(hipSetDevice(h->device));
    if (h->fsched && h->ttab.empty()) return fail(EBM_ERR_ARG, "ebm_step: column schedules need the time table (ebm_set_time_table)");
    return do_step(h, cos2pit, cos2pit_next, f, write_diag, h->clock);
}

int ebm_run(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int diag_last) {
    if (!h || nsteps < 0 || first_step < 0) return fail(EBM_ERR_ARG, "ebm_run: bad argument");
    if (h->ttab.empty()) return fail(EBM_ERR_ARG, "ebm_run: call ebm_set_time_table first");
    HIPCHK(hipSetDevice(h->device));
    const long long nt = (long long)h->ttab.size();
    int s = 0;
    if (h->use_graph && nsteps >= 2 * kGraphSteps) {
        // launch-bound shapes: replay a captured graph of kGraphSteps launches (still one launch
        // per step); the per-step scalars travel through a small device table
        int rc = h->graph.exec ? EBM_OK : build_graph(h);
        if (rc) return rc;
        if (h->book.replay_needs_a_direct_step() && nsteps > (diag_last ? 1 : 0)) {
            const long long ti = first_step % nt;
            if ((rc = do_step(h, h->ttab[ti], h->ttab[(ti + 1) % nt], f_steps ? f_steps[0] : 0.0, 0, first_step))) return rc;
            s = 1;
        }
        std::vector<ebm::StepSched> sched(kGraphSteps);
        const int last_graph_step = nsteps - (diag_last ? 1 : 0);     // a diagnostic last step is launched directly
        for (; s + kGraphSteps <= last_graph_step; s += kGraphSteps) {
            fill_sched(h, first_step + s, first_step + s, kGraphSteps, f_steps ? f_steps + s : nullptr, sched.data());
            // pageable source: the copy is staged before the call returns, so `sched` can be refilled
            HIPCHK(hipMemcpyAsync(h->graph.sched.get(), sched.data(), sizeof(ebm::StepSched) * kGraphSteps,
                                  hipMemcpyHostToDevice, main_stream(h)));
            if ((rc = set_state_layout(h, true))) return rc;       // the captured launches expect the one-step layout
            // ... and, where they elide zero lines, flags that are true (the direct step above took another kernel)
            const ebm::StepPlan captured = ebm::plan_step(h->cfg, step_variant(h, ebm::OUT_STATE, true));   // as build_graph's launch_step
            if (captured.zero_lines) HIPCHK(clear_untrusted_zero_flags(h));
            HIPCHK(hipGraphLaunch(h->graph.exec.get(), main_stream(h)));
            record_launches(h, captured, kGraphSteps, kGraphSteps, first_step + s + kGraphSteps - 1, false);
        }
    }
    for (; s < nsteps; ++s) {
        const long long ti = (first_step + s) % nt;
        const double f = f_steps ? f_steps[s] : 0.0;
        int rc = do_step(h, h->ttab[ti], h->ttab[(ti + 1) % nt], f, diag_last && s == nsteps - 1, first_step + s);
        if (rc) return rc;
    }
    return EBM_OK;
}

// nsteps steps, steps_per_launch to a launch, the per-step scalars from a device table: time-table entry tab_first + i and
// model-time step clock_first + i for step i.  save: savesol!'s running sums from every step (OUT_LOOP_SAVE), else plain
// fused stepping (OUT_LOOP).
static int fused_range(ebm_ctx *h, long long tab_first, long long clock_first, int nsteps, const double *f_steps, int diag_last,
                       int steps_per_launch, const SaveTarget *save) {
    // forcing noise: the kernels draw a launch's innovations one step per lane, so a launch takes at most kNoiseMaxFused
    // steps (same bits, more launches)
    if (h->noise.rec) steps_per_launch = std::min(steps_per_launch, ebm::kNoiseMaxFused);
    std::vector<ebm::StepSched> sched;
    for (int s0 = 0; s0 < nsteps; s0 += kFusedTable) {
        const int n = std::min(kFusedTable, nsteps - s0);
        sched.resize(n);
        fill_sched(h, tab_first + s0, clock_first + s0, n, f_steps ? f_steps + s0 : nullptr, sched.data());
        // the table used two batches ago: its launches must have ended before it is refilled (normally long since).  The copy is
        // synchronous for the host but not ordered with the handle's (non-blocking) streams.
        auto &tb = h->sched_tab[h->sched_next];
        h->sched_next ^= 1;
        if (!tb.dev) {
            ebm_ctx::SchedTable t;
            HIPCHK(dev_alloc(t.dev, kFusedTable));
            HIPCHK(hipEventCreateWithFlags(t.done.out(), hipEventDisableTiming));
            tb = std::move(t);
        }
        if (tb.in_use) HIPCHK(hipEventSynchronize(tb.done.get()));
        HIPCHK(hipMemcpy(tb.dev.get(), sched.data(), sizeof(ebm::StepSched) * (size_t)n, hipMemcpyHostToDevice));
        for (int i = 0; i < n; i += steps_per_launch) {
            ebm::StepArgs a = base_args(h);
            a.sched = tb.dev.get();
            a.slot = i;
            a.nfused = std::min(steps_per_launch, n - i);
            a.prefetch = 0;
            a.write_diag = (diag_last && s0 + i + a.nfused == nsteps) ? 1 : 0;
            if (save) save->put(a, true);
            hipError_t e = launch_step(h, a, save ? ebm::OUT_LOOP_SAVE : ebm::OUT_LOOP, clock_first + s0 + i + a.nfused - 1);
            if (e != hipSuccess) return hip_fail("fused launch", e);
        }
        HIPCHK(hipEventRecord(tb.done.get(), main_stream(h)));     // (both launch chains, joined)
        tb.in_use = true;
    }
    return EBM_OK;
}

int ebm_run_fused(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int diag_last,
                  int steps_per_launch) {
    if (!h || nsteps < 0 || first_step < 0 || steps_per_launch < 1) return fail(EBM_ERR_ARG, "ebm_run_fused: bad argument");
    if (h->ttab.empty()) return fail(EBM_ERR_ARG, "ebm_run_fused: call ebm_set_time_table first");
    // every shape has a fused-K kernel: the state in registers up to kFusedRegThreads threads per meridian (2048 cells at
    // 4 per thread; kFusedRegThreads2 at 2 per thread), resident in LDS for longer meridians and for the extension
    if (steps_per_launch == 1) return ebm_run(h, first_step, nsteps, f_steps, diag_last);
    HIPCHK(hipSetDevice(h->device));
    return fused_range(h, first_step, first_step, nsteps, f_steps, diag_last, steps_per_launch, nullptr);
}

// ebm_run_series and ebm_run_series_scalars (include/ebm_hip.h): ONE loop, the reduction passed in.  Every sample is the
// stepping of ebm_run_fused over `every` steps — so a launch never spans a sample — followed by one launch of the caller's
// reduction on the handle's stream (reduce(out, stride): row v of the sample at out + v * stride), which writes the sample's
// slot of the device series [nout][nsamples][ncol].  Nothing is synchronised between samples; the series comes down once, at
// the end.  series_call: the checks the two share, before anything of theirs.
static int series_call(const std::string &who, bool null_argument, long long first_step, int nsteps, int every, int steps_per_launch) {
    if (null_argument) return fail(EBM_ERR_ARG, who + ": null argument");
    if (nsteps < 0 || first_step < 0 || steps_per_launch < 1) return fail(EBM_ERR_ARG, who + ": bad argument");
    if (every < 1) return fail(EBM_ERR_ARG, who + ": every must be >= 1");
    if (nsteps % every) return fail(EBM_ERR_ARG, who + ": nsteps must be a multiple of every");
    return EBM_OK;
}
using SampleReduce = std::function<hipError_t(double *out, long long stride)>;
static int series_driver(ebm_ctx *h, const std::string &who, long long first_step, int nsteps, const double *f_steps, int every,
                         int steps_per_launch, int nout, int diag, const SampleReduce &reduce, double *series) {
    if (h->ttab.empty()) return fail(EBM_ERR_ARG, who + ": call ebm_set_time_table first");
    const int nsamples = nsteps / every;
    if (nsamples == 0) return EBM_OK;
    HIPCHK(hipSetDevice(h->device));
    int rc = get_copier(h);
    if (rc) return rc;
    const size_t per_var = (size_t)nsamples * (size_t)h->ncol;
    DevBuf<double> dev;
    HIPCHK(dev_alloc(dev, (size_t)nout * per_var));
    // the launches that write `dev` end before it is freed, on every path
    const auto done = finally([h] { (void)hipStreamSynchronize(main_stream(h)); });
    for (int j = 0; j < nsamples; ++j) {
        const long long first = first_step + (long long)j * every;
        const double *f = f_steps ? f_steps + (size_t)j * every : nullptr;
        rc = steps_per_launch == 1 ? ebm_run(h, first, every, f, diag)
                                   : fused_range(h, first, first, every, f, diag, steps_per_launch, nullptr);
        if (rc) return rc;
        // a one-launch-per-step diagnostic step at four cells per thread leaves the MIZ diagnostic fields pair-split, and the
        // prognostic ones too: the reduction reads the natural layout (two conversions per sample then)
        if ((rc = natural_layout(h, diag != 0))) return rc;
        hipError_t e = reduce(dev.get() + (size_t)j * (size_t)h->ncol, (long long)per_var);
        if (e != hipSuccess) return hip_fail(who + ": reduction", e);
    }
    HostCopier *c = h->copier.get();
    HIPCHK(c->wait_all());
    HIPCHK(c->order_after(main_stream(h)));
    CopyJob job;     // [nout * nsamples] packed rows of ncol doubles
    job.src = dev.get(); job.src_pitch = (size_t)h->ncol; job.row_elems = (size_t)h->ncol;
    job.nrows = (size_t)nout * (size_t)nsamples; job.dst = series;
    hipError_t e = c->run(job);
    if (e != hipSuccess) return hip_fail(who, e);
    return EBM_OK;
}

int ebm_run_series(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int every, int steps_per_launch,
                   int nvars, const int *fields, double *series) {
    if (int rc = series_call("ebm_run_series", !h || !fields || !series, first_step, nsteps, every, steps_per_launch)) return rc;
    if (nvars < 1 || nvars > ebm::kMaxQuantities) return fail(EBM_ERR_ARG, "ebm_run_series: bad number of fields");
    FieldRef vars[ebm::kMaxQuantities];
    int rc = resolve_fields(h, "ebm_run_series", nvars, fields, vars);
    if (rc) return rc;
    ebm::MeansArgs sa{};
    int diag = 0;
    for (int v = 0; v < nvars; ++v) {
        if (vars[v].diagnostic) diag = 1;
        sa.slot[v] = vars[v].slot;
    }
    sa.state = h->state.get(); sa.fstride = h->fstride;
    sa.x = x_table(h);
    sa.pitch = (int)h->pitch; sa.nlat = h->nlat; sa.nvars = nvars;
    return series_driver(h, "ebm_run_series", first_step, nsteps, f_steps, every, steps_per_launch, nvars, diag,
                         [&](double *out, long long stride) {
                             sa.out = out; sa.var_stride = stride;
                             return ebm::launch_hemispheric_means(sa, h->ncol, main_stream(h));
                         }, series);
}

// ... with the nscal column scalars of ebm_column_scalars for a sample (one launch of column_scalars_kernel)
int ebm_run_series_scalars(ebm_handle_t h, long long first_step, int nsteps, const double *f_steps, int every, int steps_per_launch,
                           int nscal, const int *spec, const double *level, double *series) {
    if (int rc = series_call("ebm_run_series_scalars", !h || !spec || !level || !series, first_step, nsteps, every, steps_per_launch))
        return rc;
    ScalarRef sc[ebm::kMaxQuantities];
    int rc = resolve_scalars(h, "ebm_run_series_scalars", nscal, spec, level, sc);
    if (rc) return rc;
    int diag = 0;
    for (int s = 0; s < nscal; ++s)
        if (sc[s].diagnostic) diag = 1;
    ebm::ScalarArgs a = scalar_args(h, nscal, sc);
    return series_driver(h, "ebm_run_series_scalars", first_step, nsteps, f_steps, every, steps_per_launch, nscal, diag,
                         [&](double *out, long long stride) {
                             a.out = out; a.out_stride = stride;
                             return ebm::launch_column_scalars(a, h->ncol, main_stream(h));
                         }, series);
}

// The outputs of one integrate call on their way to the host: the copier, views into the handle's buffers
// (ebm_ctx::integrate) and one method per action.  Host output never stalls the stepping: what has to leave the device is
// first copied device -> device into a buffer of its own on the compute stream (seasonal snapshots; the annual means come out
// of ONE finish-mean launch; raw snapshots are written by the step kernel into one half of the staging buffer), then the
// handle's copier moves it to the caller's arrays — DMA into the pinned ring on its own stream, host threads from there —
// while the following steps run.  A buffer is reused only after the job that reads it has finished.  When the owner goes out
// of scope, on every path, the copier finishes what it was given: it reads these buffers and writes the caller's arrays.
struct IntegrateOutputs {
    IntegrateOutputs(ebm_ctx *handle, const ebm::SaveConfig &c, int nv, const FieldRef *v)
        : h(handle), cp(handle->copier.get()), cfg(c), nvars(nv), vars(v), ncell((size_t)handle->ncol * handle->nlat),
          npitch((size_t)handle->ncol * handle->pitch) {}
    ~IntegrateOutputs() { (void)cp->wait_all(); }
    // The handle's buffers, grown to this call's needs; the running sums start from zero.
    int reserve(const ebm::RawStaging &staging, bool want_hm, bool want_snap) {
        ebm_ctx::Integrate &b = h->integrate;
        if (cfg.keep_raw) HIPCHK(b.stage.reserve(staging.total_elems()));
        if (want_hm) HIPCHK(b.hm.reserve((size_t)h->ncol * (size_t)nvars));
        if (cfg.want_sums) {
            HIPCHK(b.sums.reserve(npitch * (size_t)nvars));
            sums = b.sums.get();
            HIPCHK(restart_sums());
            HIPCHK(b.mean.reserve(npitch * (size_t)nvars));
        }
        if (want_snap) HIPCHK(b.snap.reserve(npitch * (size_t)nvars));
        mean = b.mean.get(); snap = b.snap.get(); hm = b.hm.get();
        stage = cfg.keep_raw ? b.stage.get() : nullptr;
        return EBM_OK;
    }
    hipError_t restart_sums() const { return hipMemsetAsync(sums, 0, sizeof(double) * npitch * (size_t)nvars, main_stream(h)); }
    // one asynchronous job per saved variable: [ncol][pitch] on the device -> packed [ncol][nlat], row (v, year) of dst_base
    hipError_t fields_out(double *dst_base, long long year, const double *dev_base) const {
        hipError_t e = cp->order_after(main_stream(h));
        for (int v = 0; v < nvars && e == hipSuccess; ++v) {
            CopyJob j;
            j.src = dev_base + (size_t)v * npitch; j.src_pitch = (size_t)h->pitch; j.row_elems = (size_t)h->nlat;
            j.nrows = (size_t)h->ncol; j.dst = dst_base + cfg.row(v, year) * ncell;
            cp->submit(j);
        }
        return e;
    }
    // seasonal snapshot: the state fields of this step, device -> device, then out
    hipError_t snapshot_out(double *dst_base, long long year) const {
        hipError_t e = cp->wait_all();                                       // the previous snapshot has left `snap`
        for (int v = 0; v < nvars && e == hipSuccess; ++v)
            e = hipMemcpyAsync(snap + (size_t)v * npitch, h->field[vars[v].field], sizeof(double) * npitch, hipMemcpyDeviceToDevice, main_stream(h));
        if (e == hipSuccess) e = fields_out(dst_base, year, snap);
        return e;
    }
    // hemispheric_mean (src/utilities.jl:397-403) of every saved variable of a padded device field set — the state fields
    // through their slots (from_mean false), or the [nvars][ncol*pitch] buffer of annual means — reduced on the device in one
    // launch, [nvars][ncol] -> out[v][year][col]
    hipError_t means_out(double *out, long long year, bool from_mean) const {
        ebm::MeansArgs m{};
        m.state = from_mean ? mean : h->state.get(); m.fstride = from_mean ? (long long)npitch : h->fstride;
        for (int v = 0; v < nvars; ++v) m.slot[v] = from_mean ? v : vars[v].slot;
        m.x = x_table(h); m.out = hm; m.var_stride = h->ncol;
        m.pitch = (int)h->pitch; m.nlat = h->nlat; m.nvars = nvars;
        hipError_t e = ebm::launch_hemispheric_means(m, h->ncol, main_stream(h));
        if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
        for (int v = 0; v < nvars && e == hipSuccess; ++v)
            e = hipMemcpy(out + cfg.row(v, year) * h->ncol, hm + (size_t)v * h->ncol, sizeof(double) * (size_t)h->ncol,
                          hipMemcpyDeviceToHost);
        return e;
    }
    // a year's end: ONE launch forms all means from the sums (and zeroes them)
    hipError_t annual_mean_out(double *avg, double *hm_avg, long long year) const {
        hipError_t e = cp->wait_all();                                       // last year's means have left `mean`
        if (e == hipSuccess)
            e = ebm::launch_finish_mean(mean, sums, (double)cfg.nt, h->ncol, nvars, (long long)npitch, h->cfg, main_stream(h));
        if (e == hipSuccess && avg) e = fields_out(avg, year, mean);
        if (e == hipSuccess && hm_avg) e = means_out(hm_avg, year, true);
        return e;
    }
    // the half just filled goes out while the steps fill the other one — whose previous contents must have left
    hipError_t flush_out(double *raw, const ebm::RawStaging &staging, const ebm::RawFlush &f) const {
        hipError_t e = cp->wait_all();
        if (e == hipSuccess) e = cp->order_after(main_stream(h));
        for (int v = 0; v < nvars && e == hipSuccess; ++v) {
            CopyJob j;      // `count` snapshots of ncol rows each: (count * ncol) rows of nlat doubles, pitch apart
            j.src = stage + staging.half_base_elems(f.half) + (size_t)v * staging.var_stride_elems();
            j.src_pitch = (size_t)h->pitch; j.row_elems = (size_t)h->nlat; j.nrows = (size_t)f.count * h->ncol;
            j.dst = raw + staging.dst_snapshot(f, v) * ncell;
            cp->submit(j);
        }
        return e;
    }

    ebm_ctx *const h;
    HostCopier *const cp;
    const ebm::SaveConfig &cfg;
    const int nvars;
    const FieldRef *const vars;
    const size_t ncell, npitch;      // packed cells per snapshot (host side); device elements per field
    double *sums = nullptr, *mean = nullptr, *snap = nullptr, *stage = nullptr, *hm = nullptr;
};
constexpr size_t kRawStageBytes = 128ull << 20;     // one half of the raw staging buffer, at most (and at least a snapshot)

// integrate + savesol! (ebm_integrate) with, optionally, the per-column hemispheric means of the seasonal outputs reduced on
// the device (ebm_integrate_hemispheric): hm_* are [nvars][dur][ncol] host arrays.  What every step owes, which stretches are
// fused and where a raw snapshot is staged is ebm_savesol.h's; here are the argument checks, the buffers, and one loop over
// the walk's items: the launches of the item, then what the item says, through IntegrateOutputs.
static int integrate_impl(ebm_handle_t h, int nt, int dur, const double *f_steps, int lastonly,
                          int winter_inx, int summer_inx, int nvars, const int *fields, double *raw,
                          double *winter, double *summer, double *avg, double *hm_winter, double *hm_summer,
                          double *hm_avg) {
    if (!h || nt < 1 || dur < 1 || nvars < 0 || nvars > ebm::kMaxQuantities || (nvars > 0 && !fields))
        return fail(EBM_ERR_ARG, "ebm_integrate: bad argument");
    if ((hm_winter || hm_summer || hm_avg) && nvars < 1) return fail(EBM_ERR_ARG, "ebm_integrate_hemispheric: no variables");
    if ((long long)h->ttab.size() != nt) return fail(EBM_ERR_ARG, "ebm_integrate: time table length must equal nt");
    FieldRef vars[ebm::kMaxQuantities];
    int rc = resolve_fields(h, "ebm_integrate", nvars, fields, vars);
    if (rc) return rc;
    SaveTarget save;
    std::memset(save.var_of, -1, sizeof(save.var_of));
    for (int v = 0; v < nvars; ++v) save.var_of[vars[v].quantity] = (signed char)v;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = get_copier(h))) return rc;
    HIPCHK(h->copier->wait_all());
    ebm::SaveConfig cfg{nt, dur, lastonly != 0, winter_inx, summer_inx};
    cfg.keep_raw = raw && nvars > 0;
    cfg.want_winter = winter || hm_winter;
    cfg.want_summer = summer || hm_summer;
    cfg.want_sums = (avg || hm_avg) && nvars > 0;
    // Stretches that need nothing but the running sums are fused, integrate_spl steps to a launch, with the state resident on
    // the chip (miz_resident_kernel<SAVE>, miz_fused_kernel<2, ..., SAVE>; plain fused stepping when no mean is asked for): MIZ
    // and MIZ_IMEX, every geometry but two cells per thread at 768 threads.
    cfg.may_fuse = h->integrate_spl > 1 && h->model == EBM_MODEL_MIZ && (!cfg.want_sums || has_step_kernel(h, ebm::OUT_LOOP_SAVE));
    IntegrateOutputs out(h, cfg, nvars, vars);
    ebm::RawStaging staging;
    if (cfg.keep_raw) staging = ebm::RawStaging(kRawStageBytes, out.npitch, nvars, cfg.nraw());
    if ((rc = out.reserve(staging, (hm_winter || hm_summer || hm_avg) && nvars > 0, (winter || summer) && nvars > 0))) return rc;
    save.sums = out.sums;
    save.sum_stride = (long long)out.npitch;
    save.stage_var_stride = (long long)staging.var_stride_elems();
    double *const season_fields[] = {nullptr, winter, summer}, *const season_means[] = {nullptr, hm_winter, hm_summer};
    const long long clock0 = h->clock;    // model time continues from the handle's step clock (0 after ebm_create)
    ebm::SaveWalk walk(cfg);
    ebm::RawFlush full;
    for (ebm::SaveItem it; walk.next(it);) {
        const double *const f = f_steps ? f_steps + it.first : nullptr;
        if (it.n > 1) {
            rc = fused_range(h, it.first, clock0 + it.first, (int)it.n, f, 0, h->integrate_spl, it.sums ? &save : nullptr);
            if (rc) return rc;
            continue;
        }
        // savesol! from the step kernel's registers: the annual-mean sums on every step, the raw snapshot on the steps that
        // are kept; the diagnostic FIELDS are only stored on steps whose snapshot is copied out of them (seasons) and on
        // the last one
        const ebm::SaveStep &s = it.step;
        const bool kept = s.raw_index >= 0;
        const ebm::RawSlot slot = staging.slot();
        save.stage = kept ? out.stage + staging.half_base_elems(slot.half) : nullptr;
        save.stage_offset = (long long)staging.slot_elems(slot);
        rc = do_step(h, h->ttab[s.tab], h->ttab[s.tab_next], f ? *f : 0.0, s.diag() ? 1 : 0, clock0 + it.first,
                     (it.sums || kept) ? &save : nullptr);
        if (rc) return rc;
        if (kept && staging.kept(full)) HIPCHK(out.flush_out(raw, staging, full));
        if (s.snapshot && (rc = natural_layout(h, true))) return rc;
        if (season_fields[s.season]) HIPCHK(out.snapshot_out(season_fields[s.season], s.year));
        if (season_means[s.season]) HIPCHK(out.means_out(season_means[s.season], s.year, false));
        if (s.mean) HIPCHK(out.annual_mean_out(avg, hm_avg, s.year));
        if (s.restart) HIPCHK(out.restart_sums());
    }
    if (staging.flush(full)) HIPCHK(out.flush_out(raw, staging, full));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    HIPCHK(h->copier->wait_all());
    return EBM_OK;
}

int ebm_integrate(ebm_handle_t h, int nt, int dur, const double *f_steps, int lastonly,
                  int winter_inx, int summer_inx, int nvars, const int *fields, double *raw,
                  double *winter, double *summer, double *avg) {
    return integrate_impl(h, nt, dur, f_steps, lastonly, winter_inx, summer_inx, nvars, fields, raw, winter, summer, avg,
                          nullptr, nullptr, nullptr);
}

int ebm_integrate_hemispheric(ebm_handle_t h, int nt, int dur, const double *f_steps, int winter_inx, int summer_inx,
                              int nvars, const int *fields, double *hm_winter, double *hm_summer, double *hm_avg) {
    if (!hm_winter && !hm_summer && !hm_avg) return fail(EBM_ERR_ARG, "ebm_integrate_hemispheric: no output requested");
    return integrate_impl(h, nt, dur, f_steps, 1, winter_inx, summer_inx, nvars, fields, nullptr, nullptr, nullptr, nullptr,
                          hm_winter, hm_summer, hm_avg);
}

// ebm_equilibrate (include/ebm_hip.h).  Every year is one fused_range over the active columns (launches of nactive
// workgroups, which step cols[b]), then equilibrium_check_kernel compares each active column's year-end fields with the
// snapshot of the year before and freezes it, and the list advances (ActiveRounds): one stream synchronisation per year.  The fused kernels store the diagnostic fields in the natural
// layout, so the fields of columns frozen in different years share one layout and nothing is un-permuted in between.
int ebm_equilibrate(ebm_handle_t h, int nt, int max_years, int min_years, const double *f_year, int nvars, const int *fields,
                    const double *tol, int *years, int *converged, double *resid) {
    if (!h || nt < 1 || nvars < 1 || !fields || !tol || !years || !converged) return fail(EBM_ERR_ARG, "ebm_equilibrate: bad argument");
    if (h->fsched)
        return fail(EBM_ERR_UNSUPPORTED, "ebm_equilibrate: per-column forcing schedules are installed (a ramped forcing has no "
                                         "equilibrium; ebm_set_column_schedule(h, NULL) clears them)");
    if (h->noise.rec)
        return fail(EBM_ERR_UNSUPPORTED, "ebm_equilibrate: forcing noise is installed (a noisy member has no repeating cycle; "
                                         "ebm_set_column_noise(h, NULL, ...) clears it)");
    if ((long long)h->ttab.size() != nt) return fail(EBM_ERR_ARG, "ebm_equilibrate: time table length must equal nt");
    if (max_years < 1) return fail(EBM_ERR_ARG, "ebm_equilibrate: max_years must be >= 1");
    if (nvars > ebm::kMaxQuantities) return fail(EBM_ERR_ARG, "ebm_equilibrate: too many fields");
    FieldRef vars[ebm::kMaxQuantities];
    int rc = resolve_fields(h, "ebm_equilibrate", nvars, fields, vars);
    if (rc) return rc;
    ebm::EquilArgs ea{};
    for (int v = 0; v < nvars; ++v) {
        if (!(tol[v] >= 0.0))
            return fail(EBM_ERR_ARG, std::string("ebm_equilibrate: the tolerance of ") + field_name(vars[v].field) + " must be >= 0 (not NaN)");
        ea.slot[v] = vars[v].slot;
        ea.tol[v] = tol[v];
    }
    if (!has_step_kernel(h, ebm::OUT_LOOP))
        return fail(EBM_ERR_UNSUPPORTED, "ebm_equilibrate: no fused-K kernel for this shape in this build");
    HIPCHK(hipSetDevice(h->device));
    if ((rc = natural_layout(h, true))) return rc;
    const int ncol = h->ncol;
    const size_t npitch = (size_t)ncol * h->pitch;
    // this call's device memory: snapshot | resid, and the active list with the year each column was last tested in
    DevBuf<double> dbl;
    ActiveRounds rounds;
    HIPCHK(dev_alloc(dbl, (size_t)nvars * npitch + (size_t)nvars * ncol));
    if ((rc = rounds.begin(h, 0))) return rc;
    {
        std::vector<double> nan((size_t)nvars * ncol, std::nan(""));
        HIPCHK(hipMemcpy(dbl.get() + (size_t)nvars * npitch, nan.data(), sizeof(double) * nan.size(), hipMemcpyHostToDevice));
    }
    ea.state = h->state.get(); ea.fstride = h->fstride;
    ea.snap = dbl.get(); ea.resid = dbl.get() + (size_t)nvars * npitch;
    ea.years = rounds.round_of; ea.frozen = rounds.frozen;
    ea.pitch = (int)h->pitch; ea.nlat = h->nlat; ea.ncol = ncol; ea.nvars = nvars;
    const long long clock0 = h->clock;
    const int first_test = std::max(2, min_years);
    for (int y = 1; y <= max_years; ++y) {
        rounds.activate();
        rc = fused_range(h, 0, clock0 + (long long)(y - 1) * nt, nt, f_year, 1, h->integrate_spl, nullptr);
        if (rc) return rc;
        ea.cols = rounds.cur;
        ea.year = y;
        ea.compare = y >= 2;
        ea.may_freeze = y >= first_test;
        hipError_t e = ebm::launch_equilibrium_check(ea, rounds.nactive, main_stream(h));
        if (e != hipSuccess) return hip_fail("ebm_equilibrate: check", e);
        if (y == max_years || !ea.may_freeze) continue;          // (nothing has frozen: the list stays)
        if ((rc = rounds.advance("ebm_equilibrate")) < 0) return rc;
        if (rc == 0) break;                                      // every column is frozen
    }
    if ((rc = rounds.download(years, converged))) return rc;
    if (resid) HIPCHK(hipMemcpy(resid, ea.resid, sizeof(double) * (size_t)nvars * ncol, hipMemcpyDeviceToHost));
    return EBM_OK;
}

// ebm_run_until (include/ebm_hip.h).  Every round is one fused_range of `every` steps over the active columns — also with
// one step per launch: the one-step kernels and a replayed graph know nothing of the list, the fused kernel at K = 1 gives
// the same bits — then passage_check_kernel takes each active column's mean and compares it with the column's level, and
// the list advances (ActiveRounds): one stream synchronisation per round.  The fused kernels read and write the natural layout, so the fields of columns frozen in different rounds
// share one layout.
// (the two entry points below share until_call — the checks before the field's own — and until_driver, the rounds: `var` the
// field, pa.scalar .. pa.edge_level the sample the check takes of it)
static int until_call(const std::string &who, bool null_argument, long long first_step, int max_samples, int every, int steps_per_launch) {
    if (null_argument) return fail(EBM_ERR_ARG, who + ": null argument");
    if (every < 1 || max_samples < 1) return fail(EBM_ERR_ARG, who + ": every and max_samples must be >= 1");
    if (steps_per_launch < 1 || first_step < 0) return fail(EBM_ERR_ARG, who + ": bad argument");
    return EBM_OK;
}
static int until_driver(ebm_ctx *h, const std::string &who, long long first_step, int max_samples, int every, const double *f_steps,
                        int steps_per_launch, int field, bool diagnostic, ebm::PassageArgs pa, const double *level, const int *direction,
                        int *samples, int *crossed, double *value) {
    int rc = EBM_OK;
    const int ncol = h->ncol;
    for (int c = 0; c < ncol; ++c) {
        if (level[c] != level[c]) return fail(EBM_ERR_ARG, who + ": level[" + std::to_string(c) + "] is NaN");
        if (direction[c] == 0)
            return fail(EBM_ERR_ARG, who + ": direction[" + std::to_string(c) + "] is 0 (> 0: upward, < 0: downward)");
    }
    if (h->ttab.empty()) return fail(EBM_ERR_ARG, who + ": call ebm_set_time_table first");
    if (!has_step_kernel(h, ebm::OUT_LOOP))
        return fail(EBM_ERR_UNSUPPORTED, who + ": no fused-K kernel for this shape in this build");
    HIPCHK(hipSetDevice(h->device));
    if ((rc = natural_layout(h, true))) return rc;
    const int diag = diagnostic ? 1 : 0;
    // this call's device memory: value | level, and the active list with the round each column was last tested in and, as
    // its extra array, the directions
    DevBuf<double> dbl;
    ActiveRounds rounds;
    HIPCHK(dev_alloc(dbl, 2 * (size_t)ncol));
    if ((rc = rounds.begin(h, 1))) return rc;
    double *value_dev = dbl.get(), *level_dev = value_dev + ncol;
    // (value needs no initial contents: round 1 tests every column)
    HIPCHK(hipMemcpy(level_dev, level, sizeof(double) * (size_t)ncol, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(rounds.extra, direction, sizeof(int) * (size_t)ncol, hipMemcpyHostToDevice));
    pa.field = h->field[field];
    pa.x = x_table(h);
    pa.level = level_dev; pa.direction = rounds.extra;
    pa.value = value_dev; pa.samples = rounds.round_of; pa.frozen = rounds.frozen;
    pa.pitch = (int)h->pitch; pa.nlat = h->nlat;
    for (int j = 1; j <= max_samples; ++j) {
        rounds.activate();
        const long long first = first_step + (long long)(j - 1) * every;
        rc = fused_range(h, first, first, every, f_steps ? f_steps + (size_t)(j - 1) * (size_t)every : nullptr, diag, steps_per_launch,
                         nullptr);
        if (rc) return rc;
        // (as ebm_run_series before its reduction; after a fused launch both hold already)
        if ((rc = natural_layout(h, diag != 0))) return rc;
        pa.cols = rounds.cur;
        pa.round = j;
        hipError_t e = ebm::launch_passage_check(pa, rounds.nactive, main_stream(h));
        if (e != hipSuccess) return hip_fail(who + ": check", e);
        if (j == max_samples) break;                             // (no further round: no list is needed)
        if ((rc = rounds.advance(who.c_str())) < 0) return rc;
        if (rc == 0) break;                                      // every column has crossed
    }
    if ((rc = rounds.download(samples, crossed))) return rc;
    if (value) HIPCHK(hipMemcpy(value, value_dev, sizeof(double) * (size_t)ncol, hipMemcpyDeviceToHost));
    return EBM_OK;
}

int ebm_run_until(ebm_handle_t h, long long first_step, int max_samples, int every, const double *f_steps, int steps_per_launch,
                  int field, const double *level, const int *direction, int *samples, int *crossed, double *value) {
    if (int rc = until_call("ebm_run_until", !h || !level || !direction || !samples || !crossed, first_step, max_samples, every, steps_per_launch))
        return rc;
    FieldRef var;
    if (int rc = resolve_fields(h, "ebm_run_until", 1, &field, &var)) return rc;
    return until_driver(h, "ebm_run_until", first_step, max_samples, every, f_steps, steps_per_launch, var.field, var.diagnostic,
                        ebm::PassageArgs{}, level, direction, samples, crossed, value);
}

// ... with m_c the column scalar spec[4], scalar_level of ebm_column_scalars (passage_scalar_kernel takes it)
int ebm_run_until_scalar(ebm_handle_t h, long long first_step, int max_samples, int every, const double *f_steps, int steps_per_launch,
                         const int *spec, double scalar_level, const double *level, const int *direction, int *samples, int *crossed,
                         double *value) {
    if (int rc = until_call("ebm_run_until_scalar", !h || !spec || !level || !direction || !samples || !crossed, first_step, max_samples, every,
                            steps_per_launch))
        return rc;
    ScalarRef sc;
    if (int rc = resolve_scalars(h, "ebm_run_until_scalar", 1, spec, &scalar_level, &sc)) return rc;
    ebm::PassageArgs pa{};
    pa.scalar = 1; pa.kind = sc.kind; pa.k0 = sc.k0; pa.k1 = sc.k1; pa.edge_level = sc.level;
    return until_driver(h, "ebm_run_until_scalar", first_step, max_samples, every, f_steps, steps_per_launch, sc.field, sc.diagnostic, pa,
                        level, direction, samples, crossed, value);
}

}  // extern "C"
