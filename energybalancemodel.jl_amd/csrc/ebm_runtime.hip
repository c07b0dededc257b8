// Host runtime behind the C ABI of include/ebm_hip.h, first of four units (ebm_runtime.h lists them): the last error, the
// options, handle creation and destruction, synchronisation, counters and HIP-event timing.  Device work is in the kernel
// .hip files of this directory (ebm_launch.hip lists the kernels).  There is deliberately no CPU fallback: without a GPU
// every entry point fails with EBM_ERR_NO_DEVICE.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "ebm_runtime.h"
#include "ebm_tables.h"

using namespace ebm_rt;

thread_local std::string ebm_rt::g_err;

// The handle's work ends before anything is freed: the copier's worker finishes its queued jobs (they read the handle's
// buffers) and is joined; then every member frees what it owns.
ebm_ctx::~ebm_ctx() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(main_stream(this));
    copier.reset();
}

namespace {

// options: the defaults, overwritten by as many fields as the caller's struct has (no environment is read)
int read_options(const ebm_options *user_opt, ebm_options &opt) {
    (void)ebm_options_default(&opt);
    if (user_opt) {
        if (user_opt->struct_bytes < (int)sizeof(int) || user_opt->struct_bytes > 4096)
            return fail(EBM_ERR_ARG, "ebm_create_ex: options.struct_bytes must be sizeof(ebm_options)");
        std::memcpy(&opt, user_opt, std::min((size_t)user_opt->struct_bytes, sizeof(opt)));
        opt.struct_bytes = (int)sizeof(opt);
    }
    if (opt.cells_per_thread != 0 && opt.cells_per_thread != 2 && opt.cells_per_thread != 4)
        return fail(EBM_ERR_ARG, "ebm_create_ex: cells_per_thread must be 0 (default), 2 or 4");
    if (opt.use_graph < -1 || opt.use_graph > 1) return fail(EBM_ERR_ARG, "ebm_create_ex: use_graph must be -1, 0 or 1");
    if (opt.prefetch_cols < -1) return fail(EBM_ERR_ARG, "ebm_create_ex: prefetch_cols must be -1 (default), 0 or a distance");
    if (opt.launch_chains != -1 && opt.launch_chains != 1 && opt.launch_chains != 2)
        return fail(EBM_ERR_ARG, "ebm_create_ex: launch_chains must be -1 (default), 1 or 2");
    if (opt.fused_state_in_lds < -1 || opt.fused_state_in_lds > 1)
        return fail(EBM_ERR_ARG, "ebm_create_ex: fused_state_in_lds must be -1 (default), 0 or 1");
    if (opt.elide_zero_lines < -1 || opt.elide_zero_lines > 1)
        return fail(EBM_ERR_ARG, "ebm_create_ex: elide_zero_lines must be -1 (default), 0 or 1");
    if (opt.integrate_steps_per_launch < -1)
        return fail(EBM_ERR_ARG, "ebm_create_ex: integrate_steps_per_launch must be -1 (default), 1 or a number of steps");
    return EBM_OK;
}

// What the options leave to the library, from the shape (h->nlat, ncol, cfg) and the device (num_cus).  No choice changes a bit.
// dynamic LDS of a one-step launch of the geometry (the MIZ step's, whatever the model: what ebm_launch_info has always reported)
size_t one_step_lds_bytes(const ebm::LaunchCfg &cfg) {
    return ebm::plan_step(cfg, {ebm::STEP_MIZ, 0, false, ebm::OUT_STATE, false, false}).lds_bytes;
}

void choose_heuristics(ebm_ctx *h, const ebm_options &opt) {
    const int nlat = h->nlat, ncol = h->ncol;
    const ebm::LaunchCfg &cfg = h->cfg;
    h->integrate_spl = opt.integrate_steps_per_launch <= 0 ? 64 : opt.integrate_steps_per_launch;
    // more columns than the register kernel runs in one round (it holds one 256-thread workgroup per CU, four of 64 threads:
    // tests/tools/r3/fused_choice_sweep.py): from there on occupancy beats latency.  The choice changes no bit.
    h->cfg.fused_in_lds = opt.fused_state_in_lds >= 0 ? opt.fused_state_in_lds != 0
                                                      : ncol > h->num_cus * std::max(1, 256 / h->cfg.threads);
    // a step of fewer than ~256K cells is launch-bound: replay graphs in ebm_run
    h->use_graph = opt.use_graph >= 0 ? opt.use_graph != 0 : ((long long)nlat * ncol <= 262144);
    {
        // One or two workgroups per CU (a long meridian fills the CU's LDS): little or nothing
        // overlaps the input loads of a workgroup, so each workgroup prefetches into L2 the inputs
        // of the one that follows it on its XCD (workgroups go round-robin over the XCDs and in
        // order within one).
        int per_cu = (int)((160u * 1024u) / one_step_lds_bytes(cfg));         // workgroups a CU holds: LDS ...
        if (per_cu > 2048 / cfg.threads) per_cu = 2048 / cfg.threads;         // ... and wave slots
        const int ahead = h->num_cus * per_cu;                                // the successor on the same XCD
        // measured: -3.5 % time at one workgroup per CU, -2.5 % at two, nothing beyond
        h->prefetch = opt.prefetch_cols >= 0 ? opt.prefetch_cols : (per_cu <= 2 && ncol > ahead ? ahead : 0);
        // two chains of launches (see ebm_ctx::stream2): on request only — the default stays one launch per step, whose
        // duration a profiler reports as such; never with graph replay (one captured stream)
        h->split_col = (opt.launch_chains == 2 && !h->use_graph && ncol >= 2) ? ncol / 2 : 0;
    }
}

// Everything the new handle owns on its device: tables, zeroed state, parameter block, counters, streams and events.
int allocate(ebm_ctx *h, const double *x) {
    const int model = h->model, ncol = h->ncol;
    h->xhost.assign(x, x + h->nlat);
    h->gstride = h->pitch;
    std::vector<double> slab((size_t)ebm::G_COUNT * h->gstride, 0.0);
    ebm_tables::build_tables(model, h->grid, h->nlat, h->gstride, h->dt, h->p, x, slab.data());
    hipError_t e = dev_alloc(h->geom, slab.size());
    if (e == hipSuccess) e = hipMemcpy(h->geom.get(), slab.data(), sizeof(double) * slab.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("ebm_create: tables", e);
    h->fstride = (long long)ncol * h->pitch;
    h->nslots = (model == EBM_MODEL_MIZ) ? (int)ebm::S_MIZ_COUNT : (int)ebm::C_COUNT;
    const size_t nbytes = sizeof(double) * (size_t)h->nslots * (size_t)h->fstride;
    e = dev_alloc(h->state, (size_t)h->nslots * (size_t)h->fstride);
    if (e == hipSuccess) e = hipMemset(h->state.get(), 0, nbytes);
    if (e == hipSuccess && model == EBM_MODEL_MIZ) {
        // the mask rows, and behind them the zero-line flag words (ebm::zero_flag_words): all clear
        const size_t mn = (size_t)ncol * h->cfg.threads + 2 * ebm::zero_flag_count(ncol, h->cfg.threads);
        e = dev_alloc(h->amask, mn);
        if (e == hipSuccess) e = hipMemset(h->amask.get(), 0, sizeof(unsigned short) * mn);
    }
    if (e == hipSuccess) e = dev_alloc(h->p_dev, 1);
    if (e == hipSuccess) e = hipMemcpy(h->p_dev.get(), &h->p, sizeof(ebm::Params), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = ebm::launch_derive_params(h->p_dev.get(), nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dev_alloc(h->hm_dev, ncol);
    if (e != hipSuccess) return hip_fail("state allocation", e);
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        const int slot = slot_of(model, f);
        h->field[f] = slot >= 0 ? h->state.get() + (size_t)slot * h->fstride : nullptr;
    }
    e = dev_alloc(h->counters, 2 * ebm::kCounterShards);
    if (e == hipSuccess) e = hipMemset(h->counters.get(), 0, sizeof(unsigned long long) * 2 * ebm::kCounterShards);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking);
    if (e == hipSuccess && h->split_col) e = hipStreamCreateWithFlags(h->stream2.out(), hipStreamNonBlocking);
    if (e == hipSuccess && h->split_col) e = hipEventCreateWithFlags(h->ev_fork.out(), hipEventDisableTiming);
    if (e == hipSuccess && h->split_col) e = hipEventCreateWithFlags(h->ev_join.out(), hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(h->ev0.out());
    if (e == hipSuccess) e = hipEventCreate(h->ev1.out());
    if (e != hipSuccess) return hip_fail("ebm_create", e);
    return EBM_OK;
}

}  // namespace

extern "C" {

const char *ebm_last_error(void) { return g_err.c_str(); }
const char *ebm_version(void) { return "ebm_hip 0.1 (gfx950)"; }

int ebm_options_default(ebm_options *opt) {
    if (!opt) return fail(EBM_ERR_ARG, "ebm_options_default: null argument");
    opt->struct_bytes = (int)sizeof(ebm_options);
    opt->cells_per_thread = 0;
    opt->use_graph = -1;
    opt->prefetch_cols = -1;
    opt->launch_chains = -1;
    opt->integrate_steps_per_launch = -1;
    opt->fused_state_in_lds = -1;
    opt->elide_zero_lines = -1;
    return EBM_OK;
}

int ebm_create(ebm_handle_t *out, int model, int grid, int nlat, int ncol, const double *x,
               const double *params, double dt, int device) {
    return ebm_create_ex(out, model, grid, nlat, ncol, x, params, dt, device, nullptr);
}

int ebm_create_ex(ebm_handle_t *out, int model, int grid, int nlat, int ncol, const double *x,
                  const double *params, double dt, int device, const ebm_options *user_opt) {
    if (!out || !x || !params) return fail(EBM_ERR_ARG, "ebm_create: null argument");
    *out = nullptr;
    ebm_options opt;
    int rc = read_options(user_opt, opt);
    if (rc) return rc;
    if (model != EBM_MODEL_MIZ && model != EBM_MODEL_CLASSIC && model != EBM_MODEL_MIZ_IMEX)
        return fail(EBM_ERR_ARG, "ebm_create: unknown model");
    const bool imex = model == EBM_MODEL_MIZ_IMEX;        // the extension is the MIZ model with one more solve per step
    if (imex) model = EBM_MODEL_MIZ;
    if (grid != EBM_GRID_IDENTITY && grid != EBM_GRID_NONUNIFORM) return fail(EBM_ERR_ARG, "ebm_create: unknown grid kind");
    if (nlat < 2 || ncol < 1) return fail(EBM_ERR_ARG, "ebm_create: need nlat >= 2 and ncol >= 1");
    if (!(dt > 0.0)) return fail(EBM_ERR_ARG, "ebm_create: dt must be positive");
    if (model == EBM_MODEL_MIZ && params[EBM_P_Tm] < 0.0 && params[EBM_P_m2] != std::floor(params[EBM_P_m2]))
        return fail(EBM_ERR_ARG, "ebm_create: Tm^m2 with Tm < 0 and non-integer m2 (DomainError in the reference, src/miz.jl:71)");
    if (opt.cells_per_thread == 2 && (imex || nlat > ebm::kMaxLat2))
        return fail(EBM_ERR_ARG, "ebm_create_ex: cells_per_thread = 2 needs nlat <= 1536 and is not built for the IMEX extension");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(EBM_ERR_NO_DEVICE, "ebm_create: no HIP device available (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(EBM_ERR_ARG, "ebm_create: device index out of range");
    ebm::LaunchCfg cfg = ebm::choose_launch(nlat, opt.cells_per_thread);      // a function of nlat and the option only
    if (cfg.threads == 0)
        return fail(EBM_ERR_UNSUPPORTED, "ebm_create: nlat > 4096 is not supported (one workgroup owns a whole meridian)");
    HIPCHK(hipSetDevice(device));
    HIPCHK(ebm::prepare_kernels(cfg));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    auto h = std::make_unique<ebm_ctx>();
    h->model = model; h->grid = grid; h->nlat = nlat; h->ncol = ncol; h->device = device;
    h->dt = dt; h->cfg = cfg; h->imex = imex;
    // (elide_zero_lines: on by default wherever the deriving kernel is — the book ignores it elsewhere)
    h->book = FieldBook(model, model == EBM_MODEL_MIZ && cfg.cells == 4, model == EBM_MODEL_MIZ && ebm::has_step_kernel(cfg, {ebm::STEP_MIZ, grid, imex, ebm::OUT_STATE, true, false}),
                        opt.elide_zero_lines != 0);
    h->num_cus = prop.multiProcessorCount;
    choose_heuristics(h.get(), opt);
    h->pitch = (long long)cfg.threads * cfg.cells;     // >= nlat; padding cells stay zero
    ebm_tables::fill_params(h->p, params, dt);
    if ((rc = allocate(h.get(), x))) return rc;
    *out = h.release();
    return EBM_OK;
}

int ebm_destroy(ebm_handle_t h) {
    delete h;
    return EBM_OK;
}

int ebm_sync(ebm_handle_t h) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_sync: null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    return EBM_OK;
}

int ebm_get_counters(ebm_handle_t h, long long *counters) {
    if (!h || !counters) return fail(EBM_ERR_ARG, "ebm_get_counters: null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    unsigned long long host[2 * ebm::kCounterShards];
    HIPCHK(hipMemcpy(host, h->counters.get(), sizeof(host), hipMemcpyDeviceToHost));
    long long solves = 0, caps = 0;
    for (int i = 0; i < ebm::kCounterShards; ++i) {
        solves += (long long)host[2 * i];
        caps += (long long)host[2 * i + 1];
    }
    counters[0] = h->n_steps;
    counters[1] = solves;
    counters[2] = caps;
    counters[3] = h->n_launches;
    return EBM_OK;
}

int ebm_reset_counters(ebm_handle_t h) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_reset_counters: null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    HIPCHK(hipMemset(h->counters.get(), 0, sizeof(unsigned long long) * 2 * ebm::kCounterShards));
    h->n_steps = 0;
    h->n_launches = 0;
    return EBM_OK;
}

int ebm_state_conversions(ebm_handle_t h, long long *count) {
    if (!h || !count) return fail(EBM_ERR_ARG, "ebm_state_conversions: null argument");
    *count = h->book.conversions();
    return EBM_OK;
}

int ebm_zero_line_flags(ebm_handle_t h, unsigned *words, int *trusted) {
    if (!h || !words || !trusted) return fail(EBM_ERR_ARG, "ebm_zero_line_flags: null argument");
    if (!h->book.elides_zero_lines())
        return fail(EBM_ERR_UNSUPPORTED, "ebm_zero_line_flags: this handle does not elide zero lines (ebm_options::elide_zero_lines)");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    HIPCHK(hipMemcpy(words, ebm::zero_flag_words(h->amask.get(), h->ncol, h->cfg.threads),
                     sizeof(unsigned) * ebm::zero_flag_count(h->ncol, h->cfg.threads), hipMemcpyDeviceToHost));
    *trusted = h->book.zero_flags_trusted() ? 1 : 0;
    return EBM_OK;
}

int ebm_timer_start(ebm_handle_t h) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_timer_start: null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->ev0.get(), main_stream(h)));
    return EBM_OK;
}

int ebm_timer_stop(ebm_handle_t h, float *elapsed_ms) {
    if (!h || !elapsed_ms) return fail(EBM_ERR_ARG, "ebm_timer_stop: null argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventRecord(h->ev1.get(), main_stream(h)));
    HIPCHK(hipEventSynchronize(h->ev1.get()));
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev0.get(), h->ev1.get()));
    return EBM_OK;
}

#ifdef EBM_STAMPS
// Diagnostic build only: allocate / fetch the phase stamps: per workgroup (ncol x 16), then per wave
// (ncol x 16 waves x 8).
int ebm_debug_stamps(ebm_handle_t h, unsigned long long *host) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_debug_stamps: null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    const size_t n = (16 + 128) * (size_t)h->ncol;
    if (!h->stamps) {
        DevBuf<unsigned long long> b;
        HIPCHK(dev_alloc(b, n));
        HIPCHK(hipMemset(b.get(), 0, sizeof(unsigned long long) * n));
        h->stamps = std::move(b);
        invalidate_graph(h);                     // the captured launches hold the old argument values
        return EBM_OK;
    }
    if (host) HIPCHK(hipMemcpy(host, h->stamps.get(), sizeof(unsigned long long) * n, hipMemcpyDeviceToHost));
    return EBM_OK;
}
#endif

int ebm_selftest_divide(int device, int n, const double *a, const double *b, double *q) {
    if (n < 0 || !a || !b || !q) return fail(EBM_ERR_ARG, "ebm_selftest_divide: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(EBM_ERR_NO_DEVICE, "ebm_selftest_divide: no HIP device available");
    HIPCHK(hipSetDevice(device));
    DevBuf<double> da, db, dq;
    const size_t nb = sizeof(double) * (size_t)n;
    HIPCHK(dev_alloc(da, n)); HIPCHK(dev_alloc(db, n)); HIPCHK(dev_alloc(dq, n));
    HIPCHK(hipMemcpy(da.get(), a, nb, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(db.get(), b, nb, hipMemcpyHostToDevice));
    hipError_t e = ebm::launch_divide(da.get(), db.get(), dq.get(), n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(q, dq.get(), nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("ebm_selftest_divide", e);
    return EBM_OK;
}

int ebm_selftest_permute(int device, int threads, int ncol, const double *in, double *split, double *back) {
    if (threads < 64 || threads > 1024 || threads % 64 || ncol < 1 || !in || !split || !back)
        return fail(EBM_ERR_ARG, "ebm_selftest_permute: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(EBM_ERR_NO_DEVICE, "ebm_selftest_permute: no HIP device available");
    HIPCHK(hipSetDevice(device));
    const size_t n = (size_t)ncol * 4 * (size_t)threads, nb = sizeof(double) * n;
    DevBuf<double> d;
    HIPCHK(dev_alloc(d, n));
    HIPCHK(hipMemcpy(d.get(), in, nb, hipMemcpyHostToDevice));
    ebm::LaunchCfg cfg{};
    cfg.threads = threads;
    cfg.cells = 4;
    hipError_t e = ebm::launch_split_fields(d.get(), 0, 1, ncol, cfg, nullptr);
    if (e == hipSuccess) e = hipMemcpy(split, d.get(), nb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = ebm::launch_unsplit_fields(d.get(), 0, 1, ncol, cfg, nullptr);
    if (e == hipSuccess) e = hipMemcpy(back, d.get(), nb, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("ebm_selftest_permute", e);
    return EBM_OK;
}

int ebm_launch_info(ebm_handle_t h, int *info) {
    if (!h || !info) return fail(EBM_ERR_ARG, "ebm_launch_info: null argument");
    info[0] = h->cfg.threads;
    info[1] = h->cfg.cells;
    info[2] = (int)one_step_lds_bytes(h->cfg);
    info[3] = h->ncol;
    return EBM_OK;
}

}  // extern "C"
