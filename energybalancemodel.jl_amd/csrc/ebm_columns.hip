// Host runtime, per-column inputs (ebm_runtime.h lists the units): forcing offsets, Forcing schedules, AR(1) noise and
// parameter sets, each installed all-or-nothing; the step clock and the time table; the resampling of whole columns and
// their packed export and import.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>

#include "ebm_runtime.h"
#include "ebm_tables.h"

using namespace ebm_rt;

namespace {

// ebm_set_column_forcing / _schedule: nwords doubles per column from `src` (null: none) into the handle's `dst`
int install_columns(ebm_ctx *h, DevBuf<double> &dst, const double *src, size_t nwords) {
    DevBuf<double> b;
    if (src) {
        HIPCHK(dev_alloc(b, nwords * (size_t)h->ncol));
        HIPCHK(hipMemcpy(b.get(), src, sizeof(double) * nwords * (size_t)h->ncol, hipMemcpyHostToDevice));
    }
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    dst = std::move(b);
    invalidate_graph(h);                         // the captured launches hold the old argument values
    return EBM_OK;
}

}  // namespace

extern "C" {

int ebm_set_column_forcing(ebm_handle_t h, const double *fcol) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_set_column_forcing: null handle");
    HIPCHK(hipSetDevice(h->device));
    return install_columns(h, h->fcol, fcol, 1);
}

int ebm_set_column_schedule(ebm_handle_t h, const double *sched) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_set_column_schedule: null handle");
    HIPCHK(hipSetDevice(h->device));
    for (int c = 0; sched && c < h->ncol; ++c) {
        const double *w = sched + (size_t)ebm::kSchedWords * c;
        if (!(w[5] <= w[6] && w[6] <= w[7] && w[7] <= w[8]))
            return fail(EBM_ERR_ARG, "ebm_set_column_schedule: breakpoints must be non-decreasing");
    }
    return install_columns(h, h->fsched, sched, ebm::kSchedWords);
}

int ebm_set_column_noise(ebm_handle_t h, const double *sigma, const double *rho, const unsigned long long *stream,
                         unsigned long long seed) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_set_column_noise: null handle");
    std::vector<ebm::NoiseRec> rec;
    if (sigma) {
        if (!rho) return fail(EBM_ERR_ARG, "ebm_set_column_noise: rho is null (pass zeros for white noise)");
        rec.resize((size_t)h->ncol);
        for (int c = 0; c < h->ncol; ++c) {
            if (!(std::isfinite(sigma[c]) && sigma[c] >= 0.0))
                return fail(EBM_ERR_ARG, "ebm_set_column_noise: sigma[" + std::to_string(c) + "] must be finite and >= 0");
            if (!(std::isfinite(rho[c]) && rho[c] >= 0.0 && rho[c] < 1.0))
                return fail(EBM_ERR_ARG, "ebm_set_column_noise: rho[" + std::to_string(c) + "] must lie in [0, 1)");
            rec[c].s = sigma[c] * std::sqrt(1.0 - rho[c] * rho[c]);
            rec[c].rho = rho[c];
            rec[c].stream = stream ? stream[c] : (unsigned long long)c;
        }
    }
    HIPCHK(hipSetDevice(h->device));
    ebm_ctx::Noise nz;                           // sigma null: no noise
    if (sigma) {
        const std::vector<double> zeros((size_t)h->ncol, 0.0);
        HIPCHK(dev_alloc(nz.rec, (size_t)h->ncol));
        HIPCHK(dev_alloc(nz.state, (size_t)h->ncol));
        HIPCHK(dev_alloc(nz.seq, ebm::kNoiseMaxFused * (size_t)h->ncol));
        HIPCHK(hipMemcpy(nz.rec.get(), rec.data(), sizeof(ebm::NoiseRec) * (size_t)h->ncol, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(nz.state.get(), zeros.data(), sizeof(double) * (size_t)h->ncol, hipMemcpyHostToDevice));
        nz.seed = seed;
    }
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    h->noise = std::move(nz);
    invalidate_graph(h);                         // the captured launches hold the old argument values
    return EBM_OK;
}

int ebm_get_noise_state(ebm_handle_t h, double *N) {
    if (!h || !N) return fail(EBM_ERR_ARG, "ebm_get_noise_state: bad argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    if (!h->noise.state) {                       // no noise: N_c = 0
        std::fill(N, N + h->ncol, 0.0);
        return EBM_OK;
    }
    HIPCHK(hipMemcpy(N, h->noise.state.get(), sizeof(double) * (size_t)h->ncol, hipMemcpyDeviceToHost));
    return EBM_OK;
}

int ebm_set_noise_state(ebm_handle_t h, const double *N) {
    if (!h || !N) return fail(EBM_ERR_ARG, "ebm_set_noise_state: bad argument");
    if (!h->noise.state) return fail(EBM_ERR_ARG, "ebm_set_noise_state: no noise installed (ebm_set_column_noise)");
    for (int c = 0; c < h->ncol; ++c)
        if (!std::isfinite(N[c])) return fail(EBM_ERR_ARG, "ebm_set_noise_state: N[" + std::to_string(c) + "] is not finite");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    HIPCHK(hipMemcpy(h->noise.state.get(), N, sizeof(double) * (size_t)h->ncol, hipMemcpyHostToDevice));
    return EBM_OK;
}

int ebm_noise_innovations(ebm_handle_t h, long long first_step, int nsteps, double *out) {
    if (!h || first_step < 0 || nsteps < 0 || (nsteps > 0 && !out)) return fail(EBM_ERR_ARG, "ebm_noise_innovations: bad argument");
    if (!h->noise.rec) return fail(EBM_ERR_ARG, "ebm_noise_innovations: no noise installed (ebm_set_column_noise)");
    if (nsteps == 0) return EBM_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->ncol * (size_t)nsteps;
    DevBuf<double> dev;
    HIPCHK(dev_alloc(dev, n));
    hipError_t e = ebm::launch_noise_innovations(h->noise.rec.get(), h->noise.seed, first_step, nsteps, h->ncol, dev.get(),
                                                 main_stream(h));
    if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
    if (e == hipSuccess) e = hipMemcpy(out, dev.get(), sizeof(double) * n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail("ebm_noise_innovations", e);
    return EBM_OK;
}

int ebm_set_column_params(ebm_handle_t h, const double *params) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_set_column_params: null handle");
    const int np = EBM_P_COUNT;
    // the rows ebm_create would refuse as its vector (ebm_create_ex)
    if (params && h->model == EBM_MODEL_MIZ)
        for (int c = 0; c < h->ncol; ++c) {
            const double *r = params + (size_t)np * c;
            if (r[EBM_P_Tm] < 0.0 && r[EBM_P_m2] != std::floor(r[EBM_P_m2]))
                return fail(EBM_ERR_ARG, "ebm_set_column_params: column " + std::to_string(c) +
                                             ": Tm^m2 with Tm < 0 and non-integer m2 (DomainError in the reference, src/miz.jl:71)");
        }
    HIPCHK(hipSetDevice(h->device));
    // distinct rows by bit pattern, in order of first appearance
    std::vector<int> col_set((size_t)h->ncol, 0);
    std::vector<const double *> rows;
    if (params) {
        std::map<std::string, int> seen;
        for (int c = 0; c < h->ncol; ++c) {
            const double *r = params + (size_t)np * c;
            auto it = seen.emplace(std::string(reinterpret_cast<const char *>(r), sizeof(double) * np), (int)rows.size());
            if (it.second) rows.push_back(r);
            col_set[c] = it.first->second;
        }
    }
    ebm_ctx::ParamSets sets;
    sets.n = (int)rows.size();
    sets.host.resize((size_t)sets.n);
    if (sets.n) {
        // every set built by the code ebm_create runs for its vector: fill_params, build_tables, derive_params_kernel
        const long long set_stride = (long long)ebm::G_COUNT * h->gstride;
        std::vector<double> slab((size_t)sets.n * set_stride, 0.0);
        for (int i = 0; i < sets.n; ++i) {
            ebm_tables::fill_params(sets.host[i], rows[i], h->dt);
            ebm_tables::build_tables(h->model, h->grid, h->nlat, h->gstride, h->dt, sets.host[i], h->xhost.data(),
                                     slab.data() + (size_t)i * set_stride);
        }
        hipError_t e = dev_alloc(sets.p, (size_t)sets.n);
        if (e == hipSuccess) e = dev_alloc(sets.geom, slab.size());
        if (e == hipSuccess && sets.n > 1) e = dev_alloc(sets.col, (size_t)h->ncol);
        if (e == hipSuccess) e = hipMemcpy(sets.p.get(), sets.host.data(), sizeof(ebm::Params) * (size_t)sets.n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(sets.geom.get(), slab.data(), sizeof(double) * slab.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && sets.col)
            e = hipMemcpy(sets.col.get(), col_set.data(), sizeof(int) * (size_t)h->ncol, hipMemcpyHostToDevice);
        for (int i = 0; i < sets.n && e == hipSuccess; ++i) e = ebm::launch_derive_params(sets.p.get() + i, h->stream.get());
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream.get());
        if (e == hipSuccess)
            e = hipMemcpy(sets.host.data(), sets.p.get(), sizeof(ebm::Params) * (size_t)sets.n, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail("ebm_set_column_params", e);
    }
    // phi as the parameters that made it give it, before Lf changes under it
    if (int rc = state_written_outside(h)) return rc;
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    h->sets = std::move(sets);
    invalidate_graph(h);                         // the captured launches hold the old argument values
    h->zonal = ebm_ctx::ZonalTables();           // the zonal tables are built again from the parameters now installed
    return EBM_OK;
}

// ebm_resample_columns (include/ebm_hip.h).  The host builds the list of moved columns and uploads it; then every array
// that is part of a column's state goes through the two passes of ebm_resample.hip, one array at a time through ONE
// staging buffer of `moved` rows: the fields that are current, then the warm-start active set with the noise state.  All
// on the handle's stream, nothing synchronised but the reuse of the pinned list.
int ebm_resample_columns(ebm_handle_t h, const int *parent) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_resample_columns: null handle");
    if (!parent) return fail(EBM_ERR_ARG, "ebm_resample_columns: parent is null");
    size_t moved = 0;
    for (int c = 0; c < h->ncol; ++c) {
        if (parent[c] < 0 || parent[c] >= h->ncol)
            return fail(EBM_ERR_ARG, "ebm_resample_columns: parent[" + std::to_string(c) + "] = " + std::to_string(parent[c]) +
                                         " is outside [0, " + std::to_string(h->ncol) + ")");
        moved += parent[c] != c;
    }
    if (moved == 0) return EBM_OK;                       // the identity: nothing is launched
    HIPCHK(hipSetDevice(h->device));
    ebm_ctx::Resample &r = h->resample;
    if (!r.uploaded) HIPCHK(hipEventCreateWithFlags(r.uploaded.out(), hipEventDisableTiming));
    if (r.in_flight) HIPCHK(hipEventSynchronize(r.uploaded.get()));      // the previous call's upload has read the pinned list
    r.in_flight = false;
    if (r.host_cap < moved) {
        r.host_cap = 0;
        HIPCHK(hipHostMalloc(r.host.out(), sizeof(int) * 2 * moved, hipHostMallocDefault));
        r.host_cap = moved;
    }
    HIPCHK(r.dev.reserve(2 * moved));
    // staging rows of pitch doubles each: the scratch of the diffusion operators if the handle has it (three whole fields)
    const bool borrowed = (bool)h->scratch;
    if (!borrowed) HIPCHK(r.stage.reserve(moved * (size_t)h->pitch));
    int *list = r.host.get();
    for (int c = 0, m = 0; c < h->ncol; ++c)
        if (parent[c] != c) {
            list[2 * m] = c;
            list[2 * m + 1] = parent[c];
            ++m;
        }
    // phi moves as a field: current first, under the parent's parameters — which the destination need not share
    if (int rc = state_written_outside(h)) return rc;
    hipStream_t s = main_stream(h);                      // joins the two launch chains: every column's last step has ended
    HIPCHK(hipMemcpyAsync(r.dev.get(), list, sizeof(int) * 2 * moved, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(r.uploaded.get(), s));
    r.in_flight = true;
    ebm::ResampleArgs a{};
    a.stage = reinterpret_cast<uint4 *>(borrowed ? h->scratch.get() : r.stage.get());
    a.stage_stride = h->pitch / 2;
    a.list = reinterpret_cast<const int2 *>(r.dev.get());
    auto two_passes = [&]() -> hipError_t {
        hipError_t e = ebm::launch_resample_stage(a, (int)moved, s);
        return e == hipSuccess ? ebm::launch_resample_scatter(a, (int)moved, s) : e;
    };
    // whole rows in whatever layout they are held (the book hears nothing); a stale field is not copied and stays stale
    a.row_stride = h->pitch / 2;
    a.units = (int)(h->pitch / 2);
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        if (!(h->book.current_mask() >> f & 1u)) continue;
        a.rows = reinterpret_cast<uint4 *>(h->field[f]);
        hipError_t e = two_passes();
        if (e != hipSuccess) return hip_fail("ebm_resample_columns", e);
    }
    // the warm-start active set (rows of `threads` unsigned shorts: threads / 8 units) and N_c
    if (h->amask || h->noise.state) {
        a.rows = reinterpret_cast<uint4 *>(h->amask.get());
        a.row_stride = a.units = h->amask ? h->cfg.threads / 8 : 0;
        a.nstate = h->noise.state.get();
        hipError_t e = two_passes();
        if (e != hipSuccess) return hip_fail("ebm_resample_columns", e);
    }
    // the diffusion operators expect their scratch zero in the padding cells
    if (borrowed) HIPCHK(hipMemsetAsync(h->scratch.get(), 0, sizeof(double) * moved * (size_t)h->pitch, s));
    return EBM_OK;
}

}  // extern "C"

namespace {

// The record of ebm_export_columns / ebm_import_columns (include/ebm_hip.h): a function of the model, nlat and
// cells_per_thread only.  `current` is the mask an export would return now.
struct RecordShape {
    int field[ebm::kExchangeSlots];                      // slot -> public field id, in enum order
    int nfields = 0, rowlen = 0, amask_units = 0;
    long long doubles = 0;
    unsigned prognostic = 0, all = 0, current = 0;
};
RecordShape record_shape(const ebm_ctx *h) {
    RecordShape r;
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        if (!h->book.has(f)) continue;
        r.field[r.nfields++] = f;
        r.all |= 1u << f;
        if (!h->book.is_diagnostic(f)) r.prognostic |= 1u << f;
    }
    r.current = h->book.current_mask();
    r.rowlen = (h->nlat + 15) / 16 * 16;                 // whole 128-byte lines; <= pitch (a multiple of 128 cells)
    r.amask_units = h->amask ? h->cfg.threads / 8 : 0;   // a row of `threads` unsigned shorts
    r.doubles = (long long)r.nfields * r.rowlen + 2 * r.amask_units + 2;
    return r;
}

// the launch arguments of either direction: the rows of the slots in `moved`, each in the layout the handle holds it in
ebm::ExchangeArgs exchange_args(ebm_ctx *h, const RecordShape &r, unsigned moved, double *buf) {
    ebm::ExchangeArgs a{};
    for (int s = 0; s < r.nfields; ++s) {
        const int f = r.field[s];
        if (!(moved >> f & 1u)) continue;
        a.row[s] = h->field[f];
        if (h->book.held_split(f)) a.split_mask |= 1u << s;
    }
    a.buf = buf;
    a.record = r.doubles;
    a.amask = h->amask.get();
    a.nstate = h->noise.state.get();
    a.nfields = r.nfields;
    a.rowlen = r.rowlen;
    a.pitch = (int)h->pitch;
    a.threads = h->cfg.threads;
    a.amask_units = r.amask_units;
    return a;
}

// the argument checks the two calls share; the message names the first offending entry
int check_exchange_args(const ebm_ctx *h, const char *who, int n, const int *cols, const void *dev_buf) {
    if (n < 0) return fail(EBM_ERR_ARG, std::string(who) + ": n = " + std::to_string(n) + " is negative");
    if (n == 0) return EBM_OK;
    if (!cols) return fail(EBM_ERR_ARG, std::string(who) + ": cols is null");
    if (!dev_buf) return fail(EBM_ERR_ARG, std::string(who) + ": dev_buf is null");
    if (reinterpret_cast<uintptr_t>(dev_buf) % 16) return fail(EBM_ERR_ARG, std::string(who) + ": dev_buf is not 16-byte aligned");
    for (int i = 0; i < n; ++i)
        if (cols[i] < 0 || cols[i] >= h->ncol)
            return fail(EBM_ERR_ARG, std::string(who) + ": cols[" + std::to_string(i) + "] = " + std::to_string(cols[i]) +
                                         " is outside [0, " + std::to_string(h->ncol) + ")");
    return EBM_OK;
}

// cols, then records if given, through the pinned list of ebm_ctx::Resample to the device, on stream s: the device list
// (n or 2n ints) is ready for the launch that follows on s, and the host arrays have been consumed on return
int upload_exchange_list(ebm_ctx *h, int n, const int *cols, const int *records, hipStream_t s) {
    ebm_ctx::Resample &r = h->resample;
    if (!r.uploaded) HIPCHK(hipEventCreateWithFlags(r.uploaded.out(), hipEventDisableTiming));
    if (r.in_flight) HIPCHK(hipEventSynchronize(r.uploaded.get()));      // the previous call's upload has read the pinned list
    r.in_flight = false;
    if (r.host_cap < (size_t)n) {
        r.host_cap = 0;
        HIPCHK(hipHostMalloc(r.host.out(), sizeof(int) * 2 * (size_t)n, hipHostMallocDefault));
        r.host_cap = (size_t)n;
    }
    HIPCHK(r.dev.reserve(2 * (size_t)n));
    int *list = r.host.get();
    std::copy(cols, cols + n, list);
    if (records) std::copy(records, records + n, list + n);
    HIPCHK(hipMemcpyAsync(r.dev.get(), list, sizeof(int) * (size_t)n * (records ? 2 : 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(r.uploaded.get(), s));
    r.in_flight = true;
    return EBM_OK;
}

}  // namespace

extern "C" {

int ebm_column_record(ebm_handle_t h, long long *record_doubles, unsigned *current_mask) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_column_record: null handle");
    const RecordShape r = record_shape(h);
    if (record_doubles) *record_doubles = r.doubles;
    if (current_mask) *current_mask = r.current;
    return EBM_OK;
}

int ebm_export_columns(ebm_handle_t h, int n, const int *cols, double *dev_buf, unsigned *mask) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_export_columns: null handle");
    if (int rc = check_exchange_args(h, "ebm_export_columns", n, cols, dev_buf)) return rc;
    const RecordShape r = record_shape(h);
    if (mask) *mask = r.current;
    if (n == 0) return EBM_OK;
    HIPCHK(hipSetDevice(h->device));
    // phi travels as a field: current first.  The state stays consistent — nothing is written
    hipError_t e = restore_phi(h);
    if (e != hipSuccess) return hip_fail("phi restore", e);
    hipStream_t s = main_stream(h);                      // joins the two launch chains: every column's last step has ended
    if (int rc = upload_exchange_list(h, n, cols, nullptr, s)) return rc;
    ebm::ExchangeArgs a = exchange_args(h, r, r.current, dev_buf);
    a.cols = h->resample.dev.get();
    e = ebm::launch_export_columns(a, n, s);
    if (e != hipSuccess) return hip_fail("ebm_export_columns", e);
    return EBM_OK;
}

int ebm_import_columns(ebm_handle_t h, int n, const int *cols, const int *records, const double *dev_buf, unsigned mask) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_import_columns: null handle");
    if (int rc = check_exchange_args(h, "ebm_import_columns", n, cols, dev_buf)) return rc;
    const RecordShape r = record_shape(h);
    if (n > 0) {
        std::vector<char> seen((size_t)h->ncol, 0);
        for (int i = 0; i < n; ++i) {
            if (seen[cols[i]])
                return fail(EBM_ERR_ARG, "ebm_import_columns: cols[" + std::to_string(i) + "] = " + std::to_string(cols[i]) +
                                             " is a repeated destination");
            seen[cols[i]] = 1;
        }
        for (int i = 0; records && i < n; ++i)
            if (records[i] < 0)
                return fail(EBM_ERR_ARG, "ebm_import_columns: records[" + std::to_string(i) + "] = " + std::to_string(records[i]) +
                                             " is negative");
    }
    for (int f = 0; f < 32; ++f) {
        if ((mask >> f & 1u) && !(r.all >> f & 1u))
            return fail(EBM_ERR_ARG, "ebm_import_columns: mask names field " + std::to_string(f) + ", which this model does not have");
        if ((r.prognostic >> f & 1u) && !(mask >> f & 1u))
            return fail(EBM_ERR_ARG, std::string("ebm_import_columns: mask lacks the prognostic field ") + field_name(f));
    }
    // a field that is current here and absent from the records would keep its old rows under another member's prognostics
    for (int s = 0; s < r.nfields; ++s)
        if ((r.current & ~mask) >> r.field[s] & 1u)
            return fail(EBM_ERR_STALE, std::string("ebm_import_columns: field ") + field_name(r.field[s]) +
                                           " is current in this handle but was stale in the exporter (absent from mask): the "
                                           "imported columns would hold it under another member's state");
    if (n == 0) return EBM_OK;
    HIPCHK(hipSetDevice(h->device));
    // Ei, h and phi are written by a non-step writer: phi current first, and the next launch loads it
    if (int rc = state_written_outside(h)) return rc;
    hipStream_t s = main_stream(h);                      // joins the two launch chains: every column's last step has ended
    if (int rc = upload_exchange_list(h, n, cols, records, s)) return rc;
    // whatever is current here is in the mask; a slot whose field is stale here is ignored, and the field stays stale
    ebm::ExchangeArgs a = exchange_args(h, r, r.current, const_cast<double *>(dev_buf));
    a.cols = h->resample.dev.get();
    a.records = records ? h->resample.dev.get() + n : nullptr;
    hipError_t e = ebm::launch_import_columns(a, n, s);
    if (e != hipSuccess) return hip_fail("ebm_import_columns", e);
    return EBM_OK;
}

int ebm_set_step_clock(ebm_handle_t h, long long step) {
    if (!h || step < 0) return fail(EBM_ERR_ARG, "ebm_set_step_clock: bad argument");
    h->clock = step;
    return EBM_OK;
}

int ebm_set_time_table(ebm_handle_t h, int nt, const double *cos2pit) {
    if (!h || !cos2pit || nt < 1) return fail(EBM_ERR_ARG, "ebm_set_time_table: bad argument");
    h->ttab.assign(cos2pit, cos2pit + nt);
    return EBM_OK;
}

}  // extern "C"
