// Host runtime, fields (ebm_runtime.h lists the units): set / get with the validity bookkeeping, device views, hemispheric
// means, the ensemble reductions, the ensemble Kalman update (ebm_update_columns) and the two diffusion operators that work on
// caller-supplied fields (ebm_diffusion, ebm_zonal_diffusion).
#include <cmath>
#include <cstring>

#include "ebm_runtime.h"
#include "ebm_tables.h"

using namespace ebm_rt;

namespace ebm_rt {

// The one executor of the book's passes (Pass, ebm_fieldbook.h): in place, on the handle's stream — which joins the two launch
// chains first (main_stream), so every column's last step has ended; never inside a graph capture (build_graph and ebm_run
// convert before they capture / replay).  The book hears of the pass only if it was enqueued.
static hipError_t exec_pass(ebm_ctx *h, Pass p) {
    double *const prog = h->field[EBM_F_Ei], *const diag = h->field[EBM_F_Tw];     // Ei .. phi: slots 0 .. 4; Tw .. T: 6 .. 10
    hipError_t e = hipSuccess;
    switch (p) {
        case Pass::NONE: return hipSuccess;
        case Pass::SPLIT_STATE: e = ebm::launch_split_fields(prog, h->fstride, 5, h->ncol, h->cfg, main_stream(h)); break;
        case Pass::UNSPLIT_STATE: e = ebm::launch_unsplit_fields(prog, h->fstride, 5, h->ncol, h->cfg, main_stream(h)); break;
        case Pass::UNSPLIT_STATE_FORM_PHI: e = ebm::launch_restore_phi(base_args(h), h->ncol, h->cfg, true, main_stream(h)); break;
        case Pass::RESTORE_PHI: e = ebm::launch_restore_phi(base_args(h), h->ncol, h->cfg, false, main_stream(h)); break;
        case Pass::UNSPLIT_DIAG: e = ebm::launch_unsplit_fields(diag, h->fstride, 5, h->ncol, h->cfg, main_stream(h)); break;
    }
    if (e == hipSuccess) h->book.done(p);
    return e;
}

int ensure_natural(ebm_ctx *h) {
    hipError_t e = exec_pass(h, h->book.diag_layout_natural());
    return e == hipSuccess ? EBM_OK : hip_fail("unsplit_fields", e);
}
hipError_t convert_state(ebm_ctx *h, bool split) { return exec_pass(h, h->book.state_layout(split)); }
int set_state_layout(ebm_ctx *h, bool split) {
    hipError_t e = convert_state(h, split);
    return e == hipSuccess ? EBM_OK : hip_fail("state layout conversion", e);
}
// What a kernel that reads whole fields where they lie needs first (the mean kernels, snapshots, the fused kernels over an
// active list): the prognostic fields natural and, if the caller reads them too, the diagnostic ones.
int natural_layout(ebm_ctx *h, bool diagnostics_too) {
    if (diagnostics_too)
        if (int rc = ensure_natural(h)) return rc;
    return set_state_layout(h, false);
}
hipError_t restore_phi(ebm_ctx *h) { return exec_pass(h, h->book.phi_readable()); }
int state_written_outside(ebm_ctx *h) {
    hipError_t e = restore_phi(h);
    if (e != hipSuccess) return hip_fail("phi restore", e);
    h->book.state_written_outside();
    return EBM_OK;
}

int get_copier(ebm_ctx *h) {
    if (h->copier) return EBM_OK;
    auto c = std::make_unique<HostCopier>();
    hipError_t e = c->init(h->device);
    if (e != hipSuccess) return hip_fail("pinned staging ring", e);
    h->copier = std::move(c);
    return EBM_OK;
}

static_assert((int)EBM_S_INTEGRAL == (int)ebm::S_INTEGRAL && (int)EBM_S_MEAN == (int)ebm::S_MEAN && (int)EBM_S_EDGE_GE == (int)ebm::S_EDGE_GE &&
              (int)EBM_S_EDGE_LE == (int)ebm::S_EDGE_LE && (int)EBM_S_COUNT == (int)ebm::S_KINDS, "enum ebm_scalar_kind");
int resolve_scalars(const ebm_ctx *h, const char *who, int nscal, const int *spec, const double *level, ScalarRef *out) {
    const std::string me(who);
    if (nscal < 1 || nscal > ebm::kMaxQuantities)
        return fail(EBM_ERR_ARG, me + ": nscal = " + std::to_string(nscal) + " is outside 1 ... " + std::to_string(ebm::kMaxQuantities));
    for (int s = 0; s < nscal; ++s) {
        const int kind = spec[4 * s], f = spec[4 * s + 1], k0 = spec[4 * s + 2], k1 = spec[4 * s + 3];
        const std::string it = me + ": scalar " + std::to_string(s) + ": ";
        const bool edge = kind == EBM_S_EDGE_GE || kind == EBM_S_EDGE_LE;
        if (kind < 0 || kind >= EBM_S_COUNT) return fail(EBM_ERR_ARG, it + "unknown kind " + std::to_string(kind));
        if (!h->book.has(f) || quantity_of(h->model, f) < 0) return fail(EBM_ERR_ARG, it + "its field is not a solution variable of this model");
        if (k0 < 0 || k1 > h->nlat - 1 || k0 > k1)
            return fail(EBM_ERR_ARG, it + "the band k0 = " + std::to_string(k0) + ", k1 = " + std::to_string(k1) + " is not 0 <= k0 <= k1 <= " +
                                         std::to_string(h->nlat - 1));
        if (!edge && k0 == k1) return fail(EBM_ERR_ARG, it + "an integral over one cell (k0 == k1 = " + std::to_string(k0) + ")");
        if (edge && level[s] != level[s]) return fail(EBM_ERR_ARG, it + "the level of an edge is NaN");
        out[s] = {f, kind, k0, k1, level[s], h->book.is_diagnostic(f)};
    }
    return EBM_OK;
}
ebm::ScalarArgs scalar_args(const ebm_ctx *h, int nscal, const ScalarRef *sc) {
    ebm::ScalarArgs a{};
    for (int s = 0; s < nscal; ++s) {
        a.row[s] = h->field[sc[s].field];
        a.kind[s] = sc[s].kind; a.k0[s] = sc[s].k0; a.k1[s] = sc[s].k1; a.level[s] = sc[s].level;
    }
    a.x = x_table(h);
    a.pitch = (int)h->pitch; a.nscal = nscal;
    return a;
}

}  // namespace ebm_rt

namespace {

// The preamble of every field reader, in this order: the arguments, the field is one of this model (check_field); it is
// current (check_current; ebm_get_field_as_of has its own rule here); the handle's device and the natural layout (make_readable).
int check_field(const ebm_ctx *h, int field, const void *out, const char *who) {
    if (!h || !out) return fail(EBM_ERR_ARG, std::string(who) + ": null argument");
    if (!h->book.has(field)) return fail(EBM_ERR_ARG, std::string(who) + ": field not part of this model");
    return EBM_OK;
}
int make_readable(ebm_ctx *h, int field) {
    HIPCHK(hipSetDevice(h->device));
    return h->book.is_split_state_field(field) ? set_state_layout(h, false) : h->book.is_split_field(field) ? ensure_natural(h) : EBM_OK;
}
int open_field(ebm_ctx *h, int field, const void *out, const char *who) {
    int rc = check_field(h, field, out, who);
    if (!rc) rc = check_current(h, field, who);
    if (!rc) rc = make_readable(h, field);
    return rc;
}

// ncol rows of nlat doubles, row pitches in doubles (nlat: packed, h->pitch: a padded device field), on the handle's stream
hipError_t copy_rows(ebm_ctx *h, double *dst, long long dst_pitch, const double *src, long long src_pitch, hipMemcpyKind kind) {
    return hipMemcpy2DAsync(dst, sizeof(double) * dst_pitch, src, sizeof(double) * src_pitch, sizeof(double) * h->nlat,
                            h->ncol, kind, main_stream(h));
}

// device -> host through the pinned ring (synchronous)
int download_field(ebm_ctx *h, int field, double *host, const char *who) {
    int rc = get_copier(h);
    if (rc) return rc;
    HostCopier *c = h->copier.get();
    HIPCHK(c->wait_all());
    HIPCHK(c->order_after(main_stream(h)));
    CopyJob j;
    j.src = h->field[field]; j.src_pitch = (size_t)h->pitch; j.row_elems = (size_t)h->nlat; j.nrows = (size_t)h->ncol; j.dst = host;
    hipError_t e = c->run(j);
    if (e != hipSuccess) return hip_fail(who, e);
    return EBM_OK;
}

// ebm_hemispheric_mean / _device: the per-column means of a readable field into dev_out
hipError_t hemispheric_mean(ebm_ctx *h, int field, double *dev_out) {
    ebm::MeansArgs m{};              // one field: slot[0] = 0
    m.state = h->field[field]; m.x = x_table(h); m.out = dev_out;
    m.pitch = (int)h->pitch; m.nlat = h->nlat; m.nvars = 1;
    return ebm::launch_hemispheric_means(m, h->ncol, main_stream(h));
}

// What ebm_ensemble_sums, ebm_ensemble_range and ebm_ensemble_histogram have in common (include/ebm_hip.h), in the order every
// one of them keeps: the arguments (ensemble_check: no device work, nothing of the handle changes), the call's own checks,
// then ensemble_open — staleness, phi made current, the launch chains joined, the weights uploaded, the rows where they lie.
// ebm_column_misfits reads the same rows under the same rules and has no member weights (member_weights = false: none uploaded).
int ensemble_check(const ebm_ctx *h, int nvars, const int *fields, bool each_once, const double *w, bool have_out, const std::string &me) {
    if (!h) return fail(EBM_ERR_ARG, me + ": null handle");
    if (!fields || !have_out) return fail(EBM_ERR_ARG, me + ": null argument");
    if (nvars < 1 || nvars > ebm::kMaxQuantities)
        return fail(EBM_ERR_ARG, me + ": nvars = " + std::to_string(nvars) + " is outside 1 ... " + std::to_string(ebm::kMaxQuantities));
    for (int v = 0; v < nvars; ++v) {
        if (!h->book.has(fields[v]) || quantity_of(h->model, fields[v]) < 0)
            return fail(EBM_ERR_ARG, me + ": fields[" + std::to_string(v) + "] is not a solution variable of this model");
        for (int u = 0; each_once && u < v; ++u)
            if (fields[u] == fields[v]) return fail(EBM_ERR_ARG, me + ": field " + field_name(fields[v]) + " is listed twice");
    }
    for (int c = 0; w && c < h->ncol; ++c)
        if (!std::isfinite(w[c])) return fail(EBM_ERR_ARG, me + ": w[" + std::to_string(c) + "] is not finite (column " + std::to_string(c) + ")");
    return EBM_OK;
}
struct EnsembleRows {
    const double *row[ebm::kMaxQuantities];              // where each lies: no field is converted
    unsigned split_mask = 0;
    const double *w = nullptr;                           // on the device, the upload enqueued on s
    hipStream_t s = nullptr;
    std::vector<double> ones;                            // the unit weights of w = NULL: alive until the call has synchronised
};
int ensemble_open(ebm_ctx *h, int nvars, const int *fields, const double *w, const char *who, EnsembleRows &r, bool member_weights = true) {
    for (int v = 0; v < nvars; ++v)
        if (int rc = check_current(h, fields[v], who)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (member_weights) HIPCHK(h->ensemble.w.reserve((size_t)h->ncol));
    // phi is read as a field: current first, in the layout the state has.  Nothing else of the handle changes
    for (int v = 0; v < nvars; ++v)
        if (fields[v] == EBM_F_phi && h->model == EBM_MODEL_MIZ) {
            hipError_t e = restore_phi(h);
            if (e != hipSuccess) return hip_fail("phi restore", e);
        }
    r.s = main_stream(h);                                // joins the two launch chains: every column's last step has ended
    if (member_weights) {
        r.ones.assign(w ? 0 : (size_t)h->ncol, 1.0);
        HIPCHK(hipMemcpyAsync(h->ensemble.w.get(), w ? w : r.ones.data(), sizeof(double) * (size_t)h->ncol, hipMemcpyHostToDevice, r.s));
        r.w = h->ensemble.w.get();
    }
    for (int v = 0; v < nvars; ++v) {
        const int f = fields[v];
        r.row[v] = h->field[f];
        if (h->book.held_split(f)) r.split_mask |= 1u << v;
    }
    return EBM_OK;
}
// the result down (host variant) and the end of the call: synchronous
int ensemble_close(hipError_t e, double *host_out, const double *dev, size_t n, hipStream_t s, const char *who) {
    if (e == hipSuccess && host_out) e = hipMemcpyAsync(host_out, dev, sizeof(double) * n, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(who, e);
    return EBM_OK;
}

// What tells the three apart: the kernels' column block, and the per-latitude input — the center of the sums (null: none) or
// the edges lo, hi of a histogram of nbins bins
struct EnsembleCall {
    enum Kind { SUMS, RANGE, HISTOGRAM } kind;
    int block;
    const double *center, *lo, *hi;
    int nbins;
    int nslots() const { return kind == HISTOGRAM ? nbins + 2 : 3; }
};
// ebm_ensemble_sums, ebm_ensemble_range, ebm_ensemble_histogram and their _device forms (include/ebm_hip.h): the checks, then
// the two launches of ebm_ensemble.hip into dev_out (the caller's device buffer) or, for host_out, into the handle's own and
// down.  Synchronous.
int ensemble_reduce(ebm_ctx *h, int nvars, const int *fields, const double *w, const EnsembleCall &c, double *host_out,
                    double *dev_out, const char *who) {
    const std::string me(who);
    const bool histogram = c.kind == EnsembleCall::HISTOGRAM;
    if (int rc = ensemble_check(h, nvars, fields, !histogram, w, host_out || dev_out, me)) return rc;
    const size_t npitch = (size_t)h->pitch;
    for (long long i = 0; c.center && i < (long long)nvars * h->nlat; ++i)
        if (!std::isfinite(c.center[i]))
            return fail(EBM_ERR_ARG, me + ": center[" + std::to_string(i / h->nlat) + "][" + std::to_string(i % h->nlat) + "] is not finite");
    std::vector<double> edges;                           // [nvars][lo, hi, s][pitch], padding zero
    if (histogram) {
        if (!c.lo || !c.hi) return fail(EBM_ERR_ARG, me + ": null argument");
        if (c.nbins < 1 || c.nbins > ebm::kHistMaxBins)
            return fail(EBM_ERR_ARG, me + ": nbins = " + std::to_string(c.nbins) + " is outside 1 ... " + std::to_string(ebm::kHistMaxBins));
        edges.assign(3 * (size_t)nvars * npitch, 0.0);
        for (int v = 0; v < nvars; ++v)
            for (int k = 0; k < h->nlat; ++k) {
                const double l = c.lo[(size_t)v * h->nlat + k], u = c.hi[(size_t)v * h->nlat + k];
                const double width = u - l, scale = (double)c.nbins / width;     // one IEEE division: part of the definition
                if (!std::isfinite(l) || !std::isfinite(u) || !(l < u) || !std::isfinite(width) || !std::isfinite(scale))
                    return fail(EBM_ERR_ARG, me + ": lo[" + std::to_string(v) + "][" + std::to_string(k) + "], hi[" + std::to_string(v) +
                                                 "][" + std::to_string(k) + "] are not finite edges with lo < hi and finite hi - lo and nbins / (hi - lo)");
                double *const e = edges.data() + 3 * (size_t)v * npitch + k;
                e[0] = l; e[npitch] = u; e[2 * npitch] = scale;
            }
    }
    EnsembleRows r;
    if (int rc = ensemble_open(h, nvars, fields, w, who, r)) return rc;
    ebm_ctx::Ensemble &b = h->ensemble;
    const int nslots = c.nslots(), nblocks = (h->ncol + c.block - 1) / c.block;
    HIPCHK(b.partial.reserve((size_t)nblocks * (size_t)nslots * (size_t)nvars * npitch));
    if (!dev_out) HIPCHK(b.out.reserve((size_t)ebm::kMaxQuantities * (ebm::kHistMaxBins + 2) * (size_t)h->nlat));
    if (c.center && !b.center.get()) {                   // all twelve rows once; the padding cells stay zero
        HIPCHK(b.center.reserve((size_t)ebm::kMaxQuantities * npitch));
        HIPCHK(hipMemsetAsync(b.center.get(), 0, sizeof(double) * ebm::kMaxQuantities * npitch, r.s));
    }
    if (histogram) HIPCHK(b.edges.reserve(3 * (size_t)ebm::kMaxQuantities * npitch));
    hipError_t e = hipSuccess;
    if (c.center)
        e = hipMemcpy2DAsync(b.center.get(), sizeof(double) * npitch, c.center, sizeof(double) * h->nlat, sizeof(double) * h->nlat,
                             (size_t)nvars, hipMemcpyHostToDevice, r.s);
    if (histogram) e = hipMemcpyAsync(b.edges.get(), edges.data(), sizeof(double) * edges.size(), hipMemcpyHostToDevice, r.s);
    ebm::EnsembleArgs a{};
    for (int v = 0; v < nvars; ++v) a.row[v] = r.row[v];
    a.split_mask = r.split_mask;
    a.w = r.w;
    a.aux = c.center ? b.center.get() : histogram ? b.edges.get() : nullptr;
    a.partial = b.partial.get();
    a.out = dev_out ? dev_out : b.out.get();
    a.pitch = (int)h->pitch; a.nlat = h->nlat; a.ncol = h->ncol; a.nvars = nvars; a.nblocks = nblocks; a.threads = h->cfg.threads;
    a.nslots = nslots;
    if (e == hipSuccess)
        e = histogram ? ebm::launch_ensemble_histogram(a, r.s)
                      : c.kind == EnsembleCall::RANGE ? ebm::launch_ensemble_range(a, r.s) : ebm::launch_ensemble_sums(a, r.s);
    return ensemble_close(e, dev_out ? nullptr : host_out, b.out.get(), (size_t)nslots * (size_t)nvars * (size_t)h->nlat, r.s, who);
}

// ebm_ensemble_covariance and its _device form (include/ebm_hip.h): the checks of the ensemble reductions on handle, fields
// and weights, the call's own on the two centers, then the rows where they lie and the two launches of ebm_covariance.hip into
// dev_out (the caller's device buffer) or, for host_out, into the handle's own and down.  Synchronous.
int ensemble_covariance(ebm_ctx *h, int field_a, int field_b, const double *w, const double *center_a, const double *center_b,
                        double *host_out, double *dev_out, const char *who) {
    const std::string me(who);
    const int fields[2] = {field_a, field_b};
    if (int rc = ensemble_check(h, 2, fields, false, w, host_out || dev_out, me)) return rc;
    const size_t nlat = (size_t)h->nlat, npitch = (size_t)h->pitch;
    const double *const center[2] = {center_a, center_b};
    for (int v = 0; v < 2; ++v)
        for (size_t k = 0; center[v] && k < nlat; ++k)
            if (!std::isfinite(center[v][k]))
                return fail(EBM_ERR_ARG, me + ": center_" + "ab"[v] + "[" + std::to_string(k) + "] is not finite");
    // rule 6 of the definition: one field against itself about one center
    const bool symmetric = field_a == field_b && ((!center_a && !center_b) ||
                                                  (center_a && center_b && !std::memcmp(center_a, center_b, sizeof(double) * nlat)));
    EnsembleRows r;
    if (int rc = ensemble_open(h, 2, fields, w, who, r)) return rc;
    ebm_ctx::Covariance &b = h->covariance;
    const int nblocks = (h->ncol + ebm::kCovBlock - 1) / ebm::kCovBlock;
    HIPCHK(b.partial.reserve((size_t)nblocks * npitch * npitch));
    if (!dev_out) HIPCHK(b.out.reserve(nlat * nlat));
    if ((center_a || center_b) && !b.center.get()) {     // both rows once; the padding cells stay zero
        HIPCHK(b.center.reserve(2 * npitch));
        HIPCHK(hipMemsetAsync(b.center.get(), 0, sizeof(double) * 2 * npitch, r.s));
    }
    hipError_t e = hipSuccess;
    for (int v = 0; v < 2 && e == hipSuccess; ++v)
        if (center[v]) e = hipMemcpyAsync(b.center.get() + v * npitch, center[v], sizeof(double) * nlat, hipMemcpyHostToDevice, r.s);
    ebm::CovarianceArgs a{};
    a.row_a = r.row[0]; a.row_b = r.row[1];
    a.split_a = r.split_mask & 1u; a.split_b = (r.split_mask >> 1) & 1u; a.symmetric = symmetric;
    a.w = r.w;
    a.center_a = center_a ? b.center.get() : nullptr;
    a.center_b = center_b ? b.center.get() + npitch : nullptr;
    a.partial = b.partial.get();
    a.out = dev_out ? dev_out : b.out.get();
    a.pitch = (int)h->pitch; a.nlat = h->nlat; a.ncol = h->ncol; a.nblocks = nblocks; a.threads = h->cfg.threads;
    if (e == hipSuccess) e = ebm::launch_ensemble_covariance(a, r.s);
    return ensemble_close(e, dev_out ? nullptr : host_out, b.out.get(), nlat * nlat, r.s, who);
}

// ebm_column_misfits and its _device form (include/ebm_hip.h): the checks of the ensemble reductions on handle and fields, the
// call's own on targets and rw, then the rows where they lie and the one launch of ebm_misfit.hip into dev_out (the caller's
// device buffer) or, for host_out, into the handle's own and down.  Synchronous.
int column_misfits(ebm_ctx *h, int nvars, const int *fields, int ntargets, const double *target, const double *rw, double *host_out,
                   double *dev_out, const char *who) {
    const std::string me(who);
    if (int rc = ensemble_check(h, nvars, fields, true, nullptr, target && (host_out || dev_out), me)) return rc;
    if (ntargets < 1 || ntargets > ebm::kMisfitMaxTargets)
        return fail(EBM_ERR_ARG, me + ": ntargets = " + std::to_string(ntargets) + " is outside 1 ... " + std::to_string(ebm::kMisfitMaxTargets));
    const long long nlat = h->nlat, per_target = (long long)nvars * nlat;
    for (long long i = 0; i < ntargets * per_target; ++i)
        if (std::isinf(target[i]))
            return fail(EBM_ERR_ARG, me + ": target[" + std::to_string(i / per_target) + "][" + std::to_string(i % per_target / nlat) + "][" +
                                         std::to_string(i % nlat) + "] is infinite (finite, or NaN for no observation)");
    for (long long i = 0; rw && i < per_target; ++i)
        if (!std::isfinite(rw[i]) || rw[i] < 0.0)
            return fail(EBM_ERR_ARG, me + ": rw[" + std::to_string(i / nlat) + "][" + std::to_string(i % nlat) + "] is not finite and >= 0");
    EnsembleRows r;
    if (int rc = ensemble_open(h, nvars, fields, nullptr, who, r, false)) return rc;
    ebm_ctx::Misfit &b = h->misfit;
    const size_t npitch = (size_t)h->pitch, nout = 2 * (size_t)ntargets * (size_t)h->ncol;
    if (!b.target.get()) {                               // all rows once; the padding cells stay zero
        HIPCHK(b.target.reserve((size_t)ebm::kMisfitMaxTargets * ebm::kMaxQuantities * npitch));
        HIPCHK(hipMemsetAsync(b.target.get(), 0, sizeof(double) * ebm::kMisfitMaxTargets * ebm::kMaxQuantities * npitch, r.s));
    }
    if (rw && !b.rw.get()) {
        HIPCHK(b.rw.reserve((size_t)ebm::kMaxQuantities * npitch));
        HIPCHK(hipMemsetAsync(b.rw.get(), 0, sizeof(double) * ebm::kMaxQuantities * npitch, r.s));
    }
    if (!dev_out) HIPCHK(b.out.reserve(2 * (size_t)ebm::kMisfitMaxTargets * (size_t)h->ncol));
    hipError_t e = hipMemcpy2DAsync(b.target.get(), sizeof(double) * npitch, target, sizeof(double) * nlat, sizeof(double) * nlat,
                                    (size_t)ntargets * nvars, hipMemcpyHostToDevice, r.s);
    if (e == hipSuccess && rw)
        e = hipMemcpy2DAsync(b.rw.get(), sizeof(double) * npitch, rw, sizeof(double) * nlat, sizeof(double) * nlat, (size_t)nvars,
                             hipMemcpyHostToDevice, r.s);
    ebm::MisfitArgs a{};
    for (int v = 0; v < nvars; ++v) a.row[v] = r.row[v];
    a.split_mask = r.split_mask;
    a.ntargets = ntargets;
    a.target = b.target.get();
    a.rw = rw ? b.rw.get() : nullptr;
    a.out = dev_out ? dev_out : b.out.get();
    a.pitch = (int)h->pitch; a.nlat = h->nlat; a.ncol = h->ncol; a.nvars = nvars; a.threads = h->cfg.threads;
    if (e == hipSuccess) e = ebm::launch_column_misfits(a, r.s);
    return ensemble_close(e, dev_out ? nullptr : host_out, b.out.get(), nout, r.s, who);
}

// ebm_column_scalars and its _device form (include/ebm_hip.h): the checks, then every field readable as ebm_hemispheric_mean
// makes its one (open_field's steps, the arguments of all scalars before the first conversion), and the one launch into dev_out
// (the caller's device buffer) or, for host_out, into the handle's own and down.  Synchronous.
int column_scalars(ebm_ctx *h, int nscal, const int *spec, const double *level, double *host_out, double *dev_out, const char *who) {
    if (!h || !spec || !level || !(host_out || dev_out)) return fail(EBM_ERR_ARG, std::string(who) + ": null argument");
    ScalarRef sc[ebm::kMaxQuantities];
    if (int rc = resolve_scalars(h, who, nscal, spec, level, sc)) return rc;
    for (int s = 0; s < nscal; ++s)
        if (int rc = check_current(h, sc[s].field, who)) return rc;
    for (int s = 0; s < nscal; ++s)
        if (int rc = make_readable(h, sc[s].field)) return rc;
    if (!dev_out) HIPCHK(h->scalars_out.reserve((size_t)ebm::kMaxQuantities * (size_t)h->ncol));
    ebm::ScalarArgs a = scalar_args(h, nscal, sc);
    a.out = dev_out ? dev_out : h->scalars_out.get();
    a.out_stride = h->ncol;
    const hipStream_t st = main_stream(h);
    return ensemble_close(ebm::launch_column_scalars(a, h->ncol, st), dev_out ? nullptr : host_out, a.out, (size_t)nscal * (size_t)h->ncol, st, who);
}

// ebm_diffusion / ebm_zonal_diffusion: three fields of [ncol][pitch], zero-padded, kept until the handle is destroyed
int get_scratch(ebm_ctx *h) {
    if (h->scratch) return EBM_OK;
    const size_t n = 3 * (size_t)h->ncol * h->pitch;
    DevBuf<double> b;
    HIPCHK(dev_alloc(b, n));
    HIPCHK(hipMemsetAsync(b.get(), 0, sizeof(double) * n, main_stream(h)));       // padding cells stay zero
    h->scratch = std::move(b);
    return EBM_OK;
}

// ebm_update_columns and its _device form (include/ebm_hip.h): every check before anything of the handle changes; then what one
// ebm_set_field per listed field does to the book, minus the conversion to the natural layout (the kernels take the rows where
// they lie); then the innovations of all columns staged from the state as it is at entry, and the product per field — the
// host variant's gain uploaded one field at a time into the handle's one pitch^2 buffer.  Synchronous.
int update_columns(ebm_ctx *h, int nvars, const int *fields, int obs_field, const double *gain, bool gain_on_device, const double *target,
                   double scale, const double *dev_perturb, const double *lo, const double *hi, const char *who) {
    const std::string me(who);
    if (!h) return fail(EBM_ERR_ARG, me + ": null handle");
    if (!fields || !gain || !target) return fail(EBM_ERR_ARG, me + ": null argument");
    if (nvars < 1 || nvars > ebm::kUpdateMaxFields)
        return fail(EBM_ERR_ARG, me + ": nvars = " + std::to_string(nvars) + " is outside 1 ... " + std::to_string(ebm::kUpdateMaxFields));
    for (int v = 0; v < nvars; ++v) {
        if (!h->book.has(fields[v]) || h->book.is_diagnostic(fields[v]))
            return fail(EBM_ERR_ARG, me + ": fields[" + std::to_string(v) + "] is not a prognostic field of this model");
        for (int u = 0; u < v; ++u)
            if (fields[u] == fields[v]) return fail(EBM_ERR_ARG, me + ": field " + field_name(fields[v]) + " is listed twice");
    }
    if (!h->book.has(obs_field) || quantity_of(h->model, obs_field) < 0)
        return fail(EBM_ERR_ARG, me + ": obs_field is not a solution variable of this model");
    if (!std::isfinite(scale)) return fail(EBM_ERR_ARG, me + ": scale is not finite");
    const size_t nlat = (size_t)h->nlat, npitch = (size_t)h->pitch;
    for (size_t i = 0; !gain_on_device && i < (size_t)nvars * nlat * nlat; ++i)
        if (!std::isfinite(gain[i]))
            return fail(EBM_ERR_ARG, me + ": gain[" + std::to_string(i / (nlat * nlat)) + "][" + std::to_string(i / nlat % nlat) + "][" +
                                         std::to_string(i % nlat) + "] is not finite (field " + field_name(fields[i / (nlat * nlat)]) +
                                         ", k = " + std::to_string(i / nlat % nlat) + ", j = " + std::to_string(i % nlat) + ")");
    for (size_t j = 0; j < nlat; ++j)
        if (std::isinf(target[j]))
            return fail(EBM_ERR_ARG, me + ": target[" + std::to_string(j) + "] is infinite (finite, or NaN for no observation)");
    const double inf = HUGE_VAL;
    ebm::UpdateArgs a{};
    for (int v = 0; v < nvars; ++v) {
        a.lo[v] = lo ? lo[v] : -inf;
        a.hi[v] = hi ? hi[v] : inf;
        if (a.lo[v] != a.lo[v] || a.hi[v] != a.hi[v] || a.lo[v] > a.hi[v])
            return fail(EBM_ERR_ARG, me + ": lo[" + std::to_string(v) + "], hi[" + std::to_string(v) + "] are not bounds with lo <= hi (NaN is none; -Inf / +Inf: no bound)");
    }
    if (gain_on_device && reinterpret_cast<uintptr_t>(gain) % 16)
        return fail(EBM_ERR_ARG, me + ": the device gain is not 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(dev_perturb) % 8) return fail(EBM_ERR_ARG, me + ": dev_perturb is not 8-byte aligned");
    if (int rc = check_current(h, obs_field, who)) return rc;
    HIPCHK(hipSetDevice(h->device));
    // device memory first: a failed allocation leaves the book as it was
    ebm_ctx::Update &b = h->update;
    const bool fresh_target = !b.target.get();
    HIPCHK(b.target.reserve(npitch));
    if (!gain_on_device) HIPCHK(b.gain.reserve(npitch * npitch));
    const bool borrowed = (bool)h->scratch;              // the staged innovations: [ncol][pitch], one owner (ebm_runtime.h)
    if (!borrowed) HIPCHK(h->resample.stage.reserve((size_t)h->ncol * npitch));
    // what ebm_set_field does before it writes a prognostic field (phi current where it lies, then no longer derived; no
    // zero-line flag trusted) — not the conversion: the rows are taken in the layout they have
    if (h->model == EBM_MODEL_MIZ)
        if (int rc = state_written_outside(h)) return rc;
    const hipStream_t s = main_stream(h);                // joins the two launch chains: every column's last step has ended
    if (fresh_target) HIPCHK(hipMemsetAsync(b.target.get(), 0, sizeof(double) * npitch, s));
    hipError_t e = hipMemcpyAsync(b.target.get(), target, sizeof(double) * nlat, hipMemcpyHostToDevice, s);
    for (int v = 0; v < nvars; ++v) {
        a.row[v] = h->field[fields[v]];
        if (h->book.held_split(fields[v])) a.split_mask |= 1u << v;
    }
    a.obs = h->field[obs_field];
    a.obs_split = h->book.held_split(obs_field);
    a.target = b.target.get();
    a.perturb = dev_perturb;
    a.d = borrowed ? h->scratch.get() : h->resample.stage.get();
    a.scale = scale;
    a.pitch = (int)h->pitch; a.nlat = h->nlat; a.ncol = h->ncol; a.nvars = nvars; a.threads = h->cfg.threads;
    if (e == hipSuccess) e = ebm::launch_update_innovations(a, s);
    if (gain_on_device) {                                // one launch over a grid z of fields
        a.gain = gain; a.gain_field = (long long)(nlat * nlat); a.gain_row = (long long)nlat;
        if (e == hipSuccess) e = ebm::launch_update_product(a, s);
    } else {
        for (int v = 0; v < nvars && e == hipSuccess; ++v) {
            ebm::UpdateArgs one = a;
            one.row[0] = a.row[v]; one.lo[0] = a.lo[v]; one.hi[0] = a.hi[v]; one.split_mask = (a.split_mask >> v) & 1u; one.nvars = 1;
            one.gain = b.gain.get(); one.gain_field = 0; one.gain_row = h->pitch;
            e = hipMemcpy2DAsync(b.gain.get(), sizeof(double) * npitch, gain + (size_t)v * nlat * nlat, sizeof(double) * nlat,
                                 sizeof(double) * nlat, nlat, hipMemcpyHostToDevice, s);
            if (e == hipSuccess) e = ebm::launch_update_product(one, s);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(who, e);
    for (int v = 0; v < nvars; ++v) h->book.field_set(fields[v]);       // the prognostic state changed: the diagnostics are older
    return EBM_OK;
}

// ebm_spd_solve_device and ebm_kalman_gain_device (include/ebm_hip.h; the kernels and the order of every operation are in
// ebm_gain.hip).  Neither reads or writes a field, the clock or a counter: the book never hears of them.
constexpr long long round_up_block(long long m) { return (m + ebm::kGainBlock - 1) / ebm::kGainBlock * ebm::kGainBlock; }
bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
// the handle's share of a solve of mp unknowns: the block inverses and the flag (with `extra` more words behind it)
int reserve_solve(ebm_ctx *h, long long mp, size_t extra) {
    HIPCHK(h->gain.inv.reserve((size_t)mp * ebm::kGainBlock));
    HIPCHK(h->gain.words.reserve(1 + extra));
    return EBM_OK;
}
// flag = 0, the factorisation, the two solves: enqueued, not awaited
hipError_t enqueue_solve(const ebm::SolveArgs &a, hipStream_t s) {
    hipError_t e = hipMemsetAsync(a.flag, 0, sizeof(int), s);
    if (e == hipSuccess) e = ebm::launch_spd_factor(a, s);
    if (e == hipSuccess) e = ebm::launch_spd_solve(a, s);
    return e;
}

int spd_solve_device(ebm_ctx *h, int m, long long nrhs, double *dev_S, long long lds, double *dev_B, long long ldb, int *info) {
    const std::string me("ebm_spd_solve_device");
    if (!h) return fail(EBM_ERR_ARG, me + ": null handle");
    if (!dev_S || !dev_B || !info) return fail(EBM_ERR_ARG, me + ": null argument");
    if (m < 1 || nrhs < 0) return fail(EBM_ERR_ARG, me + ": m = " + std::to_string(m) + ", nrhs = " + std::to_string(nrhs) + ": expected m >= 1 and nrhs >= 0");
    const long long mp = round_up_block(m);
    if (lds < mp || ldb < mp)
        return fail(EBM_ERR_ARG, me + ": lds = " + std::to_string(lds) + ", ldb = " + std::to_string(ldb) + ": both must be >= m rounded up to 64 = " +
                                     std::to_string(mp) + " (the caller pads S with the identity and B with zeros)");
    if (!aligned16(dev_S) || !aligned16(dev_B)) return fail(EBM_ERR_ARG, me + ": dev_S or dev_B is not 16-byte aligned");
    HIPCHK(hipSetDevice(h->device));
    if (int rc = reserve_solve(h, mp, 0)) return rc;
    const hipStream_t s = main_stream(h);
    ebm::SolveArgs a{dev_S, lds, dev_B, ldb, nrhs, h->gain.inv.get(), h->gain.words.get(), (int)mp};
    int pivot = 0;
    hipError_t e = enqueue_solve(a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(&pivot, a.flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(me, e);
    *info = pivot;
    if (pivot) return fail(EBM_ERR_ARG, me + ": S is not positive definite: pivot " + std::to_string(pivot) + " is not > 0 (info = " + std::to_string(pivot) + ")");
    return EBM_OK;
}

int kalman_gain_device(ebm_ctx *h, int nvars, const double *obs, const double *obs_var, double localize, double factor,
                       const double *dev_Poo, double *const *dev_Pfo, double *dev_gain, int *info) {
    const std::string me("ebm_kalman_gain_device");
    if (!h) return fail(EBM_ERR_ARG, me + ": null handle");
    if (!obs || !obs_var || !dev_Poo || !dev_Pfo || !dev_gain || !info) return fail(EBM_ERR_ARG, me + ": null argument");
    if (nvars < 1 || nvars > ebm::kUpdateMaxFields)
        return fail(EBM_ERR_ARG, me + ": nvars = " + std::to_string(nvars) + " is outside 1 ... " + std::to_string(ebm::kUpdateMaxFields));
    for (int v = 0; v < nvars; ++v) {
        if (!dev_Pfo[v]) return fail(EBM_ERR_ARG, me + ": Pfo_addr[" + std::to_string(v) + "] is null");
        if (!aligned16(dev_Pfo[v])) return fail(EBM_ERR_ARG, me + ": Pfo_addr[" + std::to_string(v) + "] is not 16-byte aligned");
    }
    if (!aligned16(dev_Poo) || !aligned16(dev_gain)) return fail(EBM_ERR_ARG, me + ": dev_Poo or dev_gain is not 16-byte aligned");
    if (!std::isfinite(factor) || !(factor > 0.0)) return fail(EBM_ERR_ARG, me + ": factor is not finite and > 0");
    if (localize != localize) return fail(EBM_ERR_ARG, me + ": localize is NaN (a half-width in x > 0, or <= 0 for no taper)");
    const int nlat = h->nlat;
    std::vector<int> words;                                  // J, padded to mp with 0 (never read), then pos
    std::vector<int> pos((size_t)nlat, -1);
    for (int j = 0; j < nlat; ++j) {
        if (std::isinf(obs[j])) return fail(EBM_ERR_ARG, me + ": obs[" + std::to_string(j) + "] is infinite (finite, or NaN for no observation)");
        if (obs[j] != obs[j]) continue;
        if (!std::isfinite(obs_var[j]) || !(obs_var[j] > 0.0))
            return fail(EBM_ERR_ARG, me + ": obs_var[" + std::to_string(j) + "] is not finite and > 0 at an observed cell");
        pos[(size_t)j] = (int)words.size();
        words.push_back(j);
    }
    const int m = (int)words.size();
    const long long mp = round_up_block(m);
    HIPCHK(hipSetDevice(h->device));
    const size_t gain_words = (size_t)nvars * (size_t)nlat * (size_t)nlat;
    if (m == 0) {                                            // nothing observed: a gain of zeros, no solve
        const hipStream_t s = main_stream(h);
        HIPCHK(hipMemsetAsync(dev_gain, 0, sizeof(double) * gain_words, s));
        HIPCHK(hipStreamSynchronize(s));
        *info = 0;
        return EBM_OK;
    }
    ebm_ctx::Gain &b = h->gain;
    if (int rc = reserve_solve(h, mp, (size_t)mp + (size_t)nlat)) return rc;
    HIPCHK(b.S.reserve((size_t)mp * (size_t)mp));
    HIPCHK(b.B.reserve((size_t)nvars * (size_t)nlat * (size_t)mp));
    HIPCHK(b.obs_var.reserve((size_t)nlat));
    words.resize((size_t)mp, 0);
    words.insert(words.end(), pos.begin(), pos.end());
    for (Event &ev : b.mark)
        if (!ev) HIPCHK(hipEventCreate(ev.out()));
    const hipStream_t s = main_stream(h);                    // joins the two launch chains
    int *const index = b.words.get() + 1;
    // pageable sources (`words`, the caller's obs_var): on every path below the stream is awaited before this returns
    hipError_t e = hipMemcpyAsync(index, words.data(), sizeof(int) * words.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(b.obs_var.get(), obs_var, sizeof(double) * (size_t)nlat, hipMemcpyHostToDevice, s);
    ebm::GainArgs g{};
    g.Poo = dev_Poo;
    for (int v = 0; v < nvars; ++v) g.Pfo[v] = dev_Pfo[v];
    g.x = x_table(h);
    g.obs_var = b.obs_var.get();
    g.index = index; g.pos = index + mp; g.flag = b.words.get();
    g.localize = localize; g.factor = factor;
    g.S = b.S.get(); g.B = b.B.get(); g.gain = dev_gain;
    g.nlat = nlat; g.nvars = nvars; g.m = m; g.mp = (int)mp;
    ebm::SolveArgs a{g.S, mp, g.B, mp, (long long)nvars * nlat, b.inv.get(), b.words.get(), (int)mp};
    int pivot = 0;
    b.timed = false;
    auto mark = [&](int i) { if (e == hipSuccess) e = hipEventRecord(b.mark[i].get(), s); };
    if (e == hipSuccess) e = hipMemsetAsync(a.flag, 0, sizeof(int), s);
    mark(0);
    if (e == hipSuccess) e = ebm::launch_gain_assemble(g, s);
    mark(1);
    if (e == hipSuccess) e = ebm::launch_spd_factor(a, s);
    mark(2);
    if (e == hipSuccess) e = ebm::launch_spd_solve(a, s);
    mark(3);
    if (e == hipSuccess) e = ebm::launch_gain_scatter(g, s);
    mark(4);
    if (e == hipSuccess) e = hipMemcpyAsync(&pivot, a.flag, sizeof(int), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);                       // nothing pending may still read `words` or obs_var
        return hip_fail(me, e);
    }
    b.timed = true;
    *info = pivot;
    if (pivot)
        return fail(EBM_ERR_ARG, me + ": the innovation covariance is not positive definite: pivot " + std::to_string(pivot) +
                                     " is not > 0, at observed latitude " + std::to_string(words[(size_t)pivot - 1]) +
                                     " (a NaN or a negative variance in dev_Poo there?)");
    return EBM_OK;
}

// The parameters of the zonal operator: the handle's vector, or the one set ebm_set_column_params installed
const ebm::Params &zonal_params(const ebm_ctx *h) { return h->sets.n ? h->sets.host[0] : h->p; }
// The zonal tables (ebm_tables::build_zonal_tables) on the device, with the segmented sweep's scratch behind them.  Built on
// first use and whenever nlon changes.
int build_zonal_tables(ebm_ctx *h, int nlon) {
    if (h->zonal.tab && h->zonal.nlon == nlon) return EBM_OK;
    ebm_tables::ZonalHostTables t;
    const int P = (int)h->pitch;
    const char *why = ebm_tables::build_zonal_tables(nlon, h->nlat, P, h->cfg.threads, h->cfg.cells, h->dt, h->xhost.data(),
                                                     zonal_params(h), t);
    if (why) return fail(EBM_ERR_ARG, why);
    const int nmember = h->ncol / nlon;
    const size_t scratch = t.seg == 1 ? 0 : 3 * (size_t)nmember * t.seg * P;
    ebm_ctx::ZonalTables z;
    HIPCHK(dev_alloc(z.tab, t.tab.size() + scratch));
    HIPCHK(hipMemcpy(z.tab.get(), t.tab.data(), sizeof(double) * t.tab.size(), hipMemcpyHostToDevice));
    z.M = z.tab.get(); z.E = z.M + t.chain_rows * P; z.rM = z.E + t.chain_rows * P; z.rE = z.rM + t.red_rows * P;
    z.a = z.rE + t.red_rows * P; z.a2 = z.a + P; z.W = z.a2 + P;
    z.su = z.W + P; z.sg = z.su + scratch / 3; z.sy = z.sg + scratch / 3;
    z.nlon = nlon;
    z.seg = t.seg;
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    h->zonal = std::move(z);
    return EBM_OK;
}
hipError_t zonal_sweep(ebm_ctx *h, const double *T, double *outZ, double *outU) {
    const ebm_ctx::ZonalTables &z = h->zonal;
    const int nmember = h->ncol / z.nlon;
    const double rtheta = zonal_params(h).cw / h->dt;
    if (z.seg == 1)
        return ebm::launch_zonal_sweep(T, outZ, outU, z.M, z.E, z.a, z.W, z.nlon, nmember, (int)h->pitch, rtheta, main_stream(h));
    return ebm::launch_zonal_sweep_segmented(T, outZ, outU, z.M, z.E, z.rM, z.rE, z.a, z.a2, z.W, z.su, z.sg, z.sy, z.nlon,
                                             z.seg, nmember, (int)h->pitch, rtheta, main_stream(h));
}

}  // namespace

extern "C" {

int ebm_set_field(ebm_handle_t h, int field, const double *host) {
    int rc = check_field(h, field, host, "ebm_set_field");
    if (rc) return rc;
    HIPCHK(hipSetDevice(h->device));
    if ((rc = get_copier(h))) return rc;
    const bool prognostic = h->book.is_split_state_field(field);
    if (h->book.is_split_field(field)) {
        rc = ensure_natural(h);                   // the other diagnostic fields keep their values, in the natural layout
        if (rc) return rc;
    }
    if (prognostic && (rc = set_state_layout(h, false))) return rc;     // ... and so do the prognostic ones
    // a caller's Ei, h or phi is honoured as it is: the next step loads phi (any prognostic field counts: when in doubt)
    if (prognostic && (rc = state_written_outside(h))) return rc;
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    HIPCHK(h->copier->wait_all());
    HIPCHK(h->copier->upload(h->field[field], (size_t)h->pitch, host, (size_t)h->nlat, (size_t)h->ncol));
    if (field == EBM_F_T0 && h->model == EBM_MODEL_MIZ) {
        // the stepping kernels carry the warm start as its active set: rebuild it from the new T0
        hipError_t e = ebm::launch_mask_from_t0(base_args(h), h->ncol, h->cfg, main_stream(h));
        if (e != hipSuccess) return hip_fail("mask_from_t0", e);
        HIPCHK(hipStreamSynchronize(main_stream(h)));
    }
    h->book.field_set(field);
    return EBM_OK;
}

int ebm_get_field(ebm_handle_t h, int field, double *host) {
    int rc = open_field(h, field, host, "ebm_get_field");
    return rc ? rc : download_field(h, field, host, "ebm_get_field");
}

int ebm_get_field_as_of(ebm_handle_t h, int field, long long step, double *host) {
    int rc = check_field(h, field, host, "ebm_get_field_as_of");
    if (rc) return rc;
    const long long have = h->book.written_step(field, -2);
    if (have != step)
        return fail(EBM_ERR_STALE, std::string("ebm_get_field_as_of: field ") + field_name(field) + " is not as of step " +
                                       std::to_string(step) + (have == -2 ? " (it has never been written)"
                                                                          : " (it was last written by step " + std::to_string(have) + ")"));
    if ((rc = make_readable(h, field))) return rc;
    return download_field(h, field, host, "ebm_get_field_as_of");
}

int ebm_field_step(ebm_handle_t h, int field, long long *written_step, long long *state_step, int *current) {
    if (!h) return fail(EBM_ERR_ARG, "ebm_field_step: null handle");
    if (!h->book.has(field)) return fail(EBM_ERR_ARG, "ebm_field_step: field not part of this model");
    if (written_step) *written_step = h->book.written_step(field);
    if (state_step) *state_step = h->book.state_step();
    if (current) *current = h->book.is_current(field) ? 1 : 0;
    return EBM_OK;
}

int ebm_hemispheric_mean(ebm_handle_t h, int field, double *out) {
    int rc = open_field(h, field, out, "ebm_hemispheric_mean");
    if (rc) return rc;
    hipError_t e = hemispheric_mean(h, field, h->hm_dev.get());
    if (e == hipSuccess) e = hipMemcpyAsync(out, h->hm_dev.get(), sizeof(double) * (size_t)h->ncol, hipMemcpyDeviceToHost, main_stream(h));
    if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
    if (e != hipSuccess) return hip_fail("ebm_hemispheric_mean", e);
    return EBM_OK;
}

int ebm_hemispheric_mean_device(ebm_handle_t h, int field, double *dev_out) {
    int rc = open_field(h, field, dev_out, "ebm_hemispheric_mean_device");
    if (rc) return rc;
    hipError_t e = hemispheric_mean(h, field, dev_out);
    if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
    if (e != hipSuccess) return hip_fail("ebm_hemispheric_mean_device", e);
    return EBM_OK;
}

int ebm_ensemble_sums(ebm_handle_t h, int nvars, const int *fields, const double *w, const double *center, double *out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::SUMS, ebm::kSumsBlock, center, nullptr, nullptr, 0}, out, nullptr, "ebm_ensemble_sums");
}

int ebm_ensemble_sums_device(ebm_handle_t h, int nvars, const int *fields, const double *w, const double *center, double *dev_out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::SUMS, ebm::kSumsBlock, center, nullptr, nullptr, 0}, nullptr, dev_out, "ebm_ensemble_sums_device");
}

int ebm_ensemble_covariance(ebm_handle_t h, int field_a, int field_b, const double *w, const double *center_a, const double *center_b,
                            double *out) {
    return ensemble_covariance(h, field_a, field_b, w, center_a, center_b, out, nullptr, "ebm_ensemble_covariance");
}

int ebm_ensemble_covariance_device(ebm_handle_t h, int field_a, int field_b, const double *w, const double *center_a,
                                   const double *center_b, double *dev_out) {
    return ensemble_covariance(h, field_a, field_b, w, center_a, center_b, nullptr, dev_out, "ebm_ensemble_covariance_device");
}

int ebm_ensemble_range(ebm_handle_t h, int nvars, const int *fields, const double *w, double *out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::RANGE, ebm::kRangeBlock, nullptr, nullptr, nullptr, 0}, out, nullptr, "ebm_ensemble_range");
}

int ebm_ensemble_range_device(ebm_handle_t h, int nvars, const int *fields, const double *w, double *dev_out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::RANGE, ebm::kRangeBlock, nullptr, nullptr, nullptr, 0}, nullptr, dev_out, "ebm_ensemble_range_device");
}

int ebm_ensemble_histogram(ebm_handle_t h, int nvars, const int *fields, const double *w, int nbins, const double *lo,
                           const double *hi, double *out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::HISTOGRAM, ebm::kHistBlock, nullptr, lo, hi, nbins}, out, nullptr, "ebm_ensemble_histogram");
}

int ebm_ensemble_histogram_device(ebm_handle_t h, int nvars, const int *fields, const double *w, int nbins, const double *lo,
                                  const double *hi, double *dev_out) {
    return ensemble_reduce(h, nvars, fields, w, {EnsembleCall::HISTOGRAM, ebm::kHistBlock, nullptr, lo, hi, nbins}, nullptr, dev_out, "ebm_ensemble_histogram_device");
}

int ebm_column_misfits(ebm_handle_t h, int nvars, const int *fields, int ntargets, const double *target, const double *rw, double *out) {
    return column_misfits(h, nvars, fields, ntargets, target, rw, out, nullptr, "ebm_column_misfits");
}

int ebm_column_misfits_device(ebm_handle_t h, int nvars, const int *fields, int ntargets, const double *target, const double *rw,
                              double *dev_out) {
    return column_misfits(h, nvars, fields, ntargets, target, rw, nullptr, dev_out, "ebm_column_misfits_device");
}

int ebm_update_columns(ebm_handle_t h, int nvars, const int *fields, int obs_field, const double *gain, const double *target,
                       double scale, const double *dev_perturb, const double *lo, const double *hi) {
    return update_columns(h, nvars, fields, obs_field, gain, false, target, scale, dev_perturb, lo, hi, "ebm_update_columns");
}

int ebm_update_columns_device(ebm_handle_t h, int nvars, const int *fields, int obs_field, const double *dev_gain, const double *target,
                              double scale, const double *dev_perturb, const double *lo, const double *hi) {
    return update_columns(h, nvars, fields, obs_field, dev_gain, true, target, scale, dev_perturb, lo, hi, "ebm_update_columns_device");
}

int ebm_spd_solve_device(ebm_handle_t h, int m, long long nrhs, double *dev_S, long long lds, double *dev_B, long long ldb, int *info) {
    return spd_solve_device(h, m, nrhs, dev_S, lds, dev_B, ldb, info);
}

int ebm_kalman_gain_device(ebm_handle_t h, int nvars, const double *obs, const double *obs_var, double localize, double factor,
                           const double *dev_Poo, double **Pfo_addr, double *dev_gain, int *info) {
    return kalman_gain_device(h, nvars, obs, obs_var, localize, factor, dev_Poo, Pfo_addr, dev_gain, info);
}

int ebm_kalman_gain_phases(ebm_handle_t h, float *elapsed_ms) {
    if (!h || !elapsed_ms) return fail(EBM_ERR_ARG, "ebm_kalman_gain_phases: null argument");
    if (!h->gain.timed) return fail(EBM_ERR_ARG, "ebm_kalman_gain_phases: no ebm_kalman_gain_device call of this handle has run a solve yet");
    HIPCHK(hipSetDevice(h->device));
    for (int i = 0; i < 4; ++i) HIPCHK(hipEventElapsedTime(elapsed_ms + i, h->gain.mark[i].get(), h->gain.mark[i + 1].get()));
    return EBM_OK;
}

int ebm_column_scalars(ebm_handle_t h, int nscal, const int *spec, const double *level, double *out) {
    return column_scalars(h, nscal, spec, level, out, nullptr, "ebm_column_scalars");
}

int ebm_column_scalars_device(ebm_handle_t h, int nscal, const int *spec, const double *level, double *dev_out) {
    return column_scalars(h, nscal, spec, level, nullptr, dev_out, "ebm_column_scalars_device");
}

int ebm_get_field_device(ebm_handle_t h, int field, double *dev_out) {
    int rc = open_field(h, field, dev_out, "ebm_get_field_device");
    if (rc) return rc;
    HIPCHK(copy_rows(h, dev_out, h->nlat, h->field[field], h->pitch, hipMemcpyDeviceToDevice));
    HIPCHK(hipStreamSynchronize(main_stream(h)));
    return EBM_OK;
}

int ebm_field_device_ptr(ebm_handle_t h, int field, double **dptr, long long *pitch) {
    int rc = open_field(h, field, dptr, "ebm_field_device_ptr");
    if (rc) return rc;
    // (the caller may write through the view of a prognostic field)
    if (h->book.is_split_state_field(field) && (rc = state_written_outside(h))) return rc;
    // the view is of the natural layout as of this call
    if (h->book.is_split_field(field) || h->book.is_split_state_field(field)) HIPCHK(hipStreamSynchronize(main_stream(h)));
    *dptr = h->field[field];
    if (pitch) *pitch = h->pitch;
    return EBM_OK;
}

int ebm_diffusion(ebm_handle_t h, const double *temp, const double *base, double *out) {
    if (!h || !temp || !out) return fail(EBM_ERR_ARG, "ebm_diffusion: null argument");
    if (h->model != EBM_MODEL_MIZ)
        return fail(EBM_ERR_ARG, "ebm_diffusion: needs a MIZ handle (the classic model carries get_diffop unscaled inside kappa, src/classic.jl:21)");
    HIPCHK(hipSetDevice(h->device));
    const size_t npitch = (size_t)h->ncol * h->pitch;
    int rc = get_scratch(h);                             // temp | base | out
    if (rc) return rc;
    double *buf = h->scratch.get();
    hipError_t e = copy_rows(h, buf, h->pitch, temp, h->nlat, hipMemcpyHostToDevice);
    if (e == hipSuccess && base) e = copy_rows(h, buf + npitch, h->pitch, base, h->nlat, hipMemcpyHostToDevice);
    const ebm::StepArgs a = base_args(h);                // the column's parameter set (ebm_set_column_params)
    if (e == hipSuccess)
        e = ebm::launch_diffusion(buf, base ? buf + npitch : nullptr, buf + 2 * npitch, a.geom, a.gstride, a.p, a.pset,
                                  a.set_stride, h->grid, (int)h->pitch, h->nlat, h->ncol, main_stream(h));
    if (e == hipSuccess) e = copy_rows(h, out, h->nlat, buf + 2 * npitch, h->pitch, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
    if (e != hipSuccess) return hip_fail("ebm_diffusion", e);
    return EBM_OK;
}

int ebm_zonal_diffusion(ebm_handle_t h, int nlon, const double *temp, double *out_U, double *out_Z) {
    if (!h || !temp || (!out_U && !out_Z)) return fail(EBM_ERR_ARG, "ebm_zonal_diffusion: null argument");
    if (h->model != EBM_MODEL_MIZ) return fail(EBM_ERR_ARG, "ebm_zonal_diffusion: needs a MIZ handle (cw and D are MIZ parameters of this operator)");
    if (nlon < 3) return fail(EBM_ERR_ARG, "ebm_zonal_diffusion: needs nlon >= 3 (longitudes per member)");
    if (h->ncol % nlon) return fail(EBM_ERR_ARG, "ebm_zonal_diffusion: the handle's column count must be a multiple of nlon");
    if (h->sets.n > 1)
        return fail(EBM_ERR_UNSUPPORTED, "ebm_zonal_diffusion: needs one parameter set (its tables come from one D and one cw; "
                                         "ebm_set_column_params installed " + std::to_string(h->sets.n) + ")");
    HIPCHK(hipSetDevice(h->device));
    int rc = build_zonal_tables(h, nlon);
    if (rc) return rc;
    const size_t npitch = (size_t)h->ncol * h->pitch;
    if ((rc = get_scratch(h))) return rc;                // temp | U | Z
    double *buf = h->scratch.get();
    hipError_t e = hipMemsetAsync(buf, 0, sizeof(double) * npitch, main_stream(h));            // (an earlier call left it permuted)
    if (e == hipSuccess) e = copy_rows(h, buf, h->pitch, temp, h->nlat, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = ebm::launch_split_fields(buf, 0, 1, h->ncol, h->cfg, main_stream(h));
    if (e == hipSuccess) e = zonal_sweep(h, buf, buf + 2 * npitch, buf + npitch);
    if (e == hipSuccess) e = ebm::launch_unsplit_fields(buf + npitch, (long long)npitch, 2, h->ncol, h->cfg, main_stream(h));
    if (e == hipSuccess && out_U) e = copy_rows(h, out_U, h->nlat, buf + npitch, h->pitch, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out_Z) e = copy_rows(h, out_Z, h->nlat, buf + 2 * npitch, h->pitch, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipStreamSynchronize(main_stream(h));
    if (e != hipSuccess) return hip_fail("ebm_zonal_diffusion", e);
    return EBM_OK;
}

}  // extern "C"
