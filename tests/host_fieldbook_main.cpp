// Stand-alone walk of csrc/ebm_fieldbook.h for tests/test_host_fieldbook.py and tests/test_gpu_state_layout.py: no HIP, no GPU.
//   walk DEPTH              every sequence of 1 .. DEPTH events of the alphabet below, for each of the four shapes; prints the
//                           counts of sequences, passes, events and deriving-kernel decisions per shape
//   replay SHAPE EVENT...   one sequence; prints the passes of every event and the final n_conversions
// Exit status 1 and a line "VIOLATION ..." naming the sequence and the first invariant that broke.
//
// The program plays the library's calls as events: each performs the preamble the real call performs (the order is that of
// csrc/ebm_fields.hip, ebm_drive.hip and ebm_columns.hip) — it asks the book, runs the passes the book names and reports
// them done — and then "runs the kernel" on Mem, a model of device memory that is written here and takes nothing from the
// header: where each field lies in which layout, which state each diagnostic field belongs to, whether memory holds the
// current phi, and whether phi is the function of Ei and h or a caller's value.  The kernels of the model state what they
// expect of memory (need); after every event the book's answers are compared with the model's truth (check).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../energybalancemodel.jl_amd/csrc/ebm_fieldbook.h"

using ebm_rt::FieldBook;
using ebm_rt::Pass;

namespace {

struct Shape { const char *name; int model; bool cells4, derive; };
const Shape kShapes[4] = {{"miz4_derive", EBM_MODEL_MIZ, true, true}, {"miz4_imex", EBM_MODEL_MIZ, true, false},
                          {"miz2", EBM_MODEL_MIZ, false, false}, {"classic", EBM_MODEL_CLASSIC, true, false}};
enum Event { STEP_STATE, STEP_DIAG, STEP_SAVE, GRAPH, FUSED, FUSED_DIAG, FUSED_ACTIVE, GET_PROG, GET_DIAG, GET_T0, SET_PROG,
             SET_DIAG, VIEW_PROG, MEAN, RESAMPLE, EXPORT, IMPORT, PARAMS, SUMS_PHI, SUMS_OTHER, N_EVENTS };
const char *const kEventName[N_EVENTS] = {"step_state", "step_diag", "step_save", "graph", "fused", "fused_diag", "fused_active",
                                          "get_prog", "get_diag", "get_T0", "set_prog", "set_diag", "view_prog", "mean",
                                          "resample", "export", "import", "params", "sums_phi", "sums_other"};
const char *const kPassName[6] = {"none", "split_state", "unsplit_state", "unsplit_state_form_phi", "restore_phi", "unsplit_diag"};
constexpr int kGraphSteps = 64;     // csrc/ebm_drive.hip

// the model's own knowledge of the fields (include/ebm_hip.h), not the header's
bool t_miz(const Shape &s) { return s.model == EBM_MODEL_MIZ; }
bool t_has(const Shape &s, int f) {
    return t_miz(s) ? f <= EBM_F_T : (f == EBM_F_E || f == EBM_F_Tg || f == EBM_F_T || f == EBM_F_h);
}
bool t_diag(const Shape &s, int f) { return t_miz(s) ? f >= EBM_F_T0 : (f == EBM_F_T || f == EBM_F_h); }
bool t_prog5(const Shape &s, int f) { return t_miz(s) && f <= EBM_F_phi; }
bool t_diag5(const Shape &s, int f) { return t_miz(s) && f >= EBM_F_Tw && f <= EBM_F_T; }
bool t_two_layouts(const Shape &s) { return t_miz(s) && s.cells4; }

struct Mem {
    bool split[EBM_F_COUNT] = {};
    long long belongs[EBM_F_COUNT], wstep[EBM_F_COUNT];   // diagnostic fields: the state they belong to (-1: none), its step
    long long state = 0, state_step = -1;                 // the present prognostic state (a fresh number per change), its step
    bool phi_in_memory = true;                            // memory holds the current phi
    bool phi_is_function = true;                          // phi == concentration(Ei, h) under the present parameters
    long long conversions = 0;
    Mem() {
        for (int f = 0; f < EBM_F_COUNT; ++f) belongs[f] = wstep[f] = -1;
        belongs[EBM_F_T0] = 0;                            // the warm start is zero, as the reference's
    }
};

struct World {
    const Shape *sh;
    FieldBook book;
    Mem mem;
    long long clock = 0;
    bool graph_built = false, graph_derives = false;
    int npass = 0;
    explicit World(const Shape &s) : sh(&s), book(s.model, s.model == EBM_MODEL_MIZ && s.cells4, s.derive) {}
};

struct Stats { long long sequences, pass[6], event[N_EVENTS], refused_event[N_EVENTS], chosen, not_chosen; } g_stats;
int g_seq[64], g_len = 0;
bool g_trace = false;

void need(const World &w, bool ok, const char *what) {
    if (ok) return;
    std::printf("VIOLATION shape=%s after:", w.sh->name);
    for (int i = 0; i < g_len; ++i) std::printf(" %s", kEventName[g_seq[i]]);
    std::printf(": %s\n", what);
    std::exit(1);
}
bool truth_current(const World &w, int f) { return !t_diag(*w.sh, f) || w.mem.belongs[f] == w.mem.state; }

// ---- the executor of the passes on the model
void exec(World &w, Pass p) {
    if (p == Pass::NONE) return;
    const Shape &s = *w.sh;
    Mem &m = w.mem;
    ++w.npass;
    ++g_stats.pass[(int)p];
    if (g_trace) std::printf(" %s", kPassName[(int)p]);
    need(w, t_two_layouts(s), "a pass on a handle with one layout");
    const bool state_pass = p == Pass::SPLIT_STATE || p == Pass::UNSPLIT_STATE || p == Pass::UNSPLIT_STATE_FORM_PHI;
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        if (state_pass && t_prog5(s, f)) {
            need(w, m.split[f] == (p != Pass::SPLIT_STATE), "state pass: the fields are not in the layout it converts from");
            m.split[f] = p == Pass::SPLIT_STATE;
        }
        if (p == Pass::UNSPLIT_DIAG && t_diag5(s, f)) {
            need(w, m.split[f], "un-split of diagnostic fields that lie natural");
            m.split[f] = false;
        }
    }
    if (p == Pass::SPLIT_STATE || p == Pass::UNSPLIT_STATE) need(w, m.phi_in_memory, "a stale phi field moved instead of formed");
    if (p == Pass::UNSPLIT_STATE_FORM_PHI || p == Pass::RESTORE_PHI) {
        need(w, m.phi_is_function, "phi formed from Ei and h over a caller's value");
        m.phi_in_memory = true;
    }
    if (state_pass) m.conversions += 1;
    w.book.done(p);
}

// ---- the kernels of the model
void wrote_diag(World &w, bool split) {
    for (int f = 0; f < EBM_F_COUNT; ++f)
        if (t_has(*w.sh, f) && t_diag(*w.sh, f)) {
            w.mem.belongs[f] = w.mem.state;
            w.mem.wstep[f] = w.mem.state_step;
            if (t_diag5(*w.sh, f)) w.mem.split[f] = split;
        }
}
void one_step_kernel(World &w, int mode, bool wd, bool derived, int nsteps) {
    const Shape &s = *w.sh;
    Mem &m = w.mem;
    for (int f = 0; f < EBM_F_COUNT; ++f)
        if (t_prog5(s, f)) need(w, m.split[f] == t_two_layouts(s), "one-step kernel: the prognostic fields are not in its layout");
    if (derived) {
        need(w, s.derive && mode == ebm::OUT_STATE, "a deriving kernel the handle does not have");
        need(w, m.phi_is_function, "the deriving kernel over a caller's phi");
    } else if (t_miz(s)) {
        need(w, m.phi_in_memory, "one-step kernel loads a stale phi");
    }
    m.state += 1;
    m.state_step = w.clock + nsteps - 1;
    if (t_miz(s)) { m.phi_in_memory = !derived; m.phi_is_function = true; }
    if (wd) wrote_diag(w, t_two_layouts(s));
}
void fused_kernel(World &w, bool wd, bool all_columns, int nsteps) {
    const Shape &s = *w.sh;
    Mem &m = w.mem;
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        if (t_prog5(s, f)) need(w, !m.split[f], "fused kernel: the prognostic fields are not natural");
        if (wd && !all_columns && t_diag5(s, f)) need(w, !m.split[f], "diagnostic rows of two layouts in one field");
    }
    if (t_miz(s)) need(w, m.phi_in_memory, "fused kernel loads a stale phi");
    m.state += 1;
    m.state_step = w.clock + nsteps - 1;
    if (all_columns) m.phi_is_function = true;
    if (wd) wrote_diag(w, false);
}
void read_as_it_lies(World &w, int f, bool check_held) {
    need(w, truth_current(w, f), "a stale field is read");
    if (check_held) need(w, w.book.held_split(f) == w.mem.split[f], "a reader of the rows as they lie is told the wrong layout");
    if (f == EBM_F_phi && t_miz(*w.sh)) need(w, w.mem.phi_in_memory, "phi read from memory while it is not current there");
}
void read_natural(World &w, int f) {
    need(w, !w.mem.split[f], "a reader of the natural layout finds the field pair-split");
    read_as_it_lies(w, f, false);
}

// ---- the library's calls
// launch_step + record_launches (ebm_drive.hip)
void launch_step(World &w, int mode, bool wd, int nsteps, bool active) {
    const bool one_step = mode == ebm::OUT_STATE || mode == ebm::OUT_DIAG || mode == ebm::OUT_SAVE;
    const bool derived = w.book.step_derives_phi(mode, false);
    if (mode == ebm::OUT_STATE) ++(derived ? g_stats.chosen : g_stats.not_chosen);
    if (one_step && !derived) exec(w, w.book.phi_readable());
    exec(w, w.book.state_layout(one_step));
    if (one_step) one_step_kernel(w, mode, wd, derived, nsteps);
    else fused_kernel(w, wd, !active, nsteps);
    w.clock += nsteps;
    w.book.steps(nsteps, w.clock - 1, wd, one_step && w.sh->cells4, derived, !active);
}
// ebm_run with graph replay, 2 kGraphSteps steps
void run_graph(World &w) {
    if (!w.graph_built) {                                 // build_graph
        exec(w, w.book.state_layout(true));
        w.graph_derives = w.book.step_derives_phi(ebm::OUT_STATE, true);
        need(w, !w.graph_derives || w.sh->derive, "a deriving kernel captured that the handle does not have");
        w.graph_built = true;
    }
    int s = 0;
    if (w.book.replay_needs_a_direct_step()) { launch_step(w, ebm::OUT_STATE, false, 1, false); s = 1; }
    for (; s + kGraphSteps <= 2 * kGraphSteps; s += kGraphSteps) {
        exec(w, w.book.state_layout(true));
        one_step_kernel(w, ebm::OUT_STATE, false, w.graph_derives, kGraphSteps);
        w.clock += kGraphSteps;
        w.book.steps(kGraphSteps, w.clock - 1, false, false, w.book.step_derives_phi(ebm::OUT_STATE, true), true);
    }
    for (; s < 2 * kGraphSteps; ++s) launch_step(w, ebm::OUT_STATE, false, 1, false);
}
// check_field, check_current, make_readable (ebm_fields.hip); false: the call is refused
bool open_field(World &w, int f, bool quantity = false) {
    if (!w.book.has(f) || (quantity && ebm_rt::quantity_of(w.sh->model, f) < 0)) return false;
    if (!w.book.is_current(f)) {
        need(w, !truth_current(w, f), "a current field is refused as stale");
        return false;
    }
    return true;
}
void make_readable(World &w, int f) {
    if (w.book.is_split_state_field(f)) exec(w, w.book.state_layout(false));
    else if (w.book.is_split_field(f)) exec(w, w.book.diag_layout_natural());
}
void state_written_outside(World &w) {
    exec(w, w.book.phi_readable());
    w.book.written_outside();
    if (t_miz(*w.sh)) {
        need(w, w.mem.phi_in_memory, "Ei, h or the parameters change while phi is not stored");
        w.mem.phi_is_function = false;
    }
}
void natural_layout(World &w, bool diagnostics_too) {
    if (diagnostics_too) exec(w, w.book.diag_layout_natural());
    exec(w, w.book.state_layout(false));
}
void exchange_rows(World &w) {
    for (int f = 0; f < EBM_F_COUNT; ++f)
        if (w.book.current_mask() >> f & 1u) read_as_it_lies(w, f, true);
}

// one event; false: the call was refused (stale, or not a field of the model)
bool play(World &w, int ev) {
    const Shape &s = *w.sh;
    const int prog = t_miz(s) ? EBM_F_phi : EBM_F_E, written = t_miz(s) ? EBM_F_h : EBM_F_E, diag = EBM_F_T;
    switch (ev) {
        case STEP_STATE: launch_step(w, ebm::OUT_STATE, false, 1, false); return true;
        case STEP_DIAG: launch_step(w, ebm::OUT_DIAG, true, 1, false); return true;
        case STEP_SAVE:      // ebm_integrate, one launch per step, a year of three steps, the annual mean only
            launch_step(w, ebm::OUT_SAVE, false, 1, false);
            launch_step(w, ebm::OUT_SAVE, false, 1, false);
            launch_step(w, ebm::OUT_SAVE, true, 1, false);
            return true;
        case GRAPH: run_graph(w); return true;
        case FUSED: launch_step(w, ebm::OUT_LOOP, false, 4, false); launch_step(w, ebm::OUT_LOOP, false, 4, false); return true;
        case FUSED_DIAG: launch_step(w, ebm::OUT_LOOP, false, 4, false); launch_step(w, ebm::OUT_LOOP, true, 4, false); return true;
        case FUSED_ACTIVE:   // ebm_run_until on a diagnostic field, one round of two launches
            natural_layout(w, true);
            launch_step(w, ebm::OUT_LOOP, false, 4, true);
            launch_step(w, ebm::OUT_LOOP, true, 4, true);
            natural_layout(w, true);
            read_natural(w, diag);
            return true;
        case GET_PROG: case GET_DIAG: case GET_T0: case MEAN: {
            const int f = ev == GET_DIAG ? diag : ev == GET_T0 ? EBM_F_T0 : prog;
            if (!open_field(w, f)) return false;
            make_readable(w, f);
            read_natural(w, f);
            return true;
        }
        case SET_PROG: case SET_DIAG: {
            const int f = ev == SET_PROG ? written : diag;
            if (w.book.is_split_field(f)) exec(w, w.book.diag_layout_natural());
            if (w.book.is_split_state_field(f)) { exec(w, w.book.state_layout(false)); state_written_outside(w); }
            need(w, !w.mem.split[f], "a field is set while it lies pair-split");
            if (t_diag(s, f)) { w.mem.belongs[f] = w.mem.state; w.mem.wstep[f] = w.mem.state_step; }
            else w.mem.state += 1;
            w.book.field_set(f);
            return true;
        }
        case VIEW_PROG:      // (taking the view writes nothing; the caller may write later)
            if (!open_field(w, prog)) return false;
            make_readable(w, prog);
            if (w.book.is_split_state_field(prog)) state_written_outside(w);
            read_natural(w, prog);
            return true;
        case RESAMPLE:
            state_written_outside(w);
            for (int f = 0; f < EBM_F_COUNT; ++f)
                if (w.book.current_mask() >> f & 1u) read_as_it_lies(w, f, false);
            return true;
        case EXPORT: exec(w, w.book.phi_readable()); exchange_rows(w); return true;
        case IMPORT:         // of what an export of this moment returned
            exec(w, w.book.phi_readable());
            exchange_rows(w);
            state_written_outside(w);
            exchange_rows(w);
            return true;
        case PARAMS: state_written_outside(w); w.graph_built = false; return true;
        case SUMS_PHI: case SUMS_OTHER: {
            const int f = ev == SUMS_PHI ? EBM_F_phi : diag;
            if (!open_field(w, f, true)) return false;
            if (f == EBM_F_phi && t_miz(s)) exec(w, w.book.phi_readable());
            read_as_it_lies(w, f, true);
            return true;
        }
    }
    return false;
}

// the book's answers against the model's truth
void check(const World &w) {
    const Shape &s = *w.sh;
    const FieldBook &b = w.book;
    need(w, b.phi_stored() || b.state_split(), "phi is not stored while the state is natural");
    need(w, b.phi_stored() == w.mem.phi_in_memory || !t_miz(s), "phi_stored is not what memory holds");
    unsigned mask = 0;
    for (int f = 0; f < EBM_F_COUNT; ++f) {
        need(w, b.has(f) == t_has(s, f), "has(f)");
        if (!t_has(s, f)) continue;
        need(w, b.is_diagnostic(f) == t_diag(s, f), "is_diagnostic(f)");
        need(w, b.is_current(f) == truth_current(w, f), "is_current(f) is not the model's truth");
        need(w, b.held_split(f) == w.mem.split[f], "held_split(f) is not the model's layout");
        need(w, b.written_step(f) == (!t_diag(s, f) ? w.mem.state_step : w.mem.belongs[f] < 0 ? -1 : w.mem.wstep[f]),
             "written_step(f) is not the step the field belongs to");
        if (truth_current(w, f)) mask |= 1u << f;
    }
    need(w, b.current_mask() == mask, "current_mask is not the model's");
    need(w, b.state_step() == w.mem.state_step, "state_step");
    need(w, b.conversions() == w.mem.conversions, "n_conversions is not the number of split and un-split passes executed");
}

void walk(const World &w, int depth) {
    for (int ev = 0; ev < N_EVENTS; ++ev) {
        World c = w;
        g_seq[g_len++] = ev;
        ++g_stats.sequences;
        ++(play(c, ev) ? g_stats.event : g_stats.refused_event)[ev];
        check(c);
        if (ev <= FUSED_ACTIVE) {                         // a step event again: the state already fits it
            World r = c;
            r.npass = 0;
            g_seq[g_len++] = ev;
            play(r, ev);
            need(r, r.npass == 0, "the repeat of a step event asked for a pass");
            check(r);
            --g_len;
        }
        if (depth > 1) walk(c, depth - 1);
        --g_len;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "walk")) {
        const int depth = std::atoi(argv[2]);
        if (depth < 1 || depth > 16) return 2;
        for (const Shape &s : kShapes) {
            g_stats = Stats{};
            World w(s);
            check(w);
            walk(w, depth);
            std::printf("shape %s sequences %lld chosen %lld not_chosen %lld\n", s.name, g_stats.sequences, g_stats.chosen, g_stats.not_chosen);
            for (int p = 1; p < 6; ++p) std::printf("pass %s %lld\n", kPassName[p], g_stats.pass[p]);
            for (int e = 0; e < N_EVENTS; ++e) std::printf("event %s %lld refused %lld\n", kEventName[e], g_stats.event[e], g_stats.refused_event[e]);
        }
        return 0;
    }
    if (argc >= 3 && !std::strcmp(argv[1], "replay")) {
        const Shape *s = nullptr;
        for (const Shape &k : kShapes) if (!std::strcmp(k.name, argv[2])) s = &k;
        if (!s) { std::fprintf(stderr, "unknown shape %s\n", argv[2]); return 2; }
        g_trace = true;
        World w(*s);
        for (int i = 3; i < argc && g_len < 63; ++i) {
            int ev = 0;
            while (ev < N_EVENTS && std::strcmp(kEventName[ev], argv[i])) ++ev;
            if (ev == N_EVENTS) { std::fprintf(stderr, "unknown event %s\n", argv[i]); return 2; }
            g_seq[g_len++] = ev;
            std::printf("%s:", argv[i]);
            const bool done = play(w, ev);
            std::printf("%s\n", done ? "" : " (refused)");
            check(w);
        }
        std::printf("n_conversions %lld\n", w.book.conversions());
        return 0;
    }
    std::fprintf(stderr, "usage: %s walk DEPTH | replay SHAPE EVENT...\n", argv[0]);
    return 2;
}
