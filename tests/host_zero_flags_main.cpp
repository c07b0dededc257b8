// Stand-alone walk of the zero-line rule of csrc/ebm_fieldbook.h (zero_flags_trusted) for tests/test_host_zero_flags.py: no
// HIP, no GPU.  The companion of tests/host_fieldbook_main.cpp, which walks validity, layout and phi.
//   walk DEPTH              every sequence of 1 .. DEPTH events of the alphabet below, on a handle that elides zero lines and
//                           on one that does not; prints the counts of sequences, clears, eliding launches and skipped stores
//   replay EVENT...         one sequence on the eliding handle; prints per event whether the flags were cleared and whether the
//                           book trusts them afterwards
// Exit status 1 and a line "VIOLATION ..." naming the sequence and the invariant that broke.
//
// The model of device memory is written here and takes nothing from the header.  A handle of kCols columns; of every column
// two groups of cells, each of which is all zero bits or not.  In the pair-split layout group g fills line g of the column;
// in the natural layout every line holds cells of both groups, so it is zero only if both are.  One flag per line, as on the
// device.  The eliding kernel is played as csrc/ebm_miz_step.h states it: a flagged line is not loaded and taken as zero —
// which must be what memory holds (THE invariant) — and a line whose new values are zero is not stored if its flag was set;
// the new flag is whether the new values are zero.  Every other writer writes what it likes and knows nothing of the flags.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../energybalancemodel.jl_amd/csrc/ebm_fieldbook.h"

using ebm_rt::FieldBook;
using ebm_rt::Pass;

namespace {

constexpr int kCols = 2, kGraphSteps = 64;
enum Event { STEP, STEP_FREEZE, STEP_CHAIN0, STEP_DIAG, GRAPH, FUSED, GET_PROG, SET_PROG, VIEW_PROG, RESAMPLE, IMPORT, PARAMS,
             SUMS_PHI, N_EVENTS };
const char *const kEventName[N_EVENTS] = {"step", "step_freeze", "step_chain0", "step_diag", "graph", "fused", "get_prog",
                                          "set_prog", "view_prog", "resample", "import", "params", "sums_phi"};

struct Mem {
    bool split = false;               // the layout the prognostic fields lie in
    bool zero[kCols][2];              // group g of column c is all zero bits (the VALUE of the state)
    bool flag[kCols][2] = {};         // the device's flag of line g of column c
    Mem() { for (auto &c : zero) c[0] = c[1] = true; }     // ebm_create: the state is zero, the flags clear
    // what HBM holds in line l of column c, in the present layout
    bool line_zero(int c, int l) const { return split ? zero[c][l] : (zero[c][0] && zero[c][1]); }
};

struct World {
    FieldBook book;
    Mem mem;
    long long clock = 0;
    int melt = 0;                     // the model's "physics": which groups the next step leaves zero
    explicit World(bool elide) : book(EBM_MODEL_MIZ, true, true, elide) {}
};

struct Stats { long long sequences, clears, eliding, plain, skipped_stores, skipped_loads; } g_stats;
int g_seq[64], g_len = 0;
bool g_cleared = false;

void need(bool ok, const char *what) {
    if (ok) return;
    std::printf("VIOLATION after:");
    for (int i = 0; i < g_len; ++i) std::printf(" %s", kEventName[g_seq[i]]);
    std::printf(": %s\n", what);
    std::exit(1);
}

void exec(World &w, Pass p) {
    if (p == Pass::NONE) return;
    if (p == Pass::SPLIT_STATE) w.mem.split = true;
    if (p == Pass::UNSPLIT_STATE || p == Pass::UNSPLIT_STATE_FORM_PHI) w.mem.split = false;
    w.book.done(p);
}
// clear_untrusted_zero_flags (ebm_drive.hip)
void clear_untrusted(World &w) {
    if (!w.book.zero_flags_need_clear()) return;
    std::memset(w.mem.flag, 0, sizeof(w.mem.flag));
    w.book.zero_flags_cleared();
    ++g_stats.clears;
    g_cleared = true;
}
// the step's new values of column c: a pattern that walks through freeze-up and melt of both groups
void new_values(World &w, int c, bool freeze, bool out[2]) {
    const int k = freeze ? 3 : (w.melt + c) & 3;
    out[0] = !(k & 1);
    out[1] = !(k & 2);
}
void one_step_kernel(World &w, bool eliding, bool freeze, int first, int count) {
    Mem &m = w.mem;
    need(m.split, "one-step kernel: the prognostic fields are not in its layout");
    for (int c = first; c < first + count; ++c) {
        bool nv[2];
        new_values(w, c, freeze, nv);
        for (int l = 0; l < 2; ++l) {
            if (!eliding) { m.zero[c][l] = nv[l]; continue; }
            if (m.flag[c][l]) {
                need(m.line_zero(c, l), "a set flag over a line that does not hold zero bits: the kernel steps from a wrong state");
                ++g_stats.skipped_loads;
            }
            if (m.flag[c][l] && nv[l]) ++g_stats.skipped_stores;     // memory keeps what it holds: zero, as checked above
            else m.zero[c][l] = nv[l];
            m.flag[c][l] = nv[l];
        }
    }
    ++(eliding ? g_stats.eliding : g_stats.plain);
}
// launch_step + record_launches (ebm_drive.hip); chain0: the launch of the first of two chains alone (column 0)
void launch_step(World &w, int mode, bool freeze = false, bool chain0 = false) {
    const bool one_step = mode != ebm::OUT_LOOP;
    const bool derived = w.book.step_derives_phi(mode, false), zl = w.book.step_elides_zero_lines(mode, false);
    if (one_step && !derived) exec(w, w.book.phi_readable());
    exec(w, w.book.state_layout(one_step));
    if (zl) clear_untrusted(w);
    if (one_step) one_step_kernel(w, zl, freeze, 0, chain0 ? 1 : kCols);
    else {                                                // the fused kernels: natural layout, every line stored
        need(!w.mem.split, "fused kernel: the prognostic fields are not natural");
        for (int c = 0; c < kCols; ++c) new_values(w, c, false, w.mem.zero[c]);
    }
    w.melt += 1;
    w.clock += 1;
    w.book.steps(1, w.clock - 1, mode == ebm::OUT_DIAG, one_step, derived, true, zl);
}
void run_graph(World &w) {                                // ebm_run with graph replay: a direct step if phi is a caller's, one replay
    exec(w, w.book.state_layout(true));                   // build_graph
    if (w.book.replay_needs_a_direct_step()) launch_step(w, ebm::OUT_STATE);
    exec(w, w.book.state_layout(true));
    const bool zl = w.book.step_elides_zero_lines(ebm::OUT_STATE, true);
    if (zl) clear_untrusted(w);
    for (int i = 0; i < 2; ++i) { one_step_kernel(w, zl, false, 0, kCols); w.melt += 1; }     // (two of the kGraphSteps nodes)
    w.clock += kGraphSteps;
    w.book.steps(kGraphSteps, w.clock - 1, false, false, w.book.step_derives_phi(ebm::OUT_STATE, true), true, zl);
}
void state_written_outside(World &w) {
    exec(w, w.book.phi_readable());
    w.book.state_written_outside();
}

void play(World &w, int ev) {
    Mem &m = w.mem;
    switch (ev) {
        case STEP: launch_step(w, ebm::OUT_STATE); return;
        case STEP_FREEZE: launch_step(w, ebm::OUT_STATE, true); return;
        case STEP_CHAIN0: launch_step(w, ebm::OUT_STATE, false, true); return;
        case STEP_DIAG: launch_step(w, ebm::OUT_DIAG); return;
        case GRAPH: run_graph(w); return;
        case FUSED: launch_step(w, ebm::OUT_LOOP); return;
        case GET_PROG: exec(w, w.book.state_layout(false)); return;
        case SET_PROG:       // one icy cell into group 0 of the last column
            exec(w, w.book.state_layout(false));
            state_written_outside(w);
            m.zero[kCols - 1][0] = false;
            w.book.field_set(EBM_F_h);
            return;
        case VIEW_PROG:      // the caller writes through the view at once
            exec(w, w.book.state_layout(false));
            state_written_outside(w);
            m.zero[0][1] = false;
            return;
        case RESAMPLE: case IMPORT:     // rows copied as they lie, in whatever layout: column 0 takes a state without a zero
            state_written_outside(w);
            m.zero[0][0] = m.zero[0][1] = false;
            return;
        case PARAMS: state_written_outside(w); return;
        case SUMS_PHI: exec(w, w.book.phi_readable()); return;       // phi restored where it lies: no flagged field is written
    }
}

// after every event: what the book trusts is true
void check(const World &w) {
    if (!w.book.zero_flags_trusted()) return;
    for (int c = 0; c < kCols; ++c)
        for (int l = 0; l < 2; ++l)
            need(!w.mem.flag[c][l] || w.mem.line_zero(c, l), "the book trusts a set flag over a line that does not hold zero bits");
}

void walk(const World &w, int depth) {
    for (int ev = 0; ev < N_EVENTS; ++ev) {
        World c = w;
        g_seq[g_len++] = ev;
        ++g_stats.sequences;
        play(c, ev);
        check(c);
        if (depth > 1) walk(c, depth - 1);
        --g_len;
    }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "walk")) {
        const int depth = std::atoi(argv[2]);
        if (depth < 1 || depth > 16) return 2;
        for (int elide = 1; elide >= 0; --elide) {
            g_stats = Stats{};
            World w(elide != 0);
            check(w);
            walk(w, depth);
            std::printf("elide %d sequences %lld clears %lld eliding %lld plain %lld skipped_stores %lld skipped_loads %lld\n", elide,
                        g_stats.sequences, g_stats.clears, g_stats.eliding, g_stats.plain, g_stats.skipped_stores, g_stats.skipped_loads);
        }
        return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "replay")) {
        World w(true);
        for (int i = 2; i < argc && g_len < 63; ++i) {
            int ev = 0;
            while (ev < N_EVENTS && std::strcmp(kEventName[ev], argv[i])) ++ev;
            if (ev == N_EVENTS) { std::fprintf(stderr, "unknown event %s\n", argv[i]); return 2; }
            g_seq[g_len++] = ev;
            g_cleared = false;
            play(w, ev);
            check(w);
            std::printf("%s:%s %s\n", argv[i], g_cleared ? " clear" : "", w.book.zero_flags_trusted() ? "trusted" : "untrusted");
        }
        return 0;
    }
    std::fprintf(stderr, "usage: %s walk DEPTH | replay EVENT...\n", argv[0]);
    return 2;
}
