// The field book: THE one owner of what every reader and writer of a field of the handle sees — which diagnostic fields are
// current, which layout device memory holds, and whether phi lies in memory or is formed from Ei and h.  Plain C++17, no HIP:
// the book launches nothing.  It answers queries, names the PASS a caller must run before it touches the fields (Pass), and
// is told what happened (done, steps, written_outside, field_set); the .hip files keep the execution (exec_pass,
// csrc/ebm_fields.hip).  A failed launch reports nothing, so the book stays as it was.  tests/host_fieldbook_main.cpp walks
// every short sequence of the library's calls over this header against an independent model of device memory, without a GPU.
//
// Validity.  `epoch` counts every change of the prognostic state (steps taken, prognostic fields overwritten), `state_step`
// is the global index of the last step taken (-1: none).  A diagnostic field — one that only some steps write, the fp64 T0
// included — is current iff written_epoch[f] == epoch; a prognostic field always is.
//
// Layout.  At four cells per thread the MIZ kernels have a second, pair-split layout (csrc/ebm_miz_step.h):
//   diag_split    a one-step launch stored the five diagnostic fields split; their first reader un-splits them (UNSPLIT_DIAG)
//   state_split   the five prognostic fields lie split BETWEEN one-step launches: such a launch asks state_layout(true),
//                 every other reader or writer of a prognostic field — field I/O and views, the fused and resident kernels,
//                 series, means, snapshots — state_layout(false).  A steady ebm_run / ebm_step loop converts nothing;
//                 conversions() counts the passes (ebm_state_conversions)
// Without a second layout (classic, two cells per thread: the pair is the chunk) both stay false and no pass is ever named.
//
// phi.  A state-only one-step launch of the reference's step does not store phi where the handle has the deriving kernel
// (derive_phi): after any step phi is concentration(Ei, h) of the stored fields, and the kernel forms it from them.
//   phi_stored       the phi field in memory is current.  Cleared by a deriving launch, so false only while state_split.
//                    Who reads phi where it lies asks phi_readable (RESTORE_PHI); the un-split pass forms it on the way
//                    (UNSPLIT_STATE_FORM_PHI).  With the bit set neither is named: a steady run restores nothing
//   phi_consistent   Ei, h and phi were last written by step kernels, so phi IS that function of Ei and h under the column's
//                    parameters.  Cleared by every other writer of one of them and by a change of the parameters
//                    (written_outside, after phi_readable); set again by the next step launch over all columns.  Only then
//                    does a launch derive; else it steps with the phi the caller left
//
// Zero-line flags.  Where the handle elides zero lines (elide_zero_lines: the deriving kernel's variant that neither loads
// nor stores state lines that hold only zero bits, csrc/ebm_miz_step.h ZERO_LINES) the device keeps one flag per (column,
// wave, pair, field of Ei, Ew, h, D): SET MEANS that this KiB of the pair-split field holds only zero bits in HBM.  A clear
// flag claims nothing, so cleared flags are always true, and only the eliding kernel ever sets one.
//   zero_flags_trusted   every set flag is true.  Cleared by whoever else may write a prognostic field or move it to the
//                        other layout: every other step kernel (steps), the split and un-split passes (done), every outside
//                        writer (state_written_outside: ebm_set_field goes through it, and through the un-split pass
//                        before).  Before the next eliding launch — a graph replay of such launches included — the
//                        runtime owes a clear of all flags (zero_flags_need_clear; it reports zero_flags_cleared), and
//                        that launch rebuilds the flags of the columns it steps from what it stores.
//                        Flags are per column: an eliding launch over some columns leaves the others' as they were, true
#pragma once
#include "../../include/ebm_hip.h"
#include "ebm_types.h"

namespace ebm_rt {

// Per public field id, in the order of enum ebm_field:        Ei  Ew  h  D  phi  T0  Tw  Ti  n  E  T  Tg
// slab slot of a field for this model (MIZ: the id itself, Ei .. T), -1 if the model does not have it
inline int slot_of(int model, int f) {
    static const signed char classic[EBM_F_COUNT] = {-1, -1, ebm::C_h, -1, -1, -1, -1, -1, -1, ebm::C_E, ebm::C_T, ebm::C_Tg};
    if (f < 0 || f >= EBM_F_COUNT) return -1;
    return model == EBM_MODEL_MIZ ? (f <= EBM_F_T ? f : -1) : classic[f];
}
// quantity index (ebm::MizQuantity / ClassicQuantity) of a field, -1 if the step kernels do not produce it (the hidden warm
// start T0 is not a solution variable)
inline int quantity_of(int model, int f) {
    static const signed char miz[EBM_F_COUNT] = {ebm::Q_Ei, ebm::Q_Ew, ebm::Q_h, ebm::Q_D, ebm::Q_phi, -1,
                                                 ebm::Q_Tw, ebm::Q_Ti, ebm::Q_n, ebm::Q_E, ebm::Q_T, -1};
    static const signed char classic[EBM_F_COUNT] = {-1, -1, ebm::QC_h, -1, -1, -1, -1, -1, -1, ebm::QC_E, ebm::QC_T, ebm::QC_Tg};
    if (f < 0 || f >= EBM_F_COUNT) return -1;
    return (model == EBM_MODEL_MIZ ? miz : classic)[f];
}
inline const char *field_name(int f) {
    static const char *names[EBM_F_COUNT] = {"Ei", "Ew", "h", "D", "phi", "T0", "Tw", "Ti", "n", "E", "T", "Tg"};
    return (f >= 0 && f < EBM_F_COUNT) ? names[f] : "?";
}

// an in-place pass over fields of the handle; who is told to run one launches it and reports FieldBook::done
enum class Pass {
    NONE,
    SPLIT_STATE,              // the five prognostic fields, natural -> pair-split
    UNSPLIT_STATE,            // ... and back
    UNSPLIT_STATE_FORM_PHI,   // ... and back, phi formed from Ei and h instead of moved
    RESTORE_PHI,              // phi formed from Ei and h where it lies (pair-split)
    UNSPLIT_DIAG,             // the five diagnostic fields, pair-split -> natural
};

class FieldBook {
public:
    FieldBook() : FieldBook(EBM_MODEL_CLASSIC, false, false) {}
    // two_layouts: MIZ at four cells per thread; derive_phi: the handle has the deriving kernel
    // elide_zero_lines: ... and steps with its zero-line variant (only where derive_phi)
    FieldBook(int model, bool two_layouts, bool derive_phi, bool elide_zero_lines = false)
        : model_(model), two_layouts_(two_layouts), derive_phi_(derive_phi), elide_zero_lines_(elide_zero_lines && derive_phi) {
        for (int f = 0; f < EBM_F_COUNT; ++f) written_epoch_[f] = written_step_[f] = -1;
        written_epoch_[EBM_F_T0] = 0;                     // the warm start begins at zero, like the reference's (src/miz.jl:47)
    }

    // the model's fields
    bool has(int f) const { return slot_of(model_, f) >= 0; }
    // fields that only diagnostic steps write (everything else is prognostic and always current)
    bool is_diagnostic(int f) const {
        if (model_ == EBM_MODEL_MIZ)
            return f == EBM_F_T0 || f == EBM_F_Tw || f == EBM_F_Ti || f == EBM_F_n || f == EBM_F_E || f == EBM_F_T;
        return f == EBM_F_T || f == EBM_F_h;
    }
    // the diagnostic fields that a 4-cells-per-thread MIZ step stores pair-split
    bool is_split_field(int f) const {
        return model_ == EBM_MODEL_MIZ && (f == EBM_F_Tw || f == EBM_F_Ti || f == EBM_F_n || f == EBM_F_E || f == EBM_F_T);
    }
    // the prognostic fields that a 4-cells-per-thread MIZ one-step launch keeps pair-split
    bool is_split_state_field(int f) const { return model_ == EBM_MODEL_MIZ && f >= EBM_F_Ei && f <= EBM_F_phi; }

    // validity
    bool is_current(int f) const { return !is_diagnostic(f) || written_epoch_[f] == epoch_; }
    unsigned current_mask() const {                       // bit f: the model has field f and it is current
        unsigned m = 0;
        for (int f = 0; f < EBM_F_COUNT; ++f)
            if (has(f) && is_current(f)) m |= 1u << f;
        return m;
    }
    long long state_step() const { return state_step_; }
    bool never_written(int f) const { return is_diagnostic(f) && written_epoch_[f] < 0; }
    // the step whose state field f holds (ebm_field_step, ebm_get_field_as_of); `never` if nobody has written it
    long long written_step(int f, long long never = -1) const {
        return !is_diagnostic(f) ? state_step_ : never_written(f) ? never : written_step_[f];
    }

    // layout: the row of field f lies pair-split now
    bool held_split(int f) const { return (is_split_state_field(f) && state_split_) || (is_split_field(f) && diag_split_); }
    bool state_split() const { return state_split_; }
    bool phi_stored() const { return phi_stored_; }
    long long conversions() const { return n_conversions_; }

    // decisions: the pass that must run before ...
    // ... the prognostic fields are touched by somebody who expects them split / natural
    Pass state_layout(bool split) const {
        if (!two_layouts_) split = false;
        if (state_split_ == split) return Pass::NONE;
        return split ? Pass::SPLIT_STATE : phi_stored_ ? Pass::UNSPLIT_STATE : Pass::UNSPLIT_STATE_FORM_PHI;
    }
    // ... the diagnostic fields are read
    Pass diag_layout_natural() const { return diag_split_ ? Pass::UNSPLIT_DIAG : Pass::NONE; }
    // ... phi is read where it lies, in whatever layout the state has
    Pass phi_readable() const { return phi_stored_ ? Pass::NONE : Pass::RESTORE_PHI; }
    // the pass has been enqueued
    void done(Pass p) {
        switch (p) {
            case Pass::NONE: return;
            case Pass::RESTORE_PHI: phi_stored_ = true; return;      // (phi has no flags)
            case Pass::UNSPLIT_DIAG: diag_split_ = false; return;
            default:
                zero_flags_disturbed();                   // the lines of Ei, Ew, h, D have moved
                phi_stored_ = true;
                state_split_ = p == Pass::SPLIT_STATE;
                n_conversions_ += 1;
        }
    }
    // A step launch of OutMode `mode` takes the deriving kernel.  capturing: into a graph, whose launches are replayed later
    // — the book stays, and ebm_run makes the state fit them before a replay (replay_needs_a_direct_step)
    bool step_derives_phi(int mode, bool capturing) const {
        return mode == ebm::OUT_STATE && derive_phi_ && (capturing || phi_consistent_);
    }
    // the captured launches derive phi where the handle can: a state somebody else wrote takes one step directly first, with
    // the phi that is stored, and is consistent from then on
    bool replay_needs_a_direct_step() const { return derive_phi_ && !phi_consistent_; }
    // ... and the variant of it that trusts and maintains the zero-line flags: wherever the handle elides, a deriving launch
    // does.  Before it is enqueued — or a graph of such launches replayed — untrusted flags are cleared
    bool step_elides_zero_lines(int mode, bool capturing) const { return elide_zero_lines_ && step_derives_phi(mode, capturing); }
    bool elides_zero_lines() const { return elide_zero_lines_; }
    bool zero_flags_trusted() const { return elide_zero_lines_ && zero_flags_trusted_; }
    bool zero_flags_need_clear() const { return elide_zero_lines_ && !zero_flags_trusted_; }
    void zero_flags_cleared() { zero_flags_trusted_ = true; }

    // events
    // Launches have been enqueued that take `nsteps` steps, the last of them global step `last_step`.  wrote_diag: the last
    // one stored the diagnostic fields, pair-split if `split`.  Every step kernel leaves Ei, h and the phi it stores — or,
    // phi_derived, would have stored — consistent; a launch over a list of active columns says nothing of the others.
    // zero_lines: the eliding variant, which keeps the flags of its columns true; every other kernel stores what it likes.
    void steps(long long nsteps, long long last_step, bool wrote_diag, bool split, bool phi_derived, bool all_columns,
               bool zero_lines = false) {
        if (!zero_lines) zero_flags_disturbed();
        phi_stored_ = !phi_derived;
        if (all_columns) phi_consistent_ = true;
        epoch_ += nsteps;
        state_step_ = last_step;
        if (!wrote_diag) return;
        for (int f = 0; f < EBM_F_COUNT; ++f)
            if (has(f) && is_diagnostic(f)) {
                written_epoch_[f] = epoch_;
                written_step_[f] = last_step;
            }
        if (two_layouts_) diag_split_ = split;
    }
    // Ei, h or phi are about to be written by somebody who is not a step kernel, or the parameters they are tied by change
    // (phi_readable first: phi is restored under the present ones)
    void written_outside() { phi_consistent_ = false; }
    // What the runtime reports for every outside writer (state_written_outside, csrc/ebm_fields.hip): any of the prognostic
    // fields may hold a caller's values from now on — phi is no longer the function of Ei and h, and no zero-line flag holds
    void state_written_outside() {
        written_outside();
        zero_flags_disturbed();
    }
    // the caller has set field f
    void field_set(int f) {
        if (is_diagnostic(f)) {                           // the caller's statement of what the field holds: current as of now
            written_epoch_[f] = epoch_;
            written_step_[f] = state_step_;
        } else {
            epoch_ += 1;                                  // the prognostic state changed: every diagnostic field is older than it now
        }
    }

private:
    // somebody who knows nothing of the flags — another step kernel, a layout pass, an outside writer — has written, or
    // moved, lines of Ei, Ew, h or D
    void zero_flags_disturbed() { zero_flags_trusted_ = false; }
    int model_;
    bool two_layouts_, derive_phi_, elide_zero_lines_;
    long long epoch_ = 0, state_step_ = -1;
    long long written_epoch_[EBM_F_COUNT], written_step_[EBM_F_COUNT];
    bool diag_split_ = false, state_split_ = false;
    bool phi_stored_ = true, phi_consistent_ = true;
    bool zero_flags_trusted_ = true;                      // (the words start cleared)
    long long n_conversions_ = 0;
};

}  // namespace ebm_rt
