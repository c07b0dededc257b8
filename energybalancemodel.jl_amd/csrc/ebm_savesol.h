// The savesol! schedule: THE rule for what every step of an ebm_integrate owes its outputs, which stretches of steps owe
// nothing and may be fused, and where the raw snapshots lie in the two-half staging buffer.  Plain C++17, no HIP include: the
// rule is walked exhaustively by a stand-alone host program (tests/host_savesol_main.cpp); integrate_impl (ebm_drive.hip)
// only consumes what this header returns.
//
// The reference (src/infrastructure.jl:549-591), for the 1-based step tinx of nt * dur, ti = mod1(tinx, nt) its index in
// the year and year = ceil(T[tinx]) = (tinx - 1) / nt + 1:
//   :561-571  the raw snapshot is kept at tinx, or — lastonly — at ti and only if tinx > nt * dur - nt (the last year);
//   :573-589  ONE chain: ti == winter.inx -> the winter snapshot of `year`; else ti == summer.inx -> the summer snapshot;
//             else ti == nt -> the annual mean of `year`.  So winter wins where the two indices coincide, and a year whose
//             last step is a seasonal index has no mean: its sums are dropped and the next year starts from zero.
// The indices are not checked: one outside 1 .. nt never matches, and that season is never taken.
// What the runtime adds: an output that nobody wants is not taken.  A step stores the diagnostic fields, and leaves every
// field in the natural layout, only if it falls on the index of a WANTED season (either one: with coinciding indices a
// wanted summer makes it such a step although winter takes the output) or is the run's last.  A step is PLAIN if it keeps no
// raw snapshot, falls on no wanted season's index and is not a year's last step (the run's last step is one); a stretch of
// at least two plain steps is one fused item, as long as possible, which needs nothing but the running sums.
#pragma once
#include <algorithm>
#include <cstddef>

namespace ebm {

struct SaveConfig {
    int nt, dur;                     // steps per year, years
    bool lastonly;
    int winter_inx, summer_inx;      // 1-based, unchecked
    bool keep_raw;                   // the raw snapshots are wanted
    bool want_winter, want_summer;   // the seasonal snapshot or its hemispheric means
    bool want_sums;                  // the annual means or their hemispheric means: the running sums
    bool may_fuse;                   // the handle has the kernels for fused stretches and is asked to use them
    long long total() const { return (long long)nt * dur; }
    long long nraw() const { return lastonly ? nt : total(); }         // raw snapshots per variable in the caller's array
    // row of a [nvars][dur] output: variable v, 1-based year
    size_t row(int v, long long year) const { return (size_t)v * (size_t)dur + (size_t)(year - 1); }
};

enum Season { SEASON_NONE = 0, SEASON_WINTER, SEASON_SUMMER };

// What step tinx owes.
struct SaveStep {
    int tab, tab_next;        // 0-based entries of the time table: the step's own and its successor's
    long long year;           // 1-based
    long long raw_index;      // where its raw snapshot goes in the caller's array; -1: it is not kept
    Season season;            // the seasonal output taken from it (if wanted)
    bool snapshot;            // it stores the diagnostic fields and every field is made natural after it
    bool last;                // the run's last step: it stores the diagnostic fields too
    bool mean;                // after it, the annual mean of `year` is formed from the sums (which restarts them)
    bool restart;             // after it, the sums are dropped: the year ended on a seasonal index
    bool diag() const { return snapshot || last; }
};
inline SaveStep save_step(const SaveConfig &c, long long tinx) {
    const long long ti = (tinx - 1) % c.nt + 1;
    SaveStep s{};
    s.tab = (int)(ti - 1);
    s.tab_next = (int)(ti % c.nt);
    s.year = (tinx - 1) / c.nt + 1;
    s.raw_index = !c.keep_raw ? -1 : !c.lastonly ? tinx - 1 : tinx > c.total() - c.nt ? ti - 1 : -1;
    s.snapshot = (ti == c.winter_inx && c.want_winter) || (ti == c.summer_inx && c.want_summer);
    s.last = tinx >= c.total();
    if (ti == c.winter_inx) s.season = SEASON_WINTER;
    else if (ti == c.summer_inx) s.season = SEASON_SUMMER;
    else if (ti == c.nt) s.mean = c.want_sums;
    s.restart = c.want_sums && ti == c.nt && s.season != SEASON_NONE;
    return s;
}

// The first step at or after tinx (<= nt * dur) that is not plain, computed and not searched for — tinx itself if its raw
// snapshot is kept (under lastonly the kept steps begin with a year, so a year's last step comes before the first of them),
// else the earliest of: this year's last step, a wanted season's index in what is left of this year.
inline long long next_event(const SaveConfig &c, long long tinx) {
    if (save_step(c, tinx).raw_index >= 0) return tinx;
    const long long before = (tinx - 1) / c.nt * c.nt;              // steps before this year
    long long e = before + c.nt;
    const auto season = [&](bool wanted, int inx) {
        if (wanted && inx >= 1 && inx <= c.nt && before + inx >= tinx) e = std::min(e, before + inx);
    };
    season(c.want_winter, c.winter_inx);
    season(c.want_summer, c.summer_inx);
    return e;
}

// One item of the walk: n >= 2 plain steps to be fused, or (n == 1) the single step `step`.
struct SaveItem {
    long long first;          // 0-based step of the run that the item begins with
    long long n;
    bool sums;                // its launches add to the running sums
    SaveStep step;            // n == 1 only
};
constexpr long long kMaxStretch = 1 << 30;     // a fused stretch's length is an int of the runtime

// The steps 1 .. nt * dur as items, in order, each step once: for (SaveItem it; walk.next(it);)
class SaveWalk {
public:
    explicit SaveWalk(const SaveConfig &cfg) : c(cfg) {}
    bool next(SaveItem &it) {
        if (tinx > c.total()) return false;
        const long long plain = c.may_fuse ? std::min(next_event(c, tinx) - tinx, kMaxStretch) : 0;
        it.first = tinx - 1;
        it.n = plain >= 2 ? plain : 1;
        it.sums = c.want_sums;
        it.step = save_step(c, tinx);
        tinx += it.n;
        return true;
    }

private:
    SaveConfig c;
    long long tinx = 1;
};

// The raw snapshots on the device: two halves of [nvars][chunk] snapshots of npitch elements; the steps fill one half while
// the other leaves for the host.  Counts in snapshots; the *_elems answers in elements of the buffer.
struct RawSlot {
    int half;
    long long offset;         // snapshot of the half, per variable
};
struct RawFlush {
    int half;
    long long count, raw_base;    // `count` snapshots per variable, the first of them raw index raw_base of the caller's array
};
class RawStaging {
public:
    RawStaging() = default;         // nothing is kept
    // chunk: what fits budget_bytes in one half, at least one snapshot, at most all of them
    RawStaging(size_t budget_bytes, size_t npitch, int nvars, long long nraw) : npitch_(npitch), nvars_((size_t)nvars), nraw_(nraw) {
        chunk_ = (long long)(budget_bytes / (sizeof(double) * npitch_ * nvars_));
        if (chunk_ < 1) chunk_ = 1;
        if (chunk_ > nraw_) chunk_ = nraw_;
    }
    long long chunk() const { return chunk_; }
    size_t total_elems() const { return 2 * half_elems(); }
    size_t half_base_elems(int half) const { return (size_t)half * half_elems(); }
    size_t var_stride_elems() const { return (size_t)chunk_ * npitch_; }                      // between variables of a half
    size_t slot_elems(const RawSlot &s) const { return (size_t)s.offset * npitch_; }         // within a variable of a half
    // first snapshot of variable v of a flush, counted in snapshots of the caller's [nvars][nraw] array
    size_t dst_snapshot(const RawFlush &f, int v) const { return (size_t)v * (size_t)nraw_ + (size_t)f.raw_base; }
    // where the next kept step is written
    RawSlot slot() const { return {half_, staged_}; }
    // a kept step has been written to slot(): true if its half is full and leaves now, as `f`
    bool kept(RawFlush &f) { return ++staged_ == chunk_ && flush(f); }
    // the run has ended: true if something is still staged and leaves now, as `f`
    bool flush(RawFlush &f) {
        if (!staged_) return false;
        f = RawFlush{half_, staged_, raw_base_};
        raw_base_ += staged_;
        staged_ = 0;
        half_ ^= 1;
        return true;
    }

private:
    size_t half_elems() const { return nvars_ * (size_t)chunk_ * npitch_; }
    size_t npitch_ = 0, nvars_ = 0;
    long long nraw_ = 0, chunk_ = 0, staged_ = 0, raw_base_ = 0;
    int half_ = 0;
};

}  // namespace ebm
