// Stand-alone play of csrc/ebm_solve.h on the host for tests/test_host_solve.py: no HIP, no GPU.  The header's three functions
// (partition_solve_r, halo_exchange, halo_exchange_waves) are straight-line SPMD code with uniform barriers; here a workgroup is T
// fibers (glibc ucontext), one per thread, and a scheduler that owns every barrier: it runs ONE barrier interval at a time, the
// threads one after the other in an order it chooses, and keeps a copy of the LDS image at every barrier.  A race between threads
// that leave the same barrier then shows as a result, or an LDS image, that depends on the order.
//   solve    [options]          partition_solve_r<C, R, COMPACT> over every geometry, system and schedule; per case the error
//                               against a long double Thomas solve beside fp64 Thomas's own, per family the largest ratio
//   contract MODE [options]     two systems through two solves back to back in every thread.  MODE: sync (one barrier between
//                               them), nosync (none), reuse-sync / reuse-nosync (the caller overwrites the buffer that the header
//                               says may still be read on exit, after a barrier / at once)
//   halo     MODE [options]     halo_exchange and halo_exchange_waves twice in a row against the directly indexed neighbours.
//                               MODE: sync (the callers' barrier between the calls), nosync (none)
//   options: --seeds N (random schedules, default 8)  --shard I N (every N-th case from the I-th)
//            --sizes default|full|small (default: every T for R = 4, seven for R = 2 and 8; small: T = 64, 192, 1024)
// Exit status 1 if anything was reported, with a line "REPORT ..." that names the case, the two schedules, the first barrier
// at which the LDS images differ and the first differing word's buffer and offset.  A thread-serial order is stricter than the
// hardware's lock-step waves; the header passes it, so it is held to it.
//
// What is NOT played: the kernels that call these functions (their own reuse of P0/P1 between the solve and what follows), a
// race that writes the value already there, and the hardware's memory model.
#include <ucontext.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#define PLAY_ASAN 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define PLAY_ASAN 1
#endif
#endif
#ifdef PLAY_ASAN
#include <sanitizer/asan_interface.h>
#include <sanitizer/common_interface_defs.h>
#endif

// ---- the workgroup ------------------------------------------------------------------------------------------------------------
namespace play {

constexpr int kMaxT = 1024, kWave = 64;
// (under AddressSanitizer every switch clears the shadow of the whole stack it switches to: small stacks keep that leg quick;
// the solve's frames take a few KiB, and the canary at the low end of every stack is checked after every run)
#ifdef PLAY_ASAN
constexpr size_t kStack = 32 * 1024;
#else
constexpr size_t kStack = 64 * 1024;
#endif
constexpr uint64_t kCanary = 0x5AFE57AC5AFE57ACull;
enum State : unsigned char { RUNNING, AT_BARRIER, AT_WAVE, DONE };

struct Schedule {
    enum Kind { ASC, DESC, WAVES_REV, LANES_REV, FIRST, LAST, RANDOM } kind;
    int which;   // FIRST, LAST: the straggler, an index into {0, pivot - 1, pivot, T - 1}; RANDOM: the seed
    int straggler(int T, int pivot) const {
        const int s[4] = {0, pivot - 1, pivot, T - 1};
        return s[which];
    }
    std::string name(int T, int pivot) const {
        switch (kind) {
            case ASC: return "ascending";
            case DESC: return "descending";
            case WAVES_REV: return "waves-descending-lanes-ascending";
            case LANES_REV: return "waves-ascending-lanes-descending";
            case FIRST: return "thread-" + std::to_string(straggler(T, pivot)) + "-first";
            case LAST: return "thread-" + std::to_string(straggler(T, pivot)) + "-last";
            default: return "random-" + std::to_string(which);
        }
    }
    // the order in which the threads run barrier interval `interval`
    void fill(int interval, int T, int pivot, std::vector<int> &o) const {
        o.resize(T);
        for (int i = 0; i < T; ++i) o[i] = i;
        switch (kind) {
            case ASC: return;
            case DESC: std::reverse(o.begin(), o.end()); return;
            case WAVES_REV:
                for (int i = 0; i < T; ++i) o[i] = (T / kWave - 1 - i / kWave) * kWave + i % kWave;
                return;
            case LANES_REV:
                for (int i = 0; i < T; ++i) o[i] = (i / kWave) * kWave + (kWave - 1 - i % kWave);
                return;
            case FIRST: case LAST: {
                const int s = straggler(T, pivot);
                o.erase(o.begin() + s);
                o.insert(kind == FIRST ? o.begin() : o.end(), s);
                return;
            }
            case RANDOM: {
                uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)(which + 1) + 0xD1B54A32D192ED03ull * (uint64_t)(interval + 1);
                for (int i = T - 1; i > 0; --i) {      // Fisher-Yates on splitmix64
                    z += 0x9E3779B97F4A7C15ull;
                    uint64_t r = z;
                    r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
                    r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
                    r ^= r >> 31;
                    std::swap(o[i], o[(int)(r % (uint64_t)(i + 1))]);
                }
                return;
            }
        }
    }
};

struct Group {
    int T = 0, cur = -1, prev = -1;
    void (*body)(int) = nullptr;
    ucontext_t main_ctx, ctx[kMaxT];
    char *stacks = nullptr;
    std::vector<int> order, queue;    // the interval's order; what is still to run in it (a released wave is put in again)
    size_t pos = 0;
    State st[kMaxT];
    int n_barrier = 0, n_done = 0;
    int wave_arrived[kMaxT / kWave];
    int lane_word[kMaxT], lane_index[kMaxT], lane_result[kMaxT];
    const void *main_bottom = nullptr;
    size_t main_size = 0;
} g;

void transfer(int from, int to, bool dying = false) {
    ucontext_t *src = from < 0 ? &g.main_ctx : &g.ctx[from], *dst = to < 0 ? &g.main_ctx : &g.ctx[to];
    g.prev = from;
    g.cur = to;
#ifdef PLAY_ASAN
    void *fake = nullptr;
    __sanitizer_start_switch_fiber(dying ? nullptr : &fake, to < 0 ? g.main_bottom : g.stacks + (size_t)to * kStack,
                                   to < 0 ? g.main_size : kStack);
#else
    (void)dying;
#endif
    swapcontext(src, dst);
#ifdef PLAY_ASAN
    __sanitizer_finish_switch_fiber(fake, nullptr, nullptr);
#endif
}

// the running thread has stopped (barrier, wave exchange, return): on to the next of the interval, or back to the scheduler
void pass_on(int me, bool dying) {
    ++g.pos;
    const int to = g.pos < g.queue.size() ? g.queue[g.pos] : -1;
    if (to == me) return;             // (the first lane of a wave that this thread has just released)
    transfer(me, to, dying);
}

void entry() {
#ifdef PLAY_ASAN
    const void *bottom;
    size_t size;
    __sanitizer_finish_switch_fiber(nullptr, &bottom, &size);
    if (g.prev < 0) g.main_bottom = bottom, g.main_size = size;
#endif
    const int me = g.cur;
    g.body(me);
    g.st[me] = DONE;
    ++g.n_done;
    pass_on(me, true);
    std::abort();                     // a thread that returned is never resumed
}

void barrier() {
    const int me = g.cur;
    g.st[me] = AT_BARRIER;
    ++g.n_barrier;
    pass_on(me, false);
}

// ds_bpermute_b32: every lane publishes its word; once the whole wave has, lane i holds the word of lane (index_i / 4) % 64.
// The wave is released when its last lane arrives and runs on at once, in the interval's order, before any other thread.
int bpermute(int byte_index, int word) {
    const int me = g.cur, w = me / kWave;
    g.lane_word[me] = word;
    g.lane_index[me] = (byte_index >> 2) & (kWave - 1);
    g.st[me] = AT_WAVE;
    if (++g.wave_arrived[w] == kWave) {
        g.wave_arrived[w] = 0;
        std::vector<int> lanes;
        for (int t : g.order)
            if (t / kWave == w) lanes.push_back(t);
        for (int t : lanes) {
            g.lane_result[t] = g.lane_word[w * kWave + g.lane_index[t]];
            g.st[t] = RUNNING;
        }
        g.queue.insert(g.queue.begin() + g.pos + 1, lanes.begin(), lanes.end());
    }
    pass_on(me, false);
    return g.lane_result[me];
}

// One workgroup run: T threads through `body` under schedule s.  at_barrier(k) is called when all T threads wait at their
// k-th barrier.  Returns "" or what went wrong with the barriers themselves.
std::string run(int T, void (*body)(int), const Schedule &s, int pivot, const std::function<void(int)> &at_barrier) {
    if (!g.stacks) g.stacks = (char *)std::aligned_alloc(4096, (size_t)kMaxT * kStack);
    g.T = T;
    g.body = body;
    g.n_done = 0;
    std::memset(g.wave_arrived, 0, sizeof(g.wave_arrived));
    for (int t = 0; t < T; ++t) {
#ifdef PLAY_ASAN
        __asan_unpoison_memory_region(g.stacks + (size_t)t * kStack, kStack);     // (frames of a thread that never returned)
#endif
        for (int i = 0; i < 8; ++i) std::memcpy(g.stacks + (size_t)t * kStack + 8 * i, &kCanary, 8);
        getcontext(&g.ctx[t]);
        g.ctx[t].uc_stack.ss_sp = g.stacks + (size_t)t * kStack;
        g.ctx[t].uc_stack.ss_size = kStack;
        g.ctx[t].uc_link = nullptr;
        makecontext(&g.ctx[t], entry, 0);
        g.st[t] = RUNNING;
    }
    auto stacks_held = [T] {
        for (int t = 0; t < T; ++t)
            for (int i = 0; i < 8; ++i)
                if (std::memcmp(g.stacks + (size_t)t * kStack + 8 * i, &kCanary, 8)) return false;
        return true;
    };
    for (int interval = 0;; ++interval) {
        s.fill(interval, T, pivot, g.order);
        g.queue = g.order;
        g.pos = 0;
        g.n_barrier = 0;
        transfer(-1, g.queue[0]);
        for (int t = 0; t < T; ++t)
            if (g.st[t] == AT_WAVE)
                return "thread " + std::to_string(t) + " waits in a wave exchange that its wave never completed (interval " +
                       std::to_string(interval) + ")";
        if (!stacks_held()) {
            std::fprintf(stderr, "a thread's stack of %zu bytes overflowed\n", kStack);
            std::abort();
        }
        if (g.n_done == T) return "";
        if (g.n_barrier != T) {
            int done = 0, waits = 0;
            for (int t = 0; t < T; ++t) (g.st[t] == DONE ? done : waits) = t;
            return "thread " + std::to_string(done) + " returned while thread " + std::to_string(waits) + " waits at barrier " +
                   std::to_string(interval);
        }
        at_barrier(interval);
        for (int t = 0; t < T; ++t) g.st[t] = RUNNING;
    }
}

}  // namespace play

// ---- the header under test, with stand-ins for the little of HIP it uses --------------------------------------------------------
#define EBM_SOLVE_ON_HOST
#define __device__
#define __forceinline__ inline
#define __builtin_amdgcn_ds_bpermute play::bpermute
inline void __syncthreads() { play::barrier(); }
inline int __double2loint(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (int)(uint32_t)u;
}
inline int __double2hiint(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (int)(uint32_t)(u >> 32);
}
inline double __hiloint2double(int hi, int lo) {
    const uint64_t u = ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}
namespace ebm {
inline double fast_rcp(double x) { return 1.0 / x; }      // correctly rounded: the header calls the solve's arithmetic free
}  // namespace ebm

#include "../energybalancemodel.jl_amd/csrc/ebm_solve.h"

namespace {

using play::Schedule;

// ---- LDS ----------------------------------------------------------------------------------------------------------------------
constexpr size_t kGuard = 1024;     // (wide enough to hold a buffer overrun by a third at T = 1024: reported, not a crash)
constexpr uint64_t kGuardBits = 0x7FF8000A5A5A5A5Aull, kPoisonBits = 0x7FF80000C3C3C3C3ull;     // two NaN payloads
double from_bits(uint64_t u) {
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}
uint64_t to_bits(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
}

// One LDS buffer: an allocation of its own, n doubles between two guard bands
struct Buffer {
    std::vector<double> store;
    size_t n = 0;
    void reset(size_t words) {
        n = words;
        store.assign(n + 2 * kGuard, from_bits(kPoisonBits));
        for (size_t i = 0; i < kGuard; ++i) store[i] = store[kGuard + n + i] = from_bits(kGuardBits);
    }
    double *p() { return store.data() + kGuard; }
    bool guards_intact() const {
        for (size_t i = 0; i < kGuard; ++i)
            if (to_bits(store[i]) != kGuardBits || to_bits(store[kGuard + n + i]) != kGuardBits) return false;
        return true;
    }
};

struct Result {
    std::string error;
    std::vector<uint64_t> out;
    std::vector<std::vector<uint64_t>> images;     // at every barrier: P0's words, then P1's
    bool guards = true;
};

struct Totals {
    long long cases = 0, runs = 0, barriers = 0, reported = 0;
} g_totals;
int g_seeds = 8, g_shard = 0, g_shards = 1;
long long g_case_index = 0;

std::vector<Schedule> schedules() {
    std::vector<Schedule> s = {{Schedule::ASC, 0}, {Schedule::DESC, 0}, {Schedule::WAVES_REV, 0}, {Schedule::LANES_REV, 0}};
    for (int i = 0; i < 4; ++i) s.push_back({Schedule::FIRST, i}), s.push_back({Schedule::LAST, i});
    for (int i = 0; i < g_seeds; ++i) s.push_back({Schedule::RANDOM, i});
    return s;
}

bool my_case() { return g_case_index++ % g_shards == g_shard; }

// One case: the body under every schedule, each run from poisoned LDS and poisoned outputs.  Verdicts (a) the outputs, (b) the
// LDS image at every barrier — whole images: the header passes that — bit-identical under every schedule, (c) no NaN in the
// outputs, (d) the guard bands intact.  Prints the first thing wrong, if `quiet` is not set; returns whether anything was.
bool play_case(const std::string &name, int T, int pivot, void (*body)(int), Buffer &B0, size_t n0, Buffer &B1, size_t n1,
               std::vector<double> &out, const std::function<void()> &bind, bool quiet, std::vector<double> *first_out = nullptr) {
    const std::vector<Schedule> all = schedules();
    Result ref;
    bool bad = false;
    ++g_totals.cases;
    for (size_t k = 0; k < all.size() && !bad; ++k) {
        Result r;
        B0.reset(n0);
        B1.reset(n1);
        std::fill(out.begin(), out.end(), from_bits(kPoisonBits));
        bind();
        r.error = play::run(T, body, all[k], pivot, [&](int) {
            std::vector<uint64_t> img(n0 + n1);
            std::memcpy(img.data(), B0.p(), n0 * 8);
            std::memcpy(img.data() + n0, B1.p(), n1 * 8);
            r.images.push_back(std::move(img));
        });
        r.guards = B0.guards_intact() && B1.guards_intact();
        r.out.resize(out.size());
        std::memcpy(r.out.data(), out.data(), out.size() * 8);
        ++g_totals.runs;
        g_totals.barriers += (long long)r.images.size();
        const std::string me = all[k].name(T, pivot), first = all[0].name(T, pivot);
        auto report = [&](const std::string &what) {
            bad = true;
            if (!quiet) std::printf("REPORT %s: schedule %s against %s: %s\n", name.c_str(), me.c_str(), first.c_str(), what.c_str());
        };
        if (!r.error.empty()) { report(r.error); break; }
        if (!r.guards) { report("a guard band of P0 or P1 was written"); break; }
        for (size_t i = 0; i < r.out.size(); ++i)
            if (std::isnan(from_bits(r.out[i]))) { report("output " + std::to_string(i) + " is NaN: a word nobody wrote took part in it"); break; }
        if (bad) break;
        if (k == 0) {
            if (first_out) *first_out = out;
            ref = std::move(r);
            continue;
        }
        if (r.images.size() != ref.images.size()) { report("another number of barriers"); break; }
        for (size_t b = 0; b < r.images.size() && !bad; ++b)
            for (size_t i = 0; i < n0 + n1; ++i)
                if (r.images[b][i] != ref.images[b][i]) {
                    report("the LDS images differ first at barrier " + std::to_string(b) + ", word " +
                           std::to_string(i < n0 ? i : i - n0) + " of " + (i < n0 ? "P0" : "P1"));
                    break;
                }
        if (bad) break;
        for (size_t i = 0; i < r.out.size(); ++i)
            if (r.out[i] != ref.out[i]) { report("output " + std::to_string(i) + " differs"); break; }
    }
    g_totals.reported += bad;
    return bad;
}

// ---- systems ------------------------------------------------------------------------------------------------------------------
struct Rng {
    uint64_t z;
    uint64_t next() {
        z += 0x9E3779B97F4A7C15ull;
        uint64_t r = z;
        r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
        r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
        return r ^ (r >> 31);
    }
    double uniform(double lo, double hi) { return lo + (hi - lo) * ((double)(next() >> 11) * 0x1p-53); }
    double sign() { return (next() & 1) ? 1.0 : -1.0; }
};

struct System {
    std::vector<double> a, b, c, d;
};
enum Family { RANDOM_DOMINANT, T0_SHAPE, DECOUPLED, IMEX_CONSTANT, N_FAMILIES };
const char *const kFamilyName[N_FAMILIES] = {"random", "t0", "decoupled", "imex"};

// N rows of which the first n are the system and the rest the identity padding the kernels feed (b = 1, a = c = d = 0).
// a[0] is zero, as the solve needs it (its interface rows carry a[0] on); c[n - 1] is left as drawn in the random family:
// the solve must ignore it, as Thomas elimination does (the next chunk's summary is taken as zero past the meridian).
System make_system(int family, int N, int n, uint64_t seed, int CR) {
    Rng rng{seed * 0x2545F4914F6CDD1Dull + (uint64_t)family};
    System s;
    s.a.assign(N, 0.0);
    s.b.assign(N, 1.0);
    s.c.assign(N, 0.0);
    s.d.assign(N, 0.0);
    if (family == RANDOM_DOMINANT) {
        for (int k = 0; k < n; ++k) {
            s.a[k] = k ? rng.uniform(-1.0, 1.0) : 0.0;
            s.c[k] = rng.uniform(-1.0, 1.0);
            s.b[k] = rng.sign() * (std::fabs(s.a[k]) + std::fabs(s.c[k]) + rng.uniform(0.05, 2.0));
            s.d[k] = rng.uniform(-1.0, 1.0);
        }
    } else if (family == T0_SHAPE) {
        // conductances of the cell edges up to 0.7e7, so that lo + up reaches 1.4e7; rows switched off in runs of random
        // length up to 3 C R, so that exactly decoupled runs cross chunk and second-level group boundaries
        const double scale = 0.7e7 * std::pow(10.0, -rng.uniform(0.0, 4.0));
        std::vector<double> e(n + 1);
        for (int k = 0; k <= n; ++k) e[k] = (k == 0 || k == n) ? 0.0 : scale * rng.uniform(0.2, 1.0);
        bool on = rng.next() & 1;
        int left = 1 + (int)(rng.next() % (uint64_t)(3 * CR));
        for (int k = 0; k < n; ++k) {
            const double kappa = rng.uniform(1.0, 20.0);
            if (on) {
                s.a[k] = -e[k];
                s.c[k] = -e[k + 1];
                s.b[k] = e[k] + e[k + 1] + kappa;
            } else {
                s.b[k] = kappa;
            }
            s.d[k] = rng.uniform(-300.0, 300.0);
            if (--left == 0) {
                on = !on;
                left = 1 + (int)(rng.next() % (uint64_t)(3 * CR));
            }
        }
    } else if (family == DECOUPLED) {
        for (int k = 0; k < n; ++k) {
            s.b[k] = rng.sign() * rng.uniform(0.5, 50.0);
            s.d[k] = rng.uniform(-100.0, 100.0);
        }
    } else {
        // I - theta Dif on n cells equally spaced in x = sin(latitude): edge k at x = -1 + k dx carries D (1 - x^2) / dx^2
        const double D = 0.6, theta = (1.0 / 2000.0) / 9.8, dx = 2.0 / n;
        for (int k = 0; k < n; ++k) {
            const double xl = -1.0 + k * dx, xr = -1.0 + (k + 1) * dx;
            const double lo = k ? D * (1.0 - xl * xl) / (dx * dx) : 0.0, up = k + 1 < n ? D * (1.0 - xr * xr) / (dx * dx) : 0.0;
            s.a[k] = -theta * lo;
            s.c[k] = -theta * up;
            s.b[k] = 1.0 + theta * (lo + up);
            s.d[k] = 15.0 - 40.0 * (xl + 0.5 * dx) * (xl + 0.5 * dx) + rng.uniform(-2.0, 2.0);
        }
    }
    return s;
}

template <typename F>
std::vector<F> thomas(const System &s) {
    const int N = (int)s.b.size();
    std::vector<F> cp(N), dp(N), x(N);
    cp[0] = (F)s.c[0] / (F)s.b[0];
    dp[0] = (F)s.d[0] / (F)s.b[0];
    for (int k = 1; k < N; ++k) {
        const F m = (F)s.b[k] - (F)s.a[k] * cp[k - 1];
        cp[k] = (F)s.c[k] / m;
        dp[k] = ((F)s.d[k] - (F)s.a[k] * dp[k - 1]) / m;
    }
    x[N - 1] = dp[N - 1];
    for (int k = N - 2; k >= 0; --k) x[k] = dp[k] - cp[k] * x[k + 1];
    return x;
}

// the largest error of x against the long double solve, in units of eps max|x|
template <typename F>
double error_units(const std::vector<F> &x, const std::vector<long double> &ref) {
    long double top = 0, err = 0;
    for (size_t k = 0; k < ref.size(); ++k) {
        top = std::max(top, std::fabs(ref[k]));
        err = std::max(err, std::fabs((long double)x[k] - ref[k]));
    }
    return (double)(err / (2.220446049250313e-16L * top));
}

// ---- partition_solve_r --------------------------------------------------------------------------------------------------------
enum Mode { SINGLE, TWO_SYNC, TWO_NOSYNC, REUSE_SYNC, REUSE_NOSYNC };
struct Job {
    int T = 0, mode = SINGLE;
    double *P0 = nullptr, *P1 = nullptr, *still_read = nullptr, *x = nullptr;
    const System *sys[2] = {nullptr, nullptr};
} g_job;

template <int C, int R, bool COMPACT>
void solve_body(int t) {
    const Job &j = g_job;
    const int N = j.T * C, solves = j.mode == SINGLE ? 1 : 2;
    for (int rep = 0; rep < solves; ++rep) {
        if (rep) {
            if (j.mode == TWO_SYNC || j.mode == REUSE_SYNC) __syncthreads();
            // the caller takes the buffer for something of its own, as the kernels do for their halo exchanges
            if (j.mode == REUSE_SYNC || j.mode == REUSE_NOSYNC) j.still_read[t] = -0.5 - t;
        }
        const System &s = *j.sys[rep];
        double a[C], b[C], c[C], d[C], x[C];
        for (int i = 0; i < C; ++i) a[i] = s.a[t * C + i], b[i] = s.b[t * C + i], c[i] = s.c[t * C + i], d[i] = s.d[t * C + i];
        ebm::partition_solve_r<C, R, COMPACT>(a, b, c, d, x, t, j.T, j.P0, j.P1);
        for (int i = 0; i < C; ++i) j.x[rep * N + t * C + i] = x[i];
    }
}

struct Variant {
    int C, R;
    bool compact;
    void (*body)(int);
    std::string name() const {
        return "C" + std::to_string(C) + " R" + std::to_string(R) + (compact ? " compact" : " plain");
    }
};
const Variant kVariants[] = {
    {2, 2, false, solve_body<2, 2, false>}, {2, 4, false, solve_body<2, 4, false>}, {2, 4, true, solve_body<2, 4, true>},
    {2, 8, false, solve_body<2, 8, false>}, {2, 8, true, solve_body<2, 8, true>},   {4, 2, false, solve_body<4, 2, false>},
    {4, 4, false, solve_body<4, 4, false>}, {4, 4, true, solve_body<4, 4, true>},   {4, 8, false, solve_body<4, 8, false>},
    {4, 8, true, solve_body<4, 8, true>},
};

std::vector<int> sizes_for(const std::string &sizes, int R) {
    if (sizes == "small") return {64, 192, 1024};
    if (sizes == "full" || R == 4) {
        std::vector<int> all;
        for (int T = 64; T <= 1024; T += 64) all.push_back(T);
        return all;
    }
    return {64, 128, 192, 448, 576, 768, 1024};
}

int solve_sweep(const std::string &sizes) {
    double worst_ratio[N_FAMILIES] = {}, worst_solve[N_FAMILIES] = {}, worst_thomas[N_FAMILIES] = {};
    Buffer B0, B1;
    for (const Variant &v : kVariants)
        for (int T : sizes_for(sizes, v.R))
            for (int family = 0; family < N_FAMILIES; ++family)
                for (int ragged = 0; ragged < 2; ++ragged) {
                    if (!my_case()) continue;
                    const int N = T * v.C, CR = v.C * v.R;
                    const uint64_t seed = (uint64_t)(((T * 16 + v.C) * 16 + v.R) * 4 + v.compact * 2 + ragged);
                    Rng pad{seed ^ 0xABCDEFull};
                    const int n = ragged ? N - 1 - (int)(pad.next() % (uint64_t)(3 * CR)) : N;
                    const System s = make_system(family, N, n, seed, CR);
                    std::vector<double> x(N), got;
                    const std::string name = "solve " + v.name() + " T" + std::to_string(T) + " " + kFamilyName[family] +
                                             (ragged ? " ragged " : " full ") + std::to_string(n);
                    const bool bad = play_case(name, T, T / v.R, v.body, B0, 3 * (size_t)T, B1, (v.compact ? 1 : 3) * (size_t)T, x, [&] {
                        g_job = Job{T, SINGLE, B0.p(), B1.p(), nullptr, x.data(), {&s, nullptr}};
                    }, false, &got);
                    if (bad) continue;
                    const std::vector<long double> ref = thomas<long double>(s);
                    const double es = error_units(got, ref), et = error_units(thomas<double>(s), ref), ratio = es / std::max(et, 1.0);
                    std::printf("case %s: partition %.3f thomas %.3f ratio %.3f\n", name.c_str(), es, et, ratio);
                    worst_ratio[family] = std::max(worst_ratio[family], ratio);
                    worst_solve[family] = std::max(worst_solve[family], es);
                    worst_thomas[family] = std::max(worst_thomas[family], et);
                }
    for (int f = 0; f < N_FAMILIES; ++f)
        std::printf("family %s ratio %.4f partition %.4f thomas %.4f\n", kFamilyName[f], worst_ratio[f], worst_solve[f], worst_thomas[f]);
    return 0;
}

int contract_sweep(int mode) {
    Buffer B0, B1;
    for (const Variant &v : kVariants) {
        long long reported = 0, cases = 0;
        for (int T : {64, 192, 448, 1024}) {
            if (!my_case()) continue;
            const int N = T * v.C;
            const System s0 = make_system(RANDOM_DOMINANT, N, N, 7000 + T, v.C * v.R), s1 = make_system(T0_SHAPE, N, N - 3, 9000 + T, v.C * v.R);
            std::vector<double> x(2 * (size_t)N);
            // on exit the interface solution may still be read: from P0, compact from P1
            ++cases;
            reported += play_case("contract " + v.name() + " T" + std::to_string(T), T, T / v.R, v.body, B0, 3 * (size_t)T, B1,
                                  (v.compact ? 1 : 3) * (size_t)T, x, [&] {
                g_job = Job{T, mode, B0.p(), B1.p(), v.compact ? B1.p() : B0.p(), x.data(), {&s0, &s1}};
            }, false);
        }
        std::printf("reported %s: %lld of %lld\n", v.name().c_str(), reported, cases);
    }
    return 0;
}

// ---- the halo exchanges -------------------------------------------------------------------------------------------------------
struct HaloJob {
    int T = 0;
    bool waves = false, sync = true;
    double *E = nullptr, *out = nullptr;
} g_halo;
double halo_first(int t, int call) { return 1000.25 + t + 5000.0 * call; }
double halo_last(int t, int call) { return -2000.5 - t - 5000.0 * call; }

void halo_body(int t) {
    const HaloJob &j = g_halo;
    for (int call = 0; call < 2; ++call) {
        if (call && j.sync) __syncthreads();
        double l, r;
        if (j.waves) ebm::halo_exchange_waves(j.E, t, j.T, halo_first(t, call), halo_last(t, call), l, r);
        else ebm::halo_exchange(j.E, j.E + j.T, t, j.T, halo_first(t, call), halo_last(t, call), l, r);
        j.out[4 * t + 2 * call] = l;
        j.out[4 * t + 2 * call + 1] = r;
    }
}

int halo_sweep(bool sync) {
    Buffer B0, B1;
    for (int waves = 0; waves < 2; ++waves) {
        long long reported = 0, cases = 0;
        for (int T = 64; T <= 1024; T += 64) {
            if (!my_case()) continue;
            std::vector<double> out(4 * (size_t)T), got;
            const std::string name = std::string(waves ? "halo_exchange_waves" : "halo_exchange") + " T" + std::to_string(T);
            // halo_exchange: E0 and E1 of T doubles each, as its callers pass them (P0, P0 + T); halo_exchange_waves: 32 words
            ++cases;
            bool bad = play_case(name, T, T / 4, halo_body, B0, waves ? 32 : 2 * (size_t)T, B1, 0, out, [&] {
                g_halo = HaloJob{T, waves != 0, sync, B0.p(), out.data()};
            }, false, &got);
            for (int t = 0; t < T && !bad; ++t)
                for (int call = 0; call < 2 && !bad; ++call) {
                    const double l = t > 0 ? halo_last(t - 1, call) : 0.0, r = t + 1 < T ? halo_first(t + 1, call) : 0.0;
                    if (got[4 * t + 2 * call] != l || got[4 * t + 2 * call + 1] != r) {
                        std::printf("REPORT %s: thread %d, call %d: not its neighbours' values\n", name.c_str(), t, call);
                        bad = true;
                        ++g_totals.reported;
                    }
                }
            reported += bad;
        }
        std::printf("reported %s: %lld of %lld\n", waves ? "halo_exchange_waves" : "halo_exchange", reported, cases);
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    std::string command = argc > 1 ? argv[1] : "", mode, sizes = "default";
    int i = 2;
    if (i < argc && argv[i][0] != '-') mode = argv[i++];
    for (; i < argc; ++i) {
        const std::string o = argv[i];
        if (o == "--seeds" && i + 1 < argc) g_seeds = std::atoi(argv[++i]);
        else if (o == "--shard" && i + 2 < argc) g_shard = std::atoi(argv[i + 1]), g_shards = std::atoi(argv[i + 2]), i += 2;
        else if (o == "--sizes" && i + 1 < argc) sizes = argv[++i];
        else command = "";
    }
    const bool shard_ok = g_shards >= 1 && g_shard >= 0 && g_shard < g_shards && g_seeds >= 0 && g_seeds <= 1000;
    const bool sizes_ok = sizes == "default" || sizes == "full" || sizes == "small";
    int known = -1;
    if (command == "solve" && mode.empty()) known = solve_sweep(sizes);
    else if (command == "contract" && mode == "sync") known = contract_sweep(TWO_SYNC);
    else if (command == "contract" && mode == "nosync") known = contract_sweep(TWO_NOSYNC);
    else if (command == "contract" && mode == "reuse-sync") known = contract_sweep(REUSE_SYNC);
    else if (command == "contract" && mode == "reuse-nosync") known = contract_sweep(REUSE_NOSYNC);
    else if (command == "halo" && (mode == "sync" || mode == "nosync")) known = halo_sweep(mode == "sync");
    if (known < 0 || !shard_ok || !sizes_ok) {
        std::fprintf(stderr, "usage: %s solve | contract sync|nosync|reuse-sync|reuse-nosync | halo sync|nosync\n"
                             "       [--seeds N] [--shard I N] [--sizes default|full|small]\n", argv[0]);
        return 2;
    }
    std::printf("runs cases %lld schedules %zu runs %lld barriers %lld reported %lld\n", g_totals.cases, schedules().size(),
                g_totals.runs, g_totals.barriers, g_totals.reported);
    return g_totals.reported ? 1 : 0;
}
