// Stand-alone play of the first Newton pass of the one-step kernels (csrc/ebm_miz_step.h, the kernels of the batched head) on the
// host, for tests/test_host_step_lds.py: no HIP, no GPU.  What tests/host_solve_main.cpp leaves out — "the kernels that call
// these functions (their own reuse of P0/P1 between the solve and what follows)" — for the one place where the kernel strings
// the header's functions together without a barrier of its own between them:
//   1. halo_exchange_two: r's and the masked g's first and last values behind one barrier (three words in P0, one in P1[0, T));
//   2. the kernel's barrier, after which the thread's words in P0 are dead (poisoned here);
//   3. partition_solve (four rows per thread, four second-level rows), whose first write is W1[t] = P1[t];
//   4. publish_then_vote: Tbar's first and last values into P1[0, 2T), the vote as the barrier,
//   5. the neighbours' words read after it; P0 (the interface solution Y) is dead from here and poisoned;
//   6. where the vote said "again": a second pass with halo_exchange through P0[0, 2T), after whose barrier the published
//      words in P1 are dead (poisoned), and the same solve, publication and vote.
// The scheduler, the schedules (ascending, descending, waves and lanes reversed, stragglers first and last, seeded
// permutations), the poisoned LDS between guard bands and the verdicts (results and the LDS image at every barrier the same
// bits under every schedule, no NaN in a result) are host_solve_main.cpp's, compiled into this program as it stands with its
// main renamed.  The rows are the kernel's (newton_iteration's expressions) on made-up conductances; the pointwise physics is
// not played: r, h and Tw are data.  The stash (h, Tw: words that only their owner touches) is plain memory here.
//   play ORDER [--seeds N]      T = 64, 128, 192, 320, 1024, each with a mask that is the fixed point (one pass) and with one
//                               that is not (two passes).  ORDER: shipped, or one of the three orders that must be reported:
//                               no-second-barrier (step 2 left out: W1[t] races the neighbour's read of g's last value),
//                               read-before-vote (step 5 before the vote's barrier), tbar-in-p0 (step 4 into P0, over Y)
// Exit status 1 if anything was reported.
#define main host_solve_player_main
#include "host_solve_main.cpp"
#undef main

namespace {

constexpr int kC = 4, kMaxPass = 3, kWords = 4 + kMaxPass * (kC + 3) + 1;     // per thread: rl rr gl gr, per pass x[4] tbl tbr again, passes
enum Order { SHIPPED, NO_SECOND_BARRIER, READ_BEFORE_VOTE, TBAR_IN_P0 };

struct StepJob {
    int T = 0, n = 0, order = SHIPPED;
    double *P0 = nullptr, *P1 = nullptr, *out = nullptr;
    const double *lo = nullptr, *up = nullptr, *dd = nullptr, *ph = nullptr, *r = nullptr, *c0 = nullptr, *h = nullptr, *tw = nullptr;
    const unsigned *mask0 = nullptr;
    double Tm = -1.25;
} g_step;

int g_vote[kMaxPass], g_votes_taken[play::kMaxT];

void poison(double *p) { *p = from_bits(kPoisonBits); }

// Tbar of cell k from the solution, phase D's expressions in its order
double tbar_of(const StepJob &j, int k, double x) {
    const double T0 = x + j.Tm;
    const double ti = T0 < j.Tm ? T0 : j.Tm;
    const double Ti = (j.h[k] == 0.0) ? 0.0 : ti;
    return Ti * j.ph[k] + (1.0 - j.ph[k]) * j.tw[k];
}

void step_body(int t) {
    const StepJob &j = g_step;
    const int T = j.T, k0 = t * kC;
    double *P0 = j.P0, *P1 = j.P1, *out = j.out + (size_t)t * kWords;
    double lo[kC], up[kC], dd[kC], ph[kC], r[kC], rd[kC], xs[kC], g[kC], gl, gr;
    for (int i = 0; i < kC; ++i) lo[i] = j.lo[k0 + i], up[i] = j.up[k0 + i], dd[i] = j.dd[k0 + i], ph[i] = j.ph[k0 + i], r[i] = j.r[k0 + i];
    unsigned smask = j.mask0[t];
    int it = 0;
    bool again;
    do {
        for (int i = 0; i < kC; ++i) g[i] = ((smask >> i) & 1u) ? ph[i] : 0.0;
        if (it == 0) {
            double rl, rr;
            ebm::halo_exchange_two(P0, P1, t, T, r[0], r[kC - 1], g[0], g[kC - 1], rl, rr, gl, gr);
            out[0] = rl, out[1] = rr, out[2] = gl, out[3] = gr;
            for (int i = 0; i < kC; ++i) {
                const double rm = i > 0 ? r[i - 1] : rl, rp = i < kC - 1 ? r[i + 1] : rr;
                rd[i] = -(j.c0[k0 + i] + __builtin_fma(up[i], rp - r[i], lo[i] * (rm - r[i])));
            }
            if (j.order != NO_SECOND_BARRIER) {
                __syncthreads();
                poison(P0 + t), poison(P0 + T + t), poison(P0 + 2 * T + t);
            }
        } else {
            ebm::halo_exchange(P0, P0 + T, t, T, g[0], g[kC - 1], gl, gr);
            poison(P1 + t), poison(P1 + T + t);      // the words published under the vote that said "again"
        }
        double ra[kC], rb[kC], rc[kC];
        for (int i = 0; i < kC; ++i) {
            ra[i] = lo[i] * (i > 0 ? g[i - 1] : gl);
            rc[i] = up[i] * (i < kC - 1 ? g[i + 1] : gr);
            rb[i] = -__builtin_fma(lo[i] + up[i], g[i], dd[i]);
        }
        ebm::partition_solve<kC, 1024>(ra, rb, rc, rd, xs, t, T, P0, P1);
        unsigned snew = 0;
        for (int i = 0; i < kC; ++i) snew |= (xs[i] < 0.0) ? (1u << i) : 0u;
        const int nvalid = j.n - k0;
        snew &= nvalid >= kC ? ~0u : (nvalid > 0 ? (1u << nvalid) - 1u : 0u);
        const int changed = snew != smask;
        smask = snew;
        const double first = tbar_of(j, k0, xs[0]), last = tbar_of(j, k0 + kC - 1, xs[kC - 1]);
        double tbl, tbr;
        if (j.order == READ_BEFORE_VOTE) {
            P1[t] = first;
            P1[T + t] = last;
            const double l = P1[T + (t > 0 ? t - 1 : 0)], rr = P1[t + 1 < T ? t + 1 : t];
            tbl = t > 0 ? l : 0.0;
            tbr = t + 1 < T ? rr : 0.0;
            again = __syncthreads_or(changed) != 0;
        } else {
            again = ebm::publish_then_vote(j.order == TBAR_IN_P0 ? P0 : P1, t, T, first, last, changed, tbl, tbr);
        }
        if (j.order != TBAR_IN_P0) poison(P0 + t), poison(P0 + T + t), poison(P0 + 2 * T + t);      // Y is dead after the vote
        double *o = out + 4 + it * (kC + 3);
        for (int i = 0; i < kC; ++i) o[i] = xs[i];
        o[kC] = tbl, o[kC + 1] = tbr, o[kC + 2] = again ? 1.0 : 0.0;
        ++it;
    } while (again && it < kMaxPass);
    for (int p = it; p < kMaxPass; ++p)
        for (int i = 0; i < kC + 3; ++i) out[4 + p * (kC + 3) + i] = 0.0;
    out[kWords - 1] = it;
}

struct StepData {
    std::vector<double> lo, up, dd, ph, r, c0, h, tw;
    std::vector<unsigned> fixed, mask0;
};

// n live cells of 4 T: weak conductances against a diagonal excess of 1 .. 3 and |c0| of 1 .. 3, so that the solution's signs
// are those of c0 whatever the active set (the coupling moves x by less than 0.3, |x| > 1/3): the fixed point is known.  c0
// changes sign in runs that cross chunk boundaries.  Padding cells: decoupled rows with zero right-hand side, never active.
StepData make_step(int T, int n, uint64_t seed, bool at_fixed_point) {
    const int N = T * kC;
    Rng rng{seed};
    StepData s;
    s.lo.assign(N, 0.0), s.up.assign(N, 0.0), s.dd.assign(N, 1.0), s.ph.assign(N, 0.0), s.r.assign(N, 0.0), s.c0.assign(N, 0.0);
    s.h.assign(N, 0.0), s.tw.assign(N, 0.0), s.fixed.assign(T, 0u);
    std::vector<double> e(n + 1);
    for (int k = 0; k <= n; ++k) e[k] = (k == 0 || k == n) ? 0.0 : rng.uniform(0.01, 0.05);
    double sign = rng.sign();
    int left = 1 + (int)(rng.next() % 11);
    for (int k = 0; k < n; ++k) {
        s.lo[k] = e[k], s.up[k] = e[k + 1];
        s.dd[k] = rng.uniform(1.0, 3.0);
        s.ph[k] = (rng.next() % 5) ? rng.uniform(0.05, 1.0) : 0.0;
        s.r[k] = rng.uniform(-0.1, 0.1);
        s.c0[k] = sign * rng.uniform(1.0, 3.0);
        s.h[k] = (rng.next() % 4) ? rng.uniform(0.1, 2.0) : 0.0;
        s.tw[k] = rng.uniform(-1.0, 5.0);
        if (sign < 0) s.fixed[k / kC] |= 1u << (k % kC);
        if (--left == 0) sign = -sign, left = 1 + (int)(rng.next() % 11);
    }
    s.mask0 = s.fixed;
    if (!at_fixed_point)      // a few threads start from another set, at both ends, at a wave boundary and in between
        for (int t : {0, T / 2 - 1, T / 2, T - 1, 63 % T, 64 % T, (int)(rng.next() % (uint64_t)T)}) s.mask0[t] ^= 0xFu & (unsigned)(1 + rng.next() % 15);
    return s;
}

int step_sweep(int order) {
    Buffer B0, B1;
    long long reported = 0, cases = 0;
    for (int T : {64, 128, 192, 320, 1024})
        for (int fixed = 1; fixed >= 0; --fixed) {
            const int n = T * kC - (T == 64 ? 0 : 1 + T % 7);
            const StepData s = make_step(T, n, 0x5EED0000ull + (uint64_t)T * 2 + fixed, fixed != 0);
            std::vector<double> out((size_t)T * kWords), got;
            const std::string name = std::string("step T") + std::to_string(T) + (fixed ? " one pass" : " two passes");
            ++cases;
            bool bad = play_case(name, T, T / 4, step_body, B0, 3 * (size_t)T, B1, 3 * (size_t)T, out, [&] {
                g_step = StepJob{T, n, order, B0.p(), B1.p(), out.data(), s.lo.data(), s.up.data(), s.dd.data(), s.ph.data(), s.r.data(),
                                 s.c0.data(), s.h.data(), s.tw.data(), s.mask0.data()};
                std::memset(g_vote, 0, sizeof(g_vote));
                std::memset(g_votes_taken, 0, sizeof(g_votes_taken));
            }, false, &got);
            // under the first schedule: the number of passes, and every halo against the directly indexed neighbour
            auto wrong = [&](const std::string &what) {
                if (!bad) std::printf("REPORT %s: %s\n", name.c_str(), what.c_str()), ++g_totals.reported;
                bad = true;
            };
            for (int t = 0; t < T && !bad; ++t) {
                const double *o = got.data() + (size_t)t * kWords;
                const int passes = (int)o[kWords - 1], k0 = t * kC;
                if (passes != (fixed ? 1 : 2)) wrong("thread " + std::to_string(t) + " took " + std::to_string(passes) + " passes");
                auto gm = [&](int k) { return ((s.mask0[k / kC] >> (k % kC)) & 1u) ? s.ph[k] : 0.0; };
                const double rl = t ? s.r[k0 - 1] : 0.0, rr = t + 1 < T ? s.r[k0 + kC] : 0.0, gl = t ? gm(k0 - 1) : 0.0, gr = t + 1 < T ? gm(k0 + kC) : 0.0;
                if (o[0] != rl || o[1] != rr || o[2] != gl || o[3] != gr) wrong("thread " + std::to_string(t) + ": r's or g's halo is not its neighbours'");
                for (int p = 0; p < passes && !bad; ++p) {
                    const double *q = o + 4 + p * (kC + 3);
                    const double tbl = t ? tbar_of(g_step, k0 - 1, got[(size_t)(t - 1) * kWords + 4 + p * (kC + 3) + kC - 1]) : 0.0;
                    const double tbr = t + 1 < T ? tbar_of(g_step, k0 + kC, got[(size_t)(t + 1) * kWords + 4 + p * (kC + 3)]) : 0.0;
                    if (q[kC] != tbl || q[kC + 1] != tbr) wrong("thread " + std::to_string(t) + ", pass " + std::to_string(p) + ": Tbar's halo is not its neighbours'");
                    for (int i = 0; i < kC; ++i)
                        if (k0 + i < n && (q[i] < 0.0) != (s.c0[k0 + i] < 0.0)) wrong("thread " + std::to_string(t) + ": the solution's sign is not the fixed point's");
                }
            }
            reported += bad;
        }
    std::printf("reported step: %lld of %lld\n", reported, cases);
    return 0;
}

}  // namespace

// the vote: every thread's predicate into the vote's word, the barrier, the word
int __syncthreads_or(int changed) {
    const int k = g_votes_taken[play::g.cur]++;
    g_vote[k] |= changed != 0;
    play::barrier();
    return g_vote[k];
}

int main(int argc, char **argv) {
    const std::string command = argc > 1 ? argv[1] : "", order = argc > 2 ? argv[2] : "";
    int known = -1;
    if (argc == 5 && std::string(argv[3]) == "--seeds") g_seeds = std::atoi(argv[4]);
    else if (argc != 3) known = -2;
    const char *const names[] = {"shipped", "no-second-barrier", "read-before-vote", "tbar-in-p0"};
    if (command == "play" && known == -1 && g_seeds >= 0 && g_seeds <= 1000)
        for (int o = 0; o < 4; ++o)
            if (order == names[o]) known = step_sweep(o);
    if (known < 0) {
        std::fprintf(stderr, "usage: %s play shipped|no-second-barrier|read-before-vote|tbar-in-p0 [--seeds N]\n", argv[0]);
        return 2;
    }
    std::printf("runs cases %lld schedules %zu runs %lld barriers %lld reported %lld\n", g_totals.cases, schedules().size(),
                g_totals.runs, g_totals.barriers, g_totals.reported);
    return g_totals.reported ? 1 : 0;
}
