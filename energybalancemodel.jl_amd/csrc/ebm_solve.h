// The tridiagonal solve of one meridian by one workgroup (chunk partition + parallel cyclic reduction in LDS) and the
// halo exchanges between neighbouring threads.
#pragma once
#ifndef EBM_SOLVE_ON_HOST   // tests/host_solve_main.cpp plays this header on the host and brings its own stand-ins; no build of the library defines it
#include "ebm_device.h"
#else
int __syncthreads_or(int);     // the vote, as tests/host_step_lds_main.cpp plays it; the solve's own player never calls it
#endif

namespace ebm {

// Halo exchange: every thread publishes its first and last value; returns the last value of
// the previous chunk and the first value of the next chunk (0 outside the meridian).
__device__ __forceinline__ void halo_exchange(double *E0, double *E1, int t, int T, double first,
                                              double last, double &left, double &right) {
    E0[t] = first;
    E1[t] = last;
    __syncthreads();
    const int tl = t > 0 ? t - 1 : 0, tr = t + 1 < T ? t + 1 : t;
    const double l = E1[tl], r = E0[tr];
    left = t > 0 ? l : 0.0;
    right = t + 1 < T ? r : 0.0;
}

// The same exchange for the kernel whose LDS holds the state: inside a wave through the lane crossbar, between waves
// through 32 words of E (wave w: last value at E[w], first value at E[16 + w]; T <= 1024).
__device__ __forceinline__ void halo_exchange_waves(double *E, int t, int T, double first, double last,
                                                    double &left, double &right) {
    const int lane = t & 63, w = t >> 6, nw = T >> 6;
    // (ds_bpermute with the lane taken from t, not __shfl_up / __shfl_down: their own lane id is loop-invariant and
    // would be kept in a register across the caller's step loop)
    auto from_lane = [](int src_lane, double v) {
        const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
        const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
        return __hiloint2double(hi, lo);
    };
    double l = from_lane((lane + 63) & 63, last), r = from_lane((lane + 1) & 63, first);
    if (lane == 63) E[w] = last;
    if (lane == 0) E[16 + w] = first;
    __syncthreads();
    const double pl = E[w > 0 ? w - 1 : 0], nr = E[16 + (w + 1 < nw ? w + 1 : w)];
    if (lane == 0) l = w > 0 ? pl : 0.0;
    if (lane == 63) r = w + 1 < nw ? nr : 0.0;
    left = l;
    right = r;
}

// Two halo exchanges behind one barrier, for two quantities that both exist before it (the one-step kernels' first Newton
// pass: r and the masked g).  a's first and last values and b's first go through P0's 3T doubles, b's last through P1[0, T).
// On entry P0 and P1[0, T) must be free.  On exit the neighbours may still be reading all four words: the caller puts a
// barrier between this call and its next write to P0 or to P1[0, T) — partition_solve_r's very first write is W1 = P1[t].
__device__ __forceinline__ void halo_exchange_two(double *P0, double *P1, int t, int T, double afirst, double alast,
                                                  double bfirst, double blast, double &aleft, double &aright,
                                                  double &bleft, double &bright) {
    P0[t] = afirst;
    P0[T + t] = alast;
    P0[2 * T + t] = bfirst;
    P1[t] = blast;
    __syncthreads();
    const int tl = t > 0 ? t - 1 : 0, tr = t + 1 < T ? t + 1 : t;
    const double al = P0[T + tl], ar = P0[tr], bl = P1[tl], br = P0[2 * T + tr];
    aleft = t > 0 ? al : 0.0;
    aright = t + 1 < T ? ar : 0.0;
    bleft = t > 0 ? bl : 0.0;
    bright = t + 1 < T ? br : 0.0;
}

// A halo exchange whose barrier is the workgroup's vote: every thread publishes its first and last value in P1[0, 2T), the
// vote (did any thread's `changed` differ from zero) is the barrier, the neighbours' words are read after it.  For a caller
// that has just left partition_solve_r (not COMPACT): P1 is free once the solve's last barrier is passed — P0 is not, the
// interface solution Y may still be read there.  On exit the neighbours may still be reading P1[0, 2T): the caller's next
// write to it (a solve's W1) must come after another barrier.  Returns the vote.
__device__ __forceinline__ bool publish_then_vote(double *P1, int t, int T, double first, double last, int changed,
                                                  double &left, double &right) {
    P1[t] = first;
    P1[T + t] = last;
    const bool any = __syncthreads_or(changed) != 0;
    const int tl = t > 0 ? t - 1 : 0, tr = t + 1 < T ? t + 1 : t;
    const double l = P1[T + tl], r = P1[tr];
    left = t > 0 ? l : 0.0;
    right = t + 1 < T ? r : 0.0;
    return any;
}

// ---- tridiagonal solve of one meridian, T threads x C rows -----------------------------------
// Row k: a_k x_{k-1} + b_k x_k + c_k x_{k+1} = d_k.  Thread t owns rows t*C..t*C+C-1.
//  1. Thomas-eliminate the C-1 leading rows of the chunk with the left interface value
//     L = x_{t*C-1} carried as a parameter:  x_i = dp_i + lp_i*L - cp_i*x_{i+1}.
//  2. Collapse that to the chunk's first unknown as an affine function of (L, R = x_{t*C+C-1}).
//  3. The chunk's last row, with x_{C-2} and the next chunk's first unknown substituted, is a
//     tridiagonal system in the T interface values y_t = x_{t*C+C-1}: solve it by parallel
//     cyclic reduction (normalised rows: one reciprocal per row per level) in LDS.
//  4. Back-substitute inside the chunk.
// P0/P1: 3T doubles each.  On entry P1 must be free and P0 free after the first barrier inside;
// on exit other threads may still be reading P0/P1 (callers put a barrier before reuse).
// Rows per thread of the second level: 4 at every workgroup size.  Measured with each variant passing
// test_every_workgroup_size (tests/tools/ab_variants.sh): 2 rows 0.1688, 8 rows 0.1681 against 0.1644 ms on the
// 4096 x 2048 shape; 2 rows for T <= 128 only (the 180-band shapes): within 0.3 % of 4 rows once the benchmark's state
// is pinned (--preroll 0).  -DEBM_SECOND_LEVEL_ROWS=n (2, 4 or 8) for A/B builds.
constexpr int second_level_rows(int /*T*/) {
#ifdef EBM_SECOND_LEVEL_ROWS
    return EBM_SECOND_LEVEL_ROWS;
#else
    return 4;
#endif
}

//
// COMPACT (miz_resident_kernel, whose LDS holds the state): the same arithmetic in 4T doubles instead of 6T — P0 = 3T,
// P1 = T.  The chunk summaries go through P0 as well (one more barrier before the interface rows overwrite them), the
// second level's summaries and the interface solution through P1, the reduction's two buffers through P0.  On entry
// P0 must be free and P1 free after the first barrier inside; on exit P0 is free and P1 may still be read.
template <int C, int R, bool COMPACT = false>
__device__ __forceinline__ void partition_solve_r(const double (&a)[C], const double (&b)[C],
                                                  const double (&c)[C], const double (&d)[C],
                                                  double (&x)[C], int t, int T, double *P0,
                                                  double *P1) {
    double cp[C - 1], dp[C - 1], lp[C - 1];
    {
        const double w = fast_rcp(b[0]);
        cp[0] = c[0] * w;
        dp[0] = d[0] * w;
        lp[0] = -a[0] * w;
    }
#pragma unroll
    for (int i = 1; i < C - 1; ++i) {
        const double w = fast_rcp(__builtin_fma(-a[i], cp[i - 1], b[i]));
        cp[i] = c[i] * w;
        dp[i] = __builtin_fma(-a[i], dp[i - 1], d[i]) * w;
        lp[i] = -(a[i] * lp[i - 1]) * w;
    }
    double u = dp[C - 2], v = lp[C - 2], wr = -cp[C - 2];
#pragma unroll
    for (int i = C - 3; i >= 0; --i) {
        u = __builtin_fma(-cp[i], u, dp[i]);
        v = __builtin_fma(-cp[i], v, lp[i]);
        wr = -cp[i] * wr;
    }
    double *const W1 = COMPACT ? P0 : P1;
    W1[t] = u;
    W1[T + t] = v;
    W1[2 * T + t] = wr;
    __syncthreads();
    const bool has_next = t + 1 < T;
    const int tn = has_next ? t + 1 : t;
    double un = W1[tn], vn = W1[T + tn], wn = W1[2 * T + tn];
    un = has_next ? un : 0.0;
    vn = has_next ? vn : 0.0;
    wn = has_next ? wn : 0.0;
    double pa, pc, pd;
    {
        const double ae = a[C - 1], be = b[C - 1], ce = c[C - 1], de = d[C - 1];
        const double RA = ae * lp[C - 2];
        const double RB = __builtin_fma(ce, vn, __builtin_fma(-ae, cp[C - 2], be));
        const double RC = ce * wn;
        const double RD = __builtin_fma(-ce, un, __builtin_fma(-ae, dp[C - 2], de));
        const double rinv = fast_rcp(RB);
        pa = RA * rinv;
        pc = RC * rinv;
        pd = RD * rinv;
    }
    // Second partition level: the T interface rows (unit diagonal) are handed to the first
    // G = T/R threads, R consecutive rows each, which repeat steps 1-3 on them; only the
    // G second-level interface rows go through parallel cyclic reduction.  Waves beyond the first
    // G threads only take part in the barriers.  Rows are exchanged through LDS transposed
    // (row q of group g at [q*G + g]) so that both sides access consecutive words.
    const int G = T / R;
    const bool lvl2 = t < G;
    if (COMPACT) __syncthreads();                         // the neighbours' summaries are read: P0 takes the rows
    {
        const int q = t % R, g = t / R;
        P0[q * G + g] = pa;
        P0[T + q * G + g] = pc;
        P0[2 * T + q * G + g] = pd;
    }
    __syncthreads();
    double a2[R], c2[R], d2[R], cq[R - 1], dq[R - 1], lq[R - 1];
    // U is dead once every second-level thread has read its neighbour's entry, i.e. after the barrier that follows the
    // S0 writes: the reduction's second buffer reuses it, and P1's 3T doubles suffice for R = 2 as well (6G = 3T)
    double *U = P1, *S0 = COMPACT ? P0 : P1 + 3 * G, *S1 = COMPACT ? P0 + 3 * G : P1;
    double *const Y = COMPACT ? P1 : P0;                  // the interface solution, row q of group g at [q*G + g]
    static_assert(R == 2 || R == 4 || R == 8, "second-level rows: P1 holds 6 T / R doubles");
    static_assert(!COMPACT || R >= 4, "compact: the 3 T / R second-level summaries share P1's T doubles");
    if (lvl2) {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            a2[i] = P0[i * G + t];
            c2[i] = P0[T + i * G + t];
            d2[i] = P0[2 * T + i * G + t];
        }
        cq[0] = c2[0];
        dq[0] = d2[0];
        lq[0] = -a2[0];
#pragma unroll
        for (int i = 1; i < R - 1; ++i) {
            const double w = fast_rcp(__builtin_fma(-a2[i], cq[i - 1], 1.0));
            cq[i] = c2[i] * w;
            dq[i] = __builtin_fma(-a2[i], dq[i - 1], d2[i]) * w;
            lq[i] = -(a2[i] * lq[i - 1]) * w;
        }
        double u2 = dq[R - 2], v2 = lq[R - 2], w2 = -cq[R - 2];
#pragma unroll
        for (int i = R - 3; i >= 0; --i) {
            u2 = __builtin_fma(-cq[i], u2, dq[i]);
            v2 = __builtin_fma(-cq[i], v2, lq[i]);
            w2 = -cq[i] * w2;
        }
        U[t] = u2;
        U[G + t] = v2;
        U[2 * G + t] = w2;
    }
    __syncthreads();
    double qa = 0.0, qc = 0.0, qd = 0.0;
    if (lvl2) {
        const bool nxt = t + 1 < G;
        const int gn = nxt ? t + 1 : t;
        double un2 = U[gn], vn2 = U[G + gn], wn2 = U[2 * G + gn];
        un2 = nxt ? un2 : 0.0;
        vn2 = nxt ? vn2 : 0.0;
        wn2 = nxt ? wn2 : 0.0;
        const double ae = a2[R - 1], ce = c2[R - 1], de = d2[R - 1];
        const double RA = ae * lq[R - 2];
        const double RB = __builtin_fma(ce, vn2, __builtin_fma(-ae, cq[R - 2], 1.0));
        const double RC = ce * wn2;
        const double RD = __builtin_fma(-ce, un2, __builtin_fma(-ae, dq[R - 2], de));
        const double rinv = fast_rcp(RB);
        qa = RA * rinv;
        qc = RC * rinv;
        qd = RD * rinv;
        S0[t] = qa;
        S0[G + t] = qc;
        S0[2 * G + t] = qd;
    }
    __syncthreads();
    // Out-of-range neighbours need no special case: by induction qa == 0 exactly whenever row
    // t-s does not exist (and qc == 0 when t+s does not), so reading a clamped, finite row and
    // multiplying by that zero contributes nothing.
    double *src = S0, *dst = S1;
    for (int s = 1; s < G; s <<= 1) {
        if (lvl2) {
            const int im = t - s >= 0 ? t - s : t, ip = t + s < G ? t + s : t;
            const double am = src[im], cm = src[G + im], dm = src[2 * G + im];
            const double ap = src[ip], cn = src[G + ip], dn = src[2 * G + ip];
            const double r = fast_rcp(__builtin_fma(-qc, ap, __builtin_fma(-qa, cm, 1.0)));
            const double nqd = __builtin_fma(-qc, dn, __builtin_fma(-qa, dm, qd)) * r;
            const double nqa = -(qa * am) * r;
            const double nqc = -(qc * cn) * r;
            qa = nqa;
            qc = nqc;
            qd = nqd;
            dst[t] = qa;
            dst[G + t] = qc;
            dst[2 * G + t] = qd;
        }
        __syncthreads();
        double *tmp = src;
        src = dst;
        dst = tmp;
    }
    if (lvl2) {
        const double L2raw = src[2 * G + (t > 0 ? t - 1 : 0)];
        const double L2 = t > 0 ? L2raw : 0.0;
        double y = qd;
        Y[(R - 1) * G + t] = y;   // the level-1 rows in P0 (compact: the summaries in P1) were consumed before the barriers above
#pragma unroll
        for (int i = R - 2; i >= 0; --i) {
            y = __builtin_fma(-cq[i], y, __builtin_fma(lq[i], L2, dq[i]));
            Y[i * G + t] = y;
        }
    }
    __syncthreads();
    pd = Y[(t % R) * G + t / R];
    const int tm = t > 0 ? t - 1 : 0;
    const double Lraw = Y[(tm % R) * G + tm / R];
    const double L = t > 0 ? Lraw : 0.0;
    x[C - 1] = pd;
#pragma unroll
    for (int i = C - 2; i >= 0; --i) x[i] = __builtin_fma(-cp[i], x[i + 1], __builtin_fma(lp[i], L, dp[i]));
}
// TT: the workgroup size if it is a compile-time constant (the MIZ kernels), 0 if only known at run time (classic)
template <int C, int TT = 0, bool COMPACT = false>
__device__ __forceinline__ void partition_solve(const double (&a)[C], const double (&b)[C],
                                                const double (&c)[C], const double (&d)[C],
                                                double (&x)[C], int t, int T, double *P0, double *P1) {
    // (run-time T: one copy of the solve only — two would take the classic K-step kernel past its 128 VGPRs)
    partition_solve_r<C, second_level_rows(TT != 0 ? TT : 1024), COMPACT>(a, b, c, d, x, t, T, P0, P1);
}

}  // namespace ebm
