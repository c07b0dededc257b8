// Device-side basics every kernel family may use: the streamed-store and stamp macros, the constant-address-space
// parameter block, the column lookups, Julia's IEEE semantics, the IEEE division of the bit-exact physics, the solves'
// reciprocal, a column's forcing, and the 16-byte chunk loads / stores.
#pragma once
#include "ebm_internal.h"

namespace ebm {

// Outputs are streamed: written once per step and not read again before the next launch.  With
// the non-temporal policy they do not allocate in L2 and drain faster (0.238 -> 0.217 ms per step on
// the 4096 x 2048 workload; the same policy on the loads was slower and is not used).
#if defined(EBM_TIMING_NO_STORES)
// Timing-only A/B build (never shipped, results are garbage): the streamed output stores are dropped, what
// remains is loads + arithmetic — the ceiling a design that hid every store would reach.  The values
// are kept alive so that the arithmetic is not eliminated.
#define EBM_STORE2(ptr, v)                                                            \
    do {                                                                              \
        asm volatile("" ::"v"((v).x), "v"((v).y), "s"(ptr));                          \
    } while (0)
#elif !defined(EBM_PLAIN_STORES)
typedef double ebm_dvec2 __attribute__((ext_vector_type(2)));
#define EBM_STORE2(ptr, v)                                                            \
    do {                                                                              \
        ebm_dvec2 t_;                                                                 \
        t_.x = (v).x;                                                                 \
        t_.y = (v).y;                                                                 \
        __builtin_nontemporal_store(t_, reinterpret_cast<ebm_dvec2 *>(ptr));          \
    } while (0)
#else
#define EBM_STORE2(ptr, v) (*reinterpret_cast<double2 *>(ptr) = (v))
#endif

// Diagnostic build only (-DEBM_STAMPS): wave 0 of every workgroup records s_memtime at phase
// boundaries into a.stamps[col*16 + n].  Never enabled in the shipped library.
#ifdef EBM_STAMPS
#define EBM_STAMP(n)                                                                   \
    do {                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                             \
        unsigned long long t_;                                                         \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
        __builtin_amdgcn_sched_barrier(0);                                             \
        if (threadIdx.x == 0 && a.stamps) a.stamps[(size_t)blockIdx.x * 16 + (n)] = t_; \
    } while (0)
// per-wave variant: lane 0 of every wave records into a.stamps[ncol*16 + (col*16 + wave)*8 + n]
#define EBM_STAMPW(n)                                                                  \
    do {                                                                               \
        __builtin_amdgcn_sched_barrier(0);                                             \
        unsigned long long t_;                                                         \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");      \
        __builtin_amdgcn_sched_barrier(0);                                             \
        if ((threadIdx.x & 63) == 0 && a.stamps)                                       \
            a.stamps[(size_t)a.ncol * 16 + ((size_t)blockIdx.x * 16 + (threadIdx.x >> 6)) * 8 + (n)] = t_; \
    } while (0)
// the two pairs are waited for here, so that the stamp that follows is taken once they have arrived
#define EBM_ARRIVED2(u, v) asm volatile("" ::"v"((u).x), "v"((u).y), "v"((v).x), "v"((v).y))
#else
#define EBM_STAMP(n) do {} while (0)
#define EBM_STAMPW(n) do {} while (0)
#define EBM_ARRIVED2(u, v) do {} while (0)
#endif

// The parameter block is never written by a kernel: read it through the constant address space so
// that every access is a scalar load, also after the kernel's own global stores (through a plain
// pointer hipcc falls back to per-lane vector loads once the kernel has stored anything).
typedef const __attribute__((address_space(4))) Params ConstParams;

// The parameter set of a column (ebm_set_column_params): one scalar load per workgroup, from the constant address space
// like the parameter block itself, and none without a table (every column set 0).  The column is the GLOBAL one
// (col0 + blockIdx.x: launch chains).
__device__ __forceinline__ int param_set(const StepArgs &a, int col) {
    typedef const __attribute__((address_space(4))) int ConstInt;
    return a.pset ? reinterpret_cast<ConstInt *>(reinterpret_cast<uintptr_t>(a.pset))[col] : 0;
}
// The column workgroup blockIdx.x of a launch steps: entry col0 + blockIdx.x of the active list (ebm_equilibrate: frozen
// columns get no workgroup), one scalar load per workgroup, none without a list (the identity).  The fused-K kernels and
// the classic kernel only: miz_step_kernel is never launched on a list.
__device__ __forceinline__ int step_column(const StepArgs &a) {
    typedef const __attribute__((address_space(4))) int ConstInt;
    const int b = a.col0 + (int)blockIdx.x;
    return a.cols ? reinterpret_cast<ConstInt *>(reinterpret_cast<uintptr_t>(a.cols))[b] : b;
}

// ---- Julia IEEE semantics ----------------------------------------------------------------
__device__ __forceinline__ double jl_min(double x, double y) {
    // Base.min(::Float64, ::Float64): NaN-propagating, -0.0 < +0.0
    double diff = x - y;
    double am = __builtin_signbit(diff) ? x : y;
    return (__builtin_isnan(x) || __builtin_isnan(y)) ? diff : am;
}
__device__ __forceinline__ double jl_clamp(double x, double lo, double hi) {
    return x > hi ? hi : (x < lo ? lo : x);
}
__device__ __forceinline__ double bool_mul(double x, bool b) {
    return b ? x : __builtin_copysign(0.0, x);   // Bool "strong zero"
}

// IEEE fp64 division for the bit-exact physics.  hipcc expands a/b to v_div_scale x2, v_rcp_f64,
// two Newton steps, a residual correction, v_div_fmas and v_div_fixup.  The two scalings and
// div_fmas only act when an operand or the quotient is near the exponent limits; for every other
// input the sequence below (the same instructions without the scaling) returns the same bits, and
// v_div_fixup still produces the IEEE results for zero, infinite and NaN operands.
// -DEBM_FULL_DIV selects the compiler's expansion instead.
__device__ __forceinline__ double div_rcp(double b) {     // refined reciprocal of the sequence
#if defined(EBM_TIMING_NO_TRANS)        // TIMING ONLY (results garbage): what the v_rcp_f64 themselves cost
    const double r0 = __builtin_bit_cast(double, 0x7FDE6238502484BAll - __builtin_bit_cast(long long, b));   // +-12 %
#else
    const double r0 = __builtin_amdgcn_rcp(b);
#endif
#if defined(EBM_TIMING_CHEAP_DIV)       // TIMING ONLY (results garbage): what all the refinement work costs
    return r0;
#else
    const double e0 = __builtin_fma(-b, r0, 1.0);
    const double r1 = __builtin_fma(r0, e0, r0);
    const double e1 = __builtin_fma(-b, r1, 1.0);
    return __builtin_fma(r1, e1, r1);
#endif
}
__device__ __forceinline__ double div_with_rcp(double a, double b, double r2) {
#if defined(EBM_FULL_DIV)
    return a / b;
#elif defined(EBM_TIMING_CHEAP_DIV)
    return a * r2;
#else
    const double q0 = a * r2;
    const double rem = __builtin_fma(-b, q0, a);
    const double q = __builtin_fma(rem, r2, q0);
    return __builtin_amdgcn_div_fixup(q, b, a);
#endif
}
__device__ __forceinline__ double ieee_div(double a, double b) {
#ifdef EBM_FULL_DIV
    return a / b;
#else
    return div_with_rcp(a, b, div_rcp(b));
#endif
}

// ---- solver arithmetic (not order-constrained) ---------------------------------------------
__device__ __forceinline__ double fast_rcp(double x) {
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}

// Forcing of one column at one step: the step's scalar, plus the column's constant offset, plus the
// column's own Forcing{false} schedule (src/infrastructure.jl:208-241) evaluated at the model time
// T of the step exactly as the reference does (:294-307): hold, ramp up, hold, ramp down, hold.
// (schedule_forcing: the schedule's part alone, on top of f = the step's scalar plus the column's offset — for the kernel
// that has requested the offset already, miz_step_kernel's StepHead)
__device__ __forceinline__ double schedule_forcing(const StepArgs &a, int col, double f, double tyear) {
    if (a.fsched) {
        const double *w = a.fsched + (size_t)kSchedWords * col;     // wave-uniform: scalar loads
        const double base = w[0], peak = w[1], cool = w[2], up = w[3], down = w[4];
        const double d1 = w[5], d2 = w[6], d3 = w[7], d4 = w[8];
        double v = cool;
        if (tyear < d1) v = base;
        else if (tyear < d2) v = base + up * (tyear - d1);
        else if (tyear < d3) v = peak;
        else if (tyear < d4) v = peak + down * (tyear - d3);
        f = f + v;
    }
    return f;
}
__device__ __forceinline__ double column_forcing(const StepArgs &a, int col, double ft, double tyear) {
    return schedule_forcing(a, col, a.fcol ? ft + a.fcol[col] : ft, tyear);
}

// ---- chunk loads / stores: 8*C contiguous bytes per lane, 16-byte accesses ------------------
// `f` is a wave-uniform base (kept in SGPRs), `k0` the lane's first cell: the access compiles to
// the saddr + voffset form, so no per-lane 64-bit pointers are kept alive.
template <int C>
__device__ __forceinline__ void load_chunk(const double *__restrict__ f, unsigned k0, double (&v)[C]) {
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        double2 d = *reinterpret_cast<const double2 *>(f + (k0 + 2 * j));
        v[2 * j] = d.x;
        v[2 * j + 1] = d.y;
    }
}
// The fields miz_step_kernel owns between its launches (the prognostics) and the diagnostic fields it stores are in the
// pair-split layout: where pair j of the lane whose first cell is k0 = 4t lies, split_index(t, j, T), as the sum of a
// wave-uniform part (the pair's) and the lane's part 2t, formed as k0/2 (C = 2: the natural place).
template <int C, int T>
__device__ __forceinline__ constexpr unsigned state_pair_base(int j) {
    return C == 4 ? split_index(0u, (unsigned)j, (unsigned)T) : 2u * (unsigned)j;
}
template <int C>
__device__ __forceinline__ unsigned state_lane(unsigned k0) { return C == 4 ? k0 / 2u : k0; }
template <int C, int T>
__device__ __forceinline__ unsigned state_index(unsigned k0, int j) { return state_pair_base<C, T>(j) + state_lane<C>(k0); }
template <int C, int T>
__device__ __forceinline__ void load_state(const double *__restrict__ f, unsigned k0, double (&v)[C]) {
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        double2 d = *reinterpret_cast<const double2 *>(f + state_index<C, T>(k0, j));
        v[2 * j] = d.x;
        v[2 * j + 1] = d.y;
    }
}
// ---- zero-line flags (miz_step_kernel, ZERO_LINES) -------------------------------------------
// One 32-bit word per (column, wave), behind the mask rows in their allocation (zero_flag_words, ebm_internal.h); bit
// 4*j + slot of it, slot = S_Ei, S_Ew, S_h, S_D: the KiB that the wave's access to pair j of that field covers in the
// pair-split layout holds only zero bits in HBM.  The word is wave-uniform: read with a scalar load through the constant
// address space (the kernel's one write to it is its last instruction), written by the wave's first lane.  A wave reads its
// OWN word before it writes it, and nobody else writes that word.  The SUCCESSOR's words, read for the prefetch, belong to a
// workgroup of the same launch that may be running already and storing them: what is read there may be the old or the new
// word, and it is a hint only — it decides which lines are prefetched, never what is loaded or stored.
__device__ __forceinline__ constexpr unsigned zero_flag_bit(int j, int slot) { return 1u << (4 * j + slot); }
template <int T>
__device__ __forceinline__ unsigned zero_flag_word(const StepArgs &a, int col, unsigned wave) {
    typedef const __attribute__((address_space(4))) unsigned ConstWord;
    return reinterpret_cast<ConstWord *>(reinterpret_cast<uintptr_t>(zero_flag_words(a.amask, a.ncol, T)))[(size_t)col * (T / 64) + wave];
}
template <int T>
__device__ __forceinline__ void store_zero_flag_word(const StepArgs &a, int col, int t, unsigned word) {
    if ((t & 63) == 0) zero_flag_words(a.amask, a.ncol, T)[(size_t)col * (T / 64) + ((unsigned)t >> 6)] = word;
}
// all 64 lanes' two values are zero bits (-0.0 is not)
__device__ __forceinline__ bool wave_holds_zero_bits(const double2 &d) {
    const bool mine = (__builtin_bit_cast(unsigned long long, d.x) | __builtin_bit_cast(unsigned long long, d.y)) != 0ull;
    return __builtin_amdgcn_ballot_w64(mine) == 0ull;
}
// one pair, or +0.0 without a load where the wave-uniform `flagged` is set
__device__ __forceinline__ double2 load_pair_unless_zero(const double *__restrict__ f, unsigned flagged) {
    double2 d;
    d.x = 0.0;
    d.y = 0.0;
    if (!flagged) d = *reinterpret_cast<const double2 *>(f);
    return d;
}
// load_state with the pairs whose flag is set left at +0.0: bit 4*j of `flags` is pair j's (the word shifted by the slot)
template <int C, int T>
__device__ __forceinline__ void load_state_unless_zero(const double *__restrict__ f, unsigned k0, double (&v)[C], unsigned flags) {
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        const double2 d = load_pair_unless_zero(f + state_index<C, T>(k0, j), flags & zero_flag_bit(j, 0));
        v[2 * j] = d.x;
        v[2 * j + 1] = d.y;
    }
}
// ---- the head of a one-step launch (miz_step_kernel) -------------------------------------------
// Every word that a wave needs before its first vector load and that depends on nothing but the kernel arguments and the
// column: its own zero-line flag word, the successor column's two (for the L2 prefetch), the step's scalars (entry `slot` of
// the schedule table, or the launch arguments), the column's forcing offset and its parameter set.  All are requested in
// one batch of scalar loads behind ONE wait: asked for one by one, each where it is first used, they form a chain of
// dependent scalar-cache misses in front of the state loads (profiles/EXPERIMENTS.md, r30).  A table that is absent is not
// branched around — the branch would end the batch: the load goes to the parameter block instead (a.p, always there and
// larger than any entry), and what it returns is dropped.
struct StepHead {
    unsigned zold, znext0, znext1;   // ZERO_LINES only (else 0)
    int pset;
    double ct, ft, tyear, fcol;      // fcol: the column's offset, +0.0 bits without a table (never added then)
    long long n;
};
template <bool ZERO_LINES, int T>
__device__ __forceinline__ StepHead step_head(const StepArgs &a, int col, unsigned wave) {
    typedef const __attribute__((address_space(4))) unsigned long long ConstU64;
    typedef const __attribute__((address_space(4))) int ConstInt;
    const uintptr_t spare = reinterpret_cast<uintptr_t>(a.p);
    StepHead h;
    h.zold = h.znext0 = h.znext1 = 0;
    if constexpr (ZERO_LINES) {
        constexpr unsigned W = T / 64;
        // (no successor: the column's own words, unused.  readfirstlane: free where the load is scalar, as in the shipped
        // library; the -DEBM_STAMPS build of the 64-thread kernel loads the words per lane, and the pin below wants SGPRs)
        const int nxt = (a.prefetch > 0 && col + a.prefetch < a.ncol) ? col + a.prefetch : col;
        h.zold = (unsigned)__builtin_amdgcn_readfirstlane((int)zero_flag_word<T>(a, col, wave));
        h.znext0 = (unsigned)__builtin_amdgcn_readfirstlane((int)zero_flag_word<T>(a, nxt, (2u * wave) % W));
        h.znext1 = (unsigned)__builtin_amdgcn_readfirstlane((int)zero_flag_word<T>(a, nxt, (2u * wave + 1u) % W));
    }
    ConstU64 *const se = reinterpret_cast<ConstU64 *>(a.sched ? reinterpret_cast<uintptr_t>(a.sched + a.slot) : spare);
    static_assert(sizeof(Params) >= sizeof(StepSched), "the spare target holds a whole entry");
    static_assert(offsetof(StepSched, ct) % 8 == 0 && offsetof(StepSched, ft) % 8 == 0 && offsetof(StepSched, tyear) % 8 == 0 &&
                  offsetof(StepSched, n) % 8 == 0 && sizeof(double) == 8 && sizeof(long long) == 8, "the entry as 64-bit words");
    unsigned long long ct = se[offsetof(StepSched, ct) / 8], ft = se[offsetof(StepSched, ft) / 8],
                       ty = se[offsetof(StepSched, tyear) / 8], n = se[offsetof(StepSched, n) / 8];
    unsigned long long fc = reinterpret_cast<ConstU64 *>(a.fcol ? reinterpret_cast<uintptr_t>(a.fcol + col) : spare)[0];
    int ps = reinterpret_cast<ConstInt *>(a.pset ? reinterpret_cast<uintptr_t>(a.pset + col) : spare)[0];
    // the one wait: every word is consumed here, so every request stands above this line and none is sunk to its use
    // (one asm for all of them, and not `volatile`: hipcc takes a volatile asm for a write to memory and reads every
    // plain-pointer word after it — the forcing schedule, N_c — with per-lane vector loads instead of scalar ones)
    if constexpr (ZERO_LINES)
        asm("" : "+s"(h.zold), "+s"(h.znext0), "+s"(h.znext1), "+s"(ct), "+s"(ft), "+s"(ty), "+s"(n), "+s"(fc), "+s"(ps));
    else
        asm("" : "+s"(ct), "+s"(ft), "+s"(ty), "+s"(n), "+s"(fc), "+s"(ps));
    if constexpr (ZERO_LINES) {
        constexpr unsigned W = T / 64;
        h.znext0 >>= 4u * ((2u * wave) / W);
        h.znext1 >>= 4u * ((2u * wave + 1u) / W);
    }
    h.ct = a.sched ? __builtin_bit_cast(double, ct) : a.ct;
    h.ft = a.sched ? __builtin_bit_cast(double, ft) : a.ft;
    h.tyear = a.sched ? __builtin_bit_cast(double, ty) : a.tyear;
    h.n = a.sched ? (long long)n : a.step;
    h.fcol = __builtin_bit_cast(double, fc);
    h.pset = a.pset ? ps : 0;
    return h;
}
// The same words asked for in place, each where it is first used and none where its table is absent: the head of the kernels
// that do not take the batch (miz_step_kernel: IMEX, two cells per thread; none of them elides zero lines).
__device__ __forceinline__ StepHead step_head_in_place(const StepArgs &a, int col) {
    StepHead h;
    h.zold = h.znext0 = h.znext1 = 0;
    h.pset = param_set(a, col);
    h.ct = a.sched ? a.sched[a.slot].ct : a.ct;
    h.ft = a.sched ? a.sched[a.slot].ft : a.ft;
    h.tyear = a.sched ? a.sched[a.slot].tyear : a.tyear;
    h.n = a.sched ? a.sched[a.slot].n : a.step;
    h.fcol = a.fcol ? a.fcol[col] : 0.0;
    return h;
}

template <int C>
__device__ __forceinline__ void store_chunk(double *__restrict__ f, const double (&v)[C], unsigned k0, int nlat) {
#pragma unroll
    for (int j = 0; j < C / 2; ++j) {
        double2 d;
        d.x = ((int)k0 + 2 * j < nlat) ? v[2 * j] : 0.0;           // padding cells stay zero
        d.y = ((int)k0 + 2 * j + 1 < nlat) ? v[2 * j + 1] : 0.0;
        EBM_STORE2(f + (k0 + 2 * j), d);
    }
}

}  // namespace ebm
