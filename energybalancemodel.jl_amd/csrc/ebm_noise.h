// Forcing noise on the device: the Philox generator, the innovation, and a column's AR(1) state inside a step kernel.
#pragma once
#include "ebm_device.h"

namespace ebm {

// ---- forcing noise (ebm_set_column_noise; THE DEFINITION is in include/ebm_hip.h) ----------------------------------
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011; the Random123 constants): ten rounds, the key bumped between rounds.
// The operands are wave-uniform in the step kernels: scalar integer arithmetic.
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
    }
}
// xi(seed, stream, n): the standard normal innovation of global step n (two 53-bit uniforms, Box-Muller's first output).
// The one definition: the step kernels and noise_innovations_kernel (ebm_noise_innovations) call it.
__device__ __forceinline__ double noise_innovation(unsigned long long seed, unsigned long long stream, long long n) {
    const unsigned long long un = (unsigned long long)n;
    unsigned w[4] = {(unsigned)un, (unsigned)(un >> 32), (unsigned)stream, (unsigned)(stream >> 32)};
    philox4x32_10(w, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned long long ia = ((unsigned long long)w[0] << 21) | (w[1] >> 11);
    const unsigned long long ib = ((unsigned long long)w[2] << 21) | (w[3] >> 11);
    const double u1 = (double)(ia + 1) * 0x1p-53, u2 = (double)ib * 0x1p-53;     // (0, 1] and [0, 1), exact
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}
__device__ __forceinline__ double uniform_double(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// A column's noise inside a step kernel (only touched when a.noise is set).  load() runs before the workgroup's first
// barrier and store() — thread 0, an ordinary store — after its last: another wave's write-back of N_c can then never
// overtake this wave's read.  N_c <- rho*N_c + s*xi once per step (two products and a sum, no contraction).
struct ColumnNoise {
    double s, rho, N;
    unsigned long long stream;
    double Nv;                       // fused launches: lane l holds N_c after step l of the launch
    __device__ __forceinline__ void load(const StepArgs &a, int col) {
        typedef const __attribute__((address_space(4))) NoiseRec ConstNoise;     // never written by a kernel
        ConstNoise &r = *reinterpret_cast<ConstNoise *>(reinterpret_cast<uintptr_t>(a.noise + col));
        s = r.s;
        rho = r.rho;
        stream = r.stream;
        N = uniform_double(a.nstate[col]);                                        // written by kernels: a plain load
        Nv = 0.0;
    }
    __device__ __forceinline__ double advance(double xi) {
        N = rho * N + s * xi;
        return N;
    }
    __device__ __forceinline__ void store(const StepArgs &a, int col) const {
        if (threadIdx.x == 0) a.nstate[col] = N;
    }
    // Fused launches (a.nfused <= kNoiseMaxFused, the runtime's cap): the launch's innovations are independent of each
    // other, so lane l evaluates that of step l — one evaluation's latency per launch instead of one per step — and the
    // recurrence then runs over the lanes in step order (wave-uniform): lane l ends with N_c after step l.  The step loop
    // only reads N_c of its step.  Where it is held (MEM, a kernel template argument):
    //   registers  (miz_fused_kernel up to kFusedRegThreads threads: the latency-bound shapes) every wave of the
    //              workgroup runs this at the start of the launch, before the state is loaded, and keeps Nv (two VGPRs);
    //   memory     (every other fused-K kernel: their register budgets are spent) noise_sequence_kernel runs it before the
    //              launch, into the column's row of a.nseq, and also advances N_c; the step reads entry `step` of the
    //              row beside the step's other table loads, and the kernel touches no other noise word.
    // -DEBM_NOISE_SERIAL (A/B timing builds only, profiles/r07_noise_cost.txt): the register kernels evaluate every step's
    // innovation inside the loop instead, on the scalar path (this spills registers).
    __device__ __forceinline__ double sequence(const StepArgs &a, int nloop) {
        const int l = (int)(threadIdx.x & 63u);
        const double xi = l < nloop ? noise_innovation(a.seed, stream, a.sched[a.slot + l].n) : 0.0;
        double n = N, nl = 0.0;
        for (int i = 0; i < nloop; ++i) {
            n = rho * n + s * __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(xi), i),
                                               __builtin_amdgcn_readlane(__double2loint(xi), i));
            nl = l == i ? n : nl;
        }
        N = n;
        return nl;
    }
    __device__ __forceinline__ void prepare_launch(const StepArgs &a, int nloop) {
#ifndef EBM_NOISE_SERIAL
        Nv = sequence(a, nloop);
#else
        (void)a;
        (void)nloop;
#endif
    }
    template <bool MEM>
    __device__ __forceinline__ double at_step(const StepArgs &a, int col, int step, long long n) {
        if constexpr (MEM) {
            // (the column made opaque: the row's address is formed at every step, not kept across the step loop)
            int c = col;
            asm volatile("" : "+s"(c));
            return uniform_double(a.nseq[(size_t)c * kNoiseMaxFused + step]);
        }
#ifndef EBM_NOISE_SERIAL
        (void)n;
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(Nv), step),
                                __builtin_amdgcn_readlane(__double2loint(Nv), step));
#else
        (void)step;
        return advance(noise_innovation(a.seed, stream, n));
#endif
    }
};
// The forcing of a one-step launch (global step n): column_forcing — with the column's offset `fcol` as the kernel's head
// has loaded it (StepHead) — plus N_c after its update if the handle has noise
__device__ __forceinline__ double step_forcing(const StepArgs &a, ColumnNoise &nz, int col, double ft, double fcol, double tyear, long long n) {
    const double f = schedule_forcing(a, col, a.fcol ? ft + fcol : ft, tyear);
    return a.noise ? f + nz.advance(noise_innovation(a.seed, nz.stream, n)) : f;
}

}  // namespace ebm
