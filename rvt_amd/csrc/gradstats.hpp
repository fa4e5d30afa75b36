// Gradient statistics and the non-finite verdict on the device: what the reference's GradFlowLogCallback (callbacks/gradflow.py,
// callbacks/utils/visualization.py: param.grad.abs().mean() per named parameter) and the GradScaler of `precision: 16` (a step whose
// gradients hold an inf or a NaN is dropped) need from the gradients, as two launches over the optimizer's own chunk table
// (optim.hpp: OptimChunk).  Rows and records are declared in include/rvt_hip.h (RvtGradStat, RvtGradStatHead).
//
// gradstats_partial_kernel: workgroups stride over the chunks; one RvtGradStat per chunk into the workspace.
//     An element is non-finite when its exponent bits are all set: an integer test, which no fast-math flag folds away (this library
//     is compiled with -fno-honor-nans).  Per lane, in element order: sum |g| and sum g^2 in double over the finite gradient elements
//     ((double)g * (double)g is exact: 48 significant bits; FLT_MAX^2 = 1.2e77 is far from the double range), max |g| on the bit
//     patterns (for non-negative floats the unsigned order IS the float order, and no denormal mode can touch it), the int32 count of
//     the non-finite ones, and sum p^2 in double over the finite parameter elements.  Then a fixed xor-shuffle tree inside the wave,
//     the four wave results through LDS, folded by thread 0 in wave order.
// gradstats_fold_kernel: ONE workgroup of 16 waves.  Wave w folds tensors w, w + 16, ...: lane l adds the partial rows
//     first + l, first + l + 64, ... in that order, then the same shuffle tree; lane 0 writes the tensor's row into the ring slot
//     *step % ring.  After a barrier wave 0 folds the tensor rows, staged in LDS, into the slot's head and the verdict, strictly in
//     index order: ((r0 + r1) + r2) + ...
// No atomics anywhere: every sum has one fixed association, so the result is bit-reproducible and independent of the partial
// pass's grid.  16-byte loads when g and p of a chunk are 16-byte aligned, element by element otherwise (the rule of rvt_optim_step).
#pragma once
#include "common.hpp"
#include "optim.hpp"

namespace rvt {

constexpr int GRADSTAT_THREADS = OPTIM_THREADS;
constexpr int GRADSTAT_WAVES = GRADSTAT_THREADS / 64;
constexpr int GRADSTAT_FOLD_WAVES = 16;
constexpr int GRADSTAT_FOLD_THREADS = 64 * GRADSTAT_FOLD_WAVES;

static_assert(sizeof(RvtGradStat) == 32 && alignof(RvtGradStat) == 8, "RvtGradStat layout is part of the C ABI");
static_assert(sizeof(RvtGradStatHead) == 64 && alignof(RvtGradStatHead) == 8, "RvtGradStatHead layout is part of the C ABI");
static_assert(sizeof(((RvtGradStatHead*)0)->scalars) == 4 * RVT_GRADSTAT_MAX_SCALARS, "scalars[] holds RVT_GRADSTAT_MAX_SCALARS floats");

struct GradScalarPtrs { const float* p[RVT_GRADSTAT_MAX_SCALARS]; };

// the running statistics of one lane / wave / chunk / tensor; amax holds the bit pattern of max |g|
struct GradAcc {
    double abs_sum, sq_sum, param_sq_sum;
    unsigned amax;
    int nonfinite;
};

__device__ __forceinline__ GradAcc gradacc_zero() { return GradAcc{0.0, 0.0, 0.0, 0u, 0}; }

__device__ __forceinline__ void gradacc_element(GradAcc& a, float g, float p) {
    const unsigned gb = __builtin_bit_cast(unsigned, g), pb = __builtin_bit_cast(unsigned, p);
    if ((gb & 0x7f800000u) == 0x7f800000u) {
        a.nonfinite += 1;
    } else {
        const unsigned ab = gb & 0x7fffffffu;
        const double gd = (double)__builtin_bit_cast(float, ab);
        a.abs_sum += gd;
        a.sq_sum += gd * gd;
        a.amax = ab > a.amax ? ab : a.amax;
    }
    if ((pb & 0x7f800000u) != 0x7f800000u) {
        const double pd = (double)p;
        a.param_sq_sum += pd * pd;
    }
}

// a += b, field by field
__device__ __forceinline__ void gradacc_merge(GradAcc& a, const GradAcc& b) {
    a.abs_sum += b.abs_sum;
    a.sq_sum += b.sq_sum;
    a.param_sq_sum += b.param_sq_sum;
    a.amax = b.amax > a.amax ? b.amax : a.amax;
    a.nonfinite += b.nonfinite;
}

// xor-shuffle tree over the 64 lanes; every lane ends with the wave's result.  (lane ^ m adds symmetrically: x + y in both lanes,
// and fp64 addition commutes, so all lanes hold the same bits.)
__device__ __forceinline__ void gradacc_wave(GradAcc& a) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        GradAcc b;
        b.abs_sum = __shfl_xor(a.abs_sum, m);
        b.sq_sum = __shfl_xor(a.sq_sum, m);
        b.param_sq_sum = __shfl_xor(a.param_sq_sum, m);
        b.amax = __shfl_xor(a.amax, m);
        b.nonfinite = __shfl_xor(a.nonfinite, m);
        gradacc_merge(a, b);
    }
}

__device__ __forceinline__ GradAcc gradacc_load(const RvtGradStat& r) {
    return GradAcc{r.abs_sum, r.sq_sum, r.param_sq_sum, __builtin_bit_cast(unsigned, r.abs_max), r.nonfinite};
}

__device__ __forceinline__ void gradacc_store(RvtGradStat* r, const GradAcc& a) {
    r->abs_sum = a.abs_sum;
    r->sq_sum = a.sq_sum;
    r->param_sq_sum = a.param_sq_sum;
    r->abs_max = __builtin_bit_cast(float, a.amax);
    r->nonfinite = a.nonfinite;
}

__global__ void __launch_bounds__(GRADSTAT_THREADS)
gradstats_partial_kernel(const OptimChunk* __restrict__ chunks, int n_chunks, RvtGradStat* __restrict__ partial) {
    constexpr int T = GRADSTAT_THREADS, NV = OPTIM_CHUNK / (4 * GRADSTAT_THREADS);
    __shared__ GradAcc wave_acc[GRADSTAT_WAVES];
    const int tid = threadIdx.x;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimChunk ch = chunks[c];
        const int n = ch.n < 0 ? 0 : (ch.n < OPTIM_CHUNK ? ch.n : OPTIM_CHUNK);
        const bool aligned = (((size_t)ch.p | (size_t)ch.g) & 15) == 0;
        GradAcc a = gradacc_zero();
        int done = 0;
        if (aligned && n == OPTIM_CHUNK) {
            f32x4 g[NV], p[NV];
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int i = (j * T + tid) * 4;
                g[j] = *reinterpret_cast<const f32x4*>(ch.g + i);
                p[j] = *reinterpret_cast<const f32x4*>(ch.p + i);
            }
#pragma unroll
            for (int j = 0; j < NV; j++)
#pragma unroll
                for (int u = 0; u < 4; u++) gradacc_element(a, g[j][u], p[j][u]);
            done = n;
        } else if (aligned) {
            for (int i = tid * 4; i + 4 <= n; i += T * 4) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(ch.g + i);
                const f32x4 p = *reinterpret_cast<const f32x4*>(ch.p + i);
#pragma unroll
                for (int u = 0; u < 4; u++) gradacc_element(a, g[u], p[u]);
            }
            done = n & ~3;
        }
        for (int i = done + tid; i < n; i += T) gradacc_element(a, ch.g[i], ch.p[i]);
        gradacc_wave(a);
        if ((tid & 63) == 0) wave_acc[tid >> 6] = a;
        __syncthreads();
        if (tid == 0) {
            GradAcc r = wave_acc[0];
#pragma unroll
            for (int w = 1; w < GRADSTAT_WAVES; w++) gradacc_merge(r, wave_acc[w]);
            gradacc_store(partial + c, r);
        }
        __syncthreads();                                   // wave_acc is written again in the next round
    }
}

__global__ void __launch_bounds__(GRADSTAT_FOLD_THREADS)
gradstats_fold_kernel(const RvtGradStat* __restrict__ partial, const int* __restrict__ tensor_first, int n_tensors, int n_chunks,
                      const long long* __restrict__ step, GradScalarPtrs scalars, int n_scalars, RvtGradStat* __restrict__ stats,
                      int stat_stride, RvtGradStatHead* __restrict__ heads, int ring, long long* __restrict__ verdict) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long k = *step;
    const int slot = (int)(((k % ring) + ring) % ring);
    RvtGradStat* rows = stats + (size_t)slot * stat_stride;
    for (int t = wave; t < n_tensors; t += GRADSTAT_FOLD_WAVES) {
        int first = tensor_first[t], last = tensor_first[t + 1];
        first = first < 0 ? 0 : first;
        last = last > n_chunks ? n_chunks : last;          // (a table the host did not build: read nothing outside the workspace)
        GradAcc a = gradacc_zero();
        for (int c = first + lane; c < last; c += 64) gradacc_merge(a, gradacc_load(partial[c]));
        gradacc_wave(a);
        if (last <= first) a.nonfinite = -1;
        if (lane == 0) gradacc_store(rows + t, a);
    }
    // The totals.  sq_sum strictly in INDEX order, ((r0 + r1) + r2) + ...: the whole workgroup stages up to 1024 tensor rows in LDS
    // per round (behind the barrier the rows of this workgroup's other waves are visible), then wave 0 walks them in order; every
    // lane of it runs the same chain on LDS broadcasts, whose loads do not wait for the additions.
    __shared__ double s_sq[GRADSTAT_FOLD_THREADS];
    __shared__ unsigned s_max[GRADSTAT_FOLD_THREADS];
    __shared__ int s_nf[GRADSTAT_FOLD_THREADS];
    double sq = 0.0;
    unsigned amax = 0u;
    long long nonfinite = 0;
    for (int base = 0; base < n_tensors; base += GRADSTAT_FOLD_THREADS) {
        __syncthreads();                                   // the rows are written / the last round's LDS has been read
        const int t = base + tid;
        if (t < n_tensors) {
            const RvtGradStat r = rows[t];
            s_sq[tid] = r.sq_sum;
            s_max[tid] = __builtin_bit_cast(unsigned, r.abs_max);
            s_nf[tid] = r.nonfinite > 0 ? r.nonfinite : 0;
        }
        __syncthreads();
        if (wave == 0) {
            const int live = n_tensors - base < GRADSTAT_FOLD_THREADS ? n_tensors - base : GRADSTAT_FOLD_THREADS;
            for (int l = 0; l < live; l++) {
                sq += s_sq[l];
                amax = s_max[l] > amax ? s_max[l] : amax;
                nonfinite += s_nf[l];
            }
        }
    }
    if (wave != 0) return;
    RvtGradStatHead* h = heads + slot;
    if (lane == 0) {
        h->step = k;
        h->nonfinite = nonfinite;
        h->sq_sum = sq;
        h->abs_max = __builtin_bit_cast(float, amax);
        h->n_scalars = n_scalars;
        verdict[0] = nonfinite;
    }
    if (lane < RVT_GRADSTAT_MAX_SCALARS) h->scalars[lane] = lane < n_scalars ? *scalars.p[lane] : 0.f;
}

// the trailing launch of rvt_optim_step_guarded: the one writer of the step count and of the skip count
__global__ void optim_advance_guarded_kernel(long long* step, long long* verdict) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (verdict[0] != 0) verdict[1] = verdict[1] + 1;
        else *step = *step + 1;
    }
}

}  // namespace rvt
