// The optimizer step on the device: gradient clipping by value, AdamW and the OneCycle learning-rate schedule for every parameter of
// every parameter group in ONE table-driven launch.  Reference: modules/detection.py:360-392 (configure_optimizers: th.optim.AdamW +
// OneCycleLR, linear, cycle_momentum=False), train.py (gradient_clip_val by VALUE), i.e. per step and parameter
//     clip_grad_value_(g, clip);  AdamW without amsgrad (decoupled weight decay);  scheduler.step()
//
// Two device tables the host builds once (rows declared in include/rvt_hip.h; built by rvt_amd/optim.py):
//   chunks: one OptimChunk per piece of at most OPTIM_CHUNK consecutive elements of one parameter (a tensor shorter than that is one
//           entry), naming the piece of the parameter, its gradient and its two moments, and the parameter group it belongs to;
//   groups: one OptimGroup per parameter group, all double like the Python floats torch keeps them in.
// The step count lives on the device too (`step` = optimizer steps done so far): the launch reads k = *step + 1, a trailing
// one-thread launch of the same library call writes it back, so every workgroup sees the same k and a captured graph replays with
// nothing written by the host.
//
// Per workgroup, once per parameter group it meets, in double (optim_scalars):
//     lr  = OneCycle schedule at position k - 1 (optim_lr below);  bc1 = 1 - beta1^k;  bc2 = 1 - beta2^k
//     and each constant torch hands to its fp32 tensor ops, rounded to fp32 once: 1 - lr*wd, 1 - beta1, beta2, 1 - beta2, lr / bc1,
//     sqrt(bc2), eps.  beta^k is a square-and-multiply product (k is an integer; at most 126 double multiplications).
// Per element, in fp32, one rounded operation each (this translation unit is compiled with -ffp-contract=off):
//     g = clamp(g, -clip, +clip)            (clip < 0: no clipping; the STORED gradient is not modified)
//     p = p * (1 - lr*wd)
//     m = m + (1 - beta1) * (g - m)
//     v = beta2 * v + ((1 - beta2) * g) * g
//     p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
// A pure streaming kernel: 16 bytes read, 12 written per element.  A chunk whose four pointers are 16-byte aligned moves as float4
// per lane (a full chunk: four float4 per array and lane, all sixteen loads issued before the first use); an unaligned chunk and the
// last n % 4 elements of a chunk go element by element.  Plain vector stores, no atomics, no LDS.
#pragma once
#include "common.hpp"

namespace rvt {

constexpr int OPTIM_THREADS = 256;
constexpr int OPTIM_CHUNK = RVT_OPTIM_CHUNK_ELEMS;    // elements per table entry: 4 float4 per lane
constexpr int OPTIM_MAX_GRID = 2048;                  // 256 CUs x 8 workgroups; the chunks beyond are walked grid-stride

// the rows are declared in include/rvt_hip.h; the empty derived structs keep the kernel's symbol name
struct OptimChunk : RvtOptimChunk {};
static_assert(sizeof(OptimChunk) == 40 && sizeof(OptimChunk) == sizeof(RvtOptimChunk), "OptimChunk layout is part of the C ABI");
struct OptimGroup : RvtOptimGroup {};
static_assert(sizeof(OptimGroup) == 80 && sizeof(OptimGroup) == sizeof(RvtOptimGroup), "OptimGroup layout is part of the C ABI");

struct OptimScalars { float clip, decay, w1, beta2, w2, step, bc2s, eps; };

// torch.optim.lr_scheduler.OneCycleLR (three_phase=False, anneal_strategy='linear') at position pos = steps done so far.
// Past the last position torch raises; here the rate stays at its final value.
__device__ __forceinline__ double optim_lr(const OptimGroup& gr, double pos) {
    if (pos <= gr.warm_end) return gr.warm_end > 0.0 ? (gr.lr_max - gr.lr_init) * (pos / gr.warm_end) + gr.lr_init : gr.lr_max;
    if (pos <= gr.last) return (gr.lr_final - gr.lr_max) * ((pos - gr.warm_end) / (gr.last - gr.warm_end)) + gr.lr_max;
    return gr.lr_final;
}

__device__ __forceinline__ double optim_powi(double b, long long k) {
    double r = 1.0;
    for (; k > 0; k >>= 1) {
        if (k & 1) r *= b;
        b *= b;
    }
    return r;
}

__device__ __forceinline__ OptimScalars optim_scalars(const OptimGroup& gr, long long k) {
    const double lr = optim_lr(gr, (double)(k - 1));
    const double bc1 = 1.0 - optim_powi(gr.beta1, k), bc2 = 1.0 - optim_powi(gr.beta2, k);
    OptimScalars s;
    s.clip = (float)gr.clip;
    s.decay = (float)(1.0 - lr * gr.weight_decay);
    s.w1 = (float)(1.0 - gr.beta1);
    s.beta2 = (float)gr.beta2;
    s.w2 = (float)(1.0 - gr.beta2);
    s.step = (float)(lr / bc1);
    s.bc2s = (float)sqrt(bc2);
    s.eps = (float)gr.eps;
    return s;
}

__device__ __forceinline__ void optim_update(const OptimScalars& s, float& p, float g, float& m, float& v) {
    if (s.clip >= 0.f) g = g < -s.clip ? -s.clip : (g > s.clip ? s.clip : g);
    p = p * s.decay;
    m = m + s.w1 * (g - m);
    v = s.beta2 * v + (s.w2 * g) * g;
    p = p - s.step * (m / (sqrtf(v) / s.bc2s + s.eps));
}

__device__ __forceinline__ void optim_update4(const OptimScalars& s, f32x4& p, const f32x4& g, f32x4& m, f32x4& v) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float pu = p[u], mu = m[u], vu = v[u];
        optim_update(s, pu, g[u], mu, vu);
        p[u] = pu; m[u] = mu; v[u] = vu;
    }
}

// The step of every chunk this workgroup owns.  GUARDED (rvt_optim_step_guarded): every workgroup reads verdict[0], the non-finite
// total of the latest rvt_grad_stats, first and touches nothing when it is not zero; with a zero verdict the two instantiations run
// the same instructions on the same values.
template <bool GUARDED>
__device__ __forceinline__ void optim_step_body(const OptimChunk* __restrict__ chunks, int n_chunks, const OptimGroup* __restrict__ groups,
                                                int n_groups, const long long* __restrict__ step, const long long* __restrict__ verdict) {
    constexpr int T = OPTIM_THREADS, NV = OPTIM_CHUNK / (4 * OPTIM_THREADS);
    if (GUARDED && verdict[0] != 0) return;
    const int tid = threadIdx.x;
    const long long k = *step + 1;
    int cur = -1;
    OptimScalars s = {};
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const OptimChunk ch = chunks[c];
        if (ch.group < 0 || ch.group >= n_groups) continue;            // (a table the host did not build: touch nothing)
        if (ch.group != cur) {
            cur = ch.group;
            s = optim_scalars(groups[cur], k);
        }
        const int n = ch.n < OPTIM_CHUNK ? ch.n : OPTIM_CHUNK;
        const bool aligned = (((size_t)ch.p | (size_t)ch.g | (size_t)ch.m | (size_t)ch.v) & 15) == 0;
        int done = 0;
        if (aligned && n == OPTIM_CHUNK) {
            f32x4 p[NV], g[NV], m[NV], v[NV];
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int i = (j * T + tid) * 4;
                g[j] = *reinterpret_cast<const f32x4*>(ch.g + i);
                p[j] = *reinterpret_cast<const f32x4*>(ch.p + i);
                m[j] = *reinterpret_cast<const f32x4*>(ch.m + i);
                v[j] = *reinterpret_cast<const f32x4*>(ch.v + i);
            }
#pragma unroll
            for (int j = 0; j < NV; j++) {
                const int i = (j * T + tid) * 4;
                optim_update4(s, p[j], g[j], m[j], v[j]);
                *reinterpret_cast<f32x4*>(ch.p + i) = p[j];
                *reinterpret_cast<f32x4*>(ch.m + i) = m[j];
                *reinterpret_cast<f32x4*>(ch.v + i) = v[j];
            }
            continue;
        }
        if (aligned) {
            for (int i = tid * 4; i + 4 <= n; i += T * 4) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(ch.g + i);
                f32x4 p = *reinterpret_cast<const f32x4*>(ch.p + i);
                f32x4 m = *reinterpret_cast<const f32x4*>(ch.m + i);
                f32x4 v = *reinterpret_cast<const f32x4*>(ch.v + i);
                optim_update4(s, p, g, m, v);
                *reinterpret_cast<f32x4*>(ch.p + i) = p;
                *reinterpret_cast<f32x4*>(ch.m + i) = m;
                *reinterpret_cast<f32x4*>(ch.v + i) = v;
            }
            done = n & ~3;
        }
        for (int i = done + tid; i < n; i += T) {
            float p = ch.p[i], m = ch.m[i], v = ch.v[i];
            optim_update(s, p, ch.g[i], m, v);
            ch.p[i] = p; ch.m[i] = m; ch.v[i] = v;
        }
    }
}

__global__ void __launch_bounds__(OPTIM_THREADS)
optim_step_kernel(const OptimChunk* __restrict__ chunks, int n_chunks, const OptimGroup* __restrict__ groups, int n_groups,
                  const long long* __restrict__ step) {
    optim_step_body<false>(chunks, n_chunks, groups, n_groups, step, nullptr);
}

__global__ void __launch_bounds__(OPTIM_THREADS)
optim_step_guarded_kernel(const OptimChunk* __restrict__ chunks, int n_chunks, const OptimGroup* __restrict__ groups, int n_groups,
                          const long long* __restrict__ step, const long long* __restrict__ verdict) {
    optim_step_body<true>(chunks, n_chunks, groups, n_groups, step, verdict);
}

// stream-ordered behind optim_step_kernel: the one writer of the step count
__global__ void optim_advance_kernel(long long* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step = *step + 1;
}

}  // namespace rvt
