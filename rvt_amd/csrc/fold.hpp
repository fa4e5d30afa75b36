// Split-K folds: the reduction launches behind every kernel that leaves per-slice or per-workgroup fp32 partials in a workspace
// (the split-K weight-gradient GEMMs of gemm.hpp / ppgemm_tn.hpp, the in-kernel weight gradients of the MLP and ConvLSTM-scan parts).
//
// The one helper header that holds kernels: splitk_reduce_kernel, strided_reduce_kernel and fold_jobs_kernel.  They are `static`
// (internal linkage), because every part of the library that includes this file gets its own copy of the three.
#pragma once
#include "common.hpp"

namespace rvt {

// A workgroup owns 32 consecutive outputs x 8 slice lanes: thread (e, g) sums slices g, g + 8, ... of output e
// (four independent chains), the eight partial sums meet in LDS in a fixed order (deterministic).  The one-thread-per-output
// form walked all slices in one thread: nsplit / 8 dependent round trips - 10-20 us for the 256-512 slices of the small
// weight gradients, 1.2 ms per Base step over 73 launches.  Grid: reduce_grid(count) workgroups (any grid is correct).
inline int reduce_grid(size_t count) {
    size_t g = (count + 31) / 32;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
template <class Addr>
__device__ __forceinline__ void reduce_rows_32x8(const float* __restrict__ ws, int nrec, size_t count, const Addr& addr,
                                                  float* __restrict__ out, int t_cols, unsigned bid, unsigned nblk) {
    __shared__ float red[8][33];
    const int e = threadIdx.x & 31, g = threadIdx.x >> 5;
    for (size_t i0 = (size_t)bid * 32; i0 < count; i0 += (size_t)nblk * 32) {
        const size_t i = i0 + e;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        if (i < count) {
            int s = g;
            for (; s + 24 < nrec; s += 32) {
                a0 += ws[addr(s) + i]; a1 += ws[addr(s + 8) + i]; a2 += ws[addr(s + 16) + i]; a3 += ws[addr(s + 24) + i];
            }
            for (; s < nrec; s += 8) a0 += ws[addr(s) + i];
        }
        red[g][e] = (a0 + a1) + (a2 + a3);
        __syncthreads();
        if (g == 0 && i < count) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) t += red[k][e];
            size_t o = i;
            if (t_cols > 0) { const size_t r = i / t_cols, c = i % t_cols; o = c * (count / t_cols) + r; }
            out[o] += t;
        }
        __syncthreads();
    }
}
// out[i] += sum_s ws[s][i]; with t_cols > 0 the partial tiles are [count / t_cols][t_cols] and `out` is their transpose
static __global__ void __launch_bounds__(256)
splitk_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int nsplit, size_t count, int t_cols) {
    reduce_rows_32x8(ws, nsplit, count, [count](int s) { return (size_t)s * count; }, out, t_cols, blockIdx.x, gridDim.x);
}
// out[i] += sum_s ws[s * stride + i], i < count  (per-workgroup partial RECORDS of `stride` floats each)
static __global__ void __launch_bounds__(256)
strided_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out, int nrec, size_t stride, size_t count) {
    reduce_rows_32x8(ws, nrec, count, [stride](int s) { return (size_t)s * stride; }, out, 0, blockIdx.x, gridDim.x);
}
// Several folds of ONE producer launch in one launch (round 6): a weight gradient and its bias column sums, the four outputs of
// an MLP weight-gradient kernel, a ConvLSTM weight block and its bias rows.  73 fold launches per RVT-Base step were 0.8 ms, most
// of it the launches themselves (a bias fold is one or two workgroups).  Job j owns the workgroups [block0, block0 + blocks).
struct FoldJob { const float* ws; float* out; size_t count, stride, sub_stride; int nrec, t_cols, sub; unsigned block0, blocks; };
struct FoldJobs {
    static constexpr int MAX = 4;
    FoldJob j[MAX]; int n; unsigned total;
    FoldJobs() : n(0), total(0) {}
    // out[i] += sum_s ws[s * stride + i], i < count; t_cols as splitk_reduce_kernel.  sub > 1: every record holds `sub` rows, sub_stride
    // apart, that all fold into the SAME output (two jobs must never share an output: their workgroups run side by side).
    void add(const float* ws, float* out, int nrec, size_t stride, size_t count, int t_cols = 0, int sub = 1, size_t sub_stride = 0) {
        FoldJob& f = j[n++];
        f.ws = ws; f.out = out; f.count = count; f.stride = stride; f.nrec = nrec * sub; f.t_cols = t_cols; f.sub = sub; f.sub_stride = sub_stride;
        f.block0 = total; f.blocks = (unsigned)reduce_grid(count);
        total += f.blocks;
    }
};
static __global__ void __launch_bounds__(256)
fold_jobs_kernel(FoldJobs jobs) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < FoldJobs::MAX; i++) k += (i < jobs.n && blockIdx.x >= jobs.j[i].block0) ? 1 : 0;
    const FoldJob f = jobs.j[k];
    const size_t stride = f.stride, sub_stride = f.sub_stride;
    const int sub = f.sub;
    if (sub == 1)
        reduce_rows_32x8(f.ws, f.nrec, f.count, [stride](int s) { return (size_t)s * stride; }, f.out, f.t_cols, blockIdx.x - f.block0, f.blocks);
    else
        reduce_rows_32x8(f.ws, f.nrec, f.count, [stride, sub_stride, sub](int s) { return (size_t)(s / sub) * stride + (size_t)(s % sub) * sub_stride; },
                         f.out, f.t_cols, blockIdx.x - f.block0, f.blocks);
}
inline void launch_fold_jobs(const FoldJobs& jobs, hipStream_t st) {
    if (jobs.n > 0) hipLaunchKernelGGL(fold_jobs_kernel, dim3(jobs.total), dim3(256), 0, st, jobs);
}

}  // namespace rvt
