// extern "C" entry points, part 14: the optimizer step (optim.hpp; reference modules/detection.py configure_optimizers and the
// trainer's gradient clipping by value), the gradient statistics over the same chunk table and the step that obeys their non-finite
// verdict (gradstats.hpp; reference callbacks/gradflow.py and the GradScaler step-skip of `precision: 16`).  Compiled without fused multiply-add contraction (Makefile): every fp32 and fp64 line of
// the update is one rounded operation, as in torch's unfused AdamW and in the scheduler's Python arithmetic.
#include <stdint.h>

#include "host.hpp"
#include "optim.hpp"
#include "gradstats.hpp"

using namespace rvt;

extern "C" {

int rvt_optim_step(const RvtOptimChunk* chunks, int n_chunks, const RvtOptimGroup* groups, int n_groups, long long* step, int max_blocks, void* stream) {
    RVT_CHECK(chunks && groups && step, "optim_step: null argument");
    RVT_CHECK(n_chunks >= 1 && n_groups >= 1, "optim_step: n_chunks=%d n_groups=%d must be positive", n_chunks, n_groups);
    RVT_CHECK(max_blocks >= 0, "optim_step: max_blocks=%d is negative", max_blocks);
    RVT_CHECK(((uintptr_t)chunks & 7) == 0 && ((uintptr_t)groups & 7) == 0 && ((uintptr_t)step & 7) == 0,
              "optim_step: tables and step count must be 8-byte aligned");
    const int cap = max_blocks > 0 ? imin(max_blocks, OPTIM_MAX_GRID) : OPTIM_MAX_GRID;
    hipStream_t st = (hipStream_t)stream;
    // (OptimChunk / OptimGroup add nothing to the header's rows - same size, asserted in optim.hpp - and exist only for the kernel's
    //  symbol name: the downcast re-labels device memory that the host never dereferences)
    hipLaunchKernelGGL(optim_step_kernel, dim3((unsigned)imin(n_chunks, cap)), dim3(OPTIM_THREADS), 0, st, static_cast<const OptimChunk*>(chunks),
                       n_chunks, static_cast<const OptimGroup*>(groups), n_groups, (const long long*)step);
    RVT_TRY(check_launch("optim_step"));
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, st, step);
    return check_launch("optim_step (advance)");
}

int rvt_optim_step_guarded(const RvtOptimChunk* chunks, int n_chunks, const RvtOptimGroup* groups, int n_groups, long long* step,
                           long long* verdict, int max_blocks, void* stream) {
    RVT_CHECK(chunks && groups && step && verdict, "optim_step_guarded: null argument");
    RVT_CHECK(n_chunks >= 1 && n_groups >= 1, "optim_step_guarded: n_chunks=%d n_groups=%d must be positive", n_chunks, n_groups);
    RVT_CHECK(max_blocks >= 0, "optim_step_guarded: max_blocks=%d is negative", max_blocks);
    RVT_CHECK((((uintptr_t)chunks | (uintptr_t)groups | (uintptr_t)step | (uintptr_t)verdict) & 7) == 0,
              "optim_step_guarded: tables, step count and verdict must be 8-byte aligned");
    const int cap = max_blocks > 0 ? imin(max_blocks, OPTIM_MAX_GRID) : OPTIM_MAX_GRID;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(optim_step_guarded_kernel, dim3((unsigned)imin(n_chunks, cap)), dim3(OPTIM_THREADS), 0, st,
                       static_cast<const OptimChunk*>(chunks), n_chunks, static_cast<const OptimGroup*>(groups), n_groups,
                       (const long long*)step, (const long long*)verdict);
    RVT_TRY(check_launch("optim_step_guarded"));
    hipLaunchKernelGGL(optim_advance_guarded_kernel, dim3(1), dim3(1), 0, st, step, verdict);
    return check_launch("optim_step_guarded (advance)");
}

size_t rvt_grad_stats_ws_bytes(int n_chunks) { return n_chunks > 0 ? (size_t)n_chunks * sizeof(RvtGradStat) : 0; }

int rvt_grad_stats(const RvtOptimChunk* chunks, int n_chunks, const int* tensor_first, int n_tensors, const long long* step,
                   const float* const* scalars, int n_scalars, RvtGradStat* stats, int stat_stride, RvtGradStatHead* heads, int ring,
                   long long* verdict, void* ws, size_t ws_bytes, int max_blocks, void* stream) {
    RVT_CHECK(chunks && tensor_first && step && stats && heads && verdict && ws, "grad_stats: null argument");
    RVT_CHECK(n_chunks >= 1 && n_tensors >= 1, "grad_stats: n_chunks=%d n_tensors=%d must be positive", n_chunks, n_tensors);
    RVT_CHECK(ring >= 1, "grad_stats: ring=%d must be at least 1", ring);
    RVT_CHECK(stat_stride >= n_tensors, "grad_stats: stat_stride=%d is smaller than n_tensors=%d", stat_stride, n_tensors);
    RVT_CHECK(n_scalars >= 0 && n_scalars <= RVT_GRADSTAT_MAX_SCALARS, "grad_stats: n_scalars=%d is outside 0..%d", n_scalars,
              (int)RVT_GRADSTAT_MAX_SCALARS);
    RVT_CHECK(n_scalars == 0 || scalars, "grad_stats: %d scalars but no pointer array", n_scalars);
    RVT_CHECK(max_blocks >= 0, "grad_stats: max_blocks=%d is negative", max_blocks);
    RVT_CHECK(ws_bytes >= rvt_grad_stats_ws_bytes(n_chunks), "grad_stats: workspace of %zu bytes, %zu needed", ws_bytes,
              rvt_grad_stats_ws_bytes(n_chunks));
    RVT_CHECK((((uintptr_t)chunks | (uintptr_t)step | (uintptr_t)stats | (uintptr_t)heads | (uintptr_t)verdict | (uintptr_t)ws) & 7) == 0,
              "grad_stats: table, step count, ring, verdict and workspace must be 8-byte aligned");
    RVT_CHECK(((uintptr_t)tensor_first & 3) == 0, "grad_stats: tensor_first must be 4-byte aligned");
    GradScalarPtrs sp = {};
    for (int i = 0; i < n_scalars; i++) {
        RVT_CHECK(scalars[i] && ((uintptr_t)scalars[i] & 3) == 0, "grad_stats: scalar %d is null or not 4-byte aligned", i);
        sp.p[i] = scalars[i];
    }
    const int cap = max_blocks > 0 ? imin(max_blocks, OPTIM_MAX_GRID) : OPTIM_MAX_GRID;
    hipStream_t st = (hipStream_t)stream;
    RvtGradStat* partial = static_cast<RvtGradStat*>(ws);
    hipLaunchKernelGGL(gradstats_partial_kernel, dim3((unsigned)imin(n_chunks, cap)), dim3(GRADSTAT_THREADS), 0, st,
                       static_cast<const OptimChunk*>(chunks), n_chunks, partial);
    RVT_TRY(check_launch("grad_stats (partial)"));
    hipLaunchKernelGGL(gradstats_fold_kernel, dim3(1), dim3(GRADSTAT_FOLD_THREADS), 0, st, (const RvtGradStat*)partial, tensor_first,
                       n_tensors, n_chunks, step, sp, n_scalars, stats, stat_stride, heads, ring, verdict);
    return check_launch("grad_stats (fold)");
}

}  // extern "C"
