// extern "C" entry points, part 14: the optimizer step (optim.hpp; reference modules/detection.py configure_optimizers and the
// trainer's gradient clipping by value).  Compiled without fused multiply-add contraction (Makefile): every fp32 and fp64 line of
// the update is one rounded operation, as in torch's unfused AdamW and in the scheduler's Python arithmetic.
#include <stdint.h>

#include "host.hpp"
#include "optim.hpp"

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

}  // extern "C"
