// extern "C" entry points, part 15: raw event streams -> a whole sequence of stacked-histogram windows, slicing and half-scale
// down-sampling on the device (evseq.hpp; reference scripts/genx/preprocess_dataset.py:480-534).  Compiled without fused
// multiply-add contraction and without fast-math (Makefile): the bin rule is one correctly rounded fp32 division and one product.
#include <stdint.h>

#include "host.hpp"
#include "evseq.hpp"

using namespace rvt;

static_assert(sizeof(EvStream) == 48, "stream table row is 48 bytes (include/rvt_hip.h)");

// cells of one scratch image, rounded up so that every image starts 64-byte aligned
static size_t evseq_slot_cells(int bins, int H, int W, int ds) {
    const size_t cells = (size_t)2 * bins * (ds ? H / 2 : H) * (ds ? W / 2 : W);
    return (cells + 15) & ~(size_t)15;
}

extern "C" {

size_t rvt_event_sequence_ws_bytes(int bins, int H, int W, int downsample_by_2, int windows_in_flight) {
    if (bins < 1 || H < 1 || W < 1 || windows_in_flight < 1) return 0;
    return evseq_slot_cells(bins, H, W, downsample_by_2) * sizeof(unsigned) * (size_t)windows_in_flight;
}

int rvt_event_sequence(const void* streams, int B, int T, int coord_bytes, long long window_us, long long window_events, int bins,
                       int H, int W, int downsample_by_2, int count_cutoff, int fastmode, long long* bounds, void* scratch,
                       int windows_in_flight, int count_blocks, unsigned char* out, void* stream) {
    RVT_CHECK(streams && bounds && scratch && out, "event_sequence: null argument");
    RVT_CHECK(B >= 1 && T >= 1 && (long long)B * T <= (1 << 24), "event_sequence: B=%d T=%d out of range", B, T);
    RVT_CHECK(coord_bytes == 2 || coord_bytes == 4 || coord_bytes == 8, "event_sequence: coord_bytes=%d is not 2, 4 or 8", coord_bytes);
    RVT_CHECK((window_us > 0) != (window_events > 0) && window_us >= 0 && window_events >= 0,
              "event_sequence: exactly one of window_us=%lld and window_events=%lld must be positive", window_us, window_events);
    RVT_CHECK(bins >= 1 && H >= 1 && W >= 1 && count_cutoff >= 1 && count_cutoff <= 255,
              "event_sequence: bad geometry bins=%d H=%d W=%d cutoff=%d", bins, H, W, count_cutoff);
    RVT_CHECK(!downsample_by_2 || (H >= 2 && W >= 2), "event_sequence: downsample_by_2 needs H=%d and W=%d >= 2", H, W);
    RVT_CHECK(windows_in_flight >= 1 && windows_in_flight <= 65535, "event_sequence: windows_in_flight=%d outside 1..65535", windows_in_flight);
    RVT_CHECK(count_blocks >= 0 && count_blocks <= 65535, "event_sequence: count_blocks=%d outside 0..65535", count_blocks);
    RVT_CHECK(((uintptr_t)streams & 7) == 0 && ((uintptr_t)bounds & 7) == 0 && ((uintptr_t)scratch & 15) == 0,
              "event_sequence: streams / bounds must be 8-byte and scratch 16-byte aligned");
    const int ds = downsample_by_2 ? 1 : 0;
    const size_t cells = (size_t)2 * bins * (ds ? H / 2 : H) * (ds ? W / 2 : W);
    const size_t slot = evseq_slot_cells(bins, H, W, ds);
    hipStream_t st = (hipStream_t)stream;
    const EvStream* table = (const EvStream*)streams;
    const int windows = B * T;

    hipLaunchKernelGGL(evseq_bounds_kernel, dim3((windows + EVSEQ_THREADS - 1) / EVSEQ_THREADS), dim3(EVSEQ_THREADS), 0, st, table, B, T,
                       window_us, window_events, bounds);
    const size_t nvec = cells / 16;
    const int fin_blocks = (int)(nvec / EVSEQ_THREADS < 1 ? 1 : (nvec / EVSEQ_THREADS > 1024 ? 1024 : nvec / EVSEQ_THREADS));
    for (int g0 = 0; g0 < windows; g0 += windows_in_flight) {
        const int nw = imin(windows_in_flight, windows - g0);
        // the bounds are on the device: a fixed number of workgroups per window, about 2048 over the chunk unless the caller knows better
        const int cb = count_blocks > 0 ? count_blocks : imax(8, imin(256, 2048 / nw));
        const dim3 cgrid((unsigned)cb, (unsigned)nw), fgrid((unsigned)fin_blocks, (unsigned)nw);
        unsigned* ws = (unsigned*)scratch;
        if (coord_bytes == 2)
            hipLaunchKernelGGL((evseq_count_kernel<short>), cgrid, dim3(EVSEQ_THREADS), 0, st, table, (const long long*)bounds, g0, B, T, bins,
                               H, W, ds, slot, ws);
        else if (coord_bytes == 4)
            hipLaunchKernelGGL((evseq_count_kernel<int>), cgrid, dim3(EVSEQ_THREADS), 0, st, table, (const long long*)bounds, g0, B, T, bins,
                               H, W, ds, slot, ws);
        else
            hipLaunchKernelGGL((evseq_count_kernel<long long>), cgrid, dim3(EVSEQ_THREADS), 0, st, table, (const long long*)bounds, g0, B, T,
                               bins, H, W, ds, slot, ws);
        hipLaunchKernelGGL(evseq_finalize_kernel, fgrid, dim3(EVSEQ_THREADS), 0, st, ws, out, g0, cells, slot, count_cutoff, fastmode);
    }
    return check_launch("event_sequence");
}

}  // extern "C"
