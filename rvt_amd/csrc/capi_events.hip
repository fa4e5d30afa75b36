// extern "C" entry points, part 15: raw event streams -> a whole sequence of stacked-histogram or mixed-density-stack windows,
// slicing and half-scale down-sampling on the device (evseq.hpp; reference scripts/genx/preprocess_dataset.py:480-534 and
// data/utils/representations.py:130-218).  Compiled without fused multiply-add contraction and without fast-math (Makefile): the
// bin rules are one correctly rounded fp32 division and one product (histogram) or that division's exponent (mixed density).
// Also what comes before the stream (evprep.hpp): the decode of packed Prophesee records and the reader's timestamp repair.
#include <stdint.h>

#include "host.hpp"
#include "evseq.hpp"
#include "evprep.hpp"

using namespace rvt;

static_assert(sizeof(EvStream) == 48 && sizeof(EvStream) == sizeof(RvtEventStream), "stream table row is 48 bytes (include/rvt_hip.h)");

// planes of one window: polarity x bins for the stacked histogram, bins for the mixed-density stack
static size_t evseq_planes(int bins, int rep) { return (size_t)(rep == EVSEQ_MIXED ? 1 : 2) * bins; }

// cells of one scratch image, rounded up so that every image starts 64-byte aligned
static size_t evseq_slot_cells(int bins, int H, int W, int ds, int rep) {
    const size_t cells = evseq_planes(bins, rep) * (ds ? H / 2 : H) * (ds ? W / 2 : W);
    return (cells + 15) & ~(size_t)15;
}

template <int REP>
static void evseq_launch_count(dim3 grid, hipStream_t st, int coord_bytes, const EvStream* table, const long long* bounds, int g0, int B,
                               int T, int bins, int H, int W, int ds, size_t slot, unsigned* ws) {
    if (coord_bytes == 2)
        hipLaunchKernelGGL((evseq_count_kernel<short, REP>), grid, dim3(EVSEQ_THREADS), 0, st, table, bounds, g0, B, T, bins, H, W, ds, slot, ws);
    else if (coord_bytes == 4)
        hipLaunchKernelGGL((evseq_count_kernel<int, REP>), grid, dim3(EVSEQ_THREADS), 0, st, table, bounds, g0, B, T, bins, H, W, ds, slot, ws);
    else
        hipLaunchKernelGGL((evseq_count_kernel<long long, REP>), grid, dim3(EVSEQ_THREADS), 0, st, table, bounds, g0, B, T, bins, H, W, ds,
                           slot, ws);
}

// what the two sequence entries share: the argument checks (the cutoff is the entry's own), one bounds launch, then the windows in
// chunks of windows_in_flight with one count and one narrowing launch each
static int evseq_run(const char* what, int rep, const RvtEventStream* streams, int B, int T, int coord_bytes, long long window_us,
                     long long window_events, int bins, int H, int W, int downsample_by_2, int count_cutoff, int fastmode, long long* bounds,
                     void* scratch, int windows_in_flight, int count_blocks, void* out, void* stream) {
    RVT_CHECK(streams && bounds && scratch && out, "%s: null argument", what);
    RVT_CHECK(B >= 1 && T >= 1 && (long long)B * T <= (1 << 24), "%s: B=%d T=%d out of range", what, B, T);
    RVT_CHECK(coord_bytes == 2 || coord_bytes == 4 || coord_bytes == 8, "%s: coord_bytes=%d is not 2, 4 or 8", what, coord_bytes);
    RVT_CHECK((window_us > 0) != (window_events > 0) && window_us >= 0 && window_events >= 0,
              "%s: exactly one of window_us=%lld and window_events=%lld must be positive", what, window_us, window_events);
    RVT_CHECK(bins >= 1 && H >= 1 && W >= 1, "%s: bad geometry bins=%d H=%d W=%d", what, bins, H, W);
    RVT_CHECK(!downsample_by_2 || (H >= 2 && W >= 2), "%s: downsample_by_2 needs H=%d and W=%d >= 2", what, H, W);
    RVT_CHECK(windows_in_flight >= 1 && windows_in_flight <= 65535, "%s: windows_in_flight=%d outside 1..65535", what, windows_in_flight);
    RVT_CHECK(count_blocks >= 0 && count_blocks <= 65535, "%s: count_blocks=%d outside 0..65535", what, count_blocks);
    RVT_CHECK(((uintptr_t)streams & 7) == 0 && ((uintptr_t)bounds & 7) == 0 && ((uintptr_t)scratch & 15) == 0,
              "%s: streams / bounds must be 8-byte and scratch 16-byte aligned", what);
    const int ds = downsample_by_2 ? 1 : 0;
    const size_t plane = (size_t)(ds ? H / 2 : H) * (ds ? W / 2 : W);
    const size_t cells = evseq_planes(bins, rep) * plane;
    const size_t slot = evseq_slot_cells(bins, H, W, ds, rep);
    hipStream_t st = (hipStream_t)stream;
    // (EvStream adds nothing to RvtEventStream - same size, asserted above - and exists only for the kernels' symbol names: the downcast
    //  re-labels device memory that the host never dereferences)
    const EvStream* table = static_cast<const EvStream*>(streams);
    const int windows = B * T;

    hipLaunchKernelGGL(evseq_bounds_kernel, dim3((windows + EVSEQ_THREADS - 1) / EVSEQ_THREADS), dim3(EVSEQ_THREADS), 0, st, table, B, T,
                       window_us, window_events, bounds);
    const size_t nvec = (rep == EVSEQ_MIXED ? plane : cells) / 16;            // lanes of a narrowing launch: 16 cells / 16 pixels each
    const int fin_blocks = (int)(nvec / EVSEQ_THREADS < 1 ? 1 : (nvec / EVSEQ_THREADS > 1024 ? 1024 : nvec / EVSEQ_THREADS));
    for (int g0 = 0; g0 < windows; g0 += windows_in_flight) {
        const int nw = imin(windows_in_flight, windows - g0);
        // the bounds are on the device: a fixed number of workgroups per window, about 2048 over the chunk unless the caller knows better
        const int cb = count_blocks > 0 ? count_blocks : imax(8, imin(256, 2048 / nw));
        const dim3 cgrid((unsigned)cb, (unsigned)nw), fgrid((unsigned)fin_blocks, (unsigned)nw);
        unsigned* ws = (unsigned*)scratch;
        if (rep == EVSEQ_MIXED) {
            evseq_launch_count<EVSEQ_MIXED>(cgrid, st, coord_bytes, table, (const long long*)bounds, g0, B, T, bins, H, W, ds, slot, ws);
            hipLaunchKernelGGL(evseq_md_finalize_kernel, fgrid, dim3(EVSEQ_THREADS), 0, st, ws, (signed char*)out, g0, bins, plane, slot,
                               count_cutoff);
        } else {
            evseq_launch_count<EVSEQ_HIST>(cgrid, st, coord_bytes, table, (const long long*)bounds, g0, B, T, bins, H, W, ds, slot, ws);
            hipLaunchKernelGGL(evseq_finalize_kernel, fgrid, dim3(EVSEQ_THREADS), 0, st, ws, (unsigned char*)out, g0, cells, slot, count_cutoff,
                               fastmode);
        }
    }
    return check_launch(what);
}

// workgroups per stream when the caller leaves the choice to the library: about 2048 over the batch
static int evprep_blocks(int B, int blocks_per_stream) {
    return blocks_per_stream > 0 ? blocks_per_stream : imax(8, imin(1024, 2048 / B));
}

static int evprep_check(const char* what, const void* streams, int B, const void* carry, const void* repaired, const void* ws,
                        bool need_ws, int blocks_per_stream) {
    RVT_CHECK(streams && (ws || !need_ws), "%s: null argument", what);
    RVT_CHECK(B >= 1 && B <= 65535, "%s: B=%d outside 1..65535", what, B);
    RVT_CHECK(blocks_per_stream >= 0 && blocks_per_stream <= EVPREP_MAX_BLOCKS, "%s: blocks_per_stream=%d outside 0..%d", what,
              blocks_per_stream, EVPREP_MAX_BLOCKS);
    RVT_CHECK((((uintptr_t)streams | (uintptr_t)carry | (uintptr_t)repaired | (uintptr_t)ws) & 7) == 0,
              "%s: streams, carry, repaired and ws must be 8-byte aligned", what);
    return 0;
}

template <class CT>
static void evprep_launch_decode(dim3 grid, hipStream_t st, EvStream* table, const void* const* records, const long long* n_records,
                                 long long capacity, int repair, long long* carry, long long* repaired, const long long* ws) {
    hipLaunchKernelGGL((evprep_scan_kernel<EVPREP_DECODE, CT>), grid, dim3(EVPREP_THREADS), 0, st, table, records, n_records, capacity, repair,
                       carry, repaired, ws);
}

extern "C" {

size_t rvt_event_prep_ws_bytes(int B, int blocks_per_stream) {
    if (B < 1 || B > 65535 || blocks_per_stream < 0 || blocks_per_stream > EVPREP_MAX_BLOCKS) return 0;
    return (size_t)B * (evprep_blocks(B, blocks_per_stream) + 1) * sizeof(long long);
}

int rvt_event_time_repair(const RvtEventStream* streams, int B, long long* carry, long long* repaired, void* ws, int blocks_per_stream,
                          void* stream) {
    if (evprep_check("event_time_repair", streams, B, carry, repaired, ws, true, blocks_per_stream)) return 1;
    hipStream_t st = (hipStream_t)stream;
    // (the rows are const for the caller: this entry writes the timestamps they point at, never the rows)
    EvStream* table = const_cast<EvStream*>(static_cast<const EvStream*>(streams));
    const dim3 grid((unsigned)evprep_blocks(B, blocks_per_stream), (unsigned)B);
    hipLaunchKernelGGL(evprep_reduce_kernel<EVPREP_REPAIR>, grid, dim3(EVPREP_THREADS), 0, st, (const EvStream*)table,
                       (const void* const*)nullptr, (const long long*)nullptr, 0LL, (const long long*)carry, (long long*)ws);
    hipLaunchKernelGGL((evprep_scan_kernel<EVPREP_REPAIR, short>), grid, dim3(EVPREP_THREADS), 0, st, table, (const void* const*)nullptr,
                       (const long long*)nullptr, 0LL, 1, carry, repaired, (const long long*)ws);
    return check_launch("event_time_repair");
}

int rvt_event_decode_dat(const void* const* records, const long long* n_records, long long capacity, RvtEventStream* streams, int B,
                         int coord_bytes, int repair, long long* carry, long long* repaired, void* ws, int blocks_per_stream, void* stream) {
    if (evprep_check("event_decode_dat", streams, B, carry, repaired, ws, repair != 0, blocks_per_stream)) return 1;
    RVT_CHECK(records && n_records && (((uintptr_t)records | (uintptr_t)n_records) & 7) == 0,
              "event_decode_dat: records / n_records null or not 8-byte aligned");
    RVT_CHECK(capacity >= 0, "event_decode_dat: capacity=%lld is negative", capacity);
    RVT_CHECK(coord_bytes == 2 || coord_bytes == 4 || coord_bytes == 8, "event_decode_dat: coord_bytes=%d is not 2, 4 or 8", coord_bytes);
    hipStream_t st = (hipStream_t)stream;
    EvStream* table = static_cast<EvStream*>(streams);
    const dim3 grid((unsigned)evprep_blocks(B, blocks_per_stream), (unsigned)B);
    if (repair)
        hipLaunchKernelGGL(evprep_reduce_kernel<EVPREP_DECODE>, grid, dim3(EVPREP_THREADS), 0, st, (const EvStream*)table, records, n_records,
                           capacity, (const long long*)carry, (long long*)ws);
    if (coord_bytes == 2) evprep_launch_decode<short>(grid, st, table, records, n_records, capacity, repair ? 1 : 0, carry, repaired, (const long long*)ws);
    else if (coord_bytes == 4) evprep_launch_decode<int>(grid, st, table, records, n_records, capacity, repair ? 1 : 0, carry, repaired, (const long long*)ws);
    else evprep_launch_decode<long long>(grid, st, table, records, n_records, capacity, repair ? 1 : 0, carry, repaired, (const long long*)ws);
    return check_launch("event_decode_dat");
}

size_t rvt_event_sequence_ws_bytes(int bins, int H, int W, int downsample_by_2, int windows_in_flight) {
    if (bins < 1 || H < 1 || W < 1 || windows_in_flight < 1) return 0;
    return evseq_slot_cells(bins, H, W, downsample_by_2, EVSEQ_HIST) * sizeof(unsigned) * (size_t)windows_in_flight;
}

int rvt_event_sequence(const RvtEventStream* streams, int B, int T, int coord_bytes, long long window_us, long long window_events, int bins,
                       int H, int W, int downsample_by_2, int count_cutoff, int fastmode, long long* bounds, void* scratch,
                       int windows_in_flight, int count_blocks, unsigned char* out, void* stream) {
    RVT_CHECK(count_cutoff >= 1 && count_cutoff <= 255, "event_sequence: count_cutoff=%d outside 1..255", count_cutoff);
    return evseq_run("event_sequence", EVSEQ_HIST, streams, B, T, coord_bytes, window_us, window_events, bins, H, W, downsample_by_2,
                     count_cutoff, fastmode, bounds, scratch, windows_in_flight, count_blocks, out, stream);
}

size_t rvt_event_sequence_mixed_ws_bytes(int bins, int H, int W, int downsample_by_2, int windows_in_flight) {
    if (bins < 1 || H < 1 || W < 1 || windows_in_flight < 1) return 0;
    return evseq_slot_cells(bins, H, W, downsample_by_2, EVSEQ_MIXED) * sizeof(int) * (size_t)windows_in_flight;
}

int rvt_event_sequence_mixed(const RvtEventStream* streams, int B, int T, int coord_bytes, long long window_us, long long window_events, int bins,
                             int H, int W, int downsample_by_2, int count_cutoff, long long* bounds, void* scratch,
                             int windows_in_flight, int count_blocks, signed char* out, void* stream) {
    RVT_CHECK(count_cutoff <= 127, "event_sequence_mixed: count_cutoff=%d above 127 (negative = none)", count_cutoff);
    return evseq_run("event_sequence_mixed", EVSEQ_MIXED, streams, B, T, coord_bytes, window_us, window_events, bins, H, W,
                     downsample_by_2, count_cutoff < 0 ? -1 : count_cutoff, 0, bounds, scratch, windows_in_flight, count_blocks, out, stream);
}

int rvt_mixed_density_stack(const long long* x, const long long* y, const long long* pol, const long long* time, size_t n_events,
                            int bins, int H, int W, int count_cutoff, int* scratch, signed char* out, void* stream) {
    RVT_CHECK(scratch && out && (n_events == 0 || (x && y && pol && time)), "mixed_density_stack: null argument");
    RVT_CHECK(bins >= 1 && H >= 1 && W >= 1 && count_cutoff <= 127, "mixed_density_stack: bad geometry bins=%d H=%d W=%d cutoff=%d", bins, H,
              W, count_cutoff);
    RVT_CHECK(((uintptr_t)scratch & 15) == 0, "mixed_density_stack: scratch must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const size_t plane = (size_t)H * W;
    if (n_events > 0)
        hipLaunchKernelGGL(evseq_md_window_kernel, dim3(grid_for(n_events, 4096)), dim3(EVSEQ_THREADS), 0, st, x, y, pol, time, n_events, bins,
                           H, W, (unsigned*)scratch);
    const size_t nvec = plane / 16;
    const int fin_blocks = (int)(nvec / EVSEQ_THREADS < 1 ? 1 : (nvec / EVSEQ_THREADS > 1024 ? 1024 : nvec / EVSEQ_THREADS));
    hipLaunchKernelGGL(evseq_md_finalize_kernel, dim3((unsigned)fin_blocks), dim3(EVSEQ_THREADS), 0, st, (unsigned*)scratch, out, 0, bins,
                       plane, (size_t)0, count_cutoff < 0 ? -1 : count_cutoff);
    return check_launch("mixed_density_stack");
}

}  // extern "C"
