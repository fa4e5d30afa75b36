// extern "C" entry points, part 16: the sparse frame cache (framecache.hpp): byte planes packed to bitmap + non-zero bytes on the
// device and unpacked by frame index, plain or through the training augmentation (frames_augment.hpp), and gathered by address
// out of several packed stores, pinned host memory included (frames_gather.hpp).  Integer work: bit-exact.
#include <stdint.h>

#include "host.hpp"
#include "framecache.hpp"
#include "frames_augment.hpp"
#include "frames_gather.hpp"

using namespace rvt;

namespace {
struct FrameGeom { long long Gf, Sf; };
static inline FrameGeom frame_geom(long long E) {
    const long long Gf = (E + FC_GROUP - 1) / FC_GROUP;
    return FrameGeom{Gf, (Gf + 63) / 64};
}
static inline bool frames_shape_ok(long long F, long long E) { return F >= 1 && F <= 0x7fffffffLL && E >= 1 && E < (1LL << 31); }
// one wave per segment, FC_WAVES of them per workgroup
static inline bool frames_grid(long long waves, dim3& grid) {
    const long long blocks = (waves + FC_WAVES - 1) / FC_WAVES;
    if (blocks > 0x7fffffffLL) return false;
    grid = dim3((unsigned)blocks);
    return true;
}
// the argument checks rvt_frames_unpack and rvt_frames_unpack_augment share; who: the entry point's name in the messages, table:
// rvt_frames_unpack_augment's (has_table), checked like the other arrays
static int frames_unpack_checks(const char* who, const void* masks, const void* seg_offset, const void* value_base, const void* values,
                                long long values_len, long long F, long long E, const long long* index, long long Fout, const void* out,
                                const void* status, bool has_table, const void* table) {
    RVT_CHECK(masks && seg_offset && value_base && out && status && (table || !has_table), "%s: null argument", who);
    RVT_CHECK(frames_shape_ok(F, E) && Fout >= 1, "%s: F=%lld, Fout=%lld frames of E=%lld bytes outside the supported range", who, F, Fout, E);
    RVT_CHECK(values_len >= 0 && (values || values_len == 0), "%s: values_len=%lld without a values array", who, values_len);
    RVT_CHECK(index || Fout <= F, "%s: without an index Fout=%lld must not exceed F=%lld", who, Fout, F);
    RVT_CHECK(((uintptr_t)masks & 7) == 0 && ((uintptr_t)value_base & 7) == 0 && ((uintptr_t)index & 7) == 0 &&
              ((uintptr_t)seg_offset & 3) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)table & 3) == 0,
              "%s: masks / value_base / index need 8-byte, seg_offset / status%s 4-byte alignment", who, has_table ? " / table" : "");
    return 0;
}
}  // namespace

extern "C" {

size_t rvt_frames_pack_ws_bytes(long long F, long long E) {
    if (!frames_shape_ok(F, E)) return 0;
    const FrameGeom g = frame_geom(E);
    return (((size_t)F * (size_t)g.Sf + (size_t)F) * 4 + 15) & ~(size_t)15;   // the segments' counts, then the frames'
}

int rvt_frames_pack(const void* frames, long long F, long long E, void* masks, void* seg_offset, void* value_base, void* values,
                    long long capacity, void* status, void* ws, size_t ws_bytes, void* stream) {
    RVT_CHECK(frames && masks && seg_offset && value_base && status && ws, "frames_pack: null argument");
    RVT_CHECK(frames_shape_ok(F, E), "frames_pack: F=%lld frames of E=%lld bytes outside the supported range (F >= 1, 1 <= E < 2^31)", F, E);
    RVT_CHECK(capacity >= 0 && (values || capacity == 0), "frames_pack: capacity=%lld without a values array", capacity);
    RVT_CHECK(ws_bytes >= rvt_frames_pack_ws_bytes(F, E), "frames_pack: workspace of %zu bytes, rvt_frames_pack_ws_bytes says %zu", ws_bytes,
              rvt_frames_pack_ws_bytes(F, E));
    RVT_CHECK(((uintptr_t)masks & 7) == 0 && ((uintptr_t)value_base & 7) == 0 && ((uintptr_t)seg_offset & 3) == 0 &&
              ((uintptr_t)status & 3) == 0 && ((uintptr_t)ws & 3) == 0, "frames_pack: masks / value_base need 8-byte, seg_offset / status / ws 4-byte alignment");
    const FrameGeom g = frame_geom(E);
    dim3 grid;
    RVT_CHECK(frames_grid(F * g.Sf, grid), "frames_pack: F=%lld frames of %lld segments exceed the grid", F, g.Sf);
    unsigned* seg_count = (unsigned*)ws;
    unsigned* frame_count = seg_count + (size_t)F * (size_t)g.Sf;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frames_mask_kernel, grid, dim3(FC_THREADS), 0, st, (const unsigned char*)frames, F, E, g.Gf, g.Sf,
                       (unsigned long long*)masks, seg_count);
    hipLaunchKernelGGL(frames_seg_scan_kernel, dim3((unsigned)F), dim3(FC_THREADS), 0, st, (const unsigned*)seg_count, g.Sf,
                       (unsigned*)seg_offset, frame_count);
    hipLaunchKernelGGL(frames_base_scan_kernel, dim3(1), dim3(FC_THREADS), 0, st, (const unsigned*)frame_count, F, capacity,
                       (long long*)value_base, (int*)status);
    if (capacity > 0)
        hipLaunchKernelGGL(frames_compact_kernel, grid, dim3(FC_THREADS), 0, st, (const unsigned char*)frames, F, E, g.Sf,
                           (const unsigned*)seg_offset, (const long long*)value_base, (unsigned char*)values, capacity);
    return check_launch("frames_pack");
}

int rvt_frames_unpack(const void* masks, const void* seg_offset, const void* value_base, const void* values, long long values_len,
                      long long F, long long E, const long long* index, long long Fout, void* out, void* status, void* stream) {
    RVT_TRY(frames_unpack_checks("frames_unpack", masks, seg_offset, value_base, values, values_len, F, E, index, Fout, out, status, false, nullptr));
    const FrameGeom g = frame_geom(E);
    dim3 grid;
    RVT_CHECK(Fout <= 0x7fffffffLL && frames_grid(Fout * g.Sf, grid), "frames_unpack: Fout=%lld frames of %lld segments exceed the grid", Fout, g.Sf);
    hipLaunchKernelGGL(frames_unpack_kernel, grid, dim3(FC_THREADS), 0, (hipStream_t)stream, (const unsigned long long*)masks,
                       (const unsigned*)seg_offset, (const long long*)value_base, (const unsigned char*)values, values_len, F, E, g.Gf, g.Sf,
                       index, Fout, (unsigned char*)out, (int*)status);
    return check_launch("frames_unpack");
}

int rvt_frames_unpack_augment(const void* masks, const void* seg_offset, const void* value_base, const void* values, long long values_len,
                              long long F, long long E, const long long* index, long long Fout, const int* table, int B, int C, int H, int W,
                              void* out, void* status, void* stream) {
    RVT_TRY(frames_unpack_checks("frames_unpack_augment", masks, seg_offset, value_base, values, values_len, F, E, index, Fout, out, status, true, table));
    RVT_CHECK(B >= 1 && C >= 1 && H >= 1 && W >= 1, "frames_unpack_augment: B=%d C=%d H=%d W=%d must be positive", B, C, H, W);
    RVT_CHECK(W <= AUG_MAX_W, "frames_unpack_augment: W=%d outside the supported range 1..%d", W, AUG_MAX_W);
    RVT_CHECK((long long)C * H <= (1 << 24), "frames_unpack_augment: C*H=%lld rows per frame outside the supported range", (long long)C * H);
    RVT_CHECK((long long)C * H * W == E, "frames_unpack_augment: a frame of E=%lld bytes is not C*H*W = %d*%d*%d", E, C, H, W);
    const FrameGeom g = frame_geom(E);
    const int chunks = (C * H + AUG_CHUNK - 1) / AUG_CHUNK;
    RVT_CHECK(Fout * chunks <= 0x7fffffffLL, "frames_unpack_augment: Fout=%lld frames of %d rows exceed the grid", Fout, C * H);
    const bool vec = W % 16 == 0 && (uintptr_t)out % 16 == 0;
    hipLaunchKernelGGL(vec ? frames_unpack_augment_kernel<true> : frames_unpack_augment_kernel<false>, dim3((unsigned)(Fout * chunks)),
                       dim3(AUG_THREADS), 0, (hipStream_t)stream, (const unsigned long long*)masks, (const unsigned*)seg_offset,
                       (const long long*)value_base, (const unsigned char*)values, values_len, F, E, g.Gf, g.Sf, index, table, B, C, H, W,
                       chunks, (unsigned char*)out, (int*)status);
    return check_launch("frames_unpack_augment");
}

int rvt_frames_gather(const long long* table, long long n, long long E, void* masks, void* seg_offset, void* value_base, void* values,
                      long long capacity, void* status, int max_blocks, void* stream) {
    RVT_CHECK(n >= 0 && n <= 0x7fffffffLL && E >= 1 && E < (1LL << 31), "frames_gather: n=%lld frames of E=%lld bytes outside the supported range (n >= 0, 1 <= E < 2^31)", n, E);
    if (n == 0) return 0;
    RVT_CHECK(table && masks && seg_offset && value_base && status, "frames_gather: null argument");
    RVT_CHECK(capacity >= 0 && (values || capacity == 0), "frames_gather: capacity=%lld without a values array", capacity);
    RVT_CHECK(max_blocks >= 0, "frames_gather: max_blocks=%d is negative (0 = the default)", max_blocks);
    RVT_CHECK(((uintptr_t)table & 7) == 0 && ((uintptr_t)masks & 7) == 0 && ((uintptr_t)value_base & 7) == 0 &&
              ((uintptr_t)seg_offset & 3) == 0 && ((uintptr_t)status & 3) == 0,
              "frames_gather: table / masks / value_base need 8-byte, seg_offset / status 4-byte alignment");
    const FrameGeom g = frame_geom(E);
    // pieces of the copy: masks and seg_offset of every frame, and the value bytes the destination has room for
    const long long MU = (g.Gf * 8 + GA_PIECE - 1) / GA_PIECE, SU = ((g.Sf + 1) * 4 + GA_PIECE - 1) / GA_PIECE;
    const long long room = capacity < n * E ? capacity : n * E;
    const long long units = n * (MU + SU) + (room > 0 ? (15 + room + GA_PIECE - 1) / GA_PIECE : 0);
    long long blocks = (units + FC_WAVES - 1) / FC_WAVES;
    const long long cap_blocks = max_blocks > 0 ? max_blocks : GA_DEFAULT_BLOCKS;
    if (blocks > cap_blocks) blocks = cap_blocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(frames_gather_scan_kernel, dim3(1), dim3(FC_THREADS), 0, st, table, n, E, capacity, (long long*)value_base,
                       (int*)status);
    hipLaunchKernelGGL(frames_gather_copy_kernel, dim3((unsigned)blocks), dim3(FC_THREADS), 0, st, table, n, E, g.Gf, g.Sf,
                       (unsigned long long*)masks, (unsigned*)seg_offset, (const long long*)value_base, (unsigned char*)values, capacity);
    return check_launch("frames_gather");
}

}  // extern "C"
