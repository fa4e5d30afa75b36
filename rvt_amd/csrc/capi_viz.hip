// extern "C" entry points, part 17: detection previews (include/rvt_hip.h: rvt_render_preview; host mirror rvt_amd/viz.py).  The device
// counterpart of the reference's detection visualisation callback (callbacks/viz_base.py:164-174 ev_repr_to_img, callbacks/detection.py:
// 52-62, utils/evaluation/prophesee/visualize/vis_utils.py:88-106): event planes to a grey / white / black image, the boxes of up to
// two lists drawn into one copy each, the copies stacked.  Integer work: bit-exact.  The kernel lives in this part (the include-graph
// test of the kernel headers lists every .hpp of this directory by name).
//
// One launch.  A workgroup takes a chunk of consecutive base rows of one output image; a lane owns 16 consecutive base pixels of a
// row (a "piece"), so a chunk holds about 256 pieces.
//   boxes   every thread prepares box j of a panel (integer corners, tag row, colour, text word), keeps it when its outline or tag
//           touches the chunk's rows and the image's columns, and an order-preserving workgroup scan compacts the kept records into
//           LDS (6 ints each, at most 512 per panel: 24 KiB, six workgroups to a CU).  A chunk that no box touches runs an empty loop.
//   planes  one 16-byte load per channel (VEC) or up to 16 byte loads (any other shape or alignment); four bytes of a dword are summed
//           as two 16-bit lanes of two accumulators (C / 2 * 255 < 2^16 for C <= 512), int8 planes biased by 128 on both sides of the
//           difference.  The planes of a frame are read once for all panels.
//   pixels  16 packed 0x00BBGGRR registers per lane; the records are walked in row order (all lanes read the same LDS address) and a
//           record that touches the lane's row and columns paints a 16-bit mask of them: painter's order, later covers earlier.  Tag
//           ink is a 16-bit mask put together from the 5-bit glyph rows of the at most four characters under the piece.
//   stores  the 48 * s bytes of the piece per replicated row as 3 * s 16-byte stores (VEC) or byte stores; each output byte is written
//           exactly once, nothing is read back.
// status is or-ed by a plain load and store of one thread per offending image: every writer stores the old value with bit 0 set,
// so no atomic is needed.
#include <stdint.h>

#include "host.hpp"

using namespace rvt;

namespace {

constexpr int VZ_THREADS = 256, VZ_WAVES = VZ_THREADS / 64;
constexpr int VZ_MAX_BOXES = RVT_VIZ_MAX_BOXES;
constexpr int VZ_PIECES = 256;                    // pieces of a chunk, about: rows per chunk = VZ_PIECES / pieces per row
constexpr int VZ_MAX_ROWS = 64;
constexpr int VZ_NAME = RVT_VIZ_NAME_BYTES, VZ_GLYPH_ROWS = RVT_VIZ_GLYPH_ROWS;
constexpr int VZ_HAS_SCORE = 1 << 11, VZ_HAS_TAG = 1 << 12;   // text word: name length | q << 4 | these | name index << 16
constexpr int VZ_REC = 6;                         // ints of a record: x0 y0 x1 y1, colour | VZ_TAG_BELOW, text word
constexpr int VZ_TAG_BELOW = 1 << 24;             // the tag's top row is y0 + 1 (pushed inside), not y0 - 9
constexpr int VZ_MAX_NAMES = 4096, VZ_MAX_C = 512, VZ_MAX_HW = 1 << 20;

struct VizPanel { const float* rows; const int* count; int N, kind; };
struct VizTables { const unsigned char *palette, *names, *glyphs; int n_palette, n_names; };

__device__ __forceinline__ int vz_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int vz_max(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ float vz_float(unsigned bits) { return __builtin_bit_cast(float, bits); }
__device__ __forceinline__ unsigned vz_bits(float v) { return __builtin_bit_cast(unsigned, v); }
// not finite, or of magnitude >= 2^20: on the bits, so that no float comparison ever sees a NaN
__device__ __forceinline__ bool vz_bad(unsigned bits) { return (bits & 0x7fffffffu) >= 0x49800000u; }
__device__ __forceinline__ bool vz_nonfinite(unsigned bits) { return (bits & 0x7fffffffu) >= 0x7f800000u; }
// bits lo .. hi (0 <= lo <= hi <= 15) / bit k when it is one of the piece's 16
__device__ __forceinline__ unsigned vz_span(int lo, int hi) { return ((2u << hi) - 1u) & ~((1u << lo) - 1u); }
__device__ __forceinline__ unsigned vz_bit(int k) { return (unsigned)k < 16u ? 1u << k : 0u; }

// exclusive sum over the workgroup of one tile of a longer sequence: what lies in front of this thread's value; `run` = the total of
// the tiles in front, advanced by this tile's.  part: LDS, one row per parity of the tile number.  Every thread calls it.
__device__ __forceinline__ int vz_block_scan(int v, int& run, int (*part)[VZ_WAVES], int par) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl(inc, (lane - d) & 63);
        if (lane >= d) inc += up;
    }
    if (lane == 63) part[par][wave] = inc;
    __syncthreads();
    int pre = run + inc - v;
#pragma unroll
    for (int q = 0; q < VZ_WAVES; q++) {
        const int t = part[par][q];
        if (q < wave) pre += t;
        run += t;
    }
    return pre;
}

// One row of a box list -> its record; returns whether the box is drawn at all and touches the base rows [ra, rb) of a W-wide image.
__device__ __forceinline__ bool vz_prepare(const float* __restrict__ row, int kind, const VizTables& tb, int flags, int W, int ra, int rb,
                                           int (&r)[VZ_REC]) {
    const unsigned* __restrict__ u = reinterpret_cast<const unsigned*>(row);
    float x, y, w, h;
    unsigned bc, bs = 0;
    if (kind == RVT_VIZ_KIND_DET) {                   // x1 y1 x2 y2 obj class_conf class
        const unsigned b0 = u[0], b1 = u[1], b2 = u[2], b3 = u[3];
        if (vz_nonfinite(b0) || vz_nonfinite(b1) || vz_nonfinite(b2) || vz_nonfinite(b3)) return false;   // (w or h would not be finite)
        x = vz_float(b0); y = vz_float(b1);
        w = vz_float(b2) - x; h = vz_float(b3) - y;
        bs = u[5]; bc = u[6];
    } else {                                          // t x y w h class_id conf
        const unsigned b1 = u[1], b2 = u[2], b3 = u[3], b4 = u[4];
        if (vz_bad(b1) || vz_bad(b2) || vz_bad(b3) || vz_bad(b4)) return false;
        x = vz_float(b1); y = vz_float(b2); w = vz_float(b3); h = vz_float(b4);
        bc = u[5];
    }
    if (vz_bad(vz_bits(x)) || vz_bad(vz_bits(y)) || vz_bad(vz_bits(w)) || vz_bad(vz_bits(h)) || vz_bad(bc)) return false;
    const float c = vz_float(bc);
    if (w < 0.f || h < 0.f || c < 0.f) return false;
    const int x0 = (int)x, y0 = (int)y, x1 = x0 + (int)w, y1 = y0 + (int)h, cls = (int)c;
    const unsigned char* __restrict__ pc = tb.palette + 3 * (cls % tb.n_palette);
    const int color = (int)pc[0] | ((int)pc[1] << 8) | ((int)pc[2] << 16);
    int txt = 0, ty = 0, xe = x0 - 1;                 // xe: the tag's last column
    if (flags & RVT_VIZ_TEXT) {
        const int ni = cls % tb.n_names;
        const unsigned char* __restrict__ nm = tb.names + VZ_NAME * ni;
        int len = 0;
        while (len < VZ_NAME && nm[len]) len++;
        int q = 0, nch = len;
        txt = VZ_HAS_TAG | (ni << 16);
        if (kind == RVT_VIZ_KIND_DET) {
            if (vz_nonfinite(bs)) {
                q = bs == 0x7f800000u ? 100 : 0;      // +inf prints 1.00, -inf and NaN 0.00
            } else {
                const float t = vz_float(bs) * 100.0f + 0.5f;
                q = t >= 100.f ? 100 : (t <= 0.f ? 0 : (int)t);
            }
            txt |= VZ_HAS_SCORE;
            nch += 5;
        }
        txt |= len | (q << 4);
        ty = y0 - 9 >= 0 ? y0 - 9 : y0 + 1;
        xe = x0 + 6 * nch;
    }
    r[0] = x0; r[1] = y0; r[2] = x1; r[3] = y1; r[4] = color | (ty > y0 ? VZ_TAG_BELOW : 0); r[5] = txt;
    const bool outline = y1 >= ra && y0 < rb && x1 >= 0 && x0 < W;
    const bool tag = (txt & VZ_HAS_TAG) && ty + 8 >= ra && ty < rb && xe >= 0 && x0 < W;
    return outline || tag;
}

// character ci of a tag: the name, then for a detection ' ', the score as d.dd
__device__ __forceinline__ int vz_char(const VizTables& tb, int txt, int ci) {
    const int len = txt & 15, q = (txt >> 4) & 127;
    if (ci < len) return tb.names[VZ_NAME * (txt >> 16) + ci];
    switch (ci - len) {
        case 0: return ' ';
        case 1: return '0' + q / 100;
        case 2: return '.';
        case 3: return '0' + (q / 10) % 10;
        default: return '0' + q % 10;
    }
}

template <bool VEC>
__device__ __forceinline__ u32x4 vz_load(const unsigned char* __restrict__ p, int nv) {
    if constexpr (VEC) {
        return *reinterpret_cast<const u32x4*>(p);
    } else {
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nv) v[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
        return v;
    }
}
// the first min(nbytes, 16) bytes of the line (VEC: all 16, one store)
template <bool VEC>
__device__ __forceinline__ void vz_store(unsigned char* __restrict__ p, const u32x4& v, int nbytes) {
    if constexpr (VEC) {
        *reinterpret_cast<u32x4*>(p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k < nbytes) p[k] = (unsigned char)((v[k >> 2] >> (8 * (k & 3))) & 0xffu);
    }
}

__device__ __forceinline__ void vz_paint(unsigned (&pix)[16], unsigned mask, unsigned color) {
#pragma unroll
    for (int k = 0; k < 16; k++) pix[k] = (mask >> k) & 1u ? color : pix[k];
}

// sums of one half of the channels: acc_e holds pixels 0 and 2, acc_o pixels 1 and 3 of each dword as 16-bit lanes
template <bool VEC>
__device__ __forceinline__ void vz_sum(const unsigned char* __restrict__ src, size_t HW, int c0, int c1, unsigned bias, int nv,
                                       unsigned (&acc_e)[4], unsigned (&acc_o)[4]) {
#pragma unroll 4
    for (int c = c0; c < c1; c++) {
        const u32x4 v = vz_load<VEC>(src + (size_t)c * HW, nv);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned wv = v[k] ^ bias;
            acc_e[k] += wv & 0x00ff00ffu;
            acc_o[k] += (wv >> 8) & 0x00ff00ffu;
        }
    }
}

template <bool VEC, int S>
__global__ void __launch_bounds__(VZ_THREADS)
viz_render_kernel(const unsigned char* __restrict__ planes, int planes_signed, long long F, int C, int H, int W, VizPanel p0, VizPanel p1,
                  int P, const long long* __restrict__ frame_index, VizTables tb, int flags, int chunk_rows, int chunks,
                  unsigned char* __restrict__ out, int* __restrict__ status) {
    __shared__ __attribute__((aligned(16))) int rec[2][VZ_MAX_BOXES][VZ_REC];
    __shared__ int part[2][VZ_WAVES];
    const int tid = threadIdx.x;
    const long long i = (long long)(blockIdx.x / (unsigned)chunks);
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const int ra = chunk * chunk_rows, rb = vz_min(H, ra + chunk_rows);
    const long long f = frame_index ? frame_index[i] : i;
    const bool present = f >= 0 && f < F;
    if (!present && f != -1 && chunk == 0 && tid == 0) *status = *status | RVT_VIZ_STATUS_INDEX;

    // ---- the boxes that touch this chunk, in row order, into LDS
    int n0 = 0, n1 = 0, par = 0;
    for (int p = 0; p < P; p++) {
        const VizPanel& pn = p ? p1 : p0;
        int n = 0;
        if (present && pn.rows) n = vz_max(0, vz_min(pn.count[f], vz_min(pn.N, VZ_MAX_BOXES)));
        int run = 0;
        for (int base = 0; base < n; base += VZ_THREADS, par ^= 1) {
            const int j = base + tid;
            int r[VZ_REC];
            bool alive = false;
            if (j < n) alive = vz_prepare(pn.rows + ((size_t)f * pn.N + j) * 7, pn.kind, tb, flags, W, ra, rb, r);
            const int pos = vz_block_scan(alive ? 1 : 0, run, part, par);
            if (alive) {
#pragma unroll
                for (int k = 0; k < VZ_REC; k++) rec[p][pos][k] = r[k];
            }
        }
        if (p) n1 = run; else n0 = run;
    }
    __syncthreads();

    // ---- the pieces of the chunk
    const int pieces = (W + 15) >> 4, units = (rb - ra) * pieces;
    const size_t HW = (size_t)H * W, Ws3 = (size_t)W * S * 3;
    const unsigned bias = planes_signed ? 0x80808080u : 0u;
    for (int un = tid; un < units; un += VZ_THREADS) {
        const int row = un / pieces, piece = un - row * pieces;
        const int y = ra + row, xa = piece * 16, xb = xa + 15, nv = vz_min(16, W - xa);
        unsigned base[16];
        if (present) {
            unsigned ne[4] = {0u, 0u, 0u, 0u}, no[4] = {0u, 0u, 0u, 0u}, pe[4] = {0u, 0u, 0u, 0u}, po[4] = {0u, 0u, 0u, 0u};
            const unsigned char* __restrict__ src = planes + (size_t)f * C * HW + (size_t)y * W + xa;
            vz_sum<VEC>(src, HW, 0, C / 2, bias, nv, ne, no);
            vz_sum<VEC>(src, HW, C / 2, C, bias, nv, pe, po);
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int wd = k >> 2, sh = 16 * ((k >> 1) & 1);
                const int neg = (int)((((k & 1) ? no[wd] : ne[wd]) >> sh) & 0xffffu);
                const int pos = (int)((((k & 1) ? po[wd] : pe[wd]) >> sh) & 0xffffu);
                base[k] = pos > neg ? 0xffffffu : (pos < neg ? 0u : 0x7f7f7fu);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) base[k] = 0u;
        }

#pragma unroll 1
        for (int p = 0; p < P; p++) {
            unsigned pix[16];
#pragma unroll
            for (int k = 0; k < 16; k++) pix[k] = base[k];
            const int n = p ? n1 : n0;
            for (int j = 0; j < n; j++) {
                const int* __restrict__ q = rec[p][j];
                const int x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], txt = q[5];
                const unsigned color = (unsigned)q[4] & 0xffffffu;
                const int ty = (q[4] & VZ_TAG_BELOW) ? y0 + 1 : y0 - 9;
                if (y >= y0 && y <= y1 && x1 >= xa && x0 <= xb) {
                    const unsigned m = (y == y0 || y == y1) ? vz_span(vz_max(x0, xa) - xa, vz_min(x1, xb) - xa)
                                                            : vz_bit(x0 - xa) | vz_bit(x1 - xa);
                    vz_paint(pix, m, color);
                }
                if (txt & VZ_HAS_TAG) {
                    const int nch = (txt & 15) + ((txt & VZ_HAS_SCORE) ? 5 : 0), xe = x0 + 6 * nch, v = y - ty;
                    if (v >= 0 && v <= 8 && xe >= xa && x0 <= xb) {
                        const unsigned tm = vz_span(vz_max(x0, xa) - xa, vz_min(xe, xb) - xa);
                        unsigned ink = 0u;
                        if (v >= 1 && v <= VZ_GLYPH_ROWS) {
                            const int c_lo = vz_max(xa - x0 - 1, 0) / 6, c_hi = vz_min(vz_max(xb - x0 - 1, 0) / 6, nch - 1);
                            for (int ci = c_lo; ci <= c_hi; ci++) {
                                const int ch = vz_char(tb, txt, ci) & 127;
                                const unsigned g = tb.glyphs[ch * VZ_GLYPH_ROWS + v - 1];
                                const unsigned rev = ((g & 1u) << 4) | ((g & 2u) << 2) | (g & 4u) | ((g & 8u) >> 2) | ((g & 16u) >> 4);
                                const int sh = x0 + 1 + 6 * ci - xa;          // -5 .. 16
                                ink |= sh >= 0 ? rev << sh : rev >> -sh;
                            }
                        }
                        ink &= tm;
                        const unsigned sum = (color & 255u) + ((color >> 8) & 255u) + ((color >> 16) & 255u);
                        vz_paint(pix, tm & ~ink, color);
                        vz_paint(pix, ink, sum >= 384u ? 0u : 0xffffffu);
                    }
                }
            }

            // the piece's 16 * S output pixels of one row are 3 * S lines of 16 bytes; the S replicated rows hold the same bytes
            unsigned char* __restrict__ o = out + ((((size_t)i * P + p) * H + y) * S) * Ws3 + (size_t)xa * S * 3;
            const int nbytes = nv * S * 3;
#pragma unroll
            for (int j = 0; j < 3 * S; j++) {
                u32x4 line;
#pragma unroll
                for (int d = 0; d < 4; d++) {
                    unsigned wv = 0u;
#pragma unroll
                    for (int bb = 0; bb < 4; bb++) {
                        const int byte = 16 * j + 4 * d + bb, op = byte / 3, comp = byte - 3 * op;
                        wv |= ((pix[op / S] >> (8 * comp)) & 0xffu) << (8 * bb);
                    }
                    line[d] = wv;
                }
                if constexpr (VEC) {
#pragma unroll
                    for (int r = 0; r < S; r++) vz_store<true>(o + (size_t)r * Ws3 + 16 * j, line, 16);
                } else {
#pragma unroll 1
                    for (int r = 0; r < S; r++) vz_store<false>(o + (size_t)r * Ws3 + 16 * j, line, nbytes - 16 * j);
                }
            }
        }
    }
}

typedef void (*VizKernel)(const unsigned char*, int, long long, int, int, int, VizPanel, VizPanel, int, const long long*, VizTables, int, int,
                          int, unsigned char*, int*);
template <bool VEC> static VizKernel viz_kernel_of(int scale) {
    return scale == 1 ? viz_render_kernel<VEC, 1> : (scale == 2 ? viz_render_kernel<VEC, 2> : viz_render_kernel<VEC, 4>);
}

}  // namespace

extern "C" {

int rvt_render_preview(const void* planes, int planes_signed, long long F, int C, int H, int W, const float* rows0, const int* count0, int N0,
                       int kind0, const float* rows1, const int* count1, int N1, int kind1, int P, const long long* frame_index,
                       long long Fout, const unsigned char* palette, int n_palette, const unsigned char* names, int n_names,
                       const unsigned char* glyphs, int scale, int flags, void* out, int* status, void* stream) {
    RVT_CHECK(planes && palette && out && status, "render_preview: null argument");
    RVT_CHECK(F >= 1 && F <= 0x7fffffffLL && Fout >= 1 && Fout <= 0x7fffffffLL, "render_preview: F=%lld, Fout=%lld frames outside the supported range", F, Fout);
    RVT_CHECK(C >= 2 && C % 2 == 0 && C <= VZ_MAX_C, "render_preview: C=%d channels must be even and in 2..%d", C, VZ_MAX_C);
    RVT_CHECK(H >= 1 && W >= 1 && H <= VZ_MAX_HW && W <= VZ_MAX_HW, "render_preview: H=%d W=%d outside the supported range 1..%d", H, W, VZ_MAX_HW);
    RVT_CHECK(scale == 1 || scale == 2 || scale == 4, "render_preview: scale=%d is not 1, 2 or 4", scale);
    RVT_CHECK(P == 1 || P == 2, "render_preview: P=%d panels, 1 or 2 are supported", P);
    RVT_CHECK((flags & ~RVT_VIZ_TEXT) == 0, "render_preview: unknown bits in flags=%d", flags);
    RVT_CHECK(frame_index || Fout <= F, "render_preview: without a frame_index Fout=%lld must not exceed F=%lld", Fout, F);
    const VizPanel pn[2] = {{rows0, count0, N0, kind0}, {rows1, count1, N1, kind1}};
    for (int p = 0; p < 2; p++) {
        RVT_CHECK((pn[p].rows == nullptr) == (pn[p].count == nullptr), "render_preview: panel %d has rows without count or count without rows", p);
        RVT_CHECK(p < P || !pn[p].rows, "render_preview: a box list for panel %d but P=%d", p, P);
        if (!pn[p].rows) continue;
        RVT_CHECK(pn[p].N >= 1, "render_preview: panel %d has N=%d rows per frame", p, pn[p].N);
        RVT_CHECK(pn[p].kind == RVT_VIZ_KIND_DET || pn[p].kind == RVT_VIZ_KIND_LABEL, "render_preview: panel %d has kind=%d, not 0 (detections) or 1 (labels)", p, pn[p].kind);
        RVT_CHECK(((uintptr_t)pn[p].rows & 3) == 0 && ((uintptr_t)pn[p].count & 3) == 0, "render_preview: rows / count of panel %d need 4-byte alignment", p);
    }
    RVT_CHECK(n_palette >= 1, "render_preview: n_palette=%d colours", n_palette);
    if (flags & RVT_VIZ_TEXT)
        RVT_CHECK(names && glyphs && n_names >= 1 && n_names <= VZ_MAX_NAMES, "render_preview: RVT_VIZ_TEXT needs names (n_names=%d in 1..%d) and glyphs", n_names, VZ_MAX_NAMES);
    RVT_CHECK(((uintptr_t)frame_index & 7) == 0 && ((uintptr_t)status & 3) == 0, "render_preview: frame_index needs 8-byte, status 4-byte alignment");
    const int pieces = (W + 15) / 16;
    const int chunk_rows = imax(1, imin(VZ_MAX_ROWS, VZ_PIECES / pieces));
    const int chunks = (H + chunk_rows - 1) / chunk_rows;
    RVT_CHECK(Fout * chunks <= 0x7fffffffLL, "render_preview: Fout=%lld images of %d rows exceed the grid", Fout, H);
    const bool vec = W % 16 == 0 && (uintptr_t)planes % 16 == 0 && (uintptr_t)out % 16 == 0;
    const VizTables tb = {palette, names, glyphs, n_palette, n_names};
    hipLaunchKernelGGL(vec ? viz_kernel_of<true>(scale) : viz_kernel_of<false>(scale), dim3((unsigned)(Fout * chunks)), dim3(VZ_THREADS), 0,
                       (hipStream_t)stream, (const unsigned char*)planes, planes_signed != 0 ? 1 : 0, F, C, H, W, pn[0], pn[1], P, frame_index, tb,
                       flags, chunk_rows, chunks, (unsigned char*)out, status);
    return check_launch("render_preview");
}

}  // extern "C"
