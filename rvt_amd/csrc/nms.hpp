// Detection post-processing: score filter + greedy per-class (or class-agnostic) NMS, batched over the images of a step with no
// host synchronisation.  Reference: models/detection/yolox/utils/boxes.py:32-76 (`postprocess`: corner boxes, class max, the
// obj * class_conf >= conf_thre mask, torchvision.ops.batched_nms / nms, a Python loop over the images with boolean-mask indexing).
//
// One workgroup of 1024 threads per image, one launch for the whole batch (images are independent: no grid-wide barrier):
//   1. score every anchor, compact the candidates into 64-bit keys  (order-preserving score bits << 32 | ~anchor);
//   2. sort the keys descending: bitonic sort of 4096-key chunks in LDS, chunks merged by rank (binary search in the other chunks).
//      Unsigned order of the key = descending score, and on an exact score tie the lower anchor first (stable, deterministic);
//   3. gather the sorted candidates' corner boxes / areas / classes / scores into the workspace (struct of arrays, L2 resident);
//   4. greedy NMS over blocks of 64 sorted candidates.  The block's 64x64 triangle is pure geometry, so the 16 waves compute it
//      together ahead of time: every wave holds the block (one box per lane), broadcasts 4 of its boxes with shuffles and leaves a
//      4-bit "suppressed by" nibble per lane in LDS.  Wave 0 then resolves the block with bit logic only (a ballot gives the
//      survivors; each survivor in turn clears the lanes whose 64-bit row has its bit set).  Then all waves apply the block's kept
//      boxes (at most 64, LDS broadcast reads) to every later candidate still alive and compute the next block's triangle, whose
//      boxes they loaded first, in the same barrier interval, while wave 0 also writes the block's kept rows.
//      Work = sum over blocks of kept x remaining (+ 64 per candidate), at most n^2 / 2 IoU evaluations; no n x n bit matrix, no
//      single-thread scan.
// IoU is torchvision's CPU formula in fp32, in its operation order, with HIP's correctly rounded divide; this translation unit is
// compiled with -ffp-contract=off, so every keep / kill decision is the one the same formula gives in torch, bit for bit.
#pragma once
#include "common.hpp"
#include "simota.hpp"    // YoloLevels, sigmoid_exact: the decode kernel's own expressions

namespace rvt {

constexpr int NMS_THREADS = 1024;      // 16 waves: 4 per SIMD
constexpr int NMS_CHUNK = 4096;        // keys sorted in LDS at once (32 KB)
constexpr int NMS_MAX_A = 16384;       // anchors per image (dead flags: one LDS byte per candidate, inside the sort buffer)
constexpr int NMS_MAX_NC = 80;

struct NmsWs {                          // every array is [B][A]
    unsigned long long *keys, *sorted;
    float *x1, *y1, *x2, *y2, *area, *obj, *conf;   // of sorted candidate j
    int *cls, *acls;                    // class of sorted candidate j / of anchor a
};

__device__ __forceinline__ unsigned long long wave_ballot(bool p) {
#ifndef RVT_EMU
    return __ballot(p ? 1 : 0);
#else
    unsigned long long m = p ? 1ull << (threadIdx.x & 63) : 0ull;
    for (int s = 1; s < 64; s <<= 1) m |= __shfl_xor(m, s);
    return m;
#endif
}

// fp32 -> unsigned with the same order (-0 and +0 coincide, as they compare equal)
__device__ __forceinline__ unsigned nms_score_key(float s) {
    unsigned u = __builtin_bit_cast(unsigned, s);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// does kept box a suppress candidate b?  torchvision's nms_kernel_impl order: inter / (area_a + area_b - inter) > thr, no "+1".
// A zero union never suppresses (0 / 0 is NaN there and NaN > thr is false; this file is built with -fno-honor-nans, hence explicit).
__device__ __forceinline__ bool nms_suppresses(float ax1, float ay1, float ax2, float ay2, float aarea,
                                               float bx1, float by1, float bx2, float by2, float barea, float thr) {
    const float iw = fmaxf(0.f, fminf(ax2, bx2) - fmaxf(ax1, bx1));
    const float ih = fmaxf(0.f, fminf(ay2, by2) - fmaxf(ay1, by1));
    const float inter = iw * ih;
    if (!(inter > 0.f) && thr >= 0.f) return false;                    // disjoint: iou = 0 (or 0 / 0), never > thr; skips the divide
    const float uni = aarea + barea - inter;
    return uni > 0.f && inter / uni > thr;
}

// Where one image's anchors come from.  A source gives, for anchor a in [0, A):
//   score(a, bc):  obj * max class score (one fp32 multiply) and the class that holds the max (lowest index on an exact tie);
//   fetch(a, c, ...): the decoded box cx cy w h, the objectness score and the score of class c.
// NmsPredSrc: rows of the decoded fp32 tensor [A][5+nc] (rvt_yolox_decode's pred_infer): everything is a copy.
struct NmsPredSrc {
    const float* p;
    int nc;
    __device__ __forceinline__ float score(int a, int& bc) const {
        const float* r = p + (size_t)a * (5 + nc);
        float best = r[5];
        bc = 0;
        for (int c = 1; c < nc; c++) {
            const float v = r[5 + c];
            if (v > best) { best = v; bc = c; }                       // the lowest class index wins an exact tie
        }
        return r[4] * best;
    }
    __device__ __forceinline__ void fetch(int a, int c, float& cx, float& cy, float& bw, float& bh, float& obj, float& conf) const {
        const float* r = p + (size_t)a * (5 + nc);
        cx = r[0]; cy = r[1]; bw = r[2]; bh = r[3];
        obj = r[4];
        conf = r[5 + c];
    }
};

// NmsMapSrc: the head's per-level prediction maps themselves (reg_obj [B*H*W][ld_ro], cls [B*H*W][ld_cls], as yolox_decode_kernel
// reads them), decoded on the fly with that kernel's expressions in its operation order: the scores for every anchor, the box only
// for the anchors that became candidates.  The class max runs over the SIGMOID values (two logits may round to one sigmoid; the lower
// class must still win), so score / class / box are the bits the decoded tensor would hold.
struct DetectMaps {
    const void *ro[8], *cl[8];
    int ld_ro, ld_cls;
};
template <class T>
struct NmsMapSrc {
    const DetectMaps& m;
    const YoloLevels& lv;
    int b, nc;
    // level of anchor a by a chain of selects over the (uniform) level table: no dynamically indexed kernel argument
    __device__ __forceinline__ void locate(int a, const T*& rr, const T*& cc, float& gx, float& gy, float& st) const {
        int a0 = 0, W = lv.w[0], hw = lv.h[0] * lv.w[0], s = lv.stride[0];
        const T *ro = (const T*)m.ro[0], *cl = (const T*)m.cl[0];
#pragma unroll
        for (int i = 1; i < 8; i++)
            if (i < lv.n && a >= lv.a0[i]) {
                a0 = lv.a0[i]; W = lv.w[i]; hw = lv.h[i] * lv.w[i]; s = lv.stride[i];
                ro = (const T*)m.ro[i]; cl = (const T*)m.cl[i];
            }
        const int q = a - a0;                                          // in [0, hw): the levels add up to A (checked by the host)
        const size_t row = (size_t)b * hw + q;
        rr = ro + row * m.ld_ro;
        cc = cl + row * m.ld_cls;
        gx = (float)(q % W); gy = (float)(q / W); st = (float)s;
    }
    __device__ __forceinline__ float score(int a, int& bc) const {
        const T *rr, *cc;
        float gx, gy, st;
        locate(a, rr, cc, gx, gy, st);
        float best = sigmoid_exact((float)cc[0]);
        bc = 0;
        for (int c = 1; c < nc; c++) {
            const float v = sigmoid_exact((float)cc[c]);
            if (v > best) { best = v; bc = c; }
        }
        return sigmoid_exact((float)rr[4]) * best;
    }
    __device__ __forceinline__ void fetch(int a, int c, float& cx, float& cy, float& bw, float& bh, float& obj, float& conf) const {
        const T *rr, *cc;
        float gx, gy, st;
        locate(a, rr, cc, gx, gy, st);
        cx = ((float)rr[0] + gx) * st; cy = ((float)rr[1] + gy) * st;
        bw = expf((float)rr[2]) * st; bh = expf((float)rr[3]) * st;
        obj = sigmoid_exact((float)rr[4]);
        conf = sigmoid_exact((float)cc[c]);
    }
};

// One image (blockIdx.x) of `src` -> det [B][max_det][7] (x1 y1 x2 y2 obj class_conf class_pred), count [B] (kept, before
// the max_det cap), anchor_idx [B][max_det] (nullptr = skip).  Rows past min(count, max_det) are zero / -1.
// Every index is an integer derived from A and the compaction counter, never from a float: any input bits terminate in bounds.
template <class Src>
__device__ __forceinline__ void nms_image(const Src& src, int A, float conf_thre, float nms_thre, int agnostic, int max_det,
                                          float* __restrict__ det, int* __restrict__ count, int* __restrict__ anchor_idx, const NmsWs& w) {
    __shared__ unsigned long long skey[NMS_CHUNK];
    __shared__ float kx1[64], ky1[64], kx2[64], ky2[64], karea[64];
    __shared__ int kcls[64];
    __shared__ unsigned char snib[NMS_THREADS / 64][64];                // snib[w][l]: which of the boxes 4w .. 4w+3 suppress box l
    __shared__ unsigned long long s_mask;
    __shared__ int s_n, s_total;
    constexpr int T = NMS_THREADS;
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t img = (size_t)b * A;
    unsigned long long* keys = w.keys + img;
    unsigned long long* sorted = w.sorted + img;
    float *bx1 = w.x1 + img, *by1 = w.y1 + img, *bx2 = w.x2 + img, *by2 = w.y2 + img, *barea = w.area + img;
    float *bobj = w.obj + img, *bconf = w.conf + img;
    int *bcls = w.cls + img, *acls = w.acls + img;

    // ---- 1. score, class, candidate keys (compaction order is arbitrary: the sort decides) ------------------------------
    if (tid == 0) s_n = 0;
    __syncthreads();
    for (int a = tid; a < A; a += T) {
        int bc;
        const float score = src.score(a, bc);
        acls[a] = bc;
        if (score >= conf_thre) {
            const int slot = atomicAdd(&s_n, 1);                      // < A: one increment per anchor at most
            keys[slot] = ((unsigned long long)nms_score_key(score) << 32) | (unsigned)~a;
        }
    }
    __syncthreads();
    const int n = s_n < A ? s_n : A;

    // ---- 2. sort descending ----------------------------------------------------------------------------------------------
    const int nch = (n + NMS_CHUNK - 1) / NMS_CHUNK;
    for (int c = 0; c < nch; c++) {
        const int base = c * NMS_CHUNK, m = n - base < NMS_CHUNK ? n - base : NMS_CHUNK;
        int P = 2;
        while (P < m) P <<= 1;
        for (int i = tid; i < P; i += T) skey[i] = i < m ? keys[base + i] : 0ull;      // 0 sorts after every real key (~a != 0)
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += T) {
                    const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), q = i | j;
                    const unsigned long long u = skey[i], v = skey[q];
                    if (((i & k) == 0) ? u < v : u > v) { skey[i] = v; skey[q] = u; }
                }
                __syncthreads();
            }
        }
        for (int i = tid; i < m; i += T) sorted[base + i] = skey[i];
        __syncthreads();
    }
    const unsigned long long* order = sorted;
    if (nch > 1) {                                                      // rank merge: keys are unique, the positions a permutation
        for (int e = tid; e < n; e += T) {
            const int c = e / NMS_CHUNK;
            const unsigned long long key = sorted[e];
            int pos = e - c * NMS_CHUNK;
            for (int c2 = 0; c2 < nch; c2++) {
                if (c2 == c) continue;
                const int base = c2 * NMS_CHUNK, m2 = n - base < NMS_CHUNK ? n - base : NMS_CHUNK;
                int lo = 0, hi = m2;
                for (int it = 0; it < 13 && lo < hi; it++) {            // 2^12 = NMS_CHUNK: 13 halvings close any interval
                    const int mid = (lo + hi) >> 1;
                    if (sorted[base + mid] > key) lo = mid + 1; else hi = mid;
                }
                pos += lo;
            }
            keys[pos < n ? pos : n - 1] = key;
        }
        __syncthreads();
        order = keys;
    }

    // ---- 3. gather the sorted candidates ---------------------------------------------------------------------------------
    unsigned char* dead = reinterpret_cast<unsigned char*>(skey);       // NMS_MAX_A bytes <= 32 KB; the sort is finished
    for (int j = tid; j < n; j += T) {
        int a = (int)~(unsigned)order[j];
        a = a < 0 ? 0 : (a < A ? a : A - 1);
        const int c = acls[a];
        float cx, cy, bw, bh, obj, conf;
        src.fetch(a, c, cx, cy, bw, bh, obj, conf);
        const float hw = bw / 2, hh = bh / 2;
        const float x1 = cx - hw, y1 = cy - hh, x2 = cx + hw, y2 = cy + hh;
        bx1[j] = x1; by1[j] = y1; bx2[j] = x2; by2[j] = y2;
        barea[j] = (x2 - x1) * (y2 - y1);
        bcls[j] = c;
        bobj[j] = obj;
        bconf[j] = conf;
        dead[j] = 0;
    }
    __syncthreads();

    // ---- 4. greedy NMS, 64 candidates per block ---------------------------------------------------------------------------
    int nkept = 0;                                                      // wave 0's running row count
    const int nblk = (n + 63) >> 6, wave = tid >> 6, lane = tid & 63;
    // every wave holds the current block, one box per lane; the next block is loaded one barrier interval ahead
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f, ar = 0.f;
    int c = 0;
    auto load_block = [&](int blk, float& ox1, float& oy1, float& ox2, float& oy2, float& oar, int& oc) {
        const int j = (blk << 6) + lane, jj = j < n ? j : n - 1;
        ox1 = bx1[jj]; oy1 = by1[jj]; ox2 = bx2[jj]; oy2 = by2[jj]; oar = barea[jj]; oc = bcls[jj];
    };
    // triangle of a block: bits of the (geometric) relation "box i suppresses the later box l of the same block"
    auto triangle = [&](float tx1, float ty1, float tx2, float ty2, float tar, int tc) {
        unsigned nib = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int i = 4 * wave + q;
            const float ax1 = __shfl(tx1, i), ay1 = __shfl(ty1, i), ax2 = __shfl(tx2, i), ay2 = __shfl(ty2, i), aar = __shfl(tar, i);
            const int ac = __shfl(tc, i);
            if (i < lane && (agnostic || ac == tc) && nms_suppresses(ax1, ay1, ax2, ay2, aar, tx1, ty1, tx2, ty2, tar, nms_thre)) nib |= 1u << q;
        }
        snib[wave][lane] = (unsigned char)nib;
    };
    if (nblk > 0) {
        load_block(0, x1, y1, x2, y2, ar, c);
        triangle(x1, y1, x2, y2, ar, c);
    }
    __syncthreads();
    for (int blk = 0; blk < nblk; blk++) {
        const int j0 = blk << 6, j = j0 + lane, jj = j < n ? j : n - 1;
        bool alive = false;
        unsigned long long mask = 0ull;
        if (tid < 64) {                                                 // resolve: bit logic only, nothing from global memory
            kx1[tid] = x1; ky1[tid] = y1; kx2[tid] = x2; ky2[tid] = y2; karea[tid] = ar; kcls[tid] = c;
            unsigned long long sup = 0ull;                              // bit i: box i of this block suppresses mine, if it is kept
#pragma unroll
            for (int w2 = 0; w2 < NMS_THREADS / 64; w2++) sup |= (unsigned long long)snib[w2][tid] << (4 * w2);
            alive = j < n && dead[jj] == 0;
            mask = wave_ballot(alive);
            unsigned long long done = 0ull;
            for (int it = 0; it < 64; it++) {
                const unsigned long long rem = mask & ~done;
                if (rem == 0ull) break;
                const int i = __builtin_ctzll(rem);                     // the best survivor not applied yet: kept for good
                if ((sup >> i) & 1ull) alive = false;
                mask = wave_ballot(alive);
                done = (2ull << i) - 1ull;
            }
            if (tid == 0) s_mask = mask;
        }
        __syncthreads();
        const bool more = blk + 1 < nblk;
        float nx1 = 0.f, ny1 = 0.f, nx2 = 0.f, ny2 = 0.f, nar = 0.f;
        int ncl = 0;
        if (more) load_block(blk + 1, nx1, ny1, nx2, ny2, nar, ncl);    // issued first: their latency overlaps the work below
        if (tid < 64) {                                                 // the block's kept rows, beside the other waves' work
            const int row = nkept + __builtin_popcountll(mask & ((1ull << tid) - 1ull));
            if (alive && row < max_det) {
                int a = (int)~(unsigned)order[jj];
                a = a < 0 ? 0 : (a < A ? a : A - 1);
                float* d = det + ((size_t)b * max_det + row) * 7;
                d[0] = x1; d[1] = y1; d[2] = x2; d[3] = y2; d[4] = bobj[jj]; d[5] = bconf[jj]; d[6] = (float)c;
                if (anchor_idx != nullptr) anchor_idx[(size_t)b * max_det + row] = a;
            }
            nkept += __builtin_popcountll(mask);
        }
        const unsigned long long kept = s_mask;
        for (int k = j0 + 64 + tid; k < n; k += T) {
            if (dead[k]) continue;
            const float cx1 = bx1[k], cy1 = by1[k], cx2 = bx2[k], cy2 = by2[k], car = barea[k];
            const int cc = bcls[k];
            unsigned long long rem = kept;
            for (int it = 0; it < 64 && rem != 0ull; it++) {
                const int i = __builtin_ctzll(rem);
                rem &= rem - 1ull;
                if ((agnostic || kcls[i] == cc) &&
                    nms_suppresses(kx1[i], ky1[i], kx2[i], ky2[i], karea[i], cx1, cy1, cx2, cy2, car, nms_thre)) {
                    dead[k] = 1;
                    break;
                }
            }
        }
        if (more) {                                                     // read by wave 0 after the barrier; independent of `dead`
            triangle(nx1, ny1, nx2, ny2, nar, ncl);
            x1 = nx1; y1 = ny1; x2 = nx2; y2 = ny2; ar = nar; c = ncl;
        }
        __syncthreads();
    }

    // ---- count, zero the unused rows -------------------------------------------------------------------------------------
    if (tid == 0) { s_total = nkept; count[b] = nkept; }
    __syncthreads();
    const int first = s_total < max_det ? s_total : max_det;
    float* dz = det + ((size_t)b * max_det + first) * 7;
    for (int i = tid; i < (max_det - first) * 7; i += T) dz[i] = 0.f;
    if (anchor_idx != nullptr)
        for (int i = first + tid; i < max_det; i += T) anchor_idx[(size_t)b * max_det + i] = -1;
}

// pred [B][A][5+nc] (cx cy w h obj cls...), the decoded tensor
__global__ void __launch_bounds__(NMS_THREADS)
yolox_postprocess_kernel(const float* __restrict__ pred, int A, int nc, float conf_thre, float nms_thre, int agnostic, int max_det,
                         float* __restrict__ det, int* __restrict__ count, int* __restrict__ anchor_idx, NmsWs w) {
    const NmsPredSrc src{pred + (size_t)blockIdx.x * A * (5 + nc), nc};
    nms_image(src, A, conf_thre, nms_thre, agnostic, max_det, det, count, anchor_idx, w);
}

// the head's prediction maps: decode + score filter + NMS in one launch (rvt_yolox_detect)
template <class T>
__global__ void __launch_bounds__(NMS_THREADS)
yolox_detect_kernel(DetectMaps m, YoloLevels lv, int A, int nc, float conf_thre, float nms_thre, int agnostic, int max_det,
                    float* __restrict__ det, int* __restrict__ count, int* __restrict__ anchor_idx, NmsWs w) {
    const NmsMapSrc<T> src{m, lv, (int)blockIdx.x, nc};
    nms_image(src, A, conf_thre, nms_thre, agnostic, max_det, det, count, anchor_idx, w);
}

}  // namespace rvt
