// Prophesee / COCO mAP evaluation of detections on the device.  Reference: utils/evaluation/prophesee/ (io/box_filtering.py
// filter_boxes, evaluation.py evaluate_list, metrics/coco_eval.py) and the COCOeval core it calls (evaluateImg / accumulate,
// bbox mode, iscrowd false everywhere, maxDets = 100): there every frame is copied to the host, turned into one Python dict per
// box and matched in a per-image, per-category, per-threshold Python loop.
//
// coco_match_kernel: one launch for a batch of frames, ONE WAVE per (frame, category).
//   The 40 (IoU threshold, area range) matchers of a (frame, category) are independent sequential scans over the same D x G IoU
//   tile (D <= 100 detections, G ground-truth boxes of the category), so the wave computes the tile once, in double, into LDS
//   (D * G / 64 divides per lane) and then runs one matcher per lane: lane = 4 * threshold + area range, lanes 40 .. 63 idle.
//   Every lane walks the same (d, g) sequence, so the tile reads are LDS broadcasts and `iou < lowest threshold` is a wave-uniform
//   skip that removes almost every pair; the state a lane keeps is the 128-bit "matched" set of its ground truth.  Two ballots per
//   detection give the record's 40-bit matched / ignored masks directly.  COCOeval's ordering of the ground truth (non-ignored
//   first, stable) and its early exit are restated per lane as "best non-ignored candidate, else best ignored candidate", both with
//   `>=` so that the later box wins an exact tie.
//   Before that the wave applies the Prophesee filter to the frame's labels and detections (fp32, no fused multiply-add), decides
//   whether the frame is an image (one surviving label of any class), counts the surviving detections per class (LDS atomics: the
//   record offset of category k is the sum of min(100, count) over the categories before it) and selects its category's top 100
//   by class_conf with a bitonic sort of 64-bit keys (score bits << 32 | ~row: descending score, the earlier row first on a tie).
//   A workgroup of several waves would only add barriers: the frames and categories of a batch already give 72 .. 128 independent
//   waves, and a wave's LDS tile (GMAX = 32: 26 KB, GMAX = 128: 100 KB of the CU's 160 KB) bounds how many share a CU.
// The three accumulate kernels turn the records, read through the order of a (category, descending score, arrival) sort, into
// COCOeval's precision table without one integer plane per (threshold, area): chunks of 1024 records are counted per lane
// (coco_count_kernel), the chunk counts become exclusive prefixes (coco_scan_kernel), and a second walk (coco_emit_kernel) turns
// every true positive into tp / (tp + fp + eps) and keeps the maximum per recall bucket with a 64-bit atomic max (positive
// doubles order like their bits).  precision[t][r] is then the maximum over the buckets >= r (coco_finish_kernel): exactly the
// reference's right-to-left maximum sampled at the first index whose recall reaches level r, since tp only grows along the list.
// Every quotient is one correctly rounded double division of small integers, as in numpy.
#pragma once
#include "common.hpp"

namespace rvt {

constexpr int EVAL_MAX_DET = 1024;     // detection rows per frame (the sort buffer, 8 KB of LDS)
constexpr int EVAL_MAX_G = 128;        // label rows per frame (two 64-bit words of matched / ignored bits per lane)
constexpr int EVAL_MAX_NC = 16;
constexpr int EVAL_TOP = 100;          // COCOeval maxDets[-1]
constexpr int EVAL_T = 10, EVAL_A = 4, EVAL_LANES = EVAL_T * EVAL_A, EVAL_R = 101;
constexpr int EVAL_CHUNK = 1024;       // records per counted chunk
constexpr long long EVAL_NO_RECORD = 0x7fffffffffffffffLL;   // key of an unused record slot: sorts behind every category
// counters (int32, accumulated over the launches of an evaluation): npig[k][a] at 4k + a, kept detections of category k at
// 64 + k, images at 80, images with at least one surviving detection at 81, frames with count > max_det at 82
constexpr int EVAL_CNT_NDET = 4 * EVAL_MAX_NC, EVAL_CNT_IMAGES = EVAL_CNT_NDET + EVAL_MAX_NC, EVAL_CNT_IMAGES_DET = EVAL_CNT_IMAGES + 1,
              EVAL_CNT_TRUNCATED = EVAL_CNT_IMAGES + 2, EVAL_COUNTERS = 96;

__device__ __forceinline__ unsigned long long eval_ballot(bool p) {
#ifndef RVT_EMU
    return __ballot(p ? 1 : 0);
#else
    unsigned long long m = p ? 1ull << (threadIdx.x & 63) : 0ull;
    for (int s = 1; s < 64; s <<= 1) m |= __shfl_xor(m, s);
    return m;
#endif
}

// fp32 -> unsigned with the same order (-0 and +0 coincide, as they compare equal)
__device__ __forceinline__ unsigned eval_score_key(float s) {
    unsigned u = __builtin_bit_cast(unsigned, s);
    if ((u << 1) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ bool eval_box_kept(float w, float h, float min_diag2, float min_side) {
    return w * w + h * h >= min_diag2 && w >= min_side && h >= min_side;
}

// COCOeval areaRng: all, small, medium, large; outside = ignored
__device__ __forceinline__ unsigned eval_area_outside(float area_f32) {
    const double ar = (double)area_f32;
    unsigned m = 0;
    if (ar < 0.0 || ar > 1e10) m |= 1u;
    if (ar < 0.0 || ar > 1024.0) m |= 2u;
    if (ar < 1024.0 || ar > 9216.0) m |= 4u;
    if (ar < 9216.0 || ar > 1e10) m |= 8u;
    return m;
}

__device__ __forceinline__ void eval_atomic_max(unsigned long long* p, unsigned long long v) {
#ifndef RVT_EMU
    atomicMax(p, v);
#else
    if (*p < v) *p = v;
#endif
}

// det [F][max_det][7] (x1 y1 x2 y2 obj class_conf class; xywh != 0: x y w h instead of the corners), count [F], lab [F][G][7]
// (t x y w h class_id class_confidence), lcount [F] (<= 0: no labels), t_us [F], iou_thr [10].  rkey / rmatched / rignored
// [F][R]: the frame's records, category by category, R >= min(max_det, 100 K); unused slots get EVAL_NO_RECORD.
// Every index derives from the clamped counts, never from a float: any input bits terminate in bounds.
template <int GMAX>
__global__ void __launch_bounds__(64)
coco_match_kernel(const float* __restrict__ det, const int* __restrict__ count, const float* __restrict__ lab,
                  const int* __restrict__ lcount, const long long* __restrict__ t_us, const double* __restrict__ iou_thr, int max_det,
                  int G, int K, int R, int xywh, float min_diag2, float min_side, long long* __restrict__ rkey,
                  long long* __restrict__ rmatched, long long* __restrict__ rignored, int* __restrict__ counters) {
    __shared__ unsigned long long skey[EVAL_MAX_DET];
    __shared__ double tile[EVAL_TOP * GMAX];
    __shared__ float gx[GMAX], gy[GMAX], gw[GMAX], gh[GMAX];
    __shared__ float dx[EVAL_TOP], dy[EVAL_TOP], dw[EVAL_TOP], dh[EVAL_TOP];
    __shared__ unsigned char dout[EVAL_TOP];
    __shared__ unsigned long long s_ign[EVAL_A][2];
    __shared__ int s_cnt[EVAL_MAX_NC];
    const int f = blockIdx.x / K, k = blockIdx.x - f * K, lane = threadIdx.x;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const bool t_ok = t_us[f] > 500000LL;
    const int cnt_raw = count[f];
    const int n = cnt_raw < 0 ? 0 : (cnt_raw < max_det ? cnt_raw : max_det);
    int lc = lcount[f];
    lc = lc < 0 ? 0 : (lc < G ? lc : G);
    if (lane < EVAL_MAX_NC) s_cnt[lane] = 0;
    if (lane < 2 * EVAL_A) s_ign[lane >> 1][lane & 1] = 0ull;
    __syncthreads();

    // ---- ground truth: filter, image decision, this category's boxes in their original order -----------------------------
    bool image = false;
    int gk = 0;
    for (int g0 = 0; g0 < lc; g0 += 64) {
        const int g = g0 + lane;
        const float* r = lab + ((size_t)f * G + (g < lc ? g : lc - 1)) * 7;
        const float x = r[1], y = r[2], w = r[3], h = r[4], c = r[5];
        const bool keep = g < lc && t_ok && eval_box_kept(w, h, min_diag2, min_side);
        const bool mine = keep && c == (float)k;
        image = image || eval_ballot(keep) != 0ull;
        const unsigned long long bm = eval_ballot(mine);
        const int pos = gk + __builtin_popcountll(bm & lt);
        if (mine && pos < GMAX) {
            gx[pos] = x; gy[pos] = y; gw[pos] = w; gh[pos] = h;
        }
        gk += __builtin_popcountll(bm);
    }
    gk = gk < GMAX ? gk : GMAX;
    __syncthreads();
    for (int c0 = 0; c0 < gk; c0 += 64) {
        const int g = c0 + lane;
        const unsigned out = g < gk ? eval_area_outside(gw[g] * gh[g]) : 0u;
#pragma unroll
        for (int a = 0; a < EVAL_A; a++) {
            const unsigned long long b = eval_ballot(((out >> a) & 1u) != 0u);
            if (lane == 0) s_ign[a][c0 >> 6] = b;
        }
    }
    __syncthreads();

    // ---- detections: filter, per-class counts, this category's sort keys ---------------------------------------------------
    int m = 0;
    bool any_det = false;
    if (image) {
        for (int j0 = 0; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const float* r = det + ((size_t)f * max_det + (j < n ? j : n - 1)) * 7;
            const float w = xywh ? r[2] : r[2] - r[0], h = xywh ? r[3] : r[3] - r[1], c = r[6];
            const bool keep = j < n && t_ok && eval_box_kept(w, h, min_diag2, min_side);
            any_det = any_det || eval_ballot(keep) != 0ull;
            if (keep && c >= 0.f && c < (float)K) {
                const int ci = (int)c;
                if ((float)ci == c) atomicAdd(&s_cnt[ci], 1);
            }
            const bool mine = keep && c == (float)k;
            const unsigned long long bm = eval_ballot(mine);
            const int pos = m + __builtin_popcountll(bm & lt);
            if (mine) skey[pos] = ((unsigned long long)eval_score_key(r[5]) << 32) | (unsigned)~j;   // pos < n <= EVAL_MAX_DET
            m += __builtin_popcountll(bm);
        }
    }
    __syncthreads();
    if (m > 1) {                                                         // bitonic sort, descending; 0 pads sort last (~j != 0)
        int P = 2;
        while (P < m) P <<= 1;
        for (int i = m + lane; i < P; i += 64) skey[i] = 0ull;
        __syncthreads();
        for (int kk = 2; kk <= P; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                for (int t = lane; t < (P >> 1); t += 64) {
                    const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1)), q = i | jj;
                    const unsigned long long u = skey[i], v = skey[q];
                    if (((i & kk) == 0) ? u < v : u > v) { skey[i] = v; skey[q] = u; }
                }
                __syncthreads();
            }
        }
    }
    const int D = m < EVAL_TOP ? m : EVAL_TOP;
    for (int d = lane; d < D; d += 64) {
        int j = (int)~(unsigned)skey[d];
        j = j < 0 ? 0 : (j < n ? j : n - 1);
        const float* r = det + ((size_t)f * max_det + j) * 7;
        const float w = xywh ? r[2] : r[2] - r[0], h = xywh ? r[3] : r[3] - r[1];
        dx[d] = r[0]; dy[d] = r[1]; dw[d] = w; dh[d] = h;
        dout[d] = (unsigned char)eval_area_outside(w * h);
    }
    __syncthreads();

    // ---- IoU tile in double on the widened fp32 x y w h (the bbIou of the COCO API) -----------------------------------------------
    for (int idx = lane; idx < D * gk; idx += 64) {
        const int d = idx / gk, g = idx - d * gk;
        const double Dx = dx[d], Dy = dy[d], Dw = dw[d], Dh = dh[d], Gx = gx[g], Gy = gy[g], Gw = gw[g], Gh = gh[g];
        const double iw = fmin(Dx + Dw, Gx + Gw) - fmax(Dx, Gx), ih = fmin(Dy + Dh, Gy + Gh) - fmax(Dy, Gy);
        double v = 0.0;
        if (iw > 0.0 && ih > 0.0) {
            const double i = iw * ih;
            v = i / (Dw * Dh + Gw * Gh - i);
        }
        tile[idx] = v;
    }
    __syncthreads();

    // ---- record slots of this (frame, category) ---------------------------------------------------------------------------------------
    int off = 0, total = 0;
    for (int c = 0; c < K; c++) {
        const int v = image ? (s_cnt[c] < EVAL_TOP ? s_cnt[c] : EVAL_TOP) : 0;
        if (c < k) off += v;
        total += v;
    }
    total = total < R ? total : R;
    const size_t base = (size_t)f * R;

    // ---- 40 greedy matchers, one per lane -----------------------------------------------------------------------------------------------
    const int a = lane & 3;
    const bool active = lane < EVAL_LANES;
    const double thr = active ? iou_thr[lane >> 2] : 2.0;
    const double best0 = thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10;
    double thr_lo = best0;
    for (int s = 1; s < 64; s <<= 1) {
        const double o = __shfl_xor(thr_lo, s);
        thr_lo = o < thr_lo ? o : thr_lo;
    }
    const unsigned long long ig0 = s_ign[a][0], ig1 = s_ign[a][1];
    unsigned long long mt0 = 0ull, mt1 = 0ull;
    for (int d = 0; d < D; d++) {
        double b1 = best0, b2 = best0;
        int m1 = -1, m2 = -1;
        const double* row = tile + d * gk;
        for (int g = 0; g < gk; g++) {
            const double v = row[g];
            if (v < thr_lo) continue;                                    // wave-uniform: no lane can take this pair
            const bool hi = g >= 64;
            const int sh = g & 63;
            const bool used = (((hi ? mt1 : mt0) >> sh) & 1ull) != 0ull, ign = (((hi ? ig1 : ig0) >> sh) & 1ull) != 0ull;
            if (!used) {
                if (!ign) { if (v >= b1) { b1 = v; m1 = g; } }
                else if (v >= b2) { b2 = v; m2 = g; }
            }
        }
        const int mm = m1 >= 0 ? m1 : m2;
        const bool has = active && mm >= 0;
        bool ignored = active && ((dout[d] >> a) & 1) != 0;
        if (has) {
            ignored = m1 < 0;                                            // a match inherits the ignore flag of its ground truth
            if (mm >= 64) mt1 |= 1ull << (mm - 64); else mt0 |= 1ull << mm;
        }
        const unsigned long long MM = eval_ballot(has), IM = eval_ballot(ignored);
        if (lane == 0 && off + d < R) {
            const unsigned sk = (unsigned)(skey[d] >> 32);
            rkey[base + off + d] = (long long)(((unsigned long long)k << 32) | (unsigned)~sk);
            rmatched[base + off + d] = (long long)MM;
            rignored[base + off + d] = (long long)IM;
        }
    }
    if (k == K - 1)
        for (int i = total + lane; i < R; i += 64) {
            rkey[base + i] = EVAL_NO_RECORD; rmatched[base + i] = 0; rignored[base + i] = 0;
        }

    // ---- counters ---------------------------------------------------------------------------------------------------------------------------
    if (image && lane < EVAL_A) {
        const int npig = gk - __builtin_popcountll(s_ign[lane][0]) - __builtin_popcountll(s_ign[lane][1]);
        if (npig > 0) atomicAdd(&counters[4 * k + lane], npig);
    }
    if (lane == 0) {
        if (image && D > 0) atomicAdd(&counters[EVAL_CNT_NDET + k], (off + D <= R ? D : (R > off ? R - off : 0)));
        if (k == 0) {
            if (image) atomicAdd(&counters[EVAL_CNT_IMAGES], 1);
            if (image && any_det) atomicAdd(&counters[EVAL_CNT_IMAGES_DET], 1);
            if (cnt_raw > max_det) atomicAdd(&counters[EVAL_CNT_TRUNCATED], 1);
        }
    }
}

// ---- accumulate ------------------------------------------------------------------------------------------------------------------------------
// The sorted list holds category k in [start_k, start_k + n_k), n_k = counters[64 + k]; perm[i] is the record slot at sorted
// position i.  All three walks clamp positions and slots into [0, N).
struct EvalSeg { long long start, n; };

__device__ __forceinline__ EvalSeg eval_segment(const int* counters, int k, long long N) {
    long long s = 0;
    for (int c = 0; c < k; c++) s += counters[EVAL_CNT_NDET + c] > 0 ? counters[EVAL_CNT_NDET + c] : 0;
    long long n = counters[EVAL_CNT_NDET + k] > 0 ? counters[EVAL_CNT_NDET + k] : 0;
    s = s < N ? s : N;
    n = s + n <= N ? n : N - s;
    return EvalSeg{s, n};
}

// one wave per (chunk j, category k): cnt[(k * nch + j) * 40 + lane] = true positives | false positives << 32 of the chunk
__global__ void __launch_bounds__(64)
coco_count_kernel(const long long* __restrict__ perm, const long long* __restrict__ rmatched, const long long* __restrict__ rignored,
                  long long N, int nch, const int* __restrict__ counters, unsigned long long* __restrict__ cnt) {
    __shared__ unsigned long long sm[64], si[64];
    const int k = blockIdx.x / nch, j = blockIdx.x - k * nch, lane = threadIdx.x;
    const EvalSeg seg = eval_segment(counters, k, N);
    const long long lo = (long long)j * EVAL_CHUNK;
    if (lo >= seg.n) return;
    const long long hi = lo + EVAL_CHUNK < seg.n ? lo + EVAL_CHUNK : seg.n;
    unsigned tp = 0, fp = 0;
    for (long long i0 = lo; i0 < hi; i0 += 64) {
        const long long i = i0 + lane;
        unsigned long long mm = 0ull, ig = ~0ull;
        if (i < hi) {
            long long p = perm[seg.start + i];
            p = p < 0 ? 0 : (p < N ? p : N - 1);
            mm = (unsigned long long)rmatched[p]; ig = (unsigned long long)rignored[p];
        }
        __syncthreads();
        sm[lane] = mm; si[lane] = ig;
        __syncthreads();
        const int cnt64 = hi - i0 < 64 ? (int)(hi - i0) : 64;
        for (int q = 0; q < cnt64; q++) {
            const unsigned mb = (unsigned)(sm[q] >> lane) & 1u, ib = (unsigned)(si[q] >> lane) & 1u;
            tp += mb & ~ib & 1u;
            fp += ~mb & ~ib & 1u;
        }
    }
    if (lane < EVAL_LANES) cnt[((size_t)k * nch + j) * EVAL_LANES + lane] = (unsigned long long)tp | ((unsigned long long)fp << 32);
}

// one workgroup of 16 waves per category: the chunk counts become exclusive prefixes (a contiguous run of chunks per wave, the
// waves' totals through LDS), and the category's bucket maxima are cleared
__global__ void __launch_bounds__(1024)
coco_scan_kernel(long long N, int nch, const int* __restrict__ counters, unsigned long long* __restrict__ cnt,
                 unsigned long long* __restrict__ bucket) {
    __shared__ unsigned s_tp[16][EVAL_LANES], s_fp[16][EVAL_LANES];
    const int k = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const EvalSeg seg = eval_segment(counters, k, N);
    for (int i = threadIdx.x; i < EVAL_LANES * EVAL_R; i += 1024) bucket[(size_t)k * EVAL_LANES * EVAL_R + i] = 0ull;
    int used = (int)((seg.n + EVAL_CHUNK - 1) / EVAL_CHUNK);
    used = used < nch ? used : nch;
    const int per = (used + 15) / 16, c0 = wave * per < used ? wave * per : used, c1 = c0 + per < used ? c0 + per : used;
    unsigned tp = 0, fp = 0;
    if (lane < EVAL_LANES) {
        for (int c = c0; c < c1; c++) {
            const unsigned long long v = cnt[((size_t)k * nch + c) * EVAL_LANES + lane];
            tp += (unsigned)v; fp += (unsigned)(v >> 32);
        }
        s_tp[wave][lane] = tp; s_fp[wave][lane] = fp;
    }
    __syncthreads();
    if (lane < EVAL_LANES) {
        tp = 0; fp = 0;
        for (int w = 0; w < wave; w++) { tp += s_tp[w][lane]; fp += s_fp[w][lane]; }
        for (int c = c0; c < c1; c++) {
            unsigned long long* p = cnt + ((size_t)k * nch + c) * EVAL_LANES + lane;
            const unsigned long long v = *p;
            *p = (unsigned long long)tp | ((unsigned long long)fp << 32);
            tp += (unsigned)v; fp += (unsigned)(v >> 32);
        }
    }
}

// one wave per (chunk, category): every true positive of lane (t, a) becomes pr = tp / (tp + fp + eps) and raises the maximum of
// its recall bucket b = the last level r with level_r <= tp / npig, found through need[a][r] = the least tp that reaches level r
__global__ void __launch_bounds__(64)
coco_emit_kernel(const long long* __restrict__ perm, const long long* __restrict__ rmatched, const long long* __restrict__ rignored,
                 long long N, int nch, const int* __restrict__ counters, const double* __restrict__ rec_thr,
                 const unsigned long long* __restrict__ cnt, unsigned long long* __restrict__ bucket) {
    __shared__ unsigned long long sm[64], si[64];
    __shared__ int need[EVAL_A][EVAL_R];
    const int k = blockIdx.x / nch, j = blockIdx.x - k * nch, lane = threadIdx.x;
    const EvalSeg seg = eval_segment(counters, k, N);
    const long long lo = (long long)j * EVAL_CHUNK;
    if (lo >= seg.n) return;
    const long long hi = lo + EVAL_CHUNK < seg.n ? lo + EVAL_CHUNK : seg.n;
    for (int e = lane; e < EVAL_A * EVAL_R; e += 64) {
        const int a = e / EVAL_R, r = e - a * EVAL_R;
        const int npig = counters[4 * k + a];
        int c = 0x7fffffff;                                              // never reached
        if (npig > 0) {
            const double lvl = rec_thr[r], np = (double)npig;
            const double guess = lvl * np;
            c = guess < 0.0 ? 0 : (guess > np ? npig : (int)guess);
            while (c > 0 && (double)(c - 1) / np >= lvl) c--;
            while (c <= npig && (double)c / np < lvl) c++;
        }
        need[a][r] = c;
    }
    const int a = lane & 3;
    const bool active = lane < EVAL_LANES && counters[4 * k + a] > 0;
    unsigned tp = 0, fp = 0;
    if (lane < EVAL_LANES) {
        const unsigned long long v = cnt[((size_t)k * nch + j) * EVAL_LANES + lane];
        tp = (unsigned)v; fp = (unsigned)(v >> 32);
    }
    unsigned long long* mine = bucket + ((size_t)k * EVAL_LANES + (lane < EVAL_LANES ? lane : 0)) * EVAL_R;
    int rn = 0, cur_b = -1;
    double cur = 0.0;
    for (long long i0 = lo; i0 < hi; i0 += 64) {
        const long long i = i0 + lane;
        unsigned long long mm = 0ull, ig = ~0ull;
        if (i < hi) {
            long long p = perm[seg.start + i];
            p = p < 0 ? 0 : (p < N ? p : N - 1);
            mm = (unsigned long long)rmatched[p]; ig = (unsigned long long)rignored[p];
        }
        __syncthreads();
        sm[lane] = mm; si[lane] = ig;
        __syncthreads();
        const int cnt64 = hi - i0 < 64 ? (int)(hi - i0) : 64;
        for (int q = 0; q < cnt64; q++) {
            const unsigned mb = (unsigned)(sm[q] >> lane) & 1u, ib = (unsigned)(si[q] >> lane) & 1u;
            fp += ~mb & ~ib & 1u;
            if (active && (mb & ~ib & 1u)) {
                tp++;
                while (rn < EVAL_R && need[a][rn] <= (int)tp) rn++;
                const double pr = (double)tp / ((double)(fp + tp) + 2.220446049250313e-16);
                if (rn - 1 != cur_b) {
                    if (cur_b >= 0) eval_atomic_max(mine + cur_b, __builtin_bit_cast(unsigned long long, cur));
                    cur_b = rn - 1; cur = pr;
                } else if (pr > cur) cur = pr;
            }
        }
    }
    if (cur_b >= 0) eval_atomic_max(mine + cur_b, __builtin_bit_cast(unsigned long long, cur));
}

// precision [10][101][K][4]: -1 where the cell has no non-ignored ground truth, else the maximum over the buckets >= r
__global__ void __launch_bounds__(64)
coco_finish_kernel(int K, const int* __restrict__ counters, const unsigned long long* __restrict__ bucket, double* __restrict__ precision) {
    const int k = blockIdx.x, lane = threadIdx.x;
    if (lane >= EVAL_LANES) return;
    const int t = lane >> 2, a = lane & 3;
    const bool have = counters[4 * k + a] > 0;
    const unsigned long long* mine = bucket + ((size_t)k * EVAL_LANES + lane) * EVAL_R;
    double run = 0.0;
    for (int r = EVAL_R - 1; r >= 0; r--) {
        const double v = __builtin_bit_cast(double, mine[r]);
        run = v > run ? v : run;
        precision[(((size_t)t * EVAL_R + r) * K + k) * EVAL_A + a] = have ? run : -1.0;
    }
}

// ---- recall ----------------------------------------------------------------------------------------------------------------------------------
// COCOeval's recall cell at maxDets m is tp_total / npig, tp_total = the true positives among the records whose rank inside their
// own (frame, category) list is below m: it does not depend on the global score order, so it needs neither the sort nor the scan.
// One wave per frame row (a wave walks the rows blockIdx.x, blockIdx.x + gridDim.x, ...).  Per row: the records per category are
// counted (LDS integer atomics), an exclusive prefix gives every category's first slot (a row holds its categories one after the
// other), and rank = slot - first slot.  Lane 4 t + a then owns column (t, a) of the wave's [3][K][40] counters in LDS: rank < 1,
// < 10, < 100 (each adds to its own and the wider cuts), true positive = matched & ~ignored.  The wave's totals go to the global
// table with 64-bit INTEGER atomics: sums of integers, the same bits whatever the grid and the arrival order.
// Every index is a slot below R or a category checked against [0, K): any key bits terminate in bounds.
__device__ __forceinline__ void eval_atomic_add(unsigned long long* p, unsigned long long v) {
#ifndef RVT_EMU
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

constexpr int EVAL_RECALL_GRID = 1024;   // waves of a launch at most: one flush of 120 K atomics each

__global__ void __launch_bounds__(64)
coco_recall_kernel(const long long* __restrict__ rkey, const long long* __restrict__ rmatched, const long long* __restrict__ rignored,
                   int F, int R, int K, unsigned long long* __restrict__ tp) {
    __shared__ int s_cnt[EVAL_MAX_NC], s_first[EVAL_MAX_NC];
    __shared__ unsigned s_tp[3][EVAL_MAX_NC][EVAL_LANES];
    __shared__ unsigned long long s_hit[64];
    __shared__ int s_cat[64], s_rank[64];
    const int lane = threadIdx.x;
    for (int e = lane; e < 3 * EVAL_MAX_NC * EVAL_LANES; e += 64) (&s_tp[0][0][0])[e] = 0u;
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        const size_t base = (size_t)f * R;
        if (lane < EVAL_MAX_NC) s_cnt[lane] = 0;
        __syncthreads();
        for (int i = lane; i < R; i += 64) {
            const long long key = rkey[base + i], c = key >> 32;
            if (key != EVAL_NO_RECORD && c >= 0 && c < K) atomicAdd(&s_cnt[(int)c], 1);
        }
        __syncthreads();
        if (lane < EVAL_MAX_NC) {
            int first = 0;
            for (int c = 0; c < lane; c++) first += s_cnt[c];
            s_first[lane] = first;
        }
        __syncthreads();
        for (int i0 = 0; i0 < R; i0 += 64) {
            const int i = i0 + lane;
            unsigned long long hit = 0ull;
            int cat = 0, rank = EVAL_TOP;
            if (i < R) {
                const long long key = rkey[base + i], c = key >> 32;
                if (key != EVAL_NO_RECORD && c >= 0 && c < K) {
                    cat = (int)c;
                    rank = i - s_first[cat];
                    if (rank >= 0 && rank < EVAL_TOP) hit = (unsigned long long)rmatched[base + i] & ~(unsigned long long)rignored[base + i];
                }
            }
            __syncthreads();
            s_hit[lane] = hit; s_cat[lane] = cat; s_rank[lane] = rank;
            __syncthreads();
            const int cnt64 = R - i0 < 64 ? R - i0 : 64;
            if (lane < EVAL_LANES)
                for (int q = 0; q < cnt64; q++) {
                    const unsigned long long h = s_hit[q];
                    if (h == 0ull) continue;                             // wave-uniform: no true positive in this record
                    if ((h >> lane) & 1ull) {
                        const int c = s_cat[q], r = s_rank[q];
                        s_tp[2][c][lane]++;
                        if (r < 10) s_tp[1][c][lane]++;
                        if (r < 1) s_tp[0][c][lane]++;
                    }
                }
        }
        __syncthreads();
    }
    __syncthreads();
    for (int e = lane; e < 3 * K * EVAL_LANES; e += 64) {
        const int m = e / (K * EVAL_LANES), rest = e - m * K * EVAL_LANES, k = rest / EVAL_LANES, l = rest - k * EVAL_LANES;
        const unsigned v = s_tp[m][k][l];
        if (v) eval_atomic_add(tp + e, (unsigned long long)v);
    }
}

}  // namespace rvt
