// Token rows in MFMA-operand form (lane = row, 16 bytes of the row per k-step: piece (ks, half) = columns 16 ks + 8 half .. + 7) and
// their LayerNorm: statistics are an in-lane sum plus one exchange with lane ^ 32.  One row per lane (mc_*: the chained and streamed
// MLPs, dgrad + LayerNorm, LayerNorm + linear) or NB rows per lane (ab_*: the fused attention half, one row per 32-token block of
// the partition).  No kernel.
#pragma once
#include "common.hpp"
#include "opm.hpp"              // load_cols

namespace rvt {

// one token row per lane (row = tile * 32 + lane & 31) in operand form; LayerNorm in place
template <class T, int C>
__device__ __forceinline__ void mc_load_row(frag_t<T> (&f)[C / 16], const T* __restrict__ src, int row, bool valid, int half) {
#pragma unroll
    for (int ks = 0; ks < C / 16; ks++) {
        const frag_t<T> v = frag_load<T>(src + (size_t)(valid ? row : 0) * C + (2 * ks + half) * 8);
        const frag_t<T> z = frag_zero<T>();
        f[ks] = valid ? v : z;
    }
}
template <class T, int C>
__device__ __forceinline__ void mc_layernorm(const frag_t<T> (&xf)[C / 16], frag_t<T> (&uf)[C / 16], const float* k_lnw,
                                              const float* k_lnb, bool valid, int half, float eps, float& mean, float& rstd) {
    constexpr int KS = C / 16;
    float s = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int e = 0; e < 8; e++) s += (float)xf[ks][e];
    s += __shfl_xor(s, 32);
    mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ks++)
#pragma unroll
        for (int e = 0; e < 8; e++) { const float d = (float)xf[ks][e] - mean; q += d * d; }
    q += __shfl_xor(q, 32);
    rstd = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
    for (int ks = 0; ks < KS; ks++) {
        float w[8], bb[8];
        load_cols<8>(k_lnw, 16 * ks + 8 * half, w);
        load_cols<8>(k_lnb, 16 * ks + 8 * half, bb);
        frag_t<T> o;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] = (T)(valid ? ((float)xf[ks][e] - mean) * rstd * w[e] + bb[e] : 0.f);
        uf[ks] = o;
    }
}

// token rows of this lane (one per 32-token block of the partition) in operand form: piece (ks, half) = 16 bytes
template <class T, int C, int NB>
__device__ __forceinline__ void ab_load_rows(frag_t<T> (&f)[NB][C / 16], const T* __restrict__ src, const int (&tok)[NB],
                                              const bool (&valid)[NB], int half) {
#pragma unroll
    for (int b = 0; b < NB; b++)
#pragma unroll
        for (int ks = 0; ks < C / 16; ks++) {
            const frag_t<T> v = frag_load<T>(src + (size_t)tok[b] * C + (2 * ks + half) * 8);     // padded rows read token 0
            const frag_t<T> z = frag_zero<T>();
            f[b][ks] = valid[b] ? v : z;
        }
}

// LayerNorm (maxvit.py:229) of the rows held in operand form; keeps mean / rstd for the backward.  (mc_layernorm for each of the NB
// rows, written out: with a call per row hipcc emits different code for the attention kernels - tried, NOTES 5.1a.)
template <class T, int C, int NB>
__device__ __forceinline__ void ab_layernorm(const frag_t<T> (&xf)[NB][C / 16], frag_t<T> (&uf)[NB][C / 16], const float* k_lnw,
                                              const float* k_lnb, const bool (&valid)[NB], int half, float eps,
                                              float (&mean)[NB], float (&rstd)[NB]) {
    constexpr int KS = C / 16;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        float s = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
#pragma unroll
            for (int e = 0; e < 8; e++) s += (float)xf[b][ks][e];
        s += __shfl_xor(s, 32);
        mean[b] = s / (float)C;
        float q = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
#pragma unroll
            for (int e = 0; e < 8; e++) { const float d = (float)xf[b][ks][e] - mean[b]; q += d * d; }
        q += __shfl_xor(q, 32);
        rstd[b] = 1.0f / sqrtf(q / (float)C + eps);
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            float w[8], bb[8];
            load_cols<8>(k_lnw, 16 * ks + 8 * half, w);
            load_cols<8>(k_lnb, 16 * ks + 8 * half, bb);
#pragma unroll
            for (int e = 0; e < 8; e++)
                uf[b][ks][e] = (T)(valid[b] ? ((float)xf[b][ks][e] - mean[b]) * rstd[b] * w[e] + bb[e] : 0.f);
        }
    }
}

}  // namespace rvt
