// Shared pieces of the partitioned multi-head self-attention kernels (reference maxvit.py:343-354 on the partitions of
// maxvit.py:273-304): partition geometry / token addressing (AttnGeom, attn_token), operand-chunk loads (load_chunk), the
// 4-channel row store (store4), the in-lane column softmax (ab_softmax_cols) and the backward's P / dS scratch layout
// (AbBwdScratch).  No kernel: those are in attn_core2.hpp (attention core on a saved qkv tensor) and attn_block.hpp
// (fused attention half); the accumulator <-> operand conversions they chain products with are in acc_frags.hpp.
//
// The qkv activations stay in IMAGE token order [F*H*W][3C] (per-head channel layout [q|k|v], dh each — reference
// maxvit.py:347); window / grid partitioning is pure index arithmetic on the token rows that a partition gathers, so the
// reference's four permute().contiguous() copies per block never exist.
//
// MFMA formulation (L <= 96 tokens per partition, dh <= 32):
//   S^T = K Q^T        A = K rows (keys j), B = Q rows (queries i)  -> lane owns ONE query column i, its 16*NB accumulator
//                      registers run over keys  => softmax max / sum are in-lane reductions plus one exchange with lane^32.
//   O^T = V^T P^T      B = P^T straight from the accumulator registers: the MFMA pairs A's and B's k-slots one-to-one, so the
//                      keys are enumerated in the order the lane already holds them ( j = 32bj+16q+8(e>>2)+4*half+(e&3) ).
#pragma once
#include "common.hpp"

namespace rvt {

struct AttnGeom {
    int F, H, W, C, dh, heads, ph, pw, L, window;   // L = ph*pw
    int nPw;        // partitions along x
    int P;          // partitions per frame
    float scale;
    FastDiv dGroups, dP, dnPw, dpw;   // dGroups: head groups (of HG heads) per partition
};

// image-order token row of slot l of partition p of frame f
__device__ __forceinline__ int attn_token(const AttnGeom& g, int f, int p, int l) {
    uint32_t py, px, ly, lx;
    g.dnPw.divmod((uint32_t)p, py, px);
    g.dpw.divmod((uint32_t)l, ly, lx);
    int y, x;
    if (g.window) { y = py * g.ph + ly; x = px * g.pw + lx; }                  // maxvit.py:273-279
    else { y = ly * (g.H / g.ph) + py; x = lx * (g.W / g.pw) + px; }           // maxvit.py:290-296 (dilated grid)
    return (f * g.H + y) * g.W + x;
}

template <class T> __device__ __forceinline__ frag_t<T> load_chunk(const T* row, int chunk, int dh, bool valid) {
    // branch-free: padded rows point at token 0 (always mapped); the select zeroes what is not real
    const bool ok = valid & (chunk * 8 < dh);
    const frag_t<T> v = frag_load<T>(row + (ok ? chunk * 8 : 0));
    const frag_t<T> z = frag_zero<T>();
    return ok ? v : z;
}

// store 4 consecutive channels of one token row as ONE 8-byte (bf16) / 16-byte (f32) write
template <class T> __device__ __forceinline__ void store4(T* dst, float a, float b, float c, float d) {
    typedef __attribute__((ext_vector_type(4))) T vec4;
    vec4 v;
    v[0] = (T)a; v[1] = (T)b; v[2] = (T)c; v[3] = (T)d;
    *reinterpret_cast<vec4*>(dst) = v;
}

// S^T column softmax for one query block.  In: raw scores s[bj][r] (keys down the registers, this lane's query).  Out:
// p[bj][r] = exp(scale (s - max)) (UN-normalised) and the column's 1/sum.  Padded keys (j >= L) only exist in the LAST
// 32-key block: they are selected away by comparing the (compile-time) accumulator row of register r with one per-lane
// limit; exp2 with scale * log2(e) folded into one multiply.
template <int NB>
__device__ __forceinline__ float ab_softmax_cols(const f32x16 (&s)[NB], float (&p)[NB][16], int klim, float scale_log2e) {
    float mx = -3.0e38f;
#pragma unroll
    for (int bj = 0; bj < NB; bj++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float v = (bj == NB - 1 && ((r & 3) + 8 * (r >> 2)) >= klim) ? -1.0e30f : s[bj][r];
            p[bj][r] = v;
            mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    float sum = 0.f;
#pragma unroll
    for (int bj = 0; bj < NB; bj++)
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float e = fast_exp2((p[bj][r] - mx) * scale_log2e);
            p[bj][r] = e;
            sum += e;
        }
    sum += __shfl_xor(sum, 32);
    return 1.0f / sum;
}

// LDS scratch of the backward kernels (attn_block.hpp, attn_core2.hpp)
template <class T, int NB> struct AbBwdScratch {          // per wave: P and dS blocks [32 queries][32 NB keys]
    static constexpr int KTJ = 32 * NB * (int)sizeof(T) / 128 + ((32 * NB * (int)sizeof(T)) % 128 ? 1 : 0);
    static constexpr int ONE = KTJ * 32 * 128;
    static constexpr int BYTES = 2 * ONE;
};

}  // namespace rvt
