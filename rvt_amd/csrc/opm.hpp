// The operand-major LDS matrix: [rows][K] stored as K / BK sub-tiles of [rows][128 bytes], 16-byte chunks XOR-swizzled like the GEMM
// tiles (common.hpp lds_chunk_off).  Weights and operand tiles of the fused MLP, the fused attention half, the chained MLP,
// dgrad + LayerNorm and the ConvLSTM scans all live in LDS in this form.
//
//   opm_subtile, opm_elem_ptr                     addressing
//   opm_store_frag, opm_load_frag                 one 8-element operand piece
//   acc_elem_off                                  the element under accumulator register r, from one per-lane base
//   opm_stage, opm_stage_weights                  a row-major global block -> operand matrix (the latter optionally with its
//                                                 32-column blocks in accumulator order)
//   ab_tr_frag, ab_acc_to_lds                     accumulator blocks written as row pieces and read back transposed
//   load_cols                                     N consecutive fp32 per-column constants (LDS or global) into registers
// No kernel.
#pragma once
#include "common.hpp"

namespace rvt {

template <class T> __device__ __forceinline__ char* opm_subtile(char* base, int rows, int kt) { return base + (size_t)kt * rows * 128; }

// store an 8-element fragment at (row, kcol0 = 8*fcg)
template <class T> __device__ __forceinline__ void opm_store_frag(char* base, int rows, int row, int fcg, const frag_t<T>& v) {
    constexpr int FPR = TileGeom<T>::FPR;
    tile_store_frag<T>(opm_subtile<T>(base, rows, fcg / FPR), row, fcg % FPR, v);
}

// address of element (row, kcol) of an LDS operand matrix [rows][K] (K-subtiles of [rows][128 B], swizzled 16-B chunks)
template <class T> __device__ __forceinline__ T* opm_elem_ptr(char* base, int rows, int row, int kcol) {
    constexpr int BK = TileGeom<T>::BK;
    const int kt = kcol / BK, kc = kcol % BK;
    const int byte = kc * (int)sizeof(T);
    return reinterpret_cast<T*>(base + (size_t)kt * rows * 128 + lds_chunk_off(row, byte >> 4) + (byte & 15));
}
template <class T> __device__ __forceinline__ frag_t<T> opm_load_frag(const char* base, int rows, int row, int fcg) {
    constexpr int FPR = TileGeom<T>::FPR;
    return tile_load_frag<T>(base + (size_t)(fcg / FPR) * rows * 128, row, fcg % FPR);
}

// LDS byte offset of element (R0 + rowc(r), ch) of a swizzled tile, r = accumulator register index of the 32x32 MFMA C/D
// layout, GIVEN the offset `base` of element (R0, ch) with R0 = 32*w + 4*(lane>>5): rowc(r) = (r&3) + 8*(r>>2) never
// carries out of the low five row bits, so the two swizzle terms of lds_chunk_off split into a per-lane part (already in
// `base`) XOR a function of r alone:  ((row>>1)&7) -> ((r>>1)&1) | ((r>>2)&1)<<2,  ((row>>4)&7) -> (r>>3).
// One v_xor plus an immediate offset per access instead of a dozen integer ops, and ONE register instead of sixteen.
__device__ __forceinline__ int acc_elem_off(int base, int r) {
    const int k = (((r >> 1) & 1) | (((r >> 2) & 1) << 2)) ^ ((r >> 3) & 1);
    return (base ^ (k << 4)) + ((r & 3) + 8 * (r >> 2)) * 128;
}

// stage a row-major global block [rows][kcols] (leading dimension ld elements) into an operand matrix; all 256 threads
template <class T> __device__ __forceinline__ void opm_stage(char* base, const T* g, int ld, int rows, int kcols, int tid) {
    const int fpr_g = kcols / 8;
    for (int f = tid; f < rows * fpr_g; f += 256) {
        const int row = f / fpr_g, fcg = f % fpr_g;
        opm_store_frag<T>(base, rows, row, fcg, frag_load<T>(g + (size_t)row * ld + fcg * 8));
    }
}

// stage a row-major [rows][K] weight matrix into an operand matrix, `nthreads` threads; PERM: the 32-column blocks are stored in
// accumulator order (position 16 q + 8 half + e holds column (e & 3) + 8 (2 q + (e >> 2)) + 4 half)
template <class T, int K, bool PERM>
__device__ __forceinline__ void opm_stage_weights(char* dst, const T* __restrict__ src, int rows, int tid, int nthreads) {
    constexpr int FPR = K / 8;
    for (int f = tid; f < rows * FPR; f += nthreads) {
        const int row = f / FPR, fcg = f % FPR;
        frag_t<T> v;
        if (!PERM) {
            v = frag_load<T>(src + (size_t)row * K + fcg * 8);
        } else {
            const int blk = fcg >> 2, q = (fcg >> 1) & 1, half = fcg & 1;
            const T* p = src + (size_t)row * K + blk * 32 + 16 * q + 4 * half;
#pragma unroll
            for (int e = 0; e < 4; e++) { v[e] = p[e]; v[4 + e] = p[8 + e]; }
        }
        opm_store_frag<T>(dst, rows, row, fcg, v);
    }
}

// Transposed operand piece in ACCUMULATOR order from a row-major LDS tile X[row][col] (opm layout, `rows` rows):
//   f[e] = X[row0 + (e & 3) + 8 (e >> 2) + 4 (lane >> 5)][col0 + (lane & 31)],  e = 0..7
// i.e. the operand "row = column col0 + lane&31, contraction over the 16 rows row0..row0+15" whose slot order matches
// accumulator registers 8 q .. 8 q + 7 of the other operand (row0 = 16 q within a 32-row block).
template <class T> __device__ __forceinline__ frag_t<T> ab_tr_frag(char* base, int rows, int row0, int col0, int lane) {
    if constexpr (sizeof(T) == 2) {
        const int rl = 4 * (lane >> 5) + ((lane & 15) >> 2), cl = col0 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
        return frag_from_tr<T>(reinterpret_cast<const bf16*>(opm_elem_ptr<T>(base, rows, row0 + rl, cl)),
                               reinterpret_cast<const bf16*>(opm_elem_ptr<T>(base, rows, row0 + rl + 8, cl)));
    } else {
        frag_t<T> f;
#pragma unroll
        for (int e = 0; e < 8; e++)
            f[e] = *opm_elem_ptr<T>(base, rows, row0 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), col0 + (lane & 31));
        return f;
    }
}

// write a T-form accumulator block (col = lane & 31 = LDS row, registers = 32 columns col0..col0+31) as 4-element row pieces
template <class T> __device__ __forceinline__ void ab_acc_to_lds(char* base, int rows, int row, int col0, const float (&v)[16], int half) {
    typedef __attribute__((ext_vector_type(4))) T vec4;
#pragma unroll
    for (int gq = 0; gq < 4; gq++) {
        vec4 t;
#pragma unroll
        for (int w = 0; w < 4; w++) t[w] = (T)v[4 * gq + w];
        *reinterpret_cast<vec4*>(opm_elem_ptr<T>(base, rows, row, col0 + 8 * gq + 4 * half)) = t;
    }
}

template <int N> __device__ __forceinline__ void load_cols(const float* p, int c0, float (&v)[N]) {
#pragma unroll
    for (int q = 0; q < N / 4; q++) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + c0 + q * 4);
        v[q * 4 + 0] = t[0]; v[q * 4 + 1] = t[1]; v[q * 4 + 2] = t[2]; v[q * 4 + 3] = t[3];
    }
}

}  // namespace rvt
