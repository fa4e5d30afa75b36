// Accumulator <-> operand conversions of the chained ("accumulator of one MFMA is the operand of the next") kernels: the fused
// attention half, the attention core, the chained / streamed MLPs, dgrad + LayerNorm, LayerNorm + linear and the ConvLSTM scans.
//
// C/D layout of a 32x32 MFMA block: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  Read as an A/B operand the same
// registers are "row = col, contraction over the rows in accumulator order": registers 8 q .. 8 q + 7 are k-step q of that operand.
//
//   acc_slot_frag, arr_slot_frag, acc_to_frags   accumulator registers (vector / array) -> operand pieces
//   acc_add_rows, acc_load_rows                  per-row constants added to / as the initial value of an accumulator block
//   make_identity_frags                          the identity operand: an MFMA against it transposes a piece block, exactly
//   wave_lds_sync                                LDS hand-off between the lanes of one wave
//   static_for                                   a loop whose index is a compile-time constant in the body
// No kernel.
#pragma once
#include <type_traits>
#include <utility>
#include "common.hpp"

namespace rvt {

// LDS hand-off between the lanes of ONE wave (private slice): DS operations of a wave execute in issue order, so draining
// lgkmcnt (plus a compiler barrier) is all the synchronisation there is to do — no s_barrier across the workgroup.
__device__ __forceinline__ void wave_lds_sync() {
#ifdef RVT_EMU
    emu::wave_barrier();          // emulator: lanes are fibers; the LDS hand-off is between the lanes of this wave only
#else
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}

template <class T> __device__ __forceinline__ frag_t<T> acc_slot_frag(const f32x16& a, int q) {
    frag_t<T> f;
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = (T)a[8 * q + e];
    return f;
}

template <class T> __device__ __forceinline__ frag_t<T> arr_slot_frag(const float (&a)[16], int q) {
    frag_t<T> f;
#pragma unroll
    for (int e = 0; e < 8; e++) f[e] = (T)a[8 * q + e];
    return f;
}

template <class T> __device__ __forceinline__ void acc_to_frags(const f32x16& a, frag_t<T> (&f)[2]) {
    f[0] = acc_slot_frag<T>(a, 0);
    f[1] = acc_slot_frag<T>(a, 1);
}

// per-row (= per accumulator register) additive constants of a T-form block: p points at the 32 values of the block
__device__ __forceinline__ void acc_add_rows(f32x16& c, const float* p, int half) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 8 * g + 4 * half);
#pragma unroll
        for (int w = 0; w < 4; w++) c[4 * g + w] += t[w];
    }
}
// ... and the same constants as the INITIAL value of the accumulator (bias folded into the first MFMA: no zero fill, no adds)
__device__ __forceinline__ void acc_load_rows(f32x16& c, const float* p, int half) {
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 8 * g + 4 * half);
#pragma unroll
        for (int w = 0; w < 4; w++) c[4 * g + w] = t[w];
    }
}

// identity operand pieces of a 32-column block: row n = lane & 31, k-step cc: 1 at slot k = 16 cc + 8 half + e == n
template <class T> __device__ __forceinline__ void make_identity_frags(frag_t<T> (&idf)[2], int li, int half) {
#pragma unroll
    for (int cc = 0; cc < 2; cc++)
#pragma unroll
        for (int e = 0; e < 8; e++) idf[cc][e] = (T)((16 * cc + 8 * half + e == li) ? 1.0f : 0.0f);
}

// f(std::integral_constant<int, 0>()), ..., f(std::integral_constant<int, N - 1>()): the body reads its index as decltype(i)::value
template <int... I, class F> __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>()), ...);
}
template <int N, class F> __device__ __forceinline__ void static_for(F&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

}  // namespace rvt
