// Buffer-resource memory access and the LDS-DMA path (global -> LDS with buffer_load_dwordx4 ... lds, no loader registers), for
// every kernel that streams operands this way: the 256-wide GEMMs (ppgemm.hpp, ppgemm_tn.hpp), the streamed MLP (mlp_stream.hpp),
// LayerNorm + linear (ln_linear.hpp), the streamed ConvLSTM scan (lstm_scan3.hpp) and the exact-range resources and full-line row
// stores of line_bounce.hpp (attn_core2.hpp, stem.hpp).
//
//   pp_rsrc, pp_make_rsrc              a buffer descriptor over [base, base + bytes): loads beyond it return zeros, stores are dropped
//   pp_glds16, pp_load16, pp_store16   one 16-byte piece per lane: memory -> LDS, memory -> registers, registers -> memory
//   pp_wait_vm, pp_barrier, pp_wave_sync, pp_setprio        the counted waits and rendezvous of a load stream
//   ms_*                               the LDS image such a stream fills (sub-tiles of [rows][128 B], one swizzle term) and its reads
//
// Both forms of every primitive live here: the gfx950 builtins and the host emulator's (RVT_EMU).  No kernel.
#pragma once
#include "common.hpp"

namespace rvt {

#ifdef RVT_EMU
struct pp_rsrc { const char* base; unsigned bytes; };
__device__ __forceinline__ pp_rsrc pp_make_rsrc(const void* base, unsigned bytes) { return pp_rsrc{(const char*)base, bytes}; }
// one LDS-DMA piece: LDS[lds_off + 16 lane ..) = mem[voff + soff ..), zeros when out of range
__device__ __forceinline__ void pp_glds16(const pp_rsrc& rs, char* smem, int lds_off, int voff, int soff) {
    char* d = smem + lds_off + 16 * emu::g.cur->lane;
    const size_t o = (size_t)(unsigned)voff + (size_t)(unsigned)soff;
    if (o + 16 <= rs.bytes) memcpy(d, rs.base + o, 16);
    else memset(d, 0, 16);
}
__device__ __forceinline__ u32x4 pp_load16(const pp_rsrc& rs, int voff) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if ((size_t)(unsigned)voff + 16 <= rs.bytes) memcpy(&v, rs.base + (unsigned)voff, 16);
    return v;
}
__device__ __forceinline__ void pp_store16(const pp_rsrc& rs, int voff, const u32x4& v) {
    if ((size_t)(unsigned)voff + 16 <= rs.bytes) memcpy(const_cast<char*>(rs.base) + (unsigned)voff, &v, 16);
}
template <int N> __device__ __forceinline__ void pp_wait_vm() {}
__device__ __forceinline__ void pp_barrier() { __syncthreads(); }
__device__ __forceinline__ void pp_wave_sync() { emu::wave_barrier(); }
__device__ __forceinline__ void pp_setprio(int) {}
#else
typedef __amdgpu_buffer_rsrc_t pp_rsrc;
__device__ __forceinline__ pp_rsrc pp_make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void pp_glds16(const pp_rsrc& rs, char* smem, int lds_off, int voff, int soff) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (__attribute__((address_space(3))) void*)(smem + lds_off), 16, voff, soff, 0, 0);
}
__device__ __forceinline__ u32x4 pp_load16(const pp_rsrc& rs, int voff) { return __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0); }
__device__ __forceinline__ void pp_store16(const pp_rsrc& rs, int voff, const u32x4& v) { __builtin_amdgcn_raw_buffer_store_b128(v, rs, voff, 0, 0); }
template <int N> __device__ __forceinline__ void pp_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void pp_barrier() { __builtin_amdgcn_s_barrier(); }
__device__ __forceinline__ void pp_wave_sync() {}
#define pp_setprio(x) __builtin_amdgcn_s_setprio(x)
#endif

// LDS image of a streamed matrix chunk: sub-tiles of [rows][128 B] with the 16-byte chunk index XOR (row >> 1) & 7 — the first term of
// lds_chunk_off only.  (Its second term spreads the WRITES of the transposing loader; an LDS-DMA image has no such writer, and
// with it the swizzle of row 32 cb + li would depend on cb: one address register per (cb, chunk) instead of one per chunk.)
// A fragment address is (row * 128 + swz * 16) ^ (chunk * 16): a per-lane base XOR a compile-time constant.
__device__ __forceinline__ int ms_swz(int row) { return (row >> 1) & 7; }
__device__ __forceinline__ int ms_rowbase(int row) { return row * 128 + (ms_swz(row) << 4); }
// ... and the lane's half (k-slots 8 half .. of a k-step = fragment 2 ks + half) folded into the per-lane base as well: every
// fragment address of a lane is then ONE of a few registers (base ^ compile-time chunk) plus an immediate offset
template <class T> __device__ __forceinline__ int ms_rowbase_h(int row, int half) { return ms_rowbase(row) ^ ((half * TileGeom<T>::CPF) << 4); }
// fragment fcg (8 elements; the EVEN index 2 ks when `rb` comes from ms_rowbase_h) of the row whose base is `rb`, in a sub-tile
// array with `rows` rows per sub-tile
template <class T> __device__ __forceinline__ frag_t<T> ms_load_frag(const char* base, int rows, int rb, int fcg) {
    constexpr int FPR = TileGeom<T>::FPR, CPF = TileGeom<T>::CPF;
    const char* const t = base + (fcg / FPR) * rows * 128;
    frag_t<T> v;
    u32x4* dst = reinterpret_cast<u32x4*>(&v);
#pragma unroll
    for (int c = 0; c < CPF; c++) dst[c] = *reinterpret_cast<const u32x4*>(t + (rb ^ ((((fcg % FPR) * CPF + c)) << 4)));
    return v;
}
template <class T> __device__ __forceinline__ void ms_store_frag(char* base, int rows, int rb, int fcg, const frag_t<T>& v) {
    constexpr int FPR = TileGeom<T>::FPR, CPF = TileGeom<T>::CPF;
    char* const t = base + (fcg / FPR) * rows * 128;
    const u32x4* src = reinterpret_cast<const u32x4*>(&v);
#pragma unroll
    for (int c = 0; c < CPF; c++) *reinterpret_cast<u32x4*>(t + (rb ^ ((((fcg % FPR) * CPF + c)) << 4))) = src[c];
}
// per-lane source offsets (bytes) of this wave's LDS-DMA pieces: piece p = wave + i * WPB of a [rows][ld] matrix chunk whose
// LDS image is `subtiles` sub-tiles of [rows_per_subtile][128 B] (lane -> row 8 p' + lane / 8, chunk position lane % 8)
template <class T, int NPW, int WPB>
__device__ __forceinline__ void ms_piece_offsets(int (&v)[NPW], int wave, int lane, int rows_per_subtile, int ld) {
    constexpr int EPC = 16 / (int)sizeof(T);              // elements per 16-byte chunk
    const int rgs = rows_per_subtile / 8;                 // 1-KiB pieces per sub-tile
#pragma unroll
    for (int i = 0; i < NPW; i++) {
        const int p = wave + i * WPB, kt = p / rgs, r = (p % rgs) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ms_swz(r);
        v[i] = (r * ld + kt * TileGeom<T>::BK + c * EPC) * (int)sizeof(T);
    }
}

}  // namespace rvt
