// conv_device.hpp — device helpers shared by the convolution kernel files (conv_igemm.hip, wino_f32.hip, wino128.hip) and the
// streaming kernels (net_kernels.hip): vector types, buffer loads, the write-through pair, the packed / per-element f32 forms,
// the XCD-banded walk and the streaming launchers' grid.  (wino_tile.hpp keeps its own plain-C++ fma_s4 / sub_s4 / add_s4: see there.)
#pragma once
#include "net_kernels.hpp"

namespace fpc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));   // native vector: stays in registers (HIP's float4 struct copies can land in scratch)
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

// split_bf3 / pack_hi16: common.hpp (shared with conv_wgrad.hip)

// split_h2: common.hpp (shared with lateral.hip)

// raw buffer descriptor over [base, base + 2 GB): offsets are 32-bit, an offset >= 2^31 reads zeros without
// touching memory (measured, tools_dev/dma_vs_mfma.hip) — the zero fill of the convolution padding
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
__device__ __forceinline__ f32x4 buf_load4(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, 0));
}

// 16 bytes that another workgroup of the same launch reads (fused split-K): write-through stores / cache-bypassing loads
// at agent scope (sc1), so that neither side needs a whole-L2 write-back or invalidate; ordered by the drain + ticket
// of k_conv_igemm's epilogue.
typedef __attribute__((address_space(1))) unsigned long long gmem_u64;
__device__ __forceinline__ void store_wt128(float* p, f32x4 v) {
    const float a0 = v[0], a1 = v[1], a2 = v[2], a3 = v[3];      // (bit_cast of a vector ELEMENT expression misbehaves: scalars first)
    const unsigned long long lo = (unsigned long long)__builtin_bit_cast(unsigned, a0) | ((unsigned long long)__builtin_bit_cast(unsigned, a1) << 32);
    const unsigned long long hi = (unsigned long long)__builtin_bit_cast(unsigned, a2) | ((unsigned long long)__builtin_bit_cast(unsigned, a3) << 32);
    __hip_atomic_store((gmem_u64*)p, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store((gmem_u64*)p + 1, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ f32x4 load_wt128(const float* p) {
    const unsigned long long lo = __hip_atomic_load((gmem_u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long hi = __hip_atomic_load((gmem_u64*)p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return f32x4{__builtin_bit_cast(float, (unsigned)lo), __builtin_bit_cast(float, (unsigned)(lo >> 32)),
                 __builtin_bit_cast(float, (unsigned)hi), __builtin_bit_cast(float, (unsigned)(hi >> 32))};
}

// a - b as two v_pk_add_f32 with negated second operand (the compiler splits a vector subtraction into four
// v_sub_f32).  Same IEEE result as the scalar subtraction.
__device__ __forceinline__ f32x4 sub_pk(f32x4 a, f32x4 b) {
    f32x2 al = __builtin_shufflevector(a, a, 0, 1), ah = __builtin_shufflevector(a, a, 2, 3);
    f32x2 bl = __builtin_shufflevector(b, b, 0, 1), bh = __builtin_shufflevector(b, b, 2, 3);
    f32x2 rl, rh;
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(rl) : "v"(al), "v"(bl));
    asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(rh) : "v"(ah), "v"(bh));
    return __builtin_shufflevector(rl, rh, 0, 1, 2, 3);
}

// Scalar forms for code that runs between bf16 matrix instructions: there a packed f32 instruction costs more than the two
// scalar ones it replaces (MI355X_MICROARCH.md, "price of one filler beside MFMAs"), and the SLP vectorizer would pack
// plain C++ arithmetic again — hence inline asm, one instruction per element.  Same IEEE results as the packed forms.
__device__ __forceinline__ f32x4 sub_s4(f32x4 a, f32x4 b) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) { float x = a[k], y = b[k], z; asm("v_sub_f32 %0, %1, %2" : "=v"(z) : "v"(x), "v"(y)); r[k] = z; }
    return r;
}
__device__ __forceinline__ f32x4 add_s4(f32x4 a, f32x4 b) {
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) { float x = a[k], y = b[k], z; asm("v_add_f32 %0, %1, %2" : "=v"(z) : "v"(x), "v"(y)); r[k] = z; }
    return r;
}
__device__ __forceinline__ f32x4 fma_s4(float s, f32x4 b, f32x4 a) {      // s * b + a, fused
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) { float x = b[k], y = a[k], z; asm("v_fma_f32 %0, %1, %2, %3" : "=v"(z) : "v"(s), "v"(x), "v"(y)); r[k] = z; }
    return r;
}

// sigmoid and swish (v * sigmoid(v)) of the EfficientNet epilogues as one correctly rounded division each (common.hpp: div_ieee, never
// a compiler-expanded `/`).  v = 100: exp(-v) underflows, the results are 1 and v; v = -100: exp(-v) = inf, the results are 0 and -0.
__device__ __forceinline__ float sigmoid(float v) { return div_ieee(1.0f, 1.0f + expf(-v)); }
__device__ __forceinline__ float swish(float v) { return div_ieee(v, 1.0f + expf(-v)); }

// LDS operand rows are 32 floats (128 B) with NO padding: the 16-byte chunk c of row r lives in slot c ^ (r & 7), which
// keeps both the staging writes and the fragment reads conflict-free (8 consecutive rows hit 8 distinct slots of
// each half of the 64-bank window).  32 KB for the 64x64 tiling, 48 KB for 64x128 / 128x64 (36-float padded rows:
// 36.9 / 55.3 KB), i.e. room for 3 instead of 2 of the latter per CU.  (A fifth 64x64 workgroup per CU — registers
// squeezed to 96 — did not shorten the 1200-workgroup launches: their workgroups share the matrix pipe.)
constexpr int kLdsRow = kConvBK;

// The XCD-banded workgroup order.  Workgroups go to the 8 XCDs round-robin by linear id, and each XCD has its own L2; a kernel whose
// items read NEIGHBOURING rows (pooling windows, bilinear taps, the channel tiles of one pixel tile) then makes every L2 fetch every
// row.  With a grid that is a multiple of 8, XCD x = block % 8 works on the x-th contiguous eighth of the tile or item list with its
// own blocks, so a row is fetched by one L2 (two at a band border).  The contract:
//   - the grid is a multiple of 8 for the banded order (launchers: xcd_grid); any other grid runs in plain launch order;
//   - where the launcher rounded the grid up, a remapped id may lie past the list: the kernel compares it with the list's length,
//   - and such a workgroup leaves before any barrier (a kernel with a barrier and no such test launches its exact count).
// xcd_logical is a permutation of [0, grid); the spans of xcd_span over all blocks and slots visit [0, total) once each
// (tests/test_xcd_order_host.py through fpc_xcd_order).  A span is 32-bit: `first + k * step` must not wrap, so launchers keep
// total below kWalkLimit (common.hpp).
__host__ __device__ __forceinline__ unsigned xcd_banded(unsigned block, unsigned grid) { return (block & 7) * (grid >> 3) + (block >> 3); }      // grid % 8 == 0
__host__ __device__ __forceinline__ unsigned xcd_logical(unsigned block, unsigned grid) { return (grid & 7) == 0 ? xcd_banded(block, grid) : block; }
// The items of slot `slot` (of per_block per workgroup and step) of workgroup `block`: first, first + step, ... below end.  T is the
// caller's index type (unsigned; int in stem.hip, whose task arithmetic is signed).  The other four keep the caller's types: plain
// integers on the host, and in a kernel the four below, each READ WHERE IT IS USED, on the taken side of the test, as the hand-written
// walks read them (as values they are loaded in front of the test, and every walking kernel's instruction list changes).
struct XcdBlockDim { __device__ __forceinline__ operator unsigned() const { return blockDim.x; } };
struct XcdThreadIdx { __device__ __forceinline__ operator unsigned() const { return threadIdx.x; } };
struct XcdBlockIdx { __device__ __forceinline__ operator unsigned() const { return blockIdx.x; } };
struct XcdGridDim { __device__ __forceinline__ operator unsigned() const { return gridDim.x; } };
template <class T> struct XcdSpanT { T first, end, step; };
using XcdSpan = XcdSpanT<unsigned>;
template <class T, class P, class S, class B, class G>
__host__ __device__ __forceinline__ XcdSpanT<T> xcd_span(T total, P per_block, S slot, B block, G grid) {
    if ((grid & 7) != 0) return XcdSpanT<T>{(T)(block * per_block + slot), total, (T)(grid * per_block)};
    const T per = (total + 7) >> 3;
    const auto band = block & 7, turn = block >> 3;      // this workgroup's XCD and its place among that XCD's workgroups
    const T lo = (T)(band * per), hi = lo + per < total ? lo + per : total;      // (no min(): the host has none for unsigned)
    return XcdSpanT<T>{(T)(lo + turn * per_block + slot), hi, (T)((grid >> 3) * per_block)};
}
__device__ __forceinline__ unsigned xcd_block() { return xcd_logical(blockIdx.x, gridDim.x); }
// ... without the test, for a launcher that rounds EVERY grid up to a multiple of 8 (the grouped 3x3 family: with the test its stride-2
// sites measured 1 - 2.6 % slower, profiles/xcd_order_ledger.md)
__device__ __forceinline__ unsigned xcd_block_rounded() { return xcd_banded(blockIdx.x, gridDim.x); }
__device__ __forceinline__ XcdSpan xcd_walk(unsigned total) { return xcd_span(total, XcdBlockDim{}, XcdThreadIdx{}, XcdBlockIdx{}, XcdGridDim{}); }
template <class T>      // rpb rows a workgroup and step, this thread on row slot r of them
__device__ __forceinline__ XcdSpanT<T> xcd_rows(T total, T rpb, T r) { return xcd_span(total, rpb, r, XcdBlockIdx{}, XcdGridDim{}); }

// the launcher half: a grid of at least 8 workgroups rounded up to a multiple of 8, a smaller one as it is (plain order)
inline long long xcd_grid(long long blocks) { return blocks < 8 ? blocks : (blocks + 7) / 8 * 8; }

inline int stream_grid(long long work_items) {
    const long long g = (work_items + 255) / 256;
    return (int)xcd_grid(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

}  // namespace fpc
