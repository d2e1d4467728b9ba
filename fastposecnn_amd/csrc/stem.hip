// stem.hip — k_stem7x7: the encoder's 7x7 / stride-2 stem convolution (3 -> 64 channels, folded BatchNorm + ReLU; smp ResNetEncoder
// conv1 / bn1 / relu, F/lib/pose_regressor.py:709-743) as a weight-resident product for large batches.
//
// The implicit-GEMM kernel runs the stem as a 7x1 convolution over 8-pixel groups of the NHWC4 image (K = 7 rows x 8 taps x 4
// channels = 224, net.hip) on 128 x 64 tiles: every workgroup stages its own copy of the weight rows per K-step and splits its
// activation registers on the way into LDS — 650-810 us for a 32-frame batch whose matrix work is 170 us and whose output
// (630 MB) takes 115 us to write.  Here the WEIGHTS stay: a persistent workgroup of 8 waves copies the three bf16 planes
// k_pack_weight_bf3 already wrote ([plane][Npad][Kpad], k = (kh * 8 + tap) * 4 + channel) into LDS once, fragment-major
// ([k-group 14][plane 3][column tile 2][lane 64][16 bytes]: lane-linear, conflict-free ds_read_b128), and every wave walks
// 64-pixel segments of output rows: per kernel row and 4-tap group a lane fetches the two pixels of ITS output pixel's
// fragment straight from the image (2 x 16 bytes, neighbours overlap in L1), splits them into the three planes, and issues six
// v_mfma_f32_32x32x16_bf16 per 32-pixel half and 32-channel tile (the products p_i q_j with i + j <= 4: common.hpp) against B
// fragments read once per 64 pixels; the image loads run four k-groups ahead of their use.  Taps left / right of the image
// read as zero (a row outside the image likewise: predicated, not branched).  Epilogue: y = relu(acc * scale + shift), accumulator registers stored as they stand (one channel per lane, two
// full 128-byte lines per store instruction).  Bound: the matrix pipe (14 x 24 MFMAs per 64 pixels) beside ~2 300 vector
// instructions of loading and splitting per wave and tile.
// k_stem_pool_h3 (below) is the same product on two fp16 pieces with the 3x3 / stride-2 max-pool in its epilogue: split level 3.
#include <algorithm>
#include <type_traits>

#include "conv_device.hpp"

namespace fpc {

typedef float f32x3 __attribute__((ext_vector_type(3)));

constexpr int kStemKG = 14;                       // 16-deep k-groups: 7 kernel rows x (taps 0-3 | taps 4-7)
constexpr int kStemLds = kStemKG * 3 * 2 * 1024;  // bytes

__global__ __launch_bounds__(512, 1) void k_stem7x7(const StemArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_w[kStemLds];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, col = lane & 31, h = lane >> 5;
    // ---- weight planes -> LDS, fragment-major: chunk (kg, plane, nt, lane) = column nt * 32 + (lane & 31), k = 16 kg + 8 (lane >> 5) .. + 7
    for (int c = tid; c < kStemKG * 3 * 2 * 64; c += 512) {
        const int l = c & 63, nt = (c >> 6) & 1, pk = c >> 7, plane = pk % 3, kg = pk / 3;
        const unsigned short* src = a.wpl + ((size_t)plane * a.Npad + nt * 32 + (l & 31)) * a.Kpad + 16 * kg + 8 * (l >> 5);
        *reinterpret_cast<u32x4*>(&s_w[(size_t)c * 16]) = *reinterpret_cast<const u32x4*>(src);
    }
    float sc[2], sh[2];                             // this lane's two output channels (column tiles 0 / 1)
    sc[0] = a.scale ? a.scale[col] : 1.f; sc[1] = a.scale ? a.scale[32 + col] : 1.f;
    sh[0] = a.shift ? a.shift[col] : 0.f; sh[1] = a.shift ? a.shift[32 + col] : 0.f;
    __syncthreads();

    const int segs = a.Wo >> 6;                     // 64-pixel segments per output row
    const int ntile = a.B * a.Ho * segs;            // < 2^31: launch_stem7x7
    // XCD-banded walk (conv_device.hpp) of the tiles (row segments in raster order), a tile per wave: the 3.5 output rows that share
    // an input row are served by one L2
    const XcdSpanT<int> wk = xcd_rows(ntile, 8, wv);
    for (int tile = wk.first; tile < wk.end; tile += wk.step) {
        const int t2 = tile / segs, seg = tile - t2 * segs;
        const int b = t2 / a.Ho, oy = t2 - b * a.Ho;
        const int ox0 = seg * 64;
        const float* img = a.in + (size_t)b * a.Hi * a.Wi * 4;         // NHWC4 image (uniform)
        f32x16 acc[2][2];                                               // [32-pixel half][column tile]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[s][nt][i] = 0.f;
        // input x of this lane's first tap of k-group half g2 and pixel half s: 2 (ox0 + 32 s + col) - 3 + 4 g2 + 2 h
        const int ixb = 2 * (ox0 + col) - 3 + 2 * h;
        // The 14 k-groups (kernel row j / 2, taps 4 (j % 2) ..) run fully unrolled with the image loads kPre groups ahead of their use
        // (a group's loads take 1-2 us to land, its 24 MFMAs 0.3 us, and two waves share a SIMD): a ring of kPre x 4 sixteen-byte
        // registers, slot j % kPre refilled right after group j's split.  A kernel row above / below the image is predicated off
        // (its loads return zero and its MFMAs add nothing: 1.5 % of the rows of a 240-row output) instead of branched around, so the
        // whole tile is one basic block; the scheduling barriers keep the compiler from hoisting all 56 loads to the top.
        constexpr int kPre = 4;
        f32x4 ring[kPre][4];
        unsigned keep[kPre][4];                             // all ones / zero: the tap lies inside / outside the image
        // (loads are unconditional from a clamped address and masked at their use: a load under a lane predicate becomes a branch,
        // and with branches between them the compiler's wait counts fall back to vmcnt(0))
        auto issue = [&](int j, f32x4 (&r)[4], unsigned (&m)[4]) {
            const int kh = j >> 1, g2 = j & 1;
            const int iy = 2 * oy - 3 + kh;
            const bool rowok = iy >= 0 && iy < a.Hi;
            const float* rowp = img + (size_t)min(max(iy, 0), a.Hi - 1) * a.Wi * 4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ix = ixb + 64 * (q >> 1) + 4 * g2 + (q & 1);
                m[q] = (rowok && ix >= 0 && ix < a.Wi) ? 0xFFFFFFFFu : 0u;
                r[q] = *reinterpret_cast<const f32x4*>(rowp + (size_t)min(max(ix, 0), a.Wi - 1) * 4);
            }
        };
        auto masked = [](f32x4 v, unsigned m) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float x = v[e]; o[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & m); }
            return o;
        };
#pragma unroll
        for (int j = 0; j < kPre; ++j) issue(j, ring[j], keep[j]);
#pragma unroll
        for (int j = 0; j < kStemKG; ++j) {
            u32x4 A1[2], A2[2], A3[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                u32x2 p1, p2, p3, q1, q2, q3;
                split_bf3(masked(ring[j % kPre][2 * s], keep[j % kPre][2 * s]), p1, p2, p3);
                split_bf3(masked(ring[j % kPre][2 * s + 1], keep[j % kPre][2 * s + 1]), q1, q2, q3);
                A1[s] = u32x4{p1[0], p1[1], q1[0], q1[1]};
                A2[s] = u32x4{p2[0], p2[1], q2[0], q2[1]};
                A3[s] = u32x4{p3[0], p3[1], q3[0], q3[1]};
            }
            if (j + kPre < kStemKG) issue(j + kPre, ring[j % kPre], keep[j % kPre]);
            const unsigned char* wb = &s_w[(size_t)(j * 3 * 2) * 1024 + lane * 16];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const bf16x8 b1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wb + (0 * 2 + nt) * 1024));
                const bf16x8 b2 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wb + (1 * 2 + nt) * 1024));
                const bf16x8 b3 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wb + (2 * 2 + nt) * 1024));
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    f32x16 c = acc[s][nt];
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A3[s]), b1, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1[s]), b3, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A2[s]), b2, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A2[s]), b1, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1[s]), b2, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A1[s]), b1, c, 0, 0, 0);
                    acc[s][nt] = c;
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- epilogue: accumulator register i of half s = pixel ox0 + 32 s + 8 (i / 4) + (i % 4) + 4 h, channel nt * 32 + col
        float* orow = a.out + (((size_t)b * a.Ho + oy) * a.Wo + ox0 + 4 * h) * a.Cout + col;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float v = acc[s][nt][i] * sc[nt] + sh[nt];
                    if (a.relu) v = fmaxf(v, 0.f);
                    orow[(size_t)(32 * s + 8 * (i >> 2) + (i & 3)) * a.Cout + 32 * nt] = v;
                }
    }
}

// ------------------------------------------------------------------------------------------
// k_stem_pool_h3: the stem and its 3x3 / stride-2 / pad-1 max-pool in ONE launch, on three fp16 piece products.  The 240 x 320 x 64
// stem output of a 480 x 640 frame is never written: a wave walks DOWN a strip of 64 conv columns (32 pool columns) over a band of
// R pool rows (2 R + 1 conv rows), keeps 32 running maxima per lane and stores a pool row after every second conv row.
//   products   weights: k_pack_weight_h3's two fp16 planes (same k order as above), 57 KB of LDS; activations: split_h2;
//              acc += A2 B1 + A1 B2 + A1 B1 on v_mfma_f32_32x32x16_f16, 1 / s (a power of two) folded into the BN multiplier.
//   pooling    after ReLU every value is >= 0, so padding and the running maximum start at 0.  In the accumulator layout a lane
//              owns a channel and 4 consecutive pixels of every group of 8: the pool columns 4 G + 2 h and 4 G + 2 h + 1 are
//              v_max3 of its own registers and ONE value of lane ^ 32 (the neighbouring four pixels' last).
//   halo       pool column 32 s needs conv column 64 s - 1 of the strip to the left.  It is RECOMPUTED, batched over the band's
//              rows: before its walk a wave runs one 32-pixel tile whose pixels are (conv row y0 + m, column 64 s - 1), m < 2 R + 1
//              <= 32, and parks the 32 x 64 results in a wave-private LDS slot (8 KB) — no barrier, no neighbour to wait for, and
//              84 matrix instructions against the walk's 3 528 (2.4 %).  launch_stem_pool_h3 counts what is computed twice.
//   loads      as k_stem7x7: unconditional from clamped addresses, masked at use, four k-groups ahead — here across conv rows too
//              (the body is a pair of rows, 28 groups, so a ring slot keeps its static register).
constexpr int kSpLdsW = kStemKG * 2 * 2 * 1024;     // weight image, bytes
constexpr int kSpHaloRows = 32;

// k_stem_pool_h3's halo tile: conv column ox0 - 1 of rows y0 .. y0 + 31 (lane's pixel = row y0 + col) -> halo[row][channel] after
// BN + ReLU.  Its own function (not inlined): the walk's registers are allocated without it.
__device__ __attribute__((noinline)) void stem_pool_halo(const char* img, const unsigned char* s_w, float* halo, int y0, int ox0, int Hi,
                                                         unsigned rowB, float sc0, float sc1, float sh0, float sh1) {
    const int lane = threadIdx.x & 63, col = lane & 31, h = lane >> 5;
    const float sc[2] = {sc0, sc1}, sh[2] = {sh0, sh1};
    float m1 = -1.f;
    asm volatile("" : "+s"(m1));
    auto masked = [](f32x3 v, unsigned m) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 3; ++e) { const float x = v[e]; o[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & m); }
        o[3] = 0.f;
        return o;
    };
                const int iyb = 2 * (y0 + col) - 3;
                const int ixh = 2 * (ox0 - 1) - 3 + 2 * h;      // > 0 and < Wi - 8: no column mask
                f32x16 hacc[2];
    #pragma unroll
                for (int nt = 0; nt < 2; ++nt)
    #pragma unroll
                    for (int i = 0; i < 16; ++i) hacc[nt][i] = 0.f;
                constexpr int kPreH = 4;
                f32x3 hr[kPreH][2];
                unsigned hk[kPreH];
                auto hissue = [&](int j, f32x3 (&r)[2], unsigned& m) {
                    const int kh = j >> 1, g2 = j & 1, iy = iyb + kh;
                    m = (iy >= 0 && iy < Hi) ? 0xFFFFFFFFu : 0u;
                    const unsigned off = (unsigned)min(max(iy, 0), Hi - 1) * rowB + (unsigned)(ixh + 4 * g2) * 16u;
                    r[0] = *reinterpret_cast<const f32x3*>(img + off);
                    r[1] = *reinterpret_cast<const f32x3*>(img + off + 16u);
                };
    #pragma unroll
                for (int j = 0; j < kPreH; ++j) hissue(j, hr[j], hk[j]);
    #pragma unroll
                for (int j = 0; j < kStemKG; ++j) {
                    u32x2 p1, p2, q1, q2;
                    split_h2(masked(hr[j % kPreH][0], hk[j % kPreH]), m1, p1, p2);
                    split_h2(masked(hr[j % kPreH][1], hk[j % kPreH]), m1, q1, q2);
                    const u32x4 A1 = u32x4{p1[0], p1[1], q1[0], q1[1]}, A2 = u32x4{p2[0], p2[1], q2[0], q2[1]};
                    if (j + kPreH < kStemKG) hissue(j + kPreH, hr[j % kPreH], hk[j % kPreH]);
                    const unsigned char* wb = &s_w[(size_t)(j * 2 * 2) * 1024 + lane * 16];
    #pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const f16x8 b1 = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(wb + (0 * 2 + nt) * 1024));
                        const f16x8 b2 = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(wb + (1 * 2 + nt) * 1024));
                        f32x16 c = hacc[nt];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A2), b1, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A1), b2, c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A1), b1, c, 0, 0, 0);
                        hacc[nt] = c;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
    #pragma unroll
                for (int nt = 0; nt < 2; ++nt)
    #pragma unroll
                    for (int i = 0; i < 16; ++i)
                        halo[(8 * (i >> 2) + (i & 3) + 4 * h) * 64 + 32 * nt + col] = fmaxf(hacc[nt][i] * sc[nt] + sh[nt], 0.f);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(512, 1) void k_stem_pool_h3(const StemPoolArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_w[kSpLdsW];
    __shared__ float s_halo[8][kSpHaloRows][64];
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the task, its rows and every row address are wave-uniform
    for (int c = tid; c < kStemKG * 2 * 2 * 64; c += 512) {
        const int l = c & 63, nt = (c >> 6) & 1, pk = c >> 7, plane = pk & 1, kg = pk >> 1;
        const unsigned short* src = a.wpl + ((size_t)plane * a.Npad + nt * 32 + (l & 31)) * a.Kpad + 16 * kg + 8 * (l >> 5);
        *reinterpret_cast<u32x4*>(&s_w[(size_t)c * 16]) = *reinterpret_cast<const u32x4*>(src);
    }
    // 1 / s of the weight image sits behind its two planes; a power of two, so folding it into the BN multiplier is exact
    const float isc = reinterpret_cast<const float*>(a.wpl)[(size_t)a.Npad * a.Kpad];
    float sc[2], sh[2];
    sc[0] = (a.scale ? a.scale[col] : 1.f) * isc; sc[1] = (a.scale ? a.scale[32 + col] : 1.f) * isc;
    sh[0] = a.shift ? a.shift[col] : 0.f; sh[1] = a.shift ? a.shift[32 + col] : 0.f;
    float m1 = -1.f;
    asm volatile("" : "+s"(m1));      // split_h2's -1 in a scalar register
    __syncthreads();

    const int strips = a.Wo >> 6, bands = (a.Hp + a.band - 1) / a.band;
    const int ntask = a.B * bands * strips;           // < 2^31: launch_stem_pool_h3
    const XcdSpanT<int> wk = xcd_rows(ntask, 8, wv);      // XCD-banded walk, as k_stem7x7
    const unsigned rowB = (unsigned)a.Wi * 16u;       // bytes of an image row
    // a pixel is loaded as its three real channels (the fourth of the NHWC4 image is zero: a constant, not a register)
    auto masked = [](f32x3 v, unsigned m) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 3; ++e) { const float x = v[e]; o[e] = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & m); }
        o[3] = 0.f;
        return o;
    };
    float* halo = &s_halo[wv][0][0];
    for (int task = wk.first; task < wk.end; task += wk.step) {
        const int t2 = task / strips, strip = task - t2 * strips;
        const int b = t2 / bands, band = t2 - b * bands;
        const int r0 = band * a.band, nr = min(a.band, a.Hp - r0);
        const int y0 = 2 * r0 - 1;                    // first conv row of the band (-1: above the image, skipped)
        const int ox0 = strip * 64;
        const char* img = reinterpret_cast<const char*>(a.in + (size_t)b * a.Hi * a.Wi * 4);
        // ---- the left neighbour's last conv column for every row of the band -> LDS (rows y0 + m; m = this lane's pixel)
        if (strip > 0) stem_pool_halo(img, s_w, halo, y0, ox0, a.Hi, rowB, sc[0], sc[1], sh[0], sh[1]);
        else {
#pragma unroll
            for (int i = 0; i < kSpHaloRows * 64 / 256; ++i) *reinterpret_cast<f32x4*>(&halo[(i * 64 + lane) * 4]) = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // ---- column offsets (bytes) and masks of this lane's 8 taps: fixed for the whole walk.  index = 4 s + 2 g2 + tap
        unsigned xoff[8], xm[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int ix = 2 * (ox0 + col) - 3 + 2 * h + 64 * (k >> 2) + 4 * ((k >> 1) & 1) + (k & 1);
            xm[k] = (ix >= 0 && ix < a.Wi) ? 0xFFFFFFFFu : 0u;
            xoff[k] = (unsigned)min(max(ix, 0), a.Wi - 1) * 16u;
        }
        constexpr int kPre = 4;
        f32x3 ring[kPre][4];
        // k-group j of conv row y -> ring slot `slot`
        auto issue = [&](int y, int j, f32x3 (&r)[4]) {
            const int kh = j >> 1, g2 = j & 1;
            const unsigned ro = (unsigned)min(max(2 * y - 3 + kh, 0), a.Hi - 1) * rowB;      // wave-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = *reinterpret_cast<const f32x3*>(img + (ro + xoff[4 * (q >> 1) + 2 * g2 + (q & 1)]));
        };
        const unsigned olane = (unsigned)(2 * h * 64 + col) * 4u;      // this lane's byte offset inside a pool row's strip
        float run[2][16];                             // running maxima: [column tile][pool column 2 G + k of this lane]
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int i = 0; i < 16; ++i) run[nt][i] = 0.f;
        // one conv row: 14 k-groups from ring slots (j + SL) % 4, the next groups requested (row yn once this row's are out), then
        // BN + ReLU, the horizontal 3-tap maxima and their place in the vertical one
        auto conv_row = [&](auto Mc, int y, int yn, int prow) {
            constexpr int MODE = decltype(Mc)::value;      // 0: the band's first row, 1: an even row, 2: an odd row (closes pool row `prow`)
            constexpr int SL = MODE == 1 ? 2 : 0;          // ring phase: 14 groups per row, 4 slots
            // conv pixel ox0 - 1 of this row for the two column tiles (strip 0: zeros, the pool's padding).  Read here, unconditionally:
            // a conditional read inside the epilogue cost the loop 60 spilled registers
            float hlv[2];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) hlv[nt] = halo[(y - y0) * 64 + 32 * nt + col];
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc[2][2];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[s][nt][i] = 0.f;
#pragma unroll
            for (int j = 0; j < kStemKG; ++j) {
                const int slot = (j + SL) % kPre;
                const int kh = j >> 1, g2 = j & 1;
                const int iy = 2 * y - 3 + kh;
                const unsigned rm = (iy >= 0 && iy < a.Hi) ? 0xFFFFFFFFu : 0u;      // wave-uniform
                const unsigned char* wb = &s_w[(size_t)(j * 2 * 2) * 1024 + lane * 16];
                f16x8 bw[2][2];      // [plane][column tile]
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    bw[0][nt] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(wb + (0 * 2 + nt) * 1024));
                    bw[1][nt] = __builtin_bit_cast(f16x8, *reinterpret_cast<const u32x4*>(wb + (1 * 2 + nt) * 1024));
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {      // (one half's pieces at a time: 8 operand registers live, not 16)
                    u32x2 p1, p2, q1, q2;
                    split_h2(masked(ring[slot][2 * s], xm[4 * s + 2 * g2] & rm), m1, p1, p2);
                    split_h2(masked(ring[slot][2 * s + 1], xm[4 * s + 2 * g2 + 1] & rm), m1, q1, q2);
                    const u32x4 A1 = u32x4{p1[0], p1[1], q1[0], q1[1]}, A2 = u32x4{p2[0], p2[1], q2[0], q2[1]};
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        f32x16 c = acc[s][nt];
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A2), bw[0][nt], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A1), bw[1][nt], c, 0, 0, 0);
                        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A1), bw[0][nt], c, 0, 0, 0);
                        acc[s][nt] = c;
                    }
                }
                if (j + kPre < kStemKG) issue(y, j + kPre, ring[slot]);
                else issue(yn, j + kPre - kStemKG, ring[slot]);
                __builtin_amdgcn_sched_barrier(0);
            }
            // register i of half s = conv pixel 32 s + 8 (i / 4) + (i % 4) + 4 h: group G = 4 s + i / 4 holds pixels 8 G + 4 h + (i % 4).
            // Each horizontal maximum goes straight into the running maximum (and, on a closing row, out): no second array
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                float recv[8];
#pragma unroll
                for (int G = 0; G < 8; ++G)
                    recv[G] = __shfl_xor(fmaxf(acc[G >> 2][nt][4 * (G & 3) + 3] * sc[nt] + sh[nt], 0.f), 32, 64);
                const float hl = hlv[nt];
#pragma unroll
                for (int G = 0; G < 8; ++G) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[G >> 2][nt][4 * (G & 3) + e] * sc[nt] + sh[nt], 0.f);
                    // pool column 4 G + 2 h: pixels 8 G + 4 h - 1 .. + 1; pool column 4 G + 2 h + 1: pixels 8 G + 4 h + 1 .. + 3
                    const float left = h ? recv[G] : (G ? recv[G ? G - 1 : 0] : hl);
                    const float hm0 = fmaxf(fmaxf(v[0], v[1]), left), hm1 = fmaxf(fmaxf(v[1], v[2]), v[3]);
                    if (MODE == 2) {      // closes pool row `prow` ...
                        // (a wave-uniform row base + one lane offset + immediates: 32 separate addresses would not fit the registers)
                        char* ob = reinterpret_cast<char*>(a.out + (((size_t)b * a.Hp + prow) * a.Wp + 32 * strip) * 64) + olane;
                        float* o = reinterpret_cast<float*>(ob) + (4 * G) * 64 + 32 * nt;
                        o[0] = fmaxf(run[nt][2 * G], hm0);
                        o[64] = fmaxf(run[nt][2 * G + 1], hm1);
                    }
                    if (MODE == 0) {      // the band's first row (row -1 of the first band: every tap masked, its relu(shift) is no input)
                        run[nt][2 * G] = y >= 0 ? hm0 : 0.f;
                        run[nt][2 * G + 1] = y >= 0 ? hm1 : 0.f;
                    } else if (MODE == 2) {      // ... and opens the next
                        run[nt][2 * G] = hm0;
                        run[nt][2 * G + 1] = hm1;
                    } else {
                        run[nt][2 * G] = fmaxf(run[nt][2 * G], hm0);
                        run[nt][2 * G + 1] = fmaxf(run[nt][2 * G + 1], hm1);
                    }
                    __builtin_amdgcn_sched_barrier(0);      // (group by group: scheduled as one block the 64 BN results are all live at once)
                }
            }
        };
        // conv row y0 opens pool row r0; then per pool row r0 + p the even row y0 + 2 p + 1 and the odd row y0 + 2 p + 2, which closes it
#pragma unroll
        for (int j = 0; j < kPre; ++j) issue(y0, j, ring[j]);
        conv_row(std::integral_constant<int, 0>{}, y0, y0 + 1, 0);
        for (int p = 0; p < nr; ++p) {
            conv_row(std::integral_constant<int, 1>{}, y0 + 2 * p + 1, y0 + 2 * p + 2, 0);
            conv_row(std::integral_constant<int, 2>{}, y0 + 2 * p + 2, y0 + 2 * p + 3, r0 + p);
        }
    }
}

// bands x strips of one frame and the conv outputs the launch computes beyond Ho x Wo (per frame): the band overlap rows and the
// halo tiles.  Host arithmetic only (tests/test_stem_pool_tasks.py reads it through fpc_stem_pool_tasks).
void stem_pool_tasks(int Ho, int Wo, int band, long long out4[4]) {
    const int Hp = Ho / 2, strips = Wo / 64, bands = (Hp + band - 1) / band;
    long long rows = 0;
    for (int bd = 0; bd < bands; ++bd) {
        const int r0 = bd * band, nr = std::min(band, Hp - r0);
        rows += 2 * nr + 1 - (r0 == 0 ? 1 : 0);      // conv rows 2 r0 - 1 .. 2 (r0 + nr) - 1 inside the image
    }
    out4[0] = bands; out4[1] = strips;
    out4[2] = rows * Wo + (long long)bands * (strips - 1) * 32;      // conv outputs computed
    out4[3] = (long long)Ho * Wo;                                    // conv outputs that exist
}

int launch_stem_pool_h3(const StemPoolArgs& a, hipStream_t s) {
    if (!a.in || !a.wpl || !a.out || a.B < 1 || !a.relu || a.Npad < 64 || a.Kpad != 224 || (a.Wo & 63) != 0 || a.Ho < 2 || (a.Ho & 1) ||
        a.Ho != (a.Hi + 6 - 7) / 2 + 1 || a.Wo != (a.Wi + 6 - 7) / 2 + 1 || a.Hp != a.Ho / 2 || a.Wp != a.Wo / 2 ||
        a.band < 1 || 2 * a.band + 1 > kSpHaloRows || (long long)a.Hi * a.Wi * 16 >= (1LL << 31))
        return FPC_EINVAL;
    const long long tasks = (long long)a.B * ((a.Hp + a.band - 1) / a.band) * (a.Wo >> 6);
    if (tasks >= (1LL << 31) - 8 * 4096) return FPC_EINVAL;
    const int grid = (int)std::min<long long>(a.grid > 0 ? a.grid : 256, (tasks + 7) / 8);
    hipLaunchKernelGGL(k_stem_pool_h3, dim3(grid), dim3(512), 0, s, a);
    return check_launch();
}

int launch_stem7x7(const StemArgs& a, hipStream_t s) {
    if (!a.in || !a.wpl || !a.out || a.B < 1 || a.Cout != 64 || a.Npad < 64 || a.Kpad != 224 || (a.Wo & 63) != 0 || a.Ho < 1 ||
        a.Ho != (a.Hi + 6 - 7) / 2 + 1 || a.Wo != (a.Wi + 6 - 7) / 2 + 1 || (long long)a.Hi * a.Wi * 4 >= (1LL << 31))
        return FPC_EINVAL;
    const long long waves = (long long)a.B * a.Ho * (a.Wo >> 6);
    if (waves >= (1LL << 31) - 8 * 4096) return FPC_EINVAL;
    const int grid = (int)std::min<long long>(a.grid > 0 ? a.grid : 256, (waves + 7) / 8);
    hipLaunchKernelGGL(k_stem7x7, dim3(grid), dim3(512), 0, s, a);
    return check_launch();
}

}  // namespace fpc
