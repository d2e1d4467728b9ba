// conv_grouped_train.hip — data and weight gradients of the grouped 3x3 convolution of the ResNeXt encoders (conv_grouped.hip is
// the forward), for the training step: fpc_conv2d_grouped_dgrad and fpc_conv2d_grouped_wgrad.  Channel-last f32, C a multiple
// of 32, CG = C / groups in {4, 8, 16, 32, 64}, pad 1, stride 1 or 2.  Plain f32 products (v_fma_f32), a fixed summation order
// everywhere, no atomics: results are bit-identical run to run (DESIGN.md 4.2a'').
//
// Data gradient, stride 1: k_conv3x3_grouped itself over dy, on the image k_pack_grouped's mode 1 writes (the weights transposed
// inside each group and flipped, read straight from the OIHW tensor).
//
// Data gradient, stride 2: k_conv3x3_grouped_dgrad_s2<CG>.  Per axis dx[2a] = dy[a] w[1], dx[2a + 1] = dy[a] w[2] + dy[a + 1] w[0],
// so the 2 x 2 block of dx at (2a, 2b) takes dy[a..a+1][b..b+1] and 1 + 2 + 2 + 4 = 9 tap products per channel pair: the minimal
// multiply-add count, no zero insertion.  A workgroup takes 16 x 32 pixels of dx (8 x 16 blocks) x 32 channels and stages the 9 x 17
// window of dy (zero past Ho / Wo) with the forward's 36-float pixel pitch; a thread owns 4 consecutive channels of 4 consecutive
// blocks of a block row (64 accumulators), so every thread runs the same schedule: per quad of dy channels 10 dy float4 and 36
// weight float4 from LDS for 576 FMAs.  Summation order (pass, channel quad, ky, kx, channel).
//
// Weight gradient: k_conv3x3_grouped_wgrad<CG, STRIDE>, then k_wgrad_grouped_reduce.  A workgroup takes 32 output channels (CG =
// 64: and one half of the group's input channels) and a contiguous slice of the (frame, tile) list; per tile it stages the x window
// and the dy tile as the forward does.  A thread owns 4 output channels x 4 input channels x 9 taps (144 accumulators); 2 CG (CG
// >= 32: 64) threads cover the channel pairs and the other lanes and waves split the tile's pixels into 256 / pairs sub-slabs of
// whole row segments.  A step takes two pixels of a row: 2 dy float4 and 12 (stride 2: 15) x float4 for 288 FMAs.  At the end of
// its slice the workgroup adds its sub-slabs pairwise through LDS (a fixed tree) and writes ONE partial [slice][C][CG][9];
// k_wgrad_grouped_reduce adds the slices in slice order into OIHW (one slice: the workgroups write OIHW themselves).
#include <string.h>

#include <algorithm>

#include "conv_device.hpp"

#define FPC_TRY(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

namespace fpc {

namespace {

constexpr int kGtCC = 32;       // channels per workgroup
constexpr int kGtPix = 36;      // floats per LDS pixel: 32 channels + 4 of padding (conv_grouped.hip)
constexpr int kGtThreads = 256;

// ---- data gradient, stride 2 ---------------------------------------------------------------------------------------------

struct GrpDgradArgs {
    const float* dy;      // [B][Ho][Wo][C]
    const float* w;       // k_pack_grouped's mode-2 image
    float* dx;            // [B][Hi][Wi][C]
    int B, Hi, Wi, Ho, Wo, C;
    int tx, ty;           // tiles of 16 x 32 pixels of dx per frame
};

template <int CG>
struct DgGeom {
    static constexpr int KB = CG < 16 ? CG : 16, NPASS = CG / KB;
    static constexpr int BH = 8, BW = 16;                // 2 x 2 blocks of dx per tile
    static constexpr int DH = BH + 1, DW = BW + 1;       // the dy window
    static constexpr int IN_FLOATS = DH * DW * kGtPix, W_FLOATS = 9 * KB * kGtCC;
    static_assert((IN_FLOATS + W_FLOATS) * 4 <= 65536, "static LDS");
};

template <int CG>
__global__ __launch_bounds__(kGtThreads) void k_conv3x3_grouped_dgrad_s2(const GrpDgradArgs a) {
    using G = DgGeom<CG>;
    constexpr int KB = G::KB, DW = G::DW;
    __shared__ __attribute__((aligned(16))) float s_dy[G::IN_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_w[G::W_FLOATS];
    const int tid = threadIdx.x;
    // XCD-banded order, as k_conv3x3_grouped (the ids past the list leave before any barrier)
    const int bid = (int)xcd_block_rounded();
    const int nchunk = a.C / kGtCC;
    if (bid >= a.B * a.ty * a.tx * nchunk) return;
    const int chunk = bid % nchunk;
    int r = bid / nchunk;
    const int txi = r % a.tx; r /= a.tx;
    const int tyi = r % a.ty;
    const int b = r / a.ty;
    const int c0 = chunk * kGtCC;
    const int a0 = tyi * G::BH, b0 = txi * G::BW;      // the tile's first block = its first dy pixel
    const int q = tid & 7, pq = tid >> 3, brow = pq >> 2, bc = (pq & 3) * 4;
    const int kin = CG < 32 ? (4 * q / CG) * CG : 0;      // the thread's group inside the 32 staged channels

    f32x4 acc[4][4];      // [block][2 py + px]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[i][p] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* wimg = a.w + (size_t)chunk * G::NPASS * G::W_FLOATS;
    const float* dyb = a.dy + (long long)b * a.Ho * a.Wo * a.C;
#pragma unroll 1
    for (int pass = 0; pass < G::NPASS; ++pass) {
        if (pass > 0) __syncthreads();      // the previous pass is read out
        if ((pass * KB) % 32 == 0) {        // the window of the next 32 channels of dy (CG <= 32: once)
            const int cin0 = CG <= 32 ? c0 : (c0 / CG) * CG + pass * KB;
            for (int i = tid; i < G::DH * DW * 8; i += kGtThreads) {
                const int pix = i >> 3, c4 = i & 7, iy = pix / DW, ix = pix - iy * DW;
                const int gy = a0 + iy, gx = b0 + ix;
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (gy < a.Ho && gx < a.Wo)
                    v = *reinterpret_cast<const f32x4*>(dyb + ((long long)gy * a.Wo + gx) * a.C + cin0 + 4 * c4);
                *reinterpret_cast<f32x4*>(s_dy + pix * kGtPix + 4 * c4) = v;
            }
        }
        for (int i = tid; i < G::W_FLOATS / 4; i += kGtThreads)
            *reinterpret_cast<f32x4*>(s_w + 4 * i) = *reinterpret_cast<const f32x4*>(wimg + (size_t)pass * G::W_FLOATS + 4 * i);
        __syncthreads();
        const int koff = CG < 32 ? kin : (pass * KB) & 31;
        const float* dp = s_dy + (brow * DW + bc) * kGtPix + koff;
#pragma unroll 1
        for (int j = 0; j < KB / 4; ++j) {
            f32x4 d[2][5];
#pragma unroll
            for (int ry = 0; ry < 2; ++ry)
#pragma unroll
                for (int i = 0; i < 5; ++i) d[ry][i] = *reinterpret_cast<const f32x4*>(dp + (ry * DW + i) * kGtPix + 4 * j);
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    // the forward's tap k reaches dx of parity (k != 1) from dy at offset (k == 0)
                    const int py = ky == 1 ? 0 : 1, ry = ky == 0 ? 1 : 0, px = kx == 1 ? 0 : 1, rx = kx == 0 ? 1 : 0;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(s_w + ((ky * 3 + kx) * KB + 4 * j + c) * kGtCC + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float dv = d[ry][i + rx][c];
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[i][2 * py + px][e] = __builtin_fmaf(dv, w[e], acc[i][2 * py + px][e]);
                        }
                    }
                }
        }
    }

    const int c = c0 + 4 * q;
    float* dxb = a.dx + (long long)b * a.Hi * a.Wi * a.C + c;
#pragma unroll
    for (int py = 0; py < 2; ++py) {
        const int y = 2 * (a0 + brow) + py;
        if (y >= a.Hi) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int px = 0; px < 2; ++px) {
                const int x = 2 * (b0 + bc + i) + px;
                if (x < a.Wi) *reinterpret_cast<f32x4*>(dxb + ((long long)y * a.Wi + x) * a.C) = acc[i][2 * py + px];
            }
    }
}

template <int CG>
int launch_dgrad_s2_t(GrpDgradArgs a, hipStream_t s) {
    a.ty = cdiv(a.Hi, 2 * DgGeom<CG>::BH);
    a.tx = cdiv(a.Wi, 2 * DgGeom<CG>::BW);
    const long long blocks = (long long)a.B * a.ty * a.tx * (a.C / kGtCC);
    if (blocks < 1 || blocks > (1LL << 30)) return FPC_EINVAL;
    const unsigned grid = (unsigned)xcd_grid(blocks < 8 ? 8 : blocks);      // always banded: at least 8 workgroups
    hipLaunchKernelGGL((k_conv3x3_grouped_dgrad_s2<CG>), dim3(grid), dim3(kGtThreads), 0, s, a);
    return check_launch();
}

// ---- weight gradient -----------------------------------------------------------------------------------------------------

struct GrpWgradArgs {
    const float* x;       // pixel (b, y, x): x + b sb + y sh + x sw, its C channels contiguous
    const float* dy;      // [B][Ho][Wo][C]
    float* part;          // [nslice][C][CG][9] (nslice == 1: dw itself)
    long long sb, sh, sw;
    int B, Hi, Wi, Ho, Wo, C;
    int tx, ty, nslice;
};

template <int CG, int STRIDE>
struct WgGeom {
    static constexpr int TH = 8, TW = STRIDE == 1 ? 16 : 8;
    static constexpr int CGE = CG < 32 ? CG : 32;            // input channels of a group a workgroup takes
    static constexpr int HALVES = CG / CGE;                   // CG = 64: two workgroups per 32 output channels
    static constexpr int NQ = CGE / 4;                        // input-channel quads per output-channel quad
    static constexpr int PAIRS = 8 * NQ;                      // (output quad, input quad) pairs of a chunk
    static constexpr int PS = kGtThreads / PAIRS;             // pixel sub-slabs
    static constexpr int PPS = TH * TW / PS;                  // pixels of a tile per sub-slab
    static constexpr int SEG = PPS < TW ? PPS : TW;           // ... in row segments of SEG pixels
    static constexpr int NSEG = PPS / SEG;
    static constexpr int IH = (TH - 1) * STRIDE + 3, IW = (TW - 1) * STRIDE + 3;
    static constexpr int NXC = STRIDE + 3;                    // x columns under two pixels of a row
    static constexpr int X_FLOATS = IH * IW * kGtPix, DY_FLOATS = TH * TW * kGtPix;
    static_assert(SEG % 2 == 0 && TW % SEG == 0 && PPS % SEG == 0, "row segments of pixel pairs");
    static_assert(X_FLOATS >= 36 * 128, "the reduction's buffer lies over the x window");
    static_assert((X_FLOATS + DY_FLOATS) * 4 <= 65536, "static LDS");
};

template <int CG, int STRIDE>
__global__ __launch_bounds__(kGtThreads, 2) void k_conv3x3_grouped_wgrad(const GrpWgradArgs a) {
    using G = WgGeom<CG, STRIDE>;
    constexpr int TW = G::TW, IW = G::IW, NXC = G::NXC, PAIRS = G::PAIRS;
    __shared__ __attribute__((aligned(16))) float s_x[G::X_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_dy[G::DY_FLOATS];
    const int tid = threadIdx.x;
    const int nce = a.C / kGtCC * G::HALVES;
    const int ce = blockIdx.x % nce, slice = blockIdx.x / nce;
    const int chunk = ce / G::HALVES, half = ce % G::HALVES;
    const int c0 = chunk * kGtCC;
    const int cin0 = CG <= 32 ? c0 : (c0 / CG) * CG + half * 32;      // the 32 input channels staged
    const int pair = tid % PAIRS, split = tid / PAIRS;
    const int coq = pair / G::NQ, cq = pair % G::NQ;
    const int xoff = (CG < 32 ? (4 * coq / CG) * CG : 0) + 4 * cq;    // the thread's 4 input channels inside the staged 32

    float acc[4][4][9];      // [output channel][input channel][tap]
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int t = 0; t < 9; ++t) acc[o][i][t] = 0.f;

    const int ntile = a.B * a.ty * a.tx;
    const int t0 = (int)((long long)slice * ntile / a.nslice), t1 = (int)((long long)(slice + 1) * ntile / a.nslice);
#pragma unroll 1
    for (int tile = t0; tile < t1; ++tile) {
        const int txi = tile % a.tx;
        int r = tile / a.tx;
        const int tyi = r % a.ty;
        const int b = r / a.ty;
        const int oy0 = tyi * G::TH, ox0 = txi * TW;
        const int gy0 = oy0 * STRIDE - 1, gx0 = ox0 * STRIDE - 1;
        if (tile > t0) __syncthreads();      // the previous tile is read out
        const float* xb = a.x + (long long)b * a.sb + cin0;
        for (int i = tid; i < G::IH * IW * 8; i += kGtThreads) {
            const int pix = i >> 3, c4 = i & 7, iy = pix / IW, ix = pix - iy * IW;
            const int gy = gy0 + iy, gx = gx0 + ix;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
            if (gy >= 0 && gy < a.Hi && gx >= 0 && gx < a.Wi)
                v = *reinterpret_cast<const f32x4*>(xb + (long long)gy * a.sh + (long long)gx * a.sw + 4 * c4);
            *reinterpret_cast<f32x4*>(s_x + pix * kGtPix + 4 * c4) = v;
        }
        const float* dyb = a.dy + (long long)b * a.Ho * a.Wo * a.C + c0;
        for (int i = tid; i < G::TH * TW * 8; i += kGtThreads) {
            const int pix = i >> 3, c4 = i & 7, iy = pix / TW, ix = pix - iy * TW;
            const int gy = oy0 + iy, gx = ox0 + ix;
            f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};      // dy past the map: the pixel adds nothing
            if (gy < a.Ho && gx < a.Wo)
                v = *reinterpret_cast<const f32x4*>(dyb + ((long long)gy * a.Wo + gx) * a.C + 4 * c4);
            *reinterpret_cast<f32x4*>(s_dy + pix * kGtPix + 4 * c4) = v;
        }
        __syncthreads();
#pragma unroll 1
        for (int sg = 0; sg < G::NSEG; ++sg) {
            const int lin = split * G::PPS + sg * G::SEG, row = lin / TW, col0 = lin % TW;
#pragma unroll 1
            for (int st = 0; st < G::SEG; st += 2) {
                const int col = col0 + st;
                const float* xp = s_x + (row * STRIDE * IW + col * STRIDE) * kGtPix + xoff;
                const float* dp = s_dy + (row * TW + col) * kGtPix + 4 * coq;
                f32x4 xw[3][NXC], d[2];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int i = 0; i < NXC; ++i) xw[ky][i] = *reinterpret_cast<const f32x4*>(xp + (ky * IW + i) * kGtPix);
#pragma unroll
                for (int p = 0; p < 2; ++p) d[p] = *reinterpret_cast<const f32x4*>(dp + p * kGtPix);
#pragma unroll
                for (int p = 0; p < 2; ++p)
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                            for (int o = 0; o < 4; ++o)
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    acc[o][i][ky * 3 + kx] = __builtin_fmaf(d[p][o], xw[ky][p * STRIDE + kx][i], acc[o][i][ky * 3 + kx]);
            }
        }
    }

    // the sub-slabs, pairwise in a fixed tree: slab s + h into slab s, h = PS / 2 .. 1, 36 floats of a thread at a time
    __syncthreads();
    float* red = s_x;
#pragma unroll
    for (int h = G::PS / 2; h >= 1; h >>= 1) {
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            if (split >= h && split < 2 * h) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < 9; ++t) red[(i * 9 + t) * 128 + tid - h * PAIRS] = acc[o][i][t];
            }
            __syncthreads();
            if (split < h) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < 9; ++t) acc[o][i][t] = acc[o][i][t] + red[(i * 9 + t) * 128 + tid];
            }
            __syncthreads();
        }
    }
    if (split != 0) return;
    const int ci0 = half * 32 + 4 * cq;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        float* dst = a.part + (((size_t)slice * a.C + c0 + 4 * coq + o) * CG + ci0) * 9;      // 36 floats: (input channel, tap)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[o][(4 * k + e) / 9][(4 * k + e) % 9];
            *reinterpret_cast<f32x4*>(dst + 4 * k) = v;
        }
    }
}

// dw[i] = part[0][i] + part[1][i] + ... in slice order; n4 float4 per slice
__global__ __launch_bounds__(256) void k_wgrad_grouped_reduce(const float* __restrict__ part, float* __restrict__ dw, long long n4,
                                                              int nslice) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(part + 4 * i);
    for (int s = 1; s < nslice; ++s) v = v + *reinterpret_cast<const f32x4*>(part + 4 * ((long long)s * n4 + i));
    *reinterpret_cast<f32x4*>(dw + 4 * i) = v;
}

template <int CG, int STRIDE>
int launch_wgrad_t(GrpWgradArgs a, float* dw, hipStream_t s) {
    using G = WgGeom<CG, STRIDE>;
    const long long blocks = (long long)a.nslice * (a.C / kGtCC) * G::HALVES;
    if (blocks < 1 || blocks > (1LL << 30)) return FPC_EINVAL;
    if (a.nslice == 1) a.part = dw;
    hipLaunchKernelGGL((k_conv3x3_grouped_wgrad<CG, STRIDE>), dim3((unsigned)blocks), dim3(kGtThreads), 0, s, a);
    FPC_TRY(check_launch());
    if (a.nslice == 1) return FPC_OK;
    const long long n4 = (long long)a.C * CG * 9 / 4;
    hipLaunchKernelGGL(k_wgrad_grouped_reduce, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, a.part, dw, n4, a.nslice);
    return check_launch();
}

inline bool grouped_shape_ok(int C, int groups) {
    return C >= 32 && C % 32 == 0 && groups >= 1 && C % groups == 0 && grouped_cg_ok(C / groups);
}

// Slices of the weight gradient's (frame, tile) list: a function of the output map alone, so that the workspace size names it.
// Enough for two workgroups per compute unit (the kernel's occupancy), at most one per tile, and few enough that the partials
// stay under a quarter of the operand bytes (x is at least as large as dy): nslice C CG 36 <= 2 B Ho Wo C 4 / 4.
int wgrad_slices(int B, int Ho, int Wo, int C, int CG, int stride) {
    const long long ntile = (long long)B * cdiv(Ho, 8) * cdiv(Wo, stride == 1 ? 16 : 8);
    const long long nce = (long long)(C / kGtCC) * (CG > 32 ? 2 : 1);
    long long n = std::max<long long>(1, 512 / nce);
    n = std::min(n, 2LL * B * Ho * Wo / (36LL * CG));
    n = std::min(n, ntile);
    return (int)std::max<long long>(1, n);
}

}  // namespace

}  // namespace fpc

using namespace fpc;

// ---- stand-alone gradients of the grouped 3x3 convolution (lib/train_conv.py: _GroupedConv2dFn) -------------------------
// workspace: k_pack_grouped's image of the transposed weights, C * (C / groups) * 9 floats (0: a shape the call refuses)
extern "C" size_t fpc_conv2d_grouped_dgrad_workspace_bytes(int C, int groups) {
    if (!grouped_shape_ok(C, groups)) return 0;
    return std::max<size_t>(align_up((size_t)C * (C / groups) * 9 * sizeof(float), 256), 256);
}

extern "C" int fpc_conv2d_grouped_dgrad(const float* dy, const float* w_oihw, float* dx, int B, int Hi, int Wi, int C, int groups,
                                        int stride, void* ws, size_t ws_bytes, fpc_stream_t stream) {
    if (!dy || !w_oihw || !dx || !ws || B < 1 || Hi < 1 || Wi < 1 || !grouped_shape_ok(C, groups) || (stride != 1 && stride != 2))
        return FPC_EINVAL;
    if (!al16(dy) || !al16(w_oihw) || !al16(dx) || ((uintptr_t)ws & 255)) return FPC_EINVAL;
    if (ws_bytes < fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups)) return FPC_EINVAL;
    if ((long long)B * Hi * Wi * C >= (1LL << 40)) return FPC_EINVAL;
    const int CG = C / groups, Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    // (the launchers' workgroup limit, tested here so that nothing is packed for a request they would refuse: tiles of 8 x 16
    // pixels of dx at stride 1, 16 x 32 at stride 2)
    if ((long long)B * cdiv(Hi, stride == 1 ? 8 : 16) * cdiv(Wi, stride == 1 ? 16 : 32) * (C / kGtCC) > (1LL << 30)) return FPC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {      // the forward kernel over dy on the transposed, flipped image
        GroupedArgs g;
        memset(&g, 0, sizeof(g));
        g.in = dy; g.w = (const float*)ws; g.out = dx;
        g.in_sb = (long long)Hi * Wi * C; g.in_sh = (long long)Wi * C; g.in_sw = C;
        g.B = B; g.Hi = Hi; g.Wi = Wi; g.Ho = Hi; g.Wo = Wi; g.C = C; g.CG = CG; g.stride = 1;
        FPC_TRY(launch_pack_grouped(w_oihw, (float*)ws, C, CG, s, 1));
        return launch_conv3x3_grouped(g, s);
    }
    GrpDgradArgs a;
    memset(&a, 0, sizeof(a));
    a.dy = dy; a.w = (const float*)ws; a.dx = dx;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.C = C;
    FPC_TRY(launch_pack_grouped(w_oihw, (float*)ws, C, CG, s, 2));
    switch (CG) {
        case 4: return launch_dgrad_s2_t<4>(a, s);
        case 8: return launch_dgrad_s2_t<8>(a, s);
        case 16: return launch_dgrad_s2_t<16>(a, s);
        case 32: return launch_dgrad_s2_t<32>(a, s);
        case 64: return launch_dgrad_s2_t<64>(a, s);
    }
    return FPC_EINVAL;
}

// workspace: the slices' partials, [nslice][C][C / groups][9] floats (0: a shape the call refuses).  The slice count of a call is
// this size over C * (C / groups) * 36, or the call's tile count (8 x 16 output pixels at stride 1, 8 x 8 at stride 2) if that is less
extern "C" size_t fpc_conv2d_grouped_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int groups) {
    if (!grouped_shape_ok(C, groups) || B < 1 || Ho < 1 || Wo < 1) return 0;
    const int CG = C / groups;      // (stride 2 has the narrower tiles: its slice count is the larger of the two)
    return (size_t)wgrad_slices(B, Ho, Wo, C, CG, 2) * C * CG * 9 * sizeof(float);
}

extern "C" int fpc_conv2d_grouped_wgrad(const float* x, int64_t sb, int64_t sh, int64_t sw, const float* dy, float* dw, int B, int Hi,
                                        int Wi, int C, int groups, int stride, void* ws, size_t ws_bytes, fpc_stream_t stream) {
    if (!x || !dy || !dw || !ws || B < 1 || Hi < 1 || Wi < 1 || !grouped_shape_ok(C, groups) || (stride != 1 && stride != 2))
        return FPC_EINVAL;
    if (!al16(x) || !al16(dy) || !al16(dw) || ((uintptr_t)ws & 255)) return FPC_EINVAL;
    if ((sb | sh | sw) % 4 || sw < C || sb < 0 || sh < 0) return FPC_EINVAL;
    if ((long long)B * Hi * Wi * C >= (1LL << 40)) return FPC_EINVAL;
    const int CG = C / groups, Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    if (ws_bytes < fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups)) return FPC_EINVAL;
    GrpWgradArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.dy = dy; a.part = (float*)ws; a.sb = sb; a.sh = sh; a.sw = sw;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.C = C;
    a.ty = cdiv(Ho, 8); a.tx = cdiv(Wo, stride == 1 ? 16 : 8);
    if ((long long)B * a.ty * a.tx > (1LL << 30)) return FPC_EINVAL;
    a.nslice = wgrad_slices(B, Ho, Wo, C, CG, stride);
    hipStream_t s = (hipStream_t)stream;
#define FPC_GRP_CASE(cg)                                                                               \
    case cg: return stride == 1 ? launch_wgrad_t<cg, 1>(a, dw, s) : launch_wgrad_t<cg, 2>(a, dw, s);
    switch (CG) {
        FPC_GRP_CASE(4)
        FPC_GRP_CASE(8)
        FPC_GRP_CASE(16)
        FPC_GRP_CASE(32)
        FPC_GRP_CASE(64)
    }
#undef FPC_GRP_CASE
    return FPC_EINVAL;
}
