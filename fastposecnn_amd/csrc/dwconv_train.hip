// dwconv_train.hip — data and weight gradients of the depthwise 3x3 / pad 1 convolution of the MobileNetV2 encoder (mobilenet.hip's
// k_dwconv3x3 is the forward, in training too: act 0, scale 1, shift 0), for the training step: fpc_dwconv3x3_dgrad and
// fpc_dwconv3x3_wgrad.  Dense channel-last f32, C a multiple of 4, stride 1 or 2, lanes along the channel quads with 16-byte loads
// and stores, the weights torch's [C][1][3][3] read and written in place.  Plain f32 FMAs in an order the shape alone fixes, no
// atomics, no float division, no scratch: results are bit-identical run to run (DESIGN.md 4.2a''''''').
//
// Data gradient, stride 1: k_dwconv3x3_dgrad_s1, the forward's strip loop over dy with the taps flipped,
// dx[h][w] = sum dy[h + 1 - kh][w + 1 - kw] w[kh][kw]: one thread per (row, strip of 4 columns, channel quad), 3 x 6 quads of dy for
// 4 of dx, nine FMAs per output in ascending (row, column) order of dy.
//
// Data gradient, stride 2: k_dwconv3x3_dgrad_s2.  Per axis dx[2a] = dy[a] w[1], dx[2a + 1] = dy[a] w[2] + dy[a + 1] w[0], so the 2 x 2
// block of dx at (2a, 2b) takes dy[a..a+1][b..b+1] and 1 + 2 + 2 + 4 = 9 tap products per channel: no zero insertion.  One thread
// per (block row, strip of 2 blocks, channel quad): 2 x 3 quads of dy for 2 x 4 of dx; dy past Ho / Wo counts as zero, rows and
// columns of dx past Hi / Wi are not written.  Taps in ascending (kh, kw) order.
//
// Weight gradient: k_dwconv3x3_wgrad<S>, then k_dwconv3x3_wgrad_reduce.  The (frame, output row) list is cut into
// dw_wgrad_slices(B, Ho, Wo, C) contiguous slices; a workgroup takes one slice for a chunk of 8 channel quads (128 bytes of a
// pixel) on 32 pixel slots.  A slot takes the slice's (row, segment of 8 output columns) units u = slot, slot + 32, ... and walks a
// segment with the x columns sliding in registers: per output pixel one quad of dy and 3 (stride 2: 6) new quads of x for 36 FMAs
// into the thread's 4 channels x 9 taps.  The slots are added pairwise through LDS (slot s + h into slot s, h = 16 .. 1) and the
// workgroup writes ONE partial [slice][C][9]; the second launch adds the slices in double — sixteen contiguous ranges of slices,
// each in ascending order, then the ranges in ascending order — and writes OIHW.  x and dy leave memory once, plus the rows a
// slice shares with its neighbours (the workgroups of neighbouring slices run on one XCD: one L2).
#include <algorithm>

#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr long long kDwWalkLimit = (1LL << 32) - 4096LL * 256 - 8;      // mobilenet.hip's kWalkLimit: the 32-bit walks' bound

// ---- data gradient --------------------------------------------------------------------------------------------------------------

// dy, dx [B][H][W][C] (stride 1: one shape), w [C][1][3][3]; total = B H WT CQ items with WT strips of 4 columns per row
__global__ __launch_bounds__(256) void k_dwconv3x3_dgrad_s1(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dx, unsigned total, int H, int W, int WT, int CQ) {
    constexpr int TW = 4, NC = TW + 2;
    const int C = 4 * CQ;
    const XcdWalk wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned h = t % (unsigned)H, b = t / (unsigned)H;
        float wf[36];      // [channel of the quad][kh][kw]
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(w + 36 * (size_t)cq + 4 * i);
            wf[4 * i] = v[0]; wf[4 * i + 1] = v[1]; wf[4 * i + 2] = v[2]; wf[4 * i + 3] = v[3];
        }
        f32x4 acc[TW];
#pragma unroll
        for (int o = 0; o < TW; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int w0 = (int)wt * TW;
#pragma unroll
        for (int r = 0; r < 3; ++r) {      // the row of dy at h - 1 + r meets the tap row kh = 2 - r
            const int hy = (int)h - 1 + r;
            const bool rowok = hy >= 0 && hy < H;
            f32x4 d[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int wy = w0 - 1 + c;
                d[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (rowok && wy >= 0 && wy < W) d[c] = *reinterpret_cast<const f32x4*>(dy + (((size_t)b * H + hy) * W + wy) * C + 4 * cq);
            }
#pragma unroll
            for (int o = 0; o < TW; ++o)
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(d[o + s][j], wf[9 * j + 3 * (2 - r) + (2 - s)], acc[o][j]);
        }
#pragma unroll
        for (int o = 0; o < TW; ++o)
            if (w0 + o < W) *reinterpret_cast<f32x4*>(dx + (((size_t)b * H + h) * W + w0 + o) * C + 4 * cq) = acc[o];
    }
}

// dy [B][Ho][Wo][C], dx [B][Hi][Wi][C], Ho = (Hi - 1) / 2 + 1 block rows; total = B Ho WT CQ items with WT strips of 2 blocks
__global__ __launch_bounds__(256) void k_dwconv3x3_dgrad_s2(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dx, unsigned total, int Hi, int Wi, int Ho, int Wo,
                                                            int WT, int CQ) {
    constexpr int TB = 2;
    const int C = 4 * CQ;
    const XcdWalk wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned a = t % (unsigned)Ho, b = t / (unsigned)Ho;
        float wf[36];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(w + 36 * (size_t)cq + 4 * i);
            wf[4 * i] = v[0]; wf[4 * i + 1] = v[1]; wf[4 * i + 2] = v[2]; wf[4 * i + 3] = v[3];
        }
        const int b0 = (int)wt * TB;
        f32x4 d[2][TB + 1];
#pragma unroll
        for (int ry = 0; ry < 2; ++ry)
#pragma unroll
            for (int i = 0; i <= TB; ++i) {
                const int ya = (int)a + ry, xb = b0 + i;
                d[ry][i] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (ya < Ho && xb < Wo) d[ry][i] = *reinterpret_cast<const f32x4*>(dy + (((size_t)b * Ho + ya) * Wo + xb) * C + 4 * cq);
            }
        f32x4 acc[TB][4];      // [block][2 py + px]
#pragma unroll
        for (int i = 0; i < TB; ++i)
#pragma unroll
            for (int p = 0; p < 4; ++p) acc[i][p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                // the forward's tap k reaches dx of parity (k != 1) from dy at offset (k == 0)
                const int py = ky == 1 ? 0 : 1, ry = ky == 0 ? 1 : 0, px = kx == 1 ? 0 : 1, rx = kx == 0 ? 1 : 0;
#pragma unroll
                for (int i = 0; i < TB; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][2 * py + px][j] = fmaf(d[ry][i + rx][j], wf[9 * j + 3 * ky + kx], acc[i][2 * py + px][j]);
            }
#pragma unroll
        for (int py = 0; py < 2; ++py) {
            const int y = 2 * (int)a + py;
            if (y >= Hi) continue;
#pragma unroll
            for (int i = 0; i < TB; ++i)
#pragma unroll
                for (int px = 0; px < 2; ++px) {
                    const int x = 2 * (b0 + i) + px;
                    if (x < Wi) *reinterpret_cast<f32x4*>(dx + (((size_t)b * Hi + y) * Wi + x) * C + 4 * cq) = acc[i][2 * py + px];
                }
        }
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------

constexpr int kDwQuads = 8;                    // channel quads per workgroup: 128 bytes of a pixel
constexpr int kDwSlots = 256 / kDwQuads;       // pixel slots per workgroup
constexpr int kDwSeg = 8;                      // output columns of a unit
constexpr int kDwRanges = 16;                  // k_dwconv3x3_wgrad_reduce: contiguous ranges of slices per sum

struct DwWgradArgs {
    const float* x;       // [B][Hi][Wi][C]
    const float* dy;      // [B][Ho][Wo][C]
    float* part;          // [nslice][C][9]
    int B, Hi, Wi, Ho, Wo, C, CQ;
    int nchunk, nslice, nseg;
    unsigned blocks;      // nchunk * nslice
};

template <int S>
__global__ __launch_bounds__(256) void k_dwconv3x3_wgrad(const DwWgradArgs a) {
    __shared__ float red[36 * 128];
    // XCD-aware order: the workgroups of one XCD take a contiguous eighth of the (slice, chunk) list (the ids past it leave before
    // any barrier)
    unsigned bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (bid >= a.blocks) return;
    const int chunk = (int)(bid % (unsigned)a.nchunk), slice = (int)(bid / (unsigned)a.nchunk);
    const int tid = threadIdx.x, q = tid % kDwQuads, slot = tid / kDwQuads;
    const int qg = chunk * kDwQuads + q;
    const bool on = qg < a.CQ;
    const long long rows = (long long)a.B * a.Ho;
    const unsigned r0 = (unsigned)(slice * rows / a.nslice), r1 = (unsigned)((slice + 1) * rows / a.nslice);
    const unsigned units = (r1 - r0) * (unsigned)a.nseg;

    float acc[36];      // [channel of the quad][kh][kw]
#pragma unroll
    for (int k = 0; k < 36; ++k) acc[k] = 0.f;

    if (on) {
        const size_t C = (size_t)a.C;
#pragma unroll 1
        for (unsigned u = slot; u < units; u += kDwSlots) {
            const unsigned row = r0 + u / (unsigned)a.nseg;
            const int seg = (int)(u % (unsigned)a.nseg), b = (int)(row / (unsigned)a.Ho), ho = (int)(row % (unsigned)a.Ho);
            const int w0 = seg * kDwSeg, w1 = min(a.Wo, w0 + kDwSeg);
            const float* xr[3];
            bool rowok[3];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int hi = ho * S - 1 + kh;
                rowok[kh] = hi >= 0 && hi < a.Hi;
                xr[kh] = a.x + (((size_t)b * a.Hi + (rowok[kh] ? hi : 0)) * a.Wi) * C + 4 * (size_t)qg;
            }
            const float* dyr = a.dy + (((size_t)b * a.Ho + ho) * a.Wo) * C + 4 * (size_t)qg;
            auto col = [&](int kh, int wi) {
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (rowok[kh] && wi >= 0 && wi < a.Wi) v = *reinterpret_cast<const f32x4*>(xr[kh] + (size_t)wi * C);
                return v;
            };
            f32x4 xa[3], xb[3], xc[3];      // the columns under taps kw = 0, 1, 2
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                xa[kh] = col(kh, w0 * S - 1);
                if (S == 1) xb[kh] = col(kh, w0);
            }
#pragma unroll 1
            for (int wo = w0; wo < w1; ++wo) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + (size_t)wo * C);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    if (S == 2) xb[kh] = col(kh, 2 * wo);
                    xc[kh] = col(kh, wo * S + 1);
                }
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        acc[9 * j + 3 * kh] = fmaf(d[j], xa[kh][j], acc[9 * j + 3 * kh]);
                        acc[9 * j + 3 * kh + 1] = fmaf(d[j], xb[kh][j], acc[9 * j + 3 * kh + 1]);
                        acc[9 * j + 3 * kh + 2] = fmaf(d[j], xc[kh][j], acc[9 * j + 3 * kh + 2]);
                    }
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    if (S == 1) { xa[kh] = xb[kh]; xb[kh] = xc[kh]; }
                    else xa[kh] = xc[kh];
                }
            }
        }
    }

    // the pixel slots, pairwise in a fixed tree: slot s + h into slot s, h = 16 .. 1
#pragma unroll 1
    for (int h = kDwSlots / 2; h >= 1; h >>= 1) {
        if (slot >= h && slot < 2 * h) {
#pragma unroll
            for (int k = 0; k < 36; ++k) red[k * 128 + tid - h * kDwQuads] = acc[k];
        }
        __syncthreads();
        if (slot < h) {
#pragma unroll
            for (int k = 0; k < 36; ++k) acc[k] = acc[k] + red[k * 128 + tid];
        }
        __syncthreads();
    }
    if (slot != 0 || !on) return;
    float* dst = a.part + ((size_t)slice * a.C + 4 * (size_t)qg) * 9;      // 36 floats: (channel, tap)
#pragma unroll
    for (int k = 0; k < 9; ++k) *reinterpret_cast<f32x4*>(dst + 4 * k) = f32x4{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
}

// dw[i] = sum over the slices of part[slice][i], in double: thread (range r, quad i4) adds the slices of range r in ascending
// order, then the ranges are added in ascending order.  n4 float4 per slice; a workgroup takes 16 of them
__global__ __launch_bounds__(256) void k_dwconv3x3_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int n4, int nslice) {
    __shared__ double sh[kDwRanges][16][4];
    const int t = threadIdx.x, c = t & 15, r = t >> 4;
    const int i4 = blockIdx.x * 16 + c;
    const int s0 = (int)((long long)r * nslice / kDwRanges), s1 = (int)((long long)(r + 1) * nslice / kDwRanges);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (i4 < n4) {
#pragma unroll 8
        for (int sl = s0; sl < s1; ++sl) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(part + 4 * ((size_t)sl * n4 + i4));
            s[0] += (double)v[0]; s[1] += (double)v[1]; s[2] += (double)v[2]; s[3] += (double)v[3];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[r][c][e] = s[e];
    __syncthreads();
    if (r != 0 || i4 >= n4) return;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        double v = sh[0][c][e];
        for (int k = 1; k < kDwRanges; ++k) v += sh[k][c][e];
        o[e] = (float)v;
    }
    *reinterpret_cast<f32x4*>(dw + 4 * (size_t)i4) = o;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool dw_shape_ok(int B, int Hi, int Wi, int C, int stride) {
    return B >= 1 && Hi >= 1 && Wi >= 1 && C >= 4 && C % 4 == 0 && (stride == 1 || stride == 2) &&
           (long long)B * Hi * Wi * (C / 4) < kDwWalkLimit;      // every kernel's item count is at most this
}

// Slices of the weight gradient's (frame, output row) list, a function of (B, Ho, Wo, C) alone (include/fpc.h states it): enough
// for four workgroups per compute unit over the channel chunks, at most one per row, and no more than leave every slice 32 units
// (one per pixel slot) of 8 output columns.
int dw_wgrad_slices(int B, int Ho, int Wo, int C) {
    const long long rows = (long long)B * Ho, nseg = cdiv(Wo, kDwSeg), chunks = cdiv(C / 4, kDwQuads);
    long long n = std::max<long long>(1, 1024 / chunks);
    n = std::min(n, rows * nseg / kDwSlots);
    n = std::min(n, rows);
    return (int)std::max<long long>(1, n);
}

}  // namespace

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_dwconv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int stride,
                                   fpc_stream_t stream) {
    if (!dy || !w || !dx || !al16(dy) || !al16(w) || !al16(dx) || !dw_shape_ok(B, Hi, Wi, C, stride)) return FPC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {
        const int WT = cdiv(Wi, 4);
        const long long total = (long long)B * Hi * WT * (C / 4);
        hipLaunchKernelGGL(k_dwconv3x3_dgrad_s1, dim3(stream_grid(total)), dim3(256), 0, s, dy, w, dx, (unsigned)total, Hi, Wi, WT, C / 4);
    } else {
        const int Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1, WT = cdiv(Wo, 2);
        const long long total = (long long)B * Ho * WT * (C / 4);
        hipLaunchKernelGGL(k_dwconv3x3_dgrad_s2, dim3(stream_grid(total)), dim3(256), 0, s, dy, w, dx, (unsigned)total, Hi, Wi, Ho, Wo, WT, C / 4);
    }
    return check_launch();
}

// workspace: the slices' partials, [slices][C][9] floats (0: a shape the call refuses); the slice count is this size over 36 C
extern "C" size_t fpc_dwconv3x3_wgrad_workspace_bytes(int B, int Ho, int Wo, int C) {
    if (!dw_shape_ok(B, Ho, Wo, C, 1)) return 0;
    return (size_t)dw_wgrad_slices(B, Ho, Wo, C) * C * 9 * sizeof(float);
}

extern "C" int fpc_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int stride, void* ws,
                                   size_t ws_bytes, fpc_stream_t stream) {
    if (!x || !dy || !dw || !ws || !al16(x) || !al16(dy) || !al16(dw) || !dw_shape_ok(B, Hi, Wi, C, stride)) return FPC_EINVAL;
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    if (((uintptr_t)ws & 255) || ws_bytes < fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)) return FPC_EWORKSPACE;
    DwWgradArgs a;
    a.x = x; a.dy = dy; a.part = (float*)ws;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.C = C; a.CQ = C / 4;
    a.nchunk = cdiv(a.CQ, kDwQuads); a.nslice = dw_wgrad_slices(B, Ho, Wo, C); a.nseg = cdiv(Wo, kDwSeg);
    const long long blocks = (long long)a.nchunk * a.nslice;      // (at most max(nchunk, 1024))
    a.blocks = (unsigned)blocks;
    const unsigned grid = (unsigned)(blocks >= 8 ? (blocks + 7) / 8 * 8 : blocks);
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) hipLaunchKernelGGL(k_dwconv3x3_wgrad<1>, dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_dwconv3x3_wgrad<2>, dim3(grid), dim3(256), 0, s, a);
    int rc = check_launch();
    if (rc) return rc;
    const int n4 = C * 9 / 4;
    hipLaunchKernelGGL(k_dwconv3x3_wgrad_reduce, dim3(cdiv(n4, 16)), dim3(256), 0, s, (const float*)ws, dw, n4, a.nslice);
    return check_launch();
}
