// vgg_train.hip — the training step's two VGG pieces no other file expresses (lib/backbone.py VGGEncoder under autograd; lib/train_conv.py:
// _VggConv0Fn, _MaxPool2x2Fn): the weight and bias gradient of features.0 (3 -> 64 channels, 3x3 / stride 1 / pad 1, at full resolution)
// and the backward of MaxPool2d(2, 2).  The forward halves are the inference kernels of vgg.hip (k_conv3x3_c3, k_maxpool2x2), unchanged.
// f32 throughout, no atomics, a summation order that is a function of the shape alone: two launches agree bit for bit.  No kernel
// divides a float.  Workgroups walk in the XCD-banded order of the other streaming kernels.
//
// k_c3_wgrad + k_c3_wgrad_reduce:
//   dw[co][ci][kh][kw] = sum over b, y, x of dy[b][y][x][co] * img[b][y + kh - 1][x + kw - 1][ci]      (zero outside the image)
//   db[co]             = sum over b, y, x of dy[b][y][x][co]
// As a GEMM: M = 64 output channels, K = the pixels, N = 48 columns, column n = 4 tap + c with tap = 3 kh + kw: 9 taps x 4 channels =
// 36 columns, 27 of them weights.  The image's fourth channel never enters a result: it is replaced by 0 while staging (a zero
// weight would not do: NaN x 0 is NaN), and the lanes of column 19 — the centre tap's fourth channel — feed the constant 1 instead of
// what they read, which makes that column db: dy is read once for both.  Columns 36 .. 47 and the other fourth channels are computed
// and never read.  dy is 256 bytes a pixel against 16 of image, so the kernel has to be bound by reading dy: at B = 8, 640 x 480 that
// is 629 MB, 126 us at 5 TB/s; v_mfma_f32_16x16x4_f32 (exact f32 products, 64 FLOP a clock and SIMD) on N = 48 issues
// 2 * 64 * 48 * 2 457 600 = 15.1 GFLOP for 8.5 useful, 96 us at the matrix peak (N = 64 on 32 x 32 x 2 tiles: 20.1 GFLOP, 128 us —
// over the read).
// A unit is (frame, row, 64-pixel segment); a workgroup of 4 waves walks a contiguous slice of the unit list — wave m owns output
// channels 16 m .. 16 m + 15 and all three 16-column tiles: three accumulators of four registers — and writes ONE partial [64][48]
// at the end of its slice.  Per unit the workgroup stages
//   the 64 x 64 dy tile (zeros past the row's end) in rows of 80 floats, so that the four pixels of an A fragment fall into four
//     different quarters of the banks, and
//   the 3 image rows under the segment, 64 + 2 pixels of 16 bytes each (zeros outside the image: the loads are from a clamped address
//     and a select zeroes them — predicated, not branched),
// and issues 16 K-steps of 3 MFMAs per wave: A = dy[px][co] (lane l: pixel 4 ks + (l >> 4), channel 16 m + (l & 15)), B = the image
// word (kh, px + kw, c) of the lane's column (three lane constants, + 16 floats a K-step).  The next unit's global loads (5 float4 per
// thread) are in flight under the current unit's MFMAs.
// k_c3_wgrad_reduce adds the partials in slice order, in double, and writes OIHW [64][3][3][3] and [64].
//
// k_maxpool2x2_bwd: windows do not overlap, so a dx element belongs to one window: it is dy of the window where it is the arg-max by
// torch's rule — the FIRST maximum in row-major order (val > max) — and 0 elsewhere.  The arg-max is recomputed from x (no index plane
// is kept).  One thread per (window, channel quad), 16-byte accesses: four loads of x, one of dy, four stores — every dx element is
// written, no zero fill.  Inputs are finite: NaN (and infinities) are outside the contract.
#include <string.h>

#include <algorithm>

#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr int kCwThreads = 256;               // 4 waves: one per 16 output channels
constexpr int kCwSeg = 64;                    // pixels of a unit
constexpr int kCwDyRow = 80;                  // floats of a staged dy pixel: 64 channels + 16 of padding
constexpr int kCwRowPx = kCwSeg + 2;          // image pixels under a segment
constexpr int kCwRowF = kCwRowPx * 4;         // ... floats
constexpr int kCwImg4 = 3 * kCwRowPx;         // float4 of the image stage (198)
constexpr int kCwN = 48;                      // columns of a partial
constexpr int kCwDbCol = 19;                  // the centre tap's fourth channel: the bias gradient
constexpr int kCwMinUnits = 8;                // units per slice at least: a partial (12 KB) costs less than one unit's operands
constexpr int kCwMaxSlices = 1024;            // four workgroups per compute unit
constexpr int kCwOut = 64 * 27 + 64;          // dw and db elements: 56 * 32

struct C3WgradArgs {
    const float* img;     // [B][H][W][4]
    const float* dy;      // [B][H][W][64]
    float* part;          // [nslice][64][48]
    int B, H, W, nseg, nunit, nslice;
};

__global__ __launch_bounds__(kCwThreads) void k_c3_wgrad(const C3WgradArgs a) {
    __shared__ __attribute__((aligned(16))) float s_dy[kCwSeg * kCwDyRow];
    __shared__ __attribute__((aligned(16))) float s_im[kCwImg4 * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int m = __builtin_amdgcn_readfirstlane(tid >> 6);
    // XCD-banded order (conv_device.hpp) over the slices (the grid is nslice): neighbouring rows of the image and of dy in one L2
    const int slice = (int)xcd_block();
    const int u0 = (int)((long long)slice * a.nunit / a.nslice), u1 = (int)((long long)(slice + 1) * a.nunit / a.nslice);
    const int per_frame = a.H * a.nseg;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x4 acc[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) acc[t] = zero;

    f32x4 rd[4], ri = zero;
    auto load = [&](int u) {
        const int b = u / per_frame, r = u - b * per_frame;
        const int y = r / a.nseg, x0 = (r - y * a.nseg) * kCwSeg;
        const float* dyr = a.dy + ((long long)b * a.H + y) * a.W * 64;
        const float* imb = a.img + (long long)b * a.H * a.W * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tid + kCwThreads * j;      // < 1024: pixel i >> 4, channel quad i & 15
            const int px = x0 + (i >> 4);
            const f32x4 v = *reinterpret_cast<const f32x4*>(dyr + (long long)min(px, a.W - 1) * 64 + 4 * (i & 15));
            rd[j] = px < a.W ? v : zero;
        }
        if (tid < kCwImg4) {
            const int row = tid / kCwRowPx, xi = tid - row * kCwRowPx;
            const int iy = y - 1 + row, ix = x0 - 1 + xi;
            f32x4 v = *reinterpret_cast<const f32x4*>(imb + ((long long)min(max(iy, 0), a.H - 1) * a.W + min(max(ix, 0), a.W - 1)) * 4);
            v[3] = 0.f;      // the fourth channel, whatever it holds
            ri = (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) ? v : zero;
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = tid + kCwThreads * j;
            *reinterpret_cast<f32x4*>(s_dy + (i >> 4) * kCwDyRow + 4 * (i & 15)) = rd[j];
        }
        if (tid < kCwImg4) *reinterpret_cast<f32x4*>(s_im + tid * 4) = ri;
    };

    // the lane's fragments: A = dy[pixel 4 ks + kq][channel 16 m + j], B = column 16 t + j at that pixel
    const int j = lane & 15, kq = lane >> 4;
    const float* pa = s_dy + kq * kCwDyRow + 16 * m + j;
    const float* pb[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int tap = min(4 * t + (j >> 2), 8);      // (columns 36 .. 47: any word of the stage; never read afterwards)
        const int kh = tap / 3, kw = tap - 3 * kh;
        pb[t] = s_im + kh * kCwRowF + (kq + kw) * 4 + (j & 3);
    }
    const bool db_col = j == kCwDbCol - 16;      // tile 1's lanes of column 19

    if (u0 < u1) load(u0);
#pragma unroll 1
    for (int u = u0; u < u1; ++u) {
        store();
        __syncthreads();
        if (u + 1 < u1) load(u + 1);
#pragma unroll
        for (int ks = 0; ks < kCwSeg / 4; ++ks) {
            const float av = pa[4 * ks * kCwDyRow];
            const float b0 = pb[0][16 * ks], b1r = pb[1][16 * ks], b2 = pb[2][16 * ks];
            const float b1 = db_col ? 1.0f : b1r;
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b1, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b2, acc[2], 0, 0, 0);
        }
        __syncthreads();      // the stage is read out
    }

    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg
    float* out = a.part + (size_t)slice * 64 * kCwN + (size_t)(16 * m + 4 * kq) * kCwN + j;
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[r * kCwN + 16 * t] = acc[t][r];
}

// Element o < 1728: dw[co][ci][kh][kw] = sum over the slices, in slice order, of part[slice][co][4 (3 kh + kw) + ci]; element
// 1728 + co: db[co] = ... of part[slice][co][19] (db NULL: skipped).  32 elements per workgroup; eight threads per element take the
// eighths of the slice list (in double), thread 0 of them adds the eight in order.
__global__ __launch_bounds__(256) void k_c3_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                         int nslice) {
    __shared__ double s_sum[8][32];
    const int jj = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int o = blockIdx.x * 32 + jj;      // < 1792 = 56 * 32
    const bool bias = o >= 64 * 27;
    const int ob = bias ? 0 : o;
    const int co = bias ? o - 64 * 27 : ob / 27, r = ob - (ob / 27) * 27, ci = r / 9, tap = r - ci * 9;
    const float* src = part + (size_t)co * kCwN + (bias ? kCwDbCol : 4 * tap + ci);
    const int per = (nslice + 7) >> 3, s0 = sub * per, s1 = min(nslice, s0 + per);
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += (double)src[(size_t)s * 64 * kCwN];
    s_sum[sub][jj] = acc;
    __syncthreads();
    if (sub == 0) {
#pragma unroll
        for (int k = 1; k < 8; ++k) acc += s_sum[k][jj];
        if (!bias) dw[o] = (float)acc;
        else if (db) db[co] = (float)acc;
    }
}

// x, dx [B][H][W][C], dy [B][H / 2][W / 2][C]; items = B (H / 2) (W / 2) (C / 4): item g is dy's channel quad g
__global__ __launch_bounds__(256) void k_maxpool2x2_bwd(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                        unsigned items, int Wo, int C) {
    const unsigned C4 = (unsigned)C >> 2;
    const XcdSpan wk = xcd_walk(items);      // < kWalkLimit: fpc_maxpool2x2_bwd
    const size_t row = (size_t)2 * Wo * C;   // one input row
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned c4 = g % C4;
        unsigned r = g / C4;
        const unsigned wo = r % (unsigned)Wo; r /= (unsigned)Wo;      // r = b Ho + ho: input row 2 r of the batch's rows
        const size_t off = (size_t)2 * r * row + (size_t)2 * wo * C + 4 * c4;
        const float* p = x + off;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + C);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(p + row), v3 = *reinterpret_cast<const f32x4*>(p + row + C);
        const f32x4 q = *reinterpret_cast<const f32x4*>(dy + (size_t)g * 4);
        f32x4 d0, d1, d2, d3;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float best = v0[e];
            int am = 0;
            bool w = v1[e] > best; best = w ? v1[e] : best; am = w ? 1 : am;
            w = v2[e] > best; best = w ? v2[e] : best; am = w ? 2 : am;
            w = v3[e] > best; am = w ? 3 : am;
            d0[e] = am == 0 ? q[e] : 0.f;
            d1[e] = am == 1 ? q[e] : 0.f;
            d2[e] = am == 2 ? q[e] : 0.f;
            d3[e] = am == 3 ? q[e] : 0.f;
        }
        float* o = dx + off;
        *reinterpret_cast<f32x4*>(o) = d0;
        *reinterpret_cast<f32x4*>(o + C) = d1;
        *reinterpret_cast<f32x4*>(o + row) = d2;
        *reinterpret_cast<f32x4*>(o + row + C) = d3;
    }
}

// Slices of the unit list: a function of the shape alone (never of the device), so that two calls agree bit for bit
int c3_wgrad_slices(int B, int H, int W) {
    const long long units = (long long)B * H * cdiv(W, kCwSeg);
    return (int)std::max<long long>(1, std::min<long long>(kCwMaxSlices, units / kCwMinUnits));
}

}  // namespace

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_conv3x3_c3_wgrad_slices(int B, int H, int W) { return conv3x3_c3_ok(B, H, W) ? c3_wgrad_slices(B, H, W) : 0; }

extern "C" size_t fpc_conv3x3_c3_wgrad_workspace_bytes(int B, int H, int W) {
    return (size_t)fpc_conv3x3_c3_wgrad_slices(B, H, W) * 64 * kCwN * sizeof(float);
}

extern "C" int fpc_conv3x3_c3_wgrad(const float* img4, const float* dy, float* dw, float* db, int B, int H, int W, void* ws,
                                    size_t ws_bytes, fpc_stream_t stream) {
    if (!img4 || !dy || !dw || !ws || !conv3x3_c3_ok(B, H, W)) return FPC_EINVAL;
    if (!al16(img4) || !al16(dy) || !al16(dw) || !al16(db) || !al16(ws)) return FPC_EINVAL;
    if (ws_bytes < fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W)) return FPC_EINVAL;
    C3WgradArgs a;
    memset(&a, 0, sizeof(a));
    a.img = img4; a.dy = dy; a.part = (float*)ws;
    a.B = B; a.H = H; a.W = W;
    a.nseg = cdiv(W, kCwSeg);
    a.nunit = B * H * a.nseg;      // <= B H W < 2^28: conv3x3_c3_ok
    a.nslice = c3_wgrad_slices(B, H, W);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_c3_wgrad, dim3((unsigned)a.nslice), dim3(kCwThreads), 0, s, a);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_c3_wgrad_reduce, dim3(kCwOut / 32), dim3(256), 0, s, (const float*)ws, dw, db, a.nslice);
    return check_launch();
}

extern "C" int fpc_maxpool2x2_bwd(const float* x, const float* dy, float* dx, int B, int H, int W, int C, fpc_stream_t stream) {
    if (!x || !dy || !dx || !al16(x) || !al16(dy) || !al16(dx) || !maxpool2x2_ok(B, H, W, C)) return FPC_EINVAL;
    const long long items = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(k_maxpool2x2_bwd, dim3(stream_grid(items)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (unsigned)items, W / 2, C);
    return check_launch();
}
