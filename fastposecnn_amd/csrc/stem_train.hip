// stem_train.hip — the training step's 7x7 / stride-2 stem and the 3x3 / stride-2 max-pool behind it (smp's ResNet encoder conv1 /
// maxpool, F/lib/pose_regressor.py:608, under Lightning's training step): the stem's weight gradient, the max-pool's backward, and
// entry points to the kernels the inference engine already has for the forward halves (k_nchw3_to_nhwc4, k_stem7x7 through
// fpc_conv2d's code 3000, k_maxpool3x3s2).  f32 throughout, no atomics, a fixed summation order: bit-identical from run to run.
//
// k_stem_wgrad + k_stem_wgrad_reduce:
//   dw[co][c][kh][kw] = sum over b, oy, ox of dy[b][oy][ox][co] * img[b][2 oy + kh - 3][2 ox + kw - 3][c]      (zero outside the image)
// As a GEMM: M = 64 output channels, N = the forward's K layout (column n = kh * 32 + tap * 4 + c: 7 kernel rows x 8 taps x 4
// channels = 224, 147 of them real — tap 7 and channel 3 are computed and never read), K = the pixels.  A unit is (frame, output row,
// 64-pixel segment); a workgroup of 7 waves walks a contiguous slice of the unit list with the 64 x 224 accumulator in registers —
// wave kh owns kernel row kh: the 32 columns of that row x 64 channels = two 32 x 32 tiles — and writes ONE partial [64][224] at the
// end of its slice.  Per unit the workgroup stages
//   the 7 image rows under the segment, 2 * 64 + 6 pixels of 16 bytes each (15 KB; zeros outside the image: the loads are from a
//     clamped address and a select zeroes them — predicated, not branched), and
//   the 64 x 64 dy tile (16 KB; zeros past the row's end), laid out in the A fragment's own order ([pixel pair][32-channel half]
//     [pixel of the pair][channel]: lane-linear reads),
// and feeds v_mfma_f32_32x32x2_f32 (exact f32 products) with A = dy[px][co], B = lds[kh][2 px + tap][c]: lane l reads word
// 16 pair + 8 (l >> 5) + (l & 31) of its row, 40 consecutive words per instruction.  The next unit's global loads (6 float4 per
// thread) are in flight under the current unit's 64 MFMAs per wave.  Work at B = 8, 640 x 480: 2 * 64 * 224 * 614 400 = 17.6 GFLOP
// issued for 11.6 useful, 157 MB of dy and 39 MB of image read once.
// k_stem_wgrad_reduce adds the partials in slice order, in double, and writes OIHW [64][3][7][7].
//
// k_maxpool3x3s2_bwd: the max-pool's backward in GATHER form, NHWC, C % 4 == 0, one float4 of channels per thread: no stored
// indices, no atomics, every dx element written exactly once.  Per axis an even input index lies in one window and an odd one in two,
// so a dx element sums dy over 1, 2, 2 or 4 windows — those of which it is the arg-max.  The arg-max is recomputed from x by torch's
// rule: scan the window row-major over its in-bounds elements and keep the FIRST maximum (val > max), padding never wins.  After a
// ReLU half the values are exactly 0 and ties are the common case.  A thread takes the 2 x 2 block of dx at (2a, 2b): the four
// windows (a .. a + 1) x (b .. b + 1) are all that reach it and they lie inside the 5 x 5 patch of x at (2a - 1, 2b - 1), loaded
// once (-inf outside the image: it never wins) — 25 + 4 loads for 4 elements where an element alone would scan up to 36 (that
// form, one element per thread, measured 415 us at B = 8, 64 channels, 240 x 320).  Each window's arg-max is found once per
// thread; an element takes the dy of the windows whose arg-max it is, added in (window row, window column) order.  Inputs are
// finite: NaN (and infinities) are outside the contract.
#include <string.h>

#include <algorithm>

#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr int kSwThreads = 448;               // 7 waves: one per kernel row
constexpr int kSwSeg = 64;                    // output pixels of a unit
constexpr int kSwRowPx = 2 * kSwSeg + 6;      // image pixels under a segment
constexpr int kSwRowF = kSwRowPx * 4;         // ... floats
constexpr int kSwN = 224;                     // columns of a partial
constexpr int kSwImg4 = 7 * kSwRowPx;         // float4 of the image stage (938)
constexpr int kSwDy4 = kSwSeg * 16;           // float4 of the dy stage (1024)
constexpr int kSwMinUnits = 8;                // units per slice at least: a partial (57 KB) costs as much as two units' operands
constexpr int kSwMaxSlices = 512;             // two workgroups per compute unit

struct StemWgradArgs {
    const float* img;     // [B][Hi][Wi][4]
    const float* dy;      // [B][Ho][Wo][64]
    float* part;          // [nslice][64][224]
    int B, Hi, Wi, Ho, Wo, nseg, nunit, nslice;
};

__global__ __launch_bounds__(kSwThreads) void k_stem_wgrad(const StemWgradArgs a) {
    __shared__ __attribute__((aligned(16))) float s_dy[kSwDy4 * 4];
    __shared__ __attribute__((aligned(16))) float s_im[kSwImg4 * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int kh = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slice = blockIdx.x;
    const int u0 = (int)((long long)slice * a.nunit / a.nslice), u1 = (int)((long long)(slice + 1) * a.nunit / a.nslice);
    const int per_frame = a.Ho * a.nseg;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    f32x16 acc0, acc1;      // output channels 0-31 / 32-63 x this wave's 32 columns
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }

    f32x4 rd[3], ri[3];
    auto load = [&](int u) {
        const int b = u / per_frame, r = u - b * per_frame;
        const int oy = r / a.nseg, ox0 = (r - oy * a.nseg) * kSwSeg;
        const float* dyr = a.dy + ((long long)b * a.Ho + oy) * a.Wo * 64;
        const float* imb = a.img + (long long)b * a.Hi * a.Wi * 4;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = tid + kSwThreads * j;
            if (i < kSwDy4) {
                const int px = ox0 + (i >> 4), c4 = i & 15;
                const f32x4 v = *reinterpret_cast<const f32x4*>(dyr + (long long)min(px, a.Wo - 1) * 64 + 4 * c4);
                rd[j] = px < a.Wo ? v : zero;
            }
            if (i < kSwImg4) {
                const int row = i / kSwRowPx, xi = i - row * kSwRowPx;
                const int iy = 2 * oy - 3 + row, ix = 2 * ox0 - 3 + xi;
                const f32x4 v = *reinterpret_cast<const f32x4*>(imb + ((long long)min(max(iy, 0), a.Hi - 1) * a.Wi + min(max(ix, 0), a.Wi - 1)) * 4);
                ri[j] = (iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi) ? v : zero;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int i = tid + kSwThreads * j;
            if (i < kSwDy4) {      // pixel p = i >> 4, channels 4 (i & 15) ..: [p >> 1][channel half][p & 1][channel & 31]
                const int p = i >> 4, c4 = i & 15;
                *reinterpret_cast<f32x4*>(s_dy + ((p >> 1) * 2 + (c4 >> 3)) * 64 + (p & 1) * 32 + (c4 & 7) * 4) = rd[j];
            }
            if (i < kSwImg4) *reinterpret_cast<f32x4*>(s_im + i * 4) = ri[j];
        }
    };

    if (u0 < u1) load(u0);
    const float* pa = s_dy + lane;
    const float* pb = s_im + kh * kSwRowF + 8 * (lane >> 5) + (lane & 31);
#pragma unroll 1
    for (int u = u0; u < u1; ++u) {
        store();
        __syncthreads();
        if (u + 1 < u1) load(u + 1);
#pragma unroll
        for (int kp = 0; kp < kSwSeg / 2; ++kp) {      // pixel pair kp: A[co][k] = dy[2 kp + k][co], B[k][n] = image word 16 kp + 8 k + n
            const float a0 = pa[(2 * kp) * 64], a1 = pa[(2 * kp + 1) * 64], bv = pb[16 * kp];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
        __syncthreads();      // the stage is read out
    }

    // C/D layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    float* out = a.part + (size_t)slice * 64 * kSwN + kh * 32 + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        out[(size_t)co * kSwN] = acc0[r];
        out[(size_t)(co + 32) * kSwN] = acc1[r];
    }
}

// dw[co][c][kh][kw] = sum over the slices, in slice order, of part[slice][co][kh * 32 + kw * 4 + c].  32 elements per workgroup;
// eight threads per element take the eighths of the slice list (in double), thread 0 of them adds the eight in order.
__global__ __launch_bounds__(256) void k_stem_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int nslice) {
    __shared__ double s_sum[8][32];
    const int j = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int o = blockIdx.x * 32 + j;      // < 64 * 147 = 294 * 32
    const int co = o / 147, r = o - co * 147, c = r / 49, r2 = r - c * 49, kh = r2 / 7, kw = r2 - kh * 7;
    const float* src = part + (size_t)co * kSwN + kh * 32 + kw * 4 + c;
    const int per = (nslice + 7) >> 3, s0 = sub * per, s1 = min(nslice, s0 + per);
    double acc = 0.0;
    for (int s = s0; s < s1; ++s) acc += (double)src[(size_t)s * 64 * kSwN];
    s_sum[sub][j] = acc;
    __syncthreads();
    if (sub == 0) {
#pragma unroll
        for (int k = 1; k < 8; ++k) acc += s_sum[k][j];
        dw[o] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void k_maxpool3x3s2_bwd(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                          int B, int Hi, int Wi, int C, int Ho, int Wo) {
    const int C4 = C >> 2, Hb = (Hi + 1) >> 1, Wb = (Wi + 1) >> 1;      // blocks of 2 x 2 elements of dx
    const long long total = (long long)B * Hb * Wb * C4;
    const float ninf = -__builtin_huge_valf();
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < total; g += (long long)gridDim.x * 256) {
        const int c4 = (int)(g % C4);
        long long r = g / C4;
        const int bx = (int)(r % Wb); r /= Wb;
        const int by = (int)(r % Hb);
        const int b = (int)(r / Hb);
        const float* xb = x + (size_t)b * Hi * Wi * C + 4 * c4;
        const float* dyb = dy + (size_t)b * Ho * Wo * C + 4 * c4;
        float* dxb = dx + (size_t)b * Hi * Wi * C + 4 * c4;
        // the patch: rows 2 by - 1 .. 2 by + 3, columns 2 bx - 1 .. 2 bx + 3; element p = 5 row + column.  Loads from a clamped
        // address, -inf outside the image
        f32x4 v[25];
#pragma unroll
        for (int py = 0; py < 5; ++py)
#pragma unroll
            for (int px = 0; px < 5; ++px) {
                const int hy = 2 * by - 1 + py, wx = 2 * bx - 1 + px;
                const bool in = hy >= 0 && hy < Hi && wx >= 0 && wx < Wi;
                const f32x4 e = *reinterpret_cast<const f32x4*>(xb + ((size_t)min(max(hy, 0), Hi - 1) * Wi + min(max(wx, 0), Wi - 1)) * C);
                v[5 * py + px] = in ? e : f32x4{ninf, ninf, ninf, ninf};
            }
        // window (by + i, bx + j) covers patch rows 2 i .. 2 i + 2, columns 2 j .. 2 j + 2: its first maximum, per channel
        // (a window past Ho / Wo does not exist: its dy reads as zero)
        int am[2][2][4];
        f32x4 gq[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bool wok = by + i < Ho && bx + j < Wo;
                const f32x4 q = *reinterpret_cast<const f32x4*>(dyb + ((size_t)min(by + i, Ho - 1) * Wo + min(bx + j, Wo - 1)) * C);
                gq[i][j] = wok ? q : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float best = ninf;
                    int bp = -1;
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) {
                            const int p = 5 * (2 * i + ky) + 2 * j + kx;
                            const bool w = v[p][e] > best;
                            best = w ? v[p][e] : best;
                            bp = w ? p : bp;
                        }
                    am[i][j][e] = bp;
                }
            }
        // element (2 by + rr, 2 bx + cc) = patch element 5 (rr + 1) + cc + 1, inside the windows i <= rr, j <= cc
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int p0 = 5 * (rr + 1) + cc + 1;
                f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i <= rr; ++i)
#pragma unroll
                    for (int j = 0; j <= cc; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) sum[e] += am[i][j][e] == p0 ? gq[i][j][e] : 0.f;
                const int iy = 2 * by + rr, ix = 2 * bx + cc;
                if (iy < Hi && ix < Wi) *reinterpret_cast<f32x4*>(dxb + ((size_t)iy * Wi + ix) * C) = sum;
            }
    }
}

inline bool stem_shape_ok(int B, int Hi, int Wi) {
    return B >= 1 && Hi >= 8 && Wi >= 8 && Hi % 2 == 0 && Wi % 2 == 0 && (long long)B * Hi * Wi < (1LL << 31);
}

// Slices of the unit list: a function of the shape alone (never of the device), so that two calls agree bit for bit
int stem_wgrad_slices(int B, int Hi, int Wi) {
    const long long units = (long long)B * (Hi / 2) * cdiv(Wi / 2, kSwSeg);
    return (int)std::max<long long>(1, std::min<long long>(kSwMaxSlices, units / kSwMinUnits));
}

inline bool pool_shape_ok(int B, int Hi, int Wi, int C) {
    return B >= 1 && Hi >= 1 && Wi >= 1 && C >= 4 && C % 4 == 0 && (long long)B * Hi * Wi * C < (1LL << 32);
}

}  // namespace

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_image_nhwc4(const float* x, float* out, int B, int H, int W, fpc_stream_t stream) {
    if (!x || !out || !al16(x) || !al16(out) || B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1LL << 31) || (long long)H * W >= (1LL << 30))
        return FPC_EINVAL;
    return launch_nchw3_to_nhwc4(x, out, B, H * W, (hipStream_t)stream);
}

extern "C" int fpc_stem_wgrad_slices(int B, int Hi, int Wi) { return stem_shape_ok(B, Hi, Wi) ? stem_wgrad_slices(B, Hi, Wi) : 0; }

extern "C" size_t fpc_stem_wgrad_workspace_bytes(int B, int Hi, int Wi) {
    return (size_t)fpc_stem_wgrad_slices(B, Hi, Wi) * 64 * kSwN * sizeof(float);
}

extern "C" int fpc_stem_wgrad(const float* img4, const float* dy, float* dw, int B, int Hi, int Wi, void* ws, size_t ws_bytes,
                              fpc_stream_t stream) {
    if (!img4 || !dy || !dw || !ws || !stem_shape_ok(B, Hi, Wi)) return FPC_EINVAL;
    if (!al16(img4) || !al16(dy) || !al16(dw) || ((uintptr_t)ws & 255)) return FPC_EINVAL;
    if (ws_bytes < fpc_stem_wgrad_workspace_bytes(B, Hi, Wi)) return FPC_EWORKSPACE;
    StemWgradArgs a;
    memset(&a, 0, sizeof(a));
    a.img = img4; a.dy = dy; a.part = (float*)ws;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Hi / 2; a.Wo = Wi / 2;
    a.nseg = cdiv(a.Wo, kSwSeg);
    a.nunit = B * a.Ho * a.nseg;      // < 2^31: stem_shape_ok
    a.nslice = stem_wgrad_slices(B, Hi, Wi);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_stem_wgrad, dim3((unsigned)a.nslice), dim3(kSwThreads), 0, s, a);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_stem_wgrad_reduce, dim3(64 * 147 / 32), dim3(256), 0, s, (const float*)ws, dw, a.nslice);
    return check_launch();
}

extern "C" int fpc_maxpool3x3s2_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, fpc_stream_t stream) {
    if (!x || !y || !al16(x) || !al16(y) || !pool_shape_ok(B, Hi, Wi, C)) return FPC_EINVAL;
    return launch_maxpool3x3s2(x, y, B, Hi, Wi, C, (Hi - 1) / 2 + 1, (Wi - 1) / 2 + 1, (hipStream_t)stream);
}

extern "C" int fpc_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int B, int Hi, int Wi, int C, fpc_stream_t stream) {
    if (!x || !dy || !dx || !al16(x) || !al16(dy) || !al16(dx) || !pool_shape_ok(B, Hi, Wi, C)) return FPC_EINVAL;
    const long long items = (long long)B * ((Hi + 1) / 2) * ((Wi + 1) / 2) * (C / 4);      // 2 x 2 blocks of dx x channel quads
    hipLaunchKernelGGL(k_maxpool3x3s2_bwd, dim3(stream_grid(items)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, B, Hi, Wi, C,
                       (Hi - 1) / 2 + 1, (Wi - 1) / 2 + 1);
    return check_launch();
}
