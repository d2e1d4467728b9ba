// vgg.hip — the two kernels of the VGG encoders (torchvision's vgg11 .. vgg19_bn features as smp wraps them: lib/backbone.py
// VGGEncoder) that no other file expresses, for inference; every other convolution of a VGG plan is an ordinary site of the
// planner (3x3 / stride 1 / pad 1, Cin % 8 == 0, Cout % 64 == 0: Winograd or the implicit GEMM).  Activations are dense channel-last
// f32.  No atomics, no split sums: two launches agree bit for bit.  No kernel divides a float.  Workgroups walk their items in the
// XCD-banded order of the other streaming kernels (conv_device.hpp: xcd_walk), so neighbouring rows are fetched by one L2.
//
//   k_conv3x3_c3   features.0: dense 3x3 / stride 1 / pad 1 over the NHWC4 image to 64 channels at full resolution.  Write-bound:
//                  16 bytes read against 256 written per pixel.  k_stem3x3s2's shape (mobilenet.hip): sixteen threads per output
//                  pixel, each with the 4 x 27 weights of its channel quad in registers for the whole launch; the nine 16-byte
//                  pixels of a window are the same addresses for those sixteen lanes (one fetch); a wave stores 4 x 256 contiguous
//                  bytes.  A thread computes two horizontally neighbouring pixels from the 3 x 4 window they share: the kernel is
//                  bound by instruction issue (16 lanes a pixel), so the index arithmetic and a third of the loads are spent once per
//                  pair.  27 FMAs per channel in (kh, kw, ci) order.  A tap outside the image is a select on a load from a clamped,
//                  valid address: nothing outside the tensor is read; a wave wholly inside the image skips clamps and selects.
//                  The image's fourth channel never enters a product.
//   k_maxpool2x2   MaxPool2d(2, 2): max(max(x00, x01), max(x10, x11)), one thread per (pooled pixel, channel quad), 16-byte accesses.
#include "conv_device.hpp"

namespace fpc {

// One thread's pixel pair: outputs (y0, x0) and (y0, x0 + 1), x0 even, of its channel quad, from the 3 x 4 window of 16-byte pixels
// they share.  INTERIOR: the whole window and both outputs lie inside the image — no clamp, no select, two stores.  Otherwise every
// address is clamped into the image and a tap outside it is a select of zero; the second output is stored where x0 + 1 < W.  Either
// way a channel's 27 FMAs run from 0 in (kh, kw, ci) order.
template <bool AFF, bool INTERIOR>
__device__ __forceinline__ void c3_pair(const float* __restrict__ img, const float (&wr)[108], const f32x4 sc, const f32x4 sh,
                                        float* __restrict__ o0, int y0, int x0, int H, int W, int act) {
    float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
        const int hi = y0 - 1 + kh;
        const int hc = INTERIOR ? hi : min(max(hi, 0), H - 1);
        float v[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int wi = x0 - 1 + j;
            const int wc = INTERIOR ? wi : min(max(wi, 0), W - 1);
            const f32x4 t = *reinterpret_cast<const f32x4*>(img + ((size_t)hc * W + wc) * 4);      // always inside the image
            const bool ok = INTERIOR || (hi == hc && wi == wc);
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) v[j][ci] = ok ? t[ci] : 0.f;
        }
#pragma unroll
        for (int kw = 0; kw < 3; ++kw)
#pragma unroll
            for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float wv = wr[27 * j + 9 * ci + 3 * kh + kw];
                    a0[j] = fmaf(v[kw][ci], wv, a0[j]);
                    a1[j] = fmaf(v[kw + 1][ci], wv, a1[j]);
                }
    }
    f32x4 r0, r1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float u0 = AFF ? a0[j] * sc[j] + sh[j] : a0[j] + sh[j], u1 = AFF ? a1[j] * sc[j] + sh[j] : a1[j] + sh[j];
        r0[j] = act ? fmaxf(u0, 0.f) : u0;
        r1[j] = act ? fmaxf(u1, 0.f) : u1;
    }
    *reinterpret_cast<f32x4*>(o0) = r0;
    if (INTERIOR || x0 + 1 < W) *reinterpret_cast<f32x4*>(o0 + 64) = r1;
}

// n / d for n < 2^31 by the launcher's reciprocal (net_kernels.hpp: wino_recip)
__device__ __forceinline__ unsigned div_by(unsigned n, const WinoRecip r) { return (unsigned)(((unsigned long long)n * r.m) >> r.sh); }

// in4 [B][H][W][4] (the fourth channel is not used), w [64][3][3][3], out [B][H][W][64].  An item is a pair of horizontally
// neighbouring pixels (x0 even; Wp = (W + 1) / 2 pairs a row, the last with one pixel where W is odd): items = B H Wp.  Sixteen
// threads an item.  AFF: scale is read (BatchNorm folded with the conv bias); without it the epilogue is sum + shift (the bias
// alone).  A wave whose four items all lie inside takes the path without clamps and selects (one scalar branch).
template <bool AFF>
__global__ __launch_bounds__(256) void k_conv3x3_c3(const float* __restrict__ in4, const float* __restrict__ w,
                                                    const float* __restrict__ scale, const float* __restrict__ shift,
                                                    float* __restrict__ out, unsigned items, int H, int W, int Wp, const WinoRecip rWp,
                                                    const WinoRecip rH, int act) {
    const unsigned q = threadIdx.x & 15, pl = threadIdx.x >> 4;
    float wr[108];      // channels 4 q .. 4 q + 3: [channel][ci][kh][kw]
#pragma unroll
    for (int i = 0; i < 27; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + 108 * q + 4 * i);
        wr[4 * i] = v[0]; wr[4 * i + 1] = v[1]; wr[4 * i + 2] = v[2]; wr[4 * i + 3] = v[3];
    }
    f32x4 sc = f32x4{1.f, 1.f, 1.f, 1.f};
    if (AFF) sc = *reinterpret_cast<const f32x4*>(scale + 4 * q);
    const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + 4 * q);
    const XcdSpan wk = xcd_rows(items, 16u, pl);
    for (unsigned it = wk.first; it < wk.end; it += wk.step) {
        const unsigned t = div_by(it, rWp), xp = it - t * (unsigned)Wp;      // t = b H + y0: the row of the batch
        const unsigned b = div_by(t, rH);
        const int y0 = (int)(t - b * (unsigned)H), x0 = 2 * (int)xp;
        const float* img = in4 + (size_t)b * H * W * 4;
        float* o0 = out + ((size_t)t * W + x0) * 64 + 4 * q;
        const bool inside = y0 >= 1 && y0 + 1 < H && x0 >= 1 && x0 + 2 < W;
        if (__all(inside)) c3_pair<AFF, true>(img, wr, sc, sh, o0, y0, x0, H, W, act);
        else c3_pair<AFF, false>(img, wr, sc, sh, o0, y0, x0, H, W, act);
    }
}

// x [B][H][W][C] -> y [B][H / 2][W / 2][C]; H, W even, C % 4 == 0; items = B (H / 2) (W / 2) (C / 4)
__global__ __launch_bounds__(256) void k_maxpool2x2(const float* __restrict__ x, float* __restrict__ y, unsigned items, int Ho, int Wo, int C) {
    const unsigned C4 = (unsigned)C >> 2;
    const XcdSpan wk = xcd_walk(items);      // < kWalkLimit: launch_maxpool2x2
    const size_t row = (size_t)2 * Wo * C;   // one input row
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned c4 = g % C4;
        unsigned r = g / C4;
        const unsigned wo = r % (unsigned)Wo; r /= (unsigned)Wo;      // r = b Ho + ho: input row 2 r of the batch's rows
        const float* p = x + (size_t)2 * r * row + (size_t)2 * wo * C + 4 * c4;
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + C);
        const f32x4 c = *reinterpret_cast<const f32x4*>(p + row), d = *reinterpret_cast<const f32x4*>(p + row + C);
        f32x4 m;
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = fmaxf(fmaxf(a[j], b[j]), fmaxf(c[j], d[j]));
        *reinterpret_cast<f32x4*>(y + (size_t)g * 4) = m;
    }
}

// The stated bound of the entry: 16 B H W below kWalkLimit.  (The walk itself is over B H (W + 1) / 2 pixel pairs, sixteen threads
// each: no more than B H W items, which that bound keeps below 2^28 — the 32-bit walk cannot wrap and the reciprocal divisions are exact.)
bool conv3x3_c3_ok(int B, int H, int W) { return B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W * 16 < kWalkLimit; }

int launch_conv3x3_c3(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int H, int W, int act,
                      hipStream_t s) {
    if (!conv3x3_c3_ok(B, H, W) || act < 0 || act > 1 || !shift) return FPC_EINVAL;
    const int Wp = (W + 1) / 2;
    const long long items = (long long)B * H * Wp;      // (< 2^28: conv3x3_c3_ok, so the reciprocal divisions are exact)
    // (a thread loads its 108 weights once: a grid of items / 256 workgroups gives it sixteen pixel pairs to spend them on)
    const dim3 grid(stream_grid(items)), blk(256);
    const WinoRecip rWp = wino_recip((unsigned)Wp), rH = wino_recip((unsigned)H);
    if (scale) hipLaunchKernelGGL(k_conv3x3_c3<true>, grid, blk, 0, s, in4, w, scale, shift, out, (unsigned)items, H, W, Wp, rWp, rH, act);
    else hipLaunchKernelGGL(k_conv3x3_c3<false>, grid, blk, 0, s, in4, w, scale, shift, out, (unsigned)items, H, W, Wp, rWp, rH, act);
    return check_launch();
}

bool maxpool2x2_ok(int B, int H, int W, int C) {
    return B >= 1 && H >= 2 && W >= 2 && !(H & 1) && !(W & 1) && C >= 4 && C % 4 == 0 && (long long)B * (H / 2) * (W / 2) * (C / 4) < kWalkLimit;
}

int launch_maxpool2x2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s) {
    if (!maxpool2x2_ok(B, H, W, C)) return FPC_EINVAL;
    const long long items = (long long)B * (H / 2) * (W / 2) * (C / 4);
    hipLaunchKernelGGL(k_maxpool2x2, dim3(stream_grid(items)), dim3(256), 0, s, x, y, (unsigned)items, H / 2, W / 2, C);
    return check_launch();
}

// shift[c] += scale[c] * bias[c]: a convolution's bias folded behind its folded BatchNorm (once per load)
__global__ void k_fold_conv_bias(const float* __restrict__ scale, const float* __restrict__ bias, float* __restrict__ shift, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) shift[c] = shift[c] + scale[c] * bias[c];
}

int launch_fold_conv_bias(const float* scale, const float* bias, float* shift, int C, hipStream_t s) {
    if (C < 1) return FPC_EINVAL;
    hipLaunchKernelGGL(k_fold_conv_bias, dim3(cdiv(C, 256)), dim3(256), 0, s, scale, bias, shift, C);
    return check_launch();
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_conv3x3_c3(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int H, int W,
                              int Cout, int act, fpc_stream_t stream) {
    if (!in4 || !w || !shift || !out || !al16(in4) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out)) return FPC_EINVAL;
    if (Cout != 64) return FPC_EINVAL;
    return launch_conv3x3_c3(in4, w, scale, shift, out, B, H, W, act, (hipStream_t)stream);
}

extern "C" int fpc_maxpool2x2_fwd(const float* x, float* y, int B, int H, int W, int C, fpc_stream_t stream) {
    if (!x || !y || !al16(x) || !al16(y)) return FPC_EINVAL;
    return launch_maxpool2x2(x, y, B, H, W, C, (hipStream_t)stream);
}
