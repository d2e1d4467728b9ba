// efficientnet.hip — the gate kernels and the entries of the EfficientNet-B0 encoder (smp's EfficientNetEncoder over
// efficientnet_pytorch, restated in lib/backbone.py EfficientNetEncoder), for inference, on mobilenet.hip's conventions: dense channel-last f32, BatchNorm folded to
// per-channel scale / shift, no atomics and no split over K — every sum runs in an order the shape alone fixes, so two launches agree
// bit for bit —, the XCD-banded walks of conv_device.hpp.  act 0 is none, 1 ReLU6, 2 swish v / (1 + exp(-v)); every division is
// div_ieee's (conv_device.hpp: sigmoid, swish).  The pads are efficientnet_pytorch's static "same" ones for the declared 224 image,
// fixed numbers: stride 1 (k - 1) / 2 on every side; stride 2 pads 0 before and 1 after for k = 3, 1 and 2 for k = 5.
//
//   k_mb_pool      per-channel partial sums of the gate's operand: one workgroup per (slab of pixels, frame), lanes along the channel
//                  quads, the slab's pixels dealt to thread rows, a fixed-order LDS reduction over the rows; partial[b][slab][C].
//   k_mb_excite    one workgroup per frame: the slabs added in slab order and divided by H W; the reduce 1x1 (a wave per four hidden
//                  units: a lane adds its channel quads in ascending order, xor butterfly), bias, swish; the expand 1x1 (16 lanes
//                  per channel: a lane adds its hidden units in ascending order, xor butterfly), bias, sigmoid; gate[b][C].
// The stem (3x3 / stride 2, pads 0 and 1, swish) and the 1x1 sites (swish, the gated in operand, K up to 2048) are the MB
// instantiations of mobilenet.hip's k_stem3x3s2, k_conv1x1_f32 and k_conv1x1_f32_small; their stand-alone entries are here.  The
// depthwise K x K convolution (fpc_mbconv_dw) is depthwise.hip's k_dw_fwd<K, S, same pad, true>.
#include "conv_device.hpp"

namespace fpc {

// grid (slabs, B).  x [B][HW][C]; partial [B][slabs][C], every element written once.  lanes = min(C / 4, 256) threads take the channel
// quads of a pixel, rows = 256 / lanes thread rows take the slab's pixels in turn (the threads behind rows * lanes only keep the
// barriers company); C / 4 > 256: one row, a thread walks several quads
__global__ __launch_bounds__(256) void k_mb_pool(const float* __restrict__ x, float* __restrict__ partial, int HW, int C, int lanes,
                                                 int rows, int slab_px) {
    __shared__ f32x4 s_acc[256];
    const int t = threadIdx.x, slab = blockIdx.x, b = blockIdx.y, slabs = gridDim.x;
    const int CQ = C >> 2;
    const int r = t / lanes, q0 = t - r * lanes;
    const int p0 = slab * slab_px, p1 = min(p0 + slab_px, HW);
    const float* xb = x + (size_t)b * HW * C;
    float* out = partial + ((size_t)b * slabs + slab) * C;
    for (int qb = 0; qb < CQ; qb += lanes) {      // (uniform over the workgroup: the barriers below)
        const int q = qb + q0;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < rows && q < CQ) {      // eight loads in flight, added in pixel order
            int p = p0 + r;
            for (; p + 7 * rows < p1; p += 8 * rows) {
                f32x4 v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const f32x4*>(xb + (size_t)(p + i * rows) * C + 4 * q);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc = acc + v[i];
            }
            for (; p < p1; p += rows) acc = acc + *reinterpret_cast<const f32x4*>(xb + (size_t)p * C + 4 * q);
        }
        s_acc[t] = acc;
        __syncthreads();
        if (r == 0 && q < CQ) {      // the rows in row order
            for (int k = 1; k < rows; ++k) acc = acc + s_acc[k * lanes + q0];
            *reinterpret_cast<f32x4*>(out + 4 * q) = acc;
        }
        __syncthreads();
    }
}

// grid (B), 1024 threads: one workgroup per frame streams both weight matrices (2 C Cs floats: 442 KB at C = 1152), so what bounds it
// is the loads it keeps in flight — 16 waves, four output rows per wave (reduce) or per 16-lane group (expand) at a time, and in
// each of the three phases a lane's loads go out eight or sixteen together, ahead of the additions, which keep their order.  (A
// first form with 256 threads, one hidden unit per wave and one channel per thread took 51 us for 1152 x 48 on one frame.)
// w1 [Cs][C], b1 [Cs], w2 [C][Cs], b2 [C]: torch's layouts of _se_reduce and _se_expand.
constexpr int kMbExciteThreads = 1024;
__global__ __launch_bounds__(kMbExciteThreads) void k_mb_excite(const float* __restrict__ partial, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, float* __restrict__ gate, int slabs, int C,
                                                                int Cs, float hw) {
    __shared__ f32x4 s_mean4[kMbMaxC / 4];
    __shared__ float s_hid[kMbMaxCs];
    float* s_mean = reinterpret_cast<float*>(s_mean4);
    const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
    const float* part = partial + (size_t)b * slabs * C;
    for (int c = t; c < C; c += kMbExciteThreads) {
        float s = 0.f;      // slab order
        int k = 0;
        for (; k + 8 <= slabs; k += 8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(k + i) * C + c];
#pragma unroll
            for (int i = 0; i < 8; ++i) s += v[i];
        }
        for (; k < slabs; ++k) s += part[(size_t)k * C + c];
        s_mean[c] = div_ieee(s, hw);
    }
    __syncthreads();
    // reduce: hidden units j0 .. j0 + 3 per wave (16 waves: every Cs <= 64 in one step); a lane adds its quads of C in ascending
    // order, then the xor butterfly
    const int CQ = C >> 2;
    for (int j0 = 4 * wave; j0 < Cs; j0 += 4 * (kMbExciteThreads / 64)) {      // (uniform over the wave: the shuffles are full)
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q0 = lane; q0 < CQ; q0 += 4 * 64) {      // four quads of four rows: sixteen 16-byte loads together
            f32x4 w[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    w[u][r] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (q0 + 64 * u < CQ && j0 + r < Cs) w[u][r] = *reinterpret_cast<const f32x4*>(w1 + (size_t)(j0 + r) * C + 4 * (q0 + 64 * u));
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (q0 + 64 * u < CQ) {
                    const f32x4 m = s_mean4[q0 + 64 * u];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        acc[r] += w[u][r][0] * m[0]; acc[r] += w[u][r][1] * m[1]; acc[r] += w[u][r][2] * m[2]; acc[r] += w[u][r][3] * m[3];
                    }
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off);
            if (lane == 0 && j0 + r < Cs) s_hid[j0 + r] = swish(acc[r] + b1[j0 + r]);
        }
    }
    __syncthreads();
    // expand: 16 lanes per channel, channels c .. c + 3 of a group per step (C % 4 == 0: a group's four rows are inside C or all
    // outside, and the shuffles stay inside the group); a lane adds its hidden units in ascending order
    const int sub = t & 15, grp = t >> 4;
    for (int c0 = 0; c0 < C; c0 += 4 * (kMbExciteThreads / 16)) {      // (uniform over the workgroup)
        const int c = c0 + 4 * grp;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < C) {      // (Cs <= 64: at most four hidden units per lane; sixteen loads together)
            float w[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) w[u][r] = sub + 16 * u < Cs ? w2[(size_t)(c + r) * Cs + sub + 16 * u] : 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (sub + 16 * u < Cs) {
                    const float h = s_hid[sub + 16 * u];
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] += w[u][r] * h;
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off);
            if (sub == 0 && c < C) gate[(size_t)b * C + c + r] = sigmoid(acc[r] + b2[c + r]);
        }
    }
}

int launch_mb_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* partial, int B,
                   int H, int W, int C, int Cs, hipStream_t s) {
    const int slabs = mb_pool_slabs(H, W, C);
    if (B < 1 || B > 65535 || !slabs || Cs < 1 || Cs > kMbMaxCs) return FPC_EINVAL;
    const int lanes = mb_pool_lanes(C), rows = 256 / lanes;
    hipLaunchKernelGGL(k_mb_pool, dim3(slabs, B), dim3(256), 0, s, x, partial, H * W, C, lanes, rows, rows * kMbRowPixels);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_mb_excite, dim3(B), dim3(kMbExciteThreads), 0, s, partial, w1, b1, w2, b2, gate, slabs, C, Cs, (float)((long long)H * W));
    return check_launch();
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_mbconv_gate_slabs(int H, int W, int C) { return mb_pool_slabs(H, W, C); }

extern "C" size_t fpc_mbconv_gate_scratch_floats(int B, int H, int W, int C) {
    return B < 1 ? 0 : (size_t)B * mb_pool_slabs(H, W, C) * C;
}

extern "C" int fpc_mbconv_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                               float* scratch, int B, int H, int W, int C, int Cs, fpc_stream_t stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !gate || !scratch) return FPC_EINVAL;
    if (!al16(x) || !al16(w1) || !al16(b1) || !al16(w2) || !al16(b2) || !al16(gate) || !al16(scratch)) return FPC_EINVAL;
    return launch_mb_gate(x, w1, b1, w2, b2, gate, scratch, B, H, W, C, Cs, (hipStream_t)stream);
}

extern "C" int fpc_mbconv_pw(const float* in, const float* gate, const float* w, const float* scale, const float* shift, const float* res,
                             float* out, int B, int64_t HW, int Cin, int Cout, int act, fpc_stream_t stream) {
    if (!in || !w || !scale || !shift || !out || !al16(in) || !al16(gate) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out) || !al16(res))
        return FPC_EINVAL;
    return launch_mb_conv1x1(in, gate, w, scale, shift, res, out, B, (long long)HW, Cin, Cout, act, (hipStream_t)stream);
}

extern "C" int fpc_mbconv_pw_form(int B, int64_t HW, int Cin, int Cout) {
    if (!mb_conv1x1_ok(B, (long long)HW, Cin, Cout)) return FPC_EINVAL;
    return conv1x1_f32_tiles((long long)B * HW, Cout);
}

extern "C" int fpc_mbconv_stem(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                               int Cout, fpc_stream_t stream) {
    if (!in4 || !w || !scale || !shift || !out || !al16(in4) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out)) return FPC_EINVAL;
    if (Cout != 32) return FPC_EINVAL;
    return launch_mb_stem3x3s2(in4, w, scale, shift, out, B, Hi, Wi, (hipStream_t)stream);
}
