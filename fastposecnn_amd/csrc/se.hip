// se.hip — the squeeze-and-excitation gate of the SE-ResNet encoders (se_resnet50 / 101 / 152: smp's SENetEncoder over
// pretrainedmodels.senet, built at F/lib/pose_regressor.py:608-613 through smp.encoders.get_encoder), for inference:
//     y = relu(x * sigmoid(fc2(relu(fc1(mean_hw(x))))) + residual)
// behind a block's conv3 + bn3.  NHWC f32, C a multiple of 64, 256-thread workgroups.  No float atomics: every sum runs in an order
// that depends on the shape alone (never on the CU count or on the order workgroups arrive in), so two launches agree bit for bit.
//
//   k_se_pool            per-channel partial sums: one workgroup per (slab of pixels, frame); lanes along the channels with 16-byte
//                        loads, the slab's pixels dealt to `rows` thread rows (they span the waves), a fixed-order LDS reduction over
//                        the rows; writes partial[b][slab][C].  se_pool_slabs(H, W, C) is a function of the shape only.
//   k_se_excite          one workgroup per frame: the slabs added in slab order and multiplied by 1 / (H W); fc1 with one wave per
//                        output row, four rows at once (lanes stride over C, xor butterfly), bias, ReLU; fc2 with 16 lanes per
//                        output row, bias, 1 / (1 + exp(-v)) through div_ieee; writes gate[b][C].  k_se_excite<true> (the training
//                        step: launch_se_excite_train, se_train.hip) also writes the means and the hidden activations.
//   k_se_scale_add_relu  y = max(x * gate[b][c] + res, 0), one float4 per thread and step on the XCD-banded walk of the other
//                        streaming kernels; may run in place (y == x).
// The SE-ResNet stem's max-pool (3x3 / stride 2 / no padding / ceil_mode) is k_maxpool3x3s2<0> in net_kernels.hip; its stand-alone
// entry is here with the gate's.
#include <math.h>

#include "conv_device.hpp"

namespace fpc {

// (kSeThreads, kSeRowPixels, kSeMaxC, se_lanes, se_rows, se_shape_ok: net_kernels.hpp, shared with se_train.hip)

int se_pool_slabs(int H, int W, int C) {
    if (H < 1 || W < 1 || C < 64 || C % 64) return 0;
    const long long px = (long long)H * W, per = (long long)se_rows(C) * kSeRowPixels;
    return (int)((px + per - 1) / per);
}

// grid (slabs, B).  x [B][HW][C]; partial [B][slabs][C], every element written once.
__global__ __launch_bounds__(256) void k_se_pool(const float* __restrict__ x, float* __restrict__ partial, int HW, int C, int lanes,
                                                 int rows, int slab_px) {
    __shared__ float4 s_acc[kSeThreads];
    const int t = threadIdx.x, slab = blockIdx.x, b = blockIdx.y, slabs = gridDim.x;
    const int CQ = C >> 2;
    const int r = t / lanes, q0 = t - r * lanes;
    const int p0 = slab * slab_px, p1 = min(p0 + slab_px, HW);
    const float* xb = x + (size_t)b * HW * C;
    float* out = partial + ((size_t)b * slabs + slab) * C;
    // (C / 4 > 256: rows == 1 and a thread walks several quads, each over every pixel of the slab; else one quad per thread)
    for (int q = q0; q < CQ; q += lanes) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows)
            for (int p = p0 + r; p < p1; p += rows) {
                const float4 v = *reinterpret_cast<const float4*>(xb + (size_t)p * C + 4 * q);
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
        if (rows == 1) {      // (uniform over the workgroup; 128 < C / 4 < 256 leaves the threads behind the last quad idle)
            if (r == 0) *reinterpret_cast<float4*>(out + 4 * q) = acc;
            continue;
        }
        s_acc[t] = acc;
        __syncthreads();
        if (r == 0) {      // the rows in row order
            for (int k = 1; k < rows; ++k) {
                const float4 v = s_acc[k * lanes + q0];
                acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
            }
            *reinterpret_cast<float4*>(out + 4 * q) = acc;
        }
        __syncthreads();
    }
}

// grid (B).  Dynamic LDS: C + Cr floats.  w1 [Cr][C], b1 [Cr], w2 [C][Cr], b2 [C] (torch's layouts of the two 1x1 convolutions).
// One workgroup streams both weight matrices (2 C Cr floats: 2 MB at C = 2048), so what bounds it is the loads in flight: a wave
// (fc1) or a 16-lane group (fc2) works on four output rows at once, with 16-byte loads where Cr allows them.
// SAVE (the training step, launch_se_excite_train): the means and the hidden activations also go to mean_out [B][C] / hid_out [B][Cr],
// the values the gate is computed from; SAVE = false is the inference kernel, which never reads the two pointers.
template <bool SAVE>
__global__ __launch_bounds__(256) void k_se_excite(const float* __restrict__ partial, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                   const float* __restrict__ b2, float* __restrict__ gate, int slabs, int C, int Cr,
                                                   float inv_hw, float* __restrict__ mean_out, float* __restrict__ hid_out) {
    extern __shared__ float4 s_se4[];      // (float4: the 16-byte alignment of both halves, C % 4 == 0)
    float* s_mean = reinterpret_cast<float*>(s_se4);
    float* s_hid = s_mean + C;
    const int t = threadIdx.x, b = blockIdx.x, lane = t & 63, wave = t >> 6;
    const float* part = partial + (size_t)b * slabs * C;
    for (int c = t; c < C; c += kSeThreads) {
        float s = 0.f;
        for (int k = 0; k < slabs; ++k) s += part[(size_t)k * C + c];      // slab order
        s_mean[c] = s * inv_hw;
        if (SAVE) mean_out[(size_t)b * C + c] = s_mean[c];
    }
    __syncthreads();
    // fc1: rows j0 .. j0 + 3 per wave and step; a lane adds its quads of C in ascending order, then the xor butterfly
    const int CQ = C >> 2;
    for (int j0 = 4 * wave; j0 < Cr; j0 += 4 * (kSeThreads / 64)) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = lane; q < CQ; q += 64) {
            const float4 m = s_se4[q];
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j0 + r < Cr) {      // (uniform over the wave)
                    const float4 w = *reinterpret_cast<const float4*>(w1 + (size_t)(j0 + r) * C + 4 * q);
                    acc[r] += w.x * m.x; acc[r] += w.y * m.y; acc[r] += w.z * m.z; acc[r] += w.w * m.w;
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off);
            if (lane == 0 && j0 + r < Cr) {
                s_hid[j0 + r] = fmaxf(acc[r] + b1[j0 + r], 0.f);
                if (SAVE) hid_out[(size_t)b * Cr + j0 + r] = s_hid[j0 + r];
            }
        }
    }
    __syncthreads();
    // fc2: 16 lanes per output row, rows c0 + 4 g .. + 3 of group g per step (C % 64 == 0: every thread stays in the loop, the shuffles
    // are full); 16-byte loads where the rows of w2 are 16-byte aligned (Cr % 4 == 0), else one float at a time
    const int sub = t & 15, grp = t >> 4;
    const bool vec = (Cr & 3) == 0;
    for (int c0 = 0; c0 < C; c0 += 4 * (kSeThreads / 16)) {
        const int c = c0 + 4 * grp;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec) {
            const float4* h4 = s_se4 + CQ;
            for (int q = sub; q < (Cr >> 2); q += 16) {
                const float4 h = h4[q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float4 w = *reinterpret_cast<const float4*>(w2 + (size_t)(c + r) * Cr + 4 * q);
                    acc[r] += w.x * h.x; acc[r] += w.y * h.y; acc[r] += w.z * h.z; acc[r] += w.w * h.w;
                }
            }
        } else {
            for (int j = sub; j < Cr; j += 16) {
                const float h = s_hid[j];
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] += w2[(size_t)(c + r) * Cr + j] * h;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) acc[r] += __shfl_xor(acc[r], off);
            if (sub == 0) {
                const float v = acc[r] + b2[c + r];
                gate[(size_t)b * C + c + r] = div_ieee(1.0f, 1.0f + expf(-v));      // v = 100: 1 / (1 + 4e-44) = 1; v = -100: 1 / inf = 0
            }
        }
    }
}

// x, res, y [B][HW][C]; gate [B][C].  y may be x (every item reads its own four floats before it writes them): no __restrict__ there.
__global__ __launch_bounds__(256) void k_se_scale_add_relu(const float* x, const float* __restrict__ gate,
                                                           const float* __restrict__ res, float* y, unsigned total, unsigned CQ,
                                                           unsigned frame_items) {
    const XcdSpan wk = xcd_walk(total);      // < 2^32 with a grid stride of headroom: launch_se_scale_add_relu
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned b = g / frame_items, c4 = g % CQ;
        const float4 v = *reinterpret_cast<const float4*>(x + (size_t)g * 4);
        const float4 r = *reinterpret_cast<const float4*>(res + (size_t)g * 4);
        const float4 s = *reinterpret_cast<const float4*>(gate + (size_t)b * CQ * 4 + 4 * c4);
        float4 o;
        o.x = fmaxf(v.x * s.x + r.x, 0.f); o.y = fmaxf(v.y * s.y + r.y, 0.f);
        o.z = fmaxf(v.z * s.z + r.z, 0.f); o.w = fmaxf(v.w * s.w + r.w, 0.f);
        *reinterpret_cast<float4*>(y + (size_t)g * 4) = o;
    }
}

int launch_se_pool(const float* x, float* partial, int B, int H, int W, int C, hipStream_t s) {
    if (!se_shape_ok(B, H, W, C)) return FPC_EINVAL;
    const int rows = se_rows(C);
    hipLaunchKernelGGL(k_se_pool, dim3(se_pool_slabs(H, W, C), B), dim3(kSeThreads), 0, s, x, partial, H * W, C, se_lanes(C), rows,
                       rows * kSeRowPixels);
    return check_launch();
}

int launch_se_excite(const float* partial, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, int B, int H,
                     int W, int C, int R, hipStream_t s) {
    if (!se_shape_ok(B, H, W, C) || R < 1 || C % R) return FPC_EINVAL;
    const int Cr = C / R;
    hipLaunchKernelGGL(k_se_excite<false>, dim3(B), dim3(kSeThreads), (size_t)(C + Cr) * sizeof(float), s, partial, w1, b1, w2, b2, gate,
                       se_pool_slabs(H, W, C), C, Cr, 1.0f / (float)((long long)H * W), (float*)nullptr, (float*)nullptr);
    return check_launch();
}

int launch_se_excite_train(const float* partial, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                           float* mean, float* hidden, int B, int H, int W, int C, int R, hipStream_t s) {
    if (!se_shape_ok(B, H, W, C) || R < 1 || C % R || !mean || !hidden) return FPC_EINVAL;
    const int Cr = C / R;
    hipLaunchKernelGGL(k_se_excite<true>, dim3(B), dim3(kSeThreads), (size_t)(C + Cr) * sizeof(float), s, partial, w1, b1, w2, b2, gate,
                       se_pool_slabs(H, W, C), C, Cr, 1.0f / (float)((long long)H * W), mean, hidden);
    return check_launch();
}

int launch_se_scale_add_relu(const float* x, const float* gate, const float* res, float* y, int B, int H, int W, int C, hipStream_t s) {
    if (!se_shape_ok(B, H, W, C)) return FPC_EINVAL;
    const long long frame = (long long)H * W * (C / 4), total = (long long)B * frame;
    hipLaunchKernelGGL(k_se_scale_add_relu, dim3(stream_grid(total)), dim3(kSeThreads), 0, s, x, gate, res, y, (unsigned)total,
                       (unsigned)(C / 4), (unsigned)frame);
    return check_launch();
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_se_pool_slabs(int H, int W, int C) { return se_pool_slabs(H, W, C); }

extern "C" size_t fpc_se_scratch_floats(int B, int H, int W, int C) {
    return B < 1 ? 0 : (size_t)B * se_pool_slabs(H, W, C) * C;
}

extern "C" int fpc_se_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* scratch,
                           int B, int H, int W, int C, int R, fpc_stream_t stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !gate || !scratch) return FPC_EINVAL;
    if (!al16(x) || !al16(w1) || !al16(b1) || !al16(w2) || !al16(b2) || !al16(gate) || !al16(scratch)) return FPC_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 || R < 1 || C % R) return FPC_EINVAL;
    int rc = launch_se_pool(x, scratch, B, H, W, C, (hipStream_t)stream);
    if (rc) return rc;
    return launch_se_excite(scratch, w1, b1, w2, b2, gate, B, H, W, C, R, (hipStream_t)stream);
}

extern "C" int fpc_se_scale_add_relu(const float* x, const float* gate, const float* res, float* y, int B, int H, int W, int C,
                                     fpc_stream_t stream) {
    if (!x || !gate || !res || !y || !al16(x) || !al16(gate) || !al16(res) || !al16(y)) return FPC_EINVAL;
    return launch_se_scale_add_relu(x, gate, res, y, B, H, W, C, (hipStream_t)stream);
}

extern "C" int fpc_maxpool3x3s2_ceil_fwd(const float* x, float* y, int B, int Hi, int Wi, int C, fpc_stream_t stream) {
    if (!x || !y || !al16(x) || !al16(y) || B < 1 || Hi < 2 || Wi < 2 || C < 64 || C % 64) return FPC_EINVAL;
    if ((long long)B * Hi * Wi * C >= (1LL << 32)) return FPC_EINVAL;
    return launch_maxpool3x3s2_ceil(x, y, B, Hi, Wi, C, (hipStream_t)stream);
}
