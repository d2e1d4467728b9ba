// se_train.hip — the squeeze-and-excitation block of the SE-ResNet encoders in the TRAINING step: the backward of
//     y = relu(x * g + res),   g = sigmoid(w2 h + b2),   h = relu(w1 m + b1),   m = mean_hw(x)
// (autograd through pretrainedmodels.senet.SEModule and the add / ReLU of SEResNetBottleneck.forward in the reference, reached from
// F/lib/pose_regressor.py:608-613).  The forward is se.hip's three kernels, k_se_excite in its SAVE instantiation, which also writes
// m and h (launch_se_excite_train).  Conventions of se.hip: NHWC f32, C a multiple of 64 (at most 8192), 256-thread workgroups, no
// float atomics, every sum in an order fixed by the shape alone (two launches agree bit for bit), 16-byte loads and stores along C.
// With d = gy * (y > 0):
//
//   k_se_bwd_reduce   grid (slabs, B), k_se_pool's slab geometry (se_pool_slabs / se_rows / se_lanes of net_kernels.hpp):
//                     partial[b][slab][c] = sum over the slab's pixels of d * x; gy, y and x are read once.  A thread row adds its
//                     pixels in ascending order, the rows are added in row order.
//   k_se_excite_bwd   one workgroup per frame.  dg[c] = the slabs in slab order; dv = dg * g * (1 - g);
//                     dh[j] = (h[j] > 0) * sum_c dv[c] w2[c][j]: LANES ALONG j within a row of w2, four neighbouring j per lane
//                     with one 16-byte load where Cr % 4 == 0 (else one j per lane): JL = the power of two >= min(Cr / 4, 256)
//                     lanes, so a wave's loads are one contiguous run of w2; the 256 / JL thread slices deal the rows c among
//                     themselves (slice s takes c = s, s + slices, ... ascending), the slices are added in slice order through LDS;
//                     dm[c] = sum_j dh[j] w1[j][c]: lanes along c, a channel quad per lane (a row of w1 is contiguous), j ascending.
//                     Writes dv [B][C], dh [B][Cr], dm [B][C].
//   k_se_param_grad   dw2[c][j] = sum_b dv[b][c] h[b][j], db2[c] = sum_b dv[b][c], dw1[j][c] = sum_b dh[b][j] m[b][c],
//                     db1[j] = sum_b dh[b][j]: one item (four neighbouring elements of one row where Cr % 4 == 0, else one element)
//                     per thread, the batch in batch order, every element written exactly once.
//   k_se_bwd_apply    dx = d * g[b][c] + dm[b][c] * (1 / (H W)) (the factor the forward's mean was multiplied by), dres = d when the
//                     residual needs a gradient; one float4 per thread and step on xcd_walk, like k_se_scale_add_relu.  gy is only read.
#include "conv_device.hpp"

namespace fpc {

namespace {

__device__ __forceinline__ float4 relu_mask(const float4 gy, const float4 y) {
    return make_float4(y.x > 0.f ? gy.x : 0.f, y.y > 0.f ? gy.y : 0.f, y.z > 0.f ? gy.z : 0.f, y.w > 0.f ? gy.w : 0.f);
}

}  // namespace

// grid (slabs, B).  gy, y, x [B][HW][C]; partial [B][slabs][C], every element written once.  (k_se_pool's loop over d * x.)
__global__ __launch_bounds__(256) void k_se_bwd_reduce(const float* __restrict__ gy, const float* __restrict__ y,
                                                       const float* __restrict__ x, float* __restrict__ partial, int HW, int C,
                                                       int lanes, int rows, int slab_px) {
    __shared__ float4 s_acc[kSeThreads];
    const int t = threadIdx.x, slab = blockIdx.x, b = blockIdx.y, slabs = gridDim.x;
    const int CQ = C >> 2;
    const int r = t / lanes, q0 = t - r * lanes;
    const int p0 = slab * slab_px, p1 = min(p0 + slab_px, HW);
    const size_t frame = (size_t)b * HW * C;
    float* out = partial + ((size_t)b * slabs + slab) * C;
    for (int q = q0; q < CQ; q += lanes) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows)
            for (int p = p0 + r; p < p1; p += rows) {
                const size_t at = frame + (size_t)p * C + 4 * q;
                const float4 d = relu_mask(*reinterpret_cast<const float4*>(gy + at), *reinterpret_cast<const float4*>(y + at));
                const float4 v = *reinterpret_cast<const float4*>(x + at);
                acc.x += d.x * v.x; acc.y += d.y * v.y; acc.z += d.z * v.z; acc.w += d.w * v.w;
            }
        if (rows == 1) {      // (uniform over the workgroup)
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

// grid (B).  V = 4 where Cr % 4 == 0 (16-byte loads along the rows of w2), else 1.  JL, a power of two (1 .. 256), is the lanes along
// the Cr / V items of a row of w2.  Dynamic LDS: C + Cr floats, + 256 V when JL < 256 (the slices' partial sums, element-major).
template <int V>
__global__ __launch_bounds__(256) void k_se_excite_bwd(const float* __restrict__ partial, const float* __restrict__ gate,
                                                       const float* __restrict__ hidden, const float* __restrict__ w1,
                                                       const float* __restrict__ w2, float* __restrict__ dv_out,
                                                       float* __restrict__ dh_out, float* __restrict__ dm_out, int slabs, int C, int Cr,
                                                       int JL) {
    extern __shared__ float s_seb[];
    float* s_dv = s_seb;
    float* s_dh = s_dv + C;
    float* s_red = s_dh + Cr;      // (only there, and only touched, when JL < 256)
    const int t = threadIdx.x, b = blockIdx.x;
    const float* part = partial + (size_t)b * slabs * C;
    for (int c = t; c < C; c += kSeThreads) {
        float s = 0.f;
        for (int k = 0; k < slabs; ++k) s += part[(size_t)k * C + c];      // slab order
        const float g = gate[(size_t)b * C + c];
        const float dv = s * g * (1.0f - g);
        s_dv[c] = dv;
        dv_out[(size_t)b * C + c] = dv;
    }
    __syncthreads();
    const int jl = t & (JL - 1), sl = t / JL, slices = kSeThreads / JL, items = Cr / V;
    for (int jb = 0; jb < items; jb += JL) {      // (uniform bounds: every thread reaches the barriers)
        const int it = jb + jl;
        const bool live = it < items;
        float acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = 0.f;
        if (live) {
#pragma unroll 4
            for (int c = sl; c < C; c += slices) {
                const float dv = s_dv[c];
                if constexpr (V == 4) {
                    const float4 w = *reinterpret_cast<const float4*>(w2 + (size_t)c * Cr + 4 * it);
                    acc[0] += dv * w.x; acc[1] += dv * w.y; acc[2] += dv * w.z; acc[3] += dv * w.w;
                } else {
                    acc[0] += dv * w2[(size_t)c * Cr + it];
                }
            }
        }
        if (slices > 1) {
#pragma unroll
            for (int e = 0; e < V; ++e) s_red[e * kSeThreads + t] = acc[e];
            __syncthreads();
            if (sl == 0)
                for (int k = 1; k < slices; ++k) {      // slice order
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e] += s_red[e * kSeThreads + k * JL + jl];
                }
        }
        if (sl == 0 && live) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const int j = V * it + e;
                const float dh = hidden[(size_t)b * Cr + j] > 0.f ? acc[e] : 0.f;
                s_dh[j] = dh;
                dh_out[(size_t)b * Cr + j] = dh;
            }
        }
        __syncthreads();
    }
    for (int q = t; q < (C >> 2); q += kSeThreads) {      // a channel quad per thread: 16-byte loads along the rows of w1
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int j = 0; j < Cr; ++j) {
            const float dh = s_dh[j];
            const float4 w = *reinterpret_cast<const float4*>(w1 + (size_t)j * C + 4 * q);
            acc.x += dh * w.x; acc.y += dh * w.y; acc.z += dh * w.z; acc.w += dh * w.w;
        }
        *reinterpret_cast<float4*>(dm_out + (size_t)b * C + 4 * q) = acc;
    }
}

// One item = V neighbouring elements of one row (V = 4 where Cr % 4 == 0, else 1); the items of dw2 [C][Cr], dw1 [Cr][C], db2 [C] and
// db1 [Cr] follow one another.  dv, m [B][C]; dh, h [B][Cr].
template <int V>
__global__ __launch_bounds__(256) void k_se_param_grad(const float* __restrict__ dv, const float* __restrict__ dh,
                                                       const float* __restrict__ m, const float* __restrict__ h,
                                                       float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                       float* __restrict__ db2, int B, int C, int Cr) {
    const unsigned nW = (unsigned)C * (unsigned)Cr / V, nB2 = (unsigned)C / V, nB1 = (unsigned)Cr / V;
    unsigned i = blockIdx.x * (unsigned)kSeThreads + threadIdx.x;
    if (i >= 2 * nW + nB2 + nB1) return;
    // out[e] = sum_b a[b sa] * v[b sv + e] (a == nullptr: the factor is 1)
    const float* a = nullptr;
    const float* v;
    float* out;
    int sa = 0, sv;
    if (i < nW) {      // dw2[c][j0 ..]
        const unsigned e0 = i * V, c = e0 / Cr, j0 = e0 - c * Cr;
        a = dv + c; sa = C; v = h + j0; sv = Cr; out = dw2 + e0;
    } else if (i < 2 * nW) {      // dw1[j][c0 ..]
        const unsigned e0 = (i - nW) * V, j = e0 / C, c0 = e0 - j * C;
        a = dh + j; sa = Cr; v = m + c0; sv = C; out = dw1 + e0;
    } else if (i < 2 * nW + nB2) {
        const unsigned e0 = (i - 2 * nW) * V;
        v = dv + e0; sv = C; out = db2 + e0;
    } else {
        const unsigned e0 = (i - 2 * nW - nB2) * V;
        v = dh + e0; sv = Cr; out = db1 + e0;
    }
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    for (int b = 0; b < B; ++b) {      // batch order
        const float f = a ? a[(size_t)b * sa] : 1.0f;
        const float* vb = v + (size_t)b * sv;
        if constexpr (V == 4) {
            const float4 q = *reinterpret_cast<const float4*>(vb);
            if (a) { acc[0] += f * q.x; acc[1] += f * q.y; acc[2] += f * q.z; acc[3] += f * q.w; }
            else { acc[0] += q.x; acc[1] += q.y; acc[2] += q.z; acc[3] += q.w; }
        } else {
            acc[0] += a ? f * vb[0] : vb[0];
        }
    }
    if constexpr (V == 4) *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else out[0] = acc[0];
}

// gy, y, dx, dres [B][HW][C]; gate, dm [B][C].  dres may be null (the residual needs no gradient); dx and dres are the caller's fresh
// tensors, distinct from gy and from one another.
__global__ __launch_bounds__(256) void k_se_bwd_apply(const float* __restrict__ gy, const float* __restrict__ y,
                                                      const float* __restrict__ gate, const float* __restrict__ dm,
                                                      float* __restrict__ dx, float* __restrict__ dres, float inv_hw, unsigned total,
                                                      unsigned CQ, unsigned frame_items) {
    const XcdSpan wk = xcd_walk(total);      // < 2^32 with a grid stride of headroom: se_shape_ok
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned b = g / frame_items, c4 = g % CQ;
        const float4 d = relu_mask(*reinterpret_cast<const float4*>(gy + (size_t)g * 4), *reinterpret_cast<const float4*>(y + (size_t)g * 4));
        const float4 s = *reinterpret_cast<const float4*>(gate + (size_t)b * CQ * 4 + 4 * c4);
        const float4 p = *reinterpret_cast<const float4*>(dm + (size_t)b * CQ * 4 + 4 * c4);
        float4 o;
        o.x = d.x * s.x + p.x * inv_hw; o.y = d.y * s.y + p.y * inv_hw;
        o.z = d.z * s.z + p.z * inv_hw; o.w = d.w * s.w + p.w * inv_hw;
        *reinterpret_cast<float4*>(dx + (size_t)g * 4) = o;
        if (dres) *reinterpret_cast<float4*>(dres + (size_t)g * 4) = d;      // (uniform over the launch)
    }
}

// scratch of the backward: partial [B][slabs][C], dv [B][C], dm [B][C], dh [B][Cr] (last: B Cr floats need not be a multiple of four)
static size_t se_bwd_scratch_floats(int B, int H, int W, int C, int R) {
    if (!se_shape_ok(B, H, W, C) || R < 1 || C % R) return 0;
    return (size_t)B * ((size_t)se_pool_slabs(H, W, C) * C + 2 * (size_t)C + (size_t)(C / R));
}

static int launch_se_bwd(const float* x, const float* y, const float* gy, const float* gate, const float* mean, const float* hidden,
                         const float* w1, const float* w2, float* dx, float* dres, float* dw1, float* db1, float* dw2, float* db2,
                         float* scratch, int B, int H, int W, int C, int R, hipStream_t s) {
    if (!se_shape_ok(B, H, W, C) || R < 1 || C % R) return FPC_EINVAL;
    const int Cr = C / R, slabs = se_pool_slabs(H, W, C), rows = se_rows(C);
    float* partial = scratch;
    float* dv = partial + (size_t)B * slabs * C;
    float* dm = dv + (size_t)B * C;
    float* dh = dm + (size_t)B * C;
    hipLaunchKernelGGL(k_se_bwd_reduce, dim3(slabs, B), dim3(kSeThreads), 0, s, gy, y, x, partial, H * W, C, se_lanes(C), rows,
                       rows * kSeRowPixels);
    int rc = check_launch();
    if (rc) return rc;
    const int V = Cr % 4 == 0 ? 4 : 1;
    int JL = 1;
    while (JL < Cr / V && JL < kSeThreads) JL *= 2;
    // <= 64 KB: JL < 256 only where Cr <= 128 V, and C + Cr alone is at most 16384 floats
    const size_t lds = (size_t)(C + Cr + (JL < kSeThreads ? kSeThreads * V : 0)) * sizeof(float);
    if (V == 4)
        hipLaunchKernelGGL(k_se_excite_bwd<4>, dim3(B), dim3(kSeThreads), lds, s, partial, gate, hidden, w1, w2, dv, dh, dm, slabs, C, Cr,
                           JL);
    else
        hipLaunchKernelGGL(k_se_excite_bwd<1>, dim3(B), dim3(kSeThreads), lds, s, partial, gate, hidden, w1, w2, dv, dh, dm, slabs, C, Cr,
                           JL);
    if ((rc = check_launch())) return rc;
    if (Cr % 4 == 0) {
        const unsigned items = (2u * C * Cr + C + Cr) / 4;
        hipLaunchKernelGGL(k_se_param_grad<4>, dim3((items + kSeThreads - 1) / kSeThreads), dim3(kSeThreads), 0, s, dv, dh, mean, hidden,
                           dw1, db1, dw2, db2, B, C, Cr);
    } else {
        const unsigned items = 2u * C * Cr + C + Cr;
        hipLaunchKernelGGL(k_se_param_grad<1>, dim3((items + kSeThreads - 1) / kSeThreads), dim3(kSeThreads), 0, s, dv, dh, mean, hidden,
                           dw1, db1, dw2, db2, B, C, Cr);
    }
    if ((rc = check_launch())) return rc;
    const long long frame = (long long)H * W * (C / 4), total = (long long)B * frame;
    hipLaunchKernelGGL(k_se_bwd_apply, dim3(stream_grid(total)), dim3(kSeThreads), 0, s, gy, y, gate, dm, dx, dres,
                       1.0f / (float)((long long)H * W), (unsigned)total, (unsigned)(C / 4), (unsigned)frame);
    return check_launch();
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_se_gate_train(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                                 float* mean, float* hidden, float* scratch, int B, int H, int W, int C, int R, fpc_stream_t stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !gate || !mean || !hidden || !scratch) return FPC_EINVAL;
    if (!al16(x) || !al16(w1) || !al16(b1) || !al16(w2) || !al16(b2) || !al16(gate) || !al16(mean) || !al16(hidden) || !al16(scratch))
        return FPC_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 || R < 1 || C % R || !se_shape_ok(B, H, W, C)) return FPC_EINVAL;
    int rc = launch_se_pool(x, scratch, B, H, W, C, (hipStream_t)stream);
    if (rc) return rc;
    return launch_se_excite_train(scratch, w1, b1, w2, b2, gate, mean, hidden, B, H, W, C, R, (hipStream_t)stream);
}

extern "C" size_t fpc_se_bwd_scratch_floats(int B, int H, int W, int C, int R) { return se_bwd_scratch_floats(B, H, W, C, R); }

extern "C" int fpc_se_bwd(const float* x, const float* y, const float* gy, const float* gate, const float* mean, const float* hidden,
                          const float* w1, const float* w2, float* dx, float* dres, float* dw1, float* db1, float* dw2, float* db2,
                          float* scratch, int B, int H, int W, int C, int R, fpc_stream_t stream) {
    if (!x || !y || !gy || !gate || !mean || !hidden || !w1 || !w2 || !dx || !dw1 || !db1 || !dw2 || !db2 || !scratch) return FPC_EINVAL;
    if (!al16(x) || !al16(y) || !al16(gy) || !al16(gate) || !al16(mean) || !al16(hidden) || !al16(w1) || !al16(w2) || !al16(dx) ||
        !al16(dres) || !al16(dw1) || !al16(db1) || !al16(dw2) || !al16(db2) || !al16(scratch))
        return FPC_EINVAL;
    if (B < 1 || H < 1 || W < 1 || C < 64 || C % 64 || R < 1 || C % R || !se_shape_ok(B, H, W, C)) return FPC_EINVAL;
    return launch_se_bwd(x, y, gy, gate, mean, hidden, w1, w2, dx, dres, dw1, db1, dw2, db2, scratch, B, H, W, C, R, (hipStream_t)stream);
}
