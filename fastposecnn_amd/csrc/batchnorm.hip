// batchnorm.hip — training-mode BatchNorm2d on channel-last activations, fused with the residual add and the ReLU that follow
// it in a ResNet block — or with the ReLU6 behind it in a MobileNetV2 block —, forward and backward, for the training step (BASELINE.json configs[4]).  The reference's encoder is
// the smp / torchvision ResNet built at F/lib/pose_regressor.py:608: conv -> BatchNorm2d -> ReLU, and at a block's end
// conv -> BatchNorm2d -> (+ identity) -> ReLU, under autograd; torch runs that as three MIOpen kernels plus an aten add and
// ReLU each way.
//
// Activations are [P, C] f32, P = B H W pixels, C a multiple of 4; the statistics of a channel run over all P pixels:
//   forward   mean, var (biased) per channel; z = (x - mean) rstd gamma + beta (+ res); y = relu(z), min(max(z, 0), 6) or z
//   backward  g = dy [y > 0], dy [0 < y < 6] (the mask from the SAVED output: bit-consistent with the forward) or dy;
//             dbeta = sum g, dgamma = sum g xhat;  dx = gamma rstd (g - dbeta / P - xhat dgamma / P);  dres = g
// Three launches each way: per-chunk partial sums (f32 per thread over <= 8 values, combined in double), one fold of the
// partials per channel quad (double, a fixed tree: deterministic; no atomics), then the elementwise pass.  A workgroup of the
// first and the last takes kBnChunk pixels by kBnQuads channel quads (one f32x4 of a pixel per thread and step).
#include "common.hpp"

namespace fpc {

constexpr int kBnChunk = 128;     // pixels per workgroup
constexpr int kBnQuads = 16;      // channel quads per workgroup: 256 B of a pixel, sixteen pixels per step of 256 threads
constexpr int kBnRows = 256 / kBnQuads;

struct BnArgs {
    const float* x;       // [P, C] channel-last: the convolution's output
    const float* res;     // forward: the block's identity, added before the ReLU (null: none)
    const float* y;       // backward: the forward's output (the ReLU mask)
    const float* dy;      // backward: gradient of the output
    float* out;           // forward: y; backward: dx (null: not wanted)
    float* dres;          // backward: gradient of the residual (null: not wanted)
    const float* gamma; const float* beta;
    float* running_mean; float* running_var;      // both or neither
    float* part;          // [chunks][C][2]: forward {sum, centred sum of squares}, backward {sum g, sum g xhat}
    float* stats;         // [C][2] mean, rstd (written by the forward, read by the backward)
    float* dgamma; float* dbeta;      // [C]
    int P, C, Q, chunks, act;      // act: 0 none, 1 ReLU, 2 ReLU6
    float eps, momentum;
};

__device__ __forceinline__ int bn_chunk_pixels(const BnArgs& a, int chunk) { return min(a.P, (chunk + 1) * kBnChunk) - chunk * kBnChunk; }

// per channel of the chunk: the sum of its values and the sum of squares ABOUT THE CHUNK'S OWN (rounded) MEAN, from a second sweep
// that the caches serve — the centred form of k_gn4_stats (groupnorm.hip), for the reason given there: E[x^2] - mean^2 from plain
// sums loses every digit once |mean| >> std.
__global__ __launch_bounds__(256) void k_bn_stats(const BnArgs a) {
    __shared__ f32x4 red[256];
    __shared__ f32x4 s_mean[kBnQuads];
    const int t = threadIdx.x, q = t % kBnQuads, r = t / kBnQuads;
    const int chunk = blockIdx.x, qg = blockIdx.y * kBnQuads + q;
    const bool on = qg < a.Q;
    const int p0 = chunk * kBnChunk, p1 = min(a.P, p0 + kBnChunk);
    const float* xq = a.x + 4 * (size_t)qg;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (on)
        for (int p = p0 + r; p < p1; p += kBnRows) s += *reinterpret_cast<const f32x4*>(xq + (size_t)p * a.C);
    red[t] = s;
    __syncthreads();
    f32x4 sum = {0.f, 0.f, 0.f, 0.f};
    if (r == 0) {
        f32x4 m;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double ds = 0.0;
            for (int k = 0; k < kBnRows; ++k) ds += red[k * kBnQuads + q][e];
            sum[e] = (float)ds;                                    // the partial as it is stored: the fold recomputes this very mean
            m[e] = (float)div_ieee((double)sum[e], (double)(p1 - p0));
        }
        s_mean[q] = m;
    }
    __syncthreads();
    const f32x4 m = s_mean[q];
    f32x4 ss = {0.f, 0.f, 0.f, 0.f};
    if (on)
        for (int p = p0 + r; p < p1; p += kBnRows) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(xq + (size_t)p * a.C) - m;
            ss += d * d;
        }
    red[t] = ss;
    __syncthreads();
    if (r == 0 && on) {
        f32x4 o0, o1;      // {sum, ss} of channels 4 qg .. 4 qg + 3, interleaved
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double dss = 0.0;
            for (int k = 0; k < kBnRows; ++k) dss += red[k * kBnQuads + q][e];
            v[e] = (float)dss;
        }
        o0 = f32x4{sum[0], v[0], sum[1], v[1]};
        o1 = f32x4{sum[2], v[2], sum[3], v[3]};
        float* o = a.part + ((size_t)chunk * a.C + 4 * (size_t)qg) * 2;
        *reinterpret_cast<f32x4*>(o) = o0;
        *reinterpret_cast<f32x4*>(o + 4) = o1;
    }
}

// Sums over the chunks for the four channels of quad blockIdx.x: thread t takes chunks t, t + 256, ... and hands term() the
// chunk's eight floats {v0, w0, v1, w1, v2, w2, v3, w3} (as two f32x4), which adds to acc[8] in double; then the 256 partial
// sums are added in a fixed tree (wave shuffles, the four waves in order).  The totals are valid in thread 0.
template <typename F>
__device__ __forceinline__ void bn_fold(const BnArgs& a, double (*sh)[8], double* acc, F term) {
    const int t = threadIdx.x;
    const float* base = a.part + 8 * (size_t)blockIdx.x;
    for (int k = t; k < a.chunks; k += 256) {
        const float* o = base + (size_t)k * a.C * 2;
        term(*reinterpret_cast<const f32x4*>(o), *reinterpret_cast<const f32x4*>(o + 4), k, acc);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = wave_reduce_add(acc[i]);
    if ((t & (kWave - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sh[t / kWave][i] = acc[i];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = ((sh[0][i] + sh[1][i]) + sh[2][i]) + sh[3][i];
    }
}

// One workgroup per channel quad: mean and rstd of its four channels by Chan's formula over the chunk partials, and the update of
// the module's running statistics (torch.nn.BatchNorm2d: the unbiased variance goes into running_var).  One sweep over the
// partials: the squares are first collected about m0, the f32 mean of chunk 0 (as close to the mean as any chunk's: the shift
// to the true mean below takes n (mean - m0)^2, about 1/128 of the sum, away — no cancellation to speak of),
//   sum (x - m0)^2 = sum_c [ sum (x - m_c)^2 + 2 (m_c - m0) (sum_c - n_c m_c) + n_c (m_c - m0)^2 ],  m_c = the f32 chunk mean.
__global__ __launch_bounds__(256) void k_bn_finalize(const BnArgs a) {
    __shared__ double sh[4][8];
    const float* first = a.part + 8 * (size_t)blockIdx.x;
    const double n0 = (double)bn_chunk_pixels(a, 0);
    double m0[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) m0[e] = (double)(float)div_ieee((double)first[2 * e], n0);
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // {sum, sum of squares about m0} x 4
    bn_fold(a, sh, acc, [&](const f32x4 lo, const f32x4 hi, int k, double* s) {
        const double nc = (double)bn_chunk_pixels(a, k);
        const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double sc = (double)v[2 * e];
            const double mc = (double)(float)div_ieee(sc, nc), d = mc - m0[e];
            s[2 * e] += sc;
            s[2 * e + 1] += (double)v[2 * e + 1] + 2.0 * d * (sc - nc * mc) + nc * d * d;
        }
    });
    if (threadIdx.x == 0) {
        const double n = (double)a.P, mo = (double)a.momentum;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t ch = 4 * (size_t)blockIdx.x + e;
            const double mean = div_ieee(acc[2 * e], n), d = mean - m0[e];
            const double m2 = fmax(acc[2 * e + 1] - n * d * d, 0.0);
            a.stats[2 * ch] = (float)mean;
            a.stats[2 * ch + 1] = (float)div_ieee(1.0, sqrt(div_ieee(m2, n) + (double)a.eps));
            if (a.running_mean) {
                a.running_mean[ch] = (float)((1.0 - mo) * (double)a.running_mean[ch] + mo * mean);
                a.running_var[ch] = (float)((1.0 - mo) * (double)a.running_var[ch] + mo * div_ieee(m2, n - 1.0));
            }
        }
    }
}

// MODE 0: y = z;  1: y = relu(z);  2: y = relu(z + res);  3: y = min(max(z, 0), 6)
template <int MODE>
__global__ __launch_bounds__(256) void k_bn_apply(const BnArgs a) {
    const int t = threadIdx.x, q = t % kBnQuads, r = t / kBnQuads;
    const int qg = blockIdx.y * kBnQuads + q;
    if (qg >= a.Q) return;
    const int p0 = blockIdx.x * kBnChunk, p1 = min(a.P, p0 + kBnChunk);
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.gamma + 4 * (size_t)qg), be = *reinterpret_cast<const f32x4*>(a.beta + 4 * (size_t)qg);
    const f32x4 st0 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg), st1 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg + 4);
    const f32x4 mean = {st0[0], st0[2], st1[0], st1[2]}, rstd = {st0[1], st0[3], st1[1], st1[3]};
#pragma unroll 4
    for (int p = p0 + r; p < p1; p += kBnRows) {
        const size_t o = (size_t)p * a.C + 4 * (size_t)qg;
        f32x4 z = (*reinterpret_cast<const f32x4*>(a.x + o) - mean) * rstd * g + be;
        if (MODE == 2) z += *reinterpret_cast<const f32x4*>(a.res + o);
        if (MODE >= 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) z[e] = MODE == 3 ? fminf(fmaxf(z[e], 0.f), 6.f) : fmaxf(z[e], 0.f);
        }
        *reinterpret_cast<f32x4*>(a.out + o) = z;
    }
}

// per channel of the chunk: sum g and sum g * xhat
__global__ __launch_bounds__(256) void k_bn_bwd_reduce(const BnArgs a) {
    __shared__ f32x4 red[2][256];
    const int t = threadIdx.x, q = t % kBnQuads, r = t / kBnQuads;
    const int chunk = blockIdx.x, qg = blockIdx.y * kBnQuads + q;
    const bool on = qg < a.Q;
    const int p0 = chunk * kBnChunk, p1 = min(a.P, p0 + kBnChunk);
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
    if (on) {
        const f32x4 st0 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg), st1 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg + 4);
        const f32x4 mean = {st0[0], st0[2], st1[0], st1[2]}, rstd = {st0[1], st0[3], st1[1], st1[3]};
#pragma unroll 4
        for (int p = p0 + r; p < p1; p += kBnRows) {
            const size_t o = (size_t)p * a.C + 4 * (size_t)qg;
            f32x4 g = *reinterpret_cast<const f32x4*>(a.dy + o);
            if (a.act) {
                const f32x4 y = *reinterpret_cast<const f32x4*>(a.y + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = (y[e] > 0.f && (a.act == 1 || y[e] < 6.f)) ? g[e] : 0.f;
            }
            const f32x4 xh = (*reinterpret_cast<const f32x4*>(a.x + o) - mean) * rstd;
            sa += g; sb += g * xh;
        }
    }
    red[0][t] = sa; red[1][t] = sb;
    __syncthreads();
    if (r == 0 && on) {
        float va[4], vb[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double da = 0.0, db = 0.0;
            for (int k = 0; k < kBnRows; ++k) { da += red[0][k * kBnQuads + q][e]; db += red[1][k * kBnQuads + q][e]; }
            va[e] = (float)da; vb[e] = (float)db;
        }
        float* o = a.part + ((size_t)chunk * a.C + 4 * (size_t)qg) * 2;
        *reinterpret_cast<f32x4*>(o) = f32x4{va[0], vb[0], va[1], vb[1]};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{va[2], vb[2], va[3], vb[3]};
    }
}

// dbeta, dgamma of the four channels of quad blockIdx.x
__global__ __launch_bounds__(256) void k_bn_bwd_finalize(const BnArgs a) {
    __shared__ double sh[4][8];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // {sum g, sum g xhat} x 4
    bn_fold(a, sh, acc, [](const f32x4 lo, const f32x4 hi, int, double* s) {
        s[0] += (double)lo[0]; s[1] += (double)lo[1]; s[2] += (double)lo[2]; s[3] += (double)lo[3];
        s[4] += (double)hi[0]; s[5] += (double)hi[1]; s[6] += (double)hi[2]; s[7] += (double)hi[3];
    });
    if (threadIdx.x == 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a.dbeta[4 * (size_t)blockIdx.x + e] = (float)acc[2 * e];
            a.dgamma[4 * (size_t)blockIdx.x + e] = (float)acc[2 * e + 1];
        }
    }
}

// dx and / or dres of one chunk
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const BnArgs a) {
    const int t = threadIdx.x, q = t % kBnQuads, r = t / kBnQuads;
    const int qg = blockIdx.y * kBnQuads + q;
    if (qg >= a.Q) return;
    const int p0 = blockIdx.x * kBnChunk, p1 = min(a.P, p0 + kBnChunk);
    const f32x4 st0 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg), st1 = *reinterpret_cast<const f32x4*>(a.stats + 8 * (size_t)qg + 4);
    const f32x4 mean = {st0[0], st0[2], st1[0], st1[2]}, rstd = {st0[1], st0[3], st1[1], st1[3]};
    const f32x4 db = *reinterpret_cast<const f32x4*>(a.dbeta + 4 * (size_t)qg), dg = *reinterpret_cast<const f32x4*>(a.dgamma + 4 * (size_t)qg);
    const f32x4 gr = *reinterpret_cast<const f32x4*>(a.gamma + 4 * (size_t)qg) * rstd;
    f32x4 m1, m2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { m1[e] = div_ieee(db[e], (float)a.P); m2[e] = div_ieee(dg[e], (float)a.P); }
#pragma unroll 4
    for (int p = p0 + r; p < p1; p += kBnRows) {
        const size_t o = (size_t)p * a.C + 4 * (size_t)qg;
        f32x4 g = *reinterpret_cast<const f32x4*>(a.dy + o);
        if (a.act) {
            const f32x4 y = *reinterpret_cast<const f32x4*>(a.y + o);
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = (y[e] > 0.f && (a.act == 1 || y[e] < 6.f)) ? g[e] : 0.f;
        }
        if (a.dres) *reinterpret_cast<f32x4*>(a.dres + o) = g;
        if (a.out) {
            const f32x4 xh = (*reinterpret_cast<const f32x4*>(a.x + o) - mean) * rstd;
            *reinterpret_cast<f32x4*>(a.out + o) = gr * (g - m1 - xh * m2);
        }
    }
}

static bool bn_bad16(const void* p) { return !p || ((uintptr_t)p & 15); }

static int bn_args(BnArgs& a, const float* x, const float* gamma, float* part, float* stats, int P, int C) {
    if (C < 4 || C % 4 != 0 || P < 2) return FPC_EINVAL;
    if (bn_bad16(x) || bn_bad16(gamma) || bn_bad16(part) || bn_bad16(stats)) return FPC_EINVAL;
    a.x = x; a.gamma = gamma; a.part = part; a.stats = stats;
    a.P = P; a.C = C; a.Q = C / 4; a.chunks = cdiv(P, kBnChunk);
    if (cdiv(a.Q, kBnQuads) > 65535) return FPC_EINVAL;
    return FPC_OK;
}

}  // namespace fpc

using namespace fpc;

// floats of scratch (`part`) for the forward or the backward of one call
extern "C" size_t fpc_batchnorm_scratch_floats(int P, int C) {
    return (P < 1 || C < 4) ? 0 : (size_t)cdiv(P, kBnChunk) * C * 2;
}

// act: 0 none, 1 ReLU, 2 ReLU6 (a residual goes with ReLU alone)
extern "C" int fpc_batchnorm_act_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, float* y, float* stats, float* part, int P, int C, float eps, float momentum,
                                     int act, fpc_stream_t stream) {
    if (act < 0 || act > 2) return FPC_EINVAL;
    BnArgs a{};
    int rc = bn_args(a, x, gamma, part, stats, P, C);
    if (rc) return rc;
    if (bn_bad16(beta) || bn_bad16(y) || (res && (((uintptr_t)res & 15) || act != 1))) return FPC_EINVAL;
    if (!running_mean != !running_var || ((uintptr_t)running_mean & 3) || ((uintptr_t)running_var & 3)) return FPC_EINVAL;
    a.res = res; a.beta = beta; a.out = y; a.running_mean = running_mean; a.running_var = running_var;
    a.eps = eps; a.momentum = momentum; a.act = act;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.chunks, cdiv(a.Q, kBnQuads));
    hipLaunchKernelGGL(k_bn_stats, grid, dim3(256), 0, s, a);
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_bn_finalize, dim3(a.Q), dim3(256), 0, s, a);
    rc = check_launch();
    if (rc) return rc;
    if (res) hipLaunchKernelGGL(k_bn_apply<2>, grid, dim3(256), 0, s, a);
    else if (act == 2) hipLaunchKernelGGL(k_bn_apply<3>, grid, dim3(256), 0, s, a);
    else if (act) hipLaunchKernelGGL(k_bn_apply<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_bn_apply<0>, grid, dim3(256), 0, s, a);
    return check_launch();
}

extern "C" int fpc_batchnorm_fwd(const float* x, const float* res, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, float* y, float* stats, float* part, int P, int C, float eps, float momentum,
                                 int relu, fpc_stream_t stream) {
    return fpc_batchnorm_act_fwd(x, res, gamma, beta, running_mean, running_var, y, stats, part, P, C, eps, momentum, relu != 0, stream);
}

extern "C" int fpc_batchnorm_act_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* stats, float* dx,
                                     float* dres, float* dgamma, float* dbeta, float* part, int P, int C, int act, fpc_stream_t stream) {
    if (act < 0 || act > 2) return FPC_EINVAL;
    BnArgs a{};
    int rc = bn_args(a, x, gamma, part, const_cast<float*>(stats), P, C);
    if (rc) return rc;
    if (bn_bad16(dy) || bn_bad16(dgamma) || bn_bad16(dbeta) || (act && bn_bad16(y))) return FPC_EINVAL;
    if (((uintptr_t)dx & 15) || ((uintptr_t)dres & 15) || (dres && act != 1)) return FPC_EINVAL;
    a.y = y; a.dy = dy; a.out = dx; a.dres = dres; a.dgamma = dgamma; a.dbeta = dbeta; a.act = act;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.chunks, cdiv(a.Q, kBnQuads));
    hipLaunchKernelGGL(k_bn_bwd_reduce, grid, dim3(256), 0, s, a);
    rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_bn_bwd_finalize, dim3(a.Q), dim3(256), 0, s, a);
    rc = check_launch();
    if (rc || (!dx && !dres)) return rc;
    hipLaunchKernelGGL(k_bn_bwd_apply, grid, dim3(256), 0, s, a);
    return check_launch();
}

extern "C" int fpc_batchnorm_bwd(const float* x, const float* y, const float* dy, const float* gamma, const float* stats, float* dx,
                                 float* dres, float* dgamma, float* dbeta, float* part, int P, int C, int relu, fpc_stream_t stream) {
    return fpc_batchnorm_act_bwd(x, y, dy, gamma, stats, dx, dres, dgamma, dbeta, part, P, C, relu != 0, stream);
}
