// net_kernels.hip — the small streaming kernels of the backbone engine (encoder + FPN decoders + heads), which replaces the
// torch/cuDNN op chain of PoseRegressor.pure_model_forward (F/lib/pose_regressor.py:709-743; encoder / FPNDecoder /
// SegmentationHead come from segmentation_models_pytorch, call sites :608-666) for inference.  The convolutions live in files of
// their own: conv_igemm.hip (implicit GEMM), wino_f32.hip and the wino_*.hip family (Winograd), pointwise.hip, lateral.hip, stem.hip.
//
//   k_maxpool3x3s2, k_gn_finalize, k_gn_relu_up2, k_merge_head, k_up4_compress: HBM-bound
//                       streaming kernels, lanes along the contiguous (channel or x) axis.
//   k_nchw3_to_nhwc4, k_fold_bn: the stem's input layout and the eval-mode BatchNorm fold (once per plan).
#include "conv_device.hpp"

namespace fpc {

// ------------------------------------------------------------------------------------------
// max pooling 3x3 stride 2, NHWC, one float4 of channels per thread.  PAD = 1: torchvision's stem pool (windows start at -1);
// PAD = 0: the SE-ResNet stem's MaxPool2d(3, 2, ceil_mode=True) — windows start at 2 i, Ho = Hi / 2, the last one clipped

template <int PAD>
__global__ __launch_bounds__(256) void k_maxpool3x3s2(const float* __restrict__ in, float* __restrict__ out, int B,
                                                      int Hi, int Wi, int C, int Ho, int Wo) {
    const unsigned C4 = C >> 2;
    const XcdSpan wk = xcd_walk((unsigned)B * Ho * Wo * C4);      // < 2^32: launch_maxpool3x3s2
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        int c4 = (int)(g % C4);
        unsigned r = g / C4;
        int wo = (int)(r % Wo); r /= Wo;
        int ho = (int)(r % Ho);
        int b = (int)(r / Ho);
        float4 m = make_float4(-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf());
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            int hi = ho * 2 - PAD + dy;
            if (hi < 0 || hi >= Hi) continue;
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                int wi = wo * 2 - PAD + dx;
                if (wi < 0 || wi >= Wi) continue;
                float4 v = *reinterpret_cast<const float4*>(in + (((size_t)b * Hi + hi) * Wi + wi) * C + 4 * c4);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        *reinterpret_cast<float4*>(out + (size_t)g * 4) = m;
    }
}

// ------------------------------------------------------------------------------------------
// GroupNorm statistics: partial sums -> per (image, channel) affine  y = x*a + b
// grid (groups, B, sites * kMaxGroup), 64 threads; fp64 combine in fixed order.  One launch serves every site whose
// statistics are complete (the four first segmentation blocks of a frame: one launch instead of four).

__global__ __launch_bounds__(64) void k_gn_finalize(const GnFinArgs a) {
    const int g = blockIdx.x, b = blockIdx.y, z = blockIdx.z;
    const int cpg = a.C / a.groups;
    const int site = z / kMaxGroup;
    const int P = a.P[site];
    const long long count = a.count[site];
    const float* part = a.gn_part[z] + (size_t)b * P * a.C * 2;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < P * cpg; i += 64) {
        int tile = i / cpg, c = g * cpg + (i - tile * cpg);
        const float* q = part + ((size_t)tile * a.C + c) * 2;
        s1 += (double)q[0]; s2 += (double)q[1];
    }
    s1 = wave_reduce_add(s1);
    s2 = wave_reduce_add(s2);
    s1 = __shfl(s1, 0, 64); s2 = __shfl(s2, 0, 64);
    double mean = s1 / (double)count;
    double var = s2 / (double)count - mean * mean;
    if (var < 0.0) var = 0.0;
    float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
    float fmean = (float)mean;
    if ((int)threadIdx.x < cpg) {
        int c = g * cpg + threadIdx.x;
        float ga = a.gamma[z][c], be = a.beta[z][c];
        float sa = rstd * ga;
        float* o = a.affine[z] + ((size_t)b * a.C + c) * 2;
        o[0] = sa;
        o[1] = be - fmean * sa;
    }
}

// Lerp / lerp_coord / lerp_scaled: net_kernels.hpp (shared with up4.hip)

__device__ __forceinline__ float4 gn_relu4(const float* p, float4 sa, float4 sb) {
    float4 v = *reinterpret_cast<const float4*>(p);
    v.x = fmaxf(v.x * sa.x + sb.x, 0.f); v.y = fmaxf(v.y * sa.y + sb.y, 0.f);
    v.z = fmaxf(v.z * sa.z + sb.z, 0.f); v.w = fmaxf(v.w * sa.w + sb.w, 0.f);
    return v;
}

__device__ __forceinline__ float4 bilerp4(float4 v00, float4 v01, float4 v10, float4 v11, Lerp ly, Lerp lx) {
    float4 r;
    r.x = ly.l0 * (lx.l0 * v00.x + lx.l1 * v01.x) + ly.l1 * (lx.l0 * v10.x + lx.l1 * v11.x);
    r.y = ly.l0 * (lx.l0 * v00.y + lx.l1 * v01.y) + ly.l1 * (lx.l0 * v10.y + lx.l1 * v11.y);
    r.z = ly.l0 * (lx.l0 * v00.z + lx.l1 * v01.z) + ly.l1 * (lx.l0 * v10.z + lx.l1 * v11.z);
    r.w = ly.l0 * (lx.l0 * v00.w + lx.l1 * v01.w) + ly.l1 * (lx.l0 * v10.w + lx.l1 * v11.w);
    return r;
}

// affine [B][C][2] interleaved (a, b): two float4 loads give (a0,b0,a1,b1),(a2,b2,a3,b3)
__device__ __forceinline__ void load_affine4(const float* aff, float4& sa, float4& sb) {
    float4 u = *reinterpret_cast<const float4*>(aff), v = *reinterpret_cast<const float4*>(aff + 4);
    sa = make_float4(u.x, u.z, v.x, v.z);
    sb = make_float4(u.y, u.w, v.y, v.w);
}

// GN + ReLU + x2 bilinear upsample (Conv3x3GNReLU with upsample=True), grid-stride, grid.y = job * kMaxGroup + group.
// A thread = one 2 x 2 output block x one channel quad (round 5; one output pixel before): the block's taps lie in a 3 x 3
// neighbourhood of the input (the align_corners scale is < 1/2), so 9 loads and GroupNorm + ReLU evaluations serve four
// outputs instead of 16, and the index arithmetic is 32-bit (the per-pixel form divided 64-bit indices three times per
// element).  Every output is the per-pixel expression on the same four operands, selected from the neighbourhood (as in
// k_merge_head): bit-identical.
__global__ __launch_bounds__(256) void k_gn_relu_up2(const GnUpArgs a) {
    const int z = blockIdx.y;
    const float* in = a.in[z];
    const float* aff = a.affine[z];
    float* out = a.out[z];
    const int job = z / kMaxGroup;
    const int ah = a.h[job], aw = a.w[job];
    const int C4 = a.C >> 2, H2 = 2 * ah, W2 = 2 * aw;
    const float sy = H2 > 1 ? (float)(ah - 1) / (float)(H2 - 1) : 0.f, sx = W2 > 1 ? (float)(aw - 1) / (float)(W2 - 1) : 0.f;
    const XcdSpan wk = xcd_walk((unsigned)a.B * ah * aw * C4);      // < 2^32: launch_gn_relu_up2; an XCD walks a band of rows
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned c4 = g % C4;
        unsigned r = g / C4;
        const int bx = (int)(r % aw); r /= aw;
        const int by = (int)(r % ah);
        const int b = (int)(r / ah);
        const int Y = 2 * by, X = 2 * bx;
        const Lerp lya = lerp_scaled(Y, ah, sy), lyb = lerp_scaled(Y + 1, ah, sy);
        const Lerp lxa = lerp_scaled(X, aw, sx), lxb = lerp_scaled(X + 1, aw, sx);
        const int rb = lya.i0, cb = lxa.i0;
        const bool sy1 = lyb.i0 != rb, sx1 = lxb.i0 != cb;  // the second row / column's first tap is the next one
        const int rr[3] = {rb, min(rb + 1, ah - 1), min(rb + 2, ah - 1)}, cc[3] = {cb, min(cb + 1, aw - 1), min(cb + 2, aw - 1)};
        float4 sa4, sb4;
        load_affine4(aff + ((size_t)b * a.C + 4 * c4) * 2, sa4, sb4);
        const f32x4 sa = {sa4.x, sa4.y, sa4.z, sa4.w}, sb = {sb4.x, sb4.y, sb4.z, sb4.w};      // native vectors: float4 structs selected by ?: land in scratch
        const float* base = in + (size_t)b * ah * aw * a.C + 4 * c4;
        auto gnr = [&](int i, int j) {
            f32x4 v = *reinterpret_cast<const f32x4*>(base + ((size_t)rr[i] * aw + cc[j]) * a.C) * sa + sb;
            v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
            return v;
        };
        const f32x4 t00 = gnr(0, 0), t01 = gnr(0, 1), t02 = gnr(0, 2), t10 = gnr(1, 0), t11 = gnr(1, 1), t12 = gnr(1, 2),
                    t20 = gnr(2, 0), t21 = gnr(2, 1), t22 = gnr(2, 2);
        float* o = out + (((size_t)b * H2 + Y) * W2 + X) * a.C + 4 * c4;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const Lerp ly = dy ? lyb : lya, lx = dx ? lxb : lxa;
                const bool sr = dy && sy1, sc = dx && sx1;
                // rows (r0, r0 + 1) and columns (c0, c0 + 1) of the neighbourhood
                const f32x4 a0 = sr ? t10 : t00, a1 = sr ? t11 : t01, a2 = sr ? t12 : t02;      // upper tap row
                const f32x4 b0 = sr ? t20 : t10, b1 = sr ? t21 : t11, b2 = sr ? t22 : t12;      // lower tap row
                const f32x4 v00 = sc ? a1 : a0, v01 = sc ? a2 : a1, v10 = sc ? b1 : b0, v11 = sc ? b2 : b1;
                // bilerp4's expression, component-wise
                const f32x4 res = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
                *reinterpret_cast<f32x4*>(o + ((size_t)dy * W2 + dx) * a.C) = res;
            }
    }
}

// ------------------------------------------------------------------------------------------
// FPN merge ("add" of the four segmentation blocks' outputs, smp MergeBlock) fused with the last
// GN+ReLU(+x2 upsample) of each branch and with the 1x1 segmentation head:
//   merged = up2(relu(gn(t5))) + up2(relu(gn(t4))) + up2(relu(gn(t3))) + relu(gn(t2))   (sum order of sum([...]))
//   logits_lowres[pixel][ch] = bias[ch] + sum_c merged[pixel][c] * W[ch][c]
// One workgroup = 32 pixels of one image (an 8 x 4 patch where the map divides into patches); merged tile and head weights live in LDS.
// Dropout2d is the identity in eval mode.  grid (ceil(H2*W2/64), B, G).
constexpr int kMhPx = 32;
constexpr int kMhMaxC = 128;
constexpr int kMhMaxCh = 32;

#ifdef FPC_STAMP_MH      // diagnostic build: summed phase ticks of lane 0 / wave 0 of every workgroup
__device__ unsigned long long g_mh[6];
#define FPC_MH_STAMP(I) do { if (threadIdx.x == 0) { long long n_ = clock64(); atomicAdd(&g_mh[I], (unsigned long long)(n_ - mh_t)); mh_t = n_; } } while (0)
#else
#define FPC_MH_STAMP(I) do { } while (0)
#endif

__global__ __launch_bounds__(256) void k_merge_head(const MergeHeadArgs a) {
#ifdef FPC_STAMP_MH
    long long mh_t = clock64();
#endif
    __shared__ __attribute__((aligned(16))) float s_m[kMhPx][kMhMaxC + 4];
    __shared__ __attribute__((aligned(16))) float s_w[kMhMaxCh][kMhMaxC + 4];
    const int z = blockIdx.z, b = blockIdx.y;
    const int H2 = 2 * a.h, W2 = 2 * a.w, C = a.C, C4 = C >> 2;
    const int ch = a.ch[z], chp = a.chp[z];
    // C4 divides 256 (C = 128): a thread's channel quad is fixed — no division inside the loops
    const int c4f = threadIdx.x % C4, prow = threadIdx.x / C4, pstep = 256 / C4;
    for (int r = prow; r < kMhMaxCh; r += pstep)            // rows past ch: zero (the MFMA tile is 32 wide)
        *reinterpret_cast<f32x4*>(&s_w[r][4 * c4f]) =
            r < ch ? *reinterpret_cast<const f32x4*>(a.hw[z] + (size_t)r * C + 4 * c4f) : f32x4{0.f, 0.f, 0.f, 0.f};
    const int p0 = blockIdx.x * kMhPx;
    // the thread's GroupNorm affines are loaded once
    f32x4 la[3], lb[3], ha, hb;
    {
        float4 sa, sb;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            load_affine4(a.a_lo[z][k] + ((size_t)b * C + 4 * c4f) * 2, sa, sb);
            la[k] = f32x4{sa.x, sa.y, sa.z, sa.w}; lb[k] = f32x4{sb.x, sb.y, sb.z, sb.w};
        }
        load_affine4(a.a_hi[z] + ((size_t)b * C + 4 * c4f) * 2, sa, sb);
        ha = f32x4{sa.x, sa.y, sa.z, sa.w}; hb = f32x4{sb.x, sb.y, sb.z, sb.w};
    }
    FPC_MH_STAMP(0);      // head weights -> LDS, affines
    auto gnr = [](const float* ptr, f32x4 sa, f32x4 sb) {
        f32x4 v = *reinterpret_cast<const f32x4*>(ptr) * sa + sb;
        v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f);
        return v;
    };
    // bilinear source scales (align_corners): computed once, same arithmetic as lerp_coord
    const float sy = H2 > 1 ? (float)(a.h - 1) / (float)(H2 - 1) : 0.f, sx = W2 > 1 ? (float)(a.w - 1) / (float)(W2 - 1) : 0.f;
    // the workgroup's 32 pixels: an 8 x 4 patch where the map divides into patches (its taps are 5 x 3 low-resolution pixels per
    // branch instead of the 17 x 2 of a 32-pixel row segment: less than half the L2 -> L1 bytes), else 32 consecutive pixels
    const bool patch = (W2 % 8 == 0) && (H2 % 4 == 0);
    const int tpr = W2 >> 3;                                 // patches per patch row
    const int y0 = patch ? 4 * (blockIdx.x / tpr) : p0 / W2, x0 = patch ? 8 * (blockIdx.x % tpr) : p0 - y0 * W2;      // workgroup-uniform
    if (patch && C4 == 32) {
        // a thread = one 2 x 2 output block of the patch x one channel quad.  The block's taps lie in a 3 x 3 low-resolution
        // neighbourhood (the x2 align_corners scale is < 1/2: the second row / column starts at most one tap later), so a
        // branch costs 9 loads and GroupNorm + ReLU evaluations for FOUR pixels instead of 16, and the horizontal lerp of a
        // tap row serves both output rows.  Every pixel's value is the expression of the per-pixel loop below on the same
        // operands, selected from the neighbourhood: bit-identical.
        const int blk = threadIdx.x >> 5, c4 = c4f;
        const int Y = y0 + 2 * (blk >> 2), X = x0 + 2 * (blk & 3);
        const Lerp lya = lerp_scaled(Y, a.h, sy), lyb = lerp_scaled(Y + 1, a.h, sy);
        const Lerp lxa = lerp_scaled(X, a.w, sx), lxb = lerp_scaled(X + 1, a.w, sx);
        const int rb = lya.i0, cb = lxa.i0;
        const bool sy1 = lyb.i0 != rb, sx1 = lxb.i0 != cb;  // the second row / column's first tap is the next one
        const int rr[3] = {rb, min(rb + 1, a.h - 1), min(rb + 2, a.h - 1)}, cc[3] = {cb, min(cb + 1, a.w - 1), min(cb + 2, a.w - 1)};
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i >> 1][i & 1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* base = a.t_lo[z][k] + (size_t)b * a.h * a.w * C + 4 * c4;
            f32x4 g[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) g[r][c] = gnr(base + ((size_t)rr[r] * a.w + cc[c]) * C, la[k], lb[k]);
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const Lerp lxx = dx ? lxb : lxa;
                const bool s = dx && sx1;
                f32x4 hrow[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) hrow[r] = lxx.l0 * (s ? g[r][1] : g[r][0]) + lxx.l1 * (s ? g[r][2] : g[r][1]);
                acc[0][dx] += lya.l0 * hrow[0] + lya.l1 * hrow[1];
                acc[1][dx] += lyb.l0 * (sy1 ? hrow[1] : hrow[0]) + lyb.l1 * (sy1 ? hrow[2] : hrow[1]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int dy = i >> 1, dx = i & 1;
            acc[dy][dx] += gnr(a.t_hi[z] + ((size_t)b * H2 * W2 + (size_t)(Y + dy) * W2 + X + dx) * C + 4 * c4, ha, hb);
            *reinterpret_cast<f32x4*>(&s_m[(2 * (blk >> 2) + dy) * 8 + 2 * (blk & 3) + dx][4 * c4]) = acc[dy][dx];
        }
    } else
#pragma unroll 2
    for (int pl = prow; pl < kMhPx; pl += pstep) {
        const int c4 = c4f;
        int p = patch ? (y0 + (pl >> 3)) * W2 + x0 + (pl & 7) : p0 + pl;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (p < H2 * W2) {
            int y = y0, x = x0 + pl;
            if (patch) { y = y0 + (pl >> 3); x = x0 + (pl & 7); }
            while (x >= W2) { x -= W2; ++y; }
            Lerp ly = lerp_scaled(y, a.h, sy), lx = lerp_scaled(x, a.w, sx);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float* base = a.t_lo[z][k] + (size_t)b * a.h * a.w * C + 4 * c4;
                f32x4 v00 = gnr(base + ((size_t)ly.i0 * a.w + lx.i0) * C, la[k], lb[k]);
                f32x4 v01 = gnr(base + ((size_t)ly.i0 * a.w + lx.i1) * C, la[k], lb[k]);
                f32x4 v10 = gnr(base + ((size_t)ly.i1 * a.w + lx.i0) * C, la[k], lb[k]);
                f32x4 v11 = gnr(base + ((size_t)ly.i1 * a.w + lx.i1) * C, la[k], lb[k]);
                acc += ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
            }
            acc += gnr(a.t_hi[z] + ((size_t)b * H2 * W2 + p) * C + 4 * c4, ha, hb);
        }
        *reinterpret_cast<f32x4*>(&s_m[pl][4 * c4]) = acc;
    }
    FPC_MH_STAMP(1);      // gather + GroupNorm + ReLU + bilinear merge
    __syncthreads();
    FPC_MH_STAMP(2);      // barrier
    // head (1x1 conv, C -> ch <= 32) on the matrix cores: the 32 px x 32 ch tile, K = C split over the four waves
    // (wave w owns channels [w C/4, (w+1) C/4)); A = merged activations, B = head weights, both read from LDS as
    // 16-byte fragments (2 x C/32 ds_read_b128 per wave — the scalar-FMA form needed ~900 wave-level LDS reads
    // per workgroup and was LDS-bound: 40 us for the four decoders).  Partials are summed in wave order.
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int kq = C >> 2;                                   // K range of a wave (C % 32 == 0, checked by the launcher)
    for (int k0 = wv * kq; k0 < (wv + 1) * kq; k0 += 8) {
        f32x4 fa = *reinterpret_cast<const f32x4*>(&s_m[li][k0 + 4 * lh]);
        f32x4 fb = *reinterpret_cast<const f32x4*>(&s_w[li][k0 + 4 * lh]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[e], acc, 0, 0, 0);
    }
    FPC_MH_STAMP(3);      // MFMA head
    __syncthreads();                                         // all fragments read: s_m becomes the partial buffer
    float* part = &s_m[0][0];                                // [4 waves][32 px][33]: 4224 floats = sizeof(s_m)
    static_assert(kMhPx * (kMhMaxC + 4) >= 4 * 32 * 33, "partial buffer");
#pragma unroll
    for (int r = 0; r < 16; ++r) part[(wv * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh) * 33 + li] = acc[r];
    __syncthreads();
    // the 32 pixels' outputs are one contiguous block of 32 * chp floats; 32 lanes per pixel (k < chp active)
    const int nvalid = patch ? kMhPx : min(kMhPx, H2 * W2 - p0);
    float* ob = a.out[z] + (size_t)b * H2 * W2 * chp;
    const int ok = threadIdx.x & 31;
    const float bias = ok < ch ? a.hb[z][ok] : 0.f;
    for (int pl = threadIdx.x >> 5; pl < nvalid; pl += 8) {
        if (ok >= chp) continue;
        float v = 0.f;
        if (ok < ch) {
            v = bias;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += part[(w * 32 + pl) * 33 + ok];
        }
        const int p = patch ? (y0 + (pl >> 3)) * W2 + x0 + (pl & 7) : p0 + pl;
        ob[(size_t)p * chp + ok] = v;
    }
    FPC_MH_STAMP(4);      // partial exchange + stores
#ifdef FPC_STAMP_MH
    if (threadIdx.x == 0) atomicAdd(&g_mh[5], 1ull);
#endif
}

#ifdef FPC_STAMP_MH
extern "C" int fpc_dbg_merge_head_stamps(unsigned long long* out6) {
    unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
    if (hipMemcpyFromSymbol(out6, HIP_SYMBOL(g_mh), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_mh), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

// ------------------------------------------------------------------------------------------
// x4 bilinear upsample (UpsamplingBilinear2d, align_corners=True) of the four heads' low-res
// logits to full resolution, the xyz -> xy / z channel split (pose_regressor.py:729-732) and
// class compression (pose_regressor.py:445-457, gpu_tensor_funcs.py:37-99) in one pass.
// One thread per output pixel, lanes along x: every full-res plane store is a coalesced
// 256-byte wave row; the low-res taps (5 MB in total) are served by L1/L2.

template <int MAXC>
__global__ __launch_bounds__(256) void k_up4_compress(const Up4Args a) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.W) return;
    const int HW = a.H * a.W, C = a.C, G = C - 1;
    const size_t p = (size_t)y * a.W + x;
    Lerp ly = lerp_coord(y, a.hl, a.H), lx = lerp_coord(x, a.wl, a.W);
    const size_t t00 = ((size_t)b * a.hl + ly.i0) * a.wl + lx.i0, t01 = ((size_t)b * a.hl + ly.i0) * a.wl + lx.i1;
    const size_t t10 = ((size_t)b * a.hl + ly.i1) * a.wl + lx.i0, t11 = ((size_t)b * a.hl + ly.i1) * a.wl + lx.i1;
    auto tap = [&](const float* L, int stride, int c) {
        return ly.l0 * (lx.l0 * L[t00 * stride + c] + lx.l1 * L[t01 * stride + c]) +
               ly.l1 * (lx.l0 * L[t10 * stride + c] + lx.l1 * L[t11 * stride + c]);
    };
    // mask logits + arg-max of the log-softmax (first maximal index on ties), as class_compress.hip
    float v[MAXC];
    float mx = -__builtin_huge_valf();
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) {
            v[c] = tap(a.lm, a.pm, c);
            mx = fmaxf(mx, v[c]);
            if (a.o_mask) a.o_mask[((size_t)b * C + c) * HW + p] = v[c];
        }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
        if (c < C) s += expf(v[c] - mx);
    float lse = logf(s);
    float best = (v[0] - mx) - lse;
    int cls = 0;
#pragma unroll
    for (int c = 1; c < MAXC; ++c)
        if (c < C) {
            float val = (v[c] - mx) - lse;
            if (val > best) { best = val; cls = c; }
        }
    a.cat_mask[(size_t)b * HW + p] = cls;
    if (a.fg_bits) {            // rows start on word boundaries (the host checked W % 64 == 0): a wave = one word
        const unsigned long long fgm = __ballot(cls != 0);
        if ((threadIdx.x & 63) == 0) a.fg_bits[(size_t)b * a.fg_stride + (p >> 6)] = fgm;
    }
    const int g = cls - 1;
    float q[4] = {0, 0, 0, 0}, sc[3] = {0, 0, 0}, vxy[2] = {0, 0}, zz = 0.f;
    for (int k = 0; k < G; ++k) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float u = tap(a.lq, a.pq, 4 * k + e);
            if (a.o_quat) a.o_quat[((size_t)b * 4 * G + 4 * k + e) * HW + p] = u;
            if (k == g) q[e] = u;
        }
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            float u = tap(a.ls, a.ps, 3 * k + e);
            if (a.o_scales) a.o_scales[((size_t)b * 3 * G + 3 * k + e) * HW + p] = u;
            if (k == g) sc[e] = u;
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float u = tap(a.lt, a.pt, 3 * k + e);
            if (a.o_xy) a.o_xy[((size_t)b * 2 * G + 2 * k + e) * HW + p] = u;
            if (k == g) vxy[e] = u;
        }
        float u = tap(a.lt, a.pt, 3 * k + 2);
        if (a.o_z) a.o_z[((size_t)b * G + k) * HW + p] = u;
        if (k == g) zz = u;
    }
    float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nq == 0.0f) nq = 1.0f;
    float nv = sqrtf(vxy[0] * vxy[0] + vxy[1] * vxy[1]);
    if (nv == 0.0f) nv = 1.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) a.cq[((size_t)b * 4 + e) * HW + p] = q[e] / nq;
#pragma unroll
    for (int e = 0; e < 3; ++e) a.cs[((size_t)b * 3 + e) * HW + p] = sc[e];
#pragma unroll
    for (int e = 0; e < 2; ++e) a.cxy[((size_t)b * 2 + e) * HW + p] = vxy[e] / nv;
    a.cz[(size_t)b * HW + p] = zz;
}

// The same for the reference's 7 classes (bg + 6): every channel index is a compile-time constant, so the
// four low-res taps are fetched as 18 float4 (channel strides 8 / 24 / 20 / 20, 16-byte aligned pixels)
// instead of 67 scalars each, and all 67 interpolated values stay in registers.
__global__ __launch_bounds__(256) void k_up4_compress7(const Up4Args a) {
    const int b = blockIdx.z, y = blockIdx.y;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.W) return;
    constexpr int C = 7, G = 6;
    const int HW = a.H * a.W;
    const size_t p = (size_t)y * a.W + x;
    Lerp ly = lerp_coord(y, a.hl, a.H), lx = lerp_coord(x, a.wl, a.W);
    const size_t t00 = ((size_t)b * a.hl + ly.i0) * a.wl + lx.i0, t01 = ((size_t)b * a.hl + ly.i0) * a.wl + lx.i1;
    const size_t t10 = ((size_t)b * a.hl + ly.i1) * a.wl + lx.i0, t11 = ((size_t)b * a.hl + ly.i1) * a.wl + lx.i1;
    auto quad = [&](const float* L, int stride, int q) {
        f32x4 v00 = *reinterpret_cast<const f32x4*>(L + t00 * stride + 4 * q);
        f32x4 v01 = *reinterpret_cast<const f32x4*>(L + t01 * stride + 4 * q);
        f32x4 v10 = *reinterpret_cast<const f32x4*>(L + t10 * stride + 4 * q);
        f32x4 v11 = *reinterpret_cast<const f32x4*>(L + t11 * stride + 4 * q);
        return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
    };
    float vm[8], vq[24], vt[20], vs[20];
#pragma unroll
    for (int q = 0; q < 2; ++q) { f32x4 r = quad(a.lm, 8, q); vm[4 * q] = r[0]; vm[4 * q + 1] = r[1]; vm[4 * q + 2] = r[2]; vm[4 * q + 3] = r[3]; }
#pragma unroll
    for (int q = 0; q < 6; ++q) { f32x4 r = quad(a.lq, 24, q); vq[4 * q] = r[0]; vq[4 * q + 1] = r[1]; vq[4 * q + 2] = r[2]; vq[4 * q + 3] = r[3]; }
#pragma unroll
    for (int q = 0; q < 5; ++q) { f32x4 r = quad(a.lt, 20, q); vt[4 * q] = r[0]; vt[4 * q + 1] = r[1]; vt[4 * q + 2] = r[2]; vt[4 * q + 3] = r[3]; }
#pragma unroll
    for (int q = 0; q < 5; ++q) { f32x4 r = quad(a.ls, 20, q); vs[4 * q] = r[0]; vs[4 * q + 1] = r[1]; vs[4 * q + 2] = r[2]; vs[4 * q + 3] = r[3]; }
    // arg-max of the log-softmax, first maximal index on ties (as class_compress.hip)
    float mx = vm[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mx = fmaxf(mx, vm[c]);
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) sum += expf(vm[c] - mx);
    float lse = logf(sum);
    float best = (vm[0] - mx) - lse;
    int cls = 0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
        float val = (vm[c] - mx) - lse;
        if (val > best) { best = val; cls = c; }
    }
    a.cat_mask[(size_t)b * HW + p] = cls;
    if (a.fg_bits) {            // rows start on word boundaries (the host checked W % 64 == 0): a wave = one word
        const unsigned long long fgm = __ballot(cls != 0);
        if ((threadIdx.x & 63) == 0) a.fg_bits[(size_t)b * a.fg_stride + (p >> 6)] = fgm;
    }
    if (a.o_mask) {
        // the 67 full-resolution logit planes (82 MB per frame) are the caller's output: nothing on this path reads them back,
        // so they go out as streaming stores (the categorical planes below are read by the aggregation next: ordinary stores)
#pragma unroll
        for (int c = 0; c < C; ++c) __builtin_nontemporal_store(vm[c], a.o_mask + ((size_t)b * C + c) * HW + p);
#pragma unroll
        for (int c = 0; c < 4 * G; ++c) __builtin_nontemporal_store(vq[c], a.o_quat + ((size_t)b * 4 * G + c) * HW + p);
#pragma unroll
        for (int c = 0; c < 3 * G; ++c) __builtin_nontemporal_store(vs[c], a.o_scales + ((size_t)b * 3 * G + c) * HW + p);
#pragma unroll
        for (int k = 0; k < G; ++k) {
            __builtin_nontemporal_store(vt[3 * k], a.o_xy + ((size_t)b * 2 * G + 2 * k) * HW + p);
            __builtin_nontemporal_store(vt[3 * k + 1], a.o_xy + ((size_t)b * 2 * G + 2 * k + 1) * HW + p);
            __builtin_nontemporal_store(vt[3 * k + 2], a.o_z + ((size_t)b * G + k) * HW + p);
        }
    }
    float q[4] = {0, 0, 0, 0}, sc[3] = {0, 0, 0}, vxy[2] = {0, 0}, zz = 0.f;
#pragma unroll
    for (int k = 0; k < G; ++k)
        if (k == cls - 1) {
            q[0] = vq[4 * k]; q[1] = vq[4 * k + 1]; q[2] = vq[4 * k + 2]; q[3] = vq[4 * k + 3];
            sc[0] = vs[3 * k]; sc[1] = vs[3 * k + 1]; sc[2] = vs[3 * k + 2];
            vxy[0] = vt[3 * k]; vxy[1] = vt[3 * k + 1]; zz = vt[3 * k + 2];
        }
    float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (nq == 0.0f) nq = 1.0f;
    float nv = sqrtf(vxy[0] * vxy[0] + vxy[1] * vxy[1]);
    if (nv == 0.0f) nv = 1.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) a.cq[((size_t)b * 4 + e) * HW + p] = q[e] / nq;
#pragma unroll
    for (int e = 0; e < 3; ++e) a.cs[((size_t)b * 3 + e) * HW + p] = sc[e];
#pragma unroll
    for (int e = 0; e < 2; ++e) a.cxy[((size_t)b * 2 + e) * HW + p] = vxy[e] / nv;
    a.cz[(size_t)b * HW + p] = zz;
}

// image NCHW [B,3,H,W] -> NHWC4 [B,H,W,4] (4th channel 0): 16-byte pixels for the stem's loader
__global__ __launch_bounds__(256) void k_nchw3_to_nhwc4(const float* __restrict__ x, float* __restrict__ out, int B,
                                                        int HW) {
    long long total = (long long)B * HW;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        long long b = g / HW, p = g - b * HW;
        const float* s = x + b * 3 * HW + p;
        *reinterpret_cast<f32x4*>(out + g * 4) = f32x4{s[0], s[HW], s[2 * (long long)HW], 0.f};
    }
}

// eval-mode BatchNorm as y = x*scale + shift (torch: (x - mean) / sqrt(var + eps) * gamma + beta)
__global__ void k_fold_bn(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean,
                          const float* __restrict__ var, float eps, int C, float* __restrict__ scale,
                          float* __restrict__ shift) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float inv = 1.0f / sqrtf(var[c] + eps);
    float s = gamma[c] * inv;
    scale[c] = s;
    shift[c] = beta[c] - mean[c] * s;
}

// ------------------------------------------------------------------------------------------
// launch wrappers

int launch_maxpool3x3s2(const float* in, float* out, int B, int Hi, int Wi, int C, int Ho, int Wo, hipStream_t s) {
    // (xcd_walk's 32-bit `first + k * step` must not wrap: one grid stride — at most 4096 x 256 items — of headroom below 2^32)
    if (C % 4 != 0 || (long long)B * Ho * Wo * (C / 4) >= kWalkLimit) return FPC_EINVAL;
    hipLaunchKernelGGL(k_maxpool3x3s2<1>, dim3(stream_grid((long long)B * Ho * Wo * (C / 4))), dim3(256), 0, s, in, out, B,
                       Hi, Wi, C, Ho, Wo);
    return check_launch();
}

// the pad-0 ceil-mode form: out [B][Hi / 2][Wi / 2][C] (torch's output size for every Hi, Wi >= 2: no window starts outside)
int launch_maxpool3x3s2_ceil(const float* in, float* out, int B, int Hi, int Wi, int C, hipStream_t s) {
    const int Ho = Hi / 2, Wo = Wi / 2;
    if (C % 4 != 0 || Hi < 2 || Wi < 2 || (long long)B * Ho * Wo * (C / 4) >= kWalkLimit) return FPC_EINVAL;
    hipLaunchKernelGGL(k_maxpool3x3s2<0>, dim3(stream_grid((long long)B * Ho * Wo * (C / 4))), dim3(256), 0, s, in, out, B,
                       Hi, Wi, C, Ho, Wo);
    return check_launch();
}

int launch_gn_finalize(const GnFinArgs& a, int groups, hipStream_t s) {
    if (a.C % a.groups != 0 || a.C / a.groups > 64) return FPC_EINVAL;
    if (a.sites < 1 || a.sites > kMaxGnSites || groups != kMaxGroup) return FPC_EINVAL;
    hipLaunchKernelGGL(k_gn_finalize, dim3(a.groups, a.B, a.sites * kMaxGroup), dim3(64), 0, s, a);
    return check_launch();
}

int launch_gn_relu_up2(const GnUpArgs& a, int groups, hipStream_t s) {
    if (a.C % 4 != 0) return FPC_EINVAL;
    if (a.jobs < 1 || a.jobs > kMaxUpJobs || groups != kMaxGroup) return FPC_EINVAL;
    long long most = 0;
    for (int j = 0; j < a.jobs; ++j) most = std::max(most, (long long)a.B * a.h[j] * a.w[j] * (a.C / 4));      // 2 x 2 blocks x channel quads
    if (most >= (1LL << 31)) return FPC_EINVAL;
    hipLaunchKernelGGL(k_gn_relu_up2, dim3(stream_grid(most), a.jobs * kMaxGroup), dim3(256), 0, s, a);
    return check_launch();
}

int launch_merge_head(const MergeHeadArgs& a, int groups, hipStream_t s) {
    if (a.C > kMhMaxC || a.C % 32 != 0 || 256 % (a.C / 4) != 0) return FPC_EINVAL;      // the head splits C over 4 waves in 8-channel steps
    for (int z = 0; z < groups; ++z)
        if (a.ch[z] > kMhMaxCh || a.chp[z] > kMhMaxCh || a.chp[z] < a.ch[z]) return FPC_EINVAL;
    hipLaunchKernelGGL(k_merge_head, dim3(cdiv(4 * a.h * a.w, kMhPx), a.B, groups), dim3(256), 0, s, a);
    return check_launch();
}

int launch_up4_compress(const Up4Args& a, hipStream_t s, bool allow_wide) {
    if (a.C < 2 || a.C > 32 || a.H > 65535 || a.B > 65535) return FPC_EINVAL;
    if (a.fg_bits && a.W % 64 != 0) return FPC_EINVAL;
    dim3 grid(cdiv(a.W, 256), a.H, a.B);
    const bool seven = a.C == 7 && a.pm == 8 && a.pq == 24 && a.pt == 20 && a.ps == 20;
    const bool all_or_none = (a.o_mask != nullptr) == (a.o_quat != nullptr) && (a.o_mask != nullptr) == (a.o_scales != nullptr) &&
                             (a.o_mask != nullptr) == (a.o_xy != nullptr) && (a.o_mask != nullptr) == (a.o_z != nullptr);
    if (seven && a.W % 4 == 0 && ((long long)a.H * a.W) % 256 == 0 && (long long)a.H * a.W < (1LL << 31) && all_or_none)
        launch_up4_compress7x4(a, s);
    else if (seven)
        hipLaunchKernelGGL(k_up4_compress7, dim3(cdiv(a.W, 128), a.H, a.B), dim3(128), 0, s, a);
    else if (a.C <= 8) hipLaunchKernelGGL(k_up4_compress<8>, grid, dim3(256), 0, s, a);
    // 9 to 32 classes: four pixels per thread (up4.hip) on a plan's own channel strides and a x4 map whose rows hold whole
    // thread quads and whose frames hold whole waves; any other shape, and FPC_UP4_WIDE=0, keep the one-pixel kernel
    else if (allow_wide && a.pm == (a.C + 3) / 4 * 4 && a.pq == 4 * (a.C - 1) && a.pt == (3 * (a.C - 1) + 3) / 4 * 4 && a.ps == a.pt &&
             a.H == 4 * a.hl && a.W == 4 * a.wl && ((long long)a.H * a.W) % 256 == 0 && (long long)a.H * a.W < (1LL << 31) &&
             (long long)a.hl * a.wl * a.pq < (1LL << 32) && all_or_none)
        launch_up4_compress_wide(a, s);
    else hipLaunchKernelGGL(k_up4_compress<32>, grid, dim3(256), 0, s, a);
    return check_launch();
}

int launch_nchw3_to_nhwc4(const float* x, float* out, int B, int HW, hipStream_t s) {
    hipLaunchKernelGGL(k_nchw3_to_nhwc4, dim3(stream_grid((long long)B * HW)), dim3(256), 0, s, x, out, B, HW);
    return check_launch();
}

int launch_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
                   float* scale, float* shift, hipStream_t s) {
    hipLaunchKernelGGL(k_fold_bn, dim3(cdiv(C, 256)), dim3(256), 0, s, gamma, beta, mean, var, eps, C, scale, shift);
    return check_launch();
}

}  // namespace fpc
