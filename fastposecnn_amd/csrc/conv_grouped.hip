// conv_grouped.hip — k_conv3x3_grouped: the grouped 3x3 convolution of the ResNeXt encoders (conv2 of every Bottleneck block,
// fastposecnn_amd/lib/backbone.py: Bottleneck with groups = 32), on channel-last f32 activations.
//
// out[b][oy][ox][c] = epilogue(sum over ky, kx and the CG input channels of c's group of in[b][s oy + ky - 1][s ox + kx - 1][g CG + ci]
// * w[c][ci][ky][kx]), pad 1, stride s = 1 or 2, groups = C / CG, CG in {4, 8, 16, 32, 64}; epilogue = per-channel scale / shift
// (folded BatchNorm) and ReLU, as the engine's other kernels.
//
// Products are plain f32 (v_fma_f32: exact f32 products, f32 accumulation) — the ONE form built (form 0).  A group is a block
// of a block-diagonal matrix; the vector unit wastes nothing on the zeros around it whatever CG is, and the f32 matrix
// instructions run at the vector rate on this chip, so they would buy nothing here (DESIGN.md 4.2a').
//
// Workgroup: a tile of 8 x TW output pixels (TW = 16 at stride 1, 8 at stride 2) x 32 output channels.  The input window of the
// tile (its 32 channels where CG <= 32; 32 channels of the group per pass where CG = 64) is staged in LDS by 16-byte loads that
// are contiguous over the 128 bytes of a pixel's channel slice, with zeros outside the image; a pixel takes 36 floats of LDS so
// that the four pixel quads of a wave start in different banks.  The weights of the 32 output channels come from an image
// k_pack_grouped writes once per plan in the order the kernel reads, [C / 32][pass][tap][ci][32 channels], in passes of KB =
// min(CG, 16) input channels (18 KB of LDS at most).  A thread owns 4 consecutive output channels (one 16-byte store) of 4
// consecutive pixels of a row: per (tap row, input-channel quad) it reads its 6 (stride 2: 9) input float4 and 12 weight float4
// from LDS and issues 192 FMAs.  The summation order is fixed (pass, ky, ci quad, kx, ci): no atomics, no split over K,
// results are bit-identical run to run.  Workgroups run in an XCD-aware order: with the grid a multiple of 8, XCD x takes the
// x-th contiguous eighth of the (frame, tile row, tile column, channel block) list, so tiles that share halo rows and the
// channel blocks of one tile meet in one L2.
#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr int kGrpCC = 32;      // output channels per workgroup
constexpr int kGrpTH = 8;       // output rows per tile
constexpr int kGrpPix = 36;     // floats per LDS pixel: 32 channels + 4 of padding

template <int CG, int STRIDE>
struct GrpGeom {
    static constexpr int TW = STRIDE == 1 ? 16 : 8;
    static constexpr int THREADS = (kGrpCC / 4) * kGrpTH * (TW / 4);
    static constexpr int KB = CG < 16 ? CG : 16;      // input channels per pass
    static constexpr int NPASS = CG / KB;
    static constexpr int IH = (kGrpTH - 1) * STRIDE + 3, IW = (TW - 1) * STRIDE + 3;
    static constexpr int NX = 3 * STRIDE + 3;         // input columns under a thread's 4 pixels
    static constexpr int IN_FLOATS = IH * IW * kGrpPix, W_FLOATS = 9 * KB * kGrpCC;
    static_assert((IN_FLOATS + W_FLOATS) * 4 <= 65536, "static LDS");
};

// torch's [C][CG][3][3] -> [C / 32][pass][tap][ci in pass][32].  mode 0: the forward's image.  mode 1: the image of the stride-1
// data gradient, W'[g CG + ci][co][ky][kx] = W[g CG + co][ci][2 - ky][2 - kx] (transposed inside each group and flipped), read
// straight from the OIHW source.  mode 2: transposed inside each group, taps as they are (k_conv3x3_grouped_dgrad_s2 names the
// forward's tap itself).
__global__ __launch_bounds__(256) void k_pack_grouped(const float* __restrict__ w, float* __restrict__ packed, int C, int CG, int mode) {
    const int KB = CG < 16 ? CG : 16, NPASS = CG / KB;
    const long long total = (long long)C * CG * 9;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int co = (int)(i & 31);
    long long r = i >> 5;
    const int k = (int)(r % KB); r /= KB;
    const int t = (int)(r % 9); r /= 9;
    const int pass = (int)(r % NPASS);
    const int chunk = (int)(r / NPASS);
    const int c = chunk * kGrpCC + co, ci = pass * KB + k;
    if (mode == 0) {
        packed[i] = w[((size_t)c * CG + ci) * 9 + t];
    } else {
        const int g = c / CG, cl = c - g * CG;
        packed[i] = w[((size_t)(g * CG + ci) * CG + cl) * 9 + (mode == 1 ? 8 - t : t)];
    }
}

template <int CG, int STRIDE>
__global__ __launch_bounds__((GrpGeom<CG, STRIDE>::THREADS)) void k_conv3x3_grouped(const GroupedArgs a) {
    using G = GrpGeom<CG, STRIDE>;
    constexpr int TW = G::TW, KB = G::KB, IW = G::IW, NX = G::NX;
    __shared__ __attribute__((aligned(16))) float s_in[G::IN_FLOATS];
    __shared__ __attribute__((aligned(16))) float s_w[G::W_FLOATS];
    const int tid = threadIdx.x;
    // XCD-banded order (conv_device.hpp; the launcher rounds every grid), the channel chunk fastest; the ids past the list leave before any barrier
    const int bid = (int)xcd_block_rounded();
    const int nchunk = a.C / kGrpCC;
    if (bid >= a.B * a.ty * a.tx * nchunk) return;
    const int chunk = bid % nchunk;
    int r = bid / nchunk;
    const int txi = r % a.tx; r /= a.tx;
    const int tyi = r % a.ty;
    const int b = r / a.ty;
    const int c0 = chunk * kGrpCC;
    const int oy0 = tyi * kGrpTH, ox0 = txi * TW;
    const int q = tid & 7, pq = tid >> 3, prow = pq / (TW / 4), pcol = pq % (TW / 4);
    const int kin = CG < 32 ? (4 * q / CG) * CG : 0;      // the thread's group inside the 32 staged channels

    f32x4 acc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) acc[p] = f32x4{0.f, 0.f, 0.f, 0.f};

    const float* wimg = a.w + (size_t)chunk * G::NPASS * G::W_FLOATS;
    const float* inb = a.in + (long long)b * a.in_sb;
    const int gy0 = oy0 * STRIDE - 1, gx0 = ox0 * STRIDE - 1;
#pragma unroll 1
    for (int pass = 0; pass < G::NPASS; ++pass) {
        if (pass > 0) __syncthreads();      // the previous pass is read out
        if ((pass * KB) % 32 == 0) {        // the window of the next 32 input channels (CG <= 32: once)
            const int cin0 = CG <= 32 ? c0 : (c0 / CG) * CG + pass * KB;
            for (int i = tid; i < G::IH * IW * 8; i += G::THREADS) {
                const int pix = i >> 3, c4 = i & 7, iy = pix / IW, ix = pix - iy * IW;
                const int gy = gy0 + iy, gx = gx0 + ix;
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (gy >= 0 && gy < a.Hi && gx >= 0 && gx < a.Wi)
                    v = *reinterpret_cast<const f32x4*>(inb + (long long)gy * a.in_sh + (long long)gx * a.in_sw + cin0 + 4 * c4);
                *reinterpret_cast<f32x4*>(s_in + pix * kGrpPix + 4 * c4) = v;
            }
        }
        for (int i = tid; i < G::W_FLOATS / 4; i += G::THREADS)
            *reinterpret_cast<f32x4*>(s_w + 4 * i) = *reinterpret_cast<const f32x4*>(wimg + (size_t)pass * G::W_FLOATS + 4 * i);
        __syncthreads();
        const int koff = CG < 32 ? kin : (pass * KB) & 31;
#pragma unroll 1
        for (int ky = 0; ky < 3; ++ky) {
            const float* rowp = s_in + ((prow * STRIDE + ky) * IW + pcol * 4 * STRIDE) * kGrpPix + koff;
#pragma unroll
            for (int j = 0; j < KB / 4; ++j) {
                f32x4 x[NX];
#pragma unroll
                for (int i = 0; i < NX; ++i) x[i] = *reinterpret_cast<const f32x4*>(rowp + i * kGrpPix + 4 * j);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(s_w + ((ky * 3 + kx) * KB + 4 * j + c) * kGrpCC + 4 * q);
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            const float xv = x[p * STRIDE + kx][c];
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[p][e] = __builtin_fmaf(xv, w[e], acc[p][e]);
                        }
                    }
            }
        }
    }

    const int c = c0 + 4 * q, oy = oy0 + prow;
    if (oy >= a.Ho) return;
    f32x4 sc = f32x4{1.f, 1.f, 1.f, 1.f}, sh = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.scale) sc = *reinterpret_cast<const f32x4*>(a.scale + c);
    if (a.shift) sh = *reinterpret_cast<const f32x4*>(a.shift + c);
    float* orow = a.out + (((long long)b * a.Ho + oy) * a.Wo) * a.C + c;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int ox = ox0 + pcol * 4 + p;
        if (ox >= a.Wo) continue;
        f32x4 v = acc[p];
        if (a.scale) v = v * sc;
        if (a.shift) v = v + sh;
        if (a.relu) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
        }
        *reinterpret_cast<f32x4*>(orow + (long long)ox * a.C) = v;
    }
}

template <int CG, int STRIDE>
int launch_grouped_t(GroupedArgs a, hipStream_t s) {
    using G = GrpGeom<CG, STRIDE>;
    a.tx = cdiv(a.Wo, G::TW);
    a.ty = cdiv(a.Ho, kGrpTH);
    const long long blocks = (long long)a.B * a.ty * a.tx * (a.C / kGrpCC);
    if (blocks < 1 || blocks > (1LL << 30)) return FPC_EINVAL;
    const unsigned grid = (unsigned)xcd_grid(blocks < 8 ? 8 : blocks);      // always banded: at least 8 workgroups
    hipLaunchKernelGGL((k_conv3x3_grouped<CG, STRIDE>), dim3(grid), dim3(G::THREADS), 0, s, a);
    return check_launch();
}

}  // namespace

bool grouped_cg_ok(int cg) { return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64; }

int launch_pack_grouped(const float* w, float* packed, int C, int CG, hipStream_t s, int mode) {
    if (!w || !packed || C < 32 || C % 32 || !grouped_cg_ok(CG) || C % CG || mode < 0 || mode > 2) return FPC_EINVAL;
    const long long total = (long long)C * CG * 9;
    hipLaunchKernelGGL(k_pack_grouped, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w, packed, C, CG, mode);
    return check_launch();
}

int launch_conv3x3_grouped(const GroupedArgs& a, hipStream_t s) {
    if (!a.in || !a.w || !a.out || !al16(a.in) || !al16(a.w) || !al16(a.out) || !al16(a.scale) || !al16(a.shift) || a.form != 0 ||
        a.B < 1 || a.Hi < 1 || a.Wi < 1 || a.C < 32 || a.C % 32 || !grouped_cg_ok(a.CG) || a.C % a.CG ||
        (a.stride != 1 && a.stride != 2) || (a.in_sb | a.in_sh | a.in_sw) % 4 || a.in_sw < a.C)
        return FPC_EINVAL;
    if (a.Ho != (a.Hi - 1) / a.stride + 1 || a.Wo != (a.Wi - 1) / a.stride + 1) return FPC_EINVAL;
    if ((long long)a.B * a.Ho * a.Wo * a.C >= (1LL << 40)) return FPC_EINVAL;
#define FPC_GRP_CASE(cg)                                                                               \
    case cg: return a.stride == 1 ? launch_grouped_t<cg, 1>(a, s) : launch_grouped_t<cg, 2>(a, s);
    switch (a.CG) {
        FPC_GRP_CASE(4)
        FPC_GRP_CASE(8)
        FPC_GRP_CASE(16)
        FPC_GRP_CASE(32)
        FPC_GRP_CASE(64)
    }
#undef FPC_GRP_CASE
    return FPC_EINVAL;
}

}  // namespace fpc
