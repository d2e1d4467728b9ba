// pointwise.hip — k_conv1x1: a 1x1 convolution on channel-last activations as a plain GEMM, for the Bottleneck encoders'
// 1x1 sites (conv1, conv3, the stride-1 / stride-2 downsample) and the FPN laterals of their wide maps
// (fastposecnn_amd/lib/backbone.py: Bottleneck, FPNBlock).
//
// out[m][n] = sum_k in[row(m)][k] * w[n][k] over M = B * Ho * Wo output pixels (tiles cross image boundaries: layer4 of a
// 640 x 480 frame has 300 pixels per image), N = Cout per group (the four decoders' laterals share one input: groups = 4) and
// K = Cin, a multiple of 64.  Output pixel (b, ho, wo) reads input row (b, s ho, s wo), s = 1 or 2.
//
// Products are the engine's exact bf16 x 3 split with f32 accumulation, the contract of k_conv_igemm's split form: the weight
// operand is k_pack_weight_bf3's three planes ([plane][Npad][Kpad] bf16, no new image), activations are split in registers
// after staging (common.hpp: split_bf3), six v_mfma_f32_32x32x16_bf16 per 16-deep k-group (the piece products p_i q_j with
// i + j <= 4, smallest first).
//
// Tile: BM = 32 WM pixels x 64 channels, 2 WM waves of one 32 x 32 product each (variant 0: WM = 2, 4 waves, 2 workgroups per
// CU; variant 1: WM = 4, 8 waves, 1).  K-step 64: per step the f32 activation rows (BM x 256 B) and the three weight planes
// (3 x 64 x 128 B) go global -> LDS by 16-byte global_load_lds into the other half of a double-buffered image while this half feeds the MFMAs.
// The DMA writes LDS lane-linearly, so the XOR swizzle sits on the per-lane SOURCE address: activation row r keeps its 16-byte
// chunk c in slot c ^ (r & 15) of its 256-byte row, weight row n in slot c ^ ((n >> 1) & 7) of its 128-byte row — every
// ds_read_b128 group of 16 lanes then touches 16 different slots of a bank row (the lateral kernel's layout, lateral.hip).
// The MFMA puts channels on the accumulator rows and pixels on the lanes: a lane holds four consecutive channels of one pixel
// per register quad, so the epilogue (folded BatchNorm or bias, residual, nearest-x2 top-down addend, ReLU) loads and stores
// 16 bytes per lane.  Workgroups run in an XCD-aware order (channel tiles of one pixel tile on one XCD: the activation rows
// are fetched into one L2).  No atomics, no split over K: the summation order is fixed, results are bit-identical run to run.
#include "conv_device.hpp"

namespace fpc {

namespace {

#define FPC_GLOBAL(p) ((const __attribute__((address_space(1))) void*)(p))
#define FPC_LOCAL(p) ((__attribute__((address_space(3))) void*)(p))

template <int WM>
__global__ __launch_bounds__(128 * WM) void k_conv1x1(const PwArgs a) {
    constexpr int BM = 32 * WM, NW = 2 * WM;
    constexpr int ABYTES = BM * 256, BBYTES = 3 * 64 * 128, BUFB = ABYTES + BBYTES;
    constexpr int NA = ABYTES / 1024 / NW, NB = BBYTES / 1024 / NW;      // 16-byte DMA instructions per wave and K-step
    static_assert(NA * NW * 1024 == ABYTES && NB * NW * 1024 == BBYTES, "DMA share per wave");
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * BUFB];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wv & 1, wm = wv >> 1;
    const int HoWo = a.Ho * a.Wo, M = a.B * HoWo;
    const int ntg = a.Cout >> 6, nt = a.groups * ntg;
    // XCD-banded order (conv_device.hpp): the channel tiles of one pixel tile (the fast index) share an L2 for the activation rows
    const int bid = (int)xcd_block();
    const int tn = bid % nt, tm = bid / nt;
    const int d = tn / ntg, n0 = (tn - d * ntg) * 64, m0 = tm * BM;

    // ---- per-lane DMA sources: activation rows (pixel rows past M re-read the last pixel: finite, never stored)
    const float* asrc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int q = (wv * NA + i) * 64 + lane, row = q >> 4, gc = (q & 15) ^ (row & 15);
        const int m = min(m0 + row, M - 1), b = m / HoWo, p = m - b * HoWo, ho = p / a.Wo, wo = p - ho * a.Wo;
        asrc[i] = a.in + (long long)b * a.in_sb + (long long)(ho * a.stride) * a.in_sh + (long long)(wo * a.stride) * a.in_sw + 4 * gc;
    }
    const unsigned short* bsrc[NB];
    const unsigned short* wpl = a.wpl[d];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int q = (wv * NB + i) * 64 + lane, plane = q >> 9, n = (q >> 3) & 63, gc = (q & 7) ^ ((n >> 1) & 7);
        bsrc[i] = wpl + ((size_t)plane * a.Npad + n0 + n) * a.Kpad + 8 * gc;
    }
    auto issue = [&](int buf) {
        unsigned char* base = lds + buf * BUFB;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            __builtin_amdgcn_global_load_lds(FPC_GLOBAL(asrc[i]), FPC_LOCAL(base + (wv * NA + i) * 1024), 16, 0, 0);
            asrc[i] += 64;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            __builtin_amdgcn_global_load_lds(FPC_GLOBAL(bsrc[i]), FPC_LOCAL(base + ABYTES + (wv * NB + i) * 1024), 16, 0, 0);
            bsrc[i] += 64;
        }
    };

    // ---- fragment addresses inside one buffer: activation row wm * 32 + r, weight row wn * 32 + r
    const int arow = (wm * 32 + r) * 256, asw = r & 15;
    const int wrow = ABYTES + (wn * 32 + r) * 128, wsw = ((wn * 32 + r) >> 1) & 7;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    const int nks = a.Kpad >> 6;
    issue(0);
    for (int ks = 0; ks < nks; ++ks) {
        const int buf = ks & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this step's DMA has landed (own share) ...
        __syncthreads();                                       // ... everybody's, and the other buffer is read out
        if (ks + 1 < nks) issue(buf ^ 1);
        const unsigned char* sb = lds + buf * BUFB;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 4 * g + 2 * h;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(sb + arow + ((c ^ asw) << 4));
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(sb + arow + (((c + 1) ^ asw) << 4));
            const int o = wrow + (((2 * g + h) ^ wsw) << 4);
            const bf16x8 w1 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(sb + o));
            const bf16x8 w2 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(sb + 8192 + o));
            const bf16x8 w3 = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(sb + 16384 + o));
            u32x2 p1, p2, p3, q1, q2, q3;
            split_bf3(v0, p1, p2, p3);
            split_bf3(v1, q1, q2, q3);
            const bf16x8 x1 = __builtin_bit_cast(bf16x8, u32x4{p1[0], p1[1], q1[0], q1[1]});
            const bf16x8 x2 = __builtin_bit_cast(bf16x8, u32x4{p2[0], p2[1], q2[0], q2[1]});
            const bf16x8 x3 = __builtin_bit_cast(bf16x8, u32x4{p3[0], p3[1], q3[0], q3[1]});
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x3, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w3, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, x2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w2, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w1, x1, acc, 0, 0, 0);
        }
    }

    // ---- epilogue: accumulator register 4 j + e = channel n0 + wn * 32 + 8 j + 4 h + e of pixel m
    const int m = m0 + wm * 32 + r;
    if (m >= M) return;
    const int cb = n0 + wn * 32 + 4 * h;
    const size_t orow = (size_t)m * a.Cout;
    size_t urow = 0;
    if (a.has_up) {
        const int b = m / HoWo, p = m - b * HoWo, ho = p / a.Wo, wo = p - ho * a.Wo;
        urow = (((size_t)b * (a.Ho >> 1) + (ho >> 1)) * (a.Wo >> 1) + (wo >> 1)) * a.Cout;
    }
    float* out = a.out[d];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = cb + 8 * j;
        f32x4 x = {acc[4 * j], acc[4 * j + 1], acc[4 * j + 2], acc[4 * j + 3]};
        if (a.has_scale) x = x * *reinterpret_cast<const f32x4*>(a.scale[d] + n);
        if (a.has_shift) x = x + *reinterpret_cast<const f32x4*>(a.shift[d] + n);
        if (a.has_res) x += *reinterpret_cast<const f32x4*>(a.res[d] + orow + n);
        if (a.has_up) x += *reinterpret_cast<const f32x4*>(a.up[d] + urow + n);
        if (a.relu) { x[0] = fmaxf(x[0], 0.f); x[1] = fmaxf(x[1], 0.f); x[2] = fmaxf(x[2], 0.f); x[3] = fmaxf(x[3], 0.f); }
        *reinterpret_cast<f32x4*>(out + orow + n) = x;
    }
}

#undef FPC_GLOBAL
#undef FPC_LOCAL

}  // namespace

int launch_conv1x1(const PwArgs& a, hipStream_t s) {
    if (a.variant < 0 || a.variant > 1 || a.groups < 1 || a.groups > kMaxGroup || a.B < 1 || a.Ho < 1 || a.Wo < 1 ||
        (a.stride != 1 && a.stride != 2) || a.Cin < 64 || a.Cin % 64 != 0 || a.Kpad != a.Cin || a.Cout < 64 ||
        a.Cout % 64 != 0 || a.Npad < a.Cout || !a.in || !al16(a.in) || (a.in_sw & 3) || (a.in_sh & 3) || (a.in_sb & 3) ||
        a.in_sw < a.Cin)
        return FPC_EINVAL;
    if ((long long)a.B * a.Ho * a.Wo >= (1LL << 31) || (long long)(a.Ho - 1) * a.stride * a.in_sh >= (1LL << 31) ||
        (long long)(a.Wo - 1) * a.stride * a.in_sw >= (1LL << 31))
        return FPC_EINVAL;
    if (a.has_up && ((a.Ho | a.Wo) & 1)) return FPC_EINVAL;
    for (int g = 0; g < a.groups; ++g) {
        // every group has the same epilogue operands (flags), 16-byte aligned
        if (!a.wpl[g] || !al16(a.wpl[g]) || !a.out[g] || !al16(a.out[g]) || (a.scale[g] != nullptr) != (a.has_scale != 0) ||
            (a.shift[g] != nullptr) != (a.has_shift != 0) || (a.res[g] != nullptr) != (a.has_res != 0) ||
            (a.up[g] != nullptr) != (a.has_up != 0) || !al16(a.scale[g]) || !al16(a.shift[g]) || !al16(a.res[g]) || !al16(a.up[g]))
            return FPC_EINVAL;
    }
    const int bm = pw_tile_pixels(a.variant);
    const long long grid = (long long)((a.B * a.Ho * a.Wo + bm - 1) / bm) * a.groups * (a.Cout / 64);
    if (grid >= (1LL << 31)) return FPC_EINVAL;
    if (a.variant == 0) hipLaunchKernelGGL((k_conv1x1<2>), dim3((unsigned)grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_conv1x1<4>), dim3((unsigned)grid), dim3(512), 0, s, a);
    return check_launch();
}

}  // namespace fpc
