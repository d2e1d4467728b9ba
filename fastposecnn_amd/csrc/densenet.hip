// densenet.hip — the kernels of the DenseNet encoders (torchvision's DenseNet.features as smp wraps it: lib/backbone.py
// DenseNetEncoder), for inference.  Activations are channel-last f32; a block's layers share ONE concatenation buffer
// [pixels][C_end], so the kernels here take ROW PITCHES: a 1x1 reads the channel prefix [0, K) of rows ldi apart and nothing at or
// behind channel K (later layers' data, or nothing yet, lies there), a 3x3 writes the 32 channels [c0, c0 + 32) of rows ldo apart
// and nothing else.  BatchNorm arrives folded as per-channel scale / shift.  Exact f32 products on v_mfma_f32_32x32x2_f32 /
// v_mfma_f32_16x16x4_f32 with f32 accumulation, no atomics, every sum in an order the shape (and the form) alone fixes: two
// launches agree bit for bit.  No kernel divides a float.
//
//   k_dense_pw32 / k_dense_pw16   the pre-activated 1x1: out[m][n] = act(s2[n] sum_k pre(in[m][k]) w[n][k] + t2[n]) with
//                  pre(v) = max(s1[k] v + t1[k], 0) (norm1 + relu1 of a dense layer) applied to the operand as it arrives, rounded
//                  to f32 before it enters the matrix instruction.  Kernels of their own, not instantiations of mobilenet.hip's
//                  k_conv1x1_f32: those address rows Cin apart, clamp channels past Cout and take K-steps of 8; here K and Cout are
//                  multiples of 32, so there are no tails at all and the two pitches and the prologue's operand set are the whole
//                  difference.  Same lane layouts and the same two-set software pipeline: both operands straight from memory, a
//                  16-byte load feeds four instructions, the next K-step of 32's loads in flight under the current one's MFMAs.
//                  pw32: one wave per 32 x 32 tile, no LDS, no barrier.  pw16, for few rows: a workgroup per 16 x 16 tile, K split
//                  over its four waves and added through LDS in wave order.
//   k_dense_conv3_tile / _split   the 3x3 / pad 1 / stride 1 of 128 -> 32 channels as an implicit GEMM of K = 9 x 128 over a
//                  weight image re-laid at load time to [tap][32][128] (k_dense_pack_w), streamed tap by tap from L2.
//                  _tile: one wave per 64 pixels x 32 channels (two 32 x 32 tiles share every weight load), 1152 instructions.
//                  _split, for few pixels: a workgroup of nine waves per 16 pixels; wave = tap sums its tap's 128 channels for both
//                  16-channel halves on 16 x 16 x 4 tiles (64 instructions and one memory round trip instead of a chain of 576
//                  and 36), taps 1 .. 8 hand their partial tiles over through LDS and wave 0 adds them in tap order.
//   k_dense_norm_pool   skip = act(s x + t) and, for a transition, the 2 x 2 mean of skip in the order 0.25 ((a + b) + (c + d)).
//   k_dense_place  the pooled stem [M][C] into channels [0, C) of block 1's buffer: a pitched copy.
#include "conv_device.hpp"

namespace fpc {

namespace {

__device__ __forceinline__ f32x4 pre_act(f32x4 v, f32x4 s, f32x4 t) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaxf(s[e] * v[e] + t[e], 0.f);
    return r;
}

}  // namespace

// in rows ldi apart, w [Cout][K], out rows ldo apart; waves = mtiles * ntiles, the channel tile fastest.  K % 32 == 0, Cout % 32 == 0.
// Lane l holds row / channel l & 31 and k = k0 + 4 (l >> 5) + e of a K-step of 8; four K-steps per operand set, two sets in turn.
template <bool PRE>
__global__ __launch_bounds__(256) void k_dense_pw32(const float* __restrict__ in, const float* __restrict__ s1, const float* __restrict__ t1,
                                                    const float* __restrict__ w, const float* __restrict__ s2, const float* __restrict__ t2,
                                                    float* __restrict__ out, unsigned M, int K, int ldi, int ldo, int act,
                                                    unsigned mtiles, unsigned ntiles) {
    const unsigned lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const unsigned wid = xcd_block() * 4 + (threadIdx.x >> 6);
    if (wid >= mtiles * ntiles) return;      // (no barrier in this kernel)
    const unsigned nt = wid % ntiles, mt = wid / ntiles, m0 = mt * 32, n0 = nt * 32;
    const float* pa = in + (size_t)min(m0 + li, M - 1) * ldi + 4 * lh;      // a row past M loads the last valid one; never written
    const float* pb = w + (size_t)(n0 + li) * K + 4 * lh;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    struct Set { f32x4 a[4], b[4], s[4], t[4]; };
    Set x0, x1;
    auto load_set = [&](Set& x, int k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x.a[j] = *reinterpret_cast<const f32x4*>(pa + k + 8 * j);
            x.b[j] = *reinterpret_cast<const f32x4*>(pb + k + 8 * j);
            if constexpr (PRE) {
                x.s[j] = *reinterpret_cast<const f32x4*>(s1 + k + 8 * j + 4 * lh);
                x.t[j] = *reinterpret_cast<const f32x4*>(t1 + k + 8 * j + 4 * lh);
            }
        }
    };
    auto mma_set = [&](const Set& x) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            f32x4 a = x.a[j];
            if constexpr (PRE) a = pre_act(a, x.s[j], x.t[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], x.b[j][e], acc, 0, 0, 0);
        }
    };
    const int iters = K >> 5;
    load_set(x0, 0);
    int it = 0;
    for (; it + 2 <= iters; it += 2) {
        load_set(x1, (it + 1) * 32);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x0);
        __builtin_amdgcn_sched_barrier(0);
        load_set(x0, (it + 2 < iters ? it + 2 : it + 1) * 32);      // (behind the last pair: a set nobody reads, inside [0, K))
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (it < iters) mma_set(x0);
    // C/D layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    const unsigned nn = n0 + li;
    const float sc = s2 ? s2[nn] : 1.f, sh = s2 ? t2[nn] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        float v = s2 ? acc[r] * sc + sh : acc[r];
        if (act) v = fmaxf(v, 0.f);
        if (m < M) out[(size_t)m * ldo + nn] = v;
    }
}

// The same product on 16 x 16 tiles for a site with few rows, where a wave per tile would be a chain of K / 32 dependent memory
// round trips on a mostly idle chip: a WORKGROUP per tile, its four waves taking the operand sets (32 channels of K each) in turn —
// wave v the sets v, v + 4, ... — and the partial tiles of waves 1 .. 3 handed over through LDS; wave 0 stores ((p0 + p1) + p2) + p3.
// Lane l holds row / channel l & 15 and k = k0 + 4 (l >> 4) + e of a K-step of 16; two K-steps per operand set, a wave's sets two
// at a time in turn; two accumulators take the K-steps in turn and are added at the end.
template <bool PRE>
__global__ __launch_bounds__(256) void k_dense_pw16(const float* __restrict__ in, const float* __restrict__ s1, const float* __restrict__ t1,
                                                    const float* __restrict__ w, const float* __restrict__ s2, const float* __restrict__ t2,
                                                    float* __restrict__ out, unsigned M, int K, int ldi, int ldo, int act,
                                                    unsigned mtiles, unsigned ntiles) {
    __shared__ f32x4 part[3][64];
    const unsigned lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, wave = threadIdx.x >> 6;
    const unsigned wid = xcd_block();
    if (wid >= mtiles * ntiles) return;      // (the whole workgroup leaves: nobody waits at the barrier below)
    const unsigned nt = wid % ntiles, mt = wid / ntiles, m0 = mt * 16, n0 = nt * 16;
    const float* pa = in + (size_t)min(m0 + li, M - 1) * ldi + 4 * g;
    const float* pb = w + (size_t)(n0 + li) * K + 4 * g;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    struct Set { f32x4 a[2], b[2], s[2], t[2]; };
    Set x0, x1;
    auto load_set = [&](Set& x, int k) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            x.a[j] = *reinterpret_cast<const f32x4*>(pa + k + 16 * j);
            x.b[j] = *reinterpret_cast<const f32x4*>(pb + k + 16 * j);
            if constexpr (PRE) {
                x.s[j] = *reinterpret_cast<const f32x4*>(s1 + k + 16 * j + 4 * g);
                x.t[j] = *reinterpret_cast<const f32x4*>(t1 + k + 16 * j + 4 * g);
            }
        }
    };
    auto mma_set = [&](const Set& x) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 a = x.a[j];
            if constexpr (PRE) a = pre_act(a, x.s[j], x.t[j]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], x.b[j][e], acc[j], 0, 0, 0);
        }
    };
    const int iters = K >> 5, mine = ((int)wave < iters) ? (iters - (int)wave + 3) >> 2 : 0;      // this wave's sets: wave + 4 i, i < mine
    auto kof = [&](int i) { return ((int)wave + 4 * i) * 32; };
    if (mine) load_set(x0, kof(0));
    int it = 0;
    for (; it + 2 <= mine; it += 2) {
        load_set(x1, kof(it + 1));
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x0);
        __builtin_amdgcn_sched_barrier(0);
        load_set(x0, kof(it + 2 < mine ? it + 2 : it + 1));      // (behind the last pair: a set nobody reads, inside [0, K))
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (it < mine) mma_set(x0);
    const f32x4 own = acc[0] + acc[1];
    if (wave > 0) part[wave - 1][lane] = own;
    __syncthreads();
    if (wave > 0) return;
    const f32x4 tot = ((own + part[0][lane]) + part[1][lane]) + part[2][lane];
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg
    const unsigned nn = n0 + li;
    const float sc = s2 ? s2[nn] : 1.f, sh = s2 ? t2[nn] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned m = m0 + 4 * g + r;
        const float sum = tot[r];
        float v = s2 ? sum * sc + sh : sum;
        if (act) v = fmaxf(v, 0.f);
        if (m < M) out[(size_t)m * ldo + nn] = v;
    }
}

// torch's [32][128][3][3] -> wt [tap = 3 kh + kw][32][128]: a (tap, channel)'s 128 input channels contiguous, as the lanes load them
__global__ __launch_bounds__(256) void k_dense_pack_w(const float* __restrict__ w, float* __restrict__ wt) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;      // 9 * 32 * 128 = 144 workgroups exactly
    const unsigned c = i & 127, n = (i >> 7) & 31, tap = i >> 12;
    wt[i] = w[((size_t)n * 128 + c) * 9 + tap];
}

// The pixel a lane reads for tap (kh, kw) of output pixel p = (b, h, w): its offset in floats into in [B][H][W][128], or the
// pixel's own (a valid address whose values the caller discards) with ok = false on the padding.
struct TapPix { size_t off; bool ok; };
__device__ __forceinline__ TapPix tap_pixel(unsigned b, int h, int w, int kh, int kw, int H, int W) {
    const int hi = h + kh - 1, wi = w + kw - 1;
    const bool ok = hi >= 0 && hi < H && wi >= 0 && wi < W;
    return TapPix{(((size_t)b * H + (ok ? hi : h)) * W + (ok ? wi : w)) * 128, ok};
}

// in [B][H][W][128], wt [9][32][128], out rows ldo apart, channels [c0, c0 + 32).  One wave per 64 pixels (two row tiles of 32);
// 36 operand sets of 32 input channels in (tap, channel) order, two sets in turn.
__global__ __launch_bounds__(256) void k_dense_conv3_tile(const float* __restrict__ in, const float* __restrict__ wt, float* __restrict__ out,
                                                          unsigned M, int H, int W, int c0, int ldo, unsigned mtiles) {
    const unsigned lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const unsigned wid = xcd_block() * 4 + (threadIdx.x >> 6);
    if (wid >= mtiles) return;      // (no barrier in this kernel)
    const unsigned m0 = wid * 64;
    unsigned pb_[2]; int ph[2], pw[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const unsigned p = min(m0 + 32 * t + li, M - 1);      // a pixel past M computes the last valid one; never written
        pw[t] = (int)(p % (unsigned)W);
        const unsigned q = p / (unsigned)W;
        ph[t] = (int)(q % (unsigned)H); pb_[t] = q / (unsigned)H;
    }
    const float* pwt = wt + (size_t)li * 128 + 4 * lh;
    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    struct Set { f32x4 a[2][4], b[4]; };
    Set x0, x1;
    auto load_set = [&](Set& x, int i) {      // set i: tap i >> 2, input channels 32 (i & 3) ..
        const int tap = i >> 2, kh = tap / 3, kw = tap - 3 * kh, c = (i & 3) * 32;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const TapPix tp = tap_pixel(pb_[t], ph[t], pw[t], kh, kw, H, W);
            const float* pa = in + tp.off + c + 4 * lh;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(pa + 8 * j);
                x.a[t][j] = tp.ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) x.b[j] = *reinterpret_cast<const f32x4*>(pwt + (size_t)tap * 4096 + c + 8 * j);
    };
    auto mma_set = [&](const Set& x) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < 2; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.a[t][j][e], x.b[j][e], acc[t], 0, 0, 0);
    };
    load_set(x0, 0);
    for (int it = 0; it < 36; it += 2) {
        load_set(x1, it + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x0);
        __builtin_amdgcn_sched_barrier(0);
        load_set(x0, it + 2 < 36 ? it + 2 : it + 1);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(x1);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned m = m0 + 32 * t + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (m < M) out[(size_t)m * ldo + c0 + li] = acc[t][r];
        }
}

// The form for few pixels: workgroup = 16 pixels, nine waves, wave = tap.  A wave sums its tap's 128 input channels for both halves
// of the 32 output channels (two 16 x 16 tiles: the pixel operand is loaded once) in two operand sets of 64 channels, both in flight
// at once, two accumulators per tile in turn; the partial tiles of taps 1 .. 8 go through LDS and wave 0 stores
// (((p0 + p1) + p2) + ... ) + p8, in tap order.
__global__ __launch_bounds__(576) void k_dense_conv3_split(const float* __restrict__ in, const float* __restrict__ wt, float* __restrict__ out,
                                                           unsigned M, int H, int W, int c0, int ldo) {
    __shared__ f32x4 part[8][2][64];
    const unsigned lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4, tap = threadIdx.x >> 6;
    const int kh = (int)tap / 3, kw = (int)tap - 3 * kh;
    const unsigned m0 = xcd_block() * 16;
    const unsigned p = min(m0 + li, M - 1);      // a pixel past M computes the last valid one; never written
    const int pw = (int)(p % (unsigned)W);
    const unsigned q = p / (unsigned)W;
    const int ph = (int)(q % (unsigned)H);
    const TapPix tp = tap_pixel(q / (unsigned)H, ph, pw, kh, kw, H, W);
    const float* pa = in + tp.off + 4 * g;
    const float* pwt = wt + ((size_t)tap * 32 + li) * 128 + 4 * g;
    f32x4 a[8], b[2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(pa + 16 * j);
        a[j] = tp.ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) b[hf][j] = *reinterpret_cast<const f32x4*>(pwt + (size_t)hf * 16 * 128 + 16 * j);
    }
    f32x4 acc[2][2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) acc[hf][0] = acc[hf][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) acc[hf][j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[hf][j][e], acc[hf][j & 1], 0, 0, 0);
    f32x4 sum[2] = {acc[0][0] + acc[0][1], acc[1][0] + acc[1][1]};
    if (tap > 0) { part[tap - 1][0][lane] = sum[0]; part[tap - 1][1][lane] = sum[1]; }
    __syncthreads();      // (every wave of the workgroup arrives: none has left)
    if (tap > 0) return;
#pragma unroll
    for (int t = 0; t < 8; ++t) { sum[0] = sum[0] + part[t][0][lane]; sum[1] = sum[1] + part[t][1][lane]; }
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned m = m0 + 4 * g + r;
            if (m < M) out[(size_t)m * ldo + c0 + 16 * hf + li] = sum[hf][r];
        }
}

// x / skip [B][H][W][C]; POOL: pooled [B][H / 2][W / 2][C], one thread per (pooled pixel, channel quad), else per (pixel, quad)
template <bool POOL>
__global__ __launch_bounds__(256) void k_dense_norm_pool(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ t,
                                                         float* __restrict__ skip, float* __restrict__ pooled, unsigned total, int H, int W,
                                                         int CQ, int act) {
    const int C = 4 * CQ;
    const XcdSpan wk = xcd_walk(total);
    for (unsigned i = wk.first; i < wk.end; i += wk.step) {
        const unsigned cq = i % (unsigned)CQ, px = i / (unsigned)CQ;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(s + 4 * cq), sh = *reinterpret_cast<const f32x4*>(t + 4 * cq);
        auto one = [&](size_t pixel) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(x + pixel * C + 4 * cq);
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) { r[e] = sc[e] * v[e] + sh[e]; if (act) r[e] = fmaxf(r[e], 0.f); }
            *reinterpret_cast<f32x4*>(skip + pixel * C + 4 * cq) = r;
            return r;
        };
        if constexpr (POOL) {
            const unsigned Wo = (unsigned)W >> 1, Ho = (unsigned)H >> 1;
            const unsigned wo = px % Wo, q = px / Wo, ho = q % Ho, b = q / Ho;
            const size_t p00 = ((size_t)b * H + 2 * ho) * W + 2 * wo;
            const f32x4 a = one(p00), bb = one(p00 + 1), c = one(p00 + W), d = one(p00 + W + 1);
            f32x4 r;
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = 0.25f * ((a[e] + bb[e]) + (c[e] + d[e]));
            *reinterpret_cast<f32x4*>(pooled + (size_t)px * C + 4 * cq) = r;
        } else {
            one(px);
        }
    }
}

// in [M][C] -> out[m][0 .. C) of rows ld apart
__global__ __launch_bounds__(256) void k_dense_place(const float* __restrict__ in, float* __restrict__ out, unsigned total, int CQ, int ld) {
    const XcdSpan wk = xcd_walk(total);
    for (unsigned i = wk.first; i < wk.end; i += wk.step) {
        const unsigned cq = i % (unsigned)CQ, m = i / (unsigned)CQ;
        *reinterpret_cast<f32x4*>(out + (size_t)m * ld + 4 * cq) = *reinterpret_cast<const f32x4*>(in + (size_t)i * 4);
    }
}

// ---- the host side: the forms (functions of the shape alone), the checks and the launches

bool dense_pw_ok(long long M, int K, int Cout, int ldi, int ldo) {
    return M >= 1 && M < (1LL << 31) - 64 && K >= 32 && K <= 2048 && K % 32 == 0 && Cout >= 32 && Cout <= 1024 && Cout % 32 == 0 &&
           ldi >= K && ldi % 4 == 0 && ldo >= Cout;
}

// 1 = 32 x 32 tiles where they give every SIMD of the chip a wave (1024), else 0 = 16 x 16 tiles
int dense_pw_form(long long M, int Cout) { return ((M + 31) / 32) * (Cout / 32) >= 1024 ? 1 : 0; }

int launch_dense_pw(const float* in, const float* s1, const float* t1, const float* w, const float* s2, const float* t2, float* out,
                    long long M, int K, int Cout, int ldi, int ldo, int act, int form, hipStream_t s) {
    if (!dense_pw_ok(M, K, Cout, ldi, ldo) || act < 0 || act > 1 || form < -1 || form > 1 || !s1 != !t1 || !s2 != !t2) return FPC_EINVAL;
    if (form < 0) form = dense_pw_form(M, Cout);
    const int tile = form ? 32 : 16;
    const long long mtiles = (M + tile - 1) / tile, ntiles = Cout / tile, waves = mtiles * ntiles;
    if (waves >= (1LL << 31)) return FPC_EINVAL;
    const long long grid = xcd_grid(form ? (waves + 3) / 4 : waves);      // (form 0: a workgroup per tile); the workgroups past the last tile leave at once
    const dim3 g((unsigned)grid), b(256);
#define FPC_DENSE_PW(KERNEL) hipLaunchKernelGGL(KERNEL, g, b, 0, s, in, s1, t1, w, s2, t2, out, (unsigned)M, K, ldi, ldo, act, (unsigned)mtiles, (unsigned)ntiles)
    if (form) { if (s1) FPC_DENSE_PW(k_dense_pw32<true>); else FPC_DENSE_PW(k_dense_pw32<false>); }
    else { if (s1) FPC_DENSE_PW(k_dense_pw16<true>); else FPC_DENSE_PW(k_dense_pw16<false>); }
#undef FPC_DENSE_PW
    return check_launch();
}

int launch_dense_pack_w(const float* w, float* wt, hipStream_t s) {
    hipLaunchKernelGGL(k_dense_pack_w, dim3(kDenseWtFloats / 256), dim3(256), 0, s, w, wt);
    return check_launch();
}

bool dense_conv3_ok(int B, int H, int W, int c0, int ldo) {
    return B >= 1 && H >= 1 && W >= 1 && (long long)B * H * W < (1LL << 31) - 64 && c0 >= 0 && c0 % 32 == 0 && ldo >= 32 && c0 <= ldo - 32;
}

// 1 = k_dense_conv3_tile where its waves of 64 pixels give every SIMD of the chip one (1024), else 0 = k_dense_conv3_split
int dense_conv3_form(long long M) { return (M + 63) / 64 >= 1024 ? 1 : 0; }

int launch_dense_conv3(const float* in, const float* wt, float* out, int B, int H, int W, int c0, int ldo, int form, hipStream_t s) {
    if (!dense_conv3_ok(B, H, W, c0, ldo) || form < -1 || form > 1) return FPC_EINVAL;
    const long long M = (long long)B * H * W;
    if (form < 0) form = dense_conv3_form(M);
    if (form) {
        const long long mtiles = (M + 63) / 64;
        const long long grid = xcd_grid((mtiles + 3) / 4);
        hipLaunchKernelGGL(k_dense_conv3_tile, dim3((unsigned)grid), dim3(256), 0, s, in, wt, out, (unsigned)M, H, W, c0, ldo, (unsigned)mtiles);
    } else {
        // (exactly one workgroup per 16 pixels: the kernel has a barrier, so no workgroup may be past the last tile; a grid that is
        // no multiple of 8 walks in launch order)
        hipLaunchKernelGGL(k_dense_conv3_split, dim3((unsigned)((M + 15) / 16)), dim3(576), 0, s, in, wt, out, (unsigned)M, H, W, c0, ldo);
    }
    return check_launch();
}

int launch_dense_norm_pool(const float* x, const float* sc, const float* sh, float* skip, float* pooled, int B, int H, int W, int C, int act,
                           hipStream_t s) {
    if (B < 1 || H < 1 || W < 1 || C < 4 || C % 4 || act < 0 || act > 1 || (pooled && ((H | W) & 1))) return FPC_EINVAL;
    const long long total = (long long)B * H * W * (C / 4) / (pooled ? 4 : 1);
    if ((long long)B * H * W * (C / 4) >= kWalkLimit) return FPC_EINVAL;
    if (pooled) hipLaunchKernelGGL(k_dense_norm_pool<true>, dim3(stream_grid(total)), dim3(256), 0, s, x, sc, sh, skip, pooled, (unsigned)total, H, W, C / 4, act);
    else hipLaunchKernelGGL(k_dense_norm_pool<false>, dim3(stream_grid(total)), dim3(256), 0, s, x, sc, sh, skip, pooled, (unsigned)total, H, W, C / 4, act);
    return check_launch();
}

int launch_dense_place(const float* in, float* out, long long M, int C, int ld, hipStream_t s) {
    if (M < 1 || C < 4 || C % 4 || ld < C || ld % 4) return FPC_EINVAL;
    const long long total = M * (C / 4);
    if (total >= kWalkLimit) return FPC_EINVAL;
    hipLaunchKernelGGL(k_dense_place, dim3(stream_grid(total)), dim3(256), 0, s, in, out, (unsigned)total, C / 4, ld);
    return check_launch();
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_dense_pw(const float* in, const float* s1, const float* t1, const float* w, const float* s2, const float* t2, float* out,
                            int64_t M, int K, int Cout, int ldi, int ldo, int act, int form, fpc_stream_t stream) {
    if (!in || !w || !out || !al16(in) || !al16(s1) || !al16(t1) || !al16(w) || !al16(s2) || !al16(t2) || !al16(out)) return FPC_EINVAL;
    return launch_dense_pw(in, s1, t1, w, s2, t2, out, (long long)M, K, Cout, ldi, ldo, act, form, (hipStream_t)stream);
}

extern "C" int fpc_dense_pw_form(int64_t M, int K, int Cout) {
    if (!dense_pw_ok((long long)M, K, Cout, K, Cout)) return FPC_EINVAL;
    return dense_pw_form((long long)M, Cout);
}

extern "C" int fpc_dense_conv3x3_pack(const float* w, float* wt, fpc_stream_t stream) {
    if (!w || !wt || !al16(w) || !al16(wt)) return FPC_EINVAL;
    return launch_dense_pack_w(w, wt, (hipStream_t)stream);
}

extern "C" int fpc_dense_conv3x3(const float* in, const float* wt, float* out, int B, int H, int W, int c0, int ldo, int form,
                                 fpc_stream_t stream) {
    if (!in || !wt || !out || !al16(in) || !al16(wt) || !al16(out)) return FPC_EINVAL;
    return launch_dense_conv3(in, wt, out, B, H, W, c0, ldo, form, (hipStream_t)stream);
}

extern "C" int fpc_dense_conv3x3_form(int B, int H, int W) {
    if (!dense_conv3_ok(B, H, W, 0, 32)) return FPC_EINVAL;
    return dense_conv3_form((long long)B * H * W);
}

extern "C" int fpc_dense_norm_pool(const float* x, const float* s, const float* t, float* skip, float* pooled, int B, int H, int W, int C,
                                   int act, fpc_stream_t stream) {
    if (!x || !s || !t || !skip || !al16(x) || !al16(s) || !al16(t) || !al16(skip) || !al16(pooled)) return FPC_EINVAL;
    return launch_dense_norm_pool(x, s, t, skip, pooled, B, H, W, C, act, (hipStream_t)stream);
}

extern "C" int fpc_dense_place(const float* in, float* out, int64_t M, int C, int ld, fpc_stream_t stream) {
    if (!in || !out || !al16(in) || !al16(out)) return FPC_EINVAL;
    return launch_dense_place(in, out, (long long)M, C, ld, (hipStream_t)stream);
}
