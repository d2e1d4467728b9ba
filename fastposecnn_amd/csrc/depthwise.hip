// depthwise.hip — the depthwise K x K convolution of the MobileNetV2 and EfficientNet-B0 encoders, forward and both gradients, one
// family of kernels for both.  Dense channel-last f32, C a multiple of 4, K 3 or 5, stride S 1 or 2, lanes along the channel quads
// with 16-byte loads and stores, the weights torch's [C][1][K][K] read and written in place.  Plain f32 FMAs in an order the shape
// alone fixes, no atomics, no scratch: results are bit-identical run to run (DESIGN.md 4.2a''''''' and 4.2a''''''''').  The streaming
// kernels walk their items in the XCD-banded order of conv_device.hpp (xcd_walk), so neighbouring rows are fetched by one L2.
//
// The two encoders differ in the pad before the window, PB, a template parameter of every kernel, and in the output extent:
//   pad 1 (MobileNetV2, fpc_dwconv3x3*): K = 3, PB = 1 at either stride, Ho = (Hi - 1) / S + 1, any extent;
//   "same" (EfficientNet, fpc_mbconv_dw*): efficientnet_pytorch's static pads for the declared 224 image, same_pad_before(K, S) =
//          (K - 1) / 2 at stride 1, (K - 3) / 2 at stride 2 (even extents only), Ho = Hi / S.  (K, S) = (3, 1) is pad 1 on every
//          side: those entries take the pad-1 instances.
//
// Forward: k_dw_fwd<K, S, PB, SWISH>, out = act(scale . conv + shift) with BatchNorm folded into scale / shift (training: act 0,
// scale 1, shift 0).  One thread per (row, strip of 4 (S = 1) or 2 (S = 2) output columns, channel quad): a 3x3 strip reads 3 x 6
// (3 x 5) input quads for 4 (2) outputs instead of 9 each, a 5x5 strip at stride 1 5 x 8 for 4.  K K FMAs per output in (kh, kw) order.
// act 0 none, 1 ReLU6; SWISH (the EfficientNet instances alone) adds 2 = swish v / (1 + exp(-v)) on div_ieee, the others keep their
// two-way select and divide nothing.
//
// Data gradient, stride 1: k_dw_dgrad_s1<K, PB>, the forward's strip loop over dy with the taps flipped,
// dx[h][w] = sum dy[h + PB - kh][w + PB - kw] w[kh][kw]: K K FMAs per output in ascending (row, column) order of dy.
//
// Both take the ROWS switch: K = 3 holds the quad's 36 weights in registers with the three rows unrolled; K = 5 keeps the rows a
// loop, each with its own 4 x 5 weights (100 hoisted weights plus the window do not fit the registers of a 256-thread workgroup).
//
// Data gradient, stride 2: k_dw_dgrad_s2<K, PB>, no zero insertion.  Per axis dx[i] = sum over the taps k with i + PB - k even of
// dy[(i + PB - k) / 2] w[k]:
//   K = 3, PB 1:  dx[2a] = dy[a] w[1],                    dx[2a + 1] = dy[a] w[2] + dy[a + 1] w[0]            9 products per block
//   K = 3, PB 0:  dx[2a] = dy[a] w[0] + dy[a - 1] w[2],   dx[2a + 1] = dy[a] w[1]                              9 products
//   K = 5, PB 1:  dx[2a] = dy[a] w[1] + dy[a - 1] w[3],   dx[2a + 1] = dy[a + 1] w[0] + dy[a] w[2] + dy[a - 1] w[4]      25 products
// One thread per (block row a, strip of 2 blocks of 2 x 2 of dx, channel quad); it writes the block's two rows of dx one after the
// other, each from the tap rows of its parity in ascending kh, a tap row from one row of dy in ascending kw.  Under pad 1 an odd
// Hi / Wi leaves the last block row / column half outside dx: those rows and columns are not written.
//
// Weight gradient: k_dw_wgrad<K, S, PB>, then k_dw_wgrad_reduce.  The (frame, output row) list is cut into
// dw_wgrad_slices(B, Ho, Wo, C, slots) contiguous slices; a workgroup takes one slice for a chunk of 8 channel quads (128 bytes of a
// pixel).  K = 3: 256 threads, a thread holds a quad's 36 accumulators, 32 pixel slots.  K = 5: a quad's 100 accumulators do not
// fit beside five sliding rows, so the taps are split over threads — a thread per (channel quad, tap row kh) holds 4 x 5
// accumulators and one row's 5 sliding column quads —, 320 threads, 8 pixel slots of 8 quads x 5 tap rows.  A slot takes the
// slice's (row, segment of 8 output columns) units u = slot, slot + slots, ... and walks a segment with the x columns sliding in
// registers: per output pixel one quad of dy and S new quads of x per tap row.  The slots are added pairwise through LDS (slot
// s + h into slot s, h = slots / 2 .. 1) and the workgroup writes ONE partial [slice][C][K K]; the second launch adds the slices in
// double — sixteen contiguous ranges of slices, each in ascending order, then the ranges in ascending order — and writes OIHW.  x
// and dy leave memory once, plus the rows a slice shares with its neighbours (the workgroups of neighbouring slices run on one
// XCD: one L2).
#include <algorithm>

#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr int same_pad_before(int K, int S) { return S == 1 ? (K - 1) / 2 : (K - 3) / 2; }

template <bool SWISH>
__device__ __forceinline__ float dw_act(float v, int act) {
    if constexpr (SWISH) return act == 2 ? swish(v) : act == 1 ? fminf(fmaxf(v, 0.f), 6.f) : v;
    else return act ? fminf(fmaxf(v, 0.f), 6.f) : v;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------

// in [B][Hi][Wi][C], w [C][1][K][K], out [B][Ho][Wo][C]; total = B Ho WT CQ items with WT strips of TW output columns per row
template <int K, int S, int PB, bool SWISH>
__global__ __launch_bounds__(256) void k_dw_fwd(const float* __restrict__ in, const float* __restrict__ w,
                                                const float* __restrict__ scale, const float* __restrict__ shift,
                                                float* __restrict__ out, unsigned total, int Hi, int Wi, int Ho, int Wo, int WT, int CQ,
                                                int act) {
    constexpr int TW = S == 1 ? 4 : 2, NC = (TW - 1) * S + K;
    const int C = 4 * CQ;
    const XcdSpan wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned ho = t % (unsigned)Ho, b = t / (unsigned)Ho;
        // K = 3: the quad's 36 weights [channel][kh][kw] in registers (nine 16-byte loads) and the three rows unrolled.  K = 5: the
        // rows stay a loop and each takes its own 4 x 5 weights [channel][kw] (one float at a time: a row of 5 is not 16-byte aligned)
        constexpr bool ROWS = K == 5;
        constexpr int KH_UNROLL = ROWS ? 1 : K;
        float wf[ROWS ? 4 * K : 4 * K * K];
        const float* wq = w + 4 * K * K * (size_t)cq;
        if constexpr (!ROWS) {
#pragma unroll
            for (int i = 0; i < K * K; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(wq + 4 * i);
                wf[4 * i] = v[0]; wf[4 * i + 1] = v[1]; wf[4 * i + 2] = v[2]; wf[4 * i + 3] = v[3];
            }
        }
        f32x4 acc[TW];
#pragma unroll
        for (int o = 0; o < TW; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int wo0 = (int)wt * TW, wi0 = wo0 * S - PB;
#pragma unroll KH_UNROLL
        for (int kh = 0; kh < K; ++kh) {
            if constexpr (ROWS) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) wf[K * j + kw] = wq[K * K * j + K * kh + kw];
            }
            const int hi = (int)ho * S - PB + kh;
            const bool rowok = hi >= 0 && hi < Hi;
            f32x4 x[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int wi = wi0 + c;
                x[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (rowok && wi >= 0 && wi < Wi) x[c] = *reinterpret_cast<const f32x4*>(in + (((size_t)b * Hi + hi) * Wi + wi) * C + 4 * cq);
            }
#pragma unroll
            for (int o = 0; o < TW; ++o)
#pragma unroll
                for (int kw = 0; kw < K; ++kw)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(x[o * S + kw][j], wf[ROWS ? K * j + kw : K * K * j + K * kh + kw], acc[o][j]);
        }
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * cq), sh = *reinterpret_cast<const f32x4*>(shift + 4 * cq);
#pragma unroll
        for (int o = 0; o < TW; ++o) {
            if (wo0 + o >= Wo) continue;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = dw_act<SWISH>(acc[o][j] * sc[j] + sh[j], act);
            *reinterpret_cast<f32x4*>(out + (((size_t)b * Ho + ho) * Wo + wo0 + o) * C + 4 * cq) = v;
        }
    }
}

// ---- data gradient --------------------------------------------------------------------------------------------------------------

// dy, dx [B][H][W][C] (stride 1: one shape), w [C][1][K][K]; total = B H WT CQ items with WT strips of 4 columns per row
template <int K, int PB>
__global__ __launch_bounds__(256) void k_dw_dgrad_s1(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                     unsigned total, int H, int W, int WT, int CQ) {
    constexpr int TW = 4, NC = TW + K - 1;
    const int C = 4 * CQ;
    const XcdSpan wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned h = t % (unsigned)H, b = t / (unsigned)H;
        constexpr bool ROWS = K == 5;      // as k_dw_fwd's
        constexpr int R_UNROLL = ROWS ? 1 : K;
        float wf[ROWS ? 4 * K : 4 * K * K];
        const float* wq = w + 4 * K * K * (size_t)cq;
        if constexpr (!ROWS) {
#pragma unroll
            for (int i = 0; i < K * K; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(wq + 4 * i);
                wf[4 * i] = v[0]; wf[4 * i + 1] = v[1]; wf[4 * i + 2] = v[2]; wf[4 * i + 3] = v[3];
            }
        }
        f32x4 acc[TW];
#pragma unroll
        for (int o = 0; o < TW; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int w0 = (int)wt * TW;
#pragma unroll R_UNROLL
        for (int r = 0; r < K; ++r) {      // the row of dy at h - PB + r meets the tap row kh = K - 1 - r
            const int kh = K - 1 - r;
            if constexpr (ROWS) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int kw = 0; kw < K; ++kw) wf[K * j + kw] = wq[K * K * j + K * kh + kw];
            }
            const int hy = (int)h - PB + r;
            const bool rowok = hy >= 0 && hy < H;
            f32x4 d[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int wy = w0 - PB + c;
                d[c] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (rowok && wy >= 0 && wy < W) d[c] = *reinterpret_cast<const f32x4*>(dy + (((size_t)b * H + hy) * W + wy) * C + 4 * cq);
            }
#pragma unroll
            for (int o = 0; o < TW; ++o)
#pragma unroll
                for (int s = 0; s < K; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[o][j] = fmaf(d[o + s][j], wf[ROWS ? K * j + (K - 1 - s) : K * K * j + K * kh + (K - 1 - s)], acc[o][j]);
        }
#pragma unroll
        for (int o = 0; o < TW; ++o)
            if (w0 + o < W) *reinterpret_cast<f32x4*>(dx + (((size_t)b * H + h) * W + w0 + o) * C + 4 * cq) = acc[o];
    }
}

// Stride 2.  One row of dx, y = 2 a + PY, of the blocks b0, b0 + 1: the tap rows kh = K0, K0 + 2, ... of parity PY in ascending kh, tap
// row kh from the row a + (PY + PB - kh) / 2 of dy in ascending kw; dy outside its map counts as zero, columns of dx past Wi (an odd
// extent under pad 1) are not written
template <int K, int PB, int PY>
__device__ __forceinline__ void dw_dgrad_s2_row(const float* __restrict__ dyb, const float* __restrict__ wq, float* __restrict__ dxrow,
                                                int a, int b0, int Ho, int Wo, int Wi, int C) {
    constexpr int TB = 2;
    constexpr int K0 = (PY + PB) & 1, NT = (K - K0 + 1) / 2;      // tap rows of this parity
    // offsets into dy a tap can have, from tap K - 1 to tap 0: (K, PB) = (3, 1) 0..1, (3, 0) -1..0, (5, 1) -1..1
    constexpr int OMIN = (((K - 1 + PB) & 1) + PB - (K - 1)) / 2, OMAX = (PB + 1) / 2, NC = TB + OMAX - OMIN;
    f32x4 acc[TB][2];
#pragma unroll
    for (int i = 0; i < TB; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int t = 0; t < NT; ++t) {
        const int kh = K0 + 2 * t;
        const int ya = a + (PY + PB - K0) / 2 - t;      // (PY + PB - K0 is even)
        float wf[4 * K];      // [channel of the quad][kw]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) wf[K * j + kw] = wq[K * K * j + K * kh + kw];
        const bool rowok = ya >= 0 && ya < Ho;
        f32x4 d[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int xb = b0 + OMIN + c;
            d[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (rowok && xb >= 0 && xb < Wo) d[c] = *reinterpret_cast<const f32x4*>(dyb + ((size_t)ya * Wo + xb) * C);
        }
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
            const int px = (kw + PB) & 1, off = (px + PB - kw) / 2;      // (compile-time after unrolling; px + PB - kw is even)
#pragma unroll
            for (int i = 0; i < TB; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][px][j] = fmaf(d[i + off - OMIN][j], wf[K * j + kw], acc[i][px][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < TB; ++i)
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            const int x = 2 * (b0 + i) + px;
            if (x < Wi) *reinterpret_cast<f32x4*>(dxrow + (size_t)x * C) = acc[i][px];
        }
}

// dy [B][Ho][Wo][C], dx [B][Hi][Wi][C], Ho block rows of two rows of dx (the last one of an odd Hi has one); total = B Ho WT CQ
// items with WT strips of 2 blocks
template <int K, int PB>
__global__ __launch_bounds__(256) void k_dw_dgrad_s2(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                     unsigned total, int Hi, int Wi, int Ho, int Wo, int WT, int CQ) {
    const int C = 4 * CQ;
    const XcdSpan wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned a = t % (unsigned)Ho, b = t / (unsigned)Ho;
        const float* wq = w + 4 * K * K * (size_t)cq;
        const float* dyb = dy + (size_t)b * Ho * Wo * C + 4 * cq;
        float* dxb = dx + ((size_t)b * Hi + 2 * a) * (size_t)Wi * C + 4 * cq;
        dw_dgrad_s2_row<K, PB, 0>(dyb, wq, dxb, (int)a, 2 * (int)wt, Ho, Wo, Wi, C);
        if (2 * (int)a + 1 < Hi) dw_dgrad_s2_row<K, PB, 1>(dyb, wq, dxb + (size_t)Wi * C, (int)a, 2 * (int)wt, Ho, Wo, Wi, C);
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------

constexpr int kDwQuads = 8;                    // channel quads per workgroup: 128 bytes of a pixel
constexpr int kDwSeg = 8;                      // output columns of a unit
constexpr int kDwRanges = 16;                  // k_dw_wgrad_reduce: contiguous ranges of slices per sum
constexpr int dw_wgrad_threads(int K) { return K == 5 ? 320 : 256; }
constexpr int dw_wgrad_slots(int K) { return K == 5 ? 8 : 32; }      // pixel slots per workgroup

struct DwWgradArgs {
    const float* x;       // [B][Hi][Wi][C]
    const float* dy;      // [B][Ho][Wo][C]
    float* part;          // [nslice][C][K K]
    int B, Hi, Wi, Ho, Wo, C, CQ;
    int nchunk, nslice, nseg;
    unsigned blocks;      // nchunk * nslice
};

template <int K, int S, int PB>
__global__ __launch_bounds__(dw_wgrad_threads(K)) void k_dw_wgrad(const DwWgradArgs a) {
    constexpr int KHT = K == 5 ? 1 : K;                 // tap rows a thread holds
    constexpr int TPS = kDwQuads * (K / KHT);           // threads of a pixel slot
    constexpr int SLOTS = dw_wgrad_slots(K), HALF = SLOTS / 2 * TPS, NACC = 4 * KHT * K;
    static_assert(SLOTS * TPS == dw_wgrad_threads(K), "threads = slots x quads x tap rows");
    __shared__ float red[NACC * HALF];
    // XCD-banded order (conv_device.hpp) over the (slice, chunk) list, the chunk fastest; the ids past it leave before any barrier
    const unsigned bid = xcd_block();
    if (bid >= a.blocks) return;
    const int chunk = (int)(bid % (unsigned)a.nchunk), slice = (int)(bid / (unsigned)a.nchunk);
    const int tid = threadIdx.x, q = tid % kDwQuads, kh0 = (tid / kDwQuads) % (K / KHT) * KHT, slot = tid / TPS;
    const int qg = chunk * kDwQuads + q;
    const bool on = qg < a.CQ;
    const long long rows = (long long)a.B * a.Ho;
    const unsigned r0 = (unsigned)(slice * rows / a.nslice), r1 = (unsigned)((slice + 1) * rows / a.nslice);
    const unsigned units = (r1 - r0) * (unsigned)a.nseg;

    float acc[NACC];      // [channel of the quad][tap row of the thread][kw]
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.f;

    if (on) {
        const size_t C = (size_t)a.C;
#pragma unroll 1
        for (unsigned u = slot; u < units; u += SLOTS) {
            const unsigned row = r0 + u / (unsigned)a.nseg;
            const int seg = (int)(u % (unsigned)a.nseg), b = (int)(row / (unsigned)a.Ho), ho = (int)(row % (unsigned)a.Ho);
            const int w0 = seg * kDwSeg, w1 = min(a.Wo, w0 + kDwSeg);
            const float* xr[KHT];
            bool rowok[KHT];
#pragma unroll
            for (int r = 0; r < KHT; ++r) {
                const int hi = ho * S - PB + kh0 + r;
                rowok[r] = hi >= 0 && hi < a.Hi;
                xr[r] = a.x + (((size_t)b * a.Hi + (rowok[r] ? hi : 0)) * a.Wi) * C + 4 * (size_t)qg;
            }
            const float* dyr = a.dy + (((size_t)b * a.Ho + ho) * a.Wo) * C + 4 * (size_t)qg;
            auto col = [&](int r, int wi) {
                f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                if (rowok[r] && wi >= 0 && wi < a.Wi) v = *reinterpret_cast<const f32x4*>(xr[r] + (size_t)wi * C);
                return v;
            };
            f32x4 xw[KHT][K];      // the columns under taps kw = 0 .. K - 1: S new ones per output pixel, the rest slide
#pragma unroll
            for (int r = 0; r < KHT; ++r)
#pragma unroll
                for (int kw = 0; kw < K - S; ++kw) xw[r][kw] = col(r, w0 * S - PB + kw);
#pragma unroll 1
            for (int wo = w0; wo < w1; ++wo) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + (size_t)wo * C);
#pragma unroll
                for (int r = 0; r < KHT; ++r)
#pragma unroll
                    for (int kw = K - S; kw < K; ++kw) xw[r][kw] = col(r, wo * S - PB + kw);
#pragma unroll
                for (int r = 0; r < KHT; ++r)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int kw = 0; kw < K; ++kw) acc[(j * KHT + r) * K + kw] = fmaf(d[j], xw[r][kw][j], acc[(j * KHT + r) * K + kw]);
#pragma unroll
                for (int r = 0; r < KHT; ++r)
#pragma unroll
                    for (int kw = 0; kw < K - S; ++kw) xw[r][kw] = xw[r][kw + S];
            }
        }
    }

    // the pixel slots, pairwise in a fixed tree: slot s + h into slot s, h = SLOTS / 2 .. 1
#pragma unroll 1
    for (int h = SLOTS / 2; h >= 1; h >>= 1) {
        if (slot >= h && slot < 2 * h) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) red[k * HALF + tid - h * TPS] = acc[k];
        }
        __syncthreads();
        if (slot < h) {
#pragma unroll
            for (int k = 0; k < NACC; ++k) acc[k] = acc[k] + red[k * HALF + tid];
        }
        __syncthreads();
    }
    if (slot != 0 || !on) return;
    float* dst = a.part + ((size_t)slice * a.C + 4 * (size_t)qg) * (K * K);      // 4 K K floats: (channel, tap)
    if constexpr (KHT == K) {
#pragma unroll
        for (int k = 0; k < K * K; ++k) *reinterpret_cast<f32x4*>(dst + 4 * k) = f32x4{acc[4 * k], acc[4 * k + 1], acc[4 * k + 2], acc[4 * k + 3]};
    } else {      // the thread's tap row of each of the four channels
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int kw = 0; kw < K; ++kw) dst[j * K * K + kh0 * K + kw] = acc[j * K + kw];
    }
}

// dw[i] = sum over the slices of part[slice][i], in double: thread (range r, quad i4) adds the slices of range r in ascending
// order, then the ranges are added in ascending order.  n4 float4 per slice; a workgroup takes 16 of them
__global__ __launch_bounds__(256) void k_dw_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int n4, int nslice) {
    __shared__ double sh[kDwRanges][16][4];
    const int t = threadIdx.x, c = t & 15, r = t >> 4;
    const int i4 = blockIdx.x * 16 + c;
    const int s0 = (int)((long long)r * nslice / kDwRanges), s1 = (int)((long long)(r + 1) * nslice / kDwRanges);
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (i4 < n4) {
#pragma unroll 8
        for (int sl = s0; sl < s1; ++sl) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(part + 4 * ((size_t)sl * n4 + i4));
            s[0] += (double)v[0]; s[1] += (double)v[1]; s[2] += (double)v[2]; s[3] += (double)v[3];
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[r][c][e] = s[e];
    __syncthreads();
    if (r != 0 || i4 >= n4) return;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        double v = sh[0][c][e];
        for (int k = 1; k < kDwRanges; ++k) v += sh[k][c][e];
        o[e] = (float)v;
    }
    *reinterpret_cast<f32x4*>(dw + 4 * (size_t)i4) = o;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------

inline bool dw_shape_ok(int B, int Hi, int Wi, int C, int stride) {
    return B >= 1 && Hi >= 1 && Wi >= 1 && C >= 4 && C % 4 == 0 && (stride == 1 || stride == 2) &&
           (long long)B * Hi * Wi * (C / 4) < kWalkLimit;      // every kernel's item count is at most this
}
// ... and under the "same" pads: their tap counts, and even extents at stride 2 (an odd one would need another pad table)
inline bool mb_dw_shape_ok(int B, int Hi, int Wi, int C, int k, int stride) {
    return dw_shape_ok(B, Hi, Wi, C, stride) && (k == 3 || k == 5) && !(stride == 2 && ((Hi | Wi) & 1));
}

// Slices of the weight gradient's (frame, output row) list, a function of (B, Ho, Wo, C) and the kernel's pixel slots alone
// (include/fpc.h states it): enough for four workgroups per compute unit over the channel chunks, at most one per row, and no more
// than leave every slice one unit of 8 output columns per pixel slot (32 slots at k = 3, 8 at k = 5).
int dw_wgrad_slices(int B, int Ho, int Wo, int C, int slots) {
    const long long rows = (long long)B * Ho, nseg = cdiv(Wo, kDwSeg), chunks = cdiv(C / 4, kDwQuads);
    long long n = std::max<long long>(1, 1024 / chunks);
    n = std::min(n, rows * nseg / slots);
    n = std::min(n, rows);
    return (int)std::max<long long>(1, n);
}

// The forward of a checked shape: same = the "same" pads and the three-way activation, else pad 1 (k = 3)
int launch_dw_fwd(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int Ho,
                  int Wo, int C, int k, int stride, bool same, int act, hipStream_t s) {
    const int TW = stride == 1 ? 4 : 2, WT = (Wo + TW - 1) / TW;
    const long long total = (long long)B * Ho * WT * (C / 4);
    if (total >= kWalkLimit) return FPC_EINVAL;
#define FPC_DW_FWD(K, S, PB, SWISH) hipLaunchKernelGGL((k_dw_fwd<K, S, PB, SWISH>), dim3(stream_grid(total)), dim3(256), 0, s, in, w, scale, shift, out, (unsigned)total, Hi, Wi, Ho, Wo, WT, C / 4, act)
    if (!same) { if (stride == 1) FPC_DW_FWD(3, 1, 1, false); else FPC_DW_FWD(3, 2, 1, false); }
    else if (k == 3 && stride == 1) FPC_DW_FWD(3, 1, same_pad_before(3, 1), true);
    else if (k == 3) FPC_DW_FWD(3, 2, same_pad_before(3, 2), true);
    else if (stride == 1) FPC_DW_FWD(5, 1, same_pad_before(5, 1), true);
    else FPC_DW_FWD(5, 2, same_pad_before(5, 2), true);
#undef FPC_DW_FWD
    return check_launch();
}

// The data gradient of a checked shape
int launch_dw_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int k, int stride, bool same,
                    hipStream_t s) {
    const int WT = stride == 1 ? cdiv(Wi, 4) : cdiv(Wo, 2);
    const long long total = (long long)B * Ho * WT * (C / 4);
    const dim3 grid(stream_grid(total)), block(256);
    if (stride == 1) {      // one pad, (K - 1) / 2, under both conventions
        if (k == 3) hipLaunchKernelGGL((k_dw_dgrad_s1<3, 1>), grid, block, 0, s, dy, w, dx, (unsigned)total, Hi, Wi, WT, C / 4);
        else hipLaunchKernelGGL((k_dw_dgrad_s1<5, 2>), grid, block, 0, s, dy, w, dx, (unsigned)total, Hi, Wi, WT, C / 4);
    } else {
        if (!same) hipLaunchKernelGGL((k_dw_dgrad_s2<3, 1>), grid, block, 0, s, dy, w, dx, (unsigned)total, Hi, Wi, Ho, Wo, WT, C / 4);
        else if (k == 3) hipLaunchKernelGGL((k_dw_dgrad_s2<3, same_pad_before(3, 2)>), grid, block, 0, s, dy, w, dx, (unsigned)total, Hi, Wi, Ho, Wo, WT, C / 4);
        else hipLaunchKernelGGL((k_dw_dgrad_s2<5, same_pad_before(5, 2)>), grid, block, 0, s, dy, w, dx, (unsigned)total, Hi, Wi, Ho, Wo, WT, C / 4);
    }
    return check_launch();
}

// The weight gradient of a checked shape and workspace: the partials, then their sum
int launch_dw_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int Ho, int Wo, int C, int k, int stride, bool same,
                    void* ws, hipStream_t s) {
    DwWgradArgs a;
    a.x = x; a.dy = dy; a.part = (float*)ws;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.C = C; a.CQ = C / 4;
    a.nchunk = cdiv(a.CQ, kDwQuads); a.nslice = dw_wgrad_slices(B, Ho, Wo, C, dw_wgrad_slots(k)); a.nseg = cdiv(Wo, kDwSeg);
    const long long blocks = (long long)a.nchunk * a.nslice;      // (at most max(nchunk, 1024))
    a.blocks = (unsigned)blocks;
    const unsigned grid = (unsigned)xcd_grid(blocks);
#define FPC_DW_WGRAD(K, S, PB) hipLaunchKernelGGL((k_dw_wgrad<K, S, PB>), dim3(grid), dim3(dw_wgrad_threads(K)), 0, s, a)
    if (k == 3 && stride == 1) FPC_DW_WGRAD(3, 1, 1);
    else if (k == 3 && !same) FPC_DW_WGRAD(3, 2, 1);
    else if (k == 3) FPC_DW_WGRAD(3, 2, same_pad_before(3, 2));
    else if (stride == 1) FPC_DW_WGRAD(5, 1, same_pad_before(5, 1));
    else FPC_DW_WGRAD(5, 2, same_pad_before(5, 2));
#undef FPC_DW_WGRAD
    int rc = check_launch();
    if (rc) return rc;
    const int n4 = C * k * k / 4;
    hipLaunchKernelGGL(k_dw_wgrad_reduce, dim3(cdiv(n4, 16)), dim3(256), 0, s, (const float*)ws, dw, n4, a.nslice);
    return check_launch();
}

}  // namespace

int launch_dwconv3x3(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                     int stride, int act, hipStream_t s) {
    if (B < 1 || Hi < 1 || Wi < 1 || C < 4 || C % 4 || (stride != 1 && stride != 2) || act < 0 || act > 1) return FPC_EINVAL;
    return launch_dw_fwd(in, w, scale, shift, out, B, Hi, Wi, (Hi - 1) / stride + 1, (Wi - 1) / stride + 1, C, 3, stride, false, act, s);
}

int launch_mb_dwconv(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                     int k, int stride, int act, hipStream_t s) {
    if (B < 1 || Hi < 1 || Wi < 1 || C < 4 || C % 4 || (k != 3 && k != 5) || (stride != 1 && stride != 2) || act < 0 || act > 2) return FPC_EINVAL;
    if (stride == 2 && ((Hi | Wi) & 1)) return FPC_EINVAL;      // (an odd extent would need another pad table)
    return launch_dw_fwd(in, w, scale, shift, out, B, Hi, Wi, Hi / stride, Wi / stride, C, k, stride, true, act, s);
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_dwconv3x3(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                             int C, int stride, int act, fpc_stream_t stream) {
    if (!in || !w || !scale || !shift || !out || !al16(in) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out)) return FPC_EINVAL;
    return launch_dwconv3x3(in, w, scale, shift, out, B, Hi, Wi, C, stride, act, (hipStream_t)stream);
}

extern "C" int fpc_mbconv_dw(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                             int C, int k, int stride, int act, fpc_stream_t stream) {
    if (!in || !w || !scale || !shift || !out || !al16(in) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out)) return FPC_EINVAL;
    return launch_mb_dwconv(in, w, scale, shift, out, B, Hi, Wi, C, k, stride, act, (hipStream_t)stream);
}

extern "C" int fpc_dwconv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int stride,
                                   fpc_stream_t stream) {
    if (!dy || !w || !dx || !al16(dy) || !al16(w) || !al16(dx) || !dw_shape_ok(B, Hi, Wi, C, stride)) return FPC_EINVAL;
    return launch_dw_dgrad(dy, w, dx, B, Hi, Wi, (Hi - 1) / stride + 1, (Wi - 1) / stride + 1, C, 3, stride, false, (hipStream_t)stream);
}

extern "C" int fpc_mbconv_dw_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int k, int stride,
                                   fpc_stream_t stream) {
    if (!dy || !w || !dx || !al16(dy) || !al16(w) || !al16(dx) || !mb_dw_shape_ok(B, Hi, Wi, C, k, stride)) return FPC_EINVAL;
    return launch_dw_dgrad(dy, w, dx, B, Hi, Wi, Hi / stride, Wi / stride, C, k, stride, true, (hipStream_t)stream);
}

// workspace: the slices' partials, [slices][C][k k] floats (0: a shape the call refuses); the slice count is this size over 4 k k C
extern "C" size_t fpc_dwconv3x3_wgrad_workspace_bytes(int B, int Ho, int Wo, int C) {
    if (!dw_shape_ok(B, Ho, Wo, C, 1)) return 0;
    return (size_t)dw_wgrad_slices(B, Ho, Wo, C, dw_wgrad_slots(3)) * C * 9 * sizeof(float);
}

extern "C" size_t fpc_mbconv_dw_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int k) {
    if (!mb_dw_shape_ok(B, Ho, Wo, C, k, 1)) return 0;
    return (size_t)dw_wgrad_slices(B, Ho, Wo, C, dw_wgrad_slots(k)) * C * k * k * sizeof(float);
}

extern "C" int fpc_dwconv3x3_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int stride, void* ws,
                                   size_t ws_bytes, fpc_stream_t stream) {
    if (!x || !dy || !dw || !ws || !al16(x) || !al16(dy) || !al16(dw) || !dw_shape_ok(B, Hi, Wi, C, stride)) return FPC_EINVAL;
    const int Ho = (Hi - 1) / stride + 1, Wo = (Wi - 1) / stride + 1;
    if (((uintptr_t)ws & 255) || ws_bytes < fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)) return FPC_EWORKSPACE;
    return launch_dw_wgrad(x, dy, dw, B, Hi, Wi, Ho, Wo, C, 3, stride, false, ws, (hipStream_t)stream);
}

extern "C" int fpc_mbconv_dw_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int k, int stride, void* ws,
                                   size_t ws_bytes, fpc_stream_t stream) {
    if (!x || !dy || !dw || !ws || !al16(x) || !al16(dy) || !al16(dw) || !mb_dw_shape_ok(B, Hi, Wi, C, k, stride)) return FPC_EINVAL;
    const int Ho = Hi / stride, Wo = Wi / stride;
    if (((uintptr_t)ws & 255) || ws_bytes < fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k)) return FPC_EWORKSPACE;
    return launch_dw_wgrad(x, dy, dw, B, Hi, Wi, Ho, Wo, C, k, stride, true, ws, (hipStream_t)stream);
}
