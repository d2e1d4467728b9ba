// mbconv_train.hip — data and weight gradients of the static-"same" depthwise K x K convolution of the EfficientNet-B0 encoder
// (efficientnet.hip's k_mb_dwconv<K, S> is the forward, in training too: act 0, scale 1, shift 0), for the training step:
// fpc_mbconv_dw_dgrad and fpc_mbconv_dw_wgrad.  dwconv_train.hip's conventions: dense channel-last f32, C a multiple of 4, K 3 or 5,
// stride 1 or 2, lanes along the channel quads with 16-byte loads and stores, the weights torch's [C][1][K][K] read and written in
// place.  Plain f32 FMAs in an order the shape alone fixes, no atomics, no float division, no scratch: results are bit-identical
// run to run (DESIGN.md 4.2a''''''''').  The pads are the forward's compile-time constants: pad-before PB = (K - 1) / 2 at stride 1,
// (K - 3) / 2 at stride 2 (even extents only), Ho = Hi / stride.  (K, stride) = (3, 1) is pad 1 on every side: the entries hand it
// to fpc_dwconv3x3_dgrad / _wgrad (dwconv_train.hip), whose kernels are not touched.
//
// Data gradient, stride 1 (K = 5): k_mb_dw_dgrad_s1<K>, the forward's strip loop over dy with the taps flipped,
// dx[h][w] = sum dy[h + PB - kh][w + PB - kw] w[kh][kw]: one thread per (row, strip of 4 columns, channel quad); the K rows of dy
// stay a loop, each with its own 4 x K weights, as k_mb_dwconv<5, S> (100 hoisted weights plus the window do not fit).
//
// Data gradient, stride 2: k_mb_dw_dgrad_s2<K>.  Per axis dx[i] = sum over the taps k with i + PB - k even of dy[(i + PB - k) / 2] w[k]:
//   K = 3, PB 0:  dx[2a] = dy[a] w[0] + dy[a - 1] w[2],  dx[2a + 1] = dy[a] w[1]                               9 products per block
//   K = 5, PB 1:  dx[2a] = dy[a] w[1] + dy[a - 1] w[3],  dx[2a + 1] = dy[a + 1] w[0] + dy[a] w[2] + dy[a - 1] w[4]      25 products
// no zero insertion.  One thread per (block row a, strip of 2 blocks, channel quad); it writes the block's two rows of dx one after
// the other, each from the tap rows of its parity in ascending kh, a tap row from one row of dy (4 quads) in ascending kw.
//
// Weight gradient: k_mb_dw_wgrad<K, S>, then k_mb_dw_wgrad_reduce: dwconv_train.hip's scheme.  The (frame, output row) list is cut
// into mb_dw_wgrad_slices(B, Ho, Wo, C, K) contiguous slices; a workgroup takes one slice for a chunk of 8 channel quads.  K = 3: 256
// threads, a thread holds a quad's 36 accumulators, 32 pixel slots.  K = 5: a quad's 100 accumulators do not fit beside five sliding
// rows, so the taps are split over threads — a thread per (channel quad, tap row kh) holds 4 x 5 accumulators and one row's 5
// sliding column quads —, 320 threads, 8 pixel slots of 8 quads x 5 tap rows.  A slot takes the slice's (row, segment of 8 output
// columns) units u = slot, slot + slots, ... and walks a segment with the x columns sliding in registers.  The slots are added
// pairwise through LDS (slot s + h into slot s, h = slots / 2 .. 1), the workgroup writes ONE partial [slice][C][K K]; the second
// launch adds the slices in double — sixteen contiguous ranges of slices, each in ascending order, then the ranges in ascending
// order — and writes OIHW.
#include <algorithm>

#include "conv_device.hpp"

namespace fpc {

namespace {

constexpr long long kMbWalkLimit = (1LL << 32) - 4096LL * 256 - 8;      // efficientnet.hip's kWalkLimit: the 32-bit walks' bound

constexpr int mb_pad_before(int K, int S) { return S == 1 ? (K - 1) / 2 : (K - 3) / 2; }

// ---- data gradient --------------------------------------------------------------------------------------------------------------

// dy, dx [B][H][W][C] (stride 1: one shape), w [C][1][K][K]; total = B H WT CQ items with WT strips of 4 columns per row
template <int K>
__global__ __launch_bounds__(256) void k_mb_dw_dgrad_s1(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                        unsigned total, int H, int W, int WT, int CQ) {
    constexpr int TW = 4, NC = TW + K - 1, PB = mb_pad_before(K, 1);
    const int C = 4 * CQ;
    const XcdWalk wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned h = t % (unsigned)H, b = t / (unsigned)H;
        const float* wq = w + 4 * K * K * (size_t)cq;
        f32x4 acc[TW];
#pragma unroll
        for (int o = 0; o < TW; ++o) acc[o] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int w0 = (int)wt * TW;
#pragma unroll 1
        for (int r = 0; r < K; ++r) {      // the row of dy at h - PB + r meets the tap row kh = K - 1 - r
            const int kh = K - 1 - r;
            float wf[4 * K];               // [channel of the quad][kw]
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int kw = 0; kw < K; ++kw) wf[K * j + kw] = wq[K * K * j + K * kh + kw];
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
                    for (int j = 0; j < 4; ++j) acc[o][j] = fmaf(d[o + s][j], wf[K * j + (K - 1 - s)], acc[o][j]);
        }
#pragma unroll
        for (int o = 0; o < TW; ++o)
            if (w0 + o < W) *reinterpret_cast<f32x4*>(dx + (((size_t)b * H + h) * W + w0 + o) * C + 4 * cq) = acc[o];
    }
}

// One row of dx, y = 2 a + PY, of the blocks b0, b0 + 1: the tap rows kh = K0, K0 + 2, ... of parity PY, tap row kh from the row
// a + (PY + PB - kh) / 2 of dy
template <int K, int PY>
__device__ __forceinline__ void mb_dgrad_s2_row(const float* __restrict__ dyb, const float* __restrict__ wq, float* __restrict__ dxrow,
                                                int a, int b0, int Ho, int Wo, int C) {
    constexpr int TB = 2, PB = mb_pad_before(K, 2);
    constexpr int K0 = (PY + PB) & 1, NT = (K - K0 + 1) / 2;      // tap rows of this parity
    constexpr int OMIN = -1, OMAX = (K - 3) / 2, NC = TB + OMAX - OMIN;      // offsets into dy a tap can have: K 3 -1..0, K 5 -1..1
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
    for (int i = 0; i < TB; ++i) {
        if (b0 + i >= Wo) continue;
#pragma unroll
        for (int px = 0; px < 2; ++px) *reinterpret_cast<f32x4*>(dxrow + (size_t)(2 * (b0 + i) + px) * C) = acc[i][px];
    }
}

// dy [B][Ho][Wo][C], dx [B][2 Ho][2 Wo][C]; total = B Ho WT CQ items with WT strips of 2 blocks
template <int K>
__global__ __launch_bounds__(256) void k_mb_dw_dgrad_s2(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                        unsigned total, int Ho, int Wo, int WT, int CQ) {
    const int C = 4 * CQ;
    const XcdWalk wk = xcd_walk(total);
    for (unsigned g = wk.first; g < wk.end; g += wk.step) {
        const unsigned cq = g % (unsigned)CQ;
        unsigned t = g / (unsigned)CQ;
        const unsigned wt = t % (unsigned)WT;
        t /= (unsigned)WT;
        const unsigned a = t % (unsigned)Ho, b = t / (unsigned)Ho;
        const float* wq = w + 4 * K * K * (size_t)cq;
        const float* dyb = dy + (size_t)b * Ho * Wo * C + 4 * cq;
        float* dxb = dx + ((size_t)b * 2 * Ho + 2 * a) * (2 * (size_t)Wo) * C + 4 * cq;
        mb_dgrad_s2_row<K, 0>(dyb, wq, dxb, (int)a, 2 * (int)wt, Ho, Wo, C);
        mb_dgrad_s2_row<K, 1>(dyb, wq, dxb + 2 * (size_t)Wo * C, (int)a, 2 * (int)wt, Ho, Wo, C);
    }
}

// ---- weight gradient ------------------------------------------------------------------------------------------------------------

constexpr int kMbQuads = 8;                    // channel quads per workgroup: 128 bytes of a pixel
constexpr int kMbSeg = 8;                      // output columns of a unit
constexpr int kMbRanges = 16;                  // k_mb_dw_wgrad_reduce: contiguous ranges of slices per sum
constexpr int mb_wgrad_threads(int K) { return K == 5 ? 320 : 256; }
constexpr int mb_wgrad_slots(int K) { return K == 5 ? 8 : 32; }      // pixel slots per workgroup

struct MbWgradArgs {
    const float* x;       // [B][Hi][Wi][C]
    const float* dy;      // [B][Ho][Wo][C]
    float* part;          // [nslice][C][K K]
    int B, Hi, Wi, Ho, Wo, C, CQ;
    int nchunk, nslice, nseg;
    unsigned blocks;      // nchunk * nslice
};

template <int K, int S>
__global__ __launch_bounds__(mb_wgrad_threads(K)) void k_mb_dw_wgrad(const MbWgradArgs a) {
    constexpr int PB = mb_pad_before(K, S);
    constexpr int KHT = K == 5 ? 1 : K;                 // tap rows a thread holds
    constexpr int TPS = kMbQuads * (K / KHT);           // threads of a pixel slot
    constexpr int SLOTS = mb_wgrad_slots(K), HALF = SLOTS / 2 * TPS, NACC = 4 * KHT * K;
    static_assert(SLOTS * TPS == mb_wgrad_threads(K), "threads = slots x quads x tap rows");
    __shared__ float red[NACC * HALF];
    // XCD-aware order: the workgroups of one XCD take a contiguous eighth of the (slice, chunk) list (the ids past it leave before
    // any barrier)
    unsigned bid = blockIdx.x;
    if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    if (bid >= a.blocks) return;
    const int chunk = (int)(bid % (unsigned)a.nchunk), slice = (int)(bid / (unsigned)a.nchunk);
    const int tid = threadIdx.x, q = tid % kMbQuads, kh0 = (tid / kMbQuads) % (K / KHT) * KHT, slot = tid / TPS;
    const int qg = chunk * kMbQuads + q;
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
            const int w0 = seg * kMbSeg, w1 = min(a.Wo, w0 + kMbSeg);
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
__global__ __launch_bounds__(256) void k_mb_dw_wgrad_reduce(const float* __restrict__ part, float* __restrict__ dw, int n4, int nslice) {
    __shared__ double sh[kMbRanges][16][4];
    const int t = threadIdx.x, c = t & 15, r = t >> 4;
    const int i4 = blockIdx.x * 16 + c;
    const int s0 = (int)((long long)r * nslice / kMbRanges), s1 = (int)((long long)(r + 1) * nslice / kMbRanges);
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
        for (int k = 1; k < kMbRanges; ++k) v += sh[k][c][e];
        o[e] = (float)v;
    }
    *reinterpret_cast<f32x4*>(dw + 4 * (size_t)i4) = o;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline bool mb_dw_shape_ok(int B, int Hi, int Wi, int C, int k, int stride) {
    return B >= 1 && Hi >= 1 && Wi >= 1 && C >= 4 && C % 4 == 0 && (k == 3 || k == 5) && (stride == 1 || stride == 2) &&
           !(stride == 2 && ((Hi | Wi) & 1)) &&                     // (an odd extent would need another pad table: fpc_mbconv_dw)
           (long long)B * Hi * Wi * (C / 4) < kMbWalkLimit;      // every kernel's item count is at most this
}

// Slices of the weight gradient's (frame, output row) list, a function of (B, Ho, Wo, C, k) alone (include/fpc.h states it): enough
// for four workgroups per compute unit over the channel chunks, at most one per row, and no more than leave every slice one unit
// of 8 output columns per pixel slot (32 slots at k = 3 — fpc_dwconv3x3_wgrad's count —, 8 at k = 5).
int mb_dw_wgrad_slices(int B, int Ho, int Wo, int C, int k) {
    const long long rows = (long long)B * Ho, nseg = cdiv(Wo, kMbSeg), chunks = cdiv(C / 4, kMbQuads);
    long long n = std::max<long long>(1, 1024 / chunks);
    n = std::min(n, rows * nseg / mb_wgrad_slots(k));
    n = std::min(n, rows);
    return (int)std::max<long long>(1, n);
}

}  // namespace

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_mbconv_dw_dgrad(const float* dy, const float* w, float* dx, int B, int Hi, int Wi, int C, int k, int stride,
                                   fpc_stream_t stream) {
    if (!dy || !w || !dx || !al16(dy) || !al16(w) || !al16(dx) || !mb_dw_shape_ok(B, Hi, Wi, C, k, stride)) return FPC_EINVAL;
    if (k == 3 && stride == 1) return fpc_dwconv3x3_dgrad(dy, w, dx, B, Hi, Wi, C, 1, stream);      // pad 1 on every side
    hipStream_t s = (hipStream_t)stream;
    if (stride == 1) {
        const int WT = cdiv(Wi, 4);
        const long long total = (long long)B * Hi * WT * (C / 4);
        hipLaunchKernelGGL(k_mb_dw_dgrad_s1<5>, dim3(stream_grid(total)), dim3(256), 0, s, dy, w, dx, (unsigned)total, Hi, Wi, WT, C / 4);
    } else {
        const int Ho = Hi / 2, Wo = Wi / 2, WT = cdiv(Wo, 2);
        const long long total = (long long)B * Ho * WT * (C / 4);
        if (k == 3) hipLaunchKernelGGL(k_mb_dw_dgrad_s2<3>, dim3(stream_grid(total)), dim3(256), 0, s, dy, w, dx, (unsigned)total, Ho, Wo, WT, C / 4);
        else hipLaunchKernelGGL(k_mb_dw_dgrad_s2<5>, dim3(stream_grid(total)), dim3(256), 0, s, dy, w, dx, (unsigned)total, Ho, Wo, WT, C / 4);
    }
    return check_launch();
}

// workspace: the slices' partials, [slices][C][k k] floats (0: a shape the call refuses); the slice count is this size over 4 k k C
extern "C" size_t fpc_mbconv_dw_wgrad_workspace_bytes(int B, int Ho, int Wo, int C, int k) {
    if (!mb_dw_shape_ok(B, Ho, Wo, C, k, 1)) return 0;
    return (size_t)mb_dw_wgrad_slices(B, Ho, Wo, C, k) * C * k * k * sizeof(float);
}

extern "C" int fpc_mbconv_dw_wgrad(const float* x, const float* dy, float* dw, int B, int Hi, int Wi, int C, int k, int stride, void* ws,
                                   size_t ws_bytes, fpc_stream_t stream) {
    if (!x || !dy || !dw || !ws || !al16(x) || !al16(dy) || !al16(dw) || !mb_dw_shape_ok(B, Hi, Wi, C, k, stride)) return FPC_EINVAL;
    const int Ho = Hi / stride, Wo = Wi / stride;
    if (((uintptr_t)ws & 255) || ws_bytes < fpc_mbconv_dw_wgrad_workspace_bytes(B, Ho, Wo, C, k)) return FPC_EWORKSPACE;
    if (k == 3 && stride == 1) return fpc_dwconv3x3_wgrad(x, dy, dw, B, Hi, Wi, C, 1, ws, ws_bytes, stream);      // (the same slice count)
    MbWgradArgs a;
    a.x = x; a.dy = dy; a.part = (float*)ws;
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Ho = Ho; a.Wo = Wo; a.C = C; a.CQ = C / 4;
    a.nchunk = cdiv(a.CQ, kMbQuads); a.nslice = mb_dw_wgrad_slices(B, Ho, Wo, C, k); a.nseg = cdiv(Wo, kMbSeg);
    const long long blocks = (long long)a.nchunk * a.nslice;      // (at most max(nchunk, 1024))
    a.blocks = (unsigned)blocks;
    const unsigned grid = (unsigned)(blocks >= 8 ? (blocks + 7) / 8 * 8 : blocks);
    hipStream_t s = (hipStream_t)stream;
    if (k == 3) hipLaunchKernelGGL((k_mb_dw_wgrad<3, 2>), dim3(grid), dim3(mb_wgrad_threads(3)), 0, s, a);
    else if (stride == 1) hipLaunchKernelGGL((k_mb_dw_wgrad<5, 1>), dim3(grid), dim3(mb_wgrad_threads(5)), 0, s, a);
    else hipLaunchKernelGGL((k_mb_dw_wgrad<5, 2>), dim3(grid), dim3(mb_wgrad_threads(5)), 0, s, a);
    int rc = check_launch();
    if (rc) return rc;
    const int n4 = C * k * k / 4;
    hipLaunchKernelGGL(k_mb_dw_wgrad_reduce, dim3(cdiv(n4, 16)), dim3(256), 0, s, (const float*)ws, dw, n4, a.nslice);
    return check_launch();
}
