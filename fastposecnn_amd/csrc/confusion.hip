// confusion.hip — the confusion matrix of the arg-max mask against the ground-truth mask, accumulated on the device: the
// sufficient statistic of every per-class mask metric (IoU, dice, F1; lib/metrics_device.py).  The reference takes its
// mask metrics from pl.metrics.functional (F/train.py:190-207); Lightning is not a dependency here.
// Bandwidth-bound: 16 B per pixel (two i64 labels).  Each thread loads two pixels of each plane as one 16-byte vector,
// four such loads in flight per plane; a wave counts into its own u32 histograms in LDS (no traffic between waves): as
// many copies of the C x C cells as fit its 4 KB, up to 16, lane l using copy l mod R, so that lanes meeting one cell queue
// on R addresses and not on one; and where a whole wave meets one cell (background, the inside of an object) one lane adds
// the wave's count.  A workgroup flushes its non-zero cells once, with 64-bit integer atomics, so the global state cannot
// wrap at 2^32 and the result does not depend on the order of arrival.
#include "common.hpp"

namespace fpc {

constexpr int kCfMaxClasses = 32, kCfCells = kCfMaxClasses * kCfMaxClasses;
constexpr int kCfThreads = 256, kCfWaves = kCfThreads / kWave, kCfUnroll = 4;
constexpr int kCfMaxBlocks = 1024;                      // 4 workgroups of 4 waves on each of 256 CUs: 128 KB of loads in flight per CU
constexpr int kCfMaxCopies = 16;

typedef long long i64x2 __attribute__((ext_vector_type(2)));

// one pixel into the wave's histograms (`mine`: this lane's copy); returns 1 for a pixel left out.  `active`: this lane holds a pixel.
__device__ __forceinline__ unsigned count_pixel(unsigned* hist, unsigned* mine, bool active, long long g, long long p, int C) {
    const bool in = active && g >= 0 && g < C && p >= 0 && p < C;
    const int key = in ? (int)g * C + (int)p : -1;     // < C * C <= kCfCells
    const int first = __builtin_amdgcn_readfirstlane(key);
    const unsigned long long same = __ballot(key == first);
    if (same == __ballot(true)) {                       // (wave-uniform) every lane here meets the same cell
        if (first >= 0 && key == first && (int)__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u)) == 0)
            atomicAdd(hist + first, (unsigned)__popcll(same));
    } else if (in) {
        atomicAdd(mine + key, 1u);
    }
    return (active && !in) ? 1u : 0u;
}

// grid (<= kCfMaxBlocks), block 256.  kVec: both planes 16-byte aligned.  npairs = n / 2; an odd n's last pixel goes to thread 0.
template <bool kVec>
__global__ __launch_bounds__(kCfThreads) void k_confusion(const long long* __restrict__ pred, const long long* __restrict__ gt,
                                                          long long n, int C, unsigned long long* __restrict__ state) {
    __shared__ unsigned s_hist[kCfWaves][kCfCells];
    __shared__ unsigned s_skip[kCfWaves];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int cells = C * C;
    int copies = 1;                                     // R: the largest power of two with R * C * C <= 1024, at most 16
    while (copies < kCfMaxCopies && 2 * copies * cells <= kCfCells) copies *= 2;
    for (int k = lane; k < copies * cells; k += kWave) s_hist[wave][k] = 0u;
    __syncthreads();
    unsigned* hist = s_hist[wave];
    unsigned* mine = hist + (lane & (copies - 1)) * cells;
    unsigned skipped = 0;
    const long long npairs = n >> 1, stride = (long long)gridDim.x * kCfThreads;
    for (long long base = (long long)blockIdx.x * kCfThreads + tid; base - tid < npairs; base += stride * kCfUnroll) {
        // (the loop condition is uniform over the workgroup: `base - tid` is the workgroup's first pair)
        i64x2 pv[kCfUnroll], gv[kCfUnroll];
        bool on[kCfUnroll];
#pragma unroll
        for (int u = 0; u < kCfUnroll; ++u) {
            const long long q = base + u * stride;
            on[u] = q < npairs;
            pv[u] = i64x2{0, 0};
            gv[u] = i64x2{0, 0};
            if (on[u]) {
                if (kVec) {
                    pv[u] = *reinterpret_cast<const i64x2*>(pred + 2 * q);
                    gv[u] = *reinterpret_cast<const i64x2*>(gt + 2 * q);
                } else {
                    pv[u] = i64x2{pred[2 * q], pred[2 * q + 1]};
                    gv[u] = i64x2{gt[2 * q], gt[2 * q + 1]};
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kCfUnroll; ++u) {
            skipped += count_pixel(hist, mine, on[u], gv[u].x, pv[u].x, C);
            skipped += count_pixel(hist, mine, on[u], gv[u].y, pv[u].y, C);
        }
    }
    {
        const bool tail = (n & 1) && blockIdx.x == 0 && tid == 0;        // wave 0 of workgroup 0, all its lanes call
        if (blockIdx.x == 0 && wave == 0) skipped += count_pixel(hist, mine, tail, tail ? gt[n - 1] : 0, tail ? pred[n - 1] : 0, C);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) skipped += __shfl_down(skipped, o, kWave);
    if (lane == 0) s_skip[wave] = skipped;
    __syncthreads();
    for (int k = tid; k < cells; k += kCfThreads) {
        unsigned long long s = 0;
        for (int w = 0; w < kCfWaves; ++w)
            for (int r = 0; r < copies; ++r) s += s_hist[w][r * cells + k];
        if (s) atomicAdd(state + k, s);
    }
    if (tid == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kCfWaves; ++w) s += s_skip[w];
        if (s) atomicAdd(state + cells, s);
    }
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_confusion_update(const int64_t* pred, const int64_t* gt, int64_t n, int num_classes, int64_t* state,
                                    fpc_stream_t stream) {
    if (n < 0 || num_classes < 1 || num_classes > kCfMaxClasses) return FPC_EINVAL;
    if (n == 0) return FPC_OK;
    if (!pred || !gt || !state) return FPC_EINVAL;
    const long long per_block = (long long)kCfThreads * kCfUnroll;
    const long long want = ((n >> 1) + per_block - 1) / per_block;
    const int blocks = (int)(want < 1 ? 1 : (want > kCfMaxBlocks ? kCfMaxBlocks : want));
    const bool vec = ((uintptr_t)pred % 16 == 0) && ((uintptr_t)gt % 16 == 0);
    auto* p = reinterpret_cast<const long long*>(pred);
    auto* g = reinterpret_cast<const long long*>(gt);
    auto* s = reinterpret_cast<unsigned long long*>(state);
    if (vec) hipLaunchKernelGGL(k_confusion<true>, dim3(blocks), dim3(kCfThreads), 0, (hipStream_t)stream, p, g, (long long)n, num_classes, s);
    else hipLaunchKernelGGL(k_confusion<false>, dim3(blocks), dim3(kCfThreads), 0, (hipStream_t)stream, p, g, (long long)n, num_classes, s);
    return check_launch();
}
