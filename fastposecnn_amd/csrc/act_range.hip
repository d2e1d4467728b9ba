// act_range.hip — k_act_range: the survey pass behind fpc_net_survey_next (net.hip) and fpc_act_range (fpc.h).  One read of a
// contiguous f32 tensor, accumulated into a 4-word record: rec[0] = the bits of max |x| over the FINITE elements (a non-negative
// float: atomicMax on the unsigned word keeps the order), rec[1] += the number of non-finite elements, rec[2] += n (saturating at
// 2^32 - 1), rec[3] is not touched.  The record accumulates over launches: the caller zeroes it.  gfx950 only.
#include <algorithm>

#include "net_kernels.hpp"

namespace fpc {

namespace {

constexpr unsigned kAbsMask = 0x7fffffffu, kInfBits = 0x7f800000u;
constexpr int kRangeThreads = 256;
// The grid's cap.  The pass is memory-bound: eight 256-thread workgroups per CU (all 32 wave slots of each of the 256 CUs) keep the
// most 16-byte loads in flight, and a grid-stride loop takes the rest, so a 32-frame p2 tensor (2.5 GB) is read by the whole chip and
// ends in at most 2 048 same-address atomics per word.  Their cost is an estimate, not measured for this kernel: k_absmax_bits's
// 4 096 took 48 us, so ~24 us here against ~0.5 ms for reading that tensor, a few percent.  A small tensor launches one workgroup
// per 1 024 elements.
constexpr int kRangeMaxGrid = 256 * 8;

__device__ __forceinline__ void range_one(unsigned bits, unsigned& m, unsigned& bad) {
    const unsigned b = bits & kAbsMask;          // |x|: -0.0 -> 0, subnormals keep their order
    const bool nf = b >= kInfBits;               // inf or NaN
    bad += nf ? 1u : 0u;
    m = max(m, nf ? 0u : b);
}

}  // namespace

// head: the 0..3 elements in front of the first 16-byte boundary; n4: whole 16-byte groups behind them; the rest is the tail
__global__ __launch_bounds__(kRangeThreads) void k_act_range(const float* __restrict__ x, long long n, int head, long long n4,
                                                             unsigned* rec) {
    __shared__ unsigned s_m[kRangeThreads / kWave], s_bad[kRangeThreads / kWave];
    unsigned m = 0u, bad = 0u;
    const f32x4* __restrict__ body = reinterpret_cast<const f32x4*>(x + head);
    for (long long g = (long long)blockIdx.x * kRangeThreads + threadIdx.x; g < n4; g += (long long)gridDim.x * kRangeThreads) {
        const f32x4 v = body[g];
        const float v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
        range_one(__builtin_bit_cast(unsigned, v0), m, bad);
        range_one(__builtin_bit_cast(unsigned, v1), m, bad);
        range_one(__builtin_bit_cast(unsigned, v2), m, bad);
        range_one(__builtin_bit_cast(unsigned, v3), m, bad);
    }
    if (blockIdx.x == 0) {      // scalar head and tail: at most 3 elements each
        const long long tail0 = head + 4 * n4;
        if ((int)threadIdx.x < head) range_one(__builtin_bit_cast(unsigned, x[threadIdx.x]), m, bad);
        if (tail0 + threadIdx.x < n) range_one(__builtin_bit_cast(unsigned, x[tail0 + threadIdx.x]), m, bad);
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        m = max(m, (unsigned)__shfl_xor((int)m, o, kWave));
        bad += (unsigned)__shfl_xor((int)bad, o, kWave);
    }
    if ((threadIdx.x & (kWave - 1)) == 0) { s_m[threadIdx.x / kWave] = m; s_bad[threadIdx.x / kWave] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        m = 0u; bad = 0u;
#pragma unroll
        for (int w = 0; w < kRangeThreads / kWave; ++w) { m = max(m, s_m[w]); bad += s_bad[w]; }
        if (m) atomicMax(rec, m);               // (a zero maximum changes nothing)
        if (bad) atomicAdd(rec + 1, bad);
        if (blockIdx.x == 0) {                  // the visit count, once per launch, saturating
            unsigned seen = rec[2], next;
            do {
                const unsigned long long sum = (unsigned long long)seen + (unsigned long long)n;
                next = sum > 0xffffffffull ? 0xffffffffu : (unsigned)sum;
                if (next == seen) break;
                const unsigned was = atomicCAS(rec + 2, seen, next);
                if (was == seen) break;
                seen = was;
            } while (true);
        }
    }
}

int launch_act_range(const float* x, long long n, unsigned* rec, hipStream_t s) {
    if (n < 0 || !rec || (n > 0 && !x) || ((uintptr_t)x & 3) || ((uintptr_t)rec & 3)) return FPC_EINVAL;
    if (n == 0) return FPC_OK;      // nothing visited: the record stays as it is
    const int head = (int)std::min<long long>(n, (long long)((16 - ((uintptr_t)x & 15)) & 15) / 4);
    const long long n4 = (n - head) / 4;
    const long long want = (n4 + 4 * kRangeThreads - 1) / (4 * kRangeThreads);      // four 16-byte loads per lane
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, kRangeMaxGrid));
    hipLaunchKernelGGL(k_act_range, dim3(grid), dim3(kRangeThreads), 0, s, x, n, head, n4, rec);
    return check_launch();
}

}  // namespace fpc

extern "C" int fpc_act_range(const float* x, long long n, unsigned* rec4, fpc_stream_t s) {
    return fpc::launch_act_range(x, n, rec4, (hipStream_t)s);
}
