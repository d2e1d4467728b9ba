// gt_build.hip — the ground-truth batch from instance-id masks (tools/dataset.py: GroundTruthUploader), the twin of
// k_agg_planes_img (aggregate.hip) on the ground-truth side:
//   class mask       F/tools/dataset.py:183-228 (the per-instance sweeps of __getitem__) as one table lookup per pixel
//   instance planes  F/tools/dataset.py:373-434 (generate_agg_data's instance_masks), one [H,W] plane per row of agg_data
// The host decides WHICH instance id of WHICH frame becomes which row (two 256-entry tables per frame, from the side file
// alone); this kernel applies the tables and nothing else.  A workgroup takes 4096 pixels of one frame: the ids are read
// once with the widest loads the stride allows, mapped through the tables (LDS) to a row index and a class per pixel, and
// staged in LDS so that every OUTPUT is then written by consecutive lanes to consecutive 16 bytes whatever its element
// size (two int64 / two f64 / four f32 / sixteen u8 per lane and store).  A thread's sixteen row indices stay in
// registers while it loops over the frame's rows first_row[b] .. first_row[b+1]; every plane is written in full (ones and
// zeros), with streaming stores: nothing here reads them back.  Written bytes = n H W elem + 8 B H W: the roofline figure.
#include "common.hpp"

namespace fpc {

constexpr int kGtThreads = 256, kGtChunk = 16 * kGtThreads, kGtCntTile = 64;

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct GtArgs {
    const uint8_t* ids;
    int64_t pix_stride, frame_stride;
    int HW, chunks, n;
    const int16_t* row_of;
    const uint8_t* class_of;
    const int32_t* first_row;
    int64_t* class_mask;
    uint8_t* inst;
    int32_t* pix_count;
};

// bit k of the low four -> byte k (0 / 1)
__device__ __forceinline__ unsigned bits_to_bytes(unsigned x) {
    return (x & 1u) | ((x & 2u) << 7) | ((x & 4u) << 14) | ((x & 8u) << 21);
}

// One group of PX = 16 / ELEM consecutive pixels of plane `dst` (element p of the chunk's part of the plane is at
// dst + p * ELEM), flag k of `bits` for pixel p + k.  vec: dst is 16-byte aligned (workgroup-uniform).
template <int ELEM>
__device__ __forceinline__ void gt_store_group(uint8_t* dst, int p, unsigned bits, bool vec, int left) {
    constexpr int PX = 16 / ELEM;
    if (p >= left) return;
    if (vec && p + PX <= left) {
        if constexpr (ELEM == 8) {
            __builtin_nontemporal_store(f64x2{(bits & 1u) ? 1.0 : 0.0, (bits & 2u) ? 1.0 : 0.0}, reinterpret_cast<f64x2*>(dst + (size_t)p * 8));
        } else if constexpr (ELEM == 4) {
            __builtin_nontemporal_store(f32x4{(bits & 1u) ? 1.f : 0.f, (bits & 2u) ? 1.f : 0.f, (bits & 4u) ? 1.f : 0.f, (bits & 8u) ? 1.f : 0.f},
                                        reinterpret_cast<f32x4*>(dst + (size_t)p * 4));
        } else {
            __builtin_nontemporal_store(u32x4{bits_to_bytes(bits), bits_to_bytes(bits >> 4), bits_to_bytes(bits >> 8), bits_to_bytes(bits >> 12)},
                                        reinterpret_cast<u32x4*>(dst + p));
        }
        return;
    }
    for (int k = 0; k < PX && p + k < left; ++k) {       // the chunk's tail, or a plane whose base is not 16-byte aligned
        const bool f = (bits >> k) & 1u;
        if constexpr (ELEM == 8) reinterpret_cast<double*>(dst)[p + k] = f ? 1.0 : 0.0;
        else if constexpr (ELEM == 4) reinterpret_cast<float*>(dst)[p + k] = f ? 1.f : 0.f;
        else dst[p + k] = f ? 1 : 0;
    }
}

// grid B * chunks, block 256.  ELEM: bytes per element of the instance planes (1 when there are none).
template <int ELEM>
__global__ __launch_bounds__(kGtThreads) void k_gt_build(const GtArgs a) {
    constexpr int PX = 16 / ELEM, G = 16 / PX;
    __shared__ __attribute__((aligned(16))) int16_t s_row[kGtChunk];
    __shared__ __attribute__((aligned(16))) uint8_t s_cls[kGtChunk];
    __shared__ int16_t s_rowof[256];
    __shared__ uint8_t s_clsof[256];
    __shared__ int s_cnt[kGtCntTile];
    const int t = threadIdx.x, lane = t & (kWave - 1);
    const int b = blockIdx.x / a.chunks, chunk = blockIdx.x - b * a.chunks;
    const int base = chunk * kGtChunk;                    // the chunk's first pixel in its frame
    const int left = min(a.HW - base, kGtChunk);          // its pixels: 1 .. 4096
    const uint8_t* src = a.ids + (int64_t)b * a.frame_stride + (int64_t)base * a.pix_stride;
    const bool src_al = ((uintptr_t)src & 15) == 0;
    // slot j of this thread is pixel pix(j) of the chunk; every pixel 0 .. 4095 is exactly one slot of one thread
    const int mode = (src_al && a.pix_stride == 1) ? 0 : (src_al && a.pix_stride == 4) ? 1 : 2;
    auto pix = [&](int j) { return mode == 0 ? 16 * t + j : mode == 1 ? 4 * ((j >> 2) * kGtThreads + t) + (j & 3) : j * kGtThreads + t; };
    unsigned id[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) id[j] = 0;
    if (mode == 0 && 16 * t + 16 <= left) {               // sixteen ids in one load
        const u32x4 v = *reinterpret_cast<const u32x4*>(src + 16 * t);
#pragma unroll
        for (int j = 0; j < 16; ++j) id[j] = (v[j >> 2] >> (8 * (j & 3))) & 255u;
    } else if (mode == 1) {                               // four RGBA pixels in one load, channel 0 of each
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int p = 4 * (g * kGtThreads + t);
            if (p + 4 <= left) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(src + (size_t)p * 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) id[4 * g + k] = v[k] & 255u;
            } else {
                for (int k = 0; k < 4 && p + k < left; ++k) id[4 * g + k] = src[(size_t)(p + k) * 4];
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int p = pix(j);
            if (p < left) id[j] = src[(int64_t)p * a.pix_stride];
        }
    }
    s_rowof[t] = a.row_of[(size_t)b * 256 + t];           // 256 threads, 256 entries
    s_clsof[t] = a.class_of[(size_t)b * 256 + t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int p = pix(j);
        const bool in = p < left;
        s_row[p] = in ? s_rowof[id[j]] : (int16_t)-1;
        s_cls[p] = in ? s_clsof[id[j]] : (uint8_t)0;
    }
    __syncthreads();

    if (a.class_mask) {
        int64_t* cm = a.class_mask + (size_t)b * a.HW + base;
        const bool vec = ((uintptr_t)cm & 15) == 0;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const int p = 2 * (g * kGtThreads + t);
            if (p >= left) continue;
            if (vec && p + 2 <= left) {
                __builtin_nontemporal_store(i64x2{(long long)s_cls[p], (long long)s_cls[p + 1]}, reinterpret_cast<i64x2*>(cm + p));
            } else {
                cm[p] = s_cls[p];
                if (p + 1 < left) cm[p + 1] = s_cls[p + 1];
            }
        }
    }

    const int lo = max(a.first_row[b], 0), hi = min(a.first_row[b + 1], a.n);      // rows outside 0 .. n-1 are never touched
    if (lo >= hi || (!a.inst && !a.pix_count)) return;
    int row[16];                                          // group g = pixels PX * (g * 256 + t) .. + PX - 1
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int k = 0; k < PX; ++k) row[g * PX + k] = s_row[PX * (g * kGtThreads + t) + k];
    for (int r0 = lo; r0 < hi; r0 += kGtCntTile) {
        const int r1 = min(r0 + kGtCntTile, hi);
        if (a.pix_count) {
            if (t < kGtCntTile) s_cnt[t] = 0;
            __syncthreads();
        }
        for (int r = r0; r < r1; ++r) {
            unsigned m = 0;
#pragma unroll
            for (int s = 0; s < 16; ++s) m |= (row[s] == r ? 1u : 0u) << s;
            if (a.inst) {
                uint8_t* plane = a.inst + ((size_t)r * a.HW + base) * ELEM;
                const bool vec = ((uintptr_t)plane & 15) == 0;
#pragma unroll
                for (int g = 0; g < G; ++g) gt_store_group<ELEM>(plane, PX * (g * kGtThreads + t), m >> (g * PX), vec, left);
            }
            if (a.pix_count && __ballot(m != 0)) {        // (wave-uniform) most rows have no pixel in most chunks
                const int w = wave_reduce_add((int)__popc(m));
                if (lane == 0) atomicAdd(&s_cnt[r - r0], w);
            }
        }
        if (a.pix_count) {
            __syncthreads();
            if (t < r1 - r0 && s_cnt[t] != 0) atomicAdd(a.pix_count + r0 + t, s_cnt[t]);
        }
    }
}

// standardize_depth(...).astype('float32') (tools/dataset.py): G * 256 + R of a colour-coded file, or the 16-bit sample
__global__ __launch_bounds__(256) void k_depth_decode(const void* __restrict__ src, int kind, int channels, int64_t total,
                                                      float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        if (kind == 0) {
            const uint8_t* p = static_cast<const uint8_t*>(src) + i * channels;
            out[i] = (float)(((unsigned)p[1] << 8) + p[0]);
        } else {
            out[i] = (float)static_cast<const uint16_t*>(src)[i];
        }
    }
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_gt_build(const uint8_t* ids, int64_t pix_stride, int64_t frame_stride, int B, int H, int W,
                            const int16_t* row_of, const uint8_t* class_of, const int32_t* first_row, int n,
                            int64_t* class_mask, void* inst_masks, int mask_elem, int32_t* pix_count, fpc_stream_t stream) {
    if (!ids || !row_of || !class_of || !first_row) return FPC_EINVAL;
    if (B < 1 || H < 1 || W < 1 || n < 0 || n > 32767) return FPC_EINVAL;
    if (pix_stride < 1 || pix_stride > 4) return FPC_EINVAL;
    const int64_t hw = (int64_t)H * W;
    if (hw > INT32_MAX - kGtChunk) return FPC_EINVAL;
    if (inst_masks) {
        if (mask_elem != 1 && mask_elem != 4 && mask_elem != 8) return FPC_EINVAL;
        if ((uintptr_t)inst_masks & 15) return FPC_EINVAL;
    }
    const int64_t chunks = (hw + kGtChunk - 1) / kGtChunk;
    if ((int64_t)B * chunks > INT32_MAX) return FPC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (pix_count && n > 0) {
        hipError_t e = hipMemsetAsync(pix_count, 0, (size_t)n * sizeof(int32_t), s);
        if (e != hipSuccess) { set_hip_error(e); return FPC_ELAUNCH; }
    }
    if (n == 0) inst_masks = nullptr, pix_count = nullptr;
    if (!class_mask && !inst_masks && !pix_count) return FPC_OK;
    GtArgs a{ids, pix_stride, frame_stride, (int)hw, (int)chunks, n, row_of, class_of, first_row, class_mask,
             static_cast<uint8_t*>(inst_masks), pix_count};
    const dim3 grid((unsigned)(B * chunks)), block(kGtThreads);
    const int elem = inst_masks ? mask_elem : 1;
    if (elem == 8) hipLaunchKernelGGL(k_gt_build<8>, grid, block, 0, s, a);
    else if (elem == 4) hipLaunchKernelGGL(k_gt_build<4>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(k_gt_build<1>, grid, block, 0, s, a);
    return check_launch();
}

extern "C" int fpc_depth_decode(const void* src, int src_kind, int channels, int B, int H, int W, float* depth_f32,
                                fpc_stream_t stream) {
    if (!src || !depth_f32 || B < 1 || H < 1 || W < 1) return FPC_EINVAL;
    if (src_kind != 0 && src_kind != 1) return FPC_EINVAL;
    if (src_kind == 0 && channels != 3 && channels != 4) return FPC_EINVAL;
    const int64_t total = (int64_t)B * H * W;
    const int64_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_depth_decode, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, (hipStream_t)stream, src, src_kind,
                       channels, total, depth_f32);
    return check_launch();
}
