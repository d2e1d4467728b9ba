// eval.hip — the evaluation maths right after the matching, one launch for all matched pairs:
//   degree error     F/lib/gpu_tensor_funcs.py:411-476  get_quat_distance / get_raw_quat_distance / get_symmetric_quat_distance
//   3-D IoU          :486-547  get_3d_ious -> get_asymmetric_3d_iou
//   offset error     :563-565  from_Ts_get_offset_error
// The reference runs ~40 small torch kernels per metric and a Python loop over the pairs for the IoU (a 4x4 torch.inverse
// and ~25 launches per pair).  One wave per pair here: the lanes share the 360 rotations of the symmetric distance; lanes
// 0-15 transform the sixteen box corners.  The per-pair arithmetic, its dtypes and the reference quirks it keeps are in
// pose_errors.hpp, shared with the metric accumulator (pose_metrics.hip).
#include "pose_errors.hpp"

namespace fpc {

// grid (n), block 64
__global__ __launch_bounds__(64) void k_pose_errors(const float* __restrict__ q0, const float* __restrict__ q1,
                                                    const int64_t* __restrict__ sym, const float* __restrict__ rot /* [nrot,4] */,
                                                    int nrot, const float* __restrict__ RT1, const float* __restrict__ RT2,
                                                    const float* __restrict__ sc1, const float* __restrict__ sc2,
                                                    const float* __restrict__ T1, const float* __restrict__ T2,
                                                    double* __restrict__ out_deg, float* __restrict__ out_iou,
                                                    float* __restrict__ out_off) {
    const int i = blockIdx.x, lane = threadIdx.x;
    if (out_deg) {
        const double d = pair_degree_error(q0 + (size_t)i * 4, q1 + (size_t)i * 4, sym && sym[i] != 0, rot, nrot, lane);
        if (lane == 0) out_deg[i] = d;
    }
    if (out_off && lane == 0) out_off[i] = pair_offset_error(T1 + (size_t)i * 3, T2 + (size_t)i * 3);
    if (out_iou) {
        const float v = pair_iou3d(RT1 + (size_t)i * 16, RT2 + (size_t)i * 16, sc1 + (size_t)i * 3, sc2 + (size_t)i * 3, lane);
        if (lane == 0) out_iou[i] = v;
    }
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_pose_errors(const float* q0, const float* q1, const int64_t* symmetric_ids, const float* rot, int nrot,
                               const float* RT1, const float* RT2, const float* scales1, const float* scales2,
                               const float* T1, const float* T2, int n, double* out_degree, float* out_iou3d,
                               float* out_offset, fpc_stream_t stream) {
    if (n < 0 || nrot < 0) return FPC_EINVAL;
    if (n == 0) return FPC_OK;
    if (out_degree && (!q0 || !q1 || (symmetric_ids && (!rot || nrot < 1)))) return FPC_EINVAL;
    if (out_iou3d && (!RT1 || !RT2 || !scales1 || !scales2)) return FPC_EINVAL;
    if (out_offset && (!T1 || !T2)) return FPC_EINVAL;
    hipLaunchKernelGGL(k_pose_errors, dim3(n), dim3(64), 0, (hipStream_t)stream, q0, q1, symmetric_ids, rot, nrot, RT1, RT2, scales1,
                       scales2, T1, T2, out_degree, out_iou3d, out_offset);
    return check_launch();
}
