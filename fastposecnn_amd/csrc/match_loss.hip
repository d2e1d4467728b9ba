// match_loss.hip — the training step's matching and matched losses without the host:
//   assignment       lib/matching.py:39-53 (F/lib/matching.py:252-299): per ground truth the first maximum of the IoU over the
//                    predictions of its class, NaN propagating, valid iff > 0; output order = ascending class, then index
//   matched losses   lib/loss.py:198-290 (F/lib/loss.py:272-541): QLoss (plain in f32, symmetric over the rotation table in
//                    f64, NaN pairs dropped before the mean), XY / Scales (sum over components of the mean), Z on log-depth
// The torch forms synchronise a dozen times per step (the IoU matrix on the CPU, one-argument torch.where, bool(isnan)) and
// issue ~1 100 aten calls on a few dozen pairs.  Three launches here, one workgroup each: the work is tens of pairs times
// 360 rotations, so latency decides, and one workgroup keeps every sum in a fixed order (two runs are bit-identical)
// without atomics on floating-point values or a second launch.  One wave per pair, the lanes sharing the rotations
// (k_pose_errors' shape, csrc/eval.hip).  Every division goes through div_ieee (common.hpp).
#include <limits.h>

#include "common.hpp"

namespace fpc {

constexpr int kMaxInst = FPC_MATCH_MAX_INSTANCES;
constexpr int kAssignThreads = 256, kLossThreads = 1024, kLossWaves = kLossThreads / kWave;

// grid 1, block 256: a wave per ground truth for the arg-max, then a thread per matched ground truth for its output rank
__global__ __launch_bounds__(kAssignThreads) void k_match_assign(const float* __restrict__ iou, const int64_t* __restrict__ gt_cls,
                                                                 const int64_t* __restrict__ pred_cls, int n1, int n2,
                                                                 int32_t* __restrict__ match_pred, int32_t* __restrict__ order,
                                                                 int32_t* __restrict__ count) {
    __shared__ int64_t s_cls[kMaxInst];
    __shared__ int s_match[kMaxInst];
    __shared__ int s_count;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    if (tid == 0) s_count = 0;
    for (int i = wave; i < n1; i += kAssignThreads / kWave) {
        const int64_t c = gt_cls[i];
        float best = 0.0f;
        int bj = -1;                    // -1: no candidate of this class yet
        bool bad = false;
        for (int j = lane; j < n2; j += kWave) {      // ascending j per lane: `>` keeps the lane's first maximum
            if (pred_cls[j] != c) continue;
            const float v = iou[(size_t)i * n2 + j];
            if (v != v) bad = true;
            else if (bj < 0 || v > best) { best = v; bj = j; }
        }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) {     // the largest value; among equals the smallest j (torch.max's first index)
            const float ob = __shfl_xor(best, o, kWave);
            const int oj = __shfl_xor(bj, o, kWave);
            if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj < bj))) { best = ob; bj = oj; }
        }
        const bool any_nan = __ballot(bad) != 0;      // a NaN among the candidates: the maximum is NaN, NaN > 0 is false
        const int m = (!any_nan && bj >= 0 && best > 0.0f) ? bj : -1;
        if (lane == 0) { s_match[i] = m; s_cls[i] = c; match_pred[i] = m; }
    }
    __syncthreads();
    for (int i = tid; i < n1; i += kAssignThreads) {
        if (s_match[i] < 0) continue;
        const int64_t c = s_cls[i];
        int rank = 0;
        for (int k = 0; k < n1; ++k) rank += (s_match[k] >= 0 && (s_cls[k] < c || (s_cls[k] == c && k < i))) ? 1 : 0;
        order[rank] = i;                // the ranks of the matched are a permutation of 0 .. count-1
        atomicAdd(&s_count, 1);
    }
    __syncthreads();
    const int cnt = s_count;
    for (int i = tid; i < n1; i += kAssignThreads)
        if (i >= cnt) order[i] = -1;
    if (tid == 0) *count = cnt;
}

struct MatchedArgs {
    const int32_t *order, *match_pred, *count;
    int n1, n2;
    const float *gq, *gxy, *gz, *gs;
    const int64_t* sym;
    const float *pq, *pxy, *pz, *ps;
    const float* rot;
    int nrot;
    double eps;
    int type[3];
    double w[4];
};

// nn.MSELoss / nn.L1Loss / nn.SmoothL1Loss(beta = 1) on d = input - target, per element, and d/dd of it
__device__ __forceinline__ float comp_loss(float d, int type) {
    const float a = fabsf(d);
    return type == FPC_LOSS_L2 ? d * d : type == FPC_LOSS_L1 ? a : (a < 1.0f ? 0.5f * d * d : a - 0.5f);
}
__device__ __forceinline__ float comp_dloss(float d, int type) {
    const float s = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    return type == FPC_LOSS_L2 ? 2.0f * d : type == FPC_LOSS_L1 ? s : (fabsf(d) < 1.0f ? d : s);
}

// quaternion_multiply(gt, rot_k) in f64: raw product over its norm, the norm rounded to f32 (gpu_tensor_funcs.normalize)
__device__ __forceinline__ void rotated_gt(const float* __restrict__ g, const float* __restrict__ r, double* o) {
    const double aw = (double)g[0], ax = (double)g[1], ay = (double)g[2], az = (double)g[3];
    const double rw = (double)r[0], rx = (double)r[1], ry = (double)r[2], rz = (double)r[3];
    o[0] = aw * rw - ax * rx - ay * ry - az * rz;
    o[1] = aw * rx + ax * rw + ay * rz - az * ry;
    o[2] = aw * ry - ax * rz + ay * rw + az * rx;
    o[3] = aw * rz + ax * ry - ay * rx + az * rw;
    const double nn = sqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2] + o[3] * o[3]);
    const double sn = nn != 0.0 ? (double)(float)nn : 1.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = div_ieee(o[e], sn);
}

// grid 1, block 1024.  Wave w takes the pairs order[w], order[w + 16], ...; its lanes 0-7 each keep one running sum
// (xy.x, xy.y, z, scales x 3, QLoss sum, QLoss pairs kept), folded over the waves in wave order at the end.
__global__ __launch_bounds__(kLossThreads) void k_matched_losses(MatchedArgs a, double* __restrict__ losses,
                                                                 double* __restrict__ task_total, double* __restrict__ matched_total,
                                                                 int32_t* __restrict__ best_rot) {
    __shared__ double s_part[kLossWaves][8];
    __shared__ double s_tot[8];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int cnt = min(max(*a.count, 0), a.n1);
    const float epsf = (float)a.eps;
    const float log_epsf = logf(epsf);                 // torch.log(torch.tensor(eps)): an f32 value in both branches
    for (int i = tid; i < a.n1; i += kLossThreads) {
        const int p = a.match_pred[i];
        if (p < 0 || p >= a.n2) best_rot[i] = -1;
    }
    double acc = 0.0;
    for (int t = wave; t < cnt; t += kLossWaves) {
        const int i = a.order[t];
        if (i < 0 || i >= a.n1) continue;              // (wave-uniform)
        const int p = a.match_pred[i];
        if (p < 0 || p >= a.n2) continue;
        float e = 0.0f;
        if (lane < 2) e = comp_loss(a.gxy[i * 2 + lane] - a.pxy[p * 2 + lane], a.type[0]);
        else if (lane == 2) e = comp_loss(logf(a.gz[i]) - logf(a.pz[p]), a.type[1]);
        else if (lane < 6) e = comp_loss(a.gs[i * 3 + lane - 3] - a.ps[p * 3 + lane - 3], a.type[2]);
        const float* g = a.gq + (size_t)i * 4;
        const float b0 = a.pq[p * 4], b1 = a.pq[p * 4 + 1], b2 = a.pq[p * 4 + 2], b3 = a.pq[p * 4 + 3];
        double ql;
        int br;
        if (a.sym[i] == 0) {
            const float dot = g[0] * b0 + g[1] * b1 + g[2] * b2 + g[3] * b3;
            const float v = logf((1.0f - dot * dot) + epsf) - log_epsf;
            ql = (double)v;
            br = v != v ? -1 : 0;
        } else {
            double best = __builtin_inf();
            int bk = INT_MAX;
            bool bad = false;
            for (int k = lane; k < a.nrot; k += kWave) {
                double r[4];
                rotated_gt(g, a.rot + (size_t)k * 4, r);
                const double dot = (double)b0 * r[0] + (double)b1 * r[1] + (double)b2 * r[2] + (double)b3 * r[3];
                const double v = log((1.0 - dot * dot) + a.eps) - (double)log_epsf;
                if (v != v) bad = true;
                else if (v < best) { best = v; bk = k; }
            }
#pragma unroll
            for (int o = kWave / 2; o > 0; o >>= 1) {  // the smallest loss; among equals the smallest k (torch.min's first index)
                const double ob = __shfl_xor(best, o, kWave);
                const int ok = __shfl_xor(bk, o, kWave);
                if (ob < best || (ob == best && ok < bk)) { best = ob; bk = ok; }
            }
            const bool dropped = __ballot(bad) != 0 || bk == INT_MAX;      // a NaN among the rotations: torch.min gives NaN
            ql = best;
            br = dropped ? -1 : bk;
        }
        if (lane < 6) acc += (double)e;                // no NaN filter: one NaN makes the loss NaN
        else if (lane == 6) acc += br >= 0 ? ql : 0.0;
        else if (lane == 7) acc += br >= 0 ? 1.0 : 0.0;
        if (lane == 0) best_rot[i] = br;
    }
    if (lane < 8) s_part[wave][lane] = acc;
    __syncthreads();
    if (tid < 8) {
        double s = 0.0;
        for (int w = 0; w < kLossWaves; ++w) s += s_part[w][tid];
        s_tot[tid] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const double qnan = nan("");
        const double n = (double)cnt;
        double L[4] = {qnan, qnan, qnan, qnan};
        if (cnt > 0) {
            if (s_tot[7] > 0.0) L[0] = div_ieee(s_tot[6], s_tot[7]);
            L[1] = div_ieee(s_tot[0], n) + div_ieee(s_tot[1], n);
            L[2] = div_ieee(s_tot[2], n);
            L[3] = div_ieee(s_tot[3], n) + div_ieee(s_tot[4], n) + div_ieee(s_tot[5], n);
        }
        double total = 0.0;
        for (int k = 0; k < 4; ++k) {
            const bool is_nan = L[k] != L[k];
            const double tt = is_nan ? qnan : a.w[k] * L[k];
            losses[k] = L[k];
            task_total[k] = tt;
            if (!is_nan) total += tt;
        }
        matched_total[0] = total;
    }
}

// grid 1, block 1024: a thread per PREDICTION walks the matched pairs in `order` order and sums the terms of its own row,
// so a prediction matched by several ground truths gets their sum in a fixed order and no atomics are needed.
__global__ __launch_bounds__(kLossThreads) void k_matched_losses_bwd(MatchedArgs a, const double* __restrict__ losses,
                                                                     const int32_t* __restrict__ best_rot, const double* __restrict__ g,
                                                                     float* __restrict__ g_q, float* __restrict__ g_xy,
                                                                     float* __restrict__ g_z, float* __restrict__ g_s) {
    __shared__ int s_i[kMaxInst], s_p[kMaxInst];
    __shared__ int s_kept;
    const int tid = threadIdx.x;
    const int cnt = min(max(*a.count, 0), a.n1);
    if (tid == 0) s_kept = 0;
    __syncthreads();
    for (int t = tid; t < cnt; t += kLossThreads) {
        const int i = a.order[t];
        int p = -1, br = -1;
        if (i >= 0 && i < a.n1) {
            p = a.match_pred[i];
            if (p < 0 || p >= a.n2) p = -1;
            br = best_rot[i];
            if (br >= a.nrot) br = -1;
        }
        s_i[t] = i;
        s_p[t] = p;
        if (p >= 0 && br >= 0) atomicAdd(&s_kept, 1);
    }
    __syncthreads();
    // a loss that was NaN in the forward contributes nothing: its terms are skipped, not multiplied by zero
    const bool on_q = losses[0] == losses[0] && s_kept > 0, on_xy = losses[1] == losses[1], on_z = losses[2] == losses[2],
               on_s = losses[3] == losses[3];
    const double n = (double)cnt;
    const double cq = on_q ? div_ieee(g[0], (double)s_kept) : 0.0, cxy = on_xy ? div_ieee(g[1], n) : 0.0,
                 cz = on_z ? div_ieee(g[2], n) : 0.0, cs = on_s ? div_ieee(g[3], n) : 0.0;
    const double eps_plain = (double)(float)a.eps;
    for (int j = tid; j < a.n2; j += kLossThreads) {
        double aq[4] = {0.0, 0.0, 0.0, 0.0}, axy[2] = {0.0, 0.0}, az = 0.0, asc[3] = {0.0, 0.0, 0.0};
        for (int t = 0; t < cnt; ++t) {
            if (s_p[t] != j) continue;
            const int i = s_i[t];
            const int br = best_rot[i];
            if (on_q && br >= 0 && br < a.nrot) {      // a pair dropped as NaN in the forward has br = -1
                const float* gt = a.gq + (size_t)i * 4;
                const float* pr = a.pq + (size_t)j * 4;
                double r[4], dot, e;
                if (a.sym[i] == 0) {
                    r[0] = (double)gt[0]; r[1] = (double)gt[1]; r[2] = (double)gt[2]; r[3] = (double)gt[3];
                    dot = (double)(gt[0] * pr[0] + gt[1] * pr[1] + gt[2] * pr[2] + gt[3] * pr[3]);
                    e = eps_plain;
                } else {
                    rotated_gt(gt, a.rot + (size_t)br * 4, r);
                    dot = (double)pr[0] * r[0] + (double)pr[1] * r[1] + (double)pr[2] * r[2] + (double)pr[3] * r[3];
                    e = a.eps;
                }
                const double f = cq * div_ieee(-2.0 * dot, (1.0 - dot * dot) + e);       // d/d dot of log(1 - dot^2 + eps)
#pragma unroll
                for (int c = 0; c < 4; ++c) aq[c] += f * r[c];
            }
            if (on_xy) {
#pragma unroll
                for (int c = 0; c < 2; ++c) axy[c] -= cxy * (double)comp_dloss(a.gxy[i * 2 + c] - a.pxy[j * 2 + c], a.type[0]);
            }
            if (on_z) {
                const float pz = a.pz[j];
                az -= cz * div_ieee((double)comp_dloss(logf(a.gz[i]) - logf(pz), a.type[1]), (double)pz);
            }
            if (on_s) {
#pragma unroll
                for (int c = 0; c < 3; ++c) asc[c] -= cs * (double)comp_dloss(a.gs[i * 3 + c] - a.ps[j * 3 + c], a.type[2]);
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) g_q[(size_t)j * 4 + c] = (float)aq[c];
        g_xy[j * 2] = (float)axy[0];
        g_xy[j * 2 + 1] = (float)axy[1];
        g_z[j] = (float)az;
#pragma unroll
        for (int c = 0; c < 3; ++c) g_s[j * 3 + c] = (float)asc[c];
    }
}

static bool matched_args(MatchedArgs& a, const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                         const float* gt_quaternion, const float* gt_xy, const float* gt_z, const float* gt_scales,
                         const int64_t* symmetric_ids, const float* quaternion, const float* xy, const float* z, const float* scales,
                         const float* rot, int nrot, double eps, int xy_type, int z_type, int scales_type, const double* weights) {
    if (!order || !match_pred || !count || !gt_quaternion || !gt_xy || !gt_z || !gt_scales || !symmetric_ids || !rot || nrot < 1 ||
        !weights)
        return false;
    if (n2 > 0 && (!quaternion || !xy || !z || !scales)) return false;
    for (int t : {xy_type, z_type, scales_type})
        if (t != FPC_LOSS_L2 && t != FPC_LOSS_L1 && t != FPC_LOSS_SMOOTH_L1) return false;
    a = MatchedArgs{order, match_pred, count, n1, n2, gt_quaternion, gt_xy, gt_z, gt_scales, symmetric_ids, quaternion, xy, z, scales,
                    rot, nrot, eps, {xy_type, z_type, scales_type}, {weights[0], weights[1], weights[2], weights[3]}};
    return true;
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_match_assign(const float* iou, const int64_t* gt_cls, const int64_t* pred_cls, int n1, int n2,
                                int32_t* match_pred, int32_t* order, int32_t* count, fpc_stream_t stream) {
    if (n1 < 0 || n2 < 0 || n1 > kMaxInst || n2 > kMaxInst) return FPC_EINVAL;
    if (n1 == 0) return FPC_OK;
    if (!gt_cls || !match_pred || !order || !count || (n2 > 0 && (!iou || !pred_cls))) return FPC_EINVAL;
    hipLaunchKernelGGL(k_match_assign, dim3(1), dim3(kAssignThreads), 0, (hipStream_t)stream, iou, gt_cls, pred_cls, n1, n2,
                       match_pred, order, count);
    return check_launch();
}

extern "C" int fpc_matched_losses(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                                  const float* gt_quaternion, const float* gt_xy, const float* gt_z, const float* gt_scales,
                                  const int64_t* symmetric_ids, const float* quaternion, const float* xy, const float* z,
                                  const float* scales, const float* rot, int nrot, double eps, int xy_type, int z_type,
                                  int scales_type, const double* weights, double* losses, double* task_total,
                                  double* matched_total, int32_t* best_rot, fpc_stream_t stream) {
    if (n1 < 0 || n2 < 0 || n1 > kMaxInst || n2 > kMaxInst) return FPC_EINVAL;
    if (n1 == 0) return FPC_OK;
    MatchedArgs a;
    if (!losses || !task_total || !matched_total || !best_rot ||
        !matched_args(a, order, match_pred, count, n1, n2, gt_quaternion, gt_xy, gt_z, gt_scales, symmetric_ids, quaternion, xy, z,
                      scales, rot, nrot, eps, xy_type, z_type, scales_type, weights))
        return FPC_EINVAL;
    hipLaunchKernelGGL(k_matched_losses, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, a, losses, task_total, matched_total,
                       best_rot);
    return check_launch();
}

extern "C" int fpc_matched_losses_backward(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                                           const float* gt_quaternion, const float* gt_xy, const float* gt_z,
                                           const float* gt_scales, const int64_t* symmetric_ids, const float* quaternion,
                                           const float* xy, const float* z, const float* scales, const float* rot, int nrot,
                                           double eps, int xy_type, int z_type, int scales_type, const double* weights,
                                           const double* losses, const int32_t* best_rot, const double* g_losses,
                                           float* g_quaternion, float* g_xy, float* g_z, float* g_scales, fpc_stream_t stream) {
    if (n1 < 0 || n2 < 0 || n1 > kMaxInst || n2 > kMaxInst) return FPC_EINVAL;
    if (n1 == 0 || n2 == 0) return FPC_OK;
    MatchedArgs a;
    if (!losses || !best_rot || !g_losses || !g_quaternion || !g_xy || !g_z || !g_scales ||
        !matched_args(a, order, match_pred, count, n1, n2, gt_quaternion, gt_xy, gt_z, gt_scales, symmetric_ids, quaternion, xy, z,
                      scales, rot, nrot, eps, xy_type, z_type, scales_type, weights))
        return FPC_EINVAL;
    hipLaunchKernelGGL(k_matched_losses_bwd, dim3(1), dim3(kLossThreads), 0, (hipStream_t)stream, a, losses, best_rot, g_losses,
                       g_quaternion, g_xy, g_z, g_scales);
    return check_launch();
}
