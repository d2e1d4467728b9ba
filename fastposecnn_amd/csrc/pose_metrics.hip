// pose_metrics.hip — the pose metrics of the evaluate / validate loop folded into a persistent device state, one launch per
// matched batch and nothing read back:
//   accumulators     F/lib/metrics.py:11-260 (DegreeErrorMeanAP, DegreeError, Iou3dAP, Iou3dAccuracy, OffsetAP, OffsetError)
//   AP curves        F/lib/gpu_tensor_funcs.py:611-713 (calculate_aps, calculate_complex_aps) over evaluate.py:238-292's
//                    per-class raw errors: kept as integer counts per class and threshold, so no match has to be stored
// The host route synchronises to learn the number of pairs, then runs fpc_pose_errors three to six times on the same pairs
// with gathers around each.  Here one workgroup reads order / match_pred / count where fpc_match_assign left them; a wave
// per pair takes the three errors through the device functions k_pose_errors uses (pose_errors.hpp), its lanes then share
// the thresholds.  Counts are i64 and added with integer atomics (any order gives the same sum); the three floating-point
// sums behind the running means are taken by one thread each over the pairs in `order` order, so two runs on the same
// input leave the same bits.  count == 0 returns before the first store.  State layout: include/fpc.h.
#include "pose_errors.hpp"

namespace fpc {

constexpr int kPmMaxInst = FPC_MATCH_MAX_INSTANCES;
constexpr int kPmThreads = 512, kPmWaves = kPmThreads / kWave;
constexpr int kPmHeader = 16, kPmMaxClasses = 4096, kPmMaxThresholds = 4096;

struct PoseMetricsArgs {
    const int32_t *order, *match_pred, *count;
    int n1, n2;
    const float *gq, *gRT, *gs, *gT;
    const int64_t *sym, *cls;
    const float *pq, *pRT, *ps, *pT;
    const float* rot;
    int nrot;
    const double *thr_deg, *thr_iou, *thr_off, *thr_cx, *thr_table;
    int n_deg, n_iou, n_off, n_cx, C;
    unsigned long long* state;
    double* raw_deg;
    float *raw_iou, *raw_off;
    int32_t* raw_cls;
    int raw_cap;
};

__device__ __forceinline__ void count_one(unsigned long long* w) { atomicAdd(w, 1ull); }

// grid 1, block 512 (8 waves: 256 registers a lane for the two f64 4x4 inverses).  Wave w takes the pairs order[w], order[w + 8], ...
__global__ __launch_bounds__(kPmThreads) void k_pose_metrics(PoseMetricsArgs a) {
    __shared__ double s_deg[kPmMaxInst], s_sq[kPmMaxInst];
    __shared__ float s_iou[kPmMaxInst];
    __shared__ double s_tot[4];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int cnt = min(max(*a.count, 0), min(a.n1, kPmMaxInst));
    if (cnt == 0) return;                               // nothing matched: not one word of the state changes
    unsigned long long* st = a.state;
    const long long cursor = (long long)st[2];          // read by everyone before thread 0 rewrites it behind two barriers
    const int nthr = a.n_deg + a.n_iou + a.n_off;
    const double qnan = nan("");
    for (int t = wave; t < cnt; t += kPmWaves) {
        const int i = a.order[t];
        int p = -1;
        if (i >= 0 && i < a.n1) p = a.match_pred[i];
        const bool pair_ok = p >= 0 && p < a.n2;       // (wave-uniform) fpc_match_assign never leaves anything else below count
        double deg = qnan, sq = qnan;
        float iou = nanf(""), off = nanf("");
        long long c = 0;
        if (pair_ok) {
            c = a.cls[i];
            deg = pair_degree_error(a.gq + (size_t)i * 4, a.pq + (size_t)p * 4, a.sym[i] != 0, a.rot, a.nrot, lane);
            off = pair_offset_error(a.gT + (size_t)i * 3, a.pT + (size_t)p * 3);
            iou = __shfl(pair_iou3d(a.gRT + (size_t)i * 16, a.pRT + (size_t)p * 16, a.gs + (size_t)i * 3, a.ps + (size_t)p * 3, lane),
                         0, kWave);
            // from_RTs_get_T_offset_errors: the camera origin under inverse(RT) is the inverse's last column over its corner
            // element; even lanes the ground truth, odd lanes the prediction, each coordinate rounded to f32 as the host holds it
            double inv[16];
            const bool ok = inverse4((lane & 1) ? a.pRT + (size_t)p * 16 : a.gRT + (size_t)i * 16, inv);
            const float wx = ok ? (float)div_ieee(inv[3], inv[15]) : nanf("");
            const float wy = ok ? (float)div_ieee(inv[7], inv[15]) : nanf("");
            const float wz = ok ? (float)div_ieee(inv[11], inv[15]) : nanf("");
            const float dx = wx - __shfl_xor(wx, 1, kWave), dy = wy - __shfl_xor(wy, 1, kWave), dz = wz - __shfl_xor(wz, 1, kWave);
            sq = (double)(dx * dx) + (double)(dy * dy) + (double)(dz * dz);
        }
        const bool in_class = pair_ok && c >= 1 && c < (long long)a.C;
        if (in_class) {
            const size_t ci = (size_t)c;
            if (lane < 3) {
                const bool is_nan = lane == 0 ? deg != deg : (lane == 1 ? iou != iou : off != off);
                count_one(st + kPmHeader + 6 * ci + 2 * lane + (is_nan ? 1 : 0));
            }
            unsigned long long* hits = st + kPmHeader + 6 * (size_t)a.C + ci * nthr;
            for (int j = lane; j < nthr; j += kWave) {
                bool hit;
                if (j < a.n_deg) hit = deg < a.thr_deg[j];
                else if (j < a.n_deg + a.n_iou) hit = (double)iou > a.thr_iou[j - a.n_deg];
                else hit = (double)off < a.thr_off[j - a.n_deg - a.n_iou];
                if (hit) count_one(hits + j);
            }
            unsigned long long* cx = st + kPmHeader + (6 + (size_t)nthr) * a.C + ci * a.n_cx;
            for (int k = lane; k < a.n_cx; k += kWave)
                if (deg < a.thr_cx[k] && (double)off < a.thr_cx[a.n_cx + k]) count_one(cx + k);
        } else if (lane == 0) {
            count_one(st + 1);
        }
        if (lane == 0) {
            if (deg < a.thr_table[0]) count_one(st + 4);
            if ((double)iou > a.thr_table[1]) count_one(st + 6);
            if ((double)off < a.thr_table[2]) count_one(st + 8);
            s_deg[t] = deg;
            s_iou[t] = iou;
            s_sq[t] = sq;
            const long long slot = cursor + t;
            if (slot >= 0 && slot < (long long)a.raw_cap) {
                a.raw_deg[slot] = deg;
                a.raw_iou[slot] = iou;
                a.raw_off[slot] = off;
                a.raw_cls[slot] = (int32_t)c;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {                                     // DegreeError: the non-NaN distances
        double s = 0.0, n = 0.0;
        for (int t = 0; t < cnt; ++t) {
            const double v = s_deg[t];
            if (v == v) { s += v; n += 1.0; }
        }
        s_tot[0] = s;
        s_tot[1] = n;
    } else if (tid == kWave) {                          // Iou3dAccuracy: iou * 100 in f32, NaN propagates
        double s = 0.0;
        for (int t = 0; t < cnt; ++t) s += (double)(s_iou[t] * 100.0f);
        s_tot[2] = s;
    } else if (tid == 2 * kWave) {                      // OffsetError: one distance over every pair and coordinate
        double s = 0.0;
        for (int t = 0; t < cnt; ++t) s += s_sq[t];
        s_tot[3] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const long long cap = a.raw_cap, end = cursor + cnt;
        const long long logged = max(0ll, min(cap, end) - min(cap, max(cursor, 0ll)));
        st[0] += 1ull;
        st[2] = (unsigned long long)end;
        if (cap > 0) st[3] += (unsigned long long)(cnt - logged);
        st[5] += (unsigned long long)s_tot[1];
        st[7] += (unsigned long long)cnt;
        st[9] += (unsigned long long)cnt;
        double* fw = reinterpret_cast<double*>(st);
        fw[10] = (fw[10] + div_ieee(s_tot[0], s_tot[1])) * 0.5;
        fw[11] = (fw[11] + div_ieee(s_tot[2], (double)cnt)) * 0.5;
        fw[12] = (fw[12] + sqrt(s_tot[3]) * 10.0) * 0.5;
    }
}

}  // namespace fpc

using namespace fpc;

extern "C" size_t fpc_pose_metrics_state_words(int num_classes, int n_deg, int n_iou, int n_off, int n_complex) {
    if (num_classes < 2 || num_classes > kPmMaxClasses || n_deg < 0 || n_iou < 0 || n_off < 0 || n_complex < 0 ||
        (long long)n_deg + n_iou + n_off + n_complex > kPmMaxThresholds)
        return 0;
    return (size_t)kPmHeader + (size_t)num_classes * (6 + (size_t)n_deg + n_iou + n_off + n_complex);
}

extern "C" int fpc_pose_metrics_update(const int32_t* order, const int32_t* match_pred, const int32_t* count, int n1, int n2,
                                       const float* gt_quaternion, const float* gt_RT, const float* gt_scales, const float* gt_T,
                                       const int64_t* symmetric_ids, const int64_t* class_ids, const float* quaternion,
                                       const float* RT, const float* scales, const float* T, const float* rot, int nrot,
                                       const double* thr_degree, int n_deg, const double* thr_iou, int n_iou,
                                       const double* thr_offset, int n_off, const double* thr_complex, int n_complex,
                                       const double* thr_table, int num_classes, int64_t* state, double* raw_degree,
                                       float* raw_iou, float* raw_offset, int32_t* raw_class, int raw_capacity,
                                       fpc_stream_t stream) {
    if (n1 < 0 || n2 < 0 || n1 > kPmMaxInst || n2 > kPmMaxInst) return FPC_EINVAL;
    if (fpc_pose_metrics_state_words(num_classes, n_deg, n_iou, n_off, n_complex) == 0 || raw_capacity < 0) return FPC_EINVAL;
    if (n1 == 0 || n2 == 0) return FPC_OK;
    if (!order || !match_pred || !count || !gt_quaternion || !gt_RT || !gt_scales || !gt_T || !symmetric_ids || !class_ids ||
        !quaternion || !RT || !scales || !T || !rot || nrot < 1 || !thr_table || !state)
        return FPC_EINVAL;
    if ((n_deg > 0 && !thr_degree) || (n_iou > 0 && !thr_iou) || (n_off > 0 && !thr_offset) || (n_complex > 0 && !thr_complex))
        return FPC_EINVAL;
    if (raw_capacity > 0 && (!raw_degree || !raw_iou || !raw_offset || !raw_class)) return FPC_EINVAL;
    PoseMetricsArgs a{order, match_pred, count, n1, n2, gt_quaternion, gt_RT, gt_scales, gt_T, symmetric_ids, class_ids,
                      quaternion, RT, scales, T, rot, nrot, thr_degree, thr_iou, thr_offset, thr_complex, thr_table,
                      n_deg, n_iou, n_off, n_complex, num_classes, reinterpret_cast<unsigned long long*>(state),
                      raw_degree, raw_iou, raw_offset, raw_class, raw_capacity};
    hipLaunchKernelGGL(k_pose_metrics, dim3(1), dim3(kPmThreads), 0, (hipStream_t)stream, a);
    return check_launch();
}
