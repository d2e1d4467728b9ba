// mobilenet.hip — the stem and the 1x1 kernels of the MobileNetV2 encoder (torchvision's, as smp wraps it: lib/backbone.py
// MobileNetV2Encoder), for inference; its depthwise 3x3 is depthwise.hip's k_dw_fwd<3, S, 1, false>.  Activations are dense
// channel-last f32; BatchNorm arrives folded as per-channel scale / shift; act 1 is ReLU6, min(max(v, 0), 6).  No atomics and no split over K: every sum runs in an order the shape alone fixes, so two launches agree bit
// for bit.  No kernel divides a float.  Workgroups walk their items in the XCD-banded order of the other streaming kernels
// (conv_device.hpp: xcd_walk), so neighbouring rows are fetched by one L2.
//
//   k_stem3x3s2    features.0: dense 3x3 / stride 2 / pad 1 over the NHWC4 image to 32 channels.  Eight threads per output pixel, each
//                  with the 4 x 27 weights of its channel quad in registers for the whole launch; the nine 16-byte pixels of a window
//                  are the same addresses for those eight lanes (one fetch).  27 FMAs per channel in (kh, kw, ci) order.
//   k_conv1x1_f32<NT>  the 1x1 sites as out[m][n] = act(scale[n] sum_k in[m][k] w[n][k] + shift[n]) (+ res[m][n]) on
//                  v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation).  One wave per (32 pixel rows, NT tiles of 32
//                  output channels), both operands straight from memory in the instruction's own lane layout (lane l: row l & 31,
//                  k = k0 + 4 (l >> 5) + e for e = 0..3: one 16-byte load feeds four instructions), the next iteration's loads (up to
//                  four K-steps of 8) in flight under the current one's MFMAs.  No LDS, no barrier.  The waves that share a pixel-row tile are neighbours
//                  in one workgroup or in the next one of the same XCD band, so a pixel row of a wide-Cin site comes from memory
//                  once and from L1 / L2 for the other channel chunks; NT (conv1x1_f32_tiles) is the most channel tiles per wave
//                  that still leaves the chip two waves per SIMD and wastes no tile.  The sum over k runs in ascending K-steps whatever NT is.
//   k_conv1x1_f32_small  the same product on 16 x 16 tiles (v_mfma_f32_16x16x4_f32) for the sites with too few pixel rows to fill
//                  the chip with 32 x 32 tiles: see the kernel.
// The stem and the two 1x1 kernels carry a template parameter MB.  Its true instantiations are the EfficientNet encoder's
// (efficientnet.hip holds that encoder's other kernels and the entries): the stem's window starts at (2 ho, 2 wo) and ends in swish;
// the 1x1 kernels know act 2 = swish and multiply a per-frame, per-channel gate into the in operand.  MB = false compiles to what
// these kernels were before the parameter: no gate pointer is read, the activation is the two-way select.
#include <initializer_list>

#include "conv_device.hpp"

namespace fpc {

namespace {

__device__ __forceinline__ float act_apply(float v, int act) { return act ? fminf(fmaxf(v, 0.f), 6.f) : v; }
// ... and with code 2, swish v / (1 + exp(-v)): the EfficientNet instantiations (MB) alone, so the others keep their two-way select
template <bool MB>
__device__ __forceinline__ float act_apply(float v, int act) {
    if constexpr (MB) return act == 2 ? swish(v) : act_apply(v, act);
    else return act_apply(v, act);
}

}  // namespace

// in4 [B][Hi][Wi][4] (the fourth channel is not read), w [32][3][3][3], out [B][Ho][Wo][32]; npix = B Ho Wo.  MB: EfficientNet's stem,
// the same sum with the window starting at (2 ho, 2 wo) (pads 0 before and 1 after) and swish in place of ReLU6
template <bool MB>
__global__ __launch_bounds__(256) void k_stem3x3s2(const float* __restrict__ in4, const float* __restrict__ w,
                                                   const float* __restrict__ scale, const float* __restrict__ shift,
                                                   float* __restrict__ out, unsigned npix, int Hi, int Wi, int Ho, int Wo) {
    const unsigned q = threadIdx.x & 7, pl = threadIdx.x >> 3;
    float wr[108];      // channels 4 q .. 4 q + 3: [channel][ci][kh][kw]
#pragma unroll
    for (int i = 0; i < 27; ++i) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + 108 * q + 4 * i);
        wr[4 * i] = v[0]; wr[4 * i + 1] = v[1]; wr[4 * i + 2] = v[2]; wr[4 * i + 3] = v[3];
    }
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * q), sh = *reinterpret_cast<const f32x4*>(shift + 4 * q);
    const XcdSpan wk = xcd_rows(npix, 32u, pl);
    for (unsigned p = wk.first; p < wk.end; p += wk.step) {
        const unsigned wo = p % (unsigned)Wo, t = p / (unsigned)Wo, ho = t % (unsigned)Ho, b = t / (unsigned)Ho;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int hi = 2 * (int)ho - (MB ? 0 : 1) + kh;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int wi = 2 * (int)wo - (MB ? 0 : 1) + kw;
                f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
                if (hi >= 0 && hi < Hi && wi >= 0 && wi < Wi) x = *reinterpret_cast<const f32x4*>(in4 + (((size_t)b * Hi + hi) * Wi + wi) * 4);
#pragma unroll
                for (int ci = 0; ci < 3; ++ci)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(x[ci], wr[27 * j + 9 * ci + 3 * kh + kw], acc[j]);
            }
        }
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = act_apply<MB>(acc[j] * sc[j] + sh[j], MB ? 2 : 1);
        *reinterpret_cast<f32x4*>(out + (size_t)p * 32 + 4 * q) = o;
    }
}

// in [M][Cin], w [Cout][Cin], out / res [M][Cout]; waves = mtiles * nchunks, the chunk index fastest.  U K-steps of 8 per loop
// iteration: their loads are issued together, one iteration ahead of the MFMAs that read them; the K-steps past the last full
// iteration (fewer than U) load together behind the loop.  Ascending K-steps whatever NT and U are.
// MB (the EfficientNet 1x1 sites): act 2 is swish, and where `gate` [M / HW][Cin] is not NULL the in operand is in[m][k] gate[m / HW][k],
// rounded to f32 before it enters the matrix instruction; the frame m / HW is a lane's own (a tile may straddle frames).  The
// instantiations without MB never read gate and HW.
template <int NT, int U, bool MB>
__global__ __launch_bounds__(256) void k_conv1x1_f32(const float* __restrict__ in, const float* __restrict__ w,
                                                     const float* __restrict__ scale, const float* __restrict__ shift,
                                                     const float* __restrict__ res, float* __restrict__ out, unsigned M, int Cin, int Cout,
                                                     int act, unsigned mtiles, unsigned nchunks, const float* __restrict__ gate, unsigned HW) {
    const unsigned lane = threadIdx.x & 63, li = lane & 31, lh = lane >> 5;
    const unsigned wid = xcd_block() * 4 + (threadIdx.x >> 6);      // the chunk index fastest: a pixel-row tile's chunks share an L2
    if (wid >= mtiles * nchunks) return;      // (no barrier in this kernel)
    const unsigned chunk = wid % nchunks, mt = wid / nchunks;
    const unsigned m0 = mt * 32, n0 = chunk * (NT * 32);
    // rows past M and channels past Cout load the last valid row instead; their results are never written
    const float* pa = in + (size_t)min(m0 + li, M - 1) * Cin + 4 * lh;
    const float* pg = nullptr;
    if constexpr (MB) pg = gate ? gate + (size_t)(min(m0 + li, M - 1) / HW) * Cin + 4 * lh : nullptr;
    const float* pb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) pb[t] = w + (size_t)min(n0 + 32 * t + li, (unsigned)Cout - 1) * Cin + 4 * lh;
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    constexpr int KU = 8 * U;
    const int iters = Cin / KU, kmain = iters * KU;
    // two operand sets taken in turn: while the MFMAs read one, the other's loads are in flight.  The scheduling barriers keep
    // the compiler from sinking a set's loads in front of the MFMAs that read it (it then waits for them inside the same iteration)
    f32x4 a[U], bq[NT][U], a1[U], bq1[NT][U];
    auto load_set = [&](f32x4 (&A)[U], f32x4 (&Bq)[NT][U], int k) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            A[j] = *reinterpret_cast<const f32x4*>(pa + k + 8 * j);
            if constexpr (MB) { if (pg) A[j] = A[j] * *reinterpret_cast<const f32x4*>(pg + k + 8 * j); }
#pragma unroll
            for (int t = 0; t < NT; ++t) Bq[t][j] = *reinterpret_cast<const f32x4*>(pb[t] + k + 8 * j);
        }
    };
    auto mma_set = [&](const f32x4 (&A)[U], const f32x4 (&Bq)[NT][U]) {
#pragma unroll
        for (int j = 0; j < U; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[j][e], Bq[t][j][e], acc[t], 0, 0, 0);
    };
    if (iters) load_set(a, bq, 0);
    int it = 0;
    for (; it + 2 <= iters; it += 2) {
        load_set(a1, bq1, (it + 1) * KU);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(a, bq);
        __builtin_amdgcn_sched_barrier(0);
        load_set(a, bq, (it + 2 < iters ? it + 2 : it + 1) * KU);      // (behind the last pair: a set nobody reads)
        __builtin_amdgcn_sched_barrier(0);
        mma_set(a1, bq1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (it < iters) mma_set(a, bq);      // an odd count: the last set
    if (U > 1) {      // the K-steps behind the last full iteration (uniform over the launch)
        const int ntail = (Cin - kmain) >> 3;
#pragma unroll
        for (int j = 0; j < U - 1; ++j)
            if (j < ntail) {
                a[j] = *reinterpret_cast<const f32x4*>(pa + kmain + 8 * j);
                if constexpr (MB) { if (pg) a[j] = a[j] * *reinterpret_cast<const f32x4*>(pg + kmain + 8 * j); }
#pragma unroll
                for (int t = 0; t < NT; ++t) bq[t][j] = *reinterpret_cast<const f32x4*>(pb[t] + kmain + 8 * j);
            }
#pragma unroll
        for (int j = 0; j < U - 1; ++j)
            if (j < ntail) {
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j][e], bq[t][j][e], acc[t], 0, 0, 0);
            }
    }
    // C/D layout: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).  The residual's 16 loads of a tile go out
    // together (a row past M reads the last valid one); only the stores are conditional
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const unsigned nn = n0 + 32 * t + li;
        if (nn >= (unsigned)Cout) continue;
        const float sc = scale[nn], sh = shift[nn];
        float rv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rv[r] = 0.f;
        if (res) {
#pragma unroll
            for (int r = 0; r < 16; ++r) rv[r] = res[(size_t)min(m0 + (r & 3) + 8 * (r >> 2) + 4 * lh, M - 1) * Cout + nn];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const unsigned m = m0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const float v = act_apply<MB>(acc[t][r] * sc + sh, act) + rv[r];
            if (m < M) out[(size_t)m * Cout + nn] = v;
        }
    }
}

// The same product for a site with few pixel rows (deep maps of one frame: M = 300 at 15 x 20), where 32 x 32 tiles leave most of the
// chip idle behind a serial chain of Cin / 2 MFMAs: one wave per 16 rows x 16 channels on v_mfma_f32_16x16x4_f32 (a quarter of the
// chain, four times the waves).  Lane l holds row / channel l & 15 and the K quad g = l >> 4 of a K-step of 16: one 16-byte load
// feeds four instructions, instruction e sums k0 + 4 g + e over g.  Four K-steps per operand set, two sets in turn as above; two
// accumulators take the K-steps in turn (the instruction's dependent latency is longer than its issue interval) and are added at
// the end: an order the shape alone fixes.  Where Cin is not a multiple of 16 the last K-step is half one: the lanes of g >= 2 read
// eight floats earlier (inside their row) and contribute zeros.  MB: as k_conv1x1_f32's.
template <bool MB>
__global__ __launch_bounds__(256) void k_conv1x1_f32_small(const float* __restrict__ in, const float* __restrict__ w,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           const float* __restrict__ res, float* __restrict__ out, unsigned M, int Cin,
                                                           int Cout, int act, unsigned mtiles, unsigned ntiles,
                                                           const float* __restrict__ gate, unsigned HW) {
    const unsigned lane = threadIdx.x & 63, li = lane & 15, g = lane >> 4;
    const unsigned wid = xcd_block() * 4 + (threadIdx.x >> 6);
    if (wid >= mtiles * ntiles) return;      // (no barrier in this kernel)
    const unsigned nt = wid % ntiles, mt = wid / ntiles;
    const unsigned m0 = mt * 16, n0 = nt * 16;
    const float* pa = in + (size_t)min(m0 + li, M - 1) * Cin + 4 * g;
    const float* pg = nullptr;
    if constexpr (MB) pg = gate ? gate + (size_t)(min(m0 + li, M - 1) / HW) * Cin + 4 * g : nullptr;
    const float* pb = w + (size_t)min(n0 + li, (unsigned)Cout - 1) * Cin + 4 * g;
    constexpr int U = 4, KU = 16 * U;
    const int iters = Cin / KU, kmain = iters * KU;
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 a[U], b[U], a1[U], b1[U];
    auto load_set = [&](f32x4 (&A)[U], f32x4 (&Bq)[U], int k) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
            A[j] = *reinterpret_cast<const f32x4*>(pa + k + 16 * j); Bq[j] = *reinterpret_cast<const f32x4*>(pb + k + 16 * j);
            if constexpr (MB) { if (pg) A[j] = A[j] * *reinterpret_cast<const f32x4*>(pg + k + 16 * j); }
        }
    };
    auto mma_set = [&](const f32x4 (&A)[U], const f32x4 (&Bq)[U]) {
#pragma unroll
        for (int j = 0; j < U; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[j][e], Bq[j][e], acc[j & 1], 0, 0, 0);
    };
    if (iters) load_set(a, b, 0);
    int it = 0;
    for (; it + 2 <= iters; it += 2) {
        load_set(a1, b1, (it + 1) * KU);
        __builtin_amdgcn_sched_barrier(0);
        mma_set(a, b);
        __builtin_amdgcn_sched_barrier(0);
        load_set(a, b, (it + 2 < iters ? it + 2 : it + 1) * KU);      // (behind the last pair: a set nobody reads)
        __builtin_amdgcn_sched_barrier(0);
        mma_set(a1, b1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (it < iters) mma_set(a, b);
    {   // the K-steps behind the last full set: up to three whole ones and a half one, loaded together (uniform over the launch)
        const int rest = Cin - kmain, whole = rest >> 4, half = (rest >> 3) & 1;
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (j < whole + half) {
                const int back = (j == whole && g >= 2) ? 8 : 0;      // the half step's upper lanes stay inside the row
                a[j] = *reinterpret_cast<const f32x4*>(pa + kmain + 16 * j - back);
                b[j] = *reinterpret_cast<const f32x4*>(pb + kmain + 16 * j - back);
                if constexpr (MB) { if (pg) a[j] = a[j] * *reinterpret_cast<const f32x4*>(pg + kmain + 16 * j - back); }
                if (back) { a[j] = f32x4{0.f, 0.f, 0.f, 0.f}; b[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
            }
#pragma unroll
        for (int j = 0; j < U; ++j)
            if (j < whole + half) {
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][e], b[j][e], acc[j & 1], 0, 0, 0);
            }
    }
    // C/D layout: column = lane & 15, row = 4 (lane >> 4) + reg
    const unsigned nn = n0 + li;
    if (nn >= (unsigned)Cout) return;
    const float sc = scale[nn], sh = shift[nn];
    float rv[4] = {0.f, 0.f, 0.f, 0.f};
    if (res) {
#pragma unroll
        for (int r = 0; r < 4; ++r) rv[r] = res[(size_t)min(m0 + 4 * g + r, M - 1) * Cout + nn];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned m = m0 + 4 * g + r;
        const float v = act_apply<MB>((acc[0][r] + acc[1][r]) * sc + sh, act) + rv[r];
        if (m < M) out[(size_t)m * Cout + nn] = v;
    }
}

int launch_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                     hipStream_t s) {
    if (B < 1 || Hi < 1 || Wi < 1) return FPC_EINVAL;
    const int Ho = (Hi - 1) / 2 + 1, Wo = (Wi - 1) / 2 + 1;
    const long long npix = (long long)B * Ho * Wo;
    if (npix * 8 >= kWalkLimit) return FPC_EINVAL;
    // (a thread loads its 108 weights once: a grid of npix / 256 workgroups gives it eight pixels to spend them on)
    hipLaunchKernelGGL(k_stem3x3s2<false>, dim3(stream_grid(npix)), dim3(256), 0, s, in4, w, scale, shift, out, (unsigned)npix, Hi, Wi, Ho, Wo);
    return check_launch();
}

// EfficientNet's stem: pads 0 before and 1 after, swish; even extents only (an odd one would read a second padded row or column)
int launch_mb_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                        hipStream_t s) {
    if (B < 1 || Hi < 2 || Wi < 2 || (Hi & 1) || (Wi & 1)) return FPC_EINVAL;
    const int Ho = Hi / 2, Wo = Wi / 2;
    const long long npix = (long long)B * Ho * Wo;
    if (npix * 8 >= kWalkLimit) return FPC_EINVAL;
    hipLaunchKernelGGL(k_stem3x3s2<true>, dim3(stream_grid(npix)), dim3(256), 0, s, in4, w, scale, shift, out, (unsigned)npix, Hi, Wi, Ho, Wo);
    return check_launch();
}

// The form of a site of M rows and Cout channels, a function of the shape alone: 0 = k_conv1x1_f32_small (16 x 16 tiles) where tiles
// of 32 x 32 would not give every SIMD of the chip a wave (fewer than 1024); else the channel tiles of 32 per wave of
// k_conv1x1_f32: the most of 5, 3, 2 that divides the site's tiles and still leaves 2048 waves (two per SIMD), else 1.
int conv1x1_f32_tiles(long long M, int Cout) {
    const long long mtiles = (M + 31) / 32;
    const int ntiles = (Cout + 31) / 32;
    if (mtiles * ntiles < 1024) return 0;
    for (int nt : {5, 3, 2})
        if (ntiles % nt == 0 && mtiles * (ntiles / nt) >= 2048) return nt;
    return 1;
}

// the launch of a checked 1x1 site on the form its shape names; MB: the EfficientNet instantiations (gate may be NULL)
template <bool MB>
static int launch_pw(const float* in, const float* w, const float* scale, const float* shift, const float* res, float* out, long long M,
                     int Cin, int Cout, int act, const float* gate, long long HW, hipStream_t s) {
    const int nt = conv1x1_f32_tiles(M, Cout);
    if (nt == 0) {
        const long long mt16 = (M + 15) / 16, nt16 = (Cout + 15) / 16;
        const long long grid = xcd_grid((mt16 * nt16 + 3) / 4);
        hipLaunchKernelGGL(k_conv1x1_f32_small<MB>, dim3((unsigned)grid), dim3(256), 0, s, in, w, scale, shift, res, out, (unsigned)M, Cin, Cout, act,
                           (unsigned)mt16, (unsigned)nt16, gate, (unsigned)HW);
        return check_launch();
    }
    const long long mtiles = (M + 31) / 32, nchunks = ((Cout + 31) / 32 + nt - 1) / nt, waves = mtiles * nchunks;
    if (waves >= (1LL << 31)) return FPC_EINVAL;
    const long long grid = xcd_grid((waves + 3) / 4);      // the workgroups past the last wave leave at once
    const dim3 g((unsigned)grid), b(256);
#define FPC_PW32(NT, U) hipLaunchKernelGGL((k_conv1x1_f32<NT, U, MB>), g, b, 0, s, in, w, scale, shift, res, out, (unsigned)M, Cin, Cout, act, (unsigned)mtiles, (unsigned)nchunks, gate, (unsigned)HW)
    if (nt == 5) FPC_PW32(5, 1);      // (K-steps per iteration: what the registers leave room for)
    else if (nt == 3) FPC_PW32(3, 2);
    else if (nt == 2) FPC_PW32(2, 4);
    else FPC_PW32(1, 4);
#undef FPC_PW32
    return check_launch();
}

int launch_conv1x1_f32(const float* in, const float* w, const float* scale, const float* shift, const float* res, float* out, long long M,
                       int Cin, int Cout, int act, hipStream_t s) {
    if (M < 1 || M >= (1LL << 31) - 64 || Cin < 8 || Cin > 1024 || Cin % 8 || Cout < 8 || Cout > 2048 || Cout % 8 || act < 0 || act > 1 ||
        (res && act))
        return FPC_EINVAL;
    return launch_pw<false>(in, w, scale, shift, res, out, M, Cin, Cout, act, nullptr, 1, s);
}

// The EfficientNet 1x1 sites: M = B HW rows, Cin up to kMbMaxCin (a project site's K is 6 x 192 = 1152), act 0 / 1 / 2 (swish), `gate`
// [B][Cin] or NULL.  The forms and their threshold are conv1x1_f32_tiles' whatever K is: NT and U are set by the registers (NT
// accumulator tiles of 16 and two operand sets of (NT + 1) U quads; the gate's quad is multiplied into the in operand's as it
// arrives and keeps no register of its own: the compiler's counts are 124 + 80 / 90 + 48 / 112 + 32 / 80 + 16 vector and accumulator
// registers for NT = 5 / 3 / 2 / 1, inside the 512 of two waves per SIMD as without the gate), not by the length of the K loop,
// which K = 1152 only makes longer (36 iterations of 32 at NT = 1, 18 of 64 on the 16 x 16 tiles); a frame's gate row is
// 4.6 KB at most and comes from L1 / L2.
int launch_mb_conv1x1(const float* in, const float* gate, const float* w, const float* scale, const float* shift, const float* res,
                      float* out, int B, long long HW, int Cin, int Cout, int act, hipStream_t s) {
    if (!mb_conv1x1_ok(B, HW, Cin, Cout) || act < 0 || act > 2 || (res && act)) return FPC_EINVAL;
    return launch_pw<true>(in, w, scale, shift, res, out, (long long)B * HW, Cin, Cout, act, gate, HW, s);
}

}  // namespace fpc

using namespace fpc;

extern "C" int fpc_conv1x1_f32(const float* in, const float* w, const float* scale, const float* shift, const float* res, float* out,
                               int64_t M, int Cin, int Cout, int act, fpc_stream_t stream) {
    if (!in || !w || !scale || !shift || !out || !al16(in) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out) || !al16(res))
        return FPC_EINVAL;
    return launch_conv1x1_f32(in, w, scale, shift, res, out, (long long)M, Cin, Cout, act, (hipStream_t)stream);
}

extern "C" int fpc_conv1x1_f32_form(int64_t M, int Cin, int Cout) {
    if (M < 1 || M >= (1LL << 31) - 64 || Cin < 8 || Cin > 1024 || Cin % 8 || Cout < 8 || Cout > 2048 || Cout % 8) return FPC_EINVAL;
    return conv1x1_f32_tiles((long long)M, Cout);
}

extern "C" int fpc_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                             int Cout, fpc_stream_t stream) {
    if (!in4 || !w || !scale || !shift || !out || !al16(in4) || !al16(w) || !al16(scale) || !al16(shift) || !al16(out)) return FPC_EINVAL;
    if (Cout != 32) return FPC_EINVAL;
    return launch_stem3x3s2(in4, w, scale, shift, out, B, Hi, Wi, (hipStream_t)stream);
}
