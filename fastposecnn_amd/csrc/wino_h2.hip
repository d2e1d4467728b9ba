// wino_h2.hip — k_conv_wino_h2: the four-wave Winograd F(2x2, 3x3) convolution (wino_w4.hip) on TWO fp16 pieces per operand
// instead of three bf16 pieces: four products in two matrix instructions per K-step instead of six in three (round 6).
//
// Why.  The split-precision forms are bound by instruction issue and by chip power: per K-step of 8 channels and
// 64 x 64 (tiles x channels) the bf16 x 3 form issues 48 matrix instructions, ~330 vector instructions (176 of them the three-way
// split, 96 operand moves) and streams 48 KB of weights.  With fp16 pieces an f32 operand needs TWO: x = h1 + h2 + rest with
// |rest| <= 3 * 2^-23 |x| (11 + 11 significant bits by TRUNCATION: the last two of x's 24 bits can be left over, 1.5 * 2^-22, and a
// mantissa of all ones attains it; residuals exact in f32; tests/test_piece_arithmetic.py).  All four piece products are
// kept: A = {h1, h1} x B = {g1, g2} and A = {h2, h2} x B = {g1, g2} — (h1 + h2)(g1 + g2) exactly, f32 accumulation; the SAME
// 16-byte weight fragment serves both, so a K-step is 32 matrix instructions, ~200 vector instructions (a pair of values
// splits in 8: v_cvt_pkrtz_f16_f32, two conversions back, two subtractions, v_cvt_pkrtz again, two copies) and 32 KB of
// weights; no {b3} fragment, no operand rebuild.
//
// Range (what fp16 pieces cost).  fp16 spans 2^-24 .. 65504.  WEIGHTS: k_wino_pack_fp16 scales the transformed weights of a
// convolution by a power of two s (from max |w| of the convolution, found on the device) so that max |U s| < 2^13, and the kernel
// multiplies its sums by 1 / s — exact.  ACTIVATIONS are not scaled: a transformed input value v (a signed sum of four activations)
// is represented to 3 * 2^-23 |v| (below 2^-21) while 2^-2 <= |v| < 2^16 and to 2^-24 ABSOLUTE below 2^-2 (fp16's subnormal spacing:
// the second piece, then the first, turn subnormal).  From |v| = 2^16 on the first piece is pinned at 65 504 and the second carries
// the excess on 11 bits: the error grows to 2^-10 (|v| - 65 504), 2^-12 of the value at 131 008 = 2 x 65 504, and beyond that the
// pair SATURATES (round-toward-zero conversions never produce infinity).  Against a tensor of scale ~1 that is f32-level accuracy
// (tests/test_gpu_net.py holds this form to the 2e-5 bar of every other form and the network to the 1e-4 float64 bars); a tensor
// whose values are all tiny (scale 1e-2) keeps ~3e-6 of ITS scale, one with transformed values beyond 6.5e4 loses precision and
// beyond 1.3e5 is wrong (tests/test_gpu_conv_operands.py; DESIGN.md 4.2, "Operand envelope").  The bf16 x 3 forms have
// neither limit and stay selectable: fpc_net_set_split_precision(net, 1) never picks this form, 2 allows it.
//
// Everything else — one wave per SIMD with 512 registers, a matrix instruction followed by its own item of the step's other work,
// weights straight into the operand registers one step ahead, the permuted LDS input image and its counted wait, operands written
// in place, the one-pass output transform — is the four-wave family's: the K loop's shape is wino_w4.hip's, the set-up around it and
// the output transform are wino_tile.hpp's; see there.
// Reference: the 3x3 / stride-1 convolutions of F/lib/pose_regressor.py:709-743 (smp encoder + FPN decoder, not vendored).
#include <algorithm>
#ifdef FPC_STAMP_WINO
#include <cstdlib>
#endif
#include "wino_tile.hpp"

namespace fpc {
using namespace wino_tile;

namespace {
constexpr int kStepBytes = 16 * 64 * 32;         // k_wino_pack_fp16<false>'s image of one K-step: [xi 16][tile 2][lane 64] x 16 bytes {g1 x 4 ch, g2 x 4 ch}
static_assert(kLdsFloats >= 2 * kInFloats, "the K loop's two input buffers live in the output image's space");
}  // namespace

// MODE (diagnostic instantiations of a -DFPC_STAMP_WINO build, FPC_H2_MODE at launch; the product is MODE 0): bit 0 = the K loop
// reloads no weights, bit 1 = it stages no input and has
// no barrier — wrong results, the same instruction stream otherwise
template <int MODE>
__global__ __launch_bounds__(256, 1) void k_conv_wino_h2(const WinoArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    long long* const dbg = kWinoStamp ? a.dbg : nullptr;      // a constant in the product build: the stamp code below folds away
    const long long t_entry = dbg ? clock64() : 0;
    const int t = threadIdx.x, lane = t & 63;
    const int wi = __builtin_amdgcn_readfirstlane(t >> 6);      // transform row of this wave (wave-uniform)
    const int li = lane & 31, lh = lane >> 5;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, HW = H * W;
    const int nkb = Cin >> 3;
    // weight slice (group, 64-channel block) fastest: fixed per XCD under round-robin dispatch (k_conv_wino)
    const WinoPatch pt = wino_patch<false>(blockIdx.x, Cout / kBN, a.groups, a.tbx, a.tby, 0, W, a.B, a.dec);
    const int nb = pt.nb, nnb = Cout / kBN;
    const ConvPtrs P = wino_group(a.p[0], a.p[1], a.p[2], a.p[3], pt.grp);
    const int y_in0 = 2 * pt.ty0 - 1, x_in0 = 2 * pt.tx0 - 1;

    f32x16 acc[4][2][2];      // [xi column j][tile half mt][32-channel tile nt]; zeroed while the first operands are on their way
    // ---- weights: buffer loads of this wave's fragments, one 16-byte {g1, g2} per (xi, 32-channel tile, lane) and K-step
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(reinterpret_cast<const char*>(P.w) + (size_t)nb * nkb * kStepBytes);
    const float inv_s = P.w[(size_t)nnb * nkb * (kStepBytes / 4)];      // 1 / (the power of two the weights were scaled by)
    const int vo_u = lane * 16;
    int so_u = wi * 4 * 2048;      // this wave's four xi; + kStepBytes per K-step
    u32x4 U[4][2];
#define FPC_H2_LOAD_U(J, NT) U[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, so_u + (J) * 2048 + (NT) * 1024, 0))
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) FPC_H2_LOAD_U(j, nt);
    if (nkb > 1) so_u += kStepBytes;
    // ---- input staging and fragment addressing (wino_tile.hpp)
    const float* isb = P.in + (size_t)pt.b * HW * Cin;            // image base, + 8 floats per step
    unsigned ivo[5];
    unsigned long long imask[5];
    wino_stage_plan<false>(ivo, imask, wi, lane, y_in0, x_in0, H, W, Cin, 0, pt.pk_ks, pt.pk_two);
#define FPC_H2_ISSUE_IN(BUF) wino_issue_in(lds + (BUF) * kInFloats, wi, ivo, imask, isb)
    int in_a[2], in_b[2];
    const float sgn = wino_frag<false>(in_a, in_b, wi, li, lh, pt.pk_ks);
    wino_zero_ring(lds, t, 2, y_in0, x_in0, H, W, false);
    FPC_H2_ISSUE_IN(0);
    if (nkb > 1) isb += 8;
    FPC_H2_ISSUE_IN(1);
    if (nkb > 2) isb += 8;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][mt][nt][r] = 0.f;

    const long long t_issued = dbg ? clock64() : 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t_landed = dbg ? clock64() : 0;
    __syncthreads();
    const long long t_synced = dbg ? clock64() : 0;

    // operands of the current step's transformed fragments, as the matrix instructions take them: TA1[j][mt] = {h1, h1},
    // TA2[j][mt] = {h2, h2} (four channels per piece); transformed values vn[mt][j] of the step
    // whose pieces are being built (xi 3's wait there across the loop's back edge)
    u32x4 TA1[4][2], TA2[4][2];
    f32x4 vn[2][4];
    // one pair of values of vn[MT][J] -> its fp16 pieces (pinned to its slot by the volatile asm that reads them, as wino_w4.hip's items)
#define FPC_H2_SPLIT_PAIR(J, MT, PAIR)                                                                        \
    do {                                                                                                      \
        const float x0_ = vn[MT][J][2 * (PAIR)], x1_ = vn[MT][J][2 * (PAIR) + 1];                             \
        const fp16x2 h_ = __builtin_amdgcn_cvt_pkrtz(x0_, x1_);                                               \
        const float r0_ = x0_ - (float)h_[0], r1_ = x1_ - (float)h_[1];                                       \
        const unsigned k1_ = __builtin_bit_cast(unsigned, h_);                                                \
        const unsigned k2_ = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0_, r1_));              \
        asm volatile("" :: "v"(k1_), "v"(k2_));                                                               \
        TA1[J][MT][PAIR] = k1_; TA1[J][MT][2 + (PAIR)] = k1_; TA2[J][MT][PAIR] = k2_; TA2[J][MT][2 + (PAIR)] = k2_; \
    } while (0)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) { TA1[j][mt] = u32x4{0u, 0u, 0u, 0u}; TA2[j][mt] = u32x4{0u, 0u, 0u, 0u}; }
    {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 e[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                e[c] = fma_s4(sgn, *reinterpret_cast<const f32x4*>(lds + in_b[c >> 1] + (c & 1) * in_cs + mt * in_ms),
                              *reinterpret_cast<const f32x4*>(lds + in_a[c >> 1] + (c & 1) * in_cs + mt * in_ms));
            vn[mt][0] = sub_s4(e[0], e[2]); vn[mt][1] = add_s4(e[1], e[2]); vn[mt][2] = sub_s4(e[2], e[1]); vn[mt][3] = sub_s4(e[1], e[3]);
#pragma unroll
            for (int j = 0; j < 3; ++j) { FPC_H2_SPLIT_PAIR(j, mt, 0); FPC_H2_SPLIT_PAIR(j, mt, 1); }
        }
    }
    __syncthreads();       // buffer 0 is refilled by step 0's DMA

#define FPC_H2_MFMA(J, MT, NT, A, B) acc[J][MT][NT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), acc[J][MT][NT], 0, 0, 0)
#define FPC_H2_PIN4(V) asm volatile("" :: "v"(V))
    int cur = 0;
    const long long c_begin = dbg ? clock64() : 0, r_begin = dbg ? wall_clock64() : 0;
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
        // input of step kb + 2 -> the buffer step kb's fragments were read from during step kb - 1 (oldest in the queue: see the wait below)
        if (!(MODE & 2) && !(MODE & 8)) FPC_H2_ISSUE_IN(cur);
        const float* In = lds + (cur ^ 1) * kInFloats;
        f32x4 da[2][4], db[2][4], e[2][4];
        __builtin_amdgcn_s_setprio(1);
        // Slot sl = 8 j + 4 g + 2 mt + nt: g = 0: h1 g1 + h1 g2, g = 1: h2 g1 + h2 g2.  One item per slot:
        //   sl  0- 3  fragment reads of step kb + 1 (two columns of one tile half each) + the split of THIS step's xi 3 (one pair of
        //             values each: half 0 pairs 0, 1, half 1 pairs 0, 1)
        //   sl  4-11  row transform e = da + sgn db (one column of one half each)      sl 12-19  column transform vn (one xi of one half each)
        //   sl 20-31  split of step kb + 1's xi 0, 1, 2 (four pairs each) — xi j's operands are overwritten after xi j's last matrix
        //             instruction (slot 8 j + 7)
        // The last matrix instruction of a weight fragment (g = 1, half 1) is followed by the fragment's reload for step kb + 1.
#define FPC_H2_SPLIT_Q(J, Q) do { if ((Q) == 0) FPC_H2_SPLIT_PAIR(J, 0, 0); if ((Q) == 1) FPC_H2_SPLIT_PAIR(J, 0, 1); if ((Q) == 2) FPC_H2_SPLIT_PAIR(J, 1, 0); if ((Q) == 3) FPC_H2_SPLIT_PAIR(J, 1, 1); } while (0)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int sl = 8 * j + 4 * g + 2 * mt + nt;
                        if (g == 0) FPC_H2_MFMA(j, mt, nt, TA1[j][mt], U[j][nt]);
                        if (g == 1) {
                            FPC_H2_MFMA(j, mt, nt, TA2[j][mt], U[j][nt]);
                            if (mt == 1 && !(MODE & 1)) FPC_H2_LOAD_U(j, nt);
                        }
                        if (sl < 4) {
#pragma unroll
                            for (int c = 2 * (sl & 1); c < 2 * (sl & 1) + 2; ++c) {
                                da[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_a[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                                db[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_b[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                            }
                            FPC_H2_SPLIT_Q(3, sl);
                        }
                        if (sl >= 4 && sl < 12) {
                            const int m_ = (sl - 4) >> 2, c = (sl - 4) & 3;
                            e[m_][c] = fma_s4(sgn, db[m_][c], da[m_][c]);
                            FPC_H2_PIN4(e[m_][c]);
                        }
                        if (sl >= 12 && sl < 20) {
                            const int m_ = (sl - 12) >> 2, jx = (sl - 12) & 3;
                            if (jx == 0) vn[m_][0] = sub_s4(e[m_][0], e[m_][2]);
                            if (jx == 1) vn[m_][1] = add_s4(e[m_][1], e[m_][2]);
                            if (jx == 2) vn[m_][2] = sub_s4(e[m_][2], e[m_][1]);
                            if (jx == 3) vn[m_][3] = sub_s4(e[m_][1], e[m_][3]);
                            FPC_H2_PIN4(vn[m_][jx]);
                        }
                        if (sl >= 20 && sl < 24) FPC_H2_SPLIT_Q(0, sl - 20);
                        if (sl >= 24 && sl < 28) FPC_H2_SPLIT_Q(1, sl - 24);
                        if (sl >= 28) FPC_H2_SPLIT_Q(2, sl - 28);
                        __builtin_amdgcn_sched_barrier(0);
                    }
#undef FPC_H2_SPLIT_Q
        __builtin_amdgcn_s_setprio(0);
        so_u += kb + 2 < nkb ? kStepBytes : 0;
        isb += kb + 3 < nkb ? 8 : 0;
        // this wave's DMA pieces (issued before the step's 8 weight loads, which stay in flight) have landed
        if (!(MODE & 2)) {
            if (MODE & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            if (!(MODE & 4)) __syncthreads();                 // everybody's have; this step's fragment reads are done
        }
        cur ^= 1;
    }
#undef FPC_H2_MFMA
#undef FPC_H2_SPLIT_PAIR
#undef FPC_H2_PIN4
#undef FPC_H2_ISSUE_IN
#undef FPC_H2_LOAD_U
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the last steps' redundant staging has landed before LDS is reused
    const long long t_kend = dbg ? clock64() : 0;
    if (dbg && lane == 0) {      // tools_dev/wino_stamps.py: shader-clock ticks and 100 MHz reference ticks of the K loop, entry -> loop
        long long* o = dbg + ((size_t)blockIdx.x * 4 + wi) * 8;
        o[0] = t_issued - t_entry; o[1] = t_landed - t_issued; o[2] = t_synced - t_landed;      // entry: set-up + issue | first operands land | barrier
        o[3] = t_kend - c_begin; o[4] = wall_clock64() - r_begin; o[5] = nkb; o[6] = c_begin - t_entry;
    }
    wino_output<false, false>(lds, acc, P, pt, WinoEpi{H, W, Cout, a.relu, a.tbx, a.tby, 0, a.exit_general}, inv_s, nullptr, dbg, t_kend, t, wi);
}

// max |w| of a convolution's weights as the bit pattern of a non-negative float (atomicMax on unsigned keeps the order): one atomic
// per workgroup, at most 64 workgroups (4 096 same-address atomics — one per wave of 1 024 workgroups — took 48 us)
__global__ __launch_bounds__(256) void k_absmax_bits(const float* __restrict__ w, long long n, unsigned* __restrict__ out) {
    __shared__ unsigned s_m[4];
    unsigned m = 0u;
    const long long n4 = n >> 2;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < n4; g += (long long)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<const f32x4*>(w)[g];
        m = max(max(m, __builtin_bit_cast(unsigned, fabsf(v[0]))), max(__builtin_bit_cast(unsigned, fabsf(v[1])),
                max(__builtin_bit_cast(unsigned, fabsf(v[2])), __builtin_bit_cast(unsigned, fabsf(v[3])))));
    }
    if (blockIdx.x == 0)
        for (long long g = 4 * n4 + threadIdx.x; g < n; g += blockDim.x) m = max(m, __builtin_bit_cast(unsigned, fabsf(w[g])));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
        if (m) atomicMax(out, m);
    }
}

int launch_absmax_bits(const float* w, long long n, unsigned* out, hipStream_t s) {
    hipLaunchKernelGGL(k_absmax_bits, dim3((unsigned)std::min<long long>((n / 4 + 255) / 256 + 1, 64)), dim3(256), 0, s, w, n, out);
    return check_launch();
}

// OIHW 3x3 weights -> U = G g G^T, scaled by s = 2^k (the largest power of two with 2.25 max |w| s < 2^13: |U| <= 2.25 max |w|) and
// split into two fp16 pieces by truncation (U s = g1 + g2 + rest, |rest| <= 3 * 2^-23 |U s| while |U s| >= 2^-2, < 2^-24 below), in
// the fragment order the lanes load.  (s = 2^(13 - e), 2.25 max |w| = m 2^e, m in [0.5, 1); 13 - e is clamped to +-100.)
// lane = (channel half) * 32 + (co & 31), tile = (co & 63) >> 5; the two forms differ only in where a fragment lands:
//   k_conv_wino_h2  [Cout/64][Cin/8][xi 16][tile 2][lane 64] x {g1 x 4 ch, g2 x 4 ch}
//   PAIR (k_conv_wino_h3)  [Cout/64][Cin/16][xi 16][tile 2][piece 2][lane 64] x {4 ch of the even K-step, 4 ch of the odd one}
// tail[0] = 1 / s (f32).  tail[1] holds max |w|'s bits (k_absmax_bits).  tr = 1: the taps are read transposed, tap (r, c) from
// (c, r): the image of a site that runs transposed (wino_h3.hip: wino_orient_rule).
template <bool PAIR>
__global__ __launch_bounds__(256) void k_wino_pack_fp16(const float* __restrict__ w, unsigned short* __restrict__ out, float* __restrict__ tail,
                                                        int Cout, int Cin, int tr) {
    const float wmax = __builtin_bit_cast(float, reinterpret_cast<const unsigned*>(tail)[1]);
    int ex = 0;
    if (wmax > 0.f && wmax < 3.0e38f) { (void)frexpf(2.25f * wmax, &ex); ex = 13 - ex; }      // 2.25 wmax = m 2^e, m in [0.5, 1): (2.25 wmax) 2^(13 - e) < 2^13
    ex = max(-100, min(100, ex));
    const float sc = ldexpf(1.0f, ex);
    if (blockIdx.x == 0 && threadIdx.x == 0) tail[0] = ldexpf(1.0f, -ex);
    const long long total = (long long)Cout * Cin;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % Cin), co = (int)(g / Cin);
        const float* k = w + ((size_t)co * Cin + ci) * 9;
        float gg[4][3];
        const int sr = tr ? 1 : 3, scol = tr ? 3 : 1;      // strides of a tap row / column in the 3 x 3 block
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g0 = k[c * scol] * sc, g1 = k[sr + c * scol] * sc, g2 = k[2 * sr + c * scol] * sc;      // (a power of two: commutes with the transform's roundings)
            gg[0][c] = g0;
            gg[1][c] = 0.5f * (g0 + g1 + g2);
            gg[2][c] = 0.5f * (g0 - g1 + g2);
            gg[3][c] = g2;
        }
        const int nb = co >> 6, col = co & 63, nt = col >> 5, kb = ci >> 3, cil = ci & 7, e = cil & 3;
        const int ln = (cil >> 2) * 32 + (col & 31);
        // 16-bit offsets: the K-step's (pair's) image; a fragment's first piece inside it per xi, its second piece behind the first
        unsigned short* img = out + (PAIR ? ((size_t)nb * (Cin >> 4) + (kb >> 1)) * (kPairBytes / 2) : ((size_t)nb * (Cin >> 3) + kb) * (kStepBytes / 2));
        const int f0 = PAIR ? (nt * 2048 + ln * 16) / 2 + (kb & 1) * 4 + e : (nt * 1024 + ln * 16) / 2 + e;
        constexpr int xi_s = PAIR ? 4096 / 2 : 2048 / 2, p2 = PAIR ? 512 : 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float r0 = gg[i][0], r1 = gg[i][1], r2 = gg[i][2];
            const float u[4] = {r0, 0.5f * (r0 + r1 + r2), 0.5f * (r0 - r1 + r2), r2};
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const float x = u[jx];
                const fp16x2 h = __builtin_amdgcn_cvt_pkrtz(x, 0.f);
                const float r = x - (float)h[0];
                const fp16x2 h2 = __builtin_amdgcn_cvt_pkrtz(r, 0.f);
                unsigned short* frag = img + (4 * i + jx) * xi_s + f0;
                frag[0] = (unsigned short)(__builtin_bit_cast(unsigned, h) & 0xFFFFu);
                frag[p2] = (unsigned short)(__builtin_bit_cast(unsigned, h2) & 0xFFFFu);
            }
        }
    }
}

// fragment-order fp16 x 2 image: 16 * Cout * Cin floats + a tail of 2 (1 / scale, max |w| bits); every byte is written
int launch_wino_pack_fp16(const float* w_oihw, float* packed, int Cout, int Cin, bool pair, const float* w_also, int Cin_also, bool transpose,
                          hipStream_t s) {
    if (Cin % (pair ? 16 : 8) != 0 || Cout % kBN != 0 || ((uintptr_t)w_oihw & 15) || ((uintptr_t)w_also & 15)) return FPC_EINVAL;
    float* tail = packed + (size_t)16 * Cout * Cin;
    if (hipMemsetAsync(tail, 0, 2 * sizeof(float), s) != hipSuccess) return FPC_ELAUNCH;
    int rc = launch_absmax_bits(w_oihw, (long long)Cout * Cin * 9, reinterpret_cast<unsigned*>(tail) + 1, s);
    if (!rc && w_also) rc = launch_absmax_bits(w_also, (long long)Cout * Cin_also * 9, reinterpret_cast<unsigned*>(tail) + 1, s);
    if (rc) return rc;
    const dim3 grid((unsigned)std::min<long long>(((long long)Cout * Cin + 255) / 256, 4096));
    if (pair) hipLaunchKernelGGL(k_wino_pack_fp16<true>, grid, dim3(256), 0, s, w_oihw, reinterpret_cast<unsigned short*>(packed), tail, Cout, Cin, transpose ? 1 : 0);
    else hipLaunchKernelGGL(k_wino_pack_fp16<false>, grid, dim3(256), 0, s, w_oihw, reinterpret_cast<unsigned short*>(packed), tail, Cout, Cin, transpose ? 1 : 0);
    return check_launch();
}

int launch_wino_pack_h2(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s) {
    return launch_wino_pack_fp16(w_oihw, packed, Cout, Cin, false, nullptr, 0, false, s);
}

// .w = the k_wino_pack_fp16<false> image (+ its tail), .waves = 8 (tby = ceil(ceil(H / 2) / 8): 8 x 8 tile patches)
int launch_conv_wino_h2(const WinoArgs& a_in, int groups, hipStream_t s) {
    long long nblk;
    if (const int rc = wino_tile_check(a_in, groups, 8, kStepBytes, false, &nblk)) return rc;
    WinoArgs a = a_in;      // + the reciprocals of the workgroup-id decode (wino_patch)
    a.dec = wino_decode(a.Cout, groups, a.tbx, a.tby, a.W, a.B, 0);
#ifdef FPC_STAMP_WINO
    static const int mode = getenv("FPC_H2_MODE") ? atoi(getenv("FPC_H2_MODE")) : 0;      // diagnostic
    if (mode == 1) hipLaunchKernelGGL(k_conv_wino_h2<1>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 2) hipLaunchKernelGGL(k_conv_wino_h2<2>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 3) hipLaunchKernelGGL(k_conv_wino_h2<3>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 5) hipLaunchKernelGGL(k_conv_wino_h2<5>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // no weights, DMA, no barrier
    else if (mode == 9) hipLaunchKernelGGL(k_conv_wino_h2<9>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // no weights, barrier, no DMA
    else if (mode == 4) hipLaunchKernelGGL(k_conv_wino_h2<4>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // everything but the barrier
    else
#endif
    hipLaunchKernelGGL(k_conv_wino_h2<0>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return check_launch();
}

}  // namespace fpc
