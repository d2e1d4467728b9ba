// wino_f32.hip — k_conv_wino, the oldest Winograd F(2x2, 3x3) kernel of the backbone engine (fpc_conv2d's forms -1 ... -5: 4 or 8
// waves, f32 products in the barrier, wave-private and all-DMA forms, bf16 x 3 products in the 8-wave barrier form), its weight
// packers k_wino_pack / k_wino_pack_bf3 and the zero page of the all-DMA forms.  The later forms have files of their own:
// wino128.hip (-6), wino_w4.hip (-7), wino_h2.hip (-8), wino_h3.hip (-9, -10).
// Reference: the 3x3 / stride-1 convolutions of F/lib/pose_regressor.py:709-743 (smp encoder + FPN decoder, not vendored).
#include "conv_device.hpp"

namespace fpc {

// ------------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) convolution (3x3, stride 1, pad 1) on the f32 matrix cores: 2.25x fewer
// multiply-adds than the direct form, all in f32.
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A  per 4x4 input patch d / 2x2 output tile, summed over Cin:
//   16 independent GEMMs  M_xi[tile][co] = sum_ci V_xi[tile][ci] * U_xi[ci][co].
// One workgroup = an 8x4 patch of tiles (16x8 output pixels) x 64 output channels x all 16 xi.
// Wave w owns transform row i = w (xi = 4i..4i+3): 4 xi x 2 column tiles of 32 = 8 MFMA accumulators.
// Per K-step of 8 input channels the RAW 18x10 input region and the pre-transformed weights
// (fpc::k_wino_pack, 32 KB contiguous per step) are staged global -> registers -> LDS; each lane builds
// its four V_xi fragments from 8 LDS reads + 8 vector adds, so the transformed input never exists in
// memory.  The output transform runs through LDS (wave i holds row i of M) and feeds the same
// epilogue as the direct kernel (BatchNorm / bias, residual, ReLU, GroupNorm partial sums).
#ifndef FPC_WINO_PRIO_HI
#define FPC_WINO_PRIO_HI 1
#endif
#ifndef FPC_WINO_STAGGER
#define FPC_WINO_STAGGER 1
#endif
#ifndef FPC_WINO_B3_OLDER
#define FPC_WINO_B3_OLDER 1
#endif
#ifndef FPC_WINO_IN_OLDER
#define FPC_WINO_IN_OLDER 0
#endif
#ifndef FPC_WINO_LATE_AT
#define FPC_WINO_LATE_AT 0
#endif
constexpr int kWinoTX = 8;                              // tile patch per workgroup: 8 wide, NW tall (NW = 4 or 8 waves)
constexpr int kWinoRW = 2 * kWinoTX + 2;                // input region width 18
constexpr int kWinoIS = 8;                              // floats per staged position (one 32-byte K-step slice)
constexpr int kWinoBN = 64;
constexpr int kWinoLdsW = 16 * kWinoBN * 8;             // 8192 floats (32 KB) per weight buffer

// NW = 4: 32 tiles (16x8 output pixels) per workgroup, 2 workgroups per CU.
// NW = 8: 64 tiles (16x16 pixels), waves 4-7 work on the lower half of the patch with the SAME weights in
//         LDS: 11.8 instead of 6.7 multiply-adds per staged byte.  The kernels sit on the ~10 B/clk/CU the
//         global -> LDS path delivers (measured: MFMA busy 52 % at 6.7 MAC/B), so this is the lever for
//         the large maps; the 4-wave form keeps more workgroups for the small ones.
// WP ("wave private", NW = 4): no barrier inside the K loop.  A wave needs only ITS four xi rows of the
// weight image (exactly the 8 KB it DMAs itself) and 5 or 8 rows of the input region, which it stages
// into a private LDS patch; every fragment of a K-step is pulled into registers first, so the single
// LDS buffer can be refilled (DMA + ds_write) under that step's 32 MFMAs.  Ablation of the barrier form:
// the two barriers per step cost 17 % of the kernel, they also force the four waves into lockstep.
// P3 (NW = 8): every operand goes global -> LDS by DMA (out-of-image positions read a zero page), three
// LDS stages, the loads of step k+2 are issued before step k's MFMAs and the wave waits with a COUNTED
// vmcnt (the newest batch stays in flight across the raw s_barrier) — guide "Pipelining across barriers".
// DBG: diagnostic instantiations that stamp the K-loop phases with s_memtime (tools_dev/wino_stamps.py; -DFPC_STAMP_WINO builds only).
// BF3 (NW = 8, barrier form): split-precision products.  The transformed input tile is split EXACTLY into three bf16
// pieces per value between the MFMAs, the weights arrive pre-split (k_wino_pack_bf3: a 32 KB {b1, b2} image in the f32
// image's own layout + a 16 KB {b3} image per K-step), and the 8-channel K-step of a 32 x 32 tile is THREE
// v_mfma_f32_32x32x16_bf16 (slots: a1 b1, a1 b2 | a2 b1, a2 b2 | a1 b3, a3 b1 for the lane half's four channels;
// dropped products < 2^-23 of the term, f32 accumulation) instead of four v_mfma_f32_32x32x2_f32: 96 instead of 256
// matrix cycles.  118 KB of LDS: one 8-wave workgroup per CU, as the f32 8-wave form.
template <int NW, bool WP, bool P3, bool DBG = false, bool BF3 = false>
__global__ __launch_bounds__(64 * NW, BF3 ? 1 : 2) void k_conv_wino(const WinoArgs a) {
    constexpr int TY = NW;                                  // tile rows of the patch
    constexpr int RH = 2 * TY + 2, POS = kWinoRW * RH;      // staged input region
    constexpr int NT = 8 * NW;                              // tiles per workgroup
    constexpr int WPI = 8 * kWinoRW * kWinoIS;              // WP: floats of a wave's private input patch (8 rows)
    constexpr int IP3 = 512 * kWinoIS;                      // P3: floats per input stage (16 pieces of 1 KB, 324 positions used)
    // barrier form: 1 KB input pieces per stage, floats per input buffer.  PERM (the BF3 form): the 16-byte units of the region
    // are PERMUTED in LDS so that the fragment reads are conflict-free — position (ry, rx), channel half hf lives in unit
    //   (((a >> 2) * 3 + (q >> 2)) * 8 + (ry & 1) * 4 + (rx & 1) * 2 + hf) * 16 + 4 * (q & 3) + (a & 3),   a = ry >> 1, q = rx >> 1:
    // the 16 lanes of a ds_read_b128 group are 4 tile rows x 4 tile columns at fixed row / column parity, i.e. 16 different
    // (a & 3, q & 3) = 16 different 16-byte bank slots (the row-major image put them on 4: every read 4-way, 1024 of the
    // ~2300 LDS cycles of a K-step).  The DMA lands lane-linear pieces, so the permutation is only the choice of the global
    // address each lane fetches; 72 x 16 units = 18 pieces with 648 of 1152 lanes active.
    constexpr bool PERM = BF3;
    constexpr int NPI = PERM ? 18 : (POS + 31) / 32, LINP = NPI * 256;
    // input pieces per wave and K-step: piece (wave + IST i), i < NIN.  NW = 8: 18 (PERM) / 11 pieces over the 8 waves, or —
    // FPC_WINO_IN_OLDER — over the four older waves only (see the {b3} pieces)
    constexpr bool INO = PERM && FPC_WINO_IN_OLDER;
    constexpr int NIN = INO ? 5 : (PERM ? 3 : 2), IST = INO ? 4 : NW;
    static_assert(!PERM || NW == 8, "permuted input image is laid out for the 18 x 18 region");
    constexpr int kWB = BF3 ? 12288 : kWinoLdsW;            // floats per weight buffer (BF3: 32 KB {b1, b2} + 16 KB {b3})
    constexpr int kLdsFloats = WP ? (kWinoLdsW + 4 * WPI) : P3 ? (3 * IP3 + 3 * kWinoLdsW) : (2 * LINP + 2 * kWB);
    static_assert(!BF3 || (NW == 8 && !WP && !P3), "split precision rides on the 8-wave barrier form");
    static_assert(!WP || NW == 4, "wave-private form is written for 4 waves");
    static_assert(!P3 || (NW == 8 && !WP), "three-stage DMA form is written for 8 waves");
    static_assert(kLdsFloats >= 2 * 4 * NT * 32, "output transform needs 2*4*NT*32 floats");
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const long long t_entry = DBG ? clock64() : 0;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int wi = wv & 3, half = wv >> 2;                  // transform row of this wave, tile-row group
    const int li = lane & 31, lh = lane >> 5;
    const int H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, HW = H * W;
    const int nkb = Cin >> 3;
    // weight slice (group, 64-channel block) fastest: fixed per XCD under round-robin dispatch, so each
    // XCD's L2 keeps the 16*64*Cin*4 bytes of transformed weights all its workgroups stream (see k_conv_igemm)
    int bid = blockIdx.x;
    const int nnb = Cout / kWinoBN;
    const int nb = bid % nnb; bid /= nnb;
    const int grp = bid % a.groups; bid /= a.groups;
    const int bx = bid % a.tbx; bid /= a.tbx;
    const int by = bid % a.tby;
    const int b = bid / a.tby;
    ConvPtrs P = a.p[0];
    if (grp == 1) P = a.p[1];
    if (grp == 2) P = a.p[2];
    if (grp == 3) P = a.p[3];
    const int ty0 = by * TY, tx0 = bx * kWinoTX;
    const int y_in0 = 2 * ty0 - 1, x_in0 = 2 * tx0 - 1;

    f32x16 acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][nt][r] = 0.f;
    // row pair (ra, rb) and sign of B^T row wi:  0: d0-d2   1: d1+d2   2: d2-d1   3: d1-d3
    const float sgn = (wi == 1) ? 1.f : -1.f;

    if constexpr (WP) {
        // ---- wave-private staging
        float* const Wp = lds + wi * 2048;                        // this wave's xi rows [4][64][8]
        float* const Ip = lds + kWinoLdsW + wi * WPI;             // this wave's input rows [<=8][18][8]
        const float* wsrc = P.w + (size_t)nb * nkb * kWinoLdsW + wi * 2048 + 4 * lane;
        const bool outer = (wi == 0 || wi == 3);                  // 5 region rows (every other one), else rows 1..8
        const int nrows = outer ? 5 : 8;
        long long i_src[5];
        int i_dst[5];
        bool i_ok[5], i_use[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            int f = lane + 64 * i;
            int q = f >> 1, hf = f & 1;
            int lr = q / kWinoRW, rx = q - lr * kWinoRW;
            i_use[i] = lr < nrows;
            int ry = outer ? 2 * lr + (wi == 3 ? 1 : 0) : lr + 1;  // region row of private row lr
            int y = y_in0 + ry, x = x_in0 + rx;
            i_ok[i] = i_use[i] && y >= 0 && y < H && x >= 0 && x < W;
            i_src[i] = ((long long)b * HW + (long long)y * W + x) * Cin + 4 * hf;
            i_dst[i] = q * kWinoIS + 4 * hf;
        }
        const int tyl = li >> 3, txl = li & 7;
        // private rows holding patch rows (2*tyl + ra) and (2*tyl + rb)
        const int lra = outer ? tyl : (wi == 1 ? 2 * tyl : 2 * tyl + 1);
        const int lrb = outer ? tyl + 1 : (wi == 1 ? 2 * tyl + 1 : 2 * tyl);
        const int in_a = (lra * kWinoRW + 2 * txl) * kWinoIS + 4 * lh;
        const int in_b = (lrb * kWinoRW + 2 * txl) * kWinoIS + 4 * lh;
        int w_frag[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            int co = nt * 32 + li;
            w_frag[nt] = co * 8 + 4 * (lh ^ ((co >> 3) & 1));
        }
        f32x4 ri[5];
#define FPC_WP_ISSUE(KB)                                                                                      \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < 8; ++i) __builtin_amdgcn_global_load_lds(                       \
            (const __attribute__((address_space(1))) void*)(wsrc + (size_t)(KB) * kWinoLdsW + 256 * i),      \
            (__attribute__((address_space(3))) void*)(Wp + i * 256), 16, 0, 0);                               \
        _Pragma("unroll") for (int i = 0; i < 5; ++i) ri[i] =                                                 \
            i_ok[i] ? *reinterpret_cast<const f32x4*>(P.in + i_src[i] + 8 * (KB)) : f32x4{0.f, 0.f, 0.f, 0.f}; \
    } while (0)
#define FPC_WP_LAND()                                                                                         \
    do {                                                                                                      \
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                      \
        _Pragma("unroll") for (int i = 0; i < 5; ++i)                                                         \
            if (i_use[i]) *reinterpret_cast<f32x4*>(Ip + i_dst[i]) = ri[i];                                   \
    } while (0)
        FPC_WP_ISSUE(0);
        FPC_WP_LAND();
        for (int kb = 0; kb < nkb; ++kb) {
            // every fragment of this K-step into registers
            f32x4 e[4], v[4], u[4][2];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                f32x4 da = *reinterpret_cast<const f32x4*>(Ip + in_a + c * kWinoIS);
                f32x4 db = *reinterpret_cast<const f32x4*>(Ip + in_b + c * kWinoIS);
                e[c] = da + sgn * db;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j][0] = *reinterpret_cast<const f32x4*>(Wp + j * 512 + w_frag[0]);
                u[j][1] = *reinterpret_cast<const f32x4*>(Wp + j * 512 + w_frag[1]);
            }
            v[0] = sub_pk(e[0], e[2]); v[1] = e[1] + e[2]; v[2] = sub_pk(e[2], e[1]); v[3] = sub_pk(e[1], e[3]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");    // LDS reads complete: the patch may be refilled
            __builtin_amdgcn_sched_barrier(0);
            if (kb + 1 < nkb) FPC_WP_ISSUE(kb + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][q], u[j][0][q], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][q], u[j][1][q], acc[j][1], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
            if (kb + 1 < nkb) FPC_WP_LAND();
        }
#undef FPC_WP_ISSUE
#undef FPC_WP_LAND
    } else if constexpr (P3) {
        // Measured on the barrier form (s_memtime stamps): while the co-resident wave of a SIMD issues its 32
        // MFMAs back to back, THIS wave's vector instructions (address maths, the input transform) get the
        // vector ALU only at MFMA boundaries — 1600 + 1350 cycles per K-step for ~60 VALU instructions beside
        // 2200 cycles of MFMA issue.  So here every vector instruction that is not an MFMA sits in the shadow
        // of the wave's OWN MFMAs: the next step's fragments are read and transformed between the MFMAs of
        // the second half of the current step, DMA addressing is scalar, and the single barrier of a step sits
        // in the middle of its MFMA block.
        float* const lds_w = lds + 3 * IP3;
        const int swv = __builtin_amdgcn_readfirstlane(wv);
        const float* wbase = P.w + (size_t)nb * nkb * kWinoLdsW + (swv * 4 * 256);     // wave-uniform
        const unsigned lane16 = 4u * lane;                                            // floats
        const float* isrc[2];
        int istep[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            int q = (swv + 8 * i) * 32 + (lane >> 1), hf = lane & 1;     // LDS position of this lane's 16 bytes
            int ry = q / kWinoRW, rx = q - ry * kWinoRW;
            int y = y_in0 + ry, x = x_in0 + rx;
            bool ok = q < POS && y >= 0 && y < H && x >= 0 && x < W;
            isrc[i] = ok ? P.in + ((long long)b * HW + (long long)y * W + x) * Cin + 4 * hf : a.zeros;
            istep[i] = ok ? 8 : 0;
        }
#define FPC_P3_ISSUE(KB, BUF)                                                                                 \
    do {                                                                                                      \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) __builtin_amdgcn_global_load_lds(                       \
            (const __attribute__((address_space(1))) void*)(wbase + (size_t)(KB) * kWinoLdsW + 256 * i + lane16), \
            (__attribute__((address_space(3))) void*)(lds_w + (BUF) * kWinoLdsW + (swv * 4 + i) * 256), 16, 0, 0); \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                       \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)isrc[i],          \
                (__attribute__((address_space(3))) void*)(lds + (BUF) * IP3 + (swv + 8 * i) * 256), 16, 0, 0); \
            isrc[i] += istep[i];                                                                              \
        }                                                                                                     \
    } while (0)
        const int tyl = (li >> 3) + 4 * half, txl = li & 7;
        const int ra = (wi == 0) ? 0 : (wi == 2 ? 2 : 1);
        const int rb = (wi == 0) ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
        const int in_a = ((2 * tyl + ra) * kWinoRW + 2 * txl) * kWinoIS + 4 * lh;
        const int in_b = ((2 * tyl + rb) * kWinoRW + 2 * txl) * kWinoIS + 4 * lh;
        int w_frag[2];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            int co = nt * 32 + li;
            w_frag[nt] = ((4 * wi) * kWinoBN + co) * 8 + 4 * (lh ^ ((co >> 3) & 1));
        }
        const f32x4 sg4 = {sgn, sgn, sgn, sgn};
#define FPC_P3_MFMA8(J, U0, U1)                                                                               \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
        acc[J][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[J][q], U0[q], acc[J][0], 0, 0, 0);                 \
        acc[J][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[J][q], U1[q], acc[J][1], 0, 0, 0);                 \
    }
        // prologue: stages 0 and 1 in flight, fragments of step 0 transformed
        FPC_P3_ISSUE(0, 0);
        if (nkb > 1) FPC_P3_ISSUE(1, 1);
        if (nkb > 1) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        f32x4 v[4];
        {
            f32x4 e[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                e[c] = __builtin_elementwise_fma(sg4, *reinterpret_cast<const f32x4*>(lds + in_b + c * kWinoIS),
                                                 *reinterpret_cast<const f32x4*>(lds + in_a + c * kWinoIS));
            v[0] = sub_pk(e[0], e[2]); v[1] = e[1] + e[2]; v[2] = sub_pk(e[2], e[1]); v[3] = sub_pk(e[1], e[3]);
        }
        long long stamp[6] = {0, 0, 0, 0, 0, 0};
        const bool dbg = DBG && a.dbg != nullptr;
#define FPC_STAMP(I) do { if (DBG && dbg) { long long now_ = clock64(); stamp[I] += now_ - tprev; tprev = now_; } } while (0)
        long long tprev = dbg ? clock64() : 0;
        const long long c_begin = tprev, r_begin = dbg ? wall_clock64() : 0;
        int cur = 0;
        for (int kb = 0; kb < nkb; ++kb) {
            int nxt = cur + 1 == 3 ? 0 : cur + 1;
            int nx2 = nxt + 1 == 3 ? 0 : nxt + 1;
            const float* Wb = lds_w + cur * kWinoLdsW;
            const float* In = lds + nxt * IP3;
            // ---- first half: xi 0, 1 of this step
            f32x4 u0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0]);
            f32x4 u1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1]);
            f32x4 p0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0] + 1 * kWinoBN * 8);
            f32x4 p1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1] + 1 * kWinoBN * 8);
            __builtin_amdgcn_s_setprio(1);
            FPC_P3_MFMA8(0, u0, u1)
            __builtin_amdgcn_sched_barrier(0);
            u0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0] + 2 * kWinoBN * 8);
            u1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1] + 2 * kWinoBN * 8);
            FPC_P3_MFMA8(1, p0, p1)
            __builtin_amdgcn_sched_barrier(0);
            p0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0] + 3 * kWinoBN * 8);
            p1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1] + 3 * kWinoBN * 8);
            FPC_STAMP(0);      // first half: 16 MFMA issued
            // ---- middle: stage kb+1 (issued a whole step ago) must have landed; everyone is past step kb-1,
            //      so stage (kb+2)%3 — read last in step kb-1 — may be refilled
            if (kb + 1 < nkb) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            FPC_STAMP(1);      // wait for this wave's DMA pieces
            __builtin_amdgcn_s_barrier();
            FPC_STAMP(2);      // barrier
            if (kb + 2 < nkb) FPC_P3_ISSUE(kb + 2, nx2);
            // ---- second half: xi 2, 3, with the NEXT step's input fragments read and transformed in between
            f32x4 da[4], db[4], e[4];
            const bool more = kb + 1 < nkb;
            if (more) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    da[c] = *reinterpret_cast<const f32x4*>(In + in_a + c * kWinoIS);
                    db[c] = *reinterpret_cast<const f32x4*>(In + in_b + c * kWinoIS);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            FPC_P3_MFMA8(2, u0, u1)
            __builtin_amdgcn_sched_barrier(0);
            f32x4 w0 = v[0], w1 = v[1], w2 = v[2];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[3][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[3][q], p0[q], acc[3][0], 0, 0, 0);
                acc[3][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[3][q], p1[q], acc[3][1], 0, 0, 0);
                if (more) {      // 8 vector instructions in the shadow of this MFMA pair
                    if (q == 0) { e[0] = __builtin_elementwise_fma(sg4, db[0], da[0]); e[1] = __builtin_elementwise_fma(sg4, db[1], da[1]); }
                    if (q == 1) { e[2] = __builtin_elementwise_fma(sg4, db[2], da[2]); e[3] = __builtin_elementwise_fma(sg4, db[3], da[3]); }
                    if (q == 2) { w0 = sub_pk(e[0], e[2]); w1 = e[1] + e[2]; }
                    if (q == 3) { w2 = sub_pk(e[2], e[1]); }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_s_setprio(0);
            if (more) { v[3] = sub_pk(e[1], e[3]); v[0] = w0; v[1] = w1; v[2] = w2; }
            FPC_STAMP(3);      // DMA issue + second half (16 MFMA + next step's fragments)
            cur = nxt;
        }
        if (dbg && lane == 0) {
            long long* o = a.dbg + ((size_t)blockIdx.x * NW + wv) * 8;
            o[0] = stamp[0]; o[1] = stamp[1] + stamp[2]; o[2] = stamp[3];
            o[3] = clock64() - c_begin; o[4] = wall_clock64() - r_begin; o[5] = nkb; o[6] = c_begin - t_entry;
        }
#undef FPC_STAMP
#undef FPC_P3_ISSUE
#undef FPC_P3_MFMA8
    } else {
    // ---- barrier form.  Both operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no
    // ds_write).  Weights: the K-step image (32 KB, already in its LDS layout), every wave moves 32/NW
    // pieces of 1 KB; the four pieces of a group share ONE address register pair and ONE M0 value and differ
    // in the instruction's immediate offset, which the hardware adds to the global AND to the LDS address
    // (measured: tools_dev/glds_offset.hip).  Input: the staged region as 1 KB pieces of 32 positions,
    // out-of-image positions read the zero page.  The K loop is unrolled by two so that every LDS address
    // of a step is register + immediate.  Per K-step this leaves ~8 address instructions beside the
    // transform's 16 packed ones (the register-staged form had ~60, and a wave's vector instructions crawl
    // while its SIMD partner issues MFMAs — see the P3 comment above).
    constexpr int NPIECE = 32 / NW, NG = NPIECE / 4;
    const int swv = __builtin_amdgcn_readfirstlane(wv);
    float* const lds_w = lds + 2 * LINP;
    // Staging addresses are SGPR base + 32-bit VGPR offset: beside a SIMD partner that issues MFMAs back to
    // back, a global_load* with a 64-bit VGPR address waits like a vector-ALU instruction (one per MFMA; a pure
    // MFMA partner starves it: 1550 cycles against 12 for the SGPR-base form — tools_dev/dma_vs_mfma.hip).
    // The bases advance on the scalar unit, the lane offsets never change: no vector instruction per K-step.
    const float* wsb = P.w + (size_t)nb * nkb * kWB + swv * NPIECE * 256;           // wave-uniform: this wave's pieces of step 0
    // BF3: the {b3} image's 16 pieces.  FPC_WINO_B3_OLDER: all of them go to the older half (waves 0-3, four each) — in the
    // staggered loop the younger half's staging burst + matrix block is the longer chain (stamps: 1093 + 1797 cycles against
    // 659 + 1668), so the older half takes 10-11 of a step's pieces and the younger 6-7 instead of 8-9 each.
    const float* wsb3 = P.w + (size_t)nb * nkb * kWB + 8192 + (FPC_WINO_B3_OLDER ? (swv & 3) * 1024 : swv * 512);
    const float* isb = P.in + (size_t)b * HW * Cin;                                // image base, + 8 floats per step
    const unsigned wvo = 16u * lane;                                               // bytes
    unsigned ivo[NIN];
    bool iok[NIN];
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
        int ry, rx, hf;
        bool inreg;
        if constexpr (PERM) {
            const int slot = (swv + IST * i) * 64 + lane;             // 16-byte unit this lane's DMA data lands in
            const int blk = slot >> 4, res = slot & 15, g = blk >> 3;
            const int ah = (g / 3) * 4 + (res & 3), qh = (g % 3) * 4 + (res >> 2);
            hf = blk & 1;
            ry = 2 * ah + ((blk >> 2) & 1); rx = 2 * qh + ((blk >> 1) & 1);
            inreg = swv + IST * i < NPI && ah <= 8 && qh <= 8 && (!INO || swv < 4);
        } else {
            const int q = (swv + NW * i) * 32 + (lane >> 1);          // LDS position of this lane's 16 bytes
            hf = lane & 1;
            ry = q / kWinoRW; rx = q - ry * kWinoRW;
            inreg = q < POS && (i == 0 || swv + NW < NPI);
        }
        int y = y_in0 + ry, x = x_in0 + rx;
        iok[i] = inreg && y >= 0 && y < H && x >= 0 && x < W;
        ivo[i] = iok[i] ? (unsigned)((((size_t)y * W + x) * Cin + 4 * hf) * sizeof(float)) : 0u;
    }
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define FPC_LDS_ADDR(PTR) ((unsigned)(size_t)(__attribute__((address_space(3))) void*)(PTR))
    // weights of one K-step -> weight buffer BUF: four 1 KB pieces per group share base, offset register and M0
    // (the immediate offset moves the global AND the LDS address, tools_dev/glds_offset.hip)
#define FPC_WB_ISSUE_W(BUF)                                                                                   \
    do {                                                                                                      \
        _Pragma("unroll") for (int g = 0; g < NG; ++g)                                                        \
            asm volatile("s_mov_b32 m0, %0\n s_nop 0\n"                                                       \
                         "global_load_lds_dwordx4 %1, %2\n global_load_lds_dwordx4 %1, %2 offset:1024\n"      \
                         "global_load_lds_dwordx4 %1, %2 offset:2048\n global_load_lds_dwordx4 %1, %2 offset:3072\n" \
                         :: "s"(FPC_LDS_ADDR(lds_w + (BUF) * kWB + (swv * NPIECE + 4 * g) * 256)), "v"(wvo),       \
                            "s"(wsb + 1024 * g) : "memory", "m0");                                            \
        if constexpr (BF3 && !FPC_WINO_B3_OLDER)                                                              \
            asm volatile("s_mov_b32 m0, %0\n s_nop 0\n"                                                       \
                         "global_load_lds_dwordx4 %1, %2\n global_load_lds_dwordx4 %1, %2 offset:1024\n"      \
                         :: "s"(FPC_LDS_ADDR(lds_w + (BUF) * kWB + 8192 + swv * 512)), "v"(wvo), "s"(wsb3) : "memory", "m0"); \
        if constexpr (BF3 && FPC_WINO_B3_OLDER)                                                               \
            if (swv < 4)                                                                                      \
                asm volatile("s_mov_b32 m0, %0\n s_nop 0\n"                                                   \
                             "global_load_lds_dwordx4 %1, %2\n global_load_lds_dwordx4 %1, %2 offset:1024\n"  \
                             "global_load_lds_dwordx4 %1, %2 offset:2048\n global_load_lds_dwordx4 %1, %2 offset:3072\n" \
                             :: "s"(FPC_LDS_ADDR(lds_w + (BUF) * kWB + 8192 + swv * 1024)), "v"(wvo), "s"(wsb3) : "memory", "m0"); \
    } while (0)
    // input region of one K-step -> input buffer BUF (in-image lanes only)
#define FPC_WB_ISSUE_IN(BUF)                                                                                  \
    do {                                                                                                      \
        _Pragma("unroll") for (int i_ = 0; i_ < NIN; ++i_)                                                    \
            if (iok[i_]) asm volatile("s_mov_b32 m0, %0\n s_nop 0\n global_load_lds_dwordx4 %1, %2\n"         \
                                      :: "s"(FPC_LDS_ADDR(lds + (BUF) * LINP + (swv + IST * i_) * 256)), "v"(ivo[i_]), "s"(isb) : "memory", "m0"); \
    } while (0)

    // ---- fragment addressing
    const int tyl = (li >> 3) + 4 * half, txl = li & 7;        // this lane's tile inside the patch
    // row pair (ra, rb) and sign of B^T row wi:  0: d0-d2   1: d1+d2   2: d2-d1   3: d1-d3
    const int ra = (wi == 0) ? 0 : (wi == 2 ? 2 : 1);
    const int rb = (wi == 0) ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
    // float offsets of the four positions (2 * txl + c, c = 0..3) of region rows 2 * tyl + ra / rb: [c >> 1] + (c & 1) * in_cs
    int in_a[2], in_b[2];
    constexpr int in_cs = PERM ? 2 * 16 * 4 : kWinoIS;
    if constexpr (PERM) {
        auto unit = [&](int r, int ch) {      // row 2 * tyl + r, column 2 * (txl + ch)
            const int ah = tyl + (r >> 1), qh = txl + ch;
            return ((((ah >> 2) * 3 + (qh >> 2)) * 8 + (r & 1) * 4 + lh) * 16 + 4 * (qh & 3) + (ah & 3)) * 4;
        };
        in_a[0] = unit(ra, 0); in_a[1] = unit(ra, 1); in_b[0] = unit(rb, 0); in_b[1] = unit(rb, 1);
    } else {
        in_a[0] = ((2 * tyl + ra) * kWinoRW + 2 * txl) * kWinoIS + 4 * lh; in_a[1] = in_a[0] + 2 * kWinoIS;
        in_b[0] = ((2 * tyl + rb) * kWinoRW + 2 * txl) * kWinoIS + 4 * lh; in_b[1] = in_b[0] + 2 * kWinoIS;
    }
    int w_frag[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        int co = nt * 32 + li;
        w_frag[nt] = ((4 * wi) * kWinoBN + co) * 8 + 4 * (lh ^ ((co >> 3) & 1));   // halves swapped on odd 8-channel groups (k_wino_pack)
    }
    const f32x4 sg4 = {sgn, sgn, sgn, sgn};

    // Software pipeline (measured on this kernel with s_memtime stamps, tools_dev/wino_stamps.py):
    //  * a burst of LDS-DMA issues holds a wave ~1500 cycles per K-step (the CU's L2 -> LDS path moves ~62 B/clk
    //    whatever the instruction form, tools_dev/dma_rate.hip) and costs as much when the instructions are
    //    spread between the wave's MFMAs (~100 cycles each there) — so the burst stays a phase of its own,
    //    beside the SIMD partner's MFMA phase;
    //  * vector ALU instructions of a wave whose partner issues MFMAs back to back advance one per MFMA
    //    (~64 cycles each), but cost 2-4 cycles between the wave's OWN MFMAs — so the input transform of step
    //    k+1 (8 LDS reads, 16 packed instructions) runs inside step k's MFMA block.
    // Step k therefore: [DMA: weights k+1 -> W[cur^1], input k+2 -> I[cur]] [32 MFMAs of step k on v and
    // W[cur], with the fragments of step k+1 read from I[cur^1] and transformed in between] [wait, barrier].
    // Input k+2 may overwrite I[cur]: step k's fragments were read from it during step k-1.  The body has no
    // branch: past the last step the sources stop advancing, so the final steps stage (and transform) the
    // last step's operands once more into buffers nobody reads.
    FPC_WB_ISSUE_W(0);      // (the weight buffers are not touched by the zero fill below: the first 48 KB are on their way meanwhile)
    // out-of-image positions are never written by the DMA (inactive lanes): a patch that reaches over the image border zeroes
    // both input buffers once.  An interior patch (workgroup-uniform) skips the fill and its barrier: every position the
    // fragment reads touch is rewritten by every step's DMA (the permuted image's padding units are never read).
    if (y_in0 < 0 || x_in0 < 0 || y_in0 + RH > H || x_in0 + kWinoRW > W) {
        for (int i = t; i < 2 * LINP / 4; i += 64 * NW) reinterpret_cast<f32x4*>(lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }
    FPC_WB_ISSUE_IN(0);
    if (nkb > 1) { wsb += kWB; wsb3 += kWB; isb += 8; }
    FPC_WB_ISSUE_IN(1);
    if (nkb > 2) isb += 8;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    f32x4 v[4];      // transformed input fragments of the current step: lanes 0-31 carry ci = q, lanes 32-63 ci = 4 + q
    {
        f32x4 e[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            e[c] = __builtin_elementwise_fma(sg4, *reinterpret_cast<const f32x4*>(lds + in_b[c >> 1] + (c & 1) * in_cs),
                                             *reinterpret_cast<const f32x4*>(lds + in_a[c >> 1] + (c & 1) * in_cs));
        v[0] = sub_pk(e[0], e[2]); v[1] = e[1] + e[2]; v[2] = sub_pk(e[2], e[1]); v[3] = sub_pk(e[1], e[3]);
    }
    // BF3: the three bf16 pieces of the transformed fragments (four channels per piece and xi), and the {b3} fragment offsets
    u32x2 pa[4][3];
    int w3_frag[2];
    int w_fragh[2] = {w_frag[0], w_frag[1]};      // BF3: the same offsets, opaque (see the operand tuples in the K loop)
    if constexpr (BF3) {
#pragma unroll
        for (int j = 0; j < 4; ++j) split_bf3(v[j], pa[j][0], pa[j][1], pa[j][2]);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            int co = nt * 32 + li;
            w3_frag[nt] = 8192 + ((4 * wi) * kWinoBN + co) * 4 + 2 * (lh ^ ((co >> 4) & 1));      // halves swapped per 16 channels (k_wino_pack_bf3)
        }
        // opaque copies: no forwarding from the 16-byte reads, and no pairing of the two {b3} reads into one
        // ds_read2 (its results would sit in adjacent registers and have to be moved into their operand tuples)
        asm volatile("" : "+v"(w_fragh[0]), "+v"(w_fragh[1]), "+v"(w3_frag[1]));
    }
    __syncthreads();       // I[0] is refilled by step 0's DMA
    long long stamp[6] = {0, 0, 0, 0, 0, 0};
    const bool dbg = DBG && a.dbg != nullptr;
#define FPC_STAMP(I) do { if (DBG && dbg) { long long now_ = clock64(); stamp[I] += now_ - tprev; tprev = now_; } } while (0)
    long long tprev = dbg ? clock64() : 0;
    const long long c_begin = tprev, r_begin = dbg ? wall_clock64() : 0;
    int cur = 0;
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
        // BF3, stagger (FPC_WINO_STAGGER): SIMD partners are waves w and w + 4.  The younger half stages first and computes
        // second, the older half computes first and stages afterwards, so that on every SIMD one wave's matrix block runs
        // beside the other's staging burst instead of both doing the same phase in lockstep.  Same buffers, same hazards:
        // W[cur ^ 1] and I[cur] were last read in step kb - 1, whichever half writes them in step kb.
        const bool stage_first = !(BF3 && FPC_WINO_STAGGER) || swv >= 4;
        if (stage_first) {
            FPC_WB_ISSUE_W(cur ^ 1);
            FPC_WB_ISSUE_IN(cur);
        }
        FPC_STAMP(0);      // issue of the staging loads
        const float* In = lds + (cur ^ 1) * LINP;
        const float* Wb = lds_w + cur * kWB;
        f32x4 da[4], db[4], e[4], vn[4];
        // MFMA issue ahead of the co-resident workgroup's staging.  BF3 (one workgroup per CU): the SIMD partners are waves w
        // and w + 4 of this workgroup, and the younger one (w + 4) loses the arbitration in the staging phase AND here
        // (stamps: 1520 + 1900 cycles per K-step against 1000 + 1500, the older waves then wait 1200 at the barrier) —
        // FPC_WINO_PRIO_HI for the younger half in this block evens the two out.
        if (BF3 && swv >= 4) __builtin_amdgcn_s_setprio(FPC_WINO_PRIO_HI);
        else __builtin_amdgcn_s_setprio(1);
        if constexpr (BF3) {
            // Operand tuples without register moves: {b1, b2} is one 16-byte read; {b3, b1} is built from two 8-byte reads
            // that land in the two halves of one register tuple (the b1 half read again through an offset the compiler cannot
            // see through, or it would forward the 16-byte read and copy) — 8 LDS instructions more, 32 vector instructions fewer per K-step
            // of a wave, in a block that is bound by vector issue (190 vector instructions beside 24 matrix instructions).
            u32x4 u0 = *reinterpret_cast<const u32x4*>(Wb + w_frag[0]), u1 = *reinterpret_cast<const u32x4*>(Wb + w_frag[1]);
            u32x2 t0 = *reinterpret_cast<const u32x2*>(Wb + w3_frag[0]), t1 = *reinterpret_cast<const u32x2*>(Wb + w3_frag[1]);
            u32x2 h0 = *reinterpret_cast<const u32x2*>(Wb + w_fragh[0]), h1 = *reinterpret_cast<const u32x2*>(Wb + w_fragh[1]);
            asm volatile("" ::: "memory");      // keeps these reads from being paired (ds_read2) with xi 1's: paired results sit in adjacent registers
            u32x2 pn[4][3];
#define FPC_WINO_BF3_MFMA(A, B0, B1)                                                                               \
    do {                                                                                                      \
        acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B0), acc[j][0], 0, 0, 0); \
        acc[j][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B1), acc[j][1], 0, 0, 0); \
    } while (0)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u32x4 n0 = u0, n1 = u1;
                u32x2 m0 = t0, m1 = t1, g0 = h0, g1 = h1;
                if (j < 3) {
                    n0 = *reinterpret_cast<const u32x4*>(Wb + w_frag[0] + (j + 1) * kWinoBN * 8);
                    n1 = *reinterpret_cast<const u32x4*>(Wb + w_frag[1] + (j + 1) * kWinoBN * 8);
                    m0 = *reinterpret_cast<const u32x2*>(Wb + w3_frag[0] + (j + 1) * kWinoBN * 4);
                    m1 = *reinterpret_cast<const u32x2*>(Wb + w3_frag[1] + (j + 1) * kWinoBN * 4);
                    g0 = *reinterpret_cast<const u32x2*>(Wb + w_fragh[0] + (j + 1) * kWinoBN * 8);
                    g1 = *reinterpret_cast<const u32x2*>(Wb + w_fragh[1] + (j + 1) * kWinoBN * 8);
                }
                if (j < 2) {
#pragma unroll
                    for (int c = 2 * j; c < 2 * j + 2; ++c) {
                        da[c] = *reinterpret_cast<const f32x4*>(In + in_a[c >> 1] + (c & 1) * in_cs);
                        db[c] = *reinterpret_cast<const f32x4*>(In + in_b[c >> 1] + (c & 1) * in_cs);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                const u32x4 A0 = {pa[j][0][0], pa[j][0][1], pa[j][0][0], pa[j][0][1]};
                const u32x4 A1 = {pa[j][1][0], pa[j][1][1], pa[j][1][0], pa[j][1][1]};
                const u32x4 A2 = {pa[j][0][0], pa[j][0][1], pa[j][2][0], pa[j][2][1]};
                const u32x4 C0 = {t0[0], t0[1], h0[0], h0[1]}, C1 = {t1[0], t1[1], h1[0], h1[1]};
                FPC_WINO_BF3_MFMA(A0, u0, u1);      // a1 b1 + a1 b2
                // the next step's fragments in the shadow of this wave's own MFMAs: transform at xi 0 / 1, split at xi 2 / 3
                if (j == 0) { e[0] = fma_s4(sgn, db[0], da[0]); e[1] = fma_s4(sgn, db[1], da[1]); }
                if (j == 1) { e[2] = fma_s4(sgn, db[2], da[2]); e[3] = fma_s4(sgn, db[3], da[3]); }
                if (j == 2) split_bf3(vn[0], pn[0][0], pn[0][1], pn[0][2]);
                if (j == 3) split_bf3(vn[2], pn[2][0], pn[2][1], pn[2][2]);
                __builtin_amdgcn_sched_barrier(0);
                FPC_WINO_BF3_MFMA(A1, u0, u1);      // a2 b1 + a2 b2
                if (j == 1) { vn[0] = sub_s4(e[0], e[2]); vn[1] = add_s4(e[1], e[2]); }
                if (j == 2) split_bf3(vn[1], pn[1][0], pn[1][1], pn[1][2]);
                if (j == 3) split_bf3(vn[3], pn[3][0], pn[3][1], pn[3][2]);
                __builtin_amdgcn_sched_barrier(0);
                FPC_WINO_BF3_MFMA(A2, C0, C1);      // a1 b3 + a3 b1
                if (j == 1) { vn[2] = sub_s4(e[2], e[1]); vn[3] = sub_s4(e[1], e[3]); }
                __builtin_amdgcn_sched_barrier(0);
                u0 = n0; u1 = n1; t0 = m0; t1 = m1; h0 = g0; h1 = g1;
                // stagger: the compute-first half stages after xi FPC_WINO_LATE_AT of its matrix block (3 = after the block): the
                // pieces land while the rest of the block runs (3415 -> 3170 cycles per K-step against staging after the block, 3123
                // after xi 0 once the older half also carries the {b3} pieces; the stage-first half staging inside its block as
                // well: 3500-4100)
                if (j == FPC_WINO_LATE_AT && FPC_WINO_LATE_AT < 3 && !stage_first) {
                    FPC_WB_ISSUE_W(cur ^ 1);
                    FPC_WB_ISSUE_IN(cur);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#undef FPC_WINO_BF3_MFMA
            __builtin_amdgcn_s_setprio(0);
#pragma unroll
            for (int j = 0; j < 4; ++j) { pa[j][0] = pn[j][0]; pa[j][1] = pn[j][1]; pa[j][2] = pn[j][2]; }
        } else {
        f32x4 u0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0]);
        f32x4 u1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // weight fragments of xi j+1 are requested before xi j's MFMAs (LDS latency behind 8 MFMAs)
            f32x4 n0 = u0, n1 = u1;
            if (j < 3) {
                n0 = *reinterpret_cast<const f32x4*>(Wb + w_frag[0] + (j + 1) * kWinoBN * 8);
                n1 = *reinterpret_cast<const f32x4*>(Wb + w_frag[1] + (j + 1) * kWinoBN * 8);
            }
            if (j < 2) {                    // raw fragments of the next step, two channel pairs per xi block
#pragma unroll
                for (int c = 2 * j; c < 2 * j + 2; ++c) {
                    da[c] = *reinterpret_cast<const f32x4*>(In + in_a[c >> 1] + (c & 1) * in_cs);
                    db[c] = *reinterpret_cast<const f32x4*>(In + in_b[c >> 1] + (c & 1) * in_cs);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[j][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][q], u0[q], acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v[j][q], u1[q], acc[j][1], 0, 0, 0);
                // 2 packed instructions in the shadow of this MFMA pair
                if (j < 2 && q >= 2) e[2 * j + q - 2] = __builtin_elementwise_fma(sg4, db[2 * j + q - 2], da[2 * j + q - 2]);
                if (j == 2 && q == 0) vn[0] = sub_pk(e[0], e[2]);
                if (j == 2 && q == 1) vn[1] = e[1] + e[2];
                if (j == 2 && q == 2) vn[2] = sub_pk(e[2], e[1]);
                if (j == 2 && q == 3) vn[3] = sub_pk(e[1], e[3]);
                __builtin_amdgcn_sched_barrier(0);
            }
            u0 = n0; u1 = n1;
        }
        __builtin_amdgcn_s_setprio(0);
        v[0] = vn[0]; v[1] = vn[1]; v[2] = vn[2]; v[3] = vn[3];
        }
        FPC_STAMP(2);      // MFMA issue + the next step's fragments (not completion)
        if (!stage_first && !(BF3 && FPC_WINO_LATE_AT < 3)) {
            FPC_WB_ISSUE_W(cur ^ 1);
            FPC_WB_ISSUE_IN(cur);
        }
        wsb += kb + 2 < nkb ? kWB : 0;
        wsb3 += kb + 2 < nkb ? kWB : 0;
        isb += kb + 3 < nkb ? 8 : 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's DMA pieces have landed
        FPC_STAMP(3);
        __syncthreads();                                      // everybody's have; this step's reads are done
        FPC_STAMP(4);      // barrier
        cur ^= 1;
    }
    if (dbg && lane == 0) {
        long long* o = a.dbg + ((size_t)blockIdx.x * NW + wv) * 8;
        o[0] = stamp[0]; o[1] = stamp[3] + stamp[4]; o[2] = stamp[2];      // issue of the staging loads | wait + barrier | MFMA block
        o[3] = clock64() - c_begin;            // shader-clock ticks of the whole K loop
        o[6] = c_begin - t_entry;              // kernel entry -> K loop
        o[4] = wall_clock64() - r_begin;       // 100 MHz reference ticks of the same span
        o[5] = nkb;
    }
#undef FPC_STAMP
#undef FPC_WB_ISSUE_W
#undef FPC_WB_ISSUE_IN
#undef FPC_LDS_ADDR
#pragma clang diagnostic pop

    }

    const long long t_kend = DBG ? clock64() : 0;
    // ---- output transform.  Column part inside the wave: z0 = m0 + m1 + m2, z1 = m1 - m2 - m3;
    // row part across the four transform-row waves through LDS: y0 = z[0] + z[1] + z[2], y1 = z[1] - z[2] - z[3].
    // LDS image Z[row i][cc][tile NT][co 32], one 32-channel half (nt) at a time.
    const int ot = t >> 3, oc4 = (t & 7) * 4;                 // output stage: thread = one tile x 4 channels
    const int oty = ty0 + (ot >> 3), otx = tx0 + (ot & 7);
    // The epilogue's own global reads — folded-BatchNorm scale / shift and the residual of this thread's 2 x 2 outputs, for both
    // 32-channel halves — are requested BEFORE the first barrier of the output transform: behind it they were issued after the
    // second barrier of each half and their latency stood exposed twice per workgroup (one workgroup per CU: nothing overlaps it;
    // a residual convolution of ResNet-34's layer1 took 266 us against 205 us without residual at batch 32).
    f32x4 e_sc[2], e_sh[2], e_res[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const int n = nb * kWinoBN + nt * 32 + oc4;
        e_sc[nt] = P.scale ? *reinterpret_cast<const f32x4*>(P.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
        e_sh[nt] = P.shift ? *reinterpret_cast<const f32x4*>(P.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int y = 2 * oty + (q >> 1), x = 2 * otx + (q & 1);
            e_res[nt][q] = (P.res && y < H && x < W) ? *reinterpret_cast<const f32x4*>(P.res + ((size_t)b * HW + (size_t)y * W + x) * Cout + n)
                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int m = half * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            float m0 = acc[0][nt][r], m1 = acc[1][nt][r], m2 = acc[2][nt][r], m3 = acc[3][nt][r];
            lds[((wi * 2 + 0) * NT + m) * 32 + li] = m0 + m1 + m2;
            lds[((wi * 2 + 1) * NT + m) * 32 + li] = m1 - m2 - m3;
        }
        __syncthreads();
        const int n = nb * kWinoBN + nt * 32 + oc4;
        f32x4 z[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) z[i][cc] = *reinterpret_cast<const f32x4*>(lds + ((i * 2 + cc) * NT + ot) * 32 + oc4);
        const f32x4 sc = e_sc[nt], sh = e_sh[nt];
        f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                int y = 2 * oty + rr, x = 2 * otx + cc;
                if (y >= H || x >= W) continue;
                f32x4 val = rr == 0 ? z[0][cc] + z[1][cc] + z[2][cc] : z[1][cc] - z[2][cc] - z[3][cc];
                if (P.scale) val = val * sc;
                val = val + sh;
                size_t o = ((size_t)b * HW + (size_t)y * W + x) * Cout + n;
                if (P.res) val += e_res[nt][2 * rr + cc];
                if (a.relu) { val[0] = fmaxf(val[0], 0.f); val[1] = fmaxf(val[1], 0.f); val[2] = fmaxf(val[2], 0.f); val[3] = fmaxf(val[3], 0.f); }
                *reinterpret_cast<f32x4*>(P.out + o) = val;
                s1 += val;
                s2 += val * val;
            }
        if (P.gn_part) {
            // per-channel sums of this workgroup's outputs.  A wave holds 8 tiles (lane bits 3-5) of 8 channel quads
            // (lane bits 0-2): butterfly over the tile bits, then the NW waves' sums through LDS in wave order
            // (a serial walk of the NT tile slots by 32 threads cost ~4000 cycles per 32-channel half).
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { s1[k] += __shfl_xor(s1[k], o, 64); s2[k] += __shfl_xor(s2[k], o, 64); }
            }
            __syncthreads();
            float* red = lds;                                  // [NW waves][32 ch][2]
            if (lane < 8) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { red[(wv * 32 + oc4 + k) * 2] = s1[k]; red[(wv * 32 + oc4 + k) * 2 + 1] = s2[k]; }
            }
            __syncthreads();
            if (t < 32) {
                float u1 = 0.f, u2 = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) { u1 += red[(w * 32 + t) * 2]; u2 += red[(w * 32 + t) * 2 + 1]; }
                int Pn = a.tbx * a.tby;
                float* g = P.gn_part + (((size_t)b * Pn + by * a.tbx + bx) * Cout + nb * kWinoBN + nt * 32 + t) * 2;
                g[0] = u1; g[1] = u2;
            }
        }
    }
    if (DBG && a.dbg != nullptr && lane == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        a.dbg[((size_t)blockIdx.x * NW + wv) * 8 + 7] = clock64() - t_kend;      // K loop end -> last store acknowledged
    }
}

// OIHW 3x3 weights -> U = G g G^T, packed [Cout/64][Cin/8][16 xi][64 co][8 ci] (one K-step image = 32 KB)
__global__ __launch_bounds__(256) void k_wino_pack(const float* __restrict__ w, float* __restrict__ out, int Cout,
                                                   int Cin) {
    long long total = (long long)Cout * Cin;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int ci = (int)(g % Cin), co = (int)(g / Cin);
        const float* k = w + ((size_t)co * Cin + ci) * 9;
        float gg[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float g0 = k[c], g1 = k[3 + c], g2 = k[6 + c];
            gg[0][c] = g0;
            gg[1][c] = 0.5f * (g0 + g1 + g2);
            gg[2][c] = 0.5f * (g0 - g1 + g2);
            gg[3][c] = g2;
        }
        int nb = co >> 6, col = co & 63, kb = ci >> 3, cil = ci & 7;
        // the step image IS the LDS image: halves (4 channels) swapped on odd 8-channel groups
        float* dst = out + (((size_t)nb * (Cin >> 3) + kb) * 16) * 512 + col * 8 + (cil ^ (4 * ((col >> 3) & 1)));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float r0 = gg[i][0], r1 = gg[i][1], r2 = gg[i][2];
            dst[(4 * i + 0) * 512] = r0;
            dst[(4 * i + 1) * 512] = 0.5f * (r0 + r1 + r2);
            dst[(4 * i + 2) * 512] = 0.5f * (r0 - r1 + r2);
            dst[(4 * i + 3) * 512] = r2;
        }
    }
}

// The same U, every value split exactly into three bf16 pieces (truncation split, as split_bf3), packed per K-step as
// [Cout/64][Cin/8][ 16 xi x 64 co x {half slot: b1 x 4 ch, b2 x 4 ch} (32 KB, the f32 image's addressing) | 16 xi x 64 co x
// {half slot: b3 x 4 ch} (16 KB) ]; half slots swapped on odd 8-channel (main) / 16-channel ({b3}) groups of co.
__global__ __launch_bounds__(256) void k_wino_pack_bf3(const float* __restrict__ w, unsigned short* __restrict__ out, int Cout,
                                                       int Cin) {
    long long total = (long long)Cout * Cin;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        int ci = (int)(g % Cin), co = (int)(g / Cin);
        const float* k = w + ((size_t)co * Cin + ci) * 9;
        float gg[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float g0 = k[c], g1 = k[3 + c], g2 = k[6 + c];
            gg[0][c] = g0;
            gg[1][c] = 0.5f * (g0 + g1 + g2);
            gg[2][c] = 0.5f * (g0 - g1 + g2);
            gg[3][c] = g2;
        }
        const int nb = co >> 6, col = co & 63, kb = ci >> 3, cil = ci & 7, hw = cil >> 2, e = cil & 3;
        unsigned short* img = out + ((size_t)nb * (Cin >> 3) + kb) * (12288 * 2);
        unsigned short* dm = img + col * 16 + 8 * (hw ^ ((col >> 3) & 1)) + e;                      // + xi * 1024;  b2 at + 4
        unsigned short* d3 = img + 8192 * 2 + col * 8 + 4 * (hw ^ ((col >> 4) & 1)) + e;            // + xi * 512
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float r0 = gg[i][0], r1 = gg[i][1], r2 = gg[i][2];
            const float u[4] = {r0, 0.5f * (r0 + r1 + r2), 0.5f * (r0 - r1 + r2), r2};
#pragma unroll
            for (int jx = 0; jx < 4; ++jx) {
                const int xi = 4 * i + jx;
                const float x = u[jx];
                const unsigned xb = __builtin_bit_cast(unsigned, x) & 0xFFFF0000u;
                const float r = x - __builtin_bit_cast(float, xb);
                const unsigned rb = __builtin_bit_cast(unsigned, r) & 0xFFFF0000u;
                const float q = r - __builtin_bit_cast(float, rb);
                dm[xi * 1024] = (unsigned short)(xb >> 16);
                dm[xi * 1024 + 4] = (unsigned short)(rb >> 16);
                d3[xi * 512] = (unsigned short)(__builtin_bit_cast(unsigned, q) >> 16);
            }
        }
    }
}

// 256 bytes of zeros that live in the code object (zero-initialised at load, never written): the zero page of the all-DMA and
// split-precision Winograd forms for callers that have no plan workspace (fpc_conv2d: one memset per call before)
__device__ __attribute__((aligned(256))) float g_fpc_zero_page[64];
const float* zero_page() {      // looked up per call: the address belongs to the CURRENT device
    void* q = nullptr;
    return hipGetSymbolAddress(&q, HIP_SYMBOL(g_fpc_zero_page)) == hipSuccess ? static_cast<const float*>(q) : nullptr;
}

int launch_conv_wino(const WinoArgs& a, int groups, hipStream_t s) {
    if (groups < 1 || groups > kMaxGroup || a.Cin % 8 != 0 || a.Cout % kWinoBN != 0 || (a.waves != 4 && a.waves != 8))
        return FPC_EINVAL;
    dim3 grid(a.tbx * a.tby * a.B * (a.Cout / kWinoBN) * groups);
    if (a.variant != 1 && !a.zeros) return FPC_EINVAL;
    if (!kWinoStamp && a.dbg) return FPC_EINVAL;
    if ((long long)a.H * a.W * a.Cin * (long long)sizeof(float) >= (1LL << 32)) return FPC_EINVAL;   // 32-bit lane offsets inside one image
#ifdef FPC_STAMP_WINO      // the stamping instantiations (the wave-private form has none)
    if (a.dbg && (a.waves == 8 || a.variant != 1)) {
        if (a.waves == 8 && a.variant == 3) hipLaunchKernelGGL((k_conv_wino<8, false, false, true, true>), grid, dim3(512), 0, s, a);
        else if (a.waves == 8 && a.variant == 2) hipLaunchKernelGGL((k_conv_wino<8, false, true, true>), grid, dim3(512), 0, s, a);
        else if (a.waves == 8) hipLaunchKernelGGL((k_conv_wino<8, false, false, true>), grid, dim3(512), 0, s, a);
        else hipLaunchKernelGGL((k_conv_wino<4, false, false, true>), grid, dim3(256), 0, s, a);
        return check_launch();
    }
#endif
    if (a.waves == 8 && a.variant == 3) hipLaunchKernelGGL((k_conv_wino<8, false, false, false, true>), grid, dim3(512), 0, s, a);
    else if (a.waves == 8 && a.variant == 2) hipLaunchKernelGGL((k_conv_wino<8, false, true>), grid, dim3(512), 0, s, a);
    else if (a.waves == 8) hipLaunchKernelGGL((k_conv_wino<8, false, false>), grid, dim3(512), 0, s, a);
    else if (a.variant == 1) hipLaunchKernelGGL((k_conv_wino<4, true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_conv_wino<4, false, false>), grid, dim3(256), 0, s, a);
    return check_launch();
}

#ifdef FPC_STAMP_WINO
// present in a -DFPC_STAMP_WINO build only: how tools_dev/wino_stamps.py knows that fpc_conv2d's relu = 77 hands gn_part to the
// Winograd kernels as their stamp buffer
extern "C" int fpc_dbg_wino_diag(void) { return 1; }
#endif

int launch_wino_pack(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s) {
    if (Cin % 8 != 0 || Cout % kWinoBN != 0) return FPC_EINVAL;
    hipLaunchKernelGGL(k_wino_pack, dim3(stream_grid((long long)Cout * Cin)), dim3(256), 0, s, w_oihw, packed, Cout, Cin);
    return check_launch();
}

// split-precision image: 24 * Cout * Cin floats (every byte is written)
int launch_wino_pack_bf3(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s) {
    if (Cin % 8 != 0 || Cout % kWinoBN != 0) return FPC_EINVAL;
    hipLaunchKernelGGL(k_wino_pack_bf3, dim3(stream_grid((long long)Cout * Cin)), dim3(256), 0, s, w_oihw,
                       reinterpret_cast<unsigned short*>(packed), Cout, Cin);
    return check_launch();
}

}  // namespace fpc
