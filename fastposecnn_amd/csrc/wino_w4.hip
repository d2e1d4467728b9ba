// wino_w4.hip — k_conv_wino_w4: the split-precision Winograd F(2x2, 3x3) convolution as FOUR waves of 512 registers (round 6).
//
// k_conv_wino<8, ..., BF3> (net_kernels.hip: 8 x 8 tile patch x 64 output channels, 8 waves = 2 per SIMD, 242 registers) spends 3 270
// cycles on a K-step that holds 1 536 cycles of matrix work: per wave 153 vector instructions beside 24 matrix instructions, and a
// wave's vector instructions crawl (one per matrix instruction) whenever its SIMD partner is the one issuing matrix instructions.
// The 128-channel shape (wino128.hip) halves the vector work per product but doubles the weight bytes per product and sits on the
// L2's ~18 TB/s (96 KB per K-step and CU: 2 400 cycles).  This kernel keeps the 64-channel shape's bytes and removes the PARTNER:
//
//   * ONE wave per SIMD (256 threads, launch bound 1 -> up to 512 registers per lane): wave w owns transform row w — its 4 xi x
//     all 64 tiles (two 32-tile halves) x 64 channels (two 32-channel tiles) = 16 accumulators of 32 x 32 = 256 accumulation
//     registers; 48 v_mfma_f32_32x32x16_bf16 per K-step of 8 input channels.  Every matrix instruction is followed by ITS share
//     (one item of 4-7 vector instructions) of the step's other work and a scheduling barrier: between a wave's own matrix
//     instructions a vector instruction costs its 4 issue cycles and nothing else, and 6-7 of them fit under the 32 cycles the
//     matrix pipe is busy.
//   * weights straight into the operand registers: a weight fragment is used by two matrix instructions of ONE wave, so LDS buys
//     nothing.  The image is k_wino_pack_bf3's, unchanged — its 16-byte {b1, b2} and 8-byte {b3} slots per (xi, channel, half) are
//     contiguous per wave: a lane offset picks the slot — fetched with buffer loads one K-step ahead into the registers the last
//     matrix instruction of the fragment has just read (48 registers of weights in flight or waiting; 48 KB per K-step and CU).
//   * input: the permuted, conflict-free 18 x 18 region image of the 8-wave kernel (18 LDS-DMA pieces of 1 KB per K-step, two
//     buffers, one barrier per K-step).  The DMA instructions are inline asm: issued BEFORE the step's 16 weight loads and waited
//     for with a COUNTED vmcnt(16), so the weight prefetch stays in flight across the barrier.
//   * the next step's fragments are transformed and split IN PLACE: the three bf16 pieces of xi j's fragments are overwritten
//     once xi j's matrix instructions are done (xi 0-2 during this step's xi 2-3, xi 3 — whose transformed values wait in eight
//     registers — during the next step's xi 0-1), so only one set of pieces (48 registers) exists.
//   Products, split and accumulation order per accumulator are the 8-wave BF3 form's: results are bit-identical to it.
//   Output transform through LDS in ONE pass (Z[row 4][cc 2][tile 64][channel 64] = 128 KB), epilogue as k_conv_wino's.
// The set-up around the K loop (patch decode, staging plan, fragment addressing) and the output transform are shared with the fp16
// forms: wino_tile.hpp.
// Reference: the 3x3 / stride-1 convolutions of F/lib/pose_regressor.py:709-743 (smp encoder + FPN decoder, not vendored).
#include <algorithm>
#ifdef FPC_STAMP_WINO
#include <cstdlib>
#endif
#include "wino_tile.hpp"

namespace fpc {
using namespace wino_tile;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

namespace {
constexpr int kStepBytes = 12288 * 4;            // k_wino_pack_bf3's image of one K-step: 32 KB {b1, b2} + 16 KB {b3}
static_assert(kLdsFloats >= 2 * kInFloats, "the K loop's two input buffers live in the output image's space");
}  // namespace

// MODE (diagnostic instantiations of a -DFPC_STAMP_WINO build, FPC_W4_MODE at launch; the product is MODE 0): bit 0 = the K loop
// reloads no weights, bit 1 = it stages no input and has
// no barrier — wrong results, the same instruction stream otherwise
template <int MODE>
__global__ __launch_bounds__(256, 1) void k_conv_wino_w4(const WinoArgs a) {
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
    const int nb = pt.nb;
    const ConvPtrs P = wino_group(a.p[0], a.p[1], a.p[2], a.p[3], pt.grp);
    const int y_in0 = 2 * pt.ty0 - 1, x_in0 = 2 * pt.tx0 - 1;

    f32x16 acc[4][2][2];      // [xi column j][tile half mt][32-channel tile nt]; zeroed while the first operands are on their way
    // ---- weights: buffer loads from k_wino_pack_bf3's image.  {b1, b2} of (xi, channel co, channel half hw): 16 bytes at
    // xi * 2048 + co * 32 + 16 * (hw ^ ((co >> 3) & 1)); {b3}: 8 bytes at 32768 + xi * 1024 + co * 16 + 8 * (hw ^ ((co >> 4) & 1))
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(reinterpret_cast<const char*>(P.w) + (size_t)nb * nkb * kStepBytes);
    const int vo_u = li * 32 + 16 * (lh ^ ((li >> 3) & 1)), vo_t = li * 16 + 8 * (lh ^ ((li >> 4) & 1));
    int so_u = wi * 8192, so_t = 32768 + wi * 4096;      // this wave's four xi; + kStepBytes per K-step
    u32x4 U[4][2];
    u32x2 T[4][2];
#define FPC_W4_LOAD_U(J, NT) U[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, so_u + (J) * 2048 + (NT) * 1024, 0))
#define FPC_W4_LOAD_T(J, NT) T[J][NT] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rs_w, vo_t, so_t + (J) * 1024 + (NT) * 512, 0))
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) { FPC_W4_LOAD_U(j, nt); FPC_W4_LOAD_T(j, nt); }
    if (nkb > 1) { so_u += kStepBytes; so_t += kStepBytes; }
    // ---- input staging and fragment addressing (wino_tile.hpp)
    const float* isb = P.in + (size_t)pt.b * HW * Cin;            // image base, + 8 floats per step
    unsigned ivo[5];
    unsigned long long imask[5];
    wino_stage_plan<false>(ivo, imask, wi, lane, y_in0, x_in0, H, W, Cin, 0, pt.pk_ks, pt.pk_two);
#define FPC_W4_ISSUE_IN(BUF) wino_issue_in(lds + (BUF) * kInFloats, wi, ivo, imask, isb)
    int in_a[2], in_b[2];
    const float sgn = wino_frag<false>(in_a, in_b, wi, li, lh, pt.pk_ks);
    wino_zero_ring(lds, t, 2, y_in0, x_in0, H, W, false);
    FPC_W4_ISSUE_IN(0);
    if (nkb > 1) isb += 8;
    FPC_W4_ISSUE_IN(1);
    if (nkb > 2) isb += 8;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][mt][nt][r] = 0.f;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // pieces of the current step's transformed fragments pa[j][mt][piece] (four channels each); transformed values vn[mt][j] of the
    // step whose pieces are being built (xi 3's wait there across the loop's back edge)
    u32x2 pa[4][2][3];
    f32x4 vn[2][4];
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
            for (int j = 0; j < 3; ++j) split_bf3(vn[mt][j], pa[j][mt][0], pa[j][mt][1], pa[j][mt][2]);
        }
    }
    __syncthreads();       // buffer 0 is refilled by step 0's DMA

#define FPC_W4_MFMA(J, MT, NT, A, B) acc[J][MT][NT] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, B), acc[J][MT][NT], 0, 0, 0)
    // one item of a three-way split: element `part` of vn[MT][J] -> its two residuals; items 1 and 3 also pack the finished pair
// (Items are PINNED to their slot: plain arithmetic has no ordering against __builtin_amdgcn_sched_barrier before instruction
// selection, and the compiler gathered 44 instructions of two splits into one slot.  An empty volatile asm that READS an item's
// results at its end is ordered against the barriers: the item cannot sink below its slot.  Input-only on purpose: an asm with
// outputs in front of the item's first instruction drew a hazard s_nop — 4 issue cycles — per item.)
#define FPC_W4_SPLIT_ITEM(J, MT, PART)                                                                        \
    do {                                                                                                      \
        const float x_ = vn[MT][J][PART];                                                                     \
        const unsigned xb_ = __builtin_bit_cast(unsigned, x_) & 0xFFFF0000u;                                  \
        const float r_ = x_ - __builtin_bit_cast(float, xb_);                                                 \
        const unsigned rb_ = __builtin_bit_cast(unsigned, r_) & 0xFFFF0000u;                                  \
        const float q_ = r_ - __builtin_bit_cast(float, rb_);                                                 \
        if ((PART) & 1) {                                                                                     \
            const unsigned k1_ = pack_hi16(sx[(PART) - 1], x_), k2_ = pack_hi16(sr[(PART) - 1], r_), k3_ = pack_hi16(sq[(PART) - 1], q_); \
            asm volatile("" :: "v"(k1_), "v"(k2_), "v"(k3_));                                                 \
            pa[J][MT][0][(PART) >> 1] = k1_; pa[J][MT][1][(PART) >> 1] = k2_; pa[J][MT][2][(PART) >> 1] = k3_; \
        } else {                                                                                              \
            asm volatile("" :: "v"(r_), "v"(q_));                                                             \
            sx[PART] = x_; sr[PART] = r_; sq[PART] = q_;                                                      \
        }                                                                                                     \
    } while (0)
#define FPC_W4_PIN4(V) asm volatile("" :: "v"(V))
    u32x4 Atup = {pa[0][0][0][0], pa[0][0][0][1], pa[0][0][0][0], pa[0][0][0][1]};      // operand of the first pair of slots (xi 0, a1 b1 + a1 b2, half 0)
    int cur = 0;
    const long long c_begin = dbg ? clock64() : 0, r_begin = dbg ? wall_clock64() : 0;
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
        // input of step kb + 2 -> the buffer step kb's fragments were read from during step kb - 1 (oldest in the queue: see the wait below)
        if (!(MODE & 2) && !(MODE & 8)) FPC_W4_ISSUE_IN(cur);
        const float* In = lds + (cur ^ 1) * kInFloats;
        f32x4 da[2][4], db[2][4], e[2][4];
        float sx[4], sr[4], sq[4];
        __builtin_amdgcn_s_setprio(1);
        // Slot sl = 12 j + 4 g + 2 mt + nt: g = 0: a1 b1 + a1 b2, g = 1: a2 b1 + a2 b2, g = 2: a1 b3 + a3 b1.  One item per slot:
        //   sl  0- 3  fragment reads of step kb + 1 (two columns of one tile half each) + split of THIS step's xi 3, half 0
        //   sl  4-11  row transform e = da + sgn db (one column of one half each)
        //   sl 12-15  split of this step's xi 3, half 1      sl 16-23  column transform vn (one xi of one half each)
        //   sl 24-35  split of step kb + 1's xi 0 (both halves), xi 1 half 0      sl 36-47  xi 1 half 1, xi 2 (both halves)
        // g = 1 slots of half 0 also build their tile's {b3, b1} operand; the last matrix instruction of a weight fragment (g = 1, half 1 /
        // g = 2, half 1) is followed by the fragment's reload for step kb + 1.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u32x4 C[2];
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    // the A operand of this pair of slots was built (and pinned) during the previous pair's first slot: a tuple
                    // written right before the matrix instruction that reads it costs hazard s_nops (4 issue cycles each)
                    const u32x4 Ause = Atup;
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int sl = 12 * j + 4 * g + 2 * mt + nt;
                        if (g < 2) FPC_W4_MFMA(j, mt, nt, Ause, U[j][nt]);
                        if (g == 1) {
                            if (mt == 0) C[nt] = u32x4{T[j][nt][0], T[j][nt][1], U[j][nt][0], U[j][nt][1]};
                            if (mt == 1 && !(MODE & 1)) FPC_W4_LOAD_U(j, nt);
                        }
                        if (g == 2) {
                            FPC_W4_MFMA(j, mt, nt, Ause, C[nt]);
                            if (mt == 1 && !(MODE & 1)) FPC_W4_LOAD_T(j, nt);
                        }
                        if (nt == 0) {      // the next pair's operand (the loop's last pair builds the next step's first)
                            const int pr = (6 * j + 2 * g + mt + 1) % 24, nj = pr / 6, ng = (pr % 6) >> 1, nm = pr & 1;
                            const u32x2 lo = pa[nj][nm][ng == 1 ? 1 : 0], hi = pa[nj][nm][ng == 0 ? 0 : (ng == 1 ? 1 : 2)];
                            Atup = u32x4{lo[0], lo[1], hi[0], hi[1]};
                            FPC_W4_PIN4(Atup);
                        }
                        if (sl < 4) {
#pragma unroll
                            for (int c = 2 * (sl & 1); c < 2 * (sl & 1) + 2; ++c) {
                                da[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_a[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                                db[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_b[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                            }
                            FPC_W4_SPLIT_ITEM(3, 0, sl);
                        }
                        if (sl >= 4 && sl < 12) {
                            const int m_ = (sl - 4) >> 2, c = (sl - 4) & 3;
                            e[m_][c] = fma_s4(sgn, db[m_][c], da[m_][c]);
                            FPC_W4_PIN4(e[m_][c]);
                        }
                        if (sl >= 12 && sl < 16) FPC_W4_SPLIT_ITEM(3, 1, sl - 12);
                        if (sl >= 16 && sl < 24) {
                            const int m_ = (sl - 16) >> 2, jx = (sl - 16) & 3;
                            if (jx == 0) vn[m_][0] = sub_s4(e[m_][0], e[m_][2]);
                            if (jx == 1) vn[m_][1] = add_s4(e[m_][1], e[m_][2]);
                            if (jx == 2) vn[m_][2] = sub_s4(e[m_][2], e[m_][1]);
                            if (jx == 3) vn[m_][3] = sub_s4(e[m_][1], e[m_][3]);
                            FPC_W4_PIN4(vn[m_][jx]);
                        }
                        if (sl >= 24) {      // 24 items: (xi 0, half 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1) x 4 parts
                            const int q = (sl - 24) >> 2;
                            FPC_W4_SPLIT_ITEM(q >> 1, q & 1, (sl - 24) & 3);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
        }
        __builtin_amdgcn_s_setprio(0);
        so_u += kb + 2 < nkb ? kStepBytes : 0;
        so_t += kb + 2 < nkb ? kStepBytes : 0;
        isb += kb + 3 < nkb ? 8 : 0;
        // this wave's DMA pieces (issued before the step's 16 weight loads, which stay in flight) have landed
        if (!(MODE & 2)) {
            if (MODE & 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            if (!(MODE & 4)) __syncthreads();                 // everybody's have; this step's fragment reads are done
        }
        cur ^= 1;
    }
#undef FPC_W4_MFMA
#undef FPC_W4_SPLIT_ITEM
#undef FPC_W4_PIN4
#undef FPC_W4_ISSUE_IN
#undef FPC_W4_LOAD_U
#undef FPC_W4_LOAD_T
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the last steps' redundant staging has landed before LDS is reused
    const long long t_kend = dbg ? clock64() : 0;
    if (dbg && lane == 0) {      // tools_dev/wino_stamps.py: shader-clock ticks and 100 MHz reference ticks of the K loop, entry -> loop
        long long* o = dbg + ((size_t)blockIdx.x * 4 + wi) * 8;
        o[0] = 0; o[1] = 0; o[2] = 0;
        o[3] = t_kend - c_begin; o[4] = wall_clock64() - r_begin; o[5] = nkb; o[6] = c_begin - t_entry;
    }
    wino_output<false, false>(lds, acc, P, pt, WinoEpi{H, W, Cout, a.relu, a.tbx, a.tby, 0, a.exit_general}, 1.0f, nullptr, dbg, t_kend, t, wi);
}

// .w = the k_wino_pack_bf3 image (as variant 3 of launch_conv_wino), .waves = 8 (tby = ceil(ceil(H / 2) / 8): 8 x 8 tile patches)
int launch_conv_wino_w4(const WinoArgs& a_in, int groups, hipStream_t s) {
    long long nblk;
    if (const int rc = wino_tile_check(a_in, groups, 8, kStepBytes, false, &nblk)) return rc;
    WinoArgs a = a_in;      // + the reciprocals of the workgroup-id decode (wino_patch)
    a.dec = wino_decode(a.Cout, groups, a.tbx, a.tby, a.W, a.B, 0);
#ifdef FPC_STAMP_WINO
    static const int mode = getenv("FPC_W4_MODE") ? atoi(getenv("FPC_W4_MODE")) : 0;      // diagnostic
    if (mode == 1) hipLaunchKernelGGL(k_conv_wino_w4<1>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 2) hipLaunchKernelGGL(k_conv_wino_w4<2>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 3) hipLaunchKernelGGL(k_conv_wino_w4<3>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    else if (mode == 5) hipLaunchKernelGGL(k_conv_wino_w4<5>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // no weights, DMA, no barrier
    else if (mode == 9) hipLaunchKernelGGL(k_conv_wino_w4<9>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // no weights, barrier, no DMA
    else if (mode == 4) hipLaunchKernelGGL(k_conv_wino_w4<4>, dim3((unsigned)nblk), dim3(256), 0, s, a);      // everything but the barrier
    else
#endif
    hipLaunchKernelGGL(k_conv_wino_w4<0>, dim3((unsigned)nblk), dim3(256), 0, s, a);
    return check_launch();
}

}  // namespace fpc
