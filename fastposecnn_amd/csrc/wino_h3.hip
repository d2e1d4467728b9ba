// wino_h3.hip — k_conv_wino_h3: wino_h2.hip's four-wave Winograd F(2x2, 3x3) convolution on two fp16 pieces per operand with THREE
// piece products instead of four, over PAIRS of 8-channel K-steps (round 6, last form).
//
// Why.  k_conv_wino_h2 runs at the chip's power limit: taking its barrier out saves 10 % of its cycles and none of its time (the clock
// drops from 1.93 to 1.77 GHz), taking a quarter of its matrix instructions out saves no cycles and 11 % of its time (the clock rises to
// 2.15 GHz) — profiles/r06_wino_forms.md.  What shortens it is less work per product, not fewer stalls.
//   x w = (h1 + h2 + rx)(g1 + g2 + rw),  |h2| < 2^-10 |x|, |g2| < 2^-10 |w|, |rx| <= 3 * 2^-23 |x|, |rw| <= 3 * 2^-23 |w|   (truncation)
// The form keeps h1 g1 + h2 g1 + h1 g2 and drops h2 g2 (< 2^-20 |x w| at worst, 2^-22 |x w| for mantissas of all ones, ~2^-23 on average: the size of the two terms every two-piece form already
// drops, x rw and rx w).  Three products do not fit two matrix instructions per 8 channels, but they fit THREE per 16: the K dimension
// of v_mfma_f32_32x32x16_f16 carries 4 channels of the even K-step and 4 of the odd one,
//   A1 = {h1 even, h1 odd}   A2 = {h2 even, h2 odd}      B1 = {g1 even, g1 odd}   B2 = {g2 even, g2 odd}
//   acc += A1 B1 + A2 B1 + A1 B2
// so that 16 channels cost 48 matrix instructions per wave instead of 64, and — the pieces of a value are written ONCE, into the half of
// the operand tuple that belongs to its K-step — none of the 32 operand copies per step of the {h1, h1} / {h2, h2} form.
//
// Schedule of a pair p (K-steps 2p, 2p + 1), one barrier:
//   E        no matrix instruction: the sixteen fragment reads of step 2p + 1 (64 KB per workgroup = 512 cycles of the LDS pipe) are
//            issued first; under them the LDS-DMA burst of steps 2p + 3 and 2p + 4 (ring of four 18 KB buffers inside the output image's
//            space; a step past the last is not staged) and the pending split of xi 3 (even half); then the transform and xi 0's split
//            into the odd halves
//   O        48 matrix instructions (xi j: A1 B1 x 4, A2 B1 x 4, A1 B2 x 4) with one item of work behind each of the first 40 — two
//            behind the first twelve: the odd step's xi 1-3 splits (before xi 1's first instruction) beside step 2p + 2's fragment
//            reads and row transform; then its column transform, and the split of xi 0-2 into the even halves once xi j's last
//            matrix instruction has issued (xi 3 waits for the next E); each weight fragment is reloaded in place for the next pair
//            after its last use
//   end      counted wait for this wave's staging pieces (the 16 weight loads behind them stay in flight), barrier
// Entry: the weight fragments of pair 0 and steps 0, 1, 2 are requested together; step 0's transform runs while steps 1 and 2 land.
// Range and scaling are wino_h2.hip's; the input image's layout, the set-up around the loop and the output transform are
// wino_tile.hpp's; Cin must be a multiple of 16.
// Reference: the 3x3 / stride-1 convolutions of F/lib/pose_regressor.py:709-743 (smp encoder + FPN decoder, not vendored).
#include <algorithm>
#ifdef FPC_STAMP_WINO
#include <cstdlib>
#endif
#include <type_traits>
#include "conv_plan.hpp"      // wino_xshare_rule
#include "wino_tile.hpp"

namespace fpc {
using namespace wino_tile;

namespace {

constexpr int kRing = 4;                         // input buffers: step s lives in buffer s & 3
static_assert(kLdsFloats >= kRing * kInFloats, "the K loop's input ring lives in the output image's space");

// a wave-uniform pointer in scalar registers (the staging asm takes its base as an "s" operand)
__device__ __forceinline__ const float* sgpr_ptr(const float* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}

}  // namespace

// VAR (diagnostic, a -DFPC_STAMP_WINO build's FPC_H3_VAR at launch; the product is VAR 0): 1 = a piece's residual by conversion + subtraction instead of v_fma_mix_f32 (the same bits)
//
// FOLD: the FPN p2 level folded into s2.0 (a.fold; p2 = L c2 + b + up2_nearest(p3) is never written).  By linearity
//   conv3x3(W, p2) = conv3x3(W L, c2) + conv3x3(W, up2(p3)) + conv3x3(W, b 1_inside)
// and the K loop runs twice into the same accumulators: phase 1 over c2 (64 channels) on the composed weights' image, phase 2 over
// p3 on an image of W with the same power-of-two scale, the bias term comes from a table by border class in the epilogue.  Phase 2 stages the 18 x 18 region of the
// UPSAMPLED image straight from p3 (each lane's DMA address is its low-resolution pixel): a tile's input rows 2i-1 .. 2i+2 are then
// the low-resolution rows [a, b, b, c], and B^T [a, b, b, c] = [a-b, 2b, 0, b-c] with an exact 0 in floating point.  Transform row 2
// and column 2 are zero: every wave skips its xi column 2 in phase 2 (operands, weight loads, matrix instructions), 36 of 48 matrix
// instructions per pair.  Row 2 is wave 2's: in phase 2 that wave only STAGES (its share of the ring zeroing, its five pieces per
// K-step, the waits for them, every barrier) and loads no weights, reads no fragments, transforms, splits and multiplies nothing
// (a.all_rows = 1: it runs the phase on its zeros as before; fpc_net_set_fold_idle_row).  Its accumulators keep phase 1's sums: the
// dropped products were +-0, and an accumulator that started from +0 is never -0, so no bit of any output changes for finite p3 (a
// non-finite p3 value made NaN in that row, inf - inf, and no longer does).  How the branch is written matters at 512 registers:
//   - ONE instance of the loop, the condition made inside it from an opaque scalar: unswitched, the second instance spilled
//     ~1 KB per wave at the phase boundary;
//   - if-then only, never if-else: the structuriser turns a diamond, uniform or not, into Flow blocks whose phis carry every
//     loop-carried register on a poison edge, the coalescer gives up and ~300 scratch instructions land in the loop;
//   - one guarded block per pair, so phase 2 issues its staging burst IN FRONT of the fragment reads (phase 1 and the other
//     kernels keep it behind them): with the reads guarded apart from the rest, 5 to 8 accumulator registers are spilled across
//     the phase;
//   - the entry's weight loads pinned in program order in the fold kernels: the counted waits in front of the loop's matrix
//     instructions merge the entry's order with the loop's, and a scheduler that moves the first load behind eight others makes
//     vmcnt(11) a vmcnt(3), which waits for staging pieces issued a moment ago (+4 % on the kernel).
// profiles/fold_idle_row_ledger.md has the listings and the measurements.
//
// PACK: the patches are cut out of a canvas of a.pack frames side by side and a patch may carry a SEAM (wino_tile.hpp: wino_patch,
// wino_stage_plan).  Only the set-up and the epilogue know about it; the K loop is the plain one.
//
// TR: the launch runs TRANSPOSED (wino_orient_rule): a.H x a.W is the virtual image H' = W, W' = H whose pixel (y, x) is the stored
// pixel (x, y), the weight image was packed from the transposed taps.  The staging plan's byte offsets and the epilogue's output and
// residual offsets know; nothing else does.  Always with PACK (a single frame per canvas row is pack = 1).
//
// XS: the X-SHARED tile map (wino_tile.hpp: wino_frag, wino_slot, z_run; packed launches whose tile-column count is even,
// wino_xshare_rule).  A lane's two tiles are neighbours in x and share two of their four region columns: a K-step reads six columns
// of two rows (12 fragment reads, not 16) and row-transforms six (not 8); the column transforms, the splits, the operands and the
// matrix instructions are the plain ones, on the same numbers: every output is the plain map's, bit for bit.
template <int VAR, bool FOLD, bool PACK, bool TR = false, bool XS = false>
__global__ __launch_bounds__(256, 1) void k_conv_wino_h3(const WinoArgs a) {
    static_assert(PACK || !XS, "the x-shared map needs the packed decode's even seams");
    constexpr int kNC = XS ? 6 : 8;      // region columns a lane reads per row and K-step; tile half mt transforms columns kNC - 4 apart
    constexpr int kNR = 2 * kNC / 4;     // fragment reads per slot 0-3 of phase O
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    long long* const dbg = kWinoStamp ? a.dbg : nullptr;      // a constant in the product build: the stamp code below folds away
    const long long t_entry = dbg ? clock64() : 0;
    const int t = threadIdx.x, lane = t & 63;
    const int wi = __builtin_amdgcn_readfirstlane(t >> 6);      // transform row of this wave (wave-uniform)
    const int li = lane & 31, lh = lane >> 5;
    const int H = a.H, W = a.W, Cout = a.Cout;
    const int nnb = Cout / kBN;
    const WinoPatch pt = wino_patch<PACK>(blockIdx.x, nnb, a.groups, a.tbx, a.tby, a.pack, W, a.B, a.dec);
    const int nb = pt.nb, grp = pt.grp, pk_ks = pt.pk_ks;
    const ConvPtrs P = wino_group(a.p[0], a.p[1], a.p[2], a.p[3], grp);
    const int y_in0 = 2 * pt.ty0 - 1, x_in0 = 2 * pt.tx0 - 1;
    // (diagnostic build, FPC_WINO_SERIAL=1: a second, 16-word record per wave behind the first ones splits entry and exit, tools_dev/wino_serial_stamps.py)
    const bool fine = kWinoStamp && dbg && a.variant == kWinoSerialStamps;
    long long t_dec = fine ? clock64() : 0, t_wld = 0, t_plan = 0, t_zero = 0;

    f32x16 acc[4][2][2];      // [xi column j][tile half mt][32-channel tile nt]; zeroed while the first operands are on their way
    float inv_s = 1.f;        // 1 / (the power of two the weights of the LAST phase were scaled by)
    long long t_issued = 0, t_landed = 0, t_synced = 0, c_begin = 0, r_begin = 0;
    const bool stamp = dbg != nullptr;      // (the loop below never names `a`: a reference to the kernel argument puts it in scratch)
    const int all_rows = a.all_rows;

    // The K loop over one input image `src` (Cs channels; up = 1: read as its nearest-x2 upsample) on the weight image `wimg`.
    // PH 0: the whole loop (acc zeroed first); 1: fold phase 2 (xi column 2 skipped).  Every phase ends after a barrier with no
    // staging in flight and the input ring free.
    auto kloop = [&](auto ph, const float* src, const float* wimg, const int Cs, const int up) __attribute__((always_inline)) {
    constexpr int PH = decltype(ph)::value;
    constexpr bool SKIPC = PH == 1;
    // fold phase 2: transform row 2 is zero like column 2, and row 2 is wave 2's.  That wave only stages (its pieces wi + 4 i have no
    // other owner) and keeps every barrier; it loads no weights, reads no fragments and issues no transform, split or matrix
    // instruction — its accumulators keep phase 1's sums, to which the dropped products would have added +-0 (a.all_rows: it runs)
    int live = 1;
    if constexpr (PH == 1) live = __builtin_amdgcn_readfirstlane(all_rows | (wi ^ 2));
    const int nkb = Cs >> 3;
    const int npair = nkb >> 1;      // (the launcher refuses an odd number of K-steps)
    // ---- weights: buffer loads of this wave's fragments, per pair of K-steps one 16-byte B1 = {g1 even, g1 odd} and one B2 = {g2 even,
    // g2 odd} per (xi, 32-channel tile, lane)
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(reinterpret_cast<const char*>(wimg) + (size_t)nb * npair * kPairBytes);
    inv_s = wimg[(size_t)nnb * npair * (kPairBytes / 4)];      // 1 / (the power of two the weights were scaled by)
    const int vo_u = lane * 16;
    int so_u = wi * 4 * 4096;      // this wave's four xi; + kPairBytes per pair
    u32x4 U1[4][2], U2[4][2];
    if (live) {
    // (a fold phase 2 loads no fragment of xi column 2: 12 weight loads per pair instead of 16)
#define FPC_H3_XI_LIVE(J) (!(SKIPC && (J) == 2))
#define FPC_H3_LOAD_U1_AT(SO, J, NT) do { if (FPC_H3_XI_LIVE(J)) U1[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, (SO) + (J) * 4096 + (NT) * 2048, 0)); } while (0)
#define FPC_H3_LOAD_U2_AT(SO, J, NT) do { if (FPC_H3_XI_LIVE(J)) U2[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, (SO) + (J) * 4096 + (NT) * 2048 + 1024, 0)); } while (0)
#define FPC_H3_LOAD_U1(J, NT) FPC_H3_LOAD_U1_AT(so_u, J, NT)
#define FPC_H3_LOAD_U2(J, NT) FPC_H3_LOAD_U2_AT(so_u, J, NT)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            FPC_H3_LOAD_U1(j, nt); FPC_H3_LOAD_U2(j, nt);
            // (the fold kernels: the loads keep this order, the oldest first in the loop's order of use — the counted waits in front of
            // the loop's matrix instructions are made from it; one moved behind eight others turns vmcnt(11) into vmcnt(3), which
            // waits for the staging pieces issued a moment ago)
            if constexpr (FOLD) __builtin_amdgcn_sched_barrier(0);
        }
    if (npair > 1) so_u += kPairBytes;
    }
    // ---- the accumulators start from +0.0 (PH 1 keeps phase 1's sums; the fold kernels: below).  Sixteen matrix instructions on zero operands with the literal 0
    // as C, each writing the 16 registers of one accumulator (0 * 0 + 0 = +0.0, the bits 256 v_accvgpr_write left at ~1 k issue cycles
    // of the only wave on the SIMD, in front of the first wait).  Four at a time — xi column J's — behind the weight requests, behind
    // the staging plan and between the three staging bursts: each group runs in the matrix pipe while the wave issues what follows.
    // ONE zero operand, declared here and passed through an empty asm per call: written plainly the compiler merges the sixteen into
    // one instruction and 240 register copies.  profiles/wino_entry_ledger.md.
    f16x8 zop = {0, 0, 0, 0, 0, 0, 0, 0};
#define FPC_H3_ZERO_ACC(J) do { if constexpr (PH == 0 && !FOLD) {                                                    \
        _Pragma("unroll") for (int mt_ = 0; mt_ < 2; ++mt_)                                                   \
        _Pragma("unroll") for (int nt_ = 0; nt_ < 2; ++nt_) {                                                 \
            asm volatile("" : "+v"(zop));                                                                     \
            acc[J][mt_][nt_] = __builtin_amdgcn_mfma_f32_32x32x16_f16(zop, zop, f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0, 0, 0); \
        } } } while (0)
    FPC_H3_ZERO_ACC(0);
    if (PH == 0) t_wld = fine ? clock64() : 0;

    // ---- input staging and fragment addressing (wino_tile.hpp)
    const float* isb = sgpr_ptr(src + (size_t)pt.b * (H >> up) * (W >> up) * Cs);      // image base, + 8 floats per step
    unsigned ivo[5];
    unsigned long long imask[5];
    wino_stage_plan<PACK, TR, XS>(ivo, imask, wi, lane, y_in0, x_in0, H, W, Cs, up, pk_ks, pt.pk_two);
#define FPC_H3_ISSUE_IN(BUF, PTR) wino_issue_in(lds + (BUF) * kInFloats, wi, ivo, imask, PTR)
    int in_a[2], in_b[2];
    const float sgn = wino_frag<PACK, XS>(in_a, in_b, wi, li, lh, pk_ks);
    // fragment read x = 0 .. kNC - 1 of row a / b: column x of the lane's six (XS), else column x & 3 of tile half x >> 2
#define FPC_H3_FA(X) wino_frag_at<XS>(in_a, (X) >> 2, XS ? (X) : (X) & 3)
#define FPC_H3_FB(X) wino_frag_at<XS>(in_b, (X) >> 2, XS ? (X) : (X) & 3)
    // tile half MT's column transform of the row-transformed columns E[]
#define FPC_H3_COLUMN(E, MT, JX) ((JX) == 0 ? sub_s4(E[(MT) * (kNC - 4)], E[(MT) * (kNC - 4) + 2]) : (JX) == 1 ? add_s4(E[(MT) * (kNC - 4) + 1], E[(MT) * (kNC - 4) + 2]) : \
                                  (JX) == 2 ? sub_s4(E[(MT) * (kNC - 4) + 2], E[(MT) * (kNC - 4) + 1]) : sub_s4(E[(MT) * (kNC - 4) + 1], E[(MT) * (kNC - 4) + 3]))
    FPC_H3_ZERO_ACC(1);
    if (PH == 0) t_plan = fine ? clock64() : 0;
    wino_zero_ring(lds, t, kRing, y_in0, x_in0, H, W, PACK && pk_ks < kTX);
    if (PH == 0) t_zero = fine ? clock64() : 0;
    // steps 0, 1, 2 -> buffers 0, 1, 2
    FPC_H3_ISSUE_IN(0, isb);
    isb += 8;                      // (nkb >= 2)
    FPC_H3_ZERO_ACC(2);
    FPC_H3_ISSUE_IN(1, isb);
    isb += 8;
    FPC_H3_ZERO_ACC(3);
    FPC_H3_ISSUE_IN(2, nkb > 2 ? isb : isb - 8);      // (nkb = 2: step 1 again — the same count of pieces in front of the first wait)
    isb += 8;
    int sn = 3;                    // the next step to stage
    // (the fold kernels keep the register writes: with the matrix form the allocator hands phase 1's weight registers, whose last
    // redundant reloads are still in flight, to phase 2's fragment reads, and the compiler guards them with vmcnt(9) .. vmcnt(1)
    // inside the loop — waits for staging pieces issued a moment ago, +29 % on the kernel: profiles/wino_entry_ledger.md)
    if constexpr (PH == 0 && FOLD) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[j][mt][nt][r] = 0.f;
    }

    t_issued = stamp ? clock64() : 0;
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");      // the weight fragments and step 0 (steps 1, 2 land under step 0's transform; the weights are issued first: right without them too)
    t_landed = stamp ? clock64() : 0;
    __syncthreads();
    t_synced = stamp ? clock64() : 0;

    // operands as the matrix instructions take them: TA1[j][mt] = {h1 of the pair's even step, h1 of its odd step}, TA2[j][mt] = {h2
    // even, h2 odd} (four channels per piece and half); vn[mt][j]: the transformed values of the step whose pieces are being built
    // (xi 3's wait there from the end of O to the next E)
    u32x4 TA1[4][2], TA2[4][2];
    f32x4 vn[2][4];
    float m1;
    asm volatile("s_mov_b32 %0, 0xbf800000" : "=s"(m1));      // -1.0f, opaque
    // one pair of values of vn[MT][J] -> its fp16 pieces, into half HALF of the operands (pinned to its slot by the volatile asm that
    // reads them, as wino_w4.hip's items)
#define FPC_H3_SPLIT_PAIR(J, MT, PAIR, HALF) FPC_H3_SPLIT_PAIR_V(vn, J, MT, PAIR, HALF)
#define FPC_H3_SPLIT_PAIR_V(V, J, MT, PAIR, HALF)                                                             \
    if (FPC_H3_XI_LIVE(J)) do {                                                                               \
        const float x0_ = V[MT][J][2 * (PAIR)], x1_ = V[MT][J][2 * (PAIR) + 1];                               \
        const fp16x2 h_ = __builtin_amdgcn_cvt_pkrtz(x0_, x1_);                                               \
        /* x - h1 in ONE instruction: v_fma_mix_f32 reads the fp16 piece in place (m1 = -1 in a scalar register the compiler cannot  \
           fold); exact like the conversion + subtraction it replaces (VAR 1) */                                                  \
        const float r0_ = VAR == 1 ? x0_ - (float)h_[0] : __builtin_fmaf((float)h_[0], m1, x0_);              \
        const float r1_ = VAR == 1 ? x1_ - (float)h_[1] : __builtin_fmaf((float)h_[1], m1, x1_);              \
        const unsigned k1_ = __builtin_bit_cast(unsigned, h_);                                                \
        const unsigned k2_ = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_pkrtz(r0_, r1_));              \
        asm volatile("" :: "v"(k1_), "v"(k2_));                                                               \
        TA1[J][MT][2 * (HALF) + (PAIR)] = k1_; TA2[J][MT][2 * (HALF) + (PAIR)] = k2_;                         \
    } while (0)
    if (live) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) { TA1[j][mt] = u32x4{0u, 0u, 0u, 0u}; TA2[j][mt] = u32x4{0u, 0u, 0u, 0u}; }
    {      // step 0 -> the even halves of xi 0-2; xi 3 stays in vn for E of pair 0
        f32x4 e[kNC];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
            for (int x = mt * 4; x < (mt ? kNC : 4); ++x)      // (XS: half 1 adds columns 4 and 5 to half 0's four)
                e[x] = fma_s4(sgn, *reinterpret_cast<const f32x4*>(lds + FPC_H3_FB(x)), *reinterpret_cast<const f32x4*>(lds + FPC_H3_FA(x)));
#pragma unroll
            for (int j = 0; j < 4; ++j) vn[mt][j] = FPC_H3_COLUMN(e, mt, j);
#pragma unroll
            for (int j = 0; j < 3; ++j) { FPC_H3_SPLIT_PAIR(j, mt, 0, 0); FPC_H3_SPLIT_PAIR(j, mt, 1, 0); }
        }
    }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // steps 1 and 2
    __syncthreads();       // everybody's have landed; buffer 0 is refilled by the pieces of step 4, issued at the top of pair 0

#define FPC_H3_MFMA(J, MT, NT, A, B) do { if (FPC_H3_XI_LIVE(J)) acc[J][MT][NT] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, A), __builtin_bit_cast(f16x8, B), acc[J][MT][NT], 0, 0, 0); } while (0)
#define FPC_H3_PIN4(V) asm volatile("" :: "v"(V))
#define FPC_H3_SPLIT_Q(J, Q, HALF) do { if ((Q) == 0) FPC_H3_SPLIT_PAIR(J, 0, 0, HALF); if ((Q) == 1) FPC_H3_SPLIT_PAIR(J, 0, 1, HALF); if ((Q) == 2) FPC_H3_SPLIT_PAIR(J, 1, 0, HALF); if ((Q) == 3) FPC_H3_SPLIT_PAIR(J, 1, 1, HALF); } while (0)
    c_begin = stamp ? clock64() : 0; r_begin = stamp ? wall_clock64() : 0;
#pragma unroll 1
    for (int p = 0; p < npair; ++p) {
        // `live` again, made inside the loop from a scalar the compiler cannot see through: ONE instance of the loop serves both kinds
        // of wave (unswitched, the second instance spilled ~1 KB per wave at the phase boundary)
        bool lv = true;
        if constexpr (PH == 1) {
            int lv_;
            asm volatile("s_mov_b32 %0, %1" : "=s"(lv_) : "s"(live));
            lv = lv_ != 0;
        }
        // ---- E: step 2p + 1's fragment reads and transform; the odd halves of xi 0 (xi 1-3 follow behind O's first matrix instructions).
        // No matrix instruction is in flight behind the barrier: plain code, the sixteen fragment reads issued together.
        {
            // the sixteen fragment reads first: 64 KB per workgroup = 512 cycles of the LDS pipe, under the staging burst and xi 3's split
            const float* InE = lds + ((2 * p + 1) & 3) * kInFloats;
            f32x4 ea[kNC], eb[kNC];
#define FPC_H3_STAGE_PAIR() do { if (sn < nkb) { FPC_H3_ISSUE_IN((sn & 3), isb); isb += 8; }                  \
                                 if (sn + 1 < nkb) { FPC_H3_ISSUE_IN(((sn + 1) & 3), isb); isb += 8; }        \
                                 sn += 2; } while (0)
            if constexpr (PH == 1) FPC_H3_STAGE_PAIR();
            if (lv) {      // (to the end of O)
#pragma unroll
            for (int x = 0; x < kNC; ++x) {
                ea[x] = *reinterpret_cast<const f32x4*>(InE + FPC_H3_FA(x));
                eb[x] = *reinterpret_cast<const f32x4*>(InE + FPC_H3_FB(x));
            }
            __builtin_amdgcn_sched_barrier(0);
            // inputs of steps 2p + 3 and 2p + 4 -> the buffers steps 2p - 1 and 2p were read from before the last barrier
            // (a step past the last is not staged: the end-of-pair wait counts the sixteen weight loads BEHIND the pieces, so fewer
            // pieces in front of them keep it exact)
            if constexpr (PH == 0) FPC_H3_STAGE_PAIR();
#pragma unroll
            for (int q = 0; q < 4; ++q) FPC_H3_SPLIT_Q(3, q, 0);      // xi 3 of step 2p: its operands were in use until the end of O
            __builtin_amdgcn_sched_barrier(0);
            {
            f32x4 e[kNC];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int x = mt * 4; x < (mt ? kNC : 4); ++x) e[x] = fma_s4(sgn, eb[x], ea[x]);
#pragma unroll
                for (int j = 0; j < 4; ++j) vn[mt][j] = FPC_H3_COLUMN(e, mt, j);
                FPC_H3_SPLIT_PAIR(0, mt, 0, 1); FPC_H3_SPLIT_PAIR(0, mt, 1, 1);
            }
            }
        __builtin_amdgcn_sched_barrier(0);
        // ---- O: the pair's 48 matrix instructions; slot sl = 12 j + 4 g + 2 mt + nt, g = 0: A1 B1, 1: A2 B1, 2: A1 B2.  One item per slot:
        //   sl  0- 3  fragment reads of step 2p + 2       sl  4-11  row transform e (XS: 6-11)       sl 12-19  column transform vn
        //   sl  0- 3 / 4-7 / 8-11  ALSO the split of xi 1 / 2 / 3 of step 2p + 1 into the odd halves (before xi 1's first matrix instruction, slot 12,
        //             and before slot 12 overwrites vn)
        //   sl 20-23 / 24-27 / 36-39  split of xi 0 / 1 / 2 of step 2p + 2 into the even halves (xi j's last matrix instruction: slot 12 j + 11)
        // A weight fragment's last matrix instruction is followed by its reload for the next pair.
        const float* In = lds + ((2 * p + 2) & 3) * kInFloats;
        // XS: three reads per slot 0-3 (read q = 3 sl ..: column q >> 1, row a / b = q & 1), the six row transforms in slots 6-11
        f32x4 da[kNC], db[kNC], e[kNC];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int sl = 12 * j + 4 * g + 2 * mt + nt;
                        if (g == 0) FPC_H3_MFMA(j, mt, nt, TA1[j][mt], U1[j][nt]);
                        if (g == 1) {
                            FPC_H3_MFMA(j, mt, nt, TA2[j][mt], U1[j][nt]);
                            if (mt == 1) FPC_H3_LOAD_U1(j, nt);
                        }
                        if (g == 2) {
                            FPC_H3_MFMA(j, mt, nt, TA1[j][mt], U2[j][nt]);
                            if (mt == 1) FPC_H3_LOAD_U2(j, nt);
                        }
                        if (sl < 4) {
#pragma unroll
                            for (int q = kNR * sl; q < kNR * sl + kNR; ++q) {
                                if ((q & 1) == 0) da[q >> 1] = *reinterpret_cast<const f32x4*>(In + FPC_H3_FA(q >> 1));
                                if ((q & 1) == 1) db[q >> 1] = *reinterpret_cast<const f32x4*>(In + FPC_H3_FB(q >> 1));
                            }
                        }
                        if (sl >= 12 - kNC && sl < 12) {
                            const int x = sl - (12 - kNC);
                            e[x] = fma_s4(sgn, db[x], da[x]);
                            FPC_H3_PIN4(e[x]);
                        }
                        if (sl < 4) FPC_H3_SPLIT_Q(1, sl, 1);
                        if (sl >= 4 && sl < 8) FPC_H3_SPLIT_Q(2, sl - 4, 1);
                        if (sl >= 8 && sl < 12) FPC_H3_SPLIT_Q(3, sl - 8, 1);
                        if (sl >= 12 && sl < 20 && !(SKIPC && ((sl - 12) & 3) == 2)) {
                            const int m_ = (sl - 12) >> 2, jx = (sl - 12) & 3;
                            vn[m_][jx] = FPC_H3_COLUMN(e, m_, jx);
                            FPC_H3_PIN4(vn[m_][jx]);
                        }
                        if (sl >= 20 && sl < 24) FPC_H3_SPLIT_Q(0, sl - 20, 0);
                        if (sl >= 24 && sl < 28) FPC_H3_SPLIT_Q(1, sl - 24, 0);
                        if (sl >= 36 && sl < 40) FPC_H3_SPLIT_Q(2, sl - 36, 0);
                        __builtin_amdgcn_sched_barrier(0);
                    }
        __builtin_amdgcn_s_setprio(0);
        so_u += p + 2 < npair ? kPairBytes : 0;
        // this wave's ten pieces (issued before the pair's 16 weight loads, which stay in flight) have landed
        if (PH == 0) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        if (PH == 1) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        }
        }
        if (!lv) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (a wave that loads no weights has only its pieces in flight)
        __syncthreads();                                       // everybody's have; this pair's fragment reads are done
    }
#undef FPC_H3_MFMA
#undef FPC_H3_SPLIT_PAIR
#undef FPC_H3_SPLIT_PAIR_V
#undef FPC_H3_SPLIT_Q
#undef FPC_H3_PIN4
#undef FPC_H3_STAGE_PAIR
#undef FPC_H3_ISSUE_IN
#undef FPC_H3_LOAD_U1
#undef FPC_H3_LOAD_U2
#undef FPC_H3_LOAD_U1_AT
#undef FPC_H3_LOAD_U2_AT
#undef FPC_H3_XI_LIVE
#undef FPC_H3_ZERO_ACC
#undef FPC_H3_FA
#undef FPC_H3_FB
#undef FPC_H3_COLUMN
    };      // kloop

    if (!FOLD) {
        kloop(std::integral_constant<int, 0>(), P.in, P.w, a.Cin, 0);
    } else {
        kloop(std::integral_constant<int, 0>(), P.in, P.w, a.Cin, 0);
        // (both images carry ONE power-of-two scale, launch_wino_pack_h3_pair: phase 2 adds into the same scaled sums)
        kloop(std::integral_constant<int, 1>(), wino_group(a.in2[0], a.in2[1], a.in2[2], a.in2[3], grp), wino_group(a.w2[0], a.w2[1], a.w2[2], a.w2[3], grp), a.Cin2, 1);
    }
    // (no staging is in flight here: a step past the last is never issued, every real step was waited for at the end of its pair; the
    // last pair's redundant weight reloads target registers, whose reuse the compiler guards itself)
    const long long t_kend = dbg ? clock64() : 0;
    // (the packed fold never stamps — its launcher refuses dbg — and would carry `lane` across both loops in scratch for this test)
    if (!(FOLD && PACK) && dbg && lane == 0) {      // tools_dev/wino_stamps.py: shader-clock ticks and 100 MHz reference ticks of the K loop, entry -> loop
        long long* o = dbg + ((size_t)blockIdx.x * 4 + wi) * 8;
        o[0] = t_issued - t_entry; o[1] = t_landed - t_issued; o[2] = t_synced - t_landed;      // entry: set-up + issue | first operands land | barrier
        o[3] = t_kend - c_begin; o[4] = wall_clock64() - r_begin; o[5] = a.Cin >> 3; o[6] = c_begin - t_entry;
    }
    long long* const fdbg = (!(FOLD && PACK) && fine) ? dbg + (size_t)gridDim.x * 32 + ((size_t)blockIdx.x * 4 + wi) * 16 : nullptr;
    if (fdbg && lane == 0) { fdbg[0] = t_dec - t_entry; fdbg[1] = t_wld - t_entry; fdbg[2] = t_plan - t_entry; fdbg[3] = t_zero - t_entry; fdbg[4] = t_issued - t_entry; }
    wino_output<PACK, FOLD, TR, XS>(lds, acc, P, pt, WinoEpi{H, W, Cout, a.relu, a.tbx, a.tby, a.pack_rx, a.exit_general}, inv_s,
                            wino_group(a.btab[0], a.btab[1], a.btab[2], a.btab[3], grp), dbg, t_kend, t, wi, fdbg);
}

// The patch geometry of one k_conv_wino_h3 launch (host arithmetic).  tcw = ceil(W / 2) tile columns per frame; G = the smallest frame
// count in 1 .. min(B, 8) that minimises ceil(G tcw / 8) / G.  Packing is eligible when `allow` (not the fold), tcw >= 8 (a patch
// then straddles at most two frames) and two consecutive frames of the input fit 32-bit lane offsets; otherwise, and where it saves
// nothing, G = 1: today's grid.  Frames g G .. g G + G - 1 form canvas row g; a ragged last row launches only the patches that
// reach its frames.
WinoPackGeom wino_pack_geometry(int H, int W, int B, int Cin, bool allow) {
    WinoPackGeom q;
    const int tcw = cdiv(W, 2), tch = cdiv(H, 2);
    q.G = 1;
    q.tby = cdiv(tch, kTY);
    if (allow && tcw >= kTX && 2LL * H * W * Cin * (long long)sizeof(float) < (1LL << 32)) {
        int best = cdiv(tcw, kTX);      // patches per G frames, compared as fractions
        for (int g = 2; g <= std::min(B, 8); ++g)
            if ((long long)cdiv(g * tcw, kTX) * q.G < (long long)best * g) { best = cdiv(g * tcw, kTX); q.G = g; }
    }
    q.tbx = cdiv(q.G * tcw, kTX);
    q.rx = 1;
    for (int f = 0; f < q.G; ++f) q.rx = std::max(q.rx, (f * tcw + tcw - 1) / kTX - (f * tcw) / kTX + 1);
    q.patches = (long long)q.tby * ((long long)(B / q.G) * q.tbx + cdiv((B % q.G) * tcw, kTX));
    q.slots = q.patches * kNT;
    q.tiles = (long long)B * tch * tcw;
    q.gn_rows = q.tby * q.rx;
    return q;
}

// ---- host views of the two tile maps (wino_tile.hpp), through the very functions the kernels call (fpc_wino_tile_*, conv2d.hip)
// fragment reads of (wave wi, lane) in a patch with seam pk_ks (>= 8: none): out[0] = n columns, then per column x the byte offsets
// of its row-a and row-b read in an input buffer
int wino_tile_frag(bool xs, int wi, int lane, int pk_ks, long long* out17) {
    if (wi < 0 || wi > 3 || lane < 0 || lane > 63 || pk_ks < 0) return FPC_EINVAL;
    int in_a[2], in_b[2];
    if (xs) wino_frag<true, true>(in_a, in_b, wi, lane & 31, lane >> 5, pk_ks);
    else wino_frag<true, false>(in_a, in_b, wi, lane & 31, lane >> 5, pk_ks);
    const int n = xs ? 6 : 8;
    out17[0] = n;
    for (int x = 0; x < n; ++x) {
        out17[1 + 2 * x] = 4 * (xs ? wino_frag_at<true>(in_a, 0, x) : wino_frag_at<false>(in_a, x >> 2, x & 3));
        out17[2 + 2 * x] = 4 * (xs ? wino_frag_at<true>(in_b, 0, x) : wino_frag_at<false>(in_b, x >> 2, x & 3));
    }
    return 0;
}
// the staging plan's view of 16-byte unit `slot` (= 64 piece + lane) of a packed patch whose region starts at pixel (y_in0, x_in0) of
// a (virtual) H x W image of Cs channels (up, tr: wino_stage_plan): out6 = {region row, region column, channel half of the unit,
// behind the seam, staged, byte offset of its source from the K-step's channels of frame b}
int wino_tile_slot(bool xs, bool tr, int slot, int y_in0, int x_in0, int H, int W, int Cs, int up, int pk_ks, int pk_two, long long* out6) {
    if (slot < 0 || slot >= 5 * 4 * 64 || pk_ks < 0 || H < 1 || W < 1 || Cs < 8 || up < 0 || up > 1) return FPC_EINVAL;
    const WinoSlot u = xs ? wino_slot<true>(slot, pk_ks) : wino_slot<false>(slot, pk_ks);
    const WinoSrc q = xs ? (tr ? wino_stage_src<true, true, true>(slot, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two != 0)
                               : wino_stage_src<true, false, true>(slot, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two != 0))
                         : (tr ? wino_stage_src<true, true, false>(slot, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two != 0)
                               : wino_stage_src<true, false, false>(slot, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two != 0));
    out6[0] = 2 * u.ah + ((u.block >> 2) & 1); out6[1] = 2 * u.qh + ((u.block >> 1) & 1); out6[2] = u.block & 1;
    out6[3] = u.qh > pk_ks; out6[4] = q.ok; out6[5] = q.off;
    return 0;
}
// the Z image.  Writer: out3 = {byte offset of the run of (wave wi, half mt, register r, channel tile nt, column cc), the tile
// (8 ty + tx) of its lanes 0-31, of its lanes 32-63}.  Reader: the byte offset of thread t_e's read of pass tp, column cc, row i.
int wino_tile_zrun(bool xs, int wi, int mt, int r, int nt, int cc, long long* out3) {
    if (wi < 0 || wi > 3 || (mt | nt | cc) < 0 || (mt | nt | cc) > 1 || r < 0 || r > 15) return FPC_EINVAL;
    out3[0] = z_run(cc, mt, r, nt, xs) + 256 * wi;
    for (int hb = 0; hb < 2; ++hb) {
        const int li = (r & 3) + 8 * (r >> 2) + 4 * hb;      // the matrix instruction's row of this register and lane half
        out3[1 + hb] = xs ? 8 * (li >> 2) + 2 * (li & 3) + mt : 32 * mt + li;
    }
    return 0;
}
int wino_tile_zread(bool xs, int t_e, int tp, int cc, int i, long long* out1) {
    if (t_e < 0 || t_e > 255 || tp < 0 || tp > 3 || cc < 0 || cc > 1 || i < 0 || i > 3) return FPC_EINVAL;
    out1[0] = z_read_base(t_e >> 4, t_e & 15, xs) + z_read_step(tp, cc, i, xs);
    return 0;
}

// the exit.  The patch decode of workgroup `patch` of a launch with one 64-channel block and one group, through wino_patch and the
// launchers' own reciprocals, and whether it takes the fast exit
int wino_tile_patch(bool packed, int H, int W, int B, int tbx, int tby, int pack, int patch, long long* out8) {
    if (H < 1 || W < 1 || B < 1 || tbx < 1 || tby < 1 || patch < 0 || (packed && (pack < 1 || pack > B))) return FPC_EINVAL;
    const WinoDecode dc = wino_decode(kBN, 1, tbx, tby, W, B, packed ? pack : 0);
    const WinoPatch q = packed ? wino_patch<true>(patch, 1, 1, tbx, tby, pack, W, B, dc) : wino_patch<false>(patch, 1, 1, tbx, tby, 0, W, B, dc);
    if (q.b >= B || q.by >= tby) return FPC_EINVAL;
    const long long o[8] = {q.b, q.ty0, q.tx0, q.pk_ks, q.pk_two, q.by, q.bx, wino_exit_fast(H, W, q.ty0, q.tx0, q.pk_ks, q.pk_two)};
    std::copy(o, o + 8, out8);
    return 0;
}
// thread t_e's 16 output (and residual) element offsets, summed as wino_output sums them
int wino_tile_out(bool tr, int H, int W, int Cout, int nb, int b, int ty0, int tx0, int pk_ks, int t_e, long long* out16) {
    if (H < 1 || W < 1 || Cout < kBN || nb < 0 || b < 0 || ty0 < 0 || tx0 < 0 || pk_ks < 0 || t_e < 0 || t_e > 255) return FPC_EINVAL;
    const WinoOut o = tr ? wino_out_base<true, true>(H, W, Cout, nb, b, ty0, tx0, pk_ks, t_e >> 4, t_e & 15)
                         : wino_out_base<true, false>(H, W, Cout, nb, b, ty0, tx0, pk_ks, t_e >> 4, t_e & 15);
    for (int tp = 0; tp < 4; ++tp)
        for (int q = 0; q < 4; ++q) out16[4 * tp + q] = o.base + wino_out_step(o, tp, q >> 1, q & 1);
    return 0;
}

// what the fold's launch needs on top of wino_tile_check (wino_output<PACK, true> RELIES on these refusals)
static int wino_fold_check(const WinoArgs& a, int groups) {
    if (a.Cin2 % 16 != 0 || (a.H | a.W) & 1 || (long long)(a.H / 2) * (a.W / 2) * a.Cin2 * (long long)sizeof(float) >= (1LL << 32) ||
        (long long)(a.Cin2 >> 4) * kPairBytes >= (1LL << 31) || a.relu || a.dbg)
        return FPC_EINVAL;
    for (int g = 0; g < groups; ++g)
        if (!a.in2[g] || !a.w2[g] || !a.btab[g] || a.p[g].scale || a.p[g].shift || a.p[g].res || a.p[g].up) return FPC_EINVAL;
    return 0;
}

// The ORIENTATION RULE of a form-9 site, a property of its output shape alone (so a site keeps one weight image): run TRANSPOSED —
// the patch's x axis walks the image's y — iff the tile columns fill whole patches and the tile rows do not, and there are at least
// 8 tile rows (below that nothing can pack along them, and the GroupNorm records of a transposed launch would no longer fit the
// reservation of cdiv(H W, 128) * 4 per frame).  Frames then pack along the image's y (wino_pack_geometry on the swapped sizes).
bool wino_orient_rule(int H, int W) {
    const int tcw = cdiv(W, 2), tch = cdiv(H, 2);
    return tcw % kTX == 0 && tch % kTY != 0 && tch >= kTY;
}

// The geometry a form-9 launch of an H x W site uses: transposed where `orient` and the rule say so (then on the virtual image
// W x H, packing whatever `pack_allow` says: fpc_net_set_wino_pack governs the plain sites only), else wino_pack_geometry's.
// FPC_H3_ORIENT_G1 (a -DFPC_STAMP_WINO build only): a transposed launch keeps one frame per canvas row — the plain launch's patch count.
WinoPackGeom wino_launch_geometry(int H, int W, int B, int Cin, bool orient, bool pack_allow, bool* transposed) {
#ifdef FPC_STAMP_WINO
    static const bool g1 = getenv("FPC_H3_ORIENT_G1") && atoi(getenv("FPC_H3_ORIENT_G1")) != 0;
#else
    constexpr bool g1 = false;
#endif
    *transposed = orient && wino_orient_rule(H, W);
    return *transposed ? wino_pack_geometry(W, H, B, Cin, !g1) : wino_pack_geometry(H, W, B, Cin, pack_allow);
}

// .w = the k_wino_pack_fp16<true> image (+ its tail; wino_h2.hip), tby = ceil(ceil(H / 2) / 8): 8 x 8 tile patches
int launch_conv_wino_h3(const WinoArgs& a_in, int groups, hipStream_t s) {
    // pairs of 8-channel K-steps; a.pack > 1: patches cut out of canvas rows of a.pack frames, the geometry must be wino_pack_geometry's own
    long long nblk;
    if (a_in.orient) {
        const WinoArgs& a = a_in;
        // a.H x a.W is the stored image; the kernel gets the virtual one.  Always the packed decode (a.pack >= 1), images packed from
        // the transposed taps (launch_wino_pack_h3 / _pair, launch_fold_compose with transpose = true)
        WinoArgs t = a;
        std::swap(t.H, t.W);
        if (a.pack < 1) return FPC_EINVAL;      // (a stamp buffer: the plain records only, and never with the fold — wino_fold_check)
        if (const int rc = wino_tile_check(t, groups, 16, kPairBytes, true, &nblk)) return rc;
        t.dec = wino_decode(t.Cout, groups, t.tbx, t.tby, t.W, t.B, t.pack);
        if (a.xshare && !wino_xshare_rule(t.W)) return FPC_EINVAL;      // (an odd seam would part a lane's tile pair)
        if (a.fold) {
            if (const int rc = wino_fold_check(a, groups)) return rc;
            if (a.xshare) hipLaunchKernelGGL((k_conv_wino_h3<0, true, true, true, true>), dim3((unsigned)nblk), dim3(256), 0, s, t);
            else hipLaunchKernelGGL((k_conv_wino_h3<0, true, true, true>), dim3((unsigned)nblk), dim3(256), 0, s, t);
        } else {
            if (a.xshare) hipLaunchKernelGGL((k_conv_wino_h3<0, false, true, true, true>), dim3((unsigned)nblk), dim3(256), 0, s, t);
            else hipLaunchKernelGGL((k_conv_wino_h3<0, false, true, true>), dim3((unsigned)nblk), dim3(256), 0, s, t);
        }
        return check_launch();
    }
    if (const int rc = wino_tile_check(a_in, groups, 16, kPairBytes, a_in.pack > 1, &nblk)) return rc;
    WinoArgs a = a_in;      // + the reciprocals of the workgroup-id decode (wino_patch)
    a.dec = wino_decode(a.Cout, groups, a.tbx, a.tby, a.W, a.B, a.pack > 1 ? a.pack : 0);
    if (a.xshare && (a.pack <= 1 || a.fold || !wino_xshare_rule(a.W))) return FPC_EINVAL;      // packed launches only
    if (a.pack > 1) {
        if (a.xshare) hipLaunchKernelGGL((k_conv_wino_h3<0, false, true, false, true>), dim3((unsigned)nblk), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_conv_wino_h3<0, false, true>), dim3((unsigned)nblk), dim3(256), 0, s, a);
        return check_launch();
    }
    // c2 + up2(p3): both phases pairs of K-steps, p2 exactly 2 x p3, the bias table and nothing else in the epilogue.  wino_output<PACK, true>
    // (wino_tile.hpp) RELIES on the refusals below: it compiles scale, shift, residual and ReLU out
    if (a.fold) {
        if (const int rc = wino_fold_check(a, groups)) return rc;
        hipLaunchKernelGGL((k_conv_wino_h3<0, true, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
        return check_launch();
    }
#ifdef FPC_STAMP_WINO
    static const int var = getenv("FPC_H3_VAR") ? atoi(getenv("FPC_H3_VAR")) : 0;      // diagnostic
    static const bool serial = getenv("FPC_WINO_SERIAL") && atoi(getenv("FPC_WINO_SERIAL")) != 0;      // the stamp buffer holds the 16-word records too
    if (serial && a.dbg) a.variant = kWinoSerialStamps;
    if (var == 1) hipLaunchKernelGGL((k_conv_wino_h3<1, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
    else
#endif
    hipLaunchKernelGGL((k_conv_wino_h3<0, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
    return check_launch();
}

// wc[o][k][tap] = sum_c W[o][c][tap] L[c][k]; btab[(rc * 4 + cc) * Cout + o] = sum over the taps a pixel of row class rc / column class
// cc sees inside the image (bit 0: first row / column: no tap above / left; bit 1: last: none below / right) of sum_c W[o][c][tap] b[c].
// f64 sums, rounded once.  tr = 1: the table of the TRANSPOSED taps (a transposed launch's classes are the virtual image's: its row
// class is the stored image's column class); wc stays in W's own tap order (the packer transposes).
__global__ __launch_bounds__(256) void k_fold_compose(const float* __restrict__ w, const float* __restrict__ l, const float* __restrict__ bias,
                                                      float* __restrict__ wc, float* __restrict__ btab, int Cout, int Cmid, int Cin, int tr) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    const int nw = Cout * Cin * 9;
    if (g < nw) {
        const int tap = g % 9, k = (g / 9) % Cin, o = g / (9 * Cin);
        double acc = 0.0;
        for (int c = 0; c < Cmid; ++c) acc += (double)w[((size_t)o * Cmid + c) * 9 + tap] * (double)l[(size_t)c * Cin + k];
        wc[g] = (float)acc;
    } else if (g < nw + 16 * Cout) {
        const int o = (g - nw) % Cout, cls = (g - nw) / Cout, rc = cls >> 2, cc = cls & 3;
        double acc = 0.0;
        for (int ky = (rc & 1); ky < 3 - ((rc >> 1) & 1); ++ky)
            for (int kx = (cc & 1); kx < 3 - ((cc >> 1) & 1); ++kx)
                for (int c = 0; c < Cmid; ++c) acc += (double)w[((size_t)o * Cmid + c) * 9 + (tr ? kx * 3 + ky : ky * 3 + kx)] * (double)bias[c];
        btab[(size_t)cls * Cout + o] = (float)acc;
    }
}

int launch_fold_compose(const float* W, const float* L, const float* bias, float* wc, float* btab, int Cout, int Cmid, int Cin,
                        bool transpose, hipStream_t s) {
    if (!W || !L || !bias || !wc || !btab || Cout < 1 || Cmid < 1 || Cin < 1) return FPC_EINVAL;
    const long long work = (long long)Cout * Cin * 9 + 16LL * Cout;
    hipLaunchKernelGGL(k_fold_compose, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, W, L, bias, wc, btab, Cout, Cmid, Cin, transpose ? 1 : 0);
    return check_launch();
}

// the fold's two images (Wc: Cin1 channels, W: Cin2) scaled by ONE power of two, from the larger max |w| of the two.  (The packer
// kernel and launch_wino_pack_fp16 live in wino_h2.hip and are built with that file's flags.)
int launch_wino_pack_h3_pair(const float* w1, float* packed1, int Cin1, const float* w2, float* packed2, int Cin2, int Cout, bool transpose,
                             hipStream_t s) {
    if (Cin2 % 16 != 0 || ((uintptr_t)w2 & 15)) return FPC_EINVAL;      // (before the first image is touched)
    const int rc = launch_wino_pack_fp16(w1, packed1, Cout, Cin1, true, w2, Cin2, transpose, s);
    return rc ? rc : launch_wino_pack_fp16(w2, packed2, Cout, Cin2, true, w1, Cin1, transpose, s);
}

// pair-order fp16 x 2 image: 16 * Cout * Cin floats + a tail of 2 (1 / scale, max |w| bits); every byte is written.  transpose: of
// the transposed taps, for a site that runs transposed (wino_orient_rule)
int launch_wino_pack_h3(const float* w_oihw, float* packed, int Cout, int Cin, bool transpose, hipStream_t s) {
    return launch_wino_pack_fp16(w_oihw, packed, Cout, Cin, true, nullptr, 0, transpose, s);
}

}  // namespace fpc
