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
// Range, scaling, the input image's layout, the entry and the output transform are wino_h2.hip's; Cin must be a multiple of 16.
// Reference: the 3x3 / stride-1 convolutions of F/lib/pose_regressor.py:709-743 (smp encoder + FPN decoder, not vendored).
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "net_kernels.hpp"

namespace fpc {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int kTX = 8, kTY = 8;                  // tile patch 8 x 8 (16 x 16 output pixels)
constexpr int kRW = 2 * kTX + 2, kRH = 2 * kTY + 2;      // staged input region 18 x 18
constexpr int kBN = 64;                          // output channels per workgroup
constexpr int kNT = kTX * kTY;                   // 64 tiles = two M halves
constexpr int kInPieces = 18;                    // 1 KB LDS-DMA pieces of one K-step's input image (k_conv_wino's permuted image)
constexpr int kInFloats = kInPieces * 256;       // 4608 floats per input buffer
constexpr int kRing = 4;                         // input buffers: step s lives in buffer s & 3
constexpr int kPairBytes = 16 * 2 * 2 * 64 * 16; // k_wino_pack_h3's image of one pair of K-steps: [xi 16][tile 2][piece 2][lane 64] x 16 bytes {4 ch of the even step, 4 ch of the odd step}
constexpr int kLdsFloats = 4 * 2 * kNT * kBN;    // output transform image = 128 KB
static_assert(kLdsFloats >= kRing * kInFloats, "the K loop's input ring lives in the output image's space");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
// one scalar instruction per element (the file is built with -fno-slp-vectorize: beside matrix instructions a packed f32 instruction
// costs more than the two scalar ones it replaces).  Plain C++, not inline asm: the compiler brackets an asm statement it cannot see
// into with hazard s_nops (4 issue cycles each).  sgn = +-1: the fused form is exact either way.
__device__ __forceinline__ f32x4 fma_s4(float s, f32x4 b, f32x4 a) {
    return f32x4{__builtin_fmaf(s, b[0], a[0]), __builtin_fmaf(s, b[1], a[1]), __builtin_fmaf(s, b[2], a[2]), __builtin_fmaf(s, b[3], a[3])};
}
// a wave-uniform pointer in scalar registers (the staging asm takes its base as an "s" operand)
__device__ __forceinline__ const float* sgpr_ptr(const float* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return reinterpret_cast<const float*>(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ f32x4 sub_s4(f32x4 a, f32x4 b) { return f32x4{a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3]}; }
__device__ __forceinline__ f32x4 add_s4(f32x4 a, f32x4 b) { return f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]}; }

}  // namespace

// VAR (diagnostic, FPC_H3_VAR at launch): 1 = a piece's residual by conversion + subtraction instead of v_fma_mix_f32 (the same bits)
//
// FOLD: the FPN p2 level folded into s2.0 (a.fold; p2 = L c2 + b + up2_nearest(p3) is never written).  By linearity
//   conv3x3(W, p2) = conv3x3(W L, c2) + conv3x3(W, up2(p3)) + conv3x3(W, b 1_inside)
// and the K loop runs twice into the same accumulators: phase 1 over c2 (64 channels) on the composed weights' image, phase 2 over
// p3 on an image of W with the same power-of-two scale, the bias term comes from a table by border class in the epilogue.  Phase 2 stages the 18 x 18 region of the
// UPSAMPLED image straight from p3 (each lane's DMA address is its low-resolution pixel): a tile's input rows 2i-1 .. 2i+2 are then
// the low-resolution rows [a, b, b, c], and B^T [a, b, b, c] = [a-b, 2b, 0, b-c] with an exact 0 in floating point.  Transform row 2
// and column 2 are zero: every wave skips its xi column 2 in phase 2 (operands, weight loads, matrix instructions), 36 of 48 matrix
// instructions per pair.  Wave 2's row is zero too, but it still runs the loop (its products add exact zeros): a branch that gave it
// only the staging made the compiler spill ~1 KB per wave at the phase boundary.
//
// PACK: the patches are cut out of a canvas of a.pack frames side by side (wino_pack_geometry; a.tbx = patches per canvas row of a
// full group).  A patch that starts at tile column tx0 of frame f and meets the frame's end after ks < 8 columns carries a SEAM: its
// tile columns k >= ks are columns k - ks of frame f + 1.  The staged region then holds ONE gap column, tile column k reads region
// columns k + (k >= ks) + ch: region column ks holds frame f's last pixel (and the zero of x = W), column ks + 1 the zero of
// x = -1 and frame f + 1's first pixel.  Only the set-up and the epilogue know about it; the K loop is the plain one.
template <int VAR, bool FOLD, bool PACK>
__global__ __launch_bounds__(256, 1) void k_conv_wino_h3(const WinoArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kLdsFloats];
    const long long t_entry = a.dbg ? clock64() : 0;
    const int t = threadIdx.x, lane = t & 63;
    const int wi = __builtin_amdgcn_readfirstlane(t >> 6);      // transform row of this wave (wave-uniform)
    const int li = lane & 31, lh = lane >> 5;
    const int H = a.H, W = a.W, Cout = a.Cout, HW = H * W;
    // weight slice (group, 64-channel block) fastest: fixed per XCD under round-robin dispatch (k_conv_wino)
    int bid = blockIdx.x;
    const int nnb = Cout / kBN;
    const int nb = bid % nnb; bid /= nnb;
    const int grp = bid % a.groups; bid /= a.groups;
    int bx, by, b, tx0;
    int pk_ks = 99, pk_raw = 99, pk_slot = 0;      // PACK: seam after pk_ks tile columns (99: none), tcw - tx0, this patch's GroupNorm record of frame b
    bool pk_two = false;                           // PACK: the frame behind the seam exists
    if constexpr (!PACK) {
        bx = bid % a.tbx; bid /= a.tbx;
        by = bid % a.tby;
        b = bid / a.tby;
        tx0 = bx * kTX;
    } else {
        const int G = a.pack, tcw = (a.W + 1) >> 1, per = a.tbx * a.tby;
        const int g = bid / per, rem = bid - g * per;
        const int nf = min(G, a.B - g * G);                        // frames of this canvas row (a ragged last group has fewer,
        const int tbxg = min(a.tbx, (nf * tcw + kTX - 1) / kTX);   // and only the patches that reach them)
        bx = rem % tbxg; by = rem / tbxg;
        const int f = (kTX * bx) / tcw;
        tx0 = kTX * bx - f * tcw;
        b = g * G + f;
        pk_raw = tcw - tx0;
        pk_ks = pk_raw < kTX ? pk_raw : 99;
        pk_two = pk_ks < kTX && f + 1 < nf;
        pk_slot = bx - (f * tcw) / kTX;
    }
    ConvPtrs P = a.p[0];
    if (grp == 1) P = a.p[1];
    if (grp == 2) P = a.p[2];
    if (grp == 3) P = a.p[3];
    const int ty0 = by * kTY;
    const int y_in0 = 2 * ty0 - 1, x_in0 = 2 * tx0 - 1;

    f32x16 acc[4][2][2];      // [xi column j][tile half mt][32-channel tile nt]; zeroed while the first operands are on their way
    float inv_s = 1.f;        // 1 / (the power of two the weights of the LAST phase were scaled by)
    long long t_issued = 0, t_landed = 0, t_synced = 0, c_begin = 0, r_begin = 0;
    const bool stamp = a.dbg != nullptr;      // (the loop below never names `a`: a reference to the kernel argument puts it in scratch)

    // The K loop over one input image `src` (Cs channels; up = 1: read as its nearest-x2 upsample) on the weight image `wimg`.
    // PH 0: the whole loop (acc zeroed first); 1: fold phase 2 (xi column 2 skipped).  Every phase ends after a barrier with no
    // staging in flight and the input ring free.
    auto kloop = [&](auto ph, const float* src, const float* wimg, const int Cs, const int up) __attribute__((always_inline)) {
    constexpr int PH = decltype(ph)::value;
    constexpr bool SKIPC = PH == 1;
    const int nkb = Cs >> 3;
    const int npair = nkb >> 1;      // (the launcher refuses an odd number of K-steps)
    // ---- weights: buffer loads of this wave's fragments, per pair of K-steps one 16-byte B1 = {g1 even, g1 odd} and one B2 = {g2 even,
    // g2 odd} per (xi, 32-channel tile, lane)
    const __amdgpu_buffer_rsrc_t rs_w = make_rsrc(reinterpret_cast<const char*>(wimg) + (size_t)nb * npair * kPairBytes);
    inv_s = wimg[(size_t)nnb * npair * (kPairBytes / 4)];      // 1 / (the power of two the weights were scaled by)
    const int vo_u = lane * 16;
    int so_u = wi * 4 * 4096;      // this wave's four xi; + kPairBytes per pair
    u32x4 U1[4][2], U2[4][2];
    // (a fold phase 2 loads no fragment of xi column 2: 12 weight loads per pair instead of 16)
#define FPC_H3_XI_LIVE(J) (!(SKIPC && (J) == 2))
#define FPC_H3_LOAD_U1_AT(SO, J, NT) do { if (FPC_H3_XI_LIVE(J)) U1[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, (SO) + (J) * 4096 + (NT) * 2048, 0)); } while (0)
#define FPC_H3_LOAD_U2_AT(SO, J, NT) do { if (FPC_H3_XI_LIVE(J)) U2[J][NT] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, vo_u, (SO) + (J) * 4096 + (NT) * 2048 + 1024, 0)); } while (0)
#define FPC_H3_LOAD_U1(J, NT) FPC_H3_LOAD_U1_AT(so_u, J, NT)
#define FPC_H3_LOAD_U2(J, NT) FPC_H3_LOAD_U2_AT(so_u, J, NT)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) { FPC_H3_LOAD_U1(j, nt); FPC_H3_LOAD_U2(j, nt); }
    if (npair > 1) so_u += kPairBytes;

    // ---- input staging: LDS-DMA pieces (wave + 4 i), i < 5 (18 pieces).  The 16-byte unit a lane's data lands in decides the
    // global address it fetches (k_conv_wino, PERM): unit = (cell * 8 + block) * 16 + 4 * (qh & 3) + (ah & 3), cell = (ah >> 2) * 3 +
    // (qh >> 2), block = (ry & 1) * 4 + (rx & 1) * 2 + channel half, ah = ry >> 1, qh = rx >> 1 (0..8)
    const int Hs = H >> up, Ws = W >> up;                      // the source image's own size
    const float* isb = sgpr_ptr(src + (size_t)b * Hs * Ws * Cs);      // image base, + 8 floats per step
    unsigned ivo[5];
    bool iok[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int slot = (wi + 4 * i) * 64 + lane;
        const int blk = slot >> 4, res = slot & 15, cell = blk >> 3;
        const int ah = (cell / 3) * 4 + (res & 3), qh = (cell % 3) * 4 + (res >> 2);
        const int hf = blk & 1;
        const int ry = 2 * ah + ((blk >> 2) & 1), rx = 2 * qh + ((blk >> 1) & 1);
        const bool far = PACK && qh > pk_ks;      // behind the seam: frame b + 1, one gap column in between
        const int y = y_in0 + ry, x = far ? rx - 2 * pk_ks - 3 : x_in0 + rx;
        const int qmax = (PACK && pk_ks < kTX) ? kTX + 1 : kTX;
        iok[i] = wi + 4 * i < kInPieces && ah <= kTY && qh <= qmax && y >= 0 && y < H && x >= 0 && x < W && (!far || pk_two);
        ivo[i] = iok[i] ? (unsigned)((((size_t)(y >> up) * Ws + (x >> up)) * Cs + 4 * hf) * sizeof(float)) +
                              (far ? (unsigned)((size_t)Hs * Ws * Cs * sizeof(float)) : 0u)
                        : 0u;
    }
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#define FPC_LDS_ADDR(PTR) ((unsigned)(size_t)(__attribute__((address_space(3))) void*)(PTR))
    // One asm block, no branch: EXEC is set to each piece's lane mask (a wave-uniform 64-bit value; 0 for a piece this wave does not
    // have or whose positions all lie outside the image: the instruction then moves nothing but still counts in vmcnt, so every wave
    // issues exactly five VMEM instructions per step whatever the patch).  The compiler's own if (mask) form cost ~10 scalar /
    // branch instructions per piece, in a loop that is bound by instruction issue.
    unsigned long long imask[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) imask[i] = __ballot(iok[i]);
#define FPC_H3_ISSUE_IN(BUF, PTR)                                                                             \
    do {                                                                                                      \
        unsigned long long sv_;                                                                               \
        const unsigned l0_ = FPC_LDS_ADDR(lds + (BUF) * kInFloats + wi * 256);                                \
        asm volatile("s_mov_b64 %0, exec\n"                                                                   \
                     "s_mov_b64 exec, %1\n s_mov_b32 m0, %6\n s_nop 0\n global_load_lds_dwordx4 %11, %16\n"   \
                     "s_mov_b64 exec, %2\n s_mov_b32 m0, %7\n s_nop 0\n global_load_lds_dwordx4 %12, %16\n"   \
                     "s_mov_b64 exec, %3\n s_mov_b32 m0, %8\n s_nop 0\n global_load_lds_dwordx4 %13, %16\n"   \
                     "s_mov_b64 exec, %4\n s_mov_b32 m0, %9\n s_nop 0\n global_load_lds_dwordx4 %14, %16\n"   \
                     "s_mov_b64 exec, %5\n s_mov_b32 m0, %10\n s_nop 0\n global_load_lds_dwordx4 %15, %16\n"  \
                     "s_mov_b64 exec, %0\n"                                                                   \
                     : "=&s"(sv_)                                                                             \
                     : "s"(imask[0]), "s"(imask[1]), "s"(imask[2]), "s"(imask[3]), "s"(imask[4]),             \
                       "s"(l0_), "s"(l0_ + 4096), "s"(l0_ + 8192), "s"(l0_ + 12288), "s"(l0_ + 16384),        \
                       "v"(ivo[0]), "v"(ivo[1]), "v"(ivo[2]), "v"(ivo[3]), "v"(ivo[4]), "s"(PTR)              \
                     : "memory", "m0");                                                                       \
    } while (0)

    // ---- fragment addressing: this lane's tile of half 0 (half 1 = four tile rows further down = + 3 cells), the two region rows of
    // transform row wi, columns 2 txl + c
    const int tyl = li >> 3, txl = (li & 7) + ((PACK && (li & 7) >= pk_ks) ? 1 : 0);
    // row pair (ra, rb) and sign of B^T row wi:  0: d0-d2   1: d1+d2   2: d2-d1   3: d1-d3
    const int ra = (wi == 0) ? 0 : (wi == 2 ? 2 : 1);
    const int rb = (wi == 0) ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
    const float sgn = (wi == 1) ? 1.f : -1.f;
    auto unit = [&](int r, int ch) {      // float offset of row 2 tyl + r, column 2 (txl + ch), this lane's channel half
        const int ah = tyl + (r >> 1), qh = txl + ch;
        return ((((ah >> 2) * 3 + (qh >> 2)) * 8 + (r & 1) * 4 + lh) * 16 + 4 * (qh & 3) + (ah & 3)) * 4;
    };
    constexpr int in_cs = 2 * 16 * 4;          // + 1 column: the (rx & 1) block bit
    constexpr int in_ms = 3 * 8 * 16 * 4;      // + 4 tile rows (tile half 1): the next row of cells
    const int in_a[2] = {unit(ra, 0), unit(ra, 1)}, in_b[2] = {unit(rb, 0), unit(rb, 1)};

    // a patch that reaches over the image border zeroes the input ring once (inactive DMA lanes leave it alone); an
    // interior patch rewrites every unit the fragment reads touch with every step's DMA
    // (a seam patch too: the units of x = W and x = -1 at the seam are never staged and must read zero)
    if (y_in0 < 0 || x_in0 < 0 || y_in0 + kRH > H || x_in0 + kRW > W || (PACK && pk_ks < kTX)) {
        for (int i = t; i < kRing * kInFloats / 4; i += 256) reinterpret_cast<f32x4*>(lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // steps 0, 1, 2 -> buffers 0, 1, 2
    FPC_H3_ISSUE_IN(0, isb);
    isb += 8;                      // (nkb >= 2)
    FPC_H3_ISSUE_IN(1, isb);
    isb += 8;
    FPC_H3_ISSUE_IN(2, nkb > 2 ? isb : isb - 8);      // (nkb = 2: step 1 again — the same count of pieces in front of the first wait)
    isb += 8;
    int sn = 3;                    // the next step to stage
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (PH == 0) acc[j][mt][nt][r] = 0.f;

    t_issued = stamp ? clock64() : 0;
    asm volatile("s_waitcnt vmcnt(10)" ::: "memory");      // the weight fragments and step 0 (steps 1, 2 land under step 0's transform)
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
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) { TA1[j][mt] = u32x4{0u, 0u, 0u, 0u}; TA2[j][mt] = u32x4{0u, 0u, 0u, 0u}; }
    {      // step 0 -> the even halves of xi 0-2; xi 3 stays in vn for E of pair 0
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 e[4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                e[c] = fma_s4(sgn, *reinterpret_cast<const f32x4*>(lds + in_b[c >> 1] + (c & 1) * in_cs + mt * in_ms),
                              *reinterpret_cast<const f32x4*>(lds + in_a[c >> 1] + (c & 1) * in_cs + mt * in_ms));
            vn[mt][0] = sub_s4(e[0], e[2]); vn[mt][1] = add_s4(e[1], e[2]); vn[mt][2] = sub_s4(e[2], e[1]); vn[mt][3] = sub_s4(e[1], e[3]);
#pragma unroll
            for (int j = 0; j < 3; ++j) { FPC_H3_SPLIT_PAIR(j, mt, 0, 0); FPC_H3_SPLIT_PAIR(j, mt, 1, 0); }
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
        // ---- E: step 2p + 1's fragment reads and transform; the odd halves of xi 0 (xi 1-3 follow behind O's first matrix instructions).
        // No matrix instruction is in flight behind the barrier: plain code, the sixteen fragment reads issued together.
        {
            // the sixteen fragment reads first: 64 KB per workgroup = 512 cycles of the LDS pipe, under the staging burst and xi 3's split
            const float* InE = lds + ((2 * p + 1) & 3) * kInFloats;
            f32x4 ea[2][4], eb[2][4];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    ea[mt][c] = *reinterpret_cast<const f32x4*>(InE + in_a[c >> 1] + (c & 1) * in_cs + mt * in_ms);
                    eb[mt][c] = *reinterpret_cast<const f32x4*>(InE + in_b[c >> 1] + (c & 1) * in_cs + mt * in_ms);
                }
            __builtin_amdgcn_sched_barrier(0);
            // inputs of steps 2p + 3 and 2p + 4 -> the buffers steps 2p - 1 and 2p were read from before the last barrier
            // (a step past the last is not staged: the end-of-pair wait counts the sixteen weight loads BEHIND the pieces, so fewer
            // pieces in front of them keep it exact)
            if (sn < nkb) { FPC_H3_ISSUE_IN((sn & 3), isb); isb += 8; }
            if (sn + 1 < nkb) { FPC_H3_ISSUE_IN(((sn + 1) & 3), isb); isb += 8; }
            sn += 2;
#pragma unroll
            for (int q = 0; q < 4; ++q) FPC_H3_SPLIT_Q(3, q, 0);      // xi 3 of step 2p: its operands were in use until the end of O
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                f32x4 e[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) e[c] = fma_s4(sgn, eb[mt][c], ea[mt][c]);
                vn[mt][0] = sub_s4(e[0], e[2]); vn[mt][1] = add_s4(e[1], e[2]); vn[mt][2] = sub_s4(e[2], e[1]); vn[mt][3] = sub_s4(e[1], e[3]);
                FPC_H3_SPLIT_PAIR(0, mt, 0, 1); FPC_H3_SPLIT_PAIR(0, mt, 1, 1);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- O: the pair's 48 matrix instructions; slot sl = 12 j + 4 g + 2 mt + nt, g = 0: A1 B1, 1: A2 B1, 2: A1 B2.  One item per slot:
        //   sl  0- 3  fragment reads of step 2p + 2       sl  4-11  row transform e       sl 12-19  column transform vn
        //   sl  0- 3 / 4-7 / 8-11  ALSO the split of xi 1 / 2 / 3 of step 2p + 1 into the odd halves (before xi 1's first matrix instruction, slot 12,
        //             and before slot 12 overwrites vn)
        //   sl 20-23 / 24-27 / 36-39  split of xi 0 / 1 / 2 of step 2p + 2 into the even halves (xi j's last matrix instruction: slot 12 j + 11)
        // A weight fragment's last matrix instruction is followed by its reload for the next pair.
        const float* In = lds + ((2 * p + 2) & 3) * kInFloats;
        f32x4 da[2][4], db[2][4], e[2][4];
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
                            for (int c = 2 * (sl & 1); c < 2 * (sl & 1) + 2; ++c) {
                                da[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_a[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                                db[sl >> 1][c] = *reinterpret_cast<const f32x4*>(In + in_b[c >> 1] + (c & 1) * in_cs + (sl >> 1) * in_ms);
                            }
                        }
                        if (sl >= 4 && sl < 12) {
                            const int m_ = (sl - 4) >> 2, c = (sl - 4) & 3;
                            e[m_][c] = fma_s4(sgn, db[m_][c], da[m_][c]);
                            FPC_H3_PIN4(e[m_][c]);
                        }
                        if (sl < 4) FPC_H3_SPLIT_Q(1, sl, 1);
                        if (sl >= 4 && sl < 8) FPC_H3_SPLIT_Q(2, sl - 4, 1);
                        if (sl >= 8 && sl < 12) FPC_H3_SPLIT_Q(3, sl - 8, 1);
                        if (sl >= 12 && sl < 20 && !(SKIPC && ((sl - 12) & 3) == 2)) {
                            const int m_ = (sl - 12) >> 2, jx = (sl - 12) & 3;
                            if (jx == 0) vn[m_][0] = sub_s4(e[m_][0], e[m_][2]);
                            if (jx == 1) vn[m_][1] = add_s4(e[m_][1], e[m_][2]);
                            if (jx == 2) vn[m_][2] = sub_s4(e[m_][2], e[m_][1]);
                            if (jx == 3) vn[m_][3] = sub_s4(e[m_][1], e[m_][3]);
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
        __syncthreads();                                       // everybody's have; this pair's fragment reads are done
    }
#undef FPC_H3_MFMA
#undef FPC_H3_SPLIT_PAIR
#undef FPC_H3_SPLIT_PAIR_V
#undef FPC_H3_SPLIT_Q
#undef FPC_H3_PIN4
#undef FPC_H3_ISSUE_IN
#undef FPC_H3_LOAD_U1
#undef FPC_H3_LOAD_U2
#undef FPC_H3_LOAD_U1_AT
#undef FPC_H3_LOAD_U2_AT
#undef FPC_H3_XI_LIVE
#undef FPC_LDS_ADDR
#pragma clang diagnostic pop
    };      // kloop

    if (!FOLD) {
        kloop(std::integral_constant<int, 0>(), P.in, P.w, a.Cin, 0);
    } else {
        kloop(std::integral_constant<int, 0>(), P.in, P.w, a.Cin, 0);
        // (both images carry ONE power-of-two scale, launch_wino_pack_h3_pair: phase 2 adds into the same scaled sums)
        const float* w2 = a.w2[0];
        const float* in2 = a.in2[0];
        if (grp == 1) { w2 = a.w2[1]; in2 = a.in2[1]; }
        if (grp == 2) { w2 = a.w2[2]; in2 = a.in2[2]; }
        if (grp == 3) { w2 = a.w2[3]; in2 = a.in2[3]; }
        kloop(std::integral_constant<int, 1>(), in2, w2, a.Cin2, 1);
    }
    // (no staging is in flight here: a step past the last is never issued, every real step was waited for at the end of its pair; the
    // last pair's redundant weight reloads target registers, whose reuse the compiler guards itself)
    const long long t_kend = a.dbg ? clock64() : 0;
    if (a.dbg && lane == 0) {      // tools_dev/wino_stamps.py: shader-clock ticks and 100 MHz reference ticks of the K loop, entry -> loop
        long long* o = a.dbg + ((size_t)blockIdx.x * 4 + wi) * 8;
        o[0] = t_issued - t_entry; o[1] = t_landed - t_issued; o[2] = t_synced - t_landed;      // entry: set-up + issue | first operands land | barrier
        o[3] = t_kend - c_begin; o[4] = wall_clock64() - r_begin; o[5] = a.Cin >> 3; o[6] = c_begin - t_entry;
    }

    // ---- output transform.  Column part inside the wave: z0 = m0 + m1 + m2, z1 = m1 - m2 - m3; row part across the four
    // transform-row waves through LDS: y0 = z[0] + z[1] + z[2], y1 = z[1] - z[2] - z[3].  Z[row][cc][tile 64][co 64], one pass.
    // Output stage: thread = (tile of a 16-tile pass, 16-byte channel quad): within a ds_read_b128 lane group the 16 quads are 16
    // different bank slots; a wave stores 4 tiles x 256 contiguous bytes.
    // (PACK: the thread's indices are rebuilt from the lane counter here instead of being carried over the K loop: the packed
    // set-up needs a few registers more, and the allocator otherwise parks these in scratch from the set-up to the epilogue)
    const int lane_e = PACK ? (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) : lane;
    const int t_e = PACK ? wi * 64 + lane_e : t;
    const int oq = t_e & 15, otl = t_e >> 4;                  // quad 0..15, tile 0..15 (+ 16 per tile pass)
    // (ot & 7 is the same in all four tile passes of a thread: it lies wholly on one side of a seam)
    const bool o_far = PACK && (otl & 7) >= pk_ks;
    const int ob = o_far ? b + 1 : b, otx = o_far ? (otl & 7) - pk_ks : tx0 + (otl & 7);
    const bool o_ok = !o_far || pk_two;
    const int n = nb * kBN + oq * 4;
    const f32x4 e_sc = P.scale ? *reinterpret_cast<const f32x4*>(P.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 e_sh = P.shift ? *reinterpret_cast<const f32x4*>(P.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float* btab = a.btab[0];
    if (grp == 1) btab = a.btab[1];
    if (grp == 2) btab = a.btab[2];
    if (grp == 3) btab = a.btab[3];
    // the residual of this thread's 4 x 4 outputs is requested BEFORE the output transform's barriers (one workgroup per CU: nothing
    // else hides that latency; k_conv_wino does the same)
    f32x4 e_res[4][4];
#pragma unroll
    for (int tp = 0; tp < 4; ++tp)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ot = otl + 16 * tp;
            const int y = 2 * (ty0 + (ot >> 3)) + (q >> 1), x = 2 * otx + (q & 1);
            e_res[tp][q] = (P.res && o_ok && y < H && x < W) ? *reinterpret_cast<const f32x4*>(P.res + ((size_t)ob * HW + (size_t)y * W + x) * Cout + n)
                                                     : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    __syncthreads();
    float* const zb = lds + ((wi * 2) * kNT + 4 * (PACK ? lane_e >> 5 : lh)) * kBN + (PACK ? lane_e & 31 : li);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // one base register per lane + a compile-time offset (< 64 KB: the instruction's immediate) per store
                const int mc = mt * 32 + (r & 3) + 8 * (r >> 2);
                const float m0 = acc[0][mt][nt][r], m1 = acc[1][mt][nt][r], m2 = acc[2][mt][nt][r], m3 = acc[3][mt][nt][r];
                zb[(0 * kNT + mc) * kBN + nt * 32] = m0 + m1 + m2;
                zb[(1 * kNT + mc) * kBN + nt * 32] = m1 - m2 - m3;
            }
    __syncthreads();
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        const int ot = otl + 16 * tp;
        const int oty = ty0 + (ot >> 3);
        f32x4 z[4][2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) z[i][cc] = *reinterpret_cast<const f32x4*>(lds + ((i * 2 + cc) * kNT + ot) * kBN + oq * 4);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int y = 2 * oty + rr, x = 2 * otx + cc;
                if (y >= H || x >= W || !o_ok) continue;
                f32x4 val = (rr == 0 ? z[0][cc] + z[1][cc] + z[2][cc] : z[1][cc] - z[2][cc] - z[3][cc]) * inv_s;      // (a power of two: exact)
                if (FOLD) {      // conv3x3(W, b 1_inside): by the output pixel's border class
                    const int cls = (((y == 0) | ((y == H - 1) << 1)) << 2) | (x == 0) | ((x == W - 1) << 1);
                    val += *reinterpret_cast<const f32x4*>(btab + (size_t)cls * Cout + n);
                }
                if (P.scale) val = val * e_sc;
                val = val + e_sh;
                const size_t o = ((size_t)ob * HW + (size_t)y * W + x) * Cout + n;
                if (P.res) val += e_res[tp][2 * rr + cc];
                if (a.relu) { val[0] = fmaxf(val[0], 0.f); val[1] = fmaxf(val[1], 0.f); val[2] = fmaxf(val[2], 0.f); val[3] = fmaxf(val[3], 0.f); }
                *reinterpret_cast<f32x4*>(P.out + o) = val;
                s1 += val;
                s2 += val * val;
            }
    }
    if (PACK && P.gn_part) {
        // one record per frame this workgroup touches: two sets of sums, a thread's go to its side of the seam; the reduction is the
        // plain one on both.  Record of frame b: slot pk_slot of row by (a.pack_rx slots per row: the most patches a frame meets),
        // of frame b + 1: slot 0.  The patch that holds a frame's last tile column zeroes the slots the frame does not use, so every
        // record k_gn_finalize reads is written by this launch.
        f32x4 q1[2] = {o_far ? f32x4{0.f, 0.f, 0.f, 0.f} : s1, o_far ? s1 : f32x4{0.f, 0.f, 0.f, 0.f}};
        f32x4 q2[2] = {o_far ? f32x4{0.f, 0.f, 0.f, 0.f} : s2, o_far ? s2 : f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int sd = 0; sd < 2; ++sd)
#pragma unroll
            for (int o = 16; o < 64; o <<= 1)
#pragma unroll
                for (int k = 0; k < 4; ++k) { q1[sd][k] += __shfl_xor(q1[sd][k], o, 64); q2[sd][k] += __shfl_xor(q2[sd][k], o, 64); }
        __syncthreads();
        float* red = lds;                                     // [2 sides][4 waves][64 ch][2]
        if (lane_e < 16) {
#pragma unroll
            for (int sd = 0; sd < 2; ++sd)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    red[((sd * 4 + wi) * kBN + oq * 4 + k) * 2] = q1[sd][k];
                    red[((sd * 4 + wi) * kBN + oq * 4 + k) * 2 + 1] = q2[sd][k];
                }
        }
        __syncthreads();
        if (t_e < 2 * kBN && (t_e < kBN || pk_two)) {
            const int sd = t_e >> 6, ch = t_e & (kBN - 1);
            float u1 = 0.f, u2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { u1 += red[((sd * 4 + w) * kBN + ch) * 2]; u2 += red[((sd * 4 + w) * kBN + ch) * 2 + 1]; }
            const int rx = a.pack_rx, Pn = a.tby * rx, slot = sd ? 0 : pk_slot;
            float* g = P.gn_part + (((size_t)(b + sd) * Pn + by * rx + slot) * Cout + nb * kBN + ch) * 2;
            g[0] = u1; g[1] = u2;
            if (sd == 0 && pk_raw <= kTX)
                for (int z = slot + 1; z < rx; ++z) { g += (size_t)Cout * 2; g[0] = 0.f; g[1] = 0.f; }
        }
    } else if (P.gn_part) {
        // per-channel sums of this workgroup's outputs: a wave holds 4 tiles (lane bits 4-5) x 16 quads (lane bits 0-3) per pass:
        // butterfly over the tile bits, then the four waves' sums through LDS in wave order
#pragma unroll
        for (int o = 16; o < 64; o <<= 1)
#pragma unroll
            for (int k = 0; k < 4; ++k) { s1[k] += __shfl_xor(s1[k], o, 64); s2[k] += __shfl_xor(s2[k], o, 64); }
        __syncthreads();
        float* red = lds;                                     // [4 waves][64 ch][2]
        if (lane < 16) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { red[(wi * kBN + oq * 4 + k) * 2] = s1[k]; red[(wi * kBN + oq * 4 + k) * 2 + 1] = s2[k]; }
        }
        __syncthreads();
        if (t < kBN) {
            float u1 = 0.f, u2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { u1 += red[(w * kBN + t) * 2]; u2 += red[(w * kBN + t) * 2 + 1]; }
            const int Pn = a.tbx * a.tby;
            float* g = P.gn_part + (((size_t)b * Pn + by * a.tbx + bx) * Cout + nb * kBN + t) * 2;
            g[0] = u1; g[1] = u2;
        }
    }
    if (a.dbg && lane == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        a.dbg[((size_t)blockIdx.x * 4 + wi) * 8 + 7] = clock64() - t_kend;      // K loop end -> last store acknowledged
    }
}

// k_wino_pack_h2's transform, scale and split; the fragment order of the PAIR form:
// [Cout/64][Cin/16][xi 16][tile 2][piece 2][lane 64] x {4 ch of the even K-step, 4 ch of the odd one}, lane = (channel half) * 32 + (co & 31),
// tile = (co & 63) >> 5; tail[0] = 1 / s (f32), tail[1] max |w|'s bits (k_absmax_bits, wino_h2.hip).
__global__ __launch_bounds__(256) void k_wino_pack_h3(const float* __restrict__ w, unsigned short* __restrict__ out, float* __restrict__ tail,
                                                      int Cout, int Cin) {
    const float wmax = __builtin_bit_cast(float, reinterpret_cast<const unsigned*>(tail)[1]);
    int ex = 0;
    if (wmax > 0.f && wmax < 3.0e38f) { (void)frexpf(2.25f * wmax, &ex); ex = 13 - ex; }
    ex = max(-100, min(100, ex));
    const float sc = ldexpf(1.0f, ex);
    if (blockIdx.x == 0 && threadIdx.x == 0) tail[0] = ldexpf(1.0f, -ex);
    const long long total = (long long)Cout * Cin;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (long long)gridDim.x * blockDim.x) {
        const int ci = (int)(g % Cin), co = (int)(g / Cin);
        const float* k = w + ((size_t)co * Cin + ci) * 9;
        float gg[4][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float g0 = k[c] * sc, g1 = k[3 + c] * sc, g2 = k[6 + c] * sc;
            gg[0][c] = g0;
            gg[1][c] = 0.5f * (g0 + g1 + g2);
            gg[2][c] = 0.5f * (g0 - g1 + g2);
            gg[3][c] = g2;
        }
        const int nb = co >> 6, col = co & 63, nt = col >> 5, kb = ci >> 3, cil = ci & 7, e = cil & 3;
        const int ln = (cil >> 2) * 32 + (col & 31);
        unsigned short* img = out + ((size_t)nb * (Cin >> 4) + (kb >> 1)) * (kPairBytes / 2);
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
                unsigned short* frag = img + ((4 * i + jx) * 4096 + nt * 2048 + ln * 16) / 2;
                frag[(kb & 1) * 4 + e] = (unsigned short)(__builtin_bit_cast(unsigned, h) & 0xFFFFu);
                frag[512 + (kb & 1) * 4 + e] = (unsigned short)(__builtin_bit_cast(unsigned, h2) & 0xFFFFu);
            }
        }
    }
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

// .w = the k_wino_pack_h3 image (+ its tail), tby = ceil(ceil(H / 2) / 8): 8 x 8 tile patches
int launch_conv_wino_h3(const WinoArgs& a, int groups, hipStream_t s) {
    if (groups < 1 || groups > kMaxGroup || a.Cin % 16 != 0 || a.Cout % kBN != 0) return FPC_EINVAL;      // pairs of 8-channel K-steps
    if ((long long)a.H * a.W * a.Cin * (long long)sizeof(float) >= (1LL << 32)) return FPC_EINVAL;      // 32-bit lane offsets inside one image
    if ((long long)(a.Cin >> 4) * kPairBytes >= (1LL << 31)) return FPC_EINVAL;                          // 31-bit buffer offsets inside one block's images
    if (a.pack > 1) {      // patches cut out of canvas rows of a.pack frames: the geometry must be wino_pack_geometry's own
        const WinoPackGeom q = wino_pack_geometry(a.H, a.W, a.B, a.Cin, !a.fold);
        if (q.G != a.pack || q.tbx != a.tbx || q.tby != a.tby || q.rx != a.pack_rx) return FPC_EINVAL;
        const long long nblk = q.patches * (a.Cout / kBN) * groups;
        if (nblk < 1 || nblk >= (1LL << 31)) return FPC_EINVAL;
        hipLaunchKernelGGL((k_conv_wino_h3<0, false, true>), dim3((unsigned)nblk), dim3(256), 0, s, a);
        return check_launch();
    }
    if (a.tbx != cdiv(cdiv(a.W, 2), kTX) || a.tby != cdiv(cdiv(a.H, 2), kTY)) return FPC_EINVAL;
    const long long nblk = (long long)a.tbx * a.tby * a.B * (a.Cout / kBN) * groups;
    if (nblk < 1 || nblk >= (1LL << 31)) return FPC_EINVAL;
    if (a.fold) {      // c2 + up2(p3): both phases pairs of K-steps, p2 exactly 2 x p3, the bias table and nothing else in the epilogue
        if (a.Cin2 % 16 != 0 || (a.H | a.W) & 1 || (long long)(a.H / 2) * (a.W / 2) * a.Cin2 * (long long)sizeof(float) >= (1LL << 32) ||
            (long long)(a.Cin2 >> 4) * kPairBytes >= (1LL << 31) || a.relu || a.dbg)
            return FPC_EINVAL;
        for (int g = 0; g < groups; ++g)
            if (!a.in2[g] || !a.w2[g] || !a.btab[g] || a.p[g].scale || a.p[g].shift || a.p[g].res || a.p[g].up) return FPC_EINVAL;
        hipLaunchKernelGGL((k_conv_wino_h3<0, true, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
        return check_launch();
    }
    static const int var = getenv("FPC_H3_VAR") ? atoi(getenv("FPC_H3_VAR")) : 0;      // diagnostic
    if (var == 1) hipLaunchKernelGGL((k_conv_wino_h3<1, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_conv_wino_h3<0, false, false>), dim3((unsigned)nblk), dim3(256), 0, s, a);
    return check_launch();
}

// wc[o][k][tap] = sum_c W[o][c][tap] L[c][k]; btab[(rc * 4 + cc) * Cout + o] = sum over the taps a pixel of row class rc / column class
// cc sees inside the image (bit 0: first row / column: no tap above / left; bit 1: last: none below / right) of sum_c W[o][c][tap] b[c].
// f64 sums, rounded once.
__global__ __launch_bounds__(256) void k_fold_compose(const float* __restrict__ w, const float* __restrict__ l, const float* __restrict__ bias,
                                                      float* __restrict__ wc, float* __restrict__ btab, int Cout, int Cmid, int Cin) {
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
                for (int c = 0; c < Cmid; ++c) acc += (double)w[((size_t)o * Cmid + c) * 9 + ky * 3 + kx] * (double)bias[c];
        btab[(size_t)cls * Cout + o] = (float)acc;
    }
}

int launch_fold_compose(const float* W, const float* L, const float* bias, float* wc, float* btab, int Cout, int Cmid, int Cin,
                        hipStream_t s) {
    if (!W || !L || !bias || !wc || !btab || Cout < 1 || Cmid < 1 || Cin < 1) return FPC_EINVAL;
    const long long work = (long long)Cout * Cin * 9 + 16LL * Cout;
    hipLaunchKernelGGL(k_fold_compose, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, s, W, L, bias, wc, btab, Cout, Cmid, Cin);
    return check_launch();
}

// the fold's two images (Wc: Cin1 channels, W: Cin2) scaled by ONE power of two, from the larger max |w| of the two
int launch_wino_pack_h3_pair(const float* w1, float* packed1, int Cin1, const float* w2, float* packed2, int Cin2, int Cout, hipStream_t s) {
    if (Cin1 % 16 != 0 || Cin2 % 16 != 0 || Cout % kBN != 0 || ((uintptr_t)w1 & 15) || ((uintptr_t)w2 & 15)) return FPC_EINVAL;
    float* tail1 = packed1 + (size_t)16 * Cout * Cin1;
    float* tail2 = packed2 + (size_t)16 * Cout * Cin2;
    if (hipMemsetAsync(tail1, 0, 2 * sizeof(float), s) != hipSuccess || hipMemsetAsync(tail2, 0, 2 * sizeof(float), s) != hipSuccess)
        return FPC_ELAUNCH;
    for (float* tail : {tail1, tail2}) {
        int rc = launch_absmax_bits(w1, (long long)Cout * Cin1 * 9, reinterpret_cast<unsigned*>(tail) + 1, s);
        if (!rc) rc = launch_absmax_bits(w2, (long long)Cout * Cin2 * 9, reinterpret_cast<unsigned*>(tail) + 1, s);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(k_wino_pack_h3, dim3((unsigned)std::min<long long>(((long long)Cout * Cin1 + 255) / 256, 4096)), dim3(256), 0, s, w1,
                       reinterpret_cast<unsigned short*>(packed1), tail1, Cout, Cin1);
    int rc = check_launch();
    if (rc) return rc;
    hipLaunchKernelGGL(k_wino_pack_h3, dim3((unsigned)std::min<long long>(((long long)Cout * Cin2 + 255) / 256, 4096)), dim3(256), 0, s, w2,
                       reinterpret_cast<unsigned short*>(packed2), tail2, Cout, Cin2);
    return check_launch();
}

// pair-order fp16 x 2 image: 16 * Cout * Cin floats + a tail of 2 (1 / scale, max |w| bits); every byte is written
int launch_wino_pack_h3(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s) {
    if (Cin % 16 != 0 || Cout % kBN != 0) return FPC_EINVAL;
    float* tail = packed + (size_t)16 * Cout * Cin;
    if (hipMemsetAsync(tail, 0, 2 * sizeof(float), s) != hipSuccess) return FPC_ELAUNCH;
    if ((uintptr_t)w_oihw & 15) return FPC_EINVAL;
    const int rc = launch_absmax_bits(w_oihw, (long long)Cout * Cin * 9, reinterpret_cast<unsigned*>(tail) + 1, s);
    if (rc) return rc;
    const long long work = (long long)Cout * Cin;
    hipLaunchKernelGGL(k_wino_pack_h3, dim3((unsigned)std::min<long long>((work + 255) / 256, 4096)), dim3(256), 0, s, w_oihw,
                       reinterpret_cast<unsigned short*>(packed), tail, Cout, Cin);
    return check_launch();
}

}  // namespace fpc
