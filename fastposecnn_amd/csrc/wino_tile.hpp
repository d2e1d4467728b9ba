// wino_tile.hpp — what the four-wave Winograd F(2x2, 3x3) kernels share (wino_w4.hip, wino_h2.hip, wino_h3.hip): one workgroup =
// an 8 x 8 tile patch (16 x 16 output pixels) x 64 output channels, 256 threads = one wave per SIMD with up to 512 registers, wave
// w owning transform row w; the K loop's input buffers and, after it, the 128 KB output transform image in LDS.  The files keep
// their K loops (the operands' number format, the slot schedule, the weight image); the set-up around the loop and everything
// behind it is here, once:
//   patch decode (wino_patch) — staging plan and LDS-DMA issue (wino_stage_plan, wino_issue_in) — fragment addressing (wino_frag)
//   and border zeroing (wino_zero_ring) — output transform and epilogue (wino_output) — the launchers' shape check
//   (wino_tile_check) — the fp16 weight packers' host entry (launch_wino_pack_fp16, defined in wino_h2.hip)
// Everything a kernel calls is __forceinline__ and takes VALUES (a reference to the kernel argument that survives inlining puts the
// argument in scratch): the kernels sit at 512 registers, and their listings are the test of a change here (tools_dev/isa_stats.py).
#pragma once
#include <algorithm>
#include <type_traits>
#include "net_kernels.hpp"

namespace fpc {
namespace wino_tile {      // the three files say `using namespace wino_tile;`: nothing else sees these names

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

constexpr int kTX = 8, kTY = 8;                  // tile patch 8 x 8 (16 x 16 output pixels)
constexpr int kRW = 2 * kTX + 2, kRH = 2 * kTY + 2;      // staged input region 18 x 18
constexpr int kBN = 64;                          // output channels per workgroup
constexpr int kNT = kTX * kTY;                   // 64 tiles = two M halves
constexpr int kInPieces = 18;                    // 1 KB LDS-DMA pieces of one K-step's input image (k_conv_wino's permuted image)
constexpr int kInFloats = kInPieces * 256;       // 4608 floats per input buffer
constexpr int kPairBytes = 16 * 2 * 2 * 64 * 16; // k_wino_pack_fp16<true>'s image of one pair of K-steps (wino_h3.hip): [xi 16][tile 2][piece 2][lane 64] x 16 bytes {4 ch of the even step, 4 ch of the odd step}
// The output transform image Z: per transform row i, column cc (z0 / z1), 64 tiles x 64 channels, as RUNS of 64 floats = the 64 lanes
// of one accumulator register: run (cc, mt, r, nt) holds channels nt * 32 .. + 31 of tile mt * 32 + (r & 3) + 8 (r >> 2) and then of the
// tile four further (wino_output).  Row i's copy of a run lies 256 bytes behind row i - 1's.  The runs of odd r live in a second
// 64 KB region that starts HALF a 256-byte bank row late: a ds_read_b128 lane group of the output stage holds eight quads of an even
// tile and eight of the odd tile beside it, all from the same half of their runs (lane bit 5 of the writer = tile bit 2, the same for
// a whole reading wave) — the shift puts the odd tile's on the other 128 bytes of the bank row, 16 different 16-byte slots per group.
// xs (the x-shared tile map, wino_frag<PACK, true>): register r of half mt holds tile row 2 (r >> 2) + (lane >> 5), tile column
// 2 (r & 3) + mt, and the even / odd tile pair of a reading lane group differs in mt: there the runs of mt = 1 live in the late region
// and r's low bit takes mt's place in the index.  The same bytes, the same two M0 bases, the same reach.
constexpr int kZOdd = 64 * 1024 + 128;           // byte offset of the odd runs' region
constexpr int z_run(int cc, int mt, int r, int nt, bool xs = false) {
    return ((((cc * 2 + (xs ? (r & 1) : mt)) * 8 + (r >> 1)) * 2 + nt) * 4) * 256 + (xs ? mt : (r & 1)) * kZOdd;
}
// byte offset of the output stage's first read of thread (tile otl of a 16-tile pass, channel quad oq): its tile of pass 0, row 0, cc 0
// (pass tp, column cc, row i: + z_run(cc, tp >> 1, 8 (tp & 1), 0) + 256 i; xs: + z_run(cc, 0, 4 tp, 0, true) + 256 i)
constexpr int z_read_base(int otl, int oq, bool xs = false) {
    return xs ? z_run(0, otl & 1, (otl >> 1) & 3, oq >> 3, true) + (otl >> 3) * 128 + (oq & 7) * 16
              : z_run(0, 0, (otl & 3) + 4 * (otl >> 3), oq >> 3) + ((otl >> 2) & 1) * 128 + (oq & 7) * 16;
}
constexpr int z_read_step(int tp, int cc, int i, bool xs = false) { return (xs ? z_run(cc, 0, 4 * tp, 0, true) : z_run(cc, tp >> 1, 8 * (tp & 1), 0)) + 256 * i; }
// ds_write_addtid_b32 adds M0's low 16 bits and a 16-bit immediate: the even runs from M0 = image + 256 wi (immediates up to 63 KB),
// the odd ones from that + kZOddM0 (immediates 960 .. 65 472); both fit while the image starts in the first kZM0Slack bytes of LDS
constexpr int kZOddM0 = 64704;
constexpr int kZM0Slack = 65535 - 3 * 256 - kZOddM0;
static_assert(z_run(1, 1, 15, 1) - kZOddM0 < 65536 && z_run(0, 0, 1, 0) >= kZOddM0 && kZM0Slack >= 0, "ds_write_addtid_b32's reach");
static_assert(z_run(1, 1, 15, 1, true) == z_run(1, 1, 15, 1) && z_run(0, 1, 0, 0, true) == z_run(0, 0, 1, 0) && z_run(1, 0, 15, 1, true) < 65536 - 3 * 256, "... and the x-shared map's");
constexpr int kLdsFloats = 4 * 2 * kNT * kBN + 32;      // the Z image = 128 KB + the odd region's shift; the K loop's input buffers live in its space
static_assert(z_run(1, 1, 15, 1) + 3 * 256 + 256 == kLdsFloats * 4, "the last run ends the image");

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
// one scalar instruction per element (the files are built with -fno-slp-vectorize: beside matrix instructions a packed f32 instruction
// costs more than the two scalar ones it replaces).  Plain C++, not inline asm: the compiler brackets an asm statement it cannot see
// into with hazard s_nops (4 issue cycles each).  sgn = +-1: the fused form is exact either way.
__device__ __forceinline__ f32x4 fma_s4(float s, f32x4 b, f32x4 a) {
    return f32x4{__builtin_fmaf(s, b[0], a[0]), __builtin_fmaf(s, b[1], a[1]), __builtin_fmaf(s, b[2], a[2]), __builtin_fmaf(s, b[3], a[3])};
}
__device__ __forceinline__ f32x4 sub_s4(f32x4 a, f32x4 b) { return f32x4{a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3]}; }
__device__ __forceinline__ f32x4 add_s4(f32x4 a, f32x4 b) { return f32x4{a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3]}; }

__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(__attribute__((address_space(3))) const void*)p; }

// ---- patch decode.  Weight slice (64-channel block, group) fastest in the workgroup id: fixed per XCD under round-robin dispatch
// (k_conv_wino).  The patch covers tiles (ty0 .., tx0 ..) of frame b.
// PACK (wino_h3.hip): the patches are cut out of a canvas of `pack` frames side by side (wino_pack_geometry; tbx = patches per canvas
// row of a full group).  A patch that starts at tile column tx0 of frame f and meets the frame's end after ks < 8 columns carries a
// SEAM: its tile columns k >= ks are columns k - ks of frame f + 1.
struct WinoPatch {
    int nb, grp, bx, by, b, tx0, ty0;
    int pk_ks, pk_raw, pk_slot;      // PACK: seam after pk_ks tile columns (99: none), tcw - tx0, this patch's GroupNorm record of frame b
    bool pk_two;                     // PACK: the frame behind the seam exists
};
// Every divisor is a launch constant and every quotient is taken by the launch's reciprocals (dc, WinoRecip: n / d = (n * m) >> sh,
// exact for 0 <= n < 2^31): the decode stands in front of the first load of the kernel, where nothing hides it.
__host__ __device__ __forceinline__ int wino_div(int n, const WinoRecip r) { return (int)(((unsigned long long)(unsigned)n * r.m) >> r.sh); }
template <bool PACK>
__host__ __device__ __forceinline__ WinoPatch wino_patch(int bid, int nnb, int groups, int tbx, int tby, int pack, int W, int B, const WinoDecode dc) {
    WinoPatch q;
    q.pk_ks = 99; q.pk_raw = 99; q.pk_slot = 0; q.pk_two = false;
    int up = wino_div(bid, dc.nnb);
    q.nb = bid - up * nnb; bid = up;
    up = wino_div(bid, dc.groups);
    q.grp = bid - up * groups; bid = up;
    if constexpr (!PACK) {
        up = wino_div(bid, dc.tbx);
        q.bx = bid - up * tbx; bid = up;
        q.b = wino_div(bid, dc.tby);
        q.by = bid - q.b * tby;
        q.tx0 = q.bx * kTX;
    } else {
        const int G = pack, tcw = (W + 1) >> 1, per = tbx * tby;
        const int g = wino_div(bid, dc.per), rem = bid - g * per;
        const int nf = G < B - g * G ? G : B - g * G;          // frames of this canvas row (a ragged last group has fewer,
        const int tbxr = (nf * tcw + kTX - 1) / kTX;           // and only the patches that reach them: dc.tbxl's divisor)
        const int tbxg = tbx < tbxr ? tbx : tbxr;
        q.by = wino_div(rem, tbxg == tbx ? dc.tbx : dc.tbxl); q.bx = rem - q.by * tbxg;
        const int f = wino_div(kTX * q.bx, dc.tcw);
        q.tx0 = kTX * q.bx - f * tcw;
        q.b = g * G + f;
        q.pk_raw = tcw - q.tx0;
        q.pk_ks = q.pk_raw < kTX ? q.pk_raw : 99;
        q.pk_two = q.pk_ks < kTX && f + 1 < nf;
        q.pk_slot = q.bx - (f * tcw) / kTX;
    }
    q.ty0 = q.by * kTY;
    return q;
}
// one decoder's entry of a per-group table (ConvPtrs, a pointer), the four entries passed as VALUES: selects, no indexed read of the
// kernel argument (and no reference to it)
template <class T>
__device__ __forceinline__ T wino_group(const T v0, const T v1, const T v2, const T v3, int grp) {
    T r = v0;
    if (grp == 1) r = v1;
    if (grp == 2) r = v2;
    if (grp == 3) r = v3;
    return r;
}

// ---- input staging: per K-step the 18 x 18 region x 8 channels as LDS-DMA pieces (wave + 4 i), i < 5 (18 pieces of 1 KB).  The image
// is PERMUTED so that the fragment reads are conflict-free, and the 16-byte unit a lane's data lands in decides the global address
// it fetches (k_conv_wino, PERM): unit = (cell * 8 + block) * 16 + 4 * (qh & 3) + (ah & 3), cell = (ah >> 2) * 3 + (qh >> 2),
// block = (ry & 1) * 4 + (rx & 1) * 2 + channel half, ah = ry >> 1, qh = rx >> 1 (0..8).  The plan is fixed for the whole K loop: a
// byte offset inside the image per lane and piece (ivo; the base moves 8 floats per step) and the piece's lane mask (imask).
// up = 1: the source is read as its nearest-x2 upsample (wino_h3.hip's fold, phase 2: a lane's address is its low-resolution pixel).
// PACK: the staged region of a seam patch holds ONE gap column, tile column k reads region columns k + (k >= ks) + ch: region column
// ks holds frame f's last pixel (and the zero of x = W), column ks + 1 the zero of x = -1 and frame f + 1's first pixel.
// TR: H x W is the VIRTUAL image of a transposed launch (wino_orient_rule): its pixel (y, x) is the stored image's pixel (x, y), whose
// rows are H pixels long.  Only the lane's byte offset knows; a frame is as large either way.
// XS (the x-shared tile map, wino_frag): a lane reads the column pairs qh = 2k + s .. 2k + s + 2 of its tile pair k = 0..3 (s = 1 behind
// a seam; the seam ks is EVEN: wino_xshare_rule), so the bank slot takes the pair index, not the column's: with the LOGICAL column
// u = qh - (qh > ks), unit = ((ah >> 2) * 3 + col) * 8 + block) * 16 + 4 * ((u >> 1) & 3) + (ah & 3), col = u & 1 — the three reads of a
// lane then sit in slots 4 k, 4 k, 4 (k + 1) + (ah & 3) whatever the seam, and column pair 1 is column pair 0's unit + one cell.
// Column 2 of the cells holds what is left: u = 8 in slot group 0, and frame f's last column pair qh = ks (whose u the first pair
// behind the seam has too) in slot group ks / 2 = that of the lane that reads it as its third.  The same 9 x 8 x 16 units.
struct WinoSlot { int ah, qh, block; bool ok; };      // of a 16-byte unit: region row pair, column pair, (ry & 1) * 4 + (rx & 1) * 2 + channel half
template <bool XS>
constexpr WinoSlot wino_slot(int slot, int ks) {
    const int blk = slot >> 4, res = slot & 15, cell = blk >> 3;
    const int ah = (cell / 3) * 4 + (res & 3);
    if (!XS) return WinoSlot{ah, (cell % 3) * 4 + (res >> 2), blk & 7, true};
    const int col = cell % 3, g = res >> 2;
    const bool seam = ks < kTX;
    if (col < 2) return WinoSlot{ah, 2 * g + col + ((seam && 2 * g + col >= ks) ? 1 : 0), blk & 7, true};
    if (seam && ks > 0 && g == (ks >> 1)) return WinoSlot{ah, ks, blk & 7, true};
    return WinoSlot{ah, kTX + (seam ? 1 : 0), blk & 7, g == 0};
}
// the unit of (row pair ah, column pair qh, block) in the x-shared image (a seam patch with ks = 0 has no tile in front of the seam
// and stages nothing there: its qh = 0 has no unit)
constexpr int wino_xs_unit(int ah, int qh, int block, int ks) {
    const bool seam = ks < kTX;
    const int u = qh - ((seam && qh > ks) ? 1 : 0);
    const bool last = seam && qh == ks;      // frame f's last column pair
    const int col = (last || u == kTX) ? 2 : (u & 1), g = last ? (ks >> 1) : ((u >> 1) & 3);
    return (((ah >> 2) * 3 + col) * 8 + block) * 16 + 4 * g + (ah & 3);
}
// what unit `slot` (= 64 piece + lane) of an input buffer is filled from: whether it is staged at all, and its byte offset from the
// K-step's channels of frame b
struct WinoSrc { bool ok; unsigned off; };
template <bool PACK, bool TR = false, bool XS = false>
constexpr WinoSrc wino_stage_src(int slot, int y_in0, int x_in0, int H, int W, int Cs, int up, int pk_ks, bool pk_two) {
    const int Hs = H >> up, Ws = W >> up;                      // the source image's own size
    const WinoSlot us = wino_slot<XS>(slot, pk_ks);
    const int blk = us.block, ah = us.ah, qh = us.qh;
    const int hf = blk & 1;
    const int ry = 2 * ah + ((blk >> 2) & 1), rx = 2 * qh + ((blk >> 1) & 1);
    const bool far = PACK && qh > pk_ks;      // behind the seam: frame b + 1, one gap column in between
    const int y = y_in0 + ry, x = far ? rx - 2 * pk_ks - 3 : x_in0 + rx;
    const int qmax = (PACK && pk_ks < kTX) ? kTX + 1 : kTX;
    const bool iok = slot < kInPieces * 64 && us.ok && ah <= kTY && qh <= qmax && y >= 0 && y < H && x >= 0 && x < W && (!far || pk_two);
    const size_t px = TR ? (size_t)(x >> up) * Hs + (y >> up) : (size_t)(y >> up) * Ws + (x >> up);
    return WinoSrc{iok, iok ? (unsigned)((px * Cs + 4 * hf) * sizeof(float)) + (far ? (unsigned)((size_t)Hs * Ws * Cs * sizeof(float)) : 0u) : 0u};
}
template <bool PACK, bool TR = false, bool XS = false>
__device__ __forceinline__ void wino_stage_plan(unsigned (&ivo)[5], unsigned long long (&imask)[5], int wi, int lane, int y_in0, int x_in0, int H,
                                                int W, int Cs, int up, int pk_ks, bool pk_two) {
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const WinoSrc q = wino_stage_src<PACK, TR, XS>((wi + 4 * i) * 64 + lane, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two);
        ivo[i] = q.off;
        imask[i] = __ballot(q.ok);
    }
}
// One K-step's pieces -> the input buffer at `buf` from the image at `src` (wave-uniform).  One asm block, no branch: EXEC is set to
// each piece's lane mask (a wave-uniform 64-bit value; 0 for a piece this wave does not have or whose positions all lie outside the
// image: the instruction then moves nothing but still counts in vmcnt, so every wave issues exactly five VMEM instructions per step
// whatever the patch).  The compiler's own if (mask) form cost ~10 scalar / branch instructions per piece, in a loop that is bound
// by instruction issue.  Nothing waits here: the caller counts the five in its s_waitcnt vmcnt.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void wino_issue_in(const float* buf, int wi, const unsigned (&ivo)[5], const unsigned long long (&imask)[5], const float* src) {
    unsigned long long sv_;
    const unsigned l0_ = lds_addr(buf + wi * 256);
    asm volatile("s_mov_b64 %0, exec\n"
                 "s_mov_b64 exec, %1\n s_mov_b32 m0, %6\n s_nop 0\n global_load_lds_dwordx4 %11, %16\n"
                 "s_mov_b64 exec, %2\n s_mov_b32 m0, %7\n s_nop 0\n global_load_lds_dwordx4 %12, %16\n"
                 "s_mov_b64 exec, %3\n s_mov_b32 m0, %8\n s_nop 0\n global_load_lds_dwordx4 %13, %16\n"
                 "s_mov_b64 exec, %4\n s_mov_b32 m0, %9\n s_nop 0\n global_load_lds_dwordx4 %14, %16\n"
                 "s_mov_b64 exec, %5\n s_mov_b32 m0, %10\n s_nop 0\n global_load_lds_dwordx4 %15, %16\n"
                 "s_mov_b64 exec, %0\n"
                 : "=&s"(sv_)
                 : "s"(imask[0]), "s"(imask[1]), "s"(imask[2]), "s"(imask[3]), "s"(imask[4]),
                   "s"(l0_), "s"(l0_ + 4096), "s"(l0_ + 8192), "s"(l0_ + 12288), "s"(l0_ + 16384),
                   "v"(ivo[0]), "v"(ivo[1]), "v"(ivo[2]), "v"(ivo[3]), "v"(ivo[4]), "s"(src)
                 : "memory", "m0");
}
#pragma clang diagnostic pop

// ---- fragment addressing: this lane's tile of half 0 (half 1 = four tile rows further down = + 3 cells), the two region rows of
// transform row wi, columns 2 txl + c.  in_a[ch] / in_b[ch]: float offsets of rows ra / rb at column 2 (txl + ch) in an input buffer;
// returns the sign.  Row pair (ra, rb) and sign of B^T row wi:  0: d0-d2   1: d1+d2   2: d2-d1   3: d1-d3.  PACK: columns behind the seam lie one further.
// XS, the x-shared map: a lane's two tiles are NEIGHBOURS in x — lane li holds tiles 2k and 2k + 1, k = li & 3, of tile row li >> 2 (half
// mt = the tile column's low bit) — and share two of their four region columns: six columns c = 0..5 at 2 (2k + s) + c, tile mt
// transforms columns 2 mt .. 2 mt + 3.  in_a[0] / in_b[0]: column pair 0 (pair 1: + in_xc), in_a[1] / in_b[1]: column pair 2.
constexpr int in_cs = 2 * 16 * 4;          // + 1 column: the (rx & 1) block bit
constexpr int in_ms = 3 * 8 * 16 * 4;      // + 4 tile rows (tile half 1): the next row of cells
constexpr int in_xc = 8 * 16 * 4;          // XS: + 1 column pair from a lane's first: the next cell
template <bool PACK, bool XS = false>
__host__ __device__ __forceinline__ float wino_frag(int (&in_a)[2], int (&in_b)[2], int wi, int li, int lh, int pk_ks) {
    const int tyl = XS ? li >> 2 : li >> 3;
    const int txl = XS ? 2 * (li & 3) + ((PACK && 2 * (li & 3) >= pk_ks) ? 1 : 0) : (li & 7) + ((PACK && (li & 7) >= pk_ks) ? 1 : 0);
    const int ra = (wi == 0) ? 0 : (wi == 2 ? 2 : 1);
    const int rb = (wi == 0) ? 2 : (wi == 1 ? 2 : (wi == 2 ? 1 : 3));
    auto unit = [&](int r, int ch) {      // float offset of row 2 tyl + r, column 2 (txl + ch), this lane's channel half
        const int ah = tyl + (r >> 1), qh = txl + ch;
        if (XS) return wino_xs_unit(ah, qh, (r & 1) * 4 + lh, PACK ? pk_ks : 99) * 4;
        return ((((ah >> 2) * 3 + (qh >> 2)) * 8 + (r & 1) * 4 + lh) * 16 + 4 * (qh & 3) + (ah & 3)) * 4;
    };
    in_a[0] = unit(ra, 0); in_a[1] = unit(ra, XS ? 2 : 1);
    in_b[0] = unit(rb, 0); in_b[1] = unit(rb, XS ? 2 : 1);
    return (wi == 1) ? 1.f : -1.f;
}
// float offset of one fragment read from the pair above.  XS: column c = 0..5; else column c = 0..3 of tile half mt
template <bool XS>
__host__ __device__ __forceinline__ int wino_frag_at(const int (&in_x)[2], int mt, int c) {
    return XS ? ((c >> 1) == 2 ? in_x[1] : in_x[0] + (c >> 1) * in_xc) + (c & 1) * in_cs : in_x[c >> 1] + (c & 1) * in_cs + mt * in_ms;
}
// a patch that reaches over the image border zeroes its nbuf input buffers once (inactive DMA lanes leave them alone); an interior
// patch rewrites every unit the fragment reads touch with every step's DMA.  (A seam patch zeroes too: the units of x = W and
// x = -1 at the seam are never staged and must read zero.)
__device__ __forceinline__ void wino_zero_ring(float* lds, int t, int nbuf, int y_in0, int x_in0, int H, int W, bool seam) {
    if (y_in0 < 0 || x_in0 < 0 || y_in0 + kRH > H || x_in0 + kRW > W || seam) {
        for (int i = t; i < nbuf * kInFloats / 4; i += 256) reinterpret_cast<f32x4*>(lds)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// ---- output transform and epilogue of the accumulators acc[xi column j][tile half mt][32-channel tile nt].  Column part inside the
// wave: z0 = m0 + m1 + m2, z1 = m1 - m2 - m3; row part across the four transform-row waves through LDS: y0 = z[0] + z[1] + z[2],
// y1 = z[1] - z[2] - z[3].  The Z image in runs of 64 floats (z_run, above), one pass.  Output stage: thread = (tile of a 16-tile pass,
// 16-byte channel quad): within a ds_read_b128 lane group the 16 quads are 16 different bank slots; a wave stores 4 tiles x 256 contiguous bytes.
// out = relu(inv_s * y [+ btab by border class] [* scale] + shift [+ res]); GroupNorm records of the stored values.  No staging may
// be in flight.  Ends with the stamp record's last word (tools_dev/wino_stamps.py).
// FOLD: the bias table and nothing else (launch_conv_wino_h3 refuses scale, shift, residual and ReLU with a fold): the 64 registers of
// residual prefetch and the tests fall away at compile time.
// inv_s = 1 / (the power of two the weights were scaled by): exact; 1.0f for an unscaled image.  btab (FOLD): conv3x3(W, b 1_inside)
// by the output pixel's border class, [16][Cout].  (The pointers and the float are arguments of their own: in a struct beside the
// ints, the fold kernel kept the struct in memory.)
// TR: y, x, H, W below are the virtual image's (wino_stage_plan); the output and the residual are stored images: pixel (x, y), rows
// of H pixels.  (The fold's border classes are the virtual image's too: k_fold_compose wrote the table for the transposed taps.)
// ADDRESSES.  A thread's 16 quads (tile pass tp, output row rr and column cc of its tile) differ by wave-uniform strides: one output
// row (sy elements), one output column (sx), four tile rows = eight output rows per pass.  ONE 64-bit element offset per thread —
// its tile of pass 0, row 0, column 0 — and quad (tp, rr, cc) lies (4 tp + rr) sy + cc sx further (wino_out_step: a scalar sum); the
// residual's offset is the output's.  A seam patch has two frames and so two wave-uniform bases — frame b from tile column tx0, frame
// b + 1 from tile column -ks — of which a thread selects its side's once.  64-bit sums throughout: no size limit of its own.
struct WinoOut { long long base, sy, sx; };
template <bool PACK, bool TR>
__host__ __device__ __forceinline__ WinoOut wino_out_base(int H, int W, int Cout, int nb, int b, int ty0, int tx0, int pk_ks, int otl, int oq) {
    const long long sy = (long long)(TR ? 1 : W) * Cout, sx = (long long)(TR ? H : 1) * Cout, frame = (long long)H * W * Cout;
    const long long row = b * frame + 2 * ty0 * sy;
    const long long s_near = row + 2 * tx0 * sx, s_far = row + frame - 2 * pk_ks * sx;
    const bool far = PACK && (otl & 7) >= pk_ks;
    return WinoOut{(far ? s_far : s_near) + (otl & 7) * (2 * sx) + (otl >> 3) * (2 * sy) + nb * kBN + oq * 4, sy, sx};
}
__host__ __device__ __forceinline__ long long wino_out_step(const WinoOut o, int tp, int rr, int cc) { return (4 * tp + rr) * o.sy + cc * o.sx; }
// THE FAST EXIT is taken by a workgroup whose every pixel lies inside its frame in both axes (of the virtual image where the launch
// is transposed), a seam patch's in both frames, the second of which exists: no quad of it is tested.  pk_ks >= 8: no seam.
__host__ __device__ __forceinline__ bool wino_exit_fast(int H, int W, int ty0, int tx0, int pk_ks, bool pk_two) {
    if (2 * (ty0 + kTY) > H) return false;
    if (pk_ks >= kTX) return 2 * (tx0 + kTX) <= W;
    return (pk_ks <= 0 || 2 * (tx0 + pk_ks) <= W) && pk_two && 2 * (kTX - pk_ks) <= W;
}
// general: every workgroup takes the general exit (fpc_net_set_wino_fast_exit, fpc_conv2d's FPC_PLAN_WINO_GENERAL_EXIT requests)
struct WinoEpi { int H, W, Cout, relu, tbx, tby, pack_rx, general; };
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // (the Z stores name m0 as clobbered)
template <bool PACK, bool FOLD, bool TR = false, bool XS = false>
__device__ __forceinline__ void wino_output(float* lds, const f32x16 (&acc)[4][2][2], const ConvPtrs P, const WinoPatch pt, const WinoEpi e,
                                            const float inv_s, const float* btab, long long* dbg, const long long t_kend, const int t,
                                            const int wi, long long* fdbg = nullptr) {
    const int H = e.H, W = e.W, Cout = e.Cout;
    // (the thread's indices are rebuilt from the lane counter here instead of being carried over the K loop: the allocator otherwise
    // parks them, and whatever of the exit's addressing it can compute from them ahead of the loop, in scratch until the epilogue)
    const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int t_e = wi * 64 + lane;
    const int oq = t_e & 15, otl = t_e >> 4;                  // quad 0..15, tile 0..15 (+ 16 per tile pass)
    // (ot & 7 is the same in all four tile passes of a thread: it lies wholly on one side of a seam)
    const bool o_far = PACK && (otl & 7) >= pt.pk_ks;
    const int otx = o_far ? (otl & 7) - pt.pk_ks : pt.tx0 + (otl & 7);
    const bool o_ok = !o_far || pt.pk_two;
    const int n = pt.nb * kBN + oq * 4;
    const f32x4 e_sc = (!FOLD && P.scale) ? *reinterpret_cast<const f32x4*>(P.scale + n) : f32x4{1.f, 1.f, 1.f, 1.f};
    const f32x4 e_sh = (!FOLD && P.shift) ? *reinterpret_cast<const f32x4*>(P.shift + n) : f32x4{0.f, 0.f, 0.f, 0.f};
    // the residual of this thread's 4 x 4 outputs is requested BEFORE the output transform's barriers (one workgroup per CU: nothing
    // else hides that latency; k_conv_wino does the same)
    // (wave-uniform, all of them: the epilogue's parts and the exit path are chosen by scalar branches, once per workgroup)
    const bool has_sc = !FOLD && P.scale, has_res = !FOLD && P.res, has_relu = !FOLD && e.relu, has_gn = P.gn_part != nullptr;
    const bool fastp = !e.general && wino_exit_fast(H, W, pt.ty0, pt.tx0, PACK ? pt.pk_ks : 99, pt.pk_two);
    const WinoOut oa = wino_out_base<PACK, TR>(H, W, Cout, pt.nb, pt.b, pt.ty0, pt.tx0, pt.pk_ks, otl, oq);
    const int oy0 = 2 * (pt.ty0 + (otl >> 3)), ox0 = 2 * otx;      // quad (tp, rr, cc): pixel (oy0 + 4 tp + rr, ox0 + cc)
    f32x4 e_res[4][4];
    if (has_res && fastp) {
        const float* const rp = P.res + oa.base;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp) {
#pragma unroll
            for (int q = 0; q < 4; ++q) e_res[tp][q] = *reinterpret_cast<const f32x4*>(rp + wino_out_step(oa, tp, q >> 1, q & 1));
            __builtin_amdgcn_sched_barrier(0);      // (a pass's four sums at a time: all 16 ahead of the loads cost 32 registers the accumulators need)
        }
    } else if (!fastp) {
        const float* const rp = P.res + oa.base;
#pragma unroll
        for (int tp = 0; tp < 4; ++tp)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                e_res[tp][q] = (has_res && o_ok && oy0 + 4 * tp + (q >> 1) < H && ox0 + (q & 1) < W) ? *reinterpret_cast<const f32x4*>(rp + wino_out_step(oa, tp, q >> 1, q & 1))
                                                                                                 : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    // (fdbg: the exit's phases in a diagnostic build, ticks since the K loop's end: words 8 .. 12 of the wave's 16-word record)
    if (kWinoStamp && fdbg && (t & 63) == 0) fdbg[8] = clock64() - t_kend;      // first barrier passed
    // Z stores: accumulator register r of (mt, nt) holds, over the wave's 64 lanes, channels nt * 32 + (lane & 31) of tile rows
    // (r & 3) + 8 (r >> 2) + 4 (lane >> 5) — one RUN of 64 floats per (row wi, cc, mt, r, nt) in lane order, which is what
    // ds_write_addtid_b32 stores (address = M0 + immediate + 4 lane, no address or base register, twice ds_write_b32's rate).  Run at
    // byte z_run(cc, mt, r, nt) + 256 wi; M0 = the wave's base (16 bits) + an immediate below 64 KB reach every run from two bases.
    // (The image is the kernels' only LDS object: it starts at LDS address 0.)
    {
        const unsigned zm0 = lds_addr(lds) + wi * 256;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int cc = 0; cc < 2; ++cc)
#pragma unroll
                    for (int odd = 0; odd < 2; ++odd) {
                        const int late = XS ? mt : odd;      // the run lies in the late region, reached from the second base
                        float z[8];
#pragma unroll
                        for (int h = 0; h < 8; ++h) {
                            const int r = 2 * h + odd;
                            const float m0 = acc[0][mt][nt][r], m1 = acc[1][mt][nt][r], m2 = acc[2][mt][nt][r], m3 = acc[3][mt][nt][r];
                            z[h] = cc == 0 ? m0 + m1 + m2 : m1 - m2 - m3;
                        }
#define FPC_Z_IMM(H) "i"(z_run(cc, mt, 2 * (H) + odd, nt, XS) - late * kZOddM0)
                        asm volatile("s_mov_b32 m0, %8\n s_nop 0\n"
                                     "ds_write_addtid_b32 %0 offset:%9\n ds_write_addtid_b32 %1 offset:%10\n"
                                     "ds_write_addtid_b32 %2 offset:%11\n ds_write_addtid_b32 %3 offset:%12\n"
                                     "ds_write_addtid_b32 %4 offset:%13\n ds_write_addtid_b32 %5 offset:%14\n"
                                     "ds_write_addtid_b32 %6 offset:%15\n ds_write_addtid_b32 %7 offset:%16\n"
                                     :: "v"(z[0]), "v"(z[1]), "v"(z[2]), "v"(z[3]), "v"(z[4]), "v"(z[5]), "v"(z[6]), "v"(z[7]),
                                        "s"(zm0 + late * kZOddM0), FPC_Z_IMM(0), FPC_Z_IMM(1), FPC_Z_IMM(2), FPC_Z_IMM(3), FPC_Z_IMM(4),
                                        FPC_Z_IMM(5), FPC_Z_IMM(6), FPC_Z_IMM(7)
                                     : "memory", "m0");
#undef FPC_Z_IMM
                    }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (the compiler does not count an asm statement's stores)
    }
    if (kWinoStamp && fdbg && (t & 63) == 0) fdbg[9] = clock64() - t_kend;       // Z stores done
    __syncthreads();
    if (kWinoStamp && fdbg && (t & 63) == 0) fdbg[10] = clock64() - t_kend;      // barrier
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
    // this thread's quad of its tile of pass 0, row 0, cc 0
    const float* const zr = lds + z_read_base(otl, oq, XS) / 4;
    // (the base through an empty asm: the compiler otherwise keeps the residual prefetch's 16 sums, 32 registers, for the stores
    // across the Z stores, where the accumulators leave it none to spare)
    long long obase = oa.base;
    asm volatile("" : "+v"(obase));
    float* const op = P.out + obase;
    // The 16 quads.  FAST: the workgroup's fast exit — no test of a pixel, and the epilogue's parts are compile-time (the caller has
    // branched on them); otherwise the general exit, every quad tested against its frame, the parts by their run-time flags.  Either
    // way every value is the same sum of the same terms in the same order, and so are the GroupNorm sums (quads in (tp, rr, cc)
    // order; a launch without records accumulates none).
    auto quads = [&](auto fast_c, auto sc_c, auto res_c, auto relu_c, auto gn_c) __attribute__((always_inline)) {
    constexpr bool FAST = decltype(fast_c)::value;
    const bool do_sc = FAST ? decltype(sc_c)::value : has_sc, do_res = FAST ? decltype(res_c)::value : has_res;
    const bool do_relu = FAST ? decltype(relu_c)::value : has_relu, do_gn = FAST ? decltype(gn_c)::value : has_gn;
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        f32x4 z[4][2];
        // tile ot = otl + 16 tp of the Z image: mt = tp >> 1, r = (otl & 3) + 4 ((otl >> 3) + 2 (tp & 1)), writer half (otl >> 2) & 1
        // (XS: mt = otl & 1, r = ((otl >> 1) & 3) + 4 tp, writer half otl >> 3)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) z[i][cc] = *reinterpret_cast<const f32x4*>(zr + z_read_step(tp, cc, i, XS) / 4);
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
#pragma unroll
            for (int cc = 0; cc < 2; ++cc) {
                const int y = oy0 + 4 * tp + rr, x = ox0 + cc;
                if (!FAST && (y >= H || x >= W || !o_ok)) continue;
                f32x4 val = (rr == 0 ? z[0][cc] + z[1][cc] + z[2][cc] : z[1][cc] - z[2][cc] - z[3][cc]) * inv_s;      // (a power of two: exact)
                if (FOLD) {
                    const int cls = (((y == 0) | ((y == H - 1) << 1)) << 2) | (x == 0) | ((x == W - 1) << 1);
                    val += *reinterpret_cast<const f32x4*>(btab + (size_t)cls * Cout + n);
                }
                if (do_sc) val = val * e_sc;
                val = val + e_sh;
                if (do_res) val += e_res[tp][2 * rr + cc];
                if (do_relu) { val[0] = fmaxf(val[0], 0.f); val[1] = fmaxf(val[1], 0.f); val[2] = fmaxf(val[2], 0.f); val[3] = fmaxf(val[3], 0.f); }
                *reinterpret_cast<f32x4*>(op + wino_out_step(oa, tp, rr, cc)) = val;
                if (do_gn) { s1 += val; s2 += val * val; }
            }
    }
    };      // quads
    {
        const std::true_type yes;
        const std::false_type no;
        // one scalar branch per part, outside the 16 quads (the fold has no part but the records: launch_conv_wino_h3)
        auto part = [](bool c, auto f) __attribute__((always_inline)) { if (c) f(std::true_type()); else f(std::false_type()); };
        if (!fastp) quads(no, no, no, no, no);
        else if constexpr (FOLD) part(has_gn, [&](auto gn_c) __attribute__((always_inline)) { quads(yes, no, no, no, gn_c); });
        else
            part(has_sc, [&](auto sc_c) __attribute__((always_inline)) {
                part(has_res, [&](auto res_c) __attribute__((always_inline)) {
                    part(has_relu, [&](auto relu_c) __attribute__((always_inline)) {
                        part(has_gn, [&](auto gn_c) __attribute__((always_inline)) { quads(yes, sc_c, res_c, relu_c, gn_c); });
                    });
                });
            });
    }
    if (kWinoStamp && fdbg && (t & 63) == 0) fdbg[11] = clock64() - t_kend;      // reads, epilogue, last store issued
    if (PACK && P.gn_part) {
        // one record per frame this workgroup touches: two sets of sums, a thread's go to its side of the seam; the reduction is the
        // plain one on both.  Record of frame b: slot pk_slot of row by (pack_rx slots per row: the most patches a frame meets),
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
        if (lane < 16) {
#pragma unroll
            for (int sd = 0; sd < 2; ++sd)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    red[((sd * 4 + wi) * kBN + oq * 4 + k) * 2] = q1[sd][k];
                    red[((sd * 4 + wi) * kBN + oq * 4 + k) * 2 + 1] = q2[sd][k];
                }
        }
        __syncthreads();
        if (t_e < 2 * kBN && (t_e < kBN || pt.pk_two)) {
            const int sd = t_e >> 6, ch = t_e & (kBN - 1);
            float u1 = 0.f, u2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { u1 += red[((sd * 4 + w) * kBN + ch) * 2]; u2 += red[((sd * 4 + w) * kBN + ch) * 2 + 1]; }
            const int rx = e.pack_rx, Pn = e.tby * rx, slot = sd ? 0 : pt.pk_slot;
            float* g = P.gn_part + (((size_t)(pt.b + sd) * Pn + pt.by * rx + slot) * Cout + pt.nb * kBN + ch) * 2;
            g[0] = u1; g[1] = u2;
            if (sd == 0 && pt.pk_raw <= kTX)
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
        if (t_e < kBN) {
            float u1 = 0.f, u2 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { u1 += red[(w * kBN + t_e) * 2]; u2 += red[(w * kBN + t_e) * 2 + 1]; }
            const int Pn = e.tbx * e.tby;
            float* g = P.gn_part + (((size_t)pt.b * Pn + pt.by * e.tbx + pt.bx) * Cout + pt.nb * kBN + t_e) * 2;
            g[0] = u1; g[1] = u2;
        }
    }
    if (kWinoStamp && fdbg && lane == 0) fdbg[12] = clock64() - t_kend;          // record reduction
    if (kWinoStamp && dbg && lane == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dbg[((size_t)blockIdx.x * 4 + wi) * 8 + 7] = clock64() - t_kend;      // K loop end -> last store acknowledged
    }
}
#pragma clang diagnostic pop

// ---- host side.  What every launcher of the family checks: no stamp buffer outside a diagnostic build, groups, Cin a multiple of kch (the form's channels per K-step or pair),
// Cout of 64, 32-bit lane offsets inside one image, 31-bit buffer offsets inside one block's weight images (step_bytes per kch
// channels), the patch grid (packed: wino_pack_geometry's own; otherwise one frame per patch row) and the workgroup
// count, returned in *nblk.  (A transposed launch, a.orient: a.H x a.W is the virtual image; it packs
// with or without the fold, and a.pack = 1 is one frame per canvas row.)
inline int wino_tile_check(const WinoArgs& a, int groups, int kch, int step_bytes, bool packed, long long* nblk) {
    if (groups < 1 || groups > kMaxGroup || a.Cin % kch != 0 || a.Cout % kBN != 0 || (!kWinoStamp && a.dbg)) return FPC_EINVAL;
    if ((long long)a.H * a.W * a.Cin * (long long)sizeof(float) >= (1LL << 32)) return FPC_EINVAL;
    if ((long long)(a.Cin / kch) * step_bytes >= (1LL << 31)) return FPC_EINVAL;
    if (packed) {
        const WinoPackGeom q = wino_pack_geometry(a.H, a.W, a.B, a.Cin, a.orient ? a.pack > 1 : !a.fold);
        if (q.G != a.pack || q.tbx != a.tbx || q.tby != a.tby || q.rx != a.pack_rx) return FPC_EINVAL;
        *nblk = q.patches * (a.Cout / kBN) * groups;
    } else {
        if (a.tbx != cdiv(cdiv(a.W, 2), kTX) || a.tby != cdiv(cdiv(a.H, 2), kTY)) return FPC_EINVAL;
        *nblk = (long long)a.tbx * a.tby * a.B * (a.Cout / kBN) * groups;
    }
    return (*nblk < 1 || *nblk >= (1LL << 31)) ? FPC_EINVAL : 0;
}
}  // namespace wino_tile

// wino_h2.hip: clears the image's two-float tail, finds max |w| (of w and, if given, of w_also too: images that share one scale),
// packs.  pair = wino_h3.hip's fragment order; transpose = the image of the transposed taps (tap (r, c) read as (c, r)).
int launch_wino_pack_fp16(const float* w_oihw, float* packed, int Cout, int Cin, bool pair, const float* w_also, int Cin_also, bool transpose,
                          hipStream_t s);

}  // namespace fpc
