// net_kernels.hpp — argument structs and launch wrappers of the backbone kernels (conv_igemm.hip, wino_f32.hip and the other
// wino_*.hip, net_kernels.hip, lateral.hip, pointwise.hip, stem.hip, ...), used by the engine (net.hip).  gfx950 only.
#pragma once
#include "common.hpp"

namespace fpc {

#ifndef FPC_IGEMM_DMA_B
#define FPC_IGEMM_DMA_B 1      // split-precision k_conv_igemm: B rows staged from the bf16 planes by LDS-DMA (0: from the f32 image through registers)
#endif

constexpr int kMaxGroup = 4;      // the four FPN decoders run as one grouped launch
constexpr int kConvBK = 32;       // K-step of the implicit GEMM (floats)
constexpr int kConvNAlign = 128;  // packed weight rows are padded to a multiple of this
constexpr int kConvTickets = 16384;   // arrival counters a plan's workspace holds (fused split-K needs one per output tile)

struct ConvPtrs {
    const float* in;      // input activation
    const float* w;       // packed weights [Npad][Kpad] (OHWI, zero padded)
    float* out;           // NHWC [B,Ho,Wo,Cout]
    const float* scale;   // per-channel multiplier (folded BatchNorm) or null
    const float* shift;   // per-channel addend (folded BatchNorm / conv bias) or null
    const float* res;     // residual, same shape as out, or null
    const float* up;      // [B,Ho/2,Wo/2,Cout]: nearest-x2 upsampled and added (FPN top-down) or null
    float* gn_part;       // [B][P][Cout][2] per-32-row-tile column sums / sums of squares, or null
};

struct ConvArgs {
    ConvPtrs p[kMaxGroup];
    float* splitk_ws;     // [G][nsplit][B][mtiles*BM][Npad] raw partial sums (nsplit > 1)
    int* tickets;         // fused split-K: one arrival counter per (group, image, m tile, n tile), zero between launches
    int fused;            // nsplit > 1: 1 = the last workgroup to arrive at a tile sums the partials and applies the epilogue
                          // inside k_conv_igemm; 0 = k_conv_splitk_epilogue does (a second launch)
    int B, Hi, Wi, Cin, Ho, Wo, Cout, Npad, Kh, Kw, stride, pad, K, Kpad;
    long long in_sb, in_sh, in_sw, in_sc;   // element strides of the input
    int relu, nsplit, mtiles, ntiles, ksteps, bm, bn, generic, groups;
    int bf3;              // MODE 0 only: split-precision matrix products (three bf16 planes per operand, six MFMAs per tile)
    int h3;               // MODE 0 only: two fp16 pieces per operand, three piece products per tile; .p[g].w = the
                          // k_pack_weight_h3 image (two planes + the 1 / scale tail), not the f32 image
    int lanepx;          // MODE 0 only: 1 = a K-step is 8 consecutive pixels of `Cin / 8` channels (one kernel ROW of the
                          // stem: Kw = 1, Cin = 32 virtual channels); horizontal padding is then per lane
    const float* wino_w[kMaxGroup];   // host side only: Winograd-packed weights per group (or null)
    const float* h3_w[kMaxGroup];     // host side only: k_pack_weight_h3 images per group (or null: the site has none)
    const float* zeros;               // host side only: 64 zero floats for the all-DMA Winograd form (or null)
    // host side only, the FPN p2 fold of s2.0 (ConvPlan::fold; null where the site cannot fold): c2, the h3 images of Wc and W, p3,
    // bias table
    const float* fold_in;
    const float* fold_w[kMaxGroup];
    const float* fold_w2[kMaxGroup];
    const float* fold_up[kMaxGroup];
    const float* fold_tab[kMaxGroup];
    int fold_cin;
    float fold_lat_ms;                // tuning: the p2 lateral's best score, the fold's time must beat lateral + s2.0
    void* dbg;                        // host side only: stamp buffer of a diagnostic build (-DFPC_STAMP_IGEMM / -DFPC_STAMP_WINO), else null
    long long wino_blocks;            // host side only, written by a form-9 launch: its workgroups
    int wino_pack;                    // host side only: a form-9 launch may use the packed patch geometry (wino_pack_geometry)
    int wino_orient;                  // host side only: a form-9 launch runs transposed where wino_orient_rule says so (wino_launch_geometry)
    int wino_rowsplit;                // host side only: 1 = a packed form-9 launch keeps the row-split tile map where wino_xshare_rule offers the x-shared one
    int wino_exit_general;            // host side only: 1 = every workgroup of a four-wave Winograd launch takes the general exit (wino_tile.hpp: wino_output)
    int wino_fold_all_rows;           // host side only: 1 = every wave of the folded s2.0 runs phase 2 (0: the wave of the zero transform row only stages there, wino_h3.hip)
    int cg;                           // host side only: > 0 = a grouped 3x3 site of Cin = Cout channels in groups of cg (conv_grouped.hip) ...
    const float* grp_w;               // ... and its k_pack_grouped image
};

// FPN lateral 1x1 convolutions of all decoders as one pixel-resident product (lateral.hip): K = Cin in {64, 128}
struct LatArgs {
    const float* in;                        // [B][Ho*Wo][K] channel-last, contiguous; shared by the groups
    const unsigned short* wpl[kMaxGroup];   // k_pack_weight_bf3's planes: [3][Npad][Kpad] bf16
    float* out[kMaxGroup];                  // [B][Ho*Wo][Cout]
    const float* shift[kMaxGroup];          // conv bias or null
    const float* up[kMaxGroup];             // [B][Ho/2][Wo/2][Cout], nearest-x2 upsampled and added; all null or none
    int B, Ho, Wo, Cout, Npad, Kpad, groups, relu;
    unsigned bias_mask;                     // set by launch_lateral1x1: 0 = no bias (shift then points at readable memory)
    int parts;                              // workgroups per 128-pixel tile: each walks (groups * Cout / 32) / parts weight tiles
    int h3;                                 // 1: wpl = k_pack_weight_h3's images ([2][Npad][Kpad] fp16 + 1 / scale), three fp16
                                            // piece products per 16-deep k group
};
int launch_lateral1x1(const LatArgs& a, hipStream_t s);

// 1x1 convolution as a GEMM over all output pixels of the batch (pointwise.hip, k_conv1x1): Cin a multiple of 64, Cout of 64,
// stride 1 or 2, bf16 x 3 products on k_pack_weight_bf3's planes; the groups share the input (FPN laterals)
struct PwArgs {
    const float* in;                        // input row of output pixel (b, ho, wo): in + b in_sb + s ho in_sh + s wo in_sw (channels contiguous)
    const unsigned short* wpl[kMaxGroup];   // k_pack_weight_bf3's planes: [3][Npad][Kpad] bf16
    float* out[kMaxGroup];                  // [B * Ho * Wo][Cout]
    const float* scale[kMaxGroup];          // folded BatchNorm multiplier or null
    const float* shift[kMaxGroup];          // folded BatchNorm addend / conv bias or null
    const float* res[kMaxGroup];            // residual [B * Ho * Wo][Cout] or null
    const float* up[kMaxGroup];             // [B][Ho/2][Wo/2][Cout], nearest-x2 upsampled and added, or null
    long long in_sb, in_sh, in_sw;
    int B, Ho, Wo, Cin, Cout, Npad, Kpad, stride, groups, relu;
    int has_scale, has_shift, has_res, has_up;   // the same for every group
    int variant;                            // 0: 64-pixel tiles (4 waves), 1: 128-pixel tiles (8 waves)
};
int launch_conv1x1(const PwArgs& a, hipStream_t s);
inline int pw_tile_pixels(int variant) { return variant == 0 ? 64 : 128; }

// grouped 3x3 / pad-1 convolution of the ResNeXt encoders (conv_grouped.hip, k_conv3x3_grouped): C channels in and out,
// C / CG groups of CG channels, CG in {4, 8, 16, 32, 64}, C a multiple of 32, stride 1 or 2, plain f32 products (form 0)
struct GroupedArgs {
    const float* in;             // pixel (b, y, x): in + b in_sb + y in_sh + x in_sw, its C channels contiguous
    const float* w;              // k_pack_grouped's image (C * CG * 9 floats)
    float* out;                  // [B][Ho][Wo][C]
    const float* scale;          // folded BatchNorm multiplier or null
    const float* shift;          // folded BatchNorm addend or null
    long long in_sb, in_sh, in_sw;
    int B, Hi, Wi, Ho, Wo, C, CG, stride, relu;
    int form;                    // 0: the only form built
    int tx, ty;                  // tile columns / rows per frame: the launcher fills them
};
constexpr int kGroupedForms = 1;
bool grouped_cg_ok(int cg);
int launch_pack_grouped(const float* w_oihw, float* packed, int C, int CG, hipStream_t s, int mode = 0);      // mode: k_pack_grouped
int launch_conv3x3_grouped(const GroupedArgs& a, hipStream_t s);
inline int grouped_tile_cols(int stride) { return stride == 1 ? 16 : 8; }      // x 8 rows x 32 channels per workgroup
// (the training step's data and weight gradients of this convolution have no launcher here: conv_grouped_train.hip holds their
// kernels and the C entries fpc_conv2d_grouped_dgrad / _wgrad)

// the 7x7 / stride-2 / pad-3 stem on the NHWC4 image as a weight-resident product (stem.hip)
struct StemArgs {
    const float* in;             // [B][Hi][Wi][4] f32 (4th channel 0), contiguous
    const unsigned short* wpl;   // k_pack_weight_bf3's planes [3][Npad][Kpad = 224], k = (kh * 8 + tap) * 4 + channel
    float* out;                  // [B][Ho][Wo][Cout = 64]
    const float* scale;          // folded BatchNorm, or null
    const float* shift;
    int B, Hi, Wi, Ho, Wo, Cout, Npad, Kpad, relu;
    int grid;                    // persistent workgroups (0: one per CU of an MI355X)
};
int launch_stem7x7(const StemArgs& a, hipStream_t s);

// the stem and its 3x3 / stride-2 / pad-1 max-pool as one launch on three fp16 piece products (stem.hip, k_stem_pool_h3): the
// stem's own output is never written.  Eligible: launch_stem7x7's shapes with even Ho / Wo and ReLU on (the pool's zero padding)
struct StemPoolArgs {
    const float* in;             // [B][Hi][Wi][4] f32 (4th channel 0), contiguous
    const unsigned short* wpl;   // k_pack_weight_h3's image: [2][Npad][Kpad = 224] fp16, k = (kh * 8 + tap) * 4 + channel, then 1 / scale
    float* out;                  // the POOLED tensor [B][Hp = Ho / 2][Wp = Wo / 2][64]; every element written exactly once
    const float* scale;          // folded BatchNorm, or null
    const float* shift;
    int B, Hi, Wi, Ho, Wo, Hp, Wp, Npad, Kpad, relu;
    int band;                    // pool rows per wave task (kStemPoolBand); a shorter last band is fine
    int grid;                    // persistent workgroups (0: one per CU of an MI355X)
};
constexpr int kStemPoolBand = 10;
int launch_stem_pool_h3(const StemPoolArgs& a, hipStream_t s);
// out4 = bands, strips per frame, conv outputs the launch computes per frame, conv outputs that exist (Ho x Wo)
void stem_pool_tasks(int Ho, int Wo, int band, long long out4[4]);

constexpr int kMaxGnSites = 4;    // segmentation sites finalized by one launch (x kMaxGroup decoders each)
struct GnFinArgs {
    const float* gn_part[kMaxGnSites * kMaxGroup];   // [site * kMaxGroup + decoder]: [B][P][C][2]
    const float* gamma[kMaxGnSites * kMaxGroup];
    const float* beta[kMaxGnSites * kMaxGroup];
    float* affine[kMaxGnSites * kMaxGroup];          // [B][C][2]: y = x*a + b
    int P[kMaxGnSites];                // partial rows per image of the site's convolution plan
    long long count[kMaxGnSites];      // elements per (image, group) = Ho*Wo*C/groups
    int B, C, groups, sites;
    float eps;
};

constexpr int kMaxUpJobs = 2;     // upsample jobs (different map sizes) of one launch (x kMaxGroup decoders each)
struct GnUpArgs {
    const float* in[kMaxUpJobs * kMaxGroup];        // [job * kMaxGroup + decoder]: [B,h,w,C]
    const float* affine[kMaxUpJobs * kMaxGroup];    // [B][C][2]
    float* out[kMaxUpJobs * kMaxGroup];             // [B,2h,2w,C]
    int h[kMaxUpJobs], w[kMaxUpJobs];
    int B, C, jobs;
};

struct MergeHeadArgs {
    const float* t_lo[kMaxGroup][3];   // three [B,h,w,C] pre-GroupNorm maps, upsampled x2 after GN+ReLU
    const float* a_lo[kMaxGroup][3];   // their affines [B][C][2]
    const float* t_hi[kMaxGroup];      // [B,2h,2w,C] pre-GroupNorm map at the merge resolution
    const float* a_hi[kMaxGroup];
    const float* hw[kMaxGroup];        // head weight [Ch][C]
    const float* hb[kMaxGroup];        // head bias [Ch]
    float* out[kMaxGroup];             // low-res logits NHWC [B,2h,2w,chp]
    int ch[kMaxGroup];                 // real head channels
    int chp[kMaxGroup];                // padded (multiple of 4) channel stride of out
    int B, h, w, C;
};

// the merge + head in two passes (merge_split.hip): LOW sums the three upsampled branches at their own resolution and applies the
// head; HI applies it to the p2 branch and adds bias + the x2 upsample of LOW's result
struct HeadPartArgs {
    const float* t[kMaxGroup][3];      // pre-GroupNorm maps [B,H,W,C] of this pass (LOW: three, HI: one)
    const float* aff[kMaxGroup][3];    // their affines [B][C][2]
    const float* hw[kMaxGroup];        // head weight [Ch][C]
    const float* hb[kMaxGroup];        // head bias [Ch] (HI)
    const float* lsum[kMaxGroup];      // HI: pass LOW's output [B,hl,wl,chp]
    float* out[kMaxGroup];             // LOW: [B,H,W,chp] without bias; HI: the low-resolution logits NHWC [B,H,W,chp]
    int ch[kMaxGroup], chp[kMaxGroup];
    int B, H, W, C, hl, wl;
};
int launch_head_part(const HeadPartArgs& a, bool hi, int groups, hipStream_t s);

struct Up4Args {
    const float* lm; const float* lq; const float* lt; const float* ls;   // low-res NHWC logits (mask, quat, xyz, scales)
    int pm, pq, pt, ps;                                                   // their channel strides
    float* o_mask; float* o_quat; float* o_scales; float* o_xy; float* o_z;   // full-res NCHW logits (nullable as a set)
    long long* cat_mask; float* cq; float* cs; float* cxy; float* cz;          // categorical outputs
    int B, hl, wl, H, W, C;                                               // C classes incl. background
    unsigned long long* fg_bits; size_t fg_stride;                        // nullable: foreground bit words [B][fg_stride] (W % 64 == 0)
};

// The Winograd kernels' diagnostics (phase stamps into WinoArgs::dbg; instantiations that skip the weight reload, the staging or the
// barrier, picked by FPC_W4_MODE / FPC_H2_MODE / FPC_W2_MODE / FPC_H3_VAR / FPC_H3_ORIENT_G1; FPC_WINO_SERIAL: the serial path's phase stamps) exist in a diagnostic build only
// (-DFPC_STAMP_WINO, tools_dev/wino_stamps.py).  Elsewhere the kernels see a constant null stamp pointer, so every stamp test and
// clock read folds away, the launchers read no environment and refuse a stamp buffer.  The structs are the same in both builds.
#ifdef FPC_STAMP_WINO
constexpr bool kWinoStamp = true;
#else
constexpr bool kWinoStamp = false;
#endif
constexpr int kWinoSerialStamps = 16;      // WinoArgs::variant of a k_conv_wino_h3 launch whose stamp buffer also holds 16-word serial-path records (set by the diagnostic launcher only)

// n / d for 0 <= n < 2^31 as (n * m) >> sh in 64 bits: two scalar multiplies and a shift where a runtime division is a software
// sequence of some tens of instructions.  sh = 31 + ceil(log2 d), m = ceil(2^sh / d) < 2^32; then 2^sh <= m d <= 2^sh + 2^(sh - 31), so
// n m / 2^sh lies in [n / d, n / d + n / (2^31 d)], and n < 2^31 keeps that below the next multiple of 1 / d: the floor is n / d's
// (Granlund & Montgomery, "Division by invariant integers using multiplication", 1994, theorem 4.2 with N = 31).  1 <= d <= 2^31.
struct WinoRecip { unsigned m; int sh; };
inline WinoRecip wino_recip(unsigned d) {
    int l = 0;
    while ((1ull << l) < d) ++l;
    const int sh = 31 + l;
    return WinoRecip{(unsigned)(((1ull << sh) + d - 1) / d), sh};
}
// The divisors of the four-wave Winograd kernels' workgroup-id decode (wino_tile.hpp: wino_patch), all launch constants; filled by
// the launchers (wino_decode).  Plain: nnb, groups, tbx, tby.  Packed: nnb, groups, per = tbx * tby, tbx, tbxl = the patches per row
// of a ragged last canvas row (tbx where there is none), tcw = tile columns per frame.
struct WinoDecode { WinoRecip nnb, groups, tbx, tby, per, tbxl, tcw; };
// of a launch on a (virtual) image W pixels wide with B frames, `pack` frames per canvas row (0: a plain launch)
inline WinoDecode wino_decode(int Cout, int groups, int tbx, int tby, int W, int B, int pack) {
    const int tcw = (W + 1) / 2, last = pack > 0 ? ((B % pack) * tcw + 7) / 8 : 0;
    return WinoDecode{wino_recip(Cout / 64), wino_recip(groups), wino_recip(tbx), wino_recip(tby), wino_recip(tbx * tby),
                      wino_recip(last ? last : tbx), wino_recip(tcw)};
}

// Winograd F(2x2,3x3) convolution (3x3, stride 1, pad 1, NHWC, Cin % 8 == 0, Cout % 64 == 0)
struct WinoArgs {
    ConvPtrs p[kMaxGroup];   // .w = Winograd-packed weights [Cout/64][Cin/8][16][64][8]; .up unused
    long long* dbg;          // -DFPC_STAMP_WINO builds: per (workgroup, wave) cycle sums of the K-loop phases, or null; otherwise null
    const float* zeros;      // >= 16 bytes of zeros, 16-byte aligned (source of out-of-image DMA pieces; variant 2)
    int variant;             // 0: barrier form, 1: wave-private barrier-free K loop (4 waves), 2: all-DMA 3-stage (8 waves),
                             // 3: split-precision barrier form (8 waves; .w = the k_wino_pack_bf3 image)
    int groups;
    int waves;               // 4: 8x4 tile patch per workgroup; 8: 8x8 patch (512 threads)
    int B, H, W, Cin, Cout, relu, tbx, tby;   // tbx = ceil(ceil(W/2)/8), tby = ceil(ceil(H/2)/waves) tile patches
    // k_conv_wino_h3 only, fold = 1 (FPN p2 folded into s2.0, wino_h3.hip): out = conv3x3(Wc, in) + conv3x3(W, up2_nearest(in2))
    // + the border-class bias table; .p[g].in = c2 (Cin channels), .p[g].w = Wc's h3 image, in2 = p3 [B][H/2][W/2][Cin2]
    const float* in2[kMaxGroup];
    const float* w2[kMaxGroup];      // W's h3 image (Cin2 channels) with .p[g].w's scale (launch_wino_pack_h3_pair)
    const float* btab[kMaxGroup];    // [4 row classes][4 column classes][Cout]: class bit 0 = first row / column, bit 1 = last
    int fold, Cin2;
    // k_conv_wino_h3 only: > 1 = the patches are cut out of canvas rows of `pack` frames side by side (wino_pack_geometry's G; tbx =
    // its patches per full row), pack_rx = GroupNorm records per frame and patch row.  0 / 1: one frame per patch row, as ever
    int pack, pack_rx;
    // k_conv_wino_h3 only: 1 = the launch runs transposed (wino_orient_rule): H x W stay the stored image's, the launcher swaps them
    // for the kernel; tbx / tby / pack / pack_rx are wino_pack_geometry's on the swapped sizes (pack >= 1), the images were packed
    // from the transposed taps
    int orient;
    // k_conv_wino_h3 only: 1 = the x-shared tile map (a lane's two tiles are neighbours in x: wino_tile.hpp, XS).  Packed launches
    // (pack > 1 or orient) whose (virtual) width has an even tile-column count only: conv_plan.hpp's wino_xshare_rule
    int xshare;
    // wino_w4.hip, wino_h2.hip, wino_h3.hip: 1 = every workgroup takes the general exit, which tests each pixel against its frame
    // (0: a workgroup whose patch lies wholly inside takes the fast one; the same results bit for bit: wino_tile.hpp, wino_output)
    int exit_general;
    // wino_w4.hip, wino_h2.hip, wino_h3.hip: the reciprocals of the workgroup-id decode; the launchers fill them (callers leave them zero)
    WinoDecode dec;
    // k_conv_wino_h3 only, fold = 1: 1 = every wave runs phase 2 (0: the wave of the zero transform row only stages there; the same
    // results bit for bit on finite operands: wino_h3.hip)
    int all_rows;
};
int launch_conv_wino(const WinoArgs& a, int groups, hipStream_t s);
const float* zero_page();      // 64 zero floats in the code object (per device context), or null
int launch_wino_pack(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s);
int launch_wino_pack_bf3(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s);
// wino128.hip: the split-precision form with 128 output channels per workgroup (8 x 4 tile patch, 4 waves; Cout % 128 == 0;
// .w = the k_wino_pack_c128 fragment-order image, .waves = 4, tby = ceil(ceil(H/2)/4))
int launch_conv_wino_c128(const WinoArgs& a, int groups, hipStream_t s);
int launch_wino_pack_c128(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s);
// wino_w4.hip, wino_h2.hip, wino_h3.hip: the four-wave family (8 x 8 tile patch x 64 channels, 256 threads; what they share: wino_tile.hpp)
// wino_w4.hip: the split-precision form as four waves of 512 registers (8 x 8 tile patch x 64 channels, weights straight into the
// operand registers; .w = the k_wino_pack_bf3 image, tby = ceil(ceil(H/2)/8))
int launch_conv_wino_w4(const WinoArgs& a, int groups, hipStream_t s);
// wino_h2.hip: the four-wave form on two fp16 pieces per operand (range-limited, see the file; .w = the k_wino_pack_fp16<false> image
// incl. its two-float tail: 16 * Cout * Cin + 2 floats)
int launch_conv_wino_h2(const WinoArgs& a, int groups, hipStream_t s);
int launch_wino_pack_h2(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s);
int launch_absmax_bits(const float* w, long long n, unsigned* out_bits, hipStream_t s);      // max |w| as the bits of a non-negative float (atomicMax into *out_bits)
// act_range.hip: one pass over n contiguous floats into a 4-word record — rec[0] max |x| over the finite elements (bits, atomicMax),
// rec[1] += non-finite elements, rec[2] += n (saturating); accumulates over launches.  x 4-byte aligned; n = 0 launches nothing.
// fpc_act_range (fpc.h) is this call.
int launch_act_range(const float* x, long long n, unsigned* rec4, hipStream_t s);
// wino_h3.hip: k_conv_wino_h2 with three of the four piece products, over pairs of K-steps (Cin a multiple of 16); its own image:
// 16 * Cout * Cin + 2 floats
int launch_conv_wino_h3(const WinoArgs& a, int groups, hipStream_t s);
// its launch geometry: G frames per canvas row (1: plain), patches per full row and patch rows, GroupNorm records per frame and
// patch row, launched patches per (64-channel block, group), their tile slots, tiles that exist, GroupNorm records per frame
struct WinoPackGeom { int G, tbx, tby, rx; long long patches, slots, tiles; int gn_rows; };
WinoPackGeom wino_pack_geometry(int H, int W, int B, int Cin, bool allow);
// the orientation rule (a property of the site's shape alone) and the geometry the launch uses under it: *transposed = the launch
// runs on the virtual image W x H (the returned geometry is that image's), pack_allow governs the plain sites only
bool wino_orient_rule(int H, int W);
WinoPackGeom wino_launch_geometry(int H, int W, int B, int Cin, bool orient, bool pack_allow, bool* transposed);
int launch_wino_pack_h3(const float* w_oihw, float* packed, int Cout, int Cin, bool transpose, hipStream_t s);
// host views of the four-wave kernels' tile maps (xs: the x-shared one), for tests: fragment reads, staging plan, Z image (wino_h3.hip)
int wino_tile_frag(bool xs, int wi, int lane, int pk_ks, long long* out17);
int wino_tile_slot(bool xs, bool tr, int slot, int y_in0, int x_in0, int H, int W, int Cs, int up, int pk_ks, int pk_two, long long* out6);
int wino_tile_zrun(bool xs, int wi, int mt, int r, int nt, int cc, long long* out3);
int wino_tile_zread(bool xs, int t_e, int tp, int cc, int i, long long* out1);
// the exit: the patch decode with its fast-exit verdict, and a thread's 16 output offsets (fpc.h: fpc_wino_tile_patch, fpc_wino_tile_out)
int wino_tile_patch(bool packed, int H, int W, int B, int tbx, int tby, int pack, int patch, long long* out8);
int wino_tile_out(bool tr, int H, int W, int Cout, int nb, int b, int ty0, int tx0, int pk_ks, int t_e, long long* out16);
// the fold's weights: wc = W . L (OIHW [Cout][Cmid -> Cin][3][3], f64 sums) and the bias table conv3x3(W, bias . 1_inside) per border
// class (WinoArgs::btab); W [Cout][Cmid][3][3], L the 1x1 lateral [Cmid][Cin], bias [Cmid]
int launch_wino_pack_h3_pair(const float* w1, float* packed1, int Cin1, const float* w2, float* packed2, int Cin2, int Cout, bool transpose,
                             hipStream_t s);
int launch_fold_compose(const float* W, const float* L, const float* bias, float* wc, float* btab, int Cout, int Cmid, int Cin,
                        bool transpose, hipStream_t s);
int launch_conv(const ConvArgs& a, int groups, hipStream_t s);
int launch_conv_splitk_epilogue(const ConvArgs& a, int groups, hipStream_t s);
int launch_maxpool3x3s2(const float* in, float* out, int B, int Hi, int Wi, int C, int Ho, int Wo, hipStream_t s);
int launch_maxpool3x3s2_ceil(const float* in, float* out, int B, int Hi, int Wi, int C, hipStream_t s);      // pad 0, ceil_mode: out [B][Hi / 2][Wi / 2][C]
// se.hip: the squeeze-and-excitation gate of the SE-ResNet encoders.  NHWC f32, C % 64 == 0 (<= 8192), fixed summation orders.
// partial [B][se_pool_slabs(H, W, C)][C] per-slab channel sums; gate [B][C] = sigmoid(w2 relu(w1 mean + b1) + b2) with w1 [C / R][C],
// w2 [C][C / R]; y = max(x gate + res, 0), y == x allowed
int se_pool_slabs(int H, int W, int C);      // a function of the shape only; 0 for a refused one
int launch_se_pool(const float* x, float* partial, int B, int H, int W, int C, hipStream_t s);
int launch_se_excite(const float* partial, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, int B, int H,
                     int W, int C, int R, hipStream_t s);
int launch_se_scale_add_relu(const float* x, const float* gate, const float* res, float* y, int B, int H, int W, int C, hipStream_t s);
// launch_se_excite that also writes mean [B][C] and hidden [B][C / R] = relu(w1 mean + b1), what the backward of se_train.hip reads:
// the SAVE instantiation of the same kernel, the same operations in the same order, so the gate's bits are launch_se_excite's
int launch_se_excite_train(const float* partial, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                           float* mean, float* hidden, int B, int H, int W, int C, int R, hipStream_t s);
// the slab geometry of k_se_pool, shared with k_se_bwd_reduce (se_train.hip): the channel quads of a pixel take min(C / 4, 256)
// lanes, the rest of the workgroup takes further pixels as thread rows; a slab is se_rows(C) * kSeRowPixels pixels
constexpr int kSeThreads = 256;
constexpr int kSeRowPixels = 64;      // pixels one thread row of k_se_pool adds per slab
constexpr int kSeMaxC = 8192;         // k_se_excite keeps the means of one frame in LDS
inline int se_lanes(int C) { return C / 4 < kSeThreads ? C / 4 : kSeThreads; }
inline int se_rows(int C) { return kSeThreads / se_lanes(C); }
inline bool se_shape_ok(int B, int H, int W, int C) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 64 && C % 64 == 0 && C <= kSeMaxC && (long long)H * W < (1LL << 31) &&
           (long long)B * H * W * (C / 4) < kWalkLimit;      // (xcd_walk's 32-bit walk: launch_maxpool3x3s2's bound)
}
// mobilenet.hip: the MobileNetV2 encoder's kernels.  Dense channel-last f32, BatchNorm folded into scale / shift, act 1 = ReLU6.
// stem: in4 [B][Hi][Wi][4] -> out [B][(Hi - 1) / 2 + 1][(Wi - 1) / 2 + 1][32] with w [32][3][3][3] and ReLU6; depthwise: w [C][1][3][3],
// C % 4 == 0, stride 1 or 2; 1x1: out [M][Cout] = act(scale . in [M][Cin] w[Cout][Cin]^T + shift) (+ res, only with act 0) on exact
// f32 matrix products, Cin % 8 == 0 (<= 1024), Cout % 8 == 0 (<= 2048)
int launch_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                     hipStream_t s);
int launch_dwconv3x3(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                     int stride, int act, hipStream_t s);
int launch_conv1x1_f32(const float* in, const float* w, const float* scale, const float* shift, const float* res, float* out, long long M,
                       int Cin, int Cout, int act, hipStream_t s);
int conv1x1_f32_tiles(long long M, int Cout);      // 0: 16 x 16 tiles (few rows), else channel tiles of 32 per wave: a function of the shape alone
// efficientnet.hip (and the MB instantiations of mobilenet.hip's stem and 1x1 kernels): the EfficientNet encoder's kernels, on the
// same conventions; act 2 = swish.  The pads are efficientnet_pytorch's static "same" ones: stride 1 (k - 1) / 2 on every side;
// stride 2 (even extents only) 0 before and 1 after for k = 3, 1 and 2 for k = 5.
// depthwise: w [C][1][k][k], k 3 or 5, C % 4 == 0, out [B][Hi / stride][Wi / stride][C].  gate: per-channel means of x [B][H][W][C] in
// mb_pool_slabs(H, W, C) slabs (partial [B][slabs][C]), then gate [B][C] = sigmoid(w2 swish(w1 mean + b1) + b2) with w1 [Cs][C],
// w2 [C][Cs].  1x1: launch_conv1x1_f32's product over B frames of HW rows with in[m][k] gate[m / HW][k] as the in operand where gate
// is not NULL, Cin up to kMbMaxCin
constexpr int kMbMaxC = 2048, kMbMaxCs = 64;      // k_mb_excite keeps one frame's means and hidden activations in LDS
constexpr int kMbMaxCin = 2048;
constexpr int kMbRowPixels = 32;                  // pixels one thread row of k_mb_pool adds per slab
inline int mb_pool_lanes(int C) { return C / 4 < 256 ? C / 4 : 256; }
inline int mb_pool_slabs(int H, int W, int C) {   // a function of the shape only; 0 for a refused one
    if (H < 1 || W < 1 || C < 4 || C % 4 || C > kMbMaxC || (long long)H * W >= (1LL << 31)) return 0;
    const long long per = (long long)(256 / mb_pool_lanes(C)) * kMbRowPixels;
    return (int)(((long long)H * W + per - 1) / per);
}
inline bool mb_conv1x1_ok(int B, long long HW, int Cin, int Cout) {
    return B >= 1 && HW >= 1 && HW < (1LL << 31) && (long long)B * HW < (1LL << 31) - 64 && Cin >= 8 && Cin <= kMbMaxCin && Cin % 8 == 0 &&
           Cout >= 8 && Cout <= 2048 && Cout % 8 == 0;
}
int launch_mb_stem3x3s2(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi,
                        hipStream_t s);
int launch_mb_dwconv(const float* in, const float* w, const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C,
                     int k, int stride, int act, hipStream_t s);
int launch_mb_gate(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* gate, float* partial, int B,
                   int H, int W, int C, int Cs, hipStream_t s);
int launch_mb_conv1x1(const float* in, const float* gate, const float* w, const float* scale, const float* shift, const float* res,
                      float* out, int B, long long HW, int Cin, int Cout, int act, hipStream_t s);
// densenet.hip: the DenseNet encoders' kernels.  Channel-last f32 with row pitches: the 1x1 reads channels [0, K) of rows ldi apart
// and writes [0, Cout) of rows ldo apart, pre(v) = max(s1[k] v + t1[k], 0) on its operand where s1 is not NULL, s2 / t2 (or NULL)
// and act 1 = ReLU behind the sum; the 3x3 (128 -> 32, pad 1) reads dense [B][H][W][128] and the [9][32][128] image of
// launch_dense_pack_w and writes channels [c0, c0 + 32) of rows ldo apart.  form: -1 = the shape's own (dense_*_form), 0 / 1 forced.
constexpr int kDenseWtFloats = 9 * 32 * 128;
bool dense_pw_ok(long long M, int K, int Cout, int ldi, int ldo);
int dense_pw_form(long long M, int Cout);
int launch_dense_pw(const float* in, const float* s1, const float* t1, const float* w, const float* s2, const float* t2, float* out,
                    long long M, int K, int Cout, int ldi, int ldo, int act, int form, hipStream_t s);
int launch_dense_pack_w(const float* w, float* wt, hipStream_t s);
int dense_conv3_form(long long M);
int launch_dense_conv3(const float* in, const float* wt, float* out, int B, int H, int W, int c0, int ldo, int form, hipStream_t s);
int launch_dense_norm_pool(const float* x, const float* sc, const float* sh, float* skip, float* pooled, int B, int H, int W, int C, int act,
                           hipStream_t s);
int launch_dense_place(const float* in, float* out, long long M, int C, int ld, hipStream_t s);
// vgg.hip: the VGG encoders' two kernels.  features.0 — the dense 3x3 / stride 1 / pad 1 of the NHWC4 image [B][H][W][4] to 64 channels,
// out = act(scale[n] sum + shift[n]), scale NULL: sum + shift[n], act 1 = ReLU — and MaxPool2d(2, 2) over dense [B][H][W][C].  The _ok
// predicates are the launchers' shape checks (the plan builder asks them before it builds).  launch_fold_conv_bias: shift += scale * bias,
// a convolution's bias behind its folded BatchNorm.
bool conv3x3_c3_ok(int B, int H, int W);
int launch_conv3x3_c3(const float* in4, const float* w, const float* scale, const float* shift, float* out, int B, int H, int W, int act,
                      hipStream_t s);
bool maxpool2x2_ok(int B, int H, int W, int C);
int launch_maxpool2x2(const float* x, float* y, int B, int H, int W, int C, hipStream_t s);
int launch_fold_conv_bias(const float* scale, const float* bias, float* shift, int C, hipStream_t s);
int launch_gn_finalize(const GnFinArgs& a, int groups, hipStream_t s);
int launch_gn_relu_up2(const GnUpArgs& a, int groups, hipStream_t s);
int launch_merge_head(const MergeHeadArgs& a, int groups, hipStream_t s);
int launch_up4_compress(const Up4Args& a, hipStream_t s, bool allow_wide = true);      // allow_wide = false: 9 to 32 classes keep k_up4_compress<32>
void launch_up4_compress7x4(const Up4Args& a, hipStream_t s);   // up4.hip; preconditions checked by launch_up4_compress
void launch_up4_compress_wide(const Up4Args& a, hipStream_t s);  // up4.hip, 9 to 32 classes; preconditions checked by launch_up4_compress

// bilinear source coordinate, align_corners=True, torch's arithmetic (UpSample.cuh):
// src = dst * (in-1)/(out-1) in f32; i0 = (int)src; l1 = src - i0; i1 = i0 + (i0 < in-1)
struct Lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lerp lerp_coord(int dst, int in, int out) {
    float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    float src = scale * (float)dst;
    Lerp L;
    L.i0 = (int)src;
    L.i1 = L.i0 + (L.i0 < in - 1 ? 1 : 0);
    L.l1 = src - (float)L.i0;
    L.l0 = 1.f - L.l1;
    return L;
}

// lerp_coord with the scale (in - 1) / (out - 1) computed by the caller once
__device__ __forceinline__ Lerp lerp_scaled(int dst, int in, float scale) {
    float src = scale * (float)dst;
    Lerp L;
    L.i0 = (int)src;
    L.i1 = L.i0 + (L.i0 < in - 1 ? 1 : 0);
    L.l1 = src - (float)L.i0;
    L.l0 = 1.f - L.l1;
    return L;
}

int launch_pack_weight(const float* w_oihw, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                       int Kpad, hipStream_t s);
// + the three bf16 planes of the same image behind it (packed + Npad * Kpad floats; 1.5 x Npad * Kpad floats more):
// the weight operand of the split-precision direct convolution.  conv_packed_floats() = the room both need.
int launch_pack_weight_bf3(const float* w_oihw, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                           int Kpad, hipStream_t s);
inline size_t conv_packed_floats(int Npad, int Kpad) { return ((size_t)Npad * Kpad * 5 / 2 + 63) / 64 * 64; }
// The same image as two fp16 planes [2][Npad][Kpad] (Npad * Kpad floats) scaled by ONE power of two s per convolution (max |w| s
// < 2^13, set on the device from max |w|), then a tail of 2 floats: 1 / s and max |w|'s bits — the weight operand of
// k_conv_igemm's three-product form (ConvArgs::h3).  h3_packed_floats() = its room.
int launch_pack_weight_h3(const float* w_oihw, float* packed, int Cout, int Cin, int Cinp, int Kh, int Kw, int Kwp, int Npad,
                          int Kpad, hipStream_t s);
inline size_t h3_packed_floats(int Npad, int Kpad) { return ((size_t)Npad * Kpad + 2 + 63) / 64 * 64; }
int launch_nchw3_to_nhwc4(const float* x, float* out, int B, int HW, hipStream_t s);
int launch_fold_bn(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
                   float* scale, float* shift, hipStream_t s);

}  // namespace fpc
