// conv_plan.hpp — the convolution planner of the backbone engine, host arithmetic only: what a packed convolution site and a launch plan are, which
// kernel forms a site may run on, the heuristic plan and the tilings the autotuner may try, the Winograd forms with the weight images they read, the plan
// codes (fpc.h, FPC_PLAN_*).  Shared by the engine (net_plan.hpp: net_build.hip, net.hip), conv_launch.hip (a plan's launch) and conv2d.hip (the stand-alone fpc_conv2d* entries).
#pragma once
#include <math.h>
#include <string.h>

#include <vector>

#include "net_kernels.hpp"

#define FPC_TRY(x) do { int rc__ = (x); if (rc__) return rc__; } while (0)

namespace fpc {

struct PackedConv {
    int Cin = 0, Cinp = 0, Cout = 0, Kh = 1, Kw = 1, stride = 1, pad = 0;   // Cinp: channels of the input LAYOUT
    int Kwp = 1;             // taps per kernel row in the packed layout (= Kw; 8 for the stem's row-per-K-step form)
    int K = 0, Kpad = 0, Npad = 0;
    int p_w = -1;            // parameter index of the OIHW weight
    int p_bn = -1;           // first of (weight, bias, running_mean, running_var) or -1
    int p_bias = -1;         // conv bias or -1
    size_t w_off = 0, scale_off = 0, shift_off = 0;   // float offsets into the workspace
    size_t wino_off = 0;     // Winograd-packed copy (eligible convs only)
    bool wino_ok = false;    // 3x3, stride 1, pad 1, Cin % 8 == 0, Cout % 64 == 0
    size_t h3_off = 0;       // k_pack_weight_h3's image (h3_ok sites only)
    bool h3_ok = false;      // a candidate of k_conv_igemm's three-product form: the direct sites of ResNet-18/34 plans that do not
                             // run on Winograd — the stride-2 3x3 and 1x1 convolutions and the p5 / p4 / p3 laterals
    int cg = 0;              // > 0: a grouped 3x3 site (conv_grouped.hip) of Cin = Cout channels in groups of cg; K = 9 cg.  It has
    size_t grp_off = 0;      // k_pack_grouped's image only (no implicit-GEMM, Winograd or h3 image)
};

struct Act { size_t off = 0; int H = 0, W = 0, C = 0; };

struct ConvPlan {
    int bm = 64, bn = 64, nsplit = 1, mtiles = 1, ntiles = 1, wino = 0, bf3 = 0, fused = 0;
    int lat = 0;             // > 0: k_lateral1x1 with this many workgroups per 128-pixel tile (lateral.hip) instead of k_conv_igemm
    int stem = 0;            // > 0: k_stem7x7 (stem.hip), a persistent grid of this many workgroups (one per CU: 256)
    int pw = 0;              // > 0: k_conv1x1 (pointwise.hip), variant pw - 1 (net_kernels.hpp: PwArgs::variant)
    int fold = 0;            // s2.0 with wino 9 only: the FPN p2 level folded into the launch (wino_h3.hip, FOLD); no p2 lateral runs
    int h3 = 0;              // k_conv_igemm on two fp16 pieces, three piece products (ConvArgs::h3; PackedConv::h3_ok sites)
    int pool = 0;            // the stem site only (with stem > 0): k_stem_pool_h3 writes the pooled tensor, no stem output, no max-pool launch
    int grp = 0;             // > 0: k_conv3x3_grouped (conv_grouped.hip), form grp - 1; the only plans of a PackedConv::cg site
};

// the 7x7 / stride-2 / pad-3 stem in its row-per-K-step layout (NHWC4 image, 8 taps x 4 channels per kernel row, K = 224) with a
// BatchNorm / bias-only epilogue and an output row that divides into 64-pixel segments
inline bool stem_ok(const ConvArgs& a) {
    return a.lanepx == 1 && a.generic == 0 && a.Kh == 7 && a.stride == 2 && a.pad == 3 && a.Cout == 64 && a.Kpad == 224 &&
           a.Wo % 64 == 0 && !a.p[0].res && !a.p[0].up && !a.p[0].gn_part && a.in_sc == 1 && a.in_sw == 4 &&
           a.in_sh == (long long)4 * a.Wi && a.in_sb == (long long)4 * a.Hi * a.Wi;
}

// a grouped 1x1 / stride-1 site with K = 64 or 128, bias-only epilogue and one input shared by the groups: the FPN laterals
// of the stride-4 and stride-8 maps (and fpc_conv2d's test hook)
inline bool lateral_ok(const ConvArgs& a, int groups) {
    if (a.Kh != 1 || a.Kw != 1 || a.stride != 1 || a.pad != 0 || a.generic != 0 || (a.Cin != 64 && a.Cin != 128) || a.Kpad != a.Cin ||
        a.Cout % 32 != 0 || a.in_sc != 1 || a.in_sw != a.Cin || a.in_sh != (long long)a.Wi * a.Cin ||
        a.in_sb != (long long)a.Hi * a.Wi * a.Cin || a.lanepx)
        return false;
    for (int g = 0; g < groups; ++g)
        if (a.p[g].in != a.p[0].in || a.p[g].scale || a.p[g].res || a.p[g].gn_part || ((a.p[g].up != nullptr) != (a.p[0].up != nullptr)))
            return false;
    return !(a.p[0].up && ((a.Ho | a.Wo) & 1));
}

// a 1x1 site k_conv1x1 takes: K a multiple of 64, Cout of 64, stride 1 or 2, channel-contiguous input shared by the groups,
// no GroupNorm partials and the same epilogue operands in every group
inline bool pw_ok(const ConvArgs& a, int groups) {
    if (a.Kh != 1 || a.Kw != 1 || a.pad != 0 || (a.stride != 1 && a.stride != 2) || a.generic != 0 || a.lanepx || a.Cin % 64 != 0 ||
        a.Kpad != a.Cin || a.Cout % 64 != 0 || a.in_sc != 1)
        return false;
    for (int g = 0; g < groups; ++g)
        if (a.p[g].in != a.p[0].in || a.p[g].gn_part || (a.p[g].scale != nullptr) != (a.p[0].scale != nullptr) ||
            (a.p[g].shift != nullptr) != (a.p[0].shift != nullptr) || (a.p[g].res != nullptr) != (a.p[0].res != nullptr) ||
            (a.p[g].up != nullptr) != (a.p[0].up != nullptr))
            return false;
    return !(a.p[0].up && ((a.Ho | a.Wo) & 1));
}

// fused split-K (ConvArgs::fused) needs one arrival counter per output tile
inline bool can_fuse(const ConvPlan& p, int groups, int B) {
    return p.nsplit > 1 && (long long)groups * B * p.mtiles * p.ntiles <= kConvTickets;
}

inline ConvPlan plan_conv(int HoWo, int B, int Cout, int ksteps, int groups, int force_bm = 0, int force_bn = 0,
                          int force_split = 0) {
    ConvPlan best;
    double best_t = 1e300;
    const int bms[2] = {64, 128}, bns[2] = {64, 128};
    for (int bi = 0; bi < 2; ++bi)
        for (int bj = 0; bj < 2; ++bj) {
            int bm = bms[bi], bn = bns[bj];
            if (force_bm && bm != force_bm) continue;
            if (force_bn && bn != force_bn) continue;
            if (!force_bn && bn == 128 && Cout <= 64) continue;
            int mt = cdiv(HoWo, bm), nt = cdiv(Cout, bn);
            for (int ns = 1; ns <= 32; ++ns) {
                if (force_split && ns != force_split) continue;
                int per = cdiv(ksteps, ns);
                if ((ns - 1) * per >= ksteps) continue;
                if (ns > 1 && (Cout % 4 != 0)) continue;
                double nblk = (double)groups * B * mt * nt * ns;
                double work = (double)(bm / 64) * (bn / 64) * per * 16.0 * 64.0 + 4000.0;
                double t = ceil(nblk / 256.0) * work + (ns > 1 ? 10000.0 + 200.0 * ns : 0.0);
                if (t < best_t) { best_t = t; best = ConvPlan{bm, bn, ns, mt, nt, 0}; }
            }
        }
    best.fused = can_fuse(best, groups, B) ? 1 : 0;
    return best;
}

// Tilings the autotuner may try for one convolution site (the heuristic plan is always among them).
inline std::vector<ConvPlan> conv_candidates(int HoWo, int B, int Cout, int ksteps, int groups) {
    std::vector<ConvPlan> out;
    const int splits[] = {1, 2, 3, 4, 6, 8, 12, 16, 24};
    for (int bm = 64; bm <= 128; bm += 64)
        for (int bn = 64; bn <= 128; bn += 64) {
            if (bn == 128 && Cout <= 64) continue;
            int mt = cdiv(HoWo, bm), nt = cdiv(Cout, bn);
            long long base = (long long)groups * B * mt * nt;
            for (int ns : splits) {
                int per = cdiv(ksteps, ns);
                if (ns > 1 && (per < 2 || (ns - 1) * per >= ksteps || Cout % 4 != 0)) continue;
                if (ns > 1 && base * ns > 4096) continue;          // already plenty of workgroups
                out.push_back(ConvPlan{bm, bn, ns, mt, nt, 0});
                if (can_fuse(out.back(), groups, B)) { ConvPlan f = out.back(); f.fused = 1; out.push_back(f); }
            }
        }
    return out;
}

inline size_t splitk_floats_for(const ConvPlan& p, int groups, int B, int Npad) {
    return p.nsplit > 1 ? (size_t)groups * p.nsplit * B * p.mtiles * p.bm * Npad : 0;
}

// ---- the Winograd forms (ConvPlan::wino = 1..9, reported and requested as -form) and the weight images they read.
// A new form adds: one row of kWinoForms, one entry of kWinoImages if it reads an image of its own, and its launcher.
// A site's image region holds the images in the order of kWinoImages, each `units` x Cout x Cin floats followed by `tail` floats; the
// 128-channel form's image is there only where Cout % 128 == 0.  Behind the last image the region keeps kWinoSlack floats.
enum WinoImage { kImgF32, kImgBf3, kImgC128, kImgH2, kImgH3, kWinoImageCount };
struct WinoImageDesc { int units, tail; int (*pack)(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s); };
inline int pack_h3_plain(const float* w_oihw, float* packed, int Cout, int Cin, hipStream_t s) { return launch_wino_pack_h3(w_oihw, packed, Cout, Cin, false, s); }
constexpr WinoImageDesc kWinoImages[kWinoImageCount] = {
    {16, 0, launch_wino_pack},            // f32
    {24, 0, launch_wino_pack_bf3},        // split precision: three bf16 planes
    {24, 0, launch_wino_pack_c128},       // ... in the 128-channel form's fragment order (wino128.hip)
    {16, 8, launch_wino_pack_h2},         // two fp16 pieces in fragment order (wino_h2.hip); the tail: its two scale floats, kept 32-byte aligned
    {16, 8, pack_h3_plain},               // ... in pair order (wino_h3.hip), with the same tail; a transposed site's: pack_wino_h3_image
};
constexpr size_t kWinoSlack = 128;      // a 64-float line for the tails + 64 zero floats (fpc_conv2d's zero page where the code object has none)

constexpr int kWinoFormCount = 10;      // forms 1..9; row 0 is "not Winograd"
constexpr int kWinoBf3 = 5, kWinoW4 = 7;     // the range-free split-precision forms a guarded site falls back to (-7 where offered, else -5)
constexpr int kWinoH2 = 8, kWinoH3 = 9;      // the fp16 x 2 form and its three-product form: the one launch that may pack frames or fold p2 in
struct WinoForm {
    int waves;               // 4: 8 x 4 tile patch per workgroup, 8: 8 x 8
    int bn, ck;              // output channels per workgroup; input channels per K-loop step: Cout and Cin are multiples of these
    int variant;             // WinoArgs::variant
    WinoImage image;
    int wg_per_cu;           // workgroups of the form that share a CU (the tuner's occupancy share)
    int min_split;           // lowest fpc_net_set_split_precision level at which the tuner offers the form
    bool zeros;              // reads the zero page (WinoArgs::zeros)
    bool range_limited;      // two fp16 pieces per operand: the activation envelope of fpc.h (fpc_net_guard_ranges demotes such a site)
    int (*launch)(const WinoArgs& a, int groups, hipStream_t s);
};
constexpr WinoForm kWinoForms[kWinoFormCount] = {
    {},
    {4, 64, 8, 0, kImgF32, 2, 0, false, false, launch_conv_wino},      // -1: 4 waves
    {8, 64, 8, 0, kImgF32, 1, 0, false, false, launch_conv_wino},      // -2: 8 waves
    {4, 64, 8, 1, kImgF32, 2, 0, false, false, launch_conv_wino},      // -3: wave-private K loop
    {8, 64, 8, 2, kImgF32, 1, 0, true, false, launch_conv_wino},       // -4: all-DMA 3-stage
    {8, 64, 8, 3, kImgBf3, 1, 1, true, false, launch_conv_wino},       // -5: split-precision products, 8 waves
    {4, 128, 8, 0, kImgC128, 1, 1, false, false, launch_conv_wino_c128},      // -6: ... 8 x 4 tiles x 128 channels per workgroup, 4 waves (wino128.hip)
    {8, 64, 8, 0, kImgBf3, 1, 1, false, false, launch_conv_wino_w4},   // -7: ... 64 channels, four waves of 512 registers, weights direct (wino_w4.hip)
    {8, 64, 8, 0, kImgH2, 1, 2, false, true, launch_conv_wino_h2},     // -8: the -7 form on two fp16 pieces per operand (range-limited: fpc.h; wino_h2.hip)
    {8, 64, 16, 0, kImgH3, 1, 3, false, true, launch_conv_wino_h3},    // -9: three of the four piece products of -8, over pairs of K-steps (wino_h3.hip)
};
// the shape rules of a form, on top of PackedConv::wino_ok
inline bool wino_form_ok(int form, int Cin, int Cout) {
    return form >= 1 && form < kWinoFormCount && Cout % kWinoForms[form].bn == 0 && Cin % kWinoForms[form].ck == 0;
}
// units and tail floats of the images in front of image `end`; c128: the region has the 128-channel form's image
struct WinoSpan { size_t units, tails; };
inline WinoSpan wino_span(int end, bool c128) {
    WinoSpan sp{0, 0};
    for (int i = 0; i < end; ++i)
        if (i != kImgC128 || c128) { sp.units += kWinoImages[i].units; sp.tails += kWinoImages[i].tail; }
    return sp;
}
static_assert(kWinoImages[kImgH2].tail + kWinoImages[kImgH3].tail <= 64, "kWinoSlack keeps one 64-float line for all tails");
// float offset of image `img` in a site's region
inline size_t wino_image_offset(WinoImage img, int Cout, int Cin) {
    const WinoSpan sp = wino_span(img, Cout % 128 == 0);
    return sp.units * Cout * Cin + sp.tails;
}
// floats of a region that ends with image `last`: what one form needs (fpc_conv2d's exact workspace), and with the last image of
// all what a site needs (fpc_net::add_conv); c128 = true bounds both (fpc_conv2d_workspace_bytes)
inline size_t wino_region_floats(WinoImage last, int Cout, int Cin, bool c128) { return (wino_span(last, c128).units + kWinoImages[last].units) * Cout * Cin + kWinoSlack; }
// a plan whose matrix products run on two fp16 pieces per operand, i.e. under the activation envelope: the range-limited Winograd
// forms (packed or not, with or without the p2 fold), the three-product direct and lateral forms, the stem fused with its max-pool
inline bool plan_range_limited(const ConvPlan& p) {
    return p.h3 || p.fold || p.pool || (p.wino && kWinoForms[p.wino].range_limited);
}
// tile patches of one frame: tbx x tby workgroups per (frame, channel block, group)
struct WinoGrid { int tbx, tby; int patches() const { return tbx * tby; } };
inline WinoGrid wino_grid(int form, int H, int W) { return {cdiv(cdiv(W, 2), 8), cdiv(cdiv(H, 2), kWinoForms[form].waves)}; }

// The X-SHARE RULE of a packed form-9 launch (pack > 1 or transposed) on a (virtual) image W pixels wide: the x-shared tile map
// (wino_tile.hpp, XS: a lane's two tiles are the neighbours 2k, 2k + 1 of one tile row and share half their input columns) iff the
// frame has an EVEN number of tile columns tcw.  A packed patch's seam lies after tcw (f + 1) - 8 bx tile columns: with tcw even it
// is even, falls between two lanes' pairs, and both tiles of a lane lie on one side of it.  Otherwise the row-split map, as ever.
inline bool wino_xshare_rule(int W) { return (((W + 1) >> 1) & 1) == 0; }

// ---- the integer a plan is reported by (fpc_net_conv_plan's out5[2]) and requested by (fpc_conv2d's `nsplit`): fpc.h, FPC_PLAN_*.
// What a request asks for (nsplit: the split-K factor, 0 = the planner's, or -form; wino: the form or 0):
struct Conv2dRequest { int nsplit; bool bf3, two_launch; int wino, lat; bool stem; int pw; bool h3, pool, pack, orient; int grp; bool rowsplit, exit_general; };
inline Conv2dRequest decode_plan(int code) {
    Conv2dRequest r{code, false, false, 0, 0, false, 0, false, false, false, false, 0, false, false};
    // -107 .. -113: the four-wave forms -7 .. -13 with every workgroup on the general exit (the two exits' A/B)
    if (code <= FPC_PLAN_WINO_GENERAL_EXIT - kWinoW4 && code >= FPC_PLAN_WINO_GENERAL_EXIT + FPC_PLAN_WINO_ORIENT_ROWSPLIT) {
        r.exit_general = true;
        code -= FPC_PLAN_WINO_GENERAL_EXIT;
        r.nsplit = code;
    }
    // -12 / -13: -10 / -11 on the row-split tile map even where wino_xshare_rule offers the x-shared one (the two maps' A/B)
    if (code == FPC_PLAN_WINO_PACKED_ROWSPLIT) { r.rowsplit = true; code = FPC_PLAN_WINO_PACKED; }
    if (code == FPC_PLAN_WINO_ORIENT_ROWSPLIT) { r.rowsplit = true; code = FPC_PLAN_WINO_ORIENT; }
    if (code >= FPC_PLAN_GROUPED && code < FPC_PLAN_GROUPED + 1000) { r.grp = code - FPC_PLAN_GROUPED + 1; r.nsplit = 1; return r; }      // + form = k_conv3x3_grouped (fpc_conv2d_grouped's request; fpc_conv2d has no groups and refuses it)
    if (code == FPC_PLAN_WINO_ORIENT) { r.orient = true; r.nsplit = -kWinoH3; }      // form -9 in the orientation its shape asks for (wino_orient_rule), transposed sites packed along y
    if (code == FPC_PLAN_WINO_PACKED) { r.pack = true; r.nsplit = -kWinoH3; }      // form -9 with its patches cut out of canvas rows of several frames (wino_pack_geometry)
    if (r.nsplit >= FPC_PLAN_LATERAL_H3 && r.nsplit < FPC_PLAN_LATERAL_H3 + 1000) { r.lat = r.nsplit - FPC_PLAN_LATERAL_H3; r.h3 = true; r.nsplit = 1; return r; }      // + parts = k_lateral1x1 on two fp16 pieces
    if (r.nsplit >= FPC_PLAN_H3 && r.nsplit < FPC_PLAN_H3 + 200) { r.h3 = true; r.nsplit -= FPC_PLAN_H3; }      // + split = k_conv_igemm's three-product form; what is left (< 200) reaches the two-launch line only
    if (r.nsplit >= FPC_PLAN_POINTWISE) { r.pw = r.nsplit - FPC_PLAN_POINTWISE + 1; r.bf3 = true; r.nsplit = 1; return r; }   // + variant = k_conv1x1 (pointwise.hip)
    if (r.nsplit == FPC_PLAN_STEM_POOL) { r.stem = true; r.pool = true; r.h3 = true; r.nsplit = 1; return r; }     // k_stem_pool_h3: NHWC4 input, `out` = the POOLED tensor
    if (r.nsplit == FPC_PLAN_STEM) { r.stem = true; r.bf3 = true; r.nsplit = 1; return r; }                   // k_stem7x7 (stem.hip): NHWC4 input
    if (r.nsplit >= FPC_PLAN_LATERAL) { r.lat = r.nsplit - FPC_PLAN_LATERAL; r.bf3 = true; r.nsplit = 1; return r; }      // + parts = k_lateral1x1 (lateral.hip)
    if (r.nsplit >= FPC_PLAN_BF3) { r.bf3 = true; r.nsplit -= FPC_PLAN_BF3; }          // + split = split-precision matrix products
    if (r.nsplit >= FPC_PLAN_TWO_LAUNCH) { r.two_launch = true; r.nsplit -= FPC_PLAN_TWO_LAUNCH; }      // + split = split-K summed by k_conv_splitk_epilogue
    if (r.nsplit <= -1 && r.nsplit > -kWinoFormCount) r.wino = -r.nsplit;      // -form: kWinoForms
    return r;
}
// What a plan reports; folded_away: the p2 lateral site while s2.0 runs with that level folded in (never a request)
inline int encode_plan(const ConvPlan& p, bool folded_away) {
    if (folded_away) return FPC_PLAN_FOLDED;
    if (p.grp) return FPC_PLAN_GROUPED + p.grp - 1;
    // the three-product form: k_conv_igemm + split (fused or not, as the plain tilings), k_lateral1x1 + parts
    if (p.h3) return p.lat ? FPC_PLAN_LATERAL_H3 + p.lat : FPC_PLAN_H3 + p.nsplit;
    if (p.pw) return FPC_PLAN_POINTWISE + p.pw - 1;
    if (p.stem) return p.pool ? FPC_PLAN_STEM_POOL : FPC_PLAN_STEM;
    if (p.lat) return FPC_PLAN_LATERAL + p.lat;
    return p.wino ? -p.wino : p.nsplit;
}

inline int conv_out(int x, int k, int s, int p) { return (x + 2 * p - k) / s + 1; }
// fills the shape and plan part of ConvArgs from conv `c` + plan `p` for a batch of B; the caller adds its workspace pointers
inline void fill_conv_shape(ConvArgs& a, int B, const PackedConv& c, const ConvPlan& p, int Hi, int Wi, int Ho, int Wo, long long sb,
                            long long sh, long long sw, long long sc, bool relu, int mode) {
    memset(&a, 0, sizeof(a));
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Cin = c.Cin; a.Ho = Ho; a.Wo = Wo; a.Cout = c.Cout; a.Npad = c.Npad;
    a.Kh = c.Kh; a.Kw = c.Kw; a.stride = c.stride; a.pad = c.pad; a.K = c.K; a.Kpad = c.Kpad;
    a.in_sb = sb; a.in_sh = sh; a.in_sw = sw; a.in_sc = sc;
    a.relu = relu ? 1 : 0; a.nsplit = p.nsplit; a.mtiles = p.mtiles; a.ntiles = p.ntiles; a.ksteps = c.Kpad / kConvBK;
    a.bm = p.bm; a.bn = p.bn; a.generic = mode;
    a.fused = p.fused;
}

// ---- conv_launch.hip: one launch of site `a` on plan `p`, whichever kernel the plan names (FPC_EINVAL where the form refuses the
// site), the GroupNorm partial rows per image a plan writes, and the stem site's fused launch to the pooled tensor
int launch_conv_plan(ConvArgs& a, const ConvPlan& p, int groups, hipStream_t s);
int plan_gn_rows(const ConvPlan& p, int Ho, int Wo, int B, int Cin, int pack, int orient);
int launch_stem_pool(const ConvArgs& a, const float* h3_image, float* pool, int Hp, int Wp, hipStream_t s);

}  // namespace fpc
