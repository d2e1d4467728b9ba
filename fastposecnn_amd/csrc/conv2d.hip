// conv2d.hip — the stand-alone convolution entry points of include/fpc.h, outside any network: fpc_conv2d* (one convolution on any plan code, for unit
// tests, micro-benchmarks and the training path), fpc_conv2d_grouped*, and the host-arithmetic exports of the launch geometry (fpc_stem_pool_tasks, fpc_xcd_order,
// fpc_wino_pack_geometry, fpc_wino_orient_geometry, fpc_wino_recip, fpc_wino_decode, fpc_wino_xshare_rule, fpc_wino_tile_*).  They plan with conv_plan.hpp and launch through conv_launch.hip.
#include <algorithm>

#include "conv_device.hpp"
#include "conv_plan.hpp"

using namespace fpc;

// k_stem_pool_h3's wave tasks for a conv output of Ho x Wo (host arithmetic, no device): out4 = bands, strips per frame, conv outputs
// computed per frame (band overlap rows and halo tiles included), conv outputs that exist.  FPC_EINVAL for a shape the launcher refuses.
extern "C" int fpc_stem_pool_tasks(int Ho, int Wo, int64_t* out4) {
    if (!out4 || Ho < 2 || (Ho & 1) || Wo < 64 || (Wo & 63)) return FPC_EINVAL;
    long long o[4];
    stem_pool_tasks(Ho, Wo, kStemPoolBand, o);
    for (int i = 0; i < 4; ++i) out4[i] = o[i];
    return FPC_OK;
}

// The XCD-banded workgroup order (conv_device.hpp; host arithmetic, no device): out4 = xcd_logical(block, grid), then first, end and
// step of xcd_span(total, per_block, slot, block, grid).
extern "C" int fpc_xcd_order(int grid, int block, int64_t total, int per_block, int slot, int64_t* out4) {
    if (!out4 || grid < 1 || block < 0 || block >= grid || per_block < 1 || slot < 0 || slot >= per_block || total < 0 || total >= kWalkLimit)
        return FPC_EINVAL;
    const XcdSpan w = xcd_span((unsigned)total, (unsigned)per_block, (unsigned)slot, (unsigned)block, (unsigned)grid);
    out4[0] = xcd_logical((unsigned)block, (unsigned)grid); out4[1] = w.first; out4[2] = w.end; out4[3] = w.step;
    return FPC_OK;
}

// k_conv_wino_h3's launch geometry for a 3x3 / stride-1 site with output H x W, batch B and Cin input channels (host arithmetic, no
// device; fold = 1: the folded s2.0, which never packs): out8 = frames per canvas row G (1: plain), patches per full canvas row,
// patch rows, launched patches per (64-channel block, decoder), their tile slots, tiles that exist, GroupNorm records per frame,
// GroupNorm records per frame and patch row.
extern "C" int fpc_wino_pack_geometry(int H, int W, int B, int Cin, int fold, int64_t* out8) {
    if (!out8 || H < 1 || W < 1 || B < 1 || Cin < 1) return FPC_EINVAL;
    const WinoPackGeom q = wino_pack_geometry(H, W, B, Cin, !fold);
    out8[0] = q.G; out8[1] = q.tbx; out8[2] = q.tby; out8[3] = q.patches; out8[4] = q.slots; out8[5] = q.tiles; out8[6] = q.gn_rows;
    out8[7] = q.rx;
    return FPC_OK;
}

// The same for a site under the orientation rule (wino_orient_rule / wino_launch_geometry; host arithmetic): out9[0] = 1 where the
// launch runs transposed — then out9[1..8] is fpc_wino_pack_geometry's out8 of the virtual image W x H, packed whatever `pack` says
// and with or without the fold — else 0 and out9[1..8] = the plain site's geometry with packing as `pack` (0 / 1) allows.
extern "C" int fpc_wino_orient_geometry(int H, int W, int B, int Cin, int fold, int pack, int64_t* out9) {
    if (!out9 || H < 1 || W < 1 || B < 1 || Cin < 1) return FPC_EINVAL;
    bool tr;
    const WinoPackGeom q = wino_launch_geometry(H, W, B, Cin, true, pack && !fold, &tr);
    out9[0] = tr ? 1 : 0;
    out9[1] = q.G; out9[2] = q.tbx; out9[3] = q.tby; out9[4] = q.patches; out9[5] = q.slots; out9[6] = q.tiles; out9[7] = q.gn_rows;
    out9[8] = q.rx;
    return FPC_OK;
}

// The reciprocals of the four-wave Winograd kernels' workgroup-id decode (wino_recip, wino_decode: host arithmetic), as the
// launchers compute them.
extern "C" int fpc_wino_recip(uint32_t d, int64_t* out2) {
    if (!out2 || d < 1 || d > (1u << 31)) return FPC_EINVAL;
    const WinoRecip r = wino_recip(d);
    out2[0] = r.m; out2[1] = r.sh;
    return FPC_OK;
}
extern "C" int fpc_wino_decode(int Cout, int groups, int tbx, int tby, int W, int B, int pack, int64_t* out14) {
    if (!out14 || Cout < 64 || groups < 1 || tbx < 1 || tby < 1 || W < 1 || B < 1 || pack < 0) return FPC_EINVAL;
    const WinoDecode d = wino_decode(Cout, groups, tbx, tby, W, B, pack);
    const WinoRecip r[7] = {d.nnb, d.groups, d.tbx, d.tby, d.per, d.tbxl, d.tcw};
    for (int i = 0; i < 7; ++i) { out14[2 * i] = r[i].m; out14[2 * i + 1] = r[i].sh; }
    return FPC_OK;
}

// The tile maps of the four-wave Winograd kernels as the kernels compute them (host arithmetic; xshare = 1: the x-shared map of
// packed form-9 launches, fpc_wino_xshare_rule; 0: the row-split map).  See fpc.h.
extern "C" int fpc_wino_xshare_rule(int W) { return W >= 1 && wino_xshare_rule(W) ? 1 : 0; }
extern "C" int fpc_wino_tile_frag(int xshare, int wi, int lane, int pk_ks, int64_t* out17) {
    long long o[17] = {0};
    if (!out17 || wino_tile_frag(xshare != 0, wi, lane, pk_ks, o)) return FPC_EINVAL;
    for (int i = 0; i < 17; ++i) out17[i] = o[i];
    return FPC_OK;
}
extern "C" int fpc_wino_tile_slot(int xshare, int tr, int slot, int y_in0, int x_in0, int H, int W, int Cs, int up, int pk_ks, int pk_two,
                                  int64_t* out6) {
    long long o[6];
    if (!out6 || wino_tile_slot(xshare != 0, tr != 0, slot, y_in0, x_in0, H, W, Cs, up, pk_ks, pk_two, o)) return FPC_EINVAL;
    for (int i = 0; i < 6; ++i) out6[i] = o[i];
    return FPC_OK;
}
extern "C" int fpc_wino_tile_zrun(int xshare, int wi, int mt, int r, int nt, int cc, int64_t* out3) {
    long long o[3];
    if (!out3 || wino_tile_zrun(xshare != 0, wi, mt, r, nt, cc, o)) return FPC_EINVAL;
    for (int i = 0; i < 3; ++i) out3[i] = o[i];
    return FPC_OK;
}
extern "C" int fpc_wino_tile_zread(int xshare, int t_e, int tp, int cc, int i, int64_t* out1) {
    long long o[1];
    if (!out1 || wino_tile_zread(xshare != 0, t_e, tp, cc, i, o)) return FPC_EINVAL;
    out1[0] = o[0];
    return FPC_OK;
}
// the exit of those kernels: the patch decode with its fast-exit verdict, a thread's 16 output offsets.  See fpc.h.
extern "C" int fpc_wino_tile_patch(int packed, int H, int W, int B, int tbx, int tby, int pack, int patch, int64_t* out8) {
    long long o[8];
    if (!out8 || wino_tile_patch(packed != 0, H, W, B, tbx, tby, pack, patch, o)) return FPC_EINVAL;
    for (int i = 0; i < 8; ++i) out8[i] = o[i];
    return FPC_OK;
}
extern "C" int fpc_wino_tile_out(int tr, int H, int W, int Cout, int nb, int b, int ty0, int tx0, int pk_ks, int t_e, int64_t* out16) {
    long long o[16];
    if (!out16 || wino_tile_out(tr != 0, H, W, Cout, nb, b, ty0, tx0, pk_ks, t_e, o)) return FPC_EINVAL;
    for (int i = 0; i < 16; ++i) out16[i] = o[i];
    return FPC_OK;
}

// ---- stand-alone convolution (unit tests / micro-benchmarks of k_conv_igemm) -----------------
extern "C" size_t fpc_conv2d_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw) {
    int K = Cin * Kh * Kw, Kpad = cdiv(K, kConvBK) * kConvBK, Npad = cdiv(Cout, kConvNAlign) * kConvNAlign;
    size_t packed = conv_packed_floats(Npad, Kpad);
    size_t splitk = (size_t)32 * B * (cdiv(Ho * Wo, 128) * 128) * Npad;
    size_t wino = wino_region_floats(kImgH3, Cout, Cin, true);      // every Winograd image + a zero page for the all-DMA form
    return (packed + splitk + wino + kConvTickets) * sizeof(float);
}

namespace {
// workspace of ONE fpc_conv2d call (floats): [packed weights | split-K partials of this plan | Winograd images + zero page |
// arrival counters]; regions a plan does not use are empty
struct Conv2dLayout { size_t packed, splitk, wino, tickets, total; };
Conv2dLayout conv2d_layout(int B, int Cin, int Cout, int Kh, int Kw, const ConvPlan& p, const Conv2dRequest& r) {
    const int K = Cin * Kh * Kw, Kpad = cdiv(K, kConvBK) * kConvBK, Npad = cdiv(Cout, kConvNAlign) * kConvNAlign;
    Conv2dLayout L;
    L.packed = r.wino ? 0 : conv_packed_floats(Npad, Kpad);
    L.splitk = r.wino ? 0 : (splitk_floats_for(p, 1, B, Npad) + 63) / 64 * 64;
    L.wino = r.wino ? wino_region_floats(kWinoForms[r.wino].image, Cout, Cin, Cout % 128 == 0) : 0;      // up to the image the form reads
    L.tickets = (!r.wino && p.fused && p.nsplit > 1) ? kConvTickets : 0;
    L.total = L.packed + L.splitk + L.wino + L.tickets;
    return L;
}
ConvPlan conv2d_plan_for(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw, int bm, int bn, const Conv2dRequest& r) {
    const int Kpad = cdiv(Cin * Kh * Kw, kConvBK) * kConvBK;
    ConvPlan p = plan_conv(Ho * Wo, B, Cout, Kpad / kConvBK, 1, r.wino ? 0 : bm, bn, r.wino ? 1 : r.nsplit);
    p.bf3 = r.bf3 ? 1 : 0;
    p.h3 = r.h3 ? 1 : 0;
    if (r.two_launch) p.fused = 0;
    p.lat = r.lat;
    p.stem = r.stem ? 256 : 0;
    p.pool = r.pool ? 1 : 0;
    p.pw = r.pw;
    p.wino = r.wino;
    return p;
}
}  // namespace

extern "C" int fpc_conv2d_plan(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw, int bm, int bn, int nsplit,
                               int* out4) {
    if (!out4) return FPC_EINVAL;
    const int Kpad = cdiv(Cin * Kh * Kw, kConvBK) * kConvBK;
    // whatever kernel or product the request selects, the tiling reported is k_conv_igemm's with the request's split-K factor (no
    // GroupNorm rows of its own for k_lateral1x1 / k_stem7x7 / k_conv1x1); a Winograd request: 64 x 64, the request, the form's rows
    const Conv2dRequest r = decode_plan(nsplit);
    ConvPlan p = plan_conv(Ho * Wo, B, Cout, Kpad / kConvBK, 1, bm, bn, r.nsplit);
    p.wino = r.wino;
    out4[0] = p.bm; out4[1] = p.bn; out4[2] = r.wino ? nsplit : p.nsplit; out4[3] = plan_gn_rows(p, Ho, Wo, B, Cin, r.pack, r.orient);
    return FPC_OK;
}

// Exact workspace of fpc_conv2d for ONE request (same bm / bn / nsplit): at most fpc_conv2d_workspace_bytes, usually far
// less (that bound reserves 32 split-K slices of the whole output).  fpc_conv2d accepts either.
extern "C" size_t fpc_conv2d_workspace_bytes_for(int B, int Ho, int Wo, int Cin, int Cout, int Kh, int Kw, int bm, int bn,
                                                 int nsplit) {
    if (B < 1 || Ho < 1 || Wo < 1 || Cin < 1 || Cout < 1 || Kh < 1 || Kw < 1) return 0;
    const Conv2dRequest r = decode_plan(nsplit);
    const ConvPlan p = conv2d_plan_for(B, Ho, Wo, Cin, Cout, Kh, Kw, bm, bn, r);
    return std::max<size_t>(conv2d_layout(B, Cin, Cout, Kh, Kw, p, r).total * sizeof(float), 256);
}

extern "C" int fpc_conv2d(const float* in, int64_t sb, int64_t sh, int64_t sw, int64_t sc, const float* w_oihw,
                          const float* scale, const float* shift, const float* res, const float* up, float* out,
                          float* gn_part, int B, int Hi, int Wi, int Cin, int Cout, int Kh, int Kw, int stride, int pad,
                          int relu, int bm, int bn, int nsplit, void* ws, size_t ws_bytes, fpc_stream_t stream) {
    if (!in || !w_oihw || !out || !ws || B < 1 || Kh != Kw) return FPC_EINVAL;
    int Ho = conv_out(Hi, Kh, stride, pad), Wo = conv_out(Wi, Kw, stride, pad);
    if (Ho < 1 || Wo < 1) return FPC_EINVAL;
    const Conv2dRequest rq = decode_plan(nsplit);
    if (rq.grp) return FPC_EINVAL;      // this entry has no groups: fpc_conv2d_grouped
    const int wino = rq.wino;
    ConvPlan p = conv2d_plan_for(B, Ho, Wo, Cin, Cout, Kh, Kw, bm, bn, rq);
    const Conv2dLayout lay = conv2d_layout(B, Cin, Cout, Kh, Kw, p, rq);
    if (ws_bytes < lay.total * sizeof(float) || ((uintptr_t)ws & 255)) return FPC_EWORKSPACE;
    PackedConv c;
    c.Cin = c.Cinp = Cin; c.Cout = Cout; c.Kh = Kh; c.Kw = Kw; c.stride = stride; c.pad = pad;
    c.K = Cin * Kh * Kw; c.Kpad = cdiv(c.K, kConvBK) * kConvBK; c.Npad = cdiv(Cout, kConvNAlign) * kConvNAlign;
    hipStream_t s = (hipStream_t)stream;
    float* packed = (float*)ws;
    if (rq.stem) {      // the engine's stem layout: NHWC4 input, 8 taps x 4 channels per kernel row (K = 224), bf16 planes only
        if (Cin != 4 || Kh != 7 || stride != 2 || pad != 3 || Cout != 64 || sc != 1 || sw != 4 || sh != (int64_t)4 * Wi ||
            sb != (int64_t)4 * Hi * Wi || res || up || gn_part)
            return FPC_EINVAL;
        c.Kwp = 8; c.K = 4 * 7 * 8; c.Kpad = 224;
        // pool: conv + BN + ReLU + max-pool 3x3 / 2 / 1 in one launch on the h3 image: out is [B][Ho / 2][Wo / 2][64]
        FPC_TRY((rq.pool ? launch_pack_weight_h3 : launch_pack_weight_bf3)(w_oihw, packed, Cout, Cin, Cin, Kh, Kw, c.Kwp, c.Npad, c.Kpad, s));
        ConvArgs a0;      // (neither stem kernel reads split-K scratch, a zero page or arrival counters)
        fill_conv_shape(a0, B, c, p, Hi, Wi, Ho, Wo, sb, sh, sw, sc, relu != 0, 0);
        a0.Cin = 8 * c.Cinp; a0.Kw = 1; a0.K = c.K; a0.lanepx = 1;
        a0.p[0] = ConvPtrs{in, packed, out, scale, shift, nullptr, nullptr, nullptr};
        return rq.pool ? launch_stem_pool(a0, packed, out, Ho / 2, Wo / 2, s) : launch_conv_plan(a0, p, 1, s);
    }
    // (the split-precision forms — bf16 x 3 tiles, k_lateral1x1 — read only the planes behind the f32 image: it is not packed for them)
    static_assert(FPC_IGEMM_DMA_B, "the split-precision direct form stages its B rows from the bf16 planes by LDS-DMA; a build that loads "
                                   "them from the f32 image must pack that image here as well");
    // (the three-product form reads its own image at the start of the packed region: conv_packed_floats() > h3_packed_floats())
    if (!wino) FPC_TRY((p.h3 ? launch_pack_weight_h3 : p.bf3 ? launch_pack_weight_bf3 : launch_pack_weight)(w_oihw, packed, Cout, Cin, Cin, Kh, Kw, Kw, c.Npad, c.Kpad, s));
    int mode = (sc == 1 && Cin % kConvBK == 0 && Kh * Kw <= 32 && ((int64_t)Hi + 2 * pad) * sh * 4 < ((int64_t)1 << 31)) ? 0
               : (sc == 1 && Cin % 4 == 0 && sw % 4 == 0 && sh % 4 == 0 && sb % 4 == 0 && ((uintptr_t)in & 15) == 0) ? 2 : 1;
    ConvArgs a;      // (no zero page and no arrival counters until a form below asks for them)
    fill_conv_shape(a, B, c, p, Hi, Wi, Ho, Wo, sb, sh, sw, sc, relu != 0, mode);
    a.wino_pack = rq.pack ? 1 : 0;      // (-9 itself stays on the plain geometry
    a.wino_orient = rq.orient ? 1 : 0;  // and in the stored orientation)
    a.wino_rowsplit = rq.rowsplit ? 1 : 0;
    a.wino_exit_general = rq.exit_general ? 1 : 0;
    a.splitk_ws = packed + lay.packed;
    a.p[0] = ConvPtrs{in, packed, out, scale, shift, res, up, gn_part};
    if (lay.tickets) {   // arrival counters of the fused split-K form, zeroed per call
        float* tk = packed + lay.packed + lay.splitk + lay.wino;
        a.tickets = (int*)tk;
        if (hipMemsetAsync(tk, 0, kConvTickets * sizeof(int), s) != hipSuccess) return FPC_ELAUNCH;
    }
#ifdef FPC_STAMP_WINO      // diagnostic builds only: relu = 77 turns ReLU off and hands gn_part to the kernel as its stamp buffer
    if (wino && relu == 77) { a.dbg = gn_part; a.p[0].gn_part = nullptr; a.relu = 0; }
#endif
#ifdef FPC_STAMP_IGEMM
    if (!wino && relu == 77) { a.dbg = gn_part; a.p[0].gn_part = nullptr; a.relu = 0; }
#endif
    if (wino) {
        if (Kh != 3 || stride != 1 || pad != 1 || Cin % 8 || Cout % 64 || sc != 1 || up || sw != Cin ||
            sh != (int64_t)Wi * Cin || sb != (int64_t)Hi * Wi * Cin)
            return FPC_EINVAL;
        float* wp = packed + lay.packed + lay.splitk;
        // (a form reads only its own image: the f32 image is not packed for a split-precision form — 78 launches of a training step)
        if (!wino_form_ok(wino, Cin, Cout)) return FPC_EINVAL;
        const WinoImage img = kWinoForms[wino].image;
        if (rq.orient && wino_orient_rule(Ho, Wo)) FPC_TRY(launch_wino_pack_h3(w_oihw, wp + wino_image_offset(img, Cout, Cin), Cout, Cin, true, s));
        else FPC_TRY(kWinoImages[img].pack(w_oihw, wp + wino_image_offset(img, Cout, Cin), Cout, Cin, s));
        a.wino_w[0] = wp;
        a.zeros = zero_page();       // (the workspace's last 64 floats stay reserved for it: fpc_conv2d_workspace_bytes is unchanged)
        if (!a.zeros) {
            float* zp = wp + lay.wino - 64;
            if (hipMemsetAsync(zp, 0, 64 * sizeof(float), s) != hipSuccess) return FPC_ELAUNCH;
            a.zeros = zp;
        }
        return launch_conv_plan(a, p, 1, s);
    }
    if (p.h3) {
        if (mode != 0) return FPC_EINVAL;
        a.h3_w[0] = packed;
        return launch_conv_plan(a, p, 1, s);
    }
    a.bf3 = (p.bf3 && mode == 0) ? 1 : 0;
    if (p.bf3 && mode != 0) return FPC_EINVAL;
    if (p.lat || p.pw) return launch_conv_plan(a, p, 1, s);
    return launch_conv_plan(a, ConvPlan{a.bm, a.bn, a.nsplit, a.mtiles, a.ntiles, 0, a.bf3, a.fused}, 1, s);      // k_conv_igemm on the tiling `a` holds
}

// ---- stand-alone grouped 3x3 convolution (unit tests / micro-benchmarks of k_conv3x3_grouped) -----------------
// workspace: k_pack_grouped's image, C * (C / groups) * 9 floats (0: a shape fpc_conv2d_grouped refuses)
extern "C" size_t fpc_conv2d_grouped_workspace_bytes(int C, int groups) {
    if (C < 32 || C % 32 || groups < 1 || C % groups || !grouped_cg_ok(C / groups)) return 0;
    return std::max<size_t>(align_up((size_t)C * (C / groups) * 9 * sizeof(float), 256), 256);
}

extern "C" int fpc_conv2d_grouped(const float* in, int64_t sb, int64_t sh, int64_t sw, int64_t sc, const float* w_oihw,
                                  const float* scale, const float* shift, float* out, int B, int Hi, int Wi, int C, int groups,
                                  int stride, int relu, int form, void* ws, size_t ws_bytes, fpc_stream_t stream) {
    if (!in || !w_oihw || !out || !ws || B < 1 || Hi < 1 || Wi < 1 || C < 32 || C % 32 || groups < 1 || C % groups ||
        !grouped_cg_ok(C / groups) || (stride != 1 && stride != 2) || sc != 1 || form < 0 || form >= 1000)
        return FPC_EINVAL;
    const Conv2dRequest rq = decode_plan(FPC_PLAN_GROUPED + form);
    if (!rq.grp || rq.grp > kGroupedForms) return FPC_EINVAL;
    if (ws_bytes < fpc_conv2d_grouped_workspace_bytes(C, groups) || ((uintptr_t)ws & 255)) return FPC_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    GroupedArgs g;
    memset(&g, 0, sizeof(g));
    g.in = in; g.w = (const float*)ws; g.out = out; g.scale = scale; g.shift = shift;
    g.in_sb = sb; g.in_sh = sh; g.in_sw = sw;
    g.B = B; g.Hi = Hi; g.Wi = Wi; g.Ho = conv_out(Hi, 3, stride, 1); g.Wo = conv_out(Wi, 3, stride, 1);
    g.C = C; g.CG = C / groups; g.stride = stride; g.relu = relu ? 1 : 0; g.form = rq.grp - 1;
    // (every refusal of the launcher is tested here first, on a null stream-free path: nothing is packed for a refused request)
    if (((uintptr_t)in | (uintptr_t)out | (uintptr_t)scale | (uintptr_t)shift | (uintptr_t)w_oihw) & 15) return FPC_EINVAL;
    if ((sb | sh | sw) % 4 || sw < C) return FPC_EINVAL;
    FPC_TRY(launch_pack_grouped(w_oihw, (float*)ws, C, g.CG, s));
    return launch_conv3x3_grouped(g, s);
}
