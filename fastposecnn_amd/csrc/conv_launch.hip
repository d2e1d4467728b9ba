// conv_launch.hip — how a convolution plan (conv_plan.hpp) becomes a launch: launch_conv_plan routes site `a` to the kernel its plan names (k_conv3x3_grouped,
// k_stem7x7, k_conv1x1, k_lateral1x1, a Winograd form, k_conv_igemm with its split-K epilogue) after that form's own preconditions, launch_stem_pool is the stem's
// fused launch, plan_gn_rows the GroupNorm rows a plan writes.  Nothing here knows a network: the engine (net.hip) and conv2d.hip fill the ConvArgs.
#include "conv_plan.hpp"

namespace fpc {

int launch_conv_plan(ConvArgs& a, const ConvPlan& p, int groups, hipStream_t s) {
    if (p.grp || a.cg) {      // a grouped site runs on k_conv3x3_grouped and on nothing else
        if (!p.grp || p.grp > kGroupedForms || !a.cg || !a.grp_w || groups != 1 || a.in_sc != 1 || a.Kh != 3 || a.pad != 1 ||
            a.Cin != a.Cout || a.p[0].res || a.p[0].up || a.p[0].gn_part)
            return FPC_EINVAL;
        GroupedArgs g;
        memset(&g, 0, sizeof(g));
        g.in = a.p[0].in; g.w = a.grp_w; g.out = a.p[0].out; g.scale = a.p[0].scale; g.shift = a.p[0].shift;
        g.in_sb = a.in_sb; g.in_sh = a.in_sh; g.in_sw = a.in_sw;
        g.B = a.B; g.Hi = a.Hi; g.Wi = a.Wi; g.Ho = a.Ho; g.Wo = a.Wo; g.C = a.Cout; g.CG = a.cg; g.stride = a.stride; g.relu = a.relu;
        g.form = p.grp - 1;
        return launch_conv3x3_grouped(g, s);
    }
    if (p.stem) {
        if (groups != 1 || !stem_ok(a)) return FPC_EINVAL;
        StemArgs t;
        memset(&t, 0, sizeof(t));
        t.in = a.p[0].in;
        t.wpl = reinterpret_cast<const unsigned short*>(a.p[0].w + (size_t)a.Npad * a.Kpad);      // the bf16 planes behind the f32 image
        t.out = a.p[0].out; t.scale = a.p[0].scale; t.shift = a.p[0].shift;
        t.B = a.B; t.Hi = a.Hi; t.Wi = a.Wi; t.Ho = a.Ho; t.Wo = a.Wo; t.Cout = a.Cout; t.Npad = a.Npad; t.Kpad = a.Kpad; t.relu = a.relu;
        t.grid = p.stem;
        return launch_stem7x7(t, s);
    }
    if (p.pw) {
        if (!pw_ok(a, groups)) return FPC_EINVAL;
        PwArgs w;
        memset(&w, 0, sizeof(w));
        w.in = a.p[0].in;
        for (int g = 0; g < groups; ++g) {
            // the three bf16 planes sit behind the f32 image (k_pack_weight_bf3)
            w.wpl[g] = reinterpret_cast<const unsigned short*>(a.p[g].w + (size_t)a.Npad * a.Kpad);
            w.out[g] = a.p[g].out; w.scale[g] = a.p[g].scale; w.shift[g] = a.p[g].shift; w.res[g] = a.p[g].res; w.up[g] = a.p[g].up;
        }
        w.in_sb = a.in_sb; w.in_sh = a.in_sh; w.in_sw = a.in_sw;
        w.B = a.B; w.Ho = a.Ho; w.Wo = a.Wo; w.Cin = a.Cin; w.Cout = a.Cout; w.Npad = a.Npad; w.Kpad = a.Kpad; w.stride = a.stride;
        w.groups = groups; w.relu = a.relu;
        w.has_scale = a.p[0].scale != nullptr; w.has_shift = a.p[0].shift != nullptr;
        w.has_res = a.p[0].res != nullptr; w.has_up = a.p[0].up != nullptr;
        w.variant = p.pw - 1;
        return launch_conv1x1(w, s);
    }
    if (p.lat) {
        if (!lateral_ok(a, groups)) return FPC_EINVAL;
        LatArgs l;
        memset(&l, 0, sizeof(l));
        l.in = a.p[0].in;
        for (int g = 0; g < groups; ++g) {
            // the three bf16 planes sit behind the f32 image (k_pack_weight_bf3); h3: the site's k_pack_weight_h3 image
            if (p.h3 && !a.h3_w[g]) return FPC_EINVAL;
            l.wpl[g] = reinterpret_cast<const unsigned short*>(p.h3 ? a.h3_w[g] : a.p[g].w + (size_t)a.Npad * a.Kpad);
            l.out[g] = a.p[g].out; l.shift[g] = a.p[g].shift; l.up[g] = a.p[g].up;
        }
        l.B = a.B; l.Ho = a.Ho; l.Wo = a.Wo; l.Cout = a.Cout; l.Npad = a.Npad; l.Kpad = a.Kpad; l.groups = groups; l.relu = a.relu;
        l.parts = p.lat;
        l.h3 = p.h3;
        return launch_lateral1x1(l, s);
    }
    if (p.wino) {
        if (!wino_form_ok(p.wino, a.Cin, a.Cout)) return FPC_EINVAL;
        const WinoForm& f = kWinoForms[p.wino];
        WinoArgs w;
        memset(&w, 0, sizeof(w));
        for (int g = 0; g < groups; ++g) {
            if (!a.wino_w[g] || a.p[g].up) return FPC_EINVAL;
            w.p[g] = a.p[g];
            w.p[g].w = a.wino_w[g] + wino_image_offset(f.image, a.Cout, a.Cin);
        }
        w.variant = f.variant;
        w.zeros = a.zeros;
        w.dbg = (long long*)a.dbg;
        w.groups = groups;
        w.B = a.B; w.H = a.Ho; w.W = a.Wo; w.Cin = a.Cin; w.Cout = a.Cout; w.relu = a.relu;
        w.waves = f.waves;
        w.exit_general = a.wino_exit_general ? 1 : 0;
        const WinoGrid wg = wino_grid(p.wino, a.Ho, a.Wo);
        w.tbx = wg.tbx; w.tby = wg.tby;
        if (p.wino == kWinoH3) {      // packing and orientation: the same workgroups, fewer of them — properties of the launch, not of the plan
            bool tr;
            const WinoPackGeom q = wino_launch_geometry(a.Ho, a.Wo, a.B, a.Cin, a.wino_orient, a.wino_pack && !p.fold, &tr);
            if (q.G > 1 || tr) { w.pack = q.G; w.tbx = q.tbx; w.tby = q.tby; w.pack_rx = q.rx; }
            w.orient = tr ? 1 : 0;
            w.xshare = ((q.G > 1 || tr) && !a.wino_rowsplit && wino_xshare_rule(tr ? a.Ho : a.Wo)) ? 1 : 0;
            a.wino_blocks = q.patches * (a.Cout / 64) * groups;
        }
        if (p.fold) {      // c2 on Wc's image + up2(p3) on W's (the p2 input of .p[g] is not read)
            if (p.wino != kWinoH3 || !a.fold_in) return FPC_EINVAL;
            for (int g = 0; g < groups; ++g) {
                w.in2[g] = a.fold_up[g]; w.w2[g] = a.fold_w2[g];
                w.btab[g] = a.fold_tab[g];
                w.p[g].in = a.fold_in; w.p[g].w = a.fold_w[g];
            }
            w.fold = 1; w.Cin2 = a.Cin; w.Cin = a.fold_cin;
            w.all_rows = a.wino_fold_all_rows ? 1 : 0;
        }
        return f.launch(w, groups, s);
    }
    a.bm = p.bm; a.bn = p.bn; a.nsplit = p.nsplit; a.mtiles = p.mtiles; a.ntiles = p.ntiles; a.groups = groups;
    a.bf3 = (p.bf3 && a.generic == 0) ? 1 : 0;
    a.fused = (p.fused && p.nsplit > 1) ? 1 : 0;
    a.h3 = 0;
    ConvArgs h;
    if (p.h3) {      // the same launch on the site's k_pack_weight_h3 images (a is left as it was: the tuner reuses it)
        if (a.generic != 0) return FPC_EINVAL;
        h = a;
        h.bf3 = 0; h.h3 = 1;
        for (int g = 0; g < groups; ++g) {
            if (!a.h3_w[g]) return FPC_EINVAL;
            h.p[g].w = a.h3_w[g];
        }
    }
    const ConvArgs& l = p.h3 ? h : a;
    int rc = launch_conv(l, groups, s);
    if (!rc && l.nsplit > 1 && !l.fused) rc = launch_conv_splitk_epilogue(l, groups, s);
    return rc;
}

// number of GroupNorm partial rows per image a plan writes
int plan_gn_rows(const ConvPlan& p, int Ho, int Wo, int B, int Cin, int pack, int orient) {
    bool tr;
    if (p.wino == kWinoH3) return wino_launch_geometry(Ho, Wo, B, Cin, orient, pack && !p.fold, &tr).gn_rows;
    return p.wino ? wino_grid(p.wino, Ho, Wo).patches() : p.mtiles * p.bm / 32;
}

// the stem site's fused launch: image -> pooled tensor (k_stem_pool_h3).  `a` as the stem site fills it; FPC_EINVAL where the shape
// is not eligible (launch_stem_pool_h3) or the h3 image is not there
int launch_stem_pool(const ConvArgs& a, const float* h3_image, float* pool, int Hp, int Wp, hipStream_t s) {
    if (!h3_image || !stem_ok(a)) return FPC_EINVAL;
    StemPoolArgs t;
    memset(&t, 0, sizeof(t));
    t.in = a.p[0].in; t.wpl = reinterpret_cast<const unsigned short*>(h3_image); t.out = pool;
    t.scale = a.p[0].scale; t.shift = a.p[0].shift;
    t.B = a.B; t.Hi = a.Hi; t.Wi = a.Wi; t.Ho = a.Ho; t.Wo = a.Wo; t.Hp = Hp; t.Wp = Wp; t.Npad = a.Npad; t.Kpad = a.Kpad; t.relu = a.relu;
    t.band = kStemPoolBand; t.grid = 256;
    return launch_stem_pool_h3(t, s);
}

}  // namespace fpc
