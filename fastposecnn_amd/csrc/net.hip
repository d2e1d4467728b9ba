// net.hip — the backbone engine behind fpc_net_* (include/fpc.h): a native plan of
// PoseRegressor.pure_model_forward + Model.class_compression
// (F/lib/pose_regressor.py:709-743, 445-457) for inference.
//
// The graph is the one segmentation_models_pytorch builds for FastPoseCNN: an encoder, four FPN decoders with merge "add", four
// 1x1 heads and the x4 bilinear upsample (fastposecnn_amd/lib/backbone.py).  Which encoders there are, and what each is made of, is
// stated in net_plan.hpp (the block kinds, the encoder descriptor) and built in net_build.hip (one builder per encoder family).
// This file knows an encoder only as its tape: a list of steps, each of one kind, which the forward walks.
// The plan owns no device memory: packed weights, activations and split-K scratch live in one caller-provided workspace.
// Launch order per frame (R18): stem conv, max-pool, 16 encoder convs (+3 downsample 1x1) with
// BatchNorm / residual / ReLU in their epilogues, then the FOUR decoders as grouped launches:
// 4 lateral 1x1 convs (FPN top-down add in the epilogue), 7 3x3 convs (GroupNorm partial sums in
// the epilogue), 7 GroupNorm finalisations, 3 GN+ReLU+x2-upsample passes, 1 merge+head kernel,
// 1 x4-upsample + class-compression kernel.
//
// This file keeps what is done WITH a plan: loading, tuning, guarding, the forward and the fpc_net_* entry points but the creating
// ones.  Beside it: net_plan.hpp (what a plan is: struct fpc_net, the tape's steps, the encoder descriptor), net_build.hip (how one is
// built, and the fpc_net_create* entries), conv_plan.hpp (the host-only convolution planner: sites, plans, predicates, Winograd forms,
// plan codes), conv_launch.hip (a plan's launch, whichever kernel it names) and conv2d.hip (the stand-alone fpc_conv2d* and geometry
// entry points).
#include <initializer_list>
#include <utility>

#include "net_plan.hpp"

// the recorded graph no longer matches the plans, the parameters or the launch geometry
static void drop_graph(fpc_net* n) {
    if (n->graph_exec) { (void)hipGraphExecDestroy(n->graph_exec); n->graph_exec = nullptr; }
}

extern "C" void fpc_net_destroy(fpc_net_t* n) {
    if (!n) return;
    if (n->graph_exec) (void)hipGraphExecDestroy(n->graph_exec);
    delete n;
}

// The three-product direct form's weight images (PackedConv::h3_ok): their room is reserved when the plan is built (the workspace
// size is fixed before the split level is known), but they are packed only at level 3 — by fpc_net_load_params, or by raising the
// level on a loaded plan (on the stream of the last load).
static int pack_h3_images(fpc_net* n, hipStream_t s) {
    for (const PackedConv& c : n->convs)
        if (c.h3_ok) {
            int rc = launch_pack_weight_h3(n->pptr[c.p_w], n->ws + c.h3_off, c.Cout, c.Cin, c.Cinp, c.Kh, c.Kw, c.Kwp, c.Npad, c.Kpad, s);
            if (rc) return rc;
        }
    if (n->c_stem >= 0) {
        const PackedConv& st = n->convs[n->c_stem];
        int rc = launch_pack_weight_h3(n->pptr[st.p_w], n->ws + n->stem_h3_off, st.Cout, st.Cin, st.Cinp, st.Kh, st.Kw, st.Kwp, st.Npad, st.Kpad, s);
        if (rc) return rc;
    }
    n->h3_packed = true;
    return FPC_OK;
}

// 1: the next autotuning pass also times the split-precision (bf16 x 3, f32 accumulation) form of every direct
// fast-path convolution and keeps it where it is faster.  Opt-in: the results then differ from the f32 product chain
// by rounding (about 2^-24 relative per product, like a different f32 summation order), not bit for bit.
extern "C" int fpc_net_set_split_precision(fpc_net_t* n, int on) {
    if (!n) return FPC_EINVAL;
    n->split_precision = on < 0 ? 0 : (on > 3 ? 3 : on);      // 0: f32 products only, 1: + bf16 x 3 forms, 2: + the fp16 x 2 Winograd form, 3: + its three-product form
    if (n->split_precision >= 3 && n->loaded && !n->h3_packed) return pack_h3_images(n, n->load_stream);
    return FPC_OK;
}

// 1 while a recorded graph replays the frame (fpc_net_set_graph, after the first frame that could be captured), else 0
extern "C" int fpc_net_graph_recorded(const fpc_net_t* n) { return n && n->use_graph && n->graph_exec ? 1 : 0; }

// on = 1 (the default): a form-9 (k_conv_wino_h3) launch lays the frames of a small map side by side and cuts its 8 x 8 tile patches
// out of that canvas wherever this needs fewer patches (wino_pack_geometry); on = 0: one frame per patch row, as before.  The plans
// do not change (a site on form 9 reports -9 either way); the recorded graph is dropped.
extern "C" int fpc_net_set_wino_pack(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    if (n->wino_pack != on) drop_graph(n);
    n->wino_pack = on;
    return FPC_OK;
}

// on = 1 (the default): a packed form-9 launch (several frames per canvas row, or transposed) whose frame has an even number of tile
// columns runs on the x-shared tile map (conv_plan.hpp: wino_xshare_rule; wino_tile.hpp, XS); on = 0: every launch on the row-split
// map.  The same outputs and GroupNorm records bit for bit; plans, images and the workspace do not change; the recorded graph is dropped.
extern "C" int fpc_net_set_wino_xshare(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    if (n->wino_xshare != on) drop_graph(n);
    n->wino_xshare = on;
    return FPC_OK;
}

// on = 1 (the default): a workgroup of the four-wave Winograd kernels whose patch lies wholly inside its frame(s) leaves through the
// fast exit, which tests no pixel (wino_tile.hpp: wino_exit_fast, wino_output); on = 0: every workgroup takes the general exit.  The
// same outputs and GroupNorm records bit for bit; plans, images and the workspace do not change; the recorded graph is dropped.
extern "C" int fpc_net_set_wino_fast_exit(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    if (n->wino_fast_exit != on) drop_graph(n);
    n->wino_fast_exit = on;
    return FPC_OK;
}

// on = 1 (the default): in phase 2 of the folded s2.0 (wino_h3.hip, FOLD) the wave of the zero transform row only stages its pieces;
// on = 0: every wave runs the phase.  The same outputs and GroupNorm records bit for bit on finite operands; plans, images and the
// workspace do not change; the recorded graph is dropped.
extern "C" int fpc_net_set_fold_idle_row(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    if (n->fold_idle_row != on) drop_graph(n);
    n->fold_idle_row = on;
    return FPC_OK;
}

// The h3 image of conv `ci` in the orientation the site runs in, and decoder d's fold images and bias table in s2.0's.
static int pack_wino_h3_image(const fpc_net* n, int ci, hipStream_t s) {
    const PackedConv& c = n->convs[ci];
    return launch_wino_pack_h3(n->pptr[c.p_w], n->ws + c.wino_off + wino_image_offset(kImgH3, c.Cout, c.Cin), c.Cout, c.Cin,
                               n->wino_orient && n->c_tr[ci], s);
}
static int pack_fold_images(const fpc_net* n, int d, hipStream_t s) {
    const PackedConv &sc = n->convs[n->dec[d].seg[6]], &lc = n->convs[n->dec[d].lat[3]];
    const bool tr = n->wino_orient && n->c_tr[n->dec[d].seg[6]];
    int rc = launch_fold_compose(n->pptr[sc.p_w], n->pptr[lc.p_w], n->pptr[lc.p_bias], n->ws + n->fold_wc_off[d],
                                 n->ws + n->fold_tab_off[d], sc.Cout, sc.Cin, lc.Cin, tr, s);
    if (!rc) rc = launch_wino_pack_h3_pair(n->ws + n->fold_wc_off[d], n->ws + n->fold_img1_off[d], lc.Cin, n->pptr[sc.p_w],
                                           n->ws + n->fold_img2_off[d], sc.Cin, sc.Cout, tr, s);
    return rc;
}

// on = 1 (the default): a form-9 launch runs TRANSPOSED at the sites wino_orient_rule names (wide maps whose tile columns fill whole
// patches and whose tile rows do not: frames then pack along the image's y); on = 0: every site in the stored orientation.  A site
// keeps ONE h3 image, in the orientation it runs in: the switch repacks the affected sites' images (and the fold's) in place from the
// parameters, on the stream of the last load, and waits for it.  The plans and the workspace do not change; the recorded graph is dropped.
extern "C" int fpc_net_set_wino_orient(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    if (n->wino_orient == on) return FPC_OK;
    drop_graph(n);
    n->wino_orient = on;
    if (!n->loaded) return FPC_OK;
    if (hipDeviceSynchronize() != hipSuccess) return FPC_ELAUNCH;      // no launch may be reading an image that is repacked
    for (size_t ci = 0; ci < n->convs.size(); ++ci)
        if (n->c_tr[ci] && wino_form_ok(kWinoH3, n->convs[ci].Cin, n->convs[ci].Cout)) { const int rc = pack_wino_h3_image(n, (int)ci, n->load_stream); if (rc) return rc; }
    if (n->fold_ok && n->c_tr[n->dec[0].seg[6]])
        for (int d = 0; d < 4; ++d) { const int rc = pack_fold_images(n, d, n->load_stream); if (rc) return rc; }
    return hipStreamSynchronize(n->load_stream) == hipSuccess ? FPC_OK : FPC_ELAUNCH;
}

// workgroups of all form-9 launches of the last forward that launched (or captured) its kernels; -1 without a plan
extern "C" int64_t fpc_net_wino_blocks(const fpc_net_t* n) { return n ? (int64_t)n->wino_blocks : -1; }

// 1: after autotuning, the ~57 launches of a frame that only touch the plan's workspace are captured once and
// replayed with one hipGraphLaunch per frame (the first and the last kernel take the caller's tensors and stay
// ordinary launches).  Changing the tilings (fpc_net_autotune_next) or the parameters drops the recorded graph.
extern "C" int fpc_net_set_graph(fpc_net_t* n, int on) {
    if (!n) return FPC_EINVAL;
    n->use_graph = on ? 1 : 0;
    if (!on) drop_graph(n);
    return FPC_OK;
}
extern "C" int fpc_net_param_count(const fpc_net_t* n) { return n ? (int)n->pnames.size() : 0; }
extern "C" const char* fpc_net_param_name(const fpc_net_t* n, int i) {
    return (n && i >= 0 && i < (int)n->pnames.size()) ? n->pnames[i].c_str() : nullptr;
}
extern "C" int64_t fpc_net_param_numel(const fpc_net_t* n, int i) {
    return (n && i >= 0 && i < (int)n->pnumel.size()) ? n->pnumel[i] : -1;
}
extern "C" size_t fpc_net_workspace_bytes(const fpc_net_t* n) { return n ? n->total_floats * sizeof(float) : 0; }

// BatchNorm's four parameters from p_bn on, over C channels (eps 1e-5 but for the EfficientNet ops: 1e-3), folded into the scale /
// shift the epilogues read
static int fold_bn_of(const fpc_net* n, int p_bn, int C, size_t scale_off, size_t shift_off, hipStream_t s, float eps = 1e-5f) {
    return launch_fold_bn(n->pptr[p_bn], n->pptr[p_bn + 1], n->pptr[p_bn + 2], n->pptr[p_bn + 3], eps, C, n->ws + scale_off, n->ws + shift_off, s);
}

extern "C" int fpc_net_load_params(fpc_net_t* n, const float* const* params, int count, void* ws, size_t ws_bytes,
                                   fpc_stream_t stream) {
    if (!n || !params || count != (int)n->pnames.size() || !ws) return FPC_EINVAL;
    if (((uintptr_t)ws & 255) != 0 || ws_bytes < n->total_floats * sizeof(float)) return FPC_EWORKSPACE;
    drop_graph(n);       // pointers may change
    for (int i = 0; i < count; ++i)
        if (!params[i] || ((uintptr_t)params[i] & 15)) return FPC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    n->ws = (float*)ws;
    n->pptr.assign(params, params + count);
    n->load_stream = s;
    n->h3_packed = false;
    if (n->split_precision >= 3) { int rc = pack_h3_images(n, s); if (rc) return rc; }
    if (hipMemsetAsync(n->ws + n->zeros_off, 0, 64 * sizeof(float), s) != hipSuccess) return FPC_ELAUNCH;
    if (hipMemsetAsync(n->ws + n->tickets_off, 0, kConvTickets * sizeof(int), s) != hipSuccess) return FPC_ELAUNCH;
    for (size_t ci = 0; ci < n->convs.size(); ++ci) {
        const PackedConv& c = n->convs[ci];
        if (c.cg) {      // a grouped site: its own image and the folded BatchNorm
            int rg = launch_pack_grouped(n->pptr[c.p_w], n->ws + c.grp_off, c.Cout, c.cg, s);
            if (!rg) rg = fold_bn_of(n, c.p_bn, c.Cout, c.scale_off, c.shift_off, s);
            if (rg) return rg;
            continue;
        }
        int rc = launch_pack_weight(n->pptr[c.p_w], n->ws + c.w_off, c.Cout, c.Cin, c.Cinp, c.Kh, c.Kw, c.Kwp, c.Npad, c.Kpad, s);
        if (rc) return rc;
        rc = launch_pack_weight_bf3(n->pptr[c.p_w], n->ws + c.w_off, c.Cout, c.Cin, c.Cinp, c.Kh, c.Kw, c.Kwp, c.Npad, c.Kpad, s);
        if (rc) return rc;
        if (c.wino_ok) {
            for (int f = 1, done = 0; f < kWinoFormCount; ++f) {      // every image a form this site may run on reads, once
                const WinoImage img = kWinoForms[f].image;
                if (!wino_form_ok(f, c.Cin, c.Cout) || (done >> img & 1)) continue;
                done |= 1 << img;
                rc = img == kImgH3 ? pack_wino_h3_image(n, (int)ci, s)      // (in the site's orientation)
                                   : kWinoImages[img].pack(n->pptr[c.p_w], n->ws + c.wino_off + wino_image_offset(img, c.Cout, c.Cin), c.Cout, c.Cin, s);
                if (rc) return rc;
            }
        }
        if (c.p_bn >= 0) {
            rc = fold_bn_of(n, c.p_bn, c.Cout, c.scale_off, c.shift_off, s);
            if (!rc && c.p_bias >= 0) rc = launch_fold_conv_bias(n->ws + c.scale_off, n->pptr[c.p_bias], n->ws + c.shift_off, c.Cout, s);      // (a VGG _bn site: the conv bias behind the fold)
            if (rc) return rc;
        }
    }
    if (n->vgg0.p_bn >= 0) {      // features.0 of a VGG _bn encoder: the same fold
        const fpc_net::VggStem& v = n->vgg0;
        int rc = fold_bn_of(n, v.p_bn, 64, v.scale_off, v.shift_off, s);
        if (!rc) rc = launch_fold_conv_bias(n->ws + v.scale_off, n->pptr[v.p_bias], n->ws + v.shift_off, 64, s);
        if (rc) return rc;
    }
    if (n->fold_ok)
        for (int d = 0; d < 4; ++d) {
            const int rc = pack_fold_images(n, d, s);
            if (rc) return rc;
        }
    for (const fpc_net::MbOp& o : n->mops) {      // the MobileNetV2 and EfficientNet encoders' ops: the folded BatchNorm (the weights are read in place)
        const int rc = fold_bn_of(n, o.p_bn, o.Cout, o.scale_off, o.shift_off, s, o.eps);
        if (rc) return rc;
    }
    for (const fpc_net::DnOp& o : n->dops) {      // the DenseNet encoders' ops: the folded BatchNorms and conv2's re-laid image (conv1 and the transitions' conv are read in place)
        int rc = FPC_OK;
        if (o.p_bn1 >= 0) rc = fold_bn_of(n, o.p_bn1, o.K, o.s1_off, o.t1_off, s);
        if (!rc && o.p_bn2 >= 0) rc = fold_bn_of(n, o.p_bn2, o.Cout, o.s2_off, o.t2_off, s);
        if (!rc && o.kind == fpc_net::kDnConv3) rc = launch_dense_pack_w(n->pptr[o.p_w], n->ws + o.wt_off, s);
        if (rc) return rc;
    }
    n->loaded = true;
    return FPC_OK;
}

namespace {

struct ConvIO {
    const float* in; long long sb, sh, sw, sc; int Hi, Wi;
    float* out; int Ho, Wo;
    const float* res; const float* up; float* gn_part;
};

// fills the shared part of ConvArgs from conv `c` + plan `p` and the plan's workspace
void fill_conv_args(const fpc_net* n, ConvArgs& a, const PackedConv& c, const ConvPlan& p, int Hi, int Wi, int Ho,
                    int Wo, long long sb, long long sh, long long sw, long long sc, bool relu, int mode) {
    fill_conv_shape(a, n->B, c, p, Hi, Wi, Ho, Wo, sb, sh, sw, sc, relu, mode);
    a.splitk_ws = n->ws + n->splitk_off; a.zeros = n->ws + n->zeros_off; a.tickets = (int*)(n->ws + n->tickets_off);
    a.wino_pack = n->wino_pack; a.wino_orient = n->wino_orient; a.wino_rowsplit = n->wino_xshare ? 0 : 1; a.wino_exit_general = n->wino_fast_exit ? 0 : 1;
    a.wino_fold_all_rows = n->fold_idle_row ? 0 : 1;
}


// Minimum elapsed time (ms) of `reps` runs of `run` (-> FPC_OK) on stream `s`, synchronising after each; 1e30 if it could not be
// timed: such a candidate is never chosen.  The autotuner's clock; its events are gone on return.
template <class F> float min_ms(hipStream_t s, int reps, F run) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    float ms = 1e30f;
    if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
        for (int rep = 0; rep < reps; ++rep) {
            float t = 0.f;
            bool timed = hipEventRecord(e0, s) == hipSuccess && run() == FPC_OK && hipEventRecord(e1, s) == hipSuccess &&
                         hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess;
            if (timed && t < ms) ms = t;
        }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return ms;
}

// The plans the autotuner times for the site `a` describes, in the order it times them (the first of equal scores is kept):
// `split` = the plan's split-precision level, `pointwise` = its encoder offers k_conv1x1 (EncoderDesc::pointwise).
std::vector<ConvPlan> tune_candidates(const ConvArgs& a, int groups, int split, bool pointwise) {
    if (a.cg) {      // a grouped site: the forms of k_conv3x3_grouped that are built
        std::vector<ConvPlan> gc;
        for (int f = 0; f < kGroupedForms; ++f) { ConvPlan q; q.grp = f + 1; gc.push_back(q); }
        return gc;
    }
    std::vector<ConvPlan> cands = conv_candidates(a.Ho * a.Wo, a.B, a.Cout, a.ksteps, groups);
    const size_t nf = cands.size();
    if (split && a.generic == 0) {          // the same tilings with split-precision matrix products
        for (size_t i = 0; i < nf; ++i) { ConvPlan q = cands[i]; q.bf3 = 1; cands.push_back(q); }
    }
    if (split >= 3 && a.generic == 0 && a.h3_w[0]) {      // ... and with the three fp16 piece products (level 3)
        for (size_t i = 0; i < nf; ++i) { ConvPlan q = cands[i]; q.h3 = 1; cands.push_back(q); }
    }
    if (split && groups == 1 && stem_ok(a)) {   // weight-resident stem (bf16 x 3 planes), one workgroup per CU
        ConvPlan sq; sq.stem = 256; cands.push_back(sq);
    }
    if (split && lateral_ok(a, groups)) {   // pixel-resident lateral product (bf16 x 3 planes)
        const int tiles = groups * (a.Cout / 32);
        for (int parts = 1; parts <= tiles; parts *= 2)
            if (tiles % parts == 0) {
                ConvPlan lq; lq.lat = parts; cands.push_back(lq);
                if (split >= 3 && a.h3_w[0]) { lq.h3 = 1; cands.push_back(lq); }      // ... on two fp16 pieces
            }
    }
    if (split && pointwise && pw_ok(a, groups)) {      // the 1x1 GEMM (bf16 x 3 planes), Bottleneck plans only
        ConvPlan pq;
        pq.pw = 1; cands.push_back(pq);
        pq.pw = 2; cands.push_back(pq);
    }
    if (a.wino_w[0] && !a.p[0].up) {
        auto offered = [&](int f) { return split >= kWinoForms[f].min_split && wino_form_ok(f, a.Cin, a.Cout) && (a.zeros || !kWinoForms[f].zeros); };
        for (int f = 1; f < kWinoFormCount; ++f) {
            // the fp16 x 2 forms (range-limited: fpc.h): all four piece products, or (level 3, Cin a multiple of 16) three of them over
            // pairs of K-steps.  Where the second form is allowed it REPLACES the first as a candidate: one launch timed from a cold
            // clock ranks them by their entry costs, the forward in steady state by their power (all sites on form 9 against all on
            // form 8: 14.05 / 14.58 and 14.21 / 15.04 ms on two boxes, while per-site timing picked form 9 for 2 of 33 sites)
            if (!offered(f) || (f == kWinoH2 && offered(kWinoH3))) continue;
            ConvPlan wq; wq.wino = f; cands.push_back(wq);
        }
    }
    return cands;
}

// Workgroups plan `q` launches on site `a` and the share of the chip's workgroup slots they take, held to [1/8, 1].
struct PlanFootprint { double nblk, share; };
PlanFootprint plan_footprint(const ConvPlan& q, const ConvArgs& a, int groups) {
    bool tr;
    double nblk = q.grp ? (double)cdiv(a.Ho, 8) * cdiv(a.Wo, grouped_tile_cols(a.stride)) * (a.Cout / 32) * a.B
                  : q.stem ? 512.0      // (a persistent 512-thread, 86 KB workgroup per CU: the whole chip, whatever its grid)
                  : q.lat ? (double)cdiv(a.Ho * a.Wo, 128) * a.B * q.lat
                  : q.pw ? (double)cdiv(a.B * a.Ho * a.Wo, pw_tile_pixels(q.pw - 1)) * (a.Cout / 64) * groups * q.pw      // (8-wave workgroups count twice)
                  : q.wino == kWinoH3 ? (double)wino_launch_geometry(a.Ho, a.Wo, a.B, a.Cin, a.wino_orient, a.wino_pack && !q.fold, &tr).patches * (a.Cout / 64) * groups
                  : q.wino ? (double)wino_grid(q.wino, a.Ho, a.Wo).patches() * a.B * (a.Cout / kWinoForms[q.wino].bn) * groups
                         : (double)q.mtiles * q.ntiles * q.nsplit * a.B * groups;
    double share = nblk / (256.0 * (q.wino ? kWinoForms[q.wino].wg_per_cu : 2));
    if (share > 1.0) share = 1.0;
    if (share < 0.125) share = 0.125;
    return {nblk, share};
}

// The survey pass of site `ci` (fpc_net_survey_next): k_act_range over every activation tensor plan `p` reads as its matrix operand,
// accumulated into the site's record.  Every engine input is a contiguous NHWC tensor of B frames (in_sb elements each; the stem's:
// the NHWC4 image, whose fourth channel is zero).  Groups that share one input (the laterals) survey it once.  The folded s2.0 reads
// two operands of their own scales, not p2: c2 into its own record, p3 at ITS resolution (nearest x2 inside the kernel: the same
// values) into the record of the p2 lateral site, which does not run while it is folded away.
int survey_site(const fpc_net* n, const ConvArgs& a, const ConvPlan& p, int groups, int ci, hipStream_t s) {
    unsigned* rec = n->survey + 4 * (size_t)ci;
    if (p.fold) {
        unsigned* rec_up = n->survey + 4 * (size_t)n->dec[0].lat[3];
        int rc = launch_act_range(a.fold_in, (long long)a.B * a.Ho * a.Wo * a.fold_cin, rec, s);
        for (int g = 0; g < groups && !rc; ++g) rc = launch_act_range(a.fold_up[g], (long long)a.B * (a.Ho / 2) * (a.Wo / 2) * a.Cin, rec_up, s);
        return rc;
    }
    for (int g = 0; g < groups; ++g) {
        bool seen = false;
        for (int h = 0; h < g; ++h) seen = seen || a.p[h].in == a.p[g].in;
        if (seen) continue;
        const int rc = launch_act_range(a.p[g].in, (long long)a.B * a.in_sb, rec, s);
        if (rc) return rc;
    }
    return FPC_OK;
}

// Runs conv site `ci` with its current plan; in tuning mode first times every candidate (HIP events on the stream,
// synchronising — only ever inside fpc_net_autotune): candidates, time each, keep the best, the fold challenger, launch.
int run_conv(fpc_net* n, ConvArgs& a, int groups, int ci, hipStream_t s) {
    if (n->tuning) {
        float best_ms = 1e30f, free_ms = 1e30f;
        ConvPlan best = n->cplan[ci];
        n->has_free[ci] = 0;
        for (const ConvPlan& q : tune_candidates(a, groups, n->split_precision, n->enc.pointwise())) {
            if (splitk_floats_for(q, groups, a.B, a.Npad) > n->splitk_floats) continue;
            if (n->guarded[ci] && plan_range_limited(q)) continue;      // a demoted site stays range-free
            int rc = launch_conv_plan(a, q, groups, s);     // warm-up (also validates the launch)
            if (rc == FPC_EINVAL) continue;                 // a candidate whose launcher refuses this site (its own preconditions) is skipped
            if (rc) return rc;
            const float ms = min_ms(s, 3, [&] { return launch_conv_plan(a, q, groups, s); });
            // objective: latency, or (throughput mode) latency x the share of the chip the launch occupies —
            // with several frames in flight a launch that leaves CUs free lets another stream's kernels run
            float score = ms;
            if (n->tune_mode >= 1) {
                const double share = plan_footprint(q, a, groups).share;
                score = ms * (float)(n->tune_mode == 2 ? share : sqrt(share));      // 2: latency x share = the launch's CU-time
            }
            if (score < best_ms) { best_ms = score; best = q; }
            if (score < free_ms && !plan_range_limited(q)) { free_ms = score; n->free_plan[ci] = q; n->has_free[ci] = 1; }      // the guard's fallback
        }
        n->tune_score[ci] = best_ms;
        // s2.0 with the FPN p2 level folded in (level 3, wino_h3.hip): it replaces the p2 lateral AND this site, so it must beat the sum
        // of both best scores (the lateral's was taken earlier in this pass).  Same timing rule as above; the whole chip: score = ms.
        if (n->split_precision >= 3 && a.fold_in && a.fold_lat_ms > 0.f && !n->guarded[ci]) {
            ConvPlan fq;
            fq.wino = kWinoH3; fq.fold = 1;
            int rc = launch_conv_plan(a, fq, groups, s);
            if (rc && rc != FPC_EINVAL) return rc;
            const float ms = rc ? 1e30f : min_ms(s, 3, [&] { return launch_conv_plan(a, fq, groups, s); });
            if (ms < best_ms + a.fold_lat_ms) best = fq;
        }
        n->cplan[ci] = best;
    }
    const ConvPlan p = n->cplan[ci];
    if (n->survey) { const int rs = survey_site(n, a, p, groups, ci, s); if (rs) return rs; }
    const int rc = launch_conv_plan(a, p, groups, s);
    if (!rc && p.wino == kWinoH3) n->wino_blocks += a.wino_blocks;
    return rc;
}

}  // namespace


// Everything between the NCHW -> NHWC4 conversion of the caller's image and the final upsample / class
// compression into the caller's tensors: ~57 launches that touch only the plan's workspace and parameters, i.e.
// identical every frame — the part that can be replayed as a HIP graph.
static int forward_middle(fpc_net* n, hipStream_t s) {
    float* ws = n->ws;
    n->wino_blocks = 0;
    const int B = n->B, H = n->H, W = n->W;
    ConvArgs a;
    auto nhwc = [&](const Act& t, long long& sb, long long& sh, long long& sw, long long& sc) {
        sc = 1; sw = t.C; sh = (long long)t.W * t.C; sb = (long long)t.H * sh;
    };
    if (n->c_stem >= 0) {
        const PackedConv& c = n->convs[n->c_stem];
        // The 7x7/2 stem as a 7x1 convolution over "pixels" of 8 x 4 channels: one K-step = one kernel row = the 8
        // consecutive 16-byte pixels starting at wi0, which are 128 contiguous bytes of the NHWC4 image — the fast
        // loader's case (scalar tap walk, two vector instructions per row and step) instead of the per-lane tap
        // decode of MODE 2 (3500 cycles per K-step of 16 MFMAs, measured).  The eighth tap has zero weights.
        fill_conv_args(n, a, c, n->cplan[n->c_stem], H, W, n->a_stem.H, n->a_stem.W, (long long)4 * H * W, (long long)4 * W, 4,
                       1, true, 0);
        a.Cin = 8 * c.Cinp; a.Kw = 1; a.K = c.K; a.lanepx = 1;
        a.p[0] = ConvPtrs{ws + n->a_img4.off, ws + c.w_off, ws + n->a_stem.off, ws + c.scale_off, ws + c.shift_off, nullptr, nullptr, nullptr};
        const float* h3img = n->h3_packed ? ws + n->stem_h3_off : nullptr;
        const bool ceil = n->enc.resnet.ceil_pool();      // the SE-ResNet stem: its pool has no padding (k_stem_pool_h3 is a pad-1 kernel: neither tuned nor forced there)
        auto pool_launch = [&]() {
            return ceil ? launch_maxpool3x3s2_ceil(ws + n->a_stem.off, ws + n->a_pool.off, B, n->a_stem.H, n->a_stem.W, 64, s)
                        : launch_maxpool3x3s2(ws + n->a_stem.off, ws + n->a_pool.off, B, n->a_stem.H, n->a_stem.W, 64, n->a_pool.H, n->a_pool.W, s);
        };
        if (n->cplan[n->c_stem].pool && !n->tuning && !ceil) {      // one launch to the pooled tensor: a_stem is not written
            if (n->survey) FPC_TRY(survey_site(n, a, n->cplan[n->c_stem], 1, n->c_stem, s));      // (not through run_conv: the image)
            FPC_TRY(launch_stem_pool(a, h3img, ws + n->a_pool.off, n->a_pool.H, n->a_pool.W, s));
        } else {
            n->cplan[n->c_stem].pool = 0;
            FPC_TRY(run_conv(n, a, 1, n->c_stem, s));
            FPC_TRY(pool_launch());
            // level 3: the fused launch against the site's best plan AND the max-pool together (it replaces both), timed as the p2
            // fold is; the whole chip: score = ms.  Kept only when it beats them
            if (n->tuning && !ceil && n->split_precision >= 3 && !n->guarded[n->c_stem] && launch_stem_pool(a, h3img, ws + n->a_pool.off, n->a_pool.H, n->a_pool.W, s) == FPC_OK) {
                const ConvPlan cur = n->cplan[n->c_stem];
                float ms_pair = 1e30f, ms_fused = 1e30f;
                for (int rep = 0; rep < 3; ++rep) {      // six runs, the two sides in turn
                    ms_pair = std::min(ms_pair, min_ms(s, 1, [&] { int rc = launch_conv_plan(a, cur, 1, s); return rc ? rc : pool_launch(); }));
                    ms_fused = std::min(ms_fused, min_ms(s, 1, [&] { return launch_stem_pool(a, h3img, ws + n->a_pool.off, n->a_pool.H, n->a_pool.W, s); }));
                }
                if (ms_fused < ms_pair) { ConvPlan q; q.stem = 256; q.pool = 1; n->cplan[n->c_stem] = q; }
            }
        }
    }
    // the encoder tape.  One site: conv `ci` from `in` to `out` with BatchNorm, the residual and ReLU in its epilogue, on whichever
    // images the site has
    auto enc_conv = [&](int ci, const Act& in, const Act& out, bool relu, const float* res) -> int {
        long long sb, sh, sw, sc;
        nhwc(in, sb, sh, sw, sc);
        const PackedConv& c = n->convs[ci];
        fill_conv_args(n, a, c, n->cplan[ci], in.H, in.W, out.H, out.W, sb, sh, sw, sc, relu, 0);
        // (a site without BatchNorm — a VGG encoder's — has its bias, read in place, as the shift and no scale)
        const float* scale = c.p_bn >= 0 ? ws + c.scale_off : nullptr;
        const float* shift = c.p_bn >= 0 ? ws + c.shift_off : c.p_bias >= 0 ? n->pptr[c.p_bias] : nullptr;
        a.p[0] = ConvPtrs{ws + in.off, ws + c.w_off, ws + out.off, scale, shift, res, nullptr, nullptr};
        if (c.wino_ok) a.wino_w[0] = ws + c.wino_off;
        if (c.h3_ok && n->h3_packed) a.h3_w[0] = ws + c.h3_off;
        if (c.cg) { a.cg = c.cg; a.grp_w = ws + c.grp_off; }
        return run_conv(n, a, 1, ci, s);
    };
    // the gate of an SE block: from Y's channel means, then Y = relu(Y * gate + residual) in place.  Refused on a plan built
    // without the gate's scratch, which lies behind the persistent region where it exists: never at offset 0
    auto se_gate = [&](int p_se, const Act& Y, const float* res) -> int {
        if (!n->se_part_off) return FPC_EINVAL;
        FPC_TRY(launch_se_pool(ws + Y.off, ws + n->se_part_off, B, Y.H, Y.W, Y.C, s));
        FPC_TRY(launch_se_excite(ws + n->se_part_off, n->pptr[p_se], n->pptr[p_se + 1], n->pptr[p_se + 2], n->pptr[p_se + 3],
                                 ws + n->se_gate_off, B, Y.H, Y.W, Y.C, n->enc.resnet.se, s));
        return launch_se_scale_add_relu(ws + Y.off, ws + n->se_gate_off, res, ws + Y.off, B, Y.H, Y.W, Y.C, s);
    };
    // an op of the MobileNetV2 or EfficientNet encoder, on the one kernel of its kind
    auto mb_op = [&](const fpc_net::MbOp& o, const Act& in, const Act& out, const float* res) -> int {
        const float *w = n->pptr[o.p_w], *sc = ws + o.scale_off, *sh = ws + o.shift_off;
        switch (o.kind) {
        case fpc_net::kMbStem: return launch_stem3x3s2(ws + in.off, w, sc, sh, ws + out.off, B, in.H, in.W, s);
        case fpc_net::kMbDw: return launch_dwconv3x3(ws + in.off, w, sc, sh, ws + out.off, B, in.H, in.W, in.C, o.stride, o.act, s);
        case fpc_net::kMbPw: return launch_conv1x1_f32(ws + in.off, w, sc, sh, res, ws + out.off, (long long)B * in.H * in.W, o.Cin, o.Cout, o.act, s);
        case fpc_net::kMbSameStem: return launch_mb_stem3x3s2(ws + in.off, w, sc, sh, ws + out.off, B, in.H, in.W, s);
        case fpc_net::kMbSameDw: return launch_mb_dwconv(ws + in.off, w, sc, sh, ws + out.off, B, in.H, in.W, in.C, o.k, o.stride, o.act, s);
        case fpc_net::kMbGatedPw:      // (the gate its block's gate step wrote just before)
            if (o.gate >= 0 && !n->mb_gate_off) return FPC_EINVAL;
            return launch_mb_conv1x1(ws + in.off, o.gate >= 0 ? ws + n->mb_gate_off : nullptr, w, sc, sh, res, ws + out.off, B,
                                     (long long)in.H * in.W, o.Cin, o.Cout, o.act, s);
        }
        return FPC_EINVAL;
    };
    // the gate of an MBConv block from its depthwise output.  Refused on a plan built without the gate's scratch, as se_gate is
    auto mb_gate = [&](const fpc_net::MbGate& g, const Act& x) -> int {
        if (!n->mb_part_off || g.C != x.C) return FPC_EINVAL;
        return launch_mb_gate(ws + x.off, n->pptr[g.p], n->pptr[g.p + 1], n->pptr[g.p + 2], n->pptr[g.p + 3], ws + n->mb_gate_off,
                              ws + n->mb_part_off, B, x.H, x.W, x.C, g.Cs, s);
    };
    // an op of a DenseNet encoder, on the one kernel of its kind and the form its shape names
    auto dense_op = [&](const fpc_net::DnOp& o) -> int {
        const long long M = (long long)B * o.H * o.W;
        switch (o.kind) {
        case fpc_net::kDnPlace: return launch_dense_place(ws + o.in_off, ws + o.out_off, M, o.K, o.ldo, s);
        case fpc_net::kDnPw:
            return launch_dense_pw(ws + o.in_off, o.p_bn1 >= 0 ? ws + o.s1_off : nullptr, o.p_bn1 >= 0 ? ws + o.t1_off : nullptr, n->pptr[o.p_w],
                                   o.p_bn2 >= 0 ? ws + o.s2_off : nullptr, o.p_bn2 >= 0 ? ws + o.t2_off : nullptr, ws + o.out_off, M, o.K, o.Cout,
                                   o.ldi, o.ldo, o.act, -1, s);
        case fpc_net::kDnConv3: return launch_dense_conv3(ws + o.in_off, ws + o.wt_off, ws + o.out_off, B, o.H, o.W, o.c0, o.ldo, -1, s);
        case fpc_net::kDnNormPool:
            return launch_dense_norm_pool(ws + o.in_off, ws + o.s1_off, ws + o.t1_off, ws + o.out_off, o.out2 ? ws + o.out2_off : nullptr, B, o.H,
                                          o.W, o.K, o.act, s);
        }
        return FPC_EINVAL;
    };
    for (const Step& st : n->tape) {
        const float* res = st.res.C ? ws + st.res.off : nullptr;
        switch (st.kind) {
        case kStepConv: FPC_TRY(enc_conv(st.op, st.in, st.out, st.relu, res)); break;
        case kStepSeGate: FPC_TRY(se_gate(st.op, st.out, res)); break;
        case kStepMb: FPC_TRY(mb_op(n->mops[st.op], st.in, st.out, res)); break;
        case kStepMbGate: FPC_TRY(mb_gate(n->mgates[st.op], st.in)); break;
        case kStepDense: FPC_TRY(dense_op(n->dops[st.op])); break;
        case kStepVggStem: {      // features.0 of a VGG encoder: the folded BatchNorm, or the bias alone, and ReLU
            const fpc_net::VggStem& v = n->vgg0;
            if (v.p_w < 0) return FPC_EINVAL;
            FPC_TRY(launch_conv3x3_c3(ws + st.in.off, n->pptr[v.p_w], v.p_bn >= 0 ? ws + v.scale_off : nullptr,
                                      v.p_bn >= 0 ? ws + v.shift_off : n->pptr[v.p_bias], ws + st.out.off, B, st.in.H, st.in.W, 1, s));
            break;
        }
        case kStepPool2: FPC_TRY(launch_maxpool2x2(ws + st.in.off, ws + st.out.off, B, st.in.H, st.in.W, st.in.C, s)); break;
        }
    }
    const Act* feat = n->a_feat;

    // ---- four decoders, grouped
    // laterals: p5 = conv(c5); p4 = up2_nearest(p5) + conv(c4); p3; p2 (not where s2.0 folds it in, outside an autotuning pass)
    const bool fold = n->cplan[n->dec[0].seg[6]].fold && !n->tuning;
    for (int i = 0; i < 4; ++i) {
        if (i == 3 && fold) continue;
        const Act& src = feat[3 - i];
        long long sb, sh, sw, sc;
        nhwc(src, sb, sh, sw, sc);
        int ci0 = n->dec[0].lat[i];
        fill_conv_args(n, a, n->convs[ci0], n->cplan[ci0], src.H, src.W, src.H, src.W, sb, sh, sw, sc, false, lateral_mode(n->convs[ci0]));
        for (int d = 0; d < 4; ++d) {
            const PackedConv& c = n->convs[n->dec[d].lat[i]];
            a.p[d] = ConvPtrs{ws + src.off, ws + c.w_off, ws + n->a_p[d][i].off, nullptr, n->pptr[c.p_bias], nullptr,
                              i > 0 ? ws + n->a_p[d][i - 1].off : nullptr, nullptr};
            if (c.h3_ok && n->h3_packed) a.h3_w[d] = ws + c.h3_off;
        }
        FPC_TRY(run_conv(n, a, 4, ci0, s));
    }
    // segmentation blocks
    auto seg_conv = [&](int si, int which) -> int {
        // input of decoder d: which < 0 -> a_p[d][-which-1], else a_up[d][which]
        int ci0 = n->dec[0].seg[si];
        const Act& in0 = which < 0 ? n->a_p[0][-which - 1] : n->a_up[0][which];
        long long sb, sh, sw, sc;
        nhwc(in0, sb, sh, sw, sc);
        const Act& o0 = n->a_seg[0][si];
        fill_conv_args(n, a, n->convs[ci0], n->cplan[ci0], in0.H, in0.W, o0.H, o0.W, sb, sh, sw, sc, false, 0);
        for (int d = 0; d < 4; ++d) {
            const PackedConv& c = n->convs[n->dec[d].seg[si]];
            const Act& in = which < 0 ? n->a_p[d][-which - 1] : n->a_up[d][which];
            a.p[d] = ConvPtrs{ws + in.off, ws + c.w_off, ws + n->a_seg[d][si].off, nullptr, nullptr, nullptr, nullptr,
                              ws + n->gn_part_off[d][si]};
            if (c.wino_ok) a.wino_w[d] = ws + c.wino_off;
        }
        if (si == 6 && n->fold_ok) {      // s2.0: what its fold reads instead of p2
            a.fold_in = ws + feat[0].off;
            a.fold_cin = feat[0].C;
            for (int d = 0; d < 4; ++d) {
                a.fold_w[d] = ws + n->fold_img1_off[d];
                a.fold_w2[d] = ws + n->fold_img2_off[d];
                a.fold_up[d] = ws + n->a_p[d][2].off;
                a.fold_tab[d] = ws + n->fold_tab_off[d];
            }
            a.fold_lat_ms = n->tune_score[n->dec[0].lat[3]];
        }
        return run_conv(n, a, 4, ci0, s);
    };
    // GroupNorm statistics of up to kMaxGnSites finished sites -> per (image, channel) affines, one launch
    auto gn_finish = [&](std::initializer_list<int> sites) -> int {
        GnFinArgs g;
        memset(&g, 0, sizeof(g));
        int k = 0;
        for (int si : sites) {
            const Act& o0 = n->a_seg[0][si];
            for (int d = 0; d < 4; ++d) {
                g.gn_part[k * kMaxGroup + d] = ws + n->gn_part_off[d][si];
                g.gamma[k * kMaxGroup + d] = n->pptr[n->dec[d].p_gn[si]];
                g.beta[k * kMaxGroup + d] = n->pptr[n->dec[d].p_gn[si] + 1];
                g.affine[k * kMaxGroup + d] = ws + n->gn_aff_off[d][si];
            }
            g.P[k] = plan_gn_rows(n->cplan[n->dec[0].seg[si]], o0.H, o0.W, B, n->convs[n->dec[0].seg[si]].Cin, n->wino_pack, n->wino_orient);
            g.count[k] = (long long)o0.H * o0.W * 4;
            ++k;
        }
        g.B = B; g.C = 128; g.groups = 32; g.sites = k; g.eps = 1e-5f;
        return launch_gn_finalize(g, 4, s);
    };
    // GN + ReLU + x2 upsample of up to kMaxUpJobs sites (si -> a_up[ui]), one launch
    auto gn_up = [&](std::initializer_list<std::pair<int, int>> jobs) -> int {
        GnUpArgs u;
        memset(&u, 0, sizeof(u));
        int k = 0;
        for (const auto& job : jobs) {
            const int si = job.first, ui = job.second;
            for (int d = 0; d < 4; ++d) {
                u.in[k * kMaxGroup + d] = ws + n->a_seg[d][si].off;
                u.affine[k * kMaxGroup + d] = ws + n->gn_aff_off[d][si];
                u.out[k * kMaxGroup + d] = ws + n->a_up[d][ui].off;
            }
            u.h[k] = n->a_seg[0][si].H; u.w[k] = n->a_seg[0][si].W;
            ++k;
        }
        u.B = B; u.C = 128; u.jobs = k;
        return launch_gn_relu_up2(u, 4, s);
    };
    // the statistics of several sites are finalized together and both first-level upsamples share a launch:
    // 3 + 2 small launches per frame instead of 7 + 3 (each ~4.7 us of latency at batch 1)
    FPC_TRY(seg_conv(0, -1));   // s5.0 on p5
    FPC_TRY(seg_conv(3, -2));   // s4.0 on p4
    FPC_TRY(seg_conv(5, -3));   // s3.0 on p3
    FPC_TRY(seg_conv(6, -4));   // s2.0 on p2
    FPC_TRY(gn_finish({0, 3, 5, 6}));
    FPC_TRY(gn_up({{0, 0}, {3, 2}}));
    FPC_TRY(seg_conv(1, 0));    // s5.1 on up(s5.0)
    FPC_TRY(seg_conv(4, 2));    // s4.1 on up(s4.0)
    FPC_TRY(gn_finish({1, 4}));
    FPC_TRY(gn_up({{1, 1}}));
    FPC_TRY(seg_conv(2, 1));    // s5.2 on up(s5.1)
    FPC_TRY(gn_finish({2}));

    // merge + head
    const int lo[3] = {2, 4, 5};     // s5.2, s4.1, s3.0 (sum order of the reference: p5-, p4-, p3-, p2-branch)
    const int split = n->merge_split;      // resolved once in fpc_net_create (FPC_MERGE_SPLIT): graph and plain runs agree, no getenv per forward
    if (split) {
        // two passes (merge_split.hip): the head of (r5 + r4 + r3) at the branches' resolution, then the head of r2 + bias + its x2 upsample
        HeadPartArgs hl, hh;
        memset(&hl, 0, sizeof(hl));
        memset(&hh, 0, sizeof(hh));
        for (int d = 0; d < 4; ++d) {
            for (int k = 0; k < 3; ++k) {
                hl.t[d][k] = ws + n->a_seg[d][lo[k]].off;
                hl.aff[d][k] = ws + n->gn_aff_off[d][lo[k]];
            }
            hh.t[d][0] = ws + n->a_seg[d][6].off;
            hh.aff[d][0] = ws + n->gn_aff_off[d][6];
            hl.hw[d] = hh.hw[d] = n->pptr[n->dec[d].p_head_w];
            hl.hb[d] = hh.hb[d] = n->pptr[n->dec[d].p_head_b];
            hl.out[d] = ws + n->a_lsum[d].off;
            hh.lsum[d] = ws + n->a_lsum[d].off;
            hh.out[d] = ws + n->a_low[d].off;
            hl.ch[d] = hh.ch[d] = n->dec[d].head_ch;
            hl.chp[d] = hh.chp[d] = n->dec[d].head_chp;
        }
        hl.B = hh.B = B; hl.C = hh.C = 128;
        hl.H = n->a_seg[0][2].H; hl.W = n->a_seg[0][2].W; hl.hl = hl.H; hl.wl = hl.W;
        hh.H = n->a_seg[0][6].H; hh.W = n->a_seg[0][6].W; hh.hl = hl.H; hh.wl = hl.W;
        FPC_TRY(launch_head_part(hl, false, 4, s));
        FPC_TRY(launch_head_part(hh, true, 4, s));
    } else {
        MergeHeadArgs m;
        memset(&m, 0, sizeof(m));
        for (int d = 0; d < 4; ++d) {
            for (int k = 0; k < 3; ++k) {
                m.t_lo[d][k] = ws + n->a_seg[d][lo[k]].off;
                m.a_lo[d][k] = ws + n->gn_aff_off[d][lo[k]];
            }
            m.t_hi[d] = ws + n->a_seg[d][6].off;
            m.a_hi[d] = ws + n->gn_aff_off[d][6];
            m.hw[d] = n->pptr[n->dec[d].p_head_w];
            m.hb[d] = n->pptr[n->dec[d].p_head_b];
            m.out[d] = ws + n->a_low[d].off;
            m.ch[d] = n->dec[d].head_ch;
            m.chp[d] = n->dec[d].head_chp;
        }
        m.B = B; m.h = n->a_seg[0][2].H; m.w = n->a_seg[0][2].W; m.C = 128;
        FPC_TRY(launch_merge_head(m, 4, s));
    }
    return FPC_OK;
}

extern "C" int fpc_net_forward(fpc_net_t* n, const float* x, float* logits_mask, float* logits_quat,
                               float* logits_scales, float* logits_xy, float* logits_z, int64_t* cat_mask, float* cq,
                               float* cs, float* cxy, float* cz, fpc_stream_t stream) {
    return fpc_net_forward_bits(n, x, logits_mask, logits_quat, logits_scales, logits_xy, logits_z, cat_mask, cq, cs, cxy, cz, nullptr, stream);
}

static int forward_bits(fpc_net_t* n, const float* x, float* logits_mask, float* logits_quat, float* logits_scales,
                        float* logits_xy, float* logits_z, int64_t* cat_mask, float* cq, float* cs, float* cxy, float* cz,
                        uint64_t* fg_bits, fpc_stream_t stream);

extern "C" int fpc_net_forward_bits(fpc_net_t* n, const float* x, float* logits_mask, float* logits_quat,
                                    float* logits_scales, float* logits_xy, float* logits_z, int64_t* cat_mask, float* cq,
                                    float* cs, float* cxy, float* cz, uint64_t* fg_bits, fpc_stream_t stream) {
    const int rc = forward_bits(n, x, logits_mask, logits_quat, logits_scales, logits_xy, logits_z, cat_mask, cq, cs, cxy, cz, fg_bits, stream);
    if (n) n->survey = nullptr;      // a survey is armed for ONE call, whatever became of it (a refused call included): never a stale pointer
    return rc;
}

static int forward_bits(fpc_net_t* n, const float* x, float* logits_mask, float* logits_quat, float* logits_scales,
                        float* logits_xy, float* logits_z, int64_t* cat_mask, float* cq, float* cs, float* cxy, float* cz,
                        uint64_t* fg_bits, fpc_stream_t stream) {
    if (!n || !n->loaded || !x || !cat_mask || !cq || !cs || !cxy || !cz) return FPC_EINVAL;
    if (fg_bits && (n->W % 64 != 0 || ((uintptr_t)fg_bits & 7))) return FPC_EINVAL;
    bool any = logits_mask || logits_quat || logits_scales || logits_xy || logits_z;
    bool all = logits_mask && logits_quat && logits_scales && logits_xy && logits_z;
    if (any && !all) return FPC_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* ws = n->ws;
    const int B = n->B, H = n->H, W = n->W;

    // stem: image -> NHWC4 (16-byte pixels), 7x7/2 with BN + ReLU in the epilogue
    FPC_TRY(launch_nchw3_to_nhwc4(x, ws + n->a_img4.off, B, H * W, s));
    // graph replay needs a capturable stream: not the null (legacy default) stream
    const bool plain = n->tuning || n->survey;      // a tuning or a survey forward launches its kernels: no capture, no replay
    if (n->use_graph && !plain && s != nullptr && !n->graph_exec) {
        // first such frame after tuning: record the launches instead of running them
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            int rc = forward_middle(n, s);
            hipError_t e = hipStreamEndCapture(s, &g);
            if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (e == hipSuccess && g) e = hipGraphInstantiate(&n->graph_exec, g, nullptr, nullptr, 0);
            if (g) (void)hipGraphDestroy(g);
            if (e != hipSuccess) n->graph_exec = nullptr;
        }
        if (!n->graph_exec) { (void)hipGetLastError(); n->use_graph = 0; }      // not capturable here: plain launches from now on
    }
    if (n->use_graph && !plain && s != nullptr && n->graph_exec) {
        if (hipGraphLaunch(n->graph_exec, s) != hipSuccess) return FPC_ELAUNCH;
    } else {
        FPC_TRY(forward_middle(n, s));
    }
    {
        Up4Args u;
        memset(&u, 0, sizeof(u));
        u.lm = ws + n->a_low[0].off; u.lq = ws + n->a_low[1].off; u.lt = ws + n->a_low[2].off; u.ls = ws + n->a_low[3].off;
        u.pm = n->dec[0].head_chp; u.pq = n->dec[1].head_chp; u.pt = n->dec[2].head_chp; u.ps = n->dec[3].head_chp;
        u.o_mask = logits_mask; u.o_quat = logits_quat; u.o_scales = logits_scales; u.o_xy = logits_xy; u.o_z = logits_z;
        u.cat_mask = (long long*)cat_mask; u.cq = cq; u.cs = cs; u.cxy = cxy; u.cz = cz;
        u.B = B; u.hl = n->a_low[0].H; u.wl = n->a_low[0].W; u.H = H; u.W = W; u.C = n->classes;
        u.fg_bits = reinterpret_cast<unsigned long long*>(fg_bits); u.fg_stride = (size_t)((H * W + 4095) / 4096) * 64;
        if (u.hl * 4 != H || u.wl * 4 != W) return FPC_EINVAL;
        FPC_TRY(launch_up4_compress(u, s, n->up4_wide != 0));
    }
    if (n->tuning) { n->tuning = false; n->tuned = true; }
    return FPC_OK;
}

// The NEXT fpc_net_forward times every candidate tiling of every convolution site on the device
// (it synchronises the stream; not capturable) and keeps the fastest; later forwards reuse the plans.
extern "C" int fpc_net_autotune_next(fpc_net_t* n, int mode) {
    if (!n || !n->loaded || mode < 0 || mode > 2) return FPC_EINVAL;
    n->tuning = true;
    n->tune_mode = mode;
    drop_graph(n);      // tilings may change
    return FPC_OK;
}

// The NEXT fpc_net_forward, and only that one, also surveys the activations: in front of every convolution site's launch k_act_range
// (act_range.hip) accumulates max |x| over the finite elements, the non-finite count and the visit count of every tensor the site's
// CURRENT plan reads as its matrix operand into records_dev[4 * site] (device memory the caller owns and zeroed; grouped sites: the
// four decoders into the index of decoder 0).  That forward launches its kernels (no graph capture or replay, as a tuning pass),
// changes no plan and writes what an ordinary forward writes.  sites = fpc_net_conv_count.  The survey is disarmed when that call
// returns, whatever it returns, and by records_dev = NULL.
extern "C" int fpc_net_survey_next(fpc_net_t* n, unsigned* records_dev, int sites) {
    if (n && !records_dev) { n->survey = nullptr; return FPC_OK; }      // NULL disarms (the caller's buffer is going away)
    if (!n || !n->loaded || ((uintptr_t)records_dev & 3) || sites != (int)n->convs.size()) return FPC_EINVAL;
    n->survey = records_dev;
    return FPC_OK;
}

// The plan a range-limited site falls back to: the autotuner's best range-free candidate where the site was tuned, else what the
// planner gives at split level 1 — a Winograd site (the folded s2.0 too: its p2 lateral keeps its own, never range-limited, plan and
// runs again) form -7 where offered, else -5; a three-product direct or lateral plan the same tiling or parts on bf16 x 3; the fused
// stem + max-pool what fpc_net_force_stem_pool(net, 0) restores.
static ConvPlan range_free_plan(const fpc_net* n, int i) {
    if (n->has_free[i]) return n->free_plan[i];
    const PackedConv& c = n->convs[i];
    ConvPlan q = n->cplan[i];
    if (q.pool) { ConvPlan st; st.stem = 256; return st; }
    if (q.wino) {
        q.wino = wino_form_ok(kWinoW4, c.Cin, c.Cout) ? kWinoW4 : kWinoBf3;
        q.fold = 0;
        return q;
    }
    q.h3 = 0; q.bf3 = 1;
    return q;
}

// Host arithmetic only.  records_host: the records of a survey forward, copied to the host.  Every site whose current plan is
// range-limited (plan_range_limited) and whose record shows a non-finite element, max |x| >= hi or 0 < max |x| < lo is demoted to
// its range-free plan (range_free_plan) and stays so: fpc_net_guarded reports it, fpc_net_load_params keeps it, fpc_net_copy_plans
// carries it, a later autotuning pass offers the site no fp16-piece form; only an explicit fpc_net_force_* puts it back.  A record
// of all zeros (every form is exact on zeros) or with no visit (not surveyed) demotes nothing.  The folded s2.0 has two operands of
// two scales and two records: c2 in its own, p3 in the p2 lateral site's; either one outside demotes it.  Returns the number of sites demoted by
// THIS call (a second call with the same records: 0) and drops the recorded graph when that is not zero.
extern "C" int fpc_net_guard_ranges(fpc_net_t* n, const unsigned* records_host, int sites, float lo, float hi) {
    if (!n || !records_host || sites != (int)n->convs.size() || !(lo >= 0.f) || !(hi > lo)) return FPC_EINVAL;
    auto outside = [&](int site) {
        const unsigned* rec = records_host + 4 * (size_t)site;
        float mx;
        memcpy(&mx, &rec[0], sizeof(mx));
        return rec[2] != 0 && (rec[1] > 0 || mx >= hi || (mx > 0.f && mx < lo));
    };
    int demoted = 0;
    for (int i = 0; i < sites; ++i) {
        if (!n->c_groups[i] || !plan_range_limited(n->cplan[i]) || records_host[4 * (size_t)i + 2] == 0) continue;
        // (the folded s2.0: its second operand, p3, was surveyed into the p2 lateral's record)
        if (!(outside(i) || (n->cplan[i].fold && outside(n->dec[0].lat[3])))) continue;
        n->cplan[i] = range_free_plan(n, i);
        n->guarded[i] = 1;
        ++demoted;
    }
    if (demoted) drop_graph(n);
    return demoted;
}

// 1: site `i` stands demoted by fpc_net_guard_ranges, 0: not (or no such site)
extern "C" int fpc_net_guarded(const fpc_net_t* n, int i) {
    return n && i >= 0 && i < (int)n->guarded.size() && n->guarded[i] ? 1 : 0;
}

// Chosen tiling of convolution site `i` (0 <= i < fpc_net_conv_count): out5 = bm, bn, nsplit, Cout, K.  nsplit 5000: the p2 lateral
// site, folded into s2.0's launch (which reports -9).
extern "C" int fpc_net_conv_count(const fpc_net_t* n) { return n ? (int)n->convs.size() : 0; }
extern "C" int fpc_net_conv_plan(const fpc_net_t* n, int i, int* out5) {
    if (!n || !out5 || i < 0 || i >= (int)n->convs.size()) return FPC_EINVAL;
    const ConvPlan& p = n->cplan[i];
    out5[0] = p.bm; out5[1] = p.bn;
    if (p.lat) { out5[0] = 128; out5[1] = 32; }      // k_lateral1x1
    if (p.stem) { out5[0] = 64; out5[1] = 64; }      // k_stem7x7 / k_stem_pool_h3 (with the max-pool)
    if (p.pw) { out5[0] = pw_tile_pixels(p.pw - 1); out5[1] = 64; }      // k_conv1x1
    if (p.grp) { out5[0] = 8 * grouped_tile_cols(n->convs[i].stride); out5[1] = 32; }      // k_conv3x3_grouped
    out5[2] = encode_plan(p, n->fold_ok && i == n->dec[0].lat[3] && n->cplan[n->dec[0].seg[6]].fold);
    out5[3] = n->convs[i].Cout; out5[4] = n->convs[i].K;
    return FPC_OK;
}

// Every 3x3 / stride-1 site that has Winograd images -> Winograd form `form` (1..9, fpc_conv2d's -form; wino_form_ok: 6 only where
// Cout % 128 == 0, 9 only where Cin % 16 == 0; other sites keep their plan): tests run the whole network on ONE form (e.g. 8: every eligible product on fp16 x 2 pieces) and
// hold it to the float64 bars.  Returns the number of sites changed, or a negative code.  Drops the recorded graph.
extern "C" int fpc_net_force_winograd(fpc_net_t* n, int form) {
    if (!n || form < 1 || form >= kWinoFormCount) return FPC_EINVAL;
    int changed = 0;
    for (size_t i = 0; i < n->convs.size(); ++i) {
        const PackedConv& c = n->convs[i];
        if (!c.wino_ok || !n->c_groups[i] || !wino_form_ok(form, c.Cin, c.Cout)) continue;
        ConvPlan q = n->cplan[i];
        q.wino = form; q.lat = 0; q.stem = 0;
        if (form != kWinoH3) q.fold = 0;      // (form 9 keeps s2.0's fold: it runs on that form)
        n->cplan[i] = q;
        n->guarded[i] = 0;      // an explicit request wins over the range guard
        ++changed;
    }
    drop_graph(n);
    return changed;
}

// s2.0 with the FPN p2 level folded in (on = 1; ResNet-18/34 plans) or back on its unfolded form 9 plan (on = 0).  Returns 1 when the
// plan changed, 0 when it was already so, or a negative code.  Drops the recorded graph.
extern "C" int fpc_net_force_fold(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1 || (on && !n->fold_ok)) return FPC_EINVAL;
    ConvPlan& p = n->cplan[n->dec[0].seg[6]];
    if (p.fold == on) return 0;
    ConvPlan q;
    q.wino = kWinoH3; q.fold = on;
    p = q;
    n->guarded[n->dec[0].seg[6]] = 0;
    drop_graph(n);
    return 1;
}

// Every 1x1 site k_conv1x1 takes (Cin and Cout multiples of 64, no padding) -> k_conv1x1 (on = 1: the variant the site was
// tuned to, else 64-pixel tiles) or back to the heuristic k_conv_igemm tiling (on = 0; sites already there are not counted).
// Returns the number of sites changed, or a negative code.  Drops the recorded graph.
extern "C" int fpc_net_force_pointwise(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1) return FPC_EINVAL;
    int changed = 0;
    for (size_t i = 0; i < n->convs.size(); ++i) {
        const PackedConv& c = n->convs[i];
        if (!n->c_groups[i] || c.Kh != 1 || c.pad != 0 || c.Cinp != c.Cin || c.Cin % 64 || c.Kpad != c.Cin || c.Cout % 64) continue;
        if (on) {
            if (n->cplan[i].pw) continue;
            ConvPlan q;
            q.pw = 1;
            n->cplan[i] = q;
        } else {
            if (!n->cplan[i].pw) continue;
            n->cplan[i] = plan_conv(n->c_howo[i], n->B, c.Cout, c.Kpad / kConvBK, n->c_groups[i]);
        }
        ++changed;
    }
    drop_graph(n);
    return changed;
}

// Every site with a k_pack_weight_h3 image (PackedConv::h3_ok; packed at split level 3 only) -> the three-product form (on = 1: a
// k_lateral1x1 site on its two-piece build, any other on its own k_conv_igemm tiling or the heuristic one) or back to the heuristic
// f32 tiling (on = 0; sites not on the form are not counted).  Returns the number of sites changed, or a negative code.  Drops the recorded graph.
extern "C" int fpc_net_force_direct_h3(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1 || (on && !n->h3_packed)) return FPC_EINVAL;      // (the images are packed at split level 3 only)
    int changed = 0;
    for (size_t i = 0; i < n->convs.size(); ++i) {
        const PackedConv& c = n->convs[i];
        if (!c.h3_ok || !n->c_groups[i] || on == n->cplan[i].h3) continue;
        const ConvPlan& p = n->cplan[i];
        ConvPlan q = plan_conv(n->c_howo[i], n->B, c.Cout, c.Kpad / kConvBK, n->c_groups[i]);
        if (on && !p.wino && !p.stem && !p.pw) q = p;      // (a k_lateral1x1 site stays on it, on two pieces)
        q.bf3 = 0;
        q.h3 = on;
        n->cplan[i] = q;
        n->guarded[i] = 0;
        ++changed;
    }
    drop_graph(n);
    return changed;
}

// The stem and its max-pool as one launch (on = 1: k_stem_pool_h3, split level 3 only — its weight image is packed there — and a
// shape the launcher takes: conv output rows even, columns a multiple of 64) or back on k_stem7x7 + k_maxpool3x3s2 (on = 0).  Returns 1
// when the plan changed, 0 when it was already so, or a negative code.  Drops the recorded graph.
extern "C" int fpc_net_force_stem_pool(fpc_net_t* n, int on) {
    if (!n || on < 0 || on > 1 || (on && !n->h3_packed)) return FPC_EINVAL;
    if (n->c_stem < 0) return FPC_EINVAL;      // the MobileNetV2, EfficientNet and VGG encoders: no 7x7 stem and no 3x3 max-pool, whatever `on` is
    if (on && n->enc.resnet.ceil_pool()) return FPC_EINVAL;      // the SE-ResNet stem pool has no padding: the fused launch computes another pool
    if (on && ((n->a_stem.H & 1) || (n->a_stem.W & 63) || (long long)n->H * n->W * 16 >= (1LL << 31))) return FPC_EINVAL;
    ConvPlan& p = n->cplan[n->c_stem];
    if (p.pool == on) return 0;
    ConvPlan q;
    q.stem = 256; q.pool = on;
    p = q;
    n->guarded[n->c_stem] = 0;
    drop_graph(n);
    return 1;
}

// Plans of `src` -> `dst` (same encoder, classes, H, W; batch sizes may differ): runs a small batch on the tilings, split-K
// factors and kernel forms a larger one was autotuned to (tests: the headline configuration's kernels against float64 on two
// frames).  A plan whose split-K partials do not fit dst's workspace keeps dst's own.  Drops dst's recorded graph.
extern "C" int fpc_net_copy_plans(fpc_net_t* dst, const fpc_net_t* src) {
    if (!dst || !src || dst->convs.size() != src->convs.size() || dst->H != src->H || dst->W != src->W) return FPC_EINVAL;
    for (size_t i = 0; i < dst->convs.size(); ++i) {
        const PackedConv &a = dst->convs[i], &b = src->convs[i];
        if (a.Cin != b.Cin || a.Cout != b.Cout || a.Kh != b.Kh || a.Kw != b.Kw || a.stride != b.stride || a.Npad != b.Npad ||
            a.Kpad != b.Kpad || a.cg != b.cg || dst->c_groups[i] != src->c_groups[i])
            return FPC_EINVAL;
    }
    for (size_t i = 0; i < dst->convs.size(); ++i) {
        const ConvPlan& q = src->cplan[i];
        if (splitk_floats_for(q, dst->c_groups[i] ? dst->c_groups[i] : 1, dst->B, dst->convs[i].Npad) > dst->splitk_floats) continue;
        if (q.nsplit > 1 && q.fused && !can_fuse(q, dst->c_groups[i] ? dst->c_groups[i] : 1, dst->B)) continue;
        if ((q.h3 || q.pool) && !dst->h3_packed) continue;      // dst is not at split level 3: no three-product images
        dst->cplan[i] = q;
    }
    // the range guard's state: the fallback plans (where they fit dst as above) and the demotions — a site that stands demoted in src
    // or in dst is demoted in dst afterwards, also where dst kept a plan of its own or src's plan for it is an fp16-piece form
    for (size_t i = 0; i < dst->convs.size(); ++i) {
        const ConvPlan& q = src->free_plan[i];
        const int groups = dst->c_groups[i] ? dst->c_groups[i] : 1;
        dst->has_free[i] = src->has_free[i] && splitk_floats_for(q, groups, dst->B, dst->convs[i].Npad) <= dst->splitk_floats &&
                           !(q.nsplit > 1 && q.fused && !can_fuse(q, groups, dst->B));
        if (dst->has_free[i]) dst->free_plan[i] = q;
        dst->guarded[i] = dst->guarded[i] || src->guarded[i];      // (a demotion of dst's own is never undone by a copy)
        if (dst->guarded[i] && plan_range_limited(dst->cplan[i])) dst->cplan[i] = range_free_plan(dst, (int)i);
    }
    dst->tuned = true;
    drop_graph(dst);
    return FPC_OK;
}

// FLOP of one forward over the whole batch: out3[0] = 2 x MACs of the direct convolutions (the algorithmic count the
// reference's cuDNN path would execute), out3[1] = multiply-adds the CURRENT plans execute (a Winograd F(2x2,3x3)
// site does 16 instead of 36 per 2x2 output tile: direct / 2.25), out3[2] = share of out3[0] on Winograd sites.
extern "C" int fpc_net_flops(const fpc_net_t* n, double* out3) {
    if (!n || !out3) return FPC_EINVAL;
    double direct = 0.0, executed = 0.0, wino = 0.0;
    for (size_t i = 0; i < n->convs.size(); ++i) {
        if (!n->c_groups[i]) continue;
        const PackedConv& c = n->convs[i];
        const double f = 2.0 * n->B * (double)n->c_howo[i] * c.Cout * (c.cg ? c.cg : c.Cin) * c.Kh * c.Kw * n->c_groups[i];
        direct += f;
        if (n->cplan[i].wino) { executed += f / 2.25; wino += f; } else executed += f;
    }
    for (const fpc_net::MbOp& o : n->mops) {      // the MobileNetV2 and EfficientNet ops: 27 (stem), k k (depthwise) or Cin products per output
        const bool stem = o.kind == fpc_net::kMbStem || o.kind == fpc_net::kMbSameStem, dw = o.kind == fpc_net::kMbDw || o.kind == fpc_net::kMbSameDw;
        const double f = 2.0 * n->B * (double)o.howo * o.Cout * (stem ? 27 : dw ? o.k * o.k : o.Cin);
        direct += f; executed += f;
    }
    for (const fpc_net::DnOp& o : n->dops) {      // the DenseNet ops' products: K per output of a 1x1, 9 x 128 of a 3x3
        if (o.kind != fpc_net::kDnPw && o.kind != fpc_net::kDnConv3) continue;
        const double f = 2.0 * n->B * (double)o.H * o.W * o.Cout * (o.kind == fpc_net::kDnConv3 ? 9 * 128 : o.K);
        direct += f; executed += f;
    }
    if (n->vgg0.p_w >= 0) {      // features.0 of a VGG encoder: 27 products per output
        const double f = 2.0 * n->B * (double)n->H * n->W * 64 * 27;
        direct += f; executed += f;
    }
    for (int d = 0; d < 4; ++d)      // the 1x1 heads run inside k_merge_head
        direct += 2.0 * n->B * (double)n->a_low[d].H * n->a_low[d].W * 128.0 * n->dec[d].head_ch,
        executed += 2.0 * n->B * (double)n->a_low[d].H * n->a_low[d].W * 128.0 * n->dec[d].head_ch;
    out3[0] = direct; out3[1] = executed; out3[2] = direct > 0.0 ? wino / direct : 0.0;
    return FPC_OK;
}

// Debug / test access to the engine's intermediate activations (NHWC f32 inside the workspace).
// name: "stem", "pool", "c2".."c5", "d<k>.p5".."d<k>.p2", "d<k>.seg<i>" (pre-GroupNorm), "d<k>.low".
extern "C" int fpc_net_tensor(const fpc_net_t* n, const char* name, const float** ptr, int* H, int* W, int* C) {
    if (!n || !n->ws || !name || !ptr || !H || !W || !C) return FPC_EINVAL;
    Act t;
    bool ok = false;
    if (!strcmp(name, "stem")) {
        if (n->c_stem >= 0 && n->cplan[n->c_stem].pool) return FPC_EINVAL;      // fused with the max-pool: never written
        t = n->a_stem; ok = true;
    }
    else if (!strcmp(name, "pool")) { t = n->a_pool; ok = n->a_pool.C > 0; }      // (the MobileNetV2 encoder has none)
    else if (name[0] == 'c' && name[1] >= '2' && name[1] <= '5' && !name[2]) { t = n->a_feat[name[1] - '2']; ok = true; }
    else if (name[0] == 'd' && name[1] >= '0' && name[1] <= '3' && name[2] == '.') {
        int d = name[1] - '0';
        const char* r = name + 3;
        if (r[0] == 'p' && r[1] >= '2' && r[1] <= '5' && !r[2]) {
            if (r[1] == '2' && n->cplan[n->dec[0].seg[6]].fold) return FPC_EINVAL;      // folded into s2.0: never written
            t = n->a_p[d]['5' - r[1]]; ok = true;
        }
        else if (!strncmp(r, "seg", 3) && r[3] >= '0' && r[3] <= '6' && !r[4]) { t = n->a_seg[d][r[3] - '0']; ok = true; }
        else if (!strcmp(r, "low")) { t = n->a_low[d]; ok = true; }
    }
    if (!ok) return FPC_EINVAL;
    *ptr = n->ws + t.off; *H = t.H; *W = t.W; *C = t.C;
    return FPC_OK;
}

