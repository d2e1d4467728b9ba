// net_plan.hpp — what a plan of the backbone engine is, host only: the encoder block kinds, the encoder descriptor, the encoder
// tape's steps and struct fpc_net.  Shared by net_build.hip, which builds a plan, and net.hip, which loads, tunes, guards and runs
// it; both speak the planner's names (conv_plan.hpp) unqualified, as this header does.
#pragma once
#include <string>

#include "conv_plan.hpp"

using namespace fpc;

// ---- the encoder block kinds, each stated once.  A block is up to three convolution sites with BatchNorm in PARAMETER order
// (encoder.layerN.i.conv1 / bn1, conv2 / bn2, conv3 / bn3), each between two of the block's buffers, then — SE only — the four
// se_module parameters, then the downsample (1x1 with the block's stride and BatchNorm, In -> D) where the block's stride is not 1 or
// its channels change.  Channels follow from the buffers: In has the predecessor's, T1 and T2 planes * width / 64 * groups, D and Y
// planes * expansion.  The ResNet family's builder (net_build.hip) turns this statement into the parameter table, the activation
// buffers and the encoder tape.
enum Buf { kBufNone, kBufIn, kBufT1, kBufT2, kBufD, kBufY, kBufRes, kBufCount };      // Res: D where the block has a downsample, else In
// k: 3 = 3x3 / pad 1, 1 = 1x1 / pad 0; strided: the site that carries the block's stride; grouped: a grouped 3x3 (add_grouped_conv) in
// an encoder with groups, dense in every other; res: the residual added in the epilogue, or kBufNone
struct BlockSite { int k; bool strided, grouped; Buf in, out; bool relu; Buf res; };
struct BlockKind {
    int nsites;
    BlockSite site[3];
    int ds_before;           // LAUNCH order: the downsample runs in front of this site, whose epilogue (or whose gate) consumes it
    bool se_gate;            // se_module.fc1 / fc2 (weight, bias) behind the last site's parameters; behind its launch the gate step: Y's
                             // channel means, the two fc layers, then Y = relu(Y * gate + Res) in place (se.hip: three launches)
    bool shared;             // true: a stage's blocks share T1 (block 0's, the largest), T2, D and two outputs in turn — only a block's
                             // output feeds the next block, which reads it as input and residual; false: every block has its own T1, Y, D
};
// BasicBlock: 3x3 (stride) -> 3x3 + residual
constexpr BlockKind kBasicBlock = {2, {{3, true, false, kBufIn, kBufT1, true, kBufNone}, {3, false, false, kBufT1, kBufY, true, kBufRes}}, 1, false, false};
// torchvision's Bottleneck: 1x1 -> 3x3 (stride; grouped in the ResNeXt encoders) -> 1x1 x 4 + residual
constexpr BlockKind kBottleneck = {3, {{1, false, false, kBufIn, kBufT1, true, kBufNone}, {3, true, true, kBufT1, kBufT2, true, kBufNone}, {1, false, false, kBufT2, kBufY, true, kBufRes}}, 2, false, true};
// pretrainedmodels' SEResNetBottleneck: 1x1 (stride) -> 3x3 (a Winograd site at every stage) -> 1x1 x 4 with BatchNorm only -> gate
constexpr BlockKind kSEBottleneck = {3, {{1, true, false, kBufIn, kBufT1, true, kBufNone}, {3, false, false, kBufT1, kBufT2, true, kBufNone}, {1, false, false, kBufT2, kBufY, false, kBufNone}}, 2, true, true};

// ---- the encoder descriptor: all that tells one encoder from another.  An encoder belongs to a FAMILY, which builds its parameters,
// buffers and tape (net_build.hip: kFamilies).  Only the block statements above, this descriptor and the families' builders know a
// family; the rest of the engine walks the tape.
enum EncoderFamily {
    kFamilyResNet,           // the 7x7 stem, a max-pool, then stage by stage blocks of one of the kinds above
    kFamilyMobileNetV2,      // torchvision's MobileNetV2 features: none of the block kinds (net_build.hip: "the MobileNetV2 encoder")
    kFamilyEfficientNet,     // efficientnet_pytorch's MBConv blocks by a table of block arguments (net_build.hip: "the EfficientNet encoders")
    kFamilyDenseNet,         // torchvision's DenseNet features: the ResNet family's stem, then dense blocks and transitions (net_build.hip: "the DenseNet encoders")
    kFamilyVgg,              // torchvision's VGG features: features.0 on its own kernel, 3x3 conv sites and 2x2 max-pools (net_build.hip: "the VGG encoders")
    kFamilyCount
};
// What the ResNet family asks beside the blocks per stage; no other family has one, so no other family is asked these questions.
struct ResNetDesc {
    int expansion = 1;            // 1: BasicBlock encoder, 4: Bottleneck (1x1, 3x3 with the stride, 1x1 x 4)
    int groups = 1, width = 64;   // Bottleneck: conv2's groups and torchvision's width_per_group (ResNeXt: 32 and 4 / 8); (1, 64) = ResNet
    int se = 0;                   // > 0: the SE-ResNet Bottleneck (pretrainedmodels.senet) with this reduction; expansion is 4 then
    const BlockKind& kind() const { return se ? kSEBottleneck : expansion == 4 ? kBottleneck : kBasicBlock; }
    const char* stem_prefix() const { return se ? "encoder.layer0." : "encoder."; }      // torchvision's stem names, pretrainedmodels'
    // the SE-ResNet stem pool: no padding, ceil_mode (other windows, the same size on the even maps every plan has): its own max-pool launch, never the fused stem + pool
    bool ceil_pool() const { return se != 0; }
};
struct EncoderDesc {
    EncoderFamily family = kFamilyResNet;
    ResNetDesc resnet;            // read where family == kFamilyResNet only; a VGG row keeps two ints of its own in it (vgg_block1, vgg_bn)
    int layers[4] = {};           // ResNet: blocks per stage; MobileNetV2: the feature modules per stage of smp's last four, behind features.1;
                                  // EfficientNet: the MBConv blocks per stage of smp's last four; DenseNet: the dense layers per block;
                                  // VGG: the convolutions of blocks 2 .. 5
    int vgg_block1() const { return resnet.expansion; }      // VGG rows: the convolutions of block 1 (1 or 2) ...
    bool vgg_bn() const { return resnet.groups != 0; }        // ... and whether a BatchNorm follows every convolution (the _bn variants)
    bool basic() const { return family == kFamilyResNet && resnet.expansion == 1; }         // c2 has 64 channels: s2.0 may fold the FPN p2 level in, and the direct sites have three-product images
    bool pointwise() const { return family == kFamilyResNet && resnet.expansion == 4; }     // the autotuner offers k_conv1x1 to the 1x1 sites
};

// ---- the encoder tape: every launch between the image and the decoders but the ResNet family's stem and max-pool, in launch order.
// A step has one kind, which says what `op` indexes, and is made by that kind's maker below and by nothing else.
enum StepKind {
    kStepConv,       // op: a conv site (fpc_net::convs) from `in` to `out`, with BatchNorm, the residual `res` (C > 0) and ReLU in its epilogue
    kStepSeGate,     // op: the first of se_module's four parameters; an SE block's gate on `out` in place, with the residual `res`
    kStepMb,         // op: an op of the MobileNetV2 or EfficientNet encoder (fpc_net::mops, whose MbOp::kind names the kernel) from `in` to `out`; a 1x1 adds `res` (C > 0)
    kStepMbGate,     // op: an MBConv block's gate (fpc_net::mgates) from the depthwise output `in`; writes the plan's gate buffer, which the block's project op reads
    kStepDense,      // op: an op of a DenseNet encoder (fpc_net::dops, whose DnOp::kind names the kernel); the op itself carries its buffer offsets, pitches and c0: `in` / `out` say which tensors it reads and writes
    kStepVggStem,    // features.0 of a VGG encoder (fpc_net::vgg0) from the NHWC4 image `in` to `out`, bias or folded BatchNorm and ReLU in its epilogue
    kStepPool2       // MaxPool2d(2, 2) from `in` to `out` (vgg.hip: k_maxpool2x2); op unused
};
struct Step { StepKind kind; int op; Act in, out; bool relu; Act res; };
inline Step conv_step(int conv, const Act& in, const Act& out, bool relu, const Act& res = Act()) {
    Step s; s.kind = kStepConv; s.op = conv; s.in = in; s.out = out; s.relu = relu; s.res = res; return s;
}
inline Step se_gate_step(int p_se, const Act& y, const Act& res) {      // Y = relu(Y * gate + res)
    Step s; s.kind = kStepSeGate; s.op = p_se; s.in = s.out = y; s.relu = true; s.res = res; return s;
}
inline Step mb_step(int mop, const Act& in, const Act& out, const Act& res = Act()) {      // (the activation is the op's own: MbOp::act)
    Step s; s.kind = kStepMb; s.op = mop; s.in = in; s.out = out; s.relu = false; s.res = res; return s;
}
inline Step mb_gate_step(int gate, const Act& x) {      // (`out` is the operand too: the gate itself lies in fpc_net::mb_gate_off)
    Step s; s.kind = kStepMbGate; s.op = gate; s.in = s.out = x; s.relu = false; return s;
}
inline Step dense_step(int dop, const Act& in, const Act& out) {
    Step s; s.kind = kStepDense; s.op = dop; s.in = in; s.out = out; s.relu = false; return s;
}
inline Step vgg_stem_step(const Act& img, const Act& out) {
    Step s; s.kind = kStepVggStem; s.op = 0; s.in = img; s.out = out; s.relu = true; return s;
}
inline Step pool2_step(const Act& in, const Act& out) {
    Step s; s.kind = kStepPool2; s.op = 0; s.in = in; s.out = out; s.relu = false; return s;
}

struct fpc_net {
    EncoderDesc enc;
    int classes, B, H, W;
    std::vector<std::string> pnames;
    std::vector<int64_t> pnumel;
    std::vector<const float*> pptr;
    std::vector<PackedConv> convs;
    size_t packed_floats = 0;     // packed weights + folded BN region (persistent across forwards)
    size_t total_floats = 0;      // + activations and scratch
    float* ws = nullptr;
    bool loaded = false;
    bool tuning = false;          // next forward times every candidate tiling per conv site and keeps the best
    bool tuned = false;
    int tune_mode = 0;            // 0: minimise latency, 1: latency x sqrt(share of the chip occupied)

    // conv indices
    int c_stem = -1;              // the 7x7 stem site (ResNet family), which runs with its max-pool in front of the tape; -1: the encoder has none
    std::vector<Step> tape;
    // The MobileNetV2 encoder's ops: the stem, a depthwise 3x3 or a 1x1, each with BatchNorm folded into scale / shift and ReLU6 where
    // act = 1.  One form each (mobilenet.hip): not PackedConv sites, not tuned, not surveyed; the weights are read in place.
    // The EfficientNet encoder's ops are further kinds of the same list (efficientnet.hip): the stem, a depthwise k x k and a 1x1 with the
    // static "same" pads, swish where act = 2, BatchNorm's eps 1e-3, and — the project 1x1 — `gate`, the MBConv gate (mgates) whose
    // values multiply the op's input; -1: none.  The same rules: one form each, not tuned, not surveyed.
    enum MbKind { kMbStem, kMbDw, kMbPw, kMbSameStem, kMbSameDw, kMbGatedPw };
    struct MbOp { MbKind kind; int p_w, p_bn, Cin, Cout, stride, act; size_t scale_off, shift_off; long long howo; int k; float eps; int gate; };
    std::vector<MbOp> mops;
    int add_mop(MbKind kind, const std::string& wname, int64_t wnumel, const std::string& bn, int Cin, int Cout, int stride, int act,
                int k = 3, float eps = 1e-5f, int gate = -1) {
        MbOp o{kind, add_param(wname, wnumel), add_bn(bn, Cout), Cin, Cout, stride, act, 0, 0, 0, k, eps, gate};
        o.scale_off = alloc(Cout); o.shift_off = alloc(Cout);
        mops.push_back(o);
        return (int)mops.size() - 1;
    }
    // An MBConv block's gate: _se_reduce (weight [Cs][C], bias) and _se_expand (weight [C][Cs], bias), four parameters from p on, read
    // in place; sigmoid(expand(swish(reduce(mean_hw(x))))) of the depthwise output x [B][H][W][C] -> mb_gate_off [B][C]
    struct MbGate { int p, C, Cs; };
    std::vector<MbGate> mgates;
    int add_mgate(const std::string& prefix, int C, int Cs) {
        const int p = add_param(prefix + "_se_reduce.weight", (int64_t)Cs * C);
        add_param(prefix + "_se_reduce.bias", Cs);
        add_param(prefix + "_se_expand.weight", (int64_t)C * Cs);
        add_param(prefix + "_se_expand.bias", C);
        mgates.push_back(MbGate{p, C, Cs});
        return (int)mgates.size() - 1;
    }
    // The DenseNet encoders' ops behind the stem and its max-pool (densenet.hip), in launch order.  Activations live in per-block
    // concatenation buffers [B][h][w][C_end] that every layer of the block reads a channel prefix of and appends 32 channels to, so
    // an op carries float offsets and row pitches of its own instead of Acts:
    //   kDnPlace     the pooled stem [M][64] (in_off) into channels [0, 64) of block 1's buffer (out_off, ldo)
    //   kDnPw        a dense layer's norm1 + relu1 + conv1 + norm2 + relu2 (pre = 1: s1 / t1 of p_bn1 over K channels, s2 / t2 of p_bn2,
    //                act 1) from the prefix [0, K) of the buffer (ldi) to the 128-channel bottleneck; or a transition's conv on the pooled
    //                tensor (pre = 0, no affine, act 0) into channels [0, Cout) of the NEXT block's buffer (ldo)
    //   kDnConv3     a dense layer's conv2: the bottleneck [M][128] to channels [c0, c0 + 32) of the buffer (ldo); wt_off: its re-laid image
    //   kDnNormPool  a transition's norm + relu to the stage's skip tensor (out_off, dense, K channels) and its 2 x 2 mean (out2_off);
    //                or norm5 (act 0, no pooled tensor: out2 = 0)
    // One form per shape each: not convolution sites, not tuned, not surveyed, not guarded.
    enum DnKind { kDnPlace, kDnPw, kDnConv3, kDnNormPool };
    struct DnOp {
        DnKind kind; int block;
        int p_w = -1, p_bn1 = -1, p_bn2 = -1;
        int K = 0, Cout = 0, ldi = 0, ldo = 0, c0 = 0, act = 0, out2 = 0;
        size_t s1_off = 0, t1_off = 0, s2_off = 0, t2_off = 0, wt_off = 0;
        size_t in_off = 0, out_off = 0, out2_off = 0;
        int H = 0, W = 0;      // the op's INPUT map
    };
    std::vector<DnOp> dops;
    // features.0 of a VGG encoder (vgg.hip: k_conv3x3_c3): the weight [64][3][3][3] and, without BatchNorm, the bias are read in place;
    // with BatchNorm scale / shift hold the fold, the conv bias folded in behind it.  Not a convolution site: one form, not tuned, not
    // surveyed (its operand is the image).  p_w -1: the plan has none.
    struct VggStem { int p_w = -1, p_bias = -1, p_bn = -1; size_t scale_off = 0, shift_off = 0; } vgg0;
    struct Dec {
        int lat[4];               // p5, p4, p3, p2 (1x1, bias)
        int seg[7];               // s5.0 s5.1 s5.2 s4.0 s4.1 s3.0 s2.0
        int p_gn[7];              // param index of GN weight (bias = +1)
        int p_head_w, p_head_b;
        int head_ch, head_chp;
    } dec[4];

    // activations (float offsets)
    Act a_img4, a_stem, a_pool;   // (a_pool: the ResNet and DenseNet families'; a VGG plan: a_stem / a_pool are block 1's / block 2's outputs, smp's feature levels 1 and 2)
    Act a_feat[4];                // c2 .. c5: the output of each stage's last block
    Act a_p[4][4];                // [decoder][p5,p4,p3,p2]
    Act a_seg[4][7];              // pre-GroupNorm conv outputs
    Act a_up[4][3];               // s5.0 -> up, s5.1 -> up, s4.0 -> up
    size_t gn_part_off[4][7], gn_aff_off[4][7];
    int gn_P[7];
    Act a_low[4];                 // low-res logits
    Act a_lsum[4];                // two-pass merge + head: the head of the three upsampled branches' sum at their own resolution
    int up4_wide = 1;             // 0: FPC_UP4_WIDE=0, plans of 9 to 32 classes keep k_up4_compress<32>
    int merge_split = -1;         // -1: two passes unless FPC_MERGE_SPLIT=0, 0: k_merge_head (one pass), 1: two passes
    size_t splitk_off = 0, splitk_floats = 0;
    size_t se_gate_off = 0, se_part_off = 0;      // SE plans: gate [B][2048] and the slab partials of the stage that needs most (k_se_pool / k_se_excite)
    size_t mb_gate_off = 0, mb_part_off = 0;      // EfficientNet plans: gate [B][widest C] of one block at a time and the slab partials of the block that needs most (k_mb_pool / k_mb_excite)
    int use_graph = 0;            // replay the frame-invariant launches as a HIP graph (fpc_net_set_graph)
    long long wino_blocks = 0;    // workgroups of the form-9 launches of the last forward that launched its kernels (fpc_net_wino_blocks)
    int wino_pack = 1;            // form-9 launches cut their patches out of canvas rows of several frames where that saves patches (fpc_net_set_wino_pack)
    int wino_orient = 1;          // form-9 launches run transposed at the sites wino_orient_rule names (fpc_net_set_wino_orient)
    int wino_xshare = 1;          // packed form-9 launches use the x-shared tile map where wino_xshare_rule offers it (fpc_net_set_wino_xshare)
    int wino_fast_exit = 1;       // workgroups of the four-wave Winograd kernels take the fast exit where their patch lies inside (fpc_net_set_wino_fast_exit)
    int fold_idle_row = 1;        // the wave of the zero transform row only stages in phase 2 of the folded s2.0 (fpc_net_set_fold_idle_row)
    std::vector<char> c_tr;       // 1: the conv is a form-9 candidate at a shape the rule transposes (every decoder's; its h3 image follows wino_orient)
    int split_precision = 0;      // autotuning may pick the bf16 x 3 form of a direct convolution (fpc_net_set_split_precision)
    hipGraphExec_t graph_exec = nullptr;
    size_t zeros_off = 0;         // 64 zero floats (DMA source for out-of-image positions)
    size_t tickets_off = 0;       // kConvTickets zero ints: arrival counters of the fused split-K convolutions

    // the FPN p2 fold of s2.0 (BasicBlock encoders: c2 has 64 channels): per decoder Wc = W L (OIHW), the h3 images of Wc and of W on
    // one scale (wino_h3.hip: launch_wino_pack_h3_pair) and the border-class bias table
    bool h3_packed = false;               // the PackedConv::h3_ok images hold the current weights (split level 3, pack_h3_images)
    hipStream_t load_stream = nullptr;    // stream of the last fpc_net_load_params
    size_t stem_h3_off = 0;               // the stem's k_pack_weight_h3 image (k_stem_pool_h3; packed with the h3_ok images)
    bool fold_ok = false;
    size_t fold_wc_off[4] = {}, fold_img1_off[4] = {}, fold_img2_off[4] = {}, fold_tab_off[4] = {};

    // per-conv launch plans (index = conv id of decoder 0 for grouped ones)
    std::vector<ConvPlan> cplan;
    std::vector<float> tune_score;       // the autotuner's best score per site (ms, or its throughput objective)
    // the activation-range guard (fpc_net_survey_next / fpc_net_guard_ranges)
    unsigned* survey = nullptr;          // device records [convs][4] the NEXT forward fills (k_act_range in front of every site's launch)
    std::vector<ConvPlan> free_plan;     // the autotuner's best-scoring candidate that is not range-limited, kept beside the best ...
    std::vector<char> has_free;          // ... 1 where the site was autotuned and had one
    std::vector<char> guarded;           // 1: the site stands demoted to a range-free plan (sticky: the tuner offers it no fp16-piece form)
    std::vector<int> c_howo, c_groups;   // output pixels per image and launch multiplicity of every planned conv site (0: not a site)

    size_t bump = 0;
    size_t alloc(size_t n) { size_t o = bump; bump += (n + 63) / 64 * 64; return o; }
    Act alloc_act(int h, int w, int c) { Act a; a.H = h; a.W = w; a.C = c; a.off = alloc((size_t)B * h * w * c); return a; }
    int add_param(const std::string& n, int64_t numel) { pnames.push_back(n); pnumel.push_back(numel); return (int)pnames.size() - 1; }
    int add_bn(const std::string& p, int C) {      // BatchNorm's four -> the index of the first
        add_param(p + ".weight", C); add_param(p + ".bias", C); add_param(p + ".running_mean", C);
        return add_param(p + ".running_var", C) - 3;
    }

    // (bias_first: the bias parameter stands in front of the BatchNorm's four — a VGG site's state-dict order; a site with both has the
    // bias folded into its shift at load)
    int add_conv(const std::string& wname, int Cin, int Cout, int k, int stride, int pad, const char* bn_prefix,
                 const char* bias_name, int Cinp = 0, int Kwp = 0, bool bias_first = false) {
        PackedConv c;
        c.Cin = Cin; c.Cinp = Cinp ? Cinp : Cin; c.Cout = Cout; c.Kh = c.Kw = k; c.stride = stride; c.pad = pad;
        c.Kwp = Kwp ? Kwp : k;
        c.K = c.Cinp * k * c.Kwp; c.Kpad = cdiv(c.K, kConvBK) * kConvBK; c.Npad = cdiv(Cout, kConvNAlign) * kConvNAlign;
        c.p_w = add_param(wname, (int64_t)Cout * Cin * k * k);
        if (bias_name && bias_first) c.p_bias = add_param(bias_name, Cout);
        if (bn_prefix) c.p_bn = add_bn(bn_prefix, Cout);
        if (bias_name && !bias_first) c.p_bias = add_param(bias_name, Cout);
        c.w_off = alloc(conv_packed_floats(c.Npad, c.Kpad));      // f32 image + its three bf16 planes
        if (bn_prefix) { c.scale_off = alloc(Cout); c.shift_off = alloc(Cout); }
        c.wino_ok = (k == 3 && stride == 1 && pad == 1 && c.Cinp == Cin && Cin % 8 == 0 && Cout % 64 == 0);
        if (c.wino_ok) c.wino_off = alloc(wino_region_floats(kImgH3, Cout, Cin, Cout % 128 == 0));      // every image (kWinoImages)
        convs.push_back(c);
        return (int)convs.size() - 1;
    }
    // a grouped 3x3 / pad-1 site of C channels in groups of cg, with BatchNorm: its packed image is k_pack_grouped's alone
    int add_grouped_conv(const std::string& wname, int C, int cg, int stride, const char* bn_prefix) {
        PackedConv c;
        c.Cin = c.Cinp = c.Cout = C; c.Kh = c.Kw = c.Kwp = 3; c.stride = stride; c.pad = 1; c.cg = cg;
        c.K = cg * 9; c.Kpad = cdiv(c.K, kConvBK) * kConvBK; c.Npad = cdiv(C, kConvNAlign) * kConvNAlign;
        c.p_w = add_param(wname, (int64_t)C * cg * 9);
        c.p_bn = add_bn(bn_prefix, C);
        c.grp_off = alloc((size_t)C * cg * 9);
        c.scale_off = alloc(C); c.shift_off = alloc(C);
        convs.push_back(c);
        return (int)convs.size() - 1;
    }
};

// the implicit GEMM's loader of a lateral site: 0 = the fast one (Cin a multiple of 32), 2 = Cin % 4 (k_conv_igemm's MODE 2)
inline int lateral_mode(const PackedConv& c) { return c.Cin % kConvBK == 0 ? 0 : 2; }
