"""SHA-256 of what the kernels that run in the XCD-banded workgroup order write (csrc/conv_device.hpp: xcd_logical, xcd_span), through
the C entries that reach them, every output buffer pre-filled with NaN (the class mask of a network with -1), the operands drawn on
the CPU from a seed the case's name alone fixes.  Written on the commit BEFORE the order's hand copies became calls of the one helper
(tests/golden/xcd_order_digests.json); tests/test_gpu_xcd_order.py compares the change against it.
    python tools_dev/xcd_order_digest.py > tests/golden/xcd_order_digests.json
Per kernel instance three launches, chosen from its launcher's tile constants so that the workgroup count is (a) below 8: the plain
order; (b) a multiple of 8: the banded order; (c) at least 9 and no multiple of 8: where the launcher rounds the grid up, the ids past
the list must leave without writing; where it launches its exact count (the lateral and pointwise GEMMs, the split dense 3x3, the VGG
weight gradient, the 7x7 stem), the plain order at an odd count.  The grouped 3x3 launchers round every grid up to a multiple of 8, so
their (a) is a list shorter than the grid of 8.  The comment behind each case gives its workgroups.  The 32 x 32 forms of the f32 1x1
exist only from 1024 waves on (2048 for more than one channel tile a wave): they have no (a).  k_stem_pool_h3 and the x4 upsample
kernels are reached only through a network: two forwards of ResNet-18 at 96 x 128, the smallest image the fused stem takes, at 7
classes (k_up4_compress7x4) and at 10 (k_up4_compress_wide), batch 1 and batch 2."""
import ctypes
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch


def cases():
    """(name, kind, parameters) in a fixed order"""
    out = []

    def add(kind, tag, *p):
        out.append(("%s-%s" % (kind, tag), kind, p))

    # fpc_conv1x1_f32 / fpc_mbconv_pw (mobilenet.hip: k_conv1x1_f32_small, k_conv1x1_f32<NT, U>), (M, Cin, Cout): 16 x 16 tiles, 4 a workgroup
    for kind in ("pw", "mbpw"):
        for tag, M, Cin, Cout in (("small-a", 40, 16, 16),           # 3 tiles: 1
                                  ("small-b", 128, 16, 64),          # 32 tiles: 8
                                  ("small-c", 144, 16, 64),          # 36 tiles: 9 -> 16
                                  ("nt1-b", 4096, 16, 256),          # 32 x 32 tiles, 1024 waves: 256
                                  ("nt1-c", 4128, 16, 256),          # 1032 waves: 258 -> 264
                                  ("nt2-b", 65536, 8, 64),           # 2048 waves of two channel tiles: 512
                                  ("nt2-c", 65568, 8, 64),           # 2049 waves: 513 -> 520
                                  ("nt3-c", 65568, 8, 96),
                                  ("nt5-c", 65568, 8, 160)):
            add(kind, tag, M, Cin, Cout)
    # fpc_maxpool2x2_fwd / _bwd (vgg.hip, vgg_train.hip), (B, H, W, C): 256 channel quads of pooled pixels a workgroup
    for kind in ("pool2", "pool2bwd"):
        for tag, shape in (("a", (1, 2, 2, 4)), ("b", (1, 64, 128, 4)), ("c", (1, 66, 128, 4))):      # 1, 8, 9 -> 16
            add(kind, tag, *shape)
    # fpc_conv3x3_c3_wgrad (k_c3_wgrad), (B, H, W): a workgroup per slice, fpc_conv3x3_c3_wgrad_slices = 3, 8, 11
    for tag, shape in (("a", (1, 24, 8)), ("b", (1, 64, 8)), ("c", (2, 44, 8))):
        add("c3wgrad", tag, *shape)
    # fpc_stem3x3s2 / fpc_mbconv_stem (k_stem3x3s2<MB>), (B, Hi, Wi): 256 output pixels a workgroup
    for kind in ("stem3", "mbstem"):
        for tag, shape in (("a", (1, 6, 10)), ("b", (1, 64, 128)), ("c", (1, 66, 128))):              # 1, 8, 9 -> 16
            add(kind, tag, *shape)
    # fpc_conv3x3_c3 (k_conv3x3_c3<AFF>), (B, H, W, scale given): 256 pixel pairs a workgroup
    for aff in (0, 1):
        for tag, shape in (("a", (1, 5, 7)), ("b", (1, 32, 128)), ("c", (1, 33, 128))):               # 1, 8, 9 -> 16
            add("c3", "aff%d-%s" % (aff, tag), *shape, aff)
    # fpc_dense_pw (k_dense_pw32<PRE>: four 32 x 32 tiles a workgroup; k_dense_pw16<PRE>: a 16 x 16 tile each), (M, K, Cout, form, pre)
    for pre in (0, 1):
        for tag, M, Cout, form in (("f1-a", 40, 32, 1), ("f1-b", 128, 256, 1), ("f1-c", 144, 256, 1),      # 1, 8, 10 -> 16
                                   ("f0-a", 40, 32, 0), ("f0-b", 64, 32, 0), ("f0-c", 72, 32, 0)):         # 6, 8, 10 -> 16
            add("densepw", "pre%d-%s" % (pre, tag), M, 64, Cout, form, pre)
    # fpc_dense_conv3x3 (k_dense_conv3_tile: 256 pixels a workgroup; k_dense_conv3_split: 16, exact), (B, H, W, form)
    for tag, shape in (("f1-a", (1, 5, 7, 1)), ("f1-b", (1, 32, 64, 1)), ("f1-c", (1, 33, 64, 1)),         # 1, 8, 9 -> 16
                       ("f0-a", (1, 5, 7, 0)), ("f0-b", (1, 8, 16, 0)), ("f0-c", (1, 9, 16, 0))):          # 3, 8, 9
        add("densec3", tag, *shape)
    # fpc_dwconv3x3_wgrad (k_dw_wgrad<3, S, 1>), (B, Hi, Wi, C, stride): 32 channels, a workgroup per slice
    for tag, shape in (("s1-a", (1, 8, 96, 32, 1)), ("s1-b", (1, 8, 256, 32, 1)), ("s1-c", (1, 16, 160, 32, 1)),      # 3, 8, 10 -> 16
                       ("s2-a", (1, 16, 192, 32, 2)), ("s2-b", (1, 16, 512, 32, 2)), ("s2-c", (1, 32, 320, 32, 2))):
        add("dwwgrad", tag, *shape)
    # fpc_conv2d_grouped (k_conv3x3_grouped<CG, S>: 8 x 16 output pixels x 32 channels at stride 1, 8 x 8 at stride 2), (B, Hi, Wi, C, groups, stride)
    for cg in (4, 8, 16, 32, 64):
        C = 64 if cg == 64 else 32
        for s, shapes in ((1, ((8, 48), (8, 128), (9, 80))), (2, ((16, 48), (16, 128), (17, 79)))):      # 3 -> 8, 8, 10 -> 16 (C = 64: twice)
            for tag, (H, W) in zip("abc", shapes):
                add("grp", "cg%d-s%d-%s" % (cg, s, tag), 1, H, W, C, C // cg, s)
    # fpc_conv2d_grouped_dgrad: stride 1 runs k_conv3x3_grouped<CG, 1> over dy; stride 2 k_conv3x3_grouped_dgrad_s2<CG>, 16 x 32 pixels of dx
    for tag, (H, W) in zip("abc", ((8, 48), (8, 128), (9, 80))):
        add("grpdgrad", "cg8-s1-%s" % tag, 1, H, W, 32, 4, 1)
    for cg in (4, 8, 16, 32, 64):
        C = 64 if cg == 64 else 32
        for tag, (H, W) in zip("abc", ((16, 96), (16, 256), (17, 160))):                                  # 3 -> 8, 8, 10 -> 16 (C = 64: twice)
            add("grpdgrad", "cg%d-s2-%s" % (cg, tag), 1, H, W, C, C // cg, 2)
    # fpc_conv2d_grouped_wgrad (its kernels keep the launch order: held as the rest of the family's entries)
    for s, (H, W) in ((1, (9, 80)), (2, (17, 79))):
        add("grpwgrad", "cg8-s%d" % s, 2, H, W, 32, 4, s)
    # fpc_conv2d on 2001 / 7001 (k_lateral1x1<KG, UP, H3>: 128 pixels a workgroup, exact), (B, Cin, H, W, Cout, k, stride, pad, code, up)
    for code in (2001, 7001):
        for cin in (64, 128):
            for up in (0, 1):
                for tag, (B, H, W) in zip("abc", ((3, 6, 8), (1, 32, 32), (1, 36, 32))):                 # 3, 8, 9
                    add("conv2d", "%d-k%d-up%d-%s" % (code, cin, up, tag), B, cin, H, W, 32, 1, 1, 0, code, up)
    # ... 3000 (k_stem7x7: 8 row segments of 64 outputs a workgroup, exact up to 256)
    for tag, Hi in zip("abcd", (48, 122, 144, 250)):                                                      # 24, 61, 72, 125 segments: 3, 8, 9, 16
        add("conv2d", "3000-%s" % tag, 1, 4, Hi, 128, 64, 7, 2, 3, 3000, 0)
    # ... 4000 / 4001 (k_conv1x1<WM>: 64 / 128 pixels x 64 channels a workgroup, exact)
    for v, bm in ((0, 64), (1, 128)):
        for tag, rows in zip("abc", (3, 8, 9)):
            add("conv2d", "%d-%s" % (4000 + v, tag), 1, 64, rows * bm // 32, 32, 64, 1, 1, 0, 4000 + v, 0)
    # fpc_net_forward: (classes, B) at 96 x 128, the stem on k_stem_pool_h3
    for classes in (7, 10):
        for B in (1, 2):
            add("net", "c%d-b%d" % (classes, B), classes, B)
    return out


def _gen(name):
    return torch.Generator().manual_seed(int(hashlib.sha256(name.encode()).hexdigest()[:12], 16))


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


@functools.lru_cache(maxsize=None)
def _model(classes):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    hp = config.INFERENCE()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet18"
    hp.PERFORM_AGGREGATION = False
    hp.ENGINE_AUTOTUNE = False
    hp.SELECTED_CLASSES = ["bg"] + ["obj%d" % i for i in range(1, classes)]
    torch.manual_seed(classes)
    m = L.pose_regressor.MODELS['PoseRegressor'].load_from_ckpt(None, hp)
    g = torch.Generator().manual_seed(classes + 1)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
            mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    assert m.classes == classes
    return m.eval().to(torch.device("cuda:0"))


def _run_net(dev, nat, L, name, classes, B):
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    H, W, G = 96, 128, classes - 1
    eng = NetEngine(_model(classes), B, H, W, dev, autotune=False, split_precision=3)
    assert eng.force_stem_pool(1) == 1, name
    x = torch.stack([synth.make_image(i, H, W) for i in range(B)]).to(dev).contiguous()
    logits = [_nan(dev, B, c, H, W) for c in (classes, 4 * G, 3 * G, 2 * G, G)]
    mask = torch.full((B, H, W), -1, dtype=torch.int64, device=dev)
    cat = [_nan(dev, B, 4, H, W), _nan(dev, B, 3, H, W), _nan(dev, B, 2, H, W), _nan(dev, B, H, W)]
    rc = L.fpc_net_forward(eng._h, x.data_ptr(), *[t.data_ptr() for t in logits], mask.data_ptr(), *[t.data_ptr() for t in cat], nat.stream())
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return logits + [mask] + cat


def run_case(dev, case):
    """the tensors the case's entry writes, on the CPU; unwritten elements stay NaN (-1 in a network's class mask)"""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    name, kind, p = case
    g = _gen(name)
    rn = lambda *s: torch.randn(s, generator=g)
    st = nat.stream()
    if kind in ("pw", "mbpw"):
        M, Cin, Cout = p
        x, w = rn(M, Cin).to(dev), (rn(Cout, Cin) / Cin ** 0.5).to(dev)
        scale, shift, res = (torch.rand(Cout, generator=g) + 0.5).to(dev), rn(Cout).to(dev), rn(M, Cout).to(dev)
        outs = [_nan(dev, M, Cout)]
        if kind == "pw":
            rc = L.fpc_conv1x1_f32(x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), res.data_ptr(), outs[0].data_ptr(), M, Cin, Cout, 0, st)
        else:      # two frames, a gate row each, swish
            gate = torch.rand(2, Cin, generator=g).to(dev)
            rc = L.fpc_mbconv_pw(x.data_ptr(), gate.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), None, outs[0].data_ptr(), 2, M // 2, Cin,
                                 Cout, 2, st)
    elif kind in ("pool2", "pool2bwd"):
        B, H, W, C = p
        x = rn(B, H, W, C).to(dev)
        if kind == "pool2":
            outs = [_nan(dev, B, H // 2, W // 2, C)]
            rc = L.fpc_maxpool2x2_fwd(x.data_ptr(), outs[0].data_ptr(), B, H, W, C, st)
        else:
            dy = rn(B, H // 2, W // 2, C).to(dev)
            outs = [_nan(dev, B, H, W, C)]
            rc = L.fpc_maxpool2x2_bwd(x.data_ptr(), dy.data_ptr(), outs[0].data_ptr(), B, H, W, C, st)
    elif kind == "c3wgrad":
        B, H, W = p
        img, dy = rn(B, H, W, 4).to(dev), rn(B, H, W, 64).to(dev)
        need = L.fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W)
        ws = _nan(dev, need // 4 + 64)
        outs = [_nan(dev, 64 * 27), _nan(dev, 64)]
        rc = L.fpc_conv3x3_c3_wgrad(img.data_ptr(), dy.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), B, H, W, ws.data_ptr(), need, st)
    elif kind in ("stem3", "mbstem"):
        B, Hi, Wi = p
        Ho, Wo = ((Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1) if kind == "stem3" else (Hi // 2, Wi // 2)
        x, w = rn(B, Hi, Wi, 4).to(dev), (rn(32, 3, 3, 3) / 5).to(dev)
        scale, shift = (torch.rand(32, generator=g) + 0.5).to(dev), rn(32).to(dev)
        outs = [_nan(dev, B, Ho, Wo, 32)]
        fn = L.fpc_stem3x3s2 if kind == "stem3" else L.fpc_mbconv_stem
        rc = fn(x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), outs[0].data_ptr(), B, Hi, Wi, 32, st)
    elif kind == "c3":
        B, H, W, aff = p
        x, w = rn(B, H, W, 4).to(dev), (rn(64, 3, 3, 3) / 5).to(dev)
        scale, shift = (torch.rand(64, generator=g) + 0.5).to(dev), rn(64).to(dev)
        outs = [_nan(dev, B, H, W, 64)]
        rc = L.fpc_conv3x3_c3(x.data_ptr(), w.data_ptr(), scale.data_ptr() if aff else None, shift.data_ptr(), outs[0].data_ptr(), B, H, W, 64, 1, st)
    elif kind == "densepw":
        M, K, Cout, form, pre = p
        x, w = rn(M, K).to(dev), (rn(Cout, K) / K ** 0.5).to(dev)
        s1, t1 = (torch.rand(K, generator=g) + 0.5).to(dev), rn(K).to(dev)
        s2, t2 = (torch.rand(Cout, generator=g) + 0.5).to(dev), rn(Cout).to(dev)
        outs = [_nan(dev, M, Cout)]
        rc = L.fpc_dense_pw(x.data_ptr(), s1.data_ptr() if pre else None, t1.data_ptr() if pre else None, w.data_ptr(), s2.data_ptr(), t2.data_ptr(),
                            outs[0].data_ptr(), M, K, Cout, K, Cout, 1, form, st)
    elif kind == "densec3":
        B, H, W, form = p
        x, w = rn(B, H, W, 128).to(dev), (rn(32, 128, 3, 3) / 34).to(dev)
        wt = _nan(dev, 9 * 32 * 128)
        rc = L.fpc_dense_conv3x3_pack(w.data_ptr(), wt.data_ptr(), st)
        assert rc == 0, (name, "pack", rc)
        outs = [_nan(dev, B, H, W, 32)]
        rc = L.fpc_dense_conv3x3(x.data_ptr(), wt.data_ptr(), outs[0].data_ptr(), B, H, W, 0, 32, form, st)
    elif kind == "dwwgrad":
        B, Hi, Wi, C, s = p
        Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
        x, dy = rn(B, Hi, Wi, C).to(dev), rn(B, Ho, Wo, C).to(dev)
        need = L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)
        ws = _nan(dev, need // 4 + 64)
        outs = [_nan(dev, C * 9)]
        rc = L.fpc_dwconv3x3_wgrad(x.data_ptr(), dy.data_ptr(), outs[0].data_ptr(), B, Hi, Wi, C, s, ws.data_ptr(), need, st)
    elif kind in ("grp", "grpdgrad", "grpwgrad"):
        B, Hi, Wi, C, groups, s = p
        cg = C // groups
        Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
        x, dy, w = rn(B, Hi, Wi, C).to(dev), rn(B, Ho, Wo, C).to(dev), (rn(C, cg, 3, 3) / (3 * cg ** 0.5)).to(dev)
        if kind == "grp":
            scale, shift = (torch.rand(C, generator=g) + 0.5).to(dev), rn(C).to(dev)
            need = L.fpc_conv2d_grouped_workspace_bytes(C, groups)
            ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            outs = [_nan(dev, B, Ho, Wo, C)]
            rc = L.fpc_conv2d_grouped(x.data_ptr(), Hi * Wi * C, Wi * C, C, 1, w.data_ptr(), scale.data_ptr(), shift.data_ptr(), outs[0].data_ptr(), B, Hi, Wi,
                                      C, groups, s, 1, 0, ws.data_ptr(), need, st)
        elif kind == "grpdgrad":
            need = L.fpc_conv2d_grouped_dgrad_workspace_bytes(C, groups)
            ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            outs = [_nan(dev, B, Hi, Wi, C)]
            rc = L.fpc_conv2d_grouped_dgrad(dy.data_ptr(), w.data_ptr(), outs[0].data_ptr(), B, Hi, Wi, C, groups, s, ws.data_ptr(), need, st)
        else:
            need = L.fpc_conv2d_grouped_wgrad_workspace_bytes(B, Ho, Wo, C, groups)
            ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
            outs = [_nan(dev, C, cg, 3, 3)]
            rc = L.fpc_conv2d_grouped_wgrad(x.data_ptr(), Hi * Wi * C, Wi * C, C, dy.data_ptr(), outs[0].data_ptr(), B, Hi, Wi, C, groups, s, ws.data_ptr(),
                                            need, st)
        assert ws.data_ptr() % 256 == 0
    elif kind == "conv2d":
        B, Cin, Hi, Wi, Cout, k, s, pad, code, up = p
        Ho, Wo = (Hi + 2 * pad - k) // s + 1, (Wi + 2 * pad - k) // s + 1
        x, w = rn(B, Hi, Wi, Cin), rn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
        if code == 3000:
            x[..., 3] = 0.0      # the NHWC4 image
        x, w = x.to(dev), w.to(dev)
        scale = (torch.rand(Cout, generator=g) + 0.5).to(dev) if code in (3000, 4000, 4001) else None
        shift = rn(Cout).to(dev)
        upt = rn(B, Ho // 2, Wo // 2, Cout).to(dev) if up else None
        ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, Ho, Wo, Cin, Cout, k, k), dtype=torch.uint8, device=dev)
        outs = [_nan(dev, B, Ho, Wo, Cout)]
        sb, sh, sw, sc = x.stride()
        rc = L.fpc_conv2d(x.data_ptr(), sb, sh, sw, sc, w.data_ptr(), nat.ptr(scale), shift.data_ptr(), None, nat.ptr(upt), outs[0].data_ptr(), None, B, Hi,
                          Wi, Cin, Cout, k, k, s, pad, int(code == 3000), 0, 0, code, ws.data_ptr(), ws.numel(), st)
    elif kind == "net":
        return [t.cpu() for t in _run_net(dev, nat, L, name, *p)]
    else:
        raise ValueError(kind)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return [t.cpu() for t in outs]


def unwritten(outs):
    """elements no kernel wrote"""
    return sum(int((t == -1).sum() if t.dtype == torch.int64 else torch.isnan(t).sum()) for t in outs)


def digest(outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    dev = torch.device("cuda:0")
    d = {}
    for case in cases():
        outs = run_case(dev, case)
        assert unwritten(outs) == 0, (case[0], "unwritten outputs")
        d[case[0]] = digest(outs)
    json.dump(d, sys.stdout, indent=0, sort_keys=True)
    print()


if __name__ == "__main__":
    main()
