#!/usr/bin/env python3
"""Record what the training front end (fastposecnn_amd/lib/train_conv.py) accepts, refuses and counts into
tests/golden/train_gate_contract.json.

Every front end — conv2d (dense, grouped, the stem), conv2d_up_add, maxpool3x3s2, upsample_bilinear, groupnorm_relu, batchnorm_act,
se_gate_add_relu — gets one accepted case at the smallest legal shape (B = 2, 8 x 8 maps, 64 channels, 16 groups of 4; the stem at
2 x 3 x 16 x 16), then one case per term of its gate with exactly ONE operand changed; the three weight-gradient families (dense,
grouped, stem) get the GradSink cases on top.  Per case: whether the front end returned None (or what it raised — a refused float64
operand reaches torch's own convolution beside f32 weights), the result's grad_fn type, shape and memory format, the non-zero
`counters` deltas after the forward and after y.sum().backward(), and for a sink case what became of the sink.  No value of a
result is recorded: this is the record of WHICH path an input takes, the kernels' numbers have their own tests.
`_plan_cache` is pinned to code 0 (no candidate is timed), every switch is on unless the case turns it off.
Left out: the terms that need a second GPU (a tensor off the current device, a parameter on another device) and the numel bounds
of the stem, the pool, BatchNorm and the SE gate, which only a tensor of 8 GiB or more can reach.
tests/test_gpu_train_gate_contract.py calls collect() on the front end under test and compares it with the file, value for value.

The file was recorded on an MI355X from the front end of commit 953ef84 ("State each encoder block kind once; split the planner
out of net.hip"), the last one that wrote every gate, sink and gradient entry out in full.  It is a record of behaviour: it is
regenerated only by a change that MEANS to change what a gate accepts or what a path counts, never by a refactoring.
    python tests/golden/make_train_gate_contract.py
"""
import contextlib
import json
import os
import sys

import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "train_gate_contract.json")

SWITCHES = {"ENABLED": True, "SPLIT_PRECISION": True, "SPLIT_F16": True, "NATIVE_GROUPED": True, "NATIVE_STEM": True,
            "NATIVE_BN": True, "NATIVE_SE": True}
F64, NCHW, OFFSET, NO_GRAD_X = {"dtype": torch.float64}, {"layout": "nchw"}, {"offset": True}, {"grad": False}
SINKS = ("good", "written", "shape", "strided", "offset", "dead")


class Pinned(dict):
    def get(self, key, default=None):      # conv_nhwc asks with .get(key): no candidate is timed, none is remembered
        return 0


class Owner:
    pass


def tensor(dev, shape, seed, dtype=torch.float32, layout="nhwc", offset=False, grad=True, scale=1.0):
    """randn of `shape` on dev: channel-last (4-D) or contiguous; offset: a view one float into a larger buffer (4 bytes off 16)"""
    v = (torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).to(dtype)
    nhwc = layout == "nhwc" and len(shape) == 4
    if offset:
        flat = torch.zeros(v.numel() + 4, dtype=dtype, device=dev)[1:1 + v.numel()]
        t = flat.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2) if nhwc else flat.view(shape)
        t.copy_(v)
    else:
        t = v.to(dev).contiguous(memory_format=torch.channels_last) if nhwc else v.to(dev)
    return t.requires_grad_(grad)


def param(dev, shape, seed, **kw):
    return tensor(dev, shape, seed, layout="nchw", scale=0.1, **kw)


def register_sink(tc, dev, w, kind):
    """-> (sink, fired, owner): a GradSink for w whose view is good / of another shape / strided / 4 bytes off, already written, or
    whose owner is gone"""
    shape = tuple(w.shape)
    if kind == "shape":
        view = torch.zeros(shape[:-1] + (shape[-1] + 1,), device=dev)
    elif kind == "strided":
        view = torch.zeros(shape[:-1] + (2 * shape[-1],), device=dev)[..., ::2]
    elif kind == "offset":
        view = torch.zeros(w.numel() + 4, device=dev)[1:1 + w.numel()].view(shape)
    else:
        view = torch.zeros(shape, device=dev)
    fired, owner = [], Owner()
    sink = tc.GradSink(view, lambda: fired.append(1), owner)
    sink.written = kind == "written"
    tc.grad_sinks[w.data_ptr()] = sink
    return sink, fired, (None if kind == "dead" else owner)


# ---- the families: spec -> (call, named leaves, weight that may have a sink) --------------------------------------------------------

def f_dense(tc, dev, s):
    cin, cout, (kh, kw) = s.get("cin", 32), s.get("cout", 64), s.get("k", (3, 3))
    x = tensor(dev, (2, cin, 8, 8), 1, **s.get("x", {}))
    w = param(dev, (cout, cin, kh, kw), 2)
    b = param(dev, (cout,), 3) if s.get("bias") else None
    return (lambda: tc.conv2d(x, w, b, s.get("stride", 1), s.get("pad", kh // 2))), {"x": x, "w": w, "b": b}, w


def f_grouped(tc, dev, s):
    C, groups = s.get("C", 64), s.get("groups", 16)
    x = tensor(dev, s.get("xshape", (2, C, 8, 8)), 1, **s.get("x", {}))
    w = param(dev, s.get("wshape", (C, C // max(groups, 1), 3, 3)), 2, **s.get("w", {}))
    b = None
    if s.get("bias"):
        b = param(dev, (2 * C,), 3)[::2] if s["bias"] == "strided" else param(dev, (C,), 3, **s["bias"])
    return (lambda: tc.conv2d(x, w, b, s.get("stride", 1), s.get("pad", 1), groups)), {"x": x, "w": w, "b": b}, w


def f_stem(tc, dev, s):
    x = tensor(dev, s.get("xshape", (2, 3, 16, 16)), 1, **dict({"layout": "nchw", "grad": False}, **s.get("x", {})))
    w = param(dev, s.get("wshape", (64, 3, 7, 7)), 2, **s.get("w", {}))
    b = param(dev, (64,), 3) if s.get("bias") else None
    return (lambda: tc.conv2d(x, w, b, s.get("stride", 2), s.get("pad", 3))), {"x": x, "w": w, "b": b}, w


def f_up_add(tc, dev, s):
    cin, cout, (kh, kw) = s.get("cin", 64), s.get("cout", 64), s.get("k", (1, 1))
    x = tensor(dev, s.get("xshape", (2, cin, 8, 8)), 1, **s.get("x", {}))
    w = param(dev, (cout, cin, kh, kw), 2)
    b = param(dev, (cout,), 3)
    top = tensor(dev, s.get("topshape", (2, cout, 4, 4)), 4, **s.get("top", {}))
    return (lambda: tc.conv2d_up_add(x, w, b, top, 0)), {"x": x, "w": w, "b": b, "top": top}, None


def f_pool(tc, dev, s):
    x = tensor(dev, s.get("xshape", (2, 64, 8, 8)), 1, **s.get("x", {}))
    return (lambda: tc.maxpool3x3s2(x)), {"x": x}, None


def f_upsample(tc, dev, s):
    x = tensor(dev, s.get("xshape", (2, 64, 8, 8)), 1, **s.get("x", {}))
    xin = x.flip(3) if s.get("flip") else x
    return (lambda: tc.upsample_bilinear(xin, s.get("scale", 2), s.get("out_nchw", False))), {"x": x}, None


def f_groupnorm(tc, dev, s):
    C, G = s.get("C", 128), s.get("G", 32)
    x = tensor(dev, s.get("xshape", (2, C, 8, 8)), 1, **s.get("x", {}))
    gn = nn.GroupNorm(G, C, affine=s.get("affine", True)).to(dev)
    return (lambda: tc.groupnorm_relu(x, gn)), {"x": x, "gamma": gn.weight, "beta": gn.bias}, None


def f_batchnorm(tc, dev, s):
    x = tensor(dev, s.get("xshape", (2, 64, 8, 8)), 1, **s.get("x", {}))
    bn = nn.BatchNorm2d(s.get("features", x.shape[1] if x.dim() == 4 else 64), **s.get("bn", {})).to(dev)
    if s.get("double"):
        bn.double()
    if s.get("eval"):
        bn.eval()
    if s.get("weight_offset"):
        bn.weight = nn.Parameter(torch.ones(68, device=dev)[1:65])
    res = tensor(dev, s.get("resshape", (2, 64, 8, 8)), 5, **s["res"]) if "res" in s else None
    call = lambda: tc.batchnorm_act(x, bn, res, **s.get("kw", {}))
    return call, {"x": x, "res": res, "gamma": bn.weight, "beta": bn.bias}, None


def f_se(tc, dev, s):
    from fastposecnn_amd.lib import backbone as bb
    C = s.get("C", 64)
    x = tensor(dev, s.get("xshape", (2, C, 8, 8)), 1, **s.get("x", {}))
    res = tensor(dev, s.get("resshape", s.get("xshape", (2, C, 8, 8))), 5, **s.get("res", {}))
    torch.manual_seed(6)
    se = bb.SEModule(C, 16)
    for name, make in s.get("swap", {}).items():
        setattr(se, name, make(C))
    se = se.to(dev)
    if s.get("double"):
        se.double()
    if s.get("weight_offset"):
        se.fc1.weight = nn.Parameter(torch.zeros(se.fc1.weight.numel() + 4, device=dev)[1:1 + se.fc1.weight.numel()].view(se.fc1.weight.shape))
    act = s["act"]() if "act" in s else None
    leaves = {"x": x, "res": res}
    leaves.update({n.replace(".", "_"): p for n, p in se.named_parameters()})
    return (lambda: tc.se_gate_add_relu(x, se, res, act)), leaves, None


FAMILIES = {"dense": f_dense, "grouped": f_grouped, "stem": f_stem, "up_add": f_up_add, "pool": f_pool, "upsample": f_upsample,
            "groupnorm": f_groupnorm, "batchnorm": f_batchnorm, "se": f_se}


def _off(name):
    return {"patch": {name: False}}


def cases():
    """[(case name, family, spec)]: per family the accepted case(s) first, then one changed operand per case"""
    c = []
    dense64 = {"cin": 64, "cout": 64}
    c += [("dense 32->64 3x3", "dense", {}), ("dense 32->64 1x1", "dense", {"k": (1, 1)}),
          ("dense 32->64 3x3 stride 2", "dense", {"stride": 2}), ("dense 32->64 1x1 stride 2", "dense", {"k": (1, 1), "stride": 2}),
          ("dense 64->64 3x3", "dense", dense64), ("dense 64->64 3x3 with bias", "dense", dict(dense64, bias=True)),
          ("dense 64->7 1x1 head with bias", "dense", {"cin": 64, "cout": 7, "k": (1, 1), "bias": True}),
          ("dense ENABLED off", "dense", _off("ENABLED")), ("dense no_grad", "dense", {"no_grad": True}),
          ("dense x without grad", "dense", {"x": NO_GRAD_X}), ("dense float64 x", "dense", {"x": F64}), ("dense NCHW x", "dense", {"x": NCHW}),
          ("dense Cin 16", "dense", {"cin": 16}), ("dense 3x1 kernel", "dense", {"k": (3, 1), "pad": 0})]
    c += [("dense sink %s" % k, "dense", dict(dense64, sink=k)) for k in SINKS]
    c += [("dense sink on the padded 7-channel head", "dense", {"cin": 64, "cout": 7, "k": (1, 1), "bias": True, "sink": "good"})]

    c += [("grouped", "grouped", {}), ("grouped stride 2", "grouped", {"stride": 2}), ("grouped with bias", "grouped", {"bias": {}}),
          ("grouped switch off", "grouped", _off("NATIVE_GROUPED")), ("grouped ENABLED off", "grouped", _off("ENABLED")),
          ("grouped no_grad", "grouped", {"no_grad": True}), ("grouped x without grad", "grouped", {"x": NO_GRAD_X}),
          ("grouped float64 x", "grouped", {"x": F64}), ("grouped NCHW x", "grouped", {"x": NCHW}),
          ("grouped offset x", "grouped", {"x": OFFSET}), ("grouped 3-D x", "grouped", {"xshape": (64, 8, 8)}),
          ("grouped float64 w", "grouped", {"w": F64}), ("grouped float64 bias", "grouped", {"bias": F64}),
          ("grouped strided bias", "grouped", {"bias": "strided"}), ("grouped offset bias", "grouped", {"bias": OFFSET}),
          ("grouped groups 0", "grouped", {"groups": 0}), ("grouped C 48", "grouped", {"C": 48, "groups": 12}),
          ("grouped groups 3", "grouped", {"groups": 3}), ("grouped 2 channels per group", "grouped", {"groups": 32}),
          ("grouped 1x1 kernel", "grouped", {"wshape": (64, 4, 1, 1)}), ("grouped Cout 128", "grouped", {"wshape": (128, 4, 3, 3)}),
          ("grouped pad 0", "grouped", {"pad": 0}), ("grouped stride 3", "grouped", {"stride": 3}),
          ("grouped empty batch", "grouped", {"xshape": (0, 64, 8, 8)})]
    c += [("grouped sink %s" % k, "grouped", {"sink": k}) for k in SINKS]

    c += [("stem", "stem", {}), ("stem switch off", "stem", _off("NATIVE_STEM")), ("stem ENABLED off", "stem", _off("ENABLED")),
          ("stem no_grad", "stem", {"no_grad": True}), ("stem x with grad", "stem", {"x": {"grad": True}}),
          ("stem w without grad", "stem", {"w": NO_GRAD_X}), ("stem float64 x", "stem", {"x": F64}),
          ("stem NHWC x", "stem", {"x": {"layout": "nhwc"}}),
          ("stem offset x", "stem", {"x": OFFSET}), ("stem 3-D x", "stem", {"xshape": (3, 16, 16)}), ("stem float64 w", "stem", {"w": F64}),
          ("stem 5x5 kernel", "stem", {"wshape": (64, 3, 5, 5)}), ("stem stride 1", "stem", {"stride": 1}), ("stem pad 2", "stem", {"pad": 2}),
          ("stem with bias", "stem", {"bias": True}), ("stem 4 channels", "stem", {"xshape": (2, 4, 16, 16)}),
          ("stem empty batch", "stem", {"xshape": (0, 3, 16, 16)}), ("stem H 6", "stem", {"xshape": (2, 3, 6, 16)}),
          ("stem W 6", "stem", {"xshape": (2, 3, 16, 6)}), ("stem H 15", "stem", {"xshape": (2, 3, 15, 16)}),
          ("stem W 15", "stem", {"xshape": (2, 3, 16, 15)})]
    c += [("stem sink %s" % k, "stem", {"sink": k}) for k in SINKS]

    c += [("up_add", "up_add", {}), ("up_add ENABLED off", "up_add", _off("ENABLED")), ("up_add no_grad", "up_add", {"no_grad": True}),
          ("up_add float64 x", "up_add", {"x": F64}), ("up_add float64 top", "up_add", {"top": F64}), ("up_add NCHW x", "up_add", {"x": NCHW}),
          ("up_add NCHW top", "up_add", {"top": NCHW}), ("up_add Cin 16", "up_add", {"cin": 16}), ("up_add 1x3 kernel", "up_add", {"k": (1, 3)}),
          ("up_add Cout 6", "up_add", {"cout": 6}), ("up_add H 7", "up_add", {"xshape": (2, 64, 7, 8)}),
          ("up_add W 7", "up_add", {"xshape": (2, 64, 8, 7)}), ("up_add top of another shape", "up_add", {"topshape": (2, 64, 4, 5)})]

    c += [("pool", "pool", {}), ("pool switch off", "pool", _off("NATIVE_STEM")), ("pool ENABLED off", "pool", _off("ENABLED")),
          ("pool no_grad", "pool", {"no_grad": True}), ("pool x without grad", "pool", {"x": NO_GRAD_X}), ("pool float64", "pool", {"x": F64}),
          ("pool NCHW", "pool", {"x": NCHW}), ("pool offset", "pool", {"x": OFFSET}), ("pool 3-D", "pool", {"xshape": (64, 8, 8)}),
          ("pool C 6", "pool", {"xshape": (2, 6, 8, 8)}), ("pool empty batch", "pool", {"xshape": (0, 64, 8, 8)})]

    c += [("upsample x2", "upsample", {}), ("upsample x4 to NCHW", "upsample", {"scale": 4, "out_nchw": True}),
          ("upsample NCHW x", "upsample", {"x": NCHW}), ("upsample flipped x", "upsample", {"flip": True}),
          ("upsample ENABLED off", "upsample", _off("ENABLED")), ("upsample no_grad", "upsample", {"no_grad": True}),
          ("upsample float64", "upsample", {"x": F64}), ("upsample 3-D", "upsample", {"xshape": (64, 8, 8)}),
          ("upsample scale 3", "upsample", {"scale": 3}), ("upsample B C 65536", "upsample", {"xshape": (1024, 64, 1, 1)})]

    c += [("groupnorm", "groupnorm", {}), ("groupnorm ENABLED off", "groupnorm", _off("ENABLED")), ("groupnorm no_grad", "groupnorm", {"no_grad": True}),
          ("groupnorm float64", "groupnorm", {"x": F64}), ("groupnorm NCHW", "groupnorm", {"x": NCHW}),
          ("groupnorm 3-D", "groupnorm", {"xshape": (128, 8, 8)}),
          ("groupnorm without affine", "groupnorm", {"affine": False}), ("groupnorm groups 8 wide", "groupnorm", {"G": 16}),
          ("groupnorm 3 groups", "groupnorm", {"C": 12, "G": 3}), ("groupnorm 128 groups", "groupnorm", {"C": 512, "G": 128}),
          ("groupnorm B 65536", "groupnorm", {"xshape": (65536, 128, 1, 1)})]

    res = {"res": {}}
    c += [("batchnorm relu", "batchnorm", {}), ("batchnorm plain", "batchnorm", {"kw": {"relu": False}}), ("batchnorm residual relu", "batchnorm", res),
          ("batchnorm switch off", "batchnorm", _off("NATIVE_BN")), ("batchnorm ENABLED off", "batchnorm", _off("ENABLED")),
          ("batchnorm refusal not counted", "batchnorm", dict(_off("NATIVE_BN"), kw={"count_refusal": False})),
          ("batchnorm no_grad", "batchnorm", {"no_grad": True}), ("batchnorm x without grad", "batchnorm", {"x": NO_GRAD_X}),
          ("batchnorm eval mode", "batchnorm", {"eval": True}), ("batchnorm without affine", "batchnorm", {"bn": {"affine": False}}),
          ("batchnorm momentum None", "batchnorm", {"bn": {"momentum": None}}),
          ("batchnorm without running statistics", "batchnorm", {"bn": {"track_running_stats": False}}),
          ("batchnorm residual without relu", "batchnorm", dict(res, kw={"relu": False})), ("batchnorm float64 x", "batchnorm", {"x": F64}),
          ("batchnorm NCHW x", "batchnorm", {"x": NCHW}), ("batchnorm offset x", "batchnorm", {"x": OFFSET}),
          ("batchnorm 3-D x", "batchnorm", {"xshape": (64, 8, 8)}), ("batchnorm C 6", "batchnorm", {"xshape": (2, 6, 8, 8)}),
          ("batchnorm 32 features", "batchnorm", {"features": 32}), ("batchnorm one value per channel", "batchnorm", {"xshape": (1, 64, 1, 1)}),
          ("batchnorm residual of another shape", "batchnorm", dict(res, resshape=(2, 64, 8, 4))),
          ("batchnorm float64 residual", "batchnorm", {"res": F64}), ("batchnorm NCHW residual", "batchnorm", {"res": NCHW}),
          ("batchnorm offset residual", "batchnorm", {"res": OFFSET}), ("batchnorm float64 parameters", "batchnorm", {"double": True}),
          ("batchnorm offset weight", "batchnorm", {"weight_offset": True})]

    c += [("se", "se", {}), ("se ReLU given", "se", {"act": lambda: nn.ReLU(inplace=True)}), ("se switch off", "se", _off("NATIVE_SE")),
          ("se ENABLED off", "se", _off("ENABLED")), ("se no_grad", "se", {"no_grad": True}),
          ("se x and res without grad", "se", {"x": NO_GRAD_X, "res": NO_GRAD_X}),
          ("se float64 x", "se", {"x": F64}), ("se float64 res", "se", {"res": F64}), ("se NCHW x", "se", {"x": NCHW}),
          ("se NCHW res", "se", {"res": NCHW}),
          ("se offset x", "se", {"x": OFFSET}), ("se offset res", "se", {"res": OFFSET}), ("se 3-D x", "se", {"xshape": (64, 8, 8)}),
          ("se res of another shape", "se", {"resshape": (2, 64, 8, 4)}), ("se C 32", "se", {"C": 32}), ("se C 8256", "se", {"C": 8256}),
          ("se B 65536", "se", {"xshape": (65536, 64, 1, 1)}), ("se H 0", "se", {"xshape": (2, 64, 0, 8)}),
          ("se block activation swapped", "se", {"act": nn.SiLU}), ("se gate activation swapped", "se", {"swap": {"relu": lambda C: nn.SiLU()}}),
          ("se sigmoid swapped", "se", {"swap": {"sigmoid": lambda C: nn.Tanh()}}),
          ("se bias-free fc1", "se", {"swap": {"fc1": lambda C: nn.Conv2d(C, C // 16, 1, bias=False)}}),
          ("se bias-free fc2", "se", {"swap": {"fc2": lambda C: nn.Conv2d(C // 16, C, 1, bias=False)}}),
          ("se fc1 of 3 channels", "se", {"swap": {"fc1": lambda C: nn.Conv2d(C, 3, 1)}}),
          ("se fc2 from 8 channels", "se", {"swap": {"fc2": lambda C: nn.Conv2d(8, C, 1)}}),
          ("se 3x3 fc1", "se", {"swap": {"fc1": lambda C: nn.Conv2d(C, C // 16, 3, padding=1)}}),
          ("se float64 parameters", "se", {"double": True}), ("se offset fc1 weight", "se", {"weight_offset": True})]
    return c


def _deltas(tc, before):
    return {k: v - before.get(k, 0) for k, v in tc.counters.items() if v != before.get(k, 0)}


def run_case(tc, dev, family, spec):
    """-> (the case's record, the tensors it produced: the result, the leaves' gradients, the sink's view)"""
    patch = dict(SWITCHES, **spec.get("patch", {}))
    saved = {k: getattr(tc, k) for k in patch}
    saved_plans, saved_sinks = tc._plan_cache, dict(tc.grad_sinks)
    rec, tensors = {}, {}
    try:
        for k, v in patch.items():
            setattr(tc, k, v)
        tc._plan_cache = Pinned()
        tc.grad_sinks.clear()
        call, leaves, w = FAMILIES[family](tc, dev, spec)
        sink = fired = owner = None
        if "sink" in spec:
            sink, fired, owner = register_sink(tc, dev, w, spec["sink"])
        before = dict(tc.counters)
        y = None
        try:
            with (torch.no_grad() if spec.get("no_grad") else contextlib.nullcontext()):
                y = call()
        except Exception as e:      # noqa: BLE001 — which exception a refused operand ends in is part of the record
            rec["raises"] = type(e).__name__
        rec["none"] = y is None
        if y is not None:
            rec["grad_fn"] = type(y.grad_fn).__name__ if y.grad_fn is not None else None
            rec["shape"] = list(y.shape)
            rec["contiguous"] = [bool(y.is_contiguous()), bool(y.dim() == 4 and y.is_contiguous(memory_format=torch.channels_last))]
            tensors["y"] = y.detach()
        rec["forward"] = _deltas(tc, before)
        before = dict(tc.counters)
        if y is not None and y.requires_grad:
            try:
                y.sum().backward()
            except Exception as e:      # noqa: BLE001
                rec["backward_raises"] = type(e).__name__
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            tensors.update({"d" + n: t.grad for n, t in leaves.items() if t is not None and t.is_leaf and t.grad is not None})
        rec["backward"] = _deltas(tc, before)
        if sink is not None:
            rec["sink"] = {"written": bool(sink.written), "weight_grad_is_none": w.grad is None, "callback_ran": len(fired),
                           "entry_kept": w.data_ptr() in tc.grad_sinks}
            tensors["sink_view"] = sink.view
        del owner
    finally:
        for k, v in saved.items():
            setattr(tc, k, v)
        tc._plan_cache = saved_plans
        tc.grad_sinks.clear()
        tc.grad_sinks.update(saved_sinks)
    return rec, tensors


def collect(dev=None):
    from fastposecnn_amd.lib import train_conv as tc
    dev = torch.device("cuda:0") if dev is None else torch.device(dev)
    return [dict({"case": name}, **run_case(tc, dev, family, spec)[0]) for name, family, spec in cases()]


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    got = collect()
    with open(OUT, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(rec, separators=(",", ":")) for rec in got) + "\n]\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(got), "cases")
