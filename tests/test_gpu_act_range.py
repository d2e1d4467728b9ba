"""The activation-range guard of the fp16-piece forms: k_act_range against numpy (exact), the survey forward against the float64
module path, and the guard on networks whose activations leave the envelope of the fp16 pieces (2^-2 .. 2^14 on max |x|) — a
saturating encoder stage, a tiny pyramid — and on one that stays inside.  Network cases: ResNet18-FPN, B = 2, 64 x 96, the shapes
and parameter sets of tests/test_gpu_conv_operands.py, whose small helpers are restated here."""
import copy
import ctypes
import functools
import warnings

import numpy as np
import pytest
import torch

from test_gpu_net import _model

pytestmark = pytest.mark.gpu

FP16_CODES = lambda c: c in (-8, -9, -10, 3100, 5000) or 6000 <= c < 6200 or 7000 <= c < 7100
NET_B, NET_H, NET_W = 2, 64, 96
LO, HI = 2.0 ** -2, 2.0 ** 14
KEYS = ("mask", "quaternion", "scales", "xy", "z")
DECODERS = ("mask_decoder", "rotation_decoder", "translation_decoder", "scales_decoder")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import _native
    _native.lib()
    return L


# ======================================================================================================================
# 1. the kernel against numpy, exactly

GUARD = 4      # floats of NaN in front of and behind the tensor: a read outside it shows in rec[1]
SENTINEL = 0x5EED5EED


def _want(x):
    bits = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    bad = bits >= np.uint32(0x7F800000)
    return [int(bits[~bad].max()) if (~bad).any() else 0, int(bad.sum()), min(int(x.size), 0xFFFFFFFF), SENTINEL]


def _families(n, rng):
    """name -> f32 array of n elements"""
    sub = np.float32(2.0 ** -140)
    base = rng.standard_normal(n).astype(np.float32)
    out = {"normal": base.copy()}
    for where, pos in (("first", 0), ("last", n - 1), ("middle", n // 2)):
        if n == 0:
            break
        pos_max, neg_max = base.copy(), base.copy()
        pos_max[pos], neg_max[pos] = 77.25, -913.5
        out["max-" + where], out["negative-max-" + where] = pos_max, neg_max
    out["negative-zero"] = np.full(n, -0.0, np.float32)
    out["subnormal-only"] = (sub * rng.integers(-7, 8, n)).astype(np.float32)
    if n:
        for name, v in (("plus-inf", np.inf), ("minus-inf", -np.inf), ("nan", np.nan)):
            alone = np.full(n, v, np.float32)
            mixed = base.copy()
            mixed[[0, n - 1, n // 2]] = v
            out[name + "-alone"], out[name + "-mixed"] = alone, mixed
        every = base.copy()
        every[::3] = np.array([np.inf, -np.inf, np.nan, -0.0, sub], np.float32)[np.arange(len(every[::3])) % 5]
        out["everything-mixed"] = every
    return out


def _launch(L, nat, buf, offset, n, rec):
    nat.check(L.fpc_act_range(buf.data_ptr() + 4 * (GUARD + offset), n, rec.data_ptr(), nat.stream()), "fpc_act_range")


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "one-float-off"])
@pytest.mark.parametrize("n", [0, 1, 3, 255, 1029, 2 ** 16 + 5])
def test_act_range_equals_numpy(lib, dev, n, offset):
    """rec[0..2] equal numpy's on every family, from a 16-byte aligned base and from one float behind it; rec[3] is not written;
    NaN guards around the tensor show a read outside it; two launches into one record accumulate."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    rng = np.random.default_rng(1000 * n + offset)
    fams = _families(n, rng)
    bufs, recs = [], torch.zeros((len(fams) + 1, 4), dtype=torch.int32, device=dev)
    recs[:, 3] = SENTINEL
    for k, x in enumerate(fams.values()):
        host = np.full(n + 2 * GUARD + 1, np.nan, np.float32)
        host[GUARD + offset:GUARD + offset + n] = x
        buf = torch.from_numpy(host).to(dev)
        assert buf.data_ptr() % 16 == 0
        bufs.append(buf)
        _launch(L, nat, buf, offset, n, recs[k])
    # accumulation: the first two families into one record
    xs = list(fams.values())[:2]
    for buf in bufs[:2]:
        _launch(L, nat, buf, offset, n, recs[len(fams)])
    torch.cuda.synchronize()
    got = (recs.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).tolist()
    for k, (name, x) in enumerate(fams.items()):
        assert got[k] == _want(x), (name, n, offset, got[k], _want(x))
    both = _want(np.concatenate(xs))
    assert got[len(fams)] == both, ("accumulated", got[len(fams)], both)
    if n:
        assert got[len(fams)][2] == 2 * n


def test_act_range_arguments(lib, dev):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    buf, rec = torch.zeros(16, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    assert L.fpc_act_range(buf.data_ptr(), -1, rec.data_ptr(), nat.stream()) == -1
    assert L.fpc_act_range(buf.data_ptr() + 2, 4, rec.data_ptr(), nat.stream()) == -1
    assert L.fpc_act_range(buf.data_ptr(), 4, None, nat.stream()) == -1
    assert L.fpc_act_range(None, 0, rec.data_ptr(), nat.stream()) == 0
    torch.cuda.synchronize()
    assert rec.tolist() == [0, 0, 0, 0]


# ======================================================================================================================
# 2. networks (helpers restated from tests/test_gpu_conv_operands.py)

def _encoder(model):
    for mod in model.modules():
        if all(hasattr(mod, a) for a in ("conv1", "bn1", "relu", "maxpool", "layer1", "layer4")):
            return mod
    raise AssertionError("no ResNet encoder in the model")


def _laterals(model):
    out = []
    for mod in model.modules():
        if all(hasattr(mod, a) for a in ("p5", "p4", "p3", "p2", "seg_blocks")):
            out += [mod.p5, mod.p4.skip_conv, mod.p3.skip_conv, mod.p2.skip_conv]
    assert out
    return out


MEAN_SHIFT = 0.5


def _checkpoint_like(m, seed=5):
    """Conv weights with a non-zero mean, folded BatchNorm scale log-uniform in [2^-2, 2^1] per channel, shifts of both signs."""
    g = torch.Generator().manual_seed(seed)
    enc = _encoder(m)
    with torch.no_grad():
        for mod in enc.modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.add_(MEAN_SHIFT * mod.weight.std() / (mod.weight[0].numel()) ** 0.5)
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.running_var.copy_(torch.rand(n, generator=g) + 0.5)
                fold = 2.0 ** (torch.rand(n, generator=g) * 3 - 2)
                mod.weight.copy_(fold * (mod.running_var + mod.eps).sqrt())
                mod.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
                mod.bias.copy_(torch.randn(n, generator=g) * 0.2)


def _saturate_c3(m, x, target=16.5):
    """The last BatchNorm of layer2 scaled by a power of two (exact) so that c3's float64 maximum lies in [2^16, 2^17]."""
    enc = _encoder(m)
    with torch.no_grad():
        top = copy.deepcopy(enc).double()(x.double())[3].abs().max().item()
        f = 2.0 ** round(target - np.log2(top))
        last = enc.layer2[-1].bn2
        last.weight.mul_(f)
        last.bias.mul_(f)


def _reference(m, hp, x):
    """float64 module path with the maxima of what EVERY convolution reads (by module name) and of c2 .. c5."""
    ref_m = copy.deepcopy(m).double()
    ref_m.HPARAM = copy.copy(hp)
    ref_m.HPARAM.USE_NATIVE_ENGINE = False
    seen, hooks = {}, []
    for name, mod in ref_m.named_modules():
        if isinstance(mod, torch.nn.Conv2d):
            hooks.append(mod.register_forward_pre_hook(lambda _m, inp, name=name: seen.__setitem__(name, inp[0].abs().max().item())))
    with torch.no_grad():
        ref = ref_m.pure_model_forward(x.double())
        feats = _encoder(ref_m)(x.double())
    for h in hooks:
        h.remove()
    return ref, seen, [f.abs().max().item() for f in feats[2:]]


@functools.lru_cache(maxsize=None)
def _net_case(name):
    from fastposecnn_amd import synth
    import fastposecnn_amd.lib as L
    m, hp = _model(L, None, "resnet18")
    x = torch.stack([synth.make_image(i, NET_H, NET_W) for i in range(NET_B)])
    if name == "checkpoint-like":
        _checkpoint_like(m)
    if name == "saturating":
        _saturate_c3(m, x)
    if name == "tiny-pyramid":
        with torch.no_grad():
            for conv in _laterals(m):
                conv.weight.mul_(2.0 ** -10)
                conv.bias.mul_(2.0 ** -10)
    ref, seen, cmax = _reference(m, hp, x)
    return m, hp, x, ref, seen, cmax


def _force_fp16(eng):
    """every site that has an fp16-piece form ON it (64 x 96 is below the smallest frame the fused stem takes)"""
    assert eng.force_winograd(9) > 0
    eng.force_fold(1)
    assert eng.force_direct_h3(1) > 0
    codes = [p[2] for p in eng.conv_plans()]
    assert sum(1 for c in codes if FP16_CODES(c)) >= 20, codes


def _engine(m, dev, level, **kw):
    """Split level 0: f32 products.  1: every Winograd site on the bf16 x 3 form -7.  3: every fp16-piece site forced on."""
    from fastposecnn_amd.engine import NetEngine
    eng = NetEngine(m, NET_B, NET_H, NET_W, dev, autotune=False, split_precision=level, **kw)
    if level == 1:
        assert eng.force_winograd(7) > 0
    if level == 3:
        _force_fp16(eng)
    else:
        assert not any(FP16_CODES(p[2]) for p in eng.conv_plans())
    return eng


def _errors(logits, ref):
    return {k: (logits[k].cpu().double() - ref[k]).abs().max().item() / max(1.0, ref[k].abs().max().item()) for k in KEYS}


def _net_errors(eng, x, ref, dev):
    with torch.no_grad():
        logits, _ = eng.forward(x.to(dev))
    return _errors(logits, ref)


def _site_names(eng):
    """module name of every convolution site: the sites are numbered in the order of their weights among the plan's parameters"""
    names = [n[:-len(".weight")] for n, t in zip(eng._names, eng._params) if n.endswith(".weight") and t.dim() == 4 and "_head." not in n]
    assert len(names) == len(eng.conv_plans())
    return names


def _site_reference(names, seen):
    """float64 maximum of what site i reads; a grouped site (the decoders share the index of decoder 0): over the four decoders;
    None for the other decoders' indices, which no launch uses"""
    out = []
    for n in names:
        if n.startswith(DECODERS[1:]):
            out.append(None)
        elif n.startswith(DECODERS[0]):
            out.append(max(seen[d + n[len(DECODERS[0]):]] for d in DECODERS))
        else:
            out.append(seen[n])
    return out


def _guard_until_stable(eng, x):
    """survey + guard until a pass demotes nothing (a site behind a saturating one is surveyed on that site's wrong output);
    returns every site demoted and the last survey's outputs and records"""
    moved = []
    for _ in range(len(eng.conv_plans()) + 1):
        logits, cat, rec = eng.survey(x)
        demoted = eng.guard_ranges(rec)
        if not demoted:
            return moved, logits, cat, rec
        moved += demoted
    raise AssertionError("the guard does not settle")


def _in_range(v):
    return v == 0 or LO <= v < HI


def test_survey_matches_the_float64_maxima_and_changes_nothing(lib, dev):
    m, hp, x, ref, seen, cmax = _net_case("checkpoint-like")
    eng = _engine(copy.deepcopy(m).to(dev), dev, 0)
    xd = x.to(dev)
    plans = eng.conv_plans()
    with torch.no_grad():
        plain, plain_cat = eng.forward(xd)
        logits, cat, rec = eng.survey(xd)
        again, _ = eng.forward(xd)
    assert eng.conv_plans() == plans and eng.guarded() == []
    for k in KEYS:
        assert torch.equal(plain[k], logits[k]) and torch.equal(plain[k], again[k]), k
        assert torch.equal(plain_cat[k], cat[k]), k
    assert rec.shape == (len(plans), 4) and rec.dtype == torch.int64
    names = _site_names(eng)
    want = _site_reference(names, seen)
    got = eng.record_max(rec).tolist()
    checked = 0
    for i, (n, w) in enumerate(zip(names, want)):
        if w is None:
            assert rec[i].tolist() == [0, 0, 0, 0], n      # a grouped site's other decoders: never written
            continue
        assert rec[i, 2].item() > 0 and rec[i, 1].item() == 0 and rec[i, 3].item() == 0, (n, rec[i].tolist())
        mod = dict(m.named_modules())[n]
        if mod.kernel_size == (3, 3) and mod.stride == (1, 1):
            assert abs(got[i] - w) <= 1e-3 * w, (n, got[i], w)
            checked += 1
    assert checked >= 8 + 7, checked
    # the visit counts: the stem reads the NHWC4 image, a grouped 3x3 site four decoders' tensors
    assert rec[0, 2].item() == NET_B * NET_H * NET_W * 4
    s50 = names.index("mask_decoder.seg_blocks.0.block.0.block.0")
    assert rec[s50, 2].item() == 4 * NET_B * (NET_H // 32) * (NET_W // 32) * 256


def _f32_bits(t):
    return int(t.reshape(1).float().cpu().view(torch.int32).item())


def test_survey_next_arguments_and_disarming(lib, dev):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    m, hp, x, ref, seen, cmax = _net_case("checkpoint-like")
    eng = _engine(copy.deepcopy(m).to(dev), dev, 0)
    xd = x.to(dev)
    sites = len(eng.conv_plans())
    rec = torch.zeros((sites + 1, 4), dtype=torch.int32, device=dev)
    assert L.fpc_net_survey_next(eng._h, rec.data_ptr(), sites + 1) == -1
    assert L.fpc_net_survey_next(eng._h, rec.data_ptr(), sites - 1) == -1
    assert L.fpc_net_survey_next(eng._h, rec.data_ptr() + 2, sites) == -1
    with torch.no_grad():
        eng.forward(xd)                      # nothing was armed
        assert L.fpc_net_survey_next(eng._h, rec.data_ptr(), sites) == 0
        assert L.fpc_net_survey_next(eng._h, None, sites) == 0      # disarmed again
        eng.forward(xd)
        assert L.fpc_net_survey_next(eng._h, rec.data_ptr(), sites) == 0
        with pytest.raises(RuntimeError):    # a call the library refuses before any launch (a logits pointer missing) disarms too
            nat.check(L.fpc_net_forward(eng._h, xd.data_ptr(), xd.data_ptr(), None, None, None, None, None, None, None, None, None,
                                        nat.stream()), "fpc_net_forward")
        eng.forward(xd)
        with pytest.raises(RuntimeError):    # the front end refuses a wrong shape before arming
            eng.survey(xd[:1])
        eng.forward(xd)
    torch.cuda.synchronize()
    assert not rec.any().item()
    with torch.no_grad():
        _, _, got = eng.survey(xd)
    assert got[:, 2].sum().item() > 0


def test_fused_stem_is_surveyed_and_demoted(lib, dev):
    """Plan 3100 (the stem fused with its max-pool) on 64 x 128, a frame its launch takes (stem output 32 x 64): the survey hook outside
    run_conv covers the NHWC4 image, an image with max |x| >= 2^14 moves the site to 3000 + max-pool, the outputs of the survey are
    those of a plain forward, and fpc_net_force_stem_pool afterwards wins."""
    from fastposecnn_amd import synth
    from fastposecnn_amd.engine import NetEngine
    H, W = 64, 128
    m, hp, _, _, _, _ = _net_case("checkpoint-like")
    eng = NetEngine(copy.deepcopy(m).to(dev), NET_B, H, W, dev, autotune=False, split_precision=3)
    assert eng.force_stem_pool(1) == 1
    before = eng.conv_plans()
    assert before[0][2] == 3100 and sum(1 for p in before if FP16_CODES(p[2])) == 1
    x = torch.stack([synth.make_image(i, H, W) for i in range(NET_B)]).to(dev)
    assert LO <= x.abs().max().item() < HI
    big = x * 2.0 ** 15
    with torch.no_grad():
        plain, plain_cat = eng.forward(x)
        logits, cat, rec = eng.survey(x)
        assert all(torch.equal(plain[k], logits[k]) and torch.equal(plain_cat[k], cat[k]) for k in KEYS)
        assert rec[0].tolist() == [_f32_bits(x.abs().max()), 0, NET_B * H * W * 4, 0]
        assert eng.guard_ranges(rec) == [] and eng.conv_plans() == before
        plain_big, _ = eng.forward(big)
        logits_big, _, rec = eng.survey(big)
        assert all(torch.equal(plain_big[k], logits_big[k]) for k in KEYS)
        assert rec[0].tolist() == [_f32_bits(big.abs().max()), 0, NET_B * H * W * 4, 0]
        assert eng.guard_ranges(rec) == [0] and eng.guarded() == [0]
        after = eng.conv_plans()
        assert after[0][2] == 3000 and after[1:] == before[1:]
        assert eng.guard_ranges(rec) == []
        # 3000 + max-pool is range-free: the same frame against float64 of the stem stage is the existing stem tests' business;
        # here: finite, and a frame in range gives what the bf16 x 3 stem gives on a plan that was never guarded
        other = NetEngine(copy.deepcopy(m).to(dev), NET_B, H, W, dev, autotune=False, split_precision=3)
        assert other.force_stem_pool(1) == 1 and other.force_stem_pool(0) == 1
        assert other.conv_plans() == after
        a, _ = eng.forward(x)
        b, _ = other.forward(x)
        assert all(torch.equal(a[k], b[k]) for k in KEYS)
        # an explicit request wins and clears the demotion; the same record demotes it again
        assert eng.force_stem_pool(1) == 1
        assert eng.guarded() == [] and eng.conv_plans() == before
        assert eng.guard_ranges(rec) == [0] and eng.conv_plans() == after


def test_demotions_outlast_a_reload_of_the_parameters(lib, dev):
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    mm = copy.deepcopy(m).to(dev)
    eng = _engine(mm, dev, 3)
    xd = x.to(dev)
    with torch.no_grad():
        moved, logits, _, _ = _guard_until_stable(eng, xd)
        assert moved
        plans, guarded = eng.conv_plans(), eng.guarded()
        eng.bind(mm)      # fpc_net_load_params
        assert eng.conv_plans() == plans and eng.guarded() == guarded
        again, _ = eng.forward(xd)
    assert all(torch.equal(again[k], logits[k]) for k in KEYS)


def _assert_saturating(seen, cmax):
    assert 2.0 ** 16 <= cmax[1] <= 2.0 ** 17, cmax
    assert LO <= cmax[0] < HI, cmax


def test_saturating_network_needs_the_guard(lib, dev):
    """c3 in [2^16, 2^17]: past the first fp16 piece.  Unguarded, the level-3 engine with every fp16-piece site on misses the
    1e-4 bar (asserted: the scenario proves itself); after survey + guard it meets it, the sites that read the oversized tensors are
    on range-free codes and in-envelope encoder sites are still on fp16 pieces."""
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    _assert_saturating(seen, cmax)
    eng = _engine(copy.deepcopy(m).to(dev), dev, 3)
    xd = x.to(dev)
    before = eng.conv_plans()
    unguarded = _net_errors(eng, xd, ref, dev)
    print("saturating level 3 unguarded", unguarded)
    assert max(unguarded.values()) > 1e-4, unguarded
    with torch.no_grad():
        moved, logits, _, rec = _guard_until_stable(eng, xd)
    guarded = _errors(logits, ref)
    after = eng.conv_plans()
    print("saturating level 3 guarded", guarded, "demoted", [(i, before[i][2], after[i][2]) for i in moved])
    assert max(guarded.values()) <= 1e-4, guarded
    assert sorted(moved) == eng.guarded()
    names = _site_names(eng)
    want = _site_reference(names, seen)
    for i, (n, w) in enumerate(zip(names, want)):
        if w is not None and w >= HI * (1 + 1e-3) and after[i][2] != 5000:      # (clear of the bound: the engine's maximum is f32's)
            assert not FP16_CODES(after[i][2]), (n, w, after[i])
    for n in ("encoder.layer3.0.conv1", "encoder.layer3.0.downsample.0", "mask_decoder.p3.skip_conv"):      # the readers of c3
        i = names.index(n)
        assert FP16_CODES(before[i][2]) and not FP16_CODES(after[i][2]) and i in moved, (n, before[i], after[i])
    # the three-product codes go to the same tiling / parts on bf16 x 3
    for i in moved:
        if 6000 <= before[i][2] < 6200:
            assert after[i][2] == before[i][2] % 100 and after[i][:2] == before[i][:2], (before[i], after[i])
        if 7000 <= before[i][2] < 7100:
            assert after[i][2] == before[i][2] - 5000, (before[i], after[i])
        if before[i][2] == -9:
            assert after[i][2] == -7
    kept = [n for i, n in enumerate(names) if n.startswith("encoder.layer1") and FP16_CODES(after[i][2])]
    assert kept, after
    # a plain forward on the guarded plans gives what the last survey gave
    with torch.no_grad():
        plain, _ = eng.forward(xd)
    assert all(torch.equal(plain[k], logits[k]) for k in KEYS)


@pytest.mark.parametrize("level", [0, 1])
def test_saturating_network_on_the_range_free_levels(lib, dev, level):
    """the control: levels 0 and 1 meet the bar on the same parameters without any guard"""
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    eng = _engine(copy.deepcopy(m).to(dev), dev, level)
    errs = _net_errors(eng, x.to(dev), ref, dev)
    print("saturating level", level, errs)
    assert max(errs.values()) <= 1e-4, errs


def test_tiny_pyramid_is_demoted_and_meets_the_bar(lib, dev):
    """Every FPN lateral x 2^-10: the decoder's 3x3 sites that read p5 .. p2 see tensors far below 2^-2."""
    m, hp, x, ref, seen, cmax = _net_case("tiny-pyramid")
    decoder = {k: v for k, v in seen.items() if "seg_blocks" in k and k.endswith("0.block.0")}
    assert len(decoder) == 16 and all(2.0 ** -8 < v < 2.0 ** -5 for v in decoder.values()), decoder
    eng = _engine(copy.deepcopy(m).to(dev), dev, 3)
    xd = x.to(dev)
    before = eng.conv_plans()
    unguarded = _net_errors(eng, xd, ref, dev)
    with torch.no_grad():
        moved, logits, _, rec = _guard_until_stable(eng, xd)
    guarded = _errors(logits, ref)
    print("tiny-pyramid level 3 unguarded", unguarded, "guarded", guarded)
    names, after = _site_names(eng), eng.conv_plans()
    for blk in (0, 1, 2, 3):      # s5.0, s4.0, s3.0, s2.0 (the fold: by its p3 record)
        i = names.index("mask_decoder.seg_blocks.%d.block.0.block.0" % blk)
        assert i in moved and before[i][2] == -9 and after[i][2] == -7, (blk, before[i], after[i])
    assert after[names.index("mask_decoder.p2.skip_conv")][2] != 5000      # the p2 lateral runs again
    assert max(guarded.values()) <= 1e-4, guarded


def test_in_envelope_network_is_left_alone(lib, dev):
    m, hp, x, ref, seen, cmax = _net_case("checkpoint-like")
    xd = x.to(dev)
    never = _engine(copy.deepcopy(m).to(dev), dev, 3)
    eng = _engine(copy.deepcopy(m).to(dev), dev, 3)
    with torch.no_grad():
        want, want_cat = never.forward(xd)
        logits, cat, rec = eng.survey(xd)
        demoted = eng.guard_ranges(rec)
        got, got_cat = eng.forward(xd)
    mx = eng.record_max(rec).tolist()
    print("in-envelope maxima of the fp16-piece sites", sorted(mx[i] for i, p in enumerate(eng.conv_plans()) if FP16_CODES(p[2]) and p[2] != 5000))
    assert demoted == [] and eng.guarded() == [], [(i, mx[i]) for i in demoted]
    assert eng.conv_plans() == never.conv_plans()
    for k in KEYS:
        assert torch.equal(want[k], logits[k]) and torch.equal(want[k], got[k]) and torch.equal(want_cat[k], got_cat[k]), k
    assert max(_errors(got, ref).values()) <= 1e-4


def test_tuned_engine_is_guarded(lib, dev):
    """autotune=True at the default level: whatever the tuner picked, after the guard no site whose input is outside the bounds is on
    an fp16-piece code, the fallbacks are range-free candidates of the tuner, and the bar holds."""
    from fastposecnn_amd.engine import NetEngine
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    eng = NetEngine(copy.deepcopy(m).to(dev), NET_B, NET_H, NET_W, dev, autotune=True, split_precision=3)
    xd = x.to(dev)
    before = eng.conv_plans()
    with torch.no_grad():
        moved, logits, _, rec = _guard_until_stable(eng, xd)
    after = eng.conv_plans()
    print("tuned: demoted", [(i, before[i][2], after[i][2]) for i in moved])
    mx = eng.record_max(rec).tolist()
    for i, p in enumerate(after):
        if FP16_CODES(p[2]) and p[2] != 5000 and rec[i, 2].item():
            assert rec[i, 1].item() == 0 and _in_range(mx[i]), (i, p, mx[i])
    assert all(not FP16_CODES(after[i][2]) for i in moved)
    errs = _errors(logits, ref)
    print("tuned guarded", errs)
    assert max(errs.values()) <= 1e-4, errs


def test_graph_is_recorded_again_after_a_demotion(lib, dev):
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    side = torch.cuda.Stream(device=dev)
    with torch.no_grad(), torch.cuda.stream(side):
        eng = _engine(copy.deepcopy(m).to(dev), dev, 3, graph=True)
        xd = x.to(dev)
        eng.forward(xd)
        assert eng.graph_recorded()
        _, _, rec = eng.survey(xd)
        assert eng.graph_recorded()          # a survey launches its kernels and keeps the recorded graph
        assert eng.guard_ranges(rec)
        assert not eng.graph_recorded()      # the plans changed
        a, _ = eng.forward(xd)
        a = {k: v.clone() for k, v in a.items()}
        b, _ = eng.forward(xd)
        assert eng.graph_recorded()
    side.synchronize()
    assert all(torch.equal(a[k], b[k]) for k in KEYS)


# ---- the module

def _module(m, hp, dev, **flags):
    """a copy of the model on the device with its level-3 plan built ahead of the first forward and every fp16-piece site forced on
    (the static plans have none), so that the first model(x) is the plan's first real forward"""
    mm = copy.deepcopy(m)
    mm.HPARAM = copy.copy(hp)
    mm.HPARAM.ENGINE_AUTOTUNE = False
    for k, v in flags.items():
        setattr(mm.HPARAM, k, v)
    mm = mm.to(dev).eval()
    return mm


def _prepare(mm, xd):
    with torch.no_grad():
        eng = mm._engine_for(xd)
    _force_fp16(eng)
    return eng


def test_module_guard_on_the_first_call(lib, dev):
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    xd = x.to(dev)
    mm = _module(m, hp, dev, ENGINE_RANGE_GUARD=True)
    eng = _prepare(mm, xd)
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        out = mm(xd)
    errs = _errors(out["logits"], ref)
    print("module, guarded first call", errs)
    assert max(errs.values()) <= 1e-4, errs
    ours = [w for w in caught if "activation-range guard" in str(w.message)]
    assert len(ours) == 1 and issubclass(ours[0].category, RuntimeWarning), [str(w.message) for w in caught]
    assert eng.guarded() and all("site %d " % i in str(ours[0].message) for i in eng.guarded())
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        again = mm(xd)
    assert not [w for w in caught if "activation-range guard" in str(w.message)]
    assert all(torch.equal(out["logits"][k], again["logits"][k]) for k in KEYS)


def test_module_without_the_flag_is_the_plain_engine(lib, dev):
    """the default (the flag never touched): the plan the model builds and what it returns equal an engine built directly, which no
    guard code ever saw; nothing is surveyed — on the saturating parameters, where a survey would demote"""
    from fastposecnn_amd import config
    assert config.DEFAULT_POSE_HPARAM.ENGINE_RANGE_GUARD is False and config.DEFAULT_POSE_HPARAM.ENGINE_RANGE_GUARD_EVERY == 0
    assert (config.DEFAULT_POSE_HPARAM.ENGINE_RANGE_LO, config.DEFAULT_POSE_HPARAM.ENGINE_RANGE_HI) == (LO, HI)
    m, hp, x, ref, seen, cmax = _net_case("saturating")
    assert "ENGINE_RANGE_GUARD" not in vars(hp)
    xd = x.to(dev)
    mm = _module(m, hp, dev)
    eng = _prepare(mm, xd)
    direct = _engine(copy.deepcopy(m).to(dev), dev, 3)
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        out = mm(xd)
        want, want_cat = direct.forward(xd)
    assert not [w for w in caught if "activation-range guard" in str(w.message)]
    assert eng.conv_plans() == direct.conv_plans() and eng.guarded() == [] and eng.guard_forwards == 0
    assert all(torch.equal(out["logits"][k], want[k]) and torch.equal(out["categorical"][k], want_cat[k]) for k in KEYS)


def test_module_surveys_every_nth_forward(lib, dev):
    """ENGINE_RANGE_GUARD_EVERY = 2: forwards 1, 3, 5, ... survey.  The third frame is the first one out of range (the image x 2^16):
    the sites are demoted then, not before, and stay so; the fourth forward (out of range again) is not surveyed."""
    m, hp, x, ref, seen, cmax = _net_case("checkpoint-like")
    xd = x.to(dev)
    mm = _module(m, hp, dev, ENGINE_RANGE_GUARD=True, ENGINE_RANGE_GUARD_EVERY=2)
    eng = _prepare(mm, xd)
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        mm(xd)
        mm(xd)
        assert eng.guarded() == [] and eng.guard_forwards == 2
        assert not [w for w in caught if "activation-range guard" in str(w.message)]
        out = mm(xd * 2.0 ** 16)      # the third forward is surveyed again
    assert eng.guarded(), eng.conv_plans()
    assert len([w for w in caught if "activation-range guard" in str(w.message)]) == 1
    assert not any(FP16_CODES(eng.conv_plans()[i][2]) for i in eng.guarded())
    assert all(torch.isfinite(out["logits"][k]).all() for k in KEYS)
    moved = eng.guarded()
    with warnings.catch_warnings(record=True) as caught, torch.no_grad():
        warnings.simplefilter("always")
        mm(xd * 2.0 ** 16)
        mm(xd)                      # the fifth: surveyed, in range
    assert eng.guarded() == moved and eng.guard_forwards == 5      # never undone
    assert not [w for w in caught if "activation-range guard" in str(w.message)]
