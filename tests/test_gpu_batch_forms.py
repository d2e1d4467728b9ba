"""The batch plans of the DenseNet, MobileNetV2 and EfficientNet-B0 encoders on the MI355X.  In these families the shape of a launch
alone decides which kernel runs (fpc_dense_conv3x3_form, fpc_dense_pw_form, fpc_conv1x1_f32_form, fpc_mbconv_pw_form are functions
of M = B H W), so the kernels a batch of 32 runs are not the ones the engine tests of a batch of 1 to 3 execute.  Per family, as
test_gpu_net.py::test_net_fullsize_config3_vs_float64 does for ResNet-34: a batch of 32 distinct frames through the native engine,
three frames OF THAT BATCH (tests/_batch_forms.py FRAMES: the first, an interior one and the last) against the float64 CPU module
path of those three frames alone, at the network bar 1e-4 max(1, |ref|max) on c2 .. c5 and all five logits; then the same three
frames as a batch of 3 on the batch-32 plans (copy_plans_from), at the same bar.

The frames are smaller than the workload's 640 x 480 (float64 of that takes tens of seconds): H, W multiples of 32 with
(H / 32)(W / 32) odd — a frame's map is 16 x odd pixels at /8, 4 x odd at /16, odd at /32: no multiple of a 64- or 32-row tile
from /8 down, nor of a 16-row tile from /16 down, so tiles straddle frames (STRADDLE: the forms that meet this here) — at which
the batch's sites still take every form a site of 32 x 480 x 640 takes.  Which form every 1x1 / 3x3 site of the encoder takes is
asserted on the host, from the form functions, with the sites' (M, K, Cout) read off the module (tests/_batch_forms.py), before
anything runs.  tests/test_batch_forms_host.py holds torch's own f32 forward of these frames to a quarter of the bar."""
import copy
import time

import pytest
import torch

import _batch_forms as BF
import _densenet_model as D

pytestmark = pytest.mark.gpu

# The form of every site at BF.BATCH x BF.SHAPES[encoder], in the module's call order (a DenseNet layer is its 1x1, then its 3x3).
#   densenet121, 32 x 352 x 416: block 1 (292 864 pixels) and block 2 (73 216 >= 65 473; 2288 a frame = 35.75 tiles) run the 3x3's tile
#   form, blocks 3 and 4 the split form; every 1x1 of blocks 1 .. 3 and every transition runs 32 x 32 tiles (block 3: 18 304 rows,
#   572 x 4 tiles >= 1024, 572 rows a frame = 17.9 tiles); block 4 (4576 rows) stays on 16 x 16 tiles — it reaches 32 x 32 tiles
#   only at the full 32 x 480 x 640, a form blocks 1 .. 3 take here and test_gpu_densenet.py::test_pw_vs_float64 holds at K up to 1920.
#   mobilenet_v2 and efficientnet-b0, 32 x 96 x 352 (the smallest frame by the rule above): the /2 and /4 maps run 32 x 32 tiles
#   with 1, 3 and 5 channel tiles a wave (and 2 on efficientnet's /8 expands), the deep maps 16 x 16 tiles — form 0, which no site
#   of the full-size batch takes.
FORMS = {
    "densenet121": "1" * 6 * 2 + "1" + "1" * 12 * 2 + "1" + "10" * 24 + "1" + "00" * 16,
    "mobilenet_v2": "1315150101010101010101010100000001",
    "efficientnet-b0": "1315151212010101010101010101010",
}
# the forms some site runs with tiles that straddle frames; the others only meet maps at /2 and /4, where a frame is a whole number
# of tiles (64 (H / 32)(W / 32) pixels at /4) — test_gpu_efficientnet_b0.py's PW_CASES hold forms 2, 3 and 5 on frames of 181 x 181,
# test_gpu_mobilenet_sweep.py forms 3 and 5 on odd row counts
STRADDLE = {
    "densenet121": {("conv3", 0), ("conv3", 1), ("pw", 0), ("pw", 1)},
    "mobilenet_v2": {("pw", 0), ("pw", 1)},
    "efficientnet-b0": {("pw", 0), ("pw", 1), ("pw", 2)},
}


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


def _check(eng, logits, pick, ref, feats, channels, what, tol=1e-4):
    for name, f, C in zip(("c2", "c3", "c4", "c5"), feats[2:], channels):
        got = eng.tensor(name)[pick].permute(0, 3, 1, 2).cpu().double()
        assert got.shape == f.shape and got.shape[1] == C, name
        err = (got - f).abs().max().item()
        print(what, name, "err", err, "ref max", f.abs().max().item())
        assert err <= tol * max(1.0, f.abs().max().item()), (what, name, err)
    for k in ("mask", "quaternion", "scales", "xy", "z"):
        got = logits[k][pick].cpu().double()
        assert got.shape == ref[k].shape, k
        err = (got - ref[k]).abs().max().item()
        print(what, k, "err", err, "ref max", ref[k].abs().max().item())
        assert err <= tol * max(1.0, ref[k].abs().max().item()), (what, k, err)


@pytest.mark.parametrize("encoder", list(BF.SHAPES))
def test_batch32_engine_vs_float64(lib, dev, encoder):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    H, W = BF.SHAPES[encoder]
    B, frames = BF.BATCH, list(BF.FRAMES)
    assert (H // 32) * (W // 32) % 2 == 1 and H % 32 == 0 and W % 32 == 0 and (H, W) != BF.FULL
    m0, hp0 = D.model(lib, encoder)
    # which kernel form every site of this batch runs, and that none of the full-size batch's is missing
    here, full = BF.site_forms(L, m0.encoder, B, H, W), BF.site_forms(L, m0.encoder, B, *BF.FULL)
    assert "".join(str(r[5]) for r in here) == FORMS[encoder], [r for r in here]
    assert BF.form_set(full) <= BF.form_set(here), BF.form_set(full) - BF.form_set(here)
    small = BF.site_forms(L, m0.encoder, 3, 64, 96)              # (the largest batch the engine tests ran before)
    assert not BF.form_set(here) <= BF.form_set(small)
    rows = lambda kind, form: {"conv3": (16, 64), "pw": (16, 32)}[kind][1 if form else 0]
    assert {(kind, form) for _, kind, M, _, _, form in here if (M // B) % rows(kind, form)} == STRADDLE[encoder]

    x32 = D.images(B, H, W)
    x3 = x32[frames].contiguous()
    ref_m = copy.deepcopy(m0).double()
    ref_m.HPARAM = copy.copy(hp0)
    ref_m.HPARAM.USE_NATIVE_ENGINE = False
    t0 = time.time()
    with torch.no_grad():
        ref, feats = ref_m.pure_model_forward(x3.double()), ref_m.encoder(x3.double())
    del ref_m
    t1 = time.time()
    m = copy.deepcopy(m0)
    m.HPARAM = copy.copy(hp0)
    m = m.to(dev)
    try:
        with torch.no_grad():
            out = m(x32.to(dev))
        torch.cuda.synchronize()
        t2 = time.time()
        e32 = m._engines[(B, H, W, next(m.parameters()).device)]
        plans32 = e32.conv_plans()
        _check(e32, out["logits"], frames, ref, feats, BF.CHANNELS[encoder], f"{encoder} batch {B}")
        del out
        torch.cuda.empty_cache()
        with torch.no_grad():
            m(x3.to(dev))                                   # builds the batch-3 engine (its own plans)
            e3 = m._engines[(3, H, W, next(m.parameters()).device)]
            e3.copy_plans_from(e32)
            assert e3.conv_plans() == plans32, "a batch-32 plan did not fit the batch-3 engine"
            out3 = m(x3.to(dev))
        torch.cuda.synchronize()
        _check(e3, out3["logits"], slice(None), ref, feats, BF.CHANNELS[encoder], f"{encoder} batch 3 on the batch-{B} plans")
        print(f"{encoder} {B} x {H} x {W}: float64 of three frames {t1 - t0:.1f} s, first batch-{B} forward (plans tuned) {t2 - t1:.1f} s, "
              f"batch 3 {time.time() - t2:.1f} s")
        del out3, e3, e32
    finally:
        m._engines.clear()                                  # later tests must not inherit the batch-32 workspace
        del m
        torch.cuda.empty_cache()
