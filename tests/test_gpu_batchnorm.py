"""The encoder's training-mode BatchNorm (+ residual add) (+ ReLU) on the native kernels (csrc/batchnorm.hip,
lib/train_conv.batchnorm_act, lib/backbone.BatchNorm2d): forward, backward, running statistics and the routing of the
ResNet blocks, against torch.nn.BatchNorm2d in float64 on the CPU.  Bars as for the decoder's GroupNorm
(test_gpu_train.py::test_native_groupnorm_relu_forward_and_backward_vs_float64)."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NHWC = torch.channels_last


@pytest.fixture(autouse=True)
def native_bn_on(monkeypatch):
    """The switch FPC_TRAIN_NATIVE_BN ships off: these tests are about the path it turns on."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_BN", True)


def _close(got, want, what, rel):
    err = (got.detach().cpu().double() - want.detach()).abs().max().item()
    bar = rel * max(1.0, want.detach().abs().max().item())
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar, (what, err, bar)


def _inputs(shape, with_res):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(shape, generator=g) * 1.5 + 0.7          # a mean that is not small against the spread
    gy = torch.randn(shape, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    res = torch.randn(shape, generator=g) if with_res else None
    return x, gy, gamma, beta, res


def _modules(C, gamma, beta, **kw):
    from fastposecnn_amd.lib import backbone
    bn = backbone.BatchNorm2d(C, **kw)
    ref = torch.nn.BatchNorm2d(C, **kw).double()
    if gamma is not None:
        bn.weight.data, bn.bias.data = gamma.clone(), beta.clone()
        ref.weight.data, ref.bias.data = gamma.double(), beta.double()
    return bn.to(DEV), ref


SHAPES = [(1, 64, 3, 5), (2, 64, 15, 20), (3, 128, 33, 17), (2, 512, 4, 5), (2, 2048, 2, 3), (8, 64, 48, 64)]


@pytest.mark.parametrize("mode", ["plain", "relu", "res+relu"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_native_batchnorm_act_forward_and_backward_vs_float64(shape, mode):
    from fastposecnn_amd.lib import train_conv
    B, C, H, W = shape
    relu, with_res = mode != "plain", mode == "res+relu"
    x, gy, gamma, beta, res = _inputs(shape, with_res)
    bn, ref = _modules(C, gamma, beta)
    xr = x.double().requires_grad_()
    rr = res.double().requires_grad_() if with_res else None
    z = ref(xr) if rr is None else ref(xr) + rr
    yr = torch.relu(z) if relu else z
    yr.backward(gy.double())

    xd = x.to(DEV).contiguous(memory_format=NHWC).requires_grad_()
    rd = res.to(DEV).contiguous(memory_format=NHWC).requires_grad_() if with_res else None
    before = dict(train_conv.counters)
    y = train_conv.batchnorm_act(xd, bn, rd, relu=relu)
    assert y is not None and train_conv.counters["bn_native"] == before["bn_native"] + 1
    assert train_conv.counters["bn_torch"] == before["bn_torch"]
    assert y.is_contiguous(memory_format=NHWC) and y.grad_fn.__class__.__name__.startswith("_BatchNormActFn")
    y.backward(gy.to(DEV).contiguous(memory_format=NHWC))
    torch.cuda.synchronize()

    assert int(bn.num_batches_tracked) == 1
    _close(bn.running_mean, ref.running_mean, "running_mean", 2e-5)
    _close(bn.running_var, ref.running_var, "running_var", 2e-5)
    # elements whose pre-activation is within rounding of 0 may take the other side of the ReLU: compare away from it
    safe = (z.detach().abs() > 1e-4) if relu else torch.ones_like(z, dtype=torch.bool)
    excluded = 1.0 - safe.double().mean().item()
    print("excluded share", excluded)
    assert excluded <= 1e-3
    _close(y.detach().cpu().double() * safe, yr.detach() * safe, "y", 2e-5)
    want = {"dx": xr.grad, "dgamma": ref.weight.grad, "dbeta": ref.bias.grad, "dres": rr.grad if with_res else None}
    if not bool(safe.all()):       # a flipped unit changes the channel's sums: compare against float64 with the native mask instead
        mask = (y.detach().cpu() > 0).double()
        xr2 = x.double().requires_grad_()
        rr2 = res.double().requires_grad_() if with_res else None
        w2, b2 = gamma.double().requires_grad_(), beta.double().requires_grad_()
        z2 = F.batch_norm(xr2, None, None, w2, b2, True, 0.1, ref.eps)
        z2 = z2 if rr2 is None else z2 + rr2
        (z2 * mask).backward(gy.double())
        want = {"dx": xr2.grad, "dgamma": w2.grad, "dbeta": b2.grad, "dres": rr2.grad if with_res else None}
    _close(xd.grad, want["dx"], "dx", 1e-4)
    _close(bn.weight.grad, want["dgamma"], "dgamma", 1e-4)
    _close(bn.bias.grad, want["dbeta"], "dbeta", 1e-4)
    if with_res:
        _close(rd.grad, want["dres"], "dres", 1e-4)


def test_native_batchnorm_statistics_survive_a_large_offset():
    """Activations with |mean| >> std: E[x^2] - mean^2 from f32 sums cancels to nothing there; the per-chunk centred sums
    combined by Chan's formula track the float64 statistics.  x itself carries 100 * 2^-24 = 6e-6 of f32 rounding against a
    spread of 0.05: 2e-4 of a normalised unit (the GroupNorm offset test's bars, for its reason)."""
    from fastposecnn_amd.lib import train_conv
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 64, 40, 56
    x = torch.randn((B, C, H, W), generator=g) * 0.05 + 100.0
    bn, ref = _modules(C, None, None)
    want = torch.relu(ref(x.double())).detach()
    y = train_conv.batchnorm_act(x.to(DEV).contiguous(memory_format=NHWC), bn, relu=True)
    assert y is not None
    torch.cuda.synchronize()
    got = y.detach().cpu().double()
    err = (got - want).abs().max().item()
    print("offset err", err, "std", got.std().item(), want.std().item())
    assert err <= 2e-3, err
    assert abs(got.std().item() - want.std().item()) <= 1e-3


def test_native_batchnorm_is_bit_reproducible():
    from fastposecnn_amd.lib import train_conv
    shape = (8, 64, 48, 64)
    x, gy, gamma, beta, res = _inputs(shape, True)
    outs = []
    for _ in range(2):
        bn, _ref = _modules(shape[1], gamma, beta)
        xd = x.to(DEV).contiguous(memory_format=NHWC).requires_grad_()
        rd = res.to(DEV).contiguous(memory_format=NHWC).requires_grad_()
        y = train_conv.batchnorm_act(xd, bn, rd, relu=True)
        y.backward(gy.to(DEV).contiguous(memory_format=NHWC))
        torch.cuda.synchronize()
        outs.append([t.detach().clone() for t in (y, xd.grad, rd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_batchnorm_entry_points_refuse_bad_arguments():
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    P, C = 40, 64
    f = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV)
    x, y, dy, dx = f(P * C + 4), f(P * C), f(P * C), f(P * C)
    gamma, beta, rm, rv, dg, db = f(C), f(C), f(C), f(C), f(C), f(C)
    stats, part = f(2 * C), f(max(int(L.fpc_batchnorm_scratch_floats(P, C)), 2 * C))
    assert L.fpc_batchnorm_scratch_floats(P, C) >= 2 * C

    def fwd(xp, g, P_, C_, res=None, relu=1):
        return L.fpc_batchnorm_fwd(xp, res, g, beta.data_ptr(), rm.data_ptr(), rv.data_ptr(), y.data_ptr(), stats.data_ptr(),
                                   part.data_ptr(), P_, C_, 1e-5, 0.1, relu, nat.stream())

    def bwd(xp, g, P_, C_):
        return L.fpc_batchnorm_bwd(xp, y.data_ptr(), dy.data_ptr(), g, stats.data_ptr(), dx.data_ptr(), None, dg.data_ptr(),
                                   db.data_ptr(), part.data_ptr(), P_, C_, 1, nat.stream())

    EINVAL = -1
    for call in (fwd, bwd):
        assert call(x.data_ptr(), gamma.data_ptr(), P, 6) == EINVAL             # C % 4 != 0
        assert call(x.data_ptr(), gamma.data_ptr(), 1, C) == EINVAL             # one value per channel: no variance
        assert call(x.data_ptr(), None, P, C) == EINVAL                         # null gamma
        assert call(x.data_ptr() + 4, gamma.data_ptr(), P, C) == EINVAL         # x not 16-byte aligned
    assert fwd(x.data_ptr(), gamma.data_ptr(), P, C, res=dy.data_ptr(), relu=0) == EINVAL      # a residual without ReLU
    torch.cuda.synchronize()
    for t in (y, dx, dg, db, stats, rm, rv):                                    # nothing was launched
        assert bool((t == 7.0).all())


@pytest.mark.parametrize("case", ["momentum=None", "affine=False", "track_running_stats=False", "nchw", "eval"])
def test_front_end_leaves_other_cases_to_torch_bit_for_bit(case):
    from fastposecnn_amd.lib import backbone, train_conv
    kw = {"momentum=None": dict(momentum=None), "affine=False": dict(affine=False),
          "track_running_stats=False": dict(track_running_stats=False)}.get(case, {})
    g = torch.Generator().manual_seed(11)
    x = torch.randn((2, 64, 6, 5), generator=g) * 1.5 + 0.7
    gy = torch.randn((2, 64, 6, 5), generator=g)
    ours, theirs = backbone.BatchNorm2d(64, **kw).to(DEV), torch.nn.BatchNorm2d(64, **kw).to(DEV)
    theirs.load_state_dict(ours.state_dict())
    if case == "eval":
        ours.eval(); theirs.eval()
    fmt = torch.contiguous_format if case == "nchw" else NHWC
    outs = []
    before = dict(train_conv.counters)
    for m in (ours, theirs):
        xd = x.to(DEV).contiguous(memory_format=fmt).requires_grad_()
        y = m(xd)
        y.backward(gy.to(DEV).contiguous(memory_format=fmt))
        outs.append([y.detach(), xd.grad] + [p.grad for p in m.parameters()] + [b.clone() for b in m.buffers()])
    torch.cuda.synchronize()
    assert train_conv.counters["bn_torch"] == before["bn_torch"] + 1 and train_conv.counters["bn_native"] == before["bn_native"]
    assert len(outs[0]) == len(outs[1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


class _RecordingReLU(torch.nn.Module):
    """The float64 reference's activation: relu(z), or z * masks[i] with the masks of another run; keeps every z."""

    def __init__(self, masks=None):
        super().__init__()
        self.masks, self.seen = masks, []

    def forward(self, z):
        self.seen.append(z.detach())
        return torch.relu(z) if self.masks is None else z * self.masks[len(self.seen) - 1]


def _block(kind):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(5)
    if kind == "basic":
        return bb.BasicBlock(64, 64), (2, 64, 24, 32), 2
    if kind == "basic-down":
        down = torch.nn.Sequential(bb.Conv2d(64, 128, 1, 2, bias=False), bb.BatchNorm2d(128))
        return bb.BasicBlock(64, 128, stride=2, downsample=down), (2, 64, 24, 32), 3
    return bb.Bottleneck(256, 64), (2, 256, 12, 16), 3


@pytest.mark.parametrize("act", ["relu", "softplus"])
@pytest.mark.parametrize("kind", ["basic", "basic-down", "bottleneck"])
def test_blocks_run_their_batchnorms_native_and_match_float64(kind, act, monkeypatch):
    from fastposecnn_amd.lib import train_conv
    block, shape, n_bn = _block(kind)
    g = torch.Generator().manual_seed(9)
    for m in block.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.num_features, generator=g) + 0.5
            m.bias.data = torch.randn(m.num_features, generator=g) * 0.3
    if act == "softplus":
        block.relu = torch.nn.Softplus()
    x = torch.randn(shape, generator=g) * 1.5 + 0.7
    ref = copy.deepcopy(block).double().train()
    if act == "relu":
        ref.relu = _RecordingReLU()
    xr = x.double().requires_grad_()
    yr = ref(xr)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())

    native_out = []
    real = train_conv.batchnorm_act

    def recording(x, bn, res=None, relu=True, **kw):
        y = real(x, bn, res, relu, **kw)
        if y is not None and relu:
            native_out.append(y.detach())
        return y

    monkeypatch.setattr(train_conv, "batchnorm_act", recording)
    block = block.to(DEV).train()
    xd = x.to(DEV).contiguous(memory_format=NHWC).requires_grad_()
    before = dict(train_conv.counters)
    y = block(xd)
    assert train_conv.counters["bn_native"] - before["bn_native"] == n_bn and train_conv.counters["bn_torch"] == before["bn_torch"]
    y.backward(gy.to(DEV).contiguous(memory_format=NHWC))
    torch.cuda.synchronize()

    for (n, b), (_, br) in zip(block.named_buffers(), ref.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1
        else:
            _close(b, br, n, 2e-5)
    safe = torch.ones_like(yr, dtype=torch.bool)
    all_safe = True
    if act == "relu":
        assert len(native_out) == len(ref.relu.seen) == (3 if kind == "bottleneck" else 2)      # every ReLU was fused
        share = sum((z.abs() <= 1e-4).sum().item() for z in ref.relu.seen) / sum(z.numel() for z in ref.relu.seen)
        print("excluded share", share)
        assert share <= 1e-3
        all_safe = share == 0.0
        safe = ref.relu.seen[-1].abs() > 1e-4
    _close(y.detach().cpu().double() * safe, yr.detach() * safe, "y", 2e-5)
    if not all_safe:          # the gradients against float64 run with the native run's ReLU masks
        ref = copy.deepcopy(block).cpu().double().train()
        ref.zero_grad()
        ref.relu = _RecordingReLU([(o.cpu() > 0).double() for o in native_out])
        xr = x.double().requires_grad_()
        ref(xr).backward(gy.double())
    _close(xd.grad, xr.grad, "dx", 1e-4)
    grads, want = dict(block.named_parameters()), dict(ref.named_parameters())
    assert set(grads) == set(want)
    for n in want:
        _close(grads[n].grad, want[n].grad, "d " + n, 1e-4)


def test_model_training_forward_is_native_and_the_engine_repacks_afterwards():
    """ResNet18 PoseRegressor: the training forward runs the encoder's BatchNorm layers native (the stem's too if its
    convolution, the one left to torch, hands over a dense channel-last tensor); the running statistics were then written
    through raw pointers, and an engine plan bound to them BEFORE must repack: evaluation through the engine equals the
    torch modules on the same weights."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet18"
    hp.ENGINE_AUTOTUNE = False
    torch.manual_seed(0)
    model = L.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(DEV)
    x = torch.stack([synth.make_image(i, 96, 128) for i in range(2)]).to(DEV)
    model.eval()
    with torch.no_grad():
        first = {k: v.clone() for k, v in model.pure_model_forward(x).items()}      # the plan now holds the initial statistics
    assert model._engines
    model.train()
    before = dict(train_conv.counters)
    out = model.pure_model_forward(x)
    sum(v.square().mean() for v in out.values()).backward()
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in ("bn_native", "bn_torch")}
    print(used)
    assert used["bn_native"] >= 19 and used["bn_torch"] <= 1 and used["bn_native"] + used["bn_torch"] == 20, used
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.encoder.parameters())
    model.eval()
    with torch.no_grad():
        got = {k: v.clone() for k, v in model.pure_model_forward(x).items()}
        model.HPARAM.USE_NATIVE_ENGINE = False
        want = model.pure_model_forward(x)
    torch.cuda.synchronize()
    moved = 0.0
    for k in want:
        bar = 1e-4 * max(1.0, want[k].abs().max().item())
        assert (got[k] - want[k]).abs().max().item() <= bar, k
        moved = max(moved, (first[k] - want[k]).abs().max().item() / bar)
    assert moved > 10.0, moved           # the step did change what evaluation computes: a stale plan would have missed the bar


def test_frozen_parameters_and_inputs_that_need_no_gradient():
    from fastposecnn_amd import _native as nat
    from fastposecnn_amd.lib import train_conv
    shape = (2, 64, 15, 20)
    x, gy, gamma, beta, _ = _inputs(shape, False)
    bn, ref = _modules(64, gamma, beta)
    gyd = gy.to(DEV).contiguous(memory_format=NHWC)
    # frozen affine parameters: dx as before, no parameter gradients
    frozen = copy.deepcopy(bn).requires_grad_(False)
    xd = x.to(DEV).contiguous(memory_format=NHWC).requires_grad_()
    y = train_conv.batchnorm_act(xd, frozen, relu=True)
    y.backward(gyd)
    torch.cuda.synchronize()
    # the float64 gradients under the native output's ReLU mask (a unit within rounding of 0 may sit on either side)
    xr = x.double().requires_grad_()
    z = ref(xr)
    assert (torch.relu(z) - y.detach().cpu().double()).abs().max().item() <= 2e-5 * max(1.0, z.abs().max().item())
    (z * (y.detach().cpu() > 0).double()).backward(gy.double())
    _close(xd.grad, xr.grad, "dx", 1e-4)
    assert frozen.weight.grad is None and frozen.bias.grad is None
    # an input that needs no gradient: the parameters' gradients alone
    xd = x.to(DEV).contiguous(memory_format=NHWC)
    y2 = train_conv.batchnorm_act(xd, bn, relu=True)
    y2.backward(gyd)
    torch.cuda.synchronize()
    assert xd.grad is None and torch.equal(y2, y)
    _close(bn.weight.grad, ref.weight.grad, "dgamma", 1e-4)
    _close(bn.bias.grad, ref.bias.grad, "dbeta", 1e-4)
    # ... and through the C ABI: without dx and dres only dgamma / dbeta are written
    L = nat.lib()
    P, C = shape[0] * shape[2] * shape[3], 64
    xx = x.double()
    stats = torch.stack([xx.mean((0, 2, 3)), (xx.var((0, 2, 3), unbiased=False) + ref.eps).rsqrt()], 1).float().contiguous().to(DEV)
    part = torch.empty(L.fpc_batchnorm_scratch_floats(P, C), dtype=torch.float32, device=DEV)
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    rc = L.fpc_batchnorm_bwd(xd.data_ptr(), y.data_ptr(), gyd.data_ptr(), bn.weight.data_ptr(), stats.data_ptr(), None, None,
                             dg.data_ptr(), db.data_ptr(), part.data_ptr(), P, C, 1, nat.stream())
    assert rc == 0
    torch.cuda.synchronize()
    _close(dg, ref.weight.grad, "dgamma (C ABI)", 1e-4)
    _close(db, ref.bias.grad, "dbeta (C ABI)", 1e-4)
