"""lib/train_conv.py::_GroupedConv2dFn on the MI355X: the ResNeXt conv2 in training mode on the native grouped kernels, forward
and backward, behind train_conv.NATIVE_GROUPED (FPC_TRAIN_NATIVE_GROUPED=1, off by default).  References: float64
conv2d(groups) autograd; bars as tests/test_gpu_train.py and tests/test_gpu_conv_grouped.py — y and dx within 2e-5 max(1,
|ref|max), dw (and db, a sum over as many pixels) within 1e-4 max(1, |ref|max)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ENC = "resnext50_32x4d"
NEW_KEYS = ("grouped_fwd_native", "grouped_dgrad_native", "grouped_wgrad_native")


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


def _close(a, ref, tol):
    return (a.detach().double().cpu() - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


def _module_step(dev, conv, x0, seed=4):
    """One forward / backward of `conv` on the GPU and of float64 conv2d on the CPU with the same upstream gradient."""
    x = x0.to(dev).requires_grad_(True)
    y = conv(x)
    gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed))
    conv.zero_grad(set_to_none=True)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    xr = x0.double().requires_grad_(True)
    wr = conv.weight.detach().double().cpu().requires_grad_(True)
    br = None if conv.bias is None else conv.bias.detach().double().cpu().requires_grad_(True)
    yr = F.conv2d(xr, wr, br, conv.stride, conv.padding, conv.dilation, conv.groups)
    yr.backward(gy.double())
    return (y, x.grad, conv.weight.grad, None if conv.bias is None else conv.bias.grad), (yr.detach(), xr.grad, wr.grad, None if br is None else br.grad)


def _check(got, ref):
    y, gx, gw, gb = got
    yr, gxr, gwr, gbr = ref
    assert _close(y, yr, 2e-5) and _close(gx, gxr, 2e-5) and _close(gw, gwr, 1e-4)
    if gbr is not None:
        assert _close(gb, gbr, 1e-4)


@pytest.mark.parametrize("stride,bias", [(1, False), (2, False), (1, True), (2, True)])
def test_switch_on_runs_native(lib, dev, monkeypatch, stride, bias):
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", True)
    torch.manual_seed(2)
    c = bb.Conv2d(128, 128, 3, stride, 1, groups=32, bias=bias).to(dev).train()
    x0 = torch.randn(2, 128, 9, 12, generator=torch.Generator().manual_seed(1))
    before = dict(train_conv.counters)
    got, ref = _module_step(dev, c, x0)
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert all(used[k] == 1 for k in NEW_KEYS), used
    assert all(v == 0 for k, v in used.items() if k not in NEW_KEYS), used
    assert got[0].is_contiguous(memory_format=torch.channels_last) and got[0].stride(1) == 1
    assert got[1].shape == x0.shape
    _check(got, ref)


def test_switch_off_moves_no_new_key(lib, dev, monkeypatch):
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", False)
    torch.manual_seed(2)
    c = bb.Conv2d(128, 128, 3, 1, 1, groups=32, bias=False).to(dev).train()
    x0 = torch.randn(2, 128, 9, 12, generator=torch.Generator().manual_seed(1))
    before = dict(train_conv.counters)
    got, ref = _module_step(dev, c, x0)
    assert dict(train_conv.counters) == before
    _check(got, ref)


@pytest.mark.parametrize("what", ["dilation2", "kernel5", "cg2"])
def test_fallbacks_with_the_switch_on(lib, dev, monkeypatch, what):
    """Outside the kernels' class the module is torch's convolution: no counter moves and the gradients are right."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", True)
    torch.manual_seed(3)
    if what == "dilation2":
        c = bb.Conv2d(128, 128, 3, 1, 2, dilation=2, groups=32, bias=False)
    elif what == "kernel5":
        c = bb.Conv2d(128, 128, 5, 1, 2, groups=32, bias=False)
    else:
        c = bb.Conv2d(128, 128, 3, 1, 1, groups=64, bias=False)
    c = c.to(dev).train()
    x0 = torch.randn(2, 128, 9, 12, generator=torch.Generator().manual_seed(1))
    before = dict(train_conv.counters)
    got, ref = _module_step(dev, c, x0)
    assert dict(train_conv.counters) == before
    y, gx, gw, _ = got
    # torch's own f32 kernels (MIOpen picks the algorithm), not the project's: held to the model-level 1e-4, not the kernels' 2e-5
    assert _close(y, ref[0], 1e-4) and _close(gx, ref[1], 1e-4) and _close(gw, ref[2], 1e-4)


def test_registered_grad_sink(lib, dev, monkeypatch):
    """A GradSink registered for the weight: the kernel writes its view, autograd gets no weight gradient, `written` is set and
    the callback fires; a second use of the weight in the same step returns its gradient the ordinary way."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", True)
    g = torch.Generator().manual_seed(9)
    w = (torch.randn((128, 4, 3, 3), generator=g) / 6).to(dev).requires_grad_(True)
    x0 = torch.randn(2, 128, 9, 12, generator=g)
    gy0 = torch.randn(2, 128, 9, 12, generator=g)
    view = torch.full((128, 4, 3, 3), float("nan"), device=dev)
    fired = []

    class Owner:
        pass
    owner = Owner()
    sink = train_conv.GradSink(view, lambda: fired.append(1), owner)
    monkeypatch.setitem(train_conv.grad_sinks, w.data_ptr(), sink)
    wr = w.detach().double().cpu().requires_grad_(True)
    F.conv2d(x0.double(), wr, None, 1, 1, 1, 32).backward(gy0.double())

    before = dict(train_conv.counters)
    y = train_conv.conv2d(x0.to(dev), w, None, 1, 1, 32)
    y.backward(gy0.to(dev))
    torch.cuda.synchronize()
    assert w.grad is None                      # nothing was returned for autograd to accumulate
    assert sink.written and fired == [1]
    assert _close(view, wr.grad, 1e-4)
    assert train_conv.counters["grouped_wgrad_native"] == before["grouped_wgrad_native"] + 1

    y = train_conv.conv2d(x0.to(dev), w, None, 1, 1, 32)      # the same step, the sink already written
    y.backward(gy0.to(dev))
    torch.cuda.synchronize()
    assert fired == [1] and w.grad is not None and _close(w.grad, wr.grad, 1e-4)
    assert _close(view, wr.grad, 1e-4)        # ... and its view was left alone


def test_training_step_native_grouped_vs_torch(lib, dev, monkeypatch):
    """tests/test_gpu_resnext.py::test_training_step_native_vs_torch with the switch on: forward + backward of the ResNeXt-50 model
    in training mode at B = 1, 64 x 96 (maps down to 2 x 3, all border) against the same model on torch's f32 kernels, each against
    float64; the 16 grouped convolutions run native forward, data gradient and weight gradient.

    Bars, those of test_training_step_native_vs_torch: loss within 1e-5, outputs within 1e-4, and over the parameter gradients
    err_native <= max(2 err_torch32, 1e-4), each error relative to the gradient's largest magnitude.

    The dense convolutions' plans are pinned for this test (the planner's heuristic tiling on plain f32 products, code 0, for every
    shape): what train_conv times and picks on a first call depends on that run's timings and on which tests filled the cache
    before, and at 64 x 96 layer4's BatchNorm, over 6 pixels, amplifies whatever rounding reaches it, so with tuned plans the same
    comparison moves from run to run (DESIGN.md 4.2a'').  The grouped path under test has one form and is not affected."""
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_GROUPED", True)

    class PinnedPlans(dict):
        def get(self, key, default=None):      # conv_nhwc asks with .get(key): no candidate is timed, none is remembered
            return 0
    monkeypatch.setattr(train_conv, "_plan_cache", PinnedPlans())
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = ENC
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if isinstance(child, torch.nn.ReLU):
                setattr(mod, name, torch.nn.Softplus())
    grouped = sum(1 for mod in model.modules() if isinstance(mod, torch.nn.Conv2d) and mod.groups > 1)
    assert grouped == 16
    x = synth.make_image(0, 64, 96)[None].to(dev)
    res = {}
    for tag in ("native", "torch32", "torch64"):
        monkeypatch.setattr(train_conv, "ENABLED", tag == "native")
        if tag == "torch64":
            model = model.double()
            x = x.double()
        model.zero_grad(set_to_none=True)
        before = dict(train_conv.counters)
        out = model.pure_model_forward(x)
        loss = sum(v.square().mean() for v in out.values())
        loss.backward()
        torch.cuda.synchronize()
        used = {k: train_conv.counters[k] - before[k] for k in before}
        res[tag] = (loss.item(), {k: v.detach().double() for k, v in out.items()},
                    {n: p.grad.detach().double() for n, p in model.named_parameters() if p.grad is not None}, used)
    ln, on, gn, used = res["native"]
    lt, ot, gt, unused = res["torch32"]
    lr, orf, gr, _ = res["torch64"]
    assert [used[k] for k in NEW_KEYS] == [16, 16, 16], used
    assert all(unused[k] == 0 for k in NEW_KEYS) and unused["fwd_native"] == 0, unused
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    assert set(gn) == set(gr)
    err_n = err_t = 0.0
    worst = []
    for n in gr:
        scale = max(gr[n].abs().max().item(), 1e-12)
        en, et = (gn[n] - gr[n]).abs().max().item() / scale, (gt[n] - gr[n]).abs().max().item() / scale
        worst.append((en, et, n))
        err_n = max(err_n, en)
        err_t = max(err_t, et)
    print(f"err native {err_n:.3e} torch32 {err_t:.3e}; the worst native ones (native, torch32, name): {sorted(worst, reverse=True)[:4]}")
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)
