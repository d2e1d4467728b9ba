"""The MobileNetV2 encoder's training step on the native depthwise kernels (csrc/depthwise.hip) and with ReLU6 as an activation
of the native BatchNorm (csrc/batchnorm.hip: fpc_batchnorm_act_fwd / _bwd), behind FPC_TRAIN_NATIVE_MBV2: the kernels against the
float64 references of _dwconv_train_refs (which tests/test_dwconv_train_host.py shows to be float64 autograd), the front end
lib/train_conv.conv2d / batchnorm_act(relu6=True), two InvertedResidual blocks and the model.  Bars: dx and y within
2e-5 max(1, |ref|max) of float64, weight and parameter gradients within 1e-4 max(1, |ref|max); outputs in NaN-filled buffers between
64-float canaries, every launch twice and bit-identical."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _dwconv_train_refs as R

pytestmark = pytest.mark.gpu

NHWC = torch.channels_last
NEW_KEYS = ("dw_fwd_native", "dw_dgrad_native", "dw_wgrad_native")


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


@pytest.fixture
def mbv2_on(monkeypatch):
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "ENABLED", True)
    monkeypatch.setattr(train_conv, "NATIVE_MBV2", True)
    return train_conv


def _twice(dev, n, launch):
    """Two launches into fresh NaN-filled buffers with 64-float canaries around the n outputs: the canaries intact, nothing left
    unwritten, both runs the same bits.  Returns the first run's outputs (CPU, flat)."""
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), float("nan"), device=dev)
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        assert launch(y.data_ptr()) == 0
        torch.cuda.synchronize()
        host = buf.cpu()
        assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary was overwritten"
        outs.append(host[64:64 + n])
    assert not torch.isnan(outs[0]).any(), "unwritten outputs"
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def _bar(out, ref, what, rel):
    err = (out.detach().double().cpu() - ref).abs().max().item()
    bar = rel * max(1.0, ref.abs().max().item())
    print(f"{what}: err {err:.3e} bar {bar:.3e}")
    assert err <= bar, (what, err, bar)


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev)


def _dgrad(dev, case, dy, w):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Hi, Wi, C, s = case
    dyd, wd = _nhwc(dy, dev), w.to(dev)
    out = _twice(dev, B * Hi * Wi * C, lambda p: L.fpc_dwconv3x3_dgrad(dyd.data_ptr(), wd.data_ptr(), p, B, Hi, Wi, C, s, nat.stream()))
    return out.view(B, Hi, Wi, C).permute(0, 3, 1, 2)


def _wgrad(dev, case, x, dy):
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, Hi, Wi, C, s = case
    Ho, Wo = R.out_hw(Hi, Wi, s)
    xd, dyd = _nhwc(x, dev), _nhwc(dy, dev)
    need = L.fpc_dwconv3x3_wgrad_workspace_bytes(B, Ho, Wo, C)
    assert need == R.wgrad_slices(B, Ho, Wo, C) * C * 36
    ws = torch.full((need // 4 + 64,), float("nan"), device=dev)      # (the partials are all written before they are read)
    assert ws.data_ptr() % 256 == 0
    out = _twice(dev, C * 9, lambda p: L.fpc_dwconv3x3_wgrad(xd.data_ptr(), dyd.data_ptr(), p, B, Hi, Wi, C, s, ws.data_ptr(), need,
                                                             nat.stream()))
    assert torch.isnan(ws[need // 4:]).all(), "the workspace was written past its size"
    return out.view(C, 1, 3, 3)


@pytest.mark.parametrize("case", R.CASES, ids=R.ids(R.CASES))
def test_dgrad_vs_float64(lib, dev, case):
    B, Hi, Wi, C, s = case
    x, w, dy = R.operands(case)
    dx = _dgrad(dev, case, dy, w)
    _bar(dx, R.dgrad_ref(dy, w, Hi, Wi, s), f"dgrad {case}", 2e-5)
    # whole numbers in [-4, 4]: every product and partial sum is exact in f32, so the kernel agrees with float64 bit for bit
    x, w, dy = R.operands(case, integer=True)
    assert torch.equal(_dgrad(dev, case, dy, w).double(), R.dgrad_ref(dy, w, Hi, Wi, s))
    # channels do not mix: dy in one channel only
    x, w, dy = R.operands(case)
    ch = C // 2 + 1
    one = torch.zeros_like(dy)
    one[:, ch] = dy[:, ch]
    dx = _dgrad(dev, case, one, w)
    _bar(dx, R.dgrad_ref(one, w, Hi, Wi, s), "one channel", 2e-5)
    other = torch.ones(C, dtype=torch.bool)
    other[ch] = False
    assert (dx[:, other] == 0).all() and (dx[:, ch] != 0).any()


@pytest.mark.parametrize("case", R.CASES_ALL, ids=R.ids(R.CASES_ALL))
def test_wgrad_vs_float64(lib, dev, case):
    B, Hi, Wi, C, s = case
    x, w, dy = R.operands(case)
    dw = _wgrad(dev, case, x, dy)
    _bar(dw, R.wgrad_ref(x, dy, s), f"wgrad {case}", 1e-4)
    x, w, dy = R.operands(case, integer=True)
    dw = _wgrad(dev, case, x, dy)
    assert torch.equal(dw.double(), R.wgrad_ref(x, dy, s))
    if (Hi, Wi) == (1, 1):      # the eight taps no pixel reaches: exact zeros, the centre is not
        flat = dw.view(C, 9)
        assert (flat[:, [0, 1, 2, 3, 5, 6, 7, 8]] == 0).all() and (flat[:, 4] != 0).any()
    x, w, dy = R.operands(case)
    ch = C // 2 + 1
    one = torch.zeros_like(dy)
    one[:, ch] = dy[:, ch]
    dw = _wgrad(dev, case, x, one)
    _bar(dw, R.wgrad_ref(x, one, s), "one channel", 1e-4)
    other = torch.ones(C, dtype=torch.bool)
    other[ch] = False
    assert (dw[other] == 0).all() and (dw[ch] != 0).any()


# ---- BatchNorm + ReLU6 through the C ABI -------------------------------------------------------------------------------------------

def _bn_call(dev, shape, x, gy, gamma, beta, act, entry):
    """forward + backward of fpc_batchnorm_act_* (entry "act") or fpc_batchnorm_* (entry "old") -> dict of CPU tensors"""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    B, C, H, W = shape
    P = B * H * W
    xd, gyd = _nhwc(x, dev), _nhwc(gy, dev)
    g, b = gamma.to(dev), beta.to(dev)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    bufs = [torch.full((P * C + 128,), float("nan"), device=dev) for _ in range(2)]      # 64-float canaries around y and dx
    y, dx = bufs[0][64:64 + P * C], bufs[1][64:64 + P * C]
    stats, dgb = torch.empty((C, 2), device=dev), torch.empty((2, C), device=dev)
    part = torch.empty(L.fpc_batchnorm_scratch_floats(P, C), device=dev)
    fwd, bwd = (L.fpc_batchnorm_act_fwd, L.fpc_batchnorm_act_bwd) if entry == "act" else (L.fpc_batchnorm_fwd, L.fpc_batchnorm_bwd)
    assert fwd(xd.data_ptr(), None, g.data_ptr(), b.data_ptr(), rm.data_ptr(), rv.data_ptr(), y.data_ptr(), stats.data_ptr(), part.data_ptr(),
               P, C, 1e-5, 0.1, act, nat.stream()) == 0
    assert bwd(xd.data_ptr(), y.data_ptr(), gyd.data_ptr(), g.data_ptr(), stats.data_ptr(), dx.data_ptr(), None, dgb.data_ptr(),
               dgb.data_ptr() + 4 * C, part.data_ptr(), P, C, act, nat.stream()) == 0
    torch.cuda.synchronize()
    for buf in bufs:
        assert torch.isnan(buf[:64]).all() and torch.isnan(buf[64 + P * C:]).all(), "a canary was overwritten"
        assert not torch.isnan(buf[64:64 + P * C]).any(), "unwritten outputs"
    to_nchw = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2).cpu()
    return {"y": to_nchw(y), "dx": to_nchw(dx), "dgamma": dgb[0].cpu(), "dbeta": dgb[1].cpu(), "rm": rm.cpu(), "rv": rv.cpu(), "stats": stats.cpu()}


@pytest.mark.parametrize("index", range(len(R.RELU6_SHAPES)), ids=[str(s) for s in R.RELU6_SHAPES])
def test_batchnorm_relu6_vs_float64(lib, dev, index):
    shape = R.RELU6_SHAPES[index]
    B, C, H, W = shape
    x, gy, gamma, beta = R.relu6_operands(index, shape)
    got = _bn_call(dev, shape, x, gy, gamma, beta, 2, "act")
    again = _bn_call(dev, shape, x, gy, gamma, beta, 2, "act")
    for k in got:
        assert torch.equal(got[k], again[k]), k
    ref = torch.nn.BatchNorm2d(C).double()
    ref.weight.data, ref.bias.data = gamma.double(), beta.double()
    xr = x.double().requires_grad_()
    z = ref(xr)
    yr = F.relu6(z)
    yr.backward(gy.double())
    y = got["y"]
    assert (y == 0).any() and (y == 6).any() and y.min() >= 0 and y.max() <= 6
    _bar(got["rm"], ref.running_mean, "running_mean", 2e-5)
    _bar(got["rv"], ref.running_var, "running_var", 2e-5)
    zd = z.detach()
    safe = (zd.abs() > 1e-4) & ((zd - 6).abs() > 1e-4)
    excluded = 1.0 - safe.double().mean().item()
    print("excluded share", excluded, "elements", int((~safe).sum()))
    assert excluded <= 1e-3
    _bar(y.double() * safe, yr.detach() * safe, "y", 2e-5)
    mask = ((y > 0) & (y < 6)).double()
    assert torch.equal(mask * safe, ((zd > 0) & (zd < 6)).double() * safe)      # the native mask is float64's away from the kinks
    want = {"dx": xr.grad, "dgamma": ref.weight.grad, "dbeta": ref.bias.grad}
    if not bool(safe.all()):      # a flipped unit changes its channel's sums: float64 with the native mask instead
        xr2, w2, b2 = x.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
        z2 = F.batch_norm(xr2, None, None, w2, b2, True, 0.1, 1e-5)
        (z2 * mask).backward(gy.double())
        want = {"dx": xr2.grad, "dgamma": w2.grad, "dbeta": b2.grad}
    _bar(got["dx"].double() * safe, want["dx"] * safe, "dx", 2e-5)
    _bar(got["dgamma"], want["dgamma"], "dgamma", 1e-4)
    _bar(got["dbeta"], want["dbeta"], "dbeta", 1e-4)


@pytest.mark.parametrize("act", [0, 1])
def test_batchnorm_act_0_and_1_are_the_old_entries_bit_for_bit(lib, dev, act):
    shape = R.RELU6_SHAPES[2]
    x, gy, gamma, beta = R.relu6_operands(2, shape)
    new, old = _bn_call(dev, shape, x, gy, gamma, beta, act, "act"), _bn_call(dev, shape, x, gy, gamma, beta, act, "old")
    for k in new:
        assert torch.equal(new[k], old[k]), k
    assert (new["y"] > 6).any() and ((new["y"] < 0).any() if act == 0 else (new["y"] == 0).any())


# ---- the front end -----------------------------------------------------------------------------------------------------------------

def _conv_step(tc, dev, x0, w0, gy0, stride, pad=1, groups=None, bias=None, grad=True):
    x = x0.to(dev).contiguous(memory_format=NHWC).requires_grad_(grad)
    w = w0.to(dev).requires_grad_(grad)
    b = None if bias is None else bias.to(dev).requires_grad_(grad)
    y = tc.conv2d(x, w, b, stride, pad, x0.shape[1] if groups is None else groups)
    if grad and torch.is_grad_enabled():
        y.backward(gy0.to(dev).contiguous(memory_format=NHWC))
    torch.cuda.synchronize()
    return y, x.grad, w.grad


@pytest.mark.parametrize("stride", [1, 2])
def test_conv2d_runs_the_depthwise_call_native(lib, dev, mbv2_on, stride):
    tc = mbv2_on
    g = torch.Generator().manual_seed(40 + stride)
    x0, w0 = torch.randn((2, 48, 9, 11), generator=g), torch.randn((48, 1, 3, 3), generator=g) / 3
    gy0 = torch.randn((2, 48, *R.out_hw(9, 11, stride)), generator=g)
    yr, dxr, dwr = R.autograd_ref(x0, w0, gy0, stride)
    before = dict(tc.counters)
    y, dx, dw = _conv_step(tc, dev, x0, w0, gy0, stride)
    used = {k: tc.counters[k] - before[k] for k in before}
    assert all(used[k] == 1 for k in NEW_KEYS) and all(v == 0 for k, v in used.items() if k not in NEW_KEYS), used
    assert y.grad_fn.__class__.__name__ == "_DepthwiseConv2dFnBackward"
    assert y.is_contiguous(memory_format=NHWC) and dx.is_contiguous(memory_format=NHWC) and dw.shape == w0.shape
    _bar(y, yr, "y", 2e-5); _bar(dx, dxr, "dx", 2e-5); _bar(dw, dwr, "dw", 1e-4)
    mbv2_on.NATIVE_MBV2 = False                  # torch's f32 kernels on the same call
    before = dict(tc.counters)
    yt, dxt, dwt = _conv_step(tc, dev, x0, w0, gy0, stride)
    assert dict(tc.counters) == before and yt.grad_fn.__class__.__name__ != "_DepthwiseConv2dFnBackward"
    _bar(y, yt.double().cpu(), "y vs torch f32", 2e-5); _bar(dx, dxt.double().cpu(), "dx vs torch f32", 2e-5)
    _bar(dw, dwt.double().cpu(), "dw vs torch f32", 1e-4)
    # only what needs_input_grad asks for: a frozen weight, an input without gradient
    mbv2_on.NATIVE_MBV2 = True
    before = dict(tc.counters)
    x = x0.to(dev).contiguous(memory_format=NHWC).requires_grad_(True)
    tc.conv2d(x, w0.to(dev), None, stride, 1, 48).backward(gy0.to(dev))
    w = w0.to(dev).requires_grad_(True)
    tc.conv2d(x0.to(dev), w, None, stride, 1, 48).backward(gy0.to(dev))
    torch.cuda.synchronize()
    used = {k: tc.counters[k] - before[k] for k in NEW_KEYS}
    assert used == {"dw_fwd_native": 2, "dw_dgrad_native": 1, "dw_wgrad_native": 1}, used
    assert torch.equal(x.grad, dx) and torch.equal(w.grad, dw)


@pytest.mark.parametrize("kind", ["good", "written", "offset", "shape"])
def test_weight_gradient_sink(lib, dev, mbv2_on, monkeypatch, kind):
    """_take_sink(w, aligned=True) / _commit_sink as _GroupedConv2dFn: a good sink is written in place and autograd gets None; one
    already written, one whose view is 4 bytes off a 16-byte boundary and one of another shape are left alone."""
    tc = mbv2_on
    g = torch.Generator().manual_seed(9)
    x0, w0, gy0 = torch.randn((2, 32, 6, 7), generator=g), torch.randn((32, 1, 3, 3), generator=g) / 3, torch.randn((2, 32, 6, 7), generator=g)
    w = w0.to(dev).requires_grad_(True)
    shape = tuple(w.shape)
    if kind == "shape":
        view = torch.zeros(shape[:-1] + (shape[-1] + 1,), device=dev)
    elif kind == "offset":
        view = torch.zeros(w.numel() + 4, device=dev)[1:1 + w.numel()].view(shape)
    else:
        view = torch.zeros(shape, device=dev)
    fired = []

    class Owner:
        pass
    owner = Owner()
    sink = tc.GradSink(view, lambda: fired.append(1), owner)
    sink.written = kind == "written"
    monkeypatch.setitem(tc.grad_sinks, w.data_ptr(), sink)
    before = dict(tc.counters)
    y = tc.conv2d(x0.to(dev).contiguous(memory_format=NHWC), w, None, 1, 1, 32)
    y.backward(gy0.to(dev))
    torch.cuda.synchronize()
    assert tc.counters["dw_wgrad_native"] == before["dw_wgrad_native"] + 1
    dwr = R.wgrad_ref(x0, gy0, 1)
    taken = kind == "good"
    assert sink.written == (taken or kind == "written") and (w.grad is None) == taken and len(fired) == int(taken)
    assert w.data_ptr() in tc.grad_sinks
    if taken:
        _bar(view, dwr, "dw in the sink", 1e-4)
    else:
        assert (view == 0).all()
        _bar(w.grad, dwr, "dw", 1e-4)


REFUSED = ["bias", "pad0", "stride3", "kernel5", "groups_half", "float64", "C6", "empty", "no_grad", "switch_off", "enabled_off"]


@pytest.mark.parametrize("term", REFUSED)
def test_each_gate_term_refuses_and_torch_runs_bit_for_bit(lib, dev, mbv2_on, term):
    tc = mbv2_on
    C, B, k, stride, pad, groups, dtype = 32, 2, 3, 1, 1, None, torch.float32
    g = torch.Generator().manual_seed(3)
    if term == "C6":
        C = 6
    if term == "empty":
        B = 0
    if term == "kernel5":
        k, pad = 5, 2
    if term == "pad0":
        pad = 0
    if term == "stride3":
        stride = 3
    if term == "float64":
        dtype = torch.float64
    groups = C // 2 if term == "groups_half" else C
    x0 = torch.randn((B, C, 9, 8), generator=g).to(dtype)
    w0 = (torch.randn((C, C // groups, k, k), generator=g) / 3).to(dtype)
    bias = torch.randn(C, generator=g).to(dtype) if term == "bias" else None
    if term == "switch_off":
        tc.NATIVE_MBV2 = False
    if term == "enabled_off":
        tc.ENABLED = False
    xd = x0.to(dev).contiguous(memory_format=NHWC)
    assert not tc._depthwise_ok(xd, w0.to(dev), None if bias is None else bias.to(dev), stride, pad, groups) or term == "no_grad"
    want_y = F.conv2d(xd, w0.to(dev), None if bias is None else bias.to(dev), stride, pad, 1, groups)
    gy0 = torch.randn(want_y.shape, generator=g).to(dtype)
    before = dict(tc.counters)
    if term == "no_grad":
        with torch.no_grad():
            assert not tc._depthwise_ok(xd, w0.to(dev), None, stride, pad, groups)
            y, _, _ = _conv_step(tc, dev, x0, w0, gy0, stride, pad, groups, bias, grad=False)
        assert y.grad_fn is None and torch.equal(y, want_y)
        assert dict(tc.counters) == before
        return
    y, dx, dw = _conv_step(tc, dev, x0, w0, gy0, stride, pad, groups, bias)
    assert dict(tc.counters) == before
    assert "Depthwise" not in y.grad_fn.__class__.__name__
    xr, wr = xd.clone().requires_grad_(True), w0.to(dev).requires_grad_(True)
    br = None if bias is None else bias.to(dev).requires_grad_(True)
    yr = F.conv2d(xr, wr, br, stride, pad, 1, groups)
    yr.backward(gy0.to(dev).contiguous(memory_format=NHWC))
    torch.cuda.synchronize()
    assert torch.equal(y, yr)
    if B:      # the gradients are torch's kernels on both sides (its weight-gradient kernels are not all deterministic: a bar, not bits)
        _bar(dx, xr.grad.double().cpu(), "dx", 2e-5)
        _bar(dw, wr.grad.double().cpu(), "dw", 1e-4)


# ---- two blocks ---------------------------------------------------------------------------------------------------------------------

class _RecordingReLU6(torch.nn.Module):
    """The float64 reference's activation: relu6(z), or z * masks[i] + 6 * tops[i] with the masks of another run; keeps every z."""

    def __init__(self, masks=None):
        super().__init__()
        self.masks, self.seen = masks, []

    def forward(self, z):
        self.seen.append(z.detach())
        if self.masks is None:
            return F.relu6(z)
        m, top = self.masks[len(self.seen) - 1]
        return z * m + 6.0 * top


@pytest.mark.parametrize("spec", [(32, 32, 1, 6), (32, 64, 2, 6)], ids=str)
def test_inverted_residual_block_fuses_relu6_and_matches_float64(lib, dev, mbv2_on, monkeypatch, spec):
    from fastposecnn_amd.lib import backbone as bb
    tc = mbv2_on
    monkeypatch.setattr(tc, "NATIVE_BN", True)
    torch.manual_seed(5)
    block = bb.InvertedResidual(*spec)
    g = torch.Generator().manual_seed(9)
    for m in block.modules():
        if isinstance(m, torch.nn.BatchNorm2d):      # pre-activations that reach both clamps
            m.weight.data = 3.0 * (torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.data = 3.0 + torch.randn(m.num_features, generator=g)
    x = torch.randn((2, 32, 9, 11), generator=g) * 1.5 + 0.7

    def f64_block(masks=None):
        ref = copy.deepcopy(block).cpu().double().train()
        ref.zero_grad()
        acts = [_RecordingReLU6(None if masks is None else [masks[i]]) for i in range(2)]
        ref.conv[0][2], ref.conv[1][2] = acts
        return ref, acts

    ref, acts = f64_block()
    xr = x.double().requires_grad_()
    yr = ref(xr)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())

    native_out = []
    real = tc.batchnorm_act

    def recording(x, bn, res=None, relu=True, **kw):
        y = real(x, bn, res, relu, **kw)
        if y is not None and kw.get("relu6"):
            native_out.append(y.detach())
        return y

    monkeypatch.setattr(tc, "batchnorm_act", recording)
    block = block.to(dev).train()
    xd = x.to(dev).contiguous(memory_format=NHWC).requires_grad_()
    before = dict(tc.counters)
    y = block(xd)
    used = {k: tc.counters[k] - before[k] for k in before}
    assert used["bn_relu6_native"] == 2 and used["bn_native"] == 3 and used["bn_torch"] == 0 and used["dw_fwd_native"] == 1, used
    y.backward(gy.to(dev).contiguous(memory_format=NHWC))
    torch.cuda.synchronize()
    used = {k: tc.counters[k] - before[k] for k in before}
    assert used["dw_dgrad_native"] == 1 and used["dw_wgrad_native"] == 1, used
    assert len(native_out) == 2 and all((o == 0).any() and (o == 6).any() for o in native_out)

    for (n, b), (_, br) in zip(block.named_buffers(), ref.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == 1
        else:
            _bar(b, br, n, 2e-5)
    seen = [a.seen[0] for a in acts]
    near = [(z.abs() <= 1e-4) | ((z - 6).abs() <= 1e-4) for z in seen]
    share = sum(n.sum().item() for n in near) / sum(z.numel() for z in seen)
    print("excluded share", share)
    assert share <= 1e-3
    # (ReLU6 is continuous: a hidden unit that lands on the other side of a kink moves y by no more than its own rounding, and the
    # block's output has no activation behind it — nothing to leave out of y; the masks matter to the gradients alone)
    _bar(y, yr.detach(), "y", 2e-5)
    if share > 0.0:      # the gradients against float64 run with the native run's masks
        masks = [(((o > 0) & (o < 6)).double().cpu(), (o >= 6).double().cpu()) for o in native_out]
        ref, _ = f64_block(masks)
        xr = x.double().requires_grad_()
        ref(xr).backward(gy.double())
    _bar(xd.grad, xr.grad, "dx", 1e-4)
    grads, want = dict(block.named_parameters()), dict(ref.named_parameters())
    assert set(grads) == set(want)
    for n in want:
        _bar(grads[n].grad, want[n].grad, "d " + n, 1e-4)


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def _model(lib, dev, softplus):
    from fastposecnn_amd import config
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "mobilenet_v2"
    hp.ENGINE_AUTOTUNE = False
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
        for name, child in list(mod.named_children()):
            if softplus and isinstance(child, (torch.nn.ReLU, torch.nn.ReLU6)):
                setattr(mod, name, torch.nn.Softplus())
    return model


def test_training_step_native_depthwise_vs_torch(lib, dev, mbv2_on, monkeypatch):
    """tests/test_gpu_mobilenet_v2.py::test_training_step_native_vs_torch with the switch on: the 17 depthwise convolutions run
    native forward, data gradient and weight gradient; its bars (loss 1e-5, outputs 1e-4, err_native <= max(2 err_torch, 1e-4) over
    the parameter gradients, its zero-gradient biases against their BatchNorm's weight gradient).  The dense convolutions' plans are
    pinned to the planner's heuristic tiling on plain f32 products (code 0), as tests/test_gpu_grouped_train_fn.py does: no
    candidate is timed, and the comparison does not depend on which tests filled the plan cache before; the depthwise path under
    test has one form."""
    from fastposecnn_amd import synth
    from test_gpu_mobilenet_v2 import _zero_grad_biases
    tc = mbv2_on

    class PinnedPlans(dict):
        def get(self, key, default=None):      # conv_nhwc asks with .get(key): nothing is timed, nothing is remembered
            return 0
    monkeypatch.setattr(tc, "_plan_cache", PinnedPlans())
    model = _model(lib, dev, softplus=True)
    x = torch.stack([synth.make_image(i, 64, 64) for i in range(2)]).to(dev)
    res = {}
    for tag in ("native", "torch32", "torch64"):
        tc.ENABLED = tag == "native"
        if tag == "torch64":
            model = model.double()
            x = x.double()
        model.zero_grad(set_to_none=True)
        before = dict(tc.counters)
        out = model.pure_model_forward(x)
        loss = sum(v.square().mean() for v in out.values())
        loss.backward()
        torch.cuda.synchronize()
        used = {k: tc.counters[k] - before[k] for k in before}
        res[tag] = (loss.item(), {k: v.detach().double() for k, v in out.items()},
                    {n: p.grad.detach().double() for n, p in model.named_parameters() if p.grad is not None}, used)
    ln, on, gn, used = res["native"]
    lt, ot, gt, unused = res["torch32"]
    lr, orf, gr, _ = res["torch64"]
    print("counters", used)
    assert [used[k] for k in NEW_KEYS] == [17, 17, 17], used
    assert all(unused[k] == 0 for k in NEW_KEYS) and unused["fwd_native"] == 0, unused
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        assert (on[k] - orf[k]).abs().max().item() <= 1e-4 * max(1.0, orf[k].abs().max().item()), k
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert set(gn) == set(gr) == set(names)
    assert sum(n.startswith("encoder.") for n in names) == 156
    zero_grad = _zero_grad_biases(model.encoder)
    err_n = err_t = 0.0
    worst = None
    for n in gr:
        ref_n = n
        if n in zero_grad:
            ref_n = n[:-len("bias")] + "weight"
            assert gr[n].abs().max().item() <= 1e-9 * gr[ref_n].abs().max().item(), n
        scale = max(gr[ref_n].abs().max().item(), 1e-12)
        e = (gn[n] - gr[n]).abs().max().item() / scale
        if e > err_n:
            worst = (n, scale)
        err_n = max(err_n, e)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    print("err native", err_n, "torch", err_t, "worst", worst)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)


def test_model_forward_fuses_every_relu6_and_the_engine_plan_follows(lib, dev, mbv2_on, monkeypatch):
    """Real ReLU6, both switches: 35 fused BatchNorms in the forward, every output within 1e-4 max(1, |ref|) of the float64 module;
    and after one optimiser-free step (the running statistics moved through raw pointers) the engine plan built from the module
    equals the plan of a copy that took the same step with the switches off."""
    from fastposecnn_amd import synth
    tc = mbv2_on
    monkeypatch.setattr(tc, "NATIVE_BN", True)
    model = _model(lib, dev, softplus=False)
    twin = copy.deepcopy(model)
    ref = copy.deepcopy(model).double()
    initial = {n: b.detach().clone() for n, b in model.named_buffers()}
    x = torch.stack([synth.make_image(i, 64, 64) for i in range(2)]).to(dev)
    before = dict(tc.counters)
    out = model.pure_model_forward(x)
    torch.cuda.synchronize()
    used = {k: tc.counters[k] - before[k] for k in before}
    print("counters", used)
    assert used["bn_relu6_native"] == 35 and used["dw_fwd_native"] == 17 and used["bn_torch"] == 0, used
    tc.ENABLED = False
    want = ref.pure_model_forward(x.double())
    for k in want:
        err = (out[k].detach().double() - want[k].detach()).abs().max().item()
        bar = 1e-4 * max(1.0, want[k].detach().abs().max().item())
        print(k, "err", err, "bar", bar)
        assert err <= bar, k
    # (c) the same step with the switches off, then the plans: parameters did not move (no optimiser), the running statistics did
    tc.ENABLED = True
    tc.NATIVE_MBV2 = False
    monkeypatch.setattr(tc, "NATIVE_BN", False)
    twin.pure_model_forward(x)
    torch.cuda.synchronize()
    moved = 0.0
    for (n, b), (_, bt) in zip(model.named_buffers(), twin.named_buffers()):
        if n.endswith("num_batches_tracked"):
            assert int(b) == int(bt) == 1
        elif n.startswith("encoder."):
            assert (b - bt).abs().max().item() <= 2e-5 * max(1.0, bt.abs().max().item()), n
            moved = max(moved, (b - initial[n]).abs().max().item())
    assert moved > 1e-3
    for m in (model, twin):
        m.eval()
    with torch.no_grad():
        a, b = model.pure_model_forward(x), twin.pure_model_forward(x)
    torch.cuda.synchronize()
    assert model._engines and twin._engines
    for k in a:
        assert (a[k] - b[k]).abs().max().item() <= 1e-4 * max(1.0, b[k].abs().max().item()), k
    ea, eb = next(iter(model._engines.values())), next(iter(twin._engines.values()))
    assert ea.conv_plans() == eb.conv_plans()
