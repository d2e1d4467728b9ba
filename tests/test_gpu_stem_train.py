"""The training step's 7x7 stem and its max-pool on the native kernels (csrc/stem_train.hip, lib/train_conv.py: _StemConvFn,
_MaxPoolFn, backbone.MaxPool2d) on the MI355X, behind train_conv.NATIVE_STEM (FPC_TRAIN_NATIVE_STEM=1, off by default).
References: float64 torch on the CPU (tests/_stem_refs.py).  Bars, the project's own: forward and data-side results within
2e-5 max(1, |ref|max), weight gradients within 1e-4 max(1, |ref|max); integer-valued operands, a max and the max-pool's gather
of integer gradients are exact and held to torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import _stem_refs as R

pytestmark = pytest.mark.gpu

NEW_KEYS = ("stem_fwd_native", "stem_wgrad_native", "pool_fwd_native", "pool_bwd_native")
EINVAL, EWORKSPACE = -1, -2
# (B, Hi, Wi): every output pixel with padding taps; Ho = 19, Wo = 35, odd and below one segment; Wo = 80, one full 64-pixel
# segment plus a partial; two full segments
WGRAD_SHAPES = [(1, 8, 8), (2, 38, 70), (3, 64, 160), (2, 96, 256)]
POOL_SHAPES = [(2, 64, 6, 10), (1, 8, 7, 9), (2, 64, 19, 35)]      # [B, C, H, W]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    import fastposecnn_amd.lib  # noqa: F401
    from fastposecnn_amd import _native
    return _native.lib()


def _image4(L, dev, img):
    from fastposecnn_amd import _native as nat
    B, _, H, W = img.shape
    x = img.to(dev).contiguous()
    img4 = torch.full((B, H, W, 4), float("nan"), device=dev)
    nat.check(L.fpc_image_nhwc4(x.data_ptr(), img4.data_ptr(), B, H, W, nat.stream()), "fpc_image_nhwc4")
    return img4


def _wgrad(L, dev, img4, dy_nhwc):
    from fastposecnn_amd import _native as nat
    B, H, W, _ = img4.shape
    dw = torch.full((64, 3, 7, 7), float("nan"), device=dev)
    ws = torch.empty(max(L.fpc_stem_wgrad_workspace_bytes(B, H, W), 256), dtype=torch.uint8, device=dev)
    nat.check(L.fpc_stem_wgrad(img4.data_ptr(), dy_nhwc.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), nat.stream()),
              "fpc_stem_wgrad")
    torch.cuda.synchronize()
    return dw


@pytest.fixture(scope="module")
def wgrad_runs(L, dev):
    """Each shape once: random operands, two native calls, the float64 reference."""
    runs = {}
    for shape in WGRAD_SHAPES:
        B, H, W = shape
        g = torch.Generator().manual_seed(100 + H)
        img = torch.randn((B, 3, H, W), generator=g)
        dy = torch.randn((B, 64, H // 2, W // 2), generator=g)
        img4 = _image4(L, dev, img)
        assert torch.equal(img4[..., :3].cpu(), img.permute(0, 2, 3, 1)) and bool((img4[..., 3] == 0).all())
        dyd = dy.to(dev).permute(0, 2, 3, 1).contiguous()
        runs[shape] = (_wgrad(L, dev, img4, dyd), _wgrad(L, dev, img4, dyd), R.stem_wgrad_ref(img, dy))
    return runs


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_vs_float64(wgrad_runs, shape):
    first, second, ref = wgrad_runs[shape]
    assert not torch.isnan(first).any(), "unwritten elements"
    ok, err, bound = R.close(first, ref, 1e-4)
    print(f"{shape}: error {err:.3e}, bound {bound:.3e}")
    assert ok, (err, bound)
    assert torch.equal(first, second)      # bit-identical from call to call


@pytest.mark.parametrize("shape", [(1, 8, 8), (2, 38, 70)])
def test_wgrad_exact_on_integers(L, dev, shape):
    """Image in [-4, 4], dy in [-2, 2]: every partial sum is an integer below 2^24 (at most 2 * 19 * 35 terms of magnitude <= 8), so
    the f32 result IS the float64 one — tap, parity and padding indexing with no tolerance to hide in."""
    B, H, W = shape
    g = torch.Generator().manual_seed(7)
    img = torch.randint(-4, 5, (B, 3, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (B, 64, H // 2, W // 2), generator=g).float()
    dw = _wgrad(L, dev, _image4(L, dev, img), dy.to(dev).permute(0, 2, 3, 1).contiguous())
    assert torch.equal(dw.double().cpu(), R.stem_wgrad_ref(img, dy))


def test_wgrad_slice_seams(L, wgrad_runs):
    """A unit is (frame, output row, 64-pixel segment); slice s takes units [s U / n, (s + 1) U / n).  Among the shapes above:
    one slice; a unit count the slice count does not divide; a slice that ends inside a frame — all held to the 1e-4 bar."""
    kinds = {}
    for (B, H, W) in WGRAD_SHAPES:
        n = L.fpc_stem_wgrad_slices(B, H, W)
        per_frame = (H // 2) * ((W // 2 + 63) // 64)
        units = B * per_frame
        ends = [s * units // n for s in range(1, n)]
        if n == 1:
            kinds.setdefault("one slice", (B, H, W))
        if n > 1 and units % n:
            kinds.setdefault("ragged slices", (B, H, W))
        if any(e % per_frame for e in ends):
            kinds.setdefault("seam inside a frame", (B, H, W))
    assert set(kinds) == {"one slice", "ragged slices", "seam inside a frame"}, kinds
    for shape in kinds.values():
        first, _, ref = wgrad_runs[shape]
        assert R.close(first, ref, 1e-4)[0], shape


def test_wgrad_refusals(L, dev):
    from fastposecnn_amd import _native as nat
    B, H, W = 1, 8, 8
    img4 = torch.zeros((B, H + 2, W, 4), device=dev)
    dy = torch.zeros((B, H // 2 + 1, W // 2, 64), device=dev)
    dw = torch.full((64 * 147 + 4,), float("nan"), device=dev)
    nbytes = L.fpc_stem_wgrad_workspace_bytes(B, H, W)
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    s = nat.stream()
    p = (img4.data_ptr(), dy.data_ptr(), dw.data_ptr())
    assert L.fpc_stem_wgrad(*p, B, H + 1, W, ws.data_ptr(), ws.numel(), s) == EINVAL            # odd Hi
    assert L.fpc_stem_wgrad(*p, B, H, W + 1, ws.data_ptr(), ws.numel(), s) == EINVAL
    assert L.fpc_stem_wgrad(*p, B, 6, W, ws.data_ptr(), ws.numel(), s) == EINVAL
    assert L.fpc_stem_wgrad(*p, 0, H, W, ws.data_ptr(), ws.numel(), s) == EINVAL
    for k in range(3):                                                                           # a null pointer, a pointer off by 4 bytes
        for bad in (None, p[k] + 4):
            q = list(p)
            q[k] = bad
            assert L.fpc_stem_wgrad(*q, B, H, W, ws.data_ptr(), ws.numel(), s) == EINVAL, (k, bad)
    assert L.fpc_stem_wgrad(*p, B, H, W, None, ws.numel(), s) == EINVAL
    assert L.fpc_stem_wgrad(*p, B, H, W, ws.data_ptr() + 16, nbytes, s) == EINVAL               # the workspace: 256 bytes
    assert L.fpc_stem_wgrad(*p, B, H, W, ws.data_ptr(), nbytes - 1, s) == EWORKSPACE            # one byte short
    x = torch.zeros((1, 64, 4, 4), device=dev)
    assert L.fpc_image_nhwc4(None, img4.data_ptr(), 1, 8, 8, s) == EINVAL
    assert L.fpc_image_nhwc4(x.data_ptr() + 4, img4.data_ptr(), 1, 8, 8, s) == EINVAL
    assert L.fpc_image_nhwc4(x.data_ptr(), img4.data_ptr(), 1, 0, 8, s) == EINVAL
    for fn, n in ((L.fpc_maxpool3x3s2_fwd, 2), (L.fpc_maxpool3x3s2_bwd, 3)):
        q = [x.data_ptr()] * n
        assert fn(*q, 1, 4, 4, 6, s) == EINVAL                                                   # C % 4 != 0
        assert fn(*q, 1, 0, 4, 64, s) == EINVAL
        assert fn(*q, 65536, 256, 256, 4, s) == EINVAL                                           # 2^34 elements
        assert fn(*([None] + q[1:]), 1, 4, 4, 64, s) == EINVAL
        assert fn(*(q[:-1] + [q[-1] + 4]), 1, 4, 4, 64, s) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()), "a refused call wrote dw"


@pytest.mark.parametrize("shape", [(2, 38, 70), (3, 64, 160), (2, 24, 256)])
def test_stem_forward_through_the_front_end(L, dev, monkeypatch, shape):
    """_StemConvFn's forward: (2, 38, 70) and (3, 64, 160) have output rows that do not divide into 64-pixel segments (the
    implicit-GEMM kernel's generic loader), (2, 24, 256) has two segments per row (k_stem7x7, code 3000)."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", True)
    B, H, W = shape
    g = torch.Generator().manual_seed(3)
    img = torch.randn((B, 3, H, W), generator=g)
    w = (torch.randn((64, 3, 7, 7), generator=g) * (2.0 / 147) ** 0.5).to(dev).requires_grad_(True)
    before = dict(train_conv.counters)
    y = train_conv.conv2d(img.to(dev), w, None, 2, 3)
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert used == {k: int(k == "stem_fwd_native") for k in before}, used
    assert y.shape == (B, 64, H // 2, W // 2) and y.stride(1) == 1 and y.is_contiguous(memory_format=torch.channels_last)
    assert y.requires_grad
    ok, err, bound = R.close(y, R.stem_forward_ref(img, w.detach()), 2e-5)
    print(f"{shape}: error {err:.3e}, bound {bound:.3e}")
    assert ok, (err, bound)


def _pool_call(L, dev, fn, *tensors, shape):
    from fastposecnn_amd import _native as nat
    B, C, H, W = shape
    nat.check(fn(*[t.data_ptr() for t in tensors], B, H, W, C, nat.stream()), "max-pool")
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def pool_inputs():
    out = {}
    for shape in POOL_SHAPES:
        x = R.tie_heavy(shape, 20 + shape[2])
        assert (x == 0).double().mean().item() >= 0.40      # ties are the common case
        out[shape] = x
    return out


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_forward_is_exact(L, dev, pool_inputs, shape):
    x = pool_inputs[shape]
    B, C, H, W = shape
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous()
    y = torch.full((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C), float("nan"), device=dev)
    _pool_call(L, dev, L.fpc_maxpool3x3s2_fwd, xd, y, shape=shape)
    assert torch.equal(y.permute(0, 3, 1, 2).cpu(), R.maxpool_ref(x))


@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_maxpool_backward(L, dev, pool_inputs, shape):
    x = pool_inputs[shape]
    B, C, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd = x.to(dev).permute(0, 2, 3, 1).contiguous()
    g = torch.Generator().manual_seed(31)
    for kind in ("integer", "random"):
        dy = torch.randint(-3, 4, (B, C, Ho, Wo), generator=g).float() if kind == "integer" else torch.randn((B, C, Ho, Wo), generator=g)
        dyd = dy.to(dev).permute(0, 2, 3, 1).contiguous()
        got = []
        for _ in range(2):
            dx = torch.full((B, H, W, C), float("nan"), device=dev)
            _pool_call(L, dev, L.fpc_maxpool3x3s2_bwd, xd, dyd, dx, shape=shape)
            got.append(dx.permute(0, 3, 1, 2).cpu())
        assert not torch.isnan(got[0]).any(), "unwritten elements"
        assert torch.equal(got[0], got[1])
        _, ref = R.maxpool_ref(x.double(), dy.double())
        if kind == "integer":
            assert torch.equal(got[0].double(), ref)
        else:
            ok, err, bound = R.close(got[0], ref, 2e-5)
            assert ok, (err, bound)


@pytest.mark.parametrize("shape", [(2, 38, 70), (1, 16, 256)])
def test_stem_segment_under_autograd(L, dev, monkeypatch, shape):
    """conv1 -> maxpool in training mode with the switch on, on integers (image in [-3, 3], weights in [-2, 2], integer upstream
    gradient): no near-tie can flip an arg-max between f32 and float64, every sum is exact, so the pooled output and weight.grad
    equal the float64 CPU run.  (1, 16, 256): the k_stem7x7 forward; (2, 38, 70): the generic one."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", True)
    B, H, W = shape
    g = torch.Generator().manual_seed(8)
    img = torch.randint(-3, 4, (B, 3, H, W), generator=g).float()
    conv = bb.Conv2d(3, 64, 7, 2, 3, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randint(-2, 3, (64, 3, 7, 7), generator=g).float())
    w0 = conv.weight.detach().clone()
    conv, pool = conv.to(dev).train(), bb.MaxPool2d(3, 2, 1).train()
    before = dict(train_conv.counters)
    z = pool(conv(img.to(dev)))
    gz = torch.randint(-2, 3, z.shape, generator=g).float()
    z.backward(gz.to(dev))
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert all(used[k] == 1 for k in NEW_KEYS), used
    assert used["dgrad_aten"] == 0 and used["wgrad_aten"] == 0 and all(v == 0 for k, v in used.items() if k not in NEW_KEYS), used
    wr = w0.double().requires_grad_(True)
    zr = F.max_pool2d(F.conv2d(img.double(), wr, None, 2, 3), 3, 2, 1)
    zr.backward(gz.double())
    assert torch.equal(z.detach().double().cpu(), zr.detach())
    assert torch.equal(conv.weight.grad.double().cpu(), wr.grad)


def test_resnet18_training_step_and_engine_repack(L, dev, monkeypatch):
    """ResNet18 PoseRegressor at (2, 3, 64, 64) with the switch on: one forward and backward in training mode runs the stem and
    the max-pool native, conv1.weight.grad is finite, and an engine plan bound BEFORE the step repacks afterwards (the training
    forward notes its unversioned writes) and evaluates without error."""
    import fastposecnn_amd.lib as lib
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", True)

    class PinnedPlans(dict):
        def get(self, key, default=None):      # conv_nhwc asks with .get(key): no candidate is timed, none is remembered
            return 0
    monkeypatch.setattr(train_conv, "_plan_cache", PinnedPlans())
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "resnet18"
    hp.ENGINE_AUTOTUNE = False
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev)
    x = torch.stack([synth.make_image(i, 64, 64) for i in range(2)]).to(dev)
    model.eval()
    with torch.no_grad():
        model.pure_model_forward(x)
    assert model._engines
    gen = model._weights_gen[0]
    model.train()
    before = dict(train_conv.counters)
    out = model.pure_model_forward(x)
    sum(v.square().mean() for v in out.values()).backward()
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert all(used[k] == 1 for k in NEW_KEYS), used
    assert used["dgrad_aten"] == 0 and used["wgrad_aten"] == 0, used
    gw = model.encoder.conv1.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and gw.abs().max().item() > 0
    assert model._weights_gen[0] > gen
    model.eval()
    with torch.no_grad():
        got = model.pure_model_forward(x)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert all(e.generation == model._weights_gen[0] for e in model._engines.values())


@pytest.mark.parametrize("what", ["x_requires_grad", "odd_width", "bias", "return_indices", "switch_off"])
def test_fallbacks_keep_torch(L, dev, monkeypatch, what):
    """Outside the native class the modules are torch's own — bit-equal to F.conv2d on the channel-last input conv2d() hands over,
    and to F.max_pool2d, forward and backward — and no counter moves."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", what != "switch_off")
    g = torch.Generator().manual_seed(13)
    before = dict(train_conv.counters)
    if what != "return_indices":      # the convolution
        x = torch.randn((2, 3, 38, 71 if what == "odd_width" else 70), generator=g).to(dev)
        x.requires_grad_(what == "x_requires_grad")
        torch.manual_seed(1)
        conv = bb.Conv2d(3, 64, 7, 2, 3, bias=(what == "bias")).to(dev).train()
        y = conv(x)
        assert torch.equal(y, F.conv2d(x.detach().contiguous(memory_format=torch.channels_last), conv.weight, conv.bias, 2, 3))
        y.sum().backward()
        assert bool(torch.isfinite(conv.weight.grad).all())
    if what in ("return_indices", "switch_off"):      # the max-pool, on a tensor of the native class
        xp = R.tie_heavy((2, 64, 19, 35), 14).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        xq = xp.detach().clone(memory_format=torch.channels_last).requires_grad_(True)
        pool = bb.MaxPool2d(3, 2, 1, return_indices=(what == "return_indices"))
        out = pool(xp)
        want = F.max_pool2d(xq, 3, 2, 1, return_indices=(what == "return_indices"))
        if what == "return_indices":
            assert torch.equal(out[1], want[1])
            out, want = out[0], want[0]
        assert torch.equal(out, want)
        gz = torch.randint(-3, 4, out.shape, generator=g).float().to(dev)
        out.backward(gz)
        want.backward(gz)
        assert torch.equal(xp.grad, xq.grad)
    torch.cuda.synchronize()
    assert dict(train_conv.counters) == before


def test_registered_grad_sink(L, dev, monkeypatch):
    """A GradSink registered for the stem weight: the kernel writes its view, autograd gets no weight gradient, `written` is set
    and the callback fires once; a second use of the weight in the same step returns its gradient the ordinary way."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_STEM", True)
    g = torch.Generator().manual_seed(9)
    w = (torch.randn((64, 3, 7, 7), generator=g) / 12).to(dev).requires_grad_(True)
    img = torch.randn((2, 3, 38, 70), generator=g)
    gy = torch.randn((2, 64, 19, 35), generator=g)
    ref = R.stem_wgrad_ref(img, gy)
    view = torch.full((64, 3, 7, 7), float("nan"), device=dev)
    fired = []

    class Owner:
        pass
    owner = Owner()
    sink = train_conv.GradSink(view, lambda: fired.append(1), owner)
    monkeypatch.setitem(train_conv.grad_sinks, w.data_ptr(), sink)
    before = dict(train_conv.counters)
    train_conv.conv2d(img.to(dev), w, None, 2, 3).backward(gy.to(dev))
    torch.cuda.synchronize()
    assert w.grad is None                      # nothing was returned for autograd to accumulate
    assert sink.written and fired == [1]
    assert R.close(view, ref, 1e-4)[0]
    assert train_conv.counters["stem_wgrad_native"] == before["stem_wgrad_native"] + 1
    train_conv.conv2d(img.to(dev), w, None, 2, 3).backward(gy.to(dev))      # the same step, the sink already written
    torch.cuda.synchronize()
    assert fired == [1] and w.grad is not None and R.close(w.grad, ref, 1e-4)[0]
    assert R.close(view, ref, 1e-4)[0]        # ... and its view was left alone
