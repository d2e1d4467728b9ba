"""The training step's VGG pieces on the native kernels (csrc/vgg_train.hip, lib/train_conv.py: _VggConv0Fn, _MaxPool2x2Fn,
backbone.VGGEncoder) on the MI355X, behind train_conv.NATIVE_VGG (FPC_TRAIN_NATIVE_VGG=1, off by default).  References: float64
torch on the CPU (tests/_vgg_train_refs.py).  Bars, the project's own: forward results within 2e-5 max(1, |ref|max), weight and bias
gradients within 1e-4 max(1, |ref|max); integer-valued operands, one-hot gradients and the max-pool's routing of dy are exact and
held to torch.equal.  Every kernel output sits between canaries and is launched twice (tests/_densenet_kernels.py: _twice)."""
import copy

import pytest
import torch
import torch.nn.functional as F

import _vgg_model as V
import _vgg_train_refs as R
from _densenet_kernels import NAN, _twice
from test_gpu_vgg import CONV_SHAPES, POOL_SHAPES

pytestmark = pytest.mark.gpu

NEW_KEYS = ("c3_fwd_native", "c3_wgrad_native", "pool2_fwd_native", "pool2_bwd_native")
EINVAL = -1
RAGGED = (2, 37, 70)      # 148 units in 18 slices: the slice count neither divides the units nor is a multiple of 8 (no banded order)
WGRAD_SHAPES = CONV_SHAPES + [RAGGED]
PATTERN = (torch.arange(64, dtype=torch.float32) % 7 - 3.0) * 0.5      # what a db that must not be written holds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L(dev):
    import fastposecnn_amd.lib  # noqa: F401
    from fastposecnn_amd import _native
    return _native.lib()


class PinnedPlans(dict):
    def get(self, key, default=None):      # conv_nhwc asks with .get(key): no candidate is timed, none is remembered
        return 0


# ------------------------------------------------------------------------------------------------------- fpc_conv3x3_c3_wgrad

def _wgrad(L, dev, img, dy, with_db=True, ws_out=None):
    """img [B,3,H,W], dy [B,64,H,W] on the CPU -> (dw [64,3,3,3], db [64] or None), the first of two canaried launches.  The image's
    fourth channel is NaN; without db the 64 floats behind dw hold a pattern that must survive."""
    from fastposecnn_amd import _native as nat
    B, _, H, W = img.shape
    x4 = torch.full((B, H, W, 4), NAN)
    x4[..., :3] = img.permute(0, 2, 3, 1)
    xd, dyd = x4.to(dev), dy.permute(0, 2, 3, 1).contiguous().to(dev)
    nbytes = L.fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W)
    ws = torch.full((nbytes // 4 + 1024,), NAN, device=dev)
    prefill = torch.cat([torch.full((64 * 27,), NAN), torch.full((64,), NAN) if with_db else PATTERN])
    out = _twice(dev, prefill, lambda y: L.fpc_conv3x3_c3_wgrad(xd.data_ptr(), dyd.data_ptr(), y, y + 64 * 27 * 4 if with_db else None,
                                                                B, H, W, ws.data_ptr(), nbytes, nat.stream()))
    assert torch.isfinite(out).all(), "the image's fourth channel reached a result"
    if ws_out is not None:
        ws_out.append(ws.cpu())
    return out[:64 * 27].view(64, 3, 3, 3), (out[64 * 27:] if with_db else None)


@pytest.fixture(scope="module")
def wgrad_runs(L, dev):
    """Each shape once: random operands, db given and db NULL, the workspace as the launch left it, the float64 reference."""
    runs = {}
    for shape in WGRAD_SHAPES:
        B, H, W = shape
        g = torch.Generator().manual_seed(100 + H)
        img = torch.randn((B, 3, H, W), generator=g)
        dy = torch.randn((B, 64, H, W), generator=g)
        ws = []
        dw, db = _wgrad(L, dev, img, dy, True, ws)
        dw0, _ = _wgrad(L, dev, img, dy, False)
        runs[shape] = (dw, db, dw0, ws[0], R.c3_wgrad_ref(img, dy))
    return runs


@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_wgrad_vs_float64(wgrad_runs, shape):
    dw, db, dw0, _, (rw, rb) = wgrad_runs[shape]
    for what, got, ref in (("dw", dw, rw), ("db", db, rb)):
        ok, err, bound = R.close(got, ref, 1e-4)
        print(f"{shape} {what}: error {err:.3e}, bound {bound:.3e}")
        assert ok, (what, err, bound)
    assert torch.equal(dw0.view(torch.int32), dw.view(torch.int32))      # db NULL: the same dw bits


def test_wgrad_slice_seams(L, wgrad_runs):
    """A unit is (frame, row, 64-pixel segment); slice s takes units [s U / n, (s + 1) U / n) and writes partial s: exactly
    fpc_conv3x3_c3_wgrad_slices partials of 64 x 48 floats are written — all of them, nothing behind them.  One slice, a slice count
    that divides the units, one that does not (in banded order, and in launch order), a seam inside a frame: all held to the bar."""
    kinds = {}
    for (B, H, W) in WGRAD_SHAPES:
        n = L.fpc_conv3x3_c3_wgrad_slices(B, H, W)
        per_frame = H * ((W + 63) // 64)
        units = B * per_frame
        assert n == max(1, min(1024, units // 8))
        ws = wgrad_runs[(B, H, W)][3]
        assert torch.isfinite(ws[:n * 64 * 48]).all() and torch.isnan(ws[n * 64 * 48:]).all(), (B, H, W)
        ends = [s * units // n for s in range(1, n)]
        if n == 1:
            kinds.setdefault("one slice", (B, H, W))
        if n > 1 and units % n == 0:
            kinds.setdefault("even slices", (B, H, W))
        if n > 1 and units % n and n % 8 == 0:
            kinds.setdefault("ragged slices, banded", (B, H, W))
        if n > 1 and units % n and n % 8:
            kinds.setdefault("ragged slices, launch order", (B, H, W))
        if any(e % per_frame for e in ends):
            kinds.setdefault("seam inside a frame", (B, H, W))
    assert set(kinds) == {"one slice", "even slices", "ragged slices, banded", "ragged slices, launch order", "seam inside a frame"}, kinds
    assert kinds["ragged slices, launch order"] == RAGGED
    for shape in kinds.values():
        dw, db, _, _, (rw, rb) = wgrad_runs[shape]
        assert R.close(dw, rw, 1e-4)[0] and R.close(db, rb, 1e-4)[0], shape


@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 33, 65)])
def test_wgrad_exact_on_integers(L, dev, shape):
    """Image in [-4, 4], dy in [-2, 2]: every partial sum is an integer below 2^24 (at most 33 * 65 terms of magnitude <= 8), so
    the f32 result IS the float64 one — tap and padding indexing, and the bias column, with no tolerance to hide in."""
    B, H, W = shape
    g = torch.Generator().manual_seed(7)
    img = torch.randint(-4, 5, (B, 3, H, W), generator=g).float()
    dy = torch.randint(-2, 3, (B, 64, H, W), generator=g).float()
    dw, db = _wgrad(L, dev, img, dy)
    rw, rb = R.c3_wgrad_ref(img, dy)
    assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb)


def test_wgrad_one_hot_pixels(L, dev):
    """dy one-hot at each corner and at one interior pixel against an image of distinct integers: dw is the 3 x 3 patch of the image
    around that pixel, not flipped, zero where it leaves the image — exactly."""
    B, H, W = 2, 5, 7
    img = (torch.arange(B * 3 * H * W, dtype=torch.float32) + 1.0).view(B, 3, H, W)
    for k, (y0, x0) in enumerate(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (2, 3))):
        b, co = k % B, 11 * k + 3
        dy = torch.zeros((B, 64, H, W))
        dy[b, co, y0, x0] = 1.0
        dw, db = _wgrad(L, dev, img, dy)
        want = torch.zeros((64, 3, 3, 3))
        for kh in range(3):
            for kw in range(3):
                yy, xx = y0 + kh - 1, x0 + kw - 1
                if 0 <= yy < H and 0 <= xx < W:
                    want[co, :, kh, kw] = img[b, :, yy, xx]
        assert torch.equal(dw, want), (y0, x0)
        rw, rb = R.c3_wgrad_ref(img, dy)
        assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb), (y0, x0)


def test_wgrad_refusals(L, dev):
    from fastposecnn_amd import _native as nat
    B, H, W = 1, 8, 8
    img4 = torch.zeros((B, H, W + 1, 4), device=dev)
    dy = torch.zeros((B, H, W + 1, 64), device=dev)
    out = torch.full((64 * 27 + 64 + 8,), NAN, device=dev)
    nbytes = L.fpc_conv3x3_c3_wgrad_workspace_bytes(B, H, W)
    ws = torch.full((nbytes // 4 + 64,), NAN, device=dev)
    s = nat.stream()
    p = [img4.data_ptr(), dy.data_ptr(), out.data_ptr(), out.data_ptr() + 64 * 27 * 4]
    tail = (ws.data_ptr(), nbytes, s)
    assert L.fpc_conv3x3_c3_wgrad(*p, 0, H, W, *tail) == EINVAL
    assert L.fpc_conv3x3_c3_wgrad(*p, B, 0, W, *tail) == EINVAL
    assert L.fpc_conv3x3_c3_wgrad(*p, B, H, -1, *tail) == EINVAL
    assert L.fpc_conv3x3_c3_wgrad(*p, 2 ** 14, 2 ** 7, 2 ** 7, *tail) == EINVAL      # B H W = 2^28: beyond conv3x3_c3_ok
    for k in range(4):                                                               # a null pointer (db may be null), a pointer off by 4 bytes
        for bad in (None, p[k] + 4):
            if k == 3 and bad is None:
                continue
            q = list(p)
            q[k] = bad
            assert L.fpc_conv3x3_c3_wgrad(*q, B, H, W, *tail) == EINVAL, (k, bad)
    assert L.fpc_conv3x3_c3_wgrad(*p, B, H, W, None, nbytes, s) == EINVAL
    assert L.fpc_conv3x3_c3_wgrad(*p, B, H, W, ws.data_ptr() + 4, nbytes, s) == EINVAL
    assert L.fpc_conv3x3_c3_wgrad(*p, B, H, W, ws.data_ptr(), nbytes - 1, s) == EINVAL        # one byte short
    assert L.fpc_conv3x3_c3_wgrad(*p, B, H, W, ws.data_ptr(), 0, s) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(ws).all()), "a refused call wrote"


# ------------------------------------------------------------------------------------------------------------- the 2x2 max-pool

@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_maxpool2x2_backward_is_exact(L, dev, monkeypatch, B, H, W, C):
    """Random, post-ReLU, all-equal windows and the maximum planted at each window position: dx is the float64 reference's dx cast to
    f32, bit for bit (every element a copy of dy or 0), and _MaxPool2x2Fn's forward is F.max_pool2d's."""
    from fastposecnn_amd import _native as nat
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    inputs = R.pool_inputs(B, H, W, C, 20 + H)
    assert (inputs["relu"] == 0).double().mean().item() >= 0.40      # ties are the common case
    g = torch.Generator().manual_seed(31)
    dy = torch.randn((B, C, H // 2, W // 2), generator=g)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    for kind, x in inputs.items():
        xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
        dx = _twice(dev, torch.full((B * H * W * C,), NAN),
                    lambda y: L.fpc_maxpool2x2_bwd(xd.data_ptr(), dyd.data_ptr(), y, B, H, W, C, nat.stream())).view(B, H, W, C)
        yref, ref = R.pool2_ref(x, dy)
        assert torch.equal(dx.permute(0, 3, 1, 2), ref.float()), kind
        assert torch.equal(ref.float().double(), ref)      # (the reference's dx is dy or 0: the cast loses nothing)
        # through the front end: forward and backward
        xn = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        before = dict(train_conv.counters)
        yn = train_conv.maxpool2x2(xn)
        assert yn is not None and type(yn.grad_fn).__name__ == "_MaxPool2x2FnBackward"
        assert torch.equal(yn.detach().cpu(), F.max_pool2d(x, 2, 2)) and torch.equal(yn.detach().cpu().double(), yref), kind
        yn.backward(dy.to(dev))
        torch.cuda.synchronize()
        assert torch.equal(xn.grad.cpu(), ref.float()), kind
        used = {k: train_conv.counters[k] - before[k] for k in before}
        assert used == {k: int(k in ("pool2_fwd_native", "pool2_bwd_native")) for k in before}, used


def test_maxpool2x2_refusals(L, dev, monkeypatch):
    from fastposecnn_amd import _native as nat
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    x = torch.zeros((1, 8, 8, 64), device=dev)
    dx = torch.full((1 * 8 * 8 * 64 + 4,), NAN, device=dev)
    s = nat.stream()
    p = [x.data_ptr(), x.data_ptr(), dx.data_ptr()]
    for shape in [(1, 7, 8, 64), (1, 8, 7, 64), (1, 8, 8, 6), (1, 8, 8, 2), (0, 8, 8, 64), (1, 0, 8, 64), (2 ** 16, 2 ** 9, 2 ** 9, 4)]:
        assert L.fpc_maxpool2x2_bwd(*p, *shape, s) == EINVAL, shape                 # odd H, odd W, C % 4, empty, 2^32 items
    for k in range(3):
        for bad in (None, p[k] + 4):
            q = list(p)
            q[k] = bad
            assert L.fpc_maxpool2x2_bwd(*q, 1, 8, 8, 64, s) == EINVAL, (k, bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()), "a refused call wrote dx"
    before = dict(train_conv.counters)
    for shape in [(1, 64, 7, 8), (1, 64, 8, 7), (1, 6, 8, 8)]:      # [B, C, H, W]
        t = torch.zeros(shape, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        assert train_conv.maxpool2x2(t) is None, shape
    ok = torch.zeros((1, 64, 8, 8), device=dev)
    assert train_conv.maxpool2x2(ok.requires_grad_(True)) is None                                       # planar
    assert train_conv.maxpool2x2(ok.detach().contiguous(memory_format=torch.channels_last)) is None     # needs no gradient
    assert dict(train_conv.counters) == before


# ------------------------------------------------------------------------------------------------------------ under autograd

def _segment(name, seed):
    """A VGGEncoder cut down to features.0 [-> BatchNorm] -> ReLU -> conv 64 -> 64 -> MaxPool2d(2, 2), run by VGGEncoder.forward."""
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(seed)
    enc = bb.VGGEncoder(name)
    n = 3 if enc.batch_norm else 2
    mods = list(enc.features[:n]) + [bb.Conv2d(64, 64, 3, padding=1), torch.nn.MaxPool2d(kernel_size=2, stride=2)]
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        mods[0].bias.copy_(torch.randn(64, generator=g) * 0.1)
        mods[n].weight.copy_(torch.randn((64, 64, 3, 3), generator=g) * (2.0 / 576) ** 0.5)
        mods[n].bias.copy_(torch.randn(64, generator=g) * 0.1)
    enc.features = torch.nn.Sequential(*mods)
    return enc.train()


@pytest.mark.parametrize("name", ["vgg11", "vgg11_bn"])
def test_segment_under_autograd(L, dev, monkeypatch, name):
    """features.0 -> [BatchNorm ->] ReLU -> conv 64 -> 64 -> pool at (2, 32, 96) with the switch on: the pooled output, features.0's
    weight.grad and bias.grad against the float64 module chain on the CPU, and each new counter moves once.
    The upstream gradient is that of a mean over the pooled plane (randn / 1536 pixels), as every loss of the training step is a
    mean.  Behind a training-mode BatchNorm the true bias gradient is exactly 0 and what any f32 path returns is N times the rounding
    error of the BatchNorm backward's own mean of g: with a sum-type gradient (plain randn) torch's f32 CPU chain alone is 3.5e-4 off
    there (|ref| 7e-13) and 5.6e-4 off on weight.grad — that would measure torch's BatchNorm, not these kernels.  With the mean-type
    gradient torch's own f32 error is 2.3e-7 / 2.8e-7, |weight.grad|max is 0.33 (vgg11: 0.089) and |bias.grad|max 0.067 (vgg11): the
    1e-4 bar is 3e-4 .. 1.5e-3 of the values, which no wrong tap, route or scale passes; the kernels' own numerics are held above."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    monkeypatch.setattr(train_conv, "_plan_cache", PinnedPlans())
    enc = _segment(name, 5)
    ref = copy.deepcopy(enc).double()
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, 3, 32, 96), generator=g)
    gz = torch.randn((2, 64, 16, 48), generator=g) / (2 * 16 * 48)
    enc = enc.to(dev)
    before = dict(train_conv.counters)
    feats = enc(x.to(dev))
    assert len(feats) == 2 and tuple(feats[0].shape) == (2, 64, 32, 96) and tuple(feats[1].shape) == (2, 64, 16, 48)
    feats[1].backward(gz.to(dev))
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert all(used[k] == 1 for k in NEW_KEYS), used
    assert used["dgrad_aten"] == 0 and used["wgrad_aten"] == 0, used
    rfeats = ref(x.double())
    rfeats[1].backward(gz.double())
    ok, err, bound = R.close(feats[1], rfeats[1].detach(), 2e-5)
    print(f"{name} y: error {err:.3e}, bound {bound:.3e}")
    assert ok, (err, bound)
    for what, got, want in (("weight.grad", enc.features[0].weight.grad, ref.features[0].weight.grad),
                            ("bias.grad", enc.features[0].bias.grad, ref.features[0].bias.grad)):
        ok, err, bound = R.close(got, want, 1e-4)
        print(f"{name} {what}: error {err:.3e}, bound {bound:.3e}")
        assert ok, (what, err, bound)


@pytest.mark.parametrize("encoder", ["vgg11_bn", "vgg11"])
def test_training_step(dev, monkeypatch, encoder):
    """One training step at (2, 64, 96) through the modules with the switch on: a finite loss, every parameter with a finite
    gradient, features.0 and all five pools native."""
    import fastposecnn_amd.lib as lib
    from fastposecnn_amd import config
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    # a plan cache of this test's own: what this test times must not decide what later tests run
    monkeypatch.setattr(train_conv, "_plan_cache", {})
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = encoder
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    x = V.images(2, 64, 96).to(dev)
    before = dict(train_conv.counters)
    out = model.pure_model_forward(x)
    loss = sum(v.square().mean() for v in out.values())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).item()
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert any(p.grad.abs().max().item() > 0 for n, p in model.named_parameters() if n.startswith("encoder.features.0."))
    used = {k: train_conv.counters[k] - before[k] for k in NEW_KEYS}
    assert used == {"c3_fwd_native": 1, "c3_wgrad_native": 1, "pool2_fwd_native": 5, "pool2_bwd_native": 5}, used


@pytest.mark.parametrize("what", ["switch_off", "x_requires_grad", "odd_pool_input", "ceil_mode", "stride_2"])
def test_fallbacks_keep_torch(L, dev, monkeypatch, what):
    """Outside the native class the modules are torch's own — bit-equal to F.conv2d on the channel-last input conv2d() hands over,
    and to F.max_pool2d, forward and backward — and no counter moves."""
    from fastposecnn_amd.lib import backbone as bb, train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", what != "switch_off")
    g = torch.Generator().manual_seed(13)
    before = dict(train_conv.counters)
    if what in ("switch_off", "x_requires_grad", "stride_2"):      # the convolution
        stride = 2 if what == "stride_2" else 1
        x = torch.randn((2, 3, 10, 14), generator=g).to(dev)
        x.requires_grad_(what == "x_requires_grad")
        torch.manual_seed(1)
        conv = bb.Conv2d(3, 64, 3, stride=stride, padding=1).to(dev).train()
        y = conv(x)
        assert torch.equal(y, F.conv2d(x.detach().contiguous(memory_format=torch.channels_last), conv.weight, conv.bias, stride, 1))
        y.sum().backward()
        assert bool(torch.isfinite(conv.weight.grad).all()) and bool(torch.isfinite(conv.bias.grad).all())
    if what in ("switch_off", "odd_pool_input", "ceil_mode"):      # the pool, as VGGEncoder.forward runs it
        enc = bb.VGGEncoder("vgg11")
        enc.features = torch.nn.Sequential(torch.nn.MaxPool2d(kernel_size=2, stride=2, ceil_mode=(what == "ceil_mode")))
        shape = (2, 64, 7, 10) if what == "odd_pool_input" else (2, 64, 6, 10)
        xp = torch.relu(torch.randn(shape, generator=g)).to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        xq = xp.detach().clone(memory_format=torch.channels_last).requires_grad_(True)
        pre, out = enc(xp)
        assert pre is xp
        want = F.max_pool2d(xq, 2, 2, ceil_mode=(what == "ceil_mode"))
        assert torch.equal(out, want)
        gz = torch.randint(-3, 4, out.shape, generator=g).float().to(dev)
        out.backward(gz)
        want.backward(gz)
        assert torch.equal(xp.grad, xq.grad)
    torch.cuda.synchronize()
    assert dict(train_conv.counters) == before


def test_registered_grad_sink(L, dev, monkeypatch):
    """A GradSink registered for features.0's weight: the kernel writes its view, autograd gets no weight gradient, `written` is set
    and the callback fires once, the bias gradient still comes back through autograd; a second use of the weight in the same step
    returns its gradient the ordinary way; a view that is not 16-byte aligned is left alone."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "NATIVE_VGG", True)
    g = torch.Generator().manual_seed(9)
    w = (torch.randn((64, 3, 3, 3), generator=g) / 5).to(dev).requires_grad_(True)
    b = (torch.randn(64, generator=g) / 10).to(dev).requires_grad_(True)
    img = torch.randn((2, 3, 19, 35), generator=g)
    gy = torch.randn((2, 64, 19, 35), generator=g)
    rw, rb = R.c3_wgrad_ref(img, gy)
    view = torch.full((64, 3, 3, 3), NAN, device=dev)
    fired = []

    class Owner:
        pass
    owner = Owner()
    sink = train_conv.GradSink(view, lambda: fired.append(1), owner)
    monkeypatch.setitem(train_conv.grad_sinks, w.data_ptr(), sink)
    before = dict(train_conv.counters)
    y = train_conv.conv2d(img.to(dev), w, b, 1, 1)
    ok, err, bound = R.close(y, R.c3_forward_ref(img, w.detach(), b.detach()), 2e-5)
    assert ok, (err, bound)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    assert w.grad is None                      # nothing was returned for autograd to accumulate
    assert sink.written and fired == [1]
    assert R.close(view, rw, 1e-4)[0] and R.close(b.grad, rb, 1e-4)[0]
    assert train_conv.counters["c3_wgrad_native"] == before["c3_wgrad_native"] + 1
    b.grad = None
    train_conv.conv2d(img.to(dev), w, b, 1, 1).backward(gy.to(dev))      # the same step, the sink already written
    torch.cuda.synchronize()
    assert fired == [1] and w.grad is not None and R.close(w.grad, rw, 1e-4)[0] and R.close(b.grad, rb, 1e-4)[0]
    assert R.close(view, rw, 1e-4)[0]        # ... and its view was left alone
    # a misaligned view: not taken
    w.grad = None
    flat = torch.full((64 * 27 + 4,), NAN, device=dev)
    off = train_conv.GradSink(flat[1:1 + 64 * 27].view(64, 3, 3, 3), lambda: fired.append(2), owner)
    assert off.view.data_ptr() % 16 == 4
    monkeypatch.setitem(train_conv.grad_sinks, w.data_ptr(), off)
    train_conv.conv2d(img.to(dev), w, b, 1, 1).backward(gy.to(dev))
    torch.cuda.synchronize()
    assert not off.written and fired == [1] and bool(torch.isnan(flat).all())
    assert w.grad is not None and R.close(w.grad, rw, 1e-4)[0]
