"""The kernels of csrc/mobilenet.hip over every shape of their loops, stand-alone, against float64 torch on the CPU.

1x1 product (fpc_conv1x1_f32): the five forms — 16 x 16 tiles, and 32 x 32 tiles with NT = 1 / 2 / 3 / 5 channel tiles per wave — at the
smallest site that gives each form, with a ragged last row tile, over Cin = every multiple of 8 up to 192 and the network's long K
up to the entry's limit of 1024.  That is 0 to 5 iterations of the pipelined loop with every tail count for U = 4 (more for U = 2
and 1: up to 128 iterations at NT = 5), the reload branch `it + 2 < iters`, odd counts, and every (whole, half) tail of the 16 x 16
form behind 0, 1 and 2 iterations; a ragged last channel tile inside a multi-tile wave on the whole sweep, full channel tiles on
five Cin.  Two operand sets per case: small integers, on which every summation order gives the same float, held to float64 BIT FOR
BIT, and the random operands of test_gpu_mobilenet_v2.py at its kernel bar 2e-5 max(1, |ref|max) (integers are exact in a
reduced-precision product too: the exact set alone would not see a lost mantissa).  ReLU6 without a residual, no activation with
one.  The four 32 x 32 forms are held to each other bit for bit on a common block (the file header's "ascending K-steps whatever NT
and U are").

Depthwise and stem (fpc_dwconv3x3, fpc_stem3x3s2): grids of 8 workgroups and more, where xcd_walk / xcd_rows take their banded
branch, with band borders inside a row and inside a strip row, and one depthwise launch of 4096 x 256 + 1024 items, where 128
threads of each band take a second grid stride; random operands at the same bar and integers bit for bit.

Every case asserts its form or its banded grid before it launches, launches twice into NaN-filled buffers between 64-float canaries
and compares the two runs' bits.  Run with -s the cases print their errors."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RELU6 = 1

# form: (M, Cout of full tiles, Cout with a ragged last tile); M = 32 (row tiles - 1) + 5.  The least row tiles that give the form
# (fpc_conv1x1_f32_form is asserted per case): 2 x 3 tiles of 32 < 1024; 17 x 61 >= 1024 with 61 prime; 64 x 64/2 = 2048;
# 98 x 63/3 = 2058; 171 x 60/5 = 2052.
FORMS = {0: (37, 48, 40), 1: (517, 1952, 1944), 2: (2021, 2048, 2040), 3: (3109, 2016, 2008), 5: (5445, 1920, 1912)}
KMAX = 1024
CIN_SWEEP = list(range(8, 193, 8)) + [320, 384, 576, 960, 1016, 1024]
CIN_FULL = [8, 64, 104, 320, 1024]
# sorted by (form, Cin): the float64 reference of a form advances along its K-prefixes (_Prefix)
PW_SWEEP = [(f, ci, co) for f, (_, full, ragged) in FORMS.items() for ci in CIN_SWEEP
            for co in ([ragged, full] if ci in CIN_FULL else [ragged])]
CROSS_CIN = [104, 320, 1016]

# (B, Hi, Wi, C, stride, banded).  2070 items, 2070 % 8 = 6: bands of 259, borders inside a row and a strip row.  The same shape
# at stride 2 has 1080 items, a grid of 5 and is NOT banded (kept: the clipped windows of an odd map at stride 2); the stride-2
# banded case with items % 8 != 0 and borders inside a row is (3, 27, 25, 28): 2058 items, bands of 258, rows of 49.
DW_BANDED = [(3, 23, 21, 20, 1, True), (3, 23, 21, 20, 2, False), (3, 27, 25, 28, 2, True), (2, 37, 45, 36, 2, True)]
DW_SECOND_STRIDE = (1, 8200, 64, 32, 1)           # 1 049 600 items = 4096 x 256 + 1024
STEM_BANDED = [(1, 87, 85), (3, 61, 67)]          # 1892 pixels: grid 8, bands of 237 (not a multiple of 32); 3162: grid 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    yield torch.device("cuda:0")
    _OPS.clear()               # (a form's operands and prefix sums are a few hundred MB)
    _CROSS.clear()


@pytest.fixture(scope="module")
def lib(dev):
    from fastposecnn_amd import _native
    return _native.lib()


def _bits(t):
    return t.view(torch.int32)


def _twice(dev, n, launch):
    """test_gpu_mobilenet_v2.py's harness with the checks on the device (outputs of up to 10 M floats): two launches into fresh
    NaN-filled buffers with 64-float canaries around the n outputs: the canaries intact, nothing left unwritten, both runs the
    same bits.  Returns the first run's outputs (device, flat)."""
    outs = []
    for _ in range(2):
        buf = torch.full((n + 128,), float("nan"), device=dev)
        y = buf[64:64 + n]
        assert y.data_ptr() % 16 == 0
        assert launch(y.data_ptr()) == 0
        torch.cuda.synchronize()
        assert torch.isnan(buf[:64]).all() and torch.isnan(buf[64 + n:]).all(), "a canary was overwritten"
        outs.append(y)
    assert not torch.isnan(outs[0]).any(), "unwritten outputs"
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    return outs[0]


_WORST = {}


def _bar(out, ref, what, key):
    err = (out.double() - ref).abs().max().item()
    _WORST[key] = max(_WORST.get(key, 0.0), err / max(1.0, ref.abs().max().item()))
    print(what, "err", err, "ref max", ref.abs().max().item(), "| worst so far of", key, "relative to the bar's scale:", _WORST[key])
    assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (what, err)


def _exact(out, ref, what):
    same = torch.equal(out.double(), ref)
    print(what, "exact", same)
    assert same, (what, (out.double() - ref).abs().max().item())


class _Prefix:
    """sum over k < K of x[m][k] w[n][k] in float64.  The value at K is a function of the operands alone; the object keeps the
    last one asked for and adds x[:, a:b] @ w[:, a:b].T to reach the next, so a form's sweep in ascending Cin costs one full-K
    product (a smaller K than the last starts again from zero)."""

    def __init__(self, x, w):
        self.x, self.w, self.k, self.acc = x.double(), w.double(), 0, None

    def upto(self, K):
        if self.acc is None or K < self.k:
            self.acc, self.k = torch.zeros((self.x.shape[0], self.w.shape[0]), dtype=torch.float64), 0
        if K > self.k:
            self.acc += self.x[:, self.k:K] @ self.w[:, self.k:K].t()
            self.k = K
        return self.acc


def _draw(g, M, Cout, exact):
    """One operand set at full K and the widest Cout; a case takes the K-prefix and the first Cout channels.  Exact: integers in
    [-4, 4], scale in {0.5, 1, 2}, integer shift in [-8, 8]: every partial sum is an integer below 2^15 and every output a multiple
    of 0.5 far below 2^24.  Random: the existing test's recipe; its 1 / sqrt(Cin) sits in the scale (_scale) instead of in w, so
    that w is one tensor for every Cin."""
    if exact:
        ints = lambda *shape: torch.randint(-4, 5, shape, generator=g).float()
        x, w, res = ints(M, KMAX), ints(Cout, KMAX), ints(M, Cout)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (Cout,), generator=g)]
        shift = torch.randint(-8, 9, (Cout,), generator=g).float()
    else:
        x, w, res = torch.randn((M, KMAX), generator=g), torch.randn((Cout, KMAX), generator=g), torch.randn((M, Cout), generator=g)
        scale = (torch.rand(Cout, generator=g) + 0.5) * 4.0
        shift = torch.randn(Cout, generator=g)
    return {"x": x, "w": w, "res": res, "scale": scale, "shift": shift, "exact": exact}


def _scale(o, Cin, Cout):
    return o["scale"][:Cout].clone() if o["exact"] else o["scale"][:Cout] / Cin ** 0.5          # (f32: what the kernel gets)


_OPS = {}


def _operands(form):
    """The two operand sets of a form and their prefix sums, from one fixed seed per form; one form is kept at a time."""
    if form not in _OPS:
        _OPS.clear()
        M, full, _ = FORMS[form]
        g = torch.Generator().manual_seed(7000 + form)
        sets = [_draw(g, M, full, True), _draw(g, M, full, False)]
        for o in sets:
            o["prefix"] = _Prefix(o["x"], o["w"])
        _OPS[form] = sets
    return _OPS[form]


def _conv1x1(L, dev, o, M, Cin, Cout, scale, act, with_res):
    from fastposecnn_amd import _native as nat
    xd, wd = o["x"][:M, :Cin].contiguous().to(dev), o["w"][:Cout, :Cin].contiguous().to(dev)
    sd, hd = scale.contiguous().to(dev), o["shift"][:Cout].contiguous().to(dev)
    rd = o["res"][:M, :Cout].contiguous().to(dev) if with_res else None
    return _twice(dev, M * Cout, lambda y: L.fpc_conv1x1_f32(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(),
                                                              rd.data_ptr() if with_res else None, y, M, Cin, Cout, act,
                                                              nat.stream())).view(M, Cout)


@pytest.mark.parametrize("form,Cin,Cout", PW_SWEEP, ids=[f"form{f}-Cin{ci}-Cout{co}" for f, ci, co in PW_SWEEP])
def test_conv1x1_f32_sweep(lib, dev, form, Cin, Cout):
    L = lib
    M = FORMS[form][0]
    assert L.fpc_conv1x1_f32_form(M, Cin, Cout) == form
    for o in _operands(form):
        kind = "exact" if o["exact"] else "random"
        what = f"conv1x1_f32 form {form} M {M} {Cin} -> {Cout} {kind}"
        scale = _scale(o, Cin, Cout)
        pre = o["prefix"].upto(Cin)[:, :Cout] * scale.double() + o["shift"][:Cout].double()
        assert (pre < 0).any() and (pre > 6).any()                 # both clamps engage
        relu = _conv1x1(L, dev, o, M, Cin, Cout, scale, RELU6, False).cpu()
        added = _conv1x1(L, dev, o, M, Cin, Cout, scale, 0, True).cpu()
        ref_relu, ref_added = pre.clamp(0.0, 6.0), pre + o["res"][:, :Cout].double()
        if o["exact"]:
            _exact(relu, ref_relu, what + " relu6")
            _exact(added, ref_added, what + " + res")
        else:
            _bar(relu, ref_relu, what + " relu6", f"1x1 form {form}")
            _bar(added, ref_added, what + " + res", f"1x1 form {form}")
        assert (relu == 0).any() and (relu == 6).any() and relu.max() <= 6 and relu.min() >= 0
        assert added.min() < 0 and added.max() > 6                 # nothing is clamped


_CROSS = {}


def _cross_operands():
    if not _CROSS:
        g = torch.Generator().manual_seed(7100)
        _CROSS.update(_draw(g, FORMS[5][0], 2048, False))
    return _CROSS


@pytest.mark.parametrize("Cin", CROSS_CIN)
def test_conv1x1_f32_forms_agree_bit_for_bit(lib, dev, Cin):
    """Each output element of a 32 x 32 form is one chain of MFMAs in ascending k, whatever NT and U are: forms 1, 2, 3 and 5, each
    at its own (M, ragged Cout) on the same rows of x and w, agree bit for bit on the block they share.  (The 16 x 16 form sums in
    another order.)"""
    L = lib
    o = _cross_operands()
    m, n = FORMS[1][0], FORMS[5][2]                                  # the common block [517][1912]
    scale = _scale(o, Cin, 2048)
    ref = o["x"][:m, :Cin].double() @ o["w"][:n, :Cin].double().t() * scale[:n].double() + o["shift"][:n].double()
    blocks = {}
    for form in (1, 2, 3, 5):
        M, _, Cout = FORMS[form]
        assert M >= m and Cout >= n and L.fpc_conv1x1_f32_form(M, Cin, Cout) == form
        out = _conv1x1(L, dev, o, M, Cin, Cout, scale[:Cout], 0, False)
        blocks[form] = out[:m, :n].contiguous()
        _bar(blocks[form].cpu(), ref, f"conv1x1_f32 form {form} Cin {Cin} common block", f"1x1 form {form}")
    for form in (2, 3, 5):
        assert torch.equal(_bits(blocks[form]), _bits(blocks[1])), (form, Cin)


def _dw_operands(g, B, Hi, Wi, C, exact):
    if exact:      # integers in [-4, 4], a power-of-two scale, an integer shift: nine products below 2^8, every order the same float
        x = torch.randint(-4, 5, (B, C, Hi, Wi), generator=g).float()
        w = torch.randint(-4, 5, (C, 1, 3, 3), generator=g).float()
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
        shift = torch.randint(-8, 9, (C,), generator=g).float()
    else:
        x = torch.randn((B, C, Hi, Wi), generator=g)
        w = torch.randn((C, 1, 3, 3), generator=g)
        scale = (torch.rand(C, generator=g) + 0.5) * 4.0            # pre-activations of order ten: both clamps engage
        shift = torch.randn(C, generator=g)
    return x, w, scale, shift


def _dw_items(B, Hi, Wi, C, s):
    Ho, Wo, TW = (Hi - 1) // s + 1, (Wi - 1) // s + 1, 4 if s == 1 else 2
    return B * Ho * ((Wo + TW - 1) // TW) * (C // 4)


def _dwconv(L, dev, case, act, exact, seed):
    from fastposecnn_amd import _native as nat
    B, Hi, Wi, C, s = case
    kind = "exact" if exact else "random"
    x, w, scale, shift = _dw_operands(torch.Generator().manual_seed(seed), B, Hi, Wi, C, exact)
    ref = F.conv2d(x.double(), w.double(), None, s, 1, 1, C) * scale.double().view(1, C, 1, 1) + shift.double().view(1, C, 1, 1)
    assert (ref < 0).any() and (ref > 6).any()
    if act:
        ref = ref.clamp(0.0, 6.0)
    Ho, Wo = (Hi - 1) // s + 1, (Wi - 1) // s + 1
    assert tuple(ref.shape) == (B, C, Ho, Wo)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, ref.numel(), lambda y: L.fpc_dwconv3x3(xd.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi, C,
                                                             s, act, nat.stream())).cpu()
    out = out.view(B, Ho, Wo, C).permute(0, 3, 1, 2)
    if exact:
        _exact(out, ref, f"dwconv3x3 {case} act {act} {kind}")
    else:
        _bar(out, ref, f"dwconv3x3 {case} act {act} {kind}", "depthwise")
    if act:
        assert (out == 0).any() and (out == 6).any() and out.max() <= 6 and out.min() >= 0
    else:
        assert out.min() < 0 and out.max() > 6                       # nothing is clamped


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("act", [RELU6, 0], ids=["relu6", "plain"])
@pytest.mark.parametrize("case", DW_BANDED, ids=[f"B{b}-{h}x{w}-C{c}-s{s}" for b, h, w, c, s, _ in DW_BANDED])
def test_dwconv3x3_banded(lib, dev, case, act, exact):
    *shape, banded = case
    items = _dw_items(*shape)
    assert ((items + 255) // 256 >= 8) == banded, items              # stream_grid: a multiple of 8 from 8 workgroups up
    _dwconv(lib, dev, tuple(shape), act, exact, 3000 + 10 * DW_BANDED.index(case) + act)


def test_dwconv3x3_second_grid_stride(lib, dev):
    """4096 x 256 + 1024 items: in each of the eight bands (131 200 items, 512 workgroups) the first 128 threads take a second item."""
    items = _dw_items(*DW_SECOND_STRIDE)
    assert items == 4096 * 256 + 1024 and (items + 7) // 8 == 512 * 256 + 128
    _dwconv(lib, dev, DW_SECOND_STRIDE, RELU6, False, 3100)
    _dwconv(lib, dev, DW_SECOND_STRIDE, RELU6, True, 3101)


@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
@pytest.mark.parametrize("B,Hi,Wi", STEM_BANDED)
def test_stem3x3s2_banded(lib, dev, B, Hi, Wi, exact):
    from fastposecnn_amd import _native as nat
    L = lib
    Ho, Wo = (Hi - 1) // 2 + 1, (Wi - 1) // 2 + 1
    assert (B * Ho * Wo + 255) // 256 >= 8                           # the banded branch of xcd_rows
    g = torch.Generator().manual_seed(3200 + Hi * 100 + Wi)
    if exact:      # 27 integer products below 2^9, a power-of-two scale, an integer shift
        x = torch.randint(-4, 5, (B, 3, Hi, Wi), generator=g).float()
        w = torch.randint(-4, 5, (32, 3, 3, 3), generator=g).float()
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (32,), generator=g)]
        shift = torch.randint(-8, 9, (32,), generator=g).float()
    else:
        x = torch.randn((B, 3, Hi, Wi), generator=g)
        w = torch.randn((32, 3, 3, 3), generator=g) / 27 ** 0.5
        scale = (torch.rand(32, generator=g) + 0.5) * 4.0
        shift = torch.randn(32, generator=g)
    ref = F.conv2d(x.double(), w.double(), None, 2, 1) * scale.double().view(1, 32, 1, 1) + shift.double().view(1, 32, 1, 1)
    assert (ref < 0).any() and (ref > 6).any()
    ref = ref.clamp(0.0, 6.0)
    assert tuple(ref.shape) == (B, 32, Ho, Wo)
    assert Hi % 2 and Wi % 2                                         # odd sizes: the NHWC4 image is built on the host
    x4 = torch.cat([x.permute(0, 2, 3, 1), torch.zeros(B, Hi, Wi, 1)], dim=3).contiguous().to(dev)
    wd, sd, hd = w.to(dev), scale.to(dev), shift.to(dev)
    out = _twice(dev, ref.numel(), lambda y: L.fpc_stem3x3s2(x4.data_ptr(), wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), y, B, Hi, Wi, 32,
                                                             nat.stream())).cpu()
    out = out.view(B, Ho, Wo, 32).permute(0, 3, 1, 2)
    if exact:
        _exact(out, ref, f"stem3x3s2 {(B, Hi, Wi)} exact")
    else:
        _bar(out, ref, f"stem3x3s2 {(B, Hi, Wi)} random", "stem")
    assert (out == 0).any() and (out == 6).any() and out.max() <= 6 and out.min() >= 0
