"""The SE-ResNet block's training path on the MI355X (csrc/se_train.hip behind FPC_TRAIN_NATIVE_SE): fpc_se_gate_train and fpc_se_bwd
against the float64 formulas of _se_train_refs (pinned to autograd by test_se_train_host.py) at the kernel bar
2e-5 max(1, |ref|max) on operands where no ReLU sits on its kink, every case launched twice and bit-identical; the gate's bits
against fpc_se_gate's; exact cases (gy = 0, a saturated gate); dres = NULL; the autograd Function against the raw entry; the routing
of SEResNetBottleneck; and one se_resnet50 training step with the switch on, off and in float64.

Whole-model wiring bar (test_whole_model_wiring): per parameter |g_on - g_off|_2 / |g_off|_2 <= 5e-2 — a ReLU mask that flips
between two f32 runs moves a gradient by up to about 6e-3 in this norm, a wiring mistake by order one.  Measured maximum on the
MI355X: 1.65e-2 and 5.8e-3 in two runs (DESIGN.md 4.2a''''')."""
import pytest
import torch

import _se_train_refs as R

pytestmark = pytest.mark.gpu

BAR = 2e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat(dev):
    from fastposecnn_amd import _native
    _native.lib()
    return _native


def _nan(dev, *shape):
    return torch.full(shape, NAN, device=dev)


def _forward(nat, dev, case, ops):
    """fpc_se_gate_train + fpc_se_scale_add_relu into NaN-filled buffers; ops: device tensors.  Returns device tensors."""
    L = nat.lib()
    B, H, W, C, Rd = case
    Cr = C // Rd
    out = dict(gate=_nan(dev, B, C), mean=_nan(dev, B, C), hidden=_nan(dev, B, Cr), y=_nan(dev, B, H, W, C))
    scratch = _nan(dev, L.fpc_se_scratch_floats(B, H, W, C))
    p = lambda t: t.data_ptr()
    assert L.fpc_se_gate_train(p(ops["x"]), p(ops["w1"]), p(ops["b1"]), p(ops["w2"]), p(ops["b2"]), p(out["gate"]), p(out["mean"]),
                               p(out["hidden"]), p(scratch), B, H, W, C, Rd, nat.stream()) == 0
    assert L.fpc_se_scale_add_relu(p(ops["x"]), p(out["gate"]), p(ops["res"]), p(out["y"]), B, H, W, C, nat.stream()) == 0
    torch.cuda.synchronize()
    return out


def _backward(nat, dev, case, ops, fwd, gy, dx=None, dres="fresh"):
    """fpc_se_bwd into NaN-filled buffers (dres=None: the NULL form).  Returns device tensors."""
    L = nat.lib()
    B, H, W, C, Rd = case
    Cr = C // Rd
    out = dict(dx=_nan(dev, B, H, W, C) if dx is None else dx, dw1=_nan(dev, Cr, C), db1=_nan(dev, Cr), dw2=_nan(dev, C, Cr),
               db2=_nan(dev, C))
    if dres is not None:
        out["dres"] = _nan(dev, B, H, W, C)
    n = L.fpc_se_bwd_scratch_floats(B, H, W, C, Rd)
    assert n == B * (L.fpc_se_pool_slabs(H, W, C) * C + 2 * C + Cr)
    scratch = _nan(dev, n)
    p = lambda t: t.data_ptr()
    gy0 = gy.clone()
    assert L.fpc_se_bwd(p(ops["x"]), p(fwd["y"]), p(gy), p(fwd["gate"]), p(fwd["mean"]), p(fwd["hidden"]), p(ops["w1"]), p(ops["w2"]),
                        p(out["dx"]), p(out["dres"]) if dres is not None else None, p(out["dw1"]), p(out["db1"]), p(out["dw2"]),
                        p(out["db2"]), p(scratch), B, H, W, C, Rd, nat.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gy, gy0), "gy was written"
    return out


def _on(dev, ops):
    return {k: v.contiguous().to(dev) for k, v in ops.items()}


@pytest.mark.parametrize("case", R.SHAPES, ids=R.IDS)
def test_kernels_vs_float64(nat, dev, case):
    """Items 1 and 2: every output of the forward-with-state and of the backward at the kernel bar, all written, twice the same
    bits; the gate's bits are fpc_se_gate's."""
    L = nat.lib()
    B, H, W, C, Rd = case
    if case == (1, 37, 41, 128, 8):
        assert L.fpc_se_pool_slabs(H, W, C) > 1
    ops, ref = R.operands(case)
    assert ref["pre_out"].abs().min().item() >= 0.2, "an output ReLU near its kink"
    assert ref["pre_hidden"].abs().min().item() >= 1e-3, "a hidden ReLU near its kink"
    d = _on(dev, ops)
    runs = []
    for _ in range(2):
        fwd = _forward(nat, dev, case, d)
        bwd = _backward(nat, dev, case, d, fwd, d["gy"])
        runs.append({k: v.cpu() for k, v in {**fwd, **bwd}.items()})
    got = runs[0]
    for k, v in got.items():
        assert torch.isfinite(v).all(), (k, "NaN or an unwritten element")
        assert torch.equal(v, runs[1][k]), (k, "two launches differ")
    assert torch.equal(got["y"] > 0, ref["y"] > 0), "the device's ReLU mask is not the reference's"
    for k in ("mean", "hidden", "gate", "y", "dx", "dres", "dw1", "db1", "dw2", "db2"):
        err = (got[k].double() - ref[k]).abs().max().item()
        bar = BAR * max(1.0, ref[k].abs().max().item())
        print("se_train", case, k, "err", err, "bar", bar)
        assert got[k].shape == ref[k].shape and err <= bar, (k, err, bar)
    gate = _nan(dev, B, C)
    scratch = _nan(dev, L.fpc_se_scratch_floats(B, H, W, C))
    assert L.fpc_se_gate(d["x"].data_ptr(), d["w1"].data_ptr(), d["b1"].data_ptr(), d["w2"].data_ptr(), d["b2"].data_ptr(),
                         gate.data_ptr(), scratch.data_ptr(), B, H, W, C, Rd, nat.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gate.cpu(), got["gate"]), "fpc_se_gate_train's gate is not fpc_se_gate's"


@pytest.mark.parametrize("case", R.SHAPES, ids=R.IDS)
def test_exact_cases(nat, dev, case):
    """Item 3: gy = 0 gives exact zeros; b2 = +-100 on alternating channels gives gates of exactly 1 / 0, g (1 - g) = 0, so the four
    parameter gradients are exactly zero, dx == d on the even channels and 0 on the odd ones, bit for bit."""
    B, H, W, C, Rd = case
    ops, _ = R.operands(case)
    d = _on(dev, ops)
    fwd = _forward(nat, dev, case, d)
    out = _backward(nat, dev, case, d, fwd, torch.zeros_like(d["gy"]))
    for k, v in out.items():
        assert torch.equal(v.cpu(), torch.zeros(v.shape)), (k, "gy = 0")
    d["b2"] = torch.where(torch.arange(C) % 2 == 0, 100.0, -100.0).to(dev)
    fwd = _forward(nat, dev, case, d)
    gate = fwd["gate"].cpu()
    assert torch.equal(gate[:, 0::2], torch.ones(B, C // 2)) and torch.equal(gate[:, 1::2], torch.zeros(B, C // 2))
    out = {k: v.cpu() for k, v in _backward(nat, dev, case, d, fwd, d["gy"]).items()}
    for k in ("dw1", "db1", "dw2", "db2"):
        assert torch.equal(out[k], torch.zeros(out[k].shape)), k
    dd = torch.where(fwd["y"].cpu() > 0, ops["gy"], torch.zeros(()))
    assert (dd != 0).any()
    assert torch.equal(out["dres"], dd)
    assert torch.equal(out["dx"][..., 0::2], dd[..., 0::2]) and torch.equal(out["dx"][..., 1::2], torch.zeros_like(dd[..., 1::2]))


@pytest.mark.parametrize("case", [R.SHAPES[1], R.SHAPES[3], R.SHAPES[5]], ids=[R.IDS[1], R.IDS[3], R.IDS[5]])
def test_dres_null(nat, dev, case):
    """Item 4: with dres = NULL dx and the parameter gradients are what they were, and nothing beside dx is written."""
    ops, _ = R.operands(case)
    d = _on(dev, ops)
    fwd = _forward(nat, dev, case, d)
    full = _backward(nat, dev, case, d, fwd, d["gy"])
    n = d["x"].numel()
    buf = _nan(dev, 64 + 2 * n + 64)            # 64 canaries, dx, then a canary the size of dres and 64 more
    dx = buf[64:64 + n].view(d["x"].shape)
    assert dx.data_ptr() % 16 == 0
    part = _backward(nat, dev, case, d, fwd, d["gy"], dx=dx, dres=None)
    host = buf.cpu()
    assert torch.isnan(host[:64]).all() and torch.isnan(host[64 + n:]).all(), "a canary beside dx was overwritten"
    for k in ("dx", "dw1", "db1", "dw2", "db2"):
        assert torch.equal(part[k].cpu(), full[k].cpu()), k


@pytest.mark.parametrize("case", [R.SHAPES[1], R.SHAPES[5]], ids=[R.IDS[1], R.IDS[5]])
def test_function_equals_raw_entry(nat, dev, case):
    """Item 5: _SEGateAddReLUFn under torch.autograd.grad, with a gy that is not channel-last, returns the raw entry's numbers."""
    from fastposecnn_amd.lib import train_conv
    B, H, W, C, Rd = case
    Cr = C // Rd
    ops, _ = R.operands(case)
    d = _on(dev, ops)
    fwd = _forward(nat, dev, case, d)
    raw = _backward(nat, dev, case, d, fwd, d["gy"])
    x = d["x"].permute(0, 3, 1, 2).requires_grad_(True)
    res = d["res"].permute(0, 3, 1, 2).requires_grad_(True)
    w1 = d["w1"].view(Cr, C, 1, 1).requires_grad_(True)
    w2 = d["w2"].view(C, Cr, 1, 1).requires_grad_(True)
    b1, b2 = d["b1"].clone().requires_grad_(True), d["b2"].clone().requires_grad_(True)
    before = dict(train_conv.counters)
    y = train_conv._SEGateAddReLUFn.apply(x, res, w1, b1, w2, b2)
    assert y.shape == x.shape and y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(y.permute(0, 2, 3, 1), fwd["y"])
    gy = d["gy"].permute(0, 3, 1, 2).contiguous()            # NCHW-contiguous: not the layout the kernels read
    if H * W > 1:
        assert not gy.is_contiguous(memory_format=torch.channels_last)
    gx, gres, gw1, gb1, gw2, gb2 = torch.autograd.grad(y, [x, res, w1, b1, w2, b2], gy)
    torch.cuda.synchronize()
    assert gw1.shape == (Cr, C, 1, 1) and gw2.shape == (C, Cr, 1, 1)
    assert torch.equal(gx.permute(0, 2, 3, 1), raw["dx"]) and torch.equal(gres.permute(0, 2, 3, 1), raw["dres"])
    assert torch.equal(gw1.view(Cr, C), raw["dw1"]) and torch.equal(gb1, raw["db1"])
    assert torch.equal(gw2.view(C, Cr), raw["dw2"]) and torch.equal(gb2, raw["db2"])
    used = {k: train_conv.counters[k] - before[k] for k in before}
    assert used["se_fwd_native"] == 1 and used["se_bwd_native"] == 1
    # the residual needs no gradient: dres = NULL, the others unchanged
    y2 = train_conv._SEGateAddReLUFn.apply(x, res.detach(), w1, b1, w2, b2)
    gx2, gw1b = torch.autograd.grad(y2, [x, w1], gy)
    assert torch.equal(gx2, gx) and torch.equal(gw1b, gw1)


def _blocks(dev):
    from fastposecnn_amd.lib import backbone as bb
    torch.manual_seed(3)
    plain = bb.SEResNetBottleneck(256, 64, 16)
    down = torch.nn.Sequential(bb.Conv2d(256, 512, 1, 2, bias=False), bb.BatchNorm2d(512))
    strided = bb.SEResNetBottleneck(256, 128, 16, stride=2, downsample=down)
    return [("plain", plain.to(dev).train()), ("stride-2 downsample", strided.to(dev).train())]


def _step(blk, x):
    from fastposecnn_amd.lib import train_conv
    before = dict(train_conv.counters)
    blk.zero_grad(set_to_none=True)
    xin = x.clone(memory_format=torch.channels_last).requires_grad_(True)
    y = blk(xin)
    y.square().mean().backward()
    torch.cuda.synchronize()
    used = {k: train_conv.counters[k] - before[k] for k in before}
    return y.detach(), xin.grad, used


def test_routing(nat, dev, monkeypatch):
    """Item 6: one native forward and one native backward per block with the switch on; none with either ReLU swapped for a
    Softplus (and then the output is that of the torch lines on the tensors this very forward fed them, up to the f32 roundings
    by which torch's own kernels differ between two calls), none with the switch off."""
    from fastposecnn_amd.lib import train_conv
    monkeypatch.setattr(train_conv, "ENABLED", True)
    x = torch.randn((2, 256, 8, 12), generator=torch.Generator().manual_seed(4)).to(dev).contiguous(memory_format=torch.channels_last)
    for name, blk in _blocks(dev):
        monkeypatch.setattr(train_conv, "NATIVE_SE", False)
        y_off, gx_off, used = _step(blk, x)
        assert used["se_fwd_native"] == 0 and used["se_bwd_native"] == 0 and used["se_torch"] == 1, (name, used)
        monkeypatch.setattr(train_conv, "NATIVE_SE", True)
        y_on, gx_on, used = _step(blk, x)
        assert used["se_fwd_native"] == 1 and used["se_bwd_native"] == 1 and used["se_torch"] == 0, (name, used)
        assert y_on.shape == y_off.shape and gx_on.shape == x.shape and torch.isfinite(gx_on).all()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters()), name
        assert blk.se_module.fc1.weight.grad.shape == blk.se_module.fc1.weight.shape
        # (f32 against f32, a continuous function: the gate's sums in another order)
        assert (y_on - y_off).abs().max().item() <= 1e-5 * max(1.0, y_off.abs().max().item()), name
        for owner, attr in ((blk, "relu"), (blk.se_module, "relu")):
            relu = getattr(owner, attr)
            setattr(owner, attr, torch.nn.Softplus())
            seen, hooks = {}, []
            try:
                hooks += [blk.bn3.register_forward_hook(lambda m, i, o: seen.__setitem__("out", o.detach().clone()))]
                if blk.downsample is not None:
                    hooks.append(blk.downsample.register_forward_hook(lambda m, i, o: seen.__setitem__("res", o.detach().clone())))
                y_sp, _, used = _step(blk, x)
                assert used["se_fwd_native"] == 0 and used["se_bwd_native"] == 0 and used["se_torch"] == 1, (name, attr, used)
                with torch.no_grad():       # the torch lines on what this very forward fed them
                    y_ref = blk.relu(blk.se_module(seen["out"]) + seen.get("res", x))
                # torch's own 1x1 convolution of the [B, C, 1, 1] means does not repeat bit for bit on this device (two calls of
                # se_module.fc1 on one input differed by 1.5e-8, the block's output by 2.4e-7 = 2^-22), so "equals the torch path"
                # is held to 1e-6 max(1, |ref|max): eight f32 roundings of the output scale.  ReLU in place of the Softplus —
                # what the native path would compute — is off by order 0.1.
                err = (y_sp - y_ref).abs().max().item()
                print("se routing", name, attr, "against the torch lines:", err)
                assert err <= 1e-6 * max(1.0, y_ref.abs().max().item()), (name, attr, err)
            finally:
                setattr(owner, attr, relu)
                for hk in hooks:
                    hk.remove()


def test_whole_model_wiring(nat, dev, monkeypatch):
    """Item 7: se_resnet50, B = 2, 64 x 96, every ReLU kept: the switch on, the switch off and float64."""
    import fastposecnn_amd.lib as lib
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    hp.ENCODER = "se_resnet50"
    torch.manual_seed(0)
    model = lib.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.p = 0.0
    x = torch.stack([synth.make_image(i, 64, 96) for i in range(2)]).to(dev)
    monkeypatch.setattr(train_conv, "ENABLED", True)
    res = {}
    for tag in ("on", "off", "float64"):
        monkeypatch.setattr(train_conv, "NATIVE_SE", tag == "on")
        if tag == "float64":
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
    l_on, o_on, g_on, used_on = res["on"]
    l_off, o_off, g_off, used_off = res["off"]
    l_ref, o_ref, g_ref, _ = res["float64"]
    assert used_on["se_fwd_native"] == 16 and used_on["se_bwd_native"] == 16 and used_on["se_torch"] == 0, used_on
    assert used_off["se_fwd_native"] == 0 and used_off["se_bwd_native"] == 0, used_off
    assert used_on["fwd_native"] >= 100
    for tag, loss, outs in (("on", l_on, o_on), ("off", l_off, o_off)):
        assert abs(loss - l_ref) <= 1e-5 * max(1.0, abs(l_ref)), (tag, loss, l_ref)
        for k in o_ref:
            assert (outs[k] - o_ref[k]).abs().max().item() <= 1e-4 * max(1.0, o_ref[k].abs().max().item()), (tag, k)
    assert set(g_on) == set(g_off) == set(g_ref)
    se_names = [n for n in g_on if ".se_module.fc" in n]
    assert len(se_names) == 64 and all(n.rsplit(".", 2)[-2] in ("fc1", "fc2") for n in se_names)
    worst = (0.0, None)
    for n in g_off:
        assert torch.isfinite(g_on[n]).all() and torch.isfinite(g_off[n]).all(), n
        assert g_on[n].shape == g_off[n].shape
        den = g_off[n].norm().item()
        num = (g_on[n] - g_off[n]).norm().item()
        rel = num / den if den > 0 else (0.0 if num == 0 else float("inf"))
        worst = max(worst, (rel, n))
    print("se_resnet50 training step, switch on against off: worst relative gradient difference", worst)
    assert worst[0] <= 5e-2, worst
