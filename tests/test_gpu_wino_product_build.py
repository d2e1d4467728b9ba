"""The product library holds no Winograd diagnostics (they need a -DFPC_STAMP_WINO build): the environment variables that used to pick
the kernels' diagnostic instantiations (weight reload, staging or barrier skipped: wrong results) change nothing, and fpc_conv2d's
relu is what fpc.h documents — any non-zero value is ReLU on, gn_part is always the GroupNorm record buffer.
Shape: B = 1, Cin = 32, 7 x 9, Cout = 128 — several K-steps, two pairs of them for form -9, two 64-channel blocks / one 128-channel block."""
import ctypes
import hashlib
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FORMS = (-6, -7, -8, -9)
B, CIN, H, W, COUT = 1, 32, 7, 9, 128
DEAD = {"FPC_W4_MODE": "3", "FPC_H2_MODE": "3", "FPC_W2_MODE": "3", "FPC_H3_VAR": "1", "FPC_H3_ORIENT_G1": "1"}


def _operands():
    g = torch.Generator().manual_seed(20)
    x = torch.randn((B, CIN, H, W), generator=g)
    w = torch.randn((COUT, CIN, 3, 3), generator=g) / (CIN * 9) ** 0.5
    return x, w, torch.rand(COUT, generator=g) + 0.5, torch.randn(COUT, generator=g)


def _conv(dev, x, w, scale, shift, form, relu):
    """3x3 / stride 1 / pad 1 with folded BatchNorm and GroupNorm records, both preset to NaN.  Returns (out NHWC, records) on the host."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    xd, wd, sd, hd = x.permute(0, 2, 3, 1).contiguous().to(dev), w.contiguous().to(dev), scale.to(dev), shift.to(dev)
    plan = (ctypes.c_int * 4)()
    nat.check(L.fpc_conv2d_plan(B, H, W, CIN, COUT, 3, 3, 0, 0, form, plan), "plan")
    out = torch.full((B, H, W, COUT), float("nan"), device=dev)
    rec = torch.full((B, plan[3], COUT, 2), float("nan"), device=dev)
    ws = torch.empty(L.fpc_conv2d_workspace_bytes(B, H, W, CIN, COUT, 3, 3), dtype=torch.uint8, device=dev)
    sb, sh, sw, sc = xd.stride()
    nat.check(L.fpc_conv2d(xd.data_ptr(), sb, sh, sw, sc, wd.data_ptr(), sd.data_ptr(), hd.data_ptr(), None, None, out.data_ptr(),
                           rec.data_ptr(), B, H, W, CIN, COUT, 3, 3, 1, 1, relu, 0, 0, form, ws.data_ptr(), ws.numel(), nat.stream()), "conv2d")
    torch.cuda.synchronize()
    return out.cpu(), rec.cpu()


def _child(check):
    """Prints one line per form: the SHA-256 of the output and of the records; `check`: also holds the output to float64."""
    dev = torch.device("cuda:0")
    x, w, scale, shift = _operands()
    ref = (F.conv2d(x.double(), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).relu()
    for form in FORMS:
        out, rec = _conv(dev, x, w, scale, shift, form, 1)
        print("HASH", form, hashlib.sha256(out.numpy().tobytes()).hexdigest(), hashlib.sha256(rec.numpy().tobytes()).hexdigest())
        if check:
            assert not torch.isnan(out).any() and not torch.isnan(rec).any(), form
            err = (out.permute(0, 3, 1, 2).double() - ref).abs().max().item()
            print("float64 error", form, err)
            assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (form, err)      # test_gpu_net.py's bar, the same for every form


def _run_child(extra_env, check):
    env = {k: v for k, v in os.environ.items() if k not in DEAD}
    env.update(extra_env)
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "check" if check else "hash"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = [l for l in p.stdout.splitlines() if l.startswith("HASH")]
    assert len(lines) == len(FORMS), p.stdout + p.stderr
    return lines


def test_diagnostic_environment_variables_are_dead():
    plain = _run_child({}, True)
    with_vars = _run_child(DEAD, False)
    print("\n".join(plain))
    assert with_vars == plain


def test_relu_77_is_relu_on_and_gn_part_stays_the_record_buffer():
    dev = torch.device("cuda:0")
    x, w, scale, shift = _operands()
    out1, rec1 = _conv(dev, x, w, scale, shift, -7, 1)
    out77, rec77 = _conv(dev, x, w, scale, shift, -7, 77)
    assert not torch.isnan(out1).any() and not torch.isnan(rec1).any() and (out1 >= 0).all() and (out1 == 0).any()
    assert torch.equal(out77.view(torch.int32), out1.view(torch.int32)) and torch.equal(rec77.view(torch.int32), rec1.view(torch.int32))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child(sys.argv[1] == "check")
