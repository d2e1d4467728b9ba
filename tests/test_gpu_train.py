"""Training side (BASELINE config 5): the native backward kernels against torch autograd over a
restatement of the reference's differentiable forward (F/lib/gpu_tensor_funcs.py:52-99, F/lib/aggregation_layer.py:119-156,
RV/ransac_voting_gpu.py:583-599), and the fused optimiser step against the published algorithms."""
import math

import numpy as np
import pytest
import torch

from _train_refs import radam_lookahead_reference as _radam_lookahead_reference

pytestmark = pytest.mark.gpu


def _logits_from_frames(frames, G=6, noise=0.05):
    """Logit tensors whose class compression reproduces the vote-bench fixture (plus noise on the other classes)."""
    from fastposecnn_amd import synth
    cat, _ = synth.make_vote_batch(frames, H=192, W=256, rmin=14.0, rmax=40.0, K=4)
    B, H, W = cat["mask"].shape
    g = torch.Generator().manual_seed(7)
    onehot = torch.nn.functional.one_hot(cat["mask"], G + 1).permute(0, 3, 1, 2).float()
    logits = {"mask": onehot * 8.0 + torch.randn((B, G + 1, H, W), generator=g) * 0.1}
    for key, a in (("quaternion", 4), ("scales", 3), ("xy", 2), ("z", 1)):
        v = cat[key] if key != "z" else cat[key].unsqueeze(1)
        full = torch.randn((B, G, a, H, W), generator=g) * noise
        sel = torch.nn.functional.one_hot((cat["mask"] - 1).clamp(min=0), G).permute(0, 3, 1, 2).unsqueeze(2).float()
        scale = 1.7 if key in ("quaternion", "xy") else 1.0          # un-normalised logits: exercises the Jacobian
        full = full + sel * (v.unsqueeze(1) * scale)
        logits[key] = full.reshape(B, G * a, H, W)
    return logits, cat


def _reference_forward(logits, cat_mask, labels, N, winners, thresh, orc, native_xy):
    """Differentiable restatement (torch ops, float64) given the forward's discrete choices: class map, instance labels,
    winning hypotheses.  The inlier set of the refinement comes from the oracle's voting kernel (exact)."""
    import fastposecnn_amd.lib  # noqa: F401  (puts lib/ on sys.path)
    import gpu_tensor_funcs as gtf
    cat = gtf._class_compress_cpu(7, cat_mask, {k: v for k, v in logits.items()})
    B, H, W = cat_mask.shape
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    out = {"quaternion": [], "scales": [], "z": [], "xy": []}
    for i in range(N):
        m = labels == (i + 1)
        b = int(torch.nonzero(m)[0, 0])
        mb = m[b]
        cnt = mb.sum()
        q = (cat["quaternion"][b].double() * mb).sum(dim=(-2, -1)) / cnt
        out["quaternion"].append(q / q.norm())
        out["scales"].append((cat["scales"][b].double() * mb).sum(dim=(-2, -1)) / cnt)
        out["z"].append(torch.exp((cat["z"][b].double() * mb).sum() / cnt).reshape(1))
        # refinement over the winner's inliers
        d = cat["xy"][b].double()[:, mb].T                         # [tn,2]
        coords = torch.stack([xx[mb], yy[mb]], dim=1)
        inl = np.zeros((1, 1, d.shape[0]), np.uint8)
        d32 = native_xy[b][:, mb].T.contiguous().numpy()            # the f32 values the kernels voted on
        orc.voting_for_hypothesis(d32[:, None, :], coords.float().numpy(),
                                  winners[i].reshape(1, 1, 2).astype(np.float32), inl, thresh)
        w = torch.from_numpy(inl[0, 0].astype(np.float64))
        if cnt < 5:
            out["xy"].append(torch.zeros(2, dtype=torch.float64))
            continue
        normal = torch.stack([d[:, 1], -d[:, 0]], dim=1) * w[:, None]
        bb = (normal * coords).sum(dim=1)
        ATA = normal.T @ normal
        ATb = (normal * bb[:, None]).sum(dim=0)
        out["xy"].append(torch.linalg.solve(ATA, ATb))
    return cat, {k: torch.stack(v) for k, v in out.items()}


def test_post_network_backward_matches_autograd(oracle):
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    import train_functions as tf
    hp = config.HEAD_TRAINING()
    hp.HV_NUM_OF_HYPOTHESES = 128
    torch.manual_seed(0)
    model = L.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).cuda()
    logits_cpu, _ = _logits_from_frames(range(2))
    logits = {k: v.cuda().requires_grad_(k != "mask") for k, v in logits_cpu.items()}
    cat = tf.class_compression_train(7, logits)
    agg = tf.post_network_train(model, cat, seed=1234)
    N = agg["class_ids"].shape[0]
    assert N >= 6
    g = torch.Generator().manual_seed(3)
    wts = {k: torch.randn(agg[k].shape, generator=g) for k in ("quaternion", "scales", "xy", "z")}
    wts["xy"] *= 0.05
    pix = {k: torch.randn(cat[k].shape, generator=g) * 1e-4 for k in ("quaternion", "scales", "xy", "z")}   # pixel-wise term
    loss = sum((agg[k] * wts[k].cuda()).sum() for k in wts) + sum((cat[k] * pix[k].cuda()).sum() for k in pix)
    loss.backward()

    # the same loss through torch autograd over the restated forward
    ref_logits = {k: v.detach().cpu().double().requires_grad_(k != "mask") for k, v in logits.items()}
    labels, n_lab = model.aggregation_layer.batchwise_break_segmentation_mask(cat["mask"])
    assert n_lab == N
    # winners: re-run the vote with the same seed and read the refinement record
    refine = torch.zeros((N, 1, 8), dtype=torch.float64, device="cuda")
    import ransac_voting_gpu_layer.ransac_voting_gpu as rvg
    vertex = torch.unsqueeze(agg["xy_mask"].permute(0, 2, 3, 1), dim=3)
    voted = rvg.ransac_voting_layer_v3(agg["instance_masks"], vertex, 128, seed=1234, refine_out=refine)
    torch.testing.assert_close(voted[:, 0, :], agg["xy"].detach())
    winners = refine[:, 0, 0:2].cpu().numpy()
    rcat, ragg = _reference_forward(ref_logits, cat["mask"].cpu(), labels.cpu(), N, winners, 0.999, oracle,
                                     cat["xy"].detach().cpu())
    for k in ("quaternion", "scales", "z", "xy"):
        torch.testing.assert_close(agg[k].detach().cpu().double().reshape(ragg[k].shape), ragg[k], rtol=2e-4, atol=2e-4)
    rloss = sum((ragg[k] * wts[k].double().reshape(ragg[k].shape)).sum() for k in wts) + \
        sum((rcat[k] * pix[k].double()).sum() for k in pix)
    rloss.backward()
    for k in ("quaternion", "scales", "xy", "z"):
        got, want = logits[k].grad.cpu().double(), ref_logits[k].grad
        assert torch.isfinite(got).all()
        scale = want.abs().max().item()
        assert scale > 0
        err = (got - want).abs().max().item()
        assert err <= 2e-4 * scale + 1e-9, (k, err, scale)
        # gradients only inside the arg-max class's channel group of foreground pixels
        assert (got != 0).sum() > 0


def test_vote_refine_fn_matches_autograd(oracle):
    import fastposecnn_amd.lib  # noqa: F401
    import train_functions as tf
    from fastposecnn_amd import synth
    cat, _ = synth.make_vote_batch(range(1), H=192, W=256, rmin=14.0, rmax=40.0, K=3)
    labels = torch.zeros((192, 256), dtype=torch.int64)
    # instance planes from the class map (one instance per class in this fixture)
    masks, verts = [], []
    for c in torch.unique(cat["mask"]):
        if c == 0:
            continue
        m = (cat["mask"][0] == c)
        masks.append(m.float())
        verts.append(cat["xy"][0] * m)
    mask = torch.stack(masks).cuda()
    v = torch.stack(verts).cuda().requires_grad_(True)                       # [n,2,H,W]
    vertex = v.permute(0, 2, 3, 1).unsqueeze(3)
    out = tf.VoteRefineFn.apply(mask, vertex, 64, 0.999, 5, 30000, 99)
    w = torch.tensor([[0.3, -0.7]], device="cuda")
    (out[:, 0, :] * w).sum().backward()
    got = v.grad.cpu().double()
    # autograd over the least squares with the oracle's inlier set for the same winner
    import ransac_voting_gpu_layer.ransac_voting_gpu as rvg
    refine = torch.zeros((mask.shape[0], 1, 8), dtype=torch.float64, device="cuda")
    rvg.ransac_voting_layer_v3(mask, vertex.detach(), 64, seed=99, refine_out=refine)
    yy, xx = torch.meshgrid(torch.arange(192, dtype=torch.float64), torch.arange(256, dtype=torch.float64), indexing="ij")
    vr = v.detach().cpu().double().requires_grad_(True)
    total = 0
    for i in range(mask.shape[0]):
        mb = mask[i].cpu() != 0
        d = vr[i][:, mb].T
        coords = torch.stack([xx[mb], yy[mb]], dim=1)
        inl = np.zeros((1, 1, d.shape[0]), np.uint8)
        oracle.voting_for_hypothesis(d.detach().float().numpy()[:, None, :], coords.float().numpy(),
                                     refine[i, 0, 0:2].cpu().numpy().reshape(1, 1, 2).astype(np.float32), inl, 0.999)
        wi = torch.from_numpy(inl[0, 0].astype(np.float64))
        normal = torch.stack([d[:, 1], -d[:, 0]], dim=1) * wi[:, None]
        x = torch.linalg.solve(normal.T @ normal, (normal * (normal * coords).sum(dim=1)[:, None]).sum(dim=0))
        total = total + (x * w[0].cpu().double()).sum()
    total.backward()
    want = vr.grad
    scale = want.abs().max().item()
    assert scale > 0 and (got - want).abs().max().item() <= 2e-4 * scale


def test_lookahead_radam_kernel():
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    n = 100003
    g = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(13)]
    want = _radam_lookahead_reference(p0, grads, 1e-3, (0.9, 0.999), 1e-8, 3e-4, 5, 0.5)
    p = p0.cuda()
    m, v, slow = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    for step, gr in enumerate(grads, start=1):
        gd = gr.cuda()
        nat.check(L.fpc_lookahead_radam_step(nat.ptr(p), nat.ptr(gd), nat.ptr(m), nat.ptr(v), nat.ptr(slow), n, 1e-3, 0.9, 0.999,
                                             1e-8, 3e-4, step, 5, 0.5, None, nat.stream()), "radam")
    torch.testing.assert_close(p.cpu().double(), want, rtol=2e-5, atol=2e-6)
    # ctl: gradient scale and the skip flag
    ctl = torch.tensor([0.5, 0.0], device="cuda")
    p1, p2 = p0.cuda(), p0.cuda()
    z = [torch.zeros_like(p1) for _ in range(6)]
    gd = grads[0].cuda()
    nat.check(L.fpc_lookahead_radam_step(nat.ptr(p1), nat.ptr(gd), nat.ptr(z[0]), nat.ptr(z[1]), nat.ptr(z[2]), n, 1e-3, 0.9, 0.999,
                                         1e-8, 0.0, 1, 5, 0.5, nat.ptr(ctl), nat.stream()), "radam")
    gh = (grads[0] * 0.5).cuda()
    nat.check(L.fpc_lookahead_radam_step(nat.ptr(p2), nat.ptr(gh), nat.ptr(z[3]), nat.ptr(z[4]), nat.ptr(z[5]), n, 1e-3, 0.9, 0.999,
                                         1e-8, 0.0, 1, 5, 0.5, None, nat.stream()), "radam")
    torch.testing.assert_close(p1, p2)
    # the guard (ctl[1] != 0): the step runs with a ZERO gradient, as the reference's zero_grad() + optimizer.step() does
    # (F/lib/pose_regressor.py:341-415) - the gradient it is given holds inf / NaN and must not leak through a product
    ctl[1] = 1.0
    bad = gd.clone(); bad[::7] = float("inf"); bad[3::11] = float("nan")
    zero = torch.zeros_like(gd)
    nat.check(L.fpc_lookahead_radam_step(nat.ptr(p1), nat.ptr(bad), nat.ptr(z[0]), nat.ptr(z[1]), nat.ptr(z[2]), n, 1e-3, 0.9, 0.999,
                                         1e-8, 3e-4, 2, 5, 0.5, nat.ptr(ctl), nat.stream()), "radam")
    nat.check(L.fpc_lookahead_radam_step(nat.ptr(p2), nat.ptr(zero), nat.ptr(z[3]), nat.ptr(z[4]), nat.ptr(z[5]), n, 1e-3, 0.9, 0.999,
                                         1e-8, 3e-4, 2, 5, 0.5, None, nat.stream()), "radam")
    assert torch.isfinite(p1).all() and torch.equal(p1, p2) and torch.equal(z[0], z[3]) and torch.equal(z[1], z[4])


def test_grad_sumsq_kernel():
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    g = torch.randn(1000003, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.zeros(2, dtype=torch.float64, device="cuda")
    nat.check(L.fpc_grad_sumsq(nat.ptr(g), g.numel(), nat.ptr(out), nat.stream()), "sumsq")
    assert abs(out[0].item() - (g.double() ** 2).sum().item()) <= 1e-9 * out[0].item()
    assert out[1].item() == 0
    g[12345] = float("inf")
    out.zero_()
    nat.check(L.fpc_grad_sumsq(nat.ptr(g), g.numel(), nat.ptr(out), nat.stream()), "sumsq")
    assert out[1].item() > 0
    g[12345] = float("nan")
    out.zero_()
    nat.check(L.fpc_grad_sumsq(nat.ptr(g), g.numel(), nat.ptr(out), nat.stream()), "sumsq")
    assert out[1].item() > 0


def test_train_step_bench_line_and_two_ranks_on_one_gpu():
    """`bench.py --train`: the whole config-5 step (network forward/backward through torch modules, post-network forward and
    backward through the HIP kernels, losses, sharded optimiser).  Two ranks share this box's one GPU over gloo (RCCL needs
    one device per rank): the bucket reduction, the sharded step and the parameter all-gather run for real, and the ranks
    must end with identical parameters."""
    import json, os, subprocess, sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FPC_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--train", "--gpus", "2", "--steps", "3", "--warmup", "2",
                        "--train-batch", "1", "--bucket-mb", "8"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 2 and line["value"] > 0
    chk = line["step_check"]
    assert chk["replicas_in_sync"] and chk["skipped_steps"] == 0 and chk["matched_instances"] >= 4
    assert math.isfinite(chk["total_loss"]) and chk["total_loss"] > 0
    for task in ("mask", "quaternion", "xy", "z", "scales"):
        assert chk["losses"][task]["task_total_loss"] is not None
    assert line["config"]["buckets"] >= 2


def test_fused_mask_losses_match_torch_forms(monkeypatch):
    """k_mask_losses (CE + CCE + Focal, forward sums and combined gradient) against the torch-op forms of lib/loss.py
    (CE / CCE pinned by the reference's goldens, Focal = pytorch_toolbelt's published formula) incl. ignored pixels."""
    import fastposecnn_amd.lib  # noqa: F401
    import loss as L
    g = torch.Generator().manual_seed(11)
    B, C, H, W = 3, 7, 37, 53
    x0 = torch.randn((B, C, H, W), generator=g) * 3
    t = torch.randint(0, C, (B, H, W), generator=g)
    res = {}
    for fused in ("0", "1"):
        monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", fused)
        x = x0.clone().cuda().requires_grad_(True)
        pred, gt = {"logits": {"mask": x}}, {"mask": t.cuda()}
        vals = [L.CE()(pred, gt), L.CCE()(pred, gt), L.Focal()(pred, gt)]
        (5.0 * vals[0] + 3.0 * vals[1] + 7.0 * vals[2]).backward()
        res[fused] = ([float(v.detach()) for v in vals], x.grad.clone())
    for a, b in zip(res["0"][0], res["1"][0]):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a)), (res["0"][0], res["1"][0])
    g0, g1 = res["0"][1], res["1"][1]
    assert (g0 - g1).abs().max().item() <= 2e-5 * g0.abs().max().item()
    # the three objects share one forward launch per (logits, target)
    monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", "1")
    x = x0.clone().cuda().requires_grad_(True)
    pred, gt = {"logits": {"mask": x}}, {"mask": t.cuda()}
    L.CE()(pred, gt)
    first = x._fpc_mask_losses[3][2]
    L.CCE()(pred, gt); L.Focal()(pred, gt)
    assert x._fpc_mask_losses[3][2] is first
    # ignored pixels (target -1) leave CCE and Focal, as nn.NLLLoss(ignore_index=-1) / toolbelt do
    t2 = t.clone(); t2[0, :5] = -1
    monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", "0")
    xa = x0.clone().cuda().requires_grad_(True)
    want = [L.CCE()({"logits": {"mask": xa}}, {"mask": t2.cuda()}), L.Focal()({"logits": {"mask": xa}}, {"mask": t2.cuda()})]
    (want[0] + want[1]).backward()
    monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", "1")
    xb = x0.clone().cuda().requires_grad_(True)
    got = [L.CCE()({"logits": {"mask": xb}}, {"mask": t2.cuda()}), L.Focal()({"logits": {"mask": xb}}, {"mask": t2.cuda()})]
    (got[0] + got[1]).backward()
    for a, b in zip(want, got):
        assert abs(float(a) - float(b)) <= 2e-6 * max(1.0, abs(float(a)))
    assert (xa.grad - xb.grad).abs().max().item() <= 2e-5 * xa.grad.abs().max().item()


# ---- convolutions of the training step (lib/train_conv.py, csrc/conv_wgrad.hip) ------------------------------------------

TRAIN_CONV_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad, bias
    (2, 64, 30, 40, 64, 3, 1, 1, False),        # encoder block: Winograd candidates forward and for the data gradient
    (2, 64, 30, 40, 128, 3, 2, 1, False),       # stride 2: data gradient as four parity convolutions of dy (round 4)
    (2, 64, 30, 40, 128, 1, 2, 0, False),       # 1x1 shortcut, stride 2
    (2, 128, 16, 24, 256, 3, 2, 1, True),       # stride 2 deeper in the encoder
    (2, 64, 15, 20, 128, 3, 2, 1, False),       # odd height: the parity form does not apply, aten's data gradient
    (3, 128, 15, 20, 256, 1, 1, 0, True),       # FPN lateral: 1x1 + bias
    (2, 256, 15, 20, 128, 3, 1, 1, False),      # decoder block
    (1, 128, 17, 23, 7, 1, 1, 0, True),         # odd-width head: dy and W zero-padded to 32 channels, both gradients native (round 4)
    (1, 128, 17, 23, 24, 1, 1, 0, True),        # head with Cout % 4 == 0 but not % 32
    (2, 128, 12, 16, 18, 1, 1, 0, True),        # scales / xyz heads
    (2, 64, 9, 11, 68, 3, 1, 1, True),          # Cout not a multiple of the 64-row tile, pixel count not a multiple of 32
    (2, 256, 6, 8, 256, 3, 1, 1, False),        # the small maps of a 96 x 128 input: fewer pixels than one tile
    (2, 512, 3, 4, 512, 3, 1, 1, False),
    (2, 128, 12, 16, 128, 3, 1, 1, False),
]


@pytest.mark.parametrize("case", TRAIN_CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_training_conv_forward_and_gradients_vs_float64_autograd(case):
    from fastposecnn_amd.lib import train_conv
    B, Cin, H, W, Cout, k, stride, pad, has_bias = case
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn((B, Cin, H, W), generator=g)
    w = torch.randn((Cout, Cin, k, k), generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) if has_bias else None
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if has_bias else None
    yr = torch.nn.functional.conv2d(xr, wr, br, stride, pad)
    gy = torch.randn(yr.shape, generator=g)
    yr.backward(gy.double())

    xd, wd = x.to(dev).requires_grad_(), w.to(dev).requires_grad_()
    bd = b.to(dev).requires_grad_() if has_bias else None
    before = dict(train_conv.counters)
    y = train_conv.conv2d(xd, wd, bd, stride, pad)
    y.backward(gy.to(dev))
    torch.cuda.synchronize()
    assert train_conv.counters["fwd_native"] == before["fwd_native"] + 1           # not the torch fallback

    def close(got, ref, what, rel):
        err = (got.detach().cpu().double() - ref).abs().max().item()
        assert err <= rel * max(1.0, ref.abs().max().item()), (what, err)

    close(y, yr.detach(), "y", 2e-5)
    close(xd.grad, xr.grad, "dx", 2e-5)
    close(wd.grad, wr.grad, "dw", 1e-4)          # sums over B*Ho*Wo pixels in f32
    if has_bias:
        close(bd.grad, br.grad, "db", 1e-4)
    native_w = Cin % 64 == 0
    native_x = stride == 1 or (H % 2 == 0 and W % 2 == 0)
    assert train_conv.counters["wgrad_native"] - before["wgrad_native"] == int(native_w)
    assert train_conv.counters["dgrad_native"] - before["dgrad_native"] == int(native_x)
    assert train_conv.counters["dgrad_aten"] - before["dgrad_aten"] == int(not native_x)


def test_wgrad_is_deterministic_and_refuses_unsupported_shapes():
    import ctypes
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    B, Cin, H, W, Cout, k = 4, 64, 60, 80, 64, 3          # 9 tiles, 19200 pixels: a deep split
    x = torch.randn((B, H, W, Cin), generator=g).to(dev)
    dy = torch.randn((B, H, W, Cout), generator=g).to(dev)
    ws = torch.empty(L.fpc_conv2d_wgrad_workspace_bytes(B, H, W, Cin, Cout, k, k), dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        dw = torch.full((Cout, Cin, k, k), float("nan"), device=dev)
        nat.check(L.fpc_conv2d_wgrad(x.data_ptr(), H * W * Cin, W * Cin, Cin, dy.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout, k, k, 1, 1,
                                     ws.data_ptr(), ws.numel(), nat.stream()), "wgrad")
        outs.append(dw.clone())
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and not torch.isnan(outs[0]).any()
    rc = L.fpc_conv2d_wgrad(x.data_ptr(), H * W * Cin, W * Cin, Cin, dy.data_ptr(), outs[0].data_ptr(), B, H, W, 48, Cout, k, k, 1, 1,
                            ws.data_ptr(), ws.numel(), nat.stream())
    assert rc == -1                                        # FPC_EINVAL: Cin % 64 != 0
    rc = L.fpc_conv2d_wgrad(x.data_ptr(), H * W * Cin, W * Cin, Cin, dy.data_ptr(), outs[0].data_ptr(), B, H, W, Cin, Cout, k, k, 1, 1,
                            ws.data_ptr(), 16, nat.stream())
    assert rc == -2                                        # FPC_EWORKSPACE


@pytest.mark.parametrize("shape", [(2, 128, 30, 40, 128, 3, 1, 1), (2, 64, 33, 47, 128, 3, 2, 1), (3, 128, 20, 24, 64, 1, 1, 0),
                                   (2, 64, 24, 40, 36, 3, 1, 1)])
def test_wgrad_split_precision_matches_float64_like_the_f32_form(shape):
    """fpc_conv2d_wgrad_split (three bf16 pieces per operand, six piece products) against the float64 weight gradient:
    its error is at the level of the plain-f32 matrix form's (both are f32 accumulations of ~10^3..10^4 terms)."""
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    dev = torch.device("cuda:0")
    B, Cin, H, W, Cout, k, stride, pad = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, Cin, H, W), generator=g)
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dy = torch.randn((B, Cout, Ho, Wo), generator=g)
    w64 = torch.zeros((Cout, Cin, k, k), dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x.double(), w64, None, stride, pad).backward(dy.double())
    ref = w64.grad
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev)
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev)
    ws = torch.empty(L.fpc_conv2d_wgrad_workspace_bytes(B, Ho, Wo, Cin, Cout, k, k), dtype=torch.uint8, device=dev)
    errs = {}
    for name in ("fpc_conv2d_wgrad", "fpc_conv2d_wgrad_split"):
        outs = []
        for _ in range(2):
            dw = torch.full((Cout, Cin, k, k), float("nan"), device=dev)
            nat.check(getattr(L, name)(xd.data_ptr(), H * W * Cin, W * Cin, Cin, dyd.data_ptr(), dw.data_ptr(), B, H, W, Cin, Cout, k, k,
                                       stride, pad, ws.data_ptr(), ws.numel(), nat.stream()), name)
            outs.append(dw.clone())
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1])                              # deterministic
        errs[name] = float((outs[0].cpu().double() - ref).abs().max() / ref.abs().max())
    assert errs["fpc_conv2d_wgrad"] <= 2e-6, errs
    assert errs["fpc_conv2d_wgrad_split"] <= 2e-6, errs                   # f32-level: 1e-4 is the bar, this is 50x inside it
    assert errs["fpc_conv2d_wgrad_split"] <= 4 * errs["fpc_conv2d_wgrad"] + 2e-7, errs


def test_training_mode_model_uses_native_convolutions_and_matches_torch_path():
    """One forward + backward of the whole network in training mode (BatchNorm on batch statistics): native convolutions
    and the same model on torch's f32 kernels, each against the model in float64.  Two f32 implementations differ from
    each other by rounding amplified through ~40 layers; the claim checked is that the native path is as close to the
    float64 gradients as torch's own f32 path is."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config, synth
    from fastposecnn_amd.lib import train_conv
    dev = torch.device("cuda:0")
    hp = config.HEAD_TRAINING()
    hp.RUNTIME_TIMING = False
    torch.manual_seed(0)
    model = L.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).to(dev).train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0                                      # the passes must see the same network
        # ReLU's derivative jumps at 0: a pre-activation within rounding of 0 gets another mask in another f32
        # implementation and the gradients downstream differ by O(1) for that unit (seen at encoder.layer3.0, while every
        # convolution agreed with aten to 1e-6 on identical inputs: tools_dev/train_conv_check.py).  A smooth activation
        # keeps the comparison about the arithmetic of the convolutions.
        for name, child in list(m.named_children()):
            if isinstance(child, torch.nn.ReLU):
                setattr(m, name, torch.nn.Softplus())
    x = torch.stack([synth.make_image(i, 96, 128) for i in range(2)]).to(dev)
    res = {}
    for tag in ("native", "torch32", "torch64"):
        train_conv.ENABLED = tag == "native"
        try:
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
        finally:
            train_conv.ENABLED = True
    ln, on, gn, used = res["native"]
    lt, ot, gt, unused = res["torch32"]
    lr, orf, gr, _ = res["torch64"]
    assert used["fwd_native"] >= 50 and used["wgrad_native"] >= 45 and used["dgrad_native"] >= 40, used
    assert used["dgrad_aten"] == 0 and used["wgrad_aten"] == 0, used      # round 4: stride-2 data gradients and odd-width heads native too
    assert unused["fwd_native"] == 0
    assert abs(ln - lr) <= 1e-5 * max(1.0, abs(lr))
    for k in orf:
        tol = 1e-4 * max(1.0, orf[k].abs().max().item())
        assert (on[k] - orf[k]).abs().max().item() <= tol, k
    assert set(gn) == set(gr)
    err_n = err_t = 0.0
    for n in gr:
        scale = max(gr[n].abs().max().item(), 1e-12)
        err_n = max(err_n, (gn[n] - gr[n]).abs().max().item() / scale)
        err_t = max(err_t, (gt[n] - gr[n]).abs().max().item() / scale)
    assert err_n <= max(2.0 * err_t, 1e-4), (err_n, err_t)


@pytest.mark.parametrize("case", [(2, 128, 15, 20, 2, "nhwc"), (2, 7, 30, 40, 4, "nhwc->nchw"), (1, 24, 12, 16, 4, "nchw"),
                                  (3, 5, 3, 4, 2, "nchw"), (1, 6, 1, 9, 4, "nhwc->nchw"), (2, 128, 2, 3, 2, "nhwc"), (2, 6, 5, 7, 2, "nchw"), (1, 12, 30, 40, 4, "nhwc"),
                                  (2, 3, 17, 24, 4, "nchw")],
                         ids=lambda c: "x".join(str(v) for v in c))
def test_native_bilinear_upsample_forward_and_adjoint_vs_torch(case):
    from fastposecnn_amd.lib import train_conv
    B, C, h, w, scale, layout = case
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn((B, C, h, w), generator=g)
    gy = torch.randn((B, C, h * scale, w * scale), generator=g)
    xr = x.double().requires_grad_()
    yr = torch.nn.functional.interpolate(xr, scale_factor=scale, mode="bilinear", align_corners=True)
    yr.backward(gy.double())
    xd = x.to(dev)
    if layout.startswith("nhwc"):
        xd = xd.contiguous(memory_format=torch.channels_last)
    xd.requires_grad_()
    y = train_conv.upsample_bilinear(xd, scale, out_nchw=layout.endswith("nchw"))
    assert y.is_contiguous(memory_format=torch.channels_last if layout == "nhwc" else torch.contiguous_format)
    gd = gy.to(dev)
    if layout == "nhwc":
        gd = gd.contiguous(memory_format=torch.channels_last)
    y.backward(gd)
    torch.cuda.synchronize()
    # the source coordinate r * o is an f32 product (ATen's arithmetic, kept): ~1e-5 of a pixel at o ~ 500
    assert (y.detach().cpu().double() - yr.detach()).abs().max().item() <= 2e-5 * max(1.0, yr.abs().max().item())
    assert (xd.grad.cpu().double() - xr.grad).abs().max().item() <= 2e-5 * max(1.0, xr.grad.abs().max().item())
    # same numbers as torch's own f32 kernel (the network's evaluation path) to rounding
    yt = torch.nn.functional.interpolate(x.to(dev), scale_factor=scale, mode="bilinear", align_corners=True)
    assert (y.detach() - yt).abs().max().item() <= 1e-6 * max(1.0, yt.abs().max().item())


@pytest.mark.parametrize("case", [(2, 128, 15, 20), (3, 128, 33, 17), (1, 64, 7, 5), (2, 256, 24, 32)], ids=str)
def test_native_groupnorm_relu_forward_and_backward_vs_float64(case):
    from fastposecnn_amd.lib import train_conv
    B, C, H, W = case
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn((B, C, H, W), generator=g) * 1.5 + 0.7          # a mean that is not small against the spread
    gy = torch.randn((B, C, H, W), generator=g)
    gn = torch.nn.GroupNorm(C // 4, C)
    gn.weight.data = torch.rand(C, generator=g) + 0.5
    gn.bias.data = torch.randn(C, generator=g) * 0.3
    ref = torch.nn.GroupNorm(C // 4, C).double()
    ref.weight.data, ref.bias.data = gn.weight.data.double(), gn.bias.data.double()
    xr = x.double().requires_grad_()
    yr = torch.relu(ref(xr))
    yr.backward(gy.double())
    gn = gn.to(dev)
    xd = x.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_()
    y = train_conv.groupnorm_relu(xd, gn)
    assert y.is_contiguous(memory_format=torch.channels_last) and y.grad_fn.__class__.__name__.startswith("_GroupNormReLUFn")
    y.backward(gy.to(dev).contiguous(memory_format=torch.channels_last))
    torch.cuda.synchronize()

    def close(got, want, what, rel=2e-5):
        err = (got.detach().cpu().double() - want).abs().max().item()
        assert err <= rel * max(1.0, want.abs().max().item()), (what, err)

    # elements whose pre-activation is within rounding of 0 may take the other side of the ReLU: compare away from it
    z = ref(x.double()).detach()
    safe = (z.abs() > 1e-4)
    close(y.detach().cpu().double() * safe, yr.detach() * safe, "y")
    if bool(safe.all()):
        close(xd.grad, xr.grad, "dx", 1e-4)
        close(gn.weight.grad, ref.weight.grad, "dgamma", 1e-4)
        close(gn.bias.grad, ref.bias.grad, "dbeta", 1e-4)
    else:                      # a flipped unit changes the group's sums: compare against torch with the native mask instead
        mask = (y.detach().cpu() > 0).double()
        xr2 = x.double().requires_grad_()
        z2 = ref(xr2)
        ref.zero_grad()
        (z2 * mask).backward(gy.double())
        close(xd.grad, xr2.grad, "dx", 1e-4)
        close(gn.weight.grad, ref.weight.grad, "dgamma", 1e-4)
        close(gn.bias.grad, ref.bias.grad, "dbeta", 1e-4)


def test_native_groupnorm_statistics_survive_a_large_offset():
    """activations with |mean| >> std.  E[x^2] - mean^2 from f32 partial sums cancels to nothing there (variance
    clamped to 0, rstd blown up); the per-chunk centred sums combined by Chan's formula track the float64 statistics."""
    from fastposecnn_amd.lib import train_conv
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    B, C, H, W = 2, 128, 40, 56
    x = torch.randn((B, C, H, W), generator=g) * 0.05 + 100.0
    gn = torch.nn.GroupNorm(C // 4, C)
    ref = torch.nn.GroupNorm(C // 4, C).double()
    want = torch.relu(ref(x.double()))
    y = train_conv.groupnorm_relu(x.to(dev).contiguous(memory_format=torch.channels_last), gn.to(dev))
    torch.cuda.synchronize()
    # x itself carries 100 * 2^-24 = 6e-6 of f32 rounding against a spread of 0.05: 2e-4 of a normalised unit
    err = (y.cpu().double() - want).abs().max().item()
    assert err <= 2e-3, err
    assert abs(y.cpu().double().std().item() - want.std().item()) <= 1e-3


def test_fpn_block_fused_lateral_conv_and_merge_matches_float64():
    """FPNBlock in training mode: skip_conv(skip) + nearest_x2(top) as one native launch (train_conv.conv2d_up_add), forward
    and all three gradients against the same block in float64."""
    from fastposecnn_amd.lib import backbone, train_conv
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    blk = backbone.FPNBlock(128, 64).to(dev).train()
    top = torch.randn((2, 128, 15, 20), generator=g).to(dev).requires_grad_()
    skip = torch.randn((2, 64, 30, 40), generator=g).to(dev).requires_grad_()
    gy = torch.randn((2, 128, 30, 40), generator=g).to(dev)
    before = train_conv.counters["fwd_native"]
    y = blk(top, skip)
    assert train_conv.counters["fwd_native"] == before + 1 and y.grad_fn.name().startswith("_ConvUpAddFn")
    y.backward(gy)
    w64 = blk.skip_conv.weight.detach().double().requires_grad_()
    b64 = blk.skip_conv.bias.detach().double().requires_grad_()
    t64, s64 = top.detach().double().requires_grad_(), skip.detach().double().requires_grad_()
    r = torch.nn.functional.interpolate(t64, scale_factor=2, mode="nearest") + torch.nn.functional.conv2d(s64, w64, b64)
    r.backward(gy.double())

    def close(a, b, what, tol):
        err = float((a.double() - b).abs().max() / b.abs().max())
        assert err <= tol, (what, err)
    close(y, r, "forward", 2e-6)
    close(top.grad, t64.grad, "d top", 2e-6)
    close(skip.grad, s64.grad, "d skip", 2e-5)
    close(blk.skip_conv.weight.grad, w64.grad, "d weight", 2e-5)
    close(blk.skip_conv.bias.grad, b64.grad, "d bias", 2e-5)
