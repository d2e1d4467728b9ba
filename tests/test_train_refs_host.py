"""The float64 references of tests/_train_refs.py checked on the CPU: against lib/loss.py's own torch-op classes in float64,
against autograd, against the CPU oracle's thinning, and (the tolerances of tests/test_gpu_train_kernels.py rest on this)
the float32 evaluation of the same formulas measured against them at every case the kernels are held to."""
import math

import numpy as np
import pytest
import torch

import _train_refs as R


def test_mask_loss_sums_match_lib_loss_in_float64(monkeypatch):
    import fastposecnn_amd.lib  # noqa: F401  (puts lib/ on sys.path)
    import loss as L
    monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", "0")
    g = torch.Generator().manual_seed(5)
    for sigma, frac in ((3.0, 0.0), (3.0, 0.2), (20.0, 0.2)):
        B, C, H, W = 2, 7, 13, 17
        x = (torch.randn((B, C, H, W), generator=g) * sigma).double()
        t = torch.randint(0, C, (B, H, W), generator=g)
        t[torch.rand((B, H, W), generator=g) < frac] = -1
        pred, gt = {"logits": {"mask": x}}, {"mask": t}
        s = R.mask_losses_ref(x, t, -100, -1, 0.5, 2.0)
        # nn.functional.cross_entropy raises on -1: CE is compared where no pixel is ignored, and by its count otherwise
        if frac == 0.0:
            assert abs(s[0] / s[1] - float(L.CE()(pred, gt))) <= 1e-12 * abs(s[0] / s[1])
        assert s[1] == float((t >= 0).sum()) and s[3] == s[5] == float((t != -1).sum())
        for which, cls in ((1, L.CCE), (2, L.Focal)):
            want = float(cls()(pred, gt))
            assert abs(s[2 * which] / s[2 * which + 1] - want) <= 1e-12 * abs(want), (which, sigma, frac)
        want = float(L.Focal(alpha=0.25, gamma=1.5)(pred, gt))
        s = R.mask_losses_ref(x, t, -100, -1, 0.25, 1.5)
        assert abs(s[4] / s[5] - want) <= 1e-12 * abs(want)


def test_mask_loss_gradient_matches_lib_loss_in_float64(monkeypatch):
    import fastposecnn_amd.lib  # noqa: F401
    import loss as L
    monkeypatch.setenv("FPC_FUSED_MASK_LOSSES", "0")
    g = torch.Generator().manual_seed(6)
    B, C, H, W = 2, 7, 11, 9
    x = (torch.randn((B, C, H, W), generator=g) * 3).double().requires_grad_(True)
    t = torch.randint(0, C, (B, H, W), generator=g)
    t[0, :3] = -1
    pred, gt = {"logits": {"mask": x}}, {"mask": t}
    (3.0 * L.CCE()(pred, gt) + 7.0 * L.Focal(alpha=0.25, gamma=1.5)(pred, gt)).backward()
    n = float((t != -1).sum())
    got = R.mask_losses_grad_ref(x.detach(), t, -100, -1, 0.25, 1.5, (0.0, 3.0 / n, 7.0 / n))
    assert (got - x.grad).abs().max().item() <= 1e-12 * x.grad.abs().max().item()


@pytest.mark.parametrize("case", R.MASK_LOSS_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_float32_form_of_the_mask_losses_is_well_inside_the_kernel_bars(case):
    """The bars of test_gpu_train_kernels.py (2e-6 of a sum, floor one unit per counted pixel; 2e-5 of the largest gradient)
    against the rounding of a float32 evaluation of the same formulas: at least 4x inside at every case."""
    C, HW, B, sigma, alpha, gamma, kind = case
    x, t = R.mask_loss_inputs(case)
    want = R.mask_losses_ref(x, t, -100, -1, alpha, gamma)
    got = R.mask_losses_ref(x, t, -100, -1, alpha, gamma, dtype=torch.float32)
    worst = 0.0
    for k in (0, 2, 4):
        assert got[k + 1] == want[k + 1]
        tol = R.MASK_SUM_RTOL * max(abs(want[k]), want[k + 1])
        if tol == 0.0:
            assert got[k] == 0.0
        else:
            worst = max(worst, abs(got[k] - want[k]) / tol)
    print("f32 sums / bar", worst)
    assert worst <= 0.25
    if gamma >= 1.0:
        w3 = R.MASK_LOSS_W3[0]
        gw = R.mask_losses_grad_ref(x, t, -100, -1, alpha, gamma, w3)
        gg = R.mask_losses_grad_ref(x, t, -100, -1, alpha, gamma, w3, dtype=torch.float32).double()
        scale = gw.abs().max().item()
        ratio = (gg - gw).abs().max().item() / (R.MASK_GRAD_RTOL * scale) if scale > 0 else float((gg != 0).any())
        print("f32 grad / bar", ratio)
        assert ratio <= 0.25


def test_class_compress_ref_matches_the_library_cpu_form():
    """The library's own CPU form divides by a float32 norm, so it is held at float32 level on the forward; the gradient
    of the reference is autograd over the pure float64 statement."""
    import fastposecnn_amd.lib  # noqa: F401
    import gpu_tensor_funcs as gtf
    for case in R.CC_CASES:
        C, HW, B = case
        cat, logits, go = R.cc_inputs(case)
        ok = torch.where((cat >= 1) & (cat < C), cat, torch.zeros_like(cat))
        lib = gtf._class_compress_cpu(C, ok.reshape(B, HW, 1), {k: v.double().reshape(B, -1, HW, 1) for k, v in logits.items()})
        ref = R.class_compress_ref(C, cat, {k: v.double() for k, v in logits.items()})
        for k in ref:
            assert (lib[k].reshape(ref[k].shape) - ref[k]).abs().max().item() <= 2e-7 * max(1.0, ref[k].abs().max().item()), (case, k)
        q = ref["quaternion"].norm(dim=1)
        zero_q = (logits["quaternion"].reshape(B, C - 1, 4, HW).abs().sum(dim=2).gather(1, (ok - 1).clamp(min=0).unsqueeze(1)).squeeze(1) == 0)
        fg = ok != 0
        assert torch.allclose(q[fg & ~zero_q], torch.ones_like(q[fg & ~zero_q]), atol=1e-12) and (q[~fg] == 0).all()
        # the float32 form of the backward against the float64 one: what the 2e-6 bar of the GPU test is set against
        g64 = R.class_compress_backward_ref(C, cat, logits, go)
        g32 = R.class_compress_backward_ref(C, cat, logits, go, dtype=torch.float32)
        for k in g64:
            ratio = (g32[k].double() - g64[k]).abs().max().item() / (R.CC_RTOL * g64[k].abs().max().item())
            print(case, k, "f32 grad / bar", ratio)
            assert ratio <= 0.25, (case, k, ratio)
        if HW >= 64:                                     # pass-through at the exactly-zero selected vectors
            sel = g64["quaternion"].reshape(B, C - 1, 4, HW)
            for p in (50, 51, 52):
                assert torch.equal(sel[:, cat[0, p] - 1, :, p], go["quaternion"][:, :, p].double())


def test_refine_gradient_formula_matches_autograd():
    rng = np.random.default_rng(3)
    for trial in range(6):
        k = int(rng.integers(5, 400))
        centre = rng.uniform(0, 60, 2)
        coords = np.stack([rng.integers(0, 64, k), rng.integers(0, 48, k)], axis=1).astype(np.float64)
        ang = np.arctan2(centre[1] - coords[:, 1], centre[0] - coords[:, 0]) + rng.normal(0, 0.03, k)
        d = (np.stack([np.cos(ang), np.sin(ang)], axis=1) * rng.uniform(0.5, 2.0, (k, 1))).astype(np.float32)
        g = rng.normal(0, 1, 2)
        x, want = R.refine_grad_autograd(d, coords, g)
        a00, a01, a11, b0, b1 = R.normal_matrix(d, coords)
        assert a00 * a11 - a01 * a01 > 1e-3 * (a00 + a11) ** 2          # well conditioned
        xs = R.solve2_sym(a00, a01, a11, b0, b1)
        np.testing.assert_allclose(xs, x, rtol=1e-10)
        lam = R.solve2_sym(a00, a01, a11, g[0], g[1])
        got = R.refine_grad(coords, d, xs, lam)
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def test_solve2_sym_singular_rule_matches_the_library():
    import fastposecnn_amd.lib  # noqa: F401
    import train_functions as tf
    rows = [(4.0, 0.0, 0.0), (0.0, 0.0, 7.0), (2.0, 2.0, 2.0), (3.0, 1.0, 2.0), (0.0, 0.0, 0.0)]
    g = torch.tensor([[0.3, -0.7]] * len(rows), dtype=torch.float64)
    a = torch.tensor(rows, dtype=torch.float64)
    l0, l1 = tf._solve2_sym(a[:, 0], a[:, 1], a[:, 2], g)
    for i, (a00, a01, a11) in enumerate(rows):
        want = R.solve2_sym(a00, a01, a11, 0.3, -0.7)
        assert abs(float(l0[i]) - want[0]) <= 1e-15 and abs(float(l1[i]) - want[1]) <= 1e-15


@pytest.mark.parametrize("seed,fg_shape,max_num", [(0, (40, 50), 300), (1234, (33, 47), 1550), (2 ** 32 + 12345, (48, 64), 17),
                                                    (2 ** 63 + 5, (21, 30), 629)])
def test_rand_keep_matches_the_oracle_thinning(oracle, seed, fg_shape, max_num):
    H, W = 48, 64
    mask = np.zeros((2, H, W), np.float32)
    mask[0, 2:2 + fg_shape[0], 3:3 + fg_shape[1]] = 1                    # instance 0: above max_num
    mask[1, 5:9, 7:11] = 1                                              # instance 1: 16 pixels
    labels, d, _ = R.vote_scene(H, W, seed=1)
    vertex = np.broadcast_to(d.reshape(2, H, W).transpose(1, 2, 0)[None, :, :, None, :], (2, H, W, 1, 2)).copy()
    _, dbg = oracle.ransac_voting_layer_v3(mask, vertex, 8, seed=seed, max_num=max_num, return_debug=True)
    for i in range(2):
        flat = mask[i].reshape(-1)
        fg = int(flat.sum())
        kept = R.kept_mask(seed, i, flat, max_num)
        assert int(kept.sum()) == int(dbg[0]["tn"][i]), (i, fg)
        if fg > max_num:
            assert 0 < kept.sum() < fg and abs(kept.sum() - max_num) <= 6 * math.sqrt(max_num)
            one = [bool(R.rand_keep(seed, i, p, fg, max_num)) for p in np.nonzero(flat)[0][:50]]   # scalar calls agree
            assert one == list(kept[np.nonzero(flat)[0][:50]])
        else:
            assert kept.sum() == fg


def test_thinned_fit_of_the_oracle_is_least_squares_over_inliers_and_kept(oracle):
    """kept_mask, inlier_mask and the refinement reference together, as the GPU tests use them: on an instance above
    max_num the oracle's own vote returns the float64 least squares over (inliers of its winner) AND (kept pixels)."""
    H, W, max_num, seed = 48, 64, 400, 2 ** 33 + 99
    mask = np.zeros((2, H, W), np.float32)
    mask[0, 2:38, 2:44] = 1
    mask[1, 2:12, 44:64] = 1
    d = np.stack([R.vote_scene(H, W, seed=k, pattern=(1,))[1] for k in range(2)]).reshape(2, 2, H, W) * mask[:, None]
    vertex = np.ascontiguousarray(d.transpose(0, 2, 3, 1)[:, :, :, None, :])
    out, dbg = oracle.ransac_voting_layer_v3(mask, vertex, 64, max_num=max_num, seed=seed, return_debug=True)
    for i in range(2):
        kept = R.kept_mask(seed, i, mask[i].reshape(-1), max_num)
        win = dbg[0]["hyp"][i, dbg[0]["win_idx"][i]]
        inl = R.inlier_mask(oracle, d[i].reshape(2, -1), W, win, 0.999, kept)
        assert int(inl.sum()) == int(dbg[0]["inlier_count"][i]) and inl.sum() >= 50
        idx = np.nonzero(inl)[0]
        coords = np.stack([idx % W, idx // W], axis=1).astype(np.float64)
        x, _ = R.refine_grad_autograd(d[i].reshape(2, -1)[:, idx].T, coords, np.ones(2))
        assert np.abs(out[i, 0] - x).max() <= 1e-5


def test_radam_rectification_switches_where_the_tests_expect():
    assert [s for s in range(1, 40) if R.radam_sma(0.999, s) >= 5][0] == 6
    first = [s for s in range(1, 40) if R.radam_sma(0.9, s) >= 5][0]
    assert 2 <= first <= 11 and R.radam_sma(0.9, first - 1) < 5
