"""The training-side kernels of csrc/train.hip, each called through the C ABI and held to the float64 references of
tests/_train_refs.py at the shapes and branches tests/test_gpu_train.py does not reach: both instantiations of
k_mask_losses and both of its grid-stride wraps, out-of-range and all-ignored targets, k_cc_backward's pass-through and
zero-fill contract, the thinning / inactive / label-above-N branches of the two refinement backwards on crafted tables,
thinned and rank-one instances through the autograd Functions, every tail length of k_sumsq and the optimiser away from
its one tested configuration.  Every output buffer is NaN before the call and must be finite after it.

What each bar is set against (float32 evaluation of the same formulas on the CPU against the float64 reference, measured
at every case below by tests/test_train_refs_host.py, which also asserts the margin):
  k_mask_losses  sums      2e-6 of max(|sum|, count) (the bar of test_fused_mask_losses_match_torch_forms on the means);
                           float32 form: at most 1.5e-7 (0.075 of the bar, C = 32, HW = 1, spread 60)
                 gradient  2e-5 of the largest gradient; float32 form: at most 2.9e-6 (0.145 of the bar; the one-pixel plane
                           C = 2, HW = 1), at most 1.3e-6 elsewhere (all targets -100, spread 20), typically 2e-7 .. 4e-7.
                           No case comes within 4x of a bar, none is loosened.
                           The kernel itself measured at most 2.6e-6 of the largest gradient (the one-pixel plane) and 1.6e-6
                           elsewhere.  Before its log-softmax took the maximum off first (y = x - (mx + log sum) rounds y to an
                           ulp of the logit) it measured 1.5e-5 at spread 20 with every target -100 and 5e-6 .. 8e-6 at spread
                           60: inside the bar, but ten times the float32 form; the spread-3 test could not see it.
                 gamma = 0.5 has no autograd reference (infinite derivative where 1 - pt rounds to 0): forward sums and a
                 finite gradient only.
  k_cc_backward            2e-6 of each tensor's largest gradient; float32 form: at most 2.2e-7 (0.11 of the bar)
  k_post_backward /        gradients are float32 casts of float64 values over the oracle's exact inlier set: 1e-6 relative,
  k_vote_refine_backward   1e-30 absolute, exactly 0.0 outside the set; through the autograd Functions 2e-4 (the bar of
                           test_vote_refine_fn_matches_autograd: the refined point is stored in float32)
  k_sumsq                  1e-12 relative against numpy's float64 sum (fp64 accumulation of exact float32 squares)
  k_lookahead_radam        rtol 2e-5, atol 2e-6 over 13 steps, as test_lookahead_radam_kernel
"""
import numpy as np
import pytest
import torch

import _train_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -1
NAN = float("nan")


def _nat():
    from fastposecnn_amd import _native as nat
    return nat, nat.lib()


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), NAN, dtype=dtype, device="cuda")


def _ids(c):
    return "-".join(str(v) for v in c)


# ---- 2. fpc_mask_losses ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", R.MASK_LOSS_CASES, ids=_ids)
def test_mask_losses_sums_and_gradient_vs_float64(case):
    nat, L = _nat()
    C, HW, B, _sigma, alpha, gamma, _kind = case
    x, t = R.mask_loss_inputs(case)
    want = R.mask_losses_ref(x, t, -100, -1, alpha, gamma)
    xd, td = x.cuda(), t.cuda()
    sums = torch.zeros(6, dtype=torch.float64, device="cuda")

    def forward():
        nat.check(L.fpc_mask_losses(nat.ptr(xd), nat.ptr(td), B, C, HW, -100, -1, alpha, gamma, nat.ptr(sums), None, None,
                                    nat.stream()), "fpc_mask_losses")
        return sums.cpu().numpy().copy()

    got = forward()
    print("sums", got, "want", want)
    for k in (0, 2, 4):
        assert got[k + 1] == want[k + 1], (k, got, want)                       # counts: exact
        assert abs(got[k] - want[k]) <= R.MASK_SUM_RTOL * max(abs(want[k]), want[k + 1]), (k, got, want)
    twice = forward()                                                          # the kernel adds onto what is there
    for k in (0, 2, 4):
        assert twice[k + 1] == 2 * got[k + 1]
        assert abs(twice[k] - 2 * got[k]) <= 1e-12 * abs(2 * got[k])

    off = (t == -1)                                                            # CE, CCE and Focal all off
    for w3 in R.MASK_LOSS_W3:
        w = torch.tensor(w3, dtype=torch.float32)
        wd = w.cuda()
        grad = _nan((B, C, HW))
        nat.check(L.fpc_mask_losses(nat.ptr(xd), nat.ptr(td), B, C, HW, -100, -1, alpha, gamma, None, nat.ptr(wd), nat.ptr(grad),
                                    nat.stream()), "fpc_mask_losses backward")
        g = grad.cpu().double()
        assert torch.isfinite(g).all()
        assert (g.permute(0, 2, 1)[off] == 0).all()
        if gamma < 1.0:
            continue
        ref = R.mask_losses_grad_ref(x, t, -100, -1, alpha, gamma, w.double().tolist())
        scale = ref.abs().max().item()
        err = (g - ref).abs().max().item()
        print("w3", w3, "grad err", err, "scale", scale)
        if scale == 0.0:
            assert (g == 0).all()
        else:
            assert err <= R.MASK_GRAD_RTOL * scale, (w3, err, scale)
    assert torch.equal(sums.cpu(), torch.from_numpy(twice))                     # the backward leaves sums6 alone


def test_mask_losses_argument_contract():
    nat, L = _nat()
    x = torch.randn((2, 7, 33), device="cuda")
    t = torch.zeros((2, 33), dtype=torch.int64, device="cuda")
    w = torch.ones(3, device="cuda")
    sums = torch.zeros(6, dtype=torch.float64, device="cuda")
    grad = _nan((2, 7, 33))

    def call(B=2, C=7, HW=33, s=sums, w3=None, g=None):
        return L.fpc_mask_losses(nat.ptr(x), nat.ptr(t), B, C, HW, -100, -1, 0.5, 2.0, nat.ptr(s), nat.ptr(w3), nat.ptr(g), nat.stream())

    assert call(C=1) == EINVAL and call(C=33) == EINVAL and call(HW=0) == EINVAL
    assert call(s=None) == EINVAL                                              # both outputs null
    assert call(s=None, g=grad) == EINVAL                                      # grad without w3
    assert call(B=0) == 0 and call(B=0, s=None, w3=w, g=grad) == 0
    torch.cuda.synchronize()
    assert (sums == 0).all() and torch.isnan(grad).all()                       # nothing touched
    assert call() == 0 and sums[1].item() == 66


# ---- 3. fpc_class_compress_backward ---------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", R.CC_CASES, ids=_ids)
def test_class_compress_backward_vs_float64(case):
    nat, L = _nat()
    C, HW, B = case
    G = C - 1
    cat, logits, go = R.cc_inputs(case)
    want = R.class_compress_backward_ref(C, cat, logits, go)
    cat_d = cat.cuda()
    q_d, xy_d = logits["quaternion"].cuda(), logits["xy"].cuda()
    go_d = {k: v.contiguous().cuda() for k, v in go.items()}

    def run(skip=None):
        out = {k: _nan((B, a * G, HW)) for k, a, _ in R.CC_HEADS}
        gp = {k: (None if k == skip else nat.ptr(go_d[k])) for k in go_d}
        nat.check(L.fpc_class_compress_backward(nat.ptr(cat_d), nat.ptr(q_d), nat.ptr(xy_d), gp["quaternion"], gp["scales"], gp["xy"],
                                                gp["z"], B, C, HW, nat.ptr(out["quaternion"]), nat.ptr(out["scales"]),
                                                nat.ptr(out["xy"]), nat.ptr(out["z"]), nat.stream()), "fpc_class_compress_backward")
        return {k: v.cpu() for k, v in out.items()}

    full = run()
    valid = (cat >= 1) & (cat < C)
    on = valid.unsqueeze(1) & ((cat - 1).unsqueeze(1) == torch.arange(G).view(1, G, 1))          # [B,G,HW]
    for k, a, _ in R.CC_HEADS:
        got = full[k].double()
        assert torch.isfinite(got).all(), k
        scale = want[k].abs().max().item()
        err = (got - want[k]).abs().max().item()
        print(case, k, "err", err, "scale", scale)
        assert err <= R.CC_RTOL * scale if scale > 0 else (got == 0).all(), (k, err, scale)
        outside = ~on.unsqueeze(2).expand(B, G, a, HW)
        assert (full[k].reshape(B, G, a, HW)[outside] == 0).all(), k          # exactly zero outside the pixel's class group
    for skip in go_d:
        part = run(skip)
        for k in part:
            if k == skip:
                assert (part[k] == 0).all(), (skip, k)
            else:
                assert torch.equal(part[k], full[k]), (skip, k)


def test_class_compress_backward_argument_contract():
    nat, L = _nat()
    cat = torch.ones((1, 8), dtype=torch.int64, device="cuda")
    bufs = [_nan((1, 24 * a, 8)) for a in (4, 3, 2, 1)]
    src = torch.ones((1, 24 * 4, 8), device="cuda")

    def call(B=1, C=7, HW=8):
        return L.fpc_class_compress_backward(nat.ptr(cat), nat.ptr(src), nat.ptr(src), None, None, None, None, B, C, HW,
                                             *[nat.ptr(b) for b in bufs], nat.stream())

    assert call(C=1) == EINVAL and call(C=33) == EINVAL and call(HW=0) == EINVAL
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(b).all() for b in bufs)
    assert call() == 0
    torch.cuda.synchronize()
    assert all((b[:, :6 * a] == 0).all() for b, a in zip(bufs, (4, 3, 2, 1)))


# ---- 4. fpc_post_network_backward / fpc_vote_refine_backward on crafted tables -------------------------------------------
N_INST = 3
THRESH = 0.999
PLANES = [(1, 1, 1), (5, 51, 1), (257, 1, 1), (48, 64, 1), (48, 64, 2)]             # H, W, B
PATTERNS_B2 = ((1, 1, 1, 1, 1, 2, 0, 4), (0, 3, 3, 10, 0, 0, 3))                    # each instance inside one image


class _Scene:
    """Labels [B,HW], directions f32 [B,2,HW] and the 16-double table of k_post_backward, all built on the host."""

    def __init__(self, H, W, B):
        self.H, self.W, self.B, self.HW = H, W, B, H * W
        parts = [R.vote_scene(H, W, seed=b, **({"pattern": PATTERNS_B2[b]} if B == 2 else {})) for b in range(B)]
        self.labels = np.stack([p[0] for p in parts])
        self.d = np.stack([p[1] for p in parts])
        rng = np.random.default_rng(H * 1000 + W + B)
        tab = np.zeros((N_INST, 16))
        tab[:, 0:8] = rng.normal(0, 1, (N_INST, 8))
        tab[:, 8:10] = rng.normal(0, 0.01, (N_INST, 2))
        self.image = np.zeros(N_INST, int)
        for i in range(N_INST):
            where = [b for b in range(B) if (self.labels[b] == i + 1).any()]
            self.image[i] = where[0] if where else 0
            c = parts[self.image[i]][2][i + 1]
            tab[i, 10:12] = c + rng.normal(0, 0.3, 2)
            tab[i, 12:14] = (c + rng.normal(0, 0.5, 2)).astype(np.float32)
            tab[i, 14] = float((self.labels == i + 1).sum())
            tab[i, 15] = 1.0
        if self.HW == 1:                                                       # the lone pixel looks straight at its winner
            tab[0, 12:14] = 5.0 * self.d[0, :, 0]
        self.tab = tab
        self.fg1 = int(tab[0, 14])

    def expected(self, oracle, tab, n_eff, max_num, seed, keep):
        """Per-pixel outputs of k_post_backward in float64 ([B,4,HW], [B,3,HW], [B,2,HW], [B,HW]) and the fitted set."""
        B, HW = self.B, self.HW
        gq, gs, gxy, gz = np.zeros((B, 4, HW)), np.zeros((B, 3, HW)), np.zeros((B, 2, HW)), np.zeros((B, HW))
        fitted = np.zeros((B, HW), bool)
        for b in range(B):
            for i in range(min(n_eff, N_INST)):
                m = self.labels[b] == i + 1
                if not m.any():
                    continue
                t = tab[i]
                gq[b][:, m] = t[0:4].astype(np.float32)[:, None]
                gs[b][:, m] = t[4:7].astype(np.float32)[:, None]
                gz[b][m] = np.float32(t[7])
                if t[15] == 0.0:
                    continue
                fg, sel = int(t[14]), m.copy()
                if fg > max_num:
                    sel &= (keep[i] != 0) if keep is not None else R.rand_keep(seed, i, np.arange(HW), fg, max_num)
                inl = R.inlier_mask(oracle, self.d[b], self.W, t[12:14], THRESH, sel)
                idx = np.nonzero(inl)[0]
                coords = np.stack([idx % self.W, idx // self.W], axis=1)
                gxy[b][:, idx] = R.refine_grad(coords, self.d[b][:, idx].T, t[10:12], t[8:10]).T
                fitted[b] |= inl
        return gq, gs, gxy, gz, fitted

    def modes(self):
        """(name, table, n_dev, max_num, seed, keep): every branch of the two kernels."""
        rng = np.random.default_rng(self.HW)
        keep = (rng.random((N_INST, self.HW)) < 0.4).astype(np.uint8)
        inactive = self.tab.copy(); inactive[1, 15] = 0.0
        fg1 = self.fg1
        return [("plain", self.tab, None, 30000, 7, None),
                ("n_dev below N", self.tab, 2, 30000, 7, None),
                ("n_dev above N", self.tab, 9, 30000, 7, None),
                ("inactive vote row", inactive, None, 30000, 7, None),
                ("fg == max_num, keep bytes ignored", self.tab, None, fg1, 7, keep),
                ("fg == max_num + 1, keep bytes", self.tab, None, fg1 - 1, 7, keep),
                ("fg == max_num, seed", self.tab, None, fg1, 2 ** 40 + 77, None),
                ("fg == max_num + 1, seed", self.tab, None, fg1 - 1, 2 ** 40 + 77, None),
                ("thinned to a third, seed", self.tab, None, max(1, fg1 // 3), 2 ** 40 + 77, None),
                ("thinned to a third, keep bytes", self.tab, None, max(1, fg1 // 3), 7, keep)]


def _assert_xy(got, want, fitted, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), what
    assert (got[~np.broadcast_to(fitted, got.shape)] == 0).all(), what          # exactly zero outside the fitted set
    bad = ~(np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-30)
    assert not bad.any(), (what, int(bad.sum()), np.abs(got - want)[bad].max())


@pytest.mark.parametrize("plane", PLANES, ids=_ids)
def test_post_network_backward_on_crafted_tables(oracle, plane):
    nat, L = _nat()
    H, W, B = plane
    sc = _Scene(H, W, B)
    HW = sc.HW
    labels_d = torch.from_numpy(sc.labels).cuda()
    d_d = torch.from_numpy(sc.d).cuda()
    assert (sc.labels > N_INST).any() or HW == 1                                # labels above N are there
    thinned_some = False
    for name, tab, n_dev, max_num, seed, keep in sc.modes():
        tab_d = torch.from_numpy(tab).cuda()
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device="cuda")
        kd = None if keep is None else torch.from_numpy(keep).cuda()
        outs = [_nan((B, a, HW)) for a in (4, 3, 2, 1)]
        nat.check(L.fpc_post_network_backward(nat.ptr(labels_d), nat.ptr(d_d), B, H, W, N_INST, nat.ptr(nd), nat.ptr(tab_d), THRESH,
                                              max_num, seed, nat.ptr(kd), *[nat.ptr(o) for o in outs], nat.stream()), name)
        n_eff = N_INST if n_dev is None else min(N_INST, n_dev)
        gq, gs, gxy, gz, fitted = sc.expected(oracle, tab, n_eff, max_num, seed, keep)
        got = [o.cpu().numpy() for o in outs]
        for g, w, what in ((got[0], gq, "q"), (got[1], gs, "scales"), (got[3][:, 0], gz, "z")):
            assert np.array_equal(g.astype(np.float64), w), (name, what)        # float32 casts of the table, zeros elsewhere
        _assert_xy(got[2], gxy, fitted[:, None, :], name)
        if name == "plain":
            plain_fit = fitted
        elif "a third" in name or "max_num + 1, keep" in name:
            thinned_some |= bool((plain_fit & ~fitted).any())
        elif "fg == max_num," in name:
            assert np.array_equal(fitted, plain_fit), name                      # not thinned at equality
        if name == "inactive vote row":
            two = sc.labels == 2                                                # xy exactly 0, the other heads still filled
            assert (got[2].transpose(0, 2, 1)[two] == 0).all() and (got[0].transpose(0, 2, 1)[two] != 0).all()
    assert thinned_some or HW < 50                                              # thinning really removed inliers


VERTEX_LAYOUTS = ("planar-permuted", "contiguous", "slice-of-3")


def _vertex_view(v_hw2, layout):
    """v_hw2: f32 [n,H,W,2] on the device -> a [n,H,W,2] view in the given stride layout with the same values."""
    n, H, W, _ = v_hw2.shape
    if layout == "planar-permuted":
        return v_hw2.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    if layout == "contiguous":
        return v_hw2.contiguous().reshape(n, H, W, 1, 2)[:, :, :, 0, :]
    big = torch.full((n, H, W, 3, 2), NAN, device=v_hw2.device)
    big[:, :, :, 1, :] = v_hw2
    return big[..., 1:2, :][:, :, :, 0, :]


@pytest.mark.parametrize("plane", PLANES, ids=_ids)
def test_vote_refine_backward_on_crafted_tables_and_vertex_layouts(oracle, plane):
    nat, L = _nat()
    H, W, B = plane
    sc = _Scene(H, W, B)
    HW = sc.HW
    mask = np.stack([(sc.labels[sc.image[i]] == i + 1) * (0.5 + i) for i in range(N_INST)]).astype(np.float32)
    mask_d = torch.from_numpy(mask).cuda()
    v = torch.from_numpy(np.stack([sc.d[sc.image[i]].reshape(2, H, W).transpose(1, 2, 0) for i in range(N_INST)])).cuda()
    views = [_vertex_view(v, lay) for lay in VERTEX_LAYOUTS]
    assert len({tuple(x.stride()) for x in views}) == 3 or HW == 1
    for name, tab, n_dev, max_num, seed, keep in sc.modes():
        if n_dev is not None:
            continue
        tab8 = np.ascontiguousarray(tab[:, [8, 9, 10, 11, 12, 13, 14, 15]])
        tab_d = torch.from_numpy(tab8).cuda()
        kd = None if keep is None else torch.from_numpy(keep).cuda()
        gq, gs, gxy, gz, fitted = sc.expected(oracle, tab, N_INST, max_num, seed, keep)
        want = np.stack([gxy[sc.image[i]] * (sc.labels[sc.image[i]] == i + 1) for i in range(N_INST)])
        fit = np.stack([fitted[sc.image[i]] & (sc.labels[sc.image[i]] == i + 1) for i in range(N_INST)])
        results = []
        for view in views:
            out = _nan((N_INST, 2, HW))
            sn, sh, sw, scn = view.stride()
            nat.check(L.fpc_vote_refine_backward(nat.ptr(mask_d), view.data_ptr(), sn, sh, sw, scn, N_INST, H, W, nat.ptr(tab_d), THRESH,
                                                 max_num, seed, nat.ptr(kd), nat.ptr(out), nat.stream()), name)
            results.append(out.cpu())
        _assert_xy(results[0].numpy(), want, fit[:, None, :], name)
        assert torch.equal(results[0], results[1]) and torch.equal(results[0], results[2]), name


def test_refinement_backward_argument_contracts():
    nat, L = _nat()
    lab = torch.full((1, 6), 2, dtype=torch.int32, device="cuda")
    xy = torch.ones((1, 2, 6), device="cuda")
    tab = torch.zeros((1, 16), dtype=torch.float64, device="cuda")
    outs = [_nan((1, a, 6)) for a in (4, 3, 2, 1)]

    def post(B=1, H=2, W=3, N=1, table=tab, o=None):
        o = outs if o is None else o
        return L.fpc_post_network_backward(nat.ptr(lab), nat.ptr(xy), B, H, W, N, None, nat.ptr(table), THRESH, 30000, 1, None,
                                           *[nat.ptr(t) for t in o], nat.stream())

    assert post(H=32769, W=32768) == EINVAL and post(B=65536, H=1, W=1) == EINVAL
    for k in range(4):
        assert post(o=[None if j == k else outs[j] for j in range(4)]) == EINVAL
    assert post(N=1, table=None) == EINVAL
    assert post(B=0) == 0
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    assert post(N=0, table=None) == 0                                          # no instances: a null table is accepted
    torch.cuda.synchronize()
    assert all((o == 0).all() for o in outs)                                   # every label is above N: zeros everywhere

    mask = torch.ones((1, 6), device="cuda")
    vert = torch.ones((1, 2, 3, 2), device="cuda")
    tab8 = torch.zeros((1, 8), dtype=torch.float64, device="cuda")
    out = _nan((1, 2, 6))

    def refine(n=1, H=2, W=3, table=tab8, o=out):
        return L.fpc_vote_refine_backward(nat.ptr(mask), nat.ptr(vert), 12, 6, 2, 1, n, H, W, nat.ptr(table), THRESH, 30000, 1, None,
                                          nat.ptr(o), nat.stream())

    assert refine(H=32769, W=32768) == EINVAL and refine(n=65536, H=1, W=1) == EINVAL
    assert refine(o=None) == EINVAL and refine(table=None) == EINVAL
    assert refine(n=0, table=None, o=None) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert refine() == 0
    torch.cuda.synchronize()
    assert (out == 0).all()                                                    # inactive row: zeros, all written


# ---- 5. thinned and degenerate instances through the autograd Functions ---------------------------------------------------


def _directions(H, W, centre, noise, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    ang = np.arctan2(centre[1] - yy, centre[0] - xx) + rng.normal(0, noise, (H, W))
    out = rng.random((H, W)) < 0.05
    ang = np.where(out, rng.uniform(0, 2 * np.pi, (H, W)), ang)
    return np.stack([np.cos(ang), np.sin(ang)]).astype(np.float32)            # [2,H,W]


def test_vote_refine_fn_thinned_instance_fits_and_differentiates_the_same_pixels(oracle):
    import fastposecnn_amd.lib  # noqa: F401
    import train_functions as tf
    import ransac_voting_gpu_layer.ransac_voting_gpu as rvg
    H, W, max_num, seed, hn = 48, 64, 400, 2 ** 33 + 99, 64
    mask = np.zeros((3, H, W), np.float32)
    mask[0, 2:38, 2:44] = 1                                                   # 1512 pixels: thinned
    mask[1, 2:12, 44:64] = 1                                                  # 200 pixels: not thinned
    mask[2, 45, 50:53] = 1                                                    # 3 pixels: below min_num
    d = np.stack([_directions(H, W, c, 0.03, k) for k, c in enumerate(((20.3, 17.6), (55.2, 6.4), (51.0, 44.0)))])
    d = d * mask[:, None]
    mask_d = torch.from_numpy(mask).cuda()
    v = torch.from_numpy(d).cuda().requires_grad_(True)                       # [n,2,H,W]
    vertex = v.permute(0, 2, 3, 1).unsqueeze(3)
    out = tf.VoteRefineFn.apply(mask_d, vertex, hn, THRESH, 5, max_num, seed)
    w = np.array([0.3, -0.7])
    (out[:, 0, :] * torch.tensor(w, dtype=torch.float32, device="cuda")).sum().backward()
    got = v.grad.cpu().double().numpy().reshape(3, 2, H * W)
    assert np.isfinite(got).all()
    refine = torch.zeros((3, 1, 8), dtype=torch.float64, device="cuda")
    again = rvg.ransac_voting_layer_v3(mask_d, vertex.detach(), hn, THRESH, min_num=5, max_num=max_num, seed=seed, refine_out=refine)
    assert torch.equal(again, out.detach())
    rec = refine.cpu().numpy()[:, 0]
    xy = out.detach().cpu().double().numpy()[:, 0]
    for i in range(2):
        flat = mask[i].reshape(-1)
        kept = R.kept_mask(seed, i, flat, max_num)
        assert (kept.sum() < flat.sum()) == (i == 0)
        inl = R.inlier_mask(oracle, d[i].reshape(2, -1), W, rec[i, 0:2], THRESH, kept)
        assert int(inl.sum()) == int(rec[i, 7]) and inl.sum() >= 50, (i, inl.sum(), rec[i, 7])   # the set the forward fitted
        idx = np.nonzero(inl)[0]
        coords = np.stack([idx % W, idx // W], axis=1).astype(np.float64)
        x, grad = R.refine_grad_autograd(d[i].reshape(2, -1)[:, idx].T, coords, w)
        assert (np.abs(xy[i] - x) <= 2e-4 * np.maximum(np.abs(x), 1.0)).all(), (i, xy[i], x)
        want = np.zeros((2, H * W)); want[:, idx] = grad.T
        scale = np.abs(want).max()
        err = np.abs(got[i] - want).max()
        print("instance", i, "inliers", idx.size, "grad err / scale", err / scale)
        assert scale > 0 and err <= 2e-4 * scale, (i, err, scale)
        assert (got[i][:, ~inl] == 0).all()                                   # nothing outside inliers AND kept
    assert (xy[2] == 0).all() and (got[2] == 0).all()                         # fewer than min_num pixels


def test_vote_refine_fn_rank_one_instance_follows_the_documented_rule(oracle):
    """Every direction parallel: the normal matrix has rank one, the forward takes solve2_sym's singular rule
    (x = A b / tr^2) and the backward the same rule for lam (lam = A g / tr^2).  The pseudo-inverse is discontinuous in the
    directions there, so this pins the documented rule, not a derivative: finite, bit-identical on a second run, and equal
    to the float64 evaluation of the rule through the per-pixel formula."""
    import fastposecnn_amd.lib  # noqa: F401
    import train_functions as tf
    H, W, seed = 48, 64, 5
    mask = np.zeros((1, H, W), np.float32)
    mask[0, 0:3, 1:64] = 1
    d = np.zeros((1, 2, H, W), np.float32)
    d[0, 0] = -1.0                                                             # all point along -x: towards (0, y)
    mask_d = torch.from_numpy(mask).cuda()
    g = np.array([0.3, -0.7])
    grads, outs = [], []
    for _ in range(2):
        v = torch.from_numpy(d).cuda().requires_grad_(True)
        out = tf.VoteRefineFn.apply(mask_d, v.permute(0, 2, 3, 1).unsqueeze(3), 64, THRESH, 5, 30000, seed)
        (out[:, 0, :] * torch.tensor(g, dtype=torch.float32, device="cuda")).sum().backward()
        grads.append(v.grad.cpu()); outs.append(out.detach().cpu())
    assert torch.isfinite(grads[0]).all() and torch.equal(grads[0], grads[1]) and torch.equal(outs[0], outs[1])
    # the parallel lines meet nowhere: every hypothesis is (0, 0) (the oracle's rule) and the pixels that see it within the
    # angle threshold are the set
    inl = R.inlier_mask(oracle, d[0].reshape(2, -1), W, (0.0, 0.0), THRESH, mask[0].reshape(-1) != 0)
    idx = np.nonzero(inl)[0]
    assert idx.size >= 50
    coords = np.stack([idx % W, idx // W], axis=1).astype(np.float64)
    dd = d[0].reshape(2, -1)[:, idx].T
    a00, a01, a11, b0, b1 = R.normal_matrix(dd, coords)
    assert a00 * a11 - a01 * a01 <= 1e-12 * (a00 + a11) ** 2                   # the singular branch
    x = R.solve2_sym(a00, a01, a11, b0, b1)
    xy = outs[0][0, 0].double().numpy()
    assert np.abs(xy - x).max() <= 2e-4 * max(1.0, np.abs(x).max()) and x[1] > 0
    lam = R.solve2_sym(a00, a01, a11, g[0], g[1])
    want = np.zeros((2, H * W)); want[:, idx] = R.refine_grad(coords, dd, xy, lam).T      # xy: the float32 point the backward reads
    got = grads[0][0].double().numpy().reshape(2, -1)
    assert np.abs(want).max() > 0
    assert (np.abs(got - want) <= 1e-6 * np.abs(want) + 1e-30).all()


def _logits_from_cat(cat, G=6, noise=0.05):
    """Logits whose class compression reproduces `cat` (plus noise on the other classes), as test_gpu_train builds them."""
    B, H, W = cat["mask"].shape
    g = torch.Generator().manual_seed(7)
    onehot = torch.nn.functional.one_hot(cat["mask"], G + 1).permute(0, 3, 1, 2).float()
    logits = {"mask": onehot * 8.0 + torch.randn((B, G + 1, H, W), generator=g) * 0.1}
    for key, a in (("quaternion", 4), ("scales", 3), ("xy", 2), ("z", 1)):
        v = cat[key] if key != "z" else cat[key].unsqueeze(1)
        full = torch.randn((B, G, a, H, W), generator=g) * noise
        sel = torch.nn.functional.one_hot((cat["mask"] - 1).clamp(min=0), G).permute(0, 3, 1, 2).unsqueeze(2).float()
        scale = 1.7 if key in ("quaternion", "xy") else 1.0
        full = full + sel * (v.unsqueeze(1) * scale)
        logits[key] = full.reshape(B, G * a, H, W)
    return logits


def test_post_network_backward_over_a_thinned_instance_matches_autograd(oracle):
    """One instance above PostNetworkFn's fixed max_num = 30000: the backward must differentiate the least squares over
    the pixels the forward fitted (inliers AND the rand_keep selection of instance l - 1), as float64 autograd does."""
    import fastposecnn_amd.lib as L
    from fastposecnn_amd import config
    import train_functions as tf
    import ransac_voting_gpu_layer.ransac_voting_gpu as rvg
    H, W, seed, max_num = 192, 256, 1234, 30000
    hp = config.HEAD_TRAINING()
    hp.HV_NUM_OF_HYPOTHESES = 64
    torch.manual_seed(0)
    model = L.pose_regressor.MODELS[hp.MODEL].load_from_ckpt(None, hp).cuda()
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), np.int64)
    m[8:184, 8:192] = 1                                                       # 176 x 184 = 32 384 pixels
    m[(xx - 225) ** 2 + (yy - 100) ** 2 <= 12 ** 2] = 2
    rng = np.random.default_rng(0)
    cat = {"mask": torch.from_numpy(m)[None], "quaternion": torch.zeros((1, 4, H, W)), "scales": torch.zeros((1, 3, H, W)),
           "xy": torch.zeros((1, 2, H, W)), "z": torch.zeros((1, H, W))}
    for cls, centre in ((1, (97.3, 101.8)), (2, (224.6, 100.3))):
        sel = torch.from_numpy(m == cls)
        n = int(sel.sum())
        cat["xy"][0][:, sel] = torch.from_numpy(_directions(H, W, centre, 0.03, cls))[:, sel]
        q = rng.normal(0, 1, 4); q /= np.linalg.norm(q)
        qq = torch.from_numpy(q[:, None] + rng.normal(0, 0.01, (4, n))).float()
        cat["quaternion"][0][:, sel] = qq / qq.norm(dim=0, keepdim=True)
        cat["scales"][0][:, sel] = torch.from_numpy(rng.uniform(0.1, 0.5, 3)[:, None] + rng.normal(0, 0.01, (3, n))).float()
        cat["z"][0][sel] = torch.from_numpy(rng.uniform(6.2, 7.2) + rng.normal(0, 0.01, n)).float()
    logits_cpu = _logits_from_cat(cat)
    logits = {k: v.cuda().requires_grad_(k != "mask") for k, v in logits_cpu.items()}
    ccat = tf.class_compression_train(7, logits)
    assert torch.equal(ccat["mask"].cpu(), cat["mask"])
    agg = tf.post_network_train(model, ccat, seed=seed)
    N = agg["class_ids"].shape[0]
    assert N == 2
    g = torch.Generator().manual_seed(3)
    keys = ("quaternion", "scales", "xy", "z")
    wts = {k: torch.randn(agg[k].shape, generator=g) for k in keys}
    wts["xy"] *= 0.05
    pix = {k: torch.randn(ccat[k].shape, generator=g) * 1e-4 for k in keys}
    loss = sum((agg[k] * wts[k].cuda()).sum() for k in keys) + sum((ccat[k] * pix[k].cuda()).sum() for k in keys)
    loss.backward()

    labels, n_lab = model.aggregation_layer.batchwise_break_segmentation_mask(ccat["mask"])
    assert n_lab == N
    refine = torch.zeros((N, 1, 8), dtype=torch.float64, device="cuda")
    vertex = torch.unsqueeze(agg["xy_mask"].permute(0, 2, 3, 1), dim=3)
    voted = rvg.ransac_voting_layer_v3(agg["instance_masks"], vertex, 64, seed=seed, refine_out=refine)
    torch.testing.assert_close(voted[:, 0, :], agg["xy"].detach())
    rec = refine.cpu().numpy()[:, 0]
    labels = labels.cpu().numpy().reshape(-1)
    native_xy = ccat["xy"].detach().cpu().numpy()[0].reshape(2, -1)           # the f32 values the kernels voted on

    ref_logits = {k: v.detach().cpu().double().reshape(1, v.shape[1], -1).requires_grad_(k != "mask") for k, v in logits.items()}
    rcat = R.class_compress_ref(7, cat["mask"].reshape(1, -1), {k: ref_logits[k] for k in keys})
    ragg = {k: [] for k in keys}
    thinned = 0
    for i in range(N):
        mb = labels == i + 1
        cnt = int(mb.sum())
        sel = torch.from_numpy(mb)
        qm = rcat["quaternion"][0][:, sel].sum(dim=1) / cnt
        ragg["quaternion"].append(qm / qm.norm())
        ragg["scales"].append(rcat["scales"][0][:, sel].sum(dim=1) / cnt)
        ragg["z"].append(torch.exp(rcat["z"][0][0][sel].sum() / cnt).reshape(1))
        kept = R.kept_mask(seed, i, mb, max_num)
        thinned += int(kept.sum() < cnt)
        inl = R.inlier_mask(oracle, native_xy, W, rec[i, 0:2], THRESH, kept)
        assert int(inl.sum()) == int(rec[i, 7]), (i, inl.sum(), rec[i, 7])     # the set the forward fitted
        idx = np.nonzero(inl)[0]
        coords = torch.from_numpy(np.stack([idx % W, idx // W], axis=1).astype(np.float64))
        ragg["xy"].append(R.refine_solve_torch(rcat["xy"][0][:, torch.from_numpy(idx)].T, coords))
    assert thinned == 1
    ragg = {k: torch.stack(v) for k, v in ragg.items()}
    for k in keys:
        torch.testing.assert_close(agg[k].detach().cpu().double().reshape(ragg[k].shape), ragg[k].detach(), rtol=2e-4, atol=2e-4)
    rloss = sum((ragg[k] * wts[k].double().reshape(ragg[k].shape)).sum() for k in keys) + \
        sum((rcat[k].reshape(pix[k].shape) * pix[k].double()).sum() for k in keys)
    rloss.backward()
    for k in keys:
        got, want = logits[k].grad.cpu().double().reshape(ref_logits[k].shape), ref_logits[k].grad
        assert torch.isfinite(got).all()
        scale = want.abs().max().item()
        err = (got - want).abs().max().item()
        print(k, "grad err / scale", err / scale)
        assert scale > 0 and err <= 2e-4 * scale + 1e-9, (k, err, scale)


# ---- 6. fpc_grad_sumsq / fpc_lookahead_radam_step -------------------------------------------------------------------------


def _aligned(n):
    buf = torch.zeros(n + 8, device="cuda")
    off = (-buf.data_ptr() // 4) % 4
    return buf[off:off + n]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 2 ** 21 + 2, 2 ** 22 + 1])
def test_grad_sumsq_every_tail_and_the_wrapped_grid(n):
    nat, L = _nat()
    host = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    g = _aligned(n)
    g.copy_(host)
    assert g.data_ptr() % 16 == 0
    out = torch.zeros(2, dtype=torch.float64, device="cuda")

    def run():
        out.zero_()
        nat.check(L.fpc_grad_sumsq(nat.ptr(g), n, nat.ptr(out), nat.stream()), "sumsq")
        return out.cpu().numpy().copy()

    got = run()
    want = float((host.numpy().astype(np.float64) ** 2).sum())
    assert abs(got[0] - want) <= 1e-12 * want and got[1] == 0, (got, want)
    n4 = n // 4
    spots = [n4 * 4 + j for j in range(n & 3)]                                 # each tail slot
    if n4:
        spots += [4 * (n4 - 1) + k for k in range(4)]                          # the last float4
    if n4 > 2048 * 256:
        spots.append(4 * (2048 * 256 + 5) + 2)                                 # an element of the loop's second trip
    for k, i in enumerate(spots):
        keep = float(g[i])
        g[i] = float("inf") if k % 2 == 0 else NAN
        assert run()[1] > 0, (n, i)
        g[i] = keep
    assert run()[1] == 0


def test_grad_sumsq_argument_contract():
    nat, L = _nat()
    g = _aligned(64)
    out = torch.tensor([3.5, 7.0], dtype=torch.float64, device="cuda")
    assert L.fpc_grad_sumsq(g[1:].data_ptr(), 8, nat.ptr(out), nat.stream()) == EINVAL      # 4 bytes off 16-byte alignment
    assert L.fpc_grad_sumsq(nat.ptr(g), 8, None, nat.stream()) == EINVAL
    assert L.fpc_grad_sumsq(nat.ptr(g), 0, nat.ptr(out), nat.stream()) == 0
    assert L.fpc_grad_sumsq(None, 0, nat.ptr(out), nat.stream()) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [3.5, 7.0]


@pytest.mark.parametrize("case", [(1, 0.999, 1, 0.5, 0.0), (257, 0.9, 5, 1.0, 3e-4), (2 ** 20 + 77, 0.999, 5, 0.5, 3e-4),
                                  (2 ** 20 + 77, 0.9, 1, 1.0, 0.0), (257, 0.999, 1, 1.0, 3e-4), (1, 0.9, 5, 0.5, 0.0)], ids=_ids)
def test_lookahead_radam_across_sizes_and_hyperparameters(case):
    nat, L = _nat()
    n, beta2, la_k, la_alpha, wd = case
    cross = next(s for s in range(1, 100) if R.radam_sma(beta2, s) >= 5)       # the first rectified step
    steps = 13
    assert 1 < cross < steps - 1                                               # both branches run, with steps to spare
    g = torch.Generator().manual_seed(n % 1000 + la_k)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(steps)]
    want = R.radam_lookahead_reference(p0, grads, 1e-3, (0.9, beta2), 1e-8, wd, la_k, la_alpha)
    p = p0.cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    slow = _nan((n,))                                                          # initialised by step 1, never read before
    for step, gr in enumerate(grads, start=1):
        gd = gr.cuda()
        nat.check(L.fpc_lookahead_radam_step(nat.ptr(p), nat.ptr(gd), nat.ptr(m), nat.ptr(v), nat.ptr(slow), n, 1e-3, 0.9, beta2,
                                             1e-8, wd, step, la_k, la_alpha, None, nat.stream()), "radam")
    assert torch.isfinite(p).all() and torch.isfinite(slow).all()
    torch.testing.assert_close(p.cpu().double(), want, rtol=2e-5, atol=2e-6)


def test_lookahead_radam_refuses_bad_arguments():
    nat, L = _nat()
    p = torch.ones(8, device="cuda")
    bufs = [torch.zeros(8, device="cuda") for _ in range(4)]

    def call(step=1, la_k=5, b1=0.9, b2=0.999):
        return L.fpc_lookahead_radam_step(nat.ptr(p), *[nat.ptr(b) for b in bufs], 8, 1e-3, b1, b2, 1e-8, 0.0, step, la_k, 0.5, None,
                                          nat.stream())

    assert call(step=0) == EINVAL and call(la_k=0) == EINVAL and call(b1=1.0) == EINVAL and call(b2=1.0) == EINVAL
    torch.cuda.synchronize()
    assert (p == 1).all()
