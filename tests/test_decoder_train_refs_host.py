"""The references of tests/_decoder_train_refs.py held against independent ones on the CPU, the reachability claims of its case
tables checked on the float32 mirror of the kernels' index arithmetic, the form codes of the upsample cases asked of
fpc_upsample_bilinear_form (host arithmetic: no GPU), and the float32 evaluation of the same formulas measured against every
bar tests/test_gpu_decoder_train_kernels.py asserts."""
import numpy as np
import pytest
import torch

import _decoder_train_refs as R

EINVAL = -1
UP_CASES = [(c, False) for c in R.UP_FWD_CASES] + [(c, True) for c in R.UP_BWD_CASES]
UP_IDS = [("bwd-" if b else "fwd-") + c["name"] for c, b in UP_CASES]


def _refs(case, backward):
    v = R.up_values(case, backward)
    s = case["scale"]
    if backward:
        return v, R.up_adjoint_A(v, s), R.up_adjoint_B(v, s), R.up_adjoint_f32(v, s), R.up_adjoint_B(v, s, torch.float32)
    return v, R.up_forward_A(v, s), R.up_forward_B(v, s), R.up_forward_f32(v, s), R.up_forward_B(v, s, torch.float32)


# ---- upsample: the references against each other ---------------------------------------------------------------------------------


@pytest.mark.parametrize("case,backward", UP_CASES, ids=UP_IDS)
def test_upsample_references_agree_and_the_float32_form_is_inside_the_bars(case, backward):
    v, (A, S), B, f32, t32 = _refs(case, backward)
    h, w, s = case["h"], case["w"], case["scale"]
    assert A.shape == B.shape == f32.shape == t32.shape
    bar_b = R.UP_B_RTOL * max(1.0, np.abs(B).max())
    assert np.abs(A - B).max() <= bar_b                                             # A against B, within B's own bar
    k = R.k_up_bwd(h, w, s) if backward else R.K_UP_FWD
    assert (S > 0).all()
    # the float32 evaluation of the mirror against A (the derived bar) and against B: what the kernels are held to
    ratio_a = (np.abs(f32.astype(np.float64) - A) / (R.gamma_k(k) * S)).max()
    ratio_b = np.abs(f32.astype(np.float64) - B).max() / bar_b
    print("k", k, "f32 form / bar A", ratio_a, "/ bar B", ratio_b)
    assert ratio_a <= 1.0 and ratio_b <= 0.5
    # torch's own float32 kernel on the CPU uses the same weights; its roundings: 6 in the forward, and in the backward a
    # product of the two weights, the product with the gradient and a sum over up to taps_x * taps_y terms
    k_torch = R.taps(w, s) * R.taps(h, s) + 2 if backward else R.K_UP_FWD
    assert (np.abs(f32.astype(np.float64) - t32.astype(np.float64)) <= R.gamma_k(k + k_torch) * S).all()


def test_weight_matrices_are_the_kernels_weights():
    for n, s in ((1, 2), (1, 4), (2, 2), (5, 4), (70, 2), (160, 4)):
        W = R.axis_weights(n, s)
        assert W.dtype == np.float32 and W.shape == (n * s, n)
        assert ((W != 0).sum(axis=1) <= 2).all() and (W >= 0).all()
        assert np.abs(W.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23      # l0 + l1 = 1 to one rounding
        assert W[0, 0] == 1.0
    assert R.up_ratio(1, 4) == 0.0 and (R.axis_weights(1, 4) == 1.0).all()


# ---- upsample: reachability --------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", [c for c in R.UP_FWD_CASES if "patch" in c["claims"]], ids=R.up_case_id)
def test_lds_cases_reach_the_patch_they_claim(case):
    rows, cols = R.patch_extent(case["h"], case["scale"], 4), R.patch_extent(case["w"], case["scale"], 64)
    assert (rows, cols) == case["claims"]["patch"]
    assert case["form"] == R.FWD_LDS


def test_the_full_patch_is_reached_by_a_case_with_a_partial_last_block():
    full = [c for c in R.UP_FWD_CASES if c["claims"].get("patch") == (R.UP_PATCH_H, R.UP_PATCH_W)]
    assert any(c["scale"] == 2 and c["w"] >= 65 and c["h"] >= 5 and (c["w"] * 2) % 64 and c["w"] * 2 > 64 and (c["h"] * 2) % 4 for c in full)
    assert {c["C"] for c in R.UP_FWD_CASES if c["form"] == R.FWD_LDS} >= {1, 7, 32}
    assert any(c["C"] == 33 and c["src"] == ("nhwc",) and not c["dst_nhwc"] and c["form"] != R.FWD_LDS for c in R.UP_FWD_CASES)
    assert any(c["h"] == 1 for c in R.UP_FWD_CASES if c["form"] == R.FWD_LDS)
    assert any(c["w"] == 1 for c in R.UP_FWD_CASES if c["form"] == R.FWD_LDS)


def test_patch_never_exceeds_its_lds_extent_and_is_tight_at_scale_2():
    for scale in (2, 4):
        widest = [R.patch_extent(n, scale, 64) for n in range(1, 2049)]
        tallest = [R.patch_extent(n, scale, 4) for n in range(1, 2049)]
        assert max(widest) <= R.UP_PATCH_W and max(tallest) <= R.UP_PATCH_H
        if scale == 4:
            assert max(widest) == 18 and max(tallest) == 3
        else:
            assert all(v == R.UP_PATCH_W for v in widest[64:]) and all(v == R.UP_PATCH_H for v in tallest[4:])
            assert max(widest[:64]) < R.UP_PATCH_W and max(tallest[:4]) < R.UP_PATCH_H


def test_rolled_branch_is_a_scale_4_matter_and_its_range_is_bounded():
    for n in range(1, 2049):
        count2, span2 = R.rolled_count(n, 2)
        count4, span4 = R.rolled_count(n, 4)
        assert count2 == 0 and span2 < R.UP_TAPS
        assert span4 <= 13
        assert (1 <= count4 <= 4) if n >= 5 else count4 == 0, (n, count4)


@pytest.mark.parametrize("case", R.UP_BWD_CASES, ids=R.up_case_id)
def test_backward_cases_take_the_branch_they_claim(case):
    rx, ry = R.rolled_count(case["w"], case["scale"])[0] > 0, R.rolled_count(case["h"], case["scale"])[0] > 0
    assert (rx, ry) == case["claims"]["rolled"]
    if case["scale"] == 2:
        assert not rx and not ry


def test_every_backward_kernel_has_a_rolled_and_an_unrolled_case():
    seen = {}
    for c in R.UP_BWD_CASES:
        for p in (1, 2):
            seen.setdefault((p, c["form"][p - 1]), set()).add(c["claims"]["rolled"][p - 1])
    assert set(seen) == set(R.BWD_KERNELS)
    for key, kinds in seen.items():
        assert kinds == {True, False}, R.BWD_KERNELS[key]
    # the row tail of k_up_bwd_x_nchw: h * scale no multiple of 4
    assert any(c["form"][0] == R.BWD_NCHW and (c["h"] * c["scale"]) % 4 for c in R.UP_BWD_CASES)


def test_adjoint_range_holds_every_output_with_weight():
    for scale in (2, 4):
        for n in range(1, 301):
            W = R.axis_weights(n, scale)
            lo, hi = R.adjoint_range(n, scale)
            o = np.arange(n * scale)[:, None]
            assert not (W[(o < lo[None, :]) | (o > hi[None, :])] != 0).any(), (n, scale)


# ---- upsample: which kernel a case runs on ---------------------------------------------------------------------------------------


def _form(L, case, backward, extra=0):
    B, C, h, w, s = (case[k] for k in ("B", "C", "h", "w", "scale"))
    st, _, _ = R.src_geometry(case["src"], B, C, h * s if backward else h, w * s if backward else w)
    code = L.fpc_upsample_bilinear_form(int(backward), R.up_low4(case, backward, extra), *st, B, C, h, w, s, case["dst_nhwc"])
    return (code & 15, code >> 4) if backward and code >= 0 else code


def test_case_tables_reach_every_form_the_launchers_have():
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    fwd = set()
    for c in R.UP_FWD_CASES:
        assert _form(L, c, False) == c["form"], c["name"]
        fwd.add(c["form"])
        if c["form"] != R.FWD_SCALAR:
            assert _form(L, R.forced_scalar(c, False), False) == R.FWD_SCALAR, c["name"]
    assert fwd == R.FWD_FORMS
    pairs = set()
    for c in R.UP_BWD_CASES:
        assert _form(L, c, True) == c["form"], c["name"]
        pairs.add(c["form"])
        if c["form"] != (R.BWD_SCALAR, R.BWD_SCALAR):
            assert _form(L, R.forced_scalar(c, True), True) == (R.BWD_SCALAR, R.BWD_SCALAR), c["name"]
    assert pairs == R.BWD_PAIRS
    # the scalar forward is reached each way the launcher has
    why = {c["name"] for c in R.UP_FWD_CASES if c["form"] == R.FWD_SCALAR}
    assert {"scalar-unaligned-nchw", "scalar-strides", "scalar-w-odd", "scalar-c6-nhwc"} <= why
    # awkward sources
    kinds = {c["src"][0] for c in R.UP_FWD_CASES + R.UP_BWD_CASES}
    assert {"nhwc_slice", "nchw_slice"} <= kinds and any(c["src"][0] == "zero" for c in R.UP_BWD_CASES)


def test_form_function_covers_every_combination_and_refuses_what_the_launchers_refuse():
    from fastposecnn_amd import _native as nat
    L = nat.lib()
    fwd, pairs = set(), set()
    for low4 in (0, 4, 8, 12):
        for C in (1, 3, 4, 32, 33):
            for w in (3, 4):
                for nhwc_src in (0, 1):
                    for pad in (0, 1):
                        for dst_nhwc in (0, 1):
                            for scale in (2, 4):
                                h = 2
                                st = (h * (w + pad) * C, 1, (w + pad) * C, C) if nhwc_src else (C * h * (w + pad), h * (w + pad), w + pad, 1)
                                f = L.fpc_upsample_bilinear_form(0, low4, *st, 2, C, h, w, scale, dst_nhwc)
                                H, W = h * scale, w * scale
                                sb = (H * (W + pad) * C, 1, (W + pad) * C, C) if nhwc_src else (C * H * (W + pad), H * (W + pad), W + pad, 1)
                                b = L.fpc_upsample_bilinear_form(1, low4, *sb, 2, C, h, w, scale, dst_nhwc)
                                assert f >= 0 and b >= 0
                                fwd.add(f); pairs.add((b & 15, b >> 4))
    assert fwd == R.FWD_FORMS and pairs == R.BWD_PAIRS
    for backward in (0, 1):
        ok = lambda **kw: L.fpc_upsample_bilinear_form(backward, 0, *kw.pop("st", (60, 20, 5, 1)), *[
            {"B": 2, "C": 3, "h": 4, "w": 5, "scale": 2, "nhwc": 0, **kw}[k] for k in ("B", "C", "h", "w", "scale", "nhwc")])
        assert ok() >= 0
        for bad in ({"scale": 1}, {"scale": 3}, {"scale": 8}, {"B": 0}, {"C": 0}, {"h": 0}, {"w": 0}, {"B": 256, "C": 256},
                    {"B": 65536, "C": 1}):
            assert ok(**bad) == EINVAL, (backward, bad)
        assert ok(B=255, C=257) >= 0                                             # 65 535 planes
    # a channel-last destination puts the images in the grid's z and the rows in its y
    assert L.fpc_upsample_bilinear_form(0, 0, 8, 1, 8, 8, 65535, 8, 1, 1, 2, 1) == R.FWD_NHWC4
    assert L.fpc_upsample_bilinear_form(0, 0, 8, 1, 8, 8, 65536, 8, 1, 1, 2, 1) == EINVAL
    assert L.fpc_upsample_bilinear_form(0, 0, 8, 1, 8, 8, 1, 8, 16384, 1, 4, 1) == EINVAL       # 65 536 output rows


# ---- GroupNorm + ReLU ---------------------------------------------------------------------------------------------------------------


def test_groupnorm_cases_cover_what_the_kernels_branch_on():
    assert {c[4] for c in R.GN_CASES} == {1, 2, 4, 8, 16, 32, 64}
    assert {c[2] * c[3] for c in R.GN_CASES} >= {1, 3, 255, 256, 257, 513}
    assert any(c[2] * c[3] * c[4] > 65536 for c in R.GN_CASES) and any(c[0] == 2 for c in R.GN_CASES)
    assert {c[5] for c in R.GN_CASES} == {1e-5, 1e-3} and {c[6] for c in R.GN_CASES} == {"randn", "offset", "constant"}
    assert all(c[1] == 4 * c[4] for c in R.GN_CASES)
    off = [c for c in R.GN_CASES if c[6] == "offset"]
    assert all(c[2] * c[3] > R.GN_CHUNK and c[2] * c[3] % R.GN_CHUNK == 1 for c in off)
    for c in R.GN_CASES:
        _, _, gamma, beta = R.gn_inputs(c)
        assert gamma[1] == 0 and (gamma > 0).any() and (gamma < 0).any() and (np.abs(beta) >= 0.01).all()


@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_case_id)
def test_groupnorm_reference_is_torch_float64_and_the_float32_form_is_inside_the_bars(case):
    B, C, H, W, Q, eps, kind = case
    x, dy, gamma, beta = R.gn_inputs(case)
    y, z, mean, rstd, xhat = R.gn_forward_ref(x, gamma, beta, Q, eps)
    mask = z > 0
    dx, dgamma, dbeta, part = R.gn_backward_ref(x, dy, gamma, beta, Q, eps, mask)
    ty, tdx, tdg, tdb = R.gn_torch_ref(x, dy, gamma, beta, H, W, Q, eps)
    # the constant group has variance 0 in both, the offset case a variance 4e6 times below the mean square: torch's float64
    # statistics carry ~1e-16 * 4e6 of that into rstd
    tol = 1e-7 if kind == "offset" else 1e-11
    for got, want, what in ((y, ty, "y"), (dx, tdx, "dx"), (dgamma, tdg, "dgamma"), (dbeta, tdb, "dbeta")):
        assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max()), what
    assert np.allclose(part.sum(axis=(0, 1))[:, 0], dbeta, rtol=1e-12, atol=1e-12)
    assert np.allclose(part.sum(axis=(0, 1))[:, 1], dgamma, rtol=1e-12, atol=1e-12)
    if kind == "constant":
        assert (rstd[0, 1] == 1.0 / np.sqrt(np.float64(np.float32(eps)))) and (y[0, :, 4:8] == np.maximum(beta[4:8], 0).astype(np.float64)).all()
    # the ReLU edge: the reference alone stays within the cap of elements left out
    edge = np.abs(z) <= R.GN_Z_EDGE
    assert edge.mean() <= R.GN_EDGE_CAP, edge.sum()

    # the float32 form against every bar of the GPU test
    y32, z32, mean32, rstd32, _ = R.gn_forward_ref(x, gamma, beta, Q, eps, np.float32)
    mask32 = z32 > 0
    assert (mask32 == mask)[~edge].all()
    rel = lambda got, want: np.abs(got.astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
    r_y = np.abs((y32.astype(np.float64) - y) * ~edge).max() / max(1.0, np.abs(y).max()) / R.GN_Y_RTOL
    r_mean = (np.abs(mean32.astype(np.float64) - mean) / np.maximum(1.0, np.abs(mean))).max() / R.GN_MEAN_RTOL
    r_rstd = (np.abs(rstd32.astype(np.float64) - rstd) / rstd).max() / (R.GN_RSTD_RTOL_OFFSET if kind == "offset" else R.GN_RSTD_RTOL)
    dx_m, dg_m, db_m, part_m = R.gn_backward_ref(x, dy, gamma, beta, Q, eps, mask32)     # float64 with the float32 form's mask
    dx32, dg32, db32, part32 = R.gn_backward_ref(x, dy, gamma, beta, Q, eps, mask32, np.float32)
    r_dx, r_dg, r_db, r_part = (rel(a, b) / R.GN_GRAD_RTOL for a, b in ((dx32, dx_m), (dg32, dg_m), (db32, db_m), (part32, part_m)))
    print("f32 form / bar: y %.3f mean %.3f rstd %.3f dx %.3f dgamma %.3f dbeta %.3f part %.3f" % (r_y, r_mean, r_rstd, r_dx, r_dg, r_db, r_part))
    assert max(r_y, r_mean, r_rstd, r_dx, r_dg, r_db, r_part) <= 0.25
