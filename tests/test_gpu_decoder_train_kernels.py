"""The training decoder's kernels, csrc/upsample.hip and csrc/groupnorm.hip, each called through the C ABI and held to the
float64 references of tests/_decoder_train_refs.py on the case tables there: every forward form and every pair of backward
forms fpc_upsample_bilinear_form can return (asserted per case, so a silent fall to the one-element-per-thread kernel fails),
the LDS patch at its full 4 x 34 extent, the rolled and the unrolled tap loop of every backward kernel, channel slices,
unaligned pointers and an expanded scalar as sources; GroupNorm at every group count, HW below, at and one past a chunk, the
wrapped grid-stride loops, a large offset, a constant group, gamma of both signs and 0.  Every destination and scratch buffer
is NaN before the call, exactly as long as the ABI says, and sits between two canary bands that must come back untouched.

What each bar is set against (float32 evaluation of the same formulas on the CPU against the float64 reference, measured at
every case by tests/test_decoder_train_refs_host.py, which also asserts the margin):
  upsample, reference A   |got - A| <= gamma_k S elementwise, S = the weights applied to |input| in float64, u = 2^-24,
                          gamma_k = k u / (1 - k u); derived in _decoder_train_refs.py, not measured: k = 6 for the forward
                          (two roundings of 1 - l1, then product, sum, product, sum), k = taps_x + taps_y for the adjoint (a
                          dot product of n taps from acc = 0 is n roundings deep; the x pass is stored in float32 and feeds
                          the y pass; 8 at scale 2, 18 .. 20 at scale 4 on these cases).
                          float32 form: at most 0.495 of the bar in the forward, 0.264 in the adjoint.
  upsample, reference B   2e-5 of max(1, |ref|max) against torch's float64 interpolate and its autograd (the bar of
                          test_native_bilinear_upsample_forward_and_adjoint_vs_torch: it allows for the float32 source
                          coordinate).  float32 form: at most 0.472 of the bar (forward, w = 130), 0.141 in the adjoint.
  vector form against     the same data through the one-element-per-thread kernel (every pointer one float off alignment):
  scalar form             within the reference-A bar of each other.  A backward run twice is bit-identical.
  GroupNorm               y 2e-5, dx / dgamma / dbeta / the per-chunk table 1e-4, each of max(1, |ref|max) (the bars of
                          test_native_groupnorm_relu_forward_and_backward_vs_float64); mean 1e-6 of max(1, |mean|); rstd 1e-5
                          relative, 2e-3 on the large-offset case.  float32 form, as a fraction of each bar: y 0.009,
                          mean 0.035, rstd 0.005, dx 0.001, dgamma 0.001, dbeta below 0.0005, table 0.001.
                          The large-offset input is stated on the grid 2^-10 with every sum the kernel rounds to float32
                          exactly representable (see _offset_input): 100 + 0.05 randn drawn freely has a group mean that
                          float32 holds to 3.8e-6, which is 7.6e-5 of a normalised unit and beyond the y bar by itself.
  ReLU edge               elements with |z_ref| <= 1e-4 are left out of the y comparison, at most 0.1 % of a case (the host test
                          holds the reference to that); the kernel's mask may differ from the reference's only there, and the
                          gradients are compared against the float64 reference evaluated with the kernel's own mask.
"""
import numpy as np
import pytest
import torch

import _decoder_train_refs as R

pytestmark = pytest.mark.gpu

EINVAL = -1
NAN = float("nan")
CANARY = 12345.0
BAND = 64                      # floats, a multiple of 4: the band keeps the alignment of what it surrounds


def _nat():
    from fastposecnn_amd import _native as nat
    return nat, nat.lib()


class _Guarded:
    """n NaN floats `off` floats past 16-byte alignment, between two bands of CANARY."""

    def __init__(self, n, off=0):
        self.n, self.lo = n, BAND + off
        self.buf = torch.full((self.lo + n + BAND,), CANARY, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[self.lo:self.lo + n] = NAN
        self.ptr = self.buf.data_ptr() + 4 * self.lo

    def inside(self):
        return self.buf[self.lo:self.lo + self.n]

    def bands_untouched(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.lo + self.n:] == CANARY).all())

    def all_nan(self):
        return bool(torch.isnan(self.inside()).all())


class _Source:
    """A host buffer on the device, `off` floats past 16-byte alignment."""

    def __init__(self, host, off=0):
        self.buf = torch.full((off + host.size,), NAN, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.buf[off:] = torch.from_numpy(host)
        self.base = self.buf.data_ptr() + 4 * off

    def ptr(self, first=0):
        return self.base + 4 * first


def _low4(*ptrs):
    bits = 0
    for p in ptrs:
        bits |= p & 15
    return bits


def _logical(flat, B, C, Y, X, nhwc):
    t = flat.cpu().numpy().astype(np.float64)
    return t.reshape(B, Y, X, C).transpose(0, 3, 1, 2) if nhwc else t.reshape(B, C, Y, X)


# ---- fpc_upsample_bilinear_fwd -------------------------------------------------------------------------------------------------------


def _run_fwd(case, values):
    nat, L = _nat()
    B, C, h, w, s = (case[k] for k in ("B", "C", "h", "w", "scale"))
    host, st, first = R.scatter_source(values, case["src"])
    src = _Source(host, case["off"][0])
    out = _Guarded(B * C * h * s * w * s, case["off"][1])
    form = L.fpc_upsample_bilinear_form(0, _low4(src.ptr(first), out.ptr), *st, B, C, h, w, s, case["dst_nhwc"])
    assert form == case["form"], (case["name"], form)
    assert _low4(src.ptr(first), out.ptr) == R.up_low4(case, False)
    nat.check(L.fpc_upsample_bilinear_fwd(src.ptr(first), *st, out.ptr, B, C, h, w, s, case["dst_nhwc"], nat.stream()), case["name"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.inside()).all()), case["name"]
    assert out.bands_untouched(), case["name"]
    return _logical(out.inside(), B, C, h * s, w * s, case["dst_nhwc"])


@pytest.mark.parametrize("case", R.UP_FWD_CASES, ids=R.up_case_id)
def test_upsample_forward_every_form_vs_float64(case):
    v = R.up_values(case, False)
    A, S = R.up_forward_A(v, case["scale"])
    ref_b = R.up_forward_B(v, case["scale"])
    got = _run_fwd(case, v)
    bar_a = R.gamma_k(R.K_UP_FWD) * S
    print(case["name"], "err / bar A", (np.abs(got - A) / bar_a).max(), "err B", np.abs(got - ref_b).max())
    assert (np.abs(got - A) <= bar_a).all()
    assert np.abs(got - ref_b).max() <= R.UP_B_RTOL * max(1.0, np.abs(ref_b).max())
    if case["form"] != R.FWD_SCALAR:
        scalar = _run_fwd(R.forced_scalar(case, False), v)
        assert (np.abs(got - scalar) <= bar_a).all()


# ---- fpc_upsample_bilinear_bwd -------------------------------------------------------------------------------------------------------


def _run_bwd(case, values):
    nat, L = _nat()
    B, C, h, w, s = (case[k] for k in ("B", "C", "h", "w", "scale"))
    host, st, first = R.scatter_source(values, case["src"])
    src = _Source(host, case["off"][0])
    din = _Guarded(B * C * h * w, case["off"][1])
    n_scratch = L.fpc_upsample_bilinear_bwd_scratch_floats(B, C, h, w, s)
    assert n_scratch == B * C * h * s * w
    scratch = _Guarded(n_scratch, case["off"][2])
    bits = _low4(src.ptr(first), din.ptr, scratch.ptr)
    code = L.fpc_upsample_bilinear_form(1, bits, *st, B, C, h, w, s, case["dst_nhwc"])
    assert (code & 15, code >> 4) == case["form"], (case["name"], code)
    assert bits == R.up_low4(case, True)
    nat.check(L.fpc_upsample_bilinear_bwd(src.ptr(first), *st, din.ptr, scratch.ptr, B, C, h, w, s, case["dst_nhwc"], nat.stream()),
              case["name"])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(din.inside()).all()) and bool(torch.isfinite(scratch.inside()).all()), case["name"]
    assert din.bands_untouched() and scratch.bands_untouched(), case["name"]
    return _logical(din.inside(), B, C, h, w, case["dst_nhwc"])


@pytest.mark.parametrize("case", R.UP_BWD_CASES, ids=R.up_case_id)
def test_upsample_backward_every_form_pair_vs_float64(case):
    g = R.up_values(case, True)
    A, S = R.up_adjoint_A(g, case["scale"])
    ref_b = R.up_adjoint_B(g, case["scale"])
    got = _run_bwd(case, g)
    bar_a = R.gamma_k(R.k_up_bwd(case["h"], case["w"], case["scale"])) * S
    print(case["name"], "err / bar A", (np.abs(got - A) / bar_a).max(), "err B", np.abs(got - ref_b).max())
    assert (np.abs(got - A) <= bar_a).all()
    assert np.abs(got - ref_b).max() <= R.UP_B_RTOL * max(1.0, np.abs(ref_b).max())
    assert np.array_equal(_run_bwd(case, g), got)                                    # no atomics: bit-identical
    if case["form"] != (R.BWD_SCALAR, R.BWD_SCALAR):
        scalar = _run_bwd(R.forced_scalar(case, True), g)
        assert (np.abs(got - scalar) <= bar_a).all()


def test_upsample_argument_contract():
    nat, L = _nat()
    B, C, h, w = 2, 3, 4, 5
    x = torch.randn((B, C, h, w), device="cuda")
    st = x.stride()
    out = _Guarded(B * C * h * 4 * w * 4)
    din = _Guarded(B * C * h * w)
    scratch = _Guarded(B * C * h * 4 * w)
    g = torch.randn((B, C, 4 * h, 4 * w), device="cuda")
    gs = g.stride()

    def fwd(src=x.data_ptr(), dst=out.ptr, B=B, C=C, scale=2, nhwc=0):
        return L.fpc_upsample_bilinear_fwd(src, *st, dst, B, C, h, w, scale, nhwc, nat.stream())

    def bwd(src=g.data_ptr(), dst=din.ptr, tmp=scratch.ptr, B=B, C=C, scale=4):
        return L.fpc_upsample_bilinear_bwd(src, *gs, dst, tmp, B, C, h, w, scale, 0, nat.stream())

    for call in (fwd, bwd):
        assert call(scale=1) == EINVAL and call(scale=3) == EINVAL
        assert call(src=None) == EINVAL and call(dst=None) == EINVAL
        assert call(B=256, C=256) == EINVAL                                          # 65 536 planes of an NCHW destination
    assert bwd(tmp=None) == EINVAL
    assert L.fpc_upsample_bilinear_form(0, 0, *st, 256, 256, h, w, 2, 0) == EINVAL
    assert L.fpc_upsample_bilinear_form(1, 0, *gs, 256, 256, h, w, 4, 0) == EINVAL
    assert L.fpc_upsample_bilinear_form(0, 0, *st, B, C, h, w, 3, 0) == EINVAL
    torch.cuda.synchronize()
    assert out.all_nan() and din.all_nan() and scratch.all_nan()                     # a refused call writes nothing
    assert out.bands_untouched() and din.bands_untouched() and scratch.bands_untouched()
    for bad in ((0, C, h, w, 2), (B, 0, h, w, 2), (B, C, 0, w, 2), (B, C, h, 0, 2), (B, C, h, w, 0), (B, C, h, w, 1), (B, C, h, w, 3)):
        assert L.fpc_upsample_bilinear_bwd_scratch_floats(*bad) == 0
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.inside()[:B * C * 4 * h * w]).all()) and bool(torch.isfinite(din.inside()).all())


# ---- fpc_groupnorm4_relu_fwd / _bwd ----------------------------------------------------------------------------------------------------


def _rel(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


@pytest.mark.parametrize("case", R.GN_CASES, ids=R.gn_case_id)
def test_groupnorm_relu_forward_and_backward_vs_float64(case):
    nat, L = _nat()
    B, C, H, W, Q, eps, kind = case
    HW = H * W
    x, dy, gamma, beta = R.gn_inputs(case)
    y_ref, z_ref, mean_ref, rstd_ref, _ = R.gn_forward_ref(x, gamma, beta, Q, eps)
    xd, dyd, gd, bd = (_Source(a.reshape(-1)) for a in (x, dy, gamma, beta))
    chunks = -(-HW // R.GN_CHUNK)
    n_part = L.fpc_groupnorm4_relu_scratch_floats(B, HW, C)
    assert n_part == B * chunks * C * 2
    y, stats, part = _Guarded(B * HW * C), _Guarded(B * Q * 2), _Guarded(n_part)
    nat.check(L.fpc_groupnorm4_relu_fwd(xd.ptr(), gd.ptr(), bd.ptr(), y.ptr, stats.ptr, part.ptr, B, HW, C, Q, eps, nat.stream()), "forward")
    torch.cuda.synchronize()
    used = B * chunks * Q * 2                                                        # the forward's table is [B][chunks][Q][2]
    assert bool(torch.isfinite(y.inside()).all()) and bool(torch.isfinite(stats.inside()).all())
    assert bool(torch.isfinite(part.inside()[:used]).all()) and bool(torch.isnan(part.inside()[used:]).all())
    assert y.bands_untouched() and stats.bands_untouched() and part.bands_untouched()
    got_y = y.inside().cpu().numpy().astype(np.float64).reshape(B, HW, C)
    got_stats = stats.inside().cpu().numpy().astype(np.float64).reshape(B, Q, 2)

    err_mean = (np.abs(got_stats[..., 0] - mean_ref) / np.maximum(1.0, np.abs(mean_ref))).max()
    err_rstd = (np.abs(got_stats[..., 1] - rstd_ref) / rstd_ref).max()
    edge = np.abs(z_ref) <= R.GN_Z_EDGE
    assert edge.mean() <= R.GN_EDGE_CAP
    mask = got_y > 0
    assert ((mask == (z_ref > 0)) | edge).all()                                      # the masks differ on the edge only
    err_y = np.abs((got_y - y_ref) * ~edge).max() / max(1.0, np.abs(y_ref).max())
    print(case, "mean", err_mean, "rstd", err_rstd, "y", err_y)
    assert err_mean <= R.GN_MEAN_RTOL
    assert err_rstd <= (R.GN_RSTD_RTOL_OFFSET if kind == "offset" else R.GN_RSTD_RTOL)
    assert err_y <= R.GN_Y_RTOL
    if kind == "constant":
        assert np.array_equal(got_y[0, :, 4:8], np.broadcast_to(np.maximum(beta[4:8], 0).astype(np.float64), (HW, 4)))
        assert abs(got_stats[0, 1, 1] * np.sqrt(np.float64(np.float32(eps))) - 1.0) <= R.GN_RSTD_RTOL and got_stats[0, 1, 0] == 0.75

    dx, part_b = _Guarded(B * HW * C), _Guarded(n_part)
    nat.check(L.fpc_groupnorm4_relu_bwd(xd.ptr(), dyd.ptr(), gd.ptr(), bd.ptr(), stats.ptr, dx.ptr, part_b.ptr, B, HW, C, Q, nat.stream()),
              "backward")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(dx.inside()).all()) and bool(torch.isfinite(part_b.inside()).all())
    assert dx.bands_untouched() and part_b.bands_untouched() and stats.bands_untouched()
    assert np.array_equal(stats.inside().cpu().numpy().astype(np.float64).reshape(B, Q, 2), got_stats)    # read, not written
    got_dx = dx.inside().cpu().numpy().astype(np.float64).reshape(B, HW, C)
    got_part = part_b.inside().cpu().numpy().astype(np.float64).reshape(B, chunks, C, 2)
    # the kernel's mask where it computed z > 0 itself: on the edge the forward's output tells which side it took
    dx_ref, dgamma_ref, dbeta_ref, part_ref = R.gn_backward_ref(x, dy, gamma, beta, Q, eps, mask)
    sums = got_part.sum(axis=(0, 1))
    errs = {"dx": _rel(got_dx, dx_ref), "dgamma": _rel(sums[:, 1], dgamma_ref), "dbeta": _rel(sums[:, 0], dbeta_ref),
            "part": _rel(got_part, part_ref)}
    print(case, errs)
    for what, err in errs.items():
        assert err <= R.GN_GRAD_RTOL, (what, err)


def test_groupnorm_argument_contract():
    nat, L = _nat()
    B, HW, C, Q = 2, 5, 16, 4
    bufs = {k: _Source(np.ones(n + 4, np.float32)) for k, n in (("x", B * HW * C), ("dy", B * HW * C), ("gamma", C), ("beta", C))}
    y, dx, stats, part = _Guarded(B * HW * C + 4), _Guarded(B * HW * C + 4), _Guarded(B * Q * 2), _Guarded(B * C * 2)

    def fwd(B=B, HW=HW, C=C, Q=Q, shift=()):
        p = {k: v.ptr(1 if k in shift else 0) for k, v in bufs.items()}
        return L.fpc_groupnorm4_relu_fwd(p["x"], p["gamma"], p["beta"], y.ptr + (4 if "y" in shift else 0), stats.ptr, part.ptr, B, HW, C, Q,
                                         1e-5, nat.stream())

    def bwd(B=B, HW=HW, C=C, Q=Q, shift=()):
        p = {k: v.ptr(1 if k in shift else 0) for k, v in bufs.items()}
        return L.fpc_groupnorm4_relu_bwd(p["x"], p["dy"], p["gamma"], p["beta"], stats.ptr, dx.ptr + (4 if "y" in shift else 0), part.ptr,
                                         B, HW, C, Q, nat.stream())

    for call in (fwd, bwd):
        assert call(C=12) == EINVAL and call(C=20) == EINVAL                         # C != 4 * groups
        assert call(C=12, Q=3) == EINVAL and call(C=512, Q=128) == EINVAL
        assert call(B=65536) == EINVAL and call(B=0) == EINVAL and call(HW=0) == EINVAL
        for name in ("x", "y", "gamma", "beta"):
            assert call(shift=(name,)) == EINVAL, name                               # 4 bytes off 16-byte alignment
    assert bwd(shift=("dy",)) == EINVAL
    for bad in ((0, HW, C), (B, 0, C), (B, HW, 3), (B, HW, 0)):
        assert L.fpc_groupnorm4_relu_scratch_floats(*bad) == 0
    torch.cuda.synchronize()
    for g in (y, dx, stats, part):
        assert g.all_nan() and g.bands_untouched()
    assert fwd() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y.inside()[:B * HW * C]).all()) and bool(torch.isfinite(dx.inside()[:B * HW * C]).all())
