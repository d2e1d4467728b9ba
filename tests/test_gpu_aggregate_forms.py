"""fpc_aggregate_bits through the C ABI on the hand-built label planes of tests/_aggregate_cases.py, in every launch form
and with every set of outputs, against the numpy float64 reference of tests/test_aggregate_reference.py (which a host test
holds against the C oracle).

Launch forms: `fused` (root_pix given: k_agg_fused, one launch) and `two_launch` (root_pix NULL: k_agg_accum, then
k_agg_planes_img, or k_agg_finalize when no plane output is wanted).  Output sets: all of masks, masked vote field, bit
words and stats; bit words (and stats) alone; masks alone; none.  With no plane output the library runs k_agg_accum +
k_agg_finalize whether root_pix is given or not.

Every output buffer has spare rows and is filled with a sentinel before the call (bit words with all ones), so an element
the kernels leave unwritten and a write past the last instance both show.  Integer outputs, planes, bit words and the
pixel count are exact; quaternion, scales, z and the mean quaternion's norm are within atol = rtol = 1e-5, the bar
tests/test_gpu_parity.py holds these fields to.  Both sides sum in float64 (the kernels in an unordered sequence of
atomics, hence no run-to-run bit identity is asked of the floats) and share the float32 tail.
"""
import numpy as np
import pytest
import torch

import _aggregate_cases as cases
import test_aggregate_reference as host

pytestmark = pytest.mark.gpu

FPC_OK, FPC_EINVAL, FPC_EWORKSPACE = 0, -1, -2
SENT_F = -777.25                     # exactly representable; no kernel output takes this value
SENT_I = -0x5A5A5A5A5A5A5A5A
SPARE = 2                            # rows behind the last one the call may write

FORMS = ("fused", "two_launch")
OUTSETS = {                          # name -> (masks, xy, bits, stats)
    "full": (True, True, True, True),
    "bits": (False, False, True, True),
    "masks": (True, False, False, False),
    "none": (False, False, False, False),
}
INT_KEYS = ("class_ids", "sample_ids")
PLANE_KEYS = ("instance_masks", "xy", "bits")
FLOAT_KEYS = ("quaternion", "scales", "z")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def nat(dev):
    from fastposecnn_amd import _native
    _native.lib()                             # raises if libfpc_hip.so is missing: no silent fallback
    return _native


_inputs = {}


def inputs(name, dev):
    """The case's inputs on the device: uploaded once, never written."""
    if name not in _inputs:
        c = cases.make(name)
        _inputs[name] = {k: torch.from_numpy(np.array(c[k])).to(dev)           # a copy: the case's arrays are read-only
                         for k in ("labels", "cat_mask", "quat", "scales", "xy", "z", "root_pix")}
    return _inputs[name]


def alloc_outputs(dev, rows, H, W, outset, nat):
    masks, xy, bits, stats = OUTSETS[outset]
    f = dict(dtype=torch.float32, device=dev)
    nw = nat.lib().fpc_mask_bits_words(H, W)
    assert nw == host.mask_bits_words(H, W)
    return {
        "class_ids": torch.full((rows,), SENT_I, dtype=torch.int64, device=dev),
        "sample_ids": torch.full((rows,), SENT_I, dtype=torch.int64, device=dev),
        "quaternion": torch.full((rows, 4), SENT_F, **f),
        "scales": torch.full((rows, 3), SENT_F, **f),
        "z": torch.full((rows, 1), SENT_F, **f),
        "instance_masks": torch.full((rows, H, W), SENT_F, **f) if masks else None,
        "xy": torch.full((rows, 2, H, W), SENT_F, **f) if xy else None,
        "bits": torch.full((rows, nw), -1, dtype=torch.int64, device=dev) if bits else None,
        "stats": torch.full((rows, 2), SENT_F, **f) if stats else None,
    }


def call(nat, dev, name, form, out, N, n_dev=None, B=None, ws=None, ws_bytes=None, xy_ptr=None, masks_ptr=None):
    """One fpc_aggregate_bits call on case `name` with capacity / count N; returns the code."""
    c, t = cases.make(name), inputs(name, dev)
    L = nat.lib()
    root = None
    if form == "fused":
        root = torch.zeros(max(N, 1), dtype=torch.int32, device=dev)        # entries past the count are never read
        k = min(N, c["n"])
        root[:k] = t["root_pix"][:k]
    if ws is None:
        wst = nat.workspace("agg", dev, L.fpc_aggregate_workspace_bytes(N))
        ws = wst.data_ptr()
        ws_bytes = wst.numel() if ws_bytes is None else ws_bytes
    with torch.cuda.device(dev):
        rc = L.fpc_aggregate_bits(
            nat.ptr(t["labels"]), nat.ptr(t["cat_mask"]), nat.ptr(t["quat"]), nat.ptr(t["scales"]),
            nat.ptr(t["xy"]) if xy_ptr is None else xy_ptr, nat.ptr(t["z"]),
            c["B"] if B is None else B, c["H"], c["W"], N, nat.ptr(n_dev),
            nat.ptr(out["class_ids"]), nat.ptr(out["sample_ids"]),
            nat.ptr(out["instance_masks"]) if masks_ptr is None else masks_ptr,
            nat.ptr(out["quaternion"]), nat.ptr(out["scales"]), nat.ptr(out["z"]), nat.ptr(out["xy"]),
            nat.ptr(out["stats"]), nat.ptr(out["bits"]), nat.ptr(root), ws, ws_bytes, nat.stream())
        torch.cuda.synchronize()
    return rc


def run(nat, dev, name, form, outset, N=None, n_dev=None):
    c = cases.make(name)
    N = c["n"] if N is None else N
    out = alloc_outputs(dev, N + SPARE, c["H"], c["W"], outset, nat)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=dev)
    assert call(nat, dev, name, form, out, N, n_dev=nd) == FPC_OK
    return out


def deviation(got, want):
    """Worst |got - want| in units of the bar atol + rtol |want| (atol = rtol = 1e-5)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / (1e-5 + 1e-5 * np.abs(want))).max()) if got.size else 0.0


def check(out, ref, k, what):
    """Rows [0, k) of every output equal the reference's, every row behind them still holds the sentinel."""
    for key, t in out.items():
        if t is None:
            continue
        got = t.cpu().numpy()
        head, tail, want = got[:k], got[k:], ref[key][:k]
        sent = -1 if key == "bits" else (SENT_I if key in INT_KEYS else np.float32(SENT_F))
        assert tail.shape[0] >= SPARE and (tail == sent).all(), f"{what}: {key} written behind row {k - 1}"
        assert head.shape == want.shape and head.dtype == want.dtype, f"{what}: {key}"
        if key in FLOAT_KEYS:
            np.testing.assert_allclose(head, want, atol=1e-5, rtol=1e-5, err_msg=f"{what}: {key}")
        elif key == "stats":
            assert np.array_equal(head[:, 0], want[:, 0]), f"{what}: pixel counts"
            np.testing.assert_allclose(head[:, 1], want[:, 1], atol=1e-5, rtol=1e-5, err_msg=f"{what}: quaternion norm")
        else:
            bad = np.flatnonzero((head != want).reshape(k, -1).any(axis=1))
            assert bad.size == 0, f"{what}: {key} differs in {bad.size} instances, first {bad[:8].tolist()}"


@pytest.mark.parametrize("outset", OUTSETS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_aggregate_equals_reference(nat, dev, name, form, outset):
    n = cases.make(name)["n"]
    check(run(nat, dev, name, form, outset), host.reference(name), n, f"{name} {form} {outset}")


@pytest.mark.parametrize("outset", OUTSETS)
@pytest.mark.parametrize("name", cases.NAMES)
def test_forms_agree(nat, dev, name, outset):
    """The fused and the two-launch form: identical integer outputs, planes and bit words, spare rows included."""
    a, b = (run(nat, dev, name, form, outset) for form in FORMS)
    for key in INT_KEYS + PLANE_KEYS:
        assert (a[key] is None) == (b[key] is None)
        if a[key] is not None:
            assert torch.equal(a[key], b[key]), f"{name} {outset}: {key}"
    if a["stats"] is not None:
        assert torch.equal(a["stats"][:, 0], b["stats"][:, 0]), f"{name} {outset}: pixel counts"


GATED = "cells8-40x72-B3"            # two images of 8 x 8 cells, dozens of instances under one workgroup


@pytest.mark.parametrize("outset", ("full", "none"))
@pytest.mark.parametrize("form", FORMS)
def test_capacity_above_the_device_count(nat, dev, form, outset):
    """N = n + 3 rows of capacity, n_dev = n: rows 0..n-1 as the reference, rows n.. untouched."""
    n = cases.make(GATED)["n"]
    out = run(nat, dev, GATED, form, outset, N=n + 3, n_dev=n)
    check(out, host.reference(GATED), n, f"capacity {form} {outset}")


@pytest.mark.parametrize("outset", ("full", "none"))
@pytest.mark.parametrize("form", FORMS)
def test_device_count_below_the_labels(nat, dev, form, outset):
    """The same gate from the other side: n_dev = n - 2 under a capacity of n + 3 drops the labels above n - 2."""
    n = cases.make(GATED)["n"]
    out = run(nat, dev, GATED, form, outset, N=n + 3, n_dev=n - 2)
    check(out, host.reference(GATED), n - 2, f"n_dev below {form} {outset}")


@pytest.mark.parametrize("outset", ("full", "none"))
@pytest.mark.parametrize("form", FORMS)
def test_n_below_the_largest_label(nat, dev, form, outset):
    """N = n - 2 without n_dev: labels n - 1 and n are present and dropped.  Instances do not depend on each other, so rows
    0..N-1 are the reference's; nothing is written behind them."""
    c = cases.make(GATED)
    n = c["n"]
    assert (c["labels"] > n - 2).any()
    ref = host.reference(GATED)
    restricted = host.reference_of(c["labels"], c["cat_mask"], c["quat"], c["scales"], c["xy"], c["z"], n - 2)
    for key in restricted:
        assert np.array_equal(restricted[key], ref[key][:n - 2]), key
    check(run(nat, dev, GATED, form, outset, N=n - 2), restricted, n - 2, f"N below {form} {outset}")


SMALL = "tiny-3x5-B1"


def _untouched(out):
    for key, t in out.items():
        if t is not None:
            sent = -1 if key == "bits" else (SENT_I if key in INT_KEYS else SENT_F)
            assert bool((t == sent).all()), key


@pytest.mark.parametrize("form", FORMS)
def test_refusals_and_empty_calls(nat, dev, form):
    """Return codes of the calls that launch nothing; the outputs keep their sentinel."""
    c = cases.make(SMALL)
    n = c["n"]
    L = nat.lib()
    out = alloc_outputs(dev, n + SPARE, c["H"], c["W"], "full", nat)
    assert call(nat, dev, SMALL, form, out, 65536) == FPC_EINVAL
    assert call(nat, dev, SMALL, form, out, n, B=65536) == FPC_EINVAL
    need = L.fpc_aggregate_workspace_bytes(n)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    assert call(nat, dev, SMALL, form, out, n, ws=ws.data_ptr(), ws_bytes=need - 1) == FPC_EWORKSPACE
    assert call(nat, dev, SMALL, form, out, n, ws=ws.data_ptr() + 128, ws_bytes=need + 256) == FPC_EWORKSPACE
    assert call(nat, dev, SMALL, form, out, n, xy_ptr=inputs(SMALL, dev)["xy"].data_ptr() + 4) == FPC_EINVAL
    assert call(nat, dev, SMALL, form, out, n, masks_ptr=out["instance_masks"].data_ptr() + 4) == FPC_EINVAL
    assert call(nat, dev, SMALL, form, out, 0) == FPC_OK
    assert call(nat, dev, SMALL, form, out, n, B=0) == FPC_OK
    _untouched(out)
    # the same buffers, the same workspace at exactly its size: the call is accepted and right
    assert call(nat, dev, SMALL, form, out, n, ws=ws.data_ptr(), ws_bytes=need) == FPC_OK
    check(out, host.reference(SMALL), n, f"refusals {form}")


def test_layer_with_more_components_than_root_pixels(nat, dev, oracle):
    """AggregationLayer on one image with 302 connected components: more than the 256 root pixels the layer keeps for
    B = 1, so neither forward nor forward_deferred may hand them to the aggregation (whose fused form would read past
    them); all outputs equal the oracle's, and the attached bit words equal the masks."""
    import fastposecnn_amd.lib  # noqa: F401  (puts the drop-in modules on sys.path)
    import aggregation_layer as al
    cat_cpu = cases.lattice_scene()
    want = oracle.aggregate(cat_cpu)
    n = want["class_ids"].shape[0]
    assert n == 302
    cat = {k: torch.from_numpy(v).to(dev) for k, v in cat_cpu.items()}
    layer = al.AggregationLayer(None, 7)
    labels, count = layer.batchwise_break_segmentation_mask(cat["mask"])
    assert count == n and np.array_equal(labels.cpu().numpy(), want["labels"])
    assert labels._fpc_root_pix[0].numel() == 256 < n
    cap = 320
    deferred, n_dev = layer.forward_deferred(cat, cap)
    assert int(n_dev.item()) == n
    for what, agg in (("forward", layer.forward(cat)), ("forward_deferred", deferred)):
        rows = n if what == "forward" else cap
        for k in ("class_ids", "sample_ids", "instance_masks", "xy"):
            got = agg[k].cpu().numpy()
            assert got.shape[0] == rows and got.dtype == want[k].dtype
            assert np.array_equal(got[:n], want[k]), f"{what}: {k}"
        for k in FLOAT_KEYS:
            got = agg[k].cpu().numpy()
            assert got.shape == (rows,) + want[k].shape[1:]
            np.testing.assert_allclose(got[:n], want[k], atol=1e-5, rtol=1e-5, err_msg=f"{what}: {k}")
        bits = al.mask_bits_of(agg["instance_masks"])
        assert bits is not None and bits.shape[0] == rows
        assert np.array_equal(bits.cpu().numpy()[:n], host.pack_bits(agg["instance_masks"].cpu().numpy()[:n])), what
