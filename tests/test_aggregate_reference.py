"""Two independent statements of the aggregation on the hand-built label planes of tests/_aggregate_cases.py, held against
each other on the host: a numpy float64 restatement written here (`reference`, which the GPU tests of
tests/test_gpu_aggregate_forms.py compare the kernels with) and the committed C oracle's fpco_aggregate on the same labels.

Integer outputs and planes must agree bit for bit, floats within atol = rtol = 1e-5 (the bar tests/test_gpu_parity.py holds
these fields to).  Both sum in float64 and share the float32 tail, so the honest difference is a few float32 ulps.  No GPU.
"""
import functools

import numpy as np
import pytest

import _aggregate_cases as cases


def mask_bits_words(H, W):
    """fpc_mask_bits_words: whole 4096-pixel chunks of 64-bit words."""
    return -(-(H * W) // 4096) * 64


def pack_bits(masks):
    """[n,H,W] masks -> i64 [n, mask_bits_words]: bit j of word w = pixel 64 w + j, zero past H W."""
    n, H, W = masks.shape
    flat = np.zeros((n, mask_bits_words(H, W) * 64), np.uint8)
    flat[:, :H * W] = masks.reshape(n, -1) != 0
    return np.packbits(flat, axis=1, bitorder="little").view(np.uint64).astype(np.int64).reshape(n, -1)


def reference_of(labels, cat_mask, quat, scales, xy, z, n):
    """The aggregation of labels 1..n in numpy: float64 sums (np.bincount), then the kernel's float32 tail — the means cast
    to float32, the quaternion's norm, the division and exp(z) in float32."""
    B, H, W = labels.shape
    HW = H * W
    lab = labels.astype(np.int64).ravel()
    lab = np.where(lab > n, 0, lab)                                  # labels above n are dropped
    cnt = np.bincount(lab, minlength=n + 1)[1:]
    assert (cnt > 0).all()

    def mean(plane):                                                 # plane [B,H,W] -> f32 [n]
        s = np.bincount(lab, weights=plane.astype(np.float64).ravel(), minlength=n + 1)[1:]
        return (s / cnt.astype(np.float64)).astype(np.float32)

    q = np.stack([mean(quat[:, a]) for a in range(4)], axis=1)
    nq = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    assert q.dtype == np.float32 and nq.dtype == np.float32
    div = np.where(nq == 0, np.float32(1), nq)
    # smallest non-zero class of the instance, 0 when there is none
    cm = cat_mask.astype(np.int64).ravel()
    big = np.iinfo(np.int64).max
    cls = np.full(n + 1, big, np.int64)
    np.minimum.at(cls, lab, np.where(cm != 0, cm, big))
    cls = np.where(cls[1:] == big, 0, cls[1:])
    # the image of an instance: that of any of its pixels
    img = np.repeat(np.arange(B), HW)
    sid = np.full(n + 1, -1, np.int64)
    sid[lab] = img
    sid = sid[1:]
    # planes: the mask of instance i inside its own image, the vote field under it
    own = labels.reshape(B, HW)[sid] == np.arange(1, n + 1)[:, None]           # [n, HW]
    masks = own.astype(np.float32).reshape(n, H, W)
    oxy = np.where(own[:, None, :], xy.reshape(B, 2, HW)[sid], np.float32(0)).astype(np.float32).reshape(n, 2, H, W)
    return {
        "class_ids": cls, "sample_ids": sid, "instance_masks": masks, "xy": oxy,
        "quaternion": (q / div[:, None]).astype(np.float32),
        "scales": np.stack([mean(scales[:, a]) for a in range(3)], axis=1),
        "z": np.exp(mean(z)).astype(np.float32)[:, None],
        "stats": np.stack([cnt.astype(np.float32), nq], axis=1),
        "bits": pack_bits(masks),
    }


@functools.lru_cache(maxsize=None)
def reference(name):
    """The expected outputs of case `name`; computed once per session, read-only."""
    c = cases.make(name)
    ref = reference_of(c["labels"], c["cat_mask"], c["quat"], c["scales"], c["xy"], c["z"], c["n"])
    for v in ref.values():
        v.setflags(write=False)
    return ref


@pytest.mark.parametrize("name", cases.NAMES)
def test_case_keeps_the_kernels_contract(name):
    c = cases.make(name)
    cases.check_contract(c)
    B, H, W = c["labels"].shape
    assert c["cat_mask"].shape == (B, H, W) and c["cat_mask"].dtype == np.int64
    assert c["quat"].shape == (B, 4, H, W) and c["scales"].shape == (B, 3, H, W)
    assert c["xy"].shape == (B, 2, H, W) and c["z"].shape == (B, H, W)
    assert all(c[k].dtype == np.float32 for k in ("quat", "scales", "xy", "z"))


def test_generator_covers_what_it_promises():
    """Shapes, batch sizes, all-background images first / middle / last, instance counts above 256 and above four per tile,
    and the special instances; with the expected values they must produce."""
    shapes = {(c["H"], c["W"]) for c in map(cases.make, cases.NAMES)}
    assert {(40, 72), (67, 93), (64, 128), (3, 5), (16, 24)} <= shapes
    assert {cases.make(n)["B"] for n in cases.NAMES} == {1, 3, 5}
    bg = {"first": 0, "middle": 0, "last": 0}
    for name in cases.NAMES:
        c = cases.make(name)
        e = [not c["labels"][b].any() for b in range(c["B"])]
        if c["B"] > 1:
            bg["first"] += e[0]; bg["last"] += e[-1]; bg["middle"] += any(e[1:-1])
    assert bg["first"] >= 1 and bg["last"] >= 1 and bg["middle"] >= 3
    assert cases.make("cells4-64x128-B1")["n"] == 512 and cases.make("everypixel-16x24-B1")["n"] == 384
    for name in ("cells8-40x72-B3", "cells8-67x93-B5", "cells4-64x128-B1"):
        lab = cases.make(name)["labels"]
        per_tile = max(np.unique(lab[b, y:y + 32, x:x + 64]).size for b in range(lab.shape[0])
                       for y in range(0, lab.shape[1], 32) for x in range(0, lab.shape[2], 64))
        assert per_tile >= 20, name                                  # far above the four LDS slots
    seam = cases.make("seams-64x128-B1")
    assert seam["n"] == len(cases.seam_pixels(64, 128)) == 20 and (np.bincount(seam["labels"].ravel())[1:] == 1).all()
    seen = {"class_1000": 0, "class_0": 0, "zero_quat": 0, "mixed": 0}
    for name in cases.NAMES:
        c, r = cases.make(name), reference(name)
        sp = c["special"]
        if sp["class_1000"] is not None:
            assert r["class_ids"][sp["class_1000"]] == 1000; seen["class_1000"] += 1
        if sp["class_0"] is not None:
            assert r["class_ids"][sp["class_0"]] == 0; seen["class_0"] += 1
        if sp["zero_quat"] is not None:
            i = sp["zero_quat"]
            assert r["stats"][i, 1] == 0 and not r["quaternion"][i].any(); seen["zero_quat"] += 1
        # an instance with class-0 pixels and two non-zero classes: the smaller non-zero one wins
        for i in range(c["n"]):
            cl = np.unique(c["cat_mask"][c["labels"] == i + 1])
            if cl.size >= 3 and cl[0] == 0:
                assert r["class_ids"][i] == cl[1] and 1 <= cl[1] <= 6; seen["mixed"] += 1
        other = np.delete(np.arange(c["n"]), [i for i in (sp["zero_quat"],) if i is not None])
        assert (r["stats"][other, 1] > 0.5).all()                    # the mean's norm stays well away from zero
    assert min(seen.values()) >= 5, seen


@pytest.mark.parametrize("name", cases.NAMES)
def test_numpy_reference_equals_oracle(oracle, name):
    c, ref = cases.make(name), reference(name)
    cat = {"mask": c["cat_mask"], "quaternion": c["quat"], "scales": c["scales"], "xy": c["xy"], "z": c["z"]}
    want = oracle.aggregate_labels(c["labels"], cat, c["n"])
    for k in ("class_ids", "sample_ids", "instance_masks", "xy"):
        assert want[k].dtype == ref[k].dtype and np.array_equal(want[k], ref[k]), k
    for k in ("quaternion", "scales", "z"):
        assert want[k].shape == ref[k].shape and want[k].dtype == ref[k].dtype == np.float32
        np.testing.assert_allclose(ref[k], want[k], atol=1e-5, rtol=1e-5, err_msg=k)
    # the parts the oracle does not state, from what it does: pixel counts and bit words follow from the masks
    assert np.array_equal(ref["stats"][:, 0], want["instance_masks"].sum(axis=(1, 2), dtype=np.float64))
    assert np.array_equal(ref["bits"], pack_bits(want["instance_masks"]))
    assert ref["bits"].shape == (c["n"], mask_bits_words(c["H"], c["W"]))


def test_oracle_refuses_a_label_above_n(oracle):
    c = cases.make("tiny-3x5-B1")
    cat = {"mask": c["cat_mask"], "quaternion": c["quat"], "scales": c["scales"], "xy": c["xy"], "z": c["z"]}
    with pytest.raises(RuntimeError):
        oracle.aggregate_labels(c["labels"], cat, c["n"] - 1)


def test_oracle_aggregate_still_labels_by_itself(oracle):
    """aggregate() = cc_label + aggregate_labels: unchanged for its callers."""
    cat = cases.lattice_scene()
    a = oracle.aggregate(cat)
    labels, n = oracle.cc_label(cat["mask"] != 0)
    assert n == 302
    b = oracle.aggregate_labels(labels, cat, n)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
