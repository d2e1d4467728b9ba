"""The host half of the device-built ground truth (tools/dataset.py: NOCSDataset.gt_item, gt_tables, build_gt_host; csrc/gt_build.hip's
argument checks).  No GPU: fpc_gt_build returns FPC_EINVAL before any launch, PNG decoding is the library's host code.
gt_item + build_gt_host — the definition of what the kernel computes — must give what `__getitem__` + `my_collate_fn` give on the
committed fixture, key by key and exactly; `__getitem__` itself, whose table code gt_item now shares, is held to nocs_sample.npz
here a second time."""
import json
import shutil

import numpy as np
import pytest

import _gt_cases as C

FPC_EINVAL = -1
P = 4096          # a non-null, 16-byte aligned address that is never dereferenced: every call below returns before a launch


@pytest.fixture(scope="module")
def D():
    from fastposecnn_amd.tools import dataset as D
    return D


@pytest.fixture(scope="module")
def L():
    from fastposecnn_amd import _native
    return _native.lib()


def test_entry_points_are_exported(L):
    from fastposecnn_amd import _native
    assert "fpc_gt_build" in _native.EXPORTED and "fpc_depth_decode" in _native.EXPORTED
    assert L.fpc_gt_build is not None and L.fpc_depth_decode is not None


GOOD = dict(ids=P, pix_stride=1, frame_stride=35, B=1, H=5, W=7, row_of=P, class_of=P, first_row=P, n=2, class_mask=P, inst=P,
            elem=8, count=P)


@pytest.mark.parametrize("change", [dict(ids=None), dict(row_of=None), dict(class_of=None), dict(first_row=None),
                                    dict(B=0), dict(H=0), dict(W=0), dict(H=-5, W=-7), dict(n=-1), dict(n=32768),
                                    dict(elem=2), dict(elem=0), dict(elem=16),
                                    dict(pix_stride=0), dict(pix_stride=5), dict(pix_stride=-1),
                                    dict(inst=P + 8), dict(inst=P + 1)],
                         ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_bad_arguments_are_refused_before_any_launch(L, change):
    a = dict(GOOD, **change)
    rc = L.fpc_gt_build(a["ids"], a["pix_stride"], a["frame_stride"], a["B"], a["H"], a["W"], a["row_of"], a["class_of"],
                        a["first_row"], a["n"], a["class_mask"], a["inst"], a["elem"], a["count"], None)
    assert rc == FPC_EINVAL


def test_depth_decode_refuses_bad_arguments(L):
    assert L.fpc_depth_decode(None, 0, 3, 1, 5, 7, P, None) == FPC_EINVAL
    assert L.fpc_depth_decode(P, 0, 3, 1, 5, 7, None, None) == FPC_EINVAL
    assert L.fpc_depth_decode(P, 2, 3, 1, 5, 7, P, None) == FPC_EINVAL
    assert L.fpc_depth_decode(P, 0, 2, 1, 5, 7, P, None) == FPC_EINVAL
    assert L.fpc_depth_decode(P, 1, 1, 0, 5, 7, P, None) == FPC_EINVAL


def test_gt_item_and_build_gt_host_equal_the_host_collate(D):
    ds = C.dataset()
    assert len(ds) == 2
    items = [ds.gt_item(i) for i in range(2)]
    for i, item in enumerate(items):
        assert set(item) == {"path", "mask_path", "ids", "class_values", "valid", "table"}
        assert item["valid"] is True and item["path"] == ds.images_fps[i] and item["mask_path"].endswith("_mask.png")
        assert set(item["table"]) == {k for k, _ in D.GT_TABLE_KEYS}
    ids = np.stack([D.imread_png(it["mask_path"]) for it in items])          # the mask files as stored: RGBA
    assert ids.dtype == np.uint8 and ids.shape == (2, 48, 64, 4)
    got, count = C.collate_gt_host(D, items, ids)
    want = D.my_collate_fn([ds[0], ds[1]])
    assert got["mask"].dtype == np.int64 and np.array_equal(got["mask"], want["mask"].numpy())
    assert set(got["agg_data"]) == set(want["agg_data"])
    for key, w in want["agg_data"].items():
        g, w = got["agg_data"][key], w.numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), key
    assert np.array_equal(count, want["agg_data"]["instance_masks"].numpy().sum(axis=(1, 2))) and (count > 0).all()
    # the first channel alone is the same batch
    got1, _ = C.collate_gt_host(D, items, np.ascontiguousarray(ids[..., 0]))
    assert np.array_equal(got1["mask"], got["mask"])
    assert np.array_equal(got1["agg_data"]["instance_masks"], got["agg_data"]["instance_masks"])


def test_item_with_an_object_behind_the_camera_is_not_valid():
    ds = C.dataset("scene_b", preprocessing=False)
    assert len(ds) == 1 and ds[0] is None and ds.gt_item(0)["valid"] is False


@pytest.mark.parametrize("bad_id", ["0", "255", "300"])
def test_side_file_with_an_id_outside_the_mask_bytes_raises(tmp_path, bad_id):
    src = C.ROOT / "scene_a"
    shutil.copy(src / "0000_color.png", tmp_path / "0000_color.png")
    side = json.load(open(src / "0000_meta+.json"))
    side["instance_dict"] = {(bad_id if k == "1" else k): v for k, v in side["instance_dict"].items()}
    json.dump(side, open(tmp_path / "0000_meta+.json", "w"))
    from fastposecnn_amd.tools import dataset as D
    ds = D.CAMERADataset(tmp_path, classes=C.gold_classes())
    assert len(ds) == 1
    with pytest.raises(ValueError):
        ds.gt_item(0)


def test_build_gt_host_on_adversarial_tables(D):
    """The restatement itself on a case whose answer is known by construction."""
    ids, row_of, class_of, first_row, n = C.adversarial(5, 7, "three_frames", 4, 0)
    cm, inst, count = D.build_gt_host(ids, 4, row_of, class_of, first_row, n, np.uint8)
    assert n == 41 and inst.dtype == np.uint8 and cm.dtype == np.int64 and count.dtype == np.int32
    assert inst[40].all() and count[40] == 35 and (cm[2] == 5).all()          # the frame that is one instance
    assert inst[:40].sum() ==(row_of[0][ids[0, ..., 0]] >= 0).sum()
    assert (count[:40] == 0).any()                                            # the listed id without a pixel


def test_getitem_still_returns_the_reference_sample():
    """tests/test_dataset_gt.py's assertion, repeated for the refactored table code."""
    gold = np.load(C.GOLD, allow_pickle=False)
    ds = C.dataset()
    order = {str(p.relative_to(C.ROOT)): i for i, p in enumerate(ds.images_fps)}
    for gi, rel in enumerate(str(p) for p in gold["paths"]):
        s = ds[order[rel]]
        assert set(s) == {"clean_image", "image", "mask", "depth", "path", "agg_data"}
        for k in ("clean_image", "image", "mask", "depth"):
            want = gold[f"s{gi}_{k}"]
            assert s[k].dtype == want.dtype and s[k].shape == want.shape, (k, s[k].dtype, want.dtype)
            assert np.array_equal(s[k], want), k
        want_keys = {k[len(f"s{gi}_agg_"):] for k in gold.files if k.startswith(f"s{gi}_agg_")}
        assert set(s["agg_data"]) == want_keys == {"class_ids", "symmetric_ids", "instance_masks", "quaternion", "scales", "xy", "z",
                                                   "T", "R", "RT"}
        assert list(s["agg_data"]) == ["class_ids", "symmetric_ids", "instance_masks", "quaternion", "scales", "xy", "z", "T", "R", "RT"]
        for k in want_keys:
            want = gold[f"s{gi}_agg_{k}"]
            got = s["agg_data"][k]
            assert got.dtype == want.dtype and got.shape == want.shape, k
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=k)
    s0 = ds[order["scene_a/0000_color.png"]]
    assert s0["agg_data"]["class_ids"].tolist() == [1.0, 2.0] and s0["agg_data"]["symmetric_ids"].tolist() == [1.0, 0.0]
    assert set(np.unique(s0["mask"]).tolist()) == {0, 1, 2}
