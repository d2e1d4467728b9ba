"""Ground-truth batches built on the device (csrc/gt_build.hip: fpc_gt_build, fpc_depth_decode; tools/dataset.py:
GroundTruthUploader) against the host path they stand in for (`__getitem__` + `my_collate_fn`) and against build_gt_host, the
numpy statement of the kernel.  Every comparison is exact: the outputs are integers, zeros and ones, and copies of float64
numbers computed on the host."""
import numpy as np
import pytest
import torch

import _gt_cases as C

pytestmark = pytest.mark.gpu

CANARY = 7
TORCH_OF = {8: torch.float64, 4: torch.float32, 1: torch.uint8}
NUMPY_OF = {8: np.float64, 4: np.float32, 1: np.uint8}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def D(dev):
    from fastposecnn_amd import _native
    _native.lib()
    from fastposecnn_amd.tools import dataset as D
    return D


@pytest.fixture(scope="module")
def fixture_batch(D, dev):
    """scene_a through the host path, once: the dataset, its gt items, its mask files and the host collate on the device."""
    ds = C.dataset()
    items = [ds.gt_item(i) for i in range(len(ds))]
    samples = [ds[i] for i in range(len(ds))]
    return ds, items, [C.mask_bytes(it) for it in items], samples, D.my_collate_fn(samples, dev)


def _same_batch(got, want, skip=()):
    assert got["mask"].dtype == torch.int64 and torch.equal(got["mask"], want["mask"])
    assert list(got["agg_data"])[:-1] == list(want["agg_data"]) and list(got["agg_data"])[-1] == "pixel_counts"
    for key, w in want["agg_data"].items():
        g = got["agg_data"][key]
        assert g.is_contiguous() and g.device == w.device, key
        if key in skip:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (key, g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        assert torch.equal(g, w), key


def test_fixture_through_upload_png_equals_the_host_collate(D, dev, fixture_batch):
    ds, items, files, samples, want = fixture_batch
    up = D.GroundTruthUploader(2, 48, 64, 4, device=dev, max_instances=8)
    got, ready = up.upload_png(files, items)
    ready.synchronize()
    _same_batch(got, want)
    agg = got["agg_data"]
    assert agg["sample_ids"].dtype == torch.int64 and agg["pixel_counts"].dtype == torch.int32
    assert torch.equal(agg["pixel_counts"].long(), agg["instance_masks"].sum(dim=(1, 2)).long())
    up.check(got)
    with pytest.raises(ValueError):
        D.GroundTruthUploader(2, 48, 64, 1, device=dev, max_instances=8).upload_png(files, items)      # RGBA files
    with pytest.raises(ValueError):
        D.GroundTruthUploader(2, 48, 32, 4, device=dev, max_instances=8).upload_png(files, items)      # another width
    with pytest.raises(ValueError):
        D.GroundTruthUploader(2, 48, 64, 4, device=dev, max_instances=2).upload_png(files, items)      # three rows
    with pytest.raises(ValueError):
        up.upload_png(files, [dict(items[0], valid=False), items[1]])


def _run_kernel(ids_dev, base_off, pix_stride, frame_stride, B, H, W, tables, n, elem, dev):
    """fpc_gt_build into buffers with one canary row behind row n-1 / one canary word behind the last pixel."""
    from fastposecnn_amd import _native as nat
    row_of, class_of, first_row = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in tables)
    cm = torch.full((B * H * W + 1,), CANARY, dtype=torch.int64, device=dev)
    inst = torch.full((n + 1, H, W), CANARY, dtype=TORCH_OF[elem], device=dev)
    count = torch.full((n + 1,), CANARY, dtype=torch.int32, device=dev)
    nat.check(nat.lib().fpc_gt_build(ids_dev.data_ptr() + base_off, pix_stride, frame_stride, B, H, W, nat.ptr(row_of), nat.ptr(class_of),
                                     nat.ptr(first_row), n, nat.ptr(cm), nat.ptr(inst), elem, nat.ptr(count), nat.stream()),
              "fpc_gt_build")
    torch.cuda.synchronize()
    return cm.cpu().numpy(), inst.cpu().numpy(), count.cpu().numpy()


def _check_against_host(D, got, ids, pix_stride, tables, n, elem):
    cm, inst, count = got
    B, H, W = ids.shape[:3]
    w_cm, w_inst, w_count = D.build_gt_host(ids, pix_stride, *tables, n, NUMPY_OF[elem])
    assert np.array_equal(cm[:-1].reshape(B, H, W), w_cm) and cm[-1] == CANARY
    assert inst.dtype == w_inst.dtype and np.array_equal(inst[:n], w_inst) and (inst[n] == CANARY).all()
    assert np.array_equal(count[:n], w_count) and count[n] == CANARY


@pytest.mark.parametrize("layout", C.LAYOUTS)
@pytest.mark.parametrize("pix_stride", [1, 4])
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_equals_build_gt_host_on_adversarial_planes(D, dev, shape, pix_stride, layout):
    H, W = shape
    ids, row_of, class_of, first_row, n = C.adversarial(H, W, layout, pix_stride, seed=H * 1000 + W)
    B = ids.shape[0]
    assert n == {"one_frame_40_rows": 40, "one_frame_one_instance": 1, "three_frames": 41}[layout]
    ids_dev = torch.from_numpy(ids).to(dev)
    for elem in (8, 4, 1):
        got = _run_kernel(ids_dev, 0, pix_stride, H * W * pix_stride, B, H, W, (row_of, class_of, first_row), n, elem, dev)
        _check_against_host(D, got, ids, pix_stride, (row_of, class_of, first_row), n, elem)


@pytest.mark.parametrize("pix_stride", [1, 2, 3, 4])
def test_kernel_on_unaligned_frames_and_every_stride(D, dev, pix_stride):
    """Frames that start 3 bytes into the allocation and lie 5 bytes apart: no frame base is 16-byte aligned, so every id is
    read by the byte path; strides 2 and 3 have no wide load at all."""
    H, W = 33, 65
    ids, row_of, class_of, first_row, n = C.adversarial(H, W, "three_frames", 1, seed=pix_stride)
    B, frame_stride = 3, H * W * pix_stride + 5
    raw = np.random.default_rng(pix_stride).integers(0, 256, 3 + B * frame_stride).astype(np.uint8)
    for b in range(B):
        raw[3 + b * frame_stride:3 + b * frame_stride + H * W * pix_stride:pix_stride] = ids[b].reshape(-1)
    raw_dev = torch.from_numpy(raw).to(dev)
    for elem in (8, 4, 1):
        got = _run_kernel(raw_dev, 3, pix_stride, frame_stride, B, H, W, (row_of, class_of, first_row), n, elem, dev)
        _check_against_host(D, got, ids, 1, (row_of, class_of, first_row), n, elem)


def test_optional_outputs_and_no_rows(D, dev):
    from fastposecnn_amd import _native as nat
    H, W = 17, 256
    ids, row_of, class_of, first_row, n = C.adversarial(H, W, "three_frames", 1, seed=5)
    w_cm, w_inst, w_count = D.build_gt_host(ids, 1, row_of, class_of, first_row, n, np.float32)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (ids, row_of, class_of, first_row)]
    L = nat.lib()

    def call(n_, cm, inst, count):
        nat.check(L.fpc_gt_build(nat.ptr(t[0]), 1, H * W, 3, H, W, nat.ptr(t[1]), nat.ptr(t[2]), nat.ptr(t[3]), n_, nat.ptr(cm),
                                 nat.ptr(inst), 4, nat.ptr(count), nat.stream()), "fpc_gt_build")
        torch.cuda.synchronize()

    count = torch.full((n,), CANARY, dtype=torch.int32, device=dev)
    call(n, None, None, count)                                        # counts alone
    assert np.array_equal(count.cpu().numpy(), w_count)
    inst = torch.full((n, H, W), CANARY, dtype=torch.float32, device=dev)
    call(n, None, inst, None)                                         # planes alone
    assert np.array_equal(inst.cpu().numpy(), w_inst)
    cm = torch.full((3, H, W), CANARY, dtype=torch.int64, device=dev)
    inst.fill_(CANARY)
    count.fill_(CANARY)
    call(0, cm, inst, count)                                          # n == 0 still writes the class mask, and nothing else
    assert np.array_equal(cm.cpu().numpy(), w_cm)
    assert (inst == CANARY).all() and (count == CANARY).all()
    inst.fill_(CANARY)
    call(40, None, inst, None)                                        # rows >= n stay: row 40 belongs to the third frame
    assert np.array_equal(inst[:40].cpu().numpy(), w_inst[:40]) and (inst[40] == CANARY).all()


def test_slot_reuse_leaves_nothing_of_the_previous_batch(D, dev, fixture_batch):
    ds, items, files, samples, _ = fixture_batch
    up = D.GroundTruthUploader(2, 48, 64, 4, device=dev, slots=1, max_instances=8)
    first = [C.synthetic_item([9, 3, 200, 254], [1, 2, 1, 2], 1), C.synthetic_item([1, 2, 3], [2, 2, 1], 2)]
    planes = np.random.default_rng(0).integers(0, 256, (2, 48, 64, 4)).astype(np.uint8)
    planes[0, ..., 0] = np.asarray([9, 3, 200, 254])[np.arange(48 * 64) % 4].reshape(48, 64)      # no background pixel at all
    planes[1, ..., 0] = np.asarray([1, 2, 3])[np.arange(48 * 64) % 3].reshape(48, 64)
    got, ready = up.upload(planes, first)
    ready.synchronize()
    assert got["agg_data"]["class_ids"].shape[0] == 7 and bool((got["mask"] > 0).all())
    want, count = C.collate_gt_host(D, first, planes)
    assert np.array_equal(got["agg_data"]["instance_masks"].cpu().numpy(), want["agg_data"]["instance_masks"])
    assert np.array_equal(got["agg_data"]["RT"].cpu().numpy(), want["agg_data"]["RT"])
    assert np.array_equal(got["agg_data"]["pixel_counts"].cpu().numpy(), count)
    assert len(items[0]["ids"]) == 2
    got, ready = up.upload_png(files[:1], items[:1])                  # two rows, one frame: the same slot
    ready.synchronize()
    _same_batch(got, D.my_collate_fn(samples[:1], dev))
    assert got["mask"].shape[0] == 1 and got["agg_data"]["class_ids"].shape[0] == 2


def test_matching_is_the_same_from_every_ground_truth_source(D, dev, fixture_batch):
    import fastposecnn_amd.lib  # noqa: F401
    import matching as mg
    ds, items, files, samples, host = fixture_batch
    gts = [host["agg_data"]]
    for dtype in (torch.float64, torch.uint8):
        got, ready = D.GroundTruthUploader(2, 48, 64, 4, device=dev, max_instances=8, mask_dtype=dtype).upload_png(files, items)
        torch.cuda.current_stream().wait_event(ready)
        assert got["agg_data"]["instance_masks"].dtype == dtype
        _same_batch(got, host, skip=() if dtype == torch.float64 else ("instance_masks",))
        assert torch.equal(got["agg_data"]["instance_masks"].double(), host["agg_data"]["instance_masks"])
        gts.append(got["agg_data"])
    masks = host["agg_data"]["instance_masks"]
    preds = {k: v.float() for k, v in host["agg_data"].items() if k not in ("sample_ids", "class_ids", "instance_masks")}
    preds.update(class_ids=host["agg_data"]["class_ids"].long(), sample_ids=host["agg_data"]["sample_ids"],
                 instance_masks=torch.roll(masks, 1, dims=2).float())          # the fixture's own instances, one pixel to the right
    res = [mg.batchwise_find_matches_device(preds, g) for g in gts]
    n = masks.shape[0]
    assert int(res[0].count.item()) == n                               # every instance overlaps its own shifted copy
    for r in res[1:]:
        assert torch.equal(r.order, res[0].order) and torch.equal(r.match_pred, res[0].match_pred)
        assert torch.equal(r.count, res[0].count)


def test_check_raises_for_an_instance_without_pixels(D, dev):
    up = D.GroundTruthUploader(1, 5, 7, 1, device=dev, max_instances=4, mask_dtype=torch.uint8)
    item = C.synthetic_item([4, 9], [1, 2], 3)
    plane = np.full((1, 5, 7), 4, np.uint8)
    plane[0, 2, 3] = 9
    got, ready = up.upload(plane, [item])
    ready.synchronize()
    up.check(got)
    assert got["agg_data"]["pixel_counts"].tolist() == [34, 1]
    plane[0, 2, 3] = 0
    got, ready = up.upload(plane, [item])
    ready.synchronize()
    assert got["agg_data"]["pixel_counts"].tolist() == [34, 0] and not bool(got["agg_data"]["instance_masks"][1].any())
    with pytest.raises(ValueError):
        up.check(got)


def test_depth_decode_equals_standardize_depth(D, dev):
    from fastposecnn_amd import _native as nat
    r = np.random.default_rng(0)
    L = nat.lib()
    for src, kind, ch in ((r.integers(0, 256, (2, 5, 7, 3)).astype(np.uint8), 0, 3),
                          (r.integers(0, 256, (2, 5, 7, 4)).astype(np.uint8), 0, 4),
                          (r.integers(0, 65536, (2, 5, 7)).astype(np.uint16), 1, 1)):
        want = np.stack([D.standardize_depth(f[..., :3] if kind == 0 else f).astype("float32") for f in src])
        src_dev = torch.from_numpy(src.view(np.uint8)).to(dev)
        out = torch.full((2 * 5 * 7 + 1,), float(CANARY), dtype=torch.float32, device=dev)
        nat.check(L.fpc_depth_decode(nat.ptr(src_dev), kind, ch, 2, 5, 7, nat.ptr(out), nat.stream()), "fpc_depth_decode")
        got = out.cpu().numpy()
        assert np.array_equal(got[:-1].reshape(2, 5, 7), want) and got[-1] == CANARY


def test_uploader_with_depth_gives_the_collate_depth(D, dev, fixture_batch):
    ds, items, files, samples, host = fixture_batch
    depth_files = [open(it["mask_path"].replace("_mask.png", "_depth.png"), "rb").read() for it in items]
    up = D.GroundTruthUploader(2, 48, 64, 4, device=dev, max_instances=8, with_depth=True)
    got, ready = up.upload_png(files, items, depth_files=depth_files)
    ready.synchronize()
    assert got["depth"].dtype == torch.float32 and torch.equal(got["depth"], host["depth"])
    decoded = np.stack([D.imread_png(f) for f in depth_files])
    got, ready = up.upload(np.stack([D.imread_png(f) for f in files]), items, depth=decoded)
    ready.synchronize()
    assert torch.equal(got["depth"], host["depth"])
    _same_batch(got, host)
