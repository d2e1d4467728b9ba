"""Shared inputs of test_gt_builder_host.py and test_gpu_gt_builder.py: the NOCS fixture as the ground-truth uploader sees it,
and adversarial id planes with their tables for fpc_gt_build."""
import os
import pathlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = pathlib.Path(HERE) / "golden" / "nocs"
GOLD = os.path.join(HERE, "golden", "nocs_sample.npz")

SHAPES = [(1, 1), (5, 7), (33, 65), (48, 64), (17, 256)]     # one pixel; below one load; odd and one partial chunk;
                                                             # a multiple of 16; more than one chunk (4096 + 256 pixels)
LAYOUTS = ["one_frame_40_rows", "one_frame_one_instance", "three_frames"]


def gold_classes():
    return [str(c) for c in np.load(GOLD, allow_pickle=False)["classes"]]


def dataset(scene="scene_a", classes=None, preprocessing=True):
    from fastposecnn_amd.tools import dataset as D
    pre = D.get_preprocessing(D.get_preprocessing_fn("resnet18", "imagenet")) if preprocessing else None
    return D.CAMERADataset(ROOT / scene, classes=classes or gold_classes(), preprocessing=pre)


def mask_bytes(item):
    return open(item["mask_path"], "rb").read()


def collate_gt_host(D, items, ids_u8, mask_dtype=np.float64):
    """gt_item dicts + id planes as decoded -> what my_collate_fn returns for 'mask' and 'agg_data', through build_gt_host."""
    row_of, class_of, first_row, n = D.gt_tables(items)
    pix_stride = ids_u8.shape[3] if ids_u8.ndim == 4 else 1
    class_mask, inst, count = D.build_gt_host(ids_u8, pix_stride, row_of, class_of, first_row, n, mask_dtype)
    agg = {"sample_ids": np.repeat(np.arange(len(items)), np.diff(first_row))}
    for key, _ in D.GT_TABLE_KEYS:
        agg[key] = np.concatenate([it["table"][key] for it in items], axis=0)
    agg["instance_masks"] = inst
    return {"mask": class_mask, "agg_data": agg}, count


def synthetic_item(ids, classes, seed):
    """A gt_item-like dict with random per-instance numbers (nothing here reads a file)."""
    from fastposecnn_amd.tools import dataset as D
    r = np.random.default_rng(seed)
    m = len(ids)
    table = {key: r.normal(size=(m,) + shape) for key, shape in D.GT_TABLE_KEYS}
    table["class_ids"] = np.asarray(classes, np.float64)
    table["z"] = np.abs(table["z"]) + 1.0
    return {"path": "synthetic-%d" % seed, "mask_path": None, "ids": list(ids), "class_values": list(classes), "valid": True,
            "table": table}


def adversarial(H, W, layout, pix_stride, seed):
    """-> (ids uint8 [B,H,W] or [B,H,W,4], row_of, class_of, first_row, n).
    The frame with 40 rows: rows handed out in a shuffled order of the ids; id 254 listed, ids 0 and 255 in the plane as
    background; five unlisted ids in the plane (row -1, class 0), one of them with a class but no row and one listed id with
    a row but class 0 (the two tables are independent); one listed id that has no pixel.  three_frames: that frame, a frame
    without rows (its plane full of ids the first frame lists), and a frame that is one single instance."""
    r = np.random.default_rng(seed)
    HW = H * W

    def many(first):
        row_of, class_of = np.full(256, -1, np.int16), np.zeros(256, np.uint8)
        perm = r.permutation(np.arange(1, 254))
        listed = np.concatenate([[254], perm[:39]])
        unlisted = perm[39:44]
        row_of[listed] = first + r.permutation(40)
        class_of[listed] = r.integers(1, 7, 40)
        class_of[listed[1]] = 0                           # a row without a class
        class_of[unlisted[0]] = 3                         # a class without a row
        palette = np.concatenate([listed[:-1], unlisted, [0, 255]])          # listed[-1] has no pixel
        plane = r.choice(palette, HW).astype(np.uint8)
        plane[:3] = [0, 254, 255][:min(3, HW)]
        return plane, row_of, class_of, 40

    def empty(first):
        return r.integers(0, 256, HW).astype(np.uint8), np.full(256, -1, np.int16), np.zeros(256, np.uint8), 0

    def single(first):
        row_of, class_of = np.full(256, -1, np.int16), np.zeros(256, np.uint8)
        row_of[254], class_of[254] = first, 5
        return np.full(HW, 254, np.uint8), row_of, class_of, 1

    frames = {"one_frame_40_rows": [many], "one_frame_one_instance": [single], "three_frames": [many, empty, single]}[layout]
    planes, rows, classes, first_row = [], [], [], [0]
    for make in frames:
        p, ro, co, m = make(first_row[-1])
        planes.append(p); rows.append(ro); classes.append(co); first_row.append(first_row[-1] + m)
    ids = np.stack(planes).reshape(len(frames), H, W)
    if pix_stride == 4:
        rgba = r.integers(0, 256, (len(frames), H, W, 4)).astype(np.uint8)
        rgba[..., 0] = ids
        ids = rgba
    return ids, np.stack(rows), np.stack(classes), np.asarray(first_row, np.int32), int(first_row[-1])
