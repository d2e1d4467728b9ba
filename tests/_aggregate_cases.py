"""Hand-built label planes for the aggregation kernels (csrc/aggregate.hip): inputs of fpc_aggregate_bits that no
segmentation would produce, at the smallest shapes that still reach every edge of the kernels' geometry.

The accumulation walks 64-pixel-wide, 8-row strips, four of them (a 64 x 32 tile) per workgroup, and combines at most four
instances per workgroup in LDS; the planes are written in 4096-pixel chunks, four pixels per lane (one by one when H W is
no multiple of 4).  The families below put many instances under one workgroup (cells), many labels inside one 64-pixel row
(columns, checker, every-pixel), a new label on every row (rows), every workgroup and chunk on one instance (almost-all)
and single pixels on both sides of every tile / strip / chunk boundary (seams).

fpc_aggregate_bits only needs a partition, so instances are not connected components here.  What it does require holds for
every case (check_contract): labels 1..n all occur, the labels of an image are a contiguous range that ascends with the image
index, and no instance covers a whole image.

Everything is built on the host from a seed derived from the case's name: the same arrays on every machine and every run.
"""
import functools
import zlib

import numpy as np

# ----------------------------------------------------------------------------- label families: local ids, 0 = background


def empty(H, W):
    return np.zeros((H, W), np.int64)


def cells(H, W, c, skip=0):
    """A lattice of c x c cells, each its own instance; every `skip`-th cell is left as background."""
    y, x = np.mgrid[0:H, 0:W]
    idx = (y // c) * ((W + c - 1) // c) + x // c
    out = idx + 1
    if skip:
        out[idx % skip == skip - 1] = 0
    return out


def cells_all_but_one_pixel(H, W, c):
    """Every cell labelled; one pixel inside a cell is background."""
    out = cells(H, W, c)
    out[H // 2 + 1, W // 2 + 1] = 0
    return out


def columns(H, W):
    """Column x is instance x: 64 labels in every 64-pixel row.  A diagonal of background pixels in every fifth column."""
    y, x = np.mgrid[0:H, 0:W]
    out = x + 1
    out[(x % 5 == 0) & (y == x % H)] = 0
    return out


def rows(H, W, k=1):
    """k image rows per instance: the wave's label changes every k rows.  Background pixels on every fourth row."""
    y, x = np.mgrid[0:H, 0:W]
    out = y // k + 1
    out[(y % 4 == 0) & (x == (3 * y) % W)] = 0
    return out


def checker(H, W):
    """Two instances alternating pixel by pixel; one background pixel."""
    y, x = np.mgrid[0:H, 0:W]
    out = 1 + (x + y) % 2
    out[H // 2, W // 2] = 0
    return out


def almost_all(H, W):
    """One instance over every pixel but one."""
    out = np.ones((H, W), np.int64)
    out[H // 2, W // 3] = 0
    return out


def seam_pixels(H, W):
    """The pixels the seams family occupies: corners, both sides of the tile column seam (x = 63 | 64), of a strip seam
    (y = 7 | 8), of a tile row seam (y = 31 | 32) and of the 1024- and 4096-pixel seams of the plane kernels."""
    want = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1),
            (3, 63), (3, 64), (20, 63), (20, 64),
            (7, 5), (8, 5), (7, 66), (8, 66),
            (31, 40), (32, 40), (31, 70), (32, 70)]
    want += [divmod(p, W) for p in (1023, 1024, 4095, 4096)]
    pix = sorted({(y, x) for y, x in want if 0 <= y < H and 0 <= x < W})
    return pix


def seams(H, W):
    out = np.zeros((H, W), np.int64)
    for k, (y, x) in enumerate(seam_pixels(H, W)):
        out[y, x] = k + 1
    return out


def every_pixel(H, W):
    return np.arange(1, H * W + 1, dtype=np.int64).reshape(H, W)


def tiny_a(H, W):
    assert (H, W) == (3, 5)
    return np.array([[1, 1, 0, 2, 2], [1, 3, 3, 3, 2], [0, 4, 4, 5, 5]], np.int64)


def tiny_b(H, W):
    assert (H, W) == (3, 5)
    return np.array([[1, 2, 3, 4, 5], [1, 2, 0, 4, 5], [1, 2, 3, 4, 0]], np.int64)


# ----------------------------------------------------------------------------- the cases: name -> (H, W, one family per image)

CASES = {
    # 40 x 72: a partial second tile column, a partial tile row, one partial chunk, H W % 4 == 0
    "cells8-40x72-B3": (40, 72, [lambda H, W: cells(H, W, 8, 7), empty, lambda H, W: cells(H, W, 8, 5)]),
    "columns-40x72-B3": (40, 72, [columns, columns, empty]),
    "rows2-40x72-B3": (40, 72, [lambda H, W: rows(H, W, 2), empty, rows]),
    "mixed-40x72-B5": (40, 72, [seams, columns, empty, almost_all, rows]),
    # 67 x 93: H W odd (scalar plane path, images off 16-byte alignment), two chunks with the second partial
    "cells8-67x93-B5": (67, 93, [empty, lambda H, W: cells(H, W, 8, 6), empty, lambda H, W: cells(H, W, 8, 11),
                                 lambda H, W: cells(H, W, 8, 3)]),
    "rows-67x93-B1": (67, 93, [rows]),
    "checker-67x93-B3": (67, 93, [checker, empty, checker]),
    "almost-67x93-B1": (67, 93, [almost_all]),
    "seams-67x93-B3": (67, 93, [seams, empty, seams]),
    # 64 x 128: exactly two full chunks, tiles aligned
    "cells4-64x128-B1": (64, 128, [lambda H, W: cells_all_but_one_pixel(H, W, 4)]),       # 512 instances
    "columns-64x128-B1": (64, 128, [columns]),
    "checker-64x128-B1": (64, 128, [checker]),
    "almost-64x128-B3": (64, 128, [almost_all, empty, almost_all]),
    "seams-64x128-B1": (64, 128, [seams]),
    # every pixel its own instance: 384 of them, the one family without a background pixel
    "everypixel-16x24-B1": (16, 24, [every_pixel]),
    # 3 x 5: smaller than a strip
    "tiny-3x5-B1": (3, 5, [tiny_a]),
    "tiny-3x5-B5": (3, 5, [empty, tiny_a, empty, tiny_b, empty]),
}

NAMES = tuple(CASES)


def number_labels(planes):
    """Local-id planes (one per image) -> labels i32 [B,H,W] numbered 1..n image by image, inside an image in raster order of
    each instance's first pixel (the order a connected-component labelling gives), and n."""
    out, n = [], 0
    for pl in planes:
        ids, first = np.unique(pl.ravel(), return_index=True)
        keep = ids != 0
        ids, first = ids[keep], first[keep]
        lut = np.zeros(int(pl.max()) + 1, np.int64)
        lut[ids[np.argsort(first, kind="stable")]] = n + 1 + np.arange(ids.size)
        out.append(lut[pl])
        n += ids.size
    return np.stack(out).astype(np.int32), n


def root_pixels(labels, n):
    """The raster-first pixel of labels 1..n as a linear index over B*H*W (what fpc_cc_label's root_pix holds)."""
    ids, first = np.unique(labels.ravel(), return_index=True)
    root = np.full(n + 1, -1, np.int64)
    root[ids] = first
    assert (root[1:] >= 0).all()
    return root[1:].astype(np.int32)


def check_contract(case):
    """What fpc_aggregate_bits (and the oracle) require of a label plane."""
    labels, n = case["labels"], case["n"]
    B, H, W = labels.shape
    assert labels.dtype == np.int32 and labels.min() >= 0 and labels.max() == n
    assert np.array_equal(np.unique(labels[labels > 0]), np.arange(1, n + 1)), "labels 1..n all occur"
    nxt = 1
    for b in range(B):
        ids = np.unique(labels[b][labels[b] > 0])
        if ids.size == 0:
            continue
        assert ids[0] == nxt and ids[-1] - ids[0] + 1 == ids.size, "an image's labels are a contiguous, ascending range"
        nxt = int(ids[-1]) + 1
        assert np.bincount(labels[b].ravel()).max() < H * W, "no instance covers a whole image"
    assert nxt == n + 1
    root = case["root_pix"]
    assert root.shape == (n,) and np.array_equal(labels.ravel()[root], np.arange(1, n + 1))


@functools.lru_cache(maxsize=None)
def make(name):
    """The inputs of case `name`: dict of labels i32 [B,H,W], cat_mask i64 [B,H,W], quat f32 [B,4,H,W], scales f32 [B,3,H,W],
    xy f32 [B,2,H,W], z f32 [B,H,W], n, root_pix i32 [n], and which instances carry the special values.  Shared by every
    test of the session: read-only."""
    H, W, fams = CASES[name]
    B = len(fams)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    labels, n = number_labels([f(H, W) for f in fams])
    lab = labels.astype(np.int64)
    fg = lab > 0
    inst = lab - 1                                                  # -1 on the background

    # quaternion: one unit vector per instance + uniform noise of amplitude 0.2 (the mean's norm stays near 1); the
    # background carries values as large, which must not reach any instance
    u = rng.normal(size=(n, 4))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    quat = rng.normal(size=(B, 4, H, W))
    noise = rng.uniform(-0.2, 0.2, size=(B, 4, H, W))
    for a in range(4):
        quat[:, a][fg] = u[inst[fg], a] + noise[:, a][fg]
    scales = rng.uniform(0.5, 2.0, size=(B, 3, H, W))
    z = rng.normal(6.0, 0.2, size=(B, H, W))
    xy = rng.normal(size=(B, 2, H, W))

    # classes: instance k is of class 1 + k % 6; every third one mixes in a second class and class-0 pixels
    k = np.arange(n)
    base = 1 + k % 6
    other = 1 + (k + 2) % 6
    cat = np.zeros((B, H, W), np.int64)
    cat[fg] = base[inst[fg]]
    pick = rng.integers(0, 3, size=(B, H, W))
    mixed = fg & (k % 3 == 1)[np.maximum(inst, 0)]
    cat[mixed & (pick == 1)] = other[inst[mixed & (pick == 1)]]
    cat[mixed & (pick == 2)] = 0
    special = {"class_1000": None, "class_0": None, "zero_quat": None}
    if n >= 2:
        # class id 1000, some of its pixels of class 0 (never the first one)
        m = lab == 1
        cat[m] = np.where(pick[m] == 2, 0, 1000)
        cat.reshape(-1)[root_pixels(labels, n)[0]] = 1000
        special["class_1000"] = 0
        # an all-zero quaternion: the nq == 0 branch
        zq = n // 2
        quat[np.broadcast_to((lab == zq + 1)[:, None], quat.shape)] = 0.0
        special["zero_quat"] = zq
    if n >= 3:
        cat[lab == n] = 0                                           # every pixel of class 0: class id 0
        special["class_0"] = n - 1

    case = {
        "name": name, "B": B, "H": H, "W": W, "n": n,
        "labels": labels, "cat_mask": cat,
        "quat": quat.astype(np.float32), "scales": scales.astype(np.float32),
        "xy": xy.astype(np.float32), "z": z.astype(np.float32),
        "root_pix": root_pixels(labels, n), "special": special,
    }
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


# ----------------------------------------------------------------------------- the scene of the Python-layer test

def lattice_scene():
    """One 64 x 128 image for AggregationLayer: 300 isolated single-pixel components on a lattice plus two blobs, i.e. 302
    connected components — more than the 256 root pixels the layer keeps for one image.  Returns a categorical dict of
    numpy arrays (mask i64 [1,H,W], quaternion, scales, xy, z)."""
    H, W = 64, 128
    rng = np.random.default_rng(302)
    m = np.zeros((1, H, W), np.int64)
    ys, xs = np.meshgrid(np.arange(1, 31, 3), np.arange(1, 121, 4), indexing="ij")       # 10 x 30, no two 4-connected
    m[0, ys, xs] = rng.integers(1, 7, size=ys.shape)
    m[0, 40:60, 10:40] = 3
    m[0, 36:62, 70:110] = 5
    m[0, 45:50, 80:90] = 2                                          # a second class inside the blob: same component
    u = rng.normal(size=(4, 1, 1))
    u /= np.linalg.norm(u)
    return {
        "mask": m,
        "quaternion": (u + rng.uniform(-0.2, 0.2, size=(1, 4, H, W))).astype(np.float32),
        "scales": rng.uniform(0.5, 2.0, size=(1, 3, H, W)).astype(np.float32),
        "xy": rng.normal(size=(1, 2, H, W)).astype(np.float32),
        "z": rng.normal(6.0, 0.2, size=(1, H, W)).astype(np.float32),
    }
