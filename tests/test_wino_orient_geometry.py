"""Orientation of the form-9 Winograd launch (fpc_wino_orient_geometry, host only).

A site whose tile columns fill whole 8-column patches while its tile rows do not runs TRANSPOSED: the kernel sees the virtual image
H' = W, W' = H (its pixel (y, x) is the stored pixel (x, y)), so the ragged direction lies along the patch's x axis, where frames
pack side by side (tests/test_wino_pack_geometry.py).  The model of that file (slot decode, seam arithmetic, fragment addressing,
GroupNorm records) runs here on the virtual image the library reports; on top of it: the virtual tiles are exactly the stored
image's tiles, the records fit the reservation cdiv(H W, 128) * 4 the plan makes per
frame, and the rule depends on the shape alone."""
import ctypes

import pytest

from test_wino_pack_geometry import cdiv, walk

CIN = 128
KEYS = ("G", "tbx", "tby", "patches", "slots", "tiles", "gn_rows", "rx")


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import _native
    return _native.lib()


def _orient(L, H, W, B, cin=CIN, fold=0, pack=1):
    out = (ctypes.c_int64 * 9)()
    assert L.fpc_wino_orient_geometry(H, W, B, cin, fold, pack, out) == 0
    return int(out[0]), dict(zip(KEYS, list(out)[1:]))


def _plain(L, H, W, B, cin=CIN, fold=0):
    out = (ctypes.c_int64 * 8)()
    assert L.fpc_wino_pack_geometry(H, W, B, cin, fold, out) == 0
    return dict(zip(KEYS, out))


def rule(H, W):
    tcw, tch = cdiv(W, 2), cdiv(H, 2)
    return tcw % 8 == 0 and tch % 8 != 0 and tch >= 8


# H, W, B: the headline's wide maps, ragged batches, a single frame, the smallest maps the rule transposes (even and odd sizes)
CASES = [(120, 160, 32), (60, 80, 32), (60, 80, 3), (60, 80, 5), (120, 160, 1), (24, 32, 2), (24, 32, 3), (24, 32, 5), (23, 31, 2),
         (23, 31, 3), (23, 31, 5), (24, 32, 1)]


@pytest.mark.parametrize("H,W,B", CASES)
def test_transposed_launch_owns_every_tile_once(hiplib, H, W, B):
    tr, q = _orient(hiplib, H, W, B)
    assert tr == 1 and rule(H, W)
    Hv, Wv = W, H                                    # the virtual image
    assert q == _plain(hiplib, Hv, Wv, B)            # wino_pack_geometry on the swapped sizes, as it stands
    nwg, written, records = walk(Hv, Wv, B, q)       # every fragment read sees its (virtual) pixel or an unstaged unit
    assert nwg == q["patches"] and q["slots"] == 64 * nwg
    tch, tcw = cdiv(H, 2), cdiv(W, 2)
    # virtual tile (row, column) = stored tile (column, row): every stored tile of every frame has one owner
    stored = sorted((b, tx, ty) for (b, ty, tx) in written)
    assert stored == [(b, ty, tx) for b in range(B) for ty in range(tch) for tx in range(tcw)]
    assert q["tiles"] == B * tch * tcw
    # every GroupNorm record k_gn_finalize reads has one writer, and they lie inside the plan's reservation, which does not grow
    assert sorted(records) == [(b, r) for b in range(B) for r in range(q["gn_rows"])]
    assert q["gn_rows"] == q["tby"] * q["rx"] <= cdiv(H * W, 128) * 4
    # never more patches than the plain launch
    assert q["patches"] <= _plain(hiplib, H, W, B)["patches"]


def test_patch_counts_at_the_headline_configuration(hiplib):
    tr, big = _orient(hiplib, 120, 160, 32)
    assert tr and (big["G"], big["tbx"], big["tby"], big["patches"]) == (2, 15, 10, 2400)      # 2 560 plain
    tr, mid = _orient(hiplib, 60, 80, 32)
    assert tr and (mid["G"], mid["tbx"], mid["tby"], mid["patches"]) == (4, 15, 5, 600)        # 640 plain
    assert big["tiles"] == big["slots"] and mid["tiles"] == mid["slots"]                       # slot use 100 %
    assert big["gn_rows"] == 80 and mid["gn_rows"] == 25
    assert _plain(hiplib, 120, 160, 32)["patches"] == 2560 and _plain(hiplib, 60, 80, 32)["patches"] == 640
    # the fold packs too when it runs transposed, and fpc_net_set_wino_pack does not govern a transposed site
    assert _orient(hiplib, 120, 160, 32, fold=1) == (1, big) and _orient(hiplib, 120, 160, 32, pack=0) == (1, big)
    # a single frame: the plain launch's patch count
    assert _orient(hiplib, 120, 160, 1)[1]["patches"] == 80 and _orient(hiplib, 60, 80, 1)[1]["patches"] == 20


@pytest.mark.parametrize("H,W", [(30, 40), (15, 20), (9, 17), (96, 128), (12, 32), (160, 120)])
def test_rule_leaves_the_other_shapes_alone(hiplib, H, W):
    """Tile columns and rows both multiples of 8, or the columns not: today's orientation and today's packing.  (12 x 32: fewer than
    8 tile rows, nothing could pack along them.)"""
    assert not rule(H, W)
    for fold in (0, 1):
        assert _orient(hiplib, H, W, 32, fold=fold, pack=1) == (0, _plain(hiplib, H, W, 32, fold=fold))
        tr, q = _orient(hiplib, H, W, 32, fold=fold, pack=0)
        assert tr == 0 and q["G"] == 1 and q["patches"] == 32 * cdiv(cdiv(W, 2), 8) * cdiv(cdiv(H, 2), 8)


def test_rule_does_not_depend_on_the_batch(hiplib):
    for H in range(1, 70, 3):
        for W in range(2, 100, 5):
            got = {_orient(hiplib, H, W, B)[0] for B in (1, 2, 3, 5, 8, 32)}
            assert got == {int(rule(H, W))}, (H, W)


def test_bad_arguments(hiplib):
    out = (ctypes.c_int64 * 9)()
    assert hiplib.fpc_wino_orient_geometry(0, 32, 4, 64, 0, 1, out) == -1
    assert hiplib.fpc_wino_orient_geometry(24, 32, 0, 64, 0, 1, out) == -1
    assert hiplib.fpc_wino_orient_geometry(24, 32, 4, 64, 0, 1, None) == -1
