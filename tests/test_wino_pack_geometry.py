"""Patch geometry of the packed form-9 Winograd launch (fpc_wino_pack_geometry, host only).

G frames of a small map lie side by side on a canvas row and the 8 x 8 tile patches are cut out of the canvas; a patch that meets a
frame's end after ks < 8 tile columns carries a seam, and its staged region one gap column.  The model below repeats the kernel's
slot decode, its seam arithmetic and its fragment addressing (csrc/wino_tile.hpp: wino_patch, wino_stage_plan, wino_frag) on the geometry the library reports and checks
that every fragment read sees the pixel it should (or an unstaged unit, which reads zero), that every tile of every frame is owned
by exactly one (patch, slot), and that every GroupNorm record k_gn_finalize reads is written exactly once."""
import ctypes

import pytest

CIN = 128


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import _native
    return _native.lib()


def cdiv(a, b):
    return -(-a // b)


def _geom(L, H, W, B, cin=CIN, fold=0):
    out = (ctypes.c_int64 * 8)()
    assert L.fpc_wino_pack_geometry(H, W, B, cin, fold, out) == 0
    return dict(zip(("G", "tbx", "tby", "patches", "slots", "tiles", "gn_rows", "rx"), out))


def slot_decode(slot):
    """LDS-DMA slot (piece * 64 + lane) -> (ah, qh, region row, region column, channel half)"""
    blk, res = slot >> 4, slot & 15
    cell = blk >> 3
    ah, qh = (cell // 3) * 4 + (res & 3), (cell % 3) * 4 + (res >> 2)
    return ah, qh, 2 * ah + ((blk >> 2) & 1), 2 * qh + ((blk >> 1) & 1), blk & 1


def unit(ah, qh, rbit, cbit, lh):
    """16-byte unit a fragment read of region row 2 ah + rbit, column 2 qh + cbit, channel half lh takes"""
    return (((ah >> 2) * 3 + (qh >> 2)) * 8 + rbit * 4 + cbit * 2 + lh) * 16 + 4 * (qh & 3) + (ah & 3)


def best_group(tcw, B):
    G = 1
    for g in range(2, min(B, 8) + 1):
        if cdiv(g * tcw, 8) * G < cdiv(G * tcw, 8) * g:
            G = g
    return G


def walk(H, W, B, q):
    """Runs the model over every launched patch; returns (patches, tiles written, GroupNorm records written per frame)."""
    tcw, tch, G, tbx, tby, rx = cdiv(W, 2), cdiv(H, 2), q["G"], q["tbx"], q["tby"], q["rx"]
    assert tby == cdiv(tch, 8) and tbx == cdiv(G * tcw, 8)
    assert G == 1 or tcw >= 8
    written, records, nwg = {}, {}, 0
    for grp in range(cdiv(B, G)):
        nf = min(G, B - grp * G)
        tbxg = min(tbx, cdiv(nf * tcw, 8))          # a ragged last group launches only the patches that reach its frames
        for by in range(tby):
            for bx in range(tbxg):
                nwg += 1
                c0 = 8 * bx
                f, tx0 = c0 // tcw, c0 % tcw
                raw = tcw - tx0
                ks = raw if (raw < 8 and G > 1) else 99
                two = ks < 8 and f + 1 < nf
                if G == 1:
                    assert f == 0
                # staging
                lds = {}
                for slot in range(18 * 64):
                    ah, qh, ry, rx_, hf = slot_decode(slot)
                    if ah > 8 or qh > (9 if ks < 8 else 8):
                        continue
                    y = 2 * 8 * by - 1 + ry
                    far = qh > ks
                    x = rx_ - 2 * ks - 3 if far else 2 * tx0 - 1 + rx_
                    if (far and not two) or y < 0 or y >= H or x < 0 or x >= W:
                        continue
                    assert slot not in lds
                    lds[slot] = (grp * G + f + far, y, x, hf)
                # fragment reads and tile ownership
                for k in range(8):
                    far = k >= ks
                    qb = k + far
                    fr, ltx = (f + 1, k - ks) if far else (f, tx0 + k)
                    for tr in range(8):
                        lty = 8 * by + tr
                        valid = fr < nf and lty < tch and ltx < tcw
                        if not valid:
                            continue
                        for r in range(4):
                            for c in range(4):
                                for lh in range(2):
                                    u = unit(tr + (r >> 1), qb + (c >> 1), r & 1, c & 1, lh)
                                    assert u < 18 * 64
                                    y, x = 2 * lty - 1 + r, 2 * ltx - 1 + c
                                    want = (grp * G + fr, y, x, lh) if (0 <= y < H and 0 <= x < W) else None
                                    assert lds.get(u) == want, (H, W, G, bx, k, tr, r, c, lds.get(u), want)
                        key = (grp * G + fr, lty, ltx)
                        assert key not in written
                        written[key] = (grp, by, bx, k, tr)
                # GroupNorm records: frame f at its own slot, the frame behind the seam at slot 0; the patch with a frame's last tile
                # column zeroes the slots that frame does not use
                if G > 1:
                    slot0 = bx - (f * tcw) // 8
                    recs = [(grp * G + f, by * rx + slot0)]
                    if two:
                        recs.append((grp * G + f + 1, by * rx))
                    if raw <= 8:
                        recs += [(grp * G + f, by * rx + z) for z in range(slot0 + 1, rx)]
                else:
                    recs = [(grp, by * tbx + bx)]
                for rec in recs:
                    assert rec not in records
                    records[rec] = 1
    return nwg, written, records


CASES = [(15, 20, 32), (30, 40, 32), (30, 40, 5), (15, 20, 7), (9, 17, 4), (60, 80, 32), (120, 160, 32), (15, 20, 1)]


@pytest.mark.parametrize("H,W,B", CASES)
def test_every_tile_once_and_every_read_sees_its_pixel(hiplib, H, W, B):
    q = _geom(hiplib, H, W, B)
    tcw, tch = cdiv(W, 2), cdiv(H, 2)
    assert q["G"] == best_group(tcw, B)
    nwg, written, records = walk(H, W, B, q)
    assert nwg == q["patches"]
    assert q["slots"] == 64 * q["patches"]
    assert len(written) == B * tch * tcw == q["tiles"]
    # every record of every frame, and nothing else
    assert sorted(records) == [(b, r) for b in range(B) for r in range(q["gn_rows"])]
    assert q["gn_rows"] == q["tby"] * q["rx"]


def test_patch_counts_at_the_headline_configuration(hiplib):
    small5, small4 = _geom(hiplib, 15, 20, 32, 512), _geom(hiplib, 30, 40, 32, 256)
    assert (small5["G"], small5["patches"]) == (4, 40)          # 64 plain: grid 512 -> 320 at 8 channel blocks
    assert (small4["G"], small4["patches"]) == (2, 160)         # 192 plain: grids 768 -> 640, 1 536 -> 1 280
    assert small5["tiles"] / small5["slots"] >= 0.93 and small4["tiles"] / small4["slots"] >= 0.93
    assert small5["tiles"] == small5["slots"]
    assert small4["tiles"] / small4["slots"] == 0.9375           # the rest is the vertical loss: 15 tile rows in two patches
    for H, W in ((60, 80), (120, 160)):
        q = _geom(hiplib, H, W, 32, 128)
        assert q["G"] == 1 and q["patches"] == cdiv(cdiv(W, 2), 8) * cdiv(cdiv(H, 2), 8) * 32
        assert q["gn_rows"] == q["tbx"] * q["tby"]


def test_ineligible_shapes_stay_on_one_frame_per_patch_row(hiplib):
    assert _geom(hiplib, 15, 20, 1)["G"] == 1                     # one frame: nothing to pack
    assert _geom(hiplib, 12, 14, 32)["G"] == 1                    # 7 tile columns: a patch could straddle three frames
    assert _geom(hiplib, 12, 10, 32)["G"] == 1
    assert _geom(hiplib, 15, 20, 32, fold=1)["G"] == 1            # the folded s2.0 never packs
    assert _geom(hiplib, 15, 20, 32, fold=0)["G"] == 4
    # two frames of the input beyond 32-bit byte offsets
    assert _geom(hiplib, 1500, 2004, 4, cin=16)["G"] == 4
    assert _geom(hiplib, 1500, 2004, 4, cin=192)["G"] == 1
    plain = _geom(hiplib, 12, 14, 32)
    assert plain["patches"] == 32 and plain["gn_rows"] == 1 and plain["rx"] == 1


def test_bad_arguments(hiplib):
    out = (ctypes.c_int64 * 8)()
    assert hiplib.fpc_wino_pack_geometry(0, 20, 4, 64, 0, out) == -1
    assert hiplib.fpc_wino_pack_geometry(15, 20, 0, 64, 0, out) == -1
    assert hiplib.fpc_wino_pack_geometry(15, 20, 4, 64, 0, None) == -1
