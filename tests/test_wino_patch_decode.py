"""The workgroup-id decode of the four-wave Winograd kernels (csrc/wino_tile.hpp: wino_patch) takes every quotient by a multiply-shift
reciprocal the launcher computes (fpc_wino_recip, fpc_wino_decode; host only): n / d = (n * m) >> sh in 64 bits.  Here the model of
that decode is held against Python's // and % for every workgroup id of every geometry fpc_wino_pack_geometry and
fpc_wino_orient_geometry produce over H, W in 1 .. 200 step 7 and the headline's maps, B in {1, 2, 3, 5, 32}, Cout / 64 in
{1, 2, 4, 8}, groups in {1, 4}.  The decode is a chain — id -> (64-channel block, group, patch id) -> patch — so the two stages are
checked on their own domains: the first over every id below the largest grid of the whole range for each (Cout / 64, groups), the
second over every patch id of every geometry; the chain as a whole on the headline's maps.  The shift width is proven, not
assumed: for each divisor the reciprocal's error term is small enough for every n < 2^31 (the launchers' limit of ids)."""
import ctypes

import numpy as np
import pytest

BATCHES = (1, 2, 3, 5, 32)
NNB = (1, 2, 4, 8)
GROUPS = (1, 4)
HEADLINE = [(120, 160), (60, 80), (30, 40), (15, 20)]
SIZES = list(range(1, 201, 7))
CIN = 64


@pytest.fixture(scope="module")
def hiplib():
    from fastposecnn_amd import _native
    return _native.lib()


def cdiv(a, b):
    return -(-a // b)


def recip(L, d):
    out = (ctypes.c_int64 * 2)()
    assert L.fpc_wino_recip(d, out) == 0
    return int(out[0]), int(out[1])


def launch_recips(L, Cout, groups, tbx, tby, W, B, pack):
    out = (ctypes.c_int64 * 14)()
    assert L.fpc_wino_decode(Cout, groups, tbx, tby, W, B, pack, out) == 0
    return dict(zip(("nnb", "groups", "tbx", "tby", "per", "tbxl", "tcw"), [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(7)]))


def rdiv(n, r):
    """the kernel's wino_div on an array of ids: 64-bit product (n < 2^31, m < 2^32: no overflow), logical shift"""
    return (n.astype(np.uint64) * np.uint64(r[0])) >> np.uint64(r[1])


def geometries(L, H, W, B):
    """[(virtual W, tbx, tby, pack (0: the plain decode), patches)] of every launch form a site of this shape can take."""
    tcw, tch = cdiv(W, 2), cdiv(H, 2)
    out = [(W, cdiv(tcw, 8), cdiv(tch, 8), 0, cdiv(tcw, 8) * cdiv(tch, 8) * B)]
    q = (ctypes.c_int64 * 8)()
    assert L.fpc_wino_pack_geometry(H, W, B, CIN, 0, q) == 0
    if q[0] > 1:
        out.append((W, int(q[1]), int(q[2]), int(q[0]), int(q[3])))
    o = (ctypes.c_int64 * 9)()
    for fold in (0, 1):
        assert L.fpc_wino_orient_geometry(H, W, B, CIN, fold, 1, o) == 0
        if o[0] == 1:
            out.append((H, int(o[2]), int(o[3]), int(o[1]), int(o[4])))
    return out


def check_patch_stage(L, Wv, tbx, tby, pack, patches, B):
    """every patch id of one geometry: the reciprocal decode against // and % (the model of wino_patch's two branches)"""
    r = launch_recips(L, 64, 1, tbx, tby, Wv, B, pack)
    p = np.arange(patches, dtype=np.int64)
    tcw = cdiv(Wv, 2)
    if pack == 0:
        up = rdiv(p, r["tbx"]).astype(np.int64)
        bx = p - up * tbx
        b = rdiv(up, r["tby"]).astype(np.int64)
        by = up - b * tby
        assert np.array_equal(bx, p % tbx) and np.array_equal(by, (p // tbx) % tby) and np.array_equal(b, p // (tbx * tby))
        assert b.max() == B - 1
        return
    per = tbx * tby
    g = rdiv(p, r["per"]).astype(np.int64)
    assert np.array_equal(g, p // per)
    rem = p - g * per
    nf = np.minimum(pack, B - g * pack)
    tbxg = np.minimum(tbx, (nf * tcw + 7) // 8)
    last = cdiv((B % pack) * tcw, 8)
    assert set(np.unique(tbxg)) <= {tbx, last}, "a canvas row that is neither full nor the ragged last one"
    by = np.where(tbxg == tbx, rdiv(rem, r["tbx"]), rdiv(rem, r["tbxl"])).astype(np.int64)
    assert np.array_equal(by, rem // tbxg)
    bx = rem - by * tbxg
    assert np.array_equal(bx, rem % tbxg) and by.max() < tby
    f = rdiv(8 * bx, r["tcw"]).astype(np.int64)
    assert np.array_equal(f, (8 * bx) // tcw)
    assert (g * pack + f).max() == B - 1


def test_patch_stage_of_every_geometry(hiplib):
    n, largest = 0, 0
    for H, W in [(h, w) for h in SIZES for w in SIZES] + HEADLINE:
        for B in BATCHES:
            for Wv, tbx, tby, pack, patches in geometries(hiplib, H, W, B):
                check_patch_stage(hiplib, Wv, tbx, tby, pack, patches, B)
                n += 1
                largest = max(largest, patches)
    print(n, "geometries; the largest has", largest, "patches")
    assert largest * max(NNB) * max(GROUPS) < 2 ** 31


def test_block_and_group_stage_over_the_largest_grid(hiplib):
    largest = max(q[4] for H, W in [(SIZES[-1], SIZES[-1])] + HEADLINE for q in geometries(hiplib, H, W, 32))
    for nnb in NNB:
        for groups in GROUPS:
            r = launch_recips(hiplib, 64 * nnb, groups, 1, 1, 2, 1, 0)
            ids = np.arange(largest * nnb * groups, dtype=np.int64)
            up = rdiv(ids, r["nnb"]).astype(np.int64)
            assert np.array_equal(up, ids // nnb)
            assert np.array_equal(rdiv(up, r["groups"]).astype(np.int64), up // groups)


def test_whole_chain_on_the_headline_maps(hiplib):
    """id -> (block, group, patch id) -> patch, every id, Cout 128 and four groups: 19 200 workgroups on the 120 x 160 map at B = 32"""
    grids = []
    for H, W in HEADLINE:
        for Wv, tbx, tby, pack, patches in geometries(hiplib, H, W, 32):
            nnb, groups = 2, 4
            r = launch_recips(hiplib, 64 * nnb, groups, tbx, tby, Wv, 32, pack)
            ids = np.arange(patches * nnb * groups, dtype=np.int64)
            grids.append(len(ids))
            up = rdiv(ids, r["nnb"]).astype(np.int64)
            nb = ids - up * nnb
            p = rdiv(up, r["groups"]).astype(np.int64)
            grp = up - p * groups
            assert np.array_equal(nb, ids % nnb) and np.array_equal(grp, (ids // nnb) % groups) and np.array_equal(p, ids // (nnb * groups))
            assert p.max() == patches - 1
    assert 19200 in grids, grids


def test_shift_width_is_proven_for_every_id_below_2_31(hiplib):
    """m d = 2^sh + e with 0 <= e < d: n m / 2^sh = n / d + n e / (d 2^sh), and n e < 2^sh keeps the floor.  Checked as stated for
    every divisor that can occur and for awkward ones, and by evaluation at the ids where a wrong reciprocal fails first: the
    multiples of d and their predecessors at the top of the range, and 2^31 - 1 itself."""
    top = 2 ** 31 - 1
    divisors = set(range(1, 400)) | {19200, 19201, 2 ** 16 - 1, 2 ** 16, 2 ** 16 + 1, 2 ** 30 - 1, 2 ** 30 + 1, top - 1, top, 2 ** 31,
                                     3 * 5 * 7 * 11 * 13 * 17, 641, 6700417, 715827883}
    for d in sorted(divisors):
        m, sh = recip(hiplib, d)
        assert 0 < m < 2 ** 32 and 31 <= sh <= 62 and 2 ** (sh - 31) >= d > 2 ** (sh - 32)
        e = m * d - 2 ** sh
        assert 0 <= e < d and e * top < 2 ** sh, (d, m, sh)
        k = top // d
        for n in {0, 1, d - 1, d, d + 1, k * d - 1, k * d, k * d + d - 1, top, top - 1, top // 2, (top // 2 // d) * d - 1}:
            if 0 <= n <= top:
                assert (n * m) >> sh == n // d, (n, d)
    out = (ctypes.c_int64 * 2)()
    assert hiplib.fpc_wino_recip(0, out) == -1 and hiplib.fpc_wino_recip(2 ** 31 + 1, out) == -1 and hiplib.fpc_wino_recip(3, None) == -1
    assert hiplib.fpc_wino_decode(64, 1, 0, 1, 8, 1, 0, (ctypes.c_int64 * 14)()) == -1
