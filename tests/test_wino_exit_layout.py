"""The exit of the four-wave Winograd kernels (csrc/wino_tile.hpp: wino_out_base, wino_out_step, wino_exit_fast; host only, through
fpc_wino_tile_out and fpc_wino_tile_patch — the very functions the kernels call).
  * A thread's 16 output offsets — one 64-bit base plus wave-uniform strides — equal ((ob H W + pixel) Cout + n) written out per quad,
    for every thread, pass and quad of plain, transposed and seam patches, at sizes whose offsets exceed 2^32 too.
  * A workgroup takes the fast exit exactly where all 256 pixels of its patch lie inside their frame and that frame exists, for
    every patch of every launch geometry of a list of sizes, in both orientations, on the plain and on the packed decode."""
import ctypes
import itertools

import pytest


@pytest.fixture(scope="module")
def L():
    from fastposecnn_amd import _native
    return _native.lib()


def expected_offsets(tr, H, W, Cout, nb, b, ty0, tx0, ks, t_e):
    """{(tp, rr, cc): element offset} of thread t_e, by the definition: frame, pixel and channel of each quad"""
    otl, oq = t_e >> 4, t_e & 15
    far = (otl & 7) >= ks
    ob = b + 1 if far else b
    otx = (otl & 7) - ks if far else tx0 + (otl & 7)
    n = nb * 64 + oq * 4
    out = {}
    for tp, rr, cc in itertools.product(range(4), range(2), range(2)):
        ot = otl + 16 * tp
        y, x = 2 * (ty0 + (ot >> 3)) + rr, 2 * otx + cc
        pixel = x * H + y if tr else y * W + x
        out[(tp, rr, cc)] = (ob * H * W + pixel) * Cout + n
    return out


# (H, W, Cout, nb, b, ty0, tx0): a small map; the issue's large one (B = 40, 480 x 640, Cout = 512: the last frame's offsets lie
# beyond 2^32 elements); a map whose single frame already does (as arithmetic: nothing is allocated)
SITES = [(24, 32, 64, 0, 1, 0, 0), (24, 32, 128, 1, 2, 8, 8), (480, 640, 512, 7, 39, 232, 312), (480, 640, 512, 3, 38, 8, 160),
         (4096, 4096, 512, 5, 3, 2040, 2040)]


@pytest.mark.parametrize("tr", (0, 1))
@pytest.mark.parametrize("site", SITES, ids=lambda s: "x".join(map(str, s)))
def test_offsets_are_the_definition(L, site, tr):
    H, W, Cout, nb, b, ty0, tx0 = site
    tcw = (W + 1) // 2
    out = (ctypes.c_int64 * 16)()
    big = 0
    # no seam, and a seam after ks tile columns (the patch then starts ks columns in front of the frame's end)
    for ks in (99, 1, 2, 4, 5, 7):
        x0 = tx0 if ks >= 8 else tcw - ks
        for t_e in range(256):
            assert L.fpc_wino_tile_out(tr, H, W, Cout, nb, b, ty0, x0, ks, t_e, out) == 0
            want = expected_offsets(tr, H, W, Cout, nb, b, ty0, x0, ks, t_e)
            for (tp, rr, cc), v in want.items():
                assert int(out[4 * tp + 2 * rr + cc]) == v, (ks, t_e, tp, rr, cc)
                big = max(big, v)
    if H >= 480:
        assert big > 1 << 32


def test_offsets_refuse_nonsense(L):
    out = (ctypes.c_int64 * 16)()
    assert L.fpc_wino_tile_out(0, 24, 32, 64, 0, 0, 0, 0, 99, 256, out) != 0
    assert L.fpc_wino_tile_out(0, 24, 32, 64, 0, 0, 0, 0, 99, 0, None) != 0
    assert L.fpc_wino_tile_out(0, 0, 32, 64, 0, 0, 0, 0, 99, 0, out) != 0


SIZES = (16, 18, 23, 24, 31, 32, 40)
BATCHES = (1, 2, 3, 5)


def brute_fast(H, W, B, G, b, ty0, tx0, ks):
    """all 256 pixels of the patch inside their frame, and that frame there: frames b and, behind a seam, b + 1 of the same canvas row"""
    for j, k, rr, cc in itertools.product(range(8), range(8), range(2), range(2)):
        far = k >= ks
        f = b + 1 if far else b
        y, x = 2 * (ty0 + j) + rr, 2 * ((k - ks) if far else (tx0 + k)) + cc
        if far and (f >= B or f % G == 0):
            return False
        if y >= H or x >= W:
            return False
    return True


@pytest.mark.parametrize("H,W", list(itertools.product(SIZES, SIZES)), ids=lambda v: str(v))
def test_fast_exit_is_the_brute_force_verdict(L, H, W):
    """(H, W) walks all ordered pairs: each pair is also the virtual image of the transposed launch of (W, H)."""
    o8, g8 = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    seen = set()
    for B in BATCHES:
        tcw, tch = (W + 1) // 2, (H + 1) // 2
        # the plain decode (one frame per patch row) and the packed one on wino_pack_geometry's canvas (also with one frame per row)
        assert L.fpc_wino_pack_geometry(H, W, B, 16, 0, g8) == 0
        G, tbx, tby, patches = (int(g8[i]) for i in range(4))
        launches = [(0, 1, -(-tcw // 8), -(-tch // 8), B * (-(-tcw // 8)) * (-(-tch // 8))), (1, G, tbx, tby, patches)]
        if G > 1:
            launches.append((1, 1, -(-tcw // 8), -(-tch // 8), B * (-(-tcw // 8)) * (-(-tch // 8))))
        for packed, g, bx, by, n in launches:
            frames = set()
            for p in range(n):
                assert L.fpc_wino_tile_patch(packed, H, W, B, bx, by, g, p, o8) == 0, (packed, g, p)
                b, ty0, tx0, ks, two, _, _, fast = (int(v) for v in o8)
                want = brute_fast(H, W, B, g, b, ty0, tx0, ks)
                assert bool(fast) == want, (B, packed, g, p, tuple(o8))
                if ks < 8:
                    assert bool(two) == (b + 1 < B and (b + 1) % g != 0), (B, packed, g, p, tuple(o8))
                seen.add((bool(fast), ks < 8))
                frames.add(b)
            assert frames == set(range(B))
    # a map of whole patches has fast patches only, any other both kinds
    if H % 16 == 0 and W % 16 == 0:
        assert all(f for f, _ in seen), seen
    else:
        assert any(not f for f, _ in seen), seen


def test_fast_seam_patches_exist(L):
    """W = 24 at B = 2: twelve tile columns, two frames per canvas row, the middle patch carries a seam after 4 and is fast where its
    rows lie inside (H = 32); at B = 3 the last canvas row is ragged and its seam patch's second frame is missing: general."""
    o8, g8 = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 8)()
    for B, want in ((2, {(4, 1, 1)}), (3, {(4, 1, 1), (4, 0, 0)})):
        assert L.fpc_wino_pack_geometry(32, 24, B, 16, 0, g8) == 0
        G, tbx, tby, patches = (int(g8[i]) for i in range(4))
        assert G == 2
        got = set()
        for p in range(patches):
            assert L.fpc_wino_tile_patch(1, 32, 24, B, tbx, tby, G, p, o8) == 0
            if o8[3] < 8:
                got.add((int(o8[3]), int(o8[4]), int(o8[7])))
        assert got == want
