"""The x-shared tile map of the packed k_conv_wino_h3 launches (csrc/wino_tile.hpp, XS; host only, through fpc_wino_tile_* — the
very functions the kernel calls).  Lane li of a wave holds the tiles 2k and 2k + 1, k = li & 3, of tile row li >> 2 of the 8 x 8
patch (tile half mt = the column's low bit) and reads six region columns of two region rows per K-step.  Held here, for a seam
after pk_ks in {0, 2, 4, 6} tile columns and for none, both `up` values, transposed or not:
  * every fragment read lands on the unit the staging plan fills from exactly the pixel the tile needs (or leaves to the zeroed
    ring where that pixel lies outside the image), at the byte offset of that pixel in the source;
  * no two (region pixel, channel half) share a unit, the staged units are the region's in-image pixels, 18 pieces = at most five
    per wave, four buffers fit the output transform image;
  * the sixteen lanes of every ds_read_b128 lane group (MI355X: lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and their upper-half
    twins) fall on sixteen different 16-byte slots of the 256-byte bank row, for all twelve reads of all four waves — and the same
    for the output stage's reads of the Z image, whose every read finds the run the accumulator's writer put there;
  * the launcher's rule takes the map exactly where the frame's tile-column count is even."""
import ctypes
import itertools

import pytest

GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS += [[l + 32 for l in g] for g in GROUPS[:2]]
ROWS = {0: (0, 2), 1: (1, 2), 2: (2, 1), 3: (1, 3)}      # region rows (ra, rb) of transform row wi: B^T's d0-d2, d1+d2, d2-d1, d1-d3
SEAMS = (0, 2, 4, 6, 99)
H, W, CS = 48, 24, 16      # the (virtual) image of the staging checks: 12 tile columns, patches from tile row 8
TY0 = 8


@pytest.fixture(scope="module")
def L():
    from fastposecnn_amd import _native
    return _native.lib()


def frag(L, xs, wi, lane, ks):
    out = (ctypes.c_int64 * 17)()
    assert L.fpc_wino_tile_frag(xs, wi, lane, ks, out) == 0
    n = int(out[0])
    return [(int(out[1 + 2 * x]), int(out[2 + 2 * x])) for x in range(n)]


def slot(L, xs, tr, s, ks, up, two=1):
    tx0 = 0 if ks >= 8 else W // 2 - ks
    out = (ctypes.c_int64 * 6)()
    assert L.fpc_wino_tile_slot(xs, tr, s, 2 * TY0 - 1, 2 * tx0 - 1, H, W, CS, up, ks, two, out) == 0
    return tuple(int(v) for v in out)


def source(ry, rx, hf, ks, up, tr, two=1):
    """(in the image, byte offset) of region pixel (ry, rx), channel half hf: the staging rule of a packed patch, written out"""
    tx0 = 0 if ks >= 8 else W // 2 - ks
    far = ks < 8 and (rx >> 1) > ks
    y = 2 * TY0 - 1 + ry
    x = rx - 2 * ks - 3 if far else 2 * tx0 - 1 + rx
    if not (0 <= y < H and 0 <= x < W and (not far or two)):
        return False, 0
    Hs, Ws = H >> up, W >> up
    px = (x >> up) * Hs + (y >> up) if tr else (y >> up) * Ws + (x >> up)
    return True, (px * CS + 4 * hf) * 4 + (Hs * Ws * CS * 4 if far else 0)


@pytest.mark.parametrize("ks,up,tr", list(itertools.product(SEAMS, (0, 1), (0, 1))))
def test_fragment_map_and_staging_plan_are_inverse(L, ks, up, tr):
    plan = [slot(L, 1, tr, s, ks, up) for s in range(5 * 4 * 64)]
    staged = {}
    for s, (ry, rx, hf, far, ok, off) in enumerate(plan):
        if ok:
            assert s < 18 * 64, "a nineteenth piece: a wave would stage more than five"
            assert (ry, rx, hf) not in staged, "two units for one (region pixel, channel half)"
            staged[(ry, rx, hf)] = s
            assert (True, off) == source(ry, rx, hf, ks, up, tr), (s, ry, rx, hf)
    # what is staged is exactly the region's pixels inside the image (a seam region is one column pair wider; the seam after 0
    # columns has no tile in front of it and stages nothing there)
    cols = range(20 if ks < 8 else 18)
    want = {(ry, rx, hf) for ry in range(18) for rx in cols for hf in (0, 1)
            if source(ry, rx, hf, ks, up, tr)[0] and not (ks == 0 and rx < 2)}
    assert set(staged) == want
    assert (18 + 3) // 4 <= 5
    seen = 0
    for wi, lane in itertools.product(range(4), range(64)):
        li, lh = lane & 31, lane >> 5
        trow, k = li >> 2, li & 3
        col0 = 2 * (2 * k + (1 if 2 * k >= ks else 0))
        reads = frag(L, 1, wi, lane, ks)
        assert len(reads) == 6
        for x, offs in enumerate(reads):
            for r, off in zip(ROWS[wi], offs):
                assert off % 16 == 0 and 0 <= off < 18 * 1024
                ry, rx = 2 * trow + r, col0 + x
                u = plan[off // 16]
                assert u[:3] == (ry, rx, lh), (wi, lane, x, r, u)
                inside, src = source(ry, rx, lh, ks, up, tr)
                assert bool(u[4]) == inside and (not inside or u[5] == src)      # outside: the zeroed ring's unit, never staged
                seen += 1
    assert seen == 4 * 64 * 12


@pytest.mark.parametrize("ks", SEAMS)
def test_a_missing_second_frame_stages_nothing_behind_the_seam(L, ks):
    for s in range(18 * 64):
        ry, rx, hf, far, ok, off = slot(L, 1, 0, s, ks, 0, two=0)
        both = slot(L, 1, 0, s, ks, 0, two=1)
        assert bool(ok) == (bool(both[4]) and not (far and ks < 8))
        assert not ok or (off == both[5] and (True, off) == source(ry, rx, hf, ks, 0, 0, two=0))


@pytest.mark.parametrize("ks", SEAMS)
def test_fragment_reads_are_bank_conflict_free(L, ks):
    for wi in range(4):
        reads = [frag(L, 1, wi, lane, ks) for lane in range(64)]
        for x, row in itertools.product(range(6), range(2)):
            for g in GROUPS:
                slots = {(reads[lane][x][row] % 256) // 16 for lane in g}
                assert len(slots) == 16, (ks, wi, x, row, g, sorted(slots))
    # column pair 1 lies one cell behind column pair 0 for every lane: the kernel reaches it by an immediate
    for wi, lane in itertools.product(range(4), range(64)):
        r = frag(L, 1, wi, lane, ks)
        assert all(r[2][j] - r[0][j] == 8 * 16 * 16 and r[1][j] - r[0][j] == 2 * 16 * 16 and r[3][j] - r[2][j] == 2 * 16 * 16
                   and r[5][j] - r[4][j] == 2 * 16 * 16 for j in (0, 1))


def test_two_lanes_halves_share_their_middle_columns(L):
    """tile 2k + 1's columns 0-1 are tile 2k's columns 2-3: one read serves both (the point of the map)"""
    for ks in SEAMS:
        for wi, lane in itertools.product(range(4), range(32)):
            if (lane & 3) < 3 and not (2 * (lane & 3) < ks <= 2 * (lane & 3) + 2):      # the next lane's pair, no seam between
                a, b = frag(L, 1, wi, lane, ks), frag(L, 1, wi, lane + 1, ks)
                assert a[4] == b[0] and a[5] == b[1]


@pytest.mark.parametrize("xs", (0, 1))
def test_output_stage_finds_every_run_and_reads_conflict_free(L, xs):
    where = {}      # (transform row, cc, tile, channel) -> byte address in the Z image
    used = set()
    for wi, mt, r, nt, cc in itertools.product(range(4), range(2), range(16), range(2), range(2)):
        out = (ctypes.c_int64 * 3)()
        assert L.fpc_wino_tile_zrun(xs, wi, mt, r, nt, cc, out) == 0
        base = int(out[0])
        assert base % 128 == 0 and base + 256 <= 128 * 1024 + 128
        assert not (used & set(range(base, base + 256, 4)))
        used |= set(range(base, base + 256, 4))
        for hb in (0, 1):
            for c in range(32):
                where[(wi, cc, int(out[1 + hb]), 32 * nt + c)] = base + 4 * (32 * hb + c)
    assert len(where) == 4 * 2 * 64 * 64 and len(used) * 4 == 128 * 1024
    if xs:      # the map itself: half mt, register r, lane half hb hold tile row 2 (r >> 2) + hb, column 2 (r & 3) + mt
        out = (ctypes.c_int64 * 3)()
        for mt, r in itertools.product(range(2), range(16)):
            L.fpc_wino_tile_zrun(1, 0, mt, r, 0, 0, out)
            assert [int(out[1]), int(out[2])] == [8 * (2 * (r >> 2) + hb) + 2 * (r & 3) + mt for hb in (0, 1)]
    assert 4 * 18 * 1024 <= max(used) + 4      # four input buffers fit the image's space
    out = (ctypes.c_int64 * 1)()
    for tp, cc, i in itertools.product(range(4), range(2), range(4)):
        addr = []
        for t_e in range(256):
            assert L.fpc_wino_tile_zread(xs, t_e, tp, cc, i, out) == 0
            a = int(out[0])
            tile, ch = (t_e >> 4) + 16 * tp, 4 * (t_e & 15)
            assert [where[(i, cc, tile, ch + j)] for j in range(4)] == [a, a + 4, a + 8, a + 12], (t_e, tp, cc, i)
            addr.append(a)
        for w in range(4):
            for g in GROUPS:
                assert len({(addr[64 * w + lane] % 256) // 16 for lane in g}) == 16, (tp, cc, i, w)


def test_rule_takes_the_map_exactly_for_even_tile_column_counts(L):
    for w in range(1, 201):
        assert L.fpc_wino_xshare_rule(w) == (1 if ((w + 1) // 2) % 2 == 0 else 0), w
    assert L.fpc_wino_xshare_rule(0) == 0
    # every packed headline site: virtual widths 120 and 60 (transposed), 40 and 20
    assert all(L.fpc_wino_xshare_rule(w) == 1 for w in (120, 60, 40, 20))
