"""Why one wave of the folded s2.0 may sit out phase 2 (csrc/wino_h3.hip, FOLD; fpc_net_set_fold_idle_row).  The phase reads p3 as
its nearest x2 upsample: the four input rows of a tile are the low-resolution rows [a, b, b, c] (a or c replaced by the zero padding
at the border), and the input transform B^T = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]] makes row 2 of them
b - b: +0 for every finite b, in float32 as in exact arithmetic.  The kernel computes that row as fma(-1, d1, d2), which is the same
subtraction.  The wave that owns row 2 therefore multiplies zeros, its products are +-0, and adding +-0 to an accumulator that
started from +0 changes no bit — such an accumulator is never -0.  Host arithmetic only (numpy float32)."""
import numpy as np
import pytest

F32_MAX = np.float32(np.finfo(np.float32).max)
F32_TINY = np.float32(np.finfo(np.float32).tiny)
DENORM = np.float32(1e-45)           # the smallest denormal
IDX = np.array([0, 1, 1, 2])         # nearest x2 upsample of three low-resolution rows (columns) into a tile's four


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _values(kind, n, rng):
    """n x 3 x 3 low-resolution neighbourhoods"""
    if kind == "random":
        return rng.standard_normal((n, 3, 3)).astype(np.float32) * np.float32(8.0)
    if kind == "zeros":
        return rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=(n, 3, 3))
    if kind == "denormals":
        return (rng.integers(-(1 << 22), 1 << 22, size=(n, 3, 3)).astype(np.float32) * DENORM).astype(np.float32)
    if kind == "largest":
        return rng.choice(np.array([F32_MAX, -F32_MAX], dtype=np.float32), size=(n, 3, 3))
    if kind == "mixed":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, F32_TINY, -F32_TINY, 1.0, -1.5, 65504.0, -1e30, F32_MAX, -F32_MAX], dtype=np.float32)
        return rng.choice(pool, size=(n, 3, 3))
    raise ValueError(kind)


KINDS = ("random", "zeros", "denormals", "largest", "mixed")
PADS = ("none", "first", "last", "both")


def _tiles(kind, pad_rows, pad_cols, n=4096, seed=0):
    """n 4 x 4 tiles of the upsampled image, the border's zero padding written over the first and / or last row and column"""
    rng = np.random.default_rng(seed)
    x = _values(kind, n, rng)
    t = x[:, IDX][:, :, IDX].copy()
    for pad, axis in ((pad_rows, 1), (pad_cols, 2)):
        sl = [slice(None)] * 3
        if pad in ("first", "both"):
            sl[axis] = 0
            t[tuple(sl)] = np.float32(0.0)
        if pad in ("last", "both"):
            sl[axis] = 3
            t[tuple(sl)] = np.float32(0.0)
    assert t.dtype == np.float32 and np.isfinite(t).all()
    return t


def _bt_rows(t):
    """B^T along axis 1, row by row as the kernel's waves compute them (row i of wave i: d_a + sgn d_b)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([t[:, 0] - t[:, 2], t[:, 1] + t[:, 2], t[:, 2] - t[:, 1], t[:, 1] - t[:, 3]], axis=1)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", KINDS)
def test_transform_row_2_is_plus_zero(kind, pad):
    for pad_cols in PADS:
        e = _bt_rows(_tiles(kind, pad, pad_cols))
        assert e.dtype == np.float32
        assert not _bits(e[:, 2]).any(), (kind, pad, pad_cols)
        # and what the column transform makes of a row of +0 is +0 again, in every column
        with np.errstate(over="ignore", invalid="ignore"):
            v = _bt_rows(e.transpose(0, 2, 1)).transpose(0, 2, 1)
        assert not _bits(v[:, 2]).any(), (kind, pad, pad_cols)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("kind", KINDS)
def test_transform_column_2_is_plus_zero(kind, pad):
    """the same along the other axis (what lets every wave skip its xi column 2): on the tile itself for every finite value, and
    behind the row transform wherever that stayed finite (a - b overflows for the largest values of opposite sign)"""
    for pad_rows in PADS:
        t = _tiles(kind, pad_rows, pad)
        c = _bt_rows(t.transpose(0, 2, 1)).transpose(0, 2, 1)
        assert not _bits(c[:, :, 2]).any(), (kind, pad_rows, pad)
        e = _bt_rows(t)
        with np.errstate(over="ignore", invalid="ignore"):
            v = _bt_rows(e.transpose(0, 2, 1)).transpose(0, 2, 1)
        finite = np.isfinite(e).all(axis=2)
        assert not _bits(v[:, :, 2])[finite].any(), (kind, pad_rows, pad)
        assert kind == "largest" or kind == "mixed" or finite.all()


def _products(kind, n, k, rng):
    if kind == "cancelling":      # x, -x, x, -x, ...: the sums pass through zero all the time
        x = rng.standard_normal((n, k // 2)).astype(np.float32)
        return np.stack([x, -x], axis=2).reshape(n, k)
    if kind == "signed-zeros":
        return rng.choice(np.array([0.0, -0.0], dtype=np.float32), size=(n, k))
    if kind == "underflowing":    # products of tiny factors: many round to +-0, the rest are denormals of both signs
        a = (rng.standard_normal((n, k)) * 1e-23).astype(np.float32)
        b = (rng.standard_normal((n, k)) * 1e-23).astype(np.float32)
        with np.errstate(under="ignore"):
            return a * b
    if kind == "random":
        return (rng.standard_normal((n, k)).astype(np.float32) * rng.standard_normal((n, k)).astype(np.float32))
    if kind == "largest":
        return rng.choice(np.array([F32_MAX, -F32_MAX, 0.0, -0.0], dtype=np.float32), size=(n, k)) * np.float32(2.0 ** -8)
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ("cancelling", "signed-zeros", "underflowing", "random", "largest"))
def test_adding_signed_zeros_changes_no_bit_of_an_accumulator_from_plus_zero(kind):
    rng = np.random.default_rng(1)
    n, k = 2048, 64
    p = _products(kind, n, k, rng)
    assert p.dtype == np.float32
    pz, nz = np.float32(0.0), np.float32(-0.0)
    acc = np.zeros(n, dtype=np.float32)      # the kernel clears its accumulators to +0 in front of phase 1
    seen_zero = False
    for i in range(k):
        with np.errstate(under="ignore", over="ignore"):
            acc = acc + p[:, i]
        assert acc.dtype == np.float32
        b = _bits(acc)
        assert not (b == 0x80000000).any(), (kind, i, "an accumulator became -0")
        seen_zero = seen_zero or bool((b == 0).any())
        with np.errstate(under="ignore"):
            for z in (pz, nz):
                assert np.array_equal(_bits(acc + z), b), (kind, i, float(z))
                assert np.array_equal(_bits((acc + z) + z), b), (kind, i, float(z))
    assert kind == "random" or seen_zero      # the zero accumulators, where the sign of a zero could show, did occur
